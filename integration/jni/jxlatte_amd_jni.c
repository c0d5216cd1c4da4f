/*
 * JNI glue between com.traneptora.jxlatte.gpu.NativeBackend and include/jxlatte_amd.h (row f4).
 *
 * NOT COMPILED OR TESTED HERE: this image has no JDK / jni.h. Build on a machine that has one:
 *   cc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include jxlatte_amd_jni.c \
 *      -L../../jxlatte_amd -ljxlatte_amd -o libjxlatte_amd_jni.so
 * Status codes are rethrown as the exceptions the reference throws at the same places.
 */
#include <jni.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "jxlatte_amd.h"

static jxl_ctx* ctx_of(JNIEnv* e, jobject self) {
    jclass cls = (*e)->GetObjectClass(e, self);
    jfieldID f = (*e)->GetFieldID(e, cls, "ctx", "J");
    return (jxl_ctx*)(intptr_t)(*e)->GetLongField(e, self, f);
}

static void rethrow(JNIEnv* e, jxl_ctx* c, jxl_status st) {
    const char* cls = st == JXL_ERR_INVALID_BITSTREAM ? "com/traneptora/jxlatte/io/InvalidBitstreamException"
                    : st == JXL_ERR_UNSUPPORTED       ? "java/lang/UnsupportedOperationException"
                    : st == JXL_ERR_INVALID_ARGUMENT  ? "java/lang/IllegalArgumentException"
                    : st == JXL_ERR_STATE             ? "java/lang/IllegalStateException"
                    : st == JXL_ERR_OOM               ? "java/lang/OutOfMemoryError"
                                                      : "java/lang/RuntimeException";
    (*e)->ThrowNew(e, (*e)->FindClass(e, cls), c ? jxl_last_error(c) : "jxlatte_amd: no context");
}
#define CHECK(call)                         \
    do {                                    \
        jxl_status st_ = (call);            \
        if (st_ != JXL_OK) {                \
            rethrow(e, c, st_);             \
            return;                         \
        }                                   \
    } while (0)
#define ADDR(buf) ((buf) ? (*e)->GetDirectBufferAddress(e, (buf)) : NULL)

/* Argument checks (r4): the library trusts the sizes its C callers state; a Java caller states them twice -- as integers and as
 * the capacity of the direct buffers it passes -- and the shim makes the two agree before anything is read or written. */
static void bad_arg(JNIEnv* e, const char* what) {
    if (!(*e)->ExceptionCheck(e)) (*e)->ThrowNew(e, (*e)->FindClass(e, "java/lang/IllegalArgumentException"), what);
}
/* a direct buffer of at least `bytes` bytes */
static int has_room(JNIEnv* e, jobject buf, jlong bytes) {
    return buf && bytes >= 0 && (*e)->GetDirectBufferAddress(e, buf) && (*e)->GetDirectBufferCapacity(e, buf) >= bytes;
}
#define NEED(buf, bytes)                                                        \
    do {                                                                        \
        if (!has_room(e, (buf), (jlong)(bytes))) {                              \
            bad_arg(e, "jxlatte_amd: direct buffer " #buf " missing or too small"); \
            return;                                                             \
        }                                                                       \
    } while (0)
/* an optional buffer: null, or large enough */
#define NEED_OPT(buf, bytes)          \
    do {                              \
        if (buf) NEED(buf, bytes);    \
    } while (0)
static jlong area(jlong h, jlong w) { return h < 0 || w < 0 ? -1 : h * w; }
/* n floats / ints of a Java array into dst; 0 (exception pending) if the array is null or shorter */
static int get_floats(JNIEnv* e, jfloatArray a, jsize n, float* dst) {
    if (!a || (*e)->GetArrayLength(e, a) < n) {
        bad_arg(e, "jxlatte_amd: float array missing or too short");
        return 0;
    }
    (*e)->GetFloatArrayRegion(e, a, 0, n, dst);
    return !(*e)->ExceptionCheck(e);
}
static int get_ints(JNIEnv* e, jintArray a, jsize n, jint* dst) {
    if (!a || (*e)->GetArrayLength(e, a) < n) {
        bad_arg(e, "jxlatte_amd: int array missing or too short");
        return 0;
    }
    (*e)->GetIntArrayRegion(e, a, 0, n, dst);
    return !(*e)->ExceptionCheck(e);
}
#define GETF(arr, n, dst)                              \
    do {                                               \
        if (!get_floats(e, (arr), (n), (dst))) return; \
    } while (0)
#define GETI(arr, n, dst)                            \
    do {                                             \
        if (!get_ints(e, (arr), (n), (dst))) return; \
    } while (0)

JNIEXPORT jlong JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_create(JNIEnv* e, jclass k, jint device) {
    (void)k;
    jxl_ctx* c = NULL;
    jxl_status st = jxl_ctx_create(device, &c);
    if (st != JXL_OK) {
        rethrow(e, c, st);
        return 0;
    }
    return (jlong)(intptr_t)c;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_destroy(JNIEnv* e, jclass k, jlong ctx) {
    (void)e; (void)k;
    jxl_ctx_destroy((jxl_ctx*)(intptr_t)ctx);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_beginFrame(JNIEnv* e, jobject self, jobject params) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_vardct_params p;
    /* (a heap ByteBuffer has no direct address: GetDirectBufferAddress returns NULL for it) */
    const void* src = params ? (*e)->GetDirectBufferAddress(e, params) : NULL;
    if (!src || (*e)->GetDirectBufferCapacity(e, params) < (jlong)sizeof p) {
        bad_arg(e, "jxlatte_amd: beginFrame needs a direct buffer holding jxl_vardct_params");
        return;
    }
    memcpy(&p, src, sizeof p);
    CHECK(jxl_vardct_begin_frame(c, &p));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_setWeights(JNIEnv* e, jobject self, jobject weights, jintArray offs) {
    jxl_ctx* c = ctx_of(e, self);
    jint o[51];
    GETI(offs, 51, o);
    NEED(weights, 4);
    CHECK(jxl_vardct_set_weights(c, (const float*)ADDR(weights), (size_t)(*e)->GetDirectBufferCapacity(e, weights) / 4, (const int32_t*)o));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_setLFGroup(JNIEnv* e, jobject self, jint lfgY, jint lfgX, jint cellsH,
        jint cellsW, jobject dctSelect, jobject hfMul, jobject sharpness, jobject xFromY, jobject bFromY, jobject blockYX, jint nBlocks,
        jobject lfX, jobject lfY, jobject lfB) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_lfgroup_desc d;
    int32_t geo[13];
    CHECK(jxl_vardct_geometry(c, geo));
    if (cellsH <= 0 || cellsW <= 0 || cellsH > 256 || cellsW > 256 || nBlocks < 0) {
        bad_arg(e, "jxlatte_amd: LF group size out of range");
        return;
    }
    {   /* every grid the library will read, sized from the stated cell counts and the frame's own subsampling shifts */
        const jlong cells = area(cellsH, cellsW), tiles = area((cellsH + 7) / 8, (cellsW + 7) / 8);
        NEED(dctSelect, cells);
        NEED(hfMul, 4 * cells);
        NEED(sharpness, 4 * cells);
        NEED(xFromY, 4 * tiles);
        NEED(bFromY, 4 * tiles);
        NEED(blockYX, 8 * (jlong)nBlocks);
        NEED_OPT(lfX, 4 * area(cellsH >> geo[7], cellsW >> geo[6]));
        NEED_OPT(lfY, 4 * area(cellsH >> geo[9], cellsW >> geo[8]));
        NEED_OPT(lfB, 4 * area(cellsH >> geo[11], cellsW >> geo[10]));
    }
    memset(&d, 0, sizeof d);
    d.lfg_y = lfgY; d.lfg_x = lfgX; d.cells_h = cellsH; d.cells_w = cellsW;
    d.dct_select = (const uint8_t*)ADDR(dctSelect);
    d.hf_mul = (const int32_t*)ADDR(hfMul);
    d.sharpness = (const int32_t*)ADDR(sharpness);
    d.x_from_y = (const int32_t*)ADDR(xFromY);
    d.b_from_y = (const int32_t*)ADDR(bFromY);
    d.block_yx = (const int32_t*)ADDR(blockYX);
    d.n_blocks = nBlocks;
    d.lf[0] = (const float*)ADDR(lfX); d.lf[1] = (const float*)ADDR(lfY); d.lf[2] = (const float*)ADDR(lfB);
    CHECK(jxl_vardct_set_lfgroup(c, &d));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_setLFGroupQuant(JNIEnv* e, jobject self, jint lfgY, jint lfgX,
        jint cellsH, jint cellsW, jobject qX, jobject qY, jobject qB, jint extraPrecision, jfloatArray scaledDequant, jint xFactorLF,
        jint bFactorLF, jboolean adaptiveSmoothing) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_lfquant_desc d;
    int32_t geo[13];
    CHECK(jxl_vardct_geometry(c, geo));
    if (cellsH <= 0 || cellsW <= 0 || cellsH > 256 || cellsW > 256) {
        bad_arg(e, "jxlatte_amd: LF group size out of range");
        return;
    }
    NEED(qX, 4 * area(cellsH >> geo[7], cellsW >> geo[6]));
    NEED(qY, 4 * area(cellsH >> geo[9], cellsW >> geo[8]));
    NEED(qB, 4 * area(cellsH >> geo[11], cellsW >> geo[10]));
    memset(&d, 0, sizeof d);
    d.lfg_y = lfgY; d.lfg_x = lfgX; d.cells_h = cellsH; d.cells_w = cellsW;
    d.lf_quant[0] = (const int32_t*)ADDR(qX); d.lf_quant[1] = (const int32_t*)ADDR(qY); d.lf_quant[2] = (const int32_t*)ADDR(qB);
    d.extra_precision = extraPrecision;
    GETF(scaledDequant, 3, d.scaled_dequant);
    d.x_factor_lf = xFactorLF; d.b_factor_lf = bFactorLF; d.adaptive_smoothing = adaptiveSmoothing ? 1 : 0;
    CHECK(jxl_vardct_set_lfgroup_lfquant(c, &d));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_putGroup(JNIEnv* e, jobject self, jint pass, jint group, jobject qx,
        jobject qy, jobject qb, jint sx, jint sy, jint sb) {
    jxl_ctx* c = ctx_of(e, self);
    const int32_t s[3] = {sx, sy, sb};
    int32_t gw[3], gh[3];
    CHECK(jxl_vardct_group_size(c, group, gw, gh));
    {   /* rows of gw samples at the caller's stride: (gh - 1) * stride + gw samples are read from each buffer */
        jobject b[3] = {qx, qy, qb};
        for (int ch = 0; ch < 3; ch++) {
            if (s[ch] < gw[ch]) {
                bad_arg(e, "jxlatte_amd: putGroup stride shorter than the group's rows");
                return;
            }
            if (!has_room(e, b[ch], (jlong)sizeof(int32_t) * (gh[ch] > 0 ? (jlong)(gh[ch] - 1) * s[ch] + gw[ch] : 0))) {
                bad_arg(e, "jxlatte_amd: putGroup coefficient buffer missing or too small for the group");
                return;
            }
        }
    }
    const int32_t* q[3] = {(const int32_t*)ADDR(qx), (const int32_t*)ADDR(qy), (const int32_t*)ADDR(qb)};
    CHECK(jxl_vardct_put_group(c, pass, group, q, s));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_putGroupI16(JNIEnv* e, jobject self, jint pass, jint group, jobject qx,
        jobject qy, jobject qb, jint sx, jint sy, jint sb) {
    jxl_ctx* c = ctx_of(e, self);
    const int32_t s[3] = {sx, sy, sb};
    int32_t gw[3], gh[3];
    CHECK(jxl_vardct_group_size(c, group, gw, gh));
    {   /* rows of gw samples at the caller's stride: (gh - 1) * stride + gw samples are read from each buffer */
        jobject b[3] = {qx, qy, qb};
        for (int ch = 0; ch < 3; ch++) {
            if (s[ch] < gw[ch]) {
                bad_arg(e, "jxlatte_amd: putGroupI16 stride shorter than the group's rows");
                return;
            }
            if (!has_room(e, b[ch], (jlong)sizeof(int16_t) * (gh[ch] > 0 ? (jlong)(gh[ch] - 1) * s[ch] + gw[ch] : 0))) {
                bad_arg(e, "jxlatte_amd: putGroupI16 coefficient buffer missing or too small for the group");
                return;
            }
        }
    }
    const int16_t* q[3] = {(const int16_t*)ADDR(qx), (const int16_t*)ADDR(qy), (const int16_t*)ADDR(qb)};
    CHECK(jxl_vardct_put_group_i16(c, pass, group, q, s));
}

/* planes of the current frame: (H >> sy) rows of (W >> sx) samples each; the sizes come from the library
 * (jxl_vardct_coeff_plane_rows), never from the caller */
JNIEXPORT jobjectArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_mapCoeffsI16(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    int16_t* pl[3];
    int32_t st[3], rows[3];
    jxl_status r = jxl_vardct_map_coeffs_i16(c, pl, st);
    if (r == JXL_OK) r = jxl_vardct_coeff_plane_rows(c, rows);
    if (r) { rethrow(e, c, r); return NULL; }
    jclass bb = (*e)->FindClass(e, "java/nio/ByteBuffer");
    if (!bb) return NULL;  /* exception pending */
    jobjectArray out = (*e)->NewObjectArray(e, 3, bb, NULL);
    if (!out) return NULL;
    for (int i = 0; i < 3; i++) {
        jobject b = (*e)->NewDirectByteBuffer(e, pl[i], (jlong)st[i] * rows[i] * 2);
        if (!b || (*e)->ExceptionCheck(e)) return NULL;
        (*e)->SetObjectArrayElement(e, out, i, b);
    }
    return out;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_commitCoeffsI16(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_vardct_commit_coeffs_i16(c));
}

/* the same planes without the zero-fill (JXL_MAP_NO_FILL): the decoder writes every sample of the groups it then names */
JNIEXPORT jobjectArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_mapCoeffsI16NoFill(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    int16_t* pl[3];
    int32_t st[3], rows[3];
    jxl_status r = jxl_vardct_map_coeffs_i16_ex(c, pl, st, JXL_MAP_NO_FILL);
    if (r == JXL_OK) r = jxl_vardct_coeff_plane_rows(c, rows);
    if (r) { rethrow(e, c, r); return NULL; }
    jclass bb = (*e)->FindClass(e, "java/nio/ByteBuffer");
    if (!bb) return NULL;  /* exception pending */
    jobjectArray out = (*e)->NewObjectArray(e, 3, bb, NULL);
    if (!out) return NULL;
    for (int i = 0; i < 3; i++) {
        jobject b = (*e)->NewDirectByteBuffer(e, pl[i], (jlong)st[i] * rows[i] * 2);
        if (!b || (*e)->ExceptionCheck(e)) return NULL;
        (*e)->SetObjectArrayElement(e, out, i, b);
    }
    return out;
}

/* written: one byte per group of the frame (non-zero = its rectangle was fully written); the length is checked by the library */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_commitCoeffsI16Groups(JNIEnv* e, jobject self, jbyteArray written) {
    jxl_ctx* c = ctx_of(e, self);
    if (!written) { rethrow(e, c, JXL_ERR_INVALID_ARGUMENT); return; }
    const jsize n = (*e)->GetArrayLength(e, written);
    jbyte* w = (*e)->GetByteArrayElements(e, written, NULL);
    if (!w) return;  /* OutOfMemoryError pending */
    const jxl_status r = jxl_vardct_commit_coeffs_i16_groups(c, (const uint8_t*)w, (int32_t)n);
    (*e)->ReleaseByteArrayElements(e, written, w, JNI_ABORT);
    if (r) rethrow(e, c, r);
}

/* ---- sparse coefficient feed: lists of (position, value) entries, the form HFCoefficients' decode loop produces (HFCoefficients.java:112-127) ---- */
/* n entries of 4 (narrow) or 8 (wide) bytes in each direct buffer; a channel without entries may pass null. The group index is checked
 * against the open frame (jxl_vardct_group_size) before any buffer is looked at; positions are checked by the library. */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_putGroupSparse(JNIEnv* e, jobject self, jint pass, jint group, jobject ex,
        jobject ey, jobject eb, jint nx, jint ny, jint nb, jboolean wide) {
    jxl_ctx* c = ctx_of(e, self);
    const int32_t n[3] = {nx, ny, nb};
    int32_t gw[3], gh[3];
    CHECK(jxl_vardct_group_size(c, group, gw, gh));
    {
        jobject b[3] = {ex, ey, eb};
        for (int ch = 0; ch < 3; ch++) {
            if (n[ch] < 0) {
                bad_arg(e, "jxlatte_amd: putGroupSparse negative entry count");
                return;
            }
            if (n[ch] > 0 && !has_room(e, b[ch], (jlong)n[ch] * (wide ? 8 : 4))) {
                bad_arg(e, "jxlatte_amd: putGroupSparse entry buffer missing or too small for its count");
                return;
            }
        }
    }
    const uint32_t* q[3] = {nx ? (const uint32_t*)ADDR(ex) : NULL, ny ? (const uint32_t*)ADDR(ey) : NULL, nb ? (const uint32_t*)ADDR(eb) : NULL};
    CHECK(jxl_vardct_put_group_sparse(c, pass, group, q, n, wide ? JXL_SPARSE_WIDE : 0));
}

/* the library's page-locked entry buffer of capacityWords 32-bit words, as ONE direct buffer of exactly that size */
JNIEXPORT jobject JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_mapSparse(JNIEnv* e, jobject self, jlong capacityWords) {
    jxl_ctx* c = ctx_of(e, self);
    uint32_t* words = NULL;
    if (capacityWords <= 0) {
        bad_arg(e, "jxlatte_amd: mapSparse capacity must be positive");
        return NULL;
    }
    jxl_status r = jxl_vardct_map_sparse(c, (size_t)capacityWords, &words);
    if (r) { rethrow(e, c, r); return NULL; }
    return (*e)->NewDirectByteBuffer(e, words, capacityWords * 4);
}

/* runs: five ints per run {group, channel, flags, count, offsetWords}; every run is checked by the library against the frame
 * and the mapped capacity before anything is queued */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_commitSparse(JNIEnv* e, jobject self, jintArray runs) {
    jxl_ctx* c = ctx_of(e, self);
    if (!runs) { rethrow(e, c, JXL_ERR_INVALID_ARGUMENT); return; }
    const jsize len = (*e)->GetArrayLength(e, runs);
    if (len % 5) {
        bad_arg(e, "jxlatte_amd: commitSparse takes five ints per run");
        return;
    }
    const jsize n = len / 5;
    jint* v = (jint*)malloc(sizeof(jint) * (size_t)(len ? len : 1));
    jxl_sparse_run* r = (jxl_sparse_run*)malloc(sizeof(jxl_sparse_run) * (size_t)(n ? n : 1));
    if (!v || !r) {
        free(v); free(r);
        rethrow(e, c, JXL_ERR_OOM);
        return;
    }
    (*e)->GetIntArrayRegion(e, runs, 0, len, v);
    jxl_status st = JXL_OK;
    if (!(*e)->ExceptionCheck(e)) {
        for (jsize i = 0; i < n; i++) {
            r[i].group = v[5 * i]; r[i].channel = v[5 * i + 1]; r[i].flags = v[5 * i + 2]; r[i].count = v[5 * i + 3];
            r[i].offset_words = v[5 * i + 4];
        }
        st = jxl_vardct_commit_sparse(c, r, (int32_t)n);
    }
    free(v); free(r);
    if (st) rethrow(e, c, st);
}

JNIEXPORT jlong JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_sparseRejected(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    int64_t n = 0;
    jxl_status r = jxl_vardct_sparse_rejected(c, &n);
    if (r) { rethrow(e, c, r); return 0; }
    return (jlong)n;
}

JNIEXPORT jobject JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_hostAlloc(JNIEnv* e, jclass k, jlong bytes) {
    (void)k;
    void* p = jxl_host_alloc((size_t)bytes);
    return p ? (*e)->NewDirectByteBuffer(e, p, bytes) : NULL;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_hostFree(JNIEnv* e, jclass k, jobject b) {
    (void)k;
    if (b) jxl_host_free((*e)->GetDirectBufferAddress(e, b));
}

/* The output buffers of readOutput / readOutputBegin / finishFrame against the library's own numbers (jxl_vardct_output_geometry, r6):
 * og[1] rows of og[0] pixels -- the full padded frame, also for chroma-subsampled frames --, og[2] bytes per sample, times 3 when the
 * format interleaves the colours into ox (RGB8 / RGB16: oy and ob may then be null), `stride` pixels apart (>= og[0]).
 * 0: an exception is pending. */
static int out_room(JNIEnv* e, jxl_ctx* c, jobject ox, jobject oy, jobject ob, jlong stride) {
    int32_t og[5];
    jxl_status st_ = jxl_vardct_output_geometry(c, og);
    if (st_ != JXL_OK) {
        rethrow(e, c, st_);
        return 0;
    }
    if (stride < og[0]) { /* the library's own rule (enqueue_output): a row stride is at least a row */
        bad_arg(e, "jxlatte_amd: output stride shorter than a row");
        return 0;
    }
    const jlong need = (jlong)og[2] * (og[3] ? 3 : 1) * ((jlong)(og[1] - 1) * stride + og[0]);
    if (!has_room(e, ox, need) || (og[4] == 3 && (!has_room(e, oy, need) || !has_room(e, ob, need)))) {
        bad_arg(e, "jxlatte_amd: output buffer missing or too small");
        return 0;
    }
    return 1;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_finishFrame(JNIEnv* e, jobject self, jobject ox, jobject oy, jobject ob,
        jlong stride) {
    jxl_ctx* c = ctx_of(e, self);
    if (!out_room(e, c, ox, oy, ob, stride)) return;
    void* out[3] = {ADDR(ox), ADDR(oy), ADDR(ob)};
    CHECK(jxl_vardct_finish_frame(c, out, stride));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_run(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_vardct_run(c));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_readOutput(JNIEnv* e, jobject self, jobject ox, jobject oy, jobject ob,
        jlong stride) {
    jxl_ctx* c = ctx_of(e, self);
    if (!out_room(e, c, ox, oy, ob, stride)) return;
    void* out[3] = {ADDR(ox), ADDR(oy), ADDR(ob)};
    CHECK(jxl_vardct_read_output(c, out, stride));
}

/* readOutput in two halves: the host drives the next frame of this context between them (direct buffers from hostAlloc) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_readOutputBegin(JNIEnv* e, jobject self, jobject ox, jobject oy, jobject ob,
        jlong stride) {
    jxl_ctx* c = ctx_of(e, self);
    if (!out_room(e, c, ox, oy, ob, stride)) return;
    void* out[3] = {ADDR(ox), ADDR(oy), ADDR(ob)};
    CHECK(jxl_vardct_read_output_begin(c, out, stride));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_readOutputWait(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_vardct_read_output_wait(c));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_prepare(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_vardct_prepare(c));
}

/* ---- resident colour planes (include/jxlatte_amd.h: jxl_planes_*) ---- */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesFromFrame(JNIEnv* e, jobject self, jint h, jint w) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_planes_from_frame(c, h, w));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesFromFrameAt(JNIEnv* e, jobject self, jint y0, jint x0, jint h, jint w) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_planes_from_frame_at(c, y0, x0, h, w));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesUpload(JNIEnv* e, jobject self, jobject p0, jobject p1, jobject p2,
        jint h, jint w) {
    jxl_ctx* c = ctx_of(e, self);
    const float* in[3] = {(const float*)ADDR(p0), (const float*)ADDR(p1), (const float*)ADDR(p2)};
    CHECK(jxl_planes_upload(c, in, h, w));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesUpsample(JNIEnv* e, jobject self, jint k, jfloatArray weights) {
    jxl_ctx* c = ctx_of(e, self);
    jfloat* w = (*e)->GetFloatArrayElements(e, weights, NULL);  /* k*k*25 floats: jxl_upsampling_weights */
    const jxl_status st = jxl_planes_upsample(c, k, w);
    (*e)->ReleaseFloatArrayElements(e, weights, w, JNI_ABORT);
    CHECK(st);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesNoise(JNIEnv* e, jobject self, jint groupDim, jlong seed0,
        jfloatArray lut, jfloat bcx, jfloat bcb) {
    jxl_ctx* c = ctx_of(e, self);
    float l[8];
    (*e)->GetFloatArrayRegion(e, lut, 0, 8, l);
    CHECK(jxl_planes_noise(c, groupDim, (uint64_t)seed0, l, bcx, bcb));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesNoiseAt(JNIEnv* e, jobject self, jint groupDim, jlong seed0,
        jfloatArray lut, jfloat bcx, jfloat bcb, jint frameH, jint frameW, jint y0, jint x0) {
    jxl_ctx* c = ctx_of(e, self);
    float l[8];
    GETF(lut, 8, l);
    CHECK(jxl_planes_noise_at(c, groupDim, (uint64_t)seed0, l, bcx, bcb, frameH, frameW, y0, x0));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesXYB(JNIEnv* e, jobject self, jfloatArray matrix, jfloatArray bias,
        jfloatArray cbrtBias, jfloat intensityTarget) {
    jxl_ctx* c = ctx_of(e, self);
    float m[9], b[3], cb[3];
    (*e)->GetFloatArrayRegion(e, matrix, 0, 9, m);
    (*e)->GetFloatArrayRegion(e, bias, 0, 3, b);
    (*e)->GetFloatArrayRegion(e, cbrtBias, 0, 3, cb);
    CHECK(jxl_planes_xyb(c, m, b, cb, intensityTarget));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesYCbCr(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_planes_ycbcr(c));
}

JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesShape(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t hw[2] = {0, 0};
    jintArray out = (*e)->NewIntArray(e, 2);
    if (jxl_planes_shape(c, &hw[0], &hw[1]) == JXL_OK && out) (*e)->SetIntArrayRegion(e, out, 0, 2, (const jint*)hw);
    return out;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesDownload(JNIEnv* e, jobject self, jobject p0, jobject p1, jobject p2) {
    jxl_ctx* c = ctx_of(e, self);
    float* out[3] = {(float*)ADDR(p0), (float*)ADDR(p1), (float*)ADDR(p2)};
    CHECK(jxl_planes_download(c, out));
}

/* ---- splines (include/jxlatte_amd.h: jxl_spline_arcs, jxl_stage_splines, jxl_planes_splines) ----
 * A frame's splines arrive as SplinesBundle holds them (SplinesBundle.java:22-73), flattened: nControl[s] control points per
 * spline, control = all (y, x) pairs back to back, coeff = per spline coeffX, coeffY, coeffB, coeffSigma (4 x 32). The three
 * arrays are copied and checked against each other before the library sees them; *mem is the copy (free it), NULL with an
 * exception pending on failure. */
static jint* spline_desc(JNIEnv* e, jint quantAdjust, jintArray nControl, jintArray control, jintArray coeff, jfloat bcx, jfloat bcb,
                         jxl_spline_desc* d) {
    if (!nControl || !control || !coeff) {
        bad_arg(e, "jxlatte_amd: spline arrays missing");
        return NULL;
    }
    const jsize n = (*e)->GetArrayLength(e, nControl), nc = (*e)->GetArrayLength(e, control), nf = (*e)->GetArrayLength(e, coeff);
    if ((jlong)nf < (jlong)n * 128) {
        bad_arg(e, "jxlatte_amd: spline coefficient array too short");
        return NULL;
    }
    jint* mem = (jint*)malloc(sizeof(jint) * ((size_t)n + (size_t)nc + (size_t)nf + 1));
    if (!mem) {
        (*e)->ThrowNew(e, (*e)->FindClass(e, "java/lang/OutOfMemoryError"), "jxlatte_amd: spline arrays");
        return NULL;
    }
    (*e)->GetIntArrayRegion(e, nControl, 0, n, mem);
    (*e)->GetIntArrayRegion(e, control, 0, nc, mem + n);
    (*e)->GetIntArrayRegion(e, coeff, 0, nf, mem + n + nc);
    if ((*e)->ExceptionCheck(e)) { /* an ArrayIndexOutOfBoundsException of a region copy is pending: throw nothing on top */
        free(mem);
        return NULL;
    }
    jlong points = 0;
    int ok = 1;
    for (jsize i = 0; ok && i < n; i++) {
        ok = mem[i] >= 1;
        points += mem[i];
    }
    if (!ok || 2 * points > (jlong)nc) {
        bad_arg(e, "jxlatte_amd: spline control point counts and array disagree");
        free(mem);
        return NULL;
    }
    d->quant_adjust = quantAdjust;
    d->n_splines = n;
    d->n_control = (const int32_t*)mem;
    d->control = (const int32_t*)(mem + n);
    d->coeff = (const int32_t*)(mem + n + nc);
    d->base_corr_x = bcx;
    d->base_corr_b = bcb;
    return mem;
}

/* Frame.renderSplines (Frame.java:739-746) on the resident planes */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesSplines(JNIEnv* e, jobject self, jint quantAdjust, jintArray nControl,
        jintArray control, jintArray coeff, jfloat baseCorrX, jfloat baseCorrB) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_spline_desc d;
    jint* mem = spline_desc(e, quantAdjust, nControl, control, coeff, baseCorrX, baseCorrB, &d);
    if (!mem) return;
    const jxl_status st = jxl_planes_splines(c, &d);
    free(mem);
    CHECK(st);
}

/* ... on three host planes of height x width floats, in place */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageSplines(JNIEnv* e, jobject self, jobject p0, jobject p1, jobject p2,
        jint h, jint w, jint quantAdjust, jintArray nControl, jintArray control, jintArray coeff, jfloat baseCorrX, jfloat baseCorrB) {
    jxl_ctx* c = ctx_of(e, self);
    float* pl[3] = {(float*)ADDR(p0), (float*)ADDR(p1), (float*)ADDR(p2)};
    if (h < 1 || w < 1) { bad_arg(e, "jxlatte_amd: plane size"); return; }
    NEED(p0, 4 * area(h, w)); NEED(p1, 4 * area(h, w)); NEED(p2, 4 * area(h, w));
    jxl_spline_desc d;
    jint* mem = spline_desc(e, quantAdjust, nControl, control, coeff, baseCorrX, baseCorrB, &d);
    if (!mem) return;
    const jxl_status st = jxl_stage_splines(c, pl, h, w, &d);
    free(mem);
    CHECK(st);
}

/* the arc table (host only): 12 ints per arc, jxl_spline_arc word for word (the floats as Float.floatToRawIntBits) */
JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_splineArcs(JNIEnv* e, jclass k, jint h, jint w, jint quantAdjust,
        jintArray nControl, jintArray control, jintArray coeff, jfloat baseCorrX, jfloat baseCorrB) {
    (void)k;
    jxl_spline_desc d;
    jint* mem = spline_desc(e, quantAdjust, nControl, control, coeff, baseCorrX, baseCorrB, &d);
    if (!mem) return NULL;
    jintArray out = NULL;
    int64_t n = jxl_spline_arcs(&d, h, w, NULL, 0);
    jxl_spline_arc* arcs = NULL;
    if (n >= 0 && n > 0x7fffffff / 12) n = JXL_ERR_OOM;
    if (n > 0 && !(arcs = (jxl_spline_arc*)malloc(sizeof(jxl_spline_arc) * (size_t)n))) n = JXL_ERR_OOM;
    if (n > 0) n = jxl_spline_arcs(&d, h, w, arcs, n);
    if (n < 0) rethrow(e, NULL, (jxl_status)n);
    else if ((out = (*e)->NewIntArray(e, (jsize)(12 * n))) && n) (*e)->SetIntArrayRegion(e, out, 0, (jsize)(12 * n), (const jint*)arcs);
    free(arcs);
    free(mem);
    return out;
}

/* ---- patches (include/jxlatte_amd.h: jxl_patch_bins, jxl_stage_patches, jxl_planes_patches) ----
 * The patch stage of a frame (JXLCodestreamDecoder.computePatches, :212-254), flattened: pos = 8 ints per position in stage order
 * (jxl_patch_pos word for word), blend = rows of (nColor + ecIsAlpha.length) x 3 ints, refShape = (h, w) per reference slot (0, 0:
 * absent). The arrays are copied and checked against each other before the library sees them; *mem is the copy (free it), NULL
 * with an exception pending on failure. */
static jint* patch_desc0(JNIEnv* e, jintArray pos, jintArray blend, jint nColor, jintArray ecIsAlpha, jintArray ecAlphaAssociated,
                         jintArray refShape, int with_shape, jxl_patch_desc* d) {
    if (!pos || !blend || !ecIsAlpha || !ecAlphaAssociated || (with_shape && !refShape)) {
        bad_arg(e, "jxlatte_amd: patch arrays missing");
        return NULL;
    }
    const jsize np = (*e)->GetArrayLength(e, pos), nb = (*e)->GetArrayLength(e, blend), ne = (*e)->GetArrayLength(e, ecIsAlpha);
    const jlong row = 3 * ((jlong)nColor + ne);
    if ((nColor != 1 && nColor != 3) || np % 8 || nb % row || (*e)->GetArrayLength(e, ecAlphaAssociated) != ne ||
        (with_shape && (*e)->GetArrayLength(e, refShape) != 8)) {
        bad_arg(e, "jxlatte_amd: patch arrays disagree");
        return NULL;
    }
    jint* mem = (jint*)malloc(sizeof(jint) * ((size_t)np + (size_t)nb + 2 * (size_t)ne + 8 + 1));
    if (!mem) {
        (*e)->ThrowNew(e, (*e)->FindClass(e, "java/lang/OutOfMemoryError"), "jxlatte_amd: patch arrays");
        return NULL;
    }
    jint* shape = mem + np + nb + 2 * ne;
    (*e)->GetIntArrayRegion(e, pos, 0, np, mem);
    (*e)->GetIntArrayRegion(e, blend, 0, nb, mem + np);
    (*e)->GetIntArrayRegion(e, ecIsAlpha, 0, ne, mem + np + nb);
    (*e)->GetIntArrayRegion(e, ecAlphaAssociated, 0, ne, mem + np + nb + ne);
    memset(shape, 0, 8 * sizeof(jint));
    if (with_shape) (*e)->GetIntArrayRegion(e, refShape, 0, 8, shape);
    if ((*e)->ExceptionCheck(e)) {
        free(mem);
        return NULL;
    }
    d->n_pos = np / 8;
    d->pos = (const jxl_patch_pos*)mem;
    d->n_rows = (int32_t)(nb / row);
    d->blend = (const int32_t*)(mem + np);
    d->n_color = nColor;
    d->n_extra = ne;
    d->ec_is_alpha = (const int32_t*)(mem + np + nb);
    d->ec_alpha_associated = (const int32_t*)(mem + np + nb + ne);
    for (int k = 0; k < 4; k++) d->ref_h[k] = shape[2 * k], d->ref_w[k] = shape[2 * k + 1];
    return mem;
}
static jint* patch_desc(JNIEnv* e, jintArray pos, jintArray blend, jint nColor, jintArray ecIsAlpha, jintArray ecAlphaAssociated,
                        jintArray refShape, jxl_patch_desc* d) {
    return patch_desc0(e, pos, blend, nColor, ecIsAlpha, ecAlphaAssociated, refShape, 1, d);
}
/* n plane buffers of a ByteBuffer[] with their types (0 float, 1 int, -1 / null: absent) against the sizes they must have;
 * 0 with an exception pending when something is missing or too small */
static int patch_planes(JNIEnv* e, jobjectArray bufs, jintArray types, jsize n, const jlong* bytes, int may_be_null, void** out, jint* type) {
    if (!bufs || !types || (*e)->GetArrayLength(e, bufs) != n || (*e)->GetArrayLength(e, types) != n) {
        bad_arg(e, "jxlatte_amd: patch plane arrays missing or of the wrong length");
        return 0;
    }
    (*e)->GetIntArrayRegion(e, types, 0, n, type);
    for (jsize i = 0; i < n; i++) {
        jobject b = (*e)->GetObjectArrayElement(e, bufs, i);
        out[i] = NULL;
        if (!b || type[i] == -1) {
            if (!may_be_null) {
                bad_arg(e, "jxlatte_amd: a frame plane is missing");
                return 0;
            }
            type[i] = -1;
            continue;
        }
        if (!has_room(e, b, bytes[i])) {
            bad_arg(e, "jxlatte_amd: a patch plane buffer is not direct or too small");
            return 0;
        }
        out[i] = (*e)->GetDirectBufferAddress(e, b);
    }
    return !(*e)->ExceptionCheck(e);
}
#define PATCH_MAX_CHAN 64

/* computePatches on host planes, in place (jxl_stage_patches), or with extra == frame planes 3.. on the resident colour planes
 * (jxl_planes_patches: height, width < 0) */
static void patches_call(JNIEnv* e, jobject self, int resident, jobjectArray frame, jintArray frameType, jint h, jint w, jobjectArray ref,
                         jintArray refType, jintArray pos, jintArray blend, jint nColor, jintArray ecIsAlpha, jintArray ecAlphaAssociated,
                         jintArray refShape) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_patch_desc d;
    jint* mem = patch_desc(e, pos, blend, nColor, ecIsAlpha, ecAlphaAssociated, refShape, &d);
    if (!mem) return;
    const int n_chan = d.n_color + d.n_extra, n_frame = resident ? d.n_extra : n_chan;
    void* fp[PATCH_MAX_CHAN];
    void* rp[4 * PATCH_MAX_CHAN];
    jint ft[PATCH_MAX_CHAN], rt[4 * PATCH_MAX_CHAN];
    jlong fb[PATCH_MAX_CHAN], rb[4 * PATCH_MAX_CHAN];
    jxl_status st = JXL_OK;
    if (n_chan > PATCH_MAX_CHAN || (resident && d.n_color != 3)) {
        bad_arg(e, "jxlatte_amd: channel count");
    } else {
        if (resident && jxl_planes_shape(c, &h, &w) != JXL_OK) h = w = 0;
        for (int i = 0; i < n_frame; i++) fb[i] = 4 * area(h, w);
        for (int k = 0; k < 4; k++)
            for (int i = 0; i < n_chan; i++) rb[k * n_chan + i] = 4 * area(d.ref_h[k], d.ref_w[k]);
        if (patch_planes(e, frame, frameType, n_frame, fb, 0, fp, ft) && patch_planes(e, ref, refType, 4 * n_chan, rb, 1, rp, rt))
            st = resident ? jxl_planes_patches(c, &d, fp, (const int32_t*)ft, (const void* const*)rp, (const int32_t*)rt)
                          : jxl_stage_patches(c, &d, fp, (const int32_t*)ft, h, w, (const void* const*)rp, (const int32_t*)rt);
    }
    free(mem);
    if (!(*e)->ExceptionCheck(e)) CHECK(st);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stagePatches(JNIEnv* e, jobject self, jobjectArray frame, jintArray frameType,
        jint h, jint w, jobjectArray ref, jintArray refType, jintArray pos, jintArray blend, jint nColor, jintArray ecIsAlpha,
        jintArray ecAlphaAssociated, jintArray refShape) {
    if (h < 1 || w < 1) { bad_arg(e, "jxlatte_amd: plane size"); return; }
    patches_call(e, self, 0, frame, frameType, h, w, ref, refType, pos, blend, nColor, ecIsAlpha, ecAlphaAssociated, refShape);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesPatches(JNIEnv* e, jobject self, jobjectArray extra, jintArray extraType,
        jobjectArray ref, jintArray refType, jintArray pos, jintArray blend, jintArray ecIsAlpha, jintArray ecAlphaAssociated, jintArray refShape) {
    patches_call(e, self, 1, extra, extraType, 0, 0, ref, refType, pos, blend, 3, ecIsAlpha, ecAlphaAssociated, refShape);
}

/* validation and tile lists (host only): { tiles, list entries, tile[tiles], start[tiles + 1], list[entries] } */
JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_patchBins(JNIEnv* e, jclass k, jint h, jint w, jintArray frameType,
        jintArray refType, jintArray pos, jintArray blend, jint nColor, jintArray ecIsAlpha, jintArray ecAlphaAssociated, jintArray refShape) {
    (void)k;
    jxl_patch_desc d;
    jint* mem = patch_desc(e, pos, blend, nColor, ecIsAlpha, ecAlphaAssociated, refShape, &d);
    if (!mem) return NULL;
    const int n_chan = d.n_color + d.n_extra;
    jint ft[PATCH_MAX_CHAN], rt[4 * PATCH_MAX_CHAN];
    jintArray out = NULL;
    jint* buf = NULL;
    if (n_chan > PATCH_MAX_CHAN || !frameType || !refType || (*e)->GetArrayLength(e, frameType) != n_chan ||
        (*e)->GetArrayLength(e, refType) != 4 * n_chan) {
        bad_arg(e, "jxlatte_amd: patch plane types missing or of the wrong length");
    } else {
        (*e)->GetIntArrayRegion(e, frameType, 0, n_chan, ft);
        (*e)->GetIntArrayRegion(e, refType, 0, 4 * n_chan, rt);
        int64_t n_list = 0;
        int32_t bad = -1;
        int64_t n = jxl_patch_bins(&d, h, w, (const int32_t*)ft, (const int32_t*)rt, NULL, NULL, NULL, 0, 0, &n_list, &bad);
        if (n >= 0 && 3 + 2 * n + n_list > 0x7fffffff) n = JXL_ERR_OOM;
        if (n >= 0 && !(buf = (jint*)malloc(sizeof(jint) * (size_t)(3 + 2 * n + n_list)))) n = JXL_ERR_OOM;
        if (n >= 0) {
            buf[0] = (jint)n, buf[1] = (jint)n_list;
            n = jxl_patch_bins(&d, h, w, (const int32_t*)ft, (const int32_t*)rt, (int32_t*)buf + 2, (int32_t*)buf + 2 + n, (int32_t*)buf + 3 + 2 * n, n,
                               n_list, &n_list, &bad);
        }
        if (n < 0) {
            const char* cls = n == JXL_ERR_INVALID_BITSTREAM ? "com/traneptora/jxlatte/io/InvalidBitstreamException"
                            : n == JXL_ERR_UNSUPPORTED       ? "java/lang/UnsupportedOperationException"
                            : n == JXL_ERR_OOM               ? "java/lang/OutOfMemoryError"
                                                             : "java/lang/IllegalArgumentException";
            (*e)->ThrowNew(e, (*e)->FindClass(e, cls), jxl_last_error(NULL));
        } else if ((out = (*e)->NewIntArray(e, (jsize)(3 + 2 * n + n_list)))) {
            (*e)->SetIntArrayRegion(e, out, 0, (jsize)(3 + 2 * n + n_list), buf);
        }
    }
    free(buf);
    free(mem);
    return out;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_runBatch0(JNIEnv* e, jclass k, jlongArray ctxs) {
    (void)k;
    const jsize n = (*e)->GetArrayLength(e, ctxs);
    jlong h[64];
    jxl_ctx* c[64];
    if (n <= 0 || n > 64) {
        rethrow(e, NULL, JXL_ERR_INVALID_ARGUMENT);
        return;
    }
    (*e)->GetLongArrayRegion(e, ctxs, 0, n, h);
    for (jsize i = 0; i < n; i++) c[i] = (jxl_ctx*)(intptr_t)h[i];
    const jxl_status st = jxl_vardct_run_batch(c, (int32_t)n);
    if (st != JXL_OK) rethrow(e, c[0], st);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularApply(JNIEnv* e, jobject self, jobjectArray chans, jintArray widths,
        jintArray heights, jintArray squeezeParams, jint rctType, jint rctBegin, jobjectArray out, jintArray outWidths, jintArray outHeights) {
    jxl_ctx* c = ctx_of(e, self);
    const jsize n = (*e)->GetArrayLength(e, chans), n_out = (*e)->GetArrayLength(e, out);
    const jsize n_sp = (*e)->GetArrayLength(e, squeezeParams) / 4;
    if (n > 256 || n_out > 256 || n_sp > 64) {
        rethrow(e, c, JXL_ERR_INVALID_ARGUMENT);
        return;
    }
    jxl_channel ci[256], co[256];
    jxl_squeeze_param sp[64];
    jint w[256], h[256], ow[256], oh[256], spv[256];
    GETI(widths, n, w);
    GETI(heights, n, h);
    GETI(outWidths, n_out, ow);
    GETI(outHeights, n_out, oh);
    GETI(squeezeParams, n_sp * 4, spv);
    for (jsize i = 0; i < n; i++) {
        jobject b = (*e)->GetObjectArrayElement(e, chans, i);
        if ((*e)->ExceptionCheck(e)) return;
        ci[i].width = w[i]; ci[i].height = h[i];
        if (area(h[i], w[i]) > 0) NEED(b, 4 * area(h[i], w[i]));
        ci[i].data = (int32_t*)ADDR(b);
    }
    for (jsize i = 0; i < n_out; i++) {
        jobject b = (*e)->GetObjectArrayElement(e, out, i);
        if ((*e)->ExceptionCheck(e)) return;
        co[i].width = ow[i]; co[i].height = oh[i];
        if (area(oh[i], ow[i]) > 0) NEED(b, 4 * area(oh[i], ow[i]));
        co[i].data = (int32_t*)ADDR(b);
    }
    for (jsize i = 0; i < n_sp; i++) {
        sp[i].horizontal = spv[4 * i]; sp[i].in_place = spv[4 * i + 1]; sp[i].begin_c = spv[4 * i + 2]; sp[i].num_c = spv[4 * i + 3];
    }
    CHECK(jxl_modular_apply(c, ci, n, sp, n_sp, rctType, rctBegin, co, n_out));
}

/* ---- context / diagnostics ---- */
JNIEXPORT jstring JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_version(JNIEnv* e, jclass k) {
    (void)k;
    return (*e)->NewStringUTF(e, jxl_version());
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_synchronize(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_ctx_synchronize(c));
}

JNIEXPORT jlong JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stream(JNIEnv* e, jobject self) {
    return (jlong)(intptr_t)jxl_ctx_stream(ctx_of(e, self));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_setStream(JNIEnv* e, jobject self, jlong hipStream) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_ctx_set_stream(c, (void*)(intptr_t)hipStream));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_copyOutputDevice(JNIEnv* e, jobject self, jlong dstDevice) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_vardct_copy_output_device(c, (void*)(intptr_t)dstDevice));
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_outElemSize(JNIEnv* e, jobject self) {
    return jxl_vardct_out_elem_size(ctx_of(e, self));
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_lastLaunchCount(JNIEnv* e, jobject self) {
    return jxl_vardct_last_launch_count(ctx_of(e, self));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_enableStageTiming(JNIEnv* e, jobject self, jboolean on) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_vardct_enable_stage_timing(c, on ? 1 : 0));
}

JNIEXPORT jfloat JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_lastStageMs(JNIEnv* e, jobject self, jint which) {
    jxl_ctx* c = ctx_of(e, self);
    float ms = 0.0f;
    const jxl_status st = jxl_vardct_last_stage_ms(c, which, &ms);
    if (st != JXL_OK) rethrow(e, c, st);
    return ms;
}

JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_coeffPlaneRows(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t rows[3] = {0, 0, 0};
    const jxl_status st = jxl_vardct_coeff_plane_rows(c, rows);
    if (st != JXL_OK) { rethrow(e, c, st); return NULL; }
    jintArray out = (*e)->NewIntArray(e, 3);
    if (out) (*e)->SetIntArrayRegion(e, out, 0, 3, (const jint*)rows);
    return out;
}

/* ---- stage entries: one reference function each (host planes in / out as direct buffers) ---- */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageIdct2d(JNIEnv* e, jobject self, jobject src, jobject dst, jint h, jint w,
        jboolean transposed) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_stage_idct2d(c, (const float*)ADDR(src), (float*)ADDR(dst), h, w, transposed ? 1 : 0));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageFdct2d(JNIEnv* e, jobject self, jobject src, jobject dst, jint h, jint w) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_stage_fdct2d(c, (const float*)ADDR(src), (float*)ADDR(dst), h, w));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageGab(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2, jobject o0,
        jobject o1, jobject o2, jint h, jint w, jfloatArray w1, jfloatArray w2) {
    jxl_ctx* c = ctx_of(e, self);
    const float* in[3] = {(const float*)ADDR(i0), (const float*)ADDR(i1), (const float*)ADDR(i2)};
    float* out[3] = {(float*)ADDR(o0), (float*)ADDR(o1), (float*)ADDR(o2)};
    float a[3], b[3];
    GETF(w1, 3, a);
    GETF(w2, 3, b);
    NEED(i0, 4 * area(h, w)); NEED(i1, 4 * area(h, w)); NEED(i2, 4 * area(h, w));
    NEED(o0, 4 * area(h, w)); NEED(o1, 4 * area(h, w)); NEED(o2, 4 * area(h, w));
    CHECK(jxl_stage_gab(c, in, out, h, w, a, b));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageEpf(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2, jobject o0,
        jobject o1, jobject o2, jint h, jint w, jint iterations, jobject invSigma, jfloat invSigmaModular, jfloatArray channelScale,
        jfloat pass0, jfloat pass2, jfloat borderSadMul) {
    jxl_ctx* c = ctx_of(e, self);
    const float* in[3] = {(const float*)ADDR(i0), (const float*)ADDR(i1), (const float*)ADDR(i2)};
    float* out[3] = {(float*)ADDR(o0), (float*)ADDR(o1), (float*)ADDR(o2)};
    float cs[3];
    GETF(channelScale, 3, cs);
    NEED(i0, 4 * area(h, w)); NEED(i1, 4 * area(h, w)); NEED(i2, 4 * area(h, w));
    NEED(o0, 4 * area(h, w)); NEED(o1, 4 * area(h, w)); NEED(o2, 4 * area(h, w));
    NEED_OPT(invSigma, 4 * area(((jlong)h + 7) / 8, ((jlong)w + 7) / 8));
    CHECK(jxl_stage_epf(c, in, out, h, w, iterations, (const float*)ADDR(invSigma), invSigmaModular, cs, pass0, pass2, borderSadMul));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageRestoreFused(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jobject o0, jobject o1, jobject o2, jint h, jint w, jobject hfMul, jobject sharpness, jobject params) {
    jxl_ctx* c = ctx_of(e, self);
    const float* in[3] = {(const float*)ADDR(i0), (const float*)ADDR(i1), (const float*)ADDR(i2)};
    float* out[3] = {(float*)ADDR(o0), (float*)ADDR(o1), (float*)ADDR(o2)};
    jxl_vardct_params p;
    const void* src = params ? (*e)->GetDirectBufferAddress(e, params) : NULL;
    if (!src || (*e)->GetDirectBufferCapacity(e, params) < (jlong)sizeof p) {
        bad_arg(e, "jxlatte_amd: stageRestoreFused needs a direct buffer holding jxl_vardct_params");
        return;
    }
    memcpy(&p, src, sizeof p);
    NEED(i0, 4 * area(h, w)); NEED(i1, 4 * area(h, w)); NEED(i2, 4 * area(h, w));
    NEED(o0, 4 * area(h, w)); NEED(o1, 4 * area(h, w)); NEED(o2, 4 * area(h, w));
    NEED_OPT(hfMul, 4 * area(((jlong)h + 7) / 8, ((jlong)w + 7) / 8));
    NEED_OPT(sharpness, 4 * area(((jlong)h + 7) / 8, ((jlong)w + 7) / 8));
    CHECK(jxl_stage_restore_fused(c, in, out, h, w, (const int32_t*)ADDR(hfMul), (const int32_t*)ADDR(sharpness), &p));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageEpfSigma(JNIEnv* e, jobject self, jobject hfMul, jobject sharpness, jint bh,
        jint bw, jfloat globalScale, jfloatArray sharpLut, jobject invSigma) {
    jxl_ctx* c = ctx_of(e, self);
    float lut[8];
    GETF(sharpLut, 8, lut);
    NEED(hfMul, 4 * area(bh, bw)); NEED(sharpness, 4 * area(bh, bw)); NEED(invSigma, 4 * area(bh, bw));
    CHECK(jxl_stage_epf_sigma(c, (const int32_t*)ADDR(hfMul), (const int32_t*)ADDR(sharpness), bh, bw, globalScale, lut, (float*)ADDR(invSigma)));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageLfDequant(JNIEnv* e, jobject self, jint lfgY, jint lfgX, jint cellsH,
        jint cellsW, jobject qX, jobject qY, jobject qB, jint extraPrecision, jfloatArray scaledDequant, jint xFactorLF, jint bFactorLF,
        jboolean adaptiveSmoothing, jfloat baseCorrX, jfloat baseCorrB, jint colorFactor, jobject o0, jobject o1, jobject o2) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_lfquant_desc d;
    memset(&d, 0, sizeof d);
    d.lfg_y = lfgY; d.lfg_x = lfgX; d.cells_h = cellsH; d.cells_w = cellsW;
    d.lf_quant[0] = (const int32_t*)ADDR(qX); d.lf_quant[1] = (const int32_t*)ADDR(qY); d.lf_quant[2] = (const int32_t*)ADDR(qB);
    d.extra_precision = extraPrecision;
    GETF(scaledDequant, 3, d.scaled_dequant);
    d.x_factor_lf = xFactorLF; d.b_factor_lf = bFactorLF; d.adaptive_smoothing = adaptiveSmoothing ? 1 : 0;
    NEED(qX, 4 * area(cellsH, cellsW)); NEED(qY, 4 * area(cellsH, cellsW)); NEED(qB, 4 * area(cellsH, cellsW));
    NEED(o0, 4 * area(cellsH, cellsW)); NEED(o1, 4 * area(cellsH, cellsW)); NEED(o2, 4 * area(cellsH, cellsW));
    float* out[3] = {(float*)ADDR(o0), (float*)ADDR(o1), (float*)ADDR(o2)};
    CHECK(jxl_stage_lf_dequant(c, &d, baseCorrX, baseCorrB, colorFactor, out));
}

/* ---- the LF image of a frame as the picture at 1:8, one launch. heads: eight ints per LF group (lfg_y, lfg_x, cells_h, cells_w,
 * extra_precision, x_factor_lf, b_factor_lf, adaptive_smoothing); scaledDequant: three floats per group; ints: every group's X, Y, B
 * planes back to back, in the groups' order, in ONE direct buffer; xyb: null, or 16 floats (matrix, opsin bias, cbrt opsin bias,
 * intensity target). o0..o2: three host planes of cellsH x cellsW floats (jxl_stage_lf_image), or all null: the planes become the
 * resident planes (jxl_planes_from_lf). ---- */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_lfImage(JNIEnv* e, jobject self, jintArray heads, jfloatArray scaledDequant,
        jobject ints, jint cellsH, jint cellsW, jfloat baseCorrX, jfloat baseCorrB, jint colorFactor, jfloatArray xyb, jobject o0, jobject o1,
        jobject o2) {
    jxl_ctx* c = ctx_of(e, self);
    if (!heads || !scaledDequant) {
        bad_arg(e, "jxlatte_amd: lfImage takes eight ints and three floats per LF group");
        return;
    }
    const jsize len = (*e)->GetArrayLength(e, heads);
    const jsize n = len / 8;
    if (len % 8 || n < 1 || n > (1 << 16) || (*e)->GetArrayLength(e, scaledDequant) != 3 * n) {
        bad_arg(e, "jxlatte_amd: lfImage takes eight ints and three floats per LF group");
        return;
    }
    jxl_lf_image_desc d;
    memset(&d, 0, sizeof d);
    if (xyb) {
        float v[16];
        GETF(xyb, 16, v);
        d.xyb = 1;
        memcpy(d.opsin_matrix, v, sizeof d.opsin_matrix);
        memcpy(d.opsin_bias, v + 9, sizeof d.opsin_bias);
        memcpy(d.cbrt_opsin_bias, v + 12, sizeof d.cbrt_opsin_bias);
        d.intensity_target = v[15];
    }
    const int to_host = o0 || o1 || o2;
    if (to_host) {
        NEED(o0, 4 * area(cellsH, cellsW)); NEED(o1, 4 * area(cellsH, cellsW)); NEED(o2, 4 * area(cellsH, cellsW));
    }
    jint* hd = (jint*)malloc(sizeof(jint) * (size_t)len);
    float* sd = (float*)malloc(sizeof(float) * 3 * (size_t)n);
    jxl_lfquant_desc* g = (jxl_lfquant_desc*)calloc((size_t)n, sizeof *g);
    int ok = hd && sd && g;
    if (!ok) (*e)->ThrowNew(e, (*e)->FindClass(e, "java/lang/OutOfMemoryError"), "jxlatte_amd: lfImage");
    if (ok) ok = get_ints(e, heads, len, hd) && get_floats(e, scaledDequant, 3 * n, sd);
    jlong at = 0;  /* int32s of `ints` used so far */
    for (jsize i = 0; ok && i < n; i++) {
        const jint* h = hd + 8 * (size_t)i;
        if (h[2] < 1 || h[3] < 1 || h[2] > 256 || h[3] > 256) {
            bad_arg(e, "jxlatte_amd: lfImage: bad LF group size");
            ok = 0;
            break;
        }
        g[i].lfg_y = h[0]; g[i].lfg_x = h[1]; g[i].cells_h = h[2]; g[i].cells_w = h[3];
        g[i].extra_precision = h[4]; g[i].x_factor_lf = h[5]; g[i].b_factor_lf = h[6]; g[i].adaptive_smoothing = h[7] ? 1 : 0;
        for (int k = 0; k < 3; k++) {
            g[i].scaled_dequant[k] = sd[3 * (size_t)i + k];
            g[i].lf_quant[k] = (const int32_t*)(intptr_t)at;  /* an offset until the buffer's size is known to hold them all */
            at += (jlong)h[2] * h[3];
        }
    }
    if (ok && !has_room(e, ints, 4 * at)) {
        bad_arg(e, "jxlatte_amd: direct buffer ints missing or too small");
        ok = 0;
    }
    jxl_status st = JXL_OK;
    if (ok) {
        const int32_t* base = (const int32_t*)ADDR(ints);
        for (jsize i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) g[i].lf_quant[k] = base + (intptr_t)g[i].lf_quant[k];
        d.n_groups = (int32_t)n; d.cells_h = cellsH; d.cells_w = cellsW; d.color_factor = colorFactor;
        d.groups = g; d.base_corr_x = baseCorrX; d.base_corr_b = baseCorrB;
        if (to_host) {
            float* out[3] = {(float*)ADDR(o0), (float*)ADDR(o1), (float*)ADDR(o2)};
            st = jxl_stage_lf_image(c, &d, out);
        } else {
            st = jxl_planes_from_lf(c, &d);
        }
    }
    free(g);
    free(sd);
    free(hd);
    if (ok) CHECK(st);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageXyb(JNIEnv* e, jobject self, jobject p0, jobject p1, jobject p2, jlong n,
        jfloatArray matrix, jfloatArray bias, jfloatArray cbrtBias, jfloat intensityTarget) {
    jxl_ctx* c = ctx_of(e, self);
    float* pl[3] = {(float*)ADDR(p0), (float*)ADDR(p1), (float*)ADDR(p2)};
    float m[9], b[3], cb[3];
    GETF(matrix, 9, m);
    GETF(bias, 3, b);
    GETF(cbrtBias, 3, cb);
    NEED(p0, 4 * n); NEED(p1, 4 * n); NEED(p2, 4 * n);
    CHECK(jxl_stage_xyb(c, pl, n, m, b, cb, intensityTarget));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageYcbcr(JNIEnv* e, jobject self, jobject p0, jobject p1, jobject p2, jlong n) {
    jxl_ctx* c = ctx_of(e, self);
    float* pl[3] = {(float*)ADDR(p0), (float*)ADDR(p1), (float*)ADDR(p2)};
    NEED(p0, 4 * n); NEED(p1, 4 * n); NEED(p2, 4 * n);
    CHECK(jxl_stage_ycbcr(c, pl, n));
}

/* transfer + quantise (PNGWriter.java:65,105-111): outF or outI is null */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageTransfer(JNIEnv* e, jobject self, jobject in, jlong n, jint transfer,
        jint maxValue, jobject outF, jobject outI) {
    jxl_ctx* c = ctx_of(e, self);
    NEED(in, 4 * n); NEED_OPT(outF, 4 * n); NEED_OPT(outI, 4 * n);
    CHECK(jxl_stage_transfer(c, (const float*)ADDR(in), n, transfer, maxValue, (float*)ADDR(outF), (int32_t*)ADDR(outI)));
}

/* JXLImage.transform's sample chain (JXLImage.java:185-286): params = struct jxl_color_params in a direct buffer; i1, i2 are null for
 * one input plane, o1, o2 for one output plane. A thin pass-through: nothing on the Java side calls it yet. */
static int color_params(JNIEnv* e, jobject params, jxl_color_params* p) {
    const void* src = params ? (*e)->GetDirectBufferAddress(e, params) : NULL;
    if (!src || (*e)->GetDirectBufferCapacity(e, params) < (jlong)sizeof *p) {
        bad_arg(e, "jxlatte_amd: a direct buffer holding jxl_color_params is needed");
        return 0;
    }
    memcpy(p, src, sizeof *p);
    return 1;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageColorConvert(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jlong n, jobject params, jobject o0, jobject o1, jobject o2) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_color_params p;
    if (!color_params(e, params, &p)) return;
    NEED(i0, 4 * n); NEED_OPT(i1, 4 * n); NEED_OPT(i2, 4 * n);
    NEED(o0, 4 * n); NEED_OPT(o1, 4 * n); NEED_OPT(o2, 4 * n);
    const void* in[3] = {ADDR(i0), ADDR(i1), ADDR(i2)};
    void* out[3] = {ADDR(o0), ADDR(o1), ADDR(o2)};
    CHECK(jxl_stage_color_convert(c, in, n, &p, out));
}

/* jxl_ctx_set_tone_map: tm = struct jxl_tone_map in a direct buffer arms the context's colour passes, null clears them */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_setToneMap(JNIEnv* e, jobject self, jobject tm) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_tone_map t;
    if (!tm) {
        CHECK(jxl_ctx_set_tone_map(c, NULL));
        return;
    }
    const void* src = (*e)->GetDirectBufferAddress(e, tm);
    if (!src || (*e)->GetDirectBufferCapacity(e, tm) < (jlong)sizeof t) {
        bad_arg(e, "jxlatte_amd: a direct buffer holding jxl_tone_map is needed");
        return;
    }
    memcpy(&t, src, sizeof t);
    CHECK(jxl_ctx_set_tone_map(c, &t));
}

/* JXLImage.determinePeak (:214-223) */
JNIEXPORT jfloat JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageColorPeak(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jint h, jint w, jobject params) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_color_params p;
    float peak = 0.0f;
    if (!color_params(e, params, &p)) return 0.0f;
    if (!has_room(e, i0, 4 * area(h, w)) || (i1 && !has_room(e, i1, 4 * area(h, w))) || (i2 && !has_room(e, i2, 4 * area(h, w)))) {
        bad_arg(e, "jxlatte_amd: direct buffer of a colour plane missing or too small");
        return 0.0f;
    }
    const void* in[3] = {ADDR(i0), ADDR(i1), ADDR(i2)};
    jxl_status st = jxl_stage_color_peak(c, in, h, w, &p, &peak);
    if (st != JXL_OK) { rethrow(e, c, st); return 0.0f; }
    return peak;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageInvHSqueeze(JNIEnv* e, jobject self, jobject avg, jint aw, jobject res,
        jint rw, jint h, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    NEED(avg, 4 * area(h, aw)); NEED(res, 4 * area(h, rw)); NEED(out, 4 * area(h, (jlong)aw + rw));
    CHECK(jxl_stage_inv_hsqueeze(c, (const int32_t*)ADDR(avg), aw, (const int32_t*)ADDR(res), rw, h, (int32_t*)ADDR(out)));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageInvVSqueeze(JNIEnv* e, jobject self, jobject avg, jint ah, jobject res,
        jint rh, jint w, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    NEED(avg, 4 * area(ah, w)); NEED(res, 4 * area(rh, w)); NEED(out, 4 * area((jlong)ah + rh, w));
    CHECK(jxl_stage_inv_vsqueeze(c, (const int32_t*)ADDR(avg), ah, (const int32_t*)ADDR(res), rh, w, (int32_t*)ADDR(out)));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageRct(JNIEnv* e, jobject self, jobject v0, jobject v1, jobject v2, jlong n,
        jint rctType) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t* v[3] = {(int32_t*)ADDR(v0), (int32_t*)ADDR(v1), (int32_t*)ADDR(v2)};
    NEED(v0, 4 * n); NEED(v1, 4 * n); NEED(v2, 4 * n);
    CHECK(jxl_stage_rct(c, v, n, rctType));
}

/* Palette branch of ModularStream.applyTransforms (ModularStream.java:327-378; jxl_stage_palette). params = {numC, nbColors,
 * nbDeltas, dPred, bitDepth}; index and pred (or null) hold height * width ints, palette palH * palW (null only when that is
 * 0), out numC buffers of height * width ints each (out[0] may be index). Every size is checked against the buffers'
 * capacities before the library sees a pointer. */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stagePalette(JNIEnv* e, jobject self, jobject index, jint h, jint w,
        jobject palette, jint palH, jint palW, jobject pred, jintArray params, jobjectArray out) {
    jxl_ctx* c = ctx_of(e, self);
    jint p[5];
    if (!get_ints(e, params, 5, p)) return;
    if (h < 1 || w < 1 || palH < 0 || palW < 0 || p[0] < 1) { bad_arg(e, "jxlatte_amd: palette geometry"); return; }
    const jlong plane = 4 * area(h, w), pal = 4 * area(palH, palW);
    NEED(index, plane);
    NEED_OPT(pred, plane);
    if (pal > 0) NEED(palette, pal);
    if (!out || (*e)->GetArrayLength(e, out) < p[0]) { bad_arg(e, "jxlatte_amd: fewer output planes than numC"); return; }
    int32_t** planes = (int32_t**)malloc(sizeof(int32_t*) * (size_t)p[0]);
    if (!planes) {
        (*e)->ThrowNew(e, (*e)->FindClass(e, "java/lang/OutOfMemoryError"), "jxlatte_amd: palette plane list");
        return;
    }
    for (jint i = 0; i < p[0]; i++) {
        jobject b = (*e)->GetObjectArrayElement(e, out, i);
        if (!has_room(e, b, plane)) {
            free(planes);
            bad_arg(e, "jxlatte_amd: palette output plane missing or too small");
            return;
        }
        planes[i] = (int32_t*)ADDR(b);
    }
    jxl_palette_desc d;
    d.num_c = p[0]; d.nb_colors = p[1]; d.nb_deltas = p[2]; d.d_pred = p[3]; d.bit_depth = p[4];
    d.pal_h = palH; d.pal_w = palW;
    d.palette = pal > 0 ? (const int32_t*)ADDR(palette) : NULL;
    d.pred = (const int32_t*)ADDR(pred);
    const jxl_status st = jxl_stage_palette(c, &d, (const int32_t*)ADDR(index), h, w, planes);
    free(planes);
    CHECK(st);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageModularToFloat(JNIEnv* e, jobject self, jobject a, jobject b, jlong n,
        jfloat scale, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    NEED(a, 4 * n); NEED_OPT(b, 4 * n); NEED(out, 4 * n);
    CHECK(jxl_stage_modular_to_float(c, (const int32_t*)ADDR(a), (const int32_t*)ADDR(b), n, scale, (float*)ADDR(out)));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageChromaUpsample(JNIEnv* e, jobject self, jobject in, jint h, jint w,
        jint xShift, jint yShift, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    if (xShift < 0 || xShift > 1 || yShift < 0 || yShift > 1) { bad_arg(e, "jxlatte_amd: chroma shift"); return; }
    NEED(in, 4 * area(h, w)); NEED(out, 4 * area((jlong)h << yShift, (jlong)w << xShift));
    CHECK(jxl_stage_chroma_upsample(c, (const float*)ADDR(in), h, w, xShift, yShift, (float*)ADDR(out)));
}

/* Frame.java:217-260 upsampling weights: packed (the bitstream's / default table) -> k * k * 25 floats */
JNIEXPORT jfloatArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_upsamplingWeights(JNIEnv* e, jclass k_, jint k, jfloatArray packed) {
    (void)k_;
    /* k first (2, 4 or 8: Frame.java:217), then the packed table's length for that k: 15, 55 or 210 weights */
    const jsize need = k == 2 ? 15 : k == 4 ? 55 : k == 8 ? 210 : -1;
    if (need < 0 || !packed || (*e)->GetArrayLength(e, packed) < need) {
        bad_arg(e, "jxlatte_amd: upsampling factor or packed weight table");
        return NULL;
    }
    jfloatArray out = (*e)->NewFloatArray(e, k * k * 25);
    if (!out) return NULL;  /* OutOfMemoryError pending */
    jfloat* p = (*e)->GetFloatArrayElements(e, packed, NULL);
    if (!p) return NULL;
    jfloat* o = (*e)->GetFloatArrayElements(e, out, NULL);
    const jxl_status st = o ? jxl_upsampling_weights(k, p, o) : JXL_ERR_OOM;
    if (o) (*e)->ReleaseFloatArrayElements(e, out, o, 0);
    (*e)->ReleaseFloatArrayElements(e, packed, p, JNI_ABORT);
    if (st != JXL_OK) { rethrow(e, NULL, st); return NULL; }
    return out;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageUpsample(JNIEnv* e, jobject self, jobject in, jint h, jint w, jint k,
        jfloatArray weights, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    if ((k != 2 && k != 4 && k != 8) || !weights || (*e)->GetArrayLength(e, weights) < k * k * 25) { bad_arg(e, "jxlatte_amd: upsampling weights"); return; }
    NEED(in, 4 * area(h, w)); NEED(out, 4 * area((jlong)h * k, (jlong)w * k));
    jfloat* wt = (*e)->GetFloatArrayElements(e, weights, NULL);
    const jxl_status st = wt ? jxl_stage_upsample(c, (const float*)ADDR(in), h, w, k, wt, (float*)ADDR(out)) : JXL_ERR_OOM;
    if (wt) (*e)->ReleaseFloatArrayElements(e, weights, wt, JNI_ABORT);
    CHECK(st);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageNoiseInit(JNIEnv* e, jobject self, jint h, jint w, jint groupDim,
        jlong seed0, jint colors, jobject o0, jobject o1, jobject o2) {
    jxl_ctx* c = ctx_of(e, self);
    float* out[3] = {(float*)ADDR(o0), (float*)ADDR(o1), (float*)ADDR(o2)};
    NEED(o0, 4 * area(h, w)); NEED(o1, 4 * area(h, w)); NEED(o2, 4 * area(h, w));
    CHECK(jxl_stage_noise_init(c, h, w, groupDim, (uint64_t)seed0, colors, out));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageNoiseAdd(JNIEnv* e, jobject self, jobject p0, jobject p1, jobject p2,
        jobject n0, jobject n1, jobject n2, jlong n, jfloatArray lut, jfloat baseCorrX, jfloat baseCorrB) {
    jxl_ctx* c = ctx_of(e, self);
    float* pl[3] = {(float*)ADDR(p0), (float*)ADDR(p1), (float*)ADDR(p2)};
    const float* nz[3] = {(const float*)ADDR(n0), (const float*)ADDR(n1), (const float*)ADDR(n2)};
    float l[8];
    GETF(lut, 8, l);
    NEED(p0, 4 * n); NEED(p1, 4 * n); NEED(p2, 4 * n); NEED(n0, 4 * n); NEED(n1, 4 * n); NEED(n2, 4 * n);
    CHECK(jxl_stage_noise_add(c, pl, nz, n, l, baseCorrX, baseCorrB));
}

/* p0..p2: the window at (y0, x0) of a frameH x frameW frame, h x w floats each, in place */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageNoiseWindow(JNIEnv* e, jobject self, jobject p0, jobject p1, jobject p2,
        jint h, jint w, jint groupDim, jlong seed0, jfloatArray lut, jfloat baseCorrX, jfloat baseCorrB, jint frameH, jint frameW, jint y0, jint x0) {
    jxl_ctx* c = ctx_of(e, self);
    float* pl[3] = {(float*)ADDR(p0), (float*)ADDR(p1), (float*)ADDR(p2)};
    float l[8];
    GETF(lut, 8, l);
    NEED(p0, 4 * area(h, w)); NEED(p1, 4 * area(h, w)); NEED(p2, 4 * area(h, w));
    CHECK(jxl_stage_noise_window(c, pl, h, w, groupDim, (uint64_t)seed0, l, baseCorrX, baseCorrB, frameH, frameW, y0, x0));
}

/* rect: {h, w, canvas_y, canvas_x, frame_y, frame_x, ref_y, ref_x} (JXLCodestreamDecoder.java:26-40, 285-422) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageBlend(JNIEnv* e, jobject self, jint mode, jint flags, jboolean isInt,
        jobject canvas, jint ch, jint cw, jobject frame, jint fh, jint fw, jobject ref, jint rh, jint rw, jobject frameAlpha, jobject refAlpha,
        jintArray rect) {
    jxl_ctx* c = ctx_of(e, self);
    jint r[8];
    GETI(rect, 8, r);
    NEED(canvas, 4 * area(ch, cw)); NEED(frame, 4 * area(fh, fw)); NEED_OPT(ref, 4 * area(rh, rw));
    NEED_OPT(frameAlpha, 4 * area(fh, fw)); NEED_OPT(refAlpha, 4 * area(rh, rw));
    jxl_blend_rect br;
    br.h = r[0]; br.w = r[1]; br.canvas_y = r[2]; br.canvas_x = r[3]; br.frame_y = r[4]; br.frame_x = r[5]; br.ref_y = r[6]; br.ref_x = r[7];
    CHECK(jxl_stage_blend(c, mode, (uint32_t)flags, isInt ? 1 : 0, ADDR(canvas), ch, cw, ADDR(frame), fh, fw, ADDR(ref), rh, rw,
                          (const float*)ADDR(frameAlpha), (const float*)ADDR(refAlpha), &br));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageOrient(JNIEnv* e, jobject self, jobject in, jint h, jint w, jint orientation,
        jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    NEED(in, 4 * area(h, w)); NEED(out, 4 * area(h, w));
    CHECK(jxl_stage_orient(c, ADDR(in), h, w, orientation, ADDR(out)));
}

/* params: {height, width, n_color, has_alpha, premultiplied, bit_depth, big_endian, is_int[4], tagged_depth[4]} (PNGWriter.java:79-111) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stagePack(JNIEnv* e, jobject self, jobjectArray planes, jintArray params,
        jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    jint pv[15];
    GETI(params, 15, pv);
    jxl_pack_params p;
    p.height = pv[0]; p.width = pv[1]; p.n_color = pv[2]; p.has_alpha = pv[3]; p.premultiplied = pv[4]; p.bit_depth = pv[5]; p.big_endian = pv[6];
    for (int i = 0; i < 4; i++) { p.is_int[i] = pv[7 + i]; p.tagged_depth[i] = pv[11 + i]; }
    const void* pl[4] = {NULL, NULL, NULL, NULL};
    if (!planes || p.n_color < 1 || p.n_color > 3 || (p.bit_depth != 8 && p.bit_depth != 16)) { bad_arg(e, "jxlatte_amd: pack parameters"); return; }
    const jsize n = (*e)->GetArrayLength(e, planes);
    const jsize want = p.n_color + (p.has_alpha ? 1 : 0);
    if (n < want) { bad_arg(e, "jxlatte_amd: pack: fewer planes than channels"); return; }
    for (jsize i = 0; i < want; i++) {
        jobject b = (*e)->GetObjectArrayElement(e, planes, i);
        NEED(b, 4 * area(p.height, p.width));
        pl[i] = ADDR(b);
    }
    NEED(out, area(p.height, p.width) * want * (p.bit_depth / 8));
    CHECK(jxl_stage_pack(c, pl, &p, ADDR(out)));
}

/* ---- the PNG's samples in one pass (PNGWriter's constructor, JXLImage.transform included): params = struct jxl_png_params in a direct
 * buffer; i1, i2 are null for one colour plane, alpha is null without an alpha channel. Thin pass-throughs. ---- */
static int png_params(JNIEnv* e, jobject params, jxl_png_params* p) {
    const void* src = params ? (*e)->GetDirectBufferAddress(e, params) : NULL;
    if (!src || (*e)->GetDirectBufferCapacity(e, params) < (jlong)sizeof *p) {
        bad_arg(e, "jxlatte_amd: a direct buffer holding jxl_png_params is needed");
        return 0;
    }
    memcpy(p, src, sizeof *p);
    if ((p->bit_depth != 8 && p->bit_depth != 16) || p->height < 1 || p->width < 1) {
        bad_arg(e, "jxlatte_amd: png parameters");
        return 0;
    }
    return 1;
}
/* the bytes of the samples `p` asks for */
static jlong png_bytes(const jxl_ctx* c, const jxl_png_params* p) {
    const int nc = (p->color.n_planes == 3 || p->color.use_matrix || jxl_ctx_tone_map_armed(c)) ? 3 : 1;
    return area(p->height, p->width) * (nc + (p->has_alpha ? 1 : 0)) * (p->bit_depth / 8);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stagePngSamples(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jobject alpha, jobject params, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_png_params p;
    if (!png_params(e, params, &p)) return;
    const jlong plane = 4 * area(p.height, p.width);
    NEED(i0, plane); NEED_OPT(i1, plane); NEED_OPT(i2, plane); NEED_OPT(alpha, plane);
    NEED(out, png_bytes(c, &p));
    const void* in[3] = {ADDR(i0), ADDR(i1), ADDR(i2)};
    CHECK(jxl_stage_png_samples(c, in, ADDR(alpha), &p, ADDR(out)));
}

/* the same on the resident planes: height and width must be theirs (the library checks) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesPngSamples(JNIEnv* e, jobject self, jobject alpha, jobject params,
        jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_png_params p;
    if (!png_params(e, params, &p)) return;
    NEED_OPT(alpha, 4 * area(p.height, p.width));
    NEED(out, png_bytes(c, &p));
    CHECK(jxl_planes_png_samples(c, ADDR(alpha), &p, ADDR(out)));
}

JNIEXPORT jfloat JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesColorPeak(JNIEnv* e, jobject self, jobject params) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_color_params p;
    float peak = 0.0f;
    if (!color_params(e, params, &p)) return 0.0f;
    jxl_status st = jxl_planes_color_peak(c, &p, &peak);
    if (st != JXL_OK) { rethrow(e, c, st); return 0.0f; }
    return peak;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesOrient(JNIEnv* e, jobject self, jint orientation) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_planes_orient(c, orientation));
}

/* ---- the PFM's samples in one pass (PFMWriter.write after its header, PFMWriter.java:30-48):
 * params: {height, width, n_planes, is_int[3], tagged_depth[3]}; i1, i2 are null for a grey image. The output buffer holds exactly
 * the file's bytes after the header: its capacity must EQUAL 4 * n_planes * width * height. ---- */
static int pfm_params(JNIEnv* e, jintArray params, jxl_pfm_params* p) {
    jint pv[9];
    if (!get_ints(e, params, 9, pv)) return 0;
    p->height = pv[0]; p->width = pv[1]; p->n_planes = pv[2];
    for (int i = 0; i < 3; i++) { p->is_int[i] = pv[3 + i]; p->tagged_depth[i] = pv[6 + i]; }
    if (p->height < 1 || p->width < 1 || (p->n_planes != 1 && p->n_planes != 3)) {
        bad_arg(e, "jxlatte_amd: pfm parameters");
        return 0;
    }
    return 1;
}
/* a direct buffer of exactly `bytes` bytes */
static int pfm_out_fits(JNIEnv* e, jobject out, jlong bytes) {
    if (has_room(e, out, bytes) && (*e)->GetDirectBufferCapacity(e, out) == bytes) return 1;
    bad_arg(e, "jxlatte_amd: the PFM output buffer must hold exactly 4 * n_planes * width * height bytes");
    return 0;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stagePfmSamples(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jintArray params, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_pfm_params p;
    if (!pfm_params(e, params, &p)) return;
    const jlong plane = 4 * area(p.height, p.width);
    NEED(i0, plane);
    if (p.n_planes == 3) { NEED(i1, plane); NEED(i2, plane); }
    if (!pfm_out_fits(e, out, plane * p.n_planes)) return;
    const void* in[3] = {ADDR(i0), p.n_planes == 3 ? ADDR(i1) : NULL, p.n_planes == 3 ? ADDR(i2) : NULL};
    CHECK(jxl_stage_pfm_samples(c, in, &p, ADDR(out)));
}

/* the same on the resident planes: height and width must be theirs (the library checks) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesPfmSamples(JNIEnv* e, jobject self, jintArray params, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_pfm_params p;
    if (!pfm_params(e, params, &p)) return;
    if (!pfm_out_fits(e, out, 4 * area(p.height, p.width) * p.n_planes)) return;
    CHECK(jxl_planes_pfm_samples(c, &p, ADDR(out)));
}

/* ---- device plane sets (the canvas and the reference frames of JXLCodestreamDecoder.decode on the device). A transfer states
 * no size of its own: the shim asks the library for the set's (jxl_canvas_describe) and the buffer must hold a plane of it. ---- */
static int canvas_desc(JNIEnv* e, jintArray desc, jxl_canvas_blend_desc* d) {
    jint head[12];
    if (!get_ints(e, desc, 12, head)) return 0;
    if (head[3] < 0 || head[3] > JXL_CANVAS_MAX_PLANES) {
        bad_arg(e, "jxlatte_amd: canvas blend: channel count");
        return 0;
    }
    jint all[12 + 5 * JXL_CANVAS_MAX_PLANES];
    if (!get_ints(e, desc, 12 + 5 * head[3], all)) return 0;
    memset(d, 0, sizeof *d);
    d->canvas = all[0]; d->frame = all[1]; d->ref = all[2]; d->n_chan = all[3];
    d->rect.h = all[4]; d->rect.w = all[5]; d->rect.canvas_y = all[6]; d->rect.canvas_x = all[7];
    d->rect.frame_y = all[8]; d->rect.frame_x = all[9]; d->rect.ref_y = all[10]; d->rect.ref_x = all[11];
    for (int i = 0; i < d->n_chan; i++) {
        const jint* v = all + 12 + 5 * i;
        d->chan[i].frame_plane = v[0]; d->chan[i].mode = v[1]; d->chan[i].flags = (uint32_t)v[2];
        d->chan[i].frame_alpha = v[3]; d->chan[i].ref_alpha = v[4];
    }
    return 1;
}
static int canvas_shape(JNIEnv* e, jintArray a, jxl_canvas_shape* s) {
    jint v[3 + JXL_CANVAS_MAX_PLANES];
    if (!get_ints(e, a, 3, v)) return 0;
    if (v[0] < 1 || v[0] > JXL_CANVAS_MAX_PLANES) {
        bad_arg(e, "jxlatte_amd: canvas shape: plane count");
        return 0;
    }
    if (!get_ints(e, a, 3 + v[0], v)) return 0;
    memset(s, 0, sizeof *s);
    s->n = v[0]; s->h = v[1]; s->w = v[2];
    for (int i = 0; i < s->n; i++) s->types[i] = v[3 + i];
    return 1;
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasCreate(JNIEnv* e, jobject self, jint h, jint w, jintArray types) {
    jxl_ctx* c = ctx_of(e, self);
    jint t[JXL_CANVAS_MAX_PLANES];
    int32_t id = -1;
    const jsize n = types ? (*e)->GetArrayLength(e, types) : 0;
    if (n > JXL_CANVAS_MAX_PLANES) { rethrow(e, NULL, JXL_ERR_UNSUPPORTED); return -1; }
    if (!get_ints(e, types, n, t)) return -1;
    const jxl_status st = jxl_canvas_create(c, n, h, w, (const int32_t*)t, &id);
    if (st != JXL_OK) { rethrow(e, c, st); return -1; }
    return id;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasDestroy(JNIEnv* e, jobject self, jint id) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_canvas_destroy(c, id));
}

JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasDescribe(JNIEnv* e, jobject self, jint id) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_canvas_shape s;
    const jxl_status st = jxl_canvas_describe(c, id, &s);
    if (st != JXL_OK) { rethrow(e, c, st); return NULL; }
    jint v[3 + JXL_CANVAS_MAX_PLANES] = {s.n, s.h, s.w};
    for (int i = 0; i < s.n; i++) v[3 + i] = s.types[i];
    jintArray out = (*e)->NewIntArray(e, 3 + s.n);
    if (out) (*e)->SetIntArrayRegion(e, out, 0, 3 + s.n, v);
    return out;
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasClone(JNIEnv* e, jobject self, jint id) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t nid = -1;
    const jxl_status st = jxl_canvas_clone(c, id, &nid);
    if (st != JXL_OK) { rethrow(e, c, st); return -1; }
    return nid;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasUpload(JNIEnv* e, jobject self, jint id, jint plane, jobject src, jint type) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_canvas_shape s;
    CHECK(jxl_canvas_describe(c, id, &s));
    NEED(src, 4 * area(s.h, s.w));
    CHECK(jxl_canvas_upload(c, id, plane, ADDR(src), type));
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasDownload(JNIEnv* e, jobject self, jint id, jint plane, jobject dst) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_canvas_shape s;
    int32_t type = -1;
    jxl_status st = jxl_canvas_describe(c, id, &s);
    if (st != JXL_OK) { rethrow(e, c, st); return -1; }
    if (!has_room(e, dst, 4 * area(s.h, s.w))) {
        bad_arg(e, "jxlatte_amd: direct buffer dst missing or too small");
        return -1;
    }
    st = jxl_canvas_download(c, id, plane, ADDR(dst), &type);
    if (st != JXL_OK) { rethrow(e, c, st); return -1; }
    return type;
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasFromPlanes(JNIEnv* e, jobject self, jintArray extraTypes) {
    jxl_ctx* c = ctx_of(e, self);
    jint t[JXL_CANVAS_MAX_PLANES];
    int32_t id = -1;
    const jsize n = extraTypes ? (*e)->GetArrayLength(e, extraTypes) : 0;
    if (n > JXL_CANVAS_MAX_PLANES - 3) { rethrow(e, NULL, JXL_ERR_UNSUPPORTED); return -1; }
    if (n > 0 && !get_ints(e, extraTypes, n, t)) return -1;
    const jxl_status st = jxl_canvas_from_planes(c, n, n > 0 ? (const int32_t*)t : NULL, &id);
    if (st != JXL_OK) { rethrow(e, c, st); return -1; }
    return id;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasCast(JNIEnv* e, jobject self, jint id, jint plane, jint depth) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_canvas_cast(c, id, plane, depth));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasBlend(JNIEnv* e, jobject self, jintArray desc) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_canvas_blend_desc d;
    if (!canvas_desc(e, desc, &d)) return;
    CHECK(jxl_canvas_blend(c, &d));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasToPlanes(JNIEnv* e, jobject self, jint id) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_canvas_to_planes(c, id));
}

/* desc: {height, width, nPlanes, then per plane {channel, addChannel, type}}; scales: one float per plane. 0: an exception is pending */
static int modular_planes_desc(JNIEnv* e, jintArray desc, jfloatArray scales, jxl_modular_planes_desc* d) {
    jint head[3];
    if (!get_ints(e, desc, 3, head)) return 0;
    if (head[2] > JXL_CANVAS_MAX_PLANES) { rethrow(e, NULL, JXL_ERR_UNSUPPORTED); return 0; }
    if (head[2] < 1) { bad_arg(e, "jxlatte_amd: modular planes: plane count"); return 0; }
    jint all[3 + 3 * JXL_CANVAS_MAX_PLANES];
    float sc[JXL_CANVAS_MAX_PLANES];
    if (!get_ints(e, desc, 3 + 3 * head[2], all) || !get_floats(e, scales, head[2], sc)) return 0;
    memset(d, 0, sizeof *d);
    d->height = all[0]; d->width = all[1]; d->n_planes = all[2];
    for (int i = 0; i < d->n_planes; i++) {
        const jint* v = all + 3 + 3 * i;
        d->plane[i].channel = v[0]; d->plane[i].add_channel = v[1]; d->plane[i].type = v[2]; d->plane[i].scale = sc[i];
    }
    return 1;
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasFromModular(JNIEnv* e, jobject self, jintArray desc, jfloatArray scales) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t id = -1;
    jxl_modular_planes_desc d;
    if (!modular_planes_desc(e, desc, scales, &d)) return -1;
    const jxl_status st = jxl_canvas_from_modular(c, &d, &id);
    if (st != JXL_OK) { rethrow(e, c, st); return -1; }
    return id;
}

/* weights: k * k * 25 floats (jxl_upsampling_weights); a k the library refuses is handed on without them */
JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasFromModularUp(JNIEnv* e, jobject self, jintArray desc, jfloatArray scales,
        jint k, jfloatArray weights) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t id = -1;
    jxl_modular_planes_desc d;
    float w[8 * 8 * 25];
    if (!modular_planes_desc(e, desc, scales, &d)) return -1;
    const int known = k == 2 || k == 4 || k == 8;
    if (known && !get_floats(e, weights, k * k * 25, w)) return -1;
    const jxl_status st = jxl_canvas_from_modular_up(c, &d, k, known ? w : NULL, &id);
    if (st != JXL_OK) { rethrow(e, c, st); return -1; }
    return id;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasTakePlanes(JNIEnv* e, jobject self, jint id) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_canvas_take_planes(c, id));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasOrient(JNIEnv* e, jobject self, jint id, jint orientation) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_canvas_orient(c, id, orientation));
}

/* the writers on a set: height and width must be the set's and the type flags its tags (the library checks) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasPngSamples(JNIEnv* e, jobject self, jint id, jint alphaPlane,
        jobject params, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_png_params p;
    if (!png_params(e, params, &p)) return;
    NEED(out, png_bytes(c, &p));
    CHECK(jxl_canvas_png_samples(c, id, alphaPlane, &p, ADDR(out)));
}

JNIEXPORT jfloat JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasColorPeak(JNIEnv* e, jobject self, jint id, jobject params) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_color_params p;
    float peak = 0.0f;
    if (!color_params(e, params, &p)) return 0.0f;
    jxl_status st = jxl_canvas_color_peak(c, id, &p, &peak);
    if (st != JXL_OK) { rethrow(e, c, st); return 0.0f; }
    return peak;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasPfmSamples(JNIEnv* e, jobject self, jint id, jintArray params, jobject out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_pfm_params p;
    if (!pfm_params(e, params, &p)) return;
    if (!pfm_out_fits(e, out, 4 * area(p.height, p.width) * p.n_planes)) return;
    CHECK(jxl_canvas_pfm_samples(c, id, &p, ADDR(out)));
}

/* ---- the image as a device tensor in one pass: params = struct jxl_tensor_params in a direct buffer, as the PNG natives take
 * theirs; out = the DEVICE address of the tensor (a long: there is no buffer object for memory the host cannot read). The shim can
 * check the host planes' sizes; whether `out` is device memory that holds the tensor is the library's question. ---- */
static int tensor_params(JNIEnv* e, jobject params, jxl_tensor_params* p) {
    const void* src = params ? (*e)->GetDirectBufferAddress(e, params) : NULL;
    if (!src || (*e)->GetDirectBufferCapacity(e, params) < (jlong)sizeof *p) {
        bad_arg(e, "jxlatte_amd: a direct buffer holding jxl_tensor_params is needed");
        return 0;
    }
    memcpy(p, src, sizeof *p);
    if (p->height < 1 || p->width < 1) {
        bad_arg(e, "jxlatte_amd: tensor parameters");
        return 0;
    }
    return 1;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageTensorSamples(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jobject alpha, jobject params, jlong out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_tensor_params p;
    if (!tensor_params(e, params, &p)) return;
    const jlong plane = 4 * area(p.height, p.width);
    NEED(i0, plane); NEED_OPT(i1, plane); NEED_OPT(i2, plane); NEED_OPT(alpha, plane);
    const void* in[3] = {ADDR(i0), ADDR(i1), ADDR(i2)};
    CHECK(jxl_stage_tensor_samples(c, in, ADDR(alpha), &p, (void*)(intptr_t)out));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesTensorSamples(JNIEnv* e, jobject self, jobject alpha, jobject params,
        jlong out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_tensor_params p;
    if (!tensor_params(e, params, &p)) return;
    NEED_OPT(alpha, 4 * area(p.height, p.width));
    CHECK(jxl_planes_tensor_samples(c, ADDR(alpha), &p, (void*)(intptr_t)out));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasTensorSamples(JNIEnv* e, jobject self, jint id, jint alphaPlane,
        jobject params, jlong out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_tensor_params p;
    if (!tensor_params(e, params, &p)) return;
    CHECK(jxl_canvas_tensor_samples(c, id, alphaPlane, &p, (void*)(intptr_t)out));
}

/* ---- the image resampled to a device tensor in one pass: the tensor natives with struct jxl_resize_params in a second direct
 * buffer. params->height / width stay the SOURCE planes' size (what the shim checks the host planes against); the tensor at `out`
 * is out_height x out_width. ---- */
static int resize_params(JNIEnv* e, jobject resize, jxl_resize_params* r) {
    const void* src = resize ? (*e)->GetDirectBufferAddress(e, resize) : NULL;
    if (!src || (*e)->GetDirectBufferCapacity(e, resize) < (jlong)sizeof *r) {
        bad_arg(e, "jxlatte_amd: a direct buffer holding jxl_resize_params is needed");
        return 0;
    }
    memcpy(r, src, sizeof *r);
    if (r->out_height < 1 || r->out_width < 1 || r->box_width < 1 || r->box_height < 1) {
        bad_arg(e, "jxlatte_amd: resize parameters");
        return 0;
    }
    return 1;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageTensorResized(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jobject alpha, jobject params, jobject resize, jlong out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_tensor_params p;
    jxl_resize_params r;
    if (!tensor_params(e, params, &p) || !resize_params(e, resize, &r)) return;
    const jlong plane = 4 * area(p.height, p.width);
    NEED(i0, plane); NEED_OPT(i1, plane); NEED_OPT(i2, plane); NEED_OPT(alpha, plane);
    const void* in[3] = {ADDR(i0), ADDR(i1), ADDR(i2)};
    CHECK(jxl_stage_tensor_resized(c, in, ADDR(alpha), &p, &r, (void*)(intptr_t)out));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesTensorResized(JNIEnv* e, jobject self, jobject alpha, jobject params,
        jobject resize, jlong out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_tensor_params p;
    jxl_resize_params r;
    if (!tensor_params(e, params, &p) || !resize_params(e, resize, &r)) return;
    NEED_OPT(alpha, 4 * area(p.height, p.width));
    CHECK(jxl_planes_tensor_resized(c, ADDR(alpha), &p, &r, (void*)(intptr_t)out));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasTensorResized(JNIEnv* e, jobject self, jint id, jint alphaPlane,
        jobject params, jobject resize, jlong out) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_tensor_params p;
    jxl_resize_params r;
    if (!tensor_params(e, params, &p) || !resize_params(e, resize, &r)) return;
    CHECK(jxl_canvas_tensor_resized(c, id, alphaPlane, &p, &r, (void*)(intptr_t)out));
}

/* ---- N images into one batch tensor in one launch: the items of jxl_tensor_resized_batch packed from arrays. heads: three ints
 * per item (source, set id, alpha plane); params / resize: n jxl_tensor_params / jxl_resize_params back to back in direct buffers;
 * the host planes of all items lie in ONE direct buffer `planes`, offsets: four longs per item (the byte offsets of its three
 * colour planes and its alpha plane there, -1: none). The shim checks that every plane an item names lies inside `planes` with
 * its item's height * width samples; `planes` may be null when no item names one. ---- */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_tensorResizedBatch(JNIEnv* e, jobject self, jintArray heads, jobject planes,
        jlongArray offsets, jobject params, jobject resize, jlong out) {
    jxl_ctx* c = ctx_of(e, self);
    if (!heads || !offsets) {
        bad_arg(e, "jxlatte_amd: tensorResizedBatch takes three ints and four longs per item");
        return;
    }
    const jsize len = (*e)->GetArrayLength(e, heads);
    const jsize n = len / 3;
    if (len % 3 || n < 1 || n > JXL_TENSOR_BATCH_MAX || (*e)->GetArrayLength(e, offsets) != 4 * n) {
        bad_arg(e, "jxlatte_amd: tensorResizedBatch takes three ints and four longs per item");
        return;
    }
    NEED(params, (jlong)n * (jlong)sizeof(jxl_tensor_params));
    NEED(resize, (jlong)n * (jlong)sizeof(jxl_resize_params));
    const char* base = (const char*)ADDR(planes);
    const jlong room = base ? (*e)->GetDirectBufferCapacity(e, planes) : 0;
    const char* ps = (const char*)ADDR(params);
    const char* rs = (const char*)ADDR(resize);
    jxl_tensor_batch_item* items = (jxl_tensor_batch_item*)calloc((size_t)n, sizeof *items);
    jint* hd = (jint*)malloc((size_t)len * sizeof(jint));
    jlong* off = (jlong*)malloc((size_t)n * 4 * sizeof(jlong));
    int ok = items && hd && off;
    if (!ok) (*e)->ThrowNew(e, (*e)->FindClass(e, "java/lang/OutOfMemoryError"), "jxlatte_amd: batch items");
    if (ok) {
        (*e)->GetIntArrayRegion(e, heads, 0, len, hd);
        (*e)->GetLongArrayRegion(e, offsets, 0, 4 * n, off);
        ok = !(*e)->ExceptionCheck(e);
    }
    for (jsize i = 0; ok && i < n; i++) {
        jxl_tensor_batch_item* it = &items[i];
        it->source = hd[3 * i], it->set_id = hd[3 * i + 1], it->alpha_plane = hd[3 * i + 2];
        memcpy(&it->p, ps + (size_t)i * sizeof it->p, sizeof it->p);
        memcpy(&it->r, rs + (size_t)i * sizeof it->r, sizeof it->r);
        if (it->p.height < 1 || it->p.width < 1 || it->r.out_height < 1 || it->r.out_width < 1 || it->r.box_width < 1 || it->r.box_height < 1) {
            bad_arg(e, "jxlatte_amd: tensor or resize parameters of a batch item");
            ok = 0;
            break;
        }
        const jlong plane = 4 * area(it->p.height, it->p.width);
        for (int k = 0; k < 4; k++) {
            const jlong o = off[4 * i + k];
            if (o == -1) continue;
            if (o < 0 || plane > room || o > room - plane) {
                bad_arg(e, "jxlatte_amd: a plane of a batch item lies outside the planes buffer");
                ok = 0;
                break;
            }
            if (k < 3) it->in[k] = base + o;
            else it->alpha = base + o;
        }
    }
    jxl_status st = JXL_OK;
    if (ok) st = jxl_tensor_resized_batch(c, (int32_t)n, items, (void*)(intptr_t)out);
    free(items);
    free(hd);
    free(off);
    if (ok) CHECK(st);
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasBlendCheck(JNIEnv* e, jclass k, jintArray desc, jintArray canvas,
        jintArray frame, jintArray ref) {
    (void)k;
    jxl_canvas_blend_desc d;
    jxl_canvas_shape sc, sf, sr;
    if (!canvas_desc(e, desc, &d) || !canvas_shape(e, canvas, &sc) || !canvas_shape(e, frame, &sf)) return;
    if (ref && !canvas_shape(e, ref, &sr)) return;
    const jxl_status st = jxl_canvas_blend_check(&d, &sc, &sf, ref ? &sr : NULL);
    if (st != JXL_OK) rethrow(e, NULL, st);
}

/* items: 3 ints per plane {set, plane, depth} (jxl_canvas_cast_item word for word) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasCastPlanes(JNIEnv* e, jobject self, jintArray items) {
    jxl_ctx* c = ctx_of(e, self);
    jint v[3 * 5 * JXL_CANVAS_MAX_PLANES];
    jxl_canvas_cast_item it[5 * JXL_CANVAS_MAX_PLANES];
    const jsize n = items ? (*e)->GetArrayLength(e, items) : -1;
    if (n < 0 || n % 3) { bad_arg(e, "jxlatte_amd: canvas cast: 3 ints per item"); return; }
    if (n > 3 * 5 * JXL_CANVAS_MAX_PLANES) { bad_arg(e, "jxlatte_amd: canvas cast: more than 80 planes in one call"); return; }
    if (n > 0 && !get_ints(e, items, n, v)) return;
    for (int i = 0; i < n / 3; i++) it[i].set = v[3 * i], it[i].plane = v[3 * i + 1], it[i].depth = v[3 * i + 2];
    CHECK(jxl_canvas_cast_planes(c, n / 3, it));
}

/* computePatches on plane sets (jxl_canvas_patches): refSet = 4 set ids (-1: absent); the patch arrays as for stagePatches, without
 * the slot sizes (the library reads them from the sets) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasPatches(JNIEnv* e, jobject self, jint frameSet, jint colorsResident,
        jintArray refSet, jintArray pos, jintArray blend, jint nColor, jintArray ecIsAlpha, jintArray ecAlphaAssociated) {
    jxl_ctx* c = ctx_of(e, self);
    jint ids[4];
    if (!refSet || (*e)->GetArrayLength(e, refSet) != 4) { bad_arg(e, "jxlatte_amd: canvas patches: 4 reference set ids"); return; }
    GETI(refSet, 4, ids);
    jxl_patch_desc d;
    jint* mem = patch_desc0(e, pos, blend, nColor, ecIsAlpha, ecAlphaAssociated, NULL, 0, &d);
    if (!mem) return;
    const jxl_status st = jxl_canvas_patches(c, &d, frameSet, colorsResident, (const int32_t*)ids);
    free(mem);
    CHECK(st);
}

/* jxl_canvas_patches_check (host only). frame: {n, h, w, types...}; refs: 4 x 19 ints, per slot {n, h, w, types[16]} with n == 0 for
 * an absent slot and n == -1 for a slot that is the frame set itself */
JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_canvasPatchesCheck(JNIEnv* e, jclass k, jintArray frame, jint colorsResident,
        jintArray refs, jintArray pos, jintArray blend, jint nColor, jintArray ecIsAlpha, jintArray ecAlphaAssociated) {
    (void)k;
    enum { SLOT = 3 + JXL_CANVAS_MAX_PLANES };
    jxl_canvas_shape sf, sr[4];
    const jxl_canvas_shape* rp[4];
    jint v[4 * SLOT];
    if (!canvas_shape(e, frame, &sf)) return -1;
    if (!refs || (*e)->GetArrayLength(e, refs) != 4 * SLOT) { bad_arg(e, "jxlatte_amd: canvas patches: 4 x 19 ints of reference shapes"); return -1; }
    if (!get_ints(e, refs, 4 * SLOT, v)) return -1;
    for (int s = 0; s < 4; s++) {
        const jint* q = v + s * SLOT;
        if (q[0] < -1 || q[0] > JXL_CANVAS_MAX_PLANES) { bad_arg(e, "jxlatte_amd: canvas shape: plane count"); return -1; }
        memset(&sr[s], 0, sizeof sr[s]);
        sr[s].n = q[0]; sr[s].h = q[1]; sr[s].w = q[2];
        for (int i = 0; i < q[0]; i++) sr[s].types[i] = q[3 + i];
        rp[s] = q[0] == 0 ? NULL : q[0] == -1 ? &sf : &sr[s];
    }
    jxl_patch_desc d;
    jint* mem = patch_desc0(e, pos, blend, nColor, ecIsAlpha, ecAlphaAssociated, NULL, 0, &d);
    if (!mem) return -1;
    int32_t bad = -1;
    const jxl_status st = jxl_canvas_patches_check(&d, &sf, colorsResident, rp, &bad);
    free(mem);
    if (st != JXL_OK) {  /* (the reason is the library's: "Patch too large", ...) */
        const char* cls = st == JXL_ERR_INVALID_BITSTREAM ? "com/traneptora/jxlatte/io/InvalidBitstreamException"
                        : st == JXL_ERR_UNSUPPORTED       ? "java/lang/UnsupportedOperationException"
                        : st == JXL_ERR_OOM               ? "java/lang/OutOfMemoryError"
                                                          : "java/lang/IllegalArgumentException";
        (*e)->ThrowNew(e, (*e)->FindClass(e, cls), jxl_last_error(NULL));
    }
    return bad;
}

/* ---- the varblock map drawn onto the picture (Frame.drawVarblocks, Frame.java:464-503; jxl_stage_varblocks,
 * jxl_planes_varblocks). blocks: nBlocks x (cy, cx, type) in frame cells, copied before the library sees it: the array must hold
 * at least 3 * nBlocks ints. Returns the copy (free it; a one-int allocation for an empty list), NULL with an exception
 * pending on failure. ---- */
static jint* varblock_desc(JNIEnv* e, jintArray blocks, jint nBlocks, jint cellsH, jint cellsW, jxl_varblock_desc* d) {
    if (!blocks || nBlocks < 0 || (jlong)(*e)->GetArrayLength(e, blocks) < 3 * (jlong)nBlocks) {
        bad_arg(e, "jxlatte_amd: varblock list missing or shorter than 3 * nBlocks");
        return NULL;
    }
    jint* mem = (jint*)malloc(sizeof(jint) * (3 * (size_t)nBlocks + 1));
    if (!mem) {
        (*e)->ThrowNew(e, (*e)->FindClass(e, "java/lang/OutOfMemoryError"), "jxlatte_amd: varblock list");
        return NULL;
    }
    (*e)->GetIntArrayRegion(e, blocks, 0, 3 * nBlocks, mem);
    if ((*e)->ExceptionCheck(e)) {
        free(mem);
        return NULL;
    }
    d->n_blocks = nBlocks;
    d->blocks = (const int32_t*)mem;
    d->cells_h = cellsH;
    d->cells_w = cellsW;
    return mem;
}

/* on three host planes of height x width floats; o0..o2 receive the result (they may be the input buffers) */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_stageVarblocks(JNIEnv* e, jobject self, jobject i0, jobject i1, jobject i2,
        jint h, jint w, jintArray blocks, jint nBlocks, jint cellsH, jint cellsW, jobject o0, jobject o1, jobject o2) {
    jxl_ctx* c = ctx_of(e, self);
    if (h < 1 || w < 1) { bad_arg(e, "jxlatte_amd: plane size"); return; }
    const jlong plane = 4 * area(h, w);
    NEED(i0, plane); NEED(i1, plane); NEED(i2, plane);
    NEED(o0, plane); NEED(o1, plane); NEED(o2, plane);
    const float* in[3] = {(const float*)ADDR(i0), (const float*)ADDR(i1), (const float*)ADDR(i2)};
    float* out[3] = {(float*)ADDR(o0), (float*)ADDR(o1), (float*)ADDR(o2)};
    jxl_varblock_desc d;
    jint* mem = varblock_desc(e, blocks, nBlocks, cellsH, cellsW, &d);
    if (!mem) return;
    const jxl_status st = jxl_stage_varblocks(c, in, h, w, &d, out);
    free(mem);
    CHECK(st);
}

/* the same on the resident planes, in place, after planesXyb / planesYcbcr */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_planesVarblocks(JNIEnv* e, jobject self, jintArray blocks, jint nBlocks,
        jint cellsH, jint cellsW) {
    jxl_ctx* c = ctx_of(e, self);
    jxl_varblock_desc d;
    jint* mem = varblock_desc(e, blocks, nBlocks, cellsH, cellsW, &d);
    if (!mem) return;
    const jxl_status st = jxl_planes_varblocks(c, &d);
    free(mem);
    CHECK(st);
}

/* ---- Modular: plan once, run, read channel by channel (ModularStream.applyTransforms, ModularStream.java:110-131) ---- */
JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularDefaultSqueezeParams(JNIEnv* e, jclass k, jintArray widths,
        jintArray heights, jint nbMeta) {
    (void)k;
    const jsize n = (*e)->GetArrayLength(e, widths);
    jint w[256], h[256];
    jxl_squeeze_param sp[64];
    if (n > 256) { rethrow(e, NULL, JXL_ERR_INVALID_ARGUMENT); return NULL; }
    if (!get_ints(e, widths, n, w) || !get_ints(e, heights, n, h)) return NULL;
    const int32_t cnt = jxl_modular_default_squeeze_params((const int32_t*)w, (const int32_t*)h, n, nbMeta, sp, 64);
    if (cnt < 0) { rethrow(e, NULL, (jxl_status)cnt); return NULL; }
    jintArray out = (*e)->NewIntArray(e, cnt * 4);
    for (int32_t i = 0; out && i < cnt; i++) {
        const jint v[4] = {sp[i].horizontal, sp[i].in_place, sp[i].begin_c, sp[i].num_c};
        (*e)->SetIntArrayRegion(e, out, i * 4, 4, v);
    }
    return out;
}

/* returns {w0, h0, w1, h1, ...} of the channel list after the forward bookkeeping of the squeeze steps */
JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularSqueezedShapes(JNIEnv* e, jclass k, jintArray widths,
        jintArray heights, jintArray squeezeParams) {
    (void)k;
    const jsize n = (*e)->GetArrayLength(e, widths), n_sp = (*e)->GetArrayLength(e, squeezeParams) / 4;
    jint w[256], h[256], spv[256];
    int32_t ow[1024], oh[1024];
    jxl_squeeze_param sp[64];
    if (n > 256 || n_sp > 64) { rethrow(e, NULL, JXL_ERR_INVALID_ARGUMENT); return NULL; }
    if (!get_ints(e, widths, n, w) || !get_ints(e, heights, n, h) || !get_ints(e, squeezeParams, n_sp * 4, spv)) return NULL;
    for (jsize i = 0; i < n_sp; i++) {
        sp[i].horizontal = spv[4 * i]; sp[i].in_place = spv[4 * i + 1]; sp[i].begin_c = spv[4 * i + 2]; sp[i].num_c = spv[4 * i + 3];
    }
    const int32_t cnt = jxl_modular_squeezed_shapes((const int32_t*)w, (const int32_t*)h, n, sp, n_sp, ow, oh, 1024);
    if (cnt < 0) { rethrow(e, NULL, (jxl_status)cnt); return NULL; }
    jintArray out = (*e)->NewIntArray(e, cnt * 2);
    for (int32_t i = 0; out && i < cnt; i++) {
        const jint v[2] = {ow[i], oh[i]};
        (*e)->SetIntArrayRegion(e, out, i * 2, 2, v);
    }
    return out;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularBegin(JNIEnv* e, jobject self, jobjectArray chans, jintArray widths,
        jintArray heights, jintArray squeezeParams, jint rctType, jint rctBegin) {
    jxl_ctx* c = ctx_of(e, self);
    const jsize n = (*e)->GetArrayLength(e, chans), n_sp = (*e)->GetArrayLength(e, squeezeParams) / 4;
    if (n > 256 || n_sp > 64) {
        rethrow(e, c, JXL_ERR_INVALID_ARGUMENT);
        return;
    }
    jxl_channel ci[256];
    jxl_squeeze_param sp[64];
    jint w[256], h[256], spv[256];
    GETI(widths, n, w);
    GETI(heights, n, h);
    GETI(squeezeParams, n_sp * 4, spv);
    for (jsize i = 0; i < n; i++) {
        jobject b = (*e)->GetObjectArrayElement(e, chans, i);
        if ((*e)->ExceptionCheck(e)) return;
        ci[i].width = w[i]; ci[i].height = h[i];
        if (area(h[i], w[i]) > 0) NEED(b, 4 * area(h[i], w[i]));  /* (an empty channel may come without a buffer) */
        ci[i].data = (int32_t*)ADDR(b);
    }
    for (jsize i = 0; i < n_sp; i++) {
        sp[i].horizontal = spv[4 * i]; sp[i].in_place = spv[4 * i + 1]; sp[i].begin_c = spv[4 * i + 2]; sp[i].num_c = spv[4 * i + 3];
    }
    CHECK(jxl_modular_begin(c, ci, n, sp, n_sp, rctType, rctBegin));
}

/* transforms: 8 ints per transform in bitstream order -- kind, begin_c, num_c, rct_type, nb_colors, nb_deltas, d_pred, n_sp;
 * squeezeSteps: the expanded steps of every Squeeze, 4 ints each, back to back in the order of the transforms */
JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularBeginChain(JNIEnv* e, jobject self, jobjectArray chans,
        jintArray widths, jintArray heights, jintArray transforms, jintArray squeezeSteps, jint bitDepth) {
    jxl_ctx* c = ctx_of(e, self);
    const jsize n = (*e)->GetArrayLength(e, chans), n_tr = (*e)->GetArrayLength(e, transforms) / 8;
    const jsize n_sp = (*e)->GetArrayLength(e, squeezeSteps) / 4;
    if (n > 256 || n_tr > 64 || n_sp > 256) {
        rethrow(e, c, JXL_ERR_INVALID_ARGUMENT);
        return;
    }
    jxl_channel ci[256];
    jxl_modular_transform tr[64];
    jxl_squeeze_param sp[256];
    jint w[256], h[256], trv[512], spv[1024];
    GETI(widths, n, w);
    GETI(heights, n, h);
    GETI(transforms, n_tr * 8, trv);
    GETI(squeezeSteps, n_sp * 4, spv);
    for (jsize i = 0; i < n; i++) {
        jobject b = (*e)->GetObjectArrayElement(e, chans, i);
        if ((*e)->ExceptionCheck(e)) return;
        ci[i].width = w[i]; ci[i].height = h[i];
        if (area(h[i], w[i]) > 0) NEED(b, 4 * area(h[i], w[i]));  /* (an empty channel may come without a buffer) */
        ci[i].data = (int32_t*)ADDR(b);
    }
    for (jsize i = 0; i < n_sp; i++) {
        sp[i].horizontal = spv[4 * i]; sp[i].in_place = spv[4 * i + 1]; sp[i].begin_c = spv[4 * i + 2]; sp[i].num_c = spv[4 * i + 3];
    }
    jsize at = 0;
    for (jsize i = 0; i < n_tr; i++) {
        const jint* v = trv + 8 * i;
        tr[i].kind = v[0]; tr[i].begin_c = v[1]; tr[i].num_c = v[2]; tr[i].rct_type = v[3];
        tr[i].nb_colors = v[4]; tr[i].nb_deltas = v[5]; tr[i].d_pred = v[6]; tr[i].n_sp = v[7];
        if (v[7] < 0 || v[7] > n_sp - at) {  /* the steps a transform counts are not in squeezeSteps */
            rethrow(e, c, JXL_ERR_INVALID_ARGUMENT);
            return;
        }
        tr[i].sp = sp + at;
        at += v[7];
    }
    CHECK(jxl_modular_begin_chain(c, ci, n, tr, n_tr, bitDepth));
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularRun(JNIEnv* e, jobject self) {
    jxl_ctx* c = ctx_of(e, self);
    CHECK(jxl_modular_run(c));
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularOutCount(JNIEnv* e, jobject self) {
    return jxl_modular_out_count(ctx_of(e, self));
}

JNIEXPORT jintArray JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularOutShape(JNIEnv* e, jobject self, jint idx) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t wh[2] = {0, 0};
    const jxl_status st = jxl_modular_out_shape(c, idx, &wh[0], &wh[1]);
    if (st != JXL_OK) { rethrow(e, c, st); return NULL; }
    jintArray out = (*e)->NewIntArray(e, 2);
    if (out) (*e)->SetIntArrayRegion(e, out, 0, 2, (const jint*)wh);
    return out;
}

JNIEXPORT void JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularReadChannel(JNIEnv* e, jobject self, jint idx, jobject dst) {
    jxl_ctx* c = ctx_of(e, self);
    int32_t cw = 0, chh = 0;
    CHECK(jxl_modular_out_shape(c, idx, &cw, &chh));
    NEED(dst, 4 * area(chh, cw));
    CHECK(jxl_modular_read_channel(c, idx, (int32_t*)ADDR(dst)));
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularLastLaunchCount(JNIEnv* e, jobject self) {
    return jxl_modular_last_launch_count(ctx_of(e, self));
}

JNIEXPORT jint JNICALL Java_com_traneptora_jxlatte_gpu_NativeBackend_modularRedoCount(JNIEnv* e, jobject self) {
    return jxl_modular_redo_count(ctx_of(e, self));
}
