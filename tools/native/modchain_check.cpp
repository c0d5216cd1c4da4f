// Stand-alone host check of jxlatte_amd/csrc/modchain_check.h (no device, no context), meant for an AddressSanitizer + UBSan
// build (tests/test_modchain_cpu.py):
//   * runs chain_plan over what jxl_modular_begin_chain refuses, one line each ("REFUSAL <name> <status> ok" / "FAIL ...")
//   * with a case file as argv[1] and an output file as argv[2]: builds every case's plan and runs it with host loops -- a Palette
//     stage in the reference's order over palette_value and palette_predict (palette_ops.h), an RCT and a Squeeze step as
//     ModularStream.java:229-326 and ModularChannel.java:23-47, 361-413 write them -- and writes the channel list of every case.
//     Every fusable Palette run is also evaluated through its path table, as k_palette_run does it; where the run has no pixel
//     that needs a neighbour, the two must agree. One line per run: "RUN <case> <stages> <fusable> <outputs> <impure pixels>".
// Case file (raw int32, native byte order): the case count, then per case bit_depth, n_chans, n_tr; per channel w, h and its
// w * h samples; per transform kind, begin_c, num_c, rct_type, nb_colors, nb_deltas, d_pred, n_sp and n_sp steps of horizontal,
// in_place, begin_c, num_c. Output per case: the channel count, then per channel w, h and the samples.
// Every buffer is an allocation of exactly its size, so a read past one is the sanitizer's to find.
// Ends with "<n> case(s)" and "<n> failure(s)".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../jxlatte_amd/csrc/modchain_check.h"
#include "../../jxlatte_amd/csrc/palette_ops.h"

using namespace jxl;

static int failures = 0;

// ---- the refusals ----
static void refusal(const char* name, const jxl_channel* ch, int n_ch, const jxl_modular_transform* tr, int n_tr, int bit_depth, int want) {
    ChainPlan p;
    const char* bad = chain_plan(ch, n_ch, tr, n_tr, bit_depth, &p);
    if (bad && p.status == want) {
        printf("REFUSAL %s %d ok\n", name, p.status);
    } else {
        printf("FAIL: %s: %s (status %d, wanted %d)\n", name, bad ? bad : "accepted", p.status, want);
        failures++;
    }
}

static jxl_modular_transform palette(int begin_c, int num_c, int nb_colors, int nb_deltas, int d_pred) {
    jxl_modular_transform t{};
    t.kind = JXL_TRANSFORM_PALETTE;
    t.begin_c = begin_c;
    t.num_c = num_c;
    t.nb_colors = nb_colors;
    t.nb_deltas = nb_deltas;
    t.d_pred = d_pred;
    return t;
}

static void refusals() {
    std::vector<int32_t> pal(3 * 5, 0), a(2 * 3, 0), b(2 * 3, 0), c(2 * 3, 0), odd(2 * 4, 0);
    const jxl_channel good[4] = {{5, 3, pal.data()}, {3, 2, a.data()}, {3, 2, b.data()}, {3, 2, c.data()}};
    const int A = JXL_ERR_INVALID_ARGUMENT, B = JXL_ERR_INVALID_BITSTREAM;
    jxl_modular_transform t = palette(0, 3, 5, 1, 2);
    {
        ChainPlan p;
        const char* bad = chain_plan(good, 4, &t, 1, 8, &p);
        if (bad || p.list.size() != 5 || p.ops.size() != 1 || !p.ops[0].fusable) {
            printf("FAIL: a good chain was refused or misplanned: %s\n", bad ? bad : "plan");
            failures++;
        }
    }
    refusal("null_channels", nullptr, 4, &t, 1, 8, A);
    refusal("null_transforms", good, 4, nullptr, 1, 8, A);
    refusal("negative_n_chans", good, -1, &t, 1, 8, A);
    refusal("negative_n_tr", good, 4, &t, -1, 8, A);
    {
        jxl_channel ch[4] = {good[0], good[1], good[2], good[3]};
        ch[2].width = -3;
        refusal("negative_channel_size", ch, 4, &t, 1, 8, A);
        ch[2] = good[2];
        ch[2].data = nullptr;
        refusal("channel_without_data", ch, 4, &t, 1, 8, A);
        ch[2] = jxl_channel{65536, 32768, b.data()};
        refusal("channel_too_many_samples", ch, 4, &t, 1, 8, A);
    }
    t.kind = 3;
    refusal("unknown_kind", good, 4, &t, 1, 8, A);
    t.kind = -1;
    refusal("negative_kind", good, 4, &t, 1, 8, A);
    // everything palette_check.h refuses for one transform, the sizes being the channels' at that point
    t = palette(0, 0, 5, 1, 2);
    refusal("palette_num_c_0", good, 4, &t, 1, 8, A);
    t = palette(0, -1, 5, 1, 2);
    refusal("palette_num_c_negative", good, 4, &t, 1, 8, A);
    t = palette(0, INT32_MAX, 5, 1, 2);
    refusal("palette_num_c_max", good, 4, &t, 1, 8, A);
    t = palette(0, 4, 5, 1, 2);
    refusal("palette_pal_h_below_num_c", good, 4, &t, 1, 8, A);
    t = palette(0, 3, 6, 1, 2);
    refusal("palette_pal_w_below_nb_colors", good, 4, &t, 1, 8, A);
    t = palette(0, 3, -1, 1, 2);
    refusal("palette_nb_colors_negative", good, 4, &t, 1, 8, A);
    t = palette(0, 3, 5, -1, 2);
    refusal("palette_nb_deltas_negative", good, 4, &t, 1, 8, A);
    t = palette(0, 3, 5, 1, -1);
    refusal("palette_d_pred_negative", good, 4, &t, 1, 8, A);
    t = palette(0, 3, 5, 1, 14);
    refusal("palette_d_pred_14", good, 4, &t, 1, 8, A);
    t = palette(0, 3, 5, 1, 2);
    refusal("palette_bit_depth_0", good, 4, &t, 1, 0, A);
    refusal("palette_bit_depth_33", good, 4, &t, 1, 33, A);
    {
        const jxl_channel ch[2] = {good[0], {0, 2, nullptr}};
        refusal("palette_index_without_samples", ch, 2, &t, 1, 8, A);
    }
    t = palette(0, 3, 5, 1, 6);
    refusal("palette_weighted_deltas", good, 4, &t, 1, 8, JXL_ERR_UNSUPPORTED);
    t = palette(0, 3, 5, 0, 6);  // no positive delta index can name the plane: accepted (a negative index then adds 0)
    {
        ChainPlan p;
        if (chain_plan(good, 4, &t, 1, 8, &p)) {
            printf("FAIL: d_pred 6 with nb_deltas 0 was refused\n");
            failures++;
        }
    }
    // a Palette whose channels leave the list
    t = palette(-1, 3, 5, 1, 2);
    refusal("palette_begin_c_negative", good, 4, &t, 1, 8, A);
    t = palette(3, 1, 5, 1, 2);
    refusal("palette_index_past_the_list", good, 4, &t, 1, 8, A);
    t = palette(INT32_MAX, 1, 5, 1, 2);
    refusal("palette_begin_c_max", good, 4, &t, 1, 8, A);
    refusal("palette_on_an_empty_list", good, 0, &t, 1, 8, A);
    {  // sizes are the channels' at that point: the second Palette undone finds a 3 x 2 channel where its palette should be
        const jxl_modular_transform two[2] = {palette(0, 1, 4, 0, 0), palette(0, 3, 5, 0, 0)};
        refusal("palette_sizes_at_that_point", good, 2, two, 2, 8, A);
    }
    // RCT
    jxl_modular_transform r{};
    r.kind = JXL_TRANSFORM_RCT;
    r.begin_c = 1;
    r.rct_type = 10;
    {
        ChainPlan p;
        if (chain_plan(good, 4, &r, 1, 8, &p)) {
            printf("FAIL: a good RCT was refused\n");
            failures++;
        }
    }
    r.begin_c = 2;
    refusal("rct_past_the_list", good, 4, &r, 1, 8, A);
    r.begin_c = -1;
    refusal("rct_begin_c_negative", good, 4, &r, 1, 8, A);
    r.begin_c = INT32_MAX;
    refusal("rct_begin_c_max", good, 4, &r, 1, 8, A);
    r.begin_c = 1;
    r.rct_type = 42;
    refusal("rct_type_42", good, 4, &r, 1, 8, A);
    r.rct_type = -1;
    refusal("rct_type_negative", good, 4, &r, 1, 8, A);
    r.rct_type = 10;
    {
        const jxl_channel ch[4] = {good[0], good[1], {4, 2, odd.data()}, good[3]};
        refusal("rct_unequal_sizes", ch, 4, &r, 1, 8, B);
    }
    // Squeeze
    jxl_squeeze_param sp{1, 1, 1, 1};
    jxl_modular_transform s{};
    s.kind = JXL_TRANSFORM_SQUEEZE;
    s.sp = &sp;
    s.n_sp = 1;
    {
        ChainPlan p;
        if (chain_plan(good, 4, &s, 1, 8, &p) || p.list.size() != 3 || p.bufs.back().w != 6) {
            printf("FAIL: a good Squeeze was refused or misplanned\n");
            failures++;
        }
    }
    sp.begin_c = 3;
    refusal("squeeze_residual_past_the_list", good, 4, &s, 1, 8, B);
    sp.begin_c = -1;
    refusal("squeeze_begin_c_negative", good, 4, &s, 1, 8, B);
    sp = jxl_squeeze_param{1, 1, 1, 0};
    refusal("squeeze_num_c_0", good, 4, &s, 1, 8, B);
    sp = jxl_squeeze_param{1, 1, INT32_MAX, INT32_MAX};
    refusal("squeeze_begin_c_max", good, 4, &s, 1, 8, B);
    sp = jxl_squeeze_param{1, 1, 0, 1};
    refusal("squeeze_horizontal_mismatch", good, 4, &s, 1, 8, A);
    sp = jxl_squeeze_param{0, 1, 0, 1};
    refusal("squeeze_vertical_mismatch", good, 4, &s, 1, 8, JXL_ERR_STATE);
    s.sp = nullptr;
    refusal("squeeze_null_steps", good, 4, &s, 1, 8, A);
    s.sp = &sp;
    s.n_sp = -1;
    refusal("squeeze_negative_n_sp", good, 4, &s, 1, 8, A);
}

// ---- the ops on the host ----
typedef std::vector<int32_t> Plane;

// ModularChannel.tendency (ModularChannel.java:23-47)
static int32_t tendency(int32_t a, int32_t b, int32_t c) {
    if (a >= b && b >= c) {
        int32_t x = jadd(jsub(jsub(jmul(4, a), jmul(3, c)), b), 6) / 12;
        const int32_t d = jmul(2, jsub(a, b)), e = jmul(2, jsub(b, c));
        if (jsub(x, x & 1) > d) x = jadd(d, 1);
        if (jadd(x, x & 1) > e) x = e;
        return x;
    }
    if (a <= b && b <= c) {
        int32_t x = jsub(jsub(jsub(jmul(4, a), jmul(3, c)), b), 6) / 12;
        const int32_t d = jmul(2, jsub(a, b)), e = jmul(2, jsub(b, c));
        if (jadd(x, x & 1) < d) x = jsub(d, 1);
        if (jsub(x, x & 1) < e) x = e;
        return x;
    }
    return 0;
}

// one line of the inverse squeeze (:361-413): n_a averages, n_r residuals, element k of an array at [k * stride]
static void unsqueeze_line(const int32_t* avg, int n_a, const int32_t* res, int n_r, int64_t sa, int64_t sr, int32_t* out, int64_t so) {
    for (int x = 0; x < n_r; x++) {
        const int32_t a = avg[x * sa];
        const int32_t next = x + 1 < n_a ? avg[(x + 1) * sa] : a;
        const int32_t left = x > 0 ? out[(2 * x - 1) * so] : a;
        const int32_t diff = jadd(res[x * sr], tendency(left, a, next));
        const int32_t first = jadd(a, diff / 2);
        out[2 * x * so] = first;
        out[(2 * x + 1) * so] = jsub(first, diff);
    }
    if (n_a > n_r) out[2 * (int64_t)n_r * so] = avg[(int64_t)n_r * sa];
}

static void rct_in_place(int32_t* v0, int32_t* v1, int32_t* v2, size_t n, int type) {
    for (size_t i = 0; i < n; i++) {
        const int32_t a = v0[i], b = v1[i], c = v2[i];
        switch (type) {
            case 1: v2[i] = jadd(c, a); break;
            case 2: v1[i] = jadd(b, a); break;
            case 3: v2[i] = jadd(c, a); v1[i] = jadd(b, a); break;
            case 4: v1[i] = jadd(b, jadd(a, c) >> 1); break;
            case 5: {
                const int32_t ac = jadd(a, c);
                v1[i] = jadd(b, jadd(a, ac) >> 1);
                v2[i] = ac;
                break;
            }
            case 6: {
                const int32_t tmp = jsub(a, c >> 1), f = jsub(tmp, b >> 1);
                v0[i] = jadd(f, b);
                v1[i] = jadd(c, tmp);
                v2[i] = f;
                break;
            }
            default: break;
        }
    }
}

static void palette_stage(const ChainPalStage& s, int bit_depth, std::vector<Plane>& buf) {
    const Plane& index = buf[(size_t)s.index];
    const PaletteLookup lk = {buf[(size_t)s.pal].data(), s.pal_w, s.nb_colors, bit_depth};
    for (int32_t c = 0; c < s.num_c; c++) {
        Plane& o = buf[(size_t)(s.out0 + c)];
        for (int32_t y = 0; y < s.h; y++)
            for (int32_t x = 0; x < s.w; x++) {
                const size_t i = (size_t)y * s.w + x;
                int32_t v = palette_value(index[i], c, lk);
                if (index[i] < s.nb_deltas && s.d_pred != 6) v = jadd(v, palette_predict_at(s.d_pred, o.data(), s.w, x, y));
                o[i] = v;
            }
    }
}

// the run through its path table, as k_palette_run walks it; returns the pixels that would have needed a neighbour
static int64_t palette_run_by_table(const ChainPlan& p, const ChainOp& op, int bit_depth, const std::vector<Plane>& buf, std::vector<Plane>* outs) {
    // all palettes back to back, nb_colors apart, as the kernel stages them
    std::vector<int32_t> lds;
    std::vector<int32_t> off;
    for (int32_t k = 0; k < op.n_stage; k++) {
        const ChainPalStage& s = p.stages[(size_t)(op.stage0 + k)];
        off.push_back((int32_t)lds.size());
        for (int32_t c = 0; c < s.num_c; c++)
            for (int32_t j = 0; j < s.nb_colors; j++) lds.push_back(buf[(size_t)s.pal][(size_t)c * s.pal_w + j]);
    }
    lds.shrink_to_fit();
    const Plane& src = buf[(size_t)op.source];
    int64_t impure = 0;
    for (int32_t o = 0; o < op.n_out; o++) {
        const ChainPalOut& po = p.outs[(size_t)(op.out0 + o)];
        Plane out(src.size());
        for (size_t i = 0; i < src.size(); i++) {
            int32_t v = src[i];
            for (int32_t d = 0; d < po.depth; d++) {
                const ChainPalStage& s = p.stages[(size_t)(op.stage0 + po.stage[d])];
                const PaletteLookup lk = {lds.data() + off[(size_t)po.stage[d]], s.nb_colors, s.nb_colors, bit_depth};
                impure += v < s.nb_deltas && !palette_pred_is_local(s.d_pred);
                v = palette_value(v, po.row[d], lk);
            }
            out[i] = v;
        }
        outs->push_back(std::move(out));
    }
    return impure;
}

static bool read_words(FILE* f, std::vector<int32_t>* v, size_t n) {
    v->resize(n);
    v->shrink_to_fit();
    return n == 0 || fread(v->data(), sizeof(int32_t), n, f) == n;
}

static bool run_case(FILE* in, FILE* res, int id) {
    std::vector<int32_t> head;
    if (!read_words(in, &head, 3)) return false;
    const int32_t bit_depth = head[0], n_chans = head[1], n_tr = head[2];
    std::vector<Plane> buf((size_t)n_chans);
    std::vector<jxl_channel> chans((size_t)n_chans);
    for (int32_t i = 0; i < n_chans; i++) {
        if (!read_words(in, &head, 2) || !read_words(in, &buf[(size_t)i], (size_t)head[0] * head[1])) return false;
        chans[(size_t)i] = jxl_channel{head[0], head[1], buf[(size_t)i].data()};
    }
    std::vector<jxl_modular_transform> tr((size_t)n_tr);
    std::vector<std::vector<jxl_squeeze_param>> steps((size_t)n_tr);
    for (int32_t i = 0; i < n_tr; i++) {
        if (!read_words(in, &head, 8)) return false;
        jxl_modular_transform& t = tr[(size_t)i];
        t.kind = head[0]; t.begin_c = head[1]; t.num_c = head[2]; t.rct_type = head[3];
        t.nb_colors = head[4]; t.nb_deltas = head[5]; t.d_pred = head[6]; t.n_sp = head[7];
        std::vector<int32_t> w;
        if (!read_words(in, &w, 4 * (size_t)t.n_sp)) return false;
        for (int32_t j = 0; j < t.n_sp; j++) steps[(size_t)i].push_back(jxl_squeeze_param{w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]});
        steps[(size_t)i].shrink_to_fit();
        t.sp = steps[(size_t)i].data();
    }
    ChainPlan p;
    const char* bad = chain_plan(chans.data(), n_chans, tr.data(), n_tr, bit_depth, &p);
    if (bad) {
        printf("FAIL: case %d refused: %s\n", id, bad);
        failures++;
        const int32_t zero = 0;
        fwrite(&zero, sizeof zero, 1, res);
        return true;
    }
    buf.resize(p.bufs.size());
    for (size_t i = (size_t)n_chans; i < p.bufs.size(); i++) {
        buf[i].assign((size_t)p.bufs[i].w * p.bufs[i].h, 0);
        buf[i].shrink_to_fit();
    }
    for (const ChainOp& op : p.ops) {
        if (op.kind == kChainSqueeze) {
            const ChainBuf a = p.bufs[(size_t)op.avg], r = p.bufs[(size_t)op.res], o = p.bufs[(size_t)op.out];
            if (op.horizontal)
                for (int32_t y = 0; y < a.h; y++)
                    unsqueeze_line(buf[(size_t)op.avg].data() + (size_t)y * a.w, a.w, buf[(size_t)op.res].data() + (size_t)y * r.w, r.w, 1, 1,
                                   buf[(size_t)op.out].data() + (size_t)y * o.w, 1);
            else
                for (int32_t x = 0; x < a.w; x++)
                    unsqueeze_line(buf[(size_t)op.avg].data() + x, a.h, buf[(size_t)op.res].data() + x, r.h, a.w, r.w, buf[(size_t)op.out].data() + x, o.w);
        } else if (op.kind == kChainRct) {
            for (int j = 0; j < 3; j++)
                if (op.dst[j] != op.src[j]) buf[(size_t)op.dst[j]] = buf[(size_t)op.src[j]];
            rct_in_place(buf[(size_t)op.dst[0]].data(), buf[(size_t)op.dst[1]].data(), buf[(size_t)op.dst[2]].data(), buf[(size_t)op.dst[0]].size(), op.type);
        } else {
            std::vector<Plane> by_table;
            int64_t impure = -1;
            if (op.fusable) impure = palette_run_by_table(p, op, bit_depth, buf, &by_table);
            for (int32_t k = 0; k < op.n_stage; k++) palette_stage(p.stages[(size_t)(op.stage0 + k)], bit_depth, buf);
            printf("RUN %d %d %d %d %lld\n", id, op.n_stage, op.fusable ? 1 : 0, op.n_out, (long long)impure);
            if (impure == 0)
                for (int32_t o = 0; o < op.n_out; o++)
                    if (by_table[(size_t)o] != buf[(size_t)p.outs[(size_t)(op.out0 + o)].buf]) {
                        printf("FAIL: case %d: output %d of a pure run differs between the path table and the stages\n", id, o);
                        failures++;
                    }
        }
    }
    const int32_t n_out = (int32_t)p.list.size();
    fwrite(&n_out, sizeof n_out, 1, res);
    for (int32_t b : p.list) {
        const int32_t wh[2] = {p.bufs[(size_t)b].w, p.bufs[(size_t)b].h};
        fwrite(wh, sizeof(int32_t), 2, res);
        if (!buf[(size_t)b].empty() && fwrite(buf[(size_t)b].data(), sizeof(int32_t), buf[(size_t)b].size(), res) != buf[(size_t)b].size()) {
            printf("FAIL: short write\n");
            failures++;
        }
    }
    return true;
}

int main(int argc, char** argv) {
    refusals();
    int cases = 0;
    if (argc > 2) {
        FILE* in = fopen(argv[1], "rb");
        FILE* res = fopen(argv[2], "wb");
        if (!in || !res) {
            printf("FAIL: cannot open %s or %s\n", argv[1], argv[2]);
            return 2;
        }
        std::vector<int32_t> head;
        if (!read_words(in, &head, 1)) return 2;
        const int32_t count = head[0];
        for (; cases < count; cases++)
            if (!run_case(in, res, cases)) break;
        if (cases != count) {
            printf("FAIL: the case file is cut short at case %d\n", cases);
            failures++;
        }
        fclose(in);
        fclose(res);
    }
    printf("%d case(s)\n", cases);
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
