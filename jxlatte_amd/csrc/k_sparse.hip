// Sparse coefficient feed: the quantised HF coefficients as lists of (position, value) entries (include/jxlatte_amd.h,
// "sparse coefficient feed") instead of dense rectangles. The reference's decode loop makes one store per decoded symbol and
// stops at a block's last non-zero (HFCoefficients.java:112-127): about 15 % of a photographic frame's samples. The entries
// cross the bus as they are and this kernel scatters them into the tiled int32 planes (coeff_off, jxl_internal.h).
#include "jxl_internal.h"

namespace jxl {

namespace {

typedef unsigned v4u_ __attribute__((ext_vector_type(4)));

struct SparseArgs {
    SparseGeom g;
    const v4u_* src[3];
    const SparseRec* recs;      // device-visible table of n_recs records, or null: the three inline ones
    SparseRec inl0, inl1, inl2;
    int32_t n_recs;
    uint32_t total_chunks;
    unsigned long long* rejected;
};

// One lane = one 16-byte chunk of a run: four narrow or two wide entries, read with one non-temporal 16-byte load through the
// host buffer's device alias; consecutive lanes read consecutive 16 bytes (the request shape of k_widen2d_host8, for its
// reason: the transfer is made of full-size read requests). The grid is bounded (bus_grid): the kernel waits on the bus, and a
// wave parked on every slot of the chip would starve the other contexts' IDCT / restoration kernels (see k_widen2d_host8).
// The run table is staged in LDS once per workgroup; a lane finds its run by binary search in the chunk prefix sums.
// Every entry ADDS with an integer atomic (Java int wrap): sums over passes, over commits and over duplicate positions are the
// same in whatever order the adds arrive, so the planes are identical on every run (a plain read-modify-write would not be
// with duplicates, and would need the runs of one sample serialised). Entries outside the group's rectangle are not stored;
// each wave adds its count of them to *rejected once, after its last chunk.
__global__ __launch_bounds__(256) void k_sparse_scatter(const SparseArgs a) {
    __shared__ SparseRec recs[kSparseMaxRuns];
    for (int i = threadIdx.x; i < a.n_recs; i += 256) recs[i] = a.recs ? a.recs[i] : (i == 0 ? a.inl0 : i == 1 ? a.inl1 : a.inl2);
    __syncthreads();
    unsigned rej = 0;
    const uint32_t step = gridDim.x * 256u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.total_chunks; i += step) {
        int lo = 0, hi = a.n_recs - 1;  // the last record whose first chunk is <= i (records without chunks are never listed)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (recs[mid].chunk_first <= i) lo = mid;
            else hi = mid - 1;
        }
        const SparseRec r = recs[lo];
        const uint32_t k = i - r.chunk_first;
        const int ch = (r.where >> 24) & 3, sel = (r.where >> 26) & 3;
        const bool wide = (r.count_wide >> 31) != 0;
        const uint32_t count = r.count_wide & 0x7fffffffu;
        const v4u_* sp = sel == 0 ? a.src[0] : sel == 1 ? a.src[1] : a.src[2];
        // a run's last chunk may be short of 16 bytes: nothing behind the run's last word is read (a caller's page-locked list may end there)
        const uint32_t left = (wide ? 2u * count : count) - 4u * k;
        v4u_ w;
        if (left >= 4u) {
            w = __builtin_nontemporal_load(sp + (size_t)r.chunk_src + k);
        } else {
            const uint32_t* tp = reinterpret_cast<const uint32_t*>(sp + (size_t)r.chunk_src + k);
            w = v4u_{tp[0], left > 1u ? tp[1] : 0u, left > 2u ? tp[2] : 0u, 0u};
        }
        int32_t* plane = ch == 0 ? a.g.plane[0] : ch == 1 ? a.g.plane[1] : a.g.plane[2];
        const int sx = ch == 0 ? a.g.sx[0] : ch == 1 ? a.g.sx[1] : a.g.sx[2];
        const int sy = ch == 0 ? a.g.sy[0] : ch == 1 ? a.g.sy[1] : a.g.sy[2];
        const SparseRect q = sparse_rect(a.g.W, a.g.H, sx, sy, (int)(r.where & 0xffffffu));
        const uint32_t e0 = wide ? 2u * k : 4u * k;
        uint32_t pos[4];
        int32_t val[4];
        if (wide) {
            pos[0] = w.x; val[0] = (int32_t)w.y;
            pos[1] = w.z; val[1] = (int32_t)w.w;
            pos[2] = pos[3] = 0; val[2] = val[3] = 0;
        } else {
            pos[0] = w.x & 0xffffu; val[0] = (int32_t)w.x >> 16;
            pos[1] = w.y & 0xffffu; val[1] = (int32_t)w.y >> 16;
            pos[2] = w.z & 0xffffu; val[2] = (int32_t)w.z >> 16;
            pos[3] = w.w & 0xffffu; val[3] = (int32_t)w.w >> 16;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (e0 + j >= count || (wide && j >= 2)) continue;  // the padding behind a run's last entry is not an entry
            const uint32_t y = pos[j] >> 8, x = pos[j] & 255u;
            if (y >= (uint32_t)q.gh || x >= (uint32_t)q.gw) { rej++; continue; }
            if (val[j] != 0) atomicAdd(reinterpret_cast<unsigned*>(plane + coeff_off(q.W, q.y0 + (int)y, q.x0 + (int)x)), (unsigned)val[j]);
        }
    }
    for (int o = 32; o > 0; o >>= 1) rej += __shfl_down(rej, o, 64);
    if ((threadIdx.x & 63) == 0 && rej) atomicAdd(a.rejected, (unsigned long long)rej);
}

// zero the group's rectangle in the three tiled planes: a lane clears 16 bytes (a quarter cell row pair), a cell is 256 bytes
__global__ __launch_bounds__(256) void k_sparse_clear(const SparseGeom g, int group) {
    const int ch = blockIdx.y;
    int32_t* plane = ch == 0 ? g.plane[0] : ch == 1 ? g.plane[1] : g.plane[2];
    const int sx = ch == 0 ? g.sx[0] : ch == 1 ? g.sx[1] : g.sx[2];
    const int sy = ch == 0 ? g.sy[0] : ch == 1 ? g.sy[1] : g.sy[2];
    const SparseRect q = sparse_rect(g.W, g.H, sx, sy, group);
    const int cw = q.gw >> 3, cells = cw * (q.gh >> 3);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cells * 16; i += gridDim.x * 256) {
        const int cell = i >> 4, cy = cell / cw, cx = cell - cy * cw;
        *reinterpret_cast<v4u_*>(plane + coeff_off(q.W, q.y0 + cy * 8, q.x0 + cx * 8) + (i & 15) * 4) = v4u_{0, 0, 0, 0};
    }
}

}  // namespace

bool sparse_entries_valid(const uint32_t* words, int32_t n_entries, bool wide, int gw, int gh) {
    const uint32_t ugw = (uint32_t)gw, ugh = (uint32_t)gh;
    unsigned bad = 0;
    if (wide) {
        for (int32_t i = 0; i < n_entries; i++) {
            const uint32_t p = words[2 * (size_t)i];
            bad |= (p >> 16) | ((p >> 8) >= ugh) | ((p & 255u) >= ugw);
        }
    } else {
        for (int32_t i = 0; i < n_entries; i++) {
            const uint32_t p = words[i] & 0xffffu;
            bad |= ((p >> 8) >= ugh) | ((p & 255u) >= ugw);
        }
    }
    return bad == 0;
}

void launch_sparse_scatter(const SparseGeom& g, const SparseRec* recs, const SparseRec* recs_dev, int n_recs, uint32_t total_chunks,
                           const void* const src[3], unsigned long long* rejected, int grid, hipStream_t s) {
    if (n_recs <= 0 || total_chunks == 0) return;
    SparseArgs a{};
    a.g = g;
    for (int k = 0; k < 3; k++) a.src[k] = static_cast<const v4u_*>(src[k]);
    if (n_recs <= 3) {
        a.inl0 = recs[0];
        if (n_recs > 1) a.inl1 = recs[1];
        if (n_recs > 2) a.inl2 = recs[2];
    } else {
        a.recs = recs_dev;
    }
    a.n_recs = n_recs;
    a.total_chunks = total_chunks;
    a.rejected = rejected;
    const unsigned need = (total_chunks + 255u) / 256u;
    hipLaunchKernelGGL(k_sparse_scatter, dim3(need < (unsigned)grid ? need : (unsigned)grid), dim3(256), 0, s, a);
}

void launch_sparse_clear(const SparseGeom& g, int group, hipStream_t s) {
    hipLaunchKernelGGL(k_sparse_clear, dim3(16, 3), dim3(256), 0, s, g, group);
}

}  // namespace jxl
