// jxl_modular_begin_chain: the inverse walk over a frame-level transform chain (ModularStream.applyTransforms,
// ModularStream.java:224-380) as channel bookkeeping, what the entry refuses, and the path table of the fused Palette run
// (k_palette_run.hip). Plain C++ (no device code, no context), so it can be compiled and run on its own
// (tools/native/modchain_check.cpp); host.hip turns the plan into device buffers and launches.
//
// The walk names buffers: buffer i < n_chans is input channel i, every later one is made by an op of the plan. An op never
// writes an input buffer (an RCT over one copies it first), so a plan can run again from its inputs.
//
// A maximal run of consecutive Palette transforms of the inverse walk becomes one ChainOp. While it stays "open" the walk keeps,
// per buffer the run makes, the input of the run it depends on and the lookups in between -- (stage, row) pairs, at most
// kPalRunMaxDepth of them. The run closes (and a new one opens) before a Palette whose palette -- channel 0 at that point -- the
// run itself makes, whose index channel hangs on another source than the run's, or that would pass the stage or depth limits.
// The buffers of a closed run that are still in the channel list are its outputs; a run is `fusable` when they are at most
// kPalRunMaxOut and its palettes together fit kPaletteRunLdsInts. The step form of the same op is its stages in order.
#pragma once
#include <cstdint>
#include <vector>

#include "palette_check.h"

namespace jxl {

constexpr int kPaletteRunLdsInts = 12288;  // all palettes of a fused run, back to back in LDS: 48 KiB (3 workgroups per CU)
constexpr int kPalRunMaxStages = 8;        // Palette transforms in one fused run
constexpr int kPalRunMaxDepth = 4;         // lookups between a run's input and one of its outputs
constexpr int kPalRunMaxOut = 32;          // output planes of one fused run

enum { kChainSqueeze = 0, kChainRct = 1, kChainPalRun = 2 };

struct ChainBuf {
    int32_t w, h;
};

struct ChainPalStage {
    int32_t pal, pal_w, pal_h;  // the buffer that is channel 0 at this point, and its size
    int32_t index, w, h;        // the index buffer and its size
    int32_t num_c, nb_colors, nb_deltas, d_pred;
    int32_t out0;               // its num_c outputs are buffers out0 .. out0 + num_c - 1
};

struct ChainPalOut {
    int32_t buf, depth;
    int32_t stage[kPalRunMaxDepth], row[kPalRunMaxDepth];  // stage: counted from the run's first
};

struct ChainOp {
    int kind;
    // kChainSqueeze: one channel pair of one step
    int horizontal;
    int32_t avg, res, out;
    // kChainRct: dst[j] != src[j] where src[j] is an input buffer (copy first, then in place on dst)
    int32_t src[3], dst[3], type;
    // kChainPalRun: stages [stage0, stage0 + n_stage) of ChainPlan::stages, outputs [out0, out0 + n_out) of ChainPlan::outs
    int32_t stage0, n_stage, out0, n_out, source;
    bool fusable;
};

struct ChainPlan {
    std::vector<ChainBuf> bufs;
    std::vector<ChainOp> ops;
    std::vector<ChainPalStage> stages;
    std::vector<ChainPalOut> outs;
    std::vector<int32_t> list;  // the channel list after the walk, as buffers
    int status = JXL_OK;        // of a refusal
};

namespace chain_detail {
struct Derived {
    int32_t buf, source, depth;
    int32_t stage[kPalRunMaxDepth], row[kPalRunMaxDepth];
};

struct OpenRun {
    bool open = false;
    int32_t stage0 = 0, n_stage = 0, source = -1;
    std::vector<Derived> made;
    const Derived* find(int32_t buf) const {
        for (const Derived& d : made)
            if (d.buf == buf) return &d;
        return nullptr;
    }
};

inline void close_run(ChainPlan* p, OpenRun* r) {
    if (!r->open) return;
    ChainOp op{};
    op.kind = kChainPalRun;
    op.stage0 = r->stage0;
    op.n_stage = r->n_stage;
    op.source = r->source;
    op.out0 = (int32_t)p->outs.size();
    int64_t entries = 0;
    for (int32_t s = 0; s < r->n_stage; s++) {
        const ChainPalStage& st = p->stages[(size_t)(r->stage0 + s)];
        entries += (int64_t)st.num_c * st.nb_colors;
    }
    for (int32_t b : p->list) {
        const Derived* d = r->find(b);
        if (!d) continue;
        ChainPalOut o{};
        o.buf = b;
        o.depth = d->depth;
        for (int k = 0; k < d->depth; k++) {
            o.stage[k] = d->stage[k];
            o.row[k] = d->row[k];
        }
        p->outs.push_back(o);
    }
    op.n_out = (int32_t)p->outs.size() - op.out0;
    op.fusable = op.n_out >= 1 && op.n_out <= kPalRunMaxOut && entries <= kPaletteRunLdsInts;
    p->ops.push_back(op);
    *r = OpenRun();
}
}  // namespace chain_detail

// nullptr: the plan is built; else what is wrong with the call (plan->status says which jxl_status)
inline const char* chain_plan(const jxl_channel* chans, int32_t n_chans, const jxl_modular_transform* tr, int32_t n_tr,
                              int32_t bit_depth, ChainPlan* plan) {
    using namespace chain_detail;
    ChainPlan& p = *plan;
    p = ChainPlan();
    auto refuse = [&](int status, const char* msg) {
        p.status = status;
        return msg;
    };
    if (n_chans < 0 || (n_chans > 0 && !chans) || n_tr < 0 || (n_tr > 0 && !tr)) return refuse(JXL_ERR_INVALID_ARGUMENT, "modular chain: bad arguments");
    for (int32_t i = 0; i < n_chans; i++) {
        if (chans[i].width < 0 || chans[i].height < 0) return refuse(JXL_ERR_INVALID_ARGUMENT, "negative channel size");
        if ((int64_t)chans[i].width * chans[i].height > INT32_MAX) return refuse(JXL_ERR_INVALID_ARGUMENT, "a channel of more than INT32_MAX samples");
        if ((int64_t)chans[i].width * chans[i].height > 0 && !chans[i].data) return refuse(JXL_ERR_INVALID_ARGUMENT, "a channel has no data");
        p.bufs.push_back(ChainBuf{chans[i].width, chans[i].height});
        p.list.push_back(i);
    }
    auto new_buf = [&](int32_t w, int32_t h) {
        p.bufs.push_back(ChainBuf{w, h});
        return (int32_t)p.bufs.size() - 1;
    };
    OpenRun run;
    for (int32_t i = n_tr - 1; i >= 0; i--) {
        const jxl_modular_transform& t = tr[i];
        if (t.kind != JXL_TRANSFORM_PALETTE) close_run(&p, &run);
        if (t.kind == JXL_TRANSFORM_SQUEEZE) {  // :229-254
            if (t.n_sp < 0 || (t.n_sp > 0 && !t.sp)) return refuse(JXL_ERR_INVALID_ARGUMENT, "squeeze: bad step list");
            for (int32_t j = t.n_sp - 1; j >= 0; j--) {
                const int64_t begin = t.sp[j].begin_c, end = begin + t.sp[j].num_c - 1, n = (int64_t)p.list.size();
                const int64_t offset = t.sp[j].in_place ? end + 1 : n + begin - end - 1;
                if (begin < 0 || end < begin || end >= n || offset < 0 || offset + (end - begin) >= n)
                    return refuse(JXL_ERR_INVALID_BITSTREAM, "a squeeze step addresses channels outside the list");
                for (int64_t k = begin; k <= end; k++) {
                    const int32_t a = p.list[(size_t)k], r = p.list[(size_t)(offset + k - begin)];
                    const ChainBuf ab = p.bufs[(size_t)a], rb = p.bufs[(size_t)r];
                    ChainOp op{};
                    op.kind = kChainSqueeze;
                    op.horizontal = t.sp[j].horizontal ? 1 : 0;
                    op.avg = a;
                    op.res = r;
                    if (op.horizontal) {
                        if ((ab.w != rb.w && ab.w != 1 + rb.w) || rb.h != ab.h) return refuse(JXL_ERR_INVALID_ARGUMENT, "Corrupted squeeze transform");
                        op.out = new_buf(ab.w + rb.w, ab.h);
                    } else {
                        if ((ab.h != rb.h && ab.h != 1 + rb.h) || rb.w != ab.w) return refuse(JXL_ERR_STATE, "Corrupted squeeze transform");
                        op.out = new_buf(ab.w, ab.h + rb.h);
                    }
                    if ((int64_t)p.bufs.back().w * p.bufs.back().h > INT32_MAX) return refuse(JXL_ERR_INVALID_ARGUMENT, "a channel of more than INT32_MAX samples");
                    p.ops.push_back(op);
                    p.list[(size_t)k] = op.out;
                }
                p.list.erase(p.list.begin() + offset, p.list.begin() + offset + (end - begin + 1));
            }
        } else if (t.kind == JXL_TRANSFORM_RCT) {  // :255-326
            if (t.rct_type < 0 || t.rct_type >= 42) return refuse(JXL_ERR_INVALID_ARGUMENT, "rct: type outside 0..41");
            if (t.begin_c < 0 || (int64_t)t.begin_c + 2 >= (int64_t)p.list.size()) return refuse(JXL_ERR_INVALID_ARGUMENT, "rct channels out of range");
            static const int lut[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};  // :35-38
            ChainOp op{};
            op.kind = kChainRct;
            op.type = t.rct_type % 7;
            for (int j = 0; j < 3; j++) {
                op.src[j] = p.list[(size_t)(t.begin_c + j)];
                const ChainBuf b = p.bufs[(size_t)op.src[j]], b0 = p.bufs[(size_t)op.src[0]];
                if (b.w != b0.w || b.h != b0.h) return refuse(JXL_ERR_INVALID_BITSTREAM, "RCT must be performed on three equal size channels");
            }
            for (int j = 0; j < 3; j++) op.dst[j] = op.src[j] < n_chans ? new_buf(p.bufs[(size_t)op.src[j]].w, p.bufs[(size_t)op.src[j]].h) : op.src[j];
            p.ops.push_back(op);
            for (int j = 0; j < 3; j++) p.list[(size_t)(t.begin_c + lut[t.rct_type / 7][j])] = op.dst[j];
        } else if (t.kind == JXL_TRANSFORM_PALETTE) {  // :327-378
            const int64_t first = (int64_t)t.begin_c + 1;
            if (t.begin_c < 0 || first >= (int64_t)p.list.size()) return refuse(JXL_ERR_INVALID_ARGUMENT, "palette: channels begin_c + 1 .. begin_c + num_c leave the list");
            if (t.nb_deltas > 0 && t.d_pred == 6)
                return refuse(JXL_ERR_UNSUPPORTED, "palette: weighted-predictor deltas need the plane the host decoder keeps");
            ChainPalStage st{};
            st.pal = p.list[0];
            st.pal_w = p.bufs[(size_t)st.pal].w;
            st.pal_h = p.bufs[(size_t)st.pal].h;
            st.index = p.list[(size_t)first];
            st.w = p.bufs[(size_t)st.index].w;
            st.h = p.bufs[(size_t)st.index].h;
            st.num_c = t.num_c;
            st.nb_colors = t.nb_colors;
            st.nb_deltas = t.nb_deltas;
            st.d_pred = t.d_pred;
            {  // palette_check.h on stand-in pointers: it looks at none of the data
                static int32_t word = 0;
                const jxl_palette_desc d = {t.num_c, t.nb_colors, t.nb_deltas, t.d_pred, bit_depth, st.pal_h, st.pal_w, &word, nullptr};
                std::vector<int32_t*> outs((size_t)(t.num_c >= 1 && t.num_c <= st.pal_h ? t.num_c : 1), &word);
                const char* bad = palette_check(&d, &word, st.h, st.w, outs.data());
                if (bad) return refuse(JXL_ERR_INVALID_ARGUMENT, bad);
            }
            // where the stage hangs in the open run, or why it cannot
            const Derived* di = run.open ? run.find(st.index) : nullptr;
            const int32_t source = di ? di->source : st.index;
            if (run.open && (run.find(st.pal) || run.source != source || run.n_stage >= kPalRunMaxStages || (di && di->depth >= kPalRunMaxDepth))) {
                close_run(&p, &run);
                di = nullptr;
            }
            Derived base{};
            if (di) base = *di;  // (a copy: `made` grows below)
            if (!run.open) {
                run.open = true;
                run.stage0 = (int32_t)p.stages.size();
                run.source = st.index;
                base.source = st.index;
                base.depth = 0;
            }
            st.out0 = (int32_t)p.bufs.size();
            for (int32_t c = 0; c < t.num_c; c++) {
                Derived d = base;
                d.buf = new_buf(st.w, st.h);
                d.stage[d.depth] = run.n_stage;
                d.row[d.depth] = c;
                d.depth++;
                run.made.push_back(d);
            }
            run.n_stage++;
            p.stages.push_back(st);
            // the list surgery: the index channel becomes num_c channels, channel 0 goes
            p.list.erase(p.list.begin() + first);
            for (int32_t c = 0; c < t.num_c; c++) p.list.insert(p.list.begin() + first + c, st.out0 + c);
            p.list.erase(p.list.begin());
        } else {
            return refuse(JXL_ERR_INVALID_ARGUMENT, "modular chain: unknown transform kind");
        }
    }
    close_run(&p, &run);
    return nullptr;
}

// jxl_modular_begin expresses "one Squeeze, then one RCT" of the inverse walk: [], [RCT], [Squeeze], [RCT, Squeeze]
inline bool chain_is_plain(const jxl_modular_transform* tr, int32_t n_tr) {
    if (n_tr == 0) return true;
    if (n_tr == 1) return tr[0].kind == JXL_TRANSFORM_RCT || tr[0].kind == JXL_TRANSFORM_SQUEEZE;
    return n_tr == 2 && tr[0].kind == JXL_TRANSFORM_RCT && tr[1].kind == JXL_TRANSFORM_SQUEEZE;
}

}  // namespace jxl
