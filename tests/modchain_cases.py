"""Named, seeded cases of jxl_modular_begin_chain for tests/test_modchain_cpu.py and test_modchain_gpu.py: the smallest shapes at
which the inverse walk, its Palette steps on device channels and the fused Palette run (k_palette_run) can go wrong.

A case is a dict: chans (the encoded channel list, 2-D int32 arrays, meta channels first), transforms (bitstream order,
dictionaries as frontend.transforms() returns them), bit_depth, and runs: what jxlatte_amd/csrc/modchain_check.h must make of
its Palette transforms -- (stages, fusable) per run, in the order undone.

expected(name) is the model's answer (tests/modchain_ref.py), computed once per process; chained(name) says per Palette, in the
order undone, whether some pixel of it needed a neighbour; stats(name, fuse) is what jxl_debug_last_palette_run reports after
the plan ran and its outputs were read."""
import numpy as np

import modchain_ref as ref
import palette_cases
from modchain_ref import PALETTE, RCT, SQUEEZE

RUN_LDS_INTS = 12288   # kPaletteRunLdsInts of jxlatte_amd/csrc/modchain_check.h: all palettes of a fused run together
RUN_MAX_STAGES, RUN_MAX_DEPTH, RUN_MAX_OUT = 8, 4, 32
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SIZES = ((1, 1), (5, 7), (33, 70))  # 1 sample; 35: a tail of 3; 2310: three workgroups and a tail of 2


def pal(begin_c, num_c, nb_colors, nb_deltas=0, d_pred=0):
    return dict(kind=PALETTE, begin_c=begin_c, num_c=num_c, rct_type=0, nb_colors=nb_colors, nb_deltas=nb_deltas, d_pred=d_pred, steps=[])


def rct(begin_c, rct_type):
    return dict(kind=RCT, begin_c=begin_c, num_c=0, rct_type=rct_type, nb_colors=0, nb_deltas=0, d_pred=0, steps=[])


def squeeze(steps):
    return dict(kind=SQUEEZE, begin_c=0, num_c=0, rct_type=0, nb_colors=0, nb_deltas=0, d_pred=0, steps=list(steps))


def _indices(rng, h, w, nb_colors, wild=0.2, negatives=False):
    """mostly entries of the palette; the rest from the cube and the ladder above it, INT32_MAX, and, where asked for, below 0"""
    n = h * w
    idx = rng.integers(0, max(nb_colors, 1), n).astype(np.int64)
    pool = [nb_colors, nb_colors + 63, nb_colors + 64, nb_colors + 64 + 624, I32_MAX, I32_MAX - 7]
    if negatives:
        pool += [-1, -143, -144, -287, I32_MIN, I32_MIN + 1]
    sel = np.flatnonzero(rng.random(n) < wild)
    idx[sel] = rng.choice(np.array(pool, np.int64), sel.size)
    if n >= 4 * len(pool):
        idx[rng.choice(n, len(pool), replace=False)] = pool
    return idx.astype(np.int32).reshape(h, w)


def _palette(rng, rows, cols, lo, hi, extra=()):
    """entries in [lo, hi) -- the next stage's indices --, and `extra` planted where there is room"""
    p = rng.integers(lo, hi, (rows, cols)).astype(np.int64)
    extra = list(extra)
    if p.size >= 2 * len(extra) and extra:
        flat = p.reshape(-1)
        flat[rng.choice(p.size, len(extra), replace=False)] = extra
    return p.astype(np.int32)


def _nested(seed, h, w, depth, preds=None, negatives_at=None, bit_depth=8):
    """one channel under `depth` palettes, each on the index channel of the one before: stage k's output is stage k + 1's index.
    The palettes undone first hold, beside plain indices of the next, its cube, its ladder, INT32_MAX and -- where preds leaves
    every stage pure -- negative values, INT32_MIN among them"""
    rng = np.random.default_rng(seed)
    preds = preds or [(0, 0)] * depth  # (nb_deltas, d_pred) per palette, in bitstream order
    colors = [11 + 6 * k for k in range(depth)]  # nb_colors per palette, bitstream order; palette k sits at channel depth - 1 - k
    chans, transforms = [], []
    for k in range(depth):
        transforms.append(pal(k, 1, colors[k], *preds[k]))
    for k in reversed(range(depth)):  # channel list: the palette undone first comes first
        if k == 0:
            p = _palette(rng, 1, colors[0] + 2, -(1 << 30), 1 << 30, [I32_MIN, I32_MAX, 0, -1])
        else:  # its values index palette k - 1
            nxt = colors[k - 1]
            pure_below = preds[k - 1][1] in (0, 6)
            extra = [nxt, nxt + 63, nxt + 64, nxt + 64 + 624, I32_MAX, I32_MAX - 1]
            if pure_below:
                extra += [-1, -143, -144, I32_MIN, I32_MIN + 1]
            p = _palette(rng, 1, colors[k] + (k & 1), 0, nxt, extra)
            if negatives_at == k:
                p[p < 0] = 0
                p[0, 3] = -2  # ONE negative value
        chans.append(p)
    index = _indices(rng, h, w, colors[depth - 1], negatives=preds[depth - 1][1] in (0, 6) and negatives_at is None)
    if negatives_at is not None:  # pixel 0 names the planted entry of the palette undone first
        assert negatives_at == depth - 1
        index.reshape(-1)[0] = 3
    chans.append(index)
    return dict(chans=chans, transforms=transforms, bit_depth=bit_depth, runs=[(depth, True)])


def _sample_shape(seed, h, w, bit_depth=8):
    """patches-lossless.jxl's own chain: three 1-channel palettes on R, G and B, then one 4-channel palette over their index
    channels and alpha. Encoded: [P4 (4 x n4), P_B, P_G, P_R, index]"""
    rng = np.random.default_rng(seed)
    nr, ng, nb, n4 = 19, 23, 17, 29
    transforms = [pal(0, 1, nr), pal(2, 1, ng), pal(4, 1, nb), pal(3, 4, n4)]
    p4 = np.stack([_palette(rng, 1, n4, 0, nr, [nr, nr + 70, -1, I32_MIN])[0], _palette(rng, 1, n4, 0, ng, [ng + 63, I32_MAX])[0],
                   _palette(rng, 1, n4, 0, nb, [-143, nb + 64 + 624])[0], _palette(rng, 1, n4, 0, 256)[0]])
    chans = [p4, _palette(rng, 1, nb, 0, 256), _palette(rng, 1, ng, 0, 256), _palette(rng, 1, nr, 0, 256), _indices(rng, h, w, n4, negatives=True)]
    return dict(chans=chans, transforms=transforms, bit_depth=bit_depth, runs=[(4, True)])


def _budget(seed, over):
    """two palettes on one channel whose entries together are the fused run's LDS budget exactly, or one more"""
    rng = np.random.default_rng(seed)
    n0 = 4096 + (1 if over else 0)
    n1 = (RUN_LDS_INTS - 4096) // 4  # a 4-channel palette undone first
    transforms = [pal(0, 1, n0), pal(1, 4, n1)]
    p1 = _palette(rng, 4, n1 + 3, 0, n0, [n0 - 1, n0, -1, I32_MAX])
    p1[:, n1 - 1] = n0 - 1  # the last entry of the palette undone first names the last entry of the other
    p0 = _palette(rng, 1, n0, -1000, 1000)
    p0[0, n0 - 1] = 123456789
    index = _indices(rng, 33, 70, n1)
    index.reshape(-1)[:2] = n1 - 1
    # undone first: P(begin 1): channel 0 = p1, index -> 4 planes; then P(begin 0): channel 0 = p0, index = plane 0
    return dict(chans=[p1, p0, index], transforms=transforms, bit_depth=8, runs=[(2, not over)])


def _build():
    cases = {}
    for h, w in SIZES:
        tag = "%dx%d" % (h, w)
        cases["depth1_" + tag] = _nested(10 + h, h, w, 1)
        cases["depth2_" + tag] = _nested(20 + h, h, w, 2)
        cases["depth3_" + tag] = _nested(30 + h, h, w, 3, bit_depth=12)
        cases["sample_shape_" + tag] = _sample_shape(40 + h, h, w)
    # delta pixels that stay pure: predictor 0 with nb_deltas > 0 at both stages, 16 bits
    cases["pure_deltas_33x70"] = _nested(50, 33, 70, 2, preds=[(5, 0), (7, 0)], bit_depth=16)
    # ONE negative value in the palette undone first, met by pixel 0: under predictor 5 at the second stage that pixel needs its
    # neighbours (one redo); under predictor 0 it does not
    cases["planted_negative_pred5"] = _nested(60, 33, 70, 2, preds=[(0, 5), (0, 0)], negatives_at=1)
    cases["planted_negative_pred0"] = _nested(60, 33, 70, 2, preds=[(0, 0), (0, 0)], negatives_at=1)
    # depth and stage limits: five nested palettes are one run of five stages cut after the fourth lookup
    c = _nested(70, 5, 7, 5)
    c["runs"] = [(4, True), (1, True)]
    cases["depth5_5x7"] = c
    # num_c 18: more channels than the cube's and the ladder's shifts have bits for
    rng = np.random.default_rng(80)
    cases["num_c_18"] = dict(chans=[_palette(rng, 19, 6, -500, 500), _indices(rng, 5, 7, 4, wild=0.6, negatives=True)],
                             transforms=[pal(0, 18, 4, 2, 0)], bit_depth=8, runs=[(1, True)])
    # a palette of more entries than k_palette_lookup stages in LDS, wider than nb_colors: the fused run holds it, the step form
    # reads it from the device channel at its pitch
    rng = np.random.default_rng(85)
    cases["palette_in_global_memory"] = dict(chans=[_palette(rng, 2, 4103, -(1 << 30), 1 << 30), _indices(rng, 5, 7, 4100, negatives=True)],
                                             transforms=[pal(0, 2, 4100)], bit_depth=8, runs=[(1, True)])
    cases["palette_in_global_memory"]["chans"][1].reshape(-1)[:2] = (4099, 0)
    cases["lds_budget_exact"] = _budget(90, False)
    cases["lds_budget_over"] = _budget(91, True)
    # the longest t-front of 257 x 769 is one more than the chain kernel's workgroup (tests/palette_cases.py): predictor 13 with
    # delta pixels, through the plan's step form
    f = palette_cases.CASES["front_257x769"]
    cases["front_257x769"] = dict(chans=[f["palette"], f["index"]], transforms=[pal(0, 1, f["nb_colors"], f["nb_deltas"], f["d_pred"])],
                                  bit_depth=f["bit_depth"], runs=[(1, True)])
    # a palette the run itself makes: [PA (2 x k), I] -> [A0, A1], and A0 is the palette of the Palette undone next
    rng = np.random.default_rng(100)
    cases["palette_made_by_the_run"] = dict(chans=[_palette(rng, 2, 9, 0, 40, [-1, 70, I32_MAX]), _indices(rng, 5, 7, 9, negatives=True)],
                                            transforms=[pal(0, 1, 6), pal(0, 2, 9)], bit_depth=8, runs=[(1, True), (1, True)])
    # a Palette on the palette channel of another (its index channel is another source: the run closes), next to channels of
    # other sizes that stay as they are. Undone: P(begin 1) on [P2, P1, P0i, X2, Y] makes P0 from P0i; P(begin 1) makes X1 from
    # X2 by P1; P(begin 0) makes X from X1 by P0
    rng = np.random.default_rng(110)
    p0i = _indices(rng, 1, 13, 7, negatives=True)
    cases["palette_of_a_palette"] = dict(
        chans=[_palette(rng, 1, 7, -300, 300), _palette(rng, 1, 9, 0, 13, [13, 90, -1]), p0i, _indices(rng, 33, 70, 9, negatives=True),
               rng.integers(I32_MIN, I32_MAX, (3, 5)).astype(np.int32)],
        transforms=[pal(0, 1, 13), pal(1, 1, 9), pal(1, 1, 7)], bit_depth=10, runs=[(1, True), (2, True)])
    # chains with the other transforms. [Palette, RCT]: the RCT is undone first, over the index channel and two more inputs
    rng = np.random.default_rng(120)
    trio = [rng.integers(-40, 40, (5, 7)).astype(np.int32) for _ in range(3)]
    cases["palette_rct"] = dict(chans=[_palette(rng, 3, 12, -(1 << 30), 1 << 30)] + trio, transforms=[pal(0, 3, 12), rct(1, 6 + 7 * 2)], bit_depth=8,
                                runs=[(1, True)])
    # [RCT, Palette]: the RCT works in place on the run's outputs, with a permutation
    cases["rct_palette"] = dict(chans=[_palette(rng, 3, 12, -(1 << 30), 1 << 30), _indices(rng, 33, 70, 12, negatives=True)],
                                transforms=[rct(0, 5 + 7 * 4), pal(0, 3, 12)], bit_depth=8, runs=[(1, True)])
    # [Palette, Squeeze]: the index channel is a horizontal step's output (17 + 16 columns), then a vertical one's
    avg, res = rng.integers(-20, 40, (5, 17)).astype(np.int32), rng.integers(-9, 9, (5, 16)).astype(np.int32)
    res2 = rng.integers(-9, 9, (4, 33)).astype(np.int32)
    cases["palette_squeeze"] = dict(chans=[_palette(rng, 2, 30, -1000, 1000), avg, res, res2],
                                    transforms=[pal(0, 2, 30), squeeze([(0, 1, 1, 1), (1, 1, 1, 1)])], bit_depth=8, runs=[(1, True)])
    # [Squeeze, Palette]: the step's average is the run's output
    cases["squeeze_palette"] = dict(chans=[_palette(rng, 1, 30, -1000, 1000), _indices(rng, 5, 7, 30), rng.integers(-9, 9, (5, 7)).astype(np.int32)],
                                    transforms=[squeeze([(1, 1, 0, 1)]), pal(0, 1, 30)], bit_depth=8, runs=[(1, True)])
    # [RCT, RCT]: the first undone copies the inputs, the second works in place on two of the copies and one input
    quad = [rng.integers(I32_MIN, I32_MAX, (5, 7)).astype(np.int32) for _ in range(4)]
    cases["rct_rct"] = dict(chans=quad, transforms=[rct(0, 6 + 7 * 1), rct(1, 4 + 7 * 5)], bit_depth=8, runs=[])
    # [RCT, Squeeze]: what jxl_modular_begin expresses
    a3 = [rng.integers(-100, 100, (9, 10)).astype(np.int32) for _ in range(3)]
    r3 = [rng.integers(-20, 20, (9, 10)).astype(np.int32) for _ in range(3)]
    cases["rct_squeeze"] = dict(chans=a3 + r3, transforms=[rct(0, 6), squeeze([(1, 0, 0, 3)])], bit_depth=8, runs=[])
    return cases


CASES = _build()
PLAIN = ("rct_squeeze",)  # chains jxl_modular_begin expresses
_expected, _chained = {}, {}


def _palette_fn(index, palette, num_c, nb_colors, nb_deltas, d_pred, bit_depth, pred=None):
    f = palette_cases.CASES["front_257x769"]
    if index is f["index"] or (index.shape == f["index"].shape and np.array_equal(index, f["index"])):
        return palette_cases.expected("front_257x769")  # (the one large model run: shared with the Palette stage's tests)
    return ref.palette_ref.inverse_palette(index, palette, num_c, nb_colors, nb_deltas, d_pred, bit_depth, pred)


def expected(name):
    if name not in _expected:
        c = CASES[name]
        flags = []
        out = ref.apply_chain(c["chans"], c["transforms"], c["bit_depth"], palette_fn=_palette_fn, chained=flags)
        for a in out:
            a.setflags(write=False)
        _expected[name], _chained[name] = out, flags
    return _expected[name]


def chained(name):
    expected(name)
    return _chained[name]


def stats(name, fuse):
    """(fused launches, step launches, redone runs) of jxl_debug_last_palette_run after one jxl_modular_run and the reading of
    its outputs. A run that is not fused runs its lookups on trust; a run that reports -- fused, or a lookup that counted delta
    pixels of a chained stage -- makes the plan run again in order: every stage's lookup, and k_palette_chain where the model
    says a pixel needed a neighbour. (Only single-run cases report here: behind a reporting run the first pass computes on
    values that are not final.)"""
    c = CASES[name]
    stages = sum(n for n, _ in c["runs"])
    fused = sum(1 for _, ok in c["runs"] if ok) if fuse else 0
    steps = sum(n for n, ok in c["runs"] if not (ok and fuse))
    redone = 0
    if any(chained(name)):
        assert len(c["runs"]) == 1
        redone = 1
        steps += stages + sum(chained(name))
    return fused, steps, redone


def write_case_file(path, names):
    """the binary hand-over to tools/native/modchain_check.cpp (its header comment has the layout)"""
    with open(path, "wb") as f:
        f.write(np.array([len(names)], np.int32).tobytes())
        for name in names:
            c = CASES[name]
            f.write(np.array([c["bit_depth"], len(c["chans"]), len(c["transforms"])], np.int32).tobytes())
            for a in c["chans"]:
                f.write(np.array([a.shape[1], a.shape[0]], np.int32).tobytes())
                f.write(np.ascontiguousarray(a, np.int32).tobytes())
            for t in c["transforms"]:
                f.write(np.array([t["kind"], t["begin_c"], t["num_c"], t["rct_type"], t["nb_colors"], t["nb_deltas"], t["d_pred"], len(t["steps"])],
                                 np.int32).tobytes())
                f.write(np.array([v for s in t["steps"] for v in s], np.int32).tobytes())


def read_result_file(path, count):
    got = np.fromfile(path, np.int32)
    at, out = 0, []
    for _ in range(count):
        n = int(got[at])
        at += 1
        chans = []
        for _ in range(n):
            w, h = int(got[at]), int(got[at + 1])
            chans.append(got[at + 2:at + 2 + w * h].reshape(h, w))
            at += 2 + w * h
        out.append(chans)
    assert at == got.size
    return out
