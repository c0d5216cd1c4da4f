"""Named, seeded cases of the inverse Palette transform for tests/test_palette_cpu.py, test_palette_gpu.py and
test_jni_shim_palette.py: the smallest shapes at which each mechanism of jxl_stage_palette can go wrong.

A case is a dict: h, w, num_c, nb_colors, nb_deltas, d_pred, bit_depth, index (h x w int32), palette (pal_h x pal_w int32, pal_h >=
num_c, pal_w >= nb_colors) and pred (h x w int32 or None). Every index class is planted in every case with room for it: inside the
palette, the 64-entry cube above it, the / 5 ladder above that (up to INT32_MAX), negative (-1, -143, -144 and INT32_MIN among them)
and, where nb_deltas > 0, positive indices below nb_deltas. Palette entries lie near +-2^30, so the sums of predictors 3 and 10-13
and the final value + prediction wrap at 32 bits.

expected(name) is the model's answer (tests/palette_ref.py), computed once per process."""
import numpy as np

import palette_ref

LDS_INTS = 8192       # kPaletteLdsInts of jxlatte_amd/csrc/jxl_internal.h: a palette of more entries is read from global memory
CHAIN_THREADS = 256   # kPaletteChainThreads: the rows of one t-front a pass of the chain kernel takes
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
BIT_DEPTHS = (1, 3, 8, 10, 16, 24, 31, 32)


def _make(seed, h, w, num_c, nb_colors, nb_deltas, d_pred, bit_depth, pal_extra=(0, 0), negatives=True, with_pred=None, delta_share=0.25):
    rng = np.random.default_rng(seed)
    n = h * w
    pal_h, pal_w = num_c + pal_extra[0], nb_colors + pal_extra[1]
    sign = rng.choice(np.array([-1, 1], np.int64), (pal_h, pal_w))
    palette = (sign * ((1 << 30) + rng.integers(-1000, 1001, (pal_h, pal_w)))).astype(np.int32)
    small = rng.random((pal_h, pal_w)) < 0.25
    palette[small] = rng.integers(-300, 301, int(small.sum()))
    # the classes an index can belong to, as generators
    classes = []
    if nb_colors > 0:
        classes.append(lambda k: rng.integers(0, nb_colors, k))
        classes.append(lambda k: np.full(k, nb_colors - 1))
    classes.append(lambda k: nb_colors + rng.integers(0, 64, k))                        # the cube
    classes.append(lambda k: nb_colors + 64 + rng.integers(0, 5 ** 4 + 40, k))          # the ladder, every digit of 4 channels
    classes.append(lambda k: rng.integers(I32_MAX - 2000, I32_MAX, k, endpoint=True))   # the ladder's far end
    if nb_deltas > 0:
        classes.append(lambda k: rng.integers(0, nb_deltas, k))                          # positive delta indices
    if negatives:
        classes.append(lambda k: -1 - rng.integers(0, 400, k))
        classes.append(lambda k: rng.integers(I32_MIN, I32_MIN + 2000, k))
    planted = [c(1)[0] for c in classes]
    if negatives:
        planted += [-1, -143, -144, -145, -286, -287, I32_MIN, I32_MIN + 1]
    planted += [nb_colors, nb_colors + 63, nb_colors + 64, nb_colors + 64 + 624, I32_MAX]
    # most pixels are plain palette entries (or cube entries without a palette); the rest is drawn from every class
    index = (rng.integers(0, nb_colors, n) if nb_colors > 0 else nb_colors + rng.integers(0, 64, n)).astype(np.int64)
    special = np.flatnonzero(rng.random(n) < delta_share)
    which = rng.integers(0, len(classes), special.size)
    for k, c in enumerate(classes):
        sel = special[which == k]
        index[sel] = c(sel.size)
    if n >= 4 * len(planted):
        at = rng.choice(n, len(planted), replace=False)
        index[at] = planted
    elif n > 1:  # a tiny shape: as many of the planted values as fit, a different choice per seed
        at = rng.permutation(n)
        index[at] = [planted[(seed + j) % len(planted)] for j in range(n)]
    else:
        index[0] = planted[seed % len(planted)]
    if with_pred is None:
        with_pred = d_pred == 6
    pred = None
    if with_pred:
        pred = rng.integers(-(1 << 20), 1 << 20, (h, w)).astype(np.int32)
        edge = rng.random((h, w)) < 0.1
        pred[edge] = rng.choice(np.array([I32_MAX, I32_MAX - 2, I32_MAX - 3, I32_MIN, -4, -3, 4, 5], np.int64), int(edge.sum())).astype(np.int32)
    return dict(h=h, w=w, num_c=num_c, nb_colors=nb_colors, nb_deltas=nb_deltas, d_pred=d_pred, bit_depth=bit_depth,
                index=index.astype(np.int32).reshape(h, w), palette=palette, pred=pred)


def _build():
    cases = {}
    # every predictor, on the two larger shapes in turn (33 x 70 spans more than one workgroup of the lookup kernel: 2310 samples
    # are 578 groups of 4, three workgroups, and end in a group of 2), every num_c and every bit depth in rotation
    for k in range(14):
        h, w = ((21, 37), (33, 70))[k & 1]
        cases["pred%02d_%dx%d" % (k, h, w)] = _make(100 + k, h, w, (1, 3, 4)[k % 3], 40 + 7 * k, (0, 5, 60)[(k // 2) % 3] if k != 9 else 300,
                                                    k, BIT_DEPTHS[k % 8], pal_extra=(k % 2, k % 3))
    # the small shapes: rows and columns of one, the first rows where NN and NEE do not exist
    for j, (h, w) in enumerate(((1, 1), (1, 1), (1, 1), (1, 7), (7, 1), (2, 5))):
        for k in (4, 13):
            cases["shape_%dx%d_%d_pred%02d" % (h, w, j, k)] = _make(200 + 10 * j + k, h, w, (3, 4, 1)[j % 3], 6, 3, k, BIT_DEPTHS[(j + k) % 8],
                                                                     delta_share=0.6)
    # the longest t-front (x + 3 y = t) of 257 x 769 has 257 pixels: one more than the chain kernel's workgroup, the smallest
    # shape that does that
    cases["front_257x769"] = _make(300, CHAIN_THREADS + 1, 3 * CHAIN_THREADS + 1, 1, 50, 10, 13, 12, delta_share=0.3)
    # the palette that fills the LDS budget exactly (with a row stride above nb_colors) and the first that does not fit
    cases["lds_exact_4x2048"] = _make(400, 33, 70, 4, LDS_INTS // 4, 100, 5, 16, pal_extra=(1, 3))
    cases["lds_over_4x2049"] = _make(401, 33, 70, 4, LDS_INTS // 4 + 1, 100, 11, 8, pal_extra=(0, 5))
    # no delta pixel although the predictor would chain: nb_deltas 0 and no negative index -> the lookup kernel alone
    cases["no_delta_pixel_pred05"] = _make(500, 21, 37, 3, 30, 0, 5, 8, negatives=False)
    # predictor 6 without the weighted predictor's plane: allowed while nb_deltas is 0, a negative index then adds 0
    cases["pred06_without_plane"] = _make(501, 21, 37, 3, 30, 0, 6, 10, with_pred=False)
    # no palette at all: every index is implicit
    cases["nb_colors_0"] = _make(502, 21, 37, 4, 0, 0, 2, 24)
    # more channels than the cube's and the ladder's shifts have bits for: index >> (2 * c) with c >= 16 counts mod 32
    cases["num_c_18"] = _make(503, 2, 5, 18, 4, 2, 1, 8, delta_share=0.8)
    return cases


CASES = _build()
_expected = {}


def expected(name):
    if name not in _expected:
        c = CASES[name]
        _expected[name] = palette_ref.inverse_palette(c["index"], c["palette"], c["num_c"], c["nb_colors"], c["nb_deltas"], c["d_pred"],
                                                      c["bit_depth"], c["pred"])
        _expected[name].setflags(write=False)
    return _expected[name]


def launches(name):
    """the kernel launches jxl_stage_palette needs: the chain kernel runs behind the lookup kernel where some pixel has index <
    nb_deltas and the predictor reads neighbours"""
    c = CASES[name]
    return 2 if c["d_pred"] not in (0, 6) and bool((c["index"] < c["nb_deltas"]).any()) else 1


def write_case_file(path, names):
    """the binary hand-over to tools/native/palette_check.cpp (its header comment has the layout)"""
    with open(path, "wb") as f:
        f.write(np.array([len(names)], np.int32).tobytes())
        for name in names:
            c = CASES[name]
            head = [c["h"], c["w"], c["num_c"], c["nb_colors"], c["nb_deltas"], c["d_pred"], c["bit_depth"], c["palette"].shape[0],
                    c["palette"].shape[1], int(c["pred"] is not None)]
            f.write(np.array(head, np.int32).tobytes())
            f.write(np.ascontiguousarray(c["index"], np.int32).tobytes())
            f.write(np.ascontiguousarray(c["palette"], np.int32).tobytes())
            if c["pred"] is not None:
                f.write(np.ascontiguousarray(c["pred"], np.int32).tobytes())
