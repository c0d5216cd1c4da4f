"""Inputs shared by tests/test_pixel_ref64_cpu.py and tests/test_pixel_ref64_gpu.py (no test in here), made hard on purpose: an LF
image whose smoothing gap lies in all three regimes, upsampling planes that clamp and planes that do not, noise frames with ragged
groups, full-range int32 for every integer stage. Cached, and never modified by a test."""
import functools

import numpy as np

import pixel_ref64 as M
from jxlatte_amd import synth

F = np.float32
SD = (1.0 / 4096 * 65536 / (2500 * 16), 1.0 / 512 * 65536 / (2500 * 16), 1.0 / 256 * 65536 / (2500 * 16))  # LFGlobal.java:71

# ---- LF ---------------------------------------------------------------------------------------------------------------------------
LF_SHAPES = [(1, 1), (2, 7), (3, 3), (9, 11), (64, 65), (5, 129)]  # one row / one lane past the kernel's 64 x 4 block
LF_ARGS = dict(x_factor_lf=140, b_factor_lf=100, base_corr_x=0.0, base_corr_b=1.0, color_factor=84)
# multiplier of the production scaledDequant per extraPrecision, chosen so that each smoothing regime (gap = 0.5, between, >= 0.75)
# holds >= 10 % of the interior cells. The samples carry the multiplier divided by 1 << extraPrecision and the gap scales them by the
# undivided value once more, so the gap goes with multiplier^2 >> extraPrecision: 4 at extraPrecision 0 is 8 at extraPrecision 2 (at 4
# every cell has gap 0.5 there, at 16 fewer than 10 % of them; the shares obtained: tests/test_pixel_ref64_cpu.py).
LF_SD_MUL = {0: 4, 2: 8}
LF_CASES = [(shape, ep, LF_SD_MUL[ep]) for shape in LF_SHAPES for ep in (0, 2)] + [((64, 65), 1, 1)]  # the last: production triple
LF_MIN_INTERIOR = 50
LF_MIN_SHARE = 0.10


def lf_sd(mul):
    return [F(s) * F(mul) for s in SD]


@functools.lru_cache(maxsize=None)
def lf_quant(shape, seed=1):
    q = np.random.default_rng(seed * 100003 + shape[0] * 300 + shape[1]).integers(-2000, 2000, size=(3,) + tuple(shape)).astype(np.int32)
    q.setflags(write=False)
    return q


# ---- k-times upsampling --------------------------------------------------------------------------------------------------------------
UP_KS = (2, 4, 8)
UP_SHAPES = [(1, 1), (2, 5), (3, 2), (37, 50)]
UP_PACKED = {2: 15, 4: 55, 8: 210}


@functools.lru_cache(maxsize=None)
def up_inputs(k, shape):
    """(packed weights, a standard normal plane, an all-negative plane: the Float.MIN_VALUE quirk)"""
    rng = np.random.default_rng(k * 1000 + shape[0] * 7 + shape[1])
    packed = (rng.standard_normal(UP_PACKED[k]) * 0.2).astype(F)
    a = rng.standard_normal(shape).astype(F)
    b = (-np.abs(rng.standard_normal(shape)) - 1).astype(F)
    for v in (packed, a, b):
        v.setflags(write=False)
    return packed, a, b


def up_runs(k, shape):
    """[(name, plane, packed weights)]: the all-negative plane runs under the weights and under their negation -- whichever sign a
    tile's weights sum to, one of the two drives its totals above zero, where the reference's max starts (Frame.java:241)"""
    packed, a, b = up_inputs(k, shape)
    return [("normal", a, packed), ("negative", b, packed), ("negative, weights negated", b, -packed)]


# ---- noise ----------------------------------------------------------------------------------------------------------------------------
NOISE_INIT = [(1, 1, 256, 3), (5, 40, 16, 1), (130, 129, 128, 3), (40, 300, 256, 3), (33, 50, 16, 2)]


def noise_seed(h, w):
    return (3 << 32) | (h * w)


NOISE_ADD_CORR = [(0.0, 1.0), (-0.3, 0.935)]


@functools.lru_cache(maxsize=None)
def noise_add_inputs():
    """(planes, noise, lut): 50 x 67, finite, rows 10..19 driven past the >= 7 branch, a LUT that leaves [0, 1] on both sides"""
    rng = np.random.default_rng(77)
    p = rng.standard_normal((3, 50, 67)).astype(F)
    p[1] += F(1.0)
    p[:, 10:20] *= F(4)
    nz = M.noise_init(50, 67, 99)[0].astype(F)
    lut = (rng.random(8) * 1.6 - 0.3).astype(F)
    for v in (p, nz, lut):
        v.setflags(write=False)
    return p, nz, lut


# ---- modularToFloat -------------------------------------------------------------------------------------------------------------------
TO_FLOAT_SCALES = (1.0 / 255, 0.0037)


@functools.lru_cache(maxsize=None)
def to_float_inputs():
    """full-range int32 (the conversion rounds beyond 2^24), pairs whose sum wraps, the extremes themselves"""
    rng = np.random.default_rng(3)
    a = rng.integers(-2 ** 31, 2 ** 31, size=(31, 17), dtype=np.int64).astype(np.int32)
    b = rng.integers(-2 ** 31, 2 ** 31, size=(31, 17), dtype=np.int64).astype(np.int32)
    a[0, :6] = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 16777217, -16777219]
    b[0, :6] = [1, -1, 2 ** 31 - 1, -2 ** 31, 0, 0]
    for v in (a, b):
        v.setflags(write=False)
    return a, b


# ---- single squeeze steps -----------------------------------------------------------------------------------------------------------------
SQUEEZE_SHAPES = [(1, 1, 0), (1, 1, 1), (3, 2, 1), (64, 64, 64), (65, 33, 32), (200, 129, 129), (7, 500, 499)]  # (other, avg, res)
LO, HI = -2 ** 31, 2 ** 31 - 1
EXTREME_POOL = np.array([HI, LO, LO, HI, HI, LO + 1, HI - 1, 0, -1, 1, LO, LO, HI, HI, 2 ** 30, -2 ** 30, HI, LO, 5, LO, HI, -7], np.int64)


@functools.lru_cache(maxsize=None)
def squeeze_random(other, an, rn):
    """(avg, res) with the squeezed axis last; averages of +-3000, Laplace residuals"""
    rng = np.random.default_rng(other * 3 + an)
    avg = rng.integers(-3000, 3000, size=(other, an)).astype(np.int32)
    res = np.rint(rng.laplace(0, 40, size=(other, rn))).astype(np.int32)
    return avg, res


@functools.lru_cache(maxsize=None)
def squeeze_extremes():
    """[(avg, res)]: triples whose true differences leave the int32 range; the short rows with zero and with extreme residuals, and
    long rows (the segmented walk) over the same pool"""
    rng = np.random.default_rng(31)
    pool = EXTREME_POOL
    rows = [pool, pool[::-1], np.resize(np.array([HI, LO]), pool.size), np.resize(np.array([LO, LO, HI]), pool.size)]
    rows += [rng.choice(pool, size=pool.size) for _ in range(60)]
    avg = np.array(rows, np.int64).astype(np.int32)
    out = [(avg, np.zeros_like(avg)),
           (avg, rng.choice(np.array([HI, LO, 0, 1, -1, 12345], np.int64), size=avg.shape).astype(np.int32))]
    out.append((rng.choice(pool, size=(70, 700)).astype(np.int32),
                rng.choice(np.array([HI, LO, 0, 3, -3], np.int64), size=(70, 700)).astype(np.int32)))
    return out


def adversarial(n=300, other=70):
    """rows whose recurrence never forgets its start (tests/test_modular_gpu.py::_adversarial, restated): averages falling by 1000 per
    pair with residual 1992 hold the chain in the slope-2 clamp of tendency(); row 1 is ordinary data"""
    a = np.empty((other, n), np.int64)
    a[:] = 10_000_000 - 1000 * np.arange(n)
    r = np.full((other, n), 1992, np.int64)
    r[:, 0] = 1994
    rng = np.random.default_rng(5)
    a[1] = rng.integers(-3000, 3000, size=n)
    r[1] = np.rint(rng.laplace(0, 40, size=n))
    return a.astype(np.int32), r.astype(np.int32)


# ---- plans -----------------------------------------------------------------------------------------------------------------------------
PLAN_FRAMES = [(1, 1, 3), (9, 9, 1), (53, 37, 3), (37, 130, 4), (611, 437, 3)]  # (width, height, channels) of synth.make_modular_frame
VH_SHAPES = [(2, 2), (65, 65), (130, 257), (193, 67)]


@functools.lru_cache(maxsize=None)
def plan_frame(w, h, ch):
    mod = synth.make_modular_frame(w, h, channels=ch, seed=w + h)
    return mod["chans"], mod["sp"]


@functools.lru_cache(maxsize=None)
def vh_inputs(htot, wtot, big=False):
    """the channel list of a two-step plan (forward H then V, so the inverse runs V then H): averages, V residuals, H residuals"""
    rng = np.random.default_rng(htot * 131 + wtot + (7 if big else 0))
    ah, rh, aw, rw = (htot + 1) // 2, htot // 2, (wtot + 1) // 2, wtot // 2
    if big:
        draw = lambda s: rng.integers(LO, HI + 1, size=s, dtype=np.int64).astype(np.int32)  # noqa: E731
        chans = [draw((ah, aw)), draw((rh, aw)), draw((htot, rw))]
    else:
        lap = lambda s: np.rint(rng.laplace(0, 40, size=s)).astype(np.int32)  # noqa: E731
        chans = [rng.integers(-3000, 3000, size=(ah, aw)).astype(np.int32), lap((rh, aw)), lap((htot, rw))]
    return chans, [(1, 1, 0, 1), (0, 1, 0, 1)]


# ---- RCT -----------------------------------------------------------------------------------------------------------------------------------
RCT_BEGIN_TYPES = [7 * p + 6 for p in range(6)]


@functools.lru_cache(maxsize=None)
def rct_planes(rct_type):
    v = np.random.default_rng(rct_type).integers(LO, HI + 1, size=(3, 19, 23), dtype=np.int64).astype(np.int32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def rct_five_channels():
    rng = np.random.default_rng(55)
    return [rng.integers(LO, HI + 1, size=(19, 23), dtype=np.int64).astype(np.int32) for _ in range(5)]


@functools.lru_cache(maxsize=None)
def rct_five_channels_squeezed():
    """five 37 x 41 channels behind one in-place H step and one in-place V step over all of them: (channels, plan)"""
    shapes = [(37, 41)] * 5
    sp = [(1, 1, 0, 5), (0, 1, 0, 5)]
    rng = np.random.default_rng(56)
    enc = synth.squeezed_shapes(shapes, sp)
    chans = [rng.integers(-70000, 70000, size=s).astype(np.int32) if i < 5 else np.rint(rng.laplace(0, 400, size=s)).astype(np.int32)
             for i, s in enumerate(enc)]
    return chans, sp
