"""CPU side of the device spline stage (include/jxlatte_amd.h: jxl_spline_arcs, jxl_stage_splines, jxl_planes_splines): the
library's host-only arc table against decoder.spline_arc_table bit for bit, the bracket model of tests/spline_ref.py, the
numpy restatement of fp_exp, and the tile binning. No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import spline_ref as R
from jxlatte_amd import _lib, abi, decoder, frontend, host

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sp(control, coeff_sigma0=6, quant_adjust=0, color=(120, 80, -60), sigma_rest=()):
    coeff = np.zeros((4, 32), np.int64)
    for c in range(3):
        coeff[c, 0], coeff[c, 1], coeff[c, 2] = color[c], color[c] // 2, -color[c] // 3
    coeff[3, 0] = coeff_sigma0
    for k, v in enumerate(sigma_rest):
        coeff[3, 1 + k] = v
    return dict(quant_adjust=quant_adjust, control=[(int(y), int(x)) for y, x in control], coeff=coeff.tolist())


ARC_CASES = {
    "one_point": ([_sp([(20, 30)])], 64, 96),
    "two_points": ([_sp([(5, 5), (40, 70)])], 64, 96),
    "repeated_points": ([_sp([(10, 10), (10, 10), (30, 50)]), _sp([(8, 9), (30, 40), (30, 40), (50, 20)]), _sp([(7, 7), (7, 7)])], 64, 96),
    "collinear": ([_sp([(10, 10), (20, 20), (30, 30), (40, 40)])], 64, 96),
    "sharp_bend": ([_sp([(10, 10), (50, 80), (11, 12), (52, 79)])], 64, 96),
    "outside_frame": ([_sp([(-40, -30), (20, 30), (100, 150)]), _sp([(-100, -100), (-90, -50)]), _sp([(63, 95), (64, 96), (80, 120)])], 64, 96),
    "quant_adjust_negative": ([_sp([(5, 5), (40, 70), (10, 90)], quant_adjust=-13)], 64, 96),
    "quant_adjust_positive": ([_sp([(5, 5), (40, 70), (10, 90)], quant_adjust=21)], 64, 96),
    "sigma_crosses_zero": ([_sp([(5, 5), (40, 70), (10, 90)], coeff_sigma0=1, sigma_rest=(4, -3, 2))], 64, 96),
    "sigma_zero": ([_sp([(5, 5), (40, 70)], coeff_sigma0=0)], 64, 96),
    "sigma_negative": ([_sp([(5, 5), (40, 70)], coeff_sigma0=-5)], 64, 96),
    "spline0_coefficients_for_all": ([_sp([(5, 5), (40, 70)]), _sp([(50, 5), (10, 70)], coeff_sigma0=12, color=(-500, 900, 10))], 64, 96),
    "random": (R.random_splines(3, 6, 100, 140, margin=30), 100, 140),
}


def _assert_same_table(splines, bcx, bcb, h, w):
    lib_t = host.spline_arcs(splines, bcx, bcb, h, w)
    py_t = decoder.spline_arc_table(splines, bcx, bcb, w, h)
    assert len(lib_t) == len(py_t), (len(lib_t), len(py_t))
    for i, (ay, ax, sigma, inv_sigma, vals, (x0, x1, y0, y1)) in enumerate(py_t):
        a = lib_t[i]
        mul = [F(F(F(0.25) * vals[c]) * sigma) for c in range(3)]
        exp = np.array([ay, ax, sigma, inv_sigma] + mul, F).view(np.uint32)
        got = np.array([a["y"], a["x"], a["sigma"], a["inv_sigma"]] + list(a["mul"]), F).view(np.uint32)
        assert np.array_equal(exp, got), (i, exp, got)
        assert (int(a["x0"]), int(a["x1"]), int(a["y0"]), int(a["y1"])) == (x0, x1, y0, y1), i
    return len(py_t)


@pytest.mark.parametrize("name", sorted(ARC_CASES))
def test_arc_table_of_the_library_equals_the_decoder_bit_for_bit(name):
    """jxl_spline_arcs (C++, host only) against decoder.spline_arc_table: positions, sigma, inv_sigma, mul, boxes, order"""
    splines, h, w = ARC_CASES[name]
    n = _assert_same_table(splines, 0.0, 1.0, h, w)
    _assert_same_table(splines, -0.125, 0.875, h, w)
    if name not in ("one_point", "sigma_zero", "sigma_negative"):  # (one point: arcLength 0 draws nothing)
        assert n > 0
    if name == "sigma_zero":  # sigma == 0 exactly: maxDist 0, a one-pixel box, 1 / sigma infinite, mul a signed zero
        t = host.spline_arcs(splines, 0.0, 1.0, h, w)
        assert len(t) > 50 and np.isinf(t["inv_sigma"]).all() and (t["mul"] == 0).all()
    if name == "repeated_points":
        # NaN knots make every distance of the walk NaN: each spline keeps its first sample and its last, the last with a NaN
        # arc length, hence NaN values and NaN mul at a finite position and in a finite box -- arcs that draw NaN
        t = host.spline_arcs(splines, 0.0, 1.0, h, w)
        assert n == 6 and int(np.isnan(t["mul"]).all(axis=1).sum()) == 3 and np.isfinite(t["y"]).all() and np.isfinite(t["x"]).all()


KNOT_CASES = {
    "distinct": [(5, 5), (40, 70), (10, 90)],
    "first_two_equal": [(10, 10), (10, 10), (30, 50)],
    "inner_two_equal": [(8, 9), (30, 40), (30, 40), (50, 20)],
    "inner_three_equal_in_a_longer_spline": [(5, 5), (20, 30), (20, 30), (20, 30), (40, 60), (12, 80)],
    "last_two_equal": [(10, 10), (20, 30), (20, 30)],
    "all_equal": [(7, 7), (7, 7)],
    "wrapping_extension": [(2000000000, -2000000000), (-2000000000, 2000000000)],
}


@pytest.mark.parametrize("name", sorted(KNOT_CASES))
def test_knots_of_the_library_equal_the_decoder_nan_and_inf_included(name):
    """Spline.upsampleControlPoints directly (a debug entry that needs no device) against decoder._spline_knots: the same
    bits, NaN where the decoder has NaN and the same infinity where it has one (repeated points divide by t[k+1] - t[k] = 0)"""
    cp = KNOT_CASES[name]
    uy, ux = decoder._spline_knots(cp)
    want = np.stack([np.array(uy, F), np.array(ux, F)])
    fn = _lib.load().jxl_debug_spline_knots
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    flat = np.array(cp, np.int32).ravel()
    n = fn(flat.ctypes.data, len(cp), None, None, 0)
    assert n == want.shape[1] == 16 * (len(cp) - 1) + 1
    got = np.zeros((2, n), F)
    assert fn(flat.ctypes.data, len(cp), got[0].ctypes.data, got[1].ctypes.data, n) == n
    assert ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all()
    bad = int(np.count_nonzero(~np.isfinite(want)))
    print("%s: %d knots, %d of their coordinates NaN or infinite" % (name, n, bad))
    assert (bad > 0) == ("equal" in name)
    assert fn(None, 2, None, None, 0) == abi.JXL_ERR_INVALID_ARGUMENT and fn(flat.ctypes.data, 0, None, None, 0) == abi.JXL_ERR_INVALID_ARGUMENT


def test_arc_table_of_wb_rainbow_read_through_the_front_end():
    data = open(os.path.join(ROOT, "tests", "golden", "samples", "wb-rainbow.jxl"), "rb").read()
    from oracle.pybackend import OracleBackend
    be = OracleBackend()
    fe = frontend.Frontend(data)
    seen = 0
    while True:
        fr = fe.next_frame(be.squeeze, be.rct)
        if fr is None:
            break
        if fr.has_splines:
            sp = fe.splines()
            h, w = fr.height * fr.upsampling, fr.width * fr.upsampling
            assert _assert_same_table(sp, fr.base_corr_x, fr.base_corr_b, h, w) > 0
            seen += len(sp)
    assert seen == 2


def test_arc_entry_argument_checks():
    lib = _lib.load()
    d, keep = abi.make_spline_desc([_sp([(1, 1), (5, 5)])], 0.0, 1.0)
    assert lib.jxl_spline_arcs(None, 8, 8, None, 0) == abi.JXL_ERR_INVALID_ARGUMENT
    assert lib.jxl_spline_arcs(C.byref(d), 0, 8, None, 0) == abi.JXL_ERR_INVALID_ARGUMENT
    assert lib.jxl_spline_arcs(C.byref(d), 8, 8, None, 4) == abi.JXL_ERR_INVALID_ARGUMENT
    d.n_splines = -1
    assert lib.jxl_spline_arcs(C.byref(d), 8, 8, None, 0) == abi.JXL_ERR_INVALID_ARGUMENT
    d.n_splines = 1
    keep[0][0] = 0  # a spline without control points
    assert lib.jxl_spline_arcs(C.byref(d), 8, 8, None, 0) == abi.JXL_ERR_INVALID_ARGUMENT
    e, _ = abi.make_spline_desc([], 0.0, 1.0)
    assert lib.jxl_spline_arcs(C.byref(e), 8, 8, None, 0) == 0
    # a spline that would need more arcs than the table may hold is a status, not an abort (turned away by the length of its
    # knot polyline, before any table grows)
    far, keep2 = abi.make_spline_desc([_sp([(0, 0), (0, 2000000000)])], 0.0, 1.0)
    assert lib.jxl_spline_arcs(C.byref(far), 8, 8, None, 0) == abi.JXL_ERR_OOM


# ---- the bracket model --------------------------------------------------------------------------------------------------------
MODEL_FRAMES = [
    ("thin", lambda: R.random_splines(11, 4, 90, 130, sigma=(2, 4)), 90, 130),
    ("thick_crossing", lambda: R.random_splines(12, 5, 90, 130, sigma=(15, 30)), 90, 130),
    ("edges_nonfinite", lambda: R.random_splines(13, 4, 60, 70, margin=25) + ARC_CASES["sigma_crosses_zero"][0], 60, 70),
]


@pytest.mark.parametrize("name,make,h,w", MODEL_FRAMES)
def test_bracket_model_mid_is_the_host_render_and_the_bracket_is_tight(name, make, h, w):
    """mid == render_splines bit for bit; lo <= mid <= hi; the bracket's width stays of the order of 2^-22 x the sum of
    |mul| |factor| over the arcs of a pixel (measured on these frames: at most 2.0 x that, printed)"""
    splines, planes = make(), R.random_planes(5, h, w)
    br = R.render_bracket(planes, splines, 0.0, 1.0)
    bufs = [p.copy() for p in planes]
    decoder.render_splines(bufs, splines, 0.0, 1.0, w, h)
    ok = (np.stack(bufs).view(np.uint32) == br["mid"].view(np.uint32)) | (np.isnan(np.stack(bufs)) & np.isnan(br["mid"]))
    assert ok.all()
    fin = np.isfinite(br["mid"])
    assert (br["lo"][fin] <= br["mid"][fin]).all() and (br["mid"][fin] <= br["hi"][fin]).all()
    assert br["touched"].any()
    width = (br["hi"].astype(np.float64) - br["lo"].astype(np.float64))
    width = np.where(fin, width, 0).max(axis=0)
    # one neighbour of E moves erf by <= 1 ulp(1) = 2^-23 ... 2^-24, factor by twice that, the term by twice again
    # (factor enters squared), and each of the roundings on the way adds its half ulp: 2^-22 per unit of |mul| |factor| covers the
    # exp share, the rest is ulp(sum) per addition
    scale = 2.0 ** -22 * br["weight"] + 8 * np.spacing(np.abs(br["mid"]).max(axis=0).astype(np.float64).astype(F)).astype(np.float64)
    ratio = float((width / scale)[br["touched"]].max())
    print("%s: largest bracket width %.3g, %.2f x (2^-22 sum|mul||factor| + 8 ulp)" % (name, float(width.max()), ratio))
    assert ratio <= 4.0


def _order_case():
    """a vertical line with sigma 1 and a huge Y value on planes that hold minus the drawn sum: every pixel cancels to ~0, so
    the order of the additions shows in the result at the scale of ulp(term) while the result itself is small"""
    sp = [_sp([(8, 20), (56, 20)], coeff_sigma0=3, color=(0, 2000000000, 0)), _sp([(56, 26), (8, 26)], coeff_sigma0=3)]
    zero = np.zeros((3, 64, 48), F)
    drawn = R.render_bracket(zero, sp, 0.0, 0.0)["mid"]
    return sp, (-drawn).astype(F), 64, 48


def _small_z_case():
    """a one-pixel-long horizontal spline with sigma ~ 2066: a pixel at distance 1 of an arc has z = (0.5 - SQRT_F) / sigma =
    7.1e-5 <= 1e-4, the small branch, where the two branches of MathHelper.erf differ most (a scan of 2.2e6 z in [-1e-4, 1e-4]:
    the other branch lies outside the bracket of the right one for 42 % of them, by up to 4.2e-7 = 2.3 widths of one erf)"""
    return [_sp([(16, 10), (16, 11)], coeff_sigma0=6200)], R.random_planes(9, 32, 32), 32, 32


@pytest.mark.parametrize("m", R.MUTATIONS)
def test_mutated_models_leave_the_bracket(m):
    """Each deliberately wrong variant of the model must leave [lo, hi] of the right one on at least one input. Margin = the
    largest distance outside the bracket in units of the largest bracket width of that frame. Measured:
        sqrt_sign 1.1e6   no_half 6.6e5   box_short 1.0e5   true_max 7.3e4   per_spline_coeff 1.3e6
    and these five must clear 100 widths. Two variants cannot be wide by construction, and are held to `outside at all`:
      reverse          reordering moves a pixel by roundings of its running sum, i.e. by ulps of its largest partial sum; the
                       bracket's width has the same origin (one ulp(1) per erf, scaled by the same terms), so on the
                       cancelling input the reversed sum lands 2.0 outside where the bracket is 3.3 wide (0.04 of the frame's
                       largest width), not hundreds.
      no_small_branch  for |z| <= 1e-4 both branches of MathHelper.erf are 1 - (~1) * E: they differ by up to 5.4e-7, a few
                       ulp(1), where a neighbouring E moves erf by one. On the input of _small_z_case, whose pixels next to
                       the arcs have z = 7.1e-5, 12 samples leave the bracket, by up to 0.48 widths. (An input whose
                       small-branch pixels all have |z| ~ 1e-8 shows nothing: there the branches agree.)
    These two margins are a few samples wide, so they must not hang on how a CPU's exp rounds: the model's exp is pinned
    (spline_ref.exp_f: long double, rounded once to float), and every other operation is an IEEE float operation."""
    sp = R.random_splines(1, 3, 120, 160, sigma=(3, 12))
    sp[1]["coeff"][3][0] += 7  # (per_spline_coeff needs splines that differ)
    splines, planes, h, w = {"reverse": _order_case, "no_small_branch": _small_z_case}.get(
        m, lambda: (sp, R.random_planes(2, 120, 160), 120, 160))()
    bcb = 0.0 if m == "reverse" else 1.0
    br = R.render_bracket(planes, splines, 0.0, bcb)
    bad = R.render_bracket(planes, splines, 0.0, bcb, mut=m)["mid"]
    out = np.maximum(bad.astype(np.float64) - br["hi"], br["lo"].astype(np.float64) - bad)
    out = np.where(np.isfinite(out), out, -np.inf)
    width = (br["hi"].astype(np.float64) - br["lo"])
    margin = float(out.max() / width[np.isfinite(width)].max())
    print("mutation %-18s leaves the bracket by %.3g widths" % (m, margin))
    assert margin > (0 if m in ("reverse", "no_small_branch") else 100), (m, margin)


# ---- fp_exp -------------------------------------------------------------------------------------------------------------------
def test_fp_exp_header_constants():
    hi, lo, q = R.fp_exp_coeffs()
    l2e = np.longdouble(1) / np.log(np.longdouble(2))
    assert hi == float(l2e) and abs(np.longdouble(lo) - (l2e - np.longdouble(hi))) < 1e-19
    assert len(q) == 14


def test_fp_exp_restatement_against_long_double_and_a_correctly_rounded_float():
    """relative error in double below 1e-15 over [-110, 90] (the kernel sees about -1e4 .. 3; float results overflow from 88.7
    on); the float result against a correctly rounded one (long double exp, rounded once to float) over 1.4e6 float
    arguments, subnormal results, underflow and overflow included: at most 1 in 10^4 may differ (measured: 0)"""
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.uniform(-110, 3, 600000), rng.uniform(-104, -87, 200000), -10 ** rng.uniform(-6, 4, 300000),
                         rng.uniform(-1e-3, 3, 100000), rng.uniform(3, 90, 200000),
                         [0.0, -0.0, -103.97, -103.98, -200.0, -1e4, -3e4, 88.7, 89.0, 90.0]])
    xs = xs.astype(F).astype(np.float64)
    got = R.fp_exp(xs)
    ref = np.exp(xs.astype(np.longdouble))
    ok = ref > np.longdouble(1e-300)
    rel = np.abs((got[ok].astype(np.longdouble) - ref[ok]) / ref[ok])
    print("fp_exp: max relative error %.3g over %d arguments" % (float(rel.max()), int(ok.sum())))
    assert float(rel.max()) < 1e-15
    with np.errstate(over="ignore", under="ignore"):
        f_got, f_ref = got.astype(F), ref.astype(F)
    diff = int(np.count_nonzero(f_got.view(np.uint32) != f_ref.view(np.uint32)))
    print("fp_exp: %d of %d float results differ from the correctly rounded one" % (diff, xs.size))
    assert diff * 10000 <= xs.size
    assert (f_got[xs < -104.0] == 0).all() and np.count_nonzero((f_got > 0) & (f_got < np.finfo(F).tiny)) > 1000
    sp = np.array([-np.inf, np.inf, np.nan])
    r = R.fp_exp(sp)
    assert r[0] == 0 and r[1] == np.inf and np.isnan(r[2])


def test_fp_exp_on_the_arguments_the_test_frames_produce():
    """the == mid cap of the GPU tests (1 in 10^4) rests on this: numpy's exp and the restatement give the same float"""
    n = diff = 0
    for _, make, h, w in MODEL_FRAMES:
        a = R.render_bracket(R.random_planes(5, h, w), make(), 0.0, 1.0, collect_args=True)["args"].astype(np.float64)
        a = a[~np.isnan(a)]
        with np.errstate(all="ignore"):
            diff += int(np.count_nonzero(R.fp_exp(a).astype(F) != np.exp(a).astype(F)))
        n += a.size
    print("fp_exp on the frames' arguments: %d of %d differ from numpy's exp" % (diff, n))
    assert n > 100000 and diff * 10000 <= n


# ---- binning ------------------------------------------------------------------------------------------------------------------
def _lib_bins(boxes, h, w):
    lib = _lib.load()
    arcs = np.zeros(len(boxes), abi.SPLINE_ARC_DTYPE)
    for i, b in enumerate(boxes):
        arcs[i]["x0"], arcs[i]["x1"], arcs[i]["y0"], arcs[i]["y1"] = b
    fn = lib.jxl_debug_spline_bins
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    nl = C.c_int64()
    nt = fn(arcs.ctypes.data, len(boxes), h, w, None, None, None, 0, 0, C.byref(nl))
    assert nt >= 0
    tile, start, lst = np.zeros(max(nt, 1), np.int32), np.zeros(nt + 1, np.int32), np.zeros(max(nl.value, 1), np.int32)
    assert fn(arcs.ctypes.data, len(boxes), h, w, tile.ctypes.data, start.ctypes.data, lst.ctypes.data, nt, nl.value, C.byref(nl)) == nt
    return list(tile[:nt]), list(start), list(lst[:nl.value])


@pytest.mark.parametrize("h,w", [(1, 1), (7, 300), (257, 255), (64, 64)])
def test_tile_lists_of_the_library_against_the_restatement_and_brute_force(h, w):
    """the host's binning (a debug entry that needs no device) == spline_ref.bin_tiles == brute force over pixels: order kept,
    every arc in every tile its box meets, no empty tile listed; boxes on tile edges, one-pixel boxes, the whole frame"""
    rng = np.random.default_rng(h * 1000 + w)
    boxes = [(0, w - 1, 0, h - 1), (0, 0, 0, 0), (w - 1, w - 1, h - 1, h - 1)]
    for x in (31, 32, 63, 64):
        for y in (7, 8, 15, 16):
            if x < w and y < h:
                boxes += [(x, x, y, y), (max(0, x - 1), x, max(0, y - 1), y), (x, min(w - 1, x + 32), y, min(h - 1, y + 8))]
    for _ in range(40):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        boxes.append((x0, min(w - 1, x0 + int(rng.integers(0, 90))), y0, min(h - 1, y0 + int(rng.integers(0, 40)))))
    tiles, start, lst, (tiles_x, tiles_y) = R.bin_tiles(boxes, h, w)
    assert (tiles, start, lst) == _lib_bins(boxes, h, w)
    # brute force: the arcs whose box holds at least one pixel of the tile
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            want = [i for i, (x0, x1, y0, y1) in enumerate(boxes)
                    if x0 < (tx + 1) * R.TILE_W and x1 >= tx * R.TILE_W and y0 < (ty + 1) * R.TILE_H and y1 >= ty * R.TILE_H]
            t = ty * tiles_x + tx
            if want:
                k = tiles.index(t)
                assert lst[start[k]:start[k + 1]] == want
            else:
                assert t not in tiles
