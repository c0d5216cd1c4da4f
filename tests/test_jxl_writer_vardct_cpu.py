"""The VarDCT route pinned to known coefficients, on the CPU: every case of jxl_writer_vardct_cases.py is written by
jxl_writer_vardct.py, read by the front-end -- whose every integer must be the SOURCE's -- and decoded on the oracle backend, whose
planes at the cut points idct / gab / epf / xyb must be the float64 models' of the SOURCE within K u (A + |model|). Then the
discrimination: nine writers that compute a context or a placement the wrong way, three expectations made the wrong way."""
import math

import numpy as np
import pytest

import jxl_writer_vardct as V
import jxl_writer_vardct_cases as C
import jxl_writer_vardct_run as R
import quant_weights_ref as Q
import vardct_ref64 as M
from jxlatte_amd import frontend

F = np.float32
NAMES = sorted(C.CASES)


@pytest.fixture(scope="module")
def backend(orc):
    from oracle.pybackend import OracleBackend
    return OracleBackend()


_decoded = {}


def decoded(name, backend):
    if name not in _decoded:
        _decoded[name] = R.decode(C.encoded(name), backend)
    return _decoded[name]


# ---- the front-end's views -------------------------------------------------------------------------------------------------------
def sparse_to_dense(entries, wide, shape):
    """jxf_get_coeffs_sparse: (y << 8 | x, value) pairs, or value << 16 | y << 8 | x where every value fits int16"""
    e = np.asarray(entries, np.uint32)
    if wide:
        pos, val = e[0::2], e[1::2].view(np.int32)
    else:
        pos, val = e & np.uint32(0xFFFF), (e.view(np.int32) >> 16)
    out = np.zeros(shape, np.int64)
    out[(pos >> 8).astype(np.int64), (pos & 0xFF).astype(np.int64)] = val
    return out, int(e.size // (2 if wide else 1))


def views_differ(data, src):
    """None when every integer the front-end hands out is the SOURCE's; else what differs first. (lf_index has no view of its own:
    it is held through the block context -- a wrong one reads the block's symbols under another cluster, case block_ctx.)"""
    geo, p = V.geometry(src), C.params_of(src)
    try:
        fe = frontend.Frontend(data)
        fr = fe.next_frame()
    except frontend.FrontendError as e:
        return "rejected: %s" % e
    sy, sx = src.get("shift_y", [0] * 3), src.get("shift_x", [0] * 3)
    shifts = list(src.get("pass_shifts", [])) + [0]
    xyb = src.get("xyb", True)
    info = fe.image
    want = dict(type=0, encoding=0, do_ycbcr=int(src.get("do_ycbcr", False)), upsampling=1, group_dim=256,
                xqm=src.get("xqm", 3) if xyb else 2, bqm=src.get("bqm", 2) if xyb else 2, lf_level=0,
                flags=V.FLAG_SKIP_ADAPTIVE_LF_SMOOTHING if src.get("skip_smoothing", False) else 0, num_passes=len(shifts),
                x0=0, y0=0, width=-(-src["width"] // (1 << max(sx))) << max(sx), height=-(-src["height"] // (1 << max(sy))) << max(sy),
                padded_width=geo["pw"], padded_height=geo["ph"], is_last=1, gab=p.gab, epf_iters=p.epf_iters,
                num_groups=geo["num_groups"], num_lf_groups=geo["num_lf_groups"], group_cols=geo["cols"], lf_group_cols=geo["lcols"],
                global_scale=src["global_scale"], quant_lf=src["quant_lf"], colour_factor=p.color_factor, x_factor_lf=p.x_factor_lf,
                b_factor_lf=p.b_factor_lf, quant_all_default=int(src.get("quant") is None), num_hf_presets=src.get("num_presets", 1),
                num_patches=0, has_splines=0, has_noise=0, num_modular_channels=0)
    for k, v in want.items():
        if getattr(fr, k) != v:
            return "FrameInfo.%s: %r for %r" % (k, getattr(fr, k), v)
    floats = dict(jpeg_up_y=sy, jpeg_up_x=sx, pass_shift=shifts, gab1=p.gab_w1, gab2=p.gab_w2, epf_sharp_lut=p.epf_sharp_lut,
                  epf_channel_scale=p.epf_channel_scale, scaled_dequant=p.scaled_dequant)
    scal = dict(epf_pass0_sigma=p.epf_pass0_sigma_scale, epf_pass2_sigma=p.epf_pass2_sigma_scale, epf_border_sad_mul=p.epf_border_sad_mul,
                base_corr_x=p.base_corr_x, base_corr_b=p.base_corr_b)
    for k, v in floats.items():
        if list(getattr(fr, k))[:len(v)] != [type(getattr(fr, k)[0])(x) for x in v]:
            return "FrameInfo.%s: %r for %r" % (k, list(getattr(fr, k)), v)
    for k, v in scal.items():
        if F(getattr(fr, k)) != F(v):
            return "FrameInfo.%s: %r for %r" % (k, getattr(fr, k), v)
    if bool(info.xyb_encoded) != xyb or (info.width, info.height) != (src["width"], src["height"]):
        return "ImageInfo"
    if [F(v) for v in info.quant_bias] != p.quant_bias or F(info.quant_bias_numerator) != p.quant_bias_numerator or \
            [F(v) for v in info.opsin_matrix] != p.opsin_matrix or [F(v) for v in info.opsin_bias] != p.opsin_bias:
        return "ImageInfo opsin"
    for i, g in enumerate(src["lfgroups"]):
        v = fe.lfgroup(i)
        blocks = sorted(g["blocks"])
        sel = np.zeros(np.asarray(g["hf_mul"]).shape, np.int64)
        for y, x, t in blocks:
            sel[y:y + V.cells(t)[0], x:x + V.cells(t)[1]] = t
        pairs = [("dct_select", sel), ("hf_mul", g["hf_mul"]), ("sharpness", g["sharpness"]), ("x_from_y", g["x_from_y"]),
                 ("b_from_y", g["b_from_y"]), ("block_yx", np.array([(y, x) for y, x, _ in blocks]))]
        # lf_quant is handed out in buffer order X, Y, B: channel cMap[i] of the stream is buffer i (LFCoefficients.java:39, :66-67)
        pairs += [("lf_quant %d" % c, g["lf_quant"][c]) for c in range(3)]
        for k, a in pairs:
            got = v["lf_quant"][int(k[-1])] if k.startswith("lf_quant") else v[k]
            if got.shape != np.asarray(a).shape or not np.array_equal(got, a):
                return "LF group %d %s" % (i, k)
        if v["extra_precision"] != g.get("extra_precision", 0) or v["n_blocks"] != len(blocks):
            return "LF group %d extra_precision / n_blocks" % i
    if src.get("quant") is not None:
        for i, q in enumerate(src["quant"]):
            v = fe.quant_params(i)
            if v["mode"] != q["mode"] or (q["mode"] == 7 and F(v["denominator"]) != F(q["denominator"])):
                return "quant %d mode / denominator" % i
            for k in ("dct", "par", "p44"):
                a, b = v[k], q[k] if q["mode"] else None
                if q["mode"] == 3 and k == "p44":
                    continue
                if (a is None) != (b is None) or (a is not None and not np.array_equal(a, np.asarray(b, F))):
                    return "quant %d %s" % (i, k)
    for k, s in enumerate(shifts):
        for grp in range(geo["num_groups"]):
            gy, gx = grp // geo["cols"], grp % geo["cols"]
            dense, sparse = fe.coeffs(k, grp), fe.coeffs_sparse(k, grp)
            for c in range(3):
                a = np.asarray(src["coeff_passes"][k][c], np.int64) << s
                a = a[(gy * 256) >> sy[c]:((gy + 1) * 256) >> sy[c], (gx * 256) >> sx[c]:((gx + 1) * 256) >> sx[c]]
                if dense[c].shape != a.shape or not np.array_equal(dense[c], a):
                    return "coefficients pass %d group %d channel %d" % (k, grp, c)
                sd, n = sparse_to_dense(sparse[c][0], sparse[c][1], sparse[c][2])
                if sparse[c][2] != a.shape or not np.array_equal(sd, a) or n != int((a != 0).sum()):
                    return "sparse coefficients pass %d group %d channel %d" % (k, grp, c)
    if fe.next_frame() is not None:
        return "a second frame"
    return None


@pytest.mark.parametrize("name", NAMES)
def test_front_end_hands_out_the_source(name):
    assert views_differ(C.encoded(name), C.source(name)) is None


def test_cases_are_what_they_claim():
    """the properties the cases are there for, checked on the SOURCE"""
    s = C.source
    assert sorted(t for n in NAMES if n.startswith("type_") for _, _, t in s(n)["lfgroups"][0]["blocks"]) == list(range(27))
    rag = s("ragged_67x83")
    assert V.padded_size(rag) == (88, 72) and len({t for _, _, t in rag["lfgroups"][0]["blocks"]}) >= 8
    taken = {}  # both branches of placeBlock: an occupied run left by an earlier, taller block; too wide for the rest of the line
    V.place_blocks(sorted(rag["lfgroups"][0]["blocks"]), 11, 9, taken)
    assert taken.get("occupied", 0) > 0 and taken.get("too_wide", 0) > 0, taken
    g = s("groups_264x264")
    assert V.geometry(g)["num_groups"] == 4 and g["num_presets"] == 2 and sorted(set(g["presets"][0])) == [0, 1]
    edge = {(y, x) for y, x, t in g["lfgroups"][0]["blocks"]}
    assert {(31, 31), (32, 31), (31, 32), (32, 32)} <= {(y + V.cells(t)[0] - 1 if y < 32 else y, x + V.cells(t)[1] - 1 if x < 32 else x)
                                                          for y, x, t in g["lfgroups"][0]["blocks"]} and edge
    assert V.geometry(s("two_lf_groups_2056x16"))["num_lf_groups"] == 2
    b = s("block_ctx")
    hf, thr = np.asarray(b["lfgroups"][0]["hf_mul"]), b["block_ctx"]["qf_thresholds"]
    assert hf.min() <= thr[0] < np.median(hf) and hf.max() > thr[1]
    for i in range(3):
        q = np.asarray(b["lfgroups"][0]["lf_quant"][i])
        assert all(q.min() <= t < q.max() for t in b["block_ctx"]["lf_thresholds"][i])
    so = {t for _, _, t in s("shared_order")["lfgroups"][0]["blocks"]}
    assert {6, 7} <= so and V.order_id(6) == V.order_id(7) == 4 and V.vertical(6) and not V.vertical(7)
    assert min(s("lf_rough")["_lf_regimes"]) >= 0.10 and s("lf_rough")["lfgroups"][0]["extra_precision"] == 3
    co = s("corr")["lfgroups"][0]
    assert np.asarray(co["x_from_y"]).shape == (3, 3) and len(np.unique(co["x_from_y"])) >= 8 and len(np.unique(co["b_from_y"])) >= 8
    assert any((y % 8) + V.cells(t)[0] > 8 or (x % 8) + V.cells(t)[1] > 8 for y, x, t in co["blocks"])  # a block across two tiles
    seen = {(q["mode"], i) for n in C.QUANT_CASES for i, q in enumerate(s(n)["quant"])}
    assert {(m, i) for m in range(1, 8) for i in range(17) if Q.legal(i, m)} <= seen and any(m == 0 for m, _ in seen)
    for n in ("epf1", "epf3", "epf2_default"):  # the filter filters: a quarter of the samples it does not copy move by > 1000 u (A + |x|)
        (e, _), (g, ga), p = C.expected(n, R.EPF), C.expected(n, R.GAB), C.params_of(s(n))
        sig = M.epf_sigma(s(n)["lfgroups"][0]["hf_mul"], s(n)["lfgroups"][0]["sharpness"], float(p.global_scale_f), [float(v) for v in p.epf_sharp_lut])
        filtered = np.repeat(np.repeat(sig <= M.COPY_THRESHOLD, 8, 0), 8, 1)
        assert 0.5 < filtered.mean() < 1.0 and (np.abs(e - g) > 1000 * M.U * (ga + np.abs(g)))[:, filtered].mean() > 0.25, n
        assert len(np.unique(s(n)["lfgroups"][0]["sharpness"])) >= 6  # (25 cells)
    for n in NAMES:
        assert C.conditions(s(n)) is None, n
        for cm, cfgs in s(n)["hf_clusters"]:
            assert len(cfgs) >= 4 and len(set(cfgs)) == len(cfgs)


# ---- the pixel cuts ----------------------------------------------------------------------------------------------------------------
def cut_ratios(name, out):
    """[(cut, stage set, ratio, K)] of one decode"""
    rows = []
    if "idct" in out:
        rows = [(cut, stage, R.ratio(out[cut], name, stage), R.bound(name, stage)) for cut, stage, _ in R.CUTS]
    fs = R.final_stage(name)
    if fs is not None:
        rows.append(("xyb", fs, R.ratio(out["xyb"], name, fs), R.bound(name, fs)))
    return rows


@pytest.mark.parametrize("name", NAMES)
def test_oracle_decode_is_the_model_at_every_cut(name, backend):
    for cut, stage, r, k in cut_ratios(name, decoded(name, backend)):
        print("%s %s (stages %d): needs K = %.2f of %d" % (name, cut, stage, r, k))
        assert r <= k, (name, cut, r, k)


def test_measured_rows_are_twice_the_largest_ratio(backend):
    """the rows of the table that are measured, not derived, for the classes and stage sets these cases add: K = ceil(2 x the largest
    oracle-vs-model ratio over the cases of the class). Rows the table already had are only held (<=)."""
    worst = {}
    for name in NAMES:
        src = C.source(name)
        for cut, stage, r, _ in cut_ratios(name, decoded(name, backend)):
            key = R.measured_row(src, stage)
            if key is not None:
                worst[key] = max(worst.get(key, 0.0), r)
    for key, r in sorted(worst.items()):
        print("row %s: largest %.2f, K %d" % (key, r, R.MEASURED[key]))
        if key in R.FILLED:
            assert R.MEASURED[key] == math.ceil(2 * r), (key, r)
        else:
            assert r <= R.MEASURED[key], (key, r)
    assert set(R.FILLED) <= set(worst)


# ---- discrimination ------------------------------------------------------------------------------------------------------------
def test_every_writer_variant_is_listed():
    assert set(C.VARIANT_CASES) == set(V.VARIANTS) and len(V.VARIANTS) == 9


@pytest.mark.parametrize("variant", V.VARIANTS)
def test_a_wrong_writer_is_rejected_or_read_back_differently(variant):
    for name in C.VARIANT_CASES[variant]:
        data = C.encoded(name, variant)
        assert data != C.encoded(name), (variant, name)
        why = views_differ(data, C.source(name))
        print("%s on %s: %s" % (variant, name, why))
        assert why is not None, (variant, name)


LARGE = 100  # "a large multiple of K"


def _swapped_qm(name):
    src = dict(C.source(name))
    src["xqm"], src["bqm"] = src["bqm"], src["xqm"]
    return C.model_frame(C.source(name), params=C.params_of(src))


def _default_weights(name):
    t = Q.tables(Q.default_params())
    return C.model_frame(C.source(name), weights=(t.w, t.offs))


CASE_VARIANTS = {
    "scale_factor with xqm and bqm exchanged": (_swapped_qm, ("xqm0_bqm7",)),
    "extra_precision ignored": (lambda name: C.model_frame(C.source(name), extra_precision=0), ("lf_rough",)),
    "default weights for the custom ones": (_default_weights, C.QUANT_CASES),
}


@pytest.mark.parametrize("what", sorted(CASE_VARIANTS))
def test_a_wrong_expectation_leaves_the_bound(what, backend):
    make, names = CASE_VARIANTS[what]
    for name in names:
        x, a, _ = M.decode(make(name), R.IDCT)
        r = R.ratio(decoded(name, backend)["idct"], name, R.IDCT, model=(x, a))
        k = R.bound(name, R.IDCT)
        print("%s on %s: %.4g K" % (what, name, r / k))
        assert r > LARGE * k, (what, name, r, k)
