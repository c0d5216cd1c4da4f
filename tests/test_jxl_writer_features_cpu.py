"""Patches and splines of a VarDCT frame, and splines and noise of a Modular one, pinned to known pixels on the CPU: every case of
jxl_writer_features_cases.py is written by the two writers, read by the front-end -- whose every integer must be the SOURCE's --
and decoded on the oracle backend, whose planes at the cut after the EPF, at the cut after the colour transforms, in the reference
slots and in the image must be the float64 models' of the SOURCE within K u (A + |model|). Then the discrimination: eight writers that
are wrong about the features' fields or their place in LfGlobal, twelve expectations made the wrong way. The decoder's two spline arc
tables are held to the float64 model's, the independent witness tests/spline_ref.py lacks."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import jxl_writer as W
import jxl_writer_features_cases as FC
import jxl_writer_features_run as FR
import jxl_writer_vardct as V
import spline_model64 as SM
from jxlatte_amd import decoder, frontend, host
from jxlatte_amd.decoder import JXLDecoder, UnsupportedOperationException

F = np.float32
U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jxl_writer_features_sha256.json")


@pytest.fixture(scope="module")
def backend(orc):
    from oracle.pybackend import OracleBackend
    return OracleBackend()


_decoded = {}


def decoded(name, backend):
    if name not in _decoded:
        _decoded[name] = FR.decode(FC.encoded(name), backend)
    return _decoded[name]


# ---- the front-end's views -------------------------------------------------------------------------------------------------------
def views_differ(data, case):
    """None when every integer the front-end hands out of the features and of what lies behind them in the stream is the
    SOURCE's; else what differs first"""
    try:
        fe = frontend.Frontend(data)
        for i, src in enumerate(case["frames"]):
            fr = fe.next_frame()
            if fr is None:
                return "frame %d is missing" % i
            modular = FC.is_modular(src)
            ftype = src.get("type", W.REGULAR)
            normal = ftype in (W.REGULAR, W.SKIP_PROGRESSIVE)
            noise, sp, patches = src.get("noise"), src.get("splines"), src.get("patches") or []
            flags = (V.FLAG_NOISE if noise is not None else 0) | (V.FLAG_PATCHES if patches else 0) | (V.FLAG_SPLINES if sp else 0)
            want = dict(type=ftype, encoding=int(modular), flags=flags, has_splines=int(bool(sp)), num_patches=len(patches),
                        has_noise=int(noise is not None), save_before_ct=int(src.get("save_before_ct", False)),
                        save_as_reference=src.get("save_as_reference", 0), is_last=int(src.get("is_last", True) if normal else False),
                        upsampling=src.get("upsampling", 1))
            for k, v in want.items():
                if getattr(fr, k) != v:
                    return "frame %d FrameInfo.%s: %r for %r" % (i, k, getattr(fr, k), v)
            if noise is not None and [F(v) for v in fr.noise] != [F(v) / F(1024) for v in noise]:  # LFGlobal.java:58
                return "frame %d FrameInfo.noise: %r for %r" % (i, list(fr.noise), noise)
            got = fe.splines()
            if len(got) != (len(sp["splines"]) if sp else 0):
                return "frame %d: %d splines" % (i, len(got))
            for k, g in enumerate(got):
                s = sp["splines"][k]
                if g["quant_adjust"] != sp["quant_adjust"]:
                    return "frame %d spline %d quant_adjust: %r" % (i, k, g["quant_adjust"])
                if np.asarray(g["control"]).tolist() != [[y, x] for x, y in s["control"]]:  # absolute points, (y, x)
                    return "frame %d spline %d control points: %r for %r" % (i, k, np.asarray(g["control"]).tolist(), s["control"])
                if np.asarray(g["coeff"]).tolist() != [list(c) for c in s["coeff"]]:
                    return "frame %d spline %d coefficients" % (i, k)
            for k, p in enumerate(patches):
                g = fe.patch(k)
                if (g["ref"], g["x0"], g["y0"], g["w"], g["h"]) != (p["ref"], p["x0"], p["y0"], p["width"], p["height"]):
                    return "frame %d patch %d header" % (i, k)
                if np.asarray(g["positions"]).tolist() != [[y, x] for x, y in p["positions"]]:
                    return "frame %d patch %d positions: %r for %r" % (i, k, np.asarray(g["positions"]).tolist(), p["positions"])
                blend = [[[b["mode"], b.get("alpha", 0), int(b.get("clamp", False))] for b in row] for row in p["blend"]]
                if np.asarray(g["blend"]).tolist() != blend:
                    return "frame %d patch %d blend" % (i, k)
            # what lies behind the features in LfGlobal and after it: a reader that lost its place shows here
            if modular:
                for c, plane in enumerate(src["planes"]):
                    if not np.array_equal(np.asarray(fe.modular_channel(c)[0]), plane):
                        return "frame %d channel %d" % (i, c)
            else:
                if (fr.global_scale, fr.quant_lf) != (src["global_scale"], src["quant_lf"]):
                    return "frame %d global_scale / quant_lf" % i
                v = fe.lfgroup(0)
                if not np.array_equal(v["hf_mul"], src["lfgroups"][0]["hf_mul"]):
                    return "frame %d hf_mul" % i
                geo = V.geometry(src)
                for grp in range(geo["num_groups"]):
                    gy, gx = grp // geo["cols"], grp % geo["cols"]
                    dense = fe.coeffs(0, grp)
                    for c in range(3):
                        a = np.asarray(src["coeff_passes"][0][c], np.int64)[gy * 256:(gy + 1) * 256, gx * 256:(gx + 1) * 256]
                        if dense[c].shape != a.shape or not np.array_equal(dense[c], a):
                            return "frame %d coefficients group %d channel %d" % (i, grp, c)
        if fe.next_frame() is not None:
            return "a frame too many"
    except frontend.FrontendError as e:
        return "rejected: %s" % e
    return None


@pytest.mark.parametrize("name", FC.NAMES)
def test_front_end_hands_out_the_source(name):
    assert views_differ(FC.encoded(name), FC.case(name)) is None


def test_the_cases_encode_to_the_bytes_recorded():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(FC.NAMES)
    for name in FC.NAMES:
        assert hashlib.sha256(FC.encoded(name)).hexdigest() == want[name], name


def test_write_patches_without_clusters_writes_the_bytes_it_wrote():
    """the flat one-cluster form is untouched by the `clusters` key: the same symbols through write_symbols"""
    p = FC.case("patches_modref_72x64")["frames"][1]["patches"]
    a, b = W.BitWriter(), W.BitWriter()
    W.write_patches(a, p, 0)
    W.write_entropy_header(b, 10)
    syms = [len(p)]
    for q in p:
        syms += [q["ref"], q["x0"], q["y0"], q["width"] - 1, q["height"] - 1, len(q["positions"]) - 1]
        px = py = 0
        for j, (x, y) in enumerate(q["positions"]):
            syms += [x, y] if j == 0 else [int(W.pack_signed(x - px)), int(W.pack_signed(y - py))]
            px, py = x, y
            m = q["blend"][j][0]
            syms += [m["mode"]] + ([int(m.get("clamp", False))] if m["mode"] > 2 else [])
    W.write_symbols(b, syms)
    assert a.tobytes() == b.tobytes()


def test_cases_are_what_they_claim():
    """the properties the cases are there for, checked on the SOURCE and the models; prints the observed condition figures"""
    for name in FC.NAMES:
        c, m = FC.case(name), FC.expected(name)
        assert FC.conditions(c, m) is None and not m["undecided"], name
        print(name, [f["figures"] for f in m["frames"]])
        for fr in c["frames"]:
            if fr.get("splines"):
                cm, cfgs = fr["splines"]["clusters"]
                assert len(cm) == 6 and len(cfgs) >= 3 and len(set(cfgs)) == len(cfgs)
            if fr.get("patches"):
                cm, cfgs = fr["patch_clusters"]
                assert len(cm) == 10 and len(cfgs) >= 4 and len(set(cfgs)) == len(cfgs)
    s = FC.case("splines_40x40")["frames"][0]["splines"]["splines"]
    assert [len(p["control"]) for p in s] == [2, 3, 5] and len({json.dumps(p["coeff"]) for p in s}) == 3
    assert [len(p["control"]) for p in FC.case("splines_one_point")["frames"][0]["splines"]["splines"]] == [3, 1, 4]
    assert FC.case("splines_quant_adjust_pos")["frames"][0]["splines"]["quant_adjust"] == 5
    assert FC.case("splines_quant_adjust_neg")["frames"][0]["splines"]["quant_adjust"] == -7
    co = FC.case("splines_corr")["frames"][0]
    assert co["corr"]["base_x"] != 0.0 and co["corr"]["base_b"] != 1.0
    assert all(any(p["coeff"][3][1:]) for p in co["splines"]["splines"])
    big = FC.case("splines_264x264")["frames"][0]
    assert V.geometry(big)["num_groups"] == 4
    pts = [pt for p in big["splines"]["splines"] for pt in p["control"]]
    assert any(x < 0 for x, y in pts) and any(y < 0 for x, y in pts) and any(x >= 264 for x, y in pts) and any(y >= 264 for x, y in pts)
    assert min(big["splines"]["splines"][1]["control"][0]) < 0  # a later spline's start position is negative
    table, _ = SM.arc_table(big["splines"], 0.0, 1.0, 264, 264, clip=False)
    boxes = np.array([t["box"] for t in table])
    assert (boxes[:, 0] < 0).any() and (boxes[:, 1] > 263).any() and (boxes[:, 2] < 0).any() and (boxes[:, 3] > 263).any()  # every edge clips
    assert any(t["box"][0] < 256 <= t["box"][1] for t in table) and any(t["box"][2] < 256 <= t["box"][3] for t in table)  # across the group lines
    up = FC.case("splines_up2_19x15_of_37x29")["frames"][0]
    assert V.image_size(up) == (29, 37) and (2 * up["height"], 2 * up["width"]) == (30, 38)
    e = FC.case("splines_epf3_gab")["frames"][0]
    assert e["epf_iters"] == 3 and e["gab"]
    pm = FC.case("patches_modref_72x64")
    ref, fr = pm["frames"]
    assert ref["planes"][0].shape == (20, 24) and ref["type"] == W.REFERENCE_ONLY and ref["save_before_ct"] and ref["save_as_reference"] == 1
    pos = [(x, y, p["width"], p["height"], b[0]) for p in fr["patches"] for (x, y), b in zip(p["positions"], p["blend"])]
    assert len(fr["patches"]) == 3 and len(pos) == 7 and {b["mode"] for *_, b in pos} == {0, 2, 3, 4}
    assert {(b["mode"], b.get("clamp", False)) for *_, b in pos} >= {(3, True), (3, False), (4, True), (4, False)}
    assert any(x + w == 72 and y + h == 64 for x, y, w, h, _ in pos)
    (x0, y0, w, h, _), (x1, y1, _, _, _) = pos[0], pos[1]
    assert abs(x0 - x1) < w and abs(y0 - y1) < h  # two positions overlap
    g = FC.case("patches_264x264")["frames"][1]
    cells = {(x // 256, y // 256) for p in g["patches"] for x, y in p["positions"]} | \
        {((x + p["width"] - 1) // 256, (y + p["height"] - 1) // 256) for p in g["patches"] for x, y in p["positions"]}
    assert cells == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(x < 256 <= x + p["width"] - 1 for p in g["patches"] for x, y in p["positions"])
    assert any(y < 256 <= y + p["height"] - 1 for p in g["patches"] for x, y in p["positions"])
    v0, v1 = FC.case("patches_vardct_ref")["frames"]
    assert not v0["is_last"] and v0["save_as_reference"] == 2 and v0["save_before_ct"] and {p["ref"] for p in v1["patches"]} == {2}
    a0, a1 = FC.case("patches_ref_after_ct")["frames"]
    assert not a0["is_last"] and a0["save_as_reference"] == 1 and not a0["save_before_ct"] and {p["ref"] for p in a1["patches"]} == {1}
    assert len(FC.case("patches_of_an_empty_slot_vardct")["frames"]) == 1
    assert FC.case("patches_up2")["frames"][1]["upsampling"] == 2
    ab0, ab1 = FC.case("patches_alpha_blend")["frames"]
    assert len(ab0["planes"]) == 4 and len(ab1["extra"]) == 1 and ab1["splines"]
    assert {(row[0]["mode"], row[1]["mode"]) for p in ab1["patches"] for row in p["blend"]} == {(2, 0), (3, 3), (3, 0), (4, 0), (0, 3)}
    ch = FC.case("patches_chain_40x40")["frames"]
    assert ch[1]["patches"] and ch[1]["save_before_ct"] and ch[1]["save_as_reference"] == 2 and {p["ref"] for p in ch[2]["patches"]} == {2}
    (nu,) = FC.case("mod_rgb8_noise_up2")["frames"]
    assert nu["upsampling"] == 2 and nu["noise"] is not None and not FC.case("mod_rgb8_noise_up2")["image"]["xyb"]
    assert max(int(p.max()) for p in nu["planes"][:2]) > 255  # (what brings 3 (G + R) to the strength's upper clamp)
    allof = FC.case("patches_splines_noise_72x64")["frames"][1]
    assert allof["patches"] and allof["splines"] and allof["noise"] is not None


@pytest.mark.parametrize("name", [n for n in FC.NAMES if any(f.get("patches") for f in FC.case(n)["frames"])])
def test_the_float64_patch_stage_is_the_patch_model_on_float32(name):
    """patches_model.compute_patches (float32, the reference's control flow) on the roundings of the same planes: within 2 u of the
    float64 stage's result per application, and an overlap applies two; BLEND (:374-375) is ten roundings per application, behind
    the two alpha planes' casts"""
    k = 24 if name == "patches_alpha_blend" else 4
    for got, want, a in FC.patch_check(name):
        r = FR.M.error_ratio(got, want, a)
        print("%s: needs K = %.2f of %d" % (name, r, k))
        assert got.dtype == np.float32 and r <= k, (name, r)


# ---- the decode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.NAMES)
def test_oracle_decode_is_the_model(name, backend):
    rows = FR.frame_ratios(name, decoded(name, backend))
    c = FC.case(name)
    assert {(i, cut) for i, cut, _, _, _ in rows} >= {(len(c["frames"]) - 1, "xyb"), (len(c["frames"]) - 1, "image")}
    for i, cut, r, k, row in rows:
        print("%s frame / slot %d %s: needs K = %.3f of %s (%s)" % (name, i, cut, r, k, row))
        assert k is not None and r <= k, (name, i, cut, r, k, row)


def test_measured_rows_are_twice_the_largest_ratio(backend):
    worst = {}
    for name in FC.NAMES:
        for i, cut, r, k, row in FR.frame_ratios(name, decoded(name, backend)):
            if row in FR.MEASURED:
                worst[row] = max(worst.get(row, 0.0), r)
    for row, r in sorted(worst.items()):
        print("row %s: largest %.3f, K %d" % (row, r, FR.MEASURED[row]))
        assert FR.MEASURED[row] == math.ceil(2 * r), (row, r)
    assert set(worst) == set(FR.MEASURED)


def test_the_spline_stage_alone_is_the_model():
    """decoder.render_splines on the float32 roundings of the model's planes in front of the spline stage -- what the stage entries of
    the device are given in test_jxl_writer_features_gpu.py: K_SPLINE_STAGE is twice the largest ratio"""
    worst = 0.0
    for name in FR.STAGE_CASES:
        planes, splines, bx, bb, (x, a) = FR.spline_stage(name)
        got = [planes[c].copy() for c in range(3)]
        decoder.render_splines(got, splines, bx, bb, planes.shape[2], planes.shape[1])
        r = FR.M.error_ratio(np.stack(got), x, a)
        print("%s %r: needs K = %.3f of %d" % (name, planes.shape, r, FR.K_SPLINE_STAGE))
        worst = max(worst, r)
    assert FR.K_SPLINE_STAGE == math.ceil(2 * worst), worst
    assert [FR.spline_stage(n)[0].shape[1:] for n in FR.STAGE_CASES] == [(40, 40), (30, 38), (64, 72)]


@pytest.mark.parametrize("name", FR.PATCH_STAGE_CASES)
def test_the_patch_stage_alone_is_the_model(name):
    """patches_model.compute_patches on the float32 planes the device's patch entries are given in test_jxl_writer_features_gpu.py,
    the alpha plane already float: within the K that FR.patch_stage derives from the SOURCE"""
    import types

    import patches_model as PM
    from blend_ref import Buf
    planes, slots, pos, blend, (x, a), k = FR.patch_stage(name)
    n_extra = planes.shape[0] - 3
    info = types.SimpleNamespace(colour_space=0, num_extra=n_extra, ec_type=[0] * n_extra, ec_alpha_associated=[False] * n_extra,
                                 ec_bits=[8] * n_extra, bits_per_sample=8)
    frame = [Buf(p.copy()) for p in planes]
    ref = [None if s is None else [Buf(p.copy()) for p in s] for s in slots]
    pl = [dict(ref=p["ref"], y0=p["y0"], x0=p["x0"], h=p["height"], w=p["width"], positions=[(y, x_) for x_, y in p["positions"]],
               blend=[[(b["mode"], 0, int(b.get("clamp", False))) for b in row] for row in p["blend"]])
          for p in FC.case(name)["frames"][-1]["patches"]]
    PM.compute_patches(info, None, pl, frame, ref)
    got = np.stack([np.asarray(b.a, F) for b in frame])
    r = FR.M.error_ratio(got, x, a)
    print("%s %r: needs K = %.2f of %d" % (name, planes.shape, r, k))
    assert 1 <= k <= 48 and r <= k, (name, r, k)
    assert len(pos) == len(blend) == sum(len(p["positions"]) for p in pl)


# ---- the arc tables ------------------------------------------------------------------------------------------------------------------
K_ARC = dict(position=261, sigma=43, values=783)  # ceil(2 x the largest ratio): test_the_arc_tables_are_the_float64_models prints them


def _arc_cases():
    for name in FC.NAMES:
        for fr in FC.case(name)["frames"]:
            if fr.get("splines"):
                k = fr.get("upsampling", 1)
                h, w = (fr["planes"][0].shape if FC.is_modular(fr) else (fr["height"], fr["width"]))
                corr = fr.get("corr") or {}
                yield name, fr["splines"], F(corr.get("base_x", 0.0)), F(corr.get("base_b", 1.0)), h * k, w * k


def test_the_arc_tables_are_the_float64_models():
    """decoder.spline_arc_table and the library's jxl_spline_arcs against spline_model64.arc_table on the cases' splines: the same
    arcs in the same order, the same boxes, and positions, sigma and values within K_ARC"""
    worst = dict(position=0.0, sigma=0.0, values=0.0)
    for name, sp, bx, bb, h, w in _arc_cases():
        table, und = SM.arc_table(sp, float(bx), float(bb), h, w)
        assert not und
        table = [t for t in table if t["box"][0] <= t["box"][1] and t["box"][2] <= t["box"][3]]
        fsp = FC.frontend_splines(sp)
        py = decoder.spline_arc_table(fsp, bx, bb, w, h)
        lib = host.spline_arcs(fsp, bx, bb, h, w)
        assert len(py) == len(table) == len(lib), (name, len(py), len(lib), len(table))
        for t, (ay, ax, sigma, inv_sigma, vals, box), rec in zip(table, py, lib):
            assert tuple(box) == t["box"] == (rec["x0"], rec["x1"], rec["y0"], rec["y1"]), (name, box, t["box"])
            for got_y, got_x, got_s in ((ay, ax, sigma), (rec["y"], rec["x"], rec["sigma"])):
                worst["position"] = max(worst["position"], abs(float(got_y) - t["y"]) / (U * max(1.0, abs(t["y"]))),
                                        abs(float(got_x) - t["x"]) / (U * max(1.0, abs(t["x"]))))
                worst["sigma"] = max(worst["sigma"], abs(float(got_s) - t["sigma"]) / (U * t["sigma_a"]))
            for c in range(3):
                worst["values"] = max(worst["values"], abs(float(vals[c]) - t["values"][c]) / (U * t["values_a"][c]))
                mul = 0.25 * t["values"][c] * t["sigma"]
                worst["values"] = max(worst["values"], abs(float(rec["mul"][c]) - mul) / (U * 0.25 * t["values_a"][c] * t["sigma_a"]))
    for k, r in sorted(worst.items()):
        print("arc %s: largest %.2f, K %d" % (k, r, K_ARC[k]))
    assert K_ARC == {k: math.ceil(2 * r) for k, r in worst.items()}, worst


# ---- discrimination ------------------------------------------------------------------------------------------------------------
def test_every_writer_variant_is_listed():
    assert set(FC.VARIANT_CASES) == set(V.FEATURE_VARIANTS) and len(V.FEATURE_VARIANTS) == 8
    assert not set(V.FEATURE_VARIANTS) & set(V.VARIANTS + V.LF_VARIANTS + W.VARIANTS)


@pytest.mark.parametrize("variant", V.FEATURE_VARIANTS)
def test_a_wrong_writer_is_rejected_or_read_back_differently(variant):
    for name in FC.VARIANT_CASES[variant]:
        data = FC.encoded(name, variant)
        assert data != FC.encoded(name), (variant, name)
        why = views_differ(data, FC.case(name))
        print("%s on %s: %s" % (variant, name, why))
        assert why is not None, (variant, name)


WRONG_CASES = {
    "patches after splines": ("patches_alpha_blend",),
    "overlapping positions applied in reverse": ("patches_alpha_blend",),
    "splines after noise": ("splines_noise_40x40", "patches_splines_noise_72x64", "mod_xyb_splines_noise_40x24"),
    "splines at the frame's size under upsampling": ("splines_up2_19x15_of_37x29",),
    "every spline with its own coefficients": ("splines_40x40", "splines_264x264"),
    "the slot taken after the colour transform": ("patches_vardct_ref", "patches_modref_72x64"),
    "the slot taken before the colour transform": ("patches_ref_after_ct",),
    "a reference frame saved after its own patches": ("patches_chain_40x40",),
    "positions as (y, x)": ("patches_vardct_ref", "patches_ref_after_ct"),
    "invQa of the other branch": ("splines_quant_adjust_pos", "splines_quant_adjust_neg"),
    "MathHelper.max as a true maximum": ("splines_40x40", "splines_corr"),
    "the first spline's start as (y, x)": ("splines_40x40", "mod_rgb8_splines_33x29"),
}
_margins = {}


@pytest.mark.parametrize("what", FC.WRONG)
def test_a_wrong_expectation_leaves_the_bound(what, backend):
    """each is held against the decode at the cut after the colour transforms of the last frame, under that cut's K; the margin is
    the ratio it needs over K"""
    for name in WRONG_CASES[what]:
        m = FC.expected(name, what)
        out = decoded(name, backend)
        last = len(out["frames"]) - 1
        row = FR.final_row(FC.case(name)["frames"][last])
        r, k = FR.ratio(out["frames"][last]["xyb"], m["frames"][last]["final"]), FR.MEASURED[row]
        _margins[what, name] = r / k
        print("%s on %s: %.4g K" % (what, name, r / k))
        assert r > k, (what, name, r, k)


def test_the_smallest_margin_of_a_wrong_expectation(backend):
    for what in FC.WRONG:
        for name in WRONG_CASES[what]:
            if (what, name) not in _margins:
                test_a_wrong_expectation_leaves_the_bound(what, backend)
    (what, name), margin = min(_margins.items(), key=lambda kv: kv[1])
    print("smallest margin: %.4g K (%s on %s)" % (margin, what, name))
    assert margin > 1.0


# ---- refusals on real streams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, why", (("splines_40x40", "splines"), ("patches_of_an_empty_slot_vardct", "patches"),
                                       ("patches_splines_noise_72x64", "not a VarDCT frame"), ("patches_modref_72x64", "not a VarDCT frame")))
def test_a_region_and_a_preview_of_a_frame_with_features_are_refused(name, why, backend):
    """before backend.vardct is called. A stream whose first frame is the Modular reference frame is refused at that frame, the
    first condition of region_rule and preview_rule after the image's own: a change of that order shows here"""
    data = FC.encoded(name)
    calls = []
    backend.vardct = backend.lf_image = lambda *a, **kw: calls.append(1)
    try:
        for prefix, kw in (("region: ", dict(region=(0, 0, 16, 16))), ("downsample=8: ", dict(downsample=8))):
            with pytest.raises(UnsupportedOperationException) as e:
                JXLDecoder(data, backend=backend, **kw).decode()
            print(name, str(e.value))
            assert str(e.value) == prefix + why, (name, str(e.value))
    finally:
        del backend.vardct, backend.lf_image
    assert not calls
