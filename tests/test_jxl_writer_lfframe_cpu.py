"""LF frames, USE_LF_FRAME and a permuted TOC pinned to known pixels, on the CPU: every case of jxl_writer_lfframe_cases.py is a
stream of several frames written by jxl_writer_vardct.encode_stream, read by the front-end -- whose every integer must be the SOURCE's,
frame by frame -- and decoded on the oracle backend. Every cut of every frame, the planes an LF frame leaves in lfBuffer and the image
must be the float64 models' of the SOURCE within K u (A + |model|). Then the discrimination: six writers that are wrong about an LF
frame's header, a consumer's header and LF groups, or the permutation; eight expectations made the wrong way. A consumer whose LF groups
reach beyond the stored planes is refused before the backend sees it."""
import math

import numpy as np
import pytest

import jxl_writer as W
import jxl_writer_lfframe_cases as L
import jxl_writer_lfframe_run as LR
import jxl_writer_vardct as V
import jxl_writer_vardct_cases as VC
import vardct_ref64 as M
from jxlatte_amd import frontend
from jxlatte_amd.decoder import InvalidBitstreamException, JXLDecoder
from test_jxl_writer_vardct_cpu import sparse_to_dense


@pytest.fixture(scope="module")
def backend(orc):
    from oracle.pybackend import OracleBackend
    return OracleBackend()


_decoded = {}


def decoded(name, backend):
    if name not in _decoded:
        _decoded[name] = LR.decode(L.encoded(name), backend)
    return _decoded[name]


# ---- the front-end's views -------------------------------------------------------------------------------------------------------
def header_of(image, fr):
    """the fields of FrameInfo the cases exercise, as the reference derives them from what the writer was given"""
    level = fr.get("lf_level", 0)
    if L.is_modular(fr):
        h, w = fr["planes"][0].shape
        rf = fr.get("restoration", {})
        return dict(type=fr.get("type", 0), encoding=1, flags=0, lf_level=level, width=w, height=h, padded_width=w, padded_height=h,
                    upsampling=1, is_last=int(not level), num_groups=1, num_lf_groups=1, do_ycbcr=int(fr.get("ycbcr", False)),
                    gab=int(rf.get("gab", False)), epf_iters=rf.get("epf_iters", 0))
    geo = V.geometry(fr)
    # FrameHeader.java:178: an LF frame is never the last; :118: upsampling is 1 in a frame that uses an LF frame
    return dict(type=W.LF_FRAME if level else W.REGULAR, encoding=0, flags=V.frame_flags(fr), lf_level=level, width=fr["width"],
                height=fr["height"], padded_width=geo["pw"], padded_height=geo["ph"], upsampling=1, is_last=int(not level),
                num_groups=geo["num_groups"], num_lf_groups=geo["num_lf_groups"], has_noise=int(fr.get("noise") is not None),
                do_ycbcr=int(fr.get("do_ycbcr", False)), gab=int(fr.get("gab", True)), epf_iters=fr.get("epf_iters", 0),
                global_scale=fr["global_scale"], quant_lf=fr["quant_lf"], num_passes=V.num_passes(fr))


def frame_differs(fe, info, image, src):
    """None when every integer the front-end hands out of the current frame is the SOURCE's; else what differs first"""
    for k, v in header_of(image, src).items():
        if getattr(info, k) != v:
            return "FrameInfo.%s: %r for %r" % (k, getattr(info, k), v)
    if L.is_modular(src):
        for i, p in enumerate(src["planes"]):  # the stream's channels in stream order
            got = np.asarray(fe.modular_channel(i)[0])[:p.shape[0], :p.shape[1]]
            if got.shape != p.shape or not np.array_equal(got, p):
                return "Modular channel %d" % i
        return None
    geo = V.geometry(src)
    for i, g in enumerate(src["lfgroups"]):
        v = fe.lfgroup(i)
        blocks = sorted(g["blocks"])
        sel = np.zeros(np.asarray(g["hf_mul"]).shape, np.int64)
        for y, x, t in blocks:
            sel[y:y + V.cells(t)[0], x:x + V.cells(t)[1]] = t
        pairs = [("dct_select", sel), ("hf_mul", g["hf_mul"]), ("sharpness", g["sharpness"]), ("x_from_y", g["x_from_y"]),
                 ("b_from_y", g["b_from_y"]), ("block_yx", np.array([(y, x) for y, x, _ in blocks]))]
        for k, a in pairs:
            if v[k].shape != np.asarray(a).shape or not np.array_equal(v[k], a):
                return "LF group %d %s" % (i, k)
        if src.get("use_lf_frame", False):  # LFCoefficients.java:44-57: no LF stream, no extra_precision
            if v["lf_quant"] is not None or v["extra_precision"] != 0:
                return "LF group %d holds LF coefficients of its own" % i
        else:
            for c in range(3):
                if not np.array_equal(v["lf_quant"][c], g["lf_quant"][c]):
                    return "LF group %d lf_quant %d" % (i, c)
            if v["extra_precision"] != g.get("extra_precision", 0):
                return "LF group %d extra_precision" % i
        if v["n_blocks"] != len(blocks):
            return "LF group %d n_blocks" % i
    shifts = list(src.get("pass_shifts", [])) + [0]
    for k, s in enumerate(shifts):
        for grp in range(geo["num_groups"]):
            gy, gx = grp // geo["cols"], grp % geo["cols"]
            dense, sparse = fe.coeffs(k, grp), fe.coeffs_sparse(k, grp)
            for c in range(3):
                a = np.asarray(src["coeff_passes"][k][c], np.int64) << s
                a = a[gy * 256:(gy + 1) * 256, gx * 256:(gx + 1) * 256]
                if dense[c].shape != a.shape or not np.array_equal(dense[c], a):
                    return "coefficients pass %d group %d channel %d" % (k, grp, c)
                sd, n = sparse_to_dense(sparse[c][0], sparse[c][1], sparse[c][2])
                if sparse[c][2] != a.shape or not np.array_equal(sd, a) or n != int((a != 0).sum()):
                    return "sparse coefficients pass %d group %d channel %d" % (k, grp, c)
    return None


def views_differ(data, case):
    try:
        fe = frontend.Frontend(data)
        if (fe.image.height, fe.image.width, bool(fe.image.xyb_encoded)) != (case["image"]["height"], case["image"]["width"], case["image"]["xyb"]):
            return "ImageInfo"
        for i, src in enumerate(case["frames"]):
            info = fe.next_frame()
            if info is None:
                return "the stream ends before frame %d" % i
            why = frame_differs(fe, info, case["image"], src)
            if why is not None:
                return "frame %d: %s" % (i, why)
        if fe.next_frame() is not None:
            return "a frame too many"
    except frontend.FrontendError as e:
        return "rejected: %s" % e
    return None


@pytest.mark.parametrize("name", L.NAMES)
def test_front_end_hands_out_the_source_of_every_frame(name):
    assert views_differ(L.encoded(name), L.case(name)) is None


def test_the_headers_of_the_cases():
    """flags, lf_level and sizes as the issue names them, on the SOURCE and through the front-end (header_of is held by the test above)"""
    def headers(name):
        fe = frontend.Frontend(L.encoded(name))
        out = []
        while True:
            fr = fe.next_frame()
            if fr is None:
                return out
            out.append((fr.type, fr.lf_level, fr.flags & V.FLAG_USE_LF_FRAME, fr.width, fr.height, fr.padded_width, fr.padded_height, fr.is_last))
    assert headers("lf1_vardct") == [(1, 1, 0, 9, 5, 16, 8, 0), (0, 0, 32, 72, 40, 72, 40, 1)]
    assert headers("lf1_modular_xyb") == [(1, 1, 0, 9, 5, 9, 5, 0), (0, 0, 32, 72, 40, 72, 40, 1)]
    assert headers("lf2_chain") == [(1, 2, 0, 3, 2, 8, 8, 0), (1, 1, 32, 17, 9, 24, 16, 0), (0, 0, 32, 136, 72, 136, 72, 1)]
    assert headers("lf1_two_lfgroups") == [(1, 1, 0, 257, 2, 264, 8, 0), (0, 0, 32, 2056, 16, 2056, 16, 1)]
    fe = frontend.Frontend(L.encoded("lf1_two_lfgroups"))
    fe.next_frame(), fe.next_frame()
    assert [(fe.lfgroup(i)["cells_h"], fe.lfgroup(i)["cells_w"]) for i in range(2)] == [(2, 256), (2, 1)]
    fe = frontend.Frontend(L.encoded("lf1_noise_up"))
    fe.next_frame()
    fr = fe.next_frame()
    assert fr.upsampling == 1 and fr.has_noise == 1 and fr.flags == V.FLAG_NOISE | V.FLAG_USE_LF_FRAME  # FrameHeader.java:113-119


def test_cases_are_what_they_claim():
    c = L.case("lf1_vardct")
    lf, co = c["frames"]
    assert lf["gab"] and lf["epf_iters"] == 1 and V.padded_size(lf) == (8, 16)
    assert {t for _, _, t in co["lfgroups"][0]["blocks"]} == set(L.MIXED)
    thr = co["block_ctx"]["lf_thresholds"]
    assert all(len(t) > 0 for t in thr)
    g = co["lfgroups"][0]
    # the thresholds would give most cells an LF index other than 0, and the cluster map tells every such index from 0
    wrong = [V.lf_index(co, g, y, x, "lf_index_from_thresholds_in_a_use_lf_frame_group") for y, x, _ in g["blocks"]]
    assert all(V.lf_index(co, g, y, x) == 0 for y, x, _ in g["blocks"]) and np.mean(np.array(wrong) != 0) > 0.5
    cm = np.array(co["block_ctx"]["cluster_map"]).reshape(-1, 12)
    assert (cm[:, 1:] != cm[:, :1]).all()
    # the filters of the LF frame filter: the stored planes are neither the planes before them nor their inverse XYB
    m = L.models("lf1_vardct")[0]
    (e, ea), (i, _) = m["epf"], m["idct"]
    assert (np.abs(e - i) > 1000 * M.U * (ea + np.abs(e))).mean() > 0.25
    ch = L.case("lf2_chain")["frames"]
    assert [f.get("lf_level", 0) for f in ch] == [2, 1, 0] and [f.get("use_lf_frame", False) for f in ch] == [False, True, True]
    two = L.case("lf1_two_lfgroups")["frames"][1]
    assert V.geometry(two)["num_lf_groups"] == 2 and np.asarray(two["lfgroups"][1]["hf_mul"]).shape == (2, 1)
    iy = L.case("lf1_int_ycbcr")
    assert not iy["image"]["xyb"] and iy["frames"][1]["do_ycbcr"] and all(p.dtype.kind == "i" for p in iy["frames"][0]["planes"])
    t = L.models("lf1_noise_up")[1]["tail"]
    print("lf1_noise_up", t)
    assert t["below"] > 0 and t["above"] > 0 and len(t["segments"]) >= 5
    p = L.case("toc_perm_groups")["frames"][0]
    n = 1 + 1 + 1 + 4 * 2  # Frame.java:150
    assert V.geometry(p)["num_groups"] == 4 and V.num_passes(p) == 2 and sorted(p["permutation"]) == list(range(n))
    code, end = V.lehmer(p["permutation"], 0)
    inverse = [p["permutation"].index(i) for i in range(n)]
    assert end == 7 < n and inverse != p["permutation"]
    assert L.case("toc_perm_1group")["frames"][0]["permutation"] == [0]
    pl = L.case("toc_perm_lf")["frames"]
    assert pl[0]["permutation"] == [0] and sorted(pl[1]["permutation"]) == list(range(5)) and pl[1]["permutation"] != list(range(5))
    # every section of a permuted frame has a length of its own: lengths in the wrong order are wrong lengths
    for name in ("toc_perm_groups", "toc_perm_lf"):
        assert L.encoded(name) != L.unpermuted(name) and len(L.encoded(name)) > len(L.unpermuted(name))


# ---- the pixel cuts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.NAMES)
def test_oracle_decode_is_the_model_at_every_cut_of_every_frame(name, backend):
    out = decoded(name, backend)
    rows = LR.frame_ratios(name, out)
    frames = L.case(name)["frames"]
    assert {(i, cut) for i, cut, _, _, _ in rows} >= {(i, "stored") for i, f in enumerate(frames) if f.get("lf_level", 0)} | {(len(frames) - 1, "image")}
    for i, cut, r, k, row in rows:
        print("%s frame %d %s: needs K = %.3f of %s (%s)" % (name, i, cut, r, k, row))
        assert r <= (k or 0), (name, i, cut, r, k)
    for slot, planes in enumerate(out["lfBuffer"]):  # the stored planes have the LF frame's padded size
        src = [f for f in frames if f.get("lf_level", 0) == slot + 1]
        assert (planes is None) == (not src)
        if src:
            want = src[-1]["planes"][0].shape if L.is_modular(src[-1]) else V.padded_size(src[-1])
            assert all(p.shape == want for p in planes), (name, slot)


def test_measured_rows_are_twice_the_largest_ratio(backend):
    worst = {}
    for name in L.NAMES:
        for i, cut, r, k, row in LR.frame_ratios(name, decoded(name, backend)):
            if isinstance(row, tuple):
                worst[row] = max(worst.get(row, 0.0), r)
    for key, r in sorted(worst.items()):
        print("row %s: largest %.3f, K %d" % (key, r, LR.MEASURED[key]))
        assert LR.MEASURED[key] == math.ceil(2 * r), (key, r)
    assert set(worst) == set(LR.MEASURED)


def test_the_noise_seed_does_not_count_the_lf_frame(backend):
    """JXLCodestreamDecoder.java:618-629: an LF frame leaves the loop before the frame counters; the consumer is the first visible frame"""
    dec = JXLDecoder(L.encoded("lf1_noise_up"), backend=backend)
    dec.decode()
    assert (dec.visibleFrames, dec.invisibleFrames) == (1, 0)


# ---- discrimination ------------------------------------------------------------------------------------------------------------
def test_every_writer_variant_is_listed():
    assert set(L.VARIANT_CASES) == set(V.LF_VARIANTS) and len(V.LF_VARIANTS) == 6


@pytest.mark.parametrize("variant", V.LF_VARIANTS)
def test_a_wrong_writer_is_rejected_or_read_back_differently(variant):
    for name in L.VARIANT_CASES[variant]:
        data = L.encoded(name, variant)
        assert data != L.encoded(name), (variant, name)
        why = views_differ(data, L.case(name))
        print("%s on %s: %s" % (variant, name, why))
        assert why is not None, (variant, name)


LARGE = 100  # "a large multiple of K"
# expectation made the wrong way -> [(case, frame, cut)] it is held against
WRONG_AT = {
    "inverse XYB applied to the stored planes": [("lf1_vardct", 0, "stored"), ("lf2_chain", 1, "stored")],
    "planes stored before Gaborish and the EPF": [("lf1_vardct", 0, "stored"), ("lf1_modular_xyb", 0, "stored")],
    "smoothing applied to the copied LF": [("lf1_vardct", 1, "idct")],
    "chroma from luma applied to the copied LF": [("lf1_vardct", 1, "idct"), ("lf1_modular_xyb", 1, "idct"), ("lf2_chain", 1, "idct")],
    "window origin lfg_x << 11": [("lf1_two_lfgroups", 1, "idct")],
    "the consumer's LF read from the level-2 planes": [("lf2_chain", 2, "idct")],
    "integer planes cast by 1 / 256": [("lf1_int_ycbcr", 1, "idct")],
    "noise seeded as if the LF frame had been a visible frame": [("lf1_noise_up", 1, "xyb")],
}


def test_every_wrong_expectation_is_listed():
    assert sorted(WRONG_AT) == sorted(L.WRONG)


@pytest.mark.parametrize("what", sorted(WRONG_AT))
def test_a_wrong_expectation_leaves_the_bound(what, backend):
    for name, i, cut in WRONG_AT[what]:
        out = decoded(name, backend)
        m = L.models(name, what)[i]
        if cut == "stored":
            got = np.stack(out["lfBuffer"][L.case(name)["frames"][i]["lf_level"] - 1])
        else:
            got = out["frames"][i][cut]
        r, k = LR.ratio(got, m["final" if cut == "xyb" else cut]), LR.bound(name, i, cut)
        print("%s on %s frame %d %s: %.4g K" % (what, name, i, cut, r / k))
        assert r > LARGE * k, (what, name, r, k)


def test_a_consumer_without_an_lf_frame_is_refused(backend):
    """JXLCodestreamDecoder.java:613-614"""
    c = L.case("lf1_vardct")
    data = V.encode_stream(c["image"], c["frames"][1:])
    calls = []
    backend.vardct = lambda *a, **kw: calls.append(1)
    try:
        with pytest.raises(InvalidBitstreamException, match="LF Level too large"):
            JXLDecoder(data, backend=backend).decode()
    finally:
        del backend.vardct
    assert not calls


def test_a_consumer_larger_than_the_stored_planes_is_refused(backend):
    """a consumer whose crop is larger than the image: 17 x 9 cells of stored planes of 16 x 8. The reference's arraycopy throws
    (LFCoefficients.java:53); numpy would hand out short planes, which travel to the device as bare pointers"""
    c = L.case("lf1_vardct")
    big = VC.draw(8190, 136, 72, use_lf_frame=True, crop=(0, 0), image_width=72, image_height=40)
    data = V.encode_stream(c["image"], [c["frames"][0], big])
    fe = frontend.Frontend(data)
    fe.next_frame()
    fr = fe.next_frame()
    assert (fr.width, fr.height, fr.flags & V.FLAG_USE_LF_FRAME) == (136, 72, 32)  # the front-end reads it: the header is legal
    calls = []
    orig = backend.vardct

    def vardct(params, *a, **kw):
        calls.append((params.width, params.height))
        return orig(params, *a, **kw)
    backend.vardct = vardct
    try:
        with pytest.raises(InvalidBitstreamException, match="LF frame too small"):
            JXLDecoder(data, backend=backend).decode()
    finally:
        del backend.vardct
    assert calls == [(16, 8)]  # the LF frame's call; the consumer's was never made


def test_a_preview_and_a_region_of_a_stream_with_an_lf_frame_are_refused(backend):
    """preview_rule and region_rule on the first frame's header, an LF frame: no backend call is made"""
    from jxlatte_amd.decoder import UnsupportedOperationException
    calls = []
    backend.vardct = backend.lf_image = lambda *a, **kw: calls.append(1)  # (the oracle backend has no lf_image: the switch asks for one)
    try:
        for switches, word in ((dict(downsample=8), "downsample=8"), (dict(region=(0, 0, 16, 16)), "region")):
            with pytest.raises(UnsupportedOperationException) as e:
                JXLDecoder(L.encoded("lf1_vardct"), backend=backend, **switches).decode()
            assert str(e.value) == word + ": not a regular frame of LF level 0 with LF coefficients of its own"
    finally:
        del backend.vardct, backend.lf_image
    assert not calls


# ---- the permuted TOC --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.PERM_CASES)
def test_a_permuted_stream_decodes_to_its_unpermuted_twin(name, backend):
    twin = JXLDecoder(L.unpermuted(name), backend=backend).decode().getBuffer()
    got = decoded(name, backend)["image"].getBuffer()
    assert len(got) == len(twin) == 3
    for a, b in zip(got, twin):
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


REGIONS = ((0, 0, 40, 40), (250, 250, 14, 14), (100, 200, 100, 64), (256, 0, 8, 264))


@pytest.mark.parametrize("box", REGIONS)
def test_a_region_of_a_permuted_frame_is_the_crop_of_the_full_decode(box, backend):
    """the group sections are looked up through the permutation: the region reads the groups its unpermuted twin reads"""
    x0, y0, w, h = box
    full = decoded("toc_perm_groups", backend)["image"].getBuffer()
    dec = JXLDecoder(L.encoded("toc_perm_groups"), backend=backend, region=box)
    twin = JXLDecoder(L.unpermuted("toc_perm_groups"), backend=backend, region=box)
    got, want = dec.decode().getBuffer(), twin.decode().getBuffer()
    for c in range(3):
        assert np.array_equal(got[c].view(np.uint32), full[c][y0:y0 + h, x0:x0 + w].view(np.uint32)), (box, c)
        assert np.array_equal(got[c].view(np.uint32), want[c].view(np.uint32)), (box, c)
    a, b = dec.stats[-1]["region"], twin.stats[-1]["region"]
    assert a["path"] == "groups" and (a["groups_read"], a["lf_groups_read"]) == (b["groups_read"], b["lf_groups_read"])
    assert a["section_bytes_read"] == b["section_bytes_read"] and a["subframe"] == b["subframe"]
    print(box, a)
    if box == REGIONS[0]:
        assert a["groups_read"] == 1 and a["groups_total"] == 4 and a["section_bytes_read"] < a["section_bytes_total"]
