"""A fifth witness, on the CPU: Modular frames that are not lossless integer RGB -- XYB frames, Gaborish, the EPF under
epf_sigma_for_modular, do_ycbcr -- written by tests/jxl_writer.py from known arrays, read by the front-end and decoded by JXLDecoder
on the oracle backend, against the expectation jxl_writer_lossy_cases.model composes from the SOURCE arrays alone.

The writer's new keys default to the bytes it wrote before (tests/golden/jxl_writer_sha256.json: every case of jxl_writer_cases.py as
the writer made it before it knew them). The mutation tables -- writers and expectations that are wrong on purpose -- show that the
comparison tells each of them from the true one, on every case listed for it, by a margin of at least 100 K where the stage is float."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import jxl_writer as W
import jxl_writer_cases as WC
import jxl_writer_lossy_cases as C
import jxl_writer_lossy_run as RUN

MARGIN = 100


@pytest.fixture(scope="module")
def backend(orc):
    from oracle.pybackend import OracleBackend
    return OracleBackend()


_decoded = {}


def decoded(name, backend):
    if name not in _decoded:
        _decoded[name] = RUN.decode(C.encoded(name), backend)
    return _decoded[name]


# ---- the writer ---------------------------------------------------------------------------------------------------------------------
def test_the_earlier_cases_encode_to_the_bytes_they_had():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jxl_writer_sha256.json")) as f:
        want = json.load(f)
    names = sorted("%s/%s" % (t, n) for t, tab in WC.TABLES.items() for n in tab)
    assert sorted(want) == names and len(want) == 206
    for t, tab in WC.TABLES.items():
        for n, im in tab.items():
            assert hashlib.sha256(W.encode(im)).hexdigest() == want["%s/%s" % (t, n)], (t, n)


# ---- the cases themselves -----------------------------------------------------------------------------------------------------------
def test_the_cases_themselves():
    """a "filter" case changes at least 20 % of its samples in the model, a "copy" case none; the sizes, sigmas and custom fields the
    cases are there for are there; no sample of any case is left out of a comparison (jxl_writer_lossy_cases.ratio takes no mask)"""
    shares = {}
    for name in C.NAMES:
        im, kind = C.image(name), C.kind(name)
        hf = C.header_fields(im)
        assert kind in ("plain", "filter", "copy", "exact"), name
        filt = hf["gab"] or hf["epf_iters"] > 0
        assert filt == (kind in ("filter", "copy")), name
        if filt:
            shares[name] = C.changed_share(name)
            assert (shares[name] >= 0.2) if kind == "filter" else (shares[name] == 0.0), (name, shares[name])
        if kind == "copy" and im["width"] * im["height"] > 1:
            assert float(np.float32(1) / np.float32(hf["epf_sigma_modular"])) > C.M.COPY_THRESHOLD, name
        elif hf["epf_iters"]:
            assert float(np.float32(1) / np.float32(hf["epf_sigma_modular"])) <= 1.0, name
        for v in [hf["epf_sigma_modular"]] + hf["lf_dequant"] + hf["gab1"] + hf["gab2"] + hf["epf_channel_scale"]:
            assert np.isfinite(v) and v > 0, name
    print("changed shares of the filter cases: %.2f .. %.2f" % (min(v for n, v in shares.items() if C.kind(n) == "filter"), max(shares.values())))
    for h, w in C.SIZES:
        combos = {(g, i) for g in (0, 1) for i in range(4) if "xyb_%dx%d_gab%d_epf%d" % (h, w, g, i) in C.CASES}
        assert combos >= {(0, 0), (1, 0), (0, 1), (0, 2), (0, 3), (1, 2)}, (h, w)
    assert "xyb_13x21_gab1_epf3" in C.CASES and "xyb_70x37_gab1_epf3" in C.CASES
    sigmas = {float(C.header_fields(C.image(n))["epf_sigma_modular"]) for n in C.NAMES if C.header_fields(C.image(n))["epf_iters"]}
    assert sigmas == {0.25, 1.0, 1.5, 2.0}
    a, b = (np.asarray(C.image("xyb_wrapping_sum")["frames"][0]["planes"][c], np.int64) for c in (0, 2))
    assert ((a + b) >= (1 << 31)).sum() >= 5 and ((a + b) < -(1 << 31)).sum() >= 5 and (np.abs(a + b) < (1 << 31)).sum() >= 5
    lfd = C.header_fields(C.image("xyb_custom_lf_dequant"))["lf_dequant"]
    assert len(set(lfd)) == 3 and not set(lfd) & {np.float32(1 / 4096.0), np.float32(1 / 512.0), np.float32(1 / 256.0)}
    hf = C.header_fields(C.image("xyb_custom_everything"))
    assert len(set(hf["gab1"])) == len(set(hf["gab2"])) == len(set(hf["epf_channel_scale"])) == 3
    assert (hf["epf_pass0_sigma"], hf["epf_pass2_sigma"], hf["epf_border_sad_mul"]) == (0.75, 5.0, 0.5)


# ---- the front-end and the oracle-backed decode -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_front_end_and_decode_against_the_source(backend, name):
    """FrameInfo equals the SOURCE's fields, the stream's channels are the SOURCE's integers, and the decode lies within the bound at
    the trace cuts mod, gab, epf and xyb and in the returned image; integer planes bit for bit"""
    out = decoded(name, backend)
    assert RUN.fields_differ(name, out) is None
    RUN.check(name, out, name)
    assert out["stats"][0]["encoding"] == "modular"


def test_measured_rows_are_twice_the_largest_ratio(backend):
    """K_MEASURED is ceil(2 x the largest oracle-vs-model ratio) over the cases of each row, and records that ratio"""
    worst = {}
    for name in C.NAMES:
        for row, r in RUN.check(name, decoded(name, backend), name).items():
            worst[row] = max(worst.get(row, 0.0), r)
        row = C.row(name, "xyb")
        if isinstance(row, str):
            worst[row] = max([worst.get(row, 0.0)] + RUN.image_ratios(name, decoded(name, backend)["planes"]))
    print({k: round(v, 3) for k, v in worst.items()})
    assert sorted(worst) == sorted(C.K_MEASURED)
    for row, (k, r) in C.K_MEASURED.items():
        assert k == math.ceil(2 * worst[row]) and abs(r - worst[row]) < 5e-4, (row, k, worst[row])


def test_no_stream_reaches_a_frame_of_another_colour_count(backend):
    """patch_sets_rule's last refusal stays without a decode: the colour count of a frame (3 for an XYB image, for a VarDCT frame and
    for do_ycbcr, else the image's: Frame.java:874-877, LFGlobal.java:88-96) differs from the image's only where the image's is 1, and
    the rule asks for a three-colour image first. The grey-tagged XYB case IS such a frame, and its three planes meet the one-colour
    canvas at plane 1 (held to the model by test_front_end_and_decode_against_the_source)"""
    from jxlatte_amd.decoder import JXLDecoder
    for colors_image, colors_frame in ((3, 3), (1, 1), (1, 3)):
        for landed in (False, True):
            assert JXLDecoder.patch_sets_rule(True, True, True, not landed, colors_image, colors_frame) != "a frame of another colour count"
    out = decoded("grey_tagged_xyb_9x11_gab1_epf2", backend)
    assert len(out["mod"]) == 3 and len(out["planes"]) == 1 and out["info"].xyb_encoded


# ---- mutations ------------------------------------------------------------------------------------------------------------------------
XYB3 = [n for n in C.NAMES if n.startswith("xyb_") and n != "xyb_wrapping_sum"]
WRITER_MUTATIONS = {
    "sigma_for_modular_before_sigma_block": [n for n in C.NAMES if C.header_fields(C.image(n))["epf_iters"] > 0],
    "quant_mul_in_a_modular_frame": ["xyb_custom_sigma_block", "xyb_custom_everything"],
    # where a filter is on: every header bit of an unfiltered full frame behind :88 is 0 up to is_last, so that one more 0 in front of
    # them can be another legal header of the same pixels (a group_size_shift of 2) when the byte padding takes it up
    "do_ycbcr_bit_in_an_xyb_image": [n for n in C.NAMES if C.image(n)["xyb"] and C.kind(n) != "plain"],
}
EXPECTATION_MUTATIONS = {
    "c_map_identity": XYB3 + ["xyb_wrapping_sum", "grey_tagged_xyb_9x11_gab1_epf2", "xyb_alpha_13x21_gab1_epf2"],
    "b_without_y": XYB3 + ["xyb_wrapping_sum", "grey_tagged_xyb_9x11_gab1_epf2"],
    "lf_dequant_c_in": XYB3 + ["xyb_wrapping_sum", "grey_tagged_xyb_9x11_gab1_epf2"],
    # where the inverse is another number: sigma 1.5, 2.0 and 0.25 (at 1 x 1 the filter is the identity under any sigma)
    "sigma_not_inverted": [n for n in C.NAMES if C.header_fields(C.image(n))["epf_iters"] > 0 and C.header_fields(C.image(n))["epf_sigma_modular"] != 1.0
                           and C.image(n)["width"] > 1],
    # where a filter runs on a frame whose size is no multiple of 8
    "padded_to_8": [n for n in C.NAMES if C.kind(n) == "filter" and (C.image(n)["width"] % 8 or C.image(n)["height"] % 8)],
    "one_colour_distance_once": [n for n in C.NAMES if n.startswith("grey8_") and C.header_fields(C.image(n))["epf_iters"] > 0],
    # 8-bit frames: at 16 bits 1 / 65536 is within 2^-16 of 1 / 65535, 128 u, which no bound of a few u can tell by a factor of 100
    "cast_by_power_of_two": [n for n in C.NAMES if n.startswith(("rgb8_", "grey8_", "ycbcr_")) and C.kind(n) != "exact"],
    "grey_plane_0": ["grey_tagged_xyb_9x11_gab1_epf2"],
    "cb_cr_exchanged": ["ycbcr_13x21", "ycbcr_13x21_gab1_epf2"],
}
_margins = {}


def test_the_mutation_tables_name_every_mutation():
    assert sorted(WRITER_MUTATIONS) == sorted(W.VARIANTS) and sorted(EXPECTATION_MUTATIONS) == sorted(C.MUTATIONS)
    assert all(len(v) >= 1 and set(v) <= set(C.NAMES) for v in list(WRITER_MUTATIONS.values()) + list(EXPECTATION_MUTATIONS.values()))


@pytest.mark.parametrize("mut", list(EXPECTATION_MUTATIONS))
def test_a_wrong_expectation_is_told_from_the_decode(backend, mut):
    """the decode is at least 100 K away from each wrong expectation, on every case listed for it"""
    worst = np.inf
    for name in EXPECTATION_MUTATIONS[mut]:
        out = decoded(name, backend)
        k = C.bound(name, "xyb")
        margin = max(RUN.image_ratios(name, out["planes"], C.model(name, mut))) / k
        worst = min(worst, margin)
        assert margin >= MARGIN, (mut, name, margin)
    _margins[mut] = worst
    print("%s: smallest margin %.0f K over %d cases" % (mut, worst, len(EXPECTATION_MUTATIONS[mut])))


@pytest.mark.parametrize("variant", list(WRITER_MUTATIONS))
def test_a_wrong_writer_is_told_from_the_decode(backend, variant):
    """a stream from a writer that is wrong on purpose does not decode to the SOURCE: the front-end or the decoder refuses it, or
    hands out a header field that is not the SOURCE's, or pixels at least 100 K away"""
    how = {}
    for name in WRITER_MUTATIONS[variant]:
        data = C.encoded(name, variant)
        assert data != C.encoded(name), (variant, name)
        try:
            out = RUN.decode(data, backend, trace=False)
        except Exception as e:  # noqa: BLE001  whatever the decoder raises for a stream that is not one
            how[name] = type(e).__name__
            continue
        diff = RUN.fields_differ(name, out)
        if diff is not None:
            how[name] = "field " + diff.split(":")[0]
            continue
        k = C.bound(name, "xyb")
        margin = max(RUN.image_ratios(name, out["planes"])) / k
        assert margin >= MARGIN, (variant, name, margin)
        how[name] = "pixels, %.0f K" % margin
    print(variant, how)
