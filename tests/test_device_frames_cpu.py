"""CPU-only, device_frames: JXLDecoder.frame_set_rule -- which frames reach the resident canvas as a plane set made from the Modular
context -- on every frame of every committed bitstream through the front-end alone, and on one synthetic header per rule; and
what jxl_canvas_from_modular_up and jxl_canvas_take_planes refuse (csrc/modplanes_check.h, csrc/canvas_check.h), through
tools/native/modplanes_up_check.cpp built under AddressSanitizer and UBSan and run as a child process."""
import glob
import os
import re
import subprocess
from types import SimpleNamespace

import pytest

from jxlatte_amd import abi, frontend
from jxlatte_amd import decoder as D
from jxlatte_amd.decoder import JXLDecoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "samples", "*.jxl")))
NAMES = [os.path.splitext(os.path.basename(p))[0] for p in SAMPLES]
R, P, S = frontend.TRANSFORM_RCT, frontend.TRANSFORM_PALETTE, frontend.TRANSFORM_SQUEEZE


def _frames(path):
    """(image header, [(copy of the frame header's fields, chain kinds)]) with the frame-level transforms deferred, as the decoder
    sees them before it chooses a route"""
    with open(path, "rb") as f:
        fe = frontend.Frontend(f.read())
    fe.set_defer_transforms(True)
    out = []
    while True:
        fr = fe.next_frame(None, None, None)
        if fr is None:
            break
        kinds = [t["kind"] for t in fe.transforms()] if fr.encoding == D.MODULAR else []
        out.append((frontend.FrameInfo.from_buffer_copy(fr), kinds))
        if fr.is_last:
            break
    return fe.image, out


def test_the_sample_list_is_the_one_the_cases_below_name():
    assert set(NAMES) == {"art", "bbb", "bench", "blendmodes_5", "lenna", "patches-lossless", "quilt", "wb-rainbow", "white"}


@pytest.mark.parametrize("name", ["blendmodes_5", "wb-rainbow"])
def test_all_ten_frames_of_the_multi_frame_samples_qualify(name):
    info, frames = _frames(SAMPLES[NAMES.index(name)])
    assert len(frames) == 5
    assert [JXLDecoder.frame_set_rule(info, fr, kinds) for fr, kinds in frames] == [None] * 5
    # the table of the samples: chains, stages and origins (what makes the three cases of _modular_frame_set)
    chains = [kinds for _, kinds in frames]
    stages = [(fr.upsampling, bool(fr.has_noise), bool(fr.has_splines)) for fr, _ in frames]
    if name == "blendmodes_5":
        assert chains == [[R]] * 5 and stages == [(1, False, False)] * 5
        assert [fr.blend_mode for fr, _ in frames] == [0, 2, 1, 4, 3]
        assert all((fr.height, fr.width, fr.y0, fr.x0) == (1024, 1024, 0, 0) for fr, _ in frames)
    else:
        assert chains == [[R], [], [], [R], []]
        assert stages == [(2, True, False), (1, False, True), (1, False, False), (1, False, False), (1, False, True)]
        assert [fr.ec_upsampling[0] for fr, _ in frames] == [2, 1, 1, 1, 1]
        assert [(fr.y0, fr.x0) for fr, _ in frames] == [(0, 0), (164, 512), (640, 512), (164, 512), (950, 1860)]
        assert all((fr.height, fr.width) == (576, 1024) for fr, _ in frames)
    assert info.num_extra == 1 and not info.xyb_encoded and info.exp_bits == 0
    # a traced decode takes the host route
    assert {JXLDecoder.frame_set_rule(info, fr, kinds, traced=True) for fr, kinds in frames} == {"a trace listener is set"}


def test_both_frames_of_patches_lossless_say_palette():
    info, frames = _frames(SAMPLES[NAMES.index("patches-lossless")])
    assert len(frames) == 2
    assert [JXLDecoder.frame_set_rule(info, fr, kinds) for fr, kinds in frames] == ["a Palette in the frame-level chain"] * 2


@pytest.mark.parametrize("name", ["bbb", "bench", "lenna", "white"])
def test_the_vardct_samples_say_not_a_modular_frame(name):
    info, frames = _frames(SAMPLES[NAMES.index(name)])
    assert frames and {JXLDecoder.frame_set_rule(info, fr, kinds) for fr, kinds in frames} == {"not a Modular frame"}


@pytest.mark.parametrize("name", ["art", "quilt"])
def test_the_single_frame_modular_samples_qualify(name):
    info, frames = _frames(SAMPLES[NAMES.index(name)])
    assert len(frames) == 1 and JXLDecoder.frame_set_rule(info, *frames[0]) is None


def _header(**kw):
    """a frame that qualifies -- RGB + alpha, 8 bits, one [RCT], blended with mode 2 away from the origin, noise and splines, saved
    after the colour transform -- with the fields of `kw` changed; (info, fr, kinds, traced)"""
    info = dict(colour_space=0, xyb_encoded=0, exp_bits=0, bits_per_sample=8, num_extra=1, ec_exp_bits=[0] * 16, ec_bits=[8] * 16)
    fr = dict(encoding=D.MODULAR, type=D.REGULAR_FRAME, lf_level=0, num_patches=0, gab=0, epf_iters=0, do_ycbcr=0, upsampling=2,
              ec_upsampling=[2] * 16, save_as_reference=1, duration=0, is_last=0, save_before_ct=0, num_modular_channels=4,
              has_noise=1, has_splines=1, x0=-7, y0=300, blend_mode=2, ec_blend_mode=[3] * 16, blend_source=2, width=50, height=40)
    kinds, traced = kw.pop("kinds", [R]), kw.pop("traced", False)
    for k, v in kw.items():
        assert k in info or k in fr, k
        (info if k in info else fr)[k] = v
    return SimpleNamespace(**info), SimpleNamespace(**fr), kinds, traced


RULES = {
    "not_modular": (dict(encoding=D.VARDCT), "not a Modular frame"),
    "palette": (dict(kinds=[P]), "a Palette in the frame-level chain"),
    "palette_after_rct": (dict(kinds=[R, P]), "a Palette in the frame-level chain"),
    "squeeze_before_rct": (dict(kinds=[S, R]), "a frame-level chain that is not one plan ([], [RCT], [Squeeze] or [RCT, Squeeze])"),
    "two_rcts": (dict(kinds=[R, R]), "a frame-level chain that is not one plan ([], [RCT], [Squeeze] or [RCT, Squeeze])"),
    "reference_only": (dict(type=D.REFERENCE_ONLY), "not a regular or skip-progressive frame of LF level 0"),
    "lf_frame": (dict(type=D.LF_FRAME), "not a regular or skip-progressive frame of LF level 0"),
    "lf_level_1": (dict(lf_level=1), "not a regular or skip-progressive frame of LF level 0"),
    "patches": (dict(num_patches=1), "patches"),
    "gaborish": (dict(gab=1), "a restoration filter or YCbCr"),
    "epf": (dict(epf_iters=2), "a restoration filter or YCbCr"),
    "ycbcr": (dict(do_ycbcr=1), "a restoration filter or YCbCr"),
    "xyb": (dict(xyb_encoded=1), "an XYB image"),
    "float_colours": (dict(exp_bits=8), "colour planes that are not three int32 planes"),
    "one_colour": (dict(colour_space=D.CE_GRAY, num_modular_channels=2), "colour planes that are not three int32 planes"),
    "seventeen_planes": (dict(num_extra=14, num_modular_channels=17), "more planes than a set holds"),
    "saved_before_ct": (dict(save_before_ct=1), "saved before the colour transform"),
    "ec_upsampling_differs": (dict(ec_upsampling=[4] + [2] * 15), "an extra channel whose upsampling is not the colours'"),
    "ec_upsampled_alone": (dict(upsampling=1), "an extra channel whose upsampling is not the colours'"),
    "traced": (dict(traced=True), "a trace listener is set"),
}


@pytest.mark.parametrize("case", sorted(RULES))
def test_one_synthetic_header_per_rule(case):
    kw, why = RULES[case]
    assert JXLDecoder.frame_set_rule(*_header(**kw)) == why


FREE = {
    "as_it_is": {}, "no_chain": dict(kinds=[]), "squeeze": dict(kinds=[S]), "rct_squeeze": dict(kinds=[R, S]),
    "skip_progressive": dict(type=D.SKIP_PROGRESSIVE), "last_frame": dict(is_last=1), "at_the_origin": dict(x0=0, y0=0),
    "every_blend_mode": dict(blend_mode=4, ec_blend_mode=[0] * 16), "slot_0": dict(blend_source=0, save_as_reference=0),
    "no_noise_no_splines": dict(has_noise=0, has_splines=0), "not_upsampled": dict(upsampling=1, ec_upsampling=[1] * 16),
    "upsampled_8": dict(upsampling=8, ec_upsampling=[8] * 16), "no_extra_channels": dict(num_extra=0, num_modular_channels=3),
    "sixteen_planes": dict(num_extra=13, num_modular_channels=16), "float_extra_channel": dict(ec_exp_bits=[8] * 16),
    "save_before_ct_on_a_frame_that_is_not_saved": dict(save_before_ct=1, is_last=1),
    "extra_channels_past_num_extra_are_not_looked_at": dict(ec_upsampling=[2, 4] + [1] * 14),
}


@pytest.mark.parametrize("case", sorted(FREE))
def test_what_the_rule_leaves_free(case):
    assert JXLDecoder.frame_set_rule(*_header(**FREE[case])) is None


def test_the_command_line_switch():
    from jxlatte_amd import __main__ as cli
    ap = cli.parser()
    assert ap.parse_args(["in.jxl", "out.png"]).device_frames is False
    assert ap.parse_args(["in.jxl", "out.png", "--device-canvas", "--device-frames"]).device_frames is True


# ---- the refusals of the two entries, through the sanitized stand-alone program --------------------------------------------
INV, UNS, STATE = abi.JXL_ERR_INVALID_ARGUMENT, abi.JXL_ERR_UNSUPPORTED, abi.JXL_ERR_STATE
# every refusal the two entries document (include/jxlatte_amd.h), with its status
REFUSALS = {
    "up_null_desc": INV, "up_no_plan_has_run": STATE, "up_no_plan_has_run_bad_k": STATE, "up_n_planes_0": INV, "up_n_planes_17": UNS,
    "up_height_0": INV, "up_width_negative": INV, "up_channel_negative": INV, "up_channel_past_the_list": INV,
    "up_empty_result_list": INV, "up_channel_lower_than_bounds": INV, "up_channel_narrower_than_bounds": INV,
    "up_add_channel_past_the_list": INV, "up_add_channel_other_size": INV, "up_type_2": INV,
    "up_k_0": INV, "up_k_1": INV, "up_k_3": INV, "up_k_16": INV, "up_k_negative": INV, "up_k_int_min": INV,
    "up_null_weights": INV, "up_int32_plane": INV, "up_last_plane_int32": INV,
    "up_height_beyond_a_set": INV, "up_width_beyond_a_set": INV,
    "take_unknown_set": INV, "take_unknown_set_without_planes": INV, "take_one_plane": INV, "take_two_planes": INV,
    "take_no_resident_planes": STATE, "take_planes_higher": INV, "take_planes_narrower": INV, "take_planes_transposed": INV,
}
ACCEPTED = {"up_three_float_planes_k2", "up_k4", "up_k8", "up_one_plane", "up_sixteen_planes", "up_bounds_1x1",
            "up_channel_larger_than_bounds", "up_plane_adds_a_channel", "up_largest_size_a_set_holds",
            "up_planes_past_n_planes_are_not_looked_at", "take_set_of_four", "take_set_of_three", "take_set_of_sixteen_int32"}


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("modplanes_up_check") / "modplanes_up_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "modplanes_up_check.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_the_program_runs_clean_under_asan_and_ubsan(check_run):
    r = check_run
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "%d case(s), 0 failure(s)" % (len(REFUSALS) + len(ACCEPTED)) in r.stdout and "FAIL" not in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_every_refusal_has_its_status(check_run):
    got = {m[0]: int(m[1]) for m in re.findall(r"^REFUSAL (\w+) (-?\d+)$", check_run.stdout, re.M)}
    assert got == REFUSALS


def test_the_edge_cases_are_accepted(check_run):
    got = {m[0]: int(m[1]) for m in re.findall(r"^ACCEPT (\w+) (-?\d+)$", check_run.stdout, re.M)}
    assert got == {name: 0 for name in ACCEPTED}
