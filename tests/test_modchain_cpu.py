"""jxl_modular_begin_chain without a GPU: the model of tests/modchain_ref.py against the front-end's own loop on a real file whose
frames undo four nested palettes; the mutation table; the walk, the refusals and the fused run's path table of
jxlatte_amd/csrc/modchain_check.h as a stand-alone host program under AddressSanitizer + UBSan (tools/native/modchain_check.cpp;
the sanitizer runtimes are linked statically, so the program needs nothing from its environment), bit for bit against the model
on every case of tests/modchain_cases.py; the declarations and the bindings."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import modchain_cases as cases
import modchain_ref as ref
from jxlatte_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")


# ---- the model against the front-end's own loop on a real file ----
def test_model_equals_the_frontends_loop_on_both_frames_of_patches_lossless():
    """decoded with the transforms deferred, each frame hands out its encoded channel list and its chain: the model's walk over
    them gives the channels jxf_apply_transforms leaves without any hook"""
    from jxlatte_amd import frontend
    fe = frontend.Frontend(open(os.path.join(SAMPLES, "patches-lossless.jxl"), "rb").read())
    try:
        fe.set_defer_transforms(True)
        shapes = []
        while True:
            fr = fe.next_frame(None, None)
            if fr is None:
                break
            transforms = fe.transforms()
            assert [t["kind"] for t in transforms] == [ref.PALETTE] * 4 and [t["num_c"] for t in transforms] == [1, 1, 1, 4]
            encoded = [fe.modular_channel(i)[0].copy() for i in range(fe.modular_channel_count())]
            assert len(encoded) == 5 and encoded[0].shape[0] == 4
            want = ref.apply_chain(encoded, transforms, fe.image.bits_per_sample)
            fe.apply_transforms(None, None, None)
            got = [fe.modular_channel(i)[0] for i in range(fe.modular_channel_count())]
            assert ref.same(got, want), "frame %d" % len(shapes)
            shapes.append(got[0].shape)
        assert shapes == [(198, 198), (1096, 1600)]
    finally:
        fe.close()


# ---- the mutation table ----
@pytest.mark.parametrize("mut", ref.MUTATIONS)
def test_every_wrong_walk_differs_from_the_model_on_some_case(mut):
    differing = []
    for name, c in cases.CASES.items():
        if name == "front_257x769" and mut not in ("deltas_ignored",):
            continue  # (the one large case: only its own mutation is worth the model's time)
        if name == "front_257x769":
            small = cases.palette_cases.CASES["shape_2x5_5_pred13"]  # the same mutation on a shape the model walks at once
            c = dict(chans=[small["palette"], small["index"]], bit_depth=small["bit_depth"],
                     transforms=[cases.pal(0, small["num_c"], small["nb_colors"], small["nb_deltas"], small["d_pred"])])
            want = ref.apply_chain(c["chans"], c["transforms"], c["bit_depth"])
        else:
            want = cases.expected(name)
        try:
            got = ref.apply_chain(c["chans"], c["transforms"], c["bit_depth"], mut=mut)
        except (AssertionError, IndexError, ValueError):
            differing.append(name)  # the wrong walk leaves the list or a palette
            continue
        if not ref.same(got, want):
            differing.append(name)
    assert differing, mut
    # and each mutation is caught where it should be
    must = {"bitstream_order": "sample_shape_5x7", "channel0_kept": "depth2_5x7", "palette_of_wrong_stage": "depth2_33x70",
            "begin_c_of_final_list": "sample_shape_33x70", "deltas_ignored": "planted_negative_pred5", "negative_not_delta": "planted_negative_pred5"}
    assert must[mut] in differing, (mut, differing)


def test_cases_cover_what_they_promise():
    cs = cases.CASES
    assert {c["chans"][-1].shape for n, c in cs.items() if n.startswith(("depth", "sample_shape"))} >= set(cases.SIZES)
    assert {len(c["transforms"]) for n, c in cs.items() if n.startswith("depth")} >= {1, 2, 3, 5}
    kinds = {tuple(t["kind"] for t in c["transforms"]) for c in cs.values()}
    P, R, S = ref.PALETTE, ref.RCT, ref.SQUEEZE
    assert kinds >= {(P, R), (R, P), (P, S), (S, P), (R, R), (R, S), (P, P, P, P), (P,), (P, P), (P, P, P)}
    assert any(t["num_c"] == 18 for t in cs["num_c_18"]["transforms"])
    # the budget cases sit on the constant of the header, which is more than the lookup kernel's own
    header = open(os.path.join(ROOT, "jxlatte_amd", "csrc", "modchain_check.h")).read()
    assert int(re.search(r"constexpr int kPaletteRunLdsInts = (\d+);", header).group(1)) == cases.RUN_LDS_INTS > cases.palette_cases.LDS_INTS
    for k, v in (("kPalRunMaxStages", cases.RUN_MAX_STAGES), ("kPalRunMaxDepth", cases.RUN_MAX_DEPTH), ("kPalRunMaxOut", cases.RUN_MAX_OUT)):
        assert int(re.search(r"constexpr int %s = (\d+);" % k, header).group(1)) == v
    entries = lambda c: sum(t["num_c"] * t["nb_colors"] for t in c["transforms"])
    assert entries(cs["lds_budget_exact"]) == cases.RUN_LDS_INTS == entries(cs["lds_budget_over"]) - 1
    big = cs["palette_in_global_memory"]["transforms"][0]
    assert cases.palette_cases.LDS_INTS < big["num_c"] * big["nb_colors"] <= cases.RUN_LDS_INTS
    # intermediate indices of every class reach a second stage: negative, past nb_colors in both implicit ranges, the int32 ends
    c = cs["depth3_33x70"]
    mid = ref.apply_chain(c["chans"][:1] + c["chans"][-1:], [cases.pal(0, 1, c["transforms"][2]["nb_colors"])], c["bit_depth"])[0].astype(np.int64)
    nc = c["transforms"][1]["nb_colors"]
    assert (mid < 0).any() and (mid == cases.I32_MIN).any() and (mid == cases.I32_MAX).any()
    assert ((mid >= nc) & (mid < nc + 64)).any() and (mid >= nc + 64).any() and ((mid >= 0) & (mid < nc)).any()
    # the planted cases: the pixels that name the one negative entry need a neighbour under predictor 5, none does under predictor 0
    assert cases.chained("planted_negative_pred5") == [False, True] and cases.chained("planted_negative_pred0") == [False, False]
    p5 = cs["planted_negative_pred5"]
    first = ref.apply_chain(p5["chans"][:1] + p5["chans"][-1:], [cases.pal(0, 1, p5["transforms"][1]["nb_colors"])], 8)[0]
    assert int((first < 0).sum()) == int((first == -2).sum()) > 0 and first[0, 0] == -2
    assert cases.chained("front_257x769") == [True]
    assert all(not any(cases.chained(n)) for n in cs if n not in ("planted_negative_pred5", "front_257x769"))
    assert cases.stats("planted_negative_pred5", True) == (1, 3, 1) and cases.stats("planted_negative_pred5", False) == (0, 5, 1)
    assert cases.stats("planted_negative_pred0", True) == (1, 0, 0) and cases.stats("sample_shape_33x70", False) == (0, 4, 0)
    assert cases.stats("lds_budget_over", True) == (0, 2, 0) and cases.stats("lds_budget_exact", True) == (1, 0, 0)
    # the channel of another size next to the runs stays as it is
    assert np.array_equal(cases.expected("palette_of_a_palette")[-1], cs["palette_of_a_palette"]["chans"][-1])


# ---- modchain_check.h as a program of its own, under the sanitizers ----
REFUSALS = {"null_channels": -1, "null_transforms": -1, "negative_n_chans": -1, "negative_n_tr": -1, "negative_channel_size": -1,
            "channel_without_data": -1, "channel_too_many_samples": -1, "unknown_kind": -1, "negative_kind": -1,
            "palette_num_c_0": -1, "palette_num_c_negative": -1, "palette_num_c_max": -1, "palette_pal_h_below_num_c": -1,
            "palette_pal_w_below_nb_colors": -1, "palette_nb_colors_negative": -1, "palette_nb_deltas_negative": -1,
            "palette_d_pred_negative": -1, "palette_d_pred_14": -1, "palette_bit_depth_0": -1, "palette_bit_depth_33": -1,
            "palette_index_without_samples": -1, "palette_weighted_deltas": -3, "palette_begin_c_negative": -1,
            "palette_index_past_the_list": -1, "palette_begin_c_max": -1, "palette_on_an_empty_list": -1, "palette_sizes_at_that_point": -1,
            "rct_past_the_list": -1, "rct_begin_c_negative": -1, "rct_begin_c_max": -1, "rct_type_42": -1, "rct_type_negative": -1,
            "rct_unequal_sizes": -2, "squeeze_residual_past_the_list": -2, "squeeze_begin_c_negative": -2, "squeeze_num_c_0": -2,
            "squeeze_begin_c_max": -2, "squeeze_horizontal_mismatch": -1, "squeeze_vertical_mismatch": -6, "squeeze_null_steps": -1,
            "squeeze_negative_n_sp": -1}


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("modchain_check")
    exe = str(tmp / "modchain_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "modchain_check.cpp"), "-o", exe])
    names = sorted(cases.CASES)
    case_file, result = str(tmp / "cases.bin"), str(tmp / "result.bin")
    cases.write_case_file(case_file, names)
    r = subprocess.run([exe, case_file, result], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    return r, names, result


def test_host_walk_equals_the_model_bit_for_bit_under_asan_and_ubsan(check_run):
    r, names, result = check_run
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "0 failure(s)" in r.stdout and "FAIL" not in r.stdout and "%d case(s)" % len(names) in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = cases.read_result_file(result, len(names))
    for name, chans in zip(names, got):
        assert ref.same(chans, cases.expected(name)), name


def test_host_plan_has_the_runs_and_the_path_tables_the_cases_name(check_run):
    """one RUN line per Palette run: its stages, whether it is fusable, and the pixels its path table found in need of a
    neighbour -- none exactly where the model says so (there the program has compared the table's planes with the stages')"""
    r, names, _ = check_run
    runs = {}
    for case, stages, fusable, outs, impure in re.findall(r"^RUN (\d+) (\d+) (\d) (\d+) (-?\d+)$", r.stdout, re.M):
        runs.setdefault(names[int(case)], []).append((int(stages), fusable == "1", int(outs), int(impure)))
    for name in names:
        got = runs.get(name, [])
        assert [(s, f) for s, f, _, _ in got] == cases.CASES[name]["runs"], name
        if len(got) == 1 and got[0][1]:
            assert (got[0][3] > 0) == any(cases.chained(name)), name
    assert [o for _, _, o, _ in runs["sample_shape_33x70"]] == [4] and [o for _, _, o, _ in runs["num_c_18"]] == [18]
    planted = cases.CASES["planted_negative_pred5"]
    assert runs["planted_negative_pred5"][0][3] == int((planted["chans"][-1] == 3).sum()) and runs["planted_negative_pred0"][0][3] == 0
    assert runs["lds_budget_over"][0][3] == -1  # (not fusable: no table to walk)


def test_header_refuses_what_the_entry_must_refuse(check_run):
    r, _, _ = check_run
    got = {n: int(s) for n, s in re.findall(r"^REFUSAL (\w+) (-?\d+) ok$", r.stdout, re.M)}
    assert got == REFUSALS


# ---- the decoder's route rules with and without device_chains, on header stand-ins ----
def _pal(nb_deltas=0, d_pred=0):
    return cases.pal(0, 1, 8, nb_deltas, d_pred)


def test_chain_rule_with_and_without_device_chains():
    from types import SimpleNamespace
    from jxlatte_amd import decoder as D
    rule = D.JXLDecoder._one_plan_chain_rule
    fr = SimpleNamespace(encoding=D.MODULAR)
    P, R, S = ref.PALETTE, ref.RCT, ref.SQUEEZE
    chains = {"four_palettes": [_pal()] * 4, "palette_rct": [_pal(), cases.rct(1, 6)], "rct_rct": [cases.rct(0, 1), cases.rct(0, 2)],
              "squeeze_rct": [cases.squeeze([(1, 1, 0, 1)]), cases.rct(0, 1)], "local_deltas": [_pal(3, 0)], "chained_deltas": [_pal(3, 5)],
              "predictor_6_without_deltas": [_pal(0, 6)]}
    for name, chain in chains.items():
        kinds = [t["kind"] for t in chain]
        off = rule(fr, kinds)
        assert off == ("a Palette in the frame-level chain" if P in kinds else
                       "a frame-level chain that is not one plan ([], [RCT], [Squeeze] or [RCT, Squeeze])"), name
        assert rule(fr, kinds, chain) is None, name
    for chain in ([], [cases.rct(0, 1)], [cases.squeeze([])], [cases.rct(0, 1), cases.squeeze([])]):
        kinds = [t["kind"] for t in chain]
        assert rule(fr, kinds) is None and rule(fr, kinds, chain) is None
    weighted = [_pal(), _pal(1, 6)]
    assert rule(fr, [P, P], weighted) == "a Palette with weighted-predictor deltas"
    assert rule(fr, [P, P]) == "a Palette in the frame-level chain"
    assert rule(SimpleNamespace(encoding=D.VARDCT), [], []) == "not a Modular frame"


def test_frame_set_rule_admits_patches_only_with_the_chain_and_the_patch_sets_rule():
    from test_device_frames_cpu import _header
    from jxlatte_amd.decoder import JXLDecoder
    info, fr, kinds, traced = _header(num_patches=3)
    chain = [cases.rct(0, 1)]
    assert JXLDecoder.frame_set_rule(info, fr, kinds, traced) == "patches"
    assert JXLDecoder.frame_set_rule(info, fr, kinds, traced, chain=chain, patch_sets=False) == "patches"
    assert JXLDecoder.frame_set_rule(info, fr, kinds, traced, chain=None, patch_sets=True) == "patches"
    assert JXLDecoder.frame_set_rule(info, fr, kinds, traced, chain=chain, patch_sets=True) is None
    # the sample the switch exists for: both frames say Palette without it; with it frame 1 qualifies where patch_sets_rule
    # holds and frame 0, reference-only, keeps its way
    from test_device_frames_cpu import NAMES, SAMPLES, _frames
    from jxlatte_amd import frontend
    info, frames = _frames(SAMPLES[NAMES.index("patches-lossless")])
    fe = frontend.Frontend(open(SAMPLES[NAMES.index("patches-lossless")], "rb").read())
    try:
        fe.set_defer_transforms(True)
        chains = []
        while fe.next_frame(None, None) is not None:
            chains.append(fe.transforms())
    finally:
        fe.close()
    assert [f.num_patches for f, _ in frames] == [0, 137]
    got = [JXLDecoder.frame_set_rule(info, f, k, False, chain=c, patch_sets=bool(f.num_patches)) for (f, k), c in zip(frames, chains)]
    assert got == ["not a regular or skip-progressive frame of LF level 0", None]
    assert JXLDecoder.frame_set_rule(info, frames[1][0], frames[1][1], False, chain=chains[1], patch_sets=False) == "patches"
    # every other rule comes behind the chain rule as before: the weighted Palette is named first
    info, fr, kinds, traced = _header(gab=1)
    assert JXLDecoder.frame_set_rule(info, fr, [ref.PALETTE], traced, chain=[_pal(1, 6)]) == "a Palette with weighted-predictor deltas"
    assert JXLDecoder.frame_set_rule(info, fr, [ref.PALETTE], traced, chain=[_pal(1, 5)]) == "a restoration filter or YCbCr"


def test_cli_and_decoder_switch_default_to_off():
    import inspect
    from jxlatte_amd.__main__ import parser
    from jxlatte_amd.decoder import JXLDecoder
    ap = parser()
    assert ap.parse_args(["a.jxl", "o.png"]).device_chains is False
    assert ap.parse_args(["a.jxl", "o.png", "--device-chains"]).device_chains is True
    assert inspect.signature(JXLDecoder.__init__).parameters["device_chains"].default is False and JXLDecoder.device_chains is False


# ---- declarations and bindings ----
def test_header_and_python_declare_the_entry_and_the_hooks_stay_outside_the_abi():
    header = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    assert re.search(r"jxl_status\s+jxl_modular_begin_chain\s*\(", header) and "ModularStream.java:224-380" in header
    vp, i32 = C.c_void_p, C.c_int32
    assert _lib.SIGNATURES["jxl_modular_begin_chain"] == (i32, [vp, C.POINTER(abi.Channel), i32, C.POINTER(abi.ModularTransform), i32, i32])
    body = re.search(r"typedef struct jxl_modular_transform \{(.*?)\} jxl_modular_transform;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:int32_t|const jxl_squeeze_param\*)\s+([^;]+);", body) for n in re.findall(r"[a-z_]+", decl)]
    assert names == [f[0] for f in abi.ModularTransform._fields_] == ["kind", "begin_c", "num_c", "rct_type", "nb_colors", "nb_deltas", "d_pred",
                                                                       "sp", "n_sp"]
    assert C.sizeof(abi.ModularTransform) == 48 and abi.ModularTransform.sp.offset == 32 and abi.ModularTransform.n_sp.offset == 40
    from jxlatte_amd import frontend
    for k, v in (("RCT", frontend.TRANSFORM_RCT), ("PALETTE", frontend.TRANSFORM_PALETTE), ("SQUEEZE", frontend.TRANSFORM_SQUEEZE)):
        assert int(re.search(r"#define JXL_TRANSFORM_%s\s+(\d+)" % k, header).group(1)) == v == getattr(ref, k)
    lib = _lib.load()
    assert hasattr(lib, "jxl_modular_begin_chain")
    for hook in ("jxl_debug_set_palette_fuse", "jxl_debug_last_palette_run"):
        assert hasattr(lib, hook) and hook not in header


def test_make_transforms_forwards_the_frontends_dictionaries():
    c = cases.CASES["palette_squeeze"]
    arr, keep = abi.make_transforms(c["transforms"])
    assert (arr[0].kind, arr[0].begin_c, arr[0].num_c, arr[0].nb_colors, arr[0].n_sp) == (ref.PALETTE, 0, 2, 30, 0)
    assert arr[1].kind == ref.SQUEEZE and arr[1].n_sp == 2
    assert [(arr[1].sp[j].horizontal, arr[1].sp[j].in_place, arr[1].sp[j].begin_c, arr[1].sp[j].num_c) for j in range(2)] == c["transforms"][1]["steps"]


def test_no_context_is_refused_without_a_crash():
    arr, keep = abi.make_transforms([cases.pal(0, 1, 2)])
    assert _lib.load().jxl_modular_begin_chain(None, None, 0, arr, 1, 8) != 0
