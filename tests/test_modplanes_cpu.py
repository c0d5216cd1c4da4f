"""CPU-only: csrc/modplanes_check.h -- what jxl_canvas_from_modular refuses before it queues anything -- compiled into a program of
its own (tools/native/modplanes_check.cpp) under AddressSanitizer and UBSan and run as a child process. The program hands the
result list over as an exact-size heap array, so a check that reads past it is reported."""
import os
import re
import subprocess

import pytest

from jxlatte_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INV, UNS, STATE = abi.JXL_ERR_INVALID_ARGUMENT, abi.JXL_ERR_UNSUPPORTED, abi.JXL_ERR_STATE
# every refusal the entry documents (include/jxlatte_amd.h), with its status
REFUSALS = {
    "null_desc": INV,
    "no_plan_has_run": STATE, "no_plan_has_run_bad_desc": STATE,
    "n_planes_0": INV, "n_planes_negative": INV, "n_planes_17": UNS, "n_planes_int_max": UNS,
    "height_0": INV, "width_0": INV, "height_negative": INV, "width_negative": INV,
    "channel_negative": INV, "channel_past_the_list": INV, "channel_int_max": INV, "empty_result_list": INV,
    "channel_lower_than_bounds": INV, "channel_narrower_than_bounds": INV, "last_plane_too_small": INV,
    "add_on_int32_plane": INV, "add_channel_negative": INV, "add_channel_past_the_list": INV, "add_channel_other_width": INV,
    "add_channel_other_height": INV,
    "type_2": INV, "type_negative": INV,
}
ACCEPTED = {"three_int32_planes", "one_plane", "sixteen_planes", "bounds_1x1_of_a_1x1_channel", "bounds_equal_to_the_channel",
            "channel_larger_than_bounds", "last_channel_of_the_list", "one_channel_in_every_plane", "float_plane_without_add",
            "float_plane_adds_itself", "xyb_mapping", "planes_past_n_planes_are_not_looked_at"}


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("modplanes_check") / "modplanes_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "modplanes_check.cpp"), "-o", exe])
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


def test_descriptor_mirror_has_the_c_layout():
    import ctypes as C
    assert C.sizeof(abi.ModularPlane) == 16
    assert C.sizeof(abi.ModularPlanesDesc) == 12 + 16 * abi.CANVAS_MAX_PLANES
    src = open(os.path.join(ROOT, "include", "jxlatte_amd.h")).read()
    body = src[src.index("typedef struct jxl_modular_plane {"):src.index("} jxl_modular_planes_desc;")]
    names = re.findall(r"\b(?:int32_t|float)\s+([\w, ]+?)(?:\[\w+\])?;", body)
    flat = [n.strip() for group in names for n in group.split(",")]
    assert flat == [f[0] for f in abi.ModularPlane._fields_] + [f[0] for f in abi.ModularPlanesDesc._fields_][:3]
