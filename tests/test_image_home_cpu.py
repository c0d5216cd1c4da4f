"""An image's home without a GPU: jxlatte_amd/csrc/image_home.h as a stand-alone host program under AddressSanitizer + UBSan
(tools/native/image_home_check.cpp), its refusal codes and upload answers over the program's matrix against the rules restated
here. Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, RESIDENT, SET = 0, 1, 2
OK, UNKNOWN_SET, NO_SUCH_PLANES, NOT_DESCRIBED = 0, 1, 2, 3
# the program's sets: per plane, int32 (1) or float (0); all 5 x 7. -1: an unknown id
VIEWS = {0: [0, 0, 0, 1, 0], 1: [1, 0, 1], 2: [0]}
SHAPE = (5, 7)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("image_home_check") / "image_home_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "image_home_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert r.stdout.strip().endswith("0 failure(s)") and "FAIL" not in r.stdout and "runtime error" not in r.stderr
    return [ln for ln in r.stdout.splitlines() if ln.startswith("CASE")]


def first_half(kind, view, n_color, alpha_plane, has_alpha):
    """the home exists and has the planes asked for"""
    if kind != SET:
        return OK
    if view < 0:
        return UNKNOWN_SET
    n = len(VIEWS[view])
    if n_color not in (1, 3) or n_color > n or not -1 <= alpha_plane < n or bool(has_alpha) != (alpha_plane >= 0):
        return NO_SUCH_PLANES
    return OK


def second_half(kind, view, n_color, alpha_plane, has_alpha, height, width, tags, alpha_tag):
    """the parameters describe the home: host planes are what the parameters say; resident planes are three float planes of their
    size; a set has its size, its planes' tags and the tag of the alpha plane asked for"""
    if kind == HOST:
        return OK
    first = first_half(kind, view, n_color, alpha_plane, has_alpha)
    if first:
        return first
    if (height, width) != SHAPE:
        return NOT_DESCRIBED
    types = [0, 0, 0] if kind == RESIDENT else VIEWS[view]
    if kind == RESIDENT and n_color != 3:
        return NOT_DESCRIBED
    if any(tags[i] != types[i] for i in range(n_color)):
        return NOT_DESCRIBED
    if kind == SET and alpha_plane >= 0 and alpha_tag != types[alpha_plane]:
        return NOT_DESCRIBED
    return OK


def test_codes_equal_the_restated_rules(lines):
    seen = set()
    for ln in lines:
        left, right = ln[5:].split(" : ")
        kind, view, n_color, alpha_plane, has_alpha, height, width, tags, alpha_tag = left.split()
        case = (int(kind), int(view), int(n_color), int(alpha_plane), int(has_alpha), int(height), int(width), [int(t) for t in tags], int(alpha_tag))
        got = [int(v) for v in right.split()]
        want = [first_half(*case[:5]), second_half(*case), int(case[0] == HOST), int(case[0] != SET)]
        assert got == want, ln
        seen.add((case[0], case[1], case[2], case[3]))
    # the matrix: a null CanvasView, n_color 0, 2 and 4, alpha_plane -2, -1, n - 1 and n, every kind of home
    params = 3 * 4 * 2
    assert len(lines) == params * (2 + 2 + 4 * 5 * 5 * 2)
    for n_color in (0, 1, 2, 3, 4):
        for view in (-1, 0, 1, 2):
            n = 5 if view < 0 else len(VIEWS[view])
            for alpha_plane in (-2, -1, n - 1, n):
                assert (SET, view, n_color, alpha_plane) in seen
    assert {(HOST, -1, 3, -1), (RESIDENT, -1, 3, -1), (RESIDENT, -1, 1, -1)} <= seen


def test_every_code_occurs(lines):
    firsts = {int(ln.split(" : ")[1].split()[0]) for ln in lines}
    seconds = {int(ln.split(" : ")[1].split()[1]) for ln in lines}
    assert firsts == {OK, UNKNOWN_SET, NO_SUCH_PLANES} and seconds == {OK, UNKNOWN_SET, NO_SUCH_PLANES, NOT_DESCRIBED}


def test_header_is_pure_host_code():
    text = open(os.path.join(ROOT, "jxlatte_amd", "csrc", "image_home.h")).read()
    for word in ("hip/", "hipStream", "hipMalloc", "jxl_internal.h", "jxl_ctx", "getenv"):
        assert word not in text, word
