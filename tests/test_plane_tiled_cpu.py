"""CPU-only: the cell-tiled plane layout of jxlatte_amd/csrc/plane_tiled.h -- the one header the IDCT launch's stores and the
restoration kernel's tile loader share -- as a stand-alone host program under AddressSanitizer + UBSan
(tools/native/plane_tiled_check.cpp: the offsets against the formula for every sample of a 72 x 40 plane and others, cells tile the
plane without overlap, the store / gather pair of the two kernels round-trips inside the allocation). The sanitizer runtimes are
linked statically, so the program needs nothing from its environment."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_tiled_layout_under_asan(tmp_path):
    exe = str(tmp_path / "plane_tiled_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "plane_tiled_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "0 failure(s)" in r.stdout and "FAIL" not in r.stdout
