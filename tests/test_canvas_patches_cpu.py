"""CPU-only checks of patches on plane sets: jxl_canvas_patches_check (through ctypes, no device) against jxl_patch_bins and its
own set-level refusals; what jxl_canvas_cast_planes refuses, through tools/native/canvas_patch_check.cpp built under
AddressSanitizer and UBSan and run as a child process (the sanitizer runtimes are linked statically, so the program needs nothing
from its environment); JXLDecoder.patch_sets_rule case by case; and the decoder's route under a backend that records its calls and
does no arithmetic."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import patch_ref as R
from jxlatte_amd import _lib, abi, host
from jxlatte_amd import decoder as D
from test_patches_cpu import _random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.dtype(np.float32), np.dtype(np.int32)
FL, IN = abi.PLANE_FLOAT, abi.PLANE_INT32


def _shape(n, h, w, types):
    s = abi.CanvasShape()
    s.n, s.h, s.w = n, h, w
    for i, t in enumerate(types[:abi.CANVAS_MAX_PLANES]):
        s.types[i] = t
    return s


def _outcome(call):
    try:
        call()
    except _lib.JxlError as e:
        return type(e), str(e), e.position
    return None


# ---- jxl_canvas_patches_check -------------------------------------------------------------------------------------------------
def test_check_entry_equals_patch_bins_on_300_seeded_cases():
    """the lists of tests/test_patches_cpu.py as they come (no type plan: many are refused): status, message and first_bad of the
    check entry on sets of the case's sizes and types are jxl_patch_bins' for the same list and types. A slot's absent plane is a
    plane of its frame plane's type (a set has every plane)"""
    n_ok = n_refused = 0
    kinds = set()
    for seed in range(300):
        info, patches, frame, reference = _random_case(seed)
        n_chan = len(frame)
        pos, blend = R.pos_table(info, patches)
        is_alpha, assoc = [t == 0 for t in info.ec_type], [bool(v) for v in info.ec_alpha_associated]
        ft = [FL if b.dtype == F else IN for b in frame]
        rt = [[-1] * n_chan if r is None else [ft[n] if a is None else (FL if a.dtype == F else IN) for n, a in enumerate(r)] for r in reference]
        shapes = [None if r is None else tuple(r[0].shape) for r in reference]
        h, w = frame[0].shape
        a = _outcome(lambda: host.patch_bins(pos, blend, 3, is_alpha, assoc, h, w, ft, shapes, rt))
        sets = [None if r is None else _shape(n_chan, shapes[k][0], shapes[k][1], rt[k]) for k, r in enumerate(reference)]
        b = _outcome(lambda: host.canvas_patches_check(pos, blend, 3, is_alpha, assoc, _shape(n_chan, h, w, ft), sets))
        assert a == b, (seed, a, b)
        n_ok += a is None
        n_refused += a is not None
        if a is not None:
            kinds.add((a[0].__name__, a[1]))
    assert n_ok > 50 and n_refused > 50 and len(kinds) >= 5, (n_ok, n_refused, kinds)


def test_check_entry_refuses_the_sets_it_cannot_run():
    pos = np.array([(4, 4, 8, 8, 0, 0, 0, 0), (20, 30, 8, 8, 2, 1, 1, 0)], abi.PATCH_POS_DTYPE)
    blend = np.array([[[2, 0, 0]] * 4], np.int32)
    frame, small, full = _shape(4, 40, 50, [FL] * 4), _shape(4, 16, 16, [FL] * 4), _shape(4, 40, 50, [FL] * 4)

    def check(frame=frame, refs=(small, None, full, None), n_color=3, blend=blend, is_alpha=(True,), resident=False):
        host.canvas_patches_check(pos, blend, n_color, list(is_alpha), [False] * len(is_alpha), frame, list(refs), colorsResident=resident)
    check()
    check(resident=True, frame=_shape(4, 40, 50, [IN, IN, IN, FL]))  # (the set's own colour planes are not looked at)
    check(refs=(small, small, full, None))  # two slots, one set
    for exc, msg, kw in (
            (_lib.IllegalArgumentException, "frame set holds one plane per channel", dict(frame=_shape(3, 40, 50, [FL] * 3))),
            (_lib.IllegalArgumentException, "reference set holds one plane per channel", dict(refs=(small, None, _shape(5, 40, 50, [FL] * 5), None))),
            (_lib.UnsupportedOperationException, "more than 16 planes",
             dict(frame=_shape(17, 40, 50, [FL] * 16), refs=(None,) * 4, blend=np.array([[[2, 0, 0]] * 17], np.int32), is_alpha=(False,) * 14)),
            (_lib.IllegalArgumentException, "three colour planes",
             dict(resident=True, n_color=1, frame=_shape(2, 40, 50, [FL] * 2), refs=(None,) * 4, blend=np.array([[[2, 0, 0]] * 2], np.int32))),
            (_lib.IllegalArgumentException, "frame set is a reference set", dict(refs=(small, None, frame, None))),
            (_lib.IllegalArgumentException, "bad plane set", dict(frame=_shape(4, 40, 50, [FL, 2, FL, FL]))),
            # ... and then jxl_patch_bins' own, on the sets' sizes and types
            (_lib.InvalidBitstreamException, "Patch too large", dict(refs=(_shape(4, 7, 16, [FL] * 4), None, full, None))),
            (_lib.IllegalArgumentException, "differ in type", dict(refs=(_shape(4, 16, 16, [FL, IN, FL, FL]), None, full, None))),
            (_lib.UnsupportedOperationException, "away from the pixel", dict(blend=np.array([[[5, 0, 0]] * 4], np.int32)))):
        with pytest.raises(exc, match=msg):
            check(**kw)
    with pytest.raises(_lib.InvalidBitstreamException) as e:
        check(frame=_shape(4, 27, 50, [FL] * 4), refs=(small, None, _shape(4, 27, 50, [FL] * 4), None))
    assert "Patch size out of bounds" in str(e.value) and e.value.position == 1
    with pytest.raises(_lib.IllegalArgumentException, match="null argument"):
        host.canvas_patches_check(pos, blend, 3, [True], [False], None, [None] * 4)


# ---- the sanitized stand-alone program ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("canvas_patch_check") / "canvas_patch_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tools", "native", "canvas_patch_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_sanitizer_program_builds_and_exits_0(program_lines):
    m = re.fullmatch(r"(\d+) case\(s\), 0 failure\(s\)", program_lines[-1])
    assert m and int(m.group(1)) == len(program_lines) - 1 >= 40, program_lines[-1]
    assert not [ln for ln in program_lines if ln.endswith("FAIL")]


def test_cast_list_refusals(program_lines):
    """what jxl_canvas_cast_planes refuses (the entry itself needs a context; tests/test_canvas_patches_gpu.py calls it): the same
    plane twice, a depth without a maximum, a plane or a set that is not there, 81 items -- and a float plane is skipped
    whatever its depth"""
    got = {ln.split()[1]: (ln.split()[0], int(ln.split()[2])) for ln in program_lines[:-1]}
    inv = ("REFUSAL", abi.JXL_ERR_INVALID_ARGUMENT)
    for name in ("cast_plane_named_twice", "cast_float_plane_named_twice", "cast_depth_0", "cast_depth_32", "cast_depth_64_after_good_items",
                 "cast_plane_past_the_set", "cast_negative_plane", "cast_unknown_set", "cast_negative_set", "cast_81_items", "cast_null_items",
                 "cast_negative_count"):
        assert got[name] == inv, (name, got[name])
    for name in ("cast_nothing", "cast_depths_1_to_31", "cast_float_plane_is_skipped_whatever_its_depth", "cast_every_int_plane_of_three_sets"):
        assert got[name] == ("ACCEPT", 0), (name, got[name])
    assert abi.CANVAS_MAX_CASTS == 80 and sum(1 for n in got if n.startswith("patches_")) >= 25


# ---- the route ----------------------------------------------------------------------------------------------------------------
def test_patch_sets_rule_case_by_case():
    rule = D.JXLDecoder.patch_sets_rule
    assert rule(True, True, True, True, 3, 3) is None
    assert rule(False, True, True, True, 3, 3) == "device_patch_sets is off"
    assert rule(True, False, True, True, 3, 3) == "device_canvas is off"
    assert rule(True, True, False, True, 3, 3) == "device_patches is off"
    assert rule(True, True, True, False, 3, 3) == "the canvas has landed"
    assert rule(True, True, True, True, 1, 1) == "one-colour image"
    assert rule(True, True, True, True, 1, 3) == "one-colour image"  # (a VarDCT frame of a grey image)
    assert rule(True, True, True, True, 3, 1) == "a frame of another colour count"
    assert rule(False, False, False, False, 1, 3) == "device_patch_sets is off"  # the first reason that failed
    # the class default is off, beside the other switches, and the CLI has the flag
    import inspect
    from jxlatte_amd import __main__ as cli
    assert D.JXLDecoder.device_patch_sets is False and D.JXLDecoder.__new__(D.JXLDecoder).device_patch_sets is False
    assert inspect.signature(D.JXLDecoder.__init__).parameters["device_patch_sets"].default is False
    a = cli.parser().parse_args(["in.jxl", "out.png", "--device-canvas", "--device-patches", "--device-patch-sets"])
    assert a.device_patch_sets and not cli.parser().parse_args(["in.jxl"]).device_patch_sets


class FakeSet:
    """host.DeviceCanvas without a device: tags and sizes only, every call noted"""
    log = None

    def __init__(self, types, shape, name):
        self.types, self.shape, self.name, self.id = [abi.PLANE_FLOAT if np.dtype(t) == F else abi.PLANE_INT32 for t in types], tuple(shape), name, 1

    @classmethod
    def create(cls, ctx, types, height, width):
        s = cls(types, (height, width), "set%d" % len(cls.log))
        cls.log.append(("create", s.name, len(types)))
        return s

    @classmethod
    def fromArrays(cls, ctx, arrays):
        s = cls.create(ctx, [a.dtype for a in arrays], *arrays[0].shape)
        for i, a in enumerate(arrays):
            s.upload(i, a)
        return s

    @property
    def dtypes(self):
        return [F if t == abi.PLANE_FLOAT else I for t in self.types]

    def __len__(self):
        return len(self.types)

    def _stand_ins(self, n):
        return [np.broadcast_to(np.zeros((), self.dtypes[c]), self.shape) for c in range(n)]

    def upload(self, plane, a):
        self.types[plane] = abi.PLANE_FLOAT if a.dtype == F else abi.PLANE_INT32
        self.log.append(("upload", self.name, plane))

    def download(self, plane):
        self.log.append(("download", self.name, plane))
        return np.zeros(self.shape, self.dtypes[plane])

    def release(self):
        self.log.append(("release", self.name))

    def canvasShape(self):
        raise AssertionError("not asked for in these runs")


def _route_run(patch_sets, mode=2, ref_origin=(4, 4), **switches):
    """a shell decoder in front of a frame with patches: 3 int32 colours + alpha, slot 0 a host list (saved before the colour
    transform), slot 1 the canvas set itself. Runs _canvas_route, then the patch stage of _chained_tail. Returns (decoder, log,
    the frame's FramePlanes, the canvas set)"""
    log = FakeSet.log = []

    def cast_planes(ctx, items):
        items = list(items)
        log.append(("cast_planes", [(s.name, n, depth) for s, n, depth in items]))
        for s, n, _ in items:
            s.types[n] = abi.PLANE_FLOAT

    def patches_on_sets(frame, refs, pos, blend, n_color, is_alpha, assoc, colorsResident=False):
        log.append(("canvas_patches", frame.name, [None if r is None else r.name for r in refs], len(pos), colorsResident))
    fake_host = types.SimpleNamespace(DeviceCanvas=FakeSet, canvas_cast_planes=cast_planes, canvas_patches=patches_on_sets,
                                      canvas_patches_check=host.canvas_patches_check, _plane_code=host._plane_code)

    class Backend:
        host, ctx, resident = fake_host, object(), True

        def patches(self, frame, ref, pos, blend, n_color, is_alpha, assoc):
            log.append(("stage_patches", len(pos)))

        def keep_planes(self, planes):
            shape = planes.shape

            class Resident:
                def patches(self, extras, ref, pos, blend, is_alpha, assoc):
                    log.append(("resident_patches", len(pos)))

                def download(self):
                    return np.zeros(shape, np.float32)
            return Resident()

        def blend(self, mode, canvas, *a, **kw):
            log.append(("blend", mode))
            return canvas
    info = R.make_info(1)
    info.xyb_encoded, info.height, info.width = 0, 40, 56
    h, w = 40, 56
    canvas = FakeSet([I] * 4, (h, w), "canvas")
    slot0 = [np.zeros((20, 30), np.int32) for _ in range(4)]
    row = [[mode, 0, 0], [mode, 0, 0]]
    patches = [R.patch(0, 1, 2, 12, 20, [(0, 0), (5, 9)], [row] * 2), R.patch(1, ref_origin[0], ref_origin[1], 9, 33, [(4, 4)], [row])]
    dec = R.shell(info, patches, [slot0, canvas, None, None], Backend())
    dec.canvas, dec._dead_sets, dec._landed = canvas, [], None
    dec.device_canvas = dec.device_patches = True
    dec.device_patch_sets = patch_sets
    for k, v in switches.items():
        setattr(dec, k, v)
    fr = types.SimpleNamespace(num_patches=len(patches), type=D.REGULAR_FRAME, encoding=D.MODULAR, upsampling=1, ec_upsampling=[1],
                               save_before_ct=0, save_as_reference=0, has_splines=0, has_noise=0, do_ycbcr=0)
    on_set = dec._canvas_route(fr, False)
    planes = D.FramePlanes(dec.backend, info, [np.zeros((h, w), np.int32) for _ in range(4)], 3)
    dec._chained_tail(fr, planes, False, True, keep=on_set)
    return dec, log, planes, canvas


def test_route_keeps_the_canvas_up_with_the_switch():
    dec, log, planes, canvas = _route_run(True)
    st = dec.stats[-1]
    assert st["canvas"] == "device" and dec._landed is None and dec.canvas is canvas and dec.reference[1] is canvas
    assert st["patches"] == dict(path="plane sets", positions=3, applications=12, segments=1)
    assert not [e for e in log if e[0] == "download"] and not [e for e in log if e[0] in ("stage_patches", "blend")]
    # the frame's planes up once, slot 0's list as a temporary set; one cast call for the frame's, the list's and the canvas'
    # planes, one patch call that names the canvas set as slot 1
    frame_set = planes.set
    assert frame_set is not None and planes.blend_set() is frame_set
    ups = [e for e in log if e[0] == "upload"]
    assert [e[1] for e in ups].count(frame_set.name) == 4 and len(ups) == 8 and "canvas" not in [e[1] for e in ups]
    casts = [e for e in log if e[0] == "cast_planes"]
    assert len(casts) == 1 and sorted(casts[0][1]) == sorted([(name, n, 8) for name in (frame_set.name, "canvas", ups[-1][1]) for n in range(4)])
    calls = [e for e in log if e[0] == "canvas_patches"]
    assert len(calls) == 1 and calls[0][1] == frame_set.name and calls[0][2] == [ups[-1][1], "canvas", None, None] and calls[0][3:] == (3, False)
    assert log.index(casts[0]) < log.index(calls[0])
    # what is left behind: float tags on the canvas (its slot's casts are its own), float planes in the list
    assert canvas.dtypes == [F] * 4 and frame_set.dtypes == [F] * 4 and [b.dtype for b in dec.reference[0]] == [F] * 4


def test_route_lands_a_list_the_launch_cannot_replay():
    """a below mode (5) whose reference rectangle is not the frame rectangle: plan.gather is False, everything lands with that
    reason and the blend calls run as without the switch"""
    dec, log, planes, canvas = _route_run(True, mode=5, ref_origin=(0, 0))
    st = dec.stats[-1]
    assert st["canvas"] == "landed: a below mode reads the frame off its own pixel" and dec._landed == st["canvas"][len("landed: "):]
    assert isinstance(dec.canvas, list) and dec.reference[1] is dec.canvas  # (the alias stays an alias)
    assert [e for e in log if e[0] == "download"] == [("download", "canvas", n) for n in range(4)]
    assert planes.set is None and not [e for e in log if e[0] in ("canvas_patches", "cast_planes", "upload")]
    # 12 applications. An application whose reads lie in earlier rows of the frame plane it writes goes through backend.blend in
    # bands of as many rows as the shift (_blend_live): position (0, 0) from origin (1, 2) reads ahead -- one call --, position
    # (5, 9) from (1, 2) is 12 rows in bands of 4, position (4, 4) from (0, 0) is 9 rows in bands of 4; four channels each
    assert st["patches"]["path"].startswith("blend calls") and len([e for e in log if e[0] == "blend"]) == 4 * (1 + 3 + 3)


@pytest.mark.parametrize("off", [dict(), dict(device_patches=False)], ids=["device_patch_sets off", "device_patches off"])
def test_route_without_the_switch_is_todays(off):
    dec, log, planes, canvas = _route_run(bool(off), **off)  # (device_patch_sets without device_patches does not act)
    st = dec.stats[-1]
    assert st["canvas"] == "landed: a frame with patches" and isinstance(dec.canvas, list) and planes.set is None
    assert [e for e in log if e[0] == "download"] == [("download", "canvas", n) for n in range(4)]
    assert not [e for e in log if e[0] in ("canvas_patches", "cast_planes", "upload", "create")]
    if off:  # device_patches off: one backend.blend per application
        assert st == dict(canvas="landed: a frame with patches", patches=dict(path="blend calls"), plane_moves=[])
        assert len([e for e in log if e[0] == "blend"]) == 12
    else:    # today's row under device_canvas + device_patches
        assert st == dict(canvas="landed: a frame with patches", patches=dict(path="resident planes", positions=3, applications=12, segments=1),
                          plane_moves=["h2d", "d2h"])
        assert [e for e in log if e[0] in ("stage_patches", "resident_patches")] == [("resident_patches", 3)]
