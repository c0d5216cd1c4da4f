"""The device patch stage on the GPU: jxl_stage_patches / jxl_planes_patches and JXLDecoder(device_patches=True) against today's
host sequence -- JXLDecoder._patches, one backend.blend per (position, channel) -- driven through oracle.pybackend.OracleBackend
(the C restatement of JXLCodestreamDecoder.java:285-413). Every comparison is tobytes() equality.

Non-finite samples: an INVALID operation (inf - inf, inf * 0, 0 / 0) yields 0xFFC00000 on the oracle's x86 host and 0x7FC00000 on
gfx950 (tests/conftest.py: assert_bits_equal), which no kernel can change; so NaN (with a payload), +-inf and -0.0 samples are
placed where IEEE 754 fixes the result's bits -- sums with finite partners -- and the alpha planes stay inside (0, 1), which keeps
blendBlend's denominator away from 0."""
import io
import os
import types

import numpy as np
import pytest

import patch_ref as R
from jxlatte_amd import _lib, decoder, host

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = os.path.join(ROOT, "tests", "golden", "samples", "patches-lossless.jxl")


@pytest.fixture(scope="module")
def oracle():
    from oracle.pybackend import OracleBackend
    return OracleBackend()


def _stage_backend(ctx):
    return types.SimpleNamespace(patches=lambda *a: host.computePatches(ctx, *a))


def _device(ctx, info, patches, frame, reference):
    fb = [b.copy() for b in frame]
    ref = [None if r is None else [None if a is None else a.copy() for a in r] for r in reference]
    dec = R.shell(info, patches, ref, _stage_backend(ctx))
    assert dec._patches_device(R.frame_rec(patches), decoder.FramePlanes(dec.backend, info, fb, 3)), dec.stats
    return fb, ref, dec.stats[-1]["patches"]


def _assert_same(got, exp, what):
    (gf, gr), (ef, er) = got, exp
    for n, (a, b) in enumerate(zip(gf, ef)):
        assert R.same_bits(a, b), "%s: frame plane %d (%s / %s), %d samples differ" % (
            what, n, a.dtype, b.dtype, -1 if a.dtype != b.dtype else int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))))
    for k in range(4):
        assert (gr[k] is None) == (er[k] is None), (what, k)
        for n, (a, b) in enumerate(zip(gr[k] or [], er[k] or [])):
            assert (a is None) == (b is None) and (a is None or R.same_bits(a, b)), "%s: reference %d plane %d" % (what, k, n)


def _case(seed, n_extra, is_int, h=37, w=75):
    """random positions over four slots: 0 smaller than the frame, 1 frame-sized (the below modes live here, at their own
    pixel), 2 absent, 3 frame-sized with missing planes"""
    rng = np.random.default_rng(seed)
    ec_type = [0 if rng.random() < 0.6 else 3 for _ in range(n_extra)]
    info = R.make_info(n_extra, ec_type=ec_type, assoc=[int(rng.integers(0, 2)) for _ in range(n_extra)])
    n_chan = 3 + n_extra

    def plane(shape, alpha):
        if is_int:
            return rng.integers(-300, 300, shape).astype(np.int32)
        if alpha:
            return rng.uniform(0.1, 0.9, shape).astype(F)
        a = rng.uniform(-0.5, 1.5, shape).astype(F)
        a.reshape(-1)[rng.choice(a.size, a.size // 40, replace=False)] = F(-0.0)
        return a
    frame = [plane((h, w), c >= 3) for c in range(n_chan)]
    small = (23, 41)
    reference = [[plane(small, c >= 3) for c in range(n_chan)], [plane((h, w), c >= 3) for c in range(n_chan)], None,
                 [None if c in (1, n_chan - 1) else plane((h, w), c >= 3) for c in range(n_chan)]]
    modes = [0, 2] + ([3, 4, 5, 6, 7] if not is_int or n_extra == 0 else [])  # (mode 1 is refused: test_mode_1_is_refused)
    patches = []
    for i in range(int(rng.integers(6, 10))):
        ph, pw = [(1, 1), (3, 5), (9, 40), (12, 70), (2, 33)][int(rng.integers(0, 5))] if rng.random() < 0.5 else (int(rng.integers(1, 20)), int(rng.integers(1, 38)))
        row = [[int(rng.choice(modes)), int(rng.integers(0, max(1, n_extra))), int(rng.integers(0, 2))] for _ in range(1 + n_extra)]
        below = any(m in (5, 7) for m, _, _ in row)
        copies_ref = any(m in (4, 6) for m, _, _ in row[1:])  # blendMulAdd's alpha case reads the slot at the frame rectangle
        slot = int(rng.choice([1, 3])) if below or copies_ref else int(rng.choice([0, 0, 1, 2, 3]))
        if slot == 3 and any(m in (3, 5) for m, _, _ in row):
            slot = 1  # blendBlend reads the slot's alpha plane, which blendBuffers does not create for these raw modes (:446-456)
        rh, rw = small if slot == 0 else (h, w)
        ph, pw = min(ph, rh), min(pw, rw)
        if below:
            y0, x0 = int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1))
            positions = [(y0, x0)]
        else:
            y0, x0 = int(rng.integers(0, rh - ph + 1)), int(rng.integers(0, rw - pw + 1))
            edge = [(0, 0), (h - ph, w - pw), (0, w - pw), (h - ph, 0)]
            positions = [edge[int(rng.integers(0, 4))] if rng.random() < 0.3 else (int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1)))
                         for _ in range(int(rng.integers(1, 6)))]
        patches.append(R.patch(slot, y0, x0, ph, pw, positions, [row] * len(positions)))
    return info, patches, frame, reference


@pytest.mark.parametrize("is_int", [False, True], ids=["float", "int"])
@pytest.mark.parametrize("n_extra", [0, 1, 2])
def test_stage_equals_the_oracle_sequence(ctx, oracle, n_extra, is_int):
    """3 colours + 0 / 1 / 2 extras, float and int: every mode x clamp x associated x is-alpha the types admit, 1x1 patches and
    patches larger than a tile, positions flush with the four frame edges, a reference smaller than the frame, an absent slot and
    NULL reference planes. The generator stays inside what today's path computes (no blendBlend against a missing alpha plane of
    the slot, below modes at their own pixel); should the yardstick still refuse a list, the next seed is drawn -- 12 lists per
    case and the modes, clamp, associated and is-alpha values reached are asserted."""
    seen, ran, seed = set(), 0, 1000 * n_extra + (500 if is_int else 0)
    while ran < 12 and seed % 500 < 200:
        seed += 1
        info, patches, frame, reference = _case(seed, n_extra, is_int)
        try:
            exp = R.host_sequence(info, patches, frame, reference, oracle)
        except RuntimeError:
            continue
        got = _device(ctx, info, patches, frame, reference)
        _assert_same(got[:2], exp, "seed %d" % seed)
        again = _device(ctx, info, patches, frame, reference)
        _assert_same(again[:2], got[:2], "seed %d, second run" % seed)
        ran += 1
        for p in patches:
            if reference[p["ref"]] is None:
                continue
            for c, (m, a, cl) in enumerate(p["blend"][0]):
                ex = c - 1
                seen.add((int(m), int(cl), bool(info.ec_alpha_associated[a]) if n_extra else False, ex >= 0 and info.ec_type[ex] == 0))
    assert ran == 12, ran
    want = {m for m in ([0, 2] if is_int and n_extra else range(8)) if m != 1}
    assert {s[0] for s in seen} == want and {s[1] for s in seen} == {0, 1}, sorted(seen)
    if n_extra:
        assert {s[2] for s in seen} == {False, True} and {s[3] for s in seen} == {False, True}, sorted(seen)


def test_deep_overlap_and_untouched_pixels_keep_their_bits(ctx, oracle):
    info = R.make_info(1)
    rng = np.random.default_rng(7)
    h, w = 64, 96
    frame = [rng.uniform(-0.5, 1.5, (h, w)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (h, w)).astype(F)]
    frame[0][::3, ::5] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), F)[0]  # NaN with a payload, -0.0: must survive where uncovered
    frame[1][1::3, ::5] = F(-0.0)
    ref = [rng.uniform(-0.5, 1.5, (20, 30)).astype(F) for _ in range(3)] + [rng.uniform(0.1, 0.9, (20, 30)).astype(F)]
    rows = [[[3, 0, 1], [3, 0, 0]], [[2, 0, 0], [0, 0, 0]], [[4, 0, 1], [2, 0, 0]], [[6, 0, 0], [3, 0, 1]]]
    frame[0][20:40, 30:60] = rng.uniform(0, 1, (20, 30)).astype(F)  # (the covered part: finite)
    patches = [R.patch(0, 0, 0, 12, 20, [(20 + k, 30 + k) for k in range(5)], [rows[(i + k) % 4] for k in range(5)]) for i in range(3)]
    depth = np.zeros((h, w), int)
    for p in patches:
        for y0, x0 in p["positions"]:
            depth[y0:y0 + 12, x0:x0 + 20] += 1
    assert depth.max() >= 8
    exp = R.host_sequence(info, patches, frame, [ref, None, None, None], oracle)
    got = _device(ctx, info, patches, frame, [ref, None, None, None])
    _assert_same(got[:2], exp, "deep overlap")
    for n in range(4):
        assert got[0][n][depth == 0].tobytes() == frame[n][depth == 0].tobytes()
    assert got[2]["segments"] == 1


def test_non_finite_samples_and_the_order_witness(ctx, oracle):
    """float ADD: NaN payloads, +-inf and -0.0 in the frame with finite reference samples, overlapping; and the witness of
    tests/test_patches_cpu.py, which changes under a reversal of the list"""
    info, patches, frame, reference = R.order_witness()
    exp = R.host_sequence(info, patches, frame, reference, oracle)
    got = _device(ctx, info, patches, frame, reference)
    _assert_same(got[:2], exp, "order witness")
    assert got[0][0][8, 12] == 0.0
    rev = R.host_sequence(info, patches[::-1], frame, reference, oracle)
    assert not R.same_bits(rev[0][0], got[0][0])
    rng = np.random.default_rng(11)
    frame = [rng.uniform(-1, 1, (24, 40)).astype(F) for _ in range(3)]
    specials = np.frombuffer(np.array([0x7FC00001, 0xFFC54321, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32).tobytes(), F)
    for c in range(3):
        frame[c].reshape(-1)[rng.choice(24 * 40, 300, replace=False)] = specials[rng.integers(0, 6, 300)]
    ref = [rng.uniform(-1, 1, (16, 32)).astype(F) for _ in range(3)]
    ref[0][:4, :8] = F(-0.0)
    patches = [R.patch(0, 0, 0, 10, 20, [(3, 5), (8, 11), (14, 20)], [[[2, 0, 0]]] * 3), R.patch(0, 0, 0, 4, 8, [(0, 0), (20, 32)], [[[2, 0, 0]]] * 2)]
    exp = R.host_sequence(info, patches, frame, [ref, None, None, None], oracle)
    got = _device(ctx, info, patches, frame, [ref, None, None, None])
    assert np.isnan(exp[0][0]).any() and np.isinf(exp[0][0]).any() and (exp[0][0].view(np.uint32) == 0x80000000).any()
    _assert_same(got[:2], exp, "non-finite samples")


def test_mode_1_is_refused(ctx, oracle):
    """patch mode 1 becomes BLEND_REPLACE, for which blendBuffers' switch has no case (JXLCodestreamDecoder.java:484, :510-511):
    host path, plan and stage entry answer "Illegal blend mode", the device routes before a plane is touched"""
    info, patches, frame, reference = _case(1001, 1, False)
    patches = patches + [R.patch(1, 2, 3, 4, 5, [(1, 1)], [[[2, 0, 0], [1, 0, 1]]])]
    with pytest.raises(decoder.InvalidBitstreamException, match="Illegal blend mode"):
        R.host_sequence(info, patches, frame, reference, oracle)
    fb = [b.copy() for b in frame]
    dec = R.shell(info, patches, [None if r is None else list(r) for r in reference], _stage_backend(ctx))
    with pytest.raises(decoder.InvalidBitstreamException, match="Illegal blend mode"):
        dec._patches_device(R.frame_rec(patches), decoder.FramePlanes(dec.backend, info, fb, 3))
    assert all(R.same_bits(a, b) for a, b in zip(fb, frame))
    pos, blend = R.pos_table(info, patches)
    with pytest.raises(_lib.InvalidBitstreamException, match="Illegal blend mode"):
        host.computePatches(ctx, fb, [None if r is None else list(r) for r in reference], pos, blend, 3, [t == 0 for t in info.ec_type],
                            [bool(v) for v in info.ec_alpha_associated])
    assert all(R.same_bits(a, b) for a, b in zip(fb, frame))


def test_casts_in_the_middle_run_as_segments(ctx, oracle):
    """int planes added as ints, then a mode that casts a plane already used: two launches with the reference's cast in between"""
    info = R.make_info(1)
    rng = np.random.default_rng(5)
    frame = [rng.integers(0, 255, (30, 50)).astype(np.int32) for _ in range(4)]
    ref = [rng.integers(0, 255, (30, 50)).astype(np.int32) for _ in range(4)]
    cast_all = R.patch(0, 0, 0, 10, 10, [(3, 3), (12, 30)], [[[2, 0, 0], [2, 0, 0]]] * 2)    # mode 2 with alpha: casts everything
    # mode 1 on ints casts nothing and then meets the switch of blendBuffers, which has no case for it: the list is refused
    refused = [R.patch(0, 2, 3, 8, 9, [(1, 1), (5, 6)], [[[1, 0, 0], [0, 0, 0]]] * 2), cast_all]
    with pytest.raises(decoder.InvalidBitstreamException, match="Illegal blend mode"):
        R.host_sequence(info, refused, frame, [ref, None, None, None], oracle)
    with pytest.raises(decoder.InvalidBitstreamException, match="Illegal blend mode"):
        _device(ctx, info, refused, frame, [ref, None, None, None])
    patches = [R.patch(0, 2, 3, 8, 9, [(1, 1), (5, 6)], [[[0, 0, 0], [6, 0, 0]]] * 2),      # mode 6 on the int alpha channel: a copy, no cast
               R.patch(0, 2, 3, 8, 9, [(4, 4)], [[[0, 0, 0], [6, 0, 1]]]), cast_all]
    exp = R.host_sequence(info, patches, frame, [ref, None, None, None], oracle)
    got = _device(ctx, info, patches, frame, [ref, None, None, None])
    _assert_same(got[:2], exp, "segments")
    assert got[2]["segments"] >= 2 and got[0][0].dtype == F


def test_resident_entry_equals_the_stage_entry(ctx, oracle):
    for base, n_extra in ((1000, 1), (2000, 2), (0, 0)):
        for seed in range(base + 1, base + 200):
            info, patches, frame, reference = _case(seed, n_extra, False)
            try:
                exp = R.host_sequence(info, patches, frame, reference, oracle)
            except RuntimeError:
                continue
            plan = decoder.patch_type_plan(info, patches, frame, reference, 3)
            if len(plan.segments) == 1:
                break
        else:
            pytest.fail("no case")
        staged = _device(ctx, info, patches, frame, reference)
        rp = host.ResidentPlanes.upload(ctx, np.stack(frame[:3]))
        extras = [b.copy() for b in frame[3:]]
        is_alpha, assoc = [t == 0 for t in info.ec_type], [bool(v) for v in info.ec_alpha_associated]
        rp.patches(extras, [None if r is None else list(r) for r in reference], plan.pos, plan.blend, is_alpha, assoc)
        got = list(rp.download()) + extras
        for n in range(3 + n_extra):
            assert R.same_bits(np.ascontiguousarray(got[n]), staged[0][n]) and R.same_bits(staged[0][n], exp[0][n]), (seed, n)
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.IllegalStateException):
            host.ResidentPlanes(fresh).patches([], [None] * 4, plan.pos, plan.blend, [], [])
    finally:
        fresh.close()


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
class _Counting:
    """DeviceBackend with its blend calls counted"""

    def __init__(self, inner):
        self.inner, self.blends = inner, 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def blend(self, *a, **kw):
        self.blends += 1
        return self.inner.blend(*a, **kw)


@pytest.fixture(scope="module")
def device_backend():
    be = decoder.DeviceBackend()
    yield be
    be.close()


def _decode(backend, **kw):
    be = _Counting(backend)
    dec = decoder.JXLDecoder(SAMPLE, backend=be, **kw)
    in_patches = []
    if not kw:
        inner = dec._patches

        def counted(*a):
            n = be.blends
            inner(*a)
            in_patches.append(be.blends - n)
        dec._patches = counted
    else:
        inner = dec._patches_device

        def counted(*a):
            n = be.blends
            r = inner(*a)
            in_patches.append(be.blends - n)
            return r
        dec._patches_device = counted
    image = dec.decode()
    out = io.BytesIO()
    decoder.PNGWriter(image).write(out)
    return dec, image, out.getvalue(), in_patches


def test_patches_lossless_sample_in_one_launch(device_backend):
    """the reference's own sample (1600 x 1096 lossless screenshot, 137 patches at 650 positions): every buffer, every dtype,
    self.reference and the PNG bytes equal the default device decode; no backend.blend inside the patch stage; the planes go up
    once and come down once"""
    d0, im0, png0, n0 = _decode(device_backend)
    d1, im1, png1, n1 = _decode(device_backend, device_patches=True)
    assert sum(n0) == 1950 and n1 == [0], (n0, n1)
    st = d1.stats[-1]
    assert st["patches"]["path"] == "resident planes" and st["patches"]["segments"] == 1 and st["patches"]["positions"] == 650
    assert st["plane_moves"].count("h2d") <= 1 and st["plane_moves"].count("d2h") <= 1, st["plane_moves"]
    assert len(im0.buffer) == len(im1.buffer)
    for a, b in zip(im0.buffer, im1.buffer):
        assert R.same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b))
    for a, b in zip(d0.canvas, d1.canvas):
        assert R.same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b))
    for k in range(4):
        assert (d0.reference[k] is None) == (d1.reference[k] is None)
        for a, b in zip(d0.reference[k] or [], d1.reference[k] or []):
            assert (a is None) == (b is None) and (a is None or R.same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b)))
    assert png0 == png1


class _Rec:
    """a frame record for _chained_tail: upsampling 2, patches, splines, noise, XYB"""
    upsampling, num_patches, has_splines, has_noise, save_before_ct, save_as_reference, do_ycbcr = 2, 2, 1, 1, 0, 0, 0
    group_dim, base_corr_x, base_corr_b = 256, 0.0, 1.0
    noise = [0.01 * (i + 1) for i in range(8)]


def _tail(device_backend, device_patches, start_resident):
    import spline_ref as S
    h, w = 48, 64
    planes = S.random_planes(51, h, w)
    splines = S.random_splines(52, 4, 2 * h, 2 * w, sigma=(3, 10))
    rng = np.random.default_rng(53)
    ref = [rng.uniform(-0.2, 0.2, (40, 60)).astype(F) for _ in range(3)]
    row = [[2, 0, 0]]
    patches = [R.patch(1, 2, 3, 20, 30, [(0, 0), (10, 15), (76, 98)], [row] * 3), R.patch(1, 0, 0, 9, 33, [(40, 50), (44, 60)], [row] * 2)]
    dec = decoder.JXLDecoder.__new__(decoder.JXLDecoder)
    dec.backend, dec.device_splines, dec.device_patches = device_backend, True, device_patches
    dec.visibleFrames, dec.invisibleFrames, dec.stats, dec.reference = 1, 0, [{}], [None, ref, None, None]

    class Info:
        bits_per_sample, xyb_encoded, intensity_target = 8, 1, 255.0
        prim_xy, white_xy = list(decoder.PRI_SRGB), list(decoder.WP_D65)
        opsin_matrix = [11.031566901960783, -9.866943921568629, -0.16462299647058826, -3.254147380392157, 4.418770392156863,
                        -0.16462299647058826, -3.6588512862745097, 2.7129230470588235, 1.9459282392156863]
        opsin_bias = [-0.0037930732552754493] * 3
        custom_up = [0, 0, 0]
        colour_space, num_extra, ec_type, ec_alpha_associated, ec_bits = decoder.CE_RGB, 0, [], [], []

    class Fe(R.Fe):
        def splines(self):
            return splines
    dec.info, dec.fe = Info, Fe(patches)
    buffers = [planes[c].copy() for c in range(3)]
    rp = device_backend.keep_planes(planes) if start_resident else None
    dec._chained_tail(_Rec, decoder.FramePlanes(device_backend, Info, buffers, 3, rp=rp), False, False)
    return np.stack(buffers[:3]), dec.stats[-1]


@pytest.mark.parametrize("start_resident", [False, True])
def test_chained_tail_keeps_the_planes_on_the_device(device_backend, start_resident):
    """upsampling 2 + patches + splines + noise + XYB with device_patches and device_splines: one way down, at the end; the samples
    equal the staged sequence, in which the planes come down for the patches' blend calls and go up again"""
    on, st_on = _tail(device_backend, True, start_resident)
    off, st_off = _tail(device_backend, False, start_resident)
    first = [] if start_resident else ["h2d"]
    assert st_on["plane_moves"] == first + ["d2h"] and st_on["patches"]["path"] == "resident planes"
    assert st_off["plane_moves"] == first + ["d2h", "h2d", "d2h"] and st_off["patches"]["path"] == "blend calls"
    assert on.shape == (3, 96, 128) and on.tobytes() == off.tobytes()
