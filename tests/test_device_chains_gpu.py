"""GPU: JXLDecoder(device_chains=True) with device_canvas, device_patches, device_patch_sets and device_frames -- any frame-level
transform chain is one plan of the Modular context, and a frame with patches stays a plane set through the patch stage --
against the default decoder: planes (dtype, shape, bits), the PNG's samples and the PFM's bytes, equality everywhere; which route
each frame takes; what crosses the bus; which backend hooks run. patches-lossless.jxl is the sample the switch exists for: its
1600 x 1096 frame undoes four nested Palette transforms and applies 137 patches. The comparison helpers and the cache of default
decodes are tests/test_device_frames_gpu.py's."""
import io

import pytest

from jxlatte_amd import frontend, host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, PFMWriter
from test_device_frames_gpu import NAMES, SET, CountingBackend, _check_image, _decode, _path, _reference

pytestmark = pytest.mark.gpu
SWITCHES = dict(device_canvas=True, device_patches=True, device_patch_sets=True, device_frames=True, device_chains=True)
SAMPLE = "patches-lossless"


class ChainBackend(CountingBackend):
    """... and a counter around the palette hook"""

    def palette(self, *a, **kw):
        self.calls["palette"] += 1
        return DeviceBackend.palette(self, *a, **kw)


@pytest.fixture(scope="module")
def backend(ctx):
    return ChainBackend(ctx)


def _encoded_bytes(name, frame):
    """the bytes of the encoded channel list of one frame, meta channels included: what jxl_modular_begin_chain takes up"""
    fe = frontend.Frontend(open(_path(name), "rb").read())
    try:
        fe.set_defer_transforms(True)
        for _ in range(frame + 1):
            assert fe.next_frame(None, None) is not None
        return sum(fe.modular_channel(i)[0].nbytes for i in range(fe.modular_channel_count()))
    finally:
        fe.close()


@pytest.mark.parametrize("device_image", [False, True], ids=["", "image"])
def test_patches_lossless_runs_its_palettes_and_patches_on_the_device(backend, device_image):
    _reference(backend, SAMPLE)  # (first: a default decode takes the context's resident planes)
    pfm = io.BytesIO()
    dec0 = JXLDecoder(_path(SAMPLE), backend=backend)
    PFMWriter(dec0.decode()).write(pfm)
    dec0.close()
    dec, im = _decode(_path(SAMPLE), backend, device_image=device_image, **SWITCHES)
    try:
        st = dec.stats
        print([s["frame"] for s in st], [s["canvas"] for s in st], [s["blend_bus"] for s in st], st[1].get("chain"), st[1].get("patches"))
        assert len(st) == 2
        assert st[1]["frame"] == SET  # (without device_chains: "host: a Palette in the frame-level chain")
        assert st[1]["canvas"] == "device"
        assert st[1]["patches"]["path"] == "plane sets"
        assert st[0]["frame"].startswith("host: ")  # the 198 x 198 reference-only frame keeps its way
        P = frontend.TRANSFORM_PALETTE
        assert st[1]["chain"] == dict(kinds=[P] * 4, runs=dict(fused=1, steps=0, redone=0)) and "chain" not in st[0]
        # no frame-level transform of frame 1 went through a hook (frame 0's palettes run in the front-end's loop)
        assert backend.calls["palette"] == backend.calls["rct"] == backend.calls["squeeze"] == 0
        assert backend.calls["modular_to_float"] == backend.calls["keep_planes"] == 0
        # the bus: the encoded channels up once, and the one reference slot that is a host list (frame 0, saved before the
        # colour transform) as the patch stage's temporary set; nothing comes down before the output samples
        slots = [r for r in dec.reference if r is not None and not dec._is_set(r)]
        slot_bytes = sum(a.nbytes for a in slots[0] if a is not None)
        encoded = _encoded_bytes(SAMPLE, 1)
        assert len(slots) == 1 and slot_bytes > 0 and 6.9e6 < encoded < 7.1e6
        assert st[1]["blend_bus"] == (encoded + slot_bytes, 0)
        assert (im.planeSet is not None) == device_image
        out = io.BytesIO()
        PFMWriter(im, deviceSamples=True).write(out)
        assert out.getvalue() == pfm.getvalue()
        _check_image(backend, SAMPLE, im)
    finally:
        dec.close()


def test_with_device_palette_only_frame_0_reaches_the_palette_hook(backend):
    dec, im = _decode(_path(SAMPLE), backend, device_palette=True, **SWITCHES)
    try:
        assert dec.stats[1]["frame"] == SET and backend.calls["palette"] == 4
        assert len(dec.stats[0]["palette"]) == 4 and dec.stats[1]["palette"] == []
        _check_image(backend, SAMPLE, im)
    finally:
        dec.close()


def test_step_form_gives_the_same_image(backend, ctx):
    before = host.setPaletteFuse(ctx, False)
    try:
        dec, im = _decode(_path(SAMPLE), backend, **SWITCHES)
        try:
            assert dec.stats[1]["frame"] == SET and dec.stats[1]["chain"]["runs"] == dict(fused=0, steps=4, redone=0)
            _check_image(backend, SAMPLE, im)
        finally:
            dec.close()
    finally:
        host.setPaletteFuse(ctx, before)


def test_switch_off_leaves_the_routes_and_the_rows(backend):
    on = dict(SWITCHES, device_chains=False)
    dec, im = _decode(_path(SAMPLE), backend, **on)
    try:
        assert [s["frame"] for s in dec.stats] == ["host: a Palette in the frame-level chain"] * 2
        assert all("chain" not in s for s in dec.stats)
        _check_image(backend, SAMPLE, im)
    finally:
        dec.close()


@pytest.mark.parametrize("name", [n for n in NAMES if n != SAMPLE])
def test_every_other_sample_decodes_to_the_default_decoders_bits(backend, name):
    _reference(backend, name)  # (first: a default decode takes the context's resident planes)
    dec, im = _decode(_path(name), backend, **SWITCHES)
    try:
        ref_stats = _reference(backend, name)[2]
        assert len(dec.stats) == len(ref_stats)
        for s in dec.stats:  # the key is there exactly for the frames whose chain ran as a plan
            assert ("chain" in s) == (s["frame"] == SET), (name, s["frame"])
        _check_image(backend, name, im)
    finally:
        dec.close()
