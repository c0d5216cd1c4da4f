"""JXLDecoder(downsample=8) on the device: the LF image of a whole frame in one launch (csrc/k_lf_image.hip).

* kernel parity: jxl_stage_lf_image against the oracle composition of tests/test_lf_preview_cpu.py (pyoracle.lf_dequant per LF group
  at a 256-cell pitch, pyoracle.xyb), bit for bit, smoothing on and off, XYB on and off, on grids of one, two and four LF groups
  whose integers put the smoothing gap into all three regimes;
* jxl_planes_from_lf + jxl_planes_download equals jxl_stage_lf_image;
* the decoder on the device backend equals the decoder on the oracle backend bit for bit, with and without device_output; the
  resident preview feeds toTensor(size=) and PNGWriter(deviceSamples=True) as the same planes do from host arrays, and nothing
  comes down."""
import io

import numpy as np
import pytest
import torch

import jxl_writer_vardct_cases as C
import pixel_ref64 as P
import pixel_ref64_cases as PC
import test_lf_preview_cpu as L
from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host
from jxlatte_amd.decoder import DeviceBackend, JXLDecoder, JXLImage, PNGWriter

pytestmark = pytest.mark.gpu
F = np.float32
# one group; two side by side (columns 255 and 256 are seam borders: copies); a one-row second group, which has no interior; four
GRIDS = [(1, 1), (2, 7), (3, 3), (33, 47), (33, 288), (257, 2), (260, 300)]
SD = PC.lf_sd(4)  # with extraPrecision 0: every smoothing regime holds a tenth of an interior (pixel_ref64_cases.LF_SD_MUL)
ARGS = PC.LF_ARGS


def grid_groups(cells, smooth):
    """the LF groups of a cells[0] x cells[1] grid over integers of +-2000, in reverse order (the entry sorts them by position)"""
    q = np.random.default_rng(cells[0] * 1000 + cells[1]).integers(-2000, 2000, size=(3,) + tuple(cells)).astype(np.int32)
    rows, cols = -(-cells[0] // 256), -(-cells[1] // 256)
    groups = []
    for p in range(rows * cols):
        y, x = p // cols * 256, p % cols * 256
        groups.append(dict(lfg_y=p // cols, lfg_x=p % cols, lf_quant=[np.ascontiguousarray(q[c, y:y + 256, x:x + 256]) for c in range(3)],
                           extra_precision=0, scaled_dequant=SD, x_factor_lf=ARGS["x_factor_lf"], b_factor_lf=ARGS["b_factor_lf"],
                           adaptive_smoothing=smooth))
    return groups[::-1]


def xyb_params():
    p = C.params_of(C.source("one_dct8"))
    return (p.opsin_matrix, p.opsin_bias, p.cbrt_opsin_bias, float(p.intensity_target))


_want = {}


def want(orc, cells, smooth, xyb):
    """the oracle composition, made once per case and shared"""
    key = (cells, smooth, xyb)
    if key not in _want:
        pre = L.compose(orc, grid_groups(cells, smooth), cells, ARGS["base_corr_x"], ARGS["base_corr_b"], ARGS["color_factor"])
        if xyb:
            m, bias, cbrt, it = xyb_params()
            pre = orc.xyb(pre, list(m), list(bias), list(cbrt), it)
        pre.setflags(write=False)
        _want[key] = pre
    return _want[key]


def run(ctx, cells, smooth, xyb, keep=False):
    return host.lfImage(ctx, grid_groups(cells, smooth), cells, ARGS["base_corr_x"], ARGS["base_corr_b"], ARGS["color_factor"],
                        xyb=xyb_params() if xyb else None, keep=keep)


@pytest.mark.parametrize("cells", GRIDS)
def test_every_group_with_an_interior_has_all_smoothing_regimes(cells):
    """tests/test_lf_stage.py's assert_all_smoothing_regimes per LF group: the gap of an interior of >= 50 cells lies in each regime
    for at least a tenth of the cells"""
    seen = 0
    for g in grid_groups(cells, True):
        gap = P.lf_stage(np.stack(g["lf_quant"]), SD, 0, smooth=True, **ARGS)[2]
        if gap is not None and gap.size >= PC.LF_MIN_INTERIOR:
            assert min(P.lf_regimes(gap)) >= PC.LF_MIN_SHARE, (cells, g["lfg_y"], g["lfg_x"], P.lf_regimes(gap))
            seen += 1
    assert seen == {(33, 47): 1, (33, 288): 2, (260, 300): 4}.get(cells, 0)  # (the fourth group of 260 x 300 is 4 x 44 cells: 84 inside)


@pytest.mark.parametrize("xyb", (False, True))
@pytest.mark.parametrize("smooth", (True, False))
@pytest.mark.parametrize("cells", GRIDS)
def test_stage_lf_image_is_the_oracle_composition(ctx, orc, cells, smooth, xyb):
    got = run(ctx, cells, smooth, xyb)
    assert_bits_equal(got, want(orc, cells, smooth, xyb), "lf image %s smooth=%d xyb=%d" % (cells, smooth, xyb))


def test_seam_columns_are_copies(ctx, orc):
    """(33, 288): columns 255 and 256 border their LF groups, so they carry the unsmoothed samples; the columns beside them do not"""
    cells = (33, 288)
    a, b = run(ctx, cells, True, False), run(ctx, cells, False, False)
    assert_bits_equal(a[:, :, 255:257], b[:, :, 255:257], "seam columns")
    assert (a[:, 1:-1, 254].view(np.uint32) != b[:, 1:-1, 254].view(np.uint32)).any() and (a[:, 1:-1, 257].view(np.uint32) != b[:, 1:-1, 257].view(np.uint32)).any()
    # (257, 2): the one-row group below is copied whole
    a, b = run(ctx, (257, 2), True, False), run(ctx, (257, 2), False, False)
    assert_bits_equal(a[:, 255:, :], b[:, 255:, :], "seam rows")


@pytest.mark.parametrize("cells,smooth,xyb", [((1, 1), True, True), ((33, 288), True, True), ((257, 2), False, False), ((260, 300), True, False)])
def test_the_two_entries_agree(ctx, orc, cells, smooth, xyb):
    rp = run(ctx, cells, smooth, xyb, keep=True)
    assert rp.shape == cells
    assert_bits_equal(rp.download(), want(orc, cells, smooth, xyb), "jxl_planes_from_lf %s" % (cells,))


def test_the_entries_refuse_what_the_validator_refuses(ctx):
    groups = grid_groups((33, 288), True)
    for bad, cells, kw in ((groups[:1], (33, 288), {}), (groups, (33, 287), {}), (groups, (33, 288), dict(colorFactor=0))):
        for keep in (False, True):
            with pytest.raises(_lib.JxlError) as e:
                host.lfImage(ctx, bad, cells, keep=keep, **kw)
            assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT and "lf image" in str(e.value)


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------
NAMES = ("lenna", "bbb", "bench", "white", "two_lf_groups_2056x16", "rgb", "noise_40x40", "ycbcr_444", "opsin_custom")


@pytest.fixture(scope="module")
def backend():
    b = DeviceBackend(0)
    yield b
    b.close()


def data_of(name):
    return L.encoded(name) if name in C.CASES else L.sample(name)


_cpu = {}


def cpu_image(orc, name):
    """the decode on the oracle backend (pinned by tests/test_lf_preview_cpu.py), once per name"""
    if name not in _cpu:
        dec, _, im = L.preview(data_of(name), orc)
        _cpu[name] = ([np.array(p, copy=True) for p in im.getBuffer(copy=False)], dec.stats[-1]["preview"])
    return _cpu[name]


@pytest.mark.parametrize("device_output", (False, True))
@pytest.mark.parametrize("name", NAMES)
def test_device_decode_equals_the_cpu_decode(backend, orc, name, device_output):
    exp, note = cpu_image(orc, name)
    dec = JXLDecoder(data_of(name), backend=backend, downsample=8, device_output=device_output)
    im = dec.decode()
    st = dec.stats[-1]
    assert note == "lf image (1:8)" + (", noise left out" if name == "noise_40x40" else "")
    assert st["preview"] == note and st["output"] == ("device" if device_output else "host")
    assert im.onDevice() == device_output and (im.getHeight(), im.getWidth()) == exp[0].shape
    assert_bits_equal(np.stack(im.getBuffer(copy=False)), np.stack(exp), name)
    assert dec.decode() is None


@pytest.mark.parametrize("name", ("bbb", "bench"))
def test_the_resident_preview_feeds_the_tensor_and_png_exits(backend, orc, name):
    exp, _ = cpu_image(orc, name)
    dec = JXLDecoder(data_of(name), backend=backend, downsample=8, device_output=True)
    im = dec.decode()
    assert im._home(3) == "resident"
    t = im.toTensor(size=(32, 32))
    assert im.tensor_bus_bytes == (0, 0) and t.shape == (3, 32, 32) and t.is_cuda
    out = io.BytesIO()
    w = PNGWriter(im, deviceSamples=True)
    w.write(out)
    assert im._buffer[0] is None, "a writer brought the planes down"
    # the same planes as host arrays
    host_im = JXLImage([np.ascontiguousarray(p) for p in exp], dec.info, backend)
    t2 = host_im.toTensor(size=(32, 32))
    assert host_im.tensor_bus_bytes == (3 * exp[0].nbytes, 0)
    assert torch.equal(t, t2)
    out2 = io.BytesIO()
    PNGWriter(host_im, deviceSamples=True).write(out2)
    assert out.getvalue() == out2.getvalue()
    if name == "bbb":
        assert out.getvalue()[16:24] == (160).to_bytes(4, "big") + (90).to_bytes(4, "big")


def test_a_refused_frame_raises_on_the_device_backend_too(backend):
    from jxlatte_amd.decoder import UnsupportedOperationException
    with pytest.raises(UnsupportedOperationException) as e:
        JXLDecoder(L.sample("patches-lossless"), backend=backend, downsample=8).decode()
    assert str(e.value) == "downsample=8: the image has extra channels"


@pytest.mark.parametrize("name", sorted(L.WRITER_RULE))
def test_a_refused_writer_case_raises_on_the_device_backend_too(backend, name):
    from jxlatte_amd.decoder import UnsupportedOperationException
    with pytest.raises(UnsupportedOperationException) as e:
        JXLDecoder(L.encoded(name), backend=backend, downsample=8).decode()
    assert str(e.value) == "downsample=8: " + L.WRITER_RULE[name]
