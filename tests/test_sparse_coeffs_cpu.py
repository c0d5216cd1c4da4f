"""Sparse coefficient feed, host side (no device): the entry format of include/jxlatte_amd.h round-trips through
host.pack_sparse / unpack_sparse in both forms, and the front-end's sparse lists (jxf_get_coeffs_sparse) describe exactly the
dense planes of jxf_get_coeffs for every (pass, group, channel) of every VarDCT frame of the committed samples."""
import os

import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd import frontend
from jxlatte_amd.host import pack_sparse, unpack_sparse

SAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")
NAMES = ["art", "quilt", "white", "blendmodes_5", "wb-rainbow", "lenna", "bbb", "patches-lossless", "bench"]  # tests/test_decoder.py


def _random_plane(rng, shape, density, lo=-300, hi=300):
    q = rng.integers(lo, hi + 1, shape).astype(np.int32)
    q[q == 0] = 1
    return np.where(rng.random(shape) < density, q, 0).astype(np.int32)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("density", [0.0, 0.15, 1.0])
def test_roundtrip_random_planes(wide, density):
    rng = np.random.default_rng(int(density * 100) + wide)
    q = _random_plane(rng, (256, 256), density)
    e = pack_sparse(q, wide)
    assert e.dtype == np.uint32 and e.ndim == 1 and e.size == np.count_nonzero(q) * (2 if wide else 1)
    assert_bits_equal(unpack_sparse(e, q.shape, wide), q, "density %.2f wide %d" % (density, wide))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("shape", [(256, 256), (8, 264 - 256), (8, 256), (264 - 256, 256)])
def test_roundtrip_group_shapes(wide, shape):
    """a full 256x256 group and the edge groups of an 8x264 / 264x8 frame (its second group is 8 samples wide / high)"""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    q = _random_plane(rng, shape, 0.5)
    q[-1, -1] = -7  # the last sample of the rectangle: the largest position of the group
    assert_bits_equal(unpack_sparse(pack_sparse(q, wide), shape, wide), q, "shape %s" % (shape,))


def test_roundtrip_three_planes_as_a_list():
    rng = np.random.default_rng(3)
    q = [_random_plane(rng, s, 0.15) for s in ((256, 256), (128, 128), (128, 256))]
    back = unpack_sparse(pack_sparse(q), [a.shape for a in q])
    for a, b in zip(back, q):
        assert_bits_equal(a, b)


def test_roundtrip_extreme_values():
    q = np.zeros((16, 16), np.int32)
    q[0, 0], q[3, 5], q[15, 15] = 32767, -32767, -32768
    for wide in (False, True):
        assert_bits_equal(unpack_sparse(pack_sparse(q, wide), q.shape, wide), q)
    e = pack_sparse(q, False)
    assert list(e) == [0x7fff0000, (0x8001 << 16) | (3 << 8) | 5, (0x8000 << 16) | (15 << 8) | 15]
    q[7, 9] = 70000
    q[8, 1] = -(2 ** 31)
    e = pack_sparse(q, True)
    assert_bits_equal(unpack_sparse(e, q.shape, True), q)
    assert e[0] == 0 and e[1] == 32767 and (7 << 8 | 9) in list(e[0::2])


def test_narrow_form_refuses_values_outside_int16():
    q = np.zeros((8, 8), np.int32)
    for v in (32768, -32769, 70000):
        q[2, 2] = v
        with pytest.raises(ValueError):
            pack_sparse(q, wide=False)
        assert unpack_sparse(pack_sparse(q, wide=True), q.shape, True)[2, 2] == v


def test_unpack_refuses_positions_outside_the_plane_and_sums_duplicates():
    with pytest.raises(ValueError):
        unpack_sparse(np.array([5 << 16 | 0 << 8 | 8], np.uint32), (8, 8))
    with pytest.raises(ValueError):
        unpack_sparse(np.array([1 << 16, 5], np.uint32), (8, 8), wide=True)  # bits above the low 16 of a wide position
    e = np.array([3 << 16 | 1 << 8 | 2, 4 << 16 | 1 << 8 | 2, 0 << 16 | 7 << 8 | 7], np.uint32)
    out = unpack_sparse(e, (8, 8))
    assert out[1, 2] == 7 and np.count_nonzero(out) == 1


@pytest.mark.parametrize("name", NAMES)
def test_frontend_sparse_lists_equal_the_dense_planes(orc, name):
    fe = frontend.Frontend(open(os.path.join(SAMPLES, name + ".jxl"), "rb").read())
    sq = lambda ins, steps, shapes: orc.modular_apply(ins, steps, rct_type=-1, out_shapes=shapes)  # noqa: E731
    rct = lambda a, b, c, t: orc.rct(np.stack([a, b, c]), t)  # noqa: E731
    checked = 0
    while True:
        fr = fe.next_frame(sq, rct)
        if fr is None:
            break
        if fr.encoding != 0:  # not VarDCT: no HF coefficients
            continue
        for pass_ in range(fr.num_passes):
            for grp in range(fr.num_groups):
                dense = fe.coeffs(pass_, grp)
                for c, (entries, wide, shape) in enumerate(fe.coeffs_sparse(pass_, grp)):
                    what = "%s pass %d group %d channel %d" % (name, pass_, grp, c)
                    assert shape == dense[c].shape, what
                    vals = entries[1::2] if wide else entries >> 16
                    assert np.all(vals != 0), what + ": an entry with value 0"
                    assert entries.size == np.count_nonzero(dense[c]) * (2 if wide else 1), what
                    assert wide == bool(dense[c].size and (dense[c].min() < -32768 or dense[c].max() > 32767)), what
                    assert_bits_equal(unpack_sparse(entries, shape, wide), dense[c], what)
                    checked += 1
    fe.close()
    vardct = {"white", "lenna", "bbb", "bench"}  # first-frame encoding 0 in tests/test_decoder.py's EXPECT_HEADERS
    assert (checked > 0) == (name in vardct), (name, checked)
