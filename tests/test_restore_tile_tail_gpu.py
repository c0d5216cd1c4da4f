"""The ragged last patch column of the fused restoration kernel's float sink (restore_fused_body.h, OutSink::row4): the output tile
is 62 = 15 x 4 + 2 pixels wide, so the patch of column 15 stores two pixels, not four. (A two-pixel wide store for it was measured
and dropped, profiles/experiments/restore_sink_store2.diff; these tests hold whichever form the sink has.)

Frame-path decodes (pooled, cell-tiled planes, float planes out) at 264 x 112 (5 x 4 tiles, ragged last tiles), 200 x 72 (4 x 3) and
136 x 72 (3 x 3, one interior tile), against the oracle bit for bit. After each run the two columns past every tile's 62nd -- the
neighbour tile's first two, which a tail store that is one pixel off would overwrite -- and the tile's own last two are compared on
their own, so that a failure names the place.
"""
import numpy as np
import pytest

import restore_variants as rv
import switch_cases as sc
from conftest import assert_bits_equal
from jxlatte_amd import host, synth

pytestmark = pytest.mark.gpu

SIZES = [(264, 112), (200, 72), (136, 72)]
TILED_BIT = 128


@pytest.fixture(scope="module")
def ctxs():
    c = rv.Contexts()
    yield c
    c.close()


_frames = {}


def _frame(size, iters, gab):
    if size not in _frames:
        _frames[size] = (rv.base_frame(size) if size in rv.SEEDS else
                         synth.make_vardct_frame(size[0], size[1], seed=815, mix="default", aligned=False))
    return sc.with_params(_frames[size], 15, gab=gab, epf_iters=iters)


@pytest.mark.parametrize("gab", [1, 0])
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_tile_tails(ctxs, orc, size, iters, gab):
    w, h = size
    f = _frame(size, iters, gab)
    cx = ctxs.pooled[0]
    fr = host.Frame.from_synth(cx, f)
    fr.run()
    got = fr.readOutput()
    ran = host.lastRestoreLaunches(cx)
    assert ran == [rv.code("SK_PLAIN", gab, iters, tiled=True)] and ran[0] & TILED_BIT, [rv.describe(c) for c in ran]
    exp = orc.vardct_frame(f)
    ow = 62 if iters == 2 else 64  # (one iteration: 64-wide tiles, no ragged column -- the four-pixel branch alone)
    for x0 in range(ow, w, ow):
        assert_bits_equal(got[:, :, x0 - 2:x0], exp[:, :, x0 - 2:x0], "%dx%d it%d gab%d: last two columns of the tile before %d" % (w, h, iters, gab, x0))
        assert_bits_equal(got[:, :, x0:x0 + 2], exp[:, :, x0:x0 + 2], "%dx%d it%d gab%d: the two columns past a tile, at %d" % (w, h, iters, gab, x0))
    assert_bits_equal(got, exp, "%dx%d it%d gab%d" % (w, h, iters, gab))
