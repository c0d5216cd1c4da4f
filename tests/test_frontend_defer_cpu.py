"""CPU-only: the front-end's deferred frame-level transforms (jxf_set_defer_transforms, jxf_get_transform*,
jxf_modular_channel_count, jxf_apply_transforms) on every committed sample, with the oracle behind the hooks: the deferred list is
the one the bitstream codes, the encoded channel list is what the transforms started from, jxf_apply_transforms gives the channels
of a decode that never deferred, and without the switch nothing changes."""
import glob
import os

import numpy as np
import pytest

from jxlatte_amd import frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")
RCT, PALETTE, SQUEEZE = frontend.TRANSFORM_RCT, frontend.TRANSFORM_PALETTE, frontend.TRANSFORM_SQUEEZE
PAL4 = [(PALETTE, None)] * 4
# per sample and frame: the frame-level chain in bitstream order as (kind, rct_type or None)
CHAINS = {
    "art": [[(RCT, 26)]],
    "quilt": [[(SQUEEZE, None)]],
    "blendmodes_5": [[(RCT, 15)]] * 5,
    "wb-rainbow": [[(RCT, 13)], [], [], [(RCT, 13)], []],
    "patches-lossless": [PAL4, PAL4],
    "bench": [[]], "white": [[]], "lenna": [[]], "bbb": [[]],
}
# channel count and first shape of the encoded list, where the frame has Modular channels
ENCODED = {"art": (3, (128, 128)), "quilt": (49, (8, 8)), "blendmodes_5": (4, (1024, 1024)), "wb-rainbow": (4, (576, 1024))}


def test_every_committed_sample_is_in_the_table():
    assert {os.path.basename(f)[:-4] for f in glob.glob(os.path.join(SAMPLES, "*.jxl"))} == set(CHAINS)


def _hooks(orc, calls):
    def squeeze(ins, steps, shapes):
        calls.append("squeeze")
        return orc.modular_apply(ins, steps, rct_type=-1, out_shapes=shapes)

    def rct(a, b, c, rct_type):
        calls.append("rct")
        return orc.rct(np.stack([a, b, c]), rct_type)
    return squeeze, rct, None


def _channels(fe):
    return [fe.modular_channel(i) for i in range(fe.modular_channel_count())]


def _same(a, b):
    return len(a) == len(b) and all(x[1] == y[1] and x[0].shape == y[0].shape and np.array_equal(x[0], y[0]) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_deferred_chain_encoded_channels_and_apply(orc, name):
    data = open(os.path.join(SAMPLES, name + ".jxl"), "rb").read()
    plain, defer = frontend.Frontend(data), frontend.Frontend(data)
    try:
        defer.set_defer_transforms(True)
        for k, chain in enumerate(CHAINS[name]):
            plain_calls, calls = [], []
            a = plain.next_frame(*_hooks(orc, plain_calls))
            b = defer.next_frame(*_hooks(orc, calls))
            assert a is not None and b is not None, k
            assert calls == [], "a hook ran while deferring"
            got = defer.transforms()
            assert [(t["kind"], t["rct_type"] if t["kind"] == RCT else None) for t in got] == chain, (k, got)
            # the list reads the same whether the transforms are pending or done
            assert plain.transforms() == got
            assert all((len(t["steps"]) > 0) == (t["kind"] == SQUEEZE) for t in got)
            assert not plain.transforms_pending()
            assert defer.transforms_pending() == (b.num_modular_channels > 0)
            assert defer.modular_channel_count() == b.num_modular_channels
            if name in ENCODED:
                n, first = ENCODED[name]
                assert defer.modular_channel_count() == n and defer.modular_channel(0)[0].shape == first
            if name == "quilt":
                # 49 encoded channels: the coarsest 8 x 8 averages first; the inverse gives the three 1024 x 1024 planes
                t = got[0]
                assert len(t["steps"]) == 16 and t["begin_c"] == 0
                from jxlatte_amd import synth
                assert [c[0].shape for c in _channels(defer)] == synth.squeezed_shapes([(1024, 1024)] * 3, t["steps"])
                assert [c[0].shape for c in _channels(plain)] == [(1024, 1024)] * 3
            if name == "patches-lossless":
                assert all(t["nb_colors"] > 0 and t["num_c"] >= 1 for t in got)
                assert defer.modular_channel(0)[0].shape[0] == got[-1]["num_c"]  # channel 0 is a meta channel: the last palette
            if chain == []:
                assert _same(_channels(defer), _channels(plain))  # nothing to undo: the lists are equal already
            encoded = _channels(defer)
            defer.apply_transforms(*_hooks(orc, calls))
            assert not defer.transforms_pending()
            assert sorted(calls) == sorted(plain_calls), (calls, plain_calls)
            assert defer.frame.num_modular_channels == a.num_modular_channels == defer.modular_channel_count()
            assert _same(_channels(defer), _channels(plain)), "frame %d: channels differ after jxf_apply_transforms" % k
            if chain:
                assert not _same(encoded, _channels(defer))
            # a second call is a no-op
            done = list(calls)
            defer.apply_transforms(*_hooks(orc, calls))
            assert calls == done and _same(_channels(defer), _channels(plain))
            # and so is one on a frame that never deferred
            plain.apply_transforms(*_hooks(orc, plain_calls))
            assert plain_calls == done
        assert plain.next_frame(*_hooks(orc, [])) is None and defer.next_frame(*_hooks(orc, [])) is None
    finally:
        plain.close()
        defer.close()


def test_switching_back_off_restores_the_default(orc):
    data = open(os.path.join(SAMPLES, "wb-rainbow.jxl"), "rb").read()
    fe, plain = frontend.Frontend(data), frontend.Frontend(data)
    try:
        calls = []
        fe.set_defer_transforms(True)
        fe.next_frame(*_hooks(orc, calls))
        plain.next_frame(*_hooks(orc, []))
        assert calls == [] and fe.transforms_pending()
        fe.set_defer_transforms(False)  # the pending frame stays pending; the next one is decoded as always
        assert fe.transforms_pending()
        for k in range(1, 5):
            fe.next_frame(*_hooks(orc, calls))
            plain.next_frame(*_hooks(orc, []))
            assert not fe.transforms_pending()
            assert _same(_channels(fe), _channels(plain)), k
        assert calls == ["rct"]  # frame 3
    finally:
        fe.close()
        plain.close()


def test_the_dry_walk_refuses_nothing_the_loop_accepts():
    """ModularStream::check_transforms walks the list over shapes only and throws what apply_transforms' loop throws. No committed
    bitstream holds a chain the loop refuses, so what is checked here is the other direction: every sample decodes under the
    switch, without any hook"""
    for name in CHAINS:
        fe = frontend.Frontend(open(os.path.join(SAMPLES, name + ".jxl"), "rb").read())
        try:
            fe.set_defer_transforms(True)
            n = 0
            while fe.next_frame(None, None, None) is not None:
                n += 1
            assert n == len(CHAINS[name])
        finally:
            fe.close()
