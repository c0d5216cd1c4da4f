"""The inverse walk over a frame-level transform chain as the reference does it: a scalar restatement of
ModularStream.applyTransforms (ModularStream.java:224-380) -- the order, and the surgery on the channel list -- written from the
reference and independent of jxlatte_amd/csrc/modchain_check.h and of the front-end's loop. The transforms themselves are the
models the project already has: palette_ref.inverse_palette (:337-372) and the exact integer RCT and inverse Squeeze of
pixel_ref64 (:229-326). It is the model jxl_modular_begin_chain, the stand-alone host program and the front-end are held against.

A transform is a dictionary as frontend.transforms() returns them: kind, begin_c, num_c, rct_type, nb_colors, nb_deltas, d_pred
and, for a Squeeze, steps: the expanded (horizontal, in_place, begin_c, num_c) list.

MUTATIONS names the wrong variants of the walk; tests/test_modchain_cpu.py asserts that each differs from the model on at least
one case of tests/modchain_cases.py."""
import numpy as np

import palette_ref
import pixel_ref64

RCT, PALETTE, SQUEEZE = 0, 1, 2  # the front-end's numbering (jxlatte_amd/frontend.py TRANSFORM_*)

MUTATIONS = (
    "bitstream_order",        # the transforms undone first to last
    "channel0_kept",          # the palette channel stays in the list
    "palette_of_wrong_stage", # row c comes from the palette of the Palette undone before this one
    "begin_c_of_final_list",  # begin_c counted in the list without the meta channels still in front of it
    "deltas_ignored",         # no delta pixel gets its prediction
    "negative_not_delta",     # with nb_deltas 0 a negative index is no delta pixel
)


def apply_chain(chans, transforms, bit_depth, mut=None, palette_fn=None, chained=None):
    """chans: the encoded channel list (2-D int32 arrays, meta channels included); returns the list after the inverse walk.
    palette_fn: a stand-in for palette_ref.inverse_palette with its signature (a cache of its answers).
    chained: a list that receives, per Palette in the order undone, whether a pixel of it needed a neighbour (a delta pixel --
    index < nb_deltas, every negative index -- under a predictor other than 0 and 6)"""
    ch = [np.asarray(c, np.int32) for c in chans]
    inverse_palette = palette_fn or palette_ref.inverse_palette
    order = list(transforms) if mut == "bitstream_order" else list(reversed(transforms))  # :228
    last_palette = None
    for pos, t in enumerate(order):
        # the meta channels of the Palettes not undone yet, this one's apart, stand in front of what the final list keeps
        metas_ahead = sum(1 for u in order[pos + 1:] if u["kind"] == PALETTE)
        shift = -metas_ahead if mut == "begin_c_of_final_list" else 0
        if t["kind"] == SQUEEZE:                                                           # :229-254
            for horizontal, in_place, begin, count in reversed(list(t["steps"])):
                end = begin + count - 1
                offset = end + 1 if in_place else len(ch) + begin - end - 1                # :235
                for c in range(begin, end + 1):
                    fn = pixel_ref64.inv_hsqueeze if horizontal else pixel_ref64.inv_vsqueeze
                    ch[c] = fn(ch[c], ch[offset + c - begin])
                del ch[offset:offset + count]                                              # :252-253
        elif t["kind"] == RCT:                                                             # :255-326
            b = t["begin_c"] + shift
            assert b >= 0 and b + 3 <= len(ch)
            ch[b:b + 3] = pixel_ref64.rct_channels(ch[b:b + 3], t["rct_type"])
        elif t["kind"] == PALETTE:                                                         # :327-378
            first = t["begin_c"] + 1 + shift                                               # :328
            assert 1 <= first < len(ch)
            c0, index = ch[0], ch[first]                                                   # :332-333
            nb_deltas, d_pred = t["nb_deltas"], t["d_pred"]
            if chained is not None:
                chained.append(d_pred not in (0, 6) and bool((index < nb_deltas).any()))
            if mut == "deltas_ignored" or (mut == "negative_not_delta" and nb_deltas == 0):
                d_pred = 0  # (the prediction of predictor 0 is 0)
            if mut == "palette_of_wrong_stage" and last_palette is not None:
                c0 = np.resize(last_palette, c0.shape)
            last_palette = ch[0]
            planes = inverse_palette(index, c0, t["num_c"], t["nb_colors"], nb_deltas, d_pred, bit_depth)
            ch[first:first + 1] = [np.ascontiguousarray(p) for p in planes]               # :334-336: num_c - 1 copies behind it
            if mut != "channel0_kept":
                del ch[0]                                                                  # :373
        else:
            raise ValueError("transform kind %r" % (t["kind"],))
    return ch


def same(a, b):
    """two channel lists, bit for bit"""
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
