"""Shared by tests/test_patches_cpu.py and tests/test_patches_gpu.py: synthetic patch stages, a JXLDecoder shell that runs the
real JXLDecoder._patches on them, and the yardstick -- today's host sequence (one backend.blend per position and channel) driven
through oracle.pybackend.OracleBackend.blend, the C restatement of JXLCodestreamDecoder.java:285-413."""
import types

import numpy as np

from jxlatte_amd import abi, decoder

F = np.float32


def make_info(n_extra, ec_type=None, assoc=None, bits=8, ec_bits=None, gray=False):
    ec_type = list(ec_type) if ec_type is not None else [0] * n_extra
    assoc = list(assoc) if assoc is not None else [0] * n_extra
    return types.SimpleNamespace(colour_space=decoder.CE_GRAY if gray else decoder.CE_RGB, num_extra=n_extra, ec_type=ec_type,
                                 ec_alpha_associated=assoc, bits_per_sample=bits, ec_bits=list(ec_bits) if ec_bits is not None else [8] * n_extra)


class Fe:
    def __init__(self, patches):
        self.patches = patches

    def patch(self, i):
        return self.patches[i]


def shell(info, patches, reference, backend):
    """a JXLDecoder with just what _patches / _patches_device read"""
    dec = decoder.JXLDecoder.__new__(decoder.JXLDecoder)
    dec.info, dec.fe, dec.reference, dec.backend, dec.stats = info, Fe(patches), reference, backend, [{}]
    return dec


def frame_rec(patches):
    return types.SimpleNamespace(num_patches=len(patches), upsampling=1, ec_upsampling=[])


def patch(ref, y0, x0, h, w, positions, blend, n_entries=1):
    """blend: per position a row of 1 + n_extra (mode, alpha, clamp) triples, as Frontend.patch hands them over"""
    return dict(ref=ref, y0=y0, x0=x0, h=h, w=w, positions=np.asarray(positions, np.int32).reshape(-1, 2),
                blend=np.asarray(blend, np.int32).reshape(len(positions), -1, 3) if len(positions) else np.zeros((0, n_entries, 3), np.int32))


def host_sequence(info, patches, frame, reference, backend, colors=3):
    """today's path on copies: returns (frame planes, reference lists)"""
    fb = [b.copy() for b in frame]
    ref = [None if r is None else [None if a is None else a.copy() for a in r] for r in reference]
    dec = shell(info, patches, ref, backend)
    dec._patches(frame_rec(patches), fb, colors)
    return fb, ref


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def special_floats(rng, shape, lo=-0.5, hi=1.5, specials=True):
    a = rng.uniform(lo, hi, shape).astype(F)
    if specials:
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, max(4, flat.size // 50), replace=False)
        vals = np.array([np.inf, -np.inf, -0.0, 0.0, 1.0, 2.5, -3.0], F)
        flat[idx] = vals[rng.integers(0, len(vals), idx.size)]
    return a


def pos_table(info, patches, colors=3):
    """the stage-order position table and per-channel blend rows of a patch list (what patch_type_plan builds)"""
    pos, rows = [], []
    for p in patches:
        for j in range(p["positions"].shape[0]):
            pos.append((int(p["positions"][j, 0]), int(p["positions"][j, 1]), p["h"], p["w"], p["ref"], p["y0"], p["x0"], len(rows)))
            rows.append(p["blend"][j][[0] * colors + list(range(1, 1 + info.num_extra))])
    return (np.array(pos, abi.PATCH_POS_DTYPE) if pos else np.zeros(0, abi.PATCH_POS_DTYPE),
            np.stack(rows).astype(np.int32) if rows else np.zeros((0, colors + info.num_extra, 3), np.int32))


def order_witness():
    """Two overlapping float ADD positions whose result depends on their order: position A adds 2^24 to a sample of 1.0 (the sum
    rounds to 2^24), position B then adds -2^24 (0.0); the other way round the sample ends as 1.0. Patch mode 2 is blendAdd:
    frame = ref + frame. Returns (info, patches, frame planes, reference)."""
    info = make_info(0)
    h, w = 24, 40
    frame = [np.full((h, w), 1.0, F) for _ in range(3)]
    ref = [np.zeros((16, 32), F) for _ in range(3)]
    for c in range(3):
        ref[c][0:4, 0:8] = F(2.0 ** 24)
        ref[c][8:12, 0:8] = F(-(2.0 ** 24))
    row = [[2, 0, 0]]
    patches = [patch(0, 0, 0, 4, 8, [(5, 9)], [row]), patch(0, 8, 0, 4, 8, [(6, 11)], [row])]
    return info, patches, frame, [ref, None, None, None]
