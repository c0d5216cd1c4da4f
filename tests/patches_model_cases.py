"""The shared cases of tests/test_patches_model_cpu.py and tests/test_patches_model_gpu.py: patch lists, frames and reference
slots as plain numpy data. Nothing of the project is imported; the lists are dicts in the layout Frontend.patch hands over
(ref, y0, x0, h, w, positions [n][2], blend [n][1 + num_extra][3]).

The generator is constructive: it knows which raw modes the reference can run on which plane types (blendBuffers' casts, :433-465,
decide that) and draws only from those, so tests/patches_model.py answers every list either with a result or -- the `refuse`
cases -- with an InvalidBitstreamException; never with a type clash, a null plane or an index outside a plane.

Geometry: frames of 37 x 75 and 9 x 33; k_patches works on tiles of 32 x 8, so position edges are put at x = 31, 32, 33 and
y = 7, 8, 9; 1 x 1 patches; patches flush with the four frame edges; 2 to 4 overlapping positions. Slots: 0 smaller than the frame,
1 of the frame's size, 2 absent, 3 of the frame's size with absent planes.

Values (float cases): alpha 0, 1, above 1, negative, NaN, +-inf; samples NaN, +-inf, -0.0; the model is compared as one NaN class."""
import types

import numpy as np

F = np.float32
CE_RGB, CE_GRAY = 0, 1
BIG, SMALL = (37, 75), (9, 33)
SLOT0 = {BIG: (23, 41), SMALL: (7, 20)}
EDGE_X, EDGE_Y = (31, 32, 33), (7, 8, 9)
SPECIAL_ALPHA = np.array([0.0, 1.0, 1.5, -0.25, np.nan, np.inf, -np.inf], F)
SPECIAL_SAMPLE = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.5], F)


def make_info(colors, n_extra, ec_type=None, assoc=None, bits=8, ec_bits=None, dim_shift=None):
    return types.SimpleNamespace(colour_space=CE_GRAY if colors == 1 else CE_RGB, num_extra=n_extra,
                                 ec_type=list(ec_type) if ec_type is not None else [0] * n_extra,
                                 ec_alpha_associated=list(assoc) if assoc is not None else [0] * n_extra, bits_per_sample=bits,
                                 ec_bits=list(ec_bits) if ec_bits is not None else [8] * n_extra,
                                 ec_dim_shift=list(dim_shift) if dim_shift is not None else [0] * n_extra)


def make_hdr(upsampling=1, ec_upsampling=()):
    return types.SimpleNamespace(upsampling=upsampling, ec_upsampling=list(ec_upsampling))


def patch(ref, y0, x0, h, w, positions, rows):
    """rows: per position 1 + n_extra (mode, alphaChannel, clamp) triples"""
    n = len(positions)
    return dict(ref=ref, y0=y0, x0=x0, h=h, w=w, positions=np.asarray(positions, np.int32).reshape(-1, 2),
                blend=np.asarray(rows, np.int32).reshape(n, -1, 3))


class Case:
    def __init__(self, name, colors, info, patches, frame, reference, hdr=None, refuse=None, tags=()):
        self.name, self.colors, self.info, self.patches, self.frame, self.reference = name, colors, info, patches, frame, reference
        self.hdr, self.refuse, self.tags = hdr, refuse, set(tags)
        self.n_chan = colors + info.num_extra

    def __repr__(self):
        return self.name


def _plane(rng, shape, kind, alpha, specials):
    if kind == "int":
        return rng.integers(-300, 300, shape).astype(np.int32)
    a = (rng.uniform(0.05, 0.95, shape) if alpha else rng.uniform(-0.5, 1.5, shape)).astype(F)
    if specials:
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, max(3, flat.size // 12), replace=False)
        vals = SPECIAL_ALPHA if alpha else SPECIAL_SAMPLE
        flat[idx] = vals[rng.integers(0, len(vals), idx.size)]
    return a


def _allowed(kind, n_extra, slot, is_alpha_type):
    """the raw modes (besides 0) the reference can run on a channel of such a case, whatever was cast before"""
    if n_extra == 0:
        return [2, 3, 4, 5, 6, 7]  # every function is blendAdd, and a type mismatch is cast away (:461)
    if kind == "float":
        # slot 3 has absent planes: raw 3 and 5 read the slot's alpha plane, which nothing creates for them (:446-456)
        return [2, 4, 6, 7] if slot == 3 else [2, 3, 4, 5, 6, 7]
    # int or mixed planes: raw 2 casts all it touches; blendMulAdd on the alpha channel itself is a copy of whole samples
    return [2, 6, 7] if is_alpha_type else [2]


def random_case(seed):
    rng = np.random.default_rng(seed)
    shape = BIG if seed % 3 else SMALL
    h, w = shape
    colors = 1 if seed % 5 == 0 else 3
    n_extra = seed % 3
    kind = ("float", "float", "int", "mixed")[(seed // 3) % 4]
    ec_type = [0 if rng.random() < 0.6 else 3 for _ in range(n_extra)]
    if n_extra == 2 and seed % 2:
        ec_type = [0, 3] if seed % 4 == 1 else [3, 0]
    info = make_info(colors, n_extra, ec_type=ec_type, assoc=[int(rng.integers(0, 2)) for _ in range(n_extra)],
                     ec_bits=[int(rng.choice([8, 12, 16])) for _ in range(n_extra)])
    n_chan = colors + n_extra

    def planes(sz, present=None):
        out = []
        for c in range(n_chan):
            k = kind if kind != "mixed" else ("int" if rng.random() < 0.5 else "float")
            out.append(None if present is not None and not present[c] else _plane(rng, sz, k, c >= colors, kind == "float" and seed % 2 == 0))
        return out
    frame = planes(shape)
    holes = [not (c == min(1, n_chan - 1) or c == n_chan - 1) or c == 0 for c in range(n_chan)]
    reference = [planes(SLOT0[shape]), planes(shape), None, planes(shape, holes)]
    sizes = [(1, 1), (3, 5), (h, w), (2, 33), (8, 32), (9, 31), (7, 33), (5, w), (h, 3)]
    patches, tags = [], {kind, "colors%d" % colors, "extra%d" % n_extra, "frame%dx%d" % shape}
    for _ in range(int(rng.integers(3, 7))):
        slot = int(rng.choice([0, 0, 1, 1, 2, 3]))
        row = []
        for c in range(1 + n_extra):
            allowed = _allowed(kind, n_extra, slot, c > 0 and ec_type[c - 1] == 0)
            mode = 0 if rng.random() < 0.15 else int(rng.choice(allowed))
            row.append([mode, int(rng.integers(0, max(1, n_extra))), int(rng.integers(0, 2))])
        modes = [m for m, _, _ in row]
        below = any(m in (5, 7) for m in modes)
        # a below mode reads the slot at the position and the frame at the patch's origin; blendMulAdd's alpha copy reads the slot
        # at the position: both want a slot that covers the frame
        wide = below or any(m in (4, 6) for m in modes[1:])
        if wide and slot == 0:
            slot = 1
        rh, rw = SLOT0[shape] if slot == 0 else shape
        ph, pw = sizes[int(rng.integers(0, len(sizes)))] if rng.random() < 0.6 else (int(rng.integers(1, 12)), int(rng.integers(1, 36)))
        ph, pw = min(ph, rh, h), min(pw, rw, w)
        y0, x0 = int(rng.integers(0, rh - ph + 1)), int(rng.integers(0, rw - pw + 1))
        if below:
            positions = [(y0, x0)]  # on its own pixel (the off-pixel ones are the `below_off` cases)
            tags.add("below_own")
        else:
            positions = []
            for _ in range(int(rng.integers(1, 5))):
                r = rng.random()
                if r < 0.25:
                    positions.append([(0, 0), (h - ph, w - pw), (0, w - pw), (h - ph, 0)][int(rng.integers(0, 4))])
                    tags.add("flush")
                elif r < 0.6:  # an edge of the rectangle on a tile edge or next to it
                    ex, ey = int(rng.choice(EDGE_X)), int(rng.choice(EDGE_Y))
                    py = ey if ey + ph <= h else max(0, min(h - ph, ey - ph))
                    px = ex if ex + pw <= w else max(0, min(w - pw, ex - pw))
                    positions.append((py, px))
                    tags.add("tile_edge")
                else:
                    positions.append((int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1))))
            if len(positions) > 1 and rng.random() < 0.5:  # overlapping copies of the first one, one pixel apart
                py, px = positions[0]
                positions = [(min(py + k, h - ph), min(px + k, w - pw)) for k in range(len(positions))]
                tags.add("overlap%d" % len(positions))
        if (ph, pw) == (1, 1):
            tags.add("1x1")
        if slot == 2:
            tags.add("absent_slot")
        if slot == 3:
            tags.add("absent_planes")
        if slot == 0:
            tags.add("small_slot")
        patches.append(patch(slot, y0, x0, ph, pw, positions, [row] * len(positions)))
    return Case("random-%d" % seed, colors, info, patches, frame, reference, tags=tags)


def _floats(rng, shape, n_chan, colors, specials=False):
    return [_plane(rng, shape, "float", c >= colors, specials) for c in range(n_chan)]


def below_off_case(mode, n_extra, shape, seed):
    """mode 5 or 7 away from its own pixel, the rectangle at patch.bounds.origin overlapping the rectangle at the position: the
    frame plane is `ref` AND the canvas, and later pixels read what earlier ones stored. Shifts in all four directions."""
    rng = np.random.default_rng(seed)
    h, w = shape
    colors = 3
    info = make_info(colors, n_extra, ec_type=[0, 3][:n_extra], assoc=[seed % 2, 0][:n_extra])
    n_chan = colors + n_extra
    frame = _floats(rng, shape, n_chan, colors)
    reference = [None, _floats(rng, shape, n_chan, colors), None, None]
    row = [[mode, 0, seed % 2]] + [[mode if e == 1 or seed % 2 else 0, 0, 1] for e in range(n_extra)]
    patches = []
    for (oy, ox), (py, px) in (((2, 3), (3, 5)), ((3, 5), (2, 3)), ((1, 20), (1, 18)), ((4, 9), (2, 9)), ((0, 26), (3, 25))):
        patches.append(patch(1, oy, ox, 4, 6, [(py, px)], [row]))
    return Case("below-off-%d-extra%d-%dx%d" % (mode, n_extra, h, w), colors, info, patches, frame, reference,
                tags={"below_off%d" % mode, "float", "colors3", "extra%d" % n_extra, "frame%dx%d" % shape})


def order_witness():
    """1 + 2^24 - 2^24: two overlapping float ADD positions whose result depends on their order"""
    info = make_info(3, 0)
    frame = [np.full(BIG, 1.0, F) for _ in range(3)]
    ref = [np.zeros((16, 32), F) for _ in range(3)]
    for c in range(3):
        ref[c][0:4, 0:8] = F(2.0 ** 24)
        ref[c][8:12, 0:8] = F(-(2.0 ** 24))
    row = [[2, 0, 0]]
    patches = [patch(0, 0, 0, 4, 8, [(5, 29)], [row]), patch(0, 8, 0, 4, 8, [(6, 31)], [row])]
    return Case("order-witness", 3, info, patches, frame, [ref, None, None, None], tags={"order_witness", "float", "colors3", "extra0"})


def zero_alpha_case(shape):
    """blendBlend, unassociated, with both alphas 0: 0 / 0, above (raw 3) and below (raw 5), next to alphas of every special value"""
    rng = np.random.default_rng(77)
    info = make_info(3, 1, ec_type=[0], assoc=[0])
    frame, ref = _floats(rng, shape, 4, 3, True), _floats(rng, shape, 4, 3, True)
    frame[3][0:4, 0:6] = 0
    ref[3][0:4, 0:6] = 0
    frame[3][4:8, 0:7] = SPECIAL_ALPHA
    patches = [patch(1, 0, 0, 8, 8, [(0, 0)], [[[3, 0, 0], [0, 0, 0]]]), patch(1, 0, 0, 8, 8, [(0, 0)], [[[5, 0, 1], [0, 0, 0]]]),
               patch(1, 0, 0, 6, 6, [(0, 0)], [[[0, 0, 0], [3, 0, 0]]])]
    return Case("zero-alpha-%dx%d" % shape, 3, info, patches, frame, [None, ref, None, None],
                tags={"zero_over_zero", "float", "colors3", "extra1", "below_own", "frame%dx%d" % shape})


def segment_cases():
    """lists in which a plane is used with one type and cast later: more than one launch with the reference's cast in between"""
    out = []
    for seed in range(12):
        rng = np.random.default_rng(900 + seed)
        shape = BIG if seed % 2 else SMALL
        h, w = shape
        n_extra = (0, 1, 2)[seed % 3]
        colors = 3
        info = make_info(colors, n_extra, ec_type=[0, 3][:n_extra], assoc=[seed % 2, 1][:n_extra], ec_bits=[8, 12][:n_extra])
        n_chan = colors + n_extra
        frame = [_plane(rng, shape, "int", c >= colors, False) for c in range(n_chan)]
        ref = [_plane(rng, shape, "int", c >= colors, False) for c in range(n_chan)]
        ph, pw = (5, 9) if shape == SMALL else (9, 34)
        if n_extra == 0:  # int sums, then raw 4 (== BLEND_MULT: everything cast) on the same planes
            first, second = [[2, 0, 0]], [[4, 0, 0]]
        else:  # the alpha channel copied as ints (blendMulAdd's alpha case), then raw 2 with an alpha channel: everything cast
            first = [[0, 0, 0], [6, 0, 0]] + [[0, 0, 0]] * (n_extra - 1)
            second = [[2, 0, seed % 2]] * (1 + n_extra)
        patches = [patch(0, 1, 2, ph, pw, [(0, 0), (2, 1)], [first] * 2), patch(0, 0, 0, ph, pw, [(1, 1), (h - ph, w - pw)], [second] * 2),
                   patch(0, 1, 1, 3, 3, [(2, 2)], [second])]
        out.append(Case("segments-%d" % seed, colors, info, patches, frame, [ref, None, None, None],
                        tags={"segments", "int", "colors3", "extra%d" % n_extra, "frame%dx%d" % shape}))
    return out


def refusal_cases():
    """lists the reference answers with an InvalidBitstreamException, each behind applications that ran (their stores stay)"""
    out = []
    rng = np.random.default_rng(5)

    def base(n_extra, ec_type=None, kind="float"):
        info = make_info(3, n_extra, ec_type=ec_type)
        frame = [_plane(rng, BIG, kind, c >= 3, False) for c in range(3 + n_extra)]
        ref0 = [_plane(rng, SLOT0[BIG], kind, c >= 3, False) for c in range(3 + n_extra)]
        ref1 = [_plane(rng, BIG, kind, c >= 3, False) for c in range(3 + n_extra)]
        return info, frame, [ref0, ref1, None, None]
    add = [2, 0, 0]
    ok1 = patch(0, 0, 0, 4, 6, [(1, 2), (30, 60)], [[add]] * 2)
    # patch mode 1: raw 1 -> mode 0, which the switch of :493-512 does not know
    for kind in ("float", "int"):
        info, frame, reference = base(0, kind=kind)
        out.append(Case("mode1-colour-%s" % kind, 3, info, [ok1, patch(0, 1, 1, 3, 3, [(0, 0), (5, 5)], [[[1, 0, 0]]] * 2)], frame, reference,
                        refuse="Illegal blend mode", tags={"mode1"}))
    for c, name in enumerate(("colour", "alpha", "extra")):  # extra channel 0 is the alpha channel, 1 is not one
        for clamp in (0, 1):
            for assoc in (0, 1):
                info, frame, reference = base(2, ec_type=[0, 3], kind="int" if clamp != assoc else "float")
                info.ec_alpha_associated = [assoc, 1 - assoc]
                ok2 = patch(0, 0, 0, 4, 6, [(1, 2)], [[add, add, add]])
                row = [[2, 0, 0], [2, 0, 0], [2, 0, 0]]  # the channels in front of the offending one are applied
                row[c] = [1, 0, clamp]
                out.append(Case("mode1-%s-clamp%d-assoc%d" % (name, clamp, assoc), 3, info, [ok2, patch(1, 1, 1, 3, 3, [(4, 4), (5, 5)], [row] * 2)],
                                frame, reference, refuse="Illegal blend mode", tags={"mode1"}))
    # the size checks, in stage order: an absent slot is skipped before any of them
    info, frame, reference = base(0)
    out.append(Case("absent-slot-out-of-bounds", 3, info, [patch(2, 0, 0, 90, 90, [(-1, -1), (36, 74)], [[add]] * 2), ok1], frame, reference,
                    tags={"absent_slot_bad_positions"}))
    info, frame, reference = base(0)
    out.append(Case("out-of-range", 3, info, [ok1, patch(4, 0, 0, 2, 2, [(0, 0)], [[add]])], frame, reference, refuse="Patch out of range"))
    info, frame, reference = base(0)
    out.append(Case("too-large", 3, info, [ok1, patch(0, 20, 40, 4, 2, [(0, 0)], [[add]])], frame, reference, refuse="Patch too large"))
    info, frame, reference = base(0)
    out.append(Case("too-large-before-bounds", 3, info, [patch(0, 0, 0, 24, 2, [(-1, 0)], [[add]])], frame, reference, refuse="Patch too large"))
    info, frame, reference = base(0)
    out.append(Case("negative-position", 3, info, [ok1, patch(0, 0, 0, 2, 2, [(3, 3), (0, -1)], [[add]] * 2)], frame, reference,
                    refuse="Patch size out of bounds"))
    info, frame, reference = base(0)
    out.append(Case("past-the-frame", 3, info, [ok1, patch(1, 0, 0, 5, 5, [(3, 3), (33, 70), (0, 71)], [[add]] * 3)], frame, reference,
                    refuse="Patch size out of bounds"))
    info, frame, reference = base(0)
    out.append(Case("bounds-before-mode1", 3, info, [patch(0, 0, 0, 2, 2, [(36, 0)], [[[1, 0, 0]]]), patch(4, 0, 0, 2, 2, [(0, 0)], [[add]])],
                    frame, reference, refuse="Patch size out of bounds"))
    # the upsampling check: mode > 3 on an extra channel of an upsampled frame whose ecUpsampling << dimShift is not the frame's
    for name, up, ecu, shift, mode, refuse in (("mismatch", 2, 1, 0, 4, True), ("mode3", 2, 1, 0, 3, False), ("equal", 2, 2, 0, 4, False),
                                               ("dim-shift", 2, 1, 1, 6, False), ("dim-shift-mismatch", 4, 1, 1, 7, True),
                                               ("not-upsampled", 1, 2, 0, 4, False), ("colour-only", 2, 1, 0, 0, False)):
        info, frame, reference = base(1)
        info.ec_dim_shift = [shift]
        rows = [[[4 if name == "colour-only" else 2, 0, 0], [mode, 0, 1]]]
        out.append(Case("upsampling-" + name, 3, info, [patch(1, 2, 2, 4, 6, [(2, 2)], rows)], frame, reference, hdr=make_hdr(up, [ecu]),
                        refuse="Alpha channel upsampling mismatch during patches" if refuse else None, tags={"upsampling"}))
    return out


def created_alpha_case(kind):
    """raw 2 (== BLEND_BLEND) on the colours alone while the slot has no alpha plane: :449-451 make it, float whatever the canvas is,
    and nothing casts it afterwards"""
    rng = np.random.default_rng(31)
    info = make_info(3, 2, ec_type=[3, 0], assoc=[0, 1], ec_bits=[8, 16])
    frame = [_plane(rng, SMALL, kind, c >= 3, False) for c in range(5)]
    ref = [_plane(rng, SMALL, kind, c >= 3, False) if c < 2 else None for c in range(5)]
    row = [[2, 1, 0], [0, 0, 0], [0, 0, 0]]
    return Case("created-alpha-%s" % kind, 3, info, [patch(3, 1, 1, 5, 31, [(0, 0), (4, 2)], [row] * 2)], frame, [None, None, None, ref],
                tags={"absent_planes", kind, "colors3", "extra2", "frame9x33"})


N_RANDOM = 120


def all_cases():
    out = [random_case(seed) for seed in range(1, N_RANDOM + 1)]
    for mode in (5, 7):
        for n_extra in (0, 1, 2):
            out.append(below_off_case(mode, n_extra, BIG if n_extra != 1 else SMALL, 40 + mode + n_extra))
    out.append(order_witness())
    out += [zero_alpha_case(BIG), zero_alpha_case(SMALL)]
    out += segment_cases()
    out += [created_alpha_case("int"), created_alpha_case("float")]
    out += refusal_cases()
    return out


def gpu_cases():
    """the cases with three colours whose planes travel as the device entries take them (every case but the one-colour ones)"""
    return [c for c in all_cases() if c.colors == 3]
