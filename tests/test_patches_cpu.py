"""The host half of the device patch stage, on the CPU: the type plan (decoder.patch_type_plan) against the real
JXLDecoder._patches / _blend_buffers, the binned table and the validation of the device-free entry (jxl_patch_bins), and the
order-sensitivity witness the GPU test uses (tests/test_patches_gpu.py)."""
import numpy as np
import pytest

import patch_ref as R
from jxlatte_amd import _lib, abi
from jxlatte_amd.decoder import InvalidBitstreamException, patch_type_plan

F = np.float32
TILE_W, TILE_H = 32, 8


# ---- the type plan ------------------------------------------------------------------------------------------------------------
class Recorder:
    """a backend that performs no arithmetic: blend hands the canvas back and notes, by identity, which planes the call was given
    and the dtypes of ALL planes at that moment"""

    def __init__(self):
        self.calls = []
        self.frame = self.reference = None

    def key_of(self, a):
        for n, b in enumerate(self.frame):
            if a is b:
                return ("f", n)
        for k, lst in enumerate(self.reference):
            for n, b in enumerate(lst or []):
                if a is b:
                    return ("r", k, n)
        return None  # (a plane that is in no list any more: the stale canvas of a channel that is its own alpha)

    def snapshot(self):
        return ([b.dtype for b in self.frame],
                {k: [None if b is None else b.dtype for b in lst] for k, lst in enumerate(self.reference) if lst is not None})

    def blend(self, mode, canvas, frame, ref, rect, frameAlpha=None, refAlpha=None, **kw):
        given = [a for a in (canvas, frame, ref, frameAlpha, refAlpha) if a is not None]
        self.calls.append(dict(pmode=mode, canvas=canvas.dtype, given=[(self.key_of(a), a.dtype) for a in given],
                               frame_alpha=None if frameAlpha is None else frameAlpha.dtype,
                               ref_alpha=None if refAlpha is None else refAlpha.dtype, types=self.snapshot(), rect=tuple(rect), kw=kw))
        return canvas


def _segments_of(rec):
    """segment boundaries derived from the recording alone: a plane handed to an earlier call of the run has changed its type"""
    out, used, first = [], {}, 0
    for k, c in enumerate(rec.calls):
        ft, rt = c["types"]
        # (the canvas of the call is what the frame list will hold after it: _blend_buffers stores the result there)
        cur = lambda key: ft[key[1]] if key[0] == "f" else rt[key[1]][key[2]]  # noqa: E731
        now = {key: dt for key, dt in c["given"] if key is not None}
        if any((c["canvas"] if key == c["d_key"] else cur(key)) != dt for key, dt in used.items()):
            out.append((first, k - 1))
            used, first = {}, k
        used.update(now)
        used[c["d_key"]] = c["canvas"]
    if rec.calls:
        out.append((first, len(rec.calls) - 1))
    return out


def _random_case(seed):
    rng = np.random.default_rng(seed)
    n_extra = int(rng.integers(0, 4))
    info = R.make_info(n_extra, ec_type=[int(rng.integers(0, 2)) * 3 for _ in range(n_extra)], assoc=[int(rng.integers(0, 2)) for _ in range(n_extra)],
                       ec_bits=[int(rng.choice([8, 16])) for _ in range(n_extra)])
    n_chan = 3 + n_extra
    h, w = 12, 20
    colour_dt = rng.choice([np.int32, np.float32])
    frame = [np.zeros((h, w), colour_dt if c < 3 else rng.choice([np.int32, np.float32])) for c in range(n_chan)]
    reference = []
    for k in range(4):
        if rng.random() < 0.25:
            reference.append(None)
            continue
        kind = rng.integers(0, 3)
        rh, rw = (h, w) if rng.random() < 0.5 else (8, 10)
        lst = []
        for c in range(n_chan):
            if c > 0 and rng.random() < 0.2:
                lst.append(None)
            else:
                dt = [np.int32, np.float32, rng.choice([np.int32, np.float32])][kind]
                lst.append(np.zeros((rh, rw), dt))
        reference.append(lst)
    patches = []
    bad = rng.random() < 0.15  # some lists break one of computePatches' rules somewhere
    for i in range(int(rng.integers(1, 5))):
        ref = int(rng.integers(0, 4))
        ph, pw = int(rng.integers(1, 5)), int(rng.integers(1, 6))
        y0, x0 = int(rng.integers(0, 4)), int(rng.integers(0, 5))
        n_pos = int(rng.integers(0, 4))
        positions = [(int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1))) for _ in range(n_pos)]
        if bad and rng.random() < 0.4:
            what = rng.integers(0, 3)
            if what == 0:
                ref = 4 + int(rng.integers(0, 3))
            elif what == 1:
                y0 = 7
            elif positions:
                positions[int(rng.integers(0, len(positions)))] = (h - ph + 1, 0) if rng.random() < 0.5 else (-1, 2)
        simple = rng.random() < 0.4  # the common shape: one mode for every channel
        rows = []
        for _ in positions:
            m = int(rng.integers(0, 8))
            rows.append([[m if simple else int(rng.integers(0, 8)), int(rng.integers(0, max(1, n_extra))), int(rng.integers(0, 2))]
                         for _ in range(1 + n_extra)])
        patches.append(R.patch(ref, y0, x0, ph, pw, positions, rows))
    return info, patches, frame, reference


def _run_host(info, patches, frame, reference):
    rec = Recorder()
    fb = [b.copy() for b in frame]
    ref = [None if r is None else [None if a is None else a.copy() for a in r] for r in reference]
    rec.frame, rec.reference = fb, ref
    dec = R.shell(info, patches, ref, rec)
    # the channel of every call (the recorder cannot see it: the stale canvas of a self-alpha channel is in no list)
    inner, seen = dec._blend_buffers, []

    def spy(idx, *a, **kw):
        n = len(rec.calls)
        inner(idx, *a, **kw)
        # (a below mode off its own pixel goes through backend.blend in pieces, every one with the same planes: one application)
        assert all((c["pmode"], c["given"], c["frame_alpha"], c["ref_alpha"]) == (rec.calls[n]["pmode"], rec.calls[n]["given"],
                   rec.calls[n]["frame_alpha"], rec.calls[n]["ref_alpha"]) for c in rec.calls[n + 1:])
        del rec.calls[n + 1:]
        for c in rec.calls[n:]:
            c["d_key"] = ("f", idx)
        seen.append(idx)
    dec._blend_buffers = spy
    err = None
    try:
        dec._patches(R.frame_rec(patches), fb, 3)
    except Exception as e:  # noqa: BLE001
        err = e
    return rec, fb, ref, err


def test_type_plan_equals_blend_buffers_on_2000_seeded_cases():
    n_cases, n_err, n_multi, n_calls, n_created = 2400, 0, 0, 0, 0
    for seed in range(n_cases):
        info, patches, frame, reference = _random_case(seed)
        rec, fb, ref, err = _run_host(info, patches, frame, reference)
        try:
            plan = patch_type_plan(info, patches, frame, reference, 3)
            perr = None
        except Exception as e:  # noqa: BLE001
            plan, perr = None, e
        if err is not None or perr is not None:
            assert type(err) is type(perr) and str(err) == str(perr), (seed, err, perr)
            n_err += 1
            continue
        # per call: the blend function and the dtypes the backend saw
        assert len(plan.calls) == len(rec.calls), seed
        for pc, rc in zip(plan.calls, rec.calls):
            assert (pc["pmode"], pc["canvas"], pc["frame_alpha"], pc["ref_alpha"]) == (rc["pmode"], rc["canvas"], rc["frame_alpha"], rc["ref_alpha"]), (seed, pc, rc)
            assert rc["d_key"] == ("f", pc["d"])
        # the segments, and the types at their entry: those after their last call
        assert [(s["first"], s["last"]) for s in plan.segments] == _segments_of(rec), seed
        for s in plan.segments:
            used = {}
            for rc in rec.calls[s["first"]:s["last"] + 1]:
                used.update({key: dt for key, dt in rc["given"] if key is not None})
                used[rc["d_key"]] = rc["canvas"]
            for key, dt in used.items():  # every plane the segment uses has ONE type in it, the plan's
                assert (s["frame"][key[1]] if key[0] == "f" else s["ref"][key[1]][key[2]]) == dt, (seed, key)
        # what is left behind
        assert plan.frame_types == [b.dtype for b in fb], seed
        for k, lst in enumerate(ref):
            if k in plan.ref_types:
                assert plan.ref_types[k] == [None if b is None else b.dtype for b in lst], (seed, k)
                for n, b in enumerate(lst):
                    assert ((k, n) in plan.created) == (b is not None and reference[k][n] is None), (seed, k, n)
            else:  # untouched
                assert all((a is None) == (b is None) and (a is None or a.dtype == b.dtype) for a, b in zip(lst or [], reference[k] or []))
        n_multi += len(plan.segments) > 1
        n_calls += len(plan.calls)
        n_created += len(plan.created)
    # the fuzz reaches what it is meant to reach
    assert n_cases >= 2000 and n_err > 50 and n_multi > 50 and n_calls > 5000 and n_created > 100, (n_err, n_multi, n_calls, n_created)


def test_type_plan_on_the_sample_shape():
    """patch mode 2 with an alpha channel: the raw mode equals BLEND_BLEND, so blendBuffers casts the frame plane, the reference
    plane and both alpha planes to float at the first applied position although the function then run is blendAdd -- all casts
    precede the first write: one segment"""
    info = R.make_info(1)
    frame = [np.zeros((16, 16), np.int32) for _ in range(4)]
    ref = [[np.zeros((16, 16), np.int32) for _ in range(4)], None, None, None]
    row = [[2, 0, 0], [0, 0, 0]]
    plan = patch_type_plan(info, [R.patch(0, 0, 0, 4, 4, [(1, 1), (2, 3)], [row, row])], frame, ref, 3)
    assert len(plan.segments) == 1 and len(plan.calls) == 6
    assert plan.frame_types == [np.dtype(F)] * 4 and plan.ref_types[0] == [np.dtype(F)] * 4 and plan.gather


# ---- the binned table ---------------------------------------------------------------------------------------------------------
def _bins(pos, blend, h, w, n_extra=0, ref_shapes=((64, 64), None, None, None), frame_types=None, ref_types=None, is_alpha=None, assoc=None):
    from jxlatte_amd import host
    n_chan = 3 + n_extra
    return host.patch_bins(pos, blend, 3, is_alpha if is_alpha is not None else [True] * n_extra, assoc if assoc is not None else [False] * n_extra,
                           h, w, frame_types if frame_types is not None else [0] * n_chan, list(ref_shapes),
                           ref_types if ref_types is not None else [[0] * n_chan] * 4)


def _pos(rows):
    return np.array(rows, abi.PATCH_POS_DTYPE)


@pytest.mark.parametrize("h,w", [(64, 96), (61, 83), (8, 32), (9, 33), (1, 1), (100, 31)])
def test_bins_list_a_position_exactly_where_the_rectangles_meet(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    rows = []
    sizes = [(1, 1), (1, w), (h, 1), (h, w), (min(h, 8), min(w, 32)), (min(h, 9), min(w, 33)), (min(h, 20), min(w, 70))]
    for ph, pw in sizes + [(int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))) for _ in range(40)]:
        ph, pw = min(ph, 64), min(pw, 64)
        for y0, x0 in [(0, 0), (h - ph, w - pw), (0, w - pw), (h - ph, 0), (int(rng.integers(0, h - ph + 1)), int(rng.integers(0, w - pw + 1)))]:
            rows.append((y0, x0, ph, pw, 0, 0, 0, 0))
    pos = _pos(rows)
    tile, start, lst = _bins(pos, np.array([[[2, 0, 0]] * 3], np.int32), h, w)
    tx_n = (w + TILE_W - 1) // TILE_W
    expect = {}
    for i, r in enumerate(rows):
        for ty in range((h + TILE_H - 1) // TILE_H):
            for tx in range(tx_n):
                if r[0] < (ty + 1) * TILE_H and r[0] + r[2] > ty * TILE_H and r[1] < (tx + 1) * TILE_W and r[1] + r[3] > tx * TILE_W:
                    expect.setdefault(ty * tx_n + tx, []).append(i)  # (appended in stage order)
    assert list(tile) == sorted(expect) and len(start) == len(tile) + 1 and start[0] == 0 and start[-1] == len(lst)
    for n, t in enumerate(tile):
        got = list(lst[start[n]:start[n + 1]])
        assert got and got == expect[int(t)], t


def test_bins_validate_in_stage_order_with_the_reference_messages():
    row = np.array([[[2, 0, 0]] * 3], np.int32)
    ok = (4, 4, 8, 8, 0, 0, 0, 0)
    h, w = 40, 50
    shapes = ((16, 16), None, (40, 50), None)
    # an absent slot is skipped before anything else is looked at: its rectangle may be anything
    tile, start, lst = _bins(_pos([ok, (30, 45, 20, 20, 1, 100, 100, 0), ok]), row, h, w, ref_shapes=shapes)
    assert set(lst) == {0, 2}
    cases = [((0, 0, 8, 8, 4, 0, 0, 0), "Patch out of range"),
             ((0, 0, 8, 8, 0, 9, 0, 0), "Patch too large"), ((0, 0, 8, 8, 0, 0, 9, 0), "Patch too large"),
             ((-1, 0, 8, 8, 0, 0, 0, 0), "Patch size out of bounds"), ((0, -1, 8, 8, 0, 0, 0, 0), "Patch size out of bounds"),
             ((33, 0, 8, 8, 0, 0, 0, 0), "Patch size out of bounds"), ((0, 43, 8, 8, 0, 0, 0, 0), "Patch size out of bounds")]
    for bad, msg in cases:
        for other, omsg in cases:
            if omsg == msg:
                continue
            # the first offence in stage order wins, whatever follows; a skipped position in front does not count
            with pytest.raises(_lib.InvalidBitstreamException) as e:
                _bins(_pos([ok, (0, 0, 99, 99, 3, 0, 0, 0), bad, other, ok]), row, h, w, ref_shapes=shapes)
            assert msg in str(e.value) and omsg not in str(e.value) and e.value.position == 2
    # "too large" comes before "out of bounds" within one position (:227-237)
    with pytest.raises(_lib.InvalidBitstreamException) as e:
        _bins(_pos([(-1, 0, 8, 8, 0, 9, 0, 0)]), row, h, w, ref_shapes=shapes)
    assert "Patch too large" in str(e.value)
    # what one blend call would refuse: a float function on int planes, an illegal mode, planes of two types
    with pytest.raises(_lib.IllegalArgumentException, match="float samples"):
        _bins(_pos([ok]), np.array([[[3, 0, 0]] * 4], np.int32), h, w, n_extra=1, ref_shapes=shapes, frame_types=[1] * 4, ref_types=[[1] * 4] * 4)
    with pytest.raises(_lib.InvalidBitstreamException, match="Illegal blend mode"):
        _bins(_pos([ok]), np.array([[[8, 0, 0]] * 3], np.int32), h, w, ref_shapes=shapes)
    with pytest.raises(_lib.IllegalArgumentException, match="differ in type"):
        _bins(_pos([ok]), row, h, w, ref_shapes=shapes, frame_types=[1, 1, 1])
    # a below mode away from its own pixel is outside the gather
    with pytest.raises(_lib.UnsupportedOperationException):
        _bins(_pos([(4, 4, 8, 8, 2, 0, 0, 0)]), np.array([[[5, 0, 0]] * 3], np.int32), h, w, ref_shapes=shapes)
    _bins(_pos([(4, 4, 8, 8, 2, 4, 4, 0)]), np.array([[[5, 0, 0]] * 3], np.int32), h, w, ref_shapes=shapes)
    # blendMulAdd on the alpha channel reads the slot at the FRAME rectangle
    with pytest.raises(_lib.IllegalArgumentException, match="outside a plane"):
        _bins(_pos([(20, 20, 8, 8, 0, 0, 0, 0)]), np.array([[[0, 0, 0]] * 3 + [[4, 0, 0]]], np.int32), h, w, n_extra=1, ref_shapes=shapes)


def test_plan_and_entry_raise_the_same_three_errors():
    info = R.make_info(0)
    frame = [np.zeros((20, 20), F) for _ in range(3)]
    ref = [[np.zeros((10, 10), F) for _ in range(3)], None, None, None]
    row = [[2, 0, 0]]
    for p, msg in [(R.patch(5, 0, 0, 4, 4, [(0, 0)], [row]), "Patch out of range"), (R.patch(0, 8, 0, 4, 4, [(0, 0)], [row]), "Patch too large"),
                   (R.patch(0, 0, 0, 4, 4, [(17, 0)], [row]), "Patch size out of bounds")]:
        patches = [R.patch(1, 0, 0, 50, 50, [(0, 0)], [row]), R.patch(0, 0, 0, 4, 4, [(1, 1)], [row]), p]
        with pytest.raises(InvalidBitstreamException) as e:
            patch_type_plan(info, patches, frame, ref, 3)
        assert str(e.value) == msg
        err = _run_host(info, patches, frame, ref)[3]
        assert type(err) is InvalidBitstreamException and str(err) == msg
        pos, blend = R.pos_table(info, patches)
        with pytest.raises(_lib.InvalidBitstreamException) as e:
            _bins(pos, blend, 20, 20, ref_shapes=((10, 10), None, None, None))
        assert msg in str(e.value) and e.value.position == 2


# ---- the order witness --------------------------------------------------------------------------------------------------------
def test_order_witness_changes_under_reversal():
    """the input the GPU test replays: on the oracle, applying the two overlapping float ADD positions in the other order changes
    samples -- so a kernel that scatters positions without order cannot pass there"""
    from oracle.pybackend import OracleBackend
    be = OracleBackend()
    info, patches, frame, reference = R.order_witness()
    fwd, _ = R.host_sequence(info, patches, frame, reference, be)
    rev, _ = R.host_sequence(info, patches[::-1], frame, reference, be)
    assert fwd[0][8, 12] == 0.0 and rev[0][8, 12] == 1.0  # (1 + 2^24) - 2^24 against (1 - 2^24) + 2^24
    assert sum(int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))) for a, b in zip(fwd, rev)) >= 3
