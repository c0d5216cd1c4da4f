"""GPU: the sparse coefficient feed (jxl_vardct_put_group_sparse / map_sparse / commit_sparse / sparse_rejected) fills the same
coefficient planes as the dense writers -- every frame below is compared bit for bit with the dense feed's and the CPU oracle's."""
import glob
import os

import numpy as np
import pytest

from conftest import assert_bits_equal
from jxlatte_amd import _lib, abi, host, synth
from jxlatte_amd.host import pack_sparse

pytestmark = pytest.mark.gpu

STAGES = abi.STAGE_IDCT | abi.STAGE_GAB | abi.STAGE_EPF


def make_frame(kind, nonzero_p=0.15, seed=0):
    if kind == "520x264":
        return synth.make_vardct_frame(520, 264, seed=77 + seed, aligned=False, nonzero_p=nonzero_p)
    if kind == "520x520":  # 3 x 3 groups
        return synth.make_vardct_frame(520, 520, seed=91 + seed, aligned=False, nonzero_p=nonzero_p)
    assert kind == "420"  # chroma-subsampled, built as tests/test_vardct_gpu.py::test_chroma_subsampled_frame builds it
    base = synth.make_vardct_frame(528, 272, seed=531 + seed, mix="dct8", xyb=0, nonzero_p=nonzero_p)
    return synth.make_subsampled(base, (1, 0, 1), (1, 0, 1))


def params_of(fr):
    p = abi.VarDCTParams.from_buffer_copy(fr["params"])
    p.stages = STAGES
    return p


def open_frame(ctx, fr):
    f = host.Frame(ctx, params_of(fr), fr["weights"], fr["woffs"])
    for g in fr["lfgroups"]:
        f.setLFGroup(g)
    return f


def dense_frame(ctx, fr):
    f = open_frame(ctx, fr)
    for grp in range(synth.num_groups(fr)):
        f.putGroup(0, grp, synth.group_view(fr, grp))
    return f.decodeFrame()


def with_coeff(fr, coeff):
    out = dict(fr)
    out["coeff"] = coeff
    return out


def group_rect(fr, grp):
    """(y0, y1, x0, x1) of a group in an unsubsampled frame"""
    grs = (fr["width"] + 255) // 256
    gy, gx = divmod(grp, grs)
    return gy * 256, min(gy * 256 + 256, fr["height"]), gx * 256, min(gx * 256 + 256, fr["width"])


def write_runs(words, at, fr, groups, planes_of=None, wide_of=lambda grp, c: False):
    """append one run per (group, channel) of `groups` at word `at` of the mapped buffer, each on a 16-byte boundary and padded
    with zero entries; -> (runs, next free word)"""
    runs = []
    for grp in groups:
        planes = planes_of(grp) if planes_of else synth.group_view(fr, grp)
        for c in range(3):
            wide = wide_of(grp, c)
            e = pack_sparse(np.ascontiguousarray(planes[c]), wide)
            end = at + ((e.size + 3) & ~3)
            words[at:at + e.size] = e
            words[at + e.size:end] = 0
            runs.append((grp, c, at, e.size // (2 if wide else 1), wide))
            at = end
    return runs, at


def capacity(fr, passes=1):
    return (passes * (2 * int(np.count_nonzero(fr["coeff"])) + 4 * 3 * synth.num_groups(fr) + 2 * 3 * 65536) + 16) & ~3


# ---- 1. single-group parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["pageable", "pinned", "misaligned"])
@pytest.mark.parametrize("nonzero_p", [0.0, 0.15, 1.0])
@pytest.mark.parametrize("kind", ["520x264", "420", "520x520"])
def test_put_group_sparse_equals_put_group(ctx, orc, kind, nonzero_p, source):
    """every group through putGroupSparse, one pass and two (split as test_int16_wire_format_and_pinned_buffers splits them: 12 or 18
    puts wrap the staging ring of 8), from pageable lists, page-locked ones the device reads in place, and page-locked ones that
    are not 16-byte aligned (the copying path again)"""
    fr = make_frame(kind, nonzero_p)
    lib = _lib.load()
    keep = []

    def feed(passes):
        f = open_frame(ctx, fr)
        for grp in range(synth.num_groups(fr)):
            planes = synth.group_view(fr, grp)
            for ps in range(passes):
                part = [(a - 3 * (passes - 1) if ps == 0 else np.full_like(a, 3)) for a in planes]
                if source == "pageable":
                    f.putGroupSparse(ps, grp, part)
                    continue
                pad = 1 if source == "misaligned" else 0
                ents = []
                for a in part:
                    e = pack_sparse(a)
                    pa = host.PinnedArray(lib, (e.size + pad,), np.uint32)
                    pa.array[pad:] = e
                    keep.append(pa)
                    ents.append(pa.array[pad:])
                    assert e.size == 0 or (ents[-1].ctypes.data % 16 == 0) == (pad == 0)
                f.putGroupSparseEntries(ps, grp, ents, False)
        out = f.decodeFrame()
        assert f.sparseRejected() == 0
        return out

    ref = dense_frame(ctx, fr)
    assert_bits_equal(ref, orc.vardct_frame(fr, stages=STAGES), "dense feed vs oracle")
    assert_bits_equal(feed(1), ref, "sparse, one pass")
    assert_bits_equal(feed(2), ref, "sparse, two passes")
    for x in keep:
        x.free()


def test_put_group_sparse_wide_entries(ctx, orc):
    """values outside int16 pick the wide form (as jxl_vardct_put_group stands in for the int16 entry); a dense group in wide
    entries is longer than a slot of the staging ring and goes up in pieces"""
    fr = make_frame("520x264", 1.0)
    big = fr["coeff"].copy()
    big[1, 3, 5] = 70000
    big[2, 200, 300] = -70000
    bigf = with_coeff(fr, big)
    f = open_frame(ctx, fr)
    for grp in range(synth.num_groups(fr)):
        f.putGroupSparse(0, grp, synth.group_view(bigf, grp), wide=True if grp == 0 else None)
    assert_bits_equal(f.decodeFrame(), orc.vardct_frame(bigf, stages=STAGES), "wide entries")


# ---- 2. mixed runs and override -------------------------------------------------------------------------------------------------
def test_commit_sparse_mixed_runs_and_dense_override(ctx, orc):
    fr = make_frame("520x264", seed=1)
    big = fr["coeff"].copy()
    big[1, 3, 5] = 70000  # group 0, channel 1: its run is wide, all others narrow
    bigf = with_coeff(fr, big)
    groups = range(synth.num_groups(fr))

    def commit(f):
        words = f.mapSparse(capacity(bigf))
        runs, _ = write_runs(words, 0, bigf, groups, wide_of=lambda grp, c: (grp, c) == (0, 1))
        assert sum(1 for r in runs if r[4]) == 1
        f.commitSparse(runs)

    f = open_frame(ctx, fr)
    commit(f)
    assert_bits_equal(f.decodeFrame(), orc.vardct_frame(bigf, stages=STAGES), "one commit, one wide run")
    assert f.sparseRejected() == 0
    # a dense put after the commit overrides its rectangle, as after the int16 commit
    alt = big.copy()
    y0, y1, x0, x1 = group_rect(fr, 1)
    alt[:, y0:y1, x0:x1] = -big[:, y0:y1, x0:x1] + 1
    altf = with_coeff(fr, alt)
    f = open_frame(ctx, fr)
    commit(f)
    f.putGroup(0, 1, synth.group_view(altf, 1))
    assert_bits_equal(f.decodeFrame(), orc.vardct_frame(altf, stages=STAGES), "putGroup after commitSparse")


# ---- 3. groups no run names ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["520x520", "420"])
def test_commit_sparse_unnamed_groups_read_as_zero(ctx, orc, kind):
    fr = make_frame(kind, seed=2)
    n = synth.num_groups(fr)
    skip = {1, n - 1}
    zeroed = dict(fr)
    f0 = open_frame(ctx, fr)  # the expected frame: the dense feed without those groups (never put: they read as zero)
    for grp in range(n):
        if grp not in skip:
            f0.putGroup(0, grp, synth.group_view(fr, grp))
    exp = f0.decodeFrame()
    if kind == "520x520":
        z = fr["coeff"].copy()
        for grp in skip:
            y0, y1, x0, x1 = group_rect(fr, grp)
            z[:, y0:y1, x0:x1] = 0
        zeroed["coeff"] = z
        assert_bits_equal(exp, orc.vardct_frame(zeroed, stages=STAGES), "dense feed without two groups vs oracle")
    f = open_frame(ctx, fr)
    words = f.mapSparse(capacity(fr))
    runs, _ = write_runs(words, 0, fr, [g for g in range(n) if g not in skip])
    f.commitSparse(runs)
    assert_bits_equal(f.decodeFrame(), exp, "commitSparse without two groups")


# ---- 4. two passes -----------------------------------------------------------------------------------------------------------------
def test_two_sparse_commits_are_two_passes(ctx, orc):
    fr = make_frame("520x520", seed=3)
    a = fr["coeff"] // 2
    b = fr["coeff"] - a
    fa, fb = with_coeff(fr, a), with_coeff(fr, b)
    groups = range(synth.num_groups(fr))
    exp = orc.vardct_frame(fr, stages=STAGES)

    f = open_frame(ctx, fr)
    words = f.mapSparse(capacity(fr))
    runs, _ = write_runs(words, 0, fr, groups)
    f.commitSparse(runs)
    one = f.decodeFrame()
    assert_bits_equal(one, exp, "one commit")

    f = open_frame(ctx, fr)
    words = f.mapSparse(capacity(fa) + capacity(fb))
    ra, at = write_runs(words, 0, fa, groups)
    rb, _ = write_runs(words, at, fb, groups)
    f.commitSparse(ra)
    f.commitSparse(rb)
    assert_bits_equal(f.decodeFrame(), one, "two commits of half values")

    f = open_frame(ctx, fr)  # the second pass from a buffer mapped again (waits for the first commit's reads only)
    words = f.mapSparse(capacity(fa))
    ra, _ = write_runs(words, 0, fa, groups)
    f.commitSparse(ra)
    words = f.mapSparse(capacity(fb))
    rb, _ = write_runs(words, 0, fb, groups)
    f.commitSparse(rb)
    assert_bits_equal(f.decodeFrame(), one, "two commits, mapped twice")

    f = open_frame(ctx, fr)
    for grp in groups:
        f.putGroup(0, grp, synth.group_view(fa, grp))
    for grp in groups:
        f.putGroup(1, grp, synth.group_view(fb, grp))
    assert_bits_equal(f.decodeFrame(), one, "dense two-pass feed")

    f = open_frame(ctx, fr)  # mixed: a sparse commit, then the later pass through the dense writer and through putGroupSparse
    words = f.mapSparse(capacity(fa))
    ra, _ = write_runs(words, 0, fa, groups)
    f.commitSparse(ra)
    for grp in groups:
        if grp % 2:
            f.putGroup(1, grp, synth.group_view(fb, grp))
        else:
            f.putGroupSparse(1, grp, synth.group_view(fb, grp))
    assert_bits_equal(f.decodeFrame(), one, "sparse commit + later pass per group")


# ---- 5. override after a dense commit ------------------------------------------------------------------------------------------
def test_pass0_sparse_put_replaces_a_densely_committed_rectangle(ctx, orc):
    fr = make_frame("520x264", seed=4)
    other = make_frame("520x264", nonzero_p=1.0, seed=5)["coeff"]  # every sample non-zero: leftovers would show
    n = synth.num_groups(fr)
    chosen = [0, 2, 3, 5]
    mixed = other.copy()
    empty = fr["coeff"].copy()
    y0, y1, x0, x1 = group_rect(fr, 3)
    empty[:, y0:y1, x0:x1] = 0  # group 3 is replaced by NO entries: its rectangle must still be cleared
    emptyf = with_coeff(fr, empty)
    for grp in chosen:
        y0, y1, x0, x1 = group_rect(fr, grp)
        mixed[:, y0:y1, x0:x1] = empty[:, y0:y1, x0:x1]
    f = open_frame(ctx, fr)
    planes = f.mapCoeffsI16()
    for c in range(3):
        planes[c][...] = other[c]
    f.commitCoeffsI16()
    for grp in chosen:
        f.putGroupSparse(0, grp, synth.group_view(emptyf, grp))
    assert_bits_equal(f.decodeFrame(), orc.vardct_frame(with_coeff(fr, mixed), stages=STAGES), "sparse override of a dense commit")
    assert n == 6


# ---- 6. rejected entries ---------------------------------------------------------------------------------------------------------
def test_entries_outside_the_rectangle_are_refused(ctx, orc):
    """group 2 of a 520x264 frame is the right edge group of the TOP group row: 8 samples wide. An entry with x >= 8 that slipped
    through would land in the first cells of the next cell row of the tiled plane -- visible samples of the frame"""
    fr = make_frame("520x264", seed=6)
    ref = dense_frame(ctx, fr)
    lib = _lib.load()
    assert group_rect(fr, 2) == (0, 256, 512, 520)
    bad = np.array([(9 << 16) | (0 << 8) | 8, (0xfff7 << 16) | (17 << 8) | 9, (5 << 16) | (255 << 8) | 255, (7 << 16) | (40 << 8) | 100],
                   np.uint32)

    def feed(pinned):
        f = open_frame(ctx, fr)
        keep = []
        for grp in range(synth.num_groups(fr)):
            ents = pack_sparse(synth.group_view(fr, grp))
            if grp == 2:
                ents[1] = np.concatenate([ents[1][:5], bad[:2], ents[1][5:], bad[2:]])
            if pinned:
                pas = [host.PinnedArray(lib, (e.size,), np.uint32) for e in ents]
                for pa, e in zip(pas, ents):
                    pa.array[:] = e
                keep.extend(pas)
                ents = [pa.array for pa in pas]
            f.putGroupSparseEntries(0, grp, ents)
        return f, keep

    f, keep = feed(True)
    got = f.decodeFrame()
    assert f.sparseRejected() == bad.size
    assert_bits_equal(got, ref, "frame with refused entries")
    # a wide entry whose position word has bits above the low 16 is refused too (later pass, in place)
    w = host.PinnedArray(lib, (4,), np.uint32)
    w.array[:] = [0x10000, 5, (300 << 8) | 1, 5]
    z = np.zeros(0, np.uint32)
    f.putGroupSparseEntries(1, 2, [w.array, z, z], True)
    assert f.sparseRejected() == bad.size + 2
    assert_bits_equal(f.decodeFrame(), ref, "frame with refused wide entries")
    for x in keep + [w]:
        x.free()
    # the copying path refuses the same call before anything is queued, and the frame goes on
    f = open_frame(ctx, fr)
    for grp in range(synth.num_groups(fr)):
        ents = pack_sparse(synth.group_view(fr, grp))
        if grp == 2:
            with pytest.raises(_lib.JxlError) as e:
                f.putGroupSparseEntries(0, grp, [ents[0], np.concatenate([ents[1], bad]), ents[2]])
            assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT
        f.putGroupSparseEntries(0, grp, ents)
    assert_bits_equal(f.decodeFrame(), ref, "after a refused call")
    assert f.sparseRejected() == 0


# ---- 7. error returns --------------------------------------------------------------------------------------------------------------
def test_sparse_error_returns_leave_the_frame_usable(ctx, orc):
    fr = make_frame("520x264", seed=7)
    ref = dense_frame(ctx, fr)
    n = synth.num_groups(fr)
    f = open_frame(ctx, fr)
    with pytest.raises(_lib.JxlError) as e:
        f.commitSparse([(0, 0, 0, 0, False)])  # nothing mapped in this frame
    assert e.value.status == abi.JXL_ERR_STATE
    cap = capacity(fr)
    words = f.mapSparse(cap)
    runs, at = write_runs(words, 0, fr, range(n))
    good = runs[0]
    for what, run in (("past the capacity", (0, 0, cap - 4, 8, False)),
                      ("wide run past the capacity", (0, 0, cap - 8, 5, True)),
                      ("channel 3", (0, 3, 0, 1, False)),
                      ("negative channel", (0, -1, 0, 1, False)),
                      ("group out of range", (n, 0, 0, 1, False)),
                      ("negative group", (-1, 0, 0, 1, False)),
                      ("misaligned offset", (0, 0, 2, 1, False)),
                      ("negative count", (0, 0, 0, -1, False)),
                      ("unknown flag", (0, 0, 0, 1, 2))):
        with pytest.raises(_lib.JxlError) as e:
            f.commitSparse([good, run])  # the bad run comes second: the first must not have been queued either
        assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT, what
    with pytest.raises(_lib.JxlError) as e:
        f.ctx.call("jxl_vardct_put_group_sparse", 0, 0, None, None, 0)
    assert e.value.status == abi.JXL_ERR_INVALID_ARGUMENT
    f.commitSparse(runs)
    assert_bits_equal(f.decodeFrame(), ref, "correct feed after the refused commits")
    assert f.sparseRejected() == 0


# ---- 8. repeatability ------------------------------------------------------------------------------------------------------------
def test_same_feed_twice_gives_identical_planes_also_with_duplicates(ctx, orc):
    """entries add, and integer adds commute: duplicate positions receive the sum of their values, the same on every run"""
    fr = make_frame("520x520", seed=8)

    def feed():
        f = open_frame(ctx, fr)
        words = f.mapSparse(2 * capacity(fr))
        runs, at = [], 0
        for grp in range(synth.num_groups(fr)):
            for c, a in enumerate(synth.group_view(fr, grp)):
                e = pack_sparse(a)
                dup = e[::3]  # every third entry arrives as two entries at its position: value - 5 here, 5 behind the others
                first = e.copy()
                first[::3] = (((dup >> 16) - 5) & 0xffff) << 16 | (dup & 0xffff)
                e = np.concatenate([first, (np.uint32(5) << 16) | (dup & 0xffff)])
                e = e[np.random.default_rng(grp * 3 + c).permutation(e.size)]
                words[at:at + e.size] = e
                runs.append((grp, c, at, e.size, False))
                at += (e.size + 3) & ~3
        f.commitSparse(runs)
        return f.decodeFrame()

    one, two = feed(), feed()
    assert_bits_equal(one, two, "same feed twice")
    assert_bits_equal(one, orc.vardct_frame(fr, stages=STAGES), "duplicates sum")


def test_commit_sparse_with_more_runs_than_one_launch_takes(ctx, orc):
    """more runs than the run table of one launch holds (2048): every 8x8 cell of every group as a run of its own"""
    fr = make_frame("520x264", seed=9)
    f = open_frame(ctx, fr)
    cells = sum(a.size // 64 for grp in range(synth.num_groups(fr)) for a in synth.group_view(fr, grp))
    words = f.mapSparse(capacity(fr) + 4 * cells)
    runs, at = [], 0
    for grp in range(synth.num_groups(fr)):
        for c, a in enumerate(synth.group_view(fr, grp)):
            for cy in range(0, a.shape[0], 8):
                for cx in range(0, a.shape[1], 8):
                    cell = np.zeros_like(a)
                    cell[cy:cy + 8, cx:cx + 8] = a[cy:cy + 8, cx:cx + 8]
                    e = pack_sparse(cell)
                    words[at:at + e.size] = e
                    runs.append((grp, c, at, e.size, False))
                    at += (e.size + 3) & ~3
    assert len(runs) == cells > 2 * 2048
    f.commitSparse(runs)
    assert_bits_equal(f.decodeFrame(), orc.vardct_frame(fr, stages=STAGES), "%d runs" % len(runs))


# ---- 10. decoder -------------------------------------------------------------------------------------------------------------------
SAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SAMPLES, "*.jxl"))))
def test_decoder_with_sparse_coeffs_gives_the_same_pixels(name):
    from jxlatte_amd.decoder import DeviceBackend, JXLDecoder
    dev = DeviceBackend(0)
    try:
        a = JXLDecoder(os.path.join(SAMPLES, name + ".jxl"), backend=dev, sparse_coeffs=True).decode()
        b = JXLDecoder(os.path.join(SAMPLES, name + ".jxl"), backend=dev).decode()
    finally:
        dev.close()
    assert len(a.buffer) == len(b.buffer) and len(a.buffer) > 0
    for c, (x, y) in enumerate(zip(a.buffer, b.buffer)):
        assert_bits_equal(x, y, "%s channel %d" % (name, c))


def test_load_vardct_frame_sparse(ctx):
    from jxlatte_amd.decoder import load_vardct_frame
    p = os.path.join(SAMPLES, "lenna.jxl")
    a, _ = load_vardct_frame(p, ctx, sparse=True)
    got = a.decodeFrame()
    b, _ = load_vardct_frame(p, ctx)
    assert_bits_equal(got, b.decodeFrame(), "load_vardct_frame(sparse=True)")
