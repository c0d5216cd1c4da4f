"""tests/restore_variants.py without a GPU: the restated geometry gives the sizes of tests/test_restore_variants_gpu.py the properties
they were chosen for, the table covers every sink kind of restore_sink.h and every (transfer, out_format) pair
jxl_vardct_begin_frame accepts, and the cases it lists promise every instantiation of every kind it claims in full."""
import os
import re

import pytest

import restore_variants as rv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jxlatte_amd", "csrc")


def _read(*path):
    with open(os.path.join(*path), encoding="utf-8") as f:
        return f.read()


def _launch_geometries():
    """(size, Gaborish, ITERS of the instantiation) of every launch of every single-frame case"""
    out = set()
    for c in rv.all_cases():
        if c.form in ("batch", "batch3"):
            continue
        for x in rv.expected_launches(c):
            out.add((c.sizes[0], x >> 6 & 1, x >> 3 & 7))
    return sorted(out)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def test_geometry_restates_the_kernel_header():
    """the numbers of rv.geo against the constants of Geo<GAB, ITERS> as the header spells them"""
    text = _read(CSRC, "restore_fused_body.h")
    for needle in ("R0 = (ITERS == 3 || ITERS == 4) ? 3 : 0", "R1 = (ITERS >= 1 && ITERS <= 3) ? 2 : 0", "R2 = (ITERS == 2 || ITERS == 3) ? 1 : 0",
                   "SHR = ITERS == 3 ? (R1 + R2) : ITERS == 2 ? R2 : 0", "WH = ITERS == 4 ? JXL_EPF0_WH : 32", "#define JXL_EPF0_WH 64",
                   "OW = 64 - 2 * SHR, OH = WH - 2 * SHR", "RT = RE + RG",
                   "tc.edge = tc.ix0 < 0 || tc.iy0 < 0 || tc.ix0 + G::IW > W || tc.iy0 + G::IH > H"):
        assert needle in text, needle
    for gab in (0, 1):
        for iters in range(5):
            r0 = 3 if iters in (3, 4) else 0
            r1 = 2 if 1 <= iters <= 3 else 0
            r2 = 1 if iters in (2, 3) else 0
            shr = r1 + r2 if iters == 3 else r2 if iters == 2 else 0
            wh = 64 if iters == 4 else 32
            assert rv.geo(gab, iters) == (64 - 2 * shr, wh - 2 * shr, r0 + r1 + r2 + gab)
    assert [rv.geo(0, it) for it in range(5)] == [(64, 32, 0), (64, 32, 2), (62, 30, 3), (58, 26, 6), (64, 64, 3)]


@pytest.mark.parametrize("size,gab,iters", [g for g in _launch_geometries() if g[0] != rv.ALL_EDGE], ids=str)
def test_size_has_interior_ragged_and_surplus(size, gab, iters):
    """every launch of a single-frame case at the two large sizes: at least one interior tile (the other code path after
    Gaborish), ragged last tiles in both directions, and a tile count that is no multiple of 8 (the grid is rounded up: the early
    exit `tile >= n_tiles` runs)"""
    w, h = size
    tx, ty = rv.tile_grid(w, h, gab, iters)
    assert rv.interior_tiles(w, h, gab, iters), (tx, ty)
    assert len(rv.interior_tiles(w, h, gab, iters)) < tx * ty  # ... and edge tiles beside them
    assert rv.ragged(w, h, gab, iters)
    assert (tx * ty) % 8 != 0 and rv.launched_workgroups(tx * ty) > tx * ty


def test_the_tile_grids_worked_by_hand():
    assert [rv.tile_grid(264, 112, 1, it) for it in (0, 1, 2, 3)] == [(5, 4), (5, 4), (5, 4), (5, 5)]
    assert rv.tile_grid(264, 136, 1, 4) == (5, 3) and rv.tile_grid(264, 136, 0, 2) == (5, 5)
    assert {j for _, j in rv.interior_tiles(264, 136, 1, 4)} == {1}  # the 64x64 launch: one interior row


def test_large_sizes_cover_every_geometry_a_case_uses():
    geos = _launch_geometries()
    assert {(g, it) for s, g, it in geos if s == rv.MAIN} == {(g, it) for g in (0, 1) for it in (0, 1, 2, 3)}
    assert {(g, it) for s, g, it in geos if s == rv.SPLIT} == {(1, 4), (0, 4), (0, 2)}
    assert all(w % 8 == 0 and h % 8 == 0 for w, h in rv.SEEDS)


def test_all_edge_size_has_no_interior_tile():
    """... at any variant with a halo; without one (no Gaborish, no iteration) a whole tile inside the frame is interior by the rule"""
    for gab in (0, 1):
        for iters in range(5):
            inner = rv.interior_tiles(rv.ALL_EDGE[0], rv.ALL_EDGE[1], gab, iters)
            assert inner == ([(0, 0)] if rv.geo(gab, iters)[2] == 0 else []), (gab, iters, inner)


def test_batch_grid_is_sized_by_the_first_frame_and_the_others_leave_workgroups():
    for gab in (0, 1):
        for iters in (0, 1, 2, 3):
            n = [tx * ty for tx, ty in (rv.tile_grid(w, h, gab, iters) for w, h in rv.BATCH)]
            assert n[0] == max(n) and n[0] % 8 != 0
            assert all(rv.launched_workgroups(n[0]) - k >= 8 for k in n[1:])  # whole rounds of surplus workgroups, on every XCD
            assert rv.interior_tiles(rv.BATCH[0][0], rv.BATCH[0][1], gab, iters)


# ---- inventory --------------------------------------------------------------------------------------------------------------------
def _sink_kinds_of_the_header():
    m = re.search(r"enum SinkKind \{(.*?)\};", _read(CSRC, "restore_sink.h"), re.S)
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return {name: int(val) for name, val in re.findall(r"(SK_[A-Z0-9_]+)\s*=\s*(\d+)", body)}


def test_every_sink_kind_has_rows():
    kinds = _sink_kinds_of_the_header()
    assert kinds.pop("SK_COUNT") == len(kinds)
    assert kinds == rv.SINK_KINDS
    for k in kinds:
        assert any(r.kind == k for r in rv.ROWS), "no row of tests/restore_variants.py leads into %s" % k
    compile_time = sorted(k for k in kinds if k not in ("SK_PLAIN", "SK_GENERIC"))
    assert compile_time == sorted(rv.COMPILE_TIME_KINDS)
    for k in compile_time:  # a kind fixed at compile time runs every launch form
        assert any(r.kind == k and r.full for r in rv.ROWS), k


def test_every_accepted_transfer_and_format_pair_has_a_row():
    header = _read(ROOT, "include", "jxlatte_amd.h")
    tfs = {n: int(v) for n, v in re.findall(r"#define JXL_TRANSFER_([A-Z_]+)\s+(\d+)", header)}
    fmts = {n: int(v) for n, v in re.findall(r"#define JXL_OUT_([A-Z0-9]+)\s+(\d+)", header)}
    assert tfs == rv.TRANSFERS and fmts == rv.OUT_FORMATS
    # jxl_vardct_begin_frame takes the whole range of both
    assert "p->out_format < 0 || p->out_format > JXL_OUT_%s || p->transfer < 0 || p->transfer > JXL_TRANSFER_%s" % (
        max(fmts, key=fmts.get), max(tfs, key=tfs.get)) in _read(CSRC, "host.hip")
    rows = [(r.transfer, r.fmt) for r in rv.ROWS]
    assert len(rows) == len(set(rows))
    assert set(rows) == {(t, f) for t in tfs for f in fmts}


def test_rows_name_the_kind_the_selection_rule_gives():
    text = re.sub(r"\s+", " ", _read(CSRC, "restore_sink.h"))
    for needle in ("if (p.transfer == JXL_TRANSFER_NONE && p.max_value == 0) return SK_PLAIN;",
                   "if (p.transfer == JXL_TRANSFER_PQ && p.max_value == 65535 && p.out_elem == 2 && p.pq_tab && p.pq16_thr) return p.interleaved ? SK_PQ_RGB16 : SK_PQ_U16;",
                   "if (p.transfer == JXL_TRANSFER_SRGB && p.max_value == 255 && p.out_elem == 1 && p.interleaved && p.srgb8_tab) return SK_SRGB_RGB8;",
                   "if (p.transfer == JXL_TRANSFER_SRGB && p.max_value == 65535 && p.out_elem == 2 && p.interleaved && p.srgb16_tab) return SK_SRGB_RGB16;"):
        assert needle in text, "sink_kind_of changed: restate it in restore_variants.sink_kind (%s)" % needle
    for r in rv.ROWS:
        assert rv.sink_kind(r.transfer, r.fmt) == r.kind, r
    assert sorted(r.kind for r in rv.ROWS if r.kind in rv.COMPILE_TIME_KINDS) == sorted(rv.COMPILE_TIME_KINDS)  # one way into each


def test_table_promises_every_instantiation_of_the_full_kinds():
    """22 per sink kind; the three-iteration single and batch launches (4 of the 22) need the child process"""
    promised = rv.promised()
    for k in rv.COMPILE_TIME_KINDS + ("SK_GENERIC",):
        inv = rv.inventory(k)
        assert len(inv) == 22 and inv <= promised, [rv.describe(x) for x in sorted(inv - promised)]
        in_child = {x for x in inv if (x >> 3 & 7) == 3}
        assert len(in_child) == 4 and in_child <= rv.promised(child=True) and not in_child & rv.promised(child=False)
        assert inv - in_child <= rv.promised(child=False)
    # the float sink: what the split form and the one light row run here; its inventory belongs to the tests named in restore_variants.py
    assert {x for x in promised if (x & 7) == 0} == {rv.code("SK_PLAIN", 1, 4), rv.code("SK_PLAIN", 0, 4), rv.code("SK_PLAIN", 1, 2),
                                                    rv.code("SK_PLAIN", 1, 2, batch=True)}
    assert all((x & 7) < len(rv.SINK_KINDS) for x in promised)


def test_codes_are_restore_fused_variant_plus_two_bits():
    assert "return (a.p.gab ? 64 : 0) | (a.p.epf_iters & 7) << 3 | sink_kind_of(a.p);" in _read(CSRC, "k_restore_fused.hip")
    assert "kRestoreTiledBit = %d, kRestoreBatchBit = %d" % (rv.TILED_BIT, rv.BATCH_BIT) in _read(CSRC, "host.hip")
    assert rv.code("SK_SRGB_RGB16", 1, 2, tiled=True) == 64 + 16 + 5 + 128
    assert rv.describe(rv.code("SK_PQ_U16", 0, 3, batch=True)) == "SK_PQ_U16 gab 0 iters 3 batch"


def test_case_ids_are_unique_and_every_form_is_known():
    ids = [rv.case_id(c) for c in rv.all_cases()]
    assert len(ids) == len(set(ids))
    assert {c.form for c in rv.all_cases()} == set(rv.FORMS)
    assert len(rv.all_cases(True)) + len(rv.all_cases(False)) == len(ids)
