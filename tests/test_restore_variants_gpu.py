"""Every instantiation of the fused restoration kernel that a quantising sink has (tests/restore_variants.py: the table, the
geometry, the runner) decodes a frame with interior tiles, ragged last tiles and surplus workgroups, in every launch form -- single
launches on raster and on cell-tiled planes, the split three-iteration pair, batch launches of three frame sizes, and, in a child
process with JXL_EPF3_SPLIT=0, three iterations in one launch and in a batch launch.

Integer output equals the oracle bit for bit. Float output behind a transfer function equals jxl_stage_transfer of the same context's
float-plane decode bit for bit, and the oracle within the bars tests/test_stages_gpu.py holds the float curves to. After every run
jxl_debug_last_restore_launches must name the instantiation the table promises -- a case that fell to another path fails -- and the
last test holds the set of instantiations seen to the promised set."""
import pytest

import restore_variants as rv
import switch_cases as sc
from conftest import assert_bits_equal
from test_switches_gpu import run_child

pytestmark = pytest.mark.gpu

_seen = {}       # case id -> the launches its contexts reported
_child_seen = None


@pytest.fixture(scope="module")
def ctxs():
    c = rv.Contexts()
    yield c
    c.close()


def _run(c, ctxs):
    seen = set()
    problems = rv.check_case(c, ctxs, assert_bits_equal, seen)
    assert not problems, "\n".join(problems)
    _seen[rv.case_id(c)] = seen


_GROUPS = [(row, form) for row in rv.ROWS for form, in_child in rv.FORMS.items() if not in_child and rv.cases_of(row, form)]


@pytest.mark.parametrize("row,form", _GROUPS, ids=["%s-%s" % (rv.row_id(r), f) for r, f in _GROUPS])
def test_sink_in_launch_form(ctxs, row, form):
    for c in rv.cases_of(row, form):
        _run(c, ctxs)


def _child():
    global _child_seen
    if _child_seen is None:
        out = run_child("restore_variants_epf3", {"JXL_EPF3_SPLIT": "0"}, 120)
        _child_seen = {int(ln.split()[1]) for ln in out.split("\n") if ln.startswith("SEEN ")}
    return _child_seen


def test_three_iterations_in_one_launch_and_in_a_batch_launch():
    """JXL_EPF3_SPLIT=0 in a fresh process (switch_cases.case_restore_variants_epf3): the child holds every result to the oracle
    and every launch to the table, and reports what it saw"""
    assert _child() == rv.promised(child=True), sorted(rv.describe(x) for x in _child() ^ rv.promised(child=True))


@pytest.mark.parametrize("kind", rv.COMPILE_TIME_KINDS)
def test_second_run_on_the_same_context_gives_the_same_bytes(ctxs, kind):
    """the wide stores of the compile-time kinds: a hazard between them showed from one run to the next. The case with interior
    tiles on raster planes, and the batch, each twice on the contexts that just ran them."""
    row = [r for r in rv.ROWS if r.kind == kind][0]
    for c in (rv.Case(row, "raster", 1, 2, (rv.MAIN,)), rv.Case(row, "batch", 1, 2, rv.BATCH)):
        first = [got.tobytes() for _, _, _, got in rv.run_case(c, ctxs)]
        for what, cx, size, got in rv.run_case(c, ctxs):
            assert rv.last_launches(cx) == rv.expected_launches(c), what
            assert got.tobytes() == first.pop(0), what + ": the second run differs from the first"
            assert_bits_equal(sc.planar(got), rv.oracle_of(c, size), what + ": second run against the oracle")


def test_every_promised_instantiation_ran(ctxs):
    """the launches seen -- here and in the child -- are the table's: 22 per compile-time kind and for the generic sink. Cases that
    have not run in this session yet (a selection of tests) run now."""
    for c in rv.all_cases(child=False):
        if rv.case_id(c) not in _seen:
            _run(c, ctxs)
    seen = set().union(*_seen.values()) | _child()
    promised = rv.promised()
    assert seen == promised, "missing: %s; unexpected: %s" % (sorted(rv.describe(x) for x in promised - seen),
                                                             sorted(rv.describe(x) for x in seen - promised))
    for kind in rv.COMPILE_TIME_KINDS + ("SK_GENERIC",):
        assert rv.inventory(kind) <= seen, kind
