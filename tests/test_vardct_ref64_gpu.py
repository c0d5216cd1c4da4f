"""The HIP kernels against tests/vardct_ref64.py, the float64 model of the reference's VarDCT pixel path, WITHOUT the oracle in the
assertion: the inputs, the bound |got - model| <= K u (A + |model|) and the K table are those of tests/test_vardct_ref64_cpu.py
(where the K of the nonlinear stages were measured on the CPU oracle, never on these kernels). Every other GPU test of the path
compares with the oracle bit for bit, which cannot see an error that oracle and kernels share; this file can.

Frames go through the C-ABI as the host hands them over (host.Frame with the case's own weight tables, decodeFrame at stage sets
1, 3, 7 and 15, float32 planes out): dense groups, the sparse coefficient feed and jxl_vardct_run_batch; then the stage entries."""
import numpy as np
import pytest

import test_vardct_ref64_cpu as T
import vardct_ref64 as M
import vardct_ref64_cases as C
from jxlatte_amd import _lib, abi, host, synth

pytestmark = pytest.mark.gpu
F = np.float32
IDCT, GAB, EPF, XYB = T.IDCT, T.GAB, T.EPF, T.XYB
SPECIALS = ["HORNUSS", "DCT2", "DCT4", "DCT4_8", "DCT8_4", "AFV0", "AFV1", "AFV2", "AFV3"]
THREE_SIZES = [(64, 64), (328, 200), (1024, 520)]  # those of tests/test_idct_items_gpu.py: below one item, ragged, many items


def decode(ctx, frame, stages):
    return host.Frame.from_synth(ctx, frame, stages=stages).decodeFrame()


def decode_sparse(ctx, frame, stages):
    p = abi.VarDCTParams.from_buffer_copy(frame["params"])
    p.stages = stages
    fr = host.Frame(ctx, p, frame["weights"], frame["woffs"])
    for g in frame["lfgroups"]:
        fr.setLFGroup(g)
    for grp in range(synth.num_groups(frame)):
        fr.putGroupSparse(0, grp, synth.group_view(frame, grp))
    out = fr.decodeFrame()
    assert fr.sparseRejected() == 0
    return out


TYPE_CASES = [(t, None) for t in range(27) if abi.TT_NAME[t] not in SPECIALS + ["DCT64"]] + \
             [(abi.TT_BY_NAME[n], s) for n in SPECIALS + ["DCT64"] for s in THREE_SIZES]


@pytest.mark.parametrize("t,size", TYPE_CASES, ids=["%s-%s" % (abi.TT_NAME[t], "x".join(map(str, s)) if s else "std") for t, s in TYPE_CASES])
def test_single_type_frame(ctx, t, size):
    fr = C.type_frame(t, size)
    assert (fr["block_types"] == t).any()
    T.check(decode(ctx, fr, IDCT), fr, IDCT, "%s %s" % (abi.TT_NAME[t], size))


@pytest.mark.parametrize("case", C.MIXED, ids=[m[0] for m in C.MIXED])
def test_mixed_frame(ctx, case):
    name, w, h, seed, mix, aligned = case
    fr = C.frame(w, h, seed, mix, aligned)
    T.check(decode(ctx, fr, IDCT), fr, IDCT, name)


@pytest.mark.parametrize("mode", sorted(C.SUBSAMPLINGS))
def test_subsampled_frame(ctx, mode):
    fr = C.subsampled_frame(mode)
    for stages in (IDCT, GAB, EPF):
        T.check(decode(ctx, fr, stages), fr, stages, "subsampled %s" % mode)


@pytest.mark.parametrize("name", [s[0] for s in C.STAGED])
def test_staged_frame(ctx, name):
    fr = C.staged_frame(name)
    for stages in (IDCT, GAB, EPF, XYB):
        T.check(decode(ctx, fr, stages), fr, stages, name)


def test_batch_of_three_frames():
    names = ["it2_gab1", "it3_gab0", "it1_gab1"]
    ctxs = [_lib.Context(0) for _ in names]
    try:
        frames = [host.Frame.from_synth(c, C.staged_frame(n), stages=XYB) for c, n in zip(ctxs, names)]
        host.Frame.runBatch(frames)
        for fr, n in zip(frames, names):
            T.check(fr.readOutput(), C.staged_frame(n), XYB, "batch %s" % n)
    finally:
        for c in ctxs:
            c.close()


SPARSE_CASES = [("DCT8", lambda: C.type_frame(0), IDCT), ("AFV2", lambda: C.type_frame(16), IDCT), ("DCT64", lambda: C.type_frame(18), IDCT),
                ("DCT256_128", lambda: C.type_frame(25), IDCT), ("all_unaligned", lambda: C.frame(512, 512, 5, "all", False), IDCT),
                ("ragged_264x520", lambda: C.frame(264, 520, 8, "default", False), IDCT),
                ("420", lambda: C.subsampled_frame("420"), EPF), ("it3_gab1", lambda: C.staged_frame("it3_gab1"), XYB)]


@pytest.mark.parametrize("case", SPARSE_CASES, ids=[c[0] for c in SPARSE_CASES])
def test_sparse_feed(ctx, case):
    """the same frames through Frame.putGroupSparse (the wild ones carry -777 and +-64: narrow entries; nothing is rejected)"""
    name, make, stages = case
    fr = make()
    T.check(decode_sparse(ctx, fr, stages), fr, stages, "sparse %s" % name)


# ---- stage entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,t", C.IDCT2D_SIZES)
def test_stage_idct2d_fdct2d(ctx, h, w, t):
    x = np.random.default_rng(h * 7 + w).standard_normal((h, w)).astype(F)
    T.stage_ratio(host.MathHelper.inverseDCT2D(ctx, x, t), *M.idct2d(x, t), "idct2d %dx%d" % (h, w), T.K_STAGE["idct2d"](h, w))
    T.stage_ratio(host.MathHelper.forwardDCT2D(ctx, x), *M.fdct2d(x), "fdct2d %dx%d" % (h, w), T.K_STAGE["idct2d"](h, w))


@pytest.mark.parametrize("h,w", C.STAGE_SIZES)
def test_stage_gab_epf(ctx, h, w):
    p, sig = C.stage_planes(h, w), C.stage_sigma(h, w)
    T.stage_ratio(host.performGabConvolution(ctx, p, *C.GAB_W), *M.gab(p, np.abs(p), *C.GAB_W), "gab %dx%d" % (h, w), T.K_STAGE["gab"])
    dead = np.repeat(np.repeat(~(sig <= M.COPY_THRESHOLD), 8, 0), 8, 1)[:h, :w]  # inf, NaN and 3.4 cells: copied, as the reference does
    for iters in range(4):
        got = host.performEdgePreservingFilter(ctx, p, iters, sig, 0.0, *C.EPF_ARGS)
        T.stage_ratio(got, *M.epf(p, np.abs(p), iters, sig, *C.EPF_ARGS), "epf %dx%d it%d" % (h, w, iters), T.K_STAGE["epf"])
        assert np.array_equal(got[:, dead], p[:, dead])


def test_stage_epf_sigma_and_xyb(ctx):
    rng = np.random.default_rng(8)
    hf = rng.integers(1, 20, size=(9, 13)).astype(np.int32)
    sh = rng.integers(0, 8, size=(9, 13)).astype(np.int32)
    par = M.params_dict(synth.default_params(8, 8))
    model = M.epf_sigma(hf, sh, 26.2144, par["epf_sharp_lut"])
    T.stage_ratio(host.epfInverseSigma(ctx, hf, sh, 26.2144, par["epf_sharp_lut"]), model, np.abs(model), "epf sigma", T.K_STAGE["epf_sigma"])
    x = C.stage_planes(37, 91) * F(3.0)
    m = host.OpsinInverseMatrix(par["opsin_matrix"], par["opsin_bias"], par["cbrt_opsin_bias"])
    for it in (255.0, 10000.0):
        T.stage_ratio(m.invertXYB(ctx, x, it), *M.xyb(x, np.abs(x), par["opsin_matrix"], par["opsin_bias"], par["cbrt_opsin_bias"], it),
                      "xyb %g" % it, T.K_STAGE["xyb"])
