"""The HIP kernels against tests/pixel_ref64.py, the second model of the stages outside the VarDCT pixel path, WITHOUT the oracle in
any assertion: the inputs, the bounds and the K table are those of tests/test_pixel_ref64_cpu.py (where the K of the nonlinear stages
were measured on the CPU oracle, never on these kernels). Integer stages and the noise generator must match exactly; float stages
obey |got - model| <= K u (A + |model|).

Everything goes through the C-ABI as the host hands it over: LFCoefficients.dequantLFCoeff and Frame.setLFGroupQuant, performUpsampling
and ResidentPlanes.upsample, initializeNoise / synthesizeNoise and ResidentPlanes.noise, modularToFloat, the ModularChannel squeeze
steps, rct and ModularStream plans under every form the plan runner has."""
import numpy as np
import pytest

import pixel_ref64 as M
import pixel_ref64_cases as C
import test_pixel_ref64_cpu as T
from jxlatte_amd import abi, host, synth

pytestmark = pytest.mark.gpu
F = np.float32
K = T.K


# ---- LF stage ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ep,mul", C.LF_CASES, ids=["%dx%d-ep%d-x%d" % (s + (e, m)) for s, e, m in C.LF_CASES])
def test_lf_stage(ctx, shape, ep, mul):
    a = C.LF_ARGS
    T.lf_check(lambda q, sd, ep, smooth: host.LFCoefficients.dequantLFCoeff(
        ctx, q, sd, ep, a["x_factor_lf"], a["b_factor_lf"], smooth, a["base_corr_x"], a["base_corr_b"], a["color_factor"]), shape, ep, mul)


def test_lf_stage_inside_a_frame(ctx):
    """Frame.setLFGroupQuant on a frame of two LF groups (256 and 3 cells wide): the device runs the LF stage of each group on its own
    and writes into the frame-level LF planes; DCT8 blocks without HF coefficients hand every cell's LF sample to its 64 pixels"""
    fr, lfq = T.lf_frame()
    p = abi.VarDCTParams.from_buffer_copy(fr["params"])
    p.stages = 1
    f = host.Frame(ctx, p, fr["weights"], fr["woffs"])
    for g, q in zip(fr["lfgroups"], lfq):
        f.setLFGroup(dict(g, lf=None))
        f.setLFGroupQuant(g["lfg_y"], g["lfg_x"], q, C.lf_sd(T.LF_FRAME["mul"]), T.LF_FRAME["ep"], T.LF_FRAME["x_factor_lf"],
                          T.LF_FRAME["b_factor_lf"], True)
    for grp in range(synth.num_groups(fr)):
        f.putGroup(0, grp, synth.group_view(fr, grp))
    T.ratio(f.decodeFrame(), *T.lf_frame_model(fr, lfq), "LF stage inside a frame", K["lf_frame"])


# ---- k-times upsampling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.UP_SHAPES, ids=["%dx%d" % s for s in C.UP_SHAPES])
@pytest.mark.parametrize("k", C.UP_KS)
def test_upsampling(ctx, k, shape):
    T.up_check(lambda plane, k, wts: host.performUpsampling(ctx, plane, k, wts), k, shape)


@pytest.mark.parametrize("k", C.UP_KS)
def test_upsampling_of_resident_planes(ctx, k):
    """the three runs of the 37 x 50 case as the three resident planes (each run brings its own weights: one upload per run)"""
    for name, plane, packed in C.up_runs(k, (37, 50)):
        wts = M.up_weights(k, packed)
        planes = np.stack([plane, plane[::-1].copy(), plane[:, ::-1].copy()])
        rp = host.ResidentPlanes.upload(ctx, planes)
        rp.upsample(k, wts.astype(F))
        got = rp.download()
        assert got.shape == (3, 37 * k, 50 * k)
        for c in range(3):
            x, a, _ = M.upsample(planes[c], k, wts)
            T.ratio(got[c], x, a, "resident upsampling k = %d %s plane %d" % (k, name, c), K["upsample"])


# ---- noise ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,gd,colors", C.NOISE_INIT)
def test_noise_init(ctx, h, w, gd, colors):
    run = lambda *a: host.initializeNoise(ctx, *a)  # noqa: E731
    T.noise_init_check(run, h, w, gd, colors)
    T.noise_bits_check(run, h, w, gd, colors)


@pytest.mark.parametrize("bcx,bcb", C.NOISE_ADD_CORR)
def test_noise_add(ctx, bcx, bcb):
    T.noise_add_check(lambda *a: host.synthesizeNoise(ctx, *a), bcx, bcb)


def test_noise_of_resident_planes(ctx):
    """ResidentPlanes.noise = initializeNoise + synthesizeNoise on the device: the model's two stages chained. The noise the kernel adds
    is its own float32 high-pass result, the model's is exact; the difference enters the sum scaled by at most 0.22 and is covered by
    the companion of the noise-add bound (which carries |noise|) with the K of the high-pass added."""
    p, _, lut = C.noise_add_inputs()
    h, w = p.shape[1:]
    seed = C.noise_seed(h, w)
    nz, na, _ = M.noise_init(h, w, seed, 16, 3)
    for bcx, bcb in C.NOISE_ADD_CORR:
        rp = host.ResidentPlanes.upload(ctx, p)
        rp.noise(16, seed, lut, bcx, bcb)
        x, a, _ = M.noise_add(p, nz, lut, bcx, bcb)
        _, a_hi, _ = M.noise_add(p, na, lut, bcx, bcb)  # the companion with the high-pass's own companion in place of |noise|
        T.ratio(rp.download(), x, np.maximum(a, a_hi), "resident noise (%g, %g)" % (bcx, bcb), K["noise_add"] + K["noise_conv"])


# ---- modularToFloat, squeeze steps, RCT ------------------------------------------------------------------------------------------------
def test_modular_to_float(ctx):
    T.to_float_check(lambda a, b, scale: host.modularToFloat(ctx, a, b, scale))


def test_inverse_squeeze_steps(ctx):
    T.squeeze_check(lambda a, r: host.ModularChannel.inverseHorizontalSqueeze(ctx, a, r),
                    lambda a, r: host.ModularChannel.inverseVerticalSqueeze(ctx, a, r))


@pytest.mark.parametrize("rct_type", range(42))
def test_rct(ctx, rct_type):
    v = C.rct_planes(rct_type)
    T.same(host.rct(ctx, v, rct_type), M.rct(v, rct_type), "rct %d" % rct_type)


# ---- plans -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_models():
    """every plan's model result, computed once"""
    plain = {name: M.apply_transforms(chans, sp) for name, chans, sp in T.plan_inputs()}
    with_rct = {name: M.apply_transforms(chans, sp, t, b) for name, chans, sp, t, b in T.rct_plan_inputs()}
    one_step = {}
    a, r = C.adversarial()
    for name, avg, res in [("adversarial", a, r), ("extremes",) + C.squeeze_extremes()[2]]:
        one_step[name, True] = ([avg, res], M.inv_hsqueeze(avg, res))
        at, rt = np.ascontiguousarray(avg.T), np.ascontiguousarray(res.T)
        one_step[name, False] = ([at, rt], M.inv_vsqueeze(at, rt))
    return plain, with_rct, one_step


def run_plans(ctx, plan_models):
    plain, with_rct, one_step = plan_models
    for name, chans, sp in T.plan_inputs():
        T.same_list(host.ModularStream(ctx, chans, sp).applyTransforms(), plain[name], name)
    for name, chans, sp, t, b in T.rct_plan_inputs():
        T.same_list(host.ModularStream(ctx, chans, sp, rctType=t, rctBegin=b).applyTransforms(), with_rct[name], name)
    for (name, horizontal), (chans, exp) in one_step.items():  # one step through the plan runner: the segmented walk, checked and redone
        out = host.ModularStream(ctx, chans, [(1 if horizontal else 0, 1, 0, 1)]).applyTransforms()
        T.same_list(out, [exp], "%s %s" % (name, "H" if horizontal else "V"))


PLAN_FORMS = [("default", {}), ("walk", {"JXL_HSQUEEZE_WALK_MAX": str(1 << 40)}), ("lds", {"JXL_HSQUEEZE_WALK_MAX": "0"}),
              ("cw16", {"JXL_VH_CW": "16"}), ("cw32", {"JXL_VH_CW": "32"}), ("no_vh", {"JXL_SQUEEZE_NO_VH": "1"}),
              ("speculate1", {"JXL_SQUEEZE_SPECULATE": "1"}), ("speculate0", {"JXL_SQUEEZE_SPECULATE": "0"})]
PLAN_SWITCHES = ("JXL_HSQUEEZE_WALK_MAX", "JXL_VH_CW", "JXL_SQUEEZE_NO_VH", "JXL_SQUEEZE_SPECULATE")


@pytest.mark.parametrize("form", PLAN_FORMS, ids=[f[0] for f in PLAN_FORMS])
def test_plans(ctx, plan_models, form, monkeypatch):
    """the default plans, the V+H pairs, the RCT at rctBegin 0..2 and the never-forgetting rows under both H kernels, both chunk widths
    of the pair kernel, without the pair kernel, and with the segment checks inside the next launch, on a side stream and in order"""
    for name in PLAN_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, val in form[1].items():
        monkeypatch.setenv(name, val)
    run_plans(ctx, plan_models)
