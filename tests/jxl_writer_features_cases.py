"""Seeded streams whose frames hold patches, splines or both -- inside a VarDCT frame, and splines and noise inside a Modular one --
for tests/jxl_writer_vardct.py and tests/jxl_writer.py, and what a decoder must make of them, computed from the SOURCE alone: never
through jxlatte_amd or oracle/.

A case is dict(image, frames): the image header's dict and the frames, each a SOURCE dict of jxl_writer_vardct or a frame dict of
jxl_writer (one with "planes"). models(name) walks the frames as JXLCodestreamDecoder.java:599-658 does and extends
jxl_writer_vardct_cases.tail_model's order to: the frame's planes on its bounds (vardct_ref64.decode, or the lossy cases' model of a
Modular frame), upsample, the slot saved before the colour transform (:630-633), PATCHES (:634), SPLINES (:635), noise (:636), inverse XYB
(:637), the blend onto the canvas (a full REPLACE frame: the crop to the image), the slot saved after the colour transform, which is
the canvas (:656-657). Every step carries (x, a), the float64 planes and their magnitude companion.

  * patches: float64, by the blend formulas of JXLCodestreamDecoder.java:285-413 as blendBuffers reaches them with patch == true
    (:466-486). The images here have no extra channel, and without one every patch mode the reference accepts stores
    frame + reference: raw mode 2 is blendAdd, raw 3 and 4 become BLEND and MULADD, which hand over to blendAdd where there is no
    extra channel (:346-349, :384-387); raw mode 1 ("replace") reaches the switch's default and throws (:510-511), so no case holds it;
    mode 0 draws nothing (:241-242). The companion of a sum is the sum of the companions. patch_check(name) runs
    patches_model.compute_patches on the float32 roundings of the same planes: the two must agree to float32 rounding.
  * splines: spline_model64.render at the UPSAMPLED bounds (Frame.java:729-730 changes the header's bounds object), with the frame's
    base correlations (a Modular frame has the defaults, LFGlobal.java:79).
  * noise: the strength reads the planes after patches and splines; the seed is (visibleFrames << 32) | invisibleFrames at the frame.

Conditions, checked on the models alone when a case is built (a violating draw is made again with the next seed, 20 tries): no
undecided spline decision (spline_model64), splines touch between 2 % and 60 % of the frame's samples, patches cover between 5 % and
60 %, and the earlier ones -- no EPF-undecided cell, the clamped share of an upsampled frame within 0.5 % - 50 %, noise inputs on both
clamps and in at least five LUT segments. Observed (test_cases_are_what_they_claim prints them):
splines touch: splines_40x40 45.9 %, splines_264x264 7.5 %, splines_one_point 30.8 %, splines_quant_adjust_pos 23.6 % / _neg 53.2 %,
splines_corr 56.6 %, splines_up2_19x15_of_37x29 35.9 %, splines_noise_40x40 28.8 %, splines_epf3_gab 55.9 %, patches_alpha_blend 16.6 %,
patches_splines_noise_72x64 8.7 %, mod_rgb8_splines_33x29 45.6 %, mod_xyb_splines_noise_40x24 33.3 %; patches cover: patches_modref_72x64
12.1 %, patches_264x264 37.1 %, patches_alpha_blend 12.4 %, patches_vardct_ref 35.1 %, patches_ref_after_ct 31.7 %, patches_chain_40x40
39.6 % and 36.3 %, patches_up2 14.3 %, patches_splines_noise_72x64 14.5 %, patches_of_an_empty_slot_vardct 0 (nothing is drawn: the one
case outside the band); clamped outputs splines_up2_19x15_of_37x29 4.0 %, patches_up2 1.7 %, mod_rgb8_noise_up2 13.8 %; noise inputs
under 0 / at or over 7: splines_noise_40x40 1024 / 470 of 3200, patches_splines_noise_72x64 4185 / 4 of 9216,
mod_xyb_splines_noise_40x24 725 / 80 of 1920, mod_rgb8_noise_up2 625 / 490 of 2280, all seven segments in each.

`wrong=` makes the WRONG expectations of test_jxl_writer_features_cpu.py (WRONG names them)."""
import functools

import numpy as np

import jxl_writer as W
import jxl_writer_lossy_cases as LC
import jxl_writer_vardct as V
import jxl_writer_vardct_cases as VC
import pixel_ref64 as P
import spline_model64 as SM
import vardct_ref64 as M

F = np.float32
WRONG = ("patches after splines", "overlapping positions applied in reverse", "splines after noise", "splines at the frame's size under upsampling",
         "every spline with its own coefficients", "the slot taken after the colour transform", "the slot taken before the colour transform",
         "a reference frame saved after its own patches", "positions as (y, x)", "invQa of the other branch", "MathHelper.max as a true maximum", "the first spline's start as (y, x)")


def is_modular(fr):
    return "planes" in fr


# ---- drawing ----------------------------------------------------------------------------------------------------------------------
def clusters(rng, n_ctx, k):
    """a cluster map of n_ctx contexts on k clusters that all exist, and k different configurations"""
    m = rng.integers(0, k, n_ctx)
    m[rng.permutation(n_ctx)[:k]] = np.arange(k)
    return m.tolist(), [W.CONFIGS[i] for i in rng.permutation(len(W.CONFIGS))[:k]]


def spline_coeff(rng, amp=8, sigma0=(3, 4), sigma_terms=1):
    """X, Y, B on the first eight coefficients, within +-amp; sigma about sigma0 / 3 with `sigma_terms` small terms beyond index 0, too
    small to bring it to 0"""
    c = np.zeros((4, 32), np.int64)
    c[:3, :8] = rng.integers(-amp, amp + 1, (3, 8))
    c[3, 0] = rng.integers(sigma0[0], sigma0[1] + 1)
    c[3, 1:1 + sigma_terms] = rng.choice([-1, 1], sigma_terms)
    return c.tolist()


def walk(rng, start, k, step):
    """k control points (x, y): a start and steps of at most `step` on either axis, no point repeated"""
    pts = [start]
    while len(pts) < k:
        d = (int(rng.integers(-step, step + 1)), int(rng.integers(-step, step + 1)))
        if abs(d[0]) + abs(d[1]) >= 3:
            pts.append((pts[-1][0] + d[0], pts[-1][1] + d[1]))
    return pts


def spline_set(rng, width, height, counts, step=12, quant_adjust=0, starts=None, **coeff):
    out = []
    for i, k in enumerate(counts):
        start = starts[i] if starts else (int(rng.integers(4, width - 4)), int(rng.integers(4, height - 4)))
        out.append(dict(control=walk(rng, start, k, step), coeff=spline_coeff(rng, **coeff)))
    assert min(out[0]["control"][0]) >= 0  # SplinesBundle.java:29-30: the first start position is two raw symbols
    return dict(quant_adjust=quant_adjust, splines=out, clusters=clusters(rng, 6, int(rng.integers(3, 6))))


def patch_set(rng, ref, ref_w, ref_h, frame_w, frame_h, sizes=((12, 10), (9, 14), (16, 7))):
    """3 patches and 7 positions: raw modes 2, 3 and 4 (3 and 4 with and without clamp) and 0 on some positions; the first two
    positions of the first patch overlap; the last position of the last patch touches the frame's last row and column"""
    out = []
    modes = ([dict(mode=2), dict(mode=3, clamp=True)], [dict(mode=3, clamp=False), dict(mode=0), dict(mode=4, clamp=True)],
             [dict(mode=4, clamp=False), dict(mode=2)])
    for i, (w, h) in enumerate(sizes):
        x0, y0 = int(rng.integers(0, ref_w - w + 1)), int(rng.integers(0, ref_h - h + 1))
        pos = [(int(rng.integers(0, frame_w - w + 1)), int(rng.integers(0, frame_h - h + 1))) for _ in modes[i]]
        if i == 0:
            pos[1] = (min(pos[0][0] + 5, frame_w - w), min(pos[0][1] + 4, frame_h - h))
        if i == 2:
            pos[1] = (frame_w - w, frame_h - h)
        out.append(dict(ref=ref, x0=x0, y0=y0, width=w, height=h, positions=pos, blend=[[m] for m in modes[i]]))
    return out


def modref(rng, w=24, h=20, slot=1):
    """a reference-only Modular XYB frame saved before the colour transform"""
    return dict(planes=LC.xyb_planes(rng, h, w), type=W.REFERENCE_ONLY, save_as_reference=slot, save_before_ct=True, restoration={})


def _single(src):
    return dict(image=V.image_of(src), frames=[src])


def splines_case(seed, width, height, counts=(2, 3, 5), up=1, image=None, step=12, quant_adjust=0, starts=None, coeff=None, **opt):
    rng = np.random.default_rng(seed)
    sp = spline_set(rng, width * up, height * up, counts, step, quant_adjust, starts, **(coeff or {}))
    if up > 1:
        opt.update(upsampling=up)
    if image:
        opt.update(image_width=image[0], image_height=image[1])
    return _single(VC.draw(seed, width, height, splines=sp, **opt))


def splines_264(seed):
    """2 x 2 groups; control points outside all four edges, a later spline with a negative start, one across the centre"""
    rng = np.random.default_rng(seed)
    j = lambda: int(rng.integers(-3, 4))  # noqa: E731
    paths = [[(5 + j(), 120 + j()), (-12 + j(), 140 + j())], [(-8 + j(), -6 + j()), (40 + j(), 30 + j())],
             [(250 + j(), 100 + j()), (275 + j(), 130 + j())], [(100 + j(), 250 + j()), (130 + j(), 280 + j())],
             [(120 + j(), 10 + j()), (140 + j(), -15 + j())], [(100 + j(), 100 + j()), (160 + j(), 150 + j()), (140 + j(), 128 + j()), (200 + j(), 60 + j())]]
    sp = dict(quant_adjust=0, splines=[dict(control=p, coeff=spline_coeff(rng, sigma0=(4, 6))) for p in paths], clusters=clusters(rng, 6, 4))
    return _single(VC.draw(seed, 264, 264, allowed=VC.MID_TYPES, density=0.03, splines=sp))


def one_point(seed):
    rng = np.random.default_rng(seed)
    sp = spline_set(rng, 40, 40, (3, 1, 4))
    return _single(VC.draw(seed, 40, 40, splines=sp))


def patches_case(seed, width, height, ref_frame="modular", up=1, splines=False, slot=1, before_ct=True, empty=False, **opt):
    rng = np.random.default_rng(seed)
    fw, fh = width * up, height * up
    if up > 1:
        opt.update(upsampling=up)
    extra = {}
    if splines:
        extra["splines"] = spline_set(rng, fw, fh, (2, 4))
    big = fw > 256
    if ref_frame == "modular":
        rw, rh = (120, 100) if big else (24, 20)
        first = modref(rng, rw, rh, slot)
    else:
        first = VC.draw(seed + 7, 40, 40, is_last=False, save_as_reference=slot, save_before_ct=before_ct) if not empty else None
        rw, rh = 40, 40
    if big:  # positions in all four groups and across the group lines
        patches = patch_set(rng, slot, rw, rh, fw, fh, ((100, 90), (60, 80), (110, 40)))
        patches[0]["positions"] = [(160, 20), (164, 24)]
        patches[1]["positions"] = [(20, 180), (200, 184), (180, 100)]
        patches[2]["positions"] = [(100, 100), (fw - 110, fh - 40)]
    else:
        patches = patch_set(rng, 3 if empty else slot, rw, rh, fw, fh)
    src = VC.draw(seed, width, height, patches=patches, patch_clusters=clusters(rng, 10, int(rng.integers(4, 7))), **extra, **opt)
    frames = [src] if first is None else [first, src]
    return dict(image=V.image_of(src), frames=frames)


def chain_case(seed):
    """three frames: a Modular reference frame (slot 1), a VarDCT frame that patches from it and is saved before the colour transform
    (slot 2: its planes BEFORE its own patches, JXLCodestreamDecoder.java:630-634), and a last frame that patches from slot 2"""
    rng = np.random.default_rng(seed)
    mid = VC.draw(seed + 7, 40, 40, is_last=False, save_as_reference=2, save_before_ct=True, patches=patch_set(rng, 1, 24, 20, 40, 40),
                  patch_clusters=clusters(rng, 10, 4))
    last = VC.draw(seed, 40, 40, patches=patch_set(rng, 2, 40, 40, 40, 40), patch_clusters=clusters(rng, 10, 5))
    return dict(image=V.image_of(last), frames=[modref(rng), mid, last])


def alpha_blend_case(seed):
    """one alpha channel in both frames. The first application is an ADD (raw mode 2, which IS BlendingInfo's BLEND: its casts make
    the two alpha planes float, JXLCodestreamDecoder.java:446-455, and every later one finds them so); then BLEND on the colours and on
    the alpha (raw 3), an overlapping BLEND that leaves the alpha alone, MULADD (raw 4), and a position that blends the alpha only"""
    rng = np.random.default_rng(seed)
    ref = modref(rng)
    ref["planes"] = ref["planes"] + [rng.integers(1, 256, (20, 24))]  # (no 0: BLEND divides by the combined alpha, :375)
    alpha = rng.integers(0, 256, (64, 72))
    bx, by = int(rng.integers(0, 50)), int(rng.integers(0, 45))
    p0 = dict(ref=1, x0=3, y0=2, width=12, height=10, positions=[(int(rng.integers(0, 60)), int(rng.integers(0, 54))), (bx, by), (bx + 5, by + 4)],
              blend=[[dict(mode=2), dict(mode=0)], [dict(mode=3, clamp=True), dict(mode=3, clamp=False)], [dict(mode=3, clamp=False), dict(mode=0)]])
    dx, dy = int(rng.integers(0, 63)), int(rng.integers(0, 50))
    p1 = dict(ref=1, x0=10, y0=4, width=9, height=14, positions=[(dx, dy), (63, 50)],
              blend=[[dict(mode=4, clamp=True), dict(mode=0)], [dict(mode=0), dict(mode=3, clamp=True)]])
    src = VC.draw(seed, 72, 64, extra=[dict(bits=8, alpha_associated=False, plane=alpha, upsampling=1)], patches=[p0, p1],
                  patch_clusters=clusters(rng, 10, 5),
                  splines=spline_set(rng, 72, 64, (2, 4), starts=[(bx + 6, by + 5), (dx + 4, dy + 7)]))  # (a spline starts inside each)
    return dict(image=V.image_of(src), frames=[ref, src])


def modular_case(seed, width, height, xyb, splines=True, noise=False):
    rng = np.random.default_rng(seed)
    # (with noise: an X channel of +-2.2 puts the strength's inputs, 3 (Y +- X), on both sides of [0, 7))
    planes = LC.xyb_planes(rng, height, width, x=(0, 9000) if noise else (40, 6)) if xyb else LC.int_planes(rng, height, width, 8, 3)
    fr = dict(planes=planes, restoration={})
    if splines:
        fr["splines"] = spline_set(rng, width, height, (2, 3), step=10, amp=8 if xyb else 3)
    if noise:
        fr["noise"] = list(VC.NOISE_LUT)
    return dict(image=dict(width=width, height=height, bits=8, xyb=xyb), frames=[fr])


def modular_noise_up_case(seed, width, height, up):
    """integer RGB, noise, upsampling: Frame.upsample casts the integers (Frame.java:228), the noise stage finds them float and draws
    at the upsampled size. The strength reads 3 (G + R) and 3 (G - R) (Frame.java:801-804), and samples within the depth's range keep
    3 (G + R) under 7; the Modular stream holds any integer, so R and G run from 0 to 1.3 of the range: smooth ramps across the
    frame, so that few of the upsampled samples are clamped"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    ramp = lambda u, t: 0.65 + 0.65 * np.sin(u / rng.uniform(5.0, 8.0) + t / rng.uniform(6.0, 9.0) + rng.uniform(0.0, 6.0))  # noqa: E731
    planes = [np.rint(255 * f + rng.uniform(-1.0, 1.0, (height, width))).astype(np.int64) for f in (ramp(x, y), ramp(y, x), 0.5 + 0 * ramp(x, y))]
    fr = dict(planes=planes, restoration={}, upsampling=up, noise=list(VC.NOISE_LUT))
    return dict(image=dict(width=width * up, height=height * up, bits=8, xyb=False), frames=[fr])


NOISE = VC.NOISE_FIELD
CORR = dict(colour_factor=100, base_x=float(np.float16(0.05)), base_b=float(np.float16(0.9)), x_factor_lf=140, b_factor_lf=100)
MAKERS = {
    "splines_40x40": (functools.partial(splines_case, width=40, height=40), 201),
    "splines_264x264": (splines_264, 202),
    "splines_one_point": (one_point, 203),
    "splines_quant_adjust_pos": (functools.partial(splines_case, width=40, height=40, quant_adjust=5), 204),
    "splines_quant_adjust_neg": (functools.partial(splines_case, width=40, height=40, quant_adjust=-7), 205),
    "splines_corr": (functools.partial(splines_case, width=40, height=40, corr=CORR, coeff=dict(sigma0=(5, 6), sigma_terms=3)), 206),
    "splines_up2_19x15_of_37x29": (functools.partial(splines_case, width=19, height=15, up=2, image=(37, 29), counts=(2, 3), step=9), 207),
    "splines_noise_40x40": (functools.partial(splines_case, width=40, height=40, coeff=dict(amp=2), **NOISE), 208),
    "splines_epf3_gab": (functools.partial(splines_case, width=40, height=40, **dict(VC._restoration(3), gab=True)), 209),
    "patches_modref_72x64": (functools.partial(patches_case, width=72, height=64), 210),
    "patches_264x264": (functools.partial(patches_case, width=264, height=264, allowed=VC.MID_TYPES, density=0.03), 211),
    "patches_alpha_blend": (alpha_blend_case, 220),
    "patches_vardct_ref": (functools.partial(patches_case, width=40, height=40, ref_frame="vardct", slot=2), 212),
    "patches_ref_after_ct": (functools.partial(patches_case, width=40, height=40, ref_frame="vardct", slot=1, before_ct=False), 213),
    "patches_of_an_empty_slot_vardct": (functools.partial(patches_case, width=40, height=40, ref_frame="vardct", empty=True), 214),
    # what a frame saved before the colour transform holds when it has patches itself
    "patches_chain_40x40": (chain_case, 219),
    "patches_up2": (functools.partial(patches_case, width=36, height=32, up=2), 215),
    "patches_splines_noise_72x64": (functools.partial(patches_case, width=72, height=64, splines=True, **NOISE), 216),
    "mod_rgb8_splines_33x29": (functools.partial(modular_case, width=33, height=29, xyb=False), 217),
    "mod_xyb_splines_noise_40x24": (functools.partial(modular_case, width=40, height=24, xyb=True, noise=True), 218),
    "mod_rgb8_noise_up2": (functools.partial(modular_noise_up_case, width=19, height=15, up=2), 221),
}
NAMES = tuple(MAKERS)
VARDCT_NAMES = tuple(n for n in NAMES if not n.startswith("mod_"))


# ---- the expectation ---------------------------------------------------------------------------------------------------------------
def patch_stage(x, a, slots, patches, yx=False, reverse=False):
    """computePatches (JXLCodestreamDecoder.java:212-254), float64: see the module docstring. Planes past the third are the alpha
    channel (float: the first application's casts have happened, :446-465). reverse: every patch's positions last to first"""
    x, a = x.copy(), a.copy()
    alpha = x.shape[0] > 3
    covered = np.zeros(x.shape[1:], bool)
    for p in patches:
        slot = slots[p["ref"]]
        if slot is None:  # :225-226
            continue
        sx, sa = slot
        h, w, ry, rx = p["height"], p["width"], p["y0"], p["x0"]
        assert ry + h <= sx.shape[1] and rx + w <= sx.shape[2]  # :227-229
        todo = list(zip(p["positions"], p["blend"]))
        for (px, py), blend in (todo[::-1] if reverse else todo):
            if yx:
                px, py = py, px
            if yx and (py + h > x.shape[1] or px + w > x.shape[2]):  # (the wrong expectation: what falls outside is left out)
                continue
            assert py + h <= x.shape[1] and px + w <= x.shape[2]  # :233-237
            f, r = (slice(py, py + h), slice(px, px + w)), (slice(ry, ry + h), slice(rx, rx + w))
            mode = blend[0]["mode"]
            if alpha:  # the colours read the frame's alpha before channel 3 of this position changes it (:238)
                na, a_na, oa, a_oa = x[3][f], a[3][f], sx[3][r], sa[3][r]
                if blend[0].get("clamp", False):
                    na = np.clip(na, 0.0, 1.0)  # :367-368, :408-409
            if mode == 0:  # :241-242
                pass
            elif mode == 2 or not alpha:  # blendAdd (:285-326), and what BLEND and MULADD do without an extra channel (:346, :384)
                assert mode in (2, 3, 4, 6)  # (1 throws, :510-511)
                x[:3, f[0], f[1]] += sx[:3, r[0], r[1]]
                a[:3, f[0], f[1]] += sa[:3, r[0], r[1]]
            elif mode == 3:  # BLEND, alpha not associated (:374-375): old is the slot, new the frame (:487-488, :363-366)
                n, a_n, o, a_o = x[:3, f[0], f[1]], a[:3, f[0], f[1]], sx[:3, r[0], r[1]], sa[:3, r[0], r[1]]
                num, den = n * na + o * oa * (1.0 - na), oa + na * (1.0 - oa)
                a_num = a_n * np.abs(na) + np.abs(n) * a_na + (a_o * np.abs(oa) + np.abs(o) * a_oa) * np.abs(1.0 - na) + np.abs(o * oa) * a_na
                a_den = a_oa + a_na * np.abs(1.0 - oa) + np.abs(na) * a_oa
                x[:3, f[0], f[1]] = num / den
                a[:3, f[0], f[1]] = a_num / np.abs(den) + np.abs(num) / (den * den) * a_den
            else:  # MULADD (:405-410): slot + alpha * frame
                assert mode == 4
                n, a_n, o, a_o = x[:3, f[0], f[1]], a[:3, f[0], f[1]], sx[:3, r[0], r[1]], sa[:3, r[0], r[1]]
                x[:3, f[0], f[1]] = o + na * n
                a[:3, f[0], f[1]] = a_o + np.abs(na) * a_n + a_na * np.abs(n)
            if alpha and blend[1]["mode"] != 0:  # the alpha channel itself under BLEND (:369-370)
                assert blend[1]["mode"] == 3
                na2 = np.clip(x[3][f], 0.0, 1.0) if blend[1].get("clamp", False) else x[3][f]
                x[3][f] = oa + na2 * (1.0 - oa)
                a[3][f] = a_oa + a_na * np.abs(1.0 - oa) + np.abs(na2) * a_oa
            if mode != 0 or (alpha and blend[1]["mode"] != 0):
                covered[f] = True
    return x, a, covered


def alpha_pair(plane, bits=8):
    """ImageBuffer.castToFloat of an integer alpha plane: v * (1f / maxValue), one rounding"""
    v = np.asarray(plane, np.float64) * float(F(1) / F((1 << bits) - 1))
    return v, np.abs(v)


def _frame_planes(image, fr):
    """(x, a, params | None) of the frame on its bounds before Frame.upsample"""
    if is_modular(fr):
        im = dict(image, width=fr["planes"][0].shape[1], height=fr["planes"][0].shape[0], extra=[], frames=[dict(fr, planes=fr["planes"][:3])])
        x, a = LC.model(im)["epf"]
        if a is None:  # integer planes: the spline or noise stage casts them (Spline.java:182, Frame.java:796)
            pairs = [P.modular_to_float(x[c], None, F(1) / F((1 << image["bits"]) - 1)) for c in range(3)]
            x, a = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        return x, a, None
    p = VC.params_of(fr)
    x, a, undecided = M.decode(VC.model_frame(fr, params=p), VC.EPF_STAGES)
    h, w = VC.frame_bounds(fr)
    return x[:, :h, :w], a[:, :h, :w], p


def models(case, wrong=None):
    """-> dict(frames=[dict(epf, pre, at, final, figures)], slots=[(x, a) | None] * 4 at the end, image=(x, a), undecided=[..])"""
    assert wrong is None or wrong in WRONG
    image = case["image"]
    ih, iw = image["height"], image["width"]
    slots, canvas, out, undecided = [None] * 4, None, [], []
    visible = invisible = 0
    for fr in case["frames"]:
        modular = is_modular(fr)
        x, a, p = _frame_planes(image, fr)
        m = dict(epf=(x, a), figures={})
        if image.get("extra"):  # one alpha channel of the frame's size: the fourth plane from here on
            assert len(image["extra"]) == 1 and fr.get("upsampling", 1) == 1
            ax, aa = alpha_pair(fr["planes"][3] if modular else fr["extra"][0]["plane"])
            x, a = np.concatenate([x, ax[None]]), np.concatenate([a, aa[None]])
        ftype = fr.get("type", W.REGULAR)
        normal = ftype in (W.REGULAR, W.SKIP_PROGRESSIVE)
        is_last = fr.get("is_last", True) if normal else False
        save = not is_last  # JXLCodestreamDecoder.java:620-621 (duration 0)
        if normal and is_last:  # :622-627
            visible, invisible = visible + 1, 0
        else:
            invisible += 1
        k = fr.get("upsampling", 1)
        if k > 1:  # (a Modular frame's integers are cast first, Frame.java:228; it has the default weights)
            h, w = x.shape[1:]
            x, a, cl = VC.upsample_model(x, a, k, VC.packed_up_weights(fr, k))
            x, a, cl = x[:, :h * k, :w * k], a[:, :h * k, :w * k], cl[:, :h * k, :w * k]
            m["figures"]["clamped"] = float(cl.mean())
        before = (x.copy(), a.copy())
        m["pre"] = before
        if save and fr.get("save_before_ct", False) and wrong != "the slot taken after the colour transform":
            slots[fr.get("save_as_reference", 0)] = before  # :630-633: before the frame's own patches
        bx, bb = (float(p.base_corr_x), float(p.base_corr_b)) if p is not None else (0.0, 1.0)  # LFGlobal.java:79

        def splines(x, a):
            if not fr.get("splines"):
                return x, a
            sh, sw = x.shape[1:]
            kw = {}
            if wrong == "splines at the frame's size under upsampling":
                sh, sw = sh // k, sw // k
            if wrong == "every spline with its own coefficients":
                kw["own_coeffs"] = True
            if wrong == "invQa of the other branch":
                kw["other_branch"] = True
            if wrong == "MathHelper.max as a true maximum":
                kw["true_max"] = True
            sp = fr["splines"]
            if wrong == "the first spline's start as (y, x)":
                sp = dict(sp, splines=[dict(s, control=[c[::-1] for c in s["control"]]) for s in sp["splines"]])
            sx, sa, und = SM.render(sp, bx, bb, sh, sw, **kw)  # (three planes: Spline.java:180)
            if wrong is None:
                undecided.extend(und)
                m["figures"]["splines touch"] = float((sa.sum(0) > 0).mean())
            x, a = x.copy(), a.copy()
            x[:3, :sh, :sw] += sx
            a[:3, :sh, :sw] += sa
            return x, a

        def patches(x, a):
            if not fr.get("patches"):
                return x, a
            x, a, cov = patch_stage(x, a, slots, fr["patches"], yx=wrong == "positions as (y, x)",
                                    reverse=wrong == "overlapping positions applied in reverse")
            if wrong is None:
                m["figures"]["patches cover"] = float(cov.mean())
            return x, a

        def noise(x, a):
            if fr.get("noise") is None:
                return x, a
            assert x.shape[0] == 3
            lut = np.asarray(fr["noise"], np.float64) / 1024.0  # LFGlobal.java:58
            nz, na, _ = P.noise_init(x.shape[1], x.shape[2], (visible << 32) | invisible, V.GROUP_DIM)
            y, _, _ = P.noise_add(x, nz, lut, bx, bb)
            _, mag, _ = P.noise_add(x, na, lut, bx, bb)
            v = 3.0 * np.stack([x[1] + x[0], x[1] - x[0]])  # Frame.java:801-804
            if wrong is None:
                m["figures"].update(below=int((v < 0).sum()), above=int((v >= 7.0).sum()),
                                    segments=sorted(set(np.floor(v[(v >= 0) & (v < 7.0)]).astype(int).tolist())))
            return y, mag + a
        order = [patches, splines, noise]
        if wrong == "patches after splines":  # (told apart only where a patch does more than add: the alpha case)
            order = [splines, patches, noise]
        elif wrong == "splines after noise":  # (the same planes as a noise strength read before the splines)
            order = [patches, noise, splines]
        m["at"] = {}  # the planes in front of each stage
        for stage in order:
            m["at"][stage.__name__] = (x, a)
            x, a = stage(x, a)
            if stage is patches and save and fr.get("save_before_ct", False) and wrong == "a reference frame saved after its own patches":
                slots[fr.get("save_as_reference", 0)] = (x.copy(), a.copy())
        rest = (x[3:], a[3:])
        x, a = x[:3], a[:3]
        if image.get("xyb", False):
            if p is None:
                bias = [F(LC.OPSIN_BIAS)] * 3
                x, a = M.xyb(x, a, [F(v) for v in LC.DEFAULT_OPSIN], bias, [F(np.cbrt(np.float64(b))) for b in bias], 255.0)
            else:
                x, a = M.xyb(x, a, p.opsin_matrix, p.opsin_bias, p.cbrt_opsin_bias, float(p.intensity_target))
        x, a = np.concatenate([x, rest[0]]), np.concatenate([a, rest[1]])
        m["final"] = (x, a)
        if normal:  # :644-655 a full REPLACE frame at the origin: the canvas is its crop to the image
            canvas = (x[:, :ih, :iw], a[:, :ih, :iw])
        if (save and not fr.get("save_before_ct", False)) or (save and wrong == "the slot taken after the colour transform"):
            slots[fr.get("save_as_reference", 0)] = canvas  # :656-657
            if wrong == "the slot taken before the colour transform":
                slots[fr.get("save_as_reference", 0)] = before
        out.append(m)
    return dict(frames=out, slots=slots, image=canvas, undecided=undecided)


def conditions(case, m=None):
    """the reason a draw is unfit, or None. m: the case's models, where they are at hand"""
    for fr in case["frames"]:
        if not is_modular(fr):
            why = VC.conditions({k: v for k, v in fr.items() if k not in ("upsampling", "noise")})  # (the tail's are checked below)
            if why is not None:
                return why
    m = m or models(case)
    if m["undecided"]:
        return "an undecided spline decision: " + m["undecided"][0]
    for f in m["frames"]:
        g = f["figures"]
        if "splines touch" in g and not 0.02 <= g["splines touch"] <= 0.60:
            return "splines touch %.1f %%" % (100 * g["splines touch"])
        if "patches cover" in g and not (0.05 <= g["patches cover"] <= 0.60 or g["patches cover"] == 0.0):
            return "patches cover %.1f %%" % (100 * g["patches cover"])
        if "clamped" in g and not 0.005 <= g["clamped"] <= 0.5:
            return "%.2f %% of the upsampled outputs clamped" % (100 * g["clamped"])
        if "below" in g and not (g["below"] > 0 and g["above"] > 0 and len(g["segments"]) >= 5):
            return "the noise strength's inputs miss a clamp or reach %d LUT segments" % len(g["segments"])
    return None


_built, _bytes, _models = {}, {}, {}


def case(name):
    if name not in _built:
        make, seed = MAKERS[name]
        for k in range(20):
            c = make(seed + 1000 * k)
            m = models(c)
            why = conditions(c, m)
            if why is None:
                _models[name, None] = m
                break
        else:
            raise AssertionError("no fit draw of %s: %s" % (name, why))
        _built[name] = c
    return _built[name]


def encoded(name, variant=None):
    if (name, variant) not in _bytes:
        c = case(name)
        _bytes[name, variant] = V.encode_stream(c["image"], c["frames"], variant)
    return _bytes[name, variant]


def expected(name, wrong=None):
    if (name, wrong) not in _models:
        _models[name, wrong] = models(case(name), wrong)
    return _models[name, wrong]


def patch_check(name):
    """patches_model.compute_patches on the float32 roundings of the planes the float64 patch stage is given -- an alpha channel as
    the integers it is in the stream: the model's own casts make it float --, per frame with patches: [(float32 result
    [3 or 4][H][W], float64 result, companion)]"""
    import types

    import patches_model as PM
    from blend_ref import Buf
    c, out = case(name), []
    image = c["image"]
    extra = image.get("extra", [])
    info = types.SimpleNamespace(colour_space=0, num_extra=len(extra), ec_type=[0] * len(extra), ec_alpha_associated=[False] * len(extra),
                                 ec_bits=[8] * len(extra), bits_per_sample=image["bits"])

    def bufs(x, src):
        planes = [Buf(np.asarray(x[ch], F).copy()) for ch in range(3)]
        if extra:
            planes.append(Buf(np.asarray(src["planes"][3] if is_modular(src) else src["extra"][0]["plane"], np.int32).copy()))
        return planes
    slots, slot_src = [None] * 4, [None] * 4
    run = models(c)
    for fr, m in zip(c["frames"], run["frames"]):
        save = not (fr.get("is_last", True) if fr.get("type", 0) in (W.REGULAR, W.SKIP_PROGRESSIVE) else False)
        if save and fr.get("save_before_ct", False):
            slots[fr.get("save_as_reference", 0)], slot_src[fr.get("save_as_reference", 0)] = m["pre"], fr
        if fr.get("patches"):
            x, a = m["pre"]
            frame = bufs(x, fr)
            ref = [None if s is None else bufs(s[0], slot_src[k]) for k, s in enumerate(slots)]
            pl = [dict(ref=p["ref"], y0=p["y0"], x0=p["x0"], h=p["height"], w=p["width"], positions=[(y, x_) for x_, y in p["positions"]],
                       blend=[[(b["mode"], 0, int(b.get("clamp", False))) for b in row] for row in p["blend"]]) for p in fr["patches"]]
            PM.compute_patches(info, None, pl, frame, ref)
            want, wa, _ = patch_stage(x, a, slots, fr["patches"])
            out.append((np.stack([np.asarray(b.a, F) for b in frame]), want, wa))
        if save and not fr.get("save_before_ct", False):
            assert not extra
            slots[fr.get("save_as_reference", 0)] = (m["final"][0][:, :image["height"], :image["width"]], m["final"][1][:, :image["height"], :image["width"]])
            slot_src[fr.get("save_as_reference", 0)] = fr
    return out


def frontend_splines(sp):
    """the SOURCE's splines in the shape frontend.Frontend.splines() hands them out: control points as (y, x)"""
    return [dict(quant_adjust=sp["quant_adjust"], control=[(y, x) for x, y in s["control"]], coeff=[list(c) for c in s["coeff"]])
            for s in sp["splines"]]


# the cases every wrong writer is shown on (each exercises the variant's branch)
VARIANT_CASES = {
    "spline_start_y_before_x": ("splines_40x40", "splines_264x264", "mod_rgb8_splines_33x29"),
    "spline_points_as_first_differences": ("splines_40x40", "splines_corr"),
    "spline_count_without_the_one": ("splines_40x40", "splines_one_point"),
    "quant_adjust_before_the_start_positions": ("splines_quant_adjust_pos", "splines_quant_adjust_neg", "splines_40x40"),
    "spline_coefficients_y_x_b_sigma": ("splines_40x40", "mod_xyb_splines_noise_40x24"),
    "splines_before_patches": ("patches_splines_noise_72x64",),
    "noise_before_splines": ("splines_noise_40x40", "patches_splines_noise_72x64", "mod_xyb_splines_noise_40x24"),
    "patch_position_differences_unsigned": ("patches_modref_72x64", "patches_264x264", "patches_up2"),
}
