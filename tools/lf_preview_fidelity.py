"""How close a VarDCT frame's LF image is to "the full decode, box-averaged 8 x 8" (profiles/lf_preview.md).

    python tools/lf_preview_fidelity.py [file.jxl ...]        (default: the VarDCT samples under tests/golden/samples)

CPU only. The full decode runs on the oracle backend with the frame's planes captured BEFORE the colour transform (the VarDCT
call once more with the XYB stage off); the LF image is pyoracle.lf_dequant per LF group of the front-end's integers, assembled
at the 256-cell pitch. Compared over whole cells: the LF cell against the float64 mean of the 8 x 8 block, in the frame's own
domain (XYB, or YCbCr for a frame that is not XYB) and, for an XYB image, in linear RGB after invertXYB (PSNR, peak 1.0).
tests/test_lf_preview_cpu.py holds the acceptance figures to this module's numbers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from jxlatte_amd import abi, frontend  # noqa: E402
from jxlatte_amd.decoder import FLAG_SKIP_ADAPTIVE_LF, FLAG_USE_LF_FRAME, JXLDecoder  # noqa: E402

F = np.float32


def lf_groups(fe, fr):
    """the frame's LF groups as backend.lf_image takes them, from the front-end's views"""
    adaptive = (fr.flags & (FLAG_SKIP_ADAPTIVE_LF | FLAG_USE_LF_FRAME)) == 0
    out = []
    for i in range(fr.num_lf_groups):
        g = fe.lfgroup(i)
        out.append(dict(lfg_y=i // fr.lf_group_cols, lfg_x=i % fr.lf_group_cols, lf_quant=g["lf_quant"], extra_precision=g["extra_precision"],
                        scaled_dequant=list(fr.scaled_dequant), x_factor_lf=fr.x_factor_lf, b_factor_lf=fr.b_factor_lf,
                        adaptive_smoothing=adaptive))
    return out


def compose(orc, groups, cells, base_corr_x, base_corr_b, color_factor):
    """the LF image before the colour transform: lf_dequant per LF group at a 256-cell pitch, cropped to `cells`"""
    rows, cols = -(-cells[0] // 256), -(-cells[1] // 256)
    full = np.zeros((3, rows * 256, cols * 256), F)
    for g in groups:
        lf = orc.lf_dequant(np.stack(g["lf_quant"]), g["scaled_dequant"], g["extra_precision"], g["x_factor_lf"], g["b_factor_lf"],
                            g["adaptive_smoothing"], base_corr_x, base_corr_b, color_factor)
        y, x = g["lfg_y"] * 256, g["lfg_x"] * 256
        full[:, y:y + lf.shape[1], x:x + lf.shape[2]] = lf
    return np.ascontiguousarray(full[:, :cells[0], :cells[1]])


def full_decode(data, backend):
    """(frame planes before the colour transform, cropped to the frame; the decoded JXLImage; the decoder)"""
    dec = JXLDecoder(data, backend=backend)
    got = {}
    orig = backend.vardct

    def vardct(params, weights, woffs, lfgroups, groups, **kw):
        groups = list(groups)
        want, xyb = params.stages, params.xyb
        params.stages, params.xyb = abi.STAGE_IDCT | abi.STAGE_GAB | abi.STAGE_EPF, 0
        got["pre"] = np.array(orig(params, weights, woffs, lfgroups, groups, **{k: v for k, v in kw.items() if k != "keep"}), copy=True)
        params.stages, params.xyb = want, xyb
        return orig(params, weights, woffs, lfgroups, groups, **kw)
    backend.vardct = vardct
    try:
        image = dec.decode()
    finally:
        del backend.vardct
    st = dec.stats[-1]
    return got["pre"][:, :st["height"], :st["width"]], image, dec


def block_means(planes):
    """float64 means of the whole 8 x 8 blocks of [3][h][w] planes: [3][h // 8][w // 8]"""
    p = np.asarray(planes, np.float64)
    hc, wc = p.shape[1] // 8, p.shape[2] // 8
    return p[:, :hc * 8, :wc * 8].reshape(3, hc, 8, wc, 8).mean(axis=(2, 4))


def psnr(a, b, peak=1.0):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse)


def measure(data, orc, backend, compose=compose):
    """dict: domain ("XYB" / "YCbCr"), range, max_abs, mean_abs (the frame's own domain, whole cells) and, for an XYB image whose
    orientation is 1, psnr_rgb of invertXYB(LF image) against the 8 x 8 means of the decoded linear RGB"""
    pre, image, dec = full_decode(data, backend)
    fe = frontend.Frontend(data)
    fe.set_lf_only(True)
    fr = fe.next_frame(backend.squeeze, backend.rct)
    info = fe.image
    cells = ((fr.height + 7) >> 3, (fr.width + 7) >> 3)
    lf = compose(orc, lf_groups(fe, fr), cells, fr.base_corr_x, fr.base_corr_b, fr.colour_factor)
    want = block_means(pre)
    hc, wc = want.shape[1:]
    diff = np.abs(lf[:, :hc, :wc].astype(np.float64) - want)
    out = dict(domain="XYB" if info.xyb_encoded else "YCbCr" if fr.do_ycbcr else "RGB", range=float(want.max() - want.min()),
               max_abs=float(diff.max()), mean_abs=float(diff.mean()), cells=(hc, wc), lf_groups=fr.num_lf_groups)
    if info.xyb_encoded and info.orientation == 1:
        rgb = orc.xyb(lf, *[list(v) for v in dec._opsin()], info.intensity_target)
        out["psnr_rgb"] = psnr(rgb[:, :hc, :wc], block_means(np.stack(image.getBuffer(copy=False)[:3])))
    return out


def main(argv):
    from oracle import pyoracle as orc
    from oracle.pybackend import OracleBackend
    orc.build()
    paths = argv or [os.path.join(ROOT, "tests", "golden", "samples", n + ".jxl") for n in ("bench", "lenna", "bbb", "white")]
    large = os.path.join(ROOT, "tests", "golden", "samples_large")
    if not argv and os.path.isdir(large):
        paths += sorted(os.path.join(large, n) for n in os.listdir(large) if n.endswith(".jxl"))
    print("| sample | LF groups | domain | range | max abs diff | mean abs diff | linear-RGB PSNR (dB) |\n|---|---|---|---|---|---|---|")
    for p in paths:
        with open(p, "rb") as f:
            data = f.read()
        be = OracleBackend()
        fe = frontend.Frontend(data)
        why = JXLDecoder.preview_rule(fe.image, fe.next_frame(be.squeeze, be.rct))
        if why is not None:
            print("| `%s` | | refused: %s | | | | |" % (os.path.basename(p), why))
            continue
        m = measure(data, orc, be)
        print("| `%s` | %d | %s | %.3f | %.3g (%.2g %%) | %.3g (%.2g %%) | %s |" % (
            os.path.basename(p), m["lf_groups"], m["domain"], m["range"], m["max_abs"], 100 * m["max_abs"] / m["range"] if m["range"] else 0,
            m["mean_abs"], 100 * m["mean_abs"] / m["range"] if m["range"] else 0, "%.1f" % m["psnr_rgb"] if "psnr_rgb" in m else "-"))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
