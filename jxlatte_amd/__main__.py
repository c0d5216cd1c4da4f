"""python -m jxlatte_amd in.jxl [out.png | out.pfm] -- the reference's CLI (J/JXLatte.java) on the MI355X back-end:
decodes a JPEG XL file (C++ front-end -> device library) and writes a PNG (HDR images as 16-bit BT.2100 PQ, like
--png-hdr=auto) or a PFM (the image's own float samples). Needs a GPU: there is no CPU fallback."""
import argparse
import sys
import time


def parser():
    ap = argparse.ArgumentParser(prog="python -m jxlatte_amd", description=__doc__)
    ap.add_argument("input")
    ap.add_argument("output", nargs="?")
    ap.add_argument("--format", choices=["png", "pfm"], default=None,
                    help="the output format; without it an output name ending in .pfm (any letter case) gives a PFM and EVERY "
                         "other name a PNG (the reference stops with 'Unable to determine output format' on an unknown "
                         "extension; that exit is not adopted). A PFM holds the image's own samples: the --png-* options "
                         "and --device-color are ignored for it")
    ap.add_argument("--png-hdr", choices=["auto", "yes", "no"], default="auto")
    ap.add_argument("--png-depth", type=int, default=-1)
    ap.add_argument("--info", action="store_true", help="print the image / frame headers and stop")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sparse-coeffs", action="store_true",
                    help="feed the HF coefficients as lists of non-zero entries (jxl_vardct_put_group_sparse); same pixels")
    ap.add_argument("--png-peak-detect", choices=["auto", "on", "off"], default="auto",
                    help="scale a PQ image by its peak when it is written as SDR: when the peak is below 1 / always / never")
    ap.add_argument("--device-color", action="store_true",
                    help="colour management of the PNG (linearise, primaries, peak, output transfer) as one device pass "
                         "(jxl_stage_color_convert); float samples within 1 ulp of the host path")
    ap.add_argument("--device-splines", action="store_true",
                    help="draw the splines on the device (jxl_planes_splines / jxl_stage_splines) instead of numpy on the host; "
                         "samples equal except where a float exp rounds the other way")
    ap.add_argument("--device-patches", action="store_true",
                    help="apply all patch positions of a frame in one kernel launch (jxl_planes_patches / jxl_stage_patches) instead "
                         "of one blend call per position and channel; same samples")
    ap.add_argument("--device-png", action="store_true",
                    help="from the coefficients to the PNG's samples on the device: a frame that is the whole image leaves its colour "
                         "planes there (JXLDecoder device_output), and colour management and sample packing are one kernel "
                         "(jxl_planes_png_samples / jxl_stage_png_samples); the same bytes as --device-color. With PFM output: "
                         "the PFM's samples in one kernel (jxl_planes_pfm_samples / jxl_stage_pfm_samples); the same bytes as "
                         "without it")
    ap.add_argument("--device-canvas", action="store_true",
                    help="keep the canvas and the reference frames of multi-frame images on the device and blend every frame in one "
                         "launch (JXLDecoder device_canvas; jxl_canvas_blend); the same samples. The image's colour planes stay on "
                         "the device where they are float: add --device-png to pack the samples there too")
    ap.add_argument("--draw-varblocks", action="store_true",
                    help="the reference's --draw-varblocks: tint every varblock of a VarDCT frame by its transform type and blacken "
                         "its top row and left column (Frame.drawVarblocks as one device pass: jxl_planes_varblocks on planes "
                         "that are on the device, jxl_stage_varblocks otherwise)")
    ap.add_argument("--device-palette", action="store_true",
                    help="undo the Palette transforms of the frame-level Modular stream on the device (JXLDecoder device_palette; "
                         "jxl_stage_palette) instead of in the front-end's loop; the same samples")
    ap.add_argument("--device-image", action="store_true",
                    help="back the decoded image by a device plane set, colours and extra channels of any type (JXLDecoder "
                         "device_image): a Modular frame that is the whole image goes up once and stays (jxl_canvas_from_modular), "
                         "and with --device-canvas the canvas set becomes the image; add --device-png so that the writers read "
                         "the set and only the file's samples come down. The same bytes")
    ap.add_argument("--device-frames", action="store_true",
                    help="with --device-canvas: a Modular frame reaches the blend as a plane set made from the Modular context "
                         "(JXLDecoder device_frames; jxl_canvas_from_modular, jxl_canvas_from_modular_up, jxl_canvas_take_planes): "
                         "its encoded channels go up once and nothing comes down. The same bytes")
    ap.add_argument("--device-patch-sets", action="store_true",
                    help="with --device-canvas and --device-patches: a frame with patches no longer lands the canvas; computePatches "
                         "runs on device plane sets (JXLDecoder device_patch_sets; jxl_canvas_patches, jxl_canvas_cast_planes): the "
                         "frame's planes go up once and no reference plane crosses the bus. The same bytes")
    ap.add_argument("--device-chains", action="store_true",
                    help="with --device-image or --device-frames: the frame-level transform chain of a Modular frame is one device "
                         "plan whatever it holds (JXLDecoder device_chains; jxl_modular_begin_chain) -- nested Palettes run as one "
                         "launch on the uploaded channels -- and with --device-frames a frame with patches stays a plane set "
                         "through the patch stage. The same bytes")
    ap.add_argument("--downsample", type=int, choices=[1, 8], default=1,
                    help="8: the image at 1:8 from the LF image of its VarDCT frame (JXLDecoder downsample; jxl_planes_from_lf / "
                         "jxl_stage_lf_image): no HF section is read, one launch makes the planes. A faithful thumbnail, not the "
                         "reference's pixels. An image whose frame does not qualify (JXLDecoder.preview_rule) stops with the reason")
    ap.add_argument("--region", type=region_arg, default=None, metavar="X0,Y0,W,H",
                    help="decode only this box of the image as delivered (JXLDecoder region): the front-end reads the groups the box "
                         "needs and no others (jxf_set_region), and the output is the box: the full decode's pixels there, bit for "
                         "bit. An image whose frame does not qualify (JXLDecoder.region_rule) stops with the reason")
    ap.add_argument("--tone-map", type=tone_map_arg, default=None, metavar="NITS[,SOURCE_NITS]",
                    help="HDR to SDR inside the PNG's device colour pass (PNGWriter toneMap; jxl_ctx_set_tone_map): the BT.2408 "
                         "luminance curve to a display of NITS, from SOURCE_NITS (default: the image's intensity target), then a "
                         "desaturation into gamut. Replaces peak detection; writes an SDR PNG; turns --device-color on when "
                         "neither it nor --device-png is given")
    ap.add_argument("--no-gamut-map", action="store_true", help="with --tone-map: leave out-of-gamut samples to the quantiser's clipping")
    return ap


def tone_map_arg(text):
    """--tone-map=nits[,source_nits] -> (nits, source_nits or None), finite and positive"""
    try:
        v = tuple(float(t) for t in text.split(","))
    except ValueError:
        v = ()
    if len(v) not in (1, 2) or any(not (x > 0 and x != float("inf")) for x in v) or (len(v) == 2 and v[1] > 10000):
        raise argparse.ArgumentTypeError("expected NITS[,SOURCE_NITS], positive numbers (SOURCE_NITS at most 10000), not %r" % text)
    return (v[0], v[1] if len(v) == 2 else None)


def tone_map_of(a):
    """the ToneMap of the parsed arguments, or None; --tone-map turns --device-color on if no device colour switch was given"""
    if a.tone_map is None:
        return None
    from .decoder import ToneMap
    if not (a.device_color or a.device_png):
        a.device_color = True
    return ToneMap(targetNits=a.tone_map[0], sourceNits=a.tone_map[1], gamut=not a.no_gamut_map)


def region_arg(text):
    """--region=x0,y0,w,h -> a tuple of four integers"""
    try:
        box = tuple(int(v) for v in text.split(","))
    except ValueError:
        box = ()
    if len(box) != 4:
        raise argparse.ArgumentTypeError("expected x0,y0,w,h, not %r" % text)
    return box


def output_format(a):
    """'png' or 'pfm' for the parsed arguments: --format, else the output name's extension (JXLatte.java:136-145, 266-276), with
    PNG for every name that does not end in .pfm"""
    if a.format:
        return a.format
    return "pfm" if a.output and a.output.lower().endswith(".pfm") else "png"


def main(argv=None):
    a = parser().parse_args(argv)
    from . import frontend
    if a.info:
        fe = frontend.Frontend(open(a.input, "rb").read())
        im = fe.image
        print("Image: %s\n    Size: %dx%d\n    Bit Depth: %d\n    Extra Channels: %d\n    XYB Encoded: %s\n    Orientation: %d" % (
            a.input, im.width, im.height, im.bits_per_sample, im.num_extra, bool(im.xyb_encoded), im.orientation))
        return 0
    from .decoder import (PEAK_DETECT_AUTO, PEAK_DETECT_OFF, PEAK_DETECT_ON, DeviceBackend, JXLDecoder, PFMWriter, PNGWriter,
                          UnsupportedOperationException)
    PEAK_DETECT = {"auto": PEAK_DETECT_AUTO, "on": PEAK_DETECT_ON, "off": PEAK_DETECT_OFF}
    t0 = time.time()
    backend = DeviceBackend(a.device)
    try:
        dec = JXLDecoder(a.input, backend=backend, sparse_coeffs=a.sparse_coeffs, device_splines=a.device_splines,
                         device_patches=a.device_patches, device_output=a.device_png, device_canvas=a.device_canvas,
                         draw_varblocks=a.draw_varblocks, device_palette=a.device_palette, device_image=a.device_image,
                         device_frames=a.device_frames, device_patch_sets=a.device_patch_sets, device_chains=a.device_chains,
                         downsample=a.downsample, region=a.region)
    except ValueError as e:
        if a.downsample == 1 and a.region is None:
            raise
        print("jxlatte_amd: %s" % e, file=sys.stderr)
        backend.close()
        return 2
    try:
        image = dec.decode()
    except UnsupportedOperationException as e:
        if not ((a.downsample == 8 and str(e).startswith("downsample=8: ")) or (a.region is not None and str(e).startswith("region: "))):
            raise
        print("jxlatte_amd: %s" % e, file=sys.stderr)  # the frame does not qualify: decode without --downsample / --region
        backend.close()
        return 2
    if image is None:
        print("jxlatte_amd: no frames", file=sys.stderr)
        return 1
    t1 = time.time()
    for i, st in enumerate(dec.stats):
        print("    frame %d: %s %dx%d, %d groups%s" % (i, st["encoding"], st["width"], st["height"], st["groups"],
                                                       (", canvas %s" % st["canvas"] if a.device_canvas else "") +
                                                       (", image %s" % st["image"] if a.device_image else "") +
                                                       (", frame %s" % st["frame"] if a.device_frames else "") +
                                                       (", preview %s" % st["preview"] if a.downsample == 8 else "") +
                                                       (", region: %d of %d groups read (%s)" % (st["region"]["groups_read"], st["region"]["groups_total"],
                                                                                                  st["region"]["path"]) if "region" in st else "")), file=sys.stderr)
    print("Decoded %dx%d in %.3f s" % (image.getWidth(), image.getHeight(), t1 - t0), file=sys.stderr)
    if a.output and output_format(a) == "pfm":
        with open(a.output, "wb") as f:
            PFMWriter(image, deviceSamples=a.device_png).write(f)
    elif a.output:
        tone_map = tone_map_of(a)
        hdr = (image.isHDR() and tone_map is None) if a.png_hdr == "auto" else a.png_hdr == "yes"
        with open(a.output, "wb") as f:
            PNGWriter(image, bitDepth=16 if hdr else a.png_depth, hdr=hdr, peakDetect=PEAK_DETECT[a.png_peak_detect],
                      deviceColor=a.device_color, deviceSamples=a.device_png, toneMap=tone_map).write(f)
    backend.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
