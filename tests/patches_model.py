"""Independent model of the patch stage: JXLCodestreamDecoder.computePatches (JXLCodestreamDecoder.java:212-254) and what it
reaches of blendBuffers with patch == true (:415-513) and of the blend functions (:285-413), written from the Java. Nothing of the
project or of its oracle is imported; tests/blend_ref.py (itself written from the Java) lends ImageBuffer (`Buf`), clampAsc and
`TypeClash`.

The planes are `blend_ref.Buf` objects. The canvas handed to blendBuffers IS frameBuffer[d] (:248); ImageBuffer.castToFloat works
in place, so a cast shows in the frame's list and in the slot's list from then on. The control flow is the reference's, statement
by statement: the order (patch, position, channel d) with c = d < colours ? 0 : d - colours + 1, an absent slot skipped before any
size is looked at, the three size exceptions and the upsampling exception at their places, the cast decisions of :433-465 taken on
the RAW info.mode compared with the frame-blend constants, the remap of :468-486 and the `default` throw of :510-511, `below`
swapping old and new while the two alpha planes and the three offsets stay where they are.

Every float operation is one numpy float32 operation in the reference's order, int sums wrap, clampAsc lets a NaN through. Where
an operand of a blend function is the canvas itself read at another place than the pixel written -- only the below modes do that:
they hand the frame plane over as `ref`, read at patch.bounds.origin -- the loops are replayed pixel by pixel in the reference's
raster order, so a later pixel reads what an earlier one stored. `Result.replayed` says that this happened.

What the reference refuses:
  InvalidBitstream(message)  InvalidBitstreamException with that message
  TypeClash                  getFloatBuffer / getIntBuffer on a plane of the other type (IllegalStateException), System.arraycopy
                             between planes of two types (ArrayStoreException)
  NullPlane                  a null plane is dereferenced (NullPointerException)
  OutOfPlane                 an index outside a plane (ArrayIndexOutOfBoundsException)
The planes keep whatever was done to them before the refusal, as in the reference.

`mut=` names one deliberately wrong variant (MUTATIONS), in the style of tests/vardct_ref64.py and tests/pixel_ref64.py: the
shared cases must tell each of them from the model (tests/test_patches_model_cpu.py)."""
import numpy as np

from blend_ref import Buf, TypeClash, _clamp01

F = np.float32
REPLACE, ADD, BLEND, MULADD, MULT = 0, 1, 2, 3, 4  # FrameFlags.java:18-22
CE_GRAY = 1  # ColorFlags.CE_GRAY
ALPHA = 0    # ExtraChannelType.ALPHA

MUTATIONS = {
    "mode1_stores_nothing": "raw mode 1 returns after its casts instead of reaching the default throw of :510-511",
    "casts_on_mapped_mode": "the cast decisions of :446-465 look at the remapped mode instead of the raw info.mode",
    "below_not_swapped": "modes 5 and 7 keep old = frame, new = reference (:489-492 skipped)",
    "alpha_copy_at_ref_offset": "blendMulAdd's alpha copy (:390) reads `ref` at refOffset instead of frameOffset",
    "premult_from_own_channel": "premult comes from the channel's own extra-channel info instead of info.alphaChannel's (:428-431)",
    "blend_info_index_d": "blendingInfos[j][d] instead of [c] (:239-240)",
    "channel_outermost": "the channel loop is the outermost one instead of the innermost",
    "absent_slot_after_size_check": "positions of an absent slot are bounds-checked before the slot is skipped (:225-226 moved down)",
    "clamp_on_sample_in_blend": "blendBlend clamps newSample instead of newAlpha (:367-368)",
    "muladd_alpha_unclamped": "blendMulAdd ignores clamp (:408-409)",
    "created_alpha_plane_int": "the alpha plane of :449-451 is created with the canvas' type, and :453 never casts such a plane",
    "no_upsampling_check": "the check of :243-247 is missing",
    "ref_plane_created_float": "the plane of :441-442 is created float instead of with the canvas' type",
    "too_large_checked_per_position": "'Patch too large' is raised inside the position loop, after the bounds check of the position",
}


class InvalidBitstream(Exception):
    """InvalidBitstreamException"""


class NullPlane(Exception):
    """NullPointerException: a plane the function reads is null"""


class OutOfPlane(Exception):
    """ArrayIndexOutOfBoundsException"""


class Result:
    def __init__(self):
        self.created = set()    # (slot, channel): planes made by `new ImageBuffer` (:442, :450)
        self.replayed = False   # some application read the canvas away from the pixel it wrote
        self.applications = 0   # blendBuffers calls that reached the switch of :493
        self.left_as_created = []  # (only the mutation created_alpha_plane_int fills it)


def _need(buf, want_int):
    if buf is None:
        raise NullPlane()
    if buf.is_int() != want_int:
        raise TypeClash()
    return buf


def _loops(res, canvas, reads, patch_start, size, fn):
    """the double loop of a blend function: canvas[patchStart + (y, x)] = fn(operands at their offsets + (y, x)). reads: (Buf, offset)
    pairs. Rectangles are checked as the loops would find them (an empty rectangle touches nothing)."""
    h, w = size
    if h <= 0 or w <= 0:
        return
    for b, off in list(reads) + [(canvas, patch_start)]:
        if off[0] < 0 or off[1] < 0 or off[0] + h > b.a.shape[0] or off[1] + w > b.a.shape[1]:
            raise OutOfPlane()
    py, px = patch_start
    off_pixel = any(b is canvas and tuple(off) != (py, px) for b, off in reads)
    with np.errstate(all="ignore"):
        if not off_pixel:
            vals = [b.a[off[0]:off[0] + h, off[1]:off[1] + w].copy() for b, off in reads]
            out = fn(*vals)
            assert out.dtype == canvas.a.dtype
            canvas.a[py:py + h, px:px + w] = out
            return
        res.replayed = True
        for y in range(h):
            for x in range(w):
                vals = [b.a[off[0] + y:off[0] + y + 1, off[1] + x:off[1] + x + 1].copy() for b, off in reads]
                out = fn(*vals)
                assert out.dtype == canvas.a.dtype
                canvas.a[py + y, px + x] = out[0, 0]


def _copy_to_canvas(res, canvas, patch_start, frame_off, size, frame):  # :34-41: System.arraycopy, row by row
    if frame is None or canvas is None:
        raise NullPlane()
    h, w = size
    for y in range(h):
        if frame_off[0] + y >= frame.a.shape[0] or frame_off[0] + y < 0 or patch_start[0] + y >= canvas.a.shape[0]:
            raise OutOfPlane()
        if canvas.a.dtype != frame.a.dtype:
            raise TypeClash()
        if frame_off[1] < 0 or patch_start[1] < 0 or frame_off[1] + w > frame.a.shape[1] or patch_start[1] + w > canvas.a.shape[1]:
            raise OutOfPlane()
        row = frame.a[frame_off[0] + y, frame_off[1]:frame_off[1] + w].copy()  # (arraycopy behaves as if through a temporary)
        canvas.a[patch_start[0] + y, patch_start[1]:patch_start[1] + w] = row


def _blend_add(res, canvas, frame, ref, patch_start, frame_off, ref_off, size):  # :285-318
    if frame is None:
        raise NullPlane()
    if frame.is_int():
        _need(canvas, True), _need(ref, True)
        fn = lambda r, f: (r.view(np.uint32) + f.view(np.uint32)).view(np.int32)  # noqa: E731
    else:
        _need(canvas, False), _need(ref, False)
        fn = lambda r, f: (r + f).astype(F)  # noqa: E731
    _loops(res, canvas, [(ref, ref_off), (frame, frame_off)], patch_start, size, fn)


def _blend_mult(res, canvas, frame, ref, patch_start, frame_off, ref_off, size, clamp):  # :320-339
    _need(canvas, False), _need(ref, False), _need(frame, False)

    def fn(r, f):
        if clamp:
            f = _clamp01(f)
        return (f * r).astype(F)
    _loops(res, canvas, [(ref, ref_off), (frame, frame_off)], patch_start, size, fn)


def _blend_blend(res, canvas, frame, ref, frame_alpha, ref_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra, clamp,
                 premult, mut):  # :341-379
    if not has_extra:
        return _blend_add(res, canvas, frame, ref, patch_start, frame_off, ref_off, size)
    if not is_alpha:
        _need(ref_alpha, False), _need(frame_alpha, False)
    _need(ref, False), _need(frame, False), _need(canvas, False)
    one = F(1)

    def fn(old_s, new_s, old_a=None, new_a=None):
        if is_alpha:
            old_a, new_a = old_s, new_s
        if clamp:
            if mut == "clamp_on_sample_in_blend":
                new_s = _clamp01(new_s)
                if is_alpha:
                    new_a = new_s
            else:
                new_a = _clamp01(new_a)
        if is_alpha:
            return (old_a + (new_a * (one - old_a)).astype(F)).astype(F)
        if premult:
            return (new_s + (old_s * (one - new_a)).astype(F)).astype(F)
        num = ((new_s * new_a).astype(F) + ((old_s * old_a).astype(F) * (one - new_a)).astype(F)).astype(F)
        den = (old_a + (new_a * (one - old_a)).astype(F)).astype(F)
        return (num / den).astype(F)
    reads = [(ref, ref_off), (frame, frame_off)]
    if not is_alpha:
        reads += [(ref_alpha, ref_off), (frame_alpha, frame_off)]
    _loops(res, canvas, reads, patch_start, size, fn)


def _blend_muladd(res, canvas, frame, ref, frame_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra, clamp, mut):  # :381-413
    if not has_extra:
        return _blend_add(res, canvas, frame, ref, patch_start, frame_off, ref_off, size)
    if is_alpha:
        off = ref_off if mut == "alpha_copy_at_ref_offset" else frame_off
        if ref is canvas and tuple(off) != tuple(patch_start):
            res.replayed = True  # (row by row through a temporary, as arraycopy: _copy_to_canvas does just that)
        return _copy_to_canvas(res, canvas, patch_start, off, size, ref)
    _need(frame_alpha, False), _need(ref, False), _need(frame, False), _need(canvas, False)

    def fn(old_s, new_s, new_a):
        if clamp and mut != "muladd_alpha_unclamped":
            new_a = _clamp01(new_a)
        return (old_s + (new_a * new_s).astype(F)).astype(F)
    _loops(res, canvas, [(ref, ref_off), (frame, frame_off), (frame_alpha, frame_off)], patch_start, size, fn)


def blend_buffers_patch(res, info, canvas, frame_buffers, ref_buffers, slot, patch_start, frame_off, ref_off, size, idx, frame_colors,
                        binfo, mut=None):
    """blendBuffers(..., patch = true) (:415-513). binfo: (mode, alphaChannel, clamp) of the BlendingInfo"""
    raw, alpha_channel, clamp = int(binfo[0]), int(binfo[1]), bool(binfo[2])
    colors = 1 if info.colour_space == CE_GRAY else 3
    frame_buffer = frame_buffers[(1 if idx == 0 else idx + 2) if colors != frame_colors else idx]  # :420
    ex = idx - colors
    is_extra = ex >= 0
    has_extra = info.num_extra > 0
    is_alpha = is_extra and info.ec_type[ex] == ALPHA
    if has_extra:
        if not 0 <= alpha_channel < info.num_extra:
            raise OutOfPlane()  # getExtraChannelInfo(info.alphaChannel)
        premult = bool(info.ec_alpha_associated[alpha_channel])
        if mut == "premult_from_own_channel":
            premult = bool(info.ec_alpha_associated[ex if is_extra else 0])
    else:
        premult = False
    depth = info.ec_bits[ex] if is_extra else info.bits_per_sample
    if canvas.is_int() != frame_buffer.is_int():  # :433-436
        frame_buffer.cast_to_float(depth)
        canvas.cast_to_float(depth)
    if raw == REPLACE or (ref_buffers is None and raw == ADD):  # :437-440 (computePatches lets neither through)
        return _copy_to_canvas(res, canvas, patch_start, frame_off, size, frame_buffer)
    # :466-486, computed here only for the mutation that decides the casts on it
    mode, below = raw, False
    if raw == 5:
        mode, below = BLEND, True
    elif raw == 6:
        mode = MULADD
    elif raw == 7:
        mode, below = MULADD, True
    else:
        mode = raw - 1
    seen = mode if mut == "casts_on_mapped_mode" else raw  # what :446-459 compare with the constants
    if ref_buffers[idx] is None:  # :441-442
        ref_buffers[idx] = Buf(np.zeros(canvas.a.shape, F if mut == "ref_plane_created_float" else canvas.a.dtype))
        res.created.add((slot, idx))
    ref_buffer = ref_buffers[idx]
    ref_alpha = ref_buffers[colors + alpha_channel] if has_extra else None
    frame_alpha = frame_buffers[frame_colors + alpha_channel] if has_extra else None
    if has_extra and seen in (BLEND, MULADD):  # :446-456
        a_depth = info.ec_bits[alpha_channel]
        if seen == BLEND:
            if ref_alpha is None:
                ref_alpha = Buf(np.zeros(canvas.a.shape, canvas.a.dtype if mut == "created_alpha_plane_int" else F))
                ref_buffers[colors + alpha_channel] = ref_alpha
                res.created.add((slot, colors + alpha_channel))
                if mut == "created_alpha_plane_int":
                    res.left_as_created.append(ref_alpha)
            if not any(b is ref_buffers[colors + alpha_channel] for b in res.left_as_created):
                ref_buffers[colors + alpha_channel].cast_to_float(a_depth)
        if frame_buffers[frame_colors + alpha_channel] is None:
            raise NullPlane()
        frame_buffers[frame_colors + alpha_channel].cast_to_float(a_depth)
    should_cast = seen == MULT or (seen == BLEND and has_extra) or (seen == MULADD and has_extra and not is_alpha)  # :457-459
    if should_cast or ref_buffer.is_int() != frame_buffer.is_int():  # :461-465
        frame_buffer.cast_to_float(depth)
        canvas.cast_to_float(depth)
        ref_buffer.cast_to_float(depth)
    if raw == 1 and mut == "mode1_stores_nothing":
        return
    old_buffer, new_buffer = frame_buffer, ref_buffer  # :487-492
    if below and mut != "below_not_swapped":
        new_buffer, old_buffer = frame_buffer, ref_buffer
    res.applications += 1
    if mode == ADD:  # :493-512; the functions name their second and third parameter `frame` and `ref`
        _blend_add(res, canvas, old_buffer, new_buffer, patch_start, frame_off, ref_off, size)
    elif mode == MULT:
        _blend_mult(res, canvas, old_buffer, new_buffer, patch_start, frame_off, ref_off, size, clamp)
    elif mode == BLEND:
        _blend_blend(res, canvas, old_buffer, new_buffer, frame_alpha, ref_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra,
                     clamp, premult, mut)
    elif mode == MULADD:
        _blend_muladd(res, canvas, old_buffer, new_buffer, frame_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra, clamp, mut)
    else:
        res.applications -= 1
        raise InvalidBitstream("Illegal blend mode")


def compute_patches(info, hdr, patches, frame, reference, frame_colors=None, mut=None):
    """computePatches (:212-254) on `frame` (list of Buf, changed in place) and `reference` (four entries: None or a list of Buf /
    None, changed in place). info: colour_space, num_extra, ec_type, ec_alpha_associated, ec_bits, bits_per_sample and -- read only
    where the frame is upsampled -- ec_dim_shift; hdr: upsampling, ec_upsampling, or None for a frame that is not upsampled; the
    frame's bounds are its planes' size. patches: dicts with ref, y0, x0, h, w (patch.bounds), positions [n][2] (y, x) and blend
    [n][1 + num_extra][3] (mode, alphaChannel, clamp). Returns a Result."""
    assert mut is None or mut in MUTATIONS, mut
    res = Result()
    colors = 1 if info.colour_space == CE_GRAY else 3
    if frame_colors is None:
        frame_colors = colors
    n_chan = colors + info.num_extra
    fh, fw = frame[0].a.shape  # header.bounds.size
    upsampling = 1 if hdr is None else hdr.upsampling

    def position(p, j, ref, channels):
        y0, x0 = int(p["positions"][j][0]), int(p["positions"][j][1])
        if y0 < 0 or x0 < 0:  # :233-234
            raise InvalidBitstream("Patch size out of bounds")
        if p["h"] + y0 > fh or p["w"] + x0 > fw:  # :235-237
            raise InvalidBitstream("Patch size out of bounds")
        if mut == "too_large_checked_per_position" and ref is not None:
            if p["y0"] + p["h"] > ref[0].a.shape[0] or p["x0"] + p["w"] > ref[0].a.shape[1]:
                raise InvalidBitstream("Patch too large")
        if ref is None:  # (only the mutation that checks before it skips comes here)
            return
        for d in channels:
            c = 0 if d < colors else d - colors + 1  # :239
            binfo = p["blend"][j][d if mut == "blend_info_index_d" else c]  # :240
            raw = int(binfo[0])
            if raw == 0:  # :241-242
                continue
            if mut != "no_upsampling_check" and raw > 3 and upsampling > 1 and c > 0 and \
                    (hdr.ec_upsampling[c - 1] << info.ec_dim_shift[c - 1]) != upsampling:  # :243-247
                raise InvalidBitstream("Alpha channel upsampling mismatch during patches")
            blend_buffers_patch(res, info, frame[d], frame, ref, p["ref"], (y0, x0), (y0, x0), (p["y0"], p["x0"]), (p["h"], p["w"]), d,
                                frame_colors, binfo, mut)

    def patch(p, channels):
        if p["ref"] > 3:  # :220-221
            raise InvalidBitstream("Patch out of range")
        ref = reference[p["ref"]]
        if ref is None:  # :225-226
            if mut == "absent_slot_after_size_check":
                for j in range(len(p["positions"])):
                    position(p, j, None, channels)
            return
        if ref[0] is None:
            raise NullPlane()
        if mut != "too_large_checked_per_position":
            if p["y0"] + p["h"] > ref[0].a.shape[0] or p["x0"] + p["w"] > ref[0].a.shape[1]:  # :227-229
                raise InvalidBitstream("Patch too large")
        for j in range(len(p["positions"])):
            position(p, j, ref, channels)

    if mut == "channel_outermost":
        for d in range(n_chan):
            for p in patches:
                patch(p, [d])
    else:
        for p in patches:
            patch(p, range(n_chan))
    return res
