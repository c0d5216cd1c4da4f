"""numpy restatement of JXLCodestreamDecoder.blendFrame + blendBuffers and the blend functions they reach
(JXLCodestreamDecoder.java:34-41, 285-537), written from the Java: ImageBuffer objects that alias (reference[k] == canvas), casts
that happen in place and persist (ImageBuffer.castToFloat, ImageBuffer.java:99-127), channels visited in canvas order. Every float
operation is one numpy float32 operation in the reference's order; the int sum wraps as Java's does.

`info` and `fr` carry the fields of the image and frame headers under the names jxlatte_amd.decoder uses (info: colour_space,
num_extra, ec_type, ec_alpha_associated, ec_bits, bits_per_sample, height, width; fr: y0, x0, height, width, upsampling,
blend_mode / _alpha / _clamp / _source and their ec_ lists), so one pair of objects feeds this model and blend_type_plan.

One place leaves the Java: with refBuffers == null a mode other than REPLACE / ADD dereferences null there (:441); the decoder
reads fresh zero planes instead (decoder.py, _blend_buffers), and so does this model."""
import numpy as np

F = np.float32
REPLACE, ADD, BLEND, MULADD, MULT = 0, 1, 2, 3, 4
CE_GRAY = 1  # jxlatte_amd.decoder.CE_GRAY (ColorFlags.CE_GRAY)


class NotModelled(Exception):
    """an operand that is the canvas itself is read away from the pixel that is written: the reference's loops then depend on
    their own order, which this whole-rectangle model does not replay"""


class TypeClash(Exception):
    """the reference would throw here (ArrayStoreException, ClassCastException): planes of two types in one function"""


class Buf:
    """ImageBuffer: one plane, int32 or float32, cast in place"""

    def __init__(self, a):
        a = np.array(a, copy=True)
        assert a.dtype in (np.int32, np.float32) and a.ndim == 2
        self.a = a

    def is_int(self):
        return self.a.dtype == np.int32

    def cast_to_float(self, depth):  # ImageBuffer.java:99-127
        if not self.is_int():
            return
        maxv = int(np.array(~((~0) << (depth & 31)), np.int64).astype(np.int32))  # Java int: the shift count counts modulo 32
        if maxv < 1:
            raise ValueError("invalid Max Value")
        scale = F(1.0) / F(maxv)
        self.a = (self.a.astype(F) * scale).astype(F)

    def copy(self):  # new ImageBuffer(b)
        return Buf(self.a)


def _clamp01(v):  # MathHelper.clampAsc: a NaN passes through
    return np.where(v < F(0), F(0), np.where(v > F(1), F(1), v)).astype(F)


def _rect(buf, off, size):
    return buf.a[off[0]:off[0] + size[0], off[1]:off[1] + size[1]]


def _store(canvas, patch_start, size, value):
    if value.dtype != canvas.a.dtype:
        raise TypeClash()
    _rect(canvas, patch_start, size)[...] = value


def copy_to_canvas(canvas, patch_start, frame_off, size, frame):  # :34-41, System.arraycopy row by row
    if canvas.a.dtype != frame.a.dtype:
        raise TypeClash()
    for y in range(size[0]):
        row = frame.a[y + frame_off[0], frame_off[1]:frame_off[1] + size[1]].copy()
        canvas.a[y + patch_start[0], patch_start[1]:patch_start[1] + size[1]] = row


def _reads(bufs_offs, canvas, patch_start, size):
    """the operand rectangles, read before the store. Exact for the reference's pixel-by-pixel loops as long as an operand that
    IS the canvas is read at the pixels that are written -- blendFrame's refOffset is its patchStart (:534)"""
    for b, off in bufs_offs:
        if b is canvas:
            if tuple(off) != tuple(patch_start):
                raise NotModelled()
    return [_rect(b, off, size).copy() for b, off in bufs_offs]


def blend_add(canvas, frame, ref, patch_start, frame_off, ref_off, size):  # :285-318
    r, f = _reads([(ref, ref_off), (frame, frame_off)], canvas, patch_start, size)
    with np.errstate(all="ignore"):
        if frame.is_int():
            if r.dtype != np.int32:
                raise TypeClash()
            out = (r.view(np.uint32) + f.view(np.uint32)).view(np.int32)
        else:
            if r.dtype != np.float32:
                raise TypeClash()
            out = (r + f).astype(F)
    _store(canvas, patch_start, size, out)


def blend_mult(canvas, frame, ref, patch_start, frame_off, ref_off, size, clamp):  # :320-339
    if frame.is_int() or ref.is_int() or canvas.is_int():
        raise TypeClash()
    r, f = _reads([(ref, ref_off), (frame, frame_off)], canvas, patch_start, size)
    with np.errstate(all="ignore"):
        if clamp:
            f = _clamp01(f)
        out = (f * r).astype(F)
    _store(canvas, patch_start, size, out)


def blend_blend(canvas, frame, ref, frame_alpha, ref_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra, clamp, premult):
    if not has_extra:  # :346-349
        return blend_add(canvas, frame, ref, patch_start, frame_off, ref_off, size)
    if frame.is_int() or ref.is_int() or canvas.is_int():
        raise TypeClash()
    old_s, new_s = _reads([(ref, ref_off), (frame, frame_off)], canvas, patch_start, size)
    if is_alpha:
        old_a, new_a = old_s, new_s
    else:
        if frame_alpha.is_int() or ref_alpha.is_int():
            raise TypeClash()
        old_a, new_a = _reads([(ref_alpha, ref_off), (frame_alpha, frame_off)], canvas, patch_start, size)
    one = F(1)
    with np.errstate(all="ignore"):
        if clamp:
            new_a = _clamp01(new_a)
        if is_alpha:
            out = old_a + new_a * (one - old_a)
        elif premult:
            out = new_s + old_s * (one - new_a)
        else:
            out = (new_s * new_a + old_s * old_a * (one - new_a)) / (old_a + new_a * (one - old_a))
    _store(canvas, patch_start, size, out.astype(F))


def blend_muladd(canvas, frame, ref, frame_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra, clamp):  # :381-413
    if not has_extra:
        return blend_add(canvas, frame, ref, patch_start, frame_off, ref_off, size)
    if is_alpha:
        if ref is canvas and tuple(frame_off) != tuple(patch_start):
            raise NotModelled()
        return copy_to_canvas(canvas, patch_start, frame_off, size, ref)  # :390: ref at frameOffset
    if frame.is_int() or ref.is_int() or canvas.is_int() or frame_alpha.is_int():
        raise TypeClash()
    old_s, new_s, new_a = _reads([(ref, ref_off), (frame, frame_off), (frame_alpha, frame_off)], canvas, patch_start, size)
    with np.errstate(all="ignore"):
        if clamp:
            new_a = _clamp01(new_a)
        out = old_s + new_a * new_s
    _store(canvas, patch_start, size, out.astype(F))


def blend_buffers(info, canvas_list, idx, frame_buffers, ref_buffers, patch_start, frame_off, ref_off, size, frame_colors, mode, alpha_channel,
                  clamp):
    """blendBuffers with patch == false (:415-513)"""
    colors = 1 if info.colour_space == CE_GRAY else 3
    canvas = canvas_list[idx]
    frame_buffer = frame_buffers[(1 if idx == 0 else idx + 2) if colors != frame_colors else idx]  # :420
    ex = idx - colors
    is_extra = ex >= 0
    has_extra = info.num_extra > 0
    is_alpha = is_extra and info.ec_type[ex] == 0
    premult = has_extra and bool(info.ec_alpha_associated[alpha_channel])
    depth = info.ec_bits[ex] if is_extra else info.bits_per_sample
    if canvas.is_int() != frame_buffer.is_int():  # :433-436
        frame_buffer.cast_to_float(depth)
        canvas.cast_to_float(depth)
    if mode == REPLACE or (ref_buffers is None and mode == ADD):  # :437-440
        return copy_to_canvas(canvas, patch_start, frame_off, size, frame_buffer)
    if ref_buffers is None:
        ref_buffers = [None] * len(canvas_list)  # (the decoder's stand-in for the reference's null dereference)
    if ref_buffers[idx] is None:  # :441-442
        ref_buffers[idx] = Buf(np.zeros(canvas.a.shape, canvas.a.dtype))
    ref_buffer = ref_buffers[idx]
    ref_alpha = ref_buffers[colors + alpha_channel] if has_extra else None
    frame_alpha = frame_buffers[frame_colors + alpha_channel] if has_extra else None
    if has_extra and mode in (BLEND, MULADD):  # :446-456
        a_depth = info.ec_bits[alpha_channel]
        if mode == BLEND:
            if ref_alpha is None:
                ref_alpha = Buf(np.zeros(canvas.a.shape, F))
                ref_buffers[colors + alpha_channel] = ref_alpha
            ref_buffers[colors + alpha_channel].cast_to_float(a_depth)
        frame_buffers[frame_colors + alpha_channel].cast_to_float(a_depth)
    should_cast = mode == MULT or (mode == BLEND and has_extra) or (mode == MULADD and has_extra and not is_alpha)
    if should_cast or ref_buffer.is_int() != frame_buffer.is_int():  # :457-465
        frame_buffer.cast_to_float(depth)
        canvas.cast_to_float(depth)
        ref_buffer.cast_to_float(depth)
    old_buffer, new_buffer = frame_buffer, ref_buffer  # the names of :487-488; the functions call them frame and ref
    if mode == ADD:
        blend_add(canvas, old_buffer, new_buffer, patch_start, frame_off, ref_off, size)
    elif mode == MULT:
        blend_mult(canvas, old_buffer, new_buffer, patch_start, frame_off, ref_off, size, clamp)
    elif mode == BLEND:
        blend_blend(canvas, old_buffer, new_buffer, frame_alpha, ref_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra, clamp, premult)
    elif mode == MULADD:
        blend_muladd(canvas, old_buffer, new_buffer, frame_alpha, patch_start, frame_off, ref_off, size, is_alpha, has_extra, clamp)
    else:
        raise ValueError("Illegal blend mode")


def blend_frame(info, fr, canvas, frame_buffers, reference):
    """blendFrame (:515-537): canvas, frame_buffers: lists of Buf; reference: four entries, None or a list of Buf -- the very
    list object `canvas` where the slot aliases the canvas"""
    ih, iw = info.height, info.width
    colors = 1 if info.colour_space == CE_GRAY else 3
    py, px = min(max(fr.y0, 0), ih), min(max(fr.x0, 0), iw)
    fy, fx = py - fr.y0, px - fr.x0
    ly, lx = fr.y0 + fr.height * fr.upsampling, fr.x0 + fr.width * fr.upsampling
    bh, bw = min(ly, ih) - py, min(lx, iw) - px
    if bh <= 0 or bw <= 0:  # (the decoder returns here; the reference's loops would run zero times behind their casts)
        return
    frame_colors = len(frame_buffers) - info.num_extra
    for c in range(len(canvas)):
        if c >= colors:
            e = c - colors
            mode, alpha, clamp, source = fr.ec_blend_mode[e], fr.ec_blend_alpha[e], fr.ec_blend_clamp[e], fr.ec_blend_source[e]
        else:
            mode, alpha, clamp, source = fr.blend_mode, fr.blend_alpha, fr.blend_clamp, fr.blend_source
        blend_buffers(info, canvas, c, frame_buffers, reference[source], (py, px), (fy, fx), (py, px), (bh, bw), frame_colors, mode, alpha,
                      bool(clamp))
