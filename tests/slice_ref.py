"""What a layer kernel left in a poisoned, strided allocation (binding.layer_debug_strided): the slice it was to write, and every
element outside the slice that it touched.

The allocation is `guard` bytes, then [npix][ld] elements of which channels [co_off, co_off + C) of every pixel are the slice,
then `guard` bytes; everything was 0xFF bytes before the launch (a NaN in fp32, bf16 and fp16).  A stray store that writes 0xFF
bytes, or one farther away than the guard, is not seen."""
from collections import namedtuple

import numpy as np

POISON = 0xFF

# region: "front guard" / "image" / "back guard".  In a guard `index` is the element's distance in elements from the guard's first
# byte and b, y, x, c are None; in the image b, y, x, c name the pixel and the channel of its ld-wide row (c < co_off: the gap in
# front of the slice, c >= co_off + C: the gap behind it).  value: the element as float, bits: its raw bits.
Stray = namedtuple("Stray", "region index b y x c value bits")
# summary: over ALL stray elements -- how many lie in either guard, and for those in the image the range of channels and the number
# of pixels they touch (a store mask that is too wide shows as one channel range over many pixels)
Slices = namedtuple("Slices", "dense strays n_strays unwritten summary")


def _to_float(a, kind):
    """raw elements -> float32: 4-byte elements are fp32; 2-byte ones bf16 (kind 1) or fp16 (kind 2), as layer_debug converts"""
    if a.dtype == np.uint32:
        return a.view(np.float32)
    if kind == 2:
        return a.view(np.float16).astype(np.float32)
    return (a.astype(np.uint32) << 16).view(np.float32)


def check(raw, elem_bytes, shape, C, ld, co_off, guard, kind=0, limit=16):
    """raw: the allocation as uint8; shape = (B, Ho, Wo).  Returns Slices: the dense slice [B][Ho][Wo][C] as float32, the first
    `limit` stray elements (address order), their total number, and the number of slice elements that are still poison."""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    B, Ho, Wo = shape
    npix = B * Ho * Wo
    assert elem_bytes in (2, 4) and guard % elem_bytes == 0 and 0 <= co_off and co_off + C <= ld
    assert raw.size == 2 * guard + npix * ld * elem_bytes, (raw.size, guard, npix, ld, elem_bytes)
    ut = np.uint32 if elem_bytes == 4 else np.uint16
    poison = ut(0xFFFFFFFF if elem_bytes == 4 else 0xFFFF)
    el = raw.view(ut)
    g = guard // elem_bytes
    img = el[g:g + npix * ld].reshape(npix, ld)
    sl = img[:, co_off:co_off + C]
    dense = _to_float(np.ascontiguousarray(sl), kind).reshape(B, Ho, Wo, C)
    unwritten = int(np.count_nonzero(sl == poison))
    touched = el != poison
    touched[g:g + npix * ld].reshape(npix, ld)[:, co_off:co_off + C] = False
    idx = np.flatnonzero(touched)
    front, back = int(np.count_nonzero(idx < g)), int(np.count_nonzero(idx >= g + npix * ld))
    inside = idx[(idx >= g) & (idx < g + npix * ld)] - g
    summary = {"front guard": front, "back guard": back, "image": int(inside.size)}
    if inside.size:
        ch = inside % ld
        summary.update(channels=(int(ch.min()), int(ch.max())), pixels=int(np.unique(inside // ld).size))
    strays = []
    for i in idx[:limit].tolist():
        bits = int(el[i])
        value = float(_to_float(el[i:i + 1], kind)[0])
        if i < g:
            strays.append(Stray("front guard", i, None, None, None, None, value, bits))
        elif i >= g + npix * ld:
            strays.append(Stray("back guard", i - g - npix * ld, None, None, None, None, value, bits))
        else:
            p, c = divmod(i - g, ld)
            b, r = divmod(p, Ho * Wo)
            y, x = divmod(r, Wo)
            strays.append(Stray("image", i - g, b, y, x, c, value, bits))
    return Slices(dense, strays, int(idx.size), unwritten, summary)


def describe(strays, n_strays, summary=None):
    """the failure message's tail: where the stray elements lie (all of them in summary, the first few one by one)"""
    if not n_strays:
        return "no stray element"
    head = ""
    if summary:
        head = f"[front guard {summary['front guard']}, back guard {summary['back guard']}, image {summary['image']}"
        if summary["image"]:
            head += f": channels {summary['channels'][0]}..{summary['channels'][1]} of {summary['pixels']} pixel(s)"
        head += "] "
    parts = []
    for s in strays:
        where = f"{s.region}[{s.index}]" if s.region != "image" else f"image b={s.b} y={s.y} x={s.x} channel={s.c}"
        parts.append(f"{where} = {s.value!r} (0x{s.bits:x})")
    return f"{n_strays} stray element(s): " + head + "; ".join(parts) + (" ..." if n_strays > len(strays) else "")
