"""Reference of the morphology setting (include/mi_unet.h: mi_unet_set_morph) in numpy + scipy.  It shares no code with
the product: the element comes from the definition, an erosion / dilation is scipy's with the border rules spelled out
(border_value = 1: the border never constrains an erosion; border_value = 0: it never seeds a dilation), and the four-step chain is
written out here on the pattern of test_targets_cpu.scipy_target_mask."""
import numpy as np
from scipy import ndimage as ndi

RECT, DISC = 0, 1
MAX_R = 31
S8 = np.ones((3, 3), bool)


def element(shape, r):
    """bool [2r + 1, 2r + 1]: the box, or { (dx, dy) : dx*dx + dy*dy <= r*r } in integer arithmetic"""
    d = np.arange(-r, r + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    if shape == RECT:
        return np.ones((2 * r + 1, 2 * r + 1), bool)
    assert shape == DISC
    return dx * dx + dy * dy <= r * r


def erode(a, shape, r):
    return ndi.binary_erosion(a, element(shape, r), border_value=1)


def dilate(a, shape, r):
    return ndi.binary_dilation(a, element(shape, r), border_value=0)


def brute_step(a, shape, r, is_dilate):
    """the definition as a plain loop over the element, positions outside the image skipped"""
    h, w = a.shape
    el = element(shape, r)
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            vals = [a[y + dy, x + dx] for dy in range(-r, r + 1) for dx in range(-r, r + 1)
                    if el[dy + r, dx + r] and 0 <= y + dy < h and 0 <= x + dx < w]
            out[y, x] = any(vals) if is_dilate else all(vals)
    return out


def min_area_of(h, w, frac):
    return int(np.float32(w * h) * np.float32(frac))


def chain(labels, cls, frac, shape=RECT, open_r=1, close_r=0):
    """fill holes -> close (dilate, erode by close_r) -> open (erode, dilate by open_r) -> area filter; u8 in {0, cls}"""
    h, w = labels.shape
    min_area = min_area_of(h, w, frac)
    fg = labels == cls
    lab, n = ndi.label(~fg, structure=S8)
    for i, sl in enumerate(ndi.find_objects(lab), start=1):
        ys, xs = sl
        comp = lab[sl] == i
        if xs.start > 0 and ys.start > 0 and xs.stop - 1 < w - 1 and ys.stop - 1 < h - 1 and int(comp.sum()) < min_area:
            fg[sl] |= comp
    fg = erode(dilate(fg, shape, close_r), shape, close_r)
    fg = dilate(erode(fg, shape, open_r), shape, open_r)
    lab, n = ndi.label(fg, structure=S8)
    out = np.zeros((h, w), np.uint8)
    if n:
        areas = np.bincount(lab.ravel(), minlength=n + 1)
        keep = areas >= min_area
        keep[0] = False
        out[keep[lab]] = cls
    return out


def masks(labels, targets, morph):
    """u8 [K][H][W]: every target's chain on one label map; morph = one (shape, open_r, close_r) for all targets or one per target"""
    assert len(morph) in (1, len(targets))
    return np.stack([chain(labels, c, f, *morph[0 if len(morph) == 1 else k]) for k, (c, f) in enumerate(targets)])


def component_areas(mask):
    """sorted pixel counts of the 8-connected components of mask != 0"""
    lab, n = ndi.label(mask != 0, structure=S8)
    return sorted(np.bincount(lab.ravel(), minlength=n + 1)[1:].tolist())
