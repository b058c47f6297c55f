"""CPU reference of the region measurement (include/mi_unet.h: mi_unet_set_measure) and of mi_unet_region_derive.

The regions of a mask: scipy.ndimage.label with the 3 x 3 structure; contour c of oracle_lib.find_contours is linked to the component
that contains its first point; every field from Python-int sums (numpy dtype=object), so nothing can wrap; `edges` from four shifted
comparisons against a zero-padded mask.  The derived quantities: the header's formulas with Python integers and math."""
import math

import numpy as np
from scipy import ndimage

import oracle_lib as orc

FIELDS = ("area", "x0", "y0", "x1", "y1", "imin", "imax", "channel", "edges", "sx", "sy", "sxx", "syy", "sxy", "si", "sii")
ZERO = dict.fromkeys(FIELDS, 0)


def crack_edges(fg):
    """per pixel: its edges towards a 4-neighbour that is not foreground (the frame counts as not foreground)"""
    p = np.pad(fg, 1)
    c = p[1:-1, 1:-1]
    return (c & ~p[1:-1, :-2]).astype(np.int64) + (c & ~p[1:-1, 2:]) + (c & ~p[:-2, 1:-1]) + (c & ~p[2:, 1:-1])


def regions_of(mask, tile=None, channel=0):
    """mask u8 [H,W], tile u8 [H,W] or [H,W,C] or None -> list of field dicts, one per external contour, in contour order"""
    fg = np.ascontiguousarray(mask) > 127
    lab, _ = ndimage.label(fg, structure=np.ones((3, 3), int))
    edges = crack_edges(fg)
    if tile is not None and tile.ndim == 2:
        tile = tile[:, :, None]
    out = []
    for cont in orc.find_contours(mask):
        x0, y0 = cont[0]
        comp = lab[y0, x0]
        assert comp > 0
        ys, xs = np.nonzero(lab == comp)
        assert (int(ys[0]), int(xs[0])) == (y0, x0)            # the contour's first point is the component's raster-first pixel
        X, Y = xs.astype(object), ys.astype(object)
        r = dict(area=len(xs), x0=int(xs.min()), y0=int(ys.min()), x1=int(xs.max()), y1=int(ys.max()), edges=int(edges[ys, xs].sum()),
                 sx=int(X.sum()), sy=int(Y.sum()), sxx=int((X * X).sum()), syy=int((Y * Y).sum()), sxy=int((X * Y).sum()))
        if tile is None:
            r.update(imin=0, imax=0, channel=-1, si=0, sii=0)
        else:
            v = tile[ys, xs, channel].astype(object)
            r.update(imin=int(v.min()), imax=int(v.max()), channel=channel, si=int(v.sum()), sii=int((v * v).sum()))
        out.append(r)
    return out


def record(rec):
    """one REGION_DTYPE record -> field dict of Python ints"""
    return {f: int(rec[f]) for f in FIELDS}


def assert_plane(regions, count, ref, what=""):
    """regions: REGION_DTYPE [cap] of one plane, count: its entry of counts; ref: regions_of(...)"""
    assert count == len(ref), f"{what}: {count} regions, reference {len(ref)}"
    for c, r in enumerate(ref):
        assert record(regions[c]) == r, f"{what}: region {c}"
    for c in range(len(ref), len(regions)):
        assert record(regions[c]) == ZERO, f"{what}: entry {c} behind the count is not zero"


def derive(r):
    """the header's formulas; r: field dict.  Exact integer numerators, one division each."""
    A = r["area"]
    m20 = (A * r["sxx"] - r["sx"] ** 2) / A ** 2
    m02 = (A * r["syy"] - r["sy"] ** 2) / A ** 2
    m11 = (A * r["sxy"] - r["sx"] * r["sy"]) / A ** 2
    a, c, b = m20 + 1 / 12, m02 + 1 / 12, m11
    root = math.sqrt((a - c) ** 2 + 4 * b * b)
    return dict(cx=r["sx"] / A, cy=r["sy"] / A, major=4 * math.sqrt(((a + c) + root) / 2), minor=4 * math.sqrt(max(((a + c) - root) / 2, 0.0)),
                theta=0.5 * math.atan2(2 * b, a - c), mean=r["si"] / A, std=math.sqrt(max((A * r["sii"] - r["si"] ** 2) / A ** 2, 0.0)))
