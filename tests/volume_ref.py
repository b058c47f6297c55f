"""Reference of the volume components (include/mi_unet.h: mi_unet_volume_components) in numpy and plain Python.  It
shares no code with the product: labelling by flood fill over an explicit neighbour list, faces by padded shifts, the order by sorted
on (-voxels, first), filter, table and ids as the header defines them.  Also the inputs and cases the CPU and the GPU tests share."""
import functools

import numpy as np

FIELDS = ("voxels", "first", "x0", "y0", "z0", "x1", "y1", "z1", "kept", "value", "faces_x", "faces_y", "faces_z", "sx", "sy", "sz")
STRUCT_BYTES = 88
MAX_TABLE = 4096
CONNECTIVITIES = (6, 18, 26)


def neighbours(connectivity):
    """the (dz, dy, dx) of every neighbour: at most 1 on every axis, on 1 / up to 2 / up to 3 axes for 6 / 18 / 26"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= (dz != 0) + (dy != 0) + (dx != 0) <= most]


def label(s, connectivity):
    """int32 [D, H, W]: -1 outside bool volume s, else the index of the voxel's component; components are numbered in the raster order
    of their first voxels.  A flood fill from every unvisited voxel, on a volume padded by one so that no step needs a bounds test."""
    d, h, w = s.shape
    pad = np.zeros((d + 2, h + 2, w + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = s
    ph, pw = h + 2, w + 2
    steps = [dz * ph * pw + dy * pw + dx for dz, dy, dx in neighbours(connectivity)]
    todo = bytearray(pad.reshape(-1).astype(np.uint8).tobytes())
    lab = np.full(pad.size, -1, np.int32)
    count = 0
    for start in np.flatnonzero(pad.reshape(-1)).tolist():      # ascending: raster order
        if not todo[start]:
            continue
        todo[start] = 0
        stack, members = [start], [start]
        while stack:
            p = stack.pop()
            for st in steps:
                q = p + st
                if todo[q]:
                    todo[q] = 0
                    stack.append(q)
                    members.append(q)
        lab[members] = count
        count += 1
    return lab.reshape(pad.shape)[1:-1, 1:-1, 1:-1].copy(), count


def faces(s):
    """three int [D, H, W]: per voxel of s the faces perpendicular to x, y, z towards a 6-neighbour that is not in s (outside is not)"""
    p = np.pad(s.astype(bool), 1, constant_values=False)
    c = p[1:-1, 1:-1, 1:-1]
    fx = (c & ~p[1:-1, 1:-1, :-2]).astype(np.int64) + (c & ~p[1:-1, 1:-1, 2:])
    fy = (c & ~p[1:-1, :-2, 1:-1]).astype(np.int64) + (c & ~p[1:-1, 2:, 1:-1])
    fz = (c & ~p[:-2, 1:-1, 1:-1]).astype(np.int64) + (c & ~p[2:, 1:-1, 1:-1])
    return fx, fy, fz


def plane(masks, value, connectivity=26, min_voxels=0, keep_largest=0, cap=256, want_ids=True):
    """one plane by the definition -> dict(out, ids, table (list of dicts, cap long), found, kept, comps (all, in order))"""
    masks = np.asarray(masks)
    s = masks == value
    d, h, w = s.shape
    lab, count = label(s, connectivity)
    fx, fy, fz = faces(s)
    z, y, x = np.nonzero(s)
    l = lab[s]
    flat = (z * h * w + y * w + x).astype(np.int64)
    comps = []
    if count:
        vox = np.bincount(l, minlength=count)

        def total(v):
            out = np.zeros(count, np.int64)
            np.add.at(out, l, v.astype(np.int64))
            return out

        def lowest(v):
            out = np.full(count, np.iinfo(np.int64).max, np.int64)
            np.minimum.at(out, l, v.astype(np.int64))
            return out

        def highest(v):
            out = np.full(count, -1, np.int64)
            np.maximum.at(out, l, v.astype(np.int64))
            return out

        cols = dict(voxels=vox, first=lowest(flat), x0=lowest(x), y0=lowest(y), z0=lowest(z), x1=highest(x), y1=highest(y), z1=highest(z),
                    faces_x=total(fx[s]), faces_y=total(fy[s]), faces_z=total(fz[s]), sx=total(x), sy=total(y), sz=total(z))
        comps = [dict({n: int(cols[n][c]) for n in cols}, value=int(value), kept=0, label=c) for c in range(count)]
    comps = sorted(comps, key=lambda c: (-c["voxels"], c["first"]))
    for r, c in enumerate(comps):
        c["kept"] = int(c["voxels"] >= min_voxels and (keep_largest == 0 or r < keep_largest))
    rank = np.zeros(count + 1, np.int64)
    keep = np.zeros(count + 1, bool)
    for r, c in enumerate(comps):
        rank[c["label"]], keep[c["label"]] = r, bool(c["kept"])
    lab1 = np.where(lab < 0, count, lab)                        # the extra entry: not kept
    kept_vox = keep[lab1]
    out = np.where(kept_vox, value, 0).astype(np.uint8)
    ids = np.where(kept_vox, np.where(rank[lab1] < cap, rank[lab1] + 1, -1), 0).astype(np.int32) if want_ids else None
    zero = {n: 0 for n in FIELDS}
    table = [{n: c[n] for n in FIELDS} for c in comps[:cap]] + [zero] * max(0, cap - len(comps))
    return dict(out=out, ids=ids, table=table, found=count, kept=sum(c["kept"] for c in comps), comps=comps, labels=lab)


def components(masks, values, connectivity=26, min_voxels=0, keep_largest=0, cap=256):
    """all planes: (out u8 [n,D,H,W], table list [n][cap] of dicts, found [n], kept [n], ids int32 [n,D,H,W])"""
    ps = [plane(masks, v, connectivity, min_voxels, keep_largest, cap) for v in values]
    return (np.stack([p["out"] for p in ps]), [p["table"] for p in ps], [p["found"] for p in ps], [p["kept"] for p in ps],
            np.stack([p["ids"] for p in ps]))


def assert_equal(got, want, what=""):
    """(out, table, found, kept, ids) of the binding against components(): every byte and every field"""
    out, table, found, kept, ids = got
    rout, rtable, rfound, rkept, rids = want
    assert list(found) == list(rfound), (what, "found", list(found), rfound)
    assert list(kept) == list(rkept), (what, "kept", list(kept), rkept)
    assert np.array_equal(out, rout), (what, "out", int((out != rout).sum()))
    if ids is not None:
        assert np.array_equal(ids, rids), (what, "ids", int((ids != rids).sum()))
    assert table.shape == (len(rtable), len(rtable[0])), (what, table.shape)
    for k, rows in enumerate(rtable):
        for f in FIELDS:
            want_col = np.array([r[f] for r in rows], np.int64)
            assert np.array_equal(table[k][f].astype(np.int64), want_col), (what, "plane", k, f,
                                                                           np.flatnonzero(table[k][f] != want_col)[:5].tolist())


def derive(c, spacing):
    """mi_unet_volume_derive's arithmetic in Python floats"""
    sx, sy, sz = (float(v) for v in spacing)
    n = float(c["voxels"])
    return dict(volume_mm3=n * sx * sy * sz,
                surface_mm2=float(c["faces_x"]) * sy * sz + float(c["faces_y"]) * sx * sz + float(c["faces_z"]) * sx * sy,
                cx_mm=(float(c["sx"]) / n + 0.5) * sx, cy_mm=(float(c["sy"]) / n + 0.5) * sy, cz_mm=(float(c["sz"]) / n + 0.5) * sz,
                extent_x_mm=float(c["x1"] - c["x0"] + 1) * sx, extent_y_mm=float(c["y1"] - c["y0"] + 1) * sy,
                extent_z_mm=float(c["z1"] - c["z0"] + 1) * sz)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
NOISE_SHAPES = ((7, 40, 72), (3, 64, 64), (16, 24, 130), (1, 48, 80))
NOISE_VALUES = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def smooth_noise(shape, seed=7):
    """u8 [D, H, W] in 0 .. 3: uniform noise averaged twice over the 6 neighbours with wrap-around, cut at the 0.35 / 0.55 / 0.8 quantiles,
    4 % of the voxels reset to 0"""
    rng = np.random.default_rng(seed)
    f = rng.random(shape)
    for _ in range(2):
        f = (f + sum(np.roll(f, sh, ax) for ax in range(3) for sh in (-1, 1))) / 7.0
    cuts = np.quantile(f, (0.35, 0.55, 0.8))
    vol = np.searchsorted(cuts, f).astype(np.uint8)
    vol[rng.random(shape) < 0.04] = 0
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def noise_ref(shape, connectivity):
    """components() of the smooth-noise volume of `shape` for NOISE_VALUES with the default filter and cap 256, computed once"""
    return components(smooth_noise(shape), NOISE_VALUES, connectivity)


@functools.lru_cache(maxsize=None)
def noise_plane(shape, value, connectivity):
    return plane(smooth_noise(shape), value, connectivity, cap=MAX_TABLE, want_ids=False)


def degeneracy(shape, value):
    """per connectivity 6, 18, 26: (found, components that span more than one slice, pairs of components of one size)"""
    rows = []
    for c in CONNECTIVITIES:
        comps = noise_plane(shape, value, c)["comps"]
        sizes = np.bincount([q["voxels"] for q in comps])
        rows.append((len(comps), sum(1 for q in comps if q["z1"] > q["z0"]), int((sizes * (sizes - 1) // 2).sum())))
    return rows


def assert_not_degenerate():
    """The conditions the noise volumes must meet before any implementation is asked, on this reference alone.  For every 3-D shape and
    value: the three connectivities give three different counts; under connectivity 6 and under 18 at least 10 components span more than
    one slice and at least 10 pairs of components tie in size; under 26 -- where most of a value's voxels join a few components:
    (7, 40, 72) value 2 has 25 components, 3 of them over several slices -- at least 10 pairs tie for every value and at least 10
    components span slices per shape, over its three values.  The one-slice shape: 18 and 26 agree, 6 differs."""
    for shape in NOISE_SHAPES:
        over26 = 0
        for v in NOISE_VALUES:
            rows = degeneracy(shape, v)
            if shape[0] == 1:
                assert rows[1] == rows[2] and rows[0][0] != rows[1][0], (shape, v, rows)
                continue
            assert len({r[0] for r in rows}) == 3, (shape, v, rows)
            assert all(r[1] >= 10 and r[2] >= 10 for r in rows[:2]) and rows[2][2] >= 10, (shape, v, rows)
            over26 += rows[2][1]
        assert shape[0] == 1 or over26 >= 10, (shape, over26)


def serpentine(d=9, h=33, w=130):
    """a one-voxel-wide path through every other row of every other slice, whole rows joined by one voxel in the row between them at
    alternating ends, slices joined by one voxel in the slice between them where one ends and the next begins (a path through EVERY
    row would touch itself along whole rows: the full volume).  It never touches itself, so it is one component under all three
    connectivities with parent chains as long as the path"""
    vol = np.zeros((d, h, w), np.uint8)
    rows = list(range(0, h, 2))
    x = 0                                                       # where the path enters the next row
    for zi, z in enumerate(range(0, d, 2)):
        ys = rows if zi % 2 == 0 else rows[::-1]
        for j, y in enumerate(ys):
            vol[z, y, :] = 1
            x = w - 1 - x                                       # walked to its other end
            if j + 1 < len(ys):
                vol[z, (y + ys[j + 1]) // 2, x] = 1
        if z + 2 < d:
            vol[z + 1, ys[-1], x] = 1
    return vol


def crowded_stack():
    """u8 [3, 5, 70] of 1050 voxels: six single voxels and a pair of value 1 in row 2 of slice 0, a moat of 0 round them, and one
    component over everything else.  What a wave of the device forms meets in it, all in one input: the 64-voxel segment 128 .. 191
    holds eight components, more than a wave reduces together, so lanes are left to add their own; the large component runs across every
    64-voxel boundary and across voxel 1024, where the second wave's span begins; that span ends after 26 voxels, in the middle of a
    segment; and W = 70 makes the segments straddle rows"""
    v = np.ones((3, 5, 70), np.uint8)
    v[0:2, 1:4, 0:25] = 0
    v[0, 2, [2, 5, 8, 11, 14, 17, 20, 21]] = 1
    return v


@functools.lru_cache(maxsize=None)
def crowded_ids():
    """(ids int32 [3, 5, 70] of crowded_stack under 7.9's numbering, m = 8)"""
    _, _, found, _, ids = components(crowded_stack(), (1,), 26)
    return np.ascontiguousarray(ids[0]), int(found[0])


def edge_cases():
    """name -> (masks u8 [D,H,W], values, expectations dict checked by test_volume_cpu.test_edge_cases_are_what_they_claim)"""
    cases = {}
    v = np.zeros((4, 9, 12), np.uint8)
    v[0:2, 0:3, 0:4] = 1
    v[0:2, 3:6, 4:8] = 1                                        # shares the edge x = 4, y = 3 with the first block, no face
    cases["edge_touch"] = (v, (1,), {6: 2, 18: 1, 26: 1})
    v = np.zeros((5, 9, 12), np.uint8)
    v[0:2, 0:3, 0:4] = 1
    v[2:4, 3:6, 4:8] = 1                                        # shares one corner only
    cases["corner_touch"] = (v, (1,), {6: 2, 18: 2, 26: 1})
    v = np.zeros((3, 5, 7), np.uint8)
    v[0, 1, 6] = 1; v[0, 2, 0] = 1                              # the end of a row and the start of the next one
    v[0, 4, 6] = 1; v[1, 0, 0] = 1                              # the last voxel of a slice and the first of the next one
    v[2, 4, 6] = 1; v[0, 0, 0] = 2                              # the last voxel of plane 0 (value 1) and the first of plane 1 (value 2)
    cases["wraps"] = (v, (1, 2), {6: 5, 18: 5, 26: 5})
    cases["serpentine"] = (serpentine(), (1,), {6: 1, 18: 1, 26: 1})
    cases["full"] = (np.full((5, 11, 70), 3, np.uint8), (3,), {6: 1, 18: 1, 26: 1})
    cases["empty"] = (np.zeros((3, 7, 66), np.uint8), (1, 2), {6: 0, 18: 0, 26: 0})
    v = np.zeros((7, 9, 11), np.uint8)
    v[1:6, 1:8, 1:10] = 1
    v[3, 3:6, 4:7] = 0                                          # a closed cavity of 1 x 3 x 3
    cases["cavity"] = (v, (1,), {6: 1, 18: 1, 26: 1})
    cases["crowded_segment"] = (crowded_stack(), (1,), {6: 8, 18: 8, 26: 8})
    return cases


def tie_case():
    """two components of one size and a smaller one: (volume, its mirror along x).  Both of the pair start in row 1 of slice 0: in the
    volume the flat one (x = 2 .. 4) has the smaller `first`, in the mirror the one that spans two slices has"""
    v = np.zeros((3, 8, 20), np.uint8)
    v[0, 1:3, 2:5] = 1                                          # 6 voxels in slice 0
    v[0:2, 1, 10:13] = 1                                        # 6 voxels over slices 0 and 1
    v[2, 7, 0:4] = 1                                            # 4 voxels
    return v, np.ascontiguousarray(v[:, :, ::-1])


@functools.lru_cache(maxsize=None)
def call_cases():
    """name -> (masks, values, keyword arguments of a call): the filter, table and ids cases of the CPU and the GPU tests"""
    n7, n3, n16 = smooth_noise((7, 40, 72)), smooth_noise((3, 64, 64)), smooth_noise((16, 24, 130))
    tie, mirrored = tie_case()
    found18 = noise_plane((3, 64, 64), 1, 18)["found"]
    return {
        "min_voxels": (n7, NOISE_VALUES, dict(connectivity=26, min_voxels=5)),
        "keep_largest": (n7, NOISE_VALUES, dict(connectivity=18, keep_largest=3)),
        "min_and_keep": (n7, NOISE_VALUES, dict(connectivity=6, min_voxels=4, keep_largest=40)),
        "keep_more_than_found": (n7, NOISE_VALUES, dict(connectivity=26, keep_largest=1000)),
        "keep_across_a_tie": (tie, (1,), dict(connectivity=26, keep_largest=1)),
        "keep_across_a_tie_mirrored": (mirrored, (1,), dict(connectivity=26, keep_largest=1)),
        "cap_1": (n3, NOISE_VALUES, dict(connectivity=18, keep_largest=20, cap=1)),
        "cap_found": (n3, (1,), dict(connectivity=18, cap=found18)),
        "cap_below_found": (n3, NOISE_VALUES, dict(connectivity=18, min_voxels=2, cap=17)),
        "cap_4096": (n16, NOISE_VALUES, dict(connectivity=6, cap=MAX_TABLE)),
    }


@functools.lru_cache(maxsize=None)
def call_ref(name):
    masks, values, kw = call_cases()[name]
    return components(masks, values, **kw)
