"""Reference of the volume neighbourhoods (include/mi_unet.h: mi_unet_volume_nbhood) in numpy.  It shares no code with
the product: levels come from volume_texture_ref's rule, the neighbourhoods are sums over 26 shifted copies of the key stack, the
distance is the number of 6-connected (in a slice: 4-connected) erosions a voxel of a component survives, computed per component and
never by a scan, zones are volume_ref.label at connectivity 26 per key as volume_zones_ref takes them.  Also the features of
mi_unet_volume_nbhood_derive in Python, and the inputs and cases the CPU and the GPU tests share."""
import functools
import math

import numpy as np

import volume_ref as vr
import volume_texture_ref as tx
import volume_zones_ref as vz

FIELDS = ("voxels", "imin", "imax", "valid", "valid_axial", "zones", "deepest", "deepest_axial", "clamped", "clamped_axial", "dependence_max")
TABLES = ("ngt_count", "ngt_diff", "dep", "ngt_count_axial", "ngt_diff_axial", "dep_axial", "dzm", "dzm_axial")
WANT = ("ngt", "dep", "ngt_axial", "dep_axial", "dzm", "dzm_axial")
ASKED = {"ngt_count": "ngt", "ngt_diff": "ngt", "dep": "dep", "ngt_count_axial": "ngt_axial", "ngt_diff_axial": "ngt_axial", "dep_axial": "dep_axial",
         "dzm": "dzm", "dzm_axial": "dzm_axial"}
NGTDM = ("coarseness", "contrast", "busyness", "complexity", "strength")
STRUCT_BYTES, OPTS_BYTES, FEATURE_BYTES = 44, 24, 304
MAX_DIST = 4096
MAX_CELLS = tx.MAX_CELLS
COUNT, WIDTH = tx.COUNT, tx.WIDTH
N26 = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def _shifted(pad, shape, dx, dy, dz):
    d, h, w = shape
    return pad[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def neighbourhoods(key, alpha):
    """per voxel (c, S, k) over N26 and over N8, int64 [D, H, W] each: sums over shifted copies of the key stack, padded with 0"""
    pad = np.pad(key, 1)
    comp, level = key >> 8, key & 255
    full = [np.zeros(key.shape, np.int64) for _ in range(3)]
    axial = [np.zeros(key.shape, np.int64) for _ in range(3)]
    for dx, dy, dz in N26:
        q = _shifted(pad, key.shape, dx, dy, dz)
        same = (key != 0) & ((q >> 8) == comp)
        ql = q & 255
        terms = (same, np.where(same, ql, 0), same & (np.abs(ql - level) <= alpha))
        for acc in (full, axial) if dz == 0 else (full,):
            for a, t in zip(acc, terms):
                a += t
    return full, axial


def _erosions(mask, steps):
    """int64: how many erosions by `steps` (outside the array counts as background) every voxel of bool `mask` survives, itself included"""
    dist = np.zeros(mask.shape, np.int64)
    cur = mask.copy()
    while cur.any():
        dist += cur
        pad = np.pad(cur, 1)
        nxt = cur.copy()
        for dx, dy, dz in steps:
            nxt &= _shifted(pad, cur.shape, dx, dy, dz)
        cur = nxt
    return dist


STEPS6 = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def distances(key, want_full=True, want_axial=True):
    """(d, d_axial) int64 [D, H, W], 0 outside every component: per component, inside its bounding box grown by nothing (the box's own
    border is either the volume's or holds voxels of something else, and what lies beyond the box is not of the component either)"""
    comp = key >> 8
    d = np.zeros(key.shape, np.int64) if want_full else None
    da = np.zeros(key.shape, np.int64) if want_axial else None
    for r in np.unique(comp[comp != 0]).tolist():
        mask = comp == r
        zz, yy, xx = np.nonzero(mask)
        box = (slice(zz.min(), zz.max() + 1), slice(yy.min(), yy.max() + 1), slice(xx.min(), xx.max() + 1))
        sub = mask[box]
        if want_full:
            d[box] += _erosions(sub, STEPS6)
        if want_axial:
            da[box] += _erosions(sub, STEPS6[:4])
    return d, da


def nbhood(ids, intensity, m, levels=32, mode=COUNT, lo=0, width=1, alpha=0, max_dist=32, want=WANT):
    """(table: list of m dicts over FIELDS, dict over TABLES of int64 arrays or None) by the definition"""
    L, Dm = levels, max_dist
    key, rows = vz.keys_of(ids, intensity, m, L, mode, lo, width)
    table = [dict(dict.fromkeys(FIELDS, 0), voxels=n, imin=a, imax=b) for n, a, b in rows]
    tabs = dict.fromkeys(TABLES)
    member = key != 0
    r, l = (key[member] >> 8) - 1, key[member] & 255
    if set(want) & {"ngt", "dep", "ngt_axial", "dep_axial"}:
        full, axial = neighbourhoods(key, alpha)
        for suffix, (c, s, k), cols in (("", full, 27), ("_axial", axial, 9)):
            c, s, k = c[member], s[member], k[member]
            if "ngt" + suffix in want:
                count, diff = np.zeros((m, L, cols), np.int64), np.zeros((m, L, cols), np.int64)
                np.add.at(count, (r, l, c), 1)
                np.add.at(diff, (r, l, c), np.abs(c * l - s))
                tabs["ngt_count" + suffix], tabs["ngt_diff" + suffix] = count, diff
                for i in range(m):
                    table[i]["valid" + suffix] = int(count[i, :, 1:].sum())
            if "dep" + suffix in want:
                dep = np.zeros((m, L, cols), np.int64)
                np.add.at(dep, (r, l, k), 1)
                tabs["dep" + suffix] = dep
                if not suffix:
                    for i in range(m):
                        used = np.flatnonzero(dep[i].sum(axis=0))
                        table[i]["dependence_max"] = int(used.max()) + 1 if used.size else 0
    if "dzm" in want or "dzm_axial" in want:
        d, da = distances(key, "dzm" in want, "dzm_axial" in want)
        zone_of = np.full(key.shape, -1, np.int64)              # a number per zone over all keys
        zone_key = []
        for k in np.unique(key[member]).tolist():
            lab, count = vr.label(key == k, 26)
            zone_of[lab >= 0] = lab[lab >= 0] + len(zone_key)
            zone_key += [k] * count
        zone_key = np.array(zone_key, np.int64)
        zr, zl = (zone_key >> 8) - 1, zone_key & 255
        for i in range(m):
            table[i]["zones"] = int((zr == i).sum())
        for name, dist in (("dzm", d), ("dzm_axial", da)):
            if name not in want:
                continue
            near = np.full(len(zone_key), 1 << 30, np.int64)
            np.minimum.at(near, zone_of[member], dist[member])
            tab = np.zeros((m, L, Dm), np.int64)
            np.add.at(tab, (zr, zl, np.minimum(near, Dm) - 1), 1)
            tabs[name] = tab
            suffix = name[3:]
            for i in range(m):
                table[i]["clamped" + suffix] = int((near[zr == i] > Dm).sum())
                mine = (key >> 8) == i + 1
                table[i]["deepest" + suffix] = int(dist[mine].max()) if table[i]["voxels"] else 0
    return table, tabs


def assert_equal(got, want, what=""):
    """(table VNBHOOD_DTYPE [m], dict of tables) of the binding against nbhood(): every field and every cell"""
    table, tabs = got
    rtable, rtabs = want
    assert table.shape == (len(rtable),), (what, table.shape, len(rtable))
    for f in FIELDS:
        col = np.array([r[f] for r in rtable], np.int64)
        assert np.array_equal(table[f].astype(np.int64), col), (what, f, np.flatnonzero(table[f] != col)[:5].tolist(),
                                                                 table[f][table[f] != col][:5].tolist(), col[table[f] != col][:5].tolist())
    for name in TABLES:
        a, b = tabs[name], rtabs[name]
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == (np.uint64 if "diff" in name else np.uint32) and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
            bad = np.argwhere(a.astype(np.int64) != b)
            assert bad.size == 0, (what, name, len(bad), bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def same_bytes(a, b):
    (ta, da), (tb, db) = a, b
    return ta.tobytes() == tb.tobytes() and all((da[n] is None and db[n] is None) or (da[n] is not None and db[n] is not None and
                                                                                      da[n].tobytes() == db[n].tobytes()) for n in TABLES)


# ---- the features in Python ----------------------------------------------------------------------------------------------------------------
def ngtdm(count, diff):
    """the five features from one component's rows [L, cols], sums exactly rounded"""
    count, diff = np.asarray(count).astype(np.int64), np.asarray(diff).astype(np.int64)
    L, cols = count.shape
    n = [int(count[l, 1:].sum()) for l in range(L)]
    s = [math.fsum(int(diff[l, c]) / c for c in range(1, cols)) for l in range(L)]
    N = sum(n)
    if N == 0:
        return dict.fromkeys(NGTDM, float("nan"))
    used = [i for i in range(L) if n[i]]
    p = [v / N for v in n]
    ps, ss = math.fsum(p[i] * s[i] for i in used), math.fsum(s[i] for i in used)
    G = len(used)
    busy = math.fsum(abs((i + 1) * p[i] - (j + 1) * p[j]) for i in used for j in used)
    return dict(coarseness=1e6 if ps == 0 else 1 / ps,
                contrast=0.0 if G == 1 else math.fsum(p[i] * p[j] * (i - j) ** 2 for i in used for j in used) / (G * (G - 1)) * ss / N,
                busyness=0.0 if busy == 0 else ps / busy,
                complexity=math.fsum(abs(i - j) * (p[i] * s[i] + p[j] * s[j]) / (p[i] + p[j]) for i in used for j in used) / N,
                strength=0.0 if ss == 0 else math.fsum((p[i] + p[j]) * (i - j) ** 2 for i in used for j in used) / ss)


def matrix(row, voxels):
    """volume_zones_ref.features over the cells of one [L, columns] matrix (j = column + 1) with sum p^2 added; None: an absent matrix"""
    cells = [] if row is None else vz.run_cells(row)
    f = vz.features(cells, voxels, 1)
    N = sum(c for _, _, c in cells)
    f["energy"] = math.fsum((c / N) ** 2 for _, _, c in cells) if N else float("nan")
    return f


def derive(row, rows, axial=False):
    """mi_unet_volume_nbhood_derive in Python: row = the entry as a dict, rows = the component's rows over TABLES"""
    sfx = "_axial" if axial else ""
    count, diff = rows.get("ngt_count" + sfx), rows.get("ngt_diff" + sfx)
    out = dict.fromkeys(NGTDM, float("nan")) if count is None else ngtdm(count, diff)
    dep = matrix(rows.get("dep" + sfx), row["voxels"])
    out["dependence_energy"] = dep.pop("energy")
    out["ngldm"] = dep
    out["gldzm"] = matrix(rows.get("dzm" + sfx), row["voxels"])
    out["gldzm"].pop("energy")
    return out


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
HAND = np.array([[1, 2, 2, 3], [1, 2, 3, 3], [4, 2, 4, 1], [4, 1, 2, 3]], np.uint16) - 1            # levels from 0
# The 4 x 4 image as one slice, 8 neighbours a pixel (values below are the levels from 1, as printed in the issue; |c l - S| is the same
# for levels from 0).  Pixel by pixel, row by row, (value: c, sum of the neighbours -> |c value - sum|):
#   row 0: 1: 3, 1+2+2=5 -> 2 | 2: 5, 1+2+1+2+3=9 -> 1 | 2: 5, 2+3+2+3+3=13 -> 3 | 3: 3, 2+3+3=8 -> 1
#   row 1: 1: 5, 1+2+2+4+2=11 -> 6 | 2: 8, 1+2+2+1+3+4+2+4=19 -> 3 | 3: 8, 2+2+3+2+3+2+4+1=19 -> 5 | 3: 5, 2+3+3+4+1=13 -> 2
#   row 2: 4: 5, 1+2+2+4+1=10 -> 10 | 2: 8, 1+2+3+4+4+4+1+2=21 -> 5 | 4: 8, 2+3+3+2+1+1+2+3=17 -> 15 | 1: 5, 3+3+4+2+3=15 -> 10
#   row 3: 4: 3, 4+2+1=7 -> 5 | 1: 5, 4+2+4+4+2=16 -> 11 | 2: 5, 2+4+1+1+3=11 -> 1 | 3: 3, 4+1+2=7 -> 2
# n = (4, 5, 4, 3) pixels of value 1 .. 4, all valid.  s_i = sum of |..| / c:
#   value 1: 2/3 + 6/5 + 10/5 + 11/5 = 91/15;  value 2: 1/5 + 3/5 + 3/8 + 5/8 + 1/5 = 2;  value 3: 1/3 + 5/8 + 2/5 + 2/3 = 81/40;
#   value 4: 10/5 + 15/8 + 5/3 = 133/24.
# Dependence at alpha = 0, j = 1 + the neighbours of the pixel's own value:
#   row 0: 1: j 2 | 2: j 3 | 2: j 3 | 3: j 3;  row 1: 1: j 2 | 2: j 4 | 3: j 3 | 3: j 3;  row 2: 4: j 2 | 2: j 3 | 4: j 1 | 1: j 1;
#   row 3: 4: j 2 | 1: j 1 | 2: j 2 | 3: j 1.
HAND_N = [4, 5, 4, 3]
HAND_S = [(91, 15), (2, 1), (81, 40), (133, 24)]
HAND_DEP = {(0, 1): 2, (0, 2): 2, (1, 2): 1, (1, 3): 3, (1, 4): 1, (2, 1): 1, (2, 3): 3, (3, 1): 1, (3, 2): 2}      # (level from 0, j) -> count
HAND_FEATURES = dict(coarseness=0.27122474925836, contrast=0.18065863715277, busyness=1.13445512820512, complexity=5.20294725529100,
                     strength=1.21535181236673)


def solid_box():
    """ids int32 [11, 21, 150]: a box of 9 x 19 x 141 voxels one voxel inside the volume: more than two of 7.15's 4 x 8 x 64 tiles on every axis"""
    ids = np.zeros((11, 21, 150), np.int32)
    ids[1:10, 1:20, 4:145] = 1
    return ids


def hollow_shell():
    """ids int32 [9, 19, 72]: a box whose inner box is empty: the distance is to the cavity as well"""
    ids = np.zeros((9, 19, 72), np.int32)
    ids[0:9, 1:18, 2:70] = 1
    ids[3:6, 6:13, 4:68] = 0
    return ids


def diagonal_line():
    """ids int32 [9, 19, 140]: one voxel per step along (1, 1, 1), through the corner (4, 8, 64) of 7.15's tiles: its voxels meet only
    through corners of the 26-neighbourhood"""
    ids = np.zeros((9, 19, 140), np.int32)
    for t in range(9):
        ids[t, 4 + t, 60 + t] = 1
    return ids


def depth_boxes(Dm):
    """(ids int32 [2 Dm + 3, 2 Dm + 3, 3 (2 Dm + 4)], intensity): three cubes of one id in the corner z = y = 0, of sides 2 Dm - 3,
    2 Dm - 1 and 2 Dm + 1, all of one level except the voxel at the centre of each.  That voxel is a zone of its own, Dm - 1, Dm and
    Dm + 1 deep (the volume's faces at z = 0 and y = 0 count as outside); the rest of each cube is a zone of distance 1"""
    side = 2 * Dm + 3
    ids = np.zeros((side, side, 3 * (side + 1)), np.int32)
    inten = np.zeros(ids.shape, np.uint16)
    for b, coat in enumerate((Dm - 2, Dm - 1, Dm)):
        x0 = b * (side + 1)
        n = 2 * coat + 1
        ids[0:n, 0:n, x0:x0 + n] = 1
        inten[coat, coat, x0 + coat] = 1000                     # the core: one voxel, coat + 1 deep
    return ids, inten


def thick_ids(shape):
    """ids int32 from 0 .. 4: a slowly varying field cut into five bands, so that regions of several ids, many voxels thick and with
    curved borders, touch each other (the components of the noise stacks are two voxels deep at most)"""
    z, y, x = np.indices(shape)
    f = np.sin(x / 9.0) + np.sin(y / 5.0 + z / 3.0) + 0.5 * np.sin((x + y) / 13.0 - z / 2.0)
    return np.clip(np.floor((f + 2.5) * 0.9), 0, 4).astype(np.int32)


def interleaved():
    """ids int32 [3, 9, 72]: ids 1 and 2 alternate in blocks of 5 along x, so several changes fall inside one 64-lane row"""
    x = np.indices((3, 9, 72))[2]
    return (1 + (x // 5) % 2).astype(np.int32)


def parity_volume(shape=(40, 512, 512)):
    z, y, x = np.indices(shape, np.int16, sparse=True)
    return np.ones(shape, np.int32), (((z + y + x) & 1) * 63).astype(np.uint16)


def parity_closed_form(shape=(40, 512, 512)):
    """The tables of parity_volume() at L = 64, width 1, lo 0, alpha 0, one component, without a neighbourhood sweep: a voxel's
    neighbours inside the volume are a product over the axes, those of the other parity (the other level) are
    (prod (1 + o_a) - prod (1 - o_a)) / 2 with o_a the steps of +-1 that stay inside along axis a; |c l - S| = 63 * (those of the other
    level) at either level, k = the ones of the voxel's own."""
    steps = [np.full(n, 2, np.int64) for n in shape]
    for o in steps:
        o[0] -= 1
        o[-1] -= 1
    oz, oy, ox = np.ix_(*steps)
    z, y, x = np.indices(shape, np.int16, sparse=True)
    level = (((z + y + x) & 1) * 63).astype(np.int64)
    out = {}
    for sfx, c, other in (("", (1 + oz) * (1 + oy) * (1 + ox) - 1, ((1 + oz) * (1 + oy) * (1 + ox) - (1 - oz) * (1 - oy) * (1 - ox)) // 2),
                          ("_axial", (1 + oy) * (1 + ox) - 1 + 0 * oz, ((1 + oy) * (1 + ox) - (1 - oy) * (1 - ox)) // 2 + 0 * oz)):
        cols = 9 if sfx else 27
        cell = (level * cols + c).reshape(-1)
        out["ngt_count" + sfx] = np.bincount(cell, minlength=64 * cols).reshape(1, 64, cols)
        out["ngt_diff" + sfx] = np.rint(np.bincount(cell, weights=(63 * other + 0 * level).reshape(-1).astype(np.float64), minlength=64 * cols)).astype(np.int64).reshape(1, 64, cols)
        out["dep" + sfx] = np.bincount((level * cols + c - other).reshape(-1), minlength=64 * cols).reshape(1, 64, cols)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids int32 [D,H,W], intensity u16, m, keyword arguments of the call)"""
    out = {}
    out["hand_4x4"] = (np.ones((1, 4, 4), np.int32), HAND.reshape(1, 4, 4), 1, dict(levels=4, mode=WIDTH, lo=0, width=1))
    stacks = {}
    for shape, conn, k in (((7, 40, 72), 26, 1), ((16, 24, 130), 6, 2), ((3, 9, 72), 26, 1), ((5, 19, 130), 18, 1)):
        _, _, found, _, ids = vr.noise_ref(shape, conn)         # (cap 256: a plane with more components marks their voxels -1)
        stacks[shape] = (np.ascontiguousarray(ids[k]), min(int(found[k]), 256))
    for shape in ((7, 40, 72), (16, 24, 130)):
        ids, m = stacks[shape]
        for kind, L, mode, alpha in (("smooth", 32, COUNT, 1), ("noisy", 8, WIDTH, 0), ("smooth", 64, WIDTH, 2), ("noisy", 16, COUNT, 0)):
            inten = tx.noisy(shape, 400 + L) if kind == "noisy" else tx.smooth(shape, 500 + L)
            kw = dict(levels=L, mode=mode, alpha=alpha, max_dist=3 if shape[0] == 16 else 32)       # (3: deeper zones are clamped)
            if mode == WIDTH:
                kw.update(lo=3000 if kind == "noisy" else 1500, width=(60000 if kind == "noisy" else 8000) // L)
            out[f"noise{shape}_{kind}_L{L}_{mode}"] = (ids, inten, m, kw)
    for shape, L, Dm in (((7, 40, 72), 8, 2), ((16, 24, 130), 16, 3)):
        out[f"thick{shape}"] = (thick_ids(shape), tx.noisy(shape, 600 + L), 4, dict(levels=L, alpha=1, max_dist=Dm))
    for shape in ((3, 9, 72), (5, 19, 130)):
        ids, m = stacks[shape]
        out[f"noise{shape}"] = (ids, tx.smooth(shape, 31), m, dict(levels=8, alpha=1))
    n1 = vr.noise_ref((1, 48, 80), 6)
    out["D1"] = (np.ascontiguousarray(n1[4][1]), tx.smooth((1, 48, 80), 21), min(int(n1[2][1]), 256), dict(levels=16))
    out["H1"] = (np.ones((6, 1, 70), np.int32), tx.smooth((6, 1, 70), 22), 1, dict(levels=16, alpha=1))
    out["one_voxel_volume"] = (np.ones((1, 1, 1), np.int32), np.full((1, 1, 1), 9, np.uint16), 1, dict())
    box = solid_box()
    out["solid_box"] = (box, np.full(box.shape, 777, np.uint16), 1, dict(levels=4))
    z, y, x = np.indices((5, 9, 72))
    out["two_ids_plane"] = ((1 + (x >= 36)).astype(np.int32), tx.smooth((5, 9, 72), 33), 2, dict(levels=8, alpha=1))
    out["two_ids_interleaved"] = (interleaved(), tx.smooth((3, 9, 72), 34), 2, dict(levels=8))
    out["flush_with_every_face"] = (np.ones((7, 19, 130), np.int32), tx.smooth((7, 19, 130), 35), 1, dict(levels=16, alpha=1))
    shell = hollow_shell()
    out["hollow_shell"] = (shell, tx.smooth(shell.shape, 36), 1, dict(levels=4))
    line = diagonal_line()
    out["diagonal_line"] = (line, np.full(line.shape, 5, np.uint16), 1, dict(levels=4))
    ids, inten = depth_boxes(4)
    out["depth_Dm-1_Dm_Dm+1"] = (ids, inten, 1, dict(levels=2, mode=WIDTH, lo=0, width=500, max_dist=4))
    out["Dm_1"] = (np.ones((5, 9, 72), np.int32), tx.noisy((5, 9, 72), 37), 1, dict(levels=16, max_dist=1))
    one = np.zeros((5, 19, 130), np.int32)
    one[:, 2:17, 10:120] = 1
    out["m1_L64_Dm4096"] = (one, tx.noisy(one.shape, 38), 1, dict(levels=64, max_dist=4096, alpha=3))
    base = out["noise(7, 40, 72)_smooth_L32_count"]
    for alpha in (0, 31):
        out[f"alpha_{alpha}"] = (base[0], base[1], base[2], dict(base[3], alpha=alpha))
    sc = tx.scattered()
    out["scattered"] = (sc, tx.noisy(sc.shape, 25), 6, dict(levels=32, alpha=4))
    ids16, _ = stacks[(16, 24, 130)]
    out["m4096_L32"] = (ids16, tx.noisy((16, 24, 130), 26), 4096, dict(levels=32, max_dist=32))
    wide = np.random.default_rng(14).integers(-1, 1026, (5, 19, 70)).astype(np.int32)
    out["m1024_L64"] = (wide, tx.noisy(wide.shape, 28), 1024, dict(levels=64, max_dist=64, alpha=5))
    small = out["noise(3, 9, 72)"]
    for w in WANT:
        out[f"without_{w}"] = (small[0], small[1], small[2], dict(small[3], want=tuple(v for v in WANT if v != w)))
    out["entry_only"] = (small[0], small[1], small[2], dict(small[3], want=()))
    out["dzm_axial_only"] = (small[0], small[1], small[2], dict(small[3], want=("dzm_axial",)))
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    ids, inten, m, kw = cases()[name]
    return nbhood(ids, inten, m, **kw)


def call(fn, name):
    """a binding entry point (Engine.volume_nbhood or binding.volume_nbhood_host) on the case"""
    ids, inten, m, kw = cases()[name]
    return fn(ids, inten, m, **kw)


def box_deepest(*sides):
    """the deepest voxel of a solid box: the middle of its shortest side"""
    return (min(sides) + 1) // 2


def assert_not_degenerate():
    """On this reference alone, what makes each case a test."""
    table, tabs = case_ref("hand_4x4")
    count, diff, dep = tabs["ngt_count_axial"][0], tabs["ngt_diff_axial"][0], tabs["dep_axial"][0]
    assert count[:, 1:].sum(axis=1).tolist() == HAND_N and np.array_equal(tabs["ngt_count"], np.pad(count, ((0, 0), (0, 18)))[None])
    from fractions import Fraction
    assert [sum(Fraction(int(diff[l, c]), c) for c in range(1, 9)) for l in range(4)] == [Fraction(a, b) for a, b in HAND_S]
    assert {(l, j + 1): int(dep[l, j]) for l, j in np.argwhere(dep).tolist()} == HAND_DEP
    assert table[0]["deepest"] == 1 and table[0]["deepest_axial"] == 2 and tabs["dzm"][0, :, 0].sum() == table[0]["zones"]
    table, tabs = case_ref("one_voxel_volume")
    assert table[0]["valid"] == 0 and tabs["ngt_count"][0, :, 0].sum() == 1 and tabs["dep"][0, :, 0].sum() == 1 and table[0]["deepest"] == 1
    assert table[0]["dependence_max"] == 1 and tabs["dzm"].sum() == 1
    table, tabs = case_ref("solid_box")
    assert tabs["ngt_count"][0, 0, 26] == 7 * 17 * 139 and tabs["dep"][0, 0, 26] == 7 * 17 * 139 and tabs["ngt_diff"].sum() == 0
    assert table[0]["deepest"] == box_deepest(9, 19, 141) == 5 and table[0]["deepest_axial"] == box_deepest(19, 141) == 10 and table[0]["zones"] == 1
    for name in ("two_ids_plane", "two_ids_interleaved"):         # neighbours of another id are not neighbours
        ids, inten, m, kw = cases()[name]
        assert case_ref(name)[1]["ngt_count"][:, :, 26].sum() < nbhood(np.ones_like(ids), inten, m, **kw)[1]["ngt_count"][0, :, 26].sum()
    assert [r["deepest_axial"] for r in case_ref("two_ids_plane")[0]] == [5, 5] and [r["deepest"] for r in case_ref("two_ids_plane")[0]] == [3, 3]
    assert case_ref("two_ids_interleaved")[0][0]["deepest_axial"] == 3       # blocks of five along x
    table, tabs = case_ref("flush_with_every_face")
    assert table[0]["deepest"] == box_deepest(7, 19, 130) and table[0]["deepest_axial"] == box_deepest(19, 130) and table[0]["valid"] == 7 * 19 * 130
    filled = hollow_shell()
    filled[3:6, 6:13, 4:68] = 1
    _, inten, m, kw = cases()["hollow_shell"]
    assert case_ref("hollow_shell")[0][0]["deepest"] == 3 < nbhood(filled, inten, m, **kw)[0][0]["deepest"] == 5
    table, tabs = case_ref("diagonal_line")
    assert tabs["ngt_count"][0, 0].tolist() == [0, 2, 7] + [0] * 24 and table[0]["zones"] == 1 and table[0]["deepest"] == 1 and tabs["ngt_count_axial"][0, 0, 0] == 9
    table, tabs = case_ref("depth_Dm-1_Dm_Dm+1")
    assert tabs["dzm"][0, 1].tolist() == [0, 0, 1, 2] and table[0]["clamped"] == 1 and table[0]["zones"] == 6 and table[0]["deepest"] == 5
    assert tabs["dzm_axial"][0, 1].tolist() == [0, 0, 1, 2] and table[0]["clamped_axial"] == 1
    table, tabs = case_ref("Dm_1")
    assert tabs["dzm"].shape[2] == 1 and sum(r["clamped"] for r in table) > 0
    table, tabs = case_ref("m1_L64_Dm4096")
    assert tabs["dzm"].shape == (1, 64, 4096) and table[0]["clamped"] == 0 and tabs["dzm"][0, :, 1:].sum() > 0
    lo, mid, hi = case_ref("alpha_0"), case_ref("noise(7, 40, 72)_smooth_L32_count"), case_ref("alpha_31")
    assert np.array_equal(hi[1]["dep"], hi[1]["ngt_count"]) and np.array_equal(hi[1]["dep_axial"], hi[1]["ngt_count_axial"])
    assert not np.array_equal(lo[1]["dep"], mid[1]["dep"]) and not np.array_equal(mid[1]["dep"], hi[1]["dep"])
    assert all(np.array_equal(lo[1][n], hi[1][n]) for n in TABLES if "dep" not in n)
    sc = cases()["scattered"][0]
    assert {-1, 0, 7} <= set(np.unique(sc).tolist()) and sum(r["voxels"] for r in case_ref("scattered")[0]) == int(((sc >= 1) & (sc <= 6)).sum())
    assert 4096 * 32 * 32 == MAX_CELLS == 1024 * 64 * 64 and len(case_ref("m4096_L32")[0]) == 4096 and len(case_ref("m1024_L64")[0]) == 1024
    assert sum(1 for r in case_ref("m1024_L64")[0] if r["voxels"]) > 1000
    big = [case_ref(n) for n in cases() if n.startswith("noise(7") or n.startswith("noise(16")]
    assert all(tabs["ngt_diff"].sum() > 0 and tabs["ngt_count"][:, :, 1:].sum() > 0 and max(r["deepest"] for r in t) == 2 for t, tabs in big)
    for t, tabs in (case_ref(n) for n in cases() if n.startswith("thick")):
        assert all(r["clamped"] > 0 and r["clamped_axial"] > 0 and r["deepest"] > 3 and r["deepest_axial"] > r["deepest"] for r in t[:3])
        assert tabs["ngt_count"][:, :, 26].sum() > 1000 and (tabs["dzm"][:, :, 1:].sum(axis=(1, 2)) > 0).all()
    for w in WANT:
        t, tabs = case_ref(f"without_{w}")
        assert [n for n in TABLES if tabs[n] is None] == [n for n in TABLES if ASKED[n] == w]
    t, tabs = case_ref("entry_only")
    assert all(v is None for v in tabs.values()) and all(r["zones"] == 0 and r["valid"] == 0 for r in t) and any(r["voxels"] for r in t)
    t, tabs = case_ref("dzm_axial_only")
    assert any(r["deepest_axial"] > 1 for r in t) and all(r["deepest"] == 0 for r in t) and any(r["zones"] for r in t)
    # the zones are volume_zones_ref's
    ids, inten, m, kw = cases()["noise(3, 9, 72)"]
    assert [r["zones"] for r in case_ref("noise(3, 9, 72)")[0]] == [r["zones"] for r in vz.zones(ids, inten, m, levels=kw["levels"], want_runs=False, want_axial=False)[0]]
