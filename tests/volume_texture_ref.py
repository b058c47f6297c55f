"""Reference of the volume texture (include/mi_unet.h: mi_unet_volume_texture) in numpy.  It shares no code with the
product: the co-occurrence tables are 13 comparisons of the volume with a shifted copy of itself, counted with np.add.at.  Also the
features of mi_unet_volume_texture_derive in Python, and the inputs and cases the CPU and the GPU tests share."""
import functools
import math

import numpy as np

import volume_ref as vr

FIELDS = ("voxels", "imin", "imax", "levels_used", "pairs", "pairs_axial")
STRUCT_BYTES = 32
MAX_LEVELS = 64
MAX_CELLS = 1 << 22
COUNT, WIDTH = "count", "width"
# (dx, dy, dz): the lexicographically positive half of the 26-neighbourhood, by (dz, dy, dx)
OFFSETS = [(dx, dy, dz) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]
FIRST_ORDER = ("mean", "variance", "skewness", "kurtosis", "entropy", "uniformity")
QUANTILES = ("median", "p10", "p90", "mode")
JOINT = ("joint_max", "joint_average", "joint_variance", "joint_entropy", "contrast", "dissimilarity", "inverse_difference",
         "inverse_difference_moment", "angular_second_moment", "correlation")


def levels_of(ids, intensity, m, L, mode, lo, width):
    """(level int64 [D, H, W] (0 outside every component), member bool, comp int64 (r, 0 outside), rows of (voxels, imin, imax))"""
    ids = np.asarray(ids).astype(np.int64)
    v = np.asarray(intensity).astype(np.int64)
    member = (ids >= 1) & (ids <= m)
    comp = np.where(member, ids - 1, 0)
    level = np.zeros(ids.shape, np.int64)
    rows = []
    for r in range(m):
        s = member & (comp == r)
        if not s.any():
            rows.append((0, 0, 0))
            continue
        lo_r, hi_r = int(v[s].min()), int(v[s].max())
        rows.append((int(s.sum()), lo_r, hi_r))
        if mode == COUNT:
            level[s] = (v[s] - lo_r) * L // (hi_r - lo_r + 1)
        else:
            level[s] = np.where(v[s] < lo, 0, np.minimum(L - 1, (v[s] - lo) // width))
    return level, member, comp, rows


def texture(ids, intensity, m, L=32, mode=COUNT, lo=0, width=1, want=("glcm", "axial")):
    """(table: list of m dicts over FIELDS, hist int64 [m, L], glcm int64 [m, L, L] or None, glcm_axial or None) by the definition"""
    level, member, comp, rows = levels_of(ids, intensity, m, L, mode, lo, width)
    d, h, w = level.shape
    hist = np.zeros((m, L), np.int64)
    np.add.at(hist, (comp[member], level[member]), 1)
    glcm = np.zeros((m, L, L), np.int64) if "glcm" in want else None
    axial = np.zeros((m, L, L), np.int64) if "axial" in want else None
    raw = np.asarray(ids).astype(np.int64)
    for dx, dy, dz in OFFSETS:
        # p over [z0:z1, y0:y1, x0:x1] so that p + d stays inside
        zs, ys, xs = slice(0, d - dz), slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
        zq, yq, xq = slice(dz, d), slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx))
        both = member[zs, ys, xs] & (raw[zs, ys, xs] == raw[zq, yq, xq])
        idx = (comp[zs, ys, xs][both], level[zs, ys, xs][both], level[zq, yq, xq][both])
        if glcm is not None:
            np.add.at(glcm, idx, 1)
        if axial is not None and dz == 0:
            np.add.at(axial, idx, 1)
    table = []
    for r in range(m):
        n, lo_r, hi_r = rows[r]
        table.append(dict(voxels=n, imin=lo_r, imax=hi_r, levels_used=int((hist[r] != 0).sum()),
                          pairs=int(glcm[r].sum()) if glcm is not None else 0, pairs_axial=int(axial[r].sum()) if axial is not None else 0))
    return table, hist, glcm, axial


def assert_equal(got, want, what=""):
    """(table VTEXTURE_DTYPE [m], hist, glcm, glcm_axial) of the binding against texture(): every field and every cell"""
    table, hist, glcm, axial = got
    rtable, rhist, rglcm, raxial = want
    assert table.shape == (len(rtable),), (what, table.shape, len(rtable))
    for f in FIELDS:
        col = np.array([r[f] for r in rtable], np.int64)
        assert np.array_equal(table[f].astype(np.int64), col), (what, f, np.flatnonzero(table[f] != col)[:5].tolist(),
                                                                 table[f][table[f] != col][:5].tolist(), col[table[f] != col][:5].tolist())
    for name, a, b in (("hist", hist, rhist), ("glcm", glcm, rglcm), ("glcm_axial", axial, raxial)):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == np.uint32 and a.shape == b.shape, (what, name, a.shape, b.shape)
            bad = np.argwhere(a.astype(np.int64) != b)
            assert bad.size == 0, (what, name, len(bad), bad[:5].tolist())


def same_bytes(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def derive(row, hist, glcm=None):
    """mi_unet_volume_texture_derive's features in Python; "bound" holds, for the two features whose sums cancel, the sum of the
    absolute terms over the same denominator"""
    hist = [int(v) for v in np.asarray(hist).reshape(-1)]
    L, n = len(hist), int(row["voxels"])
    p = [c / n for c in hist]
    mu = math.fsum((l + 1) * p[l] for l in range(L))
    m2, m3, m4 = (math.fsum(p[l] * (l + 1 - mu) ** k for l in range(L)) for k in (2, 3, 4))
    m3_abs = math.fsum(p[l] * abs(l + 1 - mu) ** 3 for l in range(L))
    out = dict(mean=mu, variance=m2, skewness=m3 / m2 ** 1.5 if m2 > 0 else 0.0, kurtosis=m4 / m2 ** 2 - 3.0 if m2 > 0 else 0.0,
               entropy=-math.fsum(q * math.log2(q) for q in p if q > 0), uniformity=math.fsum(q * q for q in p),
               mode=1 + max(range(L), key=lambda l: (hist[l], -l)))
    bound = dict(skewness=m3_abs / m2 ** 1.5 if m2 > 0 else 0.0)
    cum = np.cumsum(hist)
    for name, num in (("median", 5), ("p10", 1), ("p90", 9)):
        out[name] = 1 + int(np.argmax(cum >= -((-n * num) // 10)))
    for k in JOINT:
        out[k] = float("nan")
    if glcm is not None and int(np.asarray(glcm).sum()) > 0:
        g = np.asarray(glcm).astype(np.int64).reshape(L, L)
        pairs = int(g.sum())
        sym = (g + g.T).tolist()
        P = [[sym[i][j] / (2 * pairs) for j in range(L)] for i in range(L)]
        cells = [(i, j, P[i][j]) for i in range(L) for j in range(L)]
        ja = math.fsum((i + 1) * q for i, j, q in cells)
        jv = math.fsum((i + 1 - ja) ** 2 * q for i, j, q in cells)
        cor = math.fsum((i + 1 - ja) * (j + 1 - ja) * q for i, j, q in cells)
        out.update(joint_max=max(q for _, _, q in cells), joint_average=ja, joint_variance=jv,
                   joint_entropy=-math.fsum(q * math.log2(q) for _, _, q in cells if q > 0),
                   contrast=math.fsum((i - j) ** 2 * q for i, j, q in cells), dissimilarity=math.fsum(abs(i - j) * q for i, j, q in cells),
                   inverse_difference=math.fsum(q / (1 + abs(i - j)) for i, j, q in cells),
                   inverse_difference_moment=math.fsum(q / (1 + (i - j) ** 2) for i, j, q in cells),
                   angular_second_moment=math.fsum(q * q for _, _, q in cells), correlation=cor / jv if jv > 0 else float("nan"))
        bound["correlation"] = math.fsum(abs((i + 1 - ja) * (j + 1 - ja)) * q for i, j, q in cells) / jv if jv > 0 else 0.0
    out["bound"] = bound
    return out


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
HARALICK = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]], np.uint16)       # Haralick 1973, fig. 3
HARALICK_HORIZONTAL = [[4, 2, 1, 0], [2, 4, 0, 0], [1, 0, 6, 1], [0, 0, 1, 2]]                  # its P_H: G + G^T over (1, 0)


def noisy(shape, seed):
    """u16 [D, H, W] from a seeded generator: a twentieth of the voxels 0, a twentieth 65535, the rest uniform"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, shape, dtype=np.int64)
    pick = rng.random(shape)
    v[pick < 0.05] = 0
    v[pick > 0.95] = 65535
    return v.astype(np.uint16)


def smooth(shape, seed):
    """u16 [D, H, W]: a ramp along all three axes plus small seeded noise: neighbours mostly share a level"""
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape)
    return (1000 + 37 * x + 53 * y + 211 * z + rng.integers(0, 40, shape)).astype(np.uint16)


def scattered(m=6):
    """ids per voxel drawn from -1 .. m + 1: 0, -1 and m + 1 belong to nothing"""
    return np.random.default_rng(12).integers(-1, m + 2, (5, 19, 70)).astype(np.int32)


def closed_form_pairs(d, h, w, offsets=None):
    return sum((d - abs(dz)) * (h - abs(dy)) * (w - abs(dx)) for dx, dy, dz in (OFFSETS if offsets is None else offsets))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids int32 [D,H,W], intensity u16, m, keyword arguments of the call)"""
    out = {}
    har = HARALICK.reshape(4, 1, 4)
    out["haralick_width"] = (np.ones((4, 1, 4), np.int32), har, 1, dict(levels=4, mode=WIDTH, lo=0, width=1))
    out["haralick_count"] = (np.ones((4, 1, 4), np.int32), har, 1, dict(levels=4, mode=COUNT))
    for shape, conn, k in (((7, 40, 72), 26, 1), ((16, 24, 130), 6, 2)):
        _, _, found, _, ids = vr.noise_ref(shape, conn)         # (cap 256: a plane with more components marks their voxels -1)
        ids, m = np.ascontiguousarray(ids[k]), min(int(found[k]), 256)
        for kind, inten in (("noisy", noisy(shape, 200 + conn)), ("smooth", smooth(shape, 300 + conn))):
            for L in (8, 32, 64):
                out[f"noise{shape}c{conn}_{kind}_L{L}_count"] = (ids, inten, m, dict(levels=L, mode=COUNT))
                out[f"noise{shape}c{conn}_{kind}_L{L}_width"] = (ids, inten, m, dict(levels=L, mode=WIDTH, lo=3000 if kind == "noisy" else 1500,
                                                                                      width=(60000 if kind == "noisy" else 8000) // L))
    n1 = vr.noise_ref((1, 48, 80), 6)
    out["D1"] = (np.ascontiguousarray(n1[4][1]), noisy((1, 48, 80), 21), min(int(n1[2][1]), 256), dict(levels=16))
    out["H1"] = (np.ones((6, 1, 70), np.int32), noisy((6, 1, 70), 22), 1, dict(levels=16))
    out["one_voxel_volume"] = (np.ones((1, 1, 1), np.int32), np.full((1, 1, 1), 9, np.uint16), 1, dict())
    for value in (1234, 65535):
        out[f"constant{value}"] = (np.ones((5, 33, 65), np.int32), np.full((5, 33, 65), value, np.uint16), 1, dict())
    z, y, x = np.indices((6, 20, 96))
    out["two_in_a_slab"] = ((1 + y % 2).astype(np.int32), smooth((6, 20, 96), 23), 2, dict(levels=8))
    out["checkerboard"] = ((1 + (x + y + z) % 2).astype(np.int32), noisy((6, 20, 96), 24), 2, dict(levels=8))
    sc = scattered()
    out["scattered"] = (sc, noisy(sc.shape, 25), 6, dict(levels=32))
    crowded, m = vr.crowded_ids()                               # more ids in a segment than a wave reduces; a span that ends mid-segment
    out["crowded_segment"] = (crowded, smooth(crowded.shape, 41), m, dict(levels=8))
    _, _, found, _, ids16 = vr.noise_ref((16, 24, 130), 6)
    out["m4096_L32"] = (np.ascontiguousarray(ids16[2]), noisy((16, 24, 130), 26), 4096, dict(levels=32))
    out["m1024_L64"] = (np.ascontiguousarray(ids16[2]), smooth((16, 24, 130), 27), 1024, dict(levels=64, mode=WIDTH, lo=2000, width=100))
    # width mode clamps at both ends: values below lo (level 0) and beyond the top bin (level L - 1); component 2 is one voxel
    ids = np.ones((3, 9, 70), np.int32)
    ids[1, 4, 33] = 2
    inten = (np.arange(3 * 9 * 70, dtype=np.int64).reshape(3, 9, 70) * 37 % 4000).astype(np.uint16)
    out["width_clamped"] = (ids, inten, 2, dict(levels=16, mode=WIDTH, lo=1000, width=100))
    # the largest side on each axis: the longest tile grid the pair kernel walks along it; two ids that change every 100 voxels
    for axis, shape in enumerate(((8192, 1, 1), (1, 8192, 1), (1, 1, 8192))):
        out[f"side8192_{'DHW'[axis]}"] = ((1 + np.arange(8192) // 100 % 2).astype(np.int32).reshape(shape), noisy(shape, 40 + axis), 2, dict(levels=8))
    base = out["noise(7, 40, 72)c26_noisy_L8_count"]
    for name, want in (("no_glcm", ("axial",)), ("no_axial", ("glcm",)), ("hist_only", ())):
        out[name] = (base[0], base[1], base[2], dict(levels=8, want=want))
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    ids, inten, m, kw = cases()[name]
    kw = dict(kw)
    return texture(ids, inten, m, kw.pop("levels", 32), kw.pop("mode", COUNT), kw.pop("lo", 0), kw.pop("width", 1), kw.pop("want", ("glcm", "axial")))


def call(fn, name):
    """a binding entry point (Engine.volume_texture or binding.volume_texture_host) on the case"""
    ids, inten, m, kw = cases()[name]
    return fn(ids, inten, m, **kw)


def assert_not_degenerate():
    """On this reference alone, what makes each case a test: Haralick's published table; an asymmetric table; a table with at least 1000
    distinct cells; fewer in-plane pairs than pairs in every case with D > 1; the closed forms of the constant volume; clamping at both ends and
    the component of one voxel; a checkerboard that pairs only through diagonal offsets; ids that belong to nothing; rows no voxel fills."""
    for name in ("haralick_width", "haralick_count"):
        table, hist, glcm, axial = case_ref(name)
        assert (axial[0] + axial[0].T).tolist() == HARALICK_HORIZONTAL and hist[0].tolist() == [5, 4, 5, 2], name
        assert (table[0]["imin"], table[0]["imax"], table[0]["pairs_axial"]) == (0, 3, 12)
    big = case_ref("noise(7, 40, 72)c26_noisy_L64_count")
    sizes = [r["voxels"] for r in big[0]]
    top = int(np.argmax(sizes))
    assert len(sizes) == 25 and max(sizes) == 4783 and int((big[2][top] != 0).sum()) >= 1000, (len(sizes), max(sizes), int((big[2][top] != 0).sum()))
    assert not np.array_equal(big[2][top], big[2][top].T)
    for name, (ids, _, m, kw) in cases().items():
        table = case_ref(name)[0]
        if ids.shape[0] > 1 and "glcm" in kw.get("want", ("glcm", "axial")) and "axial" in kw.get("want", ("glcm", "axial")):
            assert all(r["pairs_axial"] <= r["pairs"] for r in table), name          # (equal for a component that lies in one slice)
            plane = ids.shape[1] * ids.shape[2] > 1                  # (a column of single voxels has no in-plane pair)
            assert (0 if plane else -1) < sum(r["pairs_axial"] for r in table) < sum(r["pairs"] for r in table), name
    for value in (1234, 65535):
        table, hist, glcm, axial = case_ref(f"constant{value}")
        assert table[0]["pairs"] == closed_form_pairs(5, 33, 65) == glcm[0, 0, 0] and table[0]["levels_used"] == 1
        assert table[0]["pairs_axial"] == closed_form_pairs(5, 33, 65, [o for o in OFFSETS if o[2] == 0]) == axial[0, 0, 0]
        assert (table[0]["imin"], table[0]["imax"]) == (value, value)
    table, hist, glcm, axial = case_ref("width_clamped")
    ids, inten, _, kw = cases()["width_clamped"]
    assert (inten < kw["lo"]).sum() > 100 and (inten >= kw["lo"] + 16 * kw["width"]).sum() > 100 and hist[0, 0] > 100 and hist[0, 15] > 100
    assert table[1]["voxels"] == 1 and table[1]["pairs"] == 0 and sorted(hist[1].tolist()) == [0] * 15 + [1] and not glcm[1].any()
    assert all(math.isnan(derive(table[1], hist[1], glcm[1])[k]) for k in JOINT)
    ids = cases()["checkerboard"][0]
    table, _, glcm, axial = case_ref("checkerboard")
    assert all(r["pairs"] > 0 for r in table)                           # every pair joins voxels whose offset has an even sum
    d, h, w = ids.shape
    even = [o for o in OFFSETS if sum(o) % 2 == 0]
    assert all(sum(1 for c in o if c) >= 2 for o in even)               # (every one of them is a diagonal)
    assert table[0]["pairs"] + table[1]["pairs"] == closed_form_pairs(d, h, w, even)
    two = case_ref("two_in_a_slab")[0]
    ids2 = cases()["two_in_a_slab"][0]
    assert two[0]["pairs"] + two[1]["pairs"] == closed_form_pairs(*ids2.shape, [o for o in OFFSETS if o[1] == 0])      # rows of other ids between
    sc = cases()["scattered"][0]
    assert {-1, 0, 7} <= set(np.unique(sc).tolist()) and sum(r["voxels"] for r in case_ref("scattered")[0]) == int(((sc >= 1) & (sc <= 6)).sum())
    for axis in "DHW":                                                  # 82 runs of 100 (the last of 92): 99 pairs a run along the one axis
        table = case_ref(f"side8192_{axis}")[0]
        assert table[0]["pairs"] + table[1]["pairs"] == 8192 - 82 and (table[0]["pairs_axial"] > 0) == (axis != "D")
    for name, m, L in (("m4096_L32", 4096, 32), ("m1024_L64", 1024, 64)):
        table = case_ref(name)[0]
        assert m * L * L == MAX_CELLS and len(table) == m and sum(1 for r in table if r["voxels"] == 0) > m // 2
