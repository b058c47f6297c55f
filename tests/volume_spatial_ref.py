"""Reference of the volume spatial statistics (include/mi_unet.h: mi_unet_volume_spatial) in numpy.  It shares no code
with the product: the pair sums enumerate all pairs by brute force, every term a double 1 / np.sqrt(d2) times an exact integer, summed
with math.fsum; the peaks enumerate the offsets of the ball of mi_unet_volume_ball directly and compare means as Python integers;
Moran's I and Geary's C are also computed as IBSI writes them, over ordered pairs, mean-centred in float64.  Also the inputs, the
cases and the error bounds the CPU and the GPU tests share."""
import functools
import math

import numpy as np

import volume_ref as vr
from miunet import binding

INT_FIELDS = ("voxels", "searched", "imin", "imax", "centre", "reserved", "gp_at", "lp_at", "sx", "sy", "sz", "si", "sii", "six", "siy",
              "siz", "gp_sum", "gp_n", "lp_sum", "lp_n", "pairs")
SUMS = ("s0", "s1", "s2", "s3")
FIELDS = INT_FIELDS + SUMS
STRUCT_BYTES = 168
INT_BYTES = 136                             # the integer part of an entry; the four doubles follow
MAX_VOXELS_LIMIT = 1 << 20
DEFAULT_MAX_VOXELS = 1 << 17
TILE = 256                                  # the device form's LDS tile (csrc/kernels.h: VSP_TILE)
EPS = float(np.finfo(np.float64).eps)
CHUNK_ELEMS = 4_000_000                     # entries of the pair matrix held at once
PARITY_MAX_VOXELS = 4096                    # the largest component a parity case may hold: P <= 8.4e6, the bound below 1 / (10 P)


def pair_sums(pts, y):
    """((s0, s1, s2, s3), (T0, T1, T2, T3)) over the unordered pairs of the rows of pts (int64 [N, 3], scaled) with y int64 [N]: fsum of
    the per-term doubles, and the sums of their magnitudes"""
    n = pts.shape[0]
    terms = [[], [], [], []]
    rows = max(1, CHUNK_ELEMS // n)
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        d2 = ((pts[i0:i1, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
        upper = np.arange(i0, i1)[:, None] < np.arange(n)[None, :]
        w = 1.0 / np.sqrt(d2[upper].astype(np.float64))
        yi = np.broadcast_to(y[i0:i1, None], d2.shape)[upper]
        yj = np.broadcast_to(y[None, :], d2.shape)[upper]
        terms[0].append(w)
        terms[1].append(w * (yi + yj).astype(np.float64))
        terms[2].append(w * (yi * yj).astype(np.float64))
        terms[3].append(w * ((yi - yj) ** 2).astype(np.float64))
    flat = [np.concatenate(t) if t else np.zeros(0) for t in terms]
    return tuple(math.fsum(t.tolist()) for t in flat), tuple(float(np.abs(t).sum()) for t in flat)


@functools.lru_cache(maxsize=None)
def ball_offsets(units, r):
    """the (dz, dy, dx) of B(r) from mi_unet_volume_ball's element"""
    (ex, ey, ez), elem = binding.volume_ball(units, r)
    dz, dy, dx = np.nonzero(np.asarray(elem).reshape(2 * ez + 1, 2 * ey + 1, 2 * ex + 1))
    return [(int(a) - ez, int(b) - ey, int(c) - ex) for a, b, c in zip(dz, dy, dx)]


def sphere_sums(intensity, units, r):
    """(s, n) int64 [D, H, W]: the intensity sum and the voxel count of every voxel's sphere, one shifted copy per offset of the ball"""
    d, h, w = intensity.shape
    v = intensity.astype(np.int64)
    s, n = np.zeros_like(v), np.zeros_like(v)
    for dz, dy, dx in ball_offsets(tuple(int(u) for u in units), int(r)):
        if abs(dz) >= d or abs(dy) >= h or abs(dx) >= w:
            continue
        dst = tuple(slice(max(0, -o), size - max(0, o)) for o, size in zip((dz, dy, dx), (d, h, w)))
        src = tuple(slice(max(0, o), size - max(0, -o)) for o, size in zip((dz, dy, dx), (d, h, w)))
        s[dst] += v[src]
        n[dst] += 1
    return s, n


def best_mean(idx, s, n):
    """(s, n, index) of the largest s / n over the candidates in ascending index order, ties to the smallest index; Python integers"""
    best = None
    for i in idx:
        si, ni = int(s[i]), int(n[i])
        if best is None or si * best[1] > best[0] * ni:
            best = (si, ni, int(i))
    return best


def spatial(ids, intensity, m, units, max_voxels=DEFAULT_MAX_VOXELS, peak_r=0):
    """the table by the definition: a list of m dicts over FIELDS, and "T": the four sums of |term|"""
    ids, intensity = np.asarray(ids), np.asarray(intensity)
    d, h, w = ids.shape
    ux, uy, uz = (int(u) for u in units)
    s_all, n_all = sphere_sums(intensity, units, peak_r)
    s_flat, n_flat, v_flat = s_all.reshape(-1), n_all.reshape(-1), intensity.reshape(-1).astype(np.int64)
    out = []
    for r in range(m):
        member = ids == r + 1
        row = {f: 0 for f in INT_FIELDS}
        row.update({f: 0.0 for f in SUMS})
        row["T"] = (0.0, 0.0, 0.0, 0.0)
        a = int(member.sum())
        if a == 0:
            out.append(row)
            continue
        z, y, x = (c.astype(np.int64) for c in np.nonzero(member))         # raster order: the index ascends
        idx = z * h * w + y * w + x
        v = v_flat[idx]
        si = int(v.sum())
        c = (2 * si + a) // (2 * a)
        row.update(voxels=a, imin=int(v.min()), imax=int(v.max()), centre=c, sx=int(x.sum()), sy=int(y.sum()), sz=int(z.sum()), si=si,
                   sii=int((v * v).sum()), six=int((v * x).sum()), siy=int((v * y).sum()), siz=int((v * z).sum()))
        row["gp_sum"], row["gp_n"], row["gp_at"] = best_mean(idx, s_flat, n_flat)
        row["lp_sum"], row["lp_n"], row["lp_at"] = best_mean(idx[v == row["imax"]], s_flat, n_flat)
        if 2 <= a <= max_voxels:
            assert a <= PARITY_MAX_VOXELS, (r, a)
            pts = np.stack([x * ux, y * uy, z * uz], axis=1)
            sums, row["T"] = pair_sums(pts, v - c)
            row.update(searched=1, pairs=a * (a - 1) // 2, **dict(zip(SUMS, sums)))
        out.append(row)
    return out


def ibsi_as_written(ids, intensity, r, units):
    """(Moran's I, Geary's C) of component r as IBSI writes them: ordered pairs i != j, w = 1 / distance, mean-centred, float64"""
    member = np.asarray(ids) == r + 1
    z, y, x = (c.astype(np.float64) for c in np.nonzero(member))
    v = np.asarray(intensity)[member].astype(np.float64)
    n = v.size
    pts = np.stack([x * units[0], y * units[1], z * units[2]], axis=1)
    mu = v.mean()
    dev = v - mu
    wsum = cross = diff = 0.0
    rows = max(1, CHUNK_ELEMS // n)
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        dist = np.sqrt(((pts[i0:i1, None, :] - pts[None, :, :]) ** 2).sum(axis=2))
        dist[np.arange(i1 - i0), np.arange(i0, i1)] = np.inf                # i == j takes no part
        wij = 1.0 / dist
        wsum += float(wij.sum())
        cross += float((wij * dev[i0:i1, None] * dev[None, :]).sum())
        diff += float((wij * (v[i0:i1, None] - v[None, :]) ** 2).sum())
    var = float((dev * dev).sum())
    return n / wsum * cross / var, (n - 1) / (2.0 * wsum) * diff / var


def derive(c, units, unit_mm):
    """mi_unet_volume_spatial_derive's arithmetic in Python: exact integer numerators"""
    s = [float(u) * float(unit_mm) for u in units]
    a, si, sii = int(c["voxels"]), int(c["si"]), int(c["sii"])
    nan = float("nan")
    geo = [(int(c[k]) / a + 0.5) * s[i] for i, k in enumerate(("sx", "sy", "sz"))]
    ic = [(int(c[k]) / si + 0.5) * s[i] if si else nan for i, k in enumerate(("six", "siy", "siz"))]
    out = dict(cx_mm=geo[0], cy_mm=geo[1], cz_mm=geo[2], icx_mm=ic[0], icy_mm=ic[1], icz_mm=ic[2],
               com_shift_mm=math.sqrt(sum((p - q) ** 2 for p, q in zip(ic, geo))), integrated_intensity=si * (s[0] * s[1] * s[2]),
               local_peak=int(c["lp_sum"]) / int(c["lp_n"]), global_peak=int(c["gp_sum"]) / int(c["gp_n"]), morans_i=nan, gearys_c=nan)
    var = float(a * sii - si * si) / a
    delta = float(si - int(c["centre"]) * a) / a
    if int(c["searched"]) and var != 0.0:
        s0, s1, s2, s3 = (float(c[k]) for k in SUMS)
        out["morans_i"] = a / (2.0 * s0) * (2.0 * (s2 - delta * s1 + delta * delta * s0)) / var
        out["gearys_c"] = (a - 1.0) / (2.0 * (2.0 * s0)) * (2.0 * s3) / var
        out["morans_scale"] = a / (2.0 * s0) * 2.0 * (abs(s2) + 0.5 * abs(s1) + 0.25 * s0) / var           # the un-cancelled magnitude
    return out


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def assert_ints_equal(table, want, what=""):
    """a VSPATIAL_DTYPE [m] table of the binding against spatial(): every integer field"""
    assert table.shape == (len(want),), (what, table.shape, len(want))
    for f in INT_FIELDS:
        col = np.array([r[f] for r in want], np.int64)
        got = table[f].astype(np.int64)
        assert np.array_equal(got, col), (what, f, np.flatnonzero(got != col)[:5].tolist(), got[got != col][:5].tolist(), col[got != col][:5].tolist())


def assert_sums_near_reference(table, want, what=""):
    """|sum - reference| <= (P + 8) eps T per sum: P terms added in any order differ from their exact sum by at most (P - 1) eps T to
    first order, and a term carries at most 8 roundings (the 4 ulp allowed on w, the conversions, the products).  A component that is
    not searched has four zeros"""
    for r, (got, ref) in enumerate(zip(table, want)):
        for k, f in enumerate(SUMS):
            if not ref["searched"]:
                assert got[f] == 0.0 and got[f].tobytes() == b"\0" * 8, (what, r, f, got[f])
                continue
            bound = (ref["pairs"] + 8) * EPS * ref["T"][k]
            assert abs(float(got[f]) - ref[f]) <= bound, (what, r, f, float(got[f]), ref[f], abs(float(got[f]) - ref[f]), bound)
            assert bound <= abs(ref["T"][k]) / (10.0 * ref["pairs"]) or ref["T"][k] == 0.0, (what, r, f)     # a dropped pair cannot hide


def assert_sums_near_each_other(dev, host, what=""):
    """device against host form where no reference is run: 2 (P + 8) eps T' per sum, T' from s0 and the largest |v - c|"""
    for r, (a, b) in enumerate(zip(dev, host)):
        ymax = float(max(int(b["imax"]) - int(b["centre"]), int(b["centre"]) - int(b["imin"])))
        scale = (1.0, 2.0 * ymax, ymax * ymax, 4.0 * ymax * ymax)
        for k, f in enumerate(SUMS):
            bound = 2.0 * (int(b["pairs"]) + 8) * EPS * float(b["s0"]) * scale[k]
            assert abs(float(a[f]) - float(b[f])) <= bound, (what, r, f, float(a[f]), float(b[f]), bound)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def intensity_for(shape, seed):
    """u16 [D, H, W] from a seeded generator: a tenth of the voxels 0, a tenth 65535, the rest uniform"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, shape, dtype=np.int64)
    pick = rng.random(shape)
    v[pick < 0.1] = 0
    v[pick > 0.9] = 65535
    return v.astype(np.uint16)


ELLIPSOID_VOXELS = 2956                     # P = 4.37e6 pairs: (P + 8) eps = 9.7e-10


def ellipsoid(shape=(12, 24, 30), semi=(6.25, 9.0, 12.75)):
    """ids of the ellipsoid round (6, 12, 15): one component of ELLIPSOID_VOXELS voxels"""
    z, y, x = np.indices(shape).astype(np.float64)
    c = [n / 2.0 for n in shape]
    return ((((z - c[0]) / semi[0]) ** 2 + ((y - c[1]) / semi[1]) ** 2 + ((x - c[2]) / semi[2]) ** 2) <= 1.0).astype(np.int32)


SCATTERED_COUNTS = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def scattered():
    """six ids of 1, 2, TILE - 1, TILE, TILE + 1 and 2 TILE + 1 single voxels, interleaved all over the volume, between them voxels of
    the ids 0, -1 and m + 1, which belong to no component"""
    rng = np.random.default_rng(12)
    shape = (5, 37, 130)
    ids = np.zeros(shape, np.int32)
    take = rng.permutation(ids.size)[:sum(SCATTERED_COUNTS) + 200]
    at = 0
    for r, c in enumerate(SCATTERED_COUNTS):
        ids.reshape(-1)[take[at:at + c]] = r + 1
        at += c
    ids.reshape(-1)[take[at:at + 100]] = -1
    ids.reshape(-1)[take[at + 100:at + 200]] = len(SCATTERED_COUNTS) + 1
    return ids


BLOB_VOXELS = 300


def blob():
    """one component of BLOB_VOXELS voxels: the first of a 4 x 9 x 11 box in raster order"""
    ids = np.zeros((4, 9, 11), np.int32)
    ids.reshape(-1)[:BLOB_VOXELS] = 1
    return ids


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids int32 [D,H,W], intensity u16, m, units, max_voxels or None, peak_r)"""
    out = {}
    ell = ellipsoid()
    out["ellipsoid(7, 7, 50)"] = (ell, intensity_for(ell.shape, 1), 1, (7, 7, 50), None, 62)
    out["ellipsoid(1, 1, 1)"] = (ell, intensity_for(ell.shape, 1), 1, (1, 1, 1), None, 3)
    for si, (shape, conn, k) in enumerate((((7, 40, 72), 26, 2), ((16, 24, 130), 6, 2), ((1, 48, 80), 26, 1))):     # W = 72, W = 130, D = 1
        _, _, found, _, ids = vr.noise_ref(shape, conn)         # (cap 256: a plane with more components marks their voxels -1)
        out[f"noise{shape}c{conn}"] = (np.ascontiguousarray(ids[k]), intensity_for(shape, 100 + si), min(int(found[k]), 256),
                                       (1, 1, 1) if conn == 6 else (7, 7, 50), 1200, 2 if conn == 6 else 20)
    sc = scattered()
    out["scattered"] = (sc, intensity_for(sc.shape, 4), len(SCATTERED_COUNTS), (3, 2, 7), None, 7)
    out["m4096"] = (sc, intensity_for(sc.shape, 4), 4096, (3, 2, 7), 2 * TILE, 3)       # id 7 is a component now; the largest is over the cap
    b = blob()
    for cap in (BLOB_VOXELS, BLOB_VOXELS - 1, 0):
        out[f"blob_cap{cap}"] = (b, intensity_for(b.shape, 5), 1, (2, 2, 5), cap, 4)
    box = np.ones((5, 6, 7), np.int32)
    out["constant"] = (box, np.full(box.shape, 1000, np.uint16), 1, (1, 1, 1), None, 2)
    corner = np.random.default_rng(6).integers(0, 100, (6, 7, 9)).astype(np.uint16)
    corner[-1, -1, -1] = 65535
    out["bright_corner"] = (np.ones(corner.shape, np.int32), corner, 1, (1, 1, 1), None, 2)
    out["peak_r0"] = (b, intensity_for(b.shape, 5), 1, (2, 2, 5), None, 0)
    out["flat_disc"] = (b, intensity_for(b.shape, 5), 1, (2, 2, 9), None, 5)            # ux <= r < uz
    thin = np.ones((3, 5, 40), np.int32)
    out["ball_wider_than_a_side"] = (thin, intensity_for(thin.shape, 8), 1, (1, 1, 1), None, 6)
    z, y, x = np.indices((6, 8, 10))
    out["checkerboard"] = (np.ones((6, 8, 10), np.int32), (((x + y + z) % 2) * 1000 + 100).astype(np.uint16), 1, (1, 1, 1), None, 1)
    out["ramp"] = (np.ones((6, 8, 10), np.int32), (100 * x + 10 * y + 50).astype(np.uint16), 1, (1, 1, 1), None, 1)
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    ids, inten, m, units, cap, peak_r = cases()[name]
    return spatial(ids, inten, m, units, DEFAULT_MAX_VOXELS if cap is None else cap, peak_r)


def call(fn, name):
    """a binding entry point (Engine.volume_spatial or binding.volume_spatial_host) on the case"""
    ids, inten, m, units, cap, peak_r = cases()[name]
    return fn(ids, inten, m=m, units=units, max_voxels=cap, peak_r=peak_r)


def assert_not_degenerate():
    """On this reference alone: the ellipsoid is one component of 2956 voxels, below the parity limit; the noise cases hold at
    least three searched components of more than one tile and at least one over their cap; the scattered ids have the voxel counts round
    the tile size and are interleaved; the constant box ties every sphere mean although n differs at the faces, and both peaks sit at
    voxel 0; the bright corner's sphere is cut on three faces; the checkerboard and the ramp have the signs the statistics are for."""
    ell = case_ref("ellipsoid(7, 7, 50)")[0]
    assert ell["voxels"] == ELLIPSOID_VOXELS <= PARITY_MAX_VOXELS and ell["searched"] == 1 and ell["pairs"] == 4_367_490
    assert ell["gp_at"] != ell["lp_at"] and ell["gp_n"] > 100
    big = over = 0
    for name in cases():
        if name.startswith("noise"):
            ref = case_ref(name)
            big += sum(1 for r in ref if r["searched"] and r["voxels"] > TILE)
            over += sum(1 for r in ref if r["voxels"] > 1200)
    assert big >= 3 and over >= 1, (big, over)
    sc = cases()["scattered"][0]
    ref = case_ref("scattered")
    assert [r["voxels"] for r in ref] == list(SCATTERED_COUNTS) and {0, -1, len(SCATTERED_COUNTS) + 1} <= set(np.unique(sc).tolist())
    assert [r["searched"] for r in ref] == [0, 1, 1, 1, 1, 1] and ref[1]["pairs"] == 1
    first = [int(np.flatnonzero(sc.reshape(-1) == r + 1)[0]) for r in range(3, 6)]
    last = [int(np.flatnonzero(sc.reshape(-1) == r + 1)[-1]) for r in range(3, 6)]
    assert max(first) < min(last)                               # interleaved
    big_m = case_ref("m4096")
    assert sum(1 for r in big_m if r["voxels"] == 0) > 4000 and big_m[6]["voxels"] == 100 and big_m[5]["searched"] == 0
    const = case_ref("constant")[0]
    full = len(ball_offsets((1, 1, 1), 2))
    assert const["gp_at"] == const["lp_at"] == 0 and const["gp_n"] < full and const["gp_sum"] == 1000 * const["gp_n"]
    assert (const["s1"], const["s2"], const["s3"]) == (0.0, 0.0, 0.0) and const["s0"] > 0.0
    corner = case_ref("bright_corner")[0]
    last_voxel = 6 * 7 * 9 - 1
    assert corner["lp_at"] == last_voxel and corner["lp_n"] < full // 2 and corner["imax"] == 65535
    r0 = case_ref("peak_r0")[0]
    assert r0["gp_at"] == r0["lp_at"] and (r0["gp_sum"], r0["gp_n"]) == (r0["imax"], 1)
    disc = ball_offsets((2, 2, 9), 5)
    assert {o[0] for o in disc} == {0} and len(disc) > 1
    for name, sign in (("checkerboard", -1), ("ramp", 1)):
        ids, inten, _, units, _, _ = cases()[name]
        i, c = ibsi_as_written(ids, inten, 0, units)
        assert sign * i > 0 and sign * (1.0 - c) > 0, (name, i, c)
