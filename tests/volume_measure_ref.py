"""Reference of the volume measurement (include/mi_unet.h: mi_unet_volume_measure) in numpy.  It shares no code with the
product and does not use the run-end argument: the diameters are searched over ALL voxels of a component, as the definition states
them, in chunks of rows of the full distance matrix.  Also the inputs and cases the CPU and the GPU tests share."""
import functools

import numpy as np

import volume_ref as vr

FIELDS = ("voxels", "ends", "imin", "imax", "d2", "dp", "dq", "a_d2", "a_p", "a_q", "sx", "sy", "sz", "sxx", "syy", "szz", "sxy", "sxz",
          "syz", "si", "sii")
STRUCT_BYTES = 128
MAX_ENDS_LIMIT = 1 << 20
DEFAULT_MAX_ENDS = 262144
TILE = 256                                  # the device form's LDS tile (csrc/kernels.h: VMS_TILE)
CHUNK_ELEMS = 4_000_000                     # entries of the distance matrix held at once


def run_ends(member):
    """bool [D, H, W]: the voxels of `member` whose x - 1 or x + 1 neighbour on the same row is not in it (outside is not)"""
    p = np.pad(member, ((0, 0), (0, 0), (1, 1)), constant_values=False)
    return member & (~p[:, :, :-2] | ~p[:, :, 2:])


def farthest(pts, idx):
    """((d2, p, q, ties), the same over the pairs with equal z) over all pairs of the rows of pts (int [N, 3], scaled; idx ascending): the
    maximum, the pair (p <= q by index) with the smallest p then the smallest q, and how many unordered pairs reach the maximum.  A
    chunk of rows i0 .. i1 meets the columns from i0 on: every pair once, but for the chunk's own square block, which holds both orders.
    The smallest row that reaches the maximum has every partner behind it: a partner before it would be a smaller row that reaches it."""
    n = pts.shape[0]
    x, y, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    state = [[-1, -1, -1, 0], [-1, -1, -1, 0]]
    rows = max(1, CHUNK_ELEMS // n)
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        dz = z[i0:i1, None] - z[None, i0:]
        d2 = (x[i0:i1, None] - x[None, i0:]) ** 2 + (y[i0:i1, None] - y[None, i0:]) ** 2 + dz ** 2
        for which, st in enumerate(state):
            if which == 1:
                d2[dz != 0] = -1
            top = int(d2.max())
            if top > st[0]:
                i = int(np.flatnonzero(d2.max(axis=1) == top)[0])
                st[:] = [top, int(idx[i0 + i]), int(idx[i0 + int(np.argmax(d2[i]))]), 0]
            if top == st[0]:
                hit = d2 == top
                square = int(hit[:, :i1 - i0].sum())
                st[3] += int(hit[:, i1 - i0:].sum()) + (square // 2 if top > 0 else square)
    return tuple(state[0]), tuple(state[1])


def measure(ids, intensity, m, units, max_ends=DEFAULT_MAX_ENDS):
    """the table by the definition: a list of m dicts over FIELDS (and "ties": the unordered pairs of voxels at the 3-D diameter)"""
    ids = np.asarray(ids)
    d, h, w = ids.shape
    ux, uy, uz = (int(u) for u in units)
    out = []
    for r in range(m):
        member = ids == r + 1
        row = {f: 0 for f in FIELDS}
        row["ties"] = 0
        n = int(member.sum())
        if n == 0:
            out.append(row)
            continue
        z, y, x = (c.astype(np.int64) for c in np.nonzero(member))         # raster order: the index ascends
        row.update(voxels=n, ends=int(run_ends(member).sum()), sx=int(x.sum()), sy=int(y.sum()), sz=int(z.sum()), sxx=int((x * x).sum()),
                   syy=int((y * y).sum()), szz=int((z * z).sum()), sxy=int((x * y).sum()), sxz=int((x * z).sum()), syz=int((y * z).sum()))
        if intensity is not None:
            v = np.asarray(intensity)[member].astype(np.int64)
            row.update(imin=int(v.min()), imax=int(v.max()), si=int(v.sum()), sii=int((v * v).sum()))
        if max_ends == 0 or row["ends"] > max_ends:
            for f in ("d2", "dp", "dq", "a_d2", "a_p", "a_q"):
                row[f] = -1
        else:
            pts = np.stack([x * ux, y * uy, z * uz], axis=1).astype(np.int32)   # (every d2 < 2^31 by the limits)
            (row["d2"], row["dp"], row["dq"], row["ties"]), (row["a_d2"], row["a_p"], row["a_q"], _) = farthest(pts, z * h * w + y * w + x)
        out.append(row)
    return out


def assert_equal(table, want, what=""):
    """a VMEASURE_DTYPE [m] table of the binding against measure(): every field"""
    assert table.shape == (len(want),), (what, table.shape, len(want))
    for f in FIELDS:
        col = np.array([r[f] for r in want], np.int64)
        assert np.array_equal(table[f].astype(np.int64), col), (what, f, np.flatnonzero(table[f] != col)[:5].tolist(),
                                                                 table[f][table[f] != col][:5].tolist(), col[table[f] != col][:5].tolist())


def derive(c, units, unit_mm):
    """mi_unet_volume_measure_derive's arithmetic in Python: exact integer numerators, numpy.linalg.eigh for the axes"""
    s = [float(u) * float(unit_mm) for u in units]
    n = int(c["voxels"])
    first = [int(c[k]) for k in ("sx", "sy", "sz")]
    second = [[int(c[k]) for k in row] for row in (("sxx", "sxy", "sxz"), ("sxy", "syy", "syz"), ("sxz", "syz", "szz"))]
    cov = np.array([[float(n * second[a][b] - first[a] * first[b]) / (float(n) * float(n)) * s[a] * s[b] + (s[a] * s[a] / 12.0 if a == b else 0.0)
                     for b in range(3)] for a in range(3)])
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1], vec[:, ::-1]
    si, sii = int(c["si"]), int(c["sii"])
    nan = float("nan")
    return dict(cx_mm=(first[0] / n + 0.5) * s[0], cy_mm=(first[1] / n + 0.5) * s[1], cz_mm=(first[2] / n + 0.5) * s[2], cov=cov, lam=lam,
                axis_mm=[2.0 * float(np.sqrt(5.0 * max(l, 0.0))) for l in lam], axis_dir=[vec[:, i] for i in range(3)], mean=si / n,
                std=float(np.sqrt(max(float(n * sii - si * si) / (float(n) * float(n)), 0.0))),
                diameter_mm=nan if c["d2"] < 0 else float(np.sqrt(float(c["d2"]))) * unit_mm,
                axial_diameter_mm=nan if c["a_d2"] < 0 else float(np.sqrt(float(c["a_d2"]))) * unit_mm)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def intensity_for(shape, seed):
    """u16 [D, H, W] from a seeded generator: a tenth of the voxels 0, a tenth 65535, the rest uniform"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, shape, dtype=np.int64)
    pick = rng.random(shape)
    v[pick < 0.1] = 0
    v[pick > 0.9] = 65535
    return v.astype(np.uint16)


def sheet(shape=(8, 24, 72)):
    """ids of the set { x + y + z = 0 mod 3 }: no voxel has an x neighbour in it, so every voxel is a run end, and the set is full of ties"""
    z, y, x = np.indices(shape)
    return ((x + y + z) % 3 == 0).astype(np.int32)


def scattered():
    """six ids of 1, 2, TILE - 1, TILE, TILE + 1 and 3 TILE + 5 single voxels (every one a run end: they sit at even x), between them voxels
    of the ids 0, -1 and m + 1, which belong to no component"""
    rng = np.random.default_rng(11)
    shape = (5, 37, 130)
    ids = np.zeros(shape, np.int32)
    counts = (1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
    z, y, x = np.indices(shape)
    free = np.flatnonzero((x % 2 == 0).reshape(-1))
    take = rng.permutation(free)[:sum(counts) + 200]
    at = 0
    for r, c in enumerate(counts):
        ids.reshape(-1)[take[at:at + c]] = r + 1
        at += c
    ids.reshape(-1)[take[at:at + 100]] = -1
    ids.reshape(-1)[take[at + 100:at + 200]] = len(counts) + 1
    return ids, counts


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids int32 [D,H,W], intensity u16 or None, m, units, max_ends or None)"""
    out = {}
    for si, shape in enumerate(vr.NOISE_SHAPES):
        for conn in (6, 26):
            k = si % len(vr.NOISE_VALUES)
            _, _, found, _, ids = vr.noise_ref(shape, conn)     # (cap 256: a plane with more components marks their voxels -1)
            out[f"noise{shape}c{conn}"] = (np.ascontiguousarray(ids[k]), intensity_for(shape, 100 + si), min(int(found[k]), 256),
                                           (1, 1, 1) if conn == 6 else (7, 7, 50), None)
    serp = vr.serpentine().astype(np.int32)
    out["serpentine"] = (serp, intensity_for(serp.shape, 3), 1, (2, 3, 5), None)
    sc, counts = scattered()
    out["scattered"] = (sc, intensity_for(sc.shape, 4), len(counts), (3, 2, 7), None)
    sh = sheet()
    for units in ((1, 1, 1), (7, 7, 50)):
        out[f"sheet{units}"] = (sh, intensity_for(sh.shape, 5), 1, units, None)
    for cap in (4607, 4608, 0):
        out[f"sheet_cap{cap}"] = (sh, intensity_for(sh.shape, 5), 1, (1, 1, 1), cap)
    out["box"] = (np.ones((4, 6, 9), np.int32), intensity_for((4, 6, 9), 6), 1, (1, 1, 1), None)
    crowded, m = vr.crowded_ids()                               # more ids in a segment than a wave reduces; a span that ends mid-segment
    out["crowded_segment"] = (crowded, intensity_for(crowded.shape, 7), m, (1, 1, 1), None)
    n16 = out[f"noise{vr.NOISE_SHAPES[2]}c6"]
    out["m4096"] = (n16[0], n16[1], 4096, (1, 1, 1), 300)       # ids past `found` are carried by no voxel; a cap that skips the large ones
    out["no_intensity"] = (out[f"noise{vr.NOISE_SHAPES[0]}c26"][0], None, 40, (1, 2, 3), None)
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    ids, inten, m, units, cap = cases()[name]
    return measure(ids, inten, m, units, DEFAULT_MAX_ENDS if cap is None else cap)


def call(fn, name):
    """a binding entry point (Engine.volume_measure or binding.volume_measure_host) on the case"""
    ids, inten, m, units, cap = cases()[name]
    return fn(ids, inten, m=m, units=units, max_ends=cap)


def assert_not_degenerate():
    """On this reference alone: the cases hold at least five components with more than one tile of run ends and at least five whose
    diameter is reached by more than one pair; the scattered ids have the run-end counts round the tile size; the box's tie rule picks
    voxel 0; on the (12, 40, 72) sheet the maximal pair differs between the two unit sets and the axial pair from the 3-D pair."""
    big = tied = 0
    for name in cases():
        if name.startswith("noise") or name == "serpentine":
            ref = case_ref(name)
            big += sum(1 for r in ref if r["ends"] > TILE)
            tied += sum(1 for r in ref if r["ties"] > 1)
    assert big >= 5 and tied >= 5, (big, tied)
    sc, counts = scattered()
    ref = case_ref("scattered")
    assert [r["ends"] for r in ref] == list(counts) == [r["voxels"] for r in ref]
    assert {0, -1, len(counts) + 1} <= set(np.unique(sc).tolist())
    box = case_ref("box")[0]
    assert box["ties"] == 4 and box["dp"] == 0 and box["dq"] == 4 * 6 * 9 - 1 and box["a_p"] == 0 and box["a_q"] == 6 * 9 - 1
    small = case_ref("sheet(1, 1, 1)")[0]
    assert small["voxels"] == small["ends"] == 4608 and small["ties"] > 1
    sh = sheet((12, 40, 72))
    iso, aniso = measure(sh, None, 1, (1, 1, 1))[0], measure(sh, None, 1, (7, 7, 50))[0]
    assert (iso["dp"], iso["dq"]) != (aniso["dp"], aniso["dq"]), (iso, aniso)
    for r in (iso, aniso):
        assert (r["dp"], r["dq"]) != (r["a_p"], r["a_q"]) and r["d2"] > r["a_d2"] > 0, r
