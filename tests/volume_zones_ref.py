"""Reference of the volume zones (include/mi_unet.h: mi_unet_volume_zones) in numpy.  It shares no code with the product:
levels come from volume_texture_ref's rule, a run's length is walked back along its offset one slab of the volume at a time, zones are
volume_ref.label at connectivity 26 per (component, level).  Also the 16 features of the two feature functions in Python, and the inputs
and cases the CPU and the GPU tests share."""
import functools
import math

import numpy as np

import volume_ref as vr
import volume_texture_ref as tx

FIELDS = ("voxels", "imin", "imax", "longest_run", "zones", "largest_zone", "runs", "runs_axial", "clamped", "clamped_axial")
ZONE_FIELDS = ("first", "component", "level", "size")
FEATURES = ("short_emphasis", "long_emphasis", "low_grey_emphasis", "high_grey_emphasis", "short_low", "short_high", "long_low", "long_high",
            "grey_nonuniformity", "grey_nonuniformity_norm", "size_nonuniformity", "size_nonuniformity_norm", "percentage", "grey_variance",
            "size_variance", "entropy")
STRUCT_BYTES, ZONE_BYTES, FEATURE_BYTES = 56, 16, 128
MAX_RUN = 8192
MAX_CAP = 1 << 24
MAX_CELLS = tx.MAX_CELLS
COUNT, WIDTH = tx.COUNT, tx.WIDTH
OFFSETS = tx.OFFSETS                                            # (dx, dy, dz), 13 of them


def keys_of(ids, intensity, m, L, mode, lo, width):
    """(key int64 [D, H, W]: (r + 1) << 8 | level, 0 outside every component; rows of (voxels, imin, imax))"""
    level, member, comp, rows = tx.levels_of(ids, intensity, m, L, mode, lo, width)
    return np.where(member, ((comp + 1) << 8) | level, 0), rows


def _pair(shape, dx, dy, dz):
    """index tuples (p, q) over which p + d = q stays inside"""
    d, h, w = shape
    p = (slice(0, d - dz), slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx)))
    q = (slice(dz, d), slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx)))
    return p, q


def run_lengths(key, dx, dy, dz):
    """(start bool [D, H, W]: the voxel is the first of a run along d; n int64: the voxels of the run from this voxel on).  The walk goes
    back from the far end of the axis the offset always advances on, a slab at a time: n(p) = 1 + n(p + d) where the keys agree."""
    n = (key != 0).astype(np.int64)
    axis = 0 if dz else 1 if dy else 2
    p, q = _pair(key.shape, dx, dy, dz)
    for c in range(key.shape[axis] - 2, -1, -1):
        cur, nxt = list(p), list(q)
        cur[axis], nxt[axis] = slice(c, c + 1), slice(c + 1, c + 2)
        cur, nxt = tuple(cur), tuple(nxt)
        same = (key[cur] != 0) & (key[cur] == key[nxt])
        n[cur] += np.where(same, n[nxt], 0)
    start = key != 0
    start[q] &= key[q] != key[p]
    return start, n


def zones(ids, intensity, m, levels=32, mode=COUNT, lo=0, width=1, max_run=32, want_runs=True, want_axial=True, cap=None):
    """(table: list of m dicts over FIELDS, rlm int64 [m, L, R] or None, rlm_axial or None, zone list: found tuples over ZONE_FIELDS in
    `first` order (not cut) or None, found or None, cap) by the definition"""
    L, R = levels, max_run
    key, rows = keys_of(ids, intensity, m, L, mode, lo, width)
    table = [dict(voxels=n, imin=a, imax=b, longest_run=0, zones=0, largest_zone=0, runs=0, runs_axial=0, clamped=0, clamped_axial=0) for n, a, b in rows]
    rlm = np.zeros((m, L, R), np.int64) if want_runs else None
    axial = np.zeros((m, L, R), np.int64) if want_axial else None
    for dx, dy, dz in OFFSETS if (want_runs or want_axial) else []:
        if not want_runs and dz:
            continue
        start, n = run_lengths(key, dx, dy, dz)
        k, n = key[start], n[start]
        idx = ((k >> 8) - 1, k & 255, np.minimum(n, R) - 1)
        for tab, run_key, clamp_key in ((rlm, "runs", "clamped"), (axial if dz == 0 else None, "runs_axial", "clamped_axial")):
            if tab is None:
                continue
            np.add.at(tab, idx, 1)
            for r in range(m):
                mine = idx[0] == r
                table[r][run_key] += int(mine.sum())
                table[r][clamp_key] += int((n[mine] > R).sum())
                if tab is rlm and mine.any():
                    table[r]["longest_run"] = max(table[r]["longest_run"], int(n[mine].max()))
    if cap is None:
        cap = min(max(key.size, 1), MAX_CAP)
    if not cap:
        return table, rlm, axial, None, None, 0
    found = []
    for k in np.unique(key[key != 0]).tolist():
        lab, count = vr.label(key == k, 26)
        flat = lab.reshape(-1)
        at = np.flatnonzero(flat >= 0)
        _, first, size = np.unique(flat[at], return_index=True, return_counts=True)
        found += [(int(at[f]), (k >> 8) - 1, k & 255, int(s)) for f, s in zip(first, size)]
        assert len(first) == count
    found.sort()
    for _, r, _, s in found:
        table[r]["zones"] += 1
        table[r]["largest_zone"] = max(table[r]["largest_zone"], s)
    return table, rlm, axial, found, len(found), cap


def assert_equal(got, want, what=""):
    """(table VZONES_DTYPE [m], rlm, rlm_axial, zones VZONE_DTYPE [cap], found) of the binding against zones(): every field, cell and record"""
    table, rlm, axial, zlist, found = got
    rtable, rrlm, raxial, rzones, rfound, cap = want
    assert table.shape == (len(rtable),), (what, table.shape, len(rtable))
    for f in FIELDS:
        col = np.array([r[f] for r in rtable], np.int64)
        assert np.array_equal(table[f].astype(np.int64), col), (what, f, np.flatnonzero(table[f] != col)[:5].tolist(),
                                                                 table[f][table[f] != col][:5].tolist(), col[table[f] != col][:5].tolist())
    for name, a, b in (("rlm", rlm, rrlm), ("rlm_axial", axial, raxial)):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == np.uint32 and a.shape == b.shape, (what, name, a.shape, b.shape)
            bad = np.argwhere(a.astype(np.int64) != b)
            assert bad.size == 0, (what, name, len(bad), bad[:5].tolist())
    assert (zlist is None) == (rzones is None) and found == rfound, (what, found, rfound)
    if zlist is not None:
        assert zlist.shape == (cap,), (what, zlist.shape, cap)
        kept = min(rfound, cap)
        rec = [tuple(int(v) for v in z) for z in zlist[:kept].tolist()]
        bad = [i for i in range(kept) if rec[i] != rzones[i]]
        assert not bad, (what, len(bad), [(rec[i], rzones[i]) for i in bad[:5]])
        assert not zlist[kept:].tobytes().strip(b"\0"), (what, "records behind the list")


def same_bytes(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and (x == y if isinstance(x, int) else x.tobytes() == y.tobytes()))
               for x, y in zip(a, b))


def features(cells, voxels, directions):
    """the 16 features over cells (i, j, count), i = level + 1, j = run length or zone size, with exactly rounded sums"""
    cells = sorted((int(i), int(j), int(c)) for i, j, c in cells if c)
    N = sum(c for _, _, c in cells)
    if N == 0:
        return {k: float("nan") for k in FEATURES}
    ni, nj = {}, {}
    for i, j, c in cells:
        ni[i] = ni.get(i, 0) + c
        nj[j] = nj.get(j, 0) + c
    mu_i, mu_j = sum(i * c for i, c in ni.items()) / N, sum(j * c for j, c in nj.items()) / N
    gn, sn = math.fsum(float(c) * float(c) for c in ni.values()), math.fsum(float(c) * float(c) for c in nj.values())
    return dict(short_emphasis=math.fsum(c / (j * j) for j, c in nj.items()) / N, long_emphasis=math.fsum(c * (j * j) for j, c in nj.items()) / N,
                low_grey_emphasis=math.fsum(c / (i * i) for i, c in ni.items()) / N, high_grey_emphasis=math.fsum(c * (i * i) for i, c in ni.items()) / N,
                short_low=math.fsum(c / (i * i * j * j) for i, j, c in cells) / N, short_high=math.fsum(c * i * i / (j * j) for i, j, c in cells) / N,
                long_low=math.fsum(c * j * j / (i * i) for i, j, c in cells) / N, long_high=math.fsum(c * i * i * j * j for i, j, c in cells) / N,
                grey_nonuniformity=gn / N, grey_nonuniformity_norm=gn / N / N, size_nonuniformity=sn / N, size_nonuniformity_norm=sn / N / N,
                percentage=N / (voxels * directions), grey_variance=math.fsum((i - mu_i) ** 2 * (c / N) for i, j, c in cells),
                size_variance=math.fsum((j - mu_j) ** 2 * (c / N) for i, j, c in cells),
                entropy=-math.fsum((c / N) * math.log2(c / N) for _, _, c in cells))


def run_cells(row):
    row = np.asarray(row)
    return [(l + 1, j + 1, int(row[l, j])) for l, j in np.argwhere(row != 0).tolist()]


def zone_cells(zone_list, r):
    cells = {}
    for _, comp, level, size in zone_list:
        if comp == r:
            cells[(level + 1, size)] = cells.get((level + 1, size), 0) + 1
    return [(i, j, c) for (i, j), c in cells.items()]


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
HAND = np.array([[0, 0, 1, 1], [0, 0, 1, 2], [3, 1, 2, 2], [3, 3, 2, 2]], np.uint16)
# The 4 x 4 image above as one slice, levels = values, by hand.  Runs (level:length) along (1, 0) by row: 0:2 1:2 | 0:2 1:1 2:1 | 3:1 1:1
# 2:2 | 3:2 2:2; along (0, 1) by column: 0:2 3:2 | 0:2 1:1 3:1 | 1:2 2:2 | 1:1 2:3; along (1, 1) by diagonal from the lower left: 3:1 | 3:2
# | 0:1 1:1 2:1 | 0:2 2:2 | 0:1 1:1 2:1 | 1:1 2:1 | 1:1; along (-1, 1) by anti-diagonal from the upper left: 0:1 | 0:2 | 1:1 0:1 3:1 | 1:3
# 3:1 | 2:2 3:1 | 2:2 | 2:1.  Every direction covers the 16 pixels once.
HAND_RLM_AXIAL = [[[4, 6, 0, 0], [9, 2, 1, 0], [5, 6, 1, 0], [6, 3, 0, 0]]]       # [level][run - 1] over the four in-plane offsets: 43 runs
HAND_HIST = [4, 4, 5, 3]                                        # with one slice, each of the 9 other offsets sees every pixel as a run of 1
# zones (8-connected in the slice): level 0 the upper left block of 4; level 1 one of 4 (the 1 of row 2 touches the 1 of row 1
# diagonally); level 2 one of 5; level 3 one of 3
HAND_ZONES = [(0, 0, 0, 4), (2, 0, 1, 4), (7, 0, 2, 5), (8, 0, 3, 3)]


def diagonals():
    """ids int32 [9, 29, 330]: 13 lines of 7 voxels, one along each offset, each through the corner (4, 8 j, 64 i) of 7.15's 4 x 8 x 64
    tiles at its middle voxel.  The lines keep two voxels apart, so each is a run of 7 along its offset and a zone of its own."""
    ids = np.zeros((9, 29, 330), np.int32)
    centres = [(4, y, x) for y in (8, 16, 24) for x in (64, 128, 192, 256, 320)]
    for (dx, dy, dz), (cz, cy, cx) in zip(OFFSETS, centres):
        for t in range(-3, 4):
            ids[cz + t * dz, cy + t * dy, cx + t * dx] = 1
    return ids


def _ramp_lengths(R):
    """ids int32 [1, 5, R + 4]: rows 0, 2 and 4 hold one run of R - 1, R and R + 1"""
    ids = np.zeros((1, 5, R + 4), np.int32)
    for row, n in ((0, R - 1), (2, R), (4, R + 1)):
        ids[0, row, 1:1 + n] = 1
    return ids


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids int32 [D,H,W], intensity u16, m, keyword arguments of the call)"""
    out = {}
    out["hand_4x4"] = (np.ones((1, 4, 4), np.int32), HAND.reshape(1, 4, 4), 1, dict(levels=4, mode=WIDTH, lo=0, width=1, max_run=4))
    stacks = {}
    for shape, conn, k in (((7, 40, 72), 26, 1), ((5, 33, 130), 18, 1), ((3, 19, 70), 26, 2), ((16, 24, 130), 6, 2)):
        _, _, found, _, ids = vr.noise_ref(shape, conn)         # (cap 256: a plane with more components marks their voxels -1)
        stacks[shape] = (np.ascontiguousarray(ids[k]), min(int(found[k]), 256))
    # every level count, both modes and both kinds of intensity on every stack, not their whole product: a zone reference costs a flood
    # fill in Python per member voxel
    plan = {(7, 40, 72): (("noisy", 8, COUNT), ("smooth", 32, WIDTH), ("smooth", 64, COUNT)),
            (5, 33, 130): (("smooth", 8, WIDTH), ("noisy", 32, COUNT), ("noisy", 64, WIDTH)),
            (3, 19, 70): (("smooth", 8, COUNT), ("noisy", 32, WIDTH), ("smooth", 64, WIDTH), ("noisy", 64, COUNT)),
            (16, 24, 130): (("smooth", 32, COUNT), ("noisy", 8, WIDTH))}
    for shape, combos in plan.items():
        ids, m = stacks[shape]
        for kind, L, mode in combos:
            inten = tx.noisy(shape, 200 + L) if kind == "noisy" else tx.smooth(shape, 300 + L)
            kw = dict(levels=L, mode=mode, max_run=3 if shape[0] == 16 else 32)       # (3: runs are clamped in noise, too)
            if mode == WIDTH:
                kw.update(lo=3000 if kind == "noisy" else 1500, width=(60000 if kind == "noisy" else 8000) // L)
            out[f"noise{shape}_{kind}_L{L}_{mode}"] = (ids, inten, m, kw)
    out["constant_slab"] = (np.ones((4, 9, 96), np.int32), np.full((4, 9, 96), 777, np.uint16), 1, dict())
    diag = diagonals()
    out["diagonals"] = (diag, np.full(diag.shape, 5, np.uint16), 1, dict(levels=4, max_run=8))
    for axis, shape in enumerate(((8192, 1, 1), (1, 8192, 1), (1, 1, 8192))):
        for R in (8192, 32):
            out[f"run8192_{'DHW'[axis]}_R{R}"] = (np.ones(shape, np.int32), np.full(shape, 9, np.uint16), 1, dict(levels=64 if R == 8192 else 2, max_run=R))
    ramp = _ramp_lengths(8)
    out["lengths_R-1_R_R+1"] = (ramp, np.full(ramp.shape, 100, np.uint16), 1, dict(levels=2, max_run=8))
    z, y, x = np.indices((5, 9, 70))
    out["checkerboard_levels"] = (np.ones((5, 9, 70), np.int32), (((x + y + z) % 2) * 1000).astype(np.uint16), 1, dict(levels=2, mode=WIDTH, lo=0, width=500))
    out["two_ids_one_level"] = ((1 + (x >= 35)).astype(np.int32), np.full((5, 9, 70), 40, np.uint16), 2, dict(levels=8))
    blobs = np.zeros((5, 9, 70), np.int32)
    blobs[1:4, 1:4, 3:20] = 1
    blobs[0:5, 5:9, 30:69] = 1
    out["two_blobs_one_id"] = (blobs, np.full((5, 9, 70), 40, np.uint16), 1, dict(levels=8))
    path = vr.serpentine(5, 17, 130)
    out["serpentine_level"] = (np.ones(path.shape, np.int32), np.where(path != 0, 100, 900).astype(np.uint16), 1, dict(levels=2, mode=WIDTH, lo=0, width=500, max_run=64))
    sc = tx.scattered()
    out["scattered"] = (sc, tx.noisy(sc.shape, 25), 6, dict(levels=32))
    n1 = vr.noise_ref((1, 48, 80), 6)
    out["D1"] = (np.ascontiguousarray(n1[4][1]), tx.smooth((1, 48, 80), 21), min(int(n1[2][1]), 256), dict(levels=16))
    out["H1"] = (np.ones((6, 1, 70), np.int32), tx.smooth((6, 1, 70), 22), 1, dict(levels=16))
    out["one_voxel_volume"] = (np.ones((1, 1, 1), np.int32), np.full((1, 1, 1), 9, np.uint16), 1, dict())
    base_name = "noise(3, 19, 70)_smooth_L8_count"
    base = out[base_name]
    for name, kw in (("no_rlm", dict(want_runs=False)), ("no_axial", dict(want_axial=False)), ("no_zones", dict(cap=0)),
                     ("entry_only", dict(want_runs=False, want_axial=False, cap=0)), ("cap_1", dict(cap=1))):
        out[name] = (base[0], base[1], base[2], dict(base[3], **kw))
    base_found = zones(base[0], base[1], base[2], **base[3])[4]
    out["cap_found-1"] = (base[0], base[1], base[2], dict(base[3], cap=base_found - 1))
    ids16, _ = stacks[(16, 24, 130)]
    out["m4096_L32_R32"] = (ids16, tx.noisy((16, 24, 130), 26), 4096, dict(levels=32, max_run=32, cap=4096))
    # more components than 7.15's key launcher takes at once at 64 levels (m L^2 = 2^24): the keys are made in four parts; ids of every
    # part, of 0, -1 and m + 1
    wide = np.random.default_rng(14).integers(-1, 4098, (5, 19, 70)).astype(np.int32)
    out["m4096_L64_R16_parts"] = (wide, tx.noisy(wide.shape, 28), 4096, dict(levels=64, max_run=16))
    out["m2048_L64_R32_parts"] = (np.minimum(wide, 2049), tx.smooth(wide.shape, 29), 2048, dict(levels=64, max_run=32, mode=WIDTH, lo=1000, width=40))
    ids3, _ = stacks[(3, 19, 70)]
    out["m1_L64_R8192"] = (ids3, tx.smooth((3, 19, 70), 27), 1, dict(levels=64, max_run=8192))
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    ids, inten, m, kw = cases()[name]
    return zones(ids, inten, m, **kw)


def call(fn, name):
    """a binding entry point (Engine.volume_zones or binding.volume_zones_host) on the case"""
    ids, inten, m, kw = cases()[name]
    return fn(ids, inten, m, **kw)


def assert_not_degenerate():
    """On this reference alone, what makes each case a test: the hand-worked tables; runs longer than 1 along every one of the 13 offsets;
    clamped runs; a run of exactly R (not clamped) beside one of R + 1; zones larger than 1; a component with several zones at one level;
    a list that is cut; ids that belong to nothing; two ids and two blobs that stay apart; a zone the merge has to travel along."""
    table, rlm, axial, zl, found, _ = case_ref("hand_4x4")
    assert axial.tolist() == HAND_RLM_AXIAL and zl == HAND_ZONES and found == 4
    assert (rlm - axial)[0].tolist() == [[9 * n, 0, 0, 0] for n in HAND_HIST]
    assert table[0]["runs_axial"] == 43 and table[0]["runs"] == 43 + 9 * 16 and table[0]["longest_run"] == 3 and table[0]["clamped"] == 0
    ids, inten, m, kw = cases()["diagonals"]
    key, _ = keys_of(ids, inten, m, 4, COUNT, 0, 1)
    for dx, dy, dz in OFFSETS:
        start, n = run_lengths(key, dx, dy, dz)
        assert sorted(n[start].tolist())[-2:] == [1, 7], (dx, dy, dz)         # one run of 7 along its own offset, 84 single voxels
    table, rlm, _, zl, found, _ = case_ref("diagonals")
    assert found == 13 and all(z[3] == 7 and z[2] == 0 for z in zl) and table[0]["zones"] == 13 and rlm[0, 0, 6] == 13
    table = case_ref("constant_slab")[0]
    assert table[0]["clamped"] > 0 and table[0]["clamped_axial"] > 0 and table[0]["longest_run"] == 96 and table[0]["zones"] == 1 and table[0]["largest_zone"] == 4 * 9 * 96
    table, rlm, axial, _, _, _ = case_ref("lengths_R-1_R_R+1")
    assert rlm[0, 0, 6] == 1 and rlm[0, 0, 7] == 2 and table[0]["clamped"] == 1 and table[0]["clamped_axial"] == 1 and table[0]["longest_run"] == 9
    for axis in "DHW":
        full, cut = case_ref(f"run8192_{axis}_R8192"), case_ref(f"run8192_{axis}_R32")
        assert full[1][0, 0, 8191] == 1 and full[0][0]["clamped"] == 0 and full[0][0]["longest_run"] == 8192 and full[0][0]["runs"] == 1 + 12 * 8192
        assert cut[1][0, 0, 31] == 1 and cut[0][0]["clamped"] == 1 and cut[0][0]["longest_run"] == 8192 and (cut[0][0]["clamped_axial"] == 1) == (axis != "D")
    table, rlm, axial, zl, found, _ = case_ref("checkerboard_levels")
    assert found == 2 and sorted(z[2] for z in zl) == [0, 1] and axial[0, :, 1:].sum() > 0        # long runs only along diagonals
    ids = cases()["checkerboard_levels"][0]
    key, _ = keys_of(*cases()["checkerboard_levels"][:3], 2, WIDTH, 0, 500)
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        start, n = run_lengths(key, *off)
        assert start.all() and (n == 1).all(), off
    assert [z[1:] for z in case_ref("two_ids_one_level")[3]] == [(0, 0, 5 * 9 * 35), (1, 0, 5 * 9 * 35)]
    assert [z[1:] for z in case_ref("two_blobs_one_id")[3]] == [(0, 0, 5 * 4 * 39), (0, 0, 3 * 3 * 17)]
    path = vr.serpentine(5, 17, 130)
    zl = case_ref("serpentine_level")[3]
    assert (0, 0, 0, int(path.sum())) in zl and int(path.sum()) > 3000
    sc = cases()["scattered"][0]
    assert {-1, 0, 7} <= set(np.unique(sc).tolist()) and sum(r["voxels"] for r in case_ref("scattered")[0]) == int(((sc >= 1) & (sc <= 6)).sum())
    big = [case_ref(n) for n in cases() if n.startswith("noise")]
    assert all(max(z[3] for z in c[3]) > 1 and c[4] > 20 for c in big)
    assert any(any(r["clamped"] > 0 for r in c[0]) for c in big)
    assert case_ref("cap_1")[4] > 1 and case_ref("cap_found-1")[5] == case_ref("cap_found-1")[4] - 1 and case_ref("cap_found-1")[4] > 20
    table = case_ref("m4096_L32_R32")[0]
    assert 4096 * 32 * 32 == MAX_CELLS and len(table) == 4096 and sum(1 for r in table if r["voxels"] == 0) > 2048 and case_ref("m4096_L32_R32")[4] > 4096
    parts = case_ref("m4096_L64_R16_parts")[0]
    assert 4096 * 64 * 16 == MAX_CELLS and all(sum(1 for r in parts[a:a + 1024] if r["voxels"]) > 500 for a in (0, 1024, 2048, 3072))
    assert case_ref("no_rlm")[1] is None and case_ref("no_axial")[2] is None and case_ref("no_zones")[3] is None
    assert all(r["longest_run"] == 0 and r["runs"] == 0 for r in case_ref("no_rlm")[0]) and any(r["runs_axial"] > 0 for r in case_ref("no_rlm")[0])
