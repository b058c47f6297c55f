"""Reference of the volume split (include/mi_unet.h: mi_unet_volume_split) in numpy and scipy.  It shares no code with
the product: the erosion is ndimage.binary_erosion with the ball built from the definition, the cores and the rest are ndimage.label,
the growth is a heapq Dijkstra over (length, marker), and table, info and ids follow from the definition by numpy reductions.  Also
the named cases the CPU and the GPU tests share, call(), assert_equal() and assert_not_degenerate()."""
import functools
import heapq

import numpy as np
from scipy import ndimage

import volume_ref

TABLE_FIELDS = volume_ref.FIELDS
INFO_FIELDS = ("core_first", "core_voxels", "reach", "cut_x", "cut_y", "cut_z")
STAT_FIELDS = ("value", "in_voxels", "core_voxels", "cores", "cores_kept", "pieces", "coreless", "max_reach")
PIECE_BYTES, STAT_BYTES = 40, 64
MAX_R = 46340
UNREACHED = (1 << 64) - 1


def structure(connectivity):
    """the 3 x 3 x 3 structuring element of ndimage.label for 6 / 18 / 26"""
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


def ball(units, r):
    """bool [2 ez + 1, 2 ey + 1, 2 ex + 1]: (dx ux)^2 + (dy uy)^2 + (dz uz)^2 <= r^2 with half-widths r // u"""
    ux, uy, uz = units
    ex, ey, ez = r // ux, r // uy, r // uz
    dz, dy, dx = np.mgrid[-ez:ez + 1, -ey:ey + 1, -ex:ex + 1]
    return (dx * ux) ** 2 + (dy * uy) ** 2 + (dz * uz) ** 2 <= r * r


def erode(s, units, r):
    """only voxels inside the volume constrain the erosion: outside counts as set"""
    return ndimage.binary_erosion(s, ball(units, r), border_value=1) & s


def steps(units, connectivity):
    ux, uy, uz = units
    return [(dz, dy, dx, (dx != 0) * ux + (dy != 0) * uy + (dz != 0) * uz) for dz, dy, dx in volume_ref.neighbours(connectivity)]


def grow(s, seeds, units, connectivity):
    """Dijkstra: s bool [D,H,W], seeds = {flat index: marker} -> (length int64 [D,H,W], marker int64 [D,H,W]), -1 where unreached"""
    d, h, w = s.shape
    inside = s.reshape(-1).tolist()
    best = {}
    heap = [(0, m, i) for i, m in seeds.items()]
    for _, m, i in heap:
        best[i] = (0, m)
    heapq.heapify(heap)
    st = steps(units, connectivity)
    while heap:
        length, m, i = heapq.heappop(heap)
        if best[i] != (length, m):
            continue
        z, rem = divmod(i, h * w)
        y, x = divmod(rem, w)
        for dz, dy, dx, cost in st:
            zz, yy, xx = z + dz, y + dy, x + dx
            if not (0 <= zz < d and 0 <= yy < h and 0 <= xx < w):
                continue
            j = (zz * h + yy) * w + xx
            if not inside[j]:
                continue
            cand = (length + cost, m)
            if j not in best or cand < best[j]:
                best[j] = cand
                heapq.heappush(heap, (cand[0], m, j))
    length = np.full(d * h * w, -1, np.int64)
    marker = np.full(d * h * w, -1, np.int64)
    if best:
        idx = np.fromiter(best.keys(), np.int64, len(best))
        vals = np.array(list(best.values()), np.int64).reshape(-1, 2)
        length[idx], marker[idx] = vals[:, 0], vals[:, 1]
    return length.reshape(s.shape), marker.reshape(s.shape)


def plane(masks, value, units=(1, 1, 1), connectivity=26, neck_r=0, min_core=1, cap=256):
    """one plane by the definition -> dict(table, info (lists of dicts, cap long), ids, found, stats, pieces (all, in order), length,
    marker, labels)"""
    s = np.asarray(masks) == value
    d, h, w = s.shape
    flat = np.arange(d * h * w, dtype=np.int64).reshape(s.shape)
    cores = erode(s, units, neck_r)
    clab, ncores = ndimage.label(cores, structure(connectivity))
    seeds, core_size, kept = {}, {}, 0
    if ncores:
        sizes = np.bincount(clab.reshape(-1), minlength=ncores + 1)
        firsts = ndimage.minimum(flat, clab, np.arange(1, ncores + 1)).astype(np.int64)
        for c in range(1, ncores + 1):
            if sizes[c] >= min_core:
                kept += 1
                core_size[int(firsts[c - 1])] = int(sizes[c])
        marker_of = np.zeros(ncores + 1, np.int64)
        marker_of[1:] = firsts
        keep = np.zeros(ncores + 1, bool)
        keep[1:] = sizes[1:] >= min_core
        sel = keep[clab]
        seeds = dict(zip(flat[sel].tolist(), marker_of[clab[sel]].tolist()))
    length, marker = grow(s, seeds, units, connectivity)
    rest = s & (marker < 0)
    rlab, nrest = ndimage.label(rest, structure(connectivity))
    # the piece of every voxel of S: the marker for a cored piece, d h w + the rest's label for a coreless one
    label = np.where(s, np.where(marker >= 0, marker, d * h * w + rlab), -1)
    names = np.unique(label[s])
    index = np.searchsorted(names, label[s])
    l = np.full(s.shape, -1, np.int64)
    l[s] = index
    count = len(names)
    z, y, x = np.nonzero(s)
    p = np.pad(l, 1, constant_values=-1)
    c = p[1:-1, 1:-1, 1:-1]
    nb = dict(x=(p[1:-1, 1:-1, :-2], p[1:-1, 1:-1, 2:]), y=(p[1:-1, :-2, 1:-1], p[1:-1, 2:, 1:-1]), z=(p[:-2, 1:-1, 1:-1], p[2:, 1:-1, 1:-1]))
    pieces = []
    if count:
        def total(v):
            out = np.zeros(count, np.int64)
            np.add.at(out, index, np.asarray(v, np.int64))
            return out

        def lowest(v):
            out = np.full(count, np.iinfo(np.int64).max, np.int64)
            np.minimum.at(out, index, np.asarray(v, np.int64))
            return out

        def highest(v):
            out = np.full(count, -1, np.int64)
            np.maximum.at(out, index, np.asarray(v, np.int64))
            return out

        cols = dict(voxels=np.bincount(index, minlength=count), first=lowest(flat[s]), x0=lowest(x), y0=lowest(y), z0=lowest(z),
                    x1=highest(x), y1=highest(y), z1=highest(z), sx=total(x), sy=total(y), sz=total(z),
                    reach=highest(np.maximum(length[s], 0)))
        for ax in "xyz":
            a, b = nb[ax]
            cols["faces_" + ax] = total(((a != c).astype(np.int64) + (b != c))[s])
            cols["cut_" + ax] = total((((a != c) & (a >= 0)).astype(np.int64) + ((b != c) & (b >= 0)))[s])
        for i in range(count):
            q = {n: int(cols[n][i]) for n in cols}
            name = int(names[i])
            cored = name < d * h * w
            q.update(value=int(value), kept=1, label=i, core_first=name if cored else -1, core_voxels=core_size[name] if cored else 0)
            pieces.append(q)
    pieces.sort(key=lambda q: (-q["voxels"], q["first"]))
    rank = np.zeros(count + 1, np.int64)
    for r, q in enumerate(pieces):
        rank[q["label"]] = r
    ids = np.where(s, np.where(rank[l] < cap, rank[l] + 1, -1), 0).astype(np.int32)
    zero_t, zero_i = {n: 0 for n in TABLE_FIELDS}, {n: 0 for n in INFO_FIELDS}
    table = [{n: q[n] for n in TABLE_FIELDS} for q in pieces[:cap]] + [zero_t] * max(0, cap - count)
    info = [{n: q[n] for n in INFO_FIELDS} for q in pieces[:cap]] + [zero_i] * max(0, cap - count)
    stats = dict(value=int(value), in_voxels=int(s.sum()), core_voxels=int(cores.sum()), cores=int(ncores), cores_kept=kept, pieces=count,
                 coreless=int(nrest), max_reach=max([q["reach"] for q in pieces], default=0))
    return dict(table=table, info=info, ids=ids, found=count, stats=stats, pieces=pieces, length=length, marker=marker, labels=l)


def split(masks, values, **kw):
    """all planes: dict(table [n][cap], info [n][cap], found [n], stats [n], ids int32 [n,D,H,W], planes)"""
    ps = [plane(masks, v, **kw) for v in values]
    return dict(table=[p["table"] for p in ps], info=[p["info"] for p in ps], found=[p["found"] for p in ps], stats=[p["stats"] for p in ps],
                ids=np.stack([p["ids"] for p in ps]), planes=ps)


def assert_equal(got, want, what=""):
    """the binding's dict against split(): table, info, ids, found and stats, every field; `rounds` is no part of the comparison"""
    assert list(got["found"]) == list(want["found"]), (what, "found", list(got["found"]), want["found"])
    if got["ids"] is not None:
        assert np.array_equal(got["ids"], want["ids"]), (what, "ids", int((got["ids"] != want["ids"]).sum()))
    for key, fields in (("table", TABLE_FIELDS), ("info", INFO_FIELDS)):
        rows_all = want[key]
        assert got[key].shape == (len(rows_all), len(rows_all[0])), (what, key, got[key].shape)
        for k, rows in enumerate(rows_all):
            for f in fields:
                col = np.array([r[f] for r in rows], np.int64)
                assert np.array_equal(got[key][k][f].astype(np.int64), col), (what, key, "plane", k, f,
                                                                              np.flatnonzero(got[key][k][f] != col)[:5].tolist())
    for k, st in enumerate(want["stats"]):
        for f in STAT_FIELDS:
            assert int(got["stats"][k][f]) == st[f], (what, "stats", k, f, int(got["stats"][k][f]), st[f])


def same_bytes(a, b, what=""):
    """two results of the binding: the same bytes in everything but `rounds`"""
    for key in ("table", "info", "found", "stats", "ids"):
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, (what, key)
            continue
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def balls(shape, centres, radii, units):
    """u8 [D,H,W]: the union of the balls ((x-cx) ux)^2 + ((y-cy) uy)^2 + ((z-cz) uz)^2 <= r^2, centres as (z, y, x)"""
    z, y, x = np.indices(shape)
    ux, uy, uz = units
    v = np.zeros(shape, bool)
    for (cz, cy, cx), r in zip(centres, radii):
        v |= ((x - cx) * ux) ** 2 + ((y - cy) * uy) ** 2 + ((z - cz) * uz) ** 2 <= r * r
    return v.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def two_balls():
    return balls((20, 24, 40), ((10, 12, 11), (10, 12, 27)), (8, 8), (1, 1, 1))


@functools.lru_cache(maxsize=None)
def aniso():
    return balls((9, 40, 80), ((4, 20, 18), (4, 20, 58)), (160, 160), (7, 7, 50))


@functools.lru_cache(maxsize=None)
def chain():
    v = balls((16, 24, 130), ((8, 12, 20), (8, 12, 38), (8, 12, 70), (8, 12, 112)), (10, 9, 7, 11), (1, 1, 1))
    v[8, 12, 70:112] = 1
    return v


@functools.lru_cache(maxsize=None)
def serpentine(w):
    v = np.zeros((3, 33, w), np.uint8)
    for r in range(33):
        if r % 2 == 0:
            v[1, r, :] = 1
        else:
            v[1, r, w - 1 if (r // 2) % 2 == 0 else 0] = 1
    v[0:3, 0:5, 0:5] = 1
    v[0:3, 28:33, w - 5:w] = 1
    return v


NOISE_SHAPE = (7, 40, 72)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (masks, values, keyword arguments of a call)"""
    noise = volume_ref.smooth_noise(NOISE_SHAPE)
    c = {}
    for neck in (3, 5):
        c[f"two_balls_neck{neck}"] = (two_balls(), (1,), dict(units=(1, 1, 1), connectivity=26, neck_r=neck))
    for neck in (100, 60):
        c[f"aniso_neck{neck}"] = (aniso(), (1,), dict(units=(7, 7, 50), connectivity=26, neck_r=neck))
    for conn in (6, 26):
        c[f"chain_{conn}"] = (chain(), (1,), dict(units=(1, 1, 1), connectivity=conn, neck_r=4))
    for w in (64, 130):
        c[f"serpentine_{w}"] = (serpentine(w), (1,), dict(units=(3, 3, 10), connectivity=6, neck_r=10))
    for conn in volume_ref.CONNECTIVITIES:
        for neck in (1, 2):
            for min_core in (1, 5):
                c[f"noise_{conn}_neck{neck}_core{min_core}"] = (noise, volume_ref.NOISE_VALUES,
                                                                dict(units=(1, 1, 1), connectivity=conn, neck_r=neck, min_core=min_core))
                c[f"noise_{conn}_neck{neck}_core{min_core}_u235"] = (noise, volume_ref.NOISE_VALUES,
                                                                     dict(units=(2, 3, 5), connectivity=conn, neck_r=neck, min_core=min_core))
    c["one_slice"] = (np.ascontiguousarray(noise[3:4]), (1, 2), dict(units=(1, 1, 1), connectivity=18, neck_r=1))
    c["side_of_1"] = (np.ascontiguousarray(noise[:, :, 5:6]), (2,), dict(units=(2, 3, 5), connectivity=26, neck_r=3))
    c["row_only"] = (np.ascontiguousarray(noise[2:3, 7:8, :]), (1, 3), dict(units=(1, 1, 1), connectivity=6, neck_r=1))
    c["value_absent"] = (noise, (2, 9), dict(units=(1, 1, 1), connectivity=26, neck_r=1))
    c["value_0"] = (noise, (0,), dict(units=(1, 1, 1), connectivity=6, neck_r=1))
    c["cap_below_found"] = (noise, volume_ref.NOISE_VALUES, dict(units=(1, 1, 1), connectivity=6, neck_r=1, cap=7))
    c["all_coreless"] = (noise, volume_ref.NOISE_VALUES, dict(units=(1, 1, 1), connectivity=18, neck_r=1, min_core=10 ** 6))
    c["identity_u235_18"] = (noise, volume_ref.NOISE_VALUES, dict(units=(2, 3, 5), connectivity=18, neck_r=1, min_core=1))
    return c


@functools.lru_cache(maxsize=None)
def case_ref(name):
    masks, values, kw = cases()[name]
    return split(masks, values, **kw)


def call(fn, name, **more):
    """fn = binding.volume_split_host or an engine's volume_split, on the named case, ids asked for"""
    masks, values, kw = cases()[name]
    return fn(masks, values, want_ids=True, **dict(kw, **more))


def sizes(ref, k=0):
    return [q["voxels"] for q in ref["planes"][k]["pieces"]]


def assert_not_degenerate():
    """what the named cases must show before any implementation is asked, on this reference alone"""
    s = two_balls() == 1
    assert int(s.sum()) == 4217 and ndimage.label(s, structure(26))[1] == 1
    for neck, core_voxels, reach in ((3, 1030, 5), (5, 246, 8)):
        r = case_ref(f"two_balls_neck{neck}")
        assert r["stats"][0]["core_voxels"] == core_voxels and sizes(r) == [2109, 2108] and r["stats"][0]["max_reach"] == reach, (neck, r["stats"])
    assert int((aniso() == 1).sum()) == 13296
    r = case_ref("aniso_neck100")
    assert sizes(r) == [6702, 6594] and r["stats"][0]["max_reach"] == 169, r["stats"]
    tie = r["planes"][0]["ids"][:, :, 38]                       # the tie plane x = 38 goes to the smaller marker, the left ball
    left = r["planes"][0]["ids"][4, 20, 18]
    assert np.all(tie[aniso()[:, :, 38] == 1] == left)
    assert sizes(case_ref("aniso_neck60")) == [13296]
    for conn in (6, 26):
        assert sizes(case_ref(f"chain_{conn}")) == [6942, 5012, 1430], conn
    ids = case_ref("chain_26")["planes"][0]["ids"]              # two pieces cross the 64-lane tile borders at x = 64 and x = 128
    assert ids[8, 12, 63] == ids[8, 12, 64] and ids[8, 12, 127] == ids[8, 12, 128]
    for w, size, reach in ((64, 611, 1269), (130, 1172, 2556)):
        r = case_ref(f"serpentine_{w}")
        assert r["stats"][0]["core_voxels"] == 24 and sizes(r) == [size, size] and r["stats"][0]["max_reach"] == reach, (w, r["stats"])
    # neck 1 is below every unit of (2, 3, 5): the pieces are the components (180, 62 and 82 of them for the values 1, 2, 3 under 18)
    r = case_ref("identity_u235_18")
    assert r["found"] == list(volume_ref.noise_ref(NOISE_SHAPE, 18)[2]) == [180, 62, 82], r["found"]
    assert all(st["cores"] == st["cores_kept"] == st["pieces"] and st["coreless"] == 0 and st["max_reach"] == 0 for st in r["stats"])
    r = case_ref("cap_below_found")
    assert all(f > 7 for f in r["found"]) and (r["ids"] == -1).any()
    r = case_ref("all_coreless")
    assert all(st["cores_kept"] == 0 and st["coreless"] == st["pieces"] > 0 for st in r["stats"])
    assert case_ref("value_absent")["found"][1] == 0
    # the noise cases split something: more pieces than components, cut faces, and coreless pieces beside cored ones
    r = case_ref("noise_6_neck1_core5")
    assert any(st["coreless"] > 0 and st["cores_kept"] > 0 and st["cores_kept"] < st["cores"] for st in r["stats"]), r["stats"]
    r = case_ref("noise_18_neck1_core1")
    assert all(st["pieces"] < st["cores"] + st["coreless"] + 1 for st in r["stats"])
    assert sum(q["cut_x"] for q in r["planes"][2]["pieces"]) == 176 and r["stats"][2]["pieces"] == 159
