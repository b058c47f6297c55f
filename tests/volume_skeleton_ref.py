"""Reference for the volume skeleton (include/mi_unet.h: mi_unet_volume_skeleton), written from the definition in numpy /
Python and importing nothing from the library: the simple-point test as two flood fills over adjacency lists (memoised per code), the
schedule voxel by voxel, the radius as a brute-force minimum over the wrapped volume, the table, the derived doubles; topology counters
that use none of the thinning code (scipy's labels, the Euler characteristic of the cubical complex); and the registry of cases the CPU
and GPU tests share."""
import functools
import math

import numpy as np
from scipy import ndimage

MAX_TABLE = 4096
MAX_SIDE = 8192
SKEL_BYTES, INFO_BYTES = 112, 16
COUNT_FIELDS = ("voxels_in", "voxels", "ends", "isolated", "junctions", "r2_sum", "r2_min", "r2_max")

# the 26 offsets (dz, dy, dx) in raster order without the centre: bit i of a code belongs to OFF[i]
OFF = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
_L1 = [abs(a) + abs(b) + abs(c) for a, b, c in OFF]
ADJ26 = [[j for j, q in enumerate(OFF) if j != i and max(abs(q[0] - o[0]), abs(q[1] - o[1]), abs(q[2] - o[2])) <= 1] for i, o in enumerate(OFF)]
N18 = [i for i in range(26) if _L1[i] <= 2]
FACE = [i for i in range(26) if _L1[i] == 1]
ADJ6 = {i: [j for j in N18 if sum(abs(a - b) for a, b in zip(OFF[i], OFF[j])) == 1] for i in N18}
# the phases: z - 1, z + 1, y - 1, y + 1, x - 1, x + 1 as (dz, dy, dx)
DIRS = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
SIMPLE, NOT_OBJECT, NOT_BACKGROUND = "simple", "object", "background"


@functools.lru_cache(maxsize=None)
def classify(code):
    """SIMPLE, or which of the two conditions of the definition fails first"""
    obj = [i for i in range(26) if code >> i & 1]
    if not obj:
        return NOT_OBJECT
    seen, stack = {obj[0]}, [obj[0]]
    while stack:
        a = stack.pop()
        for b in ADJ26[a]:
            if code >> b & 1 and b not in seen:
                seen.add(b)
                stack.append(b)
    if len(seen) != len(obj):
        return NOT_OBJECT
    comps, seen = 0, set()
    for f in FACE:
        if code >> f & 1 or f in seen:
            continue
        comps += 1
        seen.add(f)
        stack = [f]
        while stack:
            a = stack.pop()
            for b in ADJ6[a]:
                if not code >> b & 1 and b not in seen:
                    seen.add(b)
                    stack.append(b)
    return SIMPLE if comps == 1 else NOT_BACKGROUND


def is_simple(code):
    return classify(code) == SIMPLE


def simple_bits(first_word, n_words):
    """uint32 [n_words]: code c in bit c & 31 of word (c >> 5) - first_word"""
    out = np.zeros(n_words, np.uint32)
    for w in range(n_words):
        r = 0
        for b in range(32):
            r |= int(is_simple(((first_word + w) << 5) | b)) << b
        out[w] = r
    return out


def _codes(a, pts):
    """the 26 same-object bits of the voxels pts [n, 3] of the padded state a"""
    z, y, x = pts[:, 0], pts[:, 1], pts[:, 2]
    v = a[z, y, x]
    code = np.zeros(len(pts), np.int64)
    for i, (dz, dy, dx) in enumerate(OFF):
        code |= (a[z + dz, y + dy, x + dx] == v).astype(np.int64) << i
    return code


def _neighbour_count(a):
    """same-object neighbours of every voxel of the padded state (0 where it holds no id)"""
    n = np.zeros(a.shape, np.int32)
    for dz, dy, dx in OFF:
        n += (np.roll(a, (-dz, -dy, -dx), (0, 1, 2)) == a) & (a > 0)
    return n


def skeleton(ids, m, units=(1, 1, 1), max_passes=0, radius=True):
    """-> dict(ids int32 [D,H,W], r2 int32 [D,H,W], table: m dicts, passes, deleted, stable, trace).  trace: deleted per (phase, subfield),
    refusals by reason, for assert_not_degenerate."""
    ids = np.asarray(ids, np.int32)
    d, h, w = ids.shape
    clean = np.where((ids >= 1) & (ids <= m), ids, 0).astype(np.int32)
    a = np.zeros((d + 2, h + 2, w + 2), np.int32)                   # outside the volume is nothing
    a[1:-1, 1:-1, 1:-1] = clean
    trace = dict(deleted=np.zeros((6, 8), np.int64), refused={NOT_OBJECT: 0, NOT_BACKGROUND: 0, "end": 0})
    passes = deleted = 0
    while True:
        gone = 0
        endm = _neighbour_count(a) == 1
        for di, (dz, dy, dx) in enumerate(DIRS):
            nb = np.roll(a, (-dz, -dy, -dx), (0, 1, 2))
            cand = np.argwhere((a > 0) & (nb != a))
            sub = ((cand[:, 2] - 1) & 1) | (((cand[:, 1] - 1) & 1) << 1) | (((cand[:, 0] - 1) & 1) << 2)
            for s in range(8):
                pts = cand[sub == s]
                if not len(pts):
                    continue
                assert (a[pts[:, 0], pts[:, 1], pts[:, 2]] > 0).all()   # a candidate still exists: only its own sub-step deletes it
                codes = _codes(a, pts)
                dele = []
                for p, code in zip(pts, codes.tolist()):
                    if endm[p[0], p[1], p[2]]:
                        trace["refused"]["end"] += 1
                        continue
                    why = classify(code)
                    if why == SIMPLE:
                        dele.append(p)
                    else:
                        trace["refused"][why] += 1
                for p in dele:
                    a[p[0], p[1], p[2]] = 0
                gone += len(dele)
                trace["deleted"][di, s] += len(dele)
        passes += 1
        deleted += gone
        stable = int(gone == 0)
        if stable or (max_passes > 0 and passes >= max_passes):
            break
    skel = np.ascontiguousarray(a[1:-1, 1:-1, 1:-1])
    # RADIUS: the brute-force minimum over every voxel of the wrapped volume that carries another id
    r2 = np.zeros((d, h, w), np.int32)
    if radius:
        pad = np.zeros((d + 2, h + 2, w + 2), np.int64)
        pad[1:-1, 1:-1, 1:-1] = ids                                 # the ids as given
        zz, yy, xx = np.indices(pad.shape)
        ux, uy, uz = units
        for z, y, x in np.argwhere(skel > 0):
            d2 = ((xx - (x + 1)) * ux) ** 2 + ((yy - (y + 1)) * uy) ** 2 + ((zz - (z + 1)) * uz) ** 2
            r2[z, y, x] = int(d2[pad != ids[z, y, x]].min())
    # the table
    nbc = _neighbour_count(a)[1:-1, 1:-1, 1:-1]
    table = []
    for r in range(m):
        sel = skel == r + 1
        links = [0] * 7
        pts = np.argwhere(sel) + 1
        if len(pts):
            codes = _codes(a, pts)
            for i in range(13, 26):                                 # a pair from its voxel of the lower index
                dz, dy, dx = OFF[i]
                links[abs(dx) + 2 * abs(dy) + 4 * abs(dz) - 1] += int((codes >> i & 1).sum())
        vals = r2[sel].astype(np.int64)
        use = radius and len(vals)
        table.append(dict(voxels_in=int((clean == r + 1).sum()), voxels=int(sel.sum()), ends=int((nbc[sel] == 1).sum()),
                          isolated=int((nbc[sel] == 0).sum()), junctions=int((nbc[sel] >= 3).sum()), links=links,
                          r2_sum=int(vals.sum()) if use else 0, r2_min=int(vals.min()) if use else 0, r2_max=int(vals.max()) if use else 0))
    return dict(ids=skel, r2=r2, table=table, passes=passes, deleted=deleted, stable=stable, trace=trace)


def derive(c, spacing, unit_mm):
    """mi_unet_volume_skeleton_derive's arithmetic in Python floats (doubles), in its order"""
    sx, sy, sz = (float(v) for v in spacing)
    length, links = 0.0, 0
    for k in range(7):
        cls = k + 1
        ex, ey, ez = (sx if cls & 1 else 0.0), (sy if cls & 2 else 0.0), (sz if cls & 4 else 0.0)
        length += float(c["links"][k]) * math.sqrt(ex * ex + ey * ey + ez * ez)
        links += int(c["links"][k])
    v = int(c["voxels"])
    return dict(length_mm=length, radius_min_mm=math.sqrt(float(c["r2_min"])) * unit_mm, radius_max_mm=math.sqrt(float(c["r2_max"])) * unit_mm,
                radius_rms_mm=math.sqrt(float(c["r2_sum"]) / float(v)) * unit_mm if v else 0.0, loops=links - v + 1 if v else 0)


# ---- topology, without the thinning code --------------------------------------------------------------------------------------------------
def euler(mask):
    """V - E + F - C of the complex of the closed unit cubes of the set"""
    m = np.pad(np.asarray(mask, bool), 1)

    def cells(axes):
        r = m.copy()
        for ax in axes:
            r = r | np.roll(r, 1, ax)
        return int(r.sum())
    cubes = int(m.sum())
    faces = cells([0]) + cells([1]) + cells([2])
    edges = cells([0, 1]) + cells([0, 2]) + cells([1, 2])
    return cells([0, 1, 2]) - edges + faces - cubes


def topology(mask):
    """(26-components, 6-connected background cavities, Euler characteristic) of one set"""
    mask = np.asarray(mask, bool)
    n26 = ndimage.label(mask, np.ones((3, 3, 3)))[1]
    cavities = ndimage.label(~np.pad(mask, 1))[1] - 1
    return n26, cavities, euler(mask)


def topology_by_id(ids, m):
    return [topology(ids == r + 1) for r in range(m)]


# ---- comparing ---------------------------------------------------------------------------------------------------------------------------------
def assert_equal(got, want, what=""):
    """got: a result of the binding; want: skeleton()'s"""
    assert (got["passes"], got["deleted"], got["stable"]) == (want["passes"], want["deleted"], want["stable"]), (
        what, "info", (got["passes"], got["deleted"], got["stable"]), (want["passes"], want["deleted"], want["stable"]))
    if got["ids"] is not None:
        assert np.array_equal(got["ids"], want["ids"]), (what, "ids", int((got["ids"] != want["ids"]).sum()))
    if got["r2"] is not None:
        assert np.array_equal(got["r2"], want["r2"]), (what, "r2", np.argwhere(got["r2"] != want["r2"])[:5].tolist())
    assert len(got["table"]) == len(want["table"]), (what, len(got["table"]))
    for r, row in enumerate(want["table"]):
        for f in COUNT_FIELDS:
            assert int(got["table"][r][f]) == row[f], (what, "component", r, f, int(got["table"][r][f]), row[f])
        assert [int(v) for v in got["table"][r]["links"]] == row["links"], (what, "component", r, "links")


def same_bytes(a, b, what=""):
    """two results of the binding: the same bytes and the same info (`passes` is part of the definition)"""
    for key in ("table", "ids", "r2"):
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, (what, key)
            continue
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    for key in ("passes", "deleted", "stable"):
        assert a[key] == b[key], (what, key, a[key], b[key])


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def label26(mask):
    return ndimage.label(mask, np.ones((3, 3, 3)))[0].astype(np.int32)


def smooth_noise(shape, seed=7, sigma=2.0, level=0.02):
    rng = np.random.default_rng(seed)
    return ndimage.gaussian_filter(rng.standard_normal(shape), sigma) > level


def ball(shape=(25, 25, 25), centre=(12, 12, 12), r2=81):
    z, y, x = np.indices(shape)
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= r2


def rod(shape=(9, 9, 40), shift=(0, 0, 0)):
    """radius 3 round the x axis through (z, y) = (4, 4), x in 2 .. 37; shift = (dx, dy, dz)"""
    z, y, x = np.indices(shape)
    return ((z - 4 - shift[2]) ** 2 + (y - 4 - shift[1]) ** 2 <= 9) & (x >= 2 + shift[0]) & (x < 38 + shift[0])


def torus():
    z, y, x = np.indices((11, 33, 33))
    r = np.sqrt((y - 16.0) ** 2 + (x - 16.0) ** 2)
    return (r - 11) ** 2 + (z - 5.0) ** 2 <= 9


def shell():
    z, y, x = np.indices((25, 25, 25))
    q = (z - 12) ** 2 + (y - 12) ** 2 + (x - 12) ** 2
    return (q <= 100) & (q >= 36)


def y_shape(shape=(9, 41, 41), origin=(0, 0)):
    """three arms of radius sqrt(6.5) from (20, 20) to (2, 20), (36, 4), (36, 36) in the slice z = 4, moved by origin = (y, x)"""
    z, y, x = np.indices(shape)
    v = np.zeros(shape, bool)
    for t in np.linspace(0, 1, 200):
        for ey, ex in ((2, 20), (36, 4), (36, 36)):
            cy, cx = 20 + (ey - 20) * t + origin[0], 20 + (ex - 20) * t + origin[1]
            v |= (z - 4) ** 2 + (y - cy) ** 2 + (x - cx) ** 2 <= 6.5
    return v


def diamond_ring():
    """|y - 4| + |x - 4| == 3 in the middle slice of 3 x 9 x 9: twelve voxels, each with two diagonal neighbours that are not adjacent"""
    z, y, x = np.indices((3, 9, 9))
    return (z == 1) & (abs(y - 4) + abs(x - 4) == 3)


def seams():
    """id 1: the Y across the tile seams x = 64 and y = 8 .. 32; id 2: a thin rod along x across x = 64 and 128, its axis on the seams
    y = 40 and z = 4; the two touch.  W = 130 and H = 43 are no multiples of the tile (64 x 8 x 4), D = 9 neither."""
    shape = (9, 43, 130)
    z, y, x = np.indices(shape)
    ids = np.zeros(shape, np.int32)
    ids[((z - 4) ** 2 + (y - 40) ** 2 <= 2) & (x >= 3) & (x <= 128)] = 2
    ids[y_shape(shape, (0, 44))] = 1
    return ids


def tubes_in_contact():
    ids = np.zeros((9, 14, 30), np.int32)
    ids[2:7, 2:7, 2:28] = 1
    ids[2:7, 7:12, 2:28] = 2
    return ids


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids int32 [D,H,W], m, keyword arguments of a call)"""
    c = {}
    one = lambda mask: (label26(mask), 1, {})
    c["ball_r9"] = one(ball())
    c["rod"] = one(rod())
    c["torus"] = one(torus())
    c["shell"] = one(shell())
    c["y"] = one(y_shape())
    noise = label26(smooth_noise((12, 32, 32)))
    c["noise"] = (noise, int(noise.max()), {})
    v = np.zeros((3, 3, 3), bool)
    v[1, 1, 1] = True
    c["single_voxel"] = one(v)
    v = np.zeros((3, 3, 4), bool)
    v[1, 1, 1:3] = True
    c["two_voxels"] = one(v)
    v = np.zeros((3, 5, 12), bool)
    v[1, 2, 1:11] = True
    c["line"] = one(v)
    c["ring"] = one(diamond_ring())
    c["full_block"] = (np.ones((6, 7, 8), np.int32), 1, {})
    z, y, x = np.indices((1, 21, 30))
    c["one_slice"] = one(((y - 10) ** 2 * 2 + (x - 14) ** 2 <= 150) & ((y - 10) ** 2 + (x - 10) ** 2 > 6))
    for name, shift in (("rod_x1", (1, 0, 0)), ("rod_y1", (0, 1, 0)), ("rod_z1", (0, 0, 1))):
        c[name] = one(rod((10, 10, 41), shift))
    c["seams"] = (seams(), 2, {})
    c["tubes_in_contact"] = (tubes_in_contact(), 2, {})
    n6 = ndimage.label(smooth_noise((12, 32, 32), sigma=1.2, level=0.08))[0].astype(np.int32)  # faces only: different ids are 26-adjacent
    c["noise_labelled_6"] = (n6, int(n6.max()), {})
    gaps = noise.copy()
    gaps[noise == 2] = 9                                          # above m: nothing
    gaps[noise == 3] = -3
    gaps[noise == 4] = 6                                          # ids 2 .. 5 of m = 6 have no voxel
    c["absent_ids"] = (gaps, 6, {})
    c["aniso_border"] = (label26(ball((12, 14, 16), (3, 3, 3), 49)), 1, dict(units=(2, 3, 5)))
    c["aniso_noise"] = (noise, int(noise.max()), dict(units=(2, 3, 5)))
    c["ball_one_pass"] = (label26(ball()), 1, dict(max_passes=1))
    c["ball_no_radius"] = (label26(ball()), 1, dict(radius=False))
    return c


@functools.lru_cache(maxsize=None)
def case_ref(name):
    ids, m, kw = cases()[name]
    return skeleton(ids, m, **kw)


def call(fn, name, **more):
    """fn = binding.volume_skeleton_host or an engine's volume_skeleton, on the named case, ids asked for, and r2 unless the case is the
    one without radii (a call that asks for r2 computes it whatever `radius` says)"""
    ids, m, kw = cases()[name]
    return fn(ids, m, **dict(dict(want_ids=True, want_r2=kw.get("radius", True)), **dict(kw, **more)))


# what the issue's prototype found on its six cases: voxels in, skeleton voxels, ends, junctions, isolated, passes (over all components)
PROTOTYPE = {"ball_r9": (3071, 1, 0, 0, 1, 6), "rod": (1044, 32, 2, 0, 0, 3), "torus": (1812, 62, 0, 0, 0, 3), "shell": (3274, 654, 0, 654, 0, 3),
             "y": (1446, 31, 3, 1, 0, 3), "noise": (3834, 174, 8, 24, 1, 4)}


def totals(ref):
    t = ref["table"]
    return tuple(sum(r[f] for r in t) for f in ("voxels_in", "voxels", "ends", "junctions", "isolated")) + (ref["passes"],)


def assert_not_degenerate():
    """what the named cases must show before any implementation is asked, on this reference alone"""
    for name, want in PROTOTYPE.items():
        assert totals(case_ref(name)) == want, (name, totals(case_ref(name)), want)
    refs = {name: case_ref(name) for name in cases()}
    deleted = sum(r["trace"]["deleted"] for r in refs.values())
    assert (deleted > 0).all(), deleted                          # every (phase, subfield) sub-step deletes something somewhere
    assert max(r["passes"] for r in refs.values()) >= 4
    for why in (NOT_OBJECT, NOT_BACKGROUND, "end"):
        assert sum(r["trace"]["refused"][why] for r in refs.values()) > 0, why
    assert any(all(sum(row[f] for row in r["table"]) > 0 for f in ("ends", "junctions", "isolated")) and
               all(sum(row["links"][k] for row in r["table"]) > 0 for k in range(7)) for r in refs.values())
    # nothing to delete: one pass
    for name in ("single_voxel", "two_voxels", "line", "ring"):
        r = refs[name]
        assert (r["passes"], r["deleted"], r["stable"]) == (1, 0, 1) and np.array_equal(r["ids"], cases()[name][0]), name
    assert refs["two_voxels"]["table"][0]["ends"] == 2 and refs["ring"]["table"][0]["links"] == [0, 0, 12, 0, 0, 0, 0]
    r = refs["ball_one_pass"]
    assert (r["passes"], r["stable"]) == (1, 0) and r["table"][0]["voxels"] > 1
    # different ids that are 26-adjacent, an id without voxels, a component at the border with a radius from the virtual layer
    n6 = cases()["noise_labelled_6"][0]
    assert ndimage.label(n6 > 0, np.ones((3, 3, 3)))[1] < int(n6.max())
    assert [row["voxels_in"] > 0 for row in refs["absent_ids"]["table"]] == [True, False, False, False, False, True]
    border = cases()["aniso_border"][0]
    assert border[0].any() and border[:, 0].any() and border[:, :, 0].any() and refs["aniso_border"]["table"][0]["r2_min"] > 0
    s = cases()["seams"][0]
    assert (s[:, :, 63:65] == 1).any() and (s[:, :, 127:129] == 2).any() and (s[3:5, 39:41] == 2).any()
