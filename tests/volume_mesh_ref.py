"""Reference of the volume mesh (include/mi_unet.h: mi_unet_volume_mesh) in vectorised numpy, written from the
definition's text and sharing no code with the product: the exposed faces from six shifted copies of the padded set, the vertices as
the sorted unique corners the quads use (not through the cut-edge count, which the product uses), the surface-nets offsets from the
eight memberships round a corner.  Also the metrics, the cases the CPU and the GPU tests share, and the conditions under which they
are worth asking (checked on this reference alone)."""
import functools

import numpy as np

import volume_ref as vr

FACES, NETS = 0, 1
PLACEMENTS = (("faces", FACES), ("nets", NETS))
VERTEX_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32), ("ox", np.int8), ("oy", np.int8), ("oz", np.int8), ("n", np.uint8)])
STAT_FIELDS = ("value", "placement", "quads", "verts", "quads_x", "quads_y", "quads_z")

# direction d -> the neighbour's offset (dx, dy, dz), in the order -x, +x, -y, +y, -z, +z
DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
# direction d -> the four corners of the face relative to the voxel, (dx, dy, dz) each: from the corner with the smallest index,
# counter-clockwise seen from outside.  +x and -x are the definition's examples; the others follow by the cyclic change x -> y -> z -> x
# of the two in-face axes ((y, z) for x, (z, x) for y, (x, y) for z), reversed on the negative side.
CORNERS = (((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)),
           ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)),
           ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)),
           ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)),
           ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)),
           ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)))


def exposure(s):
    """bool [D, H, W, 6]: voxel in s whose 6-neighbour in direction d is not (outside the volume is not)"""
    s = np.asarray(s, bool)
    d, h, w = s.shape
    p = np.pad(s, 1, constant_values=False)
    e = np.zeros(s.shape + (6,), bool)
    for k, (dx, dy, dz) in enumerate(DIRS):
        e[..., k] = s & ~p[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return e


def mesh_set(s, placement):
    """one plane by the definition -> (verts VERTEX_DTYPE [V], quads int32 [Q, 4], dict of the counts)"""
    s = np.asarray(s, bool)
    d, h, w = s.shape
    e = exposure(s)
    vox, dirs = np.nonzero(e.reshape(-1, 6))                    # row-major: by voxel index, then by direction
    z, rem = np.divmod(vox, h * w)
    y, x = np.divmod(rem, w)
    off = np.asarray(CORNERS, np.int64)[dirs]                   # [Q, 4, 3]
    ci, cj, ck = x[:, None] + off[..., 0], y[:, None] + off[..., 1], z[:, None] + off[..., 2]
    c = (ck * (h + 1) + cj) * (w + 1) + ci                      # [Q, 4]
    assert (c[:, 0:1] <= c).all()                               # every quad starts at its smallest corner
    used = np.unique(c)
    quads = np.searchsorted(used, c).astype(np.int32).reshape(-1, 4)
    verts = np.zeros(used.size, VERTEX_DTYPE)
    k, rem = np.divmod(used, (h + 1) * (w + 1))
    j, i = np.divmod(rem, w + 1)
    verts["x"], verts["y"], verts["z"] = i, j, k
    # the eight voxels round corner (i, j, k) are (i - 1 .. i, j - 1 .. j, k - 1 .. k): m[dz][dy][dx] from the padded set
    p = np.pad(s, 1, constant_values=False)
    m = np.array([[[p[k + dz, j + dy, i + dx] for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)])      # [2, 2, 2, V]
    n = np.zeros(used.size, np.int64)
    o = np.zeros((3, used.size), np.int64)                      # ox, oy, oz
    for a in (0, 1):
        for b in (0, 1):
            cut = m[b, a, 0] != m[b, a, 1]                      # the edge along x at dy = a, dz = b
            n += cut; o[1] += cut * (2 * a - 1); o[2] += cut * (2 * b - 1)
            cut = m[b, 0, a] != m[b, 1, a]                      # along y at dx = a, dz = b
            n += cut; o[0] += cut * (2 * a - 1); o[2] += cut * (2 * b - 1)
            cut = m[0, b, a] != m[1, b, a]                      # along z at dx = a, dy = b
            n += cut; o[0] += cut * (2 * a - 1); o[1] += cut * (2 * b - 1)
    assert (n >= 1).all()
    if placement == NETS:
        verts["ox"], verts["oy"], verts["oz"], verts["n"] = o[0], o[1], o[2], n
    else:
        assert placement == FACES
        verts["n"] = 1
    counts = dict(placement=int(placement), quads=int(vox.size), verts=int(used.size),
                  quads_x=int((dirs < 2).sum()), quads_y=int(((dirs >= 2) & (dirs < 4)).sum()), quads_z=int((dirs >= 4).sum()))
    return verts, quads, counts


def mesh(masks, values, placement):
    """[(verts, quads, stat dict)] per value"""
    out = []
    for v in values:
        verts, quads, st = mesh_set(np.asarray(masks) == v, placement)
        out.append((verts, quads, dict(st, value=int(v))))
    return out


def assert_equal(got, ref, where="", cap_verts=None, cap_quads=None):
    """got: (meshes [(verts, quads)] per value, stats MESH_STAT_DTYPE [n]) as the binding returns them; ref: mesh()'s list.  Every
    byte and every field, exactly.  With caps: got holds the first min(count, cap) entries, the stats are the uncapped ones."""
    meshes, stats = got
    assert len(meshes) == len(ref) and stats.shape == (len(ref),), (where, len(meshes), stats.shape)
    for k, (rv, rq, rs) in enumerate(ref):
        for f in STAT_FIELDS:
            assert int(stats[k][f]) == rs[f], (where, k, f, int(stats[k][f]), rs[f])
        gv, gq = meshes[k]
        kv = rv.size if cap_verts is None else min(rv.size, cap_verts)
        kq = rq.shape[0] if cap_quads is None else min(rq.shape[0], cap_quads)
        assert gv.shape == (kv,) and gq.shape == (kq, 4) and gq.dtype == np.int32, (where, k, gv.shape, gq.shape)
        assert gv.tobytes() == rv[:kv].astype(gv.dtype).tobytes(), (where, k, "verts")
        assert np.array_equal(gq, rq[:kq]), (where, k, "quads", int((gq != rq[:kq]).any(axis=1).sum()))


# ---- the metrics ---------------------------------------------------------------------------------------------------------------------------
def positions64(verts, spacing):
    """float64 [V, 3]: (corner + o / (2 n)) * spacing per axis"""
    sp = np.asarray(spacing, np.float64)
    c = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)
    o = np.stack([verts["ox"], verts["oy"], verts["oz"]], 1).astype(np.float64)
    return (c + o / (2.0 * verts["n"].astype(np.float64))[:, None]) * sp


def triangles(quads):
    """int [2 Q, 3]: (0, 1, 2), (0, 2, 3) of every quad, in order"""
    q = np.asarray(quads)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)


def derive(verts, quads, spacing):
    """dict(area_mm2, volume_mm3) in float64 (numpy's sums: pairwise, not the product's sequential ones)"""
    p = positions64(verts, spacing)
    t = triangles(quads)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0
    return dict(area_mm2=float(area.sum()), volume_mm3=float(vol.sum()))


def det_sum(verts, quads):
    """the integer sum over the triangles of det(a, b, c) of the corner coordinates: 6 |S| under the outward orientation"""
    p = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.int64)
    t = triangles(quads)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return int(np.einsum("ij,ij->i", a, np.cross(b, c)).sum())


def directed_edges(quads):
    """(pairs int64 [4 Q, 2] a -> b round every quad)"""
    q = np.asarray(quads, np.int64)
    return np.stack([q, np.roll(q, -1, axis=1)], 2).reshape(-1, 2)


def edge_balance(quads, nv):
    """(every directed edge a -> b occurs as often as b -> a, the number of undirected edges, those used by more than two quads)"""
    e = directed_edges(quads)
    fwd, cf = np.unique(e[:, 0] * nv + e[:, 1], return_counts=True)
    bwd, cb = np.unique(e[:, 1] * nv + e[:, 0], return_counts=True)
    balanced = np.array_equal(fwd, bwd) and np.array_equal(cf, cb)
    und, cu = np.unique(np.minimum(e[:, 0], e[:, 1]) * nv + np.maximum(e[:, 0], e[:, 1]), return_counts=True)
    return bool(balanced), int(und.size), int((cu > 2).sum())


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
NOISE_SHAPES = ((7, 40, 72), (3, 64, 64), (16, 24, 130))      # volume_ref's 3-D noise shapes: W = 72 and 130 are no multiples of 64
NOISE_VALUES = (1, 2, 3)
FLAT_SHAPE = (1, 48, 80)                                      # its one-slice shape (every corner has at most four voxels: n <= 8)


def noise(shape):
    return vr.smooth_noise(shape)


@functools.lru_cache(maxsize=None)
def noise_ref(shape, placement):
    """mesh() of the smooth-noise volume for NOISE_VALUES, computed once"""
    return mesh(noise(shape), NOISE_VALUES, placement)


def ball(r, pad=2):
    """u8 0 / 1: the voxels whose centre is within r of the centre of a cube of side 2 (r + pad) + 1"""
    n = 2 * (int(r) + pad) + 1
    g = np.arange(n, dtype=np.float64) - (n - 1) / 2
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    return (zz * zz + yy * yy + xx * xx <= r * r).astype(np.uint8)


def checkerboard(shape=(4, 5, 6)):
    zz, yy, xx = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return ((zz + yy + xx) % 2 == 0).astype(np.uint8)


def two_shells(shape=(24, 44, 640)):
    """a box shell that touches all six faces of the volume and a second one inside it, walls one voxel thick"""
    d, h, w = shape
    v = np.zeros(shape, np.uint8)
    v[:] = 1; v[1:-1, 1:-1, 1:-1] = 0
    v[4:d - 4, 6:h - 6, 9:w - 9] = 1; v[5:d - 5, 7:h - 7, 10:w - 10] = 0
    return v


def known_answers():
    """[(name, masks u8 [D, H, W], values, (verts, quads) of the first value under either placement)]"""
    def vol(shape, *voxels):
        v = np.zeros(shape, np.uint8)
        for z, y, x in voxels:
            v[z, y, x] = 1
        return v
    cb = checkerboard()
    labels = np.zeros((3, 4, 5), np.uint8)
    labels[0, :2] = 7; labels[1:, 2:, 1:4] = 9; labels[2, 0, 0] = 200
    return [("one voxel", vol((3, 3, 3), (1, 1, 1)), (1,), (8, 6)),
            ("one voxel that is the volume", np.ones((1, 1, 1), np.uint8), (1,), (8, 6)),
            ("two sharing a face", vol((3, 3, 4), (1, 1, 1), (1, 1, 2)), (1,), (12, 10)),
            ("two sharing an edge", vol((3, 4, 4), (1, 1, 1), (1, 2, 2)), (1,), (14, 12)),
            ("two sharing a corner", vol((4, 4, 4), (1, 1, 1), (2, 2, 2)), (1,), (15, 12)),
            ("full 2 x 3 x 4", np.ones((2, 3, 4), np.uint8), (1,), (54, 52)),
            ("one slice", np.pad(np.ones((1, 2, 3), np.uint8), ((0, 0), (1, 1), (1, 1))), (1,), (24, 22)),
            ("a row", np.ones((1, 1, 70), np.uint8), (1,), (4 * 71, 4 * 70 + 2)),
            ("checkerboard", cb, (1,), (206, 6 * int(cb.sum()))),
            ("empty plane", np.zeros((2, 3, 4), np.uint8), (1,), (0, 0)),
            ("absent value", np.ones((2, 3, 4), np.uint8), (5, 1), (0, 0)),
            ("label volume", labels, (7, 9, 200, 0), (2 * 3 * 6, 2 * (10 + 5 + 2)))]


# ---- non-degeneracy, on the reference alone ----------------------------------------------------------------------------------------------
def assert_not_degenerate():
    """The conditions the noise cases must meet before any implementation is asked: for every 3-D noise shape and every value, the
    vertices show every cut-edge count n from 3 to at least 9 (a cut of the cube's edge graph has 3 .. 9 or 12 edges: no vertex has n
    of 1 or 2, and 3 must be the smallest seen), some undirected edge is used by more than two quads (a non-manifold edge), and every
    one of the six faces of the volume carries a quad.  In the one-slice shape half of every corner's voxels lie outside; n is the
    voxels of the corner in the set plus the 0, 2 or 4 cuts between them, 3 .. 6, and all four are asked for."""
    for shape in NOISE_SHAPES + (FLAT_SHAPE,):
        vol = noise(shape)
        d, h, w = shape
        for v in NOISE_VALUES:
            verts, quads, st = mesh_set(vol == v, NETS)
            top = 6 if d == 1 else 9
            have = set(np.unique(verts["n"]).tolist())
            assert set(range(3, top + 1)) <= have and min(have) == 3, (shape, v, sorted(have))
            assert edge_balance(quads, verts.size)[2] > 0, (shape, v)
            e = exposure(vol == v)
            on_face = (e[:, :, 0, 0].any(), e[:, :, w - 1, 1].any(), e[:, 0, :, 2].any(), e[:, h - 1, :, 3].any(), e[0, :, :, 4].any(),
                       e[d - 1, :, :, 5].any())
            assert all(on_face), (shape, v, on_face)
