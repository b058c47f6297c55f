"""Reference of the volume clean-up (include/mi_unet.h: mi_unet_volume_clean) in numpy, by brute force.  It shares no
code with the product: the ball by enumerating offsets, a dilation as an OR over shifted copies of an array padded with False, an
erosion as an AND over shifted copies padded with True, the fill as the background reached from the six faces by repeated
cross-dilation until nothing changes.  Also the cases the CPU and the GPU tests share, and the conditions under which they are worth
asking (checked on this reference alone)."""
import functools
import itertools

import numpy as np

UNITS = ((1, 1, 1), (2, 2, 5), (3, 1, 7))                   # (ux, uy, uz)
SHAPES = ((5, 40, 72), (7, 33, 70), (1, 48, 80), (3, 1, 130), (9, 17, 1), (2, 3, 300))
VALUES = (1, 2, 3, 4)                                       # three values of the noise, and 4, which is absent
STAT_FIELDS = ("value", "reserved", "in_voxels", "filled", "closed", "opened", "out_voxels")


def radius_pairs(units):
    """(close_r, open_r): two working pairs, two whose balls are the single voxel, one whose ball is deeper than a 5-slice stack"""
    ux, uy, uz = units
    m = max(ux, uy)
    return ((2 * m, m), (uz, 2 * uz), (0, 0), (min(units) - 1, min(units) - 1), (3 * uz, uz))


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def ball_extent(units, r):
    return r // units[0], r // units[1], r // units[2]


def ball_offsets(units, r):
    """[(dz, dy, dx)] of B(r) under units (ux, uy, uz)"""
    ex, ey, ez = ball_extent(units, r)
    return [(dz, dy, dx) for dz in range(-ez, ez + 1) for dy in range(-ey, ey + 1) for dx in range(-ex, ex + 1)
            if (dx * units[0]) ** 2 + (dy * units[1]) ** 2 + (dz * units[2]) ** 2 <= r * r]


def ball_elem(units, r):
    """((ex, ey, ez), u8 [2ez+1, 2ey+1, 2ex+1])"""
    ex, ey, ez = ball_extent(units, r)
    e = np.zeros((2 * ez + 1, 2 * ey + 1, 2 * ex + 1), np.uint8)
    for dz, dy, dx in ball_offsets(units, r):
        e[dz + ez, dy + ey, dx + ex] = 1
    return (ex, ey, ez), e


def _shifted_views(s, offsets, outside):
    """s(p + o) for every offset o that can reach into the volume, positions outside it reading `outside`"""
    d, h, w = s.shape
    offsets = [o for o in offsets if abs(o[0]) < d and abs(o[1]) < h and abs(o[2]) < w]     # (further ones read only padding)
    pz, py, px = (max([abs(o[a]) for o in offsets] + [0]) for a in range(3))
    p = np.pad(s, ((pz, pz), (py, py), (px, px)), constant_values=outside)
    for dz, dy, dx in offsets:
        yield p[pz + dz:pz + dz + d, py + dy:py + dy + h, px + dx:px + dx + w]


def dilate(s, offsets):
    """seeded only by voxels inside the volume (B is symmetric, so the OR over s(p + o) is the union of the translates)"""
    out = np.zeros_like(s)
    for v in _shifted_views(s, offsets, False):
        out |= v
    return out


def erode(s, offsets, outside=True):
    """constrained only by voxels inside the volume; outside=False is the other border rule (not the product's)"""
    out = np.ones_like(s)
    if not outside and any(abs(o[a]) >= s.shape[a] for o in offsets for a in range(3)):
        return np.zeros_like(s)
    for v in _shifted_views(s, offsets, outside):
        out &= v
    return out


CROSS = ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def fill(s):
    """s and every background voxel no 6-connected background path joins to a face of the volume"""
    bg = ~s
    faces = np.zeros_like(s)
    faces[0] = faces[-1] = True
    faces[:, 0] = faces[:, -1] = True
    faces[:, :, 0] = faces[:, :, -1] = True
    reached = bg & faces
    while True:
        grown = dilate(reached, CROSS) & bg
        if np.array_equal(grown, reached):
            return s | ~reached
        reached = grown


def clean_set(s, units, do_fill, close_r, open_r, erode_outside=True):
    """(the cleaned set, its stats without the value)"""
    s = s.astype(bool)
    n_in = int(s.sum())
    if do_fill:
        s = fill(s)
    n_fill = int(s.sum())
    bc, bo = ball_offsets(units, close_r), ball_offsets(units, open_r)
    s = erode(dilate(s, bc), bc, erode_outside)
    n_close = int(s.sum())
    s = dilate(erode(s, bo, erode_outside), bo)
    n_open = int(s.sum())
    return s, dict(reserved=0, in_voxels=n_in, filled=n_fill - n_in, closed=n_close - n_fill, opened=n_close - n_open, out_voxels=n_open)


def clean(masks, values, units, do_fill=True, close_r=0, open_r=0):
    """(out u8 [n, D, H, W], [n] dicts)"""
    out, stats = np.zeros((len(values),) + masks.shape, np.uint8), []
    for k, v in enumerate(values):
        s, st = clean_set(masks == v, units, do_fill, close_r, open_r)
        out[k][s] = v
        stats.append(dict(st, value=int(v)))
    return out, stats


def assert_equal(got_out, got_stats, ref, where=""):
    """got: (out, VCLEAN_DTYPE [n]); ref: clean()'s pair.  Every byte and every field, exactly."""
    ref_out, ref_stats = ref
    assert got_out.shape == ref_out.shape and got_out.dtype == np.uint8, (where, got_out.shape)
    assert np.array_equal(got_out, ref_out), (where, int((got_out != ref_out).sum()))
    assert got_stats.shape == (len(ref_stats),), (where, got_stats.shape)
    for k, r in enumerate(ref_stats):
        for f in STAT_FIELDS:
            assert int(got_stats[k][f]) == r[f], (where, k, f, int(got_stats[k][f]), r[f])


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(shape):
    """u8 [D, H, W] with values 0 .. 3: five random ellipsoids with semi-axes max(1.6, 0.08 .. 0.28 of each side), ellipsoid i of value
    1 + i % 3, every other one hollowed where its normalised radius^2 < 0.3, then 3 % salt-and-pepper: a background voxel drawn becomes
    a random value, any other becomes background"""
    rng = np.random.default_rng(15 + shape[0] * 1000 + shape[1])
    vol = np.zeros(shape, np.uint8)
    zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    for i in range(5):
        c = [rng.uniform(0, n - 1) for n in shape]
        a = [max(1.6, rng.uniform(0.08, 0.28) * n) for n in shape]
        q = ((zz - c[0]) / a[0]) ** 2 + ((yy - c[1]) / a[1]) ** 2 + ((xx - c[2]) / a[2]) ** 2
        vol[(q <= 1.0) & ((q >= 0.3) if i % 2 == 0 else True)] = 1 + i % 3
    hit = rng.random(shape) < 0.03
    draw = rng.integers(1, 4, shape, dtype=np.uint8)
    vol[hit] = np.where(vol[hit] == 0, draw[hit], 0)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def binary(shape):
    """u8 [D, H, W] of 0 / 1: the case's voxels of any value -- the ellipsoids XOR the salt-and-pepper, as one set"""
    vol = (case(shape) != 0).astype(np.uint8)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def case_ref(shape, units, pair, do_fill):
    """clean() of the case for VALUES, computed once"""
    out, stats = clean(case(shape), VALUES, units, do_fill, pair[0], pair[1])
    out.setflags(write=False)
    return out, stats


@functools.lru_cache(maxsize=None)
def binary_ref(shape, units, pair, do_fill):
    """clean() of the binary case for the value 1, computed once"""
    out, stats = clean(binary(shape), (1,), units, do_fill, pair[0], pair[1])
    out.setflags(write=False)
    return out, stats


def all_cases():
    for shape in SHAPES:
        for units in UNITS:
            for pair in radius_pairs(units):
                for do_fill in (True, False):
                    yield shape, units, pair, do_fill


def permuted(vol, units, perm):
    """the volume with its axes permuted (new axis i = old axis perm[i]) and the units (ux, uy, uz) along with them"""
    zyx = (units[2], units[1], units[0])
    nz, ny, nx = (zyx[perm[i]] for i in range(3))
    return np.ascontiguousarray(vol.transpose(perm)), (nx, ny, nz)


PERMS = tuple(itertools.permutations(range(3)))
MIRRORS = tuple(itertools.chain.from_iterable(itertools.combinations(range(3), k) for k in range(1, 4)))


# ---- hand-built fill cases on (7, 9, 11): (name, volume of 0 / 1, the voxels the fill adds) ------------------------------------------------
def _shell(vol, z0, z1, y0, y1, x0, x1):
    """the one-voxel-thick walls of the box z0 .. z1, y0 .. y1, x0 .. x1 (inclusive)"""
    vol[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = 1
    vol[z0 + 1:z1, y0 + 1:y1, x0 + 1:x1] = 0


def fill_cases():
    shape = (7, 9, 11)
    inner = 3 * 5 * 7                                           # the cavity of the shell z 1 .. 5, y 1 .. 7, x 1 .. 9
    out = []
    v = np.zeros(shape, np.uint8); _shell(v, 1, 5, 1, 7, 1, 9)
    out.append(("closed shell", v, inner))
    t = v.copy(); t[3, 4, 1] = 0                                # the middle of the wall x = 1: the cavity reaches the outside through a face
    out.append(("tunnel through a wall", t, 0))
    e = v.copy(); e[1, 1, 5] = 0                                # on the edge of the walls z = 1 and y = 1: (2, 2, 5) touches it only across an edge
    out.append(("edge-diagonal leak", e, inner))
    c = v.copy(); c[1, 1, 1] = 0                                # the corner: (2, 2, 2) touches it only across a corner
    out.append(("corner-diagonal leak", c, inner))
    f = np.zeros(shape, np.uint8); _shell(f, 0, 5, 1, 7, 1, 9); f[0, 2:7, 2:9] = 0      # the sixth wall is the face z = 0 of the volume
    out.append(("open towards a face of the volume", f, 0))
    n = v.copy(); _shell(n, 2, 4, 3, 5, 4, 6)                   # a 3 x 3 x 3 shell inside: its walls are set, its one-voxel cavity is filled
    out.append(("nested shells", n, inner - 27 + 1))
    return out


# ---- non-degeneracy, on the reference alone ----------------------------------------------------------------------------------------------
def assert_not_degenerate():
    """The conditions the noise case must meet before any implementation is asked, for every shape and unit triple and the first two
    radius pairs, on the binary case (a single value of the label volume is too thin a set on the small shapes: the open removes it
    whole): the close adds voxels and the open removes some; the result is neither empty nor full; and it differs from the one an
    erosion with outside = not-set would give, so the border rule is exercised.  In the label volume value 4 is absent, the other
    three are present.  The hand-built cases give their hand-computed counts on the reference."""
    for shape in SHAPES:
        vol = case(shape)
        assert not (vol == 4).any() and all((vol == v).any() for v in VALUES[:3]), shape
        for units in UNITS:
            for pair in radius_pairs(units)[:2]:
                s, st = clean_set(vol != 0, units, False, pair[0], pair[1])
                assert st["closed"] > 0 and st["opened"] > 0, (shape, units, pair, st)
                assert 0 < st["out_voxels"] < vol.size, (shape, units, pair, st)
                other, _ = clean_set(vol != 0, units, False, pair[0], pair[1], erode_outside=False)
                assert not np.array_equal(s, other), (shape, units, pair)
    for name, vol, added in fill_cases():
        _, st = clean_set(vol == 1, (1, 1, 1), True, 0, 0)
        assert st["filled"] == added, (name, st, added)
