"""Reference of the scores of a volume (include/mi_unet.h: mi_unet_score_volume) in numpy, by brute force.  It shares
no code with the product: boundaries by the 6-neighbour rule on a padded array, d2 as the integer minimum over ALL pairs of boundary
voxels (by broadcasting, in chunks), order statistics by sorting, the q16 root with math.isqrt.  Also the cases the CPU and the GPU
tests share, and the conditions under which they are worth asking (checked on this reference alone)."""
import functools
import itertools
import math

import numpy as np

import volume_ref as vr
from score_ref import DIR_FIELDS, FIELDS, confusion, derive, order_stat, q16  # noqa: F401  (2-D helpers that know no axis)

QUANTILES = (0, 50000, 500000, 999999)
UNITS = ((1, 1, 1), (2, 2, 5), (3, 1, 7))                   # (ux, uy, uz)
SHAPES = ((5, 40, 72), (7, 33, 70), (1, 48, 80), (3, 1, 130), (9, 17, 1))
VALUES = (1, 2, 3, 4)                                       # three values of the noise on both sides, and 4 on the truth side only


def boundary(s):
    """bool [D, H, W]: the voxels of s with a 6-neighbour that is not in s; outside the volume is not in s"""
    s = s.astype(bool)
    p = np.pad(s, 1, constant_values=False)
    inner = p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    return s & ~inner


def pair_d2(ps, pd, units):
    """int64 [len(ps), len(pd)]: squared distances between (z, y, x) points under units (ux, uy, uz)"""
    w = np.array([units[2], units[1], units[0]], np.int64)
    d = (ps[:, None, :] - pd[None, :, :]) * w
    return (d * d).sum(-1)


def _chunks(ps, pd):
    step = max(1, 3_000_000 // max(len(pd), 1))
    return range(0, len(ps), step), step


def directed_d2(src, dst, units):
    """int64 [n_src]: for every voxel of bool volume src (raster order) the minimum d2 to a voxel of dst (not empty)"""
    ps, pd = np.argwhere(src).astype(np.int64), np.argwhere(dst).astype(np.int64)
    out = np.empty(len(ps), np.int64)
    starts, step = _chunks(ps, pd)
    for i in starts:
        out[i:i + step] = pair_d2(ps[i:i + step], pd, units).min(1)
    return out


def _direction(d2, n, have, quantile_ppm):
    if not have:
        return dict(n=n, max_d2=-1, q_d2=-1, reserved=0, sum_d2=0, sum_d_q16=0)
    return dict(n=n, max_d2=int(d2.max()), q_d2=order_stat(d2, quantile_ppm), reserved=0, sum_d2=int(d2.sum()),
                sum_d_q16=sum(q16(v) for v in d2))


def plane_d2(pred, truth, value, units):
    """(boundary of A, boundary of T, d2 of dA -> dT, d2 of dT -> dA); the two arrays are empty when a boundary is"""
    ba, bt = boundary(pred == value), boundary(truth == value)
    have = bool(ba.any()) and bool(bt.any())
    none = np.zeros(0, np.int64)
    return ba, bt, (directed_d2(ba, bt, units) if have else none), (directed_d2(bt, ba, units) if have else none)


def score_plane(pred, truth, value, units, quantile_ppm=50000, d2=None):
    a, t = pred == value, truth == value
    ba, bt, da, dt = d2 if d2 is not None else plane_d2(pred, truth, value, units)
    na, nt = int(ba.sum()), int(bt.sum())
    have = na > 0 and nt > 0
    return dict(tp=int((a & t).sum()), fp=int((a & ~t).sum()), fn=int((t & ~a).sum()),
                q_d2_sym=order_stat(np.concatenate([da, dt]), quantile_ppm) if have else -1, value=int(value),
                quantile_ppm=int(quantile_ppm), a_to_t=_direction(da, na, have, quantile_ppm), t_to_a=_direction(dt, nt, have, quantile_ppm))


def score_volume(pred, truth, values, units, quantile_ppm=50000):
    """[n] dicts"""
    return [score_plane(pred, truth, v, units, quantile_ppm) for v in values]


def assert_equal(got, ref, where=""):
    """got: SCORE_DTYPE [n]; ref: score_volume's dicts.  Every field, exactly."""
    assert got.shape == (len(ref),), (got.shape, where)
    for k, r in enumerate(ref):
        g = got[k]
        for f in FIELDS:
            assert int(g[f]) == r[f], (where, k, f, int(g[f]), r[f])
        for d in ("a_to_t", "t_to_a"):
            for f in DIR_FIELDS:
                assert int(g[d][f]) == r[d][f], (where, k, d, f, int(g[d][f]), r[d][f])


def derive_mm(r, unit_mm):
    """mi_unet_score_volume_derive's arithmetic in Python floats"""
    m = derive(r)
    for f in ("hd", "hd_q", "assd", "rmsd"):
        m[f] = m[f] * unit_mm
    return m


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def shifted(vol, shift):
    """vol moved by shift = (dz, dy, dx), zeros moving in; a shift is cut to what the axis has room for"""
    out = np.zeros_like(vol)
    src, dst = [], []
    for n, s in zip(vol.shape, shift):
        s = max(-(n - 1), min(n - 1, s))
        dst.append(slice(max(s, 0), n + min(s, 0)))
        src.append(slice(max(-s, 0), n + min(-s, 0)))
    out[tuple(dst)] = vol[tuple(src)]
    return out


@functools.lru_cache(maxsize=None)
def case(shape):
    """(pred, truth) u8 [D, H, W]: truth = the smooth noise of volume_ref with a block of value 4 that pred does not have; pred = the
    noise moved by (1, 2, -3) with 3 % of its voxels re-drawn"""
    truth = np.array(vr.smooth_noise(shape))
    pred = shifted(truth, (1, 2, -3))
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    redraw = rng.random(shape) < 0.03
    pred[redraw] = rng.integers(0, 4, shape, dtype=np.uint8)[redraw]
    d, h, w = shape
    truth[d // 2:d // 2 + 2, h // 3:h // 3 + 4, w // 3:w // 3 + 5] = 4
    pred.setflags(write=False); truth.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def case_d2(shape, units):
    """plane_d2 of every value of the case, computed once per (shape, units)"""
    pred, truth = case(shape)
    return [plane_d2(pred, truth, v, units) for v in VALUES]


def case_ref(shape, units, quantile_ppm):
    pred, truth = case(shape)
    return [score_plane(pred, truth, v, units, quantile_ppm, d2) for v, d2 in zip(VALUES, case_d2(shape, units))]


def tie_case(units):
    """one source voxel of A and two voxels of T, one along x and one along z, at exactly the same distance under units: dx * ux ==
    dz * uz == lcm(ux, uz) (and the mirrored pairs).  Returns (pred, truth, the common d2)"""
    ux, _, uz = units
    l = ux * uz // math.gcd(ux, uz)
    dx, dz = l // ux, l // uz
    pred, truth = np.zeros((2 * dz + 1, 3, 2 * dx + 1), np.uint8), np.zeros((2 * dz + 1, 3, 2 * dx + 1), np.uint8)
    pred[dz, 1, dx] = 1
    truth[dz, 1, 0] = 1                                         # (dx, 0, 0) away
    truth[0, 1, dx] = 1                                         # (0, 0, dz) away
    return pred, truth, l * l


def mirrors(pred, truth):
    """the pair flipped along every subset of its axes"""
    for axes in itertools.chain.from_iterable(itertools.combinations(range(3), k) for k in range(1, 4)):
        yield axes, np.ascontiguousarray(np.flip(pred, axes)), np.ascontiguousarray(np.flip(truth, axes))


def wide_row_case():
    """1 x 2 x 8192, two short runs far apart: the largest row the stage takes"""
    pred, truth = np.zeros((1, 2, 8192), np.uint8), np.zeros((1, 2, 8192), np.uint8)
    pred[0, 0, 3:9] = 1
    truth[0, 1, 8180:8190] = 1
    return pred, truth


def permuted(pred, truth, units, perm):
    """the pair with its axes permuted (new axis i = old axis perm[i]) and the units (ux, uy, uz) along with them"""
    zyx = (units[2], units[1], units[0])
    nz, ny, nx = (zyx[perm[i]] for i in range(3))
    return np.ascontiguousarray(pred.transpose(perm)), np.ascontiguousarray(truth.transpose(perm)), (nx, ny, nz)


# ---- non-degeneracy, on the reference alone ----------------------------------------------------------------------------------------------
def _minimisers(ps, pd, units):
    """bool [len(ps), len(pd)] in chunks: which targets attain the minimum of each source"""
    starts, step = _chunks(ps, pd)
    for i in starts:
        d = pair_d2(ps[i:i + step], pd, units)
        yield i, d == d.min(1, keepdims=True)


@functools.lru_cache(maxsize=None)
def degeneracy(shape):
    """over the three noise values and both directions of the case -- of the two large shapes only direction a_to_t of value 1, which
    passes the bars by far: (source voxels whose every nearest target voxel
    under (1, 1, 1) lies in another slice, and per other unit triple the source voxels none of whose nearest target voxels is one under
    (1, 1, 1))"""
    pred, truth = case(shape)
    other_slice, moved = 0, {u: 0 for u in UNITS[1:]}
    small = pred.size < 5000
    for v in VALUES[:3 if small else 1]:
        ba, bt = boundary(pred == v), boundary(truth == v)
        for src, dst in ((ba, bt), (bt, ba))[:2 if small else 1]:
            ps, pd = np.argwhere(src).astype(np.int64), np.argwhere(dst).astype(np.int64)
            base = {}
            for i, m in _minimisers(ps, pd, UNITS[0]):
                base[i] = m
                same = ps[i:i + len(m), None, 0] == pd[None, :, 0]
                other_slice += int((~(m & same).any(1)).sum())
            for u in UNITS[1:]:
                for i, m in _minimisers(ps, pd, u):
                    moved[u] += int((~(m & base[i]).any(1)).sum())
    return other_slice, moved


def assert_not_degenerate():
    """The conditions the cases must meet before any implementation is asked.  Every multi-slice case: at least 10 source voxels have
    their nearest target voxel in another slice.  Under (2, 2, 5) and under (3, 1, 7), wherever the units of the axes longer than 1
    differ (on one slice (2, 2, 5) is the isotropic metric): at least 10 source voxels have a nearest target voxel that is not one
    under (1, 1, 1).  Value 4 is absent from pred and present in
    truth; the other three are present on both sides.  The tie cases hold an exact tie between the x and the z axis."""
    for shape in SHAPES:
        pred, truth = case(shape)
        assert not (pred == 4).any() and (truth == 4).any(), shape
        assert all((pred == v).any() and (truth == v).any() for v in VALUES[:3]), shape
        other_slice, moved = degeneracy(shape)
        if shape[0] > 1:
            assert other_slice >= 10, (shape, other_slice)
        for u, c in moved.items():
            if len({uu for uu, n in zip((u[2], u[1], u[0]), shape) if n > 1}) > 1:
                assert c >= 10, (shape, u, c)
    for units in UNITS:
        pred, truth, d2 = tie_case(units)
        ps, pd = np.argwhere(pred == 1).astype(np.int64), np.argwhere(truth == 1).astype(np.int64)
        d = pair_d2(ps, pd, units)
        assert d.shape == (1, 2) and d[0, 0] == d[0, 1] == d2, (units, d)
        assert pd[0, 0] != pd[1, 0] and pd[0, 2] != pd[1, 2]           # one differs from the source along z only, the other along x only
