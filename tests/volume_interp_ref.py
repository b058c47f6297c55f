"""Reference of the volume interpolation (include/mi_unet.h: mi_unet_volume_interp) in numpy.  It shares no code with
the library: the in-plane distance is the two-pass minimum written as two broadcast minima (every row of a column, then every column of
a row -- no outward scan, no early exit), and for small slices also the minimum over all pairs of pixels, which checks the separable
form itself.  The blend is the definition's comparison in int64.  Everything is exact.

SHAPES names the stacks, UNITS the in-plane units, FACTORS the factors; case(name) is a label volume with the values 1, 2, 3 (VALUES
adds 7, which no case holds), binary(name) a 0 / 1 volume.  References are cached: the CPU and the GPU tests share them."""
import functools

import numpy as np

NONE = 2**31 - 1
BIG = 1 << 40
STAT_FIELDS = ("in_voxels", "out_voxels", "mixed", "mixed_set", "ties")
VALUES = (1, 2, 3, 7)
UNITS = ((1, 1), (2, 3), (3, 1))
FACTORS = (1, 2, 3, 5, 16)
# name -> (D, H, W).  The widths: one column, one short of a wave, a wave, one more, longer than a workgroup; one row; one and two slices
SHAPES = {"discs": (5, 40, 48), "noise": (4, 24, 70), "slabs": (8, 8, 8), "w1": (3, 9, 1), "w63": (3, 5, 63), "w64": (2, 5, 64),
          "w65": (3, 6, 65), "w300": (3, 7, 300), "h1": (3, 1, 70), "d1": (1, 12, 20), "d2": (2, 12, 20), "corner": (3, 40, 300)}
PAIRS_MAX = 16 * 24                 # slices up to this many pixels are also done by all pairs


def slices(d, k):
    return (d - 1) * k + 1


def disc(h, w, cy, cx, r):
    y, x = np.mgrid[0:h, 0:w]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def _rng(name):
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(name)) + 0x1A7E)


@functools.lru_cache(maxsize=None)
def _case(name):
    d, h, w = SHAPES[name]
    rng = _rng(name)
    vol = np.zeros((d, h, w), np.uint8)
    if name == "discs":
        # three stacks of shifted discs: radii 4 / 14 / 3 ..., centres moved by 4 - 6 pixels from slice to slice
        for v, (radii, cy, cx, sy, sx) in zip((3, 2, 1), (((6, 3, 8, 5, 2), 30, 8, -1, 6), ((3, 9, 5, 11, 4), 8, 36, 5, -4),
                                                          ((4, 14, 3, 9, 12), 14, 12, 4, 5))):
            for z in range(d):
                vol[z][disc(h, w, cy + sy * z, cx + sx * z, radii[z])] = v
    elif name == "slabs":
        # empty, all 1, empty, all 2, half 1 / half 2, all 1, a single pixel, empty: all-set and all-unset slices beside each other and beside mixed ones
        vol[1] = 1
        vol[3] = 2
        vol[4, :, :4] = 1
        vol[4, :, 4:] = 2
        vol[5] = 1
        vol[6, 3, 5] = 2
    elif name == "corner":
        # the only pixel of the other state sits in a corner: the outward search of the far pixels crosses the whole row
        vol[0] = 1
        vol[0, 0, 0] = 0
        vol[1, h - 1, w - 1] = 1
        vol[2] = rng.randint(0, 4, (h, w)) * disc(h, w, 20, 150, 17)
    else:
        vol[:] = rng.randint(0, 4, (d, h, w))
        if name == "w300":
            vol[1, :, 5:290] = 2        # a long run: distances well past a wave
    return vol


def case(name):
    return _case(name).copy()


def binary(name):
    """0 / 1: the set of value 1 and 2 of the label volume (half of a noise volume)"""
    v = _case(name)
    return ((v == 1) | (v == 2)).astype(np.uint8)


def reduced(units):
    g = int(np.gcd(units[0], units[1]))
    return units[0] // g, units[1] // g


def distance(s, units):
    """e of one slice: s bool [H, W] -> int64 [H, W], NONE where the slice is all one state.  Two broadcast minima."""
    ux, uy = reduced(units)
    h, w = s.shape
    if s.all() or not s.any():
        return np.full((h, w), NONE, np.int64)
    ys, xs = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
    dy2 = ((ys[:, None] - ys[None, :]) * uy) ** 2                          # [y][y']
    dx2 = ((xs[:, None] - xs[None, :]) * ux) ** 2                          # [x][x']
    e = np.empty((h, w), np.int64)
    for state in (False, True):
        target = s != state                                                # the pixels a pixel of `state` looks for
        col = np.where(target[None, :, :], dy2[:, :, None], BIG).min(1)    # [y][x']: nearest target of column x' seen from row y
        best = (col[:, None, :] + dx2[None, :, :]).min(2)                  # [y][x]
        e[s == state] = best[s == state]
    assert (e < NONE).all() and (e >= 1).all()
    return e


def distance_pairs(s, units):
    """the same by the minimum over all pairs of pixels"""
    ux, uy = reduced(units)
    h, w = s.shape
    y, x = [a.reshape(-1).astype(np.int64) for a in np.mgrid[0:h, 0:w]]
    d2 = ((x[:, None] - x[None, :]) * ux) ** 2 + ((y[:, None] - y[None, :]) * uy) ** 2
    f = s.reshape(-1)
    d2 = np.where(f[:, None] != f[None, :], d2, BIG).min(1)
    return np.where(d2 >= BIG, NONE, d2).reshape(h, w)


def field(sets, units):
    """e of every slice of a bool [D, H, W] stack; small slices are checked against all pairs"""
    e = np.stack([distance(s, units) for s in sets])
    if sets.shape[1] * sets.shape[2] <= PAIRS_MAX:
        assert np.array_equal(e, np.stack([distance_pairs(s, units) for s in sets]))
    return e


def blend(sets, e, k):
    """bool [D, H, W] and its e -> (bool [D', H, W], stats)"""
    d = sets.shape[0]
    out = np.zeros((slices(d, k),) + sets.shape[1:], bool)
    st = dict.fromkeys(STAT_FIELDS, 0)
    st["in_voxels"] = int(sets.sum())
    out[::k] = sets
    for i in range(d - 1):
        a, b = sets[i], sets[i + 1]
        mixed = a != b
        e_set, e_unset = np.where(a, e[i], e[i + 1]), np.where(a, e[i + 1], e[i])
        for j in range(1, k):
            w_set = np.where(a, k - j, j).astype(np.int64)
            lhs, rhs = w_set * w_set * e_set, (k - w_set) * (k - w_set) * e_unset
            out[i * k + j] = np.where(mixed, lhs >= rhs, a)
            st["mixed"] += int(mixed.sum())
            st["mixed_set"] += int((mixed & (lhs >= rhs)).sum())
            st["ties"] += int((mixed & (lhs == rhs)).sum())
    st["out_voxels"] = int(out.sum())
    return out, st


def lerp(intensity, k):
    """u16 [D, H, W] -> u16 [D', H, W]"""
    a = intensity.astype(np.int64)
    out = np.zeros((slices(a.shape[0], k),) + a.shape[1:], np.int64)
    out[::k] = a
    for j in range(1, k):
        out[j::k] = ((k - j) * a[:-1] + j * a[1:] + k // 2) // k
    return out.astype(np.uint16)


def interp(masks, values, units, k):
    """the whole stage: (out u8 [n, D', H, W], list of stats)"""
    outs, stats = [], []
    for v in values:
        sets = masks == v
        o, st = blend(sets, field(sets, units), k)
        outs.append(np.where(o, v, 0).astype(np.uint8))
        stats.append(st)
    return np.stack(outs), stats


@functools.lru_cache(maxsize=None)
def _fields(name, units, which):
    vol = _case(name) if which == "case" else binary(name)
    return tuple((vol == v, field(vol == v, units)) for v in (VALUES if which == "case" else (1,)))


@functools.lru_cache(maxsize=None)
def _ref(name, units, k, which):
    vals = VALUES if which == "case" else (1,)
    done = [blend(s, e, k) for s, e in _fields(name, units, which)]
    out = np.stack([np.where(o, v, 0).astype(np.uint8) for (o, _), v in zip(done, vals)])
    out.setflags(write=False)
    return out, [st for _, st in done]


def case_ref(name, units, k):
    return _ref(name, tuple(units), k, "case")


def binary_ref(name, units, k):
    return _ref(name, tuple(units), k, "binary")


def intensity(name):
    d, h, w = SHAPES[name]
    img = _rng(name + "/i").randint(0, 65536, (d, h, w)).astype(np.uint16)
    img.reshape(-1)[:4] = (0, 65535, 0, 65535)
    if d > 1:
        img[1].reshape(-1)[:4] = (65535, 0, 0, 65535)
    return img


def assert_equal(got_out, got_stats, ref, where=""):
    """got: (out, VINTERP_DTYPE [n]); ref: (out, stats).  Every byte and every field, exactly."""
    out, stats = ref
    assert got_out.shape == out.shape and got_out.dtype == np.uint8, where
    assert np.array_equal(got_out, out), f"{where}: {int((got_out != out).sum())} bytes differ"
    assert len(got_stats) == len(stats), where
    for k, st in enumerate(stats):
        for f in STAT_FIELDS:
            assert int(got_stats[k][f]) == st[f], f"{where}: plane {k} {f} {int(got_stats[k][f])} != {st[f]}"


def neighbour_slices(sets):
    """(an all-set slice lies next to one that is neither, an all-unset one does)"""
    kind = [2 if s.all() else 0 if not s.any() else 1 for s in sets]
    near = lambda want: any(kind[z] == want and 1 in (kind[max(z - 1, 0)], kind[min(z + 1, len(kind) - 1)]) for z in range(len(kind)))
    return near(2), near(0)


def assert_not_degenerate():
    """On the reference alone, before anything else: over the label cases and over the binary cases the stage has something to decide.
    Mixed voxels and ties exist, the mixed voxels go both ways, and all-set and all-unset slices meet slices that are neither."""
    for which in ("case", "binary"):
        mixed = mixed_set = ties = 0
        full = empty = False
        for name in SHAPES:
            for units in UNITS:
                for k in FACTORS:
                    for st in _ref(name, units, k, which)[1]:
                        mixed += st["mixed"]; mixed_set += st["mixed_set"]; ties += st["ties"]
            for s, _ in _fields(name, UNITS[0], which):
                f, e = neighbour_slices(s)
                full |= f; empty |= e
        assert mixed > 0 and ties > 0, (which, mixed, ties)
        assert 0.05 * mixed <= mixed_set <= 0.95 * mixed, (which, mixed, mixed_set)
        assert full and empty, (which, full, empty)
    # the figures the generator is known by
    out, st = binary_ref("slabs", (1, 1), 4)
    assert [int(o.sum()) for o in out[0][:9]] == [0, 0, 64, 64, 64, 64, 64, 0, 0], [int(o.sum()) for o in out[0][:9]]
