"""Reference of the scores against ground truth (include/mi_unet.h: mi_unet_score_labels) in numpy, by brute force.  It
shares no code with the product: boundaries by the neighbour rule, d2 as the integer minimum over ALL pairs of boundary pixels (by
broadcasting, in chunks), order statistics by sorting, the q16 root with math.isqrt.  Also the cases the CPU and the GPU tests share."""
import math

import numpy as np

FIELDS = ("tp", "fp", "fn", "q_d2_sym", "value", "quantile_ppm")
DIR_FIELDS = ("n", "max_d2", "q_d2", "reserved", "sum_d2", "sum_d_q16")
STRUCT_BYTES = 88


def boundary(s):
    """bool [H, W]: the pixels of s with a 4-neighbour that is not in s; outside the image is not in s"""
    p = np.pad(s.astype(bool), 1, constant_values=False)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return s.astype(bool) & ~inner


def directed_d2(src, dst):
    """int64 [n_src]: for every pixel of bool map src (raster order) the minimum squared distance to a pixel of dst (not empty)"""
    ps = np.argwhere(src).astype(np.int64)
    pd = np.argwhere(dst).astype(np.int64)
    out = np.empty(len(ps), np.int64)
    step = max(1, 4_000_000 // max(len(pd), 1))
    for i in range(0, len(ps), step):
        d = ps[i:i + step, None, :] - pd[None, :, :]
        out[i:i + step] = (d * d).sum(-1).min(1)
    return out


def order_stat(values, quantile_ppm):
    s = sorted(int(v) for v in values)
    n = len(s)
    return s[n - 1 - (n * quantile_ppm) // 1_000_000]


def q16(d2):
    return math.isqrt(int(d2) << 32)


def _direction(d2, n, have, quantile_ppm):
    if not have:
        return dict(n=n, max_d2=-1, q_d2=-1, reserved=0, sum_d2=0, sum_d_q16=0)
    return dict(n=n, max_d2=int(d2.max()), q_d2=order_stat(d2, quantile_ppm), reserved=0, sum_d2=int(d2.sum()),
                sum_d_q16=sum(q16(v) for v in d2))


def score_plane(pred, truth, value, quantile_ppm=50000):
    """one plane as a dict of the struct's fields (a_to_t, t_to_a are dicts); `d2` holds the two directions' value arrays"""
    a, t = pred == value, truth == value
    ba, bt = boundary(a), boundary(t)
    na, nt = int(ba.sum()), int(bt.sum())
    have = na > 0 and nt > 0
    da = directed_d2(ba, bt) if have else np.zeros(0, np.int64)
    dt = directed_d2(bt, ba) if have else np.zeros(0, np.int64)
    return dict(tp=int((a & t).sum()), fp=int((a & ~t).sum()), fn=int((t & ~a).sum()),
                q_d2_sym=order_stat(np.concatenate([da, dt]), quantile_ppm) if have else -1, value=int(value),
                quantile_ppm=int(quantile_ppm), a_to_t=_direction(da, na, have, quantile_ppm),
                t_to_a=_direction(dt, nt, have, quantile_ppm), d2=(da, dt))


def score_labels(pred, truth, values, quantile_ppm=50000):
    """[B][n] dicts"""
    return [[score_plane(p, t, v, quantile_ppm) for v in values] for p, t in zip(pred, truth)]


def confusion(pred, truth, classes):
    """(int64 [B, classes, classes] with row = truth and column = pred, int64 [B] pixels left out)"""
    b = pred.shape[0]
    m = np.zeros((b, classes, classes), np.int64)
    skipped = np.zeros(b, np.int64)
    for i in range(b):
        ok = (pred[i] < classes) & (truth[i] < classes)
        np.add.at(m[i], (truth[i][ok].astype(int), pred[i][ok].astype(int)), 1)
        skipped[i] = int((~ok).sum())
    return m, skipped


def assert_equal(got, ref, where=""):
    """got: SCORE_DTYPE [B, n]; ref: score_labels' dicts.  Every field, exactly."""
    assert got.shape == (len(ref), len(ref[0])), (got.shape, where)
    for b, row in enumerate(ref):
        for k, r in enumerate(row):
            g = got[b, k]
            for f in FIELDS:
                assert int(g[f]) == r[f], (where, b, k, f, int(g[f]), r[f])
            for d in ("a_to_t", "t_to_a"):
                for f in DIR_FIELDS:
                    assert int(g[d][f]) == r[d][f], (where, b, k, d, f, int(g[d][f]), r[d][f])


def derive(r):
    """the metrics of one reference dict in Python floats, by the formulas of the header"""
    tp, fp, fn = r["tp"], r["fp"], r["fn"]
    ratio = lambda num, den: 1.0 if den == 0 else num / den
    out = dict(dice=ratio(2 * tp, 2 * tp + fp + fn), iou=ratio(tp, tp + fp + fn), precision=ratio(tp, tp + fp), recall=ratio(tp, tp + fn))
    a, t = r["a_to_t"], r["t_to_a"]
    if a["max_d2"] < 0:
        out.update(hd=math.nan, hd_q=math.nan, assd=math.nan, rmsd=math.nan)
    else:
        cnt = a["n"] + t["n"]
        out.update(hd=math.sqrt(max(a["max_d2"], t["max_d2"])), hd_q=math.sqrt(r["q_d2_sym"]),
                   assd=(a["sum_d_q16"] + t["sum_d_q16"]) / 65536.0 / cnt, rmsd=math.sqrt((a["sum_d2"] + t["sum_d2"]) / cnt))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def shifted_pair(maps, dy=3, dx=-2):
    """truth = the maps; pred = every class of them eroded by the 4-neighbour cross (what it loses becomes class 0), then shifted by
    (dy, dx) with class 0 moving in.  Every class keeps most of its overlap while both boundaries move."""
    pred = np.zeros_like(maps)
    for i, m in enumerate(maps):
        e = np.zeros_like(m)
        for c in np.unique(m):
            if c:
                s = m == c
                e[s & ~boundary(s)] = c
        h, w = m.shape
        sh = np.zeros_like(m)
        ys, xs = slice(max(dy, 0), h + min(dy, 0)), slice(max(dx, 0), w + min(dx, 0))
        yt, xt = slice(max(-dy, 0), h + min(-dy, 0)), slice(max(-dx, 0), w + min(-dx, 0))
        sh[ys, xs] = e[yt, xt]
        pred[i] = sh
    return pred, maps.copy()


def far_case():
    """16 x 1030, two planes: one pixel of A at (x, y) = (0, 0) against one of T at (1029, 15) -- d2 = 1029^2 + 15^2, beyond any block,
    halo or workgroup's lanes -- and a full-width stripe against a full-height one"""
    h, w = 16, 1030
    pred, truth = np.zeros((2, h, w), np.uint8), np.zeros((2, h, w), np.uint8)
    pred[0, 0, 0] = 1
    truth[0, 15, 1029] = 1
    pred[1, 7:9, :] = 1
    truth[1, :, 500:503] = 1
    return pred, truth


def edge_cases():
    """name -> (pred, truth, values): the small shapes of the issue's list, each u8 [B, H, W]"""
    rng = np.random.default_rng(11)
    cases = {}
    p = (rng.random((1, 33, 70)) < 0.5).astype(np.uint8) * 1
    p[0, 5:25, 10:50] = 1
    t = np.roll(p, (2, 3), (1, 2)).copy()
    t[0, 30:, :] = 0
    cases["odd_33x70"] = (p, t, (1,))
    far_p, far_t = far_case()
    cases["far_16x1030"] = (far_p, far_t, (1,))
    cases["far_mirrored"] = (far_p[:, ::-1, ::-1].copy(), far_t[:, ::-1, ::-1].copy(), (1,))
    line_p, line_t = np.zeros((1, 1, 200), np.uint8), np.zeros((1, 1, 200), np.uint8)
    line_p[0, 0, 10:60] = 2; line_p[0, 0, 150:] = 2
    line_t[0, 0, 20:70] = 2; line_t[0, 0, 199] = 2
    cases["row_1x200"] = (line_p, line_t, (2,))
    cases["column_200x1"] = (line_p.reshape(1, 200, 1).copy(), line_t.reshape(1, 200, 1).copy(), (2,))
    full = np.ones((1, 20, 24), np.uint8)
    inner = np.zeros((1, 20, 24), np.uint8)
    inner[0, 6:14, 5:19] = 1
    cases["whole_image"] = (full, inner, (1,))
    empty = np.zeros((1, 20, 24), np.uint8)
    cases["empty_a"] = (empty, inner, (1,))
    cases["empty_t"] = (inner, empty, (1,))
    cases["both_empty"] = (empty, empty.copy(), (1,))
    cases["equal"] = (inner, inner.copy(), (1,))
    tie_p, tie_t = np.zeros((1, 9, 15), np.uint8), np.zeros((1, 9, 15), np.uint8)
    tie_p[0, 4, 7] = 1
    tie_t[0, 4, 3] = 1; tie_t[0, 4, 11] = 1; tie_t[0, 0, 7] = 1; tie_t[0, 8, 7] = 1        # four at distance 4
    cases["ties"] = (tie_p, tie_t, (1,))
    wide_p, wide_t = np.zeros((1, 2, 20000), np.uint8), np.zeros((1, 2, 20000), np.uint8)     # a row of more than 64 KiB in the row pass
    wide_p[0, 0, 5] = 1; wide_p[0, 1, 19990:] = 1
    wide_t[0, 1, 12000:12004] = 1
    cases["wide_2x20000"] = (wide_p, wide_t, (1,))
    return cases
