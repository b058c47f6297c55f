"""Reference of the volume matching (include/mi_unet.h: mi_unet_volume_match) in numpy.  It shares no code with the
product: the contingency table is np.unique over a * (mt + 1) + b with counts, the assignment is pure Python over fractions.Fraction
and the scores are plain Python floats.  Also the inputs and cases the CPU and the GPU tests share."""
import functools
from fractions import Fraction

import numpy as np

import volume_ref as vr

SIDE_FIELDS = ("voxels", "covered", "partners", "best", "best_voxels")
PAIR_FIELDS = ("p", "t", "voxels")
MAX_TABLE = 4096
GROUPS = 4                                  # distinct keys of a 64-voxel segment the device form reduces across the wave (volume_match.hip)
CAP = 1 << 16                               # the pair list of a case that does not test the cap
THRESHOLDS = ((1, 2), (1, 4), (1, 1), (1, 65536))


def classes(ids, m):
    ids = np.asarray(ids).astype(np.int64)
    return np.where((ids >= 1) & (ids <= m), ids, 0)


def table(pred, truth, mp, mt):
    """N int64 [mp + 1][mt + 1] with N[0][0] = 0"""
    keys, counts = np.unique(classes(pred, mp) * (mt + 1) + classes(truth, mt), return_counts=True)
    n = np.zeros((mp + 1) * (mt + 1), np.int64)
    n[keys] = counts
    n[0] = 0
    return n.reshape(mp + 1, mt + 1)


def sides(n):
    """the entries of the components along the rows of n, as a dict of int64 arrays"""
    inner = n[1:, 1:]
    voxels = n[1:].sum(axis=1)
    partners = (inner > 0).sum(axis=1)
    return dict(voxels=voxels, covered=voxels - n[1:, 0], partners=partners, best=np.where(partners > 0, inner.argmax(axis=1) + 1, 0),
                best_voxels=inner.max(axis=1))


def match(pred, truth, mp, mt):
    """dict(pred_side, truth_side: dicts over SIDE_FIELDS; pairs: int64 [found][3] in (p, t) order; found)"""
    n = table(pred, truth, mp, mt)
    p, t = np.nonzero(n[1:, 1:])                                # row-major: p ascending, then t
    pairs = np.stack([p, t, n[1:, 1:][p, t]], axis=1).astype(np.int64)
    return dict(pred_side=sides(n), truth_side=sides(n.T), pairs=pairs, found=len(pairs))


def assert_equal(got, want, cap, what=""):
    """(pred_side, truth_side, pairs, found) of the binding against match(): every field, the order of the pairs, the all-zero tail"""
    ps, ts, pairs, found = got
    for side, ref, name in ((ps, want["pred_side"], "pred"), (ts, want["truth_side"], "truth")):
        assert side.shape == ref["voxels"].shape, (what, name, side.shape)
        for f in SIDE_FIELDS:
            bad = np.flatnonzero(side[f].astype(np.int64) != ref[f])
            assert bad.size == 0, (what, name, f, bad[:5].tolist(), side[f][bad[:5]].tolist(), ref[f][bad[:5]].tolist())
    assert found == want["found"], (what, found, want["found"])
    assert pairs.shape == (cap,), (what, pairs.shape)
    n = min(found, cap)
    flat = np.stack([pairs[f] for f in PAIR_FIELDS], axis=1).astype(np.int64)
    assert np.array_equal(flat[:n], want["pairs"][:n]), (what, "pairs")
    assert not flat[n:].any(), (what, "the tail behind the pairs is not all-zero")


def assign(ref, num, den):
    """the greedy one-to-one assignment over exact fractions -> (match_of_pred, match_of_truth, dict(tp, fp, fn), candidates in order)"""
    vp, vt = ref["pred_side"]["voxels"], ref["truth_side"]["voxels"]
    cands = []
    for p, t, i in ref["pairs"].tolist():
        iou = Fraction(i, int(vp[p]) + int(vt[t]) - i)
        if iou >= Fraction(num, den):
            cands.append((iou, p, t))
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    of_p, of_t = [0] * len(vp), [0] * len(vt)
    for _, p, t in cands:
        if not of_p[p] and not of_t[t]:
            of_p[p], of_t[t] = t + 1, p + 1
    tp = sum(1 for v in of_p if v)
    return of_p, of_t, dict(tp=tp, fp=int((vp > 0).sum()) - tp, fn=int((vt > 0).sum()) - tp), cands


def derive(ref, of_p, counts):
    """the scores in plain Python floats, sums in pred order; NaN where a denominator is 0"""
    nan = float("nan")
    vp, vt = ref["pred_side"]["voxels"], ref["truth_side"]["voxels"]
    inter = {(p, t): i for p, t, i in ref["pairs"].tolist()}
    iou = dice = 0.0
    for p, t1 in enumerate(of_p):
        if t1:
            i, a, b = inter[(p, t1 - 1)], int(vp[p]), int(vt[t1 - 1])
            iou += i / (a + b - i)
            dice += 2.0 * i / (a + b)
    tp, fp, fn = float(counts["tp"]), float(counts["fp"]), float(counts["fn"])
    div = lambda a, b: a / b if b else nan
    sq, rq = div(iou, tp), div(tp, tp + fp / 2 + fn / 2)
    return dict(precision=div(tp, tp + fp), recall=div(tp, tp + fn), f1=div(2 * tp, 2 * tp + fp + fn), sq=sq, rq=rq, pq=sq * rq,
                mean_dice=div(dice, tp))


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
LESIONS_SHAPE, LESIONS_MP, LESIONS_MT = (6, 40, 72), 9, 7


def lesions():
    """hand-built boxes, mp = 9 and mt = 7 (a transposed table cannot pass).  Indices below are ids: index + 1.
    pred 1 / truth 1: 1 x 2 x 6 against itself moved by 2 in x: IoU 8 / 16, exactly 1/2.
    pred 2 over truth 2 and truth 3, both at 4 / 20: two pairs of one IoU, and a tie of `best`.
    truth 4 under pred 3 and pred 4, both intersections 32: a tie of the column's `best`.
    pred 5 and pred 9 overlap nothing; truth 5 overlaps nothing.
    pred 6 / truth 6 overlap over x = 60 .. 69, across x = 63 | 64.
    pred 7 is carried by no voxel.  pred 8 / truth 7 are one box (IoU 1); a second piece of pred 8 lies under truth value 8 = mt + 1,
    which is no component; pred value 10 = mp + 1 and truth value -1 lie over parts of the others' voxels."""
    pred, truth = np.zeros(LESIONS_SHAPE, np.int32), np.zeros(LESIONS_SHAPE, np.int32)
    pred[0, 0:2, 0:6] = 1
    truth[0, 0:2, 2:8] = 1
    pred[1, 0:2, 10:18] = 2
    truth[1, 0:2, 8:12] = 2
    truth[1, 0:2, 16:20] = 3
    truth[2, 4:8, 20:40] = 4
    pred[2, 4:8, 18:28] = 3
    pred[2, 4:8, 32:44] = 4
    pred[3, 10:12, 0:5] = 5
    truth[3, 20:22, 0:5] = 5
    pred[4, 30:33, 58:70] = 6
    truth[4, 30:33, 60:72] = 6
    pred[5, 0:3, 0:3] = 8
    truth[5, 0:3, 0:3] = 7
    pred[5, 20:21, 0:4] = 9
    pred[5, 39, 2:6] = 8
    truth[5, 39, 0:4] = 8
    pred[5, 38, 60:66] = 10
    truth[5, 38, 62:68] = -1
    truth[4, 33, 58:62] = -1                                    # beside pred 6, under nothing
    pred[2, 8, 20:24] = 10                                      # beside truth 4, over nothing
    return pred, truth


@functools.lru_cache(maxsize=None)
def noise_ids(shape, value=1, connectivity=26):
    """(pred ids, truth ids, mp, mt): 7.9's numbering (by size, then by first voxel; no filter) of { smooth_noise == value } and of the
    same set moved by (0, 1, 0) without wrap-around"""
    s = vr.smooth_noise(shape) == value
    moved = np.zeros_like(s)
    moved[:, 1:, :] = s[:, :-1, :]
    sides = [vr.plane(v.astype(np.uint8), 1, connectivity, cap=MAX_TABLE) for v in (s, moved)]
    return sides[0]["ids"], sides[1]["ids"], sides[0]["found"], sides[1]["found"]


def scattered(shape, mp, mt, seed):
    """ids drawn per voxel from -1 .. m + 1: a 64-voxel segment holds far more distinct keys than the wave reduces"""
    rng = np.random.default_rng(seed)
    return rng.integers(-1, mp + 2, shape).astype(np.int32), rng.integers(-1, mt + 2, shape).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (pred ids int32 [D,H,W], truth ids, mp, mt, cap)"""
    out = {}
    lp, lt = lesions()
    out["lesions"] = (lp, lt, LESIONS_MP, LESIONS_MT, CAP)
    for si, shape in enumerate(((7, 40, 72), (16, 24, 130))):
        p, t, mp, mt = noise_ids(shape)
        out[f"noise{shape}"] = (p, t, mp, mt, CAP)
        sp, st = scattered(shape, mp, mt, 20 + si)
        out[f"scattered{shape}"] = (sp, st, mp, mt, CAP)
    out["slab"] = (np.ones((3, 24, 130), np.int32), np.ones((3, 24, 130), np.int32), 1, 1, CAP)
    p, t, _, _ = noise_ids((7, 40, 72))
    out["m1"] = ((p > 0).astype(np.int32), (t > 0).astype(np.int32) * 1, 1, 1, CAP)
    sp, st = scattered((4, 64, 64), MAX_TABLE, MAX_TABLE, 31)
    sp[3, 63, 63] = st[3, 63, 63] = MAX_TABLE                   # the table's last cell
    out["m4096"] = (sp, st, MAX_TABLE, MAX_TABLE, CAP)
    p, t, mp, mt = noise_ids((1, 40, 72))
    out["D1"] = (p, t, mp, mt, CAP)
    # volumes that end 1, 2 and 3 voxels behind a multiple of 4, and in the middle of a 64-voxel segment: 1407 voxels are more than one
    # span of the walk, 1025 end one voxel into a span, 258 two voxels into a segment
    for shape in ((3, 7, 67), (1, 1, 1025), (1, 3, 86)):
        sp, st = scattered(shape, 3, 2, 40 + shape[2])
        out[f"tail{shape}"] = (sp, st, 3, 2, CAP)
        out[f"tail_slab{shape}"] = (np.full(shape, 2, np.int32), np.full(shape, 1, np.int32), 3, 2, CAP)
    found = match(lp, lt, LESIONS_MP, LESIONS_MT)["found"]
    out["cap_short"] = (lp, lt, LESIONS_MP, LESIONS_MT, found - 4)
    out["cap_exact"] = (lp, lt, LESIONS_MP, LESIONS_MT, found)
    out["cap_long"] = (lp, lt, LESIONS_MP, LESIONS_MT, found + 13)
    return out


@functools.lru_cache(maxsize=None)
def case_ref(name):
    pred, truth, mp, mt, _ = cases()[name]
    return match(pred, truth, mp, mt)


def call(fn, name):
    """a binding entry point (Engine.volume_match or binding.volume_match_host) on the case"""
    pred, truth, mp, mt, cap = cases()[name]
    return fn(pred, truth, mp, mt, cap=cap)


def crowded_segments(pred, truth, mp, mt):
    """how many 64-voxel segments of the flat volume hold more than GROUPS distinct keys other than 0"""
    keys = (classes(pred, mp) * (mt + 1) + classes(truth, mt)).reshape(-1)
    keys = np.concatenate([keys, np.zeros(-len(keys) % 64, np.int64)]).reshape(-1, 64)
    srt = np.sort(keys, axis=1)
    distinct = (srt[:, 0] != 0).astype(np.int64) + ((srt[:, 1:] != srt[:, :-1]) & (srt[:, 1:] != 0)).sum(axis=1)
    return int((distinct > GROUPS).sum())


def assert_not_degenerate():
    """A condition, not a measurement; over the case table as a whole, on this reference alone: a pair at IoU exactly 1/2; an IoU tie
    between two candidates that share a component, decided by the index rule; a row and a column with two partners or more; an
    unmatched component on each side at the threshold 1/2; a segment with more distinct keys than the kernel reduces; found > cap."""
    half = tie = rows2 = cols2 = un_p = un_t = crowded = short = 0
    for name, (pred, truth, mp, mt, cap) in cases().items():
        ref = case_ref(name)
        vp, vt = ref["pred_side"]["voxels"], ref["truth_side"]["voxels"]
        half += sum(1 for p, t, i in ref["pairs"].tolist() if 2 * i == int(vp[p]) + int(vt[t]) - i)
        rows2 += int((ref["pred_side"]["partners"] >= 2).sum())
        cols2 += int((ref["truth_side"]["partners"] >= 2).sum())
        crowded += crowded_segments(pred, truth, mp, mt)
        short += ref["found"] > cap
        if ref["found"] <= cap:
            of_p, of_t, _, _ = assign(ref, 1, 2)
            un_p += sum(1 for r, v in enumerate(of_p) if not v and vp[r] > 0)
            un_t += sum(1 for c, v in enumerate(of_t) if not v and vt[c] > 0)
            of_p, _, _, cands = assign(ref, 1, 65536)
            for (i0, p0, t0), (i1, p1, t1) in zip(cands, cands[1:]):
                # equal IoU, one shared component, and the earlier one was accepted: the later one lost by its index alone
                tie += i0 == i1 and (p0 == p1 or t0 == t1) and of_p[p0] == t0 + 1
    assert half >= 1 and tie >= 1 and rows2 >= 1 and cols2 >= 1 and un_p >= 1 and un_t >= 1 and crowded >= 1 and short >= 1, \
        (half, tie, rows2, cols2, un_p, un_t, crowded, short)
    les = case_ref("lesions")
    assert les["pred_side"]["voxels"][6] == 0 and LESIONS_MP != LESIONS_MT          # an id that no voxel carries; no square table
    assert case_ref("slab")["pairs"].tolist() == [[0, 0, 3 * 24 * 130]]               # one key over more than 1024 consecutive voxels
    assert case_ref("m4096")["pairs"][-1].tolist()[:2] == [MAX_TABLE - 1, MAX_TABLE - 1]
