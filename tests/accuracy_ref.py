"""Plain-numpy pieces for the accuracy tests of the layer kernels on ordinary values ("Accuracy of ordinary values"):
float64 references of every layer op, the magnitude maps the error bars are relative to, fp32 emulations of the three algorithm
families (the yardsticks of the bars, and their reduced-precision variants), and the error statistics.

Nothing here touches the device or the C oracle.  Tensors are NHWC; conv weights [Cout][Cin][3][3], transposed-conv weights
[Cin][Cout][2][2], as the layer hook takes them.

u = 2^-24, the unit roundoff of binary32, is the unit of every figure."""
import functools

import numpy as np

import oracle_lib as orc
import special_ref as sr

U = 2.0 ** -24
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------- operands
def fold(w, scale):
    """the BN scale folded into conv weights as the engine folds it: the product in double, one rounding to float"""
    if scale is None:
        return np.ascontiguousarray(w, F32)
    return (np.asarray(w, np.float64) * np.asarray(scale, np.float64)[:, None, None, None]).astype(F32)


def first_layer_table():
    """the engine's u8 -> fp32 table: i / 255 in float"""
    return (np.arange(256, dtype=F32) / F32(255.0)).astype(F32)


def round16(kind):
    """the rounding a route applies to its operands (and to a 16-bit store): 0 none, 1 bfloat16, 2 binary16"""
    return (lambda a: np.asarray(a, F32), orc.bf16_round, orc.fp16_round)[kind]


def ulp16(kind, v):
    """the spacing of the 16-bit format at magnitude |v| (normal range; below it the spacing of the smallest normal binade)"""
    mant, emin = ((0, 0), (7, -126), (10, -14))[kind]
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** emin)
    return np.exp2(np.floor(np.log2(a)) - mant)


def cut_tf32(a):
    """binary32 cut to 10 fraction bits, round to nearest even"""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    r = (u + np.uint32(0xFFF) + ((u >> np.uint32(13)) & np.uint32(1))) & np.uint32(0xFFFFE000)
    return r.view(F32).reshape(np.shape(a))


def cut_bf16x2(a):
    """binary32 cut to two bfloat16 terms, hi + lo (16 significant bits when the terms are adjacent)"""
    a = np.ascontiguousarray(a, F32)
    hi = orc.bf16_round(a)
    lo = orc.bf16_round(a - hi)
    return (hi + lo).astype(F32)


# ---------------------------------------------------------------------------------------------------------- float64 references
def _conv3x3_f64(x, wf):
    B, H, W, Cin = x.shape
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    wd = np.asarray(wf, np.float64)
    out = np.zeros((B, H, W, wd.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ wd[:, :, ky, kx].T
    return out


def _convT2x2_f64(x, w):
    B, H, W, Cin = x.shape
    xd, wd = np.asarray(x, np.float64), np.asarray(w, np.float64)
    out = np.zeros((B, 2 * H, 2 * W, wd.shape[1]))
    for dy in range(2):
        for dx in range(2):
            out[:, dy::2, dx::2, :] = xd @ wd[:, :, dy, dx]
    return out


def _epilogue(pre, shift, relu):
    y = pre if shift is None else pre + np.asarray(shift, np.float64)
    return np.maximum(y, 0.0) if relu else y


def conv3x3(x, w, scale=None, shift=None, relu=False):
    """float64 conv3x3 (zero padding) of the fp32 operands x and fold(w, scale), + shift, ReLU"""
    return _epilogue(_conv3x3_f64(x, fold(w, scale)), shift, relu)


def maxpool2x2(y):
    B, H, W, C = y.shape
    return y[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def convT2x2(x, w, bias=None):
    """float64 transposed 2x2 stride-2 conv: out[b, 2y + dy, 2x + dx, co] = sum_ci x[b, y, x, ci] w[ci, co, dy, dx] + bias[co]"""
    return _epilogue(_convT2x2_f64(x, w), bias, False)


def conv3x3_first(img, w, scale=None, shift=None):
    """the first layer: u8 image through the engine's fp32 table, conv3x3, ReLU (the kernel always applies it)"""
    return conv3x3(first_layer_table()[np.asarray(img).astype(np.uint8)], w, scale, shift, relu=True)


# ---------------------------------------------------------------------------------------------------------- magnitude maps
def magnitude(x, w, scale=None, shift=None, T=False):
    """A = |x| (*) |w_folded| + |shift|: what every rounding error of a direct evaluation is relative to"""
    a = _convT2x2_f64(np.abs(x), np.abs(w)) if T else _conv3x3_f64(np.abs(x), np.abs(fold(w, scale)))
    return a if shift is None else a + np.abs(np.asarray(shift, np.float64))


BLAST = {"direct": sr.blast_direct, "wino2": sr.blast_wino2, "wino4": sr.blast_wino4, "convT": sr.blast_convT}


@functools.lru_cache(maxsize=None)
def tile_labels(fam, H, W):
    """[Ho][Wo] labels: two outputs carry the same label iff they lie in the same blast regions of special_ref, i.e. share an
    F(m x m) tile on the Winograd routes; every output has its own label on the direct routes and the transposed conv (their
    regions are footprints, not tiles: no two outputs lie in the same set of them).  (H, W) is the input size."""
    masks = np.stack([BLAST[fam](H, W, y, x) for y in range(H) for x in range(W)])             # [inputs][Ho][Wo]
    Ho, Wo = masks.shape[1:]
    if fam == "convT":                                       # one input pixel per 2x2 outputs, a 1 x 1 kernel across them
        return np.arange(Ho * Wo).reshape(Ho, Wo)
    sig = masks.reshape(len(masks), -1).T                    # [outputs][inputs]
    _, lab = np.unique(sig, axis=0, return_inverse=True)
    return lab.reshape(Ho, Wo)


def n_tiles(fam, H, W):
    return int(tile_labels(fam, H, W).max()) + 1


def spread(A, fam, H, W):
    """A^ : for each output the maximum of A over the outputs that share its tile (per image and channel).  Winograd transforms mix
    the pixels of a patch, so their error is relative to this."""
    lab = tile_labels(fam, H, W).reshape(-1)
    if len(np.unique(lab)) == lab.size:
        return A.copy()
    B, Ho, Wo, C = A.shape
    flat = A.reshape(B, Ho * Wo, C)
    order = np.argsort(lab, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(lab[order]) != 0])
    tile_max = np.maximum.reduceat(flat[:, order], starts, axis=1)                              # [B][tiles][C]
    return tile_max[:, lab].reshape(A.shape)


# ---------------------------------------------------------------------------------------------------------- fp32 emulations
def _finish32(acc, shift, relu):
    y = acc if shift is None else (acc + np.asarray(shift, F32)).astype(F32)
    return np.maximum(y, F32(0)) if relu else y


def direct_fp32(x, w, scale=None, shift=None, relu=False, rnd=None, drop_last_chunk=False):
    """conv3x3 as one sequential fp32 sum per output (tap by tap, channel by channel; a rounded product, then a rounded add).
    rnd: applied to both operands first.  drop_last_chunk: the last 16 input channels are left out (a deliberately wrong kernel)."""
    x, wf = np.ascontiguousarray(x, F32), fold(w, scale)
    if rnd is not None:
        x, wf = rnd(x), rnd(wf)
    B, H, W, Cin = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros((B, H, W, wf.shape[0]), F32)
    for ky in range(3):
        for kx in range(3):
            for ci in range(Cin - 16 if drop_last_chunk else Cin):
                acc = acc + xp[:, ky:ky + H, kx:kx + W, ci, None] * wf[:, ci, ky, kx]
    assert acc.dtype == F32
    return _finish32(acc, shift, relu)


def convT_fp32(x, w, bias=None, rnd=None):
    """transposed 2x2 conv as one sequential fp32 sum over the input channels per output"""
    x, w = np.ascontiguousarray(x, F32), np.ascontiguousarray(w, F32)
    if rnd is not None:
        x, w = rnd(x), rnd(w)
    B, H, W, Cin = x.shape
    out = np.zeros((B, 2 * H, 2 * W, w.shape[1]), F32)
    for dy in range(2):
        for dx in range(2):
            acc = np.zeros((B, H, W, w.shape[1]), F32)
            for ci in range(Cin):
                acc = acc + x[..., ci, None] * w[ci, :, dy, dx]
            out[:, dy::2, dx::2] = acc
    return _finish32(out, bias, False)


def first_fp32(img, w, scale=None, shift=None):
    return direct_fp32(first_layer_table()[np.asarray(img).astype(np.uint8)], w, scale, shift, relu=True)


def _sandwich32(M, d):
    """M d M^T in fp32 for a grid d[k][l] of equally shaped arrays: sequential sums, zero coefficients skipped"""
    n = len(d)

    def comb(coefs, terms):
        acc = None
        for c, t in zip(coefs, terms):
            if c != 0:
                p = t if c == 1 else (F32(c) * t).astype(F32)
                acc = p if acc is None else (acc + p).astype(F32)
        return acc

    rows = [[comb(M[i], [d[k][l] for k in range(n)]) for l in range(n)] for i in range(len(M))]
    return [[comb(M[j], rows[i]) for j in range(len(M))] for i in range(len(M))]


def wino_fp32(x, w, m, scale=None, shift=None, relu=False, rnd=None):
    """F(m x m, 3x3), m = 2 or 4, with the textbook matrices of special_ref: U = G g G^T in double, rounded once (the engine's
    packing); V = B^T d B, the channel sum in chunks of 16 (a sequential sum per chunk, then added to the running total) and
    Y = A^T M A in fp32.  Origin-aligned tiles, zero padding.  rnd: applied to U and V, the operands of the multiply."""
    BT, G, AT = sr._WINO[m]
    x = np.ascontiguousarray(x, F32)
    B, H, W, Cin = x.shape
    n, Th, Tw = m + 2, -(-H // m), -(-W // m)
    g = np.asarray(w, np.float64) * (1.0 if scale is None else np.asarray(scale, np.float64)[:, None, None, None])
    Uw = np.einsum("ij,ocjk,lk->iloc", G, g, G).astype(F32).reshape(n * n, g.shape[0], Cin)    # [pos][Cout][Cin]
    xp = np.zeros((B, Th * m + 2, Tw * m + 2, Cin), F32)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = [[xp[:, k:k + Th * m:m, l:l + Tw * m:m, :].reshape(-1, Cin) for l in range(n)] for k in range(n)]
    V = _sandwich32(BT, d)
    Vs = np.stack([V[i][j] for i in range(n) for j in range(n)])                               # [pos][tiles][Cin]
    if rnd is not None:
        Uw, Vs = rnd(Uw), rnd(Vs)
    acc = np.zeros((n * n, Vs.shape[1], Uw.shape[1]), F32)
    for c0 in range(0, Cin, 16):
        part = np.zeros_like(acc)
        for ci in range(c0, min(c0 + 16, Cin)):
            part = part + Vs[:, :, ci, None] * Uw[:, None, :, ci]
        acc = acc + part
    assert acc.dtype == F32
    Y = _sandwich32(AT, [[acc[i * n + j] for j in range(n)] for i in range(n)])                # [m][m] of [tiles][Cout]
    out = np.zeros((B, Th * m, Tw * m, Uw.shape[1]), F32)
    for i in range(m):
        for j in range(m):
            out[:, i::m, j::m] = Y[i][j].reshape(B, Th, Tw, -1)
    return _finish32(np.ascontiguousarray(out[:, :H, :W]), shift, relu)


# ---------------------------------------------------------------------------------------------------------- statistics
def stats(got, ref, norm):
    """(rms, max, signed mean) of (got - ref) / norm over the elements where norm > 0"""
    ok = norm > 0
    e = (np.asarray(got, np.float64)[ok] - np.asarray(ref, np.float64)[ok]) / norm[ok]
    return float(np.sqrt(np.mean(e * e))), float(np.max(np.abs(e))), float(np.mean(e))


# ---------------------------------------------------------------------------------------------------------- the bars
def a_priori_bound(A, K):
    """3a: any correct fp32 evaluation of K products per output, in any order, with or without fma, lies within this of the exact
    value: (K - 1) adds and K products are at most K roundings of relative size u each on partial sums bounded by A (first order;
    the second-order term K^2 u^2 is below 1e-7 of it here), 4 more for the fold, the scale and shift operations and the store"""
    return (K + 4) * U * A


FP32_LEVEL = 4.0              # 3b: device rms and max against the same-family fp32 emulation on the same data
BIAS_SIGMAS = 6.0             # 3c: |t| <= 6, see bias_t


def meets_fp32_level(st, yard):
    return st[0] <= FP32_LEVEL * yard[0] and st[1] <= FP32_LEVEL * yard[1]


def per_element_sigmas(st, n):
    """|mean| in units of rms / sqrt(n): the mean error's distance from zero IF the n errors were independent.  They are not: the
    errors of one output channel share its weights and its shift (a sum with spare low bits plus a fixed shift rounds the same way
    at every pixel; a u8 or 16-bit operand takes few values, so product errors repeat), and a correct fp32 sum lies 10 of these
    sigmas out on the 16-bit and first-layer data (test_accuracy_cpu.py).  Kept to show that; the bar is bias_t."""
    return abs(st[2]) / (st[0] / np.sqrt(n)) if st[0] > 0 else 0.0


def bias_t(got, ref, norm):
    """3c: Student's t of the per-channel mean errors m[co] = mean over the pixels of (got - ref) / norm against zero,
    t = mean(m) / (sd(m) / sqrt(Cout)).  Channels have their own weights and shifts, so the m[co] are independent whatever the pixels
    of a channel share; with independent elements sd(m) is rms / sqrt(pixels) and t is the mean in units of rms / sqrt(N), N the
    number of elements.  Round-to-nearest gives the m[co] either sign; truncation anywhere, or a transform constant that is off,
    gives them one sign."""
    ok = norm > 0
    e = np.where(ok, (np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / np.where(ok, norm, 1.0), 0.0)
    m = e.reshape(-1, e.shape[-1]).mean(axis=0)
    sd = m.std(ddof=1)
    if sd == 0:
        return 0.0 if m[0] == 0 else float("inf")
    return float(m.mean() / (sd / np.sqrt(m.size)))


def meets_no_bias(t):
    return abs(t) <= BIAS_SIGMAS


# ---------------------------------------------------------------------------------------------------------- data regimes
REGIMES = ("normal", "relu", "ladder_out", "ladder_in", "outlier")


def ladder_exponents(n, span):
    """n exponents from -span to span, evenly spread and rounded (the per-output-channel ladder)"""
    return np.rint(-span + 2.0 * span * np.arange(n) / max(n - 1, 1)).astype(np.int64)


def cycle_exponents(n, span):
    """-span .. span, cycled over n input channels"""
    return (np.arange(n) % (2 * span + 1)) - span


def _floor_magnitude(a, lo):
    """non-zero values below lo in magnitude moved to +-lo (fp16 data: keeps every scaled operand in the normal range)"""
    small = (a != 0) & (np.abs(a) < lo)
    return np.where(small, np.copysign(F32(lo), a), a).astype(F32)


def make_data(shape, regime, kind=0, T=False, first=False, seed=0, outlier_at=None):
    """The operands of one case: dict(x, w, scale, shift).  kind: the route's operand type (0 fp32, 1 bf16, 2 fp16); activations are
    generated on the 16-bit grid, weights are rounded by the route after the fold.  The same seed gives the same base numbers in every
    regime, so `ladder_in`, `ladder_out` and `outlier` are exact images of `normal`.  first: x is a u8 image (as float32 byte
    values).  T: a transposed conv, w [Cin][Cout][2][2], no scale.  outlier_at: [(y, x)] per image for `outlier`."""
    assert regime in REGIMES
    B, H, W, Cin, Cout = shape
    r = np.random.default_rng([seed, B, H, W, Cin, Cout, kind, int(T)])
    span = 4 if kind == 2 else 12
    if first:
        x = r.integers(0, 256, (B, H, W, Cin)).astype(F32)
    else:
        x = r.standard_normal((B, H, W, Cin), dtype=F32)
        if regime == "relu":
            x = np.maximum(x + F32(0.5), F32(0))
        x = round16(kind)(x)
    if T:
        w = (r.standard_normal((Cin, Cout, 2, 2), dtype=F32) / np.sqrt(Cin)).astype(F32)
    else:
        w = (r.standard_normal((Cout, Cin, 3, 3), dtype=F32) * np.sqrt(2.0 / (9 * Cin))).astype(F32)
    scale = None if T else (1.0 + 0.1 * r.standard_normal(Cout)).astype(F32)
    shift = (0.1 * r.standard_normal(Cout)).astype(F32)
    if kind == 2:                                   # |x|, |w| >= 2^-8: times 2^-4 and a scale of 0.5 still a normal half
        x, w = _floor_magnitude(x, 2.0 ** -8), _floor_magnitude(w, 2.0 ** -8)
    if regime == "ladder_out":
        p = np.exp2(ladder_exponents(Cout, span)).astype(F32)
        shift = shift * p
        if T:
            w = (w * p[None, :, None, None]).astype(F32)
        else:
            scale = p
    elif regime == "ladder_in":
        k = cycle_exponents(Cin, span)
        x = (x * np.exp2(k).astype(F32)).astype(F32)
        w = (w * np.exp2(-k).astype(F32)[:, None, None, None]).astype(F32) if T else (w * np.exp2(-k).astype(F32)[None, :, None, None]).astype(F32)
    elif regime == "outlier":
        for b, (y, xx) in enumerate(outlier_at):
            x[b, y, xx, :] *= F32(2.0 ** 12)
    return {"x": x, "w": w, "scale": scale, "shift": shift}
