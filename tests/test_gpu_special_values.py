"""The layer kernels on values off the ordinary range: ties, fp16 subnormals, signed zeros, infinities and NaN ("Values off
the ordinary range", C1-C6).  Every comparison is bit for bit or a finite / non-finite classification; the expectations come from
special_ref.py (checked on the CPU by test_special_values_cpu.py) and from the oracle.

  a. 16-bit stores round once, to nearest even (C4): the tables of special_ref as bias alone and as operand + bias.
  b. fp16 subnormal operands are used, not flushed (C5): exact sums of multiples of 2^-24.
  c. nothing negative, no NaN and no set sign bit after ReLU (C1), which is what the 16-bit pooling kernel relies on.
  d. 16-bit pooling returns its non-negative inputs bit for bit, +inf included (C6).
  e. one non-finite input element: non-finite where it is read (C2), the clean run's bits everywhere outside its blast region (C3).

Shapes: the smallest at which test_gpu_layers.py, test_gpu_bf16.py and test_gpu_slices.py already run each route, three images.  The
hook passes no split-K workspace, so no split-K launch is involved."""
import numpy as np
import pytest

import oracle_lib as orc
import special_ref as sr
from miunet import binding

pytestmark = pytest.mark.gpu

# The hipcc F(4x4) kernels of conv_wino4.hip (two-block at Cout = 128, one-block at Cout = 64): without these switches the hook's
# routing sends both shapes to the staged kernel, which has its own entry below
HIPCC_WINO4 = {"MIUNET_WINO4_ASM": "0", "MIUNET_WINO4S": "0"}

# op, (B, H, W, Cin, Cout), region family, forms, environment, (H, W) for the _pool forms where the shape above is odd
CONV_OPS = [
    ("conv3x3", (3, 12, 40, 32, 64), "direct", ("", "_pool"), {}, None),
    ("conv3x3_wino", (3, 12, 40, 32, 64), "wino2", ("", "_pool"), {}, None),
    ("conv3x3_wino16", (3, 12, 40, 32, 64), "wino2", ("", "_pool"), {}, None),
    ("conv3x3_wino4", (3, 21, 35, 32, 128), "wino4", ("", "_pool"), HIPCC_WINO4, (22, 36)),
    ("conv3x3_wino4", (3, 21, 35, 128, 64), "wino4", ("", "_pool"), HIPCC_WINO4, (22, 36)),
    ("conv3x3_wino4s", (3, 18, 18, 16, 64), "wino4", ("", "_pool"), {}, None),
    ("conv3x3_wino4a", (3, 16, 16, 64, 128), "wino4", ("", "_pool"), {}, None),
    ("conv3x3_wino4b", (3, 16, 32, 64, 64), "wino4", ("", "_pool"), {}, None),
]
CONVT_OPS = [
    ("convT2x2", (3, 8, 32, 64, 32), "convT", ("",), {}, None),
    ("convT2x2_taps", (3, 8, 32, 64, 32), "convT", ("",), {}, None),
]
for _t in ("bf16", "fp16"):
    CONV_OPS += [
        (f"conv3x3_{_t}", (3, 10, 34, 24, 40), "direct", ("", "_lpout", "_pool", "_pool_lpout"), {}, None),
        (f"conv3x3_{_t}w", (3, 22, 46, 40, 128), "direct", ("", "_lpout", "_pool", "_pool_lpout"), {}, None),
        (f"conv3x3_{_t}r", (3, 22, 46, 64, 32), "direct", ("_lpout", "_pool_lpout"), {}, None),
        (f"conv3x3_{_t}k", (3, 9, 40, 128, 64), "direct", ("_lpout",), {}, None),
    ]
    CONVT_OPS += [
        (f"convT2x2_{_t}", (3, 8, 32, 64, 32), "convT", ("", "_lpout"), {}, None),
        (f"convT2x2_{_t}r", (3, 9, 40, 64, 32), "convT", ("_lpout",), {}, None),
    ]
FIRST_OPS = [(op, shape) for op in ("conv3x3_first", "conv3x3_first_bf16", "conv3x3_first_fp16")
             for shape in ((3, 40, 96, 3, 32), (3, 38, 70, 1, 64))]
# the route name the hook must report (the two hipcc F(4x4) kernels share one)
ROUTE = {"conv3x3": "conv3x3_mfma", "convT2x2": "convT2x2_mfma"}
BLAST = {"direct": sr.blast_direct, "wino2": sr.blast_wino2, "wino4": sr.blast_wino4, "convT": sr.blast_convT}


def _kind(op):
    return 1 if "_bf16" in op else 2 if "_fp16" in op else 0


def _rnd(kind):
    return (lambda a: np.asarray(a, np.float32), orc.bf16_round, orc.fp16_round)[kind]


class Run:
    """one hook call through the strided entry point in the dense layout: the stored bits as they are, and their values"""

    def __init__(self, op, x, w=None, scale=None, shift=None, relu=False):
        res = binding.layer_debug_strided(op, x, w, scale, shift, relu=relu)
        self.kernel = res["kernel"]
        self.es = res["elem_bytes"]
        self.kind = _kind(op) if self.es == 2 else 0
        self.bits, self.vals = self._view(res["out"], res["out_layout"])
        self.pool_bits, self.pool_vals = self._view(res["pool"], res["pool_layout"]) if res["pool"] is not None else (None, None)

    def _view(self, raw, layout):
        shape, c, ld, co_off, guard = layout
        assert ld == c and co_off == 0 and guard == 0
        bits = np.ascontiguousarray(raw).view(np.uint16 if self.es == 2 else np.uint32).reshape(*shape, c)
        return bits, bits.view(np.float32) if self.es == 4 else sr.from_bits16(self.kind, bits)


def _set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check_route(run, op):
    core = op.replace("_lpout", "").replace("_pool", "")
    assert run.kernel == ROUTE.get(core, core), (op, run.kernel)


def _ids(cases):
    return [f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in cases]


def _weights_no_zeros(r, shape, K, kind):
    w = (r.choice([-1.0, 1.0], shape) * (0.5 + r.random(shape)) / np.sqrt(K)).astype(np.float32)
    w = _rnd(kind)(w)
    assert (w != 0).all()
    return w


# ====================================================================================================== a. store rounding (C4)
LP_STORE_OPS = [(op + f, shape) for (op, shape, fam, forms, env, pool_hw) in CONV_OPS + CONVT_OPS for f in forms if f.endswith("_lpout")]


@pytest.mark.parametrize("relu", [False, True], ids=["signed", "relu"])
@pytest.mark.parametrize("op,shape", LP_STORE_OPS, ids=_ids(LP_STORE_OPS))
def test_16bit_stores_round_once_to_nearest_even(op, shape, relu):
    """Zero weights: the stored value is RNE(bias[co]), one table entry per channel, the table cycled over Cout.  Then a delta weight
    of 1.0 (the centre tap; all four taps of a transposed conv), x = p and bias = b with t = p + b exact: the MFMA sum takes part in
    the value that is rounded.  The signed table without ReLU, its non-negative half with ReLU."""
    B, H, W, Cin, Cout = shape
    kind = _kind(op)
    T = op.startswith("convT")
    src, want = sr.table(kind, signed=not relu)
    n = len(src)
    assert n <= Cin and n <= Cout
    t = sr.f32(src)
    p, b = sr.split(kind, src)
    assert (b != 0).any() and ((want & 0x7FFF) == (0x7F80 if kind == 1 else 0x7C00)).any(), "ties and overflow are in the table"
    co = np.arange(Cout) % n
    x_any = _rnd(kind)(np.random.default_rng(1).standard_normal((B, H, W, Cin), dtype=np.float32))
    x_p = np.broadcast_to(p[np.arange(Cin) % n], (B, H, W, Cin)).astype(np.float32)
    w0 = np.zeros((Cin, Cout, 2, 2) if T else (Cout, Cin, 3, 3), np.float32)
    w1 = w0.copy()
    if T:
        w1[co, np.arange(Cout)] = 1.0
    else:
        w1[np.arange(Cout), co, 1, 1] = 1.0
    for what, x, w, bias in (("bias alone", x_any, w0, t[co]), ("operand + bias", x_p, w1, b[co])):
        run = Run(op, x, w, None, bias, relu=relu)
        _check_route(run, op)
        assert run.es == 2
        for which, bits in (("full", run.bits), ("pooled", run.pool_bits)):
            if bits is None:
                continue
            bad = bits != want[co]
            if bad.any():
                at = tuple(int(i) for i in np.argwhere(bad)[0])
                entry = int(co[at[-1]])
                raise AssertionError(f"{op} {what} ({which}): {int(bad.sum())} elements differ; first at {at}: stored {int(bits[at]):04x}, "
                                     f"RNE of {int(src[entry]):08x} is {int(want[entry]):04x}")


@pytest.mark.parametrize("mfma", ["1", "0"], ids=["mfma", "valu"])
@pytest.mark.parametrize("op,shape", [c for c in FIRST_OPS if _kind(c[0])], ids=_ids([c for c in FIRST_OPS if _kind(c[0])]))
def test_first_layer_16bit_store_rounds_once_to_nearest_even(op, shape, mfma, monkeypatch):
    """The first layer reads u8 and always applies ReLU: zero weights, the non-negative table as the shift, in both of its forms."""
    monkeypatch.setenv("MIUNET_FIRST_MFMA", mfma)
    B, H, W, Cin, Cout = shape
    kind = _kind(op)
    src, want = sr.table(kind, signed=False)
    co = np.arange(Cout) % len(src)
    x = np.random.default_rng(2).integers(0, 256, (B, H, W, Cin)).astype(np.float32)
    run = Run(op, x, np.zeros((Cout, Cin, 3, 3), np.float32), None, sr.f32(src)[co], relu=True)
    assert run.es == 2 and run.kernel == "conv3x3_first"
    bad = run.bits != want[co]
    assert not bad.any(), (op, int(bad.sum()), tuple(np.argwhere(bad)[0]), hex(int(run.bits[bad][0])))


# ====================================================================================================== b. fp16 subnormal operands (C5)
SUBNORMAL_OPS = [(op, shape, forms) for (op, shape, fam, forms, env, pool_hw) in CONV_OPS + CONVT_OPS
                 if _kind(op) == 2 for forms in [tuple(f for f in forms if "_pool" not in f)]]


@pytest.mark.parametrize("which", ["activations", "weights"])
@pytest.mark.parametrize("op,shape,forms", SUBNORMAL_OPS, ids=_ids(SUBNORMAL_OPS))
def test_fp16_subnormal_operands_are_used_not_flushed(op, shape, forms, which):
    """x = m 2^-24 (m in 1..1023: every one a subnormal half) against integer weights in -3..3, then integer x in -4..4 against
    weights n 2^-24.  Every product and partial sum is an integer multiple of 2^-24 below 2^24 * 2^-24 (9 * Cin <= 1152 terms of at
    most 4 * 1023 units), so the fp32 result is exact in any summation order: the fp32 output is the oracle's bit for bit, the 16-bit
    output its rounding."""
    B, H, W, Cin, Cout = shape
    T = op.startswith("convT")
    r = np.random.default_rng(Cin + Cout + (which == "weights"))
    q = np.float32(2.0 ** -24)
    wshape = (Cin, Cout, 2, 2) if T else (Cout, Cin, 3, 3)
    if which == "activations":
        x = r.integers(1, 1024, (B, H, W, Cin)).astype(np.float32) * q
        w = r.integers(-3, 4, wshape).astype(np.float32)
        sub = x
    else:
        x = r.integers(-4, 5, (B, H, W, Cin)).astype(np.float32)
        w = r.integers(1, 1024, wshape).astype(np.float32) * q
        sub = w
    assert np.mean((sub != 0) & (np.abs(sub) < 2.0 ** -14)) >= 0.5, "at least half of the operands are subnormal halves"
    assert np.array_equal(orc.fp16_round(x), x) and np.array_equal(orc.fp16_round(w), w)
    assert 9 * Cin * 4 * 1023 < 2 ** 24
    ref = orc.convT2x2(x, w, np.zeros(Cout, np.float32)) if T else orc.conv3x3(x, w)
    assert np.count_nonzero(ref) > ref.size // 2
    for f in forms:
        got = binding.layer_debug(op + f, x, w)
        want = orc.fp16_round(ref) if f == "_lpout" else ref
        assert np.count_nonzero(got) > 0, f"{op + f}: every output is zero -- subnormal {which} were flushed"
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (op + f, which, int(bad.sum()), tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(want[bad][0]))


# ====================================================================================================== c. sign after ReLU (C1)
def _relu_data(r, op, shape):
    """Pre-activations with exact zeros of both signs and tiny negatives.  Images: all -0.0; negative integers; ordinary numbers
    mixed with -0.0 and -2^-30.  Output channels in groups of six: zero weights with bias +0, -0, -2^-30 and (bf16: -2^-140, which a
    store that rounded before it clamped would make -0) a second tiny negative; a delta weight of 1.0 that passes x through; ordinary
    weights and bias."""
    B, H, W, Cin, Cout = shape
    kind, T, first = _kind(op), op.startswith("convT"), "first" in op
    if first:
        x = r.integers(0, 256, (B, H, W, Cin)).astype(np.float32)
        x[0] = 0.0
    else:
        x = np.empty((B, H, W, Cin), np.float32)
        x[0] = -0.0
        x[1] = -r.integers(1, 5, (H, W, Cin)).astype(np.float32)
        x[2] = _rnd(kind)(r.standard_normal((H, W, Cin), dtype=np.float32))
        x[2][r.random((H, W, Cin)) < 0.2] = -0.0
        x[2][r.random((H, W, Cin)) < 0.1] = -2.0 ** -30
    K = (1 if T else 9) * Cin
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    g = np.arange(Cout) % 6
    w[g < 5] = 0.0
    d = np.flatnonzero(g == 4)
    w[d, d % Cin, 1, 1] = 1.0
    tiny = -2.0 ** -140 if kind == 1 else -2.0 ** -40
    for grp, v in ((0, 0.0), (1, -0.0), (2, -2.0 ** -30), (3, tiny), (4, 0.0)):
        bias[g == grp] = v
    if T:                                                     # [Cin][Cout][2][2]: the same value on all four taps
        w = np.ascontiguousarray(np.broadcast_to(w[:, :, 1, 1].T[:, :, None, None], (Cin, Cout, 2, 2)))
    return x, w, bias


RELU_OPS = ([(op + f, shape, env, pool_hw) for (op, shape, fam, forms, env, pool_hw) in CONV_OPS for f in forms] +
            [(op + f, shape, env, None) for (op, shape, fam, forms, env, pool_hw) in CONVT_OPS for f in forms if op != "convT2x2_taps"] +
            [(op, shape, {}, None) for (op, shape) in FIRST_OPS])


@pytest.mark.parametrize("op,shape,env,pool_hw", RELU_OPS, ids=_ids(RELU_OPS))
def test_relu_outputs_are_never_negative_never_nan_and_carry_no_sign_bit(op, shape, env, pool_hw, monkeypatch):
    """C1.  (convT2x2_taps is left out: the per-tap transposed conv has no ReLU -- no plan asks a transposed conv for one.)"""
    _set_env(monkeypatch, env)
    if "_pool" in op and pool_hw:
        shape = (shape[0],) + pool_hw + shape[3:]
    r = np.random.default_rng(sum(shape))
    x, w, bias = _relu_data(r, op, shape)
    assert (np.signbit(x).any() or "first" in op) and np.signbit(bias).any() and (bias == 0).any() and (w == 0).any() and (w == 1).any()
    run = Run(op, x, w, None, bias, relu=True)
    if "first" not in op:
        _check_route(run, op)
    for which, vals, bits in (("full", run.vals, run.bits), ("pooled", run.pool_vals, run.pool_bits)):
        if vals is None:
            continue
        assert not np.isnan(vals).any(), (op, which, "NaN")
        neg = np.signbit(vals)
        assert not neg.any(), (op, which, int(neg.sum()), tuple(np.argwhere(neg)[0]), float(vals[neg][0]))
        top = bits >> (15 if run.es == 2 else 31)
        assert not top.any(), (op, which, "a stored sign bit", tuple(np.argwhere(top)[0]))
        assert (vals == 0).any() and (vals > 0).any()
    if run.pool_vals is not None:
        want = orc.maxpool2x2(run.vals)
        assert np.array_equal(run.pool_vals.view(np.uint32), want.view(np.uint32)), f"{op}: the pooled tensor is not the oracle's pooling of the full one"


# ====================================================================================================== d. 16-bit pooling (C6)
@pytest.mark.parametrize("op", ["maxpool_bf16", "maxpool_fp16"])
def test_16bit_pooling_returns_every_non_negative_pattern_bit_for_bit(op):
    """Every pattern from 0x0000 to +inf once as the largest of its window, at a position that cycles through the window, next to
    three smaller patterns (the one below it, half of it, zero)."""
    kind = _kind(op)
    top = 0x7F80 if kind == 1 else 0x7C00
    C, Wo = 64, 32
    Ho = -(-(top + 1) // (C * Wo))
    pat = np.zeros(Ho * Wo * C, np.uint16)
    pat[:top + 1] = np.arange(top + 1, dtype=np.uint16)
    pat = pat.reshape(1, Ho, Wo, C)
    win = np.zeros((1, Ho, 2, Wo, 2, C), np.uint16)
    slot = (np.arange(pat.size).reshape(pat.shape) % 4)
    lower = [np.maximum(pat, 1) - np.uint16(1), pat >> np.uint16(1), np.zeros_like(pat)]
    for s in range(4):
        others = iter(lower)
        for k in range(4):
            dy, dx = divmod(k, 2)
            v = pat if k == s else next(others)
            win[:, :, dy, :, dx, :] = np.where(slot == s, v, win[:, :, dy, :, dx, :])
    x_bits = win.reshape(1, 2 * Ho, 2 * Wo, C)
    assert np.array_equal(x_bits.reshape(1, Ho, 2, Wo, 2, C).max(axis=(2, 4)), pat) and len(np.unique(pat)) == top + 1
    x = sr.from_bits16(kind, x_bits)
    assert np.isinf(x).sum() == 1 and not np.isnan(x).any() and not np.signbit(x).any()
    run = Run(op, x)
    assert run.es == 2 and run.kernel == "maxpool2x2"
    bad = run.bits != pat
    assert not bad.any(), (op, int(bad.sum()), hex(int(run.bits[bad][0])), hex(int(pat[bad][0])))


@pytest.mark.parametrize("op", ["maxpool", "maxpool_bf16", "maxpool_fp16"])
def test_pooling_passes_plus_infinity(op):
    r = np.random.default_rng(7)
    x = _rnd(_kind(op))(np.abs(r.standard_normal((3, 6, 10, 16), dtype=np.float32)))
    x[0, 0, 0, 0] = x[1, 3, 5, 7] = x[2, 5, 9, 15] = x[2, 4, 8, 15] = np.inf
    got = binding.layer_debug(op, x)
    want = orc.maxpool2x2(x)
    assert np.isinf(want).sum() == 3
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ====================================================================================================== e. one non-finite element (C2, C3)
def _positions(H, W, Cin):
    """pixel (0, 0) channel 0; the pixel on a tile seam nearest the image centre (the kernels' tiles are 8 or 16 rows by 16 or 32
    columns from the origin: the last pixel before such a seam); the last pixel, last channel"""
    ys = 15 if H > 16 else 7 if H > 8 else H // 2
    xs = 31 if W > 32 else 15 if W > 16 else W // 2
    return [(0, 0, 0), (ys, xs, Cin // 2), (H - 1, W - 1, Cin - 1)]


# (the per-tap transposed conv has no ReLU -- no plan asks a transposed conv for one -- so it runs without)
POISON_OPS = [(op + f, shape, fam, env, pool_hw, relu) for (op, shape, fam, forms, env, pool_hw) in CONV_OPS + CONVT_OPS for f in forms
              for relu in (False, True) if not (relu and op == "convT2x2_taps")]


@pytest.mark.parametrize("op,shape,fam,env,pool_hw,relu", POISON_OPS, ids=[i + ("-relu" if c[5] else "-linear") for i, c in zip(_ids(POISON_OPS), POISON_OPS)])
def test_one_non_finite_input_element(op, shape, fam, env, pool_hw, relu, monkeypatch):
    """Images 0, 1, 2 carry NaN, +inf, -inf at the same pixel and channel; ordinary data elsewhere, weights without zeros, so every
    output of the footprint reads the element exactly once through a non-zero weight.
      C3: outside the blast region (and its pooled image) every stored bit is the clean run's.
      C2, no ReLU: every output of the footprint is non-finite; on the non-Winograd routes images 1 and 2 hold the oracle's infinities.
      ReLU, non-Winograd routes: the footprint is the oracle's (orc.bn_relu of the oracle's conv: +0 or +inf), and the pooled tensor is
      the oracle's pooling of the full one.  ReLU inside a Winograd blast region: nothing is promised."""
    _set_env(monkeypatch, env)
    if "_pool" in op and pool_hw:
        shape = (shape[0],) + pool_hw + shape[3:]
    B, H, W, Cin, Cout = shape
    kind, T = _kind(op), op.startswith("convT")
    r = np.random.default_rng(sum(shape) + len(op))
    x = _rnd(kind)(r.standard_normal((B, H, W, Cin), dtype=np.float32))
    w = _weights_no_zeros(r, (Cin, Cout, 2, 2) if T else (Cout, Cin, 3, 3), (1 if T else 9) * Cin, kind)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    clean = Run(op, x, w, None, shift, relu=relu)
    _check_route(clean, op)
    assert np.isfinite(clean.vals).all()
    if clean.pool_vals is not None:
        assert np.array_equal(clean.pool_vals.view(np.uint32), orc.maxpool2x2(clean.vals).view(np.uint32))
    one, zero = np.ones(Cout, np.float32), np.zeros(Cout, np.float32)
    for (y, xx, c) in _positions(H, W, Cin):
        xp = x.copy()
        xp[:, y, xx, c] = [np.nan, np.inf, -np.inf]
        got = Run(op, xp, w, None, shift, relu=relu)
        where = (op, relu, (y, xx, c))
        region = BLAST[fam](H, W, y, xx)
        foot = sr.blast_convT(H, W, y, xx) if T else sr.blast_direct(H, W, y, xx)
        assert foot.any() and not (foot & ~region).any() and not region.all()
        # ---- C3
        stray = (got.bits != clean.bits).any(axis=(0, 3)) & ~region
        assert not stray.any(), (where, "outputs outside the blast region changed", [tuple(p) for p in np.argwhere(stray)[:6]])
        if got.pool_bits is not None:
            stray = (got.pool_bits != clean.pool_bits).any(axis=(0, 3)) & ~sr.pooled(region)
            assert not stray.any(), (where, "pooled outputs outside the blast region changed", [tuple(p) for p in np.argwhere(stray)[:6]])
        # ---- inside the footprint
        inside = got.vals[:, foot]                                      # [B][pixels of the footprint][Cout]
        if fam in ("wino2", "wino4"):
            if not relu:
                assert not np.isfinite(inside).any(), (where, "finite outputs inside the footprint", int(np.isfinite(inside).sum()))
            continue
        pre = orc.convT2x2(xp, w, shift) if T else orc.conv3x3(xp, w) + shift
        pin = pre[:, foot]
        assert np.isnan(pin[0]).all() and np.isinf(pin[1:]).all() and (pin[1:] > 0).any() and (pin[1:] < 0).any()
        if not relu:
            assert not np.isfinite(inside[0]).any(), (where, "NaN became finite", inside[0][np.isfinite(inside[0])][:4])
            assert np.array_equal(inside[1:], pin[1:]), (where, "the oracle's infinities", inside[1:][inside[1:] != pin[1:]][:4])
        else:
            want = orc.bn_relu(pre, one, zero, zero, one, eps=0.0, relu=True)[:, foot]
            assert (want == 0).any() and np.isinf(want).any() and np.isin(want, [0.0, np.inf]).all()
            assert np.array_equal(inside.view(np.uint32), want.view(np.uint32)), (where, inside[inside != want][:4])
            if got.pool_vals is not None:
                assert np.array_equal(got.pool_vals.view(np.uint32), orc.maxpool2x2(got.vals).view(np.uint32)), (where, "pooled")
