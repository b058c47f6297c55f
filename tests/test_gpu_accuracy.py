"""The layer kernels on ordinary values, against float64 ("Accuracy of ordinary values"; the references, norms, yardsticks
and data regimes: tests/accuracy_ref.py, whose bars tests/test_accuracy_cpu.py shows to have teeth without a GPU).

Per route (the rows of test_gpu_special_values.py: the smallest shape at which each route already runs, three images; the per-tap
transposed conv also in its whole-batch tile shapes; the fp32 first layer) and per data regime:

  3a  the a-priori bound |got - ref| <= (K + 4) u (A + |shift|) on the direct family -- derived, holds for any correct fp32 evaluation;
  3b  rms and max of (got - ref) / norm at most 4 times those of the same family's fp32 emulation on the same data (norm: A, on the
      Winograd routes A spread over the tile);
  3c  no bias: |t| <= 6 for the per-channel mean errors against zero (accuracy_ref.bias_t): round-to-nearest has no sign;
  3d  exact scaling laws, bit for bit: a global power of two, the per-input-channel ladder, the per-output-channel ladder; the
      persistent kernels also on a capped grid, where a workgroup walks several tiles;
  3e  one pixel per image times 2^12: the normal run's bits outside its blast region, 3a (direct) or 3b (Winograd) inside.

fp32 outputs; the 16-bit routes without an fp32 form are read through their 16-bit store: got against the 16-bit rounding of the
reference, one 16-bit ulp allowed for the double rounding, and (sharper, and as derived) got inside [round16(ref - E), round16(ref + E)]
for the a-priori E: rounding is monotone.  No yardstick comes from the device.  Every case prints its figures before it asserts:
`accuracy: <row> <regime> dev rms max mean | yard rms max | ratio rms max | t <3c statistic>`, errors in units of u = 2^-24."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import accuracy_ref as ar
import persist_ref as pr
import test_gpu_special_values as sv

pytestmark = pytest.mark.gpu
F32 = np.float32

Row = namedtuple("Row", "id op form shape fam env route")


def _rows():
    rows = []
    for (op, shape, fam, forms, env, _pool_hw) in sv.CONV_OPS + sv.CONVT_OPS:
        form = "" if "" in forms else "_lpout"
        rows.append(Row(f"{op}-{'x'.join(map(str, shape))}", op, form, shape, fam, tuple(sorted(env.items())), sv.ROUTE.get(op, op)))
    taps = next(c for c in sv.CONVT_OPS if c[0] == "convT2x2_taps")
    rows.append(Row("convT2x2_taps:large-" + "x".join(map(str, taps[1])), taps[0], "", taps[1], "convT", (("MIUNET_CONVT_SMALL", "0"),), "convT2x2_taps"))
    return rows


ROWS = _rows()
FIRST_ROWS = [Row(f"{op}-{'x'.join(map(str, shape))}", op, "", shape, "direct", (), "conv3x3_first") for (op, shape) in sv.FIRST_OPS if op == "conv3x3_first"]
assert len(FIRST_ROWS) == 2 and len({r.id for r in ROWS}) == len(ROWS)


def _capped_rows():
    """one capped-grid case per persistent kernel: MIUNET_CUS=8 on the sweep's shape of fewest tiles, still more tiles than workgroups"""
    rows = []
    for kernel, ops in (("wino4a", ["conv3x3_wino4a"]), ("wino4b", ["conv3x3_wino4b"]), ("wino4_1b", ["conv3x3_wino4"]),
                        ("lpr", ["conv3x3_bf16r", "conv3x3_fp16r"]), ("lprk", ["conv3x3_bf16k", "conv3x3_fp16k"]),
                        ("convt", ["convT2x2_bf16r", "convT2x2_fp16r"])):
        shape = min((s for s, _c, _p in pr.CAPPED[kernel] if pr.nwg_of(kernel, s) > 8), key=lambda s: pr.nwg_of(kernel, s))
        env = (("MIUNET_CUS", "8"),) + ((("MIUNET_WINO4S", "0"),) if kernel == "wino4_1b" else ())
        for op in ops:
            fam = "convT" if kernel == "convt" else "wino4" if kernel.startswith("wino4") else "direct"
            rows.append(Row(f"{op}-{'x'.join(map(str, shape))}-cus8", op, "_lpout" if sv._kind(op) else "", shape, fam, env, op))
    return rows


CAPPED_ROWS = _capped_rows()


def _is_T(row):
    return row.op.startswith("convT")


def _is_first(row):
    return "first" in row.op


def _has_relu(row):
    return row.op != "convT2x2_taps"


def _K(row):
    return row.shape[3] * (1 if _is_T(row) else 9)


def _seed(row):
    return sum(map(ord, row.id))


@functools.lru_cache(maxsize=None)
def _data(row, regime):
    B, H, W, Cin, _ = row.shape
    at = [p[:2] for p in sv._positions(H, W, Cin)] if regime == "outlier" else None
    d = ar.make_data(row.shape, regime, kind=sv._kind(row.op), T=_is_T(row), first=_is_first(row), seed=_seed(row), outlier_at=at)
    for v in d.values():
        if v is not None:
            v.flags.writeable = False
    return d


def _operands(row, d):
    """what the kernel multiplies: x as given (first layer: through the table), the folded weights rounded to the route's type"""
    x = ar.first_layer_table()[d["x"].astype(np.uint8)] if _is_first(row) else d["x"]
    return x, ar.round16(sv._kind(row.op))(ar.fold(d["w"], d["scale"]))


def _yardstick(row, d, relu):
    """the fp32 emulation of the row's family on the row's data"""
    rnd = ar.round16(sv._kind(row.op)) if sv._kind(row.op) else None
    if _is_T(row):
        y = ar.convT_fp32(d["x"], d["w"], d["shift"], rnd=rnd)
        return np.maximum(y, F32(0)) if relu else y
    if _is_first(row):
        return ar.first_fp32(d["x"], d["w"], d["scale"], d["shift"])
    if row.fam == "direct":
        return ar.direct_fp32(d["x"], d["w"], d["scale"], d["shift"], relu=relu, rnd=rnd)
    return ar.wino_fp32(d["x"], d["w"], 2 if row.fam == "wino2" else 4, d["scale"], d["shift"], relu=relu)


Truth = namedtuple("Truth", "ref A norm yard")


@functools.lru_cache(maxsize=None)
def _truth(row, regime, relu):
    """float64 reference (before any 16-bit store), A, the norm of the row's family, and the yardstick's output: computed once"""
    d = _data(row, regime)
    x, wq = _operands(row, d)
    H, W = row.shape[1:3]
    if _is_T(row):
        ref, A = ar.convT2x2(x, wq, d["shift"]), ar.magnitude(x, wq, None, d["shift"], T=True)
        ref = np.maximum(ref, 0.0) if relu else ref
    else:
        ref, A = ar.conv3x3(x, wq, None, d["shift"], relu), ar.magnitude(x, wq, None, d["shift"])
    norm = ar.spread(A, row.fam, H, W) if row.fam in ("wino2", "wino4") else A
    t = Truth(ref, A, norm, _yardstick(row, d, relu))
    for a in t:
        a.flags.writeable = False
    return t


def _run(row, d, relu, **other):
    """one hook call on the case's operands; other: x, w or shift in place of the case's"""
    d = {**d, **other}
    run = sv.Run(row.op + row.form, d["x"], d["w"], d["scale"], d["shift"], relu=relu)
    assert run.kernel == row.route, (row.id, run.kernel)
    assert run.es == (2 if row.form else 4)
    return run


def _device_error(row, run, t, E, relu):
    """(got as float64 relative to what it is compared with, that reference, failures of the 16-bit interval check): fp32 outputs are
    compared with ref itself; a 16-bit store with round16(ref), one 16-bit ulp of the difference allowed"""
    got = run.vals.astype(np.float64)
    if not row.form:
        return got, t.ref, None
    kind = sv._kind(row.op)
    rnd = ar.round16(kind)
    want = rnd(t.ref.astype(F32)).astype(np.float64)
    d = got - want
    resid = np.sign(d) * np.maximum(np.abs(d) - ar.ulp16(kind, t.ref), 0.0)
    # monotone rounding: a correct fp32 value f with |f - ref| <= E stores round16(f) inside [round16(ref - E), round16(ref + E)]
    # (one fp32 ulp outwards for the float64 -> float32 step); ref is after ReLU, which is monotone too
    lo = rnd(np.maximum(np.nextafter((t.ref - E).astype(F32), F32(-np.inf)), F32(0) if relu else F32(-np.inf)))
    hi = rnd(np.nextafter((t.ref + E).astype(F32), F32(np.inf)))
    outside = (run.vals < lo) | (run.vals > hi)
    return want + resid, want, outside


def _figures(row, regime, got, ref, norm, yard, yref, sel=None):
    if sel is not None:
        got, ref, norm, yard, yref = got[sel], ref[sel], norm[sel], yard[sel], yref[sel]
    st, ys = ar.stats(got, ref, norm), ar.stats(yard, yref, norm)
    bt = ar.bias_t(got, ref, norm)
    u = ar.U
    print(f"accuracy: {row.id} {regime} dev {st[0] / u:.3f} {st[1] / u:.2f} {st[2] / u:+.4f} | yard {ys[0] / u:.3f} {ys[1] / u:.2f} | "
          f"ratio {st[0] / ys[0]:.2f} {st[1] / ys[1]:.2f} | t {bt:+.2f}")
    return st, ys, bt


REGIME_RELU = {"normal": False, "relu": True, "ladder_out": True, "ladder_in": False, "outlier": False}
ACC_CASES = [(r, g) for r in ROWS for g in ("normal", "relu", "ladder_out", "ladder_in")] + [(r, g) for r in FIRST_ROWS for g in ("normal", "ladder_out")]


# ====================================================================================================== 3a, 3b, 3c
@pytest.mark.parametrize("row,regime", ACC_CASES, ids=[f"{r.id}-{g}" for r, g in ACC_CASES])
def test_error_against_float64(row, regime, monkeypatch):
    sv._set_env(monkeypatch, dict(row.env))
    relu = _is_first(row) or (REGIME_RELU[regime] and _has_relu(row))
    d = _data(row, regime)
    t = _truth(row, regime, relu)
    run = _run(row, d, relu)
    assert np.isfinite(run.vals).all()
    E = ar.a_priori_bound(t.A, _K(row))
    got, ref, outside = _device_error(row, run, t, E, relu)
    st, ys, bt = _figures(row, regime, got, ref, t.norm, t.yard, t.ref)
    fails = []
    if row.fam in ("direct", "convT"):                                                     # ---- 3a
        over = np.abs(got - ref) > E
        if over.any():
            at = tuple(int(i) for i in np.argwhere(over)[0])
            fails.append(f"3a: {int(over.sum())} elements beyond (K + 4) u A; first at {at}: error {abs(got[at] - ref[at]):.3e}, bound {E[at]:.3e}")
        if outside is not None and outside.any():
            at = tuple(int(i) for i in np.argwhere(outside)[0])
            fails.append(f"3a: {int(outside.sum())} 16-bit stores outside [round16(ref - E), round16(ref + E)]; first at {at}: {run.vals[at]!r}, ref {t.ref[at]!r}")
    if not ar.meets_fp32_level(st, ys):                                                    # ---- 3b
        fails.append(f"3b: rms {st[0] / ys[0]:.2f} x, max {st[1] / ys[1]:.2f} x the yardstick's (at most {ar.FP32_LEVEL})")
    if not ar.meets_no_bias(bt):                                                           # ---- 3c
        fails.append(f"3c: t = {bt:+.2f} over {row.shape[4]} channels (mean {st[2] / ar.U:+.4f} u at rms {st[0] / ar.U:.3f} u)")
    assert not fails, (row.id, regime, fails)


# ====================================================================================================== 3d
def _assert_16bit_operand(kind, scaled, base, factor):
    """host side: the scaled 16-bit operand is the base operand times the power(s) of two, exactly, and every non-zero stays normal"""
    rnd = ar.round16(kind)
    assert np.array_equal(rnd(scaled), rnd(base) * factor), "rounding does not commute with this power of two for this data"
    nz = np.abs(rnd(scaled)[scaled != 0])
    assert nz.min() >= (2.0 ** -14 if kind == 2 else 2.0 ** -126) and nz.max() <= (65504.0 if kind == 2 else 3.0e38)


def _same_bits(row, got, base_vals, factor, what):
    """got: a Run whose stored bits must be those of base_vals * factor (float32 values, powers of two).  A 16-bit store is compared
    where both the base value and the expected one are zero or normal numbers of the format: below that a store rounds on another
    grid, which is outside the law."""
    want_vals = np.ascontiguousarray(base_vals * factor, F32)
    eq = got.vals.view(np.uint32) == want_vals.view(np.uint32)
    if row.form:
        kind = sv._kind(row.op)
        lo, hi = (2.0 ** -14, 65504.0) if kind == 2 else (2.0 ** -126, 3.0e38)
        inside = (want_vals == 0) | ((np.minimum(np.abs(want_vals), np.abs(base_vals)) >= lo) & (np.abs(want_vals) <= hi))
        assert inside.mean() > 0.98, (row.id, what, "too few outputs in the normal range", float(inside.mean()))
        eq |= ~inside
    else:
        assert np.isfinite(want_vals).all() and (np.abs(want_vals[want_vals != 0]) >= 2.0 ** -126).all(), (row.id, what, "the law's range")
    if not eq.all():
        at = tuple(int(i) for i in np.argwhere(~eq)[0])
        raise AssertionError(f"{row.id} {what}: {int((~eq).sum())} of {eq.size} elements differ; first at {at}: {got.vals[at]!r}, expected {want_vals[at]!r}")


@pytest.mark.parametrize("row", ROWS + CAPPED_ROWS, ids=[r.id for r in ROWS + CAPPED_ROWS])
def test_exact_scaling_laws(row, monkeypatch):
    """shift = 0 throughout.  Global: op(x 2^k, w) = op(x, w) 2^k, with and without ReLU.  ladder_in: x[ci] 2^k(ci) against
    w[ci] 2^-k(ci) gives the normal run's bits.  ladder_out: w[co] 2^k(co) gives channel co of the normal run times 2^k(co)."""
    sv._set_env(monkeypatch, dict(row.env))
    if "MIUNET_CUS" in dict(row.env):
        kernel = {"conv3x3_wino4": "wino4_1b", "conv3x3_wino4a": "wino4a", "conv3x3_wino4b": "wino4b"}.get(
            row.op, "convt" if _is_T(row) else "lprk" if row.op.endswith("k") else "lpr")
        assert pr.nwg_of(kernel, row.shape) > 8
    B, H, W, Cin, Cout = row.shape
    kind, T = sv._kind(row.op), _is_T(row)
    span, kg = (4, 4) if kind == 2 else (12, 20)
    d, li = _data(row, "normal"), _data(row, "ladder_in")
    zero = np.zeros(Cout, F32)
    wq = ar.fold(d["w"], d["scale"])
    if kind:
        kin = np.exp2(ar.cycle_exponents(Cin, span)).astype(F32)
        _assert_16bit_operand(kind, li["x"], d["x"], kin)
        _assert_16bit_operand(kind, ar.fold(li["w"], li["scale"]), wq, (1 / kin)[:, None, None, None] if T else (1 / kin)[None, :, None, None])
    relus = (False, True) if _has_relu(row) else (False,)
    for relu in relus:                                        # (the ladders below run in the last form: with ReLU where the op has one)
        base = _run(row, d, relu, shift=zero)
        assert np.isfinite(base.vals).all() and np.count_nonzero(base.vals) > base.vals.size // 3
        for k in (kg, -kg):
            s = F32(2.0 ** k)
            xs = (d["x"] * s).astype(F32)
            if kind:
                _assert_16bit_operand(kind, xs, d["x"], s)
            _same_bits(row, _run(row, d, relu, x=xs, shift=zero), base.vals, s, f"global 2^{k} relu={relu}")
    _same_bits(row, _run(row, li, relu, shift=zero), base.vals, F32(1), "ladder_in")
    p = np.exp2(ar.ladder_exponents(Cout, span)).astype(F32)
    wp = (d["w"] * (p[None, :, None, None] if T else p[:, None, None, None])).astype(F32)
    if kind:
        _assert_16bit_operand(kind, ar.fold(wp, d["scale"]), wq, p[None, :, None, None] if T else p[:, None, None, None])
    _same_bits(row, _run(row, d, relu, w=wp, shift=zero), base.vals, p, "ladder_out")


# ====================================================================================================== 3e
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_one_large_pixel_per_image(row, monkeypatch):
    """image b carries position b of the special-values test times 2^12 (the whole pixel).  Outside its blast region the stored bits
    are the normal run's (C3 with a finite value); inside, the direct routes keep 3a and the Winograd routes 3b, in the norm A^ of
    the data with the pixel in it: what a Winograd tile may lose next to a large neighbour, and nothing elsewhere."""
    sv._set_env(monkeypatch, dict(row.env))
    B, H, W, Cin, Cout = row.shape
    d0, d1 = _data(row, "normal"), _data(row, "outlier")
    at = [p[:2] for p in sv._positions(H, W, Cin)]
    assert len(at) == B and all(np.array_equal(d1["x"][b, y, x], d0["x"][b, y, x] * F32(4096)) for b, (y, x) in enumerate(at))
    assert (d1["x"] != d0["x"]).any(axis=3).sum() == B
    clean, run = _run(row, d0, False), _run(row, d1, False)
    assert np.isfinite(run.vals).all()
    region = np.stack([ar.BLAST[row.fam](H, W, y, x) for (y, x) in at])                                   # [B][Ho][Wo]
    assert region.any(axis=(1, 2)).all() and not region.all(axis=(1, 2)).any()
    stray = (run.bits != clean.bits).any(axis=3) & ~region
    assert not stray.any(), (row.id, "outputs outside the blast region changed", [tuple(p) for p in np.argwhere(stray)[:6]])
    assert ((run.bits != clean.bits).any(axis=3) & region).any()
    t = _truth(row, "outlier", False)
    E = ar.a_priori_bound(t.A, _K(row))
    got, ref, outside = _device_error(row, run, t, E, False)
    st, ys, _ = _figures(row, "outlier", got, ref, t.norm, t.yard, t.ref, sel=region)
    if row.fam in ("direct", "convT"):
        over = (np.abs(got - ref) > E)[region]
        assert not over.any(), (row.id, "3a inside the blast region", int(over.sum()))
        assert outside is None or not outside[region].any(), (row.id, "16-bit stores outside the rounded interval", int(outside[region].sum()))
    else:
        assert ar.meets_fp32_level(st, ys), (row.id, f"3b inside the blast region: rms {st[0] / ys[0]:.2f} x, max {st[1] / ys[1]:.2f} x the yardstick's")
