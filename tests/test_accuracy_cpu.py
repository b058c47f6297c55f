"""The bars of tests/test_gpu_accuracy.py have teeth, shown without a GPU ("Accuracy of ordinary values").

The fp32 C oracle and the fp32 emulations of accuracy_ref.py meet the bars of their family; the same emulations with operands cut
to tf32 or to two bf16 terms fail the fp32-level bar, by the stated separations; a direct sum that drops its last chunk of 16
channels fails the a-priori bound in the small channels of a per-channel ladder while the former 1e-4 * max bar lets it through; a
result stored by truncation fails the bias bar alone, and the errors of one channel are not independent, which is why that bar is a
t statistic over channels; the exact scaling laws hold bit for bit for every emulation; A^ >= A, with equality on the direct family.
Seeds are fixed, so nothing here is statistical at run time."""
import functools

import numpy as np
import pytest

import accuracy_ref as ar
import oracle_lib as orc
import special_ref as sr

SHAPE = (1, 20, 36, 64, 32)          # one 64 -> 32 conv at 20 x 36: K = 576, ragged F(4x4) tiles in neither direction, 45 of them
SHAPE_T = (1, 10, 18, 64, 32)
K = 9 * SHAPE[3]
F32 = np.float32


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


@functools.lru_cache(maxsize=None)
def _data(regime, T=False):
    return _frozen(ar.make_data(SHAPE_T if T else SHAPE, regime, T=T, seed=1, outlier_at=[(7, 15)]))


@functools.lru_cache(maxsize=None)
def _ref(regime):
    d = _data(regime)
    ref = ar.conv3x3(d["x"], d["w"], d["scale"], d["shift"])
    A = ar.magnitude(d["x"], d["w"], d["scale"], d["shift"])
    return ref, A, {"direct": A, "wino2": ar.spread(A, "wino2", *SHAPE[1:3]), "wino4": ar.spread(A, "wino4", *SHAPE[1:3])}


EMU = {
    "direct": lambda d, **kw: ar.direct_fp32(d["x"], d["w"], d["scale"], d["shift"], **kw),
    "wino2": lambda d, **kw: ar.wino_fp32(d["x"], d["w"], 2, d["scale"], d["shift"], **kw),
    "wino4": lambda d, **kw: ar.wino_fp32(d["x"], d["w"], 4, d["scale"], d["shift"], **kw),
}
CUTS = {"tf32": ar.cut_tf32, "bf16x2": ar.cut_bf16x2}


@functools.lru_cache(maxsize=None)
def _stats(fam, cut, regime="normal"):
    """statistics of one emulation (cut None: the fp32 yardstick) against float64, in its family's norm"""
    ref, _, norms = _ref(regime)
    got = EMU[fam](_data(regime), **({"rnd": CUTS[cut]} if cut else {}))
    assert got.dtype == F32
    return ar.stats(got, ref, norms[fam])


@functools.lru_cache(maxsize=None)
def _bias_t(fam, regime):
    ref, _, norms = _ref(regime)
    return ar.bias_t(EMU[fam](_data(regime)), ref, norms[fam])


# ------------------------------------------------------------------------------------------------ the references themselves
def test_float64_references_agree_with_the_literal_forms():
    """conv3x3 against special_ref's literal float64 Winograd (another algorithm, same exact value), the transposed conv and the
    pooling against the oracle's on integers (exact in float), the first layer against conv3x3 on the table's values"""
    d = _data("normal")
    x, w = d["x"][0, :9, :11, :8], d["w"][:5, :8]
    ref = ar.conv3x3(x[None], w)[0]
    for m in (2, 4):
        assert np.max(np.abs(sr.winograd_conv3x3(x, w, m) - ref)) < 1e-12
    r = np.random.default_rng(2)
    xi, wi = r.integers(-4, 5, (2, 3, 5, 8)).astype(F32), r.integers(-3, 4, (8, 12, 2, 2)).astype(F32)
    bi = r.integers(-2, 3, 12).astype(F32)
    assert np.array_equal(ar.convT2x2(xi, wi, bi), orc.convT2x2(xi, wi, bi))
    assert np.array_equal(ar.convT_fp32(xi, wi, bi), orc.convT2x2(xi, wi, bi))
    y = r.standard_normal((2, 6, 10, 4), dtype=F32)
    assert np.array_equal(ar.maxpool2x2(y), orc.maxpool2x2(y))
    img = r.integers(0, 256, (1, 6, 7, 3))
    w3 = r.standard_normal((8, 3, 3, 3), dtype=F32)
    assert np.array_equal(ar.conv3x3_first(img, w3), ar.conv3x3(orc.normalize_u8(img.astype(np.uint8)), w3, relu=True))
    assert np.array_equal(ar.first_fp32(img, w3), ar.direct_fp32(orc.normalize_u8(img.astype(np.uint8)), w3, relu=True))


def test_fold_is_the_product_in_double_rounded_once():
    d = _data("normal")
    wf = ar.fold(d["w"], d["scale"])
    exact = d["w"].astype(np.float64) * d["scale"].astype(np.float64)[:, None, None, None]
    assert wf.dtype == F32 and np.all(np.abs(wf - exact) <= 0.5 * np.spacing(np.abs(wf)).astype(np.float64))
    p = np.exp2(ar.ladder_exponents(SHAPE[4], 12)).astype(F32)
    assert np.array_equal(ar.fold(d["w"], p), d["w"] * p[:, None, None, None]), "a power of two folds exactly"


# ------------------------------------------------------------------------------------------------ what is correct passes
@pytest.mark.parametrize("regime", ["normal", "relu", "ladder_out", "ladder_in", "outlier"])
def test_the_c_oracle_meets_the_direct_bars(regime):
    d = _data(regime)
    ref, A, _ = _ref(regime)
    got = (orc.conv3x3(d["x"], ar.fold(d["w"], d["scale"])) + d["shift"]).astype(F32)
    assert np.all(np.abs(got - ref) <= ar.a_priori_bound(A, K))
    st, yard = ar.stats(got, ref, A), _stats("direct", None, regime)
    assert ar.meets_fp32_level(st, yard), (st, yard)
    assert ar.meets_no_bias(ar.bias_t(got, ref, A))


def test_the_c_oracle_meets_the_transposed_conv_bars():
    d = _data("normal", T=True)
    ref, A = ar.convT2x2(d["x"], d["w"], d["shift"]), ar.magnitude(d["x"], d["w"], None, d["shift"], T=True)
    yard = ar.stats(ar.convT_fp32(d["x"], d["w"], d["shift"]), ref, A)
    got = orc.convT2x2(d["x"], d["w"], d["shift"])
    assert np.all(np.abs(got - ref) <= ar.a_priori_bound(A, SHAPE_T[3]))
    st = ar.stats(got, ref, A)
    assert ar.meets_fp32_level(st, yard) and ar.meets_no_bias(ar.bias_t(got, ref, A)), (st, yard)
    assert ar.meets_no_bias(ar.bias_t(ar.convT_fp32(d["x"], d["w"], d["shift"]), ref, A))


@pytest.mark.parametrize("regime", ["normal", "relu", "ladder_out", "ladder_in", "outlier"])
@pytest.mark.parametrize("fam", ["direct", "wino2", "wino4"])
def test_the_fp32_emulations_meet_the_bars_of_their_family(fam, regime):
    ref, A, norms = _ref(regime)
    st = _stats(fam, None, regime)
    if fam == "direct":
        got = EMU[fam](_data(regime))
        assert np.all(np.abs(got - ref) <= ar.a_priori_bound(A, K))
    assert ar.meets_fp32_level(st, st)
    assert ar.meets_no_bias(_bias_t(fam, regime)), (fam, regime, _bias_t(fam, regime))


def _truncated(ref):
    """the exact result stored by truncation towards -inf instead of to nearest: within one ulp everywhere"""
    y = ref.astype(F32)
    return np.where(y > ref, np.nextafter(y, F32(-np.inf)), y).astype(F32)


def test_truncation_fails_the_bias_bar_alone():
    ref, A, _ = _ref("normal")
    got = _truncated(ref)
    assert np.all(np.abs(got - ref) <= ar.a_priori_bound(A, K))
    assert ar.meets_fp32_level(ar.stats(got, ref, A), _stats("direct", None))
    t = ar.bias_t(got, ref, A)
    assert t < -ar.BIAS_SIGMAS and not ar.meets_no_bias(t), t


@pytest.mark.parametrize("case", ["first", "convT_bf16"])
def test_errors_of_one_channel_are_not_independent(case):
    """Why 3c is a t statistic over channels and not the mean against rms / sqrt(elements).  The u8 first layer, and a transposed conv
    of 16-bit operands (products exact in fp32, sums with spare low bits, then a fixed bias): the sequential fp32 sum is a correct
    evaluation, lies beyond 6 of those per-element sigmas on some of four seeds, with either sign -- and meets the t bar on all."""
    beyond, signs = 0, set()
    for seed in range(4):
        if case == "first":
            shape = (3, 38, 70, 1, 64)
            d = ar.make_data(shape, "normal", first=True, seed=seed)
            xt = ar.first_layer_table()[d["x"].astype(np.uint8)]
            ref, A = ar.conv3x3(xt, d["w"], d["scale"], d["shift"]), ar.magnitude(xt, d["w"], d["scale"], d["shift"])
            got = ar.direct_fp32(xt, d["w"], d["scale"], d["shift"])
        else:
            kind = 1
            d = ar.make_data((3, 8, 32, 64, 32), "normal", kind=kind, T=True, seed=seed)
            wq = ar.round16(kind)(d["w"])
            ref, A = ar.convT2x2(d["x"], wq, d["shift"]), ar.magnitude(d["x"], wq, None, d["shift"], T=True)
            got = ar.convT_fp32(d["x"], d["w"], d["shift"], rnd=ar.round16(kind))
        st = ar.stats(got, ref, A)
        assert np.all(np.abs(got - ref) <= ar.a_priori_bound(A, 9 if case == "first" else 64))
        if ar.per_element_sigmas(st, ref.size) > ar.BIAS_SIGMAS:
            beyond += 1
            signs.add(np.sign(st[2]))
        assert ar.meets_no_bias(ar.bias_t(got, ref, A)), (case, seed, ar.bias_t(got, ref, A))
    assert beyond >= 1, "the per-element count has become right for this data: say so in DESIGN.md 4.6"
    print(f"accuracy-cpu: {case}: {beyond} of 4 seeds beyond 6 per-element sigmas, signs {sorted(signs)}")


# ------------------------------------------------------------------------------------------------ what is degraded fails
@pytest.mark.parametrize("cut", ["tf32", "bf16x2"])
@pytest.mark.parametrize("fam", ["direct", "wino4"])
def test_reduced_precision_operands_fail_the_fp32_level_bar(fam, cut):
    st, yard = _stats(fam, cut), _stats(fam, None)
    print(f"accuracy-cpu: {fam} {cut}: rms {st[0] / ar.U:.2f} u max {st[1] / ar.U:.1f} u; fp32 rms {yard[0] / ar.U:.2f} u max {yard[1] / ar.U:.1f} u; "
          f"ratio {st[0] / yard[0]:.1f} / {st[1] / yard[1]:.1f}")
    assert st[0] > ar.FP32_LEVEL * yard[0], "the rms bar lets it through"
    if fam == "wino4":
        assert st[1] > ar.FP32_LEVEL * yard[1], "the max bar lets it through"
    assert not ar.meets_fp32_level(st, yard)
    least = 6.0 if (fam, cut) == ("direct", "bf16x2") else 8.0
    assert st[0] >= least * yard[0], (fam, cut, st[0] / yard[0])
    assert ar.FP32_LEVEL * yard[0] < st[0] and ar.FP32_LEVEL > 1.0          # the bar lies between the yardstick and the degraded form


def test_the_yardsticks_are_at_fp32_level():
    """the rms of every yardstick is of the order of u in its own norm, far below the a-priori bound: what 3b adds to 3a"""
    for fam, most in (("direct", 1.0), ("wino2", 2.0), ("wino4", 4.0)):
        rms, mx, _ = _stats(fam, None)
        assert rms < most * ar.U and mx < (K + 4) * ar.U / 8, (fam, rms / ar.U, mx / ar.U)


# ------------------------------------------------------------------------------------------------ a lost chunk of channels
def test_a_dropped_chunk_fails_the_a_priori_bound_and_passes_the_former_bar():
    """a kernel that loses the last 16 input channels in its first group of output channels (a quarter of them: the small end of the
    ladder, scales 2^-12 .. 2^-6): a quarter of every sum is missing there, and the error is still below 1e-4 of the largest output"""
    d = _data("ladder_out")
    ref, A, _ = _ref("ladder_out")
    group = SHAPE[4] // 4
    assert d["scale"][:group].max() <= 2.0 ** -6 and d["scale"].max() == 2.0 ** 12
    whole = ar.direct_fp32(d["x"], d["w"], d["scale"], d["shift"])
    assert not (np.abs(whole - ref) > ar.a_priori_bound(A, K)).any()
    got = whole.copy()
    got[..., :group] = ar.direct_fp32(d["x"], d["w"], d["scale"], d["shift"], drop_last_chunk=True)[..., :group]
    err = np.abs(got - ref)
    assert np.max(err) < 1e-4 * max(1.0, float(np.abs(ref).max())), "the former max-norm bar lets it through"
    bad = err > ar.a_priori_bound(A, K)
    assert bad[..., :group].mean() > 0.99 and not bad[..., group:].any(), "the a-priori bound sees the lost terms, in the small channels only"


# ------------------------------------------------------------------------------------------------ exact scaling laws
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("fam", ["direct", "wino2", "wino4"])
def test_scaling_laws_hold_bit_for_bit_for_the_emulations(fam, relu):
    d, li = _data("normal"), _data("ladder_in")
    zero = np.zeros(SHAPE[4], F32)
    run = lambda x, w: EMU[fam]({"x": x, "w": w, "scale": d["scale"], "shift": zero}, relu=relu)      # noqa: E731
    base = run(d["x"], d["w"])
    assert np.count_nonzero(base) > base.size // 3
    for k in (20, -20):
        s = F32(2.0 ** k)
        assert np.array_equal(_bits(run(d["x"] * s, d["w"])), _bits(base * s)), ("global", k)
    assert np.array_equal(_bits(run(li["x"], li["w"])), _bits(base)), "ladder_in"
    p = np.exp2(ar.ladder_exponents(SHAPE[4], 12)).astype(F32)
    assert np.array_equal(_bits(run(d["x"], d["w"] * p[:, None, None, None])), _bits(base * p)), "ladder_out"


def test_scaling_laws_hold_for_the_transposed_conv_emulation():
    d, li = _data("normal", T=True), _data("ladder_in", T=True)
    base = ar.convT_fp32(d["x"], d["w"])
    for k in (20, -20):
        assert np.array_equal(_bits(ar.convT_fp32(d["x"] * F32(2.0 ** k), d["w"])), _bits(base * F32(2.0 ** k)))
    assert np.array_equal(_bits(ar.convT_fp32(li["x"], li["w"])), _bits(base))
    p = np.exp2(ar.ladder_exponents(SHAPE_T[4], 12)).astype(F32)
    assert np.array_equal(_bits(ar.convT_fp32(d["x"], d["w"] * p[None, :, None, None])), _bits(base * p))


@pytest.mark.parametrize("kind", [1, 2])
def test_16bit_data_scales_exactly_on_the_host(kind):
    """what the GPU test asserts about its own inputs, here for the CPU shape: rounding commutes with the ladders, nothing leaves
    the normal range of the format"""
    rnd, span = ar.round16(kind), 4 if kind == 2 else 12
    d = ar.make_data(SHAPE, "normal", kind=kind, seed=1)
    wf = ar.fold(d["w"], d["scale"])
    for k in (-span, span):
        s = F32(2.0 ** k)
        assert np.array_equal(rnd(d["x"] * s), rnd(d["x"]) * s) and np.array_equal(rnd(wf * s), rnd(wf) * s)
    lo = 2.0 ** (-14 if kind == 2 else -126)
    nz = np.abs(wf[wf != 0])
    assert nz.min() * 2.0 ** -span >= lo and np.abs(d["x"]).max() * 2.0 ** span < (65504.0 if kind == 2 else 3e38)


# ------------------------------------------------------------------------------------------------ the norms
@pytest.mark.parametrize("H,W", [(20, 36), (21, 35), (9, 10)])
def test_spread_norm_dominates_and_is_the_identity_on_the_direct_family(H, W):
    r = np.random.default_rng(H)
    A = np.abs(r.standard_normal((2, H, W, 3)))
    assert np.array_equal(ar.spread(A, "direct", H, W), A)
    AT = np.abs(r.standard_normal((2, 2 * H, 2 * W, 3)))
    assert np.array_equal(ar.spread(AT, "convT", H, W), AT)
    for fam, m in (("wino2", 2), ("wino4", 4)):
        S = ar.spread(A, fam, H, W)
        assert (S >= A).all() and (S > A).any()
        assert ar.n_tiles(fam, H, W) == -(-H // m) * -(-W // m)
        y, x = H - 1, W - 1                                   # the last, ragged tile: the maximum over what it holds of the image
        assert np.array_equal(S[:, y, x], A[:, y // m * m:, x // m * m:].max(axis=(1, 2)))
        assert np.array_equal(ar.spread(S, fam, H, W), S)


def test_stats():
    got, ref, norm = np.array([1.0, 2.0, 3.5, 9.0]), np.array([1.0, 1.0, 4.0, 0.0]), np.array([1.0, 2.0, 0.5, 0.0])
    rms, mx, mean = ar.stats(got, ref, norm)                  # e = 0, 0.5, -1 over the three elements with norm > 0
    assert mx == 1.0 and abs(mean + 1 / 6) < 1e-15 and abs(rms - np.sqrt(1.25 / 3)) < 1e-15
