"""Split-K launches of the two hipcc Winograd kernels, per layer, through the layer hook's `_splitk` suffix (include/mi_unet.h).

At batch 1 most 3x3 layers of the default network run as conv3x3_wino4_f32<NB, false, true> or conv3x3_wino_f32<WM, WN, true> over a
slice of K each, followed by wino_splitk_reduce, which owns shift, ReLU, the strided store and the pooling.  The hook hands the
launch a workspace poisoned with 0xFF bytes as the plan hands it the engine's, the launcher decides as in the plan, and the reported
kernel name says how many slices ran: `<route>+splitk<ks>`.  The case table is splitk_ref.CASES -- ragged slices, one-chunk slices,
both shrink loops, both F(4x4) kernels, both F(2x2) configurations -- whose ks and slice lengths tests/test_splitk_cpu.py proves from
the model of the launchers' arithmetic, and that model against the launchers' own functions.

Per case, every bar one the suite already has:
  1  the kernel name is `<route>+splitk<ks>` with the table's ks;
  2  dense, lower half (ldo = 2 Cout) and upper half (co_off = Cout) between 4096-byte guards: no stray store, no poison left, the
     strided results the dense result bit for bit (test_gpu_slices._run);
  3  scale, non-zero shift, ReLU against the oracle within 1e-4 max(1, max|ref|) (test_gpu_layers._tol): a shift added once per
     slice fails it;
  4  against float64, clause 3b of test_gpu_accuracy.py unchanged (rms and max at most FP32_LEVEL times those of ar.wino_fp32 on the
     same data, in the norm A^), regimes `normal` and `relu`; the yardstick sums the chunks in sequence, split-K re-associates them;
  5  exact integers, whatever the order: x in -2..2 and one weight tap per input channel -- a chunk that is dropped, doubled or read
     from the neighbouring slice changes integers;
  6  two runs give the same bytes;
  7  `_pool` on the even-sized rows: the pooled tensor is maxpool2x2 of the full one bit for bit, no poison;
and on three rows per family (even slices, ragged slices, a one-chunk slice):
  8  the exact scaling laws of test_gpu_accuracy.test_exact_scaling_laws (summing slabs commutes with powers of two);
  9  one NaN / +inf / -inf input element: C1, C2, C3 of test_gpu_special_values.py with special_ref's blast regions.
No bit-for-bit claim is made between a split-K launch and the full-K launch of the same layer: they are different instantiations."""
import numpy as np
import pytest

import accuracy_ref as ar
import oracle_lib as orc
import special_ref as sr
import splitk_ref as kr
import test_gpu_accuracy as ta
import test_gpu_slices as ts
import test_gpu_special_values as sv
from miunet import binding
from test_gpu_layers import _tol

pytestmark = pytest.mark.gpu
F32 = np.float32

CASE_IDS = [kr.case_id(c) for c in kr.CASES]


def LAYOUTS(Cout):
    """the three layouts of build_plan: dense, the lower and the upper half of a concat pixel"""
    return [("dense", {}), ("lower", {"ldo": 2 * Cout}), ("upper", {"ldo": 2 * Cout, "co_off": Cout})]


def _seed(case):
    return sum(map(ord, kr.case_id(case)))


def _row(case):
    """the case as a row of test_gpu_accuracy.py: its data, truth and run helpers then serve it unchanged"""
    return ta.Row(kr.case_id(case), kr.case_op(case), "", case.shape, case.fam, (), kr.case_kernel(case))


ROWS3 = [next(c for c in kr.CASES if c.fam == fam and c.shape == shape and c.slabs is None) for fam in (kr.F4, kr.F2) for shape in kr.ROWS3[fam]]
ROWS3_IDS = [kr.case_id(c) for c in ROWS3]


# ====================================================================================================== 1, 2, 3, 6, 7
@pytest.mark.parametrize("case", kr.CASES, ids=CASE_IDS)
def test_split_k_layer_in_every_layout(case, monkeypatch):
    B, H, W, Cin, Cout = case.shape
    op = kr.case_op(case)
    monkeypatch.setitem(ts.ROUTE, op, kr.case_kernel(case))                  # 1: what test_gpu_slices._run asserts of every run's name
    x, w, scale, shift = ts._conv_operands(B, H, W, Cin, Cout, _seed(case))
    assert (np.abs(shift) > 1e-3).sum() > Cout // 2, "the shift is there to be added exactly once"
    ref = ts._conv_ref(op, x, w, scale, shift)
    assert float((np.abs(shift) * (ref > 0)).max()) > 100 * _tol(ref), "a second shift would be seen: it moves a positive output by |shift|"
    dense = {}
    ts._run(op, x, w, scale, shift, True, LAYOUTS(Cout), ts._bar_fp32, ref, dense=dense)             # 2, 3
    again = binding.layer_debug(op, x, w, scale, shift, relu=True)                                   # 6
    assert np.array_equal(again.view(np.uint32), dense[op].view(np.uint32)), "two runs of one launch differ"
    if H % 2 == 0 and W % 2 == 0:                                                                    # 7
        lays = LAYOUTS(Cout) + [("lower+pool_ld", {"ldo": 2 * Cout, "pool_ld": Cout + 32})]
        ts._run(op + "_pool", x, w, scale, shift, True, lays, ts._bar_fp32, ref, orc.maxpool2x2(ref), dense=dense)
        pooled = dense[op + "_pool"]
        assert not np.isnan(pooled).any()
        assert np.array_equal(pooled.view(np.uint32), orc.maxpool2x2(dense[op]).view(np.uint32)), "the pooled tensor is not the pooling of the full one"


def test_a_layer_too_short_to_split_runs_the_full_k_route():
    """the hook's contract: with the workspace there and Cin below 8 chunks the name carries no suffix, and the route is right"""
    fam, shape = kr.NO_SPLIT
    B, H, W, Cin, Cout = shape
    x, w, scale, shift = ts._conv_operands(B, H, W, Cin, Cout, 64)
    ref = ts._conv_ref("conv3x3_wino4", x, w, scale, shift)
    res = binding.layer_debug_strided(kr.OP[fam] + "_splitk", x, w, scale, shift, relu=True, guard_bytes=ts.GUARD)
    assert res["kernel"].startswith("conv3x3_wino4") and "+splitk" not in res["kernel"], res["kernel"]
    got = ts._slice(res, "out", kr.OP[fam], "no split")
    assert float(np.max(np.abs(got - ref))) < _tol(ref)


def test_the_suffix_is_refused_on_every_other_op_and_outside_2_to_8():
    x = np.zeros((1, 16, 16, 128), F32)
    w = np.zeros((128, 128, 3, 3), F32)
    for op in ("conv3x3_splitk", "conv3x3_wino16_splitk", "conv3x3_wino4s_splitk", "conv3x3_wino4a_splitk3", "conv3x3_bf16_splitk",
               "conv3x3_wino4_splitk1", "conv3x3_wino_splitk9", "conv3x3_wino4_splitk_splitk"):
        with pytest.raises(binding.MiUnetError, match="layer_debug"):
            binding.layer_debug_strided(op, x, w)
    with pytest.raises(binding.MiUnetError, match="layer_debug"):
        binding.layer_debug_strided("convT2x2_splitk", x, np.zeros((128, 64, 2, 2), F32))


# ====================================================================================================== 4
@pytest.mark.parametrize("regime", ["normal", "relu"])
@pytest.mark.parametrize("case", kr.CASES, ids=CASE_IDS)
def test_error_against_float64(case, regime):
    """3b of test_gpu_accuracy.py on the split-K launch, the yardstick ar.wino_fp32 computed here.  Prints that file's line."""
    row = _row(case)
    relu = ta.REGIME_RELU[regime]
    d = ta._data(row, regime)
    t = ta._truth(row, regime, relu)
    run = ta._run(row, d, relu)                                              # (asserts the kernel name)
    assert np.isfinite(run.vals).all()
    got, ref, _ = ta._device_error(row, run, t, None, relu)
    st, ys, _ = ta._figures(row, regime, got, ref, t.norm, t.yard, t.ref)
    assert ar.meets_fp32_level(st, ys), (row.id, regime, f"3b: rms {st[0] / ys[0]:.2f} x, max {st[1] / ys[1]:.2f} x the yardstick's (at most {ar.FP32_LEVEL})")


# ====================================================================================================== 5
def _exact_operands(case):
    """x: integers in -2..2.  Input channel ci has exactly one non-zero weight, w[ci % Cout, ci, (ci % 9) // 3, ci % 3] = 576 on
    F(4x4) and 4 on F(2x2): G g G^T is then a matrix of integers (G holds 24ths and halves), so U, V, every product, every partial
    sum in any order and every step of the inverse transform are small integers."""
    B, H, W, Cin, Cout = case.shape
    r = np.random.default_rng(_seed(case))
    x = r.integers(-2, 3, (B, H, W, Cin)).astype(F32)
    w = np.zeros((Cout, Cin, 3, 3), F32)
    ci = np.arange(Cin)
    w[ci % Cout, ci, (ci % 9) // 3, ci % 3] = 576.0 if case.fam == kr.F4 else 4.0
    return x, w


@pytest.mark.parametrize("case", kr.CASES, ids=CASE_IDS)
def test_exact_integers_in_any_order(case):
    B, H, W, Cin, Cout = case.shape
    x, w = _exact_operands(case)
    ref = orc.conv3x3(x, w)
    # ---- on the CPU first: the inputs allow an exact answer (the fp32 Winograd emulation gives the oracle's bits), and no chunk of
    # any slice is idle (its channels alone give a non-zero output, so leaving it out, or adding it twice, changes integers)
    assert (np.count_nonzero(w.reshape(Cout, Cin, 9), axis=(0, 2)) == 1).all()
    emu = ar.wino_fp32(x, w, 4 if case.fam == kr.F4 else 2)
    assert np.array_equal(emu.view(np.uint32), ref.view(np.uint32)), "the data is not exact in fp32 Winograd arithmetic"
    kc = kr.CHUNK[case.fam]
    split = kr.case_split(case)
    assert split.chunks == -(-Cin // kc)
    for c in range(split.chunks):
        part = orc.conv3x3(np.ascontiguousarray(x[..., c * kc:(c + 1) * kc]), np.ascontiguousarray(w[:, c * kc:(c + 1) * kc]))
        assert np.count_nonzero(part), f"chunk {c} contributes nothing"
    # ---- the device
    run = sv.Run(kr.case_op(case), x, w)
    assert run.kernel == kr.case_kernel(case), run.kernel
    bad = run.bits != ref.view(np.uint32)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{kr.case_id(case)}: {int(bad.sum())} of {bad.size} outputs differ; first at {at}: {run.vals[at]!r}, exact {ref[at]!r} "
                             f"(slices {split.lens})")


# ====================================================================================================== 8
@pytest.mark.parametrize("case", ROWS3, ids=ROWS3_IDS)
def test_exact_scaling_laws(case, monkeypatch):
    """test_gpu_accuracy.test_exact_scaling_laws itself on the split-K row: global 2^+-20 with and without ReLU, ladder_in,
    ladder_out, shift = 0, bit for bit"""
    ta.test_exact_scaling_laws(_row(case), monkeypatch)


# ====================================================================================================== 9
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("case", ROWS3, ids=ROWS3_IDS)
def test_one_non_finite_input_element(case, relu):
    """NaN, +inf and -inf, one element per image at special_ref's three positions (first, tile seam, last; channels in the first, a
    middle and the last slice), the values rotating over images and positions.
      C1 (ReLU): no NaN, nothing negative, no set sign bit anywhere in the output -- the reduce kernel's ReLU sees the slabs' NaN.
      C2 (no ReLU): every output of the element's 3x3 footprint is non-finite: a slab's NaN or infinity survives the sum.
      C3: outside the blast region every stored bit is the clean run's."""
    B, H, W, Cin, Cout = case.shape
    op, name = kr.case_op(case), kr.case_kernel(case)
    r = np.random.default_rng(_seed(case) + int(relu))
    x = r.standard_normal((B, H, W, Cin), dtype=F32)
    w = sv._weights_no_zeros(r, (Cout, Cin, 3, 3), 9 * Cin, 0)
    shift = (0.1 * r.standard_normal(Cout)).astype(F32)
    clean = sv.Run(op, x, w, None, shift, relu=relu)
    assert clean.kernel == name and np.isfinite(clean.vals).all()
    special = [np.nan, np.inf, -np.inf]
    positions = sv._positions(H, W, Cin)
    kc, split = kr.CHUNK[case.fam], kr.case_split(case)
    owners = {next(k for k, (b, e) in enumerate(split.ranges) if b <= c // kc < e) for (_, _, c) in positions}
    assert owners >= {0, split.ks - 1}, "the first and the last slice each read one of the elements"
    for i, (y, xx, c) in enumerate(positions):
        xp = x.copy()
        for b in range(B):
            xp[b, y, xx, c] = special[(b + i) % 3]
        got = sv.Run(op, xp, w, None, shift, relu=relu)
        where = (kr.case_id(case), relu, (y, xx, c))
        assert got.kernel == name
        region = sv.BLAST[case.fam](H, W, y, xx)
        foot = sr.blast_direct(H, W, y, xx)
        assert foot.any() and not (foot & ~region).any() and not region.all()
        stray = (got.bits != clean.bits).any(axis=(0, 3)) & ~region                                    # ---- C3
        assert not stray.any(), (where, "outputs outside the blast region changed", [tuple(p) for p in np.argwhere(stray)[:6]])
        assert ((got.bits != clean.bits).any(axis=(0, 3)) & region).any()
        if relu:                                                                                      # ---- C1
            assert not np.isnan(got.vals).any(), (where, "NaN after ReLU", int(np.isnan(got.vals).sum()))
            assert not np.signbit(got.vals).any() and not (got.bits >> 31).any(), (where, "a negative value or a set sign bit after ReLU")
        else:                                                                                         # ---- C2
            inside = got.vals[:, foot]
            assert not np.isfinite(inside).any(), (where, "finite outputs inside the footprint", int(np.isfinite(inside).sum()))
