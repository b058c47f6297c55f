"""The references that tests/test_gpu_special_values.py stands on, checked without a GPU: the rounding tables of special_ref.py against
torch's CPU casts, oracle_lib's numpy rounding and the C oracle's; the exact operand/bias split of every table entry; bf16_round on
NaN; the blast-region functions against a literal Winograd and the oracle's direct conv with one poisoned element; what the oracle's
ReLU and pooling make of non-finite data; and the host's 16-bit converters (tests/cpu/lp_convert_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
import special_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd")


def _oracle_bits(kind, src_bits):
    """the table's expectation three ways: oracle_lib's numpy rounding, the C oracle's scalar rounding"""
    x = sr.f32(src_bits)
    rnd = orc.bf16_round if kind == 1 else orc.fp16_round
    c_rnd = orc.lib().orc_bf16_round if kind == 1 else orc.lib().orc_fp16_round
    with np.errstate(over="ignore"):                                              # numpy warns where 65520 becomes infinity
        a = sr.to_bits16(kind, rnd(x))
    b = sr.to_bits16(kind, np.array([c_rnd(float(v)) for v in x], np.float32))
    return a, b


# ---------------------------------------------------------------------------------------------------------- rounding tables
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("signed", [False, True])
def test_rounding_tables_agree_with_torch_and_the_oracle(kind, signed):
    src, want = sr.table(kind, signed)
    assert len(src) == (2 if signed else 1) * (7 if kind == 1 else 10)
    assert np.array_equal(sr.torch_bits(kind, src), want)
    a, b = _oracle_bits(kind, src)
    assert np.array_equal(a, want), "oracle_lib's numpy rounding"
    assert np.array_equal(b, want), "the C oracle's rounding"
    if signed:
        assert np.array_equal(src[1::2], src[0::2] | np.uint32(0x80000000)) and np.array_equal(want[1::2], want[0::2] | np.uint16(0x8000))


def test_tables_hold_the_cases_they_are_for():
    assert np.array_equal(sr.f32(sr.table(2, False)[0]).astype(np.float64), np.array(sr.FP16_TABLE_VALUES))
    for kind in (1, 2):
        src, want = sr.table(kind, False)
        x = sr.f32(src).astype(np.float64)
        back = sr.from_bits16(kind, want).astype(np.float64)
        # ties: the value lies exactly half way between two neighbours of the 16-bit grid
        p, b = sr.split(kind, src)
        up = sr.from_bits16(kind, sr.to_bits16(kind, p) + np.uint16(1)).astype(np.float64)
        down = sr.from_bits16(kind, np.maximum(sr.to_bits16(kind, p), 1) - np.uint16(1)).astype(np.float64)
        with np.errstate(invalid="ignore"):
            step = np.where(np.isinf(up), p - down, up - p)                        # above the largest finite value: the step below it
        tie = b.astype(np.float64) * 2 == step
        assert tie.sum() >= 3, "ties are present"
        assert (tie & (back > x)).any() and (tie & (back < x)).any(), "ties that go up and ties that go down"
        assert np.isinf(back).any(), "overflow to infinity is present"
        assert (back[~np.isinf(back)] != x[~np.isinf(back)]).any()
    src, want = sr.table(2, False)
    assert ((want > 0) & (want < 0x0400)).any() and (want == 0).any() and (want == 0x0400).any(), "fp16 subnormals, underflow to zero, the carry to normal"
    src, want = sr.table(1, False)
    assert (want == 0x3F80).sum() >= 2 and 0x7F7F in want


@pytest.mark.parametrize("kind", [1, 2])
def test_split_is_exact_and_its_operand_is_a_16bit_value(kind):
    src, want = sr.table(kind, True)
    p, b = sr.split(kind, src)
    t = sr.f32(src)
    assert p.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal((p + b).view(np.uint32), src), "p + b is t in fp32 arithmetic"
    assert np.array_equal(p.astype(np.float64) + b.astype(np.float64), t.astype(np.float64)), "... and exactly"
    assert np.isfinite(p).all() and np.all(np.abs(p) <= np.abs(t)) and np.all(np.signbit(p) == np.signbit(t))
    rnd = orc.bf16_round if kind == 1 else orc.fp16_round
    assert np.array_equal(rnd(p).view(np.uint32), p.view(np.uint32)), "p survives the hook's rounding of its operands"
    assert (b != 0).sum() >= len(src) // 2, "the bias takes part in most entries"
    if kind == 2:
        assert ((np.abs(p) > 0) & (np.abs(p) < 2.0 ** -14)).any(), "a subnormal fp16 operand is present"


# ---------------------------------------------------------------------------------------------------------- bf16_round
def test_bf16_round_keeps_nan_and_rounds_every_pattern_like_torch():
    import torch
    hi = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):                  # every bf16 pattern, six fillings of the dropped half
        u = hi | np.uint32(low)
        x = sr.f32(u)
        got = orc.bf16_round(x)
        nan = np.isnan(x)
        assert nan.sum() == (254 if low == 0 else 256)                             # 2 * 127 NaN patterns; with low bits set the infinities' rows too
        assert np.isnan(got[nan]).all(), "NaN stays NaN"
        assert not np.isnan(got[~nan]).any()
        assert not (got.view(np.uint32) & np.uint32(0xFFFF)).any(), "a bf16 value"
        want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
        c = np.array([orc.lib().orc_bf16_round(float(v)) for v in x[~nan][::97]], np.float32)
        assert np.array_equal(c.view(np.uint32), got[~nan][::97].view(np.uint32)), "the C oracle agrees"
    assert np.isnan(orc.bf16_round(sr.f32(np.array([0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001], np.uint32)))).all()
    assert orc.bf16_round(np.float32(1.0)).shape == () and orc.bf16_round(np.ones((2, 3), np.float32)).shape == (2, 3)


# ---------------------------------------------------------------------------------------------------------- blast regions
def _cases(H, W):
    return [(0, 0), (H - 1, W - 1), (H // 2, W // 2), (H // 2 - 1, W // 2 + 1), (1, W - 2), (H - 2, 0), (3, 4), (4, 3)]


@pytest.mark.parametrize("m,fn", [(2, sr.blast_wino2), (4, sr.blast_wino4)])
@pytest.mark.parametrize("H,W", [(8, 12), (7, 9), (5, 6)])
def test_winograd_blast_region_is_what_a_literal_winograd_poisons(m, fn, H, W):
    """origin-aligned tiles, as the kernels cut them (conv_wino.hip, conv_wino4.hip, conv_wino4s.hip and the assembly generators all
    start their blocks at pixel (0, 0): the headers quoted in special_ref)."""
    r = np.random.default_rng(H * W + m)
    Cin, Cout = 3, 2
    x = r.standard_normal((H, W, Cin))
    w = r.standard_normal((Cout, Cin, 3, 3)) + 3.0                                 # no zeros
    clean = sr.winograd_conv3x3(x, w, m)
    direct = orc.conv3x3(x[None].astype(np.float32), w.astype(np.float32))[0]
    assert np.max(np.abs(clean - direct)) < 1e-3, "the literal Winograd is a convolution"
    for (y, xx) in _cases(H, W):
        for bad in (np.nan, np.inf, -np.inf):
            xp = x.copy()
            xp[y, xx, 1] = bad
            with np.errstate(invalid="ignore"):
                out = sr.winograd_conv3x3(xp, w, m)
            hit = ~np.isfinite(out)
            assert np.array_equal(hit.all(axis=-1), hit.any(axis=-1))
            region = fn(H, W, y, xx)
            assert region.any()
            assert np.array_equal(hit.all(axis=-1), region), (m, H, W, y, xx, bad)
            assert np.array_equal(out[~region], clean[~region])
            assert (region & sr.blast_direct(H, W, y, xx)).sum() == sr.blast_direct(H, W, y, xx).sum(), "the footprint lies inside"


@pytest.mark.parametrize("H,W", [(8, 12), (7, 9), (2, 2)])
def test_direct_and_transposed_blast_regions_are_what_the_oracle_poisons(H, W):
    r = np.random.default_rng(H + W)
    Cin, Cout = 4, 8
    x = r.standard_normal((1, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3)) + 3.0).astype(np.float32)
    wt = (r.standard_normal((Cin, Cout, 2, 2)) + 3.0).astype(np.float32)
    bias = r.standard_normal(Cout).astype(np.float32)
    clean, clean_t = orc.conv3x3(x, w), orc.convT2x2(x, wt, bias)
    for (y, xx) in set((min(max(a, 0), H - 1), min(max(b, 0), W - 1)) for a, b in _cases(H, W)):
        for bad in (np.nan, np.inf, -np.inf):
            xp = x.copy()
            xp[0, y, xx, Cin - 1] = bad
            out, out_t = orc.conv3x3(xp, w), orc.convT2x2(xp, wt, bias)
            for o, c, region in ((out, clean, sr.blast_direct(H, W, y, xx)), (out_t, clean_t, sr.blast_convT(H, W, y, xx))):
                hit = ~np.isfinite(o[0])
                assert region.any() and np.array_equal(hit.all(axis=-1), region) and np.array_equal(hit.any(axis=-1), region)
                assert np.array_equal(o[0][~region].view(np.uint32), c[0][~region].view(np.uint32))
                if not np.isnan(bad):
                    assert np.isinf(o[0][region]).all(), "an infinity times a non-zero weight is an infinity"


def test_pooled_region():
    m = np.zeros((6, 8), bool)
    m[2:5, 3:6] = True
    want = np.zeros((3, 4), bool)
    want[1:3, 1:3] = True
    assert np.array_equal(sr.pooled(m), want)
    assert np.array_equal(sr.pooled(np.ones((5, 7), bool)), np.ones((2, 3), bool))          # odd sizes: the last row and column are dropped


# ---------------------------------------------------------------------------------------------------------- oracle classification
def test_oracle_relu_and_pooling_on_non_finite_data():
    """C1 and C6 come from oracle/unet_oracle.c (ReLU is !(v > 0) ? 0 : v, pooling compares with >): pinned here on the values the
    GPU tests feed, so those tests can take their expectation from orc.bn_relu and orc.maxpool2x2."""
    v = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, -2.0 ** -30, -2.0 ** -140, 1.5], np.float32).reshape(1, 8)
    one, zero = np.ones(8, np.float32), np.zeros(8, np.float32)
    got = orc.bn_relu(v, one, zero, zero, one, eps=0.0, relu=True)
    assert np.array_equal(got.view(np.uint32), np.array([0, 0, np.inf, 0, 0, 0, 0, 1.5], np.float32).reshape(1, 8).view(np.uint32))
    keep = orc.bn_relu(v, one, zero, zero, one, eps=0.0, relu=False)
    assert np.isnan(keep[0, 0]) and np.array_equal(keep[0, 1:], v[0, 1:])              # (-0 + the zero shift is +0: values, not bits)
    x = np.zeros((1, 2, 4, 1), np.float32)
    x[0, :, :2, 0] = [[1.0, np.inf], [0.0, 3.0]]
    x[0, :, 2:, 0] = [[0.0, 0.0], [2.0 ** -140, 0.0]]
    assert np.array_equal(orc.maxpool2x2(x).reshape(-1), np.array([np.inf, 2.0 ** -140], np.float32))


# ---------------------------------------------------------------------------------------------------------- host converters
def test_host_converters(tmp_path):
    exe = tmp_path / "lp_convert_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpu", "lp_convert_test.cpp"), "-L" + PKG, "-lmiunet", "-Wl,-rpath," + PKG])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]
    for kind, name in ((1, "bf16"), (2, "fp16")):
        src, want = sr.table(kind, True)
        r = subprocess.run([str(exe), name] + [f"{int(s):08x}" for s in src], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert [int(line, 16) for line in r.stdout.split()] == [int(v) for v in want]
