"""Every layer kernel writes its slice of a strided tensor and nothing else (mi_unet_layer_debug_strided).

The engine's tensors are halves of concat buffers: build_plan produces the dense layout (ldo = Cout), the lower half (ldo = 2 Cout,
co_off = 0: the skips) and the upper half (ldo = 2 Cout, co_off = Cout: transposed convs and upsamples).  Each case here runs one
route at shapes it is already tested at (test_gpu_layers.py, test_gpu_bf16.py, test_gpu_bilinear.py) in every layout the op admits,
between 4096-byte guards, into allocations poisoned with 0xFF bytes, and asserts for the output and for the pooled output:

  1. nothing outside the slice changed (guards, gap channels, the other half of the pixel): slice_ref's stray list is empty;
  2. nothing inside the slice is unwritten: no poison left;
  3. the slice matches the oracle at the family's bar AND is the dense hook's result bit for bit (strides move addresses, not sums);
  4. with ldc = Cin + 32 the input's gap channels hold NaN, and 2 and 3 still hold: the loaders' channel masks.

A stray store that lands farther away than the guard, or one that writes 0xFF bytes, is not seen.
Every run prints one line `slice: <op> <route> <shape> <layout>`: the listing of what ran."""
import zlib

import numpy as np
import pytest

import oracle_lib as orc
import slice_ref
from miunet import binding
from test_gpu_bilinear import _check16, upsample_ref

pytestmark = pytest.mark.gpu

GUARD = 4096

ROUTE = {
    "conv3x3": "conv3x3_mfma", "conv3x3_wino": "conv3x3_wino", "conv3x3_wino16": "conv3x3_wino16", "conv3x3_wino4": "conv3x3_wino4",
    "conv3x3_wino4s": "conv3x3_wino4s", "conv3x3_wino4a": "conv3x3_wino4a", "conv3x3_wino4b": "conv3x3_wino4b",
    "convT2x2": "convT2x2_mfma", "convT2x2_taps": "convT2x2_taps",
    "conv3x3_first": "conv3x3_first", "conv3x3_first_bf16": "conv3x3_first", "conv3x3_first_fp16": "conv3x3_first",
    "maxpool": "maxpool2x2", "maxpool_bf16": "maxpool2x2", "maxpool_fp16": "maxpool2x2",
    "upsample2x": "upsample2x_bilinear", "upsample2x_bf16": "upsample2x_bilinear", "upsample2x_fp16": "upsample2x_bilinear",
}
for _t in ("bf16", "fp16"):
    for _s in ("", "w", "r", "k"):
        ROUTE[f"conv3x3_{_t}{_s}"] = f"conv3x3_{_t}{_s}"
    for _s in ("", "r"):
        ROUTE[f"convT2x2_{_t}{_s}"] = f"convT2x2_{_t}{_s}"


def _core(op):
    for sfx in ("_lpout", "_pool"):
        if op.endswith(sfx):
            op = op[:-len(sfx)]
    return op


def _kind(op):
    return 1 if "_bf16" in op else 2 if "_fp16" in op else 0


def _rnd(op):
    return (lambda a: a, orc.bf16_round, orc.fp16_round)[_kind(op)]


def _bar_fp32(got, ref, what):
    # the bar of test_gpu_layers.py / test_gpu_bf16.py: fp32 sums in another order (16-bit operands: against the rounded-operand oracle)
    err = float(np.max(np.abs(got - ref)))
    assert err < 1e-4 * max(1.0, float(np.abs(ref).max())), (what, err)


def _bar_lp(got, ref, op, what):
    # ... and of their 16-bit outputs: within one rounding of the oracle
    ulp = 2.0 ** -7 if _kind(op) == 1 else 2.0 ** -10
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    assert err < ulp, (what, err)


def _slice(res, which, op, what):
    """assertions 1 and 2 on one returned allocation; the dense slice"""
    shape, c, ld, co_off, guard = res[which + "_layout"]
    kind = _kind(op) if res["elem_bytes"] == 2 else 0
    s = slice_ref.check(res[which], res["elem_bytes"], shape, c, ld, co_off, guard, kind, limit=6)
    assert s.n_strays == 0, f"{what}: the {which} tensor (ld {ld}, co_off {co_off}, C {c}): " + slice_ref.describe(s.strays, s.n_strays, s.summary)
    assert s.unwritten == 0, f"{what}: {s.unwritten} elements of the {which} slice are still poison"
    return s.dense


def _run(op, x, w, scale, shift, relu, layouts, bar, ref, ref_pool=None, dense=None):
    """One op on one set of operands in each layout: `bar(got, ref, what)` is the family's oracle check, `dense` caches the dense
    hook's results (the full-size tensor under the op without _pool, the pooled one under the op itself)."""
    route = ROUTE[_core(op)]
    dense = {} if dense is None else dense
    pooled = "_pool" in op
    full_op = op.replace("_pool", "")
    for o in ([full_op, op] if pooled else [op]):
        if o not in dense:
            dense[o] = binding.layer_debug(o, x, w, scale, shift, relu=relu)
    failures = []                      # every layout runs: a dense run can only show a wrong slice, the halves name the stray stores
    for name, lay in layouts:
        what = f"{op} route {route} x{tuple(x.shape)} Cout {ref.shape[-1]} layout {name} {lay}"
        res = binding.layer_debug_strided(op, x, w, scale, shift, relu=relu, guard_bytes=GUARD, **lay)
        print(f"slice: {op} {res['kernel']} {tuple(x.shape)}->{ref.shape[-1]} {name}")
        assert res["kernel"] == route, what
        try:
            got = _slice(res, "out", op, what)
            bar(got, ref, what)
            assert np.array_equal(got.view(np.uint32), dense[full_op].view(np.uint32)), what + ": differs from the dense hook's bits"
            if pooled:
                gotp = _slice(res, "pool", op, what)
                bar(gotp, ref_pool, what + " (pooled)")
                assert np.array_equal(gotp.view(np.uint32), dense[op].view(np.uint32)), what + ": pooled tensor differs from the dense hook's bits"
        except AssertionError as e:
            failures.append(str(e).split("\nassert ")[0])
    assert not failures, "\n".join(failures)


def _conv_layouts(Cin, Cout, pooled, T=False):
    """dense; the half of the concat pixel the op writes in the plan (conv3x3: lower, transposed conv: upper); that half with gap
    channels behind the input's; for the _pool forms a pooled pixel with a gap too"""
    half = {"ldo": 2 * Cout, "co_off": Cout} if T else {"ldo": 2 * Cout}
    hname = "upper" if T else "lower"
    lays = [("dense", {}), (hname, dict(half)), (hname + "+ldc", dict(half, ldc=Cin + 32))]
    if pooled:
        lays.append((hname + "+pool_ld", dict(half, pool_ld=Cout + 32)))
    return lays


def _conv_operands(B, H, W, Cin, Cout, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    return x, w, scale, shift


def _conv_ref(op, x, w, scale, shift):
    """fp32: the oracle on the operands; 16-bit: on the rounded operands (BN scale folded into the weights first, as the packing does)"""
    if not _kind(op):
        return np.maximum(orc.conv3x3(x, w) * scale + shift, 0.0)
    rnd = _rnd(op)
    wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)
    return np.maximum(orc.conv3x3(rnd(x), rnd(wf)) + shift, 0.0)


def _conv_case(ops, B, H, W, Cin, Cout, pool=False, layouts=None):
    """fp32-output forms of `ops` (with _pool where asked) on one set of operands, one oracle result"""
    x, w, scale, shift = _conv_operands(B, H, W, Cin, Cout, B * 1000 + H * 100 + W + Cin + Cout)
    refs = {}
    for op in ops:
        k = _kind(op)
        if k not in refs:
            refs[k] = _conv_ref(op, x, w, scale, shift)
        ref = refs[k]
        lays = layouts or _conv_layouts(Cin, Cout, pool)
        _run(op + ("_pool" if pool else ""), x, w, scale, shift, True, lays, _bar_fp32, ref, orc.maxpool2x2(ref) if pool else None)


# ------------------------------------------------------------------------------------------ fp32 conv3x3
@pytest.mark.parametrize("B,H,W,Cin,Cout,pool", [
    (1, 5, 7, 32, 64, False),          # ragged: partial tile in x and y
    (1, 9, 33, 24, 32, False),         # masked last chunk, Cout < the n-tile (masked columns)
    (2, 16, 64, 64, 64, False),
    (2, 16, 64, 64, 64, True),
])
@pytest.mark.parametrize("op", ["conv3x3", "conv3x3_wino", "conv3x3_wino16"])
def test_conv3x3_fp32(op, B, H, W, Cin, Cout, pool):
    _conv_case([op], B, H, W, Cin, Cout, pool)


@pytest.mark.parametrize("B,H,W,Cin,Cout,pool", [
    (1, 5, 7, 32, 128, False),         # two-block kernel, ragged
    (1, 9, 33, 24, 96, False),         # one-block: masked last chunk, masked columns
    (1, 21, 35, 128, 64, False),       # one-block, ragged
    (1, 16, 16, 32, 48, False),        # Cout < 64 (masked columns)
    (2, 32, 32, 64, 64, True),
])
def test_conv3x3_wino4_hipcc_kernels(B, H, W, Cin, Cout, pool, monkeypatch):
    """conv3x3_wino4 pinned to the hipcc kernels: two-block where Cout fills 128 channels, one-block below (both report conv3x3_wino4)"""
    monkeypatch.setenv("MIUNET_WINO4_ASM", "0")
    monkeypatch.setenv("MIUNET_WINO4S", "0")
    _conv_case(["conv3x3_wino4"], B, H, W, Cin, Cout, pool)


@pytest.mark.parametrize("B,H,W,Cin,Cout,pool", [
    (1, 9, 33, 24, 40, False),         # masked last chunk, masked columns
    (1, 18, 18, 16, 64, False),        # a 2-pixel rim past the block boundary
    (2, 16, 32, 48, 64, False),
    (2, 16, 32, 48, 64, True),
])
def test_conv3x3_wino4s(B, H, W, Cin, Cout, pool):
    _conv_case(["conv3x3_wino4s"], B, H, W, Cin, Cout, pool)


@pytest.mark.parametrize("B,H,W,Cin,Cout,pool", [
    (1, 16, 16, 64, 128, False),
    (1, 32, 32, 64, 128, True),
    (2, 32, 48, 128, 256, False),
])
def test_conv3x3_wino4a(B, H, W, Cin, Cout, pool):
    _conv_case(["conv3x3_wino4a"], B, H, W, Cin, Cout, pool)


@pytest.mark.parametrize("B,H,W,Cin,Cout,pool", [
    (1, 16, 32, 64, 64, False),
    (1, 32, 64, 64, 64, True),
    (2, 32, 64, 128, 64, False),
])
def test_conv3x3_wino4b(B, H, W, Cin, Cout, pool):
    _conv_case(["conv3x3_wino4b"], B, H, W, Cin, Cout, pool)


@pytest.mark.parametrize("op,B,H,W,Cin,Cout", [
    ("conv3x3_wino4a", 5, 128, 128, 64, 128),      # 320 blocks of 16 x 16 on 256 compute units
    ("conv3x3_wino4b", 9, 128, 128, 64, 64),       # 288 blocks of 16 x 32
])
def test_conv3x3_assembly_persistent_hand_over(op, B, H, W, Cin, Cout):
    """more blocks than compute units: a persistent workgroup's second block lies in another image, whose stride includes ldo.
    The lower half only (the layout these layers write in the plan): each run downloads about 80 MB."""
    _conv_case([op], B, H, W, Cin, Cout, layouts=[("lower", {"ldo": 2 * Cout})])


# ------------------------------------------------------------------------------------------ 16-bit conv3x3
def _lp_case(op, B, H, W, Cin, Cout, forms, seed_extra=0):
    """the listed forms ("", "_lpout", "_pool", "_pool_lpout") of one 16-bit op on one set of operands and one oracle result"""
    x, w, scale, shift = _conv_operands(B, H, W, Cin, Cout, B + 3 * H + 5 * W + Cin + Cout + seed_extra)
    ref = _conv_ref(op, x, w, scale, shift)
    refp = orc.maxpool2x2(ref) if any("_pool" in f for f in forms) else None
    dense = {}
    for f in forms:
        bar = (lambda g, r, what: _bar_lp(g, r, op, what)) if f.endswith("_lpout") else _bar_fp32
        _run(op + f, x, w, scale, shift, True, _conv_layouts(Cin, Cout, "_pool" in f), bar, ref, refp, dense)


@pytest.mark.parametrize("B,H,W,Cin,Cout,forms", [
    (1, 5, 7, 40, 64, ("", "_lpout")),                       # ragged, masked last chunk
    (1, 9, 33, 24, 32, ("", "_lpout")),                      # the 32-wide n-tile
    (1, 9, 33, 24, 40, ("", "_lpout")),                      # Cout < the 64-wide n-tile: masked lanes, masked 16-byte pieces
    (2, 16, 64, 64, 64, ("_pool", "_pool_lpout")),
    (1, 10, 34, 24, 40, ("_pool", "_pool_lpout")),           # ... and the same channel mask in the pooled tile's 16-byte store
])
@pytest.mark.parametrize("op", ["conv3x3_bf16", "conv3x3_fp16"])
def test_conv3x3_16bit(op, B, H, W, Cin, Cout, forms):
    _lp_case(op, B, H, W, Cin, Cout, forms)


@pytest.mark.parametrize("B,H,W,Cin,Cout,forms", [
    (1, 21, 45, 40, 128, ("", "_lpout")),                    # ragged in x and y, masked last chunk
    (1, 8, 8, 256, 256, ("", "_lpout", "_pool")),            # a tile mostly past the image
    (1, 40, 70, 128, 128, ("_pool_lpout",)),
])
@pytest.mark.parametrize("op", ["conv3x3_bf16w", "conv3x3_fp16w"])
def test_conv3x3_16bit_wide(op, B, H, W, Cin, Cout, forms):
    _lp_case(op, B, H, W, Cin, Cout, forms)


@pytest.mark.parametrize("B,H,W,Cin,Cout,forms", [
    (2, 16, 64, 64, 64, ("_lpout",)),
    (1, 21, 45, 64, 32, ("_lpout",)),                        # ragged in x and y, odd height
    (1, 24, 100, 32, 32, ("_lpout",)),                       # a 4-pixel tile column
    (3, 96, 80, 32, 32, ("_pool_lpout",)),                   # 16-row tiles, a 16-column tile column
    (2, 256, 512, 32, 32, ("_lpout",)),                      # 512 tiles: two per persistent workgroup
])
@pytest.mark.parametrize("op", ["conv3x3_bf16r", "conv3x3_fp16r"])
def test_conv3x3_16bit_resident(op, B, H, W, Cin, Cout, forms):
    _lp_case(op, B, H, W, Cin, Cout, forms)


@pytest.mark.parametrize("B,H,W", [(2, 9, 40), (1, 12, 100), (1, 64, 512)])
@pytest.mark.parametrize("op", ["conv3x3_bf16k", "conv3x3_fp16k"])
def test_conv3x3_16bit_k_split(op, B, H, W):
    _lp_case(op, B, H, W, 128, 64, ("_lpout",))


# ------------------------------------------------------------------------------------------ transposed conv
def _convT_case(ops, B, H, W, Cin, Cout):
    r = np.random.default_rng(H * 7 + W + Cin)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cin, Cout, 2, 2), dtype=np.float32) / np.sqrt(Cin)).astype(np.float32)
    bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    refs, dense = {}, {}
    for op in ops:
        k = _kind(op)
        if k not in refs:
            rnd = _rnd(op)
            refs[k] = orc.convT2x2(rnd(x), rnd(w), bias)
        bar = (lambda g, rf, what, op=op: _bar_lp(g, rf, op, what)) if op.endswith("_lpout") else _bar_fp32
        _run(op, x, w, None, bias, False, _conv_layouts(Cin, Cout, False, T=True), bar, refs[k], None, dense)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [
    (1, 8, 32, 64, 32),                # N = 128: taps straddle a 64-column tile boundary
    (2, 9, 70, 40, 128),               # ragged rows and columns, Cin % 32 != 0
    (1, 2, 33, 64, 576),               # two n-tiles, masked channels
])
@pytest.mark.parametrize("op", ["convT2x2", "convT2x2_taps", "convT2x2_taps:large"])
def test_convT2x2_fp32(op, B, H, W, Cin, Cout, monkeypatch):
    if op.endswith(":large"):          # the whole-batch tile shapes on the same inputs (test_gpu_layers.py)
        monkeypatch.setenv("MIUNET_CONVT_SMALL", "0")
        op = op.split(":")[0]
    _convT_case([op], B, H, W, Cin, Cout)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 8, 32, 64, 32), (1, 3, 5, 1024, 512)])
@pytest.mark.parametrize("t", ["bf16", "fp16"])
def test_convT2x2_16bit(t, B, H, W, Cin, Cout):
    _convT_case([f"convT2x2_{t}", f"convT2x2_{t}_lpout"], B, H, W, Cin, Cout)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 9, 40, 64, 32), (1, 5, 33, 128, 64), (3, 3, 70, 256, 128)])
@pytest.mark.parametrize("t", ["bf16", "fp16"])
def test_convT2x2_16bit_resident(t, B, H, W, Cin, Cout):
    _convT_case([f"convT2x2_{t}r_lpout"], B, H, W, Cin, Cout)


# ------------------------------------------------------------------------------------------ first layer
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 37, 70, 1, 64), (1, 40, 96, 3, 32)])
def test_first_layer(B, H, W, Cin, Cout, monkeypatch):
    """the fp32 form (VALU kernel) and the 16-bit forms on the MFMA kernel and, with MIUNET_FIRST_MFMA=0, on the VALU kernel; the
    first layer has an output stride only (dense, and the lower half of a pixel twice as wide)"""
    r = np.random.default_rng(H + 3 * W + Cin + Cout)
    x = r.integers(0, 256, (B, H, W, Cin)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)
    ref = np.maximum(orc.conv3x3(x / np.float32(255.0), wf) + shift, 0.0)
    lays = [("dense", {}), ("lower", {"ldo": 2 * Cout})]
    _run("conv3x3_first", x, w, scale, shift, True, lays, _bar_fp32, ref)
    for mode in ("1", "0"):
        monkeypatch.setenv("MIUNET_FIRST_MFMA", mode)
        for op in ("conv3x3_first_bf16", "conv3x3_first_fp16"):
            _run(op, x, w, scale, shift, True, [(f"{n} MIUNET_FIRST_MFMA={mode}", l) for n, l in lays],
                 lambda g, rf, what, op=op: _bar_lp(g, rf, op, what), ref)


# ------------------------------------------------------------------------------------------ upsample, pooling
@pytest.mark.parametrize("op", ["upsample2x", "upsample2x_bf16", "upsample2x_fp16"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (3, 2), (7, 5), (32, 32), (64, 128)])
@pytest.mark.parametrize("c", [16, 64, 512])
def test_upsample(op, hw, c):
    """test_upsample_layer's grid (test_gpu_bilinear.py) and its bars, at its batch sizes 1 and 3.  One run of the grid is left out:
    (64, 128) x 512 at batch 3, whose 2 C-wide allocation is 402 MB in fp32 (201 MB in 16 bits); that pair runs at batch 1 in all
    three element types (fp32: 134 MB).  As there, the 16-bit bar (round16 of the float64 reference, rare one-ulp straddles) is
    taken over both batches of the case together."""
    rng = np.random.default_rng(zlib.crc32(repr((op, hw, c)).encode()))
    es = 4 if op == "upsample2x" else 2
    lays = [("dense", {}), ("upper", {"ldo": 2 * c, "co_off": c}), ("upper+ldi", {"ldo": 2 * c, "co_off": c, "ldc": c + 32})]
    rnd, mant = (None, 0) if es == 4 else (orc.bf16_round, 7) if op.endswith("bf16") else (orc.fp16_round, 10)
    seen, top, ran = {}, 1.0, 0        # 16-bit: layout -> [(got, ref)] over the batches
    for b in (1, 3):
        if (hw, c, b) == ((64, 128), 512, 3):
            continue
        ran += 1
        x = (rng.standard_normal((b, hw[0], hw[1], c)) * 3.0).astype(np.float32)
        top = max(top, float(np.abs(x).max()))
        if es == 4:
            ref = upsample_ref(x)

            def bar(got, ref, what, top=max(1.0, float(np.abs(x).max()))):       # test_gpu_bilinear.py's bar
                err = float(np.max(np.abs(got - ref)))
                assert err <= 1e-6 * top, (what, err)
        else:
            ref = upsample_ref(rnd(x))

            def bar(got, ref, what):
                seen.setdefault(what.split(" layout ")[1], []).append((got.reshape(-1), np.asarray(ref).reshape(-1)))
        _run(op, x, None, None, None, False, lays, bar, ref)
    assert ran >= 1 and (es == 4 or len(seen) == len(lays)), "no batch of the case ran"
    for lay, pairs in seen.items():
        try:
            _check16(np.concatenate([g for g, _ in pairs]), np.concatenate([r for _, r in pairs]), rnd, mant, 1e-6 * top)
        except AssertionError as e:
            raise AssertionError(f"{op} {hw} x {c} layout {lay}: {e}") from None


@pytest.mark.parametrize("B,H,W,C", [(2, 6, 10, 64), (1, 64, 64, 128)])
@pytest.mark.parametrize("op", ["maxpool", "maxpool_bf16", "maxpool_fp16"])
def test_maxpool(op, B, H, W, C):
    """the stand-alone pooling reads the lower half of a concat buffer (ldc = 2 C) and writes dense; the 16-bit kernel orders bit
    patterns, which is the order of the non-negative (post-ReLU) values it is given"""
    x = np.random.default_rng(C).standard_normal((B, H, W, C), dtype=np.float32)
    x = np.abs(x) if _kind(op) else x
    ref = orc.maxpool2x2(_rnd(op)(x))

    def bar(got, ref, what):
        assert np.array_equal(got, ref), what
    _run(op, x, None, None, None, False, [("dense", {}), ("ldc=2C", {"ldc": 2 * C})], bar, ref)


# ------------------------------------------------------------------------------------------ the hook's own contract
def test_layouts_outside_the_bounds_are_refused_before_any_launch():
    x = np.zeros((1, 16, 32, 64), np.float32)
    w = np.zeros((64, 64, 3, 3), np.float32)
    for lay in ({"ldc": 56}, {"ldo": 56}, {"ldo": 128, "co_off": 72}, {"co_off": -8, "ldo": 128}, {"guard_bytes": 100},
                {"pool_ld": 96}):                                        # pool_ld without _pool
        with pytest.raises(binding.MiUnetError, match="layer_debug"):
            binding.layer_debug_strided("conv3x3", x, w, **lay)
    with pytest.raises(binding.MiUnetError, match="layer_debug"):
        binding.layer_debug_strided("conv3x3_pool", x, w, pool_ld=56)
    with pytest.raises(binding.MiUnetError, match="layer_debug"):
        binding.layer_debug_strided("maxpool", x, ldo=128)               # maxpool writes dense
    with pytest.raises(binding.MiUnetError, match="layer_debug"):
        binding.layer_debug_strided("conv3x3_first", np.zeros((1, 8, 8, 1), np.float32), np.zeros((32, 1, 3, 3), np.float32), co_off=32, ldo=64)
    # ... and a layout the route's own contract refuses comes back as the launcher's error: conv3x3_bf16r needs ldo % 8 == 0
    with pytest.raises(binding.MiUnetError, match="launch_route"):
        binding.layer_debug_strided("conv3x3_bf16r_lpout", x, w, ldo=132, guard_bytes=GUARD)
