"""BASELINE config 3: bf16 conv operands, fp32 accumulate (MI_UNET_CONV_BF16).  The checker is the oracle's bf16-operand
mode (same rounding points: weights after BN folding, activations at every MFMA conv input), so the tolerance stays
tight; the distance to the fp32 network is reported separately."""
import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 8, 32, 32, 64), (2, 16, 64, 64, 64), (1, 5, 7, 40, 64), (1, 12, 40, 96, 128),
                                            (1, 9, 33, 24, 32), (3, 4, 4, 128, 256), (1, 2, 2, 1024, 64)])
def test_conv3x3_bf16(B, H, W, Cin, Cout):
    r = np.random.default_rng(B * 1000 + H * 100 + W + Cin + Cout)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    got = binding.layer_debug("conv3x3_bf16", x, w, scale, shift, relu=True)
    wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)
    ref = np.maximum(orc.conv3x3(orc.bf16_round(x), orc.bf16_round(wf)) + shift, 0.0)
    assert not np.isnan(got).any()
    assert np.max(np.abs(got - ref)) < 1e-4 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("op,rnd,ulp", [("conv3x3_bf16", orc.bf16_round, 2.0 ** -8), ("conv3x3_fp16", orc.fp16_round, 2.0 ** -11),
                                        ("convT2x2_bf16", orc.bf16_round, 2.0 ** -8), ("convT2x2_fp16", orc.fp16_round, 2.0 ** -11)])
def test_16bit_output_tensors_are_the_rounded_fp32_results(op, rnd, ulp):
    """Inside the network every activation tensor of the 16-bit pipelines is 16-bit in HBM: the producing kernel rounds its
    fp32 result once (RNE) -- exactly the rounding its consumer used to apply while staging.  `<op>_lpout` returns that
    tensor: it must equal round(fp32 result) except where the two fp32 sums (different order) straddle a rounding boundary,
    and then by one unit in the last place."""
    r = np.random.default_rng(99)
    T = op.startswith("convT")
    x = r.standard_normal((2, 9, 40, 64), dtype=np.float32)          # ragged rows, two column tiles
    if T:
        w = (r.standard_normal((64, 64, 2, 2), dtype=np.float32) / 8.0).astype(np.float32)
        shift = (0.1 * r.standard_normal(64)).astype(np.float32)
        f32 = binding.layer_debug(op, x, w, None, shift)
        got = binding.layer_debug(op + "_lpout", x, w, None, shift)
    else:
        w = (r.standard_normal((128, 64, 3, 3), dtype=np.float32) * np.sqrt(2.0 / 576)).astype(np.float32)
        shift = (0.1 * r.standard_normal(128)).astype(np.float32)
        f32 = binding.layer_debug(op, x, w, None, shift, relu=True)
        got = binding.layer_debug(op + "_lpout", x, w, None, shift, relu=True)
    assert not np.isnan(got).any() and got.shape == f32.shape
    assert np.array_equal(got, rnd(f32))                               # same kernel, same sums: the store only rounds
    assert np.array_equal(rnd(got), got)                               # values are representable in the 16-bit type
    assert np.max(np.abs(got - f32)) <= ulp * float(np.abs(f32).max())


def test_conv3x3_bf16_exact_on_small_integers():
    r = np.random.default_rng(11)                       # small integers are exact in bf16 and in fp32 sums
    x = r.integers(-4, 5, (1, 10, 36, 32)).astype(np.float32)
    w = r.integers(-3, 4, (64, 32, 3, 3)).astype(np.float32)
    assert np.array_equal(binding.layer_debug("conv3x3_bf16", x, w), orc.conv3x3(x, w))


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 8, 32, 64, 32), (2, 4, 4, 128, 64), (1, 3, 5, 1024, 512)])
def test_convT2x2_bf16(B, H, W, Cin, Cout):
    r = np.random.default_rng(H * 7 + W + Cin)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cin, Cout, 2, 2), dtype=np.float32) / np.sqrt(Cin)).astype(np.float32)
    bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    got = binding.layer_debug("convT2x2_bf16", x, w, None, bias)
    ref = orc.convT2x2(orc.bf16_round(x), orc.bf16_round(w), bias)
    assert np.max(np.abs(got - ref)) < 1e-4 * max(1.0, float(np.abs(ref).max()))


def test_end_to_end_tolerances():
    """End to end the bf16-operand network is NOT reproducible to fp32 tolerance by any second implementation: an
    upstream difference of 1e-7 (summation order, fma contraction) flips some bf16 roundings of the activations and moves
    the logits by ~6e-3 (measured with the oracle against itself, weights perturbed by 1e-7).  So: each kernel is pinned
    tightly above on identical inputs, and the whole network is held to the size of the bf16 quantisation noise itself --
    within 3e-2 of the bf16-operand oracle AND no further from the fp32 oracle than that oracle's own bf16 mode is
    (x1.5), labels equal wherever the fp32 top-2 margin exceeds 0.1."""
    spec = UNetSpec()
    blob = pack_weights(spec, synth.make_weights(spec, 4321))
    imgs = synth.make_images(3, 128, 128, 1, 0xBEEF, "blobs")
    ref16, _ = orc.unet_forward(blob, imgs, bf16=True)
    ref32, lab32 = orc.unet_forward(blob, imgs)
    with binding.Engine(128, 128, max_batch=2, conv_algo="bf16") as eng:
        eng.load_weights(blob)
        labels, logits = eng.infer(imgs, want_logits=True)
    noise = float(np.max(np.abs(ref16 - ref32)))             # what bf16 operands cost in this network
    assert 1e-3 < noise < 0.1
    assert float(np.max(np.abs(logits - ref16))) < 3e-2
    assert float(np.max(np.abs(logits - ref32))) < 1.5 * noise
    srt = np.sort(ref32, axis=1)
    safe = (srt[:, -1] - srt[:, -2]) > 0.1
    assert safe.mean() > 0.5 and np.array_equal(labels[safe], lab32[safe])
    assert np.array_equal(labels, np.stack([orc.argmax_planar(l) for l in logits]))    # argmax rule is exact on its own logits


# ---------------------------------------------------------------- fp16 operands (BASELINE config 5's arithmetic)
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 8, 32, 32, 64), (1, 5, 7, 40, 32), (2, 4, 4, 128, 256)])
def test_conv3x3_fp16(B, H, W, Cin, Cout):
    r = np.random.default_rng(B + H + W + Cin + Cout)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    got = binding.layer_debug("conv3x3_fp16", x, w, scale, shift, relu=True)
    wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)
    ref = np.maximum(orc.conv3x3(orc.fp16_round(x), orc.fp16_round(wf)) + shift, 0.0)
    assert np.max(np.abs(got - ref)) < 1e-4 * max(1.0, float(np.abs(ref).max()))


def test_convT2x2_fp16():
    r = np.random.default_rng(9)
    x = r.standard_normal((1, 6, 10, 64), dtype=np.float32)
    w = (r.standard_normal((64, 32, 2, 2), dtype=np.float32) / 8).astype(np.float32)
    bias = (0.1 * r.standard_normal(32)).astype(np.float32)
    got = binding.layer_debug("convT2x2_fp16", x, w, None, bias)
    ref = orc.convT2x2(orc.fp16_round(x), orc.fp16_round(w), bias)
    assert np.max(np.abs(got - ref)) < 1e-4 * max(1.0, float(np.abs(ref).max()))


def test_config5_fp16_1024_three_channels_five_levels():
    """BASELINE config 5: 1024x1024x3, 5 levels, base 32, fp16 operands / fp32 accumulate.  fp16 carries 11 significant
    bits, so its rounding-flip noise is 8x smaller than bf16's: held to 5e-3 of the fp16-operand oracle and 1.5x that
    oracle's own distance to the fp32 network."""
    spec = UNetSpec(3, 32, 5, 3)
    blob = pack_weights(spec, synth.make_weights(spec, 555))
    imgs = synth.make_images(1, 1024, 1024, 3, 0xC5, "blobs")
    ref16, _ = orc.unet_forward(blob, imgs, fp16=True)
    ref32, lab32 = orc.unet_forward(blob, imgs)
    with binding.Engine(1024, 1024, 3, 32, 5, 3, max_batch=1, conv_algo="fp16") as eng:
        eng.load_weights(blob)
        labels, logits = eng.infer(imgs, want_logits=True)
    noise = float(np.max(np.abs(ref16 - ref32)))
    assert 1e-5 < noise < 2e-2
    assert float(np.max(np.abs(logits - ref16))) < 5e-3
    assert float(np.max(np.abs(logits - ref32))) < 1.5 * noise + 1e-3
    srt = np.sort(ref32, axis=1)
    safe = (srt[:, -1] - srt[:, -2]) > 2e-2
    assert np.array_equal(labels[safe], lab32[safe])


# ---------------------------------------------------------------- the wide-layer kernel (conv_lp2.hip: 4 x 4 register tile per wave)
@pytest.mark.parametrize("op,B,H,W,Cin,Cout", [
    ("conv3x3_bf16", 2, 16, 32, 64, 128),       # exactly one tile per image, two chunks
    ("conv3x3_bf16", 1, 21, 45, 40, 128),       # ragged in x and y, Cin % 32 != 0 (masked last chunk)
    ("conv3x3_bf16", 1, 8, 8, 256, 256),        # a deep-layer shape: two n-tiles, eight chunks, a tile mostly past the image
    ("conv3x3_fp16", 1, 32, 64, 32, 128),       # several tiles, a single chunk
    ("conv3x3_fp16", 1, 5, 7, 96, 384),         # three n-tiles
    ("conv3x3_bf16", 1, 40, 70, 128, 128),      # interior and edge tiles, four chunks, fused pooling
])
def test_conv3x3_wide_kernel(op, B, H, W, Cin, Cout):
    """Same products, same fp32 accumulation chain (chunks of 32 channels in order, taps in raster order, one v_mfma_f32_16x16x32 per
    tap and chunk) as the 2 x 2 kernel: pinned to the rounded-operand oracle at 1e-4 AND bit-identical to that kernel, 16-bit
    outputs and the fused 2 x 2 pooling included."""
    r = np.random.default_rng(B + 3 * H + 5 * W + Cin + Cout)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    rnd = orc.bf16_round if op.endswith("bf16") else orc.fp16_round
    got = binding.layer_debug(op + "w", x, w, scale, shift, relu=True)
    wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)
    ref = np.maximum(orc.conv3x3(rnd(x), rnd(wf)) + shift, 0.0)
    assert not np.isnan(got).any(), "unwritten (NaN-poisoned) outputs"
    assert np.max(np.abs(got - ref)) < 1e-4 * max(1.0, float(np.abs(ref).max()))
    assert np.array_equal(got, binding.layer_debug(op, x, w, scale, shift, relu=True))
    got16 = binding.layer_debug(op + "w_lpout", x, w, scale, shift, relu=True)
    assert np.array_equal(got16, binding.layer_debug(op + "_lpout", x, w, scale, shift, relu=True))
    assert np.array_equal(got16, rnd(got))                    # the stored 16-bit tensor = one rounding of the fp32 result
    if H % 2 == 0 and W % 2 == 0:
        pooled = binding.layer_debug(op + "w_pool_lpout", x, w, scale, shift, relu=True)
        assert np.array_equal(pooled, orc.maxpool2x2(got16))


@pytest.mark.parametrize("algo", ["bf16", "fp16"])
def test_wide_kernel_in_the_whole_network(algo, monkeypatch):
    """MIUNET_LP2=2 sends every Cout % 128 == 0 layer (fused pooling included) to the wide kernel whatever its grid, =0 none:
    identical arithmetic, so logits and label maps must agree bit for bit."""
    spec = UNetSpec(1, 64, 3, 3)
    blob = pack_weights(spec, synth.make_weights(spec, 31))
    imgs = synth.make_images(3, 88, 72, 1, 0x99, "blobs")
    out = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("MIUNET_LP2", mode)
        with binding.Engine(88, 72, 1, 64, 3, 3, max_batch=2, conv_algo=algo) as eng:
            eng.load_weights(blob)
            out[mode] = eng.infer(imgs, want_logits=True)
    assert np.array_equal(out["0"][1], out["2"][1]) and np.array_equal(out["0"][0], out["2"][0])


# ---------------------------------------------------------------- the narrow-layer kernel (conv_lpr.hip: weights in registers, persistent)
@pytest.mark.parametrize("op,B,H,W,Cin,Cout", [
    ("conv3x3_bf16", 2, 16, 64, 64, 64),        # 64 -> 64: one 32-channel block per wave, both column halves; border tiles only
    ("conv3x3_bf16", 1, 40, 96, 64, 64),        # ... with interior tiles (offsets through the scalar offset)
    ("conv3x3_fp16", 1, 24, 100, 32, 32),       # 32 -> 32, ragged in x (a 4-pixel tile column)
    ("conv3x3_fp16", 1, 21, 45, 64, 32),        # 64 -> 32, ragged in x and y, odd height
    ("conv3x3_bf16", 3, 8, 32, 32, 64),         # 32 -> 64, one tile per image
    ("conv3x3_fp16", 1, 72, 160, 32, 64),       # 32 -> 64 with interior tiles
])
def test_conv3x3_resident_weights(op, B, H, W, Cin, Cout):
    """Same products and fp32 accumulation order as the 2 x 2 kernel: its stored 16-bit tensor bit for bit, and within one
    16-bit rounding of the rounded-operand oracle."""
    r = np.random.default_rng(7 * B + 3 * H + 5 * W + Cin + Cout)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    rnd = orc.bf16_round if op.endswith("bf16") else orc.fp16_round
    got16 = binding.layer_debug(op + "r_lpout", x, w, scale, shift, relu=True)
    assert not np.isnan(got16).any(), "unwritten (NaN-poisoned) outputs"
    assert np.array_equal(got16, binding.layer_debug(op + "_lpout", x, w, scale, shift, relu=True))
    wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)
    ref = np.maximum(orc.conv3x3(rnd(x), rnd(wf)) + shift, 0.0)
    ulp = 2.0 ** -7 if op.endswith("bf16") else 2.0 ** -10
    assert np.max(np.abs(got16 - ref) / np.maximum(1.0, np.abs(ref))) < ulp


@pytest.mark.parametrize("op,Cin,Cout", [("conv3x3_fp16", 32, 32), ("conv3x3_bf16", 64, 64)])
def test_conv3x3_resident_weights_many_tiles_per_workgroup(op, Cin, Cout):
    """2 048 tiles on 256 persistent workgroups: eight tiles each, so the patch ring wraps (twice at depth 4) and every
    wait / barrier of the steady state runs; compared with the one-tile-per-workgroup kernel bit for bit."""
    r = np.random.default_rng(Cin + Cout)
    x = r.standard_normal((2, 256, 1024, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    got16 = binding.layer_debug(op + "r_lpout", x, w, None, shift, relu=True)
    assert not np.isnan(got16).any()
    assert np.array_equal(got16, binding.layer_debug(op + "_lpout", x, w, None, shift, relu=True))


@pytest.mark.parametrize("algo,in_ch,base,levels", [("fp16", 3, 32, 3), ("bf16", 1, 32, 2), ("bf16", 1, 64, 2)])
def test_resident_weight_kernel_in_the_whole_network(algo, in_ch, base, levels, monkeypatch):
    """base 32: inc.c2 (32 -> 32, pooled), down1.c1 (32 -> 64), down1.c2 (64 -> 64, pooled), the second-level up.c2 (64 -> 64)
    and the top up.c1 (64 -> 32) all fit the resident-weight kernel, and so does the last conv (32 -> 32) with the fp32 head
    fused -- every shape, the fused pooling, concat-buffer strides, the head's summation order.  base 64 (BASELINE config 3's
    network): inc.c2 (64 -> 64, pooled); its last conv (64 -> 64 + head) stays on the one-tile-per-workgroup kernel.
    MIUNET_LPR=2 sends them there whatever the grid, =0 nowhere: identical arithmetic, identical logits and labels."""
    spec = UNetSpec(in_ch, base, levels, 3)
    blob = pack_weights(spec, synth.make_weights(spec, 77))
    imgs = synth.make_images(3, 96, 80, in_ch, 0x51, "blobs")
    out, used = {}, {}
    for mode in ("0", "2"):
        monkeypatch.setenv("MIUNET_LPR", mode)
        with binding.Engine(96, 80, in_ch, base, levels, 3, max_batch=3, conv_algo=algo) as eng:
            eng.load_weights(blob)
            eng.set_profiling(True)
            out[mode] = eng.infer(imgs, want_logits=True)
            used[mode] = sorted(s["kernel"] for s in eng.kernel_stats() if "16r" in s["kernel"])
    # (a three-channel image into 32 -> 32 -- BASELINE config 5's top level: the first layer runs inside inc.c2's launch, "+first";
    # with MIUNET_LPR=0 it is a launch of its own, and the logits are the same bits)
    r = f"conv3x3_{algo}r"
    want = [r] * 4 + [r + "+first", r + "+head"] if (base, in_ch) == (32, 3) else [r] * 5 + [r + "+head"] if base == 32 else [r]
    assert used["0"] == [] and used["2"] == want
    assert np.array_equal(out["0"][1], out["2"][1]) and np.array_equal(out["0"][0], out["2"][0])


@pytest.mark.parametrize("op,B,H,W,Cin,Cout", [
    ("conv3x3_fp16", 3, 96, 80, 32, 32),        # 16-row tiles (two row blocks per wave), a 16-column tile column
    ("conv3x3_bf16", 2, 256, 512, 32, 32),      # 512 tiles: two per persistent workgroup
    ("conv3x3_bf16", 2, 40, 96, 64, 64),        # 64 -> 64 (8-row tiles)
    ("conv3x3_fp16", 1, 24, 64, 32, 64),        # 32 -> 64
])
def test_conv3x3_resident_weights_fused_pooling(op, B, H, W, Cin, Cout):
    """The 2 x 2 max pooling fused into the epilogue (in-lane: a row block is 2 rows x 16 columns): the pooled 16-bit tensor
    equals the one-tile-per-workgroup kernel's bit for bit, and the max pooling of the full-size tensor."""
    r = np.random.default_rng(11 * B + H + W + Cin + Cout)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    full = binding.layer_debug(op + "r_lpout", x, w, None, shift, relu=True)
    for _ in range(3):                        # (a race between waves would not show every time)
        pooled = binding.layer_debug(op + "r_pool_lpout", x, w, None, shift, relu=True)
        assert not np.isnan(pooled).any(), "unwritten (NaN-poisoned) pooled outputs"
        assert np.array_equal(pooled, orc.maxpool2x2(full))
    assert np.array_equal(pooled, binding.layer_debug(op + "_pool_lpout", x, w, None, shift, relu=True))


# ---------------------------------------------------------------- 128 -> 64 with the reduction split over a wave pair (conv_lprk.hip)
@pytest.mark.parametrize("op,B,H,W", [
    ("conv3x3_bf16", 1, 4, 32),         # exactly one 4 x 32 tile
    ("conv3x3_fp16", 2, 9, 40),         # ragged in x and y, border tiles only
    ("conv3x3_bf16", 1, 12, 100),       # interior tiles (precomputed DMA offsets) next to border tiles
    ("conv3x3_fp16", 1, 64, 512),       # 256 tiles: the patch ring wraps, steady-state waits and both barriers
    ("conv3x3_bf16", 2, 256, 256),      # 1 024 tiles on 256 persistent workgroups
])
def test_conv3x3_resident_weights_k_split(op, B, H, W):
    """up4.c1's shape (128 -> 64): each wave of a pair sums 64 input channels, the halves meet in LDS.  Same products as the
    2 x 2 kernel, one fp32 add associated differently -- so the stored 16-bit tensor equals the 2 x 2 kernel's except where the
    two fp32 sums straddle a rounding boundary (then by one unit in the last place, rarely), and it is within one 16-bit
    rounding of the rounded-operand oracle."""
    Cin, Cout = 128, 64
    r = np.random.default_rng(13 * B + H + 3 * W)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    rnd = orc.bf16_round if op.endswith("bf16") else orc.fp16_round
    ulp = 2.0 ** -7 if op.endswith("bf16") else 2.0 ** -10
    got = binding.layer_debug(op + "k_lpout", x, w, scale, shift, relu=True)
    assert not np.isnan(got).any(), "unwritten (NaN-poisoned) outputs"
    assert np.array_equal(rnd(got), got)
    for _ in range(2):                        # (a race between the waves of a pair would not show every time)
        assert np.array_equal(got, binding.layer_debug(op + "k_lpout", x, w, scale, shift, relu=True))
    two_by_two = binding.layer_debug(op + "_lpout", x, w, scale, shift, relu=True)
    d = np.abs(got - two_by_two)
    assert np.all(d <= ulp * np.maximum(np.abs(got), np.abs(two_by_two)) + 1e-6) and float(np.mean(d > 0)) < 5e-3
    if H * W <= 64 * 512:
        wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)
        ref = np.maximum(orc.conv3x3(rnd(x), rnd(wf)) + shift, 0.0)
        assert np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))) < ulp


@pytest.mark.parametrize("algo", ["bf16", "fp16"])
def test_k_split_kernel_in_the_whole_network(algo, monkeypatch):
    """base 64, two levels: the top up.c1 is 128 -> 64 reading the concat buffer (channel stride 128, skip first).  MIUNET_LPRK=2
    sends it to the K-split kernel whatever the grid, =0 to the 2 x 2 kernel: same logits to fp32 re-association noise amplified
    by one 16-bit rounding per layer behind it, same labels wherever the margin is not at that noise level."""
    spec = UNetSpec(1, 64, 2, 3)
    blob = pack_weights(spec, synth.make_weights(spec, 31))
    imgs = synth.make_images(2, 96, 80, 1, 0x77, "blobs")
    out, used = {}, {}
    for mode in ("0", "2"):
        monkeypatch.setenv("MIUNET_LPRK", mode)
        with binding.Engine(96, 80, 1, 64, 2, 3, max_batch=2, conv_algo=algo) as eng:
            eng.load_weights(blob)
            eng.set_profiling(True)
            out[mode] = eng.infer(imgs, want_logits=True)
            used[mode] = [s["name"] for s in eng.kernel_stats() if s["kernel"].endswith("16k")]
    assert used["0"] == [] and used["2"] == ["up2.c1"]
    diff = float(np.max(np.abs(out["0"][1] - out["2"][1])))
    assert diff < (2e-2 if algo == "bf16" else 3e-3), diff
    srt = np.sort(out["0"][1], axis=1)
    safe = (srt[:, -1] - srt[:, -2]) > 0.1
    assert np.array_equal(out["0"][0][safe], out["2"][0][safe])


@pytest.mark.parametrize("algo", ["bf16", "fp16"])
def test_tail_micro_batch_takes_other_kernels_and_gives_the_same_bits(algo, monkeypatch):
    """Kernel routing depends on the grid, hence on the micro-batch size: with max_batch = 2 a batch of three runs its third image
    alone, and at 512 x 512 several layers then fall under a routing threshold (e.g. the 128-channel level: 256 tiles fill the
    wide kernel's grid at two images, 128 do not).  The kernel families are bit-identical by construction, so the image must come
    out the same bit for bit whether it ran alone or as the first of a pair.  (The K-split 128 -> 64 kernel differs from the 2 x 2
    kernel by one fp32 add: switched off here; at the bench sizes its routing does not depend on the batch.)"""
    monkeypatch.setenv("MIUNET_LPRK", "0")
    spec = UNetSpec(1, 64, 3, 3)
    blob = pack_weights(spec, synth.make_weights(spec, 8))
    imgs = synth.make_images(3, 512, 512, 1, 0x7A11, "blobs")
    with binding.Engine(512, 512, 1, 64, 3, 3, max_batch=2, conv_algo=algo) as eng:
        eng.load_weights(blob)
        eng.set_profiling(True)
        lab3, lg3 = eng.infer(imgs, want_logits=True)                  # micro-batches of 2 and 1
        used3 = [(s["name"], s["kernel"]) for s in eng.kernel_stats()]
        eng.set_profiling(False)
        lab2, lg2 = eng.infer(imgs[[2, 0]], want_logits=True)          # the same image as the first of a pair
    n = [name for name, _ in used3].index(used3[-1][0]) + 1             # the first micro-batch ends with the plan's last launch
    pair, alone = dict(used3[:n]), dict(used3[n:])
    assert set(pair) == set(alone) and any(pair[k] != alone[k] for k in pair), "the tail micro-batch was expected to route differently"
    assert np.array_equal(lg3[2], lg2[0]) and np.array_equal(lab3[2], lab2[0])


def test_fused_first_layer_gives_the_unfused_bits_at_config5_size(monkeypatch):
    """BASELINE config 5's shape (1024 x 1024 x 3, base 32, five levels, batch 8): inc.c1 inside inc.c2's launch (conv3x3_lpr FIRST:
    fp32 MFMAs threaded between the conv's MFMA steps, window bytes by LDS-DMA) against inc.c1 as a launch of its own
    (MIUNET_FUSE_FIRST=0) -- same instruction, same K order: the logits are the same bits, on interior and border tiles alike."""
    spec = UNetSpec(in_ch=3, base=32, levels=5)
    blob = pack_weights(spec, synth.make_weights(spec, 77))
    imgs = synth.make_images(8, 1024, 1024, 3, 5, "blobs")
    out, fused = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MIUNET_FUSE_FIRST", mode)
        with binding.Engine(1024, 1024, in_ch=3, base=32, levels=5, classes=3, max_batch=8, conv_algo="fp16") as eng:
            eng.load_weights(blob)
            eng.set_profiling(True)
            out[mode] = eng.infer(imgs, want_logits=True)
            fused[mode] = [s["kernel"] for s in eng.kernel_stats() if s["kernel"].endswith("+first")]
    assert fused["0"] == [] and fused["1"] == ["conv3x3_fp16r+first"]
    assert np.array_equal(out["0"][1].view(np.uint32), out["1"][1].view(np.uint32)) and np.array_equal(out["0"][0], out["1"][0])


# ---------------------------------------------------------------- the large transposed convolutions with resident weights (convt_lpr.hip)
@pytest.mark.parametrize("op,B,H,W,Cin,Cout", [
    ("convT2x2_bf16", 1, 8, 32, 64, 32),        # exactly one 8 x 32 tile: wave = tap x half of the row blocks
    ("convT2x2_fp16", 2, 9, 40, 64, 32),        # ragged in x and y
    ("convT2x2_bf16", 1, 8, 64, 128, 64),       # 4 x 32 tiles, two channel blocks per wave
    ("convT2x2_fp16", 1, 5, 33, 128, 64),
    ("convT2x2_bf16", 1, 6, 32, 256, 128),      # 2 x 32 tiles, wave = tap x half of the channels
    ("convT2x2_fp16", 3, 3, 70, 256, 128),
])
def test_convT_resident_weights(op, B, H, W, Cin, Cout):
    """Same products and accumulation order as the one-tile-per-workgroup kernel: its 16-bit tensor bit for bit, within one
    16-bit rounding of the rounded-operand oracle."""
    r = np.random.default_rng(5 * B + H + 3 * W + Cin + Cout)
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cin, Cout, 2, 2), dtype=np.float32) / np.sqrt(Cin)).astype(np.float32)
    bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    rnd = orc.bf16_round if op.endswith("bf16") else orc.fp16_round
    got16 = binding.layer_debug(op + "r_lpout", x, w, None, bias)
    assert not np.isnan(got16).any(), "unwritten (NaN-poisoned) outputs"
    assert np.array_equal(got16, binding.layer_debug(op + "_lpout", x, w, None, bias))
    ref = orc.convT2x2(rnd(x), rnd(w), bias)
    ulp = 2.0 ** -7 if op.endswith("bf16") else 2.0 ** -10
    assert np.max(np.abs(got16 - ref) / np.maximum(1.0, np.abs(ref))) < ulp


@pytest.mark.parametrize("op,Cin,Cout,H,W", [("convT2x2_bf16", 128, 64, 256, 256), ("convT2x2_fp16", 64, 32, 512, 256), ("convT2x2_bf16", 256, 128, 128, 128)])
def test_convT_resident_weights_many_tiles_per_workgroup(op, Cin, Cout, H, W):
    """Thousands of tiles on 256 persistent workgroups: the three-deep tile ring wraps, every wait and barrier of the steady
    state runs; three runs (a race would not show every time), compared with the one-tile-per-workgroup kernel bit for bit."""
    r = np.random.default_rng(Cin + Cout)
    x = r.standard_normal((4, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cin, Cout, 2, 2), dtype=np.float32) / np.sqrt(Cin)).astype(np.float32)
    bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    ref = binding.layer_debug(op + "_lpout", x, w, None, bias)
    for _ in range(3):
        got16 = binding.layer_debug(op + "r_lpout", x, w, None, bias)
        assert not np.isnan(got16).any()
        assert np.array_equal(got16, ref)


@pytest.mark.parametrize("algo", ["bf16", "fp16"])
def test_resident_weight_convT_in_the_whole_network(algo, monkeypatch):
    """base 32, three levels: up1.t (256 -> 128), up2.t (128 -> 64) and up3.t (64 -> 32) are the three shapes of convt_lpr.hip,
    writing the upper halves of the concat buffers.  MIUNET_CONVT_LPR=2 sends them there whatever the grid, =0 nowhere."""
    spec = UNetSpec(1, 32, 3, 3)
    blob = pack_weights(spec, synth.make_weights(spec, 78))
    imgs = synth.make_images(3, 96, 80, 1, 0x52, "blobs")
    out, used = {}, {}
    for mode in ("0", "2"):
        monkeypatch.setenv("MIUNET_CONVT_LPR", mode)
        with binding.Engine(96, 80, 1, 32, 3, 3, max_batch=3, conv_algo=algo) as eng:
            eng.load_weights(blob)
            eng.set_profiling(True)
            out[mode] = eng.infer(imgs, want_logits=True)
            used[mode] = [s["kernel"] for s in eng.kernel_stats() if s["kernel"].startswith("convT") and s["kernel"].endswith("r")]
    assert used["0"] == [] and used["2"] == [f"convT2x2_{algo}r"] * 3
    assert np.array_equal(out["0"][1], out["2"][1]) and np.array_equal(out["0"][0], out["2"][0])


@pytest.mark.parametrize("seed", range(12))
def test_resident_weight_kernels_random_shapes(seed):
    """Random batch / height / width (odd sizes, tiles past both image edges, tile counts that are no multiple of 8) for every
    shape the resident-weight kernels take: 3x3 conv, its fused pooling (even sizes) and the transposed conv, each bit-identical
    to the one-tile-per-workgroup kernel.  The tile counts stay below the persistent grid (about 100 tiles at the most on 256
    compute units), so every workgroup takes one tile here: tile counts the grid does not divide are the subject of
    test_gpu_persistent_walk.py."""
    r = np.random.default_rng(1000 + seed)
    kind = ("conv", "pool", "convT")[seed % 3]
    fp16 = bool(r.integers(0, 2))
    sfx = "fp16" if fp16 else "bf16"
    B = int(r.integers(1, 4))
    if kind == "convT":
        Cin, Cout = [(64, 32), (128, 64), (256, 128)][int(r.integers(0, 3))]
        H, W = int(r.integers(1, 40)), int(r.integers(1, 100))
        x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
        w = (r.standard_normal((Cin, Cout, 2, 2), dtype=np.float32) / np.sqrt(Cin)).astype(np.float32)
        bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
        got = binding.layer_debug(f"convT2x2_{sfx}r_lpout", x, w, None, bias)
        ref = binding.layer_debug(f"convT2x2_{sfx}_lpout", x, w, None, bias)
    else:
        Cin, Cout = [(32, 32), (32, 64), (64, 32), (64, 64)][int(r.integers(0, 4))]
        H, W = int(r.integers(1, 60)), int(r.integers(1, 140))
        if kind == "pool":
            H, W = 2 * ((H + 1) // 2), 2 * ((W + 1) // 2)
        x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
        w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
        shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
        op = "_pool_lpout" if kind == "pool" else "_lpout"
        got = binding.layer_debug(f"conv3x3_{sfx}r{op}", x, w, None, shift, relu=True)
        ref = binding.layer_debug(f"conv3x3_{sfx}{op}", x, w, None, shift, relu=True)
    assert not np.isnan(got).any(), (kind, B, H, W, Cin, Cout)
    assert np.array_equal(got, ref), (kind, B, H, W, Cin, Cout)
