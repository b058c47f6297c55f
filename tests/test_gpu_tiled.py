"""Tiled inference on the device (mi_unet_infer_tiled_u8 / _raw16, mi_unet_segment_tiled_raw16): one image larger than the
engine's tile, cut into overlapping tiles (csrc/tiles.hip: gather), run through the network in tile order, stitched on the device
(each pixel from the tile that owns it) and only then postprocessed / traced at full size.

The expected results are built here with numpy from the grid definition restated in test_tiled_cpu.grid: tiles cut with slices,
the oracle (or mi_unet_infer_u8) per tile, owned rectangles copied by the cuts.

Oracle parity, low-margin pixels: a label may differ from the oracle's only where the oracle's top-2 margin is <= 1e-3, and such
pixels may be at most 0.2 % of the image.  The oracle alone gives 0.022 - 0.052 % on the four small inputs below and 0.034 % on the
1100 x 700 one (each test prints its figure), so the reference meets the cap with room."""
import ctypes

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_gpu_unet import LOGIT_TOL, check_parity
from test_tiled_cpu import grid

pytestmark = pytest.mark.gpu

EARG, ESTATE = 1, 5


def cut_tiles(img, th, tw, halo):
    """img [H,W,C] -> tiles [nt,th,tw,C] in tile order (row-major)"""
    oy, _ = grid(img.shape[0], th, halo)
    ox, _ = grid(img.shape[1], tw, halo)
    return np.stack([img[y:y + th, x:x + tw] for y in oy for x in ox])


def stitch(per_tile, H, W, th, tw, halo):
    """per_tile [nt,...,th,tw] -> [...,H,W]: every pixel from the tile that owns it"""
    oy, cy = grid(H, th, halo)
    ox, cx = grid(W, tw, halo)
    out = np.zeros(per_tile.shape[1:-2] + (H, W), per_tile.dtype)
    written = np.zeros((H, W), np.int32)
    for ty in range(len(oy)):
        for tx in range(len(ox)):
            t = ty * len(ox) + tx
            ys, xs = slice(cy[ty], cy[ty + 1]), slice(cx[tx], cx[tx + 1])
            out[..., ys, xs] = per_tile[t][..., cy[ty] - oy[ty]:cy[ty + 1] - oy[ty], cx[tx] - ox[tx]:cx[tx + 1] - ox[tx]]
            written[ys, xs] += 1
    assert (written == 1).all()
    return out


def small_net(in_ch=1, up="transpose", base=16):
    spec = UNetSpec(in_ch=in_ch, base=base, levels=3, up=up)
    return spec, pack_weights(spec, synth.make_weights(spec, 1234))


def oracle_tiled(blob, img, th, tw, halo):
    H, W = img.shape[:2]
    ref_logits, _ = orc.unet_forward(blob, cut_tiles(img, th, tw, halo))
    return stitch(ref_logits, H, W, th, tw, halo)


def parity_and_margin(labels, logits, ref_logits):
    err = float(np.max(np.abs(logits - ref_logits)))
    srt = np.sort(ref_logits, axis=0)
    low = float(((srt[-1] - srt[-2]) <= LOGIT_TOL).mean())
    n_bad = check_parity(labels[None], logits[None], ref_logits[None])
    print(f"max |logit - oracle| = {err:.3e}, label mismatches = {n_bad}, oracle low-margin pixels = {100 * low:.4f} %")
    assert low <= 0.002


@pytest.mark.parametrize("kind", ["blobs", "bytes"])
@pytest.mark.parametrize("max_batch", [16, 5])
@pytest.mark.parametrize("th,tw,H,W,halo", [(40, 24, 100, 72, 4), (64, 64, 200, 136, 8)])
def test_tiled_matches_the_oracle_per_tile_and_stitched(th, tw, H, W, halo, max_batch, kind):
    """12 tiles each; max_batch 5 ends micro-batches in the middle of a tile row"""
    spec, blob = small_net()
    img = synth.make_images(1, H, W, 1, 0x5EED, kind)[0]
    assert len(grid(H, th, halo)[0]) * len(grid(W, tw, halo)[0]) == 12
    with binding.Engine(th, tw, base=16, levels=3, max_batch=max_batch) as eng:
        eng.load_weights(blob)
        labels, logits = eng.infer_tiled(img, halo, want_logits=True)
        labels_only, none = eng.infer_tiled(img, halo)
    assert none is None and labels.shape == (H, W) and logits.shape == (3, H, W)
    parity_and_margin(labels, logits, oracle_tiled(blob, img, th, tw, halo))
    assert np.array_equal(labels_only, labels)


def test_tiled_matches_the_oracle_at_the_real_size():
    """the default engine (512 x 512, base 64, 4 levels), one 1100 x 700 image, halo 32: 3 x 2 tiles"""
    spec = UNetSpec()
    blob = pack_weights(spec, synth.make_weights(spec, 1234))
    H, W, halo = 1100, 700, 32
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    assert (len(grid(H, 512, halo)[0]), len(grid(W, 512, halo)[0])) == (3, 2)
    with binding.Engine() as eng:
        eng.load_weights(blob)
        labels, logits = eng.infer_tiled(img, halo, want_logits=True)
    parity_and_margin(labels, logits, oracle_tiled(blob, img, 512, 512, halo))


def test_one_tile_is_infer_u8():
    """H x W == tile: labels and logits bit-identical to mi_unet_infer_u8; a clone owns its own full-size buffers"""
    spec, blob = small_net()
    img = synth.make_images(1, 64, 48, 1, 0x5EED, "blobs")
    with binding.Engine(64, 48, base=16, levels=3, max_batch=2) as eng:
        eng.load_weights(blob)
        want_labels, want_logits = eng.infer(img, want_logits=True)
        for halo in (0, 7, 23):
            labels, logits = eng.infer_tiled(img[0], halo, want_logits=True)
            assert np.array_equal(labels, want_labels[0]) and np.array_equal(logits, want_logits[0])
        with eng.clone() as twin:
            labels, logits = twin.infer_tiled(img[0], 5, want_logits=True)
        assert np.array_equal(labels, want_labels[0]) and np.array_equal(logits, want_logits[0])


@pytest.mark.parametrize("variant", ["fp32", "bilinear", "bf16", "rgb"])
@pytest.mark.parametrize("th,tw,H,W,halo,max_batch", [(64, 64, 200, 144, 8, 5), (40, 24, 100, 72, 4, 16), (32, 32, 77, 99, 5, 4),
                                                      (32, 64, 32, 128, 0, 2)])
def test_tiled_is_infer_u8_on_the_stacked_tiles_then_stitched(th, tw, H, W, halo, max_batch, variant):
    """bit for bit, on any grid: image widths that are multiples of 16, of 4 and odd (the three store widths of the stitch), the
    bilinear decoder and the bf16 pipeline (which the C oracle cannot run), three input channels; halo 0 with W = 2 tile widths
    is the two halves side by side"""
    in_ch = 3 if variant == "rgb" else 1
    base = 32 if variant == "bf16" else 16
    spec, blob = small_net(in_ch, "bilinear" if variant == "bilinear" else "transpose", base)
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    if in_ch == 3:
        img = np.concatenate([img, synth.make_images(2, H, W, 1, 0xBEEF, "bytes")[:, :, :, 0].transpose(1, 2, 0)], axis=2)
    with binding.Engine(th, tw, in_ch=in_ch, base=base, levels=3, max_batch=max_batch, conv_algo="bf16" if variant == "bf16" else "auto") as eng:
        eng.load_weights(blob)
        tiles = cut_tiles(img, th, tw, halo)
        tile_labels, tile_logits = eng.infer(tiles, want_logits=True)
        labels, logits = eng.infer_tiled(img, halo, want_logits=True)
        again, _ = eng.infer_tiled(img, halo)                                 # graphs replay by now; no logits this time
    assert np.array_equal(labels, stitch(tile_labels, H, W, th, tw, halo))
    assert np.array_equal(logits, stitch(tile_logits, H, W, th, tw, halo))
    assert np.array_equal(again, labels)
    if halo == 0 and W == 2 * tw and H == th:
        assert np.array_equal(labels, np.concatenate([tile_labels[0], tile_labels[1]], axis=1))


def test_raw_form_normalises_at_full_size_like_the_oracle():
    """norm = preprocess_raw at out size == image size, byte for byte (including mn == mx, a 65535 maximum and a pixel count that
    is not a multiple of 8); labels = infer_tiled of those bytes"""
    spec, blob = small_net()
    raws = {"detector": synth.make_raw16(100, 72, seed=21), "constant": np.full((100, 72), 7, np.uint16),
            "constant_max": np.full((64, 48), 65535, np.uint16), "odd": synth.make_raw16(77, 99, seed=5, lo=0, hi=65535)}
    raws["odd"][0, 0] = 65535
    raws["full_range"] = synth.make_raw16(96, 80, seed=9)
    raws["full_range"][3, 5] = 65535
    raws["full_range"][90, 2] = 0
    with binding.Engine(40, 24, base=16, levels=3, max_batch=5) as eng:
        eng.load_weights(blob)
        for name, raw in raws.items():
            H, W = raw.shape
            norm, labels, logits = eng.infer_tiled_raw16(raw, 4, want_logits=True)
            want = orc.preprocess_raw(raw, out_w=W, out_h=H)
            assert norm.shape == (H, W) and np.array_equal(norm, want), name
            want_labels, want_logits = eng.infer_tiled(want, 4, want_logits=True)
            assert np.array_equal(labels, want_labels) and np.array_equal(logits, want_logits), name
            none, labels2, _ = eng.infer_tiled_raw16(raw, 4, want_norm=False)
            assert none is None and np.array_equal(labels2, labels)
        assert raws["odd"].max() == 65535 and raws["full_range"].max() == 65535


def test_raw_form_three_planes():
    """in_ch = 3: every plane has its own min / max and becomes one channel of the interleaved image; one array for all three"""
    spec, blob = small_net(3)
    H, W = 90, 70
    planes = [synth.make_raw16(H, W, seed=3), synth.make_raw16(H, W, seed=4, lo=1000, hi=60000), np.full((H, W), 300, np.uint16)]
    with binding.Engine(40, 24, in_ch=3, base=16, levels=3, max_batch=16) as eng:
        eng.load_weights(blob)
        norm, labels, _ = eng.infer_tiled_raw16(planes, 4)
        assert norm.shape == (H, W, 3)
        for c in range(3):
            assert np.array_equal(norm[:, :, c], orc.preprocess_raw(planes[c], out_w=W, out_h=H)), c
        assert np.array_equal(labels, eng.infer_tiled(norm, 4)[0])
        norm1, labels1, _ = eng.infer_tiled_raw16(planes[0], 4)                # the grey -> three channels replication
        assert all(np.array_equal(norm1[:, :, c], norm[:, :, 0]) for c in range(3))
        assert np.array_equal(labels1, eng.infer_tiled(norm1, 4)[0])


def _segment_scene():
    """192 x 160 RAW image for 64 x 64 tiles with halo 8 (cuts at y = 56, 104, 144 and x = 56, 104).  Values 0 / 28270 / 65535
    normalise to 0 / 110 / 255, which the threshold net labels 0 / 1 / 2."""
    H, W = 192, 160
    fg = np.zeros((H, W), bool)
    fg[20:50, 10:150] = True               # 4200 pixels across all three tile columns: more than 6 % of the image (1843)
    fg[50:80, 60:66] = True                # an arm of it across the cut y = 56: 144 pixels inside tile (1, 1), less than 6 % of a tile (245)
    fg[30:36, 40:46] = False               # a hole, filled
    fg[120:130, 20:30] = True              # 100 pixels on their own: removed
    fg[100:170, 90:150] = True             # a second component, across cuts in both directions
    raw = np.where(fg, 65535, 0).astype(np.uint16)
    raw[175:185, 5:60] = 28270             # label 1
    return raw, fg


def test_segment_form_postprocesses_and_traces_the_stitched_image():
    spec = UNetSpec(base=16, levels=2)
    blob = pack_weights(spec, synth.make_threshold_weights(spec))
    raw, fg = _segment_scene()
    H, W = raw.shape
    want_labels = np.where(fg, 2, 0).astype(np.uint8)
    want_labels[175:185, 5:60] = 1
    want_post = orc.postprocess_mask(want_labels)
    want_vis = orc.mask_to_image(want_post)
    want_cont = orc.find_contours(want_vis)
    assert want_vis[60:78, 61:65].min() == 255           # the arm survives: the area rule saw the whole component
    assert want_vis[120:130, 20:30].max() == 0 and want_vis[30:36, 40:46].min() == 255 and len(want_cont) == 2
    with binding.Engine(64, 64, base=16, levels=2, max_batch=5) as eng:
        eng.load_weights(blob)
        norm, labels, _ = eng.infer_tiled_raw16(raw, 8)
        assert np.array_equal(norm, orc.preprocess_raw(raw, out_w=W, out_h=H)) and np.array_equal(labels, want_labels)
        norm, mask, cont = eng.segment_tiled_raw16(raw, 8)
        stages = eng.last_stage_ms()
        assert np.array_equal(mask, want_vis) and cont == want_cont
        assert all(v >= 0.0 for v in stages.values()) and stages["upload_preprocess"] > 0 and stages["network"] > 0
        assert stages["postprocess"] > 0 and stages["contours"] > 0
        _, mask, cont = eng.segment_tiled_raw16(raw, 8, cap_points=4, want_norm=False)          # capacity too small: no fault
        assert cont is None and np.array_equal(mask, want_vis)
        _, mask, cont = eng.segment_tiled_raw16(raw, 8, cap_contours=1, want_norm=False)
        assert cont is None
        eng.set_postprocess(True)                                                              # the flag, on the stitched image
        assert np.array_equal(eng.infer_tiled(norm, 8)[0], want_post)
        assert np.array_equal(eng.infer_tiled_raw16(raw, 8)[1], want_post)
        eng.set_postprocess(False)
        assert np.array_equal(eng.infer_tiled(norm, 8)[0], want_labels)


def test_kernel_stats_name_the_three_kernels():
    spec, blob = small_net()
    raw = synth.make_raw16(100, 72, seed=21)
    with binding.Engine(40, 24, base=16, levels=3, max_batch=5) as eng:
        eng.load_weights(blob)
        eng.infer_tiled_raw16(raw, 4, want_logits=True)
        eng.set_profiling(True)
        eng.infer_tiled_raw16(raw, 4, want_logits=True)
        stats = eng.kernel_stats()
        eng.set_profiling(False)
    by_kernel = {}
    for s in stats:
        by_kernel.setdefault(s["kernel"], []).append(s)
    assert len(by_kernel["normalise_u16"]) == 1 and len(by_kernel["tile_gather"]) == 3 and len(by_kernel["tile_stitch"]) == 3
    assert by_kernel["normalise_u16"][0]["bytes"] == 3 * 100 * 72
    assert sum(s["bytes"] for s in by_kernel["tile_gather"]) == 2 * 12 * 40 * 24
    assert sum(s["bytes"] for s in by_kernel["tile_stitch"]) == 2 * 100 * 72 * (1 + 4 * 3)     # every pixel once: u8 label + 3 fp32 logits
    assert all(s["ms"] > 0 for k in ("normalise_u16", "tile_gather", "tile_stitch") for s in by_kernel[k])


def test_errors_leave_the_handle_usable():
    spec, blob = small_net()
    img = synth.make_images(1, 100, 72, 1, 0x5EED, "blobs")[0]
    L = binding.lib()
    with binding.Engine(40, 24, base=16, levels=3, max_batch=1) as eng:
        with pytest.raises(binding.MiUnetError) as ei:
            eng.infer_tiled(img, 4)
        assert ei.value.code == ESTATE
        eng.load_weights(blob)
        good = eng.infer_tiled(img, 4)[0]
        for bad_img, halo in ((img[:39], 4), (img[:, :23], 4), (img, -1), (img, 12), (img, 500)):
            with pytest.raises(binding.MiUnetError) as ei:
                eng.infer_tiled(bad_img, halo)
            assert ei.value.code == EARG and str(ei.value)
            assert np.array_equal(eng.infer_tiled(img, 4)[0], good)
        labels = np.empty((100, 72), np.uint8)
        raw = np.zeros((100, 72), np.uint16)
        planes = (ctypes.c_void_p * 1)(raw.ctypes.data)
        null_plane = (ctypes.c_void_p * 1)(None)
        cnt = ctypes.c_int32(0)
        i32 = np.zeros(64, np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert L.mi_unet_infer_tiled_u8(eng._h, None, 100, 72, 4, p(labels), None) == EARG
        assert L.mi_unet_infer_tiled_u8(eng._h, p(img), 100, 72, 4, None, None) == EARG
        assert L.mi_unet_infer_tiled_raw16(eng._h, None, 72, 100, 4, None, p(labels), None) == EARG
        assert L.mi_unet_infer_tiled_raw16(eng._h, null_plane, 72, 100, 4, None, p(labels), None) == EARG
        assert L.mi_unet_infer_tiled_raw16(eng._h, planes, 72, 100, 4, None, None, None) == EARG
        assert L.mi_unet_infer_tiled_raw16(eng._h, planes, 23, 100, 4, None, p(labels), None) == EARG
        assert L.mi_unet_segment_tiled_raw16(eng._h, planes, 72, 100, 4, None, None, p(i32), 8, p(i32), 8, ctypes.byref(cnt)) == EARG
        assert L.mi_unet_segment_tiled_raw16(eng._h, planes, 72, 100, 4, None, p(labels), p(i32), 0, p(i32), 8, ctypes.byref(cnt)) == EARG
        assert L.mi_unet_segment_tiled_raw16(eng._h, planes, 72, 100, 4, None, p(labels), p(i32), 8, None, 8, ctypes.byref(cnt)) == EARG
        # the full-size tail borrows the network's scratch buffer (4 * 1 * 40 * 24 * 16 = 61440 bytes here): a 100 x 72 image needs
        # 27 bytes per pixel = 194400 for postprocess_mask -- refused before anything runs, with both numbers
        eng.set_postprocess(True)
        with pytest.raises(binding.MiUnetError) as ei:
            eng.infer_tiled(img, 4)
        assert ei.value.code == EARG and "194400" in str(ei.value) and "61440" in str(ei.value)
        with pytest.raises(binding.MiUnetError) as ei:
            eng.segment_tiled_raw16(raw, 4)
        assert ei.value.code == EARG
        eng.set_postprocess(False)
        assert np.array_equal(eng.infer_tiled(img, 4)[0], good)
