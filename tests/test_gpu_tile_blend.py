"""Tile blending and mirror averaging on the device (mi_unet_set_tile_blend; csrc/tiles.hip: mirrored gather, csrc/blend.hip:
tile_blend, blend_finalize).  The definition is the one in include/mi_unet.h, restated here in numpy:

  views   k = t * nv + v: identity, X (mirror & 1), Y (mirror & 2), XY (mirror == 3), each the tile cut at its origin and mirrored;
  weights w = fl32(wy[Y - oy] * wx[X - ox]) from the tables of test_tile_blend_cpu.weight_table (OWNER: 1, owning tile only);
  sum     acc = fl32(acc + fl32(w * logit)), wsum = fl32(wsum + w), per pixel in increasing k;  logit = acc / wsum;
  label   first-max-wins argmax.

Bit identity: the views are cut and mirrored on the host and run through mi_unet_infer_u8 on the same engine (the same
micro-batches as the tiled call), then blended in numpy float32 in that order.

Oracle parity: the C oracle on the same views, blended in float64.  A blended logit is a convex combination of per-view logits, each
within LOGIT_TOL = 1e-3 of the oracle's (the per-tile bar), and the float32 blend adds a few ulps of |logit|, so the bar stays 1e-3.
A label may differ from the oracle's only where the oracle's top-2 margin is <= 1e-3, and such pixels may be at most 0.2 % of the
image (the cap of test_gpu_tiled.py); each case prints its figure."""
import ctypes

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_gpu_tiled import _segment_scene, parity_and_margin, small_net
from test_tile_blend_cpu import views, weight_table
from test_tiled_cpu import grid

pytestmark = pytest.mark.gpu

EARG = 1
SETTINGS = [(m, s, r) for m, s in (("constant", 0.125), ("gaussian", 0.125), ("gaussian", 0.25)) for r in ("", "x", "y", "xy")]
SETTINGS.append(("owner", 0.125, "xy"))
MIRROR = {"": 0, "x": 1, "y": 2, "xy": 3}


def cut_views(img, th, tw, halo, mirror):
    """img [H,W(,C)] -> view images [nt * nv, th, tw(,C)] in k order"""
    oy, _ = grid(img.shape[0], th, halo)
    ox, _ = grid(img.shape[1], tw, halo)
    out = []
    for y in oy:
        for x in ox:
            t = img[y:y + th, x:x + tw]
            for fy, fx in views(MIRROR[mirror]):
                a = t[::-1] if fy else t
                out.append(np.ascontiguousarray(a[:, ::-1] if fx else a))
    return np.stack(out)


def _unmirrored(view_logits, mirror):
    """per-view logits [nk, classes, th, tw] -> (k, logits in tile orientation) in k order"""
    vs = views(MIRROR[mirror])
    for k in range(view_logits.shape[0]):
        fy, fx = vs[k % len(vs)]
        lg = view_logits[k]
        lg = lg[:, ::-1] if fy else lg
        yield k, (lg[:, :, ::-1] if fx else lg)


def _regions(H, W, th, tw, halo, mode, nv):
    """per k: (rows, cols) slices of the image that view k contributes to and the matching slices of the tile"""
    oy, cy = grid(H, th, halo)
    ox, cx = grid(W, tw, halo)
    out = []
    for ty in range(len(oy)):
        for tx in range(len(ox)):
            if mode == "owner":
                ys, xs = slice(cy[ty], cy[ty + 1]), slice(cx[tx], cx[tx + 1])
            else:
                ys, xs = slice(oy[ty], oy[ty] + th), slice(ox[tx], ox[tx] + tw)
            ts = (slice(ys.start - oy[ty], ys.stop - oy[ty]), slice(xs.start - ox[tx], xs.stop - ox[tx]))
            out += [((ys, xs), ts)] * nv
    return out


def first_max_argmax(logits):
    """[classes, H, W] -> labels: strict '>' from -FLT_MAX in class order (head_argmax_kernel, the oracle)"""
    best = np.full(logits.shape[1:], np.float32(-3.402823466e+38), np.float32)
    idx = np.zeros(logits.shape[1:], np.uint8)
    for c in range(logits.shape[0]):
        up = logits[c] > best
        best = np.where(up, logits[c], best)
        idx[up] = c
    return idx


def blend_f32(view_logits, H, W, th, tw, halo, mode, sigma, mirror):
    """the definition, operation for operation in float32"""
    classes = view_logits.shape[1]
    nv = len(views(MIRROR[mirror]))
    w2 = (weight_table(th, mode, sigma)[:, None] * weight_table(tw, mode, sigma)[None, :]).astype(np.float32)
    if mode == "owner":
        w2 = np.ones((th, tw), np.float32)
    acc = np.zeros((classes, H, W), np.float32)
    wsum = np.zeros((H, W), np.float32)
    regions = _regions(H, W, th, tw, halo, mode, nv)
    for k, lg in _unmirrored(view_logits, mirror):
        (ys, xs), (ti, tj) = regions[k]
        w = w2[ti, tj]
        acc[:, ys, xs] = acc[:, ys, xs] + (w[None] * lg[:, ti, tj]).astype(np.float32)
        wsum[ys, xs] = wsum[ys, xs] + w
    assert (wsum > 0).all()
    logits = (acc / wsum[None]).astype(np.float32)
    return first_max_argmax(logits), logits


def blend_f64(view_logits, H, W, th, tw, halo, mode, sigma, mirror):
    """the same weights, the sum in float64: the oracle side"""
    classes = view_logits.shape[1]
    nv = len(views(MIRROR[mirror]))
    w2 = (weight_table(th, mode, sigma)[:, None] * weight_table(tw, mode, sigma)[None, :]).astype(np.float32).astype(np.float64)
    acc = np.zeros((classes, H, W), np.float64)
    wsum = np.zeros((H, W), np.float64)
    regions = _regions(H, W, th, tw, halo, mode, nv)
    for k, lg in _unmirrored(view_logits, mirror):
        (ys, xs), (ti, tj) = regions[k]
        acc[:, ys, xs] += w2[ti, tj][None] * lg[:, ti, tj].astype(np.float64)
        wsum[ys, xs] += w2[ti, tj]
    return acc / wsum[None]


@pytest.mark.parametrize("variant", ["fp32", "bilinear", "bf16", "rgb"])
@pytest.mark.parametrize("th,tw,H,W,halo,max_batch", [(64, 64, 200, 144, 8, 5), (40, 24, 100, 72, 4, 16), (32, 32, 77, 99, 5, 4),
                                                      (32, 64, 32, 128, 0, 2)])
def test_blend_is_infer_u8_on_the_views_then_blended(th, tw, H, W, halo, max_batch, variant):
    """bit for bit, every mode and mirror setting, on the grids and network variants of test_gpu_tiled.py; the repeated call replays
    the captured graphs"""
    in_ch = 3 if variant == "rgb" else 1
    base = 32 if variant == "bf16" else 16
    spec, blob = small_net(in_ch, "bilinear" if variant == "bilinear" else "transpose", base)
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    if in_ch == 3:
        img = np.concatenate([img, synth.make_images(2, H, W, 1, 0xBEEF, "bytes")[:, :, :, 0].transpose(1, 2, 0)], axis=2)
    with binding.Engine(th, tw, in_ch=in_ch, base=base, levels=3, max_batch=max_batch, conv_algo="bf16" if variant == "bf16" else "auto") as eng:
        eng.load_weights(blob)
        owner_labels, owner_logits = eng.infer_tiled(img, halo, want_logits=True)
        n_differ = []
        for mode, sigma, mirror in SETTINGS:
            case = (mode, sigma, mirror)
            eng.set_tile_blend(mode, sigma, mirror)
            _, view_logits = eng.infer(cut_views(img, th, tw, halo, mirror), want_logits=True)
            want_labels, want_logits = blend_f32(view_logits, H, W, th, tw, halo, mode, sigma, mirror)
            labels, logits = eng.infer_tiled(img, halo, want_logits=True)
            assert labels.shape == (H, W) and logits.shape == (3, H, W), case
            assert np.array_equal(logits, want_logits), (case, float(np.max(np.abs(logits - want_logits))))
            assert np.array_equal(labels, want_labels), case
            again_labels, again_logits = eng.infer_tiled(img, halo, want_logits=True)
            assert np.array_equal(again_labels, labels) and np.array_equal(again_logits, logits), case
            assert np.array_equal(eng.infer_tiled(img, halo)[0], labels), case          # labels only: the same blend
            n_differ.append(int((logits != owner_logits).sum()))
        print("logits that differ from the ownership stitch, per setting:", n_differ)


def test_owner_without_mirror_is_unchanged():
    """the default is the ownership stitch: before any setting, after setting OWNER explicitly, after another mode and then NULL"""
    spec, blob = small_net()
    img = synth.make_images(1, 100, 72, 1, 0x5EED, "blobs")[0]
    L = binding.lib()
    with binding.Engine(40, 24, base=16, levels=3, max_batch=5) as eng:
        eng.load_weights(blob)
        assert eng.get_tile_blend() == {"mode": "owner", "sigma_scale": 0.125, "mirror": ""}
        labels, logits = eng.infer_tiled(img, 4, want_logits=True)
        eng.set_tile_blend("owner")
        assert eng.get_tile_blend() == {"mode": "owner", "sigma_scale": 0.125, "mirror": ""}
        l2, g2 = eng.infer_tiled(img, 4, want_logits=True)
        assert np.array_equal(l2, labels) and np.array_equal(g2, logits)
        eng.set_tile_blend("gaussian", 0.25, "xy")
        l3, g3 = eng.infer_tiled(img, 4, want_logits=True)
        assert not np.array_equal(g3, logits)
        assert L.mi_unet_set_tile_blend(eng._h, None) == 0
        assert eng.get_tile_blend() == {"mode": "owner", "sigma_scale": 0.125, "mirror": ""}
        l4, g4 = eng.infer_tiled(img, 4, want_logits=True)
        assert np.array_equal(l4, labels) and np.array_equal(g4, logits)
        eng.set_tile_blend("constant", 0.125, "x")
        eng.set_tile_blend(None)                                                # the binding's form of NULL
        l5, g5 = eng.infer_tiled(img, 4, want_logits=True)
        assert np.array_equal(l5, labels) and np.array_equal(g5, logits)


@pytest.mark.parametrize("kind", ["blobs", "bytes"])
@pytest.mark.parametrize("th,tw,H,W,halo", [(40, 24, 100, 72, 4), (64, 64, 200, 136, 8), (64, 64, 200, 136, 16), (32, 32, 77, 99, 5)])
def test_blend_matches_the_oracle(th, tw, H, W, halo, kind):
    spec, blob = small_net()
    img = synth.make_images(1, H, W, 1, 0x5EED, kind)[0]
    with binding.Engine(th, tw, base=16, levels=3, max_batch=5) as eng:
        eng.load_weights(blob)
        for mode in ("constant", "gaussian"):
            for mirror in ("", "xy"):
                eng.set_tile_blend(mode, 0.125, mirror)
                labels, logits = eng.infer_tiled(img, halo, want_logits=True)
                ref_logits, _ = orc.unet_forward(blob, cut_views(img, th, tw, halo, mirror))
                print(mode, mirror or "-", end=": ")
                parity_and_margin(labels, logits, blend_f64(ref_logits, H, W, th, tw, halo, mode, 0.125, mirror))


def test_blend_matches_the_oracle_at_the_real_size():
    """the default engine (512 x 512, base 64, 4 levels), one 1100 x 700 image, halo 32, Gaussian, no mirror"""
    spec = UNetSpec()
    blob = pack_weights(spec, synth.make_weights(spec, 1234))
    H, W, halo = 1100, 700, 32
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    with binding.Engine() as eng:
        eng.load_weights(blob)
        eng.set_tile_blend("gaussian", 0.125, "")
        labels, logits = eng.infer_tiled(img, halo, want_logits=True)
    ref_logits, _ = orc.unet_forward(blob, cut_views(img, 512, 512, halo, ""))
    parity_and_margin(labels, logits, blend_f64(ref_logits, H, W, 512, 512, halo, "gaussian", 0.125, ""))


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_mirror_averaging_is_mirror_equivariant(mode):
    """one tile (H = th, W = tw): mirroring the input mirrors the result, bit for bit (symmetric table, two-term sums commute, results
    independent of the batch position)"""
    spec, blob = small_net()
    img = synth.make_images(1, 40, 24, 1, 0x5EED, "blobs")[0]
    with binding.Engine(40, 24, base=16, levels=3, max_batch=2) as eng:
        eng.load_weights(blob)
        eng.set_tile_blend(mode, 0.125, "x")
        labels, logits = eng.infer_tiled(img, 4, want_logits=True)
        fl, fg = eng.infer_tiled(np.ascontiguousarray(img[:, ::-1]), 4, want_logits=True)
        assert np.array_equal(fl, labels[:, ::-1]) and np.array_equal(fg, logits[:, :, ::-1])
        eng.set_tile_blend(mode, 0.125, "y")
        labels, logits = eng.infer_tiled(img, 4, want_logits=True)
        fl, fg = eng.infer_tiled(np.ascontiguousarray(img[::-1]), 4, want_logits=True)
        assert np.array_equal(fl, labels[::-1]) and np.array_equal(fg, logits[:, ::-1])


def test_blend_composes_with_postprocess_and_contours():
    """Gaussian + xy on the RAW scene of test_gpu_tiled.py: the tail runs on the blended label map"""
    spec = UNetSpec(base=16, levels=2)
    blob = pack_weights(spec, synth.make_threshold_weights(spec))
    raw, _ = _segment_scene()
    H, W = raw.shape
    with binding.Engine(64, 64, base=16, levels=2, max_batch=5) as eng:
        eng.load_weights(blob)
        owner_labels = eng.infer_tiled_raw16(raw, 8)[1]
        eng.set_tile_blend("gaussian", 0.125, "xy")
        norm, labels, logits = eng.infer_tiled_raw16(raw, 8, want_logits=True)
        assert np.array_equal(norm, orc.preprocess_raw(raw, out_w=W, out_h=H))
        _, view_logits = eng.infer(cut_views(norm[:, :, None], 64, 64, 8, "xy"), want_logits=True)
        want_labels, want_logits = blend_f32(view_logits, H, W, 64, 64, 8, "gaussian", 0.125, "xy")
        assert np.array_equal(labels, want_labels) and np.array_equal(logits, want_logits)
        print("labels that differ from the ownership stitch:", int((labels != owner_labels).sum()))
        want_post = orc.postprocess_mask(labels)
        want_vis = orc.mask_to_image(want_post)
        want_cont = orc.find_contours(want_vis)
        assert want_vis.max() == 255 and len(want_cont) >= 1
        _, mask, cont = eng.segment_tiled_raw16(raw, 8)
        assert np.array_equal(mask, want_vis) and cont == want_cont
        eng.set_postprocess(True)
        assert np.array_equal(eng.infer_tiled_raw16(raw, 8)[1], want_post)
        assert np.array_equal(eng.infer_tiled(norm, 8)[0], want_post)


def test_errors_clones_and_kernel_stats():
    spec, blob = small_net()
    img = synth.make_images(1, 100, 72, 1, 0x5EED, "blobs")[0]
    L = binding.lib()
    H, W, th, tw, halo, Bm = 100, 72, 40, 24, 4, 5
    with binding.Engine(th, tw, base=16, levels=3, max_batch=Bm) as eng:
        eng.load_weights(blob)
        owner = eng.infer_tiled(img, halo, want_logits=True)
        eng.set_tile_blend("gaussian", 0.25, "y")
        before = eng.get_tile_blend()
        good = eng.infer_tiled(img, halo, want_logits=True)
        bad = [(3, 0.125, 0), (-1, 0.125, 0)] + [(2, s, 0) for s in (0.0, -1.0, float("nan"), float("inf"))] + [(1, 0.125, 4), (1, 0.125, -1)]
        for mode, sigma, mirror in bad:
            assert L.mi_unet_set_tile_blend(eng._h, ctypes.byref(binding.TileBlend(mode, sigma, mirror))) == EARG, (mode, sigma, mirror)
            assert str(L.mi_unet_last_error(), "utf-8")
            with pytest.raises(binding.MiUnetError) as ei:
                eng.set_tile_blend(mode, sigma, mirror)
            assert ei.value.code == EARG
            assert eng.get_tile_blend() == before
            again = eng.infer_tiled(img, halo, want_logits=True)
            assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
        with eng.clone() as twin:
            assert twin.get_tile_blend() == {"mode": "owner", "sigma_scale": 0.125, "mirror": ""}
            twin_labels, twin_logits = twin.infer_tiled(img, halo, want_logits=True)
            assert np.array_equal(twin_labels, owner[0]) and np.array_equal(twin_logits, owner[1])

        for mode, mirror in (("gaussian", "xy"), ("owner", "xy"), ("constant", "")):
            eng.set_tile_blend(mode, 0.125, mirror)
            eng.infer_tiled(img, halo, want_logits=True)                       # graphs captured, buffers grown
            eng.set_profiling(True)
            eng.infer_tiled(img, halo, want_logits=True)
            stats = eng.kernel_stats()
            eng.set_profiling(False)
            stages = eng.last_stage_ms()
            by_kernel = {}
            for s in stats:
                by_kernel.setdefault(s["kernel"], []).append(s)
            nv = len(views(MIRROR[mirror]))
            nk = 12 * nv
            n_mb = -(-nk // Bm)
            # coverage counted here: each view contributes to its whole tile, or (owner) to the rectangle its tile owns
            cover = np.zeros((H, W), np.int64)
            for (ys, xs), _ in _regions(H, W, th, tw, halo, mode, nv):
                cover[ys, xs] += 1
            assert "tile_stitch" not in by_kernel
            assert len(by_kernel["tile_gather"]) == n_mb and sum(s["bytes"] for s in by_kernel["tile_gather"]) == 2 * nk * th * tw
            assert len(by_kernel["tile_blend"]) == n_mb
            assert sum(s["bytes"] for s in by_kernel["tile_blend"]) == 12 * 3 * int(cover.sum())
            assert len(by_kernel["blend_finalize"]) == 1 and by_kernel["blend_finalize"][0]["bytes"] == H * W * (4 * 3 + 1 + 4 * 3)
            assert by_kernel["blend_finalize"][0]["name"] == "tiled.finalize"
            assert all(s["ms"] > 0 for k in ("tile_gather", "tile_blend", "blend_finalize") for s in by_kernel[k])
            assert stages["upload_preprocess"] > 0 and stages["network"] > 0
            print(mode, mirror or "-", {k: (len(v), sum(s["bytes"] for s in v), round(sum(s["ms"] for s in v), 4))
                                        for k, v in by_kernel.items() if k in ("tile_gather", "tile_blend", "blend_finalize")})
        # labels only: no logits written by the finalize
        eng.set_profiling(True)
        eng.infer_tiled(img, halo)
        stats = eng.kernel_stats()
        eng.set_profiling(False)
        fin = [s for s in stats if s["kernel"] == "blend_finalize"]
        assert len(fin) == 1 and fin[0]["bytes"] == H * W * (4 * 3 + 1)
