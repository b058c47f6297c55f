"""The bilinear decoder (Pytorch-UNet bilinear=True, weight-file version 2) on the GPU: the upsampling kernel against a float64
reference, every launched step of the bilinear plan in situ, the whole network against PyTorch on the CPU, the plan's
properties, and the facade.  The C oracle knows only the transposed net: the references here are numpy and torch CPU."""
import os
import struct
import zlib

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, hostlib, synth
from miunet.spec import HEADER, UNetSpec, pack_weights
from test_bilinear_cpu import PytorchUNet, load_spec_weights
from test_gpu_insitu import _fold, _ulp16

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _axis(n_in):
    """source taps and weights of one axis, in float32 as PyTorch's CPU kernel computes them (align_corners=True)"""
    n_out = 2 * n_in
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_in > 1 else np.float32(0)
    src = (np.float32(scale) * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def upsample_ref(x):
    """bilinear x2, align_corners=True, NHWC, accumulated in float64 on the float32 weights"""
    x = np.asarray(x, np.float64)
    y0, y1, a0, a1 = _axis(x.shape[1])
    x0, x1, b0, b1 = _axis(x.shape[2])
    a0, a1 = a0.astype(np.float64)[None, :, None, None], a1.astype(np.float64)[None, :, None, None]
    b0, b1 = b0.astype(np.float64)[None, None, :, None], b1.astype(np.float64)[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    return a0 * (b0 * r0[:, :, x0] + b1 * r0[:, :, x1]) + a1 * (b0 * r1[:, :, x0] + b1 * r1[:, :, x1])


def _check16(y, ref, rnd, mant, bar):
    """the stored 16-bit tensor is round16(reference), except rare boundary straddles within one ulp"""
    want = rnd(np.asarray(ref, np.float32))
    diff = np.abs(y - want)
    tol = np.maximum(_ulp16(np.maximum(np.abs(y), np.abs(want)), mant), np.float32(bar))
    assert np.all(diff <= tol), float(diff.max())
    frac = float(np.mean(diff > 0))
    assert frac < 5e-3, frac
    assert np.array_equal(rnd(y), y)
    return float(diff.max()), frac


@pytest.mark.parametrize("op", ["upsample2x", "upsample2x_bf16", "upsample2x_fp16"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (3, 2), (7, 5), (32, 32), (64, 128)])
@pytest.mark.parametrize("c", [16, 64, 512])
def test_upsample_layer(op, hw, c):
    rng = np.random.default_rng(zlib.crc32(repr((op, hw, c)).encode()))
    ys, refs, top = [], [], 1.0
    for b in (1, 3):
        x = (rng.standard_normal((b, hw[0], hw[1], c)) * 3.0).astype(np.float32)
        y = binding.layer_debug(op, x)
        assert y.shape == (b, 2 * hw[0], 2 * hw[1], c) and not np.isnan(y).any()
        if op == "upsample2x":
            err = float(np.max(np.abs(y - upsample_ref(x))))
            assert err <= 1e-6 * max(1.0, float(np.abs(x).max())), err
        else:
            rnd = orc.bf16_round if op.endswith("bf16") else orc.fp16_round
            ys.append(y.reshape(-1))
            refs.append(upsample_ref(rnd(x)).reshape(-1))
            top = max(top, float(np.abs(x).max()))
    if ys:
        # the straddle fraction over both batches of the case: interpolation weights of ninths, fifths, ... put exact results on
        # 16-bit rounding midpoints far more often than a random sum lands there (up to ~0.2 % of the elements); results that
        # cancel to near zero are held to the fp32 bar instead of their own (tiny) 16-bit ulp
        rnd, mant = (orc.bf16_round, 7) if op.endswith("bf16") else (orc.fp16_round, 10)
        _check16(np.concatenate(ys), np.concatenate(refs), rnd, mant, 1e-6 * top)


def test_upsample_corner_values_are_copies():
    """align_corners=True: the four corner pixels of the output are the input's, exactly (and a 1 x 1 input is replicated)"""
    x = np.random.default_rng(3).standard_normal((2, 5, 7, 32)).astype(np.float32)
    y = binding.layer_debug("upsample2x", x)
    for (yo, xo), (yi, xi) in (((0, 0), (0, 0)), ((0, -1), (0, -1)), ((-1, 0), (-1, 0)), ((-1, -1), (-1, -1))):
        assert np.array_equal(y[:, yo, xo], x[:, yi, xi])
    one = binding.layer_debug("upsample2x", x[:, :1, :1])
    assert np.array_equal(one, np.broadcast_to(x[:, :1, :1], one.shape))


def _engine(spec, size, batch, algo="auto", w=None):
    h, ww = size if isinstance(size, tuple) else (size, size)
    return binding.Engine(h, ww, in_ch=spec.in_ch, base=spec.base, levels=spec.levels, classes=spec.classes, max_batch=batch, conv_algo=algo)


@pytest.mark.parametrize("algo,spec,size,batch", [
    ("auto", UNetSpec(1, 64, 4, 3, up="bilinear"), 512, 16),
    ("bf16", UNetSpec(1, 64, 4, 3, up="bilinear"), 512, 16),
    ("fp16", UNetSpec(3, 32, 5, 3, up="bilinear"), 256, 4),
])
def test_every_step_in_situ(algo, spec, size, batch):
    """every launched step of the bilinear plan on its own device input (test_gpu_insitu.py's criteria), and the tensor each
    up{i}.c1 reads is [the skip as its producer stored it, the upsample's output], bit for bit"""
    tensors = synth.make_weights(spec, 11)
    blob = pack_weights(spec, tensors)
    img = 1
    imgs = synth.make_images(batch, size, size, spec.in_ch, 0x5EED + 11, "blobs")
    lp = algo in ("bf16", "fp16")
    rnd = orc.bf16_round if algo == "bf16" else orc.fp16_round if algo == "fp16" else (lambda a: a)
    mant = 7 if algo == "bf16" else 10
    L = spec.levels
    stored = {}
    with _engine(spec, size, batch, algo) as eng:
        eng.load_weights(blob)
        layers = eng.layers()
        assert not any(l["name"].endswith(".t") for l in layers)
        assert sum(l["kind"] == "upsample2x" for l in layers) == L
        launched = 0
        for i in range(len(layers)):
            d, x, y, pooled, lab = eng.capture(imgs, i, img)
            if d["skipped"]:
                continue
            launched += 1
            assert not np.isnan(y).any(), d
            name, kind = d["name"], d["kind"]
            x = x[None]
            if kind == "upsample2x":
                lvl = L - int(name[2:name.index(".")])
                assert d["kernel"] == "upsample2x_bilinear" and (d["in_h"], d["out_h"]) == (size >> (lvl + 1), size >> lvl)
                assert d["in_c"] == d["out_c"] == spec.base << lvl and d["in_bits"] == d["out_bits"] == (16 if lp else 32)
                ref = upsample_ref(x)[0]
                if lp:
                    assert np.array_equal(rnd(x), x)
                    _check16(y, ref, rnd, mant, 1e-6 * max(1.0, float(np.abs(x).max())))
                else:
                    assert float(np.max(np.abs(y - ref))) <= 1e-6 * max(1.0, float(np.abs(x).max()))
                stored[name] = y
                continue
            if kind == "first" or (kind == "conv3x3" and d["fused_first"]):
                assert not (lp and d["fused_first"])           # no 16-bit plan here fuses the first layer (in_ch 1, or too few tiles)
                w1, s1 = _fold(tensors, "inc", 1, spec.bn_eps)
                ref = np.maximum(orc.conv3x3(orc.normalize_u8(imgs[img][None]), w1) + s1, 0.0)
                if kind == "conv3x3":
                    w2, s2 = _fold(tensors, "inc", 2, spec.bn_eps)
                    ref = np.maximum(orc.conv3x3(ref, w2) + s2, 0.0)
                ref = ref[0]
            elif kind == "conv3x3":
                if name.endswith(".c1") and name.startswith("up"):
                    lvl = L - int(name[2:name.index(".")])
                    skip = stored["inc.c2" if lvl == 0 else f"down{lvl}.c2"]
                    assert np.array_equal(x[0], np.concatenate([skip, stored[name[:-3] + ".up"]], axis=-1)), name
                wf, shift = _fold(tensors, name[:-3], int(name[-1]), spec.bn_eps)
                if lp:
                    assert d["in_bits"] == 16 and np.array_equal(rnd(x), x)
                ref = np.maximum(orc.conv3x3(x, rnd(wf)) + shift, 0.0)[0]
            elif kind == "maxpool":
                assert np.array_equal(y, orc.maxpool2x2(x)[0])
                continue
            else:
                ref = None
            if kind == "head" or d["fused_head"]:
                act = x if kind == "head" else ref[None]
                ref_logits = orc.conv1x1_planar(act, tensors["outc.w"], tensors["outc.b"])[0]
                err = float(np.max(np.abs(y - ref_logits)))
                assert err <= 1e-4 * max(1.0, float(np.abs(ref_logits).max())), (name, d["kernel"], err)
                assert np.array_equal(lab, orc.argmax_planar(y)), name
                continue
            if d["out_bits"] == 16:
                _check16(y, ref, rnd, mant, 1e-4 * max(1.0, float(np.abs(ref).max())))
                if d["pooled"]:
                    assert np.array_equal(pooled, orc.maxpool2x2(y[None])[0]), name
            else:
                err = float(np.max(np.abs(y - ref)))
                assert err <= 1e-4 * max(1.0, float(np.abs(ref).max())), (name, d["kernel"], err)
                if d["pooled"]:
                    assert np.array_equal(pooled, orc.maxpool2x2(y[None])[0]), name
            stored[name] = y
        assert launched >= 5 * L + 1


def _torch_logits(spec, tensors, imgs):
    torch.backends.mkldnn.enabled = False
    torch.manual_seed(0)
    model = load_spec_weights(PytorchUNet(spec.in_ch, spec.classes, bilinear=True, base=spec.base, levels=spec.levels), spec, tensors).eval()
    x = torch.from_numpy(np.ascontiguousarray(imgs.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))
    with torch.no_grad():
        return model(x).numpy(), model


@pytest.mark.parametrize("algo", ["auto", "direct"])
@pytest.mark.parametrize("spec,hw,batch", [
    (UNetSpec(1, 16, 3, 3, up="bilinear"), (64, 64), 2),
    (UNetSpec(1, 64, 4, 3, up="bilinear"), (48, 80), 1),
    (UNetSpec(1, 64, 4, 3, up="bilinear"), (512, 512), 2),
])
def test_end_to_end_against_torch(algo, spec, hw, batch):
    """a bilinear=True Pytorch-UNet on the CPU, its state dict through tools/import_state_dict.py, the engine on the GPU"""
    import import_state_dict as imp

    tensors = synth.make_weights(spec, 21)
    imgs = synth.make_images(batch, hw[0], hw[1], spec.in_ch, 0x5EED + 21, "blobs")
    ref, model = _torch_logits(spec, tensors, imgs)
    spec2, blob = imp.convert(model.state_dict())
    assert spec2.up == "bilinear"
    with _engine(spec, hw, batch, algo) as eng:
        eng.load_weights(blob)
        labels, logits = eng.infer(imgs, want_logits=True)
    err = float(np.max(np.abs(logits - ref)))
    assert err < 1e-3, err
    srt = np.sort(ref, axis=1)
    safe = (srt[:, -1] - srt[:, -2]) > 2e-3
    assert np.array_equal(labels[safe], np.argmax(ref, axis=1)[safe])


def test_plan_properties():
    """graph replay == eager, batch permutation, clone and a two-rank group, kernel statistics"""
    spec = UNetSpec(1, 16, 3, 3, up="bilinear")
    blob = pack_weights(spec, synth.make_weights(spec, 31))
    size, batch = 128, 16
    imgs = synth.make_images(batch, size, size, 1, 0x5EED + 31, "blobs")
    with _engine(spec, size, batch) as eng:
        eng.load_weights(blob)
        runs = [eng.infer(imgs, want_logits=True) for _ in range(3)]         # eager, captured, replayed
        for lab, lg in runs[1:]:
            assert np.array_equal(lab, runs[0][0]) and np.array_equal(lg, runs[0][1])
        perm = np.random.default_rng(5).permutation(batch)
        lab_p, lg_p = eng.infer(imgs[perm], want_logits=True)
        assert np.array_equal(lab_p, runs[0][0][perm]) and np.array_equal(lg_p, runs[0][1][perm])
        with eng.clone() as c:
            assert np.array_equal(c.infer(imgs)[0], runs[0][0])
        eng.set_profiling(True)
        eng.infer(imgs)
        stats = eng.kernel_stats()
        eng.set_profiling(False)
        ups = [s for s in stats if s["kernel"] == "upsample2x_bilinear"]
        assert len(ups) == spec.levels and all(s["bytes"] > 0 and s["flops"] == 0 for s in ups)
        assert not any(s["kernel"].startswith("convT") for s in stats)
        names = [l["name"] for l in eng.layers()]
        assert not any(n.endswith(".t") for n in names) and [n for n in names if n.endswith(".up")] == ["up1.up", "up2.up", "up3.up"]
    with binding.Group(size, size, 1, 16, 3, 3, max_batch=batch // 2, devices=[0, 0]) as g:
        g.load_weights(blob)
        assert np.array_equal(g.infer(imgs)[0], runs[0][0])


def test_v2_files_that_do_not_describe_a_network_are_refused():
    spec = UNetSpec(1, 16, 2, 3, up="bilinear")
    blob = pack_weights(spec, synth.make_weights(spec, 41))
    bad_mode = bytearray(blob)
    struct.pack_into("<I", bad_mode, HEADER.size, 7)
    short = bytearray(blob[:-8])
    struct.pack_into("<I", short, 32, spec.n_params() - 2)                  # consistent length, but not the topology's
    long_ = bytearray(blob + b"\0" * 8)
    struct.pack_into("<I", long_, 32, spec.n_params() + 2)
    with _engine(spec, 32, 1) as eng:
        for bad in (bad_mode, short, long_, bytes(blob[:-4])):
            with pytest.raises(binding.MiUnetError) as e:
                eng.load_weights(bytes(bad))
            assert e.value.code == 4                                          # MI_UNET_EFILE
        eng.load_weights(blob)                                               # and the well-formed file loads
        assert eng.infer(synth.make_images(1, 32, 32, 1, 5))[0].shape == (1, 32, 32)


def test_pipeline_and_facade_match_the_transposed_net(tmp_path, capfd):
    """make_threshold_weights routes the image through the top skip connection only, so the bilinear and the transposed net
    compute the same function: the RAW16 pipeline and the facade must give identical masks, contours and files"""
    specs = {up: UNetSpec(up=up) for up in ("transpose", "bilinear")}
    blobs = {up: pack_weights(s, synth.make_threshold_weights(s)) for up, s in specs.items()}
    raws = [synth.make_raw16(1536, 2048, seed=21), synth.make_raw16(600, 800, seed=22)]
    seg = {}
    for up, spec in specs.items():
        with _engine(spec, 512, 2) as eng:
            eng.load_weights(blobs[up])
            seg[up] = eng.segment_raw16(raws)
    (t_tiles, t_masks, t_cont), (b_tiles, b_masks, b_cont) = seg["transpose"], seg["bilinear"]
    assert np.array_equal(t_tiles, b_tiles) and np.array_equal(t_masks, b_masks) and t_cont == b_cont
    assert (t_masks > 0).any()

    rp = tmp_path / "case.raw"
    raws[0].tofile(rp)
    files = {}
    out = tmp_path / "out"                                                  # the same directory: written paths compare equal
    for up in ("transpose", "bilinear"):
        wpath = tmp_path / f"{up}.miw"
        wpath.write_bytes(blobs[up])
        out.mkdir()
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / f"log_{up}"))
        assert hostlib.process_single_image(str(rp), 2048, 1536, str(out))
        log = open(hostlib.get_log_path()).read()
        hostlib.cleanup_resources()
        assert f"upsample={up}" in log
        files[up] = {p: (out / p).read_bytes() for p in sorted(os.listdir(out))}
        for p in files[up]:
            (out / p).unlink()
        out.rmdir()
    capfd.readouterr()
    assert files["transpose"] and files["transpose"] == files["bilinear"]
