"""Every class count the engine accepts (2..6) on every head path, on the device.

mi_unet_create takes 2..6 classes and the class count steers code written separately in many places: the five template
instances of head_argmax_kernel and its lane groups (Cin / 4 = 4 .. 64 lanes per pixel), the fused heads of conv_wino4.hip,
conv_wino4s.hip, conv_lp.hip (sized for 4 classes) and conv_lpr.hip (sized for 3, guarded by routing.cpp), the plan's
`classes <= 4` fusion rule, the plane strides of the tiled stitch and blend, and the logits offsets of every micro-batch, rank
and captured image.  The inputs (seven small nets, balanced head biases so that every class wins somewhere) are defined and
proven fit by the oracle alone in test_classes_cpu.py.

Tolerances, all the project's own:
  * fp32 plans: test_gpu_unet.check_parity (BASELINE north_star: logits within 1e-3; labels equal wherever the oracle's top-2
    margin exceeds 1e-3; device labels == first-max-wins argmax of the device's own logits); mismatching labels are printed and
    may not outnumber the oracle's own low-margin pixels;
  * 16-bit plans: the bars of test_gpu_bf16.py (test_end_to_end_tolerances: within 3e-2 of the bf16 oracle, within 1.5 x that
    oracle's own distance to fp32, labels equal where the fp32 margin > 0.1; test_config5_fp16_...: 5e-3, 1.5 x + 1e-3, 2e-2);
  * fused against stand-alone head of the same plan: 1e-5, labels wherever the margin exceeds that
    (test_gpu_unet.test_wino4_fusions_on_small_grids);
  * in situ: 1e-4 of the logit range (test_gpu_insitu.py).
"""
import functools

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_classes_cpu import ARGMAX_ROWS_3, ARGMAX_ROWS_6, CLASSES, NETS, balanced_weights, case, margins
from test_gpu_insitu import _fold
from test_gpu_postprocess import _blobs
from test_gpu_tile_blend import blend_f32, cut_views, first_max_argmax
from test_gpu_tiled import cut_tiles, stitch
from test_gpu_unet import check_parity, orc_argmax_batch

pytestmark = pytest.mark.gpu

# algo -> (|device - 16-bit oracle| bar, slack added to 1.5 x the oracle's own distance to fp32, fp32 margin above which labels agree)
LP_BARS = {"bf16": (3e-2, 0.0, 0.1), "fp16": (5e-3, 1e-3, 2e-2)}


def _engine(tag, classes, algo, max_batch=2):
    in_ch, base, levels, h, w, _ = NETS[tag]
    return binding.Engine(h, w, in_ch, base, levels, classes, max_batch=max_batch, conv_algo=algo)


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _oracle16(tag, classes, algo):
    c = case(tag, classes)
    return orc.unet_forward(c["blob"], c["imgs"], bf16=algo == "bf16", fp16=algo == "fp16")[0]


def _rotated(tensors):
    """the head's rows rotated by one: row k of the new head is row (k + 1) % classes of the old one (no class keeps its slot)"""
    t = dict(tensors)
    t["outc.w"] = np.roll(tensors["outc.w"], -1, axis=0)
    t["outc.b"] = np.roll(tensors["outc.b"], -1, axis=0)
    return t


def _fused_name(algo):
    return {"bf16": "conv3x3_bf16", "fp16": "conv3x3_fp16"}[algo]


def _rows():
    """the table of the whole-network test: (plan, algo, switches, net, classes, kernel that must carry the head)"""
    rows = []

    def add(plan, algo, env, tags, classes_list, head_of):
        for tag in tags:
            for k in classes_list:
                rows.append(pytest.param(plan, algo, env, tag, k, head_of(k), id=f"{plan}-{tag}-c{k}"))

    # fp32 stand-alone: all five instances of head_argmax_kernel, lane groups 4 (C), 8 (B, D), 16 (A), 32 (E), 64 (F)
    add("standalone", "direct", {"MIUNET_FUSE_HEAD": "0"}, "ABCDEF", CLASSES, lambda k: "head_argmax")
    # fp32 F(4x4,3x3): the persistent one-block kernel and the staged one; the plan fuses the head up to 4 classes.  Net G
    # (22 x 38) puts the image edge inside the head's tile on both sides; A never does
    add("wino4", "auto", {"MIUNET_WINO4_MIN_WG": "1", "MIUNET_WINO4S": "0"}, "AG", CLASSES,
        lambda k: "conv3x3_wino4+head" if k <= 4 else "head_argmax")
    add("wino4s", "auto", {"MIUNET_WINO4_MIN_WG": "1", "MIUNET_WINO4S": "2"}, "AG", CLASSES,
        lambda k: "conv3x3_wino4s+head" if k <= 4 else "head_argmax")
    for algo in ("bf16", "fp16"):
        name = _fused_name(algo)
        # conv_lp.hip, 64-wide tile (base 64)
        add(f"{algo}-tile64", algo, {}, "AG", CLASSES, lambda k, name=name: name + "+head" if k <= 4 else "head_argmax")
        # conv_lp.hip, 32-wide tile (base 32; base 16: Cout = 16 < tile, masked columns)
        add(f"{algo}-tile32", algo, {"MIUNET_LPR": "0"}, "BCD", (2, 3, 4), lambda k, name=name: name + "+head")
        # conv_lpr.hip (resident weights): its fused head is sized for three classes; conv3x3_lpr_shape_ok refuses four, which
        # must fall back to conv_lp.hip's fused head, not to a wrong result
        add(f"{algo}-resident", algo, {"MIUNET_LPR": "2"}, "BD", CLASSES,
            lambda k, name=name: name + "r+head" if k <= 3 else name + "+head" if k == 4 else "head_argmax")
    return rows


def _check_head_kernel(kernels, head):
    assert head in kernels, (head, sorted(set(kernels)))
    fused = [k for k in kernels if k.endswith("+head")]
    if head == "head_argmax":
        assert not fused, fused
    else:
        assert "head_argmax" not in kernels and set(fused) == {head}, (head, fused)


def _check_against_oracle(tag, classes, algo, labels, logits):
    c = case(tag, classes)
    low = int((margins(c["logits"]) <= 1e-3).sum())
    if algo in LP_BARS:
        bar16, slack, clear = LP_BARS[algo]
        ref16 = _oracle16(tag, classes, algo)
        noise = float(np.max(np.abs(ref16 - c["logits"])))           # what 16-bit operands cost in this network
        e16, e32 = float(np.max(np.abs(logits - ref16))), float(np.max(np.abs(logits - c["logits"])))
        safe = margins(c["logits"]) > clear
        bad = int((labels != c["labels"]).sum())
        print(f"\n{tag} c{classes} {algo}: |dev - {algo} oracle| = {e16:.3e} (bar {bar16:g}), |dev - fp32 oracle| = {e32:.3e} "
              f"(oracle's own {noise:.3e}), labels differing from fp32 oracle = {bad}, clear-margin share = {safe.mean():.3f}")
        assert e16 < bar16
        assert e32 < 1.5 * noise + slack
        assert np.array_equal(labels[safe], c["labels"][safe])
        assert np.array_equal(labels, orc_argmax_batch(logits))      # the argmax rule is exact on the device's own logits
    else:
        err = float(np.max(np.abs(logits - c["logits"])))
        flips = check_parity(labels, logits, c["logits"], c["labels"])
        print(f"\n{tag} c{classes} {algo}: |dev - oracle| = {err:.3e}, label mismatches = {flips}, oracle low-margin pixels = {low}")
        assert flips <= low


@pytest.mark.parametrize("plan,algo,env,tag,classes,head", _rows())
def test_whole_network_every_head_path(plan, algo, env, tag, classes, head, monkeypatch):
    """One (plan, net, class count): shape, oracle parity, the micro-batch seam (max_batch = 2: batch-3 nets run 2 + 1, so the
    second micro-batch lands at logits offset 2 * hw * classes), a single-image call and a labels-only call, the kernel that
    carried the head, the stand-alone head of the same plan where the head was fused, and plane identity under a rotation of
    the head's rows.  MIUNET_SPLITK=0 is the batch-invariant mode: an image's bits do not depend on its batch."""
    c = case(tag, classes)
    _, _, _, h, w, b = NETS[tag]
    imgs, spec = c["imgs"], c["spec"]
    monkeypatch.setenv("MIUNET_SPLITK", "0")
    _setenv(monkeypatch, env)
    with _engine(tag, classes, algo) as eng:
        eng.load_weights(c["blob"])
        eng.set_profiling(True)
        labels, logits = eng.infer(imgs, want_logits=True)
        kernels = [s["kernel"] for s in eng.kernel_stats()]
        eng.set_profiling(False)
        labels_only, none = eng.infer(imgs)
        l1, g1 = eng.infer(imgs[1:2], want_logits=True)
        eng.load_weights(pack_weights(spec, _rotated(c["tensors"])))
        labels_r, logits_r = eng.infer(imgs, want_logits=True)
    assert logits.shape == (b, classes, h, w) and labels.shape == (b, h, w) and none is None
    _check_head_kernel(kernels, head)
    _check_against_oracle(tag, classes, algo, labels, logits)
    assert np.array_equal(labels_only, labels)
    assert np.array_equal(g1[0], logits[1]) and np.array_equal(l1[0], labels[1])
    assert set(np.unique(labels).tolist()) == set(range(classes))

    # plane identity: every head, stand-alone or fused, computes a class's logit as its own dot product, summed in an order that
    # does not depend on the class index -> rotating the head's rows rotates the planes bit for bit.  A plane written to the
    # wrong slot or a row read with the wrong pitch shows here even where the error is too small for the 1e-3 bar.
    want_r = np.roll(logits, -1, axis=1)
    n_diff = int((logits_r.view(np.uint32) != want_r.view(np.uint32)).sum())
    print(f"{plan} {tag} c{classes}: logits differing in bits after rotating the head's rows = {n_diff}")
    assert n_diff == 0
    assert np.array_equal(labels_r, orc_argmax_batch(logits_r))

    if head != "head_argmax":        # the same plan with the stand-alone head: same products, another summation order
        monkeypatch.setenv("MIUNET_FUSE_HEAD", "0")
        with _engine(tag, classes, algo) as eng:
            eng.load_weights(c["blob"])
            eng.set_profiling(True)
            labels_u, logits_u = eng.infer(imgs, want_logits=True)
            kernels_u = [s["kernel"] for s in eng.kernel_stats()]
        _check_head_kernel(kernels_u, "head_argmax")
        diff = float(np.max(np.abs(logits - logits_u)))
        print(f"{plan} {tag} c{classes}: fused against stand-alone head, max |difference| = {diff:.3e}")
        assert diff < 1e-5
        clear = margins(logits_u) > 1e-5
        assert np.array_equal(labels[clear], labels_u[clear])


# ---------------------------------------------------------------- in situ: the head step on the device's own input
@pytest.mark.parametrize("classes", [2, 4, 6])
@pytest.mark.parametrize("family,tag,algo,env", [
    ("fp32", "A", "auto", {"MIUNET_WINO4_MIN_WG": "1"}),
    ("bf16", "A", "bf16", {}),
    ("fp16-resident", "B", "fp16", {"MIUNET_LPR": "2"}),
])
def test_head_step_in_situ(family, tag, algo, env, classes, monkeypatch):
    """mi_unet_debug_capture of the head step -- or of the conv that ran the head in its epilogue -- for image 1 of a batch of two
    (a non-zero im * classes * hw offset into the logits): the oracle's layer(s) applied to the tensor the step READ, within
    1e-4 of the logit range."""
    c = case(tag, classes)
    t, spec, imgs = c["tensors"], c["spec"], c["imgs"][:2]
    rnd = orc.bf16_round if algo == "bf16" else orc.fp16_round if algo == "fp16" else (lambda a: a)
    _setenv(monkeypatch, env)
    with _engine(tag, classes, algo) as eng:
        eng.load_weights(c["blob"])
        n = len(eng.layers())
        d, x, y, _, lab = eng.capture(imgs, n - 1, 1)
        if d["skipped"]:
            d, x, y, _, lab = eng.capture(imgs, n - 2, 1)
            assert d["fused_head"] and d["kind"] == "conv3x3"
        else:
            assert d["kind"] == "head"
    assert bool(d["fused_head"]) == (classes <= 4), d
    if classes <= 3 and family == "fp16-resident":
        assert d["kernel"] == "conv3x3_fp16r+head"
    if d["fused_head"]:
        name = d["name"]
        wf, shift = _fold(t, name[:-3], int(name[-1]), spec.bn_eps)
        act = np.maximum(orc.conv3x3(x[None], rnd(wf)) + shift, 0.0)
    else:
        act = x[None]
    ref = orc.conv1x1_planar(act, t["outc.w"], t["outc.b"])[0]
    assert y.shape == ref.shape == (classes,) + imgs.shape[1:3]
    err = float(np.max(np.abs(y - ref)))
    print(f"\n{family} {tag} c{classes}: {d['name']} on {d['kernel']}, max |device - oracle| = {err:.3e}")
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    assert np.array_equal(lab, orc.argmax_planar(y))


# ---------------------------------------------------------------- the argmax rule on the device
HEAD_PATHS = [
    ("standalone", "A", "direct", {"MIUNET_FUSE_HEAD": "0"}, "head_argmax"),
    ("wino4", "A", "winograd", {"MIUNET_WINO4_MIN_WG": "1", "MIUNET_WINO4S": "0", "MIUNET_WINO4_GUARD": "0"}, "conv3x3_wino4+head"),
    ("wino4s", "A", "winograd", {"MIUNET_WINO4_MIN_WG": "1", "MIUNET_WINO4S": "2", "MIUNET_WINO4_GUARD": "0"}, "conv3x3_wino4s+head"),
    ("bf16", "A", "bf16", {}, "conv3x3_bf16+head"),
    ("bf16-resident", "B", "bf16", {"MIUNET_LPR": "2"}, "conv3x3_bf16r+head"),
]


def _constant_head(spec, bias):
    """zero head weights: every pixel's logits are the biases exactly (activations are finite, 0 * x = 0, 0 + b = b)"""
    t = synth.make_weights(spec, 4321)
    t["outc.w"] = np.zeros_like(t["outc.w"])
    t["outc.b"] = np.array(bias, np.float32)
    return t


@pytest.mark.parametrize("classes,rows", [(3, ARGMAX_ROWS_3), (6, ARGMAX_ROWS_6)], ids=["c3", "c6"])
@pytest.mark.parametrize("path,tag,algo,env,head", HEAD_PATHS, ids=[p[0] for p in HEAD_PATHS])
def test_argmax_rule_on_the_device(path, tag, algo, env, head, classes, rows, monkeypatch):
    """Strict '>' from -FLT_MAX in class order: ties and NaN keep the lower index (src/process.cpp:158-170 of the reference, pinned
    for the oracle by test_oracle_unet.test_argmax_rules).  Random weights never produce ties, NaN or -FLT_MAX, so the rows are fed
    as head biases under zero head weights, through each of the five device implementations; at 6 classes the plan never fuses
    the head, so every path runs head_argmax_kernel<6> (lane groups 16 and 8).  The fp32 plan is pinned to F(4x4) without the
    load-time probe (MIUNET_WINO4_GUARD=0), which would otherwise compare NaN logits."""
    in_ch, base, levels, h, w, b = NETS[tag]
    spec = UNetSpec(in_ch, base, levels, classes)
    imgs = synth.make_images(b, h, w, in_ch, 0xBEEF, "blobs")
    _setenv(monkeypatch, env)
    if classes > 4:
        head = "head_argmax"
    with _engine(tag, classes, algo) as eng:
        for bias, want in rows:
            eng.load_weights(pack_weights(spec, _constant_head(spec, bias)))
            eng.set_profiling(True)
            labels, logits = eng.infer(imgs, want_logits=True)
            kernels = [s["kernel"] for s in eng.kernel_stats()]
            eng.set_profiling(False)
            _check_head_kernel(kernels, head)
            assert (labels == want).all(), (bias, want, np.unique(labels).tolist())
            bv = np.array(bias, np.float32)
            for k in range(classes):
                if np.isnan(bv[k]):
                    assert np.isnan(logits[:, k]).all(), (bias, k)
                else:
                    assert (logits[:, k].view(np.uint32) == bv[k:k + 1].view(np.uint32)[0]).all(), (bias, k)


@pytest.mark.parametrize("classes,rows", [(3, ARGMAX_ROWS_3), (6, ARGMAX_ROWS_6)], ids=["c3", "c6"])
def test_argmax_rule_through_blend_finalize(classes, rows):
    """The same rows through tiled inference with blending `constant` + mirror `xy` (blend_finalize computes the labels), for the
    rows without NaN or infinity.  Every view's logits are the biases, so the expected result is blend_f32 (the definition of
    include/mi_unet.h, operation for operation in float32) of constant views: bit for bit.  A weighted mean of equal values may
    differ from the value by an ulp, equally in all tied planes since the weights are per pixel: tied planes stay bit-equal to
    each other and the lower index wins.  The rows holding -FLT_MAX or -1e38 overflow float32 in the weighted SUM of up to 16
    views (to -inf, by that definition), so for those the expectation is the definition's, not the row's label."""
    th, tw, H, W, halo = 40, 24, 100, 72, 4
    spec = UNetSpec(1, 16, 3, classes)
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    nk = cut_views(img, th, tw, halo, "xy").shape[0]
    with binding.Engine(th, tw, 1, 16, 3, classes, max_batch=5) as eng:
        eng.set_tile_blend("constant", 0.125, "xy")
        for bias, want in rows:
            bv = np.array(bias, np.float32)
            if not np.isfinite(bv).all():
                continue
            eng.load_weights(pack_weights(spec, _constant_head(spec, bias)))
            labels, logits = eng.infer_tiled(img, halo, want_logits=True)
            views = np.ascontiguousarray(np.broadcast_to(bv[None, :, None, None], (nk, classes, th, tw)))
            with np.errstate(over="ignore"):
                want_labels, want_logits = blend_f32(views, H, W, th, tw, halo, "constant", 0.125, "xy")
            assert np.array_equal(logits, want_logits) and np.array_equal(labels, want_labels), bias
            assert np.array_equal(labels, first_max_argmax(logits))
            for k in range(classes):
                for j in range(k + 1, classes):
                    if bv[k] == bv[j]:
                        assert np.array_equal(logits[k].view(np.uint32), logits[j].view(np.uint32)), (bias, k, j)
            if np.isfinite(want_logits).all():
                assert (labels == want).all(), (bias, want)
            else:
                assert np.abs(bv).max() >= 1e38


# ---------------------------------------------------------------- tiled, blended, grouped, downstream
GRIDS = [(40, 24, 100, 72, 4), (32, 32, 77, 99, 5)]       # image widths: a multiple of 4 and odd (two of the stitch's store widths)


def _tiled_net(classes, img, th, tw, halo):
    spec = UNetSpec(1, 16, 3, classes)
    tensors = balanced_weights(spec, 4321, cut_tiles(img, th, tw, halo))
    return spec, pack_weights(spec, tensors)


@pytest.mark.parametrize("classes", [2, 6])
@pytest.mark.parametrize("th,tw,H,W,halo", GRIDS)
def test_tiled_is_infer_on_the_stacked_tiles_then_stitched(th, tw, H, W, halo, classes):
    """bit for bit: the stitch walks `classes` planes with plane strides classes * th * tw (tiles) and H * W (image)"""
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    spec, blob = _tiled_net(classes, img, th, tw, halo)
    with binding.Engine(th, tw, 1, 16, 3, classes, max_batch=5) as eng:
        eng.load_weights(blob)
        tile_labels, tile_logits = eng.infer(cut_tiles(img, th, tw, halo), want_logits=True)
        labels, logits = eng.infer_tiled(img, halo, want_logits=True)
        again, _ = eng.infer_tiled(img, halo)
    assert logits.shape == (classes, H, W) and labels.shape == (H, W)
    assert np.array_equal(labels, stitch(tile_labels, H, W, th, tw, halo))
    assert np.array_equal(logits, stitch(tile_logits, H, W, th, tw, halo))
    assert np.array_equal(again, labels)
    assert set(np.unique(labels).tolist()) == set(range(classes))


@pytest.mark.parametrize("classes", [2, 5])
@pytest.mark.parametrize("th,tw,H,W,halo", GRIDS)
def test_blend_is_infer_on_the_views_then_blended(th, tw, H, W, halo, classes):
    """bit for bit against blend_f32 of the per-view logits (gaussian + mirror xy; constant + mirror x)"""
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    spec, blob = _tiled_net(classes, img, th, tw, halo)
    with binding.Engine(th, tw, 1, 16, 3, classes, max_batch=5) as eng:
        eng.load_weights(blob)
        for mode, sigma, mirror in (("gaussian", 0.125, "xy"), ("constant", 0.125, "x")):
            eng.set_tile_blend(mode, sigma, mirror)
            _, view_logits = eng.infer(cut_views(img, th, tw, halo, mirror), want_logits=True)
            want_labels, want_logits = blend_f32(view_logits, H, W, th, tw, halo, mode, sigma, mirror)
            labels, logits = eng.infer_tiled(img, halo, want_logits=True)
            assert logits.shape == (classes, H, W)
            assert np.array_equal(logits, want_logits), (mode, mirror, float(np.max(np.abs(logits - want_logits))))
            assert np.array_equal(labels, want_labels), (mode, mirror)
            assert np.array_equal(eng.infer_tiled(img, halo)[0], labels), (mode, mirror)
            assert set(np.unique(labels).tolist()) == set(range(classes))


def test_group_of_two_ranks_at_five_classes():
    """devices = [0, 0], batch 5 (ragged shards 3 + 2, micro-batches of 2): each rank's logits land at lo * hw * classes"""
    spec = UNetSpec(1, 16, 2, 5)
    imgs = synth.make_images(5, 64, 64, 1, 0xB5, "blobs")
    blob = pack_weights(spec, balanced_weights(spec, 4321, imgs))
    with binding.Engine(64, 64, 1, 16, 2, 5, max_batch=2) as eng:
        eng.load_weights(blob)
        lab0, log0 = eng.infer(imgs, want_logits=True)
    with binding.Group(64, 64, 1, 16, 2, classes=5, max_batch=2, devices=[0, 0]) as g:
        assert g.size == 2
        g.load_weights(blob)
        lab, log = g.infer(imgs, want_logits=True)
    assert log.shape == (5, 5, 64, 64)
    assert np.array_equal(lab, lab0) and np.array_equal(log, log0)
    ref_logits, ref_labels = orc.unet_forward(blob, imgs)
    check_parity(lab, log, ref_logits, ref_labels)
    assert set(np.unique(lab).tolist()) == set(range(5))


def _six_label_map(seed, h, w, fill):
    """random blobs of label 2 inside regions (vertical bands) of labels 3, 4, 5, 0, 1"""
    bands = np.array([3, 4, 5, 0, 1], np.uint8)[(np.arange(w) * 5) // w]
    m = np.broadcast_to(bands[None, :], (h, w)).copy()
    m[_blobs(seed, h, w, fill) == 2] = 2
    return m


@pytest.mark.parametrize("h,w", [(96, 160), (64, 64)])
def test_postprocess_of_label_maps_with_six_labels(h, w):
    """postprocess_mask takes label 2 as the foreground and everything else -- labels 3, 4, 5 included -- as background"""
    batch = np.stack([_six_label_map(200 + s, h, w, f) for s, f in enumerate([0.3, 0.5, 0.7, 0.5, 0.4])])
    assert set(np.unique(batch).tolist()) == set(range(6))
    with binding.Engine(h, w, classes=6, max_batch=2) as eng:
        got = eng.postprocess_masks(batch)
    for i in range(batch.shape[0]):
        assert np.array_equal(got[i], orc.postprocess_mask(batch[i])), i
    assert set(np.unique(got).tolist()) == {0, 2}


def test_segment_raw16_on_a_four_class_net():
    """mask_to_image has no stand-alone binding, and in mi_unet_segment_raw16 it runs behind postprocess_mask, whose output holds 0
    and 2 only: labels >= 3 cannot reach it through any entry point.  What can be reached is checked: a 4-class intensity
    classifier (make_threshold_weights plus class 3 = 3 x - 1.65, which wins above x = 0.75 = 191.25 / 255, between two 8-bit
    levels, by >= 1.9e-3) whose label maps hold 0, 1, 2 and 3; the labels meet the oracle's, and the mask image of the whole
    pipeline is mask_to_image(postprocess_mask(labels)) of the oracle, where label 3 is background like 0 and 1."""
    spec = UNetSpec(1, 16, 2, 4)
    t = synth.make_threshold_weights(spec)
    t["outc.w"][3, 0] = 3.0
    t["outc.b"][3] = -1.65
    blob = pack_weights(spec, t)
    raws = [synth.make_raw16(300, 400, seed=60), synth.make_raw16(256, 256, seed=61), synth.make_raw16(200, 360, seed=62)]
    with binding.Engine(128, 128, 1, 16, 2, 4, max_batch=2) as eng:
        eng.load_weights(blob)
        tiles, labels, logits = eng.infer_raw16(raws, want_logits=True)
        tiles2, masks, contours = eng.segment_raw16(raws)
    assert np.array_equal(tiles, tiles2) and logits.shape == (3, 4, 128, 128)
    ref_logits, ref_labels = orc.unet_forward(blob, tiles[..., None])
    check_parity(labels, logits, ref_logits, ref_labels)
    assert set(np.unique(labels).tolist()) == {0, 1, 2, 3}
    for i in range(3):
        assert np.array_equal(masks[i], orc.mask_to_image(orc.postprocess_mask(labels[i]))), i
    assert set(np.unique(masks).tolist()) == {0, 255}
