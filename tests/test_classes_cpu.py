"""Class counts 2..6: the inputs of tests/test_gpu_classes.py, proven fit by the oracle alone.  CPU only.

mi_unet_create accepts 2..6 classes, and the class count steers the head kernels, the fused epilogues, the plane strides of
the tiled stitch / blend and the logits offsets of every micro-batch.  The GPU tests run seven small nets at every class
count; this file owns those inputs and shows, before any device result is looked at, that they can tell a broken plane
from a working one:

  * `synth.make_weights` gives head biases 0.05 * ((7 i) % 5 - 2), with which class 5 of a 6-class net is never the argmax
    on most small nets, so a broken last plane would only show in the logits.  `balanced_weights` replaces the bias of
    class k by minus the mean (batch and pixels) of the oracle's class-k logit computed with zero bias: every plane then
    has zero mean and every class wins somewhere.
  * for each of the 35 (net, classes) cases: every class index occurs in >= 2 % of the pixels, pixels whose oracle top-2
    margin is <= 1e-3 (where a device label may legitimately differ) are <= 1 %, and pixels with margin > 0.1 (where the
    16-bit plans' labels are compared) are > 50 %.  Measured with the oracle alone: rarest class >= 4.9 %, low-margin
    share 0.00 - 0.48 %, clear-margin share >= 56.9 %; the test prints the figures of every case.  If a case misses a cap
    after a change to synth, change the seed, not the cap.
"""
import functools

import numpy as np
import pytest

import oracle_lib as orc
from miunet import synth
from miunet.spec import UNetSpec, pack_weights
from test_gpu_tile_blend import first_max_argmax

# tag -> (in_ch, base, levels, H, W, batch)
NETS = {
    "A": (1, 64, 2, 80, 48, 3),
    "B": (1, 32, 3, 96, 80, 3),
    "C": (1, 16, 3, 64, 64, 2),
    "D": (3, 32, 3, 96, 80, 2),
    "E": (1, 128, 2, 32, 48, 2),
    "F": (1, 256, 1, 16, 32, 2),
    # one level, both sides ragged for the 16 x 16 tile of the fp32 fused heads and for conv_lp.hip's 8 x 32 tile (net A, 80 x 48,
    # never meets an image edge inside a head tile)
    "G": (1, 64, 1, 22, 38, 2),
}
CLASSES = (2, 3, 4, 5, 6)
WEIGHT_SEED, IMAGE_SEED = 4321, 0xBEEF
MIN_CLASS_SHARE, MAX_LOW_MARGIN, MIN_CLEAR_MARGIN = 0.02, 0.01, 0.5


def net_spec(tag, classes):
    in_ch, base, levels, _, _, _ = NETS[tag]
    return UNetSpec(in_ch, base, levels, classes)


def net_images(tag):
    in_ch, _, _, h, w, b = NETS[tag]
    return synth.make_images(b, h, w, in_ch, IMAGE_SEED, "blobs")


def balanced_weights(spec, seed, imgs):
    """make_weights with outc.b[k] = -mean over batch and pixels of the oracle's class-k logit at zero bias"""
    t = synth.make_weights(spec, seed)
    t["outc.b"] = np.zeros(spec.classes, np.float32)
    logits, _ = orc.unet_forward(pack_weights(spec, t), imgs)
    t["outc.b"] = (-logits.astype(np.float64).mean(axis=(0, 2, 3))).astype(np.float32)
    return t


def margins(logits):
    """[B,classes,H,W] -> top-2 margin [B,H,W]"""
    srt = np.sort(logits, axis=1)
    return srt[:, -1] - srt[:, -2]


@functools.lru_cache(maxsize=None)
def case(tag, classes):
    """-> dict(spec, tensors, blob, imgs, logits, labels) of one (net, class count): balanced weights, the fp32 oracle's result"""
    spec, imgs = net_spec(tag, classes), net_images(tag)
    tensors = balanced_weights(spec, WEIGHT_SEED, imgs)
    blob = pack_weights(spec, tensors)
    logits, labels = orc.unet_forward(blob, imgs)
    return dict(spec=spec, tensors=tensors, blob=blob, imgs=imgs, logits=logits, labels=labels)


def input_figures(c):
    """(share of the rarest class, share of pixels with margin <= 1e-3, share with margin > 0.1)"""
    counts = np.bincount(c["labels"].reshape(-1), minlength=c["spec"].classes)
    m = margins(c["logits"])
    return float(counts.min()) / c["labels"].size, float((m <= 1e-3).mean()), float((m > 0.1).mean())


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("tag", sorted(NETS))
def test_inputs_use_every_class_with_clear_margins(tag, classes):
    c = case(tag, classes)
    in_ch, base, levels, h, w, b = NETS[tag]
    assert c["logits"].shape == (b, classes, h, w) and c["labels"].shape == (b, h, w)
    rarest, low, clear = input_figures(c)
    print(f"\nnet {tag} (in_ch {in_ch}, base {base}, {levels} levels, {h}x{w}, batch {b}), {classes} classes: rarest class "
          f"{100 * rarest:.2f} %, margin <= 1e-3 on {100 * low:.2f} %, margin > 0.1 on {100 * clear:.2f} % of the pixels")
    assert set(np.unique(c["labels"]).tolist()) == set(range(classes))
    assert rarest >= MIN_CLASS_SHARE
    assert low <= MAX_LOW_MARGIN
    assert clear > MIN_CLEAR_MARGIN


def test_balanced_biases_differ_from_the_default_and_centre_every_plane():
    """what the helper is for: with synth's biases class 5 of net A never wins; with the balanced ones every plane has zero mean"""
    spec, imgs = net_spec("A", 6), net_images("A")
    _, labels = orc.unet_forward(pack_weights(spec, synth.make_weights(spec, WEIGHT_SEED)), imgs)
    assert 5 not in np.unique(labels)
    c = case("A", 6)
    assert np.max(np.abs(c["logits"].astype(np.float64).mean(axis=(0, 2, 3)))) < 1e-5
    assert not np.array_equal(c["tensors"]["outc.b"], synth.make_weights(spec, WEIGHT_SEED)["outc.b"])


@pytest.mark.parametrize("classes", [2, 6])
@pytest.mark.parametrize("tag", ["A", "D"])
def test_oracle_batch_independence_and_first_max_wins(tag, classes):
    """the oracle's own rules beyond 3 planes: an image's result does not depend on its batch neighbours, and its labels are the
    first-max-wins argmax of its logits (strict '>' from -FLT_MAX in class order)"""
    c = case(tag, classes)
    lg1, lb1 = orc.unet_forward(c["blob"], c["imgs"][1:2])
    assert np.array_equal(lg1[0], c["logits"][1]) and np.array_equal(lb1[0], c["labels"][1])
    for b in range(c["imgs"].shape[0]):
        assert np.array_equal(c["labels"][b], first_max_argmax(c["logits"][b]))
        assert np.array_equal(c["labels"][b], orc.argmax_planar(c["logits"][b]))


FMAX = float(np.finfo(np.float32).max)
NAN = float("nan")
# (logits of one pixel, expected label): rows of test_oracle_unet.test_argmax_rules, and three rows at 6 classes
ARGMAX_ROWS_3 = [([1, 1, 1], 0), ([0, 2, 2], 1), ([NAN, NAN, NAN], 0), ([NAN, -1, NAN], 1), ([-FMAX] * 3, 0), ([-np.inf] * 3, 0),
                 ([-FMAX, -FMAX, -1e38], 2), ([3, -1, 2], 0), ([NAN, 5, 7], 2)]
ARGMAX_ROWS_6 = [([1, 2, 2, 2, 0, 2], 1), ([NAN, NAN, NAN, NAN, NAN, 4], 5), ([-FMAX] * 5 + [-1e38], 5)]


@pytest.mark.parametrize("rows", [ARGMAX_ROWS_3, ARGMAX_ROWS_6], ids=["3", "6"])
def test_argmax_rows_on_the_oracle(rows):
    """the rows the device tests feed as head biases, on the oracle's argmax and on the numpy restatement of the rule"""
    px = np.array([r for r, _ in rows], np.float32)
    logits = np.ascontiguousarray(px.T.reshape(px.shape[1], 1, -1))
    want = [w for _, w in rows]
    assert orc.argmax_planar(logits)[0].tolist() == want
    assert first_max_argmax(logits)[0].tolist() == want
