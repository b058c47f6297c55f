"""Scores against ground truth on the device (include/mi_unet.h: mi_unet_score_labels) against the brute-force
reference of score_ref.py: every field of every plane, exactly.  The cases are score_ref's, the ones test_score_cpu.py holds the host
form to.  Inputs are checked for non-degeneracy on the reference alone before the device is asked."""
import functools
import json
import math
import os

import numpy as np
import pytest

import morph_ref as mr
import score_ref as sr
from miunet import binding, hostlib, synth
from miunet.spec import UNetSpec, pack_weights
from test_gpu_targets import call_segment, raw_of
from test_morph_cpu import morph_maps
from test_score_cpu import call_with, degenerate_counts, earg_cases

pytestmark = pytest.mark.gpu

PPMS = (0, 50000, 500000, 999999)
VALUES = (1, 2, 3)


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


@functools.lru_cache(maxsize=None)
def label_case(h, w):
    pred, truth = sr.shifted_pair(morph_maps(h, w))
    return pred, truth, {ppm: sr.score_labels(pred, truth, VALUES, ppm) for ppm in PPMS}


def test_the_label_map_inputs_are_not_degenerate():
    tot = np.zeros(3, int)
    for hw in ((64, 64), (48, 80)):
        tot += degenerate_counts(label_case(*hw)[2][50000])
    assert tot[0] >= 10 and tot[1] >= 5 and tot[2] >= 3, tot


@pytest.mark.parametrize("h,w", [(64, 64), (48, 80)])
def test_label_maps_equal_the_reference_at_every_quantile(h, w):
    pred, truth, ref = label_case(h, w)
    with bare_engine() as eng:
        for ppm in PPMS:
            got = eng.score_labels(pred, truth, VALUES, ppm)
            sr.assert_equal(got, ref[ppm], f"{h}x{w} {ppm}")
            assert np.array_equal(got, binding.score_labels_host(pred, truth, VALUES, ppm))
            if ppm == 0:
                for d in ("a_to_t", "t_to_a"):
                    assert np.array_equal(got[d]["q_d2"], got[d]["max_d2"])


@pytest.mark.parametrize("name", sorted(sr.edge_cases()))
def test_edge_cases_equal_the_reference(name):
    pred, truth, values = sr.edge_cases()[name]
    with bare_engine() as eng:
        for ppm in (0, 50000):
            sr.assert_equal(eng.score_labels(pred, truth, values, ppm), sr.score_labels(pred, truth, values, ppm), name)


def test_ties_do_not_depend_on_order():
    """four boundary pixels of T at one distance from A's pixel, and the mirrored / transposed pictures: the same numbers"""
    pred, truth, values = sr.edge_cases()["ties"]
    with bare_engine() as eng:
        base = eng.score_labels(pred, truth, values, 0)[0, 0]
        assert base["a_to_t"]["max_d2"] == 16 and base["t_to_a"]["sum_d_q16"] == 4 * (4 << 16)
        for p, t in ((pred[:, ::-1], truth[:, ::-1]), (pred[:, :, ::-1], truth[:, :, ::-1]), (pred.transpose(0, 2, 1), truth.transpose(0, 2, 1))):
            other = eng.score_labels(np.ascontiguousarray(p), np.ascontiguousarray(t), values, 0)[0, 0]
            assert other.tobytes() == base.tobytes()


@pytest.mark.parametrize("classes", [1, 4, 16])
def test_confusion_matrix(classes):
    rng = np.random.default_rng(classes)
    pred = rng.integers(0, 6, (2, 37, 53)).astype(np.uint8)
    truth = np.where(rng.random((2, 37, 53)) < 0.7, pred, rng.integers(0, 6, (2, 37, 53))).astype(np.uint8)
    pred[0, 0, :5] = 200; truth[1, 3, 3] = 16; truth[0, 0, 0] = 255; pred[1, 36, 52] = classes
    values = tuple(v for v in (0, 1, 3, 5) if v < classes)
    with bare_engine() as eng:
        scores, conf, skipped = eng.score_labels(pred, truth, values, classes=classes)
    rc, rs = sr.confusion(pred, truth, classes)
    assert np.array_equal(conf, rc) and np.array_equal(skipped, rs) and (skipped > 0).all()
    assert np.array_equal(conf.sum((1, 2)) + skipped, [37 * 53] * 2)
    sr.assert_equal(scores, sr.score_labels(pred, truth, values))
    # diagonal and row / column sums reproduce tp / fp / fn -- up to the pixels left out, whose partner byte is >= classes: count them
    for b in range(2):
        out_p, out_t = pred[b] >= classes, truth[b] >= classes
        for k, v in enumerate(values):
            s = scores[b, k]
            assert conf[b, v, v] == s["tp"]
            assert conf[b, :, v].sum() - conf[b, v, v] == s["fp"] - int(((pred[b] == v) & out_t).sum())
            assert conf[b, v, :].sum() - conf[b, v, v] == s["fn"] - int(((truth[b] == v) & out_p).sum())


def test_no_weights_growth_and_shrinkage_return_the_bytes_of_fresh_engines():
    small = sr.edge_cases()["odd_33x70"]
    pred, truth, _ = label_case(48, 80)
    calls = [(small[0], small[1], (1,)), (pred, truth, VALUES), (small[0], small[1], (1, 0)), (pred[:1], truth[:1], (2,))]
    fresh = []
    for p, t, v in calls:
        with bare_engine(32, 32) as eng:
            fresh.append(eng.score_labels(p, t, v, classes=4))
    with bare_engine(32, 32) as eng:                            # one engine: the workspace grows, then serves smaller calls
        for (p, t, v), want in zip(calls, fresh):
            got = eng.score_labels(p, t, v, classes=4)
            assert all(np.array_equal(g, w) and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def threshold_weights(spec):
    """(test_gpu_morph.py's) logit_c = c * x + b_c with x = pixel / 255, the lines crossing between 8-bit levels"""
    t = synth.make_threshold_weights(spec)
    cuts = [(60.5 + 50.0 * j) / 255.0 for j in range(spec.classes - 1)]
    t["outc.w"][:] = 0
    t["outc.b"][:] = 0
    for c in range(spec.classes):
        t["outc.w"][c, 0] = float(c)
        t["outc.b"][c] = -float(sum(cuts[:c]))
    return t


def pipeline_maps(h=64, w=64):
    maps = morph_maps(h, w).copy()
    maps[:, 0, 0], maps[:, h - 1, w - 1] = 0, 3
    return maps


def test_in_the_pipeline_and_between_a_measuring_call_and_its_report():
    targets = [(2, 0.01), (1, 0.0)]
    maps = pipeline_maps()
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    rs = [raw_of(m, 1 + i % 2) for i, m in enumerate(maps)]
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, threshold_weights(spec)))
        eng.set_targets(targets)
        _, labels, _ = eng.infer_raw16(rs)
        assert np.array_equal(labels, maps)
        masks = eng.postprocess_masks_multi(labels)                       # [B][K][H][W] in {0, cls}
        want = np.stack([mr.masks(m, targets, [(mr.RECT, 1, 0)]) for m in maps])
        assert np.array_equal(masks, want)
        for k, (cls, _) in enumerate(targets):
            got = eng.score_labels(masks[:, k], maps, (cls,))
            sr.assert_equal(got, sr.score_labels(want[:, k], maps, (cls,)), f"target {k}")
            assert 0 < binding.score_derive(got[0, 0])["dice"] <= 1.0
        eng.set_measure(True)
        call_segment(binding.lib().mi_unet_segment_raw16_multi, eng._h, rs, 2, 8192, 256, 64, 64)
        ms_before = eng.last_stage_ms()
        eng.score_labels(masks[:, 0], maps, (2,), classes=4)              # between the measuring call and its report
        regions, rcounts = eng.last_regions()
        assert eng.last_stage_ms() == ms_before
        call_segment(binding.lib().mi_unet_segment_raw16_multi, eng._h, rs, 2, 8192, 256, 64, 64)
        again, acounts = eng.last_regions()
        assert regions.tobytes() == again.tobytes() and np.array_equal(rcounts, acounts) and (rcounts > 0).any()


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_score_labels, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases(5, 7):
            rc, untouched = call_with(L.mi_unet_score_labels, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error(), name
        rc, untouched = call_with(L.mi_unet_score_labels, (None,), {})
        assert rc != 0 and untouched
        pred, truth, ref = label_case(48, 80)                   # the engine still works
        sr.assert_equal(eng.score_labels(pred, truth, VALUES), ref[50000])


def _assert_score_json(path, masks, truth, labels):
    """<base>_score.json against the reference (integers) and mi_unet_score_derive (doubles, exactly; null = NaN)"""
    doc = json.loads(open(path, "rb").read())
    assert doc["quantile_ppm"] == 50000 and [t["label"] for t in doc["targets"]] == list(labels)
    for t, mask, cls in zip(doc["targets"], masks, labels):
        ref = sr.score_plane(mask, truth, cls)
        assert (t["tp"], t["fp"], t["fn"]) == (ref["tp"], ref["fp"], ref["fn"])
        want = binding.score_derive(binding.score_labels_host(mask[None], truth[None], (cls,))[0, 0])
        for f in ("dice", "iou", "hd", "hd_q", "assd", "rmsd"):
            assert (t[f] is None and math.isnan(want[f])) or t[f] == want[f], (path, cls, f, t[f], want[f])
        assert sorted(t) == sorted(["label", "tp", "fp", "fn", "dice", "iou", "hd", "hd_q", "assd", "rmsd"])


def test_facade_scores_against_a_truth_directory(tmp_path, monkeypatch):
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(pack_weights(spec, threshold_weights(spec)))
    maps = pipeline_maps()
    paths, ws, hs = [], [], []
    for i, m in enumerate(maps):
        r = raw_of(m, 1 + i % 2)
        paths.append(str(tmp_path / f"img{i}.raw"))
        r.tofile(paths[-1])
        ws.append(r.shape[1]); hs.append(r.shape[0])
    truth_dir = tmp_path / "truth"
    os.makedirs(truth_dir)
    maps[0].tofile(str(truth_dir / "img0_labels.raw"))                   # good; img1: wrong size; img2: missing
    maps[1][:10].tofile(str(truth_dir / "img1_labels.raw"))
    default = [mr.masks(m, [(2, 0.06)], [(mr.RECT, 1, 0)])[0] for m in maps]
    assert (default[0] == 2).any()
    dirs = {n: tmp_path / n for n in ("never", "off", "batch", "single", "multi", "host")}
    for d in dirs.values():
        os.makedirs(d)
    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        # truth off: the artefacts of a run that never touched the setting
        assert hostlib.process_image_batch(paths[:2], ws[:2], hs[:2], str(dirs["never"])) == 2
        assert hostlib.set_truth_dir(str(truth_dir)) and hostlib.set_truth_dir("")
        assert hostlib.process_image_batch(paths[:2], ws[:2], hs[:2], str(dirs["off"])) == 2
        assert sorted(os.listdir(dirs["never"])) == sorted(os.listdir(dirs["off"])) and len(os.listdir(dirs["off"])) == 10
        for name in os.listdir(dirs["never"]):
            assert (dirs["never"] / name).read_bytes() == (dirs["off"] / name).read_bytes(), name
        # one good, one wrong-size and one missing truth file: all three images succeed, one score file
        assert hostlib.set_truth_dir(str(truth_dir)) and hostlib.get_truth_dir() == str(truth_dir)
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs["batch"])) == 3
        assert [n for n in sorted(os.listdir(dirs["batch"])) if n.endswith("_score.json")] == ["img0_score.json"]
        assert set(os.listdir(dirs["never"])) < set(os.listdir(dirs["batch"]))
        for name in os.listdir(dirs["never"]):                           # the other artefacts do not change
            assert (dirs["never"] / name).read_bytes() == (dirs["batch"] / name).read_bytes(), name
        _assert_score_json(dirs["batch"] / "img0_score.json", [default[0]], maps[0], [2])
        # the thread's context, and the CPU tail with the host form: the same document
        assert hostlib.process_single_image(paths[0], ws[0], hs[0], str(dirs["single"]))
        assert hostlib.process_single_image(paths[1], ws[1], hs[1], str(dirs["single"]))
        assert [n for n in os.listdir(dirs["single"]) if n.endswith("_score.json")] == ["img0_score.json"]
        assert (dirs["single"] / "img0_score.json").read_bytes() == (dirs["batch"] / "img0_score.json").read_bytes()
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        assert hostlib.process_single_image(paths[0], ws[0], hs[0], str(dirs["host"]))
        assert hostlib.process_image_batch(paths[1:], ws[1:], hs[1:], str(dirs["host"])) == 2
        assert [n for n in os.listdir(dirs["host"]) if n.endswith("_score.json")] == ["img0_score.json"]
        assert (dirs["host"] / "img0_score.json").read_bytes() == (dirs["batch"] / "img0_score.json").read_bytes()
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        # several targets: one entry per target, in target order
        targets = [(2, 0.01), (1, 0.0)]
        assert hostlib.set_targets(targets)
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs["multi"])) == 3
        assert [n for n in sorted(os.listdir(dirs["multi"])) if n.endswith("_score.json")] == ["img0_score.json"]
        _assert_score_json(dirs["multi"] / "img0_score.json", mr.masks(maps[0], targets, [(mr.RECT, 1, 0)]), maps[0], [2, 1])
    finally:
        hostlib.set_truth_dir("")
        hostlib.set_targets([])
        hostlib.cleanup_resources()
