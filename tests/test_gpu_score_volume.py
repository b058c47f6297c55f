"""Scores of a volume on the device (include/mi_unet.h: mi_unet_score_volume) against the brute-force reference of
score_volume_ref.py: every field of every plane, exactly, and the bytes of the host form.  The cases are score_volume_ref's, the ones
test_score_volume_cpu.py holds the host form to; they are checked for non-degeneracy on the reference alone before the device is
asked.  Then the facade: a series with a truth directory scored as one volume, on the device and through the host route."""
import itertools
import json
import math
import os

import numpy as np
import pytest

import score_ref
import score_volume_ref as sr
import volume_ref as vr
from miunet import binding
from test_score_volume_cpu import FIRST_ILLEGAL, LAST_LEGAL, call_with, earg_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def test_the_cases_are_not_degenerate():
    sr.assert_not_degenerate()


@pytest.mark.parametrize("shape", sr.SHAPES)
def test_device_equals_the_reference_and_the_host_bytes(shape):
    pred, truth = sr.case(shape)
    with bare_engine() as eng:
        for units in sr.UNITS:
            for q in sr.QUANTILES:
                got = eng.score_volume(pred, truth, sr.VALUES, units, q)
                sr.assert_equal(got, sr.case_ref(shape, units, q), f"{shape} {units} {q}")
                assert got.tobytes() == binding.score_volume_host(pred, truth, sr.VALUES, units, q).tobytes(), (shape, units, q)


@pytest.mark.parametrize("units", sr.UNITS[1:])
def test_axis_permutations_give_the_same_bytes(units):
    pred, truth = sr.case((5, 40, 72))
    want = binding.score_volume_host(pred, truth, sr.VALUES, units, 50000).tobytes()
    with bare_engine() as eng:
        for perm in itertools.permutations(range(3)):
            p, t, u = sr.permuted(pred, truth, units, perm)
            assert eng.score_volume(p, t, sr.VALUES, u, 50000).tobytes() == want, (units, perm, p.shape, u)


@pytest.mark.parametrize("units", sr.UNITS)
def test_an_exact_tie_and_its_mirrors(units):
    pred, truth, d2 = sr.tie_case(units)
    want = sr.score_volume(pred, truth, (1,), units, 0)
    assert want[0]["a_to_t"]["max_d2"] == d2
    with bare_engine() as eng:
        got = eng.score_volume(pred, truth, (1,), units, 0)
        sr.assert_equal(got, want, f"tie {units}")
        for axes, p, t in sr.mirrors(pred, truth):
            assert eng.score_volume(p, t, (1,), units, 0).tobytes() == got.tobytes(), (units, axes)


def test_the_widest_row_and_the_d2_limit():
    pred, truth = sr.wide_row_case()
    want = sr.score_volume(pred, truth, (1,), (5, 3, 1), 0)
    assert want[0]["a_to_t"]["max_d2"] == (5 * (8180 - 3))**2 + 3**2 and (5 * 8191)**2 + 3**2 < 2**31
    far_p, far_t = np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8)
    far_p[0, 0, 0] = far_t[1, 1, 1] = 1
    with bare_engine() as eng:
        got = eng.score_volume(pred, truth, (1,), (5, 3, 1), 0)
        sr.assert_equal(got, want, "1 x 2 x 8192")
        assert got.tobytes() == binding.score_volume_host(pred, truth, (1,), (5, 3, 1), 0).tobytes()
        at_limit = eng.score_volume(far_p, far_t, (1,), LAST_LEGAL, 0)
        sr.assert_equal(at_limit, sr.score_volume(far_p, far_t, (1,), LAST_LEGAL, 0), "the diagonal at the limit")
        assert at_limit[0]["q_d2_sym"] == 2**31 - 32
        with pytest.raises(binding.MiUnetError):
            eng.score_volume(far_p, far_t, (1,), FIRST_ILLEGAL, 0)


def test_confusion_matrix_on_the_device():
    pred, truth = sr.case((7, 33, 70))
    with bare_engine() as eng:
        for classes in (3, 16):
            scores, conf, skipped = eng.score_volume(pred, truth, sr.VALUES, (2, 2, 5), classes=classes)
            want, want_skipped = score_ref.confusion(pred.reshape(1, 1, -1), truth.reshape(1, 1, -1), classes)
            assert np.array_equal(conf, want[0]) and skipped[0] == want_skipped[0]
            assert scores.tobytes() == binding.score_volume_host(pred, truth, sr.VALUES, (2, 2, 5)).tobytes()


def test_one_engine_serves_growing_and_shrinking_calls_and_the_other_stages():
    """a small call, a larger one, then smaller ones return the bytes of fresh engines; mi_unet_score_labels and
    mi_unet_volume_components in between still return their own reference bytes: the stages share a handle (and the two score stages a
    workspace)"""
    small, mid, large = sr.case((3, 1, 130)), sr.case((9, 17, 1)), sr.case((7, 33, 70))
    tie = sr.tie_case((2, 2, 5))[:2]
    calls = [(small, sr.VALUES, (1, 1, 1), 50000), (large, sr.VALUES, (3, 1, 7), 0), (small, sr.VALUES, (1, 1, 1), 50000),
             (mid, (2,), (2, 2, 5), 500000), (tie, (1,), (2, 2, 5), 0), (large, (3, 1), (2, 2, 5), 999999)]
    fresh = []
    for (p, t), v, u, q in calls:
        with bare_engine(32, 32) as eng:
            fresh.append(eng.score_volume(p, t, v, u, q).tobytes())
    assert fresh[0] == fresh[2]
    flat_pred, flat_truth = large[0][:2], large[1][:2]
    labels_want = binding.score_labels_host(flat_pred, flat_truth, (1, 2)).tobytes()
    noise = vr.smooth_noise((3, 64, 64))
    with bare_engine(32, 32) as eng:
        for i, (((p, t), v, u, q), want) in enumerate(zip(calls, fresh)):
            assert eng.score_volume(p, t, v, u, q).tobytes() == want, i
            if i % 2 == 0:
                assert eng.score_labels(flat_pred, flat_truth, (1, 2)).tobytes() == labels_want, i
            else:
                vr.assert_equal(eng.volume_components(noise, vr.NOISE_VALUES, want_ids=True), vr.noise_ref((3, 64, 64), 26), f"after call {i}")


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_score_volume, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_score_volume, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error(), name
        rc, untouched = call_with(L.mi_unet_score_volume, (None,), {})
        assert rc != 0 and untouched
        pred, truth = sr.case((3, 1, 130))                      # the engine still works
        sr.assert_equal(eng.score_volume(pred, truth, sr.VALUES, (2, 2, 5)), sr.case_ref((3, 1, 130), (2, 2, 5), 50000))


# ---- the facade: five RAW slices and their truth files through process_image_batch ----------------------------------------------------------
def _assert_volume_score(path, stacks, truths, labels, units, unit_mm):
    """volume_score.json against mi_unet_score_volume_host + mi_unet_score_volume_derive on the same stacks (doubles exactly; null = NaN)"""
    doc = json.loads(open(path, "rb").read())
    assert sorted(doc) == sorted(["slices", "unit_mm", "spacing_units", "quantile_ppm", "targets"])
    assert doc["slices"] == [f"s{z}" for z in range(5)] and doc["quantile_ppm"] == 50000
    assert (doc["unit_mm"], doc["spacing_units"]) == (unit_mm, list(units)) and [t["label"] for t in doc["targets"]] == list(labels)
    finite = 0
    for t, stack, truth in zip(doc["targets"], stacks, truths):
        host = binding.score_volume_host(stack, truth, (255,), units)
        sr.assert_equal(host, sr.score_volume(stack, truth, (255,), units))
        sc = host[0]
        assert (t["tp"], t["fp"], t["fn"]) == (int(sc["tp"]), int(sc["fp"]), int(sc["fn"]))
        want = binding.score_volume_derive(sc, unit_mm)
        for f, g in (("dice", "dice"), ("iou", "iou"), ("hd_mm", "hd"), ("hd_q_mm", "hd_q"), ("assd_mm", "assd"), ("rmsd_mm", "rmsd")):
            assert (t[f] is None and math.isnan(want[g])) or t[f] == want[g], (path, f, t[f], want[g])
        assert sorted(t) == sorted(["label", "tp", "fp", "fn", "dice", "iou", "hd_mm", "hd_q_mm", "assd_mm", "rmsd_mm"])
        finite += t["hd_mm"] is not None and t["hd_mm"] > 0.0 and 0.0 < t["dice"] < 1.0
    assert finite == len(labels)                                # a real comparison: overlap, and two surfaces apart


def test_facade_scores_a_series_as_one_volume(tmp_path, monkeypatch):
    from miunet import hostlib
    from test_gpu_targets import blob, raw_of
    from test_gpu_volume import FACADE_TARGETS, SPACING, read_stack, slice_labels
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    truth_dir = tmp_path / "truth"
    os.makedirs(truth_dir)
    paths, ws, hs, truth_maps = [], [], [], []
    for z in range(5):
        r = raw_of(slice_labels(z), 1 + z % 2)
        paths.append(str(tmp_path / f"s{z}.raw"))
        r.tofile(paths[-1])
        ws.append(r.shape[1]); hs.append(r.shape[0])
        truth_maps.append(np.roll(slice_labels(4 if z == 3 else z), (1, -2), (0, 1)))     # moved in the slice; slice 3 shows slice 4
        truth_maps[-1].tofile(str(truth_dir / f"s{z}_labels.raw"))
    truth_maps = np.stack(truth_maps)
    labels = [c for c, _ in FACADE_TARGETS]
    truths = [np.where(truth_maps == c, 255, 0).astype(np.uint8) for c in labels]
    units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
    assert (units, unit_mm) == ((70, 70, 300), 0.01)
    dirs = {n: tmp_path / n for n in ("volume_only", "truth_only", "both", "host", "keep", "missing")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        # either setting alone: no file and no line of this stage
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("volume_only")
        assert "Volume score" not in log and "Volume: 5 slices" in log and "volume_score.json" not in os.listdir(dirs["volume_only"])
        assert hostlib.set_volume(False) and hostlib.set_truth_dir(str(truth_dir))
        log = run("truth_only")
        assert "Volume" not in log and not [n for n in os.listdir(dirs["truth_only"]) if "volume" in n]
        slice_scores = sorted(n for n in os.listdir(dirs["truth_only"]) if n.endswith("_score.json"))
        assert slice_scores == [f"s{z}_score.json" for z in range(5)]
        # both: the volume's score beside everything either setting writes alone, byte for byte
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("both")
        assert log.count("Volume score: 5 slices, 2 targets, ") == 1 and "Volume score skipped" not in log
        alone = set(os.listdir(dirs["volume_only"])) | set(os.listdir(dirs["truth_only"]))
        assert set(os.listdir(dirs["both"])) == alone | {"volume_score.json"}
        for n in alone:
            src = dirs["volume_only"] if n in os.listdir(dirs["volume_only"]) else dirs["truth_only"]
            assert (dirs["both"] / n).read_bytes() == (src / n).read_bytes(), n
        stacks = [read_stack(dirs["both"], "s{z}_mask_class{cls}.png", c) for c in labels]
        _assert_volume_score(dirs["both"] / "volume_score.json", stacks, truths, labels, units, unit_mm)
        # the host route under MEDSEG_HOST_POSTPROCESS=1: the same document
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        log = run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert log.count("Volume score: 5 slices, 2 targets, ") == 1
        assert (dirs["host"] / "volume_score.json").read_bytes() == (dirs["both"] / "volume_score.json").read_bytes()
        # an active filter is scored on the filtered masks, which differ from the unfiltered ones
        assert hostlib.set_volume(True, 26, 0, 1, SPACING)
        run("keep")
        kept = [read_stack(dirs["keep"], "s{z}_volume_mask_class{cls}.png", c) for c in labels]
        assert all(0 < int((k == 255).sum()) < int((s == 255).sum()) for k, s in zip(kept, stacks))
        _assert_volume_score(dirs["keep"] / "volume_score.json", kept, truths, labels, units, unit_mm)
        assert (dirs["keep"] / "volume_score.json").read_bytes() != (dirs["both"] / "volume_score.json").read_bytes()
        # one truth file missing: the skip line, no file, and every image still succeeds
        os.remove(truth_dir / "s2_labels.raw")
        log = run("missing")
        assert "Volume score skipped: 1 of 5 slices without mask or truth" in log and "Volume score:" not in log
        assert "volume_score.json" not in os.listdir(dirs["missing"]) and "volume_report.json" in os.listdir(dirs["missing"])
    finally:
        hostlib.set_volume(False)
        hostlib.set_truth_dir("")
        hostlib.set_targets([])
        hostlib.cleanup_resources()
