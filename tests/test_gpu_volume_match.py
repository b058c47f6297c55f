"""The volume matching on the device (include/mi_unet.h: mi_unet_volume_match): every case of volume_match_ref.py equals
the numpy reference field for field and is the host form's bytes; one engine serves growing and shrinking tables between other stages;
7.9's ids chain in on the device; an engine with weights infers the same labels before and after; argument errors queue nothing."""
import numpy as np
import pytest

import volume_match_ref as vm
import volume_ref as vr
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_match_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


@pytest.fixture(scope="module")
def host():
    """the host form's result per case, computed once"""
    return {name: vm.call(binding.volume_match_host, name) for name in vm.cases()}


def check(eng, name, host):
    """the device's tables equal the reference's exactly and are the host form's bytes"""
    got = vm.call(eng.volume_match, name)
    vm.assert_equal(got, vm.case_ref(name), vm.cases()[name][4], name)
    for g, h in zip(got[:3], host[name][:3]):
        assert g.tobytes() == h.tobytes(), name
    assert got[3] == host[name][3], name
    return got


def test_the_cases_are_not_degenerate():
    vm.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vm.cases()))
def test_device_equals_reference_and_host(name, host):
    """W = 72 and 130 are no multiples of 64 and rows cross the 64-lane segments; D = 1; ids of 0, -1 and m + 1; segments with more keys
    than the wave reduces; one key over the whole walk; mp != mt; m = 1 and m = 4096; a short, an exact and a long pair list"""
    with bare_engine() as eng:
        check(eng, name, host)


def test_one_engine_serves_growing_and_shrinking_tables_between_other_stages(host):
    """before weights are loaded; the 67 MB table first, so that every later, smaller table lies inside cells the first call has written:
    a clear that misses a cell, or a workspace shared with the neighbouring stage, shows as a count that a fresh engine does not give"""
    order = ("m4096", "m1", "lesions", "noise(16, 24, 130)", "m4096", "lesions")
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name, host)
            if i == 2:
                vr.assert_equal(eng.volume_components(vr.smooth_noise((3, 64, 64)), vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))


def test_ids_of_the_components_stage_match_what_its_table_counts():
    """the two stages chained on the device: the side tables' voxels are the components tables', and the result is the case's"""
    masks = vr.smooth_noise((16, 24, 130))
    moved = np.zeros_like(masks)
    moved[:, 1:, :] = masks[:, :-1, :]
    with bare_engine() as eng:
        sides = []
        for m in (masks, moved):
            _, table, found, _, ids = eng.volume_components(m, [1], connectivity=26, cap=vm.MAX_TABLE, want_ids=True)
            sides.append((ids[0], int(found[0]), table[0]))
        (pi, mp, ptab), (ti, mt, ttab) = sides
        got = eng.volume_match(pi, ti, mp, mt, cap=vm.CAP)
    assert np.array_equal(got[0]["voxels"], ptab["voxels"][:mp]) and np.array_equal(got[1]["voxels"], ttab["voxels"][:mt])
    vm.assert_equal(got, vm.case_ref("noise(16, 24, 130)"), vm.CAP)


def test_an_engine_with_weights_infers_the_same_labels_before_and_after(host):
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, "scattered(7, 40, 72)", host)
        check(eng, "lesions", host)
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched(host):
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_match, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_match, (eng._h,), case)
            assert rc == 1 and untouched and b"mi_unet_volume_match:" in L.mi_unet_last_error(), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_match, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_match, (None,), {})
        assert rc != 0 and untouched
        check(eng, "lesions", host)                              # the engine still works


# ---- the facade: five RAW slices and their truth files through process_image_batch ----------------------------------------------------------
LESION_KEYS = ["pred", "truth", "iou_threshold", "tp", "fp", "fn", "precision", "recall", "f1", "pq", "sq", "rq", "mean_dice", "matches", "missed",
               "spurious"]


def lesions_of(stack, truth, iou, min_voxels=0, keep_largest=0):
    """the "lesions" member by the binding's host forms on the same stacks: 7.9's ids on both sides (the filter on pred only), the match,
    the assignment and the scores"""
    _, ptab, pfound, _, pids = binding.volume_components_host(stack, [255], 26, min_voxels, keep_largest, cap=vm.MAX_TABLE, want_ids=True)
    _, ttab, tfound, _, tids = binding.volume_components_host(truth, [255], 26, cap=vm.MAX_TABLE, want_ids=True)
    mp, mt = int(pfound[0]), int(tfound[0])
    ps, ts, pairs, found = binding.volume_match_host(pids[0], tids[0], max(mp, 1), max(mt, 1), cap=max(mp, 1) * max(mt, 1))
    vm.assert_equal((ps, ts, pairs, found), vm.match(pids[0], tids[0], max(mp, 1), max(mt, 1)), len(pairs))
    of_p, of_t, counts = binding.volume_match_assign(ps, ts, pairs, found, iou=iou)
    d = binding.volume_match_derive(ps, ts, pairs, found, of_p)
    inter = {(int(q["p"]), int(q["t"])): int(q["voxels"]) for q in pairs[:found]}
    want = dict(pred=mp, truth=mt, iou_threshold=list(iou), **counts)
    want.update({k: (None if np.isnan(d[k]) else d[k]) for k in ("precision", "recall", "f1", "pq", "sq", "rq", "mean_dice")})
    want["matches"] = []
    for p in range(mp):
        if of_p[p]:
            t, vp = int(of_p[p]) - 1, int(ps["voxels"][p])
            i, vt = inter[(p, t)], int(ts["voxels"][t])
            want["matches"].append(dict(pred=p, truth=t, voxels=i, iou=i / (vp + vt - i), dice=2.0 * i / (vp + vt), pred_voxels=vp, truth_voxels=vt))
    want["missed"] = [dict(truth=t, voxels=int(ts["voxels"][t])) for t in range(mt) if not of_t[t] and ts["voxels"][t] > 0]
    want["spurious"] = [p for p in range(mp) if not of_p[p] and ps["voxels"][p] > 0]
    return want


def test_facade_scores_a_series_per_lesion(tmp_path, monkeypatch):
    import json
    import os

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
    dirs = {n: tmp_path / n for n in ("never", "off", "no_truth", "on", "host", "quarter", "keep")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def check_lesions(name, pattern, iou, **filt):
        doc = json.loads((dirs[name] / "volume_score.json").read_bytes())
        plain = json.loads((dirs["never"] / "volume_score.json").read_bytes())
        seen = dict(tp=0, other=0)
        for t, c, truth in zip(doc["targets"], labels, truths):
            assert list(t)[-1] == "lesions" and list(t["lesions"]) == LESION_KEYS, list(t["lesions"])
            assert t["lesions"] == lesions_of(read_stack(dirs[name], pattern, c), truth, iou, **filt), (name, c)
            seen["tp"] += t["lesions"]["tp"]
            seen["other"] += t["lesions"]["fp"] + t["lesions"]["fn"]
            if not filt:
                del t["lesions"]
        if not filt:
            assert doc == plain                                  # the member is all the setting adds
        return seen

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING) and hostlib.set_truth_dir(str(truth_dir))
        log_never = run("never")
        # set and taken back: every artefact of a run that never heard of the setting
        assert hostlib.set_volume_match(True, (1, 3)) and hostlib.set_volume_match(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume match" not in log_never + log_off and "volume_score.json" in names
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        # matching only where there is a volume score
        assert hostlib.set_truth_dir("") and hostlib.set_volume_match(True)
        log = run("no_truth")
        assert "Volume match" not in log and "volume_score.json" not in os.listdir(dirs["no_truth"])
        assert (dirs["no_truth"] / "volume_report.json").read_bytes() == (dirs["never"] / "volume_report.json").read_bytes()
        # on, the device route: the same files, the score gains the member and nothing else
        assert hostlib.set_truth_dir(str(truth_dir))
        log = run("on")
        assert log.count("Volume match: 2 targets, ") == 1 and "Volume match error" not in log
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_score.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        seen = check_lesions("on", "s{z}_mask_class{cls}.png", (1, 2))
        assert seen["tp"] >= 1
        # the host route: the same file
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        log = run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert log.count("Volume match: 2 targets, ") == 1
        assert (dirs["host"] / "volume_score.json").read_bytes() == (dirs["on"] / "volume_score.json").read_bytes()
        # another threshold reaches the document
        assert hostlib.set_volume_match(True, (1, 4))
        run("quarter")
        check_lesions("quarter", "s{z}_mask_class{cls}.png", (1, 4))
        # under the volume filter the dropped components carry no voxel: absent, and an index is still the report's
        assert hostlib.set_volume(True, 26, 0, 1, SPACING) and hostlib.set_volume_match(True)
        run("keep")
        check_lesions("keep", "s{z}_mask_class{cls}.png", (1, 2), keep_largest=1)
        report = json.loads((dirs["keep"] / "volume_report.json").read_bytes())
        score = json.loads((dirs["keep"] / "volume_score.json").read_bytes())
        for rt, st in zip(report["targets"], score["targets"]):
            assert st["lesions"]["pred"] == min(rt["found"], vm.MAX_TABLE) and st["lesions"]["tp"] + st["lesions"]["fp"] == rt["kept"]
            for m in st["lesions"]["matches"]:
                assert rt["components"][m["pred"]]["voxels"] == m["pred_voxels"] and rt["components"][m["pred"]]["kept"] == 1
    finally:
        hostlib.set_volume_match(False)
        hostlib.set_volume(False)
        hostlib.set_truth_dir("")
        hostlib.set_targets([])
        hostlib.cleanup_resources()
