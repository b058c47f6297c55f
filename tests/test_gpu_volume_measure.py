"""The volume measurement on the device (include/mi_unet.h: mi_unet_volume_measure): every case of volume_measure_ref.py
equals the all-voxel numpy reference field for field and is the host form's bytes; one engine serves growing and shrinking calls; an
engine with weights infers the same labels before and after; argument errors queue nothing."""
import numpy as np
import pytest

import volume_measure_ref as mm
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_measure_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def check(eng, name):
    """the device's table equals the reference's exactly and is the host form's bytes"""
    got = mm.call(eng.volume_measure, name)
    mm.assert_equal(got, mm.case_ref(name), name)
    assert got.tobytes() == mm.call(binding.volume_measure_host, name).tobytes(), name
    return got


def test_the_cases_are_not_degenerate():
    mm.assert_not_degenerate()


@pytest.mark.parametrize("name", list(mm.cases()))
def test_device_equals_reference_and_host(name):
    """W = 72 and 130 are no multiples of 64 and rows cross the 64-lane segments; D = 1; ids of 0, -1 and m + 1; run-end counts round the
    LDS tile; the sheet's ties under two unit sets and three caps; m = 4096; no intensity"""
    with bare_engine() as eng:
        check(eng, name)


def test_a_search_of_more_than_one_launch_equals_the_host_form():
    """the sheet in 16 x 96 x 96 is one component of 49152 run ends: 1.2e9 pairs, more than one launch of the pair search may hold, over
    192 tiles.  (The all-voxel reference would take minutes here; the host form is compared with it on every other case.)"""
    ids = mm.sheet((16, 96, 96))
    inten = mm.intensity_for(ids.shape, 8)
    with bare_engine() as eng:
        got = eng.volume_measure(ids, inten, m=1, units=(3, 3, 10))
    assert got[0]["ends"] == got[0]["voxels"] == 49152 and 49152 * 49153 // 2 > 1 << 30
    assert got.tobytes() == binding.volume_measure_host(ids, inten, m=1, units=(3, 3, 10)).tobytes()


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state: every call gives the bytes of a
    fresh engine (the host form's); the neighbouring stage's workspace is its own"""
    import volume_ref as vr

    order = ("box", "noise(16, 24, 130)c26", "scattered", "noise(7, 40, 72)c6", "sheet(7, 7, 50)", "box", "m4096", "sheet_cap0", "no_intensity")
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name)
            if i == 2:
                vr.assert_equal(eng.volume_components(vr.smooth_noise((3, 64, 64)), vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))


def test_ids_of_the_components_stage_measure_what_its_table_counts():
    """the two stages chained on the device: voxels and the first sums of the measured table are the components table's"""
    import volume_ref as vr

    vol = vr.smooth_noise((7, 40, 72))
    with bare_engine() as eng:
        _, table, found, _, ids = eng.volume_components(vol, (2,), 18, cap=64, want_ids=True)
        m = min(int(found[0]), 64)
        got = eng.volume_measure(ids[0], None, m=m, units=(1, 1, 1))
    for f in ("voxels", "sx", "sy", "sz"):
        assert np.array_equal(got[f], table[0][f][:m]), f
    assert (got["dp"] >= table[0]["first"][:m]).all() and (got["a_p"] >= table[0]["first"][:m]).all()     # `first` is the raster-first voxel


def test_an_engine_with_weights_infers_the_same_labels_before_and_after():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, "scattered")
        check(eng, "noise(3, 64, 64)c26")
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_measure, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_measure, (eng._h,), case)
            assert rc == 1 and untouched and b"mi_unet_volume_measure:" in L.mi_unet_last_error(), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_measure, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_measure, (None,), {})
        assert rc != 0 and untouched
        check(eng, "box")                                        # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0), (2, 0.0)]
SPACING = (0.7, 0.7, 3.0)
MEASURE_KEYS = ["diameter_mm", "diameter_ends", "axial_diameter_mm", "axial_slice", "axial_ends", "axes_mm", "axes_dir", "mean", "std", "min",
                "max", "ends"]


def test_facade_measures_every_component_of_the_report(tmp_path, monkeypatch):
    import json
    import os

    import volume_ref as vr
    from miunet import hostlib
    from test_gpu_targets import blob, raw_of
    from test_gpu_volume import read_stack
    from test_gpu_volume_clean import series_labels
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    paths, ws, hs = [], [], []
    for z in range(5):
        r = raw_of(series_labels(z), 1 + z % 2)
        paths.append(str(tmp_path / f"s{z}.raw"))
        r.tofile(paths[-1])
        ws.append(r.shape[1]); hs.append(r.shape[0])
    labels = [c for c, _ in FACADE_TARGETS]
    dirs = {n: tmp_path / n for n in ("never", "off", "alone", "on", "host", "capped", "keep", "channel")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def xyz(idx):
        return [idx % 64, idx // 64 % 64, idx // 4096]

    def check_measures(name, pattern, max_ends, min_voxels=0):
        """every "measure" member against derive-of-reference on the pictures this very call wrote"""
        doc = json.loads((dirs[name] / "volume_report.json").read_bytes())
        inten = read_stack(dirs[name], "s{z}_normalized.png", 0).astype(np.uint16)
        units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
        seen = 0
        for t, c in zip(doc["targets"], labels):
            stack = read_stack(dirs[name], "s{z}_mask_class{cls}.png", c)
            plane = vr.plane(stack, 255, 26, min_voxels, 0, cap=vr.MAX_TABLE)
            rows = mm.measure(plane["ids"], inten, min(plane["found"], vr.MAX_TABLE), units, max_ends)
            assert len(t["components"]) == len(rows), c
            for comp, row in zip(t["components"], rows):
                assert list(comp)[-1] == "measure"
                got = comp["measure"]
                if row["voxels"] == 0:                          # dropped by the volume filter
                    assert got is None and comp["kept"] == 0
                    continue
                seen += 1
                want = mm.derive(row, units, unit_mm)
                assert list(got) == MEASURE_KEYS and got["ends"] == row["ends"] and (got["min"], got["max"]) == (row["imin"], row["imax"])
                if row["d2"] < 0:
                    assert [got[k] for k in MEASURE_KEYS[:5]] == [None] * 5
                else:
                    assert got["diameter_mm"] == want["diameter_mm"] and got["axial_diameter_mm"] == want["axial_diameter_mm"]
                    assert got["diameter_ends"] == [xyz(row["dp"]), xyz(row["dq"])] and got["axial_ends"] == [xyz(row["a_p"]), xyz(row["a_q"])]
                    assert got["axial_slice"] == f"s{row['a_p'] // 4096}"
                assert got["axes_mm"] == pytest.approx(want["axis_mm"], rel=1e-12) and got["mean"] == pytest.approx(want["mean"], rel=1e-15)
                assert got["std"] == pytest.approx(want["std"], rel=1e-12)
                for v in got["axes_dir"]:
                    assert abs(sum(a * a for a in v) - 1.0) < 1e-14
        return doc, seen

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log_never = run("never")
        # set and taken back: every artefact of a run that never touched the setting
        assert hostlib.set_volume_measure(True, 0, 1000) and hostlib.set_volume_measure(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume measure" not in log_never + log_off
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        # measuring only together with `volume on`
        assert hostlib.set_volume(False) and hostlib.set_volume_measure(True)
        log = run("alone")
        assert "Volume" not in log and not [n for n in os.listdir(dirs["alone"]) if "volume" in n]
        # on, the device route: the same files, the report gains the members and nothing else
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("on")
        assert log.count("Volume measure: 5 slices, 3 targets, ") == 1
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc, seen = check_measures("on", "s{z}_mask_class{cls}.png", mm.DEFAULT_MAX_ENDS)
        assert seen >= 2
        plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
        for t in doc["targets"]:
            for comp in t["components"]:
                del comp["measure"]
        assert doc == plain
        # the host route: the same report bytes
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert (dirs["host"] / "volume_report.json").read_bytes() == (dirs["on"] / "volume_report.json").read_bytes()
        # a cap below the largest component's run ends: its diameters are null, the rest of the member stays
        assert hostlib.set_volume_measure(True, 0, 40)
        run("capped")
        cdoc, _ = check_measures("capped", "s{z}_mask_class{cls}.png", 40)
        assert any(comp["measure"]["diameter_mm"] is None for t in cdoc["targets"] for comp in t["components"])
        # under a filter a dropped component has no member to give
        assert hostlib.set_volume(True, 26, 1500, 0, SPACING) and hostlib.set_volume_measure(True)
        run("keep")
        kdoc, kept = check_measures("keep", "s{z}_mask_class{cls}.png", mm.DEFAULT_MAX_ENDS, 1500)
        assert 0 < kept < seen
        # a channel the engine does not have ends only this step: the report of a run without the setting
        assert hostlib.set_volume(True, 26, 0, 0, SPACING) and hostlib.set_volume_measure(True, 3)
        log = run("channel")
        assert "Volume measure error: channel 3 of 1" in log
        assert (dirs["channel"] / "volume_report.json").read_bytes() == (dirs["never"] / "volume_report.json").read_bytes()
    finally:
        hostlib.set_volume_measure(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
