"""The volume zones on the device (include/mi_unet.h: mi_unet_volume_zones): every case of volume_zones_ref.py equals
the numpy reference cell for cell and record for record and is the host form's bytes; one engine serves growing and shrinking calls; the
stage chains with the components and the measurement stages; an engine with weights infers the same labels before and after; argument
errors queue nothing; the facade writes a "zones" member into volume_report.json."""
import numpy as np
import pytest

import volume_zones_ref as vz
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_zones_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def check(eng, name):
    """the device's result equals the reference's exactly and is the host form's bytes: table, both tables, the list and found"""
    got = vz.call(eng.volume_zones, name)
    vz.assert_equal(got, vz.case_ref(name), name)
    assert vz.same_bytes(got, vz.call(binding.volume_zones_host, name)), name
    return got


def test_the_cases_are_not_degenerate():
    vz.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vz.cases()))
def test_device_equals_reference_and_host(name):
    """W = 72, 130, 70, 96 and 330 are no multiples of the 64-voxel tile row, H = 40, 33, 19, 9 and 29 none of its 8 rows, D = 7, 5, 3 and 9
    none of its 4 slices; runs that cross tile borders along every offset (a constant slab; lines through tile corners); a run of 8192
    along each axis, clamped and not; runs of R - 1, R and R + 1; zones that meet only diagonally, two ids and two blobs that stay apart, a
    zone the merge has to travel along; ids of 0, -1 and m + 1; D = 1, H = 1 and one voxel; each output NULL; a list that is cut; both
    ends of the cell limit"""
    with bare_engine() as eng:
        check(eng, name)


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state: every call gives the bytes of a
    fresh engine (the host form's); the neighbouring stages' workspaces are their own"""
    import volume_ref as vr
    import volume_texture_ref as tx

    order = ("hand_4x4", "noise(16, 24, 130)_smooth_L32_count", "scattered", "noise(7, 40, 72)_noisy_L8_count", "m4096_L32_R32", "one_voxel_volume",
             "constant_slab", "entry_only", "m1_L64_R8192", "cap_1", "checkerboard_levels", "no_zones", "serpentine_level")
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name)
            if i == 2:
                vr.assert_equal(eng.volume_components(vr.smooth_noise((3, 64, 64)), vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))
            if i == 5:
                tx.assert_equal(tx.call(eng.volume_texture, "scattered"), tx.case_ref("scattered"), "texture between")


def test_ids_of_the_components_stage_and_the_measurement_agree_with_the_zones():
    """7.9, 7.13 and this stage chained on the device: voxels, imin and imax are what volume_measure reports for the same ids and
    intensity; each table sums to its runs and the zones of a component to its voxels"""
    import volume_ref as vr
    import volume_texture_ref as tx

    vol = vr.smooth_noise((7, 40, 72))
    inten = tx.smooth(vol.shape, 31)
    with bare_engine() as eng:
        _, _, found, _, ids = eng.volume_components(vol, (2,), 18, cap=64, want_ids=True)
        m = min(int(found[0]), 64)
        measured = eng.volume_measure(ids[0], inten, m=m, units=(1, 1, 1))
        table, rlm, axial, zones, n = eng.volume_zones(ids[0], inten, m, levels=16)
    assert m > 5 and table["voxels"].min() > 0 and n > m
    for f in ("voxels", "imin", "imax"):
        assert np.array_equal(table[f], measured[f]), f
    assert np.array_equal(rlm.sum(axis=(1, 2), dtype=np.int64), table["runs"]) and table["runs"].max() > 1000
    assert np.array_equal(axial.sum(axis=(1, 2), dtype=np.int64), table["runs_axial"])
    assert np.array_equal(np.bincount(zones["component"][:n], zones["size"][:n], minlength=m).astype(np.int64), table["voxels"])
    assert np.array_equal(np.bincount(zones["component"][:n], minlength=m), table["zones"])


def test_an_engine_with_weights_infers_the_same_labels_before_and_after():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, "scattered")
        check(eng, "noise(7, 40, 72)_smooth_L32_width")
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_zones, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_zones, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error().startswith(b"mi_unet_volume_zones:"), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_zones, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_zones, (None,), {})
        assert rc != 0 and untouched
        check(eng, "two_ids_one_level")                          # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0), (2, 0.0)]
SPACING = (0.7, 0.7, 3.0)
ZONES_KEYS = ["levels", "mode", "max_run", "glrlm", "glrlm_axial", "glszm"]


def test_facade_adds_the_zones_of_every_component_to_the_report(tmp_path, monkeypatch):
    import json
    import math
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
    dirs = {n: tmp_path / n for n in ("never", "off", "alone", "on", "host", "width", "both", "channel")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def close(got, want):
        return (got is None and math.isnan(want)) or (got is not None and abs(got - want) <= 1e-12 * abs(want))

    def check_zones(name, L, mode, lo=0, width=1, R=32):
        """every "zones" member against features-of-reference on the pictures this very call wrote"""
        doc = json.loads((dirs[name] / "volume_report.json").read_bytes())
        inten = read_stack(dirs[name], "s{z}_normalized.png", 0).astype(np.uint16)
        seen = 0
        for t, c in zip(doc["targets"], labels):
            stack = read_stack(dirs[name], "s{z}_mask_class{cls}.png", c)
            plane = vr.plane(stack, 255, 26, 0, 0, cap=vr.MAX_TABLE)
            m = min(plane["found"], vr.MAX_TABLE)
            rows, rlm, axial, zl, found, _ = vz.zones(plane["ids"], inten, m, L, mode, lo, width, R)
            assert len(t["components"]) == m, c
            for r, comp in enumerate(t["components"]):
                assert list(comp)[-1] == "zones"
                got = comp["zones"]
                seen += 1
                assert list(got) == ZONES_KEYS and (got["levels"], got["mode"], got["max_run"]) == (L, mode, R)
                for key, tab, directions, runs, clamped in (("glrlm", rlm[r], 13, rows[r]["runs"], rows[r]["clamped"]),
                                                             ("glrlm_axial", axial[r], 4, rows[r]["runs_axial"], rows[r]["clamped_axial"])):
                    want = vz.features(vz.run_cells(tab), rows[r]["voxels"], directions)
                    assert list(got[key]) == ["runs", "clamped", "longest"] + list(vz.FEATURES)
                    assert (got[key]["runs"], got[key]["clamped"]) == (runs, clamped) and got["glrlm"]["longest"] == rows[r]["longest_run"]
                    for k in vz.FEATURES:
                        assert close(got[key][k], want[k]), (c, r, key, k, got[key][k], want[k])
                want = vz.features(vz.zone_cells(zl, r), rows[r]["voxels"], 1)
                assert list(got["glszm"]) == ["zones", "largest"] + list(vz.FEATURES)
                assert (got["glszm"]["zones"], got["glszm"]["largest"]) == (rows[r]["zones"], rows[r]["largest_zone"])
                for k in vz.FEATURES:
                    assert close(got["glszm"][k], want[k]), (c, r, k, got["glszm"][k], want[k])
        return doc, seen

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log_never = run("never")
        # set and taken back: every artefact of a run that never touched the setting
        assert hostlib.set_volume_zones(True, 0, "width", 16, 10, 20, 8) and hostlib.set_volume_zones(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume zones" not in log_never + log_off
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        # zones only together with `volume on`
        assert hostlib.set_volume(False) and hostlib.set_volume_zones(True)
        log = run("alone")
        assert "Volume" not in log and not [n for n in os.listdir(dirs["alone"]) if "volume" in n]
        # on, the device route: the same files, the report gains the members and nothing else
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("on")
        assert log.count("Volume zones: 5 slices, 3 targets, ") == 1 and "Volume texture" not in log
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc, seen = check_zones("on", 32, "count")
        assert seen >= 2
        plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
        for t in doc["targets"]:
            for comp in t["components"]:
                del comp["zones"]
        assert doc == plain
        # the host route: the same report bytes
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert (dirs["host"] / "volume_report.json").read_bytes() == (dirs["on"] / "volume_report.json").read_bytes()
        # fixed bin size, 64 levels, a short last bin
        assert hostlib.set_volume_zones(True, 0, "width", 64, 40, 3, 4)
        run("width")
        check_zones("width", 64, "width", 40, 3, 4)
        # with the texture also on, "texture" precedes "zones" and is what it is without the zones
        assert hostlib.set_volume_texture(True) and hostlib.set_volume_zones(True)
        log = run("both")
        assert log.index("Volume texture: 5 slices") < log.index("Volume zones: 5 slices")
        both = json.loads((dirs["both"] / "volume_report.json").read_bytes())
        for t, t_on in zip(both["targets"], json.loads((dirs["on"] / "volume_report.json").read_bytes())["targets"]):
            for comp, comp_on in zip(t["components"], t_on["components"]):
                assert list(comp)[-2:] == ["texture", "zones"] and comp["zones"] == comp_on["zones"] and comp["texture"] is not None
        # a channel the engine does not have ends only this step: the report of a run without the setting
        assert hostlib.set_volume_texture(False) and hostlib.set_volume_zones(True, 3)
        log = run("channel")
        assert "Volume zones error: channel 3 of 1" in log
        assert (dirs["channel"] / "volume_report.json").read_bytes() == (dirs["never"] / "volume_report.json").read_bytes()
    finally:
        hostlib.set_volume_zones(False)
        hostlib.set_volume_texture(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
