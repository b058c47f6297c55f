"""The volume spatial statistics on the device (include/mi_unet.h: mi_unet_volume_spatial): every case of
volume_spatial_ref.py equals the brute-force numpy reference in every integer field, is the host form's bytes over the integer part
of the table and has its four pair sums within the derived bound; a search of more than one launch; two calls give the same bytes;
one engine serves growing and shrinking calls; an engine with weights infers the same labels before and after; argument errors queue
nothing."""
import numpy as np
import pytest

import volume_spatial_ref as sp
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_spatial_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def int_bytes(table):
    """the integer part of every entry"""
    return table.view(np.uint8).reshape(len(table), sp.STRUCT_BYTES)[:, :sp.INT_BYTES].tobytes()


def check(eng, name):
    """the device's integers equal the reference's and are the host form's bytes; its sums are within (P + 8) eps T of the reference"""
    got, ref = sp.call(eng.volume_spatial, name), sp.case_ref(name)
    sp.assert_ints_equal(got, ref, name)
    assert int_bytes(got) == int_bytes(sp.call(binding.volume_spatial_host, name)), name
    sp.assert_sums_near_reference(got, ref, name)
    return got


def test_the_cases_are_not_degenerate():
    sp.assert_not_degenerate()


@pytest.mark.parametrize("name", list(sp.cases()))
def test_device_equals_reference_and_host(name):
    """the ellipsoid under two unit sets; W = 72 and 130 are no multiples of 64 and rows cross the 64-lane segments; D = 1; ids of 0, -1
    and m + 1; A = 1, 2 and round the tile; interleaved components; m = 4096; the caps; constant intensity; the clipped spheres"""
    with bare_engine() as eng:
        got = check(eng, name)
        if name == "constant":                                  # y == 0 everywhere: exact zeros, and the rational tie rule
            assert (got[0]["s1"], got[0]["s2"], got[0]["s3"]) == (0.0, 0.0, 0.0) and got[0]["gp_at"] == 0 and got[0]["lp_at"] == 0
        if name.startswith("blob_cap") and name != f"blob_cap{sp.BLOB_VOXELS}":
            full = sp.call(eng.volume_spatial, f"blob_cap{sp.BLOB_VOXELS}")[0]
            for f in sp.INT_FIELDS:
                if f not in ("searched", "pairs"):
                    assert got[0][f] == full[f], f


def test_a_search_of_more_than_one_launch_equals_the_host_form():
    """a full box 16 x 48 x 32 is one component of 24576 voxels: 3.02e8 pairs, more than one launch of the pair sums may hold, over 96
    tiles.  (The all-pairs reference is not run here; the host form is compared with it on every other case.)"""
    ids = np.ones((16, 48, 32), np.int32)
    inten = sp.intensity_for(ids.shape, 8)
    with bare_engine() as eng:
        got = eng.volume_spatial(ids, inten, m=1, units=(3, 3, 10), peak_r=9)
    assert got[0]["voxels"] == 24576 and got[0]["searched"] == 1 and got[0]["pairs"] == 24576 * 24575 // 2 > 1 << 28
    host = binding.volume_spatial_host(ids, inten, m=1, units=(3, 3, 10), peak_r=9)
    assert int_bytes(got) == int_bytes(host)
    sp.assert_sums_near_each_other(got, host, "box")


def test_two_calls_give_the_same_bytes():
    """doubles included: the points are in index order whatever order the fill left, and every sum is added up in a fixed order"""
    with bare_engine() as eng:
        for name in ("ellipsoid(7, 7, 50)", "scattered", "noise(7, 40, 72)c26"):
            first = sp.call(eng.volume_spatial, name).tobytes()
            for _ in range(3):
                assert sp.call(eng.volume_spatial, name).tobytes() == first, name
    with bare_engine() as other:
        assert sp.call(other.volume_spatial, "noise(7, 40, 72)c26").tobytes() == first


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state; the neighbouring stage's
    workspace is its own"""
    import volume_ref as vr

    order = ("constant", "noise(16, 24, 130)c6", "scattered", "noise(7, 40, 72)c26", "ellipsoid(1, 1, 1)", "constant", "m4096", "blob_cap0",
             "peak_r0")
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name)
            if i == 2:
                vr.assert_equal(eng.volume_components(vr.smooth_noise((3, 64, 64)), vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))


def test_ids_of_the_components_stage_give_what_its_table_counts():
    """the two stages chained on the device: voxels and the first sums of the table are the components table's"""
    import volume_ref as vr

    vol = vr.smooth_noise((7, 40, 72))
    with bare_engine() as eng:
        _, table, found, _, ids = eng.volume_components(vol, (2,), 18, cap=64, want_ids=True)
        m = min(int(found[0]), 64)
        got = eng.volume_spatial(ids[0], sp.intensity_for(vol.shape, 9), m=m, units=(1, 1, 1), max_voxels=500, peak_r=2)
    for f in ("voxels", "sx", "sy", "sz"):
        assert np.array_equal(got[f], table[0][f][:m]), f
    assert (got["gp_at"] >= table[0]["first"][:m]).all() and (got["lp_at"] >= table[0]["first"][:m]).all()     # `first` is the raster-first voxel


def test_an_engine_with_weights_infers_the_same_labels_before_and_after():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, "scattered")
        check(eng, "noise(7, 40, 72)c26")
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_spatial, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_spatial, (eng._h,), case)
            assert rc == 1 and untouched and b"mi_unet_volume_spatial:" in L.mi_unet_last_error(), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_spatial, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_spatial, (None,), {})
        assert rc != 0 and untouched
        check(eng, "constant")                                   # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0), (2, 0.0)]
SPACING = (0.7, 0.7, 3.0)
SPATIAL_KEYS = ["morans_i", "gearys_c", "pairs", "com_shift_mm", "intensity_centroid_mm", "integrated_intensity", "local_peak", "local_peak_at",
                "global_peak", "global_peak_at"]


def test_facade_adds_the_spatial_member_to_every_component_of_the_report(tmp_path, monkeypatch):
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

    def number(v):
        return None if math.isnan(v) else v

    def check_members(name, direct, max_voxels, peak_mm=hostlib.VSPATIAL_DEFAULT_PEAK_MM, min_voxels=0):
        """every "spatial" member against derive of a direct call (`direct`: the device or the host form) on the ids of the pictures this
        very call wrote"""
        doc = json.loads((dirs[name] / "volume_report.json").read_bytes())
        inten = read_stack(dirs[name], "s{z}_normalized.png", 0).astype(np.uint16)
        units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
        peak_r = int(math.floor(peak_mm / unit_mm + 0.5))
        seen = skipped = 0
        for t, c in zip(doc["targets"], labels):
            stack = read_stack(dirs[name], "s{z}_mask_class{cls}.png", c)
            plane = vr.plane(stack, 255, 26, min_voxels, 0, cap=vr.MAX_TABLE)
            m = min(plane["found"], vr.MAX_TABLE)
            assert len(t["components"]) == m, c
            if m == 0:
                continue
            rows = direct(plane["ids"], inten, m=m, units=units, max_voxels=max_voxels, peak_r=peak_r)
            for comp, row in zip(t["components"], rows):
                assert list(comp)[-1] == "spatial"
                got = comp["spatial"]
                if row["voxels"] == 0:                          # dropped by the volume filter
                    assert got is None and comp["kept"] == 0
                    continue
                seen += 1
                want = binding.volume_spatial_derive(row, units, unit_mm)
                assert list(got) == SPATIAL_KEYS and got["pairs"] == row["pairs"]
                assert got["local_peak_at"] == xyz(int(row["lp_at"])) and got["global_peak_at"] == xyz(int(row["gp_at"]))
                for k in ("morans_i", "gearys_c", "com_shift_mm", "integrated_intensity", "local_peak", "global_peak"):
                    assert got[k] == number(want[k]), (name, k, got[k], want[k])            # 17 digits: the same double
                assert got["intensity_centroid_mm"] == [number(want[k]) for k in ("icx_mm", "icy_mm", "icz_mm")]
                if not row["searched"]:
                    skipped += 1
                    assert got["morans_i"] is None and got["gearys_c"] is None and got["pairs"] == 0
        return doc, seen, skipped

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log_never = run("never")
        # set and taken back: every artefact of a run that never touched the setting
        assert hostlib.set_volume_spatial(True, 0, 1000, 3.0) and hostlib.set_volume_spatial(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume spatial" not in log_never + log_off
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        # only together with `volume on`
        assert hostlib.set_volume(False) and hostlib.set_volume_spatial(True)
        log = run("alone")
        assert "Volume" not in log and not [n for n in os.listdir(dirs["alone"]) if "volume" in n]
        # on, the device route: the same files, the report gains the members and nothing else
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("on")
        assert log.count("Volume spatial: 5 slices, 3 targets, ") == 1
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        with bare_engine() as eng:
            doc, seen, _ = check_members("on", eng.volume_spatial, sp.DEFAULT_MAX_VOXELS)
        assert seen >= 2
        plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
        for t in doc["targets"]:
            for comp in t["components"]:
                del comp["spatial"]
        assert doc == plain
        # the host route: the host form's numbers
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        _, seen_host, _ = check_members("host", binding.volume_spatial_host, sp.DEFAULT_MAX_VOXELS)
        assert seen_host == seen
        # a cap below the largest component's voxels and a smaller sphere: its two statistics are null, the rest of the member stays
        assert hostlib.set_volume_spatial(True, 0, 40, 2.0)
        run("capped")
        with bare_engine() as eng:
            _, _, skipped = check_members("capped", eng.volume_spatial, 40, 2.0)
        assert skipped >= 1
        # under a filter a dropped component has no member to give
        assert hostlib.set_volume(True, 26, 1500, 0, SPACING) and hostlib.set_volume_spatial(True)
        run("keep")
        with bare_engine() as eng:
            _, kept, _ = check_members("keep", eng.volume_spatial, sp.DEFAULT_MAX_VOXELS, min_voxels=1500)
        assert 0 < kept < seen
        # a channel the engine does not have ends only this step: the report of a run without the setting
        assert hostlib.set_volume(True, 26, 0, 0, SPACING) and hostlib.set_volume_spatial(True, 3)
        log = run("channel")
        assert "Volume spatial error: channel 3 of 1" in log
        assert (dirs["channel"] / "volume_report.json").read_bytes() == (dirs["never"] / "volume_report.json").read_bytes()
    finally:
        hostlib.set_volume_spatial(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
