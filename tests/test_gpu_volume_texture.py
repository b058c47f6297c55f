"""The volume texture on the device (include/mi_unet.h: mi_unet_volume_texture): every case of volume_texture_ref.py
equals the numpy reference cell for cell and is the host form's bytes; one engine serves growing and shrinking calls; the stage chains
with the components and the measurement stages; an engine with weights infers the same labels before and after; argument errors queue
nothing; the facade writes a "texture" member into volume_report.json."""
import numpy as np
import pytest

import volume_texture_ref as tx
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_texture_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def check(eng, name):
    """the device's result equals the reference's exactly and is the host form's bytes: table, hist and both tables"""
    got = tx.call(eng.volume_texture, name)
    tx.assert_equal(got, tx.case_ref(name), name)
    assert tx.same_bytes(got, tx.call(binding.volume_texture_host, name)), name
    return got


def test_the_cases_are_not_degenerate():
    tx.assert_not_degenerate()


@pytest.mark.parametrize("name", list(tx.cases()))
def test_device_equals_reference_and_host(name):
    """W = 72, 130, 70, 96 and 65 are no multiples of the 64-voxel tile row, H = 40, 33, 19 and 9 none of its 8 rows, D = 7, 5 and 3 none of
    its 4 slices; components touch every face of the volume; D = 1, H = 1 and one voxel; a constant component (one cell takes every
    count); two ids row by row and as a checkerboard (the component that owns the LDS tables changes, the other goes to memory); ids
    of 0, -1 and m + 1; both caps; clamping; either table NULL; a side of 8192 on each axis (the longest tile grid along it)"""
    with bare_engine() as eng:
        check(eng, name)


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state: every call gives the bytes of a
    fresh engine (the host form's); the neighbouring stage's workspace is its own"""
    import volume_ref as vr

    order = ("haralick_count", "noise(16, 24, 130)c6_noisy_L64_count", "scattered", "noise(7, 40, 72)c26_smooth_L8_width", "m4096_L32",
             "one_voxel_volume", "constant65535", "hist_only", "m1024_L64", "checkerboard")
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name)
            if i == 2:
                vr.assert_equal(eng.volume_components(vr.smooth_noise((3, 64, 64)), vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))


def test_ids_of_the_components_stage_and_the_measurement_agree_with_the_texture():
    """7.9, 7.13 and this stage chained on the device: voxels, imin and imax are what volume_measure reports for the same ids and
    intensity; each hist row sums to voxels and each table to its pairs"""
    import volume_ref as vr

    vol = vr.smooth_noise((7, 40, 72))
    inten = tx.noisy(vol.shape, 31)
    with bare_engine() as eng:
        _, _, found, _, ids = eng.volume_components(vol, (2,), 18, cap=64, want_ids=True)
        m = min(int(found[0]), 64)
        measured = eng.volume_measure(ids[0], inten, m=m, units=(1, 1, 1))
        table, hist, glcm, axial = eng.volume_texture(ids[0], inten, m, levels=16)
    assert m > 5 and table["voxels"].min() > 0
    for f in ("voxels", "imin", "imax"):
        assert np.array_equal(table[f], measured[f]), f
    assert np.array_equal(hist.sum(axis=1), table["voxels"])
    assert np.array_equal(glcm.sum(axis=(1, 2), dtype=np.int64), table["pairs"]) and table["pairs"].max() > 1000
    assert np.array_equal(axial.sum(axis=(1, 2), dtype=np.int64), table["pairs_axial"])


def test_an_engine_with_weights_infers_the_same_labels_before_and_after():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, "scattered")
        check(eng, "noise(7, 40, 72)c26_noisy_L32_count")
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_texture, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_texture, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error().startswith(b"mi_unet_volume_texture:"), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_texture, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_texture, (None,), {})
        assert rc != 0 and untouched
        check(eng, "two_in_a_slab")                              # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0), (2, 0.0)]
SPACING = (0.7, 0.7, 3.0)
TEXTURE_KEYS = ["levels", "mode", "range", "levels_used", "histogram", "glcm", "glcm_axial"]
HISTOGRAM_KEYS = ["mean", "variance", "skewness", "kurtosis", "median", "p10", "p90", "mode", "entropy", "uniformity", "counts"]


def test_facade_adds_the_texture_of_every_component_to_the_report(tmp_path, monkeypatch):
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
    dirs = {n: tmp_path / n for n in ("never", "off", "alone", "on", "host", "width", "keep", "both", "channel")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def close(got, want, scale):
        return (got is None and math.isnan(want)) or (got is not None and abs(got - want) <= 1e-12 * scale)

    def check_textures(name, L, mode, lo=0, width=1, min_voxels=0):
        """every "texture" member against derive-of-reference on the pictures this very call wrote"""
        doc = json.loads((dirs[name] / "volume_report.json").read_bytes())
        inten = read_stack(dirs[name], "s{z}_normalized.png", 0).astype(np.uint16)
        seen = 0
        for t, c in zip(doc["targets"], labels):
            stack = read_stack(dirs[name], "s{z}_mask_class{cls}.png", c)
            plane = vr.plane(stack, 255, 26, min_voxels, 0, cap=vr.MAX_TABLE)
            m = min(plane["found"], vr.MAX_TABLE)
            rows, hist, glcm, axial = tx.texture(plane["ids"], inten, m, L, mode, lo, width)
            assert len(t["components"]) == m, c
            for r, comp in enumerate(t["components"]):
                assert list(comp)[-1] == "texture"
                got = comp["texture"]
                if rows[r]["voxels"] == 0:                      # dropped by the volume filter
                    assert got is None and comp["kept"] == 0
                    continue
                seen += 1
                assert list(got) == TEXTURE_KEYS and list(got["histogram"]) == HISTOGRAM_KEYS
                assert (got["levels"], got["mode"], got["range"], got["levels_used"]) == (L, mode, [rows[r]["imin"], rows[r]["imax"]], rows[r]["levels_used"])
                assert got["histogram"]["counts"] == hist[r].tolist() and sum(got["histogram"]["counts"]) == comp["voxels"]
                for key, g, pairs in (("glcm", glcm[r], rows[r]["pairs"]), ("glcm_axial", axial[r], rows[r]["pairs_axial"])):
                    want = tx.derive(rows[r], hist[r], g)
                    assert list(got[key]) == ["pairs"] + list(tx.JOINT) and got[key]["pairs"] == pairs
                    for k in tx.JOINT:
                        scale = want["bound"].get("correlation", 0.0) if k == "correlation" else abs(want[k])
                        assert close(got[key][k], want[k], scale), (c, r, key, k, got[key][k], want[k])
                    for k in tx.QUANTILES:
                        assert got["histogram"][k] == want[k], (c, r, k)
                    for k in tx.FIRST_ORDER:
                        scale = want["bound"]["skewness"] if k == "skewness" else want[k] + 3.0 if k == "kurtosis" and want["variance"] else abs(want[k])
                        assert close(got["histogram"][k], want[k], scale), (c, r, k, got["histogram"][k], want[k])
        return doc, seen

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log_never = run("never")
        # set and taken back: every artefact of a run that never touched the setting
        assert hostlib.set_volume_texture(True, 0, "width", 16, 10, 20) and hostlib.set_volume_texture(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume texture" not in log_never + log_off
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        # texture only together with `volume on`
        assert hostlib.set_volume(False) and hostlib.set_volume_texture(True)
        log = run("alone")
        assert "Volume" not in log and not [n for n in os.listdir(dirs["alone"]) if "volume" in n]
        # on, the device route: the same files, the report gains the members and nothing else
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("on")
        assert log.count("Volume texture: 5 slices, 3 targets, ") == 1 and "Volume measure" not in log
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc, seen = check_textures("on", 32, "count")
        assert seen >= 2
        plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
        for t in doc["targets"]:
            for comp in t["components"]:
                del comp["texture"]
        assert doc == plain
        # the host route: the same report bytes
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert (dirs["host"] / "volume_report.json").read_bytes() == (dirs["on"] / "volume_report.json").read_bytes()
        # fixed bin size, 64 levels
        assert hostlib.set_volume_texture(True, 0, "width", 64, 40, 3)
        run("width")
        check_textures("width", 64, "width", 40, 3)
        # under a filter a dropped component has no member to give
        assert hostlib.set_volume(True, 26, 1500, 0, SPACING) and hostlib.set_volume_texture(True, 0, "count", 8)
        run("keep")
        _, kept = check_textures("keep", 8, "count", min_voxels=1500)
        assert 0 < kept < seen
        # with the measurement also on, "measure" precedes "texture" and is what it is without the texture
        assert hostlib.set_volume(True, 26, 0, 0, SPACING) and hostlib.set_volume_measure(True) and hostlib.set_volume_texture(True)
        log = run("both")
        assert log.index("Volume measure: 5 slices") < log.index("Volume texture: 5 slices")
        both = json.loads((dirs["both"] / "volume_report.json").read_bytes())
        for t, t_on in zip(both["targets"], json.loads((dirs["on"] / "volume_report.json").read_bytes())["targets"]):
            for comp, comp_on in zip(t["components"], t_on["components"]):
                assert list(comp)[-2:] == ["measure", "texture"] and comp["texture"] == comp_on["texture"] and comp["measure"] is not None
        # a channel the engine does not have ends only this step: the report of a run without the setting
        assert hostlib.set_volume_measure(False) and hostlib.set_volume_texture(True, 3)
        log = run("channel")
        assert "Volume texture error: channel 3 of 1" in log
        assert (dirs["channel"] / "volume_report.json").read_bytes() == (dirs["never"] / "volume_report.json").read_bytes()
    finally:
        hostlib.set_volume_texture(False)
        hostlib.set_volume_measure(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
