"""The volume neighbourhoods on the device (include/mi_unet.h: mi_unet_volume_nbhood): every case of
volume_nbhood_ref.py equals the numpy reference cell for cell and is the host form's bytes; a checkerboard of 10^7 voxels equals its
closed form, one cell above 2^32; both forms of the gather kernel give the same bytes; one engine serves growing and shrinking calls;
the stage chains with the components, the measurement, the texture and the zones stages; an engine with weights infers the same labels
before and after; argument errors queue nothing; the facade writes a "nbhood" member into volume_report.json."""
import numpy as np
import pytest

import volume_nbhood_ref as nb
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_nbhood_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def check(eng, name):
    """the device's result equals the reference's exactly and is the host form's bytes: the entries and every table"""
    got = nb.call(eng.volume_nbhood, name)
    nb.assert_equal(got, nb.case_ref(name), name)
    assert nb.same_bytes(got, nb.call(binding.volume_nbhood_host, name)), name
    return got


def test_the_cases_are_not_degenerate():
    nb.assert_not_degenerate()


@pytest.mark.parametrize("name", list(nb.cases()))
def test_device_equals_reference_and_host(name):
    """W = 72, 130, 140 and 150 are no multiples of the 64-voxel tile row, H = 9, 19, 21 and 40 none of its 8 rows, D = 3, 5, 7, 9 and 11
    none of its 4 slices; D = 1, H = 1 and one voxel; a solid box over several tiles on every axis; two ids that touch along a plane and
    two interleaved inside one 64-lane row; a component flush with every face; a hollow shell; a diagonal line through a tile's corner;
    zones Dm - 1, Dm and Dm + 1 deep; Dm = 1 and 4096; alpha = 0, 1 and L - 1; ids of 0, -1 and m + 1; both ends of the cell limit; each
    output NULL in turn and all of them"""
    with bare_engine() as eng:
        check(eng, name)


def test_a_checkerboard_of_ten_million_voxels_passes_2_32_in_one_cell():
    """the 64-bit sums: 40 x 512 x 512 of levels 0 and 63 by parity against the closed form (test_volume_nbhood_cpu.py holds the host
    form to the same numbers); with the zone half on, the two zones, both at distance 1, and the box's closed-form depth"""
    ids, inten = nb.parity_volume()
    with bare_engine() as eng:
        table, tabs = eng.volume_nbhood(ids, inten, 1, levels=64, mode="width", lo=0, width=1)
    assert int(tabs["ngt_diff"][0, 0, 26]) == 882 * 38 * 510 * 510 // 2 > 1 << 32
    for name, ref in nb.parity_closed_form().items():
        assert np.array_equal(tabs[name].astype(np.int64), ref), name
    row = table[0]
    assert (int(row["voxels"]), int(row["valid"]), int(row["valid_axial"]), int(row["dependence_max"])) == (40 * 512 * 512,) * 3 + (13,)
    assert (int(row["zones"]), int(row["deepest"]), int(row["deepest_axial"]), int(row["clamped"])) == (2, nb.box_deepest(40, 512, 512), 256, 0)
    assert tabs["dzm"][0, :, 0].tolist() == [1] + [0] * 62 + [1] and tabs["dzm"].sum() == 2 and tabs["dzm_axial"][0, :, 0].sum() == 2


@pytest.mark.parametrize("form", ["1", "2"])
def test_both_forms_of_the_gather_give_the_reference(form, monkeypatch):
    """MIUNET_VNB_EXP=1 sends every count of k_vnb_gather to memory, 2 keeps the leading component's in LDS (one of them is what ships):
    large components that own the LDS tables over many tiles, tiles of several ids where the tables change hands or stay where they
    are, ids of more components than a tile has rows, 64 levels"""
    monkeypatch.setenv("MIUNET_VNB_EXP", form)
    with bare_engine() as eng:
        for name in ("solid_box", "thick(16, 24, 130)", "two_ids_interleaved", "scattered", "m1024_L64", "noise(7, 40, 72)_smooth_L64_width", "without_ngt"):
            check(eng, name)


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state: every call gives the bytes of a
    fresh engine (the host form's); the neighbouring stages' workspaces are their own"""
    import volume_ref as vr
    import volume_zones_ref as vz

    order = ("hand_4x4", "noise(16, 24, 130)_smooth_L32_count", "scattered", "thick(7, 40, 72)", "m4096_L32", "one_voxel_volume", "solid_box",
             "entry_only", "m1_L64_Dm4096", "without_dzm", "dzm_axial_only", "thick(16, 24, 130)", "diagonal_line")
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name)
            if i == 2:
                vr.assert_equal(eng.volume_components(vr.smooth_noise((3, 64, 64)), vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))
            if i == 5:
                vz.assert_equal(vz.call(eng.volume_zones, "scattered"), vz.case_ref("scattered"), "zones between")


def test_ids_of_the_components_stage_the_measurement_the_texture_and_the_zones_agree():
    """7.9, 7.13 and this stage chained on the device: voxels, imin and imax are what volume_measure reports for the same ids and
    intensity; zones is what volume_zones counts; ngt_count summed over c is 7.15's histogram"""
    import volume_ref as vr
    import volume_texture_ref as tx

    vol = vr.smooth_noise((7, 40, 72))
    inten = tx.smooth(vol.shape, 31)
    with bare_engine() as eng:
        _, _, found, _, ids = eng.volume_components(vol, (2,), 18, cap=64, want_ids=True)
        m = min(int(found[0]), 64)
        measured = eng.volume_measure(ids[0], inten, m=m, units=(1, 1, 1))
        table, tabs = eng.volume_nbhood(ids[0], inten, m, levels=16, alpha=1)
        zones = eng.volume_zones(ids[0], inten, m, levels=16, want_runs=False, want_axial=False)[0]
        hist = eng.volume_texture(ids[0], inten, m, levels=16, want=())[1]
    assert m > 5 and table["voxels"].min() > 0
    for f in ("voxels", "imin", "imax"):
        assert np.array_equal(table[f], measured[f]), f
    assert np.array_equal(table["zones"], zones["zones"]) and table["zones"].sum() > m
    assert np.array_equal(tabs["ngt_count"].sum(axis=2), hist) and np.array_equal(tabs["ngt_count_axial"].sum(axis=2), hist)
    assert np.array_equal(tabs["dep"].sum(axis=2), hist) and np.array_equal(tabs["dzm"].sum(axis=(1, 2)), table["zones"])


def test_an_engine_with_weights_infers_the_same_labels_before_and_after():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, "scattered")
        check(eng, "thick(7, 40, 72)")
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_nbhood, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_nbhood, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error().startswith(b"mi_unet_volume_nbhood:"), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_nbhood, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_nbhood, (None,), {})
        assert rc != 0 and untouched
        check(eng, "two_ids_plane")                              # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0), (2, 0.0)]
SPACING = (0.7, 0.7, 3.0)
NBHOOD_KEYS = ["levels", "mode", "alpha", "max_dist", "ngtdm", "ngtdm_axial", "ngldm", "ngldm_axial", "gldzm", "gldzm_axial", "deepest", "deepest_axial"]


def test_facade_adds_the_nbhood_of_every_component_to_the_report(tmp_path, monkeypatch):
    import json
    import math
    import os

    import volume_ref as vr
    import volume_zones_ref as vz
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

    def check_nbhood(name, eng, L, mode, lo=0, width=1, alpha=0, Dm=32):
        """every "nbhood" member against the direct call (whose tables are the reference's) and the features in Python, on the pictures
        this very call wrote"""
        doc = json.loads((dirs[name] / "volume_report.json").read_bytes())
        inten = read_stack(dirs[name], "s{z}_normalized.png", 0).astype(np.uint16)
        seen = 0
        for t, c in zip(doc["targets"], labels):
            stack = read_stack(dirs[name], "s{z}_mask_class{cls}.png", c)
            plane = vr.plane(stack, 255, 26, 0, 0, cap=vr.MAX_TABLE)
            m = min(plane["found"], vr.MAX_TABLE)
            assert len(t["components"]) == m, c
            if not m:
                continue
            table, tabs = eng.volume_nbhood(plane["ids"], inten, m, L, mode, lo, width, alpha, Dm)
            rows, rtabs = nb.nbhood(plane["ids"], inten, m, L, mode, lo, width, alpha, Dm)
            nb.assert_equal((table, tabs), (rows, rtabs), f"facade {name} {c}")
            for r, comp in enumerate(t["components"]):
                assert list(comp)[-1] == "nbhood"
                got = comp["nbhood"]
                seen += 1
                assert list(got) == NBHOOD_KEYS and (got["levels"], got["mode"], got["alpha"], got["max_dist"]) == (L, mode, alpha, Dm)
                assert (got["deepest"], got["deepest_axial"]) == (rows[r]["deepest"], rows[r]["deepest_axial"])
                for sfx, axial in (("", False), ("_axial", True)):
                    want = nb.derive(rows[r], {n: rtabs[n][r] for n in nb.TABLES}, axial)
                    g = got["ngtdm" + sfx]
                    assert list(g) == ["valid"] + list(nb.NGTDM) and g["valid"] == rows[r]["valid" + sfx]
                    for k in nb.NGTDM:
                        assert close(g[k], want[k]), (c, r, sfx, k, g[k], want[k])
                    g = got["ngldm" + sfx]
                    assert list(g) == ["dependence_max"] + list(vz.FEATURES) + ["dependence_energy"] and g["dependence_max"] == rows[r]["dependence_max"]
                    assert close(g["dependence_energy"], want["dependence_energy"])
                    for k in vz.FEATURES:
                        assert close(g[k], want["ngldm"][k]), (c, r, sfx, k, g[k], want["ngldm"][k])
                    g = got["gldzm" + sfx]
                    assert list(g) == ["zones", "clamped"] + list(vz.FEATURES)
                    assert (g["zones"], g["clamped"]) == (rows[r]["zones"], rows[r]["clamped" + sfx])
                    for k in vz.FEATURES:
                        assert close(g[k], want["gldzm"][k]), (c, r, sfx, k, g[k], want["gldzm"][k])
        return doc, seen

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log_never = run("never")
        # set and taken back: every artefact of a run that never touched the setting
        assert hostlib.set_volume_nbhood(True, 0, "width", 16, 10, 20, 2, 8) and hostlib.set_volume_nbhood(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume nbhood" not in log_never + log_off
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        # nbhood only together with `volume on`
        assert hostlib.set_volume(False) and hostlib.set_volume_nbhood(True)
        log = run("alone")
        assert "Volume" not in log and not [n for n in os.listdir(dirs["alone"]) if "volume" in n]
        # on, the device route: the same files, the report gains the members and nothing else
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("on")
        assert log.count("Volume nbhood: 5 slices, 3 targets, ") == 1 and "Volume zones" not in log
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        with bare_engine() as eng:
            doc, seen = check_nbhood("on", eng, 32, "count")
            assert seen >= 2
            plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
            for t in doc["targets"]:
                for comp in t["components"]:
                    del comp["nbhood"]
            assert doc == plain
            # the host route: the same report bytes
            monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
            run("host")
            monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
            assert (dirs["host"] / "volume_report.json").read_bytes() == (dirs["on"] / "volume_report.json").read_bytes()
            # fixed bin size, 64 levels, a tolerance, a short last bin
            assert hostlib.set_volume_nbhood(True, 0, "width", 64, 40, 3, 2, 2)
            run("width")
            check_nbhood("width", eng, 64, "width", 40, 3, 2, 2)
        # with the zones also on, "zones" precedes "nbhood" and is what it is without the neighbourhoods
        assert hostlib.set_volume_zones(True) and hostlib.set_volume_nbhood(True)
        log = run("both")
        assert log.index("Volume zones: 5 slices") < log.index("Volume nbhood: 5 slices")
        both = json.loads((dirs["both"] / "volume_report.json").read_bytes())
        for t, t_on in zip(both["targets"], json.loads((dirs["on"] / "volume_report.json").read_bytes())["targets"]):
            for comp, comp_on in zip(t["components"], t_on["components"]):
                assert list(comp)[-2:] == ["zones", "nbhood"] and comp["nbhood"] == comp_on["nbhood"] and comp["zones"] is not None
        # a channel the engine does not have ends only this step: the report of a run without the setting
        assert hostlib.set_volume_zones(False) and hostlib.set_volume_nbhood(True, 3)
        log = run("channel")
        assert "Volume nbhood error: channel 3 of 1" in log
        assert (dirs["channel"] / "volume_report.json").read_bytes() == (dirs["never"] / "volume_report.json").read_bytes()
    finally:
        hostlib.set_volume_nbhood(False)
        hostlib.set_volume_zones(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
