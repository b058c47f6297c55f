"""Volume interpolation on the device (include/mi_unet.h: mi_unet_volume_interp) against the numpy reference of
volume_interp_ref.py: the bytes of every plane and every count, exactly, and the bytes of the host form.  The inputs and cases are
volume_interp_ref's, the ones test_volume_interp_cpu.py holds the host form to: widths of 1, 63, 64, 65 and 300, one row, one and two
slices, all-set and all-empty slices, a slice whose only other pixel sits in a corner, factors 1, 2, 3, 5 and 16, units (1, 1), (2, 3),
(3, 1).  The inputs are checked for non-degeneracy on the reference alone before the device is asked."""
import numpy as np
import pytest

import volume_interp_ref as vr
from miunet import binding
from test_volume_interp_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def check(eng, masks, values, units, k, what, want=None, intensity=None):
    """the device's bytes and counts equal the reference's exactly and are the host form's bytes"""
    got = eng.volume_interp(masks, values, units, k, intensity)
    vr.assert_equal(got[0], got[1], want if want is not None else vr.interp(masks, values, units, k), what)
    host = binding.volume_interp_host(masks, values, units, k, intensity)
    assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes(), what
    if intensity is not None:
        assert np.array_equal(got[2], vr.lerp(intensity, k)) and got[2].tobytes() == host[2].tobytes(), what
    return got


def test_the_cases_are_not_degenerate():
    vr.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vr.SHAPES))
def test_device_equals_reference_and_host(name):
    """every unit pair x factor: three values of the label volume and one that is absent, and the binary case with its intensity"""
    with bare_engine() as eng:
        for units in vr.UNITS:
            for k in vr.FACTORS:
                where = f"{name} {units} k={k}"
                check(eng, vr.case(name), vr.VALUES, units, k, where, vr.case_ref(name, units, k))
                check(eng, vr.binary(name), (1,), units, k, where + " binary", vr.binary_ref(name, units, k), vr.intensity(name))


def test_units_with_a_common_factor_are_the_reduced_ones():
    with bare_engine() as eng:
        for name in ("discs", "corner"):
            out, stats = check(eng, vr.case(name), vr.VALUES, (7, 7), 3, name, vr.case_ref(name, (1, 1), 3))
            assert stats[0]["mixed"] > 0 and stats[0]["mixed_set"] > 0


def test_the_search_crosses_the_whole_row():
    """the corner case by itself: in slice 0 the far end of row 0 finds its only partner 299 columns away, and the slice pair decides
    by distances that long"""
    vol = vr.binary("corner")
    assert vol[0].sum() == vol[0].size - 1 and vol[1].sum() == 1
    e = vr.field(vol != 0, (3, 1))
    assert e[0, 0, 299] == (3 * 299) ** 2 and e[1, 0, 0] == (3 * 299) ** 2 + 39 ** 2
    with bare_engine() as eng:
        for units in vr.UNITS:
            _, stats = check(eng, vol, (1,), units, 5, f"corner {units}", vr.binary_ref("corner", units, 5))
            assert stats[0]["mixed"] == 4 * (vol[0] != vol[1]).sum() + 4 * (vol[1] != vol[2]).sum()


def test_flips_and_the_transposition_commute():
    vol, units, k = vr.case("discs"), (2, 3), 3
    with bare_engine() as eng:
        base_out, base_stats = check(eng, vol, vr.VALUES, units, k, "base", vr.case_ref("discs", units, k))
        for axis in (0, 1, 2):
            out, stats = eng.volume_interp(np.flip(vol, axis), vr.VALUES, units, k)
            assert np.array_equal(out, np.flip(base_out, 1 + axis)) and np.array_equal(stats, base_stats), axis
        out, stats = eng.volume_interp(vol.transpose(0, 2, 1), vr.VALUES, units[::-1], k)
        assert np.array_equal(out, base_out.transpose(0, 1, 3, 2)) and np.array_equal(stats, base_stats)


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state (the counts and the slice flags of
    a smaller call lie inside what a larger one left behind); the neighbouring stages' workspaces are their own"""
    import volume_clean_ref as cr
    import volume_ref as vol_ref

    calls = [("d2", (1, 1), 2, False), ("corner", (2, 3), 16, True), ("d2", (1, 1), 2, False), ("slabs", (3, 1), 5, True), ("w1", (1, 1), 3, False),
             ("discs", (2, 3), 3, True), ("d1", (1, 1), 16, False)]
    noise = vol_ref.smooth_noise((3, 64, 64))
    shape, cunits = cr.SHAPES[3], cr.UNITS[1]
    pair = cr.radius_pairs(cunits)[0]
    with bare_engine(32, 32) as eng:
        for i, (name, units, k, with_intensity) in enumerate(calls):
            check(eng, vr.case(name), vr.VALUES, units, k, f"call {i}", vr.case_ref(name, units, k), vr.intensity(name) if with_intensity else None)
            if i == 1:
                vol_ref.assert_equal(eng.volume_components(noise, vol_ref.NOISE_VALUES, 26, want_ids=True), vol_ref.noise_ref((3, 64, 64), 26))
            if i == 3:
                out, stats = eng.volume_clean(cr.case(shape), cr.VALUES, cunits, True, pair[0], pair[1])
                cr.assert_equal(out, stats, cr.case_ref(shape, cunits, pair, True))


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_interp, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_interp, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error().startswith(b"mi_unet_volume_interp:"), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_interp, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_interp, (None,), {})
        assert rc != 0 and untouched
        check(eng, vr.case("noise"), vr.VALUES, (2, 3), 3, "after the refusals", vr.case_ref("noise", (2, 3), 3))      # the engine still works


# ---- the facade: five RAW slices through process_image_batch -----------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0)]
SPACING = (0.7, 0.7, 3.0)
FACTOR = 3


def series_labels(z):
    """five 64 x 64 label maps: class 1 -- a disc whose radius and centre change from slice to slice, absent in the last one; class 3 --
    a block over slices 1 .. 3 that moves by three pixels a slice"""
    m = np.zeros((64, 64), np.uint8)
    if z < 4:
        m[vr.disc(64, 64, 20 + 2 * z, 22 + 3 * z, (6, 13, 9, 4)[z])] = 1
    if 1 <= z <= 3:
        m[44:56, 5 + 3 * z:25 + 3 * z] = 3
    m[0, 0], m[63, 63] = 0, 3                              # both ends of the grey range (test_gpu_targets.raw_of)
    return m


def test_facade_interpolates_the_stack_the_mesh_sees(tmp_path, monkeypatch):
    import json
    import os

    from miunet import hostlib
    from test_gpu_targets import blob, raw_of
    from test_gpu_volume import read_stack
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
    units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
    dirs = {n: tmp_path / n for n in ("never", "off", "on", "host", "iso", "nomesh")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def timeless(log, name):
        import re
        return re.sub(r"[0-9.]+", "#", log.replace(str(dirs[name]), "DIR"))

    stls = [f"volume_mesh_class{c}.stl" for c in labels]
    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING) and hostlib.set_volume_mesh(True, "nets")
        log_never = run("never")
        # set and taken back: every artefact and every log line of a run that never touched the setting; no "interp" member
        assert hostlib.set_volume_interp(True, FACTOR) and hostlib.set_volume_interp(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and set(stls) <= set(names)
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        assert "Volume interp" not in log_never and "Volume interp" not in log_off
        assert timeless(log_off, "off") == timeless(log_never, "never")
        plain = json.loads((dirs["off"] / "volume_report.json").read_bytes())
        assert "interp" not in plain and "mesh" in plain
        # on: the same files; the report gains "interp" in front of "mesh"; the mesh is that of the interpolated stack
        assert hostlib.set_volume_interp(True, FACTOR)
        log = run("on")
        assert log.count("Volume interp: 5 slices -> 13, 2 targets, factor 3, ") == 1 and log.count("Volume mesh: 13 slices, 2 targets, nets, ") == 1
        assert log.index("Volume interp:") < log.index("Volume mesh:")
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_report.json" and n not in stls:
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc = json.loads((dirs["on"] / "volume_report.json").read_bytes())
        assert list(doc) == list(plain)[:-1] + ["interp", "mesh"]
        for key in plain:
            if key != "mesh":
                assert doc[key] == plain[key], key                              # components stay on the original slices
        interp = doc["interp"]
        assert list(interp) == ["factor", "slices", "spacing_z_mm", "targets"]
        assert (interp["factor"], interp["slices"], interp["spacing_z_mm"]) == (FACTOR, 13, SPACING[2] / FACTOR)
        for t, c, mesh_t, plain_t in zip(interp["targets"], labels, doc["mesh"]["targets"], plain["mesh"]["targets"]):
            stack = read_stack(dirs["on"], "s{z}_mask_class{cls}.png", c)       # the pictures this very call wrote
            ref_out, ref_stats = vr.interp(stack, (255,), units[:2], FACTOR)
            h_out, h_stats = binding.volume_interp_host(stack, (255,), units[:2], FACTOR)
            vr.assert_equal(h_out, h_stats, (ref_out, ref_stats), f"class {c}")
            want = dict(label=c, **{f: int(h_stats[0][f]) for f in ("in_voxels", "out_voxels", "mixed", "ties")})
            want["volume_mm3"] = int(h_stats[0]["out_voxels"]) * SPACING[0] * SPACING[1] * SPACING[2] / FACTOR
            assert t == want and t["mixed"] > 0 and t["out_voxels"] > t["in_voxels"], c
            # the mesh of the interpolated stack, under spacing_z / factor
            meshes, mstats = binding.volume_mesh_host(ref_out[0], (255,), "nets")
            m = binding.volume_mesh_derive(meshes[0][0], meshes[0][1], (SPACING[0], SPACING[1], SPACING[2] / FACTOR))
            assert (mesh_t["quads"], mesh_t["verts"]) == (int(mstats[0]["quads"]), int(mstats[0]["verts"])) and mesh_t["quads"] != plain_t["quads"]
            assert mesh_t["area_mm2"] == m["area_mm2"] and mesh_t["volume_mm3"] == m["volume_mm3"]
        # the host form under MEDSEG_HOST_POSTPROCESS=1: the same report and STL bytes
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        for n in ["volume_report.json"] + stls:
            assert (dirs["host"] / n).read_bytes() == (dirs["on"] / n).read_bytes(), n
            assert (dirs["on"] / n).read_bytes() != (dirs["never"] / n).read_bytes(), n
        # iso: llround(3.0 / 0.7) = 4
        assert hostlib.set_volume_interp(True, "iso")
        assert "Volume interp: 5 slices -> 17, 2 targets, factor 4, " in run("iso")
        iso = json.loads((dirs["iso"] / "volume_report.json").read_bytes())["interp"]
        assert (iso["factor"], iso["slices"], iso["spacing_z_mm"]) == (4, 17, SPACING[2] / 4)
        # without the mesh the report still gains the object and nothing else changes; without `volume on` nothing happens
        assert hostlib.set_volume_mesh(False) and hostlib.set_volume_interp(True, FACTOR)
        run("nomesh")
        nomesh = json.loads((dirs["nomesh"] / "volume_report.json").read_bytes())
        assert nomesh["interp"] == interp and "mesh" not in nomesh and not [n for n in os.listdir(dirs["nomesh"]) if n.endswith(".stl")]
        assert hostlib.set_volume(False)
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs["nomesh"])) == 5
        assert "Volume" not in open(hostlib.get_log_path(), "rb").read()[before:].decode()
    finally:
        hostlib.set_volume_interp(False)
        hostlib.set_volume_mesh(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
