"""The volume mesh on the device (include/mi_unet.h: mi_unet_volume_mesh) against the numpy reference of
volume_mesh_ref.py: every vertex, every quad and every count, exactly, and the bytes of the host form.  The inputs are
volume_mesh_ref's, the ones test_volume_mesh_cpu.py holds the host form to; they are small and cross every boundary the kernels have:
rows that are no multiple of a wave, volumes of many workgroups, a scan of two levels.  The inputs are checked for non-degeneracy on
the reference alone before the device is asked."""
import ctypes as C

import numpy as np
import pytest

import volume_mesh_ref as mr
from miunet import binding
from test_volume_mesh_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def check(eng, masks, values, what, want=None):
    """under both placements the device's mesh and counts equal the reference's exactly and are the host form's bytes"""
    for pname, placement in mr.PLACEMENTS:
        where = f"{what} {pname}"
        got = eng.volume_mesh(masks, values, pname)
        mr.assert_equal(got, want[placement] if want is not None else mr.mesh(masks, values, placement), where)
        host = binding.volume_mesh_host(masks, values, pname)
        assert got[1].tobytes() == host[1].tobytes(), where
        for (gv, gq), (hv, hq) in zip(got[0], host[0]):
            assert gv.tobytes() == hv.tobytes() and gq.tobytes() == hq.tobytes(), where


def test_the_cases_are_not_degenerate():
    mr.assert_not_degenerate()


def test_known_answers():
    with bare_engine() as eng:
        for name, masks, values, (nv, nq) in mr.known_answers():
            check(eng, masks, values, name)
            stats = eng.volume_mesh(masks, values, "nets")[1]
            assert (int(stats[0]["verts"]), int(stats[0]["quads"])) == (nv, nq), name


@pytest.mark.parametrize("shape", mr.NOISE_SHAPES + (mr.FLAT_SHAPE,))
def test_device_equals_reference_and_host_on_noise(shape):
    """three values per call; W = 72 and 130 are no multiples of 64, the one-slice shape has D = 1; the noise touches all six faces"""
    with bare_engine() as eng:
        check(eng, mr.noise(shape), mr.NOISE_VALUES, str(shape), {p: mr.noise_ref(shape, p) for _, p in mr.PLACEMENTS})


def test_two_shells_across_many_workgroups_and_two_scan_levels():
    """24 x 44 x 640: 2640 workgroups of voxels and 2817 of corners, so both scans take their second level; the outer shell touches
    all six faces of the volume"""
    vol = mr.two_shells()
    assert vol.size // 256 > 1024 and vol[0].all() and vol[:, 0].all() and vol[:, :, 0].all()
    with bare_engine() as eng:
        check(eng, vol, (1,), "two shells")


def test_checkerboard_has_six_quads_per_voxel():
    vol = mr.checkerboard((6, 9, 70))
    with bare_engine() as eng:
        check(eng, vol, (1, 0), "checkerboard")
        stats = eng.volume_mesh(vol, (1,), "nets")[1]
    assert stats[0]["quads"] == 6 * int(vol.sum())


def test_caps_do_not_change_the_prefixes_or_the_counts():
    shape = mr.NOISE_SHAPES[0]
    vol = mr.noise(shape)
    ref = mr.noise_ref(shape, mr.NETS)
    nv, nq = min(r[0].size for r in ref), min(r[1].shape[0] for r in ref)
    L = binding.lib()
    with bare_engine() as eng:
        for cap in ((nv // 2, nq // 2), (0, nq // 2), (nv // 2, 0), (0, 0), (7, 1 << 16), (1 << 16, 7)):
            got = eng.volume_mesh(vol, mr.NOISE_VALUES, "nets", cap=cap)
            mr.assert_equal(got, ref, f"caps {cap}", cap[0], cap[1])
            verts, quads, stats = eng.volume_mesh(vol, mr.NOISE_VALUES, "nets", cap=cap, raw=True)
            for k, (rv, rq, _) in enumerate(ref):                  # the zero tails
                assert not verts[k, min(rv.size, cap[0]):].tobytes().strip(b"\0") and not quads[k, min(rq.shape[0], cap[1]):].any(), (cap, k)
        # a kept quad keeps its true indices where they are >= cap_verts
        (_, gq), = eng.volume_mesh(vol, (1,), "nets", cap=(3, nq))[0]
        assert np.array_equal(gq, ref[0][1][:nq]) and gq.max() >= 3
        # NULL arrays: the counting call
        stats = np.zeros(3, binding.MESH_STAT_DTYPE)
        vals = np.array(mr.NOISE_VALUES, np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.mi_unet_volume_mesh(eng._h, ptr(np.ascontiguousarray(vol)), *shape, ptr(vals), 3, 1, None, 0, None, 0, ptr(stats)) == 0
        for k, (_, _, rs) in enumerate(ref):
            assert all(int(stats[k][f]) == rs[f] for f in mr.STAT_FIELDS), k


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state; the neighbouring stages'
    workspaces are their own"""
    import volume_clean_ref as cr
    import volume_ref as vr

    small, big = mr.FLAT_SHAPE, mr.NOISE_SHAPES[2]
    noise = vr.smooth_noise((3, 64, 64))
    units = cr.UNITS[1]
    pair = cr.radius_pairs(units)[0]
    with bare_engine(32, 32) as eng:
        for i, shape in enumerate((small, big, small, mr.NOISE_SHAPES[0], small)):
            check(eng, mr.noise(shape), mr.NOISE_VALUES, f"call {i}", {p: mr.noise_ref(shape, p) for _, p in mr.PLACEMENTS})
            if i == 1:
                vr.assert_equal(eng.volume_components(noise, vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))
            if i == 2:
                out, stats = eng.volume_clean(cr.case(cr.SHAPES[1]), cr.VALUES, units, True, pair[0], pair[1])
                cr.assert_equal(out, stats, cr.case_ref(cr.SHAPES[1], units, pair, True))


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_mesh, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_mesh, (eng._h,), case)
            assert rc == 1 and untouched and b"mi_unet_volume_mesh:" in L.mi_unet_last_error(), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_mesh, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_mesh, (None,), {})
        assert rc != 0 and untouched
        check(eng, mr.noise(mr.FLAT_SHAPE), mr.NOISE_VALUES, "after the refusals")       # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0), (2, 0.0)]
SPACING = (0.7, 0.7, 3.0)


def parse_stl(data):
    """(normals float32 [T, 3], vertices float32 [T, 3, 3]) of a binary STL; the header, the count and the attributes are checked"""
    assert data[:18] == b"medseg volume mesh" and not data[18:80].strip(b"\0")
    count = int(np.frombuffer(data[80:84], "<u4")[0])
    assert len(data) == 84 + 50 * count
    rec = np.frombuffer(data[84:], np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    assert not rec["attr"].any()
    return rec["n"], rec["v"]


def test_facade_writes_the_labelled_stack_as_stl(tmp_path, monkeypatch):
    import json
    import os

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
    dirs = {n: tmp_path / n for n in ("never", "off", "alone", "on", "host", "faces", "keep")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def check_meshes(name, pname, placement, pattern):
        """the report's "mesh" object and every STL file against the reference on the pictures this very call wrote"""
        doc = json.loads((dirs[name] / "volume_report.json").read_bytes())
        assert list(doc)[-2:] == ["targets", "mesh"] and doc["mesh"]["placement"] == pname
        assert [t["label"] for t in doc["mesh"]["targets"]] == labels
        for t, c in zip(doc["mesh"]["targets"], labels):
            stack = read_stack(dirs[name], pattern, c)
            verts, quads, st = mr.mesh_set(stack == 255, placement)
            assert (t["quads"], t["verts"]) == (st["quads"], st["verts"]), c
            file = dirs[name] / f"volume_mesh_class{c}.stl"
            if st["quads"] == 0:
                assert t["file"] is None and not file.exists() and t["area_mm2"] == 0 and t["volume_mm3"] == 0
                continue
            assert t["file"] == file.name
            want = binding.volume_mesh_derive(verts.astype(binding.MESH_VERTEX_DTYPE), quads, SPACING)
            assert t["area_mm2"] == want["area_mm2"] and t["volume_mm3"] == want["volume_mm3"], c
            normals, tri = parse_stl(file.read_bytes())
            xyz = binding.volume_mesh_positions(verts.astype(binding.MESH_VERTEX_DTYPE), SPACING)
            assert tri.shape[0] == 2 * st["quads"] and tri.tobytes() == xyz[mr.triangles(quads)].tobytes(), c
            p = xyz[mr.triangles(quads)].astype(np.float64)
            cross = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
            length = np.linalg.norm(cross, axis=1, keepdims=True)
            ref = np.where(length > 0, cross / np.where(length > 0, length, 1.0), 0.0)
            assert np.abs(normals - ref).max() <= 1e-6, c
        return doc

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log_never = run("never")
        # set and taken back: every artefact of a run that never touched the setting
        assert hostlib.set_volume_mesh(True, "nets") and hostlib.set_volume_mesh(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume mesh" not in log_never + log_off
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        assert "mesh" not in json.loads((dirs["off"] / "volume_report.json").read_bytes())
        # meshing only together with `volume on`
        assert hostlib.set_volume(False) and hostlib.set_volume_mesh(True, "nets")
        log = run("alone")
        assert "Volume" not in log and not [n for n in os.listdir(dirs["alone"]) if "volume" in n]
        # on, surface nets, the device route: class 2 is absent and writes no file
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("on")
        assert log.count("Volume mesh: 5 slices, 3 targets, nets, ") == 1
        stl = [f"volume_mesh_class{c}.stl" for c in (1, 3)]
        assert sorted(os.listdir(dirs["on"])) == sorted(names + stl)
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc = check_meshes("on", "nets", mr.NETS, "s{z}_mask_class{cls}.png")
        plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
        assert {k: v for k, v in doc.items() if k != "mesh"} == plain
        assert doc["mesh"]["targets"][0]["quads"] > 1000 and doc["mesh"]["targets"][2]["quads"] == 0
        # the host route: the same files and the same "mesh" object
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        for n in stl:
            assert (dirs["host"] / n).read_bytes() == (dirs["on"] / n).read_bytes(), n
        assert json.loads((dirs["host"] / "volume_report.json").read_bytes())["mesh"] == doc["mesh"]
        # voxel faces: the area is the components' surface, the volume their voxels
        assert hostlib.set_volume_mesh(True, "faces")
        run("faces")
        fdoc = check_meshes("faces", "faces", mr.FACES, "s{z}_mask_class{cls}.png")
        for t, rep in zip(fdoc["mesh"]["targets"], fdoc["targets"]):
            area, volume = sum(c["surface_mm2"] for c in rep["components"]), sum(c["volume_mm3"] for c in rep["components"])
            assert abs(t["area_mm2"] - area) <= 1e-9 * max(area, 1) and abs(t["volume_mm3"] - volume) <= 1e-9 * max(volume, 1)
        # under a filter the filtered stack is meshed: the second block of class 1 (240 pixels a slice) goes
        assert hostlib.set_volume(True, 26, 1500, 0, SPACING) and hostlib.set_volume_mesh(True, "nets")
        run("keep")
        kdoc = check_meshes("keep", "nets", mr.NETS, "s{z}_volume_mask_class{cls}.png")
        assert 0 < kdoc["mesh"]["targets"][0]["quads"] < doc["mesh"]["targets"][0]["quads"]
    finally:
        hostlib.set_volume_mesh(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
