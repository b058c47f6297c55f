"""The volume skeleton on the device (include/mi_unet.h: mi_unet_volume_skeleton): the engine's bytes equal the reference
of volume_skeleton_ref.py and the host form on every shared case, `passes` included; calls repeat; the kernels' simple-point test equals
the host form's on all 2^26 codes; the topology of the device's skeleton is the input's; one engine serves calls of any size between
other stages; the skeleton chains into the stages that take an id stack; argument errors queue nothing."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import volume_ref as vr
import volume_skeleton_ref as vk
from miunet import binding
from test_volume_skeleton_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


@pytest.fixture(scope="module")
def engine():
    with bare_engine() as eng:
        yield eng


def check(eng, name):
    """the device's table, info, out_ids and r2 equal the reference's and are the host form's bytes"""
    got = vk.call(eng.volume_skeleton, name)
    vk.assert_equal(got, vk.case_ref(name), name)
    vk.same_bytes(got, vk.call(binding.volume_skeleton_host, name), name)
    return got


def test_the_cases_are_not_degenerate():
    vk.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vk.cases()))
def test_device_equals_reference_and_host(engine, name):
    got = check(engine, name)
    assert got["passes"] == vk.case_ref(name)["passes"]             # part of the definition


def test_two_calls_and_a_second_engine_give_the_same_bytes(engine):
    for name in ("noise_labelled_6", "seams", "aniso_noise"):
        first, second = vk.call(engine.volume_skeleton, name), vk.call(engine.volume_skeleton, name)
        vk.same_bytes(first, second, name)
        with bare_engine(32, 32) as other:
            vk.same_bytes(first, vk.call(other.volume_skeleton, name), name)


def test_the_kernels_simple_point_test_equals_the_host_form_on_every_code(engine):
    """one launch over all 2^26 codes, the host form's table (in eight parts, side by side), one comparison; the host form is compared
    with the definition in test_volume_skeleton_cpu.py"""
    device = engine.volume_skeleton_simple()
    assert device.shape == (binding.SKELETON_CODE_WORDS,)
    part = binding.SKELETON_CODE_WORDS // 8
    with ThreadPoolExecutor(8) as pool:
        host = np.concatenate(list(pool.map(lambda k: binding.volume_skeleton_simple_host(k * part, part), range(8))))
    diff = np.flatnonzero(device != host)
    assert diff.size == 0, [(int(w), hex(int(device[w])), hex(int(host[w]))) for w in diff[:5]]
    assert np.array_equal(engine.volume_skeleton_simple(12345, 7), host[12345:12352])       # a range that starts inside


@pytest.mark.parametrize("name", ["shell", "torus", "noise", "seams", "noise_labelled_6", "tubes_in_contact", "full_block"])
def test_topology_of_the_devices_skeleton_is_the_inputs(engine, name):
    ids, m, _ = vk.cases()[name]
    got = vk.call(engine.volume_skeleton, name)
    clean = np.where((ids >= 1) & (ids <= m), ids, 0)
    assert np.all((got["ids"] == 0) | (got["ids"] == clean))
    assert vk.topology_by_id(got["ids"], m) == vk.topology_by_id(clean, m)


def test_options_without_outputs(engine):
    """no out_ids, no r2, no radius: the table's counts are those of the full call; r2 alone with radius off is still the radius"""
    ids, m, _ = vk.cases()["noise"]
    full = engine.volume_skeleton(ids, m, want_r2=True)
    bare = engine.volume_skeleton(ids, m, radius=False, want_ids=False)
    only_r2 = engine.volume_skeleton(ids, m, radius=False, want_ids=False, want_r2=True)
    assert bare["ids"] is None and bare["r2"] is None and only_r2["r2"].tobytes() == full["r2"].tobytes()
    for got in (bare, only_r2):
        assert got["table"].tobytes() == binding.volume_skeleton_host(ids, m, radius=False)["table"].tobytes()
        assert got["passes"] == full["passes"] and got["deleted"] == full["deleted"]


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state; the neighbouring stages'
    workspaces are their own"""
    order = ("single_voxel", "seams", "one_slice", "aniso_noise", "ball_r9", "two_voxels", "shell", "line")
    noise = vr.smooth_noise((3, 64, 64))
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name)
            if i == 2:
                vr.assert_equal(eng.volume_components(noise, vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))
            if i == 4:
                out, _ = eng.volume_clean(noise, (1,), (1, 1, 1), fill=1, close_r=1, open_r=2)
                ref, _ = binding.volume_clean_host(noise, (1,), (1, 1, 1), fill=1, close_r=1, open_r=2)
                assert out.tobytes() == ref.tobytes()
                assert np.array_equal(eng.volume_skeleton_simple(0, 64), binding.volume_skeleton_simple_host(0, 64))


def test_chained_behind_the_components_stage_measure_reports_the_skeletons_voxels(engine):
    vol = vr.smooth_noise((12, 40, 72))
    _, table, found, _, ids = engine.volume_components(vol, (1,), 26, cap=vr.MAX_TABLE, want_ids=True)
    m = int(found[0])
    got = engine.volume_skeleton(ids[0], m, units=(2, 3, 5))
    assert m > 1 and np.array_equal(got["table"]["voxels_in"], table[0]["voxels"][:m]) and got["stable"] == 1
    measured = engine.volume_measure(got["ids"], None, m=m, units=(2, 3, 5))
    assert np.array_equal(measured["voxels"], got["table"]["voxels"]) and 0 < int(got["table"]["voxels"].sum()) < int(table[0]["voxels"][:m].sum())
    vk.same_bytes(got, binding.volume_skeleton_host(ids[0], m, units=(2, 3, 5)), "chained")


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_skeleton, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_skeleton, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error().startswith(b"mi_unet_volume_skeleton:"), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_skeleton, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_skeleton, (None,), {})
        assert rc != 0 and untouched
        bits = np.full(4, 0x55555555, np.uint32)
        assert L.mi_unet_volume_skeleton_simple(eng._h, 1 << 21, 1, bits.ctypes.data) == 1 and (bits == 0x55555555).all()
        assert L.mi_unet_last_error().startswith(b"mi_unet_volume_skeleton_simple:")
        check(eng, "y")                                          # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0)]
SPACING = (0.7, 0.7, 3.0)


def ring_and_bar(z):
    """a 64 x 64 label map: class 1 -- an annulus of radii 9 .. 15 (stacked: a thick-walled tube, one tunnel); class 3 -- a bar of
    5 x 40 pixels and, apart from it, a block of 2 x 2"""
    y, x = np.mgrid[0:64, 0:64]
    m = np.zeros((64, 64), np.uint8)
    q = (x - 24) ** 2 + (y - 24) ** 2
    m[(q >= 81) & (q <= 225)] = 1
    m[52:57, 10:50] = 3
    m[44:46, 58:60] = 3
    m[0, 0], m[63, 63] = 0, 3                              # both ends of the grey range (test_gpu_targets.raw_of)
    return m


def test_facade_reports_a_skeleton_member_per_component(tmp_path, monkeypatch):
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
        r = raw_of(ring_and_bar(z), 1 + z % 2)
        paths.append(str(tmp_path / f"s{z}.raw"))
        r.tofile(paths[-1])
        ws.append(r.shape[1]); hs.append(r.shape[0])
    dirs = {n: tmp_path / n for n in ("never", "on", "host", "bare", "off")}
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
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log_never = run("never")
        assert "Volume skeleton" not in log_never and b"skeleton" not in (dirs["never"] / "volume_report.json").read_bytes()
        names = sorted(os.listdir(dirs["never"]))
        # on with pictures, the device route: the same files and per slice and target a skeleton picture; every component with its member
        assert hostlib.set_volume_skeleton(True, True, True, 0)
        log = run("on")
        pictures = sorted(f"s{z}_volume_skeleton_class{cls}.png" for z in range(5) for cls, _ in FACADE_TARGETS)
        assert sorted(os.listdir(dirs["on"])) == sorted(names + pictures)
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc = json.loads((dirs["on"] / "volume_report.json").read_bytes())
        units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
        passes = 0
        with bare_engine() as eng:
            for t, (cls, _) in zip(doc["targets"], FACADE_TARGETS):
                stack = read_stack(dirs["on"], "s{z}_mask_class{cls}.png", cls)
                _, _, found, _, ids = eng.volume_components(stack, (255,), 26, cap=vr.MAX_TABLE, want_ids=True)
                m = int(found[0])
                got = eng.volume_skeleton(ids[0], m, units=units)
                passes += got["passes"]
                assert m == len(t["components"]) >= 1
                for comp, row in zip(t["components"], got["table"]):
                    want = binding.volume_skeleton_derive(row, SPACING, unit_mm)
                    assert list(comp)[-1] == "skeleton"
                    assert comp["skeleton"] == {"voxels": int(row["voxels"]), "ends": int(row["ends"]), "junctions": int(row["junctions"]),
                                                "isolated": int(row["isolated"]), "loops": want["loops"], "length_mm": want["length_mm"],
                                                "radius_min_mm": want["radius_min_mm"], "radius_max_mm": want["radius_max_mm"],
                                                "radius_rms_mm": want["radius_rms_mm"], "stable": 1}
                drawn = read_stack(dirs["on"], "s{z}_volume_skeleton_class{cls}.png", cls)
                assert np.array_equal(drawn > 0, got["ids"] > 0)
        assert log.count(f"Volume skeleton: 5 slices, 2 targets, {passes} passes, ") == 1
        tube = doc["targets"][0]["components"][0]["skeleton"]
        assert tube["loops"] >= 1 and tube["ends"] == 0 and 0 < tube["radius_min_mm"] <= tube["radius_rms_mm"] <= tube["radius_max_mm"]
        bar = doc["targets"][1]["components"][0]["skeleton"]
        assert bar["ends"] == 2 and bar["loops"] == 0 and bar["length_mm"] > 20 * 0.7
        # the host route: the same report and pictures, byte for byte
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        for n in ["volume_report.json"] + pictures:
            assert (dirs["host"] / n).read_bytes() == (dirs["on"] / n).read_bytes(), n
        # radius off, no pictures, one pass: nulls, no picture, not stable
        assert hostlib.set_volume_skeleton(True, False, False, 1)
        run("bare")
        assert sorted(os.listdir(dirs["bare"])) == names
        bare = json.loads((dirs["bare"] / "volume_report.json").read_bytes())["targets"][0]["components"][0]["skeleton"]
        assert bare["radius_min_mm"] is None and bare["radius_max_mm"] is None and bare["radius_rms_mm"] is None and bare["stable"] == 0
        assert bare["voxels"] > tube["voxels"]
        # off again: every artefact of a run that never touched the setting
        assert hostlib.set_volume_skeleton(False)
        log_off = run("off")
        assert "Volume skeleton" not in log_off and sorted(os.listdir(dirs["off"])) == names
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
    finally:
        hostlib.set_volume_skeleton(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
