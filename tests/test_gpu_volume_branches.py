"""The volume branch graph on the device (include/mi_unet.h: mi_unet_volume_branches): the engine's bytes equal the
reference of volume_branches_ref.py and the host form on every shared case -- both tables, the per-id table, map, out_ids, info; calls
repeat; outputs may be left out; one engine serves calls of any size between other stages; the stage chains behind the device's own
skeleton; argument errors queue nothing; the facade reports a "branches" member per component."""
import json
import os

import numpy as np
import pytest

import volume_branches_ref as vb
import volume_ref as vr
import volume_skeleton_ref as vk
from miunet import binding
from test_volume_branches_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


@pytest.fixture(scope="module")
def engine():
    with bare_engine() as eng:
        yield eng


def check(eng, name):
    """the device's tables, per-id table, map, out_ids and info equal the reference's and are the host form's bytes"""
    got = vb.call(eng.volume_branches, name)
    vb.check(got, name)
    vb.same_bytes(got, vb.call(binding.volume_branches_host, name), name)
    return got


def test_the_cases_are_not_degenerate():
    vb.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vb.cases()))
def test_device_equals_reference_and_host(engine, name):
    check(engine, name)


def test_two_calls_and_a_second_engine_give_the_same_bytes(engine):
    for name in ("noise_block", "seams", "serpentine", "noise_prune3", "spur_on_spur"):
        first, second = vb.call(engine.volume_branches, name), vb.call(engine.volume_branches, name)
        vb.same_bytes(first, second, name)
        with bare_engine(32, 32) as other:
            vb.same_bytes(first, vb.call(other.volume_branches, name), name)


def test_options_without_outputs(engine):
    """no map, no out_ids, no r2, caps of 0: what is still asked for is what the full call gives; without r2 the radius fields are zero"""
    ids, m, r2, _ = vb.cases()["noise"]
    full = engine.volume_branches(ids, m, r2, prune_voxels=3, want_map=True, want_ids=True)
    bare = engine.volume_branches(ids, m, r2, prune_voxels=3, want_map=False, want_ids=False, cap_nodes=0, cap_branches=0)
    assert bare["map"] is None and bare["ids"] is None and len(bare["nodes"]) == 0 and len(bare["branches"]) == 0
    assert bare["graph"].tobytes() == full["graph"].tobytes()
    assert all(bare[k] == full[k] for k in ("found_nodes", "found_branches", "rounds", "stable"))
    plain = engine.volume_branches(ids, m, None, prune_voxels=3, want_map=True, want_ids=True)
    vb.same_bytes(plain, binding.volume_branches_host(ids, m, None, prune_voxels=3, want_map=True, want_ids=True), "no r2")
    assert plain["map"].tobytes() == full["map"].tobytes() and plain["ids"].tobytes() == full["ids"].tobytes()
    assert full["branches"]["r2_max"].any() and full["nodes"]["r2_max"].any()
    for f in ("r2_min", "r2_max", "r2_sum"):
        assert not plain["branches"][f].any()
    assert not plain["nodes"]["r2_min"].any() and not plain["nodes"]["r2_max"].any()
    for f in ("first", "att_lo", "att_hi", "node_a", "node_b", "voxels", "links", "kind", "id"):
        assert np.array_equal(plain["branches"][f], full["branches"][f]), f


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state; the neighbouring stages'
    workspaces are their own"""
    order = ("single_voxel", "seams", "star_prune2", "noise_block", "serpentine", "two_voxels", "shell", "spur_on_spur", "line")
    noise = vr.smooth_noise((3, 64, 64))
    with bare_engine(32, 32) as eng:
        for i, name in enumerate(order):
            check(eng, name)
            if i == 2:
                vr.assert_equal(eng.volume_components(noise, vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))
            if i == 4:
                vk.same_bytes(vk.call(eng.volume_skeleton, "y"), vk.call(binding.volume_skeleton_host, "y"), "y")


def test_chained_behind_the_devices_own_skeleton(engine):
    vol = vr.smooth_noise((12, 40, 72))
    _, _, found, _, ids = engine.volume_components(vol, (1,), 26, cap=vr.MAX_TABLE, want_ids=True)
    m = int(found[0])
    sk = engine.volume_skeleton(ids[0], m, units=(2, 3, 5), want_r2=True)
    got = engine.volume_branches(sk["ids"], m, sk["r2"], units=(2, 3, 5), want_ids=True)
    assert m > 1 and sk["stable"] == 1 and got["found_branches"] > 0 and np.array_equal(got["ids"], sk["ids"])
    for mine, theirs in (("ends", "ends"), ("isolated", "isolated"), ("junction_voxels", "junctions")):
        assert np.array_equal(got["graph"][mine], sk["table"][theirs]), mine
    assert np.all(got["graph"]["links"] <= sk["table"]["links"])
    assert int(got["branches"]["voxels"].sum()) + int(got["nodes"]["voxels"].sum()) == int(sk["table"]["voxels"].sum())
    vb.same_bytes(got, binding.volume_branches_host(sk["ids"], m, sk["r2"], units=(2, 3, 5), want_ids=True), "chained")


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_branches, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_branches, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error().startswith(b"mi_unet_volume_branches:"), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_branches, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_branches, (None,), {})
        assert rc != 0 and untouched
        check(eng, "y")                                          # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
def expected_member(got, r, shape, spacing, unit_mm, radii=True):
    """the "branches" member of component r from a direct call's result"""
    g = got["graph"][r]
    d = binding.volume_branches_derive(g, got["branches"], got["found_nodes"], r + 1, spacing, unit_mm)
    listed = []
    for row in got["branches"][got["branches"]["id"] == r + 1][:64]:
        b = binding.volume_branches_derive_branch(row, shape, spacing, unit_mm)
        listed.append({"node_a": int(row["node_a"]), "node_b": int(row["node_b"]), "kind": int(row["kind"]), "voxels": int(row["voxels"]),
                       "length_mm": b["length_mm"], "chord_mm": b["chord_mm"], "tortuosity": b["tortuosity"],
                       "radius_min_mm": b["radius_min_mm"] if radii else None, "radius_max_mm": b["radius_max_mm"] if radii else None,
                       "radius_rms_mm": b["radius_rms_mm"] if radii else None})
    return {"nodes": int(g["nodes"]), "ends": int(g["ends"]), "junctions": int(g["junction_nodes"]), "branches": int(g["branches"]),
            "closed": int(g["closed"]), "parts": d["parts"], "loops": d["loops"], "length_mm": d["length_mm"], "pruned_spurs": int(g["pruned_spurs"]),
            "list": listed, "listed": len(listed), "found": int(g["branches"])}


def test_facade_reports_a_branches_member_per_component(tmp_path, monkeypatch):
    from miunet import hostlib
    from test_gpu_targets import blob, raw_of
    from test_gpu_volume import read_stack
    from test_gpu_volume_skeleton import FACADE_TARGETS, SPACING, ring_and_bar
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
    dirs = {n: tmp_path / n for n in ("never", "on", "host", "plain", "alone", "off")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def same_files(a, b, but=()):
        assert sorted(os.listdir(dirs[a])) == sorted(os.listdir(dirs[b]))
        for n in os.listdir(dirs[a]):
            if n not in but:
                assert (dirs[a] / n).read_bytes() == (dirs[b] / n).read_bytes(), n

    def report(name):
        return json.loads((dirs[name] / "volume_report.json").read_bytes())

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        assert hostlib.set_volume_skeleton(True, True, False, 0)
        log_never = run("never")
        assert "Volume branches" not in log_never and b"\"branches\"" not in (dirs["never"] / "volume_report.json").read_bytes()
        # on, the device route: the same files, every component with its member behind the skeleton's, nothing else in the report moved
        assert hostlib.set_volume_branches(True, 3, 0)
        log = run("on")
        same_files("on", "never", but=("volume_report.json",))
        doc, base = report("on"), report("never")
        units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
        totals = [0, 0, 0]
        with bare_engine() as eng:
            for t, t0, (cls, _) in zip(doc["targets"], base["targets"], FACADE_TARGETS):
                stack = read_stack(dirs["on"], "s{z}_mask_class{cls}.png", cls)
                _, _, found, _, ids = eng.volume_components(stack, (255,), 26, cap=vr.MAX_TABLE, want_ids=True)
                m = int(found[0])
                sk = eng.volume_skeleton(ids[0], m, units=units, want_r2=True)
                got = eng.volume_branches(sk["ids"], m, sk["r2"], units=units, prune_voxels=3)
                totals = [totals[0] + got["found_nodes"], totals[1] + got["found_branches"], totals[2] + got["rounds"]]
                assert m == len(t["components"]) >= 1
                for r, (comp, comp0) in enumerate(zip(t["components"], t0["components"])):
                    assert list(comp)[-2:] == ["skeleton", "branches"]
                    assert comp["branches"] == expected_member(got, r, (5, 64, 64), SPACING, unit_mm)
                    assert {k: v for k, v in comp.items() if k != "branches"} == comp0
        assert log.count(f"Volume branches: 5 slices, 2 targets, {totals[0]} nodes, {totals[1]} branches, {totals[2]} rounds, ") == 1
        tube = doc["targets"][0]["components"][0]["branches"]
        assert tube["loops"] >= 1 and tube["ends"] == 0 and tube["parts"] == 1
        bar = doc["targets"][1]["components"][0]["branches"]
        assert (bar["ends"], bar["loops"], bar["parts"]) == (2, 0, 1) and bar["length_mm"] > 20 * 0.7
        assert all(0 < b["radius_min_mm"] <= b["radius_rms_mm"] <= b["radius_max_mm"] for b in bar["list"] if b["voxels"])
        # the host route: the same report, byte for byte
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert (dirs["host"] / "volume_report.json").read_bytes() == (dirs["on"] / "volume_report.json").read_bytes()
        # the skeleton's radius off: the branches get no r2 and report no radii
        assert hostlib.set_volume_skeleton(True, False, False, 0)
        run("plain")
        first = report("plain")["targets"][1]["components"][0]["branches"]
        assert first["list"] and all(b["radius_min_mm"] is None and b["radius_rms_mm"] is None and b["radius_max_mm"] is None for b in first["list"])
        assert {k: v for k, v in first.items() if k != "list"} == {k: v for k, v in bar.items() if k != "list"}
        # without the skeleton the setting does nothing
        assert hostlib.set_volume_skeleton(False)
        log_alone = run("alone")
        assert "Volume branches" not in log_alone and b"\"branches\"" not in (dirs["alone"] / "volume_report.json").read_bytes()
        # off again: every artefact of a run that never touched the setting
        assert hostlib.set_volume_skeleton(True, True, False, 0) and hostlib.set_volume_branches(False)
        log_off = run("off")
        assert "Volume branches" not in log_off
        same_files("off", "never")
    finally:
        hostlib.set_volume_branches(False)
        hostlib.set_volume_skeleton(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
