"""The volume split on the device (include/mi_unet.h: mi_unet_volume_split): the engine's bytes equal the reference
of volume_split_ref.py and the host form on every shared case (`rounds` is diagnostic and no part of the comparison); calls repeat;
the rounds of the growth follow the tiles a path crosses, not its voxels; one engine serves calls of any size between other stages;
the pieces chain into the stages that take a components table or an id stack; argument errors queue nothing."""
import numpy as np
import pytest

import volume_ref as vr
import volume_split_ref as vs
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_split_cpu import call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


@pytest.fixture(scope="module")
def engine():
    with bare_engine() as eng:
        yield eng


def check(eng, name):
    """the device's table, info, ids, found and stats equal the reference's and are the host form's bytes"""
    got = vs.call(eng.volume_split, name)
    vs.assert_equal(got, vs.case_ref(name), name)
    vs.same_bytes(got, vs.call(binding.volume_split_host, name), name)
    return got


def test_the_cases_are_not_degenerate():
    vs.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vs.cases()))
def test_device_equals_reference_and_host(engine, name):
    check(engine, name)


def test_two_calls_and_a_second_engine_give_the_same_bytes(engine):
    for name in ("chain_26", "noise_18_neck2_core1_u235", "serpentine_130"):
        first, second = vs.call(engine.volume_split, name), vs.call(engine.volume_split, name)
        vs.same_bytes(first, second, name)
        with bare_engine(32, 32) as other:
            vs.same_bytes(first, vs.call(other.volume_split, name), name)


def test_rounds_follow_the_tiles_of_a_path_not_its_voxels(engine, record_property):
    """serpentine W = 130: each piece's path is 852 voxel steps long (2556 / 3) and winds through three tiles along x, seventeen
    rows and five tiles along y; a round takes a path through a whole tile, so the rounds stay near the tiles crossed -- 17 rows x 3
    tiles is 51, and the two cores grow at once -- and far below the steps: at most 200 whatever the scheduling."""
    got = check(engine, "serpentine_130")
    rounds = int(got["rounds"][0])
    record_property("rounds", rounds)
    print("serpentine_130 rounds:", rounds)
    assert 2 <= rounds <= 200
    assert int(got["stats"][0]["max_reach"]) == 2556
    assert int(check(engine, "value_absent")["rounds"][1]) == 0                # a plane without a voxel grows nothing


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state; the neighbouring stages'
    workspaces are their own"""
    order = ("row_only", "chain_26", "one_slice", "noise_6_neck2_core1_u235", "two_balls_neck5", "row_only", "aniso_neck100", "side_of_1")
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


def test_chained_behind_the_components_stage_the_pieces_add_up_to_the_components(engine):
    """the components stage's `out` split on the device: every piece lies in one component, and the pieces of a component have its voxels"""
    vol = vr.smooth_noise(vs.NOISE_SHAPE)
    out, table, found, _, ids = engine.volume_components(vol, (3,), 18, min_voxels=4, cap=vr.MAX_TABLE, want_ids=True)
    got = engine.volume_split(out[0], (3,), (2, 3, 5), 18, neck_r=2, cap=vr.MAX_TABLE, want_ids=True)
    assert int(got["found"][0]) > int((table[0]["kept"] == 1).sum()) > 0
    comp, piece = ids[0].reshape(-1), got["ids"][0].reshape(-1)
    assert np.array_equal(comp > 0, piece > 0)
    inside = comp > 0
    pairs = np.unique(np.stack([piece[inside], comp[inside]]), axis=1)
    assert len(np.unique(pairs[0])) == pairs.shape[1] == int(got["found"][0])  # a piece lies in one component
    sums = np.zeros(int(found[0]) + 1, np.int64)
    np.add.at(sums, pairs[1], got["table"][0]["voxels"][pairs[0] - 1])
    kept = table[0]["kept"][:int(found[0])] == 1
    assert np.array_equal(sums[1:][kept], table[0]["voxels"][:int(found[0])][kept])


def test_volume_measure_on_the_split_ids_reports_the_pieces(engine):
    got = vs.call(engine.volume_split, "chain_26")
    m = int(got["found"][0])
    measured = engine.volume_measure(got["ids"][0], None, m=m, units=(1, 1, 1))
    assert m == 3 and list(measured["voxels"]) == [6942, 5012, 1430] == list(got["table"][0]["voxels"][:m])


def test_an_engine_with_weights_infers_the_same_labels_before_and_after():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, "two_balls_neck3")
        check(eng, "noise_26_neck2_core5_u235")
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_split, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_split, (eng._h,), case)
            assert rc == 1 and untouched and b"mi_unet_volume_split:" in L.mi_unet_last_error(), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_split, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_split, (None,), {})
        assert rc != 0 and untouched
        check(eng, "two_balls_neck3")                            # the engine still works


# ---- the facade: five RAW slices through process_image_batch ------------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0)]
SPACING = (0.7, 0.7, 3.0)
NECK_MM = 3.5


def touching_discs(z):
    """a 64 x 64 label map: class 1 -- two discs of radius 10 whose centres lie 18 apart, so they overlap in a lens 8 pixels wide;
    stacked, two cylinders joined along that lens.  A ball of 3.5 mm reaches 5 pixels in the slice: the cores are two cylinders of
    radius 5, and the lens is no core.  Class 3 is a block of 3 x 3 pixels (and the corner pixel): columns too thin to hold a core."""
    y, x = np.mgrid[0:64, 0:64]
    m = np.zeros((64, 64), np.uint8)
    m[((x - 20) ** 2 + (y - 32) ** 2 <= 100) | ((x - 38) ** 2 + (y - 32) ** 2 <= 100)] = 1
    m[50:53, 50:53] = 3
    m[0, 0], m[63, 63] = 0, 3                              # both ends of the grey range (test_gpu_targets.raw_of)
    return m


def test_facade_reports_the_pieces_with_a_split_member_each(tmp_path, monkeypatch):
    import json
    import math
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
        r = raw_of(touching_discs(z), 1 + z % 2)
        paths.append(str(tmp_path / f"s{z}.raw"))
        r.tofile(paths[-1])
        ws.append(r.shape[1]); hs.append(r.shape[0])
    dirs = {n: tmp_path / n for n in ("never", "on", "host", "measured", "off")}
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
        plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
        assert len(plain["targets"][0]["components"]) == 1 and len(plain["targets"][1]["components"]) >= 1 and "Volume split" not in log_never
        assert b"split" not in (dirs["never"] / "volume_report.json").read_bytes()
        # on, the device route: the same files; the report shows the pieces, every component and every target with its member
        assert hostlib.set_volume_split(True, NECK_MM, 1)
        log = run("on")
        units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
        neck_r = int(math.floor(NECK_MM / unit_mm + 0.5))
        assert neck_r // units[0] == 5 and neck_r // units[2] == 1         # five pixels in the slice, one slice
        assert log.count(f"Volume split: 5 slices, 2 targets, neck {neck_r} units") == 1
        names = sorted(os.listdir(dirs["never"]))
        assert sorted(os.listdir(dirs["on"])) == names
        for n in names:
            if n != "volume_report.json":
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc = json.loads((dirs["on"] / "volume_report.json").read_bytes())
        with bare_engine() as eng:
            for t, (cls, _) in zip(doc["targets"], FACADE_TARGETS):
                stack = read_stack(dirs["on"], "s{z}_mask_class{cls}.png", cls)
                got = eng.volume_split(stack, (255,), units, 26, neck_r=neck_r, min_core=1, cap=vr.MAX_TABLE)
                st, m = got["stats"][0], int(got["found"][0])
                assert list(t)[-1] == "split" and t["found"] == t["kept"] == m == len(t["components"])
                assert t["split"] == {"neck_mm": NECK_MM, "cores": int(st["cores"]), "cores_kept": int(st["cores_kept"]), "pieces": m,
                                      "coreless": int(st["coreless"])}
                for comp, row, piece in zip(t["components"], got["table"][0], got["info"][0]):
                    want = binding.volume_split_derive(piece, SPACING, unit_mm)
                    assert list(comp)[-1] == "split" and comp["voxels"] == row["voxels"] and comp["kept"] == 1
                    assert comp["split"] == {"core_voxels": int(piece["core_voxels"]), "reach_mm": want["reach_mm"], "cut_mm2": want["cut_mm2"]}
        discs, column = doc["targets"]
        assert discs["split"]["pieces"] == 2 and discs["split"]["cores"] == 2 and discs["split"]["coreless"] == 0
        assert sum(c["voxels"] for c in discs["components"]) == plain["targets"][0]["components"][0]["voxels"]
        assert all(c["split"]["cut_mm2"] > 0 and c["split"]["core_voxels"] > 0 for c in discs["components"])
        thin = len(plain["targets"][1]["components"])             # without a core the pieces are the components
        assert column["split"] == {"neck_mm": NECK_MM, "cores": 0, "cores_kept": 0, "pieces": thin, "coreless": thin}
        assert all(c["split"] == {"core_voxels": 0, "reach_mm": 0.0, "cut_mm2": 0.0} for c in column["components"])
        # the host route: the same report, byte for byte
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert (dirs["host"] / "volume_report.json").read_bytes() == (dirs["on"] / "volume_report.json").read_bytes()
        # a stage behind it takes the pieces: two measured components where the plain report has one
        assert hostlib.set_volume_measure(True)
        run("measured")
        measured = json.loads((dirs["measured"] / "volume_report.json").read_bytes())
        comps = measured["targets"][0]["components"]
        assert len(comps) == 2 and all(list(c)[-2:] == ["measure", "split"] and c["measure"] is not None for c in comps)
        assert hostlib.set_volume_measure(False)
        # off again: every artefact of a run that never touched the setting
        assert hostlib.set_volume_split(False)
        log_off = run("off")
        assert "Volume split" not in log_off and sorted(os.listdir(dirs["off"])) == names
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
    finally:
        hostlib.set_volume_measure(False)
        hostlib.set_volume_split(False)
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
