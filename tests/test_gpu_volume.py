"""Volume components on the device (include/mi_unet.h: mi_unet_volume_components) against the flood-fill reference of
volume_ref.py: out, ids, table, found and kept of every plane, exactly, and the bytes of the host form.  The inputs and cases are
volume_ref's, the ones test_volume_cpu.py holds the host form to.  The inputs are checked for non-degeneracy on the reference alone
before the device is asked."""
import numpy as np
import pytest

import volume_ref as vr
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_volume_cpu import call_with, earg_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def same_bytes(a, b):
    return all((x is None and y is None) or (x.tobytes() == y.tobytes() and x.shape == y.shape) for x, y in zip(a, b))


def check(eng, masks, values, what, want=None, **kw):
    """the device's five outputs equal the reference's exactly and are the host form's bytes"""
    got = eng.volume_components(masks, values, want_ids=True, **kw)
    vr.assert_equal(got, want if want is not None else vr.components(masks, values, **kw), what)
    assert same_bytes(got, binding.volume_components_host(masks, values, want_ids=True, **kw)), what
    return got


def test_the_noise_volumes_are_not_degenerate():
    vr.assert_not_degenerate()


@pytest.mark.parametrize("shape", vr.NOISE_SHAPES)
def test_noise_volumes_equal_the_reference_under_every_connectivity(shape):
    with bare_engine() as eng:
        for c in vr.CONNECTIVITIES:
            check(eng, vr.smooth_noise(shape), vr.NOISE_VALUES, f"{shape} {c}", vr.noise_ref(shape, c), connectivity=c)


@pytest.mark.parametrize("name", sorted(vr.edge_cases()))
def test_edge_cases_equal_the_reference(name):
    masks, values, claims = vr.edge_cases()[name]
    with bare_engine() as eng:
        for c in vr.CONNECTIVITIES:
            got = check(eng, masks, values, f"{name} {c}", connectivity=c, cap=8)
            assert got[2][0] == claims[c]


@pytest.mark.parametrize("name", sorted(vr.call_cases()))
def test_filter_table_and_ids_equal_the_reference(name):
    masks, values, kw = vr.call_cases()[name]
    with bare_engine() as eng:
        check(eng, masks, values, name, vr.call_ref(name), **kw)


def test_out_may_alias_masks():
    import ctypes as C
    vol = np.array(vr.smooth_noise((3, 64, 64)))
    want = vr.components(vol, (2,), 18, min_voxels=6, cap=4)
    table, found, kept = np.zeros((1, 4), binding.VCOMP_DTYPE), np.zeros(1, np.int32), np.zeros(1, np.int32)
    vals = np.array([2], np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    with bare_engine() as eng:
        rc = binding.lib().mi_unet_volume_components(eng._h, ptr(vol), 3, 64, 64, ptr(vals), 1, C.byref(binding.VolumeOpts(18, 6, 0)),
                                                     ptr(vol), None, ptr(table), 4, ptr(found), ptr(kept))
    assert rc == 0
    vr.assert_equal((vol[None], table, found, kept, None), want)


def test_repeated_smaller_and_larger_calls_return_the_bytes_of_fresh_engines():
    """two calls in a row give the same bytes; a call after a larger one still gives the right bytes: the workspace keeps no state"""
    n16, n3 = vr.smooth_noise((16, 24, 130)), vr.smooth_noise((3, 64, 64))
    snake = vr.edge_cases()["serpentine"][0]
    calls = [(n3, (1, 2), dict(connectivity=6, keep_largest=5, cap=3)), (n3, (1, 2), dict(connectivity=6, keep_largest=5, cap=3)),
             (n16, vr.NOISE_VALUES, dict(connectivity=6, cap=vr.MAX_TABLE)), (n3, (3,), dict(connectivity=26, min_voxels=3, cap=300)),
             (snake, (1,), dict(connectivity=18)), (n3, (1, 2), dict(connectivity=6, keep_largest=5, cap=3))]
    fresh = []
    for m, v, kw in calls:
        with bare_engine(32, 32) as eng:
            fresh.append(eng.volume_components(m, v, want_ids=True, **kw))
    assert same_bytes(fresh[0], fresh[1])
    vr.assert_equal(fresh[3], vr.components(n3, (3,), connectivity=26, min_voxels=3, cap=300))
    with bare_engine(32, 32) as eng:                            # one engine: the workspace grows, then serves smaller calls
        for i, ((m, v, kw), want) in enumerate(zip(calls, fresh)):
            assert same_bytes(eng.volume_components(m, v, want_ids=True, **kw), want), i


def test_an_engine_with_weights_of_another_tile_size():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=4)
    shape = (7, 40, 72)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 3)))
        labels_before, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        check(eng, vr.smooth_noise(shape), vr.NOISE_VALUES, "with weights", vr.noise_ref(shape, 18), connectivity=18)
        labels_after, _ = eng.infer(synth.make_images(2, 64, 64, 1, 5, "blobs"), want_logits=True)
        assert np.array_equal(labels_before, labels_after)


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_components, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_components, (eng._h,), case)
            assert rc == 1 and untouched and L.mi_unet_last_error(), name
        rc, untouched = call_with(L.mi_unet_volume_components, (None,), {})
        assert rc != 0 and untouched
        shape = (3, 64, 64)                                     # the engine still works
        check(eng, vr.smooth_noise(shape), vr.NOISE_VALUES, "after the refusals", vr.noise_ref(shape, 26), connectivity=26)


# ---- the facade: five RAW slices through process_image_batch ---------------------------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0)]
SPACING = (0.7, 0.7, 3.0)


def slice_labels(z):
    """five 64 x 64 label maps that stack into: class 1 -- a block over slices 0 .. 2 (drifting in x), one in slice 2 and one in slice 4
    alone; class 3 -- a block over slices 1 .. 3 and one in slice 0 alone.  Every block survives the 3 x 3 open"""
    m = np.zeros((64, 64), np.uint8)
    if z <= 2:
        m[10:20, 10 + z:22 + z] = 1
    if z == 2:
        m[40:45, 20:26] = 1
    if z == 4:
        m[40:46, 40:50] = 1
    if 1 <= z <= 3:
        m[30:38, 5:15] = 3
    if z == 0:
        m[50:55, 50:56] = 3
    m[0, 0], m[63, 63] = 0, 3                              # both ends of the grey range (test_gpu_targets.raw_of)
    return m


def read_stack(out_dir, pattern, cls):
    from miunet import hostlib
    return np.stack([hostlib.read_png(str(out_dir / pattern.format(z=z, cls=cls))) for z in range(5)])


def test_facade_labels_a_batch_as_one_volume(tmp_path, monkeypatch):
    import json
    import os

    from miunet import hostlib
    from test_gpu_targets import blob, raw_of
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    paths, ws, hs = [], [], []
    for z in range(5):
        r = raw_of(slice_labels(z), 1 + z % 2)
        paths.append(str(tmp_path / f"s{z}.raw"))
        r.tofile(paths[-1])
        ws.append(r.shape[1]); hs.append(r.shape[0])
    dirs = {n: tmp_path / n for n in ("never", "off", "on", "host", "keep")}
    for d in dirs.values():
        os.makedirs(d)
    run = lambda name: hostlib.process_image_batch(paths, ws, hs, str(dirs[name]))
    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert run("never") == 5
        assert hostlib.set_volume(True, 26, 0, 0, SPACING) and hostlib.set_volume(False)
        assert run("off") == 5
        # off: no volume artefact, and the artefacts of a run that never touched the setting
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and len(names) == 5 * 6 and not [n for n in names if "volume" in n]
        # on without a filter: the report, and every other artefact byte for byte
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        assert run("on") == 5
        assert sorted(os.listdir(dirs["on"])) == sorted(names + ["volume_report.json"])
        for n in names:
            assert (dirs["on"] / n).read_bytes() == (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc = json.loads((dirs["on"] / "volume_report.json").read_bytes())
        assert doc["slices"] == [f"s{z}" for z in range(5)] and doc["missing"] == []
        assert (doc["connectivity"], doc["min_voxels"], doc["keep_largest"], doc["spacing"]) == (26, 0, 0, list(SPACING))
        assert [t["label"] for t in doc["targets"]] == [1, 3]
        spanning = 0
        for t, (cls, _) in zip(doc["targets"], FACADE_TARGETS):
            stack = read_stack(dirs["on"], "s{z}_mask_class{cls}.png", cls)      # the pictures this very call wrote
            assert set(np.unique(stack)) == {0, 255}
            ref = vr.plane(stack, 255, 26, cap=vr.MAX_TABLE)
            assert (t["found"], t["kept"]) == (ref["found"], ref["kept"]) and len(t["components"]) == ref["found"]
            for got, c in zip(t["components"], ref["comps"]):
                assert (got["voxels"], got["kept"]) == (c["voxels"], c["kept"])
                assert got["bbox"] == [c[f] for f in ("x0", "y0", "z0", "x1", "y1", "z1")]
                m = binding.volume_derive(binding.VComp(*[c[f] for f in vr.FIELDS]), SPACING)
                assert got["centroid_mm"] == [m["cx_mm"], m["cy_mm"], m["cz_mm"]]
                assert (got["volume_mm3"], got["surface_mm2"]) == (m["volume_mm3"], m["surface_mm2"])
                assert got["extent_mm"] == [m["extent_x_mm"], m["extent_y_mm"], m["extent_z_mm"]]
                spanning += c["z1"] > c["z0"]
        # the stack is not degenerate: several components for a target, and components over several slices
        assert [t["found"] for t in doc["targets"]] == [3, 2] and spanning == 2
        assert doc["targets"][0]["components"][0]["voxels"] == 3 * 10 * 12 and doc["targets"][0]["components"][0]["bbox"] == [10, 10, 0, 23, 19, 2]
        # the host form under MEDSEG_HOST_POSTPROCESS=1: the same report
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        assert run("host") == 5
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        assert (dirs["host"] / "volume_report.json").read_bytes() == (dirs["on"] / "volume_report.json").read_bytes()
        # keep 1: the filtered stack as pictures, beside the unchanged artefacts
        assert hostlib.set_volume(True, 26, 0, 1, SPACING)
        assert run("keep") == 5
        extra = [f"s{z}_volume_mask_class{c}.png" for z in range(5) for c, _ in FACADE_TARGETS]
        assert sorted(os.listdir(dirs["keep"])) == sorted(names + ["volume_report.json"] + extra)
        for n in names:
            assert (dirs["keep"] / n).read_bytes() == (dirs["off"] / n).read_bytes(), n
        kept_doc = json.loads((dirs["keep"] / "volume_report.json").read_bytes())
        for t, (cls, _) in zip(kept_doc["targets"], FACADE_TARGETS):
            stack = read_stack(dirs["keep"], "s{z}_mask_class{cls}.png", cls)
            ref = vr.plane(stack, 255, 26, keep_largest=1)
            assert np.array_equal(read_stack(dirs["keep"], "s{z}_volume_mask_class{cls}.png", cls), ref["out"])
            assert t["kept"] == 1 and [c["kept"] for c in t["components"]] == [1] + [0] * (t["found"] - 1)
            assert 0 < int((ref["out"] == 255).sum()) < int((stack == 255).sum())
    finally:
        hostlib.set_volume(False)
        hostlib.set_targets([])
        hostlib.cleanup_resources()
