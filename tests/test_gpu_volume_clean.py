"""Volume clean-up on the device (include/mi_unet.h: mi_unet_volume_clean) against the brute-force reference of
volume_clean_ref.py: the bytes of every plane and every count, exactly, and the bytes of the host form.  The inputs and cases are
volume_clean_ref's, the ones test_volume_clean_cpu.py holds the host form to.  The inputs are checked for non-degeneracy on the
reference alone before the device is asked."""
import ctypes as C

import numpy as np
import pytest

import volume_clean_ref as cr
from miunet import binding
from test_volume_clean_cpu import PROP_SHAPE, PROP_UNITS, call_with, earg_cases, legal_cases

pytestmark = pytest.mark.gpu


def bare_engine(h=64, w=64):
    """an engine with no weights: the stage needs the device, not the network (and its H, W are not the engine's)"""
    return binding.Engine(h, w, 1, 16, 4, 4, max_batch=2)


def check(eng, masks, values, units, fill, pair, what, want=None):
    """the device's bytes and counts equal the reference's exactly and are the host form's bytes"""
    out, stats = eng.volume_clean(masks, values, units, fill, pair[0], pair[1])
    cr.assert_equal(out, stats, want if want is not None else cr.clean(masks, values, units, fill, pair[0], pair[1]), what)
    h_out, h_stats = binding.volume_clean_host(masks, values, units, fill, pair[0], pair[1])
    assert out.tobytes() == h_out.tobytes() and stats.tobytes() == h_stats.tobytes(), what
    return out, stats


def test_the_cases_are_not_degenerate():
    cr.assert_not_degenerate()


@pytest.mark.parametrize("shape", cr.SHAPES)
def test_device_equals_reference_and_host(shape):
    """every unit triple x radius pair, fill on and off: three values of the label volume and one that is absent, and the binary case"""
    with bare_engine() as eng:
        for units in cr.UNITS:
            for pair in cr.radius_pairs(units):
                for fill in (True, False):
                    where = f"{shape} {units} {pair} fill={fill}"
                    check(eng, cr.case(shape), cr.VALUES, units, fill, pair, where, cr.case_ref(shape, units, pair, fill))
                    check(eng, cr.binary(shape), (1,), units, fill, pair, where + " binary", cr.binary_ref(shape, units, pair, fill))


def test_fill_cases_equal_the_reference():
    with bare_engine() as eng:
        for name, vol, added in cr.fill_cases():
            for units in cr.UNITS:
                _, stats = check(eng, vol, (1,), units, True, (0, 0), name)
                assert stats[0]["filled"] == added, name
            two = np.where(vol == 1, 0, 5).astype(np.uint8)     # the same sets under two values at once: the shell is the plane of 0
            _, stats = check(eng, two, (0, 5), (1, 1, 1), True, (0, 0), name + " two planes")
            assert stats[0]["filled"] == added, name


def test_a_cavity_across_many_workgroups():
    """a shell around 20 x 40 x 300 voxels: its background spans hundreds of 64-lane segments and many workgroups, with a second, open
    shell beside it"""
    vol = np.zeros((24, 44, 640), np.uint8)
    cr._shell(vol, 1, 22, 1, 42, 1, 302)
    cr._shell(vol, 1, 22, 1, 42, 320, 620)
    vol[10, 20, 620] = 0                                        # a tunnel through the second shell's wall
    with bare_engine() as eng:
        out, stats = eng.volume_clean(vol, (1,), (1, 1, 1), True)
    assert stats[0]["filled"] == 20 * 40 * 300 and stats[0]["in_voxels"] == int(vol.sum())
    want = vol.copy()
    want[2:22, 2:42, 2:302] = 1
    assert np.array_equal(out[0], want)
    h_out, h_stats = binding.volume_clean_host(vol, (1,), (1, 1, 1), True)
    assert out.tobytes() == h_out.tobytes() and stats.tobytes() == h_stats.tobytes()


def test_axis_permutations_and_mirrors_commute():
    vol, units = cr.case(PROP_SHAPE), PROP_UNITS
    pair = cr.radius_pairs(units)[0]
    with bare_engine() as eng:
        base_out, base_stats = check(eng, vol, cr.VALUES, units, True, pair, "base", cr.case_ref(PROP_SHAPE, units, pair, True))
        for perm in cr.PERMS:
            pv, pu = cr.permuted(vol, units, perm)
            out, stats = eng.volume_clean(pv, cr.VALUES, pu, True, pair[0], pair[1])
            assert np.array_equal(out, base_out.transpose((0,) + tuple(1 + a for a in perm))) and np.array_equal(stats, base_stats), perm
        for axes in cr.MIRRORS:
            out, stats = eng.volume_clean(np.flip(vol, axes), cr.VALUES, units, True, pair[0], pair[1])
            assert np.array_equal(out, np.flip(base_out, tuple(1 + a for a in axes))) and np.array_equal(stats, base_stats), axes


def test_one_engine_serves_growing_and_shrinking_calls_between_other_stages():
    """before weights are loaded; the workspace grows, then serves smaller calls, and keeps no state; the neighbouring stages'
    workspaces are their own"""
    import score_volume_ref as sr
    import volume_ref as vr

    small, big = cr.SHAPES[3], cr.SHAPES[0]
    calls = [(small, cr.UNITS[1], cr.radius_pairs(cr.UNITS[1])[0], True), (big, cr.UNITS[2], cr.radius_pairs(cr.UNITS[2])[1], True),
             (small, cr.UNITS[1], cr.radius_pairs(cr.UNITS[1])[0], True), (cr.SHAPES[1], cr.UNITS[0], cr.radius_pairs(cr.UNITS[0])[4], False),
             (small, cr.UNITS[0], (0, 0), True)]
    pred, truth = sr.case(sr.SHAPES[1])
    noise = vr.smooth_noise((3, 64, 64))
    with bare_engine(32, 32) as eng:
        for i, (shape, units, pair, fill) in enumerate(calls):
            check(eng, cr.case(shape), cr.VALUES, units, fill, pair, f"call {i}", cr.case_ref(shape, units, pair, fill))
            if i == 1:
                vr.assert_equal(eng.volume_components(noise, vr.NOISE_VALUES, 26, want_ids=True), vr.noise_ref((3, 64, 64), 26))
            if i == 2:
                sr.assert_equal(eng.score_volume(pred, truth, sr.VALUES, sr.UNITS[1]), sr.case_ref(sr.SHAPES[1], sr.UNITS[1], 50000))


def test_out_may_alias_masks():
    shape, units = cr.SHAPES[1], cr.UNITS[1]
    pair = cr.radius_pairs(units)[0]
    vol = np.array(cr.binary(shape))
    stats = np.zeros(1, binding.VCLEAN_DTYPE)
    vals, un = np.array([1], np.int32), np.array(units, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    with bare_engine() as eng:
        rc = binding.lib().mi_unet_volume_clean(eng._h, ptr(vol), *shape, ptr(vals), 1, ptr(un),
                                                C.byref(binding.VolumeCleanOpts(1, pair[0], pair[1])), ptr(vol), ptr(stats))
    assert rc == 0
    cr.assert_equal(vol[None], stats, cr.binary_ref(shape, units, pair, True))


def test_argument_errors_queue_nothing_and_leave_outputs_untouched():
    L = binding.lib()
    with bare_engine() as eng:
        rc, untouched = call_with(L.mi_unet_volume_clean, (eng._h,), {})
        assert rc == 0 and not untouched
        for name, case in earg_cases():
            rc, untouched = call_with(L.mi_unet_volume_clean, (eng._h,), case)
            assert rc == 1 and untouched and b"mi_unet_volume_clean:" in L.mi_unet_last_error(), name
        for name, case in legal_cases():
            assert call_with(L.mi_unet_volume_clean, (eng._h,), case)[0] == 0, name
        rc, untouched = call_with(L.mi_unet_volume_clean, (None,), {})
        assert rc != 0 and untouched
        shape, units = cr.SHAPES[2], cr.UNITS[0]                # the engine still works
        pair = cr.radius_pairs(units)[0]
        check(eng, cr.case(shape), cr.VALUES, units, True, pair, "after the refusals", cr.case_ref(shape, units, pair, True))


# ---- the facade: five RAW slices and their truth files through process_image_batch ----------------------------------------------------------
FACADE_TARGETS = [(1, 0.0), (3, 0.0)]
SPACING = (0.7, 0.7, 3.0)
CLOSE_MM, OPEN_MM = 1.5, 0.8                      # in units of 0.01 mm under 0.7 mm pixels: a disc of 2 pixels, the plus


def series_labels(z):
    """five 64 x 64 label maps that stack into: class 1 -- two blocks over all slices, two pixels apart (the close joins them), the
    first with a 4 x 4 hole in slice 2 alone (a cavity: the slices above and below are solid); class 3 -- a block over slices 1 .. 3.
    The open takes the corners of every block."""
    m = np.zeros((64, 64), np.uint8)
    m[10:30, 10:30] = 1
    m[10:30, 32:44] = 1
    if z == 2:
        m[18:22, 18:22] = 0
    if 1 <= z <= 3:
        m[40:50, 5:25] = 3
    m[0, 0], m[63, 63] = 0, 3                              # both ends of the grey range (test_gpu_targets.raw_of)
    return m


def test_facade_cleans_the_stack_before_it_labels_and_scores_it(tmp_path, monkeypatch):
    import json
    import os

    from miunet import hostlib
    from test_gpu_score_volume import _assert_volume_score
    from test_gpu_targets import blob, raw_of
    from test_gpu_volume import read_stack
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    truth_dir = tmp_path / "truth"
    os.makedirs(truth_dir)
    paths, ws, hs, truth_maps = [], [], [], []
    for z in range(5):
        r = raw_of(series_labels(z), 1 + z % 2)
        paths.append(str(tmp_path / f"s{z}.raw"))
        r.tofile(paths[-1])
        ws.append(r.shape[1]); hs.append(r.shape[0])
        truth_maps.append(np.roll(series_labels(z), (1, -2), (0, 1)))
        truth_maps[-1].tofile(str(truth_dir / f"s{z}_labels.raw"))
    truth_maps = np.stack(truth_maps)
    labels = [c for c, _ in FACADE_TARGETS]
    truths = [np.where(truth_maps == c, 255, 0).astype(np.uint8) for c in labels]
    units, unit_mm = binding.score_volume_units(SPACING, (5, 64, 64))
    assert (units, unit_mm) == ((70, 70, 300), 0.01)
    close_r, open_r = 150, 80
    dirs = {n: tmp_path / n for n in ("never", "off", "on", "host", "keep", "big")}
    for d in dirs.values():
        os.makedirs(d)

    def run(name):
        """the batch into its directory -> what the call added to the log"""
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs[name])) == 5
        return open(hostlib.get_log_path(), "rb").read()[before:].decode()

    def timeless(log, name):
        """the log without its output directory and its numbers (clock readings, rates)"""
        import re
        return re.sub(r"[0-9.]+", "#", log.replace(str(dirs[name]), "DIR"))

    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.set_targets(FACADE_TARGETS)
        assert hostlib.set_volume(True, 26, 0, 0, SPACING) and hostlib.set_truth_dir(str(truth_dir))
        log_never = run("never")
        # set and taken back: every artefact and every log line of a run that never touched the setting
        assert hostlib.set_volume_clean(True, True, CLOSE_MM, OPEN_MM) and hostlib.set_volume_clean(False)
        log_off = run("off")
        names = sorted(os.listdir(dirs["never"]))
        assert names == sorted(os.listdir(dirs["off"])) and "Volume clean" not in log_never
        for n in names:
            assert (dirs["off"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        assert "Volume clean" not in log_off
        assert timeless(log_off, "off") == timeless(log_never, "never")
        # clean only together with `volume on`
        assert hostlib.set_volume(False) and hostlib.set_volume_clean(True, True, CLOSE_MM, OPEN_MM)
        before = len(open(hostlib.get_log_path(), "rb").read())
        assert hostlib.process_image_batch(paths, ws, hs, str(dirs["big"])) == 5
        assert "Volume" not in open(hostlib.get_log_path(), "rb").read()[before:].decode()
        assert not [n for n in os.listdir(dirs["big"]) if "volume" in n]
        # on: the cleaned stack as pictures, the counts in the report, the score of the cleaned stack; the other artefacts unchanged
        assert hostlib.set_volume(True, 26, 0, 0, SPACING)
        log = run("on")
        assert log.count("Volume clean: 5 slices, 2 targets, fill on, close 150, open 80 (unit 0.01 mm), ") == 1
        extra = [f"s{z}_volume_mask_class{c}.png" for z in range(5) for c in labels]
        assert sorted(os.listdir(dirs["on"])) == sorted(names + extra)
        for n in names:
            if n not in ("volume_report.json", "volume_score.json"):
                assert (dirs["on"] / n).read_bytes() == (dirs["never"] / n).read_bytes(), n
        doc = json.loads((dirs["on"] / "volume_report.json").read_bytes())
        plain = json.loads((dirs["never"] / "volume_report.json").read_bytes())
        assert list(doc) == ["slices", "missing", "connectivity", "min_voxels", "keep_largest", "spacing", "clean", "targets"]
        assert list(plain) == [k for k in doc if k != "clean"]
        clean = doc["clean"]
        assert [clean[k] for k in ("fill", "close_mm", "open_mm", "unit_mm", "close_r", "open_r")] == [True, CLOSE_MM, OPEN_MM, unit_mm, close_r, open_r]
        cleaned = []
        for t, c in zip(clean["targets"], labels):
            stack = read_stack(dirs["on"], "s{z}_mask_class{cls}.png", c)       # the pictures this very call wrote
            ref_out, ref_stats = cr.clean(stack, (255,), units, True, close_r, open_r)
            assert t == dict(label=c, **{f: ref_stats[0][f] for f in ("in_voxels", "filled", "closed", "opened", "out_voxels")})
            assert np.array_equal(read_stack(dirs["on"], "s{z}_volume_mask_class{cls}.png", c), ref_out[0])
            cleaned.append(ref_out[0])
        first = clean["targets"][0]                                # not degenerate: every step changes the first target's stack
        assert first["filled"] == 16 and first["closed"] > 0 and first["opened"] > 0
        assert [t["found"] for t in doc["targets"]] == [1, 1] and [t["found"] for t in plain["targets"]] == [2, 1]     # the close joined the blocks
        _assert_volume_score(dirs["on"] / "volume_score.json", cleaned, truths, labels, units, unit_mm)
        assert (dirs["on"] / "volume_score.json").read_bytes() != (dirs["never"] / "volume_score.json").read_bytes()
        # the host form under MEDSEG_HOST_POSTPROCESS=1: the same report, pictures and score
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        run("host")
        monkeypatch.delenv("MEDSEG_HOST_POSTPROCESS")
        for n in ["volume_report.json", "volume_score.json"] + extra:
            assert (dirs["host"] / n).read_bytes() == (dirs["on"] / n).read_bytes(), n
        # with a filter behind it: the filter sees the cleaned stack
        assert hostlib.set_volume(True, 26, 300, 0, SPACING)
        run("keep")
        kept = json.loads((dirs["keep"] / "volume_report.json").read_bytes())
        assert kept["clean"] == clean and [t["kept"] for t in kept["targets"]] == [1, 1]
        # a radius past the limit is reported like any other volume error and fails no image
        assert hostlib.set_volume_clean(True, True, 500.0, 0.0)
        log = run("big")
        assert "Volume clean error: mi_unet_volume_clean: close_r 50000 is outside 0 .. 46340" in log and "Volume: 5 slices" not in log
        assert not [n for n in os.listdir(dirs["big"]) if "volume" in n]
    finally:
        hostlib.set_volume_clean(False)
        hostlib.set_volume(False)
        hostlib.set_truth_dir("")
        hostlib.set_targets([])
        hostlib.cleanup_resources()
