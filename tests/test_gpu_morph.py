"""Morphology on the device (include/mi_unet.h: mi_unet_set_morph): the close / open kernel of csrc/morph.hip inside the
multi-target postprocess and every _multi entry point, against the numpy / scipy reference of morph_ref.py on the label maps the
engine itself returns.  Integer / byte work: every comparison is exact.

The networks are the intensity classifiers of test_gpu_targets.py (threshold_weights, copied from there), the RAW images are built
from label maps (raw_of), so the engine reads back exactly the bridges, breaks and corners that were drawn."""
import functools
import os

import numpy as np
import pytest

import morph_ref as mr
import oracle_lib as orc
from miunet import binding, hostlib, synth
from miunet.spec import UNetSpec, pack_weights
from test_gpu_targets import assert_same_results, call_segment, contours_of, raw_of
from test_morph_cpu import morph_maps

pytestmark = pytest.mark.gpu

EARG, ESTATE = 1, 5
SHAPE_NAME = {mr.RECT: "rect", mr.DISC: "disc"}


def threshold_weights(spec):
    """make_threshold_weights for any class count: logit_c = c * x + b_c with x = pixel / 255, the lines crossing at grey levels
    (60.5, 110.5, 160.5, ...) / 255 -- between 8-bit levels, so no pixel ties"""
    t = synth.make_threshold_weights(spec)
    cuts = [(60.5 + 50.0 * j) / 255.0 for j in range(spec.classes - 1)]
    t["outc.w"][:] = 0
    t["outc.b"][:] = 0
    for c in range(spec.classes):
        t["outc.w"][c, 0] = float(c)
        t["outc.b"][c] = -float(sum(cuts[:c]))
    return t


@functools.lru_cache(maxsize=None)
def blob(classes):
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=classes)
    return pack_weights(spec, threshold_weights(spec))


def engine(classes=4, h=64, w=64, max_batch=2):
    eng = binding.Engine(h, w, 1, 16, 4, classes, max_batch=max_batch)
    eng.load_weights(blob(classes))
    return eng


def named(morph):
    return [(SHAPE_NAME[s], o, c) for s, o, c in morph]


@functools.lru_cache(maxsize=None)
def pipeline_maps(h=64, w=64):
    """morph_maps with both ends of the grey range in the corners, so that the normalisation is the identity on raw_of's levels"""
    maps = morph_maps(h, w).copy()
    maps[:, 0, 0], maps[:, h - 1, w - 1] = 0, 3
    return maps


def assert_masks(got, labels, targets, morph, scale=1):
    """got [B][K][H][W] in {0, cls} (scale 1) or 0 / 255 pictures against the reference chain on every label map"""
    for b in range(len(labels)):
        want = mr.masks(labels[b], targets, morph)
        for k in range(len(targets)):
            ref = want[k] if scale == 1 else np.where(want[k] != 0, 255, 0).astype(np.uint8)
            assert np.array_equal(got[b, k], ref), (b, k, morph)


@pytest.mark.parametrize("shape", [mr.RECT, mr.DISC])
@pytest.mark.parametrize("h,w", [(64, 64), (48, 80)])
def test_postprocess_masks_multi_equals_the_reference_for_every_radius(shape, h, w):
    maps = morph_maps(h, w)                                  # B = 3 on max_batch 2: a ragged second micro-batch
    targets = [(2, 0.01)]
    changed = 0
    with binding.Engine(h, w, 1, 16, 4, 4, max_batch=2) as eng:
        eng.set_targets(targets)
        for open_r in (0, 1, 2, 7, 31):                      # 48 x 80 at 31: the element is wider than the image is high
            for close_r in (0, 1, 5):                        # { RECT, 1, 1 } puts the new kernel on the 3x3 element
                morph = [(shape, open_r, close_r)]
                eng.set_morph(named(morph))
                assert eng.get_morph() == named(morph)
                got = eng.postprocess_masks_multi(maps)
                assert_masks(got, maps, targets, morph)
                changed += not np.array_equal(got, np.stack([mr.masks(m, targets, [(mr.RECT, 1, 0)]) for m in maps]))
    assert changed >= 10


def test_three_targets_with_three_entries_and_a_broadcast_entry_in_one_launch():
    maps = morph_maps(64, 64)
    targets = [(3, 0.0), (1, 0.01), (2, 0.02)]
    each = [(mr.DISC, 3, 1), (mr.RECT, 0, 2), (mr.RECT, 31, 0)]
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=2) as eng:
        eng.set_targets(targets)
        eng.set_morph(named(each))
        got = eng.postprocess_masks_multi(maps)
        assert got.shape == (3, 3, 64, 64)
        assert_masks(got, maps, targets, each)
        eng.set_morph([("disc", 2, 1)])                      # n = 1 over K = 3
        assert_masks(eng.postprocess_masks_multi(maps), maps, targets, [(mr.DISC, 2, 1)])
        eng.set_morph([("rect", 1, 0)] * 3)                  # the default, spelled out per target: the 3x3 kernels
        assert_masks(eng.postprocess_masks_multi(maps), maps, targets, [(mr.RECT, 1, 0)])
        eng.set_morph([("rect", 1, 0), ("rect", 0, 0), ("rect", 1, 0)])     # one target with nothing to do beside two defaults
        assert_masks(eng.postprocess_masks_multi(maps), maps, targets, [(mr.RECT, 1, 0), (mr.RECT, 0, 0), (mr.RECT, 1, 0)])


def test_default_returns_the_bytes_of_the_single_class_calls_and_the_setting_does_not_leak():
    L = binding.lib()
    rs = [raw_of(m, 1 + i % 2) for i, m in enumerate(pipeline_maps())]
    with engine() as eng:
        assert eng.get_morph() == [("rect", 1, 0)]
        _, labels, _ = eng.infer_raw16(rs)
        assert np.array_equal(labels, pipeline_maps())        # the classifier reads the maps back
        a = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        b = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 1, 4096, 64, 64, 64)
        assert_same_results(a, b)
        single = eng.postprocess_masks(labels)
        assert np.array_equal(eng.postprocess_masks_multi(labels)[:, 0], single)
        eng.set_morph([("rect", 1, 0)])                      # the default, set explicitly
        assert np.array_equal(eng.postprocess_masks_multi(labels)[:, 0], single)
        # a non-default setting reaches neither the entry points without _multi nor mi_unet_set_postprocess
        eng.set_morph([("disc", 5, 3)])
        assert not np.array_equal(eng.postprocess_masks_multi(labels)[:, 0], single)
        assert np.array_equal(eng.postprocess_masks(labels), single)
        again = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        assert_same_results(a, again)
        eng.set_postprocess(True)
        _, post, _ = eng.infer_raw16(rs)
        eng.set_postprocess(False)
        for i in range(3):
            assert np.array_equal(post[i], orc.postprocess_mask(labels[i])), i
            assert np.array_equal(a[1][i], orc.mask_to_image(orc.postprocess_mask(labels[i]))), i
        assert (a[1] == 255).any()


TARGETS3 = [(2, 0.01), (3, 0.0), (1, 0.0)]
MORPH3 = [(mr.DISC, 2, 1), (mr.RECT, 1, 2), (mr.DISC, 1, 0)]


@functools.lru_cache(maxsize=None)
def raw_run():
    """three images on max_batch 2 (micro-batches 2, 1), three targets with their own entries, measuring on"""
    rs = [raw_of(m, 1 + i % 2) for i, m in enumerate(pipeline_maps())]
    with engine() as eng:
        _, labels, _ = eng.infer_raw16(rs)
        eng.set_targets(TARGETS3)
        eng.set_morph(named(MORPH3))
        eng.set_measure(True)
        out = call_segment(binding.lib().mi_unet_segment_raw16_multi, eng._h, rs, 3, 8192, 256, 64, 64)
        regions, rcounts = eng.last_regions()
    return labels, out, regions, rcounts


def test_segment_raw16_multi_over_a_ragged_batch():
    labels, (tiles, masks, xy, start, counts), _, _ = raw_run()
    assert np.array_equal(labels, pipeline_maps())
    assert_masks(masks, labels, TARGETS3, MORPH3, scale=255)
    for b in range(3):
        for k in range(3):
            assert counts[b, k] >= 0
            assert contours_of(xy[b, k], start[b, k], counts[b, k]) == orc.find_contours(masks[b, k]), (b, k)
    assert (counts.sum(axis=0) > 0).all()                    # every target found something somewhere
    plain = np.stack([np.where(mr.masks(m, TARGETS3, [(mr.RECT, 1, 0)]) != 0, 255, 0) for m in labels])
    assert not np.array_equal(masks, plain)                  # ... and the setting mattered


def test_region_areas_are_the_pixel_counts_of_the_reference_components():
    labels, (_, masks, _, _, counts), regions, rcounts = raw_run()
    assert regions.shape[0] == 9 and np.array_equal(rcounts, counts.reshape(-1))
    for b in range(3):
        want = mr.masks(labels[b], TARGETS3, MORPH3)
        for k in range(3):
            areas = mr.component_areas(want[k])
            assert len(areas) == len(orc.find_contours(masks[b, k])), (b, k)      # no component nested in a hole: each has a contour
            p = b * 3 + k
            assert sorted(regions[p, :rcounts[p]]["area"].tolist()) == areas, (b, k)


def big_labels():
    """150 x 200: blocks across the seams of the 64 x 64 tile grid, joined by thin bridges and cut by thin breaks"""
    m = np.zeros((150, 200), np.uint8)
    m[10:70, 12:90] = 2
    m[40, 12:90] = 0                                        # a one-pixel break across a tile seam
    m[30:33, 90:120] = 2                                     # a three-pixel bridge
    m[20:140, 120:170] = 2
    m[60:75, 130:150] = 1                                    # a hole
    m[100:149, 0:60] = 2                                     # touches the left edge; one row short of the bottom
    m[147:150, 170:200] = 2                                  # a sliver in the last, partial block of both axes
    m[90:96, 70:110] = 3
    m[0, 0], m[149, 199] = 0, 3
    return m


def test_tiled_multi_on_the_stitched_image():
    big = raw_of(big_labels())
    targets, morph = [(2, 0.005), (3, 0.0)], [(mr.DISC, 4, 2)]
    with engine(max_batch=4) as eng:
        _, labels, _ = eng.infer_tiled_raw16(big, 8)
        assert np.array_equal(labels, big_labels())
        eng.set_targets(targets[:1])
        eng.set_morph(named(morph))
        _, masks, cont = eng.segment_tiled_raw16_multi(big, 8, cap_points=8192, cap_contours=128)
        want = mr.masks(labels, targets[:1], morph)
        vis = np.where(want[0] != 0, 255, 0).astype(np.uint8)
        assert masks.shape == (1, 150, 200) and np.array_equal(masks[0], vis)
        assert cont[0] == orc.find_contours(vis) and len(cont[0]) >= 1
        assert not np.array_equal(want, mr.masks(labels, targets[:1], [(mr.RECT, 1, 0)]))
        _, single, _ = eng.segment_tiled_raw16(big, 8, cap_points=8192, cap_contours=128)      # without _multi: the 3x3 box, class 2 at 6 %
        assert np.array_equal(single, orc.mask_to_image(orc.postprocess_mask(labels)))


def test_length_mismatch_is_refused_before_anything_runs():
    maps = morph_maps(64, 64)
    rs = [raw_of(m) for m in pipeline_maps()[:2]]
    L = binding.lib()
    with engine() as eng:
        eng.set_targets(TARGETS3)
        eng.set_morph([("disc", 2, 0), ("rect", 1, 1)])      # 2 entries, 3 targets: accepted when set, refused when read
        assert eng.get_morph() == [("disc", 2, 0), ("rect", 1, 1)]
        out = np.full((3, 3, 64, 64), 77, np.uint8)
        assert L.mi_unet_postprocess_masks_multi(eng._h, maps.ctypes.data, 3, out.ctypes.data) == ESTATE
        assert b"morphology list" in L.mi_unet_last_error() and (out == 77).all()
        with pytest.raises(binding.MiUnetError) as e:
            eng.segment_raw16_multi(rs)
        assert e.value.code == ESTATE
        with pytest.raises(binding.MiUnetError) as e:
            eng.segment_tiled_raw16_multi(raw_of(pipeline_maps()[0]), 8)
        assert e.value.code == ESTATE
        eng.segment_raw16(rs)                                # the entry points without _multi do not read the list
        eng.set_morph([("disc", 2, 0), ("rect", 1, 1), ("rect", 0, 0)])
        morph = [(mr.DISC, 2, 0), (mr.RECT, 1, 1), (mr.RECT, 0, 0)]
        assert_masks(eng.postprocess_masks_multi(maps), maps, TARGETS3, morph)      # a later valid call on the same handle
        eng.set_targets(None)                                # set_targets does not touch the list: 3 entries, 1 target
        assert len(eng.get_morph()) == 3
        with pytest.raises(binding.MiUnetError) as e:
            eng.postprocess_masks_multi(maps)
        assert e.value.code == ESTATE


def test_validation_clone_and_group():
    L = binding.lib()
    rs = [raw_of(m, 1 + i % 2) for i, m in enumerate(pipeline_maps())]
    targets, morph = [(2, 0.01), (1, 0.0)], [(mr.DISC, 3, 1), (mr.RECT, 2, 2)]
    with engine() as eng:
        good = named(morph)
        eng.set_morph(good)
        bad_lists = [[(2, 1, 0)], [(-1, 1, 0)], [("rect", -1, 0)], [("rect", 32, 0)], [("disc", 1, -1)], [("disc", 1, 32)],
                     [("rect", 1, 0), ("disc", 40, 0)], [("rect", 1, 0)] * 6]
        for bad in bad_lists:
            with pytest.raises(binding.MiUnetError) as e:
                eng.set_morph(bad)
            assert e.value.code == EARG and eng.get_morph() == good, bad
        assert L.mi_unet_set_morph(eng._h, None, -1) == EARG and eng.get_morph() == good
        with eng.clone() as other:
            assert other.get_morph() == [("rect", 1, 0)]     # a clone starts at the default
        eng.set_targets(targets)
        want = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 2, 8192, 256, 64, 64)
        eng.set_morph(None)
        assert eng.get_morph() == [("rect", 1, 0)]           # NULL restores the default
        eng.set_morph([])
        assert eng.get_morph() == [("rect", 1, 0)]
    with binding.Group(64, 64, 1, 16, 4, 4, max_batch=2, devices=[0, 0]) as g:
        g.load_weights(blob(4))
        g.set_targets(targets)
        g.set_morph([("disc", 1, 1)])
        with pytest.raises(binding.MiUnetError) as e:
            g.set_morph([("disc", 1, 1), ("rect", 32, 0)])   # a bad entry changes no rank
        assert e.value.code == EARG
        for rank in range(2):
            arr, n = (binding.Morph * 5)(), binding.C.c_int()
            assert L.mi_unet_get_morph(L.mi_unet_group_handle(g._g, rank), arr, 5, binding.C.byref(n)) == 0
            assert n.value == 1 and (arr[0].shape, arr[0].open_r, arr[0].close_r) == (1, 1, 1), rank
        g.set_morph(named(morph))
        got = call_segment(L.mi_unet_group_segment_raw16_multi, g._g, rs, 2, 8192, 256, 64, 64)
        g.set_morph([("rect", 1, 0)] * 3)                    # 3 entries, 2 targets
        with pytest.raises(binding.MiUnetError) as e:
            g.segment_raw16_multi(rs)
        assert e.value.code == ESTATE
    assert_same_results(want, got)
    assert_masks(want[1], pipeline_maps(), targets, morph, scale=255)


def test_facade_applies_the_morphology_on_both_tails(tmp_path, monkeypatch):
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    maps = pipeline_maps()[:2]
    paths, sizes = [], []
    for i, m in enumerate(maps):
        r = raw_of(m, 1 + i)
        p = tmp_path / f"img{i}.raw"
        r.tofile(p)
        paths.append(str(p))
        sizes.append(r.shape)
    assert hostlib.set_morphology([("disc", 2, 1)])          # `morph disc 2 1`; needs no engine and survives initialize_engine
    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.get_morphology() == [("disc", 2, 1)]
        for flag in ("0", "1"):
            monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", flag)
            out_dir = tmp_path / f"out{flag}"
            os.makedirs(out_dir)
            assert hostlib.process_single_image(paths[0], sizes[0][1], sizes[0][0], str(out_dir))
            assert hostlib.process_image_batch(paths[1:], [sizes[1][1]], [sizes[1][0]], str(out_dir)) == 1
            for i, m in enumerate(maps):
                names = sorted(n for n in os.listdir(out_dir) if n.startswith(f"img{i}"))
                assert names == sorted([f"img{i}.json", f"img{i}_contour_overlay.png", f"img{i}_mask.png", f"img{i}_normalized.png",
                                        f"img{i}_original_sizes.json"]), names      # the default target list keeps the artefact names
                want = np.where(mr.chain(m, 2, 0.06, mr.DISC, 2, 1) != 0, 255, 0).astype(np.uint8)
                assert np.array_equal(hostlib.read_png(str(out_dir / f"img{i}_mask.png")), want), (flag, i)
                assert not np.array_equal(want, orc.mask_to_image(orc.postprocess_mask(m)))
        for n in os.listdir(tmp_path / "out0"):
            assert (tmp_path / "out0" / n).read_bytes() == (tmp_path / "out1" / n).read_bytes(), n
        log = open(hostlib.get_log_path()).read()
        assert hostlib.set_morphology([]) and "Morphology: rect (open 1, close 0)" in open(hostlib.get_log_path()).read()
        assert "Morphology:" not in log                      # (set before the log existed)
    finally:
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "0")
        hostlib.set_morphology([])
        hostlib.cleanup_resources()
