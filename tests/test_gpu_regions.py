"""Region measurement on the device (include/mi_unet.h: mi_unet_set_measure) against tests/regions_ref.py: the stage
alone on hand-built masks, the RAW pipeline over several micro-batches, the tiled forms, the group, and the state rules.  Every
comparison of region fields is exact."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import oracle_lib as orc
import regions_ref as ref
from miunet import binding, hostlib
from test_gpu_targets import assert_same_results, blob, call_segment, contours_of, crafted, crafted_labels, engine, raw_of

pytestmark = pytest.mark.gpu

EARG, ESTATE = 1, 5
SIZES = [(64, 64), (48, 80)]              # 80-pixel rows: the 64-pixel wave segments straddle rows


def noise(h, w, seed):
    return np.where(np.random.default_rng(seed).random((h, w)) < 0.5, 255, 0).astype(np.uint8)


def stage_masks(h, w):
    """name -> mask u8 [h, w]; 200 is foreground as well as 255, 100 is not (threshold 127)"""
    z = lambda: np.zeros((h, w), np.uint8)
    out = {"empty": z(), "full": np.full((h, w), 255, np.uint8)}
    m = z(); m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 255; out["corners"] = m
    m = z()                                # two combs, teeth alternating inside one 64-pixel segment: a per-root reduction
    m[10, :] = 255; m[31, :] = 200
    m[11:29, 0::4] = 255; m[13:31, 2::4] = 200
    out["combs"] = m
    m = z()                                # a ring with an island in its hole; a pixel of 100 in the hole stays background
    m[5:25, 5:25] = 255; m[8:22, 8:22] = 0; m[13:17, 13:17] = 255; m[9, 9] = 100
    out["ring"] = m
    m = z()                                # more than 16 segments of one component, then one that starts and ends inside runs
    m[0:21, :] = 255; m[30:36, 5:] = 255
    out["long"] = m
    m = z(); m[h - 1, :] = 255; m[:, w - 1] = 255; out["last_row_col"] = m
    for s in range(3):
        out[f"noise{s}"] = noise(h, w, 10 + s)
    return out


@functools.lru_cache(maxsize=None)
def stage_run(h, w):
    masks = stage_masks(h, w)
    names = list(masks)
    batch = np.stack([masks[n] for n in names])
    tiles = np.random.default_rng(h * 1000 + w).integers(0, 256, batch.shape, dtype=np.uint8)
    with binding.Engine(h, w, 1, 16, 4, 3, max_batch=3) as eng:         # 11 masks: micro-batches 3, 3, 3, 2; needs no weights
        regions, counts = eng.measure_regions(batch, tiles, 0, cap_contours=512)
    return names, batch, tiles, regions, counts


@pytest.mark.parametrize("h,w", SIZES)
def test_stage_alone_every_field_of_every_region(h, w):
    names, batch, tiles, regions, counts = stage_run(h, w)
    for i, name in enumerate(names):
        ref.assert_plane(regions[i], counts[i], ref.regions_of(batch[i], tiles[i]), f"{name} {h}x{w}")
    by = dict(zip(names, range(len(names))))
    assert counts[by["empty"]] == 0
    full = regions[by["full"], 0]
    assert counts[by["full"]] == 1 and full["edges"] == 2 * (h + w) and full["area"] == h * w
    assert counts[by["corners"]] == 4 and all(regions[by["corners"], c]["edges"] == 4 for c in range(4))
    assert counts[by["combs"]] == 2
    ring = regions[by["ring"], 0]
    assert counts[by["ring"]] == 1                                        # the island has no contour, so no region
    assert ring["area"] == 400 - 196 and ring["edges"] == 4 * 20 + 4 * 14    # the hole is not area; its border is perimeter
    assert counts[by["long"]] == 2 and regions[by["long"], 1]["area"] == 21 * w
    assert all(counts[by[f"noise{s}"]] > 4 for s in range(3))


def test_stage_alone_on_a_plane_that_ends_inside_a_wave_segment():
    """One 16 x 70 plane, 1120 pixels (an engine of one level takes even sides): six single pixels and a pair in row 2 behind a moat,
    one component over the rest.  The 64-pixel segment 128 .. 191 holds eight components; the large one runs across every 64-pixel
    boundary and across pixel 1024, where the second wave's span begins; that span ends in the middle of a segment"""
    m = np.full((16, 70), 255, np.uint8)
    m[1:4, 0:25] = 0
    m[2, [2, 5, 8, 11, 14, 17, 20, 21]] = 200
    tile = np.random.default_rng(1670).integers(0, 256, m.shape, dtype=np.uint8)
    with binding.Engine(16, 70, 1, 16, 1, 3, max_batch=1) as eng:
        regions, counts = eng.measure_regions(m[None], tile[None], 0, cap_contours=16)
        bare, bare_counts = eng.measure_regions(m[None], None, 0, cap_contours=16)
    ref.assert_plane(regions[0], counts[0], ref.regions_of(m, tile), "crowded 16x70")
    ref.assert_plane(bare[0], bare_counts[0], ref.regions_of(m, None), "crowded 16x70 without a tile")
    assert counts[0] == 8 and sorted(regions[0, :8]["area"].tolist()) == [1] * 6 + [2, 16 * 70 - 75]


def test_contour_overflow_zeroes_only_its_plane():
    names, batch, tiles, regions, counts = stage_run(64, 64)
    pick = [names.index("ring"), names.index("noise0"), names.index("full")]
    with binding.Engine(64, 64, 1, 16, 4, 3, max_batch=3) as eng:
        r4, c4 = eng.measure_regions(batch[pick], tiles[pick], 0, cap_contours=4)
    assert c4.tolist() == [1, -1, 1]
    assert not r4[1].tobytes().strip(b"\0")                               # the whole plane is zero
    for j in (0, 2):
        assert np.array_equal(r4[j], regions[pick[j], :4])


def test_channel_of_an_interleaved_tile():
    rng = np.random.default_rng(77)
    masks = np.stack([stage_masks(64, 64)[n] for n in ("ring", "combs", "noise1")])
    tiles = rng.integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)         # three different planes per image
    with binding.Engine(64, 64, 3, 16, 4, 3, max_batch=2) as eng:
        for ch in (0, 2):
            regions, counts = eng.measure_regions(masks, tiles, ch, cap_contours=512)
            for i in range(3):
                ref.assert_plane(regions[i], counts[i], ref.regions_of(masks[i], tiles[i], ch), f"mask {i} channel {ch}")
            assert all(int(regions[i, 0]["channel"]) == ch for i in range(3))
        regions, counts = eng.measure_regions(masks, None, 0, cap_contours=512)
        for i in range(3):
            ref.assert_plane(regions[i], counts[i], ref.regions_of(masks[i], None), f"mask {i} without a tile")
        r0 = regions[0, 0]
        assert (r0["imin"], r0["imax"], r0["si"], r0["sii"], r0["channel"]) == (0, 0, 0, 0, -1)
        with pytest.raises(binding.MiUnetError) as e:
            eng.measure_regions(masks, tiles, 3)
        assert e.value.code == EARG
        eng.set_measure(True, 2)
        with pytest.raises(binding.MiUnetError) as e:
            eng.set_measure(True, 3)
        assert e.value.code == EARG and eng.get_measure() == {"on": True, "channel": 2}      # the setting is unchanged


def assert_report(regions, counts, masks, tiles_of_plane, cap):
    """the report of a call against the reference computed from the masks and tiles the call RETURNED"""
    masks = masks.reshape((-1,) + masks.shape[-2:])
    assert regions.shape == (len(masks), cap) and counts.shape == (len(masks),)
    for p, m in enumerate(masks):
        ref.assert_plane(regions[p], counts[p], ref.regions_of(m, tiles_of_plane(p)), f"plane {p}")


def test_raw_pipeline_over_micro_batches():
    L = binding.lib()
    rs = crafted(7)                                                       # max_batch 2: four micro-batches, both tile buffers reused
    with engine(4) as eng:
        off = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        eng.set_measure(True)
        on = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        regions, counts = eng.last_regions()
        stages = eng.last_stage_ms()
    assert_same_results(on, off)                                          # measuring changes no byte of the call's own outputs
    assert all(np.array_equal(a, b) for a, b in zip(on, off))             # ... the whole of tiles, masks, xy, start and counts
    tiles, masks = on[0], on[1]
    assert_report(regions, counts, masks, lambda p: tiles[p], 64)
    assert (counts >= 1).all() and np.array_equal(counts, on[4]) and stages["contours"] > 0


def test_regions_do_not_depend_on_cap_points():
    """a plane whose points overflowed (contour count -1) still has its regions, and its region count"""
    L = binding.lib()
    rs = crafted(3)
    with engine(4) as eng:
        eng.set_measure(True)
        full = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        want_regions, want_counts = eng.last_regions()
        short = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 2, 64, 64, 64)       # two points: no contour of a block fits
        regions, counts = eng.last_regions()
    assert (full[4] >= 1).all() and (short[4] == -1).all()
    assert np.array_equal(counts, want_counts) and np.array_equal(counts, full[4]) and np.array_equal(regions, want_regions)
    assert_report(regions, counts, short[1], lambda p: short[0][p], 64)


LEVELS_OF = [np.array([0, 65 + 15 * b, 115 + 15 * b, 165 + 30 * b], np.uint16) for b in range(3)]


def test_multi_plane_reads_its_own_images_tile():
    """K = 2, B = 3: the same label map in three brightnesses (a fixed window makes the tile raw / 16), so plane b * K + k can only
    match the reference when it read image b's tile"""
    L = binding.lib()
    lab = crafted_labels(2)
    rs = [(LEVELS_OF[b][lab] * 16).astype(np.uint16) for b in range(3)]
    targets = [(1, 0.0), (3, 0.01)]
    with engine(4) as eng:
        eng.set_window("fixed", lo=0, hi=4080)
        eng.set_targets(targets)
        off = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 2, 4096, 64, 64, 64)
        eng.set_measure(True)
        on = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 2, 4096, 64, 64, 64)
        regions, counts = eng.last_regions()
    assert_same_results(on, off)
    assert all(np.array_equal(a, b) for a, b in zip(on, off))
    tiles, masks = on[0], on[1]
    for b in range(3):
        assert np.array_equal(tiles[b], LEVELS_OF[b][lab])
    assert_report(regions, counts, masks, lambda p: tiles[p // 2], 64)
    assert np.array_equal(counts.reshape(3, 2), on[4]) and (counts >= 1).all()
    big = [regions[2 * b + 1, np.argmax(regions[2 * b + 1]["area"])] for b in range(3)]      # the class-3 block of every image
    assert [int(r["imax"]) for r in big] == [165, 195, 225]


def tiled_labels():
    m = np.zeros((150, 200), np.uint8)
    m[10:74, 20:84] = crafted_labels(1)                    # across the tile seams of a 64 x 64 grid with halo 8
    m[80:140, 100:190] = 2
    m[90:100, 120:140] = 1
    m[100:130, 10:60] = 3
    m[0, 0], m[149, 199] = 0, 3
    return m


def test_tiled_forms_full_image_coordinates():
    big = raw_of(tiled_labels())
    targets = [(2, 0.02), (3, 0.0)]
    with engine(4, max_batch=8) as eng:
        eng.set_measure(True)
        norm, mask, cont = eng.segment_tiled_raw16(big, 8, cap_points=8192, cap_contours=128)
        regions, counts = eng.last_regions()
        assert_report(regions, counts, mask, lambda p: norm, 128)
        assert counts[0] == len(cont) >= 1 and int(regions[0, 0]["x1"]) >= 64       # beyond one tile: full-image coordinates
        eng.set_targets(targets)
        norm2, masks, cont2 = eng.segment_tiled_raw16_multi(big, 8, cap_points=8192, cap_contours=128)
        regions, counts = eng.last_regions()
        assert np.array_equal(norm2, norm)
        assert_report(regions, counts, masks, lambda p: norm, 128)
        assert counts.tolist() == [len(cont2[0]), len(cont2[1])] and min(counts) >= 2
        eng.set_measure(False)
        _, masks_off, cont_off = eng.segment_tiled_raw16_multi(big, 8, cap_points=8192, cap_contours=128)
        assert np.array_equal(masks_off, masks) and cont_off == cont2
        with pytest.raises(binding.MiUnetError) as e:
            eng.last_regions()
        assert e.value.code == ESTATE


def test_group_report_in_image_order():
    L = binding.lib()
    rs, targets = crafted(5), [(1, 0.0), (3, 0.01)]
    with engine(4) as eng:
        eng.set_targets(targets)
        eng.set_measure(True)
        want = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 2, 4096, 64, 64, 64)
        want_regions, want_counts = eng.last_regions()
    with binding.Group(64, 64, 1, 16, 4, 4, max_batch=2, devices=[0, 0]) as g:
        g.load_weights(blob(4))
        g.set_targets(targets)
        got_off = call_segment(L.mi_unet_group_segment_raw16_multi, g._g, rs, 2, 4096, 64, 64, 64)
        with pytest.raises(binding.MiUnetError) as e:
            g.last_regions()
        assert e.value.code == ESTATE
        with pytest.raises(binding.MiUnetError):
            g.set_measure(True, 1)                                         # in_ch = 1: no rank changes
        g.set_measure(True)
        got = call_segment(L.mi_unet_group_segment_raw16_multi, g._g, rs, 2, 4096, 64, 64, 64)
        regions, counts = g.last_regions()
    assert_same_results(got, want)
    assert_same_results(got, got_off)
    assert regions.shape == (10, 64) and np.array_equal(counts, want_counts) and np.array_equal(regions, want_regions)
    assert_report(regions, counts, got[1], lambda p: got[0][p // 2], 64)


def test_state_rules():
    L = binding.lib()
    rs = crafted(2)
    with engine(4) as eng:
        with pytest.raises(binding.MiUnetError) as e:
            eng.last_regions()                                             # before any call
        assert e.value.code == ESTATE
        assert eng.get_measure() == {"on": False, "channel": 0}
        off = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        with pytest.raises(binding.MiUnetError) as e:
            eng.last_regions()                                             # after a call with measuring off
        assert e.value.code == ESTATE
        eng.set_measure(True)
        with eng.clone() as other:
            assert other.get_measure() == {"on": False, "channel": 0}      # a clone starts off
        on = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        regions, counts = eng.last_regions()
        assert np.array_equal(counts, on[4])
        # the stage-alone calls and the calls that return no contours leave the report alone
        masks = on[1]
        cont = eng.extract_contours(masks, cap_points=4096, cap_contours=64)
        assert cont == [contours_of(on[2][b], on[3][b], on[4][b]) for b in range(2)] == [orc.find_contours(m) for m in masks]
        eng.measure_regions(masks[:1], None, 0, cap_contours=8)
        eng.infer_raw16(rs)
        r2, c2 = eng.last_regions()
        assert np.array_equal(r2, regions) and np.array_equal(c2, counts)
        # query form, and a report cut at cap_planes
        planes, cap = C.c_int(), C.c_int()
        assert L.mi_unet_last_regions(eng._h, None, None, 0, C.byref(planes), C.byref(cap)) == 0 and (planes.value, cap.value) == (2, 64)
        one, n1 = np.zeros((1, 64), binding.REGION_DTYPE), np.full(2, 77, np.int32)
        assert L.mi_unet_last_regions(eng._h, one.ctypes.data, n1.ctypes.data, 1, C.byref(planes), C.byref(cap)) == 0
        assert np.array_equal(one[0], regions[0]) and n1.tolist() == [int(counts[0]), 77] and planes.value == 2
        eng.set_measure(None)                                              # NULL restores the default
        assert eng.get_measure() == {"on": False, "channel": 0}
        again = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        assert_same_results(again, off)
        with pytest.raises(binding.MiUnetError) as e:
            eng.last_regions()
        assert e.value.code == ESTATE


def _shape_regions(doc):
    return [sh["region"] for sh in doc["shapes"]]


def _assert_json_regions(doc, records, ow, oh):
    """the region objects of a document against mi_unet_region_derive of the device's records, one per shape"""
    got = _shape_regions(doc)
    assert len(got) == len(records) >= 1
    for reg, rec in zip(got, records):
        r, d = ref.record(rec), binding.region_derive(rec)
        assert (reg["area"], reg["edges"], reg["imin"], reg["imax"]) == (r["area"], r["edges"], r["imin"], r["imax"])
        assert reg["bbox"] == [r["x0"], r["y0"], r["x1"], r["y1"]] and reg["centroid"] == [d["cx"], d["cy"]]
        assert all(reg[k] == d[k] for k in ("major", "minor", "theta", "mean", "std"))
        assert (reg["scale_x"], reg["scale_y"]) == (ow / 64, oh / 64)


def test_facade_writes_region_objects(tmp_path, monkeypatch):
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    rs = crafted(4)
    sizes = [r.shape for r in rs]
    paths = []
    for i, r in enumerate(rs):
        paths.append(str(tmp_path / f"img{i}.raw"))
        r.tofile(paths[-1])
    L = binding.lib()
    targets = [(1, 0.0), (3, 0.01)]
    with engine(4) as eng:                                      # the device's own report, for the default target and for two targets
        eng.set_measure(True)
        one = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 4096, 64, 64, 64)
        regions1, counts1 = eng.last_regions()
        eng.set_targets(targets)
        two = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 2, 4096, 64, 64, 64)
        regions2, counts2 = eng.last_regions()
    assert (counts1 >= 1).all() and (counts2 >= 1).all()
    others = ["_contour_overlay.png", "_mask.png", "_normalized.png", "_original_sizes.json"]
    assert hostlib.set_measure(True)                            # before the engine exists: the setting survives initialize_engine
    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        assert hostlib.get_measure() == {"on": True, "channel": 0}
        assert not hostlib.set_measure(True, 1) and hostlib.get_measure() == {"on": True, "channel": 0}      # in_ch = 1
        on, off = tmp_path / "on", tmp_path / "off"
        os.makedirs(on), os.makedirs(off)
        assert hostlib.process_single_image(paths[0], sizes[0][1], sizes[0][0], str(on))              # the thread's context
        assert hostlib.process_image_batch(paths[1:], [w for _, w in sizes[1:]], [h for h, _ in sizes[1:]], str(on)) == 3      # the group
        assert hostlib.set_measure(False)
        assert hostlib.process_single_image(paths[0], sizes[0][1], sizes[0][0], str(off))
        assert hostlib.process_image_batch(paths[1:], [w for _, w in sizes[1:]], [h for h, _ in sizes[1:]], str(off)) == 3
        assert sorted(os.listdir(on)) == sorted(os.listdir(off))
        for i in range(4):
            base, (oh, ow) = f"img{i}", sizes[i]
            for tail in others:                                 # the other four artefacts: byte-identical
                assert (on / (base + tail)).read_bytes() == (off / (base + tail)).read_bytes(), (i, tail)
            doc, plain = json.loads((on / f"{base}.json").read_bytes()), json.loads((off / f"{base}.json").read_bytes())
            assert all("region" not in sh for sh in plain["shapes"])
            _assert_json_regions(doc, regions1[i, :counts1[i]], ow, oh)
            for sh in doc["shapes"]:
                del sh["region"]
            assert doc == plain
        # several targets: shapes group after group, plane i * K + k
        assert hostlib.set_targets(targets) and hostlib.set_measure(True)
        multi = tmp_path / "multi"
        os.makedirs(multi)
        assert hostlib.process_single_image(paths[0], sizes[0][1], sizes[0][0], str(multi))
        assert hostlib.process_image_batch(paths[1:], [w for _, w in sizes[1:]], [h for h, _ in sizes[1:]], str(multi)) == 3
        for i in range(4):
            doc = json.loads((multi / f"img{i}.json").read_bytes())
            recs = np.concatenate([regions2[2 * i + k, :counts2[2 * i + k]] for k in range(2)])
            _assert_json_regions(doc, recs, sizes[i][1], sizes[i][0])
            assert [sh["labelIndex"] for sh in doc["shapes"]] == [0] * counts2[2 * i] + [1] * counts2[2 * i + 1]
        # a host tail traces on the CPU: no region objects, the document of a run with measuring off
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "1")
        assert hostlib.set_targets([])
        host = tmp_path / "host"
        os.makedirs(host)
        assert hostlib.process_single_image(paths[0], sizes[0][1], sizes[0][0], str(host))
        assert (host / "img0.json").read_bytes() == (off / "img0.json").read_bytes()
    finally:
        hostlib.set_measure(False)
        hostlib.cleanup_resources()


def test_settings_reach_the_second_lane_and_thread_contexts(tmp_path, monkeypatch):
    """16 files is the smallest directory-mode call that creates the second device lane; with max_batch 2 it is 8 chunks alternating
    between the lanes.  State `a` (measure on, a fixed window 0 .. 4400) is set before the engine exists, so the lane and the thread's
    context are created after the settings and must take them at creation; `b` (measure off, min/max) and `c` (measure on, a 1 %
    percentile window) are set after both exist.  In every state each of the five artefacts of file j is, byte for byte, that of
    process_single_image -- the calling thread's context -- on its source.  The fixed window maps the levels 1360 / 2160 / 4080 of the
    crafted images to 79 / 125 / 236, inside the same class bands (cuts at 60.5, 110.5, 160.5), so `a`'s tiles differ from `b`'s on
    every image: a lane or a context that missed the window at its creation would write `b`'s.  On these images both ends of the grey
    range hold far more than 1 % of the samples, so the window of `c` is the min/max window and `c`'s tiles are `b`'s (only the size JSON
    names the window)."""
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    rs = crafted(4)
    for i, r in enumerate(rs):
        r.tofile(tmp_path / f"src{i}.raw")
    many, mw, mh = [], [], []
    for j in range(16):
        os.symlink(tmp_path / f"src{j % 4}.raw", tmp_path / f"m{j:02d}.raw")
        many.append(str(tmp_path / f"m{j:02d}.raw")); mw.append(rs[j % 4].shape[1]); mh.append(rs[j % 4].shape[0])
    tails = ["_normalized.png", "_original_sizes.json", "_mask.png", "_contour_overlay.png", ".json"]

    def run(state):
        """directory mode into <state>, the four sources one by one into <state>_single; -> the artefacts of both, by (name, tail)"""
        batch, single = tmp_path / state, tmp_path / (state + "_single")
        os.makedirs(batch), os.makedirs(single)
        assert hostlib.process_image_batch(many, mw, mh, str(batch)) == 16
        for i, r in enumerate(rs):
            assert hostlib.process_single_image(str(tmp_path / f"src{i}.raw"), r.shape[1], r.shape[0], str(single))
        assert len(os.listdir(batch)) == 16 * 5 and len(os.listdir(single)) == 4 * 5
        got = {(j, t): (batch / f"m{j:02d}{t}").read_bytes() for j in range(16) for t in tails}
        want = {(i, t): (single / f"src{i}{t}").read_bytes() for i in range(4) for t in tails}
        for (j, t), data in got.items():
            w = want[(j % 4, t)]
            if t.endswith(".json"):                             # the documents name their file
                w = w.replace(f"src{j % 4}.raw".encode(), f"m{j:02d}.raw".encode())
            assert data == w, (state, j, t)
        return got

    assert hostlib.set_measure(True) and hostlib.set_window("fixed", lo=0, hi=4400)
    try:
        assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
        a = run("a")
        assert hostlib.set_measure(False) and hostlib.set_window("minmax")
        b = run("b")
        assert hostlib.set_measure(True) and hostlib.set_window("percentile", 10000, 10000)
        c = run("c")
        for j in range(16):
            for got, measured in ((a, True), (b, False), (c, True)):
                shapes = json.loads(got[(j, ".json")])["shapes"]
                assert len(shapes) >= 1 and all(("region" in sh) == measured for sh in shapes), j
            assert a[(j, "_normalized.png")] != b[(j, "_normalized.png")], j
            assert b'"window_lo"' in c[(j, "_original_sizes.json")] and b'"window_lo"' not in b[(j, "_original_sizes.json")]
            assert c[(j, "_normalized.png")] == b[(j, "_normalized.png")]
    finally:
        hostlib.set_measure(False)
        hostlib.set_window("minmax")
        hostlib.cleanup_resources()
