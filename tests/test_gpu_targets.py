"""Targets on the device (include/mi_unet.h): the multi-target postprocess and every _multi entry point against the
CPU references of test_targets_cpu.py (the scipy restatement of a target's chain, oracle_lib.find_contours), on the label maps the
engine itself returns.  Integer / byte work: every comparison is exact.

The networks are intensity classifiers (threshold_weights below: class c wins between two grey levels), and the RAW images are
built from label maps (raw_of), so the engine reads back exactly the blobs, holes at the area bound and specks that were drawn."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, hostlib, synth
from miunet.spec import UNetSpec, pack_weights
from test_targets_cpu import hand_built_maps, ref_min_area, scipy_target_mask

pytestmark = pytest.mark.gpu

EARG = 1


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


def engine(classes, h=64, w=64, max_batch=2):
    eng = binding.Engine(h, w, 1, 16, 4, classes, max_batch=max_batch)
    eng.load_weights(blob(classes))
    return eng


RAW_SIZES = [(150, 200), (96, 128), (64, 64), (200, 150), (120, 90)]


@functools.lru_cache(maxsize=None)
def raws(n):
    return [synth.make_raw16(h, w, seed=300 + i) for i, (h, w) in enumerate(RAW_SIZES[:n])]


LEVELS = np.array([0, 85, 135, 255], np.uint16)            # a grey level inside each class's band of the 4-class classifier
SQUARES = [(36, 3), (36, 11), (36, 19), (46, 3), (46, 11), (46, 19), (6, 40), (6, 50), (16, 40), (16, 50)]


def crafted_labels(seed):
    """a 64 x 64 label map of all four classes: a class-3 block with a hole just below 1 % of the image, a class-2 block with a
    class-1 island, 5 + seed class-1 squares (one contour each) and single-pixel specks of every class"""
    m = np.zeros((64, 64), np.uint8)
    m[4:30, 4:34] = 3
    m[10:13, 10:23] = 0                                    # 39 pixels: filled at min_area 40
    m[34:60, 30:62] = 2
    m[40:44, 36:40] = 1
    for y, x in SQUARES[:5 + seed]:
        m[y:y + 5, x:x + 5] = 1
    rng = np.random.default_rng(seed)
    for c in (1, 2, 3):
        ys, xs = rng.integers(1, 63, 6), rng.integers(1, 63, 6)
        m[ys, xs] = c
    m[0, 0], m[63, 63] = 0, 3                              # both ends of the grey range: the normalisation is the identity on LEVELS
    return m


def raw_of(labels, factor=1):
    """a RAW16 image that the preprocessing turns into exactly LEVELS[labels]: 16 x the level, `factor` x the size (the top-left
    aligned resample by an integer factor picks every factor-th pixel)"""
    return np.repeat(np.repeat(LEVELS[labels] * 16, factor, axis=0), factor, axis=1).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def crafted(n):
    return [raw_of(crafted_labels(i), 1 + i % 2) for i in range(n)]


def crafted_big():
    m = np.zeros((80, 112), np.uint8)
    m[8:72, 20:84] = crafted_labels(1)                     # across the tile seams of a 64 x 64 grid with halo 8
    m[30:50, 86:110] = 2
    m[2:6, 2:30] = 3                                       # 112 pixels of class 3: kept at frac 0
    m[0, 0], m[79, 111] = 0, 3
    return m


def ref_masks(labels, targets):
    """u8 [K][H][W] in {0, cls}: the CPU reference of every target on one label map"""
    return np.stack([scipy_target_mask(labels, c, f) for c, f in targets])


def call_segment(fn, handle, planes, k, cap_points, cap_contours, h, w):
    """mi_unet_(group_)segment_raw16(_multi) -> the arrays exactly as the C call filled them"""
    planes = [np.ascontiguousarray(r, np.uint16) for r in planes]
    n = len(planes)
    ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in planes])
    ws, hs = (C.c_int * n)(*[r.shape[1] for r in planes]), (C.c_int * n)(*[r.shape[0] for r in planes])
    shape = (n, k) if k else (n,)
    tiles, masks = np.zeros((n, h, w), np.uint8), np.zeros(shape + (h, w), np.uint8)
    xy, start = np.zeros(shape + (cap_points, 2), np.int32), np.zeros(shape + (cap_contours + 1,), np.int32)
    counts = np.zeros(shape, np.int32)
    rc = fn(handle, ptrs, ws, hs, n, tiles.ctypes.data, masks.ctypes.data, xy.ctypes.data, cap_points, start.ctypes.data, cap_contours,
            counts.ctypes.data)
    assert rc == 0, binding.lib().mi_unet_last_error()
    return tiles, masks, xy, start, counts


def contours_of(xy, start, count):
    return [[tuple(q) for q in xy[start[c]:start[c + 1]].tolist()] for c in range(count)]


def assert_same_results(a, b):
    """two (tiles, masks, xy, start, counts) results, any leading shape: tiles, masks and counts whole; of every plane the start
    entries up to its count and the points they delimit (what lies behind them in the caller's arrays is not output)"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].reshape(b[1].shape), b[1])
    ca, cb = a[4].reshape(-1), b[4].reshape(-1)
    assert np.array_equal(ca, cb)
    cap_points, cap1 = a[2].shape[-2], a[3].shape[-1]
    xa, xb = a[2].reshape(-1, cap_points, 2), b[2].reshape(-1, cap_points, 2)
    sa, sb = a[3].reshape(-1, cap1), b[3].reshape(-1, cap1)
    for p in range(ca.size):
        if ca[p] >= 0:
            assert np.array_equal(sa[p, :ca[p] + 1], sb[p, :ca[p] + 1]), p
            assert np.array_equal(xa[p, :sa[p, ca[p]]], xb[p, :sa[p, ca[p]]]), p


def stamp_hole(m, y0, x0, width, area):
    rows, rest = divmod(area, width)
    m[y0:y0 + rows, x0:x0 + width] = 0
    m[y0 + rows, x0:x0 + rest] = 0


def test_postprocess_masks_multi_on_hand_built_maps():
    h, w, targets = 96, 160, [(3, 0.02), (1, 0.06), (2, 0.0)]                   # unsorted on purpose
    ma3, ma1 = ref_min_area(h, w, 0.02), ref_min_area(h, w, 0.06)
    assert (ma3, ma1) == (307, 921)
    comp = np.zeros((h, w), np.uint8)
    comp[2:46, 2:78] = 3; stamp_hole(comp, 6, 8, 60, ma3 - 1)                  # filled
    comp[2:46, 82:158] = 3; stamp_hole(comp, 6, 88, 60, ma3)                   # exactly min_area: stays
    comp[50:96, 0:80] = 1; stamp_hole(comp, 54, 10, 40, ma1 - 1)               # class 1 touches two borders; its hole is filled
    comp[52:90, 90:150] = 2; comp[60:63, 100:103] = 1                          # class 2 with a class-1 island: min_area 0 leaves it
    maps = hand_built_maps(h, w)
    batch = np.stack([maps[0], comp, maps[2]])                                 # B = 3 on max_batch 2: a ragged second micro-batch
    with binding.Engine(h, w, 1, 16, 4, 4, max_batch=2) as eng:
        eng.set_targets(targets)
        got = eng.postprocess_masks_multi(batch)
        eng.set_targets(None)
        single = eng.postprocess_masks_multi(batch)
        assert np.array_equal(single[:, 0], eng.postprocess_masks(batch))      # default target: the single-class stage, bit for bit
    assert got.shape == (3, 3, h, w)
    for b in range(3):
        want = ref_masks(batch[b], targets)
        for k in range(3):
            assert np.array_equal(got[b, k], want[k]), (b, k)
    assert (got[1, 0][6:12, 8:68] == 3).all() and (got[1, 0][6:11, 88:148] == 0).all()
    assert (got[1, 1][54:70, 10:50] == 1).all() and (got[1, 2][60:63, 100:103] == 0).all()      # frac 0 fills nothing
    for k, (c, _) in enumerate(targets):
        assert set(np.unique(got[:, k])) == {0, c}


def test_default_targets_return_the_bytes_of_the_single_class_calls():
    L = binding.lib()
    rs = raws(3)
    with engine(3) as eng:
        assert eng.get_targets() == [(2, pytest.approx(0.06))]
        a = call_segment(L.mi_unet_segment_raw16, eng._h, rs, 0, 2048, 16, 64, 64)
        b = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 1, 2048, 16, 64, 64)
        assert_same_results(a, b)
        assert (a[4] >= 1).all() and (a[1] == 255).any()                        # something was segmented
        big = synth.make_raw16(80, 112, seed=9)
        n0, m0, c0 = eng.segment_tiled_raw16(big, 8, cap_points=4096, cap_contours=32)
        n1, m1, xy, st, cnt = eng.segment_tiled_raw16_multi(big, 8, cap_points=4096, cap_contours=32, raw_arrays=True)
        assert np.array_equal(n0, n1) and np.array_equal(m0, m1[0]) and cnt.shape == (1,) and cnt[0] == len(c0) >= 1
        assert contours_of(xy[0], st[0], cnt[0]) == c0
    with binding.Group(64, 64, 1, 16, 4, 3, max_batch=2, devices=[0, 0]) as g:
        g.load_weights(blob(3))
        ga = call_segment(L.mi_unet_group_segment_raw16, g._g, rs, 0, 2048, 16, 64, 64)
        gb = call_segment(L.mi_unet_group_segment_raw16_multi, g._g, rs, 1, 2048, 16, 64, 64)
    assert_same_results(ga, gb)
    assert_same_results(ga, a)


K3 = [(3, 0.01), (1, 0.0), (2, 0.03)]


@functools.lru_cache(maxsize=None)
def k3_run():
    """B = 5 on max_batch 2 (micro-batches 2, 2, 1), three targets: labels of infer_raw16 and the arrays of the _multi call"""
    with engine(4) as eng:
        _, labels, _ = eng.infer_raw16(crafted(5))
        eng.set_targets(K3)
        out = call_segment(binding.lib().mi_unet_segment_raw16_multi, eng._h, crafted(5), 3, 4096, 256, 64, 64)
        stages = eng.last_stage_ms()
    return labels, out, stages


def test_segment_raw16_multi_three_targets_ragged_batches():
    labels, (tiles, masks, xy, start, counts), stages = k3_run()
    for c in range(4):
        assert (labels == c).any(), c                                         # every class is present
    for b in range(5):
        assert np.array_equal(tiles[b], orc.preprocess_raw(crafted(5)[b], 64, 64))
        assert np.array_equal(labels[b], crafted_labels(b))                    # the classifier reads the crafted map back
        want = ref_masks(labels[b], K3)
        for k in range(3):
            vis = np.where(want[k] != 0, 255, 0).astype(np.uint8)
            assert np.array_equal(masks[b, k], vis), (b, k)
            assert counts[b, k] >= 0
            assert contours_of(xy[b, k], start[b, k], counts[b, k]) == orc.find_contours(vis), (b, k)
    assert (counts.sum(axis=0) > 0).all()                                      # every target found something somewhere
    assert set(stages) == set(binding.Engine.STAGES) and stages["postprocess"] > 0 and stages["contours"] > 0


def test_capacity_overflow_marks_only_the_target_it_hits():
    labels, (tiles, masks, xy, start, counts), _ = k3_run()
    # target 1 (class 1, frac 0: five and more squares, one contour each) needs more contours than the other two anywhere
    others = int(max(counts[:, 0].max(), counts[:, 2].max()))
    assert (counts[:, 1] > others).any(), counts
    with engine(4) as eng:
        eng.set_targets(K3)
        t2, m2, xy2, st2, c2 = call_segment(binding.lib().mi_unet_segment_raw16_multi, eng._h, crafted(5), 3, 4096, others, 64, 64)
    over = counts > others
    assert over.any() and not over[:, 0].any() and not over[:, 2].any()
    assert np.array_equal(c2, np.where(over, -1, counts))
    assert np.array_equal(m2, masks)
    for b in range(5):
        for k in range(3):
            if not over[b, k]:
                assert contours_of(xy2[b, k], st2[b, k], c2[b, k]) == contours_of(xy[b, k], start[b, k], counts[b, k]), (b, k)


def test_tiled_multi_on_the_stitched_image():
    big = raw_of(crafted_big())
    targets = [(2, 0.02), (3, 0.0)]
    with engine(4, max_batch=4) as eng:
        norm0, labels, _ = eng.infer_tiled_raw16(big, 8)
        assert np.array_equal(labels, crafted_big())
        eng.set_targets(targets)
        norm, masks, cont = eng.segment_tiled_raw16_multi(big, 8, cap_points=8192, cap_contours=128)
        assert np.array_equal(norm, norm0) and masks.shape == (2, 80, 112)
        want = ref_masks(labels, targets)                                      # min_area from the full 80 x 112 image
        assert ref_min_area(80, 112, 0.02) == 179
        for k in range(2):
            vis = np.where(want[k] != 0, 255, 0).astype(np.uint8)
            assert np.array_equal(masks[k], vis), k
            assert cont[k] == orc.find_contours(vis), k
        assert len(cont[0]) >= 2 and len(cont[1]) >= 2
    # scratch of max_batch 2: 4 * 2 * 64 * 64 * 16 = 524288 bytes holds one target's contour workspace (30 bytes a pixel) but not two
    with engine(4, max_batch=2) as eng:
        _, m1, c1 = eng.segment_tiled_raw16_multi(big, 8, cap_points=8192, cap_contours=128)
        assert np.array_equal(m1, np.where(ref_masks(labels, [(2, 0.06)]) != 0, 255, 0))
        eng.set_targets(targets)
        with pytest.raises(binding.MiUnetError) as e:
            eng.segment_tiled_raw16_multi(big, 8, cap_points=8192, cap_contours=128)
        assert e.value.code == EARG and "exceeds the scratch buffer" in str(e.value)


def test_set_targets_validation_clone_and_existing_calls():
    rs = raws(2)
    with engine(4) as eng:
        before = eng.segment_raw16(rs, cap_points=2048, cap_contours=32)
        good = [(1, 0.25), (3, 0.0)]
        eng.set_targets(good)
        bad_lists = [[(1, 0.1)] * 1 + [(2, 0.1), (3, 0.1), (1, 0.2)],           # repeated class
                     [(0, 0.1)], [(4, 0.1)], [(-1, 0.1)],                      # class outside 1 .. classes - 1
                     [(1, float("nan"))], [(1, float("inf"))], [(1, -0.01)], [(1, 1.01)],
                     [(1, 0.1), (2, 0.1), (3, 0.1), (1, 0.1), (2, 0.1), (3, 0.1)]]   # more than MI_UNET_MAX_TARGETS
        for bad in bad_lists:
            with pytest.raises(binding.MiUnetError) as e:
                eng.set_targets(bad)
            assert e.value.code == EARG, bad
            assert eng.get_targets() == [(1, 0.25), (3, 0.0)], bad
        assert binding.lib().mi_unet_set_targets(eng._h, None, -1) == EARG and eng.get_targets() == good
        with eng.clone() as other:
            assert other.get_targets() == [(2, pytest.approx(0.06))]           # a clone starts at the default
        after = eng.segment_raw16(rs, cap_points=2048, cap_contours=32)        # existing entry points ignore the setting
        for x, y in zip(before[:2], after[:2]):
            assert np.array_equal(x, y)
        assert before[2] == after[2]
        eng.set_postprocess(True)
        _, post, _ = eng.infer_raw16(rs)
        eng.set_postprocess(False)
        _, labels, _ = eng.infer_raw16(rs)
        for i in range(2):
            assert np.array_equal(post[i], orc.postprocess_mask(labels[i]))
        eng.set_targets([])
        assert eng.get_targets() == [(2, pytest.approx(0.06))]
        eng.set_targets([(1, 1.0), (2, 0.0), (3, 0.5)])
        assert len(eng.get_targets()) == 3


@functools.lru_cache(maxsize=None)
def single_target_run():
    """the entry points without _multi on the four-class maps, B = 5 on max_batch 2 (micro-batches 2, 2, 1): labels of infer_raw16,
    the labels with set_postprocess(1), the arrays of segment_raw16 and its stage times, and the same call with targets set"""
    L = binding.lib()
    with engine(4) as eng:
        _, labels, _ = eng.infer_raw16(crafted(5))
        eng.set_postprocess(True)
        _, post, _ = eng.infer_raw16(crafted(5))
        eng.set_postprocess(False)
        out = call_segment(L.mi_unet_segment_raw16, eng._h, crafted(5), 0, 4096, 64, 64, 64)
        stages = eng.last_stage_ms()
        eng.set_targets(K3)
        with_targets = call_segment(L.mi_unet_segment_raw16, eng._h, crafted(5), 0, 4096, 64, 64, 64)
    return labels, post, out, stages, with_targets


def oracle_chain(labels):
    """postprocess_mask -> mask_to_image -> find_contours of the CPU oracle on one label map"""
    pm = orc.postprocess_mask(labels)
    vis = orc.mask_to_image(pm)
    return pm, vis, orc.find_contours(vis)


def assert_oracle_segment(labels, out):
    tiles, masks, xy, start, counts = out
    for b in range(len(labels)):
        pm, vis, cont = oracle_chain(labels[b])
        assert set(np.unique(vis)) == {0, 255}, b                              # the 832-pixel class-2 block passes min_area 245
        assert (labels[b] == 1).any() and (labels[b] == 3).any()               # ... next to classes the picture must not show
        assert np.array_equal(masks[b], vis), b
        assert counts[b] == len(cont) >= 1, b
        assert contours_of(xy[b], start[b], counts[b]) == cont, b


def test_segment_raw16_on_four_class_maps_equals_the_oracle_chain():
    labels, _, out, stages, _ = single_target_run()
    assert int(64 * 64 * np.float32(0.06)) == 245
    for b in range(5):
        assert np.array_equal(labels[b], crafted_labels(b))
        assert np.array_equal(out[0][b], orc.preprocess_raw(crafted(5)[b], 64, 64))
    assert_oracle_segment(labels, out)
    assert set(stages) == set(binding.Engine.STAGES)
    for name, ms in stages.items():
        assert ms > 0, (name, stages)


def test_set_postprocess_infer_raw16_equals_the_oracle_in_place():
    labels, post, _, _, _ = single_target_run()
    for b in range(5):
        want = orc.postprocess_mask(labels[b])
        assert np.array_equal(post[b], want), b
        assert set(np.unique(post[b])) == {0, 2}, b


def test_targets_on_the_handle_do_not_reach_segment_raw16():
    labels, _, _, _, with_targets = single_target_run()
    assert_oracle_segment(labels, with_targets)                                # still class 2 at 6 %, not K3


def test_segment_tiled_raw16_equals_the_oracle_chain_on_the_stitched_labels():
    big = raw_of(crafted_big())
    with engine(4, max_batch=4) as eng:
        _, labels, _ = eng.infer_tiled_raw16(big, 8)
        _, mask, cont = eng.segment_tiled_raw16(big, 8, cap_points=8192, cap_contours=128)
    assert np.array_equal(labels, crafted_big())
    assert int(80 * 112 * np.float32(0.06)) == 537                             # min_area of the full image: the 832-pixel block stays
    pm, vis, want = oracle_chain(labels)
    assert set(np.unique(vis)) == {0, 255}
    assert np.array_equal(mask, vis) and cont == want and len(want) >= 1


def test_group_of_two_ranks_equals_the_single_handle():
    L = binding.lib()
    rs, targets = crafted(3), [(1, 0.0), (3, 0.01)]
    with engine(4) as eng:
        eng.set_targets(targets)
        want = call_segment(L.mi_unet_segment_raw16_multi, eng._h, rs, 2, 4096, 256, 64, 64)
    with binding.Group(64, 64, 1, 16, 4, 4, max_batch=2, devices=[0, 0]) as g:
        g.load_weights(blob(4))
        with pytest.raises(binding.MiUnetError):
            g.set_targets([(4, 0.1)])
        g.set_targets(targets)
        got = call_segment(L.mi_unet_group_segment_raw16_multi, g._g, rs, 2, 4096, 256, 64, 64)
        tiles, masks, cont = g.segment_raw16_multi(rs, cap_points=4096, cap_contours=256)
    assert_same_results(want, got)
    assert (want[4] >= 0).all() and (want[4].sum(axis=0) > 0).all()
    assert np.array_equal(masks, want[1]) and cont[2][1] == contours_of(want[2][2, 1], want[3][2, 1], want[4][2, 1])


def test_facade_writes_per_target_artefacts(tmp_path, monkeypatch):
    monkeypatch.setenv("MEDSEG_TILE_SIZE", "64")
    monkeypatch.setenv("MEDSEG_MAX_BATCH", "2")
    wpath = tmp_path / "eng" / "net.miw"
    os.makedirs(wpath.parent)
    wpath.write_bytes(blob(4))
    targets = [(1, 0.0), (3, 0.01)]
    sizes = [r.shape for r in crafted(4)]
    paths = []
    for i, r in enumerate(crafted(4)):
        p = tmp_path / f"img{i}.raw"
        r.tofile(p)
        paths.append(str(p))
    with engine(4) as eng:
        _, labels, _ = eng.infer_raw16(crafted(4))
    assert hostlib.initialize_engine(str(wpath), str(tmp_path / "log"))
    try:
        assert not hostlib.set_targets([(4, 0.1)]) and hostlib.get_targets() == [(2, pytest.approx(0.06))]
        assert hostlib.set_targets(targets) and hostlib.get_targets() == [(1, 0.0), (3, pytest.approx(0.01))]
        dev, host = tmp_path / "dev", tmp_path / "host"
        for out_dir, flag in ((dev, "0"), (host, "1")):
            os.makedirs(out_dir)
            monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", flag)
            assert hostlib.process_single_image(paths[0], sizes[0][1], sizes[0][0], str(out_dir))
            assert hostlib.process_image_batch(paths[1:], [w for _, w in sizes[1:]], [h for h, _ in sizes[1:]], str(out_dir)) == 3
        monkeypatch.setenv("MEDSEG_HOST_POSTPROCESS", "0")
        names = sorted(os.listdir(dev))
        assert names == sorted(os.listdir(host))
        for i in range(4):
            base = f"img{i}"
            mine = [n for n in names if n.startswith(base)]
            assert mine == sorted([f"{base}.json", f"{base}_contour_overlay.png", f"{base}_mask_class1.png", f"{base}_mask_class3.png",
                                   f"{base}_normalized.png", f"{base}_original_sizes.json"]), mine
            tile = orc.preprocess_raw(crafted(4)[i], 64, 64)
            assert np.array_equal(hostlib.read_png(str(dev / f"{base}_normalized.png")), tile)
            groups = []
            for c, f in targets:                                                # the CPU chain on the engine's label map
                vis = np.where(hostlib.postprocess_mask_target(labels[i], c, f) != 0, 255, 0).astype(np.uint8)
                assert np.array_equal(vis, np.where(scipy_target_mask(labels[i], c, f) != 0, 255, 0))
                assert np.array_equal(hostlib.read_png(str(dev / f"{base}_mask_class{c}.png")), vis), (i, c)
                groups.append((c, hostlib.extract_contours(vis)))
            oh, ow = sizes[i]
            mapped = [(c, [hostlib.map_points(k, ow / 64, oh / 64) for k in cs]) for c, cs in groups]
            assert (dev / f"{base}.json").read_bytes() == hostlib.polygon_json_text_groups(mapped, base, ow, oh), i
            ov = hostlib.read_png(str(dev / f"{base}_contour_overlay.png"), as_color=True)
            assert np.array_equal(ov, hostlib.draw_overlay_groups(tile, groups)), i      # B,G,R on both sides
            for n in mine:                                                      # the host tail writes the same files, byte for byte
                assert (dev / n).read_bytes() == (host / n).read_bytes(), n
        assert sum(len(cs) for c, cs in groups) > 0
        # back to the default: the single-class artefact names
        assert hostlib.set_targets([])
        back = tmp_path / "back"
        os.makedirs(back)
        assert hostlib.process_single_image(paths[0], sizes[0][1], sizes[0][0], str(back))
        assert "img0_mask.png" in os.listdir(back) and not [n for n in os.listdir(back) if "_mask_class" in n]
    finally:
        hostlib.cleanup_resources()
