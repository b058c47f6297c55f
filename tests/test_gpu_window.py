"""Intensity windows on the device (include/mi_unet.h: mi_unet_set_window): the exact radix selection, the windowed
quantisation of the resampling and the tiled path, the report of the applied windows, and the default path left where it was.

References: window_ref.py (np.sort for the window, an op-by-op fp64 numpy restatement for the bytes), the oracle for the network,
test_targets_cpu.scipy_target_mask and oracle_lib.find_contours behind it.  Integer / byte work: every comparison is exact.
One 64 x 64 engine of max_batch 4 with an intensity-classifier network (test_gpu_targets.threshold_weights)."""
import functools

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_gpu_targets import assert_same_results, call_segment, contours_of, threshold_weights
from test_targets_cpu import scipy_target_mask
from window_ref import HOT, SPREAD, WRAP, nine_planes, ref_normalise, ref_resample, ref_window

pytestmark = pytest.mark.gpu

EARG, ESTATE = 1, 5
T = 64
CLIPS = [(5000, 5000), (0, 20000), (999, 0)]


@functools.lru_cache(maxsize=None)
def blob():
    spec = UNetSpec(in_ch=1, base=16, levels=4, classes=3)
    return pack_weights(spec, threshold_weights(spec))


def engine(max_batch=4):
    eng = binding.Engine(T, T, 1, 16, 4, 3, max_batch=max_batch)
    eng.load_weights(blob())
    return eng


@functools.lru_cache(maxsize=None)
def default_run():
    """the nine planes under the default setting: (tiles, labels), the windows reported, and the arrays of segment_raw16"""
    with engine() as eng:
        with pytest.raises(binding.MiUnetError) as e:
            eng.last_windows()
        assert e.value.code == ESTATE                                           # no RAW-in call yet
        tiles, labels, _ = eng.infer_raw16(list(nine_planes()))
        wins = eng.last_windows()
        seg = call_segment(binding.lib().mi_unet_segment_raw16, eng._h, nine_planes(), 0, 4096, 64, T, T)
    return tiles, labels, wins, seg


@functools.lru_cache(maxsize=None)
def percentile_run(clip):
    with engine() as eng:
        eng.set_window("percentile", *clip)
        tiles, labels, _ = eng.infer_raw16(list(nine_planes()))
        return tiles, labels, eng.last_windows()


@pytest.mark.parametrize("clip", CLIPS, ids=lambda c: f"{c[0]}-{c[1]}ppm")
def test_selection_is_exact_and_bytes_follow(clip):
    tiles, labels, wins = percentile_run(clip)
    assert wins.shape == (9, 2) and wins.dtype == np.int32
    for i, p in enumerate(nine_planes()):
        want = ref_window(p, *clip)
        print(f"plane {i} {p.shape}: window {tuple(wins[i])}, reference {want}")
        assert tuple(wins[i]) == want, (i, p.shape)
        assert np.array_equal(tiles[i], ref_resample(p, *want, T, T)), i
    assert np.array_equal(labels, orc.unet_forward(blob(), tiles[..., None], want_logits=False)[1])


def test_selection_past_the_grid_cap():
    """above 512 workgroups x 1024 vectors = 4194304 samples a lane takes more than one trip of its four-load loop: 2200 x 2048,
    the ranks under different high bytes"""
    rng = np.random.default_rng(5)
    big = rng.integers(0, 40000, (2200, 2048)).astype(np.uint16)
    with engine(max_batch=1) as eng:
        eng.set_window("percentile", 123456, 234567)
        tiles, _, _ = eng.infer_raw16([big])
        want = ref_window(big, 123456, 234567)
        assert tuple(eng.last_windows()[0]) == want
        assert np.array_equal(tiles[0], ref_resample(big, *want, T, T))


def test_last_windows_in_minmax_mode_and_default_bytes():
    tiles, labels, wins, _ = default_run()
    for i, p in enumerate(nine_planes()):
        assert tuple(wins[i]) == (int(p.min()), int(p.max())), i
        assert np.array_equal(tiles[i], orc.preprocess_raw(p, T, T)), i


def test_nothing_moved():
    tiles, labels, wins, seg = default_run()
    planes = nine_planes()
    L = binding.lib()
    with engine() as eng:
        eng.set_window("percentile", 0, 0)
        assert eng.get_window() == {"mode": "percentile", "clip_lo_ppm": 0, "clip_hi_ppm": 0, "lo": 0, "hi": 65535}
        t0, l0, _ = eng.infer_raw16(list(planes))
        assert np.array_equal(t0, tiles) and np.array_equal(l0, labels)          # the u16 wrap case (all 65535) included
        assert np.array_equal(eng.last_windows(), wins)
        assert not t0[WRAP].any()
        assert_same_results(call_segment(L.mi_unet_segment_raw16, eng._h, planes, 0, 4096, 64, T, T), seg)
        with eng.clone() as other:
            assert other.get_window()["mode"] == "minmax"                       # a clone starts at the default
            t2, l2, _ = other.infer_raw16(list(planes))
            assert np.array_equal(t2, tiles) and np.array_equal(l2, labels)
        # a fixed window at a plane's own min and max
        for i in (SPREAD, HOT, 3):
            eng.set_window("fixed", lo=int(planes[i].min()), hi=int(planes[i].max()))
            t1, l1, _ = eng.infer_raw16([planes[i]])
            assert np.array_equal(t1[0], tiles[i]) and np.array_equal(l1[0], labels[i]), i
            assert eng.last_windows().tolist() == [[int(planes[i].min()), int(planes[i].max())]]
        eng.set_window(None)
        assert eng.get_window()["mode"] == "minmax"
        t3, l3, _ = eng.infer_raw16(list(planes))
        assert np.array_equal(t3, tiles) and np.array_equal(l3, labels)
        assert_same_results(call_segment(L.mi_unet_segment_raw16, eng._h, planes, 0, 4096, 64, T, T), seg)


def test_the_window_changes_what_the_network_sees():
    tiles, labels, _, _ = default_run()
    wt, wl, wins = percentile_run((5000, 5000))
    assert len(np.unique(tiles[HOT])) < 40 and len(np.unique(wt[HOT])) > 100    # one hot and one dead pixel flatten the min/max tile
    assert (tiles[HOT] != wt[HOT]).mean() > 0.9
    assert (labels[HOT] != wl[HOT]).any() and len(np.unique(wl[HOT])) == 3 and len(np.unique(labels[HOT])) < 3


def test_set_window_validation():
    with engine() as eng:
        eng.set_window("percentile", 1000, 2000)
        good = eng.get_window()
        bad = [dict(mode=3), dict(mode=-1), dict(mode="percentile", clip_lo_ppm=-1), dict(mode="percentile", clip_hi_ppm=-5),
               dict(mode="percentile", clip_lo_ppm=500000, clip_hi_ppm=500000), dict(mode="percentile", clip_lo_ppm=1000000),
               dict(mode="fixed", lo=-1, hi=10), dict(mode="fixed", lo=10, hi=10), dict(mode="fixed", lo=11, hi=10),
               dict(mode="fixed", lo=0, hi=65536)]
        for kw in bad:
            with pytest.raises(binding.MiUnetError) as e:
                eng.set_window(**kw)
            assert e.value.code == EARG, kw
            assert eng.get_window() == good, kw
        eng.set_window("percentile", 499999, 500000)                            # k_lo + k_hi = n - 1 at most: legal
        eng.set_window("fixed", lo=0, hi=65535, clip_lo_ppm=-7)                 # fields the mode does not use are ignored
        eng.set_window("minmax", lo=9, hi=3)


def test_fixed_windows_and_the_tiled_path():
    rng = np.random.default_rng(9)
    img = np.clip(rng.normal(3000.0, 400.0, (150, 200)), 0, 65535).astype(np.uint16)
    img[3, 5], img[100, 100] = 65535, 0
    with engine() as eng:
        norm0, lab0, _ = eng.infer_tiled_raw16(img, 8)
        assert eng.last_windows().tolist() == [[0, 65535]]
        for mode, args, want in (("percentile", (5000, 5000), ref_window(img, 5000, 5000)), ("percentile", (0, 0), (0, 65535)),
                                 ("fixed", (0, 0, 2500, 3500), (2500, 3500)), ("fixed", (0, 0, 0, 65535), (0, 65535))):
            eng.set_window(mode, *args)
            norm, lab, _ = eng.infer_tiled_raw16(img, 8)
            assert eng.last_windows().tolist() == [list(want)], (mode, args)
            assert np.array_equal(norm, ref_normalise(img, *want)), (mode, args)
            if want == (0, 65535):
                assert np.array_equal(norm, norm0) and np.array_equal(lab, lab0)
        assert (ref_normalise(img, 2500, 3500) != norm0).mean() > 0.9
        # the resampling path under fixed windows narrower and wider than the data
        for lo, hi in ((2800, 3200), (0, 65535), (100, 60000)):
            eng.set_window("fixed", lo=lo, hi=hi)
            tiles, _, _ = eng.infer_raw16([img, nine_planes()[2]])
            assert np.array_equal(tiles[0], ref_resample(img, lo, hi, T, T))
            assert np.array_equal(tiles[1], ref_resample(nine_planes()[2], lo, hi, T, T))
            assert eng.last_windows().tolist() == [[lo, hi]] * 2


def test_three_channels_have_three_windows():
    spec = UNetSpec(in_ch=3, base=16, levels=3, classes=3)
    planes = [nine_planes()[HOT], nine_planes()[SPREAD], nine_planes()[4], nine_planes()[3]]
    with binding.Engine(T, T, 3, 16, 3, 3, max_batch=2) as eng:
        eng.load_weights(pack_weights(spec, synth.make_weights(spec, 4321)))
        eng.set_window("percentile", 5000, 5000)
        tiles, _, _ = eng.infer_raw16(planes[:3] + [planes[3]] * 3)
        wins = eng.last_windows()
        want = [ref_window(p, 5000, 5000) for p in planes]
        assert wins.tolist() == [list(w) for w in want[:3]] + [list(want[3])] * 3
        assert len({tuple(w) for w in wins[:3].tolist()}) == 3
        for c in range(3):
            assert np.array_equal(tiles[0, :, :, c], ref_resample(planes[c], *want[c], T, T)), c
            assert np.array_equal(tiles[1, :, :, c], ref_resample(planes[3], *want[3], T, T)), c
        big = np.ascontiguousarray(planes[0][:150, :200])
        norm, _, _ = eng.infer_tiled_raw16(big, 8)                               # one array for every channel: scanned once
        w = ref_window(big, 5000, 5000)
        assert eng.last_windows().tolist() == [list(w)] * 3
        for c in range(3):
            assert np.array_equal(norm[:, :, c], ref_normalise(big, *w)), c


def test_through_the_chain_and_the_group():
    targets = [(1, 0.0), (2, 0.01)]
    imgs = [nine_planes()[HOT], synth.make_raw16(150, 200, seed=31)]
    L = binding.lib()
    with engine(max_batch=2) as eng:
        eng.set_targets(targets)
        eng.set_window("percentile", 5000, 5000)
        tiles, masks, xy, start, counts = single = call_segment(L.mi_unet_segment_raw16_multi, eng._h, imgs, 2, 8192, 512, T, T)
        stages = eng.last_stage_ms()
        assert stages["upload_preprocess"] > 0
    for b, img in enumerate(imgs):
        tile = ref_resample(img, *ref_window(img, 5000, 5000), T, T)
        assert np.array_equal(tiles[b], tile), b
        labels = orc.unet_forward(blob(), tile[None, :, :, None], want_logits=False)[1][0]
        for k, (c, f) in enumerate(targets):
            vis = np.where(scipy_target_mask(labels, c, f) != 0, 255, 0).astype(np.uint8)
            assert np.array_equal(masks[b, k], vis), (b, k)
            assert counts[b, k] >= 0
            assert contours_of(xy[b, k], start[b, k], counts[b, k]) == orc.find_contours(vis), (b, k)
    assert (counts > 0).any()
    with binding.Group(T, T, 1, 16, 4, 3, max_batch=2, devices=[0, 0]) as g:
        g.load_weights(blob())
        g.set_targets(targets)
        with pytest.raises(binding.MiUnetError):
            g.set_window("fixed", lo=5, hi=5)
        g.set_window("percentile", 5000, 5000)
        assert_same_results(call_segment(L.mi_unet_group_segment_raw16_multi, g._g, imgs, 2, 8192, 512, T, T), single)
