"""Targets (include/mi_unet.h) without a device: the min_area arithmetic, the host postprocess_mask(src, cls, frac),
the grouped polygon document, and the new symbols.

References: oracle_lib.postprocess_mask (the restatement of the single-class chain) on the label map remapped so that the target
class becomes 2 and everything else 0, and for other fractions a scipy restatement of the chain written here after
tests/golden/make_golden.py (label with the 8-neighbourhood, binary_erosion(border_value=1), binary_dilation(border_value=0)).
Everything is integer work: every comparison is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, hostlib


def ref_min_area(h, w, frac):
    return int(np.float32(w * h) * np.float32(frac))


def scipy_target_mask(labels, cls, frac):
    """the chain of a target on one label map -> u8 in {0, cls}"""
    from scipy import ndimage as ndi

    h, w = labels.shape
    s8 = np.ones((3, 3), bool)
    min_area = ref_min_area(h, w, frac)
    fg = labels == cls
    lab, n = ndi.label(~fg, structure=s8)
    for i, sl in enumerate(ndi.find_objects(lab), start=1):
        ys, xs = sl
        comp = lab[sl] == i
        if xs.start > 0 and ys.start > 0 and xs.stop - 1 < w - 1 and ys.stop - 1 < h - 1 and int(comp.sum()) < min_area:
            fg[sl] |= comp
    op = ndi.binary_dilation(ndi.binary_erosion(fg, s8, border_value=1), s8, border_value=0)
    lab, n = ndi.label(op, structure=s8)
    out = np.zeros((h, w), np.uint8)
    if n:
        areas = np.bincount(lab.ravel(), minlength=n + 1)
        keep = areas >= min_area
        keep[0] = False
        out[keep[lab]] = cls
    return out


def hand_built_maps(h, w, classes=4):
    """three label maps with blobs of every class, holes just below and exactly at a threshold, border contact and a speck"""
    maps = []
    a = np.zeros((h, w), np.uint8)
    a[6:h - 6, 6:w // 2] = 3
    a[12:20, 12:40] = 0                                   # hole inside class 3
    a[0:h // 3, w // 2 + 8:w] = 1                         # touches the top and right edges
    a[h // 2:h - 4, w // 2 + 4:w - 4] = 2
    a[h // 2 + 6:h // 2 + 10, w // 2 + 10:w // 2 + 14] = 1     # class 1 island inside class 2: a hole of class 2, a speck of class 1
    a[2, 2] = 2                                           # speck
    maps.append(a)
    b = np.full((h, w), 1, np.uint8)
    b[10:h - 10, 10:w - 10] = 2
    b[h // 2 - 8:h // 2 + 8, 30:w - 30] = 3
    b[h // 2, 30:w - 30] = 0                              # a one-pixel slit: gone after the open
    b[0, :] = 0
    maps.append(b)
    rng = np.random.default_rng(7)
    f = rng.random((h, w))
    for _ in range(4):
        f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5
    c = np.digitize(f, np.quantile(f, [0.4, 0.6, 0.8])).astype(np.uint8)
    c[rng.random((h, w)) < 0.03] = 0
    maps.append(c)
    assert all(set(np.unique(m)) <= set(range(classes)) for m in maps)
    return np.stack(maps)


def threshold_hole_maps(h, w, cls, frac):
    """a block of `cls` with a hole of min_area - 1 pixels (filled) and one with a hole of exactly min_area (not filled)"""
    ma = ref_min_area(h, w, frac)
    assert ma >= 4
    out = []
    for area in (ma - 1, ma):
        m = np.zeros((h, w), np.uint8)
        m[2:h - 2, 2:w - 2] = cls
        width = w - 12
        rows, rest = divmod(area, width)
        m[6:6 + rows, 6:6 + width] = 0
        m[6 + rows, 6:6 + rest] = 0
        assert int((m[2:h - 2, 2:w - 2] == 0).sum()) == area
        out.append(m)
    return out


@pytest.mark.parametrize("h,w,frac,known", [(512, 512, 0.06, 15728), (96, 160, 0.06, 921), (64, 64, 0.0, 0), (64, 64, 1.0, 4096),
                                            (100, 100, 0.0123, None), (100, 100, 0.3, None), (10, 10, 0.07, None)])
def test_target_min_area_is_the_float_product(h, w, frac, known):
    want = ref_min_area(h, w, frac)
    if known is not None:
        assert want == known
    assert binding.target_min_area(h, w, frac) == want


def test_target_min_area_straddles_an_integer_boundary():
    # 10000 * frac around 300: the float32 product decides on which side of the integer the bound falls
    below, above = np.nextafter(np.float32(0.03), np.float32(0)), np.nextafter(np.float32(0.03), np.float32(1))
    got = [binding.target_min_area(100, 100, float(f)) for f in (below, np.float32(0.03), above)]
    assert got == [ref_min_area(100, 100, f) for f in (below, np.float32(0.03), above)]
    assert got[0] == 299 and got[2] == 300


@pytest.mark.parametrize("cls", [1, 2, 3])
def test_host_target_mask_equals_the_oracle_on_the_remapped_goldens(golden_dir, cls):
    g = np.load(os.path.join(golden_dir, "imgproc.npz"))
    for i in range(4):
        m = g[f"mask{i}"]                                 # {0, 1, 2}: class 2 takes the role of `cls`, the others move out of the way
        relabelled = np.where(m == 2, cls, np.where(m == 1, (cls % 3) + 1, 0)).astype(np.uint8)
        got = hostlib.postprocess_mask_target(relabelled, cls, 0.06)
        remapped = np.where(relabelled == cls, 2, 0).astype(np.uint8)
        want = orc.postprocess_mask(remapped)
        assert np.array_equal(got, np.where(want == 2, cls, 0)), (cls, i)
        assert np.array_equal(want, g[f"final{i}"])        # classes other than 2 never mattered to the chain
    one = g["mask0"]
    assert np.array_equal(hostlib.postprocess_mask_target(one, 2, 0.06), hostlib.postprocess_mask(one))


@pytest.mark.parametrize("frac", [0.01, 0.0, 0.06])
def test_host_target_mask_equals_the_scipy_restatement(frac):
    maps = list(hand_built_maps(96, 160))
    for cls in (1, 2, 3):
        cases = maps + (threshold_hole_maps(96, 160, cls, frac) if frac > 0 else [])
        for i, m in enumerate(cases):
            got = hostlib.postprocess_mask_target(m, cls, frac)
            assert np.array_equal(got, scipy_target_mask(m, cls, frac)), (frac, cls, i)
            assert set(np.unique(got)) <= {0, cls}


def test_hole_of_min_area_minus_one_is_filled_and_of_min_area_is_not():
    for cls, frac in ((1, 0.01), (3, 0.06)):
        filled, kept = threshold_hole_maps(96, 160, cls, frac)
        a, b = hostlib.postprocess_mask_target(filled, cls, frac), hostlib.postprocess_mask_target(kept, cls, frac)
        assert (a[2:-2, 2:-2] == cls).all()
        assert int((b[2:-2, 2:-2] == 0).sum()) >= ref_min_area(96, 160, frac)
        assert np.array_equal(a, scipy_target_mask(filled, cls, frac)) and np.array_equal(b, scipy_target_mask(kept, cls, frac))


SQUARE = [(3, 4), (3, 9), (8, 9), (8, 4)]
TRI = [(20, 20), (25, 30), (30, 20)]


def test_grouped_polygon_document(tmp_path):
    path = tmp_path / "one.json"
    hostlib.generate_json([SQUARE, TRI], str(path), "img", 640, 480)
    existing = path.read_bytes()
    assert hostlib.polygon_json_text_groups([(2, [SQUARE, TRI])], "img", 640, 480) == existing      # the default target
    hostlib.generate_json([], str(path), "img", 640, 480)
    assert hostlib.polygon_json_text_groups([(2, [])], "img", 640, 480) == path.read_bytes()

    doc = hostlib.polygon_json_text_groups([(3, [SQUARE]), (1, []), (2, [TRI, SQUARE])], "img", 640, 480)
    d = json.loads(doc)
    assert [(s["label"], s["labelIndex"]) for s in d["shapes"]] == [(3, 0), (2, 2), (2, 2)]           # the empty group: no shape
    assert d["shapes"][0]["points"] == [list(p) for p in SQUARE] and d["shapes"][1]["points"] == [list(p) for p in TRI]
    # the rest of the document as the single-class one: same bytes once the label pairs are put back
    again = doc.replace(b'"label": 3,', b'"label": 1,').replace(b'"label": 2,', b'"label": 1,').replace(b'"labelIndex": 2,', b'"labelIndex": 0,')
    hostlib.generate_json([SQUARE, TRI, SQUARE], str(path), "img", 640, 480)
    assert again == path.read_bytes()
    # one non-default class alone keeps its own label
    assert json.loads(hostlib.polygon_json_text_groups([(1, [TRI])], "img", 64, 64))["shapes"][0]["label"] == 1
    assert json.loads(hostlib.polygon_json_text_groups([(3, [TRI])], "img", 64, 64))["shapes"][0]["label"] == 3


def test_grouped_overlay_uses_the_palette_and_starts_with_red():
    gray = np.full((40, 48), 90, np.uint8)
    assert np.array_equal(hostlib.draw_overlay_groups(gray, [(2, [SQUARE, TRI])]), hostlib.draw_overlay(gray, [SQUARE, TRI]))
    ov = hostlib.draw_overlay_groups(gray, [(1, [SQUARE]), (3, [TRI])])
    assert tuple(ov[4, 3]) == (0, 0, 255) and tuple(ov[20, 20]) == (0, 255, 0)                    # B,G,R: red, then green
    assert (ov[0, 0] == 90).all()


NEW_SYMBOLS = ["mi_unet_target_min_area", "mi_unet_set_targets", "mi_unet_get_targets", "mi_unet_postprocess_masks_multi",
               "mi_unet_segment_raw16_multi", "mi_unet_segment_tiled_raw16_multi", "mi_unet_group_set_targets",
               "mi_unet_group_segment_raw16_multi"]


def test_new_symbols_are_exported_and_bound_without_a_device():
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported and set(NEW_SYMBOLS) <= set(binding.EXPORTS)
    L = binding.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", hostlib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    host = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"medseg_postprocess_mask_target", "medseg_set_targets", "medseg_get_targets", "medseg_polygon_json_text_groups",
            "medseg_draw_overlay_groups"} <= host
    # null handles are refused, not dereferenced
    n = binding.C.c_int()
    assert L.mi_unet_set_targets(None, None, 0) == 1 and L.mi_unet_get_targets(None, None, 0, binding.C.byref(n)) == 1
    assert L.mi_unet_group_set_targets(None, None, 0) == 1
    assert not hostlib.set_targets([(1, 0.5)]) and hostlib.get_targets() == [(2, pytest.approx(0.06))]      # no engine: refused
