"""Morphology (include/mi_unet.h: mi_unet_set_morph) without a device: the element, the host chain
postprocess_mask(src, cls, frac, morph) against the numpy / scipy reference of morph_ref.py, the reference anchored to the oracle at
the default, the validation rules through the facade (which needs no engine), the REPL command and the new symbols.  Integer / byte
work: every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import morph_ref as mr
import oracle_lib as orc
from miunet import binding, hostlib
from test_targets_cpu import scipy_target_mask

CLI = os.path.join(os.path.dirname(hostlib.LIB_PATH), "medseg_cli")
SHAPES = [("rect", mr.RECT), ("disc", mr.DISC)]
DEFAULT = [("rect", 1, 0)]


def morph_maps(h, w, seed=5):
    """three label maps of classes 0 .. 3 on h x w: blocks of class 2 joined by one-pixel bridges and cut by one-pixel breaks, with
    corners, a structure on every edge and specks; a frame of class 2 around class 3 (touches all four edges); smooth noise"""
    maps = []
    a = np.zeros((h, w), np.uint8)
    a[2:h // 2, 2:w // 3] = 2
    a[h // 4, 2:w // 3] = 0                                 # a one-pixel break: a close bridges it
    a[h // 2 - 2, w // 3:w // 3 + 6] = 2                     # a one-pixel bridge to the next block: an open cuts it
    a[h // 4:h - 3, w // 3 + 6:2 * w // 3] = 2
    a[h // 2:h // 2 + 3, w // 3 + 9:w // 3 + 12] = 1        # a hole of class 1
    a[0:h // 3, w - w // 5:w] = 2                            # touches the top and right edges
    a[h - h // 4:h, 0:w // 4] = 2                            # touches the bottom and left edges
    a[h - 2, w - 2] = 2                                      # speck
    a[1, w // 2] = 3
    maps.append(a)
    b = np.full((h, w), 2, np.uint8)
    b[3:h - 3, 3:w - 3] = 3
    b[h // 2, :] = 2                                         # a one-pixel bar across the image
    b[:, w // 2 - 1:w // 2 + 1] = 2
    b[h // 3, w // 3] = 2
    maps.append(b)
    rng = np.random.default_rng(seed)
    f = rng.random((h, w))
    for _ in range(3):
        f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5
    c = np.digitize(f, np.quantile(f, [0.35, 0.55, 0.8])).astype(np.uint8)
    c[rng.random((h, w)) < 0.04] = 0
    maps.append(c)
    return np.stack(maps)


@pytest.mark.parametrize("name,shape", SHAPES)
def test_element_equals_the_definition(name, shape):
    for r in range(0, mr.MAX_R + 1):
        got = binding.morph_element(name, r)
        assert got.shape == (2 * r + 1, 2 * r + 1) and set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), mr.element(shape, r)), (name, r)
    assert np.array_equal(binding.morph_element("disc", 1), [[0, 1, 0], [1, 1, 1], [0, 1, 0]])      # the plus
    assert np.array_equal(binding.morph_element("rect", 1), np.ones((3, 3)))
    assert np.array_equal(binding.morph_element("disc", 0), [[1]]) and np.array_equal(binding.morph_element("rect", 0), [[1]])
    L = binding.lib()
    buf = np.zeros(65 * 65, np.uint8)
    for bad in ((2, 1), (-1, 1), (0, -1), (1, mr.MAX_R + 1)):
        assert L.mi_unet_morph_element(bad[0], bad[1], buf.ctypes.data) == 1, bad
    assert L.mi_unet_morph_element(0, 1, None) == 1


def test_the_scipy_steps_equal_the_plain_loop_over_the_element():
    """the reference's own anchor: scipy with border_value 1 / 0 is the definition, for both shapes and windows clipped on every side"""
    rng = np.random.default_rng(3)
    for h, w, density in ((9, 13, 0.3), (8, 8, 0.7), (5, 17, 0.9)):
        a = rng.random((h, w)) < density
        for shape in (mr.RECT, mr.DISC):
            for r in (0, 1, 2, 3, 7):
                assert np.array_equal(mr.erode(a, shape, r), mr.brute_step(a, shape, r, False)), (h, w, shape, r)
                assert np.array_equal(mr.dilate(a, shape, r), mr.brute_step(a, shape, r, True)), (h, w, shape, r)


def test_default_chain_is_anchored_to_the_oracle_on_the_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, "imgproc.npz"))
    for i in range(4):
        m = g[f"mask{i}"]
        want = orc.postprocess_mask(m)
        assert np.array_equal(mr.chain(m, 2, 0.06, mr.RECT, 1, 0), want), i                       # the reference at the default is the oracle
        assert np.array_equal(want, g[f"final{i}"])
        assert np.array_equal(hostlib.postprocess_mask_morph(m, 2, 0.06, "rect", 1, 0), want), i   # ... and so is the host chain
        assert np.array_equal(hostlib.postprocess_mask(m), want) and np.array_equal(hostlib.postprocess_mask_target(m, 2, 0.06), want)
    for cls in (1, 2, 3):
        for i, m in enumerate(morph_maps(33, 65)):
            assert np.array_equal(mr.chain(m, cls, 0.01), scipy_target_mask(m, cls, 0.01)), (cls, i)


@pytest.mark.parametrize("name,shape", SHAPES)
def test_host_chain_equals_the_reference(name, shape):
    changed = 0
    for h, w in ((33, 65), (64, 64)):
        maps = morph_maps(h, w)
        for open_r in (0, 1, 2, 5):
            for close_r in (0, 1, 3):
                for i, m in enumerate(maps):
                    for cls, frac in ((2, 0.01), (3, 0.0)):
                        got = hostlib.postprocess_mask_morph(m, cls, frac, name, open_r, close_r)
                        want = mr.chain(m, cls, frac, shape, open_r, close_r)
                        assert np.array_equal(got, want), (h, w, open_r, close_r, i, cls)
                        assert set(np.unique(got)) <= {0, cls}
                        changed += not np.array_equal(want, mr.chain(m, cls, frac))
    assert changed > 20                                      # the setting matters on these maps


@pytest.mark.parametrize("name,shape", SHAPES)
def test_host_chain_with_the_window_clipped_on_every_side(name, shape):
    rng = np.random.default_rng(11)
    maps = [np.where(rng.random((8, 8)) < d, 2, 0).astype(np.uint8) for d in (0.2, 0.6, 0.95)]
    full = np.full((8, 8), 2, np.uint8)
    one = np.zeros((8, 8), np.uint8)
    one[3, 4] = 2
    for m in maps + [full, one]:
        for open_r, close_r in ((7, 0), (0, 7), (7, 7), (3, 7)):
            got = hostlib.postprocess_mask_morph(m, 2, 0.0, name, open_r, close_r)
            assert np.array_equal(got, mr.chain(m, 2, 0.0, shape, open_r, close_r)), (open_r, close_r)
    assert (hostlib.postprocess_mask_morph(full, 2, 0.0, name, 7, 7) == 2).all()                   # the border never constrains
    assert not hostlib.postprocess_mask_morph(np.zeros((8, 8), np.uint8), 2, 0.0, name, 0, 7).any()  # ... and never seeds


def test_a_close_bridges_a_break_and_a_disc_rounds_a_corner():
    m = np.zeros((40, 40), np.uint8)
    m[5:35, 5:19] = 2
    m[5:35, 20:35] = 2                                       # two blocks of 420 and 450 pixels, one column apart
    apart = hostlib.postprocess_mask_morph(m, 2, 0.3, "rect", 1, 0)                                 # min_area 480: both fall
    joined = hostlib.postprocess_mask_morph(m, 2, 0.3, "rect", 1, 1)
    assert not apart.any() and (joined[5:35, 5:35] == 2).all()
    box = hostlib.postprocess_mask_morph(m, 2, 0.0, "rect", 4, 1)
    disc = hostlib.postprocess_mask_morph(m, 2, 0.0, "disc", 4, 1)
    assert box[5, 5] == 2 and disc[5, 5] == 0 and disc[5, 9] == 2


def test_facade_validation_leaves_the_setting_unchanged():
    assert hostlib.get_morphology() == DEFAULT
    try:
        good = [("disc", 2, 1), ("rect", 0, 31)]
        assert hostlib.set_morphology(good) and hostlib.get_morphology() == good
        bad_lists = [[(2, 1, 0)], [(-1, 1, 0)], [("rect", -1, 0)], [("rect", 32, 0)], [("disc", 1, -1)], [("disc", 1, 32)],
                     [("rect", 1, 0), ("disc", 40, 0)], [("rect", 1, 0)] * 6]
        for bad in bad_lists:
            assert not hostlib.set_morphology(bad), bad
            assert hostlib.get_morphology() == good, bad
        zero = (binding.C.c_int * 1)(0)
        assert hostlib.lib().medseg_set_morphology(zero, zero, zero, -1) == 1 and hostlib.get_morphology() == good
        assert hostlib.set_morphology([("rect", 31, 31)] * 5) and len(hostlib.get_morphology()) == 5
        assert hostlib.set_morphology([]) and hostlib.get_morphology() == DEFAULT                   # the empty list restores the default
    finally:
        assert hostlib.set_morphology([])
    with pytest.raises(RuntimeError):
        hostlib.postprocess_mask_morph(np.zeros((8, 8), np.uint8), 2, 0.0, 2, 1, 0)
    with pytest.raises(RuntimeError):
        hostlib.postprocess_mask_morph(np.zeros((8, 8), np.uint8), 2, 0.0, "rect", 32, 0)


NEW_SYMBOLS = ["mi_unet_set_morph", "mi_unet_get_morph", "mi_unet_morph_element", "mi_unet_group_set_morph"]


def test_new_symbols_are_exported_and_bound_without_a_device():
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported and set(NEW_SYMBOLS) <= set(binding.EXPORTS)
    L = binding.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", hostlib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    host = {line.split()[-1] for line in out.splitlines() if line.strip()}
    mine = {"medseg_postprocess_mask_morph", "medseg_set_morphology", "medseg_get_morphology"}
    assert mine <= host and mine <= set(hostlib.EXPORTS)
    assert [f[0] for f in binding.Morph._fields_] == ["shape", "open_r", "close_r"]
    assert (binding.MORPH_SHAPES, binding.MORPH_MAX_R, binding.DEFAULT_MORPH) == ({"rect": 0, "disc": 1}, 31, DEFAULT)
    # null handles are refused, not dereferenced
    n = binding.C.c_int()
    assert L.mi_unet_set_morph(None, None, 0) == 1 and L.mi_unet_get_morph(None, None, 0, binding.C.byref(n)) == 1
    assert L.mi_unet_group_set_morph(None, None, 0) == 1


def test_cli_morph_command():
    script = "morph\nmorph disc 2 1\nmorph\nmorph rect 4\nmorph rect 40\nmorph blob 1\nmorph disc\nmorph disc 1 x\nmorph default\nhelp\nexit\n"
    r = subprocess.run([CLI], input=script.encode(), capture_output=True, timeout=60)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0
    said = [l.replace("> ", "") for l in out.splitlines() if "Morphology:" in l]
    assert said == ["Morphology: rect 1 0", "Morphology: disc 2 1", "Morphology: disc 2 1", "Morphology: rect 4 0", "Morphology: rect 1 0"]
    assert err.count("Morphology unchanged") == 1 and err.count("Invalid morph command") == 3
    assert "morph rect|disc <open_r> [close_r]|default" in out
