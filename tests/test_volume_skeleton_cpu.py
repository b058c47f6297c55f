"""The volume skeleton (include/mi_unet.h: mi_unet_volume_skeleton) without a device: mi_unet_volume_skeleton_host against
the numpy / scipy reference of volume_skeleton_ref.py, field by field; the topology of every component before and after, counted without
the thinning code; the skeleton as a fixed point; the radius against a brute-force minimum; mi_unet_volume_skeleton_derive against the
same arithmetic in Python; the host form of the simple-point test; the argument checks, the struct sizes and the host half as a
stand-alone program."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import volume_skeleton_ref as vk
from miunet import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd")


def test_the_cases_are_not_degenerate():
    vk.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vk.cases()))
def test_host_equals_reference(name):
    """out_ids, r2 (the reference's is a brute-force minimum over the wrapped volume), every field of the table, passes, deleted, stable"""
    vk.assert_equal(vk.call(binding.volume_skeleton_host, name), vk.case_ref(name), name)


@pytest.mark.parametrize("name", list(vk.cases()))
def test_topology_is_preserved_and_the_skeleton_is_a_subset(name):
    """per component: 26-components, 6-connected cavities and the Euler characteristic, by scipy's labels and the cubical complex"""
    ids, m, _ = vk.cases()[name]
    got = vk.call(binding.volume_skeleton_host, name)
    clean = np.where((ids >= 1) & (ids <= m), ids, 0)
    assert np.all((got["ids"] == 0) | (got["ids"] == clean))
    assert vk.topology_by_id(got["ids"], m) == vk.topology_by_id(clean, m)
    assert [int(v) for v in got["table"]["voxels"]] == [int((got["ids"] == r + 1).sum()) for r in range(m)]


@pytest.mark.parametrize("name", ["ball_r9", "torus", "shell", "y", "noise", "seams", "noise_labelled_6", "absent_ids", "one_slice"])
def test_thinning_a_skeleton_again_changes_nothing(name):
    _, m, kw = vk.cases()[name]
    first = vk.call(binding.volume_skeleton_host, name)
    again = binding.volume_skeleton_host(first["ids"], m, units=kw.get("units", (1, 1, 1)), want_ids=True)
    assert np.array_equal(again["ids"], first["ids"]) and (again["passes"], again["deleted"], again["stable"]) == (1, 0, 1)
    for f in ("voxels", "ends", "isolated", "junctions", "links"):
        assert np.array_equal(again["table"][f], first["table"][f]), f
    assert np.array_equal(again["table"]["voxels_in"], first["table"]["voxels"])


def test_radius_options():
    """radius off: the three fields are zero, everything else is unchanged; r2 is still written when asked for"""
    ids, m, _ = vk.cases()["noise"]
    on = binding.volume_skeleton_host(ids, m, want_r2=True)
    off = binding.volume_skeleton_host(ids, m, radius=False, want_r2=True)
    bare = binding.volume_skeleton_host(ids, m, radius=False, want_ids=False)
    assert off["r2"].tobytes() == on["r2"].tobytes() and off["ids"].tobytes() == on["ids"].tobytes() and bare["ids"] is None and bare["r2"] is None
    for f in ("r2_min", "r2_max", "r2_sum"):
        assert on["table"][f].any() and not off["table"][f].any() and not bare["table"][f].any(), f
    for f in ("voxels_in", "voxels", "ends", "isolated", "junctions", "links"):
        assert np.array_equal(on["table"][f], off["table"][f]) and np.array_equal(on["table"][f], bare["table"][f]), f
    assert (on["r2"] > 0).sum() == (on["ids"] > 0).sum() and not on["r2"][on["ids"] == 0].any()


def test_derive_is_the_same_arithmetic():
    spacing, unit = (0.7, 0.9, 2.5), 0.1
    for name in ("noise", "torus", "aniso_noise", "absent_ids"):
        got = vk.call(binding.volume_skeleton_host, name)
        for r, row in enumerate(vk.case_ref(name)["table"]):
            assert binding.volume_skeleton_derive(got["table"][r], spacing, unit) == vk.derive(row, spacing, unit), (name, r)
    # the polyline lengths: nine x steps of the line; twelve diagonal steps of the ring, which closes once
    line = binding.volume_skeleton_derive(vk.call(binding.volume_skeleton_host, "line")["table"][0], spacing, unit)
    assert line["length_mm"] == 9 * 0.7 and line["loops"] == 0
    ring = binding.volume_skeleton_derive(vk.call(binding.volume_skeleton_host, "ring")["table"][0], spacing, unit)
    assert ring["length_mm"] == 12 * math.sqrt(0.7 * 0.7 + 0.9 * 0.9) and ring["loops"] == 1
    torus = binding.volume_skeleton_derive(vk.call(binding.volume_skeleton_host, "torus")["table"][0], spacing, unit)
    assert torus["loops"] == 1
    rec = vk.call(binding.volume_skeleton_host, "noise")["table"][0]
    for bad in ((0.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, -2.0)):
        with pytest.raises(RuntimeError):
            binding.volume_skeleton_derive(rec, bad, unit)
    for bad in (0.0, float("inf")):
        with pytest.raises(RuntimeError):
            binding.volume_skeleton_derive(rec, spacing, bad)


def test_host_simple_point_test_is_the_definition():
    """the codes the cases meet, the first 2^12, and a spread of words over the whole range"""
    rng = np.random.default_rng(26)
    assert np.array_equal(binding.volume_skeleton_simple_host(0, 128), vk.simple_bits(0, 128))
    for w in [(1 << 21) - 1] + rng.integers(0, 1 << 21, 400).tolist():
        assert np.array_equal(binding.volume_skeleton_simple_host(w, 1), vk.simple_bits(w, 1)), w
    bits = binding.volume_skeleton_simple_host(0, 1 << 16)          # 2^21 codes in one call
    assert 0 < int(np.unpackbits(bits.view(np.uint8)).sum()) < 1 << 21


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------
def earg_cases():
    """(name, dict of overrides of a good call's arguments); every one must return MI_UNET_EARG"""
    return [("null ids", dict(ids=None)), ("null units", dict(units=None)), ("null table", dict(table=None)),
            ("D = 0", dict(D=0)), ("H = 0", dict(H=0)), ("W = -1", dict(W=-1)), ("W = 8193", dict(D=1, H=1, W=8193)),
            ("2^31 voxels", dict(D=32, H=8192, W=8192)), ("m = 0", dict(m=0)), ("m = 4097", dict(m=4097)),
            ("unit 0", dict(un=[1, 0, 1])), ("unit -1", dict(un=[-1, 1, 1])),
            ("a wrapped diagonal of 2^31", dict(D=2, H=5, W=7, un=[1, 1, 15447])), ("max_passes -1", dict(max_passes=-1)),
            ("radius 2", dict(radius=2))]


def legal_cases():
    """both sides of each limit, and the arguments that may be NULL"""
    return [("null opts", dict(opts=None)), ("null out_ids", dict(out_ids=None)), ("null r2", dict(r2=None)), ("null info", dict(info=None)),
            ("m = 4096", dict(m=4096)), ("the largest unit", dict(D=2, H=5, W=7, un=[1, 1, 15446])), ("max_passes 3", dict(max_passes=3)),
            ("radius 0", dict(radius=0)), ("W = 8192", dict(D=1, H=1, W=8192))]


def call_with(fn, head, case):
    """a good 2 x 5 x 7 call with the case's overrides, through ctypes, its outputs poisoned; returns (rc, outputs untouched)"""
    d, h, w = case.get("D", 2), case.get("H", 5), case.get("W", 7)
    voxels = d * h * w if 0 < d * h * w <= 1 << 20 and min(d, h, w) > 0 else 70
    ids = np.ones(voxels, np.int32)
    un = np.asarray(case.get("un", [1, 2, 3]), np.int32)
    m = case.get("m", 2)
    rows = max(min(m, 4096), 1)
    outs = dict(out_ids=np.full(voxels, 0x55555555, np.int32), r2=np.full(voxels, 0x55555555, np.int32),
                table=np.full((rows, vk.SKEL_BYTES), 0x55, np.uint8), info=np.full(vk.INFO_BYTES, 0x55, np.uint8))
    arrays = dict(outs, ids=ids, units=un)
    opts = binding.VSkelOpts(case.get("max_passes", 0), case.get("radius", 1))
    ptr = lambda name: None if name in case and case[name] is None else arrays[name].ctypes.data_as(C.c_void_p)
    rc = fn(*head, ptr("ids"), d, h, w, m, ptr("units"), None if "opts" in case else C.cast(C.byref(opts), C.c_void_p), ptr("out_ids"), ptr("r2"),
            ptr("table"), ptr("info"))
    untouched = all((a.view(np.uint8) == 0x55).all() for a in outs.values()) and (ids == 1).all()
    return rc, bool(untouched)


def test_host_argument_errors_leave_outputs_untouched():
    L = binding.lib()
    rc, untouched = call_with(L.mi_unet_volume_skeleton_host, (), {})
    assert rc == 0 and not untouched                                        # the good call the cases are made from
    for name, case in earg_cases():
        rc, untouched = call_with(L.mi_unet_volume_skeleton_host, (), case)
        assert rc == 1 and untouched, name
        assert L.mi_unet_last_error().startswith(b"mi_unet_volume_skeleton_host:"), name
    for name, case in legal_cases():
        assert call_with(L.mi_unet_volume_skeleton_host, (), case)[0] == 0, name
    bits = np.zeros(1, np.uint32)
    for first, count in ((1 << 21, 1), (0, 0), ((1 << 21) - 1, 2)):
        assert L.mi_unet_volume_skeleton_simple_host(first, count, bits.ctypes.data_as(C.c_void_p)) == 1
        assert L.mi_unet_last_error().startswith(b"mi_unet_volume_skeleton_simple_host:")
    assert L.mi_unet_volume_skeleton_simple_host(0, 1, None) == 1


def test_struct_sizes():
    assert C.sizeof(binding.VSkel) == binding.VSKEL_DTYPE.itemsize == vk.SKEL_BYTES == 112
    assert C.sizeof(binding.VSkelInfo) == vk.INFO_BYTES == 16
    assert C.sizeof(binding.VSkelOpts) == 8 and C.sizeof(binding.VSkelMetrics) == 40
    assert binding.SKELETON_CODE_WORDS * 32 == 1 << 26


def test_host_half_as_a_stand_alone_program(tmp_path):
    """tests/cpu/volume_skeleton_host_test.cpp + csrc/volume_skeleton.cpp without its device entry points, built by a plain C++ compiler
    with -fsanitize=address,undefined and run as a program"""
    exe = tmp_path / "volume_skeleton_host_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DMIUNET_NO_DEVICE", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpu", "volume_skeleton_host_test.cpp"), os.path.join(PKG, "csrc", "volume_skeleton.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"volume_skeleton_host_test ok" in r.stdout, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]


# ---- the facade's setting (needs no engine; the batch itself needs the network: tests/test_gpu_volume_skeleton.py) ---------------------------
def test_cli_volskeleton_command():
    from miunet import hostlib
    cli = os.path.join(os.path.dirname(hostlib.LIB_PATH), "medseg_cli")
    script = ("volskeleton\nvolskeleton on\nvolskeleton on radius off png on passes 3\nvolskeleton\nvolskeleton on passes 0 png off\n"
              "volskeleton off 3\nvolskeleton on radius\nvolskeleton on size 3\nvolskeleton maybe\nvolskeleton on png yes\nvolskeleton on passes x\n"
              "volskeleton on passes -1\nvolskeleton off\nvolume\nvolsplit\nhelp\nexit\n")
    r = subprocess.run([cli], input=script.encode(), capture_output=True, timeout=60)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0
    said = [l.replace("> ", "") for l in out.splitlines() if l.replace("> ", "").startswith("Volume skeleton:")]
    assert said == ["Volume skeleton: off radius on png off passes 0", "Volume skeleton: on radius on png off passes 0",
                    "Volume skeleton: on radius off png on passes 3", "Volume skeleton: on radius off png on passes 3",
                    "Volume skeleton: on radius on png off passes 0", "Volume skeleton: off radius on png off passes 0"]
    # off with a word, a key without its word, an unknown key, an unknown word, a png that is neither on nor off, passes that is no
    # number; then the value the setting refuses
    assert err.count("Invalid volskeleton command") == 6 and err.count("Volume skeleton unchanged") == 1
    assert "volskeleton on [radius off] [png on] [passes N]|off" in out
    assert "Volume: off 26 min 0 keep 0 spacing 1 1 1" in out and "Volume split: off neck 0 mincore 1" in out    # the siblings are untouched


def test_volume_skeleton_setting_round_trips_through_the_c_view():
    from miunet import hostlib
    default = {"on": False, "radius": True, "png": False, "max_passes": 0}
    volume, split = hostlib.get_volume(), hostlib.get_volume_split()
    assert hostlib.get_volume_skeleton() == default
    try:
        assert hostlib.set_volume_skeleton(True, False, True, 5)
        want = {"on": True, "radius": False, "png": True, "max_passes": 5}
        assert hostlib.get_volume_skeleton() == want
        assert not hostlib.set_volume_skeleton(True, True, False, -1) and hostlib.get_volume_skeleton() == want
        assert hostlib.set_volume_skeleton(True) and hostlib.get_volume_skeleton() == dict(default, on=True)
        assert hostlib.get_volume() == volume and hostlib.get_volume_split() == split           # a setting of its own
    finally:
        assert hostlib.set_volume_skeleton(False)
    assert hostlib.get_volume_skeleton() == default
    for name in ("medseg_set_volume_skeleton", "medseg_get_volume_skeleton"):
        assert name in open(os.path.join(ROOT, "include", "medseg_c.h")).read()
