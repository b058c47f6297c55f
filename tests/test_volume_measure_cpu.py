"""The volume measurement (include/mi_unet.h: mi_unet_volume_measure) without a device: mi_unet_volume_measure_host
against the numpy reference of volume_measure_ref.py, which searches all voxels and so tests the run-end argument, field for field;
mi_unet_volume_measure_derive against the same arithmetic in Python with numpy.linalg.eigh; the argument checks, the struct sizes and
the host half as a stand-alone program.  Integer work is compared exactly."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import volume_measure_ref as mm
from miunet import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd")
EPS = float(np.finfo(np.float64).eps)


def test_the_cases_are_not_degenerate():
    mm.assert_not_degenerate()


@pytest.mark.parametrize("name", list(mm.cases()))
def test_host_equals_reference(name):
    mm.assert_equal(mm.call(binding.volume_measure_host, name), mm.case_ref(name), name)


def test_the_cap_acts_on_the_run_ends_and_leaves_the_rest_valid():
    full, under, zero = (mm.call(binding.volume_measure_host, f"sheet_cap{c}")[0] for c in (4608, 4607, 0))
    assert full["ends"] == 4608 and full["d2"] > 0 and full["a_d2"] > 0
    for skipped in (under, zero):
        assert [int(skipped[f]) for f in ("d2", "dp", "dq", "a_d2", "a_p", "a_q")] == [-1] * 6
        for f in mm.FIELDS:
            if f not in ("d2", "dp", "dq", "a_d2", "a_p", "a_q"):
                assert skipped[f] == full[f], f
    got = mm.call(binding.volume_measure_host, "m4096")
    assert (got["ends"] > 300).sum() >= 1 and ((got["d2"] == -1) == (got["ends"] > 300)).all()
    empty = got[got["voxels"] == 0]
    assert empty.size > 3000 and not empty.tobytes().strip(b"\0")              # an id that no voxel carries: all-zero, cap or not


def test_without_intensity_the_four_fields_are_zero_and_ids_outside_1_to_m_belong_to_nothing():
    got = mm.call(binding.volume_measure_host, "no_intensity")
    assert got["voxels"].min() > 0 and not got["imin"].any() and not got["imax"].any() and not got["si"].any() and not got["sii"].any()
    ids, inten, m, units, _ = mm.cases()["scattered"]
    fewer = binding.volume_measure_host(ids, inten, m=m - 2, units=units)        # the last two ids are now "above m"
    assert fewer.tobytes() == mm.call(binding.volume_measure_host, "scattered")[:m - 2].tobytes()


def test_one_voxel_and_a_column_of_single_voxels():
    ids = np.zeros((5, 4, 6), np.int32)
    ids[2, 1, 3] = 1
    ids[:, 3, 5] = 2                                             # one voxel per slice: no two share a z
    t = binding.volume_measure_host(ids, None, m=2, units=(2, 3, 4))
    p = 2 * 24 + 1 * 6 + 3
    assert (t[0]["voxels"], t[0]["ends"], t[0]["d2"], t[0]["dp"], t[0]["dq"], t[0]["a_d2"], t[0]["a_p"], t[0]["a_q"]) == (1, 1, 0, p, p, 0, p, p)
    first = 3 * 6 + 5
    assert (t[1]["voxels"], t[1]["ends"], t[1]["d2"], t[1]["dp"], t[1]["dq"]) == (5, 5, (4 * 4) ** 2, first, first + 4 * 24)
    assert (t[1]["a_d2"], t[1]["a_p"], t[1]["a_q"]) == (0, first, first)
    mm.assert_equal(t, mm.measure(ids, None, 2, (2, 3, 4)))


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def earg_cases():
    """(name, dict of overrides of a good call's arguments); every one must return MI_UNET_EARG"""
    return [("null ids", dict(ids=None)), ("null units", dict(units=None)), ("null table", dict(table=None)),
            ("D = 0", dict(D=0)), ("H = 0", dict(H=0)), ("W = -1", dict(W=-1)), ("W = 8193", dict(W=8193)), ("D = 8193", dict(D=8193)),
            ("2^31 voxels", dict(D=32, H=8192, W=8192)), ("m = 0", dict(m=0)), ("m = 4097", dict(m=4097)),
            ("unit 0", dict(un=[1, 0, 1])), ("unit -3", dict(un=[-3, 1, 1])), ("d2 limit", dict(un=[1, 1, 46341])),
            ("d2 limit by the sum", dict(D=2, H=2, W=2, un=[32768, 32768, 1])), ("max_ends -1", dict(max_ends=-1)),
            ("max_ends 2^20 + 1", dict(max_ends=(1 << 20) + 1))]


def legal_cases():
    """both sides of each limit, and the arguments that may be NULL"""
    return [("null intensity", dict(intensity=None)), ("null opts", dict(opts=None)), ("max_ends 0", dict(max_ends=0)),
            ("max_ends 2^20", dict(max_ends=1 << 20)), ("the largest unit", dict(un=[1, 1, 46340])), ("m = 4096", dict(m=4096, rows=4096))]


def call_with(fn, head, case):
    """a good 2 x 5 x 7 call with the case's overrides, through ctypes, its table poisoned; returns (rc, outputs untouched)"""
    ids = np.ones((2, 5, 7), np.int32)
    ids[0, 2, 3] = 2
    inten = np.full((2, 5, 7), 700, np.uint16)
    un = np.asarray(case.get("un", [1, 2, 3]), np.int32)
    table = np.full((case.get("rows", 3), mm.STRUCT_BYTES), 0x55, np.uint8)
    opts = binding.VMeasureOpts(case.get("max_ends", 100))
    arrays = dict(ids=ids, intensity=inten, units=un, table=table)
    ptr = lambda name: None if name in case and case[name] is None else arrays[name].ctypes.data_as(C.c_void_p)
    before = (ids.copy(), inten.copy())
    rc = fn(*head, ptr("ids"), ptr("intensity"), case.get("D", 2), case.get("H", 5), case.get("W", 7), case.get("m", 2), ptr("units"),
            None if "opts" in case else C.cast(C.byref(opts), C.c_void_p), ptr("table"))
    untouched = (table == 0x55).all() and np.array_equal(ids, before[0]) and np.array_equal(inten, before[1])
    return rc, bool(untouched)


def test_host_argument_errors_leave_outputs_untouched():
    L = binding.lib()
    rc, untouched = call_with(L.mi_unet_volume_measure_host, (), {})
    assert rc == 0 and not untouched                                        # the good call the cases are made from
    for name, case in earg_cases():
        rc, untouched = call_with(L.mi_unet_volume_measure_host, (), case)
        assert rc == 1 and untouched, name
        assert b"mi_unet_volume_measure_host" in L.mi_unet_last_error(), name
    for name, case in legal_cases():
        assert call_with(L.mi_unet_volume_measure_host, (), case)[0] == 0, name


def test_struct_sizes_and_header_strings():
    assert C.sizeof(binding.VMeasure) == binding.VMEASURE_DTYPE.itemsize == mm.STRUCT_BYTES == 128
    assert C.sizeof(binding.VMeasureOpts) == 4 and C.sizeof(binding.VMeasureShape) == 19 * 8
    assert tuple(n for n, _ in binding.VMeasure._fields_) == mm.FIELDS == binding.VMEASURE_DTYPE.names
    assert binding.VMEASURE_MAX_ENDS_LIMIT == mm.MAX_ENDS_LIMIT and binding.VMEASURE_DEFAULT_MAX_ENDS == mm.DEFAULT_MAX_ENDS
    header = open(os.path.join(ROOT, "include", "mi_unet.h")).read()
    assert "Volume measurement (DESIGN.md 7.13)" in header
    assert "#define MI_UNET_VMEASURE_MAX_ENDS_LIMIT 1048576   /* 2^20 */" in header
    assert "typedef struct mi_unet_vmeasure {      /* 128 bytes, no padding */" in header
    assert "typedef struct mi_unet_vmeasure_opts { int max_ends; } mi_unet_vmeasure_opts;     /* default { 262144 } */" in header
    for name in ("mi_unet_volume_measure", "mi_unet_volume_measure_host", "mi_unet_volume_measure_derive"):
        assert hasattr(binding.lib(), name) and name in binding.EXPORTS
    kernels = open(os.path.join(PKG, "csrc", "kernels.h")).read()
    assert f"constexpr int VMS_TILE = {mm.TILE};" in kernels                  # the tile the scattered ids are sized round


# ---- derive ---------------------------------------------------------------------------------------------------------------------------
def derive_rows():
    """(name, the reference's row, units) of every component with voxels in a handful of cases"""
    rows = []
    for name in ("noise(7, 40, 72)c26", "noise(16, 24, 130)c6", "noise(1, 48, 80)c6", "scattered", "sheet(7, 7, 50)", "box", "serpentine"):
        units = mm.cases()[name][3]
        rows += [(f"{name}[{r}]", row, units) for r, row in enumerate(mm.case_ref(name)) if row["voxels"]]
    return rows


def test_derive_equals_the_same_arithmetic_in_python():
    """Both eigen-solvers are backward stable: each returns the exact eigenvalues of a matrix within a few eps * ||C|| of C, so two
    of them differ by at most that much, and by Weyl's inequality so do their eigenvalues.  The bound is 1e-12 lambda_max (4500 eps);
    the largest difference seen is printed (run with -s) and recorded in DESIGN.md 7.13.  An eigenvector is compared where the gap to
    both neighbours exceeds 1e-6 lambda_max: by Davis-Kahan its sine is then at most (the two backward errors) / gap."""
    unit_mm = 0.1
    worst = worst_dir = 0.0
    rows = derive_rows()
    assert len(rows) > 300
    for name, row, units in rows:
        got, want = binding.volume_measure_derive(row, units, unit_mm), mm.derive(row, units, unit_mm)
        top = float(want["lam"][0])
        for k in ("cx_mm", "cy_mm", "cz_mm", "mean", "std", "diameter_mm", "axial_diameter_mm"):
            assert abs(got[k] - want[k]) <= 4 * EPS * max(abs(want[k]), 1.0), (name, k, got[k], want[k])        # the same operations in both
        lam = [a * a / 20.0 for a in got["axis_mm"]]
        assert lam[0] >= lam[1] >= lam[2] > 0.0, name
        for i in range(3):
            worst = max(worst, abs(lam[i] - want["lam"][i]) / top)
            assert abs(lam[i] - want["lam"][i]) <= 1e-12 * top, (name, i, lam, want["lam"])
            v = np.array(got["axis_dir"][i])
            assert abs(float(v @ v) - 1.0) <= 8 * EPS and v[int(np.argmax(np.abs(v)))] > 0.0, (name, i)
            gap = min([abs(want["lam"][i] - want["lam"][j]) for j in range(3) if j != i])
            if gap > 1e-6 * top:
                sine = math.sqrt(max(0.0, 1.0 - float(v @ want["axis_dir"][i]) ** 2))
                worst_dir = max(worst_dir, sine * gap / top)
                assert sine <= 2e-12 * top / gap + 1e-7, (name, i, sine, gap / top)    # (1e-7: sqrt(1 - dot^2) of a dot rounded at 1)
    print(f"derive: largest |dlambda| / lambda_max = {worst:.3e}; largest sine * gap / lambda_max = {worst_dir:.3e}")


def test_derive_of_one_voxel_and_of_skipped_diameters():
    one = binding.VMeasure(voxels=1, ends=1, sx=3, sy=4, sz=5, sxx=9, syy=16, szz=25, sxy=12, sxz=15, syz=20, si=7, sii=49, imin=7, imax=7)
    d = binding.volume_measure_derive(one, (7, 7, 50), 0.1)
    assert (d["cx_mm"], d["cy_mm"], d["cz_mm"]) == pytest.approx((3.5 * 0.7, 4.5 * 0.7, 5.5 * 5.0), rel=1e-15)
    assert d["axis_mm"] == pytest.approx([2 * math.sqrt(5 / 12) * s for s in (5.0, 0.7, 0.7)], rel=1e-14)       # 1.291 spacings, descending
    assert [abs(v) for v in d["axis_dir"][0]] == pytest.approx([0.0, 0.0, 1.0], abs=1e-15)
    assert d["mean"] == 7.0 and d["std"] == 0.0 and d["diameter_mm"] == 0.0 and d["axial_diameter_mm"] == 0.0
    skipped = binding.VMeasure(voxels=2, ends=2, d2=-1, dp=-1, dq=-1, a_d2=-1, a_p=-1, a_q=-1, sx=1, sxx=1)
    d = binding.volume_measure_derive(skipped, (1, 1, 1), 1.0)
    assert math.isnan(d["diameter_mm"]) and math.isnan(d["axial_diameter_mm"]) and d["axis_mm"][0] == pytest.approx(2 * math.sqrt(5 * (0.25 + 1 / 12)))


def test_derive_argument_errors_leave_the_output_untouched():
    L = binding.lib()
    good = binding.VMeasure(voxels=1, ends=1)
    units = (C.c_int * 3)(1, 1, 1)
    out = (C.c_uint8 * (19 * 8))(*([0x55] * (19 * 8)))
    shape = C.cast(out, C.POINTER(binding.VMeasureShape))
    for name, args in (("null entry", (None, units, 1.0, shape)), ("null units", (C.byref(good), None, 1.0, shape)),
                       ("null out", (C.byref(good), units, 1.0, None)), ("no voxels", (C.byref(binding.VMeasure()), units, 1.0, shape)),
                       ("unit 0", (C.byref(good), (C.c_int * 3)(1, 0, 1), 1.0, shape)), ("unit_mm 0", (C.byref(good), units, 0.0, shape)),
                       ("unit_mm inf", (C.byref(good), units, float("inf"), shape)), ("unit_mm nan", (C.byref(good), units, float("nan"), shape))):
        assert L.mi_unet_volume_measure_derive(*args) == 1 and bytes(out) == b"\x55" * (19 * 8), name
        assert b"mi_unet_volume_measure_derive" in L.mi_unet_last_error(), name
    assert L.mi_unet_volume_measure_derive(C.byref(good), units, 1.0, shape) == 0


def test_a_ball_of_radius_12_has_axes_of_24():
    """the full axes of the solid ellipsoid with a ball's moments are its diameter; the digitised ball is within 2 % on all three
    axes, on the reference first"""
    z, y, x = np.indices((29, 29, 29)) - 14
    ids = (x * x + y * y + z * z <= 144).astype(np.int32)
    ref = mm.measure(ids, None, 1, (1, 1, 1))[0]
    assert all(abs(a - 24.0) <= 0.02 * 24.0 for a in mm.derive(ref, (1, 1, 1), 1.0)["axis_mm"])
    got = binding.volume_measure_host(ids, None, m=1, units=(1, 1, 1))
    mm.assert_equal(got, [ref])
    d = binding.volume_measure_derive(got[0], (1, 1, 1), 1.0)
    assert all(abs(a - 24.0) <= 0.02 * 24.0 for a in d["axis_mm"]), d["axis_mm"]
    assert d["diameter_mm"] == pytest.approx(24.0) and d["axial_diameter_mm"] == pytest.approx(24.0)
    stretched = binding.volume_measure_derive(got[0], (2, 3, 5), 0.5)             # the same voxels under an anisotropic spacing
    assert sorted(stretched["axis_mm"]) == pytest.approx(sorted(a * s for a, s in zip(d["axis_mm"], (1.0, 1.5, 2.5))), rel=0.03)


def test_host_half_as_a_stand_alone_program(tmp_path):
    """tests/cpu/volume_measure_host_test.cpp + csrc/volume_measure.cpp without its device entry point, built by a plain C++ compiler:
    the form in which the host half runs under -fsanitize=address,undefined (the command is in the program's header); here it is
    built without"""
    exe = tmp_path / "volume_measure_host_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DMIUNET_NO_DEVICE", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpu", "volume_measure_host_test.cpp"), os.path.join(PKG, "csrc", "volume_measure.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"volume_measure_host_test ok" in r.stdout, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]


# ---- the facade's setting (needs no engine) ---------------------------------------------------------------------------------------------------
def test_cli_volmeasure_command():
    from miunet import hostlib
    cli = os.path.join(os.path.dirname(hostlib.LIB_PATH), "medseg_cli")
    script = ("volmeasure\nvolmeasure on\nvolmeasure on channel 2 ends 100\nvolmeasure\nvolmeasure on ends 5 channel 1\nvolmeasure on ends 0\n"
              "volmeasure off 3\nvolmeasure on ends\nvolmeasure on size 3\nvolmeasure maybe\nvolmeasure on ends 1048577\nvolmeasure on channel -1\n"
              "volmeasure off\nvolume\nvolmesh\nhelp\nexit\n")
    r = subprocess.run([cli], input=script.encode(), capture_output=True, timeout=60)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0
    said = [l.replace("> ", "") for l in out.splitlines() if l.replace("> ", "").startswith("Volume measure:")]
    assert said == ["Volume measure: off channel 0 ends 262144", "Volume measure: on channel 0 ends 262144", "Volume measure: on channel 2 ends 100",
                    "Volume measure: on channel 2 ends 100", "Volume measure: on channel 1 ends 5", "Volume measure: on channel 0 ends 0",
                    "Volume measure: off channel 0 ends 262144"]
    # off with a word, a key without its number, an unknown key, an unknown word; then the two values the setting refuses
    assert err.count("Invalid volmeasure command") == 4 and err.count("Volume measure unchanged") == 2
    assert "volmeasure on [channel N] [ends N]|off" in out
    assert "Volume: off 26 min 0 keep 0 spacing 1 1 1" in out and "Volume mesh: off faces" in out      # the siblings are untouched


def test_volume_measure_setting_round_trips_through_the_c_view():
    from miunet import hostlib
    default = {"on": False, "channel": 0, "max_ends": 262144}
    volume, mesh = hostlib.get_volume(), hostlib.get_volume_mesh()
    assert hostlib.get_volume_measure() == default
    try:
        assert hostlib.set_volume_measure(True, 1, 500)
        want = {"on": True, "channel": 1, "max_ends": 500}
        assert hostlib.get_volume_measure() == want
        for bad in ((True, -1, 500), (True, 0, -1), (True, 0, (1 << 20) + 1)):
            assert not hostlib.set_volume_measure(*bad) and hostlib.get_volume_measure() == want, bad
        assert hostlib.set_volume_measure(True, 0, 1 << 20) and hostlib.set_volume_measure(True, 0, 0)
        assert hostlib.set_volume_measure(True) and hostlib.get_volume_measure() == {"on": True, "channel": 0, "max_ends": 262144}
        assert hostlib.get_volume() == volume and hostlib.get_volume_mesh() == mesh          # a setting of its own
    finally:
        assert hostlib.set_volume_measure(False)
    assert hostlib.get_volume_measure() == default
    for name in ("medseg_set_volume_measure", "medseg_get_volume_measure"):
        assert name in open(os.path.join(ROOT, "include", "medseg_c.h")).read()
