"""The volume zones (include/mi_unet.h: mi_unet_volume_zones) without a device: mi_unet_volume_zones_host against the
numpy reference of volume_zones_ref.py, byte for byte; the two feature functions against the same features in Python; a 4 x 4 image
worked by hand; the argument checks, the struct sizes, the host half as a stand-alone program under the sanitizers and the facade's
setting.  Integer work is compared exactly."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import volume_zones_ref as vz
from miunet import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd")


def test_the_cases_are_not_degenerate():
    vz.assert_not_degenerate()


@pytest.mark.parametrize("name", list(vz.cases()))
def test_host_equals_reference(name):
    got = vz.call(binding.volume_zones_host, name)
    vz.assert_equal(got, vz.case_ref(name), name)
    table, rlm, axial, zones, found = got
    if rlm is not None:
        assert np.array_equal(rlm.sum(axis=(1, 2), dtype=np.int64), table["runs"])
        assert np.array_equal(rlm[:, :, -1].sum(axis=1, dtype=np.int64) >= table["clamped"], np.ones(len(table), bool))
    if axial is not None:
        assert np.array_equal(axial.sum(axis=(1, 2), dtype=np.int64), table["runs_axial"])
    if zones is not None:
        assert int(table["zones"].sum()) == found
        if found <= len(zones):                                 # the whole list: its sizes are the components' voxels
            sizes = np.bincount(zones["component"][:found], zones["size"][:found], minlength=len(table)).astype(np.int64)
            assert np.array_equal(sizes, table["voxels"])
    ids, inten, m, kw = vz.cases()[name]
    texture = binding.volume_texture_host(ids, inten, m, 2, want=())[0]      # (two levels: the three fields do not depend on them, and any m is admitted)
    for f in ("voxels", "imin", "imax"):
        assert np.array_equal(table[f], texture[f]), (name, f)


def test_a_4_x_4_image_worked_by_hand():
    """GLRLM over the four in-plane offsets and GLSZM of

        0 0 1 1
        0 0 1 2
        3 1 2 2
        3 3 2 2

    written out (volume_zones_ref.py says how each number comes about)."""
    glrlm = [[4, 6, 0, 0],      # level 0: four runs of 1, six of 2
             [9, 2, 1, 0],      # level 1: the anti-diagonal of three 1s is its one run of 3
             [5, 6, 1, 0],      # level 2: the last column holds its run of 3
             [6, 3, 0, 0]]      # level 3
    glszm = {(0, 4): 1, (1, 4): 1, (2, 5): 1, (3, 3): 1}        # (level, size) -> zones
    table, rlm, axial, zones, found = vz.call(binding.volume_zones_host, "hand_4x4")
    assert axial[0].tolist() == glrlm and found == 4
    seen = {}
    for z in zones[:found]:
        seen[(int(z["level"]), int(z["size"]))] = seen.get((int(z["level"]), int(z["size"])), 0) + 1
    assert seen == glszm and zones["first"][:4].tolist() == [0, 2, 7, 8]
    assert (int(table[0]["runs_axial"]), int(table[0]["longest_run"]), int(table[0]["zones"]), int(table[0]["largest_zone"])) == (43, 3, 4, 5)
    f = binding.volume_zones_run_features(table[0], axial[0], 4)
    assert f["percentage"] == 43 / 64 and f["short_emphasis"] == pytest.approx((24 + 17 / 4 + 2 / 9) / 43, rel=1e-15)
    g = binding.volume_zones_zone_features(table[0], zones[:found], 0, 4)         # (the all-zero records behind the list are not zones)
    assert (g["percentage"], g["entropy"], g["grey_variance"], g["size_variance"], g["size_nonuniformity"]) == (0.25, 2.0, 1.25, 0.5, 1.5)


def test_null_options_are_the_default_and_fewer_components_are_a_prefix():
    ids, inten, m, _ = vz.cases()["scattered"]
    L = binding.lib()
    table = np.zeros(m, binding.VZONES_DTYPE)
    rlm, axial = np.zeros((m, 32, 32), np.uint32), np.zeros((m, 32, 32), np.uint32)
    zones = np.zeros(ids.size, binding.VZONE_DTYPE)
    found = C.c_int(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mi_unet_volume_zones_host(ptr(ids), ptr(inten), *ids.shape, m, None, ptr(table), ptr(rlm), ptr(axial), ptr(zones), ids.size, C.byref(found)) == 0
    want = binding.volume_zones_host(ids, inten, m, 32, "count", 0, 1, 32)
    assert vz.same_bytes((table, rlm, axial, zones, found.value), want)
    fewer = binding.volume_zones_host(ids, inten, m - 2)           # the last two ids are now "above m"
    assert vz.same_bytes(fewer[:3], tuple(a[:m - 2] for a in want[:3]))
    kept = want[3][:want[4]]
    kept = kept[kept["component"] < m - 2]
    assert fewer[4] == len(kept) and fewer[3][:fewer[4]].tobytes() == kept.tobytes()


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def earg_cases():
    """(name, dict of overrides of a good call's arguments); every one must return MI_UNET_EARG"""
    return [("null ids", dict(ids=None)), ("null intensity", dict(intensity=None)), ("null table", dict(table=None)),
            ("zones without found", dict(found=None)), ("found without zones", dict(zones=None)),
            ("D = 0", dict(D=0)), ("H = 0", dict(H=0)), ("W = 0", dict(W=0)), ("D = -1", dict(D=-1)), ("H = -1", dict(H=-1)), ("W = -1", dict(W=-1)),
            ("D = 8193", dict(D=8193)), ("H = 8193", dict(H=8193)), ("W = 8193", dict(W=8193)),
            # (2^28 + 4 = 6452 * 785 * 53 is the smallest product above 2^28 of three factors below 8193)
            ("2^28 + 4 voxels", dict(D=6452, H=785, W=53)), ("2^28 + 4 voxels, W the largest", dict(D=53, H=785, W=6452)),
            ("m = 0", dict(m=0)), ("m = 4097", dict(m=4097)), ("L = 1", dict(levels=1)), ("L = 65", dict(levels=65)),
            ("R = 1", dict(max_run=1)), ("R = 8193", dict(max_run=8193)), ("m = 4096 at 32 x 33", dict(m=4096, levels=32, max_run=33)),
            ("m = 9 at 64 x 8192", dict(m=9, levels=64, max_run=8192)), ("m = 4096 at 33 levels", dict(m=4096, levels=33, max_run=32)),
            ("width 0", dict(width=0)), ("width 65537", dict(width=65537)), ("lo -1", dict(lo=-1)), ("lo 65536", dict(lo=65536)),
            ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("cap 0", dict(cap=0)), ("cap -1", dict(cap=-1)), ("cap 2^24 + 1", dict(cap=(1 << 24) + 1))]


def legal_cases():
    """the other side of each limit, and the arguments that may be NULL.  (A volume of exactly 2^28 voxels is not called: its two stacks
    are 1.5 GiB.  cap = 2^24 is called with a list of that length only in name: a 2 x 5 x 7 volume writes and clears all of it, 256 MiB,
    so the largest cap called is 2^20.)"""
    return [("D = 8192", dict(D=8192, H=1, W=1)), ("H = 8192", dict(D=1, H=8192, W=1)), ("W = 8192", dict(D=1, H=1, W=8192)),
            ("D = H = W = 1", dict(D=1, H=1, W=1)), ("null opts", dict(opts=None)), ("null rlm", dict(rlm=None)), ("null axial", dict(axial=None)),
            ("no zone half", dict(zones=None, found=None)), ("entry only", dict(rlm=None, axial=None, zones=None, found=None)),
            ("L = 2", dict(levels=2)), ("L = 64", dict(levels=64)), ("R = 2", dict(max_run=2)), ("R = 8192", dict(max_run=8192)),
            ("m = 4096 at 32 x 32", dict(m=4096, levels=32, max_run=32)), ("m = 8 at 64 x 8192", dict(m=8, levels=64, max_run=8192)),
            ("m = 4096 at 64 x 16", dict(m=4096, levels=64, max_run=16)), ("m = 1025 at 64 x 2", dict(m=1025, levels=64, max_run=2)),
            ("width 1", dict(width=1, mode=1)), ("width 65536", dict(width=65536, mode=1)), ("lo 0", dict(lo=0, mode=1)),
            ("lo 65535", dict(lo=65535, mode=1)), ("mode width", dict(mode=1)), ("cap 1", dict(cap=1)), ("cap 2^20", dict(cap=1 << 20))]


def call_with(fn, head, case):
    """a good 2 x 5 x 7 call with the case's overrides, through ctypes, its outputs poisoned; returns (rc, outputs untouched).  The stacks
    have the case's shape where that is a legal one of at most 2^20 voxels (a refused shape is never read)"""
    shape = (case.get("D", 2), case.get("H", 5), case.get("W", 7))
    if not (all(1 <= v <= 8192 for v in shape) and shape[0] * shape[1] * shape[2] <= 1 << 20):
        shape = (2, 5, 7)
    ids = np.ones(shape, np.int32)
    ids.reshape(-1)[ids.size // 2] = 2
    inten = (np.arange(ids.size, dtype=np.int64) * 900 % 65536).astype(np.uint16).reshape(shape)
    m = case.get("m", 2)
    lv, rn = (32, 32) if "opts" in case else (case.get("levels", 8), case.get("max_run", 8))       # (null options: the default)
    rows, cols, runs = (m, lv, rn) if 1 <= m <= 4096 and 2 <= lv <= 64 and 2 <= rn <= 8192 and m * lv * rn <= vz.MAX_CELLS else (2, 8, 8)
    cap = case.get("cap", 40)
    arrays = dict(ids=ids, intensity=inten, table=np.full((rows, vz.STRUCT_BYTES), 0x55, np.uint8), rlm=np.full((rows, cols, runs), 0x55555555, np.uint32),
                  axial=np.full((rows, cols, runs), 0x55555555, np.uint32), zones=np.full((cap if 1 <= cap <= 1 << 20 else 40, 4), 0x55555555, np.uint32))
    opts = binding.VZonesOpts(case.get("mode", 0), lv, case.get("lo", 100), case.get("width", 300), rn)
    found = C.c_int(0x55555555)
    ptr = lambda name: None if name in case and case[name] is None else arrays[name].ctypes.data_as(C.c_void_p)
    before = (ids.copy(), inten.copy())
    rc = fn(*head, ptr("ids"), ptr("intensity"), case.get("D", 2), case.get("H", 5), case.get("W", 7), m,
            None if "opts" in case else C.cast(C.byref(opts), C.c_void_p), ptr("table"), ptr("rlm"), ptr("axial"), ptr("zones"), cap,
            None if "found" in case and case["found"] is None else C.cast(C.byref(found), C.c_void_p))
    untouched = all((arrays[k] == (0x55 if k == "table" else 0x55555555)).all() for k in ("table", "rlm", "axial", "zones")) and found.value == 0x55555555
    return rc, bool(untouched and np.array_equal(ids, before[0]) and np.array_equal(inten, before[1]))


def test_host_argument_errors_leave_outputs_untouched():
    L = binding.lib()
    rc, untouched = call_with(L.mi_unet_volume_zones_host, (), {})
    assert rc == 0 and not untouched                                        # the good call the cases are made from
    for name, case in earg_cases():
        rc, untouched = call_with(L.mi_unet_volume_zones_host, (), case)
        assert rc == 1 and untouched, name
        assert L.mi_unet_last_error().startswith(b"mi_unet_volume_zones_host:"), name
    for name, case in legal_cases():
        assert call_with(L.mi_unet_volume_zones_host, (), case)[0] == 0, name


def test_struct_sizes_and_header_strings():
    assert C.sizeof(binding.VZones) == binding.VZONES_DTYPE.itemsize == vz.STRUCT_BYTES == 56
    assert C.sizeof(binding.VZone) == binding.VZONE_DTYPE.itemsize == vz.ZONE_BYTES == 16
    assert C.sizeof(binding.VZoneFeatures) == vz.FEATURE_BYTES == 128 and C.sizeof(binding.VZonesOpts) == 20
    assert tuple(n for n, _ in binding.VZones._fields_) == vz.FIELDS == binding.VZONES_DTYPE.names
    assert tuple(n for n, _ in binding.VZone._fields_) == vz.ZONE_FIELDS == binding.VZONE_DTYPE.names
    assert tuple(n for n, _ in binding.VZoneFeatures._fields_) == vz.FEATURES
    assert binding.VZONES_MAX_RUN == vz.MAX_RUN and binding.VZONES_MAX_CAP == vz.MAX_CAP
    header = open(os.path.join(ROOT, "include", "mi_unet.h")).read()
    assert "Volume zones (DESIGN.md 7.17)" in header and "#define MI_UNET_VZONES_MAX_RUN 8192" in header
    assert "typedef struct mi_unet_vzones {        /* 56 bytes, no padding */" in header
    for name in ("mi_unet_volume_zones", "mi_unet_volume_zones_host", "mi_unet_volume_zones_run_features", "mi_unet_volume_zones_zone_features"):
        assert hasattr(binding.lib(), name) and name in binding.EXPORTS


# ---- features ---------------------------------------------------------------------------------------------------------------------------
def feature_rows():
    """(name, the reference's row, the cells of one of its matrices, directions, how to ask the product) of every component with voxels
    in a handful of cases"""
    rows = []
    for name in ("hand_4x4", "noise(7, 40, 72)_smooth_L64_count", "noise(5, 33, 130)_noisy_L32_count", "noise(16, 24, 130)_noisy_L8_width", "constant_slab",
                 "diagonals", "checkerboard_levels", "two_blobs_one_id", "scattered", "run8192_W_R8192", "no_rlm", "no_zones"):
        table, rlm, axial, zl, found, cap = vz.case_ref(name)
        L = vz.cases()[name][3].get("levels", 32)
        zarr = None if zl is None else np.array(zl, np.int32).reshape(-1, 4).view(binding.VZONE_DTYPE).reshape(-1)
        for r, row in enumerate(table):
            if not row["voxels"]:
                continue
            for which, tab, directions in (("rlm", rlm, 13), ("axial", axial, 4)):
                if tab is not None:
                    rows.append((f"{name}[{r}].{which}", row, vz.run_cells(tab[r]), directions, lambda e, t=tab[r], d=directions: binding.volume_zones_run_features(e, t, d)))
            if zl is not None:
                rows.append((f"{name}[{r}].zones", row, vz.zone_cells(zl, r), 1, lambda e, z=zarr, r=r, L=L: binding.volume_zones_zone_features(e, z, r, L)))
    return rows


def test_features_equal_the_same_features_in_python():
    """The product sums in double in a fixed order, the reference with math.fsum (exactly rounded sums); both take mu_i and mu_j from
    exact integer sums.  Every feature is a sum of non-negative terms (the entropy of non-positive ones), each rounded a few times, so it
    is within (number of cells) * a few eps of its exact value, relatively: the 1e-12 of test_volume_texture_cpu.py's derive test holds up
    to some thousand cells, and the largest matrix here has fewer than 2000.  The largest deviation seen is printed (run with -s) and
    recorded in DESIGN.md 7.17."""
    rows = feature_rows()
    assert len(rows) > 150 and max(len(cells) for _, _, cells, _, _ in rows) < 2000
    worst, nans = {}, 0
    for name, row, cells, directions, ask in rows:
        got, want = ask(binding.VZones(**row)), vz.features(cells, row["voxels"], directions)
        for k in vz.FEATURES:
            a, b = got[k], want[k]
            if math.isnan(b):
                nans += 1
                assert math.isnan(a), (name, k, a)
                continue
            assert abs(a - b) <= 1e-12 * abs(b), (name, k, a, b)
            if b:
                worst[k] = max(worst.get(k, 0.0), abs(a - b) / abs(b))
    print("features: largest relative deviation: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_features_of_known_matrices():
    nan16 = binding.volume_zones_run_features(binding.VZones(voxels=5), np.zeros((4, 8), np.uint32), 13)
    assert all(math.isnan(v) for v in nan16.values()) and len(nan16) == 16
    # one cell: seven runs of length 2 at level 3 (i = 3)
    g = np.zeros((4, 8), np.uint32)
    g[2, 1] = 7
    f = binding.volume_zones_run_features(binding.VZones(voxels=14), g, 4)
    assert (f["short_emphasis"], f["long_emphasis"], f["high_grey_emphasis"], f["short_high"], f["long_high"]) == (0.25, 4.0, 9.0, 9 / 4, 36.0)
    # (a sum of 7 / 9 over N = 7 is not the double nearest to 1 / 9)
    assert (f["low_grey_emphasis"], f["short_low"], f["long_low"]) == pytest.approx((1 / 9, 1 / 36, 4 / 9), rel=1e-15)
    assert (f["grey_nonuniformity"], f["grey_nonuniformity_norm"], f["size_nonuniformity"], f["size_nonuniformity_norm"]) == (7.0, 1.0, 7.0, 1.0)
    assert (f["percentage"], f["grey_variance"], f["size_variance"], f["entropy"]) == (7 / 56, 0.0, 0.0, 0.0)
    # zones: two of size 1 at level 0 and one of size 3 at level 1, in any order, among records of another component
    z = np.array([(9, 0, 1, 3), (4, 1, 0, 50), (0, 0, 0, 1), (5, 0, 0, 1)], binding.VZONE_DTYPE)
    f = binding.volume_zones_zone_features(binding.VZones(voxels=5), z, 0, 2)
    assert f["percentage"] == 3 / 5 and f["size_nonuniformity"] == 5 / 3 and f["grey_nonuniformity"] == 5 / 3
    assert f["entropy"] == pytest.approx(-(2 / 3 * math.log2(2 / 3) + 1 / 3 * math.log2(1 / 3)), rel=1e-15)
    assert f["size_variance"] == pytest.approx(8 / 9, rel=1e-15) and f["grey_variance"] == pytest.approx(2 / 9, rel=1e-15)
    assert binding.volume_zones_zone_features(binding.VZones(voxels=5), z[1:2], 1, 2)["long_emphasis"] == 2500.0       # a slice of the list


def test_feature_argument_errors_leave_the_output_untouched():
    L = binding.lib()
    good = binding.VZones(voxels=1)
    row = (C.c_uint32 * (64 * 8192))(1)
    zone = binding.VZone(0, 0, 0, 1)
    out = (C.c_uint8 * 128)(*([0x55] * 128))
    feat = C.cast(out, C.POINTER(binding.VZoneFeatures))
    run = L.mi_unet_volume_zones_run_features
    for name, args in (("null entry", (None, row, 4, 4, 13, feat)), ("null row", (C.byref(good), None, 4, 4, 13, feat)), ("null out", (C.byref(good), row, 4, 4, 13, None)),
                       ("no voxels", (C.byref(binding.VZones()), row, 4, 4, 13, feat)), ("L = 1", (C.byref(good), row, 1, 4, 13, feat)),
                       ("L = 65", (C.byref(good), row, 65, 4, 13, feat)), ("R = 1", (C.byref(good), row, 4, 1, 13, feat)),
                       ("R = 8193", (C.byref(good), row, 4, 8193, 13, feat)), ("12 directions", (C.byref(good), row, 4, 4, 12, feat)),
                       ("1 direction", (C.byref(good), row, 4, 4, 1, feat))):
        assert run(*args) == 1 and bytes(out) == b"\x55" * 128, name
        assert L.mi_unet_last_error().startswith(b"mi_unet_volume_zones_run_features:"), name
    for args in ((C.byref(good), row, 2, 2, 13, feat), (C.byref(good), row, 64, 8192, 4, feat)):
        assert run(*args) == 0
    out[:] = [0x55] * 128
    zf = L.mi_unet_volume_zones_zone_features
    for name, args in (("null entry", (None, C.byref(zone), 1, 0, 4, feat)), ("null list", (C.byref(good), None, 1, 0, 4, feat)),
                       ("null out", (C.byref(good), C.byref(zone), 1, 0, 4, None)), ("nz = -1", (C.byref(good), C.byref(zone), -1, 0, 4, feat)),
                       ("no voxels", (C.byref(binding.VZones()), C.byref(zone), 1, 0, 4, feat)), ("L = 1", (C.byref(good), C.byref(zone), 1, 0, 1, feat)),
                       ("L = 65", (C.byref(good), C.byref(zone), 1, 0, 65, feat)),
                       ("level = L", (C.byref(good), C.byref(binding.VZone(0, 0, 4, 1)), 1, 0, 4, feat)),
                       ("level -1", (C.byref(good), C.byref(binding.VZone(0, 0, -1, 1)), 1, 0, 4, feat)),
                       ("size 0", (C.byref(good), C.byref(binding.VZone(0, 0, 0, 0)), 1, 0, 4, feat))):
        assert zf(*args) == 1 and bytes(out) == b"\x55" * 128, name
        assert L.mi_unet_last_error().startswith(b"mi_unet_volume_zones_zone_features:"), name
    assert zf(C.byref(good), C.byref(binding.VZone(0, 0, 3, 1)), 1, 0, 4, feat) == 0 and zf(C.byref(good), None, 0, 0, 2, feat) == 0
    assert zf(C.byref(good), C.byref(binding.VZone(0, 7, 99, 0)), 1, 0, 64, feat) == 0       # a record of another component is not judged


def test_host_half_as_a_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/cpu/volume_zones_host_test.cpp + csrc/volume_zones.cpp without its device entry point, built by g++ with
    -fsanitize=address,undefined and run: a stand-alone program with the sanitizers' runtimes linked in needs nothing preloaded"""
    exe = tmp_path / "volume_zones_host_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DMIUNET_NO_DEVICE", "-o", str(exe), os.path.join(ROOT, "tests", "cpu", "volume_zones_host_test.cpp"),
                           os.path.join(PKG, "csrc", "volume_zones.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"volume_zones_host_test ok" in r.stdout, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]


# ---- the facade's setting (needs no engine) ---------------------------------------------------------------------------------------------------
def test_cli_volzones_command():
    from miunet import hostlib
    cli = os.path.join(os.path.dirname(hostlib.LIB_PATH), "medseg_cli")
    script = ("volzones\nvolzones on\nvolzones on levels 64 width 25 lo 1000 run 128 channel 2\nvolzones\nvolzones on channel 1 count levels 8\n"
              "volzones on width 300 run 2\nvolzones off\n"
              # off with a word, a key without its number, an unknown key, an unknown word, lo without width, count and width, width twice
              "volzones off 3\nvolzones on levels\nvolzones on size 3\nvolzones maybe\nvolzones on lo 5\nvolzones on count width 3\n"
              "volzones on width 3 width 4\n"
              # the values the setting refuses
              "volzones on levels 1\nvolzones on levels 65\nvolzones on width 0\nvolzones on width 65537\nvolzones on width 2 lo 65536\n"
              "volzones on channel -1\nvolzones on run 1\nvolzones on run 8193\nvolzones\nvolume\nvoltexture\nhelp\nexit\n")
    r = subprocess.run([cli], input=script.encode(), capture_output=True, timeout=60)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0
    said = [l.replace("> ", "") for l in out.splitlines() if l.replace("> ", "").startswith("Volume zones:")]
    assert said == ["Volume zones: off channel 0 levels 32 count run 32", "Volume zones: on channel 0 levels 32 count run 32",
                    "Volume zones: on channel 2 levels 64 width 25 lo 1000 run 128", "Volume zones: on channel 2 levels 64 width 25 lo 1000 run 128",
                    "Volume zones: on channel 1 levels 8 count run 32", "Volume zones: on channel 0 levels 32 width 300 lo 0 run 2",
                    "Volume zones: off channel 0 levels 32 count run 32", "Volume zones: off channel 0 levels 32 count run 32"]
    assert err.count("Invalid volzones command") == 7 and err.count("Volume zones unchanged") == 8
    assert "volzones on [levels N] [count|width W [lo L]] [run N] [channel N]|off" in out
    assert "Volume: off 26 min 0 keep 0 spacing 1 1 1" in out and "Volume texture: off channel 0 levels 32 count" in out     # the siblings are untouched


def test_volume_zones_setting_round_trips_through_the_c_view():
    from miunet import hostlib
    default = {"on": False, "channel": 0, "mode": "count", "levels": 32, "lo": 0, "width": 1, "max_run": 32}
    volume, texture = hostlib.get_volume(), hostlib.get_volume_texture()
    assert hostlib.get_volume_zones() == default
    try:
        assert hostlib.set_volume_zones(True, 1, "width", 64, 500, 20, 4096)
        want = {"on": True, "channel": 1, "mode": "width", "levels": 64, "lo": 500, "width": 20, "max_run": 4096}
        assert hostlib.get_volume_zones() == want
        for bad in ((True, -1), (True, 0, 2), (True, 0, -1), (True, 0, "count", 1), (True, 0, "count", 65), (True, 0, "width", 8, -1),
                    (True, 0, "width", 8, 65536), (True, 0, "width", 8, 0, 0), (True, 0, "width", 8, 0, 65537), (True, 0, "count", 8, 0, 1, 1),
                    (True, 0, "count", 8, 0, 1, 8193)):
            assert not hostlib.set_volume_zones(*bad) and hostlib.get_volume_zones() == want, bad
        assert hostlib.set_volume_zones(True, 0, "count", 2, 0, 1, 2) and hostlib.set_volume_zones(True, 0, "width", 64, 65535, 65536, 8192)
        assert hostlib.set_volume_zones(True) and hostlib.get_volume_zones() == dict(default, on=True)
        assert hostlib.get_volume() == volume and hostlib.get_volume_texture() == texture          # a setting of its own
    finally:
        assert hostlib.set_volume_zones(False)
    assert hostlib.get_volume_zones() == default
    for name in ("medseg_set_volume_zones", "medseg_get_volume_zones"):
        assert name in open(os.path.join(ROOT, "include", "medseg_c.h")).read()
