"""Region measurement without a device: mi_unet_region_derive against the header's formulas (tests/regions_ref.derive: Python integers
and math), the struct layout, the argument checks that need no engine, and the facade's JSON writer (libmedseg.so through hostlib) against tests/golden/json.

Tolerance: 1e-12 relative on every derived quantity.  The library converts each exact 128-bit numerator to double once and divides by
A^2; the reference divides the exact integers.  Both are within an ulp or two (2.2e-16) of the true quotient, and the shapes below keep
the cancellation in lambda- = ((a + c) - root) / 2 mild: (a + c) / lambda- stays below 2500, so 1e-12 leaves a factor of ten."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import regions_ref as ref
from miunet import binding, hostlib

EARG = 1


def sums_of(xs, ys, vs=None):
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    vs = [0] * len(xs) if vs is None else [int(v) for v in vs]
    return dict(area=len(xs), x0=min(xs), y0=min(ys), x1=max(xs), y1=max(ys), imin=min(vs), imax=max(vs), channel=0, edges=0,
                sx=sum(xs), sy=sum(ys), sxx=sum(x * x for x in xs), syy=sum(y * y for y in ys), sxy=sum(x * y for x, y in zip(xs, ys)),
                si=sum(vs), sii=sum(v * v for v in vs))


def rect_sums(x0, y0, w, h):
    """closed-form sums of a filled w x h rectangle at (x0, y0), Python ints of any size"""
    s1 = lambda a, n: n * a + n * (n - 1) // 2                                   # sum of a .. a + n - 1
    s2 = lambda a, n: n * a * a + a * n * (n - 1) + (n - 1) * n * (2 * n - 1) // 6     # sum of their squares
    return dict(area=w * h, x0=x0, y0=y0, x1=x0 + w - 1, y1=y0 + h - 1, imin=0, imax=0, channel=-1, edges=2 * (w + h),
                sx=h * s1(x0, w), sy=w * s1(y0, h), sxx=h * s2(x0, w), syy=w * s2(y0, h), sxy=s1(x0, w) * s1(y0, h), si=0, sii=0)


def close(got, want, what):
    assert abs(got - want) <= 1e-12 * abs(want), f"{what}: {got!r} against {want!r}"


def check(r):
    got, want = binding.region_derive(binding.Region(**r)), ref.derive(r)
    for k in ("cx", "cy", "mean", "std", "major", "minor"):
        close(got[k], want[k], k)
    d = (got["theta"] - want["theta"]) % math.pi              # an axis, not a direction: compared modulo pi
    assert min(d, math.pi - d) <= 1e-12, f"theta: {got['theta']!r} against {want['theta']!r}"
    return got


def test_struct_is_96_bytes_and_matches_the_numpy_record():
    assert C.sizeof(binding.Region) == 96
    assert binding.REGION_DTYPE.itemsize == 96
    assert [binding.REGION_DTYPE.fields[n][1] for n, _ in binding.Region._fields_] == [getattr(binding.Region, n).offset for n, _ in binding.Region._fields_]
    assert C.sizeof(binding.Measure) == 8 and C.sizeof(binding.RegionShape) == 56


def test_one_pixel():
    got = check(sums_of([7], [3], [200]))
    close(got["major"], 4 / math.sqrt(12), "major")           # 1.1547: the unit square's own second moment
    close(got["minor"], 4 / math.sqrt(12), "minor")
    assert (got["cx"], got["cy"], got["mean"], got["std"], got["theta"]) == (7.0, 3.0, 200.0, 0.0, 0.0)


@pytest.mark.parametrize("n", [2, 9, 30])
def test_lines(n):
    rng = np.random.default_rng(n)
    h = check(sums_of(range(5, 5 + n), [4] * n, rng.integers(0, 256, n)))            # 1 x N
    close(h["major"], 4 * math.sqrt(n * n / 12), "major")
    close(h["minor"], 4 / math.sqrt(12), "minor")
    assert h["theta"] == 0.0
    v = check(sums_of([4] * n, range(5, 5 + n), rng.integers(0, 256, n)))            # N x 1
    close(v["major"], 4 * math.sqrt(n * n / 12), "major")
    close(abs(v["theta"]), math.pi / 2, "theta")
    d = check(sums_of(range(n), range(n)))                                           # the diagonal: a == c, b = m20
    close(d["theta"], math.pi / 4, "theta")
    close(d["minor"], 4 / math.sqrt(12), "minor")
    a = check(sums_of(range(n), range(n - 1, -1, -1)))                               # the anti-diagonal
    close(a["theta"], -math.pi / 4, "theta")


@pytest.mark.parametrize("x0,y0,w,h", [(0, 0, 1, 1), (3, 9, 17, 5), (100, 7, 6, 40), (11, 11, 8, 8)])
def test_filled_rectangle_closed_form(x0, y0, w, h):
    got = check(rect_sums(x0, y0, w, h))
    close(got["cx"], x0 + (w - 1) / 2, "cx")
    close(got["cy"], y0 + (h - 1) / 2, "cy")
    close(got["major"], 4 * math.sqrt(max(w, h) ** 2 / 12), "major")
    close(got["minor"], 4 * math.sqrt(min(w, h) ** 2 / 12), "minor")
    if w != h:
        close(abs(got["theta"]) + 1.0, (0.0 if w > h else math.pi / 2) + 1.0, "theta")


def test_sums_near_2_to_62():
    """a filled 60000 x 35000 rectangle: 2.1e9 pixels (an int32 area), sxx = 2.52e18 = 2^61.1; the numerators A * sxx - sx^2 pass
    2^90 and are formed in 128-bit integers"""
    r = rect_sums(0, 0, 60000, 35000)
    assert r["area"] < 2 ** 31 and 2 ** 61 < r["sxx"] < 2 ** 62 and r["area"] * r["sxx"] > 2 ** 90
    r.update(si=r["area"] * 255 - 12345, sii=r["area"] * 255 * 255 - 12345 * 509, imin=0, imax=255, channel=0)
    got = check(r)
    close(got["major"], 4 * math.sqrt(60000 ** 2 / 12), "major")
    close(got["minor"], 4 * math.sqrt(35000 ** 2 / 12), "minor")
    close(got["cx"], 29999.5, "cx")


def test_derive_refuses_an_empty_region_and_null():
    L = binding.lib()
    out = binding.RegionShape()
    assert L.mi_unet_region_derive(C.byref(binding.Region()), C.byref(out)) == EARG          # area 0
    assert b"area 0" in L.mi_unet_last_error()
    assert L.mi_unet_region_derive(None, C.byref(out)) == EARG
    assert L.mi_unet_region_derive(C.byref(binding.Region(area=1)), None) == EARG
    with pytest.raises(binding.MiUnetError):
        binding.region_derive(binding.Region(area=-3))


def test_reference_on_a_hand_counted_mask():
    """the reference itself, on numbers counted by hand: a 3 x 3 ring (hole not in the area, hole border in the edges) and a pixel"""
    m = np.zeros((6, 8), np.uint8)
    m[1:4, 1:4] = 255
    m[2, 2] = 0
    m[5, 7] = 255
    t = np.arange(48, dtype=np.uint8).reshape(6, 8)
    pixel, ring = ref.regions_of(m, t)                        # newest (last in raster order) first
    assert pixel == dict(area=1, x0=7, y0=5, x1=7, y1=5, imin=47, imax=47, channel=0, edges=4, sx=7, sy=5, sxx=49, syy=25, sxy=35, si=47,
                         sii=47 * 47)
    assert (ring["area"], ring["edges"], ring["x0"], ring["y0"], ring["x1"], ring["y1"]) == (8, 16, 1, 1, 3, 3)
    assert (ring["sx"], ring["sy"], ring["imin"], ring["imax"]) == (16, 16, 9, 27)


# ---------------------------------------------------------------- the facade's JSON writer (libmedseg.so through hostlib)
REGION_KEYS = ["area", "bbox", "centroid", "edges", "imax", "imin", "major", "mean", "minor", "scale_x", "scale_y", "std", "theta"]


def _poly_cases(golden_dir):
    for c in json.load(open(os.path.join(golden_dir, "json", "cases.json")))["poly"]:
        yield c, open(os.path.join(golden_dir, "json", c["case"] + ".json"), "rb").read()


def _regions_for(n, seed):
    """n plausible regions: filled rectangles with random bytes as intensities"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, binding.REGION_DTYPE)
    for i in range(n):
        x0, y0, w, h = [int(v) for v in rng.integers(0, 400, 2)] + [int(v) for v in rng.integers(1, 40, 2)]
        r = rect_sums(x0, y0, w, h)
        v = [int(t) for t in rng.integers(0, 256, w * h)]
        r.update(imin=min(v), imax=max(v), channel=0, si=sum(v), sii=sum(t * t for t in v))
        for k, val in r.items():
            out[i][k] = val
    return out


def test_json_without_regions_is_the_golden_document(golden_dir):
    for c, want in _poly_cases(golden_dir):
        groups = [(2, [[tuple(p) for p in cc] for cc in c["contours"]])]
        got = hostlib.polygon_json_text_regions(groups, None, 1.0, 1.0, c["base_name"], c["original_width"], c["original_height"])
        assert got == want, c["case"]


def test_json_with_regions_adds_one_object_per_shape_and_round_trips(golden_dir):
    seen = 0
    for n_case, (c, want) in enumerate(_poly_cases(golden_dir)):
        contours = [[tuple(p) for p in cc] for cc in c["contours"]]
        regions = _regions_for(len(contours), n_case)
        sx, sy = 2048 / 512, 1536 / 512 + 1 / 3
        got = hostlib.polygon_json_text_regions([(2, contours)], regions, sx, sy, c["base_name"], c["original_width"], c["original_height"])
        doc, ref_doc = json.loads(got), json.loads(want)
        assert len(doc["shapes"]) == len(contours)
        for shape, rec in zip(doc["shapes"], regions):
            reg = shape.pop("region")
            assert list(reg) == REGION_KEYS                                      # nlohmann's sorted order, nothing else
            assert list(shape) == sorted(shape) and "points" in shape
            r, d = ref.record(rec), binding.region_derive(rec)
            assert (reg["area"], reg["edges"], reg["imin"], reg["imax"]) == (r["area"], r["edges"], r["imin"], r["imax"])
            assert reg["bbox"] == [r["x0"], r["y0"], r["x1"], r["y1"]]
            assert reg["centroid"] == [d["cx"], d["cy"]]                          # shortest round-trip decimals: the same doubles
            for k in ("major", "minor", "theta", "mean", "std"):
                assert reg[k] == d[k] and isinstance(reg[k], float), k
            assert (reg["scale_x"], reg["scale_y"]) == (sx, sy)
            seen += 1
        assert doc == ref_doc                                                     # without the region objects: the golden document
        # ... and byte for byte: cutting the region members out of the text leaves the golden bytes
        assert re.sub(rb'            "region": \{\n(?:                .*\n)*?            \},\n', b"", got) == want, c["case"]
    assert seen > 10


def test_json_two_groups_and_a_region_that_cannot_be_derived():
    groups = [(1, [[(1, 1), (5, 1), (5, 5)]]), (3, [[(7, 7)], [(9, 9), (12, 9)]])]
    regions = _regions_for(3, 99)
    doc = json.loads(hostlib.polygon_json_text_regions(groups, regions, 1.0, 1.0, "two", 64, 64))
    assert [(s["label"], s["labelIndex"], s["region"]["area"]) for s in doc["shapes"]] == \
        [(1, 0, int(regions[0]["area"])), (3, 1, int(regions[1]["area"])), (3, 1, int(regions[2]["area"]))]
    plain = hostlib.polygon_json_text_regions(groups, None, 1.0, 1.0, "two", 64, 64)
    assert plain == hostlib.polygon_json_text_groups(groups, "two", 64, 64)
    regions[1]["area"] = 0
    with pytest.raises(RuntimeError):
        hostlib.polygon_json_text_regions(groups, regions, 1.0, 1.0, "two", 64, 64)
    with pytest.raises(ValueError):
        hostlib.polygon_json_text_regions(groups, regions[:2], 1.0, 1.0, "two", 64, 64)


def test_facade_setting_needs_no_engine():
    assert hostlib.get_measure() == {"on": False, "channel": 0}
    try:
        assert hostlib.set_measure(True, 2) and hostlib.get_measure() == {"on": True, "channel": 2}
        assert not hostlib.set_measure(True, -1) and hostlib.get_measure() == {"on": True, "channel": 2}
    finally:
        assert hostlib.set_measure(False)
    assert hostlib.get_measure() == {"on": False, "channel": 0}
