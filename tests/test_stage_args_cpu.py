"""The messages of the argument checks that the stages behind the network share (csrc/stage_common.h): every `_host` entry point on the
smallest good call -- 2 x 2 x 2, one value, one component -- with one argument broken at a time: a side of 0, a side above the stage's
maximum, a value of 256, a value listed twice, a unit of 0, and a product of the sides at 2^31 (each side within its own bound).  Each
must return MI_UNET_EARG with exactly the text written out here; nothing is read or written before a check fails, so the small
arrays serve the large claimed sizes too.

The three texture stages (csrc/texture_common.h) also share the checks of m, mode, levels, width and lo, and their derive functions
the checks of a component's voxels and of the levels: those messages are pinned the same way, with each stage's own cells bound."""
import ctypes as C

import numpy as np
import pytest

from miunet import binding


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def room():
    return np.zeros(8192, np.uint8)            # more than any output of the smallest call


def call(stage, **over):
    """the smallest good call of `stage` with the overrides; returns (rc, last error)"""
    L = binding.lib()
    a = dict(D=2, H=2, W=2, values=[1], units=[1, 1, 1], placement=0, m=1, mode=0, levels=32, lo=0, width=1, max_run=32, alpha=0, max_dist=32)
    a.update(over)
    D, H, W = a["D"], a["H"], a["W"]
    values, units = np.array(a["values"], np.int32), np.array(a["units"], np.int32)
    n = len(values)
    u8, u8b, i32, i32b, u16 = (np.ones((2, 2, 2), t) for t in (np.uint8, np.uint8, np.int32, np.int32, np.uint16))
    found = C.cast(ptr(room()), C.POINTER(C.c_int))
    common = (a["mode"], a["levels"], a["lo"], a["width"])
    vtx, vzn, vnb = binding.VTextureOpts(*common), binding.VZonesOpts(*common, a["max_run"]), binding.VNbhoodOpts(*common, a["alpha"], a["max_dist"])
    rc = {
        "score_labels": lambda: L.mi_unet_score_labels_host(ptr(u8), ptr(u8b), D, H, W, ptr(values), n, None, ptr(room()), None, None),
        "score_volume": lambda: L.mi_unet_score_volume_host(ptr(u8), ptr(u8b), D, H, W, ptr(values), n, ptr(units), None, ptr(room()), None, None),
        "volume_components": lambda: L.mi_unet_volume_components_host(ptr(u8), D, H, W, ptr(values), n, None, ptr(room()), ptr(room()), ptr(room()), 1,
                                                                      ptr(room()), ptr(room())),
        "volume_clean": lambda: L.mi_unet_volume_clean_host(ptr(u8), D, H, W, ptr(values), n, ptr(units), None, ptr(room()), ptr(room())),
        "volume_mesh": lambda: L.mi_unet_volume_mesh_host(ptr(u8), D, H, W, ptr(values), n, a["placement"], None, 0, None, 0, ptr(room())),
        "volume_measure": lambda: L.mi_unet_volume_measure_host(ptr(i32), ptr(u16), D, H, W, 1, ptr(units), None, ptr(room())),
        "volume_texture": lambda: L.mi_unet_volume_texture_host(ptr(i32), ptr(u16), D, H, W, a["m"], C.byref(vtx), ptr(room()), ptr(room()), None, None),
        "volume_zones": lambda: L.mi_unet_volume_zones_host(ptr(i32), ptr(u16), D, H, W, a["m"], C.byref(vzn), ptr(room()), None, None, None, 0, None),
        "volume_nbhood": lambda: L.mi_unet_volume_nbhood_host(ptr(i32), ptr(u16), D, H, W, a["m"], C.byref(vnb), ptr(room()), None),
        "volume_match": lambda: L.mi_unet_volume_match_host(ptr(i32), ptr(i32b), D, H, W, 1, 1, 1, ptr(room()), ptr(room()), ptr(room()), found),
    }[stage]()
    return rc, L.mi_unet_last_error().decode()


TWICE, NOT_A_BYTE, AT_2_31 = dict(values=[1, 1]), dict(values=[256]), dict(D=32, H=8192, W=8192)

CASES = {
    # (mi_unet_score_labels takes B images of H x W: D is B here)
    "score_labels": [
        (dict(H=0), "mi_unet_score_labels_host: 0 x 2 is outside 1 .. 32767 per side"),
        (dict(W=32768), "mi_unet_score_labels_host: 2 x 32768 is outside 1 .. 32767 per side"),
        (NOT_A_BYTE, "mi_unet_score_labels_host: value 256 is not a byte"),
        (TWICE, "mi_unet_score_labels_host: value 1 is listed twice"),
        (dict(D=8, H=16384, W=16384), "mi_unet_score_labels_host: B * n * H * W must stay below 2^31"),
    ],
    "score_volume": [
        (dict(D=0), "mi_unet_score_volume_host: 0 x 2 x 2 is outside 1 .. 8192 per side"),
        (dict(W=8193), "mi_unet_score_volume_host: 2 x 2 x 8193 is outside 1 .. 8192 per side"),
        (NOT_A_BYTE, "mi_unet_score_volume_host: value 256 is not a byte"),
        (TWICE, "mi_unet_score_volume_host: value 1 is listed twice"),
        (dict(units=[1, 0, 1]), "mi_unet_score_volume_host: spacing unit 0 (at least 1)"),
        (AT_2_31, "mi_unet_score_volume_host: n * D * H * W must stay below 2^31"),
    ],
    "volume_components": [
        (dict(H=0), "mi_unet_volume_components_host: 2 x 0 x 2 (every side at least 1)"),
        (NOT_A_BYTE, "mi_unet_volume_components_host: value 256 is not a byte"),
        (TWICE, "mi_unet_volume_components_host: value 1 is listed twice"),
        (AT_2_31, "mi_unet_volume_components_host: n * D * H * W must stay below 2^31"),
    ],
    "volume_clean": [
        (dict(D=0), "mi_unet_volume_clean_host: 0 x 2 x 2 (every side at least 1)"),
        (NOT_A_BYTE, "mi_unet_volume_clean_host: value 256 is not a byte"),
        (TWICE, "mi_unet_volume_clean_host: value 1 is listed twice"),
        (dict(units=[0, 1, 1]), "mi_unet_volume_clean_host: spacing unit 0 is outside 1 .. 46340"),
        (AT_2_31, "mi_unet_volume_clean_host: n * D * H * W must stay below 2^31"),
    ],
    # (the mesh bounds its corners, 6 (D + 1)(H + 1)(W + 1), which no sides bring to 2^31 itself: 6 * 711 * 710 * 710 is the first
    # such product past it, 6 * 710^3 the last below)
    "volume_mesh": [
        (dict(W=0), "mi_unet_volume_mesh_host: 2 x 2 x 0 (every side at least 1)"),
        (NOT_A_BYTE, "mi_unet_volume_mesh_host: value 256 is not a byte"),
        (TWICE, "mi_unet_volume_mesh_host: value 1 is listed twice"),
        (dict(D=710, H=709, W=709), "mi_unet_volume_mesh_host: 6 * (D + 1) * (H + 1) * (W + 1) must stay below 2^31"),
    ],
    "volume_measure": [
        (dict(W=0), "mi_unet_volume_measure_host: 2 x 2 x 0 is outside 1 .. 8192 per side"),
        (dict(D=8193), "mi_unet_volume_measure_host: 8193 x 2 x 2 is outside 1 .. 8192 per side"),
        (dict(units=[1, 1, 0]), "mi_unet_volume_measure_host: spacing unit 0 (at least 1)"),
        (AT_2_31, "mi_unet_volume_measure_host: D * H * W must stay below 2^31"),
    ],
    # (the texture's own bound is 2^28 voxels, so that is what a volume of 2^31 meets)
    "volume_texture": [
        (dict(H=0), "mi_unet_volume_texture_host: 2 x 0 x 2 is outside 1 .. 8192 per side"),
        (dict(H=8193), "mi_unet_volume_texture_host: 2 x 8193 x 2 is outside 1 .. 8192 per side"),
        (AT_2_31, "mi_unet_volume_texture_host: D * H * W must not pass 2^28"),
        (dict(m=4096, levels=64), "mi_unet_volume_texture_host: 4096 components at 64 levels pass 2^22 cells per table"),
    ],
    "volume_zones": [
        (dict(H=0), "mi_unet_volume_zones_host: 2 x 0 x 2 is outside 1 .. 8192 per side"),
        (dict(H=8193), "mi_unet_volume_zones_host: 2 x 8193 x 2 is outside 1 .. 8192 per side"),
        (AT_2_31, "mi_unet_volume_zones_host: D * H * W must not pass 2^28"),
        (dict(m=4096, levels=64), "mi_unet_volume_zones_host: 4096 components at 64 levels and max_run 32 pass 2^22 cells per table"),
    ],
    "volume_nbhood": [
        (dict(H=0), "mi_unet_volume_nbhood_host: 2 x 0 x 2 is outside 1 .. 8192 per side"),
        (dict(H=8193), "mi_unet_volume_nbhood_host: 2 x 8193 x 2 is outside 1 .. 8192 per side"),
        (AT_2_31, "mi_unet_volume_nbhood_host: D * H * W must not pass 2^28"),
        (dict(m=4096, levels=64), "mi_unet_volume_nbhood_host: 4096 components at 64 levels and max_dist 32 pass 2^22 cells per table"),
    ],
    "volume_match": [
        (dict(D=0), "mi_unet_volume_match_host: 0 x 2 x 2 (every side at least 1)"),
        (AT_2_31, "mi_unet_volume_match_host: D * H * W must stay below 2^31"),
    ],
}


# what the three texture stages refuse with one text, behind "<entry point>: "
TEXTURE_STAGES = ("volume_texture", "volume_zones", "volume_nbhood")
TEXTURE_CASES = [
    (dict(m=0), "0 components (1 .. 4096)"),
    (dict(m=4097), "4097 components (1 .. 4096)"),
    (dict(mode=2), "mode 2 does not exist"),
    (dict(levels=1), "1 levels (2 .. 64)"),
    (dict(levels=65), "65 levels (2 .. 64)"),
    (dict(width=0), "width 0 is outside 1 .. 65536"),
    (dict(width=65537), "width 65537 is outside 1 .. 65536"),
    (dict(lo=-1), "lo -1 is outside 0 .. 65535"),
    (dict(lo=65536), "lo 65536 is outside 0 .. 65535"),
]
for _stage in TEXTURE_STAGES:
    CASES[_stage] += [(over, f"mi_unet_{_stage}_host: {text}") for over, text in TEXTURE_CASES]


@pytest.mark.parametrize("stage", list(CASES))
def test_the_smallest_call_is_good(stage):
    assert call(stage)[0] == 0


@pytest.mark.parametrize("stage,case", [(s, k) for s, cases in CASES.items() for k in range(len(cases))])
def test_a_broken_argument_is_refused_with_its_message(stage, case):
    over, text = CASES[stage][case]
    assert call(stage, **over) == (1, text)


def test_the_mesh_bound_is_met_from_below():
    """6 * 710^3 passes the bound: the call is refused by the check behind it"""
    assert call("volume_mesh", D=709, H=709, W=709, placement=7) == \
        (1, "mi_unet_volume_mesh_host: placement 7 is neither MI_UNET_MESH_FACES nor MI_UNET_MESH_NETS")


def test_measure_derive_refuses_a_unit_of_zero():
    comp = binding.VMeasure()
    comp.voxels = 1
    with pytest.raises(binding.MiUnetError) as e:
        binding.volume_measure_derive(comp, (1, 0, 1), 1.0)
    assert e.value.code == 1 and str(e.value) == "libmiunet error 1: mi_unet_volume_measure_derive: spacing unit 0 (at least 1)"


def derive(fn, voxels, levels):
    """the derive function `fn` on a component of `voxels` voxels at `levels` levels, everything else good; returns (rc, last error)"""
    L = binding.lib()
    zones = binding.VZones(voxels=voxels)
    rc = {
        "mi_unet_volume_texture_derive": lambda: L.mi_unet_volume_texture_derive(C.byref(binding.VTexture(voxels=voxels)), ptr(room()), None, levels,
                                                                                 C.byref(binding.VTextureFeatures())),
        "mi_unet_volume_zones_run_features": lambda: L.mi_unet_volume_zones_run_features(C.byref(zones), ptr(room()), levels, 2, 13,
                                                                                         C.byref(binding.VZoneFeatures())),
        "mi_unet_volume_zones_zone_features": lambda: L.mi_unet_volume_zones_zone_features(C.byref(zones), None, 0, 0, levels,
                                                                                           C.byref(binding.VZoneFeatures())),
        "mi_unet_volume_nbhood_derive": lambda: L.mi_unet_volume_nbhood_derive(C.byref(binding.VNbhood(voxels=voxels)), C.byref(binding.VNbhoodOut()),
                                                                               levels, 1, 0, C.byref(binding.VNbhoodFeatures())),
    }[fn]()
    return rc, L.mi_unet_last_error().decode()


DERIVES = ("mi_unet_volume_texture_derive", "mi_unet_volume_zones_run_features", "mi_unet_volume_zones_zone_features", "mi_unet_volume_nbhood_derive")


@pytest.mark.parametrize("fn", DERIVES)
def test_the_derive_functions_refuse_a_component_without_voxels_and_a_single_level(fn):
    assert derive(fn, 1, 2)[0] == 0
    assert derive(fn, 0, 2) == (1, f"{fn}: voxels 0 (a component has at least one voxel)")
    assert derive(fn, 1, 1) == (1, f"{fn}: 1 levels (2 .. 64)")
