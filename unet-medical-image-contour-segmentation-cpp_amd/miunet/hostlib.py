"""ctypes binding of libmedseg.so (include/medseg_c.h): the C view of the C++ host facade that keeps the reference's
API names (MedicalSeg::*, Preprocess::*, postprocess_mask, Mask2Polygon::*)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libmedseg.so")
_LIB = None
_u8 = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_u16 = np.ctypeslib.ndpointer(np.uint16, flags="C_CONTIGUOUS")
_i32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")

EXPORTS = ["medseg_initialize_engine", "medseg_process_single_image", "medseg_process_image_batch", "medseg_cleanup_resources", "medseg_get_log_path",
           "medseg_preprocess_raw", "medseg_resample_normalize", "medseg_postprocess_mask", "medseg_mask_to_image",
           "medseg_extract_contours", "medseg_map_points", "medseg_generate_json", "medseg_draw_overlay", "medseg_process_single_mask",
           "medseg_write_png", "medseg_read_png", "medseg_postprocess_mask_target", "medseg_set_targets", "medseg_get_targets",
           "medseg_polygon_json_text_groups", "medseg_draw_overlay_groups",
           "medseg_set_window", "medseg_get_window", "medseg_window_of", "medseg_resample_normalize_window",
           "medseg_set_measure", "medseg_get_measure", "medseg_set_truth_dir", "medseg_get_truth_dir", "medseg_polygon_json_text_regions",
           "medseg_postprocess_mask_morph", "medseg_set_morphology", "medseg_get_morphology", "medseg_set_volume", "medseg_get_volume",
           "medseg_set_volume_clean", "medseg_get_volume_clean", "medseg_set_volume_mesh", "medseg_get_volume_mesh",
           "medseg_set_volume_interp", "medseg_get_volume_interp",
           "medseg_set_volume_measure", "medseg_get_volume_measure", "medseg_set_volume_match", "medseg_get_volume_match",
           "medseg_set_volume_texture", "medseg_get_volume_texture", "medseg_set_volume_zones", "medseg_get_volume_zones",
           "medseg_set_volume_nbhood", "medseg_get_volume_nbhood", "medseg_set_volume_spatial", "medseg_get_volume_spatial",
           "medseg_set_volume_split", "medseg_get_volume_split", "medseg_set_volume_skeleton", "medseg_get_volume_skeleton",
           "medseg_set_volume_branches", "medseg_get_volume_branches"]


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is not built (make -C unet-medical-image-contour-segmentation-cpp_amd)")
        L = C.CDLL(LIB_PATH)
        L.medseg_initialize_engine.argtypes = [C.c_char_p, C.c_char_p]
        L.medseg_process_single_image.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p]
        L.medseg_process_image_batch.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_char_p]
        L.medseg_cleanup_resources.restype = None
        L.medseg_get_log_path.restype = C.c_char_p
        L.medseg_preprocess_raw.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        L.medseg_resample_normalize.argtypes = [_u16, C.c_int, C.c_int, _u8, C.c_int, C.c_int]
        L.medseg_postprocess_mask.argtypes = [_u8, C.c_int, C.c_int, _u8]
        L.medseg_mask_to_image.argtypes = [_u8, C.c_int, C.c_int, _u8]
        L.medseg_extract_contours.argtypes = [_u8, C.c_int, C.c_int, _i32, C.c_int, _i32, C.c_int]
        L.medseg_map_points.argtypes = [_i32, C.c_int, C.c_double, C.c_double, _i32]
        L.medseg_map_points.restype = None
        L.medseg_generate_json.argtypes = [_i32, _i32, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        L.medseg_draw_overlay.argtypes = [_u8, C.c_int, C.c_int, _i32, _i32, C.c_int, _u8]
        L.medseg_process_single_mask.argtypes = [C.c_char_p] * 5
        L.medseg_process_single_mask.restype = None
        L.medseg_write_png.argtypes = [C.c_char_p, _u8, C.c_int, C.c_int, C.c_int, C.c_int]
        L.medseg_read_png.argtypes = [C.c_char_p, C.c_int, _u8, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _i = C.POINTER(C.c_int)
        L.medseg_postprocess_mask_target.argtypes = [_u8, C.c_int, C.c_int, C.c_int, C.c_float, _u8]
        L.medseg_set_targets.argtypes = [_i, C.POINTER(C.c_float), C.c_int]
        L.medseg_get_targets.argtypes = [_i, C.POINTER(C.c_float), C.c_int]
        L.medseg_polygon_json_text_groups.argtypes = [_i32, _i32, _i, _i, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.medseg_draw_overlay_groups.argtypes = [_u8, C.c_int, C.c_int, _i32, _i32, _i, _i, C.c_int, _u8]
        L.medseg_set_window.argtypes = [C.c_int] * 5
        L.medseg_get_window.argtypes = [_i] * 5
        L.medseg_get_window.restype = None
        L.medseg_window_of.argtypes = [_u16, C.c_size_t] + [C.c_int] * 5 + [_i, _i]
        L.medseg_resample_normalize_window.argtypes = [_u16, C.c_int, C.c_int, C.c_int, C.c_int, _u8, C.c_int, C.c_int]
        L.medseg_set_measure.argtypes = [C.c_int, C.c_int]
        L.medseg_get_measure.argtypes = [_i, _i]
        L.medseg_get_measure.restype = None
        L.medseg_set_truth_dir.argtypes = [C.c_char_p]
        L.medseg_get_truth_dir.argtypes = [C.c_char_p, C.c_int]
        L.medseg_polygon_json_text_regions.argtypes = [_i32, _i32, _i, _i, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_char_p, C.c_int,
                                                       C.c_int, C.c_char_p, C.c_int]
        L.medseg_postprocess_mask_morph.argtypes = [_u8, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, _u8]
        L.medseg_set_morphology.argtypes = [_i, _i, _i, C.c_int]
        L.medseg_get_morphology.argtypes = [_i, _i, _i, C.c_int]
        L.medseg_set_volume.argtypes = [C.c_int] * 4 + [C.c_double] * 3
        L.medseg_get_volume.argtypes = [_i] * 4 + [C.POINTER(C.c_double)]
        L.medseg_get_volume.restype = None
        L.medseg_set_volume_clean.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
        L.medseg_get_volume_clean.argtypes = [_i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.medseg_get_volume_clean.restype = None
        L.medseg_set_volume_mesh.argtypes = [C.c_int, C.c_int]
        L.medseg_get_volume_mesh.argtypes = [_i, _i]
        L.medseg_get_volume_mesh.restype = None
        L.medseg_set_volume_interp.argtypes = [C.c_int, C.c_int]
        L.medseg_get_volume_interp.argtypes = [_i, _i]
        L.medseg_get_volume_interp.restype = None
        L.medseg_set_volume_measure.argtypes = [C.c_int, C.c_int, C.c_int]
        L.medseg_get_volume_measure.argtypes = [_i, _i, _i]
        L.medseg_get_volume_measure.restype = None
        L.medseg_set_volume_spatial.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double]
        L.medseg_get_volume_spatial.argtypes = [_i, _i, _i, C.POINTER(C.c_double)]
        L.medseg_get_volume_spatial.restype = None
        L.medseg_set_volume_split.argtypes = [C.c_int, C.c_double, C.c_int]
        L.medseg_get_volume_split.argtypes = [_i, C.POINTER(C.c_double), _i]
        L.medseg_get_volume_split.restype = None
        L.medseg_set_volume_skeleton.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.medseg_get_volume_skeleton.argtypes = [_i, _i, _i, _i]
        L.medseg_get_volume_skeleton.restype = None
        L.medseg_set_volume_branches.argtypes = [C.c_int, C.c_int, C.c_int]
        L.medseg_get_volume_branches.argtypes = [_i, _i, _i]
        L.medseg_get_volume_branches.restype = None
        L.medseg_set_volume_match.argtypes = [C.c_int, C.c_int, C.c_int]
        L.medseg_get_volume_match.argtypes = [_i, _i, _i]
        L.medseg_get_volume_match.restype = None
        L.medseg_set_volume_texture.argtypes = [C.c_int] * 6
        L.medseg_get_volume_texture.argtypes = [_i] * 6
        L.medseg_get_volume_texture.restype = None
        L.medseg_set_volume_zones.argtypes = [C.c_int] * 7
        L.medseg_get_volume_zones.argtypes = [_i] * 7
        L.medseg_get_volume_zones.restype = None
        L.medseg_set_volume_nbhood.argtypes = [C.c_int] * 8
        L.medseg_get_volume_nbhood.argtypes = [_i] * 8
        L.medseg_get_volume_nbhood.restype = None
        _LIB = L
    return _LIB


def _b(s):
    return os.fsencode(s)


def resample_normalize(raw, out_w=512, out_h=512):
    raw = np.ascontiguousarray(raw, np.uint16)
    out = np.empty((out_h, out_w), np.uint8)
    if lib().medseg_resample_normalize(raw, raw.shape[1], raw.shape[0], out, out_w, out_h):
        raise RuntimeError("resample_normalize failed")
    return out


def preprocess_raw(raw_path, png_path, json_path, w, h) -> bool:
    return lib().medseg_preprocess_raw(_b(raw_path), _b(png_path), _b(json_path), w, h) == 0


def postprocess_mask(mask):
    m = np.ascontiguousarray(mask, np.uint8)
    out = np.empty_like(m)
    if lib().medseg_postprocess_mask(m, m.shape[1], m.shape[0], out):
        raise RuntimeError("postprocess_mask failed")
    return out


def postprocess_mask_target(mask, cls, min_area_frac):
    """postprocess_mask(src, cls, min_area_frac): u8 [h][w] label map -> u8 [h][w] in {0, cls}"""
    m = np.ascontiguousarray(mask, np.uint8)
    out = np.empty_like(m)
    if lib().medseg_postprocess_mask_target(m, m.shape[1], m.shape[0], int(cls), float(min_area_frac), out):
        raise RuntimeError("postprocess_mask failed")
    return out


MORPH_SHAPES = {"rect": 0, "disc": 1}


def _shape(shape):
    return MORPH_SHAPES[shape] if isinstance(shape, str) else int(shape)


def postprocess_mask_morph(mask, cls, min_area_frac, shape="rect", open_r=1, close_r=0):
    """postprocess_mask(src, cls, min_area_frac, morph): the chain with a close / open by a box or disc, u8 [h][w] in {0, cls}"""
    m = np.ascontiguousarray(mask, np.uint8)
    out = np.empty_like(m)
    if lib().medseg_postprocess_mask_morph(m, m.shape[1], m.shape[0], int(cls), float(min_area_frac), _shape(shape), int(open_r), int(close_r), out):
        raise RuntimeError("postprocess_mask failed")
    return out


def set_morphology(morph) -> bool:
    """MedicalSeg::set_morphology: [(shape, open_r, close_r), ...], one entry or one per target; [] restores the default; needs no engine"""
    n = len(morph)
    cols = [(C.c_int * max(n, 1))(*[int(v) for v in col]) for col in ([_shape(s) for s, _, _ in morph], [o for _, o, _ in morph], [c for _, _, c in morph])]
    return lib().medseg_set_morphology(cols[0], cols[1], cols[2], n) == 0


def get_morphology():
    s, o, c = (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 8)()
    n = lib().medseg_get_morphology(s, o, c, 8)
    names = {v: k for k, v in MORPH_SHAPES.items()}
    return [(names[s[i]], o[i], c[i]) for i in range(n)]


def _flatten_groups(groups):
    """[(cls, [contour, ...]), ...] -> flattened points, starts, class and contour count per group"""
    contours = [c for _, cs in groups for c in cs]
    flat = np.array([p for c in contours for p in c], np.int32).reshape(-1, 2)
    start = np.zeros(len(contours) + 1, np.int32)
    start[1:] = np.cumsum([len(c) for c in contours])
    n = len(groups)
    return (np.ascontiguousarray(flat).reshape(-1), start, (C.c_int * max(n, 1))(*[int(c) for c, _ in groups]),
            (C.c_int * max(n, 1))(*[len(cs) for _, cs in groups]), n)


def polygon_json_text_groups(groups, base_name, ow, oh) -> bytes:
    """Mask2Polygon::polygon_json_text for (cls, contours) groups in target order"""
    flat, start, cls, cnt, n = _flatten_groups(groups)
    cap = 4096 + 160 * (len(start) + flat.size)
    buf = C.create_string_buffer(cap)
    got = lib().medseg_polygon_json_text_groups(flat, start, cls, cnt, n, base_name.encode(), ow, oh, buf, cap)
    if got < 0:
        raise RuntimeError("polygon_json_text_groups: buffer too small")
    return buf.raw[:got]


def polygon_json_text_regions(groups, regions, scale_x, scale_y, base_name, ow, oh) -> bytes:
    """polygon_json_text_groups with a "region" object per shape: regions = one binding.REGION_DTYPE record per contour, in the order of
    the flattened groups (None: no region objects, the bytes of polygon_json_text_groups)"""
    flat, start, cls, cnt, n = _flatten_groups(groups)
    if regions is not None:
        regions = np.ascontiguousarray(regions)
        if regions.dtype.itemsize != 96 or regions.size != sum(len(cs) for _, cs in groups):
            raise ValueError("one 96-byte region record per contour")
    cap = 4096 + 160 * (len(start) + flat.size) + 1024 * (0 if regions is None else regions.size)
    buf = C.create_string_buffer(cap)
    got = lib().medseg_polygon_json_text_regions(flat, start, cls, cnt, n, None if regions is None else regions.ctypes.data, float(scale_x),
                                                 float(scale_y), base_name.encode(), ow, oh, buf, cap)
    if got < 0:
        raise RuntimeError("polygon_json_text_regions: " + ("buffer too small" if got == -1 else "a region cannot be derived"))
    return buf.raw[:got]


def set_measure(on=True, channel=0) -> bool:
    """MedicalSeg::set_measure: every shape of <base>.json gains a "region" object; needs no engine"""
    return lib().medseg_set_measure(int(bool(on)), int(channel)) == 0


def set_truth_dir(path="") -> bool:
    """MedicalSeg::set_truth_dir: score every processed image that has <path>/<base>_labels.raw into <base>_score.json; "" / None = off"""
    return lib().medseg_set_truth_dir(os.fsencode(path) if path else b"") == 0


def get_truth_dir() -> str:
    buf = C.create_string_buffer(4096)
    n = lib().medseg_get_truth_dir(buf, 4096)
    return os.fsdecode(buf.raw[:n]) if n >= 0 else ""


def set_volume(on=True, connectivity=26, min_voxels=0, keep_largest=0, spacing=(1.0, 1.0, 1.0)) -> bool:
    """MedicalSeg::set_volume: process_image_batch labels its images as the slices of one volume and writes volume_report.json (and
    <base>_volume_mask*.png under a filter); spacing = (x, y, z) in mm on the tile grid; needs no engine"""
    return lib().medseg_set_volume(int(bool(on)), int(connectivity), int(min_voxels), int(keep_largest), *[float(v) for v in spacing]) == 0


def get_volume():
    v, sp = [C.c_int() for _ in range(4)], (C.c_double * 3)()
    lib().medseg_get_volume(*[C.byref(x) for x in v], sp)
    return {"on": bool(v[0].value), "connectivity": v[1].value, "min_voxels": v[2].value, "keep_largest": v[3].value, "spacing": tuple(sp)}


def set_volume_clean(on=True, fill=True, close_mm=0.0, open_mm=0.0) -> bool:
    """MedicalSeg::set_volume_clean: with set_volume on, process_image_batch cleans the stack as a volume before it labels it (3-D cavity
    fill, close and open by a ball in mm) and writes the cleaned stack and a "clean" object in volume_report.json; needs no engine"""
    return lib().medseg_set_volume_clean(int(bool(on)), int(bool(fill)), float(close_mm), float(open_mm)) == 0


def get_volume_clean():
    on, fill, c, o = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    lib().medseg_get_volume_clean(C.byref(on), C.byref(fill), C.byref(c), C.byref(o))
    return {"on": bool(on.value), "fill": bool(fill.value), "close_mm": c.value, "open_mm": o.value}


MESH_PLACEMENTS = {"faces": 0, "nets": 1}


def set_volume_mesh(on=True, placement="faces") -> bool:
    """MedicalSeg::set_volume_mesh: with set_volume on, process_image_batch meshes every target's labelled plane (placement "faces" or
    "nets", or the raw C value) into volume_mesh*.stl and a "mesh" object in volume_report.json; needs no engine"""
    return lib().medseg_set_volume_mesh(int(bool(on)), MESH_PLACEMENTS[placement] if isinstance(placement, str) else int(placement)) == 0


def get_volume_mesh():
    on, placement = C.c_int(), C.c_int()
    lib().medseg_get_volume_mesh(C.byref(on), C.byref(placement))
    return {"on": bool(on.value), "placement": {v: k for k, v in MESH_PLACEMENTS.items()}[placement.value]}


def set_volume_interp(on=True, factor=0) -> bool:
    """MedicalSeg::set_volume_interp: with set_volume on, process_image_batch puts factor - 1 shape-based slices between the slices of
    every target's labelled plane before it is meshed (factor 0 or "iso": spacing_z over the smaller in-plane spacing, 1 .. 16) and adds
    an "interp" object to volume_report.json; needs no engine"""
    return lib().medseg_set_volume_interp(int(bool(on)), 0 if factor == "iso" else int(factor)) == 0


def get_volume_interp():
    on, factor = C.c_int(), C.c_int()
    lib().medseg_get_volume_interp(C.byref(on), C.byref(factor))
    return {"on": bool(on.value), "factor": factor.value}


def set_volume_measure(on=True, channel=0, max_ends=262144) -> bool:
    """MedicalSeg::set_volume_measure: with set_volume on, process_image_batch measures every component of the labelled stack
    (mi_unet_volume_measure over `channel` of the normalised tiles) into a "measure" member of volume_report.json; needs no engine"""
    return lib().medseg_set_volume_measure(int(bool(on)), int(channel), int(max_ends)) == 0


def get_volume_measure():
    on, channel, ends = C.c_int(), C.c_int(), C.c_int()
    lib().medseg_get_volume_measure(C.byref(on), C.byref(channel), C.byref(ends))
    return {"on": bool(on.value), "channel": channel.value, "max_ends": ends.value}


VSPATIAL_DEFAULT_PEAK_MM = 6.2035           # the radius of the sphere of 1 cm^3


def set_volume_spatial(on=True, channel=0, max_voxels=131072, peak_mm=VSPATIAL_DEFAULT_PEAK_MM) -> bool:
    """MedicalSeg::set_volume_spatial: with set_volume on, process_image_batch adds Moran's I, Geary's C, the centre-of-mass shift, the
    integrated intensity and the local / global intensity peak of every component of the labelled stack (mi_unet_volume_spatial over
    `channel` of the normalised tiles) as a "spatial" member of volume_report.json; needs no engine"""
    return lib().medseg_set_volume_spatial(int(bool(on)), int(channel), int(max_voxels), float(peak_mm)) == 0


def get_volume_spatial():
    on, channel, voxels, peak = C.c_int(), C.c_int(), C.c_int(), C.c_double()
    lib().medseg_get_volume_spatial(C.byref(on), C.byref(channel), C.byref(voxels), C.byref(peak))
    return {"on": bool(on.value), "channel": channel.value, "max_voxels": voxels.value, "peak_mm": peak.value}


def set_volume_split(on=True, neck_mm=0.0, min_core=1) -> bool:
    """MedicalSeg::set_volume_split: with set_volume on, process_image_batch splits the touching objects of the labelled stack
    (mi_unet_volume_split behind the components stage: cores of the erosion by a ball of neck_mm, regrown by geodesic distance) and
    hands the pieces to the report and to every stage behind it; every component and every target of volume_report.json gains a
    "split" member; needs no engine"""
    return lib().medseg_set_volume_split(int(bool(on)), float(neck_mm), int(min_core)) == 0


def get_volume_split():
    on, neck, core = C.c_int(), C.c_double(), C.c_int()
    lib().medseg_get_volume_split(C.byref(on), C.byref(neck), C.byref(core))
    return {"on": bool(on.value), "neck_mm": neck.value, "min_core": core.value}


def set_volume_skeleton(on=True, radius=True, png=False, max_passes=0) -> bool:
    """MedicalSeg::set_volume_skeleton: with set_volume on, process_image_batch thins every component of the labelled stack to its
    medial line (mi_unet_volume_skeleton on the ids of the components stage, or of the split) and every component of
    volume_report.json gains a last member "skeleton"; with png the skeleton of every slice is written as a picture; needs no engine"""
    return lib().medseg_set_volume_skeleton(int(bool(on)), int(bool(radius)), int(bool(png)), int(max_passes)) == 0


def get_volume_skeleton():
    on, radius, png, passes = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    lib().medseg_get_volume_skeleton(C.byref(on), C.byref(radius), C.byref(png), C.byref(passes))
    return {"on": bool(on.value), "radius": bool(radius.value), "png": bool(png.value), "max_passes": passes.value}


def set_volume_branches(on=True, prune_voxels=0, prune_rounds=0) -> bool:
    """MedicalSeg::set_volume_branches: with set_volume and set_volume_skeleton on, process_image_batch splits every skeleton into nodes
    and branches (mi_unet_volume_branches on the skeleton stage's ids and radii), prunes spurs of at most prune_voxels voxels, and every
    component of volume_report.json gains a last member "branches"; needs no engine"""
    return lib().medseg_set_volume_branches(int(bool(on)), int(prune_voxels), int(prune_rounds)) == 0


def get_volume_branches():
    on, prune, rounds = C.c_int(), C.c_int(), C.c_int()
    lib().medseg_get_volume_branches(C.byref(on), C.byref(prune), C.byref(rounds))
    return {"on": bool(on.value), "prune_voxels": prune.value, "prune_rounds": rounds.value}


VTEX_MODES = ("count", "width")           # MI_UNET_VTEX_COUNT, MI_UNET_VTEX_WIDTH


def set_volume_texture(on=True, channel=0, mode="count", levels=32, lo=0, width=1) -> bool:
    """MedicalSeg::set_volume_texture: with set_volume on, process_image_batch adds the grey-level histogram and the co-occurrence
    texture of every component of the labelled stack (mi_unet_volume_texture over `channel` of the normalised tiles) as a "texture"
    member of volume_report.json; needs no engine"""
    mode = VTEX_MODES.index(mode) if mode in VTEX_MODES else int(mode)
    return lib().medseg_set_volume_texture(int(bool(on)), int(channel), mode, int(levels), int(lo), int(width)) == 0


def get_volume_texture():
    v = [C.c_int() for _ in range(6)]
    lib().medseg_get_volume_texture(*[C.byref(x) for x in v])
    on, channel, mode, levels, lo, width = (x.value for x in v)
    return {"on": bool(on), "channel": channel, "mode": VTEX_MODES[mode], "levels": levels, "lo": lo, "width": width}


def set_volume_zones(on=True, channel=0, mode="count", levels=32, lo=0, width=1, max_run=32) -> bool:
    """MedicalSeg::set_volume_zones: with set_volume on, process_image_batch adds the run-length and size-zone matrices' features of
    every component of the labelled stack (mi_unet_volume_zones over `channel` of the normalised tiles) as a "zones" member of
    volume_report.json; needs no engine"""
    mode = VTEX_MODES.index(mode) if mode in VTEX_MODES else int(mode)
    return lib().medseg_set_volume_zones(int(bool(on)), int(channel), mode, int(levels), int(lo), int(width), int(max_run)) == 0


def get_volume_zones():
    v = [C.c_int() for _ in range(7)]
    lib().medseg_get_volume_zones(*[C.byref(x) for x in v])
    on, channel, mode, levels, lo, width, max_run = (x.value for x in v)
    return {"on": bool(on), "channel": channel, "mode": VTEX_MODES[mode], "levels": levels, "lo": lo, "width": width, "max_run": max_run}


def set_volume_nbhood(on=True, channel=0, mode="count", levels=32, lo=0, width=1, alpha=0, max_dist=32) -> bool:
    """MedicalSeg::set_volume_nbhood: with set_volume on, process_image_batch adds the neighbourhood-difference, dependence and
    distance-zone features of every component of the labelled stack (mi_unet_volume_nbhood over `channel` of the normalised tiles) as
    a "nbhood" member of volume_report.json; needs no engine"""
    mode = VTEX_MODES.index(mode) if mode in VTEX_MODES else int(mode)
    return lib().medseg_set_volume_nbhood(int(bool(on)), int(channel), mode, int(levels), int(lo), int(width), int(alpha), int(max_dist)) == 0


def get_volume_nbhood():
    v = [C.c_int() for _ in range(8)]
    lib().medseg_get_volume_nbhood(*[C.byref(x) for x in v])
    on, channel, mode, levels, lo, width, alpha, max_dist = (x.value for x in v)
    return {"on": bool(on), "channel": channel, "mode": VTEX_MODES[mode], "levels": levels, "lo": lo, "width": width, "alpha": alpha, "max_dist": max_dist}


def set_volume_match(on=True, iou=(1, 2)) -> bool:
    """MedicalSeg::set_volume_match: where set_volume on and set_truth_dir produce volume_score.json, every target gains a "lesions"
    member (mi_unet_volume_match, then the one-to-one assignment at the IoU threshold iou = (num, den)); needs no engine"""
    return lib().medseg_set_volume_match(int(bool(on)), int(iou[0]), int(iou[1])) == 0


def get_volume_match():
    on, num, den = C.c_int(), C.c_int(), C.c_int()
    lib().medseg_get_volume_match(C.byref(on), C.byref(num), C.byref(den))
    return {"on": bool(on.value), "iou": (num.value, den.value)}


def get_measure():
    on, ch = C.c_int(), C.c_int()
    lib().medseg_get_measure(C.byref(on), C.byref(ch))
    return {"on": bool(on.value), "channel": ch.value}


def draw_overlay_groups(gray, groups):
    """gray u8 [h][w] + (cls, contours) groups -> BGR u8 [h][w][3], group g in colour g of the palette"""
    g = np.ascontiguousarray(gray, np.uint8)
    flat, start, cls, cnt, n = _flatten_groups(groups)
    out = np.empty(g.shape + (3,), np.uint8)
    if lib().medseg_draw_overlay_groups(g, g.shape[1], g.shape[0], flat, start, cls, cnt, n, out.reshape(-1)):
        raise RuntimeError("draw_overlay failed")
    return out


def set_targets(targets) -> bool:
    """MedicalSeg::set_targets: [(cls, min_area_frac), ...]; [] restores the default"""
    n = len(targets)
    return lib().medseg_set_targets((C.c_int * max(n, 1))(*[int(c) for c, _ in targets]),
                                    (C.c_float * max(n, 1))(*[float(f) for _, f in targets]), n) == 0


def get_targets():
    cls, frac = (C.c_int * 8)(), (C.c_float * 8)()
    n = lib().medseg_get_targets(cls, frac, 8)
    return [(cls[i], float(frac[i])) for i in range(n)]


WINDOW_MODES = {"minmax": 0, "percentile": 1, "fixed": 2}


def _mode(mode):
    return WINDOW_MODES[mode] if isinstance(mode, str) else int(mode)


def set_window(mode="minmax", clip_lo_ppm=0, clip_hi_ppm=0, lo=0, hi=65535) -> bool:
    """MedicalSeg::set_window: mode "minmax" | "percentile" | "fixed" (or the raw C value); needs no engine"""
    return lib().medseg_set_window(_mode(mode), int(clip_lo_ppm), int(clip_hi_ppm), int(lo), int(hi)) == 0


def get_window():
    v = [C.c_int() for _ in range(5)]
    lib().medseg_get_window(*[C.byref(x) for x in v])
    return {"mode": {b: a for a, b in WINDOW_MODES.items()}[v[0].value], "clip_lo_ppm": v[1].value, "clip_hi_ppm": v[2].value,
            "lo": v[3].value, "hi": v[4].value}


def window_of(samples, mode="minmax", clip_lo_ppm=0, clip_hi_ppm=0, lo=0, hi=65535):
    """Preprocess::window_of: (lo, hi) of the u16 samples under a window setting"""
    a = np.ascontiguousarray(samples, np.uint16).reshape(-1)
    wlo, whi = C.c_int(), C.c_int()
    if lib().medseg_window_of(a, a.size, _mode(mode), int(clip_lo_ppm), int(clip_hi_ppm), int(lo), int(hi), C.byref(wlo), C.byref(whi)):
        raise ValueError("window_of: illegal window or no samples")
    return wlo.value, whi.value


def resample_normalize_window(raw, lo, hi, out_w=512, out_h=512):
    raw = np.ascontiguousarray(raw, np.uint16)
    out = np.empty((out_h, out_w), np.uint8)
    if lib().medseg_resample_normalize_window(raw, raw.shape[1], raw.shape[0], int(lo), int(hi), out, out_w, out_h):
        raise RuntimeError("resample_normalize_window failed")
    return out


def mask_to_image(mask):
    m = np.ascontiguousarray(mask, np.uint8)
    out = np.empty_like(m)
    lib().medseg_mask_to_image(m, m.shape[1], m.shape[0], out)
    return out


def extract_contours(mask):
    m = np.ascontiguousarray(mask, np.uint8)
    h, w = m.shape
    cap_p, cap_c = 2 * h * w + 16, h * w + 2
    xy = np.zeros((cap_p, 2), np.int32)
    st = np.zeros(cap_c + 1, np.int32)
    n = lib().medseg_extract_contours(m, w, h, xy.reshape(-1), cap_p, st, cap_c)
    if n < 0:
        raise RuntimeError("contour capacity")
    return [[tuple(p) for p in xy[st[i]:st[i + 1]].tolist()] for i in range(n)]


def map_points(pts, sx, sy):
    a = np.ascontiguousarray(np.array(pts, np.int32).reshape(-1, 2))
    out = np.empty_like(a)
    lib().medseg_map_points(a.reshape(-1), a.shape[0], sx, sy, out.reshape(-1))
    return [tuple(p) for p in out.tolist()]


def generate_json(contours, json_path, base_name, ow, oh):
    flat = np.array([p for c in contours for p in c], np.int32).reshape(-1, 2)
    start = np.zeros(len(contours) + 1, np.int32)
    start[1:] = np.cumsum([len(c) for c in contours])
    if lib().medseg_generate_json(np.ascontiguousarray(flat).reshape(-1), start, len(contours), _b(json_path), base_name.encode(), ow, oh):
        raise RuntimeError("generate_json failed")


def draw_overlay(gray, contours):
    """gray u8 [h][w] + contours -> BGR u8 [h][w][3] (the _contour_overlay.png pixels)"""
    g = np.ascontiguousarray(gray, np.uint8)
    flat = np.array([p for c in contours for p in c], np.int32).reshape(-1, 2)
    start = np.zeros(len(contours) + 1, np.int32)
    start[1:] = np.cumsum([len(c) for c in contours])
    out = np.empty(g.shape + (3,), np.uint8)
    if lib().medseg_draw_overlay(g, g.shape[1], g.shape[0], np.ascontiguousarray(flat).reshape(-1), start, len(contours), out.reshape(-1)):
        raise RuntimeError("draw_overlay failed")
    return out


def process_single_mask(mask_path, output_dir, json_path, original_png, base_name):
    lib().medseg_process_single_mask(_b(mask_path), _b(output_dir), _b(json_path), _b(original_png), base_name.encode())


def write_png(path, img, level0=True):
    a = np.ascontiguousarray(img, np.uint8)
    ch = 1 if a.ndim == 2 else a.shape[2]
    return lib().medseg_write_png(_b(path), a.reshape(-1), a.shape[1], a.shape[0], ch, int(level0)) == 0


def read_png(path, as_color=False):
    buf = np.empty(64 << 20, np.uint8)
    w, h = C.c_int(), C.c_int()
    if lib().medseg_read_png(_b(path), int(as_color), buf, buf.size, C.byref(w), C.byref(h)):
        return None
    n = w.value * h.value * (3 if as_color else 1)
    return buf[:n].reshape((h.value, w.value, 3) if as_color else (h.value, w.value)).copy()


def initialize_engine(weight_path, log_dir) -> bool:
    return lib().medseg_initialize_engine(_b(weight_path), _b(log_dir)) == 0


def process_single_image(raw_path, w, h, output_dir) -> bool:
    return lib().medseg_process_single_image(_b(raw_path), w, h, _b(output_dir)) == 0


def process_image_batch(raw_paths, widths, heights, output_dir) -> int:
    n = len(raw_paths)
    arr = (C.c_char_p * n)(*[_b(p) for p in raw_paths])
    return lib().medseg_process_image_batch(arr, (C.c_int * n)(*widths), (C.c_int * n)(*heights), n, _b(output_dir))


def cleanup_resources():
    lib().medseg_cleanup_resources()


def get_log_path() -> str:
    return lib().medseg_get_log_path().decode()
