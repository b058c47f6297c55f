"""ctypes binding of libmiunet.so (include/mi_unet.h) for the tests and bench.py.

The library is the product; this file is plumbing.  It raises if the shared object is missing or if a call fails --
there is no Python/CPU fallback of any kind.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MIUNET_LIB: another build of the same library (same-card A/B measurements of a kernel change, tools/dev/)
LIB_PATH = os.environ.get("MIUNET_LIB") or os.path.join(PKG_DIR, "libmiunet.so")

EXPORTS = [
    "mi_unet_default_config", "mi_unet_create", "mi_unet_load_weights", "mi_unet_load_weights_from_memory",
    "mi_unet_infer_u8", "mi_unet_infer_u8_device", "mi_unet_infer_raw16", "mi_unet_set_postprocess", "mi_unet_postprocess_masks", "mi_unet_extract_contours", "mi_unet_segment_raw16", "mi_unet_set_stream", "mi_unet_sync", "mi_unet_timer_begin",
    "mi_unet_timer_end", "mi_unet_set_profiling", "mi_unet_get_kernel_stats", "mi_unet_layer_debug", "mi_unet_layer_debug_strided", "mi_unet_destroy",
    "mi_unet_last_error", "mi_unet_device_count", "mi_unet_clone",
    "mi_unet_debug_layer_count", "mi_unet_debug_layer_info", "mi_unet_debug_capture", "mi_unet_last_stage_ms", "mi_unet_numeric_guard", "mi_unet_host_alloc", "mi_unet_host_free",
    "mi_unet_group_create", "mi_unet_group_clone", "mi_unet_group_size", "mi_unet_group_handle", "mi_unet_group_load_weights",
    "mi_unet_group_load_weights_from_memory", "mi_unet_group_set_gather", "mi_unet_group_set_postprocess",
    "mi_unet_group_weight_transport", "mi_unet_group_gather", "mi_unet_group_infer_u8", "mi_unet_group_infer_raw16",
    "mi_unet_group_segment_raw16", "mi_unet_group_destroy", "mi_unet_shard_range",
    "mi_unet_tile_axis", "mi_unet_infer_tiled_u8", "mi_unet_infer_tiled_raw16", "mi_unet_segment_tiled_raw16",
    "mi_unet_set_tile_blend", "mi_unet_get_tile_blend", "mi_unet_tile_blend_weights",
    "mi_unet_target_min_area", "mi_unet_set_targets", "mi_unet_get_targets", "mi_unet_postprocess_masks_multi",
    "mi_unet_segment_raw16_multi", "mi_unet_segment_tiled_raw16_multi", "mi_unet_group_set_targets",
    "mi_unet_group_segment_raw16_multi",
    "mi_unet_set_window", "mi_unet_get_window", "mi_unet_window_of", "mi_unet_last_windows", "mi_unet_group_set_window",
    "mi_unet_set_measure", "mi_unet_get_measure", "mi_unet_last_regions", "mi_unet_measure_regions", "mi_unet_region_derive",
    "mi_unet_group_set_measure", "mi_unet_group_last_regions",
    "mi_unet_set_morph", "mi_unet_get_morph", "mi_unet_morph_element", "mi_unet_group_set_morph",
    "mi_unet_score_labels", "mi_unet_score_labels_host", "mi_unet_score_derive",
    "mi_unet_volume_components", "mi_unet_volume_components_host", "mi_unet_volume_derive",
    "mi_unet_score_volume", "mi_unet_score_volume_host", "mi_unet_score_volume_units", "mi_unet_score_volume_derive",
    "mi_unet_volume_clean", "mi_unet_volume_clean_host", "mi_unet_volume_ball",
    "mi_unet_volume_mesh", "mi_unet_volume_mesh_host", "mi_unet_volume_mesh_positions", "mi_unet_volume_mesh_derive",
    "mi_unet_volume_measure", "mi_unet_volume_measure_host", "mi_unet_volume_measure_derive",
    "mi_unet_volume_spatial", "mi_unet_volume_spatial_host", "mi_unet_volume_spatial_derive",
    "mi_unet_volume_split", "mi_unet_volume_split_host", "mi_unet_volume_split_derive",
    "mi_unet_volume_skeleton", "mi_unet_volume_skeleton_host", "mi_unet_volume_skeleton_derive",
    "mi_unet_volume_skeleton_simple", "mi_unet_volume_skeleton_simple_host",
    "mi_unet_volume_branches", "mi_unet_volume_branches_host", "mi_unet_volume_branches_derive_branch", "mi_unet_volume_branches_derive",
    "mi_unet_volume_texture", "mi_unet_volume_texture_host", "mi_unet_volume_texture_derive",
    "mi_unet_volume_match", "mi_unet_volume_match_host", "mi_unet_volume_match_assign", "mi_unet_volume_match_derive",
    "mi_unet_volume_interp", "mi_unet_volume_interp_host", "mi_unet_volume_interp_slices",
    "mi_unet_volume_zones", "mi_unet_volume_zones_host", "mi_unet_volume_zones_run_features", "mi_unet_volume_zones_zone_features",
    "mi_unet_volume_nbhood", "mi_unet_volume_nbhood_host", "mi_unet_volume_nbhood_derive",
]


class Config(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("in_ch", C.c_int), ("base", C.c_int), ("levels", C.c_int),
                ("classes", C.c_int), ("max_batch", C.c_int), ("device", C.c_int), ("conv_algo", C.c_int)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kernel", C.c_char * 32), ("flops", C.c_double), ("bytes", C.c_double),
                ("ms", C.c_float)]


class LayerInfo(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kernel", C.c_char * 32), ("kind", C.c_int), ("in_h", C.c_int), ("in_w", C.c_int),
                ("in_c", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int), ("out_c", C.c_int), ("in_bits", C.c_int),
                ("out_bits", C.c_int), ("pooled", C.c_int), ("fused_head", C.c_int), ("skipped", C.c_int), ("fused_first", C.c_int)]

    KINDS = ("first", "conv3x3", "convT2x2", "maxpool", "head", "upsample2x")

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["name"], d["kernel"], d["kind"] = self.name.decode(), self.kernel.decode(), self.KINDS[self.kind]
        return d


class DebugLayout(C.Structure):
    _fields_ = [("ldc", C.c_int), ("ldo", C.c_int), ("co_off", C.c_int), ("pool_ld", C.c_int), ("guard_bytes", C.c_longlong)]


class DebugStridedInfo(C.Structure):
    _fields_ = [("elem_bytes", C.c_int), ("out_bytes", C.c_ulonglong), ("pool_bytes", C.c_ulonglong), ("kernel", C.c_char * 32)]


class TileBlend(C.Structure):
    _fields_ = [("mode", C.c_int), ("sigma_scale", C.c_float), ("mirror", C.c_int)]


class Target(C.Structure):
    _fields_ = [("cls", C.c_int), ("min_area_frac", C.c_float)]


class Morph(C.Structure):
    _fields_ = [("shape", C.c_int), ("open_r", C.c_int), ("close_r", C.c_int)]


class Window(C.Structure):
    _fields_ = [("mode", C.c_int), ("clip_lo_ppm", C.c_int), ("clip_hi_ppm", C.c_int), ("lo", C.c_int), ("hi", C.c_int)]


class Region(C.Structure):
    """mi_unet_region: 96 bytes, eight int32 then eight int64; REGION_DTYPE is the same layout for numpy"""
    _fields_ = [("area", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("imin", C.c_int32),
                ("imax", C.c_int32), ("channel", C.c_int32), ("edges", C.c_int64), ("sx", C.c_int64), ("sy", C.c_int64),
                ("sxx", C.c_int64), ("syy", C.c_int64), ("sxy", C.c_int64), ("si", C.c_int64), ("sii", C.c_int64)]


REGION_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in Region._fields_])


class Measure(C.Structure):
    _fields_ = [("on", C.c_int), ("channel", C.c_int)]


class RegionShape(C.Structure):
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("mean", C.c_double), ("std", C.c_double), ("major", C.c_double),
                ("minor", C.c_double), ("theta", C.c_double)]


class ScoreDir(C.Structure):
    """mi_unet_score_dir: 32 bytes"""
    _fields_ = [("n", C.c_int32), ("max_d2", C.c_int32), ("q_d2", C.c_int32), ("reserved", C.c_int32), ("sum_d2", C.c_int64),
                ("sum_d_q16", C.c_int64)]


class Score(C.Structure):
    """mi_unet_score: 88 bytes; SCORE_DTYPE is the same layout for numpy (a_to_t, t_to_a are nested records)"""
    _fields_ = [("tp", C.c_int32), ("fp", C.c_int32), ("fn", C.c_int32), ("q_d2_sym", C.c_int32), ("value", C.c_int32),
                ("quantile_ppm", C.c_int32), ("a_to_t", ScoreDir), ("t_to_a", ScoreDir)]


SCORE_DIR_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in ScoreDir._fields_])
SCORE_DTYPE = np.dtype([(n, SCORE_DIR_DTYPE if t is ScoreDir else np.int32) for n, t in Score._fields_])
SCORE_MAX_VALUES = 8
SCORE_MAX_CLASSES = 16


class ScoreOpts(C.Structure):
    _fields_ = [("quantile_ppm", C.c_int), ("classes", C.c_int)]


class ScoreMetrics(C.Structure):
    _fields_ = [("dice", C.c_double), ("iou", C.c_double), ("precision", C.c_double), ("recall", C.c_double), ("hd", C.c_double),
                ("hd_q", C.c_double), ("assd", C.c_double), ("rmsd", C.c_double)]


def _score_call(fn, head, pred, truth, values, quantile_ppm, classes):
    """mi_unet_score_labels (head = (handle,)) or its host form (head = ()): pred, truth u8 [B,H,W] (or [H,W]) -> SCORE_DTYPE
    [B, n], and (confusion int64 [B, classes, classes], skipped int64 [B]) behind it when classes > 0.  The library checks the values."""
    pred, truth = np.ascontiguousarray(pred, np.uint8), np.ascontiguousarray(truth, np.uint8)
    if pred.ndim == 2:
        pred, truth = pred[None], truth[None]
    if pred.ndim != 3 or pred.shape != truth.shape:
        raise ValueError(f"pred {pred.shape} and truth {truth.shape} must be two u8 [B,H,W] arrays of one shape")
    b, hh, ww = pred.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    scores = np.zeros((b, max(vals.size, 1)), SCORE_DTYPE)
    conf = np.zeros((b, classes, classes), np.int64) if classes > 0 else None
    skipped = np.zeros(b, np.int64) if classes > 0 else None
    _check(fn(*head, _ptr(pred), _ptr(truth), b, hh, ww, _ptr(vals), vals.size, C.byref(ScoreOpts(int(quantile_ppm), int(classes))),
              _ptr(scores), _ptr(conf), _ptr(skipped)))
    return (scores, conf, skipped) if classes > 0 else scores


SCORE_VOLUME_MAX_SIDE = 8192


def _score_volume_call(fn, head, pred, truth, values, spacing_units, quantile_ppm, classes):
    """mi_unet_score_volume (head = (handle,)) or its host form (head = ()): pred, truth u8 [D,H,W], spacing_units (ux, uy, uz) ->
    SCORE_DTYPE [n], and (confusion int64 [classes, classes], skipped int64 [1]) behind it when classes > 0.  The library checks the
    values."""
    pred, truth = np.ascontiguousarray(pred, np.uint8), np.ascontiguousarray(truth, np.uint8)
    if pred.ndim != 3 or pred.shape != truth.shape:
        raise ValueError(f"pred {pred.shape} and truth {truth.shape} must be two u8 [D,H,W] arrays of one shape")
    d, hh, ww = pred.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    units = np.ascontiguousarray(spacing_units, np.int32).reshape(-1)
    if units.size != 3:
        raise ValueError("spacing_units holds three integers: x, y, z")
    scores = np.zeros(max(vals.size, 1), SCORE_DTYPE)
    conf = np.zeros((classes, classes), np.int64) if classes > 0 else None
    skipped = np.zeros(1, np.int64) if classes > 0 else None
    _check(fn(*head, _ptr(pred), _ptr(truth), d, hh, ww, _ptr(vals), vals.size, _ptr(units), C.byref(ScoreOpts(int(quantile_ppm), int(classes))),
              _ptr(scores), _ptr(conf), _ptr(skipped)))
    return (scores, conf, skipped) if classes > 0 else scores


class VComp(C.Structure):
    """mi_unet_vcomp: 88 bytes, ten int32 then six int64; VCOMP_DTYPE is the same layout for numpy"""
    _fields_ = [("voxels", C.c_int32), ("first", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("z0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32), ("z1", C.c_int32), ("kept", C.c_int32), ("value", C.c_int32), ("faces_x", C.c_int64),
                ("faces_y", C.c_int64), ("faces_z", C.c_int64), ("sx", C.c_int64), ("sy", C.c_int64), ("sz", C.c_int64)]


VCOMP_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in VComp._fields_])
VOLUME_MAX_VALUES = 8
VOLUME_MAX_TABLE = 4096


class VolumeOpts(C.Structure):
    _fields_ = [("connectivity", C.c_int), ("min_voxels", C.c_int), ("keep_largest", C.c_int)]


class VCompMetrics(C.Structure):
    _fields_ = [("volume_mm3", C.c_double), ("surface_mm2", C.c_double), ("cx_mm", C.c_double), ("cy_mm", C.c_double),
                ("cz_mm", C.c_double), ("extent_x_mm", C.c_double), ("extent_y_mm", C.c_double), ("extent_z_mm", C.c_double)]


def _volume_call(fn, head, masks, values, connectivity, min_voxels, keep_largest, cap, want_ids):
    """mi_unet_volume_components (head = (handle,)) or its host form (head = ()): masks u8 [D,H,W] (or [H,W]: one slice) ->
    (out u8 [n,D,H,W], table VCOMP_DTYPE [n, cap], found int32 [n], kept int32 [n], ids int32 [n,D,H,W] or None).  The library
    checks the values."""
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.ndim == 2:
        masks = masks[None]
    if masks.ndim != 3:
        raise ValueError(f"masks {masks.shape} must be one u8 [D,H,W] array")
    d, hh, ww = masks.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    n = max(vals.size, 1)
    out = np.zeros((n, d, hh, ww), np.uint8)
    ids = np.zeros((n, d, hh, ww), np.int32) if want_ids else None
    table = np.zeros((n, max(int(cap), 1)), VCOMP_DTYPE)
    found, kept = np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(fn(*head, _ptr(masks), d, hh, ww, _ptr(vals), vals.size, C.byref(VolumeOpts(int(connectivity), int(min_voxels), int(keep_largest))),
              _ptr(out), _ptr(ids), _ptr(table), int(cap), _ptr(found), _ptr(kept)))
    return out, table, found, kept, ids


class VPiece(C.Structure):
    """mi_unet_vpiece: 40 bytes, two int32 then four int64; VPIECE_DTYPE is the same layout for numpy"""
    _fields_ = [("core_first", C.c_int32), ("core_voxels", C.c_int32), ("reach", C.c_int64), ("cut_x", C.c_int64), ("cut_y", C.c_int64),
                ("cut_z", C.c_int64)]


class VSplitStat(C.Structure):
    """mi_unet_vsplit_stat: 64 bytes, eight int64; VSPLIT_STAT_DTYPE is the same layout for numpy"""
    _fields_ = [(n, C.c_int64) for n in ("value", "in_voxels", "core_voxels", "cores", "cores_kept", "pieces", "coreless", "max_reach")]


VPIECE_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in VPiece._fields_])
VSPLIT_STAT_DTYPE = np.dtype([(n, np.int64) for n, _ in VSplitStat._fields_])


class VSplitOpts(C.Structure):
    _fields_ = [("connectivity", C.c_int), ("neck_r", C.c_int), ("min_core", C.c_int)]


class VPieceMetrics(C.Structure):
    _fields_ = [("reach_mm", C.c_double), ("cut_mm2", C.c_double)]


def _volume_split_call(fn, head, masks, values, units, connectivity, neck_r, min_core, cap, want_ids):
    """mi_unet_volume_split (head = (handle,)) or its host form (head = ()): masks u8 [D,H,W] (or [H,W]: one slice), units (ux, uy, uz)
    -> dict(table VCOMP_DTYPE [n, cap], info VPIECE_DTYPE [n, cap], found int32 [n], stats VSPLIT_STAT_DTYPE [n], ids int32 [n,D,H,W] or
    None, rounds int32 [n]).  The library checks the values."""
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.ndim == 2:
        masks = masks[None]
    if masks.ndim != 3:
        raise ValueError(f"masks {masks.shape} must be one u8 [D,H,W] array")
    d, hh, ww = masks.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    un = np.ascontiguousarray(units, np.int32).reshape(-1)
    if un.size != 3:
        raise ValueError("units holds three integers: x, y, z")
    n = max(vals.size, 1)
    ids = np.zeros((n, d, hh, ww), np.int32) if want_ids else None
    table = np.zeros((n, max(int(cap), 1)), VCOMP_DTYPE)
    info = np.zeros((n, max(int(cap), 1)), VPIECE_DTYPE)
    found, rounds = np.zeros(n, np.int32), np.zeros(n, np.int32)
    stats = np.zeros(n, VSPLIT_STAT_DTYPE)
    _check(fn(*head, _ptr(masks), d, hh, ww, _ptr(vals), vals.size, _ptr(un), C.byref(VSplitOpts(int(connectivity), int(neck_r), int(min_core))),
              _ptr(ids), _ptr(table), _ptr(info), int(cap), _ptr(found), _ptr(stats), _ptr(rounds)))
    return dict(table=table, info=info, found=found, stats=stats, ids=ids, rounds=rounds)


class VSkel(C.Structure):
    """mi_unet_vskel: 112 bytes, thirteen int64 then two int32; VSKEL_DTYPE is the same layout for numpy"""
    _fields_ = [(n, C.c_int64) for n in ("voxels_in", "voxels", "ends", "isolated", "junctions")] + [("links", C.c_int64 * 7), ("r2_sum", C.c_int64),
                                                                                                    ("r2_min", C.c_int32), ("r2_max", C.c_int32)]


VSKEL_DTYPE = np.dtype([(n, np.int64) for n in ("voxels_in", "voxels", "ends", "isolated", "junctions")] +
                       [("links", np.int64, (7,)), ("r2_sum", np.int64), ("r2_min", np.int32), ("r2_max", np.int32)])


class VSkelOpts(C.Structure):
    _fields_ = [("max_passes", C.c_int), ("radius", C.c_int)]


class VSkelInfo(C.Structure):
    _fields_ = [("deleted", C.c_int64), ("passes", C.c_int32), ("stable", C.c_int32)]


class VSkelMetrics(C.Structure):
    _fields_ = [("length_mm", C.c_double), ("radius_min_mm", C.c_double), ("radius_max_mm", C.c_double), ("radius_rms_mm", C.c_double),
                ("loops", C.c_int64)]


def _volume_skeleton_call(fn, head, ids, m, units, max_passes, radius, want_ids, want_r2):
    """mi_unet_volume_skeleton (head = (handle,)) or its host form (head = ()): ids int32 [D,H,W] (or [H,W]: one slice), units (ux, uy, uz)
    -> dict(table VSKEL_DTYPE [m], ids int32 [D,H,W] or None, r2 int32 [D,H,W] or None, passes, deleted, stable).  The library checks m
    and the units."""
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.ndim == 2:
        ids = ids[None]
    if ids.ndim != 3:
        raise ValueError(f"ids {ids.shape} must be one int32 [D,H,W] array")
    d, hh, ww = ids.shape
    un = np.ascontiguousarray(units, np.int32).reshape(-1)
    if un.size != 3:
        raise ValueError("units holds three integers: x, y, z")
    out = np.zeros((d, hh, ww), np.int32) if want_ids else None
    r2 = np.zeros((d, hh, ww), np.int32) if want_r2 else None
    table = np.zeros(max(int(m), 1), VSKEL_DTYPE)
    info = VSkelInfo()
    _check(fn(*head, _ptr(ids), d, hh, ww, int(m), _ptr(un), C.byref(VSkelOpts(int(max_passes), int(radius))), _ptr(out), _ptr(r2), _ptr(table),
              C.byref(info)))
    return dict(table=table, ids=out, r2=r2, passes=int(info.passes), deleted=int(info.deleted), stable=int(info.stable))


SKELETON_CODE_WORDS = 1 << 21      # 2^26 neighbourhood codes, 32 to a word


class VBranch(C.Structure):
    """mi_unet_vbranch: 88 bytes, four int64 then fourteen int32; VBRANCH_DTYPE is the same layout for numpy"""
    _fields_ = [(n, C.c_int64) for n in ("first", "att_lo", "att_hi", "r2_sum")] + [(n, C.c_int32) for n in ("id", "kind", "node_a", "node_b", "voxels")] + [
        ("links", C.c_int32 * 7), ("r2_min", C.c_int32), ("r2_max", C.c_int32)]


VBRANCH_DTYPE = np.dtype([(n, np.int64) for n in ("first", "att_lo", "att_hi", "r2_sum")] + [(n, np.int32) for n in ("id", "kind", "node_a", "node_b", "voxels")] +
                         [("links", np.int32, (7,)), ("r2_min", np.int32), ("r2_max", np.int32)])
VNODE_DTYPE = np.dtype([(n, np.int64) for n in ("first", "sz", "sy", "sx")] + [(n, np.int32) for n in ("id", "kind", "voxels", "degree", "r2_min", "r2_max")])
VGRAPH_DTYPE = np.dtype([(n, np.int64) for n in ("nodes", "ends", "junction_nodes", "isolated", "junction_voxels", "branches", "closed")] +
                        [("links", np.int64, (7,)), ("pruned_spurs", np.int64), ("pruned_voxels", np.int64)])
VBRANCH_MAX_ROWS = 1 << 20         # MI_UNET_VBRANCH_MAX_ROWS
VBRANCH_KINDS = ("path", "closed", "zero-voxel")
VNODE_KINDS = ("isolated", "end", "junction")


class VGraph(C.Structure):
    """mi_unet_vgraph: 128 bytes, sixteen int64; VGRAPH_DTYPE is the same layout for numpy"""
    _fields_ = [(n, C.c_int64) for n in ("nodes", "ends", "junction_nodes", "isolated", "junction_voxels", "branches", "closed")] + [
        ("links", C.c_int64 * 7), ("pruned_spurs", C.c_int64), ("pruned_voxels", C.c_int64)]


class VBranchOpts(C.Structure):
    _fields_ = [("prune_voxels", C.c_int), ("prune_rounds", C.c_int)]


class VBranchInfo(C.Structure):
    _fields_ = [("found_nodes", C.c_int64), ("found_branches", C.c_int64), ("rounds", C.c_int32), ("stable", C.c_int32)]


class VBranchMetrics(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("length_mm", "chord_mm", "tortuosity", "radius_min_mm", "radius_max_mm", "radius_rms_mm")]


class VGraphMetrics(C.Structure):
    _fields_ = [("length_mm", C.c_double), ("parts", C.c_int64), ("loops", C.c_int64)]


def _volume_branches_call(fn, head, ids, m, r2, units, prune_voxels, prune_rounds, cap_nodes, cap_branches, want_map, want_ids):
    """mi_unet_volume_branches (head = (handle,)) or its host form (head = ()): ids int32 [D,H,W] (or [H,W]: one slice) as
    volume_skeleton writes them, r2 int32 of the same shape or None -> dict(nodes VNODE_DTYPE [min(found, cap)], branches VBRANCH_DTYPE
    [min(found, cap)], graph VGRAPH_DTYPE [m], map int32 [D,H,W] or None, ids int32 [D,H,W] or None, found_nodes, found_branches, rounds,
    stable).  The library checks m, the units, the caps and the options."""
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.ndim == 2:
        ids = ids[None]
    if ids.ndim != 3:
        raise ValueError(f"ids {ids.shape} must be one int32 [D,H,W] array")
    d, hh, ww = ids.shape
    if r2 is not None:
        r2 = np.ascontiguousarray(r2, np.int32).reshape(-1)
        if r2.size != ids.size:
            raise ValueError("r2 has the shape of ids")
    un = np.ascontiguousarray(units, np.int32).reshape(-1)
    if un.size != 3:
        raise ValueError("units holds three integers: x, y, z")
    nodes = np.zeros(max(int(cap_nodes), 0), VNODE_DTYPE)
    branches = np.zeros(max(int(cap_branches), 0), VBRANCH_DTYPE)
    graph = np.zeros(max(int(m), 1), VGRAPH_DTYPE)
    vmap = np.zeros((d, hh, ww), np.int32) if want_map else None
    out = np.zeros((d, hh, ww), np.int32) if want_ids else None
    info = VBranchInfo()
    _check(fn(*head, _ptr(ids), _ptr(r2), d, hh, ww, int(m), _ptr(un), C.byref(VBranchOpts(int(prune_voxels), int(prune_rounds))),
              _ptr(nodes) if nodes.size else None, int(cap_nodes), _ptr(branches) if branches.size else None, int(cap_branches), _ptr(graph),
              _ptr(vmap), _ptr(out), C.byref(info)))
    return dict(nodes=nodes[:min(int(info.found_nodes), nodes.size)], branches=branches[:min(int(info.found_branches), branches.size)], graph=graph,
                map=vmap, ids=out, found_nodes=int(info.found_nodes), found_branches=int(info.found_branches), rounds=int(info.rounds),
                stable=int(info.stable))


class VCleanStat(C.Structure):
    """mi_unet_volume_clean_stat: 48 bytes, two int32 then five int64; VCLEAN_DTYPE is the same layout for numpy"""
    _fields_ = [("value", C.c_int32), ("reserved", C.c_int32), ("in_voxels", C.c_int64), ("filled", C.c_int64), ("closed", C.c_int64),
                ("opened", C.c_int64), ("out_voxels", C.c_int64)]


VCLEAN_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in VCleanStat._fields_])
VOLUME_CLEAN_MAX_R = 46340


class VolumeCleanOpts(C.Structure):
    _fields_ = [("fill", C.c_int), ("close_r", C.c_int), ("open_r", C.c_int)]


def _volume_clean_call(fn, head, masks, values, units, fill, close_r, open_r):
    """mi_unet_volume_clean (head = (handle,)) or its host form (head = ()): masks u8 [D,H,W] (or [H,W]: one slice), units (ux, uy, uz)
    -> (out u8 [n,D,H,W], stats VCLEAN_DTYPE [n]).  The library checks the values."""
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.ndim == 2:
        masks = masks[None]
    if masks.ndim != 3:
        raise ValueError(f"masks {masks.shape} must be one u8 [D,H,W] array")
    d, hh, ww = masks.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    un = np.ascontiguousarray(units, np.int32).reshape(-1)
    if un.size != 3:
        raise ValueError("units holds three integers: x, y, z")
    n = max(vals.size, 1)
    out = np.zeros((n, d, hh, ww), np.uint8)
    stats = np.zeros(n, VCLEAN_DTYPE)
    _check(fn(*head, _ptr(masks), d, hh, ww, _ptr(vals), vals.size, _ptr(un), C.byref(VolumeCleanOpts(int(fill), int(close_r), int(open_r))),
              _ptr(out), _ptr(stats)))
    return out, stats


class VInterpStat(C.Structure):
    """mi_unet_vinterp_stat: 40 bytes, five int64; VINTERP_DTYPE is the same layout for numpy"""
    _fields_ = [("in_voxels", C.c_int64), ("out_voxels", C.c_int64), ("mixed", C.c_int64), ("mixed_set", C.c_int64), ("ties", C.c_int64)]


VINTERP_DTYPE = np.dtype([(n, np.int64) for n, _ in VInterpStat._fields_])
VINTERP_MAX_FACTOR = 16
VINTERP_NONE = 2**31 - 1


def _volume_interp_call(fn, head, masks, values, units_xy, factor, intensity):
    """mi_unet_volume_interp (head = (handle,)) or its host form (head = ()): masks u8 [D,H,W] (or [H,W]: one slice), units_xy (ux, uy),
    factor k, intensity u16 [D,H,W] or None -> (out u8 [n,D',H,W], stats VINTERP_DTYPE [n][, intensity_out u16 [D',H,W]]) with
    D' = (D - 1) k + 1.  The library checks the values; an argument it refuses leaves D' at D."""
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.ndim == 2:
        masks = masks[None]
    if masks.ndim != 3:
        raise ValueError(f"masks {masks.shape} must be one u8 [D,H,W] array")
    d, hh, ww = masks.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    un = np.ascontiguousarray(units_xy, np.int32).reshape(-1)
    if un.size != 2:
        raise ValueError("units_xy holds two integers: x, y")
    if intensity is not None:
        intensity = np.ascontiguousarray(intensity, np.uint16)
        if intensity.shape != masks.shape:
            raise ValueError(f"intensity {intensity.shape} must have the shape of masks {masks.shape}")
    dp = max(volume_interp_slices(d, factor), d)
    n = max(vals.size, 1)
    out = np.zeros((n, dp, hh, ww), np.uint8)
    stats = np.zeros(n, VINTERP_DTYPE)
    iout = np.zeros((dp, hh, ww), np.uint16) if intensity is not None else None
    _check(fn(*head, _ptr(masks), d, hh, ww, _ptr(vals), vals.size, _ptr(un), int(factor), _ptr(intensity), _ptr(out), _ptr(iout), _ptr(stats)))
    return (out, stats) if intensity is None else (out, stats, iout)


class MeshVertex(C.Structure):
    """mi_unet_mesh_vertex: 16 bytes, three int32, three int8, one uint8; MESH_VERTEX_DTYPE is the same layout for numpy"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("z", C.c_int32), ("ox", C.c_int8), ("oy", C.c_int8), ("oz", C.c_int8), ("n", C.c_uint8)]


class MeshStat(C.Structure):
    """mi_unet_mesh_stat: 48 bytes, two int32 then five int64; MESH_STAT_DTYPE is the same layout for numpy"""
    _fields_ = [("value", C.c_int32), ("placement", C.c_int32), ("quads", C.c_int64), ("verts", C.c_int64), ("quads_x", C.c_int64),
                ("quads_y", C.c_int64), ("quads_z", C.c_int64)]


class MeshMetrics(C.Structure):
    _fields_ = [("area_mm2", C.c_double), ("volume_mm3", C.c_double)]


MESH_VERTEX_DTYPE = np.dtype([(n, {C.c_int32: np.int32, C.c_int8: np.int8, C.c_uint8: np.uint8}[t]) for n, t in MeshVertex._fields_])
MESH_STAT_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in MeshStat._fields_])
MESH_PLACEMENTS = {"faces": 0, "nets": 1}


def _volume_mesh_call(fn, head, masks, values, placement, cap, raw=False):
    """mi_unet_volume_mesh (head = (handle,)) or its host form (head = ()): masks u8 [D,H,W] (or [H,W]: one slice), placement by name
    (MESH_PLACEMENTS) or as the raw C value, cap = None (a counting call, then one sized by the largest counts), one int for both caps
    or (cap_verts, cap_quads) -> ([(verts MESH_VERTEX_DTYPE [V], quads int32 [Q, 4]) per value], stats MESH_STAT_DTYPE [n]), the
    arrays trimmed to min(count, cap); raw=True returns the untrimmed (verts [n, cap_verts], quads [n, cap_quads, 4], stats).  The
    library checks the values."""
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.ndim == 2:
        masks = masks[None]
    if masks.ndim != 3:
        raise ValueError(f"masks {masks.shape} must be one u8 [D,H,W] array")
    d, hh, ww = masks.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    n = max(vals.size, 1)
    pl = MESH_PLACEMENTS[placement] if isinstance(placement, str) else int(placement)
    stats = np.zeros(n, MESH_STAT_DTYPE)
    if cap is None:
        _check(fn(*head, _ptr(masks), d, hh, ww, _ptr(vals), vals.size, pl, None, 0, None, 0, _ptr(stats)))
        cap = (int(stats["verts"].max()), int(stats["quads"].max()))
    cap_v, cap_q = (int(cap), int(cap)) if np.isscalar(cap) else (int(cap[0]), int(cap[1]))
    verts = np.zeros((n, max(cap_v, 0)), MESH_VERTEX_DTYPE)
    quads = np.zeros((n, max(cap_q, 0), 4), np.int32)
    _check(fn(*head, _ptr(masks), d, hh, ww, _ptr(vals), vals.size, pl, _ptr(verts) if cap_v else None, cap_v, _ptr(quads) if cap_q else None,
              cap_q, _ptr(stats)))
    if raw:
        return verts, quads, stats
    return [(verts[k, :min(int(stats[k]["verts"]), cap_v)].copy(), quads[k, :min(int(stats[k]["quads"]), cap_q)].copy()) for k in range(n)], stats


class VMeasure(C.Structure):
    """mi_unet_vmeasure: 128 bytes, ten int32 then eleven int64; VMEASURE_DTYPE is the same layout for numpy"""
    _fields_ = ([(n, C.c_int32) for n in ("voxels", "ends", "imin", "imax", "d2", "dp", "dq", "a_d2", "a_p", "a_q")] +
                [(n, C.c_int64) for n in ("sx", "sy", "sz", "sxx", "syy", "szz", "sxy", "sxz", "syz", "si", "sii")])


class VMeasureOpts(C.Structure):
    _fields_ = [("max_ends", C.c_int)]


class VMeasureShape(C.Structure):
    _fields_ = [("cx_mm", C.c_double), ("cy_mm", C.c_double), ("cz_mm", C.c_double), ("axis_mm", C.c_double * 3),
                ("axis_dir", (C.c_double * 3) * 3), ("mean", C.c_double), ("std", C.c_double), ("diameter_mm", C.c_double),
                ("axial_diameter_mm", C.c_double)]


VMEASURE_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in VMeasure._fields_])
VMEASURE_MAX_ENDS_LIMIT = 1 << 20
VMEASURE_DEFAULT_MAX_ENDS = 262144


def _ids_intensity(ids, intensity, optional=False):
    """ids as one contiguous int32 [D,H,W] array ([H,W] is one slice) and intensity as u16 of its shape (None stays None where optional)"""
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.ndim == 2:
        ids = ids[None]
    if ids.ndim != 3:
        raise ValueError(f"ids {ids.shape} must be one int32 [D,H,W] array")
    if intensity is not None or not optional:
        intensity = np.ascontiguousarray(intensity, np.uint16).reshape(ids.shape)
    return ids, intensity


def _table_rows(m, cells):
    """the rows to allocate for m components of `cells` cells each: one for a call that the library refuses (no need for the memory)"""
    rows = max(int(m), 1)
    return 1 if rows * cells > 2 * VTEX_MAX_CELLS else rows


class VSpatial(C.Structure):
    """mi_unet_vspatial: 168 bytes, eight int32, thirteen int64, then the four pair sums as doubles; VSPATIAL_DTYPE is the same layout
    for numpy"""
    _fields_ = ([(n, C.c_int32) for n in ("voxels", "searched", "imin", "imax", "centre", "reserved", "gp_at", "lp_at")] +
                [(n, C.c_int64) for n in ("sx", "sy", "sz", "si", "sii", "six", "siy", "siz", "gp_sum", "gp_n", "lp_sum", "lp_n", "pairs")] +
                [(n, C.c_double) for n in ("s0", "s1", "s2", "s3")])


class VSpatialOpts(C.Structure):
    _fields_ = [("max_voxels", C.c_int), ("peak_r", C.c_int)]


class VSpatialMetrics(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("cx_mm", "cy_mm", "cz_mm", "icx_mm", "icy_mm", "icz_mm", "com_shift_mm", "integrated_intensity",
                                          "local_peak", "global_peak", "morans_i", "gearys_c")]


VSPATIAL_DTYPE = np.dtype([(n, {C.c_int32: np.int32, C.c_int64: np.int64, C.c_double: np.float64}[t]) for n, t in VSpatial._fields_])
VSPATIAL_INT_BYTES = 8 * 4 + 13 * 8         # the integer part of an entry; the doubles follow
VSPATIAL_MAX_VOXELS_LIMIT = 1 << 20
VSPATIAL_DEFAULT_MAX_VOXELS = 1 << 17
VSPATIAL_MAX_BALL_ROWS = 4096
VSPATIAL_MAX_BALL_VOXELS = 1 << 23


def _volume_spatial_call(fn, head, ids, intensity, m, units, max_voxels, peak_r):
    """mi_unet_volume_spatial (head = (handle,)) or its host form (head = ()): ids int32 [D,H,W] (or [H,W]: one slice), intensity u16 of
    the same shape, m components, units = the spacing (ux, uy, uz) as integers, max_voxels = None (the library's default) or the cap
    of the pair sums, peak_r = the radius of the peak sphere in the spacing unit -> table VSPATIAL_DTYPE [m].  The library checks the
    values."""
    ids, intensity = _ids_intensity(ids, intensity)
    d, hh, ww = ids.shape
    un = np.ascontiguousarray(units, np.int32).reshape(-1)
    if un.size != 3:
        raise ValueError("units holds three integers: ux, uy, uz")
    table = np.zeros(max(int(m), 1), VSPATIAL_DTYPE)
    opts = C.byref(VSpatialOpts(VSPATIAL_DEFAULT_MAX_VOXELS if max_voxels is None else int(max_voxels), int(peak_r)))
    _check(fn(*head, _ptr(ids), _ptr(intensity), d, hh, ww, int(m), _ptr(un), opts, _ptr(table)))
    return table


def _volume_measure_call(fn, head, ids, intensity, m, units, max_ends):
    """mi_unet_volume_measure (head = (handle,)) or its host form (head = ()): ids int32 [D,H,W] (or [H,W]: one slice), intensity u16 of
    the same shape or None, m components, units = the spacing (ux, uy, uz) as integers, max_ends = None (the library's default) or the
    cap -> table VMEASURE_DTYPE [m].  The library checks the values."""
    ids, intensity = _ids_intensity(ids, intensity, optional=True)
    d, hh, ww = ids.shape
    un = np.ascontiguousarray(units, np.int32).reshape(-1)
    if un.size != 3:
        raise ValueError("units holds three integers: ux, uy, uz")
    table = np.zeros(max(int(m), 1), VMEASURE_DTYPE)
    opts = None if max_ends is None else C.byref(VMeasureOpts(int(max_ends)))
    _check(fn(*head, _ptr(ids), _ptr(intensity), d, hh, ww, int(m), _ptr(un), opts, _ptr(table)))
    return table


class VTextureOpts(C.Structure):
    """mi_unet_vtexture_opts; the default is { VTEX_COUNT, 32, 0, 1 }"""
    _fields_ = [("mode", C.c_int), ("levels", C.c_int), ("lo", C.c_int), ("width", C.c_int)]


class VTexture(C.Structure):
    """mi_unet_vtexture: 32 bytes, four int32 then two int64; VTEXTURE_DTYPE is the same layout for numpy"""
    _fields_ = ([(n, C.c_int32) for n in ("voxels", "imin", "imax", "levels_used")] + [(n, C.c_int64) for n in ("pairs", "pairs_axial")])


class VTextureFeatures(C.Structure):
    _fields_ = ([(n, C.c_double) for n in ("mean", "variance", "skewness", "kurtosis", "entropy", "uniformity")] +
                [(n, C.c_int32) for n in ("median", "p10", "p90", "mode")] +
                [(n, C.c_double) for n in ("joint_max", "joint_average", "joint_variance", "joint_entropy", "contrast", "dissimilarity",
                                           "inverse_difference", "inverse_difference_moment", "angular_second_moment", "correlation")])


VTEXTURE_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in VTexture._fields_])
VTEX_MODES = {"count": 0, "width": 1}       # MI_UNET_VTEX_COUNT, MI_UNET_VTEX_WIDTH
VTEX_MAX_LEVELS = 64
VTEX_MAX_CELLS = 1 << 22


def _volume_texture_call(fn, head, ids, intensity, m, levels, mode, lo, width, want):
    """mi_unet_volume_texture (head = (handle,)) or its host form (head = ()): ids int32 [D,H,W] (or [H,W]: one slice), intensity u16 of
    the same shape, m components, levels / mode ("count", "width" or the number) / lo / width = the options, want = which of "glcm" and
    "axial" to compute -> (table VTEXTURE_DTYPE [m], hist u32 [m, L], glcm u32 [m, L, L] or None, glcm_axial or None).  The library
    checks the values."""
    ids, intensity = _ids_intensity(ids, intensity)
    d, hh, ww = ids.shape
    lv = min(max(int(levels), 1), VTEX_MAX_LEVELS)
    rows = _table_rows(m, lv * lv)
    table = np.zeros(rows, VTEXTURE_DTYPE)
    hist = np.zeros((rows, lv), np.uint32)
    glcm = np.zeros((rows, lv, lv), np.uint32) if "glcm" in want else None
    axial = np.zeros((rows, lv, lv), np.uint32) if "axial" in want else None
    opts = VTextureOpts(int(VTEX_MODES.get(mode, mode)), int(levels), int(lo), int(width))
    _check(fn(*head, _ptr(ids), _ptr(intensity), d, hh, ww, int(m), C.byref(opts), _ptr(table), _ptr(hist), _ptr(glcm), _ptr(axial)))
    return table, hist, glcm, axial


class VZonesOpts(C.Structure):
    """mi_unet_vzones_opts; the default is { VTEX_COUNT, 32, 0, 1, 32 }"""
    _fields_ = [("mode", C.c_int), ("levels", C.c_int), ("lo", C.c_int), ("width", C.c_int), ("max_run", C.c_int)]


class VZones(C.Structure):
    """mi_unet_vzones: 56 bytes, six int32 then four int64; VZONES_DTYPE is the same layout for numpy"""
    _fields_ = ([(n, C.c_int32) for n in ("voxels", "imin", "imax", "longest_run", "zones", "largest_zone")] +
                [(n, C.c_int64) for n in ("runs", "runs_axial", "clamped", "clamped_axial")])


class VZone(C.Structure):
    """mi_unet_vzone: 16 bytes; VZONE_DTYPE is the same layout for numpy"""
    _fields_ = [(n, C.c_int32) for n in ("first", "component", "level", "size")]


class VZoneFeatures(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("short_emphasis", "long_emphasis", "low_grey_emphasis", "high_grey_emphasis", "short_low", "short_high",
                                          "long_low", "long_high", "grey_nonuniformity", "grey_nonuniformity_norm", "size_nonuniformity",
                                          "size_nonuniformity_norm", "percentage", "grey_variance", "size_variance", "entropy")]


VZONES_DTYPE = np.dtype([(n, np.int32 if t is C.c_int32 else np.int64) for n, t in VZones._fields_])
VZONE_DTYPE = np.dtype([(n, np.int32) for n, _ in VZone._fields_])
VZONES_MAX_RUN = 8192
VZONES_MAX_CAP = 1 << 24


def _volume_zones_call(fn, head, ids, intensity, m, levels, mode, lo, width, max_run, want_runs, want_axial, cap):
    """mi_unet_volume_zones (head = (handle,)) or its host form (head = ()): ids int32 [D,H,W] (or [H,W]: one slice), intensity u16 of
    the same shape, m components, levels / mode ("count", "width" or the number) / lo / width / max_run = the options, want_runs and
    want_axial = which tables to compute, cap = the length of the zone list (None: a record per voxel, at most 2^24; 0: no zone half)
    -> (table VZONES_DTYPE [m], rlm u32 [m, L, R] or None, rlm_axial or None, zones VZONE_DTYPE [cap] or None, found or None).  The
    library checks the values."""
    ids, intensity = _ids_intensity(ids, intensity)
    d, hh, ww = ids.shape
    lv, rn = min(max(int(levels), 1), VTEX_MAX_LEVELS), min(max(int(max_run), 1), VZONES_MAX_RUN)
    rows = _table_rows(m, lv * rn)
    table = np.zeros(rows, VZONES_DTYPE)
    rlm = np.zeros((rows, lv, rn), np.uint32) if want_runs else None
    axial = np.zeros((rows, lv, rn), np.uint32) if want_axial else None
    if cap is None:
        cap = min(max(ids.size, 1), VZONES_MAX_CAP)
    cap = int(cap)
    zones = np.zeros(min(max(cap, 1), VZONES_MAX_CAP), VZONE_DTYPE) if cap else None
    found = C.c_int(0)
    opts = VZonesOpts(int(VTEX_MODES.get(mode, mode)), int(levels), int(lo), int(width), int(max_run))
    _check(fn(*head, _ptr(ids), _ptr(intensity), d, hh, ww, int(m), C.byref(opts), _ptr(table), _ptr(rlm), _ptr(axial), _ptr(zones), cap,
              C.byref(found) if cap else None))
    return table, rlm, axial, zones, (found.value if cap else None)


class VNbhoodOpts(C.Structure):
    """mi_unet_vnbhood_opts; the default is { VTEX_COUNT, 32, 0, 1, 0, 32 }"""
    _fields_ = [("mode", C.c_int), ("levels", C.c_int), ("lo", C.c_int), ("width", C.c_int), ("alpha", C.c_int), ("max_dist", C.c_int)]


class VNbhood(C.Structure):
    """mi_unet_vnbhood: 44 bytes, eleven int32; VNBHOOD_DTYPE is the same layout for numpy"""
    _fields_ = [(n, C.c_int32) for n in ("voxels", "imin", "imax", "valid", "valid_axial", "zones", "deepest", "deepest_axial", "clamped",
                                         "clamped_axial", "dependence_max")]


VNBHOOD_TABLES = ("ngt_count", "ngt_diff", "dep", "ngt_count_axial", "ngt_diff_axial", "dep_axial", "dzm", "dzm_axial")


class VNbhoodOut(C.Structure):
    """mi_unet_vnbhood_out: the eight table pointers of a call, or the row pointers of one component"""
    _fields_ = [(n, C.c_void_p) for n in VNBHOOD_TABLES]


class VNbhoodFeatures(C.Structure):
    _fields_ = ([(n, C.c_double) for n in ("coarseness", "contrast", "busyness", "complexity", "strength")] + [("ngldm", VZoneFeatures)] +
                [("dependence_energy", C.c_double), ("gldzm", VZoneFeatures)])


VNBHOOD_DTYPE = np.dtype([(n, np.int32) for n, _ in VNbhood._fields_])
VNBHOOD_MAX_DIST = 4096
VNBHOOD_WANT = ("ngt", "dep", "ngt_axial", "dep_axial", "dzm", "dzm_axial")


def _vnbhood_shapes(rows, lv, dm):
    return {"ngt_count": ((rows, lv, 27), np.uint32), "ngt_diff": ((rows, lv, 27), np.uint64), "dep": ((rows, lv, 27), np.uint32),
            "ngt_count_axial": ((rows, lv, 9), np.uint32), "ngt_diff_axial": ((rows, lv, 9), np.uint64), "dep_axial": ((rows, lv, 9), np.uint32),
            "dzm": ((rows, lv, dm), np.uint32), "dzm_axial": ((rows, lv, dm), np.uint32)}


def _volume_nbhood_call(fn, head, ids, intensity, m, levels, mode, lo, width, alpha, max_dist, want):
    """mi_unet_volume_nbhood (head = (handle,)) or its host form (head = ()): ids int32 [D,H,W] (or [H,W]: one slice), intensity u16 of
    the same shape, m components, levels / mode ("count", "width" or the number) / lo / width / alpha / max_dist = the options, want =
    which of VNBHOOD_WANT to compute ("ngt" and "ngt_axial" are a count and a diff table each) -> (table VNBHOOD_DTYPE [m], dict over
    VNBHOOD_TABLES: u32 / u64 [m, L, 27 | 9 | max_dist], or None for a table that was not asked for).  The library checks the values."""
    ids, intensity = _ids_intensity(ids, intensity)
    unknown = set(want) - set(VNBHOOD_WANT)
    if unknown:
        raise ValueError(f"want {sorted(unknown)} is not among {VNBHOOD_WANT}")
    d, hh, ww = ids.shape
    lv, dm = min(max(int(levels), 1), VTEX_MAX_LEVELS), min(max(int(max_dist), 1), VNBHOOD_MAX_DIST)
    rows = _table_rows(m, lv * max(lv, 32, dm))
    table = np.zeros(rows, VNBHOOD_DTYPE)
    asked = {"ngt_count": "ngt", "ngt_diff": "ngt", "dep": "dep", "ngt_count_axial": "ngt_axial", "ngt_diff_axial": "ngt_axial",
             "dep_axial": "dep_axial", "dzm": "dzm", "dzm_axial": "dzm_axial"}
    tables = {n: (np.zeros(shape, dt) if asked[n] in want else None) for n, (shape, dt) in _vnbhood_shapes(rows, lv, dm).items()}
    out = VNbhoodOut(*[None if tables[n] is None else tables[n].ctypes.data for n in VNBHOOD_TABLES])
    opts = VNbhoodOpts(int(VTEX_MODES.get(mode, mode)), int(levels), int(lo), int(width), int(alpha), int(max_dist))
    _check(fn(*head, _ptr(ids), _ptr(intensity), d, hh, ww, int(m), C.byref(opts), _ptr(table), C.byref(out)))
    return table, tables


class VMatchCounts(C.Structure):
    _fields_ = [("tp", C.c_int32), ("fp", C.c_int32), ("fn", C.c_int32)]


class VMatchScores(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("precision", "recall", "f1", "sq", "rq", "pq", "mean_dice")]


VMATCH_SIDE_DTYPE = np.dtype([(n, np.int32) for n in ("voxels", "covered", "partners", "best", "best_voxels")])   # mi_unet_vmatch_side
VMATCH_PAIR_DTYPE = np.dtype([(n, np.int32) for n in ("p", "t", "voxels")])                                       # mi_unet_vmatch_pair


def _volume_match_call(fn, head, pred_ids, truth_ids, mp, mt, cap):
    """mi_unet_volume_match (head = (handle,)) or its host form (head = ()): pred_ids, truth_ids int32 [D,H,W] (or [H,W]: one slice) of
    one shape, mp and mt components, cap = the length of the pair list -> (pred_side VMATCH_SIDE_DTYPE [mp], truth_side [mt], pairs
    VMATCH_PAIR_DTYPE [cap], found).  The library checks the values."""
    pred_ids = np.ascontiguousarray(pred_ids, np.int32)
    truth_ids = np.ascontiguousarray(truth_ids, np.int32)
    if pred_ids.ndim == 2:
        pred_ids = pred_ids[None]
    if truth_ids.ndim == 2:
        truth_ids = truth_ids[None]
    if pred_ids.ndim != 3 or truth_ids.shape != pred_ids.shape:
        raise ValueError(f"pred_ids {pred_ids.shape} and truth_ids {truth_ids.shape} must be two int32 [D,H,W] arrays of one shape")
    d, hh, ww = pred_ids.shape
    ps = np.zeros(max(int(mp), 1), VMATCH_SIDE_DTYPE)
    ts = np.zeros(max(int(mt), 1), VMATCH_SIDE_DTYPE)
    pairs = np.zeros(max(int(cap), 1), VMATCH_PAIR_DTYPE)
    found = C.c_int(0)
    _check(fn(*head, _ptr(pred_ids), _ptr(truth_ids), d, hh, ww, int(mp), int(mt), int(cap), _ptr(ps), _ptr(ts), _ptr(pairs), C.byref(found)))
    return ps, ts, pairs, found.value


def _last_regions(fn, handle):
    """(regions REGION_DTYPE [planes, cap_contours], counts int32 [planes]) of mi_unet_last_regions or its group form"""
    planes, cap = C.c_int(), C.c_int()
    _check(fn(handle, None, None, 0, C.byref(planes), C.byref(cap)))
    regions = np.zeros((planes.value, cap.value), REGION_DTYPE)
    counts = np.zeros(planes.value, np.int32)
    _check(fn(handle, _ptr(regions), _ptr(counts), planes.value, C.byref(planes), C.byref(cap)))
    return regions, counts


WINDOW_MODES = {"minmax": 0, "percentile": 1, "fixed": 2}


def _window(mode, clip_lo_ppm=0, clip_hi_ppm=0, lo=0, hi=65535):
    """mode by name (WINDOW_MODES) or as the raw C value, which the library checks; None -> None (restores the default)"""
    if mode is None:
        return None
    return C.byref(Window(WINDOW_MODES[mode] if isinstance(mode, str) else int(mode), int(clip_lo_ppm), int(clip_hi_ppm), int(lo), int(hi)))


MAX_TARGETS = 5
DEFAULT_TARGETS = [(2, 0.06)]
MORPH_SHAPES = {"rect": 0, "disc": 1}
MORPH_MAX_R = 31
DEFAULT_MORPH = [("rect", 1, 0)]


def _morph_array(morph):
    """[(shape, open_r, close_r), ...], shape by name (MORPH_SHAPES) or as the raw C value -> (Morph array or None, n); None restores the
    default.  The library checks the values."""
    if morph is None:
        return None, 0
    morph = list(morph)
    return (Morph * max(len(morph), 1))(*[Morph(MORPH_SHAPES[s] if isinstance(s, str) else int(s), int(o), int(c)) for s, o, c in morph]), len(morph)


def _target_array(targets):
    """[(cls, min_area_frac), ...] -> (Target array or None, n); None restores the default.  The library checks the values."""
    if targets is None:
        return None, 0
    targets = list(targets)
    return (Target * max(len(targets), 1))(*[Target(int(c), float(f)) for c, f in targets]), len(targets)


BLEND_MODES = {"owner": 0, "constant": 1, "gaussian": 2}
MIRRORS = {"": 0, "x": 1, "y": 2, "xy": 3}


def _tile_blend(mode, sigma_scale, mirror) -> TileBlend:
    """mode / mirror by name (BLEND_MODES, MIRRORS) or as the raw C values, which the library checks"""
    return TileBlend(BLEND_MODES[mode] if isinstance(mode, str) else int(mode), float(sigma_scale),
                     MIRRORS[mirror] if isinstance(mirror, str) else int(mirror))


class MiUnetError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmiunet error {code}: {msg}")
        self.code = code


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(make -C unet-medical-image-contour-segmentation-cpp_amd)")
        L = C.CDLL(LIB_PATH)
        L.mi_unet_last_error.restype = C.c_char_p
        L.mi_unet_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
        L.mi_unet_load_weights.argtypes = [C.c_void_p, C.c_char_p]
        L.mi_unet_load_weights_from_memory.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.mi_unet_infer_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mi_unet_infer_u8_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mi_unet_infer_raw16.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_set_postprocess.argtypes = [C.c_void_p, C.c_int]
        L.mi_unet_postprocess_masks.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_extract_contours.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_segment_raw16.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.mi_unet_sync.argtypes = [C.c_void_p]
        L.mi_unet_timer_begin.argtypes = [C.c_void_p]
        L.mi_unet_timer_end.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.mi_unet_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.mi_unet_get_kernel_stats.argtypes = [C.c_void_p, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int)]
        L.mi_unet_layer_debug.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.mi_unet_layer_debug_strided.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DebugLayout), C.c_void_p,
                                                  C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(DebugStridedInfo)]
        L.mi_unet_destroy.argtypes = [C.c_void_p]
        L.mi_unet_destroy.restype = None
        L.mi_unet_default_config.argtypes = [C.POINTER(Config)]
        L.mi_unet_default_config.restype = None
        L.mi_unet_clone.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.mi_unet_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        L.mi_unet_host_free.argtypes = [C.c_void_p]
        L.mi_unet_host_free.restype = None
        L.mi_unet_numeric_guard.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.mi_unet_numeric_guard.restype = C.c_char_p
        L.mi_unet_last_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.mi_unet_debug_layer_count.argtypes = [C.c_void_p]
        L.mi_unet_debug_layer_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(LayerInfo)]
        L.mi_unet_debug_capture.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(LayerInfo)]
        L.mi_unet_group_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        L.mi_unet_group_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mi_unet_group_size.argtypes = [C.c_void_p]
        L.mi_unet_group_handle.argtypes = [C.c_void_p, C.c_int]
        L.mi_unet_group_handle.restype = C.c_void_p
        L.mi_unet_group_load_weights.argtypes = [C.c_void_p, C.c_char_p]
        L.mi_unet_group_load_weights_from_memory.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.mi_unet_group_set_gather.argtypes = [C.c_void_p, C.c_int]
        L.mi_unet_group_set_postprocess.argtypes = [C.c_void_p, C.c_int]
        L.mi_unet_group_weight_transport.argtypes = [C.c_void_p]
        L.mi_unet_group_weight_transport.restype = C.c_char_p
        L.mi_unet_group_gather.argtypes = [C.c_void_p]
        L.mi_unet_group_infer_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mi_unet_group_infer_raw16.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_group_segment_raw16.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_group_destroy.argtypes = [C.c_void_p]
        L.mi_unet_group_destroy.restype = None
        L.mi_unet_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_unet_tile_axis.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_unet_infer_tiled_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.mi_unet_infer_tiled_raw16.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p]
        L.mi_unet_segment_tiled_raw16.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_set_tile_blend.argtypes = [C.c_void_p, C.POINTER(TileBlend)]
        L.mi_unet_get_tile_blend.argtypes = [C.c_void_p, C.POINTER(TileBlend)]
        L.mi_unet_tile_blend_weights.argtypes = [C.c_int, C.POINTER(TileBlend), C.c_void_p]
        L.mi_unet_target_min_area.argtypes = [C.c_int, C.c_int, C.c_float]
        L.mi_unet_set_targets.argtypes = [C.c_void_p, C.POINTER(Target), C.c_int]
        L.mi_unet_get_targets.argtypes = [C.c_void_p, C.POINTER(Target), C.c_int, C.POINTER(C.c_int)]
        L.mi_unet_postprocess_masks_multi.argtypes = L.mi_unet_postprocess_masks.argtypes
        L.mi_unet_segment_raw16_multi.argtypes = L.mi_unet_segment_raw16.argtypes
        L.mi_unet_segment_tiled_raw16_multi.argtypes = L.mi_unet_segment_tiled_raw16.argtypes
        L.mi_unet_group_set_targets.argtypes = [C.c_void_p, C.POINTER(Target), C.c_int]
        L.mi_unet_group_segment_raw16_multi.argtypes = L.mi_unet_group_segment_raw16.argtypes
        L.mi_unet_set_window.argtypes = [C.c_void_p, C.POINTER(Window)]
        L.mi_unet_get_window.argtypes = [C.c_void_p, C.POINTER(Window)]
        L.mi_unet_window_of.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(Window), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_unet_last_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.mi_unet_group_set_window.argtypes = [C.c_void_p, C.POINTER(Window)]
        L.mi_unet_set_measure.argtypes = [C.c_void_p, C.POINTER(Measure)]
        L.mi_unet_get_measure.argtypes = [C.c_void_p, C.POINTER(Measure)]
        L.mi_unet_last_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_unet_measure_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_region_derive.argtypes = [C.POINTER(Region), C.POINTER(RegionShape)]
        L.mi_unet_score_labels_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_score_labels.argtypes = [C.c_void_p] + L.mi_unet_score_labels_host.argtypes
        L.mi_unet_score_derive.argtypes = [C.POINTER(Score), C.POINTER(ScoreMetrics)]
        L.mi_unet_volume_components_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_components.argtypes = [C.c_void_p] + L.mi_unet_volume_components_host.argtypes
        L.mi_unet_volume_derive.argtypes = [C.POINTER(VComp), C.POINTER(C.c_double), C.POINTER(VCompMetrics)]
        L.mi_unet_score_volume_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_score_volume.argtypes = [C.c_void_p] + L.mi_unet_score_volume_host.argtypes
        L.mi_unet_score_volume_units.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.mi_unet_score_volume_derive.argtypes = [C.POINTER(Score), C.c_double, C.POINTER(ScoreMetrics)]
        L.mi_unet_volume_clean_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
        L.mi_unet_volume_clean.argtypes = [C.c_void_p] + L.mi_unet_volume_clean_host.argtypes
        L.mi_unet_volume_ball.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_mesh_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_volume_mesh.argtypes = [C.c_void_p] + L.mi_unet_volume_mesh_host.argtypes
        L.mi_unet_volume_mesh_positions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_mesh_derive.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MeshMetrics)]
        L.mi_unet_volume_measure_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_measure.argtypes = [C.c_void_p] + L.mi_unet_volume_measure_host.argtypes
        L.mi_unet_volume_measure_derive.argtypes = [C.POINTER(VMeasure), C.c_void_p, C.c_double, C.POINTER(VMeasureShape)]
        L.mi_unet_volume_spatial_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_spatial.argtypes = [C.c_void_p] + L.mi_unet_volume_spatial_host.argtypes
        L.mi_unet_volume_spatial_derive.argtypes = [C.POINTER(VSpatial), C.c_void_p, C.c_double, C.POINTER(VSpatialMetrics)]
        L.mi_unet_volume_split_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_split.argtypes = [C.c_void_p] + L.mi_unet_volume_split_host.argtypes
        L.mi_unet_volume_split_derive.argtypes = [C.POINTER(VPiece), C.POINTER(C.c_double), C.c_double, C.POINTER(VPieceMetrics)]
        L.mi_unet_volume_skeleton_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]
        L.mi_unet_volume_skeleton.argtypes = [C.c_void_p] + L.mi_unet_volume_skeleton_host.argtypes
        L.mi_unet_volume_skeleton_derive.argtypes = [C.POINTER(VSkel), C.POINTER(C.c_double), C.c_double, C.POINTER(VSkelMetrics)]
        L.mi_unet_volume_skeleton_simple_host.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        L.mi_unet_volume_skeleton_simple.argtypes = [C.c_void_p] + L.mi_unet_volume_skeleton_simple_host.argtypes
        L.mi_unet_volume_branches_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_branches.argtypes = [C.c_void_p] + L.mi_unet_volume_branches_host.argtypes
        L.mi_unet_volume_branches_derive_branch.argtypes = [C.POINTER(VBranch), C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double,
                                                            C.POINTER(VBranchMetrics)]
        L.mi_unet_volume_branches_derive.argtypes = [C.POINTER(VGraph), C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_double), C.c_double,
                                                     C.POINTER(VGraphMetrics)]
        L.mi_unet_volume_texture_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        L.mi_unet_volume_texture.argtypes = [C.c_void_p] + L.mi_unet_volume_texture_host.argtypes
        L.mi_unet_volume_texture_derive.argtypes = [C.POINTER(VTexture), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(VTextureFeatures)]
        L.mi_unet_volume_interp_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_interp.argtypes = [C.c_void_p] + L.mi_unet_volume_interp_host.argtypes
        L.mi_unet_volume_interp_slices.argtypes = [C.c_int, C.c_int]
        L.mi_unet_volume_zones_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mi_unet_volume_zones.argtypes = [C.c_void_p] + L.mi_unet_volume_zones_host.argtypes
        L.mi_unet_volume_zones_run_features.argtypes = [C.POINTER(VZones), C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(VZoneFeatures)]
        L.mi_unet_volume_zones_zone_features.argtypes = [C.POINTER(VZones), C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(VZoneFeatures)]
        L.mi_unet_volume_nbhood_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mi_unet_volume_nbhood.argtypes = [C.c_void_p] + L.mi_unet_volume_nbhood_host.argtypes
        L.mi_unet_volume_nbhood_derive.argtypes = [C.POINTER(VNbhood), C.POINTER(VNbhoodOut), C.c_int, C.c_int, C.c_int, C.POINTER(VNbhoodFeatures)]
        L.mi_unet_volume_match_host.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
        L.mi_unet_volume_match.argtypes = [C.c_void_p] + L.mi_unet_volume_match_host.argtypes
        L.mi_unet_volume_match_assign.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.POINTER(VMatchCounts)]
        L.mi_unet_volume_match_derive.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                  C.POINTER(VMatchScores)]
        L.mi_unet_group_set_measure.argtypes = [C.c_void_p, C.POINTER(Measure)]
        L.mi_unet_group_last_regions.argtypes = L.mi_unet_last_regions.argtypes
        L.mi_unet_set_morph.argtypes = [C.c_void_p, C.POINTER(Morph), C.c_int]
        L.mi_unet_get_morph.argtypes = [C.c_void_p, C.POINTER(Morph), C.c_int, C.POINTER(C.c_int)]
        L.mi_unet_morph_element.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.mi_unet_group_set_morph.argtypes = [C.c_void_p, C.POINTER(Morph), C.c_int]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise MiUnetError(rc, lib().mi_unet_last_error().decode(errors="replace"))


class PinnedArray:
    """A numpy view of page-locked host memory (mi_unet_host_alloc): RAW images kept in one are uploaded without a staging copy.
    Keep the object alive as long as the view `.a` is used; close() (or garbage collection) releases the memory."""

    def __init__(self, shape, dtype):
        self._p = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _check(lib().mi_unet_host_alloc(n, C.byref(self._p)))
        self.a = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(n,)).view(dtype).reshape(shape)

    def close(self):
        if self._p:
            self.a = None
            lib().mi_unet_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    return int(lib().mi_unet_device_count())


def default_config() -> Config:
    c = Config()
    lib().mi_unet_default_config(C.byref(c))
    return c


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Engine:
    """One engine handle = one GPU's context (the reference's thread-local TensorRTContext, include/process.h:13-23)."""

    CONV_ALGOS = {"auto": 0, "direct": 1, "winograd": 2, "winograd16": 3, "bf16": 4, "fp16": 5}

    def __init__(self, height=512, width=512, in_ch=1, base=64, levels=4, classes=3, max_batch=16, device=0,
                 conv_algo="auto"):
        self.cfg = Config(height, width, in_ch, base, levels, classes, max_batch, device, self.CONV_ALGOS[conv_algo])
        self._h = C.c_void_p()
        _check(lib().mi_unet_create(C.byref(self.cfg), C.byref(self._h)))

    def clone(self, max_batch=0) -> "Engine":
        """A second context on the same device sharing this engine's weight blob (mi_unet_clone)."""
        other = object.__new__(Engine)
        other.cfg = Config(self.cfg.height, self.cfg.width, self.cfg.in_ch, self.cfg.base, self.cfg.levels, self.cfg.classes,
                           max_batch if max_batch > 0 else self.cfg.max_batch, self.cfg.device, self.cfg.conv_algo)
        other._h = C.c_void_p()
        _check(lib().mi_unet_clone(self._h, max_batch, C.byref(other._h)))
        return other

    def close(self):
        if self._h:
            lib().mi_unet_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, path_or_blob):
        if isinstance(path_or_blob, (bytes, bytearray, memoryview)):
            buf = (C.c_char * len(path_or_blob)).from_buffer_copy(path_or_blob)
            _check(lib().mi_unet_load_weights_from_memory(self._h, C.cast(buf, C.c_void_p), len(path_or_blob)))
        else:
            _check(lib().mi_unet_load_weights(self._h, os.fsencode(path_or_blob)))

    def infer(self, imgs: np.ndarray, want_logits=False):
        """imgs u8 [B,H,W,C] (host) -> labels u8 [B,H,W], logits f32 [B,classes,H,W] or None"""
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        b = imgs.shape[0]
        c = self.cfg
        if imgs.shape[1:] != (c.height, c.width, c.in_ch):
            raise ValueError(f"Input size must be {c.height}x{c.width}x{c.in_ch}, got {imgs.shape[1:]}")
        labels = np.empty((b, c.height, c.width), np.uint8)
        logits = np.empty((b, c.classes, c.height, c.width), np.float32) if want_logits else None
        _check(lib().mi_unet_infer_u8(self._h, _ptr(imgs), b, _ptr(labels), _ptr(logits)))
        return labels, logits

    def _raw_args(self, raws):
        """list of u16 planes (in_ch per image, image-major) -> (keep-alive list, pointer / width / height arrays, B)"""
        raws = [np.ascontiguousarray(r, dtype=np.uint16) for r in raws]
        n, c = len(raws), self.cfg
        if n % c.in_ch:
            raise ValueError(f"{n} planes for an engine with in_ch = {c.in_ch}")
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in raws])
        ws = (C.c_int * n)(*[r.shape[1] for r in raws])
        hs = (C.c_int * n)(*[r.shape[0] for r in raws])
        return raws, ptrs, ws, hs, n // c.in_ch

    def _tile_buf(self, b):
        c = self.cfg
        return np.empty((b, c.height, c.width) if c.in_ch == 1 else (b, c.height, c.width, c.in_ch), np.uint8)

    def infer_raw16(self, raws, want_tiles=True, want_logits=False):
        """raws: list of u16 [h_i][w_i] planes, in_ch per image -> (tiles u8 [B,H,W(,C)] or None, labels u8 [B,H,W], logits or None)"""
        c = self.cfg
        raws, ptrs, ws, hs, b = self._raw_args(raws)
        tiles = self._tile_buf(b) if want_tiles else None
        labels = np.empty((b, c.height, c.width), np.uint8)
        logits = np.empty((b, c.classes, c.height, c.width), np.float32) if want_logits else None
        _check(lib().mi_unet_infer_raw16(self._h, ptrs, ws, hs, b, _ptr(tiles), _ptr(labels), _ptr(logits)))
        return tiles, labels, logits

    def set_postprocess(self, on: bool):
        _check(lib().mi_unet_set_postprocess(self._h, int(on)))

    def postprocess_masks(self, labels: np.ndarray):
        labels = np.ascontiguousarray(labels, np.uint8)
        out = np.empty_like(labels)
        _check(lib().mi_unet_postprocess_masks(self._h, _ptr(labels), labels.shape[0], _ptr(out)))
        return out

    def extract_contours(self, masks: np.ndarray, cap_points=8192, cap_contours=256):
        """masks u8 [B,H,W] -> per image a list of contours [(x, y), ...] (None where a capacity overflowed)"""
        masks = np.ascontiguousarray(masks, np.uint8)
        b = masks.shape[0]
        xy = np.zeros((b, cap_points, 2), np.int32)
        start = np.zeros((b, cap_contours + 1), np.int32)
        counts = np.zeros(b, np.int32)
        _check(lib().mi_unet_extract_contours(self._h, _ptr(masks), b, _ptr(xy), cap_points, _ptr(start), cap_contours, _ptr(counts)))
        out = []
        for i in range(b):
            if counts[i] < 0:
                out.append(None)
                continue
            out.append([[tuple(p) for p in xy[i, start[i, c]:start[i, c + 1]].tolist()] for c in range(counts[i])])
        return out

    def segment_raw16_prepare(self, raws, cap_points=8192, cap_contours=64):
        """argument block of mi_unet_segment_raw16 for these images: pointer arrays and caller-owned output buffers, built once"""
        c = self.cfg
        raws, ptrs, ws, hs, b = self._raw_args(raws)
        return dict(raws=raws, ptrs=ptrs, ws=ws, hs=hs, b=b, cap_points=cap_points, cap_contours=cap_contours,
                    tiles=self._tile_buf(b), masks=np.empty((b, c.height, c.width), np.uint8),
                    xy=np.zeros((b, cap_points, 2), np.int32), start=np.zeros((b, cap_contours + 1), np.int32),
                    counts=np.zeros(b, np.int32))

    def segment_raw16_run(self, p):
        """the C call alone (what a C or C++ host pays)"""
        _check(lib().mi_unet_segment_raw16(self._h, p["ptrs"], p["ws"], p["hs"], p["b"], _ptr(p["tiles"]), _ptr(p["masks"]), _ptr(p["xy"]),
                                           p["cap_points"], _ptr(p["start"]), p["cap_contours"], _ptr(p["counts"])))

    @staticmethod
    def segment_raw16_decode(p):
        xy, start, counts = p["xy"], p["start"], p["counts"]
        cont = []
        for i in range(p["b"]):
            cont.append(None if counts[i] < 0 else
                        [[tuple(q) for q in xy[i, start[i, k]:start[i, k + 1]].tolist()] for k in range(counts[i])])
        return p["tiles"], p["masks"], cont

    def segment_raw16(self, raws, cap_points=8192, cap_contours=64):
        """RAW16 images -> (tiles, mask images 0/255, contours per image) with every stage on the device"""
        p = self.segment_raw16_prepare(raws, cap_points, cap_contours)
        self.segment_raw16_run(p)
        return self.segment_raw16_decode(p)

    def infer_tiled(self, img: np.ndarray, halo: int, want_logits=False):
        """One image u8 [H,W(,C)] of any size >= the engine's tile -> labels u8 [H,W], logits f32 [classes,H,W] or None; run as
        overlapping tiles of the engine's size, each pixel taken from the tile that owns it (tile_axis) or, after set_tile_blend,
        the weighted mean of the tiles (and mirrored views) that cover it."""
        c = self.cfg
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim == 2:
            img = img[:, :, None]
        if img.ndim != 3 or img.shape[2] != c.in_ch:
            raise ValueError(f"Input must be [H,W,{c.in_ch}], got {img.shape}")
        hh, ww = img.shape[:2]
        labels = np.empty((hh, ww), np.uint8)
        logits = np.empty((c.classes, hh, ww), np.float32) if want_logits else None
        _check(lib().mi_unet_infer_tiled_u8(self._h, _ptr(img), hh, ww, halo, _ptr(labels), _ptr(logits)))
        return labels, logits

    def set_tile_blend(self, mode="owner", sigma_scale=0.125, mirror=""):
        """How the tiled calls combine overlapping tiles (mi_unet_set_tile_blend): mode "owner" | "constant" | "gaussian", mirror
        "" | "x" | "y" | "xy" (test-time mirror averaging).  mode=None restores the default (owner, 0.125, no mirror)."""
        b = None if mode is None else C.byref(_tile_blend(mode, sigma_scale, mirror))
        _check(lib().mi_unet_set_tile_blend(self._h, b))

    def get_tile_blend(self):
        """-> {"mode": name, "sigma_scale": float, "mirror": name}"""
        b = TileBlend()
        _check(lib().mi_unet_get_tile_blend(self._h, C.byref(b)))
        return {"mode": {v: k for k, v in BLEND_MODES.items()}[b.mode], "sigma_scale": b.sigma_scale,
                "mirror": {v: k for k, v in MIRRORS.items()}[b.mirror]}

    def _tiled_planes(self, planes):
        """in_ch u16 planes of one size [H,W] -> (keep-alive list, pointer array, H, W)"""
        c = self.cfg
        if isinstance(planes, np.ndarray) and planes.ndim == 2:
            planes = [planes] * c.in_ch
        keep = []
        for p in planes:                                     # the same array passed twice keeps ONE pointer (uploaded once)
            q = next((k for k, orig in keep if orig is p), None)
            keep.append((np.ascontiguousarray(p, dtype=np.uint16) if q is None else q, p))
        arrs = [k for k, _ in keep]
        if len(arrs) != c.in_ch or any(a.ndim != 2 or a.shape != arrs[0].shape for a in arrs):
            raise ValueError(f"need {c.in_ch} u16 planes of one [H,W] shape")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        return arrs, ptrs, arrs[0].shape[0], arrs[0].shape[1]

    def _norm_buf(self, hh, ww):
        return np.empty((hh, ww) if self.cfg.in_ch == 1 else (hh, ww, self.cfg.in_ch), np.uint8)

    def infer_tiled_raw16(self, planes, halo: int, want_norm=True, want_logits=False):
        """planes: in_ch u16 [H,W] arrays (or one array, used for every channel) -> (norm u8 [H,W(,C)] or None, labels u8 [H,W],
        logits f32 [classes,H,W] or None) at the image's own resolution"""
        c = self.cfg
        arrs, ptrs, hh, ww = self._tiled_planes(planes)
        norm = self._norm_buf(hh, ww) if want_norm else None
        labels = np.empty((hh, ww), np.uint8)
        logits = np.empty((c.classes, hh, ww), np.float32) if want_logits else None
        _check(lib().mi_unet_infer_tiled_raw16(self._h, ptrs, ww, hh, halo, _ptr(norm), _ptr(labels), _ptr(logits)))
        return norm, labels, logits

    def segment_tiled_raw16(self, planes, halo: int, cap_points=65536, cap_contours=256, want_norm=True):
        """-> (norm or None, mask image 0/255 u8 [H,W], contours [[(x, y), ...], ...] in full-image coordinates, or None when a
        capacity was too small)"""
        arrs, ptrs, hh, ww = self._tiled_planes(planes)
        norm = self._norm_buf(hh, ww) if want_norm else None
        mask = np.empty((hh, ww), np.uint8)
        xy = np.zeros((cap_points, 2), np.int32)
        start = np.zeros(cap_contours + 1, np.int32)
        count = C.c_int32(0)
        _check(lib().mi_unet_segment_tiled_raw16(self._h, ptrs, ww, hh, halo, _ptr(norm), _ptr(mask), _ptr(xy), cap_points, _ptr(start),
                                                 cap_contours, C.byref(count)))
        n = count.value
        cont = None if n < 0 else [[tuple(q) for q in xy[start[k]:start[k + 1]].tolist()] for k in range(n)]
        return norm, mask, cont

    # ---- targets (mi_unet_set_targets): which classes the _multi calls segment, and each one's area rule
    def set_targets(self, targets):
        """targets: [(cls, min_area_frac), ...] (at most MAX_TARGETS); None or [] restores the default [(2, 0.06)]"""
        arr, n = _target_array(targets)
        _check(lib().mi_unet_set_targets(self._h, arr, n))

    def get_targets(self):
        arr, n = (Target * MAX_TARGETS)(), C.c_int()
        _check(lib().mi_unet_get_targets(self._h, arr, MAX_TARGETS, C.byref(n)))
        return [(arr[k].cls, float(arr[k].min_area_frac)) for k in range(n.value)]

    # ---- morphology (mi_unet_set_morph): element and radii of the close / open of the _multi calls, one entry or one per target
    def set_morph(self, morph):
        """morph: [(shape, open_r, close_r), ...] with shape "rect" | "disc"; None or [] restores the default [("rect", 1, 0)]"""
        arr, n = _morph_array(morph)
        _check(lib().mi_unet_set_morph(self._h, arr, n))

    def get_morph(self):
        arr, n = (Morph * MAX_TARGETS)(), C.c_int()
        _check(lib().mi_unet_get_morph(self._h, arr, MAX_TARGETS, C.byref(n)))
        names = {v: k for k, v in MORPH_SHAPES.items()}
        return [(names[arr[k].shape], arr[k].open_r, arr[k].close_r) for k in range(n.value)]

    def postprocess_masks_multi(self, labels: np.ndarray):
        """labels u8 [B,H,W] -> u8 [B,K,H,W], plane k in {0, cls_k}"""
        labels = np.ascontiguousarray(labels, np.uint8)
        out = np.empty((labels.shape[0], len(self.get_targets())) + labels.shape[1:], np.uint8)
        _check(lib().mi_unet_postprocess_masks_multi(self._h, _ptr(labels), labels.shape[0], _ptr(out)))
        return out

    def segment_raw16_multi_prepare(self, raws, cap_points=8192, cap_contours=64):
        """argument block of mi_unet_segment_raw16_multi for the targets set now (segment_raw16_prepare with [B][K] outputs)"""
        c, k = self.cfg, len(self.get_targets())
        raws, ptrs, ws, hs, b = self._raw_args(raws)
        return dict(raws=raws, ptrs=ptrs, ws=ws, hs=hs, b=b, k=k, cap_points=cap_points, cap_contours=cap_contours,
                    tiles=self._tile_buf(b), masks=np.empty((b, k, c.height, c.width), np.uint8),
                    xy=np.zeros((b, k, cap_points, 2), np.int32), start=np.zeros((b, k, cap_contours + 1), np.int32),
                    counts=np.zeros((b, k), np.int32))

    def segment_raw16_multi_run(self, p):
        _check(lib().mi_unet_segment_raw16_multi(self._h, p["ptrs"], p["ws"], p["hs"], p["b"], _ptr(p["tiles"]), _ptr(p["masks"]),
                                                 _ptr(p["xy"]), p["cap_points"], _ptr(p["start"]), p["cap_contours"], _ptr(p["counts"])))

    def segment_raw16_multi(self, raws, cap_points=8192, cap_contours=64, raw_arrays=False):
        """RAW16 images -> (tiles, masks 0/255 u8 [B,K,H,W], contours[b][k] = list of contours, or None where a capacity of that
        (image, target) overflowed); raw_arrays=True returns (tiles, masks, xy, start, counts) as the C call filled them"""
        p = self.segment_raw16_multi_prepare(raws, cap_points, cap_contours)
        self.segment_raw16_multi_run(p)
        if raw_arrays:
            return p["tiles"], p["masks"], p["xy"], p["start"], p["counts"]
        return p["tiles"], p["masks"], _decode_multi(p["xy"], p["start"], p["counts"])

    def segment_tiled_raw16_multi(self, planes, halo: int, cap_points=65536, cap_contours=256, want_norm=True, raw_arrays=False):
        """-> (norm or None, masks 0/255 u8 [K,H,W], contours[k] in full-image coordinates, None where a capacity overflowed)"""
        k = len(self.get_targets())
        arrs, ptrs, hh, ww = self._tiled_planes(planes)
        norm = self._norm_buf(hh, ww) if want_norm else None
        mask = np.empty((k, hh, ww), np.uint8)
        xy = np.zeros((k, cap_points, 2), np.int32)
        start = np.zeros((k, cap_contours + 1), np.int32)
        counts = np.zeros(k, np.int32)
        _check(lib().mi_unet_segment_tiled_raw16_multi(self._h, ptrs, ww, hh, halo, _ptr(norm), _ptr(mask), _ptr(xy), cap_points,
                                                       _ptr(start), cap_contours, _ptr(counts)))
        if raw_arrays:
            return norm, mask, xy, start, counts
        return norm, mask, _decode_multi(xy[None], start[None], counts[None])[0]

    # ---- intensity window (mi_unet_set_window): which sample range of a RAW16 plane becomes 0..255 in every RAW-in call
    def set_window(self, mode="minmax", clip_lo_ppm=0, clip_hi_ppm=0, lo=0, hi=65535):
        """mode "minmax" (default: the exact min / max) | "percentile" (clip_lo_ppm / clip_hi_ppm parts per million of the samples
        clipped at the dark / bright end) | "fixed" (lo..hi); mode=None restores the default"""
        _check(lib().mi_unet_set_window(self._h, _window(mode, clip_lo_ppm, clip_hi_ppm, lo, hi)))

    def get_window(self):
        """-> {"mode": name, "clip_lo_ppm", "clip_hi_ppm", "lo", "hi"}"""
        w = Window()
        _check(lib().mi_unet_get_window(self._h, C.byref(w)))
        return {"mode": {v: k for k, v in WINDOW_MODES.items()}[w.mode], "clip_lo_ppm": w.clip_lo_ppm, "clip_hi_ppm": w.clip_hi_ppm,
                "lo": w.lo, "hi": w.hi}

    def last_windows(self):
        """the (lo, hi) the last RAW-in call applied, one row per plane in call order: int32 [planes, 2] (mi_unet_last_windows)"""
        n = C.c_int()
        _check(lib().mi_unet_last_windows(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 2), np.int32)
        _check(lib().mi_unet_last_windows(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    # ---- region measurement (mi_unet_set_measure): every contour-returning call also measures the regions behind its contours
    def set_measure(self, on=True, channel=0):
        """on=None restores the default (off, channel 0)"""
        _check(lib().mi_unet_set_measure(self._h, None if on is None else C.byref(Measure(int(bool(on)), int(channel)))))

    def get_measure(self):
        m = Measure()
        _check(lib().mi_unet_get_measure(self._h, C.byref(m)))
        return {"on": bool(m.on), "channel": m.channel}

    def last_regions(self):
        """the regions of the last contour-returning call: (REGION_DTYPE [planes, cap_contours], counts int32 [planes])"""
        return _last_regions(lib().mi_unet_last_regions, self._h)

    def measure_regions(self, masks: np.ndarray, tiles=None, channel=0, cap_contours=256):
        """the stage alone: masks u8 [B,H,W], tiles u8 [B,H,W(,C)] or None -> (REGION_DTYPE [B, cap_contours], counts int32 [B])"""
        masks = np.ascontiguousarray(masks, np.uint8)
        b = masks.shape[0]
        if tiles is not None:
            tiles = np.ascontiguousarray(tiles, np.uint8)
            if tiles.size != masks.size * self.cfg.in_ch:
                raise ValueError(f"tiles must be [B,H,W,{self.cfg.in_ch}] for these masks, got {tiles.shape}")
        regions = np.zeros((b, cap_contours), REGION_DTYPE)
        counts = np.zeros(b, np.int32)
        _check(lib().mi_unet_measure_regions(self._h, _ptr(masks), _ptr(tiles), b, int(channel), _ptr(regions), cap_contours, _ptr(counts)))
        return regions, counts

    # ---- scores against ground truth (mi_unet_score_labels): needs the device, not the weights
    def score_labels(self, pred, truth, values, quantile_ppm=50000, classes=0):
        """pred, truth u8 [B,H,W] of any size, values = the bytes to compare -> SCORE_DTYPE [B, n]; with classes > 0 also the confusion
        matrix int64 [B, classes, classes] (row = truth, column = pred) and the pixels left out of it, int64 [B]"""
        return _score_call(lib().mi_unet_score_labels, (self._h,), pred, truth, values, quantile_ppm, classes)

    # ---- a stack of masks as one volume (mi_unet_volume_components): needs the device, not the weights
    def volume_components(self, masks, values, connectivity=26, min_voxels=0, keep_largest=0, cap=256, want_ids=False):
        """masks u8 [D,H,W] of any size, values = the bytes whose sets are labelled -> (out u8 [n,D,H,W], table VCOMP_DTYPE [n, cap],
        found int32 [n], kept int32 [n], ids int32 [n,D,H,W] or None)"""
        return _volume_call(lib().mi_unet_volume_components, (self._h,), masks, values, connectivity, min_voxels, keep_largest, cap, want_ids)

    # ---- slices put between the slices of a stack of masks (mi_unet_volume_interp): needs the device, not the weights
    def volume_interp(self, masks, values, units_xy, factor, intensity=None):
        """masks u8 [D,H,W], in-plane units (ux, uy), factor k in 1 .. 16, intensity u16 [D,H,W] or None
        -> (out u8 [n,D',H,W], stats VINTERP_DTYPE [n][, intensity_out u16 [D',H,W]]), D' = (D - 1) k + 1"""
        return _volume_interp_call(lib().mi_unet_volume_interp, (self._h,), masks, values, units_xy, factor, intensity)

    # ---- a stack of masks cleaned as one volume (mi_unet_volume_clean): needs the device, not the weights
    def volume_clean(self, masks, values, units, fill=True, close_r=0, open_r=0):
        """masks u8 [D,H,W] of any size, values = the bytes whose sets are cleaned, units = the spacing (ux, uy, uz) as integers, the
        radii in the same unit -> (out u8 [n,D,H,W], stats VCLEAN_DTYPE [n])"""
        return _volume_clean_call(lib().mi_unet_volume_clean, (self._h,), masks, values, units, fill, close_r, open_r)

    # ---- the border of a stack as a quad mesh (mi_unet_volume_mesh): needs the device, not the weights
    def volume_mesh(self, masks, values, placement="faces", cap=None, raw=False):
        """masks u8 [D,H,W] of any size, values = the bytes whose sets are meshed, placement "faces" or "nets" -> ([(verts
        MESH_VERTEX_DTYPE [V], quads int32 [Q, 4]) per value], stats MESH_STAT_DTYPE [n]).  cap=None makes a counting call, then a sized
        one; cap = an int or (cap_verts, cap_quads) makes one call and trims to min(count, cap); raw=True returns the untrimmed arrays"""
        return _volume_mesh_call(lib().mi_unet_volume_mesh, (self._h,), masks, values, placement, cap, raw)

    # ---- the texture of the components of a labelled stack (mi_unet_volume_texture): needs the device, not the weights
    def volume_texture(self, ids, intensity, m, levels=32, mode="count", lo=0, width=1, want=("glcm", "axial")):
        """ids int32 [D,H,W], intensity u16 [D,H,W], m components -> (table VTEXTURE_DTYPE [m], hist u32 [m, levels], glcm u32
        [m, levels, levels] or None, glcm_axial or None): per component its grey-level histogram and its 3-D co-occurrence counts over
        the 13 forward neighbours and over the 4 in-plane ones (include/mi_unet.h)"""
        return _volume_texture_call(lib().mi_unet_volume_texture, (self._h,), ids, intensity, m, levels, mode, lo, width, want)

    # ---- the run-length and size-zone matrices of the components of a labelled stack (mi_unet_volume_zones): needs the device, not the weights
    def volume_zones(self, ids, intensity, m, levels=32, mode="count", lo=0, width=1, max_run=32, want_runs=True, want_axial=True, cap=None):
        """ids int32 [D,H,W], intensity u16 [D,H,W], m components -> (table VZONES_DTYPE [m], rlm u32 [m, levels, max_run] or None,
        rlm_axial or None, zones VZONE_DTYPE [cap] or None, found or None); cap = None: a record per voxel (at most 2^24), 0: no zone
        half.  The library checks the values and the limits"""
        return _volume_zones_call(lib().mi_unet_volume_zones, (self._h,), ids, intensity, m, levels, mode, lo, width, max_run, want_runs,
                                  want_axial, cap)

    # ---- the neighbourhood-difference, dependence and distance-zone tables of the components of a labelled stack (mi_unet_volume_nbhood):
    # needs the device, not the weights
    def volume_nbhood(self, ids, intensity, m, levels=32, mode="count", lo=0, width=1, alpha=0, max_dist=32, want=VNBHOOD_WANT):
        """ids int32 [D,H,W], intensity u16 [D,H,W], m components -> (table VNBHOOD_DTYPE [m], dict over VNBHOOD_TABLES of u32 / u64
        [m, levels, 27 | 9 | max_dist], None for a table not in `want`).  The library checks the values and the limits"""
        return _volume_nbhood_call(lib().mi_unet_volume_nbhood, (self._h,), ids, intensity, m, levels, mode, lo, width, alpha, max_dist, want)

    # ---- the components of a labelled stack measured (mi_unet_volume_measure): needs the device, not the weights
    def volume_measure(self, ids, intensity=None, m=1, units=(1, 1, 1), max_ends=None):
        """ids int32 [D,H,W] of any size as mi_unet_volume_components writes them, intensity u16 [D,H,W] or None, m = the components
        to measure (ids 1 .. m), units = the spacing (ux, uy, uz) as integers, max_ends = the cap of the diameter search (None: 262144)
        -> table VMEASURE_DTYPE [m]"""
        return _volume_measure_call(lib().mi_unet_volume_measure, (self._h,), ids, intensity, m, units, max_ends)

    # ---- touching objects split into pieces (mi_unet_volume_split): needs the device, not the weights
    def volume_split(self, masks, values, units=(1, 1, 1), connectivity=26, neck_r=0, min_core=1, cap=256, want_ids=False):
        """masks u8 [D,H,W] of any size, values = the bytes whose sets are split, units = the spacing (ux, uy, uz), neck_r = the radius
        of the eroding ball in the spacing unit -> dict(table VCOMP_DTYPE [n, cap], info VPIECE_DTYPE [n, cap], found, stats
        VSPLIT_STAT_DTYPE [n], ids int32 [n,D,H,W] when want_ids, rounds)"""
        return _volume_split_call(lib().mi_unet_volume_split, (self._h,), masks, values, units, connectivity, neck_r, min_core, cap, want_ids)

    # ---- components thinned to medial lines (mi_unet_volume_skeleton): needs the device, not the weights
    def volume_skeleton(self, ids, m=1, units=(1, 1, 1), max_passes=0, radius=True, want_ids=True, want_r2=False):
        """mi_unet_volume_skeleton: ids int32 [D,H,W] (component r is ids == r + 1), units (ux, uy, uz) -> dict(table VSKEL_DTYPE [m], ids
        int32 [D,H,W] when want_ids, r2 int32 [D,H,W] when want_r2, passes, deleted, stable)"""
        return _volume_skeleton_call(lib().mi_unet_volume_skeleton, (self._h,), ids, m, units, max_passes, radius, want_ids, want_r2)

    # ---- a skeleton split into nodes and branches (mi_unet_volume_branches): needs the device, not the weights
    def volume_branches(self, ids, m=1, r2=None, units=(1, 1, 1), prune_voxels=0, prune_rounds=0, cap_nodes=4096, cap_branches=4096, want_map=True,
                        want_ids=False):
        """mi_unet_volume_branches: ids int32 [D,H,W] as volume_skeleton writes them, r2 its radius field or None -> dict(nodes VNODE_DTYPE,
        branches VBRANCH_DTYPE (the first min(found, cap) rows of each), graph VGRAPH_DTYPE [m], map int32 [D,H,W] when want_map, ids int32
        [D,H,W] when want_ids (the ids after pruning), found_nodes, found_branches, rounds, stable)"""
        return _volume_branches_call(lib().mi_unet_volume_branches, (self._h,), ids, m, r2, units, prune_voxels, prune_rounds, cap_nodes, cap_branches,
                                     want_map, want_ids)

    def volume_skeleton_simple(self, first_word=0, n_words=SKELETON_CODE_WORDS):
        """mi_unet_volume_skeleton_simple: the kernels' simple-point test on codes 32 * first_word .. 32 * (first_word + n_words) - 1 ->
        uint32 [n_words], the layout of volume_skeleton_simple_host"""
        bits = np.zeros(max(int(n_words), 1), np.uint32)
        _check(lib().mi_unet_volume_skeleton_simple(self._h, int(first_word), int(n_words), _ptr(bits)))
        return bits

    # ---- where the intensity of the components of a labelled stack sits (mi_unet_volume_spatial): needs the device, not the weights
    def volume_spatial(self, ids, intensity, m=1, units=(1, 1, 1), max_voxels=None, peak_r=0):
        """ids int32 [D,H,W] of any size as mi_unet_volume_components writes them, intensity u16 [D,H,W], m = the components to take
        (ids 1 .. m), units = the spacing (ux, uy, uz) as integers, max_voxels = the cap of the pair sums (None: 131072), peak_r = the
        radius of the peak sphere in the spacing unit -> table VSPATIAL_DTYPE [m]"""
        return _volume_spatial_call(lib().mi_unet_volume_spatial, (self._h,), ids, intensity, m, units, max_voxels, peak_r)

    # ---- the components of two labelled stacks matched (mi_unet_volume_match): needs the device, not the weights
    def volume_match(self, pred_ids, truth_ids, mp, mt, cap=4096):
        """pred_ids, truth_ids int32 [D,H,W] of any size as mi_unet_volume_components writes them, mp and mt = the components a side
        (ids 1 .. m), cap = the length of the pair list -> (pred_side VMATCH_SIDE_DTYPE [mp], truth_side [mt], pairs VMATCH_PAIR_DTYPE
        [cap], found)"""
        return _volume_match_call(lib().mi_unet_volume_match, (self._h,), pred_ids, truth_ids, mp, mt, cap)

    # ---- scores of a stack as one volume (mi_unet_score_volume): needs the device, not the weights
    def score_volume(self, pred, truth, values, spacing_units, quantile_ppm=50000, classes=0):
        """pred, truth u8 [D,H,W] of any size, values = the bytes to compare, spacing_units = (ux, uy, uz) positive integers ->
        SCORE_DTYPE [n]; with classes > 0 also the confusion matrix int64 [classes, classes] (row = truth, column = pred) over the whole
        volume and the voxels left out of it, int64 [1]"""
        return _score_volume_call(lib().mi_unet_score_volume, (self._h,), pred, truth, values, spacing_units, quantile_ppm, classes)

    def infer_device(self, d_imgs_ptr: int, b: int, d_labels_ptr: int, d_logits_ptr: int = 0):
        _check(lib().mi_unet_infer_u8_device(self._h, C.c_void_p(d_imgs_ptr), b, C.c_void_p(d_labels_ptr),
                                             C.c_void_p(d_logits_ptr) if d_logits_ptr else None))

    def set_stream(self, stream_ptr: int, reset: bool = False):
        """Run on the caller's hipStream_t.  Handle 0 is the legacy default stream, which mi_unet_set_stream reads as
        "restore the engine's own (non-blocking) stream": work on it is NOT ordered against the default stream, so a
        zero handle is only accepted with reset=True (the caller says that is what they mean)."""
        if not stream_ptr and not reset:
            raise ValueError("stream handle 0 = restore the engine's own stream; pass reset=True or a non-default stream "
                             "(e.g. torch.cuda.Stream(dev).cuda_stream)")
        _check(lib().mi_unet_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def sync(self):
        _check(lib().mi_unet_sync(self._h))

    def timer_begin(self):
        _check(lib().mi_unet_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_float()
        _check(lib().mi_unet_timer_end(self._h, C.byref(ms)))
        return float(ms.value)

    def numeric_guard(self):
        """(text, tripped, diff) of mi_unet_numeric_guard: did this weight set keep F(4x4,3x3)?"""
        t, d = C.c_int(), C.c_float()
        text = lib().mi_unet_numeric_guard(self._h, C.byref(t), C.byref(d)).decode()
        return text, bool(t.value), float(d.value)

    STAGES = ("upload_preprocess", "network", "postprocess", "contours", "download")

    def last_stage_ms(self):
        """device time per stage of the last infer_raw16 / segment_raw16 call (mi_unet_last_stage_ms)"""
        ms = (C.c_float * len(self.STAGES))()
        _check(lib().mi_unet_last_stage_ms(self._h, ms))
        return dict(zip(self.STAGES, (float(v) for v in ms)))

    def layers(self):
        """the launch plan, step by step (mi_unet_debug_layer_info): list of dicts with name / kind / per-image shapes"""
        out = []
        for i in range(lib().mi_unet_debug_layer_count(self._h)):
            info = LayerInfo()
            _check(lib().mi_unet_debug_layer_info(self._h, i, C.byref(info)))
            out.append(info.as_dict())
        return out

    def capture(self, imgs: np.ndarray, layer: int, img: int = 0):
        """mi_unet_debug_capture: run the plan eagerly on `imgs` up to step `layer`; returns (info dict, in, out, pooled, labels)
        of image `img` as float32 NHWC arrays (out = planar logits [classes,H,W] when the step ran the fused head)."""
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        st = LayerInfo()
        _check(lib().mi_unet_debug_layer_info(self._h, layer, C.byref(st)))
        x = np.empty((st.in_h, st.in_w, st.in_c), np.float32)
        n_out = max(st.out_c, self.cfg.classes)
        y = np.full(st.out_h * st.out_w * n_out, np.nan, np.float32)
        p = np.full((st.out_h // 2, st.out_w // 2, st.out_c), np.nan, np.float32)
        lab = np.full((st.out_h, st.out_w), 255, np.uint8)
        info = LayerInfo()
        _check(lib().mi_unet_debug_capture(self._h, _ptr(imgs), imgs.shape[0], layer, img, _ptr(x), _ptr(y), _ptr(p), _ptr(lab),
                                           C.byref(info)))
        d = info.as_dict()
        if d["skipped"]:
            return d, None, None, None, None
        if d["fused_first"]:             # the step read the u8 image (the first layer ran in its loader): `in` holds the image
            x = x.reshape(-1)[: st.in_h * st.in_w * self.cfg.in_ch].reshape(st.in_h, st.in_w, self.cfg.in_ch).copy()
        if d["fused_head"] or d["kind"] == "head":
            y = y[: self.cfg.classes * st.out_h * st.out_w].reshape(self.cfg.classes, st.out_h, st.out_w)
        else:
            y = y[: st.out_h * st.out_w * st.out_c].reshape(st.out_h, st.out_w, st.out_c)
            lab = None
        return d, x, y, (p if d["pooled"] else None), lab

    def set_profiling(self, on: bool):
        _check(lib().mi_unet_set_profiling(self._h, int(on)))

    def kernel_stats(self, cap=8192):
        n = C.c_int()
        arr = (KernelStat * cap)()
        _check(lib().mi_unet_get_kernel_stats(self._h, arr, cap, C.byref(n)))
        return [dict(name=arr[i].name.decode(), kernel=arr[i].kernel.decode(), flops=arr[i].flops, bytes=arr[i].bytes,
                     ms=arr[i].ms) for i in range(min(n.value, cap))]


def _decode_multi(xy, start, counts):
    """contour arrays [B][K]... -> contours[b][k] = [[(x, y), ...], ...] or None"""
    return [[None if counts[i, k] < 0 else
             [[tuple(q) for q in xy[i, k, start[i, k, c]:start[i, k, c + 1]].tolist()] for c in range(counts[i, k])]
             for k in range(counts.shape[1])] for i in range(counts.shape[0])]


def morph_element(shape, r: int) -> np.ndarray:
    """mi_unet_morph_element: the structuring element as u8 [2r + 1, 2r + 1] of 0 / 1 (needs no device)"""
    elem = np.zeros((2 * max(int(r), 0) + 1,) * 2, np.uint8)
    _check(lib().mi_unet_morph_element(MORPH_SHAPES[shape] if isinstance(shape, str) else int(shape), int(r), _ptr(elem)))
    return elem


def target_min_area(height: int, width: int, frac: float) -> int:
    """mi_unet_target_min_area: the pixel count behind a target's min_area_frac on a height x width image (needs no device)"""
    return int(lib().mi_unet_target_min_area(height, width, frac))


def window_of(samples, mode="minmax", clip_lo_ppm=0, clip_hi_ppm=0, lo=0, hi=65535):
    """mi_unet_window_of: the (lo, hi) of these u16 samples under a window setting -- the definition the kernels meet (needs no device)"""
    a = np.ascontiguousarray(samples, np.uint16).reshape(-1)
    wlo, whi = C.c_int(), C.c_int()
    _check(lib().mi_unet_window_of(_ptr(a) if a.size else None, a.size, _window(mode, clip_lo_ppm, clip_hi_ppm, lo, hi), C.byref(wlo), C.byref(whi)))
    return wlo.value, whi.value


def score_labels_host(pred, truth, values, quantile_ppm=50000, classes=0):
    """mi_unet_score_labels_host: Engine.score_labels as pure host arithmetic (needs no device)"""
    return _score_call(lib().mi_unet_score_labels_host, (), pred, truth, values, quantile_ppm, classes)


def volume_components_host(masks, values, connectivity=26, min_voxels=0, keep_largest=0, cap=256, want_ids=False):
    """mi_unet_volume_components_host: Engine.volume_components as pure host arithmetic (needs no device)"""
    return _volume_call(lib().mi_unet_volume_components_host, (), masks, values, connectivity, min_voxels, keep_largest, cap, want_ids)


def volume_interp_host(masks, values, units_xy, factor, intensity=None):
    """mi_unet_volume_interp_host: Engine.volume_interp as sequential host arithmetic (needs no device)"""
    return _volume_interp_call(lib().mi_unet_volume_interp_host, (), masks, values, units_xy, factor, intensity)


def volume_interp_slices(d, factor) -> int:
    """mi_unet_volume_interp_slices: (d - 1) factor + 1, or -1 for a d outside 1 .. 8192 or a factor outside 1 .. 16"""
    return int(lib().mi_unet_volume_interp_slices(int(d), int(factor)))


def volume_clean_host(masks, values, units, fill=True, close_r=0, open_r=0):
    """mi_unet_volume_clean_host: Engine.volume_clean as sequential host arithmetic (needs no device)"""
    return _volume_clean_call(lib().mi_unet_volume_clean_host, (), masks, values, units, fill, close_r, open_r)


def volume_mesh_host(masks, values, placement="faces", cap=None, raw=False):
    """mi_unet_volume_mesh_host: Engine.volume_mesh as sequential host arithmetic (needs no device)"""
    return _volume_mesh_call(lib().mi_unet_volume_mesh_host, (), masks, values, placement, cap, raw)


def volume_measure_host(ids, intensity=None, m=1, units=(1, 1, 1), max_ends=None):
    """mi_unet_volume_measure_host: Engine.volume_measure as sequential host arithmetic (needs no device)"""
    return _volume_measure_call(lib().mi_unet_volume_measure_host, (), ids, intensity, m, units, max_ends)


def volume_texture_host(ids, intensity, m, levels=32, mode="count", lo=0, width=1, want=("glcm", "axial")):
    """mi_unet_volume_texture_host: Engine.volume_texture as sequential host arithmetic (needs no device)"""
    return _volume_texture_call(lib().mi_unet_volume_texture_host, (), ids, intensity, m, levels, mode, lo, width, want)


def volume_zones_host(ids, intensity, m, levels=32, mode="count", lo=0, width=1, max_run=32, want_runs=True, want_axial=True, cap=None):
    """mi_unet_volume_zones_host: Engine.volume_zones as sequential host arithmetic (needs no device)"""
    return _volume_zones_call(lib().mi_unet_volume_zones_host, (), ids, intensity, m, levels, mode, lo, width, max_run, want_runs, want_axial, cap)


def _vzones_entry(comp):
    return comp if isinstance(comp, VZones) else VZones(**{n: int(comp[n]) for n, _ in VZones._fields_})


def volume_zones_run_features(comp, rlm_row, directions=13):
    """mi_unet_volume_zones_run_features of one component (a VZones, or one VZONES_DTYPE record) and its row u32 [L, R] of rlm (directions
    13) or rlm_axial (4) -> dict of the 16 features"""
    rlm_row = np.ascontiguousarray(rlm_row, np.uint32)
    out = VZoneFeatures()
    _check(lib().mi_unet_volume_zones_run_features(C.byref(_vzones_entry(comp)), _ptr(rlm_row), int(rlm_row.shape[0]), int(rlm_row.shape[1]),
                                                   int(directions), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VZoneFeatures._fields_}


def volume_zones_zone_features(comp, zones, r, levels):
    """mi_unet_volume_zones_zone_features of component r (its VZones, or one VZONES_DTYPE record) over zones VZONE_DTYPE [nz] (the whole
    list or a slice) -> dict of the 16 features"""
    zones = np.ascontiguousarray(zones, VZONE_DTYPE)
    out = VZoneFeatures()
    _check(lib().mi_unet_volume_zones_zone_features(C.byref(_vzones_entry(comp)), _ptr(zones), int(zones.size), int(r), int(levels), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VZoneFeatures._fields_}


def volume_nbhood_host(ids, intensity, m, levels=32, mode="count", lo=0, width=1, alpha=0, max_dist=32, want=VNBHOOD_WANT):
    """mi_unet_volume_nbhood_host: Engine.volume_nbhood as sequential host arithmetic (needs no device)"""
    return _volume_nbhood_call(lib().mi_unet_volume_nbhood_host, (), ids, intensity, m, levels, mode, lo, width, alpha, max_dist, want)


def volume_nbhood_derive(comp, rows, axial=False):
    """mi_unet_volume_nbhood_derive of one component (a VNbhood, or one VNBHOOD_DTYPE record) and `rows`: a dict over VNBHOOD_TABLES of
    that component's rows (tables[name][r]; None or missing: an absent matrix); axial reads the three [L, 9] rows and dzm_axial -> a
    dict of the five NGTDM features, "ngldm" and "gldzm" (dicts of 16) and dependence_energy"""
    entry = comp if isinstance(comp, VNbhood) else VNbhood(**{n: int(comp[n]) for n, _ in VNbhood._fields_})
    kept = {n: np.ascontiguousarray(rows[n], np.uint64 if "diff" in n else np.uint32) for n in VNBHOOD_TABLES if rows.get(n) is not None}
    shapes = {a.shape[0] for a in kept.values()}
    if len(shapes) > 1:
        raise ValueError("the rows of one component have one number of levels")
    levels = shapes.pop() if shapes else 2
    dist = [kept[n].shape[1] for n in ("dzm", "dzm_axial") if n in kept]
    ptrs = VNbhoodOut(*[kept[n].ctypes.data if n in kept else None for n in VNBHOOD_TABLES])
    out = VNbhoodFeatures()
    _check(lib().mi_unet_volume_nbhood_derive(C.byref(entry), C.byref(ptrs), int(levels), int(dist[0]) if dist else 1, int(bool(axial)), C.byref(out)))
    vz = lambda f: {n: getattr(f, n) for n, _ in VZoneFeatures._fields_}
    res = {n: getattr(out, n) for n in ("coarseness", "contrast", "busyness", "complexity", "strength", "dependence_energy")}
    res["ngldm"], res["gldzm"] = vz(out.ngldm), vz(out.gldzm)
    return res


def volume_texture_derive(comp, hist, glcm=None):
    """mi_unet_volume_texture_derive of one component (a VTexture, or one VTEXTURE_DTYPE record), its histogram row u32 [L] and one of its
    co-occurrence tables u32 [L, L] (or None: the ten joint features are NaN) -> a dict of the features"""
    if not isinstance(comp, VTexture):
        comp = VTexture(**{n: int(comp[n]) for n, _ in VTexture._fields_})
    hist = np.ascontiguousarray(hist, np.uint32).reshape(-1)
    if glcm is not None:
        glcm = np.ascontiguousarray(glcm, np.uint32).reshape(hist.size, hist.size)
    out = VTextureFeatures()
    _check(lib().mi_unet_volume_texture_derive(C.byref(comp), _ptr(hist), _ptr(glcm), int(hist.size), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VTextureFeatures._fields_}


def volume_spatial_host(ids, intensity, m=1, units=(1, 1, 1), max_voxels=None, peak_r=0):
    """mi_unet_volume_spatial_host: Engine.volume_spatial as sequential host arithmetic (needs no device)"""
    return _volume_spatial_call(lib().mi_unet_volume_spatial_host, (), ids, intensity, m, units, max_voxels, peak_r)


def volume_split_host(masks, values, units=(1, 1, 1), connectivity=26, neck_r=0, min_core=1, cap=256, want_ids=False):
    """mi_unet_volume_split_host: Engine.volume_split as sequential host arithmetic (needs no device)"""
    return _volume_split_call(lib().mi_unet_volume_split_host, (), masks, values, units, connectivity, neck_r, min_core, cap, want_ids)


def volume_skeleton_host(ids, m=1, units=(1, 1, 1), max_passes=0, radius=True, want_ids=True, want_r2=False):
    """mi_unet_volume_skeleton_host: Engine.volume_skeleton as sequential host arithmetic (needs no device)"""
    return _volume_skeleton_call(lib().mi_unet_volume_skeleton_host, (), ids, m, units, max_passes, radius, want_ids, want_r2)


def volume_skeleton_derive(comp, spacing, unit_mm):
    """mi_unet_volume_skeleton_derive of one component (a VSkel, or one VSKEL_DTYPE record) with spacing (sx, sy, sz) in mm and the length
    of the spacing unit in mm -> dict(length_mm, radius_min_mm, radius_max_mm, radius_rms_mm, loops)"""
    if not isinstance(comp, VSkel):
        rec = comp
        comp = VSkel()
        for n, _ in VSkel._fields_:
            if n == "links":
                comp.links = (C.c_int64 * 7)(*[int(v) for v in rec["links"]])
            else:
                setattr(comp, n, int(rec[n]))
    out = VSkelMetrics()
    _check(lib().mi_unet_volume_skeleton_derive(C.byref(comp), (C.c_double * 3)(*[float(v) for v in spacing]), float(unit_mm), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VSkelMetrics._fields_}


def volume_branches_host(ids, m=1, r2=None, units=(1, 1, 1), prune_voxels=0, prune_rounds=0, cap_nodes=4096, cap_branches=4096, want_map=True,
                         want_ids=False):
    """mi_unet_volume_branches_host: Engine.volume_branches as sequential host arithmetic (needs no device)"""
    return _volume_branches_call(lib().mi_unet_volume_branches_host, (), ids, m, r2, units, prune_voxels, prune_rounds, cap_nodes, cap_branches, want_map,
                                 want_ids)


def _fill(struct, rec):
    """a ctypes structure from one record of the numpy dtype of the same layout"""
    out = struct()
    for n, t in struct._fields_:
        setattr(out, n, t(*[int(v) for v in rec[n]]) if hasattr(t, "_length_") else int(rec[n]))
    return out


def volume_branches_derive_branch(row, shape, spacing, unit_mm):
    """mi_unet_volume_branches_derive_branch of one branch (a VBranch, or one VBRANCH_DTYPE record) of a volume of shape (D, H, W) with
    spacing (sx, sy, sz) in mm and the length of the spacing unit in mm -> dict(length_mm, chord_mm, tortuosity, radius_min_mm,
    radius_max_mm, radius_rms_mm)"""
    if not isinstance(row, VBranch):
        row = _fill(VBranch, row)
    out = VBranchMetrics()
    _check(lib().mi_unet_volume_branches_derive_branch(C.byref(row), int(shape[-2]), int(shape[-1]), (C.c_double * 3)(*[float(v) for v in spacing]),
                                                       float(unit_mm), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VBranchMetrics._fields_}


def volume_branches_derive(graph_row, branches, found_nodes, comp_id, spacing, unit_mm):
    """mi_unet_volume_branches_derive of one id (its VGRAPH_DTYPE record, the call's VBRANCH_DTYPE table, info's found_nodes) ->
    dict(length_mm, parts, loops); RuntimeError when the table holds fewer rows of the id than the record counts"""
    g = graph_row if isinstance(graph_row, VGraph) else _fill(VGraph, graph_row)
    table = np.ascontiguousarray(branches, VBRANCH_DTYPE)
    out = VGraphMetrics()
    _check(lib().mi_unet_volume_branches_derive(C.byref(g), _ptr(table) if table.size else None, int(table.size), int(found_nodes), int(comp_id),
                                                (C.c_double * 3)(*[float(v) for v in spacing]), float(unit_mm), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VGraphMetrics._fields_}


def volume_skeleton_simple_host(first_word=0, n_words=SKELETON_CODE_WORDS):
    """mi_unet_volume_skeleton_simple_host: the host form's simple-point test on codes 32 * first_word .. 32 * (first_word + n_words) - 1
    -> uint32 [n_words], code c in bit c & 31 of word (c >> 5) - first_word"""
    bits = np.zeros(max(int(n_words), 1), np.uint32)
    _check(lib().mi_unet_volume_skeleton_simple_host(int(first_word), int(n_words), _ptr(bits)))
    return bits


def volume_split_derive(piece, spacing, unit_mm):
    """mi_unet_volume_split_derive of one piece (a VPiece, or one VPIECE_DTYPE record) with spacing (sx, sy, sz) in mm and the length of
    the spacing unit in mm -> dict(reach_mm, cut_mm2)"""
    if not isinstance(piece, VPiece):
        piece = VPiece(*[int(piece[n]) for n, _ in VPiece._fields_])
    out = VPieceMetrics()
    _check(lib().mi_unet_volume_split_derive(C.byref(piece), (C.c_double * 3)(*[float(v) for v in spacing]), float(unit_mm), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VPieceMetrics._fields_}


def volume_spatial_derive(comp, units, unit_mm):
    """mi_unet_volume_spatial_derive of one component (a VSpatial, or one VSPATIAL_DTYPE record) with the spacing units (ux, uy, uz) and
    the unit in mm -> dict of cx_mm .. cz_mm, icx_mm .. icz_mm, com_shift_mm, integrated_intensity, local_peak, global_peak, morans_i,
    gearys_c"""
    if not isinstance(comp, VSpatial):
        comp = VSpatial(*[(float if t is C.c_double else int)(comp[n]) for n, t in VSpatial._fields_])
    out = VSpatialMetrics()
    _check(lib().mi_unet_volume_spatial_derive(C.byref(comp), (C.c_int * 3)(*[int(v) for v in units]), float(unit_mm), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VSpatialMetrics._fields_}


def volume_measure_derive(comp, units, unit_mm):
    """mi_unet_volume_measure_derive of one component (a VMeasure, or one VMEASURE_DTYPE record) with the spacing units (ux, uy, uz) and
    the unit in mm -> dict of cx_mm, cy_mm, cz_mm, axis_mm [3], axis_dir [3][3], mean, std, diameter_mm, axial_diameter_mm"""
    if not isinstance(comp, VMeasure):
        comp = VMeasure(*[int(comp[n]) for n, _ in VMeasure._fields_])
    out = VMeasureShape()
    _check(lib().mi_unet_volume_measure_derive(C.byref(comp), (C.c_int * 3)(*[int(v) for v in units]), float(unit_mm), C.byref(out)))
    d = {n: getattr(out, n) for n, _ in VMeasureShape._fields_}
    d["axis_mm"] = [float(v) for v in out.axis_mm]
    d["axis_dir"] = [[float(v) for v in row] for row in out.axis_dir]
    return d


def volume_match_host(pred_ids, truth_ids, mp, mt, cap=4096):
    """mi_unet_volume_match_host: Engine.volume_match as sequential host arithmetic (needs no device)"""
    return _volume_match_call(lib().mi_unet_volume_match_host, (), pred_ids, truth_ids, mp, mt, cap)


def _vmatch_tables(pred_side, truth_side, pairs):
    return (np.ascontiguousarray(pred_side, VMATCH_SIDE_DTYPE), np.ascontiguousarray(truth_side, VMATCH_SIDE_DTYPE),
            np.ascontiguousarray(pairs, VMATCH_PAIR_DTYPE))


def volume_match_assign(pred_side, truth_side, pairs, found, iou=(1, 2)):
    """mi_unet_volume_match_assign: the one-to-one assignment of the pair list (all `found` pairs present) at the IoU threshold
    iou = (num, den) -> (match_of_pred int32 [mp], match_of_truth int32 [mt], each 1 + the partner or 0, dict of tp, fp, fn)"""
    ps, ts, pr = _vmatch_tables(pred_side, truth_side, pairs)
    of_p, of_t = np.zeros(len(ps), np.int32), np.zeros(len(ts), np.int32)
    counts = VMatchCounts()
    _check(lib().mi_unet_volume_match_assign(_ptr(ps), len(ps), _ptr(ts), len(ts), _ptr(pr), int(found), len(pr), int(iou[0]), int(iou[1]),
                                             _ptr(of_p), _ptr(of_t), C.byref(counts)))
    return of_p, of_t, {"tp": counts.tp, "fp": counts.fp, "fn": counts.fn}


def volume_match_derive(pred_side, truth_side, pairs, found, match_of_pred):
    """mi_unet_volume_match_derive: the scores of an assignment -> dict of precision, recall, f1, sq, rq, pq, mean_dice (NaN where
    undefined)"""
    ps, ts, pr = _vmatch_tables(pred_side, truth_side, pairs)
    of_p = np.ascontiguousarray(match_of_pred, np.int32)
    if of_p.shape != (len(ps),):
        raise ValueError("match_of_pred holds one entry per pred component")
    out = VMatchScores()
    _check(lib().mi_unet_volume_match_derive(_ptr(ps), len(ps), _ptr(ts), len(ts), _ptr(pr), int(found), len(pr), _ptr(of_p), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VMatchScores._fields_}


def _spacing3(spacing):
    sp = np.ascontiguousarray(spacing, np.float64).reshape(-1)
    if sp.size != 3:
        raise ValueError("spacing holds three numbers: x, y, z")
    return sp


def volume_mesh_positions(verts, spacing):
    """mi_unet_volume_mesh_positions: verts MESH_VERTEX_DTYPE [V], spacing (sx, sy, sz) in mm -> float32 [V, 3] (needs no device)"""
    verts = np.ascontiguousarray(verts, MESH_VERTEX_DTYPE).reshape(-1)
    sp = _spacing3(spacing)
    xyz = np.zeros((verts.size, 3), np.float32)
    _check(lib().mi_unet_volume_mesh_positions(_ptr(verts) if verts.size else None, verts.size, _ptr(sp), _ptr(xyz) if verts.size else None))
    return xyz


def volume_mesh_derive(verts, quads, spacing):
    """mi_unet_volume_mesh_derive: one plane's mesh and the spacing in mm -> dict(area_mm2, volume_mm3) (needs no device)"""
    verts = np.ascontiguousarray(verts, MESH_VERTEX_DTYPE).reshape(-1)
    quads = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
    sp = _spacing3(spacing)
    m = MeshMetrics()
    _check(lib().mi_unet_volume_mesh_derive(_ptr(verts) if verts.size else None, verts.size, _ptr(quads) if quads.size else None, quads.shape[0],
                                            _ptr(sp), C.byref(m)))
    return dict(area_mm2=m.area_mm2, volume_mm3=m.volume_mm3)


def volume_ball(units, r):
    """mi_unet_volume_ball: the ball of radius r under the spacing units (ux, uy, uz) -> ((ex, ey, ez), elem u8 [2ez+1, 2ey+1, 2ex+1])"""
    un = np.ascontiguousarray(units, np.int32).reshape(-1)
    if un.size != 3:
        raise ValueError("units holds three integers: x, y, z")
    ext = np.zeros(3, np.int32)
    _check(lib().mi_unet_volume_ball(_ptr(un), int(r), _ptr(ext), None))
    ex, ey, ez = (int(v) for v in ext)
    elem = np.zeros((2 * ez + 1, 2 * ey + 1, 2 * ex + 1), np.uint8)
    _check(lib().mi_unet_volume_ball(_ptr(un), int(r), _ptr(ext), _ptr(elem)))
    return (ex, ey, ez), elem


def volume_derive(comp, spacing):
    """mi_unet_volume_derive of one component (a VComp, or one VCOMP_DTYPE record) with spacing (sx, sy, sz) in mm -> dict of
    volume_mm3, surface_mm2, cx_mm, cy_mm, cz_mm, extent_x_mm, extent_y_mm, extent_z_mm"""
    if not isinstance(comp, VComp):
        comp = VComp(*[int(comp[n]) for n, _ in VComp._fields_])
    out = VCompMetrics()
    _check(lib().mi_unet_volume_derive(C.byref(comp), (C.c_double * 3)(*[float(v) for v in spacing]), C.byref(out)))
    return {n: getattr(out, n) for n, _ in VCompMetrics._fields_}


def score_derive(score):
    """mi_unet_score_derive of one score (a Score, or one SCORE_DTYPE record) -> dict of dice, iou, precision, recall, hd, hd_q, assd, rmsd"""
    out = ScoreMetrics()
    _check(lib().mi_unet_score_derive(C.byref(_as_score(score)), C.byref(out)))
    return {n: getattr(out, n) for n, _ in ScoreMetrics._fields_}


def _as_score(score):
    if isinstance(score, Score):
        return score
    dirs = [ScoreDir(*[int(score[d][n]) for n, _ in ScoreDir._fields_]) for d in ("a_to_t", "t_to_a")]
    return Score(*[int(score[n]) for n, _ in Score._fields_[:6]], *dirs)


def score_volume_host(pred, truth, values, spacing_units, quantile_ppm=50000, classes=0):
    """mi_unet_score_volume_host: Engine.score_volume as sequential host arithmetic (needs no device)"""
    return _score_volume_call(lib().mi_unet_score_volume_host, (), pred, truth, values, spacing_units, quantile_ppm, classes)


def score_volume_units(spacing_mm, shape):
    """mi_unet_score_volume_units: spacing (sx, sy, sz) in mm and the volume's shape (D, H, W) -> ((ux, uy, uz), unit_mm)"""
    units, unit_mm = (C.c_int * 3)(), C.c_double()
    d, hh, ww = (int(v) for v in shape)
    _check(lib().mi_unet_score_volume_units((C.c_double * 3)(*[float(v) for v in spacing_mm]), d, hh, ww, units, C.byref(unit_mm)))
    return tuple(units), unit_mm.value


def score_volume_derive(score, unit_mm):
    """mi_unet_score_volume_derive of one score (a Score, or one SCORE_DTYPE record) -> dict of dice, iou, precision, recall and hd,
    hd_q, assd, rmsd in mm"""
    out = ScoreMetrics()
    _check(lib().mi_unet_score_volume_derive(C.byref(_as_score(score)), float(unit_mm), C.byref(out)))
    return {n: getattr(out, n) for n, _ in ScoreMetrics._fields_}


def region_derive(region):
    """mi_unet_region_derive of one region (a Region, or one REGION_DTYPE record) -> dict of cx, cy, mean, std, major, minor, theta"""
    if not isinstance(region, Region):
        region = Region(*[int(region[n]) for n, _ in Region._fields_])
    out = RegionShape()
    _check(lib().mi_unet_region_derive(C.byref(region), C.byref(out)))
    return {n: getattr(out, n) for n, _ in RegionShape._fields_}


def shard_range(n_items: int, rank: int, world: int):
    lo, hi = C.c_int(), C.c_int()
    _check(lib().mi_unet_shard_range(n_items, rank, world, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def tile_axis(L: int, T: int, halo: int):
    """The tile grid of one axis (mi_unet_tile_axis): (origins[n], cuts[n + 1]); tile k owns [cuts[k], cuts[k + 1])."""
    n = lib().mi_unet_tile_axis(L, T, halo, None, None)
    if n < 0:
        raise ValueError(f"illegal tile axis: L={L}, T={T}, halo={halo} (need L >= T, halo >= 0, 2 * halo < T)")
    origins, cuts = (C.c_int * n)(), (C.c_int * (n + 1))()
    lib().mi_unet_tile_axis(L, T, halo, origins, cuts)
    return list(origins), list(cuts)


def tile_blend_weights(T: int, mode="gaussian", sigma_scale=0.125, mirror=""):
    """The weight table of one tile axis of length T that the blending kernels use (mi_unet_tile_blend_weights): f32 [T]."""
    w = np.empty(T if T > 0 else 0, np.float32)
    _check(lib().mi_unet_tile_blend_weights(T, C.byref(_tile_blend(mode, sigma_scale, mirror)), _ptr(w)))
    return w


class Group:
    """mi_unet_group_*: one engine + worker thread per device in this process, contiguous image shards."""

    GATHER = {"host": 0, "xgmi": 1}

    def __init__(self, height=512, width=512, in_ch=1, base=64, levels=4, classes=3, max_batch=16, devices=None,
                 n_devices=0, conv_algo="auto"):
        self.cfg = Config(height, width, in_ch, base, levels, classes, max_batch, 0, Engine.CONV_ALGOS[conv_algo])
        self._g = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            _check(lib().mi_unet_group_create(C.byref(self.cfg), arr, len(devices), C.byref(self._g)))
        else:
            _check(lib().mi_unet_group_create(C.byref(self.cfg), None, n_devices, C.byref(self._g)))

    def clone(self) -> "Group":
        other = object.__new__(Group)
        other.cfg = self.cfg
        other._g = C.c_void_p()
        _check(lib().mi_unet_group_clone(self._g, C.byref(other._g)))
        return other

    def close(self):
        if self._g:
            lib().mi_unet_group_destroy(self._g)
            self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return int(lib().mi_unet_group_size(self._g))

    @property
    def weight_transport(self):
        return lib().mi_unet_group_weight_transport(self._g).decode()

    def load_weights(self, blob: bytes):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        _check(lib().mi_unet_group_load_weights_from_memory(self._g, C.cast(buf, C.c_void_p), len(blob)))

    def set_gather(self, mode: str):
        _check(lib().mi_unet_group_set_gather(self._g, self.GATHER[mode]))

    def set_postprocess(self, on: bool):
        _check(lib().mi_unet_group_set_postprocess(self._g, int(on)))

    def set_targets(self, targets):
        """Engine.set_targets on every rank"""
        arr, n = _target_array(targets)
        _check(lib().mi_unet_group_set_targets(self._g, arr, n))

    def set_morph(self, morph):
        """Engine.set_morph on every rank (all or none)"""
        arr, n = _morph_array(morph)
        _check(lib().mi_unet_group_set_morph(self._g, arr, n))

    def set_window(self, mode="minmax", clip_lo_ppm=0, clip_hi_ppm=0, lo=0, hi=65535):
        """Engine.set_window on every rank"""
        _check(lib().mi_unet_group_set_window(self._g, _window(mode, clip_lo_ppm, clip_hi_ppm, lo, hi)))

    def set_measure(self, on=True, channel=0):
        """Engine.set_measure on every rank"""
        _check(lib().mi_unet_group_set_measure(self._g, None if on is None else C.byref(Measure(int(bool(on)), int(channel)))))

    def last_regions(self):
        """Engine.last_regions of the last sharded segment call, planes in image order"""
        return _last_regions(lib().mi_unet_group_last_regions, self._g)

    def _n_targets(self):
        n = C.c_int()
        _check(lib().mi_unet_get_targets(lib().mi_unet_group_handle(self._g, 0), None, 0, C.byref(n)))
        return n.value

    def segment_raw16_multi(self, raws, cap_points=8192, cap_contours=64, raw_arrays=False):
        """Engine.segment_raw16_multi, the batch split across the ranks"""
        raws = [np.ascontiguousarray(r, dtype=np.uint16) for r in raws]
        n, c, k = len(raws), self.cfg, self._n_targets()
        b = n // c.in_ch
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in raws])
        ws = (C.c_int * n)(*[r.shape[1] for r in raws])
        hs = (C.c_int * n)(*[r.shape[0] for r in raws])
        tiles = np.empty((b, c.height, c.width) if c.in_ch == 1 else (b, c.height, c.width, c.in_ch), np.uint8)
        masks = np.empty((b, k, c.height, c.width), np.uint8)
        xy = np.zeros((b, k, cap_points, 2), np.int32)
        start = np.zeros((b, k, cap_contours + 1), np.int32)
        counts = np.zeros((b, k), np.int32)
        _check(lib().mi_unet_group_segment_raw16_multi(self._g, ptrs, ws, hs, b, _ptr(tiles), _ptr(masks), _ptr(xy), cap_points,
                                                       _ptr(start), cap_contours, _ptr(counts)))
        if raw_arrays:
            return tiles, masks, xy, start, counts
        return tiles, masks, _decode_multi(xy, start, counts)

    def infer(self, imgs: np.ndarray, want_logits=False):
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        b, c = imgs.shape[0], self.cfg
        labels = np.empty((b, c.height, c.width), np.uint8)
        logits = np.empty((b, c.classes, c.height, c.width), np.float32) if want_logits else None
        _check(lib().mi_unet_group_infer_u8(self._g, _ptr(imgs), b, _ptr(labels), _ptr(logits)))
        return labels, logits

    def segment_raw16(self, raws, cap_points=8192, cap_contours=64):
        raws = [np.ascontiguousarray(r, dtype=np.uint16) for r in raws]
        n, c = len(raws), self.cfg
        b = n // c.in_ch
        ptrs = (C.c_void_p * n)(*[r.ctypes.data for r in raws])
        ws = (C.c_int * n)(*[r.shape[1] for r in raws])
        hs = (C.c_int * n)(*[r.shape[0] for r in raws])
        tiles = np.empty((b, c.height, c.width) if c.in_ch == 1 else (b, c.height, c.width, c.in_ch), np.uint8)
        masks = np.empty((b, c.height, c.width), np.uint8)
        xy = np.zeros((b, cap_points, 2), np.int32)
        start = np.zeros((b, cap_contours + 1), np.int32)
        counts = np.zeros(b, np.int32)
        _check(lib().mi_unet_group_segment_raw16(self._g, ptrs, ws, hs, b, _ptr(tiles), _ptr(masks), _ptr(xy), cap_points, _ptr(start),
                                                 cap_contours, _ptr(counts)))
        cont = [None if counts[i] < 0 else
                [[tuple(p) for p in xy[i, start[i, k]:start[i, k + 1]].tolist()] for k in range(counts[i])] for i in range(b)]
        return tiles, masks, cont


def _layer_debug_shapes(op, x, w):
    """(pooled, weights, Cout, output shape [B, Ho, Wo, C], pooled shape or None) of a layer hook call"""
    b, h, ww, cin = x.shape
    if op.endswith("_lpout"):         # 16-bit conv ops: the output tensor is 16-bit on the device too
        op = op[:-6]
    pooled = op.endswith("_pool")     # conv3x3 ops: the fused 2x2 max-pooled tensor
    if pooled:
        op = op[:-5]
    cout = 0
    if op.startswith("conv3x3"):
        w = np.ascontiguousarray(w, np.float32)
        cout = w.shape[0]
        shape = (b, h, ww, cout)
    elif op.startswith("convT2x2"):
        w = np.ascontiguousarray(w, np.float32)
        cout = w.shape[1]
        shape = (b, 2 * h, 2 * ww, cout)
    elif op in ("maxpool", "maxpool_bf16", "maxpool_fp16"):            # 16-bit: non-negative input, rounded first
        shape = (b, h // 2, ww // 2, cin)
    elif op in ("upsample2x", "upsample2x_bf16", "upsample2x_fp16"):   # bilinear x2, align_corners=True (16-bit: input rounded first)
        shape = (b, 2 * h, 2 * ww, cin)
    else:
        raise ValueError(op)
    return pooled, w, cout, shape, (b, h // 2, ww // 2, cout) if pooled else None


def layer_debug(op, x, w=None, scale=None, shift=None, relu=False, device=0):
    """Run one layer kernel on host NHWC fp32 data (parity hook)."""
    x = np.ascontiguousarray(x, np.float32)
    b, h, ww, cin = x.shape
    pooled, w, cout, shape, pshape = _layer_debug_shapes(op, x, w)
    out = np.empty(pshape if pooled else shape, np.float32)
    scale = None if scale is None else np.ascontiguousarray(scale, np.float32)
    shift = None if shift is None else np.ascontiguousarray(shift, np.float32)
    _check(lib().mi_unet_layer_debug(device, op.encode(), _ptr(x), b, h, ww, cin, _ptr(w), _ptr(scale), _ptr(shift), cout,
                                     int(relu), _ptr(out)))
    return out


def layer_debug_strided(op, x, w=None, scale=None, shift=None, relu=False, ldc=0, ldo=0, co_off=0, pool_ld=0, guard_bytes=0, device=0):
    """The layer hook in a strided layout between poisoned guards (mi_unet_layer_debug_strided).  Returns a dict: `out` / `pool` the
    complete device allocations as uint8 arrays (pool None without _pool), `elem_bytes`, `kernel` (the route that ran), and the
    geometry of either tensor as the checker takes it: `out_layout` / `pool_layout` = (npix shape [B, Ho, Wo], C, ld, co_off, guard)."""
    x = np.ascontiguousarray(x, np.float32)
    b, h, ww, cin = x.shape
    pooled, w, cout, shape, pshape = _layer_debug_shapes(op, x, w)
    c = shape[3]
    ld, pld = ldo or c, pool_ld or c
    # room for 4-byte elements; the library says which size the op stores (info.elem_bytes) and how much of the buffers it filled
    out = np.empty(2 * guard_bytes + shape[0] * shape[1] * shape[2] * ld * 4, np.uint8)
    pool = np.empty(2 * guard_bytes + pshape[0] * pshape[1] * pshape[2] * pld * 4, np.uint8) if pooled else None
    scale = None if scale is None else np.ascontiguousarray(scale, np.float32)
    shift = None if shift is None else np.ascontiguousarray(shift, np.float32)
    lay = DebugLayout(ldc, ldo, co_off, pool_ld, guard_bytes)
    info = DebugStridedInfo()
    _check(lib().mi_unet_layer_debug_strided(device, op.encode(), _ptr(x), b, h, ww, cin, _ptr(w), _ptr(scale), _ptr(shift), cout, int(relu),
                                             C.byref(lay), _ptr(out), out.nbytes, _ptr(pool), 0 if pool is None else pool.nbytes,
                                             C.byref(info)))
    es = info.elem_bytes
    assert info.out_bytes == 2 * guard_bytes + shape[0] * shape[1] * shape[2] * ld * es
    out = out[:info.out_bytes]
    if pooled:
        assert info.pool_bytes == 2 * guard_bytes + pshape[0] * pshape[1] * pshape[2] * pld * es
        pool = pool[:info.pool_bytes]
    return {"out": out, "pool": pool, "elem_bytes": es, "kernel": info.kernel.decode(),
            "out_layout": (shape[:3], c, ld, co_off, guard_bytes), "pool_layout": (pshape[:3], c, pld, 0, guard_bytes) if pooled else None}
