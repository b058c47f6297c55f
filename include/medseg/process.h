// Per-image pipeline.  Reference: include/process.h:26-30, src/process.cpp:123-262.
#pragma once
#include <string>
#include <vector>

#include "../mi_unet.h"
#include "image.h"

namespace MedicalSeg {

// RAW16 -> <base>_normalized.png + <base>_original_sizes.json -> UNet label map -> postprocess_mask ->
// <base>_mask.png -> <base>_contour_overlay.png + <base>.json.  Returns false (message on stderr and in the log) on failure.
bool process_single_image(const std::string &raw_path, int width, int height, const std::string &output_dir);

// N images in one device call (the reference's directory mode loops process_single_image, src/main.cpp:148-164): min/max,
// resample, quantise, UNet and argmax run on the GPU for the whole batch, the per-image artefacts and the CPU tail follow.
// Returns the number of images that succeeded; failures are reported like process_single_image's.
int process_image_batch(const std::vector<std::string> &raw_paths, const std::vector<int> &widths,
                        const std::vector<int> &heights, const std::string &output_dir);

// Which classes the two functions above segment, and each one's area rule (mi_unet_target in include/mi_unet.h; at most
// MI_UNET_MAX_TARGETS).  The default is { { 2, 0.06f } }: the reference's one foreground class, and with it every artefact is what it
// always was.  With any other list an image gets, in place of <base>_mask.png, one <base>_mask_class<cls>.png (0 / 255) per target,
// one <base>_contour_overlay.png with every target's contours (target k in colour k of Mask2Polygon::draw_overlay's palette) and one
// <base>.json whose shapes carry "label": cls and "labelIndex": k.  set_targets needs an initialised engine (the classes are the
// network's); it returns false, message on stderr, and changes nothing for a list the engine refuses.  An empty list restores the
// default, and so does initialize_engine.
struct Target {
    int cls;
    float min_area_frac;
};
bool set_targets(const std::vector<Target> &targets);
std::vector<Target> get_targets();

// The morphology of the targets' clean-up (mi_unet_morph in include/mi_unet.h): one entry for every target or one per
// target, in target order; an empty list restores the default { { MI_UNET_MORPH_RECT, 1, 0 } }, the reference's 3x3 open, under which
// every artefact is what it always was.  Needs no engine; the setting survives initialize_engine and reaches the group, the second lane
// and every thread's context.  false, message on stderr, setting unchanged: an unknown shape, a radius outside 0 ..
// MI_UNET_MORPH_MAX_R, more than MI_UNET_MAX_TARGETS entries.  A list that is neither 1 nor as long as the target list fails the next
// process call.  No artefact changes its name or format; MEDSEG_HOST_POSTPROCESS=1 applies the same setting on the CPU.
using Morph = mi_unet_morph;
bool set_morphology(const std::vector<Morph> &morph);
std::vector<Morph> get_morphology();

// The intensity window of the RAW input (mi_unet_window in include/mi_unet.h) that the two functions above apply, on the
// device and on the MEDSEG_HOST_PREPROCESS route alike: the default min/max stretch, a percentile clip or a fixed lo..hi.  Needs no
// engine (the setting survives initialize_engine and is handed to every engine, lane and thread context); false, message on stderr,
// and nothing changed for a setting the engine refuses.  Under a non-default window the size JSON of an image gains "window_lo" and
// "window_hi", the window it got; under the default every artefact is what it always was.
bool set_window(const mi_unet_window &window);
mi_unet_window get_window();

// Region measurement (mi_unet_set_measure in include/mi_unet.h).  With it on, the all-device routes of
// process_single_image and process_image_batch measure every contoured region on the device, and each shape of <base>.json gains a
// "region" object (host/json_io.h: area, bbox, centroid, edges, major, minor, theta, mean, std, imin, imax in tile pixels, and the
// scale_x / scale_y that map_contour_points applied); the other artefacts are unchanged byte for byte, and so is every artefact with it
// off.  A shape list the device did not trace (MEDSEG_HOST_POSTPROCESS / _CONTOURS / _PREPROCESS = 1, or a capacity overflow) carries
// no region.  Needs no engine; the setting survives initialize_engine and reaches the group, the second lane and every thread's
// context.  false, setting unchanged: a negative channel, or one the loaded network does not have.
bool set_measure(bool on, int channel = 0);
mi_unet_measure get_measure();

// Scores against ground truth (mi_unet_score_labels in include/mi_unet.h).  With a truth directory set, the two process
// functions look for <dir>/<base>_labels.raw per image: headerless u8 [H][W] class indices at the engine's tile size.  When it is there
// and holds exactly H * W bytes, the final mask of every target is scored against it (the mask as {0, cls}, the truth as == cls), in
// one mi_unet_score_labels call per device call of the batch, and <base>_score.json is written: "quantile_ppm" and per target "label",
// "tp", "fp", "fn", "dice", "iou", "hd", "hd_q", "assd", "rmsd", the distance metrics null when undefined.  A missing file is a log
// line and no score file, a file of another size a warning on stderr and no score file; neither fails the image.  An empty string
// turns it off, which is the default: then every artefact and every log line is what it always was.  Needs no engine and survives
// initialize_engine.  MEDSEG_HOST_POSTPROCESS=1 scores with mi_unet_score_labels_host; the routes with a host tail score image by image.
bool set_truth_dir(const std::string &dir);
std::string get_truth_dir();

// The images of a batch as the slices of one volume (mi_unet_volume_components in include/mi_unet.h).  With it on,
// process_image_batch treats its paths, in the order given, as slices z = 0, 1, ...: whatever the target list is, the batch takes the
// per-target route; the K final 0 / 255 planes of every image are collected into one [K][D][H][W] stack at the TILE size (a slice that
// failed is an all-zero plane), and after the last device call ONE pass labels every target's stack as a volume -- one
// mi_unet_volume_components call per target with values = { 255 } on the group's first engine, mi_unet_volume_components_host under
// MEDSEG_HOST_POSTPROCESS=1.  It writes <output_dir>/volume_report.json: "slices" (base names in z order), "missing" (the slices that
// failed), "connectivity", "min_voxels", "keep_largest", "spacing" and "targets", per target "label", "found", "kept" and "components"
// in table order (at most MI_UNET_VOLUME_MAX_TABLE), per component "voxels", "kept", "bbox" [x0, y0, z0, x1, y1, z1], "centroid_mm",
// "volume_mm3", "surface_mm2", "extent_mm" (mi_unet_volume_derive).  Only when a filter is active (min_voxels > 0 or keep_largest > 0)
// it also writes per slice <base>_volume_mask.png, or <base>_volume_mask_class<cls>.png under a non-default target list: the filtered
// stack, 0 / 255.  Coordinates and spacing are those of the TILE grid -- the masks are at the tile size; spacing_x / _y are millimetres
// per tile pixel, spacing_z per slice; an image's scale_x / scale_y to its own pixels are in its <base>_original_sizes.json.  Every
// artefact that exists without the setting is written exactly as before, and with it off (the default) nothing changes at all.
// With a truth directory set as well (set_truth_dir), the stack -- the filtered one under a filter -- is also scored against
// <dir>/<base>_labels.raw of every slice as ONE volume (mi_unet_score_volume; one call per target, units from
// mi_unet_score_volume_units on the spacing): <output_dir>/volume_score.json with "slices", "unit_mm", "spacing_units", "quantile_ppm"
// and per target "label", "tp", "fp", "fn", "dice", "iou", "hd_mm", "hd_q_mm", "assd_mm", "rmsd_mm".  Only a series whose every slice
// completed and has a truth file of the tile's size is scored; otherwise one log line says how many slices lack mask or truth.
// process_single_image is one slice and ignores the setting.  Needs no engine and survives initialize_engine.  false, message on
// stderr, setting unchanged: a connectivity other than 6, 18, 26, a negative min_voxels or keep_largest, a spacing that is not finite
// and positive.
struct Volume {
    bool on = false;
    int connectivity = 26, min_voxels = 0, keep_largest = 0;
    double spacing_x = 1.0, spacing_y = 1.0, spacing_z = 1.0;
};
bool set_volume(const Volume &volume);
Volume get_volume();

// The stack cleaned as a volume before it is labelled (mi_unet_volume_clean in include/mi_unet.h).  It acts only
// together with set_volume's `on`: before the components are labelled, every target's plane of the stack goes through one
// mi_unet_volume_clean call with values = { 255 } (mi_unet_volume_clean_host under MEDSEG_HOST_POSTPROCESS=1): the 3-D cavity fill
// when `fill`, then a close by a ball of close_mm and an open by a ball of open_mm millimetres under the volume setting's spacing.  The
// integer units come from mi_unet_score_volume_units on that spacing and a radius is llround(mm / unit_mm); a radius or unit past
// MI_UNET_VOLUME_CLEAN_MAX_R is reported as "Volume clean error: ..." and the volume stage of that batch is skipped.  The cleaned stack
// is what set_volume's filter sees and what the volume score scores; it is written per slice as <base>_volume_mask*.png whether or not
// a filter is active, and volume_report.json gains a "clean" object behind "spacing": "fill", "close_mm", "open_mm", "unit_mm",
// "close_r", "open_r" and "targets" with per target "label", "in_voxels", "filled", "closed", "opened", "out_voxels".  One log line per
// batch.  With it off (the default) every artefact and every log line is what it is without the setting.  Needs no engine and
// survives initialize_engine.  false, message on stderr, setting unchanged: a radius that is not finite or is negative.
struct VolumeClean {
    bool on = false;
    bool fill = true;
    double close_mm = 0, open_mm = 0;
};
bool set_volume_clean(const VolumeClean &clean);
VolumeClean get_volume_clean();

// The border of the labelled stack as a surface (mi_unet_volume_mesh in include/mi_unet.h).  It acts only together
// with set_volume's `on`: once the components are labelled, every target's plane that was labelled -- the filtered stack under a
// filter, else the (cleaned) stack -- goes through one mi_unet_volume_mesh call with values = { 255 } (mi_unet_volume_mesh_host under
// MEDSEG_HOST_POSTPROCESS=1) under `placement` (MI_UNET_MESH_FACES or MI_UNET_MESH_NETS), and is written as binary STL in millimetres
// of the volume setting's spacing: <output_dir>/volume_mesh.stl, or volume_mesh_class<cls>.stl under a non-default target list; a
// target without quads writes no file.  The file: an 80-byte header that starts "medseg volume mesh" and is padded with zeros, the
// triangle count as uint32, then per triangle -- (0, 1, 2) and (0, 2, 3) of every quad, in order -- the unit normal of the float
// positions (computed in double, rounded to float; 0, 0, 0 for a zero cross product), the three mi_unet_volume_mesh_positions vertices
// and an attribute of 0.  volume_report.json gains a "mesh" object behind "targets": "placement" and "targets" with per target "label",
// "quads", "verts", "area_mm2", "volume_mm3" (mi_unet_volume_mesh_derive) and "file" (null without quads).  One log line per batch; a
// failure is reported as "Volume mesh error: ..." and ends only this step.  With it off (the default) every artefact and every log
// line is what it is without the setting.  Needs no engine and survives initialize_engine.  false, message on stderr, setting
// unchanged: a placement that is neither of the two.
struct VolumeMesh {
    bool on = false;
    int placement = 0;                                      // MI_UNET_MESH_FACES
};
bool set_volume_mesh(const VolumeMesh &mesh);
VolumeMesh get_volume_mesh();

// Slices put between the slices of the stack before it is meshed (mi_unet_volume_interp in include/mi_unet.h).  It acts
// only together with set_volume's `on`, and it is deliberately narrow: once the components are labelled, every target's plane that the
// mesh would have seen -- the filtered stack under a filter, else the (cleaned) stack -- goes through one mi_unet_volume_interp call with
// values = { 255 } (mi_unet_volume_interp_host under MEDSEG_HOST_POSTPROCESS=1), the in-plane integer units mi_unet_score_volume_units
// finds for the volume setting's spacing, and `factor`; factor 0 means "iso": clamp(llround(spacing_z / min(spacing_x, spacing_y)), 1,
// 16).  With set_volume_mesh on, the mesh step then takes the interpolated stack with spacing_z / factor.  Components, measure, texture,
// score and match stay on the original slices: their reports name slices by file.  volume_report.json gains an "interp" object behind
// "targets" (in front of "mesh"): "factor", "slices", "spacing_z_mm" and "targets" with per target "label", "in_voxels", "out_voxels",
// "mixed", "ties" and "volume_mm3" = out_voxels * spacing_x * spacing_y * spacing_z / factor.  One log line per batch; a failure is
// reported as "Volume interp error: ..." and ends only this step: the mesh then runs on the original stack.  With it off (the default)
// every artefact and every log line is what it is without the setting.  Needs no engine and survives initialize_engine.  false, message
// on stderr, setting unchanged: a factor outside 0 .. MI_UNET_VINTERP_MAX_FACTOR.
struct VolumeInterp {
    bool on = false;
    int factor = 0;                                         // 0 = iso
};
bool set_volume_interp(const VolumeInterp &interp);
VolumeInterp get_volume_interp();

// Every component of the labelled stack measured (mi_unet_volume_measure in include/mi_unet.h).  It acts only together
// with set_volume's `on`: the stack also keeps `channel` of every slice's normalised tile (the bytes of <base>_normalized.png for
// channel 0) widened to 16 bits, a failed slice all-zero; mi_unet_volume_components hands out its ids, and one mi_unet_volume_measure
// call per target (mi_unet_volume_measure_host under MEDSEG_HOST_POSTPROCESS=1) measures the components of the report's table under the
// integer units mi_unet_score_volume_units finds for the volume setting's spacing, with `max_ends` as the cap of the diameter search.
// Every component object of volume_report.json gains a last member "measure": "diameter_mm", "diameter_ends" (two [x, y, z]),
// "axial_diameter_mm", "axial_slice" (the slice's reported name), "axial_ends", "axes_mm", "axes_dir", "mean", "std", "min", "max" and
// "ends"; the four diameter members of a component past the cap are null, and the whole member is null for a component the volume
// filter dropped (its voxels carry no id).  One log line per batch; a failure is reported as "Volume measure error: ..." and ends only
// this step: the report is then written without the member.  With it off (the default) every artefact and every log line is what it is
// without the setting.  Needs no engine and survives initialize_engine.  false, message on stderr, setting unchanged: a negative
// channel, or max_ends outside 0 .. MI_UNET_VMEASURE_MAX_ENDS_LIMIT.  A channel the engine does not have is reported when a batch runs.
struct VolumeMeasure {
    bool on = false;
    int channel = 0;
    int max_ends = 262144;
};
bool set_volume_measure(const VolumeMeasure &measure);
VolumeMeasure get_volume_measure();

// Where the intensity of every component of the labelled stack sits (mi_unet_volume_spatial in include/mi_unet.h).  It
// acts only together with set_volume's `on`: the stack also keeps `channel` of every slice's normalised tile widened to 16 bits (beside
// the channels the other settings keep, when it differs from all of them), a failed slice all-zero; mi_unet_volume_components hands out
// its ids, and one mi_unet_volume_spatial call per target (mi_unet_volume_spatial_host under MEDSEG_HOST_POSTPROCESS=1) takes the
// components of the report's table under the integer units mi_unet_score_volume_units finds for the volume setting's spacing, with
// `max_voxels` as the cap of the pair sums and peak_r = llround(peak_mm / unit_mm) as the radius of the peak sphere (6.2035 mm: the
// sphere of 1 cm^3).  Every component object of volume_report.json gains a last member "spatial": "morans_i", "gearys_c", "pairs",
// "com_shift_mm", "intensity_centroid_mm" ([x, y, z]), "integrated_intensity", "local_peak", "local_peak_at" ([x, y, z]), "global_peak"
// and "global_peak_at"; the first two are null for a component past the cap or of one voxel, and the whole member is null for a component
// the volume filter dropped (its voxels carry no id).  One log line per batch; a failure is reported as "Volume spatial error: ..." and
// ends only this step: the report is then written without the member.  With it off (the default) every artefact and every log line is
// what it is without the setting.  Needs no engine and survives initialize_engine.  false, message on stderr, setting unchanged: a
// negative channel, max_voxels outside 0 .. MI_UNET_VSPATIAL_MAX_VOXELS_LIMIT, or a peak_mm that is not finite and >= 0.  A channel
// the engine does not have, or a sphere past the stage's limits under the batch's units, is reported when a batch runs.
struct VolumeSpatial {
    bool on = false;
    int channel = 0;
    int max_voxels = 131072;
    double peak_mm = 6.2035;
};
bool set_volume_spatial(const VolumeSpatial &spatial);
VolumeSpatial get_volume_spatial();

// Touching objects of the labelled stack split into pieces (mi_unet_volume_split in include/mi_unet.h).  It acts only
// together with set_volume's `on`: behind the components stage, which still applies the size filter, one mi_unet_volume_split call per
// target (mi_unet_volume_split_host under MEDSEG_HOST_POSTPROCESS=1) takes the stack that stage kept, under the setting's connectivity,
// the integer units mi_unet_score_volume_units finds for the volume setting's spacing, neck_r = llround(neck_mm / unit_mm) as
// set_volume_clean converts its radii, and `min_core`.  The PIECES' table, counts and ids then stand where the components' stood for
// everything downstream: the report, measure, texture, zones, nbhood, spatial and the lesion matching of set_volume_match.  Every
// component object of volume_report.json gains a last member "split": "core_voxels", "reach_mm", "cut_mm2"; every target object gains
// a last member "split": "neck_mm", "cores", "cores_kept", "pieces", "coreless".  One log line per batch; a failure is reported as
// "Volume split error: ..." and ends only this step: the report then shows the components, without the members.  With it off (the
// default) every artefact and every log line is what it is without the setting.  Needs no engine and survives initialize_engine.
// false, message on stderr, setting unchanged: a neck_mm that is not finite and >= 0, or a negative min_core.  A neck past the stage's
// limit under the batch's units is reported when a batch runs.
struct VolumeSplit {
    bool on = false;
    double neck_mm = 0.0;
    int min_core = 1;
};
bool set_volume_split(const VolumeSplit &split);
VolumeSplit get_volume_split();

// Every component of the labelled stack thinned to its medial line (mi_unet_volume_skeleton in include/mi_unet.h).  It
// acts only together with set_volume's `on`: one mi_unet_volume_skeleton call per target (mi_unet_volume_skeleton_host under
// MEDSEG_HOST_POSTPROCESS=1) on the ids the components stage hands out -- the pieces' ids with set_volume_split on -- with
// m = min(found, MI_UNET_VOLUME_MAX_TABLE), the integer units mi_unet_score_volume_units finds for the volume setting's spacing and
// `max_passes` (0: until a pass deletes nothing), then mi_unet_volume_skeleton_derive of every row.  Every component object of
// volume_report.json gains a last member "skeleton": "voxels", "ends", "junctions", "isolated", "loops", "length_mm", "radius_min_mm",
// "radius_max_mm", "radius_rms_mm" (the three null with `radius` off, which also skips the distance work) and "stable"; the member is
// null for a component the volume filter dropped.  With `png` per slice <base>_volume_skeleton.png is written (0 / 255; or
// <base>_volume_skeleton_class<cls>.png under a non-default target list).  One log line per batch, "Volume skeleton: D slices, K
// targets, P passes, t ms" (P over all targets); a failure is reported as "Volume skeleton error: ..." and ends only this step.  With it
// off (the default) every artefact and every log line is what it is without the setting.  Needs no engine and survives
// initialize_engine.  false, message on stderr, setting unchanged: a negative max_passes.
struct VolumeSkeleton {
    bool on = false;
    bool radius = true;
    bool png = false;
    int max_passes = 0;
};
bool set_volume_skeleton(const VolumeSkeleton &skeleton);
VolumeSkeleton get_volume_skeleton();

// The skeleton of every component split into nodes and branches (mi_unet_volume_branches in include/mi_unet.h).  It acts
// only together with set_volume's `on` and set_volume_skeleton's `on`: one mi_unet_volume_branches call per target
// (mi_unet_volume_branches_host under MEDSEG_HOST_POSTPROCESS=1) on the skeleton stage's out_ids, and its r2 unless that setting's
// `radius` is off, with `prune_voxels` and `prune_rounds`, tables of 4096 nodes and 4096 branches, then
// mi_unet_volume_branches_derive per component and mi_unet_volume_branches_derive_branch per listed branch.  Every component object of
// volume_report.json gains a last member "branches": "nodes", "ends", "junctions" (junction nodes), "branches", "closed", "parts",
// "loops", "length_mm", "pruned_spurs", a "list" of at most 64 of the component's branches in table order, each with "node_a", "node_b",
// "kind", "voxels", "length_mm", "chord_mm", "tortuosity", "radius_min_mm", "radius_max_mm", "radius_rms_mm" (the three null without
// radii), and "listed" / "found"; "parts" and "loops" are null where the table of 4096 did not hold every branch of the component; the
// member is null for a component the volume filter dropped.  One log line per batch, "Volume branches: D slices, K targets, N nodes, B
// branches, R rounds, t ms" (over all targets); a failure is reported as "Volume branches error: ..." and ends only this step.  With it
// off (the default) every artefact and every log line is what it is without the setting.  Needs no engine and survives
// initialize_engine.  false, message on stderr, setting unchanged: prune_voxels or prune_rounds outside 0 .. 2^20.
struct VolumeBranches {
    bool on = false;
    int prune_voxels = 0;
    int prune_rounds = 0;
};
bool set_volume_branches(const VolumeBranches &branches);
VolumeBranches get_volume_branches();

// The texture of every component of the labelled stack (mi_unet_volume_texture in include/mi_unet.h).  It acts only
// together with set_volume's `on`.  The stack keeps `channel` of every slice's normalised tile widened to 16 bits (beside the channel
// set_volume_measure keeps, when the two differ), a failed slice all-zero; one mi_unet_volume_texture call per target
// (mi_unet_volume_texture_host under MEDSEG_HOST_POSTPROCESS=1) on the ids mi_unet_volume_components hands out, with
// m = min(found, MI_UNET_VOLUME_MAX_TABLE, 2^22 / levels^2) -- the log line says so when that cuts the table short -- and
// mi_unet_volume_texture_derive on every row.  mode is MI_UNET_VTEX_COUNT (levels bins over each component's own range) or
// MI_UNET_VTEX_WIDTH (bins of `width` from `lo`).  Every component object of volume_report.json gains a last member "texture" (behind
// "measure" when both are on): "levels", "mode" ("count" or "width"), "range" ([imin, imax]), "levels_used", "histogram" ("mean",
// "variance", "skewness", "kurtosis", "median", "p10", "p90", "mode", "entropy", "uniformity" and "counts") and "glcm" and "glcm_axial"
// (each "pairs", "joint_max", "joint_average", "joint_variance", "joint_entropy", "contrast", "dissimilarity", "inverse_difference",
// "inverse_difference_moment", "angular_second_moment", "correlation"); a number that is not defined is null, and the member itself is
// null for a component the volume filter dropped or one beyond the measured count.  One log line per batch; a failure is reported as
// "Volume texture error: ..." and ends only this step: the report is then written without the member.  Off (the default), every
// artefact and every log line is what it was.  false with a message: a negative channel, a mode that does not exist, levels outside
// 2 .. 64, lo outside 0 .. 65535 or width outside 1 .. 65536.
struct VolumeTexture {
    bool on = false;
    int channel = 0;
    int mode = 0;                      // MI_UNET_VTEX_COUNT
    int levels = 32;
    int lo = 0;
    int width = 1;
};
bool set_volume_texture(const VolumeTexture &texture);
VolumeTexture get_volume_texture();

// The run-length and size-zone matrices of every component of the labelled stack (mi_unet_volume_zones in include/mi_unet.h, DESIGN.md
// 7.17).  It acts only together with set_volume's `on`.  The stack keeps `channel` of every slice's normalised tile widened to 16 bits
// (beside the channels set_volume_measure and set_volume_texture keep, when they differ), a failed slice all-zero; one
// mi_unet_volume_zones call per target (mi_unet_volume_zones_host under MEDSEG_HOST_POSTPROCESS=1) on the ids mi_unet_volume_components
// hands out, with m = min(found, MI_UNET_VOLUME_MAX_TABLE, 2^22 / (levels * max_run)) -- the log line says so when that cuts the table
// short -- and a zone list of one record per voxel of the stack, at most 2^24; the list is sorted by component once and its slices go to
// mi_unet_volume_zones_zone_features, the rows of both tables to mi_unet_volume_zones_run_features.  mode, levels, lo and width are
// set_volume_texture's; max_run is the length of the last bin of the run tables.  Every component object of volume_report.json gains a
// last member "zones" (behind "texture" when both are on): "levels", "mode" ("count" or "width"), "max_run", "glrlm" and "glrlm_axial"
// ("runs", "clamped", "longest" -- the longest run over the 13 offsets, in both -- and the 16 features of mi_unet_vzone_features by their
// names) and "glszm" ("zones", "largest" and the same 16).  Doubles carry 17 significant digits and a NaN is null.  The member is null
// for a component that the volume filter dropped (no voxel carries its id) or that lies beyond m; "glszm" is null where the zone list
// was cut, and the log says so.  The log gains "Volume zones: D slices, K targets, t ms".  A failure is reported as "Volume zones
// error: ..." and ends only this step: the report is then written without the member.  Off (the default), every artefact and every log
// line is what it was.  false with a message: a negative channel, a mode that does not exist, levels outside 2 .. 64, lo outside
// 0 .. 65535, width outside 1 .. 65536 or max_run outside 2 .. 8192.
struct VolumeZones {
    bool on = false;
    int channel = 0;
    int mode = 0;                      // MI_UNET_VTEX_COUNT
    int levels = 32;
    int lo = 0;
    int width = 1;
    int max_run = 32;
};
bool set_volume_zones(const VolumeZones &zones);
VolumeZones get_volume_zones();

// The neighbourhood-difference, dependence and distance-zone tables of every component of the labelled stack (mi_unet_volume_nbhood in
// include/mi_unet.h).  It acts only together with set_volume's `on`.  The stack keeps `channel` of every slice's
// normalised tile widened to 16 bits (beside the channels set_volume_measure, set_volume_texture and set_volume_zones keep, when it
// differs from all of them), a failed slice all-zero; one mi_unet_volume_nbhood call per target (mi_unet_volume_nbhood_host under
// MEDSEG_HOST_POSTPROCESS=1) on the ids mi_unet_volume_components hands out, all eight tables, with m = min(found,
// MI_UNET_VOLUME_MAX_TABLE, 2^22 / (levels * max(levels, 32, max_dist))) -- the log line says so when that cuts the table short -- and
// the rows of every component go to mi_unet_volume_nbhood_derive, once for the 26 neighbours and once for the 8 in the slice.  mode,
// levels, lo and width are set_volume_texture's; alpha is the largest difference of levels at which a neighbour still depends; max_dist
// is the last bin of the distance-zone tables.  Every component object of volume_report.json gains a last member "nbhood" (behind
// "zones"): "levels", "mode" ("count" or "width"), "alpha", "max_dist", "ngtdm" and "ngtdm_axial" ("valid" and the five features
// "coarseness", "contrast", "busyness", "complexity", "strength"), "ngldm" and "ngldm_axial" ("dependence_max" -- over the 26
// neighbours, in both --, the 16 features of mi_unet_vzone_features by their names and "dependence_energy"), "gldzm" and "gldzm_axial"
// ("zones", "clamped" and the same 16), "deepest" and "deepest_axial".  Doubles carry 17 significant digits and a NaN is null.  The
// member is null for a component that the volume filter dropped (no voxel carries its id) or that lies beyond m.  The log gains
// "Volume nbhood: D slices, K targets, t ms".  A failure is reported as "Volume nbhood error: ..." and ends only this step: the report
// is then written without the member.  Off (the default), every artefact and every log line is what it was.  false with a message: a
// negative channel, a mode that does not exist, levels outside 2 .. 64, lo outside 0 .. 65535, width outside 1 .. 65536, alpha outside
// 0 .. levels - 1 or max_dist outside 1 .. 4096.
struct VolumeNbhood {
    bool on = false;
    int channel = 0;
    int mode = 0;                      // MI_UNET_VTEX_COUNT
    int levels = 32;
    int lo = 0;
    int width = 1;
    int alpha = 0;
    int max_dist = 32;
};
bool set_volume_nbhood(const VolumeNbhood &nbhood);
VolumeNbhood get_volume_nbhood();

// The scored stack per lesion (mi_unet_volume_match in include/mi_unet.h).  It acts only where set_volume's `on` and
// set_truth_dir already produce volume_score.json.  Per target the truth stack, recoded by truth == cls, is labelled with
// mi_unet_volume_components under the volume setting's connectivity, no filter and a table of MI_UNET_VOLUME_MAX_TABLE; the pred ids
// are the ones the volume report numbers, so a pred index is an index into that target's "components" in volume_report.json (a
// component the volume filter dropped carries no voxel and counts as absent).  One mi_unet_volume_match call per target
// (mi_unet_volume_match_host under MEDSEG_HOST_POSTPROCESS=1), then mi_unet_volume_match_assign at iou_num / iou_den and
// mi_unet_volume_match_derive.  Every target object of volume_score.json gains a last member "lesions": "pred", "truth" (components a
// side), "iou_threshold" ([num, den]), "tp", "fp", "fn", "precision", "recall", "f1", "pq", "sq", "rq", "mean_dice" (null where
// undefined), "matches" in pred order ("pred", "truth", "voxels", "iou", "dice", "pred_voxels", "truth_voxels"), "missed" ("truth",
// "voxels"), "spurious" (pred indices) and, only when a side had more components than the table holds, "truncated": true.  One log line
// per batch; a failure is reported as "Volume match error: ..." and ends only this step: volume_score.json is then written without the
// member.  With it off (the default) every artefact and every log line is what it is without the setting.  Needs no engine and
// survives initialize_engine.  false, message on stderr, setting unchanged: a threshold outside 1 <= iou_num <= iou_den <= 65536.
struct VolumeMatch {
    bool on = false;
    int iou_num = 1;
    int iou_den = 2;
};
bool set_volume_match(const VolumeMatch &match);
VolumeMatch get_volume_match();

// The device seam (src/process.cpp:123-175): 8-bit tile -> class-index map through mi_unet_infer_u8.
// Throws std::runtime_error("Inference failed: ...") like the reference.
medseg::Image8 execute_inference(const medseg::Image8 &gray_img);

// Batched form of the same seam for directory mode (src/main.cpp:148-164 loops files one by one): N tiles, one call.
std::vector<medseg::Image8> execute_inference_batch(const std::vector<medseg::Image8> &gray_imgs);

// 0/1/2 -> 0/128/255 (src/process.cpp:178-185)
medseg::Image8 mask_to_image(const medseg::Image8 &mask);

}  // namespace MedicalSeg
