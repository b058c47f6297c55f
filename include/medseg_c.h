/*
 * medseg_c.h -- C view of the C++ host facade (the headers under include/medseg/) so that tests and non-C++ hosts can drive the same
 * functions the reference exposes as C++ free functions.  Each entry names the reference function it mirrors.
 * All functions return 0 on success, non-zero on failure unless stated otherwise.
 */
#ifndef MEDSEG_C_H
#define MEDSEG_C_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* MedicalSeg::initialize_engine / process_single_image / cleanup_resources (include/initialize.h:12, process.h:29, cleanup.h:7) */
int medseg_initialize_engine(const char *weight_path, const char *log_dir);
int medseg_process_single_image(const char *raw_path, int width, int height, const char *output_dir);
/* MedicalSeg::process_image_batch: n RAW paths of sizes widths[i] x heights[i]; returns the number of successes */
int medseg_process_image_batch(const char *const *raw_paths, const int *widths, const int *heights, int n, const char *output_dir);
void medseg_cleanup_resources(void);
const char *medseg_get_log_path(void);

/* Preprocess::preprocess_raw (include/preprocess.h:20) and its in-memory core (src/preprocess.cpp:81-118) */
int medseg_preprocess_raw(const char *raw_path, const char *png_path, const char *json_path, int w, int h);
int medseg_resample_normalize(const uint16_t *src, int w, int h, uint8_t *dst, int out_w, int out_h);

/* postprocess_mask (src/postprocess.cpp:47) and mask_to_image (src/process.cpp:178) on w*h u8 buffers */
int medseg_postprocess_mask(const uint8_t *mask, int w, int h, uint8_t *out);
int medseg_mask_to_image(const uint8_t *mask, int w, int h, uint8_t *out);

/* postprocess_mask(src, cls, min_area_frac) (include/medseg/postprocess.h): the chain for any class and area rule, output in {0, cls} */
int medseg_postprocess_mask_target(const uint8_t *mask, int w, int h, int cls, float min_area_frac, uint8_t *out);
/* MedicalSeg::set_targets / get_targets: n pairs (cls[i], min_area_frac[i]); n == 0 restores the default.  get returns the count and
 * fills at most cap entries. */
int medseg_set_targets(const int *cls, const float *min_area_frac, int n);
int medseg_get_targets(int *cls, float *min_area_frac, int cap);
/* Morphology (mi_unet_morph in include/mi_unet.h): postprocess_mask(src, cls, min_area_frac, morph) on the CPU, and
 * MedicalSeg::set_morphology / get_morphology as n triples (shape[i], open_r[i], close_r[i]); n == 0 restores the default, no engine
 * needed; set returns 0 on success, 1 and nothing changed otherwise; get returns the count and fills at most cap entries. */
int medseg_postprocess_mask_morph(const uint8_t *mask, int w, int h, int cls, float min_area_frac, int shape, int open_r, int close_r,
                                  uint8_t *out);
int medseg_set_morphology(const int *shape, const int *open_r, const int *close_r, int n);
int medseg_get_morphology(int *shape, int *open_r, int *close_r, int cap);
/* Intensity windows (mi_unet_window in include/mi_unet.h): MedicalSeg::set_window / get_window as (mode, clip_lo_ppm, clip_hi_ppm, lo,
 * hi) -- 0 on success, 1 and nothing changed for a setting the engine refuses; no engine needed -- and the CPU arithmetic:
 * Preprocess::window_of (0 on success) and Preprocess::resample_normalize_window */
int medseg_set_window(int mode, int clip_lo_ppm, int clip_hi_ppm, int lo, int hi);
void medseg_get_window(int *mode, int *clip_lo_ppm, int *clip_hi_ppm, int *lo, int *hi);
int medseg_window_of(const uint16_t *src, size_t n, int mode, int clip_lo_ppm, int clip_hi_ppm, int lo, int hi, int *out_lo, int *out_hi);
int medseg_resample_normalize_window(const uint16_t *src, int w, int h, int lo, int hi, uint8_t *dst, int out_w, int out_h);
/* Region measurement: MedicalSeg::set_measure / get_measure (0 on success; the setting is unchanged on failure), and
 * Mask2Polygon::polygon_json_text for groups with a "region" object per shape: regions holds one mi_unet_region (include/mi_unet.h,
 * 96 bytes) per contour of the flattened list, in tile pixels; scale_x / scale_y are written into every object.  regions == NULL gives
 * the bytes of medseg_polygon_json_text_groups.  Returns the length, -1 when cap bytes are too few, -2 for a region that cannot be
 * derived (area < 1). */
int medseg_set_measure(int on, int channel);
void medseg_get_measure(int *on, int *channel);
/* Scores against ground truth: MedicalSeg::set_truth_dir / get_truth_dir.  NULL or "" turns it off (the default); 0 on success.
 * medseg_get_truth_dir copies the directory (no terminator) into out and returns its length, or -1 when cap is too small. */
int medseg_set_truth_dir(const char *dir);
int medseg_get_truth_dir(char *out, int cap);
/* The images of a batch as the slices of one volume: MedicalSeg::set_volume / get_volume (include/medseg/process.h).  0 on success;
 * medseg_get_volume fills the seven values (spacing: three doubles, x y z). */
int medseg_set_volume(int on, int connectivity, int min_voxels, int keep_largest, double spacing_x, double spacing_y, double spacing_z);
void medseg_get_volume(int *on, int *connectivity, int *min_voxels, int *keep_largest, double *spacing_xyz);
/* The stack cleaned as a volume before it is labelled: MedicalSeg::set_volume_clean / get_volume_clean (include/medseg/process.h).
 * 0 on success; medseg_get_volume_clean fills the four values. */
int medseg_set_volume_clean(int on, int fill, double close_mm, double open_mm);
void medseg_get_volume_clean(int *on, int *fill, double *close_mm, double *open_mm);
/* The border of the labelled stack as binary STL: MedicalSeg::set_volume_mesh / get_volume_mesh (include/medseg/process.h); placement is
 * MI_UNET_MESH_FACES or MI_UNET_MESH_NETS.  0 on success; medseg_get_volume_mesh fills the two values. */
int medseg_set_volume_mesh(int on, int placement);
void medseg_get_volume_mesh(int *on, int *placement);
/* Slices put between the slices of the stack before it is meshed: MedicalSeg::set_volume_interp / get_volume_interp
 * (include/medseg/process.h); factor is 0 ("iso") .. 16.  0 on success; medseg_get_volume_interp fills the two values. */
int medseg_set_volume_interp(int on, int factor);
void medseg_get_volume_interp(int *on, int *factor);
/* Every component of the labelled stack measured: MedicalSeg::set_volume_measure / get_volume_measure (include/medseg/process.h).  0 on
 * success; medseg_get_volume_measure fills the three values. */
int medseg_set_volume_measure(int on, int channel, int max_ends);
void medseg_get_volume_measure(int *on, int *channel, int *max_ends);
/* Where the intensity of every component of the labelled stack sits: MedicalSeg::set_volume_spatial / get_volume_spatial
 * (include/medseg/process.h).  0 on success; medseg_get_volume_spatial fills the four values. */
int medseg_set_volume_spatial(int on, int channel, int max_voxels, double peak_mm);
void medseg_get_volume_spatial(int *on, int *channel, int *max_voxels, double *peak_mm);
/* Touching objects of the labelled stack split into pieces: MedicalSeg::set_volume_split / get_volume_split
 * (include/medseg/process.h).  0 on success; medseg_get_volume_split fills the three values. */
int medseg_set_volume_split(int on, double neck_mm, int min_core);
void medseg_get_volume_split(int *on, double *neck_mm, int *min_core);
/* Every component of the labelled stack thinned to its medial line: MedicalSeg::set_volume_skeleton / get_volume_skeleton
 * (include/medseg/process.h).  0 on success; medseg_get_volume_skeleton fills the four values. */
int medseg_set_volume_skeleton(int on, int radius, int png, int max_passes);
void medseg_get_volume_skeleton(int *on, int *radius, int *png, int *max_passes);
/* Every skeleton split into nodes and branches, short spurs pruned: MedicalSeg::set_volume_branches / get_volume_branches
 * (include/medseg/process.h).  0 on success; medseg_get_volume_branches fills the three values. */
int medseg_set_volume_branches(int on, int prune_voxels, int prune_rounds);
void medseg_get_volume_branches(int *on, int *prune_voxels, int *prune_rounds);
/* The scored stack per lesion: MedicalSeg::set_volume_match / get_volume_match (include/medseg/process.h).  0 on success;
 * medseg_get_volume_match fills the three values. */
int medseg_set_volume_match(int on, int iou_num, int iou_den);
void medseg_get_volume_match(int *on, int *iou_num, int *iou_den);
/* The texture of every component of the labelled stack: MedicalSeg::set_volume_texture / get_volume_texture
 * (include/medseg/process.h).  0 on success; medseg_get_volume_texture fills the six values. */
int medseg_set_volume_texture(int on, int channel, int mode, int levels, int lo, int width);
void medseg_get_volume_texture(int *on, int *channel, int *mode, int *levels, int *lo, int *width);
/* The run-length and size-zone matrices of every component of the labelled stack: MedicalSeg::set_volume_zones / get_volume_zones
 * (include/medseg/process.h).  0 on success; medseg_get_volume_zones fills the seven values. */
int medseg_set_volume_zones(int on, int channel, int mode, int levels, int lo, int width, int max_run);
void medseg_get_volume_zones(int *on, int *channel, int *mode, int *levels, int *lo, int *width, int *max_run);
/* The neighbourhood-difference, dependence and distance-zone tables of every component of the labelled stack:
 * MedicalSeg::set_volume_nbhood / get_volume_nbhood (include/medseg/process.h).  0 on success; medseg_get_volume_nbhood fills the eight
 * values. */
int medseg_set_volume_nbhood(int on, int channel, int mode, int levels, int lo, int width, int alpha, int max_dist);
void medseg_get_volume_nbhood(int *on, int *channel, int *mode, int *levels, int *lo, int *width, int *alpha, int *max_dist);
int medseg_polygon_json_text_regions(const int32_t *xy, const int32_t *start, const int *group_cls, const int *group_contours, int ngroups,
                                     const void *regions, double scale_x, double scale_y, const char *base_name, int original_width,
                                     int original_height, char *out, int cap);
/* Mask2Polygon::polygon_json_text for groups: group g has class group_cls[g] and the next group_contours[g] contours of the flattened
 * list (xy / start as in medseg_generate_json).  Writes the document (no terminator) into out and returns its length, or -1 when cap
 * bytes are too few. */
int medseg_polygon_json_text_groups(const int32_t *xy, const int32_t *start, const int *group_cls, const int *group_contours, int ngroups,
                                    const char *base_name, int original_width, int original_height, char *out, int cap);
/* Mask2Polygon::draw_overlay for groups (same layout): group g in colour g of the palette; bgr_out is w*h*3 bytes */
int medseg_draw_overlay_groups(const uint8_t *gray, int w, int h, const int32_t *xy, const int32_t *start, const int *group_cls,
                               const int *group_contours, int ngroups, uint8_t *bgr_out);

/* Mask2Polygon::extract_contours (src/mask2polygon.cpp:29): xy receives x,y pairs; start[c]..start[c+1] delimits contour c.
 * Returns the number of contours, or -1 when a capacity is too small. */
int medseg_extract_contours(const uint8_t *mask, int w, int h, int32_t *xy, int cap_points, int32_t *start, int cap_contours);
/* map_contour_points (src/mask2polygon.cpp:41) */
void medseg_map_points(const int32_t *xy, int n, double scale_x, double scale_y, int32_t *out);
/* generate_json (src/mask2polygon.cpp:68): writes the document for the given contours */
int medseg_generate_json(const int32_t *xy, const int32_t *start, int ncontours, const char *json_path, const char *base_name,
                         int original_width, int original_height);
/* the picture create_overlay_image writes (src/mask2polygon.cpp:114-129): the grey tile replicated to B,G,R with every contour
 * drawn as a closed red polyline of thickness 1 (cv::drawContours(-1, (0,0,255), 1), LINE_8); bgr_out is w*h*3 bytes */
int medseg_draw_overlay(const uint8_t *gray, int w, int h, const int32_t *xy, const int32_t *start, int ncontours, uint8_t *bgr_out);
/* Mask2Polygon::process_single_mask (src/mask2polygon.cpp:134) */
void medseg_process_single_mask(const char *mask_path, const char *output_dir, const char *json_path, const char *original_png,
                                const char *base_name);
/* PNG helpers standing in for cv::imwrite / cv::imread: channels 1 or 3 (B,G,R) */
int medseg_write_png(const char *path, const uint8_t *data, int w, int h, int channels, int level0);
int medseg_read_png(const char *path, int as_color, uint8_t *data, int cap_bytes, int *w, int *h);

#ifdef __cplusplus
}
#endif
#endif
