// capi.cpp -- extern "C" wrappers of include/medseg_c.h around the C++ facade.
#include "../../include/medseg_c.h"

#include <cstring>
#include <string>

#include "../../include/medseg/cleanup.h"
#include "../../include/medseg/initialize.h"
#include "../../include/medseg/mask2polygon.h"
#include "../../include/medseg/postprocess.h"
#include "../../include/medseg/preprocess.h"
#include "../../include/medseg/process.h"
#include "png_io.h"

using medseg::Contour;
using medseg::Image8;

namespace {
Image8 wrap(const uint8_t *p, int w, int h, int ch = 1)
{
    Image8 m(h, w, ch);
    memcpy(m.data.data(), p, m.data.size());
    return m;
}
std::vector<Contour> unflatten(const int32_t *xy, const int32_t *start, int n)
{
    std::vector<Contour> cs(n);
    for (int c = 0; c < n; ++c)
        for (int k = start[c]; k < start[c + 1]; ++k) cs[c].emplace_back(xy[2 * k], xy[2 * k + 1]);
    return cs;
}
std::vector<medseg::ClassContours> ungroup(const int32_t *xy, const int32_t *start, const int *group_cls, const int *group_contours, int ngroups)
{
    std::vector<medseg::ClassContours> gs(ngroups);
    int c0 = 0;
    for (int g = 0; g < ngroups; ++g) {
        gs[g].cls = group_cls[g];
        for (int c = c0; c < c0 + group_contours[g]; ++c) {
            Contour cc;
            for (int k = start[c]; k < start[c + 1]; ++k) cc.emplace_back(xy[2 * k], xy[2 * k + 1]);
            gs[g].contours.push_back(std::move(cc));
        }
        c0 += group_contours[g];
    }
    return gs;
}
thread_local std::string t_log_path;
}  // namespace

extern "C" {

int medseg_initialize_engine(const char *weight_path, const char *log_dir)
{
    return MedicalSeg::initialize_engine(weight_path, log_dir) ? 0 : 1;
}
int medseg_process_single_image(const char *raw_path, int width, int height, const char *output_dir)
{
    return MedicalSeg::process_single_image(raw_path, width, height, output_dir) ? 0 : 1;
}
int medseg_process_image_batch(const char *const *raw_paths, const int *widths, const int *heights, int n, const char *output_dir)
{
    std::vector<std::string> p(raw_paths, raw_paths + n);
    return MedicalSeg::process_image_batch(p, std::vector<int>(widths, widths + n), std::vector<int>(heights, heights + n), output_dir);
}
void medseg_cleanup_resources(void) { MedicalSeg::cleanup_resources(); }
const char *medseg_get_log_path(void)
{
    t_log_path = MedicalSeg::get_log_path();
    return t_log_path.c_str();
}

int medseg_preprocess_raw(const char *raw_path, const char *png_path, const char *json_path, int w, int h)
{
    return Preprocess::preprocess_raw(raw_path, png_path, json_path, w, h) ? 0 : 1;
}
int medseg_resample_normalize(const uint16_t *src, int w, int h, uint8_t *dst, int out_w, int out_h)
{
    if (!src || !dst || w <= 0 || h <= 0 || out_w <= 0 || out_h <= 0) return 1;
    const Image8 r = Preprocess::resample_normalize(src, w, h, out_w, out_h);
    memcpy(dst, r.data.data(), r.data.size());
    return 0;
}

int medseg_postprocess_mask(const uint8_t *mask, int w, int h, uint8_t *out)
{
    try {
        const Image8 r = postprocess_mask(wrap(mask, w, h));
        memcpy(out, r.data.data(), r.data.size());
        return 0;
    } catch (...) { return 1; }
}
int medseg_postprocess_mask_target(const uint8_t *mask, int w, int h, int cls, float min_area_frac, uint8_t *out)
{
    try {
        const Image8 r = postprocess_mask(wrap(mask, w, h), cls, min_area_frac);
        memcpy(out, r.data.data(), r.data.size());
        return 0;
    } catch (...) { return 1; }
}
int medseg_set_targets(const int *cls, const float *min_area_frac, int n)
{
    std::vector<MedicalSeg::Target> t;
    for (int i = 0; i < n; ++i) t.push_back({ cls[i], min_area_frac[i] });
    return MedicalSeg::set_targets(t) ? 0 : 1;
}
int medseg_get_targets(int *cls, float *min_area_frac, int cap)
{
    const std::vector<MedicalSeg::Target> t = MedicalSeg::get_targets();
    for (int i = 0; i < (int)t.size() && i < cap; ++i) { cls[i] = t[i].cls; min_area_frac[i] = t[i].min_area_frac; }
    return (int)t.size();
}
int medseg_postprocess_mask_morph(const uint8_t *mask, int w, int h, int cls, float min_area_frac, int shape, int open_r, int close_r,
                                  uint8_t *out)
{
    try {
        const Image8 r = postprocess_mask(wrap(mask, w, h), cls, min_area_frac, mi_unet_morph{ shape, open_r, close_r });
        memcpy(out, r.data.data(), r.data.size());
        return 0;
    } catch (...) { return 1; }
}
int medseg_set_morphology(const int *shape, const int *open_r, const int *close_r, int n)
{
    if (n < 0) return 1;
    std::vector<MedicalSeg::Morph> m;
    for (int i = 0; i < n; ++i) m.push_back({ shape[i], open_r[i], close_r[i] });
    return MedicalSeg::set_morphology(m) ? 0 : 1;
}
int medseg_get_morphology(int *shape, int *open_r, int *close_r, int cap)
{
    const std::vector<MedicalSeg::Morph> m = MedicalSeg::get_morphology();
    for (int i = 0; i < (int)m.size() && i < cap; ++i) { shape[i] = m[i].shape; open_r[i] = m[i].open_r; close_r[i] = m[i].close_r; }
    return (int)m.size();
}
int medseg_set_window(int mode, int clip_lo_ppm, int clip_hi_ppm, int lo, int hi)
{
    return MedicalSeg::set_window(mi_unet_window{ mode, clip_lo_ppm, clip_hi_ppm, lo, hi }) ? 0 : 1;
}
void medseg_get_window(int *mode, int *clip_lo_ppm, int *clip_hi_ppm, int *lo, int *hi)
{
    const mi_unet_window w = MedicalSeg::get_window();
    *mode = w.mode; *clip_lo_ppm = w.clip_lo_ppm; *clip_hi_ppm = w.clip_hi_ppm; *lo = w.lo; *hi = w.hi;
}
int medseg_window_of(const uint16_t *src, size_t n, int mode, int clip_lo_ppm, int clip_hi_ppm, int lo, int hi, int *out_lo, int *out_hi)
{
    if (!src || !out_lo || !out_hi) return 1;
    return Preprocess::window_of(src, n, mi_unet_window{ mode, clip_lo_ppm, clip_hi_ppm, lo, hi }, *out_lo, *out_hi) ? 0 : 1;
}
int medseg_resample_normalize_window(const uint16_t *src, int w, int h, int lo, int hi, uint8_t *dst, int out_w, int out_h)
{
    if (!src || !dst || w <= 0 || h <= 0 || out_w <= 0 || out_h <= 0 || lo < 0 || lo > hi || hi > 65535) return 1;
    const Image8 r = Preprocess::resample_normalize_window(src, w, h, lo, hi, out_w, out_h);
    memcpy(dst, r.data.data(), r.data.size());
    return 0;
}
int medseg_polygon_json_text_groups(const int32_t *xy, const int32_t *start, const int *group_cls, const int *group_contours, int ngroups,
                                    const char *base_name, int original_width, int original_height, char *out, int cap)
{
    const std::string s = Mask2Polygon::polygon_json_text(ungroup(xy, start, group_cls, group_contours, ngroups), base_name, original_width,
                                                          original_height);
    if ((int)s.size() > cap) return -1;
    memcpy(out, s.data(), s.size());
    return (int)s.size();
}
int medseg_set_measure(int on, int channel) { return MedicalSeg::set_measure(on != 0, channel) ? 0 : 1; }
void medseg_get_measure(int *on, int *channel)
{
    const mi_unet_measure m = MedicalSeg::get_measure();
    *on = m.on; *channel = m.channel;
}
int medseg_set_truth_dir(const char *dir) { return MedicalSeg::set_truth_dir(dir ? dir : "") ? 0 : 1; }
int medseg_get_truth_dir(char *out, int cap)
{
    const std::string s = MedicalSeg::get_truth_dir();
    if (!out || (int)s.size() > cap) return -1;
    memcpy(out, s.data(), s.size());
    return (int)s.size();
}
int medseg_set_volume(int on, int connectivity, int min_voxels, int keep_largest, double spacing_x, double spacing_y, double spacing_z)
{
    return MedicalSeg::set_volume({ on != 0, connectivity, min_voxels, keep_largest, spacing_x, spacing_y, spacing_z }) ? 0 : 1;
}
void medseg_get_volume(int *on, int *connectivity, int *min_voxels, int *keep_largest, double *spacing_xyz)
{
    const MedicalSeg::Volume v = MedicalSeg::get_volume();
    *on = v.on; *connectivity = v.connectivity; *min_voxels = v.min_voxels; *keep_largest = v.keep_largest;
    spacing_xyz[0] = v.spacing_x; spacing_xyz[1] = v.spacing_y; spacing_xyz[2] = v.spacing_z;
}
int medseg_set_volume_clean(int on, int fill, double close_mm, double open_mm)
{
    return MedicalSeg::set_volume_clean({ on != 0, fill != 0, close_mm, open_mm }) ? 0 : 1;
}
void medseg_get_volume_clean(int *on, int *fill, double *close_mm, double *open_mm)
{
    const MedicalSeg::VolumeClean c = MedicalSeg::get_volume_clean();
    *on = c.on; *fill = c.fill; *close_mm = c.close_mm; *open_mm = c.open_mm;
}
int medseg_set_volume_mesh(int on, int placement) { return MedicalSeg::set_volume_mesh({ on != 0, placement }) ? 0 : 1; }
void medseg_get_volume_mesh(int *on, int *placement)
{
    const MedicalSeg::VolumeMesh m = MedicalSeg::get_volume_mesh();
    *on = m.on; *placement = m.placement;
}
int medseg_set_volume_interp(int on, int factor) { return MedicalSeg::set_volume_interp({ on != 0, factor }) ? 0 : 1; }
void medseg_get_volume_interp(int *on, int *factor)
{
    const MedicalSeg::VolumeInterp v = MedicalSeg::get_volume_interp();
    if (on) *on = v.on ? 1 : 0;
    if (factor) *factor = v.factor;
}
int medseg_set_volume_measure(int on, int channel, int max_ends) { return MedicalSeg::set_volume_measure({ on != 0, channel, max_ends }) ? 0 : 1; }
void medseg_get_volume_measure(int *on, int *channel, int *max_ends)
{
    const MedicalSeg::VolumeMeasure m = MedicalSeg::get_volume_measure();
    *on = m.on; *channel = m.channel; *max_ends = m.max_ends;
}
int medseg_set_volume_spatial(int on, int channel, int max_voxels, double peak_mm)
{
    return MedicalSeg::set_volume_spatial({ on != 0, channel, max_voxels, peak_mm }) ? 0 : 1;
}
void medseg_get_volume_spatial(int *on, int *channel, int *max_voxels, double *peak_mm)
{
    const MedicalSeg::VolumeSpatial v = MedicalSeg::get_volume_spatial();
    *on = v.on; *channel = v.channel; *max_voxels = v.max_voxels; *peak_mm = v.peak_mm;
}
int medseg_set_volume_split(int on, double neck_mm, int min_core) { return MedicalSeg::set_volume_split({ on != 0, neck_mm, min_core }) ? 0 : 1; }
void medseg_get_volume_split(int *on, double *neck_mm, int *min_core)
{
    const MedicalSeg::VolumeSplit v = MedicalSeg::get_volume_split();
    *on = v.on; *neck_mm = v.neck_mm; *min_core = v.min_core;
}
int medseg_set_volume_skeleton(int on, int radius, int png, int max_passes)
{
    return MedicalSeg::set_volume_skeleton({ on != 0, radius != 0, png != 0, max_passes }) ? 0 : 1;
}
void medseg_get_volume_skeleton(int *on, int *radius, int *png, int *max_passes)
{
    const MedicalSeg::VolumeSkeleton v = MedicalSeg::get_volume_skeleton();
    *on = v.on; *radius = v.radius; *png = v.png; *max_passes = v.max_passes;
}
int medseg_set_volume_branches(int on, int prune_voxels, int prune_rounds)
{
    return MedicalSeg::set_volume_branches({ on != 0, prune_voxels, prune_rounds }) ? 0 : 1;
}
void medseg_get_volume_branches(int *on, int *prune_voxels, int *prune_rounds)
{
    const MedicalSeg::VolumeBranches v = MedicalSeg::get_volume_branches();
    *on = v.on; *prune_voxels = v.prune_voxels; *prune_rounds = v.prune_rounds;
}
int medseg_set_volume_texture(int on, int channel, int mode, int levels, int lo, int width)
{
    return MedicalSeg::set_volume_texture({ on != 0, channel, mode, levels, lo, width }) ? 0 : 1;
}
void medseg_get_volume_texture(int *on, int *channel, int *mode, int *levels, int *lo, int *width)
{
    const MedicalSeg::VolumeTexture t = MedicalSeg::get_volume_texture();
    *on = t.on; *channel = t.channel; *mode = t.mode; *levels = t.levels; *lo = t.lo; *width = t.width;
}
int medseg_set_volume_zones(int on, int channel, int mode, int levels, int lo, int width, int max_run)
{
    return MedicalSeg::set_volume_zones({ on != 0, channel, mode, levels, lo, width, max_run }) ? 0 : 1;
}
void medseg_get_volume_zones(int *on, int *channel, int *mode, int *levels, int *lo, int *width, int *max_run)
{
    const MedicalSeg::VolumeZones z = MedicalSeg::get_volume_zones();
    *on = z.on; *channel = z.channel; *mode = z.mode; *levels = z.levels; *lo = z.lo; *width = z.width; *max_run = z.max_run;
}
int medseg_set_volume_nbhood(int on, int channel, int mode, int levels, int lo, int width, int alpha, int max_dist)
{
    return MedicalSeg::set_volume_nbhood({ on != 0, channel, mode, levels, lo, width, alpha, max_dist }) ? 0 : 1;
}
void medseg_get_volume_nbhood(int *on, int *channel, int *mode, int *levels, int *lo, int *width, int *alpha, int *max_dist)
{
    const MedicalSeg::VolumeNbhood n = MedicalSeg::get_volume_nbhood();
    *on = n.on; *channel = n.channel; *mode = n.mode; *levels = n.levels; *lo = n.lo; *width = n.width; *alpha = n.alpha; *max_dist = n.max_dist;
}
int medseg_set_volume_match(int on, int iou_num, int iou_den) { return MedicalSeg::set_volume_match({ on != 0, iou_num, iou_den }) ? 0 : 1; }
void medseg_get_volume_match(int *on, int *iou_num, int *iou_den)
{
    const MedicalSeg::VolumeMatch m = MedicalSeg::get_volume_match();
    *on = m.on; *iou_num = m.iou_num; *iou_den = m.iou_den;
}
int medseg_polygon_json_text_regions(const int32_t *xy, const int32_t *start, const int *group_cls, const int *group_contours, int ngroups,
                                     const void *regions, double scale_x, double scale_y, const char *base_name, int original_width,
                                     int original_height, char *out, int cap)
{
    try {
        const std::vector<medseg::ClassContours> gs = ungroup(xy, start, group_cls, group_contours, ngroups);
        medseg::RegionTable table;
        table.scale_x = scale_x; table.scale_y = scale_y;
        const mi_unet_region *r = static_cast<const mi_unet_region *>(regions);
        for (const auto &g : gs) {
            table.regions.emplace_back(r ? r : nullptr, r ? r + g.contours.size() : nullptr);
            if (r) r += g.contours.size();
        }
        const std::string s = Mask2Polygon::polygon_json_text(gs, base_name, original_width, original_height, regions ? &table : nullptr);
        if ((int)s.size() > cap) return -1;
        memcpy(out, s.data(), s.size());
        return (int)s.size();
    } catch (...) { return -2; }
}
int medseg_draw_overlay_groups(const uint8_t *gray, int w, int h, const int32_t *xy, const int32_t *start, const int *group_cls,
                               const int *group_contours, int ngroups, uint8_t *bgr_out)
{
    try {
        const Image8 r = Mask2Polygon::draw_overlay(wrap(gray, w, h), ungroup(xy, start, group_cls, group_contours, ngroups));
        memcpy(bgr_out, r.data.data(), r.data.size());
        return 0;
    } catch (...) { return 1; }
}
int medseg_mask_to_image(const uint8_t *mask, int w, int h, uint8_t *out)
{
    const Image8 r = MedicalSeg::mask_to_image(wrap(mask, w, h));
    memcpy(out, r.data.data(), r.data.size());
    return 0;
}

int medseg_extract_contours(const uint8_t *mask, int w, int h, int32_t *xy, int cap_points, int32_t *start, int cap_contours)
{
    const std::vector<Contour> cs = Mask2Polygon::extract_contours(wrap(mask, w, h));
    if ((int)cs.size() > cap_contours) return -1;
    int o = 0;
    for (size_t c = 0; c < cs.size(); ++c) {
        start[c] = o;
        if (o + (int)cs[c].size() > cap_points) return -1;
        for (const auto &p : cs[c]) { xy[2 * o] = p.x; xy[2 * o + 1] = p.y; ++o; }
    }
    start[cs.size()] = o;
    return (int)cs.size();
}
void medseg_map_points(const int32_t *xy, int n, double scale_x, double scale_y, int32_t *out)
{
    Contour c;
    for (int i = 0; i < n; ++i) c.emplace_back(xy[2 * i], xy[2 * i + 1]);
    const auto m = Mask2Polygon::map_contour_points({ c }, scale_x, scale_y);
    for (int i = 0; i < n; ++i) { out[2 * i] = m[0][i].x; out[2 * i + 1] = m[0][i].y; }
}
int medseg_generate_json(const int32_t *xy, const int32_t *start, int ncontours, const char *json_path, const char *base_name,
                         int original_width, int original_height)
{
    try {
        Mask2Polygon::generate_json(unflatten(xy, start, ncontours), json_path, base_name, original_width, original_height);
        return 0;
    } catch (...) { return 1; }
}
int medseg_draw_overlay(const uint8_t *gray, int w, int h, const int32_t *xy, const int32_t *start, int ncontours, uint8_t *bgr_out)
{
    try {
        const Image8 r = Mask2Polygon::draw_overlay(wrap(gray, w, h), unflatten(xy, start, ncontours));
        memcpy(bgr_out, r.data.data(), r.data.size());
        return 0;
    } catch (...) { return 1; }
}
void medseg_process_single_mask(const char *mask_path, const char *output_dir, const char *json_path, const char *original_png,
                                const char *base_name)
{
    Mask2Polygon::process_single_mask(mask_path, output_dir, json_path, original_png ? original_png : "", base_name);
}
int medseg_write_png(const char *path, const uint8_t *data, int w, int h, int channels, int level0)
{
    return medseg::write_png(path, wrap(data, w, h, channels), level0 != 0) ? 0 : 1;
}
int medseg_read_png(const char *path, int as_color, uint8_t *data, int cap_bytes, int *w, int *h)
{
    const Image8 r = medseg::read_png(path, as_color != 0);
    if (r.empty() || (int)r.data.size() > cap_bytes) return 1;
    memcpy(data, r.data.data(), r.data.size());
    *w = r.cols; *h = r.rows;
    return 0;
}

}  // extern "C"
