// volume_route.cpp -- the volume chain of MedicalSeg::process_image_batch (set_volume): the stages of include/mi_unet.h that take the
// batch's masks as one volume -- clean, components, interpolation, mesh, measure, texture, zones, neighbourhoods, scores against a truth directory, lesion matching -- and
// the reports they write (volume_report.json, volume_score.json, the STL files, the <base>_volume_mask pictures).  routes.cpp fills the
// stack and calls finish_volume; volume_route.h is what the two share.
#include <algorithm>
#include <cmath>
#include <filesystem>
#include <fstream>
#include <functional>
#include <sstream>

#include "json_io.h"
#include "volume_route.h"

namespace fs = std::filesystem;

namespace MedicalSeg {

namespace {

// the spacing of a volume setting and, for a stack of D slices of the engine's tile, the integer units mi_unet_score_volume_units finds for it
struct VolumeUnits {
    double spacing[3];
    int units[3];
    double unit_mm;
};
VolumeUnits volume_units(const Volume &v, size_t D)
{
    VolumeUnits u{ { v.spacing_x, v.spacing_y, v.spacing_z }, { 0, 0, 0 }, 0.0 };
    checked(mi_unet_score_volume_units, u.spacing, (int)D, g_cfg.height, g_cfg.width, u.units, &u.unit_mm);
    return u;
}

// set_volume_clean: every target's plane of the stack through one mi_unet_volume_clean call with values = { 255 } on `h`
// (mi_unet_volume_clean_host under MEDSEG_HOST_POSTPROCESS=1), in place, before label_volume.  The integer units come from
// mi_unet_score_volume_units on the volume setting's spacing; a radius is llround(mm / unit_mm).  `json` receives the "clean" object of
// volume_report.json.  A failure is reported, leaves the stack as it was and returns false: the batch's volume stage ends there.
bool clean_volume(VolumeStack &st, const Settings &s, mi_unet_t *h, std::ostream &lg, std::string &json)
{
    try {
        const std::vector<mi_unet_target> &targets = s.targets;
        const VolumeClean &c = s.volume_clean;
        const size_t K = targets.size(), D = st.D, hw = st.hw;
        const VolumeUnits u = volume_units(s.volume, D);
        auto radius = [&](double mm, const char *which) {
            const double q = mm / u.unit_mm;
            if (!(q < 2147483647.0)) throw std::runtime_error(std::string(which) + " radius is out of range");     // (llround of it must fit an int)
            return (int)std::llround(q);
        };
        const mi_unet_volume_clean_opts opts{ c.fill ? 1 : 0, radius(c.close_mm, "close"), radius(c.open_mm, "open") };
        const int value = 255;
        std::vector<uint8_t> cleaned(K * D * hw);
        std::vector<mi_unet_volume_clean_stat> stats(K);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t)
            stage_call(h, mi_unet_volume_clean, mi_unet_volume_clean_host, st.planes.data() + t * D * hw, (int)D, g_cfg.height, g_cfg.width, &value, 1,
                       u.units, &opts, cleaned.data() + t * D * hw, &stats[t]);
        lg << "Volume clean: " << D << " slices, " << K << " targets, fill " << (c.fill ? "on" : "off") << ", close " << opts.close_r << ", open "
           << opts.open_r << " (unit " << u.unit_mm << " mm), " << ms_since(t0) << " ms" << std::endl;
        std::ostringstream js;
        js << "  \"clean\": {\"fill\": " << (c.fill ? "true" : "false") << ", \"close_mm\": " << json_number(c.close_mm) << ", \"open_mm\": "
           << json_number(c.open_mm) << ", \"unit_mm\": " << json_number(u.unit_mm) << ", \"close_r\": " << opts.close_r << ", \"open_r\": "
           << opts.open_r << ", \"targets\": [";
        for (size_t t = 0; t < K; ++t) {
            const mi_unet_volume_clean_stat &cs = stats[t];
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"in_voxels\": " << cs.in_voxels << ", \"filled\": " << cs.filled
               << ", \"closed\": " << cs.closed << ", \"opened\": " << cs.opened << ", \"out_voxels\": " << cs.out_voxels << "}";
        }
        js << "\n  ]},\n";
        json = js.str();
        st.planes.swap(cleaned);
        return true;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume clean error: ") + e.what());
        return false;
    }
}

// set_volume_mesh: every target's plane of `planes` ([K][D][H][W], the stack label_volume labelled) through mi_unet_volume_mesh with
// values = { 255 } on `h` (mi_unet_volume_mesh_host under MEDSEG_HOST_POSTPROCESS=1) -- a counting call, then one sized by its counts --
// then the positions and metrics under the volume setting's spacing and the STL file of every target that has quads.  Returns the
// "mesh" member of volume_report.json, from its leading comma on.  A failure is reported and returns an empty text: only this step ends.
// `spacing_z` is the distance of the D slices handed in: the volume setting's, or that over the factor behind interp_volume.
std::string mesh_volume(const uint8_t *planes, size_t D, size_t hw, double spacing_z, const Settings &s, mi_unet_t *h, const std::string &output_dir,
                        std::ostream &lg)
{
    try {
        const std::vector<mi_unet_target> &targets = s.targets;
        const size_t K = targets.size();
        const double spacing[3] = { s.volume.spacing_x, s.volume.spacing_y, spacing_z };
        const int value = 255, where = s.volume_mesh.placement;
        const char *const placement = where == MI_UNET_MESH_NETS ? "nets" : "faces";
        std::ostringstream js;
        js << ",\n  \"mesh\": {\"placement\": \"" << placement << "\", \"targets\": [";
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const uint8_t *const in = planes + t * D * hw;
            auto call = [&](mi_unet_mesh_vertex *verts, int cap_verts, int32_t *quads, int cap_quads, mi_unet_mesh_stat *st) {
                stage_call(h, mi_unet_volume_mesh, mi_unet_volume_mesh_host, in, (int)D, g_cfg.height, g_cfg.width, &value, 1, where, verts, cap_verts,
                           quads, cap_quads, st);
            };
            mi_unet_mesh_stat st{};
            call(nullptr, 0, nullptr, 0, &st);
            std::vector<mi_unet_mesh_vertex> verts((size_t)st.verts);
            std::vector<int32_t> quads((size_t)st.quads * 4);
            if (st.quads > 0) call(verts.data(), (int)st.verts, quads.data(), (int)st.quads, &st);
            mi_unet_mesh_metrics m{};
            checked(mi_unet_volume_mesh_derive, verts.data(), (int)verts.size(), quads.data(), (int)st.quads, spacing, &m);
            std::string file;
            if (st.quads > 0) {
                std::vector<float> xyz(verts.size() * 3);
                checked(mi_unet_volume_mesh_positions, verts.data(), (int)verts.size(), spacing, xyz.data());
                file = is_default(targets) ? "volume_mesh.stl" : "volume_mesh_class" + std::to_string(targets[t].cls) + ".stl";
                VolumeMeshArtefact a;
                a.output_dir = output_dir; a.file = file; a.xyz = xyz.data(); a.quads = quads.data(); a.nv = verts.size(); a.nq = (size_t)st.quads;
                write_volume_mesh(a);
            }
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"quads\": " << st.quads << ", \"verts\": " << st.verts
               << ", \"area_mm2\": " << json_number(m.area_mm2) << ", \"volume_mm3\": " << json_number(m.volume_mm3) << ", \"file\": "
               << (file.empty() ? std::string("null") : "\"" + file + "\"") << "}";
        }
        js << "\n  ]}";
        lg << "Volume mesh: " << D << " slices, " << K << " targets, " << placement << ", " << ms_since(t0) << " ms" << std::endl;
        return js.str();
    } catch (const std::exception &e) {
        report(lg, std::string("Volume mesh error: ") + e.what());
        return std::string();
    }
}

// set_volume_interp: every target's plane of `planes` ([K][D][H][W], the stack the mesh would have seen) through one
// mi_unet_volume_interp call with values = { 255 } on `h` (mi_unet_volume_interp_host under MEDSEG_HOST_POSTPROCESS=1) under the in-plane
// units of mi_unet_score_volume_units and the setting's factor (0: spacing_z over the smaller in-plane spacing, 1 .. 16).  `fine` receives
// the interpolated stack [K][D'][H][W] and `factor` the factor used.  Returns the "interp" member of volume_report.json, from its leading
// comma on.  A failure is reported, leaves `fine` empty and returns an empty text: only this step ends.
std::string interp_volume(const uint8_t *planes, size_t D, size_t hw, const Settings &s, mi_unet_t *h, std::ostream &lg, std::vector<uint8_t> &fine,
                          int &factor)
{
    try {
        const std::vector<mi_unet_target> &targets = s.targets;
        const Volume &v = s.volume;
        const size_t K = targets.size();
        const VolumeUnits u = volume_units(v, D);
        factor = s.volume_interp.factor;
        if (factor == 0) {
            const double q = v.spacing_z / std::min(v.spacing_x, v.spacing_y);
            factor = q < 1.0 ? 1 : q > (double)MI_UNET_VINTERP_MAX_FACTOR ? MI_UNET_VINTERP_MAX_FACTOR : (int)std::llround(q);
        }
        const int Dp = mi_unet_volume_interp_slices((int)D, factor);
        if (Dp < 1) throw std::runtime_error(std::to_string(D) + " slices at factor " + std::to_string(factor) + " cannot be interpolated");
        const int value = 255;
        std::vector<uint8_t> out(K * (size_t)Dp * hw);
        std::vector<mi_unet_vinterp_stat> stats(K);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t)
            stage_call(h, mi_unet_volume_interp, mi_unet_volume_interp_host, planes + t * D * hw, (int)D, g_cfg.height, g_cfg.width, &value, 1, u.units,
                       factor, (const uint16_t *)nullptr, out.data() + t * (size_t)Dp * hw, (uint16_t *)nullptr, &stats[t]);
        lg << "Volume interp: " << D << " slices -> " << Dp << ", " << K << " targets, factor " << factor << ", " << ms_since(t0) << " ms" << std::endl;
        std::ostringstream js;
        js << ",\n  \"interp\": {\"factor\": " << factor << ", \"slices\": " << Dp << ", \"spacing_z_mm\": " << json_number(v.spacing_z / factor)
           << ", \"targets\": [";
        for (size_t t = 0; t < K; ++t) {
            const mi_unet_vinterp_stat &is = stats[t];
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"in_voxels\": " << is.in_voxels << ", \"out_voxels\": " << is.out_voxels
               << ", \"mixed\": " << is.mixed << ", \"ties\": " << is.ties << ", \"volume_mm3\": "
               << json_number((double)is.out_voxels * v.spacing_x * v.spacing_y * v.spacing_z / factor) << "}";
        }
        js << "\n  ]}";
        fine.swap(out);
        return js.str();
    } catch (const std::exception &e) {
        report(lg, std::string("Volume interp error: ") + e.what());
        fine.clear();
        return std::string();
    }
}

// set_volume_measure: per target one mi_unet_volume_measure call on `h` (mi_unet_volume_measure_host under MEDSEG_HOST_POSTPROCESS=1) over
// the ids mi_unet_volume_components wrote ([K][D][H][W]) and the stack's intensity, with m = min(found, cap) and the integer units of
// mi_unet_score_volume_units for the volume setting's spacing.  Returns, per target and table row, the "measure" member of the row's
// component object in volume_report.json, from its leading comma on.  A failure is reported and returns nothing: only this step ends.
std::vector<std::vector<std::string>> measure_volume(const VolumeStack &st, const std::vector<int32_t> &ids, const std::vector<int32_t> &found,
                                                     size_t cap, const Settings &s, mi_unet_t *h, std::ostream &lg)
{
    try {
        const size_t K = s.targets.size(), D = st.D, hw = st.hw;
        const int W = g_cfg.width;
        if (s.volume_measure.channel >= g_cfg.in_ch)
            throw std::runtime_error("channel " + std::to_string(s.volume_measure.channel) + " of " + std::to_string(g_cfg.in_ch));
        const VolumeUnits u = volume_units(s.volume, D);
        const mi_unet_vmeasure_opts opts{ s.volume_measure.max_ends };
        std::vector<std::vector<std::string>> members(K);
        auto point = [&](int32_t idx) {
            const size_t p = (size_t)idx % hw;
            return "[" + std::to_string(p % (size_t)W) + ", " + std::to_string(p / (size_t)W) + ", " + std::to_string((size_t)idx / hw) + "]";
        };
        auto ends = [&](int32_t p, int32_t q) { return "[" + point(p) + ", " + point(q) + "]"; };
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const int m = (int)std::min<size_t>((size_t)found[t], cap);
            if (m < 1) continue;
            std::vector<mi_unet_vmeasure> table((size_t)m);
            stage_call(h, mi_unet_volume_measure, mi_unet_volume_measure_host, ids.data() + t * D * hw, st.intensity.data(), (int)D, g_cfg.height,
                       g_cfg.width, m, u.units, &opts, table.data());
            for (const mi_unet_vmeasure &c : table) {
                if (c.voxels < 1) {                             // dropped by the volume filter: its voxels carry no id
                    members[t].push_back(", \"measure\": null");
                    continue;
                }
                mi_unet_vmeasure_shape sh{};
                checked(mi_unet_volume_measure_derive, &c, u.units, u.unit_mm, &sh);
                const bool searched = c.d2 >= 0;
                std::ostringstream js;
                js << ", \"measure\": {\"diameter_mm\": " << (searched ? json_number(sh.diameter_mm) : "null") << ", \"diameter_ends\": "
                   << (searched ? ends(c.dp, c.dq) : "null") << ", \"axial_diameter_mm\": " << (searched ? json_number(sh.axial_diameter_mm) : "null")
                   << ", \"axial_slice\": " << (searched ? "\"" + medseg::json_escape(st.names[(size_t)c.a_p / hw]) + "\"" : std::string("null"))
                   << ", \"axial_ends\": " << (searched ? ends(c.a_p, c.a_q) : "null") << ", \"axes_mm\": [" << json_number(sh.axis_mm[0]) << ", "
                   << json_number(sh.axis_mm[1]) << ", " << json_number(sh.axis_mm[2]) << "], \"axes_dir\": [";
                for (int i = 0; i < 3; ++i)
                    js << (i ? ", " : "") << "[" << json_number(sh.axis_dir[i][0]) << ", " << json_number(sh.axis_dir[i][1]) << ", "
                       << json_number(sh.axis_dir[i][2]) << "]";
                js << "], \"mean\": " << json_number(sh.mean) << ", \"std\": " << json_number(sh.std) << ", \"min\": " << c.imin << ", \"max\": "
                   << c.imax << ", \"ends\": " << c.ends << "}";
                members[t].push_back(js.str());
            }
        }
        lg << "Volume measure: " << D << " slices, " << K << " targets, " << ms_since(t0) << " ms" << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume measure error: ") + e.what());
        return {};
    }
}

using Members = std::vector<std::vector<std::string>>;            // per target and table row, one member of the row's component object

// What the texture stages (texture_volume, zones_volume, nbhood_volume) share: per target, `call(t, m)` runs the stage `name` on the first
// m = min(found, cap, 2^22 / cells) components, then `row(r, js)` writes the object of row r behind "\"<name>\": " and returns whether the
// row has voxels.  A row beyond m, or one the volume filter dropped (no voxel carries its id), gets null.  `at` is what the log says the
// count was cut at, `tail` what a stage adds to its log line.  A failure is reported and returns nothing: only this step ends.
template <class Call, class Row>
Members per_component(const std::string &name, int channel, size_t cells, const std::string &at, const VolumeStack &st, const std::vector<int32_t> &found,
                      size_t cap, const Settings &s, std::ostream &lg, Call call, Row row, const std::function<void()> &tail = [] {})
{
    try {
        const size_t K = s.targets.size();
        if (channel >= g_cfg.in_ch) throw std::runtime_error("channel " + std::to_string(channel) + " of " + std::to_string(g_cfg.in_ch));
        const size_t most = (size_t)MI_UNET_VTEX_MAX_CELLS / cells;
        Members members(K);
        size_t cut = 0;                                         // components beyond the measured count, over all targets
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const size_t rows = std::min<size_t>((size_t)found[t], cap);
            const int m = (int)std::min(rows, most);
            if (m < 1) continue;
            cut += rows - (size_t)m;
            call(t, m);
            for (size_t r = 0; r < rows; ++r) {
                std::ostringstream js;
                js << ", \"" << name << "\": ";
                members[t].push_back(r < (size_t)m && row(r, js) ? js.str() : ", \"" + name + "\": null");
            }
        }
        lg << "Volume " << name << ": " << st.D << " slices, " << K << " targets, " << ms_since(t0) << " ms";
        if (cut) lg << " (the first " << most << " components of a target at " << at << "; " << cut << " not measured)";
        tail();
        lg << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, "Volume " + name + " error: " + e.what());
        return {};
    }
}

// the head of a texture stage's object: the quantiser's levels and mode
void quantiser_head(std::ostream &js, int levels, int mode)
{
    js << "{\"levels\": " << levels << ", \"mode\": \"" << (mode == MI_UNET_VTEX_WIDTH ? "width" : "count") << "\"";
}

// the 16 features of a level-by-size matrix, each from its leading comma on
void matrix_features(std::ostream &js, const mi_unet_vzone_features &f)
{
    const double *const v = &f.short_emphasis;
    static const char *const names[16] = { "short_emphasis", "long_emphasis", "low_grey_emphasis", "high_grey_emphasis", "short_low", "short_high",
                                           "long_low", "long_high", "grey_nonuniformity", "grey_nonuniformity_norm", "size_nonuniformity",
                                           "size_nonuniformity_norm", "percentage", "grey_variance", "size_variance", "entropy" };
    for (int k = 0; k < 16; ++k) js << ", \"" << names[k] << "\": " << json_number(v[k]);
}

// set_volume_texture: per target one mi_unet_volume_texture call on `h` (mi_unet_volume_texture_host under MEDSEG_HOST_POSTPROCESS=1) over
// the ids mi_unet_volume_components wrote ([K][D][H][W]) and the stack's texture channel, with m = min(found, cap, 2^22 / levels^2), then
// mi_unet_volume_texture_derive of every row and of both its tables.  Returns, per target and table row, the "texture" member of the row's
// component object in volume_report.json, from its leading comma on.
Members texture_volume(const VolumeStack &st, const std::vector<int32_t> &ids, const std::vector<int32_t> &found, size_t cap, const Settings &s,
                       mi_unet_t *h, std::ostream &lg)
{
    const VolumeTexture &texture = s.volume_texture;
    const size_t D = st.D, hw = st.hw, L = (size_t)texture.levels;
    const mi_unet_vtexture_opts opts{ texture.mode, texture.levels, texture.lo, texture.width };
    std::vector<mi_unet_vtexture> table;
    std::vector<uint32_t> hist, glcm, axial;
    auto call = [&](size_t t, int m) {
        table.assign((size_t)m, mi_unet_vtexture{});
        hist.assign((size_t)m * L, 0);
        glcm.assign((size_t)m * L * L, 0);
        axial.assign((size_t)m * L * L, 0);
        stage_call(h, mi_unet_volume_texture, mi_unet_volume_texture_host, ids.data() + t * D * hw, st.texture_intensity(), (int)D, g_cfg.height,
                   g_cfg.width, m, &opts, table.data(), hist.data(), glcm.data(), axial.data());
    };
    auto row = [&](size_t r, std::ostream &js) {
        const mi_unet_vtexture &c = table[r];
        if (c.voxels < 1) return false;
        mi_unet_vtexture_features f{}, fa{};
        checked(mi_unet_volume_texture_derive, &c, hist.data() + r * L, glcm.data() + r * L * L, (int)L, &f);
        checked(mi_unet_volume_texture_derive, &c, hist.data() + r * L, axial.data() + r * L * L, (int)L, &fa);
        quantiser_head(js, texture.levels, texture.mode);
        js << ", \"range\": [" << c.imin << ", " << c.imax << "], \"levels_used\": " << c.levels_used << ", \"histogram\": {\"mean\": "
           << json_number(f.mean) << ", \"variance\": " << json_number(f.variance) << ", \"skewness\": " << json_number(f.skewness) << ", \"kurtosis\": "
           << json_number(f.kurtosis) << ", \"median\": " << f.median << ", \"p10\": " << f.p10 << ", \"p90\": " << f.p90 << ", \"mode\": "
           << f.mode << ", \"entropy\": " << json_number(f.entropy) << ", \"uniformity\": " << json_number(f.uniformity) << ", \"counts\": [";
        for (size_t l = 0; l < L; ++l) js << (l ? ", " : "") << hist[r * L + l];
        js << "]}";
        auto joint = [&](const char *key, int64_t pairs, const mi_unet_vtexture_features &g) {
            js << ", \"" << key << "\": {\"pairs\": " << pairs << ", \"joint_max\": " << json_number(g.joint_max) << ", \"joint_average\": "
               << json_number(g.joint_average) << ", \"joint_variance\": " << json_number(g.joint_variance) << ", \"joint_entropy\": "
               << json_number(g.joint_entropy) << ", \"contrast\": " << json_number(g.contrast) << ", \"dissimilarity\": " << json_number(g.dissimilarity)
               << ", \"inverse_difference\": " << json_number(g.inverse_difference) << ", \"inverse_difference_moment\": "
               << json_number(g.inverse_difference_moment) << ", \"angular_second_moment\": " << json_number(g.angular_second_moment)
               << ", \"correlation\": " << json_number(g.correlation) << "}";
        };
        joint("glcm", c.pairs, f);
        joint("glcm_axial", c.pairs_axial, fa);
        js << "}";
        return true;
    };
    return per_component("texture", texture.channel, L * L, std::to_string(L) + " levels", st, found, cap, s, lg, call, row);
}

// set_volume_zones: per target one mi_unet_volume_zones call on `h` (mi_unet_volume_zones_host under MEDSEG_HOST_POSTPROCESS=1) over the
// ids mi_unet_volume_components wrote ([K][D][H][W]) and the stack's zones channel, with m = min(found, cap, 2^22 / (levels * max_run))
// and a zone list of one record per voxel of the stack, at most 2^24; the list is sorted by component once (a stable sort: a
// component's records keep their order), its slices go to mi_unet_volume_zones_zone_features and the rows of both tables to
// mi_unet_volume_zones_run_features.  Returns, per target and table row, the "zones" member of the row's component object in
// volume_report.json, from its leading comma on.
Members zones_volume(const VolumeStack &st, const std::vector<int32_t> &ids, const std::vector<int32_t> &found, size_t cap, const Settings &s,
                     mi_unet_t *h, std::ostream &lg)
{
    const VolumeZones &zs = s.volume_zones;
    const size_t D = st.D, hw = st.hw, L = (size_t)zs.levels, R = (size_t)zs.max_run;
    const mi_unet_vzones_opts opts{ zs.mode, zs.levels, zs.lo, zs.width, zs.max_run };
    const int list_cap = (int)std::min<size_t>(D * hw, (size_t)MI_UNET_VZONES_MAX_CAP);
    size_t lists_cut = 0;                                       // targets whose list was cut
    std::vector<mi_unet_vzones> table;
    std::vector<uint32_t> rlm, axial;
    std::vector<mi_unet_vzone> list;
    std::vector<size_t> first;                                  // component r's records are list[first[r] .. first[r + 1])
    bool whole = true;
    auto call = [&](size_t t, int m) {
        table.assign((size_t)m, mi_unet_vzones{});
        rlm.assign((size_t)m * L * R, 0);
        axial.assign((size_t)m * L * R, 0);
        list.assign((size_t)list_cap, mi_unet_vzone{});
        int n_zones = 0;
        stage_call(h, mi_unet_volume_zones, mi_unet_volume_zones_host, ids.data() + t * D * hw, st.zones_intensity(), (int)D, g_cfg.height,
                   g_cfg.width, m, &opts, table.data(), rlm.data(), axial.data(), list.data(), list_cap, &n_zones);
        whole = n_zones <= list_cap;
        lists_cut += !whole;
        list.resize((size_t)std::min(n_zones, list_cap));
        std::stable_sort(list.begin(), list.end(), [](const mi_unet_vzone &a, const mi_unet_vzone &b) { return a.component < b.component; });
        first.assign((size_t)m + 1, 0);
        for (const mi_unet_vzone &z : list) ++first[(size_t)z.component + 1];
        for (int r = 0; r < m; ++r) first[(size_t)r + 1] += first[(size_t)r];
    };
    auto row = [&](size_t r, std::ostream &js) {
        const mi_unet_vzones &c = table[r];
        if (c.voxels < 1) return false;
        auto runs = [&](const char *key, const uint32_t *cells, int directions, int64_t n, int64_t clamped) {
            mi_unet_vzone_features f{};
            checked(mi_unet_volume_zones_run_features, &c, cells, (int)L, (int)R, directions, &f);
            js << ", \"" << key << "\": {\"runs\": " << n << ", \"clamped\": " << clamped << ", \"longest\": " << c.longest_run;
            matrix_features(js, f);
            js << "}";
        };
        quantiser_head(js, zs.levels, zs.mode);
        js << ", \"max_run\": " << R;
        runs("glrlm", rlm.data() + r * L * R, 13, c.runs, c.clamped);
        runs("glrlm_axial", axial.data() + r * L * R, 4, c.runs_axial, c.clamped_axial);
        if (whole) {
            mi_unet_vzone_features f{};
            checked(mi_unet_volume_zones_zone_features, &c, list.data() + first[r], (int)(first[r + 1] - first[r]), (int)r, (int)L, &f);
            js << ", \"glszm\": {\"zones\": " << c.zones << ", \"largest\": " << c.largest_zone;
            matrix_features(js, f);
            js << "}}";
        } else {
            js << ", \"glszm\": null}";
        }
        return true;
    };
    return per_component("zones", zs.channel, L * R, std::to_string(L) + " levels and run " + std::to_string(R), st, found, cap, s, lg, call, row, [&] {
        if (lists_cut) lg << " (the zone list of " << lists_cut << " targets was cut at " << list_cap << " records: no glszm there)";
    });
}

// set_volume_nbhood: per target one mi_unet_volume_nbhood call on `h` (mi_unet_volume_nbhood_host under MEDSEG_HOST_POSTPROCESS=1) over
// the ids mi_unet_volume_components wrote ([K][D][H][W]) and the stack's neighbourhood channel, all eight tables, with m = min(found,
// cap, 2^22 / (levels * max(levels, 32, max_dist))); the rows of every component go to mi_unet_volume_nbhood_derive twice, for the 26
// neighbours and for the 8 in the slice.  Returns, per target and table row, the "nbhood" member of the row's component object in
// volume_report.json, from its leading comma on.
Members nbhood_volume(const VolumeStack &st, const std::vector<int32_t> &ids, const std::vector<int32_t> &found, size_t cap, const Settings &s,
                      mi_unet_t *h, std::ostream &lg)
{
    const VolumeNbhood &ns = s.volume_nbhood;
    const size_t D = st.D, hw = st.hw, L = (size_t)ns.levels, Dm = (size_t)ns.max_dist;
    const mi_unet_vnbhood_opts opts{ ns.mode, ns.levels, ns.lo, ns.width, ns.alpha, ns.max_dist };
    std::vector<mi_unet_vnbhood> table;
    std::vector<uint32_t> count, dep, count_a, dep_a, dzm, dzm_a;
    std::vector<uint64_t> diff, diff_a;
    auto call = [&](size_t t, int m) {
        const size_t M = (size_t)m;
        table.assign(M, mi_unet_vnbhood{});
        for (std::vector<uint32_t> *v : { &count, &dep }) v->assign(M * L * 27, 0);
        for (std::vector<uint32_t> *v : { &count_a, &dep_a }) v->assign(M * L * 9, 0);
        for (std::vector<uint32_t> *v : { &dzm, &dzm_a }) v->assign(M * L * Dm, 0);
        diff.assign(M * L * 27, 0);
        diff_a.assign(M * L * 9, 0);
        const mi_unet_vnbhood_out out{ count.data(), diff.data(), dep.data(), count_a.data(), diff_a.data(), dep_a.data(), dzm.data(), dzm_a.data() };
        stage_call(h, mi_unet_volume_nbhood, mi_unet_volume_nbhood_host, ids.data() + t * D * hw, st.nbhood_intensity(), (int)D, g_cfg.height,
                   g_cfg.width, m, &opts, table.data(), &out);
    };
    auto row = [&](size_t r, std::ostream &js) {
        const mi_unet_vnbhood &c = table[r];
        if (c.voxels < 1) return false;
        const mi_unet_vnbhood_out rows{ count.data() + r * L * 27, diff.data() + r * L * 27, dep.data() + r * L * 27, count_a.data() + r * L * 9,
                                        diff_a.data() + r * L * 9,  dep_a.data() + r * L * 9,  dzm.data() + r * L * Dm,  dzm_a.data() + r * L * Dm };
        mi_unet_vnbhood_features full{}, axial{};
        checked(mi_unet_volume_nbhood_derive, &c, &rows, (int)L, (int)Dm, 0, &full);
        checked(mi_unet_volume_nbhood_derive, &c, &rows, (int)L, (int)Dm, 1, &axial);
        auto ngtdm = [&](const char *key, const mi_unet_vnbhood_features &f, int valid) {
            js << ", \"" << key << "\": {\"valid\": " << valid << ", \"coarseness\": " << json_number(f.coarseness)
               << ", \"contrast\": " << json_number(f.contrast) << ", \"busyness\": " << json_number(f.busyness)
               << ", \"complexity\": " << json_number(f.complexity) << ", \"strength\": " << json_number(f.strength) << "}";
        };
        auto ngldm = [&](const char *key, const mi_unet_vnbhood_features &f) {
            js << ", \"" << key << "\": {\"dependence_max\": " << c.dependence_max;
            matrix_features(js, f.ngldm);
            js << ", \"dependence_energy\": " << json_number(f.dependence_energy) << "}";
        };
        auto gldzm = [&](const char *key, const mi_unet_vnbhood_features &f, int clamped) {
            js << ", \"" << key << "\": {\"zones\": " << c.zones << ", \"clamped\": " << clamped;
            matrix_features(js, f.gldzm);
            js << "}";
        };
        quantiser_head(js, ns.levels, ns.mode);
        js << ", \"alpha\": " << ns.alpha << ", \"max_dist\": " << Dm;
        ngtdm("ngtdm", full, c.valid);
        ngtdm("ngtdm_axial", axial, c.valid_axial);
        ngldm("ngldm", full);
        ngldm("ngldm_axial", axial);
        gldzm("gldzm", full, c.clamped);
        gldzm("gldzm_axial", axial, c.clamped_axial);
        js << ", \"deepest\": " << c.deepest << ", \"deepest_axial\": " << c.deepest_axial << "}";
        return true;
    };
    return per_component("nbhood", ns.channel, L * std::max<size_t>({ L, 32, Dm }), std::to_string(L) + " levels and dist " + std::to_string(Dm), st, found,
                         cap, s, lg, call, row);
}

// set_volume_spatial: per target one mi_unet_volume_spatial call on `h` (mi_unet_volume_spatial_host under MEDSEG_HOST_POSTPROCESS=1) over
// the ids mi_unet_volume_components wrote ([K][D][H][W]) and the stack's spatial channel, with m = min(found, cap), the integer units of
// mi_unet_score_volume_units for the volume setting's spacing and peak_r = llround(peak_mm / unit_mm), then
// mi_unet_volume_spatial_derive of every row.  Returns, per target and table row, the "spatial" member of the row's component object in
// volume_report.json, from its leading comma on.  A failure is reported and returns nothing: only this step ends.
Members spatial_volume(const VolumeStack &st, const std::vector<int32_t> &ids, const std::vector<int32_t> &found, size_t cap, const Settings &s,
                       mi_unet_t *h, std::ostream &lg)
{
    try {
        const size_t K = s.targets.size(), D = st.D, hw = st.hw;
        const int W = g_cfg.width;
        const VolumeSpatial &sp = s.volume_spatial;
        if (sp.channel >= g_cfg.in_ch) throw std::runtime_error("channel " + std::to_string(sp.channel) + " of " + std::to_string(g_cfg.in_ch));
        const VolumeUnits u = volume_units(s.volume, D);
        const double r = sp.peak_mm / u.unit_mm;
        if (!(r <= (double)MI_UNET_VOLUME_CLEAN_MAX_R))
            throw std::runtime_error("a peak sphere of " + json_number(sp.peak_mm) + " mm is more than " + std::to_string(MI_UNET_VOLUME_CLEAN_MAX_R) + " units");
        const mi_unet_vspatial_opts opts{ sp.max_voxels, (int)std::llround(r) };
        Members members(K);
        auto point = [&](int32_t idx) {
            const size_t p = (size_t)idx % hw;
            return "[" + std::to_string(p % (size_t)W) + ", " + std::to_string(p / (size_t)W) + ", " + std::to_string((size_t)idx / hw) + "]";
        };
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const int m = (int)std::min<size_t>((size_t)found[t], cap);
            if (m < 1) continue;
            std::vector<mi_unet_vspatial> table((size_t)m);
            stage_call(h, mi_unet_volume_spatial, mi_unet_volume_spatial_host, ids.data() + t * D * hw, st.spatial_intensity(), (int)D, g_cfg.height,
                       g_cfg.width, m, u.units, &opts, table.data());
            for (const mi_unet_vspatial &c : table) {
                if (c.voxels < 1) {                             // dropped by the volume filter: its voxels carry no id
                    members[t].push_back(", \"spatial\": null");
                    continue;
                }
                mi_unet_vspatial_metrics f{};
                checked(mi_unet_volume_spatial_derive, &c, u.units, u.unit_mm, &f);
                std::ostringstream js;
                js << ", \"spatial\": {\"morans_i\": " << json_number(f.morans_i) << ", \"gearys_c\": " << json_number(f.gearys_c) << ", \"pairs\": "
                   << c.pairs << ", \"com_shift_mm\": " << json_number(f.com_shift_mm) << ", \"intensity_centroid_mm\": [" << json_number(f.icx_mm)
                   << ", " << json_number(f.icy_mm) << ", " << json_number(f.icz_mm) << "], \"integrated_intensity\": "
                   << json_number(f.integrated_intensity) << ", \"local_peak\": " << json_number(f.local_peak) << ", \"local_peak_at\": "
                   << point(c.lp_at) << ", \"global_peak\": " << json_number(f.global_peak) << ", \"global_peak_at\": " << point(c.gp_at) << "}";
                members[t].push_back(js.str());
            }
        }
        lg << "Volume spatial: " << D << " slices, " << K << " targets, peak radius " << opts.peak_r << " units, " << ms_since(t0) << " ms" << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume spatial error: ") + e.what());
        return {};
    }
}

// set_volume_split: per target one mi_unet_volume_split call on `h` (mi_unet_volume_split_host under MEDSEG_HOST_POSTPROCESS=1) over
// `labelled` ([K][D][H][W], the stack the components stage kept) with values = { 255 }, the volume setting's connectivity, the integer
// units of mi_unet_score_volume_units and neck_r = llround(neck_mm / unit_mm).  On success the pieces' table, counts and (when `ids` is
// not empty) ids stand where the components' stood -- every piece is kept -- and `members` / `target_members` hold the "split" member of
// every row and of every target, from its leading comma on.  A failure is reported and leaves everything as the components stage
// wrote it: only this step ends.
struct SplitMembers {
    std::vector<std::vector<std::string>> rows;
    std::vector<std::string> targets;
};
SplitMembers split_volume(const uint8_t *labelled, size_t D, size_t hw, size_t cap, const Settings &s, mi_unet_t *h, std::ostream &lg,
                          std::vector<mi_unet_vcomp> &table, std::vector<int32_t> &found, std::vector<int32_t> &kept, std::vector<int32_t> &ids)
{
    try {
        const size_t K = s.targets.size();
        const VolumeSplit &sp = s.volume_split;
        const VolumeUnits u = volume_units(s.volume, D);
        const double q = sp.neck_mm / u.unit_mm;
        if (!(q <= (double)MI_UNET_VOLUME_CLEAN_MAX_R))
            throw std::runtime_error("a neck of " + json_number(sp.neck_mm) + " mm is more than " + std::to_string(MI_UNET_VOLUME_CLEAN_MAX_R) + " units");
        const mi_unet_vsplit_opts opts{ s.volume.connectivity, (int)std::llround(q), sp.min_core };
        const double spacing[3] = { s.volume.spacing_x, s.volume.spacing_y, s.volume.spacing_z };
        const int value = 255;
        std::vector<mi_unet_vcomp> pieces(K * cap);
        std::vector<mi_unet_vpiece> info(K * cap);
        std::vector<int32_t> piece_ids(ids.size()), piece_found(K);
        std::vector<mi_unet_vsplit_stat> stats(K);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t)
            stage_call(h, mi_unet_volume_split, mi_unet_volume_split_host, labelled + t * D * hw, (int)D, g_cfg.height, g_cfg.width, &value, 1, u.units,
                       &opts, piece_ids.empty() ? nullptr : piece_ids.data() + t * D * hw, pieces.data() + t * cap, info.data() + t * cap, (int)cap,
                       &piece_found[t], &stats[t], nullptr);
        SplitMembers m;
        m.rows.resize(K);
        m.targets.resize(K);
        int64_t all = 0;
        for (size_t t = 0; t < K; ++t) {
            const size_t rows = std::min<size_t>((size_t)piece_found[t], cap);
            for (size_t r = 0; r < rows; ++r) {
                const mi_unet_vpiece &p = info[t * cap + r];
                mi_unet_vpiece_metrics pm{};
                checked(mi_unet_volume_split_derive, &p, spacing, u.unit_mm, &pm);
                m.rows[t].push_back(", \"split\": {\"core_voxels\": " + std::to_string(p.core_voxels) + ", \"reach_mm\": " + json_number(pm.reach_mm) +
                                    ", \"cut_mm2\": " + json_number(pm.cut_mm2) + "}");
            }
            const mi_unet_vsplit_stat &st = stats[t];
            m.targets[t] = ", \"split\": {\"neck_mm\": " + json_number(sp.neck_mm) + ", \"cores\": " + std::to_string(st.cores) + ", \"cores_kept\": " +
                           std::to_string(st.cores_kept) + ", \"pieces\": " + std::to_string(st.pieces) + ", \"coreless\": " +
                           std::to_string(st.coreless) + "}";
            all += st.pieces;
        }
        lg << "Volume split: " << D << " slices, " << K << " targets, neck " << opts.neck_r << " units (unit " << u.unit_mm << " mm), " << all
           << " pieces, " << ms_since(t0) << " ms" << std::endl;
        table.swap(pieces);
        ids.swap(piece_ids);
        kept = piece_found;
        found.swap(piece_found);
        return m;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume split error: ") + e.what());
        return {};
    }
}

// set_volume_skeleton: per target one mi_unet_volume_skeleton call on `h` (mi_unet_volume_skeleton_host under MEDSEG_HOST_POSTPROCESS=1) over
// the ids the components stage -- or split_volume -- wrote ([K][D][H][W]), with m = min(found, cap), the integer units of
// mi_unet_score_volume_units for the volume setting's spacing and the setting's max_passes, then mi_unet_volume_skeleton_derive of every
// row.  Returns, per target and table row, the "skeleton" member of the row's component object in volume_report.json, from its leading
// comma on; with the setting's png, `picture` receives the skeletons as 0 / 255 ([K][D][H][W]).  With set_volume_branches on, `lines`
// receives the skeletons' ids ([K][D][H][W]) and, unless `radius` is off, `radii` their r2.  A failure is reported, returns nothing
// and leaves `picture` empty: only this step ends.
Members skeleton_volume(size_t D, size_t hw, const std::vector<int32_t> &ids, const std::vector<int32_t> &found, size_t cap, const Settings &s,
                        mi_unet_t *h, std::ostream &lg, std::vector<uint8_t> &picture, std::vector<int32_t> &lines, std::vector<int32_t> &radii)
{
    try {
        const size_t K = s.targets.size();
        const VolumeSkeleton &sk = s.volume_skeleton;
        const bool keep = s.volume_branches.on;
        std::vector<int32_t> kept_ids(keep ? K * D * hw : 0), kept_r2(keep && sk.radius ? K * D * hw : 0);
        const VolumeUnits u = volume_units(s.volume, D);
        const mi_unet_vskel_opts opts{ sk.max_passes, sk.radius ? 1 : 0 };
        Members members(K);
        std::vector<uint8_t> drawn(sk.png ? K * D * hw : 0);
        std::vector<int32_t> thin(sk.png || keep ? D * hw : 0);
        int64_t passes = 0;
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const int m = (int)std::min<size_t>((size_t)found[t], cap);
            if (m < 1) continue;
            std::vector<mi_unet_vskel> table((size_t)m);
            mi_unet_vskel_info info{};
            stage_call(h, mi_unet_volume_skeleton, mi_unet_volume_skeleton_host, ids.data() + t * D * hw, (int)D, g_cfg.height, g_cfg.width, m, u.units,
                       &opts, thin.empty() ? nullptr : thin.data(), kept_r2.empty() ? nullptr : kept_r2.data() + t * D * hw, table.data(), &info);
            passes += info.passes;
            for (size_t i = 0; i < drawn.size() / K; ++i) drawn[t * D * hw + i] = thin[i] > 0 ? 255 : 0;
            if (keep) std::copy(thin.begin(), thin.end(), kept_ids.begin() + t * D * hw);
            for (const mi_unet_vskel &c : table) {
                if (c.voxels_in < 1) {                          // dropped by the volume filter: its voxels carry no id
                    members[t].push_back(", \"skeleton\": null");
                    continue;
                }
                mi_unet_vskel_metrics f{};
                checked(mi_unet_volume_skeleton_derive, &c, u.spacing, u.unit_mm, &f);
                auto radius = [&](double mm) { return sk.radius ? json_number(mm) : std::string("null"); };
                std::ostringstream js;
                js << ", \"skeleton\": {\"voxels\": " << c.voxels << ", \"ends\": " << c.ends << ", \"junctions\": " << c.junctions << ", \"isolated\": "
                   << c.isolated << ", \"loops\": " << f.loops << ", \"length_mm\": " << json_number(f.length_mm) << ", \"radius_min_mm\": "
                   << radius(f.radius_min_mm) << ", \"radius_max_mm\": " << radius(f.radius_max_mm) << ", \"radius_rms_mm\": "
                   << radius(f.radius_rms_mm) << ", \"stable\": " << info.stable << "}";
                members[t].push_back(js.str());
            }
        }
        lg << "Volume skeleton: " << D << " slices, " << K << " targets, " << passes << " passes, " << ms_since(t0) << " ms" << std::endl;
        picture.swap(drawn);
        lines.swap(kept_ids);
        radii.swap(kept_r2);
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume skeleton error: ") + e.what());
        picture.clear();
        lines.clear();
        radii.clear();
        return {};
    }
}

// set_volume_branches: per target one mi_unet_volume_branches call on `h` (mi_unet_volume_branches_host under MEDSEG_HOST_POSTPROCESS=1) over
// the skeletons skeleton_volume kept (`lines` [K][D][H][W], `radii` the same or empty), with m = min(found, cap), the setting's pruning and
// tables of kRows nodes and branches, then mi_unet_volume_branches_derive per component and mi_unet_volume_branches_derive_branch per
// listed branch.  Returns, per target and table row, the "branches" member of the row's component object in volume_report.json, from its
// leading comma on.  A failure is reported and returns nothing: only this step ends.
Members branches_volume(size_t D, size_t hw, const std::vector<int32_t> &lines, const std::vector<int32_t> &radii, const std::vector<int32_t> &found,
                        size_t cap, const Settings &s, mi_unet_t *h, std::ostream &lg)
{
    constexpr int kRows = 4096, kListed = 64;
    try {
        const size_t K = s.targets.size();
        const VolumeUnits u = volume_units(s.volume, D);
        const mi_unet_vbranch_opts opts{ s.volume_branches.prune_voxels, s.volume_branches.prune_rounds };
        Members members(K);
        std::vector<mi_unet_vnode> nodes(kRows);
        std::vector<mi_unet_vbranch> rows(kRows);
        int64_t n_nodes = 0, n_branches = 0, rounds = 0;
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            const int m = (int)std::min<size_t>((size_t)found[t], cap);
            if (m < 1) continue;
            std::vector<mi_unet_vgraph> graph((size_t)m);
            mi_unet_vbranch_info info{};
            stage_call(h, mi_unet_volume_branches, mi_unet_volume_branches_host, lines.data() + t * D * hw,
                       radii.empty() ? nullptr : radii.data() + t * D * hw, (int)D, g_cfg.height, g_cfg.width, m, u.units, &opts, nodes.data(), kRows,
                       rows.data(), kRows, graph.data(), nullptr, nullptr, &info);
            n_nodes += info.found_nodes; n_branches += info.found_branches; rounds += info.rounds;
            const int64_t held = std::min<int64_t>(info.found_branches, kRows);
            for (int r = 0; r < m; ++r) {
                const mi_unet_vgraph &g = graph[r];
                if (g.nodes + g.branches + g.pruned_voxels < 1) {   // no skeleton voxel: dropped by the volume filter
                    members[t].push_back(", \"branches\": null");
                    continue;
                }
                mi_unet_vgraph_metrics f{};
                int64_t mine = 0;
                for (int64_t b = 0; b < held; ++b) mine += rows[b].id == r + 1;
                const bool whole = mine >= g.branches;
                if (whole) checked(mi_unet_volume_branches_derive, &g, rows.data(), held, info.found_nodes, r + 1, u.spacing, u.unit_mm, &f);
                else f.length_mm = 0.0;
                std::ostringstream js;
                js << ", \"branches\": {\"nodes\": " << g.nodes << ", \"ends\": " << g.ends << ", \"junctions\": " << g.junction_nodes << ", \"branches\": "
                   << g.branches << ", \"closed\": " << g.closed << ", \"parts\": " << (whole ? std::to_string(f.parts) : "null") << ", \"loops\": "
                   << (whole ? std::to_string(f.loops) : "null") << ", \"length_mm\": ";
                if (!whole) {                                       // the length needs the per-id links alone
                    mi_unet_vgraph bare = g;
                    bare.branches = 0;
                    checked(mi_unet_volume_branches_derive, &bare, rows.data(), (int64_t)0, info.found_nodes, r + 1, u.spacing, u.unit_mm, &f);
                }
                js << json_number(f.length_mm) << ", \"pruned_spurs\": " << g.pruned_spurs << ", \"list\": [";
                int listed = 0;
                for (int64_t b = 0; b < held && listed < kListed; ++b) {
                    if (rows[b].id != r + 1) continue;
                    mi_unet_vbranch_metrics bm{};
                    checked(mi_unet_volume_branches_derive_branch, &rows[b], g_cfg.height, g_cfg.width, u.spacing, u.unit_mm, &bm);
                    auto radius = [&](double mm) { return radii.empty() ? std::string("null") : json_number(mm); };
                    js << (listed ? ", " : "") << "{\"node_a\": " << rows[b].node_a << ", \"node_b\": " << rows[b].node_b << ", \"kind\": " << rows[b].kind
                       << ", \"voxels\": " << rows[b].voxels << ", \"length_mm\": " << json_number(bm.length_mm) << ", \"chord_mm\": "
                       << json_number(bm.chord_mm) << ", \"tortuosity\": " << json_number(bm.tortuosity) << ", \"radius_min_mm\": "
                       << radius(bm.radius_min_mm) << ", \"radius_max_mm\": " << radius(bm.radius_max_mm) << ", \"radius_rms_mm\": "
                       << radius(bm.radius_rms_mm) << "}";
                    ++listed;
                }
                js << "], \"listed\": " << listed << ", \"found\": " << g.branches << "}";
                members[t].push_back(js.str());
            }
        }
        lg << "Volume branches: " << D << " slices, " << K << " targets, " << n_nodes << " nodes, " << n_branches << " branches, " << rounds
           << " rounds, " << ms_since(t0) << " ms" << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume branches error: ") + e.what());
        return {};
    }
}

// One mi_unet_volume_components call per target with values = { 255 } on `h` (mi_unet_volume_components_host under
// MEDSEG_HOST_POSTPROCESS=1), then volume_report.json and, under a filter, the <base>_volume_mask pictures.  A failure is reported and
// fails no image.  Under a filter `filtered` receives the filtered stack [K][D][H][W]; it stays empty without one, or after a failure.
// A stack that clean_volume cleaned comes with its "clean" object for the report and is written as pictures whether or not a filter
// is active (without one they are the cleaned stack itself).  With set_volume_mesh on, the planes that were labelled -- `out` under a
// filter, else the stack -- are meshed (mesh_volume) and the report gains the "mesh" object behind "targets"; with set_volume_interp on
// those planes are interpolated first (interp_volume), the report gains the "interp" object in front of "mesh", and the mesh sees the
// interpolated stack.  With set_volume_measure on,
// the components stage also hands out its ids, they are measured (measure_volume) and every component object gains a last member
// "measure".  With set_volume_texture on, the ids are handed out likewise and every component object gains a last member "texture"
// (texture_volume), with set_volume_zones on a last member "zones" behind it (zones_volume), and with set_volume_nbhood on a last member
// "nbhood" behind that (nbhood_volume), and with set_volume_spatial on a last member "spatial" behind them all (spatial_volume).  With set_volume_split on, the planes that were labelled are split behind the components stage
// (split_volume) and everything below -- the report, the stages above, `numbered` -- takes the pieces' table, counts and ids; every
// component object gains a last member "split" and every target object one too.  With `numbered` given (set_volume_match) the ids [K][D][H][W] and the counts per target are handed out too; it stays
// empty after a failure.
struct VolumeIds {
    std::vector<int32_t> ids, found;
};
void label_volume(const VolumeStack &st, const Settings &s, mi_unet_t *h, const std::string &output_dir, std::ostream &lg,
                  std::vector<uint8_t> &filtered, const std::string &clean_json, VolumeIds *numbered)
{
    filtered.clear();
    try {
        const std::vector<mi_unet_target> &targets = s.targets;
        const Volume &v = s.volume;
        const size_t K = targets.size(), D = st.D, hw = st.hw, cap = MI_UNET_VOLUME_MAX_TABLE;
        const bool filter = v.min_voxels > 0 || v.keep_largest > 0 || !clean_json.empty();
        std::vector<uint8_t> out(filter ? K * D * hw : 0);
        std::vector<mi_unet_vcomp> table(K * cap);
        std::vector<int32_t> found(K), kept(K), ids(s.volume_measure.on || s.volume_texture.on || s.volume_zones.on || s.volume_nbhood.on || s.volume_spatial.on || s.volume_skeleton.on || numbered ? K * D * hw : 0);
        const mi_unet_volume_opts opts{ v.connectivity, v.min_voxels, v.keep_largest };
        const int value = 255;
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t)
            stage_call(h, mi_unet_volume_components, mi_unet_volume_components_host, st.planes.data() + t * D * hw, (int)D, g_cfg.height, g_cfg.width,
                       &value, 1, &opts, filter ? out.data() + t * D * hw : nullptr, ids.empty() ? nullptr : ids.data() + t * D * hw,
                       table.data() + t * cap, (int)cap, &found[t], &kept[t]);
        lg << "Volume: " << D << " slices, " << K << " targets, connectivity " << v.connectivity << ", " << ms_since(t0) << " ms" << std::endl;
        // the stack the mesh sees: with set_volume_interp on, its interpolated form under spacing_z / factor (the original after a failure)
        const uint8_t *const labelled = filter ? out.data() : st.planes.data();
        const SplitMembers split = s.volume_split.on ? split_volume(labelled, D, hw, cap, s, h, lg, table, found, kept, ids) : SplitMembers();
        std::vector<uint8_t> fine;
        int factor = 1;
        const std::string interp_json = s.volume_interp.on ? interp_volume(labelled, D, hw, s, h, lg, fine, factor) : std::string();
        const bool use_fine = !fine.empty();
        const std::string mesh_json = !s.volume_mesh.on ? std::string()
                                      : use_fine ? mesh_volume(fine.data(), fine.size() / (K * hw), hw, v.spacing_z / factor, s, h, output_dir, lg)
                                                 : mesh_volume(labelled, D, hw, v.spacing_z, s, h, output_dir, lg);
        const std::vector<std::vector<std::string>> measured =
            s.volume_measure.on ? measure_volume(st, ids, found, cap, s, h, lg) : std::vector<std::vector<std::string>>();
        const std::vector<std::vector<std::string>> textured =
            s.volume_texture.on ? texture_volume(st, ids, found, cap, s, h, lg) : std::vector<std::vector<std::string>>();
        const std::vector<std::vector<std::string>> zoned =
            s.volume_zones.on ? zones_volume(st, ids, found, cap, s, h, lg) : std::vector<std::vector<std::string>>();
        const std::vector<std::vector<std::string>> nbhooded =
            s.volume_nbhood.on ? nbhood_volume(st, ids, found, cap, s, h, lg) : std::vector<std::vector<std::string>>();
        const Members spatialised = s.volume_spatial.on ? spatial_volume(st, ids, found, cap, s, h, lg) : Members();
        std::vector<uint8_t> skeleton_picture;
        std::vector<int32_t> lines, radii;
        const Members skeletons = s.volume_skeleton.on ? skeleton_volume(D, hw, ids, found, cap, s, h, lg, skeleton_picture, lines, radii) : Members();
        const Members branched = s.volume_branches.on && !lines.empty() ? branches_volume(D, hw, lines, radii, found, cap, s, h, lg) : Members();
        const double spacing[3] = { v.spacing_x, v.spacing_y, v.spacing_z };
        std::ostringstream js;
        auto names =[&](const char *key, bool missing) {
            js << "  \"" << key << "\": [";
            bool first = true;
            for (size_t z = 0; z < D; ++z) {
                if (missing && !st.bases[z].empty()) continue;
                js << (first ? "" : ", ") << "\"" << medseg::json_escape(st.names[z]) << "\"";
                first = false;
            }
            js << "],\n";
        };
        js << "{\n";
        names("slices", false);
        names("missing", true);
        js << "  \"connectivity\": " << v.connectivity << ",\n  \"min_voxels\": " << v.min_voxels << ",\n  \"keep_largest\": " << v.keep_largest
           << ",\n  \"spacing\": [" << json_number(spacing[0]) << ", " << json_number(spacing[1]) << ", " << json_number(spacing[2])
           << "],\n" << clean_json << "  \"targets\": [";
        for (size_t t = 0; t < K; ++t) {
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"found\": " << found[t] << ", \"kept\": " << kept[t]
               << ", \"components\": [";
            const size_t rows = std::min<size_t>((size_t)found[t], cap);
            for (size_t r = 0; r < rows; ++r) {
                const mi_unet_vcomp &c = table[t * cap + r];
                mi_unet_vcomp_metrics m{};
                checked(mi_unet_volume_derive, &c, spacing, &m);
                js << (r ? "," : "") << "\n      {\"voxels\": " << c.voxels << ", \"kept\": " << c.kept << ", \"bbox\": [" << c.x0 << ", " << c.y0 << ", "
                   << c.z0 << ", " << c.x1 << ", " << c.y1 << ", " << c.z1 << "], \"centroid_mm\": [" << json_number(m.cx_mm) << ", "
                   << json_number(m.cy_mm) << ", " << json_number(m.cz_mm) << "], \"volume_mm3\": " << json_number(m.volume_mm3)
                   << ", \"surface_mm2\": " << json_number(m.surface_mm2) << ", \"extent_mm\": [" << json_number(m.extent_x_mm) << ", "
                   << json_number(m.extent_y_mm) << ", " << json_number(m.extent_z_mm) << "]" << (measured.empty() ? std::string() : measured[t][r])
                   << (textured.empty() ? std::string() : textured[t][r]) << (zoned.empty() ? std::string() : zoned[t][r])
                   << (nbhooded.empty() ? std::string() : nbhooded[t][r]) << (spatialised.empty() ? std::string() : spatialised[t][r])
                   << (split.rows.empty() ? std::string() : split.rows[t][r]) << (skeletons.empty() ? std::string() : skeletons[t][r])
                   << (branched.empty() ? std::string() : branched[t][r]) << "}";
            }
            js << (rows ? "\n    " : "") << "]" << (split.targets.empty() ? std::string() : split.targets[t]) << "}";
        }
        js << "\n  ]" << interp_json << mesh_json << "\n}\n";
        VolumeArtefacts a;
        a.output_dir = output_dir; a.report = js.str(); a.targets = &targets; a.bases = &st.bases; a.out = filter ? out.data() : nullptr;
        a.height = g_cfg.height; a.width = g_cfg.width;
        a.skeleton = skeleton_picture.empty() ? nullptr : skeleton_picture.data();
        write_volume_artefacts(a);
        filtered.swap(out);
        if (numbered) {
            numbered->ids.swap(ids);
            numbered->found.swap(found);
        }
    } catch (const std::exception &e) {
        report(lg, std::string("Volume error: ") + e.what());
    }
}

// set_volume_match: per target the truth stack (0 / 255, [D][H][W] at truth_planes + t * D * hw) labelled by mi_unet_volume_components
// under the setting's connectivity, no filter and a table of MI_UNET_VOLUME_MAX_TABLE, then one mi_unet_volume_match call on `h`
// (the host forms under MEDSEG_HOST_POSTPROCESS=1) against the ids label_volume numbered, mi_unet_volume_match_assign at the setting's
// threshold and mi_unet_volume_match_derive.  Returns per target the "lesions" member of its object in volume_score.json, from its
// leading comma on.  A failure is reported and returns nothing: only this step ends.
std::vector<std::string> match_volume(const VolumeIds &numbered, const std::vector<uint8_t> &truth_planes, size_t D, size_t hw, const Settings &s,
                                      mi_unet_t *h, std::ostream &lg)
{
    try {
        const VolumeMatch &match = s.volume_match;
        const size_t K = s.targets.size(), table_cap = MI_UNET_VOLUME_MAX_TABLE;
        if (numbered.ids.size() != K * D * hw || numbered.found.size() != K) throw std::runtime_error("the labelled stack is missing");
        const mi_unet_volume_opts opts{ s.volume.connectivity, 0, 0 };
        const int value = 255;
        std::vector<std::string> members(K);
        std::vector<int32_t> truth_ids(D * hw);
        std::vector<mi_unet_vcomp> truth_table(table_cap);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            int32_t truth_found = 0, truth_kept = 0;
            stage_call(h, mi_unet_volume_components, mi_unet_volume_components_host, truth_planes.data() + t * D * hw, (int)D, g_cfg.height, g_cfg.width,
                       &value, 1, &opts, nullptr, truth_ids.data(), truth_table.data(), (int)table_cap, &truth_found, &truth_kept);
            const size_t mp = std::min<size_t>((size_t)numbered.found[t], table_cap), mt = std::min<size_t>((size_t)truth_found, table_cap);
            const bool truncated = (size_t)numbered.found[t] > table_cap || (size_t)truth_found > table_cap;
            // a side without components is matched as one id that no voxel carries: an all-zero entry, which is not present
            const size_t np = std::max<size_t>(mp, 1), nt = std::max<size_t>(mt, 1);
            const size_t cap = std::min(np * nt, D * hw);       // a pair holds a cell and a voxel of its own: the list is never truncated
            std::vector<mi_unet_vmatch_side> ps(np), ts(nt);
            std::vector<mi_unet_vmatch_pair> pairs(cap);
            int found = 0;
            stage_call(h, mi_unet_volume_match, mi_unet_volume_match_host, numbered.ids.data() + t * D * hw, truth_ids.data(), (int)D, g_cfg.height,
                       g_cfg.width, (int)np, (int)nt, (int)cap, ps.data(), ts.data(), pairs.data(), &found);
            std::vector<int32_t> of_p(np), of_t(nt);
            mi_unet_vmatch_counts c{};
            mi_unet_vmatch_scores sc{};
            checked(mi_unet_volume_match_assign, ps.data(), (int)np, ts.data(), (int)nt, pairs.data(), found, (int)cap, match.iou_num, match.iou_den,
                    of_p.data(), of_t.data(), &c);
            checked(mi_unet_volume_match_derive, ps.data(), (int)np, ts.data(), (int)nt, pairs.data(), found, (int)cap, of_p.data(), &sc);
            std::ostringstream js;
            js << ", \"lesions\": {\"pred\": " << mp << ", \"truth\": " << mt << ", \"iou_threshold\": [" << match.iou_num << ", " << match.iou_den
               << "], \"tp\": " << c.tp << ", \"fp\": " << c.fp << ", \"fn\": " << c.fn << ", \"precision\": " << json_number(sc.precision)
               << ", \"recall\": " << json_number(sc.recall) << ", \"f1\": " << json_number(sc.f1) << ", \"pq\": " << json_number(sc.pq)
               << ", \"sq\": " << json_number(sc.sq) << ", \"rq\": " << json_number(sc.rq) << ", \"mean_dice\": " << json_number(sc.mean_dice)
               << ", \"matches\": [";
            bool first = true;
            for (size_t r = 0; r < mp; ++r) {
                if (!of_p[r]) continue;
                const int32_t tc = of_p[r] - 1;
                const mi_unet_vmatch_pair *q = pairs.data();
                while (q->p != (int32_t)r || q->t != tc) ++q;   // (derive has found it: the match is in the list)
                const double i = q->voxels, vp = ps[r].voxels, vt = ts[tc].voxels;
                js << (first ? "" : ", ") << "{\"pred\": " << r << ", \"truth\": " << tc << ", \"voxels\": " << q->voxels << ", \"iou\": "
                   << json_number(i / (vp + vt - i)) << ", \"dice\": " << json_number(2.0 * i / (vp + vt)) << ", \"pred_voxels\": " << ps[r].voxels
                   << ", \"truth_voxels\": " << ts[tc].voxels << "}";
                first = false;
            }
            js << "], \"missed\": [";
            first = true;
            for (size_t k = 0; k < mt; ++k) {
                if (of_t[k] || ts[k].voxels < 1) continue;
                js << (first ? "" : ", ") << "{\"truth\": " << k << ", \"voxels\": " << ts[k].voxels << "}";
                first = false;
            }
            js << "], \"spurious\": [";
            first = true;
            for (size_t r = 0; r < mp; ++r) {
                if (of_p[r] || ps[r].voxels < 1) continue;
                js << (first ? "" : ", ") << r;
                first = false;
            }
            js << "]" << (truncated ? ", \"truncated\": true" : "") << "}";
            members[t] = js.str();
        }
        lg << "Volume match: " << K << " targets, " << ms_since(t0) << " ms" << std::endl;
        return members;
    } catch (const std::exception &e) {
        report(lg, std::string("Volume match error: ") + e.what());
        return {};
    }
}

// set_volume with set_truth_dir: the stack against <dir>/<base>_labels.raw of every slice as ONE volume (mi_unet_score_volume in
// include/mi_unet.h).  One call per target with values = { 255 } on `h` (mi_unet_score_volume_host under
// MEDSEG_HOST_POSTPROCESS=1): pred is the target's plane of `filtered` when the volume filter is active, else of the stack; truth is
// recoded to 0 / 255 by truth == cls.  The integer units come from mi_unet_score_volume_units on the setting's spacing.  Writes
// <output_dir>/volume_score.json.  Only a stack whose every slice completed and has a truth file of the tile's size is scored; a
// failure is reported and fails no image.  With set_volume_match on, every target object gains a last member "lesions" (match_volume)
// from the ids label_volume numbered.
void score_volume_stack(const VolumeStack &st, const std::vector<uint8_t> &filtered, const Settings &s, mi_unet_t *h, const std::string &output_dir,
                        std::ostream &lg, const VolumeIds &numbered)
{
    try {
        const std::vector<mi_unet_target> &targets = s.targets;
        const Volume &v = s.volume;
        const bool match = s.volume_match.on;
        const size_t K = targets.size(), D = st.D, hw = st.hw;
        const bool filter = !filtered.empty() || v.min_voxels > 0 || v.keep_largest > 0;       // (a cleaned stack comes filtered too)
        if (filter && filtered.size() != K * D * hw) throw std::runtime_error("the filtered stack is missing");
        std::vector<uint8_t> labels(D * hw), truth(D * hw), truth_planes(match ? K * D * hw : 0);
        size_t without = 0;
        for (size_t z = 0; z < D; ++z) {
            bool good = !st.bases[z].empty();
            if (good) {
                const std::string path = s.truth_dir + "/" + st.bases[z] + "_labels.raw";
                std::error_code ec;
                const auto size = fs::file_size(path, ec);
                std::ifstream f(path, std::ios::binary);
                good = !ec && size == hw && f.read(reinterpret_cast<char *>(labels.data() + z * hw), (std::streamsize)hw);
            }
            without += !good;
        }
        if (without) {
            lg << "Volume score skipped: " << without << " of " << D << " slices without mask or truth" << std::endl;
            return;
        }
        const VolumeUnits u = volume_units(v, D);
        const mi_unet_score_opts opts{ 50000, 0 };
        const int value = 255;
        std::vector<mi_unet_score> scores(K);
        const auto t0 = hr_clock::now();
        for (size_t t = 0; t < K; ++t) {
            for (size_t i = 0; i < D * hw; ++i) truth[i] = labels[i] == targets[t].cls ? 255 : 0;
            stage_call(h, mi_unet_score_volume, mi_unet_score_volume_host, (filter ? filtered.data() : st.planes.data()) + t * D * hw, truth.data(), (int)D,
                       g_cfg.height, g_cfg.width, &value, 1, u.units, &opts, &scores[t], nullptr, nullptr);
            if (match) std::copy(truth.begin(), truth.end(), truth_planes.begin() + t * D * hw);
        }
        lg << "Volume score: " << D << " slices, " << K << " targets, " << ms_since(t0) << " ms" << std::endl;
        const std::vector<std::string> lesions = match ? match_volume(numbered, truth_planes, D, hw, s, h, lg) : std::vector<std::string>();
        std::ostringstream js;
        js << "{\n  \"slices\": [";
        for (size_t z = 0; z < D; ++z) js << (z ? ", " : "") << "\"" << medseg::json_escape(st.names[z]) << "\"";
        js << "],\n  \"unit_mm\": " << json_number(u.unit_mm) << ",\n  \"spacing_units\": [" << u.units[0] << ", " << u.units[1] << ", " << u.units[2]
           << "],\n  \"quantile_ppm\": " << opts.quantile_ppm << ",\n  \"targets\": [";
        for (size_t t = 0; t < K; ++t) {
            const mi_unet_score &sc = scores[t];
            mi_unet_score_metrics m{};
            checked(mi_unet_score_volume_derive, &sc, u.unit_mm, &m);
            js << (t ? "," : "") << "\n    {\"label\": " << targets[t].cls << ", \"tp\": " << sc.tp << ", \"fp\": " << sc.fp << ", \"fn\": " << sc.fn
               << ", \"dice\": " << json_number(m.dice) << ", \"iou\": " << json_number(m.iou) << ", \"hd_mm\": " << json_number(m.hd)
               << ", \"hd_q_mm\": " << json_number(m.hd_q) << ", \"assd_mm\": " << json_number(m.assd) << ", \"rmsd_mm\": " << json_number(m.rmsd)
               << (lesions.empty() ? std::string() : lesions[t]) << "}";
        }
        js << "\n  ]\n}\n";
        write_volume_score(output_dir, js.str());
    } catch (const std::exception &e) {
        report(lg, std::string("Volume score error: ") + e.what());
    }
}

}  // namespace

void finish_volume(VolumeStack &stack, const Settings &s, mi_unet_t *h, const std::string &output_dir, std::ostream &lg)
{
    std::vector<uint8_t> filtered;
    std::string clean_json;
    if (s.volume_clean.on && !clean_volume(stack, s, h, lg, clean_json)) return;
    const bool match = s.volume_match.on && !s.truth_dir.empty();
    VolumeIds numbered;
    label_volume(stack, s, h, output_dir, lg, filtered, clean_json, match ? &numbered : nullptr);
    if (!s.truth_dir.empty()) score_volume_stack(stack, filtered, s, h, output_dir, lg, numbered);
}

}  // namespace MedicalSeg
