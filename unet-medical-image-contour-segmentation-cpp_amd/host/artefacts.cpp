// artefacts.cpp -- write_image_artefacts (artefacts.h): what every route of the facade does with a finished image (the facade's units:
// routes.cpp).
#include "artefacts.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <future>
#include <stdexcept>

#include "../../include/medseg/mask2polygon.h"
#include "../../include/medseg/preprocess.h"
#include "png_io.h"

namespace MedicalSeg {

static std::vector<medseg::Contour> contours_of(const PlaneShapes &p, const medseg::Image8 &vis)
{
    if (p.count < 0) return Mask2Polygon::extract_contours(vis);
    std::vector<medseg::Contour> contours;
    for (int c = 0; c < p.count; ++c) {
        medseg::Contour cc;
        for (int q = p.start[c]; q < p.start[c + 1]; ++q) cc.emplace_back(p.xy[2 * q], p.xy[2 * q + 1]);
        contours.push_back(std::move(cc));
    }
    return contours;
}

ArtefactTimes write_image_artefacts(const ImageArtefacts &a)
{
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    const std::vector<mi_unet_target> &targets = *a.targets;
    const std::string stem = a.output_dir + "/" + a.base_name;
    std::vector<medseg::ClassContours> groups;
    medseg::RegionTable table;
    table.regions.resize(targets.size());
    bool measured = true;                                  // a table is used only when every plane has one
    for (size_t t = 0; t < targets.size(); ++t) {
        const PlaneShapes &p = a.planes[t];
        groups.push_back({ targets[t].cls, contours_of(p, a.masks[t]) });
        if (p.regions && p.count >= 0) table.regions[t].assign(p.regions, p.regions + p.count);
        else measured = false;
    }
    ArtefactTimes times;
    const auto t_all = clk::now();
    auto normalized = [&] {
        const auto t0 = clk::now();
        const bool ok = Preprocess::write_preprocess_outputs(*a.tile, a.raw_path, stem + "_normalized.png", stem + "_original_sizes.json",
                                                             a.width, a.height);
        times.norm_ms = ms_since(t0);
        return ok;
    };
    auto masks = [&] {
        const auto t0 = clk::now();
        bool ok = true;
        for (size_t t = 0; t < targets.size() && ok; ++t)
            ok = medseg::write_png(stem + (is_default(targets) ? "_mask.png" : "_mask_class" + std::to_string(targets[t].cls) + ".png"),
                                   a.masks[t], /*level0=*/true);
        times.mask_ms = ms_since(t0);
        return ok;
    };
    auto polygons = [&] {
        const auto t0 = clk::now();
        if (a.class_lines)
            Mask2Polygon::write_polygon_outputs(groups, *a.tile, a.output_dir, a.base_name, a.width, a.height, *a.console,
                                                measured ? &table : nullptr);
        else            // one group of the default class: the same files, the reference's console text
            Mask2Polygon::write_polygon_outputs(groups[0].contours, *a.tile, a.output_dir, a.base_name, a.width, a.height, *a.console,
                                                measured ? &table : nullptr);
        times.poly_ms = ms_since(t0);
    };
    bool norm_ok, mask_ok = true;
    if (a.concurrent) {
        auto f_norm = std::async(std::launch::async, normalized);
        auto f_mask = std::async(std::launch::async, masks);
        polygons();
        norm_ok = f_norm.get(); mask_ok = f_mask.get();
    } else if ((norm_ok = normalized()) && (mask_ok = masks())) {
        polygons();
    }
    times.total_ms = ms_since(t_all);
    if (!norm_ok) throw std::runtime_error("Preprocessing failed");
    if (!mask_ok) throw std::runtime_error("Failed to save mask");
    return times;
}

void write_volume_artefacts(const VolumeArtefacts &a)
{
    std::ofstream o(a.output_dir + "/volume_report.json", std::ios::binary);
    o << a.report;
    o.close();
    if (!o) throw std::runtime_error("Failed to save volume report");
    // a stack u8 [K][D][H][W] as one picture per target and named slice: <base>_volume_<what>.png or <base>_volume_<what>_class<cls>.png
    auto pictures = [&](const uint8_t *stack, const std::string &what) {
        const std::vector<mi_unet_target> &targets = *a.targets;
        const size_t hw = (size_t)a.height * a.width, D = a.bases->size();
        for (size_t t = 0; t < targets.size(); ++t)
            for (size_t z = 0; z < D; ++z) {
                if ((*a.bases)[z].empty()) continue;
                medseg::Image8 m(a.height, a.width, 1);
                std::copy(stack + (t * D + z) * hw, stack + (t * D + z + 1) * hw, m.data.begin());
                const std::string name = "_volume_" + what + (is_default(targets) ? std::string() : "_class" + std::to_string(targets[t].cls)) + ".png";
                if (!medseg::write_png(a.output_dir + "/" + (*a.bases)[z] + name, m, /*level0=*/true))
                    throw std::runtime_error("Failed to save volume " + what);
            }
    };
    if (a.out) pictures(a.out, "mask");
    if (a.skeleton) pictures(a.skeleton, "skeleton");
}

void write_volume_mesh(const VolumeMeshArtefact &a)
{
    static_assert(sizeof(float) == 4, "binary STL holds IEEE single floats");
    std::string buf(84 + a.nq * 2 * 50, '\0');
    const char title[] = "medseg volume mesh";
    std::copy(title, title + sizeof(title) - 1, buf.begin());
    const uint32_t triangles = (uint32_t)(a.nq * 2);
    std::memcpy(&buf[80], &triangles, 4);
    char *at = &buf[84];
    for (size_t q = 0; q < a.nq; ++q)
        for (int t = 0; t < 2; ++t) {
            const float *const p[3] = { a.xyz + 3 * (size_t)a.quads[4 * q], a.xyz + 3 * (size_t)a.quads[4 * q + 1 + t],
                                        a.xyz + 3 * (size_t)a.quads[4 * q + 2 + t] };
            const double u[3] = { (double)p[1][0] - p[0][0], (double)p[1][1] - p[0][1], (double)p[1][2] - p[0][2] };
            const double w[3] = { (double)p[2][0] - p[0][0], (double)p[2][1] - p[0][1], (double)p[2][2] - p[0][2] };
            const double n[3] = { u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0] };
            const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            float rec[12];
            for (int c = 0; c < 3; ++c) rec[c] = len > 0.0 ? (float)(n[c] / len) : 0.f;
            for (int v = 0; v < 3; ++v)
                for (int c = 0; c < 3; ++c) rec[3 + 3 * v + c] = p[v][c];
            std::memcpy(at, rec, 48);                           // (the two attribute bytes behind it stay 0)
            at += 50;
        }
    std::ofstream o(a.output_dir + "/" + a.file, std::ios::binary);
    o.write(buf.data(), (std::streamsize)buf.size());
    o.close();
    if (!o) throw std::runtime_error("Failed to save volume mesh");
}

void write_volume_score(const std::string &output_dir, const std::string &score)
{
    std::ofstream o(output_dir + "/volume_score.json", std::ios::binary);
    o << score;
    o.close();
    if (!o) throw std::runtime_error("Failed to save volume score");
}

}  // namespace MedicalSeg
