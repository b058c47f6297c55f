// artefacts.h -- the five artefacts of one image whose device or host work is finished: <base>_normalized.png,
// <base>_original_sizes.json, the mask picture(s), <base>_contour_overlay.png and <base>.json.  Pure host code: no device call, no
// facade state (tests/cpu/artefacts_test.cpp builds it without the facade).
#pragma once
#include <ostream>
#include <string>
#include <vector>

#include "../../include/medseg/image.h"

namespace MedicalSeg {

inline bool is_default(const std::vector<mi_unet_target> &t) { return t.size() == 1 && t[0].cls == 2 && t[0].min_area_frac == 0.06f; }

// What a device call left for one mask plane: its slices of the call's xy / start arrays and its count.  A negative count -- a capacity
// overflow on the device, or no device tracer at all -- hands the mask picture to the host tracer (xy and start are not read then).
// `regions`, when the call measured this plane (MedicalSeg::set_measure), are the `count` records of its region report.
struct PlaneShapes {
    const int32_t *xy = nullptr, *start = nullptr;
    int count = -1;
    const mi_unet_region *regions = nullptr;
};

struct ImageArtefacts {
    const medseg::Image8 *tile = nullptr;              // the grey tile the network read
    const std::vector<mi_unet_target> *targets = nullptr;   // K targets: the default list names the one mask <base>_mask.png,
    const medseg::Image8 *masks = nullptr;             //   any other list <base>_mask_class<cls>.png; K pictures, 0 / 255
    const PlaneShapes *planes = nullptr;               // K entries, in target order
    int width = 0, height = 0;                         // of the original image
    std::string raw_path, output_dir, base_name;
    std::ostream *console = nullptr;                   // the text of Mask2Polygon::write_polygon_outputs
    bool class_lines = false;                          // that text counts the contours per class (the per-target routes), not in one line
    bool concurrent = false;                           // the three groups below side by side (the single-image all-device route)
};

// milliseconds of the three artefact groups -- {normalized.png + sizes.json}, {mask pictures}, {overlay.png + polygon json} -- and of
// all three from the first start to the last end; the contour lists are built before the clocks start
struct ArtefactTimes { double norm_ms = 0, mask_ms = 0, poly_ms = 0, total_ms = 0; };

// Writes them all.  The .json carries "region" objects only when every plane has regions.  Throws std::runtime_error("Preprocessing
// failed") / ("Failed to save mask"); with `concurrent` only after all three groups have ended.
ArtefactTimes write_image_artefacts(const ImageArtefacts &a);

// The artefacts of a batch labelled as one volume (MedicalSeg::set_volume): <output_dir>/volume_report.json with the text `report`
// and, when `out` is given -- the filtered stack u8 [K][D][H][W], 0 / 255, K = targets, D = bases -- per slice
// <base>_volume_mask.png, or <base>_volume_mask_class<cls>.png under a non-default target list.  A slice without a name has no
// picture.  When `skeleton` is given (MedicalSeg::set_volume_skeleton with png) -- the same layout -- per slice
// <base>_volume_skeleton.png, or <base>_volume_skeleton_class<cls>.png.  Throws std::runtime_error("Failed to save volume report") /
// ("Failed to save volume mask") / ("Failed to save volume skeleton").
struct VolumeArtefacts {
    std::string output_dir, report;
    const std::vector<mi_unet_target> *targets = nullptr;
    const std::vector<std::string> *bases = nullptr;
    const uint8_t *out = nullptr;
    const uint8_t *skeleton = nullptr;
    int height = 0, width = 0;
};
void write_volume_artefacts(const VolumeArtefacts &a);

// The border of one target's labelled stack (MedicalSeg::set_volume_mesh) as binary STL, <output_dir>/<file>: `xyz` are the nv vertex
// positions in millimetres (mi_unet_volume_mesh_positions), `quads` the nq quads over them; every quad gives the triangles (0, 1, 2)
// and (0, 2, 3).  An 80-byte header that starts "medseg volume mesh" and is padded with zeros, the triangle count as uint32, then per
// triangle the unit normal of the float positions -- computed in double, rounded to float; 0, 0, 0 for a zero cross product --, the three
// vertices and an attribute of 0, all little-endian.  Throws std::runtime_error("Failed to save volume mesh").
struct VolumeMeshArtefact {
    std::string output_dir, file;
    const float *xyz = nullptr;
    const int32_t *quads = nullptr;
    size_t nv = 0, nq = 0;
};
void write_volume_mesh(const VolumeMeshArtefact &a);

// The scores of a batch as one volume against ground truth (MedicalSeg::set_volume with set_truth_dir): <output_dir>/volume_score.json
// with the text `score`.  Throws std::runtime_error("Failed to save volume score").
void write_volume_score(const std::string &output_dir, const std::string &score);

}  // namespace MedicalSeg
