// json_io.h -- byte-exact emitter for the two documents the reference writes through nlohmann::json 3.12
// (include/nlohmann/json.hpp in the reference; pinned in tests against oracle/_ref/json_probe, which is built from that
// header) and a small reader for the size file.  nlohmann specifics reproduced: std::map key order (byte-wise sorted),
// dump() without indent = no whitespace at all, dump(4) = every array element and object member on its own line,
// "{}" / "[]" for empty containers, string escaping of dump() with ensure_ascii = false.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/medseg/image.h"

namespace medseg {

std::string json_escape(const std::string &s);

// {"<raw filename>":{"original_height":h,"original_width":w,"scaled_height":sh,"scaled_width":sw}}\n  (src/preprocess.cpp:126-134)
// lo_hi (an intensity window, Preprocess::set_window) appends ,"window_hi":hi,"window_lo":lo -- keys in nlohmann's sorted order
std::string size_json_text(const std::string &raw_filename, int w, int h, int scaled_w, int scaled_h, const int *lo_hi = nullptr);

// src/mask2polygon.cpp:68-109 with std::setw(4)
std::string polygon_json_text(const std::vector<Contour> &contours, const std::string &base_name, int original_width,
                              int original_height);

// The same document for the targets of MedicalSeg::set_targets: the shapes of group g carry "label": groups[g].cls and
// "labelIndex": g, group after group; a group without contours contributes no shape; everything else as above.  One exception keeps
// the reference's document: a single group of class 2 -- the default target list -- is the function above ("label": 1,
// "labelIndex": 0, the reference's name for its one foreground class).
// With `regions` (MedicalSeg::set_measure; regions->regions[g][c] for groups[g].contours[c]) every shape gains a "region" object
// between "points" and "shape_type", keys in nlohmann's sorted order: area, bbox [x0, y0, x1, y1], centroid [cx, cy], edges, imax,
// imin, major, mean, minor, scale_x, scale_y, std, theta -- the region's integers and mi_unet_region_derive of it, in TILE pixels;
// scale_x / scale_y convert to the points' coordinates.  Integers as std::to_string writes them, doubles as nlohmann's dump() does:
// the shortest decimal that reads back as the same double, with ".0" appended to one without '.', 'e' or 'E'.  Without `regions`
// the document is unchanged byte for byte.
std::string polygon_json_text(const std::vector<ClassContours> &groups, const std::string &base_name, int original_width,
                              int original_height, const RegionTable *regions = nullptr);
std::string json_double(double v);

// Parses an object of objects of integers (the size file).  Throws std::runtime_error on malformed input.
std::map<std::string, std::map<std::string, long long>> parse_size_json(const std::string &text);

}  // namespace medseg
