#include "json_io.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <stdexcept>

namespace medseg {

std::string json_escape(const std::string &s)
{
    std::string o;
    o.reserve(s.size() + 2);
    for (unsigned char c : s) {
        switch (c) {
        case '"': o += "\\\""; break;
        case '\\': o += "\\\\"; break;
        case '\b': o += "\\b"; break;
        case '\f': o += "\\f"; break;
        case '\n': o += "\\n"; break;
        case '\r': o += "\\r"; break;
        case '\t': o += "\\t"; break;
        default:
            if (c < 0x20) {                           // nlohmann escapes control characters as \u00XX (DEL passes when ensure_ascii is off)
                char b[8];
                snprintf(b, sizeof b, "\\u%04x", c);
                o += b;
            } else {
                o += (char)c;                         // UTF-8 passes through (ensure_ascii = false)
            }
        }
    }
    return o;
}

std::string size_json_text(const std::string &raw_filename, int w, int h, int scaled_w, int scaled_h, const int *lo_hi)
{
    std::string o = "{\"" + json_escape(raw_filename) + "\":{";
    o += "\"original_height\":" + std::to_string(h);
    o += ",\"original_width\":" + std::to_string(w);
    o += ",\"scaled_height\":" + std::to_string(scaled_h);
    o += ",\"scaled_width\":" + std::to_string(scaled_w);
    if (lo_hi) o += ",\"window_hi\":" + std::to_string(lo_hi[1]) + ",\"window_lo\":" + std::to_string(lo_hi[0]);
    o += "}}\n";
    return o;
}

namespace {
// the document around a list of shapes, each with its label pair (src/mask2polygon.cpp:68-109 with std::setw(4))
struct Shape { const Contour *pts; int label, label_index; const mi_unet_region *region = nullptr; };

// the "region" member of a shape (16 spaces deep), keys sorted byte-wise
std::string region_member(const mi_unet_region &r, double scale_x, double scale_y)
{
    mi_unet_region_shape s{};
    if (mi_unet_region_derive(&r, &s) != MI_UNET_OK) throw std::runtime_error(std::string("region_derive failed: ") + mi_unet_last_error());
    const std::string in1 = "                ", in2 = "                    ";
    auto ints = [&](const char *key, std::initializer_list<std::string> vals) {
        std::string o = in1 + "\"" + key + "\": [\n";
        size_t k = 0;
        for (const std::string &v : vals) o += in2 + v + (++k < vals.size() ? ",\n" : "\n");
        return o + in1 + "],\n";
    };
    std::string o = "            \"region\": {\n";
    o += in1 + "\"area\": " + std::to_string(r.area) + ",\n";
    o += ints("bbox", { std::to_string(r.x0), std::to_string(r.y0), std::to_string(r.x1), std::to_string(r.y1) });
    o += ints("centroid", { json_double(s.cx), json_double(s.cy) });
    o += in1 + "\"edges\": " + std::to_string(r.edges) + ",\n";
    o += in1 + "\"imax\": " + std::to_string(r.imax) + ",\n";
    o += in1 + "\"imin\": " + std::to_string(r.imin) + ",\n";
    o += in1 + "\"major\": " + json_double(s.major) + ",\n";
    o += in1 + "\"mean\": " + json_double(s.mean) + ",\n";
    o += in1 + "\"minor\": " + json_double(s.minor) + ",\n";
    o += in1 + "\"scale_x\": " + json_double(scale_x) + ",\n";
    o += in1 + "\"scale_y\": " + json_double(scale_y) + ",\n";
    o += in1 + "\"std\": " + json_double(s.std) + ",\n";
    o += in1 + "\"theta\": " + json_double(s.theta) + "\n";
    o += "            },\n";
    return o;
}

std::string polygon_document(const std::vector<Shape> &shapes, const std::string &base_name, int original_width, int original_height,
                             double scale_x = 1.0, double scale_y = 1.0)
{
    std::string o;
    o += "{\n";
    o += "    \"flags\": {},\n";
    o += "    \"imageData\": null,\n";
    o += "    \"imageHeight\": " + std::to_string(original_height) + ",\n";
    o += "    \"imagePath\": \"" + json_escape(base_name + ".raw") + "\",\n";       // always .raw (src/mask2polygon.cpp:76)
    o += "    \"imageWidth\": " + std::to_string(original_width) + ",\n";
    if (shapes.empty()) {
        o += "    \"shapes\": [],\n";
    } else {
        o += "    \"shapes\": [\n";
        for (size_t c = 0; c < shapes.size(); ++c) {
            const Contour &pts = *shapes[c].pts;
            o += "        {\n";
            o += "            \"description\": \"\",\n";
            o += "            \"flags\": {},\n";
            o += "            \"group_id\": null,\n";
            o += "            \"label\": " + std::to_string(shapes[c].label) + ",\n";
            o += "            \"labelIndex\": " + std::to_string(shapes[c].label_index) + ",\n";
            o += "            \"mask\": null,\n";
            if (pts.empty()) {
                o += "            \"points\": null,\n";      // a default-constructed nlohmann::json that was never push_back'ed
            } else {
                o += "            \"points\": [\n";
                for (size_t k = 0; k < pts.size(); ++k) {
                    o += "                [\n";
                    o += "                    " + std::to_string(pts[k].x) + ",\n";
                    o += "                    " + std::to_string(pts[k].y) + "\n";
                    o += (k + 1 < pts.size()) ? "                ],\n" : "                ]\n";
                }
                o += "            ],\n";
            }
            if (shapes[c].region) o += region_member(*shapes[c].region, scale_x, scale_y);
            o += "            \"shape_type\": \"polygon\"\n";
            o += (c + 1 < shapes.size()) ? "        },\n" : "        }\n";
        }
        o += "    ],\n";
    }
    o += "    \"version\": \"1.0.2.812\"\n";
    o += "}\n";
    return o;
}
}  // namespace

std::string polygon_json_text(const std::vector<Contour> &contours, const std::string &base_name, int original_width,
                              int original_height)
{
    std::vector<Shape> shapes;
    for (const Contour &c : contours) shapes.push_back({ &c, 1, 0 });
    return polygon_document(shapes, base_name, original_width, original_height);
}

std::string polygon_json_text(const std::vector<ClassContours> &groups, const std::string &base_name, int original_width,
                              int original_height, const RegionTable *regions)
{
    if (regions) {
        if (regions->regions.size() != groups.size()) throw std::runtime_error("polygon_json_text: one list of regions per group");
        for (size_t g = 0; g < groups.size(); ++g)
            if (regions->regions[g].size() != groups[g].contours.size()) throw std::runtime_error("polygon_json_text: one region per contour");
    }
    const bool reference = groups.size() == 1 && groups[0].cls == 2;      // the reference's name for its one foreground class
    if (reference && !regions) return polygon_json_text(groups[0].contours, base_name, original_width, original_height);
    std::vector<Shape> shapes;
    for (size_t g = 0; g < groups.size(); ++g)
        for (size_t c = 0; c < groups[g].contours.size(); ++c)
            shapes.push_back({ &groups[g].contours[c], reference ? 1 : groups[g].cls, reference ? 0 : (int)g,
                               regions ? &regions->regions[g][c] : nullptr });
    return polygon_document(shapes, base_name, original_width, original_height, regions ? regions->scale_x : 1.0,
                            regions ? regions->scale_y : 1.0);
}

std::string json_double(double v)
{
    char b[40];
    for (int p = 1; p <= 17; ++p) {
        snprintf(b, sizeof b, "%.*g", p, v);
        if (strtod(b, nullptr) == v) break;
    }
    std::string o = b;
    if (o.find_first_of(".eE") == std::string::npos) o += ".0";
    return o;
}

namespace {
struct Parser {
    const std::string &s;
    size_t i = 0;
    explicit Parser(const std::string &t) : s(t) {}
    [[noreturn]] void bad(const char *what) { throw std::runtime_error(std::string("size JSON parse error: ") + what); }
    void ws() { while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\r' || s[i] == '\t')) ++i; }
    void expect(char c) { ws(); if (i >= s.size() || s[i] != c) bad("unexpected character"); ++i; }
    bool peek(char c) { ws(); return i < s.size() && s[i] == c; }
    std::string str()
    {
        expect('"');
        std::string o;
        while (i < s.size() && s[i] != '"') {
            if (s[i] == '\\') {
                if (++i >= s.size()) bad("dangling escape");
                switch (s[i]) {
                case 'n': o += '\n'; break; case 't': o += '\t'; break; case 'r': o += '\r'; break;
                case 'b': o += '\b'; break; case 'f': o += '\f'; break;
                case 'u': {
                    if (i + 4 >= s.size()) bad("short \\u escape");
                    const unsigned cp = (unsigned)std::stoul(s.substr(i + 1, 4), nullptr, 16);
                    if (cp < 0x80) o += (char)cp;
                    else if (cp < 0x800) { o += (char)(0xC0 | cp >> 6); o += (char)(0x80 | (cp & 0x3F)); }
                    else { o += (char)(0xE0 | cp >> 12); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
                    i += 4;
                    break;
                }
                default: o += s[i];
                }
                ++i;
            } else {
                o += s[i++];
            }
        }
        expect('"');
        return o;
    }
    long long integer()
    {
        ws();
        size_t j = i;
        if (j < s.size() && s[j] == '-') ++j;
        while (j < s.size() && s[j] >= '0' && s[j] <= '9') ++j;
        if (j == i) bad("expected an integer");
        const long long v = std::stoll(s.substr(i, j - i));
        i = j;
        return v;
    }
};
}  // namespace

std::map<std::string, std::map<std::string, long long>> parse_size_json(const std::string &text)
{
    Parser p(text);
    std::map<std::string, std::map<std::string, long long>> out;
    p.expect('{');
    if (!p.peek('}')) {
        for (;;) {
            const std::string key = p.str();
            p.expect(':');
            p.expect('{');
            auto &inner = out[key];
            if (!p.peek('}')) {
                for (;;) {
                    const std::string k = p.str();
                    p.expect(':');
                    inner[k] = p.integer();
                    if (p.peek(',')) { p.expect(','); continue; }
                    break;
                }
            }
            p.expect('}');
            if (p.peek(',')) { p.expect(','); continue; }
            break;
        }
    }
    p.expect('}');
    return out;
}

}  // namespace medseg
