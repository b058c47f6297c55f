// postprocess.cpp -- label map -> cleaned {0,2} mask.  Reference: src/postprocess.cpp:5-79 (OpenCV there).
// Own algorithms: run-based two-pass union-find labelling with per-component bbox/area (instead of one full-image
// `labels == i` pass per component, the reference's O(nc*H*W) loops at :41 and :71), two-pass erosion / dilation by a box or disc.
#include "../../include/medseg/postprocess.h"

#include "../../include/mi_unet.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

namespace {

constexpr int FOREGROUND_VALUE = 2;          // src/postprocess.cpp:5
constexpr float MIN_AREA_RATIO = 0.06f;      // src/postprocess.cpp:9

struct Stat { int left, top, right, bottom, area; };

struct Labelling {
    std::vector<int> labels;                 // per pixel, 0 = background, otherwise a ROOT id
    std::vector<Stat> stats;                 // indexed by root id (entries of non-roots unused)
};

int find(std::vector<int> &p, int a)
{
    while (p[a] != a) { p[a] = p[p[a]]; a = p[a]; }
    return a;
}

// 8-connected components of fg != 0 (cv::connectedComponentsWithStats(..., 8): membership, bbox, area).
Labelling label8(const uint8_t *fg, int w, int h)
{
    Labelling L;
    L.labels.assign((size_t)w * h, 0);
    std::vector<int> parent(1, 0);
    for (int y = 0; y < h; ++y) {
        int *row = L.labels.data() + (size_t)y * w;
        const int *up = y ? row - w : nullptr;
        const uint8_t *f = fg + (size_t)y * w;
        for (int x = 0; x < w; ++x) {
            if (!f[x]) continue;
            int lab = 0;
            auto join = [&](int other) {
                if (!other) return;
                other = find(parent, other);
                if (!lab) lab = other;
                else if (lab != other) { const int a = std::min(lab, other), b = std::max(lab, other); parent[b] = a; lab = a; }
            };
            if (x) join(row[x - 1]);
            if (up) {
                if (x) join(up[x - 1]);
                join(up[x]);
                if (x + 1 < w) join(up[x + 1]);
            }
            if (!lab) { lab = (int)parent.size(); parent.push_back(lab); }
            row[x] = lab;
        }
    }
    L.stats.assign(parent.size(), Stat{ w, h, -1, -1, 0 });
    for (int y = 0; y < h; ++y) {
        int *row = L.labels.data() + (size_t)y * w;
        for (int x = 0; x < w; ++x) {
            if (!row[x]) continue;
            const int r = find(parent, row[x]);
            row[x] = r;
            Stat &s = L.stats[r];
            s.left = std::min(s.left, x); s.right = std::max(s.right, x);
            s.top = std::min(s.top, y); s.bottom = std::max(s.bottom, y);
            ++s.area;
        }
    }
    return L;
}

// One erosion (dilate = false) or dilation of a 0 / 255 plane by the box or disc of radius r, in two passes.  A stopper is
// a background pixel for an erosion, a foreground pixel for a dilation; positions outside the image are never stoppers (OpenCV's
// default morphology border never constrains an erosion and never seeds a dilation).  Pass 1, down and up every column: g = distance
// to the nearest stopper of the column within r, else r + 1.  Pass 2, along the rows: the pixel is hit when some |dx| <= r inside the
// image has g <= r (box) or g * g + dx * dx <= r * r (disc).  An erosion keeps what is not hit, a dilation sets what is.
void morph_step(const std::vector<uint8_t> &src, std::vector<uint8_t> &dst, int w, int h, int shape, int r, bool dilate)
{
    if (r == 0) { dst = src; return; }
    std::vector<uint8_t> g((size_t)w * h);
    for (int x = 0; x < w; ++x) {
        int d = r + 1;
        for (int y = 0; y < h; ++y) {
            const bool stop = (src[(size_t)y * w + x] != 0) == dilate;
            d = stop ? 0 : std::min(d + 1, r + 1);
            g[(size_t)y * w + x] = (uint8_t)d;
        }
        d = r + 1;
        for (int y = h - 1; y >= 0; --y) {
            const bool stop = (src[(size_t)y * w + x] != 0) == dilate;
            d = stop ? 0 : std::min(d + 1, r + 1);
            g[(size_t)y * w + x] = (uint8_t)std::min<int>(g[(size_t)y * w + x], d);
        }
    }
    dst.assign(src.size(), 0);
    const bool disc = shape == MI_UNET_MORPH_DISC;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            bool hit = false;
            for (int xx = std::max(0, x - r); xx <= std::min(w - 1, x + r) && !hit; ++xx) {
                const int gv = g[(size_t)y * w + xx], dx = xx - x;
                hit = disc ? gv * gv + dx * dx <= r * r : gv <= r;
            }
            dst[(size_t)y * w + x] = hit == dilate ? 255 : 0;
        }
}

}  // namespace

medseg::Image8 postprocess_mask(const medseg::Image8 &src) { return postprocess_mask(src, FOREGROUND_VALUE, MIN_AREA_RATIO); }

medseg::Image8 postprocess_mask(const medseg::Image8 &src, int cls, float min_area_frac)
{
    return postprocess_mask(src, cls, min_area_frac, mi_unet_morph{ MI_UNET_MORPH_RECT, 1, 0 });
}

medseg::Image8 postprocess_mask(const medseg::Image8 &src, int cls, float min_area_frac, const mi_unet_morph &morph)
{
    if ((morph.shape != MI_UNET_MORPH_RECT && morph.shape != MI_UNET_MORPH_DISC) || morph.open_r < 0 || morph.open_r > MI_UNET_MORPH_MAX_R ||
        morph.close_r < 0 || morph.close_r > MI_UNET_MORPH_MAX_R)
        throw std::runtime_error("postprocess_mask: unknown shape or radius outside 0.." + std::to_string(MI_UNET_MORPH_MAX_R));
    if (src.empty() || src.channels != 1) throw std::runtime_error("postprocess_mask: need a non-empty single-channel mask");
    if (cls < 1 || cls > 255) throw std::runtime_error("postprocess_mask: class outside 1..255");
    const uint8_t fgv = (uint8_t)cls;
    const int w = src.cols, h = src.rows;
    const size_t n = (size_t)w * h;
    const int min_area = mi_unet_target_min_area(h, w, min_area_frac);      // evaluated in float, src/postprocess.cpp:30,:66
    std::vector<uint8_t> mask(src.data);

    // 1. fill holes: components of (mask != cls) whose bbox touches no edge and whose area < min_area
    {
        std::vector<uint8_t> inv(n);
        for (size_t i = 0; i < n; ++i) inv[i] = mask[i] == fgv ? 0 : 255;
        const Labelling L = label8(inv.data(), w, h);
        std::vector<uint8_t> fill(L.stats.size(), 0);
        for (size_t r = 1; r < L.stats.size(); ++r) {
            const Stat &s = L.stats[r];
            fill[r] = s.area > 0 && s.left > 0 && s.top > 0 && s.right < w - 1 && s.bottom < h - 1 && s.area < min_area;
        }
        for (size_t i = 0; i < n; ++i)
            if (L.labels[i] && fill[L.labels[i]]) mask[i] = fgv;
    }
    // 2. binarise, close (dilate, erode), open (erode, dilate): the reference's is the 3x3 open alone
    std::vector<uint8_t> bin(n), tmp, op;
    for (size_t i = 0; i < n; ++i) bin[i] = mask[i] == fgv ? 255 : 0;
    morph_step(bin, tmp, w, h, morph.shape, morph.close_r, true);
    morph_step(tmp, bin, w, h, morph.shape, morph.close_r, false);
    morph_step(bin, tmp, w, h, morph.shape, morph.open_r, false);
    morph_step(tmp, op, w, h, morph.shape, morph.open_r, true);
    // 3. area filter, 4. map back to {0, cls}
    const Labelling L = label8(op.data(), w, h);
    medseg::Image8 out(h, w, 1, 0);
    for (size_t i = 0; i < n; ++i)
        if (L.labels[i] && L.stats[L.labels[i]].area >= min_area) out.data[i] = fgv;
    return out;
}
