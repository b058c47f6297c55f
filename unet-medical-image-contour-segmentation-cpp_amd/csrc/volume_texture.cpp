// volume_texture.cpp -- per component of a labelled stack its grey-level histogram and its 3-D co-occurrence tables (include/mi_unet.h:
// mi_unet_volume_texture): the argument checks, the definition as sequential host arithmetic
// (mi_unet_volume_texture_host), the function that turns the counts of one component into features (mi_unet_volume_texture_derive) and
// the entry point on the handle, which owns the stage's workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled
// (stage_common.h; tests/cpu/volume_texture_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "texture_common.h"

static_assert(sizeof(mi_unet_vtexture) == 32, "mi_unet_vtexture is 32 bytes without padding");
static_assert(sizeof(mi_unet_vtexture_opts) == 16, "mi_unet_vtexture_opts is four ints");
static_assert(sizeof(mi_unet_vtexture_features) == 144, "mi_unet_vtexture_features is 16 doubles and four int32 without padding");

namespace miunet {

namespace {

constexpr mi_unet_vtexture_opts kDefaultOpts{ MI_UNET_VTEX_COUNT, 32, 0, 1 };

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_texture_args(const char *fn, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vtexture_opts &o,
                       const mi_unet_vtexture *table, const uint32_t *hist)
{
    const std::string f = fn;
    if (!ids || !intensity || !table || !hist) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_texture_volume(f, D, H, W, m, o)) return rc;
    if ((int64_t)m * o.levels * o.levels > (int64_t)MI_UNET_VTEX_MAX_CELLS)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components at " + std::to_string(o.levels) + " levels pass 2^22 cells per table");
    return check_texture_bins(f, o);
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_texture_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vtexture_opts *opts,
                                mi_unet_vtexture *table, uint32_t *hist, uint32_t *glcm, uint32_t *glcm_axial)
{
    const mi_unet_vtexture_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_texture_args("mi_unet_volume_texture_host", ids, intensity, D, H, W, m, o, table, hist)) return rc;
    const int L = o.levels;
    const size_t dhw = (size_t)D * H * W, LL = (size_t)L * L;
    std::vector<mi_unet_vtexture> t((size_t)m);
    std::memset(t.data(), 0, t.size() * sizeof(mi_unet_vtexture));
    auto member = [&](int32_t id) { return id >= 1 && id <= m; };
    const std::vector<int32_t> key = texture_keys(ids, intensity, dhw, o, t);
    auto level = [&](size_t i) { return (size_t)(key[i] & 255); };
    std::memset(hist, 0, (size_t)m * L * sizeof(uint32_t));
    for (size_t i = 0; i < dhw; ++i)
        if (key[i]) ++hist[(size_t)(ids[i] - 1) * L + level(i)];
    for (int r = 0; r < m; ++r)
        for (int l = 0; l < L; ++l) t[r].levels_used += hist[(size_t)r * L + l] != 0;
    if (glcm) std::memset(glcm, 0, (size_t)m * LL * sizeof(uint32_t));
    if (glcm_axial) std::memset(glcm_axial, 0, (size_t)m * LL * sizeof(uint32_t));
    if (glcm || glcm_axial) {
        const int32_t *p = ids;
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x, ++p) {
                    if (!member(*p)) continue;
                    const size_t i = (size_t)(p - ids), row = ((size_t)(*p - 1) * L + level(i)) * L;
                    for (int dz = 0; dz <= (glcm ? 1 : 0); ++dz)
                        for (int dy = dz ? -1 : 0; dy <= 1; ++dy)
                            for (int dx = (dz || dy) ? -1 : 1; dx <= 1; ++dx) {
                                if (z + dz >= D || y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W) continue;
                                const size_t q = i + ((size_t)dz * H + dy) * W + dx;     // (dy, dx may be -1: size_t arithmetic wraps back)
                                if (ids[q] != *p) continue;
                                if (glcm) ++glcm[row + level(q)];
                                if (glcm_axial && dz == 0) ++glcm_axial[row + level(q)];
                            }
                }
        for (int r = 0; r < m; ++r)
            for (size_t c = 0; c < LL; ++c) {
                if (glcm) t[r].pairs += glcm[(size_t)r * LL + c];
                if (glcm_axial) t[r].pairs_axial += glcm_axial[(size_t)r * LL + c];
            }
    }
    std::memcpy(table, t.data(), t.size() * sizeof(mi_unet_vtexture));
    return MI_UNET_OK;
}

int mi_unet_volume_texture_derive(const mi_unet_vtexture *c, const uint32_t *hist, const uint32_t *glcm, int L, mi_unet_vtexture_features *out)
{
    const std::string f = "mi_unet_volume_texture_derive";
    if (!c || !hist || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_texture_component(f, c->voxels, L)) return rc;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    mi_unet_vtexture_features o;
    const double n = (double)c->voxels;
    double mu = 0.0;
    for (int l = 0; l < L; ++l) mu += (double)(l + 1) * ((double)hist[l] / n);
    double m2 = 0.0, m3 = 0.0, m4 = 0.0, ent = 0.0, uni = 0.0;
    int mode = 0;
    for (int l = 0; l < L; ++l) {
        const double p = (double)hist[l] / n, d = (double)(l + 1) - mu;
        m2 += p * d * d;
        m3 += p * d * d * d;
        m4 += p * d * d * d * d;
        if (hist[l]) ent -= p * std::log2(p);
        uni += p * p;
        if (hist[l] > hist[mode]) mode = l;
    }
    o.mean = mu;
    o.variance = m2;
    o.skewness = m2 > 0.0 ? m3 / (m2 * std::sqrt(m2)) : 0.0;
    o.kurtosis = m2 > 0.0 ? m4 / (m2 * m2) - 3.0 : 0.0;
    o.entropy = ent;
    o.uniformity = uni;
    o.mode = mode + 1;
    // the smallest level whose cumulative count reaches ceil(q voxels), q = num / 10
    auto quantile = [&](int64_t num) {
        const int64_t need = ((int64_t)c->voxels * num + 9) / 10;
        int64_t cum = 0;
        for (int l = 0; l < L; ++l) {
            cum += hist[l];
            if (cum >= need) return l + 1;
        }
        return L;                                               // (a histogram that holds fewer than `voxels`)
    };
    o.median = quantile(5);
    o.p10 = quantile(1);
    o.p90 = quantile(9);
    o.joint_max = o.joint_average = o.joint_variance = o.joint_entropy = o.contrast = o.dissimilarity = o.inverse_difference =
        o.inverse_difference_moment = o.angular_second_moment = o.correlation = nan;
    int64_t pairs = 0;
    if (glcm)
        for (int k = 0; k < L * L; ++k) pairs += glcm[k];
    if (pairs > 0) {
        const double den = 2.0 * (double)pairs;
        auto P = [&](int i, int j) { return ((double)glcm[i * L + j] + (double)glcm[j * L + i]) / den; };
        double jm = 0.0, ja = 0.0;
        for (int i = 0; i < L; ++i)
            for (int j = 0; j < L; ++j) {
                const double p = P(i, j);
                jm = std::max(jm, p);
                ja += (double)(i + 1) * p;
            }
        double jv = 0.0, je = 0.0, con = 0.0, dis = 0.0, inv = 0.0, idm = 0.0, asm2 = 0.0, cor = 0.0;
        for (int i = 0; i < L; ++i)
            for (int j = 0; j < L; ++j) {
                const double p = P(i, j), di = (double)(i + 1) - ja, dj = (double)(j + 1) - ja, k = (double)std::abs(i - j);
                jv += di * di * p;
                if (p > 0.0) je -= p * std::log2(p);
                con += k * k * p;
                dis += k * p;
                inv += p / (1.0 + k);
                idm += p / (1.0 + k * k);
                asm2 += p * p;
                cor += di * dj * p;
            }
        o.joint_max = jm; o.joint_average = ja; o.joint_variance = jv; o.joint_entropy = je; o.contrast = con; o.dissimilarity = dis;
        o.inverse_difference = inv; o.inverse_difference_moment = idm; o.angular_second_moment = asm2;
        o.correlation = jv > 0.0 ? cor / jv : nan;
    }
    *out = o;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_texture(mi_unet_t *h, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m,
                           const mi_unet_vtexture_opts *opts, mi_unet_vtexture *table, uint32_t *hist, uint32_t *glcm, uint32_t *glcm_axial)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vtexture_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_texture_args("mi_unet_volume_texture", ids, intensity, D, H, W, m, o, table, hist)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, M = (size_t)m, L = (size_t)o.levels;
    const size_t table_bytes = M * sizeof(mi_unet_vtexture), hist_bytes = M * L * sizeof(uint32_t), cells_bytes = M * L * L * sizeof(uint32_t);
    // device: keys (ids in place), intensity, table, hist, inter (then glcm), axial | range; pinned: the same up to axial
    Layout lay;
    const size_t at_keys = lay.take(dhw * sizeof(int32_t)), at_int = lay.take(dhw * sizeof(uint16_t)), at_table = lay.take(table_bytes);
    const size_t at_hist = lay.take(hist_bytes), at_inter = lay.take(cells_bytes), at_axial = lay.take(cells_bytes), host_need = lay.end;
    const size_t at_range = lay.take(M * sizeof(int2));
    hipStream_t s = h->stream;
    if (int rc = h->ws_vtx.reserve(lay.end, host_need, s)) return rc;
    uint8_t *const d = h->ws_vtx.d, *const p = h->ws_vtx.p;
    if (int rc = upload_stacks(h, h->ws_vtx, at_keys, ids, at_int, intensity, dhw)) return rc;
    const VolumeTextureArgs a = texture_args(D, H, W, m, o);
    // the 13-offset table is the sum of its two parts, so it needs both
    const int want = glcm ? (VTX_WANT_AXIAL | VTX_WANT_INTER) : glcm_axial ? VTX_WANT_AXIAL : 0;
    bool lds_table = true;
#ifdef MIUNET_EXPERIMENTS
    if (const char *v = std::getenv("MIUNET_VTX_EXP")) lds_table = std::atoi(v) != 1;            // 1: every count straight to memory
#endif
    int32_t *const d_keys = reinterpret_cast<int32_t *>(d + at_keys);
    int2 *const d_range = reinterpret_cast<int2 *>(d + at_range);
    mi_unet_vtexture *const d_table = reinterpret_cast<mi_unet_vtexture *>(d + at_table);
    uint32_t *const d_hist = reinterpret_cast<uint32_t *>(d + at_hist), *const d_inter = reinterpret_cast<uint32_t *>(d + at_inter);
    uint32_t *const d_axial = reinterpret_cast<uint32_t *>(d + at_axial);
    hipError_t e = launch_volume_texture_keys(d_keys, reinterpret_cast<const uint16_t *>(d + at_int), a, d_range, s);
    if (e == hipSuccess) e = launch_volume_texture_pairs(d_keys, a, want, lds_table, d_hist, d_inter, d_axial, s);
    if (e == hipSuccess) e = launch_volume_texture_finish(d_range, a, want, d_hist, d_inter, d_axial, d_table, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume texture launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p + at_table, d_table, table_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p + at_hist, d_hist, hist_bytes, hipMemcpyDeviceToHost, s));
    if (glcm) HIP_TRY(hipMemcpyAsync(p + at_inter, d_inter, cells_bytes, hipMemcpyDeviceToHost, s));
    if (glcm_axial) HIP_TRY(hipMemcpyAsync(p + at_axial, d_axial, cells_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    mi_unet_vtexture *const t = reinterpret_cast<mi_unet_vtexture *>(p + at_table);
    if (!glcm_axial)
        for (int r = 0; r < m; ++r) t[r].pairs_axial = 0;       // (a part of glcm, not asked for as a table)
    std::memcpy(table, t, table_bytes);
    std::memcpy(hist, p + at_hist, hist_bytes);
    if (glcm) std::memcpy(glcm, p + at_inter, cells_bytes);
    if (glcm_axial) std::memcpy(glcm_axial, p + at_axial, cells_bytes);
    return MI_UNET_OK;
}
#endif

}  // extern "C"
