// volume_mesh.cpp -- the border of a stack of masks as a quad mesh (include/mi_unet.h: mi_unet_volume_mesh): the argument
// checks, the definition as sequential host arithmetic (mi_unet_volume_mesh_host), the two functions that turn a mesh into millimetres
// (mi_unet_volume_mesh_positions, _derive) and the entry point on the handle, which owns the stage's workspace.  With
// MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h; tests/cpu/volume_mesh_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_mesh_vertex) == 16, "mi_unet_mesh_vertex is 16 bytes without padding");
static_assert(sizeof(mi_unet_mesh_stat) == 48, "mi_unet_mesh_stat is 48 bytes without padding");

namespace miunet {

namespace {

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_mesh_args(const char *fn, const uint8_t *masks, int D, int H, int W, const int *values, int n, int placement,
                    const mi_unet_mesh_vertex *verts, int cap_verts, const int32_t *quads, int cap_quads, const mi_unet_mesh_stat *stats)
{
    const std::string f = fn;
    if (!masks || !values || !stats) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_min1(f, D, H, W)) return rc;
    if (int rc = check_values(f, values, n, MI_UNET_VOLUME_MAX_VALUES)) return rc;
    if (!product_below_2_31(6, (long long)D + 1, (long long)H + 1, (long long)W + 1)) return fail(MI_UNET_EARG, f + ": 6 * (D + 1) * (H + 1) * (W + 1) must stay below 2^31");
    if (placement != MI_UNET_MESH_FACES && placement != MI_UNET_MESH_NETS)
        return fail(MI_UNET_EARG, f + ": placement " + std::to_string(placement) + " is neither MI_UNET_MESH_FACES nor MI_UNET_MESH_NETS");
    if (cap_verts < 0 || cap_quads < 0)
        return fail(MI_UNET_EARG, f + ": caps " + std::to_string(cap_verts) + ", " + std::to_string(cap_quads) + " (0 .. 2^31 - 1)");
    if ((!verts && cap_verts) || (!quads && cap_quads)) return fail(MI_UNET_EARG, f + ": a null array takes a cap of 0");
    return MI_UNET_OK;
}

mi_unet_mesh_stat make_stat(int value, int placement, int64_t quads, int64_t verts, int64_t qx, int64_t qy, int64_t qz)
{
    mi_unet_mesh_stat s;
    s.value = value; s.placement = placement;
    s.quads = quads; s.verts = verts; s.quads_x = qx; s.quads_y = qy; s.quads_z = qz;
    return s;
}

// the corners of the face in direction d relative to the voxel's own corner, (dx, dy, dz) each (include/mi_unet.h: ORIENTATION)
constexpr int kFace[6][4][3] = {
    { { 0, 0, 0 }, { 0, 0, 1 }, { 0, 1, 1 }, { 0, 1, 0 } }, { { 1, 0, 0 }, { 1, 1, 0 }, { 1, 1, 1 }, { 1, 0, 1 } },
    { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 0, 1 }, { 0, 0, 1 } }, { { 0, 1, 0 }, { 0, 1, 1 }, { 1, 1, 1 }, { 1, 1, 0 } },
    { { 0, 0, 0 }, { 0, 1, 0 }, { 1, 1, 0 }, { 1, 0, 0 } }, { { 0, 0, 1 }, { 1, 0, 1 }, { 1, 1, 1 }, { 0, 1, 1 } } };

// One plane: the vertices in corner order (with `map`, corner -> vertex index or -1), then the quads in voxel order.
void mesh_plane(const uint8_t *masks, int D, int H, int W, int value, int placement, mi_unet_mesh_vertex *verts, int cap_verts, int32_t *quads,
                int cap_quads, mi_unet_mesh_stat *stat, std::vector<int32_t> &map)
{
    const size_t hw = (size_t)H * W;
    auto in = [&](int x, int y, int z) { return x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D && masks[(size_t)z * hw + (size_t)y * W + x] == value; };
    int64_t nv = 0, nq = 0, per_axis[3] = { 0, 0, 0 };
    size_t c = 0;
    for (int k = 0; k <= D; ++k)
        for (int j = 0; j <= H; ++j)
            for (int i = 0; i <= W; ++i, ++c) {
                bool m[2][2][2];                                // [dz][dy][dx]
                for (int b = 0; b < 8; ++b) m[b >> 2][(b >> 1) & 1][b & 1] = in(i - 1 + (b & 1), j - 1 + ((b >> 1) & 1), k - 1 + (b >> 2));
                int cut = 0, o[3] = { 0, 0, 0 };
                for (int p = 0; p < 2; ++p)
                    for (int q = 0; q < 2; ++q) {
                        if (m[q][p][0] != m[q][p][1]) { ++cut; o[1] += 2 * p - 1; o[2] += 2 * q - 1; }     // along x at dy = p, dz = q
                        if (m[q][0][p] != m[q][1][p]) { ++cut; o[0] += 2 * p - 1; o[2] += 2 * q - 1; }     // along y at dx = p, dz = q
                        if (m[0][q][p] != m[1][q][p]) { ++cut; o[0] += 2 * p - 1; o[1] += 2 * q - 1; }     // along z at dx = p, dy = q
                    }
                map[c] = cut ? (int32_t)nv : -1;
                if (!cut) continue;
                if (nv < cap_verts) {
                    mi_unet_mesh_vertex &v = verts[nv];
                    v.x = i; v.y = j; v.z = k;
                    const bool nets = placement == MI_UNET_MESH_NETS;
                    v.ox = (int8_t)(nets ? o[0] : 0); v.oy = (int8_t)(nets ? o[1] : 0); v.oz = (int8_t)(nets ? o[2] : 0);
                    v.n = (uint8_t)(nets ? cut : 1);
                }
                ++nv;
            }
    const int w1 = W + 1;
    const size_t hw1 = (size_t)(H + 1) * w1;
    static const int dir[6][3] = { { -1, 0, 0 }, { 1, 0, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 0, -1 }, { 0, 0, 1 } };
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                if (!in(x, y, z)) continue;
                for (int d = 0; d < 6; ++d) {
                    if (in(x + dir[d][0], y + dir[d][1], z + dir[d][2])) continue;
                    if (nq < cap_quads)
                        for (int j = 0; j < 4; ++j)
                            quads[4 * nq + j] = map[(size_t)(z + kFace[d][j][2]) * hw1 + (size_t)(y + kFace[d][j][1]) * w1 + (x + kFace[d][j][0])];
                    ++nq;
                    ++per_axis[d >> 1];
                }
            }
    if (verts && nv < cap_verts) std::memset(verts + nv, 0, (size_t)(cap_verts - nv) * sizeof(mi_unet_mesh_vertex));
    if (quads && nq < cap_quads) std::memset(quads + 4 * nq, 0, (size_t)(cap_quads - nq) * 4 * sizeof(int32_t));
    *stat = make_stat(value, placement, nq, nv, per_axis[0], per_axis[1], per_axis[2]);
}

bool good_spacing(const double *s)
{
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(s[a]) || !(s[a] > 0.0)) return false;
    return true;
}

inline void position(const mi_unet_mesh_vertex &v, const double *sp, double *p)
{
    const double den = 2.0 * v.n;
    p[0] = (v.x + v.ox / den) * sp[0];
    p[1] = (v.y + v.oy / den) * sp[1];
    p[2] = (v.z + v.oz / den) * sp[2];
}

int check_vertices(const std::string &f, const mi_unet_mesh_vertex *verts, int nv, const double *spacing)
{
    if (nv < 0) return fail(MI_UNET_EARG, f + ": " + std::to_string(nv) + " vertices");
    if (!spacing || (!verts && nv)) return fail(MI_UNET_EARG, f + ": null argument");
    if (!good_spacing(spacing)) return fail(MI_UNET_EARG, f + ": every spacing must be finite and > 0");
    for (int i = 0; i < nv; ++i)
        if (verts[i].n == 0) return fail(MI_UNET_EARG, f + ": vertex " + std::to_string(i) + " has n == 0");
    return MI_UNET_OK;
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_mesh_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, int placement, mi_unet_mesh_vertex *verts,
                             int cap_verts, int32_t *quads, int cap_quads, mi_unet_mesh_stat *stats)
{
    if (int rc = check_mesh_args("mi_unet_volume_mesh_host", masks, D, H, W, values, n, placement, verts, cap_verts, quads, cap_quads, stats)) return rc;
    std::vector<int32_t> map((size_t)(D + 1) * (H + 1) * (W + 1));
    for (int k = 0; k < n; ++k)
        mesh_plane(masks, D, H, W, values[k], placement, verts ? verts + (size_t)k * cap_verts : nullptr, cap_verts,
                   quads ? quads + (size_t)k * cap_quads * 4 : nullptr, cap_quads, stats + k, map);
    return MI_UNET_OK;
}

int mi_unet_volume_mesh_positions(const mi_unet_mesh_vertex *verts, int nv, const double spacing_xyz[3], float *xyz)
{
    const std::string f = "mi_unet_volume_mesh_positions";
    if (int rc = check_vertices(f, verts, nv, spacing_xyz)) return rc;
    if (!xyz && nv) return fail(MI_UNET_EARG, f + ": null argument");
    for (int i = 0; i < nv; ++i) {
        double p[3];
        position(verts[i], spacing_xyz, p);
        for (int a = 0; a < 3; ++a) xyz[3 * (size_t)i + a] = (float)p[a];
    }
    return MI_UNET_OK;
}

int mi_unet_volume_mesh_derive(const mi_unet_mesh_vertex *verts, int nv, const int32_t *quads, int nq, const double spacing_xyz[3],
                               mi_unet_mesh_metrics *out)
{
    const std::string f = "mi_unet_volume_mesh_derive";
    if (!out) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_vertices(f, verts, nv, spacing_xyz)) return rc;
    if (nq < 0) return fail(MI_UNET_EARG, f + ": " + std::to_string(nq) + " quads");
    if (!quads && nq) return fail(MI_UNET_EARG, f + ": null argument");
    for (size_t i = 0; i < (size_t)nq * 4; ++i)
        if (quads[i] < 0 || quads[i] >= nv)
            return fail(MI_UNET_EARG, f + ": quad " + std::to_string(i / 4) + " refers to vertex " + std::to_string(quads[i]) + " of " + std::to_string(nv));
    double area = 0.0, volume = 0.0;
    for (int q = 0; q < nq; ++q) {
        double p[4][3];
        for (int j = 0; j < 4; ++j) position(verts[quads[4 * (size_t)q + j]], spacing_xyz, p[j]);
        for (int t = 0; t < 2; ++t) {
            const double *a = p[0], *b = p[1 + t], *c = p[2 + t];
            const double u[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, w[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
            const double nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
            area += 0.5 * std::sqrt(nx * nx + ny * ny + nz * nz);
            const double bx = b[1] * c[2] - b[2] * c[1], by = b[2] * c[0] - b[0] * c[2], bz = b[0] * c[1] - b[1] * c[0];
            volume += (a[0] * bx + a[1] * by + a[2] * bz) / 6.0;
        }
    }
    out->area_mm2 = area;
    out->volume_mm3 = volume;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_mesh(mi_unet_t *h, const uint8_t *masks, int D, int H, int W, const int *values, int n, int placement,
                        mi_unet_mesh_vertex *verts, int cap_verts, int32_t *quads, int cap_quads, mi_unet_mesh_stat *stats)
{
    if (int rc = check_handle(h, false)) return rc;
    if (int rc = check_mesh_args("mi_unet_volume_mesh", masks, D, H, W, values, n, placement, verts, cap_verts, quads, cap_quads, stats)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, count_bytes = 5 * sizeof(unsigned long long);
    // device: the volume, the counts, the kernels' workspace; pinned: the volume, the counts.  The kept prefixes of one plane have buffers
    // of their own, sized once its counts are known
    const size_t at_counts = up256(dhw), at_ws = at_counts + up256(count_bytes);
    const size_t dev_need = at_ws + volume_mesh_workspace_bytes(D, H, W), host_need = at_ws;
    hipStream_t s = h->stream;
    if (int rc = h->ws_vmesh.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vmesh.d, *const p = h->ws_vmesh.p;
    host_copy(h, p, masks, dhw);
    HIP_TRY(hipMemcpyAsync(d, p, dhw, hipMemcpyHostToDevice, s));
    for (int k = 0; k < n; ++k) {
        VolumeMeshArgs a;
        a.D = D; a.H = H; a.W = W; a.value = values[k]; a.placement = placement;
        hipError_t e = launch_volume_mesh_count(d, a, reinterpret_cast<unsigned long long *>(d + at_counts), d + at_ws, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume mesh launch: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(p + at_counts, d + at_counts, count_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                       // the counts size the plane's outputs
        const unsigned long long *const c = reinterpret_cast<const unsigned long long *>(p + at_counts);
        stats[k] = make_stat(values[k], placement, (int64_t)c[0], (int64_t)c[1], (int64_t)c[2], (int64_t)c[3], (int64_t)c[4]);
        const int keep_v = (int)std::min<int64_t>(stats[k].verts, cap_verts), keep_q = (int)std::min<int64_t>(stats[k].quads, cap_quads);
        mi_unet_mesh_vertex *const out_v = verts ? verts + (size_t)k * cap_verts : nullptr;
        int32_t *const out_q = quads ? quads + (size_t)k * cap_quads * 4 : nullptr;
        if (keep_v || keep_q) {
            const size_t v_bytes = (size_t)keep_v * sizeof(mi_unet_mesh_vertex), q_bytes = (size_t)keep_q * 4 * sizeof(int32_t);
            const size_t at_q = up256(v_bytes), out_need = at_q + up256(q_bytes);
            if (int rc = h->ws_vmesh_out.reserve(out_need, out_need, s)) return rc;     // (nothing of the stage is in flight on it here)
            uint8_t *const od = h->ws_vmesh_out.d, *const op = h->ws_vmesh_out.p;
            e = launch_volume_mesh_emit(a, d + at_ws, keep_v ? reinterpret_cast<mi_unet_mesh_vertex *>(od) : nullptr, keep_v,
                                        keep_q ? reinterpret_cast<int32_t *>(od + at_q) : nullptr, keep_q, s);
            if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume mesh launch: ") + hipGetErrorString(e));
            if (keep_v) HIP_TRY(hipMemcpyAsync(op, od, v_bytes, hipMemcpyDeviceToHost, s));
            if (keep_q) HIP_TRY(hipMemcpyAsync(op + at_q, od + at_q, q_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (keep_v) host_copy(h, out_v, op, v_bytes);
            if (keep_q) host_copy(h, out_q, op + at_q, q_bytes);
        }
        // the zero tails: the complement of the kept prefixes
        if (out_v && keep_v < cap_verts) std::memset(out_v + keep_v, 0, (size_t)(cap_verts - keep_v) * sizeof(mi_unet_mesh_vertex));
        if (out_q && keep_q < cap_quads) std::memset(out_q + 4 * (size_t)keep_q, 0, (size_t)(cap_quads - keep_q) * 4 * sizeof(int32_t));
    }
    return MI_UNET_OK;
}
#endif

}  // extern "C"
