// volume_interp.hip -- slices put between the slices of a stack of masks, shape-based (include/mi_unet.h: mi_unet_volume_interp;
// DESIGN.md 7.16).  Per value plane and slice the exact squared in-plane distance of every pixel to the nearest pixel of the other
// state, in two passes -- down and up the columns, then along the rows out of LDS -- built like score.hip's k_score_columns / k_score_rows
// and volume_clean.hip's k_vc_z / k_vc_x, but unthresholded, two-sided (either state is a seed for the other) and anisotropic in the
// plane.  The signed field is computed once per slice; the blend reads two of its slices per slice pair and decides every voxel between
// them by one comparison of 64-bit products.  Byte and integer work, exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "wave.h"

namespace miunet {

namespace vi {

using namespace wave;

constexpr unsigned SENT = 0x7FFFu;          // no pixel of the other state in this column (a distance is at most 8191)
constexpr unsigned STATE = 0x8000u;         // bit 15 of a column word: the pixel is in the set

// The workspace of a call: N = n * D * H * W input voxels of all planes.
struct Ws {
    uint16_t *g;                    // [N] column words: the index distance along y to the nearest pixel of the other state | the state
    int32_t *field;                 // [N] + e where set, - e where unset
    unsigned *both;                 // [n * D] bit 0: the slice has a set pixel, bit 1: an unset one; 3 = a search can end
    size_t total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline Ws carve(void *base, size_t N, size_t slices)
{
    uint8_t *p = static_cast<uint8_t *>(base);
    Ws w;
    size_t at = 0;
    w.g = reinterpret_cast<uint16_t *>(p + at); at += up256(N * sizeof(uint16_t));
    w.field = reinterpret_cast<int32_t *>(p + at); at += up256(N * sizeof(int32_t));
    w.both = reinterpret_cast<unsigned *>(p + at); at += up256(slices * sizeof(unsigned));
    w.total = at;
    return w;
}

struct Vals { int v[VOLUME_MAX_VALUES]; };

// ---- columns: the 1-D distance to the other state ------------------------------------------------------------------------------------
// One wave per 64 columns of slice blockIdx.y of plane blockIdx.z, a lane per column, consecutive lanes along x.  Down the column the
// distance to the last pixel above whose state differs from the pixel's own, back up the minimum with the distance to the next one
// below.  The wave's columns tell whether the slice holds set and unset pixels: one atomic per wave.
__global__ __launch_bounds__(64) void k_vi_columns(const uint8_t *__restrict__ masks, Vals a, int H, int W, uint16_t *__restrict__ g_all,
                                                   unsigned *both)
{
    const int z = blockIdx.y, D = gridDim.y, k = blockIdx.z, x = blockIdx.x * 64 + threadIdx.x;
    const int v = pick_value(a.v, k);
    const size_t hw = (size_t)H * W;
    const uint8_t *const m = masks + (size_t)z * hw;
    uint16_t *const g = g_all + ((size_t)k * D + z) * hw;
    bool any_set = false, any_unset = false;
    if (x < W) {
        unsigned d = SENT;
        bool prev = false;
#pragma unroll 4
        for (int y = 0; y < H; ++y) {
            const bool cur = m[(size_t)y * W + x] == v;
            d = (y > 0 && cur != prev) ? 1u : min(d + 1u, SENT);
            g[(size_t)y * W + x] = (uint16_t)(d | (cur ? STATE : 0u));
            any_set |= cur; any_unset |= !cur;
            prev = cur;
        }
        d = SENT;
#pragma unroll 4
        for (int y = H - 1; y >= 0; --y) {
            const unsigned w = g[(size_t)y * W + x];
            const bool cur = (w & STATE) != 0;
            d = (y < H - 1 && cur != prev) ? 1u : min(d + 1u, SENT);
            if (d < (w & SENT)) g[(size_t)y * W + x] = (uint16_t)(d | (w & STATE));
            prev = cur;
        }
    }
    const unsigned bits = (__ballot(any_set) ? 1u : 0u) | (__ballot(any_unset) ? 2u : 0u);
    if (threadIdx.x == 0) atomicOr(&both[k * D + z], bits);
}

// ---- rows: the signed squared distance, the hot path -----------------------------------------------------------------------------------
// Workgroup (y, z, plane) owns one row.  In a slice that is all one state every pixel is + NONE or - NONE and nothing is searched.
// Otherwise the row's column words are staged in LDS -- whatever the width: the nearest pixel may lie anywhere -- and a lane per pixel
// scans outward from x: a pixel of the other state at dx contributes (ux dx)^2, one of the same state (ux dx)^2 + (uy h)^2 with h its
// column distance.  The scan stops once (ux dx)^2 alone reaches the best so far, or when both sides have left the row.  (ux dx) and
// (uy h) stay below 46341 by the stage's limit, dx <= W - 1 and h <= H - 1, so every term and every sum is a positive int.
__global__ __launch_bounds__(256) void k_vi_rows(const uint16_t *__restrict__ g_all, const unsigned *__restrict__ both, int H, int W, int ux,
                                                 int uy, int32_t *__restrict__ field)
{
    __shared__ uint16_t s_g[VINTERP_MAX_SIDE];
    const int y = blockIdx.x, z = blockIdx.y, D = gridDim.y, k = blockIdx.z;
    const size_t row = (((size_t)k * D + z) * H + y) * (size_t)W;
    const uint16_t *const g = g_all + row;
    int32_t *const f = field + row;
    const int tid = threadIdx.x;
    if (both[k * D + z] != 3u) {                                // (workgroup-uniform)
        for (int x = tid; x < W; x += 256) f[x] = (g[x] & STATE) ? VINTERP_NONE : -VINTERP_NONE;
        return;
    }
    for (int x = tid; x < W; x += 256) s_g[x] = g[x];
    __syncthreads();
    for (int x = tid; x < W; x += 256) {
        const unsigned w0 = s_g[x], st = w0 & STATE;
        const int h0 = (int)(w0 & SENT);
        int best = h0 == (int)SENT ? VINTERP_NONE : (uy * h0) * (uy * h0);
        for (int dx = 1; ; ++dx) {
            const int xl = x - dx, xr = x + dx;
            if (xl < 0 && xr >= W) break;
            const int t = (ux * dx) * (ux * dx);
            if (t >= best) break;
            if (xl >= 0) {
                const unsigned c = s_g[xl];
                const int h = (int)(c & SENT);
                if ((c & STATE) != st) best = t;                // (t < best)
                else if (h != (int)SENT) best = min(best, t + (uy * h) * (uy * h));
            }
            if (xr < W) {
                const unsigned c = s_g[xr];
                const int h = (int)(c & SENT);
                if ((c & STATE) != st) best = min(best, t);
                else if (h != (int)SENT) best = min(best, t + (uy * h) * (uy * h));
            }
        }
        f[x] = st ? best : -best;
    }
}

// ---- blend: the k output slices of a slice pair ------------------------------------------------------------------------------------------
// A lane per (y, x) of the pair (z, z + 1) of one plane, consecutive lanes along x: both signed values are read once, the stores of a
// wave are 64 consecutive bytes of one output slice.  Pair D - 1 is the last slice by itself.  counts [plane][pair][5] = in_voxels (the
// j = 0 slices are the input slices, each once), out_voxels, mixed, mixed_set, ties: summed in the wave, then in LDS, one atomic per
// workgroup and non-zero count into the pair's own five words -- atomics on one address are served one after another, and one set of
// words for a whole plane made this kernel wait for them; the caller adds the pairs up.
__global__ __launch_bounds__(256) void k_vi_blend(const int32_t *__restrict__ field, Vals a, int D, unsigned hw, int kf, uint8_t *__restrict__ out,
                                                  unsigned long long *counts)
{
    __shared__ int s_c[4][5];
    const int z = blockIdx.y, p = blockIdx.z;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    int c_in = 0, c_out = 0, c_mixed = 0, c_mset = 0, c_ties = 0;
    if (i < hw) {
        const uint8_t v = (uint8_t)pick_value(a.v, p);
        const size_t Dp = (size_t)(D - 1) * kf + 1;
        const int32_t fa = field[((size_t)p * D + z) * hw + i];
        uint8_t *o = out + ((size_t)p * Dp + (size_t)z * kf) * hw + i;
        const bool sa = fa > 0;
        o[0] = sa ? v : (uint8_t)0;
        c_in = c_out = sa;
        if (z + 1 < D) {
            const int32_t fb = field[((size_t)p * D + z + 1) * hw + i];
            const bool sb = fb > 0;
            const unsigned long long e_set = (unsigned long long)(sa ? fa : fb), e_unset = (unsigned long long)(sa ? -fb : -fa);
            for (int j = 1; j < kf; ++j) {
                o += hw;
                bool set = sa;
                if (sa != sb) {
                    const unsigned long long w_set = (unsigned long long)(sa ? kf - j : j), w_unset = (unsigned long long)kf - w_set;
                    const unsigned long long lhs = w_set * w_set * e_set, rhs = w_unset * w_unset * e_unset;
                    set = lhs >= rhs;
                    ++c_mixed;
                    c_mset += set;
                    c_ties += lhs == rhs;
                }
                *o = set ? v : (uint8_t)0;
                c_out += set;
            }
        }
    }
    c_in = wave_sum(c_in); c_out = wave_sum(c_out); c_mixed = wave_sum(c_mixed); c_mset = wave_sum(c_mset); c_ties = wave_sum(c_ties);
    if ((threadIdx.x & 63) == 0) {
        int *const w = s_c[threadIdx.x >> 6];
        w[0] = c_in; w[1] = c_out; w[2] = c_mixed; w[3] = c_mset; w[4] = c_ties;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int tot = s_c[0][threadIdx.x] + s_c[1][threadIdx.x] + s_c[2][threadIdx.x] + s_c[3][threadIdx.x];
        if (tot) atomicAdd(counts + ((size_t)p * D + z) * 5 + threadIdx.x, (unsigned long long)tot);
    }
}

// ---- lerp: the intensity between the slices ----------------------------------------------------------------------------------------------
// A lane per (y, x) of the pair (z, z + 1): slice z k + j = ((k - j) a + j b + k / 2) / k, at most 16 * 65535 + 8.
__global__ __launch_bounds__(256) void k_vi_lerp(const uint16_t *__restrict__ in, int D, unsigned hw, int kf, uint16_t *__restrict__ out)
{
    const int z = blockIdx.y;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= hw) return;
    const unsigned va = in[(size_t)z * hw + i];
    uint16_t *o = out + (size_t)z * kf * hw + i;
    o[0] = (uint16_t)va;
    if (z + 1 >= D) return;
    const unsigned vb = in[(size_t)(z + 1) * hw + i], k = (unsigned)kf;
    for (unsigned j = 1; j < k; ++j) {
        o += hw;
        *o = (uint16_t)(((k - j) * va + j * vb + k / 2) / k);
    }
}

}  // namespace vi

size_t volume_interp_workspace_bytes(int D, int H, int W, int n) { return vi::carve(nullptr, (size_t)D * H * W * n, (size_t)D * n).total; }

hipError_t launch_volume_interp(const uint8_t *masks, const uint16_t *intensity, const VolumeInterpArgs &a, uint8_t *out,
                                uint16_t *intensity_out, unsigned long long *counts, void *ws, hipStream_t s)
{
    const int D = a.D, H = a.H, W = a.W, n = a.n, k = a.k;
    if (!masks || !out || !counts || !ws || n < 1 || n > VOLUME_MAX_VALUES || k < 1 || k > VINTERP_MAX_FACTOR) return hipErrorInvalidValue;
    if (D < 1 || H < 1 || W < 1 || D > VINTERP_MAX_SIDE || H > VINTERP_MAX_SIDE || W > VINTERP_MAX_SIDE) return hipErrorInvalidValue;
    if ((intensity == nullptr) != (intensity_out == nullptr) || a.ux < 1 || a.uy < 1) return hipErrorInvalidValue;
    const unsigned long long Dp = (unsigned long long)(D - 1) * k + 1, hw64 = (unsigned long long)H * W;
    if (Dp * hw64 * n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned long long tx = (unsigned long long)(W - 1) * a.ux, ty = (unsigned long long)(H - 1) * a.uy;
    if ((W > 1 && a.ux > 46340 / (W - 1)) || (H > 1 && a.uy > 46340 / (H - 1)) || tx * tx + ty * ty >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned hw = (unsigned)hw64;
    const vi::Ws w = vi::carve(ws, (size_t)D * hw * n, (size_t)D * n);
    vi::Vals vals;
    for (int j = 0; j < VOLUME_MAX_VALUES; ++j) vals.v[j] = a.v[j];
    if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * D * 5 * sizeof(unsigned long long), s)) return e;
    if (hipError_t e = hipMemsetAsync(w.both, 0, (size_t)n * D * sizeof(unsigned), s)) return e;
    hipLaunchKernelGGL(vi::k_vi_columns, dim3((unsigned)(W + 63) / 64u, (unsigned)D, (unsigned)n), dim3(64), 0, s, masks, vals, H, W, w.g, w.both);
    hipLaunchKernelGGL(vi::k_vi_rows, dim3((unsigned)H, (unsigned)D, (unsigned)n), dim3(256), 0, s, w.g, w.both, H, W, a.ux, a.uy, w.field);
    const unsigned gx = (hw + 255u) / 256u;
    hipLaunchKernelGGL(vi::k_vi_blend, dim3(gx, (unsigned)D, (unsigned)n), dim3(256), 0, s, w.field, vals, D, hw, k, out, counts);
    if (intensity) hipLaunchKernelGGL(vi::k_vi_lerp, dim3(gx, (unsigned)D), dim3(256), 0, s, intensity, D, hw, k, intensity_out);
    return hipGetLastError();
}

}  // namespace miunet
