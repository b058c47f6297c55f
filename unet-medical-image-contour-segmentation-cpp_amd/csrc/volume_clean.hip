// volume_clean.hip -- a stack of masks cleaned as one volume, per value plane: 3-D cavity fill, then close and open by a ball given in
// the caller's spacing unit (include/mi_unet.h: mi_unet_volume_clean).  A dilation by the ball B(r) is the set of
// voxels whose squared distance to the set is at most r^2: a separable, thresholded, exact distance transform in three passes -- along
// z, along y, along x -- built like score_volume.hip's, whose cost grows with the ball's half-widths, not with its volume.  An erosion
// is the complement of the dilation of the complement taken inside the volume.  The fill labels the complement with volume.hip's
// lock-free union-find.  Byte and integer work, exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "cc_common.h"
#include "kernel_common.h"
#include "wave.h"

namespace miunet {

namespace vc {

using namespace wave;

// The workspace of a call: N = n * D * H * W voxels of all planes.  The fill's forest and flags lie in f and g, which the passes of
// the morphology use only after the fill has written cur.
struct Ws {
    uint8_t *cur;                   // [N] the planes' current sets, 0 / 1
    uint16_t *g;                    // [N] index distance along z to the nearest seed of the (y, x) column, capped; the fill's flags (bytes)
    unsigned *f;                    // [N] min over dy of (g uz)^2 + (dy uy)^2, saturated at r^2 + 1; the fill's forest
    size_t total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline Ws carve(void *base, size_t N)
{
    uint8_t *p = static_cast<uint8_t *>(base);
    Ws w;
    size_t at = 0;
    w.cur = p + at; at += up256(N);
    w.g = reinterpret_cast<uint16_t *>(p + at); at += up256(N * sizeof(uint16_t));
    w.f = reinterpret_cast<unsigned *>(p + at); at += up256(N * sizeof(unsigned));
    w.total = at;
    return w;
}

struct Vals { int v[VOLUME_MAX_VALUES]; };

// One ball under one spacing: the half-widths already cut to the sides they run along (a longer one reaches nothing more).
struct Ball { int ux, uy, uz, ex, ey, ez; unsigned r2; };

// the workgroup's sum of c, added to *dst by one lane (every lane of the workgroup calls this)
__device__ __forceinline__ void block_count(int c, unsigned long long *dst, int *s_n)
{
    const int tot = wave_offsets(wave_sum(c), s_n).y;
    if (threadIdx.x == 0 && tot) atomicAdd(dst, (unsigned long long)tot);
}

// Every kernel below but k_vc_z and k_vc_faces runs one lane per voxel, consecutive lanes along x: workgroup blockIdx.x of plane
// blockIdx.y takes the voxels 256 * blockIdx.x .. + 255 of the plane.

// ---- set: the plane's set as bytes 0 / 1 (no fill) -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vc_set(const uint8_t *__restrict__ masks, Vals a, unsigned dhw, uint8_t *__restrict__ cur,
                                                unsigned long long *counts)
{
    __shared__ int s_n[4];
    const unsigned k = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    int c = 0;
    if (i < dhw) {
        c = masks[i] == pick_value(a.v, (int)k);
        cur[(size_t)k * dhw + i] = (uint8_t)c;
    }
    block_count(c, counts + 4 * k, s_n);
}

// ---- fill: the complement labelled with connectivity 6 (k_vol_init and k_vol_merge<1> of volume.hip, on the test masks != v) -----------
// The parent of a background voxel is the first voxel of its run inside the lane's 64-voxel segment; a run never continues from
// x = W - 1 (dhw is a multiple of W, so x == 0 marks the start of every row, slice and plane).
__global__ __launch_bounds__(256) void k_vc_bg_init(const uint8_t *__restrict__ masks, Vals a, unsigned dhw, int W, int *parent)
{
    const unsigned k = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    const bool in = i < dhw;
    const bool f = in && masks[i] != pick_value(a.v, (int)k);
    const unsigned x = (in ? i : 0u) % (unsigned)W;
    const int lane = threadIdx.x & 63;
    const unsigned long long fm = __ballot(f);
    const unsigned long long prev = (fm << 1) & ~__ballot(x == 0);
    const unsigned long long starts = fm & ~prev;
    if (in) {
        const int gi = (int)(k * dhw + i);
        int p = -1;
        if (f) {
            const unsigned long long below = starts & ((2ull << lane) - 1ull);
            p = gi - (lane - (63 - __builtin_clzll(below)));
        }
        parent[gi] = p;
    }
}

// Unions with the three earlier face neighbours, the implied ones left out (volume.hip: the left neighbour is in the voxel's run
// unless the run was cut at a 64-lane boundary; a neighbour above, in y or in z, is skipped when the left neighbour and its neighbour
// above are background too).  Every union is pp::unite; its loop ends by its own data.
__global__ __launch_bounds__(256) void k_vc_bg_merge(const uint8_t *__restrict__ masks, Vals a, unsigned dhw, int H, int W, int *parent)
{
    const unsigned k = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= dhw) return;
    const int v = pick_value(a.v, (int)k);
    if (masks[i] == v) return;
    const int hw = H * W;
    const int z = (int)(i / (unsigned)hw), rem = (int)(i - (unsigned)z * (unsigned)hw), y = rem / W, x = rem - y * W;
    const uint8_t *const m = masks + i;
    const int gi = (int)(k * dhw + i);
    const bool l = x > 0 && m[-1] != v;
    if (l && (threadIdx.x & 63) == 0) pp::unite(parent, gi, gi - 1);
    if (y > 0 && m[-W] != v && !(l && m[-W - 1] != v)) pp::unite(parent, gi, gi - W);
    if (z > 0 && m[-hw] != v && !(l && m[-hw - 1] != v)) pp::unite(parent, gi, gi - hw);
}

// The roots that reach a face, flagged from the faces' own voxels: item j of a plane is a voxel of the two z faces (H W each, lanes
// along x), then of the two y faces (D W each, lanes along x), then of the two x faces (D H each).  The forest is final here; every
// lane that reaches a root stores the same 1.
__global__ __launch_bounds__(256) void k_vc_faces(const int *__restrict__ parent, unsigned dhw, int D, int H, int W, uint8_t *flag)
{
    const unsigned k = blockIdx.y;
    const long long hw = (long long)H * W, dw = (long long)D * W, dh = (long long)D * H;
    long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    long long local;
    if (j < 2 * hw) {
        local = (j >= hw ? (D - 1) * hw + (j - hw) : j);
    } else if ((j -= 2 * hw) < 2 * dw) {
        const int side = j >= dw;
        const long long r = j - side * dw, z = r / W, x = r - z * W;
        local = z * hw + (side ? (long long)(H - 1) * W : 0) + x;
    } else if ((j -= 2 * dw) < 2 * dh) {
        const int side = j >= dh;
        const long long r = j - side * dh, z = r / H, y = r - z * H;
        local = z * hw + y * W + (side ? W - 1 : 0);
    } else {
        return;
    }
    const int gi = (int)(k * dhw + (unsigned)local);
    if (parent[gi] >= 0) flag[pp::find_root_ro(parent, gi)] = 1;
}

// The filled set: the plane's own voxels and every background voxel whose root no face flagged.
__global__ __launch_bounds__(256) void k_vc_fill_write(const uint8_t *__restrict__ masks, Vals a, unsigned dhw, const int *__restrict__ parent,
                                                       const uint8_t *__restrict__ flag, uint8_t *__restrict__ cur, unsigned long long *counts)
{
    __shared__ int s_n[4];
    __shared__ int s_m[4];
    const unsigned k = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    int c0 = 0, c1 = 0;
    if (i < dhw) {
        const int gi = (int)(k * dhw + i);
        c0 = masks[i] == pick_value(a.v, (int)k);
        c1 = c0;
        if (!c0 && !flag[pp::find_root_ro(parent, gi)]) c1 = 1;     // (a background voxel: parent[gi] >= 0)
        cur[gi] = (uint8_t)c1;
    }
    block_count(c0, counts + 4 * k, s_n);
    block_count(c1, counts + 4 * k + 1, s_m);
}

// ---- dilation, pass z: index distances down and up the column, capped -------------------------------------------------------------------
// One lane per (y, x) column of one plane, consecutive lanes along x.  A seed is a voxel of the set (inv == 0) or of its complement
// (inv == 1: the erosion).  g = the index distance to the nearest seed of the column when that is at most ez, else ez + 1.
__global__ __launch_bounds__(256) void k_vc_z(const uint8_t *__restrict__ cur, int inv, int D, unsigned hw, int ez, uint16_t *__restrict__ g)
{
    const unsigned k = blockIdx.y, c = blockIdx.x * 256u + threadIdx.x;
    if (c >= hw) return;
    const size_t base = (size_t)k * D * hw + c;
    const unsigned cap = (unsigned)ez + 1u;
    unsigned d = cap;
#pragma unroll 2
    for (int z = 0; z < D; ++z) {
        const bool seed = (cur[base + (size_t)z * hw] != 0) != (inv != 0);
        d = seed ? 0u : min(d + 1u, cap);
        g[base + (size_t)z * hw] = (uint16_t)d;
    }
    d = cap;
#pragma unroll 2
    for (int z = D - 1; z >= 0; --z) {
        const unsigned gv = g[base + (size_t)z * hw];
        d = gv == 0 ? 0u : min(d + 1u, cap);
        if (d < gv) g[base + (size_t)z * hw] = (uint16_t)d;
    }
}

// ---- dilation, pass y: f = min over |dy| <= ey of (g uz)^2 + (dy uy)^2, saturated at r^2 + 1 ----------------------------------------------
// A g of ez + 1 stands for no seed within reach and contributes nothing.  g uz <= ez uz <= r and dy uy <= r, so every term is at most
// r^2 < 2^31 and a sum of two fits 32 unsigned bits.  The scan outward from y ends at the half-width, or sooner once (dy uy)^2 alone
// reaches the best so far.
__global__ __launch_bounds__(256) void k_vc_y(const uint16_t *__restrict__ g, unsigned dhw, int H, int W, Ball b, unsigned *__restrict__ f)
{
    const unsigned k = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= dhw) return;
    const int y = (int)((i / (unsigned)W) % (unsigned)H);
    const uint16_t *const gp = g + (size_t)k * dhw + i;
    const unsigned sat = b.r2 + 1u;
    const unsigned g0 = gp[0];
    unsigned best = g0 > (unsigned)b.ez ? sat : (g0 * b.uz) * (g0 * b.uz);
    for (int dy = 1; dy <= b.ey; ++dy) {
        const unsigned t = (unsigned)(dy * b.uy) * (unsigned)(dy * b.uy);
        if (t >= best) break;
        if (y - dy >= 0) {
            const unsigned gl = gp[-(long long)dy * W];
            if (gl <= (unsigned)b.ez) best = min(best, t + (gl * b.uz) * (gl * b.uz));
        }
        if (y + dy < H) {
            const unsigned gr = gp[(long long)dy * W];
            if (gr <= (unsigned)b.ez) best = min(best, t + (gr * b.uz) * (gr * b.uz));
        }
    }
    f[(size_t)k * dhw + i] = min(best, sat);
}

// ---- dilation, pass x: min over |dx| <= ex of f + (dx ux)^2, compared with r^2 -------------------------------------------------------------
// f <= r^2 + 1 and (dx ux)^2 <= r^2: the sum fits 32 unsigned bits.  The scan ends at the half-width, or as soon as the voxel is
// within reach.  The result is written complemented for an erosion; with `count` the voxels of the new set are counted, reduced in the
// wave, then in LDS, one atomic per workgroup.
__global__ __launch_bounds__(256) void k_vc_x(const unsigned *__restrict__ f, int inv, unsigned dhw, int W, Ball b, uint8_t *__restrict__ cur,
                                              unsigned long long *count)
{
    __shared__ int s_n[4];
    const unsigned k = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    int c = 0;
    if (i < dhw) {
        const int x = (int)(i % (unsigned)W);
        const unsigned *const fp = f + (size_t)k * dhw + i;
        unsigned best = fp[0];
        for (int dx = 1; dx <= b.ex && best > b.r2; ++dx) {
            const unsigned t = (unsigned)(dx * b.ux) * (unsigned)(dx * b.ux);
            if (x - dx >= 0) best = min(best, t + fp[-dx]);
            if (x + dx < W) best = min(best, t + fp[dx]);
        }
        c = (best <= b.r2) != (inv != 0);
        cur[(size_t)k * dhw + i] = (uint8_t)c;
    }
    if (count) block_count(c, count + 4 * k, s_n);              // (workgroup-uniform)
}

// ---- emit: 0 / 1 -> 0 / the plane's value ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vc_emit(const uint8_t *__restrict__ cur, Vals a, unsigned dhw, uint8_t *__restrict__ out)
{
    const unsigned k = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= dhw) return;
    out[(size_t)k * dhw + i] = cur[(size_t)k * dhw + i] ? (uint8_t)pick_value(a.v, (int)k) : (uint8_t)0;
}

// One ball of a call: the half-widths cut to the sides they run along.  A radius below every unit is the single voxel: no morphology.
inline Ball make_ball(const VolumeCleanArgs &a, int r)
{
    Ball b;
    b.ux = a.ux; b.uy = a.uy; b.uz = a.uz; b.r2 = (unsigned)r * (unsigned)r;
    b.ex = r / a.ux < a.W - 1 ? r / a.ux : a.W - 1;
    b.ey = r / a.uy < a.H - 1 ? r / a.uy : a.H - 1;
    b.ez = r / a.uz < a.D - 1 ? r / a.uz : a.D - 1;
    return b;
}
inline bool single_voxel(const VolumeCleanArgs &a, int r) { return r / a.ux == 0 && r / a.uy == 0 && r / a.uz == 0; }

// one dilation (inv == 0) or erosion (inv == 1) of every plane by the ball b, in place in w.cur: the three passes
struct Morph {
    Ws w;
    const VolumeCleanArgs &a;
    hipStream_t s;
    void run(const Ball &b, int inv, unsigned long long *count) const
    {
        const unsigned hw = (unsigned)a.H * (unsigned)a.W, dhw = (unsigned)a.D * hw;
        const dim3 blk(256), gv((dhw + 255u) / 256u, (unsigned)a.n), gc((hw + 255u) / 256u, (unsigned)a.n);
        hipLaunchKernelGGL(k_vc_z, gc, blk, 0, s, w.cur, inv, a.D, hw, b.ez, w.g);
        hipLaunchKernelGGL(k_vc_y, gv, blk, 0, s, w.g, dhw, a.H, a.W, b, w.f);
        hipLaunchKernelGGL(k_vc_x, gv, blk, 0, s, w.f, inv, dhw, a.W, b, w.cur, count);
    }
};

}  // namespace vc

size_t volume_clean_workspace_bytes(int D, int H, int W, int n) { return vc::carve(nullptr, (size_t)D * H * W * n).total; }

hipError_t launch_volume_clean(const uint8_t *masks, const VolumeCleanArgs &a, uint8_t *out, unsigned long long *counts, void *ws, hipStream_t s)
{
    const int D = a.D, H = a.H, W = a.W, n = a.n;
    if (!masks || !out || !counts || !ws || D < 1 || H < 1 || W < 1 || n < 1 || n > VOLUME_MAX_VALUES) return hipErrorInvalidValue;
    const unsigned long long dhw64 = (unsigned long long)D * H * W, N64 = dhw64 * n;
    if ((unsigned long long)D * H > 0x7FFFFFFFull || N64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    for (int u : { a.ux, a.uy, a.uz })
        if (u < 1 || u > VOLUME_CLEAN_MAX_R) return hipErrorInvalidValue;
    if (a.close_r < 0 || a.close_r > VOLUME_CLEAN_MAX_R || a.open_r < 0 || a.open_r > VOLUME_CLEAN_MAX_R) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)dhw64, hw = (unsigned)H * (unsigned)W;
    const size_t N = (size_t)N64;
    const vc::Ws w = vc::carve(ws, N);
    vc::Vals vals;
    for (int k = 0; k < VOLUME_MAX_VALUES; ++k) vals.v[k] = a.v[k];
    if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * 4 * sizeof(unsigned long long), s)) return e;
    const dim3 blk(256), gv((dhw + 255u) / 256u, (unsigned)n);
    if (a.fill) {
        int *const parent = reinterpret_cast<int *>(w.f);
        uint8_t *const flag = reinterpret_cast<uint8_t *>(w.g);
        if (hipError_t e = hipMemsetAsync(flag, 0, N, s)) return e;
        hipLaunchKernelGGL(vc::k_vc_bg_init, gv, blk, 0, s, masks, vals, dhw, W, parent);
        hipLaunchKernelGGL(vc::k_vc_bg_merge, gv, blk, 0, s, masks, vals, dhw, H, W, parent);
        const unsigned long long faces = 2ull * ((unsigned long long)hw + (unsigned long long)D * W + (unsigned long long)D * H);
        hipLaunchKernelGGL(vc::k_vc_faces, dim3((unsigned)((faces + 255ull) / 256ull), (unsigned)n), blk, 0, s, parent, dhw, D, H, W, flag);
        hipLaunchKernelGGL(vc::k_vc_fill_write, gv, blk, 0, s, masks, vals, dhw, parent, flag, w.cur, counts);
    } else {
        hipLaunchKernelGGL(vc::k_vc_set, gv, blk, 0, s, masks, vals, dhw, w.cur, counts);
    }
    const vc::Morph m{ w, a, s };
    auto morph = [&](const vc::Ball &b, int inv, unsigned long long *count) { m.run(b, inv, count); };
    auto ball = [&](int r) { return vc::make_ball(a, r); };
    auto single = [&](int r) { return vc::single_voxel(a, r); };
    if (!single(a.close_r)) {
        const vc::Ball b = ball(a.close_r);
        morph(b, 0, nullptr);
        morph(b, 1, counts + 2);
    }
    if (!single(a.open_r)) {
        const vc::Ball b = ball(a.open_r);
        morph(b, 1, nullptr);
        morph(b, 0, counts + 3);
    }
    hipLaunchKernelGGL(vc::k_vc_emit, gv, blk, 0, s, w.cur, vals, dhw, out);
    return hipGetLastError();
}

// The erosion alone, for mi_unet_volume_split's cores: cores [n][D][H][W] = 0 / 1, the erosion of every plane's set by B(a.open_r);
// counts[4 k] = the plane's voxels, counts[4 k + 3] = its core voxels (a single-voxel ball: the cores are the set and only
// counts[4 k] is written).  a.fill and a.close_r are not looked at.  The same workspace as launch_volume_clean.
hipError_t launch_volume_erode(const uint8_t *masks, const VolumeCleanArgs &a, uint8_t *cores, unsigned long long *counts, void *ws, hipStream_t s)
{
    const int D = a.D, H = a.H, W = a.W, n = a.n;
    if (!masks || !cores || !counts || !ws || D < 1 || H < 1 || W < 1 || n < 1 || n > VOLUME_MAX_VALUES) return hipErrorInvalidValue;
    const unsigned long long dhw64 = (unsigned long long)D * H * W, N64 = dhw64 * n;
    if ((unsigned long long)D * H > 0x7FFFFFFFull || N64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    for (int u : { a.ux, a.uy, a.uz })
        if (u < 1 || u > VOLUME_CLEAN_MAX_R) return hipErrorInvalidValue;
    if (a.open_r < 0 || a.open_r > VOLUME_CLEAN_MAX_R) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)dhw64;
    vc::Ws w = vc::carve(ws, (size_t)N64);
    w.cur = cores;                                              // the passes work in place in the caller's array
    vc::Vals vals;
    for (int k = 0; k < VOLUME_MAX_VALUES; ++k) vals.v[k] = a.v[k];
    if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * 4 * sizeof(unsigned long long), s)) return e;
    hipLaunchKernelGGL(vc::k_vc_set, dim3((dhw + 255u) / 256u, (unsigned)n), dim3(256), 0, s, masks, vals, dhw, w.cur, counts);
    if (!vc::single_voxel(a, a.open_r)) vc::Morph{ w, a, s }.run(vc::make_ball(a, a.open_r), 1, counts + 3);
    return hipGetLastError();
}

}  // namespace miunet
