// volume_skeleton.hip -- the components of an id stack thinned to medial lines without a change of topology, and the lines counted
// (include/mi_unet.h: mi_unet_volume_skeleton).  A pass marks the end points, then runs six directional phases of
// eight subfield sub-steps; a sub-step deletes, at once, the candidates of its subfield that are simple points of the current state.
// The simple-point test is evaluated in registers: the 26 same-object bits laid out as a 3 x 3 x 3 word, both floods as shifts under
// constant masks.  Candidates are compacted once per phase into one list per subfield (wave.h's ballots and shared cursors), so a
// sub-step touches the surface voxels of one subfield and nothing else.  The sweeps that look at every voxel's 26 neighbours (end
// points, final statistics) walk key_tile.h's tile with its halo in LDS.  Exact integers; the result does not depend on the order in
// which lanes, waves or workgroups run.  gfx950 only.
#include <algorithm>

#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "key_tile.h"
#include "wave.h"

namespace miunet {

namespace vsk {

using namespace wave;
using key_tile::KX;
using key_tile::KY;
using key_tile::ROWS;
using key_tile::TX;
using key_tile::TY;
using key_tile::TZ;
using key_tile::walk_tile;

constexpr int WG = 256;
constexpr int KZ = TZ + 2;                               // a tile with one voxel of halo on every side: 66 x 10 x 6 keys, 15.5 KiB
constexpr int TILE_KEYS = KX * KY * KZ;
constexpr unsigned MAX_GRID = 4096;                      // workgroups of a grid-stride launch

struct Ws {
    int32_t *dist;                  // [dhw] the squared distance to another id (behind begin); dist_z's output on the way
    int32_t *list;                  // [8][cap8] the candidates of a phase by subfield; dist_y's output on the way
    uint8_t *endm;                  // [dhw] 1 = marked an end point at the pass's start
    size_t cap8, total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline Ws carve(void *base, int D, int H, int W)
{
    Ws w;
    const size_t dhw = (size_t)D * H * W;
    w.cap8 = (size_t)((D + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2);      // no subfield holds more voxels; 8 cap8 >= dhw
    uint8_t *p = static_cast<uint8_t *>(base);
    size_t at = 0;
    w.dist = reinterpret_cast<int32_t *>(p + at); at += up256(dhw * sizeof(int32_t));
    w.list = reinterpret_cast<int32_t *>(p + at); at += up256(8 * w.cap8 * sizeof(int32_t));
    w.endm = p + at; at += up256(dhw);
    w.total = at;
    return w;
}

inline unsigned blocks(size_t n) { return (unsigned)std::min<size_t>((n + WG - 1) / WG, MAX_GRID); }

// ---- the simple-point test -----------------------------------------------------------------------------------------------------------------
// The 26-bit code (bit i = the i-th offset of the raster order without the centre) becomes a 27-bit word with bit
// j = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) and the centre, bit 13, clear.  A step along x is a shift by 1 that must not leave its row of
// three, along y a shift by 3 inside a slice of nine, along z a shift by 9.
constexpr uint32_t M27 = 0x7FFFFFFu;
constexpr uint32_t X_LO = 0x1249249u, X_HI = X_LO << 2;          // dx = -1, dx = +1
constexpr uint32_t Y_LO = 0x01C0E07u, Y_HI = Y_LO << 6;          // dy = -1, dy = +1
constexpr uint32_t CORNERS = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26);
constexpr uint32_t N18 = M27 & ~CORNERS & ~(1u << 13);
constexpr uint32_t FACES = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);

__device__ __forceinline__ uint32_t step_x(uint32_t v) { return ((v & ~X_HI) << 1) | ((v & ~X_LO) >> 1); }
__device__ __forceinline__ uint32_t step_y(uint32_t v) { return ((v & ~Y_HI) << 3) | ((v & ~Y_LO) >> 3); }
__device__ __forceinline__ uint32_t step_z(uint32_t v) { return ((v << 9) & M27) | (v >> 9); }

__device__ __forceinline__ bool simple_point(uint32_t code)
{
    const uint32_t obj = (code & 0x1FFFu) | ((code >> 13) << 14);
    if (!obj) return false;
    // the object: one 26-component?  A 26-step is an x, a y and a z step of at most one each.
    uint32_t seen = obj & (0u - obj);
    for (int it = 0; it < 26; ++it) {                           // (a flood that grows adds a bit: 26 rounds bound it)
        uint32_t g = seen | step_x(seen);
        g |= step_y(g);
        g |= step_z(g);
        g &= obj;
        if (g == seen) break;
        seen = g;
    }
    if (seen != obj) return false;
    // the background inside the 18 neighbours: one 6-component that holds every background face neighbour, and at least one of those
    const uint32_t bg = ~obj & N18, faces = bg & FACES;
    if (!faces) return false;
    seen = faces & (0u - faces);
    for (int it = 0; it < 18; ++it) {
        const uint32_t g = (seen | step_x(seen) | step_y(seen) | step_z(seen)) & bg;
        if (g == seen) break;
        seen = g;
    }
    return (faces & ~seen) == 0u;
}

__global__ __launch_bounds__(WG) void k_vsk_simple(uint32_t first_word, uint32_t n_words, uint32_t *__restrict__ bits)
{
    for (uint32_t w = blockIdx.x * WG + threadIdx.x; w < n_words; w += gridDim.x * WG) {
        const uint32_t base = (first_word + w) << 5;
        uint32_t r = 0;
        for (int b = 0; b < 32; ++b) r |= (uint32_t)simple_point(base + b) << b;
        bits[w] = r;
    }
}

// ---- begin: the ids normalised, the table cleared, the input counted ---------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_vsk_clear(mi_unet_vskel *table, int m)
{
    const int r = blockIdx.x * WG + threadIdx.x;
    if (r >= m) return;
    mi_unet_vskel t{};
    t.r2_min = 0x7FFFFFFF;                                      // (k_vsk_table puts 0 where nothing lowered it)
    table[r] = t;
}

__global__ __launch_bounds__(WG) void k_vsk_init(int32_t *__restrict__ cur, unsigned dhw, int m, mi_unet_vskel *table)
{
    const unsigned n_up = (dhw + 63u) & ~63u;                   // (whole waves: the ballots below are wave-uniform)
    for (unsigned i = blockIdx.x * WG + threadIdx.x; i < n_up; i += gridDim.x * WG) {
        int v = 0;
        if (i < dhw) {
            v = cur[i];
            if (v < 1 || v > m) v = 0;
            cur[i] = v;
        }
        peel<64>(v, 0, [&](int k0, bool, u64 mask, int leader) {
            if ((int)(threadIdx.x & 63) == leader)
                atomicAdd(reinterpret_cast<u64 *>(&table[k0 - 1].voxels_in), (u64)__popcll(mask));
        });
    }
}

// ---- the squared distance to the nearest voxel of another id -------------------------------------------------------------------------------------
// Separable although the labels are many: for a voxel p of id L the column term of a voxel p' in p's slice row is 0 where p' carries another
// id and otherwise the column's distance from p' to another id than ITS OWN, which is L.  So each pass looks along its axis while the id
// stays L and stops at the first voxel of another id (anything behind it costs more), or at the layer of "nothing" outside the volume.
__global__ __launch_bounds__(WG) void k_vsk_dist_z(const int32_t *__restrict__ cur, int D, unsigned hw, int uz, int32_t *__restrict__ gz)
{
    const unsigned c = blockIdx.x * WG + threadIdx.x;
    if (c >= hw) return;
    int prev = -1, run = 0;
    for (int z = 0; z < D; ++z) {                               // the index distance back to another id (the layer at -1: z + 1)
        const int v = cur[(size_t)z * hw + c];
        run = v == prev ? run + 1 : 1;
        prev = v;
        gz[(size_t)z * hw + c] = run;
    }
    prev = -1;
    for (int z = D - 1; z >= 0; --z) {
        const int v = cur[(size_t)z * hw + c];
        run = v == prev ? run + 1 : 1;
        prev = v;
        const int g = min(run, gz[(size_t)z * hw + c]) * uz;    // (at most D uz <= 46340)
        gz[(size_t)z * hw + c] = g * g;
    }
}

// along an axis of `n` voxels `stride` apart, from position `at` of the line that starts at `line`: in[] holds the term of the passes before
__device__ __forceinline__ int dist_scan(const int32_t *__restrict__ cur, const int32_t *__restrict__ in, size_t line, size_t stride, int at,
                                         int n, int u)
{
    const int L = cur[line + at * stride];
    int best = in[line + at * stride];
#pragma unroll
    for (int dir = -1; dir <= 1; dir += 2)
        for (int d = 1;; ++d) {
            const int step = d * u * d * u;                     // (d <= n, so d u <= 46340)
            if (step >= best) break;
            const int q = at + dir * d;
            if (q < 0 || q >= n || cur[line + q * stride] != L) { best = step; break; }
            best = min(best, step + in[line + q * stride]);
        }
    return best;
}

__global__ __launch_bounds__(WG) void k_vsk_dist_y(const int32_t *__restrict__ cur, unsigned dhw, int H, int W, int uy, const int32_t *__restrict__ gz,
                                                   int32_t *__restrict__ f)
{
    for (unsigned i = blockIdx.x * WG + threadIdx.x; i < dhw; i += gridDim.x * WG) {
        if (!cur[i]) continue;
        const unsigned x = i % (unsigned)W, zy = i / (unsigned)W, y = zy % (unsigned)H, z = zy / (unsigned)H;
        f[i] = dist_scan(cur, gz, (size_t)z * H * W + x, (size_t)W, (int)y, H, uy);
    }
}

__global__ __launch_bounds__(WG) void k_vsk_dist_x(const int32_t *__restrict__ cur, unsigned dhw, int W, int ux, const int32_t *__restrict__ f,
                                                   int32_t *__restrict__ dist)
{
    for (unsigned i = blockIdx.x * WG + threadIdx.x; i < dhw; i += gridDim.x * WG) {
        if (!cur[i]) continue;
        const unsigned x = i % (unsigned)W;
        dist[i] = dist_scan(cur, f, (size_t)(i - x), (size_t)1, (int)x, W, ux);
    }
}

__global__ __launch_bounds__(WG) void k_vsk_ends(const int32_t *__restrict__ cur, int D, int H, int W, int tiles_x, int tiles_y, int n_tiles,
                                                 uint8_t *__restrict__ endm)
{
    __shared__ int s_keys[TILE_KEYS];
    const int t_end = min(n_tiles, ((int)blockIdx.x + 1) * VTX_TILES_PER_WG);
    for (int tile = (int)blockIdx.x * VTX_TILES_PER_WG; tile < t_end; ++tile) {
        __syncthreads();                                        // the tile before is done with s_keys
        const int3 o = key_tile::tile_origin<1>(tile, tiles_x, tiles_y);
        key_tile::load_key_tile<KZ, 1>(s_keys, cur, o, D, H, W);
        __syncthreads();
        walk_tile(s_keys, o, D, H, W, [&](size_t i, bool, int v, uint32_t code) {
            if (v) endm[i] = __popc(code) == 1;                 // (read only where cur holds an id)
        });
    }
}

// ---- a phase: its candidates, by subfield ---------------------------------------------------------------------------------------------------------
// dir 0 .. 5 = z - 1, z + 1, y - 1, y + 1, x - 1, x + 1.  The order inside a list depends on the run; what a sub-step does with it does not.
__global__ __launch_bounds__(WG) void k_vsk_candidates(const int32_t *__restrict__ cur, const uint8_t *__restrict__ endm, unsigned dhw, int D, int H,
                                                       int W, int dir, size_t cap8, int32_t *__restrict__ list, unsigned *count)
{
    const unsigned n_up = (dhw + 63u) & ~63u;
    for (unsigned i = blockIdx.x * WG + threadIdx.x; i < n_up; i += gridDim.x * WG) {
        int sub = -1;
        const int v = i < dhw ? cur[i] : 0;
        if (v && !endm[i]) {
            const int x = (int)(i % (unsigned)W), zy = (int)(i / (unsigned)W), y = zy % H, z = zy / H;
            const int axis = dir >> 1, sgn = (dir & 1) ? 1 : -1;
            const int q = (axis == 0 ? z : axis == 1 ? y : x) + sgn, n = axis == 0 ? D : axis == 1 ? H : W;
            const long long off = (long long)sgn * (axis == 0 ? (long long)H * W : axis == 1 ? W : 1);
            const bool same = q >= 0 && q < n && cur[(long long)i + off] == v;
            if (!same) sub = (x & 1) | (y & 1) << 1 | (z & 1) << 2;
        }
        peel<64>(sub, -1, [&](int k0, bool mine, u64 mask, int leader) {
            const unsigned pos = wave_take(count + k0, mask, leader);
            if (mine) list[(size_t)k0 * cap8 + pos] = (int32_t)i;      // (pos < cap8: a subfield has no more voxels)
        });
    }
}

// ---- a sub-step: the candidates of one subfield that are simple go, all at once ---------------------------------------------------------------------
// No read here can race a write: a lane writes its own voxel only, every other lane's voxel is of the same subfield, so it differs by
// an even amount on every axis and lies outside this lane's 3 x 3 x 3 neighbourhood.  What the lane reads was written by an earlier launch.
__global__ __launch_bounds__(WG) void k_vsk_substep(int32_t *cur, int D, int H, int W, const int32_t *__restrict__ list, const unsigned *__restrict__ count,
                                                    unsigned *deleted)
{
    const unsigned n = *count, n_up = (n + 63u) & ~63u;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n_up; j += gridDim.x * WG) {
        bool del = false;
        if (j < n) {
            const unsigned i = (unsigned)list[j];
            const int x = (int)(i % (unsigned)W), zy = (int)(i / (unsigned)W), y = zy % H, z = zy / H;
            const int v = cur[i];
            uint32_t code = 0;
            int bit = 0;
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!dz && !dy && !dx) continue;
                        const int zz = z + dz, yy = y + dy, xx = x + dx;
                        if (zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W)
                            code |= (uint32_t)(cur[((size_t)zz * H + yy) * W + xx] == v) << bit;
                        ++bit;
                    }
            del = simple_point(code);
            if (del) cur[i] = 0;
        }
        const u64 mask = __ballot(del);
        if (mask && (threadIdx.x & 63) == 0) atomicAdd(deleted, (unsigned)__popcll(mask));
    }
}

// ---- the skeleton counted -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void add64(int64_t *p, u64 v)
{
    if (v) atomicAdd(reinterpret_cast<u64 *>(p), v);
}

__global__ __launch_bounds__(WG) void k_vsk_stats(const int32_t *__restrict__ cur, int D, int H, int W, int tiles_x, int tiles_y, int n_tiles,
                                                  const int32_t *__restrict__ dist, int want_radius, int32_t *__restrict__ r2, mi_unet_vskel *table)
{
    __shared__ int s_keys[TILE_KEYS];
    const int t_end = min(n_tiles, ((int)blockIdx.x + 1) * VTX_TILES_PER_WG);
    for (int tile = (int)blockIdx.x * VTX_TILES_PER_WG; tile < t_end; ++tile) {
        __syncthreads();
        const int3 o = key_tile::tile_origin<1>(tile, tiles_x, tiles_y);
        key_tile::load_key_tile<KZ, 1>(s_keys, cur, o, D, H, W);
        __syncthreads();
        walk_tile(s_keys, o, D, H, W, [&](size_t i, bool inside, int v, uint32_t code) {
            const int d = v && dist ? dist[i] : 0;
            if (r2 && inside) r2[i] = d;
            if (!__ballot(v != 0)) return;                      // (wave-uniform) no skeleton voxel in the row
            // a pair is counted from its voxel of the lower index: the 13 offsets behind the centre, bits 13 .. 25, in raster order
            const int nb = __popc(code);
            // six 10-bit fields a word (a wave adds at most 64 to each): voxels ends isolated junctions l0 l1 | l2 l3 l4 l5 l6
            u64 a = 0, b = 0;
            if (v) {
                a = 1ull | (u64)(nb == 1) << 10 | (u64)(nb == 0) << 20 | (u64)(nb >= 3) << 30;
                int bit = 13;
#pragma unroll
                for (int dz = 0; dz <= 1; ++dz)
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (dz == 0 && (dy < 0 || (dy == 0 && dx <= 0))) continue;
                            const int c = (dx != 0) + 2 * (dy != 0) + 4 * (dz != 0) - 1;
                            const u64 on = (code >> bit) & 1u;
                            if (c < 2) a += on << (40 + 10 * c);
                            else b += on << (10 * (c - 2));
                            ++bit;
                        }
            }
            int key = v;
            peel<64>(key, 0, [&](int k0, bool mine, u64, int leader) {
                const u64 sa = wave_sum(mine ? a : 0ull), sb = wave_sum(mine ? b : 0ull);
                u64 sd = 0;
                int dmin = 0x7FFFFFFF, dmax = 0;
                if (want_radius) {
                    sd = wave_sum(mine ? (u64)d : 0ull);
                    dmin = wave_min(mine ? d : 0x7FFFFFFF);
                    dmax = wave_max(mine ? d : 0);
                }
                if ((int)(threadIdx.x & 63) != leader) return;
                mi_unet_vskel *const t = table + (k0 - 1);
                add64(&t->voxels, sa & 1023u);
                add64(&t->ends, (sa >> 10) & 1023u);
                add64(&t->isolated, (sa >> 20) & 1023u);
                add64(&t->junctions, (sa >> 30) & 1023u);
                add64(&t->links[0], (sa >> 40) & 1023u);
                add64(&t->links[1], (sa >> 50) & 1023u);
#pragma unroll
                for (int c = 2; c < 7; ++c) add64(&t->links[c], (sb >> (10 * (c - 2))) & 1023u);
                if (want_radius) {
                    add64(&t->r2_sum, sd);
                    lower(&t->r2_min, dmin);
                    raise(&t->r2_max, dmax);
                }
            });
        });
    }
}

__global__ __launch_bounds__(WG) void k_vsk_table(mi_unet_vskel *table, int m, int want_radius)
{
    const int r = blockIdx.x * WG + threadIdx.x;
    if (r >= m) return;
    if (!want_radius || table[r].voxels == 0) table[r].r2_min = 0;
}

inline bool fits(const VolumeSkeletonArgs &a)
{
    return a.D >= 1 && a.H >= 1 && a.W >= 1 && a.D <= SCORE_VOLUME_MAX_SIDE && a.H <= SCORE_VOLUME_MAX_SIDE && a.W <= SCORE_VOLUME_MAX_SIDE &&
           (long long)a.D * a.H * a.W < (1ll << 31) && a.m >= 1 && a.m <= VOLUME_MAX_TABLE && a.ux >= 1 && a.uy >= 1 && a.uz >= 1;
}

struct Tiles { int tx, ty, n; unsigned grid; };
inline Tiles tiles_of(const VolumeSkeletonArgs &a)
{
    Tiles t;
    t.tx = (a.W + TX - 1) / TX; t.ty = (a.H + TY - 1) / TY;
    t.n = t.tx * t.ty * ((a.D + TZ - 1) / TZ);                  // (at most 2^21: a side is at most 8192 and the volume 2^31)
    t.grid = (unsigned)((t.n + VTX_TILES_PER_WG - 1) / VTX_TILES_PER_WG);
    return t;
}

}  // namespace vsk

size_t volume_skeleton_workspace_bytes(int D, int H, int W) { return vsk::carve(nullptr, D, H, W).total; }

hipError_t launch_volume_skeleton_begin(int32_t *cur, const VolumeSkeletonArgs &a, bool want_dist, mi_unet_vskel *table, void *ws, hipStream_t s)
{
    if (!cur || !table || !ws || !vsk::fits(a)) return hipErrorInvalidValue;
    const vsk::Ws w = vsk::carve(ws, a.D, a.H, a.W);
    const unsigned hw = (unsigned)a.H * (unsigned)a.W, dhw = (unsigned)a.D * hw;
    hipLaunchKernelGGL(vsk::k_vsk_clear, dim3((a.m + vsk::WG - 1) / vsk::WG), dim3(vsk::WG), 0, s, table, a.m);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vsk::k_vsk_init, dim3(vsk::blocks(dhw)), dim3(vsk::WG), 0, s, cur, dhw, a.m, table);
    if (hipError_t e = hipGetLastError()) return e;
    if (!want_dist) return hipSuccess;
    hipLaunchKernelGGL(vsk::k_vsk_dist_z, dim3((hw + vsk::WG - 1) / vsk::WG), dim3(vsk::WG), 0, s, (const int32_t *)cur, a.D, hw, a.uz, w.dist);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vsk::k_vsk_dist_y, dim3(vsk::blocks(dhw)), dim3(vsk::WG), 0, s, (const int32_t *)cur, dhw, a.H, a.W, a.uy,
                       (const int32_t *)w.dist, w.list);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vsk::k_vsk_dist_x, dim3(vsk::blocks(dhw)), dim3(vsk::WG), 0, s, (const int32_t *)cur, dhw, a.W, a.ux, (const int32_t *)w.list,
                       w.dist);
    return hipGetLastError();
}

hipError_t launch_volume_skeleton_pass(int32_t *cur, const VolumeSkeletonArgs &a, void *ws, VskPass *pass_state, hipStream_t s)
{
    if (!cur || !ws || !pass_state || !vsk::fits(a)) return hipErrorInvalidValue;
    const vsk::Ws w = vsk::carve(ws, a.D, a.H, a.W);
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    const vsk::Tiles t = vsk::tiles_of(a);
    if (hipError_t e = hipMemsetAsync(pass_state, 0, sizeof(VskPass), s)) return e;
    hipLaunchKernelGGL(vsk::k_vsk_ends, dim3(t.grid), dim3(vsk::WG), 0, s, (const int32_t *)cur, a.D, a.H, a.W, t.tx, t.ty, t.n, w.endm);
    if (hipError_t e = hipGetLastError()) return e;
    const unsigned sub_grid = vsk::blocks(w.cap8);
    for (int dir = 0; dir < 6; ++dir) {
        hipLaunchKernelGGL(vsk::k_vsk_candidates, dim3(vsk::blocks(dhw)), dim3(vsk::WG), 0, s, (const int32_t *)cur, (const uint8_t *)w.endm, dhw, a.D,
                           a.H, a.W, dir, w.cap8, w.list, pass_state->count[dir]);
        if (hipError_t e = hipGetLastError()) return e;
        for (int sub = 0; sub < 8; ++sub) {
            hipLaunchKernelGGL(vsk::k_vsk_substep, dim3(sub_grid), dim3(vsk::WG), 0, s, cur, a.D, a.H, a.W, (const int32_t *)(w.list + sub * w.cap8),
                               (const unsigned *)&pass_state->count[dir][sub], &pass_state->deleted);
            if (hipError_t e = hipGetLastError()) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_volume_skeleton_finish(const int32_t *cur, const VolumeSkeletonArgs &a, bool want_dist, bool want_radius, int32_t *r2,
                                         mi_unet_vskel *table, void *ws, hipStream_t s)
{
    if (!cur || !table || !ws || !vsk::fits(a) || ((r2 || want_radius) && !want_dist)) return hipErrorInvalidValue;
    const vsk::Ws w = vsk::carve(ws, a.D, a.H, a.W);
    const vsk::Tiles t = vsk::tiles_of(a);
    hipLaunchKernelGGL(vsk::k_vsk_stats, dim3(t.grid), dim3(vsk::WG), 0, s, cur, a.D, a.H, a.W, t.tx, t.ty, t.n,
                       want_dist ? (const int32_t *)w.dist : nullptr, (int)want_radius, r2, table);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(vsk::k_vsk_table, dim3((a.m + vsk::WG - 1) / vsk::WG), dim3(vsk::WG), 0, s, table, a.m, (int)want_radius);
    return hipGetLastError();
}

hipError_t launch_volume_skeleton_simple(uint32_t first_word, uint32_t n_words, uint32_t *bits, hipStream_t s)
{
    if (!bits || n_words < 1 || (unsigned long long)first_word + n_words > (1ull << 21)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vsk::k_vsk_simple, dim3(vsk::blocks(n_words)), dim3(vsk::WG), 0, s, first_word, n_words, bits);
    return hipGetLastError();
}

}  // namespace miunet
