// volume_split.hip -- touching objects split into pieces, per value plane: the plane eroded to cores (volume_clean.hip's erosion), the
// cores labelled (cc_common.h's lock-free union-find), and the cores grown back inside the plane by geodesic distance: every voxel
// takes the smallest (length, marker) any kept core reaches it with (include/mi_unet.h: mi_unet_volume_split).  The
// growth is the hot path: tiles of key_tile.h's geometry relaxed in LDS, round after round, only where something changed.  The pieces
// then go through volume.hip's chain -- a slot per piece, sums, keys, exact select, table, ids -- with "same piece" where that chain
// asks "in the set".  Exact integers; the result does not depend on the order in which workgroups run.  gfx950 only.
#include "../../include/mi_unet.h"
#include "cc_common.h"
#include "kernel_common.h"
#include "key_tile.h"
#include "wave.h"

namespace miunet {

namespace vs {

using namespace wave;
using key_tile::TX;
using key_tile::TY;
using key_tile::TZ;

constexpr int NO_SLOT = -1;
constexpr int RUN = 16;                                  // 64-voxel segments a wave of k_vs_stats carries a piece over (volume.hip's RUN)
constexpr u64 UNREACHED = ~0ull;                         // the key of a voxel no kept core has reached (and of every voxel outside S)
constexpr int KX = TX + 2, KY = TY + 2, KZ = TZ + 2;     // a tile with one voxel of halo on every side: 66 x 10 x 6 keys, 31 KiB

// what a plane counts besides volume.hip's accumulators
struct PlaneCount { unsigned long long cores, cores_kept, coreless, max_reach; };

struct Ws {
    VolumeRankAcc *acc;             // [n] volume.hip's accumulators of a plane: the slot cursor, the table's threshold
    PlaneCount *cnt;                // [n]
    unsigned long long *counts;     // [n][4] launch_volume_erode's: [0] the plane's voxels, [3] its core voxels
    uint8_t *flags[2];              // [n][tiles] each: the tiles that run in an even / an odd round
    uint8_t *sel;                   // [N] 0 / 1: the cores; behind the growth the voxels of S that no core reached
    int *parent;                    // [N] the forest of the cores, then of the rest; at the end the root of every voxel's piece, -1 outside S
    int *csize;                     // [N] valid at the root of a core: its voxels
    int *slot;                      // [N] valid at the root of a piece: the piece's slot in its plane
    u64 *key;                       // [N] (length << 31) | marker, or UNREACHED
    mi_unet_vcomp *stat;            // [n][S] per slot, in the layout of the table
    mi_unet_vpiece *info;           // [n][S]
    u64 *okey;                      // [n][S] the order key: (voxels << 31) | (2^31 - 1 - first)
    int *tidx;                      // [n][S] 1 + the table index of the slot's piece, 0 when it is not in the table
    void *erode;                    // launch_volume_erode's workspace
    size_t total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Grid { int tx, ty, tz, tiles; };                  // the tiles of one plane along x, y, z and their number
inline Grid grid_of(int D, int H, int W)
{
    Grid g;
    g.tx = (W + TX - 1) / TX; g.ty = (H + TY - 1) / TY; g.tz = (D + TZ - 1) / TZ;
    g.tiles = g.tx * g.ty * g.tz;
    return g;
}

inline Ws carve(void *base, int D, int H, int W, int n)
{
    const size_t dhw = (size_t)D * H * W, N = dhw * n, S = volume_slots_per_plane(dhw) * n, T = (size_t)grid_of(D, H, W).tiles * n;
    uint8_t *p = static_cast<uint8_t *>(base);
    Ws w;
    size_t at = 0;
    auto take = [&](size_t bytes) { uint8_t *q = p + at; at += up256(bytes); return q; };
    w.acc = reinterpret_cast<VolumeRankAcc *>(take((size_t)n * sizeof(VolumeRankAcc)));
    w.cnt = reinterpret_cast<PlaneCount *>(take((size_t)n * sizeof(PlaneCount)));
    w.counts = reinterpret_cast<unsigned long long *>(take((size_t)n * 4 * sizeof(unsigned long long)));
    w.flags[0] = take(T);
    w.flags[1] = take(T);
    w.sel = take(N);
    w.parent = reinterpret_cast<int *>(take(N * sizeof(int)));
    w.csize = reinterpret_cast<int *>(take(N * sizeof(int)));
    w.slot = reinterpret_cast<int *>(take(N * sizeof(int)));
    w.key = reinterpret_cast<u64 *>(take(N * sizeof(u64)));
    w.stat = reinterpret_cast<mi_unet_vcomp *>(take(S * sizeof(mi_unet_vcomp)));
    w.info = reinterpret_cast<mi_unet_vpiece *>(take(S * sizeof(mi_unet_vpiece)));
    w.okey = reinterpret_cast<u64 *>(take(S * sizeof(u64)));
    w.tidx = reinterpret_cast<int *>(take(S * sizeof(int)));
    w.erode = take(volume_clean_workspace_bytes(D, H, W, n));
    w.total = at;
    return w;
}

// keys that another workgroup may store in the same launch: relaxed, agent scope, 64 bits at once (cc_common.h does the same for
// parents).  A stale read is harmless, a torn one is not.
__device__ __forceinline__ u64 ld_key(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_key(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the same inside the workgroup's LDS, where the four waves of a sweep read each other's rows
__device__ __forceinline__ u64 ld_lds(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_lds(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

struct Dims { int D, H, W; unsigned dhw; };

// ---- labels: the components of the set sel under the connectivity -----------------------------------------------------------------------
// Voxel i of plane k is i = k * dhw + z * hw + y * W + x.  Every voxel of the set starts as its own root and unites with those of its
// 13 earlier neighbours that the connectivity allows (AXES = 1, 2, 3 for 6, 18, 26) and that are in the set; parents only decrease, so
// a root is its component's raster-first voxel.  Every union is pp::unite; its loop ends by its own data.
__global__ __launch_bounds__(256) void k_vs_init(const uint8_t *__restrict__ sel, int *parent, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < N) parent[i] = sel[i] ? (int)i : -1;
}

template <int AXES>
__global__ __launch_bounds__(256) void k_vs_merge(const uint8_t *__restrict__ sel, Dims d, int *parent, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || !sel[i]) return;
    const unsigned src = i % d.dhw;
    const int W = d.W, H = d.H, hw = H * W;
    const int z = (int)(src / (unsigned)hw), rem = (int)(src - (unsigned)z * (unsigned)hw), y = rem / W, x = rem - y * W;
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int axes = (dz != 0) + (dy != 0) + (dx != 0);
                const bool earlier = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
                if (!earlier || axes > AXES) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                const int j = (int)i + dz * hw + dy * W + dx;
                if (sel[j]) pp::unite(parent, (int)i, j);
            }
}

// ---- core sizes: flatten + one count per core voxel at the core's root, merged per root inside a wave -----------------------------------
__global__ __launch_bounds__(256) void k_vs_core_count(int *parent, int *csize, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    int r = -1;
    if (i < N && parent[i] >= 0) {
        r = pp::find_root_ro(parent, (int)i);
        parent[i] = r;
    }
    const int lane = threadIdx.x & 63;
    peel<64>(r, -1, [&](int r0, bool, u64 mm, int leader) {
        if (lane == leader) atomicAdd(csize + r0, (int)__builtin_popcountll(mm));
    });
}

// ---- seed: the keys before the growth, the tiles of round 0, the plane's cores -----------------------------------------------------------
__global__ __launch_bounds__(256) void k_vs_seed(const uint8_t *__restrict__ sel, const int *__restrict__ parent, const int *__restrict__ csize,
                                                 Dims d, Grid g, int min_core, u64 *key, uint8_t *flags, PlaneCount *cnt, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    u64 q = UNREACHED;
    if (sel[i]) {
        const int r = parent[i];                                // (flattened by k_vs_core_count)
        const unsigned k = i / d.dhw, src = i - k * d.dhw;
        const bool kept = csize[r] >= min_core;
        if (r == (int)i) {
            atomicAdd(&cnt[k].cores, 1ull);
            if (kept) atomicAdd(&cnt[k].cores_kept, 1ull);
        }
        if (kept) {
            q = (u64)((unsigned)r - k * d.dhw);
            const int hw = d.H * d.W;
            const int z = (int)(src / (unsigned)hw), rem = (int)(src - (unsigned)z * (unsigned)hw), y = rem / d.W, x = rem - y * d.W;
            // round 0 runs the voxel's tile and, for a voxel on the tile's border, the tiles that hold one of its 26 neighbours:
            // a core voxel never changes, so no later round would tell them
            const int own = ((z / TZ) * g.ty + y / TY) * g.tx + x / TX;
            flags[(size_t)k * g.tiles + own] = 1;
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int zz = z + dz, yy = y + dy, xx = x + dx;
                        if (zz < 0 || zz >= d.D || yy < 0 || yy >= d.H || xx < 0 || xx >= d.W) continue;
                        const int t = ((zz / TZ) * g.ty + yy / TY) * g.tx + xx / TX;
                        if (t != own) flags[(size_t)k * g.tiles + t] = 1;
                    }
        }
    }
    key[i] = q;
}

// ---- grow: one round of the growth, the hot path ------------------------------------------------------------------------------------------
// A workgroup per tile of every plane; one whose flag is clear ends at once.  The tile's keys and one voxel of halo on every side go
// into LDS (a position outside the volume holds UNREACHED, as every voxel outside S does, so no step needs a test of its own).  A wave
// takes the rows w, w + 4, ... of the tile, a lane one voxel of each: the voxel's key becomes the minimum of itself and key(u) + (the
// step's cost, 0) over its neighbours u under the connectivity.  Each lane writes only its own voxels; the four waves read each
// other's rows while they change, which by 7.21 (a) costs sweeps at most, never the result.  A sweep ends at a barrier that also tells
// whether any lane changed a key; the loop ends when none did.  Then the lanes store the keys they changed and the workgroup flags,
// for the next round, every neighbour tile whose halo holds one of them: face, edge or corner, as far as the connectivity looks.
// The halo was read while its owners may have been storing: whoever stored a boundary voxel flags this tile again, so a stale read is
// made good in the next round.
struct GrowArgs { Dims d; Grid g; int ux, uy, uz; int v[VOLUME_MAX_VALUES]; };

template <int AXES>
__global__ __launch_bounds__(256) void k_vs_grow(const uint8_t *__restrict__ masks, GrowArgs a, u64 *key_all, uint8_t *flags_in,
                                                 uint8_t *flags_out, unsigned *active)
{
    __shared__ u64 s_key[KX * KY * KZ];
    __shared__ unsigned s_mark;
    const unsigned b = blockIdx.x, k = b / (unsigned)a.g.tiles, t = b - k * (unsigned)a.g.tiles;
    if (!flags_in[b]) return;                                   // (workgroup-uniform; cleared below, behind a barrier)
    const int D = a.d.D, H = a.d.H, W = a.d.W;
    const int3 o = key_tile::tile_origin<1>((int)t, a.g.tx, a.g.ty);
    u64 *const key = key_all + (size_t)k * a.d.dhw;
    for (int e = threadIdx.x; e < KX * KY * KZ; e += 256) {
        const int lz = e / (KX * KY), rem = e - lz * (KX * KY), ly = rem / KX, lx = rem - ly * KX;
        const int gx = o.x + lx, gy = o.y + ly, gz = o.z + lz;
        u64 q = UNREACHED;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H && gz >= 0 && gz < D) q = ld_key(key + ((size_t)gz * H + gy) * W + gx);
        s_key[e] = q;
    }
    if (threadIdx.x == 0) s_mark = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        flags_in[b] = 0;
        atomicAdd(active + k, 1u);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int PER = key_tile::ROWS / 4;                     // rows of the tile per wave
    const int value = pick_value(a.v, (int)k);
    u64 mine[PER];
    unsigned in_s = 0, changed = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int row = w + 4 * j, ly = row % TY, lz = row / TY;
        const int gx = o.x + 1 + lane, gy = o.y + 1 + ly, gz = o.z + 1 + lz;
        mine[j] = s_key[((lz + 1) * KY + ly + 1) * KX + lane + 1];
        if (gx < W && gy < H && gz < D && masks[((size_t)gz * H + gy) * W + gx] == value) in_s |= 1u << j;
    }
    const u64 cx = (u64)a.ux << 31, cy = (u64)a.uy << 31, cz = (u64)a.uz << 31;
    for (;;) {
        int moved = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (!((in_s >> j) & 1u)) continue;
            const int row = w + 4 * j, ly = row % TY, lz = row / TY;
            u64 *const c = s_key + ((lz + 1) * KY + ly + 1) * KX + lane + 1;
            u64 best = mine[j];
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int axes = (dz != 0) + (dy != 0) + (dx != 0);
                        if (axes == 0 || axes > AXES) continue;
                        const u64 q = ld_lds(c + (dz * KY + dy) * KX + dx);
                        const u64 cand = q + ((dx ? cx : 0) + (dy ? cy : 0) + (dz ? cz : 0));
                        if (q != UNREACHED && cand < best) best = cand;
                    }
            if (best < mine[j]) {
                mine[j] = best;
                st_lds(c, best);
                changed |= 1u << j;
                moved = 1;
            }
        }
        if (!__syncthreads_or(moved)) break;
    }
    // the keys this lane changed, and the directions in which one of them lies on the tile's border
    unsigned mark = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (!((changed >> j) & 1u)) continue;
        const int row = w + 4 * j, ly = row % TY, lz = row / TY;
        const int gx = o.x + 1 + lane, gy = o.y + 1 + ly, gz = o.z + 1 + lz;
        st_key(key + ((size_t)gz * H + gy) * W + gx, mine[j]);
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int axes = (dz != 0) + (dy != 0) + (dx != 0);
                    if (axes == 0 || axes > AXES) continue;
                    const bool on_x = dx == 0 || (dx < 0 ? lane == 0 : lane == TX - 1);
                    const bool on_y = dy == 0 || (dy < 0 ? ly == 0 : ly == TY - 1);
                    const bool on_z = dz == 0 || (dz < 0 ? lz == 0 : lz == TZ - 1);
                    if (on_x && on_y && on_z) mark |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
                }
    }
    mark = wave_reduce(mark, [](unsigned p, unsigned q) { return p | q; });
    if (lane == 0 && mark) atomicOr(&s_mark, mark);
    __syncthreads();
    if (threadIdx.x < 27 && ((s_mark >> threadIdx.x) & 1u)) {
        const int dir = threadIdx.x, dz = dir / 9 - 1, dy = (dir / 3) % 3 - 1, dx = dir % 3 - 1;
        const int tx = (int)t % a.g.tx + dx, ty = ((int)t / a.g.tx) % a.g.ty + dy, tz = (int)t / (a.g.tx * a.g.ty) + dz;
        if (tx >= 0 && tx < a.g.tx && ty >= 0 && ty < a.g.ty && tz >= 0 && tz < a.g.tz)
            flags_out[(size_t)k * a.g.tiles + (tz * a.g.ty + ty) * a.g.tx + tx] = 1;
    }
}

// ---- rest: the voxels of S that no kept core reached, as the set of the second labelling ------------------------------------------------
__global__ __launch_bounds__(256) void k_vs_rest(const uint8_t *__restrict__ masks, GrowArgs a, const u64 *__restrict__ key, uint8_t *sel,
                                                 unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const unsigned k = i / a.d.dhw, src = i - k * a.d.dhw;
    sel[i] = masks[src] == pick_value(a.v, (int)k) && key[i] == UNREACHED;
}

// ---- pieces: the root of every voxel's piece -- the marker's voxel, or the root of its component of the rest ------------------------------
__global__ __launch_bounds__(256) void k_vs_pieces(const uint8_t *__restrict__ masks, GrowArgs a, const u64 *__restrict__ key,
                                                   const uint8_t *__restrict__ sel, int *parent, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const unsigned k = i / a.d.dhw, src = i - k * a.d.dhw;
    if (sel[i]) parent[i] = pp::find_root_ro(parent, (int)i);   // (every store is the final root: racing walks stay right)
    else if (masks[src] == pick_value(a.v, (int)k)) parent[i] = (int)(k * a.d.dhw + (unsigned)(key[i] & 0x7FFFFFFFull));
}

// ---- roots: a slot for every piece ----------------------------------------------------------------------------------------------------------
// The root of a cored piece is its marker's voxel, whose key is (0, itself); that of a coreless piece is its raster-first voxel.
__global__ __launch_bounds__(256) void k_vs_roots(const int *__restrict__ parent, const uint8_t *__restrict__ sel, const int *__restrict__ csize,
                                                  GrowArgs a, unsigned S, VolumeRankAcc *acc, PlaneCount *cnt, int *slot, mi_unet_vcomp *stat,
                                                  mi_unet_vpiece *info, int *tidx, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const bool root = i < N && parent[i] == (int)i;
    unsigned k = root ? i / a.d.dhw : 0xFFFFFFFFu;
    unsigned s = 0;
    peel<64>(k, 0xFFFFFFFFu, [&](unsigned k0, bool mine, u64 mk, int leader) {
        const unsigned slot_k0 = wave_take(&acc[k0].nroots, mk, leader);
        if (mine) s = slot_k0;
    });
    if (!root) return;
    if (s >= S) { slot[i] = NO_SLOT; acc[k].overflow = 1u; return; }
    slot[i] = (int)s;
    mi_unet_vcomp c;
    c.voxels = 0; c.first = 0x7FFFFFFF;
    c.x0 = c.y0 = c.z0 = 0x7FFFFFFF; c.x1 = c.y1 = c.z1 = -1;
    c.kept = 1; c.value = pick_value(a.v, (int)k);
    c.faces_x = c.faces_y = c.faces_z = 0; c.sx = c.sy = c.sz = 0;
    stat[(size_t)k * S + s] = c;
    mi_unet_vpiece p;
    const bool coreless = sel[i] != 0;
    p.core_first = coreless ? -1 : (int)(i - k * a.d.dhw);
    p.core_voxels = coreless ? 0 : csize[i];
    p.reach = 0; p.cut_x = p.cut_y = p.cut_z = 0;
    info[(size_t)k * S + s] = p;
    tidx[(size_t)k * S + s] = 0;
    if (coreless) atomicAdd(&cnt[k].coreless, 1ull);
}

// ---- stats: the sums of every piece (k_vol_stats with "same piece" for "in the set") -------------------------------------------------------
// A wave reduces per distinct piece inside a 64-voxel segment and carries that piece's sums over RUN consecutive segments; it issues
// its atomics only when the piece changes, from eighteen lanes at once.
__global__ __launch_bounds__(256) void k_vs_stats(const int *__restrict__ parent, const u64 *__restrict__ key, Dims d, unsigned S,
                                                  const int *__restrict__ slot, mi_unet_vcomp *stat, mi_unet_vpiece *info, unsigned N)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * 256 + threadIdx.x) >> 6) * (64LL * RUN);
    const int W = d.W, H = d.H, D = d.D, hw = H * W;
    int ar = -1, an = 0, af = 0x7FFFFFFF, lo[3] = { 0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF }, hi[3] = { -1, -1, -1 };       // (wave-uniform)
    int fc[3] = { 0, 0, 0 }, ct[3] = { 0, 0, 0 };
    long long sm[3] = { 0, 0, 0 }, reach = 0;
    auto flush = [&]() {
        if (ar < 0) return;                                     // (wave-uniform)
        const int s = slot[ar];
        if (s == NO_SLOT) return;
        const size_t at = (size_t)((unsigned)ar / d.dhw) * S + s;
        mi_unet_vcomp *const c = stat + at;
        mi_unet_vpiece *const p = info + at;
        switch (lane) {
        case 0: atomicAdd(&c->voxels, an); break;
        case 1: atomicMin(&c->x0, lo[0]); break;
        case 2: atomicMin(&c->y0, lo[1]); break;
        case 3: atomicMin(&c->z0, lo[2]); break;
        case 4: atomicMax(&c->x1, hi[0]); break;
        case 5: atomicMax(&c->y1, hi[1]); break;
        case 6: atomicMax(&c->z1, hi[2]); break;
        case 7: atomicAdd(reinterpret_cast<u64 *>(&c->faces_x), (u64)fc[0]); break;
        case 8: atomicAdd(reinterpret_cast<u64 *>(&c->faces_y), (u64)fc[1]); break;
        case 9: atomicAdd(reinterpret_cast<u64 *>(&c->faces_z), (u64)fc[2]); break;
        case 10: atomicAdd(reinterpret_cast<u64 *>(&c->sx), (u64)sm[0]); break;
        case 11: atomicAdd(reinterpret_cast<u64 *>(&c->sy), (u64)sm[1]); break;
        case 12: atomicAdd(reinterpret_cast<u64 *>(&c->sz), (u64)sm[2]); break;
        case 13: atomicMin(&c->first, af); break;
        case 14: atomicMax(reinterpret_cast<u64 *>(&p->reach), (u64)reach); break;
        case 15: atomicAdd(reinterpret_cast<u64 *>(&p->cut_x), (u64)ct[0]); break;
        case 16: atomicAdd(reinterpret_cast<u64 *>(&p->cut_y), (u64)ct[1]); break;
        case 17: atomicAdd(reinterpret_cast<u64 *>(&p->cut_z), (u64)ct[2]); break;
        default: break;
        }
    };
    for (int sg = 0; sg < RUN; ++sg) {
        const long long i = first + 64LL * sg + lane;
        if (first + 64LL * sg >= (long long)N) break;           // (wave-uniform)
        int r = -1, co[3] = { 0, 0, 0 }, f[3] = { 0, 0, 0 }, cu[3] = { 0, 0, 0 }, idx = 0x7FFFFFFF;
        long long len = 0;
        if (i < (long long)N && parent[i] >= 0) {
            r = parent[i];
            const unsigned k = (unsigned)i / d.dhw, src = (unsigned)i - k * d.dhw;
            const int z = (int)(src / (unsigned)hw), rem = (int)(src - (unsigned)z * (unsigned)hw), y = rem / W, x = rem - y * W;
            const int *const m = parent + i;
            const u64 q = key[i];
            co[0] = x; co[1] = y; co[2] = z;
            idx = (int)src;
            len = q == UNREACHED ? 0 : (long long)(q >> 31);
            // the piece of a 6-neighbour: -1 outside the volume and outside S
            const int nb[6] = { x > 0 ? m[-1] : -1, x + 1 < W ? m[1] : -1, y > 0 ? m[-W] : -1, y + 1 < H ? m[W] : -1,
                                z > 0 ? m[-hw] : -1, z + 1 < D ? m[hw] : -1 };
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                f[j / 2] += nb[j] != r;
                cu[j / 2] += nb[j] != r && nb[j] >= 0;
            }
        }
        peel<64>(r, -1, [&](int r0, bool mine, u64 mm, int) {
            if (r0 != ar) {
                flush();
                ar = r0; an = 0; af = 0x7FFFFFFF; reach = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) { lo[j] = 0x7FFFFFFF; hi[j] = -1; fc[j] = 0; ct[j] = 0; sm[j] = 0; }
            }
            an += __builtin_popcountll(mm);
            af = min(af, wave_min(mine ? idx : 0x7FFFFFFF));
            reach = max(reach, wave_max(mine ? len : 0LL));
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lo[j] = min(lo[j], wave_min(mine ? co[j] : 0x7FFFFFFF));
                hi[j] = max(hi[j], wave_max(mine ? co[j] : -1));
                fc[j] += wave_sum(mine ? f[j] : 0);
                ct[j] += wave_sum(mine ? cu[j] : 0);
                sm[j] += wave_sum(mine ? (long long)co[j] : 0LL);
            }
        });
    }
    flush();
}

// ---- keys: the order key of every slot; the plane's largest reach -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vs_keys(unsigned S, const VolumeRankAcc *acc, PlaneCount *cnt, const mi_unet_vcomp *__restrict__ stat,
                                                 const mi_unet_vpiece *__restrict__ info, u64 *okey)
{
    const unsigned k = blockIdx.y;
    const unsigned found = min(acc[k].nroots, S);
    u64 reach = 0;
    for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < found; s += gridDim.x * 256u) {
        const mi_unet_vcomp *const c = stat + (size_t)k * S + s;
        okey[(size_t)k * S + s] = ((u64)(unsigned)c->voxels << 31) | (u64)(0x7FFFFFFF - c->first);
        reach = max(reach, (u64)info[(size_t)k * S + s].reach);
    }
    reach = wave_max(reach);
    if ((threadIdx.x & 63) == 0 && reach) atomicMax(&cnt[k].max_reach, reach);
}

// ---- table: the selected keys of a plane with their slots, sorted by one workgroup in LDS (k_vol_table) ----------------------------------
// The keys >= thr[1] of a plane are its min(found, cap) largest (keys are unique): at most 4096.  The slot travels with its key through
// the bitonic sort, descending, over the next power of two (0 pads: every real key is >= 2^31).  Also here: the plane's counts.
__global__ __launch_bounds__(256) void k_vs_table(int cap, int single, unsigned S, const VolumeRankAcc *acc, const PlaneCount *cnt,
                                                  const unsigned long long *counts, const u64 *__restrict__ key_all,
                                                  const mi_unet_vcomp *__restrict__ stat, const mi_unet_vpiece *__restrict__ info, int *tidx,
                                                  mi_unet_vcomp *table, mi_unet_vpiece *tinfo, VolumeSplitResult *res)
{
    __shared__ u64 s_key[VOLUME_MAX_TABLE];
    __shared__ int s_slot[VOLUME_MAX_TABLE];
    __shared__ unsigned s_n;
    const unsigned k = blockIdx.x, t = threadIdx.x;
    const VolumeRankAcc pa = acc[k];
    const unsigned found = min(pa.nroots, S);
    if (t == 0) {
        VolumeSplitResult r;
        r.in_voxels = (long long)counts[4 * k];
        r.core_voxels = (long long)counts[4 * k + (single ? 0 : 3)];
        r.cores = (long long)cnt[k].cores; r.cores_kept = (long long)cnt[k].cores_kept;
        r.coreless = (long long)cnt[k].coreless; r.max_reach = (long long)cnt[k].max_reach;
        r.found = pa.overflow ? -1 : (int)found; r.reserved = 0;
        res[k] = r;
        s_n = 0;
    }
    __syncthreads();
    const u64 *const key = key_all + (size_t)k * S;
    for (unsigned s = t; s < found; s += 256) {
        const u64 q = key[s];
        if (q >= pa.thr[1]) {
            const unsigned pos = atomicAdd(&s_n, 1u);
            if (pos < (unsigned)VOLUME_MAX_TABLE) { s_key[pos] = q; s_slot[pos] = (int)s; }
        }
    }
    __syncthreads();
    const unsigned m = min(s_n, (unsigned)cap);
    unsigned P = 2;
    while (P < m) P <<= 1;
    for (unsigned j = m + t; j < P; j += 256) { s_key[j] = 0; s_slot[j] = NO_SLOT; }
    __syncthreads();
    for (unsigned kk = 2; kk <= P; kk <<= 1)
        for (unsigned j = kk >> 1; j > 0; j >>= 1) {
            for (unsigned idx = t; idx < P; idx += 256) {
                const unsigned other = idx ^ j;
                if (other > idx) {
                    const u64 x = s_key[idx], y = s_key[other];
                    const bool desc = (idx & kk) == 0;
                    if (desc ? x < y : x > y) {
                        const int sx = s_slot[idx], sy = s_slot[other];
                        s_key[idx] = y; s_key[other] = x;
                        s_slot[idx] = sy; s_slot[other] = sx;
                    }
                }
            }
            __syncthreads();
        }
    for (unsigned j = t; j < m; j += 256) {
        const int s = s_slot[j];
        table[(size_t)k * cap + j] = stat[(size_t)k * S + s];
        if (tinfo) tinfo[(size_t)k * cap + j] = info[(size_t)k * S + s];
        tidx[(size_t)k * S + s] = (int)j + 1;
    }
}

// ---- write: ids ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vs_write(Dims d, unsigned S, const int *__restrict__ parent, const int *__restrict__ slot,
                                                  const int *__restrict__ tidx, int32_t *ids, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const int r = parent[i];
    int id = 0;
    if (r >= 0) {
        const int s = slot[r];
        id = -1;
        if (s != NO_SLOT) {
            const int ti = tidx[(size_t)((unsigned)r / d.dhw) * S + s];
            if (ti) id = ti;
        }
    }
    ids[i] = id;
}

struct Call { Ws w; Dims d; Grid g; GrowArgs ga; unsigned N, S; int axes; };

inline bool make_call(const uint8_t *masks, const VolumeSplitArgs &a, void *ws, Call &c)
{
    if (!masks || !ws || a.D < 1 || a.H < 1 || a.W < 1 || a.n < 1 || a.n > VOLUME_MAX_VALUES) return false;
    if (a.cap < 1 || a.cap > VOLUME_MAX_TABLE || a.min_core < 0 || a.neck_r < 0 || a.neck_r > VOLUME_CLEAN_MAX_R) return false;
    if (a.connectivity != 6 && a.connectivity != 18 && a.connectivity != 26) return false;
    for (int u : { a.ux, a.uy, a.uz })
        if (u < 1 || u > VOLUME_CLEAN_MAX_R) return false;
    const unsigned long long dhw64 = (unsigned long long)a.D * a.H * a.W, N64 = dhw64 * a.n;
    if ((unsigned long long)a.D * a.H > 0x7FFFFFFFull || N64 > 0x7FFFFFFFull) return false;
    if (dhw64 * ((unsigned long long)a.ux + a.uy + a.uz) >= (1ull << 33)) return false;
    c.w = carve(ws, a.D, a.H, a.W, a.n);
    c.d = Dims{ a.D, a.H, a.W, (unsigned)dhw64 };
    c.g = grid_of(a.D, a.H, a.W);
    c.ga.d = c.d; c.ga.g = c.g; c.ga.ux = a.ux; c.ga.uy = a.uy; c.ga.uz = a.uz;
    for (int k = 0; k < VOLUME_MAX_VALUES; ++k) c.ga.v[k] = a.v[k];
    c.N = (unsigned)N64;
    c.S = (unsigned)volume_slots_per_plane((size_t)dhw64);
    c.axes = a.connectivity == 6 ? 1 : a.connectivity == 18 ? 2 : 3;
    return true;
}

inline void label(const Call &c, hipStream_t s)
{
    const dim3 g((c.N + 255u) / 256u), blk(256);
    hipLaunchKernelGGL(k_vs_init, g, blk, 0, s, c.w.sel, c.w.parent, c.N);
    if (c.axes == 1) hipLaunchKernelGGL(k_vs_merge<1>, g, blk, 0, s, c.w.sel, c.d, c.w.parent, c.N);
    else if (c.axes == 2) hipLaunchKernelGGL(k_vs_merge<2>, g, blk, 0, s, c.w.sel, c.d, c.w.parent, c.N);
    else hipLaunchKernelGGL(k_vs_merge<3>, g, blk, 0, s, c.w.sel, c.d, c.w.parent, c.N);
}

}  // namespace vs

size_t volume_split_workspace_bytes(int D, int H, int W, int n) { return vs::carve(nullptr, D, H, W, n).total; }

hipError_t launch_volume_split_seed(const uint8_t *masks, const VolumeSplitArgs &a, void *ws, hipStream_t s)
{
    vs::Call c;
    if (!vs::make_call(masks, a, ws, c)) return hipErrorInvalidValue;
    const vs::Ws &w = c.w;
    VolumeCleanArgs ea;
    ea.D = a.D; ea.H = a.H; ea.W = a.W; ea.n = a.n; ea.ux = a.ux; ea.uy = a.uy; ea.uz = a.uz; ea.fill = 0; ea.close_r = 0; ea.open_r = a.neck_r;
    for (int k = 0; k < VOLUME_MAX_VALUES; ++k) ea.v[k] = a.v[k];
    if (hipError_t e = launch_volume_erode(masks, ea, w.sel, w.counts, w.erode, s)) return e;
    if (hipError_t e = hipMemsetAsync(w.acc, 0, (size_t)a.n * sizeof(VolumeRankAcc), s)) return e;
    if (hipError_t e = hipMemsetAsync(w.cnt, 0, (size_t)a.n * sizeof(vs::PlaneCount), s)) return e;
    if (hipError_t e = hipMemsetAsync(w.flags[0], 0, (size_t)a.n * c.g.tiles, s)) return e;
    if (hipError_t e = hipMemsetAsync(w.flags[1], 0, (size_t)a.n * c.g.tiles, s)) return e;
    if (hipError_t e = hipMemsetAsync(w.csize, 0, (size_t)c.N * sizeof(int), s)) return e;
    vs::label(c, s);
    const dim3 g((c.N + 255u) / 256u), blk(256);
    hipLaunchKernelGGL(vs::k_vs_core_count, g, blk, 0, s, w.parent, w.csize, c.N);
    hipLaunchKernelGGL(vs::k_vs_seed, g, blk, 0, s, w.sel, w.parent, w.csize, c.d, c.g, a.min_core, w.key, w.flags[0], w.cnt, c.N);
    return hipGetLastError();
}

hipError_t launch_volume_split_round(const uint8_t *masks, const VolumeSplitArgs &a, void *ws, int round, unsigned *active, hipStream_t s)
{
    vs::Call c;
    if (!vs::make_call(masks, a, ws, c) || !active || round < 0) return hipErrorInvalidValue;
    const dim3 g((unsigned)a.n * (unsigned)c.g.tiles), blk(256);
    uint8_t *const in = c.w.flags[round & 1], *const out = c.w.flags[(round + 1) & 1];
    if (c.axes == 1) hipLaunchKernelGGL(vs::k_vs_grow<1>, g, blk, 0, s, masks, c.ga, c.w.key, in, out, active);
    else if (c.axes == 2) hipLaunchKernelGGL(vs::k_vs_grow<2>, g, blk, 0, s, masks, c.ga, c.w.key, in, out, active);
    else hipLaunchKernelGGL(vs::k_vs_grow<3>, g, blk, 0, s, masks, c.ga, c.w.key, in, out, active);
    return hipGetLastError();
}

hipError_t launch_volume_split_finish(const uint8_t *masks, const VolumeSplitArgs &a, int32_t *ids, mi_unet_vcomp *table, mi_unet_vpiece *info,
                                      VolumeSplitResult *res, void *ws, hipStream_t s)
{
    vs::Call c;
    if (!vs::make_call(masks, a, ws, c) || !table || !res) return hipErrorInvalidValue;
    const vs::Ws &w = c.w;
    if (hipError_t e = hipMemsetAsync(table, 0, (size_t)a.n * a.cap * sizeof(mi_unet_vcomp), s)) return e;
    if (info)
        if (hipError_t e = hipMemsetAsync(info, 0, (size_t)a.n * a.cap * sizeof(mi_unet_vpiece), s)) return e;
    const dim3 g((c.N + 255u) / 256u), blk(256);
    hipLaunchKernelGGL(vs::k_vs_rest, g, blk, 0, s, masks, c.ga, w.key, w.sel, c.N);
    vs::label(c, s);
    hipLaunchKernelGGL(vs::k_vs_pieces, g, blk, 0, s, masks, c.ga, w.key, w.sel, w.parent, c.N);
    hipLaunchKernelGGL(vs::k_vs_roots, g, blk, 0, s, w.parent, w.sel, w.csize, c.ga, c.S, w.acc, w.cnt, w.slot, w.stat, w.info, w.tidx, c.N);
    const unsigned sblocks = (unsigned)(((unsigned long long)c.N + 256ull * vs::RUN - 1) / (256ull * vs::RUN));
    hipLaunchKernelGGL(vs::k_vs_stats, dim3(sblocks), blk, 0, s, w.parent, w.key, c.d, c.S, w.slot, w.stat, w.info, c.N);
    unsigned lblocks = (c.S + 255u) / 256u;
    if (lblocks > 1024u) lblocks = 1024u;
    hipLaunchKernelGGL(vs::k_vs_keys, dim3(lblocks, (unsigned)a.n), blk, 0, s, c.S, w.acc, w.cnt, w.stat, w.info, w.okey);
    VolumeArgs va;
    va.D = a.D; va.H = a.H; va.W = a.W; va.n = a.n; va.cap = a.cap; va.connectivity = a.connectivity;
    if (hipError_t e = launch_volume_select(va, c.S, w.acc, w.okey, s)) return e;
    const int single = a.neck_r / a.ux == 0 && a.neck_r / a.uy == 0 && a.neck_r / a.uz == 0;
    hipLaunchKernelGGL(vs::k_vs_table, dim3((unsigned)a.n), blk, 0, s, a.cap, single, c.S, w.acc, w.cnt, w.counts, w.okey, w.stat, w.info,
                       w.tidx, table, info, res);
    if (ids) hipLaunchKernelGGL(vs::k_vs_write, g, blk, 0, s, c.d, c.S, w.parent, w.slot, w.tidx, ids, c.N);
    return hipGetLastError();
}

}  // namespace miunet
