// volume_branches.hip -- a skeleton split into nodes and branches, short spurs pruned (include/mi_unet.h: mi_unet_volume_branches;
// DESIGN.md 7.23).  One sweep over the volume (key_tile.h's tile with its halo in LDS) classifies every object voxel by its number of
// same-object neighbours and compacts the object voxels into a list; everything behind it runs over that list and gathers its 26
// neighbours from memory.  Junction clusters and branches are the sets of a lock-free union-find on (id, class) whose parents only
// decrease, so a set's root is its lowest voxel: the definition's `first` and key.  Roots and keys are numbered in raster order through
// two bitmaps and a two-level scan of their popcounts.  A pruning round regathers the classes and runs the same kernels again.  Exact
// integers (sums, counts, minima, maxima), vector stores only; no result depends on the order in which lanes, waves or workgroups run,
// no workgroup waits for another, and every loop is bounded by a list length or a side.  gfx950 only.
#include <algorithm>

#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "key_tile.h"
#include "wave.h"

namespace miunet {

namespace vbr {

using namespace wave;
using key_tile::KX;
using key_tile::KY;
using key_tile::TX;
using key_tile::TY;
using key_tile::TZ;
using key_tile::walk_tile;

constexpr int WG = 256;
constexpr int KZ = TZ + 2;                               // a tile with one voxel of halo on every side, as 7.22's
constexpr int TILE_KEYS = KX * KY * KZ;
constexpr unsigned MAX_GRID = 4096;                      // workgroups of a grid-stride launch
constexpr int CHUNK_WORDS = 8;                           // a chunk of the numbering: 256 voxels, 8 words of a bitmap
constexpr int NO_ATT_LO = 0x7FFFFFFF;

enum : uint8_t { NONE = 0, ISOLATED = 1, END = 2, BRANCH = 3, JUNCTION = 4 };

struct Ws {
    int32_t *list;                  // [dhw] the object voxels of the input, in the order of arrival (nothing below shows it)
    int32_t *parent;                // [dhw] at object voxels: the forest; behind k_vbr_flatten the set's lowest voxel
    int32_t *nvox, *att_lo, *att_hi;  // [dhw] at a branch's root: its voxels and the smaller / larger attached node voxel
    uint8_t *cls, *dead;            // [dhw] at object voxels: the class; whether the round deletes the voxel
    uint32_t *node_bits, *branch_bits;  // [words] a bit per voxel: the node's first voxel, the branch's key
    int2 *chunk_base, *super_total, *super_base;   // the scan: (nodes, branches) before a chunk inside its block of 256 chunks; per block
    size_t words, chunks, supers, total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline Ws carve(void *base, int D, int H, int W)
{
    Ws w;
    const size_t dhw = (size_t)D * H * W;
    w.chunks = (dhw + 255) / 256;
    w.words = w.chunks * CHUNK_WORDS;
    w.supers = (w.chunks + WG - 1) / WG;
    uint8_t *p = static_cast<uint8_t *>(base);
    size_t at = 0;
    auto take = [&](size_t bytes) { uint8_t *r = p + at; at += up256(bytes); return r; };
    w.list = reinterpret_cast<int32_t *>(take(dhw * sizeof(int32_t)));
    w.parent = reinterpret_cast<int32_t *>(take(dhw * sizeof(int32_t)));
    w.nvox = reinterpret_cast<int32_t *>(take(dhw * sizeof(int32_t)));
    w.att_lo = reinterpret_cast<int32_t *>(take(dhw * sizeof(int32_t)));
    w.att_hi = reinterpret_cast<int32_t *>(take(dhw * sizeof(int32_t)));
    w.cls = take(dhw);
    w.dead = take(dhw);
    w.node_bits = reinterpret_cast<uint32_t *>(take(2 * w.words * sizeof(uint32_t)));     // (both bitmaps: one clear)
    w.branch_bits = w.node_bits + w.words;
    w.chunk_base = reinterpret_cast<int2 *>(take(w.chunks * sizeof(int2)));
    w.super_total = reinterpret_cast<int2 *>(take(w.supers * sizeof(int2)));
    w.super_base = reinterpret_cast<int2 *>(take(w.supers * sizeof(int2)));
    w.total = at;
    return w;
}

inline unsigned blocks(size_t n) { return (unsigned)std::min<size_t>(std::max<size_t>((n + WG - 1) / WG, 1), MAX_GRID); }

// the pointers every list kernel takes
struct View {
    int32_t *cur;
    const int32_t *list;
    const unsigned *listed;
    int32_t *parent, *nvox, *att_lo, *att_hi;
    uint8_t *cls, *dead;
    int D, H, W;
};

__device__ __forceinline__ uint8_t class_of(int deg) { return deg == 0 ? ISOLATED : deg == 1 ? END : deg == 2 ? BRANCH : JUNCTION; }

// f(q, c) for every same-object neighbour q of voxel i with id v, c its link class |dx| + 2 |dy| + 4 |dz| - 1; gathered from memory
template <class F>
__device__ __forceinline__ void neighbours(const View &g, int i, int v, F f)
{
    const int x = (int)((unsigned)i % (unsigned)g.W), zy = (int)((unsigned)i / (unsigned)g.W), y = zy % g.H, z = zy / g.H;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!dz && !dy && !dx) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || zz >= g.D || yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) continue;
                const int q = (zz * g.H + yy) * g.W + xx;       // (< 2^31)
                if (g.cur[q] == v) f(q, (dx != 0) + 2 * (dy != 0) + 4 * (dz != 0) - 1);
            }
}

// the only neighbour of an end voxel
__device__ __forceinline__ int only_neighbour(const View &g, int i, int v)
{
    int only = i;
    neighbours(g, i, v, [&](int q, int) { only = q; });
    return only;
}

__device__ __forceinline__ void reset_voxel(const View &g, int i, int deg)
{
    g.cls[i] = class_of(deg);
    g.parent[i] = i;
    g.nvox[i] = 0;
    g.att_lo[i] = NO_ATT_LO;
    g.att_hi[i] = -1;
    g.dead[i] = 0;
}

// ---- begin: the ids normalised, the per-id table and the words cleared ------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_vbr_clear(mi_unet_vgraph *graph, int m, VbrState *state)
{
    const int r = blockIdx.x * WG + threadIdx.x;
    if (r < m) graph[r] = mi_unet_vgraph{};
    if (r == 0) *state = VbrState{};
}

__global__ __launch_bounds__(WG) void k_vbr_init(int32_t *__restrict__ cur, unsigned dhw, int m)
{
    for (unsigned i = blockIdx.x * WG + threadIdx.x; i < dhw; i += gridDim.x * WG) {
        const int v = cur[i];
        if (v < 1 || v > m) cur[i] = 0;
    }
}

// ---- the one sweep over the volume: degree, class, and the list of object voxels ------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_vbr_classify(View g, int tiles_x, int tiles_y, int n_tiles, int32_t *__restrict__ list, unsigned *listed)
{
    __shared__ int s_keys[TILE_KEYS];
    const int t_end = min(n_tiles, ((int)blockIdx.x + 1) * VTX_TILES_PER_WG);
    for (int tile = (int)blockIdx.x * VTX_TILES_PER_WG; tile < t_end; ++tile) {
        __syncthreads();                                        // the tile before is done with s_keys
        const int3 o = key_tile::tile_origin<1>(tile, tiles_x, tiles_y);
        key_tile::load_key_tile<KZ, 1>(s_keys, g.cur, o, g.D, g.H, g.W);
        __syncthreads();
        walk_tile(s_keys, o, g.D, g.H, g.W, [&](size_t i, bool, int v, uint32_t code) {
            if (v) reset_voxel(g, (int)i, __popc(code));
            int key = v ? 0 : -1;
            peel<64>(key, -1, [&](int, bool mine, u64 mask, int leader) {
                const unsigned pos = wave_take(listed, mask, leader);
                if (mine) list[pos] = (int32_t)i;               // (pos < dhw: a voxel is listed once)
            });
        });
    }
}

// a later round: the classes of what is left, the degrees gathered from memory as k_vsk_substep gathers its bits
__global__ __launch_bounds__(WG) void k_vbr_regather(View g)
{
    const unsigned n = *g.listed;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n; j += gridDim.x * WG) {
        const int i = g.list[j], v = g.cur[i];
        if (!v) { g.cls[i] = NONE; continue; }
        int deg = 0;
        neighbours(g, i, v, [&](int, int) { ++deg; });
        reset_voxel(g, i, deg);
    }
}

// ---- the forest: clusters and branches ------------------------------------------------------------------------------------------------------------------
// Parents only decrease and a voxel's parent is a voxel of its set, so a walk up ends at a root after fewer steps than the list is long.
__device__ __forceinline__ int find(int32_t *parent, int x)
{
    for (;;) {
        const int p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
        if (p == x) return x;
        x = p;
    }
}

// the sets of a and b become one.  The higher root is hung under the lower; where another lane was faster (the word no longer holds
// the root itself) the minimum still stands and what it replaced is joined next, so no link is lost.  Every retry follows a link that
// another lane made, and there are fewer links than voxels.
__device__ __forceinline__ void unite(int32_t *parent, int a, int b)
{
    for (;;) {
        a = find(parent, a);
        b = find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(WG) void k_vbr_link(View g)
{
    const unsigned n = *g.listed;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n; j += gridDim.x * WG) {
        const int i = g.list[j], v = g.cur[i];
        const uint8_t c = v ? g.cls[i] : (uint8_t)NONE;
        if (c != BRANCH && c != JUNCTION) continue;
        neighbours(g, i, v, [&](int q, int) {
            if (q < i && g.cls[q] == c) unite(g.parent, i, q);  // (a pair from its higher voxel)
        });
    }
}

__global__ __launch_bounds__(WG) void k_vbr_flatten(View g)
{
    const unsigned n = *g.listed;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n; j += gridDim.x * WG) {
        const int i = g.list[j];
        if (!g.cur[i] || g.cls[i] < BRANCH) continue;
        const int r = find(g.parent, i);
        __atomic_store_n(g.parent + i, r, __ATOMIC_RELAXED);    // (whoever reads the old value still walks up to r)
    }
}

// ---- a branch's voxels and its two attached node voxels ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_vbr_attach(View g)
{
    const unsigned n = *g.listed, n_up = (n + 63u) & ~63u;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n_up; j += gridDim.x * WG) {
        const int i = j < n ? g.list[j] : 0, v = j < n ? g.cur[i] : 0;
        int root = v && g.cls[i] == BRANCH ? g.parent[i] : -1;
        peel<64>(root, -1, [&](int r0, bool, u64 mask, int leader) {
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(g.nvox + r0, (int)__popcll(mask));
        });
        if (root < 0) continue;
        neighbours(g, i, v, [&](int q, int) {
            if (g.cls[q] == BRANCH) return;
            lower(g.att_lo + root, q);
            raise(g.att_hi + root, q);
        });
    }
}

// the branch with root r: open, one node an end and the other a junction, short enough
__device__ __forceinline__ bool spur_at(const View &g, int r, int prune_voxels)
{
    const int lo = g.att_lo[r], hi = g.att_hi[r];
    if (hi < 0 || g.nvox[r] >= prune_voxels) return false;      // (voxels + 1 <= prune_voxels)
    const uint8_t a = g.cls[lo], b = g.cls[hi];
    return (a == END && b == JUNCTION) || (a == JUNCTION && b == END);
}

// ---- the spurs of the state's graph: counted at their end voxels, their voxels flagged; nothing is deleted here, so every read is of a
// state no lane of this launch writes
__global__ __launch_bounds__(WG) void k_vbr_mark(View g, int prune_voxels, unsigned *spurs)
{
    const unsigned n = *g.listed, n_up = (n + 63u) & ~63u;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n_up; j += gridDim.x * WG) {
        bool end_of_spur = false;
        if (j < n) {
            const int i = g.list[j], v = g.cur[i];
            const uint8_t c = v ? g.cls[i] : (uint8_t)NONE;
            bool dead = false;
            if (c == BRANCH) dead = spur_at(g, g.parent[i], prune_voxels);
            if (c == END) {
                const int q = only_neighbour(g, i, v);
                const uint8_t cq = g.cls[q];
                dead = cq == JUNCTION ? prune_voxels >= 1 : cq == BRANCH && spur_at(g, g.parent[q], prune_voxels);
                end_of_spur = dead;
            }
            if (v) g.dead[i] = dead;
        }
        const u64 mask = __ballot(end_of_spur);
        if (mask && (threadIdx.x & 63) == 0) atomicAdd(spurs, (unsigned)__popcll(mask));
    }
}

__device__ __forceinline__ void add64(int64_t *p, u64 v)
{
    if (v) atomicAdd(reinterpret_cast<u64 *>(p), v);
}

// a lane writes its own voxel only and reads no other voxel's id
__global__ __launch_bounds__(WG) void k_vbr_delete(View g, mi_unet_vgraph *graph)
{
    const unsigned n = *g.listed, n_up = (n + 63u) & ~63u;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n_up; j += gridDim.x * WG) {
        int id = 0;
        bool end = false;
        if (j < n) {
            const int i = g.list[j], v = g.cur[i];
            if (v && g.dead[i]) {
                id = v;
                end = g.cls[i] == END;
                g.cur[i] = 0;
            }
        }
        peel<64>(id, 0, [&](int k0, bool mine, u64 mask, int leader) {
            const u64 ends = __ballot(mine && end);
            if ((int)(threadIdx.x & 63) != leader) return;
            add64(&graph[k0 - 1].pruned_voxels, (u64)__popcll(mask));
            add64(&graph[k0 - 1].pruned_spurs, (u64)__popcll(ends));
        });
    }
}

// ---- the numbering: a bit per first voxel and per key, their popcounts scanned in raster order -------------------------------------------------------------
// an end voxel that keys a zero-voxel branch: its only neighbour is a junction voxel, or an end voxel of a higher index
__device__ __forceinline__ bool keys_zero_branch(const View &g, int i, int q)
{
    const uint8_t cq = g.cls[q];
    return cq == JUNCTION || (cq == END && q > i);
}

__global__ __launch_bounds__(WG) void k_vbr_flags(View g, uint32_t *node_bits, uint32_t *branch_bits)
{
    const unsigned n = *g.listed;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n; j += gridDim.x * WG) {
        const int i = g.list[j], v = g.cur[i];
        if (!v) continue;
        const uint8_t c = g.cls[i];
        const bool root = c >= BRANCH && g.parent[i] == i;
        const bool node = c == ISOLATED || c == END || (c == JUNCTION && root);
        const bool key = (c == BRANCH && root) || (c == END && keys_zero_branch(g, i, only_neighbour(g, i, v)));
        if (node) atomicOr(node_bits + ((unsigned)i >> 5), 1u << (i & 31));
        if (key) atomicOr(branch_bits + ((unsigned)i >> 5), 1u << (i & 31));
    }
}

// the exclusive sum of `mine` over the 256 lanes of the workgroup (nodes in the low word, branches in the high) and the workgroup's total;
// s_w: four words of LDS, free again behind the barrier the caller puts before its next use
__device__ __forceinline__ u64 block_scan(u64 mine, u64 *s_w, u64 &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    u64 before = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < w) before += s_w[k];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return before + incl - mine;
}

__global__ __launch_bounds__(WG) void k_vbr_scan_chunks(const uint32_t *__restrict__ node_bits, const uint32_t *__restrict__ branch_bits, unsigned chunks,
                                                        int2 *__restrict__ chunk_base, int2 *__restrict__ super_total)
{
    __shared__ u64 s_w[4];
    const unsigned c = blockIdx.x * WG + threadIdx.x;
    u64 mine = 0;
    if (c < chunks) {
#pragma unroll
        for (int k = 0; k < CHUNK_WORDS; ++k)
            mine += (u64)__popc(node_bits[(size_t)c * CHUNK_WORDS + k]) | (u64)__popc(branch_bits[(size_t)c * CHUNK_WORDS + k]) << 32;
    }
    u64 total;
    const u64 before = block_scan(mine, s_w, total);
    if (c < chunks) chunk_base[c] = make_int2((int)(uint32_t)before, (int)(before >> 32));
    if (threadIdx.x == 0) super_total[blockIdx.x] = make_int2((int)(uint32_t)total, (int)(total >> 32));
}

// one workgroup: the blocks' totals scanned, 256 at a time (at most 2^15 blocks: 128 turns)
__global__ __launch_bounds__(WG) void k_vbr_scan_supers(const int2 *__restrict__ super_total, unsigned supers, int2 *__restrict__ super_base, VbrState *state)
{
    __shared__ u64 s_w[4];
    u64 carry = 0;
    for (unsigned at = 0; at < supers; at += WG) {
        const unsigned k = at + threadIdx.x;
        u64 mine = 0;
        if (k < supers) mine = (u64)(uint32_t)super_total[k].x | (u64)(uint32_t)super_total[k].y << 32;
        u64 total;
        const u64 before = carry + block_scan(mine, s_w, total);
        if (k < supers) super_base[k] = make_int2((int)(uint32_t)before, (int)(before >> 32));
        carry += total;
        __syncthreads();                                        // s_w is free for the next turn
    }
    if (threadIdx.x == 0) {
        state->found_nodes = (uint32_t)carry;
        state->found_branches = (uint32_t)(carry >> 32);
    }
}

struct Ranks {
    const uint32_t *node_bits, *branch_bits;
    const int2 *chunk_base, *super_base;
};

// how many bits of `bits` are set before voxel i: the number of its node or branch in raster order
template <bool BRANCHES>
__device__ __forceinline__ int rank_of(const Ranks &r, int i)
{
    const uint32_t *const bits = BRANCHES ? r.branch_bits : r.node_bits;
    const unsigned c = (unsigned)i >> 8, w = (unsigned)i >> 5;
    const int2 sb = r.super_base[c >> 8], cb = r.chunk_base[c];
    int rank = BRANCHES ? sb.y + cb.y : sb.x + cb.x;
    for (unsigned k = c * CHUNK_WORDS; k < w; ++k) rank += __popc(bits[k]);     // (at most 7 words)
    return rank + __popc(bits[w] & ((1u << (i & 31)) - 1u));
}

// ---- the rows ---------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_vbr_rows_clear(mi_unet_vnode *nodes, int n_nodes, mi_unet_vbranch *branches, int n_branches, int want_r2)
{
    const int r = blockIdx.x * WG + threadIdx.x;
    if (r < n_nodes) {
        mi_unet_vnode t{};
        if (want_r2) t.r2_min = 0x7FFFFFFF;
        nodes[r] = t;
    }
    if (r < n_branches) {
        mi_unet_vbranch t{};
        if (want_r2) t.r2_min = 0x7FFFFFFF;                     // (k_vbr_rows_fix puts 0 where the branch has no voxel)
        branches[r] = t;
    }
}

// One pass over the list.  Every pair that belongs to a branch is counted at the branch's side: a branch voxel counts its attachment
// pairs and, from the lower voxel, the pairs with its own branch; the end voxel that keys a zero-voxel branch counts its one pair.  So a
// lane adds to one branch row, one node row and one id row; a wave merges per row before its atomics.  The lane of a root or key writes
// the row's fields that are no sums.
__global__ __launch_bounds__(WG) void k_vbr_rows(View g, Ranks rk, const int32_t *__restrict__ r2, mi_unet_vnode *nodes, int n_nodes,
                                                 mi_unet_vbranch *branches, int n_branches, mi_unet_vgraph *graph, int32_t *__restrict__ map)
{
    const unsigned n = *g.listed, n_up = (n + 63u) & ~63u;
    for (unsigned j = blockIdx.x * WG + threadIdx.x; j < n_up; j += gridDim.x * WG) {
        const int i = j < n ? g.list[j] : 0, v = j < n ? g.cur[i] : 0;
        if (!__ballot(v != 0)) continue;                        // (wave-uniform)
        const uint8_t c = v ? g.cls[i] : (uint8_t)NONE;
        const int d = v && r2 ? r2[i] : 0;
        const bool root = c >= BRANCH && g.parent[i] == i;
        // the node side
        int node = -1;
        const bool node_first = c == ISOLATED || c == END || (c == JUNCTION && root);
        if (c == ISOLATED || c == END || c == JUNCTION) node = rank_of<false>(rk, c == JUNCTION ? g.parent[i] : i);
        // the branch side: the row and the pairs this voxel counts, 10 bits a class (a lane adds at most 2, a wave 128)
        int branch = -1, only = -1;
        bool key = false;
        u64 la = 0, lb = 0;                                     // l0 .. l4 | l5 l6
        auto count = [&](int cl) { if (cl < 5) la += 1ull << (10 * cl); else lb += 1ull << (10 * (cl - 5)); };
        if (c == BRANCH) {
            branch = rank_of<true>(rk, g.parent[i]);
            key = root;
            neighbours(g, i, v, [&](int q, int cl) {
                if (g.cls[q] != BRANCH || q > i) count(cl);
            });
        } else if (c == END) {
            only = only_neighbour(g, i, v);
            if (keys_zero_branch(g, i, only)) {
                branch = rank_of<true>(rk, i);
                key = true;
                neighbours(g, i, v, [&](int, int cl) { count(cl); });
            }
        }
        if (map && v) map[i] = c == BRANCH ? branch + 1 : -(node + 1);
        // what the lane of a key knows about its branch
        int att_lo = -1, att_hi = -1, node_a = -1, node_b = -1;
        bool closed = false;
        if (key) {
            if (c == BRANCH) {
                att_hi = g.att_hi[i];
                closed = att_hi < 0;
                if (!closed) att_lo = g.att_lo[i];
            } else {
                att_lo = min(i, only); att_hi = max(i, only);
            }
            if (!closed) {
                node_a = rank_of<false>(rk, g.cls[att_lo] == JUNCTION ? g.parent[att_lo] : att_lo);
                node_b = rank_of<false>(rk, g.cls[att_hi] == JUNCTION ? g.parent[att_hi] : att_hi);
                if (node_a < n_nodes) atomicAdd(&nodes[node_a].degree, 1);
                if (node_b < n_nodes) atomicAdd(&nodes[node_b].degree, 1);
            }
            if (branch < n_branches) {
                mi_unet_vbranch *const t = branches + branch;
                t->first = i; t->att_lo = att_lo; t->att_hi = att_hi;
                t->id = v; t->kind = closed ? 1 : c == BRANCH ? 0 : 2; t->node_a = node_a; t->node_b = node_b;
            }
        }
        if (node_first && node < n_nodes) {
            mi_unet_vnode *const t = nodes + node;
            t->first = i; t->id = v; t->kind = c == ISOLATED ? 0 : c == END ? 1 : 2;
        }
        // the id's row: seven counts of at most 64 in 8 bits each, and the links
        {
            const u64 cnt = (u64)node_first | (u64)(c == END) << 8 | (u64)(c == JUNCTION && root) << 16 | (u64)(c == ISOLATED) << 24 |
                            (u64)(c == JUNCTION) << 32 | (u64)key << 40 | (u64)closed << 48;
            int id = v;
            peel<64>(id, 0, [&](int k0, bool mine, u64, int leader) {
                const u64 sc = wave_sum(mine ? cnt : 0ull), sa = wave_sum(mine ? la : 0ull), sb = wave_sum(mine ? lb : 0ull);
                if ((int)(threadIdx.x & 63) != leader) return;
                mi_unet_vgraph *const t = graph + (k0 - 1);
                add64(&t->nodes, sc & 255u);
                add64(&t->ends, (sc >> 8) & 255u);
                add64(&t->junction_nodes, (sc >> 16) & 255u);
                add64(&t->isolated, (sc >> 24) & 255u);
                add64(&t->junction_voxels, (sc >> 32) & 255u);
                add64(&t->branches, (sc >> 40) & 255u);
                add64(&t->closed, (sc >> 48) & 255u);
#pragma unroll
                for (int cl = 0; cl < 7; ++cl) add64(&t->links[cl], cl < 5 ? (sa >> (10 * cl)) & 1023u : (sb >> (10 * (cl - 5))) & 1023u);
            });
        }
        // the branch's row
        {
            int row = branch >= 0 && branch < n_branches ? branch : -1;
            peel<64>(row, -1, [&](int r0, bool mine, u64, int leader) {
                const bool vox = mine && c == BRANCH;
                const u64 voxels = __ballot(vox);
                const u64 sa = wave_sum(mine ? la : 0ull), sb = wave_sum(mine ? lb : 0ull);
                u64 sd = 0;
                int dmin = 0x7FFFFFFF, dmax = 0;
                if (r2) {
                    sd = wave_sum(vox ? (u64)d : 0ull);
                    dmin = wave_min(vox ? d : 0x7FFFFFFF);
                    dmax = wave_max(vox ? d : 0);
                }
                if ((int)(threadIdx.x & 63) != leader) return;
                mi_unet_vbranch *const t = branches + r0;
                if (voxels) atomicAdd(&t->voxels, (int)__popcll(voxels));
#pragma unroll
                for (int cl = 0; cl < 7; ++cl) {
                    const int add = (int)(cl < 5 ? (sa >> (10 * cl)) & 1023u : (sb >> (10 * (cl - 5))) & 1023u);
                    if (add) atomicAdd(&t->links[cl], add);
                }
                if (r2 && voxels) {
                    add64(&t->r2_sum, sd);
                    lower(&t->r2_min, dmin);
                    raise(&t->r2_max, dmax);
                }
            });
        }
        // the node's row: the coordinates of at most 64 voxels, 21 bits a sum (a coordinate is below 2^13)
        {
            int row = node >= 0 && node < n_nodes ? node : -1;
            const unsigned x = (unsigned)i % (unsigned)g.W, zy = (unsigned)i / (unsigned)g.W, y = zy % (unsigned)g.H, z = zy / (unsigned)g.H;
            const u64 zyx = (u64)z << 42 | (u64)y << 21 | (u64)x;
            peel<64>(row, -1, [&](int r0, bool mine, u64 mask, int leader) {
                const u64 s = wave_sum(mine ? zyx : 0ull);
                int dmin = 0x7FFFFFFF, dmax = 0;
                if (r2) {
                    dmin = wave_min(mine ? d : 0x7FFFFFFF);
                    dmax = wave_max(mine ? d : 0);
                }
                if ((int)(threadIdx.x & 63) != leader) return;
                mi_unet_vnode *const t = nodes + r0;
                atomicAdd(&t->voxels, (int)__popcll(mask));
                add64(&t->sz, s >> 42);
                add64(&t->sy, (s >> 21) & 0x1FFFFFu);
                add64(&t->sx, s & 0x1FFFFFu);
                if (r2) {
                    lower(&t->r2_min, dmin);
                    raise(&t->r2_max, dmax);
                }
            });
        }
    }
}

__global__ __launch_bounds__(WG) void k_vbr_rows_fix(mi_unet_vbranch *branches, int n_branches)
{
    const int r = blockIdx.x * WG + threadIdx.x;
    if (r < n_branches && branches[r].voxels == 0) branches[r].r2_min = 0;
}

inline bool fits(const VolumeBranchesArgs &a)
{
    return a.D >= 1 && a.H >= 1 && a.W >= 1 && a.D <= SCORE_VOLUME_MAX_SIDE && a.H <= SCORE_VOLUME_MAX_SIDE && a.W <= SCORE_VOLUME_MAX_SIDE &&
           (long long)a.D * a.H * a.W < (1ll << 31) && a.m >= 1 && a.m <= VOLUME_MAX_TABLE && a.prune_voxels >= 0;
}

inline View view_of(int32_t *cur, const VolumeBranchesArgs &a, const Ws &w, const VbrState *state)
{
    return View{ cur, w.list, &state->listed, w.parent, w.nvox, w.att_lo, w.att_hi, w.cls, w.dead, a.D, a.H, a.W };
}

}  // namespace vbr

#define VBR_LAUNCH(kernel, grid, ...)                                                      \
    do {                                                                                   \
        hipLaunchKernelGGL(vbr::kernel, dim3(grid), dim3(vbr::WG), 0, s, __VA_ARGS__);     \
        if (hipError_t e_ = hipGetLastError()) return e_;                                  \
    } while (0)

size_t volume_branches_workspace_bytes(int D, int H, int W) { return vbr::carve(nullptr, D, H, W).total; }

hipError_t launch_volume_branches_begin(int32_t *cur, const VolumeBranchesArgs &a, mi_unet_vgraph *graph, VbrState *state, void *ws, hipStream_t s)
{
    if (!cur || !graph || !state || !ws || !vbr::fits(a)) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    VBR_LAUNCH(k_vbr_clear, (a.m + vbr::WG - 1) / vbr::WG, graph, a.m, state);
    VBR_LAUNCH(k_vbr_init, vbr::blocks(dhw), cur, dhw, a.m);
    return hipSuccess;
}

hipError_t launch_volume_branches_round(int32_t *cur, const VolumeBranchesArgs &a, bool first, VbrState *state, void *ws, hipStream_t s)
{
    if (!cur || !state || !ws || !vbr::fits(a)) return hipErrorInvalidValue;
    const vbr::Ws w = vbr::carve(ws, a.D, a.H, a.W);
    const vbr::View g = vbr::view_of(cur, a, w, state);
    const unsigned grid = vbr::blocks((size_t)a.D * a.H * a.W);     // (over the list, whose length only the device knows)
    if (hipError_t e = hipMemsetAsync(&state->spurs, 0, sizeof(unsigned), s)) return e;
    if (first) {
        const int tx = (a.W + vbr::TX - 1) / vbr::TX, ty = (a.H + vbr::TY - 1) / vbr::TY, nt = tx * ty * ((a.D + vbr::TZ - 1) / vbr::TZ);
        VBR_LAUNCH(k_vbr_classify, (unsigned)((nt + VTX_TILES_PER_WG - 1) / VTX_TILES_PER_WG), g, tx, ty, nt, w.list, &state->listed);
    } else {
        VBR_LAUNCH(k_vbr_regather, grid, g);
    }
    VBR_LAUNCH(k_vbr_link, grid, g);
    VBR_LAUNCH(k_vbr_flatten, grid, g);
    VBR_LAUNCH(k_vbr_attach, grid, g);
    VBR_LAUNCH(k_vbr_mark, grid, g, a.prune_voxels, &state->spurs);
    return hipSuccess;
}

hipError_t launch_volume_branches_delete(int32_t *cur, const VolumeBranchesArgs &a, mi_unet_vgraph *graph, VbrState *state, void *ws, hipStream_t s)
{
    if (!cur || !graph || !state || !ws || !vbr::fits(a)) return hipErrorInvalidValue;
    const vbr::Ws w = vbr::carve(ws, a.D, a.H, a.W);
    VBR_LAUNCH(k_vbr_delete, vbr::blocks((size_t)a.D * a.H * a.W), vbr::view_of(cur, a, w, state), graph);
    return hipSuccess;
}

hipError_t launch_volume_branches_number(int32_t *cur, const VolumeBranchesArgs &a, VbrState *state, void *ws, hipStream_t s)
{
    if (!cur || !state || !ws || !vbr::fits(a)) return hipErrorInvalidValue;
    const vbr::Ws w = vbr::carve(ws, a.D, a.H, a.W);
    if (hipError_t e = hipMemsetAsync(w.node_bits, 0, 2 * w.words * sizeof(uint32_t), s)) return e;
    VBR_LAUNCH(k_vbr_flags, vbr::blocks((size_t)a.D * a.H * a.W), vbr::view_of(cur, a, w, state), w.node_bits, w.branch_bits);
    VBR_LAUNCH(k_vbr_scan_chunks, (unsigned)w.supers, (const uint32_t *)w.node_bits, (const uint32_t *)w.branch_bits, (unsigned)w.chunks, w.chunk_base,
               w.super_total);
    VBR_LAUNCH(k_vbr_scan_supers, 1, (const int2 *)w.super_total, (unsigned)w.supers, w.super_base, state);
    return hipSuccess;
}

hipError_t launch_volume_branches_rows(int32_t *cur, const int32_t *r2, const VolumeBranchesArgs &a, mi_unet_vnode *nodes, int n_nodes,
                                       mi_unet_vbranch *branches, int n_branches, mi_unet_vgraph *graph, int32_t *map, VbrState *state, void *ws,
                                       hipStream_t s)
{
    if (!cur || !graph || !state || !ws || !vbr::fits(a) || n_nodes < 0 || n_branches < 0 || (n_nodes && !nodes) || (n_branches && !branches))
        return hipErrorInvalidValue;
    const vbr::Ws w = vbr::carve(ws, a.D, a.H, a.W);
    const size_t dhw = (size_t)a.D * a.H * a.W;
    if (map)
        if (hipError_t e = hipMemsetAsync(map, 0, dhw * sizeof(int32_t), s)) return e;
    const int rows = std::max(n_nodes, n_branches);
    if (rows) VBR_LAUNCH(k_vbr_rows_clear, (rows + vbr::WG - 1) / vbr::WG, nodes, n_nodes, branches, n_branches, (int)(r2 != nullptr));
    const vbr::Ranks rk{ w.node_bits, w.branch_bits, w.chunk_base, w.super_base };
    VBR_LAUNCH(k_vbr_rows, vbr::blocks(dhw), vbr::view_of(cur, a, w, state), rk, r2, nodes, n_nodes, branches, n_branches, graph, map);
    if (n_branches && r2) VBR_LAUNCH(k_vbr_rows_fix, (n_branches + vbr::WG - 1) / vbr::WG, branches, n_branches);
    return hipSuccess;
}

#undef VBR_LAUNCH

}  // namespace miunet
