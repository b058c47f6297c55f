// volume.hip -- a stack of masks labelled as one volume, per value plane: 6 / 18 / 26-connected components with their voxel counts,
// bounding boxes, face counts and coordinate sums, the size filter and the ordered table (include/mi_unet.h:
// mi_unet_volume_components).  Byte and integer work, exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "cc_common.h"
#include "kernel_common.h"
#include "wave.h"

namespace miunet {

namespace vl {

using namespace wave;

constexpr int NO_SLOT = -1;
constexpr int RUN = 16;                                  // 64-voxel segments a wave of k_vol_stats carries a root over (cc_stats' CC_RUN)
constexpr int RADIX_BITS = 11, RADIX_BINS = 1 << RADIX_BITS, RADIX_PASSES = 6;      // 6 x 11 = 66 bits cover the 62-bit key
constexpr int LIST_BLOCKS = 1024;                        // most workgroups per plane in the pass over the slots

typedef VolumeRankAcc PlaneAcc;       // (kernels.h) the accumulators of one plane, zeroed on the stream before the first kernel

// A plane has at most ceil(D H W / 2) components under every connectivity: one voxel of each is an independent set of the grid graph,
// which has a Hamiltonian path (the serpentine), and an independent set takes at most every other vertex of a path.
__host__ __device__ inline size_t slots_per_plane(size_t dhw) { return (dhw + 1) / 2; }

struct Ws {
    PlaneAcc *acc;                  // [n]
    int *parent;                    // [N] the forest; flattened by k_vol_stats; -1 outside the set
    int *slot;                      // [N] valid at roots: the root's slot in its plane
    mi_unet_vcomp *stat;            // [n][S] per slot, in the layout of the table
    unsigned long long *key;        // [n][S] (voxels << 31) | (2^31 - 1 - first)
    int *tidx;                      // [n][S] 1 + the table index of the slot's component, 0 when it is not in the table
    size_t total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline Ws carve(void *base, size_t dhw, int n)
{
    const size_t N = dhw * n, S = slots_per_plane(dhw) * n;
    uint8_t *p = static_cast<uint8_t *>(base);
    Ws w;
    size_t at = 0;
    w.acc = reinterpret_cast<PlaneAcc *>(p + at); at += up256((size_t)n * sizeof(PlaneAcc));
    w.parent = reinterpret_cast<int *>(p + at); at += up256(N * sizeof(int));
    w.slot = reinterpret_cast<int *>(p + at); at += up256(N * sizeof(int));
    w.stat = reinterpret_cast<mi_unet_vcomp *>(p + at); at += up256(S * sizeof(mi_unet_vcomp));
    w.key = reinterpret_cast<unsigned long long *>(p + at); at += up256(S * sizeof(unsigned long long));
    w.tidx = reinterpret_cast<int *>(p + at); at += up256(S * sizeof(int));
    w.total = at;
    return w;
}

// ---- init: the parent of a set voxel is the first voxel of its run inside the lane's 64-voxel segment -----------------------------------
// (cc_init in three dimensions.)  Voxel i of plane k is i = k * dhw + z * hw + y * W + x; dhw is a multiple of W, so x == 0 marks the
// start of every row, of every slice and of every plane: a run never continues from x = W - 1 into any of them.
__global__ __launch_bounds__(256) void k_vol_init(const uint8_t *__restrict__ masks, VolumeArgs a, unsigned dhw, int *parent, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const bool in = i < N;
    const unsigned k = in ? i / dhw : 0u, src = in ? i - k * dhw : 0u;
    const bool f = in && masks[src] == pick_value(a.v, (int)k);
    const unsigned x = src % (unsigned)a.W;
    const int lane = threadIdx.x & 63;
    const unsigned long long fm = __ballot(f);
    const unsigned long long prev = (fm << 1) & ~__ballot(x == 0);
    const unsigned long long starts = fm & ~prev;
    if (in) {
        int p = -1;
        if (f) {
            const unsigned long long below = starts & ((2ull << lane) - 1ull);
            p = (int)i - (lane - (63 - __builtin_clzll(below)));
        }
        parent[i] = p;
    }
}

// ---- merge: unions with the earlier neighbours ------------------------------------------------------------------------------------------
// AXES = 1, 2, 3 for connectivity 6, 18, 26: a pair is adjacent when it differs on at most AXES axes.  Of the 13 neighbours before a
// voxel in raster order -- 4 in its slice, 9 in the slice above -- the voxel unites with those the connectivity allows, EXCEPT where
// other unions already make the connection:
//   x      the left neighbour is in the voxel's run (k_vol_init) unless the run was cut at a 64-lane boundary: lane 0 unites there.
//   y, z   the face neighbour above (in y, or in z) is skipped when the left neighbour and ITS face neighbour above are set too
//          (cc_merge's `l && ul`).  Along a row, take the stretch to the left over which the voxel and the one above it are both set:
//          its leftmost voxel fails the test and unites, and both rows are joined along x up to here.
//   edges, corners   a diagonal neighbour q (2 or 3 axes differ) is skipped when any voxel of the box spanned by the two, other than
//          themselves, is set: that voxel m differs from each of them on fewer axes, so (p, m) and (m, q) are adjacent under the same
//          connectivity and are connected by induction on the number of differing axes (whichever of the two comes later in
//          raster order makes or inherits the connection; faces are the base case above).
// Every union is pp::unite; its loop ends by its own data.
__host__ __device__ constexpr int nb_bit(int dz, int dy, int dx) { return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }

template <int AXES>
__global__ __launch_bounds__(256) void k_vol_merge(const uint8_t *__restrict__ masks, VolumeArgs a, unsigned dhw, int *parent, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const unsigned k = i / dhw, src = i - k * dhw;
    const int v = pick_value(a.v, (int)k);
    if (masks[src] != v) return;
    const int W = a.W, H = a.H, hw = H * W;
    const int z = (int)(src / (unsigned)hw), rem = (int)(src - (unsigned)z * (unsigned)hw), y = rem / W, x = rem - y * W;
    const uint8_t *const m = masks + src;
    // the set bits of the slice above and of this slice around the voxel, as far as the rules below look
    unsigned nb = 0;
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int axes = (dz != 0) + (dy != 0) + (dx != 0);
                if (axes == 0 || axes > (AXES < 2 ? 2 : AXES)) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                if (m[dz * hw + dy * W + dx] == v) nb |= 1u << nb_bit(dz, dy, dx);
            }
    auto set = [&](int dz, int dy, int dx) { return (nb >> nb_bit(dz, dy, dx)) & 1u; };
    const int gi = (int)i;
    const bool l = set(0, 0, -1);
    if (l && (threadIdx.x & 63) == 0) pp::unite(parent, gi, gi - 1);
    if (set(0, -1, 0) && !(l && set(0, -1, -1))) pp::unite(parent, gi, gi - W);
    if (set(-1, 0, 0) && !(l && set(-1, 0, -1))) pp::unite(parent, gi, gi - hw);
    if constexpr (AXES >= 2) {
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int axes = (dz != 0) + (dy != 0) + (dx != 0);
                    const bool earlier = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
                    if (!earlier || axes < 2 || axes > AXES) continue;
                    if (!set(dz, dy, dx)) continue;
                    bool bridged = false;
#pragma unroll
                    for (int sel = 1; sel < 7; ++sel) {         // the other voxels of the box: every proper, non-empty choice of the axes
                        const int ez = (sel & 4) ? dz : 0, ey = (sel & 2) ? dy : 0, ex = (sel & 1) ? dx : 0;
                        const bool self = ez == 0 && ey == 0 && ex == 0, other = ez == dz && ey == dy && ex == dx;
                        if (self || other) continue;
                        bridged = bridged || set(ez, ey, ex);
                    }
                    if (!bridged) pp::unite(parent, gi, gi + dz * hw + dy * W + dx);
                }
    }
}

// ---- roots: a slot for every root ---------------------------------------------------------------------------------------------------------
// A root takes the next slot of its plane and clears it.  parents only decrease, so the root of a component is its raster-first voxel:
// `first` is known here.  The lanes of a wave that are roots of one plane send ONE add to the plane's cursor.
__global__ __launch_bounds__(256) void k_vol_roots(const int *__restrict__ parent, VolumeArgs a, unsigned dhw, unsigned S, PlaneAcc *acc,
                                                   int *slot, mi_unet_vcomp *stat, int *tidx, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const bool root = i < N && parent[i] == (int)i;
    unsigned k = root ? i / dhw : 0xFFFFFFFFu;
    unsigned s = 0;
    peel<64>(k, 0xFFFFFFFFu, [&](unsigned k0, bool mine, u64 mk, int leader) {
        const unsigned slot_k0 = wave_take(&acc[k0].nroots, mk, leader);
        if (mine) s = slot_k0;
    });
    if (!root) return;
    if (s >= S) { slot[i] = NO_SLOT; acc[k].overflow = 1u; return; }
    slot[i] = (int)s;
    mi_unet_vcomp c;
    c.voxels = 0; c.first = (int)(i - k * dhw);
    c.x0 = c.y0 = c.z0 = 0x7FFFFFFF; c.x1 = c.y1 = c.z1 = -1;
    c.kept = 0; c.value = pick_value(a.v, (int)k);
    c.faces_x = c.faces_y = c.faces_z = 0; c.sx = c.sy = c.sz = 0;
    stat[(size_t)k * S + s] = c;
    tidx[(size_t)k * S + s] = 0;
}

// ---- stats: flatten + the statistics of every component -----------------------------------------------------------------------------------
// cc_stats in three dimensions: a volume is a handful of roots and same-address atomics serialise, so a wave reduces per distinct root
// inside a 64-voxel segment and carries that root's sums over RUN consecutive segments; it issues its atomics only when the root
// changes, thirteen of them from thirteen lanes at once.  The sums a wave carries: at most 64 * RUN voxels, 2 faces per voxel and axis.
__global__ __launch_bounds__(256) void k_vol_stats(const uint8_t *__restrict__ masks, VolumeArgs a, unsigned dhw, unsigned S, int *parent,
                                                   const int *__restrict__ slot, mi_unet_vcomp *stat, unsigned N)
{
    const int lane = threadIdx.x & 63;
    const long long first = (((long long)blockIdx.x * 256 + threadIdx.x) >> 6) * (64LL * RUN);
    const int W = a.W, H = a.H, D = a.D, hw = H * W;
    int ar = -1, an = 0, lo[3] = { 0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF }, hi[3] = { -1, -1, -1 }, fc[3] = { 0, 0, 0 };   // (wave-uniform)
    long long sm[3] = { 0, 0, 0 };
    auto flush = [&]() {
        if (ar < 0) return;                                     // (wave-uniform)
        const int s = slot[ar];
        if (s == NO_SLOT) return;
        mi_unet_vcomp *const c = stat + (size_t)((unsigned)ar / dhw) * S + s;
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
        default: break;
        }
    };
    for (int sg = 0; sg < RUN; ++sg) {
        const long long i = first + 64LL * sg + lane;
        if (first + 64LL * sg >= (long long)N) break;           // (wave-uniform)
        int r = -1, co[3] = { 0, 0, 0 }, f[3] = { 0, 0, 0 };
        if (i < (long long)N && parent[i] >= 0) {
            r = pp::find_root_ro(parent, (int)i);
            parent[i] = r;
            const unsigned k = (unsigned)i / dhw, src = (unsigned)i - k * dhw;
            const int v = pick_value(a.v, (int)k);
            const int z = (int)(src / (unsigned)hw), rem = (int)(src - (unsigned)z * (unsigned)hw), y = rem / W, x = rem - y * W;
            const uint8_t *const m = masks + src;
            co[0] = x; co[1] = y; co[2] = z;
            f[0] = !(x > 0 && m[-1] == v) + !(x + 1 < W && m[1] == v);
            f[1] = !(y > 0 && m[-W] == v) + !(y + 1 < H && m[W] == v);
            f[2] = !(z > 0 && m[-hw] == v) + !(z + 1 < D && m[hw] == v);
        }
        peel<64>(r, -1, [&](int r0, bool mine, u64 mm, int) {
            if (r0 != ar) {
                flush();
                ar = r0; an = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) { lo[j] = 0x7FFFFFFF; hi[j] = -1; fc[j] = 0; sm[j] = 0; }
            }
            an += __builtin_popcountll(mm);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lo[j] = min(lo[j], wave_min(mine ? co[j] : 0x7FFFFFFF));
                hi[j] = max(hi[j], wave_max(mine ? co[j] : -1));
                fc[j] += wave_sum(mine ? f[j] : 0);
                sm[j] += wave_sum(mine ? (long long)co[j] : 0LL);
            }
        });
    }
    flush();
}

// ---- keys: the order key of every slot; the roots that pass min_voxels -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vol_keys(VolumeArgs a, unsigned S, PlaneAcc *acc, const mi_unet_vcomp *__restrict__ stat,
                                                  unsigned long long *key)
{
    const unsigned k = blockIdx.y;
    const unsigned found = min(acc[k].nroots, S);
    int pass = 0;
    for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < found; s += gridDim.x * 256u) {
        const mi_unet_vcomp *const c = stat + (size_t)k * S + s;
        const int vox = c->voxels;
        key[(size_t)k * S + s] = ((unsigned long long)(unsigned)vox << 31) | (unsigned long long)(0x7FFFFFFF - c->first);
        pass += vox >= a.min_voxels;
    }
    pass = wave_sum(pass);
    if ((threadIdx.x & 63) == 0 && pass) atomicAdd(&acc[k].n_min, (unsigned)pass);
}

// ---- select: the rank-th largest key of a plane, exactly ----------------------------------------------------------------------------------
// One workgroup per (plane, selection): selection 0 = the keep_largest-th largest key, 1 = the cap-th largest; a selection whose rank
// is not below the plane's count keeps thr == 0 (every key passes).  A radix select from the top, 11 bits a pass: the histogram of the
// pass's digit over the keys that share the prefix found so far (2048 LDS bins; the lanes of a wave that hold the same digit send ONE
// add -- the keys of small components share all their high digits), a scan from the top bin down, the bin that holds the rank.  Six
// linear passes over the plane's keys; keys are unique (`first` is), so the result is the key itself.
__global__ __launch_bounds__(256) void k_vol_select(VolumeArgs a, unsigned S, PlaneAcc *acc, const unsigned long long *__restrict__ key_all)
{
    __shared__ unsigned s_hist[RADIX_BINS];
    __shared__ unsigned s_tot[4], s_rank;
    __shared__ unsigned long long s_prefix;
    const unsigned k = blockIdx.x >> 1, sel = blockIdx.x & 1, t = threadIdx.x;
    const int lane = t & 63;
    const unsigned found = min(acc[k].nroots, S);
    unsigned rank = sel == 0 ? (unsigned)a.keep_largest : (unsigned)a.cap;      // 1-based from the top
    if (rank == 0 || rank >= found) return;                     // (workgroup-uniform)
    const unsigned long long *const key = key_all + (size_t)k * S;
    unsigned long long prefix = 0;
    for (int pass = 0; pass < RADIX_PASSES; ++pass) {
        const int shift = RADIX_BITS * (RADIX_PASSES - 1 - pass);
        for (int b = t; b < RADIX_BINS; b += 256) s_hist[b] = 0;
        __syncthreads();
        for (unsigned base = t & ~63u; base < found; base += 256) {               // (wave-uniform)
            const unsigned s = base + lane;
            unsigned digit = 0xFFFFFFFFu;
            if (s < found) {
                const unsigned long long q = key[s];
                if (pass == 0 || (q >> (shift + RADIX_BITS)) == prefix) digit = (unsigned)(q >> shift) & (RADIX_BINS - 1);
            }
            peel<64>(digit, 0xFFFFFFFFu, [&](unsigned d0, bool, u64 mm, int leader) {
                if (lane == leader) atomicAdd(&s_hist[d0], (unsigned)__builtin_popcountll(mm));
            });
        }
        __syncthreads();
        // lane t owns the bins RADIX_BINS - 1 - (8 t + j), j = 0 .. 7: from the top down
        unsigned c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) c += s_hist[RADIX_BINS - 1 - (8 * t + j)];
        unsigned inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = (unsigned)__shfl_up((int)inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) s_tot[t >> 6] = inc;
        __syncthreads();
        for (unsigned wv = 0; wv < (t >> 6); ++wv) inc += s_tot[wv];
        unsigned exc = inc - c;
        if (exc < rank && rank <= inc) {                        // exactly one lane
            for (int j = 0; j < 8; ++j) {
                const unsigned bin = RADIX_BINS - 1 - (8 * t + j), bc = s_hist[bin];
                if (rank <= exc + bc) { s_prefix = (prefix << RADIX_BITS) | bin; s_rank = rank - exc; break; }
                exc += bc;
            }
        }
        __syncthreads();
        prefix = s_prefix; rank = s_rank;
    }
    if (t == 0) acc[k].thr[sel] = prefix;
}

// ---- table: the selected keys of a plane, sorted by one workgroup in LDS ------------------------------------------------------------------
// The keys >= thr[1] of a plane are its min(found, cap) largest (keys are unique): at most 4096, 32 KiB.  A bitonic sort, descending,
// over the next power of two (0 pads: every real key is >= 2^31).  Entry j: its key names the component's first voxel, that is its
// root, whose slot holds the statistics.  Also here: the plane's counts.
__global__ __launch_bounds__(256) void k_vol_table(VolumeArgs a, unsigned dhw, unsigned S, const PlaneAcc *acc,
                                                   const unsigned long long *__restrict__ key_all, const int *__restrict__ slot,
                                                   const mi_unet_vcomp *__restrict__ stat, int *tidx, mi_unet_vcomp *table, int32_t *counts)
{
    __shared__ unsigned long long s_key[VOLUME_MAX_TABLE];
    __shared__ unsigned s_n;
    const unsigned k = blockIdx.x, t = threadIdx.x;
    const PlaneAcc pa = acc[k];
    const unsigned found = min(pa.nroots, S);
    if (t == 0) {
        counts[k] = pa.overflow ? -1 : (int)found;
        counts[a.n + k] = (int)(a.keep_largest > 0 ? min(pa.n_min, (unsigned)a.keep_largest) : pa.n_min);
        s_n = 0;
    }
    __syncthreads();
    const unsigned long long *const key = key_all + (size_t)k * S;
    for (unsigned s = t; s < found; s += 256) {
        const unsigned long long q = key[s];
        if (q >= pa.thr[1]) {
            const unsigned pos = atomicAdd(&s_n, 1u);
            if (pos < (unsigned)VOLUME_MAX_TABLE) s_key[pos] = q;
        }
    }
    __syncthreads();
    const unsigned m = min(s_n, (unsigned)a.cap);
    unsigned P = 2;
    while (P < m) P <<= 1;
    for (unsigned j = m + t; j < P; j += 256) s_key[j] = 0;
    __syncthreads();
    for (unsigned kk = 2; kk <= P; kk <<= 1)
        for (unsigned j = kk >> 1; j > 0; j >>= 1) {
            for (unsigned idx = t; idx < P; idx += 256) {
                const unsigned other = idx ^ j;
                if (other > idx) {
                    const unsigned long long x = s_key[idx], y = s_key[other];
                    const bool desc = (idx & kk) == 0;
                    if (desc ? x < y : x > y) { s_key[idx] = y; s_key[other] = x; }
                }
            }
            __syncthreads();
        }
    for (unsigned j = t; j < m; j += 256) {
        const unsigned long long q = s_key[j];
        const unsigned first = 0x7FFFFFFFu - (unsigned)(q & 0x7FFFFFFFull);
        const int s = slot[(size_t)k * dhw + first];
        if (s == NO_SLOT) continue;                             // (only behind an overflow, which fails the call)
        mi_unet_vcomp c = stat[(size_t)k * S + s];
        c.kept = (c.voxels >= a.min_voxels && q >= pa.thr[0]) ? 1 : 0;
        table[(size_t)k * a.cap + j] = c;
        tidx[(size_t)k * S + s] = (int)j + 1;
    }
}

// ---- write: out and ids in one pass ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vol_write(VolumeArgs a, unsigned dhw, unsigned S, const PlaneAcc *__restrict__ acc,
                                                   const int *__restrict__ parent, const int *__restrict__ slot,
                                                   const unsigned long long *__restrict__ key, const int *__restrict__ tidx, uint8_t *out,
                                                   int32_t *ids, unsigned N)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const int r = parent[i];
    int o = 0, id = 0;
    if (r >= 0) {
        const unsigned k = (unsigned)r / dhw;
        const int s = slot[r];
        if (s != NO_SLOT) {
            const unsigned long long q = key[(size_t)k * S + s];
            if ((long long)(q >> 31) >= (long long)a.min_voxels && q >= acc[k].thr[0]) {
                o = pick_value(a.v, (int)k);
                const int ti = tidx[(size_t)k * S + s];
                id = ti ? ti : -1;
            }
        }
    }
    out[i] = (uint8_t)o;
    if (ids) ids[i] = id;
}

}  // namespace vl

size_t volume_slots_per_plane(size_t dhw) { return vl::slots_per_plane(dhw); }

hipError_t launch_volume_select(const VolumeArgs &a, unsigned S, VolumeRankAcc *acc, const unsigned long long *key, hipStream_t s)
{
    hipLaunchKernelGGL(vl::k_vol_select, dim3(2u * a.n), dim3(256), 0, s, a, S, acc, key);
    return hipGetLastError();
}

size_t volume_workspace_bytes(int D, int H, int W, int n) { return vl::carve(nullptr, (size_t)D * H * W, n).total; }

hipError_t launch_volume_components(const uint8_t *masks, const VolumeArgs &a, uint8_t *out, int32_t *ids, mi_unet_vcomp *table,
                                    int32_t *counts, void *ws, hipStream_t s)
{
    if (!masks || !out || !table || !counts || !ws || a.D < 1 || a.H < 1 || a.W < 1 || a.n < 1 || a.n > VOLUME_MAX_VALUES)
        return hipErrorInvalidValue;
    if (a.cap < 1 || a.cap > VOLUME_MAX_TABLE || a.min_voxels < 0 || a.keep_largest < 0) return hipErrorInvalidValue;
    if (a.connectivity != 6 && a.connectivity != 18 && a.connectivity != 26) return hipErrorInvalidValue;
    const unsigned long long dhw64 = (unsigned long long)a.D * a.H * a.W, N64 = dhw64 * a.n;
    if ((unsigned long long)a.D * a.H > 0x7FFFFFFFull || N64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)dhw64, N = (unsigned)N64, S = (unsigned)vl::slots_per_plane(dhw);
    const vl::Ws w = vl::carve(ws, dhw, a.n);
    if (hipError_t e = hipMemsetAsync(w.acc, 0, (size_t)a.n * sizeof(vl::PlaneAcc), s)) return e;
    if (hipError_t e = hipMemsetAsync(table, 0, (size_t)a.n * a.cap * sizeof(mi_unet_vcomp), s)) return e;
    const dim3 g((N + 255u) / 256u), blk(256);
    hipLaunchKernelGGL(vl::k_vol_init, g, blk, 0, s, masks, a, dhw, w.parent, N);
    if (a.connectivity == 6) hipLaunchKernelGGL(vl::k_vol_merge<1>, g, blk, 0, s, masks, a, dhw, w.parent, N);
    else if (a.connectivity == 18) hipLaunchKernelGGL(vl::k_vol_merge<2>, g, blk, 0, s, masks, a, dhw, w.parent, N);
    else hipLaunchKernelGGL(vl::k_vol_merge<3>, g, blk, 0, s, masks, a, dhw, w.parent, N);
    hipLaunchKernelGGL(vl::k_vol_roots, g, blk, 0, s, w.parent, a, dhw, S, w.acc, w.slot, w.stat, w.tidx, N);
    const unsigned sblocks = (unsigned)(((unsigned long long)N + 256ull * vl::RUN - 1) / (256ull * vl::RUN));
    hipLaunchKernelGGL(vl::k_vol_stats, dim3(sblocks), blk, 0, s, masks, a, dhw, S, w.parent, w.slot, w.stat, N);
    unsigned lblocks = (S + 255u) / 256u;
    if (lblocks > (unsigned)vl::LIST_BLOCKS) lblocks = vl::LIST_BLOCKS;
    hipLaunchKernelGGL(vl::k_vol_keys, dim3(lblocks, (unsigned)a.n), blk, 0, s, a, S, w.acc, w.stat, w.key);
    hipLaunchKernelGGL(vl::k_vol_select, dim3(2u * a.n), blk, 0, s, a, S, w.acc, w.key);
    hipLaunchKernelGGL(vl::k_vol_table, dim3((unsigned)a.n), blk, 0, s, a, dhw, S, w.acc, w.key, w.slot, w.stat, w.tidx, table, counts);
    hipLaunchKernelGGL(vl::k_vol_write, g, blk, 0, s, a, dhw, S, w.acc, w.parent, w.slot, w.key, w.tidx, out, ids, N);
    return hipGetLastError();
}

}  // namespace miunet
