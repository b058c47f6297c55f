// volume_match.hip -- the contingency table of two labelled stacks and what is read off it (include/mi_unet.h: mi_unet_volume_match;
// DESIGN.md 7.14).  k_vmt_count, the hot path: a lane per voxel, the wave reduces per distinct key a (mt + 1) + b and carries the
// counts of a few keys until they are displaced (wave.h's peel, written out, with four slots).  k_vmt_rows, k_vmt_cols and k_vmt_cols_end: the
// side tables of the pred and of the truth components.  k_vmt_scan: the exclusive prefix of the rows' pair counts.  k_vmt_pairs: every
// pair at its final position.  Every result is an integer sum or maximum, so nothing depends on the order in which atomics arrive; no
// workgroup waits for another.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "kernels.h"
#include "wave.h"

namespace miunet {

namespace vmt {

using namespace wave;

constexpr unsigned WG = 256;                // lanes per workgroup
constexpr int RUN = 16;                     // 64-voxel segments of one span of a wave's walk
constexpr int GROUPS = 4;                   // distinct keys of a segment that are reduced across the wave; lanes beyond them add their own
constexpr int SLOTS = 4;                    // keys a wave of k_vmt_count carries at once (a power of two)
constexpr unsigned MAX_WGS = 2048;          // workgroups of k_vmt_count: eight a CU on 256 CUs, whatever the volume's size
constexpr int COL_ROWS = 64;                // rows of the table one workgroup of k_vmt_cols walks
constexpr int SCAN_PER_LANE = (MI_UNET_VOLUME_MAX_TABLE + (int)WG - 1) / (int)WG;      // rows one lane of k_vmt_scan sums

// the largest count wins, among equal counts the smallest index: one order-free maximum (DESIGN.md 7.13's key)
__device__ __forceinline__ u64 best_key(int count, int index) { return ((u64)(unsigned)count << 32) | (u64)(~(unsigned)index); }

__device__ __forceinline__ void store_side(::mi_unet_vmatch_side *o, int voxels, int none, int partners, u64 key)
{
    o->voxels = voxels;
    o->covered = voxels - none;
    o->partners = partners;
    o->best = key ? (int)(~(unsigned)key) + 1 : 0;
    o->best_voxels = (int)(key >> 32);
}

// ---- count: one lane per voxel, consecutive lanes along x ----------------------------------------------------------------------------------
// A wave walks spans of RUN 64-voxel segments, span after span at the stride of the grid.  Per segment it takes up to GROUPS distinct
// keys, each by ballot and popcount, and adds the count to the key's slot: it carries SLOTS keys at once, from segment to segment and
// from span to span, and a key that finds no slot takes the one whose turn it is, whose count goes out as one atomic; the walk's end
// sends the rest.  One slot is what k_vol_stats carries; a row through a lesion alternates between "pred only", "both" and "truth only", and
// with one slot every change sent an atomic to one of a handful of hot cells (docs/EXPERIMENTS.md R5.11: 282 -> 124 us on the bench's
// blobs).  A segment without a key changes nothing, so keys are carried across background.  Lanes whose key is none of the segment's
// first GROUPS add their own voxel.  (Four voxels per lane from one 16-byte load was measured too and is slower.)
__global__ __launch_bounds__(256) void k_vmt_count(const int32_t *__restrict__ pred, const int32_t *__restrict__ truth, unsigned dhw, int mp,
                                                   int mt, int32_t *table)
{
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (WG / 64);
    int ck[SLOTS], cc[SLOTS], next = 0;                         // (wave-uniform) the keys carried and their counts; key 0 is an empty slot
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) ck[sl] = cc[sl] = 0;
    for (u64 span = ((u64)blockIdx.x * WG + threadIdx.x) >> 6; span * (64ull * RUN) < (u64)dhw; span += waves) {
        const u64 first = span * (64ull * RUN);
        for (int sg = 0; sg < RUN; ++sg) {
            if (first + 64ull * sg >= (u64)dhw) break;          // (wave-uniform)
            const u64 i = first + 64ull * sg + lane;
            int k = 0;
            if (i < (u64)dhw) {
                const int a = pred[i], b = truth[i];
                k = (a >= 1 && a <= mp ? a : 0) * (mt + 1) + (b >= 1 && b <= mt ? b : 0);     // (< 4097^2)
            }
            // (wave.h's peel<GROUPS>, written out: with the four slots as the loop's body the compiler turns a select of the peel form into
            // a branch, and the bench's noise case measured 6 % slower; docs/EXPERIMENTS.md R5.19)
            u64 todo = __ballot(k != 0);
            for (int g = 0; g < GROUPS && todo; ++g) {          // (wave-uniform)
                const int k0 = __shfl(k, __builtin_ctzll(todo), 64);
                const bool mine = k == k0;
                const u64 mm = __ballot(mine);
                const int n = __popcll(mm);
                bool hit = false;
#pragma unroll
                for (int sl = 0; sl < SLOTS; ++sl)
                    if (ck[sl] == k0) {
                        cc[sl] += n;
                        hit = true;
                    }
                if (!hit) {                                     // the slots in turn: the one whose turn it is goes out
#pragma unroll
                    for (int sl = 0; sl < SLOTS; ++sl)
                        if (sl == next) {
                            if (ck[sl] && lane == 0) atomicAdd(table + ck[sl], cc[sl]);
                            ck[sl] = k0;
                            cc[sl] = n;
                        }
                    next = (next + 1) & (SLOTS - 1);
                }
                todo &= ~mm;
                if (mine) k = 0;
            }
            if (k) atomicAdd(table + k, 1);                     // a segment of many small components: the lane adds its own voxel
        }
    }
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl)
        if (ck[sl] && lane == sl) atomicAdd(table + ck[sl], cc[sl]);
}

// ---- rows: a wave per pred component, lanes along the row ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vmt_rows(const int32_t *__restrict__ table, int mp, int mt, ::mi_unet_vmatch_side *__restrict__ side,
                                                  int32_t *__restrict__ row_pairs)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)((blockIdx.x * WG + threadIdx.x) >> 6);
    if (r >= mp) return;                                        // (wave-uniform)
    const int32_t *const row = table + (size_t)(r + 1) * (size_t)(mt + 1);
    int voxels = 0, partners = 0;
    u64 key = 0;
    for (int b = lane; b <= mt; b += 64) {
        const int v = row[b];
        voxels += v;
        if (b >= 1 && v > 0) {
            ++partners;
            const u64 k = best_key(v, b - 1);
            key = k > key ? k : key;
        }
    }
    const int none = __shfl(lane == 0 ? row[0] : 0, 0, 64);
    voxels = wave_sum(voxels);
    partners = wave_sum(partners);
    key = wave_max(key);
    if (lane == 0) {
        store_side(side + r, voxels, none, partners, key);
        row_pairs[r] = partners;
    }
}

// ---- columns: a lane per truth component walking rows, so a wave's reads stay coalesced ------------------------------------------------------
// blockIdx.y takes COL_ROWS rows of the table, so that a table of 4097 rows is spread over the device, not walked by 64 waves; the parts
// meet in three integer atomics per column and part (none where the part of the column is empty), and k_vmt_cols_end writes the entry.
__global__ __launch_bounds__(64) void k_vmt_cols(const int32_t *__restrict__ table, int mp, int mt, int32_t *acc_voxels, int32_t *acc_partners,
                                                 u64 *acc_key)
{
    const int c = (int)(blockIdx.x * 64 + threadIdx.x);
    if (c >= mt) return;
    const int a0 = (int)blockIdx.y * COL_ROWS, a1 = min(a0 + COL_ROWS, mp + 1);
    const int32_t *col = table + (c + 1);
    int voxels = 0, partners = 0;
    u64 key = 0;
#pragma unroll 8
    for (int a = a0; a < a1; ++a) {
        const int v = col[(size_t)a * (size_t)(mt + 1)];
        voxels += v;
        if (a >= 1 && v > 0) {
            ++partners;
            const u64 k = best_key(v, a - 1);
            key = k > key ? k : key;
        }
    }
    if (voxels) atomicAdd(acc_voxels + c, voxels);
    if (partners) {
        atomicAdd(acc_partners + c, partners);
        atomicMax(acc_key + c, key);
    }
}

__global__ __launch_bounds__(64) void k_vmt_cols_end(const int32_t *__restrict__ table, int mt, const int32_t *__restrict__ acc_voxels,
                                                     const int32_t *__restrict__ acc_partners, const u64 *__restrict__ acc_key,
                                                     ::mi_unet_vmatch_side *__restrict__ side)
{
    const int c = (int)(blockIdx.x * 64 + threadIdx.x);
    if (c >= mt) return;
    store_side(side + c, acc_voxels[c], table[c + 1], acc_partners[c], acc_key[c]);
}

// ---- scan: the exclusive prefix of at most MI_UNET_VOLUME_MAX_TABLE row counts, one workgroup ------------------------------------------------
__global__ __launch_bounds__(256) void k_vmt_scan(const int32_t *__restrict__ row_pairs, int mp, int32_t *__restrict__ row_first,
                                                  int32_t *__restrict__ found)
{
    __shared__ int s_sum[WG];
    const int t = threadIdx.x, r0 = t * SCAN_PER_LANE;
    int own = 0;
    for (int j = 0; j < SCAN_PER_LANE; ++j)
        if (r0 + j < mp) own += row_pairs[r0 + j];
    s_sum[t] = own;
    __syncthreads();
    for (int o = 1; o < (int)WG; o <<= 1) {                     // inclusive scan over the lanes' sums
        const int v = t >= o ? s_sum[t - o] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    int at = s_sum[t] - own;
    for (int j = 0; j < SCAN_PER_LANE; ++j)
        if (r0 + j < mp) {
            row_first[r0 + j] = at;
            at += row_pairs[r0 + j];
        }
    if (t == (int)WG - 1) *found = s_sum[t];
}

// ---- pairs: a wave per row writes the row's pairs behind row_first, t ascending --------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vmt_pairs(const int32_t *__restrict__ table, int mp, int mt, const int32_t *__restrict__ row_first,
                                                   ::mi_unet_vmatch_pair *__restrict__ pairs, int keep_pairs)
{
    const int lane = threadIdx.x & 63;
    const int r = (int)((blockIdx.x * WG + threadIdx.x) >> 6);
    if (r >= mp) return;                                        // (wave-uniform)
    const int32_t *const row = table + (size_t)(r + 1) * (size_t)(mt + 1);
    int at = row_first[r];
    for (int b0 = 1; b0 <= mt && at < keep_pairs; b0 += 64) {   // (wave-uniform)
        const int b = b0 + lane;
        const int v = b <= mt ? row[b] : 0;
        const u64 mm = __ballot(v > 0);
        const int slot = at + __popcll(mm & lanes_below());
        if (v > 0 && slot < keep_pairs) {
            pairs[slot].p = r;
            pairs[slot].t = b - 1;
            pairs[slot].voxels = v;
        }
        at += __popcll(mm);
    }
}

bool fits(const VolumeMatchArgs &a)
{
    if (a.D < 1 || a.H < 1 || a.W < 1 || a.mp < 1 || a.mt < 1 || a.mp > MI_UNET_VOLUME_MAX_TABLE || a.mt > MI_UNET_VOLUME_MAX_TABLE) return false;
    return (long long)a.D * a.H < (1LL << 31) && (long long)a.D * a.H * a.W < (1LL << 31);
}

}  // namespace vmt

hipError_t launch_volume_match_count(const int32_t *pred, const int32_t *truth, const VolumeMatchArgs &a, int32_t *table, hipStream_t s)
{
    if (!pred || !truth || !table || !vmt::fits(a)) return hipErrorInvalidValue;
    const unsigned dhw = (unsigned)a.D * (unsigned)a.H * (unsigned)a.W;
    if (hipError_t e = hipMemsetAsync(table, 0, (size_t)(a.mp + 1) * (size_t)(a.mt + 1) * sizeof(int32_t), s)) return e;
    const unsigned spans = (dhw + 64u * vmt::RUN - 1) / (64u * vmt::RUN);
    const unsigned wgs = (spans + 3) / 4;
    hipLaunchKernelGGL(vmt::k_vmt_count, dim3(wgs < vmt::MAX_WGS ? wgs : vmt::MAX_WGS), dim3(vmt::WG), 0, s, pred, truth, dhw, a.mp, a.mt, table);
    return hipGetLastError();
}

hipError_t launch_volume_match_tables(const int32_t *table, const VolumeMatchArgs &a, ::mi_unet_vmatch_side *pred_side,
                                      ::mi_unet_vmatch_side *truth_side, int32_t *row_pairs, int32_t *row_first, int32_t *found,
                                      void *col_acc, ::mi_unet_vmatch_pair *pairs, int keep_pairs, hipStream_t s)
{
    if (!table || !pred_side || !truth_side || !row_pairs || !row_first || !found || !col_acc || !pairs || keep_pairs < 1 || !vmt::fits(a))
        return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(col_acc, 0, (size_t)a.mt * VMT_COL_ACC_BYTES, s)) return e;
    vmt::u64 *const acc_key = static_cast<vmt::u64 *>(col_acc);                 // [mt] keys, then [mt] voxels, then [mt] partners
    int32_t *const acc_voxels = reinterpret_cast<int32_t *>(acc_key + a.mt), *const acc_partners = acc_voxels + a.mt;
    const unsigned col_wgs = ((unsigned)a.mt + 63) / 64;
    const unsigned row_wgs = ((unsigned)a.mp + 3) / 4;          // a wave per row, four waves a workgroup
    hipLaunchKernelGGL(vmt::k_vmt_rows, dim3(row_wgs), dim3(vmt::WG), 0, s, table, a.mp, a.mt, pred_side, row_pairs);
    hipLaunchKernelGGL(vmt::k_vmt_cols, dim3(col_wgs, ((unsigned)a.mp + vmt::COL_ROWS) / vmt::COL_ROWS), dim3(64), 0, s, table, a.mp, a.mt,
                       acc_voxels, acc_partners, acc_key);
    hipLaunchKernelGGL(vmt::k_vmt_cols_end, dim3(col_wgs), dim3(64), 0, s, table, a.mt, acc_voxels, acc_partners, acc_key, truth_side);
    hipLaunchKernelGGL(vmt::k_vmt_scan, dim3(1), dim3(vmt::WG), 0, s, row_pairs, a.mp, row_first, found);
    hipLaunchKernelGGL(vmt::k_vmt_pairs, dim3(row_wgs), dim3(vmt::WG), 0, s, table, a.mp, a.mt, row_first, pairs, keep_pairs);
    return hipGetLastError();
}

}  // namespace miunet
