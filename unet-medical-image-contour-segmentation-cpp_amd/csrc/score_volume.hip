// score_volume.hip -- a stack of predicted masks against a stack of ground truth as ONE volume, per value plane: overlap counts, the
// confusion matrix, and the exact squared distances between the two 3-D boundaries under an anisotropic integer spacing, with their
// maximum, sums and order statistics (include/mi_unet.h: mi_unet_score_volume).  A separable exact distance transform
// in three passes -- along z, along y, along x -- evaluated only where a source boundary voxel will read it.  The counts, the radix
// select and the final step are score.hip's (score_common.h).  Byte and integer work, exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "score_common.h"

namespace miunet {

namespace sv {

using sc::ScoreAcc;
using sc::SENT;                                         // g of a column without a boundary voxel (real index distances are <= 8191)
constexpr unsigned F_INF = 0xFFFFFFFFu;                 // f of a voxel whose (z, x) line holds no finite g: above every d2 (< 2^31) and every sum of two terms
constexpr int MAX_ITEMS = 1 << 20;                      // workgroups of a launch at most; every kernel walks its items with a grid stride

struct Ws {
    ScoreAcc *acc;                  // [P]
    unsigned long long *conf;       // [classes * classes], then skipped
    unsigned *hist;                 // [P][5][65536]
    uint8_t *rows;                  // [P][2][D * H]: 1 where row (z, y) of the set holds boundary voxels
    size_t zero_bytes;              // the four above are one run from acc
    uint16_t *g;                    // [P][2][D * H * W]: index distance along z to the nearest boundary voxel of the (y, x) column
    unsigned *f;                    // [P][2][D * H * W]: min over y' of (g * uz)^2 + ((y - y') * uy)^2, in the rows the other set's sources read
    int *d2;                        // [P][2][D * H * W]: the direction's values, cursor[] of them, in no particular order
    size_t total;
};

inline Ws carve(void *base, int D, int H, int W, int n, int classes)
{
    const size_t P = (size_t)n, dhw = (size_t)D * H * W;
    uint8_t *p = static_cast<uint8_t *>(base);
    Ws w;
    size_t at = 0;
    w.acc = reinterpret_cast<ScoreAcc *>(p + at); at += sc::up256(P * sizeof(ScoreAcc));
    w.conf = reinterpret_cast<unsigned long long *>(p + at); at += sc::up256((size_t)(classes * classes + 1) * 8);
    w.hist = reinterpret_cast<unsigned *>(p + at); at += P * sc::HIST_BYTES_PER_PLANE;
    w.rows = p + at; at += sc::up256(P * 2 * (size_t)D * H);
    w.zero_bytes = at;
    w.g = reinterpret_cast<uint16_t *>(p + at); at += sc::up256(P * 2 * dhw * sizeof(uint16_t));
    w.f = reinterpret_cast<unsigned *>(p + at); at += sc::up256(P * 2 * dhw * sizeof(unsigned));
    w.d2 = reinterpret_cast<int *>(p + at); at += sc::up256(P * 2 * dhw * sizeof(int));
    w.total = at;
    return w;
}

struct Dims { int D, H, W, ux, uy, uz; };

// ---- pass (a): boundaries and distances along z ----------------------------------------------------------------------------------------
// One lane per (y, x) column of one set of one plane, consecutive lanes along x.  Down the column: the boundary test of the voxel (it
// is in the set and one of its 6-neighbours is not; outside the volume is not) and the running index distance to the last boundary
// voxel above; back up: the minimum with the distance to the next one below.  g == 0 marks the boundary voxels themselves; a column
// without any holds SENT.  A row (z, y) that holds a boundary voxel is flagged: every lane that finds one stores the same 1.
__global__ __launch_bounds__(256) void k_sv_columns(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ truth, Dims dm, int cblocks,
                                                    ScoreValues vals, uint16_t *__restrict__ g_all, uint8_t *__restrict__ rows_all, ScoreAcc *acc)
{
    __shared__ int s_n[4];
    const int D = dm.D, H = dm.H, W = dm.W;
    const size_t hw = (size_t)H * W, dhw = hw * D;
    const int items = 2 * vals.n * cblocks;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {        // (workgroup-uniform)
        const int q = item / cblocks, cb = item - q * cblocks, p = q >> 1, set = q & 1;
        const int v = sc::pick_value(vals.v, p);
        const uint8_t *const map = set ? truth : pred;
        uint16_t *const g = g_all + (size_t)q * dhw;
        uint8_t *const rows = rows_all + (size_t)q * D * H;
        const size_t i = (size_t)cb * 256 + threadIdx.x;
        int count = 0;
        if (i < hw) {
            const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
            const bool has_l = x > 0, has_r = x + 1 < W, has_u = y > 0, has_d = y + 1 < H;
            bool below = false, cur = map[i] == v;
            unsigned d = SENT;
#pragma unroll 2
            for (int z = 0; z < D; ++z) {
                const uint8_t *const at = map + (size_t)z * hw + i;
                const bool nxt = z + 1 < D && at[hw] == v;
                const bool l = has_l && at[-1] == v, r = has_r && at[1] == v;
                const bool u = has_u && at[-W] == v, dn = has_d && at[W] == v;
                const bool bnd = cur && !(below && nxt && l && r && u && dn);
                d = bnd ? 0u : min(d + 1, SENT);
                g[(size_t)z * hw + i] = (uint16_t)d;
                if (bnd) rows[(size_t)z * H + y] = 1;
                count += bnd;
                below = cur; cur = nxt;
            }
            d = SENT;
#pragma unroll 2
            for (int z = D - 1; z >= 0; --z) {
                const unsigned gv = g[(size_t)z * hw + i];
                d = gv == 0 ? 0u : min(d + 1, SENT);
                if (d < gv) g[(size_t)z * hw + i] = (uint16_t)d;
            }
        }
        count = sc::wave_sum(count);
        if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int tot = s_n[0] + s_n[1] + s_n[2] + s_n[3];
            if (tot) atomicAdd(&acc[p].n[set], tot);
        }
        __syncthreads();
    }
}

// ---- pass (b): along y inside a slice, in the rows some source voxel will read -------------------------------------------------------------
// f(z, y, x) of a set = min over y' of (g(z, y', x) * uz)^2 + ((y - y') * uy)^2 is read by the OTHER set's boundary voxels of row (z, y):
// a row the other set did not flag is left alone.  One lane per x, consecutive lanes along x; a scan outward from y that stops once
// (dy * uy)^2 >= the best so far, or when both sides have left the slice.  Exact for any distance: no block, no halo.  Every term is
// below 2^31 (the d2 limit of the call), so a sum of two fits 32 unsigned bits and stays below F_INF.
__global__ __launch_bounds__(256) void k_sv_y(Dims dm, int n, int wblocks, const uint16_t *__restrict__ g_all, const uint8_t *__restrict__ rows_all,
                                              unsigned *__restrict__ f_all, const ScoreAcc *acc)
{
    const int D = dm.D, H = dm.H, W = dm.W;
    const size_t hw = (size_t)H * W, dhw = hw * D;
    const long long per_set = (long long)D * H * wblocks, items = 2ll * n * per_set;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {  // (workgroup-uniform)
        const int q = (int)(item / per_set), p = q >> 1;
        if (acc[p].n[0] == 0 || acc[p].n[1] == 0) continue;    // an empty boundary: no distances
        const long long rest = item - (long long)q * per_set;
        const int row = (int)(rest / wblocks), xb = (int)(rest - (long long)row * wblocks);
        if (!rows_all[(size_t)(q ^ 1) * D * H + row]) continue; // no source voxel of the other set in this row
        const int x = xb * 256 + threadIdx.x;
        if (x >= W) continue;
        const int z = row / H, y = row - z * H;
        const uint16_t *const g = g_all + (size_t)q * dhw + (size_t)z * hw + x;      // + y' * W
        const unsigned g0 = g[(size_t)y * W];
        unsigned best = g0 == SENT ? F_INF : (g0 * dm.uz) * (g0 * dm.uz);
        for (int dy = 1; ; ++dy) {
            const unsigned t = (unsigned)(dy * dm.uy) * (unsigned)(dy * dm.uy);
            const int yl = y - dy, yr = y + dy;
            if (t >= best || (yl < 0 && yr >= H)) break;
            if (yl >= 0) {
                const unsigned gl = g[(size_t)yl * W];
                if (gl != SENT) best = min(best, t + (gl * dm.uz) * (gl * dm.uz));
            }
            if (yr < H) {
                const unsigned gr = g[(size_t)yr * W];
                if (gr != SENT) best = min(best, t + (gr * dm.uz) * (gr * dm.uz));
            }
        }
        f_all[(size_t)q * dhw + (size_t)row * W + x] = best;
    }
}

// ---- pass (c): d2 at the source boundary voxels of one row ----------------------------------------------------------------------------------
// A workgroup takes flagged rows (z, y) of one direction of one plane.  It lists the row's source boundary voxels (g_src == 0) in LDS and
// stages the whole row of the other set's f in LDS; each lane takes source voxels off the list: d2 = min over x' of ((x - x') * ux)^2 +
// f(z, y, x') by a scan outward from x that stops once (dx * ux)^2 >= the best so far, or when both sides have left the row.  When the
// other boundary is not empty some (z, x') line is finite in every row, so every d2 is a true distance below 2^31.  The values go to
// the direction's list behind one cursor add per row; maximum and sums are reduced in the wave, then in LDS, one global atomic each per
// row.
__global__ __launch_bounds__(256) void k_sv_rows(Dims dm, int n, const uint16_t *__restrict__ g_all, const uint8_t *__restrict__ rows_all,
                                                 const unsigned *__restrict__ f_all, int *__restrict__ d2_all, ScoreAcc *acc)
{
    extern __shared__ __attribute__((aligned(16))) unsigned s_dyn[];
    __shared__ unsigned s_cnt, s_base;
    __shared__ int s_max[4];
    __shared__ unsigned long long s_sum[4], s_q[4];
    const int D = dm.D, H = dm.H, W = dm.W, tid = threadIdx.x;
    unsigned *const s_f = s_dyn;
    uint16_t *const s_list = reinterpret_cast<uint16_t *>(s_dyn + W);
    const size_t dhw = (size_t)D * H * W;
    const long long per_set = (long long)D * H, items = 2ll * n * per_set;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {  // (workgroup-uniform, and so is every `continue` below)
        const int q = (int)(item / per_set), p = q >> 1, dir = q & 1;
        ScoreAcc *const a = acc + p;
        if (a->n[0] == 0 || a->n[1] == 0) continue;
        const long long row = item - (long long)q * per_set;
        if (!rows_all[(size_t)q * D * H + row]) continue;
        const uint16_t *const gsrc = g_all + (size_t)q * dhw + (size_t)row * W;
        const unsigned *const fdst = f_all + (size_t)(q ^ 1) * dhw + (size_t)row * W;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int x = tid; x < W; x += 256) {
            s_f[x] = fdst[x];
            if (gsrc[x] == 0) s_list[atomicAdd(&s_cnt, 1u)] = (uint16_t)x;
        }
        __syncthreads();
        const int cnt = (int)s_cnt;                             // (>= 1: the row is flagged)
        if (tid == 0) s_base = atomicAdd(&a->cursor[dir], (unsigned)cnt);
        __syncthreads();
        int *const out = d2_all + (size_t)q * dhw + s_base;
        int t_max = 0;
        unsigned long long t_sum = 0, t_q = 0;
        for (int i = tid; i < cnt; i += 256) {
            const int x = s_list[i];
            unsigned best = s_f[x];
            for (int dx = 1; ; ++dx) {
                const unsigned t = (unsigned)(dx * dm.ux) * (unsigned)(dx * dm.ux);
                const int xl = x - dx, xr = x + dx;
                if (t >= best || (xl < 0 && xr >= W)) break;
                if (xl >= 0) {
                    const unsigned fl = s_f[xl];
                    if (fl != F_INF) best = min(best, t + fl);
                }
                if (xr < W) {
                    const unsigned fr = s_f[xr];
                    if (fr != F_INF) best = min(best, t + fr);
                }
            }
            out[i] = (int)best;
            t_max = max(t_max, (int)best);
            t_sum += best;
            t_q += sc::sqrt_q16((int)best);
        }
        t_max = sc::wave_max(t_max);
        t_sum = sc::wave_sum(t_sum);
        t_q = sc::wave_sum(t_q);
        if ((tid & 63) == 0) { s_max[tid >> 6] = t_max; s_sum[tid >> 6] = t_sum; s_q[tid >> 6] = t_q; }
        __syncthreads();
        if (tid == 0) {
            atomicMax(&a->max_d2[dir], max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
            const unsigned long long sd = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3], sq = s_q[0] + s_q[1] + s_q[2] + s_q[3];
            if (sd) atomicAdd(&a->sum_d2[dir], sd);
            if (sq) atomicAdd(&a->sum_q[dir], sq);
        }
        __syncthreads();                                        // the next row reuses the LDS
    }
}

}  // namespace sv

size_t score_volume_workspace_bytes(int D, int H, int W, int n, int classes) { return sv::carve(nullptr, D, H, W, n, classes).total; }

hipError_t launch_score_volume(const uint8_t *pred, const uint8_t *truth, const ScoreVolumeArgs &a, void *ws, mi_unet_score *scores,
                               const unsigned long long **conf, hipStream_t s)
{
    const int D = a.D, H = a.H, W = a.W, n = a.vals.n;
    if (!pred || !truth || !ws || !scores || n < 1 || n > SCORE_MAX_VALUES) return hipErrorInvalidValue;
    if (D < 1 || H < 1 || W < 1 || D > SCORE_VOLUME_MAX_SIDE || H > SCORE_VOLUME_MAX_SIDE || W > SCORE_VOLUME_MAX_SIDE) return hipErrorInvalidValue;
    if (a.classes < 0 || a.classes > 16 || a.quantile_ppm < 0 || a.quantile_ppm > 999999) return hipErrorInvalidValue;
    const long long hw = (long long)H * W, dhw = hw * D;
    if (n * dhw > 0x7FFFFFFFLL || a.ux < 1 || a.uy < 1 || a.uz < 1) return hipErrorInvalidValue;
    // every term (side - 1) * unit stays below 2^15.5, so the products below are exact, and their squares sum to less than 2^31
    const long long ex = (long long)(W - 1) * a.ux, ey = (long long)(H - 1) * a.uy, ez = (long long)(D - 1) * a.uz;
    if (ex > 46340 || ey > 46340 || ez > 46340 || ex * ex + ey * ey + ez * ez > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    const sv::Ws w = sv::carve(ws, D, H, W, n, a.classes);
    if (hipError_t e = hipMemsetAsync(w.acc, 0, w.zero_bytes, s)) return e;
    const dim3 blk(256);
    const sv::Dims dm{ D, H, W, a.ux, a.uy, a.uz };
    auto grid = [](long long items) { return dim3((unsigned)(items < sv::MAX_ITEMS ? items : sv::MAX_ITEMS)); };
    sc::launch_score_counts(pred, truth, 1, dhw, a.vals, a.classes, w.acc, w.conf, s);         // the volume as one image
    const int cblocks = (int)((hw + 255) / 256), wblocks = (W + 255) / 256;
    hipLaunchKernelGGL(sv::k_sv_columns, grid(2ll * n * cblocks), blk, 0, s, pred, truth, dm, cblocks, a.vals, w.g, w.rows, w.acc);
    hipLaunchKernelGGL(sv::k_sv_y, grid(2ll * n * D * H * wblocks), blk, 0, s, dm, n, wblocks, w.g, w.rows, w.f, w.acc);
    const size_t lds = (size_t)W * sizeof(unsigned) + (size_t)((W + 1) & ~1) * sizeof(uint16_t);   // the row of f and the list: 49152 bytes at W = 8192
    hipLaunchKernelGGL(sv::k_sv_rows, grid(2ll * n * D * H), blk, lds, s, dm, n, w.g, w.rows, w.f, w.d2, w.acc);
    sc::launch_score_select(n, (size_t)dhw, a.vals, a.quantile_ppm, w.acc, w.d2, w.hist, scores, s);
    if (conf) *conf = w.conf;
    return hipGetLastError();
}

}  // namespace miunet
