// score.hip -- a prediction against ground truth, per (image, value) plane: overlap counts, the confusion matrix, and the exact
// squared distances between the two boundaries with their maximum, sums and order statistics (include/mi_unet.h:
// mi_unet_score_labels).  Byte and integer work, exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "score_common.h"

namespace miunet {

namespace sc {

constexpr int D2_INF = 0x7FFFFFFF;                      // above every d2 (<= 2 * 32766^2)
constexpr int HIST_BLOCKS = 8;                          // workgroups per (plane, direction) list in the histogram passes

struct Ws {
    ScoreAcc *acc;                  // [P]
    unsigned long long *conf;       // [B][classes * classes], then [B] skipped
    unsigned *hist;                 // [P][5][65536]: high halves of direction 0, 1; low halves of selection 0, 1, 2
    size_t zero_bytes;              // the three above are one run from acc
    uint16_t *g;                    // [P][2][H * W]: vertical distance to the nearest boundary pixel of the column, of dA and of dT
    int *d2;                        // [P][2][H * W]: the direction's values, cursor[] of them, in no particular order
    size_t total;
};

inline Ws carve(void *base, int B, int H, int W, int n, int classes)
{
    const size_t P = (size_t)B * n, hw = (size_t)H * W;
    uint8_t *p = static_cast<uint8_t *>(base);
    Ws w;
    size_t at = 0;
    w.acc = reinterpret_cast<ScoreAcc *>(p + at); at += up256(P * sizeof(ScoreAcc));
    w.conf = reinterpret_cast<unsigned long long *>(p + at); at += up256((size_t)B * (classes * classes + 1) * 8);
    w.hist = reinterpret_cast<unsigned *>(p + at); at += P * HIST_BYTES_PER_PLANE;
    w.zero_bytes = at;
    w.g = reinterpret_cast<uint16_t *>(p + at); at += up256(P * 2 * hw * sizeof(uint16_t));
    w.d2 = reinterpret_cast<int *>(p + at); at += up256(P * 2 * hw * sizeof(int));
    w.total = at;
    return w;
}

// hist[key] += 1 for every lane whose key is not NONE: the lanes of a wave that hold the same key send ONE add (boundary distances of a
// fair prediction pile onto a handful of small values; see cc_stats in DESIGN 7 for what same-address atomics cost).  Every lane of
// the wave must call it.
__device__ __forceinline__ void wave_hist_add(unsigned *hist, unsigned key)
{
    const int lane = threadIdx.x & 63;
    peel<64>(key, NONE, [&](unsigned k0, bool, u64 m, int leader) {
        if (lane == leader) atomicAdd(&hist[k0], (unsigned)__builtin_popcountll(m));
    });
}

// ---- counts: tp / fp / fn of every value and the confusion matrix, both maps read once ------------------------------------------
// A wave counts with ballots: the sums of its 64 pixels are wave-uniform and stay in registers until the end.  The confusion matrix
// has a private LDS histogram per wave that only the leader lane of a group of equal (truth, pred) pairs adds to, so LDS sees no
// atomics at all; one global add per non-empty counter per workgroup.
template <bool CONF>
__global__ __launch_bounds__(256) void k_score_counts(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ truth, int hw,
                                                      ScoreValues vals, int classes, ScoreAcc *acc, unsigned long long *conf)
{
    __shared__ int s_cnt[3 * SCORE_MAX_VALUES];
    __shared__ unsigned s_conf[CONF ? 4 : 1][CONF ? 257 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
    if (tid < 3 * SCORE_MAX_VALUES) s_cnt[tid] = 0;
    if constexpr (CONF)
        for (int i = tid; i < 4 * 257; i += 256) (&s_conf[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *const pp = pred + (size_t)b * hw, *const tp_ = truth + (size_t)b * hw;
    int c_tp[SCORE_MAX_VALUES] = {}, c_fp[SCORE_MAX_VALUES] = {}, c_fn[SCORE_MAX_VALUES] = {};
    const long long stride = (long long)gridDim.x * 256;
    for (long long base = (long long)blockIdx.x * 256 + 64 * wv; base < hw; base += stride) {      // (wave-uniform)
        const long long i = base + lane;
        const bool valid = i < hw;
        const int p = valid ? pp[i] : -1, t = valid ? tp_[i] : -1;
#pragma unroll
        for (int k = 0; k < SCORE_MAX_VALUES; ++k) {
            if (k < vals.n) {
                const unsigned long long ma = __ballot(p == vals.v[k]), mt = __ballot(t == vals.v[k]);
                c_tp[k] += __builtin_popcountll(ma & mt);
                c_fp[k] += __builtin_popcountll(ma & ~mt);
                c_fn[k] += __builtin_popcountll(mt & ~ma);
            }
        }
        if constexpr (CONF) {
            unsigned key = NONE;
            if (valid) key = (p < classes && t < classes) ? (unsigned)(t * classes + p) : 256u;
            peel<64>(key, NONE, [&](unsigned k0, bool, u64 m, int leader) {
                if (lane == leader) s_conf[wv][k0] += (unsigned)__builtin_popcountll(m);
            });
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SCORE_MAX_VALUES; ++k) {
            if (k < vals.n) {
                if (c_tp[k]) atomicAdd(&s_cnt[3 * k], c_tp[k]);
                if (c_fp[k]) atomicAdd(&s_cnt[3 * k + 1], c_fp[k]);
                if (c_fn[k]) atomicAdd(&s_cnt[3 * k + 2], c_fn[k]);
            }
        }
    }
    __syncthreads();
    if (tid < 3 * vals.n && s_cnt[tid]) {
        ScoreAcc *a = acc + (size_t)b * vals.n + tid / 3;
        atomicAdd(tid % 3 == 0 ? &a->tp : tid % 3 == 1 ? &a->fp : &a->fn, s_cnt[tid]);
    }
    if constexpr (CONF) {
        const int cc = classes * classes;
        for (int i = tid; i < 257; i += 256) {
            const unsigned sum = s_conf[0][i] + s_conf[1][i] + s_conf[2][i] + s_conf[3][i];
            if (!sum) continue;
            if (i < cc) atomicAdd(&conf[(size_t)b * cc + i], (unsigned long long)sum);
            else if (i == 256) atomicAdd(&conf[(size_t)gridDim.y * cc + b], (unsigned long long)sum);
        }
    }
}

// ---- boundaries and column distances --------------------------------------------------------------------------------------------
// One lane per column of one set of one plane.  Down the column: the boundary test of the pixel (it is in the set and one of its
// 4-neighbours is not; outside the image is not) and the running distance to the last boundary pixel above, uncapped; back up: the
// minimum with the distance to the next one below.  g == 0 marks the boundary pixels themselves; a column without any holds SENT.
__global__ __launch_bounds__(256) void k_score_columns(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ truth, int H, int W,
                                                       int wblocks, ScoreValues vals, uint16_t *__restrict__ g_all, ScoreAcc *acc)
{
    __shared__ int s_n[4];
    const int q = blockIdx.x / wblocks, xb = blockIdx.x - q * wblocks, p = q >> 1, set = q & 1;
    const int b = p / vals.n, v = pick_value(vals.v, p - b * vals.n);
    const size_t hw = (size_t)H * W;
    const uint8_t *const map = (set ? truth : pred) + (size_t)b * hw;
    uint16_t *const g = g_all + (size_t)q * hw;
    const int x = xb * 256 + threadIdx.x;
    int count = 0;
    if (x < W) {
        const bool has_l = x > 0, has_r = x + 1 < W;
        bool up = false, cur = map[x] == v;
        unsigned d = SENT;
#pragma unroll 4
        for (int y = 0; y < H; ++y) {
            const uint8_t *const row = map + (size_t)y * W;
            const bool nxt = y + 1 < H && row[W + x] == v;
            const bool l = has_l && row[x - 1] == v, r = has_r && row[x + 1] == v;
            const bool bnd = cur && !(up && nxt && l && r);
            d = bnd ? 0u : min(d + 1, SENT);
            g[(size_t)y * W + x] = (uint16_t)d;
            count += bnd;
            up = cur; cur = nxt;
        }
        d = SENT;
#pragma unroll 4
        for (int y = H - 1; y >= 0; --y) {
            const unsigned gv = g[(size_t)y * W + x];
            d = gv == 0 ? 0u : min(d + 1, SENT);
            if (d < gv) g[(size_t)y * W + x] = (uint16_t)d;
        }
    }
    count = wave_sum(count);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = s_n[0] + s_n[1] + s_n[2] + s_n[3];
        if (tot) atomicAdd(&acc[p].n[set], tot);
    }
}

// ---- row pass: d2 at the source boundary pixels of one row --------------------------------------------------------------------------
// A workgroup owns row y of one direction of one plane.  It lists the row's source boundary pixels (g_src == 0) in LDS; a row without
// any ends there.  Otherwise the whole row of g_dst is staged in LDS -- whatever the width: the nearest pixel may lie anywhere -- and
// each lane takes source pixels off the list: d2 = min over x' of (x - x')^2 + g_dst(x', y)^2 by a scan outward from x that stops once
// dx^2 >= the best so far, or when both sides have left the row.  Exact for any distance up to the image diagonal.  When dT (dA) is
// not empty every row holds a finite g: a column with a boundary pixel is finite in all its rows.  The values go to the direction's
// list behind one cursor add per row; maximum and sums are reduced in the wave, then in LDS, one global atomic each per workgroup.
__global__ __launch_bounds__(256) void k_score_rows(int H, int W, const uint16_t *__restrict__ g_all, int *__restrict__ d2_all,
                                                    ScoreAcc *acc)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t s_dyn[];
    __shared__ unsigned s_cnt, s_base;
    __shared__ int s_max[4];
    __shared__ unsigned long long s_sum[4], s_q[4];
    const unsigned q = blockIdx.x / (unsigned)H;
    const int y = (int)(blockIdx.x - q * (unsigned)H), p = (int)(q >> 1), dir = (int)(q & 1);
    ScoreAcc *const a = acc + p;
    if (a->n[0] == 0 || a->n[1] == 0) return;                  // (workgroup-uniform) an empty boundary: no distances
    const int wp = (W + 1) & ~1;
    uint16_t *const s_g = s_dyn, *const s_list = s_dyn + wp;
    const size_t hw = (size_t)H * W;
    const uint16_t *const gsrc = g_all + ((size_t)2 * p + dir) * hw + (size_t)y * W;
    const uint16_t *const gdst = g_all + ((size_t)2 * p + (dir ^ 1)) * hw + (size_t)y * W;
    const int tid = threadIdx.x;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int x = tid; x < W; x += 256)
        if (gsrc[x] == 0) s_list[atomicAdd(&s_cnt, 1u)] = (uint16_t)x;
    __syncthreads();
    const int cnt = (int)s_cnt;
    if (cnt == 0) return;                                       // (workgroup-uniform)
    for (int x = tid; x < W; x += 256) s_g[x] = gdst[x];
    if (tid == 0) s_base = atomicAdd(&a->cursor[dir], (unsigned)cnt);
    __syncthreads();
    int *const out = d2_all + ((size_t)2 * p + dir) * hw + s_base;
    int t_max = 0;
    unsigned long long t_sum = 0, t_q = 0;
    for (int i = tid; i < cnt; i += 256) {
        const int x = s_list[i];
        const int g0 = s_g[x];
        int best = g0 == (int)SENT ? D2_INF : g0 * g0;
        for (int dx = 1; ; ++dx) {
            const int dx2 = dx * dx, xl = x - dx, xr = x + dx;
            if (dx2 >= best || (xl < 0 && xr >= W)) break;
            if (xl >= 0) {
                const int gl = s_g[xl];
                if (gl != (int)SENT) best = min(best, dx2 + gl * gl);
            }
            if (xr < W) {
                const int gr = s_g[xr];
                if (gr != (int)SENT) best = min(best, dx2 + gr * gr);
            }
        }
        out[i] = best;
        t_max = max(t_max, best);
        t_sum += (unsigned)best;
        t_q += sqrt_q16(best);
    }
    t_max = wave_max(t_max);
    t_sum = wave_sum(t_sum);
    t_q = wave_sum(t_q);
    if ((tid & 63) == 0) { s_max[tid >> 6] = t_max; s_sum[tid >> 6] = t_sum; s_q[tid >> 6] = t_q; }
    __syncthreads();
    if (tid == 0) {
        atomicMax(&a->max_d2[dir], max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
        const unsigned long long sd = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3], sq = s_q[0] + s_q[1] + s_q[2] + s_q[3];
        if (sd) atomicAdd(&a->sum_d2[dir], sd);
        if (sq) atomicAdd(&a->sum_q[dir], sq);
    }
}

// ---- the order statistics: a two-level radix select over the 31-bit values, 16 + 16 bits ------------------------------------------
// LOW = false: hist[p][dir] += the high halves of the direction's values.  LOW = true: the low halves of the values whose high half holds
// the rank of the direction's own selection (hist[p][2 + dir]) and of the selection over both directions (hist[p][4]).
template <bool LOW>
__global__ __launch_bounds__(256) void k_score_hist(size_t hw, const int *__restrict__ d2_all, const ScoreAcc *acc, unsigned *hist_all)
{
    const unsigned q = blockIdx.x / HIST_BLOCKS, j = blockIdx.x - q * HIST_BLOCKS, p = q >> 1, dir = q & 1;
    const ScoreAcc *const a = acc + p;
    const unsigned cnt = a->cursor[dir];
    if (cnt == 0) return;                                       // (workgroup-uniform)
    const int *const v = d2_all + (size_t)q * hw;
    unsigned *const hist = hist_all + (size_t)p * 5 * 65536;
    const unsigned own = LOW ? a->sel_bin[dir] : 0, sym = LOW ? a->sel_bin[2] : 0;
    for (unsigned base = j * 256 + (threadIdx.x & ~63u); base < cnt; base += HIST_BLOCKS * 256) {     // (wave-uniform)
        const unsigned i = base + (threadIdx.x & 63);
        const unsigned d = i < cnt ? (unsigned)v[i] : NONE;
        if constexpr (LOW) {
            wave_hist_add(hist + (size_t)(2 + dir) * 65536, (d != NONE && (d >> 16) == own) ? (d & 0xFFFFu) : NONE);
            wave_hist_add(hist + (size_t)4 * 65536, (d != NONE && (d >> 16) == sym) ? (d & 0xFFFFu) : NONE);
        } else {
            wave_hist_add(hist + (size_t)dir * 65536, d != NONE ? (d >> 16) : NONE);
        }
    }
}

// One workgroup per (plane, selection): the bin of the 65536-bin histogram that holds the rank and the rank inside it.  A lane sums
// its run of 256 bins, the runs are scanned across the workgroup, and the lane whose run holds the rank walks it.  LOW = false:
// the rank is n - 1 - floor(n * ppm / 1e6) of the selection's n values, the histogram that of the high halves (both directions'
// added for the third selection).  LOW = true: the rank left inside the high half, the histogram of its low halves.
template <bool LOW>
__global__ __launch_bounds__(256) void k_score_pick(int quantile_ppm, ScoreAcc *acc, const unsigned *hist_all)
{
    __shared__ unsigned s_tot[4];
    const unsigned p = blockIdx.x / 3, sel = blockIdx.x - 3 * p, t = threadIdx.x;
    ScoreAcc *const a = acc + p;
    if (a->n[0] == 0 || a->n[1] == 0) return;                  // (workgroup-uniform)
    const unsigned *const hist = hist_all + (size_t)p * 5 * 65536;
    const unsigned *h0, *h1 = nullptr;
    unsigned rank;
    if constexpr (LOW) {
        h0 = hist + (size_t)(2 + sel) * 65536;
        rank = a->sel_rest[sel];
    } else {
        h0 = hist + (size_t)(sel == 1 ? 1 : 0) * 65536;
        if (sel == 2) h1 = hist + 65536;
        const unsigned long long n = sel == 0 ? (unsigned)a->n[0] : sel == 1 ? (unsigned)a->n[1] : (unsigned long long)(unsigned)a->n[0] + (unsigned)a->n[1];
        rank = (unsigned)(n - 1 - n * (unsigned)quantile_ppm / 1000000ull);
    }
    unsigned c = 0;
    for (int i = 0; i < 256; ++i) c += h0[t * 256 + i] + (h1 ? h1[t * 256 + i] : 0u);
    unsigned inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = (unsigned)__shfl_up((int)inc, o, 64);
        if ((t & 63) >= (unsigned)o) inc += u;
    }
    if ((t & 63) == 63) s_tot[t >> 6] = inc;
    __syncthreads();
    for (unsigned wv = 0; wv < (t >> 6); ++wv) inc += s_tot[wv];
    unsigned exc = inc - c;
    if (exc <= rank && rank < inc) {                            // exactly one lane
        for (int i = 0; i < 256; ++i) {
            const unsigned bc = h0[t * 256 + i] + (h1 ? h1[t * 256 + i] : 0u);
            if (rank < exc + bc) {
                if constexpr (LOW) a->sel_lo[sel] = t * 256 + i;
                else { a->sel_bin[sel] = t * 256 + i; a->sel_rest[sel] = rank - exc; }
                break;
            }
            exc += bc;
        }
    }
}

__global__ __launch_bounds__(256) void k_score_final(int P, ScoreValues vals, int quantile_ppm, const ScoreAcc *acc, mi_unet_score *out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const ScoreAcc a = acc[p];
    const bool have = a.n[0] > 0 && a.n[1] > 0;
    mi_unet_score s;
    s.tp = a.tp; s.fp = a.fp; s.fn = a.fn;
    s.q_d2_sym = have ? (int)((a.sel_bin[2] << 16) | a.sel_lo[2]) : -1;
    s.value = pick_value(vals.v, p % vals.n);
    s.quantile_ppm = quantile_ppm;
    mi_unet_score_dir d[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        d[j].n = a.n[j];
        d[j].max_d2 = have ? a.max_d2[j] : -1;
        d[j].q_d2 = have ? (int)((a.sel_bin[j] << 16) | a.sel_lo[j]) : -1;
        d[j].reserved = 0;
        d[j].sum_d2 = have ? (long long)a.sum_d2[j] : 0;
        d[j].sum_d_q16 = have ? (long long)a.sum_q[j] : 0;
    }
    s.a_to_t = d[0]; s.t_to_a = d[1];
    out[p] = s;
}

void launch_score_counts(const uint8_t *pred, const uint8_t *truth, int B, long long hw, const ScoreValues &vals, int classes, ScoreAcc *acc,
                         unsigned long long *conf, hipStream_t s)
{
    long long cblocks = (hw + 256 * 16 - 1) / (256 * 16);      // 16 pixels per lane
    if (cblocks > 1024) cblocks = 1024;
    const dim3 cg((unsigned)cblocks, (unsigned)B), blk(256);
    if (classes > 0) hipLaunchKernelGGL(k_score_counts<true>, cg, blk, 0, s, pred, truth, (int)hw, vals, classes, acc, conf);
    else hipLaunchKernelGGL(k_score_counts<false>, cg, blk, 0, s, pred, truth, (int)hw, vals, classes, acc, conf);
}

void launch_score_select(int P, size_t stride, const ScoreValues &vals, int quantile_ppm, ScoreAcc *acc, const int *d2, unsigned *hist,
                         ::mi_unet_score *scores, hipStream_t s)
{
    const dim3 hg((unsigned)(2 * P * HIST_BLOCKS)), pg((unsigned)(3 * P)), blk(256);
    hipLaunchKernelGGL(k_score_hist<false>, hg, blk, 0, s, stride, d2, acc, hist);
    hipLaunchKernelGGL(k_score_pick<false>, pg, blk, 0, s, quantile_ppm, acc, hist);
    hipLaunchKernelGGL(k_score_hist<true>, hg, blk, 0, s, stride, d2, acc, hist);
    hipLaunchKernelGGL(k_score_pick<true>, pg, blk, 0, s, quantile_ppm, acc, hist);
    hipLaunchKernelGGL(k_score_final, dim3((unsigned)((P + 255) / 256)), blk, 0, s, P, vals, quantile_ppm, acc, scores);
}

}  // namespace sc

size_t score_workspace_bytes(int B, int H, int W, int n, int classes) { return sc::carve(nullptr, B, H, W, n, classes).total; }

hipError_t launch_score(const uint8_t *pred, const uint8_t *truth, int B, int H, int W, const ScoreValues &vals, int quantile_ppm,
                        int classes, void *ws, mi_unet_score *scores, const unsigned long long **conf, hipStream_t s)
{
    const int n = vals.n;
    if (!pred || !truth || !ws || !scores || B < 1 || n < 1 || n > SCORE_MAX_VALUES || H < 1 || W < 1 || H > 32767 || W > 32767)
        return hipErrorInvalidValue;
    if (classes < 0 || classes > 16 || quantile_ppm < 0 || quantile_ppm > 999999) return hipErrorInvalidValue;
    const long long P = (long long)B * n, hw = (long long)H * W;
    if (P * hw > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    const int wblocks = (W + 255) / 256;
    // at most 32767 planes (MI_UNET_SCORE_MAX_PLANES, refused by the entry points with MI_UNET_EARG): every grid below stays under
    // 2^31 workgroups -- 2 P H <= 2 * 32767^2 is the largest -- and B fits gridDim.y
    if (P > 32767) return hipErrorInvalidValue;
    const sc::Ws w = sc::carve(ws, B, H, W, n, classes);
    if (hipError_t e = hipMemsetAsync(w.acc, 0, w.zero_bytes, s)) return e;
    const dim3 blk(256);
    sc::launch_score_counts(pred, truth, B, hw, vals, classes, w.acc, w.conf, s);
    hipLaunchKernelGGL(sc::k_score_columns, dim3((unsigned)(2 * P * wblocks)), blk, 0, s, pred, truth, H, W, wblocks, vals, w.g, w.acc);
    const size_t lds = (size_t)2 * ((W + 1) & ~1) * sizeof(uint16_t);      // the row of g and the list: at most 131072 bytes at W = 32767
    if (lds > 65536)
        if (hipError_t e = ensure_dynamic_lds(sc::k_score_rows, lds)) return e;
    hipLaunchKernelGGL(sc::k_score_rows, dim3((unsigned)(2 * P * H)), blk, lds, s, H, W, w.g, w.d2, w.acc);
    sc::launch_score_select((int)P, (size_t)hw, vals, quantile_ppm, w.acc, w.d2, w.hist, scores, s);
    if (conf) *conf = w.conf;
    return hipGetLastError();
}

}  // namespace miunet
