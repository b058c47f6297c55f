// score_common.h -- what score.hip and score_volume.hip (7.10) share: the accumulators of a plane, the exact q16 root, and the launchers of the kernels that do not care how many axes a plane has -- the counts over a
// run of bytes and the 16 + 16-bit radix select over a direction's list with the final step.  The kernels themselves live in
// score.hip.  Internal to libmiunet.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "kernels.h"
#include "wave.h"

namespace miunet {

namespace sc {

using namespace wave;

constexpr unsigned SENT = 0xFFFFu;                      // g of a column without a boundary pixel (real distances are <= 32766)
constexpr unsigned NONE = 0xFFFFFFFFu;

// The accumulators of one plane, zeroed on the stream before the first kernel.
struct ScoreAcc {
    int tp, fp, fn;
    int n[2];                       // boundary pixels of A, of T
    int max_d2[2];                  // per direction (0: dA -> dT, 1: dT -> dA)
    unsigned cursor[2];             // values appended to the direction's list
    unsigned sel_bin[3], sel_rest[3], sel_lo[3];   // per selection (a_to_t, t_to_a, both): the high half that holds the rank, the rank inside it, the low half
    unsigned long long sum_d2[2], sum_q[2];
};
static_assert(sizeof(ScoreAcc) % 8 == 0, "ScoreAcc rows stay 8-byte aligned");

constexpr size_t HIST_BYTES_PER_PLANE = (size_t)5 * 65536 * sizeof(unsigned);   // high halves of direction 0, 1; low halves of selection 0, 1, 2

__host__ __device__ inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// floor(2^16 sqrt(d2)) exactly: the fp64 root of d2 << 32 (exact in fp64: 31 significant bits), corrected to the integer floor
__device__ __forceinline__ unsigned long long sqrt_q16(int d2)
{
    const unsigned long long v = (unsigned long long)(unsigned)d2 << 32;
    unsigned long long r = (unsigned long long)sqrt((double)v);         // r < 2^31.5: r * r and (r + 1)^2 fit
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// counts: tp / fp / fn of every value over B runs of hw bytes (acc[b * vals.n + k]) and, with classes > 0, the confusion matrix
// u64 [B][classes][classes] with the [B] skipped counts behind it; acc and conf zeroed by the caller
void launch_score_counts(const uint8_t *pred, const uint8_t *truth, int B, long long hw, const ScoreValues &vals, int classes, ScoreAcc *acc,
                         unsigned long long *conf, hipStream_t s);
// select + final: the order statistics of the P planes' lists (d2 [P][2][stride], acc[p].cursor[dir] values each; hist [P][5][65536]
// zeroed by the caller), then one mi_unet_score per plane
void launch_score_select(int P, size_t stride, const ScoreValues &vals, int quantile_ppm, ScoreAcc *acc, const int *d2, unsigned *hist,
                         ::mi_unet_score *scores, hipStream_t s);

}  // namespace sc

}  // namespace miunet
