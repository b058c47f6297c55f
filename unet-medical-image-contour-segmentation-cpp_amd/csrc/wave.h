// wave.h -- what the kernels of the stages behind the network do inside one 64-lane wave, and among the four waves of a workgroup
// (DESIGN.md 7.19): the butterfly reduction, the distinct keys of a wave taken one after the other, atomics merged per key, a cursor
// shared by a wave, the waves' totals through LDS.  Three things hold for every caller and are what these helpers rest on:
//   * control flow is wave-uniform: a helper that shuffles or ballots is called by every lane of the wave (wave_offsets: of the
//     workgroup), and every loop here runs on a ballot, the same in every lane;
//   * results are integer sums, minima, maxima and counts, so neither the order of the butterfly nor that of the atomics shows;
//   * keys are taken lowest lane first, so "the first LIMIT keys of a segment" means the same on every run.
// Internal to libmiunet.so, device code only.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace miunet {

namespace wave {

typedef unsigned long long u64;

// ---- the butterfly: op over the 64 lanes, the result in every lane.  64-bit values go through __shfl_xor as they are. -----------------
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
// (T: int, unsigned, long long, unsigned long long; k_vsp_pairs adds doubles with wave_sum: the butterfly is the same tree on every run
// and a + b == b + a bit for bit, so every lane ends with the same bits, call after call)
template <class T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <class T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return b < a ? b : a; }); }
template <class T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return b > a ? b : a; }); }

// the lanes of the wave below this one: a lane's rank among the set lanes of a ballot is popcount(ballot & lanes_below())
__device__ __forceinline__ u64 lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// ---- a word that only grows (raise) or only shrinks (lower) ------------------------------------------------------------------------------
// A plain read that already shows a value at least as good makes the atomic unnecessary (a stale read costs an atomic, never a result):
// the atomics of thousands of waves on the one word of a large component are served one after another, and after the first few none of
// them changes anything.
__device__ __forceinline__ int peek(const int *word) { return __builtin_nontemporal_load(word); }
__device__ __forceinline__ void raise(int *word, int v)
{
    if (peek(word) < v) atomicMax(word, v);
}
__device__ __forceinline__ void lower(int *word, int v)
{
    if (peek(word) > v) atomicMin(word, v);
}

// ---- peel: the distinct keys of the wave other than `none`, lowest lane first, at most LIMIT of them -------------------------------------
// f(k0, mine, mask, leader) is called wave-uniformly once per key: k0 the key, mine whether this lane holds it, mask the ballot of the
// lanes that do, leader the lowest of them.  The key of a lane that was handled becomes `none`, so after a bounded peel the lanes left
// over are those with key != none.  LIMIT = 64 is the unbounded form: every key is handled, nothing is left over, and key is left as
// it was.
template <int LIMIT, class K, class F>
__device__ __forceinline__ void peel(K &key, K none, F f)
{
    u64 todo = __ballot(key != none);
    for (int g = 0; (LIMIT >= 64 || g < LIMIT) && todo; ++g) {  // (wave-uniform)
        const int leader = __builtin_ctzll(todo);
        const K k0 = (K)__shfl((int)key, leader, 64);
        const bool mine = key == k0;
        const u64 mask = __ballot(mine);
        f(k0, mine, mask, leader);
        todo &= ~mask;
        if (LIMIT < 64 && mine) key = none;
    }
}

// ---- merged_add: one count into tab[cell] from every lane that is `on`, merged per cell -----------------------------------------------------
// `tab` is a table in LDS or in memory.  The wave merges the lanes that name the same cell, for the first MERGE distinct cells, into one
// atomic each (in a homogeneous component nearly every lane names the same cell, and 64 atomics on one address would be served one
// after another); the lanes left over add their own.  With `sums` (wave-uniform, may be null) the same lanes add `val` into
// sums[cell]: 64 bits in memory, 32 in a workgroup's LDS.  This is peel<MERGE> on the pair (on, cell), written out: the hot paths want the
// loop unrolled and the cell kept apart from `on`, which peel's callers do not.
template <int MERGE, class S>
__device__ __forceinline__ void merged_add(uint32_t *tab, S *sums, bool on, unsigned cell, unsigned val)
{
    u64 todo = __ballot(on);
#pragma unroll
    for (int g = 0; g < MERGE; ++g) {
        if (!todo) break;                                       // (wave-uniform)
        const int leader = __builtin_ctzll(todo);
        const unsigned c0 = (unsigned)__shfl((int)cell, leader, 64);
        const bool same = on && cell == c0;
        const u64 mask = __ballot(same);
        unsigned total = 0;
        if (sums) total = wave_sum(same ? val : 0u);
        if ((int)(threadIdx.x & 63) == leader) {
            atomicAdd(tab + c0, (uint32_t)__popcll(mask));
            if (total) atomicAdd(sums + c0, (S)total);
        }
        todo &= ~mask;
        if (same) on = false;
    }
    if (on) {
        atomicAdd(tab + cell, 1u);
        if (sums && val) atomicAdd(sums + cell, (S)val);
    }
}
template <int MERGE>
__device__ __forceinline__ void merged_add(uint32_t *tab, bool on, unsigned cell)
{
    merged_add<MERGE>(tab, (uint32_t *)nullptr, on, cell, 0u);
}

// ---- wave_take: one add to a cursor for the lanes of `mask`, every one of them takes base + its rank ---------------------------------------
// Called by every lane of the wave (inside peel); the value returned means something in the lanes of `mask`.
template <class T>
__device__ __forceinline__ T wave_take(T *cursor, u64 mask, int leader)
{
    T base = 0;
    if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(cursor, (T)__popcll(mask));
    base = (T)__shfl((int)base, leader, 64);
    return base + (T)__popcll(mask & lanes_below());
}

// ---- the four waves' totals through LDS -> (the sum of the waves before this one, the workgroup's sum) ------------------------------------
// Every lane of a workgroup of 256 calls this; s_w is four ints of LDS that nobody else touches until the next barrier.
__device__ __forceinline__ int2 wave_offsets(int wave_total, int *s_w)
{
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    const int w = threadIdx.x >> 6;
    int before = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j < w) before += s_w[j];
    return make_int2(before, s_w[0] + s_w[1] + s_w[2] + s_w[3]);
}

// v[k] of a table that is a kernel argument, by a chain of selects: a run-time index would put the table into scratch memory
template <int N>
__device__ __forceinline__ int pick_value(const int (&v)[N], int k)
{
    int r = v[0];
#pragma unroll
    for (int j = 1; j < N; ++j)
        if (k == j) r = v[j];
    return r;
}

}  // namespace wave

}  // namespace miunet
