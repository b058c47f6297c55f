// upsample.hip -- bilinear x2 upsampling with align_corners=True: the decoder step of a bilinear=True UNet (Pytorch-UNet's
// nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)), writing the upper half of a concat buffer.
//
// A gather with no reuse in registers: every output element is four taps of the input.  One lane per (output pixel, 16-byte
// channel group) -- 4 fp32 or 8 bf16 / fp16 channels -- with consecutive lanes on consecutive channel groups, then the next pixel
// along x: each of the four taps is a 16-byte load, and the store is a full 16-byte global_store_dwordx4 into the concat slice,
// the pixels of a wave one contiguous run of slice bytes each.  Neighbouring output pixels share their source pixels (each input
// pixel feeds 4 x 4 output pixels), so the re-reads hit L1 / L2 and HBM sees the input about once.  The grid is 1-D with one
// lane per element (measured against grid-stride launches of 1..32 workgroups per CU); the kernel keeps its
// grid-stride loop, so any grid is correct.
#include <algorithm>

#include "kernel_common.h"

namespace miunet {
namespace {

template <typename T> struct UpVec;                     // 16 bytes of T
template <> struct UpVec<float> { typedef float v __attribute__((ext_vector_type(4))); static constexpr int N = 4; };
template <> struct UpVec<__bf16> { typedef __bf16 v __attribute__((ext_vector_type(8))); static constexpr int N = 8; };
template <> struct UpVec<_Float16> { typedef _Float16 v __attribute__((ext_vector_type(8))); static constexpr int N = 8; };

// q = n / d, r = n - q d; by a shift when d is a power of two (every tensor of the engine's plans), a division otherwise
__device__ __forceinline__ unsigned divmod(unsigned n, unsigned d, int shift, unsigned &r)
{
    const unsigned q = shift >= 0 ? n >> shift : n / d;
    r = n - q * d;
    return q;
}

// Source taps and weights along one axis, in fp32 as PyTorch's CPU kernel computes them (align_corners=True):
// src = scale * dst (rounded once: no contraction into the subtraction), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0.
struct Taps { int i0, i1; float l0, l1; };
__device__ __forceinline__ Taps taps(float scale, int dst, int in)
{
#pragma clang fp contract(off)                          // (hipcc otherwise fuses scale * dst into src - i0: l1 off by an ulp of src)
    const float src = scale * (float)dst;
    int i0 = (int)src;
    i0 = i0 < in - 1 ? i0 : in - 1;                     // (src <= in - 1 in exact arithmetic; keeps every load in the image)
    Taps t;
    t.i0 = i0;
    t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)i0;
    t.l0 = 1.f - t.l1;
    return t;
}

// in [nimg][H][W][ldi] -> out [nimg][2H][2W][ldo] (out already points at the slice's first channel); total = nimg * 2H * 2W * CG
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_bilinear_kernel(const T *__restrict__ in, int ldi, T *__restrict__ out, int ldo, int H, int W,
                                                                  int CG, int cg_shift, int wo_shift, int ho_shift, unsigned total, float sh, float sw)
{
    typedef UpVec<T> V;
    typedef typename V::v vec;
    const int Wo = 2 * W, Ho = 2 * H;
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        unsigned cg, xo, yo;
        const unsigned p = divmod(e, (unsigned)CG, cg_shift, cg);          // output pixel over [nimg][Ho][Wo]
        const unsigned by = divmod(p, (unsigned)Wo, wo_shift, xo);
        const unsigned b = divmod(by, (unsigned)Ho, ho_shift, yo);
        const Taps ty = taps(sh, (int)yo, H), tx = taps(sw, (int)xo, W);
        const T *img = in + (size_t)b * H * W * ldi + cg * V::N;
        const T *r0 = img + (size_t)ty.i0 * W * ldi, *r1 = img + (size_t)ty.i1 * W * ldi;
        const vec a = *reinterpret_cast<const vec *>(r0 + (size_t)tx.i0 * ldi);
        const vec bb = *reinterpret_cast<const vec *>(r0 + (size_t)tx.i1 * ldi);
        const vec c = *reinterpret_cast<const vec *>(r1 + (size_t)tx.i0 * ldi);
        const vec d = *reinterpret_cast<const vec *>(r1 + (size_t)tx.i1 * ldi);
        vec o;
#pragma unroll
        for (int k = 0; k < V::N; ++k) {
            const float v = ty.l0 * (tx.l0 * (float)a[k] + tx.l1 * (float)bb[k]) + ty.l1 * (tx.l0 * (float)c[k] + tx.l1 * (float)d[k]);
            o[k] = (T)v;                                // 16-bit tensors: one round-to-nearest-even, as the conv epilogues do
        }
        *reinterpret_cast<vec *>(out + (size_t)p * ldo + cg * V::N) = o;
    }
}

int log2_exact(unsigned v) { return (v & (v - 1)) == 0 ? __builtin_ctz(v) : -1; }

// one launch per chunk of images whose lane count stays below 2^31 (32-bit index arithmetic in the kernel)
// max_blocks: the grid's cap (0 = one lane per element)
template <typename T>
hipError_t launch_typed(const T *in, int ldi, T *out, int ldo, int B, int H, int W, int C, long long max_blocks, hipStream_t s)
{
    constexpr int N = UpVec<T>::N;
    const int CG = C / N, Ho = 2 * H, Wo = 2 * W;
    const float sh = H > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, sw = W > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const long long per_img = (long long)Ho * Wo * CG;
    if (per_img >= (1ll << 31)) return hipErrorInvalidValue;
    const int chunk = (int)std::max(1ll, std::min<long long>(B, (1ll << 31) / per_img));
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const unsigned total = (unsigned)(per_img * nb);
        const long long want = ((long long)total + 255) / 256;
        const unsigned blocks = (unsigned)std::max(1ll, max_blocks > 0 ? std::min(want, max_blocks) : want);
        hipLaunchKernelGGL(upsample2x_bilinear_kernel<T>, dim3(blocks), dim3(256), 0, s, in + (size_t)b0 * H * W * ldi, ldi,
                           out + (size_t)b0 * Ho * Wo * ldo, ldo, H, W, CG, log2_exact((unsigned)CG), log2_exact((unsigned)Wo),
                           log2_exact((unsigned)Ho), total, sh, sw);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_upsample2x_bilinear(const void *in, int ldi, void *out, int ldo, int co_off, int B, int H, int W, int C, int elem_kind,
                                      const Routing &rt, hipStream_t s)
{
    if (elem_kind < 0 || elem_kind > 2 || B < 0 || H <= 0 || W <= 0 || C <= 0 || C % 16) return hipErrorInvalidValue;
    if (ldi < C || ldo < co_off + C || co_off < 0) return hipErrorInvalidValue;
    const size_t es = elem_kind ? 2 : 4;
    const uintptr_t pi = reinterpret_cast<uintptr_t>(in), po = reinterpret_cast<uintptr_t>(out) + (size_t)co_off * es;
    if (pi % 16 || po % 16 || (ldi * es) % 16 || (ldo * es) % 16) return hipErrorInvalidValue;
    if (B == 0) return hipSuccess;
    (void)rt;                                           // the grid does not depend on the CU count (one lane per element)
    if (elem_kind == 0)
        return launch_typed(static_cast<const float *>(in), ldi, static_cast<float *>(out) + co_off, ldo, B, H, W, C, 0, s);
    if (elem_kind == 1)
        return launch_typed(static_cast<const __bf16 *>(in), ldi, static_cast<__bf16 *>(out) + co_off, ldo, B, H, W, C, 0, s);
    return launch_typed(static_cast<const _Float16 *>(in), ldi, static_cast<_Float16 *>(out) + co_off, ldo, B, H, W, C, 0, s);
}

}  // namespace miunet
