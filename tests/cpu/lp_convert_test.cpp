// lp_convert_test.cpp -- the host's 16-bit converters (weights.cpp: bf16_bits, fp16_bits, bf16_to_float, fp16_to_float) of the built
// libmiunet.so.  The layer hook rounds its operands with them and converts 16-bit results back, so the GPU tests on special values
// stand on these four functions.
//   no argument: round-trips all 2^16 patterns of either format (a NaN stays a NaN, its payload may change; every other pattern returns
//     its bits), then every midpoint between adjacent finite values and the value on either side of it, both signs (round to nearest,
//     ties to even; the midpoint above the largest finite value goes to infinity).  Prints one line per failure, exit status 1 if any.
//   bf16|fp16 <fp32 bits in hex>...: prints the 16-bit pattern of each argument, one per line (tests/test_special_values_cpu.py
//     compares them with the tables of tests/special_ref.py).
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include lp_convert_test.cpp -L<pkg> -lmiunet -Wl,-rpath,<pkg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/engine_internal.h"

using namespace miunet;

namespace {

int g_fail = 0;

void fail(const char *what, unsigned a, unsigned got, unsigned want)
{
    if (++g_fail <= 20) printf("FAIL %s: input %08x gives %04x, expected %04x\n", what, a, got, want);
}

float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Format {
    const char *name;
    uint16_t (*to)(float);
    float (*from)(uint16_t);
    unsigned exp_mask, man_mask, max_finite;      // of the 16-bit pattern
    double above_max;                              // the value the format would hold one step above max_finite
};
const Format kBf16 = { "bf16", bf16_bits, bf16_to_float, 0x7F80u, 0x007Fu, 0x7F7Fu, 3.402823669209384634633746074317682e+38 /* 2^128 */ };
const Format kFp16 = { "fp16", fp16_bits, fp16_to_float, 0x7C00u, 0x03FFu, 0x7BFFu, 65536.0 };

void round_trip(const Format &f)
{
    for (unsigned b = 0; b < 0x10000u; ++b) {
        const float v = f.from((uint16_t)b);
        const unsigned back = f.to(v);
        const bool nan = (b & f.exp_mask) == f.exp_mask && (b & f.man_mask);
        if (nan) {
            if (!std::isnan(v) || !((back & f.exp_mask) == f.exp_mask && (back & f.man_mask)))
                fail((std::string(f.name) + " NaN round trip").c_str(), b, back, b);
        } else if (back != b || std::isnan(v)) {
            fail((std::string(f.name) + " round trip").c_str(), b, back, b);
        }
    }
}

void midpoints(const Format &f)
{
    for (unsigned h = 0; h <= f.max_finite; ++h) {
        const double lo = f.from((uint16_t)h), hi = h == f.max_finite ? f.above_max : (double)f.from((uint16_t)(h + 1));
        const float mid = (float)((lo + hi) / 2);                     // exact: one more significand bit than the format has
        if ((double)mid != (lo + hi) / 2) { fail((std::string(f.name) + " midpoint not exact").c_str(), h, 0, 0); continue; }
        const unsigned even = (h & 1) ? h + 1 : h;                    // h + 1 above max_finite is the pattern of infinity
        for (unsigned sign = 0; sign < 2; ++sign) {
            const uint32_t s32 = sign << 31;
            const unsigned s16 = sign << 15;
            const uint32_t m = bits_of(mid);
            if (f.to(from_bits(m | s32)) != (even | s16)) fail((std::string(f.name) + " tie").c_str(), m | s32, f.to(from_bits(m | s32)), even | s16);
            if (f.to(from_bits((m - 1) | s32)) != (h | s16)) fail((std::string(f.name) + " below tie").c_str(), (m - 1) | s32, f.to(from_bits((m - 1) | s32)), h | s16);
            if (f.to(from_bits((m + 1) | s32)) != ((h + 1) | s16)) fail((std::string(f.name) + " above tie").c_str(), (m + 1) | s32, f.to(from_bits((m + 1) | s32)), (h + 1) | s16);
        }
    }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2) {
        const Format *f = !strcmp(argv[1], "bf16") ? &kBf16 : !strcmp(argv[1], "fp16") ? &kFp16 : nullptr;
        if (!f) { printf("usage: lp_convert_test [bf16|fp16 <fp32 bits in hex>...]\n"); return 2; }
        for (int i = 2; i < argc; ++i) printf("%04x\n", (unsigned)f->to(from_bits((uint32_t)strtoul(argv[i], nullptr, 16))));
        return 0;
    }
    for (const Format *f : { &kBf16, &kFp16 }) {
        round_trip(*f);
        midpoints(*f);
    }
    // infinities and NaN from fp32
    if (bf16_bits(INFINITY) != 0x7F80u || bf16_bits(-INFINITY) != 0xFF80u) fail("bf16 inf", 0x7F800000u, bf16_bits(INFINITY), 0x7F80u);
    if (fp16_bits(INFINITY) != 0x7C00u || fp16_bits(-INFINITY) != 0xFC00u) fail("fp16 inf", 0x7F800000u, fp16_bits(INFINITY), 0x7C00u);
    for (uint32_t n : { 0x7FC00000u, 0x7F800001u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0xFF800001u }) {
        if (!std::isnan(bf16_to_float(bf16_bits(from_bits(n))))) fail("bf16 NaN from fp32", n, bf16_bits(from_bits(n)), 0x7FC0u);
        if (!std::isnan(fp16_to_float(fp16_bits(from_bits(n))))) fail("fp16 NaN from fp32", n, fp16_bits(from_bits(n)), 0x7E00u);
    }
    printf(g_fail ? "%d failures\n" : "ok\n", g_fail);
    return g_fail ? 1 : 0;
}
