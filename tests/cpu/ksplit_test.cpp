// The split-K decision of csrc/routing.cpp (wino4_ksplit, wino_ksplit) and the slice ranges of csrc/kernels.h (ksplit_range) on a CPU:
// prints `<family> <chunks> <grid> <workspace> <ks> <begin>:<end> ...` for a sweep, which tests/test_splitk_cpu.py holds against
// tests/splitk_ref.py, and `misaligned <family> <what> <ks>` for the layouts the reduce kernel's 16-byte accesses cannot take.
//   wino4: chunks 1..200 x grids 1..160 (Cin = 16 chunks, batch = grid, one 16 x 16 tile x 128 channels per workgroup, two-block)
//   wino2: chunks 1..400 x grids 1..160 (Cin = 8 chunks, batch = grid, one 8 x 16 tile x 128 channels per workgroup)
//   workspace: `full` = the engine's 64 MiB; on every 7th chunk count and a few grids also `null` and 0..8 slabs
#include <cstdio>
#include <initializer_list>

#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/routing.h"

using namespace miunet;

namespace {

float dummy[4];

ConvArgs layer(bool f4, int chunks, int grid)
{
    ConvArgs a{};
    a.B = grid; a.H = f4 ? 16 : 8; a.W = 16;
    a.Cin = a.ldc = chunks * (f4 ? WINO4_KC : WINO_KC);
    a.Cout = a.ldo = a.CoutPad = 128;
    a.ksplit_ws = dummy; a.ksplit_ws_bytes = (size_t)64 << 20;
    return a;
}

void line(bool f4, int chunks, int grid, const char *ws, const ConvArgs &a)
{
    const int ks = f4 ? wino4_ksplit(a, 2) : wino_ksplit(a);
    std::printf("%s %d %d %s %d", f4 ? "wino4" : "wino2", chunks, grid, ws, ks);
    for (int k = 0; k < ks; ++k) {
        const KRange r = ksplit_range(chunks, ks, k, f4 ? 1 : WINO_SC / WINO_KC);
        std::printf(" %d:%d", r.begin, r.end);
    }
    std::printf("\n");
}

}  // namespace

int main()
{
    static_assert(ksplit_range(21, 5, 4, 1).begin == 20 && ksplit_range(21, 5, 4, 1).end == 21, "constexpr, usable in a kernel");
    for (int f = 0; f < 2; ++f) {
        const bool f4 = f == 0;
        for (int chunks = 1; chunks <= (f4 ? 200 : 400); ++chunks)
            for (int grid = 1; grid <= 160; ++grid) line(f4, chunks, grid, "full", layer(f4, chunks, grid));
        for (int chunks = 1; chunks <= (f4 ? 200 : 400); chunks += 7)
            for (int grid : { 1, 2, 3, 4, 7, 16, 31, 32, 33, 64, 128, 129 }) {
                ConvArgs a = layer(f4, chunks, grid);
                const size_t slab = (size_t)a.B * a.H * a.W * a.Cout * sizeof(float);
                for (int n = 0; n <= 8; ++n) {
                    char ws[8];
                    std::snprintf(ws, sizeof ws, "%d", n);
                    a.ksplit_ws_bytes = n * slab;
                    line(f4, chunks, grid, ws, a);
                }
                a.ksplit_ws = nullptr; a.ksplit_ws_bytes = (size_t)64 << 20;
                line(f4, chunks, grid, "null", a);
            }
        // a layer that splits eight ways, then one misalignment at a time
        const ConvArgs base = layer(f4, 64, 1);
        auto ks_of = [&](const ConvArgs &a) { return f4 ? wino4_ksplit(a, 2) : wino_ksplit(a); };
        ConvArgs a = base;
        std::printf("misaligned %s none %d\n", f4 ? "wino4" : "wino2", ks_of(a));
        a = base; a.Cout = 126;
        std::printf("misaligned %s Cout %d\n", f4 ? "wino4" : "wino2", ks_of(a));
        a = base; a.ldo = 130;
        std::printf("misaligned %s ldo %d\n", f4 ? "wino4" : "wino2", ks_of(a));
        a = base; a.ldo = 260; a.co_off = 130;
        std::printf("misaligned %s co_off %d\n", f4 ? "wino4" : "wino2", ks_of(a));
        a = base; a.ldo = 256; a.co_off = 128;
        std::printf("misaligned %s upper_half %d\n", f4 ? "wino4" : "wino2", ks_of(a));
        if (f4) {
            a = base; a.Cout = a.ldo = 64; a.head_w = dummy;
            std::printf("misaligned wino4 head %d\n", wino4_ksplit(a, 1));
            a.head_w = nullptr;
            std::printf("misaligned wino4 no_head %d\n", wino4_ksplit(a, 1));
        }
    }
    return 0;
}
