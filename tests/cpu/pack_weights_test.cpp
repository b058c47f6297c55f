// pack_weights_test.cpp -- what miunet::engine_pack_weights of the built libmiunet.so makes of a weight file, for each conv
// algorithm 1..5: the packed blob's length, a 64-bit FNV-1a hash of its bytes and every offset of the layout, one JSON object per
// line.  tests/test_weights_cpu.py compares the lines with tests/golden/packed_weights.json, exactly.
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include pack_weights_test.cpp -L<pkg> -lmiunet -Wl,-rpath,<pkg>
// Run: pack_weights_test <in_ch> <base> <levels> <classes> <weight file>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/engine_internal.h"

using namespace miunet;

int main(int argc, char **argv)
{
    if (argc != 6) { printf("usage: pack_weights_test <in_ch> <base> <levels> <classes> <weight file>\n"); return 2; }
    mi_unet_config cfg{};
    cfg.height = cfg.width = 64; cfg.in_ch = atoi(argv[1]); cfg.base = atoi(argv[2]); cfg.levels = atoi(argv[3]); cfg.classes = atoi(argv[4]);
    cfg.max_batch = 1;
    std::ifstream f(argv[5], std::ios::binary);
    const std::vector<char> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    for (int algo = 1; algo <= 5; ++algo) {
        HostWeights hw;
        if (int rc = engine_pack_weights(cfg, algo, file.data(), file.size(), hw)) { printf("engine_pack_weights failed: %d\n", rc); return 1; }
        unsigned long long h = 0xcbf29ce484222325ull;
        const unsigned char *p = reinterpret_cast<const unsigned char *>(hw.blob.data());
        for (size_t i = 0; i < hw.blob.size() * sizeof(float); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
        printf("{\"algo\": %d, \"up_mode\": %d, \"floats\": %zu, \"fnv1a64\": \"%016llx\", ", algo, hw.up_mode, hw.blob.size(), h);
        auto offs = [](const char *name, const std::vector<HostWeights::Off> &v) {
            printf("\"%s\": [", name);
            for (size_t i = 0; i < v.size(); ++i) printf("%s[%zu, %zu, %zu]", i ? ", " : "", v[i].w, v[i].shift, v[i].w4);
            printf("], ");
        };
        offs("conv", hw.conv);
        offs("convT", hw.convT);
        printf("\"head\": [%zu, %zu]}\n", hw.head.w, hw.head.shift);
    }
    return 0;
}
