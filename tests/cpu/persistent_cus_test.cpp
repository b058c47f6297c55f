// persistent_cus_test.cpp -- Routing::cus as csrc/routing.cpp computes it (persistent_cus), on a CPU: the device's CU count floored at 8,
// MIUNET_CUS clamped to [8, that].  Prints one line "<device_cus> <text or -> <result>" per case for tests/test_persist_cpu.py, which
// holds the same cases against its model (tests/persist_ref.py clamp_cus).
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include persistent_cus_test.cpp ../../<pkg>/csrc/routing.cpp
#include <cstdio>

#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/routing.h"

int main()
{
    const int devices[] = { 1, 2, 7, 8, 9, 64, 104, 256, 304 };
    const char *texts[] = { nullptr, "", "0", "-3", "1", "7", "8", "9", "12", "16", "23", "255", "256", "257", "1000000", "junk" };
    for (int d : devices)
        for (const char *t : texts) printf("%d %s %d\n", d, t == nullptr ? "-" : *t ? t : "empty", miunet::persistent_cus(d, t));
    return 0;
}
