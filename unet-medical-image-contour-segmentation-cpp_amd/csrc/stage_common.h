// stage_common.h -- what the host halves of the stages behind the network share (score.cpp, score_volume.cpp, volume.cpp,
// volume_clean.cpp, volume_mesh.cpp, volume_measure.cpp, volume_spatial.cpp, volume_match.cpp, volume_texture.cpp, volume_interp.cpp, volume_zones.cpp, volume_nbhood.cpp, volume_split.cpp, volume_skeleton.cpp, volume_branches.cpp): how a stage file is compiled, and the
// argument checks that more than one of them makes with the same text.  What only the texture stages share (volume_texture.cpp,
// volume_zones.cpp, volume_nbhood.cpp) is in texture_common.h, which includes this file.
// With MIUNET_NO_DEVICE only a stage's host arithmetic is compiled, with no HIP header: a plain C++ compiler builds it into a program that
// supplies miunet::engine_fail (tests/cpu/*_host_test.cpp).  Without it the stage also has its entry point on the handle.
#pragma once
#include <cstdint>
#include <string>

#ifdef MIUNET_NO_DEVICE
#include "../../include/mi_unet.h"
namespace miunet {
int engine_fail(int code, const std::string &msg);
inline int fail(int code, const std::string &msg) { return engine_fail(code, msg); }
}
#else
#include <hip/hip_runtime.h>

#include "engine_handle.h"
#endif

namespace miunet {

// The checks below take the entry point's name as `f` and return MI_UNET_OK, or MI_UNET_EARG with the message set.  A stage's own
// check_*_args calls them where its order of checks has them; a check whose text or bound is a stage's own stays in that stage.

// n values of 0 .. 255, 1 .. max of them, none listed twice
inline int check_values(const std::string &f, const int *values, int n, int max)
{
    if (n < 1 || n > max) return fail(MI_UNET_EARG, f + ": " + std::to_string(n) + " values (1 .. " + std::to_string(max) + ")");
    for (int k = 0; k < n; ++k) {
        if (values[k] < 0 || values[k] > 255) return fail(MI_UNET_EARG, f + ": value " + std::to_string(values[k]) + " is not a byte");
        for (int j = 0; j < k; ++j)
            if (values[j] == values[k]) return fail(MI_UNET_EARG, f + ": value " + std::to_string(values[k]) + " is listed twice");
    }
    return MI_UNET_OK;
}

inline std::string sides_text(int D, int H, int W) { return std::to_string(D) + " x " + std::to_string(H) + " x " + std::to_string(W); }

inline int check_sides_min1(const std::string &f, int D, int H, int W)
{
    if (D < 1 || H < 1 || W < 1) return fail(MI_UNET_EARG, f + ": " + sides_text(D, H, W) + " (every side at least 1)");
    return MI_UNET_OK;
}

inline bool sides_within(int D, int H, int W, int max) { return D >= 1 && H >= 1 && W >= 1 && D <= max && H <= max && W <= max; }

inline int check_sides_max(const std::string &f, int D, int H, int W, int max)
{
    if (!sides_within(D, H, W, max))
        return fail(MI_UNET_EARG, f + ": " + sides_text(D, H, W) + " is outside 1 .. " + std::to_string(max) + " per side");
    return MI_UNET_OK;
}

inline int check_units_min1(const std::string &f, const int *units, int count = 3)      // (2: the in-plane units alone)
{
    for (int a = 0; a < count; ++a)
        if (units[a] < 1) return fail(MI_UNET_EARG, f + ": spacing unit " + std::to_string(units[a]) + " (at least 1)");
    return MI_UNET_OK;
}

// ((W - 1) ux)^2 + ((H - 1) uy)^2 + ((D - 1) uz)^2 < 2^31, without overflow for any unit: a term of 46341 or more fails by itself
// (the limit of mi_unet_score_volume, which mi_unet_volume_measure and mi_unet_volume_spatial take over)
template <class U>
inline bool d2_fits(int D, int H, int W, const U *units)
{
    const int64_t side[3] = { W - 1, H - 1, D - 1 };
    int64_t sum = 0;
    for (int a = 0; a < 3; ++a) {
        if (side[a] != 0 && units[a] > 46340 / side[a]) return false;
        sum += side[a] * units[a] * side[a] * units[a];
    }
    return sum < ((int64_t)1 << 31);
}

// a * b * c * d < 2^31 for factors of at least 1, step by step: the product itself could pass 64 bits
inline bool product_below_2_31(long long a, long long b, long long c, long long d)
{
    long long v = 0x7FFFFFFFLL / a;
    v /= b;
    v /= c;
    return v >= d;
}

}  // namespace miunet
