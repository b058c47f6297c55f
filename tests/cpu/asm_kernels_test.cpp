// asm_kernels_test.cpp -- csrc/wino4_asm.cpp on a CPU: who owns the assembly kernels' code objects, and what their one launcher hands
// to the kernels.  The HIP module calls and the four blob symbols are stubs in this file: a "module" is a counted token, a "launch"
// keeps the 128-byte argument block it was given.  The expected argument blocks are the values the two launch functions the launcher
// replaced (launch_conv3x3_wino4a / _wino4b) computed for the same shapes, worked out by hand from their code.
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include asm_kernels_test.cpp ../../<pkg>/csrc/{wino4_asm,routing}.cpp
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
#include <string>

#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/kernels.h"
#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/routing.h"

extern "C" {
extern const unsigned char miunet_wino4a_hsaco[] = { 0xA };
extern const unsigned char miunet_wino4a_hsaco_end[] = { 0 };
extern const unsigned char miunet_wino4b_hsaco[] = { 0xB };
extern const unsigned char miunet_wino4b_hsaco_end[] = { 0 };
}

namespace {

// ---- the stub's state
struct Module { int which; };                       // 0: loaded from the wino4a blob, 1: from the wino4b blob
struct Function { const Module *mod; std::string name; };
int g_device = 0;                                   // the "current device"
std::string g_arch = "gfx950:sramecc+:xnack-";
int g_fail_load = -1, g_fail_lookup = -1;           // which blob's load / look-up fails
int g_loads[2], g_unloads[2], g_unload_device[2];
std::set<const Module *> g_live, g_modules;         // loaded now; ever loaded
std::set<const Function *> g_functions;
struct LaunchRecord { int n = 0; const Function *fn; unsigned grid[3], block[3], lds; hipStream_t stream; unsigned char args[128]; size_t size; } g_launch;

void reset_stub()
{
    g_device = 0; g_arch = "gfx950:sramecc+:xnack-"; g_fail_load = g_fail_lookup = -1;
    for (int i = 0; i < 2; ++i) g_loads[i] = g_unloads[i] = 0, g_unload_device[i] = -1;
    g_launch = LaunchRecord{};
}

}  // namespace

extern "C" {
hipError_t hipGetDevice(int *d) { *d = g_device; return hipSuccess; }
hipError_t hipSetDevice(int d) { g_device = d; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int)
{
    memset(p, 0, sizeof *p);
    snprintf(p->gcnArchName, sizeof p->gcnArchName, "%s", g_arch.c_str());
    p->multiProcessorCount = 256;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
hipError_t hipModuleLoadData(hipModule_t *m, const void *image)
{
    const int which = image == miunet_wino4a_hsaco ? 0 : image == miunet_wino4b_hsaco ? 1 : -1;
    if (which < 0) return hipErrorInvalidImage;
    if (which == g_fail_load) return hipErrorSharedObjectInitFailed;
    Module *mod = new Module{ which };
    g_live.insert(mod);
    g_modules.insert(mod);
    ++g_loads[which];
    *m = reinterpret_cast<hipModule_t>(mod);
    return hipSuccess;
}
hipError_t hipModuleGetFunction(hipFunction_t *f, hipModule_t m, const char *name)
{
    const Module *mod = reinterpret_cast<const Module *>(m);
    if (!g_live.count(mod)) return hipErrorInvalidHandle;
    if (mod->which == g_fail_lookup || strcmp(name, mod->which == 0 ? "conv3x3_wino4a_f32" : "conv3x3_wino4b_f32") != 0) return hipErrorNotFound;
    Function *fn = new Function{ mod, name };
    g_functions.insert(fn);
    *f = reinterpret_cast<hipFunction_t>(fn);
    return hipSuccess;
}
hipError_t hipModuleUnload(hipModule_t m)
{
    const Module *mod = reinterpret_cast<const Module *>(m);
    if (!g_live.erase(mod)) return hipErrorInvalidHandle;
    ++g_unloads[mod->which];
    g_unload_device[mod->which] = g_device;
    return hipSuccess;                              // (the token is kept: a launch on a function of an unloaded module is detected)
}
hipError_t hipModuleLaunchKernel(hipFunction_t f, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned by, unsigned bz, unsigned lds,
                                 hipStream_t s, void **params, void **extra)
{
    const Function *fn = reinterpret_cast<const Function *>(f);
    if (!g_functions.count(fn) || !g_live.count(fn->mod) || params != nullptr || !extra) return hipErrorInvalidHandle;
    if (extra[0] != HIP_LAUNCH_PARAM_BUFFER_POINTER || extra[2] != HIP_LAUNCH_PARAM_BUFFER_SIZE || extra[4] != HIP_LAUNCH_PARAM_END) return hipErrorInvalidValue;
    LaunchRecord &r = g_launch;
    ++r.n; r.fn = fn; r.grid[0] = gx; r.grid[1] = gy; r.grid[2] = gz; r.block[0] = bx; r.block[1] = by; r.block[2] = bz; r.lds = lds; r.stream = s;
    r.size = *static_cast<size_t *>(extra[3]);
    if (r.size != sizeof r.args) return hipErrorInvalidValue;
    memcpy(r.args, extra[1], sizeof r.args);
    return hipSuccess;
}
}

using namespace miunet;

namespace {

int bad = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++bad; }        \
    } while (0)

// the kernels' argument block as csrc/asm/gen_wino4_asm.py reads it (a copy: the library keeps its own private)
struct Args {
    const float *in, *u, *bias;
    float *out, *pool;
    int32_t H, W, pix_in_bytes, nchunks, tiles_x, tiles_y, m_tiles, nwg;
    uint32_t magic_m, magic_x, magic_y;
    uint32_t u_pos_bytes, u_bytes, img_in_bytes, pix_out_bytes, co_off_bytes, img_out_bytes, pix_pool_bytes, img_pool_bytes;
    float relu_lo;
    int32_t grid, flags;
};
static_assert(sizeof(Args) == 128, "128 bytes of arguments");

float buf[8];

// down2.c1-like: 2 images of 32 x 48, 128 -> 256 channels into the second half of a 512-channel concat buffer, pooled, ReLU
ConvArgs shape_a()
{
    ConvArgs a{};
    a.in = buf; a.wpk4 = buf + 1; a.bias = buf + 2; a.out = buf + 3; a.pool_out = buf + 4;
    a.B = 2; a.H = 32; a.W = 48; a.Cin = 128; a.ldc = 128; a.Cout = 256; a.CoutPad = 256; a.ldo = 512; a.co_off = 256; a.relu = 1; a.pool_ld = 256;
    a.rt.cus = 256;
    return a;
}

// 3 images of 16 x 64, 96 -> 64 channels (packed to 128), no pooling, no ReLU, on a "chip" of 4 CUs
ConvArgs shape_b()
{
    ConvArgs a{};
    a.in = buf; a.wpk4 = buf + 1; a.bias = buf + 2; a.out = buf + 3;
    a.B = 3; a.H = 16; a.W = 64; a.Cin = 96; a.ldc = 96; a.Cout = 64; a.CoutPad = 128; a.ldo = 64; a.co_off = 0; a.relu = 0;
    a.rt.cus = 4;
    return a;
}

void test_ownership()
{
    reset_stub();
    g_device = 3;                                    // the caller's device is not the owner's
    {
        auto a = std::make_shared<AsmKernels>(1);
        CHECK(a->available() && a->error().empty());
        CHECK(g_loads[0] == 1 && g_loads[1] == 1 && g_live.size() == 2);
        CHECK(g_device == 3);                        // restored
        CHECK(a->function(AsmKernels::WINO4A) != nullptr && a->function(AsmKernels::WINO4B) != nullptr);
        {
            AsmKernels b(1);                         // a second owner on the same device: modules of its own
            CHECK(b.available() && g_loads[0] == 2 && g_loads[1] == 2 && g_live.size() == 4);
            CHECK(b.function(AsmKernels::WINO4A) != a->function(AsmKernels::WINO4A));
            CHECK(reinterpret_cast<const Function *>(b.function(AsmKernels::WINO4B))->mod != reinterpret_cast<const Function *>(a->function(AsmKernels::WINO4B))->mod);
        }
        CHECK(g_unloads[0] == 1 && g_unloads[1] == 1 && g_live.size() == 2);      // b's went, a's stayed
        std::shared_ptr<AsmKernels> clone = a;       // a clone's hold
        a.reset();                                   // the first holder goes
        CHECK(g_unloads[0] == 1 && g_unloads[1] == 1 && g_live.size() == 2);
        CHECK(launch_conv3x3_wino4_asm(clone.get(), AsmKernels::WINO4A, shape_a(), nullptr) == hipSuccess && g_launch.n == 1);
        g_device = 5;
    }
    CHECK(g_loads[0] == 2 && g_loads[1] == 2 && g_unloads[0] == 2 && g_unloads[1] == 2 && g_live.empty());   // one unload per load
    CHECK(g_unload_device[0] == 1 && g_unload_device[1] == 1 && g_device == 5);   // unloaded on the owner's device, the caller's restored
}

void test_failures()
{
    for (int which = 0; which < 2; ++which) {
        reset_stub();
        g_fail_load = which;
        {
            AsmKernels k(0);
            CHECK(!k.available() && !k.error().empty() && k.error().find("hipModuleLoadData") != std::string::npos);
            CHECK(g_live.empty() && g_loads[which] == 0 && g_unloads[1 - which] == g_loads[1 - which]);     // whatever did load is gone
            CHECK(k.function(AsmKernels::WINO4A) == nullptr && k.function(AsmKernels::WINO4B) == nullptr);
            CHECK(launch_conv3x3_wino4_asm(&k, AsmKernels::WINO4A, shape_a(), nullptr) != hipSuccess && g_launch.n == 0);
        }
        CHECK(g_unloads[0] == g_loads[0] && g_unloads[1] == g_loads[1]);          // ... once
        reset_stub();
        g_fail_lookup = which;
        {
            AsmKernels k(0);
            CHECK(!k.available() && k.error().find("hipModuleGetFunction") != std::string::npos);
            CHECK(g_live.empty() && g_loads[which] == 1 && g_unloads[0] == g_loads[0] && g_unloads[1] == g_loads[1]);
        }
        CHECK(g_unloads[0] == g_loads[0] && g_unloads[1] == g_loads[1]);
    }
    reset_stub();
    g_arch = "gfx942:sramecc+:xnack-";
    {
        AsmKernels k(0);
        CHECK(!k.available() && k.error().find("gfx942") != std::string::npos);
        CHECK(g_loads[0] == 0 && g_loads[1] == 0 && g_live.empty());
    }
    reset_stub();
    CHECK(launch_conv3x3_wino4_asm(nullptr, AsmKernels::WINO4B, shape_b(), nullptr) != hipSuccess && g_launch.n == 0);   // no owner: an error, no launch
}

void test_contracts()
{
    reset_stub();
    AsmKernels k(0);
    auto refused = [&](AsmKernels::Which w, ConvArgs a) { return launch_conv3x3_wino4_asm(&k, w, a, nullptr) == hipErrorInvalidValue; };
    ConvArgs a = shape_a();
    CHECK(conv3x3_wino4a_shape_ok(a));
    a = shape_a(); a.H = 20; CHECK(refused(AsmKernels::WINO4A, a));              // ragged H
    a = shape_a(); a.W = 40; CHECK(refused(AsmKernels::WINO4A, a));              // W % 16
    a = shape_a(); a.Cin = 48; CHECK(refused(AsmKernels::WINO4A, a));            // Cin % 32
    a = shape_a(); a.Cin = 32; CHECK(refused(AsmKernels::WINO4A, a));            // fewer than four K chunks
    a = shape_a(); a.Cout = 64; CHECK(refused(AsmKernels::WINO4A, a));           // Cout % 128
    a = shape_a(); a.wpk4 = nullptr; CHECK(refused(AsmKernels::WINO4A, a));      // not packed for F(4x4)
    a = shape_a(); a.head_w = buf; CHECK(refused(AsmKernels::WINO4A, a));        // fused head
    a = shape_a(); a.out_lp = 1; CHECK(refused(AsmKernels::WINO4A, a));
    a = shape_a(); a.co_off = 2; CHECK(refused(AsmKernels::WINO4A, a));
    ConvArgs b = shape_b();
    CHECK(conv3x3_wino4b_shape_ok(b));
    CHECK(refused(AsmKernels::WINO4A, b));                                       // 64 channels: wino4b's, not wino4a's
    b = shape_b(); b.W = 48; CHECK(refused(AsmKernels::WINO4B, b));              // W % 32
    b = shape_b(); b.H = 24; CHECK(refused(AsmKernels::WINO4B, b));
    b = shape_b(); b.Cout = 96; CHECK(refused(AsmKernels::WINO4B, b));           // Cout % 64
    b = shape_b(); b.Cin = 80; CHECK(refused(AsmKernels::WINO4B, b));
    b = shape_b(); b.first_img = reinterpret_cast<const uint8_t *>(buf); CHECK(refused(AsmKernels::WINO4B, b));   // no fused first layer
    b = shape_b(); b.pool_out = buf; b.pool_ld = 6; CHECK(refused(AsmKernels::WINO4B, b));
    CHECK(g_launch.n == 0);
}

void test_argument_blocks()
{
    reset_stub();
    AsmKernels k(0);
    hipStream_t stream = reinterpret_cast<hipStream_t>(buf + 7);
    Args g;
    {
        CHECK(launch_conv3x3_wino4_asm(&k, AsmKernels::WINO4A, shape_a(), stream) == hipSuccess && g_launch.n == 1);
        memcpy(&g, g_launch.args, sizeof g);
        CHECK(g_launch.fn == reinterpret_cast<const Function *>(k.function(AsmKernels::WINO4A)) && g_launch.fn->name == "conv3x3_wino4a_f32" && g_launch.fn->mod->which == 0);
        CHECK(g_launch.grid[0] == 24 && g_launch.grid[1] == 1 && g_launch.grid[2] == 1);
        CHECK(g_launch.block[0] == 256 && g_launch.block[1] == 1 && g_launch.block[2] == 1 && g_launch.lds == 0 && g_launch.stream == stream);
        CHECK(g.in == buf && g.u == buf + 1 && g.bias == buf + 2 && g.out == buf + 3 && g.pool == buf + 4);
        CHECK(g.H == 32 && g.W == 48 && g.pix_in_bytes == 512 && g.nchunks == 8);
        CHECK(g.tiles_x == 3 && g.tiles_y == 2 && g.m_tiles == 12 && g.nwg == 24);                        // 16-pixel tiles, 128-channel groups
        CHECK(g.magic_m == 357913942u && g.magic_x == 1431655766u && g.magic_y == 2147483648u);           // ceil(2^32 / 12), / 3, / 2
        CHECK(g.u_pos_bytes == 16384u && g.u_bytes == 4718592u && g.img_in_bytes == 786432u);
        CHECK(g.pix_out_bytes == 2048u && g.co_off_bytes == 1024u && g.img_out_bytes == 3145728u);
        CHECK(g.pix_pool_bytes == 1024u && g.img_pool_bytes == 393216u);
        CHECK(g.relu_lo == 0.f && g.grid == 24 && g.flags == 1);
    }
    {
        CHECK(launch_conv3x3_wino4_asm(&k, AsmKernels::WINO4B, shape_b(), nullptr) == hipSuccess && g_launch.n == 2);
        memcpy(&g, g_launch.args, sizeof g);
        CHECK(g_launch.fn == reinterpret_cast<const Function *>(k.function(AsmKernels::WINO4B)) && g_launch.fn->name == "conv3x3_wino4b_f32" && g_launch.fn->mod->which == 1);
        CHECK(g_launch.grid[0] == 4 && g_launch.grid[1] == 1 && g_launch.grid[2] == 1 && g_launch.block[0] == 256 && g_launch.stream == nullptr);
        CHECK(g.in == buf && g.u == buf + 1 && g.bias == buf + 2 && g.out == buf + 3 && g.pool == nullptr);
        CHECK(g.H == 16 && g.W == 64 && g.pix_in_bytes == 384 && g.nchunks == 6);
        CHECK(g.tiles_x == 2 && g.tiles_y == 1 && g.m_tiles == 6 && g.nwg == 6);                          // 32-pixel tiles, 64-channel groups
        CHECK(g.magic_m == 715827883u && g.magic_x == 2147483648u && g.magic_y == 0u);                    // ceil(2^32 / 6), / 2, d == 1
        CHECK(g.u_pos_bytes == 8192u && g.u_bytes == 1769472u && g.img_in_bytes == 393216u);
        CHECK(g.pix_out_bytes == 256u && g.co_off_bytes == 0u && g.img_out_bytes == 262144u);
        CHECK(g.pix_pool_bytes == 0u && g.img_pool_bytes == 0u);
        CHECK(g.relu_lo == -INFINITY && g.grid == 4 && g.flags == 0);                             // 6 workgroups on 4 CUs: persistent
    }
}

}  // namespace

int main()
{
    test_ownership();
    test_failures();
    test_contracts();
    test_argument_blocks();
    for (const Function *f : g_functions) delete f;
    for (const Module *m : g_modules) delete m;
    if (bad) { printf("%d assembly-kernel owner checks failed\n", bad); return 1; }
    printf("all assembly-kernel owner checks passed\n");
    return 0;
}
