// wino4_asm.cpp -- host side of conv3x3_wino4a_f32 and conv3x3_wino4b_f32, the hand-scheduled persistent forms of the Winograd
// F(4x4,3x3) kernels.  Both are generated assembly (csrc/asm/gen_wino4_asm.py, gen_wino4b_asm.py on wino4_asm_lib.py -> build/wino4?_gfx950.s -> code
// object), embedded in this library as byte blobs (build/wino4?_blob.o).  An AsmKernels (kernels.h) loads the two code objects for one
// device when an engine is created and unloads them with the last handle that holds it: nothing here is process-wide.  Same weights
// (a.wpk4) and the same tensors as conv3x3_wino4_f32<2> and conv3x3_wino4s_f32 (csrc/conv_wino4.hip, conv_wino4s.hip), which serve
// every shape outside the contracts below and every layer of an engine whose code objects did not load.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "routing.h"

extern "C" const unsigned char miunet_wino4a_hsaco[];
extern "C" const unsigned char miunet_wino4a_hsaco_end[];
extern "C" const unsigned char miunet_wino4b_hsaco[];
extern "C" const unsigned char miunet_wino4b_hsaco_end[];

namespace miunet {

namespace {

// the kernels' argument block (csrc/asm/wino4_asm_lib.py: s[8:39] after two s_load_dwordx16)
struct Wino4aArgs {
    const float *in, *u, *bias;
    float *out, *pool;
    int32_t H, W, pix_in_bytes, nchunks, tiles_x, tiles_y, m_tiles, nwg;
    uint32_t magic_m, magic_x, magic_y;
    uint32_t u_pos_bytes, u_bytes, img_in_bytes, pix_out_bytes, co_off_bytes, img_out_bytes, pix_pool_bytes, img_pool_bytes;
    float relu_lo;
    int32_t grid, flags;
};
static_assert(sizeof(Wino4aArgs) == 128, "the kernel loads 128 bytes of arguments");

// What tells the two kernels apart, indexed by AsmKernels::Which.  A workgroup takes a block of 16 x tile_w pixels x cout_group channels:
// wino4a 16 tiles x 128 channels, wino4b 32 tiles x 64 channels (a wave = 32 tiles x 16 channels, V single-buffered).
struct AsmKernel {
    const unsigned char *blob;
    const char *symbol;
    int tile_w, cout_group;
    bool (*shape_ok)(const ConvArgs &);
};
const AsmKernel kKernels[2] = {
    { miunet_wino4a_hsaco, "conv3x3_wino4a_f32", 16, 128, conv3x3_wino4a_shape_ok },
    { miunet_wino4b_hsaco, "conv3x3_wino4b_f32", 32, 64, conv3x3_wino4b_shape_ok },
};

// ceil(2^32 / d); 0 encodes d == 1.  q = mulhi(n, magic) == n / d for every n with n * d < 2^32.
uint32_t magic_of(uint32_t d) { return d <= 1 ? 0u : (uint32_t)(((1ull << 32) + d - 1) / d); }

// the caller's device while `device` is current
struct DeviceScope {
    int prev = 0;
    bool have;
    explicit DeviceScope(int device) : have(hipGetDevice(&prev) == hipSuccess) { (void)hipSetDevice(device); }
    ~DeviceScope() { if (have) (void)hipSetDevice(prev); }
};

}  // namespace

AsmKernels::AsmKernels(int device) : device_(device)
{
    DeviceScope on(device_);
    hipDeviceProp_t p;
    if (hipError_t e = hipGetDeviceProperties(&p, device_); e != hipSuccess) {
        error_ = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return;
    }
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
        error_ = std::string("the code objects are gfx950, the device is ") + p.gcnArchName;
        return;
    }
    for (int w = 0; w < 2 && error_.empty(); ++w) {
        const AsmKernel &k = kKernels[w];
        const void *image = k.blob;
#ifdef MIUNET_EXPERIMENTS                              // lab build only: a code object FILE instead of the embedded one (same-card A/Bs of kernel variants)
        std::vector<char> file_image;
        if (const char *path = getenv(w == WINO4A ? "MIUNET_WINO4A_HSACO" : "MIUNET_WINO4B_HSACO")) {
            if (FILE *f = fopen(path, "rb")) {
                fseek(f, 0, SEEK_END); file_image.resize((size_t)ftell(f)); fseek(f, 0, SEEK_SET);
                if (fread(file_image.data(), 1, file_image.size(), f) == file_image.size()) image = file_image.data();
                fclose(f);
            }
        }
#endif
        hipError_t e = hipModuleLoadData(&mod_[w], image);
        if (e != hipSuccess) {
            mod_[w] = nullptr;
            error_ = std::string("hipModuleLoadData(") + k.symbol + "): " + hipGetErrorString(e);
        } else if (e = hipModuleGetFunction(&fn_[w], mod_[w], k.symbol); e != hipSuccess) {
            error_ = std::string("hipModuleGetFunction(") + k.symbol + "): " + hipGetErrorString(e);
        }
    }
    if (!error_.empty()) unload();                     // all or nothing: an owner that is not available() holds no module
}

AsmKernels::~AsmKernels()
{
    DeviceScope on(device_);
    unload();
}

void AsmKernels::unload()
{
    for (int w = 0; w < 2; ++w) {
        if (mod_[w]) (void)hipModuleUnload(mod_[w]);
        mod_[w] = nullptr;
        fn_[w] = nullptr;
    }
}

hipError_t launch_conv3x3_wino4_asm(const AsmKernels *owner, AsmKernels::Which which, const ConvArgs &a, hipStream_t s)
{
    const AsmKernel &kd = kKernels[which];
    if (!kd.shape_ok(a)) return hipErrorInvalidValue;
    if (!owner || !owner->available()) return hipErrorSharedObjectInitFailed;
    Wino4aArgs k;
    memset(&k, 0, sizeof k);
    k.in = a.in; k.u = a.wpk4; k.bias = a.bias; k.out = a.out; k.pool = a.pool_out;
    k.H = a.H; k.W = a.W; k.pix_in_bytes = a.ldc * 4; k.nchunks = a.Cin / 16;
    k.tiles_x = a.W / kd.tile_w; k.tiles_y = a.H / 16; k.m_tiles = k.tiles_x * k.tiles_y * a.B; k.nwg = k.m_tiles * (a.Cout / kd.cout_group);
    k.magic_m = magic_of((uint32_t)k.m_tiles); k.magic_x = magic_of((uint32_t)k.tiles_x); k.magic_y = magic_of((uint32_t)k.tiles_y);
    k.u_pos_bytes = (uint32_t)a.CoutPad * 64u;
    k.u_bytes = (uint32_t)k.nchunks * 36u * k.u_pos_bytes;
    k.img_in_bytes = (uint32_t)a.H * a.W * a.ldc * 4u;
    k.pix_out_bytes = (uint32_t)a.ldo * 4u; k.co_off_bytes = (uint32_t)a.co_off * 4u;
    k.img_out_bytes = (uint32_t)a.H * a.W * a.ldo * 4u;
    const bool pool = a.pool_out != nullptr;
    k.pix_pool_bytes = pool ? (uint32_t)a.pool_ld * 4u : 0u;
    k.img_pool_bytes = pool ? (uint32_t)(a.H / 2) * (a.W / 2) * a.pool_ld * 4u : 0u;
    k.relu_lo = a.relu ? 0.f : -__builtin_inff();
    const int cus = a.rt.cus;
    k.grid = k.nwg < cus ? k.nwg : cus;             // persistent: one workgroup per CU walks its XCD's tiles
    k.flags = pool ? 1 : 0;
    size_t size = sizeof k;
    void *extra[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, &k, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END };
    return hipModuleLaunchKernel(owner->function(which), (unsigned)k.grid, 1, 1, 256, 1, 1, 0, s, nullptr, extra);
}

}  // namespace miunet
