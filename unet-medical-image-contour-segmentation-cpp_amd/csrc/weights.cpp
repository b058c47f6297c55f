// weights.cpp -- the "MIUNETW1" weight file (miunet/spec.py) on its way to the device: BN folding, every packed layout the
// kernels read (one size function and one packer per layout) and the 16-bit conversions.  Host code only, no HIP runtime call:
// the CPU tests build it with g++ next to routing.cpp and plan.cpp.  This thread's error string lives here too, so those tests
// link the real engine_fail.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"

namespace miunet {

static thread_local std::string g_err;

int engine_fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

const std::string &engine_last_error() { return g_err; }

size_t round_up(size_t v, size_t g) { return (v + g - 1) / g * g; }

// float -> bfloat16 bits, round-to-nearest-even (what the device's v_cvt_pk_bf16_f32 does to the activations)
uint16_t bf16_bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x40);   // quiet NaN
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// float -> IEEE binary16 bits, round-to-nearest-even (v_cvt_f16_f32 semantics incl. subnormals and overflow to inf)
uint16_t fp16_bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const int32_t e = (int32_t)((u >> 23) & 0xFF) - 127;
    uint32_t m = u & 0x7FFFFFu;
    if (e == 128) return (uint16_t)(sign | 0x7C00u | (m ? 0x200u : 0));                 // inf / NaN
    if (e > 15) return (uint16_t)(sign | 0x7C00u);                                       // overflow
    if (e >= -14) {                                                                      // normal
        uint32_t h = ((uint32_t)(e + 15) << 10) | (m >> 13);
        const uint32_t rem = m & 0x1FFFu;
        if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) ++h;                           // carries into the exponent correctly
        return (uint16_t)(sign | h);
    }
    if (e < -25) return (uint16_t)sign;                                                  // underflow to zero
    m |= 0x800000u;                                                                      // subnormal: shift the 24-bit significand
    const int shift = -14 - e + 13;
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (h & 1))) ++h;
    return (uint16_t)(sign | h);
}

float bf16_to_float(uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

float fp16_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) u = sign;
        else {                                              // subnormal: renormalise
            int e = -1;
            uint32_t m = man;
            do { ++e; m <<= 1; } while (!(m & 0x400u));
            u = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3FFu) << 13);
        }
    } else if (exp == 31) u = sign | 0x7F800000u | (man << 13);
    else u = sign | ((exp + 127 - 15) << 23) | (man << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

namespace {

// U = G g G^T for F(2x2,3x3); g is one 3x3 filter (row-major), out is 4x4 (row-major, position p = 4*xi + nu)
void wino_filter_transform(const double g[9], double out[16])
{
    static const double G[4][3] = { { 1, 0, 0 }, { 0.5, 0.5, 0.5 }, { 0.5, -0.5, 0.5 }, { 0, 0, 1 } };
    double t[4][3];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[i * 4 + j] = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];
}

// pack one conv3x3 (PyTorch [Cout][Cin][3][3], per-channel scale) into the Winograd layout [Cin/8][16][CoutPad][8]
void pack_wino(const float *w, const double *scale, int cin, int cout, float *dst, size_t cpad)
{
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            double g[9], u[16];
            for (int t = 0; t < 9; ++t) g[t] = (double)w[((size_t)co * cin + ci) * 9 + t] * (scale ? scale[co] : 1.0);
            wino_filter_transform(g, u);
            for (int p = 0; p < 16; ++p)
                dst[(((size_t)(ci / WINO_KC) * 16 + p) * cpad + co) * WINO_KC + ci % WINO_KC] = (float)u[p];
        }
}

// U = G g G^T for F(4x4,3x3) (6x6, position p = 6*xi + nu), packed for conv3x3_wino4_f32 as [Cin/16][36][CoutPad][16]
void pack_wino4(const float *w, const double *scale, int cin, int cout, float *dst, size_t cpad)
{
    static const double G[6][3] = { { 1.0 / 4, 0, 0 },          { -1.0 / 6, -1.0 / 6, -1.0 / 6 }, { -1.0 / 6, 1.0 / 6, -1.0 / 6 },
                                    { 1.0 / 24, 1.0 / 12, 1.0 / 6 }, { 1.0 / 24, -1.0 / 12, 1.0 / 6 }, { 0, 0, 1 } };
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            double g[9], t[6][3];
            for (int k = 0; k < 9; ++k) g[k] = (double)w[((size_t)co * cin + ci) * 9 + k] * (scale ? scale[co] : 1.0);
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j)
                    dst[(((size_t)(ci / WINO4_KC) * 36 + i * 6 + j) * cpad + co) * WINO4_KC + ci % WINO4_KC] =
                        (float)(t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2]);
        }
}

// convT [Cin][Cout][2][2] packed per tap for convT2x2_taps_f32: [ceil(Cin/32)*4][4 taps][cpad][8], zeros elsewhere
size_t convT_taps_floats(int cin, int cout) { return (size_t)((cin + 31) / 32) * 4 * 4 * convT_taps_cpad(cout) * 8; }
void pack_convT_taps(const float *w, int cin, int cout, float *dst)
{
    const size_t cpad = (size_t)convT_taps_cpad(cout);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int tap = 0; tap < 4; ++tap)
                dst[(((size_t)(ci / 8) * 4 + tap) * cpad + co) * 8 + ci % 8] = w[((size_t)ci * cout + co) * 4 + tap];
}

// same U, packed for conv3x3_wino16_f32: [Cin/8][8 position pairs][CoutPad][16], element 4*(k/2) + 2*(pos&1) + (k&1)
void pack_wino16(const float *w, const double *scale, int cin, int cout, float *dst, size_t cpad)
{
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            double g[9], u[16];
            for (int t = 0; t < 9; ++t) g[t] = (double)w[((size_t)co * cin + ci) * 9 + t] * (scale ? scale[co] : 1.0);
            wino_filter_transform(g, u);
            const int k = ci % WINO_KC;
            for (int p = 0; p < 16; ++p)
                dst[(((size_t)(ci / WINO_KC) * 8 + p / 2) * cpad + co) * 16 + (k >> 1) * 4 + (p & 1) * 2 + (k & 1)] = (float)u[p];
        }
}

typedef uint16_t (*lp_cvt_fn)(float);

// conv3x3 (PyTorch [Cout][Cin][3][3], per-channel scale) -> 16-bit [Cin/32][9][CoutPad][32]; dst counts uint16 elements
void pack_conv_bf16(const float *w, const double *scale, int cin, int cout, uint16_t *dst, size_t cpad, lp_cvt_fn cvt)
{
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t)
                dst[(((size_t)(ci / KC_BF16) * 9 + t) * cpad + co) * KC_BF16 + ci % KC_BF16] =
                    cvt((float)((double)w[((size_t)co * cin + ci) * 9 + t] * (scale ? scale[co] : 1.0)));
}

// conv3x3 (PyTorch [Cout][Cin][3][3], per-channel scale) -> MFMA layout [Cin/16][9][CoutPad][16]
void pack_conv_mfma(const float *w, const double *scale, int cin, int cout, float *dst, size_t cpad)
{
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t)
                dst[(((size_t)(ci / KC) * 9 + t) * cpad + co) * KC + ci % KC] = (float)((double)w[((size_t)co * cin + ci) * 9 + t] * (scale ? scale[co] : 1.0));
}

// convT (PyTorch [Cin][Cout][2][2]) -> MFMA layout [Cin/16][1][NPad][16] with n = k * Cout + co
void pack_convT_mfma(const float *w, int cin, int cout, float *dst, size_t npad)
{
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int k = 0; k < 4; ++k)
                dst[((size_t)(ci / KC) * npad + (size_t)k * cout + co) * KC + ci % KC] = w[((size_t)ci * cout + co) * 4 + k];
}

// convT (PyTorch [Cin][Cout][2][2]) -> bf16 [Cin/32][1][NPad][32] with n = k * Cout + co
void pack_convT_bf16(const float *w, int cin, int cout, uint16_t *dst, size_t npad, lp_cvt_fn cvt)
{
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int k = 0; k < 4; ++k)
                dst[((size_t)(ci / KC_BF16) * npad + (size_t)k * cout + co) * KC_BF16 + ci % KC_BF16] =
                    cvt(w[((size_t)ci * cout + co) * 4 + k]);
}

// FIRST layer layout: [tap][ci][co], BN scale folded
void pack_first(const float *w, const double *scale, int cin, int cout, float *dst)
{
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t)
                dst[((size_t)t * cin + ci) * cout + co] = (float)((double)w[((size_t)co * cin + ci) * 9 + t] * (scale ? scale[co] : 1.0));
}

}  // namespace

void first_layer_lut(float lut[256])
{
    for (int i = 0; i < 256; ++i) lut[i] = static_cast<float>(i) / 255.0f;   // src/process.cpp:38, true division
}

size_t packed_npad(Pack p, int cout)
{
    if (p == Pack::TAPS) return (size_t)convT_taps_cpad(cout);
    const bool T = p == Pack::MFMA_T || p == Pack::LP_T;
    return round_up(T ? (size_t)4 * cout : (size_t)cout, NPAD);
}

size_t packed_floats(Pack p, int cin, int cout)
{
    const size_t npad = packed_npad(p, cout);
    auto chunks = [&](int kc) { return (size_t)((cin + kc - 1) / kc); };
    switch (p) {
    case Pack::FIRST: return (size_t)9 * cin * cout;
    case Pack::MFMA: return chunks(KC) * 9 * npad * KC;
    case Pack::MFMA_T: return chunks(KC) * npad * KC;
    case Pack::TAPS: return convT_taps_floats(cin, cout);
    case Pack::WINO:
    case Pack::WINO16: return chunks(WINO_KC) * 16 * npad * WINO_KC;
    case Pack::WINO4: return chunks(WINO4_KC) * 36 * npad * WINO4_KC;
    case Pack::LP: return (chunks(KC_BF16) * 9 * npad * KC_BF16 + 1) / 2;       // 16-bit elements, counted in floats
    case Pack::LP_T: return (chunks(KC_BF16) * npad * KC_BF16 + 1) / 2;
    default: break;                                   // NONE, UP: no weights
    }
    return 0;
}

void pack_weights(Pack p, bool fp16, const float *w, const double *scale, int cin, int cout, float *dst)
{
    const size_t npad = packed_npad(p, cout);
    const lp_cvt_fn cvt = fp16 ? fp16_bits : bf16_bits;
    switch (p) {
    case Pack::FIRST: pack_first(w, scale, cin, cout, dst); break;
    case Pack::MFMA: pack_conv_mfma(w, scale, cin, cout, dst, npad); break;
    case Pack::MFMA_T: pack_convT_mfma(w, cin, cout, dst, npad); break;
    case Pack::TAPS: pack_convT_taps(w, cin, cout, dst); break;
    case Pack::WINO: pack_wino(w, scale, cin, cout, dst, npad); break;
    case Pack::WINO16: pack_wino16(w, scale, cin, cout, dst, npad); break;
    case Pack::WINO4: pack_wino4(w, scale, cin, cout, dst, npad); break;
    case Pack::LP: pack_conv_bf16(w, scale, cin, cout, reinterpret_cast<uint16_t *>(dst), npad, cvt); break;
    case Pack::LP_T: pack_convT_bf16(w, cin, cout, reinterpret_cast<uint16_t *>(dst), npad, cvt); break;
    default: break;                                   // NONE, UP: no weights
    }
}

// parse "MIUNETW1" (miunet/spec.py): version 1, or version 2 with its up_mode; fold BN, repack
int engine_pack_weights(const mi_unet_config &cfg, int algo, const void *blob, size_t len, HostWeights &hw)
{
    const unsigned char *p = static_cast<const unsigned char *>(blob);
    if (len < 36 || memcmp(p, "MIUNETW1", 8) != 0) return engine_fail(MI_UNET_EFILE, "weight blob: bad magic (want MIUNETW1)");
    uint32_t h[5], n;
    float eps;
    memcpy(h, p + 8, 20);
    memcpy(&eps, p + 28, 4);
    memcpy(&n, p + 32, 4);
    size_t payload_at = 36;
    hw.up_mode = UP_TRANSPOSE;
    if (h[0] == 2) {                             // version 2: u32 up_mode between the header and the payload
        uint32_t mode;
        if (len < 40) return engine_fail(MI_UNET_EFILE, "weight blob: version 2 header truncated");
        memcpy(&mode, p + 36, 4);
        if (mode != UP_TRANSPOSE && mode != UP_BILINEAR)
            return engine_fail(MI_UNET_EFILE, "weight blob: unknown up_mode " + std::to_string(mode) + " (want 0 transposed 2x2 or 1 bilinear x2)");
        hw.up_mode = (int)mode;
        payload_at = 40;
    } else if (h[0] != 1) {
        return engine_fail(MI_UNET_EFILE, "weight blob: unsupported version " + std::to_string(h[0]) + " (want 1 or 2)");
    }
    const bool bilinear = hw.up_mode == UP_BILINEAR;
    if ((int)h[1] != cfg.in_ch || (int)h[2] != cfg.base || (int)h[3] != cfg.levels || (int)h[4] != cfg.classes)
        return engine_fail(MI_UNET_EFILE, "weight blob: topology (in_ch/base/levels/classes) does not match the engine config");
    if (len < payload_at + (size_t)n * 4) return engine_fail(MI_UNET_EFILE, "weight blob: truncated payload");
    const float *cur = reinterpret_cast<const float *>(p + payload_at);
    size_t left = n;
    auto take = [&](size_t k) -> const float * {
        if (left < k) return nullptr;
        const float *r = cur;
        cur += k; left -= k;
        return r;
    };
    const int L = cfg.levels;
    int ch[8];
    for (int i = 0; i <= L; ++i) ch[i] = cfg.base << i;
    auto &out = hw.blob;
    auto alloc = [&](size_t k) { size_t o = out.size(); out.resize(o + round_up(k, 4), 0.f); return o; };

    const bool fp16 = algo == MI_UNET_CONV_FP16, lp = fp16 || algo == MI_UNET_CONV_BF16;
    bool first_done = false;
    auto add_conv = [&](int cin, int cout) -> int {
        const float *w = take((size_t)cout * cin * 9);
        const float *g = take(cout), *be = take(cout), *mu = take(cout), *va = take(cout);
        if (!w || !g || !be || !mu || !va) return engine_fail(MI_UNET_EFILE, "weight blob: payload shorter than the topology needs");
        std::vector<double> sc(cout);
        HostWeights::Off off{};
        off.shift = alloc(cout);
        for (int co = 0; co < cout; ++co) {
            sc[co] = (double)g[co] / std::sqrt((double)va[co] + (double)eps);
            out[off.shift + co] = (float)((double)be[co] - (double)mu[co] * sc[co]);
        }
        // the layout the kernels of `algo` read: first layer [tap][ci][co]; 16-bit, Winograd (U = G g G^T) or MFMA [chunk][tap][n (padded)][KC],
        // BN scale folded before any rounding
        const Pack pk = !first_done ? Pack::FIRST : lp ? Pack::LP : algo == MI_UNET_CONV_WINOGRAD16 ? Pack::WINO16
                        : algo != MI_UNET_CONV_DIRECT ? Pack::WINO : Pack::MFMA;
        first_done = true;
        off.w = alloc(packed_floats(pk, cin, cout));
        pack_weights(pk, fp16, w, sc.data(), cin, cout, &out[off.w]);
        if (pk == Pack::WINO && algo == MI_UNET_CONV_WINOGRAD && cout % 64 == 0) {   // second packing: the F(4x4,3x3) kernel takes
            off.w4 = alloc(packed_floats(Pack::WINO4, cin, cout));                    // the layer whenever its grid fills the chip
            pack_weights(Pack::WINO4, false, w, sc.data(), cin, cout, &out[off.w4]);
        }
        hw.conv.push_back(off);
        return 0;
    };
    auto add_dconv = [&](int cin, int cout, int mid) -> int {
        int rc = add_conv(cin, mid);
        return rc ? rc : add_conv(mid, cout);
    };
    int rc = add_dconv(cfg.in_ch, ch[0], ch[0]);
    for (int i = 1; i <= L && !rc; ++i) {
        const int c = (bilinear && i == L) ? ch[L - 1] : ch[i];       // the bilinear net's bottleneck keeps ch[L-1] channels
        rc = add_dconv(ch[i - 1], c, c);
    }
    for (int i = 1; i <= L && !rc && bilinear; ++i) {                  // up_i: 2 ch[lvl] -> ch[lvl] -> ch[lvl] / 2 (ch[0] last)
        const int lvl = L - i, c = ch[lvl];
        rc = add_dconv(2 * c, lvl > 0 ? c / 2 : c, c);
    }
    for (int i = 1; i <= L && !rc && !bilinear; ++i) {
        const int cin = ch[L - i + 1], cout = cin / 2;
        const float *w = take((size_t)cin * cout * 4), *b = take(cout);
        if (!w || !b) return engine_fail(MI_UNET_EFILE, "weight blob: payload shorter than the topology needs");
        HostWeights::Off off{};
        off.shift = alloc(cout);
        for (int co = 0; co < cout; ++co) out[off.shift + co] = b[co];
        const Pack pk = lp ? Pack::LP_T : Pack::MFMA_T;
        off.w = alloc(packed_floats(pk, cin, cout));
        pack_weights(pk, fp16, w, nullptr, cin, cout, &out[off.w]);
        if (!lp && cout % 64 == 0) {   // second packing: the per-tap GEMM kernel (convt_taps.hip)
            off.w4 = alloc(packed_floats(Pack::TAPS, cin, cout));
            pack_weights(Pack::TAPS, false, w, nullptr, cin, cout, &out[off.w4]);
        }
        hw.convT.push_back(off);
        rc = add_dconv(cin, cout, cout);
    }
    if (rc) return rc;
    const float *ow = take((size_t)cfg.classes * ch[0]), *ob = take(cfg.classes);
    if (!ow || !ob || left != 0) return engine_fail(MI_UNET_EFILE, "weight blob: payload length does not match the topology");
    hw.head.w = alloc((size_t)cfg.classes * ch[0]);
    memcpy(&out[hw.head.w], ow, sizeof(float) * cfg.classes * ch[0]);
    hw.head.shift = alloc(cfg.classes);
    memcpy(&out[hw.head.shift], ob, sizeof(float) * cfg.classes);
    return 0;
}

}  // namespace miunet
