"""Plain-numpy reference pieces for the tests on values off the ordinary range ("Values off the ordinary range"):
rounding tables for the 16-bit stores, the exact split of each table entry into a 16-bit operand and an fp32 bias, the blast region
of one non-finite input element per route family, and a literal Winograd F(m x m, 3x3) to check those regions against.

kind: 1 = bfloat16, 2 = IEEE binary16 (the numbering of mi_unet_layer_debug's operand types)."""
import numpy as np

# ---------------------------------------------------------------------------------------------------------- rounding tables
# (fp32 bit pattern, the 16-bit pattern round-to-nearest-even gives).  Non-negative entries; signed_table() adds the negatives.
BF16_TABLE = [
    (0x3F808000, 0x3F80),      # 1 + 2^-8: a tie, the even neighbour is below
    (0x3F818000, 0x3F82),      # 1 + 3 * 2^-8: a tie, the even neighbour is above
    (0x3F807FFF, 0x3F80),      # one fp32 ulp below the first tie
    (0x3F808001, 0x3F81),      # ... and one above it
    (0x3F7FFFFF, 0x3F80),      # the carry runs through the whole mantissa into the exponent: 1.0
    (0x7F7F7FFF, 0x7F7F),      # just below the tie at the top: the largest finite bf16
    (0x7F7F8000, 0x7F80),      # that tie: the even neighbour is infinity
]
FP16_TABLE = [
    (0x3F801000, 0x3C00),      # 1 + 2^-11: a tie, down to 1.0
    (0x3F803000, 0x3C02),      # 1 + 3 * 2^-11: a tie, up
    (0x477FE000, 0x7BFF),      # 65504, the largest finite half
    (0x477FEFFF, 0x7BFF),      # 65519.996: still 65504
    (0x477FF000, 0x7C00),      # 65520: the tie whose even neighbour is infinity
    (0x387FE000, 0x0400),      # 2^-14 - 2^-25: a tie in the subnormal range, up to the smallest normal
    (0x33000000, 0x0000),      # 2^-25: the tie between 0 and the smallest subnormal
    (0x33000001, 0x0001),      # 2^-25 (1 + 2^-23): above it
    (0x33C00000, 0x0002),     # 3 * 2^-25: the tie between the subnormals 1 and 2
    (0x33800000, 0x0001),      # 2^-24: the smallest subnormal itself
]
# what the comments above say, as numbers (the CPU test holds the bit patterns against them)
FP16_TABLE_VALUES = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504.0, 65519.99609375, 65520.0, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -25,
                     2.0 ** -25 * (1 + 2.0 ** -23), 3 * 2.0 ** -25, 2.0 ** -24]


def table(kind, signed):
    """(fp32 bits uint32[n], expected 16-bit patterns uint16[n]); signed: every entry followed by its negative"""
    t = BF16_TABLE if kind == 1 else FP16_TABLE
    src = np.array([e[0] for e in t], np.uint32)
    want = np.array([e[1] for e in t], np.uint16)
    if signed:
        src = np.stack([src, src | np.uint32(0x80000000)], 1).reshape(-1)
        want = np.stack([want, want | np.uint16(0x8000)], 1).reshape(-1)
    return src, want


def f32(bits):
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def to_bits16(kind, a):
    """the 16-bit patterns of float32 values that lie on the 16-bit grid (no rounding happens here)"""
    a = np.ascontiguousarray(a, np.float32)
    if kind == 1:
        u = a.view(np.uint32)
        assert not (u & np.uint32(0xFFFF)).any(), "not a bfloat16 value"
        return (u >> np.uint32(16)).astype(np.uint16)
    h = a.astype(np.float16)
    assert np.array_equal(h.astype(np.float32).view(np.uint32), a.view(np.uint32)) or np.isnan(a).any(), "not a binary16 value"
    return h.view(np.uint16)


def from_bits16(kind, b):
    b = np.ascontiguousarray(b, np.uint16)
    if kind == 1:
        return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return b.view(np.float16).astype(np.float32)


def torch_bits(kind, src_bits):
    """the table's expectation from torch's own CPU casts"""
    import torch
    t = torch.from_numpy(f32(src_bits).copy())
    return t.to(torch.bfloat16 if kind == 1 else torch.float16).view(torch.int16).numpy().view(np.uint16)


def split(kind, src_bits):
    """t = p + b with p the 16-bit truncation (towards zero) of t: p is a 16-bit operand, b an fp32 bias, and p + b is exact in
    fp32 because b only holds the bits of t below p's last place."""
    src_bits = np.ascontiguousarray(src_bits, np.uint32)
    t = f32(src_bits)
    if kind == 1:
        p = f32(src_bits & np.uint32(0xFFFF0000))
    else:
        normal = f32(src_bits & np.uint32(0xFFFFE000))                       # 10 fraction bits kept
        q = 2.0 ** -24                                                       # below 2^-14: multiples of the subnormal step
        sub = (np.trunc(t.astype(np.float64) / q) * q).astype(np.float32)
        p = np.where(np.abs(t) >= np.float32(2.0 ** -14), normal, sub).astype(np.float32)
    b = (t.astype(np.float64) - p.astype(np.float64)).astype(np.float32)
    return p, b


# ---------------------------------------------------------------------------------------------------------- blast regions
# Which outputs may change when input pixel (y, x) of an H x W image goes non-finite: boolean [Ho][Wo] masks.

def blast_direct(H, W, y, x):
    """the direct (non-Winograd) 3x3 routes: the 3x3 footprint, which is also exactly the set of outputs that read the pixel"""
    m = np.zeros((H, W), bool)
    m[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    return m


def blast_convT(H, W, y, x):
    """transposed 2x2 stride-2 conv: the 2x2 outputs of the pixel"""
    m = np.zeros((2 * H, 2 * W), bool)
    m[2 * y:2 * y + 2, 2 * x:2 * x + 2] = True
    return m


def _blast_wino(m, H, W, y, x):
    # origin-aligned m x m output tiles; tile t reads input rows m t - 1 .. m t + m
    out = np.zeros((H, W), bool)
    ty = [t for t in range((H + m - 1) // m) if m * t - 1 <= y <= m * t + m]
    tx = [t for t in range((W + m - 1) // m) if m * t - 1 <= x <= m * t + m]
    for a in ty:
        for b in tx:
            out[m * a:m * a + m, m * b:m * b + m] = True
    return out


def blast_wino2(H, W, y, x):
    """F(2x2,3x3) routes (conv3x3_wino, _wino16): the 2x2 output tiles whose 4x4 input patch holds the pixel.  conv_wino.hip tiles
    from the image origin (a workgroup owns 16 x 8*WM output pixels from pixel (0, 0) on, 2x2 tiles inside it)."""
    return _blast_wino(2, H, W, y, x)


def blast_wino4(H, W, y, x):
    """F(4x4,3x3) routes (conv3x3_wino4, _wino4s, _wino4a, _wino4b): the 4x4 output tiles whose 6x6 patch holds the pixel.  Every one
    of these kernels cuts the image into blocks of 16 x 16 or 16 x 32 output pixels from the origin, 4x4 tiles inside a block
    (headers of conv_wino4.hip, conv_wino4s.hip, asm/gen_wino4_asm.py, asm/gen_wino4b_asm.py)."""
    return _blast_wino(4, H, W, y, x)


def pooled(mask):
    """the 2x2-pooled image of a region: the pooled pixels whose window touches it"""
    H, W = mask.shape
    return mask[:H // 2 * 2, :W // 2 * 2].reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))


# ---------------------------------------------------------------------------------------------------------- literal Winograd
_WINO = {
    2: (np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64),                                  # B^T
        np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64),                                          # G
        np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)),                                                              # A^T
    4: (np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                  [0, 4, 0, -5, 0, 1]], np.float64),
        np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                  [0, 0, 1]], np.float64),
        np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)),
}


def winograd_conv3x3(x, w, m):
    """Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A as written, in float64 with plain matrix products (so a zero coefficient times a
    non-finite value is NaN, as IEEE has it), origin-aligned m x m tiles, zero padding.  x [H][W][Cin], w [Cout][Cin][3][3]."""
    BT, G, AT = _WINO[m]
    H, W, Cin = x.shape
    Th, Tw = (H + m - 1) // m, (W + m - 1) // m
    xp = np.zeros((Th * m + 2, Tw * m + 2, Cin), np.float64)
    xp[1:H + 1, 1:W + 1] = x
    U = np.einsum("ij,ocjk,lk->ocil", G, w.astype(np.float64), G)               # [Cout][Cin][m+2][m+2]
    out = np.zeros((Th * m, Tw * m, w.shape[0]), np.float64)
    for a in range(Th):
        for b in range(Tw):
            d = xp[m * a:m * a + m + 2, m * b:m * b + m + 2]                     # [m+2][m+2][Cin]
            V = np.stack([BT @ d[:, :, c] @ BT.T for c in range(Cin)])          # [Cin][m+2][m+2]
            M = (U * V[None]).sum(axis=1)                                       # [Cout][m+2][m+2]
            out[m * a:m * a + m, m * b:m * b + m] = np.stack([AT @ M[o] @ AT.T for o in range(w.shape[0])], axis=-1)
    return out[:H, :W]
