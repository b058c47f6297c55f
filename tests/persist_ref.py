"""The tile walk of the persistent kernels as a plain model, each kernel's tile geometry, and the case tables of
tests/test_gpu_persistent_walk.py (checked on the CPU by tests/test_persist_cpu.py).

Six kernels launch grid = min(nwg, cus) workgroups and walk nwg logical tiles with one partition (conv_wino4.hip PERSIST, conv_lpr.hip,
conv_lprk.hip, convt_lpr.hip in C++; csrc/asm/wino4_asm_lib.py restates it in scalar assembly for conv3x3_wino4a / conv3x3_wino4b):

  XCD x = bid & 7 owns the logical tiles [x q + min(x, r), ... + q + (x < r)), q = nwg >> 3, r = nwg & 7;
  the workgroup in slot bid >> 3 takes every slots-th tile of that range, slots = (grid >> 3) + (x < (grid & 7)).

The F(4x4,3x3) kernels number their tiles channel group first: tile t works on channel group t // m_tiles, m_tiles = the pixel blocks
of the whole batch.  A workgroup whose consecutive tiles lie in different groups changes its weights (U), bias and output base mid-walk.

Nothing here imports the library: these are statements about the inputs of the GPU tests, not about the kernels."""
from collections import namedtuple

CAPS = (8, 9, 12, 16, 23)            # the MIUNET_CUS values of the capped sweep
DEEPEST_RING = 4                     # patch / tile ring depths: conv_lpr 2-4, conv_lprk and convt_lpr 3


def clamp_cus(device_cus, env_text=None):
    """Routing::cus (csrc/routing.cpp persistent_cus): the device's count floored at 8, MIUNET_CUS clamped to [8, that]"""
    cus = max(8, device_cus)
    if not env_text:
        return cus
    try:
        n = int(env_text)
    except ValueError:
        n = 0
    return min(max(n, 8), cus)


def walk(nwg, cus):
    """{bid: [logical tiles in the order the workgroup takes them]} of a launch of min(nwg, cus) workgroups"""
    grid = min(nwg, cus)
    q, r = nwg >> 3, nwg & 7
    out = {}
    for bid in range(grid):
        x, slot = bid & 7, bid >> 3
        slots = (grid >> 3) + (1 if x < (grid & 7) else 0)
        start, count = x * q + min(x, r), q + (1 if x < r else 0)
        out[bid] = [start + t for t in range(slot, count, slots)]
    return out


def _cdiv(a, b):
    return -(-a // b)


# ---- geometry: shape (B, H, W, Cin, Cout) -> (nwg, m_tiles); m_tiles is None where the tiles have no channel-group index
def _wino4a(B, H, W, Cin, Cout):
    assert H % 16 == 0 and W % 16 == 0 and Cin % 32 == 0 and Cin >= 64 and Cout % 128 == 0      # conv3x3_wino4a_shape_ok
    m = (H // 16) * (W // 16) * B
    return m * (Cout // 128), m


def _wino4b(B, H, W, Cin, Cout):
    assert H % 16 == 0 and W % 32 == 0 and Cin % 32 == 0 and Cin >= 64 and Cout % 64 == 0       # conv3x3_wino4b_shape_ok
    m = (H // 16) * (W // 32) * B
    return m * (Cout // 64), m


def _wino4_1b(B, H, W, Cin, Cout):
    assert Cout <= 64 or Cout % 128 == 64          # the shapes route_wino4 gives the one-block kernel under MIUNET_WINO4S=0
    m = _cdiv(H, 16) * _cdiv(W, 16) * B
    return m * _cdiv(Cout, 64), m


def _lpr(B, H, W, Cin, Cout):
    assert Cin in (32, 64) and Cout in (32, 64)
    rows = 16 if (Cin, Cout) == (32, 32) else 8    # launch_lpr: two row blocks for 32 -> 32 only
    return _cdiv(W, 32) * _cdiv(H, rows) * B, None


def _lprk(B, H, W, Cin, Cout):
    assert (Cin, Cout) == (128, 64)
    return _cdiv(W, 32) * _cdiv(H, 4) * B, None


def _convt(B, H, W, Cin, Cout):
    assert (Cin, Cout) in ((64, 32), (128, 64), (256, 128))
    rows = 32 * 1024 // (Cin * 2) // 32
    return _cdiv(W, 32) * _cdiv(H, rows) * B, None


GEOMETRY = {"wino4a": _wino4a, "wino4b": _wino4b, "wino4_1b": _wino4_1b, "lpr": _lpr, "lprk": _lprk, "convt": _convt}
F44 = ("wino4a", "wino4b", "wino4_1b")


def nwg_of(kernel, shape):
    return GEOMETRY[kernel](*shape)[0]


def group_of(kernel, shape, t):
    """channel group of logical tile t (0 for the kernels without one)"""
    m = GEOMETRY[kernel](*shape)[1]
    return 0 if m is None else t // m


Props = namedtuple("Props", "nwg grid per_wg crossing")      # per_wg: sorted tile counts; crossing: walks that change channel group


def props(kernel, shape, cus):
    nwg = nwg_of(kernel, shape)
    w = walk(nwg, cus)
    crossing = sum(1 for tiles in w.values() if len({group_of(kernel, shape, t) for t in tiles}) > 1)
    return Props(nwg, min(nwg, cus), sorted(len(t) for t in w.values()), crossing)


# ---- the capped sweep: kernel -> [(shape (B, H, W, Cin, Cout), MIUNET_CUS, pooled)]
# Cin is the smallest K each kernel takes (64 for the fp32 kernels, 32 for conv_lpr); ragged sizes where the kernel allows them.
CAPPED = {
    "wino4a": [
        ((1, 48, 48, 64, 256), 8, False),        # 18 tiles, 2-3 per workgroup
        ((1, 80, 48, 64, 384), 9, False),        # 45 tiles on a grid of 9: XCD 0 has two slots (3 + 3), the others 5-6 each
        ((3, 32, 48, 64, 256), 12, True),
        ((1, 80, 48, 64, 384), 16, False),
        ((3, 48, 48, 64, 256), 23, False),
        ((1, 48, 48, 64, 256), 23, False),       # 18 tiles under a cap of 23: grid = nwg, not a multiple of 8
    ],
    "wino4b": [
        ((1, 48, 96, 64, 192), 8, False),        # 27 tiles
        ((1, 80, 96, 64, 192), 9, False),        # 45
        ((1, 32, 96, 64, 192), 12, True),        # 18
        ((2, 48, 96, 64, 128), 16, False),       # 36
        ((2, 48, 96, 64, 192), 23, False),       # 54
        ((1, 32, 96, 64, 192), 23, False),
    ],
    "wino4_1b": [
        ((1, 40, 45, 64, 192), 8, False),        # 27 tiles of ragged 16 x 16 blocks
        ((1, 70, 45, 64, 192), 9, False),        # 45
        ((3, 30, 40, 64, 64), 12, True),         # 18, one channel group
        ((1, 36, 50, 64, 192), 16, False),       # 36
        ((2, 40, 45, 64, 192), 23, False),       # 54
        ((3, 30, 40, 64, 64), 23, False),
    ],
    "lpr": [
        ((2, 72, 90, 32, 32), 8, True),          # 30 tiles of 16 rows
        ((3, 40, 70, 64, 64), 9, False),         # 45 tiles of 8 rows
        ((1, 40, 90, 32, 64), 12, False),        # 15
        ((1, 72, 90, 64, 32), 16, True),         # 27
        ((2, 72, 90, 32, 32), 23, False),
        ((1, 40, 90, 32, 64), 23, True),
    ],
    "lprk": [
        ((1, 18, 90, 128, 64), 8, False),        # 15 tiles of 4 rows
        ((2, 34, 70, 128, 64), 9, False),        # 54
        ((1, 26, 100, 128, 64), 12, False),      # 28
        ((1, 40, 90, 128, 64), 16, False),       # 30
        ((3, 13, 70, 128, 64), 23, False),       # 36
        ((1, 18, 90, 128, 64), 23, False),
    ],
    "convt": [
        ((2, 20, 90, 64, 32), 8, False),         # 18 tiles of 8 rows
        ((3, 18, 90, 128, 64), 9, False),        # 45 tiles of 4 rows
        ((1, 13, 70, 256, 128), 12, False),      # 21 tiles of 2 rows
        ((3, 20, 90, 64, 32), 16, False),        # 27
        ((2, 18, 70, 128, 64), 23, False),       # 30
        ((1, 9, 70, 256, 128), 23, False),       # 15
    ],
}

# the exact-integer case of each F(4x4,3x3) kernel: a shape and cap of the sweep whose walk crosses a channel-group boundary
EXACT = {"wino4a": ((1, 48, 48, 64, 256), 8), "wino4b": ((1, 48, 96, 64, 192), 8), "wino4_1b": ((1, 40, 45, 64, 192), 8)}

# ---- the production grid: one case per kernel with cus < nwg < 2 cus and nwg & 7 != 0.  The shapes give 300 tiles, which is
# that at 256 CUs; on another device the height moves in steps of the tile (second entry) until the model meets both conditions.
PRODUCTION = {
    "wino4a": ((1, 160, 160, 64, 384), 16),
    "wino4b": ((2, 160, 160, 64, 192), 16),
    "wino4_1b": ((1, 150, 150, 32, 192), 16),
    "lpr": ((1, 160, 960, 32, 32), 16),
    "lprk": ((1, 40, 960, 128, 64), 4),
    "convt": ((1, 80, 960, 64, 32), 8),
}


def production_ok(kernel, shape, cus):
    n = nwg_of(kernel, shape)
    return cus < n < 2 * cus and (n & 7) != 0


def production_shape(kernel, cus):
    """the PRODUCTION shape, its height moved by the fewest tile rows at which production_ok holds on a device of `cus` CUs"""
    (B, H, W, Cin, Cout), step = PRODUCTION[kernel]
    for k in range(0, 4096):
        for h in ((H + k * step, H - k * step) if k else (H,)):
            if h >= step and production_ok(kernel, (B, h, W, Cin, Cout), cus):
                return (B, h, W, Cin, Cout)
    raise AssertionError(f"no {kernel} shape with cus < nwg < 2 cus and nwg & 7 != 0 at {cus} CUs")
