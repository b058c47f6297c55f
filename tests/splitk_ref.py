"""An integer model of the split-K decision of the two hipcc Winograd launchers (csrc/routing.cpp: wino4_ksplit, wino_ksplit; csrc/kernels.h:
ksplit_range) and the case table of tests/test_gpu_splitk.py.

A launch whose (tile, channel) grid cannot fill the chip cuts K = Cin into ks slices; workgroup (tile, k) walks the chunks
[begin, end) of slice k and writes raw partial sums into slab k of a workspace, and wino_splitk_reduce sums the slabs.  F(4x4,3x3)
counts K in chunks of 16 channels and cuts at any chunk; F(2x2,3x3) in chunks of 8 and cuts at whole super-chunks of 4 (the raw
patch of 32 channels it stages at a time).

Nothing here imports the library: tests/test_splitk_cpu.py holds this model against the C++ functions (tests/cpu/ksplit_test.cpp) and
proves the case table from the model alone."""
from collections import namedtuple

WS_BYTES = 64 << 20                   # the engine's workspace (engine.cpp), and what the layer hook's _splitk gives at most
F4, F2 = "wino4", "wino2"
CHUNK = {F4: 16, F2: 8}               # input channels per K chunk
GRANULE = {F4: 1, F2: 4}              # chunks a slice boundary is a multiple of
MIN_CHUNKS = {F4: 8, F2: 16}          # fewer chunks: never split
PER_SLICE = {F4: 4, F2: 8}            # chunks every slice keeps at least, before rounding

# ks: the slices of the launch (1 = the full-K kernel); wanted: before the workspace and the no-empty-slice loop; fit: after the
# workspace; ranges: [(begin, end)] in chunks; lens: their lengths
Split = namedtuple("Split", "ks wanted fit ranges lens grid chunks")


def slice_range(chunks, ks, k, granule):
    """ksplit_range of kernels.h"""
    per = ((chunks + ks - 1) // ks + granule - 1) // granule * granule
    begin = k * per
    return begin, min(begin + per, chunks)


def split(fam, grid, chunks, slab_bytes, ws_bytes=WS_BYTES, aligned=True, head=False):
    """the decision for a launch of `grid` workgroups before the split, `chunks` K chunks and slabs of slab_bytes; ws_bytes None =
    no workspace.  aligned: Cout, ldo and co_off are multiples of 4; head: the fused head (F(4x4) only)."""
    g = GRANULE[fam]
    one = Split(1, 1, 1, [(0, chunks)], [chunks], grid, chunks)
    if ws_bytes is None or head or not aligned or grid > 128 or chunks < MIN_CHUNKS[fam]:
        return one
    wanted = min(256 // grid, 8, chunks // PER_SLICE[fam])
    ks = wanted
    while ks > 1 and ks * slab_bytes > ws_bytes:
        ks -= 1
    fit = ks
    while ks > 1 and slice_range(chunks, ks, ks - 1, g)[0] >= chunks:
        ks -= 1
    ranges = [slice_range(chunks, ks, k, g) for k in range(ks)]
    return Split(ks, wanted, fit, ranges, [e - b for b, e in ranges], grid, chunks)


def wino4_nb(Cout):
    """channel blocks per wave of the hipcc F(4x4) kernel route_wino4 picks for a layer with more than 64 input channels: 2 (128
    channels per workgroup) where Cout fills them, else 1"""
    return 2 if Cout >= 128 and (Cout % 128 == 0 or Cout % 128 > 64) else 1


def grid_of(fam, shape):
    B, H, W, Cin, Cout = shape
    if fam == F4:
        per_wg = 64 * wino4_nb(Cout)
        return -(-W // 16) * -(-H // 16) * B * -(-Cout // per_wg)
    rows, per_wg = (8, 128) if Cout > 64 else (16, 64)
    return -(-W // 16) * -(-H // rows) * B * -(-Cout // per_wg)


def layer(fam, shape, ws_bytes=WS_BYTES, ldo=None, co_off=0, head=False):
    """the decision for a layer [B][H][W][Cin] -> Cout stored with pixel stride ldo at channel co_off"""
    B, H, W, Cin, Cout = shape
    ldo = Cout if ldo is None else ldo
    aligned = Cout % 4 == 0 and ldo % 4 == 0 and co_off % 4 == 0
    return split(fam, grid_of(fam, shape), -(-Cin // CHUNK[fam]), B * H * W * Cout * 4, ws_bytes, aligned, head)


def hook_ws_bytes(shape, slabs=None):
    """the workspace of the layer hook: `_splitk` 8 slabs, at most WS_BYTES; `_splitk<N>` exactly N slabs"""
    B, H, W, _, Cout = shape
    slab = B * H * W * Cout * 4
    return min(8 * slab, WS_BYTES) if slabs is None else slabs * slab


# ------------------------------------------------------------------------------------------------------------ the GPU case table
# op suffix ("" = _splitk, "3" = _splitk3), (B, H, W, Cin, Cout), ks, slice lengths in chunks (None: not stated), what the row is there for
Case = namedtuple("Case", "fam slabs shape ks lens why")
CASES = [
    Case(F4, None, (1, 16, 16, 128, 128), 2, [4, 4], "smallest two-block split"),
    Case(F4, None, (1, 16, 16, 136, 128), 2, [5, 4], "last chunk half-full: the channel mask inside a slice"),
    Case(F4, None, (1, 21, 35, 208, 128), 3, [5, 5, 3], "ragged tiles, ragged last slice, odd slice lengths"),
    Case(F4, None, (3, 16, 16, 336, 128), 5, [5, 5, 5, 5, 1], "a one-chunk slice: its opening prefetch of c_begin + 1 lies past Cin"),
    Case(F4, None, (1, 16, 16, 272, 64), 4, [5, 5, 5, 2], "one-block kernel"),
    Case(F4, None, (1, 16, 16, 400, 128), 5, None, "the no-empty-slice loop shrinks 6 to 5"),
    Case(F4, None, (1, 16, 16, 512, 256), 8, [4] * 8, "two channel groups"),
    Case(F4, None, (1, 18, 18, 144, 192), 2, [5, 4], "one-block, three channel groups, 2-pixel rim"),
    Case(F4, None, (3, 22, 36, 128, 128), 2, None, "even sizes, for the _pool form"),
    Case(F4, None, (1, 16, 16, 128, 48), 2, None, "masked columns; Cout % 4 == 0"),
    Case(F4, None, (1, 4, 4, 1024, 512), 8, [8] * 8, "the bottleneck at batch 1"),
    Case(F4, 3, (3, 16, 16, 336, 128), 3, [7, 7, 7], "shrink-to-fit on the device"),
    Case(F2, None, (1, 8, 16, 128, 128), 2, [8, 8], "smallest split"),
    Case(F2, None, (1, 8, 16, 136, 128), 2, [12, 5], "ragged last slice"),
    Case(F2, None, (1, 9, 33, 200, 128), 3, [12, 12, 1], "ragged tiles, one-chunk slice"),
    Case(F2, None, (1, 16, 16, 264, 64), 3, [12, 12, 9], "the 64 x 64 configuration; the loop shrinks 4 to 3"),
    Case(F2, None, (1, 8, 16, 392, 128), 5, [12, 12, 12, 12, 1], "five slices, the last of one chunk"),
    Case(F2, None, (1, 8, 16, 512, 128), 8, None, "eight slices"),
    Case(F2, None, (3, 12, 40, 132, 64), 2, [12, 5], "Cin % 8 != 0: masked last chunk"),
    Case(F2, None, (1, 2, 2, 1024, 64), 8, [16] * 8, "the bottleneck of a 32 x 32 input"),
]
# the contract case: Cin below 8 chunks, the hook's workspace is there and the full-K route runs
NO_SPLIT = (F4, (1, 16, 16, 64, 128))
# three rows per family for the scaling laws and the special values: even slices, ragged ones, a one-chunk slice
ROWS3 = {
    F4: [(3, 22, 36, 128, 128), (1, 21, 35, 208, 128), (3, 16, 16, 336, 128)],
    F2: [(1, 8, 16, 128, 128), (3, 12, 40, 132, 64), (1, 9, 33, 200, 128)],
}

OP = {F4: "conv3x3_wino4", F2: "conv3x3_wino"}


def case_split(c):
    return layer(c.fam, c.shape, hook_ws_bytes(c.shape, c.slabs))


def case_op(c):
    """the hook's op of a case"""
    return OP[c.fam] + "_splitk" + ("" if c.slabs is None else str(c.slabs))


def case_kernel(c):
    """... and the kernel name it must report"""
    return OP[c.fam] + (f"+splitk{c.ks}" if c.ks > 1 else "")


def case_id(c):
    return case_op(c) + "-" + "x".join(map(str, c.shape))
