"""wino4_asm_lib.py -- what the generators of the persistent gfx950 Winograd F(4x4,3x3) assembly kernels share: gen_wino4_asm.py
(conv3x3_wino4a_f32) and gen_wino4b_asm.py (conv3x3_wino4b_f32) are the same program up to numbers wherever this module speaks.

  * the emitter, the register formatters, the LDS wait model, the packed-f32 helpers and the scalar arithmetic helpers;
  * the scalar register map and the argument block (one launcher and one argument block serve both kernels: csrc/wino4_asm.cpp);
  * Kernel: what tells one kernel from the other, as plain numbers -- LDS geometry, vector register bases, shifts, counts;
  * the bring-up checkpoints (--stop N, --dump lds|vgpr|agpr);
  * the arithmetic of the forward transform V = B^T d B and of the inverse transform Y = A^T M A (when it runs is each kernel's own);
  * the blocks of the kernel that do not depend on the schedule: ids and lane constants, descriptors, the XCD tile range, the decode
    of the next tile, the join, the end of the program, the kernel descriptor.

Shared code never asks which kernel it serves: a difference is a number in the Kernel, or a small callable the generator hands in.
Each generator keeps its chunk body, its transform schedule, its vmcnt model, the opening of a tile's loads and the tile loop.
"""
from dataclasses import dataclass

# ---------------------------------------------------------------------------------------------------------------- registers
# SGPRs.  s[8:39] are the argument block after two s_load_dwordx16, field by field Wino4aArgs of csrc/wino4_asm.cpp.
S_KARG = 0          # s[0:1]: the argument pointer; dead once the arguments are loaded (each kernel then has its own use for the pair)
S_WG = 2
S_T0, S_T1, S_T2, S_T3, S_T4 = 3, 4, 5, 6, 7          # temporaries
A_IN, A_U, A_BIAS, A_OUT, A_POOL = 8, 10, 12, 14, 16   # pointers (pairs)
A_H, A_W, A_PIXIN, A_NCH, A_TX, A_TY, A_MT, A_NWG = 18, 19, 20, 21, 22, 23, 24, 25
A_MAGM, A_MAGX, A_MAGY, A_UPOS, A_UBYTES, A_IMGIN = 26, 27, 28, 29, 30, 31
A_PIXOUT, A_COOFF, A_IMGOUT, A_PIXPOOL, A_IMGPOOL, A_RELU, A_GRID, A_FLAGS = 32, 33, 34, 35, 36, 37, 38, 39
R_IN, R_U, R_OUT, R_POOL = 40, 44, 48, 52             # buffer descriptors (quads)
N_OUTB, N_POOLB = 56, 58                              # next tile: base address pairs of its out / pool descriptors
N_TOUT, N_TPOOL, N_UBASE, N_HAS = 60, 61, 62, 63      # next tile: scalar byte offsets, U base, "there is a next tile"
L_TT, L_TCOUNT, L_TSTART, L_SLOTS = 64, 65, 66, 67
L_UOFF, L_DMAOFF, L_PAIRS, L_WAVE = 68, 69, 70, 71
K_4, K_M5, K_2, K_M2, K_ALPHA, K_BETA, K_MBETA, K_M4, K_8 = 72, 74, 76, 78, 80, 82, 84, 86, 88   # packed-f32 constant pairs
C_TOUT, C_TPOOL = 90, 91                              # current tile: scalar byte offsets of its outputs
L_M0BASE = 92                                         # LDS address of this wave's first raw-patch load in buffer 0
L_BY0M1, L_BX0M1, L_BASEPIX = 93, 94, 95
S_ROW = 96                                            # s[96:99] per-row scalar offsets in the epilogue; s[100:101] are each kernel's own

# VGPRs that sit at the same place in both kernels (the rest of the map is in the Kernel)
U0 = 0                       # the U ring
ACCV = 224                   # accumulators of positions 32..35 (positions 0..31 are the 256 AGPRs)


@dataclass(frozen=True)
class Kernel:
    """One kernel as the shared code sees it.  A workgroup takes 16 rows x (16 << TILE_W_SHIFT - 4) pixels x 4 waves' channels."""
    name: str
    # LDS: the raw-patch buffers start at LDS_R0, RAWBUF_B each; a wave issues DMA_PER_WAVE wave-wide LDS-DMA loads (16 slots of 64 B) per chunk
    LDS_BYTES: int
    LDS_R0: int
    RAWBUF_B: int
    DMA_PER_WAVE: int
    # slot g of a raw buffer -> patch pixel: row g / ROWP, and with sl = g % ROWP column 4 (sl % COL_SLOTS) + sl / COL_SLOTS; live while
    # g < RAW_SLOTS and the column < PATCH_W.  The divisions are multiply-shifts: g * ROW_MAGIC >> 16, sl * COL_MAGIC >> COL_SHIFT
    ROWP: int
    ROW_MAGIC: int
    COL_SLOTS: int
    COL_MAGIC: int
    COL_SHIFT: int
    PATCH_W: int
    TILE_W_SHIFT: int        # log2 of the block's width in pixels
    WAVE_CH_SHIFT: int       # log2 of the channels of a wave
    GROUP_CH_SHIFT: int      # log2 of the channels of a workgroup
    N_BIAS: int              # bias registers of a lane: one per 16 channels of its wave
    VRD1_OFF: int            # bytes from the V fragment address in V_VRD0 to the one in V_VRD1
    S_PROW: int              # s[S_PROW:S_PROW+1]: scalar offsets of the two pooled rows in the epilogue
    # VGPRs
    PX0: int                 # two banks of 16: patch columns of the transform
    CR0: int                 # [2 rows][6 cols][4]: its column pass
    E0: int                  # 16: its row pass
    TV0: int                 # 3 quads
    V_VRD0: int
    V_VRD1: int
    V_UVOFF: int
    V_REL0: int              # DMA_PER_WAVE
    V_VOFF0: int             # DMA_PER_WAVE
    V_PYPX0: int             # DMA_PER_WAVE
    V_OUTOFF: int
    V_POOLOFF: int
    V_BIAS0: int             # N_BIAS
    V_CHAN4: int
    V_T0: int                # eight temporaries (set-up code only)

    def __post_init__(self):
        assert self.ROWP == 4 * self.COL_SLOTS and self.V_T0 + 8 <= ACCV and self.EP_VXP + 8 <= self.V_VRD0, self

    RAW_SLOTS = property(lambda k: 18 * k.ROWP)  # 18 patch rows
    # epilogue temporaries (alias the transform's registers; none is live across the K loop)
    EP_M = property(lambda k: k.PX0)             # 6 pairs
    EP_S = property(lambda k: k.PX0 + 12)        # 4 pairs
    EP_Y = property(lambda k: k.PX0 + 20)        # 4 pairs
    EP_C = property(lambda k: k.PX0 + 28)        # 2 pairs (pooling carries)
    EP_T = property(lambda k: k.CR0)             # [4][6] pairs = 48
    EP_VX = property(lambda k: k.E0)             # 16 per-x voffsets
    EP_VXP = property(lambda k: k.TV0)           # 8 per-x pooled voffsets

    def lane_ids(self):
        """TID, LANE, J16, KQ, TT, TQ of emit_entry and two scratch registers: V_T0 .. V_T0 + 7"""
        return tuple(self.V_T0 + i for i in range(8))


def v(n, cnt=1):
    return f"v{n}" if cnt == 1 else f"v[{n}:{n + cnt - 1}]"


def a(n, cnt=1):
    return f"a{n}" if cnt == 1 else f"a[{n}:{n + cnt - 1}]"


def s(n, cnt=1):
    return f"s{n}" if cnt == 1 else f"s[{n}:{n + cnt - 1}]"


def option(argv, flag, default, parse=str):
    """the value behind `flag` on the command line"""
    return parse(argv[argv.index(flag) + 1]) if flag in argv else default


def positions(text):
    return tuple(int(x) for x in text.split(","))


class Emitter:
    """The program text so far.  k: the Kernel; opt: the command line, parsed once in main() -- every generator gives it
    stop_at  bring-up: leave the kernel at checkpoint N (0 = run everything); gen_*.py out.s --stop N
    dump     bring-up: at that checkpoint, workgroup 0 writes "lds" | "vgpr" | "agpr" to the OUTPUT buffer instead of going on
    st_policy  cache-policy modifier of the epilogue's output stores (--store-policy)"""

    def __init__(self, k, opt):
        self.k = k
        self.opt = opt
        self.lines = []
        self.stats = {}

    def checkpoint(self, n, what):
        self.c(f"checkpoint {n}: {what}")
        if self.opt.stop_at == n:
            if self.opt.dump:
                emit_dump(self, self.opt.dump)
            self.i("s_branch .Lend_program")

    def i(self, text):
        self.lines.append("\t" + text)
        op = text.split()[0]
        self.stats[op] = self.stats.get(op, 0) + 1

    def label(self, name):
        self.lines.append(name + ":")

    def c(self, text):
        self.lines.append("\t// " + text)

    def write(self, out, top):
        open(out, "w").write("\n".join(self.lines) + "\n")
        most = sorted(self.stats.items(), key=lambda kv: -kv[1])[:top]
        return f"{out}: {sum(self.stats.values())} instructions; " + ", ".join(f"{op} {n}" for op, n in most)


def emit_dump(E, what):
    """bring-up only: workgroup 0 copies its LDS image (linear), or registers ([register][thread]), into the output tensor"""
    k = E.k
    E.i(f"s_cmp_lg_u32 {s(S_WG)}, 0")
    E.i("s_cbranch_scc1 .Lend_program")
    E.i("s_waitcnt vmcnt(0) lgkmcnt(0)")
    E.i("s_barrier")
    E.i(f"s_mov_b32 {s(S_ROW)}, {s(A_OUT)}")
    E.i(f"s_and_b32 {s(S_ROW + 1)}, {s(A_OUT + 1)}, 0xffff")
    E.i(f"s_mov_b32 {s(S_ROW + 2)}, 0x7ffffff0")
    E.i(f"s_mov_b32 {s(S_ROW + 3)}, 0x00020000")
    t, o = k.V_T0, k.V_T0 + 1
    E.i(f"v_mbcnt_lo_u32_b32 {v(t)}, -1, 0")
    E.i(f"v_mbcnt_hi_u32_b32 {v(t)}, -1, {v(t)}")
    E.i(f"s_lshl_b32 {s(S_T0)}, {s(L_WAVE)}, 6")
    E.i(f"v_add_u32 {v(t)}, {s(S_T0)}, {v(t)}")                              # thread index
    if what == "lds":
        E.i(f"v_lshlrev_b32 {v(o)}, 4, {v(t)}")
        E.i(f"v_add_u32 {v(t)}, 61440, {v(o)}")
        E.i(f"v_add_u32 {v(k.V_T0 + 3)}, 122880, {v(o)}")
        for i in range(k.LDS_BYTES // 4096):
            base, off = (o, i * 4096) if i < 15 else (t, (i - 15) * 4096) if i < 30 else (k.V_T0 + 3, (i - 30) * 4096)
            E.i(f"ds_read_b128 {v(k.PX0, 4)}, {v(base)} offset:{off}")
            E.i("s_waitcnt lgkmcnt(0)")
            E.i(f"s_mov_b32 {s(S_T1)}, {i * 4096}")
            E.i(f"buffer_store_dwordx4 {v(k.PX0, 4)}, {v(o)}, {s(S_ROW, 4)}, {s(S_T1)} offen")
            E.i("s_waitcnt vmcnt(0)")
    else:
        E.i(f"v_lshlrev_b32 {v(o)}, 2, {v(t)}")
        for r in range(256):
            if r in (k.V_T0, k.V_T0 + 1, k.V_T0 + 2):
                continue
            E.i(f"s_mov_b32 {s(S_T1)}, {r * 1024}")
            if what == "agpr":
                E.i(f"v_accvgpr_read_b32 {v(k.V_T0 + 2)}, {a(r)}")
                E.i("s_nop 1")
                E.i(f"buffer_store_dword {v(k.V_T0 + 2)}, {v(o)}, {s(S_ROW, 4)}, {s(S_T1)} offen")
            else:
                E.i(f"buffer_store_dword {v(r)}, {v(o)}, {s(S_ROW, 4)}, {s(S_T1)} offen")
    E.i("s_waitcnt vmcnt(0)")


def acc_reg(p, blk, r=0, cnt=4):
    """accumulator registers of position p, block blk (a channel block or a tile group: the second 4 of the position's 8):
    AGPRs for p < 32, VGPRs for the last four positions"""
    if p < 32:
        return a(8 * p + 4 * blk + r, cnt)
    return v(ACCV + 8 * (p - 32) + 4 * blk + r, cnt)


# ------------------------------------------------------------------------------------------------------------ LDS wait model
class LdsQueue:
    """LDS operations of a wave complete in order; lgkmcnt(k) = at most k outstanding.  Tracks issue order inside one body
    (every body starts after lgkmcnt(0)) and gives the exact count for "everything up to this tag has completed"."""

    def __init__(self):
        self.q = []

    def issue(self, tag):
        self.q.append(tag)

    def wait_count(self, tag):
        """count that guarantees completion of the LAST op carrying `tag`; None if nothing with that tag is outstanding"""
        idx = None
        for n, t in enumerate(self.q):
            if t == tag:
                idx = n
        if idx is None:
            return None
        k = len(self.q) - 1 - idx
        self.q = self.q[idx + 1:]
        return k


def waitcnt(E, vm=None, lgkm=None):
    parts = []
    if vm is not None:
        assert 0 <= vm <= 63, vm
        parts.append(f"vmcnt({vm})")
    if lgkm is not None:
        assert 0 <= lgkm <= 15, lgkm
        parts.append(f"lgkmcnt({lgkm})")
    if parts:
        E.i("s_waitcnt " + " ".join(parts))


# ---------------------------------------------------------------------------------------------------------- packed helpers
def pk_fma(E, dst, k_sgpr, x, y):
    """dst(quad) = K * x + y on four floats: two v_pk_fma_f32 (constant pair in SGPRs: one constant-bus read)"""
    for h in (0, 2):
        E.i(f"v_pk_fma_f32 {v(dst + h, 2)}, {s(k_sgpr, 2)}, {v(x + h, 2)}, {v(y + h, 2)}")


def pk_add(E, dst, x, y):
    for h in (0, 2):
        E.i(f"v_pk_add_f32 {v(dst + h, 2)}, {v(x + h, 2)}, {v(y + h, 2)}")


def pk_sub(E, dst, x, y):
    for h in (0, 2):
        E.i(f"v_pk_add_f32 {v(dst + h, 2)}, {v(x + h, 2)}, {v(y + h, 2)} neg_lo:[0,1] neg_hi:[0,1]")


# -------------------------------------------------------------------------------------------------------------- transform
# V = B^T d B of one 16-channel chunk, cut by rows of B^T (csrc/conv_wino4.hip):
#   role A: patch rows 1..4 -> xi rows (1,2) resp. (3,4): ta = d4 + alpha d2, tb = d3 + alpha d1, ta +- beta tb
#   role B: patch rows (0,2,4) resp. (1,3,5) -> xi 0 resp. 5: 4 d0 - 5 d1 + d2
# lane = (tile, channel quad); which rows a wave takes is in its alpha / beta and its lane constants.  The pieces: patch column k
# arrives in a PX bank (each kernel's tr_load), C(k) column pass, P(row) / S(row, nu) row pass, then each kernel's tr_write.
def px_bank(k, col):
    return k.PX0 + 16 * (col & 1)


def cr(k, row, col):
    return k.CR0 + 4 * (6 * row + col)


def tr_col(E, role, col):
    k = E.k
    d = [px_bank(k, col) + 4 * i for i in range(4)]
    if role == "A":
        ta, tb = k.TV0, k.TV0 + 4
        pk_fma(E, ta, K_ALPHA, d[1], d[3])
        pk_fma(E, tb, K_ALPHA, d[0], d[2])
        pk_fma(E, cr(k, 0, col), K_BETA, tb, ta)
        pk_fma(E, cr(k, 1, col), K_MBETA, tb, ta)
    else:
        t = k.TV0
        pk_fma(E, t, K_4, d[0], d[2])
        pk_fma(E, cr(k, 0, col), K_M5, d[1], t)


def tr_prep(E, row):
    E0 = E.k.E0
    c = [cr(E.k, row, col) for col in range(6)]
    pk_fma(E, E0, K_M4, c[2], c[4])
    pk_fma(E, E0 + 4, K_M4, c[1], c[3])
    pk_sub(E, E0 + 8, c[4], c[2])
    pk_sub(E, E0 + 12, c[3], c[1])


def tr_store_calc(E, row, nu, dst):
    E0 = E.k.E0
    c = [cr(E.k, row, col) for col in range(6)]
    if nu == 0:
        pk_fma(E, dst, K_4, c[0], c[4])
        pk_fma(E, dst, K_M5, c[2], dst)
    elif nu == 1:
        pk_add(E, dst, E0, E0 + 4)
    elif nu == 2:
        pk_sub(E, dst, E0, E0 + 4)
    elif nu == 3:
        pk_fma(E, dst, K_2, E0 + 12, E0 + 8)
    elif nu == 4:
        pk_fma(E, dst, K_M2, E0 + 12, E0 + 8)
    else:
        pk_fma(E, dst, K_4, c[1], c[5])
        pk_fma(E, dst, K_M5, c[3], dst)


# ----------------------------------------------------------------------------------------------------------------- set-up
def mul64_add(E, dst_pair, base_pair, a_s, b_s):
    """s[dst:dst+1] = s[base:base+1] + a * b (unsigned 32 x 32 -> 64)"""
    E.i(f"s_mul_i32 {s(S_T3)}, {s(a_s)}, {s(b_s)}")
    E.i(f"s_mul_hi_u32 {s(S_T4)}, {s(a_s)}, {s(b_s)}")
    E.i(f"s_add_u32 {s(dst_pair)}, {s(base_pair)}, {s(S_T3)}")
    E.i(f"s_addc_u32 {s(dst_pair + 1)}, {s(base_pair + 1)}, {s(S_T4)}")


def udiv_magic(E, q, n, magic):
    """q = n / d with magic = ceil(2^32 / d) (exact while n * d < 2^32); magic == 0 encodes d == 1"""
    E.i(f"s_mul_hi_u32 {s(q)}, {s(n)}, {s(magic)}")
    E.i(f"s_cmp_eq_u32 {s(magic)}, 0")
    E.i(f"s_cselect_b32 {s(q)}, {s(n)}, {s(q)}")


def emit_setup_tile(E):
    """Decode the logical tile index in s[S_T0] and make it the NEXT tile: LDS-DMA descriptor and per-lane offsets (what the raw
    loads use from now on), U base, output bases / offsets for its epilogue, its bias values.  Uses s3..s7, V_T0 / V_T0 + 1, vcc."""
    k = E.k
    # n_tile = L / m_tiles, m = L % m_tiles
    udiv_magic(E, S_T1, S_T0, A_MAGM)
    E.i(f"s_mul_i32 {s(S_T2)}, {s(S_T1)}, {s(A_MT)}")
    E.i(f"s_sub_u32 {s(S_T0)}, {s(S_T0)}, {s(S_T2)}")                       # m
    E.i(f"s_lshl_b32 {s(N_UBASE)}, {s(S_T1)}, {k.GROUP_CH_SHIFT + 6}")       # n_tile * the group's channels * 64 bytes
    E.i(f"s_lshl_b32 {s(N_TOUT)}, {s(S_T1)}, {k.GROUP_CH_SHIFT + 2}")        # n_tile * the group's channels * 4 bytes (outputs)
    E.i(f"s_mov_b32 {s(N_TPOOL)}, {s(N_TOUT)}")
    # bias of this channel group: issued now, consumed at the start of the tile
    E.i(f"v_add_u32 {v(k.V_T0)}, {s(N_TOUT)}, {v(k.V_CHAN4)}")
    for blk in range(k.N_BIAS):
        E.i(f"global_load_dword {v(k.V_BIAS0 + blk)}, {v(k.V_T0)}, {s(A_BIAS, 2)}" + (f" offset:{64 * blk}" if blk else ""))
    # q1 = m / tiles_x, tx = m % tiles_x; b = q1 / tiles_y, ty = q1 % tiles_y
    udiv_magic(E, S_T1, S_T0, A_MAGX)
    E.i(f"s_mul_i32 {s(S_T2)}, {s(S_T1)}, {s(A_TX)}")
    E.i(f"s_sub_u32 {s(S_T2)}, {s(S_T0)}, {s(S_T2)}")                       # tx
    udiv_magic(E, S_T4, S_T1, A_MAGY)                                          # b
    E.i(f"s_mul_i32 {s(S_T3)}, {s(S_T4)}, {s(A_TY)}")
    E.i(f"s_sub_u32 {s(S_T3)}, {s(S_T1)}, {s(S_T3)}")                       # ty
    # descriptors: in (LDS-DMA), next out, next pool -- base + b * image bytes
    E.i(f"s_mov_b32 {s(S_T0)}, {s(S_T4)}")                                   # b (mul64_add clobbers T3/T4)
    E.i(f"s_lshl_b32 {s(S_T1)}, {s(S_T3)}, 4")                               # by0
    E.i(f"s_lshl_b32 {s(S_T2)}, {s(S_T2)}, {k.TILE_W_SHIFT}")                # bx0
    mul64_add(E, R_IN, A_IN, S_T0, A_IMGIN)
    E.i(f"s_and_b32 {s(R_IN + 1)}, {s(R_IN + 1)}, 0xffff")
    mul64_add(E, N_OUTB, A_OUT, S_T0, A_IMGOUT)
    E.i(f"s_and_b32 {s(N_OUTB + 1)}, {s(N_OUTB + 1)}, 0xffff")
    mul64_add(E, N_POOLB, A_POOL, S_T0, A_IMGPOOL)
    E.i(f"s_and_b32 {s(N_POOLB + 1)}, {s(N_POOLB + 1)}, 0xffff")
    # pixel offsets
    E.i(f"s_mul_i32 {s(S_T3)}, {s(S_T1)}, {s(A_W)}")
    E.i(f"s_add_u32 {s(S_T3)}, {s(S_T3)}, {s(S_T2)}")                       # by0 * W + bx0
    E.i(f"s_mul_i32 {s(L_BASEPIX)}, {s(S_T3)}, {s(A_PIXIN)}")
    E.i(f"s_mul_i32 {s(S_T4)}, {s(S_T3)}, {s(A_PIXOUT)}")
    E.i(f"s_add_u32 {s(N_TOUT)}, {s(N_TOUT)}, {s(S_T4)}")
    E.i(f"s_lshr_b32 {s(S_T3)}, {s(S_T1)}, 1")                               # by0 / 2
    E.i(f"s_lshr_b32 {s(S_T4)}, {s(A_W)}, 1")                                # Wp
    E.i(f"s_mul_i32 {s(S_T3)}, {s(S_T3)}, {s(S_T4)}")
    E.i(f"s_lshr_b32 {s(S_T4)}, {s(S_T2)}, 1")                               # bx0 / 2
    E.i(f"s_add_u32 {s(S_T3)}, {s(S_T3)}, {s(S_T4)}")
    E.i(f"s_mul_i32 {s(S_T3)}, {s(S_T3)}, {s(A_PIXPOOL)}")
    E.i(f"s_add_u32 {s(N_TPOOL)}, {s(N_TPOOL)}, {s(S_T3)}")
    E.i(f"s_sub_u32 {s(L_BY0M1)}, {s(S_T1)}, 1")
    E.i(f"s_sub_u32 {s(L_BX0M1)}, {s(S_T2)}, 1")
    # per-lane LDS-DMA offsets: zero padding by the buffer range check (voffset 0xFFFFFFFF reads zeros)
    for j in range(k.DMA_PER_WAVE):
        E.i(f"v_and_b32 {v(k.V_T0)}, 0xffff, {v(k.V_PYPX0 + j)}")
        E.i(f"v_lshrrev_b32 {v(k.V_T0 + 1)}, 16, {v(k.V_PYPX0 + j)}")
        E.i(f"v_add_u32 {v(k.V_T0)}, {s(L_BY0M1)}, {v(k.V_T0)}")
        E.i(f"v_add_u32 {v(k.V_T0 + 1)}, {s(L_BX0M1)}, {v(k.V_T0 + 1)}")
        E.i(f"v_cmp_gt_u32 vcc, {s(A_H)}, {v(k.V_T0)}")
        E.i(f"v_cmp_gt_u32 {s(S_T3, 2)}, {s(A_W)}, {v(k.V_T0 + 1)}")
        E.i(f"s_and_b64 vcc, vcc, {s(S_T3, 2)}")
        E.i(f"v_add_u32 {v(k.V_T0)}, {s(L_BASEPIX)}, {v(k.V_REL0 + j)}")
        E.i(f"v_cndmask_b32 {v(k.V_VOFF0 + j)}, -1, {v(k.V_T0)}, vcc")


def emit_next_tile(E, skip):
    """Inside the tile loop, where the last pair of middle bodies is next: from here on the LDS-DMA loads fetch the NEXT tile's first
    raw chunks.  Decodes that tile if this workgroup has one (N_HAS), else branches to `skip`."""
    E.i(f"s_add_u32 {s(S_T0)}, {s(L_TT)}, {s(L_SLOTS)}")
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 0")
    E.i(f"s_mov_b32 {s(N_HAS)}, 0")
    E.i(f"s_cmp_lt_u32 {s(S_T0)}, {s(L_TCOUNT)}")
    E.i(f"s_cbranch_scc0 {skip}")
    E.i(f"s_mov_b32 {s(N_HAS)}, 1")
    E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, {s(L_TSTART)}")
    emit_setup_tile(E)


def emit_dma_chunk(E, buf):
    """this wave's LDS-DMA loads of one raw chunk (the one L_DMAOFF points at) into raw buffer `buf`"""
    for j in range(E.k.DMA_PER_WAVE):
        E.i(f"s_add_u32 m0, {s(L_M0BASE)}, {buf * E.k.RAWBUF_B + 4096 * j}")
        E.i("s_nop 0")
        E.i(f"buffer_load_dwordx4 {v(E.k.V_VOFF0 + j)}, {s(R_IN, 4)}, {s(L_DMAOFF)} offen lds")


# --------------------------------------------------------------------------------------------------------------- epilogue
# Y = A^T M A in-lane (lane = channel, accumulator register r = tile column, kq = tile row), ReLU by a lower bound, 4x4 stores per
# tile (+ the 2x2 pooled maxima).  Unit = (block, pair of tile columns): packed arithmetic on the register pair.  A generator's
# emit_epilogue(E, pool) is ep_out_offsets, ep_pool_offsets if it pools, whatever its second block needs, then ep_units.
def ep_out_offsets(E):
    """per-x voffsets (x = pixel column 0..15 of the block) and per-row scalar offsets"""
    k = E.k
    E.i(f"v_mov_b32 {v(k.EP_VX)}, {v(k.V_OUTOFF)}")
    for x in range(1, 16):
        E.i(f"v_add_u32 {v(k.EP_VX + x)}, {s(A_PIXOUT)}, {v(k.EP_VX + x - 1)}")
    E.i(f"s_mul_i32 {s(S_T0)}, {s(A_W)}, {s(A_PIXOUT)}")                     # bytes per image row
    E.i(f"s_mov_b32 {s(S_ROW)}, {s(C_TOUT)}")
    for i in range(1, 4):
        E.i(f"s_add_u32 {s(S_ROW + i)}, {s(S_ROW + i - 1)}, {s(S_T0)}")


def ep_pool_offsets(E):
    k = E.k
    E.i(f"v_mov_b32 {v(k.EP_VXP)}, {v(k.V_POOLOFF)}")
    for x in range(1, 8):
        E.i(f"v_add_u32 {v(k.EP_VXP + x)}, {s(A_PIXPOOL)}, {v(k.EP_VXP + x - 1)}")
    E.i(f"s_lshr_b32 {s(S_T0)}, {s(A_W)}, 1")
    E.i(f"s_mul_i32 {s(S_T0)}, {s(S_T0)}, {s(A_PIXPOOL)}")                   # bytes per pooled row
    E.i(f"s_mov_b32 {s(k.S_PROW)}, {s(C_TPOOL)}")
    E.i(f"s_add_u32 {s(k.S_PROW + 1)}, {s(k.S_PROW)}, {s(S_T0)}")


def first_pass(E, m, dst_t, stride):
    """A^T along one axis.  m: six register pairs m0..m5; writes t0..t3 at dst_t + stride * {0,1,2,3} (pairs)"""
    s12, d12, s34, d34 = E.k.EP_S, E.k.EP_S + 2, E.k.EP_S + 4, E.k.EP_S + 6
    E.i(f"v_pk_add_f32 {v(s12, 2)}, {v(m[1], 2)}, {v(m[2], 2)}")
    E.i(f"v_pk_add_f32 {v(d12, 2)}, {v(m[1], 2)}, {v(m[2], 2)} neg_lo:[0,1] neg_hi:[0,1]")
    E.i(f"v_pk_add_f32 {v(s34, 2)}, {v(m[3], 2)}, {v(m[4], 2)}")
    E.i(f"v_pk_add_f32 {v(d34, 2)}, {v(m[3], 2)}, {v(m[4], 2)} neg_lo:[0,1] neg_hi:[0,1]")
    t = [dst_t + stride * i for i in range(4)]
    E.i(f"v_pk_add_f32 {v(t[0], 2)}, {v(m[0], 2)}, {v(s12, 2)}")
    E.i(f"v_pk_add_f32 {v(t[0], 2)}, {v(t[0], 2)}, {v(s34, 2)}")
    E.i(f"v_pk_fma_f32 {v(t[1], 2)}, {s(K_2, 2)}, {v(d34, 2)}, {v(d12, 2)}")
    E.i(f"v_pk_fma_f32 {v(t[2], 2)}, {s(K_4, 2)}, {v(s34, 2)}, {v(s12, 2)}")
    E.i(f"v_pk_fma_f32 {v(t[3], 2)}, {s(K_8, 2)}, {v(d34, 2)}, {v(d12, 2)}")
    E.i(f"v_pk_add_f32 {v(t[3], 2)}, {v(t[3], 2)}, {v(m[5], 2)}")


def ep_units(E, pool, second_block):
    """The four units.  Block 0 is stored at the row's scalar offset.  second_block(E, row_sgpr, pooled) says where block 1 goes: it
    returns the scalar offset register and the instruction modifier of that row's stores, and may emit scalar code to make them."""
    k = E.k
    EP_M, EP_T, EP_Y, EP_C = k.EP_M, k.EP_T, k.EP_Y, k.EP_C
    policy = " " + E.opt.st_policy if E.opt.st_policy else ""
    for blk in range(2):
        for h2 in range(2):
            r0 = 2 * h2
            # ---- first pass: for every nu, the six xi rows -> t[i][nu] (pairs at EP_T + 2 * (6 * i + nu))
            for nu in range(6):
                m = []
                for xi in range(6):
                    p = 6 * xi + nu
                    if p < 32:
                        dst = EP_M + 2 * xi
                        E.i(f"v_accvgpr_read_b32 {v(dst)}, {a(8 * p + 4 * blk + r0)}")
                        E.i(f"v_accvgpr_read_b32 {v(dst + 1)}, {a(8 * p + 4 * blk + r0 + 1)}")
                        m.append(dst)
                    else:
                        m.append(ACCV + 8 * (p - 32) + 4 * blk + r0)
                first_pass(E, m, EP_T + 2 * nu, 12)
            # ---- second pass per output row i
            for i in range(4):
                t = [EP_T + 2 * (6 * i + nu) for nu in range(6)]
                first_pass(E, t, EP_Y, 2)                                    # y[k] pairs at EP_Y + 2 k
                for col in range(4):
                    for rr in range(2):
                        E.i(f"v_max_f32 {v(EP_Y + 2 * col + rr)}, {s(A_RELU)}, {v(EP_Y + 2 * col + rr)}")
                row_s, mod = second_block(E, S_ROW + i, False) if blk else (S_ROW + i, "")
                for col in range(4):
                    for rr in range(2):
                        x = 4 * (r0 + rr) + col
                        E.i(f"buffer_store_dword {v(EP_Y + 2 * col + rr)}, {v(k.EP_VX + x)}, {s(R_OUT, 4)}, {s(row_s)} offen" + mod + policy)
                if pool:
                    if i % 2 == 0:
                        for rr in range(2):
                            E.i(f"v_max_f32 {v(EP_C + rr)}, {v(EP_Y + rr)}, {v(EP_Y + 2 + rr)}")
                            E.i(f"v_max_f32 {v(EP_C + 2 + rr)}, {v(EP_Y + 4 + rr)}, {v(EP_Y + 6 + rr)}")
                    else:
                        for rr in range(2):
                            E.i(f"v_max3_f32 {v(EP_C + rr)}, {v(EP_Y + rr)}, {v(EP_Y + 2 + rr)}, {v(EP_C + rr)}")
                            E.i(f"v_max3_f32 {v(EP_C + 2 + rr)}, {v(EP_Y + 4 + rr)}, {v(EP_Y + 6 + rr)}, {v(EP_C + 2 + rr)}")
                        prow = k.S_PROW + (i >> 1)
                        prow_s, mod = second_block(E, prow, True) if blk else (prow, "")
                        for rr in range(2):
                            for j in range(2):
                                xp = 2 * (r0 + rr) + j
                                E.i(f"buffer_store_dword {v(EP_C + 2 * j + rr)}, {v(k.EP_VXP + xp)}, {s(R_POOL, 4)}, {s(prow_s)} offen" + mod + policy)


def emit_epilogue_dispatch(E, emit_epilogue):
    """the epilogue with and without pooling, entered at .Lepilogue by every wave; the generator's way back follows .Lepi_return"""
    E.label(".Lepilogue")
    E.i(f"s_bitcmp1_b32 {s(A_FLAGS)}, 0")
    E.i("s_cbranch_scc0 .Lepi_nopool")
    emit_epilogue(E, True)
    E.i("s_branch .Lepi_return")
    E.label(".Lepi_nopool")
    emit_epilogue(E, False)
    E.label(".Lepi_return")


# ----------------------------------------------------------------------------------------------------------------- kernel
def emit_entry(E):
    """the kernel's entry: its arguments (requested; the caller waits), the wave number in s[L_WAVE], the lane's indices in
    Kernel.lane_ids()"""
    name = E.k.name
    TID, LANE, J16, KQ, TT, TQ, TMPA, TMPB = E.k.lane_ids()
    E.lines += [
        '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"',
        "\t.amdhsa_code_object_version 6",
        "\t.text",
        f"\t.protected\t{name}",
        f"\t.globl\t{name}",
        "\t.p2align\t8",
        f"\t.type\t{name},@function",
        f"{name}:",
    ]
    E.i(f"s_load_dwordx16 {s(8, 16)}, {s(S_KARG, 2)}, 0x0")
    E.i(f"s_load_dwordx16 {s(24, 16)}, {s(S_KARG, 2)}, 0x40")
    E.i(f"v_and_b32 {v(TID)}, 0x3ff, v0")
    E.i(f"v_lshrrev_b32 {v(TMPA)}, 6, {v(TID)}")
    # gfx940+: a VALU write of a VGPR needs one wait state before v_readfirstlane reads it (the assembler pads nothing; without it the
    # wave number was whatever the register held before -- tools/dev/asm_probes/probe_ids.s); a VALU-written SGPR needs two before
    # another VALU reads it (none does here: every such SGPR goes through SALU first)
    E.i("s_nop 1")
    E.i(f"v_readfirstlane_b32 {s(L_WAVE)}, {v(TMPA)}")
    E.i("s_nop 1")
    E.i(f"v_and_b32 {v(LANE)}, 63, {v(TID)}")
    E.i(f"v_and_b32 {v(J16)}, 15, {v(LANE)}")
    E.i(f"v_lshrrev_b32 {v(KQ)}, 4, {v(LANE)}")
    E.i(f"v_lshrrev_b32 {v(TT)}, 2, {v(LANE)}")                              # transform tile
    E.i(f"v_and_b32 {v(TQ)}, 3, {v(LANE)}")                                  # transform channel quad


def emit_mfma_lane_constants(E):
    """V fragment of tile j16, k-quad kq (V_VRD0, V_VRD1); U fragment and bias of channel (wave << WAVE_CH_SHIFT) + j16"""
    k = E.k
    TID, LANE, J16, KQ, TT, TQ, TMPA, TMPB = k.lane_ids()
    E.i(f"v_lshrrev_b32 {v(TMPA)}, 1, {v(J16)}")
    E.i(f"v_and_b32 {v(TMPA)}, 2, {v(TMPA)}")                                # swz(j16)
    E.i(f"v_xor_b32 {v(TMPA)}, {v(TMPA)}, {v(KQ)}")
    E.i(f"v_lshlrev_b32 {v(TMPA)}, 4, {v(TMPA)}")
    E.i(f"v_lshl_or_b32 {v(k.V_VRD0)}, {v(J16)}, 6, {v(TMPA)}")
    E.i(f"v_add_u32 {v(k.V_VRD1)}, {k.VRD1_OFF}, {v(k.V_VRD0)}")
    E.i(f"s_lshl_b32 {s(S_T0)}, {s(L_WAVE)}, {k.WAVE_CH_SHIFT + 6}")         # wave * its channels * 64 bytes
    E.i(f"v_lshlrev_b32 {v(TMPA)}, 4, {v(KQ)}")
    E.i(f"v_lshl_or_b32 {v(TMPA)}, {v(J16)}, 6, {v(TMPA)}")
    E.i(f"v_add_u32 {v(k.V_UVOFF)}, {s(S_T0)}, {v(TMPA)}")
    E.i(f"s_lshl_b32 {s(S_T0)}, {s(L_WAVE)}, {k.WAVE_CH_SHIFT + 2}")         # wave * its channels * 4 bytes
    E.i(f"v_lshlrev_b32 {v(TMPA)}, 2, {v(J16)}")
    E.i(f"v_add_u32 {v(k.V_CHAN4)}, {s(S_T0)}, {v(TMPA)}")


def emit_packed_constants(E, scc_rows12):
    """the constant pairs of both transforms; scc_rows12: the instruction that sets SCC in the waves whose two-row piece of the
    forward transform is xi rows (1,2) (alpha -4, beta 1) and clears it where it is rows (3,4) (alpha -1, beta 2).  Ends with the
    wait for the arguments."""
    def kpair(reg, value):
        E.i(f"s_mov_b32 {s(reg)}, {value}")
        E.i(f"s_mov_b32 {s(reg + 1)}, {value}")
    kpair(K_4, "4.0"); kpair(K_M5, "0xc0a00000"); kpair(K_2, "2.0"); kpair(K_M2, "-2.0"); kpair(K_M4, "-4.0"); kpair(K_8, "0x41000000")
    E.i(scc_rows12)
    for reg, v0_, v1_ in ((K_ALPHA, "-4.0", "-1.0"), (K_BETA, "1.0", "2.0"), (K_MBETA, "-1.0", "-2.0")):
        E.i(f"s_cselect_b32 {s(reg)}, {v0_}, {v1_}")
        E.i(f"s_mov_b32 {s(reg + 1)}, {s(reg)}")
    E.i("s_waitcnt lgkmcnt(0)")


def emit_dma_lane_constants(E):
    """LDS-DMA lane constants (need W and the pixel stride): load L = wave + 4 j, slot g = 16 L + lane / 4 -> patch pixel (py, px)"""
    k = E.k
    for g in range(64 * k.DMA_PER_WAVE):                 # the multiply-shifts below, checked on every slot there is
        assert (g * k.ROW_MAGIC) >> 16 == g // k.ROWP, g
    for sl in range(k.ROWP):
        assert (sl * k.COL_MAGIC) >> k.COL_SHIFT == sl // k.COL_SLOTS, sl
    TID, LANE, J16, KQ, TT, TQ, TMPA, TMPB = k.lane_ids()
    E.i(f"s_lshl_b32 {s(S_T0)}, {s(L_WAVE)}, 10")
    E.i(f"s_add_u32 {s(L_M0BASE)}, {s(S_T0)}, {k.LDS_R0}")
    E.i(f"s_mov_b32 {s(S_T2)}, {k.ROW_MAGIC}")
    for j in range(k.DMA_PER_WAVE):
        g, py, sl, c, px = TMPA, TMPB, k.V_PYPX0 + j, k.V_REL0 + j, k.V_VOFF0 + j      # scratch in registers that are defined below
        E.i(f"s_lshl_b32 {s(S_T0)}, {s(L_WAVE)}, 4")
        E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, {64 * j}")                     # (wave + 4 j) * 16
        E.i(f"v_add_u32 {v(g)}, {s(S_T0)}, {v(TT)}")                         # slot index
        E.i(f"v_mul_lo_u32 {v(py)}, {v(g)}, {s(S_T2)}")
        E.i(f"v_lshrrev_b32 {v(py)}, 16, {v(py)}")                           # g / ROWP
        E.i(f"v_mul_u32_u24 {v(sl)}, {k.ROWP}, {v(py)}")
        E.i(f"v_sub_u32 {v(sl)}, {v(g)}, {v(sl)}")                           # g % ROWP
        E.i(f"v_mul_u32_u24 {v(c)}, {k.COL_MAGIC}, {v(sl)}")
        E.i(f"v_lshrrev_b32 {v(c)}, {k.COL_SHIFT}, {v(c)}")                  # c = sl / COL_SLOTS
        E.i(f"v_mul_u32_u24 {v(px)}, {k.COL_SLOTS}, {v(c)}")
        E.i(f"v_sub_u32 {v(px)}, {v(sl)}, {v(px)}")                          # sl % COL_SLOTS
        E.i(f"v_lshl_add_u32 {v(px)}, {v(px)}, 2, {v(c)}")                   # pixel column 4 (sl % COL_SLOTS) + c
        # live = g < RAW_SLOTS && px < PATCH_W
        E.i(f"v_cmp_gt_u32 vcc, {k.RAW_SLOTS}, {v(g)}")
        E.i(f"v_cmp_gt_u32 {s(S_T3, 2)}, {k.PATCH_W}, {v(px)}")
        E.i(f"s_and_b64 vcc, vcc, {s(S_T3, 2)}")
        # rel = ((py - 1) * W + (px - 1)) * pixel bytes + 16 * quad
        E.i(f"v_add_u32 {v(g)}, -1, {v(py)}")
        E.i(f"v_mul_lo_u32 {v(g)}, {v(g)}, {s(A_W)}")
        E.i(f"v_add_u32 {v(g)}, {v(g)}, {v(px)}")
        E.i(f"v_add_u32 {v(g)}, -1, {v(g)}")
        E.i(f"v_mul_lo_u32 {v(g)}, {v(g)}, {s(A_PIXIN)}")
        E.i(f"v_lshl_add_u32 {v(k.V_REL0 + j)}, {v(TQ)}, 4, {v(g)}")
        # pypx = py | px << 16; dead slots get row 0x7fff (never inside an image)
        E.i(f"v_lshl_or_b32 {v(py)}, {v(px)}, 16, {v(py)}")
        E.i(f"v_mov_b32 {v(g)}, 0x7fff")
        E.i(f"v_cndmask_b32 {v(k.V_PYPX0 + j)}, {v(g)}, {v(py)}, vcc")


def emit_output_constants(E):
    """output lane constants, and the descriptors that never change"""
    k = E.k
    TID, LANE, J16, KQ, TT, TQ, TMPA, TMPB = k.lane_ids()
    E.i(f"s_lshl_b32 {s(S_T0)}, {s(A_W)}, 2")
    E.i(f"s_mul_i32 {s(S_T0)}, {s(S_T0)}, {s(A_PIXOUT)}")                    # 4 rows of pixels
    E.i(f"v_mul_lo_u32 {v(TMPA)}, {v(KQ)}, {s(S_T0)}")
    E.i(f"v_add_u32 {v(TMPA)}, {v(TMPA)}, {v(k.V_CHAN4)}")
    E.i(f"v_add_u32 {v(k.V_OUTOFF)}, {s(A_COOFF)}, {v(TMPA)}")
    E.i(f"s_mul_i32 {s(S_T0)}, {s(A_W)}, {s(A_PIXPOOL)}")                    # 2 pooled rows = W/2 * 2 pixels
    E.i(f"v_mul_lo_u32 {v(TMPA)}, {v(KQ)}, {s(S_T0)}")
    E.i(f"v_add_u32 {v(k.V_POOLOFF)}, {v(TMPA)}, {v(k.V_CHAN4)}")
    E.i(f"s_mov_b32 {s(R_U)}, {s(A_U)}")
    E.i(f"s_and_b32 {s(R_U + 1)}, {s(A_U + 1)}, 0xffff")
    E.i(f"s_mov_b32 {s(R_U + 2)}, {s(A_UBYTES)}")
    E.i(f"s_mov_b32 {s(R_U + 3)}, 0x00020000")
    E.i(f"s_mov_b32 {s(R_IN + 2)}, {s(A_IMGIN)}")
    E.i(f"s_mov_b32 {s(R_IN + 3)}, 0x00020000")
    E.i(f"s_mov_b32 {s(R_OUT + 2)}, {s(A_IMGOUT)}")
    E.i(f"s_mov_b32 {s(R_OUT + 3)}, 0x00020000")
    E.i(f"s_mov_b32 {s(R_POOL + 2)}, {s(A_IMGPOOL)}")
    E.i(f"s_mov_b32 {s(R_POOL + 3)}, 0x00020000")


def emit_tile_range(E):
    """This workgroup's share of its XCD's logical tile range (csrc/kernel_common.h: blocks b and b + 8 share an XCD; tests/persist_ref.py
    mirrors the arithmetic).  Leaves the kernel if the share is empty, else s[S_T0] = its first tile, ready for emit_setup_tile."""
    E.i(f"s_and_b32 {s(S_T0)}, {s(S_WG)}, 7")                                # xcd
    E.i(f"s_lshr_b32 {s(L_TT)}, {s(S_WG)}, 3")                               # slot
    E.i(f"s_lshr_b32 {s(L_SLOTS)}, {s(A_GRID)}, 3")
    E.i(f"s_and_b32 {s(S_T1)}, {s(A_GRID)}, 7")
    E.i(f"s_cmp_lt_u32 {s(S_T0)}, {s(S_T1)}")
    E.i(f"s_addc_u32 {s(L_SLOTS)}, {s(L_SLOTS)}, 0")                         # + (xcd < G & 7)
    E.i(f"s_lshr_b32 {s(S_T1)}, {s(A_NWG)}, 3")                              # q
    E.i(f"s_and_b32 {s(S_T2)}, {s(A_NWG)}, 7")                               # r
    E.i(f"s_min_u32 {s(S_T3)}, {s(S_T0)}, {s(S_T2)}")                        # min(xcd, r)
    E.i(f"s_mul_i32 {s(L_TSTART)}, {s(S_T0)}, {s(S_T1)}")
    E.i(f"s_add_u32 {s(L_TSTART)}, {s(L_TSTART)}, {s(S_T3)}")                # xcd * q + min(xcd, r)
    E.i(f"s_cmp_lt_u32 {s(S_T0)}, {s(S_T2)}")
    E.i(f"s_addc_u32 {s(L_TCOUNT)}, {s(S_T1)}, 0")                           # q + (xcd < r)
    E.i(f"s_cmp_ge_u32 {s(L_TT)}, {s(L_TCOUNT)}")
    E.i("s_cbranch_scc1 .Lend_program")
    E.i(f"s_add_u32 {s(S_T0)}, {s(L_TSTART)}, {s(L_TT)}")


def emit_loads_home(E):
    """after a tile's last chunk: every load that opens the next tile (its U ring, raw chunks, bias) must be home BEFORE the
    epilogue's stores join the queue; the wait states: an MFMA result needs 11 before anything but its accumulate chain touches it,
    and the epilogue reads the accumulators"""
    E.i("s_waitcnt vmcnt(0)")
    E.i("s_nop 7")
    E.i("s_nop 7")


def emit_join(E):
    """join: the next tile becomes the current one"""
    E.i(f"s_mov_b32 {s(R_OUT)}, {s(N_OUTB)}")
    E.i(f"s_mov_b32 {s(R_OUT + 1)}, {s(N_OUTB + 1)}")
    E.i(f"s_mov_b32 {s(R_POOL)}, {s(N_POOLB)}")
    E.i(f"s_mov_b32 {s(R_POOL + 1)}, {s(N_POOLB + 1)}")
    E.i(f"s_mov_b32 {s(C_TOUT)}, {s(N_TOUT)}")
    E.i(f"s_mov_b32 {s(C_TPOOL)}, {s(N_TPOOL)}")
    E.i(f"s_lshr_b32 {s(L_PAIRS)}, {s(A_NCH)}, 1")
    E.i(f"s_sub_u32 {s(L_PAIRS)}, {s(L_PAIRS)}, 1")
    # bias = the initial value of position (xi, nu) = (1, 1): A^T e1 e1^T A is the all-ones tile.  With one bias register the two
    # blocks are tile groups of the same channels
    for blk in range(2):
        for r in range(4):
            E.i(f"v_accvgpr_write_b32 {a(8 * 7 + 4 * blk + r)}, {v(E.k.V_BIAS0 + blk % E.k.N_BIAS)}")


def emit_end(E):
    """behind .Lend_program: the end of the program, its pad, the kernel descriptor and the metadata"""
    name, lds = E.k.name, E.k.LDS_BYTES
    E.i("s_waitcnt vmcnt(0) lgkmcnt(0)")
    E.i("s_endpgm")
    # the instruction prefetcher runs past s_endpgm: without this pad of s_code_end words (what hipcc emits behind every kernel) the
    # fetch can leave the code object's mapping -- a "memory access fault" that comes and goes with the allocation layout
    E.lines += ["\t.p2alignl 6, 3212836864", "\t.fill 256, 4, 3212836864"]
    E.lines += [
        "\t.section\t.rodata,\"a\",@progbits",
        "\t.p2align\t6, 0x0",
        f"\t.amdhsa_kernel {name}",
        f"\t\t.amdhsa_group_segment_fixed_size {lds}",
        "\t\t.amdhsa_private_segment_fixed_size 0",
        "\t\t.amdhsa_kernarg_size 128",
        "\t\t.amdhsa_user_sgpr_count 2",
        "\t\t.amdhsa_user_sgpr_dispatch_ptr 0",
        "\t\t.amdhsa_user_sgpr_queue_ptr 0",
        "\t\t.amdhsa_user_sgpr_kernarg_segment_ptr 1",
        "\t\t.amdhsa_user_sgpr_dispatch_id 0",
        "\t\t.amdhsa_user_sgpr_kernarg_preload_length 0",
        "\t\t.amdhsa_user_sgpr_kernarg_preload_offset 0",
        "\t\t.amdhsa_user_sgpr_private_segment_size 0",
        "\t\t.amdhsa_uses_dynamic_stack 0",
        "\t\t.amdhsa_enable_private_segment 0",
        "\t\t.amdhsa_system_sgpr_workgroup_id_x 1",
        "\t\t.amdhsa_system_sgpr_workgroup_id_y 0",
        "\t\t.amdhsa_system_sgpr_workgroup_id_z 0",
        "\t\t.amdhsa_system_sgpr_workgroup_info 0",
        "\t\t.amdhsa_system_vgpr_workitem_id 0",
        "\t\t.amdhsa_next_free_vgpr 512",
        "\t\t.amdhsa_next_free_sgpr 102",
        "\t\t.amdhsa_accum_offset 256",
        "\t\t.amdhsa_reserve_vcc 1",
        "\t\t.amdhsa_float_round_mode_32 0",
        "\t\t.amdhsa_float_round_mode_16_64 0",
        "\t\t.amdhsa_float_denorm_mode_32 3",
        "\t\t.amdhsa_float_denorm_mode_16_64 3",
        "\t\t.amdhsa_dx10_clamp 1",
        "\t\t.amdhsa_ieee_mode 1",
        "\t\t.amdhsa_fp16_overflow 0",
        "\t\t.amdhsa_tg_split 0",
        "\t\t.amdhsa_exception_fp_ieee_invalid_op 0",
        "\t\t.amdhsa_exception_fp_denorm_src 0",
        "\t\t.amdhsa_exception_fp_ieee_div_zero 0",
        "\t\t.amdhsa_exception_fp_ieee_overflow 0",
        "\t\t.amdhsa_exception_fp_ieee_underflow 0",
        "\t\t.amdhsa_exception_fp_ieee_inexact 0",
        "\t\t.amdhsa_exception_int_div_zero 0",
        "\t.end_amdhsa_kernel",
        "\t.text",
        "\t.amdgpu_metadata",
        "---",
        "amdhsa.kernels:",
        "  - .agpr_count:     256",
        "    .args:",
        "      - .offset:         0",
        "        .size:           128",
        "        .value_kind:     by_value",
        f"    .group_segment_fixed_size: {lds}",
        "    .kernarg_segment_align: 8",
        "    .kernarg_segment_size: 128",
        "    .max_flat_workgroup_size: 256",
        f"    .name:           {name}",
        "    .private_segment_fixed_size: 0",
        "    .sgpr_count:     108",
        "    .sgpr_spill_count: 0",
        f"    .symbol:         {name}.kd",
        "    .uniform_work_group_size: 1",
        "    .uses_dynamic_stack: false",
        "    .vgpr_count:     512",
        "    .vgpr_spill_count: 0",
        "    .wavefront_size: 64",
        "amdhsa.target:   amdgcn-amd-amdhsa--gfx950",
        "amdhsa.version:",
        "  - 1",
        "  - 2",
        "...",
        "",
        "\t.end_amdgpu_metadata",
    ]
