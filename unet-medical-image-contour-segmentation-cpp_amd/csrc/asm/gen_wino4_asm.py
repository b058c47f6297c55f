#!/usr/bin/env python3
"""gen_wino4_asm.py -- emits the gfx950 assembly of the persistent two-block Winograd F(4x4,3x3) kernel (conv3x3_wino4a).

Why assembly (profiles/r04_fp32_mfma_filler_probe.txt): next to v_mfma_f32_16x16x4_f32 with one wave per SIMD,
ANY vector-ALU instruction costs 6-13 cycles of matrix-pipe time (a packed-f32 one the same as a plain one), while SALU, s_waitcnt,
s_nop and ds_read cost nothing.  hipcc's K loop of conv3x3_wino4_f32<2> carries ~190 VALU per 288 MFMAs (96 of them the transform
itself, the rest address arithmetic, parity selects and register copies) and pays ~25 k cycles per tile outside the loop.  Here:

  * the K loop holds exactly the transform's packed operations (96 / 48 per wave and chunk) in a few large groups, every address is
    a loop-invariant register plus an immediate, buffer parities are unrolled, every wait count is exact;
  * the workgroup is PERSISTENT (one per CU): the opening loads of tile T+1 (its first two raw chunks by LDS-DMA, its U ring) are
    issued inside the last two chunks of tile T, its first transform runs before the epilogue of T, so a tile costs its chunks plus
    an epilogue -- no launch, no cold loads;
  * same data layouts as csrc/conv_wino4.hip (U = [Cin/16][36][CoutPad][16], V / raw-patch LDS images of csrc/wino4_common.h), so
    the weights are shared and the hipcc kernel remains the fallback for shapes this one does not take.

Shape contract (checked by the launcher, csrc/wino4_asm.cpp): H % 16 == 0, W % 16 == 0, Cin % 32 == 0 and Cin >= 64, Cout % 128 == 0,
CoutPad == Cout, no fused head, no split-K.  Optional fused 2x2 max pooling, ReLU by a lower bound.

What the kernel shares with conv3x3_wino4b (gen_wino4b_asm.py) is in wino4_asm_lib.py; here are this kernel's register layout, its
chunk body with the transform threaded between the MFMAs, its vmcnt model, the opening of a tile's loads and the tile loop.

usage: gen_wino4_asm.py out.s [--stop N [--dump lds|vgpr|agpr]] [--stamps] [--timing-only WHAT,..] [--u-policy P] [--store-policy P]
                              [--dma-pos P0,..,P5] [--dma-pos-first P0,..,P5]
"""
import sys
from types import SimpleNamespace

from wino4_asm_lib import *          # noqa: F403  (the scalar register map, the formatters, the shared blocks)

UD = 9                       # U ring depth in positions (36 % UD == 0)
VPOS_B = 1024                # bytes per position of a V buffer (16 tiles x 64 B)
VBUF_B = 36 * VPOS_B         # 36864
RAW_ROW = 20
RAW_LOADS = 24               # wave-wide LDS-DMA loads per chunk (23 live + 1 so that every wave issues six)
RAWBUF_B = RAW_LOADS * 1024  # 24576
LDS_R0 = 2 * VBUF_B          # 73728: behind the V buffers V0 and V1, three raw-patch buffers (chunk G lives in buffer G % 3, G counted across tiles)
LDS_BYTES = LDS_R0 + 3 * RAWBUF_B   # 147456

# ---------------------------------------------------------------------------------------------------------------- registers
# SGPRs of this kernel alone (the shared map: wino4_asm_lib.py)
L_RIDX, L_M0CUR = 0, 1   # s[0:1] once the arguments are loaded: raw-buffer index of the current body's chunk (G % 3); LDS address this wave's LDS-DMA loads of the body start at
S_PROW = 100             # s[100:101] pooled rows of the epilogue

# VGPRs
AV0 = 8 * UD                 # 72
PX0 = AV0 + 8                # 80: two banks of 16
CR0 = PX0 + 32               # 112: [2 rows][6 cols][4]
E0 = CR0 + 48                # 160
TV0 = E0 + 16                # 176: 3 quads
V_VRD0, V_VRD1, V_UVOFF, V_PRD, V_VWR = 188, 189, 190, 191, 192
V_REL0 = 193                 # 6
V_VOFF0 = 199                # 6
V_PYPX0 = 205                # 6
V_OUTOFF, V_POOLOFF = 211, 212
V_BIAS0, V_BIAS1, V_CHAN4 = 213, 214, 215
V_T0 = 216                   # 216..223: eight temporaries (set-up code only)
assert V_PYPX0 + 6 <= V_OUTOFF and V_T0 + 8 <= ACCV and TV0 + 12 <= V_VRD0

K = Kernel(
    name="conv3x3_wino4a_f32",
    LDS_BYTES=LDS_BYTES, LDS_R0=LDS_R0, RAWBUF_B=RAWBUF_B, DMA_PER_WAVE=RAW_LOADS // 4,
    # slot g -> patch row g / 20 = g * 3277 >> 16, column 4 (sl % 5) + sl / 5 with sl / 5 = sl * 13 >> 6; 18 x 18 live pixels
    ROWP=RAW_ROW, ROW_MAGIC=3277, COL_SLOTS=5, COL_MAGIC=13, COL_SHIFT=6, PATCH_W=18,
    # a block of 16 x 16 pixels x 128 channels, a wave 32 of them: two channel blocks of 16, a bias register each
    TILE_W_SHIFT=4, WAVE_CH_SHIFT=5, GROUP_CH_SHIFT=7, N_BIAS=2,
    VRD1_OFF=VBUF_B, S_PROW=S_PROW,
    PX0=PX0, CR0=CR0, E0=E0, TV0=TV0, V_VRD0=V_VRD0, V_VRD1=V_VRD1, V_UVOFF=V_UVOFF, V_REL0=V_REL0, V_VOFF0=V_VOFF0, V_PYPX0=V_PYPX0,
    V_OUTOFF=V_OUTOFF, V_POOLOFF=V_POOLOFF, V_BIAS0=V_BIAS0, V_CHAN4=V_CHAN4, V_T0=V_T0)

# ------------------------------------------------------------------------------------------------------------------ options
# E.opt, parsed once in main() (stop_at, dump: wino4_asm_lib.Emitter):
DMA_POS = (0, 2, 4, 6, 8, 10)     # dma_pos: positions of a chunk body at which the six LDS-DMA loads of the raw patch are issued (tuning: --dma-pos;
                                  # same-card sweep, profiles/r04_ab_asm_dma_positions.txt: early positions 1.6 % faster than every fourth)
DMA_POS_FIRST = (22, 23, 24, 25, 26, 27)   # dma_pos_first: ... of a tile's FIRST body: late, once the chip-wide store burst of the epilogues has drained
                                  # (profiles/r04_asm_stamps.txt: LDS-DMA issued into that burst made the first body 5.8 k cycles longer)
U_POLICY = ""                # u_policy: cache-policy modifier of the U loads (tuning: --u-policy "nt" | "sc0" | "sc1" | "sc0 sc1")
ST_POLICY = "nt"             # st_policy: ... of the epilogue's output stores: non-temporal -- the next layer reads them a launch later, from HBM / the Infinity
                             # Cache either way, and keeping them out of L2 leaves it to U and the halos (same card: the 14 layers 10.08 -> 9.89 ms;
                             # sc1 / sc0 sc1: 10.02; profiles/r04_ab_store_policy.txt; tuning: --store-policy "")
# timing_only ("")           tuning builds with WRONG results: "notransform" | "nodma" | "nouload" | "novread" (comma-separated)
# stamps (False)             bring-up / tuning: s_memtime stamps at the phase boundaries of a tile, summed per wave, written to the POOL pointer


def dma_positions(opt, kind):
    return opt.dma_pos_first if kind == "first" else opt.dma_pos


V_ST = V_T0 + 2              # six per-wave phase sums (stamp builds only; v216 / v217 stay the set-up code's temporaries)
S_PREV = S_PROW + 1


def stamp(E, k):
    """tuning builds: add the cycles since the previous stamp to phase k (only at points where lgkmcnt is 0 and s3..s7 are dead)"""
    if not E.opt.stamps:
        return
    E.i(f"s_memtime {s(S_T3, 2)}")
    E.i("s_waitcnt lgkmcnt(0)")
    E.i(f"s_sub_u32 {s(S_T2)}, {s(S_T3)}, {s(S_PREV)}")
    E.i(f"v_add_u32 {v(V_ST + k)}, {s(S_T2)}, {v(V_ST + k)}")
    E.i(f"s_mov_b32 {s(S_PREV)}, {s(S_T3)}")


# -------------------------------------------------------------------------------------------------------------- transform
# The arithmetic is wino4_asm_lib.py's: role A = waves 0, 1, role B = waves 2, 3.  The pieces: L(k) patch column k into a PX bank,
# C(k) column pass, P(row) / S(row, nus) row pass.
def tr_load(E, role, k, rbuf, lq):
    rows = 4 if role == "A" else 3
    rstep = 1 if role == "A" else 2
    for i in range(rows):
        off = ((k & 3) * 5 + (k >> 2)) * 64 + i * rstep * RAW_ROW * 64      # (the buffer is in V_PRD: emit_rotate)
        E.i(f"ds_read_b128 {v(px_bank(K, k) + 4 * i, 4)}, {v(V_PRD)} offset:{off}")
        lq.issue(("L", k))


def tr_write(E, row, nu, src, wbuf, lq):
    off = nu * VPOS_B + row * 6 * VPOS_B + wbuf * VBUF_B
    E.i(f"ds_write_b128 {v(V_VWR)}, {v(src, 4)} offset:{off}")
    lq.issue(("W", row, nu))


def transform_schedule(role):
    """position -> (valu actions, lds actions after them).  Actions are tuples understood by emit_body."""
    sch = {}
    if role == "A":
        sch[1] = ([], [("L", 0), ("L", 1)])
        sch[3] = ([("waitL", 1), ("C", 0), ("C", 1)], [("L", 2), ("L", 3)])
        sch[6] = ([("waitL", 3), ("C", 2), ("C", 3)], [("L", 4), ("L", 5)])
        sch[9] = ([("waitL", 5), ("C", 4), ("C", 5)], [])
        sch[12] = ([("P", 0), ("S", 0, (0, 1, 2))], [])
        sch[14] = ([("S", 0, (3, 4, 5)), ("P", 1)], [])
        sch[16] = ([("S", 1, (0, 1, 2))], [])
        sch[18] = ([("S", 1, (3, 4, 5))], [])
    else:
        sch[1] = ([], [("L", 0), ("L", 1)])
        sch[3] = ([("waitL", 1), ("C", 0), ("C", 1)], [("L", 2), ("L", 3)])
        sch[6] = ([("waitL", 3), ("C", 2), ("C", 3)], [("L", 4), ("L", 5)])
        sch[9] = ([("waitL", 5), ("C", 4), ("C", 5)], [])
        sch[12] = ([("P", 0), ("S", 0, (0, 1, 2))], [])
        sch[14] = ([("S", 0, (3, 4, 5))], [])
    return sch


def emit_transform_alone(E, role, rbuf, wbuf):
    """the whole transform of one chunk with nothing beside it (a tile's first chunk)"""
    lq = LdsQueue()
    E.c(f"first transform, role {role}: Raw{rbuf} -> V{wbuf}")
    tr_load(E, role, 0, rbuf, lq)
    tr_load(E, role, 1, rbuf, lq)
    for k in range(6):
        waitcnt(E, lgkm=lq.wait_count(("L", k)))
        tr_col(E, role, k)
        if k + 2 < 6:
            tr_load(E, role, k + 2, rbuf, lq)
    for row in range(2 if role == "A" else 1):
        tr_prep(E, row)
        for grp in ((0, 1, 2), (3, 4, 5)):
            for n, nu in enumerate(grp):
                tr_store_calc(E, row, nu, TV0 + 4 * n)
            for n, nu in enumerate(grp):
                tr_write(E, row, nu, TV0 + 4 * n, wbuf, lq)
            E.i("s_nop 1")       # the three TV quads are rewritten by the next group: the ds_writes read them as they issue


# ------------------------------------------------------------------------------------------------------------- chunk body
def vm_wait_for_position(opt, p, kind):
    """vmcnt that guarantees the U fragments of position p: they were issued at the end of position p - UD; younger than them are
    the refills of positions p-UD+1 .. p-1 (two each) and the LDS-DMA loads issued in those positions (of this body, or of the tail
    of the body before it).  A count that is too SMALL only waits longer, so the previous body is taken as whichever kind issues
    the fewest loads there -- except that a mid body may follow a first body, whose loads come late: counted exactly for both."""
    lo, hi = p - UD + 1, p - 1                       # positions whose loads are younger (negative = previous body)
    here = sum(1 for q in dma_positions(opt, kind) if max(0, lo) <= q <= hi)
    def tail(k):
        return sum(1 for q in dma_positions(opt, k) if lo <= q - 36 <= hi)
    prevs = {"first": ("last",), "mid": ("mid", "first"), "last": ("mid",)}[kind]
    return 2 * (UD - 1) + here + min(tail(k) for k in prevs)


def emit_body(E, role, par, kind):
    """One K chunk: 288 MFMAs on V[par] and the U ring; beside them the V fragment reads, the U refills, the LDS-DMA of the raw
    patch two chunks ahead into Raw[par], and (kind != last) the transform Raw[par^1] -> V[par^1] of the next chunk."""
    assert kind in ("first", "mid", "last")
    opt = E.opt
    lq = LdsQueue()
    sch = transform_schedule(role) if (kind != "last" and "notransform" not in opt.timing_only) else {}
    vrd = V_VRD0 if par == 0 else V_VRD1
    rbuf = wbuf = par ^ 1
    E.c(f"---- chunk body: role {role}, V{par}, {kind}")
    emit_rotate(E)
    DMA_HERE = dma_positions(opt, kind)
    E.i(f"ds_read_b128 {v(AV0, 4)}, {v(vrd)} offset:0")
    lq.issue(("AV", 0))
    pending_writes = []          # (row, nu, src) ds_writes to spread over the next MFMA gaps
    for p in range(36):
        av = AV0 + 4 * (p & 1)
        slot = p % UD
        vm = None if ((kind == "first" and p < UD) or "nouload" in opt.timing_only) else vm_wait_for_position(opt, p, kind)
        waitcnt(E, vm=vm, lgkm=lq.wait_count(("AV", p)))
        valu, ldsops = sch.get(p, ([], []))
        dma_idx = [j for j, q in enumerate(DMA_HERE) if q == p] if "nodma" not in opt.timing_only else []      # (at most two per position)
        for m in range(8):
            st, blk = m >> 1, m & 1
            acc = acc_reg(p, blk)
            csrc = "0" if (kind == "first" and p != 7 and st == 0) else acc      # a tile's first MFMA of a chain starts from the literal 0
            for n, j in enumerate(dma_idx):
                if m == 1 + 2 * n:
                    E.i(f"s_add_u32 m0, {s(L_M0CUR)}, {4096 * j}")
            E.i(f"v_mfma_f32_16x16x4_f32 {acc}, {v(av + st)}, {v(U0 + 8 * slot + 4 * blk + st)}, {csrc}")
            if m == 0 and p + 1 < 36 and "novread" not in opt.timing_only:
                E.i(f"ds_read_b128 {v(AV0 + 4 * ((p + 1) & 1), 4)}, {v(vrd)} offset:{(p + 1) * VPOS_B}")
                lq.issue(("AV", p + 1))
            for n, j in enumerate(dma_idx):
                if m == 1 + 2 * n:
                    E.i(f"buffer_load_dwordx4 {v(V_VOFF0 + j)}, {s(R_IN, 4)}, {s(L_DMAOFF)} offen lds")
            if m == 3:
                for act in valu:
                    if act[0] == "waitL":
                        waitcnt(E, lgkm=lq.wait_count(("L", act[1])))
                    elif act[0] == "C":
                        tr_col(E, role, act[1])
                    elif act[0] == "P":
                        tr_prep(E, act[1])
                    elif act[0] == "S":
                        for n, nu in enumerate(act[2]):
                            tr_store_calc(E, act[1], nu, TV0 + 4 * n)
                            pending_writes.append((act[1], nu, TV0 + 4 * n))
                for act in ldsops:
                    tr_load(E, role, act[1], rbuf, lq)
            if m >= 4 and pending_writes and m - 4 < 3:
                row, nu, src = pending_writes.pop(0)
                tr_write(E, row, nu, src, wbuf, lq)
            if (m == 6 or m == 7) and "nouload" not in opt.timing_only:
                if kind == "last" and p == 36 - UD and m == 6:
                    E.i(f"s_mov_b32 {s(L_UOFF)}, {s(N_UBASE)}")        # the ring now fills with the NEXT tile's first positions
                E.i(f"buffer_load_dwordx4 {v(U0 + 8 * slot + 4 * blk, 4)}, {v(V_UVOFF)}, {s(R_U, 4)}, {s(L_UOFF)} offen" +
                    (" offset:1024" if blk else "") + (" " + opt.u_policy if opt.u_policy else ""))
        assert not pending_writes
        E.i(f"s_add_u32 {s(L_UOFF)}, {s(L_UOFF)}, {s(A_UPOS)}")
        if p == max(DMA_HERE):
            E.i(f"s_add_u32 {s(L_DMAOFF)}, {s(L_DMAOFF)}, 64")
    # No vmcnt wait here: the raw chunk these LDS-DMA loads fetch is three chunks ahead and is first read two bodies on; every U wait
    # of the NEXT body (at most 19 + a few loads may be outstanding there) already implies that they landed, and that body's closing
    # barrier publishes them to the other waves.  The last body of a tile neither transforms nor writes V: no barrier behind it.
    if kind != "last":
        waitcnt(E, lgkm=0)
        E.i("s_barrier")


def emit_rotate(E):
    """start of every chunk body: the chunk index G advances; r = G % 3 is the raw buffer this body's LDS-DMA fills (chunk G + 3),
    (r + 1) % 3 the one its transform reads (chunk G + 1) -- V_PRD follows by +1 buffer or -2 buffers, m0's base by SALU"""
    E.i(f"s_add_u32 {s(L_RIDX)}, {s(L_RIDX)}, 1")
    E.i(f"s_cmp_eq_u32 {s(L_RIDX)}, 3")
    E.i(f"s_cselect_b32 {s(L_RIDX)}, 0, {s(L_RIDX)}")
    E.i(f"s_mul_i32 {s(S_T0)}, {s(L_RIDX)}, {RAWBUF_B}")
    E.i(f"s_add_u32 {s(L_M0CUR)}, {s(L_M0BASE)}, {s(S_T0)}")
    E.i(f"s_mov_b32 {s(S_T0)}, {RAWBUF_B}")
    E.i(f"s_cmp_eq_u32 {s(L_RIDX)}, 2")                                       # then the read buffer wraps from 2 to 0
    E.i(f"s_cselect_b32 {s(S_T0)}, {-2 * RAWBUF_B & 0xffffffff}, {s(S_T0)}")
    E.i(f"v_add_u32 {v(V_PRD)}, {s(S_T0)}, {v(V_PRD)}")


# ----------------------------------------------------------------------------------------------------------------- set-up
def emit_u_ring_fill(E):
    for j in range(UD):
        for blk in range(2):
            E.i(f"buffer_load_dwordx4 {v(U0 + 8 * j + 4 * blk, 4)}, {v(V_UVOFF)}, {s(R_U, 4)}, {s(L_UOFF)} offen" + (" offset:1024" if blk else ""))
        E.i(f"s_add_u32 {s(L_UOFF)}, {s(L_UOFF)}, {s(A_UPOS)}")


def emit_transform_lane_constants(E):
    """transform-role lane constants: row0 = 1 (waves 0, 1), wave - 2 (waves 2, 3); xi_a = 1, 3, 0, 5"""
    TID, LANE, J16, KQ, TT, TQ, TMPA, TMPB = K.lane_ids()
    E.i(f"s_sub_u32 {s(S_T0)}, {s(L_WAVE)}, 2")
    E.i(f"s_cmp_lt_u32 {s(L_WAVE)}, 2")
    E.i(f"s_cselect_b32 {s(S_T0)}, 1, {s(S_T0)}")                            # row0
    E.i(f"s_mul_i32 {s(S_T0)}, {s(S_T0)}, {RAW_ROW * 64}")
    E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, {LDS_R0}")
    E.i(f"v_lshrrev_b32 {v(TMPA)}, 2, {v(TT)}")                              # ty
    E.i(f"v_and_b32 {v(TMPB)}, 3, {v(TT)}")                                  # tx
    E.i(f"v_mul_u32_u24 {v(V_PRD)}, {4 * RAW_ROW * 64}, {v(TMPA)}")
    E.i(f"v_lshl_add_u32 {v(V_PRD)}, {v(TMPB)}, 6, {v(V_PRD)}")
    E.i(f"v_lshl_add_u32 {v(V_PRD)}, {v(TQ)}, 4, {v(V_PRD)}")
    E.i(f"v_add_u32 {v(V_PRD)}, {s(S_T0)}, {v(V_PRD)}")
    E.i(f"s_cmp_eq_u32 {s(L_WAVE)}, 0")
    E.i(f"s_cselect_b32 {s(S_T0)}, 1, 3")
    E.i(f"s_cmp_eq_u32 {s(L_WAVE)}, 2")
    E.i(f"s_cselect_b32 {s(S_T0)}, 0, {s(S_T0)}")
    E.i(f"s_cmp_eq_u32 {s(L_WAVE)}, 3")
    E.i(f"s_cselect_b32 {s(S_T0)}, 5, {s(S_T0)}")                            # xi_a
    E.i(f"s_mul_i32 {s(S_T0)}, {s(S_T0)}, {6 * VPOS_B}")
    E.i(f"v_and_b32 {v(TMPA)}, 1, {v(TMPA)}")                                # ty & 1
    E.i(f"v_lshlrev_b32 {v(TMPA)}, 1, {v(TMPA)}")                            # swz(tile)
    E.i(f"v_xor_b32 {v(TMPA)}, {v(TMPA)}, {v(TQ)}")
    E.i(f"v_lshlrev_b32 {v(TMPA)}, 4, {v(TMPA)}")
    E.i(f"v_lshl_or_b32 {v(TMPA)}, {v(TT)}, 6, {v(TMPA)}")
    E.i(f"v_add_u32 {v(V_VWR)}, {s(S_T0)}, {v(TMPA)}")


# --------------------------------------------------------------------------------------------------------------- epilogue
def emit_epilogue(E, pool):
    """units = (channel block, pair of tile columns); the second channel block is 16 channels = 64 bytes on in every pixel: an
    immediate offset on its stores"""
    E.c("epilogue" + (" + pooling" if pool else ""))
    ep_out_offsets(E)
    if pool:
        ep_pool_offsets(E)
    ep_units(E, pool, lambda E, row_s, pooled: (row_s, " offset:64"))


# ----------------------------------------------------------------------------------------------------------------- kernel
def emit_kernel(E):
    emit_entry(E)
    emit_mfma_lane_constants(E)
    emit_transform_lane_constants(E)
    emit_packed_constants(E, f"s_cmp_eq_u32 {s(L_WAVE)}, 0")                 # wave 0 has rows (1,2), wave 1 rows (3,4); 2 and 3 do not use them
    E.checkpoint(1, "arguments loaded, lane constants of the two roles computed; no vector memory access so far")
    emit_dma_lane_constants(E)
    emit_output_constants(E)
    emit_tile_range(E)
    # ---- first tile: set up, open its loads
    E.checkpoint(2, "tile range of this workgroup known")
    emit_setup_tile(E)
    E.checkpoint(3, "first tile decoded, its two bias loads issued")
    E.i(f"s_mov_b32 {s(N_HAS)}, 1")
    E.i(f"s_mov_b32 {s(L_UOFF)}, {s(N_UBASE)}")
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 0")
    emit_dma_chunk(E, 0)
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 64")
    emit_dma_chunk(E, 1)
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 128")
    emit_dma_chunk(E, 2)
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 192")
    E.i(f"s_mov_b32 {s(L_RIDX)}, 2")                                         # the first body's rotation makes it 0 (chunk G = 0)
    E.checkpoint(4, "LDS-DMA of the first three raw chunks issued")
    emit_u_ring_fill(E)
    E.checkpoint(5, "U ring filled")
    E.i("s_waitcnt vmcnt(0)")
    E.i("s_barrier")
    if E.opt.stamps:
        for k in range(6):
            E.i(f"v_mov_b32 {v(V_ST + k)}, 0")
        E.i(f"s_memtime {s(S_T3, 2)}")
        E.i("s_waitcnt lgkmcnt(0)")
        E.i(f"s_mov_b32 {s(S_PREV)}, {s(S_T3)}")
    E.i(f"s_cmp_lt_u32 {s(L_WAVE)}, 2")
    E.i("s_cbranch_scc0 .Lrole_B")
    for role in ("A", "B"):
        R = role
        E.label(f".Lrole_{R}")
        emit_transform_alone(E, role, 0, 0)
        E.checkpoint(6, "first transform done")
        E.i(f"s_branch .Ljoin_{R}")
        # ================================================================================================ tile loop
        E.label(f".Ltile_{R}")
        E.checkpoint(7, "joined: bias in the accumulators, V0 complete")
        stamp(E, 5)
        emit_body(E, role, 0, "first")
        stamp(E, 0)
        E.checkpoint(8, "first chunk done")
        E.label(f".Lloop_{R}")
        E.i(f"s_cmp_eq_u32 {s(L_PAIRS)}, 1")
        E.i(f"s_cbranch_scc0 .Lnosetup_{R}")
        # ---- the final pair of middle bodies is next: from here on the LDS-DMA loads fetch the NEXT tile's first three chunks
        emit_next_tile(E, f".Lnosetup_{R}")
        E.label(f".Lnosetup_{R}")
        emit_body(E, role, 1, "mid")
        emit_body(E, role, 0, "mid")
        E.i(f"s_sub_u32 {s(L_PAIRS)}, {s(L_PAIRS)}, 1")
        E.i(f"s_cmp_lg_u32 {s(L_PAIRS)}, 0")
        E.i(f"s_cbranch_scc1 .Lloop_{R}")
        stamp(E, 1)
        emit_body(E, role, 1, "last")
        stamp(E, 2)
        E.checkpoint(9, "every chunk of the tile done; epilogue next")
        # ---- the next tile's first transform (its chunk 0 landed two bodies ago; V0 is free: the last body read V1), then the loads
        # that open the next tile come home
        E.i(f"s_cmp_eq_u32 {s(N_HAS)}, 0")
        E.i(f"s_cbranch_scc1 .Lepi_{R}")
        emit_transform_alone(E, role, 0, 0)
        E.label(f".Lepi_{R}")
        emit_loads_home(E)
        stamp(E, 3)
        E.i("s_branch .Lepilogue")                                          # one copy for both roles; it returns by wave number
        E.label(f".Lepi_done_{R}")
        stamp(E, 4)
        E.i(f"s_cmp_eq_u32 {s(N_HAS)}, 0")
        E.i("s_cbranch_scc1 .Lend_program")
        E.i(f"s_add_u32 {s(L_TT)}, {s(L_TT)}, {s(L_SLOTS)}")
        E.label(f".Ljoin_{R}")
        emit_join(E)
        E.i("s_waitcnt lgkmcnt(0)")
        E.i("s_barrier")
        E.i(f"s_branch .Ltile_{R}")
    # ---- the epilogue (shared by both roles: it only touches accumulators, lane constants of the MFMA role and scalars)
    emit_epilogue_dispatch(E, emit_epilogue)
    E.i(f"s_cmp_lt_u32 {s(L_WAVE)}, 2")
    E.i("s_cbranch_scc1 .Lepi_done_A")
    E.i("s_branch .Lepi_done_B")
    E.label(".Lend_program")
    if E.opt.stamps:
        E.i(f"s_lshl_b32 {s(S_T0)}, {s(S_WG)}, 2")
        E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, {s(L_WAVE)}")
        E.i(f"s_lshl_b32 {s(S_T0)}, {s(S_T0)}, 5")
        E.i(f"v_mov_b32 {v(V_T0)}, {s(S_T0)}")
        for k in range(6):
            E.i(f"global_store_dword {v(V_T0)}, {v(V_ST + k)}, {s(A_POOL, 2)} offset:{4 * k}")
    emit_end(E)


def main():
    argv = sys.argv
    opt = SimpleNamespace(
        stop_at=option(argv, "--stop", 0, int), dump=option(argv, "--dump", ""), stamps="--stamps" in argv,
        timing_only=option(argv, "--timing-only", ""), u_policy=option(argv, "--u-policy", U_POLICY),
        st_policy=option(argv, "--store-policy", ST_POLICY),
        dma_pos=option(argv, "--dma-pos", DMA_POS, positions), dma_pos_first=option(argv, "--dma-pos-first", DMA_POS_FIRST, positions))
    assert len(opt.dma_pos) == 6 and all(opt.dma_pos.count(q) <= 2 for q in opt.dma_pos)
    out = argv[1] if len(argv) > 1 else "wino4a_gfx950.s"
    assert 36 % UD == 0
    E = Emitter(K, opt)
    emit_kernel(E)
    print(E.write(out, 12), file=sys.stderr)


if __name__ == "__main__":
    main()
