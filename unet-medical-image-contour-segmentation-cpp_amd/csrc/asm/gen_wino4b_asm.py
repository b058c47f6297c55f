#!/usr/bin/env python3
"""gen_wino4b_asm.py -- emits the gfx950 assembly of conv3x3_wino4b_f32: Winograd F(4x4,3x3) for the layers with 64 output channels
per workgroup (the fp32 plan's 512^2-resolution layers), persistent, hand-scheduled.

Why a second shape.  conv3x3_wino4a_f32 gives a wave 16 tiles x 32 channels: at Cout = 64 that is half a workgroup.
conv3x3_wino4s_f32 (hipcc) gives a wave 16 tiles x 16 channels, 144 accumulators, two workgroups per CU: twice the U and V operand
traffic per MFMA, and a prologue / epilogue per 16 tiles x 64 channels.  Here a wave owns 32 tiles x 16 channels -- the same 288
accumulators as the two-block kernel, with the two accumulator blocks being two TILE GROUPS (the left and the right 16x16 pixels of
a 16x32 block) that share every U fragment: half the U bytes per MFMA of either other kernel.

  * workgroup = 4 waves = a block of 16 x 32 output pixels (32 tiles) x 64 channels, one per CU, persistent over its XCD's blocks;
  * V = B^T d B of a 16-channel chunk for 32 tiles is 72 KB: ONE buffer, so a chunk is two phases -- transform (raw patch -> V), barrier,
    288 MFMAs per wave -- which costs nothing against threading the transform between the MFMAs: on gfx950 the fp32 MFMA never
    co-executes with VALU work (profiles/r04_fp32_mfma_filler_probe.txt), only the LDS latencies of the transform are exposed;
  * the raw patch (18 x 34 pixels x 16 channels) is double-buffered and arrives by LDS-DMA two chunks ahead, during the MFMA phase;
  * U ring, exact wait counts, tile-to-tile hand-over (next block's first two raw chunks and its U ring requested inside the last two
    chunks, every load home before the epilogue's stores), in-lane inverse transform: as in gen_wino4_asm.py, from wino4_asm_lib.py.

Shape contract (csrc/wino4_asm.cpp): H % 16 == 0, W % 32 == 0, Cin % 32 == 0 and >= 64, Cout % 64 == 0, fp32, no fused head.
usage: gen_wino4b_asm.py out.s [--stop N [--dump lds|vgpr|agpr]] [--ud N] [--store-policy P] [--dma-pos P0,..,P10]
"""
import sys
from dataclasses import dataclass
from types import SimpleNamespace

from wino4_asm_lib import *          # noqa: F403  (the scalar register map, the formatters, the shared blocks)

UD = 12                      # ud: U ring depth in positions (one 16-channel fragment = 4 registers per position; same-card A/B of 6 / 9 / 12:
                             # up4.c1 1.543 / 1.518 / 1.506 ms, profiles/r04_ab_wino4b_variants.txt; tuning: --ud)
VPOS_B = 2048                # bytes per position of V: 32 tiles x 64 B
VBUF_B = 36 * VPOS_B         # 73728
ROWP = 36                    # pixel slots per patch row (34 live): pixel x = 4 a + c sits in slot 9 c + a
RAW_LOADS = 44               # wave-wide LDS-DMA loads per chunk (41 live; eleven per wave)
DMA_PER_WAVE = 11
RAWBUF_B = RAW_LOADS * 1024  # 45056
LDS_R0 = VBUF_B
LDS_BYTES = LDS_R0 + 2 * RAWBUF_B    # 163840 = the whole LDS of a CU

# ---------------------------------------------------------------------------------------------------------------- registers
# SGPRs of this kernel alone (the shared map: wino4_asm_lib.py)
S_G1, S_PG1 = 100, 101       # byte offset of the right tile group in an output row / a pooled row
S_PROW = 0                   # s[0:1]: pooled rows (the argument pointer is dead by then)


@dataclass(frozen=True)
class Wino4b(Kernel):
    UD: int
    AV0: int                 # [2 position parities][2 groups][4]
    V_PRD: int               # V_PRD / V_VWR: raw read and V write base of the wave's two-row piece of the transform
    V_VWR: int
    V_PRD2: int              # ..2: of its one-row piece
    V_VWR2: int


def layout(ud):
    """the kernel with the vector register map for a U ring of `ud` positions (4 registers each)"""
    AV0 = 4 * ud
    PX0 = AV0 + 16
    CR0 = PX0 + 32
    E0 = CR0 + 48
    TV0 = E0 + 16
    base = TV0 + 12
    V_VRD0, V_VRD1, V_UVOFF, V_PRD, V_VWR, V_PRD2, V_VWR2 = (base + i for i in range(7))
    V_REL0 = base + 7            # 11
    V_VOFF0 = V_REL0 + 11        # 11
    V_PYPX0 = V_VOFF0 + 11       # 11
    V_OUTOFF, V_POOLOFF, V_BIAS0, V_CHAN4 = (V_PYPX0 + 11 + i for i in range(4))
    V_T0 = V_CHAN4 + 1           # eight temporaries (set-up code only)
    assert V_T0 + 8 <= ACCV, (ud, V_T0)
    return Wino4b(
        name="conv3x3_wino4b_f32",
        LDS_BYTES=LDS_BYTES, LDS_R0=LDS_R0, RAWBUF_B=RAWBUF_B, DMA_PER_WAVE=DMA_PER_WAVE,
        # slot g -> patch row g / 36 = g * 1821 >> 16 (for g < 704), column 4 (sl % 9) + sl / 9 with sl / 9 = sl * 57 >> 9; 18 x 34 live pixels
        ROWP=ROWP, ROW_MAGIC=1821, COL_SLOTS=9, COL_MAGIC=57, COL_SHIFT=9, PATCH_W=34,
        # a block of 16 x 32 pixels x 64 channels, a wave 16 of them: the two blocks of its accumulators are tile groups, one bias register
        TILE_W_SHIFT=5, WAVE_CH_SHIFT=4, GROUP_CH_SHIFT=6, N_BIAS=1,
        VRD1_OFF=32 * VPOS_B, S_PROW=S_PROW,                 # V_VRD1: positions 32..35, past the 16-bit offset of a ds_read
        PX0=PX0, CR0=CR0, E0=E0, TV0=TV0, V_VRD0=V_VRD0, V_VRD1=V_VRD1, V_UVOFF=V_UVOFF, V_REL0=V_REL0, V_VOFF0=V_VOFF0, V_PYPX0=V_PYPX0,
        V_OUTOFF=V_OUTOFF, V_POOLOFF=V_POOLOFF, V_BIAS0=V_BIAS0, V_CHAN4=V_CHAN4, V_T0=V_T0,
        UD=ud, AV0=AV0, V_PRD=V_PRD, V_VWR=V_VWR, V_PRD2=V_PRD2, V_VWR2=V_VWR2)


# -------------------------------------------------------------------------------------------------------------- transform
# One tile group at a time: the 16x16 pixels at column offset 16 g of the block; lane = (tile of the group, channel quad), the wave's
# role = rows of B^T (wino4_asm_lib.py).  A whole chunk (both groups) runs with nothing beside it, so the only scheduling is the
# software pipeline of the patch reads: column k + 2 is requested while column k is combined.
def lq_reserve(E, lq, n):
    """lgkmcnt counts at most 15 outstanding LDS operations: before n more are issued, retire the oldest ones (long done)"""
    if len(lq.q) + n > 15:
        keep = min(len(lq.q), 15 - n - 3)
        E.i(f"s_waitcnt lgkmcnt({keep})")
        lq.q = lq.q[len(lq.q) - keep:]


def tr_load(E, role, g, k, rbuf, lq):
    """patch column k of this lane's rows (g only tags the pass: the tile group's columns are part of the base register)"""
    rows = 4 if role == "A" else 3
    rstep = 1 if role == "A" else 2
    prd = E.k.V_PRD if role == "A" else E.k.V_PRD2
    lq_reserve(E, lq, rows)
    for i in range(rows):
        off = (9 * (k & 3) + (k >> 2)) * 64 + i * rstep * ROWP * 64 + rbuf * RAWBUF_B
        assert off < 65536
        E.i(f"ds_read_b128 {v(px_bank(E.k, k) + 4 * i, 4)}, {v(prd)} offset:{off}")
        lq.issue(("L", g, k))


def tr_write(E, role, g, row, nu, src, lq):
    off = nu * VPOS_B + row * 6 * VPOS_B
    assert off < 65536
    lq_reserve(E, lq, 1)
    E.i(f"ds_write_b128 {v(E.k.V_VWR if role == 'A' else E.k.V_VWR2)}, {v(src, 4)} offset:{off}")
    lq.issue(("W", g, row, nu))


def emit_transform(E, rbuf):
    """V = B^T d B of one chunk, Raw[rbuf] -> V, for both tile groups.  The work is cut into eight (tile group, rows of B^T) pieces --
    two rows (1,2) or (3,4): 96 packed operations, one row 0 or 5: 48 -- and every wave takes a two-row piece of one group and a
    one-row piece of the OTHER group: 144 packed operations each, no wave waits for a heavier one at the barrier.  Which pieces is
    in the wave's lane constants (V_PRD / V_VWR, V_PRD2 / V_VWR2, alpha / beta): one instruction stream for all four waves."""
    TV0 = E.k.TV0
    lq = LdsQueue()
    E.c(f"transform: Raw{rbuf} -> V")
    seq = [("A", 0, k) for k in range(6)] + [("B", 1, k) for k in range(6)]
    tr_load(E, seq[0][0], seq[0][1], seq[0][2], rbuf, lq)
    tr_load(E, seq[1][0], seq[1][1], seq[1][2], rbuf, lq)
    for n, (role, g, k) in enumerate(seq):
        waitcnt(E, lgkm=lq.wait_count(("L", g, k)))
        tr_col(E, role, k)
        if n + 2 < len(seq):
            tr_load(E, seq[n + 2][0], seq[n + 2][1], seq[n + 2][2], rbuf, lq)      # into the bank column k just left
        if k == 5:                                         # the pass's six columns are combined: its row pass
            for row in range(2 if role == "A" else 1):
                tr_prep(E, row)
                for grp in ((0, 1, 2), (3, 4, 5)):
                    for m, nu in enumerate(grp):
                        tr_store_calc(E, row, nu, TV0 + 4 * m)
                    for m, nu in enumerate(grp):
                        tr_write(E, role, g, row, nu, TV0 + 4 * m, lq)
                    E.i("s_nop 1")       # the three TV quads are rewritten by the next group: the ds_writes read them as they issue


# ------------------------------------------------------------------------------------------------------------- chunk body
# E.opt, parsed once in main() (stop_at, dump: wino4_asm_lib.Emitter):
ST_POLICY = ""               # st_policy: cache policy of the output stores: the default one -- "nt", which pays in gen_wino4_asm.py, costs here (same card: up4.c1
                             # 1.45 -> 1.51 ms, profiles/r04_ab_store_policy.txt); tuning: --store-policy
DMA_POS = tuple(range(1, 34, 3))          # dma_pos: one LDS-DMA load every third position of the MFMA phase (tuning: --dma-pos; same card: the first
                                          # eleven positions 1.518 ms, every second 1.504, every third 1.47, positions 12..22 1.53)


def vm_wait_for_position(E, p):
    """U fragment of position p: issued at the end of position p - UD; younger: one refill per position since, and the LDS-DMA
    loads of positions p-UD+1 .. p-1 of this body (none at the tail of the previous one)"""
    UD = E.k.UD
    dmas = sum(1 for q in E.opt.dma_pos if max(0, p - UD + 1) <= q < p)
    return (UD - 1) + dmas


def emit_body(E, par, kind):
    assert kind in ("first", "mid", "last")
    k, dma_pos = E.k, E.opt.dma_pos
    E.c(f"---- chunk body: Raw{par}, {kind}")
    # raw(c) is in LDS (requested two bodies ago: every U wait of the previous body implies it; the first tile waited for everything),
    # and every wave has finished the MFMA phase that read V: then the transform may overwrite V
    E.i("s_barrier")
    emit_transform(E, par)
    waitcnt(E, lgkm=0)
    E.i("s_barrier")
    lq = LdsQueue()
    for g in range(2):
        E.i(f"ds_read_b128 {v(k.AV0 + 4 * g, 4)}, {v(k.V_VRD0)} offset:{g * 1024}")
        lq.issue(("AV", 0, g))
    for p in range(36):
        avb = k.AV0 + 8 * (p & 1)
        slot = p % k.UD
        vm = None if (kind == "first" and p < k.UD) else vm_wait_for_position(E, p)
        waitcnt(E, vm=vm, lgkm=lq.wait_count(("AV", p, 1)))
        dma = p in dma_pos
        for m in range(8):
            st, g = m >> 1, m & 1
            acc = acc_reg(p, g)
            csrc = "0" if (kind == "first" and p != 7 and st == 0) else acc
            if dma and m == 2:
                E.i(f"s_add_u32 m0, {s(L_M0BASE)}, {par * RAWBUF_B + 4096 * dma_pos.index(p)}")
            E.i(f"v_mfma_f32_16x16x4_f32 {acc}, {v(avb + 4 * g + st)}, {v(U0 + 4 * slot + st)}, {csrc}")
            if m < 2 and p + 1 < 36:
                q = p + 1
                base, off = (k.V_VRD0, q * VPOS_B) if q < 32 else (k.V_VRD1, (q - 32) * VPOS_B)
                E.i(f"ds_read_b128 {v(k.AV0 + 8 * (q & 1) + 4 * m, 4)}, {v(base)} offset:{off + m * 1024}")
                lq.issue(("AV", q, m))
            if dma and m == 2:
                E.i(f"buffer_load_dwordx4 {v(k.V_VOFF0 + dma_pos.index(p))}, {s(R_IN, 4)}, {s(L_DMAOFF)} offen lds")
            if m == 7:
                if kind == "last" and p == 36 - k.UD:
                    E.i(f"s_mov_b32 {s(L_UOFF)}, {s(N_UBASE)}")
                E.i(f"buffer_load_dwordx4 {v(U0 + 4 * slot, 4)}, {v(k.V_UVOFF)}, {s(R_U, 4)}, {s(L_UOFF)} offen")
        E.i(f"s_add_u32 {s(L_UOFF)}, {s(L_UOFF)}, {s(A_UPOS)}")
        if p == max(dma_pos):
            E.i(f"s_add_u32 {s(L_DMAOFF)}, {s(L_DMAOFF)}, 64")


# ----------------------------------------------------------------------------------------------------------------- set-up
def emit_u_ring_fill(E):
    for j in range(E.k.UD):
        E.i(f"buffer_load_dwordx4 {v(U0 + 4 * j, 4)}, {v(E.k.V_UVOFF)}, {s(R_U, 4)}, {s(L_UOFF)} offen")
        E.i(f"s_add_u32 {s(L_UOFF)}, {s(L_UOFF)}, {s(A_UPOS)}")


def emit_transform_lane_constants(E):
    """Wave w: two-row piece (rows 1,2 for even w: alpha -4, beta 1; rows 3,4 for odd w: alpha -1, beta 2) of tile group w >> 1,
    one-row piece (row 0 for even w, row 5 for odd w) of the OTHER group.  Patch rows: two-row pieces read rows 1..4 (row0 = 1,
    step 1), row 0 reads rows 0,2,4 (row0 = 0, step 2), row 5 reads rows 1,3,5 (row0 = 1, step 2)."""
    k = E.k
    TID, LANE, J16, KQ, TT, TQ, TMPA, TMPB = k.lane_ids()
    E.i(f"v_lshrrev_b32 {v(TMPA)}, 2, {v(TT)}")                              # ty
    E.i(f"v_and_b32 {v(TMPB)}, 3, {v(TT)}")                                  # tx (inside the group)
    E.i(f"v_mul_u32_u24 {v(k.V_PRD)}, {4 * ROWP * 64}, {v(TMPA)}")
    E.i(f"v_lshl_add_u32 {v(k.V_PRD)}, {v(TMPB)}, 6, {v(k.V_PRD)}")
    E.i(f"v_lshl_add_u32 {v(k.V_PRD)}, {v(TQ)}, 4, {v(k.V_PRD)}")            # (4 ty rows, tx, quad) of the lane
    E.i(f"s_lshr_b32 {s(S_T1)}, {s(L_WAVE)}, 1")                             # g1 = w >> 1
    E.i(f"s_and_b32 {s(S_T2)}, {s(L_WAVE)}, 1")                              # odd
    E.i(f"s_lshl_b32 {s(S_T0)}, {s(S_T1)}, 8")                               # g1 * 4 slots * 64 bytes
    E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, {LDS_R0 + ROWP * 64}")            # + row 1
    E.i(f"s_xor_b32 {s(S_T3)}, {s(S_T1)}, 1")                                # g2 = 1 - g1
    E.i(f"s_lshl_b32 {s(S_T4)}, {s(S_T3)}, 8")
    E.i(f"s_mul_i32 {s(S_T3)}, {s(S_T2)}, {ROWP * 64}")                      # row0 of the one-row piece = odd
    E.i(f"s_add_u32 {s(S_T4)}, {s(S_T4)}, {s(S_T3)}")
    E.i(f"s_add_u32 {s(S_T4)}, {s(S_T4)}, {LDS_R0}")
    E.i(f"v_add_u32 {v(k.V_PRD2)}, {s(S_T4)}, {v(k.V_PRD)}")
    E.i(f"v_add_u32 {v(k.V_PRD)}, {s(S_T0)}, {v(k.V_PRD)}")
    # V write bases: position row xi_a of the piece, tile 16 g + t, quad ^ swz(t)
    E.i(f"v_and_b32 {v(TMPA)}, 1, {v(TMPA)}")
    E.i(f"v_lshlrev_b32 {v(TMPA)}, 1, {v(TMPA)}")                            # swz(tile)
    E.i(f"v_xor_b32 {v(TMPA)}, {v(TMPA)}, {v(TQ)}")
    E.i(f"v_lshlrev_b32 {v(TMPA)}, 4, {v(TMPA)}")
    E.i(f"v_lshl_or_b32 {v(TMPA)}, {v(TT)}, 6, {v(TMPA)}")
    E.i(f"s_lshl_b32 {s(S_T0)}, {s(S_T2)}, 1")
    E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, 1")                                # xi_a = 1 (even) or 3 (odd)
    E.i(f"s_mul_i32 {s(S_T0)}, {s(S_T0)}, {6 * VPOS_B}")
    E.i(f"s_lshl_b32 {s(S_T3)}, {s(S_T1)}, 10")                              # g1 * 16 tiles * 64 bytes
    E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, {s(S_T3)}")
    E.i(f"v_add_u32 {v(k.V_VWR)}, {s(S_T0)}, {v(TMPA)}")
    E.i(f"s_mul_i32 {s(S_T0)}, {s(S_T2)}, {5 * 6 * VPOS_B}")                 # xi = 0 (even) or 5 (odd)
    E.i(f"s_xor_b32 {s(S_T3)}, {s(S_T1)}, 1")
    E.i(f"s_lshl_b32 {s(S_T3)}, {s(S_T3)}, 10")
    E.i(f"s_add_u32 {s(S_T0)}, {s(S_T0)}, {s(S_T3)}")
    E.i(f"v_add_u32 {v(k.V_VWR2)}, {s(S_T0)}, {v(TMPA)}")


# --------------------------------------------------------------------------------------------------------------- epilogue
def right_group(E, row_s, pooled):
    """the second block's stores: the right tile group, a run-time number of bytes to the right of the row's scalar offset"""
    E.i(f"s_add_u32 {s(S_T1)}, {s(row_s)}, {s(S_PG1 if pooled else S_G1)}")
    return S_T1, ""


def emit_epilogue(E, pool):
    """units = (tile group, pair of tile columns); lane = (channel j16 of the wave's 16, tile row kq)"""
    E.c("epilogue" + (" + pooling" if pool else ""))
    ep_out_offsets(E)
    E.i(f"s_lshl_b32 {s(S_G1)}, {s(A_PIXOUT)}, 4")                           # 16 pixels to the right
    if pool:
        ep_pool_offsets(E)
        E.i(f"s_lshl_b32 {s(S_PG1)}, {s(A_PIXPOOL)}, 3")                     # 8 pooled pixels to the right
    ep_units(E, pool, right_group)


# ----------------------------------------------------------------------------------------------------------------- kernel
def emit_kernel(E):
    emit_entry(E)
    emit_mfma_lane_constants(E)
    emit_transform_lane_constants(E)
    emit_packed_constants(E, f"s_bitcmp0_b32 {s(L_WAVE)}, 0")                 # even wave: rows 1, 2
    E.checkpoint(1, "arguments loaded, lane constants of the two roles computed")
    emit_dma_lane_constants(E)
    emit_output_constants(E)
    emit_tile_range(E)
    emit_setup_tile(E)
    E.checkpoint(3, "first block decoded, its bias load issued")
    E.i(f"s_mov_b32 {s(N_HAS)}, 1")
    E.i(f"s_mov_b32 {s(L_UOFF)}, {s(N_UBASE)}")
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 0")
    emit_dma_chunk(E, 0)
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 64")
    emit_dma_chunk(E, 1)
    E.i(f"s_mov_b32 {s(L_DMAOFF)}, 128")
    emit_u_ring_fill(E)
    E.checkpoint(5, "first two raw chunks and the U ring requested")
    E.i("s_waitcnt vmcnt(0)")
    E.i("s_branch .Ljoin_A")                                                  # one instruction stream for the four waves (labels .._A)
    # ================================================================================================ tile loop
    E.label(".Ltile_A")
    emit_body(E, 0, "first")
    E.checkpoint(8, "first chunk done")
    E.label(".Lloop_A")
    emit_body(E, 1, "mid")
    E.i(f"s_cmp_eq_u32 {s(L_PAIRS)}, 1")
    E.i("s_cbranch_scc0 .Lnosetup_A")
    # ---- the next block: from here on the LDS-DMA loads fetch ITS first two chunks
    emit_next_tile(E, ".Lnosetup_A")
    E.label(".Lnosetup_A")
    emit_body(E, 0, "mid")
    E.i(f"s_sub_u32 {s(L_PAIRS)}, {s(L_PAIRS)}, 1")
    E.i(f"s_cmp_lg_u32 {s(L_PAIRS)}, 0")
    E.i("s_cbranch_scc1 .Lloop_A")
    emit_body(E, 1, "last")
    E.checkpoint(9, "every chunk of the block done; epilogue next")
    emit_loads_home(E)
    E.i("s_branch .Lepilogue")
    E.label(".Lepi_done_A")
    E.i(f"s_cmp_eq_u32 {s(N_HAS)}, 0")
    E.i("s_cbranch_scc1 .Lend_program")
    E.i(f"s_add_u32 {s(L_TT)}, {s(L_TT)}, {s(L_SLOTS)}")
    E.label(".Ljoin_A")
    emit_join(E)
    E.checkpoint(7, "joined: bias in the accumulators")
    E.i("s_branch .Ltile_A")
    emit_epilogue_dispatch(E, emit_epilogue)
    E.i("s_branch .Lepi_done_A")
    E.label(".Lend_program")
    emit_end(E)


def main():
    argv = sys.argv
    out = argv[1] if len(argv) > 1 else "wino4b_gfx950.s"
    opt = SimpleNamespace(
        stop_at=option(argv, "--stop", 0, int), dump=option(argv, "--dump", ""),
        st_policy=option(argv, "--store-policy", ST_POLICY), dma_pos=option(argv, "--dma-pos", DMA_POS, positions))
    assert len(opt.dma_pos) == DMA_PER_WAVE and len(set(opt.dma_pos)) == DMA_PER_WAVE and max(opt.dma_pos) < 36
    K = layout(option(argv, "--ud", UD, int))
    assert 36 % K.UD == 0 and LDS_BYTES <= 163840
    E = Emitter(K, opt)
    emit_kernel(E)
    print(E.write(out, 10), file=sys.stderr)


if __name__ == "__main__":
    main()
