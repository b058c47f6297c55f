"""The gfx950 assembly hipcc makes of every kernel file, scanned for the one hazard it was caught not padding: a VMEM store of
more than 64 bits whose data registers a VALU overwrites within two wait states (the store reads them after it issues).
hipcc pads it inside a basic block but missed it at a branch join in conv_lpr.hip -- random lanes of a fused-pooling store
were garbage on the GPU (csrc/kernel_common.h: wide_store_guard).  No GPU needed: hipcc cross-compiles."""
import glob
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools", "dev"))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# hipcc is part of the build image (the GPU box runs the same one): its absence FAILS these tests instead of skipping them, so a
# toolchain change cannot silently switch the hazard checks off.  MIUNET_NO_HIPCC_OK=1 restores the skip elsewhere.
NEEDS_HIPCC = pytest.mark.skipif(not os.path.exists(HIPCC) and os.environ.get("MIUNET_NO_HIPCC_OK") == "1", reason="hipcc not installed")


# the Makefile's extra flag for the files whose fully unrolled loops hold many inline-asm MFMAs (the size estimate of an asm trips the
# pragma-unroll limit, and a loop left rolled indexes its register arrays through scratch)
EXTRA_FLAGS = {"conv_wino4.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"], "conv_lpr.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"]}


@NEEDS_HIPCC
@pytest.mark.parametrize("src", sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip"))))
def test_no_wide_store_data_hazard(src, tmp_path):
    import scan_store_hazard
    asm = tmp_path / (src + ".s")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only"]
    flags += EXTRA_FLAGS.get(src, [])
    subprocess.run([HIPCC, *flags, "-o", str(asm), os.path.join(CSRC, src)], check=True, capture_output=True, timeout=600)
    hits = scan_store_hazard.scan(str(asm))
    assert hits == [], "\n".join(hits)


def test_scanner_sees_the_hazard(tmp_path):
    import scan_store_hazard
    s = tmp_path / "h.s"
    s.write_text("\tbuffer_store_dwordx4 v[16:19], v20, s[40:43], s87 offen\n.LBB0_2:\n\tv_add_f32_e32 v16, v114, v0\n"
                 "\tbuffer_store_dwordx4 v[0:3], v9, s[36:39], 0 offen\n\ts_nop 1\n\tv_mov_b32_e32 v0, v5\n"
                 "\tglobal_store_dwordx4 v[8:9], v[4:7], off\n\ts_cbranch_scc1 .LBB0_9\n\ts_endpgm\n.LBB0_9:\n\tv_mov_b32_e32 v6, 0\n")
    hits = scan_store_hazard.scan(str(s))
    assert len(hits) == 2 and "v16" in hits[0] and "v6" in hits[1]


@NEEDS_HIPCC
def test_resident_weight_kernels_do_not_spill(tmp_path):
    """conv_lpr.hip counts its own LDS-DMA loads with vmcnt; a register spill adds scratch loads and stores to the same
    counter, and hipcc's waits for THOSE drain the patch ring (measured: the fused-head variant 0.27 -> 0.53 ms with 24 scratch
    accesses per tile).  Every instantiation must fit its register budget."""
    for src, kernels in (("conv_lpr.hip", 12), ("convt_lpr.hip", 6), ("conv_lprk.hip", 2)):       # shapes x two operand types
        asm = tmp_path / (src + ".s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", *EXTRA_FLAGS.get(src, []), "-o", str(asm),
                        os.path.join(CSRC, src)], check=True, capture_output=True, timeout=600)
        text = asm.read_text()
        assert text.count(".amdhsa_kernel ") >= kernels
        assert "scratch_" not in text, [l for l in text.splitlines() if "scratch_" in l][:5]


LP_SOURCES = ("conv_lp.hip", "conv_lp2.hip", "conv_lpr.hip", "conv_lprk.hip", "convt_lpr.hip")


@NEEDS_HIPCC
@pytest.mark.parametrize("src", LP_SOURCES)
def test_inline_asm_mfmas_have_their_wait_states(src, tmp_path):
    """The 16-bit kernels issue v_mfma_f32_16x16x32 through inline asm (in-place accumulation: csrc/lpr_common.h), and hipcc pads
    nothing around an asm: between such an MFMA and any other access to its destination there must be 12 wait states in the
    instruction stream itself (mfma16_drain), and no VALU may write one of its operands within two states in front of it
    (the chains start from the literal 0, not from a v_mov).  tools/dev/scan_mfma_hazard.py walks the assembly of every
    instantiation; the accumulate chain (the next MFMA taking the destination whole as its C) is exempt."""
    import scan_mfma_hazard
    asm = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", *EXTRA_FLAGS.get(src, []), "-o", str(asm),
                    os.path.join(CSRC, src)], check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    assert text.count("v_mfma_f32_16x16x32") > 100 and "v_mfma_f32_32x32x16" not in text       # one MFMA shape in the 16-bit kernels
    hits = scan_mfma_hazard.scan(str(asm))
    assert hits == [], "\n".join(hits[:10])


def test_mfma_scanner_sees_both_hazards(tmp_path):
    import scan_mfma_hazard
    s = tmp_path / "h.s"
    s.write_text("\tv_mov_b32_e32 v4, 0\n\tv_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]\n"
                 "\tv_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]\n\ts_nop 3\n\tv_add_f32_e32 v0, v5, v1\n\ts_endpgm\n")
    hits = scan_mfma_hazard.scan(str(s))
    assert any("v_add_f32" in h for h in hits) and any("v_mov_b32" in h for h in hits)
    ok = tmp_path / "ok.s"
    ok.write_text("\tv_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], 0\n\tv_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]\n"
                  "\ts_nop 7\n\ts_nop 7\n\tv_add_f32_e32 v0, v5, v1\n\ts_endpgm\n")
    assert scan_mfma_hazard.scan(str(ok)) == []
    # an MFMA at a loop tail against a VALU read at the loop HEAD (the back-edge), and the same loop with the wait states in place
    loop = tmp_path / "loop.s"
    loop.write_text(".LBB0_1:\n\tv_add_f32_e32 v0, v5, v1\n\ts_nop 7\n\ts_nop 7\n\tv_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]\n"
                    "\ts_cbranch_scc1 .LBB0_1\n\ts_nop 7\n\ts_nop 7\n\ts_endpgm\n")
    hits = scan_mfma_hazard.scan(str(loop))
    assert len(hits) == 1 and "v_add_f32" in hits[0]
    loop.write_text(".LBB0_1:\n\ts_nop 7\n\ts_nop 7\n\tv_add_f32_e32 v0, v5, v1\n\tv_mfma_f32_16x16x32_bf16 v[4:7], v[8:11], v[12:15], v[4:7]\n"
                    "\ts_cbranch_scc1 .LBB0_1\n\ts_nop 7\n\ts_nop 7\n\ts_endpgm\n")
    assert scan_mfma_hazard.scan(str(loop)) == []


# ------------------------------------------------------------------------------------------ the generated assembly kernel
GEN = os.path.join(CSRC, "asm", "gen_wino4_asm.py")
GEN_B = os.path.join(CSRC, "asm", "gen_wino4b_asm.py")
LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def test_assembly_kernel_scanner_sees_each_hazard(tmp_path):
    """the assembler pads nothing: tools/dev/scan_asm_kernel.py must flag each wait state LLVM's hazard recognizer would have inserted"""
    import scan_asm_kernel
    cases = {
        "readfirstlane": "\tv_lshrrev_b32 v2, 6, v1\n\tv_readfirstlane_b32 s71, v2\n\ts_endpgm\n",
        "sgpr_valu": "\tv_cmp_gt_u32 vcc, s18, v216\n\ts_nop 0\n\tv_cndmask_b32 v199, -1, v216, vcc\n\ts_endpgm\n",
        "sgpr_vmem": "\tv_readfirstlane_b32 s68, v2\n\ts_nop 2\n\tbuffer_load_dwordx4 v[0:3], v190, s[44:47], s68 offen\n\ts_endpgm\n",
        "m0": "\ts_add_u32 m0, s1, 4096\n\tbuffer_load_dwordx4 v199, s[40:43], s69 offen lds\n\ts_endpgm\n",
        "mfma": "\tv_mfma_f32_16x16x4_f32 a[0:3], v72, v0, a[0:3]\n\ts_nop 7\n\tv_accvgpr_read_b32 v80, a1\n\ts_endpgm\n",
        "loop": ".Lhead:\n\tv_accvgpr_read_b32 v80, a1\n\ts_nop 7\n\ts_nop 7\n\tv_mfma_f32_16x16x4_f32 a[0:3], v72, v0, a[0:3]\n\ts_cbranch_scc1 .Lhead\n\ts_endpgm\n",
    }
    for name, text in cases.items():
        p = tmp_path / (name + ".s")
        p.write_text(text)
        assert len(scan_asm_kernel.scan(str(p))) == 1, name
    ok = tmp_path / "ok.s"
    ok.write_text("\tv_lshrrev_b32 v2, 6, v1\n\ts_nop 0\n\tv_readfirstlane_b32 s71, v2\n\ts_nop 1\n\tv_add_u32 v3, s71, v2\n"
                  "\ts_add_u32 m0, s1, 4096\n\ts_nop 0\n\tbuffer_load_dwordx4 v199, s[40:43], s69 offen lds\n"
                  "\tv_mfma_f32_16x16x4_f32 a[0:3], v72, v0, 0\n\tv_mfma_f32_16x16x4_f32 a[0:3], v73, v1, a[0:3]\n\ts_nop 7\n\ts_nop 3\n\tv_accvgpr_read_b32 v80, a1\n\ts_endpgm\n")
    assert scan_asm_kernel.scan(str(ok)) == []


@NEEDS_HIPCC
def test_generated_assembly_kernel_assembles_and_has_its_wait_states(tmp_path):
    """csrc/asm/gen_wino4_asm.py -> gfx950 assembly: assembles with the ROCm clang, carries every wait state the assembler does not
    insert, is padded behind s_endpgm (the instruction prefetcher runs past it), and declares the LDS / registers it uses."""
    import scan_asm_kernel
    asm = tmp_path / "wino4a.s"
    subprocess.run([sys.executable, GEN, str(asm)], check=True, capture_output=True, timeout=300)
    text = asm.read_text()
    assert text.count("v_mfma_f32_16x16x4_f32") == 2 * 4 * 288          # two roles x (first, two middle, last) chunk bodies
    assert ".amdhsa_group_segment_fixed_size 147456" in text and ".amdhsa_next_free_vgpr 512" in text and ".amdhsa_accum_offset 256" in text
    tail = text[text.rindex("s_endpgm"):]
    assert ".fill 256, 4, 3212836864" in tail                            # s_nop pad behind the end of the program
    assert scan_asm_kernel.scan(str(asm)) == []
    obj = tmp_path / "wino4a.o"
    subprocess.run([os.path.join(LLVM_BIN, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(asm), "-o", str(obj)],
                   check=True, capture_output=True, timeout=300)
    assert obj.stat().st_size > 40000
    # the sibling kernel for the 64-channel layers (gen_wino4b_asm.py): the whole 160 KB of LDS, same checks
    asm_b = tmp_path / "wino4b.s"
    subprocess.run([sys.executable, GEN_B, str(asm_b)], check=True, capture_output=True, timeout=300)
    tb = asm_b.read_text()
    assert tb.count("v_mfma_f32_16x16x4_f32") == 4 * 288 and ".amdhsa_group_segment_fixed_size 163840" in tb          # one stream for the four waves
    assert ".fill 256, 4, 3212836864" in tb[tb.rindex("s_endpgm"):]
    assert scan_asm_kernel.scan(str(asm_b)) == []
    subprocess.run([os.path.join(LLVM_BIN, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(asm_b), "-o", str(obj)],
                   check=True, capture_output=True, timeout=300)
    # every timing-only / dump / stamp variant of the generator still assembles (they are bring-up tools, never shipped)
    variants = [(GEN, flags) for flags in (["--stamps"], ["--stop", "5", "--dump", "lds"], ["--timing-only", "nouload,novread,notransform,nodma"],
                                           ["--dma-pos", "0,4,8,12,16,20"])]
    variants += [(GEN_B, flags) for flags in (["--ud", "6"], ["--ud", "9"], ["--store-policy", "nt"], ["--dma-pos", "0,1,2,3,4,5,6,7,8,9,10"],
                                              ["--stop", "5", "--dump", "lds"])]
    for gen, flags in variants:
        v = tmp_path / "variant.s"
        subprocess.run([sys.executable, gen, str(v)] + flags, check=True, capture_output=True, timeout=300)
        subprocess.run([os.path.join(LLVM_BIN, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(v), "-o", str(obj)],
                       check=True, capture_output=True, timeout=300)
