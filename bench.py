#!/usr/bin/env python3
"""bench.py -- images/sec of the UNet inference hot path on MI355X (BASELINE.json metric), one process per GPU.

A step = one pass of the hot path (u8 tiles resident in HBM -> UNet forward -> u8 label maps in HBM) over one batch of
16 synthetic 512x512x1 images per GPU (BASELINE.json configs[1]); for N > 1 ranks each rank processes its own shard
(weak scaling) and the per-batch label maps are gathered to rank 0 over RCCL inside the timed region, after the
weights were broadcast from rank 0 over RCCL at start-up (north_star: "RCCL-over-xGMI broadcast of weights and
per-rank gather of mask tensors").

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full [--no-cpu-baseline] [--no-extras]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

`python bench.py --gpus N` with N > 1 and no torchrun environment starts that torchrun command itself as a CHILD
process (before this process touches the GPU) and returns its exit code.

A plain run measures the headline and nothing else: set-up (weights, image sets, the first eager pass of each graph key), W
warm-up steps, K timed steps (`value`, `ms_per_step`), the label maps of the last timed step written to DIR/labels.npy
(float32; beyond 64 MB a fixed, seeded sample of whole images, listed in DIR/labels_index.npy) when --dump-outputs is given,
and the JSON line.  Every other record and check below (1 and 3-7, the label-map checks of 2) runs only under --full.

What --full runs, in this order (DESIGN.md "Measurement" describes every field of the ONE JSON line rank 0 prints):
  1. parity gate   the first images of the timed batch against the oracle (labels equal wherever the oracle's top-2
                   margin exceeds 1e-3, logits within 1e-3); a mismatch makes the run exit non-zero
  2. `value`       W warm-up steps, then K steps of the SHIPPED path (hipGraph replay, profiling off) between
                   barrier + synchronize fences
  3. `roofline`    K more steps with an event pair around every launch (eager launches) for the per-kernel figures
  4. `e2e_host`    the same batch through mi_unet_infer_u8 (pinned H2D + D2H inside), N = 1 only
  5. `configs`     short driver-measured runs of BASELINE configs[2] (bf16, batch 128) and configs[4] (fp16, 1024^2 x 3)
  6. `pipeline`    RAW16 -> polygons in one device call next to the facade's host route and the all-CPU chain
  6b. `group`      mi_unet_group_infer_u8 (the C++ host's own multi-GPU path, ONE process) on a batch of 512 over every visible
                   device, both gather modes -- in a child process with a deadline
  With N > 1 ranks (or BENCH_FORCE_DIST=1) `configs` carries BASELINE configs[3] measured in the same launch: global batch
  512 in contiguous shards, label maps gathered over RCCL inside the timed region ("scaling": "strong").
  7. `cpu_baseline` the oracle on the host cores over a bounded sample of the same workload
"""
import argparse
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd")
sys.path.insert(0, PKG)

# ONE set of peaks prices every roofline figure of this file and of profiles/summarize_pmc.py: the NOMINAL ones of
# MI355X_MICROARCH.md (2.4 GHz).  The kernel headers (csrc/conv_lpr.hip, conv_lp2.hip) also quote what this card SUSTAINS -- 1.89
# PFLOP/s for a register-only bf16 MFMA loop (the clock drops to 1.80 GHz under dense 16-bit matrix work), 6.29 TB/s for an HBM copy
# -- as the practical ceilings their design notes argue against; those are never the denominator of a reported fraction.
FP32_PEAK_TFLOPS = 157.3      # fp32 matrix peak (v_mfma_f32_32x32x2_f32 / 16x16x4_f32); the fp32 loop holds 2.38 GHz: 155.6 TF/s measured
LP_PEAK_TFLOPS = 2500.0       # dense bf16 / fp16 MFMA peak (the same per clock for v_mfma_f32_16x16x32 and 32x32x16; the kernels use 16x16x32)
HBM_PEAK_GBS = 8000.0

# multiplies the MFMA pipe executes per algorithmic (direct-convolution) multiply, by kernel family
WINOGRAD_REDUCTION = {"conv3x3_wino4": 4.0, "conv3x3_wino4a": 4.0, "conv3x3_wino4b": 4.0, "conv3x3_wino4s": 4.0, "conv3x3_wino": 2.25, "conv3x3_wino16": 2.25}
CONV_FAMILIES = ("conv3x3_mfma", "conv3x3_wino", "conv3x3_wino16", "conv3x3_wino4", "conv3x3_wino4a", "conv3x3_wino4b", "conv3x3_wino4s", "conv3x3_bf16", "conv3x3_fp16",
                 "conv3x3_bf16w", "conv3x3_fp16w", "conv3x3_bf16r", "conv3x3_fp16r", "conv3x3_bf16k", "conv3x3_fp16k")
LP_FAMILIES = ("conv3x3_bf16", "conv3x3_fp16", "conv3x3_bf16w", "conv3x3_fp16w", "conv3x3_bf16r", "conv3x3_fp16r", "conv3x3_bf16k", "conv3x3_fp16k", "convT2x2_bf16",
               "convT2x2_fp16", "convT2x2_bf16r", "convT2x2_fp16r")
ROCPROF_NAME = {"conv3x3_wino": "miunet::conv3x3_wino_f32<*>", "conv3x3_wino16": "miunet::conv3x3_wino16_f32",
                "conv3x3_wino4": "miunet::conv3x3_wino4_f32<*>", "conv3x3_wino4a": "conv3x3_wino4a_f32", "conv3x3_wino4b": "conv3x3_wino4b_f32", "conv3x3_wino4s": "miunet::conv3x3_wino4s_f32<*>",
                "conv3x3_mfma": "miunet::conv_mfma_f32<*>", "convT2x2_taps": "miunet::convT2x2_taps_f32<*>",
                "convT2x2_mfma": "miunet::conv_mfma_f32<*>", "conv3x3_first": "miunet::conv3x3_first_kernel<*>",
                "conv3x3_bf16": "miunet::conv_mfma_bf16<*>", "conv3x3_fp16": "miunet::conv_mfma_bf16<*>",
                "convT2x2_bf16": "miunet::conv_mfma_bf16<*>", "convT2x2_fp16": "miunet::conv_mfma_bf16<*>",
                "conv3x3_bf16w": "miunet::conv3x3_lp2n<*>", "conv3x3_fp16w": "miunet::conv3x3_lp2n<*>",
                "conv3x3_bf16r": "miunet::conv3x3_lpr<*>", "conv3x3_fp16r": "miunet::conv3x3_lpr<*>",
                "conv3x3_bf16k": "miunet::conv3x3_lprk<*>", "conv3x3_fp16k": "miunet::conv3x3_lprk<*>",
                "convT2x2_bf16r": "miunet::convT2x2_lpr<*>", "convT2x2_fp16r": "miunet::convT2x2_lpr<*>"}


def family(kernel):
    """kernel family of a launch: the fused-head launches of a conv kernel belong to that kernel"""
    return kernel.split("+")[0]


def kernel_source_sha():
    """sha256 over the kernel and engine sources: a committed PMC summary is only quoted while it still describes them"""
    h = hashlib.sha256()
    for p in sorted(glob.glob(os.path.join(PKG, "csrc", "*")) + glob.glob(os.path.join(PKG, "csrc", "asm", "*"))):
        if os.path.isfile(p):
            h.update(os.path.basename(p).encode())
            h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def pmc_summary(tag):
    """HBM bytes per launch / MFMA busy of the dominant kernel from the committed rocprofv3 PMC passes of this same command
    (counters cannot be read from inside the process).  A summary whose recorded source hash is not the tree's is stale and
    is NOT quoted.  tag: "fp32" | "bf16" | "fp16" selects profiles/r*_pmc_<tag>.json."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_{tag}.json")))
    if not files:
        return None, "no PMC summary committed for this plan"
    try:
        d = json.load(open(files[-1]))
    except ValueError:
        return None, f"{os.path.basename(files[-1])}: unreadable"
    if d.get("kernel_source_sha") != kernel_source_sha():
        return None, f"{os.path.basename(files[-1])} predates the current kernels (source hash differs): not quoted"
    return d, "profiles/" + os.path.basename(files[-1])


def oracle():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as orc
    return orc


def cpu_baseline(blob, h, w, in_ch, probe_s):
    """Oracle (oracle/liboracle.so: the CPU restatement, kind "port") timed on this host's cores on a bounded sample of the
    bench workload; `probe_s` = seconds one image took in the parity gate (sizes the sample to about 10-30 s)."""
    import numpy as np
    from miunet import synth
    orc = oracle()
    cores = int(orc.lib().orc_num_threads())
    n = int(min(32, max(1, np.ceil(20.0 / max(probe_s, 1e-3)))))
    imgs = synth.make_images(n, h, w, in_ch, 0x5EED, "bytes")
    t0 = time.perf_counter()
    orc.unet_forward(blob, imgs, want_logits=False)
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "images/s", "cores": cores, "kind": "port",
            "sample": f"{n} image(s) {h}x{w}x{in_ch} of the same synthetic workload through oracle/unet_oracle.c "
                      f"(normalise + UNet forward + argmax; OpenMP, {cores} threads), {dt:.2f} s",
            "ms_per_image": dt / n * 1e3}


def parity_gate(eng, blob, imgs_host, n, mode="fp32"):
    """The first n images of the timed batch, device vs oracle.  fp32: logits within 1e-3 and labels equal wherever the
    oracle's top-2 margin exceeds 1e-3 (BASELINE north_star).  bf16 / fp16: against the oracle fed with identically
    rounded operands, at the tolerances of tests/test_gpu_bf16.py (the 16-bit networks amplify rounding noise:
    DESIGN.md 5.1), labels compared with the fp32 oracle's where ITS margin is wide."""
    import numpy as np
    orc = oracle()
    sub = np.ascontiguousarray(imgs_host[:n])
    t0 = time.perf_counter()
    ref_logits, ref_labels = orc.unet_forward(blob, sub)
    oracle_s = (time.perf_counter() - t0) / n
    labels, logits = eng.infer(sub, want_logits=True)
    srt = np.sort(ref_logits, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    rec = {"images": n, "against": "oracle/unet_oracle.c (fp32)"}
    if mode == "fp32":
        tol, mtol = 1e-3, 1e-3
        err = float(np.max(np.abs(logits - ref_logits)))
    else:
        # A 16-bit-operand network is not reproducible to fp32 tolerance by ANY second implementation: a 1e-7 upstream
        # difference flips some roundings of the activations.  The bar is the size of the quantisation noise
        # itself: no further from the fp32 oracle than 1.5 x the distance of the oracle's own 16-bit mode (every kernel is
        # pinned at 1e-4 on identical operands in tests/test_gpu_bf16.py).
        lp_logits, _ = orc.unet_forward(blob, sub, bf16=(mode == "bf16"), fp16=(mode == "fp16"))
        noise = float(np.max(np.abs(lp_logits - ref_logits)))
        tol, mtol = 1.5 * noise + 1e-3, (0.1 if mode == "bf16" else 2e-2)
        err = float(np.max(np.abs(logits - ref_logits)))
        rec["against"] = f"fp32 oracle, tolerance = 1.5 x the {mode}-operand oracle's own distance to it + 1e-3"
        rec["oracle_16bit_noise"] = noise
        rec["max_abs_err_vs_16bit_oracle"] = float(np.max(np.abs(logits - lp_logits)))
    safe = margin > mtol
    bad = int((labels[safe] != ref_labels[safe]).sum())
    rec.update({"max_abs_logit_err": err, "logit_tolerance": tol, "margin": mtol,
                "mismatches_above_margin": bad, "mismatches_below_margin": int((labels[~safe] != ref_labels[~safe]).sum()),
                "pixels_compared": int(safe.sum()), "ok": bool(bad == 0 and err < tol)})
    return rec, oracle_s


VERBOSE = False               # --verbose: the per-family arrays stay in the JSON line (they always go to gpurun_out/bench_families.json)
FAMILY_TABLES = {}


def roofline_from_stats(stats, spec_macs, ips_per_gpu, tag):
    """Per-kernel figures of the dominant conv kernel from the engine's own per-launch event pairs."""
    by = {}
    for s in stats:
        f = family(s["kernel"])
        if f in CONV_FAMILIES:
            by[f] = by.get(f, 0.0) + s["ms"]
    dom_kernel = max(by, key=by.get) if by else "conv3x3_mfma"
    dom = [s for s in stats if family(s["kernel"]) == dom_kernel]
    dom_flops = sum(s["flops"] for s in dom)
    dom_ms = sum(s["ms"] for s in dom)
    all_ms = sum(s["ms"] for s in stats)
    lp = dom_kernel in LP_FAMILIES
    peak = LP_PEAK_TFLOPS if lp else FP32_PEAK_TFLOPS
    red = WINOGRAD_REDUCTION.get(dom_kernel, 1.0)
    algorithmic = dom_flops / (dom_ms * 1e-3) / 1e12 if dom_ms else 0.0
    executed = algorithmic / red
    insn = ("v_mfma_f32_16x16x32_f16" if "fp16" in dom_kernel else "v_mfma_f32_16x16x32_bf16" if lp
            else "v_mfma_f32_16x16x4_f32" if dom_kernel in ("conv3x3_wino4", "conv3x3_wino4a", "conv3x3_wino4b") else "v_mfma_f32_32x32x2_f32")
    pmc, pmc_src = pmc_summary(tag)
    rk = (pmc or {}).get("kernels", {}).get(ROCPROF_NAME.get(dom_kernel, ""), {})
    # every kernel family of the step, same arithmetic: executed = algorithmic / winograd_reduction (1 for the direct forms)
    fam = {}
    for s in stats:
        e = fam.setdefault(family(s["kernel"]), [0, 0.0, 0.0, 0.0])
        e[0] += 1; e[1] += s["ms"]; e[2] += s["flops"]; e[3] += s["bytes"]
    families = []
    for name, (n, ms, fl, by) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        r = WINOGRAD_REDUCTION.get(name, 1.0)
        pk = LP_PEAK_TFLOPS if name in LP_FAMILIES else FP32_PEAK_TFLOPS
        c = (pmc or {}).get("kernels", {}).get(ROCPROF_NAME.get(name, ""), {})
        families.append({"kernel": name, "launches": n, "share_of_device_time": ms / all_ms if all_ms else None,
                         "avg_launch_ms": ms / n, "algorithmic_tflops": fl / ms / 1e9, "executed_tflops": fl / ms / 1e9 / r,
                         "frac_of_mfma_peak": fl / ms / 1e9 / r / pk, "algorithmic_gbs": by / ms / 1e6,
                         "frac_of_hbm_peak": by / ms / 1e6 / HBM_PEAK_GBS,
                         "mfma_busy_pmc": c.get("mfma_busy"), "hbm_bytes_per_launch_pmc": c.get("hbm_bytes_per_launch")})
    FAMILY_TABLES[tag] = families
    rec = {
        "bound": "mfma", "kernel": f"{dom_kernel} ({insn})",
        "algorithm": {4.0: "winograd F(4x4,3x3)", 2.25: "winograd F(2x2,3x3)"}.get(red, "direct implicit GEMM"),
        # the roofline fraction: FLOPs the matrix pipe EXECUTES per second over its peak (never above 1)
        "achieved": executed, "peak": peak, "unit": "TFLOP/s", "frac": executed / peak,
        "achieved_basis": "executed MFMA FLOPs = algorithmic (direct-convolution) FLOPs / winograd_reduction",
        "algorithmic_tflops": algorithmic, "winograd_reduction": red,
        "traffic": rk.get("hbm_bytes_per_launch"), "mfma_busy": rk.get("mfma_busy"),
        "mfma_busy_at_measured_clock": rk.get("mfma_busy_at_measured_clock"), "clock_ghz_from_sq_busy": rk.get("clock_ghz_from_sq_busy"),
        "pmc_source": pmc_src,
        "launches": len(dom), "avg_launch_ms": dom_ms / max(1, len(dom)),
        "avg_launch_gflop": dom_flops / max(1, len(dom)) / 1e9,
        "share_of_device_time": dom_ms / all_ms if all_ms else None,
        "whole_net_algorithmic_tflops": 2.0 * spec_macs * ips_per_gpu / 1e12,
    }
    # the driver keeps only the tail of stdout: the per-family arrays (22-27 numbers each) pushed configs[2]'s value out of
    # BENCH_r03.json.  They go to gpurun_out/bench_families.json; the line carries them only under --verbose.
    if VERBOSE:
        rec["families"] = families
    else:
        rec["families_compact"] = {f["kernel"]: [f["launches"], round(f["share_of_device_time"] or 0, 3), round(f["frac_of_mfma_peak"], 3)] for f in families}
        rec["families_compact_columns"] = ["launches", "share_of_device_time", "executed_frac_of_mfma_peak"]
    return rec


def per_layer_table(stats, steps, wall_ms):
    per = {}
    for s in stats:
        e = per.setdefault(s["name"], [s["kernel"], 0.0, 0.0, 0.0, 0])
        e[1] += s["ms"]; e[2] += s["flops"]; e[3] += s["bytes"]; e[4] += 1
    print(f"{'layer':14s} {'kernel':20s} {'ms/launch':>10s} {'TFLOP/s':>9s} {'GB/s(alg)':>10s}", file=sys.stderr)
    for name, (k, ms, fl, by, n) in per.items():
        print(f"{name:14s} {k:20s} {ms / n:10.3f} {fl / ms / 1e9:9.1f} {by / ms / 1e6:10.0f}", file=sys.stderr)
    print(f"sum of kernel time per step: {sum(s['ms'] for s in stats) / steps:.3f} ms; wall per step (graph replay): "
          f"{wall_ms:.3f} ms", file=sys.stderr)


def run_config(binding, synth, torch, dev, stream, name, spec, H, B, max_batch, algo, steps, warmup, tol_mode):
    """One of the other BASELINE configs, short: parity gate on one image, K timed graph-replay steps, one profiled step."""
    from miunet.spec import pack_weights
    blob = pack_weights(spec, synth.make_weights(spec, 1234))
    imgs_host = synth.make_images(B, H, H, spec.in_ch, 0x5EED, "bytes")
    with binding.Engine(H, H, spec.in_ch, spec.base, spec.levels, spec.classes, max_batch=max_batch, device=dev.index,
                        conv_algo=algo) as eng:
        eng.load_weights(blob)
        par, _ = parity_gate(eng, blob, imgs_host, 1, tol_mode)
        eng.set_stream(stream.cuda_stream)
        imgs = torch.from_numpy(imgs_host).to(dev)
        labels = torch.empty((B, H, H), dtype=torch.uint8, device=dev)
        for _ in range(warmup):
            eng.infer_device(imgs.data_ptr(), B, labels.data_ptr(), 0)
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.infer_device(imgs.data_ptr(), B, labels.data_ptr(), 0)
        stream.synchronize()
        dt = time.perf_counter() - t0
        eng.set_profiling(True)
        eng.infer_device(imgs.data_ptr(), B, labels.data_ptr(), 0)
        stats = eng.kernel_stats()
        eng.set_profiling(False)
    ips = B * steps / dt
    return {"config": name, "value": ips, "unit": "images/s", "ms_per_image": 1e3 / ips, "batch": B, "micro_batch": max_batch,
            "steps": steps, "warmup": warmup, "dtype": {"bf16": "bf16", "fp16": "fp16"}.get(algo, "fp32"), "parity": par,
            "roofline": roofline_from_stats(stats, spec.macs_per_image(H, H), ips, tol_mode)}


def run_pipeline(binding, synth, dev_index, nimg=16):
    """SURVEY 8f rows f1-f3 as one record: RAW16 2048x1536 -> tile -> UNet -> postprocess -> contours.
      device_one_call : mi_unet_segment_raw16 (host RAW buffers in, tiles / masks / contours out), everything on the GPU
      facade_device   : MedicalSeg::process_image_batch, files in, the five artefacts per image out (all-device route)
      facade_host     : the same with MEDSEG_HOST_PREPROCESS/POSTPROCESS/CONTOURS=1 -- CPU pre/post/contours around the GPU
                        network, the reference's own stage order (src/process.cpp:188-262)
      cpu_chain       : the oracle's chain for ONE image, all on the CPU (preprocess + UNet + postprocess + contours):
                        the closest thing to the reference's process() without a GPU"""
    import numpy as np
    from miunet import hostlib
    from miunet.spec import UNetSpec, pack_weights
    orc = oracle()
    spec = UNetSpec()
    blob = pack_weights(spec, synth.make_threshold_weights(spec))
    raws = [synth.make_raw16(1536, 2048, seed=100 + i) for i in range(nimg)]
    out = {"workload": f"{nimg} synthetic RAW16 images 2048x1536 -> 512x512 tiles, intensity-threshold weights (structured "
                       "masks so contours exist), 4-level base-64 fp32 UNet"}
    with binding.Engine(512, 512, max_batch=nimg, device=dev_index) as eng:
        eng.load_weights(blob)

        def timed(images):
            """the C call alone -- argument block and output buffers prepared once, Python decoding outside the clock"""
            prep = eng.segment_raw16_prepare(images, 1 << 15, 64)
            for _ in range(2):
                eng.segment_raw16_run(prep)                              # warm-up: staging buffers grow, graphs are captured
            reps = 5
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.segment_raw16_run(prep)
            dt = (time.perf_counter() - t0) / reps
            return dt, eng.last_stage_ms(), eng.segment_raw16_decode(prep)

        dt, stages, (tiles, masks, cont) = timed(raws)
        # the same images in page-locked host memory (mi_unet_host_alloc): no staging copy on the calling thread
        pins = [binding.PinnedArray(r.shape, np.uint16) for r in raws]
        for pa, r in zip(pins, raws):
            pa.a[...] = r
        dt_p, stages_p, (tiles_p, masks_p, cont_p) = timed([pa.a for pa in pins])
        pinned_same = bool(np.array_equal(tiles_p, tiles) and np.array_equal(masks_p, masks) and cont_p == cont)
        tiles, masks = tiles.copy(), masks.copy()
        for pa in pins:
            pa.close()
        # the steady state: 64 images through the same engine (micro-batches of 16), where the first chunk's exposed upload and the
        # last chunk's exposed postprocess + contours are amortised over four network passes instead of one
        raws64 = raws + [r.copy() for r in raws * 3]
        dt64, stages64, (_, masks64, cont64) = timed(raws64)
        b64_same = bool(all(np.array_equal(masks64[i], masks[i % nimg]) and cont64[i] == cont[i % nimg] for i in range(0, 64, 7)))
        del raws64
    out["device_one_call"] = {"images_per_s": nimg / dt, "ms_per_image": dt / nimg * 1e3,
                              "contours_first_image": len(cont[0]) if cont[0] is not None else -1, "stages_ms": stages,
                              "what": "mi_unet_segment_raw16, RAW images in ordinary (pageable) host memory"}
    out["device_one_call_pinned"] = {"images_per_s": nimg / dt_p, "ms_per_image": dt_p / nimg * 1e3, "stages_ms": stages_p,
                                     "same_results": pinned_same,
                                     "what": "the same call with the RAW images in page-locked host memory (mi_unet_host_alloc)"}
    out["device_one_call_b64"] = {"images_per_s": 64 / dt64, "ms_per_image": dt64 / 64 * 1e3, "stages_ms": stages64, "same_results": b64_same,
                                  "what": "the same call on 64 images (the 16 above four times over), micro-batches of 16"}
    # parity of image 0 against the oracle chain, which is also the all-CPU timing sample
    t0 = time.perf_counter()
    tile0 = orc.preprocess_raw(raws[0])
    _, lab0 = orc.unet_forward(blob, tile0[None, ..., None], want_logits=False)
    vis0 = orc.mask_to_image(orc.postprocess_mask(lab0[0]))
    cont0 = orc.find_contours(vis0)
    cpu_s = time.perf_counter() - t0
    out["cpu_chain"] = {"images_per_s": 1.0 / cpu_s, "ms_per_image": cpu_s * 1e3, "cores": int(orc.lib().orc_num_threads()),
                        "sample": "1 image: orc_preprocess_raw + orc_unet_forward + orc_postprocess_mask + orc_find_contours"}
    out["parity"] = {"tile_equal": bool(np.array_equal(tiles[0], tile0)), "mask_equal": bool(np.array_equal(masks[0], vis0)),
                     "contours_equal": cont[0] == cont0}
    out["parity"]["pinned_route_equal"] = pinned_same
    out["parity"]["ok"] = all(out["parity"].values())
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "engine"))
        wp = os.path.join(d, "engine", "unet.miw")
        open(wp, "wb").write(blob)
        paths = []
        for i, r in enumerate(raws):
            p = os.path.join(d, f"img{i:03d}.raw")
            r.tofile(p)
            paths.append(p)
        ws, hs = [2048] * nimg, [1536] * nimg
        os.environ["MEDSEG_DEVICES"] = "1"                          # this record is a ONE-GPU figure whatever the node holds
        out["facade_devices"] = 1
        for route, env in (("facade_device", "0"), ("facade_host", "1")):
            for k in ("MEDSEG_HOST_PREPROCESS", "MEDSEG_HOST_POSTPROCESS", "MEDSEG_HOST_CONTOURS"):
                os.environ[k] = env
            od = os.path.join(d, "out_" + route)
            os.makedirs(od)
            devnull = os.open(os.devnull, os.O_WRONLY)
            saved = os.dup(1)
            sys.stdout.flush()
            os.dup2(devnull, 1)                                   # the facade prints a line per image
            try:
                if not hostlib.initialize_engine(wp, os.path.join(d, "log_" + route)):
                    raise RuntimeError("facade initialize_engine failed")
                if route == "facade_host":
                    ok = sum(hostlib.process_single_image(p, 2048, 1536, od) for p in paths[:2])      # warm-up
                    t0 = time.perf_counter()
                    ok = sum(hostlib.process_single_image(p, 2048, 1536, od) for p in paths)
                else:
                    hostlib.process_image_batch(paths, ws, hs, od)                                     # warm-up
                    t0 = time.perf_counter()
                    ok = hostlib.process_image_batch(paths, ws, hs, od)
                dt = time.perf_counter() - t0
                if route == "facade_device":
                    # the reference's own call pattern: MedicalSeg::process_single_image in a loop, one image per call
                    od1 = os.path.join(d, "out_single")
                    os.makedirs(od1)
                    for p in paths[:3]:
                        hostlib.process_single_image(p, 2048, 1536, od1)                               # warm-up
                    t1 = time.perf_counter()
                    ok1 = sum(hostlib.process_single_image(p, 2048, 1536, od1) for p in paths)
                    dt1 = time.perf_counter() - t1
                    log_text = open(hostlib.get_log_path()).read()
                    stage_lines = [l for l in log_text.splitlines() if "Stage times (ms):" in l]
                    out["facade_numeric_guard"] = next((l.strip() for l in log_text.splitlines() if "numeric guard" in l), None)
                    single = {"single_image_ms": dt1 / nimg * 1e3, "images_per_s": nimg / dt1, "succeeded": int(ok1),
                              "what": "MedicalSeg::process_single_image per file (mapped RAW -> one device call -> five artefacts "
                                      "written concurrently), 2048x1536 RAW16"}
                    if stage_lines:
                        import re
                        vals = [[float(x) for x in re.findall(r"(?<![\w.])(\d+\.\d+)", l.split("Stage times (ms):")[1])] for l in stage_lines[-nimg:]]
                        names = ["read", "device_call", "upload_preprocess", "network", "postprocess", "contours", "download", "artefacts",
                                 "normalized_png_and_sizes_json", "mask_png", "overlay_png_and_polygon_json"]
                        if all(len(v) == len(names) for v in vals):
                            single["stages_ms_mean"] = {n: sum(v[i] for v in vals) / len(vals) for i, n in enumerate(names)}
                    out["facade_single_image"] = single
                hostlib.cleanup_resources()
            finally:
                os.dup2(saved, 1)
                os.close(saved)
                os.close(devnull)
            out[route] = {"images_per_s": nimg / dt, "ms_per_image": dt / nimg * 1e3, "succeeded": int(ok),
                          "artefacts": "normalized.png, original_sizes.json, mask.png, contour_overlay.png, polygon json"}
        for k in ("MEDSEG_HOST_PREPROCESS", "MEDSEG_HOST_POSTPROCESS", "MEDSEG_HOST_CONTOURS"):
            os.environ.pop(k, None)
    return out


def run_pipeline_config5(binding, synth, dev_index, nimg=8):
    """BASELINE configs[4] as BASELINE.json states it -- "1024x1024 3-channel input, 5-level UNet (base=32ch) fp16, fused preprocess
    + on-device mask2polygon contour extraction" -- as ONE call: nimg images x 3 RAW16 planes 2048x1536 -> mi_unet_segment_raw16
    on the 1024^2 x 3 fp16 engine -> tiles, masks, polygons.  Gated on exact parity of image 0 against the oracle chain (the
    structured weights make the label maps exact under fp16 operands; tests/test_gpu_group.py::test_config5_in_one_call_...).
    Reference seam: src/process.cpp:211-242."""
    import numpy as np
    from miunet.spec import UNetSpec, pack_weights
    orc = oracle()
    spec = UNetSpec(3, 32, 5, 3)
    blob = pack_weights(spec, synth.make_threshold_weights(spec))
    planes = [synth.make_raw16(1536, 2048, seed=300 + k) for k in range(3 * nimg)]
    out = {"config": "BASELINE.json configs[4] (whole): 1024x1024x3, 5-level base 32, fp16 operands / fp32 accumulate, fused preprocess "
                     "(three RAW16 planes 2048x1536 per image) + device postprocess + on-device mask2polygon contour extraction, one call",
           "images": nimg, "dtype": "fp16"}
    with binding.Engine(1024, 1024, 3, 32, 5, 3, max_batch=nimg, device=dev_index, conv_algo="fp16") as eng:
        eng.load_weights(blob)
        prep = eng.segment_raw16_prepare(planes, 1 << 16, 64)
        for _ in range(2):
            eng.segment_raw16_run(prep)
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.segment_raw16_run(prep)
        dt = (time.perf_counter() - t0) / reps
        stages = eng.last_stage_ms()
        tiles, masks, cont = eng.segment_raw16_decode(prep)
        tiles, masks = tiles.copy(), masks.copy()
    out.update({"value": nimg / dt, "unit": "images/s", "ms_per_image": dt / nimg * 1e3, "stages_ms": stages,
                "what": "mi_unet_segment_raw16 from pageable host memory (PCIe-inclusive: 3 x 6 MB of RAW16 per image go up, a "
                        "3 MB tile, a 1 MB mask and the contour points come back)"})
    tile0 = np.stack([orc.preprocess_raw(planes[c], 1024, 1024) for c in range(3)], axis=-1)
    _, lab0 = orc.unet_forward(blob, tile0[None], want_logits=False, fp16=True)
    vis0 = orc.mask_to_image(orc.postprocess_mask(lab0[0]))
    cont0 = orc.find_contours(vis0)
    out["parity"] = {"tile_equal": bool(np.array_equal(tiles[0], tile0)), "mask_equal": bool(np.array_equal(masks[0], vis0)),
                     "contours_equal": cont[0] == cont0, "contours_first_image": len(cont0), "mask_nonempty": bool(vis0.max() == 255)}
    out["parity"]["ok"] = all(bool(v) for v in out["parity"].values())
    return out


def summary_of(out):
    """the headline figures once more, compact, as the LAST key of the line (the driver keeps the tail of stdout)"""
    wl = out["config"]["workload"]
    head = (wl.split(":")[0].replace("BASELINE.json ", "") if wl.startswith("BASELINE.json") else "custom") + "_" + str(out["dtype"])
    s = {head + "_images_per_s": round(out["value"], 1), "ms_per_step": round(out["ms_per_step"], 3),
         "roofline_frac": round(out["roofline"]["frac"], 4), "parity_ok": (out.get("parity") or {}).get("ok")}
    for c in out.get("configs") or []:
        if "value" in c:
            key = "configs[3]_strong" if "configs[3]" in c["config"] else "configs[2]_bf16" if "configs[2]" in c["config"] else "configs[4]_fp16_network"
            s[key + "_images_per_s"] = round(c["value"], 1)
            if "roofline" in c:
                s[key + "_whole_net_tflops"] = round(c["roofline"]["whole_net_algorithmic_tflops"], 1)
            if "parity" in c:
                s[key + "_parity_ok"] = c["parity"]["ok"]
    pc5 = out.get("pipeline_config5") or {}
    if "value" in pc5:
        s["configs[4]_whole_one_call_images_per_s"] = round(pc5["value"], 1)
        s["configs[4]_whole_parity_ok"] = pc5["parity"]["ok"]
    pl = out.get("pipeline") or {}
    for k in ("device_one_call", "device_one_call_b64", "facade_device", "facade_single_image"):
        if k in pl and "images_per_s" in pl[k]:
            s["pipeline_" + k + "_images_per_s"] = round(pl[k]["images_per_s"], 1)
    if "parity" in pl:
        s["pipeline_parity_ok"] = pl["parity"]["ok"]
    if out.get("cpu_baseline"):
        s["cpu_baseline_images_per_s"] = round(out["cpu_baseline"]["value"], 3)
    return s


DUMP_LIMIT_BYTES = 64 << 20


def write_outputs(d, labels):
    """--dump-outputs DIR: the label maps [N, H, W] a caller of the timed path receives from its last step, as DIR/labels.npy in
    float32.  Past DUMP_LIMIT_BYTES a fixed, seeded sample of whole images is kept (their indices, ascending, in
    DIR/labels_index.npy); if not even one image fits, a seeded sample of pixels of the flattened maps."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    labels = np.asarray(labels)
    n, per = labels.shape[0], labels[0].size * 4
    budget = DUMP_LIMIT_BYTES - 4096 - 8 * max(n, 1)              # npy headers and the index array
    index = None
    if labels.size * 4 > budget:
        rng = np.random.default_rng(0x5EED)
        if per <= budget:
            index = np.sort(rng.choice(n, budget // per, replace=False))
            labels = labels[index]
        else:
            flat = labels.reshape(-1)
            index = np.sort(rng.choice(flat.size, (DUMP_LIMIT_BYTES - 4096) // 12, replace=False))   # 4 + 8 bytes a pixel
            labels = flat[index]
    np.save(os.path.join(d, "labels.npy"), labels.astype(np.float32))
    ip = os.path.join(d, "labels_index.npy")
    if index is not None:
        np.save(ip, index.astype(np.float64))
    elif os.path.exists(ip):
        os.remove(ip)                                                # left by an earlier, sampled dump
    return {"labels": list(labels.shape), "sampled": index is not None}


def group_child_main():
    """`bench.py --group-child`: the C++ host's own multi-GPU path (mi_unet_group_*: ONE process, one worker thread per device,
    weights packed once and sent device-to-device, contiguous image shards -- the slot of the reference's sequential file
    loop, src/main.cpp:148-164) timed on BASELINE configs[3]'s batch of 512 over every visible device, both gather modes.
    Runs as a child that the parent started BEFORE it touched the GPU and that waits on stdin until the parent's own timed
    regions are over; its one JSON line goes back on stdout.  A hang in a transport that has never met a second GPU costs
    this record (the parent kills the child by PID after a deadline), never the headline."""
    line = sys.stdin.readline()
    if not line.startswith("go"):
        return 0
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from miunet import binding, synth
    from miunet.spec import UNetSpec, pack_weights
    spec = UNetSpec()
    rec = {"what": "mi_unet_group_infer_u8, one process, host buffers in / out (PCIe-inclusive)", "global_batch": 512}
    try:
        ndev = binding.device_count()
        blob = pack_weights(spec, synth.make_weights(spec, 1234))
        imgs = synth.make_images(512, 512, 512, 1, 0x5EED, "bytes")
        plans = [("all_visible_devices", None, ndev)]
        if ndev == 1:
            plans.append(("two_ranks_sharing_device_0 (rehearsal of the shard logic on one card)", [0, 0], 2))
        rec["visible_devices"] = ndev
        rec["runs"] = []
        ref = None
        for name, devs, n in plans:
            with binding.Group(512, 512, max_batch=16, devices=devs, n_devices=0 if devs is None else len(devs)) as g:
                g.load_weights(blob)
                run = {"group": name, "ranks": g.size, "weight_transport": g.weight_transport}
                for mode in ("host", "xgmi"):
                    try:
                        g.set_gather(mode)
                    except binding.MiUnetError as e:
                        run[mode + "_gather"] = {"skipped": str(e)}
                        continue
                    g.infer(imgs[:32 * g.size])                               # warm-up: buffers, graphs
                    t0 = time.perf_counter()
                    labels, _ = g.infer(imgs)
                    labels, _ = g.infer(imgs)
                    dt = (time.perf_counter() - t0) / 2
                    if ref is None:
                        ref = labels.copy()
                    run[mode + "_gather"] = {"images_per_s": 512 / dt, "ms_per_step": dt * 1e3, "labels_equal_first_run": bool(np.array_equal(labels, ref))}
                rec["runs"].append(run)
        rec["measured_on_more_than_one_device"] = bool(ndev > 1)
    except Exception as e:
        rec["error"] = repr(e)
    sys.stdout.write(json.dumps(rec) + "\n")
    sys.stdout.flush()
    return 0


def under_profiler():
    """rocprofv3 preloads its tool library, which initialises the GPU before Python starts: a fork + exec from here on is an exec
    from a GPU process (it takes the machine down on this pool)"""
    env = os.environ
    return bool(env.get("ROCP_TOOL_LIBRARIES") or env.get("ROCPROFILER_REGISTER_FORCE_LOAD") or any(k.startswith("ROCPROF") for k in env)
                or "rocprof" in env.get("LD_PRELOAD", "") or "rocprofiler" in env.get("HSA_TOOLS_LIB", ""))


def start_group_child():
    """started before this process initialises the GPU (a later fork + exec would be an exec from a GPU process); idles on stdin"""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "BENCH_FORCE_DIST", "TORCHELASTIC_RUN_ID", "GROUP_RANK",
              "LOCAL_WORLD_SIZE", "ROLE_RANK", "ROLE_WORLD_SIZE"):
        env.pop(k, None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--group-child"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                            stderr=sys.stderr, env=env, text=True)


def finish_group_child(child, run, deadline_s=240):
    """tell the idle child to run (or to leave), read its one line with a deadline, kill exactly that PID if it overruns"""
    if child is None:
        return None
    try:
        out, _ = child.communicate(input="go\n" if run else "no\n", timeout=deadline_s if run else 30)
        if not run:
            return None
        lines = [l for l in out.splitlines() if l.startswith("{")]
        return json.loads(lines[-1]) if lines else {"error": f"group child exited {child.returncode} without a record"}
    except subprocess.TimeoutExpired:
        child.kill()
        child.wait()
        return {"error": f"group child exceeded {deadline_s} s and was killed (a transport that never met a second GPU may hang)"}


def spawn_torchrun(args):
    """--gpus N > 1 without a torchrun environment: run the documented launch line as a child process (this process has
    not touched the GPU yet, and never replaces itself) and hand back its exit code."""
    port = os.environ.get("BENCH_MASTER_PORT", "29533")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16, help="images per GPU per step")
    ap.add_argument("--global-batch", type=int, default=0, help="strong scaling (BASELINE configs[3]: 512): this many images per "
                    "step over ALL ranks, contiguous shards of miunet.shard.shard_range; overrides --batch")
    ap.add_argument("--micro-batch", type=int, default=16, help="engine max_batch: images per launch (a batch larger than this runs in "
                    "micro-batches)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--in-ch", type=int, default=1)
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--full", action="store_true", help="also run every record and check besides the headline: parity gate, label-map "
                    "checks, roofline pass, e2e_host, configs, pipeline, group, cpu_baseline (off: set-up, warm-up, timed steps, line)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the label maps of the last timed step to DIR/labels.npy (float32, "
                    "at most 64 MB: a fixed, seeded sample of images beyond that, indices in DIR/labels_index.npy)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the cpu_baseline record")
    ap.add_argument("--no-extras", action="store_true", help="(--full) skip the e2e_host / configs / pipeline records")
    ap.add_argument("--per-layer", action="store_true", help="(--full) also print a per-layer table to stderr")
    ap.add_argument("--conv-algo", choices=["auto", "direct", "winograd", "winograd16", "bf16", "fp16"], default="auto")
    ap.add_argument("--no-group", action="store_true", help="skip the `group` record (mi_unet_group_* in one process)")
    ap.add_argument("--group-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--verbose", action="store_true", help="keep the per-kernel-family arrays of every roofline record in the JSON line "
                    "(default: compact form in the line, full arrays in gpurun_out/bench_families.json)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.per_layer and not args.full:
        ap.error("--per-layer needs --full (the per-kernel pass runs only there)")
    global VERBOSE
    VERBOSE = args.verbose

    if args.group_child:
        raise SystemExit(group_child_main())
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_torchrun(args))
    # the `group` record's process: started now, while this process has not touched the GPU; it idles until told to run
    default_workload = (args.in_ch, args.base, args.levels, args.size, args.conv_algo, args.global_batch) == (1, 64, 4, 512, "auto", 0)
    want_group = (int(os.environ.get("RANK", "0")) == 0 and args.full and not args.no_group and not args.no_extras and default_workload)
    group_skipped = None
    if want_group and under_profiler():
        want_group, group_skipped = False, "a profiler's preloaded library has initialised the GPU: no child process is started from here"
    group_child = start_group_child() if want_group else None

    # stdout carries exactly ONE line, the JSON record: everything libraries print while the bench runs (RCCL's version
    # banner at the first collective, the facade's per-image lines) goes to stderr instead
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import numpy as np
    import torch

    from miunet import binding, shard, synth
    from miunet.spec import UNetSpec, pack_weights

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    # BENCH_FORCE_DIST=1 runs the RCCL code path (init, weight broadcast, label gather, barrier) even with one rank, so it
    # can be rehearsed on a 1-GPU box
    use_dist = world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    spec = UNetSpec(args.in_ch, args.base, args.levels, 3)
    H = W = args.size
    B = args.batch
    if args.global_batch:
        if args.global_batch % world:
            raise SystemExit("--global-batch must be a multiple of the number of ranks (dist.gather wants equal shards)")
        lo, hi = shard.shard_range(args.global_batch, rank, world)
        B = hi - lo
    lp_mode = args.conv_algo if args.conv_algo in ("bf16", "fp16") else "fp32"

    # ---- weights: rank 0 generates, everybody else receives them over RCCL
    blob = pack_weights(spec, synth.make_weights(spec, 1234)) if rank == 0 else None
    if use_dist:
        blob = shard.broadcast_blob(blob, spec.n_params() * 4 + 36, dev)

    eng = binding.Engine(H, W, spec.in_ch, spec.base, spec.levels, spec.classes, max_batch=min(B, args.micro_batch), device=local_rank,
                         conv_algo=args.conv_algo)
    eng.load_weights(blob)

    # ---- this rank's shard of the synthetic batch.  Two image sets alternate step by step so that a label gather that ran
    # ahead of (or behind) its forward pass cannot go unnoticed: stale label maps differ from the expected ones.
    sets_host = [synth.make_images(B, H, W, spec.in_ch, 0x5EED + 1000 * rank + 500 * j, "bytes") for j in range(2)]

    # ---- 1. parity gate on the timed batch (rank 0: the oracle is a CPU program)
    parity, oracle_s = (None, 1.0)
    if rank == 0 and args.full:
        parity, oracle_s = parity_gate(eng, blob, sets_host[0], 1 if (world > 1 or args.no_cpu_baseline) else min(B, 2), lp_mode)

    # Everything below runs on ONE explicit, non-default stream shared by the engine, the copies and the collectives: the
    # gather is then ordered behind the forward pass that produced its input (torch's legacy default stream is handle 0,
    # which mi_unet_set_stream would take for "use the engine's own stream" -- an unordered pair).
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        sets = [torch.from_numpy(s).to(dev) for s in sets_host]
        labels = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        gathered = [torch.empty_like(labels) for _ in range(world)] if (use_dist and rank == 0) else None

        def step(i):
            eng.infer_device(sets[i & 1].data_ptr(), B, labels.data_ptr(), 0)
            if use_dist:
                dist.gather(labels, gathered, dst=0)

        def fence():
            if use_dist:
                dist.barrier()
            torch.cuda.synchronize(dev)

        # the first, eager, pass of each graph key (--full: also the expected label maps of both sets)
        expect = []
        for j in range(2):
            eng.infer_device(sets[j].data_ptr(), B, labels.data_ptr(), 0)
            stream.synchronize()
            if args.full:
                expect.append(labels.clone())

        # ---- 2. the shipped path: hipGraph replay, profiling off
        for i in range(args.warmup):
            step(i)
        fence()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        fence()
        dt = time.perf_counter() - t0
        # what a caller of the timed path receives from its last step (rank 0: the maps of every rank, gathered)
        outputs = (torch.cat(gathered) if use_dist else labels).cpu().numpy() if (args.dump_outputs and rank == 0) else None
        last = (args.steps - 1) & 1
        if args.full:
            if not torch.equal(labels, expect[last]) and os.environ.get("BENCH_TIMING_ONLY") != "1":    # (timing-only kernel experiments, tools/dev)
                raise SystemExit("label maps of the last timed step differ from that image set's expected maps")
            if use_dist:
                sums = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
                dist.all_gather(sums, expect[last].to(torch.int64).sum().reshape(1))
                if rank == 0:
                    for r in range(world):
                        if int(gathered[r].to(torch.int64).sum()) != int(sums[r]):
                            raise SystemExit(f"gathered label maps of rank {r} are stale or corrupt")
                    if not torch.equal(gathered[0], expect[last]):
                        raise SystemExit("gathered label maps differ from rank 0's own")

        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        if use_dist:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())

        # ---- 3. per-kernel pass: K more steps, eager, an event pair around every launch on the launch stream
        stats = []
        if args.full:
            eng.set_profiling(True)
            for i in range(args.steps):
                eng.infer_device(sets[i & 1].data_ptr(), B, labels.data_ptr(), 0)
            stats = eng.kernel_stats()
            eng.set_profiling(False)
            stream.synchronize()

        # ---- 3b. BASELINE configs[3] in the same launch: a GLOBAL batch of 512 cut into contiguous shards (strong scaling),
        # each rank walking its shard in micro-batches, the label maps gathered to rank 0 inside the timed region
        cfg4 = None
        if args.full and use_dist and default_workload and 512 % world == 0:
            lo4, hi4 = shard.shard_range(512, rank, world)
            B4 = hi4 - lo4
            imgs4 = torch.from_numpy(synth.make_images(512, H, W, spec.in_ch, 0xC0F4, "bytes")[lo4:hi4]).to(dev)
            labels4 = torch.empty((B4, H, W), dtype=torch.uint8, device=dev)
            gathered4 = [torch.empty_like(labels4) for _ in range(world)] if rank == 0 else None

            def step4():
                eng.infer_device(imgs4.data_ptr(), B4, labels4.data_ptr(), 0)
                dist.gather(labels4, gathered4, dst=0)

            step4(); step4()                                       # every micro-batch key: eager once, captured once
            fence()
            t4 = time.perf_counter()
            steps4 = 3
            for _ in range(steps4):
                step4()
            fence()
            d4 = torch.tensor([time.perf_counter() - t4], dtype=torch.float64, device=dev)
            dist.all_reduce(d4, op=dist.ReduceOp.MAX)
            sums4 = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
            dist.all_gather(sums4, labels4.to(torch.int64).sum().reshape(1))
            ok4 = True
            if rank == 0:
                ok4 = all(int(gathered4[r].to(torch.int64).sum()) == int(sums4[r]) for r in range(world))
                # the shard's first micro-batch against the SAME images run on their own (a different graph key, batch 16)
                probe = torch.empty((min(16, B4), H, W), dtype=torch.uint8, device=dev)
                eng.infer_device(imgs4.data_ptr(), probe.shape[0], probe.data_ptr(), 0)
                stream.synchronize()
                ok4 = ok4 and bool(torch.equal(probe, gathered4[0][: probe.shape[0]]))
                cfg4 = {"config": "BASELINE.json configs[3]: global batch 512 x 512x512x1 fp32, contiguous shards of 512 / N images "
                                  "per rank in micro-batches of 16, RCCL label-map gather to rank 0 inside the timed region",
                        "scaling": "strong", "n_gpus": world, "value": 512 * steps4 / float(d4.item()), "unit": "images/s",
                        "ms_per_step": float(d4.item()) / steps4 * 1e3, "steps": steps4, "warmup": 2, "images_per_rank": B4,
                        "micro_batch": min(B4, args.micro_batch), "global_batch": 512,
                        "gather": "torch.distributed.gather over RCCL (grouped ncclSend / ncclRecv into rank 0), on the engine's stream, "
                                  "inside the timed region; weights: one RCCL broadcast from rank 0 at start-up",
                        "gathered_label_maps_verified": bool(ok4),
                        "measured_on_more_than_one_device": bool(world > 1),
                        "reference_slot": "the sequential file loop of directory mode, src/main.cpp:148-164"}
            del imgs4, labels4, gathered4

    if rank == 0:
        images = B * world * args.steps
        ips = images / dt
        is_cfg1 = (spec.in_ch, spec.base, spec.levels, H) == (1, 64, 4, 512)
        is_cfg5 = (spec.in_ch, spec.base, spec.levels, H) == (3, 32, 5, 1024)
        lp = lp_mode != "fp32"
        arith = (lp_mode + " operands / fp32 accumulate") if lp else "fp32"
        cfg_idx = (2 if lp else 3 if args.global_batch else 1) if is_cfg1 else 4
        out = {
            "metric": f"images/sec, {H}x{W} UNet {arith} inference (u8 tile -> u8 label map)",
            "value": ips, "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "ms_per_image": dt / images * 1e3 * world,
            "higher_is_better": True, "scaling": "strong" if args.global_batch else "weak", "vs_baseline": None, "dtype": lp_mode, "data": "synthetic",
            "launch_mode": "hipGraph replay (the shipped path; profiling off)",
            "config": {"workload": (f"BASELINE.json configs[{cfg_idx}]: " if (is_cfg1 or is_cfg5) else "") +
                                   f"batch {B} x {H}x{W}x{spec.in_ch} u8 per GPU, {spec.levels}-level UNet base {spec.base}, "
                                   f"{arith}, argmax label maps", "images_per_gpu_per_step": B, "global_batch": B * world,
                       "parallelism": f"dp{world}" + (" (RCCL weight broadcast + per-step label-map gather)" if use_dist else "")},
        }
        if args.full:
            out["parity"] = parity
            out["roofline"] = roofline_from_stats(stats, spec.macs_per_image(H, W), ips / world, lp_mode)
            prof_ms = sum(s["ms"] for s in stats) / args.steps
            out["roofline"]["kernel_ms_per_step_eager_profiled"] = prof_ms
        if cfg4 is not None:
            out["configs"] = [cfg4]
        if args.per_layer:
            per_layer_table(stats, args.steps, dt / args.steps * 1e3)
    if use_dist:
        # the process group ends HERE: ranks > 0 leave (their GPUs are free for the one-process group record below), rank 0
        # goes on alone with the records that need no collective
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        eng.close()
        sys.exit(0)

    if not args.full:
        # a plain run ends here: the headline, the outputs if asked for, the line
        eng.close()
        if args.dump_outputs:
            print("dump-outputs: " + json.dumps(write_outputs(args.dump_outputs, outputs)), file=sys.stderr)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
        sys.exit(0)

    if rank == 0:
        extras = world == 1 and not args.no_extras and not use_dist
        if extras:
            # ---- 4. the same batch from HOST buffers: pinned staging, H2D, forward, D2H inside the call
            eng.set_stream(0, reset=True)
            for _ in range(2):
                eng.infer(sets_host[0])
            t0 = time.perf_counter()
            n_e2e = max(3, args.steps // 2)
            for i in range(n_e2e):
                lab_h, _ = eng.infer(sets_host[i & 1])
            dte = time.perf_counter() - t0
            out["e2e_host"] = {"value": B * n_e2e / dte, "unit": "images/s", "ms_per_image": dte / (B * n_e2e) * 1e3,
                               "steps": n_e2e, "what": "mi_unet_infer_u8: u8 tiles in pageable host memory -> pinned staging -> "
                               "H2D -> forward -> D2H -> u8 label maps in host memory (PCIe-inclusive; never `value`)"}
        eng.close()
        if extras:
            stream2 = torch.cuda.Stream(dev)
            try:
                out["configs"] = out.get("configs", []) + [
                    run_config(binding, synth, torch, dev, stream2, "BASELINE.json configs[2]: batch 128 x 512x512x1, bf16 operands / "
                               "fp32 accumulate, micro-batches of 16", UNetSpec(1, 64, 4, 3), 512, 128, 16, "bf16", 5, 2, "bf16"),
                    run_config(binding, synth, torch, dev, stream2, "BASELINE.json configs[4] (network half): batch 8 x 1024x1024x3, "
                               "5-level base 32, fp16 operands / fp32 accumulate", UNetSpec(3, 32, 5, 3), 1024, 8, 8, "fp16", 20, 5, "fp16"),
                ]
            except Exception as e:                                            # an extra record never costs the headline
                out["configs"] = out.get("configs", []) + [{"error": repr(e)}]
            try:
                out["pipeline"] = run_pipeline(binding, synth, local_rank)
            except Exception as e:
                out["pipeline"] = {"error": repr(e)}
            try:
                out["pipeline_config5"] = run_pipeline_config5(binding, synth, local_rank)
            except Exception as e:
                out["pipeline_config5"] = {"error": repr(e)}
        if group_skipped:
            out["group"] = {"skipped": group_skipped}
        if group_child is not None:
            # ---- 6b. the C++ host's own multi-GPU path, one process over every visible device (a child process; see group_child_main)
            try:
                out["group"] = finish_group_child(group_child, run=True)
            except Exception as e:                                            # an extra record never costs the headline
                out["group"] = {"error": repr(e)}
        if not args.no_cpu_baseline:
            # N > 1: rank 0 alone, after the process group has ended and the other ranks have left the host's cores
            out["cpu_baseline"] = cpu_baseline(blob, H, W, spec.in_ch, oracle_s)
        else:
            out["cpu_baseline"] = None
        out["summary"] = summary_of(out)
        try:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            json.dump(FAMILY_TABLES, open(os.path.join(ROOT, "gpurun_out", "bench_families.json"), "w"), indent=1)
        except OSError:
            pass
        if args.dump_outputs:
            print("dump-outputs: " + json.dumps(write_outputs(args.dump_outputs, outputs)), file=sys.stderr)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
        bad = [k for k in ("parity",) if out.get(k) and not out[k]["ok"]]
        if extras and isinstance(out.get("configs"), list):           # recorded; only the headline and the exact pipeline gate the exit code
            for c in out["configs"]:
                if "parity" in c and not c["parity"]["ok"]:
                    print("parity of an extra config outside its tolerance: " + c["config"], file=sys.stderr)
        if extras and isinstance(out.get("pipeline"), dict) and "parity" in out["pipeline"] and not out["pipeline"]["parity"]["ok"]:
            bad.append("pipeline")
        if extras and isinstance(out.get("pipeline_config5"), dict) and "parity" in out["pipeline_config5"] and not out["pipeline_config5"]["parity"]["ok"]:
            bad.append("pipeline_config5")
        if bad:
            print("PARITY FAILURE: " + ", ".join(bad), file=sys.stderr)
            rc = 3
        else:
            rc = 0
    sys.exit(rc)


if __name__ == "__main__":
    main()
