#!/usr/bin/env python3
"""Tile blending and mirror averaging (mi_unet_set_tile_blend) against the parent commit's tiled call, on one GPU.
Not the headline metric (bench.py).

The image and engine of tools/bench_tiled.py: default fp32 engine (512 x 512, base 64, 4 levels, max_batch 16), one 2048 x 1536
image, halo 32 = 20 tiles, labels only, host clock around the C call.  Four configurations:
  (a) the parent commit's mi_unet_infer_tiled_u8, from a separate checkout (--parent, a tree whose libmiunet.so is built), run in a
      child process of its own;
  (b) this tree, OWNER without mirror (the default);   (c) GAUSSIAN 0.125 without mirror;   (d) GAUSSIAN 0.125 with XY mirrors.
Each of --rounds rounds runs (a), (b), (c), (d) in turn, --calls calls each after the warm-up of the first round, so slow drifts
of the card reach all four alike.  Then one profiled call of (b), (c) and (d) for the kernel statistics.  Writes one JSON document
(--out, default profiles/tile_blend_2048x1536.json).

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/unet-medical-image-contour-segmentation-cpp_amd libmiunet.so
    python tools/bench_tile_blend.py --parent /tmp/parent"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"


def summary(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"n": len(a), "median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "std_ms": float(a.std())}


def setup(pkg_root, H, W):
    """the engine, weights and image of one side (its own package: this tree's, or the parent's in the child process)"""
    sys.path.insert(0, os.path.join(pkg_root, PKG_REL))
    from miunet import binding, synth
    from miunet.spec import UNetSpec, pack_weights
    spec = UNetSpec()
    eng = binding.Engine()
    eng.load_weights(pack_weights(spec, synth.make_weights(spec, 1234)))
    return binding, eng, synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]


def timed_calls(binding, eng, img, H, W, halo, n):
    import numpy as np
    L = binding.lib()
    labels = np.empty((H, W), np.uint8)
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        binding._check(L.mi_unet_infer_tiled_u8(eng._h, binding._ptr(img), H, W, halo, binding._ptr(labels), None))
        out.append((time.perf_counter() - t0) * 1e3)
    return out, labels


def child(a):
    """(a): the parent tree's tiled call, warm-up then --calls timed calls; times and a label digest on stdout"""
    import hashlib
    binding, eng, img = setup(a.parent, a.height, a.width)
    timed_calls(binding, eng, img, a.height, a.width, a.halo, a.warmup)
    ms, labels = timed_calls(binding, eng, img, a.height, a.width, a.halo, a.calls)
    print(json.dumps({"ms": ms, "labels_sha1": hashlib.sha1(labels.tobytes()).hexdigest()}))


def kernel_table(stats):
    out = {}
    for fam in ("tile_gather", "tile_stitch", "tile_blend", "blend_finalize"):
        rows = [s for s in stats if s["kernel"] == fam]
        if rows:
            ms, nbytes = sum(s["ms"] for s in rows), sum(s["bytes"] for s in rows)
            out[fam] = {"launches": len(rows), "ms": ms, "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3) if ms > 0 else None}
    out["network_kernels_ms"] = sum(s["ms"] for s in stats if s["kernel"] not in out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checkout of the parent commit with its libmiunet.so built")
    ap.add_argument("--height", type=int, default=1536)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_blend_2048x1536.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import hashlib

    import numpy as np
    binding, eng, img = setup(ROOT, a.height, a.width)
    if binding.device_count() < 1:
        raise SystemExit("bench_tile_blend needs a HIP device")
    H, W, halo = a.height, a.width, a.halo
    configs = {"b_owner": ("owner", 0.125, ""), "c_gaussian": ("gaussian", 0.125, ""), "d_gaussian_xy": ("gaussian", 0.125, "xy")}
    times = {"a_parent": [], **{k: [] for k in configs}}
    digests = {}
    for k, cfg in configs.items():                                         # warm-up: buffers, routes, captured graphs
        eng.set_tile_blend(*cfg)
        timed_calls(binding, eng, img, H, W, halo, a.warmup)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--height", str(H), "--width", str(W),
           "--halo", str(halo), "--calls", str(a.calls), "--warmup", str(a.warmup)]
    for r in range(a.rounds):
        res = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1])
        times["a_parent"] += res["ms"]
        digests["a_parent"] = res["labels_sha1"]
        for k, cfg in configs.items():
            eng.set_tile_blend(*cfg)
            ms, labels = timed_calls(binding, eng, img, H, W, halo, a.calls)
            times[k] += ms
            digests[k] = hashlib.sha1(labels.tobytes()).hexdigest()
        print(f"round {r}: " + ", ".join(f"{k} {np.median(v[-a.calls:]):.3f} ms" for k, v in times.items()), flush=True)
    stages, kernels = {}, {}
    for k, cfg in configs.items():
        eng.set_tile_blend(*cfg)
        timed_calls(binding, eng, img, H, W, halo, 1)
        stages[k] = eng.last_stage_ms()
        eng.set_profiling(True)
        timed_calls(binding, eng, img, H, W, halo, 1)
        kernels[k] = kernel_table(eng.kernel_stats())
        eng.set_profiling(False)
    eng.close()
    s = {k: summary(v) for k, v in times.items()}
    ma, sa = s["a_parent"]["median_ms"], s["a_parent"]["std_ms"]
    doc = {
        "what": "labels-only mi_unet_infer_tiled_u8: (a) the parent commit in its own process, (b)-(d) this tree with three tile blend settings",
        "device": "one MI355X", "engine": "512 x 512, base 64, 4 levels, fp32 default plan, max_batch 16",
        "image": f"{W} x {H} (W x H), halo {halo}: 20 tiles (80 view images with xy mirrors)",
        "rounds": a.rounds, "calls_per_round": a.calls, "warmup": a.warmup,
        "timing": "host clock around the C call (each call ends in a stream synchronise); the four configurations alternate per round",
        "settings": {k: {"mode": c[0], "sigma_scale": c[1], "mirror": c[2]} for k, c in configs.items()},
        "summary": s,
        "b_minus_a_median_ms": s["b_owner"]["median_ms"] - ma,
        "b_within_2_std_of_a": bool(abs(s["b_owner"]["median_ms"] - ma) <= 2 * sa),
        "c_minus_a_median_ms": s["c_gaussian"]["median_ms"] - ma,
        "c_over_a_median": s["c_gaussian"]["median_ms"] / ma,
        "d_over_a_median": s["d_gaussian_xy"]["median_ms"] / ma,
        "b_labels_equal_a": digests["a_parent"] == digests["b_owner"],
        "stage_ms_of_one_call": stages,
        "kernels_of_one_profiled_call": kernels,
        "raw_ms": times,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "raw_ms"}))


if __name__ == "__main__":
    main()
