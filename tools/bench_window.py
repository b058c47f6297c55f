#!/usr/bin/env python3
"""What an intensity window costs in front of the network (mi_unet_set_window), on one GPU.  Not the headline metric
(bench.py).

The default engine (512 x 512, base 64, 4 levels, 3 classes, max_batch 16) on
  raw   : 16 RAW images of 2048 x 1536 through mi_unet_segment_raw16 (resampled to the tile), and
  tiled : one 4096 x 4096 image through mi_unet_infer_tiled_raw16 (halo 32, native resolution),
each under MINMAX (the default), PERCENTILE (5000 / 5000 ppm) and FIXED (the image's own 0.5 % / 99.5 % values): the device time of
MI_UNET_STAGE_UPLOAD_PRE (mi_unet_last_stage_ms: staging copy + H2D + min/max or selection + resample / normalise) and the wall time
of the whole call.  Every side runs in a child process of its own, --calls calls after a warm-up; medians and the spread
(max - min) / median are reported.  With --parent (a checkout of the parent commit whose libmiunet.so is built) the parent's
default path runs before AND after this tree's, so that a drift of the card shows as the distance of the two parent runs:

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/unet-medical-image-contour-segmentation-cpp_amd libmiunet.so
    python tools/bench_window.py --parent /tmp/parent

Writes one JSON document (--out, default profiles/window_2048x1536x16.json) and prints the table of DESIGN.md 7.5."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
CLIP = (5000, 5000)


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def summary(rows):
    """rows of (upload_pre ms, network ms, wall ms) -> medians and relative spreads"""
    out = {}
    for k, name in enumerate(("upload_pre_ms", "network_ms", "call_ms")):
        v = [r[k] for r in rows]
        out[name] = median(v)
        out[name.replace("_ms", "_spread")] = (max(v) - min(v)) / median(v)
    return out


def child(a):
    """one process: the library of `a.tree`, every mode it knows, both workloads"""
    sys.path.insert(0, os.path.join(a.tree, PKG_REL))
    import numpy as np
    from miunet import binding, synth
    from miunet.spec import UNetSpec, pack_weights
    spec = UNetSpec()
    eng = binding.Engine(max_batch=a.batch)
    eng.load_weights(pack_weights(spec, synth.make_threshold_weights(spec)))
    raws = [synth.make_raw16(1536, 2048, seed=21 + i) for i in range(a.batch)]
    big = np.tile(synth.make_raw16(1024, 1024, seed=5), (a.tiled_size // 1024, a.tiled_size // 1024))
    modes = ["minmax"] + (["percentile", "fixed"] if hasattr(eng, "set_window") else [])
    p = eng.segment_raw16_prepare(raws, cap_points=1 << 15, cap_contours=64)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        st = eng.last_stage_ms()
        return st["upload_preprocess"], st["network"], wall

    doc = {}
    for mode in modes:
        for name, imgs, fn in (("raw", raws, lambda: eng.segment_raw16_run(p)),
                               ("tiled", [big], lambda: eng.infer_tiled_raw16(big, 32, want_norm=False))):
            if mode == "percentile":
                eng.set_window("percentile", *CLIP)
            elif mode == "fixed":
                s = np.sort(imgs[0].reshape(-1))
                eng.set_window("fixed", lo=int(s[s.size // 200]), hi=int(s[s.size - 1 - s.size // 200]))
            for _ in range(a.warmup):
                fn()
            doc[f"{name}.{mode}"] = summary([timed(fn) for _ in range(a.calls)])
    print(json.dumps(doc))


def run_child(tree, a):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--batch", str(a.batch), "--calls", str(a.calls),
                        "--warmup", str(a.warmup), "--tiled-size", str(a.tiled_size)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"child for {tree} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with libmiunet.so built")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tiled-size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_2048x1536x16.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    doc = {"batch": a.batch, "calls": a.calls, "warmup": a.warmup, "tiled_size": a.tiled_size, "clip_ppm": list(CLIP)}
    if a.parent:
        doc["parent_before"] = run_child(a.parent, a)
    doc["this_tree"] = run_child(ROOT, a)
    if a.parent:
        doc["parent_after"] = run_child(a.parent, a)
    print("| side | workload.mode | UPLOAD_PRE ms (spread) | NETWORK ms | whole call ms (spread) |")
    print("|---|---|---|---|---|")
    for side in ("parent_before", "this_tree", "parent_after"):
        for key, s in doc.get(side, {}).items():
            print(f"| {side} | {key} | {s['upload_pre_ms']:.3f} ({100 * s['upload_pre_spread']:.1f} %) | {s['network_ms']:.3f} | "
                  f"{s['call_ms']:.3f} ({100 * s['call_spread']:.1f} %) |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
