#!/usr/bin/env python3
"""What scoring masks against ground truth costs (mi_unet_score_labels), on one GPU.  Not the headline metric (bench.py).

Two cases, in a child process of its own: 16 planes of 512 x 512 (B = 16 label maps, one value) and 3 values on one 2048 x 1536 map.
Truth is a seeded smooth 4-class label map, the prediction the same map shifted by (3, -2) with 1 % of its pixels re-drawn.  --rounds
rounds of --calls calls after --warmup warm-up calls; the wall time of the whole call (host buffers in, scores out) as median and
spread (max - min) / median over all calls.  Beside each case the same planes through scipy on this host's CPU -- binary_erosion for
both boundaries and distance_transform_edt both ways, what a user would otherwise run -- timed --scipy-calls times, and the check
that both give the same Hausdorff distances.

Writes one JSON document (--out, default profiles/score_cases.json) and prints the table of DESIGN.md 7.8."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
CASES = (("512x512x16", 16, 512, 512, (2,)), ("2048x1536x3values", 1, 1536, 2048, (1, 2, 3)))


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def make_maps(b, h, w, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    truth = np.zeros((b, h, w), np.uint8)
    for i in range(b):
        f = rng.random((h // 16 + 2, w // 16 + 2))
        f = np.kron(f, np.ones((16, 16)))[:h, :w]
        for _ in range(6):
            f = (f + np.roll(f, 3, 0) + np.roll(f, -3, 0) + np.roll(f, 3, 1) + np.roll(f, -3, 1)) / 5
        truth[i] = np.digitize(f, np.quantile(f, [0.35, 0.55, 0.8]))
    pred = np.roll(truth, (3, -2), (1, 2)).copy()
    noise = rng.random(pred.shape) < 0.01
    pred[noise] = rng.integers(0, 4, int(noise.sum()))
    return pred, truth


def child(a):
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    import numpy as np
    from scipy import ndimage as ndi
    from miunet import binding
    doc = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        for name, b, h, w, values in CASES:
            pred, truth = make_maps(b, h, w, 7)
            for _ in range(a.warmup):
                got = eng.score_labels(pred, truth, values)
            ms = []
            for _ in range(a.rounds):
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    got = eng.score_labels(pred, truth, values)
                    ms.append((time.perf_counter() - t0) * 1e3)
            cpu, hd = [], None
            for _ in range(a.scipy_calls):
                t0 = time.perf_counter()
                hd = []
                for i in range(b):
                    for v in values:
                        sa, st = pred[i] == v, truth[i] == v
                        sa, st = sa & ~ndi.binary_erosion(sa), st & ~ndi.binary_erosion(st)
                        da, dt = ndi.distance_transform_edt(~st)[sa], ndi.distance_transform_edt(~sa)[st]
                        hd.append(max(da.max(), dt.max()))
                cpu.append((time.perf_counter() - t0) * 1e3)
            same = all(abs(binding.score_derive(got[i, k])["hd"] - hd[i * len(values) + k]) < 1e-9 for i in range(b) for k in range(len(values)))
            doc[name] = {"planes": b * len(values), "height": h, "width": w, "boundary_pixels": int(got["a_to_t"]["n"].sum() + got["t_to_a"]["n"].sum()),
                         "call_ms": median(ms), "call_spread": (max(ms) - min(ms)) / median(ms), "scipy_ms": median(cpu),
                         "scipy_calls": a.scipy_calls, "hd_equal_scipy": bool(same)}
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scipy-calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_cases.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup",
                        str(a.warmup), "--scipy-calls", str(a.scipy_calls)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"child failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "cases": json.loads(r.stdout.strip().splitlines()[-1])}
    print("| case | planes | boundary pixels | mi_unet_score_labels ms (spread) | scipy on the CPU ms | same HD |")
    print("|---|---|---|---|---|---|")
    for name, s in doc["cases"].items():
        print(f"| {name} | {s['planes']} | {s['boundary_pixels']} | {s['call_ms']:.3f} ({100 * s['call_spread']:.1f} %) | {s['scipy_ms']:.0f} | {s['hd_equal_scipy']} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
