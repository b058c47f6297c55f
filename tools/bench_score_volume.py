#!/usr/bin/env python3
"""What scoring a stack of masks against ground truth as one volume costs (mi_unet_score_volume), on one GPU.  Not the
headline metric (bench.py).

Four cases, in a child process of its own: a 64 x 512 x 512 stack with one value -- a few smooth blobs against themselves moved by
(dz, dy, dx) = (3, -2, 1) with 1 % of the voxels re-drawn -- under the units (7, 7, 50) of 0.7 x 0.7 x 5 mm; a 16 x 512 x 512 stack with
three values of dense smooth noise against itself moved by (1, -2, 3), under (1, 1, 1) and under (7, 7, 50); and the worst case of the
outward scans, two small blobs in opposite corners of 64 x 512 x 512.  --rounds rounds of --calls calls after --warmup warm-up calls;
the wall time of the whole call (host buffers in, scores out) as median and spread (max - min) / median over all calls.  Beside each
case the same planes through scipy.ndimage.binary_erosion + distance_transform_edt(sampling=...) on this host's CPU -- what medpy
runs -- timed --scipy-calls times when scipy imports (null otherwise), and the check that both sides agree on the Hausdorff distance
to within 1e-9 relative: both are square roots of the same integer.

Writes one JSON document (--out, default profiles/score_volume_cases.json) and prints the table of DESIGN.md 7.10."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CASES = (("blobs_64x512x512_u7_7_50", "blobs", (64, 512, 512), (1,), (7, 7, 50)), ("noise_16x512x512_u1_1_1", "noise", (16, 512, 512), (1, 2, 3), (1, 1, 1)),
         ("noise_16x512x512_u7_7_50", "noise", (16, 512, 512), (1, 2, 3), (7, 7, 50)), ("far_64x512x512_u7_7_50", "far", (64, 512, 512), (1,), (7, 7, 50)))


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def moved(vol, shift):
    """vol moved by (dz, dy, dx), zeros moving in"""
    import numpy as np
    out = np.zeros_like(vol)
    dst = tuple(slice(max(s, 0), n + min(s, 0)) for n, s in zip(vol.shape, shift))
    src = tuple(slice(max(-s, 0), n + min(-s, 0)) for n, s in zip(vol.shape, shift))
    out[dst] = vol[src]
    return out


def make_pair(kind, shape, seed):
    """(pred, truth) u8 [D, H, W]"""
    import numpy as np
    from bench_volume import make_volume
    if kind == "far":
        d, h, w = shape
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij", sparse=True)
        ball = lambda cz, cy, cx: (((z - cz) / 3.0) ** 2 + ((y - cy) / 12.0) ** 2 + ((x - cx) / 12.0) ** 2 <= 1.0).astype(np.uint8)
        return ball(4, 20, 20), ball(d - 5, h - 21, w - 21)
    truth = make_volume(kind, shape, seed)
    if kind == "noise":
        return moved(truth, (1, -2, 3)), truth
    pred = moved(truth, (3, -2, 1))
    rng = np.random.default_rng(seed + 1)
    redraw = rng.random(shape) < 0.01
    pred[redraw] = rng.integers(0, 2, shape, dtype=np.uint8)[redraw]
    return pred, truth


def scipy_hd(ndi, pred, truth, values, units):
    """the largest Hausdorff distance over the values, in units, the way medpy computes it"""
    import numpy as np
    sampling = (units[2], units[1], units[0])
    hd = []
    for v in values:
        a, t = pred == v, truth == v
        ba, bt = a & ~ndi.binary_erosion(a), t & ~ndi.binary_erosion(t)
        if not ba.any() or not bt.any():
            hd.append(math.nan)
            continue
        to_t, to_a = ndi.distance_transform_edt(~bt, sampling=sampling), ndi.distance_transform_edt(~ba, sampling=sampling)
        hd.append(float(max(to_t[ba].max(), to_a[bt].max())))
    return hd


def child(a):
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    from miunet import binding
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    doc = {}
    pairs = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        for name, kind, shape, values, units in CASES:
            pred, truth = pairs.setdefault((kind, shape), make_pair(kind, shape, 7))
            for _ in range(a.warmup):
                got = eng.score_volume(pred, truth, values, units)
            ms = []
            for _ in range(a.rounds):
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    got = eng.score_volume(pred, truth, values, units)
                    ms.append((time.perf_counter() - t0) * 1e3)
            hd = [math.sqrt(max(int(s["a_to_t"]["max_d2"]), int(s["t_to_a"]["max_d2"]))) for s in got]
            cpu, ref, same = [], None, None
            if ndi is not None:
                for _ in range(a.scipy_calls):
                    t0 = time.perf_counter()
                    ref = scipy_hd(ndi, pred, truth, values, units)
                    cpu.append((time.perf_counter() - t0) * 1e3)
                same = all(abs(g - r) <= 1e-9 * r for g, r in zip(hd, ref))
            doc[name] = {"planes": len(values), "depth": shape[0], "height": shape[1], "width": shape[2], "units": list(units),
                         "boundary_voxels": [[int(s["a_to_t"]["n"]), int(s["t_to_a"]["n"])] for s in got], "hd_units": hd, "scipy_hd_units": ref,
                         "call_ms": median(ms), "call_spread": (max(ms) - min(ms)) / median(ms),
                         "scipy_ms": median(cpu) if cpu else None, "scipy_calls": a.scipy_calls if cpu else 0, "hd_equal_scipy": same}
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scipy-calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_volume_cases.json"))
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
    print("| case | planes | boundary voxels (pred, truth) | mi_unet_score_volume ms (spread) | scipy on the CPU ms | same Hausdorff distance |")
    print("|---|---|---|---|---|---|")
    for name, s in doc["cases"].items():
        cpu = "not measured" if s["scipy_ms"] is None else f"{s['scipy_ms']:.0f}"
        print(f"| {name} | {s['planes']} | {s['boundary_voxels']} | {s['call_ms']:.3f} ({100 * s['call_spread']:.1f} %) | {cpu} | {s['hd_equal_scipy']} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
