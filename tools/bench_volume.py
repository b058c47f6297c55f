#!/usr/bin/env python3
"""What labelling a stack of masks as one volume costs (mi_unet_volume_components), on one GPU.  Not the headline metric
(bench.py).

Three cases, in a child process of its own: a 64 x 512 x 512 stack with one value under connectivity 26 -- a few smooth blobs, what a
segmented organ looks like -- and a 16 x 512 x 512 stack with three values of dense smooth noise (thousands of components a value)
under connectivity 6 and under 26.  --rounds rounds of --calls calls after --warmup warm-up calls; the wall time of the whole call
(host buffers in; out, table, found and kept out) as median and spread (max - min) / median over all calls.  Beside each case the same
planes through scipy.ndimage.label + numpy.bincount + scipy.ndimage.find_objects on this host's CPU -- what a user would otherwise
run -- timed --scipy-calls times when scipy imports (null otherwise), and the check that both give the same number of components
and the same largest size.

Writes one JSON document (--out, default profiles/volume_cases.json) and prints the table of DESIGN.md 7.9."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
CASES = (("blobs_64x512x512_c26", "blobs", (64, 512, 512), (1,), 26), ("noise_16x512x512_c6", "noise", (16, 512, 512), (1, 2, 3), 6),
         ("noise_16x512x512_c26", "noise", (16, 512, 512), (1, 2, 3), 26))


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def make_volume(kind, shape, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind == "noise":         # uniform noise averaged twice over the 6 neighbours, cut into classes 0 .. 3, 4 % reset to 0 (tests/volume_ref.py)
        f = rng.random(shape)
        for _ in range(2):
            f = (f + sum(np.roll(f, sh, ax) for ax in range(3) for sh in (-1, 1))) / 7.0
        vol = np.searchsorted(np.quantile(f, (0.35, 0.55, 0.8)), f).astype(np.uint8)
        vol[rng.random(shape) < 0.04] = 0
        return vol
    d, h, w = shape             # six ellipsoids, apart from each other
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij", sparse=True)
    vol = np.zeros(shape, np.uint8)
    for cz, cy, cx, rz, ry, rx in ((20, 128, 128, 14, 90, 70), (40, 380, 140, 18, 60, 100), (30, 256, 380, 25, 150, 60), (8, 440, 440, 5, 30, 30),
                                   (56, 60, 440, 6, 40, 50), (50, 450, 300, 10, 25, 80)):
        vol[((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = 1
    return vol


def child(a):
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    import numpy as np
    from miunet import binding
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    doc = {}
    vols = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        for name, kind, shape, values, conn in CASES:
            vol = vols.setdefault((kind, shape), make_volume(kind, shape, 7))
            for _ in range(a.warmup):
                got = eng.volume_components(vol, values, conn, cap=4096)
            ms = []
            for _ in range(a.rounds):
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    got = eng.volume_components(vol, values, conn, cap=4096)
                    ms.append((time.perf_counter() - t0) * 1e3)
            _, table, found, _, _ = got
            cpu, same = [], None
            if ndi is not None:
                structure = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
                for _ in range(a.scipy_calls):
                    t0 = time.perf_counter()
                    counts, largest = [], []
                    for v in values:
                        lab, cnt = ndi.label(vol == v, structure)
                        sizes = np.bincount(lab.reshape(-1))[1:]
                        boxes = ndi.find_objects(lab)
                        counts.append(cnt); largest.append(int(sizes.max()) if cnt else 0)
                        del boxes
                    cpu.append((time.perf_counter() - t0) * 1e3)
                same = counts == found.tolist() and largest == [int(table[k]["voxels"][0]) for k in range(len(values))]
            doc[name] = {"planes": len(values), "depth": shape[0], "height": shape[1], "width": shape[2], "connectivity": conn,
                         "found": found.tolist(), "largest": [int(table[k]["voxels"][0]) for k in range(len(values))],
                         "call_ms": median(ms), "call_spread": (max(ms) - min(ms)) / median(ms),
                         "scipy_ms": median(cpu) if cpu else None, "scipy_calls": a.scipy_calls if cpu else 0, "equal_scipy": same}
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scipy-calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_cases.json"))
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
    print("| case | planes | components | mi_unet_volume_components ms (spread) | scipy on the CPU ms | same count and largest |")
    print("|---|---|---|---|---|---|")
    for name, s in doc["cases"].items():
        cpu = "not measured" if s["scipy_ms"] is None else f"{s['scipy_ms']:.0f}"
        print(f"| {name} | {s['planes']} | {s['found']} | {s['call_ms']:.3f} ({100 * s['call_spread']:.1f} %) | {cpu} | {s['equal_scipy']} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
