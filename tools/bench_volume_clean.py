#!/usr/bin/env python3
"""What cleaning a stack of masks as one volume costs (mi_unet_volume_clean), on one GPU.  Not the headline metric
(bench.py).

Four cases, in a child process of its own.  A 64 x 512 x 512 stack with one value -- a few smooth blobs, two of them hollow, with 1 %
salt-and-pepper -- under the units (7, 7, 50) of 0.7 x 0.7 x 5 mm at 0.1 mm: the fill alone, then fill + close + open by a ball of
2 mm, then of 4 mm (the design claims the cost follows the ball's half-widths, about 2 x, not its volume, about 8 x: the ratio is
reported).  And a 16 x 512 x 512 stack with three values of dense smooth noise under isotropic units with radius 3.  --rounds rounds of
--calls calls after --warmup warm-up calls; the wall time of the whole call (host buffers in; out and stats out) as median and spread
(max - min) / median over all calls.  Beside each case mi_unet_volume_clean_host on this host's CPU, timed --host-calls times, and the
check that both give the same bytes and counts.

Writes one JSON document (--out, default profiles/volume_clean_cases.json) and prints the table of DESIGN.md 7.11."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
# (name, kind, shape, values, units, fill, close_r, open_r)
CASES = (("blobs_64x512x512_fill", "blobs", (64, 512, 512), (1,), (7, 7, 50), True, 0, 0),
         ("blobs_64x512x512_2mm", "blobs", (64, 512, 512), (1,), (7, 7, 50), True, 20, 20),
         ("blobs_64x512x512_4mm", "blobs", (64, 512, 512), (1,), (7, 7, 50), True, 40, 40),
         ("noise_16x512x512_r3", "noise", (16, 512, 512), (1, 2, 3), (1, 1, 1), True, 3, 3))


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def make_volume(kind, shape, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind == "noise":         # uniform noise averaged twice over the 6 neighbours, cut into classes 0 .. 3, 4 % reset to 0 (tools/bench_volume.py)
        f = rng.random(shape)
        for _ in range(2):
            f = (f + sum(np.roll(f, sh, ax) for ax in range(3) for sh in (-1, 1))) / 7.0
        vol = np.searchsorted(np.quantile(f, (0.35, 0.55, 0.8)), f).astype(np.uint8)
        vol[rng.random(shape) < 0.04] = 0
        return vol
    d, h, w = shape             # six ellipsoids, apart from each other (tools/bench_volume.py), the first two hollow, then 1 % of the voxels flipped
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij", sparse=True)
    vol = np.zeros(shape, np.uint8)
    for i, (cz, cy, cx, rz, ry, rx) in enumerate(((20, 128, 128, 14, 90, 70), (40, 380, 140, 18, 60, 100), (30, 256, 380, 25, 150, 60),
                                                  (8, 440, 440, 5, 30, 30), (56, 60, 440, 6, 40, 50), (50, 450, 300, 10, 25, 80))):
        q = ((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2
        vol[(q <= 1.0) & ((q >= 0.3) if i < 2 else True)] = 1
    vol ^= (rng.random(shape) < 0.01).astype(np.uint8)
    return vol


def child(a):
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    from miunet import binding
    doc = {}
    vols = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        for name, kind, shape, values, units, fill, close_r, open_r in CASES:
            vol = vols.setdefault((kind, shape), make_volume(kind, shape, 7))
            for _ in range(a.warmup):
                out, stats = eng.volume_clean(vol, values, units, fill, close_r, open_r)
            ms = []
            for _ in range(a.rounds):
                for _ in range(a.calls):
                    t0 = time.perf_counter()
                    out, stats = eng.volume_clean(vol, values, units, fill, close_r, open_r)
                    ms.append((time.perf_counter() - t0) * 1e3)
            cpu, same = [], None
            for _ in range(a.host_calls):
                t0 = time.perf_counter()
                h_out, h_stats = binding.volume_clean_host(vol, values, units, fill, close_r, open_r)
                cpu.append((time.perf_counter() - t0) * 1e3)
                same = out.tobytes() == h_out.tobytes() and stats.tobytes() == h_stats.tobytes()
            ext, _ = binding.volume_ball(units, max(close_r, open_r))
            doc[name] = {"planes": len(values), "depth": shape[0], "height": shape[1], "width": shape[2], "units": list(units), "fill": fill,
                         "close_r": close_r, "open_r": open_r, "half_widths": list(ext),
                         "stats": [{f: int(s[f]) for f in ("in_voxels", "filled", "closed", "opened", "out_voxels")} for s in stats],
                         "call_ms": median(ms), "call_spread": (max(ms) - min(ms)) / median(ms),
                         "host_ms": median(cpu) if cpu else None, "host_calls": a.host_calls, "equal_host": same}
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_clean_cases.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup",
                        str(a.warmup), "--host-calls", str(a.host_calls)], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"child failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "cases": json.loads(r.stdout.strip().splitlines()[-1])}
    c = doc["cases"]
    doc["ratio_4mm_to_2mm"] = c["blobs_64x512x512_4mm"]["call_ms"] / c["blobs_64x512x512_2mm"]["call_ms"]
    print("| case | planes | half-widths x, y, z | filled / closed / opened | mi_unet_volume_clean ms (spread) | _host on the CPU ms | same bytes |")
    print("|---|---|---|---|---|---|---|")
    for name, s in c.items():
        cpu = "not measured" if s["host_ms"] is None else f"{s['host_ms']:.0f}"
        counts = "; ".join(f"{t['filled']} / {t['closed']} / {t['opened']}" for t in s["stats"])
        print(f"| {name} | {s['planes']} | {s['half_widths']} | {counts} | {s['call_ms']:.3f} ({100 * s['call_spread']:.1f} %) | {cpu} | {s['equal_host']} |")
    print(f"4 mm / 2 mm: {doc['ratio_4mm_to_2mm']:.2f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
