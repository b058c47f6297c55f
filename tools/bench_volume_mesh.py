#!/usr/bin/env python3
"""What meshing a stack of masks as one volume costs (mi_unet_volume_mesh), on one GPU.  Not the headline metric
(bench.py).

One stack, in a child process of its own: 64 x 512 x 512 with one value -- six smooth organ-like blobs, two of them hollow, with
0.05 % of the voxels flipped -- under both placements.  Two calls are timed per placement, as the wall time of the whole call (host
buffers in; vertices, quads and stats out): the counting call (NULL arrays), and the sized call with caps equal to the counts.
--rounds rounds of --calls calls after --warmup warm-up calls; median and spread (max - min) / median over all calls.  The bytes the
stage must move are the volume once (D H W) and the two arrays once (16 bytes per vertex and per quad); the achieved GB/s is that over
the sized call's time.  Beside it mi_unet_volume_mesh_host on this host's CPU, timed --host-calls times, and the check that both give
the same bytes and counts.

Writes one JSON document (--out, default profiles/volume_mesh_cases.json) and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
SHAPE = (64, 512, 512)


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def make_volume(shape, seed):
    """six ellipsoids, apart from each other (tools/bench_volume_clean.py), the first two hollow, then 0.05 % of the voxels flipped"""
    import numpy as np
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij", sparse=True)
    vol = np.zeros(shape, np.uint8)
    for i, (cz, cy, cx, rz, ry, rx) in enumerate(((20, 128, 128, 14, 90, 70), (40, 380, 140, 18, 60, 100), (30, 256, 380, 25, 150, 60),
                                                  (8, 440, 440, 5, 30, 30), (56, 60, 440, 6, 40, 50), (50, 450, 300, 10, 25, 80))):
        q = ((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2
        vol[(q <= 1.0) & ((q >= 0.3) if i < 2 else True)] = 1
    vol ^= (rng.random(shape) < 0.0005).astype(np.uint8)
    return vol


def child(a):
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    from miunet import binding
    vol = make_volume(SHAPE, 7)
    doc = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        for placement in ("faces", "nets"):
            _, _, stats = eng.volume_mesh(vol, (1,), placement, cap=0, raw=True)
            caps = (int(stats[0]["verts"]), int(stats[0]["quads"]))
            times = {}
            for what, cap in (("count", 0), ("sized", caps)):
                for _ in range(a.warmup):
                    got = eng.volume_mesh(vol, (1,), placement, cap=cap, raw=True)
                ms = []
                for _ in range(a.rounds):
                    for _ in range(a.calls):
                        t0 = time.perf_counter()
                        got = eng.volume_mesh(vol, (1,), placement, cap=cap, raw=True)
                        ms.append((time.perf_counter() - t0) * 1e3)
                times[what] = ms
            cpu, same = [], None
            for _ in range(a.host_calls):
                t0 = time.perf_counter()
                host = binding.volume_mesh_host(vol, (1,), placement, cap=caps, raw=True)
                cpu.append((time.perf_counter() - t0) * 1e3)
                same = all(g.tobytes() == h.tobytes() for g, h in zip(got, host))
            moved = vol.size + 16 * (caps[0] + caps[1])
            sized = median(times["sized"])
            doc[placement] = {"depth": SHAPE[0], "height": SHAPE[1], "width": SHAPE[2], "voxels_in_set": int(vol.sum()), "verts": caps[0],
                              "quads": caps[1], "bytes_moved": moved, "count_ms": median(times["count"]),
                              "count_spread": (max(times["count"]) - min(times["count"])) / median(times["count"]), "sized_ms": sized,
                              "sized_spread": (max(times["sized"]) - min(times["sized"])) / sized, "sized_gb_per_s": moved / sized * 1e-6,
                              "host_ms": median(cpu) if cpu else None, "host_calls": a.host_calls, "equal_host": same}
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_mesh_cases.json"))
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
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
