#!/usr/bin/env python3
"""What the spatial statistics of the components of a labelled stack cost (mi_unet_volume_spatial), on one GPU.  Not the
headline metric (bench.py).

Three stacks (those of tools/bench_volume_measure.py), in a child process of its own:
  blobs   64 x 512 x 512, six smooth organ-like blobs, two of them hollow, 0.05 % of the voxels flipped; ids from
          mi_unet_volume_components under connectivity 26 with a table of 4096
  noise   16 x 256 x 256 of dense noise (30 % set) under connectivity 6: thousands of small components
  sheet   64 x 128 x 48, the set { x + y + z = 0 mod 3 } as one component: 131072 voxels -- the default cap exactly
Each with a seeded u16 intensity, the units (7, 7, 50) and a peak sphere of 62 units (6.2 mm at 0.1 mm per unit).  The wall time of the
whole call is timed (host buffers in, the table out): --rounds rounds of --calls calls after --warmup warm-up calls; median and spread
(max - min) / median over all calls.  The pair rate is the pairs of the searched components over the whole call's time, and over the
time the call takes beyond the same call with max_voxels = 0 (the sums and the peaks alone).  Beside it mi_unet_volume_spatial_host on
this host's CPU, timed --host-calls times where the case holds fewer than --host-pairs pairs (default 1e10: under a minute), and the
check that both give the same integer bytes and pair sums within 2 (P + 8) eps T'.

Writes one JSON document (--out, default profiles/volume_spatial_cases.json) and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
UNITS = (7, 7, 50)
PEAK_R = 62
INT_BYTES = 136                             # the integer part of a mi_unet_vspatial


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def make_blobs(shape, seed):
    """six ellipsoids, apart from each other (tools/bench_volume_mesh.py), the first two hollow, then 0.05 % of the voxels flipped"""
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


def time_calls(fn, a):
    for _ in range(a.warmup):
        got = fn()
    ms = []
    for _ in range(a.rounds):
        for _ in range(a.calls):
            t0 = time.perf_counter()
            got = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
    return got, ms


def child(a):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    from miunet import binding
    doc = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        stacks = {}
        for name, vol, conn in (("blobs", make_blobs((64, 512, 512), 7), 26),
                                ("noise", (np.random.default_rng(9).random((16, 256, 256)) < 0.3).astype(np.uint8), 6)):
            _, _, found, _, ids = eng.volume_components(vol, (1,), conn, cap=4096, want_ids=True)
            stacks[name] = (np.ascontiguousarray(ids[0]), min(int(found[0]), 4096))
        z, y, x = np.indices((64, 128, 48))
        stacks["sheet"] = (((x + y + z) % 3 == 0).astype(np.int32), 1)
        eps = float(np.finfo(np.float64).eps)
        for name, (ids, m) in stacks.items():
            inten = np.random.default_rng(5).integers(0, 65536, ids.shape).astype(np.uint16)
            got, ms = time_calls(lambda: eng.volume_spatial(ids, inten, m=m, units=UNITS, peak_r=PEAK_R), a)
            _, ms0 = time_calls(lambda: eng.volume_spatial(ids, inten, m=m, units=UNITS, max_voxels=0, peak_r=PEAK_R), a)
            pairs = int(got["pairs"].sum())
            cpu, same, near = [], None, None
            for _ in range(a.host_calls if pairs < a.host_pairs else 0):
                t0 = time.perf_counter()
                host = binding.volume_spatial_host(ids, inten, m=m, units=UNITS, peak_r=PEAK_R)
                cpu.append((time.perf_counter() - t0) * 1e3)
                ints = lambda t: t.view(np.uint8).reshape(len(t), -1)[:, :INT_BYTES].tobytes()
                same = ints(got) == ints(host)
                ymax = np.maximum(host["imax"] - host["centre"], host["centre"] - host["imin"]).astype(np.float64)
                near = True
                for f, scale in (("s0", 1.0), ("s1", 2.0 * ymax), ("s2", ymax * ymax), ("s3", 4.0 * ymax * ymax)):
                    near = near and bool((np.abs(got[f] - host[f]) <= 2.0 * (host["pairs"] + 8) * eps * host["s0"] * scale).all())
            whole, sums = median(ms), median(ms0)
            doc[name] = {"depth": ids.shape[0], "height": ids.shape[1], "width": ids.shape[2], "components": m,
                         "voxels_in_components": int(got["voxels"].sum()), "largest_voxels": int(got["voxels"].max()),
                         "searched": int(got["searched"].sum()), "skipped_by_cap": int(((got["voxels"] > 1) & (got["searched"] == 0)).sum()),
                         "pairs": pairs, "ms": whole, "spread": (max(ms) - min(ms)) / whole, "ms_without_pairs": sums,
                         "spread_without_pairs": (max(ms0) - min(ms0)) / sums, "pairs_per_s_whole_call": pairs / whole * 1e3,
                         "pairs_per_s_search": pairs / (whole - sums) * 1e3 if whole - sums > 0.05 * whole else None,
                         "host_ms": median(cpu) if cpu else None, "host_calls": len(cpu), "equal_host_integers": same, "sums_within_bound": near}
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--host-pairs", type=float, default=1e10, help="the host form is timed on the cases with fewer pairs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_spatial_cases.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup",
                        str(a.warmup), "--host-calls", str(a.host_calls), "--host-pairs", str(a.host_pairs)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"child failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "units": list(UNITS), "peak_r": PEAK_R, "cases": json.loads(r.stdout.strip().splitlines()[-1])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
