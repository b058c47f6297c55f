#!/usr/bin/env python3
"""What matching the components of two labelled stacks costs (mi_unet_volume_match), on one GPU.  Not the headline
metric (bench.py).

Three pairs of id stacks, in a child process of its own:
  blobs      64 x 512 x 512, six smooth organ-like blobs, two of them hollow, 0.05 % of the voxels flipped (tools/bench_volume_measure.py's
             stack) against the same stack moved by (3, -2, 1) in (z, y, x) without wrap-around; ids of both from
             mi_unet_volume_components under connectivity 26 with a table of 4096
  noise      16 x 512 x 512 of dense noise (30 % set) against itself moved by (0, 1, 0), ids under connectivity 6 with a table of 4096:
             thousands of components, of which the table's 4096 largest a side take part
  scattered  64 x 512 x 512, ids drawn per voxel from -1 .. 4097 on both sides, mp = mt = 4096: nearly every voxel a key of its own, and
             the 67 MB table to clear -- the worst case for the atomics
The wall time of the whole call is timed (host buffers in, the tables out): --rounds rounds of --calls calls after --warmup warm-up
calls; median and spread (max - min) / median over all calls.  Beside it mi_unet_volume_match_host and np.unique over the keys with
counts (the reference's table) on this host's CPU, each timed --host-calls times, and the check that device and host form give the
same bytes.  There is no figure of an earlier version: the stage is new.

Writes one JSON document (--out, default profiles/volume_match_cases.json) and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
CAP = 1 << 16


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def moved(vol, dz, dy, dx):
    """vol moved by (dz, dy, dx) without wrap-around"""
    import numpy as np
    out = np.zeros_like(vol)
    src = tuple(slice(max(0, -s), vol.shape[a] - max(0, s)) for a, s in enumerate((dz, dy, dx)))
    dst = tuple(slice(max(0, s), vol.shape[a] - max(0, -s)) for a, s in enumerate((dz, dy, dx)))
    out[dst] = vol[src]
    return out


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
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_volume_measure import make_blobs
    from miunet import binding
    doc = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        def ids_of(vol, conn):
            _, _, found, _, ids = eng.volume_components(vol, (1,), conn, cap=4096, want_ids=True)
            return np.ascontiguousarray(ids[0]), min(int(found[0]), 4096)

        stacks = {}
        blobs = make_blobs((64, 512, 512), 7)
        stacks["blobs"] = ids_of(blobs, 26) + ids_of(moved(blobs, 3, -2, 1), 26)
        noise = (np.random.default_rng(9).random((16, 512, 512)) < 0.3).astype(np.uint8)
        stacks["noise"] = ids_of(noise, 6) + ids_of(moved(noise, 0, 1, 0), 6)
        rng = np.random.default_rng(13)
        stacks["scattered"] = (rng.integers(-1, 4098, (64, 512, 512)).astype(np.int32), 4096,
                               rng.integers(-1, 4098, (64, 512, 512)).astype(np.int32), 4096)
        for name, (pred, mp, truth, mt) in stacks.items():
            if a.only and name not in a.only:
                continue
            got, ms = time_calls(lambda: eng.volume_match(pred, truth, mp, mt, cap=CAP), a)
            cpu, uniq, same = [], [], None
            for _ in range(a.host_calls):
                t0 = time.perf_counter()
                host = binding.volume_match_host(pred, truth, mp, mt, cap=CAP)
                cpu.append((time.perf_counter() - t0) * 1e3)
                same = all(g.tobytes() == h.tobytes() for g, h in zip(got[:3], host[:3])) and got[3] == host[3]
                t0 = time.perf_counter()
                ca = np.where((pred >= 1) & (pred <= mp), pred, 0).astype(np.int64)
                cb = np.where((truth >= 1) & (truth <= mt), truth, 0).astype(np.int64)
                np.unique(ca * (mt + 1) + cb, return_counts=True)
                uniq.append((time.perf_counter() - t0) * 1e3)
            whole = median(ms)
            doc[name] = {"depth": pred.shape[0], "height": pred.shape[1], "width": pred.shape[2], "pred_components": mp, "truth_components": mt,
                         "table_bytes": (mp + 1) * (mt + 1) * 4, "found": int(got[3]), "voxels_in_pred": int(got[0]["voxels"].sum()),
                         "voxels_in_truth": int(got[1]["voxels"].sum()), "voxels_in_both": int(got[0]["covered"].sum()),
                         "stack_bytes_read": 2 * pred.size * 4, "ms": whole, "spread": (max(ms) - min(ms)) / whole,
                         "host_ms": median(cpu) if cpu else None, "np_unique_ms": median(uniq) if uniq else None, "host_calls": len(cpu),
                         "equal_host": same}
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--only", nargs="*", default=[], help="the cases to run (default: all three)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_match_cases.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup",
                        str(a.warmup), "--host-calls", str(a.host_calls), "--only"] + a.only, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"child failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "cap": CAP, "cases": json.loads(r.stdout.strip().splitlines()[-1])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
