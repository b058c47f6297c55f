#!/usr/bin/env python3
"""What thinning the components of a mask stack to their medial lines costs (mi_unet_volume_skeleton), on one GPU.  Not
the headline metric (bench.py).

Three stacks, each in a child process of its own under its own time limit (--limit seconds), each labelled once by
mi_unet_volume_components under connectivity 26 (its ids are the input; m = min(found, 4096)):
  tree   64 x 512 x 512, a tube tree: a trunk of radius 9 that forks four times, the radius falling to 3; one component of thin, long,
         branching parts -- few passes, a long skeleton with ends and junctions
  blobs  64 x 512 x 512, six smooth organ-like blobs apart from each other (tools/bench_volume.py's kind), units (7, 7, 50): thick
         parts -- many passes, each over a shrinking surface, next to no skeleton
  noise  16 x 256 x 256 of dense noise (30 % set): thousands of components, most of a few voxels, one that percolates
The wall time of the whole call is timed (the host ids in; table, info, out_ids and r2 out): --rounds rounds of --calls calls after
--warmup warm-up calls; median and spread (max - min) / median over all calls.  Beside it the same call with radius off and no r2 (no
distance work), the passes the call reports, and the launches a call makes, counted from them: 2 to begin (5 with the distances),
per pass one memset, the end marks and per phase the candidates and eight sub-steps (56), 2 to finish.  On the same stack:
mi_unet_volume_skeleton_host on this host's CPU, timed --host-calls times, with the check that device and host give the same bytes
and the same passes.

Writes one JSON document (--out, default profiles/volume_skeleton_cases.json) and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
CASES = ("tree", "blobs", "noise")


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def draw_tube(vol, p0, p1, r):
    """the voxels within r of the segment p0 .. p1 (z, y, x), inside the segment's bounding box"""
    import numpy as np
    lo = [max(int(min(a, b) - r - 1), 0) for a, b in zip(p0, p1)]
    hi = [min(int(max(a, b) + r + 2), n) for a, b, n in zip(p0, p1, vol.shape)]
    z, y, x = np.meshgrid(*(np.arange(l, h, dtype=np.float64) for l, h in zip(lo, hi)), indexing="ij", sparse=True)
    d = [b - a for a, b in zip(p0, p1)]
    t = np.clip(((z - p0[0]) * d[0] + (y - p0[1]) * d[1] + (x - p0[2]) * d[2]) / sum(v * v for v in d), 0.0, 1.0)
    near = (z - p0[0] - t * d[0]) ** 2 + (y - p0[1] - t * d[1]) ** 2 + (x - p0[2] - t * d[2]) ** 2 <= r * r
    vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][near] = 1


def make_tree(shape):
    """a trunk along x that forks four times: the children leave in y, by less each time, and alternately up and down in z"""
    import numpy as np
    vol = np.zeros(shape, np.uint8)
    spread = (0.0, 120.0, 56.0, 28.0, 14.0)                     # the leaves end 28 apart in y: no two branches meet again
    todo = [((32.0, 256.0, 16.0), 0, 1.0)]
    while todo:
        p0, level, sign = todo.pop()
        p1 = (min(max(p0[0] + sign * 6.0 * (level > 0), 10.0), shape[0] - 11.0), p0[1] + sign * spread[level], p0[2] + 96.0)
        draw_tube(vol, p0, p1, 9.0 - 1.5 * level)
        if level < 4:
            todo += [(p1, level + 1, 1.0), (p1, level + 1, -1.0)]
    return vol


def make_blobs(shape):
    """six ellipsoids that do not touch"""
    import numpy as np
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij", sparse=True)
    vol = np.zeros(shape, np.uint8)
    for cz, cy, cx, rz, ry, rx in ((20, 100, 100, 14, 70, 60), (22, 110, 290, 12, 60, 70), (40, 380, 100, 18, 60, 70), (38, 370, 270, 14, 70, 60),
                                   (30, 250, 430, 25, 100, 45), (34, 440, 440, 10, 40, 40)):
        vol[((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = 1
    return vol


def make_case(name):
    import numpy as np
    if name == "tree":
        return make_tree((64, 512, 512)), (1, 1, 1)
    if name == "blobs":
        return make_blobs((64, 512, 512)), (7, 7, 50)
    return (np.random.default_rng(9).random((16, 256, 256)) < 0.3).astype(np.uint8), (1, 1, 1)


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
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    from miunet import binding
    vol, units = make_case(a.child)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        _, _, found, _, ids = eng.volume_components(vol, (1,), 26, cap=4096, want_ids=True)
        ids, m = ids[0], min(int(found[0]), 4096)
        got, ms = time_calls(lambda: eng.volume_skeleton(ids, m, units=units, want_ids=True, want_r2=True), a)
        bare, ms0 = time_calls(lambda: eng.volume_skeleton(ids, m, units=units, radius=False, want_ids=True), a)
    cpu, same = [], None
    for _ in range(a.host_calls):
        t0 = time.perf_counter()
        host = binding.volume_skeleton_host(ids, m, units=units, want_ids=True, want_r2=True)
        cpu.append((time.perf_counter() - t0) * 1e3)
        same = all(got[k].tobytes() == host[k].tobytes() for k in ("table", "ids", "r2")) and got["passes"] == host["passes"]
    t = got["table"]
    whole, no_radius = median(ms), median(ms0)
    print(json.dumps({"depth": vol.shape[0], "height": vol.shape[1], "width": vol.shape[2], "units": list(units), "components": int(found[0]), "m": m,
                      "voxels_in": int(t["voxels_in"].sum()), "voxels": int(t["voxels"].sum()), "ends": int(t["ends"].sum()),
                      "junctions": int(t["junctions"].sum()), "isolated": int(t["isolated"].sum()), "passes": got["passes"],
                      "deleted": got["deleted"], "launches": 5 + 56 * got["passes"] + 2, "launches_radius_off": 2 + 56 * bare["passes"] + 2,
                      "ms": whole, "spread": (max(ms) - min(ms)) / whole, "ms_radius_off": no_radius, "spread_radius_off": (max(ms0) - min(ms0)) / no_radius,
                      "host_ms": median(cpu) if cpu else None, "host_calls": len(cpu), "equal_host_bytes": same}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_skeleton_cases.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cases = {}
    for name in CASES:
        # a case that fails or overruns its limit ends the run: nothing more is started on the device behind it
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(a.rounds),
                            "--calls", str(a.calls), "--warmup", str(a.warmup), "--host-calls", str(a.host_calls)], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"case {name} failed with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        cases[name] = json.loads(r.stdout.strip().splitlines()[-1])
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "cases": cases}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
