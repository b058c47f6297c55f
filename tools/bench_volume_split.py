#!/usr/bin/env python3
"""What splitting the touching objects of a mask stack costs (mi_unet_volume_split), on one GPU.  Not the headline
metric (bench.py).

Three stacks, each in a child process of its own under its own time limit (--limit seconds):
  blobs       64 x 512 x 512, six smooth organ-like blobs pushed together in pairs so that the two of a pair touch along a neck;
              connectivity 26, units (7, 7, 50), neck 150 units (15 mm at 0.1 mm per unit): three components, six pieces
  noise       16 x 256 x 256 of dense noise (30 % set) under connectivity 6, units (1, 1, 1), neck 1: thousands of cores and of
              coreless pieces
  serpentine  3 x 257 x 512: one path of a voxel's width through every other row of the middle slice, a block at either end as the
              two cores (tests/volume_split_ref.py's serpentine, longer); connectivity 6, units (3, 3, 10), neck 10: the growth
              crosses the same tiles again and again
The wall time of the whole call is timed (the host stack in; table, info, ids and stats out): --rounds rounds of --calls calls after
--warmup warm-up calls; median and spread (max - min) / median over all calls; the rounds of the growth as the call reports them.
The share of the growth is the time the call takes beyond the same call with min_core above every core -- no core kept, no round
with a tile to run, every piece coreless -- over the whole.  Beside it, on the same stack: mi_unet_volume_components (the stage's
floor: one labelling, one table) and mi_unet_volume_split_host on this host's CPU, timed --host-calls times, with the check that
device and host give the same bytes.

Writes one JSON document (--out, default profiles/volume_split_cases.json) and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
CASES = ("blobs", "noise", "serpentine")
NO_CORE = 2 ** 31 - 1


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def make_blobs(shape):
    """three pairs of ellipsoids; the centres of a pair lie 0.98 of the sum of their half-axes apart along x, so the two overlap in a
    lens much thinner than either"""
    import numpy as np
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij", sparse=True)
    vol = np.zeros(shape, np.uint8)
    for cz, cy, cx, rz, ry, rx in ((20, 110, 110, 14, 80, 70), (22, 120, 247, 12, 60, 70), (40, 380, 110, 18, 60, 80), (38, 370, 257, 14, 70, 70),
                                   (30, 250, 380, 25, 100, 50), (34, 260, 468, 10, 50, 40)):
        vol[((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = 1
    return vol


def make_serpentine(h, w):
    import numpy as np
    v = np.zeros((3, h, w), np.uint8)
    for r in range(h):
        if r % 2 == 0:
            v[1, r, :] = 1
        else:
            v[1, r, w - 1 if (r // 2) % 2 == 0 else 0] = 1
    v[0:3, 0:5, 0:5] = 1
    v[0:3, h - 5:h, (w - 5 if ((h - 1) // 2) % 2 == 0 else 0):(w if ((h - 1) // 2) % 2 == 0 else 5)] = 1
    return v


def make_case(name):
    import numpy as np
    if name == "blobs":
        return make_blobs((64, 512, 512)), dict(units=(7, 7, 50), connectivity=26, neck_r=150)
    if name == "noise":
        return (np.random.default_rng(9).random((16, 256, 256)) < 0.3).astype(np.uint8), dict(units=(1, 1, 1), connectivity=6, neck_r=1)
    return make_serpentine(257, 512), dict(units=(3, 3, 10), connectivity=6, neck_r=10)


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
    vol, kw = make_case(a.child)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        got, ms = time_calls(lambda: eng.volume_split(vol, (1,), cap=4096, want_ids=True, **kw), a)
        _, ms0 = time_calls(lambda: eng.volume_split(vol, (1,), cap=4096, want_ids=True, min_core=NO_CORE, **kw), a)
        comp, msc = time_calls(lambda: eng.volume_components(vol, (1,), kw["connectivity"], cap=4096, want_ids=True), a)
    cpu, same = [], None
    for _ in range(a.host_calls):
        t0 = time.perf_counter()
        host = binding.volume_split_host(vol, (1,), cap=4096, want_ids=True, **kw)
        cpu.append((time.perf_counter() - t0) * 1e3)
        same = all(got[k].tobytes() == host[k].tobytes() for k in ("table", "info", "found", "stats", "ids"))
    st = got["stats"][0]
    whole, bare, floor = median(ms), median(ms0), median(msc)
    print(json.dumps({"depth": vol.shape[0], "height": vol.shape[1], "width": vol.shape[2], "units": list(kw["units"]),
                      "connectivity": kw["connectivity"], "neck_r": kw["neck_r"], "voxels": int(st["in_voxels"]), "core_voxels": int(st["core_voxels"]),
                      "components": int(comp[2][0]), "cores": int(st["cores"]), "pieces": int(st["pieces"]), "coreless": int(st["coreless"]),
                      "max_reach": int(st["max_reach"]), "rounds": int(got["rounds"][0]), "ms": whole, "spread": (max(ms) - min(ms)) / whole,
                      "ms_without_growth": bare, "growth_share": (whole - bare) / whole, "components_ms": floor,
                      "spread_components": (max(msc) - min(msc)) / floor, "host_ms": median(cpu) if cpu else None, "host_calls": len(cpu),
                      "equal_host_bytes": same}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_split_cases.json"))
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
