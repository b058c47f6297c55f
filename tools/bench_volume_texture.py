#!/usr/bin/env python3
"""What the texture of the components of a labelled stack costs (mi_unet_volume_texture), on one GPU.  Not the headline
metric (bench.py).

Three stacks of 64 x 512 x 512, each at 32 and at 64 levels, in a child process of its own:
  blobs_smooth  six smooth organ-like blobs, two of them hollow, 0.05 % of the voxels flipped (tools/bench_volume_measure.py's stack), ids
                from mi_unet_volume_components under connectivity 26 with a table of 4096; the intensity a ramp along the three axes
                plus noise of a level's width: nearly every pair falls into a few diagonal cells -- the contention case
  blobs_noise   the same ids under seeded uniform noise: every one of the L x L cells is hit
  dense_noise   dense noise (30 % set) labelled under connectivity 6 with a table of 4096, uniform noise intensity: thousands of small
                components (m = 4096 at 32 levels, the 1024 the cell limit admits at 64), nearly every tile a mixture of ids
The wall time of the whole call is timed (host buffers in, the tables out): --rounds rounds of --calls calls after --warmup warm-up
calls; median and spread (max - min) / median over all calls.  Beside it mi_unet_volume_texture_host on this host's CPU, timed
--host-calls times, and the check that device and host form give the same bytes.  With --lab-lib PATH (libmiunet_exp.so of `make lab`)
the blobs are timed once more in a second child through that library with MIUNET_VTX_EXP=1, which sends every count straight to memory
instead of the workgroup's LDS tables: the with / without comparison of 7.15.  There is no figure of an earlier version: the stage is new.

Writes one JSON document (--out, default profiles/volume_texture_cases.json) and prints it as one line."""
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

        rng = np.random.default_rng(17)
        z, y, x = np.indices(SHAPE, dtype=np.int32)
        smooth = (2000 + 40 * x + 30 * y + 300 * z + rng.integers(0, 600, SHAPE)).astype(np.uint16)
        del z, y, x
        noise = rng.integers(0, 65536, SHAPE).astype(np.uint16)
        blobs = ids_of(make_blobs(SHAPE, 7), 26)
        dense = ids_of((np.random.default_rng(9).random(SHAPE) < 0.3).astype(np.uint8), 6)
        stacks = {"blobs_smooth": blobs + (smooth,), "blobs_noise": blobs + (noise,), "dense_noise": dense + (noise,)}
        for name, (ids, m, inten) in stacks.items():
            if a.only and name not in a.only:
                continue
            for levels in a.levels:
                mm = min(m, binding.VTEX_MAX_CELLS // (levels * levels))
                got, ms = time_calls(lambda: eng.volume_texture(ids, inten, mm, levels), a)
                cpu, same = [], None
                for _ in range(a.host_calls):
                    t0 = time.perf_counter()
                    host = binding.volume_texture_host(ids, inten, mm, levels)
                    cpu.append((time.perf_counter() - t0) * 1e3)
                    same = all(g.tobytes() == h.tobytes() for g, h in zip(got, host))
                whole = median(ms)
                top = int(np.argmax(got[0]["voxels"]))
                doc[f"{name}_L{levels}"] = {"depth": SHAPE[0], "height": SHAPE[1], "width": SHAPE[2], "components": mm, "levels": levels,
                                            "voxels_in_components": int(got[0]["voxels"].sum()), "pairs": int(got[0]["pairs"].sum()),
                                            "cells_of_the_largest": int((got[2][top] != 0).sum()), "table_bytes": mm * levels * levels * 4,
                                            "stack_bytes_read": ids.size * 6, "ms": whole, "spread": (max(ms) - min(ms)) / whole,
                                            "gb_per_s": ids.size * 6 / whole / 1e6, "host_ms": median(cpu) if cpu else None,
                                            "host_calls": len(cpu), "equal_host": same}
    print(json.dumps(doc))


def run_child(a, only, host_calls, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup",
                        str(a.warmup), "--host-calls", str(host_calls), "--levels"] + [str(v) for v in a.levels] + ["--only"] + only, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise SystemExit(f"child failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--only", nargs="*", default=[], help="the stacks to run (default: all three)")
    ap.add_argument("--levels", nargs="*", type=int, default=[32, 64], help="the level counts to run (default: 32 64)")
    ap.add_argument("--lab-lib", default="", help="libmiunet_exp.so: time the blobs once more without the LDS tables")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_texture_cases.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "cases": run_child(a, a.only, a.host_calls)}
    if a.lab_lib:
        blobs = [n for n in ("blobs_smooth", "blobs_noise") if not a.only or n in a.only]
        for key, exp in (("lab_with_lds_table", "0"), ("lab_without_lds_table", "1")):
            env = dict(os.environ, MIUNET_LIB=os.path.abspath(a.lab_lib), MIUNET_VTX_EXP=exp)
            doc[key] = {k: {f: v[f] for f in ("ms", "spread", "equal_host")} for k, v in run_child(a, blobs, 1, env).items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
