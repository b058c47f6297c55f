#!/usr/bin/env python3
"""What the neighbourhood-difference, dependence and distance-zone tables of the components of a labelled stack cost
(mi_unet_volume_nbhood), on one GPU.  Not the headline metric (bench.py).

tools/bench_volume_zones.py's three stacks of 64 x 512 x 512, each at 32 and at 64 levels with alpha 1 and max_dist 32, in a child
process of its own:
  blobs_smooth  six smooth organ-like blobs, two of them hollow, 0.05 % of the voxels flipped, ids from mi_unet_volume_components under
                connectivity 26 with a table of 4096; the intensity a ramp along the three axes plus noise of a level's width: most
                voxels have all 26 neighbours and name a handful of cells, the blobs are tens of voxels deep
  blobs_noise   the same ids under seeded uniform noise: the lanes of a wave name many cells, nearly every voxel is a zone of its own
  dense_noise   dense noise (30 % set) labelled under connectivity 6 with a table of 4096, uniform noise intensity: thousands of small
                components (m = 4096 at 32 levels, the 1024 the cell limit admits at 64), nearly every tile a mixture of ids
The wall time of the whole call is timed (host buffers in, all eight tables out): --rounds rounds of --calls calls after --warmup
warm-up calls; median and spread (max - min) / median over all calls.  Every call times, one after the other in the one process and in
an order that rotates from call to call, the call as shipped, the call with every count of k_vnb_gather sent to memory
(MIUNET_VNB_EXP=1), the call with the leading component's counts in LDS (MIUNET_VNB_EXP=2), and three partial calls that say where the
time goes: no table (upload, keys, voxels), the six neighbourhood tables alone, the two distance-zone tables alone.  Beside it mi_unet_volume_nbhood_host on this host's CPU, timed
--host-calls times, and the check that device and host form give the same bytes.  There is no figure of an earlier version: the stage
is new.

Writes one JSON document (--out, default profiles/volume_nbhood_cases.json) and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
SHAPE = (64, 512, 512)
ALPHA, MAX_DIST = 1, 32
GATHER = ("ngt", "dep", "ngt_axial", "dep_axial")
ZONES = ("dzm", "dzm_axial")


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


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
                mm = min(m, binding.VTEX_MAX_CELLS // (levels * max(levels, 32, MAX_DIST)))
                call = lambda want=binding.VNBHOOD_WANT: eng.volume_nbhood(ids, inten, mm, levels, alpha=ALPHA, max_dist=MAX_DIST, want=want)
                # (name, MIUNET_VNB_EXP or None, want)
                variants = (("ms", None, binding.VNBHOOD_WANT), ("memory_form_ms", "1", binding.VNBHOOD_WANT), ("lds_form_ms", "2", binding.VNBHOOD_WANT),
                            ("entry_only_ms", None, ()), ("neighbourhoods_only_ms", None, GATHER), ("zones_only_ms", None, ZONES))
                times = {v[0]: [] for v in variants}
                got = None

                def one(key, exp, want):
                    if exp is None:
                        os.environ.pop("MIUNET_VNB_EXP", None)
                    else:
                        os.environ["MIUNET_VNB_EXP"] = exp
                    t0 = time.perf_counter()
                    res = call(want)
                    dt = (time.perf_counter() - t0) * 1e3
                    os.environ.pop("MIUNET_VNB_EXP", None)
                    return res, dt

                for _ in range(a.warmup):
                    for v in variants:
                        one(*v)
                for i in range(a.rounds * a.calls):
                    for v in variants[i % len(variants):] + variants[:i % len(variants)]:      # interleaved, and every variant in every position
                        res, dt = one(*v)
                        times[v[0]].append(dt)
                        if v[0] == "ms":
                            got = res
                forms = [one(*v)[0] for v in variants[1:3]]
                forms_equal = all(f[0].tobytes() == got[0].tobytes() and all(f[1][n].tobytes() == got[1][n].tobytes() for n in binding.VNBHOOD_TABLES) for f in forms)
                cpu, same = [], None
                for _ in range(a.host_calls):
                    t0 = time.perf_counter()
                    host = binding.volume_nbhood_host(ids, inten, mm, levels, alpha=ALPHA, max_dist=MAX_DIST)
                    cpu.append((time.perf_counter() - t0) * 1e3)
                    same = got[0].tobytes() == host[0].tobytes() and all(got[1][n].tobytes() == host[1][n].tobytes() for n in binding.VNBHOOD_TABLES)
                table, tabs = got
                rec = {"depth": SHAPE[0], "height": SHAPE[1], "width": SHAPE[2], "components": mm, "levels": levels, "alpha": ALPHA, "max_dist": MAX_DIST,
                       "voxels_in_components": int(table["voxels"].sum()), "valid": int(table["valid"].sum()), "zones": int(table["zones"].sum()),
                       "deepest": int(table["deepest"].max()), "deepest_axial": int(table["deepest_axial"].max()), "clamped": int(table["clamped"].sum()),
                       "dependence_max": int(table["dependence_max"].max()), "largest_diff_cell": int(tabs["ngt_diff"].max()),
                       "table_bytes_returned": int(sum(t.nbytes for t in tabs.values())), "stack_bytes_read": ids.size * 6}
                for key, ms in times.items():
                    rec[key] = median(ms)
                rec["spread"] = (max(times["ms"]) - min(times["ms"])) / rec["ms"]
                rec.update({"forms_equal": forms_equal, "host_ms": median(cpu) if cpu else None, "host_calls": len(cpu), "equal_host": same})
                doc[f"{name}_L{levels}"] = rec
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--only", nargs="*", default=[], help="the stacks to run (default: all three)")
    ap.add_argument("--levels", nargs="*", type=int, default=[32, 64], help="the level counts to run (default: 32 64)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_nbhood_cases.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "cases": run_child(a, a.only, a.host_calls)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
