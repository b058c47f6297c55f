#!/usr/bin/env python3
"""What splitting skeletons into nodes and branches costs (mi_unet_volume_branches), on one GPU.  Not the headline
metric (bench.py).

The input is the skeletons of tools/bench_volume_skeleton.py's three stacks -- the tube tree, six blobs, dense noise -- made once per
case by mi_unet_volume_components and mi_unet_volume_skeleton (ids and r2; m = min(found, 4096)), and the tube tree again with
prune_voxels = 5.  Each case runs in a child process of its own under its own time limit (--limit seconds).  The wall time of the whole
call is timed (the host ids and r2 in; both tables of 4096 rows, the per-id table, the map, out_ids and info out): --rounds rounds of
--calls calls after --warmup warm-up calls; median and spread (max - min) / median over all calls.  On the same input:
mi_unet_volume_branches_host on this host's CPU, timed --host-calls times, the ratio of the two medians, and the check that device and
host give the same bytes.  Per case the counts of the graph, and over all ids parts and loops from mi_unet_volume_branches_derive (null
where an id's branches did not fit the table).

Writes one JSON document (--out, default profiles/volume_branches_cases.json) and prints it as one line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
CASES = {"tree": ("tree", 0), "blobs": ("blobs", 0), "noise": ("noise", 0), "tree_prune5": ("tree", 5)}      # name -> (stack, prune_voxels)
ROWS = 4096


def child(a):
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_volume_skeleton import make_case, median, time_calls
    from miunet import binding
    stack, prune = CASES[a.child]
    vol, units = make_case(stack)
    kw = dict(units=units, prune_voxels=prune, cap_nodes=ROWS, cap_branches=ROWS, want_map=True, want_ids=True)
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        _, _, found, _, ids = eng.volume_components(vol, (1,), 26, cap=4096, want_ids=True)
        m = min(int(found[0]), 4096)
        sk = eng.volume_skeleton(ids[0], m, units=units, want_ids=True, want_r2=True)
        got, ms = time_calls(lambda: eng.volume_branches(sk["ids"], m, sk["r2"], **kw), a)
    cpu, same = [], None
    for _ in range(a.host_calls):
        t0 = time.perf_counter()
        host = binding.volume_branches_host(sk["ids"], m, sk["r2"], **kw)
        cpu.append((time.perf_counter() - t0) * 1e3)
        same = all(got[k].tobytes() == host[k].tobytes() for k in ("nodes", "branches", "graph", "map", "ids")) and all(
            got[k] == host[k] for k in ("found_nodes", "found_branches", "rounds", "stable"))
    g = got["graph"]
    parts = loops = None
    if got["found_branches"] <= ROWS:
        derived = [binding.volume_branches_derive(g[r], got["branches"], got["found_nodes"], r + 1, (1.0, 1.0, 1.0), 1.0) for r in range(m)]
        parts, loops = sum(d["parts"] for d in derived), sum(d["loops"] for d in derived)
    whole = median(ms)
    print(json.dumps({"depth": vol.shape[0], "height": vol.shape[1], "width": vol.shape[2], "m": m, "prune_voxels": prune,
                      "skeleton_voxels": int(sk["table"]["voxels"].sum()), "skeleton_ends": int(sk["table"]["ends"].sum()),
                      "skeleton_junction_voxels": int(sk["table"]["junctions"].sum()), "nodes": got["found_nodes"], "branches": got["found_branches"],
                      "ends": int(g["ends"].sum()), "junction_nodes": int(g["junction_nodes"].sum()), "junction_voxels": int(g["junction_voxels"].sum()),
                      "isolated": int(g["isolated"].sum()), "closed": int(g["closed"].sum()), "links": int(g["links"].sum()), "parts": parts,
                      "loops": loops, "rounds": got["rounds"], "stable": got["stable"], "pruned_spurs": int(g["pruned_spurs"].sum()),
                      "pruned_voxels": int(g["pruned_voxels"].sum()), "ms": whole, "spread": (max(ms) - min(ms)) / whole,
                      "host_ms": median(cpu) if cpu else None, "host_calls": len(cpu), "host_over_device": median(cpu) / whole if cpu else None,
                      "equal_host_bytes": same}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_branches_cases.json"))
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
