#!/usr/bin/env python3
"""What putting slices between the slices of a stack of masks costs (mi_unet_volume_interp), on one GPU.  Not the
headline metric (bench.py).

Stacks of 64 x 512 x 512 under the in-plane units (1, 1), in a child process of its own:
  blobs_k2 / _k4 / _k7  six smooth organ-like blobs, two of them hollow, 0.05 % of the voxels flipped (tools/bench_volume_measure.py's
                        stack) at the factors 2, 4 and 7: 127, 253 and 442 output slices
  dense_noise_k4        seeded noise, half of the voxels set: every search ends at once, every other voxel between two slices is mixed
  blobs_k4_intensity    blobs at factor 4 with a u16 intensity stack blended beside the masks
The wall time of the whole call is timed (host buffers in, the interpolated stack out): --rounds rounds of --calls calls after --warmup
warm-up calls; median and spread (max - min) / median over all calls.  Beside it mi_unet_volume_interp_host on this host's CPU, timed
--host-calls times, and the check that device and host form give the same bytes.  There is no figure of an earlier version: the stage
is new.  The kernels' own times come from a rocprofv3 --kernel-trace run of the child (--child --only <case> behind the profiler).

"ball" is computed by the host forms alone and needs no device (--ball-only prints just that): a ball of radius 20 pixels sampled every
5 pixels along z (spacing 1, 1, 5), its surface-nets mesh area and voxel volume on the original stack and on the stack interpolated at
factor 5, against 4 pi r^2 and 4/3 pi r^3.

Writes one JSON document (--out, default profiles/volume_interpolate_cases.json) and prints it as one line."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
SHAPE = (64, 512, 512)
CASES = (("blobs_k2", "blobs", 2, False), ("blobs_k4", "blobs", 4, False), ("blobs_k7", "blobs", 7, False), ("dense_noise_k4", "noise", 4, False),
         ("blobs_k4_intensity", "blobs", 4, True))


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


def imports():
    sys.path.insert(0, os.path.join(ROOT, PKG_REL))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from miunet import binding
    return np, binding


def child(a):
    np, binding = imports()
    from bench_volume_measure import make_blobs
    stacks = {"blobs": make_blobs(SHAPE, 7), "noise": (np.random.default_rng(9).random(SHAPE) < 0.5).astype(np.uint8)}
    inten = np.random.default_rng(17).integers(0, 65536, SHAPE).astype(np.uint16)
    doc = {}
    with binding.Engine(64, 64, 1, 16, 4, 4, max_batch=1) as eng:       # the stage needs the device, not the network
        for name, stack, k, with_intensity in CASES:
            if a.only and name not in a.only:
                continue
            vol, img = stacks[stack], inten if with_intensity else None
            got, ms = time_calls(lambda: eng.volume_interp(vol, (1,), (1, 1), k, img), a)
            cpu, same = [], None
            for _ in range(a.host_calls):
                t0 = time.perf_counter()
                host = binding.volume_interp_host(vol, (1,), (1, 1), k, img)
                cpu.append((time.perf_counter() - t0) * 1e3)
                same = all(g.tobytes() == h.tobytes() for g, h in zip(got, host))
            whole, st = median(ms), got[1][0]
            moved = vol.size + got[0].size + (img.nbytes + got[2].nbytes if with_intensity else 0)
            doc[name] = {"depth": SHAPE[0], "height": SHAPE[1], "width": SHAPE[2], "factor": k, "slices": int(got[0].shape[1]),
                         "in_voxels": int(st["in_voxels"]), "out_voxels": int(st["out_voxels"]), "mixed": int(st["mixed"]),
                         "mixed_set": int(st["mixed_set"]), "ties": int(st["ties"]), "bytes_over_the_bus": int(moved), "ms": whole,
                         "spread": (max(ms) - min(ms)) / whole, "host_ms": median(cpu) if cpu else None, "host_calls": len(cpu), "equal_host": same}
    print(json.dumps(doc))


def ball():
    """host forms only"""
    np, binding = imports()
    r, step, side = 20, 5, 48
    z, y, x = np.mgrid[0:45, 0:side, 0:side]
    fine = ((z - 22) ** 2 + (y - 24) ** 2 + (x - 24) ** 2 <= r * r).astype(np.uint8)
    coarse = np.ascontiguousarray(fine[2::step])                         # 9 slices, the middle one through the centre
    out, stats = binding.volume_interp_host(coarse, (1,), (1, 1), step)

    def mesh(vol, spacing):
        meshes, _ = binding.volume_mesh_host(vol, (1,), "nets")
        return binding.volume_mesh_derive(meshes[0][0], meshes[0][1], spacing)

    m0, m1 = mesh(coarse, (1, 1, step)), mesh(out[0], (1, 1, 1))
    return {"radius_px": r, "slice_step_px": step, "slices": int(coarse.shape[0]), "factor": step, "slices_interpolated": int(out.shape[1]),
            "sphere_area": 4 * math.pi * r * r, "sphere_volume": 4 / 3 * math.pi * r ** 3, "fine_voxels": int(fine.sum()),
            "original": {"voxel_volume": int(coarse.sum()) * step, "nets_area": m0["area_mm2"], "nets_volume": m0["volume_mm3"]},
            "interpolated": {"voxel_volume": int(stats[0]["out_voxels"]), "nets_area": m1["area_mm2"], "nets_volume": m1["volume_mm3"]}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--only", nargs="*", default=[], help="the cases to run (default: all)")
    ap.add_argument("--ball-only", action="store_true", help="print the ball's figures (host forms, no device) and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_interpolate_cases.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    if a.ball_only:
        print(json.dumps(ball()))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup",
                        str(a.warmup), "--host-calls", str(a.host_calls), "--only"] + a.only, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"child failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    doc = {"rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "cases": json.loads(r.stdout.strip().splitlines()[-1]), "ball": ball()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
