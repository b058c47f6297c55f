#!/usr/bin/env python3
"""Tiled inference against the same tiles through mi_unet_infer_u8, on one GPU.  Not the headline metric (bench.py): the
measurement behind DESIGN.md 7.2.

Default fp32 engine (512 x 512, base 64, 4 levels), one 2048 x 1536 image, halo 32 = 5 x 4 = 20 tiles.  After a warm-up the two
calls alternate in one process: mi_unet_infer_tiled_u8 on the image, and mi_unet_infer_u8 on the 20 tiles cut on the host
beforehand (that path is the one every earlier version of the library has; cutting the tiles is not timed).  Both go through
the C entry points with buffers allocated once.  Then one profiled call of each tiled form for the three kernels of
csrc/tiles.hip: time and algorithmic bytes from mi_unet_get_kernel_stats, the resulting rate, and its share of the 6.3 TB/s a
float4 copy reaches on this chip.  Writes one JSON document (--out, default profiles/tiled_2048x1536.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd"))
import numpy as np  # noqa: E402

from miunet import binding, synth  # noqa: E402
from miunet.binding import _check, _ptr  # noqa: E402
from miunet.spec import UNetSpec, pack_weights  # noqa: E402

HBM_COPY_RATE = 6.3e12          # bytes/s of a float4 copy on an MI355X


def summary(ms):
    a = np.sort(np.asarray(ms))
    return {"n": len(a), "median_ms": float(np.median(a)), "mean_ms": float(a.mean()), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)), "std_ms": float(a.std())}


def kernel_table(stats):
    out = {}
    for fam in ("tile_gather", "normalise_u16", "tile_stitch"):
        rows = [s for s in stats if s["kernel"] == fam]
        ms, nbytes = sum(s["ms"] for s in rows), sum(s["bytes"] for s in rows)
        rate = nbytes / (ms * 1e-3) if ms > 0 else None
        out[fam] = {"launches": len(rows), "ms": ms, "algorithmic_bytes": nbytes, "bytes_per_s": rate,
                    "share_of_hbm_copy_rate": rate / HBM_COPY_RATE if rate else None}
    out["network_ms"] = sum(s["ms"] for s in stats if s["kernel"] not in out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1536)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_2048x1536.json"))
    a = ap.parse_args()
    if binding.device_count() < 1:
        raise SystemExit("bench_tiled needs a HIP device")
    H, W, halo = a.height, a.width, a.halo
    spec = UNetSpec()
    blob = pack_weights(spec, synth.make_weights(spec, 1234))
    img = synth.make_images(1, H, W, 1, 0x5EED, "blobs")[0]
    raw = synth.make_raw16(H, W, seed=21)
    oy, cy = binding.tile_axis(H, 512, halo)
    ox, cx = binding.tile_axis(W, 512, halo)
    tiles = np.ascontiguousarray(np.stack([img[y:y + 512, x:x + 512] for y in oy for x in ox]))
    nt = len(tiles)
    L = binding.lib()
    labels = np.empty((H, W), np.uint8)
    tile_labels = np.empty((nt, 512, 512), np.uint8)
    with binding.Engine() as eng:
        eng.load_weights(blob)

        def tiled():
            _check(L.mi_unet_infer_tiled_u8(eng._h, _ptr(img), H, W, halo, _ptr(labels), None))

        def stacked():
            _check(L.mi_unet_infer_u8(eng._h, _ptr(tiles), nt, _ptr(tile_labels), None))

        for _ in range(a.warmup):
            tiled()
            stacked()
        # same results: the stitched label map is the owned rectangles of the per-tile label maps
        want = np.empty((H, W), np.uint8)
        for ty in range(len(oy)):
            for tx in range(len(ox)):
                want[cy[ty]:cy[ty + 1], cx[tx]:cx[tx + 1]] = tile_labels[ty * len(ox) + tx][cy[ty] - oy[ty]:cy[ty + 1] - oy[ty],
                                                                                              cx[tx] - ox[tx]:cx[tx + 1] - ox[tx]]
        same = bool(np.array_equal(want, labels))
        t_tiled, t_stacked = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            tiled()
            t1 = time.perf_counter()
            stacked()
            t2 = time.perf_counter()
            t_tiled.append((t1 - t0) * 1e3)
            t_stacked.append((t2 - t1) * 1e3)
        tiled()
        stages = eng.last_stage_ms()
        # the three kernels, profiled (event pairs around every launch; graphs off while profiling)
        eng.set_profiling(True)
        tiled()
        k_u8 = kernel_table(eng.kernel_stats())
        eng.set_profiling(True)
        eng.infer_tiled_raw16(raw, halo, want_norm=True, want_logits=True)
        k_raw = kernel_table(eng.kernel_stats())
        eng.set_profiling(False)
    doc = {
        "what": "mi_unet_infer_tiled_u8 on one image against mi_unet_infer_u8 on the same tiles cut on the host, alternating in one process",
        "device": "one MI355X", "engine": "512 x 512, base 64, 4 levels, fp32 default plan, max_batch 16",
        "image": f"{W} x {H} (W x H), halo {halo}: {len(ox)} x {len(oy)} = {nt} tiles",
        "calls": a.calls, "warmup": a.warmup, "timing": "host clock around the C call (each call ends in a stream synchronise)",
        "results_identical": same,
        "tiled_call": summary(t_tiled), "infer_u8_on_host_tiles": summary(t_stacked),
        "tiled_over_infer_u8_median": float(np.median(t_tiled) / np.median(t_stacked)),
        "pcie_bytes": {"tiled_up": int(img.nbytes), "tiled_down": int(labels.nbytes), "infer_u8_up": int(tiles.nbytes),
                       "infer_u8_down": int(tile_labels.nbytes)},
        "stage_ms_of_one_tiled_call": stages,
        "kernels_u8_form_labels_only": k_u8,
        "kernels_raw_form_with_logits": k_raw,
        "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
