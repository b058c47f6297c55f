#!/usr/bin/env python3
"""What a morphology setting costs in the segmentation tail (mi_unet_set_morph), on one GPU.  Not the headline metric
(bench.py).

The default engine (512 x 512, base 64, 4 levels, max_batch 16) on 16 RAW images of 512 x 512 through mi_unet_segment_raw16_multi,
--rounds rounds of --calls calls after a warm-up, at K = 1 (3 classes, the default target) and K = 3 targets (4 classes): the device
time of MI_UNET_STAGE_POSTPROCESS (mi_unet_last_stage_ms), the wall time of the whole call and images / s, for the default setting
(the two 3x3 launches), the box and the disc at r = 4 and 31, the disc at r = 1 (the box at r = 1 IS the default) and { RECT, 2, 2 }.
Then one 2048 x 1536 image through mi_unet_segment_tiled_raw16_multi at the default and at { DISC, 4, 0 }.  Every side runs in a
child process of its own; medians over all calls and the spread (max - min) / median are reported.  With --parent (a checkout of the
parent commit whose libmiunet.so is built) the parent's default runs before AND after this tree's, so that a drift of the card shows
as the distance of the two parent runs:

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/unet-medical-image-contour-segmentation-cpp_amd libmiunet.so
    python tools/bench_morph.py --parent /tmp/parent

Writes one JSON document (--out, default profiles/morph_512x16.json) and prints the table of DESIGN.md 7.7."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
K3 = [(1, 0.01), (2, 0.06), (3, 0.0)]       # needs a 4-class network: the K = 3 sides run on one
SETTINGS = [("default", None), ("disc1", ("disc", 1, 0)), ("rect4", ("rect", 4, 0)), ("disc4", ("disc", 4, 0)),
            ("rect31", ("rect", 31, 0)), ("disc31", ("disc", 31, 0)), ("rect2close2", ("rect", 2, 2))]


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def summary(rows, batch):
    """rows of (postprocess ms, wall ms) -> medians and relative spreads"""
    out = {}
    for k, name in enumerate(("postprocess_ms", "call_ms")):
        v = [r[k] for r in rows]
        out[name] = median(v)
        out[name.replace("_ms", "_spread")] = (max(v) - min(v)) / median(v)
    out["images_per_s"] = batch / (out["call_ms"] * 1e-3)
    return out


def threshold_weights(synth, spec):
    """the intensity classifier with one band per class: cuts at 60.5, 110.5, ..."""
    t = synth.make_threshold_weights(spec)
    if spec.classes != 3:
        cuts = [(60.5 + 50.0 * j) / 255.0 for j in range(spec.classes - 1)]
        t["outc.w"][:] = 0
        t["outc.b"][:] = 0
        for c in range(spec.classes):
            t["outc.w"][c, 0] = float(c)
            t["outc.b"][c] = -float(sum(cuts[:c]))
    return t


def child(a):
    """one process: the library of `a.tree`; the settings it knows (a tree without mi_unet_set_morph runs the default alone)"""
    sys.path.insert(0, os.path.join(a.tree, PKG_REL))
    from miunet import binding, synth
    from miunet.spec import UNetSpec, pack_weights
    raws = [synth.make_raw16(512, 512, seed=21 + i) for i in range(a.batch)]
    doc = {}

    def measure(eng, fn, batch):
        def timed():
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
            return eng.last_stage_ms()["postprocess"], wall

        rows = []
        for _ in range(a.rounds):
            for _ in range(a.warmup):
                fn()
            rows += [timed() for _ in range(a.calls)]
        return summary(rows, batch)

    for classes, targets in ((3, None), (4, K3)):
        spec = UNetSpec(classes=classes)
        eng = binding.Engine(classes=classes, max_batch=a.batch)
        eng.load_weights(pack_weights(spec, threshold_weights(synth, spec)))
        if targets:
            eng.set_targets(targets)
        p = eng.segment_raw16_multi_prepare(raws, cap_points=1 << 15, cap_contours=64)
        for name, morph in SETTINGS:
            if morph is not None and not hasattr(eng, "set_morph"):
                continue
            if hasattr(eng, "set_morph"):
                eng.set_morph(None if morph is None else [morph])
            doc[f"k{len(targets) if targets else 1}.{name}"] = measure(eng, lambda: eng.segment_raw16_multi_run(p), a.batch)
        if not targets and a.tiled:
            big = synth.make_raw16(1536, 2048, seed=77)
            for name, morph in (("default", None), ("disc4", ("disc", 4, 0))):
                if morph is not None and not hasattr(eng, "set_morph"):
                    continue
                if hasattr(eng, "set_morph"):
                    eng.set_morph(None if morph is None else [morph])
                fn = lambda: eng.segment_tiled_raw16_multi(big, 32, cap_points=1 << 16, cap_contours=256, want_norm=False, raw_arrays=True)
                doc[f"tiled2048x1536.{name}"] = measure(eng, fn, 1)
        eng.close()
    print(json.dumps(doc))


def run_child(tree, a):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--batch", str(a.batch), "--calls", str(a.calls),
                        "--warmup", str(a.warmup), "--rounds", str(a.rounds)] + ([] if a.tiled else ["--no-tiled"]),
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"child for {tree} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with libmiunet.so built")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-tiled", dest="tiled", action="store_false", help="skip the 2048 x 1536 tiled call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_512x16.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    doc = {"batch": a.batch, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "targets_k3": [list(t) for t in K3],
           "settings": {n: m for n, m in SETTINGS}}
    if a.parent:
        doc["parent_before"] = run_child(a.parent, a)
    doc["this_tree"] = run_child(ROOT, a)
    if a.parent:
        doc["parent_after"] = run_child(a.parent, a)
    print("| side | case | POSTPROCESS ms (spread) | over the default | whole call ms (spread) | images / s |")
    print("|---|---|---|---|---|---|")
    for side in ("parent_before", "this_tree", "parent_after"):
        rows = doc.get(side, {})
        for key, s in rows.items():
            base = rows.get(key.split(".")[0] + ".default")
            extra = f"{s['postprocess_ms'] - base['postprocess_ms']:+.3f}" if base and base is not s else ""
            print(f"| {side} | {key} | {s['postprocess_ms']:.3f} ({100 * s['postprocess_spread']:.1f} %) | {extra} | {s['call_ms']:.3f} "
                  f"({100 * s['call_spread']:.1f} %) | {s['images_per_s']:.0f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
