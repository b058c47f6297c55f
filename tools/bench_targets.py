#!/usr/bin/env python3
"""What K targets cost behind the network (mi_unet_set_targets), on one GPU.  Not the headline metric (bench.py).

The default engine (512 x 512, base 64, 4 levels, 3 classes, max_batch 16) on 16 RAW images: MI_UNET_STAGE_POSTPROCESS and
MI_UNET_STAGE_CONTOURS (mi_unet_last_stage_ms, device time) of
  (a) mi_unet_segment_raw16 of the parent commit, from a separate checkout whose libmiunet.so is built (--parent), in a child
      process of its own; without --parent, of this tree (the same entry point, which this feature does not touch);
  (b) mi_unet_segment_raw16_multi of this tree with K = 1 .. 5 targets.  A 3-class network has two foreground classes, so the
      network of (b) has 6 classes (the tail reads label maps only; the class count does not enter its cost) and the threshold
      weights of the tests, extended so that every class owns a band of grey levels.
"K separate tails" is K x (a): what K host-driven passes of the single-target tail would cost.  Each of --rounds rounds runs (a) and
every K in turn, --calls calls each after a warm-up, so slow drifts of the card reach all alike; medians are reported.  Writes one
JSON document (--out, default profiles/targets_512x16.json) and prints the table of DESIGN.md 7.4.

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/unet-medical-image-contour-segmentation-cpp_amd libmiunet.so
    python tools/bench_targets.py --parent /tmp/parent"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_REL = "unet-medical-image-contour-segmentation-cpp_amd"
FRACS = [0.06, 0.01, 0.03, 0.002, 0.0]


def weights(synth, spec):
    """miunet.synth.make_threshold_weights for any class count: class c owns the grey levels between two cuts"""
    t = synth.make_threshold_weights(spec)
    cuts = [(40.5 + 200.0 * (j + 1) / spec.classes) / 255.0 for j in range(spec.classes - 1)]
    t["outc.w"][:] = 0
    t["outc.b"][:] = 0
    for c in range(spec.classes):
        t["outc.w"][c, 0] = float(c)
        t["outc.b"][c] = -float(sum(cuts[:c]))
    return t


def setup(pkg_root, classes, batch):
    sys.path.insert(0, os.path.join(pkg_root, PKG_REL))
    from miunet import binding, synth
    from miunet.spec import UNetSpec, pack_weights
    spec = UNetSpec(classes=classes)
    eng = binding.Engine(classes=classes, max_batch=batch)
    eng.load_weights(pack_weights(spec, weights(synth, spec)))
    raws = [synth.make_raw16(1536, 2048, seed=21 + i) for i in range(batch)]
    return binding, eng, raws


def tail_ms(eng, run, p, n):
    out = []
    for _ in range(n):
        run(p)
        st = eng.last_stage_ms()
        out.append((st["postprocess"], st["contours"]))
    return out


def single_side(pkg_root, a):
    """(a): warm-up, then --rounds x --calls calls of the single-target entry point"""
    binding, eng, raws = setup(pkg_root, 3, a.batch)
    p = eng.segment_raw16_prepare(raws, cap_points=1 << 15, cap_contours=64)
    tail_ms(eng, eng.segment_raw16_run, p, a.warmup)
    return [tail_ms(eng, eng.segment_raw16_run, p, a.calls) for _ in range(a.rounds)]


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with libmiunet.so built")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_512x16.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(single_side(a.parent, a)))
        return
    if a.parent:                                             # a fresh process: the parent's library and binding, nothing of this tree
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", a.parent, "--batch", str(a.batch), "--rounds",
                            str(a.rounds), "--calls", str(a.calls), "--warmup", str(a.warmup)], capture_output=True, text=True, check=True)
        single = json.loads(r.stdout.strip().splitlines()[-1])
    else:
        single = None
    binding, eng, raws = setup(ROOT, 6, a.batch)
    own = None
    if single is None:
        _, eng3, raws3 = setup(ROOT, 3, a.batch)
        p3 = eng3.segment_raw16_prepare(raws3, cap_points=1 << 15, cap_contours=64)
        tail_ms(eng3, eng3.segment_raw16_run, p3, a.warmup)
        own = []
    multi = {k: [] for k in range(1, 6)}
    for _ in range(a.rounds):
        if own is not None:
            own.append(tail_ms(eng3, eng3.segment_raw16_run, p3, a.calls))
        for k in range(1, 6):
            eng.set_targets([(5 - j, FRACS[j]) for j in range(k)])
            p = eng.segment_raw16_multi_prepare(raws, cap_points=1 << 15, cap_contours=64)
            tail_ms(eng, eng.segment_raw16_multi_run, p, 1)
            multi[k] += tail_ms(eng, eng.segment_raw16_multi_run, p, a.calls)
    single = [x for r in (single if single is not None else own) for x in r]
    s_pp, s_ct = median([x[0] for x in single]), median([x[1] for x in single])
    rows = []
    print(f"single-target tail ({'parent commit' if a.parent else 'this tree'}): postprocess {s_pp:.3f} ms, contours {s_ct:.3f} ms, "
          f"sum {s_pp + s_ct:.3f} ms  ({a.batch} images of 512 x 512)")
    print("| K | postprocess (ms) | contours (ms) | sum (ms) | K separate tails (ms) | ratio |")
    print("|---|---|---|---|---|---|")
    for k in range(1, 6):
        pp, ct = median([x[0] for x in multi[k]]), median([x[1] for x in multi[k]])
        sep = k * (s_pp + s_ct)
        rows.append({"K": k, "postprocess_ms": pp, "contours_ms": ct, "sum_ms": pp + ct, "k_separate_tails_ms": sep, "ratio": (pp + ct) / sep})
        print(f"| {k} | {pp:.3f} | {ct:.3f} | {pp + ct:.3f} | {sep:.3f} | {(pp + ct) / sep:.2f} |")
    doc = {"batch": a.batch, "rounds": a.rounds, "calls": a.calls, "single_from": "parent" if a.parent else "this tree",
           "single_postprocess_ms": s_pp, "single_contours_ms": s_ct, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
