"""What an engine handle owns: the assembly kernels' code objects (loaded at create, shared with clones, unloaded with the last handle
that holds them) and the environment switches it parsed at create.  libmiunet.so keeps nothing of either per process, so engines
made under different settings live side by side in one process."""
import contextlib
import os
import tempfile

import numpy as np
import pytest

import oracle_lib as orc
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights

pytestmark = pytest.mark.gpu

# 64 x 64, base 64, 2 levels: with MIUNET_WINO4_MIN_WG=1 and MIUNET_WINO4S=2 every 3x3 layer of a batch of 2 is on the F(4x4,3x3)
# family, down1.c1 (64 -> 128 at 32 x 32) on conv3x3_wino4a and up2.c1 (128 -> 64 at 64 x 64) on conv3x3_wino4b
SPEC = UNetSpec(1, 64, 2, 3)
ASM = ("conv3x3_wino4a", "conv3x3_wino4b")


@pytest.fixture(scope="module")
def net():
    blob = pack_weights(SPEC, synth.make_weights(SPEC, 1234))
    imgs = synth.make_images(2, 64, 64, 1, 0x5EED, "blobs")
    ref_logits, _ = orc.unet_forward(blob, imgs)
    return blob, imgs, ref_logits


def _engine(blob):
    eng = binding.Engine(64, 64, base=SPEC.base, levels=SPEC.levels, classes=SPEC.classes, max_batch=2, conv_algo="winograd")
    eng.load_weights(blob)
    return eng


def _kernels(eng, imgs):
    """layer name -> kernel name of a batch of `imgs`, from the launch log (mi_unet_get_kernel_stats).  Engine.layers() lists the steps;
    which kernel a step gets depends on the batch, so the name is only known per launch."""
    eng.set_profiling(True)
    eng.infer(imgs)
    stats = eng.kernel_stats()
    eng.set_profiling(False)
    assert {s["name"] for s in stats} <= {l["name"] for l in eng.layers()}
    return {s["name"]: s["kernel"] for s in stats}


def test_assembly_kernels_follow_the_engine_lifetime(net, monkeypatch):
    blob, imgs, ref_logits = net
    monkeypatch.setenv("MIUNET_WINO4_MIN_WG", "1")
    monkeypatch.setenv("MIUNET_WINO4S", "2")
    a = _engine(blob)
    kernels = _kernels(a, imgs)
    assert kernels["down1.c1"] == "conv3x3_wino4a" and kernels["up2.c1"] == "conv3x3_wino4b", kernels
    assert "assembly kernels not available" not in a.numeric_guard()[0]
    runs = [a.infer(imgs, want_logits=True)]
    b = a.clone()                        # shares A's code objects ...
    a.close()                            # ... and keeps them when A goes
    runs.append(b.infer(imgs, want_logits=True))
    b.close()                            # the last holder: unloaded
    c = _engine(blob)                    # loaded again
    runs.append(c.infer(imgs, want_logits=True))
    assert _kernels(c, imgs) == kernels
    c.close()
    for labels, logits in runs[1:]:
        assert np.array_equal(labels, runs[0][0]) and np.array_equal(logits, runs[0][1])
    err = float(np.max(np.abs(runs[0][1] - ref_logits)))
    print(f"max |logit - oracle| = {err:.3e}")
    assert err < 1e-3                    # the fp32 bar (tests/test_gpu_product_build.py)


def test_wino4_asm_switch_is_per_engine_and_reaches_the_hipcc_kernels(net, monkeypatch):
    """MIUNET_WINO4_ASM=0 -- and so a handle whose code objects did not load, which is told the same way -- names neither assembly
    kernel and keeps the same layers on the hipcc F(4x4,3x3) kernels; an engine made before the variable was set is not touched."""
    blob, imgs, ref_logits = net
    monkeypatch.setenv("MIUNET_WINO4_MIN_WG", "1")
    monkeypatch.setenv("MIUNET_WINO4S", "2")
    with _engine(blob) as with_asm:
        monkeypatch.setenv("MIUNET_WINO4_ASM", "0")
        with _engine(blob) as without:
            k1, k0 = _kernels(with_asm, imgs), _kernels(without, imgs)
            l1, g1 = with_asm.infer(imgs, want_logits=True)
            l0, g0 = without.infer(imgs, want_logits=True)
    assert "conv3x3_wino4a" in k1.values() and "conv3x3_wino4b" in k1.values(), k1
    assert not set(ASM) & set(k0.values()), k0
    assert k0.keys() == k1.keys()
    for name, kern in k1.items():
        if kern in ASM:
            assert k0[name] in ("conv3x3_wino4", "conv3x3_wino4s"), (name, k0[name])
        else:
            assert k0[name] == kern, (name, kern, k0[name])
    # the same algorithm on other kernels: both inside the fp32 bar
    assert float(np.max(np.abs(g1 - ref_logits))) < 1e-3 and float(np.max(np.abs(g0 - ref_logits))) < 1e-3


@contextlib.contextmanager
def _stderr_to(path):
    """fd 2 of this process (the library's fprintf(stderr)) into a file"""
    keep = os.dup(2)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        os.dup2(fd, 2)
        yield
    finally:
        os.dup2(keep, 2)
        os.close(fd)
        os.close(keep)


def test_raw_pipeline_switches_are_per_engine(monkeypatch):
    """Three engines in one process: MIUNET_RAW_SPLIT=0 + MIUNET_RAW_TRACE=1, MIUNET_RAW_TRACE=1 alone, and neither.  All give the same
    masks and contours; the traced timelines show one micro-batch under RAW_SPLIT=0 and the default cut (4 + 4 of 8 images) without,
    and the third engine traces nothing -- each handle kept what it parsed at create."""
    spec = UNetSpec(1, 32, 2, 3)
    blob = pack_weights(spec, synth.make_threshold_weights(spec))
    raws = [synth.make_raw16(64, 64, seed=500 + i) for i in range(8)]

    def engine():
        eng = binding.Engine(64, 64, base=spec.base, levels=spec.levels, classes=spec.classes, max_batch=8)
        eng.load_weights(blob)
        return eng

    monkeypatch.setenv("MIUNET_RAW_TRACE", "1")
    monkeypatch.setenv("MIUNET_RAW_SPLIT", "0")
    whole = engine()
    monkeypatch.delenv("MIUNET_RAW_SPLIT")
    cut = engine()
    monkeypatch.delenv("MIUNET_RAW_TRACE")
    quiet = engine()
    out, trace = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, eng in (("whole", whole), ("cut", cut), ("quiet", quiet)):
            path = os.path.join(tmp, name)
            with _stderr_to(path):
                out[name] = eng.segment_raw16(raws)
            trace[name] = open(path).read()
            eng.close()
    tiles, masks, cont = out["whole"]
    assert masks.any() and any(cont)
    for name in ("cut", "quiet"):
        assert np.array_equal(out[name][0], tiles) and np.array_equal(out[name][1], masks) and out[name][2] == cont, name
    enq = {name: [ln for ln in t.splitlines() if "enqueued" in ln] for name, t in trace.items()}
    assert len(enq["whole"]) == 1 and len(enq["cut"]) == 2 and "[raw" not in trace["quiet"], trace
