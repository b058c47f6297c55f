"""The device-buffer entry point (mi_unet_infer_u8_device with mi_unet_set_stream, mi_unet_sync and the timer) on caller-owned device
buffers and the caller's own streams, through its eager, capturing and replaying calls: the path bench.py times and INTEGRATION.md
tells a PyTorch host to use.  The layer kernels have their own files; this one is about the dispatch in front of them -- micro-batch
pointer offsets, ordering on the caller's stream, graph keys, the cache's eviction, stream switches (include/mi_unet.h states the
contract, DESIGN.md 5.2 the design).

Every comparison is bit identity with the host form (Engine.infer) of an engine that never captures (MIUNET_GRAPH=0) -- both forms
walk the same micro-batches, so that holds with split-K on as well -- except the one anchor to the C oracle, which uses check_parity
of tests/test_gpu_unet.py.  Device tensors and streams are torch's; every buffer the engine is given lies inside a larger allocation,
at an address that is 16-byte but not 256-byte aligned, between canaries."""
from collections import namedtuple

import numpy as np
import pytest

import oracle_lib as orc
import splitk_ref as kr
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights
from test_gpu_unet import check_parity

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EARG, ESTATE = 1, 5                       # include/mi_unet.h
MARGIN = 4096                             # canary bytes on each side of a buffer, at least
CANARY = 0xA5                             # ... and what the buffer itself holds before a call: no label of a 3-class net

LP_ENV = {"MIUNET_LPR": "2", "MIUNET_LP2": "2", "MIUNET_LPRK": "2", "MIUNET_CONVT_LPR": "2"}
# must: for every entry, a kernel whose reported name contains one of its alternatives ran in the profiled call of profile_B images
Plan = namedtuple("Plan", "id env algo spec H W profile_B must")
PLANS = [
    Plan("fp32", {}, "auto", UNetSpec(1, 32, 3, 3), 80, 72, 2, [("conv3x3_wino",), ("convT2x2",)]),
    # F(4x4) forced onto small grids, its one-block layers onto the staged kernel: both assembly kernels (code objects, launched through
    # the module API) and the fused first layer and head.  96 x 64: down1.c1 (64 -> 128 at 48 x 32, whole 16 x 16 tiles, too few K
    # chunks to split) is the two-block assembly kernel's, up2.c1 (128 -> 64 at 96 x 64, whole 16 x 32 blocks) its sibling's
    Plan("fp32-wino4", {"MIUNET_WINO4_MIN_WG": "1", "MIUNET_WINO4S": "2"}, "auto", UNetSpec(1, 64, 2, 3), 96, 64, 2,
         [("conv3x3_wino4a",), ("conv3x3_wino4b",), ("+first",), ("+head",)]),
    # batch 1, base 64: the second level's 128 -> 256 convolution leaves 4 workgroups, and K is cut (asserted from splitk_ref below)
    Plan("fp32-splitk", {}, "auto", UNetSpec(1, 64, 2, 3), 64, 64, 1, [("conv3x3_wino",)]),
    # the persistent 16-bit kernels whatever the grid: resident weights, the wide tile, the K-split 128 -> 64, the transposed conv
    Plan("bf16", LP_ENV, "bf16", UNetSpec(1, 64, 2, 3), 96, 80, 2, [("conv3x3_bf16r",), ("conv3x3_bf16w",), ("conv3x3_bf16k",), ("convT2x2_bf16r",)]),
    Plan("fp16", LP_ENV, "fp16", UNetSpec(3, 32, 3, 3), 96, 80, 2,
         [("conv3x3_fp16r",), ("conv3x3_fp16w",), ("conv3x3_fp16k",), ("convT2x2_fp16r",), ("fp16r+first",), ("fp16r+head",)]),
    Plan("bilinear", {}, "auto", UNetSpec(1, 16, 3, 3, up="bilinear"), 64, 64, 2, [("upsample",), ("conv3x3_wino",)]),
]
BY_ID = {p.id: p for p in PLANS}


@pytest.fixture(params=PLANS, ids=[p.id for p in PLANS])
def plan(request):
    return request.param


@pytest.fixture(params=[BY_ID["fp32"], BY_ID["fp32-wino4"], BY_ID["bf16"]], ids=["fp32", "fp32-wino4", "bf16"])
def plan3(request):
    """the cases about streams and keys rather than kernels: the default plan, the assembly one, a 16-bit one"""
    return request.param


# ---------------------------------------------------------------------------------------------------------------- shared pieces
_BLOBS, _IMAGES, _HOST = {}, {}, {}


def _blob(p):
    if p.id not in _BLOBS:
        _BLOBS[p.id] = pack_weights(p.spec, synth.make_weights(p.spec, 4242))
    return _BLOBS[p.id]


def _images(p, n, seed):
    key = (p.id, n, seed)
    if key not in _IMAGES:
        a = synth.make_images(n, p.H, p.W, p.spec.in_ch, seed, "blobs")
        a.setflags(write=False)
        _IMAGES[key] = a
    return _IMAGES[key]


def _engine(p, monkeypatch, max_batch, graph=True, weights=True):
    """environment switches are read at create"""
    for k, v in p.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MIUNET_GRAPH", "1" if graph else "0")
    s = p.spec
    eng = binding.Engine(p.H, p.W, in_ch=s.in_ch, base=s.base, levels=s.levels, classes=s.classes, max_batch=max_batch, conv_algo=p.algo)
    if weights:
        eng.load_weights(_blob(p))
    return eng


def _host(p, monkeypatch, max_batch, n, seed, B=None):
    """(labels, logits) of the host form on images [:B] of _images(p, n, seed), from an engine that never captures a graph; computed
    once per key, read-only"""
    B = n if B is None else B
    key = (p.id, max_batch, n, seed, B)
    if key not in _HOST:
        with _engine(p, monkeypatch, max_batch, graph=False) as eng:
            labels, logits = eng.infer(_images(p, n, seed)[:B], want_logits=True)
        assert not np.isnan(logits).any() and labels.max() < p.spec.classes
        labels.setflags(write=False)
        logits.setflags(write=False)
        _HOST[key] = (labels, logits)
    return _HOST[key]


class Arena:
    """`nbytes` of device memory at an address = 16 mod 256, inside a larger allocation filled with CANARY"""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes + 2 * MARGIN + 512,), CANARY, dtype=torch.uint8, device="cuda")
        self.off = MARGIN + (16 - (self.buf.data_ptr() + MARGIN)) % 256
        self.n = nbytes
        assert self.ptr % 256 == 16 and self.off >= MARGIN and len(self.buf) - self.off - nbytes >= MARGIN

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def bytes(self, lo=0, hi=None):
        return self.buf[self.off + lo: self.off + (self.n if hi is None else hi)]

    def wipe(self):
        self.bytes().fill_(CANARY)

    def intact(self):
        return bool((self.buf[: self.off] == CANARY).all()) and bool((self.buf[self.off + self.n:] == CANARY).all())


class DevIO:
    """the three buffers of a device call for up to `n` images of plan `p`.  torch works on its default stream here and the engine on
    another, so every method that touches the buffers ends (put, wipe) or begins (the caller's eng.sync() / stream.synchronize())
    with a host synchronisation."""

    def __init__(self, p, n):
        self.p, self.n = p, n
        self.img_bytes, self.lab_bytes, self.log_bytes = p.H * p.W * p.spec.in_ch, p.H * p.W, p.spec.classes * p.H * p.W * 4
        self.img, self.lab, self.log = Arena(n * self.img_bytes), Arena(n * self.lab_bytes), Arena(n * self.log_bytes)
        self.held = None
        torch.cuda.synchronize()

    def put(self, imgs):
        self.held = np.ascontiguousarray(imgs).reshape(-1)
        self.img.bytes(0, self.held.size).copy_(torch.from_numpy(self.held.copy()))
        torch.cuda.synchronize()
        return self

    def wipe(self):
        self.lab.wipe()
        self.log.wipe()
        torch.cuda.synchronize()

    def args(self, B, logits=True, first=0):
        """infer_device's arguments for images [first, first + B)"""
        return (self.img.ptr + first * self.img_bytes, B, self.lab.ptr + first * self.lab_bytes,
                self.log.ptr + first * self.log_bytes if logits else 0)

    def labels(self, B, first=0):
        p = self.p
        return self.lab.bytes(first * self.lab_bytes, (first + B) * self.lab_bytes).cpu().numpy().reshape(B, p.H, p.W)

    def logits(self, B, first=0):
        p = self.p
        raw = self.log.bytes(first * self.log_bytes, (first + B) * self.log_bytes).cpu().numpy()
        return raw.view(np.float32).reshape(B, p.spec.classes, p.H, p.W)

    def untouched_outside(self, B, logits=True, first=0):
        """canaries intact, the images as they were put, and nothing written outside the slices of images [first, first + B)"""
        ok = self.img.intact() and self.lab.intact() and self.log.intact()
        ok = ok and np.array_equal(self.img.bytes(0, self.held.size).cpu().numpy(), self.held)
        for arena, per, used in ((self.lab, self.lab_bytes, True), (self.log, self.log_bytes, logits)):
            lo, hi = (first * per, (first + B) * per) if used else (0, 0)
            ok = ok and bool((arena.bytes(0, lo) == CANARY).all()) and bool((arena.bytes(hi) == CANARY).all())
        return ok


def _same(io, B, want, what, logits=True, first=0):
    """the device buffers hold exactly `want` = (labels, logits) of the host form"""
    assert np.array_equal(io.labels(B, first), want[0]), what
    if logits:
        assert np.array_equal(io.logits(B, first).view(np.uint32), want[1].view(np.uint32)), what


def _pinned(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8).pin_memory()


# ------------------------------------------------------------------------------------------------------------- the plans' routing
def test_each_plan_contains_the_kernels_it_is_there_for(plan, monkeypatch):
    """One profiled (hence eager) device call per plan: the kernel families the plan was chosen for ran, at the batch the other cases
    replay.  Routing is a function of the plan and the micro-batch size alone, so the same launches are inside the captured graphs."""
    p = plan
    B = p.profile_B
    io = DevIO(p, B).put(_images(p, 5, 11)[:B])
    with _engine(p, monkeypatch, max_batch=2) as eng:
        eng.set_profiling(True)
        eng.infer_device(*io.args(B))
        eng.sync()
        stats = eng.kernel_stats()
        layers = {l["name"]: l for l in eng.layers()}
    kernels = [s["kernel"] for s in stats]
    print(f"\n  {p.id} B={B}: " + " ".join(f"{s['name']}={s['kernel']}" for s in stats))
    for alts in p.must:
        assert any(a in k for a in alts for k in kernels), (p.id, alts, kernels)
    _same(io, B, _host(p, monkeypatch, 2, 5, 11, B), p.id)
    if p.id == "fp32-splitk":
        # The statistics do not say how many slices a launch was cut into.  As in tests/test_gpu_insitu.py: the two hipcc Winograd
        # launchers ask csrc/routing.cpp, tests/test_splitk_cpu.py holds that against the model of tests/splitk_ref.py, and the model is
        # applied here to the shapes of the layers that ran on those two kernels (fused and staged ones never split).
        split = {}
        for s in stats:
            fam = {"conv3x3_wino4": kr.F4, "conv3x3_wino": kr.F2}.get(s["kernel"])
            l = layers.get(s["name"])
            if fam and l and l["kind"] == "conv3x3":
                split[s["name"]] = kr.layer(fam, (B, l["in_h"], l["in_w"], l["in_c"], l["out_c"])).ks
        print(f"  slices by the model: {split}")
        assert any(ks > 1 for ks in split.values()), split


# ------------------------------------------------------------------------------------------------ (a) device form = host form, (b)
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_device_form_equals_host_form_and_writes_only_its_slice(plan, B, monkeypatch):
    """a + b: B = 1, max_batch, max_batch + 1, 2 * max_batch + 1 at max_batch 2; three calls each (eager, capturing, replaying), with
    and without logits, the outputs wiped in between; the slice of a 5-image buffer that starts at image 5 - B, so that every
    micro-batch pointer is an offset from an offset; canaries, the images and the rest of the buffers unchanged"""
    p = plan
    imgs = _images(p, 5, 11)
    first = 5 - B
    io = DevIO(p, 5).put(imgs)
    with _engine(p, monkeypatch, max_batch=2) as eng:
        host = eng.infer(imgs[first:], want_logits=True)               # the same engine's host form
        for logits in (True, False):
            for call in ("eager", "capture", "replay"):
                io.wipe()
                eng.infer_device(*io.args(B, logits, first))
                eng.sync()
                _same(io, B, host, (p.id, B, logits, call), logits, first)
                assert io.untouched_outside(B, logits, first), (p.id, B, logits, call)
    want = _host(p, monkeypatch, 2, 5, 11) if B == 5 else None        # ... and, for the whole buffer, the engine that never captures
    if want is not None:
        assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1])


def test_device_form_against_the_oracle(monkeypatch):
    """the anchor outside the library: the default fp32 plan's device form, replayed, against the C oracle on the bar of test_gpu_unet"""
    p = BY_ID["fp32"]
    imgs = _images(p, 5, 11)[:3]
    ref_logits, ref_labels = orc.unet_forward(_blob(p), imgs)
    io = DevIO(p, 3).put(imgs)
    with _engine(p, monkeypatch, max_batch=2) as eng:
        for _ in range(3):
            io.wipe()
            eng.infer_device(*io.args(3))
        eng.sync()
    check_parity(io.labels(3), io.logits(3), ref_logits, ref_labels)


# ------------------------------------------------------------------------------------------------------- (c) eager, capture, replay
def test_replay_follows_the_buffer_contents(plan, monkeypatch):
    """c: four calls on one key, then two more after the images were overwritten in place: a graph bakes in addresses, not contents"""
    p = plan
    a, b = _images(p, 3, 21), _images(p, 3, 22)
    want = {"a": _host(p, monkeypatch, 2, 3, 21), "b": _host(p, monkeypatch, 2, 3, 22)}
    assert not np.array_equal(want["a"][0], want["b"][0])
    io = DevIO(p, 3)
    with _engine(p, monkeypatch, max_batch=2) as eng:
        for k, which in enumerate("aaaabb"):
            if k in (0, 4):
                io.put(a if which == "a" else b)
            io.wipe()
            eng.infer_device(*io.args(3))
            eng.sync()
            _same(io, 3, want[which], (p.id, k))
    assert io.untouched_outside(3)


# -------------------------------------------------------------------------------------------------------------------------- (d) keys
def test_every_key_gets_its_own_graph(plan3, monkeypatch):
    """d: two image sets x two output buffers x B in {1, 2}: eight keys, interleaved so that each passes through its eager, capturing
    and replaying call with the others in between; profiling toggled in the middle (eager, then back to the cached graphs) and the
    same weights loaded again (the cache starts over)"""
    p = plan3
    sets = [DevIO(p, 2).put(_images(p, 2, 31 + i)) for i in range(2)]
    outs = [DevIO(p, 2) for _ in range(2)]
    want = {(i, B): _host(p, monkeypatch, 2, 2, 31 + i, B) for i in range(2) for B in (1, 2)}
    keys = [(i, o, B) for i in range(2) for o in range(2) for B in (1, 2)]

    def round_(eng, tag):
        for i, o, B in keys:
            outs[o].wipe()
            eng.infer_device(sets[i].img.ptr, B, outs[o].lab.ptr, outs[o].log.ptr)
            eng.sync()
            _same(outs[o], B, want[(i, B)], (p.id, tag, i, o, B))

    with _engine(p, monkeypatch, max_batch=2) as eng:
        for r in range(3):
            round_(eng, f"round {r}")
        eng.set_profiling(True)
        round_(eng, "profiling")
        eng.set_profiling(False)
        round_(eng, "after profiling")
        eng.load_weights(_blob(p))
        for r in range(3):
            round_(eng, f"reloaded, round {r}")
    assert all(o.lab.intact() and o.log.intact() for o in outs) and all(s.img.intact() for s in sets)


# ------------------------------------------------------------------------------------- (e) ordered on the caller's stream, no host sync
@pytest.mark.parametrize("timed", [False, True], ids=["plain", "timed"])
def test_ordered_on_the_callers_stream_without_host_synchronisation(plan, timed, monkeypatch):
    """e: eight iterations of (unrelated work, async upload into the image buffer, infer_device, async download of both outputs) on a
    torch stream, nothing synchronised until the end: iteration k must give the maps of image set k & 1, so every call -- the eager,
    the capturing and six replays -- ran behind its own upload and ahead of the next.  With the timer around the loop: a positive,
    finite time."""
    p = plan
    B = 3
    want = [_host(p, monkeypatch, 2, 3, 41 + i) for i in range(2)]
    assert not np.array_equal(want[0][0], want[1][0])
    io = DevIO(p, B)
    pinned_set = [torch.from_numpy(_images(p, 3, 41 + i).reshape(-1).copy()).pin_memory() for i in range(2)]
    res_lab = [_pinned(B * io.lab_bytes) for _ in range(8)]
    res_log = [_pinned(B * io.log_bytes) for _ in range(8)]
    x = torch.randn(768, 768, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _engine(p, monkeypatch, max_batch=2) as eng:
        eng.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            if timed:
                eng.timer_begin()
            for k in range(8):
                y = x
                for _ in range(4):
                    y = (y @ x) * (1.0 / 768)
                io.img.bytes().copy_(pinned_set[k & 1], non_blocking=True)
                eng.infer_device(*io.args(B))
                res_lab[k].copy_(io.lab.bytes(), non_blocking=True)
                res_log[k].copy_(io.log.bytes(), non_blocking=True)
            if timed:
                ms = eng.timer_end()
                assert np.isfinite(ms) and ms > 0
        stream.synchronize()
        for k in range(8):
            assert np.array_equal(res_lab[k].numpy().reshape(want[0][0].shape), want[k & 1][0]), (p.id, k)
            assert np.array_equal(res_log[k].numpy().view(np.uint32).reshape(want[0][1].shape), want[k & 1][1].view(np.uint32)), (p.id, k)
    assert io.img.intact() and io.lab.intact() and io.log.intact()


# ------------------------------------------------------------------------------------------------------------- (f) stream switches
def test_stream_switches_follow_the_contract(plan3, monkeypatch):
    """f: own stream, caller's A, caller's B, A again, own again; the stream being left is synchronised before each switch
    (include/mi_unet.h).  Three calls per visit: on a first visit eager, capturing, replaying, on a return all replays of that
    stream's graphs.  mi_unet_sync returns after the current stream's work: a pinned result enqueued behind the call on that stream
    is read on the host right after it.  Then the engine is destroyed while A is alive and current."""
    p = plan3
    B = 3
    imgs = _images(p, 3, 21)
    want = _host(p, monkeypatch, 2, 3, 21)
    io = DevIO(p, B).put(imgs)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    lab, log = _pinned(B * io.lab_bytes), _pinned(B * io.log_bytes)
    eng = _engine(p, monkeypatch, max_batch=2)
    try:
        for visit, s in enumerate([None, sa, sb, sa, None, sa]):
            if visit:
                eng.sync()                                            # the caller orders the switch
                eng.set_stream(s.cuda_stream if s else 0, reset=s is None)
            for call in range(3):
                io.wipe()
                lab.fill_(CANARY)
                log.fill_(CANARY)
                eng.infer_device(*io.args(B))
                if s is None:
                    eng.sync()
                    _same(io, B, want, (p.id, visit, call))
                else:
                    with torch.cuda.stream(s):
                        lab.copy_(io.lab.bytes(), non_blocking=True)
                        log.copy_(io.log.bytes(), non_blocking=True)
                    eng.sync()                                        # ... and nothing else: the host reads the pinned copies
                    assert np.array_equal(lab.numpy().reshape(want[0].shape), want[0]), (p.id, visit, call)
                    assert np.array_equal(log.numpy().view(np.uint32).reshape(want[1].shape), want[1].view(np.uint32)), (p.id, visit, call)
        eng.sync()
        io.wipe()
        eng.infer_device(*io.args(B))                                 # in flight on A when the handle goes
    finally:
        eng.close()
    sa.synchronize()
    with torch.cuda.stream(sa):                                       # A is still a working stream
        t = torch.ones(16, device="cuda") * 2
    sa.synchronize()
    assert float(t.sum()) == 32.0
    _same(io, B, want, (p.id, "last call before destroy"))
    assert io.untouched_outside(B)


# ------------------------------------------------------------------------------------------------ (g) two contexts, two caller streams
def test_two_contexts_on_two_streams_from_one_thread(plan3, monkeypatch):
    """g: an engine and its clone, each on a torch stream of its own, ten calls each enqueued alternately with nothing synchronised in
    between, on different images; every call's outputs are copied aside on its stream.  The two forward passes overlap on the
    device and share the weights and the code objects, nothing else.  Then the source is destroyed and the clone runs on."""
    p = plan3
    B = 3
    want = [_host(p, monkeypatch, 2, 3, 41 + i) for i in range(2)]
    ios = [DevIO(p, B).put(_images(p, 3, 41 + i)) for i in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = [[(_pinned(B * ios[0].lab_bytes), _pinned(B * ios[0].log_bytes)) for _ in range(12)] for _ in range(2)]

    def call(e, k):
        engs[e].infer_device(*ios[e].args(B))
        with torch.cuda.stream(streams[e]):
            res[e][k][0].copy_(ios[e].lab.bytes(), non_blocking=True)
            res[e][k][1].copy_(ios[e].log.bytes(), non_blocking=True)

    def check(e, k):
        assert np.array_equal(res[e][k][0].numpy().reshape(want[e][0].shape), want[e][0]), (p.id, e, k)
        assert np.array_equal(res[e][k][1].numpy().view(np.uint32).reshape(want[e][1].shape), want[e][1].view(np.uint32)), (p.id, e, k)

    src = _engine(p, monkeypatch, max_batch=2)
    engs = [src, src.clone()]
    try:
        for e in range(2):
            engs[e].set_stream(streams[e].cuda_stream)
        for k in range(10):
            for e in range(2):
                call(e, k)
        for s in streams:
            s.synchronize()
        for k in range(10):
            for e in range(2):
                check(e, k)
        src.close()
        for k in (10, 11):
            call(1, k)
        streams[1].synchronize()
        for k in (10, 11):
            check(1, k)
    finally:
        for e in engs:
            e.close()
    assert all(io.untouched_outside(B) for io in ios)


# -------------------------------------------------------------------------------------------------------- (h) the cache past 64 keys
def test_cache_eviction_past_64_keys(plan, monkeypatch):
    """h: max_batch 1 and one buffer of 70 images, so one call of B = 70 is 70 keys.  Image 0 alone three times (eager, capture,
    replay); without a synchronisation a call of 70, whose first micro-batch replays image 0's graph and whose 65th evicts it while
    that replay may still be running; image 0 three more times (a fresh entry: eager, capture, replay); 70 twice more (a replay of
    image 0, then evictions again -- no other key ever replays: DESIGN.md 5.2).  The handle waits for the stream before it destroys
    an evicted executable (csrc/engine.cpp: GraphRetire)."""
    p = plan
    N = 70
    imgs = _images(p, N, 51)
    want = _host(p, monkeypatch, 1, N, 51)
    one = (want[0][:1], want[1][:1])
    io = DevIO(p, N).put(imgs)
    with _engine(p, monkeypatch, max_batch=1) as eng:
        for _ in range(3):
            eng.infer_device(*io.args(1))
        eng.infer_device(*io.args(N))                                  # no synchronisation before it
        eng.sync()
        _same(io, N, want, (p.id, "first call of 70"))
        for k in range(3):
            io.wipe()
            eng.infer_device(*io.args(1))
            eng.sync()
            _same(io, 1, one, (p.id, "image 0 again", k))
            assert io.untouched_outside(1)
        for k in range(2):
            io.wipe()
            eng.infer_device(*io.args(N))
            if k == 0:
                eng.infer_device(*io.args(1))                          # ... and straight behind it, the evicted key again
            eng.sync()
            _same(io, N, want, (p.id, "call of 70", k))
    assert io.untouched_outside(N)


# -------------------------------------------------------------------------------------------------- (i) postprocess on the device form
def test_postprocess_on_the_device_form(monkeypatch):
    """i: mi_unet_set_postprocess(1): the clean-up is enqueued behind the graph on the caller's stream, outside it.  Threshold weights
    (label maps with regions large enough to survive), B = 3 on max_batch 2, eager, capturing and replaying, on a torch stream"""
    p = BY_ID["fp32"]
    blob = pack_weights(p.spec, synth.make_threshold_weights(p.spec))
    imgs = synth.make_images(3, p.H, p.W, 1, 0x77, "blobs")
    io = DevIO(p, 3).put(imgs)
    stream = torch.cuda.Stream()
    with _engine(p, monkeypatch, max_batch=2, weights=False) as eng:
        eng.load_weights(blob)
        plain, _ = eng.infer(imgs)
        want = np.stack([orc.postprocess_mask(m) for m in plain])
        assert (want == 2).any() and not np.array_equal(want, plain), "the inputs of this test must give the clean-up something to do"
        eng.set_postprocess(True)
        eng.set_stream(stream.cuda_stream)
        for call in range(4):
            io.wipe()
            eng.infer_device(*io.args(3))
            eng.sync()
            assert np.array_equal(io.labels(3), want), call
        eng.sync()
        eng.set_stream(0, reset=True)
        post_host, _ = eng.infer(imgs)
        assert np.array_equal(post_host, want)
    assert io.untouched_outside(3)


# ------------------------------------------------------------------------------------------------------------------- (j) refusals
def test_refusals_leave_the_handle_and_the_buffers_alone(monkeypatch):
    """j: null pointers and B < 0 are MI_UNET_EARG, a call before the weights MI_UNET_ESTATE, B = 0 a success that enqueues nothing; after
    each the handle still gives the right result and nothing was written"""
    p = BY_ID["fp32"]
    imgs = _images(p, 3, 21)
    want = _host(p, monkeypatch, 2, 3, 21)
    io = DevIO(p, 3).put(imgs)
    img, B, lab, log = io.args(3)

    def refused(eng, code, *args):
        with pytest.raises(binding.MiUnetError) as ei:
            eng.infer_device(*args)
        assert ei.value.code == code, (args, str(ei.value))
        eng.sync()
        assert io.untouched_outside(0)                                # nothing at all was written

    with _engine(p, monkeypatch, max_batch=2, weights=False) as eng:
        refused(eng, ESTATE, img, B, lab, log)
        eng.load_weights(_blob(p))
        for bad in ((0, B, lab, log), (img, B, 0, log), (img, -1, lab, log), (0, 0, 0, 0)):
            io.wipe()
            refused(eng, EARG, *bad)
            eng.infer_device(img, 0, lab, log)                        # B = 0
            eng.sync()
            assert io.untouched_outside(0)
            for _ in range(2):
                io.wipe()
                eng.infer_device(img, B, lab, log)
                eng.sync()
                _same(io, 3, want, bad)
    assert io.untouched_outside(3)
