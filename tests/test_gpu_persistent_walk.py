"""The tile walk of the six persistent kernels on tile counts their grid does not divide (the model and the case tables:
tests/persist_ref.py, checked by tests/test_persist_cpu.py).

Capped sweep: MIUNET_CUS lowers the persistent grid to 8, 9, 12, 16 or 23 workgroups, so a few dozen tiles walk the partition that
thousands walk on the whole chip: nwg & 7 != 0, workgroups of one launch with different tile counts (one past the deepest ring next to
fewer than its depth), walks that cross a channel group, grids that are no multiple of 8.  That exercises the LOGIC of the walk; only
the production-grid cases (no cap, a few tiles more than compute units) run it at one workgroup per CU.  Per case:

  nothing unwritten  no poison left in the slice (an unvisited tile);
  nothing stray      the run is in a strided layout (ldo = Cout + 32, co_off = 16) between 4096-byte guards, tests/slice_ref.py finds
                     no touched element outside the slice (a tile decoded past the end of its range);
  right              fp32 kernels against the oracle at 1e-4 * max(1, max|ref|) with a per-channel scale and shift of order one (a
                     stale bias or U slice of the previous channel group is of order one too); 16-bit kernels at the bars of
                     test_gpu_bf16.py: within one 16-bit rounding of the rounded-operand oracle, bit-equal to the one-tile-per-workgroup
                     kernel (conv_lprk: within one ulp of it at under 0.5 % of the elements);
  schedule-independent  the same call without the cap (grid = nwg, one tile per workgroup) leaves the same bytes in the whole
                     allocation: one workgroup forms a tile's sums in a fixed order, whichever tiles it took before.

Every run prints one line `walk: <kernel> <op> <shape> cus <n> nwg <n> tiles/wg <lo>-<hi> crossing <n> err <e>`: what ran."""
import functools

import numpy as np
import pytest

import oracle_lib as orc
import persist_ref as pr
import slice_ref
from miunet import binding, synth
from miunet.spec import UNetSpec, pack_weights

pytestmark = pytest.mark.gpu

GUARD = 4096
FP32_OP = {"wino4a": "conv3x3_wino4a", "wino4b": "conv3x3_wino4b", "wino4_1b": "conv3x3_wino4"}
FP32_ROUTE = {"wino4a": "conv3x3_wino4a", "wino4b": "conv3x3_wino4b", "wino4_1b": "conv3x3_wino4"}


@functools.lru_cache(maxsize=None)
def _device_cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _layout(Cout, pooled):
    lay = {"ldo": Cout + 32, "co_off": 16, "guard_bytes": GUARD}
    if pooled:
        lay["pool_ld"] = Cout + 32
    return lay


def _kind(op):
    return 1 if "_bf16" in op else 2 if "_fp16" in op else 0


def _slice(res, which, op, what):
    """nothing stray, nothing unwritten in one returned allocation; the dense slice"""
    shape, c, ld, co_off, guard = res[which + "_layout"]
    kind = _kind(op) if res["elem_bytes"] == 2 else 0
    s = slice_ref.check(res[which], res["elem_bytes"], shape, c, ld, co_off, guard, kind, limit=6)
    assert s.n_strays == 0, f"{what}: the {which} tensor: " + slice_ref.describe(s.strays, s.n_strays, s.summary)
    assert s.unwritten == 0, f"{what}: {s.unwritten} elements of the {which} slice are still poison (an unvisited tile)"
    assert not np.isnan(s.dense).any(), what
    return s.dense


def _run(op, operands, relu, lay, cus, monkeypatch):
    """one strided run of the hook under MIUNET_CUS = cus (None: not set)"""
    if cus is None:
        monkeypatch.delenv("MIUNET_CUS", raising=False)
    else:
        monkeypatch.setenv("MIUNET_CUS", str(cus))
    x, w, scale, shift = operands
    return binding.layer_debug_strided(op, x, w, scale, shift, relu=relu, **lay)


def _same_bytes(a, b, what):
    assert np.array_equal(a["out"], b["out"]), what + ": the output allocation depends on the schedule"
    if a["pool"] is not None:
        assert np.array_equal(a["pool"], b["pool"]), what + ": the pooled allocation depends on the schedule"


def _say(kernel, op, shape, cus, err):
    p = pr.props(kernel, shape, cus)
    print(f"walk: {kernel} {op} {shape} cus {cus} nwg {p.nwg} tiles/wg {p.per_wg[0]}-{p.per_wg[-1]} crossing {p.crossing} err {err:.3e}")


# ------------------------------------------------------------------------------------------ operands and references, computed once
@functools.lru_cache(maxsize=None)
def _conv_fp32(shape):
    B, H, W, Cin, Cout = shape
    r = np.random.default_rng([B, H, W, Cin, Cout])
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = r.uniform(0.5, 2.0, Cout).astype(np.float32)             # per channel, of order one: the previous group's would show
    shift = r.standard_normal(Cout).astype(np.float32)
    ref = np.maximum(orc.conv3x3(x, w) * scale + shift, 0.0)
    return _frozen(x, w, scale, shift, ref)


@functools.lru_cache(maxsize=None)
def _conv_lp(shape, t):
    B, H, W, Cin, Cout = shape
    r = np.random.default_rng([B, H, W, Cin, Cout, 16])
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cout, Cin, 3, 3), dtype=np.float32) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    scale = (1.0 + 0.1 * r.standard_normal(Cout)).astype(np.float32)
    shift = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    rnd = orc.bf16_round if t == "bf16" else orc.fp16_round
    wf = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None]).astype(np.float32)    # the packing folds the scale first
    ref = np.maximum(orc.conv3x3(rnd(x), rnd(wf)) + shift, 0.0)
    return _frozen(x, w, scale, shift, ref)


@functools.lru_cache(maxsize=None)
def _convT_lp(shape, t):
    B, H, W, Cin, Cout = shape
    r = np.random.default_rng([B, H, W, Cin, Cout, 17])
    x = r.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (r.standard_normal((Cin, Cout, 2, 2), dtype=np.float32) / np.sqrt(Cin)).astype(np.float32)
    bias = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    rnd = orc.bf16_round if t == "bf16" else orc.fp16_round
    ref = orc.convT2x2(rnd(x), rnd(w), bias)
    return _frozen(x, w, bias, ref)


def _bar_fp32(got, ref, what):
    err = float(np.max(np.abs(got - ref)))
    assert err < 1e-4 * max(1.0, float(np.abs(ref).max())), (what, err)
    return err


def _bar_lp(got, ref, t, what):
    ulp = 2.0 ** -7 if t == "bf16" else 2.0 ** -10
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    assert err < ulp, (what, err)
    return err


# ------------------------------------------------------------------------------------------ one case of each family
def _fp32_case(kernel, shape, cus_a, cus_b, pooled, monkeypatch):
    """the F(4x4,3x3) kernel under MIUNET_CUS = cus_a (None: the device's grid), all four assertions; the schedule check against cus_b"""
    if kernel == "wino4_1b":
        monkeypatch.setenv("MIUNET_WINO4S", "0")         # the persistent one-block hipcc kernel instead of the staged one
    op = FP32_OP[kernel] + ("_pool" if pooled else "")
    x, w, scale, shift, ref = _conv_fp32(shape)
    lay = _layout(shape[4], pooled)
    what = f"{op} {shape} MIUNET_CUS={cus_a}"
    a = _run(op, (x, w, scale, shift), True, lay, cus_a, monkeypatch)
    assert a["kernel"] == FP32_ROUTE[kernel], (what, a["kernel"])     # (conv3x3_wino4: the hipcc kernel, not conv3x3_wino4a / 4b / 4s)
    got = _slice(a, "out", op, what)
    err = _bar_fp32(got, ref, what)
    if pooled:
        gotp = _slice(a, "pool", op, what)
        assert np.array_equal(gotp, orc.maxpool2x2(got)), what + ": the pooled store is not the max of what was stored"
        _bar_fp32(gotp, orc.maxpool2x2(ref), what + " (pooled)")
    b = _run(op, (x, w, scale, shift), True, lay, cus_b, monkeypatch)
    assert b["kernel"] == a["kernel"]
    _same_bytes(a, b, what + f" against MIUNET_CUS={cus_b}")
    _say(kernel, op, shape, cus_a if cus_a is not None else _device_cus(), err)


def _lp_case(kernel, t, shape, cus_a, cus_b, pooled, monkeypatch):
    """conv_lpr / conv_lprk under MIUNET_CUS = cus_a: the four assertions at the bars of test_gpu_bf16.py"""
    sfx = ("_pool" if pooled else "") + "_lpout"
    op, one_tile = f"conv3x3_{t}{'r' if kernel == 'lpr' else 'k'}{sfx}", f"conv3x3_{t}{sfx}"
    x, w, scale, shift, ref = _conv_lp(shape, t)
    lay = _layout(shape[4], pooled)
    what = f"{op} {shape} MIUNET_CUS={cus_a}"
    a = _run(op, (x, w, scale, shift), True, lay, cus_a, monkeypatch)
    assert a["kernel"] == f"conv3x3_{t}{'r' if kernel == 'lpr' else 'k'}", (what, a["kernel"])
    got = _slice(a, "out", op, what)
    err = _bar_lp(got, ref, t, what)
    gotp = _slice(a, "pool", op, what) if pooled else None
    if pooled:
        assert np.array_equal(gotp, orc.maxpool2x2(got)), what + ": the pooled store is not the max of what was stored"
    b = _run(op, (x, w, scale, shift), True, lay, cus_b, monkeypatch)
    _same_bytes(a, b, what + f" against MIUNET_CUS={cus_b}")
    monkeypatch.delenv("MIUNET_CUS", raising=False)
    other = binding.layer_debug(one_tile, x, w, scale, shift, relu=True)          # (with _pool: the pooled tensor)
    mine = gotp if pooled else got
    if kernel == "lpr":
        assert np.array_equal(mine, other), what + ": differs from the one-tile-per-workgroup kernel's bits"
    else:                                     # one fp32 add associated differently: rare one-ulp straddles of a rounding boundary
        ulp = 2.0 ** -7 if t == "bf16" else 2.0 ** -10
        d = np.abs(mine - other)
        assert np.all(d <= ulp * np.maximum(np.abs(mine), np.abs(other)) + 1e-6) and float(np.mean(d > 0)) < 5e-3, what
    _say(kernel, op, shape, cus_a if cus_a is not None else _device_cus(), err)


def _convT_case(t, shape, cus_a, cus_b, monkeypatch):
    op, one_tile = f"convT2x2_{t}r_lpout", f"convT2x2_{t}_lpout"
    x, w, bias, ref = _convT_lp(shape, t)
    lay = _layout(shape[4], False)
    what = f"{op} {shape} MIUNET_CUS={cus_a}"
    a = _run(op, (x, w, None, bias), False, lay, cus_a, monkeypatch)
    assert a["kernel"] == f"convT2x2_{t}r", (what, a["kernel"])
    got = _slice(a, "out", op, what)
    err = _bar_lp(got, ref, t, what)
    b = _run(op, (x, w, None, bias), False, lay, cus_b, monkeypatch)
    _same_bytes(a, b, what + f" against MIUNET_CUS={cus_b}")
    monkeypatch.delenv("MIUNET_CUS", raising=False)
    assert np.array_equal(got, binding.layer_debug(one_tile, x, w, None, bias)), what + ": differs from the one-tile-per-workgroup kernel's bits"
    _say("convt", op, shape, cus_a if cus_a is not None else _device_cus(), err)


def _one_tile_each_without_the_cap(kernel, shape):
    assert pr.nwg_of(kernel, shape) <= _device_cus(), "without MIUNET_CUS this case was to run one tile per workgroup"


def _ids(cases):
    return ["x".join(map(str, s)) + f"-cus{c}" + ("-pool" if p else "") for s, c, p in cases]


# ------------------------------------------------------------------------------------------ the capped sweep
@pytest.mark.parametrize("shape,cap,pooled", pr.CAPPED["wino4a"], ids=_ids(pr.CAPPED["wino4a"]))
def test_capped_wino4a(shape, cap, pooled, monkeypatch):
    _one_tile_each_without_the_cap("wino4a", shape)
    _fp32_case("wino4a", shape, cap, None, pooled, monkeypatch)


@pytest.mark.parametrize("shape,cap,pooled", pr.CAPPED["wino4b"], ids=_ids(pr.CAPPED["wino4b"]))
def test_capped_wino4b(shape, cap, pooled, monkeypatch):
    _one_tile_each_without_the_cap("wino4b", shape)
    _fp32_case("wino4b", shape, cap, None, pooled, monkeypatch)


@pytest.mark.parametrize("shape,cap,pooled", pr.CAPPED["wino4_1b"], ids=_ids(pr.CAPPED["wino4_1b"]))
def test_capped_one_block_hipcc_kernel(shape, cap, pooled, monkeypatch):
    _one_tile_each_without_the_cap("wino4_1b", shape)
    _fp32_case("wino4_1b", shape, cap, None, pooled, monkeypatch)


@pytest.mark.parametrize("t", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,cap,pooled", pr.CAPPED["lpr"], ids=_ids(pr.CAPPED["lpr"]))
def test_capped_resident_weights(shape, cap, pooled, t, monkeypatch):
    _one_tile_each_without_the_cap("lpr", shape)
    _lp_case("lpr", t, shape, cap, None, pooled, monkeypatch)


@pytest.mark.parametrize("t", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,cap,pooled", pr.CAPPED["lprk"], ids=_ids(pr.CAPPED["lprk"]))
def test_capped_resident_weights_k_split(shape, cap, pooled, t, monkeypatch):
    _one_tile_each_without_the_cap("lprk", shape)
    _lp_case("lprk", t, shape, cap, None, pooled, monkeypatch)


@pytest.mark.parametrize("t", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,cap,pooled", pr.CAPPED["convt"], ids=_ids(pr.CAPPED["convt"]))
def test_capped_resident_weights_convT(shape, cap, pooled, t, monkeypatch):
    _one_tile_each_without_the_cap("convt", shape)
    _convT_case(t, shape, cap, None, monkeypatch)


@pytest.mark.parametrize("kernel", pr.F44)
def test_capped_exact_integers_across_a_channel_group(kernel, monkeypatch):
    """The 576-weight single-tap construction of test_gpu_layers.py (every U entry and every intermediate an exactly representable
    integer) with an integer shift per channel, on a walk that crosses a channel group: bit-equal to the oracle, taps in every group --
    a U slice or a bias of the previous tile's group gives other integers."""
    shape, cap = pr.EXACT[kernel]
    B, H, W, Cin, Cout = shape
    assert pr.props(kernel, shape, cap).crossing >= 1
    if kernel == "wino4_1b":
        monkeypatch.setenv("MIUNET_WINO4S", "0")
    monkeypatch.setenv("MIUNET_CUS", str(cap))
    r = np.random.default_rng(31)
    x = r.integers(-2, 3, (B, H, W, Cin)).astype(np.float32)
    shift = r.integers(-3, 4, Cout).astype(np.float32)
    G = 128 if kernel == "wino4a" else 64                 # channels of a group: a tap in the first and last channel of each
    taps = [(0, 2, 5, 7), (2, 0, Cin - 1, Cout - 1), (1, 1, 0, G), (0, 0, 17, G - 1), (2, 2, 9, Cout - G), (1, 0, 3, G + 3)]
    for (ky, kx, ci, co) in taps:
        w = np.zeros((Cout, Cin, 3, 3), np.float32)
        w[co, ci, ky, kx] = 576.0
        res = binding.layer_debug_strided(FP32_OP[kernel], x, w, None, shift, relu=False, **_layout(Cout, False))
        assert res["kernel"] == FP32_ROUTE[kernel]
        got = _slice(res, "out", FP32_OP[kernel], f"{kernel} tap {(ky, kx, ci, co)}")
        ref = orc.conv3x3(x, w) + shift
        assert (ref < 0).any() and np.array_equal(got, ref), (kernel, ky, kx, ci, co)


# ------------------------------------------------------------------------------------------ the production grid, no cap
@pytest.mark.parametrize("kernel", pr.F44)
def test_production_grid_fp32(kernel, monkeypatch):
    """cus < nwg < 2 cus, nwg & 7 != 0 at one workgroup per CU: some workgroups take two tiles, their neighbours one; the schedule
    check is against the same call on a grid of 8"""
    shape = pr.production_shape(kernel, _device_cus())
    assert pr.production_ok(kernel, shape, _device_cus())
    _fp32_case(kernel, shape, None, 8, False, monkeypatch)


@pytest.mark.parametrize("kernel,t", [("lpr", "bf16"), ("lprk", "fp16"), ("convt", "bf16")])
def test_production_grid_16bit(kernel, t, monkeypatch):
    shape = pr.production_shape(kernel, _device_cus())
    assert pr.production_ok(kernel, shape, _device_cus())
    if kernel == "convt":
        _convT_case(t, shape, None, 8, monkeypatch)
    else:
        _lp_case(kernel, t, shape, None, 8, False, monkeypatch)


# ------------------------------------------------------------------------------------------ the whole network: the fused heads
def _network(monkeypatch, env, spec, algo, seed):
    """one engine at 96 x 80, batch 3, under MIUNET_CUS=8 and one without: (kernel names, labels, logits) of each"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blob = pack_weights(spec, synth.make_weights(spec, seed))
    imgs = synth.make_images(3, 96, 80, spec.in_ch, 0x51 + seed, "blobs")
    out = {}
    for cap in ("8", None):
        if cap is None:
            monkeypatch.delenv("MIUNET_CUS", raising=False)
        else:
            monkeypatch.setenv("MIUNET_CUS", cap)
        with binding.Engine(96, 80, spec.in_ch, spec.base, spec.levels, 3, max_batch=3, conv_algo=algo) as eng:
            eng.load_weights(blob)
            eng.set_profiling(True)
            labels, logits = eng.infer(imgs, want_logits=True)
            out[cap] = ([(s["name"], s["kernel"]) for s in eng.kernel_stats()], labels, logits)
    return out["8"], out[None]


def _same_network(capped, free, must_run):
    assert capped[0] == free[0], "the cap changed a route"
    names = [k for _, k in capped[0]]
    for k in must_run:
        assert k in names, (k, names)
    assert np.array_equal(capped[2].view(np.uint32), free[2].view(np.uint32)), "logits depend on the schedule"
    assert np.array_equal(capped[1], free[1])


@pytest.mark.parametrize("wino4s,head", [("0", "conv3x3_wino4+head"), ("1", "conv3x3_wino4s+head")])
def test_whole_network_fp32_under_the_cap(wino4s, head, monkeypatch):
    """fp32 plan, MIUNET_SPLITK=0 (no route then depends on the CU count: the kernel names are asserted equal).  MIUNET_WINO4S=0 puts
    the Cout = 64 layers and the fused head on the persistent one-block kernel, which the layer hook cannot run with a head: 90 tiles
    on 8 workgroups.  The numeric guard is off in both engines, so F(4x4,3x3) stays whatever the synthetic weights' range."""
    spec = UNetSpec(1, 64, 2, 3)
    env = {"MIUNET_SPLITK": "0", "MIUNET_WINO4S": wino4s, "MIUNET_WINO4_GUARD": "0"}
    capped, free = _network(monkeypatch, env, spec, "winograd", 77)
    _same_network(capped, free, [head])


@pytest.mark.parametrize("algo,in_ch", [("bf16", 3), ("fp16", 3), ("bf16", 1), ("fp16", 1)])
def test_whole_network_16bit_under_the_cap(algo, in_ch, monkeypatch):
    """base 32, three levels, every resident-weight kernel whatever the grid (test_resident_weight_kernel_in_the_whole_network):
    conv3x3_*r with the fused pooling, +first (three-channel image) and +head, conv3x3_*k and the three convT2x2_*r shapes walk
    several tiles per workgroup on a grid of 8, and give the bytes of the uncapped engine."""
    spec = UNetSpec(in_ch, 32, 3, 3)
    env = {"MIUNET_LPR": "2", "MIUNET_LPRK": "2", "MIUNET_CONVT_LPR": "2"}
    capped, free = _network(monkeypatch, env, spec, algo, 78)
    must = [f"conv3x3_{algo}r", f"conv3x3_{algo}r+head", f"conv3x3_{algo}k", f"convT2x2_{algo}r"] + ([f"conv3x3_{algo}r+first"] if in_ch == 3 else [])
    _same_network(capped, free, must)
