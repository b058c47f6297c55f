"""The split-K decision of the hipcc Winograd launchers on the CPU: csrc/routing.cpp's wino4_ksplit / wino_ksplit and
csrc/kernels.h's ksplit_range (tests/cpu/ksplit_test.cpp, built with g++) against the model of tests/splitk_ref.py over a sweep, the
properties a split must have for the reduce kernel to be right, and the case table of tests/test_gpu_splitk.py proven from the
model alone -- conditions on the inputs of the GPU tests, which say nothing about the kernels."""
import os
import subprocess

import pytest

import splitk_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB_GRIDS = (1, 2, 3, 4, 7, 16, 31, 32, 33, 64, 128, 129)
MAX_CHUNKS = {kr.F4: 200, kr.F2: 400}
SLAB = {kr.F4: 16 * 16 * 128 * 4, kr.F2: 8 * 16 * 128 * 4}           # per image of the sweep's layers


@pytest.fixture(scope="module")
def cpp_lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ksplit") / "ksplit_test"
    pkg = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpu", "ksplit_test.cpp"), os.path.join(pkg, "csrc", "routing.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, timeout=300, check=True)
    return r.stdout.decode().split("\n")[:-1]


def _model_line(fam, chunks, grid, ws):
    slab = grid * SLAB[fam]
    ws_bytes = kr.WS_BYTES if ws == "full" else None if ws == "null" else int(ws) * slab
    s = kr.split(fam, grid, chunks, slab, ws_bytes)
    return f"{fam} {chunks} {grid} {ws} {s.ks} " + " ".join(f"{b}:{e}" for b, e in s.ranges)


def _sweep():
    for fam in (kr.F4, kr.F2):
        for chunks in range(1, MAX_CHUNKS[fam] + 1):
            for grid in range(1, 161):
                yield fam, chunks, grid, "full"
        for chunks in range(1, MAX_CHUNKS[fam] + 1, 7):
            for grid in SUB_GRIDS:
                for ws in [str(n) for n in range(9)] + ["null"]:
                    yield fam, chunks, grid, ws


def _parse(line):
    fam, chunks, grid, ws, ks, *ranges = line.split(" ")
    return fam, int(chunks), int(grid), ws, int(ks), [tuple(map(int, r.split(":"))) for r in ranges]


def test_the_library_decides_as_the_model_over_the_whole_sweep(cpp_lines):
    """d: every line of the C++ sweep -- ks and every slice's range -- is the model's"""
    got = [l for l in cpp_lines if not l.startswith("misaligned")]
    want = [_model_line(*c) for c in _sweep()]
    assert len(got) == len(want) == 2 * 160 * 300 + (29 + 58) * len(SUB_GRIDS) * 10
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    ks_seen = {(l.split(" ")[0], int(l.split(" ")[4])) for l in got}
    assert ks_seen == {(f, k) for f in (kr.F4, kr.F2) for k in range(1, 9)}, "the sweep reaches every slice count"


def test_every_split_of_the_sweep_is_a_partition_that_fits(cpp_lines):
    """a: no slice is empty, the ranges are disjoint and cover [0, chunks); b: F(2x2) slices begin at whole super-chunks; c: the
    slabs fit the workspace.  On the library's own output."""
    n_split = 0
    for l in cpp_lines:
        if l.startswith("misaligned"):
            continue
        fam, chunks, grid, ws, ks, ranges = _parse(l)
        assert len(ranges) == ks >= 1, l
        assert ranges[0][0] == 0 and ranges[-1][1] == chunks, l
        assert all(b < e for b, e in ranges), l
        assert all(ranges[k][1] == ranges[k + 1][0] for k in range(ks - 1)), l
        if fam == kr.F2:
            assert all(b % 4 == 0 for b, _ in ranges), l
        if ks > 1:
            n_split += 1
            assert ws != "null" and grid <= 128 and chunks >= kr.MIN_CHUNKS[fam], l
            ws_bytes = kr.WS_BYTES if ws == "full" else int(ws) * grid * SLAB[fam]
            assert ks * grid * SLAB[fam] <= ws_bytes, l
            assert ks * grid <= 256 and ks <= 8, l
    assert n_split > 10000


def test_misaligned_layouts_and_the_fused_head_never_split(cpp_lines):
    """the reduce kernel reads and writes 16 bytes at a time and knows no head: Cout, ldo or co_off off a multiple of 4, or head
    operands, give ks = 1 on a layer that otherwise splits eight ways (the upper half of a concat pixel is aligned, and splits)"""
    got = dict(l.split(" ", 1)[1].rsplit(" ", 1) for l in cpp_lines if l.startswith("misaligned"))
    want = {f"{f} {w}": k for f in (kr.F4, kr.F2) for w, k in (("none", "8"), ("Cout", "1"), ("ldo", "1"), ("co_off", "1"), ("upper_half", "8"))}
    want.update({"wino4 head": "1", "wino4 no_head": "8"})
    assert got == want
    for fam in (kr.F4, kr.F2):
        shape = (1, 16, 16, 1024, 128)
        assert kr.layer(fam, shape).ks == 8 and kr.layer(fam, shape, ldo=256, co_off=128).ks == 8
        assert kr.layer(fam, shape, ldo=130).ks == 1 and kr.layer(fam, shape, ldo=260, co_off=130).ks == 1
        assert kr.layer(fam, (1, 16, 16, 1024, 126)).ks == 1 and kr.layer(fam, shape, head=True).ks == 1


@pytest.mark.parametrize("case", kr.CASES, ids=[kr.case_id(c) for c in kr.CASES])
def test_each_case_of_the_gpu_table_has_the_split_it_claims(case):
    """e: ks and the slice lengths of every row, from the model with the hook's workspace"""
    s = kr.case_split(case)
    assert s.ks == case.ks > 1, (case, s)
    if case.lens is not None:
        assert s.lens == case.lens, (case, s)
    assert sum(s.lens) == s.chunks == -(-case.shape[3] // kr.CHUNK[case.fam])
    assert case.shape[4] % 4 == 0 and case.shape[0] * case.shape[1] * case.shape[2] * case.shape[4] * 4 < 2 << 20, "every tensor small"


def test_the_gpu_table_contains_every_condition_it_is_there_for():
    """f: each condition the table names is met by some row, decided by the model alone"""
    rows = [(c, kr.case_split(c)) for c in kr.CASES]
    f4 = [(c, s) for c, s in rows if c.fam == kr.F4]
    f2 = [(c, s) for c, s in rows if c.fam == kr.F2]

    def some(rs, pred):
        return any(pred(c, s, *c.shape) for c, s in rs)

    # ---- F(4x4)
    assert some(f4, lambda c, s, B, H, W, Ci, Co: s.grid == 1 and kr.wino4_nb(Co) == 2 and s.chunks == 8 and s.ks == 2), "smallest two-block split"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: Ci % 16 != 0), "a half-full last chunk"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: H % 16 and W % 16 and s.lens[-1] < s.lens[0] and s.lens[0] % 2 == 1), "ragged tiles, ragged and odd slices"
    # a slice of one chunk whose second opening load (chunk begin + 1) lies past the last chunk of the layer
    assert some(f4, lambda c, s, B, H, W, Ci, Co: s.lens[-1] == 1 and s.ranges[-1][0] + 1 >= s.chunks and B > 1), "a one-chunk slice"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: kr.wino4_nb(Co) == 1 and Co == 64), "the one-block kernel"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: s.ks < s.fit == s.wanted), "the no-empty-slice loop shrinks the split"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: kr.wino4_nb(Co) == 2 and Co == 256), "two channel groups of the two-block kernel"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: kr.wino4_nb(Co) == 1 and Co == 192 and H % 16 == 2 and W % 16 == 2), "one-block, three groups, a rim"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: H % 2 == 0 and W % 2 == 0 and H % 16 and B > 1), "even ragged sizes for _pool"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: Co % 64 and Co % 4 == 0), "masked columns"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: s.ks == 8 and s.lens == [8] * 8 and H == 4), "the bottleneck at batch 1"
    assert some(f4, lambda c, s, B, H, W, Ci, Co: c.slabs is not None and s.ks == s.fit == c.slabs < s.wanted), "the workspace shrinks the split"
    # ---- F(2x2)
    assert some(f2, lambda c, s, B, H, W, Ci, Co: s.grid == 1 and s.chunks == 16 and s.ks == 2), "smallest split"
    assert some(f2, lambda c, s, B, H, W, Ci, Co: s.lens[-1] < s.lens[0] and s.lens[-1] % 4), "a ragged last slice that ends inside a super-chunk"
    assert some(f2, lambda c, s, B, H, W, Ci, Co: s.lens[-1] == 1 and (H % 8 or W % 16)), "ragged tiles, one-chunk slice"
    assert some(f2, lambda c, s, B, H, W, Ci, Co: Co <= 64 and s.ks < s.fit == s.wanted), "64 x 64 configuration, the loop shrinks the split"
    assert some(f2, lambda c, s, B, H, W, Ci, Co: s.ks == 5 and s.lens[-1] == 1), "five slices"
    assert some(f2, lambda c, s, B, H, W, Ci, Co: s.ks == 8 and Co > 64) and some(f2, lambda c, s, B, H, W, Ci, Co: s.ks == 8 and Co <= 64), "eight slices in both configurations"
    assert some(f2, lambda c, s, B, H, W, Ci, Co: Ci % 8 != 0 and B > 1), "a masked last chunk"
    # ---- the rows of the scaling-law and special-value tests are rows of the table: even, ragged, one-chunk
    for fam, shapes in kr.ROWS3.items():
        picked = [next(s for c, s in rows if c.fam == fam and c.shape == sh and c.slabs is None) for sh in shapes]
        assert len(set(picked[0].lens)) == 1 and picked[1].lens[-1] < picked[1].lens[0] and picked[2].lens[-1] == 1, (fam, picked)
    # ---- and the contract case does not split, with the same workspace
    fam, shape = kr.NO_SPLIT
    assert kr.layer(fam, shape, kr.hook_ws_bytes(shape)).ks == 1 and kr.layer(fam, shape[:3] + (128, 128), kr.hook_ws_bytes(shape)).ks == 2
