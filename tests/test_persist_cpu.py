"""The model of the persistent kernels' tile walk (tests/persist_ref.py) and the case tables of tests/test_gpu_persistent_walk.py,
on the CPU: the walk is complete, the CU clamp of csrc/routing.cpp is the model's, and the cases are not degenerate -- conditions on
the inputs of the GPU tests, decided by the model alone."""
import os
import subprocess

import pytest

import persist_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _complete(nwg, cus):
    seen = sorted(t for tiles in pr.walk(nwg, cus).values() for t in tiles)
    return seen == list(range(nwg))


@pytest.mark.parametrize("cus_range,nwg_range", [(range(8, 41), range(1, 700)), ((256, 304), range(1, 3000))])
def test_the_walk_visits_every_tile_exactly_once(cus_range, nwg_range):
    bad = [(cus, nwg) for cus in cus_range for nwg in nwg_range if not _complete(nwg, cus)]
    assert not bad, bad[:10]


def test_the_walk_of_a_workgroup_is_ascending_inside_its_xcd_range():
    for cus in (8, 9, 12, 16, 23, 256):
        for nwg in (1, 7, 8, 9, 18, 45, 54, 300, 511):
            q, r = nwg >> 3, nwg & 7
            for bid, tiles in pr.walk(nwg, cus).items():
                x = bid & 7
                lo = x * q + min(x, r)
                assert tiles == sorted(tiles) and all(lo <= t < lo + q + (x < r) for t in tiles), (cus, nwg, bid)


def test_below_eight_workgroups_the_partition_loses_tiles_and_the_clamp_closes_it():
    """grid = min(nwg, cus) < 8 with nwg > cus leaves XCDs that own tiles without a slot (cus = 1, nwg = 2: tile 1 is never computed);
    Routing::cus is therefore never below 8, whatever the device reports and whatever MIUNET_CUS asks for"""
    assert not _complete(2, 1) and not _complete(20, 7)
    for dev in range(1, 8):
        assert pr.clamp_cus(dev) == 8 and pr.clamp_cus(dev, "1") == 8
        assert all(_complete(nwg, pr.clamp_cus(dev)) for nwg in range(1, 200))


def test_the_clamp_of_the_library_is_the_model(tmp_path):
    """persistent_cus of csrc/routing.cpp (tests/cpu/persistent_cus_test.cpp) on device counts below, at and above 8 and on every
    kind of MIUNET_CUS text: floor 8, never above the device's own count, unset or empty = the device's count"""
    exe = tmp_path / "persistent_cus_test"
    pkg = os.path.join(ROOT, "unet-medical-image-contour-segmentation-cpp_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpu", "persistent_cus_test.cpp"), os.path.join(pkg, "csrc", "routing.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, timeout=60, check=True)
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == 9 * 16
    for line in lines:
        dev, text, got = line.split(" ")
        dev, got = int(dev), int(got)
        want = pr.clamp_cus(dev, {"-": None, "empty": ""}.get(text, text))
        assert got == want, line
        assert 8 <= got <= max(8, dev), line
    assert "256 - 256" in lines and "256 23 23" in lines and "256 7 8" in lines and "256 257 256" in lines and "1 - 8" in lines and "7 23 8" in lines


def test_the_model_gives_the_figures_the_tables_were_chosen_by():
    p = pr.props("wino4a", (1, 48, 48, 64, 256), 8)
    assert (p.nwg, p.grid, p.per_wg[0], p.per_wg[-1], p.crossing) == (18, 8, 2, 3, 1)
    p = pr.props("wino4a", (3, 32, 48, 64, 256), 12)
    assert (p.nwg, p.per_wg[0], p.per_wg[-1], p.crossing) == (36, 2, 4, 2)
    p = pr.props("wino4a", (1, 80, 48, 64, 384), 16)
    assert (p.nwg, p.per_wg[0], p.per_wg[-1], p.crossing) == (45, 2, 3, 2)
    p = pr.props("wino4a", (3, 48, 48, 64, 256), 23)
    assert (p.nwg, p.per_wg[0], p.per_wg[-1], p.crossing) == (54, 2, 3, 1)
    p = pr.props("wino4b", (1, 48, 96, 64, 192), 8)
    assert (p.nwg, p.per_wg[0], p.per_wg[-1], p.crossing) == (27, 3, 4, 1)
    p = pr.props("wino4a", (1, 160, 160, 64, 384), 256)
    assert (p.nwg, p.per_wg[0], p.per_wg[-1], p.crossing) == (300, 1, 2, 11)


@pytest.mark.parametrize("kernel", sorted(pr.CAPPED))
def test_the_capped_cases_are_not_degenerate(kernel):
    cases = pr.CAPPED[kernel]
    P = [pr.props(kernel, shape, cap) for shape, cap, _ in cases]
    assert {cap for _, cap, _ in cases} == set(pr.CAPS)
    assert all(cap == pr.clamp_cus(256, str(cap)) for _, cap, _ in cases)                       # no cap the library would move
    assert any(p.nwg & 7 and p.nwg > p.grid for p in P), "(i) nwg & 7 != 0 with nwg > grid"
    assert any(len(set(p.per_wg)) >= 2 for p in P), "(ii) two tiles-per-workgroup counts in one launch"
    assert any(p.per_wg[-1] >= pr.DEEPEST_RING + 1 for p in P), "(iii) a workgroup one tile past the deepest ring"
    # ... next to a workgroup of the same launch with fewer tiles than that ring is deep: nt below the depth and above it
    assert any(p.per_wg[-1] >= pr.DEEPEST_RING + 1 and p.per_wg[0] < pr.DEEPEST_RING for p in P)
    if kernel in pr.F44:
        assert any(p.crossing >= 1 for p in P), "(iv) a walk that crosses a channel-group boundary"
        assert sum(p.crossing >= 1 for p in P) >= 3
    assert any(p.nwg < cap for p, (_, cap, _) in zip(P, cases)), "(v) nwg < cus under the cap"
    assert any(p.grid & 7 for p in P), "(vi) grid & 7 != 0"
    assert any(p.grid & 7 and p.nwg > p.grid for p in P)                                        # ... with several tiles per workgroup
    assert any(pooled for _, _, pooled in cases) or kernel in ("lprk", "convt")                 # the fused pooling where the kernel has it
    assert all(p.nwg <= 64 for p in P)                                                          # a few dozen tiles: quick, and one tile per workgroup without the cap


@pytest.mark.parametrize("kernel", pr.F44)
def test_the_exact_cases_cross_a_channel_group(kernel):
    shape, cap = pr.EXACT[kernel]
    assert (shape, cap) in [(s, c) for s, c, _ in pr.CAPPED[kernel]]
    assert pr.props(kernel, shape, cap).crossing >= 1


def test_the_one_block_cases_have_ragged_blocks_and_both_channel_counts():
    shapes = [s for s, _, _ in pr.CAPPED["wino4_1b"]]
    assert {s[4] for s in shapes} == {64, 192}
    assert any(s[1] % 16 and s[2] % 16 for s in shapes)


def test_the_resident_weight_cases_cover_every_channel_pair():
    assert {s[3:] for s, _, _ in pr.CAPPED["lpr"]} == {(32, 32), (32, 64), (64, 32), (64, 64)}
    assert {s[3:] for s, _, _ in pr.CAPPED["convt"]} == {(64, 32), (128, 64), (256, 128)}
    for k in ("lpr", "lprk", "convt"):                                                          # partial edge tiles in x and y
        assert any(s[2] % 32 for s, _, _ in pr.CAPPED[k])


@pytest.mark.parametrize("kernel", sorted(pr.PRODUCTION))
def test_the_production_cases(kernel):
    """cus < nwg < 2 cus and nwg & 7 != 0: at 256 CUs the listed shapes themselves (300 tiles); at other CU counts a shape is found"""
    assert pr.production_shape(kernel, 256) == pr.PRODUCTION[kernel][0]
    p = pr.props(kernel, pr.PRODUCTION[kernel][0], 256)
    assert p.nwg == 300 and p.grid == 256 and p.per_wg[0] == 1 and p.per_wg[-1] == 2
    if kernel in pr.F44:
        assert p.crossing >= 1
    for cus in (64, 104, 228, 304):
        shape = pr.production_shape(kernel, cus)
        assert pr.production_ok(kernel, shape, cus)
        assert set(pr.props(kernel, shape, cus).per_wg) == {1, 2}
