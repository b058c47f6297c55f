"""Reference for the volume branch graph (include/mi_unet.h: mi_unet_volume_branches), written from the definition in
numpy / scipy and importing nothing from the library: degrees by shifted comparisons, clusters and branches by scipy.ndimage.label with the
3 x 3 x 3 structure per id and class (no union-find, no flood fill of its own), rows by sorting the sets' lowest voxels, the pruning
rounds on top, the derived doubles (parts by scipy's connected_components); and the registry of cases the CPU and GPU tests share."""
import functools
import math

import numpy as np
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import volume_skeleton_ref as vk

BRANCH_BYTES, NODE_BYTES, GRAPH_BYTES, INFO_BYTES = 88, 56, 128, 24
MAX_ROWS = 1 << 20
OFF = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
FULL = np.ones((3, 3, 3), int)
ISOLATED, END, BRANCH, JUNCTION = 1, 2, 3, 4
NODE_FIELDS = ("first", "sz", "sy", "sx", "id", "kind", "voxels", "degree", "r2_min", "r2_max")
BRANCH_FIELDS = ("first", "att_lo", "att_hi", "r2_sum", "id", "kind", "node_a", "node_b", "voxels", "r2_min", "r2_max")
GRAPH_FIELDS = ("nodes", "ends", "junction_nodes", "isolated", "junction_voxels", "branches", "closed", "pruned_spurs", "pruned_voxels")


def link_class(dz, dy, dx):
    return abs(dx) + 2 * abs(dy) + 4 * abs(dz) - 1


def graph_of(clean, m, r2=None):
    """the graph of one state: clean int32 [D,H,W] with values 0 .. m -> dict(nodes, branches: lists of dicts in table order, graph: m dicts
    without the pruning counts, map int32 [D,H,W])"""
    d, h, w = clean.shape
    a = np.zeros((d + 2, h + 2, w + 2), np.int32)
    a[1:-1, 1:-1, 1:-1] = clean
    deg = np.zeros(a.shape, np.int32)
    for dz, dy, dx in OFF:
        deg += (np.roll(a, (-dz, -dy, -dx), (0, 1, 2)) == a) & (a > 0)
    cls = np.where(a > 0, np.minimum(deg, 3) + 1, 0)                # 1 isolated, 2 end, 3 branch voxel, 4 junction voxel
    lin = lambda p: ((int(p[0]) - 1) * h + (int(p[1]) - 1)) * w + (int(p[2]) - 1)      # a padded position -> the linear index
    rad = np.zeros(a.shape, np.int64)
    if r2 is not None:
        rad[1:-1, 1:-1, 1:-1] = r2
    present = [int(v) for v in np.unique(clean) if v > 0]
    # NODES
    nodes = []
    for p in np.argwhere((cls == ISOLATED) | (cls == END)):
        nodes.append(dict(pts=p[None], id=int(a[tuple(p)]), kind=0 if cls[tuple(p)] == ISOLATED else 1))
    for v in present:
        lab, n = ndimage.label((a == v) & (cls == JUNCTION), FULL)
        for pts in _groups(lab, n):
            nodes.append(dict(pts=pts, id=v, kind=2))
    for nd in nodes:
        nd["first"] = min(lin(p) for p in nd["pts"])
    nodes.sort(key=lambda nd: nd["first"])
    node_at = {}
    for k, nd in enumerate(nodes):
        pts = nd["pts"]
        vals = rad[pts[:, 0], pts[:, 1], pts[:, 2]]
        nd.update(sz=int((pts[:, 0] - 1).sum()), sy=int((pts[:, 1] - 1).sum()), sx=int((pts[:, 2] - 1).sum()), voxels=len(pts), degree=0,
                  r2_min=int(vals.min()) if r2 is not None else 0, r2_max=int(vals.max()) if r2 is not None else 0)
        for p in pts:
            node_at[lin(p)] = k
    # BRANCHES
    branches = []
    for v in present:
        lab, n = ndimage.label((a == v) & (cls == BRANCH), FULL)
        for pts in _groups(lab, n):
            links, att = [0] * 7, []
            for p in pts:
                for dz, dy, dx in OFF:
                    q = (p[0] + dz, p[1] + dy, p[2] + dx)
                    if a[q] != v:
                        continue
                    if cls[q] != BRANCH:
                        att.append(lin(q))
                        links[link_class(dz, dy, dx)] += 1
                    elif lin(q) > lin(p):
                        links[link_class(dz, dy, dx)] += 1
            assert len(att) in (0, 2), (len(att), "attachments of a voxel branch")
            vals = rad[pts[:, 0], pts[:, 1], pts[:, 2]]
            use = r2 is not None
            branches.append(dict(pts=pts, first=min(lin(p) for p in pts), id=v, kind=0 if att else 1, att=att, voxels=len(pts), links=links,
                                 r2_sum=int(vals.sum()) if use else 0, r2_min=int(vals.min()) if use else 0, r2_max=int(vals.max()) if use else 0))
    for p in np.argwhere(cls == END):
        v = int(a[tuple(p)])
        for dz, dy, dx in OFF:
            q = (p[0] + dz, p[1] + dy, p[2] + dx)
            if a[q] == v and (cls[q] == JUNCTION or (cls[q] == END and lin(q) > lin(p))):
                links = [0] * 7
                links[link_class(dz, dy, dx)] = 1
                branches.append(dict(pts=np.zeros((0, 3), int), first=lin(p), id=v, kind=2, att=[lin(p), lin(q)], voxels=0, links=links,
                                     r2_sum=0, r2_min=0, r2_max=0))
    branches.sort(key=lambda b: b["first"])
    assert len({b["first"] for b in branches}) == len(branches)
    vmap = np.zeros((d, h, w), np.int32)
    for k, b in enumerate(branches):
        if b["att"]:
            b["att_lo"], b["att_hi"] = min(b["att"]), max(b["att"])
            b["node_a"], b["node_b"] = node_at[b["att_lo"]], node_at[b["att_hi"]]
            for q in b["att"]:
                nodes[node_at[q]]["degree"] += 1
        else:
            b["att_lo"] = b["att_hi"] = b["node_a"] = b["node_b"] = -1
        pts = b["pts"]
        vmap[pts[:, 0] - 1, pts[:, 1] - 1, pts[:, 2] - 1] = k + 1
    for k, nd in enumerate(nodes):
        pts = nd["pts"]
        vmap[pts[:, 0] - 1, pts[:, 1] - 1, pts[:, 2] - 1] = -(k + 1)
    graph = []
    for r in range(m):
        ns, bs = [nd for nd in nodes if nd["id"] == r + 1], [b for b in branches if b["id"] == r + 1]
        graph.append(dict(nodes=len(ns), ends=sum(nd["kind"] == 1 for nd in ns), junction_nodes=sum(nd["kind"] == 2 for nd in ns),
                          isolated=sum(nd["kind"] == 0 for nd in ns), junction_voxels=sum(nd["voxels"] for nd in ns if nd["kind"] == 2),
                          branches=len(bs), closed=sum(b["kind"] == 1 for b in bs), links=[sum(b["links"][c] for b in bs) for c in range(7)],
                          pruned_spurs=0, pruned_voxels=0))
    return dict(nodes=nodes, branches=branches, graph=graph, map=vmap)


def _groups(lab, n):
    """the positions [k, 3] of each of the n labels"""
    if not n:
        return []
    pts = np.argwhere(lab > 0)
    which = lab[pts[:, 0], pts[:, 1], pts[:, 2]]
    order = np.argsort(which, kind="stable")
    cuts = np.flatnonzero(np.diff(which[order])) + 1
    return np.split(pts[order], cuts)


def is_spur(g, b, prune_voxels):
    if b["kind"] == 1 or b["voxels"] + 1 > prune_voxels:
        return False
    kinds = sorted((g["nodes"][b["node_a"]]["kind"], g["nodes"][b["node_b"]]["kind"]))
    return kinds == [1, 2]


def branches(ids, m, r2=None, prune_voxels=0, prune_rounds=0):
    """-> dict(nodes, branches, graph, map, ids, found_nodes, found_branches, rounds, stable)"""
    ids = np.asarray(ids, np.int32)
    d, h, w = ids.shape
    cur = np.where((ids >= 1) & (ids <= m), ids, 0).astype(np.int32)
    pruned = [[0, 0] for _ in range(m)]
    rounds = 0
    while True:
        g = graph_of(cur, m, r2)
        spurs = [b for b in g["branches"] if is_spur(g, b, prune_voxels)]
        stable = int(not spurs)
        if stable or (prune_rounds > 0 and rounds >= prune_rounds):
            break
        nxt = cur.copy().reshape(-1)
        for b in spurs:
            pts = b["pts"]
            if len(pts):
                nxt[((pts[:, 0] - 1) * h + (pts[:, 1] - 1)) * w + (pts[:, 2] - 1)] = 0
            nxt[b["att_lo"] if g["nodes"][b["node_a"]]["kind"] == 1 else b["att_hi"]] = 0
            pruned[b["id"] - 1][0] += 1
            pruned[b["id"] - 1][1] += b["voxels"] + 1
        cur = nxt.reshape(d, h, w)
        rounds += 1
    for r in range(m):
        g["graph"][r]["pruned_spurs"], g["graph"][r]["pruned_voxels"] = pruned[r]
    return dict(g, ids=cur, found_nodes=len(g["nodes"]), found_branches=len(g["branches"]), rounds=rounds, stable=stable)


def length_of(links, spacing):
    sx, sy, sz = (float(v) for v in spacing)
    length = 0.0
    for k in range(7):
        c = k + 1
        ex, ey, ez = (sx if c & 1 else 0.0), (sy if c & 2 else 0.0), (sz if c & 4 else 0.0)
        length += float(links[k]) * math.sqrt(ex * ex + ey * ey + ez * ez)
    return length


def derive_branch(b, shape, spacing, unit_mm):
    """mi_unet_volume_branches_derive_branch's arithmetic in Python floats, in its order"""
    h, w = shape[-2:]
    length, chord = length_of(b["links"], spacing), 0.0
    if b["kind"] != 1:
        lo, hi = int(b["att_lo"]), int(b["att_hi"])
        ex = float(hi % (h * w) % w - lo % (h * w) % w) * float(spacing[0])
        ey = float(hi % (h * w) // w - lo % (h * w) // w) * float(spacing[1])
        ez = float(hi // (h * w) - lo // (h * w)) * float(spacing[2])
        chord = math.sqrt(ex * ex + ey * ey + ez * ez)
    v = int(b["voxels"])
    return dict(length_mm=length, chord_mm=chord, tortuosity=length / chord if b["kind"] != 1 and chord > 0.0 else 0.0,
                radius_min_mm=math.sqrt(float(b["r2_min"])) * unit_mm, radius_max_mm=math.sqrt(float(b["r2_max"])) * unit_mm,
                radius_rms_mm=math.sqrt(float(b["r2_sum"]) / float(v)) * unit_mm if v else 0.0)


def derive(ref, comp_id, spacing):
    """per id: length from the summed links, parts by scipy's connected components of the id's nodes plus one per closed branch, loops"""
    g = ref["graph"][comp_id - 1]
    mine = [k for k, nd in enumerate(ref["nodes"]) if nd["id"] == comp_id]
    pos = {k: j for j, k in enumerate(mine)}
    edges = [(pos[b["node_a"]], pos[b["node_b"]]) for b in ref["branches"] if b["id"] == comp_id and b["kind"] != 1]
    parts = g["closed"]
    if mine:
        rows, cols = ([e[0] for e in edges], [e[1] for e in edges]) if edges else ([], [])
        parts += connected_components(coo_matrix((np.ones(len(edges)), (rows, cols)), shape=(len(mine), len(mine))), directed=False)[0]
    return dict(length_mm=length_of(g["links"], spacing), parts=parts, loops=g["branches"] - g["nodes"] - g["closed"] + parts)


# ---- comparing ---------------------------------------------------------------------------------------------------------------------------------
def assert_equal(got, want, what="", cap_nodes=None, cap_branches=None):
    """got: a result of the binding; want: branches()'s"""
    info = lambda r: (r["found_nodes"], r["found_branches"], r["rounds"], r["stable"])
    assert info(got) == info(want), (what, "info", info(got), info(want))
    for key, fields, cap in (("nodes", NODE_FIELDS, cap_nodes), ("branches", BRANCH_FIELDS, cap_branches)):
        rows = want[key] if cap is None else want[key][:cap]
        assert len(got[key]) == len(rows), (what, key, len(got[key]), len(rows))
        for k, row in enumerate(rows):
            for f in fields:
                assert int(got[key][k][f]) == row[f], (what, key, k, f, int(got[key][k][f]), row[f])
            if key == "branches":
                assert [int(v) for v in got[key][k]["links"]] == row["links"], (what, "branch", k, "links", got[key][k]["links"], row["links"])
    assert len(got["graph"]) == len(want["graph"])
    for r, row in enumerate(want["graph"]):
        for f in GRAPH_FIELDS:
            assert int(got["graph"][r][f]) == row[f], (what, "id", r + 1, f, int(got["graph"][r][f]), row[f])
        assert [int(v) for v in got["graph"][r]["links"]] == row["links"], (what, "id", r + 1, "links")
    if got["map"] is not None:
        assert np.array_equal(got["map"], want["map"]), (what, "map", np.argwhere(got["map"] != want["map"])[:5].tolist())
    if got["ids"] is not None:
        assert np.array_equal(got["ids"], want["ids"]), (what, "ids", int((got["ids"] != want["ids"]).sum()))


def same_bytes(a, b, what=""):
    for key in ("nodes", "branches", "graph", "map", "ids"):
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, (what, key)
            continue
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    for key in ("found_nodes", "found_branches", "rounds", "stable"):
        assert a[key] == b[key], (what, key, a[key], b[key])


# ---- hand-built inputs: (y, x) positions in the middle slice of three unless said otherwise -------------------------------------------------------
def plane(points, shape):
    v = np.zeros((3,) + tuple(shape), np.int32)
    for y, x in points:
        v[1, y, x] = 1
    return v


def diamond(cy, cx):
    return [(y, x) for y in range(cy - 3, cy + 4) for x in range(cx - 3, cx + 4) if abs(y - cy) + abs(x - cx) == 3]


def single_voxel_loop():
    """(1, 2) has two neighbours, (2, 2) and (2, 3), which are adjacent junction voxels, each with a tail"""
    return plane([(1, 2), (2, 2), (2, 3), (3, 1), (4, 1), (5, 1), (3, 4), (4, 4), (5, 4)], (7, 6))


def lollipop():
    return plane(diamond(4, 4) + [(4, 8), (4, 9), (4, 10)], (9, 12))


def figure_eight():
    return plane(sorted(set(diamond(4, 4) + diamond(4, 10))), (9, 15))


def plus():
    """two lines that cross: the centre and its four neighbours are pairwise adjacent enough to be one cluster of five"""
    return plane([(5, x) for x in range(11)] + [(y, 5) for y in range(11)], (11, 11))


def serpentine():
    """one path through 5 x 20 x 140: four rows 1 .. 138 along x that climb in z, joined by diagonal corners and runs along y at x = 0 and
    139; it crosses tile borders (64 x 8 x 4) on all three axes"""
    v = np.zeros((5, 20, 140), np.int32)
    zs = lambda x: min(4, x // 28)
    for k, y in enumerate((0, 6, 12, 18)):
        for x in range(1, 139):
            v[zs(x), y, x] = 1
        if k < 3:
            x_turn, z_turn = (139, zs(138)) if k % 2 == 0 else (0, zs(1))
            for yy in range(y + 1, y + 6):
                v[z_turn, yy, x_turn] = 1
    return v


def interleaved():
    """1 x 4 x 64: row 0 holds segments of five voxels whose ids alternate and touch; rows 2 and 3 are two lines of different ids that
    touch along their whole length"""
    v = np.zeros((1, 4, 64), np.int32)
    v[0, 0] = 1 + (np.arange(64) // 5) % 2
    v[0, 2], v[0, 3] = 1, 2
    return v


def noise_block():
    rng = np.random.default_rng(23)
    return ((rng.random((6, 12, 70)) < 0.3) * (1 + (rng.random((6, 12, 70)) < 0.5))).astype(np.int32)


def border_path():
    """along three edges of a 4 x 5 x 6 volume, through two of its corners, both ends in corners"""
    v = np.zeros((4, 5, 6), np.int32)
    v[0, 0, :] = 1
    v[0, :, 5] = 1
    v[:, 4, 5] = 1
    return v


def y_with_arm(length):
    """a junction at (5, 5), two diagonal arms of five voxels, a third arm of `length` voxels straight up"""
    pts = [(5, 5)] + [(5 + k, 5 - k) for k in range(1, 6)] + [(5 + k, 5 + k) for k in range(1, 6)] + [(5 - k, 5) for k in range(1, length + 1)]
    return plane(pts, (11, 11))


def comb():
    pts = [(6, x) for x in range(31)]
    for k in range(5):
        pts += [(6 - j, 4 + 5 * k) for j in range(1, k + 2)]
    return plane(pts, (8, 31))


def spur_on_spur():
    """a spine, an arm that bends where a twig leaves it: the twig and the arm's outer part are spurs of the first state, what is left of
    the arm is a spur of the second"""
    pts = [(10, x) for x in range(21)] + [(9, 10), (8, 10), (7, 10), (6, 10), (5, 11), (4, 12), (3, 13), (5, 9), (4, 8)]
    return plane(pts, (12, 21))


def star():
    return plane([(5, 5), (4, 4), (3, 3), (4, 6), (3, 7), (6, 5), (7, 5)], (9, 9))


SKELETON_CASES = ("y", "line", "rod", "two_voxels", "single_voxel", "torus", "ring", "one_slice", "shell", "seams", "tubes_in_contact", "noise",
                  "absent_ids")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids int32 [D,H,W], m, r2 int32 [D,H,W] or None, keyword arguments of a call)"""
    c = {}
    for name in SKELETON_CASES:
        sk = vk.case_ref(name)
        c[name] = (sk["ids"], vk.cases()[name][1], sk["r2"], {})
    for name, v in (("single_voxel_loop", single_voxel_loop()), ("lollipop", lollipop()), ("figure_eight", figure_eight()), ("plus", plus()),
                    ("serpentine", serpentine()), ("border_path", border_path())):
        c[name] = (v, 1, None, {})
    c["interleaved"] = (interleaved(), 2, None, {})
    block = noise_block()
    c["noise_block"] = (block, 2, (block * 3 + 1).astype(np.int32), {})
    noise = c["noise"]
    c["noise_caps_below"] = noise[:3] + (dict(cap_nodes=7, cap_branches=5),)
    c["noise_caps_0"] = noise[:3] + (dict(cap_nodes=0, cap_branches=0),)
    for length in (1, 2, 3):
        for prune in (1, 2, 3, 4):
            c[f"y_arm{length}_prune{prune}"] = (y_with_arm(length), 1, None, dict(prune_voxels=prune))
    c["comb_prune3"] = (comb(), 1, None, dict(prune_voxels=3))
    c["spur_on_spur"] = (spur_on_spur(), 1, None, dict(prune_voxels=3))
    c["spur_on_spur_one_round"] = (spur_on_spur(), 1, None, dict(prune_voxels=3, prune_rounds=1))
    c["star_prune2"] = (star(), 1, None, dict(prune_voxels=2))
    c["noise_prune3"] = noise[:3] + (dict(prune_voxels=3),)
    return c


@functools.lru_cache(maxsize=None)
def case_ref(name):
    ids, m, r2, kw = cases()[name]
    return branches(ids, m, r2, kw.get("prune_voxels", 0), kw.get("prune_rounds", 0))


def call(fn, name, **more):
    """fn = binding.volume_branches_host or an engine's volume_branches, on the named case, the map and the ids asked for"""
    ids, m, r2, kw = cases()[name]
    return fn(ids, m, r2, **dict(dict(want_map=True, want_ids=True), **dict(kw, **more)))


def check(got, name):
    kw = cases()[name][3]
    assert_equal(got, case_ref(name), name, kw.get("cap_nodes", 4096), kw.get("cap_branches", 4096))


def summary(ref):
    """(nodes, ends, junction nodes, junction voxels, isolated, branches, closed, zero-voxel branches, links)"""
    g = ref["graph"]
    tot = lambda f: sum(r[f] for r in g)
    return (tot("nodes"), tot("ends"), tot("junction_nodes"), tot("junction_voxels"), tot("isolated"), tot("branches"), tot("closed"),
            sum(b["kind"] == 2 for b in ref["branches"]), sum(sum(r["links"]) for r in g))


# what the issue's prototype found on the reference skeletons, in summary()'s order; None = not stated
PROTOTYPE = {"y": (4, 3, 1, 1, 0, 3, 0, None, 30), "line": (2, None, None, None, None, 1, None, None, 9), "rod": (2, None, None, None, None, 1, None, None, 31),
             "two_voxels": (2, None, None, None, None, 1, 0, 1, None), "single_voxel": (1, 0, 0, 0, 1, 0, 0, 0, None),
             "torus": (0, 0, 0, 0, 0, 1, 1, 0, 62), "ring": (0, 0, 0, 0, 0, 1, 1, 0, 12), "one_slice": (0, 0, 0, 0, 0, 1, 1, 0, 34),
             "shell": (1, 0, 1, 654, 0, 0, 0, 0, None), "seams": (6, 5, 1, None, None, 4, None, None, 153),
             "tubes_in_contact": (4, 4, 0, 0, 0, 2, None, None, None), "noise": (20, 8, 11, 24, 1, 22, None, 3, 163)}


def invariants(ref, ids_after):
    """what holds on every case: a voxel branch has 0 or 2 attachments (asserted in graph_of), the degrees sum to twice the open
    branches, branch voxels and node voxels are the object voxels"""
    assert sum(nd["degree"] for nd in ref["nodes"]) == 2 * sum(b["kind"] != 1 for b in ref["branches"])
    assert sum(b["voxels"] for b in ref["branches"]) + sum(nd["voxels"] for nd in ref["nodes"]) == int((ids_after > 0).sum())


def assert_not_degenerate():
    """what the named cases must show before any implementation is asked, on this reference alone"""
    refs = {name: case_ref(name) for name in cases()}
    for name, want in PROTOTYPE.items():
        got = summary(refs[name])
        assert all(w is None or w == g for w, g in zip(want, got)), (name, got, want)
    for name, r in refs.items():
        invariants(r, r["ids"])
    every = lambda key: {x["kind"] for r in refs.values() for x in r[key]}
    assert every("nodes") == {0, 1, 2} and every("branches") == {0, 1, 2}
    assert any(b["kind"] == 0 and b["node_a"] == b["node_b"] for r in refs.values() for b in r["branches"])         # a loop back into one cluster
    loop = refs["single_voxel_loop"]
    assert [b["voxels"] for b in loop["branches"] if b["node_a"] == b["node_b"]] == [1] and derive(loop, 1, (1, 1, 1))["loops"] == 1
    assert (derive(refs["lollipop"], 1, (1, 1, 1))["loops"], refs["lollipop"]["graph"][0]["junction_nodes"]) == (1, 1)
    assert (derive(refs["figure_eight"], 1, (1, 1, 1))["loops"], refs["figure_eight"]["graph"][0]["junction_nodes"]) == (2, 1)
    assert max(nd["voxels"] for nd in refs["plus"]["nodes"]) == 5
    s = refs["serpentine"]
    assert summary(s)[:6] == (2, 2, 0, 0, 0, 1) and 550 < s["branches"][0]["voxels"] < 650
    assert max(len({int(v) for v in row[k:k + 64] if v}) for row in cases()["interleaved"][0][0] for k in (0,)) == 2
    block = refs["noise_block"]
    assert sum(g["junction_voxels"] for g in block["graph"]) * 2 > int((cases()["noise_block"][0] > 0).sum())
    assert refs["noise"]["found_nodes"] > 7 and refs["noise"]["found_branches"] > 5                 # the caps of noise_caps_below truncate
    assert [g["nodes"] > 0 for g in refs["absent_ids"]["graph"]] == [True, False, False, False, False, True]
    # pruning: the third arm goes exactly when it is short enough; two rounds; the star collapses
    for length in (1, 2, 3):
        for prune in (1, 2, 3, 4):
            r = refs[f"y_arm{length}_prune{prune}"]
            gone = prune >= length
            assert (r["rounds"], r["stable"], r["graph"][0]["pruned_spurs"], r["graph"][0]["pruned_voxels"]) == (int(gone), 1, int(gone), length * gone)
            assert summary(r)[:6] == ((2, 2, 0, 0, 0, 1) if gone else (4, 3, 1, 1, 0, 3))
    # the comb: a tooth's first voxel belongs to the spine's cluster, so teeth 2, 3 and 4 are spurs of 1, 2 and 3 voxels, tooth 1 is none and
    # tooth 5 is too long; the spine's left end (x = 0 .. 2 before the cluster at x = 3) is a spur of 3 voxels as well
    assert (refs["comb_prune3"]["graph"][0]["pruned_spurs"], refs["comb_prune3"]["graph"][0]["pruned_voxels"]) == (4, 1 + 2 + 3 + 3)
    assert (refs["spur_on_spur"]["rounds"], refs["spur_on_spur"]["stable"]) == (2, 1)
    assert (refs["spur_on_spur_one_round"]["rounds"], refs["spur_on_spur_one_round"]["stable"]) == (1, 0)
    star_ref = refs["star_prune2"]
    assert summary(star_ref)[:6] == (1, 0, 0, 0, 1, 0) and star_ref["graph"][0]["pruned_spurs"] == 3 and int((star_ref["ids"] > 0).sum()) == 1
    assert refs["noise_prune3"]["rounds"] >= 1
