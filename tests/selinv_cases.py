"""Explicit skeletons at the split points of the selected-inversion plan (buildSelInvPlan).  Every case
returns (solver, expect): expect(plan) asserts, on Solver._testSelInvPlan(), that the shape takes the
path it was built for.  Used by test_selinv_plan_cpu.py (plan only) and test_selinv_edges_gpu.py
(plan and values)."""
import numpy as np

from selinv_ref import SkelBuilder, lump_path, split_sizes

SMALL_W, SMALL_CHAINS, SMALL_ELEMS, NODE_W = 16, 16, 512, 64


def _one_lump(n, below_sizes, head_spans=None):
    """lump 0 (width n) above one lump holding the given chain spans"""
    b = SkelBuilder()
    head = b.lump(head_spans or [n])
    if below_sizes:
        tail = b.lump(below_sizes)
        b.couple(head, tail)
    return b.solver(), head


def _expect_path(head, path, n, k, r):
    def expect(plan):
        kind, rec = lump_path(plan, head)
        assert kind == path, (kind, rec)
        if kind == "small":
            assert (rec["n"], rec["k"], rec["r"]) == (n, k, r), rec
        else:
            assert sum(x["w"] for x in rec) == n and rec[-1]["c0"] == 0, rec
            assert rec[-1]["r"] == (n - rec[-1]["w"]) + r, rec
    return expect


# (name, n, chain sizes below, path): both sides of each limit of the small path
SMALL_LIMITS = [
    ("at_all_limits", 16, [2] * 16, "small"),
    ("n17_k1", 17, [1], "node"),
    ("n1_17_chains", 1, [1] * 17, "node"),
    ("n1_16_chains", 1, [1] * 16, "small"),
    ("n1_r513", 1, [33] * 15 + [18], "node"),
    ("n1_r512", 1, [32] * 16, "small"),
    ("n3_r171", 3, [11] * 15 + [6], "node"),
    ("n3_r170", 3, [11] * 15 + [5], "small"),
    ("n16_r33", 16, [3] * 11, "node"),
    ("n16_r32_k17", 16, [2] * 15 + [1, 1], "node"),
    ("n1_alone", 1, [], "small"),
    ("n16_alone", 16, [], "small"),
    ("n17_alone", 17, [], "node"),
]


def small_limit_case(name):
    _, n, below, path = next(c for c in SMALL_LIMITS if c[0] == name)
    sol, head = _one_lump(n, below)
    return sol, _expect_path(head, path, n, len(below), sum(below))


NODE_WIDTHS = [17, 63, 64, 65, 128, 129, 200]
NODE_ROWS = [0, 1, 63, 64, 65, 127, 128, 129]
MIXED = list(range(1, 24))


def node_width_case(width):
    """one skeleton per lump width: independent pairs (lump of `width`, spans of sizes 1..23 mixed;
    lump of r rows below it) for every r of NODE_ROWS"""
    b = SkelBuilder()
    heads = []
    for i, r in enumerate(NODE_ROWS):
        h = b.lump(split_sizes(width, MIXED[i:] + MIXED[:i]))
        if r:
            t = b.lump(split_sizes(r, MIXED[::-1]))
            b.couple(h, t)
        heads.append((h, r))

    def expect(plan):
        for h, r in heads:
            kind, nodes = lump_path(plan, h)
            assert kind == "node", (width, r)
            ws = [x["w"] for x in nodes]
            assert ws[0] == (width - 1) % NODE_W + 1 and all(w == NODE_W for w in ws[1:]), ws
            assert [x["c0"] for x in nodes] == [NODE_W * j for j in range(len(ws))][::-1]
            assert nodes[0]["r"] == r
            assert [x["nTiles"] for x in nodes] == [-(-x["r"] // 64) for x in nodes]
        # ragged rightmost node and a node boundary inside a span, where the widths make them
        if width % NODE_W:
            assert any(lump_path(plan, h)[1][0]["w"] < NODE_W for h, _ in heads)
        if width > NODE_W:
            assert any(_cut_spans(sol, h) for h, _ in heads), "no span crosses a node boundary"
    sol = b.solver()
    return sol, expect


def _cut_spans(sol, lump):
    """spans of a lump cut by a node boundary (c0 = 64 k inside the span)"""
    sk = sol.skel()
    ls, ss, l2s = sk["lumpStart"], sk["spanStart"], sk["lumpToSpan"]
    out = []
    for s in range(int(l2s[lump]), int(l2s[lump + 1])):
        a, e = int(ss[s] - ls[lump]), int(ss[s + 1] - ls[lump])
        if (a // NODE_W) != ((e - 1) // NODE_W):
            out.append(s)
    return out


def big_param_case():
    """one parameter of size 100: a span cut by the node boundary at column 64"""
    b = SkelBuilder()
    h = b.lump([100])
    t = b.lump([5, 7, 3])
    b.couple(h, t)
    sol = b.solver()

    def expect(plan):
        kind, nodes = lump_path(plan, h)
        assert kind == "node" and [x["w"] for x in nodes] == [36, 64]
        assert _cut_spans(sol, h) == [0]
    return sol, expect


SPLITK_ROWS = [511, 512, 513, 1000, 2049]


def split_k_case(r, crowded):
    """node(s) of width 2 above one lump of r rows (spans of 7, so never small).  crowded=False: one
    node alone in its level, so the level's Z_RR U product is split along K where r allows it;
    crowded=True: enough nodes on the same level for >= 512 tiles, so nk == 1"""
    b = SkelBuilder()
    tiles = -(-r // 64)
    n_heads = -(-512 // tiles) if crowded else 1
    heads = [b.lump([2]) for _ in range(n_heads)]
    t = b.lump(split_sizes(r, [7]))
    for h in heads:
        b.couple(h, t)

    def expect(plan):
        recs = [lump_path(plan, h) for h in heads]
        assert all(k == "node" and len(nd) == 1 for k, nd in recs)
        nd = recs[0][1][0]
        lvl = plan["node"]["level"] == nd["level"]
        assert (plan["node"]["lump"][lvl] < len(heads)).all()  # the heads only
        assert int(plan["node"]["nTiles"][lvl].sum()) == n_heads * tiles
        assert nd["r"] == r
        if crowded:
            assert n_heads * tiles >= 512 and nd["nk"] == 1, nd
        elif r >= 512:
            assert nd["nk"] > 1, nd
            last = r - (nd["nk"] - 1) * nd["kChunk"]
            assert 0 < last <= nd["kChunk"], nd
            if r % nd["kChunk"]:
                assert last < nd["kChunk"]
        else:
            assert nd["nk"] == 1, nd
    return b.solver(), expect


def many_chains_case():
    """a lump with 210 chains (one-row spans in three lumps, which fill among themselves)"""
    b = SkelBuilder()
    h = b.lump([4])
    tails = [b.lump([1] * 70) for _ in range(3)]
    b.couple(h, *tails)

    def expect(plan):
        kind, nodes = lump_path(plan, h)
        assert kind == "node" and nodes[0]["r"] == 210
    return b.solver(), expect


def mixed_owners_case():
    """chain rows owned by small lumps and by a node lump in the same column"""
    b = SkelBuilder()
    h = b.lump(split_sizes(70, [3, 5]))
    s1 = b.lump([2])
    s2 = b.lump([3])
    big = b.lump(split_sizes(80, [9, 11]))
    b.couple(h, s1, s2, big)

    def expect(plan):
        assert lump_path(plan, h)[0] == "node"
        assert lump_path(plan, s1)[0] == "small" and lump_path(plan, s2)[0] == "small"
        assert lump_path(plan, big)[0] == "node"
    return b.solver(), expect


def forest_case():
    """independent trees with roots at different depths: small items and nodes share levels, also
    past level 0.  (A node with r = 0 is the rightmost block of a lump with nothing below: level 0,
    where every node has r = 0; the plan test asserts that, so such levels cannot mix.)"""
    b = SkelBuilder()
    # tree 1: a chain of 6 small lumps
    chain = [b.lump([2]) for _ in range(6)]
    for a, c in zip(chain, chain[1:]):
        b.couple(a, c)
    # tree 2: a node child below a wide root (3 nodes)
    child = b.lump(split_sizes(40, [4]))
    root2 = b.lump(split_sizes(150, [6, 1]))
    b.couple(child, root2)
    # tree 3: small child below a small root
    c3 = b.lump([5])
    r3 = b.lump([3, 3])
    b.couple(c3, r3)
    # tree 4: a lone wide lump (r = 0 on its one node)
    lone = b.lump([30, 20])

    def expect(plan):
        sl, nl = set(plan["small"]["level"].tolist()), set(plan["node"]["level"].tolist())
        assert sl & nl, "no level holds small items and nodes"
        assert {l for l in sl & nl if l > 0}, "no level past the roots holds small items and nodes"
        assert lump_path(plan, lone)[0] == "node"
    return b.solver(), expect


def all_cases():
    """(name, builder) of every explicit case"""
    out = [("small/" + c[0], (lambda nm=c[0]: small_limit_case(nm))) for c in SMALL_LIMITS]
    out += [("width%d" % w, (lambda w=w: node_width_case(w))) for w in NODE_WIDTHS]
    out += [("param100", big_param_case)]
    out += [("splitk%d%s" % (r, "_crowded" if c else ""), (lambda r=r, c=c: split_k_case(r, c)))
            for r in SPLITK_ROWS for c in (False, True)]
    out += [("chains210", many_chains_case), ("mixed_owners", mixed_owners_case), ("forest", forest_case)]
    return out


def case_names():
    return [n for n, _ in all_cases()]


def build_case(name):
    return dict(all_cases())[name]()
