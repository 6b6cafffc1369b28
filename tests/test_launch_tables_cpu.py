"""Host derivations of the launch paths (csrc/hip_plan.cpp), checked without a GPU: the launch tables
the factor uploads beside its plan (buildLaunchTables: self-contained task records, split-K lists, the
potrf-fold order) and the steps of the dense part of a solve (buildSolveSchedule: levels, block groups,
persistent sweeps, inverse slots).  Solver._testLaunchTables / _testSolveSchedule dump what the launch
code itself would build for the plan over every lump."""
import numpy as np
import pytest

from kf_structures import bipartite, blocks_over_separator, dense_solver

LAZY = {"lazy_plan": 1}
UPD_CHUNK, SPLIT_MIN_K, SPLIT_K, SPLIT_MAX_TILES, FOLD_MAX_TILES = 32, 128, 96, 512, 512
SEG_INTRA = 0
SWEEP_W, SWEEP_FAR_ROWS, PANEL, OUTER = 192, 48, 64, 256

STRUCTURES = {
    "sep_even": lambda: blocks_over_separator([130, 130, 200, 200], 150, hip_options=LAZY),
    "sep_ragged": lambda: blocks_over_separator([130, 97, 200, 70], 150, hip_options=LAZY),
    "dense1600": lambda: dense_solver(1600, hip_options=LAZY),   # tail levels
    "dense64": lambda: dense_solver(64, hip_options=LAZY),
    "dense65": lambda: dense_solver(65, hip_options=LAZY),
    "bipartite": lambda: bipartite(60, 12, 3, 9, 5, hip_options=LAZY),  # an elimination range (3-wide points)
    # ... and one whose points are wider than the small-lump kernels take: the range has bigLevels
    "bipartite_wide": lambda: bipartite(12, 4, 20, 9, 5, hip_options=LAZY),
}
_tables = {}


def tables(name):
    if name not in _tables:
        _tables[name] = STRUCTURES[name]()._testLaunchTables()
    return _tables[name]


def rows(table, idx):
    return {f: v[idx] for f, v in table.items()}


def main_levels(t):
    lv = t["levels"]
    main = np.flatnonzero(lv["range"] == -1)
    assert len(main) == t["numMainLevels"] and np.array_equal(main, np.arange(len(lv["range"]) - len(main), len(lv["range"])))
    return {f: v[main] for f, v in lv.items()}


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_sizes_and_slow_prefix(name):
    t = tables(name)
    n = t["numUpdTasks"]
    fat, wide, slow = t["updTasksFat"], t["updTasksWide"], t["slowPrefix"]
    assert len(fat["K"]) == n and len(wide["K"]) == n and len(slow) == n + 1
    if name == "bipartite_wide":
        assert (t["levels"]["range"] >= 0).any()
    assert len(t["levelPanelDescs"]["nb"]) == t["numLevelPanels"]
    assert len(t["trsmTasksFat"]["nb"]) == t["numTrsmTasks"]
    assert slow[0] == 0
    step = np.diff(slow)
    fast = (wide["kind"] == SEG_INTRA) & (wide["K"] > 0) & (wide["K"] % UPD_CHUNK == 0)
    assert np.array_equal(step == 0, fast) and np.array_equal(step == 1, ~fast)
    assert np.array_equal(fat["fast"], fast.astype(np.int64))
    for f in ("srcOff", "tgtBase", "lda", "K", "rowsBelow", "segEnd", "rowTile", "colTile", "tgtStride", "rowMin",
              "atomic"):
        assert np.array_equal(fat[f], wide[f]), f


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_fold_order(name):
    t = tables(name)
    lv, lp = main_levels(t), t["levelPanelDescs"]
    tiles = lv["trsmEnd"] - lv["trsmBegin"]
    cand = []
    for li in range(t["numMainLevels"]):
        pb, pe = int(lv["panelBegin"][li]), int(lv["panelEnd"][li])
        if (lv["tail"][li] == 0 and lv["directPanel"][li] < 0 and pe > pb and 1 <= tiles[li] <= FOLD_MAX_TILES
                and (lp["rowsBelow"][pb:pe] > 0).all()):
            cand.append(li)
    rank = t["foldRank"]
    assert len(rank) == t["numMainLevels"]
    assert sorted(np.flatnonzero(rank >= 0).tolist()) == cand
    order = sorted(cand, key=lambda li: int(rank[li]))
    assert [int(rank[li]) for li in order] == list(range(len(cand)))
    assert np.array_equal(t["foldTiles"], tiles[order])
    assert (np.diff(t["foldTiles"]) >= 0).all()
    for a, b in zip(order, order[1:]):
        assert tiles[a] < tiles[b] or a < b    # ties in level order
    counts = [int(lv["panelEnd"][li] - lv["panelBegin"][li]) for li in order]
    assert np.array_equal(t["foldPanelEnd"], np.cumsum(counts, dtype=np.int64))
    idx = [q for li in order for q in range(int(lv["panelBegin"][li]), int(lv["panelEnd"][li]))]
    for f, v in t["foldDescs"].items():
        assert np.array_equal(v, lp[f][idx]), f
    for batch in (1, 2, 8, 64, 512):
        fits = [tiles[li] * batch <= FOLD_MAX_TILES for li in order]
        assert fits == sorted(fits, reverse=True)   # a prefix of the order
    if name == "sep_ragged":
        assert len(set(t["foldTiles"].tolist())) >= 2


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_split_lists(name):
    t = tables(name)
    lv, wide, split = t["levels"], t["updTasksWide"], t["updTasksSplit"]
    ranges = {int(u): (int(b), int(e)) for u, b, e in zip(*(t["splitRange"][f] for f in ("updBegin", "begin", "end")))}
    assert len(ranges) == len(t["splitRange"]["updBegin"])
    pieces_of = lambda k: -(-k // SPLIT_K)
    expected, split_tiles = set(), 0
    for li in range(len(lv["range"])):
        ub, ue = int(lv["updBegin"][li]), int(lv["updEnd"][li])
        n, K = ue - ub, wide["K"][ub:ue]
        big = K >= SPLIT_MIN_K
        after = n + sum(pieces_of(int(k)) - 1 for k in K[big])
        if not (lv["directPanel"][li] < 0 and 1 <= n <= SPLIT_MAX_TILES and big.any() and after <= 2 * SPLIT_MAX_TILES):
            continue
        assert ub not in expected
        expected.add(ub)
        assert ub in ranges
        pos, end = ranges[ub]
        assert end - pos == after
        for i in range(ub, ue):
            tile = rows(wide, i)
            if tile["K"] < SPLIT_MIN_K:
                assert rows(split, pos) == tile
                pos += 1
                continue
            m = pieces_of(int(tile["K"]))
            split_tiles += 1
            for j in range(m):
                piece = rows(split, pos + j)
                assert piece["K"] <= SPLIT_K
                assert piece["srcOff"] == tile["srcOff"] + SPLIT_K * j and piece["atomic"] == tile["atomic"] | 1
                for f in tile:
                    if f not in ("K", "srcOff", "atomic"):
                        assert piece[f] == tile[f], f
            assert split["K"][pos:pos + m].sum() == tile["K"]
            pos += m
        assert pos == end
    assert set(ranges) == expected
    spans = sorted(ranges.values())
    assert [b for b, _ in spans] == [0] * bool(spans) + [e for _, e in spans[:-1]]
    assert (spans[-1][1] if spans else 0) == len(split["K"])
    if name == "sep_even":
        assert ranges and split_tiles >= 1


# ---- solve schedule ------------------------------------------------------------------------------------
SCHED = {
    "dense64": (lambda: dense_solver(64, hip_options=LAZY), 768),
    "dense100": (lambda: dense_solver(100, hip_options=LAZY), 768),
    "dense700": (lambda: dense_solver(700, hip_options=LAZY), 768),
    "dense1600": (lambda: dense_solver(1600, hip_options=LAZY), 768),
    "sep_even": (lambda: blocks_over_separator([130, 130, 200, 200], 150, hip_options=LAZY), 768),
}
_solvers = {}


def schedule(name, sweeps, block, inverses):
    if name not in _solvers:
        _solvers[name] = SCHED[name][0]()
    return _solvers[name]._testSolveSchedule(sweeps, block, inverses, SCHED[name][1])


@pytest.mark.parametrize("inverses", [False, True])
@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("sweeps", [False, True])
@pytest.mark.parametrize("name", sorted(SCHED))
def test_solve_schedule(name, sweeps, block, inverses):
    """(block solve off: no block groups, and every item that is not a sweep is a single level -- the
    launch code asks for sweeps only with block solve on, the builder does not couple the two)"""
    s = schedule(name, sweeps, block, inverses)
    lv, it = s["levels"], s["items"]
    n_lv, n_it = len(lv["panels"]), len(it["kind"])
    min_width = SCHED[name][1]
    # cover: contiguous, no overlap
    assert n_it > 0 and it["l"][0] == 0 and it["e"][-1] == n_lv
    assert (it["e"] > it["l"]).all() and np.array_equal(it["e"][:-1], it["l"][1:])
    slot, xchg, sweep_w, sweep_below, wgs, wgs_m, groups = 0, 0, [], [], [], [], []
    for i in range(n_it):
        kind, l, e = int(it["kind"][i]), int(it["l"][i]), int(it["e"][i])
        lump, col, nb = lv["lump"][l:e], lv["col"][l:e], lv["nb"][l:e]
        if kind == 0:
            assert e - l == 1 and it["slot"][i] == -1
            continue
        assert (lv["panels"][l:e] == 1).all() and (lump == lump[0]).all() and lump[0] >= 0
        if kind == 1:
            assert block and 2 <= e - l <= 4
            assert col[0] % OUTER == 0 and (np.diff(col) == PANEL).all() and col[-1] < col[0] + OUTER
            assert (it["slot"][i] >= 0) == inverses
            groups.append(e - l)
        else:
            assert kind == 2 and sweeps
            w = int(nb.sum())
            assert w == it["w"][i] and w >= min_width
            assert (nb[:-1] == PANEL).all() and np.array_equal(col[1:], col[:-1] + nb[:-1])
            nblk = -(-w // SWEEP_W)
            assert it["nBlocks"][i] == nblk and it["rowsBelow"][i] == lv["rowsBelow"][e - 1]
            assert it["xchgOff"][i] == xchg and it["invSlot"][i] == it["slot"][i] and it["slot"][i] >= 0
            xchg += 2 * nblk * SWEEP_W
            fwd = 5 * nblk + -(-int(it["rowsBelow"][i]) // SWEEP_FAR_ROWS)
            assert it["fwdWgs"][i] == fwd and it["bwdWgs"][i] == 4 * nblk
            sweep_w.append(w)
            sweep_below.append(int(it["rowsBelow"][i]))
            wgs.append(max(fwd, 4 * nblk))
            wgs_m.append(max(fwd, 5 * nblk))
        if it["slot"][i] >= 0:
            assert it["slot"][i] == slot
            for f in ("lump", "col", "nb", "rowsBelow"):
                assert np.array_equal(s["invPanels"][f][slot:slot + e - l], lv[f][l:e]), f
            slot += e - l
    assert slot == len(s["invPanels"]["lump"])
    assert s["numSweeps"] == len(sweep_w) and s["sweepInstStride"] == xchg
    assert s["maxSweepW"] == max(sweep_w, default=0) and s["maxSweepBelow"] == max(sweep_below, default=0)
    assert s["maxSweepWgs"] == max(wgs, default=0) and s["maxSweepWgsM"] == max(wgs_m, default=0)
    if not sweeps:
        assert s["numSweeps"] == 0
    if not block:
        assert not groups
    if name == "dense700":
        assert s["numSweeps"] == 0
        if block:
            assert groups == [4, 4, 3]
    if name == "dense1600" and sweeps:
        assert s["numSweeps"] >= 1
