"""Solver structures shared by the known-factor GPU tests (tests/test_known_factor_gpu.py,
tests/test_partial_factor_gpu.py): each builds a Solver on the host; nothing here touches the GPU."""
import numpy as np

import baspacho_amd as B
from baspacho_amd import testing as T


def dense_solver(W, span=8, hip_options=None):
    sizes = [span] * (W // span) + ([W % span] if W % span else [])
    cols = [list(range(c, len(sizes))) for c in range(len(sizes))]
    st = B.Settings(findSparseEliminationRanges=False, hipOptions=hip_options)
    return B.create_solver(st, np.asarray(sizes, dtype=np.int64), T.columns_to_structure(cols), [])


def blocks_over_separator(widths, sep, hip_options=None):
    """independent dense blocks over a common separator (levels of several panels)"""
    n = sum(widths) + sep
    cols, base = [], 0
    for w in widths:
        for i in range(w):
            cols.append(set(range(base + i, base + w)) | set(range(n - sep, n)))
        base += w
    for i in range(sep):
        cols.append(set(range(n - sep + i, n)))
    return B.create_solver(B.Settings(hipOptions=hip_options), np.ones(n, dtype=np.int64),
                           T.columns_to_structure(cols))


def bipartite(num_pts, num_cams, pt_size, cam_size, seed, track=4, hip_options=None, ranges=None):
    """points (eliminated, pt_size wide) seen by `track` cameras (cam_size rows per block) each, and the
    point range [0, num_pts) as the given elimination range (`ranges`: given boundaries instead, from
    0 to num_pts; the points are independent, so any cut of them is a valid set of ranges)"""
    rng = np.random.default_rng(seed)
    pt = np.repeat(np.arange(num_pts, dtype=np.int64), track)
    cam = rng.integers(0, num_cams, size=num_pts * track)
    key = np.unique(pt * num_cams + cam)
    pt, cam = key // num_cams, key % num_cams
    sizes = np.concatenate([np.full(num_pts, pt_size, dtype=np.int64), np.full(num_cams, cam_size, dtype=np.int64)])
    ss = T.structure_from_pairs(num_pts + num_cams, num_pts + cam, pt)
    return B.create_solver(B.Settings(hipOptions=hip_options), sizes, ss,
                           [0, num_pts] if ranges is None else list(ranges))


def random_with_range(seed, hip_options=None):
    """a random structure whose first 150 parameters are an independent elimination range, with several
    dense lumps behind it (lump boundaries for the partial solves)"""
    cols = T.make_independent_elim_set(T.random_cols(300, 0.03, seed), 0, 150)
    sizes = np.random.default_rng(seed).integers(1, 5, size=300).astype(np.int64)
    return B.create_solver(B.Settings(hipOptions=hip_options), sizes, T.columns_to_structure(cols), [0, 150])


def _spans(width, span):
    return [span] * (width // span) + ([width % span] if width % span else [])


def lump_over_lump(top, below, top_span=8, below_span=7, hip_options=None):
    """two dense lumps, `top` columns above `below` columns: every span of the top lump sees about three
    quarters of the lower lump's spans (so the two are not merged), and the lower lump's parameters are
    placed last (the lower lump is the root)"""
    sizes = _spans(top, top_span)
    n0 = len(sizes)
    sizes = sizes + _spans(below, below_span)
    nparam = len(sizes)
    cols = [list(range(c, n0)) + [q for q in range(n0, nparam) if (q + c) % 4 != 0] for c in range(n0)]
    cols += [list(range(c, nparam)) for c in range(n0, nparam)]
    st = B.Settings(findSparseEliminationRanges=False, hipOptions=hip_options)
    sol = B.create_solver(st, np.asarray(sizes, dtype=np.int64), T.columns_to_structure(cols), [],
                          list(range(n0, nparam)))
    assert list(sol.skel()["lumpStart"]) == [0, top, top + below], sol.skel()["lumpStart"]
    return sol


def affine_plane_cameras(p, pt_size, cam_size, extra=0, extra_size=7):
    """bundle-adjustment shape: p * p cameras (the points of the affine plane over Z_p) and one point
    per line of that plane (p * p + p points, eliminated as the range [0, points)), seen by the p
    cameras on its line.  Every pair of cameras shares exactly one point, so the cameras form one dense
    lump of p * p * cam_size columns; `extra` further parameters, seen by about three quarters of the
    cameras each and placed last, form the dense lumps behind it."""
    lines = [[x * p + (m * x + b) % p for x in range(p)] for m in range(p) for b in range(p)]
    lines += [[c * p + y for y in range(p)] for c in range(p)]
    P, C = len(lines), p * p
    cams0, extra0 = P, P + C
    n = extra0 + extra
    cols = [{q} | {cams0 + c for c in line} for q, line in enumerate(lines)]
    cols += [set(range(cams0 + c, extra0)) | {q for q in range(extra0, n) if (q + c) % 4 != 0}
             for c in range(C)]
    cols += [set(range(q, n)) for q in range(extra0, n)]
    sizes = np.concatenate([np.full(P, pt_size, dtype=np.int64), np.full(C, cam_size, dtype=np.int64),
                            np.full(extra, extra_size, dtype=np.int64)])
    return B.create_solver(B.Settings(), sizes, T.columns_to_structure(cols), [0, P],
                           list(range(extra0, n)))


def reach_widths():
    """a chain of lumps of width 1, 16, 63, 64 (below the cut of the reach plan), 65 (the cut) and 7 (behind
    it), each coupled to the next two; spans of width 1, 16 and 17, lumps of several spans"""
    from selinv_ref import SkelBuilder
    b = SkelBuilder()
    lumps = [b.lump([1]), b.lump([16]), b.lump([17, 5, 16, 1, 24]), b.lump([7, 17, 40]), b.lump([30, 35]),
             b.lump([4, 3])]
    for i, l in enumerate(lumps):
        if lumps[i + 1:i + 3]:
            b.couple(l, *lumps[i + 1:i + 3])
    return b.solver()


def counter_delta(sol, name, fn):
    before = sol.runCounters()[name]
    fn()
    return sol.runCounters()[name] - before
