"""GPU: batched selected inversion (Solver.selectedInverse(list) / bsp_selected_inverse_batched_*).
Member q of a batch must be bitwise selectedInverse() of a copy of the same factor, on random
structures and every explicit skeleton of selinv_cases.py, in fp64 and fp32; members are also checked
against inv(A) in correlation units (selinv_ref.py).  The batch must run as one pass over the levels
per chunk (run counters), split into chunks under the testing cap and at the gridDim.y limit, and
stay reproducible, stream-correct and inside its members' bytes."""
import numpy as np
import pytest

import baspacho_amd as B
from baspacho_amd import testing as T
from helpers import solver_random, spd_data, to_dev
from oracle import cref
from selinv_cases import build_case, case_names
from selinv_ref import SkelBuilder, corr_error, dense_reference, lump_path

pytestmark = pytest.mark.gpu

# the bounds of test_selinv_gpu.py / test_selinv_edges_gpu.py
TOL = {np.float64: 2.5e-14, np.float32: 1e-5}
REF_RES = 1e-14
BATCHES = (1, 2, 5, 17)


def _bits(t):
    import torch
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


def _structure(name):
    if name.startswith("random"):
        i = int(name[len("random"):])
        return solver_random(57 + i, find_ranges=bool(i % 2))[0]
    if name == "elim_range":
        return solver_random(58, fill=0.05, elim=(0, 40), ranges=[0, 40])[0]
    return build_case(name)[0]


STRUCTURES = ["random0", "random1", "random2", "random3", "elim_range"] + case_names()


def _factors(sol, n, dtype=np.float64, seed=100):
    """n distinct SPD matrices of `sol`, factored by one batched factor(); (inputs, device factors)"""
    import torch
    datas = [spd_data(sol, seed + q, dtype=dtype) for q in range(n)]
    L = [to_dev(d) for d in datas]
    sol.factor(L)
    torch.cuda.synchronize()
    return datas, L


def _singles(sol, L):
    out = []
    for x in L:
        d = x.clone()
        sol.selectedInverse(d)
        out.append(d)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", STRUCTURES)
def test_bitwise_parity_and_accuracy(name, dtype):
    import torch
    sol = _structure(name)
    datas, L = _factors(sol, max(BATCHES), dtype)
    singles = _singles(sol, L)
    for nb in BATCHES:
        batch = [x.clone() for x in L[:nb]]
        sol.selectedInverse(batch)
        torch.cuda.synchronize()
        for q in range(nb):
            assert _same_bits(batch[q], singles[q]), (name, nb, q)
    # `batch` is the batch of 17 here
    for q in (0, 8, 16):
        _, want, res = dense_reference(sol, datas[q])
        assert res < REF_RES, res
        err = corr_error(sol, batch[q].cpu().numpy().astype(np.float64), want)
        assert err.value < TOL[dtype], (name, q, err)


def _launch_counts(sol):
    c = sol.runCounters()
    return c["selinv_launches"], c["selinv_chunks"]


def test_one_chunk_not_a_host_loop():
    """a batch of 8 enqueues exactly the kernels of ONE single call, in one chunk"""
    import torch
    sol, _, _ = solver_random(60, fill=0.05, elim=(0, 50), ranges=[0, 50])
    _, L = _factors(sol, 8)
    l0, c0 = _launch_counts(sol)
    sol.selectedInverse(L[0].clone())
    l1, c1 = _launch_counts(sol)
    single = l1 - l0
    assert single > 0 and c1 - c0 == 1
    plan = sol._testSelInvPlan()
    assert single >= plan["numLevels"]
    sol.selectedInverse([x.clone() for x in L])
    l2, c2 = _launch_counts(sol)
    assert (l2 - l1, c2 - c1) == (single, 1)
    torch.cuda.synchronize()


def test_chunk_cap_splits_the_batch():
    """cap 3: a batch of 7 runs as 3 chunks (3 + 3 + 1), bitwise equal to the uncapped run"""
    import torch
    sol, _, _ = solver_random(59, fill=0.05, elim=(0, 40), ranges=[0, 40])
    _, L = _factors(sol, 7)
    free = [x.clone() for x in L]
    sol.selectedInverse(free)
    single, chunks = _launch_counts(sol)  # the kernels of one chunk
    assert chunks == 1
    capped = [x.clone() for x in L]
    sol._testSetSelInvBatchChunk(3)
    try:
        l0, c0 = _launch_counts(sol)
        sol.selectedInverse(capped)
        l1, c1 = _launch_counts(sol)
    finally:
        sol._testSetSelInvBatchChunk(0)
    assert c1 - c0 == 3
    assert l1 - l0 == 3 * single
    torch.cuda.synchronize()
    for q in range(7):
        assert _same_bits(capped[q], free[q]), q
    # back to the product's rule: one chunk again
    again = [x.clone() for x in L]
    sol.selectedInverse(again)
    assert _launch_counts(sol)[1] - c1 == 1
    torch.cuda.synchronize()
    for q in range(7):
        assert _same_bits(again[q], free[q]), q


def test_grid_limit_70000_members():
    """70 000 members: more than one chunk (gridDim.y <= 65535), and every member correct.  One lump of
    width 17 (node path) above one of width 2 (small path): both kinds of kernel see gridDim.y at its
    limit.  Members are rows of one tensor; member q is base[q % 7] scaled by c_q, so its inverse is
    the base's divided by c_q"""
    import torch
    b = SkelBuilder()
    head = b.lump([17])
    tail = b.lump([2])
    b.couple(head, tail)
    sol = b.solver()
    plan = sol._testSelInvPlan()
    assert lump_path(plan, head)[0] == "node" and lump_path(plan, tail)[0] == "small"
    n, nb, nbase = sol.dataSize(), 70000, 7
    bases = [spd_data(sol, 300 + i) for i in range(nbase)]
    zb = []
    for data in bases:  # the bases, single calls, against inv(A)
        d = to_dev(data)
        sol.factor(d)
        sol.selectedInverse(d)
        _, want, res = dense_reference(sol, data)
        assert res < REF_RES
        assert corr_error(sol, d.cpu().numpy(), want).value < TOL[np.float64]
        zb.append(d)
    zb = torch.stack(zb)
    c = 1.0 + torch.arange(nb, dtype=torch.float64, device="cuda") / nb
    X = torch.stack([to_dev(x) for x in bases])[torch.arange(nb, device="cuda") % nbase] * c[:, None]
    members = [X[q] for q in range(nb)]
    for q0 in range(0, nb, 5000):
        sol.factor(members[q0:q0 + 5000])
    check = [0, 1, 65533, 65534, 65535, 65536, nb - 1]
    singles = _singles(sol, [members[q] for q in check])
    c0 = _launch_counts(sol)[1]
    sol.selectedInverse(members)
    c1 = _launch_counts(sol)[1]
    torch.cuda.synchronize()
    assert c1 - c0 >= 2, c1 - c0  # 65535 + 4465 (more if device memory is short)
    for q, s in zip(check, singles):
        assert _same_bits(members[q], s), q
    err = ((X * c[:, None] - zb[torch.arange(nb, device="cuda") % nbase]).abs().amax(dim=1) /
           zb.abs().amax()).max().item()
    assert err < 1e-12, err


def test_reproducible_and_streams():
    """two batched runs on copies are bitwise identical, and so is a run on a non-default stream"""
    import torch
    sol, _, _ = solver_random(58, fill=0.05, elim=(0, 40))
    _, L = _factors(sol, 5)
    a = [x.clone() for x in L]
    b = [x.clone() for x in L]
    d = [x.clone() for x in L]
    sol.selectedInverse(a)
    sol.selectedInverse(b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sol.setStream(s)
    try:
        with torch.cuda.stream(s):
            sol.selectedInverse(d)
        s.synchronize()
    finally:
        sol.setStream(None)
    for q in range(5):
        assert _same_bits(a[q], b[q]), q
        assert _same_bits(a[q], d[q]), q


def test_bytes_outside_the_members_untouched():
    """members are slices of one buffer with guard regions between them: only the members change"""
    import torch
    sol, _, _ = solver_random(61, fill=0.05, elim=(0, 50), ranges=[0, 50])
    nb, n, pad = 6, sol.dataSize(), 37
    _, L = _factors(sol, nb)
    singles = _singles(sol, L)
    buf = torch.full((pad + nb * (n + pad),), -1.2345e-300, dtype=torch.float64, device="cuda")
    buf[:pad] = float("nan")
    members = []
    for q in range(nb):
        m = buf[pad + q * (n + pad):pad + q * (n + pad) + n]
        m.copy_(L[q])
        members.append(m)
    before = buf.clone()
    sol.selectedInverse(members)
    torch.cuda.synchronize()
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    for q in range(nb):
        inside[pad + q * (n + pad):pad + q * (n + pad) + n] = True
        assert _same_bits(members[q], singles[q]), q
    assert torch.equal(_bits(buf)[~inside], _bits(before)[~inside])


def test_marginals_of_a_batch():
    import torch
    sol, ps, _ = solver_random(58, fill=0.05, elim=(0, 40))
    _, L = _factors(sol, 3)
    sol.selectedInverse(L)
    torch.cuda.synchronize()
    params = list(range(len(ps)))
    m = sol.marginals(L, params)
    assert isinstance(m, list) and len(m) == 3
    for q in range(3):
        one = sol.marginals(L[q], params)
        assert len(m[q]) == len(one)
        for x, y in zip(m[q], one):
            assert _same_bits(x, y)
    same = [p for p in params if ps[p] == ps[0]]
    m = sol.marginals(tuple(L), same)
    assert tuple(m.shape) == (3, len(same), int(ps[0]), int(ps[0]))
    for q in range(3):
        assert _same_bits(m[q], sol.marginals(L[q], same))


def test_bal_shaped_batch_of_two():
    """a reduced bundle-adjustment problem with its point range: many small lumps with many chains (the
    small-lump kernel) and the camera nodes; a batch of 2 is bitwise the two single calls"""
    import torch
    num_pts = 3000
    sizes, ss, _, _ = T.gen_bal_synthetic(num_cams=40, num_pts=num_pts, band=6, seed=3)
    sol = B.create_solver(B.Settings(), sizes, ss, [0, num_pts])
    plan = sol._testSelInvPlan()
    assert len(plan["small"]["lump"]) > num_pts // 2 and len(plan["node"]["lump"]) > 0
    idx = sol.skel()["chainData"][sol.skel()["chainColPtr"][:-1]]
    L = []
    for seed in (37, 38):
        h = T.random_data(sol.dataSize(), -1.0, 1.0, seed)
        w = np.diff(sol.skel()["lumpStart"]).astype(np.int64)
        rep = np.repeat(np.arange(len(w)), w)
        within = np.arange(int(w.sum())) - np.repeat(np.cumsum(w) - w, w)
        diag = idx[rep] + within * (w[rep] + 1)
        h[diag] = 1.05 * cref.abs_row_sums(sol.skel(), h) + 1e-3
        L.append(torch.from_numpy(h).cuda())
    sol.factor(L)
    singles = _singles(sol, L)
    sol.selectedInverse(L)
    torch.cuda.synchronize()
    for q in range(2):
        assert torch.isfinite(L[q]).all().item()
        assert _same_bits(L[q], singles[q]), q
