"""CPU: the history harness (tests/history.py) is shown to catch what it is for, and the committed walks
are shown to cover what they must.  No GPU: a small fake solver of pure Python runs the committed walks
under a vocabulary of the real operations' names.

The fake keeps three kinds of state between calls, each with a clean and a leaky variant:
  scratch   values staged in a buffer that only grows; the "kernel" reads 8 elements past the call's own.
            Clean: those are cleared for every call.  Leak: only the call's own elements are armed, so a
            smaller call after a larger one reads stale values.
  table     a table per (nRHS, dtype).  Leak: the cache is keyed by nRHS alone and hands the float64 table
            to a float32 call.
  flag      a mode flag set for the duration of a call.  Leak: a call that raises leaves it set.
Every leak stays inside the tolerance of the fake's own check: only the bitwise veteran / fresh
comparison of run_history can see it (test_the_leaks_pass_without_the_comparison)."""
import ast
import re

import numpy as np
import pytest

import history as H

TOL = {H.F64: 1e-10, H.F32: 1e-4}        # of the fake's check, relative to sum |x| max |t|
EPS = {H.F64: 2.0 ** -40, H.F32: 2.0 ** -20}  # weight of the staged values in the result


def _table(nrhs, dtype):
    return ((np.arange(nrhs) + 1.0) / 3.0).astype(dtype)


class FakeSolver:
    def __init__(self, leak=None):
        self.leak = leak
        self.scratch = np.zeros(0)
        self.tables = {}
        self.reverse = False

    def _table(self, nrhs, dtype):
        if self.leak != "table":
            return self.tables.setdefault((nrhs, dtype), _table(nrhs, dtype))
        if dtype == H.F64:
            return self.tables.setdefault(nrhs, _table(nrhs, dtype))
        return self.tables.get(nrhs, _table(nrhs, dtype))  # LEAK: the float64 table of an earlier call

    def call(self, x, nrhs, fail=False):
        """out[j] = sum_i x_i t_j + eps * sum of the staged values (the call's own x, then 8 cleared ones)"""
        dtype, n = x.dtype, x.size
        stuck = self.reverse  # set on entry only when an earlier call left it behind
        self.reverse = True   # (a mode for the duration of the call)
        try:
            if fail:
                raise ValueError("fake: refused")
            if self.scratch.size < n + 8:
                self.scratch = np.concatenate([self.scratch, np.zeros(n + 8 - self.scratch.size)])
            self.scratch[:n] = x.ravel()
            if self.leak != "scratch":
                self.scratch[n:n + 8] = 0.0  # (LEAK: left as an earlier, larger call wrote them)
            t = self._table(nrhs, dtype)
            acc = np.zeros(nrhs, dtype=t.dtype)
            for v in (x.ravel()[::-1] if stuck else x.ravel()):  # (the order of the sum)
                acc = acc + v * t
            return (acc + EPS[dtype] * self.scratch[:n + 8].sum()).astype(dtype)
        finally:
            if not (self.leak == "flag" and (fail or stuck)):  # LEAK: the flag survives a call that raised,
                self.reverse = False                           # and nothing clears it afterwards


def _fake_call(solver, x, nrhs, fail=False):
    return solver.call(x, nrhs, fail)


def _build(solver, dtype, batch, nrhs, seed):
    x = np.random.default_rng(seed).standard_normal((batch, 5 + nrhs)).astype(dtype)
    return {"x": x, "nrhs": nrhs, "dtype": np.dtype(dtype)}


def _run(solver, i):
    x0 = i["x"].copy()
    return {"out": _fake_call(solver, i["x"], i["nrhs"]), "_readonly": [("x", i["x"], x0)]}


def _check(i, o):
    x, t = i["x"].astype(np.float64), _table(i["nrhs"], i["dtype"]).astype(np.float64)
    want = x.sum() * t + EPS[i["dtype"]] * x.sum()
    err = np.abs(o["out"].astype(np.float64) - want).max() / (np.abs(x).sum() * np.abs(t).max())
    assert err < TOL[i["dtype"]], err
    return {"fake": err / TOL[i["dtype"]]}


def _run_refused(solver, i):
    with pytest.raises(ValueError):
        _fake_call(solver, i["x"], i["nrhs"], fail=True)
    return {}


def _fake_vocabulary():
    out = []
    for op in H.VOCABULARY:
        if op.control:
            out.append(H.Op(op.name, op.family, lambda *a: {}, lambda s, i: {}, lambda i, o: {}, control=True))
        elif op.family == "error":
            out.append(H.Op(op.name, op.family, _build, _run_refused, lambda i, o: {}))
        else:
            out.append(H.Op(op.name, op.family, _build, _run, _check, bitwise=("out",), uses_batch=op.uses_batch,
                            uses_nrhs=op.uses_nrhs))
    return out


FAKE = _fake_vocabulary()
LEAKS = ["scratch", "table", "flag"]


def _walks():
    return [(name, seed, steps) for name, ws in H.committed_walks(FAKE).items() for seed, steps in ws]


def _run_fake(steps, leak, **kw):
    return H.run_history(lambda: FakeSolver(leak), steps, hooks=H.HostHooks, **kw)


def test_the_fake_vocabulary_gets_the_walks_of_the_real_one():
    real = H.committed_walks()
    fake = H.committed_walks(FAKE)
    assert set(real) == set(H.STRUCTURES) == set(H.WALK_SEEDS)
    for name in real:
        assert len(real[name]) >= 2
        for (s0, a), (s1, b) in zip(real[name], fake[name]):
            assert s0 == s1 and H.describe(a) == H.describe(b) and len(a) == H.WALK_LENGTH
    steps = real["tail"][0][1]
    assert H.describe(H.parse(H.VOCABULARY, H.describe(steps))) == H.describe(steps)


def test_the_clean_fake_passes_every_committed_walk():
    report = {}
    for name, seed, steps in _walks():
        _run_fake(steps, None, tag="%s/%d" % (name, seed), report=report)
    assert report and all({"veteran", "fresh"} <= set(v) for v in report.values())


@pytest.mark.parametrize("leak", LEAKS)
def test_each_leak_fails_and_the_message_reproduces_it(leak):
    caught = {}
    for name, seed, steps in _walks():
        with_leak = None
        try:
            _run_fake(steps, leak, tag="%s/%d" % (name, seed))
        except H.HistoryError as e:
            with_leak = str(e)
        if with_leak is None:
            continue
        caught.setdefault(name, []).append(seed)
        # the message names the walk, the step and the steps up to it ...
        m = re.search(r"history %s/%d: the veteran / fresh comparison failed at step (\d+) \(([^)]*)\)" % (name, seed),
                      with_leak)
        assert m, with_leak
        k = int(m.group(1))
        lines = ast.literal_eval(re.search(r"steps so far: (\[.*\])", with_leak).group(1))
        assert len(lines) == k + 1 and lines[-1] == m.group(2) and lines == H.describe(steps[:k + 1])
        # ... and reproduces the failure by itself: the same step fails, and nothing before it does
        again = H.parse(FAKE, lines)
        with pytest.raises(H.HistoryError, match=r"failed at step %d " % k):
            _run_fake(again, leak)
        _run_fake(again[:-1], leak)
    # every structure's walks meet every leak (each has a smaller call after a larger one, both dtype
    # switches and a call that raises)
    assert set(caught) == set(H.WALK_SEEDS), (leak, caught)


@pytest.mark.parametrize("leak", LEAKS)
def test_the_leaks_pass_without_the_comparison(leak):
    """the leaks stay inside the check's tolerance on veteran and fresh alike: with compare=False
    run_history passes them, so the comparison is what the tests above rest on"""
    for name, seed, steps in _walks():
        _run_fake(steps, leak, compare=False)


def test_the_runner_sees_a_written_input_a_failed_check_and_an_irreproducible_operation():
    def run_writes(solver, i):
        out = _run(solver, i)
        i["x"][0, 0] += 1.0
        return out
    step = H.Step(H.Op("writes", "factor", _build, run_writes, _check), H.F64, 2, 3, 7)
    with pytest.raises(H.HistoryError, match=r"the veteran failed at step 0 .*read-only input x was written"):
        _run_fake([step], None)

    def run_off(solver, i):
        out = _run(solver, i)
        solver.calls = getattr(solver, "calls", 0) + 1
        if solver.calls == 3:
            out["out"] = out["out"] * 1.5
        return out
    steps = [H.Step(H.Op("off", "factor", _build, run_off, _check), H.F64, 1, 1, s) for s in range(4)]
    with pytest.raises(H.HistoryError, match=r"history t: the veteran failed at step 2 \(off:float64:b1:r1:s2\)"):
        _run_fake(steps, None, tag="t")

    noise = iter(range(100))

    def run_noisy(solver, i):
        out = _run(solver, i)
        out["out"] = out["out"] * (1.0 + 1e-15 * next(noise))
        return out
    step = H.Step(H.Op("noisy", "factor", _build, run_noisy, _check, bitwise=("out",)), H.F64, 1, 1, 1)
    with pytest.raises(H.HistoryError, match="two fresh solvers differ"):
        _run_fake([step], None)


def test_committed_seeds_cover_every_pair_of_families_and_every_change():
    walks = H.committed_walks()
    everything = [steps for ws in walks.values() for _, steps in ws]
    families = {op.family for op in H.VOCABULARY if not op.control}
    assert set(H.REQUIRED_FAMILIES) < families and "error" in families
    assert [m for m in H.missing_coverage(everything) if m[0] == "pair"] == []
    for name, ws in walks.items():
        assert [m for m in H.missing_coverage([steps for _, steps in ws]) if m[0] != "pair"] == [], name
        ops = {s.op.name for _, steps in ws for s in steps}
        assert "refused" in ops and any(n.startswith("setStream") for n in ops), name
    ops = {s.op.name for steps in everything for s in steps}
    assert {op.name for op in H.VOCABULARY} == ops, "an operation of the vocabulary never occurs"
