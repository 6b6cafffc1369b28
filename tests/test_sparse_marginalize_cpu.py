"""CPU: the argument checks of SymmetricPattern(keep=...) and sparse.marginalize that need no device,
and the placement of the kept params behind a lump boundary."""
import numpy as np
import pytest
import torch

from baspacho_amd import sparse as S
from marginalize_cases import random_problem


def _pattern(prob, **kw):
    return S.SymmetricPattern(prob["rows"], prob["cols"], prob["n"], param_sizes=prob["param_sizes"], **kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_kept_params_are_the_trailing_spans(seed):
    prob = random_problem(seed)
    pat = _pattern(prob, keep=prob["keep"])
    sol, sk = pat.solver, pat.solver.skel()
    spans = np.sort(sol.paramToSpan()[prob["keep_params"]])
    assert np.array_equal(spans, np.arange(pat.keep_span, sol.numSpans()))
    assert int(sk["spanOffsetInLump"][pat.keep_span]) == 0
    bar = int(sk["spanStart"][pat.keep_span])
    m = len(prob["keep"])
    assert sol.order() - bar == m
    assert np.array_equal(np.sort(pat._keep_dest), np.arange(m))
    perm = sol.scalarPermutation()
    assert np.array_equal(pat._keep_dest[perm[prob["keep"]] - bar], np.arange(m))
    sol._testSelInvPlan(pat.keep_span)  # a cut that factorAdjointUpTo accepts


def test_keep_none_is_unchanged():
    prob = random_problem(4)
    a, b = _pattern(prob), _pattern(prob, keep=None)
    assert a.keep is None and a.keep_span is None
    assert np.array_equal(a.solver.scalarPermutation(), b.solver.scalarPermutation())
    assert np.array_equal(a.solver.skel()["lumpStart"], b.solver.skel()["lumpStart"])


def test_argument_checks():
    prob = random_problem(5)
    ps, keep = prob["param_sizes"], prob["keep"]
    wide = int(np.nonzero(ps > 1)[0][0])
    first = int(np.concatenate([[0], np.cumsum(ps)])[wide])
    with pytest.raises(ValueError, match="whole params"):
        _pattern(prob, keep=[first])
    with pytest.raises(ValueError, match="distinct"):
        _pattern(prob, keep=np.concatenate([keep, keep[:1]]))
    with pytest.raises(ValueError, match="distinct"):
        _pattern(prob, keep=[prob["n"]])
    with pytest.raises(ValueError, match="distinct"):
        _pattern(prob, keep=[])
    values = torch.zeros(len(prob["rows"]), dtype=torch.float64)
    with pytest.raises(ValueError, match="device memory"):
        S.marginalize(_pattern(prob, keep=keep), values)
    assert "marginalize" in S.__all__
