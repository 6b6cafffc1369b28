"""CPU: the selected-inversion entry points (bsp_selected_inverse_f64 / _f32) are declared and exported,
fail with a message instead of crashing when there is nothing to run on, and marginals() checks its
parameter indices."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from baspacho_amd import _lib
from helpers import solver_random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bsp_selected_inverse_f64", "bsp_selected_inverse_f32"]


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "baspacho_amd.h")).read()
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(bsp_solver\* s, (double|float)\* dev_data\);" % n, hdr), n
        assert hasattr(lib, n), n


def test_null_data_is_an_error():
    lib = _lib.load()
    sol, _, _ = solver_random(57)
    for n in NAMES:
        assert getattr(lib, n)(sol._h, None) != 0
        assert b"NULL" in lib.bsp_last_error()


_NO_GPU_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
if torch.cuda.is_available():
    sys.exit(3)  # the device could not be hidden: nothing to show here
from baspacho_amd import _lib
from helpers import solver_random
lib = _lib.load()
sol, _, _ = solver_random(57)
for n in %r:
    rc = getattr(lib, n)(sol._h, ctypes.c_void_p(0x1000))
    msg = lib.bsp_last_error()
    assert rc != 0 and len(msg) > 0, (n, rc)
    print(n, msg.decode())
"""


def test_no_gpu_is_an_error():
    """in a child process that sees no device: a non-zero return and a message, no crash"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = _NO_GPU_CHILD % (ROOT, os.path.join(ROOT, "tests"), NAMES)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stdout + r.stderr
    if r.returncode == 0:
        assert all(n in r.stdout for n in NAMES), r.stdout


def test_marginals_rejects_out_of_range_parameters():
    sol, ps, _ = solver_random(57)
    data = np.zeros(sol.dataSize())  # never read: the indices are checked first
    for bad in ([len(ps)], [-1], [0, len(ps) + 3]):
        with pytest.raises(IndexError):
            sol.marginals(data, bad)
