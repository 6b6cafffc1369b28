"""CPU: the batched selected-inversion entry points (bsp_selected_inverse_batched_f64 / _f32, the
testing cap bsp_test_set_selinv_batch_chunk and the new run counters) are declared and exported; an
empty batch, a NULL array, a NULL member and two equal members are refused with a message before any
device work; the calls fail cleanly with no GPU; the Python list form refuses mixed dtypes."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from baspacho_amd import _CRunCounters, _lib
from helpers import solver_random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"bsp_selected_inverse_batched_f64": "double", "bsp_selected_inverse_batched_f32": "float"}


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "baspacho_amd.h")).read()
    lib = _lib.load()
    for n, t in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(bsp_solver\* s, %s\* const\* dev_ptrs, int32_t batch\);" % (n, t),
                         hdr), n
        assert hasattr(lib, n), n
    thdr = open(os.path.join(ROOT, "include", "baspacho_amd_testing.h")).read()
    assert re.search(r"\bint\s+bsp_test_set_selinv_batch_chunk\s*\(bsp_solver\* s, int32_t max_matrices\);",
                     thdr)
    assert hasattr(lib, "bsp_test_set_selinv_batch_chunk")


def test_run_counters_appended_at_the_end():
    hdr = open(os.path.join(ROOT, "include", "baspacho_amd.h")).read()
    body = re.search(r"typedef struct bsp_run_counters \{(.*?)\} bsp_run_counters;", hdr, re.S).group(1)
    fields = re.findall(r"int64_t\s+(\w+);", body)
    assert fields[-2:] == ["selinv_launches", "selinv_chunks"], fields
    assert [n for n, _ in _CRunCounters._fields_] == fields
    sol, _, _ = solver_random(57)
    c = sol.runCounters()
    assert c["selinv_launches"] == 0 and c["selinv_chunks"] == 0


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


@pytest.mark.parametrize("name", sorted(NAMES))
def test_bad_batches_are_errors(name):
    lib = _lib.load()
    sol, _, _ = solver_random(57)
    f = getattr(lib, name)
    cases = [
        (_ptrs([0x1000]), 0, b"empty"),
        (_ptrs([0x1000]), -2, b"empty"),
        (None, 3, b"NULL"),
        (_ptrs([0x1000, 0, 0x3000]), 3, b"member 1"),
        (_ptrs([0x1000, 0x2000, 0x3000, 0x2000]), 4, b"same pointer"),
    ]
    for arr, batch, msg in cases:
        rc = f(sol._h, arr, ctypes.c_int32(batch))
        err = lib.bsp_last_error()
        assert rc != 0, (batch, msg)
        assert msg in err, err


def test_chunk_cap_rejects_negative():
    lib = _lib.load()
    sol, _, _ = solver_random(57)
    assert lib.bsp_test_set_selinv_batch_chunk(sol._h, ctypes.c_int32(-1)) != 0
    assert len(lib.bsp_last_error()) > 0
    sol._testSetSelInvBatchChunk(3)
    sol._testSetSelInvBatchChunk(0)


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
    for vals in ([0x1000], [0x1000, 0x2000, 0x3000]):
        arr = (ctypes.c_void_p * len(vals))(*vals)
        rc = getattr(lib, n)(sol._h, arr, ctypes.c_int32(len(vals)))
        msg = lib.bsp_last_error()
        assert rc != 0 and len(msg) > 0, (n, rc)
    # the argument checks come first, with or without a device
    rc = getattr(lib, n)(sol._h, (ctypes.c_void_p * 2)(0x1000, 0x1000), ctypes.c_int32(2))
    assert rc != 0 and b"same pointer" in lib.bsp_last_error(), n
    print(n, msg.decode())
"""


def test_no_gpu_is_an_error():
    """in a child process that sees no device: a non-zero return and a message, no crash"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = _NO_GPU_CHILD % (ROOT, os.path.join(ROOT, "tests"), sorted(NAMES))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stdout + r.stderr
    if r.returncode == 0:
        assert all(n in r.stdout for n in NAMES), r.stdout


def test_python_list_form_checks_its_members():
    """mixed dtypes, an empty list and a wrong size are refused before any pointer is taken (the
    tensors here live on the host: the checks must not reach them)"""
    import torch
    sol, _, _ = solver_random(57)
    n = sol.dataSize()
    with pytest.raises(TypeError, match="dtype"):
        sol.selectedInverse([torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float32)])
    with pytest.raises(TypeError, match="dtype"):
        sol.selectedInverse((torch.zeros(n, dtype=torch.float32), torch.zeros(n, dtype=torch.float64)))
    with pytest.raises(ValueError):
        sol.selectedInverse([])
    with pytest.raises(ValueError):
        sol.selectedInverse([torch.zeros(n, dtype=torch.float64), torch.zeros(n + 1, dtype=torch.float64)])


def test_batched_marginals_check_the_batch():
    """the list form refuses an empty batch (as selectedInverse(list) does), and checks the parameter
    indices of every member before reading its data"""
    sol, ps, _ = solver_random(57)
    with pytest.raises(ValueError, match="empty batch"):
        sol.marginals([], [0])
    with pytest.raises(ValueError, match="empty batch"):
        sol.marginals((), [0])
    data = [np.zeros(sol.dataSize()), np.zeros(sol.dataSize())]  # never read: the indices come first
    with pytest.raises(IndexError):
        sol.marginals(data, [len(ps)])
