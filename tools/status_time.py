"""Time the factor status and the damping of the diagonal beside logDet, which
walks the same diagonal elements: device events, warmed up, median of --reps, fp64 and fp32, on a factor
of BAL-871 (synthetic, point range [0, 527480]) and of GRID 82x82 (problems as tools/autograd_time.py).
All three read one element per scalar at a stride of the lump width + 1, so the useful bytes are
order x sizeof(T) and the time is launch and latency, not bandwidth.  damp_entry_ms is the C entry with a
prebuilt alpha / beta pair (the kernel and its launch), damp_diagonal_py_ms the Python method, which also
packs its arguments on the device; status_read_ms adds the 32-byte read.  One JSON line per problem and type.

    python tools/status_time.py [--reps 5] [--warmup 2] [--only bal871,grid82]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baspacho_amd import testing as T  # noqa: E402
from autograd_time import problems, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="bal871,grid82")
    a = ap.parse_args()
    import torch
    for name in a.only.split(","):
        sol = problems()[name]()
        h = T.random_data(sol.dataSize(), -1.0, 1.0, 37)
        sol.damp(h, 0.0, sol.order() * 1.2)
        for dt in (torch.float64, torch.float32):
            dev = torch.from_numpy(h).to("cuda").to(dt)
            sol.factor(dev)
            rec = {"problem": name, "dtype": str(dt).split(".")[-1], "order": sol.order(), "lumps": sol.numLumps(),
                   "data_size": sol.dataSize()}
            rec["ok"] = sol.readFactorStatus(sol.factorStatus(dev))["ok"]
            rec["log_det_ms"] = timed(lambda: sol.logDet(dev), a.warmup, a.reps)
            rec["factor_status_ms"] = timed(lambda: sol.factorStatus(dev), a.warmup, a.reps)
            # the C entry with a prebuilt pair (alpha = beta = 0: the factor stays what it is): the kernel alone;
            # then Solver.dampDiagonal, which also packs its two arguments with a few small torch kernels
            ab = torch.zeros(2, dtype=dt, device="cuda")
            entry = getattr(sol._lib, "bsp_damp_" + ("f64" if dt == torch.float64 else "f32"))
            args = (sol._h, ctypes.c_void_p(dev.data_ptr()), ctypes.c_int64(0), ctypes.c_int64(sol.numSpans()),
                    ctypes.c_void_p(ab.data_ptr()))
            assert entry(*args) == 0, sol._lib.bsp_last_error()
            rec["damp_entry_ms"] = timed(lambda: entry(*args), a.warmup, a.reps)
            rec["damp_diagonal_py_ms"] = timed(lambda: sol.dampDiagonal(dev, ab[0], ab[1]), a.warmup, a.reps)
            rec["status_read_ms"] = timed(lambda: sol.readFactorStatus(sol.factorStatus(dev)), a.warmup, a.reps)
            print(json.dumps(rec), flush=True)
            del dev
        del sol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
