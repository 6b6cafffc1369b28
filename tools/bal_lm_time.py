"""Time one Levenberg-Marquardt iteration of the BAL caller loop ("LM step on the
device"): bal.lm_optimize, whose cost, retraction and candidate cost run on the host and which rebuilds the
DevicePipeline every iteration, against bal.lm_optimize_device, which keeps the problem on the device and
reads three numbers back per iteration.

Problem: the small BAL stand-in of tools/normal_eq_time.py (120 cameras, 40 000 points, the co-visibility of
testing.gen_bal_synthetic at band 16) as a geometrically consistent scene (bal.synth_scene_for), 6-wide SE3
camera blocks; --problem bal871 takes the BAL-871 stand-in of bench.py instead (871 cameras, 527 480 points,
2.79 M observations), where the stage times are those of the headline workload and not of launch overheads.  Each loop runs once to warm up and once timed, --iters iterations each; an iteration's wall
time runs from the previous iteration's log line (taken after the loop's last host read, so the device is
idle) to its own, and the median over the iterations of the timed run is reported.  Beside them the device-
event times of the four new stages (residual-only kernel, loss with the scaling pass, the two-pass sum, the
retraction), warmed up, median of --reps, and for the loss its bytes over its time against the HBM peak.  The
Hessian fill is timed in its parts: the zeroing of H and g alone, the atomic fill alone and, where the library has
it, the ordered fill alone (bsp_bal_fill_ordered_*), the wall time per iteration of lm_optimize_device with
ordered_fill=True, and the one-time build of the plan on the host with its size.  One JSON line.

    python tools/bal_lm_time.py [--problem balsmall|bal871] [--iters 10] [--reps 7] [--loss huber:2.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baspacho_amd import testing as T  # noqa: E402
from assemble_time import HBM_TBPS, timed  # noqa: E402


# (cameras, points, gen_bal_synthetic's other arguments): the stand-in of tools/normal_eq_time.py, and the
# BAL-871 stand-in of bench.py for the sizes of the headline workload
PROBLEMS = {"balsmall": (120, 40000, {"band": 16}), "bal871": (871, 527480, {})}


def _iteration_times(run):
    """wall time of every iteration of run(log): log is called once per iteration, after its host read"""
    import torch
    stamps = []
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    _, hist = run(lambda _line: stamps.append(time.perf_counter()))
    torch.cuda.synchronize()
    return np.diff(stamps) * 1e3, hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loss", default="huber:2.0", help="loss of the stage timings, name:size")
    ap.add_argument("--problem", default="balsmall", choices=sorted(PROBLEMS))
    a = ap.parse_args()
    import torch
    import baspacho_amd as B
    from baspacho_amd import bal
    assert torch.cuda.is_available(), "bal_lm_time.py needs a GPU"
    nc, npt, kw = PROBLEMS[a.problem]
    _, _, cam, pt = T.gen_bal_synthetic(num_cams=nc, num_pts=npt, **kw)
    prob = bal.synth_scene_for(nc, npt, cam, pt)
    sizes, ss, ranges = bal.bal_structure(prob, cam_size=6)
    sol = B.create_solver(B.Settings(), sizes, ss, ranges)
    n = len(prob.obs_cam)
    rec = {"problem": a.problem, "cams": nc, "pts": npt, "obs": n, "order": sol.order(), "iters": a.iters}

    loops = {"lm_optimize": lambda log: bal.lm_optimize(prob, sol, max_iters=a.iters, log=log),
             "lm_optimize_device": lambda log: bal.lm_optimize_device(prob, sol, max_iters=a.iters, log=log)}
    for name, run in loops.items():
        _iteration_times(run)   # warm-up run
        ms, hist = _iteration_times(run)
        rec[name + "_iter_ms"] = round(float(np.median(ms)), 3)
        rec[name + "_iter_ms_min_max"] = [round(float(ms.min()), 3), round(float(ms.max()), 3)]
        rec[name + "_iterations"] = len(hist)
        rec[name + "_final_cost"] = hist[-1][1] if hist[-1][1] <= hist[-1][0] else hist[-1][0]
    rec["device_over_host_loop"] = round(rec["lm_optimize_device_iter_ms"] / rec["lm_optimize_iter_ms"], 4)
    # the ordered fill is timed where the loaded library has it (a parent build loaded through BSP_LIB_PATH has not)
    ordered = hasattr(bal._lib.load(), "bsp_bal_fill_ordered_f64")
    if ordered:
        run = lambda log: bal.lm_optimize_device(prob, sol, max_iters=a.iters, log=log, ordered_fill=True)
        _iteration_times(run)
        ms, hist = _iteration_times(run)
        rec["lm_optimize_device_ordered_iter_ms"] = round(float(np.median(ms)), 3)
        rec["lm_optimize_device_ordered_iter_ms_min_max"] = [round(float(ms.min()), 3), round(float(ms.max()), 3)]
        rec["lm_optimize_device_ordered_iterations"] = len(hist)
        rec["lm_optimize_device_ordered_final_cost"] = hist[-1][1] if hist[-1][1] <= hist[-1][0] else hist[-1][0]

    kind, size = a.loss.split(":")
    pipe = bal.DevicePipeline(prob, sol, param="se3", loss=(kind, float(size)))
    step = torch.randn(sol.order(), dtype=torch.float64, device="cuda") * 1e-3
    pipe.linearize()
    J0 = (pipe.res.clone(), pipe.Jc.clone(), pipe.Jp.clone())
    rec["linearize_ms"] = timed(pipe.linearize, a.warmup, a.reps)
    rec["residuals_ms"] = timed(lambda: pipe.residuals(out=pipe.res), a.warmup, a.reps)

    def restore():   # the loss scales in place: every timed pass starts from the unscaled linearisation
        pipe.res.copy_(J0[0]), pipe.Jc.copy_(J0[1]), pipe.Jp.copy_(J0[2])
    times = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for it in range(a.warmup + a.reps):
        restore()
        torch.cuda.synchronize()
        ev[0].record()
        pipe.apply_loss()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    rec["loss_ms"] = round(float(np.median(times)), 4)
    scaled = float((pipe.res != J0[0]).view(-1, 2).any(dim=1).double().mean().item())
    rec["loss_scaled_fraction"] = round(scaled, 3)
    # bytes of the loss launch: res read, rho written, the 20 words of every scaled observation read and written
    rec["loss_tbps"] = round((n * 8 * (2 + 1) + scaled * n * 2 * 20 * 8) / (rec["loss_ms"] * 1e9), 3)
    rec["hbm_peak_tbps"] = HBM_TBPS
    rec["sum_ms"] = timed(pipe.cost_linearized, a.warmup, a.reps)
    rec["apply_step_ms"] = timed(lambda: pipe.apply_step(step), a.warmup, a.reps)
    rec["cost_ms"] = timed(pipe.cost, a.warmup, a.reps)
    H = torch.zeros(sol.dataSize(), dtype=torch.float64, device="cuda")
    g = torch.zeros(sol.order(), dtype=torch.float64, device="cuda")

    def fill():
        H.zero_(), g.zero_()
        pipe.fill_hessian(H, g, 1e-5)
    restore()
    rec["zero_fill_hessian_ms"] = timed(fill, a.warmup, a.reps)
    rec["zero_ms"] = timed(lambda: (H.zero_(), g.zero_()), a.warmup, a.reps)
    # the fills alone: they add to what H and g hold, which only grows (1e30 is far away in these few passes)
    rec["fill_hessian_ms"] = timed(lambda: pipe.fill_hessian(H, g, 1e-5), a.warmup, a.reps)
    if ordered:
        t0 = time.perf_counter()
        plan = pipe.fill_plan()
        rec["fill_plan_build_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        rec["fill_plan"] = plan.info()

        def fill_ordered():
            H.zero_(), g.zero_()
            pipe.fill_hessian_ordered(H, g, 1e-5)
        rec["zero_fill_hessian_ordered_ms"] = timed(fill_ordered, a.warmup, a.reps)
        rec["fill_hessian_ordered_ms"] = timed(lambda: pipe.fill_hessian_ordered(H, g, 1e-5), a.warmup, a.reps)
        fill_ordered()
        Ho, go = H.clone(), g.clone()
        fill_ordered()
        rec["ordered_fill_repeats_bitwise"] = bool(torch.equal(H, Ho) and torch.equal(g, go))
        fill()
        rec["ordered_vs_atomic_max_rel"] = float(((H - Ho).abs().max() / Ho.abs().max()).item())
    fill()
    Hf = H.clone()

    def factor_solve():
        H.copy_(Hf)
        sol.factor(H)
        sol.solve(H, g, sol.order(), 1)
    rec["copy_factor_solve_ms"] = timed(factor_solve, a.warmup, a.reps)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
