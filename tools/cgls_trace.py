"""Per-kernel device time of an iteration of DESIGN.md section 28 on the GRID 82x82 pose graph of
tools/normal_eq_time.py, for sparse.lstsq_cg without a preconditioner and for the composed route of
tools/cgls_time.py (3 right-hand sides, damping as there, tol = 0, 200 iterations queued without a read, three
solves of which the last is counted).

    rocprofv3 --kernel-trace -d DIR -o NAME -- python tools/cgls_trace.py run cgls|composed
    python tools/cgls_trace.py summarise DIR/.../NAME_results.db [...]     # appends to profiles/cgls_trace.txt

The summary gives, per route, the launches and the device-busy and first-start-to-last-end time of the last solve
per iteration, and the mean duration of every kernel launched at least once per iteration."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 200


def run(which):
    import torch
    from normal_eq_time import problems
    from cgls_time import composed_cg, DAMPING
    from baspacho_amd import cgls as CGLS
    from baspacho_amd import sparse as S
    sizes, (rows, cols, vals, m, n) = problems()["grid82"]()
    v = torch.from_numpy(vals).cuda()
    r3 = torch.from_numpy(np.random.default_rng(37).uniform(-1, 1, (m, 3))).cuda()
    if which == "cgls":
        op = S.JacobianOperator(rows, cols, m, n, param_sizes=sizes)
        for _ in range(3):
            S.lstsq_cg(op, v, r3, damping=DAMPING, precond=None, tol=0.0, max_steps=STEPS, check_every=None)
    else:
        jpat = S.JacobianPattern(rows, cols, m, n, param_sizes=sizes)
        csq = CGLS.column_norms(jpat.operator.product, v)
        d = CGLS.damping_vector(jpat.operator.product, csq, DAMPING[0], DAMPING[1], v)
        for _ in range(3):
            composed_cg(jpat, v, r3, d, None, 0.0, STEPS, check_every=None)
    torch.cuda.synchronize()


def summarise(paths):
    import sqlite3
    out = []
    for path in paths:
        rows = list(sqlite3.connect(path).cursor().execute("select name, start, end from kernels order by start"))
        rows = rows[len(rows) * 2 // 3:]  # the last of the three solves
        agg = {}
        for name, s, e in rows:
            name = re.sub(r"^void ", "", re.sub(r"\(.*", "", name)).replace("BaSpaCho::hipk::", "")
            a = agg.setdefault(name, [0, 0.0])
            a[0] += 1
            a[1] += (e - s) / 1e3
        busy, span = sum(a[1] for a in agg.values()), (rows[-1][2] - rows[0][1]) / 1e3
        out.append("%s: %d launches; per iteration (%d): %.2f us busy, %.2f us from first start to last end"
                   % (os.path.basename(path), len(rows), STEPS, busy / STEPS, span / STEPS))
        for name, (c, t) in sorted(agg.items(), key=lambda x: -x[1][1]):
            if c >= STEPS * 3 // 4:
                out.append("    %-72s %5d x %6.2f us" % (name[:72], c, t / c))
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "cgls_trace.txt"), "a") as f:
        f.write(text)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    run(sys.argv[2]) if sys.argv[1] == "run" else summarise(sys.argv[2:])
