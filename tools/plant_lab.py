"""GPU lab: the rk4root plant against the collocation plant, per loop, over closed-loop steps.

    python tools/plant_lab.py [--batch 256] [--steps 3] [--n-fe 20] [--all-x0]

A/B mode: the host-loop plant (_rk4root) and the fused kernel (_rk4root_fused) timed alternating in one
session from the same closed-loop state -- a host clock around a device synchronise, after a warm-up --
with the evaluator's launch time and the kernel's own HIP-event time beside them:

    python tools/plant_lab.py --ab [--batch 256] [--n-fe 20] [--reps 20] [--out out/plant_ab.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from awebox_amd import kite3 as k3  # noqa: E402
from awebox_amd.rti import BatchedRti  # noqa: E402


def ab(a, r):
    """Times _rk4root and _rk4root_fused alternating; every repetition starts from the same state (neither
    plant changes the loop), so the two integrate the same sampling time."""
    sync = torch.cuda.synchronize
    r.iterate()

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    def evaluation():
        r.ev.eval_nlp_device(r.V, r.P, r.f, r.g, r.grad, r.jac)

    for _ in range(3):                                   # warm-up
        r._rk4root(), r._rk4root_fused(), evaluation()
    ms = {"rk4root": [], "rk4root_fused": [], "kernel": [], "evaluation": []}
    for _ in range(a.reps):
        t, (x_o, res_o) = timed(r._rk4root)
        ms["rk4root"].append(t)
        t, (x_f, res_f) = timed(r._rk4root_fused)
        ms["rk4root_fused"].append(t)
        ms["kernel"].append(r.ev.last_plant_ms())
        ms["evaluation"].append(timed(evaluation)[0])
    med = {k: float(torch.tensor(v).median()) for k, v in ms.items()}
    # the host-loop plant launches the evaluator at least twice per rootfinder, 4 n_fe rootfinders
    n_eval = 2 * 4 * a.n_fe
    res = {"batch": a.batch, "n_fe": a.n_fe, "reps": a.reps, "ms_median": med,
           "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
           "speedup_median": med["rk4root"] / med["rk4root_fused"],
           "evaluator_launches_alone_ms": n_eval * med["evaluation"], "evaluations_counted": n_eval,
           "x1_max_abs_diff": float((x_o - x_f).abs().max()),
           "residual_max": {"rk4root": float(res_o.max()), "rk4root_fused": float(res_f.max())}}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({**res, "ms": ms}, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--n-fe", type=int, default=20)
    ap.add_argument("--all-x0", action="store_true", help="x0 noise on every state (SURVEY spec)")
    ap.add_argument("--circle", action="store_true", help="track the synthetic circle")
    ap.add_argument("--ab", action="store_true", help="time _rk4root against _rk4root_fused, alternating")
    ap.add_argument("--reps", type=int, default=20, help="--ab: sampling times timed per plant")
    ap.add_argument("--out", default=None, help="--ab: JSON file for the result")
    a = ap.parse_args()
    c = k3.build_constants()
    r = BatchedRti(c, a.batch, device="cuda", n_fe=a.n_fe)
    r.start(x0_entries=None if a.all_x0 else (6, 7, 10))
    if not a.circle:
        r.simulate_reference(a.steps + c.cfg.n_k + 1)
    if a.ab:
        return ab(a, r)
    for s in range(a.steps):
        r.iterate()
        x0 = r.P[:, :k3.NX].clone()
        x_c, res_c = r._plant()
        x_r, res_r = r._rk4root()
        step = (x_c - x0).abs().amax(dim=1)
        gap = (x_c - x_r).abs().amax(dim=1)
        ratio = gap / step
        q = torch.quantile(ratio, torch.tensor([0.5, 0.9, 0.99, 1.0], dtype=torch.float64, device="cuda"))
        w = int(ratio.argmax())
        print(f"step {s}: gap/step quantiles (50/90/99/max) {q.cpu().numpy()} worst loop {w}: gap {float(gap[w]):.3e} "
              f"step {float(step[w]):.3e} res_c {float(res_c[w]):.1e} res_r {float(res_r[w]):.1e} "
              f"worst per-state {(x_c[w] - x_r[w]).abs().cpu().numpy()}", flush=True)
        r._shift(x_c)
        r.step_count += 1


if __name__ == "__main__":
    main()
