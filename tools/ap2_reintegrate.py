"""GPU tool: re-integrate a solved AP2 N = 40, d = 4 trajectory with rk4root over all 40 intervals in one
launch (integrators.reintegrate), and time that against the host-loop integrator on interval 0.

    python tools/ap2_reintegrate.py [--homotopy | --load FILE.npz] [--n-fe 30] [--warmup 3] [--reps 10]
                                    [--out profiles/ap2_rk4root/reintegrate_ab.json]

The trajectory: by default the stored 35.9 s orbit (tests/fixtures/ap2_n40_orbit_35s.npz) re-solved on the HIP
evaluator from its own primal-dual point (the recipe of tests/test_regression.py), which must converge;
``--homotopy`` solves the default homotopy from the initial guess instead; ``--load`` takes ``V`` from a file as
it is.  Printed: the worst interval of the three relative errors the reference's test_discretization.py
defines (x_end, z_end, the energy) and of the rootfinder residual, beside the reference's bound for rk4root
(2e-2).  Timed, alternating in one session after the warm-up, a host clock around a device synchronise: the
fused launch over all 40 intervals against ``IntervalIntegrator.rk4root`` on interval 0, at B = 1 each.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from awebox_amd import homotopy as hm  # noqa: E402
from awebox_amd import problem as pb  # noqa: E402
from awebox_amd.evaluator import Ap2Evaluator  # noqa: E402
from awebox_amd.initial_guess import initial_guess  # noqa: E402
from awebox_amd.integrators import IntervalIntegrator, reintegrate  # noqa: E402

RK4ROOT_BOUND = 2e-2          # test/reg/test_discretization.py:186-190


def trajectory(a, consts, lay, ev):
    """(V, how it was obtained) of a converged N = 40 trajectory."""
    if a.load:
        return np.load(a.load)["V"], {"source": a.load}
    from awebox_amd.ipm import IpmOptions, solve
    from awebox_amd.trajectory import hippo_options, optimize
    if a.homotopy:
        V, summary, _, _ = optimize(consts, ev, IpmOptions(max_iter=2000))
        if not all(r["status"] == "solve_succeeded" for r in summary):
            raise SystemExit(f"the homotopy did not converge: {summary}")
        return V, {"source": "homotopy", "iterations": [r["iterations"] for r in summary]}
    fx = np.load(os.path.join(ROOT, "tests", "fixtures", "ap2_n40_orbit_35s.npz"))
    v0 = initial_guess(consts, lay)
    st = hm.schedule(consts, lay, v0)[-1]
    lbg, ubg = lay.g_bounds()
    P = pb.pack_p(lay, consts, v0, step=st.cost_step)
    opts = dataclasses.replace(hippo_options("final", IpmOptions(max_iter=300)), mu_init=1e-9)
    res = solve(ev, P, fx["V"], st.lbx, st.ubx, lbg, ubg, lam0=fx["lam_g"], zl0=fx["zl"], zu0=fx["zu"], opts=opts)
    if res.status != "solve_succeeded":
        raise SystemExit(f"the warm-started solve did not converge: {res.status}")
    return res.x, {"source": "stored orbit re-solved", "status": res.status, "iterations": int(res.iterations),
                   "f": float(res.f)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--homotopy", action="store_true")
    ap.add_argument("--load", default=None)
    ap.add_argument("--n-fe", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap2_rk4root", "reintegrate_ab.json"))
    a = ap.parse_args()
    consts, lay = pb.build_constants(), pb.NlpLayout(40, 4)
    ev = Ap2Evaluator(consts, batch=1)
    V, how = trajectory(a, consts, lay, ev)
    out = hm.outputs(consts, lay, V)
    v0 = initial_guess(consts, lay)
    P = pb.pack_p(lay, consts, v0, step=hm.schedule(consts, lay, v0)[-1].cost_step)
    Vt, Pt = torch.tensor(V[None], device="cuda"), torch.tensor(P[None], device="cuda")

    r = reintegrate(ev, lay, consts, Vt, Pt, n_fe=a.n_fe)
    worst = {}
    for name in ("x", "z", "q", "residual"):
        k = int(r[name][0].argmax())
        worst[name] = {"interval": k, "value": float(r[name][0, k])}
        over = "" if name == "residual" else ("  (over the reference's 2e-2)" if worst[name]["value"] > RK4ROOT_BOUND
                                              else "  (within the reference's 2e-2)")
        print(f"worst {name}: interval {k}: {worst[name]['value']:.3e}{over}", flush=True)
    n_over = {name: int((r[name][0] > RK4ROOT_BOUND).sum()) for name in ("x", "z", "q")}

    integ = IntervalIntegrator(ev, lay, consts.scaling, k=0, device="cuda")
    h = Vt[:, int(lay.theta()[1])] * consts.scaling[pb.W_TH0 + 1] / lay.n_k
    p = hm.power_integrand(consts)
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        o = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, o

    fused = lambda: reintegrate(ev, lay, consts, Vt, Pt, n_fe=a.n_fe)          # noqa: E731
    host = lambda: integ.rk4root(Vt, Pt, p, h, n_steps=a.n_fe)                   # noqa: E731
    for _ in range(a.warmup):
        host(), fused()
    ms = {"host_loop_interval0": [], "fused_all_intervals": [], "fused_kernel": []}
    for _ in range(a.reps):
        t, ref = timed(host)
        ms["host_loop_interval0"].append(t)
        t, new = timed(fused)
        ms["fused_all_intervals"].append(t)
        ms["fused_kernel"].append(ev.last_integrate_ms())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    x1 = Vt[0, torch.as_tensor(lay.x(1), device="cuda")]
    rec = {"trajectory": {**how, **out}, "n_k": lay.n_k, "d": lay.d, "n_fe": a.n_fe, "batch": 1,
           "worst_interval": worst, "intervals_over_2e-2": n_over, "rk4root_bound": RK4ROOT_BOUND,
           "errors": {name: r[name][0].tolist() for name in ("x", "z", "q", "residual")},
           "interval0_host_loop": {"x": float((ref["x_end"][0] - x1).abs().max() / x1.abs().max()),
                                   "residual": float(ref["residual"].max()),
                                   "x_end_max_abs_diff_to_fused": float((ref["x_end"][0] - new["x_end"][0, 0]).abs().max())},
           "warmup": a.warmup, "reps": a.reps, "ms_median": med, "ms_min": {k: min(v) for k, v in ms.items()},
           "ms_max": {k: max(v) for k, v in ms.items()},
           "speedup_median_40_intervals_vs_1": med["host_loop_interval0"] / med["fused_all_intervals"], "ms": ms}
    print(json.dumps({k: rec[k] for k in ("trajectory", "worst_interval", "intervals_over_2e-2", "ms_median",
                                          "speedup_median_40_intervals_vs_1", "interval0_host_loop")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
