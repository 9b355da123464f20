"""What one sampling time's reference window costs in ``BatchedRti._shift``, by its three sources, timed in
one session, alternating: the stored blocks of ``simulate_reference`` (``_reference_sim``: torch indexing),
the synthetic circle (``_reference_device``: torch elementwise) and the interpolated periodic trajectory
(``_reference_track``: one launch of the reference kernel, written into P in place).  Each is timed as the
branch of ``_shift`` that uses it: the window into P's ``ref`` and, for the two trajectory sources, its tail
into V.  Host clock around a device synchronise, 3 warm-up and 20 timed calls each.

    python tools/ref_window_timing.py --batch 256 --out out/ref_window_timing.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-k", type=int, default=20)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--interpolator", choices=["poly", "spline"], default="spline")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from awebox_amd import kite3 as k3
    from awebox_amd.reference import PeriodicTrajectory
    from awebox_amd.rti import BatchedRti

    c = k3.build_constants(k3.Kite3Config(n_k=a.n_k, d=a.d))
    r = BatchedRti(c, a.batch, device="cuda")
    r.start(x0_entries=(6, 7, 10))
    n_calls = a.warmup + a.calls
    r.simulate_reference(a.n_k + n_calls + 1)
    blocks, xs = r.sim_blocks, r.sim_xs
    r.track(PeriodicTrajectory.from_simulation(r), a.interpolator)
    r.sim_blocks, r.sim_xs = blocks, xs                   # both sources stay usable side by side
    lay = r.lay
    ref = slice(lay.p_ref, lay.p_ref + lay.n_v)
    tail = slice(lay.v_intervals + (lay.n_k - 1) * lay.interval_stride, lay.n_v)

    def from_sim(s):
        R = r._reference_sim(s)
        r.P[:, ref] = R
        r.V[:, tail] = R[:, tail]
        r.V[:, r.fict] = 0.0

    def from_circle(s):
        r.P[:, ref] = r._reference_device(r.t0_dev + s * c.cfg.ts)

    def from_kernel(s):
        r._reference_track(s)
        r.V[:, tail] = r.P[:, lay.p_ref + tail.start:lay.p_ref + tail.stop]
        r.V[:, r.fict] = 0.0

    paths = {"reference_sim": from_sim, "reference_device": from_circle, "reference_kernel": from_kernel}
    ms = {k: [] for k in paths}
    kernel_ms = []
    for s in range(1, n_calls + 1):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(s)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(r.ev.last_ref_ms())
    res = {"batch": a.batch, "n_k": a.n_k, "d": a.d, "interpolator": a.interpolator, "warmup": a.warmup,
           "calls": a.calls, "device": torch.cuda.get_device_name(0),
           "median_ms": {k: float(np.median(v[a.warmup:])) for k, v in ms.items()},
           "min_ms": {k: float(np.min(v[a.warmup:])) for k, v in ms.items()},
           "max_ms": {k: float(np.max(v[a.warmup:])) for k, v in ms.items()},
           "awempc_last_ref_ms_median": float(np.median(kernel_ms[a.warmup:]))}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
