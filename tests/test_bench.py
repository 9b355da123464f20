"""bench.py's command line: a plain run reports the headline figure alone, `--dump-outputs` writes
what the timed path computed, and the sampling of a dump is fixed.

The GPU test starts the benchmark because the benchmark's own command line is what it is about
(130 instances: the instance-minor path, the default from 128 instances, at a size that is no
multiple of the wavefront)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "paths", "fp64", "dual", "mpc", "sweep", "dual_sweep", "hessian", "latency_batch1",
             "cpu_baseline", "casadi_probe"}


def _load(path):
    return {n[:-4]: np.load(os.path.join(path, n)) for n in sorted(os.listdir(path))}


def test_dump_outputs_sampling_is_fixed_and_within_budget(tmp_path):
    import torch

    import bench
    B = 300
    gen = torch.Generator().manual_seed(3)
    outs = {"f": torch.randn(B, dtype=torch.float64, generator=gen),
            "g": torch.randn(B, 6103, dtype=torch.float64, generator=gen),
            # instance-minor storage, [B, n] view, as the benchmark's J_g and gradient
            "grad_f": torch.randn(6154, B, dtype=torch.float64, generator=gen).t(),
            "jac_g": torch.randn(30000, B, dtype=torch.float64, generator=gen).t()}
    bench.dump_outputs(str(tmp_path / "a"), outs, 0)
    bench.dump_outputs(str(tmp_path / "b"), outs, 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["f", "g_cols", "g_rows", "grad_f_cols", "grad_f_rows", "jac_g_cols", "jac_g_rows"]
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a"))
    assert total <= 64e6
    for name, x in a.items():
        assert x.dtype == np.float64 and np.array_equal(x, b[name]), name
    assert np.array_equal(a["f"], outs["f"].numpy())
    for name in ("g", "grad_f", "jac_g"):
        full = outs[name].numpy()
        rows, cols = a[name + "_rows"], a[name + "_cols"]
        assert rows.shape[1] == full.shape[1] and cols.shape == (B, 256)
        # each sample is a sorted selection of whole instances / whole entries of the output
        first = np.flatnonzero((full == rows[0]).all(axis=1))
        assert first.size == 1 and np.array_equal(full[first[0]], rows[0])
        col0 = np.flatnonzero((full == cols[:, :1]).all(axis=0))
        assert col0.size == 1


def test_dump_outputs_writes_small_outputs_whole(tmp_path):
    import torch

    import bench
    outs = {"f": torch.arange(4, dtype=torch.float64), "g": torch.arange(40, dtype=torch.float64).reshape(4, 10)}
    bench.dump_outputs(str(tmp_path), outs, 0)
    got = _load(tmp_path)
    assert sorted(got) == ["f", "g"]
    assert np.array_equal(got["g"], outs["g"].numpy()) and got["g"].dtype == np.float64


@pytest.mark.gpu
def test_plain_run_reports_the_headline_alone_and_dumps_the_last_step(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test on a machine without a visible GPU")
    from awebox_amd import problem as pb
    from awebox_amd.build import build
    from awebox_amd.evaluator import Ap2Evaluator
    from awebox_amd.initial_guess import batch_member, initial_guess
    build()
    B, steps = 130, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, cwd=ROOT,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line), sorted(line)
    assert line["steps"] == steps and line["unit"] == "evals/s" and line["dtype"] == "f64" and line["higher_is_better"]
    # value and ms_per_step are the same measurement
    assert line["value"] == pytest.approx(B * 1e3 / line["ms_per_step"], rel=1e-9)

    got = _load(tmp_path)
    consts = pb.build_constants()
    lay = pb.NlpLayout(consts.cfg.n_k, consts.cfg.d)
    assert got["f"].shape == (B,)
    for name, n in (("g", lay.n_g), ("grad_f", lay.n_v)):
        assert got[name + "_rows"].shape[1] == n and got[name + "_cols"].shape == (B, 256)
    assert all(x.dtype == np.float64 and np.isfinite(x).all() for x in got.values())
    # the benchmark's inputs are the documented batch members: f of the same members through the
    # host entry point (fp64 sums of the same terms in another order: 1e-12 of the largest |f|)
    v0 = initial_guess(consts, lay)
    V = np.stack([batch_member(v0, lay, b) for b in range(B)])
    P = np.stack([pb.pack_p(lay, consts, v0)] * B)
    f = np.asarray(Ap2Evaluator(consts, batch=B).eval_nlp(V, P)["f"])
    assert np.abs(got["f"] - f).max() <= 1e-12 * np.abs(f).max()
