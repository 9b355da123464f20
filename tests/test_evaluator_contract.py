"""The contract the three evaluators share through nlp_binding.NlpEvaluator, on an MI355X, at the
smallest shapes each library supports and batch 3:

* the host path and the device path with contiguous outputs run the same kernel on the same handle,
  so f, g, grad f, J_g and H agree bitwise;
* instance-minor outputs (alloc_jac / alloc_grad(instance_minor=True)): bitwise the contiguous result
  for AP2 (at batch 3 both layouts run the colour kernel, then a layout-only transpose); for the
  dual-kite and MPC libraries that call runs the generated node code instead of the colour /
  dual-number kernel, and the two agree as tests/test_dual_gpu.py and tests/test_mpc.py ask of that
  pair: |a - b| <= 1e-9 |b| + 1e-11 max|b|.  The dual-kite generated code is instantiated for d = 4
  only: at d = 3 the library must say so (generated_available is False, the call is an error), and
  the pair is compared at n_k = 5, d = 4;
* lifecycle: close() twice is harmless, a closed evaluator raises instead of crashing, and a new
  evaluator of the same shape repeats the bits, three create / evaluate / close cycles in a row.
"""
import numpy as np
import pytest

from test_gpu_parity import _close  # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

B = 3


def _ap2(n_k, d):
    from awebox_amd import problem as pb
    from awebox_amd.evaluator import Ap2Evaluator
    from awebox_amd.initial_guess import batch_member, initial_guess
    consts = pb.build_constants(pb.Ap2Config(n_k=n_k, d=d))
    lay = pb.NlpLayout(n_k, d)
    v0 = initial_guess(consts, lay)
    V = np.stack([batch_member(v0, lay, b) for b in range(B)])
    P = np.stack([pb.pack_p(lay, consts, v0)] * B)
    return (lambda: Ap2Evaluator(consts, batch=B)), V, P


def _dual(n_k, d):
    from awebox_amd import dual as du
    from awebox_amd.dual_evaluator import DualEvaluator
    mc = du.build_constants(du.MultiConfig(n_k=n_k, d=d))
    lay = du.layout_for(mc)
    V0 = du.initial_guess(mc, lay)
    V = np.stack([du.batch_member(V0, lay, b) for b in range(B)])
    P = np.stack([du.pack_p(lay, mc, V0, step, u_ref=u) for step, u in
                  (("power1", 5.0), ("fictitious0", 6.5), ("final0", 8.0))])
    return (lambda: DualEvaluator(mc, batch=B)), V, P


def _mpc(n_k, d):
    from awebox_amd import kite3 as k3
    from awebox_amd.mpc import MpcEvaluator
    c = k3.build_constants(k3.Kite3Config(n_k=n_k, d=d))
    lay = k3.MpcLayout(n_k, d)
    inst = [k3.batch_instance(c, lay, i * 13, 64) for i in range(B)]
    V, P = np.stack([v for v, _ in inst]), np.stack([p for _, p in inst])
    return (lambda: MpcEvaluator(c, batch=B)), V, P


CASES = {"ap2": (_ap2, 3, 3), "dual": (_dual, 5, 3), "mpc": (_mpc, 3, 2), "dual_d4": (_dual, 5, 4)}
_cache = {}


def _case(name):
    """(make evaluator, V, P, sigma, lam_g, host results) of a case; the host results are computed
    once, on an evaluator of their own, and shared."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test on a machine without a visible GPU")
    if name not in _cache:
        from awebox_amd.build import build
        build()
        setup, n_k, d = CASES[name]
        make, V, P = setup(n_k, d)
        ev = make()
        rng = np.random.default_rng(11)
        sigma, lam = rng.uniform(0.5, 1.5, B), rng.standard_normal((B, ev.n_g))
        ref = ev.eval_nlp(V, P)
        ref["H"] = ev.eval_hess(V, P, sigma, lam)
        ev.close()
        _cache[name] = (make, V, P, sigma, lam, ref)
    return _cache[name]


def _device_eval(ev, V, P, instance_minor):
    import torch
    f64 = dict(dtype=torch.float64, device="cuda")
    Vt, Pt = torch.tensor(V, device="cuda"), torch.tensor(P, device="cuda")
    f, g = torch.full((B,), float("nan"), **f64), torch.full((B, ev.n_g), float("nan"), **f64)
    grad, jac = ev.alloc_grad("cuda", instance_minor=instance_minor), ev.alloc_jac("cuda", instance_minor=instance_minor)
    assert grad.is_contiguous() != instance_minor and jac.is_contiguous() != instance_minor
    grad.fill_(float("nan"))
    jac.fill_(float("nan"))
    ev.eval_nlp_device(Vt, Pt, f, g, grad, jac)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in (("f", f), ("g", g), ("grad_f", grad), ("jac", jac))}


@pytest.mark.parametrize("name", ["ap2", "dual", "mpc"])
def test_host_and_contiguous_device_paths_agree_bitwise(name):
    import torch
    make, V, P, sigma, lam, ref = _case(name)
    ev = make()
    out = _device_eval(ev, V, P, instance_minor=False)
    for k in ("f", "g", "grad_f", "jac"):
        assert np.isfinite(out[k]).all() and np.array_equal(out[k], ref[k]), k
    H = torch.full((B, ev.nnz_h), float("nan"), dtype=torch.float64, device="cuda")
    ev.eval_hess_device(*(torch.tensor(a, device="cuda") for a in (V, P, sigma, lam)), H)
    torch.cuda.synchronize()
    assert np.isfinite(ref["H"]).all() and np.array_equal(H.cpu().numpy(), ref["H"])
    ev.close()


@pytest.mark.parametrize("name", ["ap2", "dual", "mpc", "dual_d4"])
def test_instance_minor_outputs(name):
    from awebox_amd.evaluator import AwegpuError
    make, V, P, _, _, ref = _case(name)
    ev = make()
    if name == "dual":                               # d = 3: no generated dual-kite code
        assert not ev.generated_available
        with pytest.raises(AwegpuError, match="generated path unavailable"):
            _device_eval(ev, V, P, instance_minor=True)
    else:
        out = _device_eval(ev, V, P, instance_minor=True)
        for k in ("f", "g", "grad_f", "jac"):
            assert np.isfinite(out[k]).all(), k
            if name == "ap2":
                assert np.array_equal(out[k], ref[k]), k
            else:
                assert ev.generated_available
                for b in range(B):
                    _close(out[k][b], ref[k][b], f"{k}[{b}] vs the contiguous path")
    ev.close()


@pytest.mark.parametrize("name", ["ap2", "dual", "mpc"])
def test_lifecycle(name):
    from awebox_amd.evaluator import AwegpuError
    make, V, P, sigma, lam, ref = _case(name)
    for _ in range(3):
        ev = make()
        out = ev.eval_nlp(V, P)
        out["H"] = ev.eval_hess(V, P, sigma, lam)
        for k in ref:
            assert np.array_equal(out[k], ref[k]), k
        ev.close()
        ev.close()
        with pytest.raises(AwegpuError):
            ev.eval_nlp(V, P)
        with pytest.raises(AwegpuError):
            ev.last_kernel_ms()
