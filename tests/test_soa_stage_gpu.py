"""The staging prologue of the instance-minor node kernels (theta0 rows, the six shared rows, the
interval slices, the destination offsets) against the node + gather path, which stages theta0 per
instance with other code: g and J_g bitwise, f and grad f to the 1e-12 of tests/test_soa_fused_gpu.py.

theta0 differs by instance and by entry here: every instance's theta0 block of P is multiplied by
1 + 1e-3 c(b, i), c(b, i) = (13 b + 7 i) mod 41 - 20 (41 is prime to 13 and 7: any two entries less
than 41 apart, and any two instances less than 41 apart, get different integers in [-20, 20]).  A
theta0 row staged from another entry or another instance's column changes g; that the perturbation
itself changes g of every instance is asserted first.

Shapes, the smallest that reach each branch of the staging:

* (n_k=5, d=4, B=65): a ragged instance block (one lane), and a shooting group whose third interval
  is past n_k (5 intervals in groups of 3);
* (n_k=3, d=3, B=130): three Radau wavefronts;
* (n_k=2, d=5, B=64): the largest image, wavefront 0 runs two nodes;
* (n_k=4, d=4, B=1): a single lane.

Each shape goes through awe_eval_nlp_im (per-instance V and P, transposed by the library) and
through awe_eval_nlp_imv (instance-minor V and P with the handle's leading dimension, padding
columns b in [B, ld) filled with NaN where ld > B); outputs are pre-filled with NaN, and a second
call on the same handle must return the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(5, 4, 65), (3, 3, 130), (2, 5, 64), (4, 4, 1)]
LABELS = ("f", "g", "grad_f", "jac")
_CASES = {}


def _close(a, b, rtol):
    scale = np.max(np.abs(b))
    assert np.all(np.abs(a - b) <= rtol * np.abs(b) + 1e-11 * scale), float(np.max(np.abs(a - b)))


def _reference(ev, V, P):
    """The node + gather path, per-instance outputs."""
    import torch
    B = ev.batch
    ev.path = "generated"
    f = torch.empty(B, dtype=torch.float64, device="cuda")
    g = torch.empty(B, ev.n_g, dtype=torch.float64, device="cuda")
    gr = ev.alloc_grad("cuda", instance_minor=False)
    jac = ev.alloc_jac("cuda", instance_minor=False)
    ev.eval_nlp_device(V, P, f, g, gr, jac)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (f, g, gr, jac)]


def _case(n_k, d, B):
    """Evaluator, inputs (theta0 perturbed) and the reference outputs of a shape, computed once."""
    key = (n_k, d, B)
    if key in _CASES:
        return _CASES[key]
    import torch

    from awebox_amd import evaluator as E
    from awebox_amd import problem as pb
    from awebox_amd.initial_guess import batch_member, initial_guess
    consts = pb.build_constants(pb.Ap2Config(n_k=n_k, d=d))
    lay = pb.NlpLayout(n_k, d)
    v0 = initial_guess(consts, lay)
    Vh = np.stack([batch_member(v0, lay, b) for b in range(B)])
    Ph0 = np.stack([pb.pack_p(lay, consts, v0, u_ref=5.0 + 0.05 * b) for b in range(B)])
    t0 = lay.n_v + pb.NW + pb.NCOST
    assert t0 + pb.NTHETA0 == lay.n_p
    c = (13 * np.arange(B)[:, None] + 7 * np.arange(pb.NTHETA0)[None, :]) % 41 - 20
    Ph = Ph0.copy()
    Ph[:, t0:t0 + pb.NTHETA0] *= 1.0 + 1e-3 * c
    ev = E.Ap2Evaluator(consts, batch=B)
    V = torch.tensor(Vh, device="cuda")
    P = torch.tensor(Ph, device="cuda")
    ref = _reference(ev, V, P)
    g0 = _reference(ev, V, torch.tensor(Ph0, device="cuda"))[1]
    # the test sees the theta0 rows: the perturbation moves g of every instance
    assert np.all(np.any(ref[1] != g0, axis=1)), "the theta0 perturbation does not reach g"
    _CASES[key] = (ev, V, P, ref)
    return _CASES[key]


def _outputs(ev):
    """NaN-filled outputs, J_g and grad f instance-minor with ld = B + 5."""
    import torch
    B, ld = ev.batch, ev.batch + 5
    nan = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device="cuda")   # noqa: E731
    return nan(B), nan(B, ev.n_g), nan(ev.n_v, ld), nan(ev.nnz, ld), ld


def _numpy(ev, f, g, gr_s, jac_s):
    import torch
    torch.cuda.synchronize()
    B = ev.batch
    return [f.cpu().numpy(), g.cpu().numpy(), gr_s[:, :B].t().cpu().numpy(), jac_s[:, :B].t().cpu().numpy()]


def _run_im(ev, V, P):
    f, g, gr_s, jac_s, ld = _outputs(ev)
    ev.path = "soa"
    ev._call("eval_nlp_im", V.data_ptr(), P.data_ptr(), f.data_ptr(), g.data_ptr(), gr_s.data_ptr(),
             jac_s.data_ptr(), ld, ev._stream(None))
    return _numpy(ev, f, g, gr_s, jac_s)


def _run_imv(ev, V, P):
    import torch
    B, ldin = ev.batch, ev.instance_ld
    assert ldin >= B
    VT = torch.full((ev.n_v, ldin), np.nan, dtype=torch.float64, device="cuda")
    PT = torch.full((ev.n_p, ldin), np.nan, dtype=torch.float64, device="cuda")
    VT[:, :B] = V.t()
    PT[:, :B] = P.t()
    f, g, gr_s, jac_s, ld = _outputs(ev)
    ev.path = "soa"
    ev._call("eval_nlp_imv", VT.data_ptr(), PT.data_ptr(), ldin, f.data_ptr(), g.data_ptr(), gr_s.data_ptr(),
             jac_s.data_ptr(), ld, ev._stream(None))
    return _numpy(ev, f, g, gr_s, jac_s)


def _check(run, n_k, d, B):
    ev, V, P, ref = _case(n_k, d, B)
    got = run(ev, V, P)
    print({lab: float(np.nanmax(np.abs(a - b))) for lab, a, b in zip(LABELS, got, ref)})
    for lab, a, b in zip(LABELS, got, ref):
        assert np.isfinite(a).all(), lab
        if lab in ("g", "jac"):
            assert np.array_equal(a, b), (lab, int(np.sum(a != b)), float(np.max(np.abs(a - b))))
        else:
            for i in range(B):
                _close(a[i], b[i], rtol=1e-12)
    again = run(ev, V, P)
    for lab, a, b in zip(LABELS, again, got):
        assert np.array_equal(a, b), ("second call", lab)


@pytest.mark.parametrize("n_k,d,B", SHAPES)
def test_staged_image_through_eval_nlp_im(n_k, d, B):
    _check(_run_im, n_k, d, B)


@pytest.mark.parametrize("n_k,d,B", SHAPES)
def test_staged_image_through_eval_nlp_imv(n_k, d, B):
    _check(_run_imv, n_k, d, B)
