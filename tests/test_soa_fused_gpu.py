"""The instance-minor path's Radau workgroup finishes its interval itself (objective, gradient,
continuity rows, partials from the staged slice, the nodes' objective terms handed over in LDS).
Forced onto the smallest shapes where that epilogue can go wrong:

* (n_k=4, d=4, B=65): one full instance block plus one lane, a ragged shooting group (4 intervals
  in groups of 3), first and last interval (the continuity row of the last one reads x[n_k]);
* (n_k=3, d=3, B=130): three wavefronts for the four virtual waves of the interval pass;
* (n_k=2, d=5, B=64): wavefront 0 runs two nodes, and the largest LDS image;
* (n_k=4, d=4, B=1): a single lane.

Against the node + gather path with the rules of tests/test_gen_path_gpu.py: g and J_g bitwise,
f and grad f to 1e-12 (the objective's sums run per lane instead of across a wavefront).  Outputs
are pre-filled with NaN and must come back finite; the padding columns b in [B, ld) of the
instance-minor J_g and gradient storage hold a sentinel that must survive; a second call on the
same inputs must return the same bits (a race on reused LDS rows would show here)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
SHAPES = [(4, 4, 65), (3, 3, 130), (2, 5, 64), (4, 4, 1)]


def _close(a, b, rtol):
    scale = np.max(np.abs(b))
    assert np.all(np.abs(a - b) <= rtol * np.abs(b) + 1e-11 * scale), float(np.max(np.abs(a - b)))


def _case(n_k, d, B):
    import torch

    from awebox_amd import evaluator as E
    from awebox_amd import problem as pb
    from awebox_amd.initial_guess import batch_member, initial_guess
    consts = pb.build_constants(pb.Ap2Config(n_k=n_k, d=d))
    lay = pb.NlpLayout(n_k, d)
    v0 = initial_guess(consts, lay)
    V = torch.tensor(np.stack([batch_member(v0, lay, b) for b in range(B)]), device="cuda")
    P = torch.tensor(np.stack([pb.pack_p(lay, consts, v0, u_ref=5.0 + 0.05 * b) for b in range(B)]), device="cuda")
    return E.Ap2Evaluator(consts, batch=B), V, P


def _reference(ev, V, P):
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


def _soa(ev, V, P):
    """One call on the instance-minor path into NaN-filled outputs; J_g and grad f instance-minor
    with ld = B + 5 and the sentinel in the padding columns (B = 1: both layouts coincide, no
    padding).  Returns the outputs and the two padding blocks (None at B = 1)."""
    import torch
    B = ev.batch
    ev.path = "soa"
    f = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    g = torch.full((B, ev.n_g), np.nan, dtype=torch.float64, device="cuda")
    if B == 1:
        gr_s = torch.full((1, ev.n_v), np.nan, dtype=torch.float64, device="cuda")
        jac_s = torch.full((1, ev.nnz), np.nan, dtype=torch.float64, device="cuda")
        gr, jac = gr_s, jac_s
    else:
        ld = B + 5
        gr_s = torch.full((ev.n_v, ld), SENTINEL, dtype=torch.float64, device="cuda")
        jac_s = torch.full((ev.nnz, ld), SENTINEL, dtype=torch.float64, device="cuda")
        gr_s[:, :B] = np.nan
        jac_s[:, :B] = np.nan
        gr, jac = gr_s.t()[:B], jac_s.t()[:B]
    ev.eval_nlp_device(V, P, f, g, gr, jac)
    torch.cuda.synchronize()
    pad = None if B == 1 else (gr_s[:, B:].cpu().numpy(), jac_s[:, B:].cpu().numpy())
    return [x.cpu().numpy() for x in (f, g, gr, jac)], pad


@pytest.mark.parametrize("n_k,d,B", SHAPES)
def test_fused_interval_pass_matches_the_node_gather_path(n_k, d, B):
    ev, V, P = _case(n_k, d, B)
    ref = _reference(ev, V, P)
    got, pad = _soa(ev, V, P)
    labels = ("f", "g", "grad_f", "jac")
    print({lab: float(np.nanmax(np.abs(a - b))) for lab, a, b in zip(labels, got, ref)})
    for lab, a, b in zip(labels, got, ref):
        assert np.isfinite(a).all(), lab
        if lab in ("g", "jac"):
            assert np.array_equal(a, b), (lab, float(np.max(np.abs(a - b))))
        else:
            for i in range(B):
                _close(a[i], b[i], rtol=1e-12)
    if pad is not None:
        for lab, x in zip(("grad_f", "jac"), pad):
            assert x.size and np.all(x == SENTINEL), lab
    again, pad2 = _soa(ev, V, P)
    for lab, a, b in zip(labels, again, got):
        assert np.array_equal(a, b), ("second call", lab)
    if pad2 is not None:
        for lab, x in zip(("grad_f", "jac"), pad2):
            assert np.all(x == SENTINEL), lab
