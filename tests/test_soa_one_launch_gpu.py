"""The instance-minor path's node work in one launch (ap2_soa_eval_kernel: Radau tiles at the low
block indices, shooting tiles at the high ones, every workgroup with the wavefronts of the larger
kind) against the node + gather path on the same handle and inputs: g and J_g bitwise (both paths
take the node code from one header), f and grad f to the 1e-12 of tests/test_soa_fused_gpu.py.

Each shape is run with instance-minor outputs (ld = B + 5) and with per-instance outputs (the
library transposes afterwards); J_g and grad f are pre-filled with NaN, so an entry nobody wrote
shows, and theta0 differs by instance and by entry as in tests/test_soa_stage_gpu.py, so a row
staged by the wrong wavefront, from the wrong entry or from another instance's column changes g.

Shapes, the smallest that reach each seam of the merged launch:

* (n_k=4, d=4, B=65): two shooting groups, the second with one real interval and two clamped ones;
  a ragged second instance block; 8 Radau and 4 shooting tiles -> both sub-grids carry padding
  blocks wherever the tile count is no multiple of 8 (the shooting one here);
* (n_k=5, d=3, B=130): 15 Radau and 6 shooting tiles, both sub-grids padded;
* (n_k=3, d=5, B=1): two Radau nodes on one wavefront, a single instance, the fourth wavefront of
  the shooting tile runs no node;
* (n_k=7, d=2, B=64): an exact block; a Radau tile with two node wavefronts in a workgroup of three;
* (n_k=4, d=1, B=3): one Radau node wavefront in a workgroup of three;
* (n_k=40, d=4, B=130): the flagship's shape, once.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 65), (5, 3, 130), (3, 5, 1), (7, 2, 64), (4, 1, 3), (40, 4, 130)]
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
    """Evaluator, inputs (theta0 perturbed by instance and entry) and reference of a shape, once."""
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
    Ph = np.stack([pb.pack_p(lay, consts, v0, u_ref=5.0 + 0.05 * b) for b in range(B)])
    t0 = lay.n_v + pb.NW + pb.NCOST
    assert t0 + pb.NTHETA0 == lay.n_p
    c = (13 * np.arange(B)[:, None] + 7 * np.arange(pb.NTHETA0)[None, :]) % 41 - 20
    Ph[:, t0:t0 + pb.NTHETA0] *= 1.0 + 1e-3 * c
    ev = E.Ap2Evaluator(consts, batch=B)
    V = torch.tensor(Vh, device="cuda")
    P = torch.tensor(Ph, device="cuda")
    _CASES[key] = (ev, V, P, _reference(ev, V, P))
    return _CASES[key]


def _soa(ev, V, P, instance_minor):
    """One call on the instance-minor path; f and g, J_g and grad f pre-filled with NaN."""
    import torch
    B = ev.batch
    nan = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device="cuda")   # noqa: E731
    f, g = nan(B), nan(B, ev.n_g)
    if instance_minor and B > 1:
        ld = B + 5
        gr, jac = nan(ev.n_v, ld).t()[:B], nan(ev.nnz, ld).t()[:B]
    else:                                                 # B = 1: both layouts coincide
        gr, jac = nan(B, ev.n_v), nan(B, ev.nnz)
    ev.path = "soa"
    ev.eval_nlp_device(V, P, f, g, gr, jac)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (f, g, gr, jac)]


def _compare(got, ref, B, what):
    print(what, {lab: float(np.nanmax(np.abs(a - b))) for lab, a, b in zip(LABELS, got, ref)})
    for lab, a, b in zip(LABELS, got, ref):
        assert np.isfinite(a).all(), (what, lab, int(np.sum(~np.isfinite(a))))
        if lab in ("g", "jac"):
            assert np.array_equal(a, b), (what, lab, int(np.sum(a != b)), float(np.max(np.abs(a - b))))
        else:
            for i in range(B):
                _close(a[i], b[i], rtol=1e-12)


@pytest.mark.parametrize("n_k,d,B", SHAPES)
def test_one_launch_matches_the_node_gather_path(n_k, d, B):
    ev, V, P, ref = _case(n_k, d, B)
    _compare(_soa(ev, V, P, True), ref, B, "instance-minor outputs")
    _compare(_soa(ev, V, P, False), ref, B, "per-instance outputs")


def test_repeated_calls_on_one_handle_see_their_own_inputs():
    """Three calls with different V on one handle: each equals the node + gather path on its own V."""
    import torch
    ev, V, P, ref = _case(4, 4, 65)
    B = ev.batch
    scale = torch.linspace(-1.0, 1.0, ev.n_v, dtype=torch.float64, device="cuda")
    for call, eps in enumerate((0.0, 2e-3, -3e-3)):
        Vc = V * (1.0 + eps * scale)
        want = ref if eps == 0.0 else _reference(ev, Vc, P)
        if call:                                          # the inputs differ: so must the results
            assert not np.array_equal(want[1], ref[1])
        _compare(_soa(ev, Vc, P, True), want, B, "call %d" % call)


def test_timing_slots_of_an_instance_minor_call():
    """Inputs and outputs instance-minor: the node launch and the finalize kernel are timed, no
    transposition runs, and last_kernel_ms splits the same evaluation in two."""
    import torch
    ev, V, P, _ = _case(4, 4, 65)
    B = ev.batch
    ev.path = "soa"
    Vt, Pt = ev.alloc_inputs("cuda")
    Vt.copy_(V)
    Pt.copy_(P)
    f = torch.empty(B, dtype=torch.float64, device="cuda")
    g = torch.empty(B, ev.n_g, dtype=torch.float64, device="cuda")
    gr, jac = ev.alloc_grad("cuda", instance_minor=True), ev.alloc_jac("cuda", instance_minor=True)
    ev.eval_nlp_device(Vt, Pt, f, g, gr, jac)
    torch.cuda.synchronize()
    ms = ev.last_kernel_ms_soa()
    main, rest = ev.last_kernel_ms()
    print(ms, main, rest)
    assert ms[1] > 0 and ms[2] > 0
    assert ms[0] < 0.05 and ms[3] < 0.05 and ms[4] < 0.05
    assert abs((main + rest) - sum(ms)) <= 1e-3
