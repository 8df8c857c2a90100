"""Every choice of LinOp::precondition (fvens_amd/csrc/precond.cpp) but the multigrid, held to a host statement of
the same operator through the k-th GMRES iterate of one backward-Euler step, through steady_backward_euler_device
and FlowFVGroup.steady_backward_euler_device as they are.

With x0 = 0, right preconditioning, lin_rtol 0 and lin_maxit k the state change of the step is the unique minimiser
over the Krylov space of A M^-1: at k = 1 it is alpha M^-1 r, the operator itself applied to the step's right-hand
side, at larger k the operator applied to k further vectors. A converged answer, an iteration count or a recorded
history forgives a wrong M^-1 (a Gauss-Seidel sweep that runs the colours forward twice, a dropped colour, a Jacobi
sweep that lands in the wrong buffer, a missing halo exchange, an fp32 copy of the wrong array: the solve only takes
more steps); the k-th iterate does not. tests/gmres_host.py states M^-1 on the host from the structures the handles
report (colouring(), lines(), permutation() / the ranks' owned-cell lists):
  * block-Jacobi with 3 sweeps (the first count at which the z / aux alternation of buf(k) matters);
  * multicolour block Gauss-Seidel with 1, 2 and 3 sweeps (k_bgs_colour[_rows], ascending then descending);
  * the colour-order block ILU(0) with 1 and 2 sweeps (the correction z += M^-1 (v - A z));
  * the line solve with 1 and 2 sweeps, on a mesh whose lines twist, come in an odd number and include single cells;
  * prec_single for the first three: D^-1 / Dt^-1, lower and upper rounded to fp32 as LinOp::setup selects them, all
    arithmetic in fp64 (fp32 line factors are not restated: test_line_solve_inverts_line_blocks[single] covers them);
  * on a 3-rank in-process group: Jacobi 3, Gauss-Seidel 2 and 3 (other ranks' cells from the previous sweep), ILU 2
    and lines 2 (other ranks' cells only in the correction's A z), ghost rows of the states NaN on entry.
(restart, k) = (60,1), (60,9), (4,10) on one handle, (60,9) on the group; cgs_refine 0. Asserted per case, as in
test_gpu_gmres.py: steps, lin_iters, lin_unconverged, finite states, u - u1 per variable within 1000 floors of the
host forms, lin_worst against the host estimate, hist[0]; and that the host forms built here from the handles'
structures agree among themselves to the floor. tests/test_gmres_host.py shows on the CPU that one Arnoldi step,
another sweep count, Jacobi for Gauss-Seidel, every sweep ascending, reversed ILU colours, one domain's form for the
group's and a missing exchange each move the iterate by at least 1000 bars, and prec_single by at least 10.
Measured on an MI355X, the largest value over each family's cases (every test prints its own; the bar on du is 2e-11,
the host forms of the same structures differ among themselves by the third column):
                          du, of max |du| per var.   host forms   lin_worst against host estimate (bar 1e-9)
  Jacobi 3       fp64     4.0e-15                    6.7e-15      1.3e-15
                 fp32     2.8e-15                    3.1e-15      6.7e-16
  Gauss-Seidel   fp64     4.0e-15                    3.6e-15      6.9e-15
                 fp32     3.6e-15                    2.6e-15      6.3e-15
  ILU(0)         fp64     6.3e-15                    3.2e-15      1.1e-14
                 fp32     3.2e-15                    4.2e-15      6.4e-15
  lines          fp64     5.2e-15                    5.4e-15      1.9e-14
  3 ranks: Jacobi 3 4.0e-15, Gauss-Seidel 3.4e-15, ILU(0) 4.0e-15, lines 3.9e-15 (lin_worst 3.8e-14 at most)
hist[0] differs from the host's by at most 2.2e-16. The device sits at the host forms' own floor in every family; with
prec_single that includes the rounding, which moves the host iterate by 6e-10 or more (30 bars), so the device's
fp32 copies hold the values the host rounds. With one mistake each built into precond.cpp (not kept) the cases that
turn red are: the backward Gauss-Seidel sweep run ascending -- all 14 Gauss-Seidel cases with 2 or 3 sweeps; the
parity of buf(k) inverted -- all 7 Jacobi cases; S.exchange dropped from the Jacobi loop -- the group's Jacobi case.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import fvens_amd as fa
import _oracle as orc
import gmres_host as gh
from test_gpu_implicit import _gather, _partitioned, to_device

pytestmark = pytest.mark.gpu

BAR = gh.BAR_FACTOR * gh.FLOOR["jacobian"]


def _torch():
    import torch
    return torch


class _Steppers:
    """one handle and one 3-rank in-process group on a step system, with the host statements built from the
    structures these handles report"""

    def __init__(self, lines):
        self.s = s = gh.line_system() if lines else gh.step_system()
        self.one = fa.FlowFV(s.m, s.p, s.n)
        self.sps, self.dus, self.glob = _partitioned(s.m, s.p, s.n, s.u0, gh.PREC_RANKS)
        self.grp = fa.FlowFVGroup(self.sps)
        self.perm = self.one.permutation()
        self.host = {False: gh.PrecHost(s, [self._rank(self.one, self.perm)]),
                     True: gh.PrecHost(s, [self._rank(h, g) for h, g in zip(self.sps, self.glob)])}

    @staticmethod
    def _rank(h, glob):
        return SimpleNamespace(glob=np.asarray(glob), colour=h.colouring()[0], lines=h.lines())

    def close(self):
        self.grp.close()
        for h in self.sps:
            h.close()
        self.one.close()


@pytest.fixture(scope="module")
def steppers():
    held = {}

    def get(lines):
        if lines not in held:
            held[lines] = _Steppers(lines)
        return held[lines]
    yield get
    for h in held.values():
        h.close()


def _check_step(S, group, kind, sweeps, restart, k, single):
    torch = _torch()
    s = S.s
    h = S.host[group].case(kind, sweeps, restart, k, single)
    u1 = orc.relaxed_update(s.u0, h.minimiser.x.reshape(-1, 4), s.p.gamma, 1.0)
    res0 = np.sqrt(np.sum(s.r[:, 3] * s.r[:, 3] * s.m.area[:s.m.nelem]))
    cfg = fa.ImplicitConfig(cgs_refine=0, cflinit=gh.STEP_CFL, cflfin=gh.STEP_CFL, tol=0.0, maxiter=1, lin_rtol=0.0,
                            lin_maxit=k, restart=restart, prec_sweeps=sweeps, min_relax=1.0, prec_gs=kind == "gs",
                            prec_ilu=kind == "ilu", prec_lines=kind == "lines", prec_single=single)
    if group:
        for spk, d, g in zip(S.sps, S.dus, S.glob):
            d.fill_(float("nan"))
            d[:spk.nown] = torch.tensor(s.u0[g], device="cuda")
        torch.cuda.synchronize()
        st, hist = S.grp.steady_backward_euler_device([d.data_ptr() for d in S.dus], cfg)
        u = _gather(s.u0, S.sps, S.dus, S.glob)
    else:
        dU = to_device(s.u0, S.perm)
        torch.cuda.synchronize()
        st, hist = S.one.steady_backward_euler_device(dU.data_ptr(), cfg)
        u = np.empty_like(s.u0)
        u[S.perm] = dU.cpu().numpy()
    err = np.abs(u - u1).max(axis=0) / np.abs(u1 - s.u0).max(axis=0)
    worst = abs(st["lin_worst"] / (h.restated[0].rnorm / h.bnorm) - 1.0)
    print(f"PRECDIFF {kind} {sweeps} {'single' if single else 'double'} {'group' if group else 'one'} ({restart},{k}): du "
          f"{err.max():.2e} = {err.max() / BAR:.4f} bar; host forms {h.floor:.2e}; lin_worst against host estimate "
          f"{worst:.2e} (bar {gh.est_bar(h):.1e}); hist[0] {abs(hist[0] / res0 - 1.0):.2e}")
    assert h.floor <= gh.FLOOR["jacobian"]          # the host forms of these handles' structures, among themselves
    assert st["steps"] == 1 and st["lin_iters"] == k and st["lin_unconverged"] == 1
    assert np.all(np.isfinite(u)) and np.all(err <= BAR), err / BAR
    assert worst <= gh.est_bar(h)
    assert abs(hist[0] - res0) <= 1e-12 * res0


@pytest.mark.parametrize("single", [False, True], ids=["double", "single"])
@pytest.mark.parametrize("restart,k", gh.PREC_STEP_CASES)
@pytest.mark.parametrize("kind,sweeps", [c for c in gh.PREC_KINDS if c[0] != "lines"])
def test_step_iterate_matches_minimiser(steppers, kind, sweeps, restart, k, single):
    _check_step(steppers(False), False, kind, sweeps, restart, k, single)


@pytest.mark.parametrize("restart,k", gh.PREC_STEP_CASES)
@pytest.mark.parametrize("kind,sweeps", [c for c in gh.PREC_KINDS if c[0] == "lines"])
def test_line_step_iterate_matches_minimiser(steppers, kind, sweeps, restart, k):
    S = steppers(True)
    twisted, singles = gh.line_coverage(S.host[False].ranks[0].lines)
    assert twisted > 0 and twisted % 2 == 1 and twisted % 32 not in (0, 31) and singles > 0
    _check_step(S, False, kind, sweeps, restart, k, False)


@pytest.mark.parametrize("restart,k", gh.PREC_GROUP_STEP_CASES)
@pytest.mark.parametrize("kind,sweeps", gh.PREC_GROUP_KINDS)
def test_group_step_iterate_matches_minimiser(steppers, kind, sweeps, restart, k):
    S = steppers(kind == "lines")
    if kind == "lines":
        for r in S.host[True].ranks:
            twisted, singles = gh.line_coverage(r.lines)
            assert twisted > 0 and singles > 0
    _check_step(S, True, kind, sweeps, restart, k, False)
