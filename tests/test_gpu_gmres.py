"""Device GMRES (fvens_amd/csrc/implicit.cpp gmres(), the vector kernels of krylov.hip under it) iterate by
iterate against the host restatements of tests/gmres_host.py, through gmres_blocks_device,
steady_backward_euler_device and FlowFVGroup.steady_backward_euler_device as they are.

With x0 = 0 and right preconditioning the iterate after k Arnoldi steps in cycles of m is unique, so the device's
x after exactly k steps (rtol 0: iters == maxit) is compared with the host's least-squares minimiser, which
shares no Hessenberg matrix, rotation or Gram-Schmidt variant with it. A converged answer forgives a wrong
Hessenberg entry, a slipped rotation, a product dropped at a group boundary of the multi-dot or a stale restart
residual (the solve only takes more steps); the k-th iterate and the reported residual norm do not.
  a. stand-alone solver on random blocks (naca_small, 2,304 cells): k across the multi-dot's groups of 8,
     restart 1, 2, 8, 9, 16, 17 with cycles cut by maxit, 1 and 2 Jacobi sweeps; x, the reported residual norm
     against the host estimate and, where |r_k| >= 1e-4 |b|, against numpy's |b - A x_device|;
  b. stopping by rtol (same count and x as the host), b = 0, maxit = 0, an exact preconditioner (lo = up = 0:
     the first projection removes all of w; one step, nothing non-finite);
  c. the steppers' paths: one backward-Euler step with lin_rtol 0 and lin_maxit k, cgs_refine 0, 1, 2 on one
     handle and on a 3-rank group: u - u0 against the minimiser's du_k per variable, lin_iters,
     lin_unconverged, lin_worst against the host estimate, hist[0];
  d. the second trip of the grid-stride loops (294,912 cells: 2 ncell > 2048 x 256 double2 lanes in
     k_mdot_partial / k_maxpy_norm, ncell > 131,072 in k_energy_partial).
Bars come from the host alone (gmres_host.py): iterate bar = 1000 x the family's floor (the largest difference
between host forms), estimate bar = 1000 x the host's gap between estimate and true residual (1e-9 where the
estimate is checked). tests/test_gmres_host.py shows that one Arnoldi step moves x by >= 1000 bars.
Measured on an MI355X, the largest difference over each family's cases (every test prints its own):
  fast      x 7.2e-15 of max |x|            (bar 3.2e-11)   residual norm: host estimate 6.0e-11 (bar of that case
                                                             1.8e-7), |b - A x| 2.2e-14 where checked (bar 1e-9)
  slow      x 2.8e-14 of max |x|            (bar 3.5e-10)   host estimate 1.1e-14, |b - A x| 1.1e-13 (bar 1e-9)
  Jacobian  du 3.3e-15 of max |du| per var. (bar 2e-11)     lin_worst 1.0e-15 (bar 1e-9), hist[0] equal
  large     x 2.7e-14 of max |x|            (bar 1.9e-10)   host estimate 4.4e-16, |b - A x| 6.7e-16, hist[0] equal
The device sits at the host forms' own measured floor (fast 8.0e-15, slow 8.6e-14, Jacobian 4.8e-15, large
4.6e-14), the six stepper variants (cgs_refine 0, 1, 2 x one handle, 3-rank group) with it.
"""
import numpy as np
import pytest

import fvens_amd as fa
import _oracle as orc
import cases
import gmres_host as gh
from test_gpu_implicit import _gather, _partitioned, to_device

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


class _Standalone:
    """one handle and the device copies of a random-block family's system (internal cell order)"""

    def __init__(self, family):
        self.s = s = gh.system_of(family)
        m = s.m
        self.N, Fi = m.nelem, m.naface - m.nbface
        self.dev = fa.FlowFV(m, cases.physics("naca"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
        self.perm = self.dev.permutation()
        self.dd = to_device(s.D.reshape(self.N, 16), self.perm)
        self.dl, self.du = to_device(s.lo.reshape(Fi, 16)), to_device(s.up.reshape(Fi, 16))
        self.dzero = _torch().zeros_like(self.dl)
        self.db = to_device(s.b, self.perm)

    def solve(self, rtol, maxit, restart, sweeps, db=None, offdiag=True):
        """-> iterations, reported residual norm, x in the mesh's cell order; d_x holds 7.0 on entry (the solver
        starts from x0 = 0 by its own fill)"""
        torch = _torch()
        dx = torch.full((self.N, 4), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dl, du = (self.dl, self.du) if offdiag else (self.dzero, self.dzero)
        it, rn = self.dev.gmres_blocks_device(self.dd.data_ptr(), dl.data_ptr(), du.data_ptr(),
                                              (self.db if db is None else db).data_ptr(), dx.data_ptr(), rtol, maxit,
                                              restart, sweeps)
        x = np.empty((self.N, 4))
        x[self.perm] = dx.cpu().numpy()
        return it, rn, x


@pytest.fixture(scope="module")
def standalone():
    held = {}

    def get(family):
        if family not in held:
            held[family] = _Standalone(family)
        return held[family]
    yield get
    for h in held.values():
        h.dev.close()


def _check_iterate(dev, family, restart, maxit, sweeps):
    h = gh.host_case(family, restart, maxit, sweeps, long=family != "large")
    s = dev.s
    it, rn, x = dev.solve(0.0, maxit, restart, sweeps)
    bar = gh.BAR_FACTOR * gh.FLOOR[family]
    err = gh.distance(family, x.ravel(), h.x, h.x)
    est = abs(rn / h.restated[1].rnorm - 1.0)
    true = abs(rn / np.linalg.norm(s.b.ravel() - s.A @ x.ravel()) - 1.0)
    print(f"GMRESDIFF {family} ({restart},{maxit},{sweeps}): x {err:.2e} = {err / bar:.3f} bar; residual norm against "
          f"host estimate {est:.2e} (bar {gh.est_bar(h):.1e}), against |b - A x| {true:.2e} (checked: {h.est_checked})")
    assert it == maxit
    assert np.all(np.isfinite(x)) and err <= bar
    assert est <= gh.est_bar(h)
    if h.est_checked:
        assert true <= gh.EST_BAR


@pytest.mark.parametrize("family,restart,maxit,sweeps",
                         [("fast",) + c for c in gh.FAST_CASES] + [("slow",) + c for c in gh.SLOW_CASES])
def test_standalone_iterate_matches_minimiser(standalone, family, restart, maxit, sweeps):
    _check_iterate(standalone(family), family, restart, maxit, sweeps)


@pytest.mark.parametrize("restart,maxit,sweeps", gh.LARGE_CASES)
def test_standalone_iterate_second_grid_stride_trip(standalone, restart, maxit, sweeps):
    """294,912 cells: an eighth of the multi-dot's and of k_maxpy_norm's lanes take a second trip"""
    dev = standalone("large")
    assert 2 * dev.N > 2048 * 256 and 2 * dev.N < 2 * 2048 * 256
    _check_iterate(dev, "large", restart, maxit, sweeps)


@pytest.mark.parametrize("rtol,restart", gh.STOP_CASES)
def test_standalone_stops_where_host_stops(standalone, rtol, restart):
    dev = standalone("fast")
    r = gh.host_case("fast", restart, gh.STOP_MAXIT, 1, rtol).restated[1]
    it, rn, x = dev.solve(rtol, gh.STOP_MAXIT, restart, 1)
    err = gh.distance("fast", x.ravel(), r.x, r.x)
    bar = gh.BAR_FACTOR * gh.FLOOR["fast"]
    print(f"GMRESDIFF stop rtol {rtol:g} restart {restart}: {it} iterations (host {r.iters}), x {err:.2e} = {err / bar:.3f} bar")
    assert it == r.iters
    assert err <= bar
    assert rn <= rtol * r.rnorm0


def test_standalone_zero_right_hand_side(standalone):
    dev = standalone("fast")
    it, rn, x = dev.solve(0.0, 5, 60, 1, db=_torch().zeros_like(dev.db))
    assert it == 0 and rn == 0.0
    assert np.array_equal(x, np.zeros_like(x))


def test_standalone_no_iterations(standalone):
    """maxit 0: x = 0 and the residual is b. |b| is a sum of 9,216 squares on both sides, each in a tree of at
    least pairwise quality: a relative error of some log2(9216) eps = 1.5e-15; the bar is 1e-13"""
    dev = standalone("fast")
    it, rn, x = dev.solve(0.0, 0, 60, 1)
    assert it == 0 and np.array_equal(x, np.zeros_like(x))
    assert abs(rn / np.linalg.norm(dev.s.b) - 1.0) <= 1e-13


def test_standalone_exact_preconditioner(standalone):
    """lo = up = 0 with one sweep: M = A, so w = v0 and the first projection removes all of it -- cgs_refine 1's
    second projection and its measured-norm branch decide the new norm from rounding alone. One step, x = D^-1 b"""
    dev = standalone("fast")
    s = dev.s
    it, rn, x = dev.solve(1e-10, 20, 60, 1, offdiag=False)
    x_ref = np.linalg.solve(s.D, s.b[..., None])[..., 0]
    err = gh.distance("fast", x.ravel(), x_ref.ravel(), x_ref.ravel())
    bar = gh.BAR_FACTOR * gh.FLOOR["fast"]
    print(f"GMRESDIFF exact preconditioner: {it} iteration, x {err:.2e} = {err / bar:.3f} bar, residual norm {rn:.2e}")
    assert it == 1
    assert np.all(np.isfinite(x)) and np.isfinite(rn)
    assert err <= bar
    assert rn <= 1e-10 * np.linalg.norm(s.b)


# ---- the steppers' paths -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def steppers():
    """one handle and one 3-rank in-process group on naca_small, kept over the cases"""
    s = gh.step_system()
    one = fa.FlowFV(s.m, s.p, s.n)
    sps, dus, glob = _partitioned(s.m, s.p, s.n, s.u0, 3)
    grp = fa.FlowFVGroup(sps)
    yield one, (sps, dus, glob, grp)
    grp.close()
    for h in sps:
        h.close()
    one.close()


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("restart,k", gh.STEP_CASES)
@pytest.mark.parametrize("group", [False, True], ids=["one", "group3"])
@pytest.mark.parametrize("refine", [0, 1, 2])
def test_backward_euler_step_iterate_matches_minimiser(steppers, refine, group, restart, k, sweeps):
    torch = _torch()
    s = gh.step_system()
    h = gh.host_case("jacobian", restart, k, sweeps)
    du = h.minimiser.x.reshape(-1, 4)
    u1 = orc.relaxed_update(s.u0, du, s.p.gamma, 1.0)
    res0 = np.sqrt(np.sum(s.r[:, 3] * s.r[:, 3] * s.m.area[:s.m.nelem]))
    cfg = fa.ImplicitConfig(cgs_refine=refine, cflinit=gh.STEP_CFL, cflfin=gh.STEP_CFL, tol=0.0, maxiter=1, lin_rtol=0.0,
                            lin_maxit=k, restart=restart, prec_sweeps=sweeps, min_relax=1.0)
    one, (sps, dus, glob, grp) = steppers
    if group:
        for spk, d, g in zip(sps, dus, glob):
            d.fill_(float("nan"))
            d[:spk.nown] = torch.tensor(s.u0[g], device="cuda")
        torch.cuda.synchronize()
        st, hist = grp.steady_backward_euler_device([d.data_ptr() for d in dus], cfg)
        u = _gather(s.u0, sps, dus, glob)
    else:
        perm = one.permutation()
        dU = to_device(s.u0, perm)
        torch.cuda.synchronize()
        st, hist = one.steady_backward_euler_device(dU.data_ptr(), cfg)
        u = np.empty_like(s.u0)
        u[perm] = dU.cpu().numpy()
    bar = gh.BAR_FACTOR * gh.FLOOR["jacobian"]
    err = np.abs(u - u1).max(axis=0) / np.abs(u1 - s.u0).max(axis=0)
    worst = abs(st["lin_worst"] / (h.restated[refine].rnorm / h.bnorm) - 1.0)
    print(f"GMRESDIFF jacobian refine {refine} {'group' if group else 'one'} ({restart},{k},{sweeps}): du {err.max():.2e} = "
          f"{err.max() / bar:.3f} bar; lin_worst against host estimate {worst:.2e} (bar {gh.est_bar(h):.1e}); "
          f"hist[0] {abs(hist[0] / res0 - 1.0):.2e}")
    assert st["steps"] == 1 and st["lin_iters"] == k and st["lin_unconverged"] == 1
    assert np.all(np.isfinite(u)) and np.all(err <= bar), err / bar
    assert worst <= gh.est_bar(h)
    assert abs(hist[0] - res0) <= 1e-12 * res0


def test_backward_euler_energy_norm_second_grid_stride_trip():
    """hist[0] = sqrt(sum r_E^2 area) over 294,912 cells: k_energy_partial's lanes below 32,768 take a second trip"""
    torch = _torch()
    m = gh.large_mesh()
    assert m.nelem > 512 * 256
    om = orc.OracleMesh.from_raw(m.raw())
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u0 = cases.state(m, p, 8)
    r, dtm = np.zeros((m.nelem, 4)), np.zeros(m.nelem)
    orc.OracleSpatial(om, p, n).compute_residual(u0, r, True, dtm)
    res0 = np.sqrt(np.sum(r[:, 3] * r[:, 3] * m.area[:m.nelem]))
    dev = fa.FlowFV(m, p, n)
    dU = to_device(u0, dev.permutation())
    torch.cuda.synchronize()
    cfg = fa.ImplicitConfig(cflinit=gh.STEP_CFL, cflfin=gh.STEP_CFL, tol=0.0, maxiter=1, lin_rtol=0.0, lin_maxit=1, restart=2,
                            prec_sweeps=1, min_relax=1.0)
    st, hist = dev.steady_backward_euler_device(dU.data_ptr(), cfg)
    finite = bool(torch.isfinite(dU).all().item())
    dev.close()
    print(f"GMRESDIFF large hist[0] {abs(hist[0] / res0 - 1.0):.2e}")
    assert st["steps"] == 1 and st["lin_iters"] == 1 and finite
    assert abs(hist[0] - res0) <= 1e-12 * res0
