"""CPU checks of the host GMRES restatements (tests/gmres_host.py) that tests/test_gpu_gmres.py holds the device
to, for every case and seed the GPU tests use:
  * floor: the host forms (the restated algorithm with cgs_refine 1 -- 0, 1 and 2 on the Jacobian system --, its
    long-double-dot variant, the least-squares minimiser) agree to the family's FLOOR constant (printed);
  * teeth: one more Arnoldi step moves x by at least 1000 iterate bars (1e6 floors), so a device iterate that
    is off by one step, or by a thousandth of one, cannot pass;
  * estimate: where |r_k| >= 1e-4 |b|, the recursion's residual estimate equals |b - A x_k| to 1e-12;
  * consistency: the restatement run to rtol 1e-12 lands on scipy's direct solution (on the large mesh, where a
    direct solve is out of reach, on |b - A x| <= 1e-12 |b| computed apart from it);
  * stopping: in the rtol-stopped cases no tested residual is within 1 % of rtol |b|, so the device's
    iteration count cannot legitimately differ from the host's.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gmres_host as gh

CASES = ([("fast",) + c for c in gh.FAST_CASES] + [("slow",) + c for c in gh.SLOW_CASES]
         + [("jacobian", m, k, s) for (m, k) in gh.STEP_CASES for s in (1, 2)] + [("large",) + c for c in gh.LARGE_CASES])


@pytest.mark.parametrize("family,restart,maxit,sweeps", CASES)
def test_floor_teeth_estimate(family, restart, maxit, sweeps):
    h = gh.host_case(family, restart, maxit, sweeps)
    bar = gh.BAR_FACTOR * gh.FLOOR[family]
    print(f"{family} ({restart},{maxit},{sweeps}): floor {h.floor:.2e} (constant {gh.FLOOR[family]:.1e}), "
          f"|x_k - x_k-1| {h.step:.2e}, |r_k|/|b| {h.true_rel:.2e}, estimate gap {h.est_gap:.2e}, "
          f"estimate checked: {h.est_checked}")
    for r in list(h.restated.values()) + [h.long]:
        assert r.iters == maxit and len(r.est) == maxit
    assert h.floor <= gh.FLOOR[family]
    assert h.step >= gh.TEETH_FACTOR * bar, "replace this case: one step moves x by less than 1000 bars"
    if h.est_checked:
        assert h.est_gap <= gh.EST_GAP


def test_estimate_is_checked_in_every_family():
    for family in ("fast", "slow", "jacobian", "large"):
        assert any(gh.host_case(*c).est_checked for c in CASES if c[0] == family), family


@pytest.mark.parametrize("family,sweeps", [("fast", 1), ("fast", 2), ("slow", 1), ("jacobian", 1), ("jacobian", 2)])
def test_restatement_converges_to_direct_solution(family, sweeps):
    s = gh.system_of(family)
    b = s.b.ravel()
    x_ref = spla.spsolve(s.A.tocsc(), b)
    Minv = gh.jacobi_prec(s.A, s.Dinv, sweeps)
    for refine in (0, 1, 2):
        r = gh.gmres_restated(s.A, Minv, b, 1e-12, 3000, 128 if family == "slow" else 60, refine)
        assert r.iters < 3000 and r.rnorm <= 1e-12 * r.rnorm0
        assert np.linalg.norm(b - s.A @ r.x) <= 1e-11 * np.linalg.norm(b)
        assert gh.distance(family, r.x, x_ref, x_ref) <= 1e-8, (family, sweeps, refine)


def test_restatement_converges_on_large_mesh():
    s = gh.system_of("large")
    b = s.b.ravel()
    r = gh.gmres_restated(s.A, gh.jacobi_prec(s.A, s.Dinv, 1), b, 1e-12, 200, 60, 1)
    assert r.iters < 200 and np.linalg.norm(b - s.A @ r.x) <= 1e-11 * np.linalg.norm(b)


@pytest.mark.parametrize("rtol,restart", gh.STOP_CASES)
def test_stopping_is_not_marginal(rtol, restart):
    h = gh.host_case("fast", restart, gh.STOP_MAXIT, 1, rtol)
    r = h.restated[1]
    print(f"rtol {rtol:g} restart {restart}: {r.iters} iterations, host forms differ by {h.floor:.2e}")
    assert 0 < r.iters < gh.STOP_MAXIT and h.long.iters == r.iters and r.rnorm <= rtol * r.rnorm0
    assert h.floor <= gh.FLOOR["fast"]
    assert np.all(np.abs(np.array(r.tested) / (rtol * r.rnorm0) - 1.0) > 0.01)
    if restart < r.iters:                       # cycles were cut: the restarts' true residuals were tested too
        assert len(r.tested) > r.iters
