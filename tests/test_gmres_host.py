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
For the other preconditioners (gmres_host.PrecHost; the device side is tests/test_gpu_precond_iterate.py), on
structures from the host builders: the same floor, teeth, estimate and consistency checks for every case, on one domain
and in the 3-rank form; that every neighbouring operator (another sweep count, Jacobi for Gauss-Seidel, every sweep
ascending, reversed ILU colours, one domain's form for the group's, no halo exchange) leaves the iterate at least 1000
bars away; that prec_single moves it by at least 10 bars; and that the line system's lines cover the line solver's paths.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import fvens_amd as fa
import gmres_host as gh
import test_precond_setup_host as psh

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


# ---- the other preconditioners (tests/test_gpu_precond_iterate.py) ----------------------------------------------------
# Structures come from the host builders (test_precond_setup_host.py's shim), which test_gpu_precond_structures.py
# shows to be the handles': one domain, and the three ranks of the RCB partition the GPU test's group runs on.

@functools.lru_cache(maxsize=None)
def prec_host(lines, nparts):
    """PrecHost of the step system (the line system if lines) on nparts ranks, structures from the host builders"""
    s = gh.line_system() if lines else gh.step_system()
    part = fa.partition_rcb(s.m, nparts) if nparts > 1 else np.zeros(s.m.nelem, np.int32)
    ranks = []
    for k in range(nparts):
        o = psh.host_structures(s.m, "naca", nparts=nparts, rank=k)
        st = o["start"]
        ranks.append(SimpleNamespace(glob=np.nonzero(part == k)[0][o["perm"]], colour=o["colour"],
                                     lines=[(o["cells"][a:b], o["faces"][a:b]) for a, b in zip(st[:-1], st[1:])]))
    return gh.PrecHost(s, ranks)


def _prec_cases():
    out = [(kind, sw, m, k, single, 1) for kind, sw in gh.PREC_KINDS for m, k in gh.PREC_STEP_CASES
           for single in ((False,) if kind == "lines" else (False, True))]
    return out + [(kind, sw, m, k, False, gh.PREC_RANKS) for kind, sw in gh.PREC_GROUP_KINDS
                  for m, k in gh.PREC_GROUP_STEP_CASES]


PREC_BAR = gh.BAR_FACTOR * gh.FLOOR["jacobian"]


@psh.needs_hipcc
def test_line_system_covers_the_line_solver():
    """twisted lines in an odd number that leaves the last twisted group part-filled, and lines of one cell, on one
    domain and on every rank; naca_small's lines are all short (what the other kinds' cases do not depend on)"""
    for nparts in (1, gh.PREC_RANKS):
        for r in prec_host(True, nparts).ranks:
            twisted, singles = gh.line_coverage(r.lines)
            print(f"{nparts} rank(s): {len(r.lines)} lines, {twisted} twisted, {singles} of one cell")
            assert twisted > 0 and singles > 0
            if nparts == 1:
                assert twisted % 2 == 1 and twisted % 32 not in (0, 31)
    assert gh.line_system().m.nelem < 5000


@psh.needs_hipcc
@pytest.mark.parametrize("kind,sweeps,restart,k,single,nparts", _prec_cases())
def test_prec_floor_teeth_estimate(kind, sweeps, restart, k, single, nparts):
    P = prec_host(kind == "lines", nparts)
    h = P.case(kind, sweeps, restart, k, single)
    print(f"{kind} {sweeps} ({restart},{k}) single {single} ranks {nparts}: floor {h.floor:.2e} (constant "
          f"{gh.FLOOR['jacobian']:.1e}), |x_k - x_k-1| {h.step:.2e}, |r_k|/|b| {h.true_rel:.2e}, estimate gap "
          f"{h.est_gap:.2e}, estimate checked: {h.est_checked}")
    assert h.iters == [k] * len(h.iters)
    assert h.floor <= gh.FLOOR["jacobian"]
    assert h.step >= gh.TEETH_FACTOR * PREC_BAR, "replace this case: one step moves x by less than 1000 bars"
    if h.est_checked:
        assert h.est_gap <= gh.EST_GAP
    if single:
        # a device that ignores prec_single, or rounds another array, is off by the distance to the fp64 iterate
        flips = int(np.count_nonzero(P.dinv(kind, True, "numpy") != P.dinv(kind, True, "inv4")))
        d = gh.distance("jacobian", h.x, P.iterate(kind, sweeps, restart, k).x, h.x)
        print(f"  fp32 against fp64 iterate {d:.2e} = {d / PREC_BAR:.0f} bars; np.linalg.inv and inv4 differ in {flips} "
              f"of {P.dinv(kind, True, 'numpy').size} fp32 entries")
        assert d >= gh.SINGLE_FACTOR * PREC_BAR, "replace this case: prec_single moves x by less than 10 bars"


def _other_forms(kind, sweeps, nparts):
    """(name, (kind, sweeps, variant, nparts)) of the host forms a case's iterate must stay away from"""
    out = [(f"{sweeps + d} sweeps", (kind, sweeps + d, None, nparts)) for d in (-1, 1) if sweeps + d >= 1]
    if kind == "gs":
        out.append(("Jacobi", ("jacobi", sweeps, None, nparts)))
        if sweeps > 1:      # also what reversing the backward colour order in LinOp::gaussSeidel gives
            out.append(("every sweep ascending", (kind, sweeps, "forward", nparts)))
    if kind == "ilu":
        out.append(("colours reversed", (kind, sweeps, "reversed", nparts)))
    if nparts > 1:
        if kind != "jacobi":    # Jacobi sweeps read the previous iterate everywhere: the group's operator is one domain's
            out.append(("one domain", (kind, sweeps, None, 1)))
        if kind in ("jacobi", "gs"):   # what dropping S.exchange before a sweep gives (ghost rows left at zero)
            out.append(("no exchange", (kind, sweeps, "noexchange", nparts)))
    return out


@psh.needs_hipcc
@pytest.mark.parametrize("kind,sweeps,restart,k,nparts", sorted({c[:4] + c[5:] for c in _prec_cases()}))
def test_prec_forms_are_told_apart(kind, sweeps, restart, k, nparts):
    """a wrong operator is not a small error: every neighbouring host form (another sweep count -- one sweep fewer
    is also what a wrong parity of buf(k) in LinOp::precondition leaves in z --, Jacobi for Gauss-Seidel, every
    sweep ascending, the ILU's colours reversed, the group's form against one domain's, no halo exchange between
    sweeps) leaves the k-th iterate at least 1000 bars from the case's"""
    x = prec_host(kind == "lines", nparts).iterate(kind, sweeps, restart, k).x
    for name, (okind, osweeps, variant, oparts) in _other_forms(kind, sweeps, nparts):
        y = prec_host(kind == "lines", oparts).iterate(okind, osweeps, restart, k, variant=variant).x
        d = gh.distance("jacobian", x, y, x)
        print(f"{kind} {sweeps} ({restart},{k}) ranks {nparts} against {name}: {d:.2e} = {d / PREC_BAR:.1e} bars")
        assert d >= gh.TEETH_FACTOR * PREC_BAR, f"replace this case: {name} is within 1000 bars"


@psh.needs_hipcc
@pytest.mark.parametrize("kind,sweeps,single,nparts", sorted({(c[0], c[1], c[4], c[5]) for c in _prec_cases()}))
def test_prec_restatement_converges_to_direct_solution(kind, sweeps, single, nparts):
    P = prec_host(kind == "lines", nparts)
    s = P.s
    b = s.b.ravel()
    x_ref = spla.spsolve(s.A.tocsc(), b)
    for route in ("numpy", "inv4") if single else ("numpy",):
        Minv = P.minv(kind, sweeps, single, route)
        for refine in (0, 1, 2):
            r = gh.gmres_restated(s.A, Minv, b, 1e-12, 3000, 60, refine)
            assert r.iters < 3000 and r.rnorm <= 1e-12 * r.rnorm0
            assert np.linalg.norm(b - s.A @ r.x) <= 1e-11 * np.linalg.norm(b)
            assert gh.distance("jacobian", r.x, x_ref, x_ref) <= 1e-8, (kind, sweeps, single, route, refine)


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
