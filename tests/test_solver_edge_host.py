"""CPU proof of the cases of tests/solver_edge_cases.py, which tests/test_gpu_solver_edge.py runs on the device: from
the oracle and numpy alone, for every listed case,
  * the system is finite and its right-hand side non-zero in every variable;
  * the host forms agree among themselves to the family's floor (the minimiser; gmres_restated with cgs_refine 0, 1
    and 2; both routes to the rounded inverse under prec_single; numpy's LU and a one-ended block Thomas in fp64 and
    np.longdouble for the line solve);
  * the case has teeth: one Arnoldi step, another sweep count, Jacobi for Gauss-Seidel and one domain's form for the
    three-rank form each move the iterate by at least TEETH_FACTOR bars;
  * gmres_restated exhausts the Krylov space within 4N steps; the explicit drivers' host loops stay finite and move.
Structures come from the host builders (test_precond_setup_host.py's shim) at LINE_THRESHOLD; the RCB partition the
shim cuts is asserted to be the explicit partition the device groups use. Every test prints its floors and steps.
"""
import functools

import numpy as np
import pytest

import fvens_amd as fa
import gmres_host as gh
import solver_edge_cases as sec
import test_precond_setup_host as psh
from test_gmres_host import _other_forms

needs_hipcc = psh.needs_hipcc
SEEN = {}          # family -> (largest floor, smallest step) over the cases run so far, printed by the last test


def _seen(family, floor, step=np.inf):
    f, s = SEEN.get(family, (0.0, np.inf))
    SEEN[family] = (max(f, floor), min(s, step))
ALL_MESHES = list(sec.P_MESHES) + [f"C{n}" for n in sec.C_LENGTHS]


@functools.lru_cache(maxsize=None)
def host_ranks(name, nparts):
    """the ranks of a mesh as gh.PrecHost takes them, from the host builders"""
    m, _ = sec.mesh(name)
    part = np.zeros(m.nelem, np.int32)
    if nparts > 1:
        part = fa.partition_rcb(m, nparts)
        assert np.array_equal(part, sec.PARTS[name]), (name, part)
    ranks = []
    for k in range(nparts):
        o = psh.host_structures(m, sec.PHYSICS, sec.LINE_THRESHOLD, nparts, k)
        st = o["start"]
        ranks.append(sec.rank_of(o["colour"], [(o["cells"][a:b], o["faces"][a:b]) for a, b in zip(st[:-1], st[1:])],
                                 np.nonzero(part == k)[0][o["perm"]]))
    return tuple(ranks)


@functools.lru_cache(maxsize=None)
def prec_host(name, nparts):
    return gh.PrecHost(sec.step_system(name), list(host_ranks(name, nparts)))


# ---- the systems ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL_MESHES)
def test_system_is_finite(name):
    """Roe + least squares + Van Albada: residual, time steps and Jacobian finite in every cell, b non-zero in every
    variable (the first-order fallback is not needed on any of these meshes)"""
    s = sec.step_system(name)
    for a in (s.u0, s.r, s.D, s.lo, s.up):
        assert np.all(np.isfinite(a)), name
    assert np.all(np.abs(s.b).max(axis=0) > 0.0)
    print(f"{name}: {s.m.nelem} cells, max |b| per variable {np.abs(s.b).max(axis=0)}, cond(A) "
          f"{np.linalg.cond(s.A.toarray()):.2e}")
    m = s.m
    assert m.naface - m.nbface == {"P11": 0, "P21": 1, "P13": 2, "P32": 7}.get(name, m.nelem - 1)


@needs_hipcc
@pytest.mark.parametrize("name", ALL_MESHES)
def test_line_shapes(name):
    """the builders' lines at LINE_THRESHOLD: a C column is one line, cut at 256; the default threshold leaves
    every cell of a column on its own (the column's coupling ratios stay below 4)"""
    lens = [len(c) for c, _ in host_ranks(name, 1)[0].lines]
    print(f"{name}: lines {lens}, colours {int(host_ranks(name, 1)[0].colour.max()) + 1}")
    if name.startswith("C"):
        assert lens == sec.expected_line_lengths(name)
        o = psh.host_structures(sec.mesh(name)[0], sec.PHYSICS, 0.0)
        assert np.all(np.diff(o["start"]) == 1)
    else:
        assert lens == {"P11": [1], "P21": [2], "P13": [3]}.get(name, lens) and sum(lens) == sec.mesh(name)[0].nelem
    assert int(host_ranks(name, 1)[0].colour.max()) + 1 == (1 if name == "P11" else 2)


# ---- the block operator and the line solve --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sec.P_MESHES))
def test_operator_bar_has_teeth(name):
    """the long-double product against the CSR product in double: inside the derived bar 32 eps (|A| |x|); one block
    dropped from a row is outside it"""
    s = sec.fast_system(name)
    y, a = sec.long_product(s, s.x)
    yd = (s.A @ s.x.ravel()).reshape(-1, 4)
    bar = 32 * np.finfo(np.float64).eps * a
    assert np.all(np.abs(yd - y) <= bar)
    ydrop = np.einsum("cij,cj->ci", s.D, s.x) if s.lo.size else 0.0 * yd
    assert np.any(np.abs(ydrop - y) > 1e6 * bar)


@needs_hipcc
@pytest.mark.parametrize("name", [f"C{n}" for n in sec.C_LENGTHS] + ["P11", "P13", "P32"])
def test_line_dense_forms_agree(name):
    """z = M^-1 v by numpy's LU and by a one-ended block Thomas in fp64 and np.longdouble: their largest disagreement
    is the floor of the device's dense comparison"""
    s = sec.line_blocks(name)
    r = host_ranks(name, 1)[0]
    M = sec.line_matrix(s, r.glob, r.lines)
    v = s.v.ravel()
    z = np.linalg.solve(M, v)
    forms = [z]
    if len(r.lines) == 1:                       # one line in order: M is block tridiagonal along it
        order = (4 * r.glob[r.lines[0][0]][:, None] + np.arange(4)[None]).ravel()
        Mo, vo = M[np.ix_(order, order)], v[order]
        for T in (np.float64, np.longdouble):
            zt = np.zeros(v.size)
            zt[order] = sec.block_thomas(Mo, vo, T).astype(np.float64)
            forms.append(zt)
    floor = max(np.abs(a - b).max() for a in forms for b in forms) / np.abs(z).max()
    print(f"{name}: line solve host forms differ by {floor:.2e} of max |z| (constant {sec.FLOORS['line_dense']:.1e}), "
          f"|M z - v| {np.abs(M @ z - v).max() / np.abs(v).max():.2e}")
    _seen("line_dense", floor)
    assert floor <= sec.FLOORS["line_dense"]
    # teeth: M without one link's blocks is far outside the bar
    if len(v) > 4 and np.any(M[4:8, 0:4]):
        M2 = M.copy()
        M2[4:8, 0:4] = 0.0
        assert np.abs(np.linalg.solve(M2, v) - z).max() >= gh.TEETH_FACTOR * sec.BAR["line_dense"] * np.abs(z).max()


# ---- stand-alone GMRES ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def standalone_case(name, restart, k, sweeps):
    s = sec.fast_system(name)
    b = s.b.ravel()
    Minv = gh.jacobi_prec(s.A, s.Dinv, sweeps)
    mn = gh.gmres_minimiser(s.A, Minv, b, k, restart)
    rs = [gh.gmres_restated(s.A, Minv, b, 0.0, k, restart, 1), gh.gmres_restated(s.A, Minv, b, 0.0, k, restart, 1, longdot=True)]
    xs = [r.x for r in rs] + [mn.x]
    floor = max(gh.distance("fast", a, c, mn.x) for a in xs for c in xs)
    return mn, rs, floor, gh.distance("fast", mn.x, mn.xprev, mn.x)


@pytest.mark.parametrize("name,restart,k,sweeps", sec.STANDALONE_CASES)
def test_standalone_floor_and_teeth(name, restart, k, sweeps):
    mn, rs, floor, step = standalone_case(name, restart, k, sweeps)
    s = sec.fast_system(name)
    print(f"{name} ({restart},{k},{sweeps}): floor {floor:.2e} (constant {sec.FLOORS['standalone']:.1e}), "
          f"|x_k - x_k-1| {step:.2e}, |r_k|/|b| {mn.rnorm / np.linalg.norm(s.b):.2e}")
    _seen("standalone", floor, step)
    assert k <= 4 * s.m.nelem - 1
    assert all(r.iters == k for r in rs)
    assert floor <= sec.FLOORS["standalone"]
    assert step >= gh.TEETH_FACTOR * sec.BAR["standalone"], "remove this case: one step moves x by less than 1000 bars"
    other = gh.gmres_minimiser(s.A, gh.jacobi_prec(s.A, s.Dinv, 3 - sweeps), s.b.ravel(), k, restart)
    d = gh.distance("fast", mn.x, other.x, mn.x)
    print(f"  against {3 - sweeps} sweep(s): {d:.2e}")
    assert d >= gh.TEETH_FACTOR * sec.BAR["standalone"], "remove this case: the other sweep count is within 1000 bars"


@pytest.mark.parametrize("name,sweeps", sec.EXHAUST_CASES)
def test_restatement_exhausts_the_space(name, sweeps):
    """rtol 1e-10, maxit 8N, restart 60: gmres_restated stops within 4N steps on a solution to the direct-solve bar"""
    s = sec.fast_system(name)
    N, b = s.m.nelem, s.b.ravel()
    Minv = gh.jacobi_prec(s.A, s.Dinv, sweeps)
    for refine in (0, 1, 2):
        r = gh.gmres_restated(s.A, Minv, b, sec.EXHAUST_RTOL, 8 * N, sec.EXHAUST_RESTART, refine)
        print(f"{name} sweeps {sweeps} refine {refine}: {r.iters} iterations of at most {4 * N}, |r|/|b| {r.rnorm / r.rnorm0:.2e}")
        assert 1 <= r.iters <= 4 * N and np.all(np.isfinite(r.x))
        assert r.rnorm <= sec.EXHAUST_RTOL * r.rnorm0
        assert np.linalg.norm(b - s.A @ r.x) <= 1e-8 * np.linalg.norm(b)
    if name == "P11":
        assert r.iters == 1


# ---- one backward-Euler step ----------------------------------------------------------------------------------------

@needs_hipcc
@pytest.mark.parametrize("name,kind,sweeps,restart,k,single", sec.step_cases())
def test_step_floor_and_teeth(name, kind, sweeps, restart, k, single):
    P = prec_host(name, 1)
    h = P.case(kind, sweeps, restart, k, single)
    fam = sec.step_family(kind)
    print(f"{name} {kind} {sweeps} ({restart},{k}) single {single}: floor {h.floor:.2e} (constant {sec.FLOORS[fam]:.1e}), "
          f"|x_k - x_k-1| {h.step:.2e}, |r_k|/|b| {h.true_rel:.2e}, iterations {h.iters}")
    _seen("step " + kind + (" fp32" if single else ""), h.floor, h.step)
    assert h.iters == [k] * len(h.iters)
    assert h.floor <= sec.FLOORS[fam]
    assert h.step >= gh.TEETH_FACTOR * sec.BAR[fam], "remove this case: one step moves x by less than 1000 bars"


@needs_hipcc
@pytest.mark.parametrize("name,kind,sweeps,restart,k", sorted({c[:5] for c in sec.step_cases()}))
def test_step_forms_are_told_apart(name, kind, sweeps, restart, k):
    """another sweep count, Jacobi for Gauss-Seidel, every sweep ascending, the ILU's colours reversed: each leaves
    the k-th iterate at least 1000 bars from the case's, or is the same operator on this mesh (then named here)"""
    P = prec_host(name, 1)
    x = P.iterate(kind, sweeps, restart, k).x
    for what, (okind, osweeps, variant, _) in _other_forms(kind, sweeps, 1):
        if sec.exact(name, kind):
            continue                                     # M = A: every sweep count and colour order is the exact solve
        y = P.iterate(okind, osweeps, restart, k, variant=variant).x
        d = gh.distance("jacobian", x, y, x)
        bar = sec.BAR[sec.step_family(kind)]
        print(f"{name} {kind} {sweeps} ({restart},{k}) against {what}: {d:.2e} = {d / bar:.1e} bars")
        assert d >= gh.TEETH_FACTOR * bar, f"remove this case: {what} is within 1000 bars"


@needs_hipcc
@pytest.mark.parametrize("name,kind,sweeps,restart,k", sec.group_step_cases())
def test_group_step_floor_and_teeth(name, kind, sweeps, restart, k):
    P, P1 = prec_host(name, 3), prec_host(name, 1)
    h = P.case(kind, sweeps, restart, k, False)
    print(f"{name} 3 ranks {kind} {sweeps} ({restart},{k}): floor {h.floor:.2e}, |x_k - x_k-1| {h.step:.2e}")
    _seen("step 3 ranks " + kind, h.floor, h.step)
    fam = sec.step_family(kind)
    assert h.iters == [k] * len(h.iters)
    assert h.floor <= sec.FLOORS[fam]
    assert h.step >= gh.TEETH_FACTOR * sec.BAR[fam]
    if kind != "jacobi":          # Jacobi sweeps read the previous iterate everywhere: one domain's operator
        if sec.exact(name, kind):
            return                # one domain's operator is A^-1: it has no second iterate to compare
        d = gh.distance("jacobian", h.x, P1.iterate(kind, sweeps, restart, k).x, h.x)
        print(f"  against one domain's form: {d:.2e} = {d / sec.BAR[fam]:.1e} bars")
        assert d >= gh.TEETH_FACTOR * sec.BAR[fam]


@needs_hipcc
def test_p13_ranks_are_block_jacobi():
    """one cell per rank: no rank has a face of its own, so Gauss-Seidel, ILU(0) and the line solve on the three ranks
    of P13 are block Jacobi with the same sweeps (recorded, not tested as a difference between them)"""
    P = prec_host("P13", 3)
    assert not P.same.any()
    v = np.random.default_rng(2).standard_normal(12)
    for sweeps in (1, 2):
        z = P.minv("jacobi", sweeps)(v)
        for kind in ("ilu", "lines"):
            assert np.abs(P.minv(kind, sweeps)(v) - z).max() <= 1e-13 * np.abs(z).max(), (kind, sweeps)
    # Gauss-Seidel starts from zero: its first sweep is D^-1 v, its s-th the (s-1)-th Jacobi correction
    assert np.abs(P.minv("gs", 1)(v) - P.minv("jacobi", 1)(v)).max() <= 1e-13 * np.abs(v).max()


@pytest.mark.parametrize("name", ["P11"])
def test_p11_every_preconditioner_is_exact(name):
    s = sec.step_system(name)
    du = np.linalg.solve(s.A.toarray(), s.b.ravel())
    r = gh.gmres_restated(s.A, gh.jacobi_prec(s.A, s.Dinv, 1), s.b.ravel(), 1e-10, 8, 60, 0)
    print(f"P11: cond(A) {np.linalg.cond(s.A.toarray()):.2e}, {r.iters} iteration, du against the dense solve "
          f"{gh.distance('jacobian', r.x, du, du):.2e}")
    assert r.iters == 1 and gh.distance("jacobian", r.x, du, du) <= sec.FLOORS["step"]


# ---- the explicit drivers -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sec.P_MESHES))
@pytest.mark.parametrize("driver,order,mode", sec.DRIVER_CASES)
def test_driver_host_loops_run(name, driver, order, mode):
    h = sec.host_driver(name, driver, order, mode)
    u0 = sec.driver_state(name)
    print(f"{name} {driver} order {order} {mode}: {h.steps} steps, time {h.time}, max |u - u0| {np.abs(h.u - u0).max():.2e}")
    assert h.steps == sec.DRIVER_STEPS and np.all(np.isfinite(h.u))
    assert np.abs(h.u - u0).max() > 1e-9          # the steps moved the state
    if h.rec is not None:
        assert h.rec.shape == (sec.DRIVER_STEPS, 6) and np.all(np.isfinite(h.rec))


def test_zz_floors_and_surviving_cases():
    """prints what the run measured (the floors of solver_edge_cases.FLOORS come from these lines) and the lists the
    device file gets; asserts what must survive"""
    for family, (floor, step) in sorted(SEEN.items()):
        print(f"FLOOR {family}: largest host-form difference {floor:.2e}, smallest step {step:.2e}")
    steps = sec.step_cases()
    print(f"stand-alone cases {len(sec.STANDALONE_CASES)}: {sec.STANDALONE_CASES}")
    print(f"step cases {len(steps)}, group step cases {len(sec.group_step_cases())}, driver cases {len(sec.DRIVER_CASES)} "
          f"on {list(sec.P_MESHES)}, line columns {sec.C_LENGTHS}")
    for name in sec.STEP_MESHES:
        for kind, sweeps in gh.PREC_KINDS:
            assert any(c[:3] == (name, kind, sweeps) for c in steps), (name, kind, sweeps)
        assert any(c[0] == name and c[2] >= 2 for c in sec.STANDALONE_CASES), name
