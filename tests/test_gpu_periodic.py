"""Periodic boundaries on the device: a periodic mesh (UMesh.periodic: each periodic face pair a pair of
connectivity faces of the mesh with itself) through the ordinary handle, whose exchanges are gathers on the
device (k_ghost_gather). The reference has no periodic flow code to compare with (abc.hpp:3), so the bar is tile
equivalence: the residual, operator and explicit steps on a periodic box P equal the ORACLE's single-domain ones
on the 3 x 3 tiling T of P (outer boundary: far field) at the centre tile's cells. Bounds 1e-12 of the largest
entry, the bar the project holds for two-sided connectivity faces against one domain (test_rankmesh.py:99-100).
Ghost rows start as NaN so that a missed exchange cannot pass."""
import numpy as np
import pytest

import fvens_amd as fa
import _oracle as orc
import cases
import periodic_meshes as pmesh
from test_rankmesh import SCHEMES

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("periodic")


_CASES = {}


class Case:
    """P (periodic), T (its tiling, product and oracle mesh) and the map of the centre tile's cells"""

    def __init__(self, workdir, nx, ny, kind, wrap_y):
        tag = f"{nx}x{ny}{kind}{int(wrap_y)}"
        pp, tp = workdir / f"P{tag}.msh", workdir / f"T{tag}.msh"
        self.wrap_y = wrap_y
        pmesh.write_tiling(pp, nx, ny, kind, 1, 1, markers=(5, 4, 5, 4) if wrap_y else (2, 4, 3, 4))
        tx, ty = (3, 3) if wrap_y else (3, 1)
        tile, local = pmesh.write_tiling(tp, nx, ny, kind, tx, ty, markers=(9, 9, 9, 9) if wrap_y else (2, 9, 3, 9))
        self.P = fa.UMesh.read_gmsh(pp).periodic([(4, 0)] + ([(5, 1)] if wrap_y else []))
        self.T = fa.UMesh.read_gmsh(tp)
        self.oT = orc.OracleMesh.read(tp)
        self.local = local
        self.centre = np.nonzero((tile[:, 0] == 1) & (tile[:, 1] == (1 if wrap_y else 0)))[0]
        np.testing.assert_array_equal(local[self.centre], np.arange(self.P.nelem))
        self.ntiles = tx * ty
        self.ref = {}

    def physics(self, kind):
        """(physics on P, physics on T): the walls of the channel on both, the far field round T only"""
        p, t = cases.physics(kind), cases.physics(kind)
        walls = [] if self.wrap_y else [fa.FlowBCConfig("slipwall", 2), fa.FlowBCConfig("slipwall", 3)]
        p.bcconf = list(walls)
        t.bcconf = walls + [fa.FlowBCConfig("farfield", 9)]
        return p, t

    def state(self, p, seed=3):
        """(smooth state on P with integer wavenumbers, its replica on T)"""
        u = pmesh.smooth_state(self.P.rc[:self.P.nelem], p, seed=seed, wrap_y=self.wrap_y)
        return u, np.ascontiguousarray(u[self.local])

    def oracle_residual(self, kind, flux, grad, rec, order2):
        """the oracle's residual and time steps on T for the replicated state, computed once per scheme"""
        key = (kind, flux, grad, rec, order2)
        if key not in self.ref:
            p, pt = self.physics(kind)
            n = cases.numerics(flux, grad, rec, order2=order2)
            u, uT = self.state(p)
            r = np.zeros((self.T.nelem, 4))
            dt = np.zeros(self.T.nelem)
            orc.OracleSpatial(self.oT, pt, n).compute_residual(uT, r, True, dt)
            assert np.isfinite(r).all() and np.isfinite(dt).all()        # the oracle alone stays finite on T
            self.ref[key] = (p, n, u, r[self.centre], dt[self.centre])
        return self.ref[key]


def case(workdir, nx=8, ny=8, kind="quad", wrap_y=True):
    key = (nx, ny, kind, wrap_y)
    if key not in _CASES:
        _CASES[key] = Case(workdir, nx, ny, kind, wrap_y)
    return _CASES[key]


def ghost_order(m):
    """connectivity face of each ghost row of a periodic handle's device arrays: (pair id, face) order"""
    return np.lexsort((np.arange(m.nconnface), m.connface[:, 4]))


def partner_face(m):
    pos = {}
    for ic in range(m.nconnface):
        pos.setdefault(int(m.connface[ic, 4]), []).append(ic)
    out = np.zeros(m.nconnface, np.int64)
    for a, b in pos.values():
        out[a], out[b] = b, a
    return out


def device_rows(sp, m, a, width):
    """reference-ordered cell array -> device array [nelem + nconnface][width], ghost rows NaN"""
    torch = _torch()
    d = torch.full((m.nelem + m.nconnface, width), float("nan"), dtype=torch.float64, device="cuda")
    d[:m.nelem] = torch.tensor(np.ascontiguousarray(a[sp.permutation()]).reshape(m.nelem, width), device="cuda")
    torch.cuda.synchronize()
    return d


def from_device(sp, d, n):
    out = np.empty(tuple(d[:n].shape))
    out[sp.permutation()] = d[:n].cpu().numpy()
    return out


# --- 1. ghost update and face traces -----------------------------------------------------------------

@pytest.mark.parametrize("nx,kind", [(8, "tri"), (2, "quad")])
def test_ghost_update_known_answer(workdir, nx, kind):
    torch = _torch()
    c = case(workdir, nx, 8 if nx == 8 else 3, kind)
    m = c.P
    p, _ = c.physics("cyl")
    sp = fa.FlowFV(m, p, cases.numerics("LLF", "NONE", "NONE", order2=False))
    st = sp.layout_stats()
    assert st["ghosts"] == m.nconnface and st["neighbours"] == 1
    order = ghost_order(m)
    for width in (1, 4, 8):
        a = 1000.0 * np.arange(m.nelem)[:, None] + np.arange(width)[None, :]
        d = device_rows(sp, m, a, width)
        sp.ghost_update_device(d.data_ptr(), width)
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        np.testing.assert_array_equal(got[:m.nelem], a[sp.permutation()])            # owned rows untouched
        want = 1000.0 * m.connface[order, 3][:, None] + np.arange(width)[None, :]   # the partner cell's values
        np.testing.assert_array_equal(got[m.nelem:], want)
    partner = partner_face(m)
    for width in (1, 4):
        left = 10.0 * np.arange(m.nconnface)[:, None] + np.arange(width)[None, :]
        dl = torch.tensor(left, device="cuda")
        dr = torch.full((m.nconnface, width), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sp.trace_exchange_device(dl.data_ptr(), dr.data_ptr(), width)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dr.cpu().numpy(), left[partner])
    with pytest.raises(RuntimeError, match="width must be 1..8"):
        sp.ghost_update_device(d.data_ptr(), 9)
    sp.close()


def test_ghost_update_without_ghosts_does_nothing():
    torch = _torch()
    m = fa.UMesh.periodic_box(4, 3)
    p = cases.physics("cyl")
    p.bcconf = [fa.FlowBCConfig("slipwall", 2), fa.FlowBCConfig("slipwall", 3), fa.FlowBCConfig("farfield", 4)]
    sp = fa.FlowFV(m, p, cases.numerics("LLF", "NONE", "NONE", order2=False))
    a = torch.arange(4.0 * m.nelem, dtype=torch.float64, device="cuda").reshape(m.nelem, 4)
    b = a.clone()
    torch.cuda.synchronize()
    sp.ghost_update_device(a.data_ptr(), 4)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    sp.close()


# --- 2. tile equivalence of the residual and the time steps ------------------------------------------

def check_residual(c, kind, flux, grad, rec, order2, device_entry=False):
    torch = _torch()
    p, n, u, r0, dt0 = c.oracle_residual(kind, flux, grad, rec, order2)
    m = c.P
    sp = fa.FlowFV(m, p, n)
    if device_entry:
        du = device_rows(sp, m, u, 4)
        dr = torch.full((m.nelem, 4), float("nan"), dtype=torch.float64, device="cuda")
        dd = torch.full((m.nelem,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sp.compute_residual_device(du.data_ptr(), dr.data_ptr(), dd.data_ptr(), True, True)
        sp.synchronize()
        r, dt = from_device(sp, dr, m.nelem), from_device(sp, dd, m.nelem)
    else:
        r, dt = np.zeros((m.nelem, 4)), np.zeros(m.nelem)
        sp.compute_residual(u, r, True, dt)
    sp.close()
    err = np.abs(r - r0).max(axis=0) / np.abs(r0).max(axis=0)
    edt = np.abs(dt - dt0).max() / np.abs(dt0).max()
    print(f"{kind} {flux} {grad} {rec}: residual {err.max():.2e} time steps {edt:.2e} of the largest")
    assert (err <= 1e-12).all(), err
    assert edt <= 1e-12, edt
    return r


@pytest.mark.parametrize("kind,flux,grad,rec,order2", SCHEMES)
@pytest.mark.parametrize("cells", ["quad", "tri", "hybrid"])
def test_residual_equals_tiling(workdir, cells, kind, flux, grad, rec, order2):
    check_residual(case(workdir, 8, 8, cells), kind, flux, grad, rec, order2, device_entry=(cells == "hybrid"))


def test_residual_two_by_three_box(workdir):
    """two cells across the period: each cell meets its neighbour through an interior face and through the seam"""
    check_residual(case(workdir, 2, 3, "quad"), "naca", "LLF", "NONE", "NONE", False)


def test_residual_channel(workdir):
    """periodic in x between slip walls, against the 3 x 1 tiling"""
    c = case(workdir, 8, 8, "quad", wrap_y=False)
    assert c.P.nbface == 16 and c.P.nconnface == 16
    check_residual(c, "naca", "ROE", "LEASTSQUARES", "VANALBADA", True, device_entry=True)


# --- 3. conservation ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["naca", "viscconst"])
def test_conservation(workdir, kind):
    """every seam face is evaluated from both sides with local normals, so the fluxes cancel to rounding"""
    c = case(workdir, 8, 8, "tri")
    p, _ = c.physics(kind)
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u, _ = c.state(p, seed=9)
    sp = fa.FlowFV(c.P, p, n)
    r = np.zeros((c.P.nelem, 4))
    sp.compute_residual(u, r)
    sp.close()
    total, scale = np.abs(r.sum(axis=0)), np.abs(r).sum(axis=0)
    print(f"{kind}: |sum r| / sum |r| = {total / scale}")
    assert (scale > 0).all() and (total <= 1e-12 * scale).all()


# --- 4. the operator ----------------------------------------------------------------------------------

def device_blocks(sp, m, du, cfl=0.0, ddtm=None):
    torch = _torch()
    N, Fi = m.nelem, m.naface - m.nbface
    dd = torch.zeros((N, 16), dtype=torch.float64, device="cuda")
    dl = torch.zeros((Fi, 16), dtype=torch.float64, device="cuda")
    dup = torch.zeros((Fi, 16), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sp.ghost_update_device(du.data_ptr(), 4)
    sp.assemble_jacobian_device(du.data_ptr(), dd.data_ptr(), dl.data_ptr(), dup.data_ptr())
    if cfl > 0:
        sp.add_pseudo_time_term_device(cfl, ddtm.data_ptr(), dd.data_ptr())
    sp.synchronize()
    return dd, dl, dup


def block_product(sp, m, blocks, x):
    """y = A x on the periodic handle: the ghost rows of x are refreshed first"""
    torch = _torch()
    dx = device_rows(sp, m, x, 4)
    dy = torch.full((m.nelem, 4), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sp.ghost_update_device(dx.data_ptr(), 4)
    sp.block_apply_device(*[b.data_ptr() for b in blocks], dx.data_ptr(), dy.data_ptr())
    sp.synchronize()
    return from_device(sp, dy, m.nelem)


@pytest.mark.parametrize("kind,flux", [("naca", "ROE"), ("naca", "HLLC"), ("viscconst", "ROE"), ("viscconst", "HLLC")])
def test_assembled_operator_equals_tiling(workdir, kind, flux):
    c = case(workdir, 8, 8, "hybrid")
    m, T = c.P, c.T
    p, pt = c.physics(kind)
    n = cases.numerics(flux, "LEASTSQUARES", "VANALBADA")
    u, uT = c.state(p, seed=4)
    x = np.random.default_rng(5).standard_normal((m.nelem, 4))
    xT = np.ascontiguousarray(x[c.local])
    d0, l0, u0 = orc.OracleSpatial(c.oT, pt, n).jacobian(uT)
    L, R = T.intfac[T.nbface:, 0], T.intfac[T.nbface:, 1]
    yT = np.einsum("cij,cj->ci", d0, xT)
    np.add.at(yT, R, np.einsum("fij,fj->fi", l0, xT[L]))
    np.add.at(yT, L, np.einsum("fij,fj->fi", u0, xT[R]))
    assert np.isfinite(yT).all()
    y0 = yT[c.centre]
    sp = fa.FlowFV(m, p, n)
    y = block_product(sp, m, device_blocks(sp, m, device_rows(sp, m, u, 4)), x)
    sp.close()
    err = np.abs(y - y0).max() / np.abs(y0).max()
    print(f"{kind} {flux}: |A x - (A x)_T| = {err:.2e} of the largest")
    assert err <= 1e-12, err


@pytest.mark.parametrize("kind", ["naca", "viscconst"])
def test_matfree_operator_equals_tiling(workdir, kind):
    """tolerance of tests/test_gpu_jacobian.py's matrix-free test (1e-6 of max|y|: the device's |x| is a parallel
    sum). The operator perturbs by eps/|x|; the replicated x on the 3 x 3 tiling has 3 times the norm of x on P
    (9 copies), so the oracle gets 3 eps and both perturb by the same step."""
    torch = _torch()
    c = case(workdir, 8, 8, "quad")
    m = c.P
    p, pt = c.physics(kind)
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u, uT = c.state(p, seed=6)
    ref = orc.OracleSpatial(c.oT, pt, n)
    resT, dtT = np.zeros((c.T.nelem, 4)), np.zeros(c.T.nelem)
    ref.compute_residual(uT, resT, True, dtT)
    mdt = m.area / (5.0 * dtT[c.centre])
    mdtT = np.ascontiguousarray(mdt[c.local])
    x = np.random.default_rng(1).standard_normal((m.nelem, 4))
    eps = 1e-7
    y0 = ref.matfree(uT, resT, mdtT, np.sqrt(c.ntiles) * eps, np.ascontiguousarray(x[c.local]))[c.centre]
    assert np.isfinite(y0).all()
    sp = fa.FlowFV(m, p, n)
    du = device_rows(sp, m, u, 4)
    dr = device_rows(sp, m, resT[c.centre], 4)
    dm = torch.tensor(mdt[sp.permutation()], device="cuda")
    dx = device_rows(sp, m, x, 4)
    dy = torch.full((m.nelem, 4), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sp.matfree_set_eps(eps)
    sp.matfree_set_state_device(du.data_ptr(), dr.data_ptr(), dm.data_ptr())
    sp.matfree_apply_device(dx.data_ptr(), dy.data_ptr())
    sp.synchronize()
    y = from_device(sp, dy, m.nelem)
    # the host-pointer entry of the same operator
    sp.matfree_set_state(u, np.ascontiguousarray(resT[c.centre]), mdt)
    yh = sp.matfree_apply(x)
    sp.close()
    err = np.abs(y - y0).max() / np.abs(y0).max()
    print(f"{kind}: matrix-free |dy| = {err:.2e} of the largest")
    assert err <= 1e-6, err
    assert np.abs(yh - y0).max() <= 1e-6 * np.abs(y0).max()


# --- 5. drivers ---------------------------------------------------------------------------------------

def test_forward_euler_equals_tiling(workdir):
    """four explicit steps: four residuals, each within the 1e-12 bar; the far field's influence travels two
    cells a step from eight cells away, so the centre tile does not see it"""
    torch = _torch()
    c = case(workdir, 8, 8, "quad")
    m = c.P
    p, pt = c.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u, uT = c.state(p, seed=8)
    steps0, _ = orc.OracleSpatial(c.oT, pt, n).forward_euler(uT, 0.5, 0.0, 4)
    assert steps0 == 4 and np.isfinite(uT).all()
    sp = fa.FlowFV(m, p, n)
    du = device_rows(sp, m, u, 4)
    steps, _, hist = sp.steady_forward_euler_device(du.data_ptr(), 0.5, 0.0, 4)
    sp.synchronize()
    got = from_device(sp, du, m.nelem)
    sp.close()
    assert steps == 4 and np.isfinite(hist).all()
    err = np.abs(got - uT[c.centre]).max() / np.abs(uT[c.centre]).max()
    print(f"forward Euler, 4 steps: |du| = {err:.2e} of max|u|")
    assert np.abs(got - u).max() > 1e-6           # the steps moved the state
    assert err <= 1e-11, err


def test_tvdrk_runs_and_conserves(workdir):
    """the unsteady explicit driver on a periodic handle: with one global time step and no boundary, every
    conserved variable's integral stays put to rounding"""
    c = case(workdir, 8, 8, "tri")
    m = c.P
    p, _ = c.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u, _ = c.state(p, seed=2)
    sp = fa.FlowFV(m, p, n)
    du = device_rows(sp, m, u, 4)
    steps, t = sp.tvdrk_device(du.data_ptr(), 2, 0.4, 1.0, 5)
    sp.synchronize()
    got = from_device(sp, du, m.nelem)
    sp.close()
    assert steps == 5 and t > 0 and np.isfinite(got).all()
    before, after = (u * m.area[:, None]).sum(axis=0), (got * m.area[:, None]).sum(axis=0)
    assert np.abs(got - u).max() > 1e-6
    assert (np.abs(after - before) <= 1e-12 * (np.abs(u) * m.area[:, None]).sum(axis=0)).all()


def test_gmres_true_residual(workdir):
    """GMRES on the periodic handle's assembled operator (rtol 1e-8): the true residual, formed with the operator
    checked above, is at most 10 rtol |b| (the factor covers the gap between the Arnoldi recurrence's residual
    and the true one). Measured |b - A x| / |b|: 8.9e-09 after 95 iterations, the recurrence's
    value to three digits."""
    torch = _torch()
    c = case(workdir, 8, 8, "hybrid")
    m = c.P
    p, _ = c.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u, _ = c.state(p, seed=4)
    sp = fa.FlowFV(m, p, n)
    r, dtm = np.zeros((m.nelem, 4)), np.zeros(m.nelem)
    sp.compute_residual(u, r, True, dtm)
    ddtm = torch.tensor(dtm[sp.permutation()], device="cuda")
    blocks = device_blocks(sp, m, device_rows(sp, m, u, 4), cfl=20.0, ddtm=ddtm)
    b = np.random.default_rng(11).standard_normal((m.nelem, 4))
    db = device_rows(sp, m, b, 4)
    dx = torch.zeros((m.nelem + m.nconnface, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rtol = 1e-8
    iters, rn = sp.gmres_blocks_device(*[q.data_ptr() for q in blocks], db.data_ptr(), dx.data_ptr(), rtol, 300, 30, 1)
    sp.synchronize()
    x = from_device(sp, dx, m.nelem)
    true = np.linalg.norm(b - block_product(sp, m, blocks, x)) / np.linalg.norm(b)
    sp.close()
    print(f"GMRES: {iters} iterations, recurrence {rn / np.linalg.norm(b):.2e}, true {true:.2e} of |b|")
    assert 0 < iters < 300
    assert true <= 10 * rtol, true


COUETTE = dict(cflinit=50.0, cflfin=500.0, tol=1e-6, maxiter=30, lin_rtol=1e-2, lin_maxit=30, restart=30)


def couette(prec):
    """tests/visc-couette/implicit.ctrl on periodic_box(8, 16): HLLC, least squares, no limiter, constant
    viscosity, M 0.2193778, Re 4000, Pr 0.708; moving isothermal wall on marker 3 (speed 1), adiabatic wall at
    rest on marker 2, marker 4 periodic along x. 30 backward-Euler steps from the free stream. The wall
    temperature is 1.1 free-stream temperatures, as cases.physics("wall"): abc.cpp:349-366 takes the value in
    non-dimensional units, where the deck's 294 is not a physical state, and with the free-stream temperature
    itself (1.0) the free stream's energy residual is exactly zero on this uniform mesh, so that the driver's
    ratio to the first residual norm (aodesolver.cpp:537) is 0/0 after one step."""
    m = fa.UMesh.periodic_box(8, 16).periodic([(4, 0)])
    p = fa.FlowPhysicsConfig(gamma=1.4, Minf=0.2193778, Tinf=294.0, Reinf=4000.0, Pr=0.708, viscous_sim=True,
                             const_visc=True, bcconf=[fa.FlowBCConfig("isothermalwall", 3, [1.0, 1.1]),
                                                      fa.FlowBCConfig("adiabaticwall", 2, [0.0])])
    n = cases.numerics("HLLC", "LEASTSQUARES", "NONE")
    sp = fa.FlowFV(m, p, n)
    u0 = np.tile(cases.freestream(p), (m.nelem, 1))
    du = device_rows(sp, m, u0, 4)
    cfg = dict(COUETTE)
    cfg.update(prec)
    st, hist = sp.steady_backward_euler_device(du.data_ptr(), fa.ImplicitConfig(**cfg))
    sp.synchronize()
    u = from_device(sp, du, m.nelem)
    ent = sp.entropy_error_device(du.data_ptr())
    funcs, faces = sp.surface_data_device(du.data_ptr(), 3)
    sp.close()
    return m, u, st, ent, funcs, faces


def row_spread(m, u, st, name):
    vx = (u[:, 1] / u[:, 0]).reshape(16, 8)            # rows of the box: cells are numbered row by row
    spread = np.abs(vx - vx.mean(axis=1, keepdims=True)).max()
    y = m.rc[:m.nelem, 1].reshape(16, 8)[:, 0]
    print(f"couette {name}: {st}; row spread {spread:.2e}; max |vx - y| = {np.abs(vx.mean(axis=1) - y).max():.3e}")
    return spread


def test_couette_channel():
    """The discrete operator commutes with the translation along x on this mesh, so only rounding separates the
    cells of a row: every cell agrees with its row's mean to 1e-8 of the wall speed; an error at the seam would be
    1e-2 or more. The linear solver has to keep that symmetry too. Point-block Jacobi does (the other
    preconditioners stop at the seam, below). GMRES does only for short cycles: the seam cells sum their faces
    in another order than the interior cells (connectivity faces come last), so every product leaves last-bit
    differences between the columns, which lie outside the x-uniform Krylov space; the orthogonalisation does
    not see them and every Arnoldi step's normalisation enlarges them by |A M^-1| / h(j+1,j). Hence four Arnoldi
    steps per pseudo-time step here. Measured spread: 1.9e-14, 1.2e-14, 7.0e-14 with 1, 2, 5 Arnoldi steps per
    pseudo-time step; 3.4e-6, 5.0e-6, 4.4e-6, 1.5e-6 with 10, 20, 30, 60 (not asserted)."""
    m, u, st, ent, funcs, faces = couette(dict(lin_maxit=4, restart=4))
    assert np.isfinite(u).all() and np.isfinite(ent) and np.isfinite(funcs).all()
    assert len(faces) == 8
    assert st["steps"] == 30 and st["resratio"] < 1.0, st
    assert row_spread(m, u, st, "jacobi, 4 Arnoldi steps") <= 1e-8


@pytest.mark.parametrize("name,prec", [("jacobi", {}), ("gs", dict(prec_gs=True)), ("ilu", dict(prec_ilu=True)),
                                       ("lines", dict(prec_lines=True)), ("amg", dict(prec_amg=3)),
                                       ("ilu_sweeps", dict(prec_ilu=True, ilu_order=1, ilu_build_sweeps=2,
                                                           ilu_apply_sweeps=2)),
                                       ("matfree", dict(matrix_free=True))])
def test_couette_every_preconditioner(name, prec):
    """backward Euler with every preconditioner on the periodic handle (GMRES(30), the deck's kind of solve).
    They drop the couplings to ghost cells, so lines, ILU, Gauss-Seidel and the aggregates stop at the seam and
    their inexact solves (lin_rtol 1e-2) are not uniform along x; the operator is, so the pseudo-time iteration
    converges to the same rows. The spread stays under the size of a seam error, 1e-2 of the wall speed."""
    m, u, st, ent, funcs, faces = couette(prec)
    assert np.isfinite(u).all() and np.isfinite(ent) and np.isfinite(funcs).all()
    assert st["steps"] > 0 and st["resratio"] < 1.0, st
    assert row_spread(m, u, st, name) <= 1e-2


# --- 6. refusals --------------------------------------------------------------------------------------

def test_periodic_handle_refusals(workdir):
    c = case(workdir, 8, 8, "quad")
    p, _ = c.physics("cyl")
    n = cases.numerics("LLF", "NONE", "NONE", order2=False)
    sp = fa.FlowFV(c.P, p, n)
    with pytest.raises(RuntimeError, match="fvhip_set_rank: a periodic handle"):
        sp.set_rank(0, 1)
    with pytest.raises(RuntimeError, match="fvhip_comm_init: a periodic handle"):
        sp.comm_init(1, 0, bytes(128))
    with pytest.raises(RuntimeError, match="a periodic handle cannot join a group"):
        fa.FlowFVGroup([sp])
    sp.close()
    mixed = fa.UMesh.periodic_box(4, 3, wrap_y=True).periodic([(4, 0), (5, 1)])
    mixed.connface[0, 2] = 1
    keep = np.ascontiguousarray(mixed.connface)
    mixed.view.connface = keep.ctypes.data_as(fa._ffi.c_int_p)
    with pytest.raises(RuntimeError, match="periodic faces on a partitioned mesh are not supported"):
        fa.FlowFV(mixed, p, n)
    # periodicity is a property of the mesh: the boundary-condition type stays refused, with the reference's text
    p.bcconf = [fa.FlowBCConfig("periodic", 4)]
    with pytest.raises(RuntimeError, match="BC type not implemented yet!"):
        fa.FlowFV(c.P, p, n)
