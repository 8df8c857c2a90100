"""The solver stack at its size edges on the device: the block operator, the stand-alone preconditioner entries, GMRES,
one backward-Euler step and the explicit drivers on meshes of one to six cells and on single columns chosen to hit
every path of the line solver, and the explicit drivers' reductions past one pass (294,912 cells > 512 x 256 lanes of
k_min_partial / k_conserved_partial). The cases, their bars and the proof that they can fail are in
tests/solver_edge_cases.py and tests/test_solver_edge_host.py (CPU); nothing here is measured on the device.

Measured on an MI355X, the largest difference over each family's cases against its bar (every test prints its own):
  operator          |y - y_long| 0.57 eps (|A| |x|) per row                       (bar 32, derived)
  line solve        |M z - v| 3.1e-16 of max |v| in fp64 (bar 1e-10), 5.1e-8 with fp32 factors (bars 1e-12 .. 1e-5);
                    z against the dense solve 8.0e-16 of max |z|                   (bar 2e-11; host forms 9.1e-16)
  ILU(0)            |M z - v| 2.9e-16 in colour order, 4.4e-16 by sweeps in orders 1 and 2 (bar 1e-10)
  multigrid         P11, P32, C16: no coarse level, refused by name; C257: 2 coarse levels (86 and 29 rows), the
                    V-cycle 4.2e-16 of max |z| from HostCycle                      (E_ref 2.2e-16, bound 1e-14)
  GMRES             x 7.4e-15 of max |x|                                           (bar 3.2e-11; host forms 7.4e-15)
                    exhausting the space: 1 / 8 / 9 / 15 iterations on P11 / P21 / P13 / P32 with one sweep, 1 / 4 /
                    5 / 8 with two (at most 4N = 4 / 8 / 12 / 24), numpy |b - A x| <= 2.9e-11 |b| (bar 1e-8)
  backward Euler    du, of max |du| per variable: Jacobi 1.4e-14, Gauss-Seidel 1.6e-14, ILU(0) 3.2e-14 (bar 2e-11;
                    host forms 8.9e-15), lines 4.2e-14 (bar 2.1e-10; host forms 5.1e-14); lin_worst against the host
                    estimate 6.5e-9 at most where the residual is not at rounding, and below 2.8e-15 |b| where the
                    preconditioner is exact; hist[0] within 2.3e-16; P11: one iteration, du 3.8e-16 from the dense solve
  explicit drivers  states, times, t and h bitwise the host loops' on one handle and on the three-rank groups; the
                    conserved sums within 2.6e-16 of sum area |u| (bar 1e-12)
  second trip       states and h bitwise; the record's sums 1.9e-16 from np.longdouble's, 7.7e-15 from the host
                    loop's (bar 1e-12); the NaN reaches 4 time steps, at internal indices 294,888 .. 294,911
With one mistake each built into the library (not kept; all of them stay in bounds) the cases that turn red are:
  * k_line_solve_rows' forward remainder one short (full + u < nf - 1): test_line_solve_inverts_line_blocks on
    C16, C18, C20, C22 and C257, fp64 and fp32 -- every column with a half whose length - 1 is no multiple of 4;
    C17 (9 | 9) and the untwisted C2, C15 stay green, as they must;
  * the stride of k_min_partial halved: nothing, and nothing should: every cell is still visited and a minimum does
    not mind a cell twice. The stride doubled (cells skipped) turns test_second_trip_ssprk and
    test_second_trip_tvdrk red (h is no longer the host's); no smaller mesh notices;
  * an early return of the lanes past the last cell in k_bjac_sweep_rows, ahead of its quad exchange: nothing. A
    cell's four lanes leave together, so no live quad loses a partner, on one cell (P11: 4 live lanes of 256) as on
    six. The kernel's clamp-and-compute form is a choice, not a necessity, on this hardware.
The whole file takes 4 s on the device.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import fvens_amd as fa
import _oracle as orc
import cases
import gmres_host as gh
import solver_edge_cases as sec
import ssprk_host as sh
from test_gpu_implicit import _gather, _ilu_host, to_device

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
C_MESHES = [f"C{n}" for n in sec.C_LENGTHS]


def _torch():
    import torch
    return torch


def _nan(rows):
    torch = _torch()
    return torch.full((rows, 4), float("nan"), dtype=torch.float64, device="cuda")


class _Handle:
    """one handle on the whole mesh and, for P13 and P32, the in-process group of its explicit partition"""

    def __init__(self, name):
        self.name = name
        self.m, self.om = sec.mesh(name)
        self.p, self.n = sec.physics(), sec.numerics()
        self.N, self.Fi = self.m.nelem, self.m.naface - self.m.nbface
        self.dev = fa.FlowFV(self.m, self.p, self.n)
        self.perm = self.dev.permutation()
        self.sps = self.grp = None

    def blocks(self, s):
        """device copies of a system's blocks (diagonal in internal order); empty arrays have null pointers"""
        held = [to_device(s.D.reshape(self.N, 16), self.perm), to_device(s.lo.reshape(self.Fi, 16)),
                to_device(s.up.reshape(self.Fi, 16))]
        if self.Fi == 0:
            assert held[1].data_ptr() == 0 and held[2].data_ptr() == 0
        return held

    def back(self, d):
        x = np.empty((self.N, 4))
        x[self.perm] = d.cpu().numpy()
        return x

    def rank(self):
        return sec.rank_of(self.dev.colouring()[0], self.dev.lines(sec.LINE_THRESHOLD), self.perm)

    def group(self):
        """(handles, global cells per rank, group) of sec.PARTS[name], created once"""
        if self.grp is None:
            part = sec.PARTS[self.name]
            self.sps = [fa.FlowFV(self.m, self.p, self.n, partition=part, rank=k) for k in range(int(part.max()) + 1)]
            self.glob = [np.nonzero(part == k)[0][sp.permutation()] for k, sp in enumerate(self.sps)]
            self.grp = fa.FlowFVGroup(self.sps)
        return self.sps, self.glob, self.grp

    def group_states(self, u0):
        """per-rank device states, ghost rows NaN"""
        torch = _torch()
        sps, glob, _ = self.group()
        dus = []
        for sp, g in zip(sps, glob):
            d = _nan(sp.nown + sp.nghost)
            d[:sp.nown] = torch.tensor(u0[g], device="cuda")
            dus.append(d)
        torch.cuda.synchronize()
        return dus

    def close(self):
        if self.grp is not None:
            self.grp.close()
            for sp in self.sps:
                sp.close()
        self.dev.close()


@pytest.fixture(scope="module")
def handles():
    held = {}

    def get(name):
        if name not in held:
            held[name] = _Handle(name)
        return held[name]
    yield get
    for h in held.values():
        h.close()


# ---- 1. the block operator ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sec.P_MESHES))
def test_block_apply_matches_long_double(handles, name):
    """y = A x against the same product in np.longdouble, per row within 32 eps (|A| |x|): a row sums at most five
    blocks of four products, so its error is under gamma_20"""
    H, s = handles(name), sec.fast_system(name)
    held = H.blocks(s)
    dx, dy = to_device(s.x, H.perm), _nan(H.N)
    _torch().cuda.synchronize()
    H.dev.block_apply_device(*[t.data_ptr() for t in held], dx.data_ptr(), dy.data_ptr())
    H.dev.synchronize()
    y = H.back(dy)
    yl, a = sec.long_product(s, s.x)
    err = np.abs(y - yl) / (EPS * a)
    print(f"EDGEDIFF operator {name}: |y - y_long| at most {float(err.max()):.2f} eps (|A| |x|) (bar 32)")
    assert np.all(np.isfinite(y)) and np.all(err <= 32.0)


# ---- 2. the stand-alone preconditioner entries ----------------------------------------------------------------------

@pytest.mark.parametrize("single", [False, True], ids=["double", "single"])
@pytest.mark.parametrize("name", C_MESHES + ["P11", "P13", "P32"])
def test_line_solve_inverts_line_blocks(handles, name, single):
    """test_gpu_implicit's test of that name on single columns (one line alone in its group, every ring remainder of
    k_line_solve_rows, the 256-cell cut) and on the tiny meshes: |M z - v| <= 1e-10 max |v| (fp32 factors: 1e-5 and
    above 1e-12), M assembled from the lines the handle reports; in fp64 also z against the dense solve of M"""
    H, s = handles(name), sec.line_blocks(name)
    lines = H.dev.lines(sec.LINE_THRESHOLD)
    lens = [len(c) for c, _ in lines]
    assert sum(lens) == H.N and np.array_equal(np.sort(np.concatenate([c for c, _ in lines])), np.arange(H.N))
    if name.startswith("C"):
        assert lens == sec.expected_line_lengths(name), lens
    held = H.blocks(s)
    dv, dz = to_device(s.v, H.perm), _nan(H.N)
    _torch().cuda.synchronize()
    H.dev.line_precondition_device(*[t.data_ptr() for t in held], dv.data_ptr(), dz.data_ptr(),
                                   line_threshold=sec.LINE_THRESHOLD, single=single)
    z = H.back(dz).ravel()
    M, v = sec.line_matrix(s, H.perm, lines), s.v.ravel()
    err = np.abs(M @ z - v).max() / np.abs(v).max()
    zd = np.linalg.solve(M, v)
    dense = np.abs(z - zd).max() / np.abs(zd).max()
    print(f"EDGEDIFF lines {name} {'fp32' if single else 'fp64'}: lines {lens[:3]}, |M z - v| {err:.2e} of max |v|, "
          f"z against the dense solve {dense:.2e} of max |z| (bar {sec.BAR['line_dense']:.1e} in fp64)")
    assert np.all(np.isfinite(z))
    assert err <= (1e-5 if single else 1e-10)
    if single:
        assert err > 1e-12
    else:
        assert dense <= sec.BAR["line_dense"]


def _ilu_matrix(H, s):
    """(colour in mesh order, Dt, neighbours) of the colour-order ILU(0) on the host"""
    m = s.m
    L, R = m.intfac[m.nbface:, 0].astype(np.int64), m.intfac[m.nbface:, 1].astype(np.int64)
    col_int, triples = H.dev.colouring()
    colour = np.empty(H.N, np.int64)
    colour[H.perm] = col_int
    assert triples == 0 and np.all(colour[L] != colour[R])
    return (colour,) + _ilu_host(H.N, colour, s.D, L, R, s.lo, s.up)


@pytest.mark.parametrize("name", list(sec.P_MESHES))
def test_ilu_solve_inverts_factors(handles, name):
    """test_gpu_implicit's test of that name on the tiny meshes: |M z - v| <= 1e-10 max |v| with the pivots restated
    by _ilu_host; on P11 z = D^-1 v"""
    H, s = handles(name), sec.line_blocks(name)
    colour, Dt, nbrs = _ilu_matrix(H, s)
    held = H.blocks(s)
    dv, dz = to_device(s.v, H.perm), _nan(H.N)
    _torch().cuda.synchronize()
    H.dev.ilu_precondition_device(*[t.data_ptr() for t in held], dv.data_ptr(), dz.data_ptr())
    z = H.back(dz)
    w = np.einsum("cij,cj->ci", Dt, z)
    for c in range(H.N):
        for k, a_ck, _ in nbrs[c]:
            if colour[k] > colour[c]:
                w[c] += a_ck @ z[k]
    y = np.linalg.solve(Dt, w[..., None])[..., 0]
    Mz = np.einsum("cij,cj->ci", Dt, y)
    for c in range(H.N):
        for k, a_ck, _ in nbrs[c]:
            if colour[k] < colour[c]:
                Mz[c] += a_ck @ y[k]
    err = np.abs(Mz - s.v).max() / np.abs(s.v).max()
    print(f"EDGEDIFF ilu {name}: |M z - v| {err:.2e} of max |v| (bar 1e-10)")
    assert np.all(np.isfinite(z)) and err <= 1e-10
    if name == "P11":
        zd = np.linalg.solve(s.D[0], s.v[0])
        assert np.abs(z[0] - zd).max() <= 1e-13 * np.abs(zd).max()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", list(sec.P_MESHES))
def test_ilu_sweeps_reach_the_sequential_factorisation(handles, name, order):
    """test_gpu_ilu_sweeps' exactness case on the tiny meshes: with depth - 1 build sweeps and depth apply sweeps the
    sweep-based ILU(0) in row order `order` is the sequential one, M = (Dt + L) Dt^-1 (Dt + U) in that order:
    |M z - v| <= 1e-10 max |v| (that file's bar), the pivots restated by _ilu_host with the order's ranks as colours"""
    H, s = handles(name), sec.line_blocks(name)
    m = s.m
    L, R = m.intfac[m.nbface:, 0].astype(np.int64), m.intfac[m.nbface:, 1].astype(np.int64)
    rank_int, depth = H.dev.ilu_order(order)
    rank = np.empty(H.N, np.int64)
    rank[H.perm] = rank_int
    assert depth >= 1 and np.array_equal(np.sort(rank), np.arange(H.N))
    Dt, nbrs = _ilu_host(H.N, rank, s.D, L, R, s.lo, s.up)
    held = H.blocks(s)
    dv, dz = to_device(s.v, H.perm), _nan(H.N)
    _torch().cuda.synchronize()
    H.dev.ilu_sweeps_precondition_device(*[t.data_ptr() for t in held], dv.data_ptr(), dz.data_ptr(), order=order,
                                         build_sweeps=max(depth - 1, 0), apply_sweeps=depth)
    z = H.back(dz)
    w = np.einsum("cij,cj->ci", Dt, z)
    for c in range(H.N):
        for k, a_ck, _ in nbrs[c]:
            if rank[k] > rank[c]:
                w[c] += a_ck @ z[k]
    y = np.linalg.solve(Dt, w[..., None])[..., 0]
    Mz = np.einsum("cij,cj->ci", Dt, y)
    for c in range(H.N):
        for k, a_ck, _ in nbrs[c]:
            if rank[k] < rank[c]:
                Mz[c] += a_ck @ y[k]
    err = np.abs(Mz - s.v).max() / np.abs(s.v).max()
    print(f"EDGEDIFF ilu sweeps {name} order {order}: depth {depth}, |M z - v| {err:.2e} of max |v| (bar 1e-10)")
    assert np.all(np.isfinite(z)) and err <= 1e-10


@pytest.mark.parametrize("name", ["P11", "P32", "C16"])
def test_multigrid_refuses_a_mesh_that_does_not_coarsen(handles, name):
    """a level of fewer than 64 rows is not coarsened (fvhip_ctx::ensureAmg), so these meshes have no coarse level:
    the multigrid refuses them by name before any of its kernels runs, and the handle goes on
    working"""
    H, s = handles(name), sec.step_system(name)
    held = H.blocks(s)
    dv, dz = to_device(s.b, H.perm), _nan(H.N)
    _torch().cuda.synchronize()
    with pytest.raises(RuntimeError, match="prec_amg: the mesh does not coarsen"):
        H.dev.amg_precondition_device(*[t.data_ptr() for t in held], levels=3, d_v=dv.data_ptr(), d_z=dz.data_ptr())
    print(f"EDGEDIFF multigrid {name}: 0 coarse levels, refused by name")
    dx, dy = to_device(s.b, H.perm), _nan(H.N)
    H.dev.block_apply_device(*[t.data_ptr() for t in held], dx.data_ptr(), dy.data_ptr())
    H.dev.synchronize()
    assert np.abs(H.back(dy).ravel() - s.A @ s.b.ravel()).max() <= 1e-13 * np.abs(s.A @ s.b.ravel()).max()


def test_multigrid_cycle_on_the_shortest_column_that_coarsens(handles):
    """C257, the smallest listed mesh with a coarse level: one V-cycle (2 sweeps, 6 on the coarsest, point-block
    finest smoother) against test_gpu_amg_cycle's HostCycle at that file's bar, the restatement's own difference
    from its np.longdouble evaluation"""
    import test_gpu_amg_cycle as cyc
    H, s = handles("C257"), sec.step_system("C257")
    held = H.blocks(s)
    ptrs = [t.data_ptr() for t in held]
    nlev = H.dev.amg_precondition_device(*ptrs, levels=3, threshold=cyc.THRESHOLD)
    assert nlev >= 1
    rank = cyc.Rank(H.dev, H.perm.astype(np.int64), s.D, ptrs, nlev)
    v = np.random.default_rng(17).standard_normal((H.N, 4))
    dv, dz = to_device(v, H.perm), _nan(H.N)
    _torch().cuda.synchronize()
    assert H.dev.amg_precondition_device(*ptrs, levels=3, threshold=cyc.THRESHOLD, sweeps=2, coarse_sweeps=6,
                                         d_v=dv.data_ptr(), d_z=dz.data_ptr()) == nlev
    z = H.back(dz)
    A = cyc.BlockOp.of(s.m, s.D, s.lo, s.up)
    zh = cyc.HostCycle(A, [rank], 0, 0, 2, 6, False).apply(v)
    e_ref = cyc.rel(zh, cyc.HostCycle(A, [rank], 0, 0, 2, 6, False, wide=True).apply(v)) if cyc.HAVE_WIDE else cyc.E_REF["one"]
    bound = cyc.bound_cycle(e_ref)
    print(f"EDGEDIFF multigrid C257: {nlev} coarse levels of {[L.n for L in rank.levels[False]]} rows, device against "
          f"the restatement {cyc.rel(z, zh):.2e} of max |z| (E_ref {e_ref:.2e}, bound {bound:.0e})")
    assert np.all(np.isfinite(z)) and cyc.rel(z, zh) <= bound


# ---- 3. stand-alone GMRES -------------------------------------------------------------------------------------------

def _solve(H, s, rtol, maxit, restart, sweeps, b=None):
    """-> iterations, reported residual norm, x in the mesh's order; d_x holds 7.0 on entry"""
    torch = _torch()
    held = H.blocks(s)
    db = to_device(s.b if b is None else b, H.perm)
    dx = torch.full((H.N, 4), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    it, rn = H.dev.gmres_blocks_device(*[t.data_ptr() for t in held], db.data_ptr(), dx.data_ptr(), rtol, maxit, restart, sweeps)
    return it, rn, H.back(dx)


@pytest.mark.parametrize("name,restart,k,sweeps", sec.STANDALONE_CASES)
def test_standalone_iterate_matches_minimiser(handles, name, restart, k, sweeps):
    """test_gpu_gmres' _check_iterate on the tiny systems, up to the largest k the host test admits"""
    H, s = handles(name), sec.fast_system(name)
    b = s.b.ravel()
    Minv = gh.jacobi_prec(s.A, s.Dinv, sweeps)
    mn = gh.gmres_minimiser(s.A, Minv, b, k, restart)
    rs = gh.gmres_restated(s.A, Minv, b, 0.0, k, restart, 1)
    it, rn, x = _solve(H, s, 0.0, k, restart, sweeps)
    err = gh.distance("fast", x.ravel(), mn.x, mn.x)
    true_rel = mn.rnorm / np.linalg.norm(b)
    est_gap = abs(rs.rnorm / mn.rnorm - 1.0)
    bar_est = gh.EST_BAR if true_rel >= gh.EST_FLAG else gh.BAR_FACTOR * max(gh.EST_GAP, est_gap)
    est = abs(rn / rs.rnorm - 1.0)
    print(f"EDGEDIFF gmres {name} ({restart},{k},{sweeps}): x {err:.2e} = {err / sec.BAR['standalone']:.4f} bar; residual "
          f"norm against host estimate {est:.2e} (bar {bar_est:.1e})")
    assert it == k
    assert np.all(np.isfinite(x)) and err <= sec.BAR["standalone"]
    assert est <= bar_est


@pytest.mark.parametrize("name,sweeps", sec.EXHAUST_CASES)
def test_standalone_exhausts_the_space(handles, name, sweeps):
    """rtol 1e-10, maxit 8N, restart 60: the device stops within 4N iterations (the space has 4N dimensions; the
    breakdown branches decide the last steps), reports a norm within rtol |b|, and numpy's |b - A x| <= 1e-8 |b|"""
    H, s = handles(name), sec.fast_system(name)
    b = s.b.ravel()
    it, rn, x = _solve(H, s, sec.EXHAUST_RTOL, 8 * H.N, sec.EXHAUST_RESTART, sweeps)
    res = np.linalg.norm(b - s.A @ x.ravel()) / np.linalg.norm(b)
    print(f"EDGEDIFF gmres exhaust {name} sweeps {sweeps}: {it} iterations of at most {4 * H.N}, reported "
          f"{rn / np.linalg.norm(b):.2e}, numpy |b - A x| / |b| {res:.2e}")
    assert 1 <= it <= 4 * H.N
    assert np.all(np.isfinite(x)) and np.isfinite(rn)
    assert rn <= sec.EXHAUST_RTOL * np.linalg.norm(b)
    assert res <= 1e-8


def test_standalone_p11_exact_preconditioner(handles):
    """P11 with one sweep: M = A exactly, test_standalone_exact_preconditioner at n = 4: one iteration, x = D^-1 b,
    nothing non-finite"""
    H, s = handles("P11"), sec.fast_system("P11")
    it, rn, x = _solve(H, s, 1e-10, 20, 60, 1)
    x_ref = np.linalg.solve(s.D[0], s.b[0])
    err = gh.distance("fast", x.ravel(), x_ref, x_ref)
    print(f"EDGEDIFF gmres P11 exact: {it} iteration, x {err:.2e} = {err / sec.BAR['standalone']:.4f} bar, norm {rn:.2e}")
    assert it == 1 and np.all(np.isfinite(x)) and np.isfinite(rn)
    assert err <= sec.BAR["standalone"]
    assert rn <= 1e-10 * np.linalg.norm(s.b)


def test_standalone_p11_zero_rhs_and_no_iterations(handles):
    """test_standalone_zero_right_hand_side and test_standalone_no_iterations on P11"""
    H, s = handles("P11"), sec.fast_system("P11")
    it, rn, x = _solve(H, s, 0.0, 5, 60, 1, b=np.zeros_like(s.b))
    assert it == 0 and rn == 0.0 and np.array_equal(x, np.zeros_like(x))
    it, rn, x = _solve(H, s, 0.0, 0, 60, 1)
    assert it == 0 and np.array_equal(x, np.zeros_like(x))
    assert abs(rn / np.linalg.norm(s.b) - 1.0) <= 1e-13


# ---- 4. one backward-Euler step -------------------------------------------------------------------------------------

def _config(kind, sweeps, restart, k, single, rtol=0.0):
    return fa.ImplicitConfig(cgs_refine=0, cflinit=gh.STEP_CFL, cflfin=gh.STEP_CFL, tol=0.0, maxiter=1, lin_rtol=rtol,
                             lin_maxit=k, restart=restart, prec_sweeps=sweeps, min_relax=1.0, prec_gs=kind == "gs",
                             prec_ilu=kind == "ilu", prec_lines=kind == "lines", prec_single=single,
                             line_threshold=sec.LINE_THRESHOLD if kind == "lines" else 0.0)


_prec_hosts = {}


def _prec_host(H, group):
    """gh.PrecHost of the mesh's step system from the structures the handles report"""
    key = (H.name, group)
    if key not in _prec_hosts:
        if group:
            sps, glob, _ = H.group()
            ranks = [sec.rank_of(sp.colouring()[0], sp.lines(sec.LINE_THRESHOLD), g) for sp, g in zip(sps, glob)]
        else:
            ranks = [H.rank()]
        _prec_hosts[key] = gh.PrecHost(sec.step_system(H.name), ranks)
    return _prec_hosts[key]


def _check_step(H, group, kind, sweeps, restart, k, single):
    """test_gpu_precond_iterate's _check_step; where the host's k-th residual is at rounding (an exact preconditioner)
    the reported norm is held to 1e-10 |b| instead of to the host's estimate, which is rounding there too"""
    torch = _torch()
    s = sec.step_system(H.name)
    h = _prec_host(H, group).case(kind, sweeps, restart, k, single)
    u1 = orc.relaxed_update(s.u0, h.minimiser.x.reshape(-1, 4), s.p.gamma, 1.0)
    res0 = np.sqrt(np.sum(s.r[:, 3] * s.r[:, 3] * s.m.area[:s.m.nelem]))
    cfg = _config(kind, sweeps, restart, k, single)
    if group:
        sps, glob, grp = H.group()
        dus = H.group_states(s.u0)
        st, hist = grp.steady_backward_euler_device([d.data_ptr() for d in dus], cfg)
        u = _gather(s.u0, sps, dus, glob)
    else:
        dU = to_device(s.u0, H.perm)
        torch.cuda.synchronize()
        st, hist = H.dev.steady_backward_euler_device(dU.data_ptr(), cfg)
        u = H.back(dU)
    fam = sec.step_family(kind)
    err = np.abs(u - u1).max(axis=0) / np.abs(u1 - s.u0).max(axis=0)
    exact = h.true_rel < 1e-10
    worst = st["lin_worst"] if exact else abs(st["lin_worst"] / (h.restated[0].rnorm / h.bnorm) - 1.0)
    wbar = 1e-10 if exact else gh.est_bar(h)
    print(f"EDGEDIFF step {H.name} {kind} {sweeps} {'fp32' if single else 'fp64'} {'group' if group else 'one'} "
          f"({restart},{k}): du {err.max():.2e} = {err.max() / sec.BAR[fam]:.4f} bar; host forms {h.floor:.2e}; lin_worst "
          f"{'(exact) ' if exact else 'against host estimate '}{worst:.2e} (bar {wbar:.1e}); hist[0] {abs(hist[0] / res0 - 1.0):.2e}")
    assert h.floor <= sec.FLOORS[fam]
    assert st["steps"] == 1 and st["lin_iters"] == k
    assert exact or st["lin_unconverged"] == 1
    assert np.all(np.isfinite(u)) and np.all(err <= sec.BAR[fam]), err / sec.BAR[fam]
    assert worst <= wbar
    assert abs(hist[0] - res0) <= 1e-12 * res0


@pytest.mark.parametrize("name,kind,sweeps,restart,k,single", sec.step_cases())
def test_step_iterate_matches_minimiser(handles, name, kind, sweeps, restart, k, single):
    H = handles(name)
    if kind == "lines":
        lens = [len(c) for c, _ in H.dev.lines(sec.LINE_THRESHOLD)]
        assert sum(lens) == H.N and (lens == [H.N]) == sec.exact(name, "lines"), lens
    _check_step(H, False, kind, sweeps, restart, k, single)


@pytest.mark.parametrize("name,kind,sweeps,restart,k", sec.group_step_cases())
def test_group_step_iterate_matches_minimiser(handles, name, kind, sweeps, restart, k):
    """P13 split three ways (every rank owns one cell and has no face of its own) and P32 split by column, ghost
    rows NaN on entry"""
    H = handles(name)
    sps, glob, _ = H.group()
    assert [sp.nown for sp in sps] == [H.N // 3] * 3
    assert all(sp.nghost >= 1 for sp in sps)
    if name == "P13":        # no face between two owned cells: every line is one cell, one colour
        assert all([len(c) for c, _ in sp.lines(sec.LINE_THRESHOLD)] == [1] and sp.colouring()[0].max() == 0 for sp in sps)
    _check_step(H, True, kind, sweeps, restart, k, False)


@pytest.mark.parametrize("kind,sweeps", gh.PREC_KINDS)
def test_p11_step_is_the_dense_solve(handles, kind, sweeps):
    """one cell: every preconditioner is A^-1, so du = A^-1 b after one iteration (lin_rtol 1e-10, up to 8 allowed)"""
    H, s = handles("P11"), sec.step_system("P11")
    du = np.linalg.solve(s.A.toarray(), s.b.ravel())
    u1 = orc.relaxed_update(s.u0, du.reshape(-1, 4), s.p.gamma, 1.0)
    res0 = np.sqrt(np.sum(s.r[:, 3] * s.r[:, 3] * s.m.area[:1]))
    dU = to_device(s.u0, H.perm)
    _torch().cuda.synchronize()
    st, hist = H.dev.steady_backward_euler_device(dU.data_ptr(), _config(kind, sweeps, 60, 8, False, rtol=1e-10))
    u = H.back(dU)
    err = np.abs(u - u1).max(axis=0) / np.abs(u1 - s.u0).max(axis=0)
    bar = sec.BAR["step"]
    print(f"EDGEDIFF step P11 {kind} {sweeps}: {st['lin_iters']} iteration, du {err.max():.2e} "
          f"(bar {bar:.1e}), hist[0] {abs(hist[0] / res0 - 1.0):.2e}")
    assert st["steps"] == 1 and st["lin_iters"] == 1
    assert np.all(np.isfinite(u)) and np.all(err <= bar)
    assert abs(hist[0] - res0) <= 1e-12 * res0


# ---- 5. the explicit drivers ----------------------------------------------------------------------------------------

def _run_driver(call, driver, order, mode, name):
    """one driver case through `call(method name)(state pointers...)`: (steps, time, record, forward Euler's ratio)"""
    if driver == "fe":
        steps, ratio, hist = call("steady_forward_euler_device", sec.DRIVER_CFL, 0.0, sec.DRIVER_STEPS)
        return steps, None, None, ratio
    if driver == "tvdrk":
        steps, t = call("tvdrk_device", order, sec.DRIVER_CFL, 1e9, sec.DRIVER_STEPS)
        return steps, t, None, None
    kw = dict(cfl=sec.DRIVER_CFL) if mode == "cfl" else dict(dt=sec.fixed_dt(name))
    st, rec = call("ssprk_device", order, 1e9, sec.DRIVER_STEPS, record=True, **kw)
    return st["steps"], st["time"], rec, None


def _one_driver(H, u0, driver, order, mode):
    du = to_device(u0, H.perm)
    _torch().cuda.synchronize()
    out = _run_driver(lambda f, *a, **kw: getattr(H.dev, f)(du.data_ptr(), *a, **kw), driver, order, mode, H.name)
    return (H.back(du),) + out


@pytest.mark.parametrize("driver,order,mode", sec.DRIVER_CASES)
@pytest.mark.parametrize("name", list(sec.P_MESHES))
def test_driver_bitwise_vs_host(handles, name, driver, order, mode):
    """three steps of every explicit driver on the tiny meshes: state, time and the record's t and h bitwise the host
    loops', the conserved sums within test_gpu_ssprk's 1e-12 of sum area |u|"""
    H = handles(name)
    u0, ref = sec.driver_state(name), sec.host_driver(name, driver, order, mode)
    u, steps, t, rec, ratio = _one_driver(H, u0, driver, order, mode)
    assert steps == ref.steps == sec.DRIVER_STEPS
    np.testing.assert_array_equal(u, ref.u)
    assert t == ref.time
    if driver == "fe":
        assert abs(ratio - ref.ratio) <= 1e-12 * abs(ref.ratio)
    if rec is not None:
        np.testing.assert_array_equal(rec[:, :2], ref.rec[:, :2])
        size = (np.abs(ref.u) * H.m.area[:H.N, None]).sum(axis=0)
        d = np.abs(rec[:, 2:] - ref.rec[:, 2:]).max(axis=0) / size
        print(f"EDGEDIFF driver {name} {driver} {order} {mode}: sums {d.max():.2e} of sum area |u| (bar 1e-12)")
        assert np.all(d <= 1e-12)


@pytest.mark.parametrize("driver,order,mode", sec.DRIVER_CASES)
@pytest.mark.parametrize("name", list(sec.PARTS))
def test_driver_group_bitwise_one_handle(handles, name, driver, order, mode):
    """the same runs on the three ranks of P13 (one cell each) and P32 (a column each), ghost rows NaN on entry"""
    H = handles(name)
    u0 = sec.driver_state(name)
    u1, steps1, t1, rec1, ratio1 = _one_driver(H, u0, driver, order, mode)
    sps, glob, grp = H.group()
    dus = H.group_states(u0)
    steps, t, rec, ratio = _run_driver(lambda f, *a, **kw: getattr(grp, f)([d.data_ptr() for d in dus], *a, **kw),
                                       driver, order, mode, name)
    u = _gather(u0, sps, dus, glob)
    assert steps == steps1 == sec.DRIVER_STEPS and t == t1
    np.testing.assert_array_equal(u, u1)
    if driver == "fe":
        assert abs(ratio - ratio1) <= 1e-12 * abs(ratio1)
    if rec is not None:
        np.testing.assert_array_equal(rec[:, :2], rec1[:, :2])
        size = (np.abs(u1) * H.m.area[:H.N, None]).sum(axis=0)
        assert np.all(np.abs(rec[:, 2:] - rec1[:, 2:]) <= 1e-12 * size)


def test_p11_nan_density_diverges_by_name(handles):
    H = handles("P11")
    u0 = sec.driver_state("P11")
    u0[0, 0] = np.nan
    for driver, order, mode in (("fe", 1, "cfl"), ("tvdrk", 2, "cfl"), ("ssprk", 2, "cfl")):
        with pytest.raises(RuntimeError, match=sec.DIVERGED[driver]):
            _one_driver(H, u0, driver, order, mode)


# ---- 6. the second trip of the explicit drivers' reductions ----------------------------------------------------------

@pytest.fixture(scope="module")
def large():
    m = gh.large_mesh()
    assert m.nelem > 2 * sec.SECOND_TRIP_LANES          # every lane takes a second trip, a quarter of them a third
    p, n = cases.physics("naca"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    om = orc.OracleMesh.from_raw(m.raw())
    dev = fa.FlowFV(m, p, n)
    L = SimpleNamespace(m=m, om=om, p=p, n=n, dev=dev, perm=dev.permutation(), N=m.nelem, name="large",
                        u0=cases.state(m, p, 5), area=np.ascontiguousarray(m.area[:m.nelem]))
    L.back = lambda d: _Handle.back(L, d)
    yield L
    dev.close()


def test_second_trip_ssprk(large):
    """SSP-RK order 2, two steps at CFL 0.4 with the record: state and h (hence the minimum time step) bitwise the
    host loop's; the four sums against np.longdouble sums of area u within 1e-12 of sum area |u| (a skipped trip
    loses more than half of a sum)"""
    L = large
    u_ref, st_ref, rec_ref = sh.ssprk(sh.oracle_residual(L.om, L.p, L.n), L.area, L.u0, 2, 1e9, 2, cfl=0.4)
    du = to_device(L.u0, L.perm)
    _torch().cuda.synchronize()
    st, rec = L.dev.ssprk_device(du.data_ptr(), 2, 1e9, 2, cfl=0.4, record=True)
    u = L.back(du)
    assert st["steps"] == 2 and st["time"] == st_ref["time"]
    np.testing.assert_array_equal(rec[:, :2], rec_ref[:, :2])
    np.testing.assert_array_equal(u, u_ref)
    W = np.longdouble
    size = (np.abs(u).astype(W) * L.area[:, None].astype(W)).sum(axis=0)
    last = (u.astype(W) * L.area[:, None].astype(W)).sum(axis=0)
    d_last = np.abs(rec[-1, 2:].astype(W) - last) / size
    d_rows = np.abs(rec[:, 2:] - rec_ref[:, 2:]).max(axis=0) / size.astype(np.float64)
    print(f"EDGEDIFF second trip ssprk: last row against long-double sums {float(d_last.max()):.2e}, rows against the host "
          f"loop's {float(d_rows.max()):.2e} of sum area |u| (bar 1e-12)")
    assert np.all(d_last <= 1e-12) and np.all(d_rows <= 1e-12)


def test_second_trip_tvdrk(large):
    """TVD-RK order 2, two steps at CFL 0.4: state and time (the sum of the steps' cfl dtmin) bitwise the host loop's"""
    from test_gpu_tvdrk import host_tvdrk
    L = large
    u_ref, steps_ref, t_ref = host_tvdrk(L.m, L.om, L.p, L.n, L.u0, 2, 0.4, 1e9, 2)
    du = to_device(L.u0, L.perm)
    _torch().cuda.synchronize()
    steps, t = L.dev.tvdrk_device(du.data_ptr(), 2, 0.4, 1e9, 2)
    assert steps == steps_ref == 2 and t == t_ref
    np.testing.assert_array_equal(L.back(du), u_ref)


def test_second_trip_nan_diverges(large):
    """a NaN density in the cell of largest internal index: every cell whose time step the oracle makes non-finite
    lies at an internal index of at least 131,072, so only lanes on their second trip see it; both drivers raise"""
    L = large
    u0 = L.u0.copy()
    u0[L.perm[-1], 0] = np.nan
    _, dtm = sh.oracle_residual(L.om, L.p, L.n)(u0)
    inv = np.empty(L.N, np.int64)
    inv[L.perm] = np.arange(L.N)
    bad = inv[~np.isfinite(dtm)]
    print(f"EDGEDIFF second trip NaN: {len(bad)} non-finite time steps, internal indices {bad.min()} .. {bad.max()}")
    assert len(bad) >= 1 and bad.min() >= sec.SECOND_TRIP_LANES
    du = to_device(u0, L.perm)
    _torch().cuda.synchronize()
    with pytest.raises(RuntimeError, match=sec.DIVERGED["ssprk"]):
        L.dev.ssprk_device(du.data_ptr(), 2, 1e9, 2, cfl=0.4, record=True)
    du = to_device(u0, L.perm)
    _torch().cuda.synchronize()
    with pytest.raises(RuntimeError, match=sec.DIVERGED["tvdrk"]):
        L.dev.tvdrk_device(du.data_ptr(), 2, 0.4, 1e9, 2)
