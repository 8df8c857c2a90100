"""The sweep-based block ILU(0)/SGS preconditioner in a row order (fvhip_implicit_config::ilu_order,
ilu_build_sweeps = b, ilu_apply_sweeps = a; blockops.hip k_ilu_sweep_factor, k_ilu_sweep_solve) against
plain-numpy restatements of its formulas, with the order fvhip_ilu_order reports (checked equal to the host shim's,
tests/test_ilu_order_host.py).

For a total order `rank` of a handle's owned cells, owned neighbour k of i is lower if rank[k] < rank[i], upper if
rank[k] > rank[i]; ghost neighbours are skipped.
    build:  Dt^0_i = A_ii,  Dt^{s+1}_i = A_ii - sum_{lower k} A_ik (Dt^s_k)^-1 A_ki  (all i at once),  b sweeps
    apply:  y^1 = Dt^-1 v,  y^{m+1}_i = Dt_i^-1 (v_i - sum_{lower k} A_ik y^m_k),  y = y^a
            z^1 = y,        z^{m+1}_i = y_i - Dt_i^-1 sum_{upper j} A_ij z^m_j,    z = z^a
With b >= depth - 1 the pivots are the sequential factorisation's, with a >= depth the solves are exact.

Blocks are random, as test_ilu_solve_inverts_factors': D = randn + 12 I, lo, up = 0.5 randn, on naca_hybrid(48,8,12,32)
(3,542 cells: not a multiple of 64, so the tail lanes run; 3- and 4-face rows; no triples, so this D-ILU is ILU(0)).

BOUND, for every comparison of a device z with its restatement, as max|z_dev - z_host| / max|z_host|: ten times the
largest difference measured on an MI355X (profiles/ilu_sweeps/restatement_differences.txt: 4.7e-16), rounded up
to a power of ten. The tests assert themselves that they can fail: restatements of neighbouring sweep counts differ
by at least 1e3 BOUND.
"""
import numpy as np
import pytest

import fvens_amd as fa
import cases
from test_gpu_residual import get_mesh
from test_ilu_order_host import host_order, longest_chain, owned_edges

pytestmark = pytest.mark.gpu

BOUND = 1e-14
ORDERS = (1, 2)


def _torch():
    import torch
    return torch


def to_device(a):
    return _torch().tensor(np.ascontiguousarray(a), device="cuda")


def rel(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


class Blocks:
    """random blocks on a handle's layout in its internal order: D [N], lo[fi] = A[R][L], up[fi] = A[L][R] over the
    layout's interior faces (Lc, Rc; ids >= N are ghosts); the directed owned couplings (i, k, A_ik, A_ki)"""

    def __init__(self, N, Lc, Rc, seed):
        rng = np.random.default_rng(seed)
        Fi = len(Lc)
        self.N, self.Fi = N, Fi
        self.D = rng.standard_normal((N, 4, 4)) + 12.0 * np.eye(4)[None]
        self.lo, self.up = 0.5 * rng.standard_normal((Fi, 4, 4)), 0.5 * rng.standard_normal((Fi, 4, 4))
        self.v = rng.standard_normal((N, 4))
        own = (Lc < N) & (Rc < N)
        self.ghost_faces = int((~own).sum())
        L, R = Lc[own].astype(np.int64), Rc[own].astype(np.int64)
        self.i = np.concatenate([R, L])
        self.k = np.concatenate([L, R])
        self.Aik = np.concatenate([self.lo[own], self.up[own]])
        self.Aki = np.concatenate([self.up[own], self.lo[own]])

    def device(self):
        return [to_device(a) for a in (self.D.reshape(-1, 16), self.lo.reshape(-1, 16), self.up.reshape(-1, 16), self.v)]


def host_pivots(B, rank, counts):
    """{b: Dt^b} for the sweep counts asked for"""
    low = rank[B.k] < rank[B.i]
    i, k, Aik, Aki = B.i[low], B.k[low], B.Aik[low], B.Aki[low]
    Dt, out = B.D.copy(), {}
    for s in range(max(counts) + 1):
        if s in counts:
            out[s] = Dt
        Dinv = np.linalg.inv(Dt)
        nxt = B.D.copy()
        np.subtract.at(nxt, i, Aik @ Dinv[k] @ Aki)
        Dt = nxt
    return out


def host_sequential(B, rank):
    """the sequential factorisation in the order: Dt_i = A_ii - sum_{lower k} A_ik Dt_k^-1 A_ki, cell after cell"""
    nbrs = [[] for _ in range(B.N)]
    for e in range(len(B.i)):
        nbrs[B.i[e]].append(e)
    Dt, Dinv = B.D.copy(), np.zeros_like(B.D)
    for c in np.argsort(rank):
        for e in nbrs[c]:
            if rank[B.k[e]] < rank[c]:
                Dt[c] -= B.Aik[e] @ Dinv[B.k[e]] @ B.Aki[e]
        Dinv[c] = np.linalg.inv(Dt[c])
    return Dt


def host_apply(B, rank, Dt, a, v=None):
    v = B.v if v is None else v
    Dinv = np.linalg.inv(Dt)
    low = rank[B.k] < rank[B.i]
    mv = lambda M, x: np.einsum("cij,cj->ci", M, x)

    def coupled(sel, x):
        s = np.zeros_like(x)
        np.add.at(s, B.i[sel], mv(B.Aik[sel], x[B.k[sel]]))
        return s
    y = mv(Dinv, v)
    for _ in range(a - 1):
        y = mv(Dinv, v - coupled(low, y))
    z = y
    for _ in range(a - 1):
        z = y - mv(Dinv, coupled(~low, z))
    return z


def exact_defect(B, rank, Dt, z):
    """max |M z - v| for M = (Dt + L) Dt^-1 (Dt + U)"""
    low = rank[B.k] < rank[B.i]
    mv = lambda M, x: np.einsum("cij,cj->ci", M, x)
    w = mv(Dt, z)
    np.add.at(w, B.i[~low], mv(B.Aik[~low], z[B.k[~low]]))
    y = np.linalg.solve(Dt, w[..., None])[..., 0]
    Mz = mv(Dt, y)
    np.add.at(Mz, B.i[low], mv(B.Aik[low], y[B.k[low]]))
    return float(np.abs(Mz - B.v).max())


class Single:
    """one handle on the hybrid mesh with random blocks, its two orders and the restatements the tests share"""

    def __init__(self):
        self.m = fa.UMesh.naca_hybrid(48, 8, 12, 32, 20.0, 1e-4)
        self.p = cases.physics("naca")
        self.n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
        self.dev = fa.FlowFV(self.m, self.p, self.n)
        self.lay = {o: host_order(self.m, "naca", o) for o in ORDERS}
        lay = self.lay[1]
        self.B = Blocks(lay["ncell"], lay["if_L"], lay["if_R"], 5)
        self.held = self.B.device()
        self.rank, self.depth = {}, {}
        for o in ORDERS:
            r, d = self.dev.ilu_order(o)
            self.rank[o], self.depth[o] = r.astype(np.int64), d
        self._piv, self._seq = {}, {}

    def z(self, order, b, a, single=False):
        torch = _torch()
        dz = torch.full((self.B.N, 4), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        D, lo, up, v = (t.data_ptr() for t in self.held)
        self.dev.ilu_sweeps_precondition_device(D, lo, up, v, dz.data_ptr(), order=order, build_sweeps=b, apply_sweeps=a,
                                                single=single)
        return dz.cpu().numpy()

    def pivots(self, order):
        if order not in self._piv:
            self._piv[order] = host_pivots(self.B, self.rank[order], {0, 1, 2, 3, self.depth[order] - 1})
        return self._piv[order]

    def sequential(self, order):
        if order not in self._seq:
            self._seq[order] = host_sequential(self.B, self.rank[order])
        return self._seq[order]


_single = []


def single_system():
    if not _single:
        _single.append(Single())
    return _single[0]


def test_orders_match_the_host_builder():
    """fvhip_ilu_order's rank and depth equal the host shim's (the same builder on the same layout), the depth equals
    the longest lower chain counted in numpy, the layout's interior faces are the mesh's in the handle's internal
    ids, and the mesh has no three pairwise-adjacent cells"""
    S = single_system()
    m, N = S.m, S.B.N
    assert N == m.nelem == 3542 and N % 64 != 0
    perm = S.dev.permutation()
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    lay = S.lay[1]
    assert np.array_equal(lay["if_L"], inv[m.intfac[m.nbface:, 0]]) and np.array_equal(lay["if_R"], inv[m.intfac[m.nbface:, 1]])
    faces = np.bincount(np.concatenate([S.B.i, S.B.k]), minlength=N) // 2
    assert set(np.unique(faces)) >= {3, 4}
    assert S.dev.colouring()[1] == 0
    Lc, Rc = owned_edges(lay)
    for o in ORDERS:
        assert np.array_equal(S.rank[o], S.lay[o]["rank"]) and S.depth[o] == S.lay[o]["depth"]
        assert S.depth[o] == longest_chain(N, Lc, Rc, S.rank[o])
        print(f"order {o}: depth {S.depth[o]}")
    assert np.array_equal(S.rank[1], np.arange(N)) and not np.array_equal(S.rank[2], np.arange(N))


@pytest.mark.parametrize("order", ORDERS)
def test_pivots_meet_the_restatement(order):
    """a = 1 gives z = (Dt^b)^-1 v: b = 0, 1, 2, depth - 1 against the restatement; b = depth - 1 also against the
    sequential factorisation; restatements of b and b + 1 (b <= 2) differ by at least 1e3 BOUND"""
    S = single_system()
    depth, P = S.depth[order], S.pivots(order)
    host = {b: host_apply(S.B, S.rank[order], P[b], 1) for b in P}
    for b in (0, 1, 2):
        gap = rel(host[b], host[b + 1])
        print(f"SELF pivots order {order} b {b} vs {b + 1}: {gap:.3e}")
        assert gap >= 1e3 * BOUND
    for b in (0, 1, 2, depth - 1):
        e = rel(S.z(order, b, 1), host[b])
        print(f"DIFF pivots order {order} b {b}: {e:.3e}")
        assert e <= BOUND
    seq = host_apply(S.B, S.rank[order], S.sequential(order), 1)
    e = rel(S.z(order, depth - 1, 1), seq)
    print(f"DIFF pivots order {order} b depth-1={depth - 1} vs sequential: {e:.3e}")
    assert e <= BOUND
    assert rel(host[depth - 1], seq) <= BOUND and rel(host[3], seq) >= 1e3 * BOUND   # exact only once b reaches depth - 1


@pytest.mark.parametrize("order", ORDERS)
def test_solve_meets_the_restatement(order):
    """b = depth - 1, a = 1, 2, 3, 4, depth against the restatement; at a = depth the solve is exact: |M z - v| <=
    1e-10 max|v| with M = (Dt + L) Dt^-1 (Dt + U) (test_ilu_solve_inverts_factors' check and bar); restatements of
    a and a + 1 (a <= 4) differ by at least 1e3 BOUND"""
    S = single_system()
    depth, rank = S.depth[order], S.rank[order]
    Dt = S.pivots(order)[depth - 1]
    host = {a: host_apply(S.B, rank, Dt, a) for a in (1, 2, 3, 4, 5, depth)}
    for a in (1, 2, 3, 4):
        gap = rel(host[a], host[a + 1])
        print(f"SELF solve order {order} a {a} vs {a + 1}: {gap:.3e}")
        assert gap >= 1e3 * BOUND
    for a in (1, 2, 3, 4, depth):
        z = S.z(order, depth - 1, a)
        e = rel(z, host[a])
        print(f"DIFF solve order {order} a {a}: {e:.3e}")
        assert e <= BOUND
    defect = exact_defect(S.B, rank, S.sequential(order), z)
    print(f"exact defect order {order} a = depth = {depth}: {defect:.3e} (max|v| {np.abs(S.B.v).max():.3f})")
    assert defect <= 1e-10 * np.abs(S.B.v).max()
    assert exact_defect(S.B, rank, S.sequential(order), host[5]) > 1e-7 * np.abs(S.B.v).max()   # a = 5 is not exact


def test_identities():
    """(b, a) = (0, 1) is point-block Jacobi, z = D^-1 v; two identical calls give bitwise equal z"""
    S = single_system()
    jac = np.linalg.solve(S.B.D, S.B.v[..., None])[..., 0]
    for order in ORDERS:
        e = rel(S.z(order, 0, 1), jac)
        print(f"DIFF identity order {order} (0, 1) vs D^-1 v: {e:.3e}")
        assert e <= BOUND
        z1, z2 = S.z(order, 3, 3), S.z(order, 3, 3)
        assert np.array_equal(z1, z2) and np.all(np.isfinite(z1))
        z1, z2 = S.z(order, 2, 4, single=True), S.z(order, 2, 4, single=True)
        assert np.array_equal(z1, z2) and np.all(np.isfinite(z1))


@pytest.mark.parametrize("order", ORDERS)
def test_single_precision_blocks(order):
    """single = 1: the blocks the sweeps read are fp32 copies (pivots factorised in fp64), vectors and arithmetic
    fp64: the error against the fp64 restatement lies between 1e-12 and 1e-5 of max|z| (the line-solve test's bars)"""
    S = single_system()
    host = host_apply(S.B, S.rank[order], S.pivots(order)[3], 3)
    e = rel(S.z(order, 3, 3, single=True), host)
    print(f"single order {order} (3, 3): {e:.3e}")
    assert 1e-12 < e <= 1e-5
    assert rel(S.z(order, 3, 3), host) <= BOUND


def test_ghost_couplings_are_dropped():
    """on a 3-rank group of naca_ogrid(64,12,8), each handle's z equals the restatement on its owned graph (the
    rank's layout from the host shim, faces to ghost cells left out), for both orders"""
    torch = _torch()
    m = fa.UMesh.naca_ogrid(64, 12, 8, 20.0, 1e-4)
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    part = fa.partition_rcb(m, 3)
    sps = [fa.FlowFV(m, p, n, partition=part, rank=k) for k in range(3)]
    grp = fa.FlowFVGroup(sps)
    for k, spk in enumerate(sps):
        for order in ORDERS:
            lay = host_order(m, "naca", order, 3, k)
            assert (spk.nown, spk.nghost) == (lay["ncell"], lay["nghost"]) and lay["nghost"] > 0
            B = Blocks(lay["ncell"], lay["if_L"], lay["if_R"], 11 + k)
            assert B.ghost_faces > 0
            rank, depth = spk.ilu_order(order)
            assert np.array_equal(rank, lay["rank"]) and depth == lay["depth"]
            rank = rank.astype(np.int64)
            held = B.device()
            for b, a in ((2, 3), (depth - 1, depth)):
                dz = torch.full((B.N, 4), float("nan"), dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                spk.ilu_sweeps_precondition_device(*[t.data_ptr() for t in held[:3]], held[3].data_ptr(), dz.data_ptr(),
                                                   order=order, build_sweeps=b, apply_sweeps=a)
                host = host_apply(B, rank, host_pivots(B, rank, {b})[b], a)
                e = rel(dz.cpu().numpy(), host)
                print(f"DIFF ghosts rank {k} order {order} ({b}, {a}): {e:.3e}")
                assert e <= BOUND
    grp.close()
    for s in sps:
        s.close()


def _step(dev, u0, **kw):
    torch = _torch()
    dU = torch.tensor(np.ascontiguousarray(u0[dev.permutation()]), device="cuda")
    torch.cuda.synchronize()
    cfg = fa.ImplicitConfig(cgs_refine=1, cflinit=100.0, cflfin=100.0, tol=0.0, maxiter=1, lin_rtol=1e-8, lin_maxit=3000,
                            restart=60, prec_sweeps=1, min_relax=1.0, **kw)
    st, _ = dev.steady_backward_euler_device(dU.data_ptr(), cfg)
    return st["lin_iters"], dU.cpu().numpy()


def test_in_the_solver():
    """test_ilu_preconditioner_cuts_iterations' case (wall-resolved O-grid, CFL 100, lin_rtol 1e-8): one step with
    (order, b, a) = (1,3,3), (2,3,3), (1, depth-1, depth) matches the point-block-Jacobi step within 1e-5 of the
    update (that test's bar); the exact-depth run needs fewer iterations than point-block Jacobi. The truncated
    counts and the colour ILU's are printed, not ranked"""
    m = fa.UMesh.naca_ogrid(128, 16, 24, 20.0, 1e-5)
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u0 = cases.state(m, p, 8)
    dev = fa.FlowFV(m, p, n)
    start = u0[dev.permutation()]
    depth = dev.ilu_order(1)[1]
    runs = {"jacobi": {}, "colour ilu": dict(prec_ilu=True),
            "(1,3,3)": dict(prec_ilu=True, ilu_order=1, ilu_build_sweeps=3, ilu_apply_sweeps=3),
            "(2,3,3)": dict(prec_ilu=True, ilu_order=2, ilu_build_sweeps=3, ilu_apply_sweeps=3),
            "exact": dict(prec_ilu=True, ilu_order=1, ilu_build_sweeps=depth - 1, ilu_apply_sweeps=depth)}
    out = {}
    for name, kw in runs.items():
        out[name] = _step(dev, u0, **kw)
    dev.close()
    print("GMRES iterations:", {k: v[0] for k, v in out.items()}, "depth (order 1):", depth)
    uj = out["jacobi"][1]
    scale = np.abs(uj - start).max(axis=0)
    for name in ("(1,3,3)", "(2,3,3)", "exact"):
        d = np.abs(out[name][1] - uj).max(axis=0)
        assert np.all(d <= 1e-5 * scale), (name, d / scale)
    assert out["exact"][0] < out["jacobi"][0]


def test_partitioned_step_same_solution():
    """one step on a 3-rank group (block-Jacobi across ranks: ghost couplings dropped from the preconditioner) with
    tight linear solves equals one handle's to 1e-8 of the update (test_partitioned_ilu_same_solution's bar)"""
    from test_gpu_implicit import _gather, _partitioned
    m, _ = get_mesh("naca_small")
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u0 = cases.state(m, p, 2)
    cfg = fa.ImplicitConfig(cgs_refine=1, cflinit=10.0, cflfin=10.0, tol=0.0, maxiter=1, lin_rtol=1e-11, lin_maxit=400,
                            restart=60, prec_sweeps=1, prec_ilu=True, ilu_order=2, ilu_build_sweeps=3, ilu_apply_sweeps=3)
    one = fa.FlowFV(m, p, n)
    perm = one.permutation()
    dU = to_device(u0[perm])
    _torch().cuda.synchronize()
    st1, _ = one.steady_backward_euler_device(dU.data_ptr(), cfg)
    u1 = np.empty_like(u0)
    u1[perm] = dU.cpu().numpy()
    one.close()
    sps, dus, glob = _partitioned(m, p, n, u0, 3)
    grp = fa.FlowFVGroup(sps)
    st, _ = grp.steady_backward_euler_device([d.data_ptr() for d in dus], cfg)
    u = _gather(u0, sps, dus, glob)
    grp.close()
    for s_ in sps:
        s_.close()
    print(f"lin iters: 1 GPU {st1['lin_iters']}, 3 ranks {st['lin_iters']}")
    scale = np.abs(u1 - u0).max(axis=0)
    assert np.all(np.abs(u - u1).max(axis=0) <= 1e-8 * scale), np.abs(u - u1).max(axis=0) / scale


def test_refusals_name_the_field():
    """every bad combination is refused by field name, through the config and through the stand-alone call; the
    present refusals hold; the handle works afterwards"""
    S = single_system()
    torch = _torch()
    m, _ = get_mesh("naca_small")
    p, n = S.p, S.n
    dev = fa.FlowFV(m, p, n)
    u0 = cases.state(m, p, 2)
    base = dict(cflinit=10.0, cflfin=10.0, tol=0.0, maxiter=1)
    ok = dict(prec_ilu=True, ilu_order=1, ilu_build_sweeps=1, ilu_apply_sweeps=1)
    for kw, field in (({**ok, "ilu_order": 3}, "ilu_order"), ({**ok, "ilu_order": -1}, "ilu_order"),
                      (dict(prec_ilu=True, ilu_build_sweeps=2), "ilu_build_sweeps"),
                      (dict(prec_ilu=True, ilu_apply_sweeps=2), "ilu_apply_sweeps"),
                      ({**ok, "prec_ilu": False}, "prec_ilu"),
                      ({**ok, "ilu_build_sweeps": -1}, "ilu_build_sweeps"),
                      ({**ok, "ilu_apply_sweeps": -1}, "ilu_apply_sweeps"),
                      ({**ok, "ilu_apply_sweeps": 0}, "ilu_apply_sweeps"),
                      ({**ok, "prec_gs": True}, "prec_gs"), ({**ok, "prec_lines": True}, "prec_lines"),
                      ({**ok, "prec_amg": 3}, "prec_amg")):
        dU = to_device(u0[dev.permutation()])
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match=field):
            dev.steady_backward_euler_device(dU.data_ptr(), fa.ImplicitConfig(**base, **kw))
    D, lo, up, v = (t.data_ptr() for t in S.held)
    dz = torch.zeros((S.B.N, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for kw, field in ((dict(order=0), "ilu_order"), (dict(order=3), "ilu_order"),
                      (dict(order=1, build_sweeps=-1), "ilu_build_sweeps"),
                      (dict(order=2, apply_sweeps=0), "ilu_apply_sweeps"),
                      (dict(order=2, apply_sweeps=-2), "ilu_apply_sweeps"),
                      (dict(order=0, build_sweeps=2, apply_sweeps=0), "ilu_build_sweeps")):
        with pytest.raises(RuntimeError, match=field):
            S.dev.ilu_sweeps_precondition_device(D, lo, up, v, dz.data_ptr(), **kw)
    for order in (0, 3):
        with pytest.raises(RuntimeError, match="ilu_order"):
            S.dev.ilu_order(order)
    with pytest.raises(RuntimeError, match="null v"):
        S.dev.ilu_sweeps_precondition_device(D, lo, up, None, dz.data_ptr(), order=1, build_sweeps=0, apply_sweeps=1)
    # both handles are usable afterwards
    jac = np.linalg.solve(S.B.D, S.B.v[..., None])[..., 0]
    assert rel(S.z(1, 0, 1), jac) <= BOUND
    dU = to_device(u0[dev.permutation()])
    torch.cuda.synchronize()
    st, _ = dev.steady_backward_euler_device(dU.data_ptr(), fa.ImplicitConfig(**base, **ok))
    assert st["steps"] == 1 and np.all(np.isfinite(dU.cpu().numpy()))
    dev.close()
