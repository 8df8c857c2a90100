"""The multigrid V-cycle (precond.cpp LinOp::amgApply / cycle; amg.hip k_amg_restrict, k_amg_prolong,
k_amg_residual; blockops.hip's finest block residual) against a host restatement, on one handle and on the ranks of a
group (fvhip_group_amg_precondition_smoother_device), where each rank's hierarchy covers its owned cells and only
the finest residuals couple the ranks.

HostCycle restates the cycle from the code in numpy: the level sweeps are test_gpu_amg_smoother's HostLevel, the
level data the handle's own (amg_level, amg_level_colours), A the host matrix of pseudo_time_system at CFL 20 on
state seed 4, the finest smoother D^-1 (LAPACK) or, with lines, the handle's own line solve as a black box
(test_line_solve_inverts_line_blocks checks that one).

BOUND_CYCLE, relative to max|z|, is not taken from the device: the same restatement is evaluated a second time in
np.longdouble (dinv refined there by one Newton step X (2I - A X)); E_ref is the largest difference of the two
evaluations over the cases of a test, BOUND_CYCLE = 10 E_ref rounded up to a power of ten and at least the smoother
file's BOUND = 1e-14. The factor covers the device's other summation order and its own 4x4 inverse. Where
np.longdouble is no wider than double the recorded E_REF below is used.

Every comparison shows that it can fail: the restatement altered in one place (the coarse levels' post-smoothing
forward instead of backward; the prolongation into the finest level left out; the coarsest level with one sweep
fewer; on ranks, the finest residuals without the ghost coupling) differs from the right one by more than
1e3 BOUND_CYCLE.

Measured on an MI355X (printed by the tests; `dev` is the device's worst difference from the restatement, the
alterations' figure their smallest distance from the right restatement over the cases of the test):
  one handle, naca_small, 3 levels (16 cases)  E_ref 7.13e-16  BOUND_CYCLE 1e-14  dev 7.00e-16
      altered: post 1.5e-03, prolong 2.7e-02, coarse 1.1e-05
  one handle, naca_small, 4 levels             E_ref 6.29e-16  BOUND_CYCLE 1e-14  dev 5.93e-16
      altered: post 1.8e-03, prolong 2.7e-02, coarse 5.6e-08
  one handle, B, 3 levels                      E_ref 1.09e-15  BOUND_CYCLE 1e-13  dev 1.11e-15
      altered: post 2.5e-03, prolong 1.1e-01, coarse 1.8e-05
  one handle, B, 4 levels                      E_ref 1.63e-15  BOUND_CYCLE 1e-13  dev 1.81e-15
      altered: post 2.5e-03, prolong 1.1e-01, coarse 4.4e-08
  ranks, naca_small on 3 (2 cases)             E_ref 4.58e-16  BOUND_CYCLE 1e-14  dev 4.49e-16
      altered: post 6.2e-03, prolong 2.9e-01, coarse 5.5e-05, ghost 1.4e-01
  ranks, A on 8                                E_ref 4.80e-16  BOUND_CYCLE 1e-14  dev 8.15e-16
      altered: post 6.3e-04, prolong 6.3e-01, coarse 3.0e-03, ghost 1.1e-01
  ranks, wall-resolved mesh on 3, lines        E_ref 3.08e-16  BOUND_CYCLE 1e-14  dev 3.63e-16
      altered: post 9.9e-04, prolong 3.7e-02, coarse 2.4e-05, ghost 3.0e-01
(mesh B's first coarse diagonal blocks are the worse conditioned, so 10 E_ref crosses 1e-14 there.) Rank
hierarchies: naca_small on 3 ranks 1,344 cells each, levels [536, 158], [533, 167], [533, 168]; A on 8 ranks
186-265 cells, levels [58], [117, 33], [69, 37], [97, 27], [60], [76, 30], [63], [129, 43].
"""
import numpy as np
import pytest
import scipy.sparse as sp

import fvens_amd as fa
import _oracle as orc
import cases
from test_gpu_residual import get_mesh
from test_gpu_implicit import pseudo_time_system, block_matrix, to_device, _cut_line_links
from test_gpu_amg_smoother import HostLevel, BOUND, MESHES

pytestmark = pytest.mark.gpu

CFL, SEED, THRESHOLD, LINE_THRESHOLD = 20.0, 4, 0.2, 4.0
WIDE = np.longdouble
HAVE_WIDE = np.finfo(np.longdouble).eps < 1e-3 * np.finfo(np.float64).eps
# E_ref where np.longdouble is no wider than double: the largest values measured with an 80-bit long double, above
E_REF = {"one": 1.631e-15, "ranks": 4.799e-16}

MAKERS = {
    "A": MESHES["A"]["mesh"],                                        # naca_ogrid(64, 12, 8, 20, 1e-4), 1,792 cells
    "B": MESHES["B"]["mesh"],                                        # naca_hybrid(48, 8, 12, 32, 20, 1e-4), 3,542 cells
    "wall": lambda: fa.UMesh.naca_ogrid(128, 16, 24, 20.0, 1e-5),    # 8,192 cells
}
NCELLS = {"naca_small": 4032, "A": 1792, "B": 3542, "wall": 8192}


def bound_cycle(e_ref):
    """10 E_ref rounded up to a power of ten, not below the smoother file's BOUND"""
    return max(BOUND, 10.0 ** np.ceil(np.log10(10.0 * e_ref)))


def rel(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


class BlockOp:
    """the host matrix as a list of 4x4 blocks (A[c][c] = D[c], A[R][L] = lower, A[L][R] = upper)"""

    def __init__(self, bi, bj, bv, N):
        self.bi, self.bj, self.bv, self.N = bi, bj, bv, N

    @classmethod
    def of(cls, m, D, lo, up):
        N, nb = m.nelem, m.nbface
        L, R = m.intfac[nb:, 0].astype(np.int64), m.intfac[nb:, 1].astype(np.int64)
        own = np.arange(N)
        return cls(np.concatenate([own, R, L]), np.concatenate([own, L, R]), np.concatenate([D, lo, up]), N)

    def astype(self, T):
        return BlockOp(self.bi, self.bj, self.bv.astype(T), self.N)

    def within(self, part):
        """the blocks whose row and column lie on one rank (no ghost coupling)"""
        k = part[self.bi] == part[self.bj]
        return BlockOp(self.bi[k], self.bj[k], self.bv[k], self.N)

    def apply(self, x):
        y = np.zeros((self.N, 4), self.bv.dtype)
        np.add.at(y, self.bi, np.einsum("kij,kj->ki", self.bv, x[self.bj]))
        return y


def newton(X, A):
    """one Newton step X (2I - A X) towards A^-1, in the precision of A"""
    X = X.astype(A.dtype)
    return np.einsum("kij,kjl->kil", X, 2.0 * np.eye(4, dtype=A.dtype)[None] - np.einsum("kij,kjl->kil", A, X))


class CycleLevel(HostLevel):
    """HostLevel with the level's residual and its aggregates; wide: the blocks in np.longdouble, dinv refined"""

    def __init__(self, L, colour, wide=False):
        super().__init__(L, colour)
        rows = np.repeat(np.arange(L["n"]), np.diff(L["rowptr"]))
        self.diag = L["val"][L["col"] == rows]
        self.agg = L["agg"].astype(np.int64)
        self.wide = wide
        if wide:
            self.vals, self.diag = self.vals.astype(WIDE), self.diag.astype(WIDE)
            self.dinv = newton(self.dinv, self.diag)

    def sweep(self, b, xin, R, fwd):
        if not self.wide:
            return super().sweep(b, xin, R, fwd)
        x = xin.copy()                                   # HostLevel.sweep, the sums in np.longdouble
        inside = (self.rows // R) == (self.cols // R)
        for q in (range(self.ncol) if fwd else range(self.ncol - 1, -1, -1)):
            sel = self.colour[self.rows] == q
            r, c = self.rows[sel], self.cols[sel]
            xv = np.where(inside[sel][:, None], x[c], xin[c])
            acc = np.zeros((self.n, 4), WIDE)
            np.add.at(acc, r, np.einsum("kij,kj->ki", self.vals[sel], xv))
            rq = np.nonzero(self.colour == q)[0]
            x[rq] = np.einsum("kij,kj->ki", self.dinv[rq], b[rq] - acc[rq])
        return x

    def residual(self, b, x):
        y = np.einsum("kij,kj->ki", self.diag, x)
        np.add.at(y, self.rows, np.einsum("kij,kj->ki", self.vals, x[self.cols]))
        return b - y

    def restrict(self, r):
        b = np.zeros((self.n, 4), r.dtype)
        np.add.at(b, self.agg, r)
        return b


class Rank:
    """one handle's share of the cycle: its owned rows (global cells in its internal order), its hierarchy
    restated (after the handle set it up) and its finest smoother"""

    def __init__(self, dev, rows, D, ptrs, nlev):
        self.dev, self.rows, self.ptrs = dev, rows, ptrs
        data = [(dev.amg_level(l), dev.amg_level_colours(l)) for l in range(1, nlev + 1)]
        self.levels = {False: [CycleLevel(L, c) for L, c in data], True: [CycleLevel(L, c, True) for L, c in data]}
        d = D[rows]
        self.dinv = {False: np.linalg.inv(d)}
        self.dinv[True] = newton(self.dinv[False], d.astype(WIDE))

    def s0(self, v, lines, wide):
        if not lines:
            return np.einsum("kij,kj->ki", self.dinv[wide], v)
        import torch
        dv = to_device(np.asarray(v, np.float64))        # the handle's line solve, a black box in double
        dz = torch.zeros_like(dv)
        torch.cuda.synchronize()
        self.dev.line_precondition_device(*self.ptrs, dv.data_ptr(), dz.data_ptr(), line_threshold=LINE_THRESHOLD)
        return dz.cpu().numpy().astype(WIDE if wide else np.float64)


class HostCycle:
    """LinOp::amgApply and LinOp::cycle restated. F finest sweeps (the entry points set F = s), s sweeps per
    coarse level, c on the coarsest; smoother 0 sweeps a whole level (R = its size), smoother 1 blocks of R rows.
    A: the global host matrix (BlockOp); ranks: the handles' shares -- S0 and the coarse cycles run per rank on
    its owned rows, nothing else couples the ranks. alter: None, or one of "post", "prolong", "coarse", "ghost"
    (then part = the cells' ranks)"""

    def __init__(self, A, ranks, smoother, R, s, c, lines, wide=False, alter=None, part=None):
        self.ranks, self.smoother, self.R, self.F, self.s, self.c = ranks, smoother, R, s, s, c
        self.lines, self.wide, self.alter = lines, wide, alter
        self.T = WIDE if wide else np.float64
        self.A = A.astype(self.T)
        if alter == "ghost":
            self.A = self.A.within(part)

    def smooth0(self, v):
        z = np.zeros_like(v)
        for rk in self.ranks:
            z[rk.rows] = rk.s0(v[rk.rows], self.lines, self.wide)
        return z

    def cycle(self, rk, l, b):
        Hs = rk.levels[self.wide]
        H = Hs[l]
        R = H.n if self.smoother == 0 else self.R
        if l + 1 == len(Hs):                              # c sweeps from zero, alternating, forward first
            return H.sweeps(b, None, R, self.c - 1 if self.alter == "coarse" else self.c, 2, True)
        x = H.sweeps(b, None, R, self.s, 0, True)         # s forward sweeps from zero
        x1 = self.cycle(rk, l + 1, Hs[l + 1].restrict(H.residual(b, x)))
        x = x + x1[Hs[l + 1].agg]
        return H.sweeps(b, x, R, self.s, 0 if self.alter == "post" else 1, False)

    def apply(self, v):
        v = v.astype(self.T)
        z = self.smooth0(v)
        for k in range(1, self.F):
            z = z + self.smooth0(v - self.A.apply(z))
        t = v - self.A.apply(z)
        for rk in self.ranks:
            H = rk.levels[self.wide][0]
            x1 = self.cycle(rk, 0, H.restrict(t[rk.rows]))
            if self.alter != "prolong":
                z[rk.rows] += x1[H.agg]
        for k in range(self.F):
            z = z + self.smooth0(v - self.A.apply(z))
        return z


_host, _one, _ranks = {}, {}, {}


def host_system(name):
    """mesh `name` with the host's blocks of one implicit step (CFL 20, state seed 4)"""
    if name in _host:
        return _host[name]
    if name == "naca_small":
        m, om = get_mesh(name)
    else:
        m = MAKERS[name]()
        om = orc.OracleMesh.from_raw(m.raw())
    assert m.nelem == NCELLS[name]
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u = cases.state(m, p, SEED)
    r, dtm, D, lo, up = pseudo_time_system(m, om, p, n, u, CFL)
    _host[name] = dict(m=m, p=p, n=n, u=u, D=D, lo=lo, up=up, N=m.nelem, Fi=m.naface - m.nbface,
                       A=BlockOp.of(m, D, lo, up), v=np.random.default_rng(17).standard_normal((m.nelem, 4)))
    return _host[name]


def one_handle(name, levels):
    """one handle on the whole mesh `name` holding the host's blocks, its hierarchy of `levels` levels set up"""
    if (name, levels) in _one:
        return _one[(name, levels)]
    S = host_system(name)
    dev = fa.FlowFV(S["m"], S["p"], S["n"])
    perm = dev.permutation()
    held = (to_device(S["D"].reshape(-1, 16), perm), to_device(S["lo"].reshape(-1, 16)), to_device(S["up"].reshape(-1, 16)))
    ptrs = [t.data_ptr() for t in held]
    nlev = dev.amg_precondition_device(*ptrs, levels=levels, threshold=THRESHOLD)
    out = dict(dev=dev, perm=perm, held=held, ptrs=ptrs, nlev=nlev, levels=levels, rank=Rank(dev, perm.astype(np.int64), S["D"], ptrs, nlev))
    _one[(name, levels)] = out
    return out


def one_cycle(H, S, s, c, lines, smoother, R):
    """the device's V-cycle of S's v on one handle, in the mesh's cell order"""
    import torch
    dv, dz = to_device(S["v"], H["perm"]), torch.full((S["N"], 4), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    nlev = H["dev"].amg_precondition_smoother_device(*H["ptrs"], levels=H["levels"],
                                                     threshold=THRESHOLD, sweeps=s, coarse_sweeps=c,
                                                     line_threshold=LINE_THRESHOLD if lines else 0.0, d_v=dv.data_ptr(),
                                                     d_z=dz.data_ptr(), smoother=smoother, block_rows=R)
    assert nlev == H["nlev"]
    z = np.empty((S["N"], 4))
    z[H["perm"]] = dz.cpu().numpy()
    return z


def judge(kind, tag, rows, alters, capsys):
    """rows: (label, device z, restatement, restatement in np.longdouble or None, {alteration: altered restatement}).
    Prints E_ref, the device's worst difference and the alterations' smallest distances, then asserts"""
    e_ref = max(rel(zh, zw) for _, _, zh, zw, _ in rows) if HAVE_WIDE else E_REF[kind]
    bound = bound_cycle(e_ref)
    worst = max(rel(zd, zh) for _, zd, zh, _, _ in rows)
    far = {a: min(rel(za[a], zh) for _, _, zh, _, za in rows) for a in alters}
    with capsys.disabled():
        print("\n[amg cycle] %s: %d cases, E_ref = %.3e (long double %s), BOUND_CYCLE = %.0e, dev = %.3e, altered: %s"
              % (tag, len(rows), e_ref, "measured" if HAVE_WIDE else "absent: recorded value", bound, worst,
                 ", ".join("%s %.2e" % kv for kv in far.items())))
    for label, zd, zh, _, za in rows:
        assert np.all(np.isfinite(zd)), label
        assert rel(zd, zh) <= bound, (label, rel(zd, zh), bound)
        for a in alters:
            assert rel(za[a], zh) > 1e3 * bound, (label, a, rel(za[a], zh), bound)
    return bound


@pytest.mark.parametrize("name,levels", [("naca_small", 3), ("naca_small", 4), ("B", 3), ("B", 4)])
def test_one_handle_cycle_meets_the_restatement(name, levels, capsys):
    """one handle: every combination of the coarse smoother (0; 1 with 64-row blocks), 1 / 2 sweeps, 1 / 6 coarsest
    sweeps and the point-block / line finest smoother, 16 cases per mesh and depth, to BOUND_CYCLE of max|z|; the
    three alterations that exist on one handle"""
    S, H = host_system(name), one_handle(name, levels)
    assert H["nlev"] >= 2                                  # a level with pre- and post-smoothing and a coarsest one
    rows = []
    for lines in (False, True):
        for smoother, R in ((0, 0), (1, 64)):
            for s in (1, 2):
                for c in (1, 6):
                    def host(**kw):
                        return HostCycle(S["A"], [H["rank"]], smoother, R, s, c, lines, **kw).apply(S["v"])
                    rows.append(((name, levels, lines, smoother, s, c), one_cycle(H, S, s, c, lines, smoother, R), host(),
                                 host(wide=True) if HAVE_WIDE else None, {a: host(alter=a) for a in ("post", "prolong", "coarse")}))
    judge("one", "one handle, %s, %d levels" % (name, levels), rows, ("post", "prolong", "coarse"), capsys)


PARTITIONS = {
    "naca3": dict(mesh="naca_small", nparts=3, levels=3, lines=False, part=lambda m: fa.partition_rcb(m, 3)),
    "A8": dict(mesh="A", nparts=8, levels=4, lines=False, part=lambda m: fa.partition_graph(m, 8, weights="cost")),
    "wall3": dict(mesh="wall", nparts=3, levels=3, lines=True, part=lambda m: fa.partition_graph(m, 3, weights="cost")),
}


def rank_setup(key):
    """partition `key` as an in-process group: each rank's blocks from the existing calls (the group's residual fills
    the ghost rows of the state and the time steps; each rank then assembles its Jacobian and adds the pseudo-time
    term), the hierarchies set up through the group call"""
    import torch
    if key in _ranks:
        return _ranks[key]
    P = PARTITIONS[key]
    S = host_system(P["mesh"])
    m, nparts = S["m"], P["nparts"]
    part = P["part"](m)
    sps = [fa.FlowFV(m, S["p"], S["n"], partition=part, rank=k) for k in range(nparts)]
    infos = [fa.partition_info(m, part, k) for k in range(nparts)]
    glob, ghost, dus, drs, dts = [], [], [], [], []
    for k, spk in enumerate(sps):
        cg, nown = infos[k]["cell_global"].astype(np.int64), infos[k]["owned"]
        assert (spk.nown, spk.nghost) == (nown, infos[k]["ghosts"]) and np.all(part[cg[:nown]] == k)
        glob.append(cg[:nown][spk.permutation()])
        ghost.append(cg[nown:])
        d = torch.full((spk.nown + spk.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
        d[:spk.nown] = torch.tensor(S["u"][glob[k]], device="cuda")
        dus.append(d)
        drs.append(torch.zeros((spk.nown, 4), dtype=torch.float64, device="cuda"))
        dts.append(torch.zeros(spk.nown, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()  # torch's stream vs the library's (non-blocking) streams
    grp = fa.FlowFVGroup(sps)
    grp.compute_residual_device([d.data_ptr() for d in dus], [d.data_ptr() for d in drs], [d.data_ptr() for d in dts], True)
    held = []
    for k, spk in enumerate(sps):
        st = spk.layout_stats()
        Fi = max(st["faces"] - st["bfaces"], 1)
        blk = [torch.zeros((n, 16), dtype=torch.float64, device="cuda") for n in (spk.nown, Fi, Fi)]
        torch.cuda.synchronize()
        spk.assemble_jacobian_device(dus[k].data_ptr(), *[t.data_ptr() for t in blk])
        spk.add_pseudo_time_term_device(CFL, dts[k].data_ptr(), blk[0].data_ptr())
        spk.synchronize()
        held.append(blk)
    ptrs = [[blk[j].data_ptr() for blk in held] for j in range(3)]       # diag / lower / upper, one pointer per rank
    nlevs = grp.amg_precondition_device(*ptrs, levels=P["levels"], threshold=THRESHOLD)
    ranks = [Rank(spk, glob[k], S["D"], [t.data_ptr() for t in held[k]], nlevs[k]) for k, spk in enumerate(sps)]
    _ranks[key] = dict(S=S, P=P, part=part, sps=sps, grp=grp, glob=glob, ghost=ghost, held=held, ptrs=ptrs, nlevs=nlevs,
                       ranks=ranks, dus=dus)
    return _ranks[key]


@pytest.mark.parametrize("key", ["naca3", "A8"])
def test_rank_hierarchies_are_galerkin_on_the_owned_block(key):
    """each rank's blocks apply as the host matrix does on its owned rows (1e-13 of max|y|; the ghost rows of x
    from partition_info's cell_global); each rank's hierarchy covers its owned cells -- every row in exactly one
    aggregate, each level at least 1.25 times smaller -- and its coarse operators are the Galerkin products of the
    owned x owned block of the host matrix (1e-13 of the largest entry, as test_amg_galerkin_operators_and_cycle;
    level 2 on from the device's level before): the ghost couplings are dropped and nothing else is. On 8 ranks of
    mesh A (186-265 owned cells) the hierarchies have different depths"""
    import torch
    G = rank_setup(key)
    S = G["S"]
    A = block_matrix(S["m"], S["D"], S["lo"], S["up"]).tocsr()
    x = np.random.default_rng(5).standard_normal((S["N"], 4))
    y = (A @ x.ravel()).reshape(-1, 4)
    owned = [spk.nown for spk in G["sps"]]
    print(key, "owned cells", owned, "coarse levels", G["nlevs"],
          "rows", [[H.n for H in rk.levels[False]] for rk in G["ranks"]])
    assert sum(owned) == S["N"]
    if key == "A8":
        assert (min(owned), max(owned)) == (186, 265), owned
        assert len(set(G["nlevs"])) > 1, G["nlevs"]         # S.each over hierarchies of different depth
    for k, spk in enumerate(G["sps"]):
        g = G["glob"][k]
        dx = to_device(np.concatenate([x[g], x[G["ghost"][k]]]))
        dy = torch.full((spk.nown, 4), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        spk.block_apply_device(*[t.data_ptr() for t in G["held"][k]], dx.data_ptr(), dy.data_ptr())
        spk.synchronize()
        assert np.abs(dy.cpu().numpy() - y[g]).max() <= 1e-13 * np.abs(y).max(), (key, k)
        idx = np.ravel(4 * g[:, None] + np.arange(4))
        Af, nf = A[idx][:, idx], spk.nown                  # owned x owned, the rank's internal order
        assert G["nlevs"][k] >= 1
        for lev in range(1, G["nlevs"][k] + 1):
            L = spk.amg_level(lev)
            agg, nc = L["agg"], L["n"]
            assert agg.shape == (nf,) and agg.min() == 0 and agg.max() == nc - 1
            assert len(np.unique(agg)) == nc and nc * 5 <= nf * 4
            Pm = sp.csr_matrix((np.ones(4 * nf), (np.arange(4 * nf), np.ravel(4 * agg[:, None] + np.arange(4)))),
                               shape=(4 * nf, 4 * nc))
            Ac = (Pm.T @ Af @ Pm).toarray()
            rows = np.repeat(np.arange(nc), np.diff(L["rowptr"]))
            Ad = np.zeros((4 * nc, 4 * nc))
            for j in range(len(L["col"])):
                Ad[4 * rows[j]:4 * rows[j] + 4, 4 * L["col"][j]:4 * L["col"][j] + 4] = L["val"][j]
            assert np.abs(Ad - Ac).max() <= 1e-13 * np.abs(Ac).max(), (key, k, lev, np.abs(Ad - Ac).max())
            Af, nf = sp.csr_matrix(Ad), nc


def group_cycle(G, s, c, smoother, R):
    """the group's V-cycle of the mesh's v, in the mesh's cell order; the ghost rows of v and z go in as NaN"""
    import torch
    S, P = G["S"], G["P"]
    dvs, dzs = [], []
    for k, spk in enumerate(G["sps"]):
        dv = torch.full((spk.nown + spk.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
        dv[:spk.nown] = torch.tensor(S["v"][G["glob"][k]], device="cuda")
        dvs.append(dv)
        dzs.append(torch.full_like(dv, float("nan")))
    torch.cuda.synchronize()
    nlevs = G["grp"].amg_precondition_device(*G["ptrs"], levels=P["levels"], threshold=THRESHOLD, sweeps=s, coarse_sweeps=c,
                                             line_threshold=LINE_THRESHOLD if P["lines"] else 0.0,
                                             d_vs=[t.data_ptr() for t in dvs], d_zs=[t.data_ptr() for t in dzs],
                                             smoother=smoother, block_rows=R)
    assert nlevs == G["nlevs"]
    z = np.full((S["N"], 4), np.nan)
    for k, spk in enumerate(G["sps"]):
        z[G["glob"][k]] = dzs[k][:spk.nown].cpu().numpy()
    return z


@pytest.mark.parametrize("key", ["naca3", "A8", "wall3"])
def test_group_cycle_meets_the_restatement(key, capsys):
    """the group's V-cycle (2 sweeps, 6 on the coarsest; smoother 0, and 1 with 64-row blocks) against HostCycle
    across ranks to BOUND_CYCLE: the global matrix in the finest residuals, S0 and the coarse cycles per rank. The
    same bits on a second call; another operator than the one-handle V-cycle (more than 1e3 BOUND_CYCLE apart);
    all four alterations, the finest residuals without the ghost coupling among them. On the wall-resolved mesh the
    finest smoother is the line solve, and lines are cut at the rank boundaries"""
    G = rank_setup(key)
    S, P = G["S"], G["P"]
    s, c = 2, 6
    H = one_handle(P["mesh"], P["levels"])
    if P["lines"]:
        cut, total = _cut_line_links(H["dev"], S["m"], G["part"])
        assert cut > 0, "no line crosses a rank boundary"
    alters = ("post", "prolong", "coarse", "ghost")
    if max(G["nlevs"]) < 2:
        pytest.fail("no rank has a level with post-smoothing")
    rows, ones = [], []
    for smoother, R in ((0, 0), (1, 64)):
        def host(**kw):
            return HostCycle(S["A"], G["ranks"], smoother, R, s, c, P["lines"], part=G["part"], **kw).apply(S["v"])
        zd = group_cycle(G, s, c, smoother, R)
        assert np.array_equal(zd, group_cycle(G, s, c, smoother, R)), (key, smoother)
        rows.append(((key, smoother), zd, host(), host(wide=True) if HAVE_WIDE else None, {a: host(alter=a) for a in alters}))
        ones.append(one_cycle(H, S, s, c, P["lines"], smoother, R))
    bound = judge("ranks", "ranks, %s" % key, rows, alters, capsys)
    for (label, zd, _, _, _), z1 in zip(rows, ones):
        assert rel(zd, z1) > 1e3 * bound, (label, rel(zd, z1))
