"""Host restatements of the device GMRES (fvens_amd/csrc/implicit.cpp gmres()) for tests/test_gmres_host.py
and tests/test_gpu_gmres.py: numpy and scipy only, no device.

With x0 = 0 and right preconditioning the iterate after k Arnoldi steps in cycles of m is unique: every cycle
minimises |r - A M^-1 V y| over its Krylov space, however the basis is orthogonalised. So x_k is computed here
in forms that share only A and M:
  * gmres_restated: the device algorithm as written (classical Gram-Schmidt with cgs_refine 0, 1 or 2,
    Givens rotations, the stopping rules, the restart residual), with its dot products in double or
    (longdot) in np.longdouble;
  * gmres_minimiser: per cycle an orthonormal basis by twice-applied modified Gram-Schmidt, a dense
    least-squares solve for y and r = b - A x from scratch; no Hessenberg matrix, no rotations.
The largest difference between any two of them is a case family's floor; the device is held to 1000 floors
(it sums each dot product over 2048 block partials and a fixed tree, the host forms share numpy's order), and
test_gmres_host.py shows that one more Arnoldi step moves x by at least 1000 such bars.

The floors below are the largest values test_gmres_host.py measures over each family's cases (it prints them
and asserts them against these constants), taken over runs with 1, 3 and 8 BLAS threads (the values move by up
to 2.7 between them: numpy's summation order changes with the thread count) and multiplied by four for another
BLAS. Measured, 8 / 1 / 3 threads: fast 8.0e-15 / 7.7e-15 / 7.7e-15 and slow 5.9e-14 / 8.6e-14 / 7.4e-14 of
max |x|, Jacobian 3.4e-15 / 4.8e-15 / 3.4e-15 of each variable's max |du|, large mesh 4.1e-14 / 1.7e-14 / 4.6e-14
of max |x|. The teeth condition leaves room above them: the smallest step of a case is 2.5e-7 (fast), 2.7e-3
(slow), 1.1e-3 (Jacobian) and 2.3e-2 (large), each at least 1e6 floors.

The other preconditioners (PrecHost below, for tests/test_gpu_precond_iterate.py) run one backward-Euler step's
system with cgs_refine 0, 1 and 2 against the minimiser, with prec_single for both routes to the rounded inverse
(np.linalg.inv and a statement of inv4; they differ in 0 of 64,512 fp32 entries). Largest floor per family, of each
variable's max |du|, 8 / 1 / 3 threads, one domain and the 3-rank form together: Jacobi 3 sweeps 6.7e-15 / 3.0e-15 /
4.6e-15 (fp32 2.5e-15 / 2.9e-15 / 3.2e-15), Gauss-Seidel 4.0e-15 / 2.9e-15 / 3.5e-15 (fp32 2.8e-15 / 3.1e-15 /
3.3e-15), ILU(0) 3.9e-15 / 4.8e-15 / 4.2e-15 (fp32 5.7e-15 / 3.9e-15 / 5.5e-15), lines 5.4e-15 with every count.
All are under FLOOR["jacobian"] = 2e-14, which these families therefore share. Smallest step of a case: Jacobi 2.0e-3,
Gauss-Seidel 1.1e-3, ILU(0) 8.1e-4, lines 7.0e-4 (bar 2e-11); prec_single moves the iterate by at least 1.6e-9
(Jacobi), 1.0e-9 (Gauss-Seidel) and 6.0e-10 (ILU(0)), 30 bars or more; the nearest other operator of
test_prec_forms_are_told_apart is 2.0e-4 away (the line solve on 3 ranks against one domain's), 1e7 bars.
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from test_gpu_implicit import block_matrix, pseudo_time_system

FLOOR = {"fast": 3.2e-14, "slow": 3.5e-13, "jacobian": 2e-14, "large": 1.9e-13}
BAR_FACTOR = 1000.0          # iterate bar = BAR_FACTOR * FLOOR[family], of max |x| (Jacobian system: per variable)
TEETH_FACTOR = 1000.0        # |x_k - x_{k-1}| >= TEETH_FACTOR * bar
EST_GAP = 1e-12              # host: |est_k / |b - A x_k| - 1| for the cases whose estimate is checked
EST_BAR = 1000.0 * EST_GAP   # device residual norm against the host estimate / the true residual (relative)
EST_FLAG = 1e-4              # the estimate is checked where the host's |r_k| / |b| is at least this

# (restart, maxit, sweeps) of the stand-alone solver, rtol 0 (iters == maxit): maxit across the multi-dot's
# groups of 8 (7, 8, 9, 16, 17), restart 1 and 2, cycles cut by maxit (8,20: 8+8+4; 9,20: 9+9+2)
FAST_CASES = [(60, 1, 1), (60, 7, 1), (60, 8, 1), (60, 9, 1), (60, 16, 1), (60, 17, 1), (1, 5, 1), (2, 5, 1),
              (8, 20, 1), (9, 20, 1), (60, 8, 2), (60, 9, 2), (2, 5, 2)]
# one sweep only: with two the Jacobi iteration of this system diverges
SLOW_CASES = [(128, 128, 1), (17, 40, 1), (16, 33, 1), (8, 17, 1)]
LARGE_CASES = [(60, 9, 1), (8, 9, 1)]
# (rtol, restart) of the rtol-stopped runs on the fast system, one sweep
STOP_CASES = [(1e-3, 60), (1e-6, 60), (1e-3, 4), (1e-6, 4)]
STOP_MAXIT = 200
# (restart, lin_maxit) of one backward-Euler step, with prec_sweeps 1 and 2 and cgs_refine 0, 1, 2
STEP_CASES = [(60, 5), (60, 9), (60, 17), (4, 10)]
STEP_CFL = 20.0
LARGE_MESH = (512, 64, 256)   # naca_ogrid: 294,912 cells, 2 ncell = 589,824 > 2048 * 256 double2 lanes
# the other preconditioners, one backward-Euler step each: (kind, prec_sweeps) and (restart, lin_maxit)
PREC_KINDS = [("jacobi", 3), ("gs", 1), ("gs", 2), ("gs", 3), ("ilu", 1), ("ilu", 2), ("lines", 1), ("lines", 2)]
PREC_GROUP_KINDS = [("jacobi", 3), ("gs", 2), ("gs", 3), ("ilu", 2), ("lines", 2)]
PREC_STEP_CASES = [(60, 1), (60, 9), (4, 10)]
PREC_GROUP_STEP_CASES = [(60, 9)]
PREC_RANKS = 3
SINGLE_FACTOR = 10.0          # prec_single moves the host iterate by at least this many bars
LINE_MESH = (48, 21, 8, 20.0, 1e-5)   # naca_ogrid, the shape test_line_solve_inverts_line_blocks twists lines on
LINE_TWIST_MIN = 16

SEED = {"fast": 11, "slow": 12, "large": 13}


def random_blocks(family, N, Fi):
    """fast: D = N(0,1) + 6 I, off-diagonal blocks 0.5 N(0,1) (one step moves x by >= 1e-7 up to k = 17);
    slow: N(0,1) + 4 I and 0.6 N(0,1) (still moving by 1e-2 at k = 128); b = N(0,1)"""
    rng = np.random.default_rng(SEED[family])
    shift, off = (4.0, 0.6) if family == "slow" else (6.0, 0.5)
    D = rng.standard_normal((N, 4, 4)) + shift * np.eye(4)[None]
    lo, up = off * rng.standard_normal((Fi, 4, 4)), off * rng.standard_normal((Fi, 4, 4))
    b = rng.standard_normal((N, 4))
    return D, lo, up, b


def block_diag_inverse(D):
    N = D.shape[0]
    return sp.bsr_matrix((np.linalg.inv(D), np.arange(N), np.arange(N + 1)), shape=(4 * N, 4 * N)).tocsr()


def jacobi_prec(A, Dinv, sweeps):
    """z = M^-1 v as LinOp::precondition applies it: z0 = D^-1 v, then z <- z + D^-1 (v - A z)"""
    def apply(v):
        z = Dinv @ v
        for _ in range(sweeps - 1):
            z = z + Dinv @ (v - A @ z)
        return z
    return apply


# ---- host statements of the other choices of LinOp::precondition (fvens_amd/csrc/precond.cpp) ------------------------
# All of them work on the global system in the mesh's (reference) cell order. A partition is a list of ranks, each a
# namespace of plain arrays as the rank's handle reports them: glob (global cell of every owned cell, in the rank's
# internal order), colour (per owned cell, FlowFV.colouring()) and lines (FlowFV.lines(): list of (cells, faces)).
# One domain is a partition of one rank with glob = FlowFV.permutation().

def round32(a):
    """what LinOp::setup's k_to_single leaves of an fp64 array once blk_row_dot(const float*, ...) widens it again"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def inv4(D):
    """inv4 of blk4.hpp for every 4x4 block of D: Gauss-Jordan on [a | b] from b = I; in column k the rows below k
    are compared with row k in turn and swapped in where |a[i][k]| > |a[k][k]| (the selects), row k is scaled by
    1 / a[k][k] and removed from every other row"""
    a = np.array(D, dtype=np.float64, copy=True)
    b = np.broadcast_to(np.eye(4), a.shape).copy()
    for k in range(4):
        for i in range(k + 1, 4):
            sw = np.abs(a[:, i, k]) > np.abs(a[:, k, k])
            for M in (a, b):
                t = M[sw, k, :].copy()
                M[sw, k, :] = M[sw, i, :]
                M[sw, i, :] = t
        piv = 1.0 / a[:, k, k]
        a[:, k, :] *= piv[:, None]
        b[:, k, :] *= piv[:, None]
        for i in range(4):
            if i != k:
                f = a[:, i, k].copy()
                a[:, i, :] -= f[:, None] * a[:, k, :]
                b[:, i, :] -= f[:, None] * b[:, k, :]
    return b


def single_rounds(kind, sweeps):
    """(dinv, lower and upper): what prec_single rounds to fp32 for one option set -- the block
    if(o.single && (o.amg || !o.lines)) of LinOp::setup without the multigrid: w.dinv (D^-1, or Dt^-1 of the ILU,
    formed in fp64) always, lower and upper if(o.sweeps > 1 || o.gs || o.ilu). With prec_lines nothing is
    converted there (k_line_factor stores fp32 factors itself, which is not restated here)"""
    if kind == "lines":
        return False, False
    return True, sweeps > 1 or kind in ("gs", "ilu")


def block_diag_of(B):
    N = B.shape[0]
    return sp.bsr_matrix((B, np.arange(N), np.arange(N + 1)), shape=(4 * N, 4 * N)).tocsr()


def jacobi_fused_prec(Off, Dinv, sweeps):
    """the same sweeps as k_bjac_sweep forms them: z0 = D^-1 v, then z <- D^-1 (v - Off z) with the off-diagonal
    blocks only. Equal to jacobi_prec up to rounding while D^-1 is D's inverse; with prec_single's rounded D^-1
    only this form is the device's (D itself is not read)"""
    def apply(v):
        z = Dinv @ v
        for _ in range(sweeps - 1):
            z = Dinv @ (v - Off @ z)
        return z
    return apply


class ColourRows:
    """the rows of an off-diagonal matrix colour by colour and rank by rank, for in-place colour sweeps"""

    def __init__(self, Off, ranks):
        self.sets = []
        for r in ranks:
            per = []
            for q in range(int(r.colour.max()) + 1):
                cells = np.asarray(r.glob)[np.asarray(r.colour) == q]
                per.append((cells, Off[(4 * cells[:, None] + np.arange(4)[None]).ravel()]))
            self.sets.append(per)

    def sweep(self, Dinv, rhs, z, order):
        """z_c = Dinv_c (rhs_c - sum_nbr A_ck z_k) in place for the cells of each colour order(nc) names, in turn
        (k_bgs_colour); the ranks share no entry of Off, so their order does not matter"""
        for per in self.sets:
            for q in order(len(per)):
                cells, O = per[q]
                z[cells] = np.einsum("cij,cj->ci", Dinv[cells], rhs[cells] - (O @ z.reshape(-1)).reshape(-1, 4))


def ascending(nc):
    return range(nc)


def descending(nc):
    return range(nc - 1, -1, -1)


def gs_prec(rows, Off_out, Dinv, sweeps, order=(ascending, descending)):
    """LinOp::gaussSeidel: from z = 0, sweep k runs the colours ascending if k is even and descending if odd, every
    cell of the current colour updated in place. rows: the couplings inside a rank; Off_out: those to other ranks'
    cells (None on one domain), which are read from the previous sweep's iterate (S.exchange before every sweep
    but the first, where they are zero)"""
    def apply(v):
        v = v.reshape(-1, 4)
        z = np.zeros_like(v)
        for k in range(sweeps):
            rhs = v - (Off_out @ z.reshape(-1)).reshape(-1, 4) if k and Off_out is not None else v
            rows.sweep(Dinv, rhs, z, order[k % 2])
        return z.reshape(-1).copy()
    return apply


def ilu_prec(rows, A, Dtinv, sweeps, reverse=False):
    """LinOp::iluSweeps: M = (Dt + L) Dt^-1 (Dt + U) in colour order applied as iluApply does -- from z = 0 the
    colours 0 .. nc-1 and then nc-2 .. 0, each a Gauss-Seidel colour update with the pivots' inverses; couplings to
    other ranks are not in rows (ghost rows stay zero) -- then sweeps - 1 corrections z += M^-1 (v - A z) with the
    full A. reverse: the colours taken from the other end (a discrimination form, no device path)"""
    def order(nc):
        q = list(range(nc)) + list(range(nc - 2, -1, -1))
        return [nc - 1 - c for c in q] if reverse else q

    def M(v):
        z = np.zeros((v.size // 4, 4))
        rows.sweep(Dtinv, v.reshape(-1, 4), z, order)
        return z.reshape(-1)

    def apply(v):
        z = M(v)
        for _ in range(sweeps - 1):
            z = z + M(v - A @ z)
        return z
    return apply


def line_prec(A, solve, sweeps):
    """LinOp::lineSweeps: z = M^-1 v with solve the factorised block-tridiagonal line part of A, then sweeps - 1
    corrections z += M^-1 (v - A z) with the full A"""
    def apply(v):
        z = solve(v)
        for _ in range(sweeps - 1):
            z = z + solve(v - A @ z)
        return z
    return apply


class PrecHost:
    """the host statements of M^-1 for one system (step_system() or line_system()) on one partition. Every operand
    is built once. minv(kind, sweeps, single, route, variant): kind jacobi / gs / ilu / lines; single: prec_single
    (the arrays single_rounds names rounded to fp32 and widened, all arithmetic in fp64); route: how the inverse
    that is rounded was formed, numpy (np.linalg.inv) or inv4; variant: a deliberately different operator for the
    discrimination checks -- forward (Gauss-Seidel: every sweep ascending), reversed (ILU: colours from the other
    end), noexchange (Jacobi and Gauss-Seidel: other ranks' cells read as zero in every sweep)"""

    def __init__(self, s, ranks):
        self.s, self.ranks = s, ranks
        m = s.m
        N = m.nelem
        self.L = m.intfac[m.nbface:, 0].astype(np.int64)
        self.R = m.intfac[m.nbface:, 1].astype(np.int64)
        owner = np.full(N, -1)
        for k, r in enumerate(ranks):
            assert np.all(owner[r.glob] == -1)
            owner[r.glob] = k
        assert np.all(owner >= 0)
        self.same = owner[self.L] == owner[self.R]
        self.memo = {}

    def _once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def off(self, which, single):
        """off-diagonal part of A: the couplings inside a rank (in), across ranks (out) or all"""
        def make():
            s = self.s
            lo, up = (round32(s.lo), round32(s.up)) if single else (s.lo, s.up)
            keep = {"in": self.same, "out": ~self.same, "all": np.ones_like(self.same)}[which][:, None, None]
            O = block_matrix(s.m, np.zeros((s.m.nelem, 4, 4)), lo * keep, up * keep)
            O.eliminate_zeros()
            return O
        return self._once(("off", which, single), make)

    def rows(self, single):
        return self._once(("rows", single), lambda: ColourRows(self.off("in", single), self.ranks))

    def pivots(self):
        """Dt of every rank's colour-order ILU(0): couplings to other ranks' cells dropped (k_ilu_factor_colour)"""
        def make():
            from test_gpu_implicit import _ilu_host
            s = self.s
            colour = np.zeros(s.m.nelem, np.int64)
            for r in self.ranks:
                colour[r.glob] = r.colour
            f = self.same
            assert np.all(colour[self.L[f]] != colour[self.R[f]])
            return _ilu_host(s.m.nelem, colour, s.D, self.L[f], self.R[f], s.lo[f], s.up[f])[0]
        return self._once("pivots", make)

    def dinv(self, kind, single, route):
        def make():
            B = self.pivots() if kind == "ilu" else self.s.D
            inv = inv4(B) if route == "inv4" else np.linalg.inv(B)
            return round32(inv) if single else inv
        return self._once(("dinv", kind == "ilu", single, route), make)

    def line_links(self):
        """(previous cell, cell) of every link of every rank's lines, global cells; on one domain the faces are
        checked against the convention of FlowFV.lines(): fi << 1 | (the previous cell is the face's R)"""
        prev, cell = [], []
        for r in self.ranks:
            g = np.asarray(r.glob)
            for cells, faces in r.lines:
                prev.append(g[cells[:-1]])
                cell.append(g[cells[1:]])
                if len(self.ranks) == 1 and len(cells) > 1:
                    fi, side = faces[1:] >> 1, faces[1:] & 1
                    assert faces[0] == -1 and np.all(np.where(side == 1, (self.R[fi] == prev[-1]) & (self.L[fi] == cell[-1]),
                                                              (self.L[fi] == prev[-1]) & (self.R[fi] == cell[-1])))
        return np.concatenate(prev), np.concatenate(cell)

    def line_solve(self):
        """M = the diagonal blocks and the blocks of A that join consecutive cells of a line, factorised once"""
        def make():
            import scipy.sparse.linalg as spla
            N = self.s.m.nelem
            for r in self.ranks:
                assert np.array_equal(np.sort(np.concatenate([c for c, _ in r.lines])), np.arange(len(r.glob)))
            p, c = self.line_links()

            def one(i, j):
                return sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(N, N)).tocsr()
            links = one(np.concatenate([p, c]), np.concatenate([c, p]))
            faces = one(np.concatenate([self.L, self.R]), np.concatenate([self.R, self.L]))
            # every link is one interior face (no link at all where every line is a single cell)
            assert (links.nnz == 0 or links.max() == 1.0) and links.multiply(faces).nnz == links.nnz
            mask = sp.kron(links + sp.identity(N, format="csr"), np.ones((4, 4)), format="csr")
            return spla.splu(self.s.A.multiply(mask).tocsc()).solve
        return self._once("lines", make)

    def minv(self, kind, sweeps, single=False, route="numpy", variant=None):
        s = self.s
        rd, ro = single_rounds(kind, sweeps) if single else (False, False)
        if kind == "lines":
            if single:
                raise ValueError("fp32 line factors are not restated on the host")
            return line_prec(s.A, self.line_solve(), sweeps)
        Dinv = self.dinv(kind, rd, route)
        if kind == "jacobi":
            # across ranks the sweep reads the previous iterate everywhere: the one-domain operator
            if not single and variant is None:
                return jacobi_prec(s.A, block_diag_of(Dinv), sweeps)
            return jacobi_fused_prec(self.off("in" if variant == "noexchange" else "all", ro), block_diag_of(Dinv), sweeps)
        if kind == "gs":
            out = None if variant == "noexchange" or self.same.all() else self.off("out", ro)
            return gs_prec(self.rows(ro), out, Dinv, sweeps, (ascending, ascending if variant == "forward" else descending))
        if kind == "ilu":
            return ilu_prec(self.rows(ro), s.A, Dinv, sweeps, reverse=variant == "reversed")
        raise KeyError(kind)

    def iterate(self, kind, sweeps, restart, k, single=False, route="numpy", variant=None):
        """the minimiser's x_k with one form of M^-1"""
        return self._once(("x", kind, sweeps, restart, k, single, route, variant), lambda: gmres_minimiser(
            self.s.A, self.minv(kind, sweeps, single, route, variant), self.s.b.ravel(), k, restart))

    def case(self, kind, sweeps, restart, k, single=False):
        """every host form of one case, as host_case: the minimiser and the restatement with cgs_refine 0, 1 and 2,
        with prec_single for both routes to the inverse; floor = the largest distance between any two of them"""
        def make():
            s = self.s
            b = s.b.ravel()
            out = SimpleNamespace(bnorm=float(np.linalg.norm(b)))
            xs, every = [], []
            for route in ("numpy", "inv4") if single else ("numpy",):
                Minv = self.minv(kind, sweeps, single, route)
                mn = self.iterate(kind, sweeps, restart, k, single, route)
                rs = {f: gmres_restated(s.A, Minv, b, 0.0, k, restart, f) for f in (0, 1, 2)}
                if route == "numpy":
                    out.minimiser, out.restated = mn, rs
                every += list(rs.values())
                xs += [r.x for r in rs.values()] + [mn.x]
            mn = out.minimiser
            out.x = mn.x
            out.floor = max(distance("jacobian", xs[i], xs[j], mn.x) for i in range(len(xs)) for j in range(i))
            out.step = distance("jacobian", mn.x, mn.xprev, mn.x)
            out.true_rel = mn.rnorm / out.bnorm
            out.est_checked = out.true_rel >= EST_FLAG
            out.est_gap = max(abs(r.rnorm / mn.rnorm - 1.0) for r in every[:3])
            out.iters = [r.iters for r in every]
            return out
        return self._once(("case", kind, sweeps, restart, k, single), make)


def _dots(V, w):
    return V @ w


def _dots_long(V, w):
    wl = w.astype(np.longdouble)
    return np.array([float(np.sum(v.astype(np.longdouble) * wl)) for v in V])


def gmres_restated(A, Minv, b, rtol, maxit, m, refine=0, longdot=False):
    """gmres() of implicit.cpp as written. Returns x, iters, rnorm (what the device reports: the estimate, or
    the restart's true residual when that stopped it), rnorm0, est (the estimate after every step) and tested
    (every value that was compared with rtol |b|, in order)"""
    dots = _dots_long if longdot else _dots

    def norm(v):
        return float(np.sqrt(dots(v[None], v)[0]))
    n = b.size
    x = np.zeros(n)
    beta0 = norm(b)
    out = SimpleNamespace(x=x, iters=0, rnorm=beta0, rnorm0=beta0, est=[], tested=[])
    if not beta0 > 0.0 or maxit <= 0:
        return out
    V = np.zeros((m + 1, n))
    H = np.zeros((m + 1, m))
    cs, sn, y = np.zeros(m), np.zeros(m), np.zeros(m)
    beta, first = beta0, True
    while True:
        if first:
            V[0] = (1.0 / beta) * b
        else:
            w = b - A @ x
            beta = norm(w)
            out.rnorm = beta
            out.tested.append(beta)
            if beta <= rtol * beta0:
                break
            V[0] = (1.0 / beta) * w
        g = np.zeros(m + 1)
        g[0] = beta
        j, done = 0, False
        while j < m and out.iters < maxit:
            w = A @ Minv(V[j])
            Vj = V[:j + 1]
            if refine != 1:
                h = dots(Vj, w)
                H[:j + 1, j] = h
                if refine == 2:
                    w = w - h @ Vj
                    h = dots(Vj, w)
                    H[:j + 1, j] += h
                w = w - h @ Vj
                hn2 = dots(w[None], w)[0]
            else:
                h1, w2 = dots(Vj, w), dots(w[None], w)[0]
                H[:j + 1, j] = h1
                w = w - h1 @ Vj
                hn2 = w2 - float(np.sum(h1 * h1))
                if not hn2 > 0.5 * w2:
                    h2, w2 = dots(Vj, w), dots(w[None], w)[0]
                    H[:j + 1, j] += h2
                    w = w - h2 @ Vj
                    hn2 = w2 - float(np.sum(h2 * h2))
                    if not hn2 > 1e-4 * w2:          # cancellation: measure
                        t = norm(w)
                        hn2 = t * t
            hn = float(np.sqrt(hn2)) if hn2 >= 0.0 else float("nan")
            H[j + 1, j] = hn
            if hn > 0.0:
                V[j + 1] = (1.0 / hn) * w
            for k in range(j):
                t = cs[k] * H[k, j] + sn[k] * H[k + 1, j]
                H[k + 1, j] = -sn[k] * H[k, j] + cs[k] * H[k + 1, j]
                H[k, j] = t
            d = float(np.hypot(H[j, j], H[j + 1, j]))
            cs[j] = H[j, j] / d if d > 0.0 else 1.0
            sn[j] = H[j + 1, j] / d if d > 0.0 else 0.0
            H[j, j], H[j + 1, j] = d, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            j += 1
            out.iters += 1
            out.rnorm = abs(g[j])
            out.est.append(out.rnorm)
            out.tested.append(out.rnorm)
            if not np.isfinite(out.rnorm):
                raise RuntimeError("GMRES: non-finite residual")
            if out.rnorm <= rtol * beta0 or hn == 0.0:
                done = True
                break
        for k in range(j - 1, -1, -1):
            s = g[k]
            for l in range(k + 1, j):
                s -= H[k, l] * y[l]
            y[k] = s / H[k, k]
        x += Minv(y[:j] @ V[:j])
        if done or out.iters >= maxit:
            break
        first = False
    return out


def gmres_minimiser(A, Minv, b, maxit, m):
    """x after maxit steps in cycles of m as the minimiser of |r - A M^-1 Q y| over each cycle's Krylov space.
    Returns x, xprev (the iterate one step earlier) and the true |b - A x|"""
    n = b.size
    x, xprev, k = np.zeros(n), np.zeros(n), 0
    while k < maxit:
        r = b - A @ x if k else b.copy()
        kc = min(m, maxit - k)
        Q, Z, AZ = np.zeros((kc, n)), np.zeros((kc, n)), np.zeros((kc, n))
        q = r
        for j in range(kc):
            for _ in range(2):
                for i in range(j):
                    q = q - (Q[i] @ q) * Q[i]
            Q[j] = q / np.linalg.norm(q)
            Z[j] = Minv(Q[j])
            AZ[j] = A @ Z[j]
            q = AZ[j]
        xprev = x + np.linalg.lstsq(AZ[:kc - 1].T, r, rcond=None)[0] @ Z[:kc - 1] if kc > 1 else x
        x = x + np.linalg.lstsq(AZ.T, r, rcond=None)[0] @ Z
        k += kc
    return SimpleNamespace(x=x, xprev=xprev, rnorm=float(np.linalg.norm(b - A @ x)))


# ---- the systems and the host values of every case, computed once per process ------------------------------------

@functools.lru_cache(maxsize=None)
def small_mesh():
    from test_gpu_residual import get_mesh
    return get_mesh("naca_small")


@functools.lru_cache(maxsize=None)
def large_mesh():
    import fvens_amd as fa
    return fa.UMesh.naca_ogrid(*LARGE_MESH)


@functools.lru_cache(maxsize=None)
def random_system(family):
    """(mesh, D, lo, up, b, A, Dinv) of a random-block family in the mesh's own (reference) cell order"""
    m = large_mesh() if family == "large" else small_mesh()[0]
    D, lo, up, b = random_blocks(family, m.nelem, m.naface - m.nbface)
    return SimpleNamespace(m=m, D=D, lo=lo, up=up, b=b, A=block_matrix(m, D, lo, up), Dinv=block_diag_inverse(D))


@functools.lru_cache(maxsize=None)
def step_system():
    """one backward-Euler step's system on naca_small (Roe, WLS, Van Albada, cases.state(m, p, 8), CFL 20)"""
    import cases
    return _step_system_on(*small_mesh(), cases.physics("naca"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))


def _step_system_on(m, om, p, n):
    """one backward-Euler step's system at CFL STEP_CFL on mesh m (oracle mesh om) with physics p and numerics n,
    from cases.state(m, p, 8)"""
    import cases
    u0 = cases.state(m, p, 8)
    r, dtm, D, lo, up = pseudo_time_system(m, om, p, n, u0, STEP_CFL)
    return SimpleNamespace(m=m, p=p, n=n, u0=u0, r=r, D=D, lo=lo, up=up, b=r, A=block_matrix(m, D, lo, up),
                           Dinv=block_diag_inverse(D))


@functools.lru_cache(maxsize=None)
def line_system():
    """the same step's system on LINE_MESH, whose lines (line_coverage) twist, come in an odd number and a half-full
    twisted group, and include single cells; naca_small's are all six cells long"""
    import fvens_amd as fa
    import _oracle as orc
    import cases
    m = fa.UMesh.naca_ogrid(*LINE_MESH)
    assert m.nelem < 5000
    return _step_system_on(m, orc.OracleMesh.from_raw(m.raw()), cases.physics("naca"),
                           cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))


def line_coverage(lines):
    """(twisted lines, lines of one cell) of a line list; a line of LINE_TWIST_MIN cells or more is solved from both
    ends, 32 such lines to a group (lines.hip k_line_factor / k_line_solve)"""
    lens = np.array([len(c) for c, _ in lines])
    return int((lens >= LINE_TWIST_MIN).sum()), int((lens == 1).sum())


def system_of(family):
    return step_system() if family == "jacobian" else random_system(family)


def scale_of(family, x):
    """what a difference of iterates is measured against: max |x|, per variable for the Jacobian system"""
    x = x.reshape(-1, 4)
    return np.abs(x).max(axis=0) if family == "jacobian" else np.full(4, np.abs(x).max())


def distance(family, xa, xb, ref):
    """largest |xa - xb| relative to scale_of(ref)"""
    return float((np.abs(xa - xb).reshape(-1, 4).max(axis=0) / scale_of(family, ref)).max())


@functools.lru_cache(maxsize=None)
def host_case(family, restart, maxit, sweeps, rtol=0.0, long=True):
    """every host form of one case: restated (by refine: 1 for the stand-alone solver, which runs cgs_refine 1;
    0, 1 and 2 for the steppers' system), its long-double variant (long: the floor needs it, a comparison with
    the device does not), and for rtol 0 the minimiser"""
    s = system_of(family)
    b = s.b.ravel()
    Minv = jacobi_prec(s.A, s.Dinv, sweeps)
    refines = (0, 1, 2) if family == "jacobian" else (1,)
    out = SimpleNamespace(restated={f: gmres_restated(s.A, Minv, b, rtol, maxit, restart, f) for f in refines},
                          bnorm=float(np.linalg.norm(b)))
    out.long = gmres_restated(s.A, Minv, b, rtol, maxit, restart, refines[-1], longdot=True) if long else None
    out.minimiser = gmres_minimiser(s.A, Minv, b, maxit, restart) if rtol == 0.0 else None
    every = list(out.restated.values()) + ([out.long] if long else [])
    forms = [r.x for r in every] + ([out.minimiser.x] if out.minimiser else [])
    ref = forms[-1]
    out.x = ref
    out.floor = max(distance(family, forms[i], forms[j], ref) for i in range(len(forms)) for j in range(i))
    if out.minimiser:
        out.step = distance(family, out.minimiser.x, out.minimiser.xprev, ref)
        out.true_rel = out.minimiser.rnorm / out.bnorm
        out.est_checked = out.true_rel >= EST_FLAG
        out.est_gap = max(abs(r.rnorm / out.minimiser.rnorm - 1.0) for r in every)
    return out


def est_bar(h):
    """relative bar of a device residual norm against the host estimate: 1000 times the host's own gap between
    the estimate and |b - A x_k| (at most EST_GAP where the estimate is checked; it grows as |r_k| / |b| falls)"""
    return EST_BAR if h.est_checked else BAR_FACTOR * max(EST_GAP, h.est_gap)
