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
    m, om = small_mesh()
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u0 = cases.state(m, p, 8)
    r, dtm, D, lo, up = pseudo_time_system(m, om, p, n, u0, STEP_CFL)
    return SimpleNamespace(m=m, p=p, n=n, u0=u0, r=r, D=D, lo=lo, up=up, b=r, A=block_matrix(m, D, lo, up),
                           Dinv=block_diag_inverse(D))


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
