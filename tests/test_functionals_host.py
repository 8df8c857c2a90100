"""CPU pin of tests/functionals_host.py (the long-double restatement the device tests compare with) against the
oracle's double-precision orc_surface and orc_entropy, on naca_small, plate_small and 2dcylinderhybrid.msh, for
every marker of each mesh.

Bar: 1e-13 of the value. The oracle adds at most 600 double terms serially, which loses at most (n - 1) 2^-53
<= 6.7e-14 of the sum of the terms' magnitudes, and each term carries a few 2^-53 of its own; the restatement's
long-double terms and fsum lose 2^-53 at most. For the entropy error every term is non-negative, so the error is
relative to the result itself (halved by the square root; up to 4032 terms, measured at most 7.1e-16). The surface sums change sign round a closed body, so the worst
case is a bound relative to sum |c_i| / sum len_i; each case prints the error on that scale (measured: at most
4.7e-15) and the cancellation sum |c_i| / |sum c_i| (at most 108, CL of the wall of naca_small), whose product
stays below 1e-13 of the value on every listed case. Values that are exactly zero (CDsf of the inviscid kinds, CDp
of the plate's horizontal markers, whose n.w is 0.0) are zero on both sides.
"""
import numpy as np
import pytest

import _oracle as orc
import cases
import functionals_host as fh
from test_gpu_residual import get_mesh

BAR = 1e-13

CASES = [("naca_small", "naca", 3), ("naca_small", "visc", 5), ("plate_small", "plate", 7),
         ("2dcylinderhybrid.msh", "cyl", 9)]


def _markers(m):
    return sorted(set(int(t) for t in np.asarray(m.btags).reshape(m.nbface, -1)[:, 0]))


@pytest.mark.parametrize("meshkey,kind,seed", CASES)
def test_surface_restatement_matches_oracle(meshkey, kind, seed):
    m, om = get_mesh(meshkey)
    p = cases.physics(kind, aoa_deg=3.0) if kind == "visc" else cases.physics(kind)
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u = cases.state(m, p, seed)
    ref = orc.OracleSpatial(om, p, n)
    grads = ref.getGradients(u)
    markers = _markers(m)
    assert len(markers) >= 2
    for marker in markers:
        rows, prods = fh.surface_rows(m, p, u, grads, marker)
        assert len(rows) > 0 and len(rows) <= 600
        mine = fh.surface_functionals(prods)
        theirs = ref.surface(u, grads, marker)
        tot = fh.fsum(prods[:, 3])
        for k, name in enumerate(("CL", "CDp", "CDsf")):
            scale = fh.fsum(np.abs(prods[:, k])) / tot
            err = abs(float(theirs[k]) - float(mine[k]))
            cancel = float(scale) / abs(float(mine[k])) if mine[k] != 0 else np.inf
            print("%s %s marker %d %s: %d faces, |oracle - long double| %.3g of sum|c|/len, cancellation %.3g"
                  % (meshkey, kind, marker, name, len(rows), err / float(scale) if scale != 0 else 0.0, cancel))
            assert err <= BAR * abs(float(mine[k])), (marker, name, theirs[k], mine[k])
        if not p.viscous_sim:
            assert mine[2] == 0 and np.all(rows[:, 3] == 0) and theirs[2] == 0.0
        elif kind != "plate" or marker == 2:
            assert np.abs(rows[:, 3]).max() > 0


@pytest.mark.parametrize("meshkey,kind,seed", CASES)
@pytest.mark.parametrize("family", ["smooth", "regime"])
def test_entropy_restatement_matches_oracle(meshkey, kind, seed, family):
    m, om = get_mesh(meshkey)
    p = cases.physics(kind)
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u = cases.state(m, p, seed, amp=0.05) if family == "smooth" else cases.regime_state(m, p, seed)
    terms = fh.entropy_terms(m, p, u)
    assert terms.shape == (m.nelem,) and np.all(terms >= 0) and np.all(np.isfinite(terms))
    mine = float(fh.entropy_error(m, p, u))
    theirs = orc.OracleSpatial(om, p, n).entropy(u)
    assert mine > 0
    print("%s %s %s: %d cells, entropy error %.17g, |oracle - long double| %.3g relative"
          % (meshkey, kind, family, m.nelem, mine, abs(theirs - mine) / mine))
    # worst case the serial double sum of N terms loses (N - 1) 2^-53 of it, halved by the square root (2.2e-13 at
    # 4032 cells); rounding errors do not line up like that, and the measured distance is at most 7.1e-16
    assert abs(theirs - mine) <= BAR * mine, (theirs, mine)


def test_entropy_of_the_free_stream_is_zero():
    m, _ = get_mesh("naca_small")
    p = cases.physics("cyl")
    u = np.tile(cases.freestream(p), (m.nelem, 1))
    t = fh.entropy_terms(m, p, u)
    # long double s of the double free stream against the long-double s_inf: the rounding of the stored energy
    # p_inf/(g - 1) + 1/2 alone, 2^-53 of 13 magnified by g - 1 over p_inf
    assert float(np.sqrt(fh.fsum(t))) <= 8 * 2.0 ** -53 * np.sqrt(m.area.sum())


def test_mistakes_move_cf():
    """the mistakes the device test guards against change the restatement's Cf on a viscous case. A cell's gradient
    block read transposed ([2 dims][4 vars] for [4 vars][2 dims]) is the restatement on the re-read blocks. The
    tangent negated gives -Cf exactly (Cf is linear in t), so it shows wherever max|Cf| > 0."""
    m, om = get_mesh("naca_small")
    p = cases.physics("visc", aoa_deg=3.0)
    u = cases.state(m, p, 5)
    grads = orc.OracleSpatial(om, p, cases.numerics()).getGradients(u)
    cf = fh.surface_rows(m, p, u, grads, 2)[0][:, 3]
    tol = 1e-12 * float(np.abs(cf).max())
    reread = np.ascontiguousarray(grads.reshape(-1, 2, 4).transpose(0, 2, 1))
    assert float(np.abs(fh.surface_rows(m, p, u, reread, 2)[0][:, 3] - cf).max()) > tol
    assert float(np.abs(-cf - cf).max()) > tol
