"""The entropy error on the device (FlowOutput::compute_entropy_cell, aoutput.cpp:28-62; k_entropy_partial and
k_entropy_sum of surface.hip, on the shared block_sum) against the long-double restatement
tests/functionals_host.py, on cell counts chosen round the kernel's block of 256: under one wave, one short of a
block, a block, one over, and round two blocks.

Bar: 1e-12 of sqrt(fsum(terms)), the project's bar for pow paths (s = p / rho^gamma is the device pow). The terms are
non-negative, so the block tree and the serial sum of the block sums lose at most (8 + nblocks) 2^-53 of the sum;
what is left of the bar is for pow. The sum is deterministic: a second call returns the same bits. A state equal to
the free stream in every cell gives exactly 0.0 (s and s_inf are then the same operations on the same numbers; the
free stream is built with the C library's cos and sin, which the host side of the library calls).
The in-process group adds the ranks' sums in rank order on the host: the same terms in another order, so its square
is within 4 nranks 2^-53 of the one handle's.
"""
import functools
import math

import numpy as np
import pytest

import fvens_amd as fa
import cases
import functionals_host as fh
from test_gpu_residual import get_mesh

pytestmark = pytest.mark.gpu

BLOCK = 256                 # cells per block of k_entropy_partial
# cell count -> generator; every count is the product the generator makes
MESHES = {
    63: lambda: fa.UMesh.periodic_box(7, 9),
    255: lambda: fa.UMesh.periodic_box(15, 17),
    256: lambda: fa.UMesh.cylinder_ogrid(16, 8),            # two triangles per (theta, r) cell
    257: lambda: fa.UMesh.flat_plate(1, 257),
    511: lambda: fa.UMesh.flat_plate(7, 73),
    512: lambda: fa.UMesh.cylinder_ogrid(16, 16),
    513: lambda: fa.UMesh.periodic_box(3, 171, jitter=0.2),
}
COUNTS = sorted(MESHES)


@functools.lru_cache(maxsize=None)
def _mesh(ncell):
    m = MESHES[ncell]()
    assert m.nelem == ncell
    return m


def _physics(aoa_deg=0.0):
    """markers 2, 3, 4, 5 all have a boundary condition (the box, the plate and the cylinder use subsets)"""
    p = cases.physics("plate_inviscid", Minf=0.6)
    p.aoa = math.radians(aoa_deg)
    return p


def _state(m, p, family, seed):
    return cases.state(m, p, seed, amp=0.05) if family == "smooth" else cases.regime_state(m, p, seed)


def _device(m, p, u, calls=1):
    import torch
    dev = fa.FlowFV(m, p, cases.numerics())
    du = torch.tensor(np.ascontiguousarray(u[dev.permutation()]), device="cuda")
    torch.cuda.synchronize()
    out = [dev.entropy_error_device(du.data_ptr()) for _ in range(calls)]
    dev.close()
    return out


def test_cell_counts_straddle_the_block():
    assert min(COUNTS) < 64
    for edge in (BLOCK, 2 * BLOCK):
        assert edge - 1 in COUNTS and edge in COUNTS and edge + 1 in COUNTS


@pytest.mark.parametrize("family", ["smooth", "regime"])
@pytest.mark.parametrize("ncell", COUNTS, ids=["cells%d" % k for k in COUNTS])
def test_entropy_error_matches_restatement(ncell, family):
    m = _mesh(ncell)
    p = _physics(aoa_deg=2.0)
    u = _state(m, p, family, 30 + ncell)
    want = float(fh.entropy_error(m, p, u))
    first, second = _device(m, p, u, calls=2)
    print("entropy %d cells %s: %.17g, device - long double %.3g relative" % (ncell, family, want, abs(first - want) / want))
    assert want > 0 and np.isfinite(first)
    assert abs(first - want) <= 1e-12 * want, (first, want)
    assert first == second                      # deterministic: same bits on the same handle and state


@pytest.mark.parametrize("aoa_deg", [0.0, 1.25], ids=["aoa0", "aoa1.25"])
@pytest.mark.parametrize("ncell", [63, 257, 513], ids=["cells63", "cells257", "cells513"])
def test_entropy_error_of_the_free_stream_is_zero(ncell, aoa_deg):
    m = _mesh(ncell)
    p = _physics(aoa_deg)
    pinf = 1.0 / (p.gamma * p.Minf * p.Minf)
    # compute_freestream_state (aphysics.cpp:43-58) with the C library's cos and sin, as the library's host side
    uinf = np.array([1.0, math.cos(p.aoa) * math.cos(0.0), math.sin(p.aoa) * math.cos(0.0),
                     pinf / (p.gamma - 1.0) + 0.5 * 1.0 * 1.0])
    got, = _device(m, p, np.tile(uinf, (ncell, 1)))
    assert got == 0.0


def test_group_entropy_error():
    """3 ranks of naca_small (graph partition), ghost rows NaN: the group's error against the restatement and
    against the one handle's"""
    import torch
    m, _ = get_mesh("naca_small")
    p, n = cases.physics("visc", aoa_deg=3.0), cases.numerics()
    nranks = 3
    part = fa.partition_graph(m, nranks, weights="cost")
    for family in ("smooth", "regime"):
        u = _state(m, p, family, 21)
        want = float(fh.entropy_error(m, p, u))
        one, = _device(m, p, u)
        sps = [fa.FlowFV(m, p, n, partition=part, rank=k) for k in range(nranks)]
        dus = []
        for k, sp in enumerate(sps):
            g = np.nonzero(part == k)[0][sp.permutation()]
            d = torch.full((sp.nown + sp.nghost, 4), float("nan"), dtype=torch.float64, device="cuda")
            d[:sp.nown] = torch.tensor(u[g], device="cuda")
            dus.append(d)
        torch.cuda.synchronize()
        grp = fa.FlowFVGroup(sps)
        got = grp.entropy_error_device([d.data_ptr() for d in dus])
        grp.close()
        for sp in sps:
            sp.close()
        print("group entropy %s: %.17g, group - long double %.3g relative, group^2 - handle^2 %.3g relative"
              % (family, want, abs(got - want) / want, abs(got * got - one * one) / (one * one)))
        assert abs(got - want) <= 1e-12 * want, (got, want)
        # both square roots are correctly rounded, so each square is within 2 2^-53 of its sum; the sums add the
        # same non-negative terms in two orders (other blocks, then the ranks on the host)
        assert abs(got * got - one * one) <= 4 * nranks * 2.0 ** -53 * one * one, (got, one)
