"""The row orders of the sweep-based block ILU(0)/SGS (fvens_amd/csrc/precond_setup.cpp iluOrder;
fvhip_implicit_config::ilu_order) on the CPU, through tests/native/ilu_order_check.cpp: the layouts are built with
the calls handle creation makes, the builder runs without a device.

Order 1 is the internal (Hilbert) order, order 2 reverse Cuthill-McKee of the owned cells' interior-face graph.
Asserted for order 2: the rank is a permutation; read backwards it lists each connected component (components in
ascending lowest internal id) by non-decreasing breadth-first distance from the component's first cell, every
other cell after one of its neighbours; its bandwidth max |rank[L] - rank[R]| over the owned interior faces is
no larger than the internal order's. For both orders: depth equals the longest chain of lower-neighbour links
counted here in numpy."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg

import fvens_amd as fa
import cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

CASES = {
    "naca_ogrid": dict(mesh=lambda: fa.UMesh.naca_ogrid(64, 12, 8, 20.0, 1e-4), physics="naca"),
    "naca_hybrid": dict(mesh=lambda: fa.UMesh.naca_hybrid(48, 8, 12, 32, 20.0, 1e-4), physics="naca"),
    "cylinder": dict(mesh=lambda: fa.UMesh.cylinder_ogrid(48, 12), physics="cyl"),
    "naca_ogrid_rank1of3": dict(mesh=lambda: fa.UMesh.naca_ogrid(64, 12, 8, 20.0, 1e-4), physics="naca", nparts=3, rank=1),
}


def _lib():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libilu_order_host.so")
    csrc = os.path.join(ROOT, "fvens_amd", "csrc")
    srcs = [os.path.join(HERE, "native", "ilu_order_check.cpp")] + [
        os.path.join(csrc, f) for f in ("precond_setup.cpp", "layout.cpp", "partition.cpp", "mesh.cpp", "amg.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in deps):
        subprocess.run([HIPCC, "-std=c++17", "-O3", "-ffp-contract=off", "-x", "hip", "--offload-arch=gfx950",
                        "-shared", "-fPIC"] + srcs + ["-o", lib], check=True, capture_output=True)
    L = ctypes.CDLL(lib)
    L.io_build.restype = ctypes.c_void_p
    L.io_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.io_error.restype = ctypes.c_char_p
    L.io_size.restype = ctypes.c_longlong
    L.io_size.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.io_copy.restype = None
    L.io_copy.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.io_free.restype = None
    L.io_free.argtypes = [ctypes.c_void_p]
    return L


def host_order(mesh, physics, order, nparts=1, rank=0):
    """iluOrder on the layout of `mesh` (or of rank `rank` of its `nparts` RCB parts): dict(ncell, nghost, depth,
    rank, if_L, if_R), internal cell ids"""
    L = _lib()
    cfg, keep = fa._config_struct(cases.physics(physics), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
    h = L.io_build(ctypes.addressof(mesh.view), ctypes.addressof(cfg), nparts, rank, order)
    del keep
    assert h, L.io_error().decode()

    def arr(what):
        a = np.zeros(int(L.io_size(h, what)), np.int32)
        if len(a):
            L.io_copy(h, what, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return a
    try:
        ncell, nghost, depth = (int(x) for x in arr(0))
        return dict(ncell=ncell, nghost=nghost, depth=depth, rank=arr(1), if_L=arr(2), if_R=arr(3))
    finally:
        L.io_free(h)


def owned_edges(o):
    """(L, R) of the interior faces between two owned cells"""
    N = o["ncell"]
    keep = (o["if_L"] < N) & (o["if_R"] < N)
    return o["if_L"][keep].astype(np.int64), o["if_R"][keep].astype(np.int64)


def longest_chain(N, Lc, Rc, rank):
    """cells of the longest chain i1 < i2 < ... of lower-neighbour links under `rank`"""
    nbrs = [[] for _ in range(N)]
    for a, b in zip(Lc, Rc):
        nbrs[a].append(b)
        nbrs[b].append(a)
    length = np.zeros(N, np.int64)
    for c in np.argsort(rank, kind="stable"):
        length[c] = 1 + max((length[k] for k in nbrs[c] if rank[k] < rank[c]), default=0)
    return int(length.max()) if N else 0


_cache = {}


def _host(name, order):
    if (name, order) not in _cache:
        c = CASES[name]
        _cache[name, order] = host_order(c["mesh"](), c["physics"], order, c.get("nparts", 1), c.get("rank", 0))
    return _cache[name, order]


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@needs_hipcc
@pytest.mark.parametrize("name", list(CASES))
def test_rcm_is_a_reversed_breadth_first_order(name):
    o = _host(name, 2)
    N, rank = o["ncell"], o["rank"].astype(np.int64)
    assert N > 0 and np.array_equal(np.sort(rank), np.arange(N))
    if "nparts" in CASES[name]:
        assert o["nghost"] > 0                       # ghost couplings exist and are left out of the graph
    Lc, Rc = owned_edges(o)
    assert len(Lc) > 0
    A = sp.coo_matrix((np.ones(len(Lc)), (Lc, Rc)), shape=(N, N)).tocsr()
    A = A + A.T
    ncomp, label = csg.connected_components(A, directed=False)
    back = np.argsort(rank)[::-1]                    # the order read backwards: the breadth-first list
    pos = np.empty(N, np.int64)
    pos[back] = np.arange(N)
    # each component is one contiguous piece of the list, components in ascending lowest internal id
    cuts = np.nonzero(np.diff(label[back]) != 0)[0] + 1
    assert len(cuts) == ncomp - 1
    pieces = np.split(back, cuts)
    lows = [int(p.min()) for p in pieces]
    assert lows == sorted(lows) and len({int(label[p[0]]) for p in pieces}) == ncomp
    for piece in pieces:
        dist = csg.shortest_path(A, directed=False, unweighted=True, indices=int(piece[0]))
        assert np.all(np.isfinite(dist[piece])) and np.all(np.diff(dist[piece]) >= 0)
    # every cell but a component's first comes after one of its neighbours
    earliest = np.full(N, N, np.int64)
    np.minimum.at(earliest, Lc, pos[Rc])
    np.minimum.at(earliest, Rc, pos[Lc])
    first = np.zeros(N, bool)
    first[[int(p[0]) for p in pieces]] = True
    assert np.all(earliest[~first] < pos[~first])
    # bandwidth no larger than the internal order's
    bw_rcm, bw_int = int(np.abs(rank[Lc] - rank[Rc]).max()), int(np.abs(Lc - Rc).max())
    print(f"{name}: bandwidth rcm {bw_rcm}, internal {bw_int}; depth rcm {o['depth']}")
    assert bw_rcm <= bw_int


@needs_hipcc
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_depth_is_the_longest_lower_chain(name, order):
    o = _host(name, order)
    N, rank = o["ncell"], o["rank"].astype(np.int64)
    if order == 1:
        assert np.array_equal(rank, np.arange(N))
    Lc, Rc = owned_edges(o)
    depth = longest_chain(N, Lc, Rc, rank)
    print(f"{name} order {order}: depth {depth} of {N} cells")
    assert o["depth"] == depth and 2 <= depth <= N
