"""The leg table of an in-process halo exchange (fvens_amd/csrc/halo_legs.hpp: haloLegs, which fvhip_group_create
stores and every group exchange walks) on the CPU, through tests/native/halo_legs_check.cpp: the mesh is split as
fvhip_partition_graph splits it, every rank's layout is built with the calls handle creation makes, and the table
is built from those layouts without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fvens_amd as fa
import cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"

MESHES = {
    "ogrid": (lambda: fa.UMesh.naca_ogrid(64, 12, 8, 20.0, 1e-4), 1792),
    "hybrid": (lambda: fa.UMesh.naca_hybrid(48, 8, 12, 32, 20.0, 1e-4), 3542),
}
SPLITS = [("ogrid", 3), ("ogrid", 8), ("hybrid", 3)]
# halo layers asked of extractPartition: 2 is what fvhip_create_partitioned builds, 1 the one-layer halo
LAYERS = [2, 1]


def _lib():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libhalo_legs_host.so")
    csrc = os.path.join(ROOT, "fvens_amd", "csrc")
    srcs = [os.path.join(HERE, "native", "halo_legs_check.cpp")] + [
        os.path.join(csrc, f) for f in ("layout.cpp", "partition.cpp", "mesh.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in deps):
        subprocess.run([HIPCC, "-std=c++17", "-O3", "-ffp-contract=off", "-x", "hip", "--offload-arch=gfx950",
                        "-shared", "-fPIC"] + srcs + ["-o", lib], check=True, capture_output=True)
    L = ctypes.CDLL(lib)
    L.hl_build.restype = ctypes.c_void_p
    L.hl_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.hl_error.restype = ctypes.c_char_p
    for f in (L.hl_rank, L.hl_legs):
        f.restype = None
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.hl_broken.restype = ctypes.c_char_p
    L.hl_broken.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.hl_free.restype = None
    L.hl_free.argtypes = [ctypes.c_void_p]
    return L


class Table:
    """the layouts and legs of one split: per rank nnbr, nghost, halo_layers and legs [nnbr][8]
    (neighbour rank, peer, kk, ghost_start, ghost count of 1 and 2 layers, the peer's send count of 1 and 2)"""

    def __init__(self, mesh, nparts, layers):
        self.L = _lib()
        m, cells = MESHES[mesh]
        m = m()
        assert m.view.nelem == cells
        cfg, keep = fa._config_struct(cases.physics("naca"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
        self.h = self.L.hl_build(ctypes.addressof(m.view), ctypes.addressof(cfg), nparts, layers)
        del keep
        assert self.h, self.L.hl_error().decode()
        self.nparts = nparts
        self.ranks = []
        for r in range(nparts):
            info = np.zeros(4, np.int32)
            self.L.hl_rank(self.h, r, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
            legs = np.zeros((int(info[3]), 8), np.int32)
            if len(legs):
                self.L.hl_legs(self.h, r, legs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
            self.ranks.append(dict(nnbr=int(info[0]), nghost=int(info[1]), layers=int(info[2]), legs=legs))

    def broken(self, rank, how):
        return self.L.hl_broken(self.h, rank, how).decode()

    def __del__(self):
        if getattr(self, "h", None):
            self.L.hl_free(self.h)


_cache = {}


def _table(mesh, nparts, layers):
    key = (mesh, nparts, layers)
    if key not in _cache:
        _cache[key] = Table(mesh, nparts, layers)
    return _cache[key]


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
splits = pytest.mark.parametrize("mesh,nparts", SPLITS)
layers_ = pytest.mark.parametrize("layers", LAYERS)


@needs_hipcc
@splits
@layers_
def test_layouts_report_the_halo_layers_asked_for(mesh, nparts, layers):
    T = _table(mesh, nparts, layers)
    assert [R["layers"] for R in T.ranks] == [layers] * nparts
    assert all(R["nnbr"] >= 1 and R["nghost"] > 0 for R in T.ranks)


@needs_hipcc
@splits
@layers_
def test_every_leg_has_its_reverse_with_equal_counts(mesh, nparts, layers):
    T = _table(mesh, nparts, layers)
    for i, R in enumerate(T.ranks):
        assert len(R["legs"]) == R["nnbr"]
        for k, (q, peer, kk, _, g1, g2, s1, s2) in enumerate(R["legs"]):
            assert peer == q != i                  # the list holds rank r at entry r
            back = T.ranks[peer]["legs"][kk]
            assert (back[0], back[1], back[2]) == (i, i, k)
            assert g1 == s1 and g2 == s2           # ghostCount(k, layers) == sendCount(kk, layers), layers 1 and 2
            assert 0 < g1 <= g2
            if layers == 1:
                assert g1 == g2
    if layers == 2:                                 # somewhere a second layer exists, or the case shows nothing
        assert any(g[4] < g[5] for R in T.ranks for g in R["legs"])


@needs_hipcc
@splits
@layers_
def test_legs_tile_the_ghost_block_once_in_order(mesh, nparts, layers):
    T = _table(mesh, nparts, layers)
    for R in T.ranks:
        at = 0
        for g in R["legs"]:
            assert g[3] == at                       # ghost_start[k]: no gap, no overlap, ascending
            at += g[5]
        assert at == R["nghost"]


@needs_hipcc
def test_a_rank_without_neighbours_has_no_legs():
    T = _table("ogrid", 1, 2)
    assert T.ranks[0]["nnbr"] == 0 and T.ranks[0]["nghost"] == 0 and len(T.ranks[0]["legs"]) == 0


@needs_hipcc
@splits
def test_damaged_lists_are_refused(mesh, nparts):
    T = _table(mesh, nparts, 2)
    for rank in range(nparts):
        assert T.broken(rank, 0) == "halo lists are not symmetric"
        assert T.broken(rank, 1) == "halo sizes differ"
