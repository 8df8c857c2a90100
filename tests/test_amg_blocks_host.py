"""The block smoother's (block, colour) offset table (fvens_amd/csrc/amg.cpp amgBlockOffsets; amg_smoother 1,
amg.hip k_amg_bjgs) on the CPU, through tests/native/amg_blocks_check.cpp: the hierarchy is built with the calls
fvhip_ctx::ensureAmg makes, the table with the call fvhip_ctx::amgBlocks makes, without a device.

A level of n rows is cut into ceil(n / R) contiguous blocks of R rows; the table gives, per block and colour, the
sub-range of the level's colour-ordered row list that lies in the block. The kernel trusts it for its LDS indices,
so every property it relies on is asserted: the ranges tile each colour's list exactly once, in block order; every
row of range (k, q) lies in block k and has colour q; the rows ascend. R = 64 gives many blocks with a partial
last one (mesh A level 1: 11 blocks, the last of 7 rows) and ranges that are empty."""
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
AMG_LEVELS, AMG_THRESHOLD = 4, 0.2

MESHES = {
    "A": dict(mesh=lambda: fa.UMesh.naca_ogrid(64, 12, 8, 20.0, 1e-4), cells=1792, levels=[647, 221, 61]),
    "B": dict(mesh=lambda: fa.UMesh.naca_hybrid(48, 8, 12, 32, 20.0, 1e-4), cells=3542, levels=[976, 265, 95]),
}
BLOCK_ROWS = (64, 128, 2048)

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def _lib():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libamg_blocks_host.so")
    csrc = os.path.join(ROOT, "fvens_amd", "csrc")
    srcs = [os.path.join(HERE, "native", "amg_blocks_check.cpp")] + [
        os.path.join(csrc, f) for f in ("precond_setup.cpp", "layout.cpp", "partition.cpp", "mesh.cpp", "amg.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in deps):
        subprocess.run([HIPCC, "-std=c++17", "-O3", "-ffp-contract=off", "-x", "hip", "--offload-arch=gfx950",
                        "-shared", "-fPIC"] + srcs + ["-o", lib], check=True, capture_output=True)
    L = ctypes.CDLL(lib)
    L.ab_build.restype = ctypes.c_void_p
    L.ab_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    L.ab_error.restype = ctypes.c_char_p
    L.ab_levels.restype = ctypes.c_int
    L.ab_levels.argtypes = [ctypes.c_void_p]
    L.ab_get.restype = ctypes.c_longlong
    L.ab_get.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ab_copy.restype = None
    L.ab_copy.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    L.ab_free.restype = None
    L.ab_free.argtypes = [ctypes.c_void_p]
    return L


ROWS, COLOUR_START, CELLS, OFFSETS = range(4)
_cache = {}


def host_levels(name):
    """per level of mesh `name`: dict(n, cstart, cells, off={R: [nblocks + 1][ncolours]})"""
    if name in _cache:
        return _cache[name]
    L = _lib()
    c = MESHES[name]
    m = c["mesh"]()
    assert m.nelem == c["cells"]
    cfg, keep = fa._config_struct(cases.physics("naca"), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
    h = L.ab_build(ctypes.addressof(m.view), ctypes.addressof(cfg), AMG_LEVELS, AMG_THRESHOLD)
    del keep
    assert h, L.ab_error().decode()

    def arr(level, what, R=0):
        k = int(L.ab_get(h, level, what, R))
        assert k >= 0, L.ab_error().decode()
        a = np.zeros(k, np.int32)
        if k:
            L.ab_copy(h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return a
    try:
        out = []
        for l in range(L.ab_levels(h)):
            lev = dict(n=int(arr(l, ROWS)[0]), cstart=arr(l, COLOUR_START), cells=arr(l, CELLS), off={})
            nc = len(lev["cstart"]) - 1
            for R in BLOCK_ROWS:
                lev["off"][R] = arr(l, OFFSETS, R).reshape(-1, nc)
            out.append(lev)
    finally:
        L.ab_free(h)
    _cache[name] = out
    return out


@needs_hipcc
@pytest.mark.parametrize("name", list(MESHES))
def test_block_colour_ranges_tile_the_colour_lists(name):
    levels = host_levels(name)
    assert [lev["n"] for lev in levels] == MESHES[name]["levels"]
    for l, lev in enumerate(levels):
        n, cstart, cells = lev["n"], lev["cstart"], lev["cells"]
        nc = len(cstart) - 1
        assert cstart[0] == 0 and cstart[-1] == n and np.array_equal(np.sort(cells), np.arange(n))
        colour = np.empty(n, np.int64)
        for q in range(nc):
            colour[cells[cstart[q]:cstart[q + 1]]] = q
        for R in BLOCK_ROWS:
            off = lev["off"][R]
            nb = -(-n // R)
            assert off.shape == (nb + 1, nc), (name, l, R, off.shape)
            # tiling: block 0 starts each colour's list, block nb ends it, the ranges follow each other
            assert np.array_equal(off[0], cstart[:-1]) and np.array_equal(off[nb], cstart[1:])
            assert np.all(np.diff(off, axis=0) >= 0)
            seen = np.zeros(n, int)
            for k in range(nb):
                for q in range(nc):
                    rows = cells[off[k, q]:off[k + 1, q]]
                    assert np.all((rows >= k * R) & (rows < min(n, (k + 1) * R))), (name, l, R, k, q)
                    assert np.all(colour[rows] == q) and np.all(np.diff(rows) > 0), (name, l, R, k, q)
                    seen[rows] += 1
            assert np.all(seen == 1), (name, l, R)


@needs_hipcc
def test_partial_last_block_and_empty_ranges_at_64_rows():
    """the shapes the GPU tests rely on: mesh A at R = 64 has 11 blocks on level 1 (the last of 7 rows), 4 on level
    2 (the last of 29), one on level 3; and some (block, colour) range is empty, so the kernel's barrier after an
    empty colour is exercised"""
    levels = host_levels("A")
    assert [lev["off"][64].shape[0] - 1 for lev in levels] == [11, 4, 1]
    assert levels[0]["n"] - 10 * 64 == 7 and levels[1]["n"] - 3 * 64 == 29
    empty = 0
    for name in MESHES:
        for lev in host_levels(name):
            off = lev["off"][64]
            empty += int((np.diff(off, axis=0) == 0).sum())
    assert empty >= 1
