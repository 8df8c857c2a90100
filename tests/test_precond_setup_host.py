"""The preconditioners' host structure builders (fvens_amd/csrc/precond_setup.cpp: cellGraph, colourCells,
buildLines, amgFineGraph, and amg.cpp's coarsening loop) on the CPU, through tests/native/precond_host_check.cpp:
the layouts are built with the calls handle creation makes, the builders run without a device.

Each case's lines, colouring and multigrid levels are compared, by sha256 of their int32 bytes and by plain
counts, with tests/fixtures/precond_structures.json, recorded from real handles by
tests/test_gpu_precond_structures.py (which checks the handles against the same file). Structural facts are
asserted directly as well, so a wrong builder is caught even against a stale fixture."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fvens_amd as fa
import cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"
FIXTURE = os.path.join(HERE, "fixtures", "precond_structures.json")
AMG_LEVELS, AMG_THRESHOLD = 4, 0.2
LINE_MAX_CELLS, LINE_TWIST_MIN = 256, 16

# the coverage each case must show (`expect`; figures of the builders on these meshes): a recording that
# misses a branch is refused by the recorder
CASES = {
    # twisted, short and single lines side by side; three coarse levels, the last below 64 rows
    "naca_ogrid": dict(mesh=lambda: fa.UMesh.naca_ogrid(64, 12, 8, 20.0, 1e-4), physics="naca", thr=0.0, cells=1792,
                       expect=dict(lines=312, twisted=18, short=74, singles=220, longest=60, colours=4,
                                   levels=[647, 221, 61])),
    # 600-cell lines cut at LINE_MAX_CELLS, every piece twisted
    "flat_plate": dict(mesh=lambda: fa.UMesh.flat_plate(8, 300, xlead=0.5, height=0.5, wallspacing=1e-5),
                       physics="plate_inviscid", thr=1.0, cells=2400,
                       expect=dict(lines=14, twisted=14, short=0, singles=0, longest=256)),
    # triangles and quadrangles: 3- and 4-neighbour rows
    "naca_hybrid": dict(mesh=lambda: fa.UMesh.naca_hybrid(48, 8, 12, 32, 20.0, 1e-4), physics="naca", thr=0.0,
                        cells=3542, expect=dict(lines=1501, twisted=57, levels=[976, 265, 95])),
    # all triangles, radius ratio 20: no line longer than 2, no twisted group, coarsening stopped after two
    # levels by the 64-row rule
    "cylinder_ratio20": dict(mesh=lambda: fa.UMesh.cylinder_ogrid(48, 12, 1.0, 20.0), physics="cyl", thr=0.0,
                             cells=1152, expect=dict(twisted=0, max_longest=2, levels=[277, 48])),
    # ... and with the generator's default radii (ratio 40): the triangles of the outer rings are stretched
    # enough to form circumferential lines of up to 96 cells
    "cylinder": dict(mesh=lambda: fa.UMesh.cylinder_ogrid(48, 12), physics="cyl", thr=0.0, cells=1152, expect=dict()),
    # nghost > 0: ghost couplings enter the ratios but not the lines, colouring or graph
    "naca_ogrid_rank1of3": dict(mesh=lambda: fa.UMesh.naca_ogrid(64, 12, 8, 20.0, 1e-4), physics="naca", thr=0.0,
                                nparts=3, rank=1, expect=dict(ghosts=True)),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.int32).tobytes()).hexdigest()


def summary(ncell, nghost, start, cells, faces, colour, triples, levels):
    """what the fixture holds of one case; levels: list of dict(n, agg, rowptr, col)"""
    lens = np.diff(start)
    return dict(
        cells=int(ncell), ghosts=int(nghost),
        lines=dict(start=sha(start), cells=sha(cells), faces=sha(faces), count=int(len(lens)),
                   twisted=int((lens >= LINE_TWIST_MIN).sum()), short=int(((lens >= 2) & (lens < LINE_TWIST_MIN)).sum()),
                   singles=int((lens == 1).sum()), longest=int(lens.max())),
        colouring=dict(colour=sha(colour), colours=int(colour.max()) + 1, triples=int(triples)),
        amg=[dict(n=int(L["n"]), nnz=int(len(L["col"])), agg=sha(L["agg"]), rowptr=sha(L["rowptr"]), col=sha(L["col"]))
             for L in levels])


def check_coverage(name, s):
    """the table of CASES against a summary"""
    e = CASES[name]["expect"]
    if "cells" in CASES[name]:
        assert s["cells"] == CASES[name]["cells"], (name, s["cells"])
    for key, field in (("lines", "count"), ("twisted", "twisted"), ("short", "short"), ("singles", "singles"),
                       ("longest", "longest")):
        if key in e:
            assert s["lines"][field] == e[key], (name, key, s["lines"])
    if "max_longest" in e:
        assert s["lines"]["longest"] <= e["max_longest"], (name, s["lines"])
    if "colours" in e:
        assert s["colouring"]["colours"] == e["colours"], (name, s["colouring"])
    if "levels" in e:
        assert [L["n"] for L in s["amg"]] == e["levels"], (name, [L["n"] for L in s["amg"]])
    if e.get("ghosts"):
        assert s["ghosts"] > 0, name
    assert s["colouring"]["triples"] == 0, name      # a conforming 2-D mesh has no three pairwise-adjacent cells


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _lib():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    lib = os.path.join(out, "libprecond_host.so")
    csrc = os.path.join(ROOT, "fvens_amd", "csrc")
    srcs = [os.path.join(HERE, "native", "precond_host_check.cpp")] + [
        os.path.join(csrc, f) for f in ("precond_setup.cpp", "layout.cpp", "partition.cpp", "mesh.cpp", "amg.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in deps):
        subprocess.run([HIPCC, "-std=c++17", "-O3", "-ffp-contract=off", "-x", "hip", "--offload-arch=gfx950",
                        "-shared", "-fPIC"] + srcs + ["-o", lib], check=True, capture_output=True)
    L = ctypes.CDLL(lib)
    L.pc_build.restype = ctypes.c_void_p
    L.pc_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                           ctypes.c_int, ctypes.c_double]
    L.pc_error.restype = ctypes.c_char_p
    L.pc_size.restype = ctypes.c_longlong
    L.pc_size.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.pc_copy.restype = None
    L.pc_copy.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.pc_free.restype = None
    L.pc_free.argtypes = [ctypes.c_void_p]
    return L


# arrays of the shim (pc_size / pc_copy); level l's are LEVEL0 + 3 (l - 1) + (agg, rowptr, col)
(SCALARS, LINE_START, LINE_CELLS, LINE_FACES, COLOUR, COLOUR_START, COLOUR_CELLS, IF_L, IF_R,
 PACK_GSTART, PACK_CELL, PACK_FACE, PACK_LEN, PERM) = range(14)
LEVEL0 = 16


def host_case(name):
    """the builders' output for one case: dict of int32 arrays and scalars"""
    c = CASES[name]
    return host_structures(c["mesh"](), c["physics"], c["thr"], c.get("nparts", 1), c.get("rank", 0))


def host_structures(m, physics, thr=0.0, nparts=1, rank=0):
    """the builders' output for a mesh (rank `rank` of its RCB partition into nparts): dict of int32 arrays and
    scalars; perm is what FlowFV.permutation() of such a handle returns"""
    L = _lib()
    cfg, keep = fa._config_struct(cases.physics(physics), cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
    thr = thr if thr > 0 else 4.0
    h = L.pc_build(ctypes.addressof(m.view), ctypes.addressof(cfg), nparts, rank, thr, AMG_LEVELS, AMG_THRESHOLD)
    del keep
    assert h, L.pc_error().decode()

    def arr(what):
        a = np.zeros(int(L.pc_size(h, what)), np.int32)
        if len(a):
            L.pc_copy(h, what, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return a
    try:
        sc = arr(SCALARS)
        out = dict(zip(("ncell", "nghost", "triples", "nlevels", "twisted_groups", "nlines", "ngroups", "nrows"),
                       [int(x) for x in sc]))
        for key, what in (("start", LINE_START), ("cells", LINE_CELLS), ("faces", LINE_FACES), ("colour", COLOUR),
                          ("colour_start", COLOUR_START), ("colour_cells", COLOUR_CELLS), ("if_L", IF_L), ("if_R", IF_R),
                          ("gstart", PACK_GSTART), ("pcell", PACK_CELL), ("pface", PACK_FACE), ("plen", PACK_LEN),
                          ("perm", PERM)):
            out[key] = arr(what)
        out["levels"] = []
        for l in range(out["nlevels"]):
            agg, rowptr, col = (arr(LEVEL0 + 3 * l + k) for k in range(3))
            out["levels"].append(dict(n=len(rowptr) - 1, agg=agg, rowptr=rowptr, col=col))
    finally:
        L.pc_free(h)
    return out


_cache = {}


def _host(name):
    if name not in _cache:
        _cache[name] = host_case(name)
    return _cache[name]


needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@needs_hipcc
@pytest.mark.parametrize("name", list(CASES))
def test_builders_match_recorded_handles(name):
    """lines, colouring and every multigrid level equal what the device handles of the recorded commit held"""
    o = _host(name)
    s = summary(o["ncell"], o["nghost"], o["start"], o["cells"], o["faces"], o["colour"], o["triples"], o["levels"])
    check_coverage(name, s)
    assert s == fixture()["cases"][name]


@needs_hipcc
@pytest.mark.parametrize("name", list(CASES))
def test_lines_cover_cells_along_shared_faces(name):
    """every owned cell in exactly one line; consecutive line cells share the recorded interior face, with the
    side bit of the earlier cell; no piece longer than LINE_MAX_CELLS; longest first; the packed lanes hold
    the same lines (twisted ones split at their middle cell)"""
    o = _host(name)
    N, start, cells, faces = o["ncell"], o["start"], o["cells"], o["faces"]
    assert np.array_equal(np.sort(cells), np.arange(N))
    lens = np.diff(start)
    assert start[0] == 0 and start[-1] == N and lens.min() >= 1 and lens.max() <= LINE_MAX_CELLS
    assert np.all(np.diff(lens) <= 0)
    first = np.zeros(N, bool)
    first[start[:-1]] = True
    assert np.all(faces[first] == -1) and np.all(faces[~first] >= 0)
    k = np.nonzero(~first)[0]
    fi, side, c, prev = faces[k] >> 1, faces[k] & 1, cells[k], cells[k - 1]
    Lc, Rc = o["if_L"][fi], o["if_R"][fi]
    assert np.all(np.where(side == 1, (Rc == prev) & (Lc == c), (Lc == prev) & (Rc == c)))
    # packed form: lane `lane` of group g holds rows gstart[g] .. of slot (row*64 + lane)
    assert o["nlines"] == len(lens) and o["ngroups"] == len(o["gstart"]) - 1 and o["nrows"] == o["gstart"][-1]
    ntw = int((lens >= LINE_TWIST_MIN).sum())
    assert o["twisted_groups"] == (ntw + 31) // 32
    seen = np.zeros(N, int)
    for g in range(o["ngroups"]):
        rows = np.arange(o["gstart"][g], o["gstart"][g + 1])
        for lane in range(64):
            n = o["plen"][64 * g + lane]
            lane_cells = o["pcell"][rows * 64 + lane]
            assert np.all(lane_cells[:n] >= 0) and np.all(lane_cells[n:] == -1)
            if g < o["twisted_groups"]:
                if lane >= 32 or n == 0:
                    continue
                line = 32 * g + lane
                full = cells[start[line]:start[line + 1]]
                t = (len(full) - 1) // 2
                bot = o["pcell"][rows * 64 + lane + 32][:o["plen"][64 * g + lane + 32]]
                assert np.array_equal(lane_cells[:n], full[:t + 1]) and np.array_equal(bot, full[:t - 1 if t else None:-1])
                seen[full] += 1
            elif n:
                line = ntw + 64 * (g - o["twisted_groups"]) + lane
                assert np.array_equal(lane_cells[:n], cells[start[line]:start[line + 1]])
                assert np.array_equal(o["pface"][rows * 64 + lane][1:n], faces[start[line] + 1:start[line + 1]])
                seen[lane_cells[:n]] += 1
    assert np.all(seen == 1)


@needs_hipcc
@pytest.mark.parametrize("name", list(CASES))
def test_colouring_is_proper(name):
    """no two owned cells sharing an interior face have the same colour; the colour lists hold every cell once,
    ascending within a colour"""
    o = _host(name)
    N, col = o["ncell"], o["colour"]
    Lc, Rc = o["if_L"], o["if_R"]
    owned = (Lc < N) & (Rc < N)
    assert owned.any() and np.all(col[Lc[owned]] != col[Rc[owned]])
    cs, cc = o["colour_start"], o["colour_cells"]
    assert cs[0] == 0 and cs[-1] == N and len(cs) == col.max() + 2
    for q in range(len(cs) - 1):
        part = cc[cs[q]:cs[q + 1]]
        assert np.all(col[part] == q) and np.all(np.diff(part) > 0)


@needs_hipcc
@pytest.mark.parametrize("name", list(CASES))
def test_every_cell_in_one_aggregate_per_level(name):
    o = _host(name)
    nf = o["ncell"]
    assert len(o["levels"]) >= 1
    for L in o["levels"]:
        assert L["agg"].shape == (nf,) and L["agg"].min() == 0 and L["agg"].max() == L["n"] - 1
        assert len(np.unique(L["agg"])) == L["n"] and nf >= 64 and L["n"] * 5 <= nf * 4
        assert np.all(np.diff(L["rowptr"]) >= 1) and L["col"].max() == L["n"] - 1
        nf = L["n"]
