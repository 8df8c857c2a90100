#!/usr/bin/env python3
"""Where a block of the fused residual kernel spends its time: reduces the shader-clock stamps of a probe
build of the library (fused.hip FVHIP_FZ_STAMPS) to per-segment statistics.

Build the probe library into a directory of its own (the product library is not touched):
  make -C fvens_amd EXTRA=-DFVHIP_FZ_STAMPS OBJDIR=<dir>/obj LIB=<dir>/libfvhip_stamps.so
and run, with FVHIP_LIB pointing at it,
  FVHIP_LIB=<dir>/libfvhip_stamps.so python tools/fz_stamps.py [--steps 30] [--label text] > out.json

Runs the headline workload (C4 mesh, Roe + WLS + MUSCL/Van Albada) and the same numerics on the C2 mesh,
`steps` residuals each, and reads the LAST launch's stamps: wave 0 of every block stamps the shader clock
at kernel entry, with the patch metadata in registers, before the first barrier (rows loaded and staged),
after barrier 1, after barrier 2 (gradients), after the second flux-staging barrier, and after its last
store. Word 7 of a block is the wall-clock ticks from the first to the last stamp, which converts its
shader cycles to microseconds (so a segment's time is its share of the block's wall time). Prints one JSON
object: per mesh and segment the median, 10th and 90th percentile over the blocks, in microseconds.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEGMENTS = ("entry_to_metadata", "metadata_to_rows_staged", "wait_barrier_1", "gradients_to_barrier_2",
            "faces_to_flux_barriers", "cell_sums_to_last_store")


def stamps_of(fa, torch, cases, mesh, steps):
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u = cases.state(mesh, p, seed=42)
    sp = fa.FlowFV(mesh, p, n, device=torch.cuda.current_device())
    du = torch.tensor(u[sp.permutation()], device="cuda")
    dr = torch.empty((sp.nown, 4), dtype=torch.float64, device="cuda")
    ddt = torch.empty(sp.nown, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(steps):
        sp.compute_residual_device(du.data_ptr(), dr.data_ptr(), ddt.data_ptr(), True, True)
    sp.synchronize()
    L = fa._ffi.lib()
    if not hasattr(L, "fvhip_debug_fz_stamps"):
        raise SystemExit("the loaded library is no probe build (make EXTRA=-DFVHIP_FZ_STAMPS; FVHIP_LIB)")
    f = L.fvhip_debug_fz_stamps
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong),
                  ctypes.POINTER(ctypes.c_int)]
    npatch = sp.layout_stats()["patches"]
    cap = 8 * 8 * ((npatch + 7) // 8)
    buf = np.zeros(cap, dtype=np.uint64)
    nb, khz = ctypes.c_longlong(0), ctypes.c_int(0)
    fa.check(f(sp._h, buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(nb), ctypes.byref(khz)))
    sp.close()
    w = buf[:8 * nb.value].reshape(-1, 8).astype(np.int64)
    w = w[w[:, 6] > 0]                       # blocks without a patch wrote nothing
    return w, khz.value, mesh.nelem


def reduce(w, khz):
    cyc = np.diff(w[:, :7], axis=1).astype(np.float64)           # six segments, shader cycles
    total = (w[:, 6] - w[:, 0]).astype(np.float64)
    wall_us = w[:, 7] / (khz * 1e-3)                                # ticks / (ticks per microsecond)
    us_per_cycle = wall_us / total
    seg = cyc * us_per_cycle[:, None]
    out = {"blocks": int(len(w)), "wall_clock_khz": int(khz),
           "shader_mhz_median": round(float(np.median(1.0 / us_per_cycle)), 1),
           "block_us": {k: round(float(v), 3) for k, v in zip(("median", "p10", "p90"),
                                                              np.percentile(wall_us, [50, 10, 90]))},
           "segments_us": {}}
    for i, name in enumerate(SEGMENTS):
        q = np.percentile(seg[:, i], [50, 10, 90])
        out["segments_us"][name] = {"median": round(float(q[0]), 3), "p10": round(float(q[1]), 3),
                                    "p90": round(float(q[2]), 3),
                                    "cycles_median": int(np.median(cyc[:, i]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    import fvens_amd as fa
    import cases
    from bench import c4_mesh
    doc = {"label": args.label, "library": os.path.basename(fa._ffi.LIB_PATH),
           "build": fa._ffi.lib().fvhip_build_info().decode() if hasattr(fa._ffi.lib(), "fvhip_build_info") else None,
           "kernel": "k_residual_wls<ROE, MUSCL, DT>", "steps": args.steps,
           "stamps": "wave 0 of every block of the last launch; segment time = its share of the block's wall-clock time",
           "meshes": {}}
    for name, mesh in (("c4", c4_mesh(fa, 1, 1)[0]), ("c2", fa.UMesh.naca_ogrid(512, 64, 192))):
        w, khz, cells = stamps_of(fa, torch, cases, mesh, args.steps)
        doc["meshes"][name] = dict(cells=cells, **reduce(w, khz))
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
