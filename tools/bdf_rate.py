#!/usr/bin/env python3
"""Cost of the implicit time-accurate driver (fvhip_bdf_device, BDF2 in dual time, line-implicit GMRES) on the
bench's C4 mesh at physical steps of --ratios times the first minimum time step, beside the explicit SSP-RK driver
of order 2 at CFL 0.4 carried to the same physical time. Host clock round calls that end in a synchronise, a warm-up
of every shape first, --repeat alternating repeats. A run is --steps steps from the same start; its first step is
the BDF1 start, so ms per step is the mean over one BDF1 and steps - 1 BDF2 steps. One JSON line per repeat; --out
keeps them all in one file.

    python tools/bdf_rate.py [--small] [--steps 3] [--ratios 100 1000] [--tol 1e-8] [--maxiter 200] [--repeat 3]
                             [--no-explicit] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fvens_amd as fa  # noqa: E402
import cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the tests' small O-grid instead of C4")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--ratios", type=float, nargs="+", default=[100.0, 1000.0])
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=200)
    ap.add_argument("--matrix-free", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-explicit", action="store_true", help="skip the SSP-RK runs to the same time")
    ap.add_argument("--out")
    a = ap.parse_args()
    m = fa.UMesh.naca_ogrid(96, 6, 18) if a.small else fa.UMesh.naca_ogrid(2048, 256, 864, 20.0, 1e-5, farmap=1)
    p = cases.physics("naca")
    n = cases.numerics("ROE", "LEASTSQUARES", "VANALBADA")
    u0 = cases.state(m, p, 42)
    sp = fa.FlowFV(m, p, n)
    d0 = torch.tensor(np.ascontiguousarray(u0[sp.permutation()]), device="cuda")
    dr = torch.zeros_like(d0)
    dd = torch.zeros(m.nelem, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sp.compute_residual_device(d0.data_ptr(), dr.data_ptr(), dd.data_ptr(), True, True)
    sp.synchronize()
    dtmin = float(dd.min())
    cfg = fa.ImplicitConfig(tol=a.tol, maxiter=a.maxiter, cflinit=1e3, cflfin=1e6, lin_rtol=1e-3, lin_maxit=60,
                            restart=30, prec_lines=True, matrix_free=a.matrix_free)
    K = a.steps

    def implicit(ratio):
        du = d0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        try:
            st, rec = sp.bdf_device(du.data_ptr(), 2, 1e9, K, cfg, dt=ratio * dtmin, record=True)
        except RuntimeError as e:
            return dict(error=str(e))
        ms = 1e3 * (time.perf_counter() - t) / K
        assert st["steps"] == K and bool(torch.isfinite(du).all())
        return dict(ms_per_step=ms, inner_per_step=[int(x) for x in rec[:, 2]], final_ratio=[float(x) for x in rec[:, 3]],
                    lin_iters=st["lin_iters"], lin_unconverged=st["lin_unconverged"],
                    inner_unconverged=st["inner_unconverged"], time=st["time"])

    def explicit(T):
        du = d0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        try:
            st, _ = sp.ssprk_device(du.data_ptr(), 2, T, 1 << 30, cfl=0.4)
        except RuntimeError as e:
            return dict(error=str(e))
        s = time.perf_counter() - t
        assert st["time"] == T and bool(torch.isfinite(du).all())
        return dict(ms=1e3 * s, steps=st["steps"], ms_per_step=1e3 * s / st["steps"])

    implicit(a.ratios[0])                                  # warm-up: every buffer and structure of both drivers
    if not a.no_explicit:
        explicit(10.0 * dtmin)
    out = {"cells": int(m.nelem), "faces": int(m.naface), "steps_per_run": K, "dtmin": dtmin, "tol": a.tol,
           "maxiter": a.maxiter, "matrix_free": bool(a.matrix_free), "runs": []}
    for _ in range(a.repeat):
        row = {}
        for ratio in a.ratios:
            r = implicit(ratio)
            if not a.no_explicit and "time" in r:
                r["ssprk2_same_time"] = explicit(r["time"])
            row["h=%g dtmin" % ratio] = r
        out["runs"].append(row)
        print(json.dumps(row), flush=True)
    sp.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
