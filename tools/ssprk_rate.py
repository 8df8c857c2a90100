#!/usr/bin/env python3
"""Step rate of the time-accurate SSP Runge-Kutta driver (fvhip_ssprk_device) on the bench's C4 mesh beside the
residual's own time: a stage is one residual plus one row pass. Host clock round calls that end in a
synchronise, a warm-up of every shape first, --repeat alternating repeats of (residuals, orders 1-3, order 3
with the record). One JSON line per repeat; --out keeps them all in one file.

    python tools/ssprk_rate.py [--small] [--steps 40] [--repeat 3] [--out FILE]
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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
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
    K = a.steps

    def residuals(k):
        t = time.perf_counter()
        for _ in range(k):
            sp.compute_residual_device(d0.data_ptr(), dr.data_ptr(), dd.data_ptr(), True, True)
        sp.synchronize()
        return (time.perf_counter() - t) / k

    def steps(order, record):
        du = d0.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        st, _ = sp.ssprk_device(du.data_ptr(), order, 1e9, K, cfl=0.4, record=record)
        dt = (time.perf_counter() - t) / K
        assert st["steps"] == K and bool(torch.isfinite(du).all())
        return dt

    residuals(20)
    steps(3, False)
    steps(3, True)
    out = {"cells": int(m.nelem), "faces": int(m.naface), "steps_per_timing": K, "cfl": 0.4, "runs": []}
    for _ in range(a.repeat):
        row = {"residual_ms": 1e3 * residuals(3 * K)}
        for order in (1, 2, 3):
            row["order%d_ms_per_step" % order] = 1e3 * steps(order, False)
        row["order3_record_ms_per_step"] = 1e3 * steps(3, True)
        out["runs"].append(row)
        print(json.dumps(row), flush=True)
    sp.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
