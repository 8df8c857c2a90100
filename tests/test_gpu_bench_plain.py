"""A plain bench.py run (no --full) on one GPU at reduced size: one JSON line with the headline fields and
none of the secondary figures, --steps timed steps, and --dump-outputs: residual.npy / dtm.npy hold the rows
of the dumped cells, in the mesh's own order, bit for bit what the library's host-pointer entry gives for
the same mesh and seeded state. --scale 8 (63,488 cells) dumps every cell, --scale 2 (1,015,808 cells) the
seeded sample of bench.DUMP_MAX_ROWS."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_ONLY = ("roofline", "valu_roofline", "kernels_ms", "cpu_baseline", "host_boundary", "fast_math", "staged_path",
             "pipelined_path", "implicit_step", "recorded", "halo_parity", "multi_gpu")


@pytest.mark.parametrize("scale,cells", [(8, 63488), (2, 1015808)])
def test_plain_run_line_and_dumped_outputs(scale, cells, tmp_path):
    import bench
    import cases
    import fvens_amd as fa
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dump = str(tmp_path / "dump")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--scale", str(scale), "--preheat-ms", "20", "--dump-outputs", dump],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    print(json.dumps({k: d[k] for k in ("value", "ms_per_step", "dump_outputs", "phases_s")}))
    assert d["metric"].startswith("Mfaces/s") and d["unit"] == "Mfaces/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["n_gpus"] == 1 and d["steps"] == 7 and d["warmup"] == 2 and d["full"] is False
    assert d["config"]["cells"] == cells
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["faces"] / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]

    picked = bench.dump_cells(cells)
    assert len(picked) == min(cells, bench.DUMP_MAX_ROWS)
    r, dt = np.load(os.path.join(dump, "residual.npy")), np.load(os.path.join(dump, "dtm.npy"))
    assert r.dtype == np.float64 and dt.dtype == np.float64
    assert r.shape == (len(picked), 4) and dt.shape == (len(picked),)
    assert r.nbytes + dt.nbytes <= 64 * 2**20

    mesh, _ = bench.c4_mesh(fa, scale)
    p = cases.physics("naca")
    u = cases.state(mesh, p, seed=42)
    dev = fa.FlowFV(mesh, p, cases.numerics("ROE", "LEASTSQUARES", "VANALBADA"))
    r0 = np.zeros((mesh.nelem, 4))
    dt0 = np.zeros(mesh.nelem)
    dev.compute_residual(u, r0, True, dt0)
    dev.close()
    assert np.isfinite(r).all() and np.abs(r).max() > 0 and (dt > 0).all()
    assert np.array_equal(r, r0[picked]) and np.array_equal(dt, dt0[picked])
