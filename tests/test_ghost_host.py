"""CPU check of the residual's boundary ghost states (fvens_amd/csrc/gasdyn.hpp ghost_state), compiled for
the host with the product's flags, against the oracle's BC::ghost: bitwise, 20,000 random interior states
(subsonic / supersonic / reversed / at rest / exact-zero velocity components) for the seven implemented BC
types, subsonic inflow included, walls with the values (0.3, 1.1) and (0.3, 2.0). On the host both sides call
glibc's pow, so a mismatch here is an arithmetic-order difference and not libm: it tells the two apart when a
pow case of test_gpu_regimes.py measures above its bar. States whose subsonic-inflow ghost state is not real
(co2 - cg^2 < 0) are redrawn and counted; at most 10 % may be. The GPU build of the same source is checked on
meshes in test_gpu_regimes.py."""
import os
import re
import subprocess

import pytest

import _oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ghost_states_match_oracle_on_host():
    orc.build()
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "ghost_host_check")
    src = os.path.join(HERE, "native", "ghost_host_check.cpp")
    odir = os.path.join(ROOT, "oracle")
    hdr = os.path.join(ROOT, "fvens_amd", "csrc", "gasdyn.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run([HIPCC, "-std=c++17", "-O3", "-ffp-contract=off", "-x", "hip", "--offload-arch=gfx950",
                        src, "-o", exe, "-L" + odir, "-loracle", "-Wl,-rpath," + odir],
                       check=True, capture_output=True)
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "20000 cases" in r.stdout and " 0 mismatches" in r.stdout
    redrawn = int(re.search(r"(\d+) redrawn", r.stdout).group(1))
    assert redrawn <= 2000, redrawn
    counts = [int(x) for x in re.search(r"(\d+) supersonic, (\d+) reversed, (\d+) supersonic outflow, (\d+) at rest",
                                        r.stdout).groups()]
    assert min(counts) >= 500, counts
