"""Meshes of the periodic-boundary tests, written as Gmsh-2 text from numpy: a box P whose interior points are
jittered, and its tx x ty tiling T with the same jitter in every tile and the seam points shared. The residual of
a periodic P must equal the single-domain residual of T at the centre tile (tests/test_gpu_periodic.py).

kind: "quad", "tri" (every quadrangle split, the diagonal alternating with the parity of i + j) or "hybrid" (lower
half of the rows quadrangles, upper half triangles). Cells are numbered row by row, the tile's cells in the same
relative order in P and in every tile of T."""
import numpy as np


def _tile_points(nx, ny, lx, ly, jitter, seed):
    """offsets [ny][nx][2] of the tile's points (i < nx, j < ny): zero on the tile's seam (i == 0 or j == 0)"""
    rng = np.random.default_rng(seed)
    d = jitter * min(lx / nx, ly / ny) * rng.uniform(-1.0, 1.0, (ny, nx, 2))
    d[0, :, :] = 0.0
    d[:, 0, :] = 0.0
    return d


def _cells_of(i, j, ny, kind):
    """node patterns of quadrangle (i, j) as indices into its corners (a, b, c, d) counter-clockwise"""
    tri = kind == "tri" or (kind == "hybrid" and j >= ny // 2)
    if not tri:
        return [(0, 1, 2, 3)]
    return [(0, 1, 2), (0, 2, 3)] if (i + j) % 2 == 0 else [(0, 1, 3), (1, 2, 3)]


def write_tiling(path, nx, ny, kind="quad", tx=1, ty=1, lx=1.0, ly=1.0, jitter=0.2, seed=7,
                 markers=(5, 4, 5, 4)):
    """writes the tx x ty tiling of the nx x ny box; markers of the (bottom, right, top, left) sides. Returns
    (tile [ncell][2] = the tile (ix, iy) of each cell, local [ncell] = its cell number within the tile)"""
    if kind != "quad":
        assert nx % 2 == 0 and ny % 2 == 0        # the diagonals' parity must repeat from tile to tile
    d = _tile_points(nx, ny, lx, ly, jitter, seed)
    NX, NY = tx * nx, ty * ny
    hx, hy = lx / nx, ly / ny

    def P(i, j):
        return j * (NX + 1) + i
    pts = np.zeros(((NX + 1) * (NY + 1), 2))
    for j in range(NY + 1):
        for i in range(NX + 1):
            off = d[j % ny, i % nx] if 0 < i < NX and 0 < j < NY else (0.0, 0.0)
            # the tile's own coordinate plus the tile's origin: every tile's points differ by whole periods
            pts[P(i, j)] = ((i % nx) * hx + off[0] + (i // nx) * lx, (j % ny) * hy + off[1] + (j // ny) * ly)
    start = {}
    n = 0
    for j in range(ny):
        for i in range(nx):
            start[(i, j)] = n
            n += len(_cells_of(i, j, ny, kind))
    cells, tile, local = [], [], []
    for j in range(NY):
        for i in range(NX):
            corners = (P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1))
            for k, pat in enumerate(_cells_of(i % nx, j % ny, ny, kind)):
                cells.append([corners[q] for q in pat])
                tile.append((i // nx, j // ny))
                local.append(start[(i % nx, j % ny)] + k)
    edges = [(P(i, 0), P(i + 1, 0), markers[0]) for i in range(NX)]
    edges += [(P(NX, j), P(NX, j + 1), markers[1]) for j in range(NY)]
    edges += [(P(i, NY), P(i - 1, NY), markers[2]) for i in range(NX, 0, -1)]
    edges += [(P(0, j), P(0, j - 1), markers[3]) for j in range(NY, 0, -1)]
    out = ["$MeshFormat", "2.2 0 8", "$EndMeshFormat", "$Nodes", str(len(pts))]
    out += ["%d %r %r 0" % (k + 1, float(x), float(y)) for k, (x, y) in enumerate(pts)]
    out += ["$EndNodes", "$Elements", str(len(edges) + len(cells))]
    eid = 1
    for a, b, tag in edges:
        out.append("%d 1 2 %d 1 %d %d" % (eid, tag, a + 1, b + 1))
        eid += 1
    for c in cells:
        out.append("%d %d 2 1 1 %s" % (eid, 2 if len(c) == 3 else 3, " ".join(str(q + 1) for q in c)))
        eid += 1
    out.append("$EndElements")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return np.array(tile, np.int64), np.array(local, np.int64)


def smooth_state(rc, p, lx=1.0, ly=1.0, seed=3, amp=0.05, wrap_y=True):
    """free stream times 1 + amp waves of integer wavenumbers over the box (periodic in x, and in y if wrap_y)"""
    rng = np.random.default_rng(seed)
    x, y = rc[:, 0] / lx, rc[:, 1] / ly
    g, M, a = p.gamma, p.Minf, p.aoa
    pinf = 1.0 / (g * M * M)

    def wave():
        k = rng.integers(1, 3, size=2)
        ph = rng.random(2)
        wy = np.cos(2 * np.pi * (k[1] * y + ph[1])) if wrap_y else 1.0 + 0.5 * y
        return np.sin(2 * np.pi * (k[0] * x + ph[0])) * wy
    rho = 1.0 + amp * wave()
    pr = pinf * (1 + amp * wave())
    vx = np.cos(a) + amp * wave()
    vy = np.sin(a) + amp * wave()
    u = np.empty((rc.shape[0], 4))
    u[:, 0] = rho
    u[:, 1] = rho * vx
    u[:, 2] = rho * vy
    u[:, 3] = pr / (g - 1.0) + 0.5 * rho * (vx * vx + vy * vy)
    return np.ascontiguousarray(u)
