"""Meshes and the float64 yardstick of the large-steps tests (test_smooth.py, test_gpu_smooth.py): the unique-edge combinatorial
Laplacian built from its definition -- a set of sorted vertex pairs -- as a dense matrix, and dense solves.  numpy only; nothing
of epsm_mitsuba3_amd.smooth is used here."""
import numpy as np


def octahedron():
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return np.array(f, np.int32), 6


def grid(nx, ny):
    """An open grid of nx x ny vertices, two triangles per cell."""
    idx = np.arange(nx * ny).reshape(ny, nx)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    return np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32), nx * ny


def fan(n=40):
    """n triangles around vertex 0: a pole of valence n + 1."""
    rim = np.arange(1, n + 1)
    return np.stack([np.zeros(n, np.int64), rim, rim + 1], 1).astype(np.int32), n + 2


def non_manifold():
    """A triangle listed twice and an edge (0, 1) shared by three (four with the repeat) triangles."""
    return np.array([[0, 1, 2], [0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32), 5


def unnamed_vertex():
    """Vertex 4 is in no triangle: degree 0."""
    return np.array([[0, 1, 2], [1, 3, 2]], np.int32), 5


def repeated_corner():
    """A triangle naming vertex 0 twice: its self-edge is ignored, its edge (0, 1) counts."""
    return np.array([[0, 0, 1], [1, 2, 3]], np.int32), 4


MESHES = {
    "octahedron": octahedron(),
    "grid_32x32": grid(32, 32),          # 1024, 1023 and 1025 vertices: the chunk edges of the reductions, with boundary
    "grid_31x33": grid(31, 33),
    "grid_25x41": grid(25, 41),
    "fan_40": fan(40),
    "non_manifold": non_manifold(),
    "unnamed_vertex": unnamed_vertex(),
    "repeated_corner": repeated_corner(),
}
SOLVE_MESHES = ("octahedron", "grid_32x32", "grid_31x33", "grid_25x41", "fan_40")
# 3 072, 6 890 (SMPL's count) and 13 312 vertices: 4, 7 and 13 rows per lane of the one-workgroup solve -- every instantiation
# beyond the two the small meshes reach, the last one full to its limit -- and 3, 7 and 13 chunks of the grid form's reductions.
# Too large for a dense matrix: their yardstick is `sparse_product` / `reference_solve` below.
LARGE = {"grid_48x64": grid(48, 64), "grid_65x106": grid(65, 106), "grid_104x128": grid(104, 128)}


def edge_set(tri):
    """{(v, w), v < w}: every undirected edge some triangle has, once."""
    edges = set()
    for t in np.asarray(tri).tolist():
        for i in range(3):
            v, w = t[i], t[(i + 1) % 3]
            if v != w:
                edges.add((min(v, w), max(v, w)))
    return edges


def neighbour_sets(tri, V):
    rows = [set() for _ in range(V)]
    for v, w in edge_set(tri):
        rows[v].add(w)
        rows[w].add(v)
    return rows


def dense_laplacian(tri, V):
    L = np.zeros((V, V), np.float64)
    for v, w in edge_set(tri):
        L[v, w] = L[w, v] = -1.0
        L[v, v] += 1.0
        L[w, w] += 1.0
    return L


def max_degree(tri, V):
    return max(len(r) for r in neighbour_sets(tri, V))


def dense_matrix(tri, V, lam):
    return np.eye(V) + lam * dense_laplacian(tri, V)


def dense_solve(tri, V, lam, b):
    return np.linalg.solve(dense_matrix(tri, V, lam), np.asarray(b, np.float64))


def rows(V, seed, cols=3):
    """(V, cols) float32 test rows, fixed by the seed."""
    return np.random.default_rng(seed).standard_normal((V, cols)).astype(np.float32)


# -- the yardstick of the LARGE meshes: the same definition, kept as an edge list instead of a dense matrix ---------------------
def edge_array(tri):
    return np.array(sorted(edge_set(tri)), np.int64).reshape(-1, 2)


def sparse_product(tri, V, lam, x, edges=None):
    """(I + lam L) x in float64 from the edge set (`edges`: edge_array(tri), to build it once for many products)."""
    e = edge_array(tri) if edges is None else edges
    x = np.asarray(x, np.float64)
    deg = np.bincount(e.ravel(), minlength=V).astype(np.float64)
    s = np.stack([np.bincount(e[:, 0], x[e[:, 1], c], V) + np.bincount(e[:, 1], x[e[:, 0], c], V) for c in range(x.shape[1])], 1)
    return x + lam * (deg[:, None] * x - s)


def reference_solve(tri, V, lam, b, tol=1e-13):
    """The solution of (I + lam L) x = b in float64 where a dense solve is too heavy: conjugate gradients in numpy on
    `sparse_product`, run until the residual RECOMPUTED from x is below tol |b| per column -- which this function asserts, so
    its own error is kappa tol at the most, nine orders below the bound it is used in."""
    b = np.asarray(b, np.float64)
    edges = edge_array(tri)
    A = lambda v: sparse_product(tri, V, lam, v, edges)
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr, bnorm = (r * r).sum(0), np.sqrt((b * b).sum(0))
    for _ in range(20 * V):
        if (np.sqrt(rr) <= 0.1 * tol * bnorm).all():
            break
        q = A(p)
        alpha = rr / (p * q).sum(0)
        x += alpha * p
        r -= alpha * q
        rr_new = (r * r).sum(0)
        p = r + (rr_new / rr) * p
        rr = rr_new
    assert (np.linalg.norm(b - A(x), axis=0) <= tol * bnorm).all()
    return x
