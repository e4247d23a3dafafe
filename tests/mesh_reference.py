"""A plain numpy statement of the mesh export's conventions (include/pnr.h, "mesh export"), and the checks a closed mesh must pass.  Not a test.

The case table is read through pnr_mesh_case_triangles: the very table the kernel uses.  Everything else -- corner and edge numbering, the
vertex formula, the vertex and triangle order, the lattice formula -- is restated here from the contract, not taken from the kernels."""
import ctypes

import numpy as np

from palettenerf_amd import _lib


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_geometry():
    """edge e = axis * 4 + k -> (axis, offset of the edge's low end inside the cell); k: the other two axes' offsets, lower axis in bit 0."""
    out = []
    for axis in range(3):
        others = [d for d in range(3) if d != axis]
        for k in range(4):
            base = np.zeros(3, int)
            base[others[0]], base[others[1]] = k & 1, k >> 1
            out.append((axis, base))
    return out


EDGES = edge_geometry()


def edge_corners(e):
    axis, base = EDGES[e]
    far = base.copy()
    far[axis] = 1
    return int(base @ [1, 2, 4]), int(far @ [1, 2, 4])


def case_table():
    """[256] lists of (e0, e1, e2) from the library."""
    lib = _lib.load()
    tab = []
    for c in range(256):
        edges = (ctypes.c_uint8 * 15)()
        n = lib.pnr_mesh_case_triangles(c, edges)
        assert 0 <= n <= 5, (c, n)
        assert all(v == 255 for v in edges[3 * n:]), c
        tab.append([tuple(edges[3 * k:3 * k + 3]) for k in range(n)])
    return tab


def lattice_axis(lo, hi, n):
    """Coordinate i of n on [lo, hi] in fp32: the two-sided form, a product and a sum, each rounded."""
    lo, hi = np.float32(lo), np.float32(hi)
    step = np.float32((hi - lo) / np.float32(n - 1))
    i = np.arange(n)
    up = (lo + (step * i.astype(np.float32)).astype(np.float32)).astype(np.float32)
    down = (hi - (step * (n - 1 - i).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return np.where(i < n // 2, up, down).astype(np.float32)


def lattice(lo, hi, n):
    """All lattice points in C order, z fastest: [nx * ny * nz, 3] fp32."""
    ax = [lattice_axis(lo[d], hi[d], n[d]) for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)


def marching_cubes(u, threshold, table=None):
    """(vertices [nv, 3] fp32 in lattice-index coordinates, triangles [nt, 3] int32) of the contract, in its order."""
    table = table or case_table()
    u = np.asarray(u, np.float32)
    thr = np.float32(threshold)
    R = u.shape
    with np.errstate(invalid="ignore"):
        ins = u > thr                                   # strict; NaN is outside
    strad = np.zeros(R + (3,), bool)
    for a in range(3):
        s0, s1 = [slice(None)] * 3, [slice(None)] * 3
        s0[a], s1[a] = slice(0, -1), slice(1, None)
        strad[tuple(s0) + (a,)] = ins[tuple(s0)] != ins[tuple(s1)]
    flat = np.flatnonzero(strad.ravel())               # ascending ((x ny + y) nz + z) * 3 + axis
    ids = -np.ones(strad.size, np.int64)
    ids[flat] = np.arange(flat.size)
    ids = ids.reshape(strad.shape)
    idx = np.stack(np.unravel_index(flat, strad.shape), 1) if flat.size else np.zeros((0, 4), np.int64)
    p0, a = idx[:, :3], idx[:, 3]
    p1 = p0.copy()
    p1[np.arange(len(a)), a] += 1
    u0, u1 = u[tuple(p0.T)], u[tuple(p1.T)]
    with np.errstate(all="ignore"):
        t = ((thr - u0).astype(np.float32) / (u1 - u0).astype(np.float32)).astype(np.float32)
    t = np.where(np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
    t = np.clip(t, np.float32(0), np.float32(1)).astype(np.float32)
    V = p0.astype(np.float32)
    V[np.arange(len(a)), a] = (V[np.arange(len(a)), a] + t).astype(np.float32)
    case = np.zeros(tuple(r - 1 for r in R), np.int64)
    for c in range(8):
        x, y, z = corner_xyz(c)
        case |= ins[x:R[0] - 1 + x, y:R[1] - 1 + y, z:R[2] - 1 + z].astype(np.int64) << c
    T = []
    for i, j, k in zip(*np.nonzero((case != 0) & (case != 255))):      # C order
        for tri in table[case[i, j, k]]:
            row = []
            for e in tri:
                axis, base = EDGES[e]
                row.append(ids[i + base[0], j + base[1], k + base[2], axis])
            T.append(row)
    T = np.array(T, np.int64).reshape(-1, 3)
    assert (T >= 0).all()
    return V, T.astype(np.int32)


def directed_edges(T):
    T = np.asarray(T, np.int64)
    return np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])


def mesh_report(V, T):
    """The properties of a mesh the tests assert on."""
    V, T = np.asarray(V), np.asarray(T, np.int64)
    he = directed_edges(T)
    key = he[:, 0] * (len(V) + 1) + he[:, 1]
    rkey = he[:, 1] * (len(V) + 1) + he[:, 0]
    a, b, c = (V[T[:, k]].astype(np.float64) for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return {
        "duplicate_directed_edges": int(len(key) - len(np.unique(key))),
        "unmatched_directed_edges": int((np.sort(key) != np.sort(rkey)).sum()),      # the multiset of edges vs the multiset of their reverses
        "euler": int(len(np.unique(T)) - len(np.unique(np.sort(he, 1), axis=0)) + len(T)),
        "volume": float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6),         # signed: positive when normals point outwards
        "zero_area": int((area == 0).sum()),
        "all_vertices_used": bool(len(np.unique(T)) == len(V)),
    }


def assert_closed(V, T, euler=None):
    r = mesh_report(V, T)
    assert r["duplicate_directed_edges"] == 0 and r["unmatched_directed_edges"] == 0, r
    assert r["zero_area"] == 0 and r["all_vertices_used"], r
    if euler is not None:
        assert r["euler"] == euler, r
    return r
