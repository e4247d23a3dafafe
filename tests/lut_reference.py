"""The closed statement of the palette weight LUT (include/pnr.h, "palette extraction, weight LUT") in numpy, parametrised by the number format:
what palettenerf_amd.extract.weight_lut / palette_weights and csrc/lut.hip are tested against (tests/test_lut_host.py, tests/test_gpu_lut.py).
No scipy.  The np.longdouble instance with the barycentrics by Cramer's rule is the TRUTH; the float64 instance (barycentrics through
np.linalg.inv) is one of the two float64 formulations whose distance from the truth is a fixture's E.

The palette in hull order (L1 distance to black, a tie to the lower row); the hull by brute force (a triple is a face when every other row
is on one side of its plane by more than 1e-9); a point is outside when its signed distance to a face plane exceeds 1e-8 and is then
replaced by the nearest of the closest points on the triangles; its weights are the barycentric coordinates in the star tetrahedron
(V[0], Vi, Vj, Vk) whose smallest coordinate is largest; the columns go back to the caller's order.

The fixtures are this repository's own numbers."""
import functools
import itertools

import numpy as np

P6 = np.array([[.05, .04, .06], [.93, .95, .90], [.80, .12, .10], [.15, .60, .20], [.10, .20, .85], [.95, .80, .15]], dtype=np.float64)
P4 = P6[[0, 2, 3, 4]]
P8 = np.concatenate([P6, np.array([[.9, .2, .8], [.1, .85, .9]], dtype=np.float64)])
PALETTES = {"P4": P4, "P6": P6, "P8": P8}
FIXTURES = [(name, norm) for name in PALETTES for norm in (False, True)]
FIXTURE_IDS = [f"{name}-{'normalised' if norm else 'plain'}" for name, norm in FIXTURES]
MIN_MARGIN = 1e-7          # every fixture point is at least this far from the inside/outside decision (the rule is 1e-8)


def require_longdouble():
    """The truth needs a format finer than float64: fail, never pass vacuously."""
    eps = np.finfo(np.longdouble).eps
    assert eps < 1e-18, f"np.longdouble has eps = {eps}: no format finer than float64 here, the truth of the LUT tests cannot be formed"


def bin_points(normalize):
    """The 32 768 five-bit bin centres as float64 (exact), r most significant; normalised: (c + 0.05) / |c + 0.05| in float64."""
    code = np.arange(32768)
    c = (np.stack([(code >> 10) & 31, (code >> 5) & 31, code & 31], axis=1).astype(np.float64) + 0.5) / 32.0
    return normalised(c) if normalize else c


def normalised(c):
    c = np.asarray(c, dtype=np.float64) + 0.05
    return c / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])[:, None]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def hull_order(palette):
    p = np.asarray(palette, dtype=np.float64)
    return np.argsort((np.abs(p[:, 0]) + np.abs(p[:, 1])) + np.abs(p[:, 2]), kind="stable")


def hull_faces(V):
    """faces (ascending triples of V) and their outward unit normals, in V's number format.  ValueError("flat") / ValueError("coplanar")."""
    eps = V.dtype.type(1e-9)
    M = V.shape[0]
    faces, normals, off_plane, fourth = [], [], False, False
    for i, j, k in itertools.combinations(range(M), 3):
        n = cross(V[j] - V[i], V[k] - V[i])
        length = np.sqrt(dot(n, n))
        if not length > 0:
            continue
        n = n / length
        d = np.array([dot(n, V[l] - V[i]) for l in range(M) if l not in (i, j, k)])
        front, behind = d > eps, d < -eps
        if not (front.any() or behind.any()):
            continue
        off_plane = True
        if front.any() and behind.any():
            continue
        if not (front | behind).all():
            fourth = True
            continue
        faces.append((i, j, k))
        normals.append(-n if front.any() else n)
    if not off_plane:
        raise ValueError("flat")
    if fourth:
        raise ValueError("coplanar")
    assert len(faces) >= 4
    return np.array(faces), np.array(normals)


def closest_on_triangle(p, a, b, c):
    """The closest point of triangle abc to every row of p [N,3]: the seven Voronoi regions of the triangle (Ericson, Real-Time Collision
    Detection, 5.1.5), later rules yielding to earlier ones."""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        s = va + vb + vc
        out = a + ab * (vb / s)[:, None] + ac * (vc / s)[:, None]
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        out = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], b + (c - b) * t[:, None], out)
        out = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], a + ac * (d2 / (d2 - d6))[:, None], out)
        out = np.where(((d6 >= 0) & (d5 <= d6))[:, None], c, out)
        out = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], a + ab * (d1 / (d1 - d3))[:, None], out)
        out = np.where(((d3 >= 0) & (d4 <= d3))[:, None], b, out)
        out = np.where(((d1 <= 0) & (d2 <= 0))[:, None], a, out)
    return out


def det3(c0, c1, c2):
    return dot(c0, cross(c1, c2))


def weights(points, palette, dtype=np.float64, cramer=False):
    """(W [N,M] in dtype, info): info["outside"] [N], info["projected"] [N,3], info["margin"] (the smallest distance of a point's largest
    signed plane distance from the 1e-8 rule), info["faces"], info["order"], info["hull_vertices"] (caller's rows)."""
    order = hull_order(palette)
    V = np.asarray(palette, dtype=np.float64)[order].astype(dtype)
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(dtype)
    faces, normals = hull_faces(V)
    rule = dtype(1e-8)
    far = np.max(np.stack([dot(normals[f], x - V[faces[f, 0]]) for f in range(len(faces))], axis=1), axis=1)
    outside = far > rule
    if outside.any():
        xo = x[outside]
        best, best_d = None, None
        for i, j, k in faces:
            q = closest_on_triangle(xo, V[i], V[j], V[k])
            d = dot(xo - q, xo - q)
            if best is None:
                best, best_d = q, d
            else:
                closer = d < best_d
                best, best_d = np.where(closer[:, None], q, best), np.where(closer, d, best_d)
        x[outside] = best
    N, M = x.shape[0], V.shape[0]
    W = np.zeros((N, M), dtype=dtype)
    best_min = np.full(N, -np.inf, dtype=dtype)
    y = x - V[0]
    for i, j, k in faces:
        if i == 0:
            continue
        c = [V[i] - V[0], V[j] - V[0], V[k] - V[0]]
        if cramer:
            det = det3(*c)
            b = [det3(y, c[1], c[2]) / det, det3(c[0], y, c[2]) / det, det3(c[0], c[1], y) / det]
        else:
            inv = np.linalg.inv(np.stack(c, axis=1))
            b = list((y @ inv.T).T)
        b0 = 1 - (b[0] + b[1] + b[2])
        smallest = np.minimum(np.minimum(b0, b[0]), np.minimum(b[1], b[2]))
        take = smallest > best_min
        best_min = np.where(take, smallest, best_min)
        row = np.zeros((N, M), dtype=dtype)
        row[:, order[0]], row[:, order[i]], row[:, order[j]], row[:, order[k]] = b0, b[0], b[1], b[2]
        W = np.where(take[:, None], row, W)
    info = {"outside": outside, "projected": x, "margin": float(np.min(np.abs(far - rule))), "faces": faces, "order": order,
            "hull_vertices": sorted(int(order[v]) for v in set(faces.ravel().tolist()))}
    return W, info


@functools.lru_cache(maxsize=None)
def truth(name, normalize):
    """The longdouble truth of a fixture, formed once a process and shared: (W [32768,M] longdouble, info).  Treat as read-only."""
    require_longdouble()
    W, info = weights(bin_points(normalize), PALETTES[name], dtype=np.longdouble, cramer=True)
    assert info["margin"] >= MIN_MARGIN, f"bad fixture {name}: a bin within {info['margin']} of the inside/outside rule"
    W.setflags(write=False)
    return W, info


@functools.lru_cache(maxsize=None)
def float64_formulation(name, normalize):
    W, info = weights(bin_points(normalize), PALETTES[name], dtype=np.float64, cramer=False)
    W.setflags(write=False)
    return W, info
