"""The closed statement of the hull simplification (include/pnr_hull.h) in numpy, parametrised by the number format, and the chain that
follows the reference's lines with scipy: what palettenerf_amd.extract.simplify_hull and csrc/hull.hip are tested against
(tests/test_hull_host.py, tests/test_gpu_hull.py).

    simplify(centers, weights, dtype=np.longdouble)   the statement: brute-force hulls, every LP by vertex enumeration.  The TRUTH.
    simplify(..., dtype=np.float64)                   the same operations in float64: what the kernel's integers are compared with at sizes the
                                                      longdouble instance is too slow for
    host(name)                                        Hull_Simplification_posternerf in its line order with scipy.spatial.ConvexHull and
                                                      scipy.optimize.linprog(method="highs") (the reference's cvxopt/GLPK does not import here):
                                                      extract.simplify_hull_per_op, the float64 host formulation whose distance from the truth is E

The fixtures are this repository's own numbers, from fixed recipes."""
import functools
import itertools
import os

import numpy as np

from palettenerf_amd import extract
from tests.lut_reference import closest_on_triangle, cross, dot, require_longdouble  # noqa: F401  (re-exported)

PLANE_EPS, OUTSIDE_EPS, DET_EPS, FEAS_EPS = 1e-9, 1e-8, 1e-12, 1e-9
OK, COPLANAR, FLAT, DENSE = 0, 1, 2, 3
STOP_NONE, STOP_ERROR, STOP_TARGET, STOP_UNCHANGED, STOP_FOUR = 0, 1, 2, 3, 4
HULL_STOPS = ["none", "error", "target", "unchanged", "four"]
MIN_PLANE_MARGIN, MIN_COST_GAP, MIN_ERROR_MARGIN = 1e-7, 1e-6, 1e-6


class Refused(Exception):
    def __init__(self, status, related=0):
        super().__init__({COPLANAR: "coplanar", FLAT: "flat", DENSE: "dense"}[status])
        self.status, self.related = status, related


# ---------------------------------------------------------------- fixtures
def mix(seed, K):
    rng = np.random.default_rng(seed)
    a = rng.uniform(.03, .97, (K // 2, 3))
    b = (rng.uniform(.1, .9, (1, 3)) + .15 * rng.standard_normal((K - K // 2, 3))).clip(.02, .98)
    return np.concatenate([a, b]), rng.integers(1, 10 ** 6, K).astype(np.float64)


def shell(seed, K=64):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((K, 3))
    pts = 0.5 + 0.45 * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(.9, 1, (K, 1))
    return pts, rng.integers(1, 10 ** 6, K).astype(np.float64)


def tiny(seed, K):
    return np.random.default_rng(seed).uniform(.05, .95, (K, 3)), np.ones(K)


FIXTURES = {"mix-1-24": lambda: mix(1, 24), "mix-2-44": lambda: mix(2, 44), **{f"mix-{s}-40": (lambda s=s: mix(s, 40)) for s in range(3, 9)},
            "shell-11": lambda: shell(11), "tiny-20-4": lambda: tiny(20, 4), "tiny-21-5": lambda: tiny(21, 5), "tiny-22-6": lambda: tiny(22, 6),
            "tiny-23-8": lambda: tiny(23, 8)}
NAMES = list(FIXTURES)
# what the issue recorded for them: (initial hull vertices, returned colours)
EXPECTED = {"mix-3-40": (25, 11), "mix-4-40": (21, 8), "mix-5-40": (14, 7), "mix-6-40": (16, 8), "mix-7-40": (16, 9), "mix-8-40": (18, 8),
            "mix-1-24": (15, 9), "mix-2-44": (22, 6), "shell-11": (55, 7), "tiny-20-4": (4, 4), "tiny-21-5": (5, 5), "tiny-22-6": (5, None),
            "tiny-23-8": (7, 6)}


@functools.lru_cache(maxsize=None)
def fixture(name):
    c, w = FIXTURES[name]()
    c.setflags(write=False)
    w.setflags(write=False)
    return c, w


# ---------------------------------------------------------------- the statement
@functools.lru_cache(maxsize=None)
def _triples(n):
    return np.array(list(itertools.combinations(range(n), 3)), dtype=np.int64).reshape(-1, 3)


def hull(P, margins=None):
    """The strict hull of the point set P [n,3]: (vertex rows of P ascending [V], faces [F,3] ascending triples in VERTEX numbering, unit outward
    normals [F,3]).  Refused(FLAT / COPLANAR).  margins: a list that receives the distance of every deciding plane test from its threshold."""
    n = P.shape[0]
    eps = P.dtype.type(PLANE_EPS)
    faces, normals, off_plane, fourth = [], [], False, False
    T = _triples(n)
    for lo in range(0, len(T), 1 << 15):
        t = T[lo:lo + (1 << 15)]
        a = P[t[:, 0]]
        nrm = cross(P[t[:, 1]] - a, P[t[:, 2]] - a)
        len2 = dot(nrm, nrm)
        ok = len2 > 0
        unit = nrm / np.sqrt(np.where(ok, len2, 1))[:, None]
        d = (unit[:, None, 0] * (P[None, :, 0] - a[:, None, 0]) + unit[:, None, 1] * (P[None, :, 1] - a[:, None, 1])) \
            + unit[:, None, 2] * (P[None, :, 2] - a[:, None, 2])
        own = np.zeros(d.shape, dtype=bool)
        own[np.arange(len(t))[:, None], t] = True
        front, behind = (d > eps) & ~own, (d < -eps) & ~own
        pos, neg = front.any(axis=1), behind.any(axis=1)
        near = (~front & ~behind & ~own).any(axis=1)
        off_plane |= bool((ok & (pos | neg)).any())
        fourth |= bool((ok & (pos ^ neg) & near).any())
        take = ok & (pos ^ neg) & ~near
        if margins is not None and n > 3:
            dm = np.where(own, np.nan, d)
            two_sided = ok & pos & neg          # stays two-sided as long as its extreme points stay off the plane
            if two_sided.any():
                margins.append(float(np.min(np.minimum(np.nanmax(dm[two_sided], axis=1) - eps, -eps - np.nanmin(dm[two_sided], axis=1)))))
            rest = ok & ~two_sided
            if rest.any():
                margins.append(float(np.nanmin(np.minimum(np.abs(dm[rest] - eps), np.abs(dm[rest] + eps)))))
        for i in np.nonzero(take)[0]:
            faces.append(t[i])
            normals.append(-unit[i] if pos[i] else unit[i])
    if not off_plane:
        raise Refused(FLAT)
    if fourth or len(faces) < 4:
        raise Refused(COPLANAR if fourth else FLAT)
    faces = np.array(faces)
    verts = np.unique(faces)
    renum = np.full(n, -1)
    renum[verts] = np.arange(len(verts))
    return verts, renum[faces], np.array(normals)


def lp_vertex(N, b, c):
    """min c.x s.t. N x >= b by vertex enumeration: (x or None, feasible vertices)."""
    m = N.shape[0]
    t = _triples(m)
    A, B, C = N[t[:, 0]], N[t[:, 1]], N[t[:, 2]]
    bc, ca, ab = cross(B, C), cross(C, A), cross(A, B)
    det = dot(A, bc)
    ok = np.abs(det) > det.dtype.type(DET_EPS)
    safe = np.where(ok, det, 1)
    x = (b[t[:, 0], None] * bc + b[t[:, 1], None] * ca + b[t[:, 2], None] * ab) / safe[:, None]
    slack = ((x[:, None, 0] * N[None, :, 0] + x[:, None, 1] * N[None, :, 1]) + x[:, None, 2] * N[None, :, 2]) - b[None, :]
    feas = ok & (slack >= -det.dtype.type(FEAS_EPS)).all(axis=1)
    if not feas.any():
        return None, 0
    obj = np.where(feas, dot(c[None, :], x), np.inf)
    return x[int(np.argmin(obj))], int(feas.sum())       # argmin: the first of equal minima, the lowest triple


def edges_of(faces):
    return sorted({(int(min(u, v)), int(max(u, v))) for f in faces for u, v in ((f[0], f[1]), (f[0], f[2]), (f[1], f[2]))})


def collapse(V, faces, normals, dense_cap=None, gaps=None):
    """One collapse of the vertex set V with its hull: (v1, v2, x, candidates, largest related-face count) or (None, None, None, 0, largest)."""
    raw = cross(V[faces[:, 1]] - V[faces[:, 0]], V[faces[:, 2]] - V[faces[:, 0]])
    raw = np.where((dot(raw, normals) < 0)[:, None], -raw, raw)           # outward, like the unit normals
    b_all = dot(normals, V[faces[:, 0]])
    best, costs, cands = None, [], 0
    edges = edges_of(faces)
    most = max(int(((faces == v1) | (faces == v2)).any(axis=1).sum()) for v1, v2 in edges)
    if dense_cap is not None and most > dense_cap:
        raise Refused(DENSE, most)
    for v1, v2 in edges:
        rel = np.nonzero(((faces == v1) | (faces == v2)).any(axis=1))[0]
        N, b = normals[rel], b_all[rel]
        c = np.zeros(3, dtype=V.dtype)
        for row in N:
            c = c + row
        x, _ = lp_vertex(N, b, c)
        if x is None:
            continue
        cands += 1
        cost = V.dtype.type(0)
        for r in rel:
            cost = cost + np.abs(dot(raw[r], x - V[faces[r, 0]])) / 6
        costs.append(float(cost))
        if best is None or cost < best[0]:
            best = (cost, v1, v2, x)
    if best is None:
        return None, None, None, 0, most
    if gaps is not None and len(costs) > 1:
        s = sorted(costs)
        gaps.append((s[1] - s[0]) / s[1])
    return best[1], best[2], best[3], cands, most


def reconstruction_error(Q, centers, weights, margins=None):
    """sqrt(sum over the outside centres of w d^2 / sum of all w) against the clipped vertex set Q; None is the reference's `fail`."""
    n = Q.shape[0]
    eps, rule = Q.dtype.type(PLANE_EPS), Q.dtype.type(OUTSIDE_EPS)
    tris, normals = [], []
    for i, j, k in _triples(n):
        nrm = cross(Q[j] - Q[i], Q[k] - Q[i])
        length = np.sqrt(dot(nrm, nrm))
        if not length > Q.dtype.type(1e-12):
            continue
        unit = nrm / length
        d = np.array([dot(unit, Q[l] - Q[i]) for l in range(n) if l not in (i, j, k)], dtype=Q.dtype)
        front, behind = bool((d > eps).any()), bool((d < -eps).any())
        if front == behind:                     # two-sided, or nothing off the plane
            continue
        tris.append((i, j, k))
        normals.append(-unit if front else unit)
    if not tris:
        return None
    tris, normals = np.array(tris), np.array(normals)
    X = centers.astype(Q.dtype)
    far = np.max(np.stack([dot(normals[f][None], X - Q[tris[f, 0]]) for f in range(len(tris))], axis=1), axis=1)
    if margins is not None:
        margins.append(float(np.min(np.abs(far - rule))))
    outside = far > rule
    total = Q.dtype.type(0)
    if outside.any():
        xo = X[outside]
        best = None
        for i, j, k in tris:
            q = closest_on_triangle(xo, Q[i], Q[j], Q[k])
            sq = dot(xo - q, xo - q)
            best = sq if best is None else np.minimum(best, sq)
        for wd in weights.astype(Q.dtype)[outside] * best:
            total = total + wd
    wsum = Q.dtype.type(0)
    for w in weights.astype(Q.dtype):
        wsum = wsum + w
    return np.sqrt(total / wsum)


def simplify(centers, weights, error_thres=5 / 255, target_size=None, dtype=np.longdouble, dense_cap=None, check_margins=False):
    """The statement.  Returns a dict: status, palette [M,3] (clipped; on a refusal the unclipped vertex set the iteration in progress started
    from, or the centres when the first hull is refused), M, collapses, initial (the first hull's vertices), stop, related (the largest
    related-face count), errors {V: error}, trace [(v1, v2, V after, candidates)], and with check_margins the three margins of the fixture rules."""
    P = np.asarray(centers, dtype=np.float64).astype(dtype)
    w = np.asarray(weights, dtype=np.float64)
    K = P.shape[0]
    planes, gaps, errs = ([], [], []) if check_margins else (None, None, None)
    out = {"status": OK, "collapses": 0, "initial": 0, "stop": STOP_NONE, "related": 0, "errors": {}, "trace": []}

    def done(Vset, stop, clip=True):
        out.update(palette=np.clip(Vset, 0, 1) if clip else Vset, M=Vset.shape[0], stop=stop)
        if check_margins:
            out.update(plane_margin=min(planes, default=np.inf), cost_gap=min(gaps, default=np.inf), error_margin=min(errs, default=np.inf))
        return out

    def refused(e, Vset):
        out["status"] = e.status
        out["related"] = max(out["related"], e.related)
        return done(Vset, STOP_NONE, clip=False)

    try:
        verts, faces, normals = hull(P, planes)
    except Refused as e:
        return refused(e, P)
    V = P[verts]
    out["initial"] = V.shape[0]
    for _ in range(max(K - 3, 1)):
        old = V
        try:
            v1, v2, x, cands, most = collapse(V, faces, normals, dense_cap, gaps)
        except Refused as e:
            return refused(e, old)
        out["related"] = max(out["related"], most)
        if x is not None:
            keep = [i for i in range(V.shape[0]) if i not in (v1, v2)]
            try:
                verts, faces, normals = hull(np.concatenate([V[keep], x[None]]), planes)
            except Refused as e:
                return refused(e, old)
            V = np.concatenate([V[keep], x[None]])[verts]
            out["collapses"] += 1
            out["trace"].append((v1, v2, V.shape[0], cands))
        n = V.shape[0]
        if n <= 10:
            if target_size is None:
                err = reconstruction_error(np.clip(V, 0, 1), P, w)
                out["errors"][n] = None if err is None else float(err)
                if err is not None and check_margins:
                    errs.append(abs(float(err) - error_thres))
                if err is None or err > error_thres:
                    return done(old, STOP_ERROR)
            elif n == target_size:
                return done(V, STOP_TARGET)
        if n == old.shape[0] or n == 4:
            return done(V, STOP_UNCHANGED if n == old.shape[0] else STOP_FOUR)
    raise AssertionError("more than K - 4 collapses")


@functools.lru_cache(maxsize=None)
def truth(name):
    """The longdouble truth of a fixture with its margins, formed once a process and shared.  Treat as read-only."""
    require_longdouble()
    c, w = fixture(name)
    return simplify(c, w, dtype=np.longdouble, check_margins=True)


@functools.lru_cache(maxsize=None)
def host(name):
    """The float64 host formulation (scipy / HiGHS) of a fixture: (palette, info)."""
    c, w = fixture(name)
    return extract.simplify_hull_per_op(c, w, return_info=True)


@functools.lru_cache(maxsize=None)
def fixture_E():
    """E: the largest distance of the host formulation's palette from the truth's over ALL fixtures the statement answers (one figure; a
    fixture it refuses has no truth to be distant from)."""
    worst = 0.0
    for name in NAMES:
        t, (p, _) = truth(name), host(name)
        if t["status"] != OK:
            continue
        assert p.shape == t["palette"].shape, name
        worst = max(worst, float(np.max(np.abs(p - t["palette"]))))
    return worst


def shell128():
    """The largest launch: 128 shell points (the recipe of shell, seed 12)."""
    return shell(12, 128)


SHELL128 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hull_shell128_host.npz")


def save_shell128(palette, info):
    """Record the host formulation's run on shell128() (extract.simplify_hull_per_op(*shell128(), return_info=True): about two minutes of
    HiGHS calls, too long for a test): the trace and the figures tests/test_gpu_hull.py compares the largest launch with."""
    np.savez(SHELL128, palette=palette, trace=np.array(info["trace"], dtype=np.int32), initial=info["initial"], related=info["related"],
             stop=HULL_STOPS.index(info["stop"]), error_sizes=np.array(list(info["errors"]), dtype=np.int32),
             errors=np.array(list(info["errors"].values()), dtype=np.float64))


def load_shell128():
    with np.load(SHELL128) as z:
        return {"palette": z["palette"], "trace": [tuple(int(v) for v in row) for row in z["trace"]], "initial": int(z["initial"]),
                "related": int(z["related"]), "stop": int(z["stop"]), "errors": dict(zip(z["error_sizes"].tolist(), z["errors"].tolist()))}


# ---------------------------------------------------------------- the cases of the hand-overs and of the dropped interior centres
def coplanar_case():
    """mix(9, 36) and four centres in the last layer of the fine grid, r = 31.5 / 32: hull vertices on one plane."""
    c, w = mix(9, 36)
    layer = np.array([[31.5 / 32, y, z] for y in (4.5 / 32, 27.5 / 32) for z in (5.5 / 32, 26.5 / 32)])
    return np.concatenate([c, layer]), np.concatenate([w, [7.0, 5.0, 3.0, 2.0]])


def flat_case():
    rng = np.random.default_rng(31)
    c = rng.uniform(.1, .9, (12, 3))
    c[:, 2] = 0.375
    return c, np.ones(12)


def dense_case(ring=70):
    """Two apexes over a ring of `ring` points, alternately 1e-4 above and below its plane: every ring point is joined to both apexes, so an
    edge at an apex has ring + 2 related faces, more than PNR_HULL_MAX_RELATED."""
    th = 2 * np.pi * (np.arange(ring) + 0.25) / ring
    pts = np.stack([0.5 + 0.4 * np.cos(th), 0.5 + 0.4 * np.sin(th), 0.5 + 1e-4 * (-1.0) ** np.arange(ring)], axis=1)
    c = np.concatenate([pts, [[0.5, 0.5, 0.95], [0.5, 0.5, 0.05]]])
    return c, np.arange(1, ring + 3, dtype=np.float64)


def interior_case():
    """tiny(23, 8) and twelve convex combinations of its points, shuffled in: the hull, and with it every collapse, is that of the 8 alone."""
    c, _ = tiny(23, 8)
    rng = np.random.default_rng(41)
    inner = (rng.dirichlet(np.ones(8), size=12) * 0.8 + 0.2 / 8) @ c
    order = rng.permutation(20)
    return np.concatenate([c, inner])[order], rng.integers(1, 100, 20).astype(np.float64), order
