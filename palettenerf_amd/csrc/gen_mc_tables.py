#!/usr/bin/env python3
"""Generate mc_tables.inc: the 256-case triangle table of marching cubes (csrc/mesh.hip).

Nothing is typed in: every case is derived from the cube's geometry by the rule below, so the table can be regenerated and audited.

Conventions (the ones tests/mesh_reference.py restates):
  corner  c = x + 2 y + 4 z                 (bit 0 = x, as the grid encoder numbers a cell's corners)
  edge    e = axis * 4 + k                  k = the offsets of the two OTHER axes, in increasing axis order, as two bits (bit 0 = the lower axis)
  case    bit c set  <=>  u[corner c] > threshold      (strict; NaN is outside)

Rule, per case:
  * on each of the six faces the straddling edges are joined by segments: two crossings give one segment; four crossings (the inside corners
    sit on a diagonal) cut off each inside corner on its own -- the same choice on both cells that share the face, which is what makes the
    surface watertight whatever the field;
  * a segment p -> q is directed so that cross(q - p, n_face) points at the inside corner it cuts off (n_face: the face's outward normal);
  * the segments are followed into closed loops;
  * each loop is triangulated as a fan, from an apex chosen so that no fan diagonal joins two cube edges of one face (such a diagonal would lie
    in the face, on top of -- or crossing -- that face's segments).  Such an apex exists for all 256 cases (asserted).
Result: at most 5 triangles per case, 820 in all.  Triangles are counter-clockwise seen from the LOW-density side: normals point out of the dense
region (case 1, corner 0 inside, has normal (+,+,+)).  Whether PyMCubes winds its triangles the same way could not be checked where this was
written; a consumer that needs the other orientation swaps two columns of the triangle array.
"""
import os


def corner_xyz(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def _edges():
    out = []
    for axis in range(3):
        others = [d for d in range(3) if d != axis]
        for k in range(4):
            base = [0, 0, 0]
            base[others[0]], base[others[1]] = k & 1, k >> 1
            far = list(base)
            far[axis] = 1
            out.append((corner_id(base), corner_id(far)))
    return out


EDGES = _edges()       # edge id -> its two corners (low end first)
EDGE_OF = {frozenset(e): i for i, e in enumerate(EDGES)}


def _faces():
    out = []
    for axis in range(3):
        others = [d for d in range(3) if d != axis]
        for side in (0, 1):
            cyc = []
            for p, q in ((0, 0), (1, 0), (1, 1), (0, 1)):
                v = [0, 0, 0]
                v[axis], v[others[0]], v[others[1]] = side, p, q
                cyc.append(corner_id(v))
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((cyc, tuple(n)))
    return out


FACES = _faces()       # (the four corners in cyclic order, outward normal)


def mid2(e):
    """Twice the midpoint of edge e (integers)."""
    a, b = corner_xyz(EDGES[e][0]), corner_xyz(EDGES[e][1])
    return tuple(a[d] + b[d] for d in range(3))


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def same_face(e0, e1):
    pts = [corner_xyz(c) for e in (e0, e1) for c in EDGES[e]]
    return any(len({p[d] for p in pts}) == 1 for d in range(3))


def face_segments(case, face):
    """Directed segments (edge -> edge) of one face for a case."""
    cyc, n = face
    inside = [(case >> c) & 1 for c in range(8)]
    crossing = [i for i in range(4) if inside[cyc[i]] != inside[cyc[(i + 1) % 4]]]
    segs = []
    if len(crossing) == 2:
        e0 = EDGE_OF[frozenset((cyc[crossing[0]], cyc[(crossing[0] + 1) % 4]))]
        e1 = EDGE_OF[frozenset((cyc[crossing[1]], cyc[(crossing[1] + 1) % 4]))]
        ic = EDGES[e0][0] if inside[EDGES[e0][0]] else EDGES[e0][1]
        segs.append((e0, e1, ic))
    elif len(crossing) == 4:
        for i in range(4):
            if inside[cyc[i]]:
                segs.append((EDGE_OF[frozenset((cyc[i - 1], cyc[i]))], EDGE_OF[frozenset((cyc[i], cyc[(i + 1) % 4]))], cyc[i]))
    out = []
    for e0, e1, ic in segs:
        p, q = mid2(e0), mid2(e1)
        side = cross(tuple(q[d] - p[d] for d in range(3)), n)
        to_corner = tuple(2 * corner_xyz(ic)[d] - p[d] for d in range(3))
        if sum(side[d] * to_corner[d] for d in range(3)) < 0:
            e0, e1 = e1, e0
        out.append((e0, e1))
    return out


def gen_case(case):
    nxt = {}
    for face in FACES:
        for e0, e1 in face_segments(case, face):
            assert e0 not in nxt
            nxt[e0] = e1
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [start], nxt[start]
        seen.add(start)
        while e != start:
            loop.append(e)
            seen.add(e)
            e = nxt[e]
        fan = None
        for r in range(len(loop)):
            rot = loop[r:] + loop[:r]
            if not any(same_face(rot[0], rot[i]) for i in range(2, len(rot) - 1)):
                fan = rot
                break
        assert fan is not None, case          # an apex without an in-face diagonal exists for every case
        for i in range(1, len(fan) - 1):
            tris.append((fan[0], fan[i], fan[i + 1]))
    return tris


def table():
    return [gen_case(c) for c in range(256)]


def main():
    tab = table()
    assert max(len(t) for t in tab) == 5 and sum(len(t) for t in tab) == 820 and not tab[0] and not tab[255]
    out = ["// GENERATED by gen_mc_tables.py -- do not edit.  Marching-cubes case table; conventions and derivation: gen_mc_tables.py.",
           "// corner c = x + 2y + 4z; edge e = axis * 4 + (offsets of the other two axes, lower axis in bit 0); case bit c = (u[corner c] > threshold).",
           "// MC_NTRI[case]: triangles of the case (<= 5).  MC_TRI[case]: their 3 * n cube edges, counter-clockwise seen from the low-density side, 255-padded.",
           "// The including file defines PNR_MC_TABLE (storage qualifiers) first.",
           "PNR_MC_TABLE unsigned char MC_NTRI[256] = {"]
    for r in range(0, 256, 32):
        out.append("  " + ", ".join(str(len(t)) for t in tab[r:r + 32]) + ",")
    out.append("};")
    out.append("PNR_MC_TABLE unsigned char MC_TRI[256][15] = {")
    for t in tab:
        flat = [e for tri in t for e in tri]
        out.append("  {" + ", ".join(str(v) for v in flat + [255] * (15 - len(flat))) + "},")
    out.append("};")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mc_tables.inc")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
