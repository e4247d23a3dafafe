// hull.hip -- the hull simplification of the palette extraction for gfx950 (include/pnr_hull.h):
//   pnr_hull_simplify   Hull_Simplification_posternerf (rgbsg/hull_simplification_posternerf.py:19-77, Convexhull_simplification.py:149-322 with
//                       option=2, Additive_mixing_layers_extraction.py:185-201): K <= 128 k-means centres -> the 4..10 palette colours
// ONE launch of ONE workgroup of 512 lanes (8 waves); the whole state lives in LDS (about 47 KB), the centres themselves in registers (lane t
// keeps centre t).  The work is serial in nature -- one edge collapse after the other -- and each step is spread over the workgroup:
//   hull      brute force.  Lane p takes the pair (i, j) = (p / n, p % n), i < j, and walks k > j: the triple is a face when every other point is
//             on one side of its plane by more than 1e-9; the walk over the other points ends at the first point on the second side.  An edge of
//             a simplicial hull has two faces, so a pair keeps at most two k (a third one is an inconsistency and refused as coplanar).  The
//             first wave then compacts the pairs' faces row by row with ballots: ascending (i, j, k) without a sort.  Points on no face are
//             dropped with the same compaction, and the faces renumbered (the map is monotone: the order stays ascending).
//   collapse  the edges are the pairs that occur in a face, compacted the same way.  A WAVE takes an edge: it gathers the related faces in
//             ascending order (ballots), every lane sums c in that order, and the lanes share the constraint pairs (a, b) and walk c > b: vertex
//             enumeration of the edge's linear program.  The best vertex of a lane, then of the wave (xor shuffles; the order (objective, triple)
//             is total, so the order of the reduction does not matter).  The first wave picks the cheapest edge the same way.
//   error     a lane per triple of the at most 10 clipped vertices (at most 120), then a lane per centre; lane 0 adds in ascending centre order.
// Every loop is bounded by K, by the face cap or by the related-face cap; nothing waits on another lane's value except at workgroup barriers, which
// every lane reaches the same number of times (the stop rules are read from LDS after a barrier and are uniform).  No atomics.  float64, built
// with -ffp-contract=off like every unit: nothing below is fused, so two runs give the same bits.
#include "pnr_common.hpp"
#include "../../include/pnr_hull.h"

namespace pnr {
namespace {

constexpr uint32_t kHullBlock = 512, kHullWaves = kHullBlock / PNR_WAVE;
constexpr uint32_t kMaxPts = PNR_EXTRACT_MAX_K;                     // 128
constexpr uint32_t kMaxPairs = kMaxPts * (kMaxPts - 1) / 2;         // 8128
constexpr uint32_t kMaxFaces = 2 * kMaxPts;                         // a simplicial hull of n points has 2n - 4 faces
constexpr uint32_t kMaxEdges = 3 * kMaxPts;                         // ... and 3n - 6 edges
constexpr uint32_t kMaxRel = PNR_HULL_MAX_RELATED;
constexpr uint32_t kErrV = 10, kErrTriples = 120;                   // C(10, 3)
constexpr double kPlaneEps = 1e-9, kOutsideEps = 1e-8, kDetEps = 1e-12, kFeasEps = 1e-9, kDegenerate = 1e-12;
static_assert(kMaxPts == 128 && kMaxRel == 64 && kMaxRel <= kMaxFaces, "the pair table keeps k in 7 bits; a triple key keeps three 6-bit constraint numbers");

struct HullLds {
    double pts[kMaxPts][3];            // the current point set; after hull(): its vertices
    double prev[kMaxPts][3];           // the vertex set the iteration in progress started from
    double fn[kMaxFaces][3];           // a face: unit outward normal, unnormalised outward normal, b = fn . (its lowest vertex)
    double fraw[kMaxFaces][3];
    double fb[kMaxFaces];
    uint8_t fi[kMaxFaces], fj[kMaxFaces], fk[kMaxFaces], fflip[kMaxFaces];
    uint8_t vflag[kMaxPts], vmap[kMaxPts];
    uint8_t rel[kHullWaves][kMaxRel];  // a wave's related faces
    union {
        struct {                       // hull(): per pair (row-major upper triangle) up to two k, bit 7 = the normal is turned
            uint8_t pk[2 * kMaxPairs];
            uint8_t pc[kMaxPairs];
        } h;
        struct {                       // collapse
            uint8_t eflag[kMaxPairs];
            uint8_t e1[kMaxEdges], e2[kMaxEdges], ehas[kMaxEdges], erel[kMaxEdges];
            double ecost[kMaxEdges];
            double ex[kMaxEdges][3];
        } e;
        struct {                       // error
            double q[kErrV][3];
            double ta[kErrTriples][3], tab[kErrTriples][3], tac[kErrTriples][3], tn[kErrTriples][3];
            double term[kMaxPts];
            uint8_t tsup[kErrTriples];
        } r;
    } u;
    double errors[8];
    double err, wsum;
    int nfaces, nverts, nedges, nonflat, coplanar, overflow, dense, anysup;
    int win, ncand, maxrel;
};

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ uint32_t pair_row(uint32_t i, uint32_t n) { return i * (2 * n - i - 1) / 2; }      // pairs (i', j) with i' < i
__device__ __forceinline__ uint32_t pair_index(uint32_t i, uint32_t j, uint32_t n) { return pair_row(i, n) + (j - i - 1); }
__device__ __forceinline__ double clip01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// the closest point of triangle (a, a + ab, a + ac) to p as a + v ab + w ac: the Voronoi regions of the triangle in the order of lut.hip
__device__ __forceinline__ void closest_vw(const double* a, const double* ab, const double* ac, const double (&p)[3], double& v, double& w) {
    double ap[3], bp[3], cp[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        ap[d] = p[d] - a[d];
        bp[d] = p[d] - (a[d] + ab[d]);
        cp[d] = p[d] - (a[d] + ac[d]);
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; }
    else if (d3 >= 0.0 && d4 <= d3) { v = 1.0; w = 0.0; }
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { v = d1 / (d1 - d3); w = 0.0; }
    else if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; }
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { v = 0.0; w = d2 / (d2 - d6); }
    else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) { w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0 - w; }
    else { const double sum = (va + vb) + vc; v = vb / sum; w = vc / sum; }
}

// The strict hull of s.pts[0..n): on PNR_HULL_OK s.pts holds the s.nverts vertices in their order and the s.nfaces faces are complete.
// Every lane calls it and gets the same status.
__device__ int hull_build(HullLds& s, uint32_t n) {
    const uint32_t tid = threadIdx.x, lane = tid & (PNR_WAVE - 1);
    if (tid == 0) s.nfaces = s.nverts = s.nonflat = s.coplanar = s.overflow = 0;
    if (tid < n) s.vflag[tid] = 0;
    __syncthreads();

    for (uint32_t p = tid; p < n * n; p += kHullBlock) {
        const uint32_t i = p / n, j = p % n;
        if (i >= j) continue;
        const uint32_t t = pair_index(i, j, n);
        uint32_t cnt = 0;
        double pi[3], e1[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            pi[d] = s.pts[i][d];
            e1[d] = s.pts[j][d] - pi[d];
        }
        for (uint32_t k = j + 1; k < n; k++) {
            double e2[3], nrm[3];
#pragma unroll
            for (int d = 0; d < 3; d++) e2[d] = s.pts[k][d] - pi[d];
            cross3(e1, e2, nrm);
            const double len2 = dot3(nrm, nrm);
            if (!(len2 > 0.0)) continue;
            const double len = sqrt(len2);
#pragma unroll
            for (int d = 0; d < 3; d++) nrm[d] = nrm[d] / len;
            bool pos = false, neg = false, near = false;
            for (uint32_t l = 0; l < n; l++) {
                if (l == i || l == j || l == k) continue;
                double r[3];
#pragma unroll
                for (int d = 0; d < 3; d++) r[d] = s.pts[l][d] - pi[d];
                const double dist = dot3(nrm, r);
                if (dist > kPlaneEps) pos = true;
                else if (dist < -kPlaneEps) neg = true;
                else near = true;
                if (pos && neg) break;                          // two-sided: no face, whatever the remaining points do
            }
            if (pos || neg) s.nonflat = 1;
            if (pos != neg) {
                if (near) s.coplanar = 1;
                else if (cnt < 2) s.u.h.pk[2 * t + cnt++] = (uint8_t)(k | (pos ? 0x80u : 0u));     // the others in front: the normal is turned
                else s.overflow = 1;
            }
        }
        s.u.h.pc[t] = (uint8_t)cnt;
    }
    __syncthreads();

    // ---- the faces in ascending (i, j, k), and the vertex flags: the first wave compacts a row of pairs 64 slots a step ----
    if (tid < PNR_WAVE) {
        uint32_t nf = 0;
        for (uint32_t i = 0; i + 1 < n; i++) {
            const uint32_t row = pair_row(i, n), slots = 2 * (n - i - 1);
            for (uint32_t base = 0; base < slots; base += PNR_WAVE) {
                const uint32_t q = base + lane;
                const bool has = q < slots && (q & 1u) < s.u.h.pc[row + (q >> 1)];
                const unsigned long long mask = __ballot(has);
                const uint32_t slot = nf + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (has && slot < kMaxFaces) {
                    const uint32_t j = i + 1 + (q >> 1), kf = s.u.h.pk[2 * row + q], k = kf & 0x7fu;
                    s.fi[slot] = (uint8_t)i;
                    s.fj[slot] = (uint8_t)j;
                    s.fk[slot] = (uint8_t)k;
                    s.fflip[slot] = (uint8_t)(kf >> 7);
                    s.vflag[i] = 1;
                    s.vflag[j] = 1;
                    s.vflag[k] = 1;
                }
                nf += (uint32_t)__popcll(mask);
            }
        }
        if (lane == 0) s.nfaces = (int)nf;
    }
    __syncthreads();
    const uint32_t F = (uint32_t)s.nfaces;
    if (!s.nonflat) return PNR_HULL_FLAT;
    if (s.coplanar || s.overflow || F > 2 * n - 4) return PNR_HULL_COPLANAR;      // (more than 2n - 4 faces cannot be a simplicial hull)
    if (F < 4) return PNR_HULL_FLAT;

    // ---- drop the points on no face, order kept ----
    if (tid < PNR_WAVE) {
        uint32_t nv = 0;
        for (uint32_t base = 0; base < n; base += PNR_WAVE) {
            const uint32_t i = base + lane;
            const bool has = i < n && s.vflag[i];
            const unsigned long long mask = __ballot(has);
            if (has) s.vmap[i] = (uint8_t)(nv + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)));
            nv += (uint32_t)__popcll(mask);
        }
        if (lane == 0) s.nverts = (int)nv;
    }
    __syncthreads();
    double mine[3] = {0.0, 0.0, 0.0};
    const bool keep = tid < n && s.vflag[tid];
    if (keep)
        for (int d = 0; d < 3; d++) mine[d] = s.pts[tid][d];
    __syncthreads();
    if (keep)
        for (int d = 0; d < 3; d++) s.pts[s.vmap[tid]][d] = mine[d];
    __syncthreads();

    // ---- the faces in the vertices' numbering, with their normals ----
    if (tid < F) {
        const uint32_t i = s.vmap[s.fi[tid]], j = s.vmap[s.fj[tid]], k = s.vmap[s.fk[tid]];
        double e1[3], e2[3], nrm[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            e1[d] = s.pts[j][d] - s.pts[i][d];
            e2[d] = s.pts[k][d] - s.pts[i][d];
        }
        cross3(e1, e2, nrm);
        const double len = sqrt(dot3(nrm, nrm));
        const bool flip = s.fflip[tid] != 0;
        double unit[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            unit[d] = nrm[d] / len;
            if (flip) { unit[d] = -unit[d]; nrm[d] = -nrm[d]; }
            s.fn[tid][d] = unit[d];
            s.fraw[tid][d] = nrm[d];
        }
        s.fb[tid] = dot3(unit, s.pts[i]);
        s.fi[tid] = (uint8_t)i;
        s.fj[tid] = (uint8_t)j;
        s.fk[tid] = (uint8_t)k;
    }
    __syncthreads();
    return PNR_HULL_OK;
}

// One collapse step on the V vertices with their faces: the winning edge in s.win (s.ncand == 0: no edge has a candidate), its point in
// s.u.e.ex[s.win].  Returns PNR_HULL_DENSE when an edge has more related faces than the cap.  Every lane calls it.
__device__ int collapse_find(HullLds& s, uint32_t V) {
    const uint32_t tid = threadIdx.x, lane = tid & (PNR_WAVE - 1), wave = tid / PNR_WAVE;
    const uint32_t F = (uint32_t)s.nfaces, pairs = V * (V - 1) / 2;
    if (tid == 0) s.nedges = s.dense = s.ncand = 0;
    for (uint32_t t = tid; t < pairs; t += kHullBlock) s.u.e.eflag[t] = 0;
    __syncthreads();
    if (tid < F) {
        const uint32_t i = s.fi[tid], j = s.fj[tid], k = s.fk[tid];
        s.u.e.eflag[pair_index(i, j, V)] = 1;
        s.u.e.eflag[pair_index(i, k, V)] = 1;
        s.u.e.eflag[pair_index(j, k, V)] = 1;
    }
    __syncthreads();
    if (tid < PNR_WAVE) {
        uint32_t ne = 0;
        for (uint32_t i = 0; i + 1 < V; i++) {
            const uint32_t row = pair_row(i, V), cols = V - i - 1;
            for (uint32_t base = 0; base < cols; base += PNR_WAVE) {
                const uint32_t q = base + lane;
                const bool has = q < cols && s.u.e.eflag[row + q];
                const unsigned long long mask = __ballot(has);
                const uint32_t slot = ne + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (has && slot < kMaxEdges) {
                    s.u.e.e1[slot] = (uint8_t)i;
                    s.u.e.e2[slot] = (uint8_t)(i + 1 + q);
                }
                ne += (uint32_t)__popcll(mask);
            }
        }
        if (lane == 0) s.nedges = (int)(ne < kMaxEdges ? ne : kMaxEdges);      // (3V - 6 <= 378 on a simplicial hull)
    }
    __syncthreads();
    const uint32_t E = (uint32_t)s.nedges;

    // ---- a wave per edge; every wave makes the same number of trips, so the barriers below are met by all ----
    for (uint32_t e0 = 0; e0 < E; e0 += kHullWaves) {
        const uint32_t e = e0 + wave;
        const bool active = e < E;
        uint32_t m = 0;
        if (active) {
            const uint32_t v1 = s.u.e.e1[e], v2 = s.u.e.e2[e];
            for (uint32_t base = 0; base < F; base += PNR_WAVE) {
                const uint32_t f = base + lane;
                bool has = false;
                if (f < F) {
                    const uint32_t i = s.fi[f], j = s.fj[f], k = s.fk[f];
                    has = i == v1 || j == v1 || k == v1 || i == v2 || j == v2 || k == v2;
                }
                const unsigned long long mask = __ballot(has);
                const uint32_t slot = m + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (has && slot < kMaxRel) s.rel[wave][slot] = (uint8_t)f;
                m += (uint32_t)__popcll(mask);
            }
            if (lane == 0) {
                s.u.e.erel[e] = (uint8_t)(m < 255u ? m : 255u);
                s.u.e.ehas[e] = 0;
                if (m > kMaxRel) s.dense = 1;
            }
        }
        __syncthreads();
        if (active && m <= kMaxRel && m >= 3) {
            const uint8_t* rel = s.rel[wave];
            double c[3] = {0.0, 0.0, 0.0};
            for (uint32_t q = 0; q < m; q++)
#pragma unroll
                for (int d = 0; d < 3; d++) c[d] = c[d] + s.fn[rel[q]][d];
            bool found = false;
            double best = 0.0, bx[3] = {0.0, 0.0, 0.0};
            uint32_t bkey = 0;
            for (uint32_t p = lane; p < m * m; p += PNR_WAVE) {
                const uint32_t ia = p / m, ib = p % m;
                if (ia >= ib) continue;
                const double* na = s.fn[rel[ia]];
                const double* nb = s.fn[rel[ib]];
                const double ba = s.fb[rel[ia]], bb = s.fb[rel[ib]];
                double ab[3];
                cross3(na, nb, ab);
                for (uint32_t ic = ib + 1; ic < m; ic++) {
                    const double* nc = s.fn[rel[ic]];
                    const double bc_ = s.fb[rel[ic]];
                    double bc[3], ca[3], x[3];
                    cross3(nb, nc, bc);
                    cross3(nc, na, ca);
                    const double det = dot3(na, bc);
                    if (!(fabs(det) > kDetEps)) continue;
#pragma unroll
                    for (int d = 0; d < 3; d++) x[d] = ((ba * bc[d] + bb * ca[d]) + bc_ * ab[d]) / det;
                    bool feasible = true;
                    for (uint32_t q = 0; q < m; q++) {
                        if (!(dot3(s.fn[rel[q]], x) - s.fb[rel[q]] >= -kFeasEps)) { feasible = false; break; }
                    }
                    if (!feasible) continue;
                    const double obj = dot3(c, x);
                    const uint32_t key = (ia << 12) | (ib << 6) | ic;
                    if (!found || obj < best || (obj == best && key < bkey)) {
                        found = true; best = obj; bkey = key; bx[0] = x[0]; bx[1] = x[1]; bx[2] = x[2];
                    }
                }
            }
            // the wave's best: (objective, triple) is a total order on the candidates, a lane without one loses to any
#pragma unroll
            for (int off = 1; off < PNR_WAVE; off <<= 1) {
                const int ofound = __shfl_xor((int)found, off, PNR_WAVE);
                const double obest = __shfl_xor(best, off, PNR_WAVE);
                const uint32_t okey = (uint32_t)__shfl_xor((int)bkey, off, PNR_WAVE);
                const double ox0 = __shfl_xor(bx[0], off, PNR_WAVE), ox1 = __shfl_xor(bx[1], off, PNR_WAVE), ox2 = __shfl_xor(bx[2], off, PNR_WAVE);
                if (ofound && (!found || obest < best || (obest == best && okey < bkey))) {
                    found = true; best = obest; bkey = okey; bx[0] = ox0; bx[1] = ox1; bx[2] = ox2;
                }
            }
            if (found && lane == 0) {
                double cost = 0.0;
                for (uint32_t q = 0; q < m; q++) {
                    const uint32_t f = rel[q];
                    double r[3];
#pragma unroll
                    for (int d = 0; d < 3; d++) r[d] = bx[d] - s.pts[s.fi[f]][d];
                    cost = cost + fabs(dot3(s.fraw[f], r)) / 6.0;
                }
                s.u.e.ehas[e] = 1;
                s.u.e.ecost[e] = cost;
#pragma unroll
                for (int d = 0; d < 3; d++) s.u.e.ex[e][d] = bx[d];
            }
        }
        __syncthreads();
    }

    // ---- the cheapest edge, a tie to the lowest; the candidates; the largest related-face count ----
    if (tid < PNR_WAVE) {
        bool found = false;
        double best = 0.0;
        uint32_t be = 0, cands = 0, most = 0;
        for (uint32_t base = 0; base < E; base += PNR_WAVE) {
            const uint32_t e = base + lane;
            const bool has = e < E && s.u.e.ehas[e];
            cands += (uint32_t)__popcll(__ballot(has));
            if (e < E && s.u.e.erel[e] > most) most = s.u.e.erel[e];
            if (has && (!found || s.u.e.ecost[e] < best)) { found = true; best = s.u.e.ecost[e]; be = e; }     // (ascending e in a lane: strict <)
        }
#pragma unroll
        for (int off = 1; off < PNR_WAVE; off <<= 1) {
            const int ofound = __shfl_xor((int)found, off, PNR_WAVE);
            const double obest = __shfl_xor(best, off, PNR_WAVE);
            const uint32_t obe = (uint32_t)__shfl_xor((int)be, off, PNR_WAVE), omost = (uint32_t)__shfl_xor((int)most, off, PNR_WAVE);
            if (ofound && (!found || obest < best || (obest == best && obe < be))) { found = true; best = obest; be = obe; }
            if (omost > most) most = omost;
        }
        if (lane == 0) {
            s.win = (int)be;
            s.ncand = (int)cands;
            if ((int)most > s.maxrel) s.maxrel = (int)most;
        }
    }
    __syncthreads();
    return s.dense ? PNR_HULL_DENSE : PNR_HULL_OK;
}

// The reconstruction error of the centres against the clipped vertices s.pts[0..V), V <= 10, into s.err (PNR_HULL_ERROR_FAIL: no supporting
// triple).  cx, cw: this lane's centre and weight (lanes below K).  Every lane calls it.
__device__ void hull_error(HullLds& s, uint32_t V, uint32_t K, const double (&cx)[3], double cw) {
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s.anysup = 0;
    if (tid < V)
        for (int d = 0; d < 3; d++) s.u.r.q[tid][d] = clip01(s.pts[tid][d]);
    __syncthreads();
    if (tid < kErrTriples) {
        // triple number tid of the ascending triples of V
        uint32_t r = tid, i = 0, j = 0, k = 0;
        bool valid = false;
        for (i = 0; i + 2 < V; i++) {
            const uint32_t cnt = (V - 1 - i) * (V - 2 - i) / 2;
            if (r < cnt) { valid = true; break; }
            r -= cnt;
        }
        if (valid) {
            for (j = i + 1; j + 1 < V; j++) {
                const uint32_t cnt = V - 1 - j;
                if (r < cnt) break;
                r -= cnt;
            }
            k = j + 1 + r;
        }
        uint8_t sup = 0;
        if (valid) {
            double e1[3], e2[3], nrm[3];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                e1[d] = s.u.r.q[j][d] - s.u.r.q[i][d];
                e2[d] = s.u.r.q[k][d] - s.u.r.q[i][d];
            }
            cross3(e1, e2, nrm);
            const double len = sqrt(dot3(nrm, nrm));
            if (len > kDegenerate) {
#pragma unroll
                for (int d = 0; d < 3; d++) nrm[d] = nrm[d] / len;
                bool pos = false, neg = false;
                for (uint32_t l = 0; l < V; l++) {
                    if (l == i || l == j || l == k) continue;
                    double rr[3];
#pragma unroll
                    for (int d = 0; d < 3; d++) rr[d] = s.u.r.q[l][d] - s.u.r.q[i][d];
                    const double dist = dot3(nrm, rr);
                    pos |= dist > kPlaneEps;
                    neg |= dist < -kPlaneEps;
                }
                if (pos != neg) {
                    sup = 1;
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        s.u.r.ta[tid][d] = s.u.r.q[i][d];
                        s.u.r.tab[tid][d] = e1[d];
                        s.u.r.tac[tid][d] = e2[d];
                        s.u.r.tn[tid][d] = pos ? -nrm[d] : nrm[d];
                    }
                    s.anysup = 1;
                }
            }
        }
        s.u.r.tsup[tid] = sup;
    }
    __syncthreads();
    if (tid < K) {
        bool outside = false;
        for (uint32_t t = 0; t < kErrTriples; t++) {
            if (!s.u.r.tsup[t]) continue;
            double r[3];
#pragma unroll
            for (int d = 0; d < 3; d++) r[d] = cx[d] - s.u.r.ta[t][d];
            outside |= dot3(s.u.r.tn[t], r) > kOutsideEps;
        }
        double term = 0.0;
        if (outside) {
            double best = 0.0;
            bool first = true;
            for (uint32_t t = 0; t < kErrTriples; t++) {
                if (!s.u.r.tsup[t]) continue;
                double v, w, e[3];
                closest_vw(s.u.r.ta[t], s.u.r.tab[t], s.u.r.tac[t], cx, v, w);
#pragma unroll
                for (int d = 0; d < 3; d++) e[d] = cx[d] - (s.u.r.ta[t][d] + (v * s.u.r.tab[t][d] + w * s.u.r.tac[t][d]));
                const double sq = dot3(e, e);
                if (first || sq < best) { first = false; best = sq; }
            }
            term = cw * best;
        }
        s.u.r.term[tid] = term;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (uint32_t t = 0; t < K; t++) total = total + s.u.r.term[t];
        s.err = s.anysup ? sqrt(total / s.wsum) : PNR_HULL_ERROR_FAIL;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kHullBlock) k_hull_simplify(const pnr_hull_simplify_args a) {
    __shared__ HullLds s;
    const uint32_t tid = threadIdx.x, K = a.K;
    double cx[3] = {0.0, 0.0, 0.0}, cw = 0.0;
    if (tid < K) {
        for (int d = 0; d < 3; d++) s.pts[tid][d] = cx[d] = a.centers[3 * tid + d];
        cw = a.center_weights[tid];
        s.u.r.term[tid] = cw;
    }
    if (tid < 8) s.errors[tid] = PNR_HULL_ERROR_NONE;
    if (tid == 0) s.maxrel = 0;
    __syncthreads();
    if (tid == 0) {
        double wsum = 0.0;
        for (uint32_t t = 0; t < K; t++) wsum = wsum + s.u.r.term[t];
        s.wsum = wsum;
    }
    __syncthreads();

    int status = hull_build(s, K);
    uint32_t V = status == PNR_HULL_OK ? (uint32_t)s.nverts : K;        // a refused first hull returns the centres themselves
    const uint32_t initial = status == PNR_HULL_OK ? V : 0;
    uint32_t collapses = 0, stop = PNR_HULL_STOP_NONE;
    bool from_prev = false;                                             // the returned set: s.prev (Vprev rows) or s.pts (V rows)
    uint32_t Vprev = V;

    for (uint32_t it = 0; status == PNR_HULL_OK && stop == PNR_HULL_STOP_NONE && it + 3 < K; it++) {
        Vprev = V;
        if (tid < V)
            for (int d = 0; d < 3; d++) s.prev[tid][d] = s.pts[tid][d];
        status = collapse_find(s, V);                                   // (begins with a barrier)
        if (status != PNR_HULL_OK) { from_prev = true; break; }
        if (s.ncand > 0) {
            const uint32_t e = (uint32_t)s.win, v1 = s.u.e.e1[e], v2 = s.u.e.e2[e], cands = (uint32_t)s.ncand;
            double mine[3] = {0.0, 0.0, 0.0};
            const bool moves = tid < V && tid != v1 && tid != v2;
            if (moves)
                for (int d = 0; d < 3; d++) mine[d] = s.pts[tid][d];
            if (tid == V)
                for (int d = 0; d < 3; d++) mine[d] = s.u.e.ex[e][d];
            __syncthreads();
            if (moves)
                for (int d = 0; d < 3; d++) s.pts[tid - (tid > v1) - (tid > v2)][d] = mine[d];
            if (tid == V)
                for (int d = 0; d < 3; d++) s.pts[V - 2][d] = mine[d];
            status = hull_build(s, V - 1);                              // (begins with a barrier)
            if (status != PNR_HULL_OK) { from_prev = true; break; }
            V = (uint32_t)s.nverts;
            if (tid == 0 && a.trace) {
                int32_t* row = a.trace + 4 * collapses;
                row[0] = (int32_t)v1; row[1] = (int32_t)v2; row[2] = (int32_t)V; row[3] = (int32_t)cands;
            }
            collapses++;
        }
        if (V <= kErrV) {
            if (a.target_size == 0) {
                hull_error(s, V, K, cx, cw);
                const double err = s.err;
                if (tid == 0) s.errors[kErrV - V] = err;
                if (err == PNR_HULL_ERROR_FAIL || err > a.error_thres) { stop = PNR_HULL_STOP_ERROR; from_prev = true; }
            } else if (V == a.target_size) {
                stop = PNR_HULL_STOP_TARGET;
            }
        }
        if (stop == PNR_HULL_STOP_NONE) {
            if (V == Vprev) stop = PNR_HULL_STOP_UNCHANGED;
            else if (V == 4) stop = PNR_HULL_STOP_FOUR;
        }
    }
    __syncthreads();

    const uint32_t M = from_prev ? Vprev : V;
    const bool clip = status == PNR_HULL_OK;
    if (tid < M) {
        for (int d = 0; d < 3; d++) {
            const double v = from_prev ? s.prev[tid][d] : s.pts[tid][d];
            const double o = clip ? clip01(v) : v;
            if (tid < PNR_HULL_MAX_M) a.palette[3 * tid + d] = o;
            if (a.vertices) a.vertices[3 * tid + d] = o;
        }
    }
    if (tid < 8 && a.errors) a.errors[tid] = s.errors[tid];
    if (tid == 0) {
        a.info[0] = status;
        a.info[1] = (int32_t)M;
        a.info[2] = (int32_t)collapses;
        a.info[3] = (int32_t)initial;
        a.info[4] = (int32_t)(status == PNR_HULL_OK ? stop : PNR_HULL_STOP_NONE);
        a.info[5] = s.maxrel;
        a.info[6] = 0;
        a.info[7] = 0;
    }
}

}  // namespace
}  // namespace pnr

using namespace pnr;

extern "C" {

int pnr_hull_simplify(const pnr_hull_simplify_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_hull_simplify_args& a = *args;
    if (!a.centers || !a.center_weights || !a.palette || !a.info) return PNR_ERR_INVALID;
    if (a.K < 4 || a.K > PNR_EXTRACT_MAX_K) return PNR_ERR_INVALID;
    if (!(a.error_thres >= 0.0)) return PNR_ERR_INVALID;                // negative or NaN
    if (a.target_size != 0 && (a.target_size < 4 || a.target_size > PNR_HULL_MAX_M)) return PNR_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(a.centers) % 8 || reinterpret_cast<uintptr_t>(a.center_weights) % 8 || reinterpret_cast<uintptr_t>(a.palette) % 8 ||
        reinterpret_cast<uintptr_t>(a.errors) % 8 || reinterpret_cast<uintptr_t>(a.vertices) % 8 || reinterpret_cast<uintptr_t>(a.info) % 4 ||
        reinterpret_cast<uintptr_t>(a.trace) % 4)
        return PNR_ERR_INVALID;
    hipLaunchKernelGGL(k_hull_simplify, dim3(1), dim3(kHullBlock), 0, as_stream(stream), a);
    return check_launch();
}

}  // extern "C"
