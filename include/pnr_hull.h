/* pnr_hull.h -- the hull simplification of the palette extraction on the device (additive to include/pnr.h, ABI 10; csrc/hull.hip).
 *
 * The link between pnr_extract_kmeans and pnr_lut_weights (include/pnr.h): Hull_Simplification_posternerf(data, prefix, pixel_counts,
 * error_thres, target_size) as palette/utils.py:230-234 calls it -- rgbsg/hull_simplification_posternerf.py:19-77, the edge collapse of
 * rgbsg/fastLayerDecomposition/Convexhull_simplification.py:149-322 with option=2, and the reconstruction error of
 * rgbsg/fastLayerDecomposition/Additive_mixing_layers_extraction.py:185-201.  It takes the K k-means centres with their weights and returns
 * the 4..10 palette colours.  The reference goes through qhull, an OBJ file per step and cvxopt's GLPK; the statement below needs neither:
 * every hull is found by brute force and every linear program by vertex enumeration.
 *
 * This header is separate from pnr.h because pnr.h's entries are held to an inventory (tests/test_guard_bands_host.py) that this change
 * does not edit; folding it into pnr.h is left to a change that may edit that inventory.  Its bindings are palettenerf_amd/_lib.py's
 * HULL_SIGNATURES, its tests tests/test_abi_hull.py and tests/test_gpu_hull.py (the guard bands of its arrays are tested there).
 *
 * pnr_hull_simplify: ONE launch of ONE workgroup of 512 lanes; the whole state (points, faces, normals, the previous vertex set) stays in
 * LDS.  float64 throughout, no atomics, every sum, minimum and tie in a fixed order: two runs give the same bits.
 *
 *   hull      of a point set: the faces are the triples i < j < k whose plane has every other point strictly on one side, by more than
 *             1e-9 along the unit normal (the rule of pnr_lut_weights), in ascending (i, j, k), turned outwards.  A point on no face is not
 *             a vertex and is dropped; the vertices keep their ascending input order (scipy's hull.vertices in 3-D).
 *   collapse  every edge (v1 < v2) of the faces in ascending order; its related faces are those that hold v1 or v2, in ascending face
 *             order; of each the unit normal n_i = cross(pj - pi, pk - pi) / sqrt(n.n), outward, and b_i = n_i . p_i at the face's lowest
 *             vertex; c = sum of the n_i in that order (Convexhull_simplification.py:180-194).  The candidate point of the edge is the
 *             solution of  min c.x  s.t.  n_i . x >= b_i  (:199-205), found by vertex enumeration: every triple of constraints a < b < c
 *             with |det| > 1e-12, x = adjugate . b / det, feasible when n_i . x - b_i >= -1e-9 for every related face; the feasible x with
 *             the smallest c.x, a tie to the lowest triple.  No feasible vertex: the edge has no candidate (the reference's
 *             status != 'optimal'; the program cannot be unbounded: c.d >= 0 on every feasible direction).  The edge's cost is
 *             sum |n_raw_i . (x - p_i)| / 6 with the unnormalised normals (:216-219); the edge with the smallest cost wins, a tie to the
 *             lowest (v1, v2).  The new point set is the old one without v1 and v2, order kept, with x appended (:282-306), and its hull
 *             is taken as above.  If no edge has a candidate the set is unchanged.
 *   error     of a vertex set (Additive_mixing_layers_extraction.py:185-201): the vertices clipped to [0,1]; over the centres outside the
 *             clipped hull sqrt(sum w d^2 / sum of ALL w), the sums in ascending centre order.  A centre is outside when its signed
 *             distance to some supporting plane exceeds 1e-8; d is its distance to the nearest supporting triangle (the closest-point
 *             routine of pnr_lut_weights, the same region order).  Clipping makes coplanar and coincident vertices ordinary, so THIS hull
 *             takes every supporting triple with a normal longer than 1e-12 and some vertex off its plane, non-strict within 1e-9: the
 *             minimum over them does not depend on a triangulation.  A clipped set without such a triple is the reference's `fail`.
 *   loop      hull_simplification_posternerf.py:42-74.  After each collapse, with V the new vertex count:
 *               V <= 10 and target_size == 0: the error; on `fail` or error > error_thres return the vertex set from BEFORE this collapse
 *                                             (PNR_HULL_STOP_ERROR)
 *               V <= 10 and V == target_size: return the current set (PNR_HULL_STOP_TARGET); a collapse that steps over target_size runs on
 *               then, V unchanged (PNR_HULL_STOP_UNCHANGED) or V == 4 (PNR_HULL_STOP_FOUR): return the current set.
 *             Every returned set is clipped to [0,1].  Each collapse removes at least one vertex: at most K - 4 happen, and K - 3 is the
 *             bound of the kernel's loop.
 *
 * centers [K,3] and center_weights [K]: float64 on the device, exactly what pnr_extract_kmeans writes; 4 <= K <= PNR_EXTRACT_MAX_K.
 * target_size: 0 (none: the error rule decides) or 4..PNR_HULL_MAX_M.
 * palette [PNR_HULL_MAX_M,3]: the first min(M, PNR_HULL_MAX_M) colours.  vertices [K,3] (optional): all M rows -- the unchanged rule and
 * the error rule can return more than PNR_HULL_MAX_M, and a hand-over usually does.
 * info [8]: the status, M, the collapses run, the initial hull's vertex count, the stop rule, the largest related-face count seen, 0, 0.
 * errors [8] (optional, a debug output): errors[10 - V] is the reconstruction error computed at V = 10..4, PNR_HULL_ERROR_NONE where none
 * was computed, PNR_HULL_ERROR_FAIL for the reference's `fail`; errors[7] = PNR_HULL_ERROR_NONE.
 * trace [K,4] (optional, a debug output): per collapse v1, v2, the vertex count after it, and the number of edges that had a candidate.
 *
 * What is known on the device only is answered in info[0], not in the return value (the contract of PNR_EXTRACT_EMPTIED):
 *   PNR_HULL_COPLANAR  a supporting plane of a hull carries a fourth point within 1e-9: the triangulation of that facet is qhull's
 *                      choice and changes the result -- refused rather than picked, as in pnr_lut_weights
 *   PNR_HULL_FLAT      no triple of a point set has a point off its plane
 *   PNR_HULL_DENSE     an edge has more than PNR_HULL_MAX_RELATED related faces
 * Then palette / vertices hold, UNCLIPPED, the vertex set the iteration in progress started from (the centres themselves when the first
 * hull was refused) and info[1] its size, info[4] = PNR_HULL_STOP_NONE, and the caller finishes on the host from that set
 * (palettenerf_amd.extract.simplify_hull does, with scipy).
 *
 * PNR_ERR_INVALID before any launch: a NULL struct, centers, center_weights, palette or info; K outside 4..PNR_EXTRACT_MAX_K; error_thres
 * negative or NaN; target_size outside {0, 4..PNR_HULL_MAX_M}; a float64 array not 8-byte aligned or an int32 array not 4-byte aligned. */
#ifndef PNR_HULL_H_
#define PNR_HULL_H_
#include "pnr.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PNR_HULL_MAX_M 16
#define PNR_HULL_MAX_RELATED 64
#define PNR_HULL_OK 0
#define PNR_HULL_COPLANAR 1
#define PNR_HULL_FLAT 2
#define PNR_HULL_DENSE 3
#define PNR_HULL_STOP_NONE 0
#define PNR_HULL_STOP_ERROR 1
#define PNR_HULL_STOP_TARGET 2
#define PNR_HULL_STOP_UNCHANGED 3
#define PNR_HULL_STOP_FOUR 4
#define PNR_HULL_ERROR_NONE (-1.0)
#define PNR_HULL_ERROR_FAIL (-2.0)
typedef struct pnr_hull_simplify_args {
    const double* centers;              /* [K,3] */
    const double* center_weights;       /* [K] */
    uint32_t K;
    double error_thres;                 /* the reference's 5 / 255 */
    uint32_t target_size;               /* 0, or 4..PNR_HULL_MAX_M */
    double* palette;                    /* [PNR_HULL_MAX_M,3] out */
    int32_t* info;                      /* [8] out */
    double* errors;                     /* [8] out, optional */
    int32_t* trace;                     /* [K,4] out, optional */
    double* vertices;                   /* [K,3] out, optional */
} pnr_hull_simplify_args;
int pnr_hull_simplify(const pnr_hull_simplify_args* args, pnr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PNR_HULL_H_ */
