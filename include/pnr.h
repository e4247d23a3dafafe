/*
 * pnr.h -- C ABI of libpnr_hip.so, the MI355X (gfx950) native replacement for the four CUDA
 * extensions of zfkuang/PaletteNeRF (`_raymarching`, `_gridencoder`, `_shencoder`, `_palette_func`).
 *
 * Conventions (they mirror the reference's pybind layer):
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - the caller allocates every buffer (inputs, outputs, scratch); kernels never allocate;
 *   - zero-initialisation contracts are the reference's (xyzs/dirs/deltas of the march kernels,
 *     grad_embeddings, SH grad_inputs are caller-zeroed);
 *   - sizes are passed explicitly, exactly as the reference's Python passes them;
 *   - `stream` is a hipStream_t (the reference launches on the legacy default stream; here the
 *     caller passes torch.cuda.current_stream().cuda_stream);
 *   - return value: 0 on success, PNR_ERR_* (<0) otherwise; pnr_error_string() describes it.
 *     The Python shim turns a non-zero return into RuntimeError (the reference raises
 *     RuntimeError through TORCH_CHECK / std::runtime_error).
 *   - threads: no entry point keeps global mutable state (pnr_set_option's switches apart); the frame calls keep a pinned control
 *     block and the previous frame's iteration count per host thread and device and work inside the caller's workspace, so
 *     several frames may be in flight at once -- one host thread, one workspace and one stream each (palettenerf_amd/pipeline.py).
 *
 * Each entry point cites the reference interface it replaces (file:line under the reference).
 */
#ifndef PNR_H_
#define PNR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNR_OK 0
#define PNR_ERR_INVALID (-1)      /* null pointer / bad size                                  */
#define PNR_ERR_UNSUPPORTED (-2)  /* C not in {1,2,4,8}, D not in 1..5, n_channel > 128, ...  */
#define PNR_ERR_LAUNCH (-3)       /* hipGetLastError() != hipSuccess after a launch           */
#define PNR_ERR_ALIGNMENT (-4)    /* pnr_mlp_*: an activation array that does not start on a 16-byte boundary or holds fewer than four floats;
                                     elsewhere: an array off the boundary its entry's comment names */

#define PNR_DTYPE_F32 0
#define PNR_DTYPE_F16 1

/* arithmetic of the fused field kernels: exact-fp32 matrix path (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain)
 * or split-fp16 (3 x v_mfma_f32_32x32x16_f16 per product, ~2^-22 relative, fp32 accumulate; ~5x fewer MFMA cycles) */
#define PNR_FIELD_FP32 0
#define PNR_FIELD_F16X3 1
/* opt-in: the COLOUR layers with weights split as above and activations rounded ONCE to fp16 (2 MFMAs per product, one conversion per activation
 * pair): ~1e-5 on a colour with unit-scale weights -- inside the 1e-4 colour contract, not fp32-class.  sigma_net keeps the split form: densities,
 * alphas, depth and the march are bit for bit those of PNR_FIELD_F16X3.  Same packed blobs.  Exists for the NeRF field and for the 4-basis PaletteNeRF
 * field without an edit head; the density-only call, other basis counts, edited and watched launches run it as PNR_FIELD_F16X3. */
#define PNR_FIELD_F16X2 2

#define PNR_CHANNEL_MAXIMUM 128   /* raymarching/src/raymarching.cu:13 */

typedef void* pnr_stream_t; /* hipStream_t */

const char* pnr_error_string(int code);
/* ABI version of this header; bumped on any signature change. */
int pnr_abi_version(void);
/* run-time switches that change speed only, for A/B measurements and tests: "block_skip" (exact jumps over empty blocks in the march),
 * "aux_fusion" (PaletteNeRF frame loop: aux composite inside the field kernel), "coop_march" (wave-cooperative march tail); these default to 1.
 * "composite_fusion" (frame loops; default 2): 2 = the field kernels do the whole compositing step of every iteration (three launches per
 * iteration), 1 = the NeRF field kernel composites the iterations with one sample per ray only, 0 = the composite launch does.  "adam_variant" (0..7, default 0): which multiply-adds of pnr_adam_step
 * are left uncontracted (kept for re-deriving the bit-exact form against a new torch build); "iteration_margin" (default 0): spare iterations
 * the frame loops enqueue beyond the previous frame's count before their first look at the control block; "hosted_tail" (default 1): the frame
 * loops' march launches hand the rays they have not finished within "march_budget" (default 2; "march_budget0" for a frame's first launch, default
 * 0 = that launch finishes every ray itself) sample-less probes to the first workgroups of the lookup launch that follows -- same rows, bit for bit;
 * "march_blocks" (default 0 = automatic): workgroup cap of such a budgeted march launch; "coarse_image" (default 1): pnr_grid_encode_backward_binned accumulates the
 * coarsest levels (tables of at most 16 384 rows) as LDS images instead of records; "cell_merge" (default 1): on its mid levels the samples of a ray that sit in
 * one cell are summed before their records are written; "scatter_staged" (default 1): its records are ordered by bucket in LDS and written coalesced
 * (0 = every lane writes its own records); "mlp_f16x3" (default 1): the training MLP launches use split-fp16 products; "train_coop" (default 1): pnr_march_rays_train*'s counting pass
 * marches four rays per wave cooperatively (same counts, same rows); "coop_march" also governs the cooperative tail of pnr_march_rays*;
 * "grid_lane_pairs" (default 1): the frame loops' lookup of one fp32 table puts the two x neighbours of a cell's corners into adjacent lanes of every gather
 * of a workgroup row's finer level (0 = every lane loads its own eight corners); same encoder output, bit for bit; "palette_waves12" (default 1): the
 * 4-basis PaletteNeRF field without a clip head runs its wide kernels (0 = the 8-wave ones); "dynamic_tiles" (default 0): the frame loops' field kernels
 * hand their wave tiles out through a device counter instead of a static schedule (measured slower); "grid_fast" (default 1): pnr_grid_encode_forward uses
 * its D = 3, C = 2 kernel where it applies (0 = the generic one; same bits); "flex_coop" (default 1): pnr_composite_rays_flex with at most 8 samples per
 * ray runs the workgroup-cooperative kernel (0 = one thread per ray; same bits); "grid_nt" (0..3, default 0): experiment, non-temporal stores (1) / input
 * loads (2) in that D = 3, C = 2 kernel.  Values outside a switch's range are clamped (masked for "adam_variant" and "grid_nt"); an unknown name or NULL
 * is PNR_ERR_INVALID.  The whole list, with each switch's range and environment variable, is palettenerf_amd/csrc/options.def. */
int pnr_set_option(const char* name, int value);

/* ---------------------------------------------------------------- raymarching: utils ------- */

/* replaces near_far_from_aabb, raymarching/src/raymarching.h:7, raymarching.cu:151-159 */
int pnr_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N,
                           float min_near, float* nears, float* fars, pnr_stream_t stream);
/* replaces sph_from_ray, raymarching.h:8, raymarching.cu:204-212 */
int pnr_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords,
                     pnr_stream_t stream);
/* replaces morton3D / morton3D_invert, raymarching.h:9-10, raymarching.cu:232-263 */
int pnr_morton3d(const int32_t* coords, uint32_t N, int32_t* indices, pnr_stream_t stream);
int pnr_morton3d_invert(const int32_t* indices, uint32_t N, int32_t* coords, pnr_stream_t stream);
/* replaces packbits, raymarching.h:11, raymarching.cu:295-303 ; N = number of output bytes */
int pnr_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, pnr_stream_t stream);

/* ---------------------------------------------------------------- raymarching: training ---- */

/* Scratch size (bytes) pnr_march_rays_train / pnr_compact_alive need for N elements. */
uint64_t pnr_scan_scratch_bytes(uint32_t N);

/* replaces march_rays_train, raymarching.h:13, raymarching.cu:485-493.
 * Same arguments plus `scratch` (>= pnr_scan_scratch_bytes(N) bytes).  Row order of `rays` and the
 * sample offsets are DETERMINISTIC (ray n -> row n, offset = counter[0] + exclusive prefix sum of
 * the per-ray counts) instead of atomicAdd-ordered; counter[0] += total, counter[1] += N. */
int pnr_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound,
                         float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                         const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                         int32_t* rays, int32_t* counter, const float* noises, void* scratch,
                         pnr_stream_t stream);

/* replaces composite_rays_train_forward / _backward, raymarching.h:14-15, raymarching.cu:647-655, 821-829 */
int pnr_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                     const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                     float* weights_sum, float* depth, float* image, pnr_stream_t stream);
int pnr_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                      const float* rgbs, const float* deltas, const int32_t* rays,
                                      const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                      float T_thresh, float* grad_sigmas, float* grad_rgbs, pnr_stream_t stream);
/* The training composite with the NeRF stage's rgb_norm regulariser as a fourth composited quantity: what nerf/renderer.py:301-332 computes
 * with spread_ray_to_sample (raymarching.cu:848-882), three elementwise ops, a repeat, a second composite_rays_train and a mean.
 * rays_gt[N,3] is indexed by ray id (rays[n,0]), as kernel_spread_ray_to_sample indexes its input; rgb_norm[index] = sum_k w_k n_k with
 * n_k = sum_c (rays_gt[index,c] - rgbs[k,c])^2 and the weights, stop rule and dead-ray rule of the plain entries.  weights_sum, depth and
 * image carry the bits of pnr_composite_rays_train_forward.  Backward: grad_rgb_norm[N] is the norm's upstream gradient,
 * grad_rgbs[k,c] = grad_image_c w_k + grad_rgb_norm w_k 2 (rgbs[k,c] - gt_c), and grad_sigmas takes the norm as a fourth channel of
 * raymarching.cu:681-761.  rays_gt receives no gradient.  N == 0 (backward: or M == 0) is PNR_OK; a NULL array is PNR_ERR_INVALID. */
int pnr_composite_rays_train_norm_forward(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                          const float* rays_gt, uint32_t M, uint32_t N, float T_thresh, float* weights_sum,
                                          float* depth, float* image, float* rgb_norm, pnr_stream_t stream);
int pnr_composite_rays_train_norm_backward(const float* grad_weights_sum, const float* grad_image, const float* grad_rgb_norm,
                                           const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                           const float* rays_gt, const float* weights_sum, const float* image,
                                           const float* rgb_norm, uint32_t M, uint32_t N, float T_thresh, float* grad_sigmas,
                                           float* grad_rgbs, pnr_stream_t stream);
/* replaces composite_rays_flex_train_forward / _backward, raymarching.h:16-17, raymarching.cu:657-668, 831-844 */
int pnr_composite_rays_flex_train_forward(const float* sigmas, const float* input, const float* deltas,
                                          const int32_t* rays, uint32_t M, uint32_t N, uint32_t n_channel,
                                          float T_thresh, float* output, pnr_stream_t stream);
int pnr_composite_rays_flex_train_backward(const float* grad_output, const float* sigmas, const float* input,
                                           const float* deltas, const int32_t* rays, const float* output,
                                           uint32_t M, uint32_t N, uint32_t n_channel, float T_thresh,
                                           float* grad_input, pnr_stream_t stream);
/* replaces spread_ray_to_sample, raymarching.h:18, raymarching.cu:884-894 */
int pnr_spread_ray_to_sample(const float* input, const int32_t* rays, uint32_t M, uint32_t N, uint32_t n_channel,
                             float* output, pnr_stream_t stream);

/* ---------------------------------------------------------------- raymarching: inference --- */

/* replaces march_rays, raymarching.h:20, raymarching.cu:1014-1021 */
int pnr_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                   const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                   uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars,
                   float* xyzs, float* dirs, float* deltas, const float* noises, pnr_stream_t stream);
/* replaces composite_rays, raymarching.h:21, raymarching.cu:1187-1193 (in place) */
int pnr_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive, float* rays_t,
                       const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum,
                       float* depth, float* image, pnr_stream_t stream);
/* replaces composite_rays_flex, raymarching.h:22, raymarching.cu:1195-1205 (in place on output) */
int pnr_composite_rays_flex(uint32_t n_alive, uint32_t n_step, uint32_t n_channel, float T_thresh,
                            const int32_t* rays_alive, const float* rays_t, const float* sigmas,
                            const float* input, const float* deltas, const float* weights_sum, float* output,
                            pnr_stream_t stream);
/* SURVEY 8(b)'s "multi-map variant" (ABI 7): the six / seven composite_rays_flex calls one march iteration of PaletteRenderer.run_cuda issues over the SAME
 * sigmas / deltas / rays_alive / weights_sum (palette/renderer.py:508-516) as ONE launch -- a ray's weights are formed once and folded into every map.  Each
 * map's output is bit for bit what pnr_composite_rays_flex gives (same fmaf chain per channel).  Legal to batch because composite_rays_flex writes neither
 * rays_alive nor rays_t nor weights_sum (raymarching.cu:1114-1185) and the reference issues all of them BEFORE the iteration's composite_rays (:517-519).
 * maps: host array of n_maps <= PNR_FLEX_MAX_MAPS entries (n_channel <= 128 each; an entry with n_channel 0 is skipped); n_step > 8 runs the maps one by one. */
#define PNR_FLEX_MAX_MAPS 8
typedef struct {
    uint32_t n_channel;
    const float* input;     /* [n_alive * n_step, n_channel] */
    float* output;          /* [N, n_channel], accumulated in place */
} pnr_flex_map;
int pnr_composite_rays_flex_multi(uint32_t n_alive, uint32_t n_step, float T_thresh, const int32_t* rays_alive,
                                  const float* rays_t, const float* sigmas, const float* deltas,
                                  const float* weights_sum, const pnr_flex_map* maps, uint32_t n_maps,
                                  pnr_stream_t stream);

/* MI355X-first additions: occupancy mip.  The bitfield is Morton-ordered, so a 4x4x4 brick of cells is one
 * aligned 8-byte word; pnr_build_occupancy_mip reduces every brick to an any-bit and an all-bit
 * (pnr_occupancy_mip_bytes(C,H) bytes, device) and appends the world-space bounding box of all occupied bricks
 * (two-cell margin).  The *_mip march entry points stage it in LDS, answer probes in uniformly empty / full bricks
 * without a global load and stop a ray once it has left the occupied box for good (no sample can follow).  Results are bit-identical to pnr_march_rays /
 * pnr_march_rays_train (which are the same kernels with mip == NULL).  Requires H % 4 == 0 and an 8-byte aligned
 * bitfield; the mip must be rebuilt whenever the bitfield changes.  `noises` may be NULL (= no perturbation). */
uint64_t pnr_occupancy_mip_bytes(uint32_t C, uint32_t H);
int pnr_build_occupancy_mip(const uint8_t* grid, uint32_t C, uint32_t H, float bound, void* mip, pnr_stream_t stream);
int pnr_march_rays_mip(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                       const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                       uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars,
                       float* xyzs, float* dirs, float* deltas, const float* noises, const void* mip,
                       pnr_stream_t stream);
/* The same march for buffers that arrive UNINITIALISED (the reference's Python zero-fills xyzs / dirs / deltas with three launches before every
 * call, raymarching.py:384-386): with fill_rows = the row count of the three buffers (>= n_alive * n_step; the alignment padding included) the
 * kernel itself zeroes every slot a ray leaves unfilled and the rows beyond n_alive * n_step.  fill_rows = 0: pnr_march_rays_mip. */
int pnr_march_rays_fill(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                       const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                       uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars,
                       float* xyzs, float* dirs, float* deltas, const float* noises, const void* mip, uint32_t fill_rows,
                       pnr_stream_t stream);
int pnr_march_rays_train_mip(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound,
                             float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                             const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                             int32_t* rays, int32_t* counter, const float* noises, void* scratch, const void* mip,
                             float* t_store /* optional [N * max_steps] floats: the counting pass keeps every sample's ray parameter there and the
                                               rows are then written 16 lanes per ray without a second walk; same outputs */,
                             pnr_stream_t stream);

/* ---------------------------------------------------------------- occupancy maintenance ----- */

/* Device-resident producer of the bitfield: replaces NeRFRenderer.update_extra_state, nerf/renderer.py:467-561
 * (= PaletteRenderer's, palette/renderer.py), whose reference form is Python over torch ops with a host read of the mean (`.item()`),
 * `nonzero`, boolean-mask scatters and raymarching.packbits (raymarching.h:11).  Per cascade c and visited cell: a jittered point
 *     p = (2 q / (H - 1) - 1) * (b_c - b_c / H) + (2 u - 1) * b_c / H,   b_c = min(2^c, bound), q = the cell's integer coordinates, u = noise
 * (fp32, operation by operation as the reference's torch expressions round on a GPU) -> sigma(p) * density_scale -> candidate of the cell;
 * then density_grid = max(density_grid * decay, candidate) where both are >= 0, mean = mean(max(density_grid, 0)),
 * bitfield = packbits(density_grid > min(mean, density_thresh)) and the brick mip of the march.  No step involves the host.
 *   mode 0 (the reference while iter_density < 16): every cell once; noise [C, H^3, 3], row = the cell's MORTON index (the order of density_grid).
 *   mode 1: per cascade n_partial uniformly drawn cells, coords int32 [C, n_partial, 3] in [0, H), followed by n_partial cells drawn from the
 *           currently occupied ones (density > 0), the k-th in ascending Morton order with k = occ_rand[c][j] % (number occupied) -- occ_rand
 *           int32 [C, n_partial] of non-negative random integers (what torch.randint reduces modulo the range); a cascade without an occupied
 *           cell skips that half (the reference raises there).  noise [C, 2 n_partial, 3] in sample order.
 * The random numbers are the CALLER's (the reference draws them with torch.rand_like / torch.randint), so two implementations can be compared.
 * Cells drawn more than once keep the LARGEST candidate (the reference keeps an unspecified one of them).
 *   pnr_occupancy_update   the whole sweep for the shipped field (16-level x 2 hash grid -> sigma_net 32 -> 64 -> 16): level-major lookup +
 *                          exact-fp32 matrix-core sigma_net (packed_sigma_net = a PNR_FIELD_FP32 blob of pnr_nerf_field_pack) + commit.
 *   any other field:       pnr_occupancy_begin; for slices of [0, pnr_occupancy_samples): pnr_occupancy_points -> caller's sigma(points)
 *                          -> pnr_occupancy_scatter; pnr_occupancy_commit.
 * points rows are float4 = world x, y, z and the global cell id c * H^3 + morton as int32 bits (-1: no sample).
 * workspace: pnr_occupancy_workspace_bytes(C, H, chunk) bytes, 256-byte aligned; `chunk` = samples in flight in pnr_occupancy_update (>= 256; the
 * other entry points need chunk 0 only).  H % 4 == 0, C <= 16, C * H^3 < 2^31.  state (optional): device float[2] = mean, threshold used. */
typedef struct pnr_occupancy_args {
    uint32_t C, H;
    float bound;
    float* density_grid;               /* [C, H^3] in/out */
    uint8_t* density_bitfield;         /* [C * H^3 / 8] out */
    void* mip;                         /* pnr_occupancy_mip_bytes(C, H) out, or NULL */
    float density_scale, decay, density_thresh;
    int mode;
    uint32_t n_partial;
    const float* noise;
    const int32_t* coords;
    const int32_t* occ_rand;
    const float* embeddings;           /* pnr_occupancy_update only: fp32 hash table [rows, 2] ... */
    const int32_t* offsets;
    uint32_t num_levels;
    float S;
    uint32_t base_resolution, gridtype;
    const float* packed_sigma_net;
    void* workspace;
    uint64_t workspace_bytes;
    float* state;
    float* points_out;                 /* pnr_occupancy_update only, optional: [samples, 4], every sample's point kept for inspection */
} pnr_occupancy_args;
uint64_t pnr_occupancy_workspace_bytes(uint32_t C, uint32_t H, uint32_t chunk);
uint32_t pnr_occupancy_samples(const pnr_occupancy_args* args);
int pnr_occupancy_update(const pnr_occupancy_args* args, pnr_stream_t stream);
int pnr_occupancy_begin(const pnr_occupancy_args* args, pnr_stream_t stream);
int pnr_occupancy_points(const pnr_occupancy_args* args, uint32_t first, uint32_t count, float* points, pnr_stream_t stream);
int pnr_occupancy_scatter(const pnr_occupancy_args* args, const float* points, const float* sigmas, uint32_t count, pnr_stream_t stream);
int pnr_occupancy_commit(const pnr_occupancy_args* args, pnr_stream_t stream);
/* replaces NeRFRenderer.mark_untrained_grid, nerf/renderer.py:395-465: cells whose centre no training camera has in its frustum (slack of one
 * cell), or that some camera sees closer than min_near (filter_close_point: or that lie within min_near of a camera), get density -1.
 * poses [B,4,4] row-major cam2world; n_marked (optional): device int32, number of cells marked. */
int pnr_mark_untrained_grid(const float* poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t C, uint32_t H, float bound, float min_near,
                            int filter_close_point, float* density_grid, int32_t* n_marked, pnr_stream_t stream);

/* Stable compaction replacing the host-side `rays_alive[rays_alive >= 0]` boolean mask
 * (nerf/renderer.py:376, palette/renderer.py:521).  Writes the surviving ids, in order, to
 * rays_alive_out and their number to n_alive_out[0].  scratch >= pnr_scan_scratch_bytes(n_alive). */
int pnr_compact_alive(uint32_t n_alive, const int32_t* rays_alive_in, int32_t* rays_alive_out,
                      int32_t* n_alive_out, void* scratch, pnr_stream_t stream);

/* ---------------------------------------------------------------- grid encoder ------------- */

/* replaces grid_encode_forward, gridencoder/src/gridencoder.h:12, gridencoder.cu:424-447.
 * dtype selects the table/outputs/dy_dx element type (PNR_DTYPE_F32 / PNR_DTYPE_F16).
 * outputs is [L,B,C] as in the reference; dy_dx may be NULL. offsets: device int32[L+1].
 * fp16 arrays (dtype PNR_DTYPE_F16: the table, outputs, dy_dx; in pnr_grid_encode_backward grad, grad_embeddings, dy_dx, grad_inputs) start on a 4-byte
 * boundary -- they move as pairs of halves, the table gradient as one 4-byte atomic per pair -- else PNR_ERR_ALIGNMENT, before anything is launched.
 * fp32 arrays need their element's alignment only. */
int pnr_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                            uint32_t gridtype, int align_corners, int dtype, pnr_stream_t stream);
/* MI355X-first addition: the same lookup with the output layout chosen by the caller.  PNR_LAYOUT_LEVELS = [L,B,C] (the reference kernel's,
 * gridencoder.cu:119); PNR_LAYOUT_ROWS = [B, L*C], what GridEncoder.forward returns after its permute-copy (gridencoder/grid.py:57) -- written
 * directly, same values.  PNR_LAYOUT_ROWS exists for D = 3, C = 2 without dy_dx (every shipped configuration); PNR_ERR_UNSUPPORTED otherwise. */
#define PNR_LAYOUT_LEVELS 0
#define PNR_LAYOUT_ROWS 1
int pnr_grid_encode_forward_layout(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                                   uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                                   uint32_t gridtype, int align_corners, int dtype, int layout, pnr_stream_t stream);
/* Two tables of the same geometry (D = 3, C = 2, fp32; the same `offsets`) at the same points in one pass: `pair_embeddings` holds them interleaved row by row,
 * [row][table 0 | table 1][2] (16-byte rows, 16-byte aligned); out0 / out1 [L, B, 2] are bit for bit what pnr_grid_encode_forward returns for table 0 / table 1.
 * (palette/network.py:156-262 looks `encoder` and `encoder_palette` up at the same x.) */
int pnr_grid_encode_forward_pair(const float* inputs, const float* pair_embeddings, const int32_t* offsets, float* out0, float* out1, uint32_t B, uint32_t L, float S,
                                 uint32_t H, uint32_t gridtype, int align_corners, pnr_stream_t stream);
/* replaces grid_encode_backward, gridencoder.h:13, gridencoder.cu:449-479.
 * grad is [L,B,C]; grad_embeddings caller-zeroed; dy_dx/grad_inputs may both be NULL. */
int pnr_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                             void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                             uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype,
                             int align_corners, int dtype, pnr_stream_t stream);

/* ---------------------------------------------------------------- fused field (MFMA) ------- */

/* MI355X-first addition, no single-call counterpart in the reference: evaluates everything
 * nerf/network.py:95-124 does after the hash-grid lookup (sigma_net 32->64->16, exp, SH degree 4, concat,
 * color_net 31->64->64->3, sigmoid) in one kernel on the fp32 matrix cores.
 *   pnr_nerf_field_pack: gathers the five bias-free nn.Linear weight matrices (row-major [out][in], device fp32)
 *                        into the MFMA-fragment-ordered blob `packed` (pnr_nerf_field_packed_bytes() bytes).  With all three colour
 *                        weights NULL only the sigma_net part is written (enough for pnr_nerf_density_forward / pnr_occupancy_update).
 *   pnr_nerf_field_forward: enc = raw [16,B,2] output of pnr_grid_encode_forward (fp32), dirs [B,3] -> sigmas [B]
 *                        (= exp(h0), NOT multiplied by density_scale), rgbs [B,3]. */
uint64_t pnr_nerf_field_packed_bytes(void);
int pnr_nerf_field_pack(const float* w_sigma0, const float* w_sigma1, const float* w_color0, const float* w_color1,
                        const float* w_color2, float* packed, int precision, pnr_stream_t stream);
int pnr_nerf_field_forward(const float* enc, const float* dirs, const float* packed, uint32_t B, float* sigmas,
                           float* rgbs, int precision, float enc_scale, pnr_stream_t stream);
/* enc_scale (here, in pnr_nerf_density_forward and in the frame / palette argument structs): a power of two the encoder features are
 * multiplied by before the split-fp16 matrix path splits them, undone exactly after the first (bias-free, positively homogeneous) stack;
 * 1 (or 0) = none.  For hash tables whose entries are tiny (the reference initialises them U(-1e-4, 1e-4), gridencoder/grid.py:107) it keeps
 * the low halves out of fp16's subnormal range.  Ignored by PNR_FIELD_FP32. */
/* sigma_net alone (NeRFNetwork.density / the frozen-geometry half of PaletteNetwork.forward: nerf/network.py:126-143,
 * palette/network.py:161-170): sigmas [B] = scale * exp(h0), geo_feat [B,15] = h[1:] (NULL: not wanted).  Same enc layout, packed blob
 * and precision modes as pnr_nerf_field_forward.  No gradient: for inference, the occupancy sweep and PaletteNeRF training (whose
 * geometry is detached). */
int pnr_nerf_density_forward(const float* enc, const float* packed, uint32_t B, float scale, float* sigmas, float* geo_feat, int precision,
                             float enc_scale, pnr_stream_t stream);

/* Device-driven inference frame of the NeRF path: the loop of nerf/renderer.py:344-380 (same n_step schedule,
 * same per-ray arithmetic, order-preserving compaction) with n_alive / n_step / step kept in a device control
 * block, so the host does not synchronise per iteration.  Outputs are the raw accumulations (weights_sum [N],
 * depth [N], image [N,3]) BEFORE the background mix / depth normalisation of nerf/renderer.py:382-383.
 * perturb (ABI 9): `noises` NULL is the unjittered frame; with `noises` the first sample of every ray is jittered as the reference's march
 * does with perturb set (raymarching.cu:927,945), in the frame's first iteration only (the loops pass `perturb if step == 0 else False`).  workspace: pnr_nerf_frame_workspace_bytes(N) bytes of device memory. */
typedef struct pnr_nerf_frame_args {
    uint32_t N;
    const float* rays_o;           /* [N,3] */
    const float* rays_d;           /* [N,3] */
    float* nears;                  /* [N]   in (pnr_near_far_from_aabb); with `aabb` set: OUT, written by the call */
    float* fars;                   /* [N]   likewise */
    const uint8_t* bitfield;       /* density bitfield, uint8[C*H^3/8] */
    const void* mip;               /* pnr_build_occupancy_mip output, or NULL */
    float bound;
    uint32_t C, H;
    float dt_gamma;
    uint32_t max_steps;
    float T_thresh;
    const float* embeddings;       /* fp32 hash table [sum T_l, 2] */
    const int32_t* offsets;        /* int32[num_levels+1] */
    uint32_t num_levels;           /* must be 16 (the fused field kernel's input width) */
    float S;                       /* log2(per_level_scale) */
    uint32_t base_resolution;
    uint32_t gridtype;             /* 0 hash, 1 tiled */
    const float* packed_weights;   /* pnr_nerf_field_pack output (packed with the same precision) */
    int field_precision;           /* PNR_FIELD_FP32 or PNR_FIELD_F16X3 */
    float density_scale;
    float* weights_sum;            /* [N]   out */
    float* depth;                  /* [N]   out */
    float* image;                  /* [N,3] out */
    void* workspace;
    uint64_t workspace_bytes;
    uint64_t* stats;               /* HOST, optional, 6 entries: [iterations, rendered samples, evaluated rows, enqueued iterations,
                                      host looks at the control block (= stream synchronisations of this frame),
                                      1 if watch_overflow saw an operand beyond fp16's range (the frame is then invalid: render it with PNR_FIELD_FP32)] */
    float* kernel_ms;              /* HOST, optional: [0] = summed HIP-event time (ms) of the grid-encode launches that did work,
                                      [1] = their number; events are recorded on `stream` around each launch */
    const int32_t* ray_order;      /* optional permutation of 0..N-1 (device): processing order of the rays, e.g. 8x8 pixel tiles per
                                      wave; NULL = as given.  The frame then runs on copies of the per-ray inputs gathered into that
                                      order; outputs are scattered back, indexed by ray id either way, and do not depend on the order */
    int finish;                    /* bit mask: apply the caller-side epilogue of run_cuda (nerf/renderer.py:382-384) before returning --
                                      bit 0: image += (1 - weights_sum) * bg_color;  bit 1: depth = max(depth - near, 0) / (far - near);
                                      bit 2 (pnr_palette_render_frame): aux_map[:, 0:3] (direct_rgb) += (1 - weights_sum) * bg_color (palette/renderer.py:529)
                                      (same fp32 operations, in the same order, as the reference's torch expressions) */
    float bg_color[3];             /* used when finish != 0 and bg_map == NULL (the reference's default is 1) */
    const float* bg_map;           /* optional per-ray background [N,3] (device) for finish */
    int table_dtype;               /* PNR_DTYPE_F32 (default) or PNR_DTYPE_F16: the reference's --fp16 tables (`embeddings` then points to halves;
                                      PaletteNeRF: embeddings_pair = both tables as interleaved halves, required without a clip head; with a
                                      clip head embeddings_triple = the three tables as pnr_interleave_tables3_half rows, required).  The lookup
                                      then reproduces the reference's half interpolation (as pnr_grid_encode_forward with dtype 1) */
    float enc_scale[3];            /* power-of-two prescale of the features of `embeddings` (PaletteNeRF: + embeddings_palette, embeddings_clip) in the
                                      split-fp16 field, see pnr_nerf_field_forward; 0 or 1 = none */
    int watch_overflow;            /* PNR_FIELD_F16X3 only: the field kernels watch the operands they split for magnitudes beyond fp16's range
                                      (65 504) and report through stats[5]; for weights whose activations the caller cannot bound (~1 VALU per operand) */
    const float* aabb;             /* optional (device, 6 floats: xmin ymin zmin xmax ymax zmax): the call computes `nears` / `fars` itself, inside its first
                                      launch, with pnr_near_far_from_aabb's arithmetic (raymarching.cu:95-148; same bits) and WRITES them to `nears` / `fars`
                                      (by ray id) -- run_cuda's near_far_from_aabb call (nerf/renderer.py:268) folded into the frame; NULL: `nears` / `fars` are inputs */
    float min_near;                /* used with `aabb` */
    float* depth_raw;              /* optional [N] out: the un-normalised depth by ray id when finish bit 1 rewrites `depth`
                                      (PaletteNeRF's depth_origin, palette/renderer.py:522) */
    const float* noises;           /* (ABI 9) optional [N] (device), indexed by RAY ID whatever `ray_order` says: the uniform [0, 1) draw per ray of
                                      march_rays(perturb=True) (raymarching/raymarching.py:388-392).  The frame's first march starts ray r at
                                      t = fmaf(clamp(near * dt_gamma, dt_min, dt_max), noises[r], near); later iterations are not jittered.  NULL: no jitter
                                      (the frame as it was before ABI 9, bit for bit; an all-zero array gives the same bits).  Read between _submit
                                      and _finish like every other input */
} pnr_nerf_frame_args;
uint64_t pnr_nerf_frame_workspace_bytes(uint32_t N);
int pnr_nerf_render_frame(const pnr_nerf_frame_args* args, pnr_stream_t stream);
/* The same frame in two calls (ABI 7).  _submit enqueues the frame's first launch, as many march iterations as the previous frame needed, the frame's last
 * launch and the 64-byte control-block read-back, and returns WITHOUT waiting: the host is free to prepare its next frame (rays, argument struct, outputs)
 * while this one runs -- the loop being replaced (nerf/renderer.py:344-380, palette/renderer.py:430-550) holds the host for the whole frame.  _finish waits for
 * the read-back, enqueues further iterations while the frame is not done (the iteration count is data) and fills `stats` / `kernel_ms`.  Rules: _finish follows
 * _submit on the same host thread, device and stream with the SAME argument struct: its address identifies the frame, and its stream, N and workspace are
 * checked -- PNR_ERR_INVALID otherwise, before anything is enqueued, and the frame stays submitted so that a correct _finish can still complete it.
 * Everything else is what _submit saw: _submit derives the frame's whole configuration once and keeps it, _finish reads no other field of the struct (nor the
 * HOST `edit` struct of a palette frame, which is copied), so a field rewritten between the two calls does not reach the frame; `stats` / `kernel_ms` are
 * written through the pointers _submit was given.  One submitted frame per host thread and device (a second _submit is PNR_ERR_INVALID; a whole-frame call
 * drops a submitted frame that was never finished); no DEVICE buffer the frame reads or writes may be touched in between.  The frame likewise keeps the
 * pnr_set_option switches _submit saw (aux_fusion, composite_fusion, hosted_tail, march_budget, march_budget0, march_blocks, iteration_margin,
 * dynamic_tiles, block_skip, coop_march, palette_waves12, grid_lane_pairs): a pnr_set_option between the two calls applies from the next frame on.
 * pnr_nerf_render_frame == _submit + _finish.  (`noises` is read by the frame's first iteration, which _submit enqueues: it is one more input the caller
 * leaves alone until _finish.) */
int pnr_nerf_render_frame_submit(const pnr_nerf_frame_args* args, pnr_stream_t stream);
int pnr_nerf_render_frame_finish(const pnr_nerf_frame_args* args, pnr_stream_t stream);

/* Appearance editing heads of the PaletteNeRF inference loop, evaluated inside the fused field kernel's epilogue (HOST struct).
 *   mode 1  RegionEdit.forward (palette/renderer.py:121-147): per basis, final colour -> HSV (pnr_rgb_to_hsv's arithmetic), hue += delta_hsv[b][0]
 *           (+360, fmod 360), saturation / value *= delta_hsv[b][1..2] (clipped at 0), -> RGB, then lerp(original, edited, weight) with
 *           weight = exp(-|xyz - mean_xyz|^2 / std_xyz) * exp(-|clip_feat - mean_clip|^2 / std_clip) (each factor only when its mean is set);
 *           weight_mode != 0 returns the weight itself in every channel (the GUI's region preview).
 *   mode 2  Stylizer.forward (palette/renderer.py:166-183): rgb = sum_b omega_b clamp(max(softplus(r) + dI_b, 0) (P_b + dP_b + offsets_b . ddelta_b), 0, 1)
 *           + view_dep  (offsets_weight / view_dep_weight do not apply, as in the reference).
 *   mode 3  (pnr_palette_field_forward only) "network heads": no composite at all -- the aux row is what PaletteNetwork.forward returns per sample
 *           (palette/network.py:156-190): omega nb (normalised) | offsets_radiance 3 nb + 1 (raw, bias added) | view_dep 3 | diffuse 3 |
 *           clip_feat clip_dim | 0-pad; sigmas = density_scale * exp(logit), rgbs = 0.  For callers that keep the reference's own renderer
 *           arithmetic (palette/renderer.py:452-499) and only want the network as one launch (palettenerf_amd.dropin.fuse_field). */
#define PNR_MAX_BASIS 10
#define PNR_MAX_CLIP 32
typedef struct pnr_palette_edit {
    int mode;                                /* 0 none, 1 RegionEdit, 2 Stylizer, 3 network heads (stand-alone op only) */
    float delta_hsv[PNR_MAX_BASIS][3];
    int has_mean_xyz;  float mean_xyz[3];  float std_xyz;
    int has_mean_clip; float mean_clip[PNR_MAX_CLIP]; float std_clip;   /* has_mean_clip = number of entries (the model's clip_dim), 0 = not set */
    int weight_mode;
    float dI[PNR_MAX_BASIS]; float dP[PNR_MAX_BASIS][3]; float ddelta[PNR_MAX_BASIS][3][3];
} pnr_palette_edit;

/* The same device-driven loop for the PaletteNeRF model (palette/renderer.py:430-550, RegionEdit / Stylizer included through `edit`):
 * `base.embeddings` is the `encoder` table, `base.packed_weights` the pnr_palette_field_pack blob (packed with base.field_precision:
 * PNR_FIELD_F16X3 or the exact PNR_FIELD_FP32).  num_basis <= PNR_MAX_BASIS, clip_dim <= PNR_MAX_CLIP.
 * aux_map [N, pnr_palette_aux_channels(nb, clip_dim)] receives the composited packed row
 * direct_rgb 3 | view_dep 3 | basis_acc nb | basis_rgb 3nb | unscaled_basis_rgb 3nb | clip_feat clip_dim | pad
 * (raw accumulations: the background mix of direct_rgb is the caller's, palette/renderer.py:541). */
typedef struct pnr_palette_frame_args {
    pnr_nerf_frame_args base;
    const float* embeddings_palette;   /* `encoder_palette` table (same offsets / level parameters as `encoder`) */
    const float* embeddings_clip;      /* `encoder_clip` table (pred_clip only) */
    uint32_t num_basis, clip_dim;
    int pred_clip;
    float offsets_weight, view_dep_weight;
    float* aux_map;                    /* [N, aux channels] out */
    const float* embeddings_pair;      /* optional: `encoder` and `encoder_palette` interleaved row by row ([rows][4] floats, built by
                                          pnr_interleave_tables; rebuild when either table changes).  Used when pred_clip == 0: one 16-byte
                                          gather serves both tables, results bit-identical to the separate lookups */
    const float* embeddings_triple;    /* optional, pred_clip != 0: all three tables interleaved ([rows][8] floats: encoder, encoder_palette,
                                          encoder_clip, 2 pad; pnr_interleave_tables3): one 32-byte row per corner, bit-identical results.
                                          With base.table_dtype == PNR_DTYPE_F16 (required then): [rows][8] HALVES instead, built by
                                          pnr_interleave_tables3_half -- one 16-byte row per corner */
    const pnr_palette_edit* edit;      /* HOST, optional: RegionEdit / Stylizer applied to every sample (NULL or mode 0: none) */
} pnr_palette_frame_args;
/* out[i] = (a[i].x, a[i].y, b[i].x, b[i].y) for two C = 2 fp32 tables of `rows` rows with the same level layout */
int pnr_interleave_tables(const float* a, const float* b, uint64_t rows, float* out, pnr_stream_t stream);
/* a, b, c: [rows][2] fp32 -> out [rows][8] = (a.x, a.y, b.x, b.y, c.x, c.y, 0, 0): the --pred_clip model's three lookups from one 32-byte row */
int pnr_interleave_tables3(const float* a, const float* b, const float* c, uint64_t rows, float* out, pnr_stream_t stream);
/* (ABI 8) a, b, c: [rows][2] fp32 -> out [rows][8] fp16 = (a.x, a.y, b.x, b.y, c.x, c.y, 0, 0), each value rounded to nearest even (the bits of
 * tensor.to(torch.float16): beyond fp16's range -> inf): the --pred_clip model's three fp16 lookups from one 16-byte row (embeddings_triple with
 * table_dtype PNR_DTYPE_F16) */
int pnr_interleave_tables3_half(const float* a, const float* b, const float* c, uint64_t rows, void* out, pnr_stream_t stream);
uint64_t pnr_palette_frame_workspace_bytes(uint32_t N, uint32_t num_basis, uint32_t clip_dim, int pred_clip);
int pnr_palette_render_frame(const pnr_palette_frame_args* args, pnr_stream_t stream);
int pnr_palette_render_frame_submit(const pnr_palette_frame_args* args, pnr_stream_t stream);   /* as pnr_nerf_render_frame_submit / _finish */
int pnr_palette_render_frame_finish(const pnr_palette_frame_args* args, pnr_stream_t stream);

/* Fused PaletteNeRF field + palette colour-basis composite (palette/network.py:156-280, palette/renderer.py:470-500, RegionEdit /
 * Stylizer included).  Split-fp16 or exact-fp32 matrix path (`precision`).  All weights are row-major [out][in]
 * device fp32 pointers of the bias-free nn.Linear layers; offsets_radiance has a bias; the palette (basis_color) and that bias are packed too. */
typedef struct pnr_palette_weights {
    const float *sigma0, *sigma1;              /* [64,32], [16,64]            */
    const float *diff0, *diff1, *diff2;        /* [64,15], [64,64], [3,64]    */
    const float *color0, *color1, *color2;     /* [64,31], [64,64], [3,64]    */
    const float *basis0, *basis1;              /* [64,35], [15,64]            */
    const float *offsets_radiance;             /* [3 nb + 1, 15]              */
    const float *omega;                        /* [nb, 15]                    */
    const float *clip0, *clip1;                /* [64,32], [clip_dim,64] (pred_clip only) */
    const float *basis_color;                  /* [nb,3] the palette (device; clamped to [0,1] at pack time, palette/renderer.py:480) */
    const float *or_bias;                      /* [3 nb + 1] offsets_radiance_net.bias (device) */
    uint32_t num_basis, clip_dim;              /* nb <= PNR_MAX_BASIS, clip_dim <= PNR_MAX_CLIP */
    int pred_clip;
    int precision;                             /* PNR_FIELD_F16X3 or PNR_FIELD_FP32: number format of the packed blob */
} pnr_palette_weights;
typedef struct pnr_palette_field_args {
    const void* ctl;               /* NULL for the stand-alone op (rows = B); internal frame control block otherwise */
    uint32_t B;                    /* rows */
    const float* enc;              /* [16, level_stride, 2] raw grid output of `encoder` */
    const float* enc_palette;      /* same for `encoder_palette` */
    const float* enc_clip;         /* same for `encoder_clip` (pred_clip only) */
    uint32_t level_stride;
    const float* dirs;             /* [B,3] */
    const float* deltas;           /* [B,2] or NULL; rows with deltas[:,0] == 0 are skipped */
    const void* packed;            /* pnr_palette_field_pack output (weights, palette and bias) */
    uint32_t num_basis, clip_dim;
    int pred_clip;
    float density_scale, offsets_weight, view_dep_weight;
    uint32_t aux_stride;           /* floats per aux row, >= pnr_palette_aux_channels(nb, clip_dim) semantics below */
    float* sigmas;                 /* [B]   = density_scale * exp(h0) */
    float* rgbs;                   /* [B,3] */
    float* aux;                    /* [B, aux_stride] = direct_rgb 3 | view_dep 3 | omega nb | basis_rgb 3nb | unscaled 3nb | clip | 0 pad */
    /* frame loop only (ctl != NULL), all three or none: in iterations with one sample per ray (ctl->n_step == 1) the aux row is
     * composited straight into aux_map (aux_map[ray] += weight * row, the arithmetic of composite_rays_flex) instead of being written
     * to `aux` and read back by the composite launch -- when the kernel can stage the tile in LDS (pnr_palette_field_stages_aux);
     * likewise with 2, 4 or 8 samples per ray (a ray's rows then sit in one 32-row tile) */
    const int32_t* rays_alive;     /* [n_alive] ray id of every slot */
    const float* weights_sum;      /* [N] of BEFORE this iteration */
    float* aux_map;                /* [N, aux_stride] */
    float T_thresh;                /* early-termination threshold of the composite (frame loop only) */
    int precision;                 /* PNR_FIELD_F16X3 / PNR_FIELD_FP32, as the blob was packed */
    const pnr_palette_edit* edit;  /* HOST, optional */
    const float* xyzs;             /* [B,3] world positions of the samples: needed by RegionEdit's spatial window (edit->has_mean_xyz) */
    const void* edit_device;       /* internal (frame loop): the edit parameters already on the device; NULL for callers */
    float enc_scale[3];            /* power-of-two prescales of enc / enc_palette / enc_clip in the split-fp16 path (0 or 1 = none) */
    int32_t* overflow_flag;        /* optional (device): set to 1 when a split-fp16 operand exceeds fp16's range (the kernel then watches its operands) */
    void* tile_counter;            /* internal (frame loop): device uint32, zero at launch -- waves fetch their 32-sample tiles from it; NULL = static schedule */
    /* internal (frame loop), all or none: with these the kernel also does the ray-state half of the iteration's compositing step (what the frame loop's
     * composite launch did): weights_sum / depth / image / rays_t of every ray, the alive list's holes, the per-chunk survivor counts */
    float* rays_t;                 /* [N] */
    float* weights_sum_rw;         /* [N] = weights_sum */
    float* depth;                  /* [N] */
    float* image;                  /* [N,3] */
    int32_t* rays_alive_rw;        /* [n_alive] = rays_alive */
    int32_t* counts_cur;           /* [chunks] survivors per 256-ray chunk of the alive list, cleared by the iteration's march launch */
} pnr_palette_field_args;
int pnr_palette_field_stages_aux(uint32_t num_basis, uint32_t clip_dim, int pred_clip);   /* 1 when the field kernel stages aux rows in LDS (then it can composite them) */
uint64_t pnr_palette_field_packed_bytes(uint32_t num_basis, uint32_t clip_dim, int pred_clip);
uint32_t pnr_palette_aux_channels(uint32_t num_basis, uint32_t clip_dim);   /* 6 + 7 nb + clip_dim rounded up to a multiple of 4 */
int pnr_palette_field_pack(const pnr_palette_weights* weights, void* packed, pnr_stream_t stream);
int pnr_palette_field_forward(const pnr_palette_field_args* args, pnr_stream_t stream);

/* ---------------------------------------------------------------- SH encoder --------------- */

/* replaces sh_encode_forward / sh_encode_backward, shencoder/src/shencoder.h:9-10, shencoder.cu:400-439.
 * fp32 only (the reference's Python forces fp32, sphere_harmonics.py:16). dy_dx may be NULL. */
int pnr_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D, uint32_t C, float* dy_dx,
                          pnr_stream_t stream);
/* color_net's input rows [SH(dirs) | tail] = torch.cat([encoder_dir(d), geo_feat], dim=-1) (nerf/network.py:109-115, palette/network.py:248-249) in one
 * launch: inputs [B,3] unit directions, tail [B,tail_cols] -> outputs [B, C*C + tail_cols]; the SH columns are pnr_sh_encode_forward's bits.
 * C*C + tail_cols <= 64.  (No Jacobian: directions get no gradient on this path; the tail's gradient is the column slice of the output's.) */
int pnr_sh_encode_cat_forward(const float* inputs, const float* tail, uint32_t tail_cols, float* outputs, uint32_t B, uint32_t C,
                              pnr_stream_t stream);
/* The seam between sigma_net and color_net of the NeRF field in training (nerf/network.py:109-121: `sigma = trunc_exp(h[..., 0])`, `geo_feat = h[..., 1:]`,
 * `torch.cat([encoder_dir(d), geo_feat], -1)`) as one launch each way, so that autograd does not zero-fill, slice-copy and add two [B, hw] gradients:
 *   forward   h [B, hw] row-major, dirs [B, 3]  ->  sigma [B] = exp(h[:, 0]),  out [B, C*C + hw - 1] = [SH_C(dirs), h[:, 1:]]
 *   backward  grad_h [B, hw] = [dsigma * exp(clamp(h[:, 0], -15, 15)), dout[:, C*C:]]   (activation.py:14-17; dsigma / dout may be NULL = zeros) */
int pnr_sigma_geo_cat_forward(const float* h, uint32_t hw, const float* dirs, uint32_t C, uint32_t B, float* sigma, float* out, pnr_stream_t stream);
int pnr_sigma_geo_cat_backward(const float* h, uint32_t hw, const float* dsigma, const float* dout, uint32_t C, uint32_t B, float* grad_h, pnr_stream_t stream);
int pnr_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D, uint32_t C,
                           const float* dy_dx, float* grad_inputs, pnr_stream_t stream);

/* Table gradient of the hash grid for D = 3, C = 2, fp32 (the shipped fields) without global atomics in the inner loop: records are
 * binned by 8192-row table bucket, each bucket is accumulated in LDS and added to the table once (csrc/grid_binned.hip).  Same
 * contract as the embeddings part of pnr_grid_encode_backward (gridencoder.cu:216-286: grad [L,B,C] level-major, accumulates into
 * the caller-zeroed grad_embeddings); total_rows = rows of the table (offsets[L]); other shapes return PNR_ERR_UNSUPPORTED (use
 * pnr_grid_encode_backward).  workspace: pnr_grid_backward_binned_workspace_bytes(B, L, total_rows) bytes (10 B per record). */
uint64_t pnr_grid_backward_binned_workspace_bytes(uint32_t B, uint32_t L, uint64_t total_rows);
int pnr_grid_encode_backward_binned(const float* grad, const float* inputs, const int32_t* offsets, float* grad_embeddings, uint32_t B, uint32_t D,
                                    uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, uint64_t total_rows,
                                    void* workspace, uint64_t workspace_bytes, pnr_stream_t stream);

/* ---------------------------------------------------------------- training: dense-layer weight gradient */

/* dW[o][i] (+)= sum_b dY[b][o] * X[b][i]: the weight gradient autograd computes for every nn.Linear(in, out, bias=False) of the
 * fields (nerf/network.py:60-93, palette/network.py:60-153; torch sends it to the BLAS library in the reference).
 *   x [B, in_dim], dy [B, out_dim] row-major, fp32 or fp16 (PNR_DTYPE_*; autocast hands over halves), dw [out_dim, in_dim] fp32;
 *   in_dim, out_dim <= 64 (every layer of both models), else PNR_ERR_UNSUPPORTED; accumulate != 0 adds to dw;
 *   workspace: pnr_linear_wgrad_workspace_bytes(B, in_dim, out_dim) bytes of device memory (per-workgroup partials, reduced in a
 *   fixed order: the result is deterministic).  Products and sums are fp32 (v_mfma_f32_32x32x2_f32). */
uint64_t pnr_linear_wgrad_workspace_bytes(uint32_t B, uint32_t in_dim, uint32_t out_dim);
int pnr_linear_wgrad(const void* x, int x_dtype, const void* dy, int dy_dtype, uint32_t B, uint32_t in_dim, uint32_t out_dim, float* dw,
                     int accumulate, void* workspace, uint64_t workspace_bytes, pnr_stream_t stream);
/* The fields' small bias-free MLPs for TRAINING as one launch forward and one launch backward (replaces the nn.Linear(bias=False) stacks
 * of nerf/network.py:33-93 and palette/network.py:60-153 under autograd: per layer a GEMM + activation kernel forward, two GEMMs + an
 * activation kernel backward).  2 or 3 layers, every width <= 64, hidden activation 0 = ReLU, 1 = ELU(alpha 1), optionally torch.sigmoid on the output;
 * fp32 (exact fma chains on v_mfma_f32_32x32x2_f32).  weights w_l are [dims[l+1]][dims[l]] row-major as nn.Linear stores them.
 *   pnr_mlp_pack      weights -> MFMA-ordered blob of pnr_mlp_packed_bytes (W_l and W_l^T, once as fp32 and once as split-fp16 pairs scaled by one power
 *                     of two per layer); call again after every optimiser step
 *   The forward runs on the fp16 matrix pipe with split operands (22-bit products, fp32 accumulation, per-tile power-of-two scaling; outputs within 2e-6
 *   of the exact launch relative to the largest output); pnr_set_option("mlp_f16x3", 0) selects the exact fp32 instructions.  The backward runs in
 *   the same split-fp16 arithmetic (k_mlp_bwd_h) for the shapes whose tile it holds without scratch -- two layers unless both ends are 64 wide, three
 *   layers with ends <= 32 wide: every stack of both fields -- and on the exact fp32 instructions otherwise, so a wide stack's forward (split-fp16) and
 *   backward (fp32) differ in arithmetic; gradients of both agree with the exact launches to 2e-6 of the largest entry (profiles/r04_grad_tolerance.txt).
 *   pnr_mlp_forward   x [B, dims[0]] -> y [B, dims[n_layers]]
 *   pnr_mlp_backward  x, dy [B, dims[n_layers]] -> dx [B, dims[0]] (NULL: not wanted), dw_l [dims[l+1]][dims[l]] (NULL: not wanted);
 *                     hidden activations are recomputed from x; dw is reduced deterministically through `workspace`.
 *                     y: the forward's output, read only with PNR_MLP_OUT_SIGMOID (dZ = dY (1 - y) y; NULL otherwise).
 *   A row-major activation array is at least two columns wide: dims[0] == 1 (plain forms), dims[n_layers] == 1 and a one-column x_tail (dims[0] == 33 in the
 *   level-major forms) are PNR_ERR_UNSUPPORTED -- the tile moves divide element indices by the width with a 32-bit reciprocal, which width 1 does not have.
 *   Every activation array (x, x_tail, y, dy, dx; the level-major forms' enc / denc) must start on a 16-byte boundary and hold at least four floats -- tiles move
 *   as 16-byte requests (round 5); PNR_ERR_ALIGNMENT otherwise (a contiguous view such as x[1:] of a 3-wide tensor starts inside an allocation: copy it). */
typedef struct {
    uint32_t n_layers;      /* 2 or 3 */
    uint32_t dims[4];       /* dims[0] = input width ... dims[n_layers] = output width, each 1..64 */
    int activation;         /* between layers: 0 ReLU, 1 ELU;  | PNR_MLP_OUT_SIGMOID: torch.sigmoid on the last layer's output as well */
} pnr_mlp_desc;
#define PNR_MLP_OUT_SIGMOID 0x100   /* colour heads: torch.sigmoid(h) behind color_net / diff_net (nerf/network.py:122, palette/network.py:245,254) */
uint64_t pnr_mlp_packed_bytes(const pnr_mlp_desc* desc);
int pnr_mlp_pack(const pnr_mlp_desc* desc, const float* w0, const float* w1, const float* w2, float* packed, pnr_stream_t stream);
int pnr_mlp_forward(const pnr_mlp_desc* desc, const float* packed, const float* x, uint32_t B, float* y, pnr_stream_t stream);
uint64_t pnr_mlp_backward_workspace_bytes(const pnr_mlp_desc* desc, uint32_t B);
int pnr_mlp_backward(const pnr_mlp_desc* desc, const float* packed, const float* x, const float* y, const float* dy, uint32_t B, float* dx, float* dw0,
                     float* dw1, float* dw2, void* workspace, uint64_t workspace_bytes, pnr_stream_t stream);

/* The same with the first 32 input columns taken straight from a hash-grid encoder output in its native level-major layout
 * enc [16][B][2] (pnr_grid_encode_forward's `outputs`) and the remaining dims[0] - 32 columns from a row-major x_tail [B, dims[0]-32]
 * (NULL when dims[0] == 32): replaces `torch.cat([encoder(x), tail])` + the [L,B,C] -> [B,L*C] copy of gridencoder/grid.py:51-52 in
 * front of sigma_net (nerf/network.py:99-101) and basis_net (palette/network.py:257-260).  The backward returns the encoder part of dX in
 * level-major layout too (what pnr_grid_encode_backward[_binned] takes as `grad`); the tail gets no gradient (the reference detaches it). */
int pnr_mlp_forward_lm(const pnr_mlp_desc* desc, const float* packed, const float* enc_level_major, uint32_t levels, const float* x_tail, uint32_t B, float* y,
                       pnr_stream_t stream);
int pnr_mlp_backward_lm(const pnr_mlp_desc* desc, const float* packed, const float* enc_level_major, uint32_t levels, const float* x_tail, const float* dy,
                        uint32_t B, float* denc_level_major, float* dw0, float* dw1, float* dw2, void* workspace, uint64_t workspace_bytes,
                        pnr_stream_t stream);

/* bias gradient of a dense layer with bias (palette/network.py:111 offsets_radiance_net, the only one): db[o] = sum_b dY[b][o];
 * workspace of pnr_linear_wgrad_workspace_bytes(B, 1, out_dim) */
int pnr_linear_bgrad(const void* dy, int dy_dtype, uint32_t B, uint32_t out_dim, float* db, int accumulate, void* workspace, uint64_t workspace_bytes,
                     pnr_stream_t stream);

/* ---------------------------------------------------------------- training: optimiser step -- */

/* torch.optim.Adam (the reference's optimiser: main_nerf.py:113, main_palette.py:223 -- lr 1e-2, betas (0.9, 0.99), eps 1e-15, no weight decay,
 * no amsgrad) for up to pnr_adam_max_tensors() fp32 tensors in ONE launch: read p, g, m, v -- write p, m, v, once.  Bit-identical to torch's
 * seven elementwise kernels per tensor (same operations, roundings and contractions; torch/optim/adam.py:_single_tensor_adam).  The scalars are
 * the ones torch forms on the host, narrowed to fp32 where its kernels narrow them:
 *   one_minus_beta1 = (float)(1 - beta1), one_minus_beta2 = (float)(1 - beta2), neg_step_size = (float)(-(lr / (1 - beta1^step))),
 *   bias_correction2_sqrt = (float)((1 - beta2^step) ** 0.5)   (torch's default foreach implementation divides by it; option "adam_variant" bit 0
 *   multiplies by its fp32 reciprocal instead, as torch's single-tensor kernels do for a division by a host scalar),
 *   inv_grad_scale: 1, or 1 / GradScaler's scale to fold `unscale_` into the same pass. */
typedef struct pnr_adam_tensor { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; uint64_t n; } pnr_adam_tensor;   /* HOST array of device pointers */
typedef struct pnr_adam_scalars { float one_minus_beta1, beta2, one_minus_beta2, bias_correction2_sqrt, eps, neg_step_size, inv_grad_scale; } pnr_adam_scalars;
uint32_t pnr_adam_max_tensors(void);
int pnr_adam_step(const pnr_adam_tensor* tensors, uint32_t count, const pnr_adam_scalars* scalars, pnr_stream_t stream);

/* The loss-scaled (-O: fp16 autocast + GradScaler) step without a read-back: what torch.amp.GradScaler.step + torch.optim.Adam compute, skipped
 * steps included, bit for bit, in two launches that never return to the host.
 *
 * pnr_grad_check: GradScaler's finite test on the SCALED gradients of up to pnr_adam_max_tensors() tensors in one launch (only `grad` and `n` of
 * every entry are used).  Every element is read once; the only store is *found_inf = 1.0f where an element is inf or nan.  It never clears the
 * flag: the caller zeroes it once per step, so several launches (more than the cap of tensors) accumulate into one flag.
 *
 * pnr_adam_step_amp: pnr_adam_step under a device control block (pnr_adam_amp_ctl, a HOST struct of device pointers):
 *   scale      torch's GradScaler._scale (fp32); the gradients are multiplied by (float)(1.0 / (double)*scale), torch's
 *              _scale.double().reciprocal().float(), whatever inv_grad_scale the rows carry
 *   found_inf  the flag of pnr_grad_check: non-zero = every workgroup returns without a store to any tensor
 *   state      int32[3]: {skipped, skipped, error}.  The number of steps skipped so far is a ping-pong pair: the launches of one step read
 *              state[parity & 1] and each writes state[(parity & 1) ^ 1] = state[parity & 1] + (*found_inf != 0) (the same value from every launch
 *              of the step); the caller flips `parity` from one step to the next.  state[2] is the error word (below).
 *   skipped_base, parity   by value
 * The bias corrections of Adam are doubles the host forms from the true step count, which a skipped step does not advance -- and the host does
 * not know about a skip without reading back.  So it passes n_rows (1..8) rows of scalars, row r formed for a step count r lower than its
 * optimistic one, and the device takes rows[skipped - skipped_base]: no pow on the device, and the update stays torch's bits.  A row index
 * outside [0, n_rows) on a finite step leaves every tensor untouched and sets state[2] = 1 (a guard: the caller bounds how far it runs ahead of
 * its last look at `skipped` by n_rows).  NULL pointers: PNR_ERR_INVALID; count above the cap, n_rows 0 or above 8: PNR_ERR_UNSUPPORTED; tensors
 * with n == 0 are skipped. */
typedef struct pnr_adam_amp_ctl { const float* scale; const float* found_inf; int32_t* state; int32_t skipped_base; int32_t parity; } pnr_adam_amp_ctl;
int pnr_grad_check(const pnr_adam_tensor* tensors, uint32_t count, float* found_inf, pnr_stream_t stream);
int pnr_adam_step_amp(const pnr_adam_tensor* tensors, uint32_t count, const pnr_adam_scalars* rows, uint32_t n_rows, const pnr_adam_amp_ctl* ctl,
                      pnr_stream_t stream);

/* The weights' average: torch_ema.ExponentialMovingAverage, which every recipe of the reference keeps over all model parameters
 * (main_nerf.py:151, main_palette.py:228: ema_decay 0.95), for up to pnr_adam_max_tensors() fp32 tensors in ONE launch over pnr_adam_step's
 * chunk table (additive entries, ABI still 10).
 *
 * pnr_ema_update: every element reads param and shadow and writes shadow, once: s' = s - fl(fl(s - p) * one_minus_decay), torch_ema's three
 * elementwise kernels per tensor (tmp = s - p; tmp.mul_(w); s.sub_(tmp)) rounding for rounding -- the product and the subtraction are not
 * contracted into one fma.  one_minus_decay is the fp32 narrowing of the host double 1.0 - decay, as torch narrows the scalar of mul_.
 *
 * pnr_ema_swap: exchanges param and shadow in place, two reads and two writes per element: `store(); copy_to()` before an evaluation and, called
 * again, `restore()` after it, without a third copy of any tensor.
 *
 * count == 0: PNR_OK.  A NULL array, or a NULL param / shadow in a tensor with n > 0: PNR_ERR_INVALID; count above the cap: PNR_ERR_UNSUPPORTED;
 * tensors with n == 0 are skipped.  param and shadow of one tensor must not overlap. */
typedef struct pnr_ema_tensor { float* param; float* shadow; uint64_t n; } pnr_ema_tensor;   /* HOST array of device pointers */
int pnr_ema_update(const pnr_ema_tensor* tensors, uint32_t count, float one_minus_decay, pnr_stream_t stream);
int pnr_ema_swap(const pnr_ema_tensor* tensors, uint32_t count, pnr_stream_t stream);

/* ---------------------------------------------------------------- cache guard -------------- */

/* 64-bit checksums of `count` (<= 24) device buffers in one launch: buffers / nbytes / word_stride are HOST arrays (device pointers, sizes in
 * bytes -- multiples of 4 --, and the stride in 4-byte words at which a buffer is sampled: 1 or 0 = every word); out = device uint64[count].
 * Order-independent sums of position-dependent word hashes: deterministic.  Used by the frame loops to notice that the parameters a packed
 * blob was derived from were rewritten behind torch's version counters (`p.data` writes: torch_ema's copy_to / restore, nerf/utils.py:829-839). */
int pnr_checksum(const void* const* buffers, const uint64_t* nbytes, const uint32_t* word_stride, uint32_t count, uint64_t* out, pnr_stream_t stream);

/* ---------------------------------------------------------------- ray generation ----------- */

/* device counterpart of the deterministic core of get_rays (nerf/utils.py:53-149; torch ops on the GPU in the reference):
 * pinhole rays through pixel centres (+0.5), normalised, rotated by the camera-to-world pose.
 *   poses [B,4,4] row-major cam2world; intrinsics = fx, fy, cx, cy (utils.py:67); inds [B,N] int64 flat pixel ids (y*W + x) or
 *   NULL = all H*W pixels in row-major order (then N must be H*W); outputs rays_o, rays_d [B,N,3].
 * Scalar spec (same in the oracle): xs = ((x + 0.5) - cx) / fx, ys likewise, n = sqrt(fma(xs,xs, fma(ys,ys, 1))),
 * d = (xs/n, ys/n, 1/n), rays_d[k] = fma(d2,R[k][2], fma(d1,R[k][1], d0*R[k][0])), rays_o[k] = pose[k][3].
 * The index selection (random / patch / error-map sampling, utils.py:75-131) stays on the torch side. */
int pnr_get_rays(const float* poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, const int64_t* inds,
                 uint32_t N, float* rays_o, float* rays_d, pnr_stream_t stream);

/* The frame's last step on the way to the video / PNG writer (nerf/utils.py:719-723, 1013-1017: `(pred * 255).astype(np.uint8)` on the
 * host, after `linear_to_srgb` when the scene is in linear colour, utils.py:43-44, 1010-1011): fp32 values -> uint8 on the device, so that
 * a frame leaves the GPU as 3 bytes per pixel.  u8 = (uint8)(v * 255) (truncation, as numpy's astype for in-range values);
 * linear_to_srgb != 0: v = v < 0.0031308 ? 12.92 v : 1.055 v^0.41666 - 0.055 first. */
int pnr_image_to_uint8(const float* src, uint64_t n, int linear_to_srgb, uint8_t* dst, pnr_stream_t stream);

/* (ABI 9) The viewer's step behind a frame -- test_gui (palette/utils.py:1106-1119, nerf/utils.py likewise) and the still camera's running mean
 * (palette/gui.py:225-231) -- in one launch: the maps rendered at src_h x src_w -> the display maps at dst_h x dst_w, fp32, on the device.
 *   out_image [dst,3]  = nearest(clamp(image, 0, 1)), then linear->sRGB when linear_to_srgb (pnr_image_to_uint8's arithmetic)
 *   out_depth [dst]    = nearest(depth)
 *   out_xyz   [dst,3]  = nearest(rays_o + rays_d * depth_origin)   optional (NULL: none; else rays_o, rays_d, depth_origin are required)
 *   out_clip  [dst,clip_dim] = nearest(clip_feat)                  optional (NULL: none); clip_feat rows are clip_stride floats apart (a view
 *                        into the frame's aux map is fine), moved 16 bytes at a time when row start, stride and clip_dim allow, 8 or 4 otherwise
 *   accum     [dst,3]  optional, caller-owned: spp == 0: accum = out_image; else accum = (accum * spp + out_image) / (spp + 1)
 * nearest: source index min((int)floorf(dst * ((float)in / out)), in - 1) per axis, as F.interpolate(size=..., mode='nearest'); equal sizes: identity.
 * Same fp32 operations in the same order as the torch expressions: the maps are bit-identical to them (the sRGB branch to an ulp of powf).
 * Returns PNR_OK for an empty destination (nothing is read), PNR_ERR_INVALID for a missing map or a zero source size. */
typedef struct pnr_present_args {
    uint32_t src_h, src_w, dst_h, dst_w;
    const float* image;            /* [src,3] */
    const float* depth;            /* [src]   normalised depth */
    const float* rays_o;           /* [src,3] with out_xyz */
    const float* rays_d;           /* [src,3] with out_xyz */
    const float* depth_origin;     /* [src]   with out_xyz: the un-normalised depth (pnr_nerf_frame_args::depth_raw) */
    const float* clip_feat;        /* [src] rows of clip_dim floats, clip_stride floats apart, with out_clip */
    uint32_t clip_dim, clip_stride;
    int linear_to_srgb;
    float* out_image;
    float* out_depth;
    float* out_xyz;
    float* out_clip;
    float* accum;
    uint32_t spp;                  /* frames already in `accum` */
} pnr_present_args;
int pnr_present_frame(const pnr_present_args* args, pnr_stream_t stream);

/* ---------------------------------------------------------------- palette ------------------ */

/* Training-mode palette colour-basis composite as one launch each way (replaces the ~40 torch launches of palette/renderer.py:344-386
 * between PaletteNetwork.forward and composite_rays_train / composite_rays_flex_train; same arithmetic):
 *   omega [M,nb], offsets_radiance [M,3nb+1] (offsets, then radiance), view_dep [M,3], diffuse [M,3], clip_feat [M,clip_dim] or NULL (zeros),
 *   smooth_norm [M] or NULL (zeros), basis_color [nb,3] (the unclamped parameter)
 *   -> rgbs [M,3] = sum_b omega_b softplus(radiance) (clamp(P_b,0,1) + offsets_b) + view_dep
 *      all_buffer [M, 13+clip_dim+nb] = omega_sparsity, view_dep_norm, offsets_norm, smooth_norm, view_dep, diffuse+view_dep, diffuse, clip_feat, omega
 * backward: grad_rgbs [M,3], grad_all [M,13+clip_dim+nb] -> gradients of every input (view_dep gets none through rgbs: the reference detaches
 * it there); grad_clip_feat / grad_smooth_norm / grad_basis_color may be NULL (not wanted).  grad_basis_color [nb,3] is reduced
 * deterministically through `workspace` (pnr_palette_train_shade_workspace_bytes).  nb <= 16. */
uint64_t pnr_palette_train_shade_workspace_bytes(uint32_t num_basis);
int pnr_palette_train_shade_forward(uint32_t M, uint32_t num_basis, uint32_t clip_dim, const float* omega, const float* offsets_radiance,
                                    const float* view_dep, const float* diffuse, const float* clip_feat, const float* smooth_norm,
                                    const float* basis_color, float* rgbs, float* all_buffer, pnr_stream_t stream);
int pnr_palette_train_shade_backward(uint32_t M, uint32_t num_basis, uint32_t clip_dim, const float* omega, const float* offsets_radiance,
                                     const float* view_dep, const float* basis_color, const float* grad_rgbs, const float* grad_all,
                                     float* grad_omega, float* grad_offsets_radiance, float* grad_view_dep, float* grad_diffuse,
                                     float* grad_clip_feat, float* grad_smooth_norm, float* grad_basis_color, void* workspace,
                                     uint64_t workspace_bytes, pnr_stream_t stream);

/* The smooth-loss block of a training step (palette/renderer.py:360-378; every step from smooth_loss_start_epoch on) as one launch for the
 * perturbed points, one for the bilateral weight and the norm, one for the gradient (replaces ~25-30 torch launches each way; additive
 * entries, the ABI version does not change).  All arrays fp32, row-major.
 *   pnr_palette_smooth_points: xyzs [M,3], noise [M,3] (torch.rand_like) -> xyzs_diff [M,3] = clamp(xyzs + noise * bound * 0.03, -bound, bound),
 *     evaluated in torch's order (noise * bound, * 0.03f, the add, the clamp; no contraction): the same bits as the torch expression (:362).
 *   pnr_palette_smooth_forward: xyzs / xyzs_diff [M,3], diffuse / diffuse_diff [M,3], omega / omega_diff [M,nb], clip_feat / clip_feat_diff
 *     [M,clip_dim] or both NULL (no clip head: opt.pred_clip off) -> smooth_weight [M] (kept for the backward), smooth_norm [M]:
 *       xw = |xyzs - xyzs_diff|^2 / bound^2 / sigma_xyz          rw = |diffuse - diffuse_diff|^2 / sigma_color               (:368-369)
 *       cw = |clip_feat - clip_feat_diff| / sigma_clip with a clip head and sigma_clip > 0, else 0 -- the norm, NOT its square (:370-373)
 *       smooth_weight = exp(-xw - rw - cw)                                                                                    (:375, detached)
 *       smooth_norm   = smooth_weight (sum_b (omega_diff_b - omega_b)^2 + sum_c (clip_feat_diff_c - clip_feat_c)^2)           (:376-378)
 *     the clip sum is added whenever a clip head is given, whether or not sigma_clip > 0 (:377).
 *   pnr_palette_smooth_backward: grad_smooth_norm [M], smooth_weight, the omega and clip pairs ->
 *       grad_omega_diff = 2 g w (omega_diff - omega), grad_omega = -grad_omega_diff, and the same pair for the clip feature (grad_clip_feat /
 *       grad_clip_feat_diff may each be NULL: not wanted).  The weight is detached: nothing reaches xyzs, diffuse or diffuse_diff.
 * 1 <= nb <= 16 and clip_dim <= 128, else PNR_ERR_UNSUPPORTED; a missing pointer, or one clip pointer of a pair without the other, is
 * PNR_ERR_INVALID; M = 0 is PNR_OK.  Every check comes before the launch. */
int pnr_palette_smooth_points(const float* xyzs, const float* noise, float bound, uint32_t M, float* xyzs_diff, pnr_stream_t stream);
int pnr_palette_smooth_forward(uint32_t M, uint32_t num_basis, uint32_t clip_dim, const float* xyzs, const float* xyzs_diff, const float* diffuse,
                               const float* diffuse_diff, const float* omega, const float* omega_diff, const float* clip_feat,
                               const float* clip_feat_diff, float bound, float sigma_xyz, float sigma_color, float sigma_clip, float* smooth_weight,
                               float* smooth_norm, pnr_stream_t stream);
int pnr_palette_smooth_backward(uint32_t M, uint32_t num_basis, uint32_t clip_dim, const float* grad_smooth_norm, const float* smooth_weight,
                                const float* omega, const float* omega_diff, const float* clip_feat, const float* clip_feat_diff, float* grad_omega,
                                float* grad_omega_diff, float* grad_clip_feat, float* grad_clip_feat_diff, pnr_stream_t stream);

/* The two heads of PaletteNetwork.color under autograd as one launch each way (replaces, per training step, the two library GEMMs + bias add +
 * softplus + add + row sum + divide of palette/network.py:262-268 and their backward -- about twenty launches):
 *   h [M, in_dim] (basis_net's output, in_dim <= 16), w_offsets_radiance [3nb+1, in_dim], b_offsets_radiance [3nb+1], w_omega [nb, in_dim]
 *   -> offsets_radiance [M, 3nb+1] = h W_or^T + b,   omega [M, nb] = s / sum(s), s = softplus(h W_om^T) + 0.05      (fp32 fma chains)
 * backward: grad_offsets_radiance [M, 3nb+1], grad_omega [M, nb] -> grad_h [M, in_dim] (NULL: not wanted) and
 *   grad_pre [M, 3nb+1+nb] = [grad_offsets_radiance | dL/d(h W_om^T)], from which pnr_linear_wgrad(h, grad_pre) gives the stacked weight
 *   gradient [3nb+1+nb, in_dim] and pnr_linear_bgrad(grad_pre)[:3nb+1] the bias gradient.  nb <= PNR_MAX_BASIS. */
int pnr_palette_heads_forward(const float* h, const float* w_offsets_radiance, const float* b_offsets_radiance, const float* w_omega, uint32_t M,
                              uint32_t num_basis, uint32_t in_dim, float* offsets_radiance, float* omega, pnr_stream_t stream);
int pnr_palette_heads_backward(const float* h, const float* w_offsets_radiance, const float* w_omega, const float* grad_offsets_radiance,
                               const float* grad_omega, uint32_t M, uint32_t num_basis, uint32_t in_dim, float* grad_h, float* grad_pre,
                               pnr_stream_t stream);

/* The ray-level tail of a training step as ONE launch each way: the renderer's epilogue (palette/renderer.py:387-403 -- background blend of
 * image and direct_rgb, depth normalisation; nerf/renderer.py:331-336) and the trainer's loss on it (palette/utils.py:483-600 with the
 * MSELoss(reduction='none') criterion of main_palette.py:181,222; nerf/utils.py:534-556 when all_map is NULL).  In torch these are ~45
 * launches of 4096-element tensors per step, forward and backward.
 *   image      = image_raw + (1 - weights_sum) bg              depth = clamp(depth_raw - nears, 0) / (fars - nears)
 *   direct_rgb = all_map[:, 7:10] + (1 - weights_sum) bg
 *   loss = mean_n mean_c (image - gt_rgb)^2                                                                  terms[1]
 *        + lambda_sparsity mean all_map[:, 0] + lambda_offsets mean all_map[:, 2] + lambda_view_dep mean all_map[:, 1]   terms[2..4]
 *        + lambda_smooth mean all_map[:, 3]                                                                  terms[5]
 *        + lambda_palette mean_b sum_c (basis_color - basis_color_origin)^2     (both NULL: 0)               terms[6]
 *        + lambda_weight mean (gt_weights - all_map[:, 13+clip_dim:])^2         (gt_weights NULL: 0)         terms[7]
 *        + mean (direct_rgb - gt_rgb)^2                                                                      terms[8]
 *        + mean (all_map[:, 13:13+clip_dim] - gt_clip)^2                        (gt_clip NULL: 0)            terms[9]
 *   terms[0] = loss;  loss_ray [N] = mean_c (image - gt_rgb)^2 (what the reference's error map reads before the scalar terms are added)
 * all_map columns are those of pnr_palette_train_shade_forward's all_buffer after the flex composite; n_channel = 13 + clip_dim + num_basis,
 * or 0 with all_map NULL (the NeRF model: only the first term).  bg_mode 0: the constant bg_const; 1: bg_color [3]; 2: bg_color [N,3]
 * (pnr_train_loss_forward / _backward send no gradient to the background; a per-ray background that trains gets its own from
 * pnr_train_loss_backward_bg).  The sums are reduced in a fixed order (workgroup partials in `workspace`, combined by the last
 * workgroup to finish), so the value is reproducible.  The backward multiplies by the device scalar *grad_loss and writes EVERY element of
 * grad_weights_sum [N], grad_image_raw [N,3], grad_all_map [N,n_channel] and (if not NULL) grad_basis_color [num_basis,3].
 * image / depth / direct_rgb / loss_ray may be NULL (not wanted); depth needs depth_raw, nears and fars. */
typedef struct pnr_train_loss_args {
    uint32_t N, n_channel, num_basis, clip_dim;
    const float* weights_sum;
    const float* depth_raw;
    const float* image_raw;
    const float* all_map;
    const float* nears;
    const float* fars;
    const float* bg_color;
    float bg_const;
    int32_t bg_mode;
    const float* gt_rgb;
    const float* gt_clip;
    const float* gt_weights;
    const float* basis_color;
    const float* basis_color_origin;
    float lambda_sparsity, lambda_offsets, lambda_view_dep, lambda_smooth, lambda_weight, lambda_palette;
    /* forward outputs */
    float* image;
    float* depth;
    float* direct_rgb;
    float* loss_ray;
    float* terms;            /* [PNR_TRAIN_LOSS_TERMS] */
    /* backward */
    const float* grad_loss;  /* device scalar */
    float* grad_weights_sum;
    float* grad_image_raw;
    float* grad_all_map;
    float* grad_basis_color;
    void* workspace;         /* forward only; pnr_train_loss_workspace_bytes(N), zero-filled once by the caller before its first use */
    uint64_t workspace_bytes;
} pnr_train_loss_args;
#define PNR_TRAIN_LOSS_TERMS 10
uint64_t pnr_train_loss_workspace_bytes(uint32_t N);
int pnr_train_loss_forward(const pnr_train_loss_args* args, pnr_stream_t stream);
int pnr_train_loss_backward(const pnr_train_loss_args* args, pnr_stream_t stream);
/* The gradient of a per-ray background (bg_mode == 2: the background model of bg_radius > 0), one launch, every element written:
 *   grad_bg_color[n,k] = (1 - weights_sum[n]) (d loss / d image[n,k] + d loss / d direct_rgb[n,k]) *grad_loss      (the second term with all_map only)
 * Reads the forward's inputs and grad_loss from `args` (the grad_* outputs and the workspace are not touched).  Any other bg_mode is
 * PNR_ERR_UNSUPPORTED; a missing grad_loss or grad_bg_color is PNR_ERR_INVALID; N = 0 is PNR_OK. */
int pnr_train_loss_backward_bg(const pnr_train_loss_args* args, float* grad_bg_color /* [N,3] */, pnr_stream_t stream);

/* replace rgb_to_hsv / hsv_to_rgb, palette/src/palette_func.h, palette.cu:135-149 */
int pnr_rgb_to_hsv(uint32_t n, const float* input, float* output, pnr_stream_t stream);
int pnr_hsv_to_rgb(uint32_t n, const float* input, float* output, pnr_stream_t stream);
/* device counterpart of compute_RGB_histogram (CPU C++ in the reference, palette/src/bindings.cpp:40-91):
 * colors_rgb [n,3], weights [n] -> bin_weights double[2^(3 bpc)] (zeroed by the callee), bin_centers float[2^(3 bpc), 3] */
int pnr_rgb_histogram(const float* colors_rgb, const float* weights, uint32_t n, int bits_per_channel, double* bin_weights,
                      float* bin_centers, pnr_stream_t stream);

/* ---------------------------------------------------------------- background model (ABI 10) - */

/* The background of an unbounded capture (bg_radius > 0: nerf/network.py:145-160, palette/network.py:205-220, fed by sph_from_ray in
 * nerf/renderer.py:270-273) for all N rays of a frame in ONE launch, one ray per lane:
 *   (u, v)  = pnr_sph_from_ray's coordinates of the ray (same arithmetic, same bits; with coords_in: read instead of computed)
 *   enc     = encoder_bg((u, v)): the D = 2, C = 2 lookup of pnr_grid_encode_forward on ((u, v) + 1) / 2 -- fp32 table: fmaf chains; fp16 table:
 *             the half accumulator of the reference's autocast lookup, upcast once
 *   rgb     = sigmoid(W1 . relu(W0 . [SH_4(d) ; enc]))       fp32 fmaf chains in input order, weights staged in LDS
 * Supported: num_levels = 4, level_dim = 2, sh_degree = 4, num_layers = 2, hidden_dim = 64 (the reference's only background architecture);
 * anything else is PNR_ERR_UNSUPPORTED, before anything is launched.  A null struct or a missing pointer is PNR_ERR_INVALID; N = 0 is PNR_OK.
 *   pnr_background_pack: bg_net.0.weight [64, 24] and bg_net.1.weight [3, 64] (row-major [out][in], device fp32) -> `packed`
 *                        (pnr_background_packed_bytes() bytes, 16-byte aligned); call again when either weight changes.
 * Alignment: coords_in / coords_out start on an 8-byte boundary (float2 accesses), the table on 8 bytes (fp32) or 4 (fp16), `packed` on 16; PNR_ERR_ALIGNMENT
 * otherwise, before anything is launched. */
typedef struct pnr_background_args {
    uint32_t N;
    const float* rays_o;           /* [N,3]; not read with coords_in */
    const float* rays_d;           /* [N,3] unit directions */
    float radius;                  /* bg_radius; not used with coords_in */
    const float* coords_in;        /* optional [N,2]: sphere coordinates already at hand (NeRFNetwork.background(x, d)); NULL: computed from the rays */
    const void* embeddings;        /* encoder_bg table [table_rows, 2], fp32 or fp16 (table_dtype) */
    int table_dtype;               /* PNR_DTYPE_F32 / PNR_DTYPE_F16 */
    const int32_t* offsets;        /* device int32[num_levels + 1], read by the kernel; a level that does not fit table_rows gives zeros */
    uint32_t table_rows;
    uint32_t num_levels, level_dim;
    float S;                       /* log2(per_level_scale) */
    uint32_t H;                    /* base_resolution */
    uint32_t gridtype;             /* 0 hash, 1 tiled */
    int align_corners;
    uint32_t sh_degree, num_layers, hidden_dim;
    const float* packed;           /* pnr_background_pack output */
    float* out;                    /* [N,3] fp32 */
    float* coords_out;             /* optional [N,2]: the sphere coordinates the lookup used */
} pnr_background_args;
uint64_t pnr_background_packed_bytes(void);
int pnr_background_pack(const float* w0, const float* w1, float* packed, pnr_stream_t stream);
int pnr_background_forward(const pnr_background_args* args, pnr_stream_t stream);

/* Training the background model (additive entries: the ABI version and pnr_background_args are unchanged).
 *   pnr_background_train_forward: pnr_background_forward's arithmetic in the same order (the same bits) from the RAW weights -- w0 = bg_net.0.weight
 *     [64, 24], w1 = bg_net.1.weight [3, 64], staged into LDS by the kernel, so no pack launch follows an optimiser step -- on the fp32 table.
 *     Writes out [N,3] and ALWAYS coords_out [N,2] (the backward reads them as coords_in).
 *   pnr_background_backward: from grad_rgb [N,3], the saved coordinates (coords_in, required), rays_d, the table and the raw weights: one ray per
 *     lane, the hidden layer recomputed, the gradient taken through sigmoid and ReLU (a NaN stays a NaN).
 *       grad_w0 [64, 24], grad_w1 [3, 64]: every workgroup leaves its rays' sums as one fp32 slab of `workspace`
 *         (pnr_background_backward_workspace_bytes(N) bytes, 16-byte aligned, no initialisation needed) and a second small launch adds the slabs in a
 *         fixed order and writes EVERY element: bitwise reproducible.
 *       grad_table [table_rows, 2] fp32, ZEROED BY THE CALLER (NULL: not wanted): 4 levels x 4 corners x 2 features per ray by float atomics, the cells
 *         of the forward; a ray whose coordinates fall outside [-1, 1] and a level that would reach beyond table_rows add nothing.
 *     No gradient goes to the coordinates or the directions (the reference's rays carry none).
 * Supported: the architecture of pnr_background_forward with an fp32 table (PNR_DTYPE_F32); anything else is PNR_ERR_UNSUPPORTED before anything is
 * launched.  A null struct or a missing pointer is PNR_ERR_INVALID, a misaligned coordinate array, table or workspace PNR_ERR_ALIGNMENT, N = 0 PNR_OK. */
typedef struct pnr_background_train_args {
    uint32_t N;
    const float* rays_o;           /* [N,3]; forward without coords_in only */
    const float* rays_d;           /* [N,3] unit directions */
    float radius;                  /* bg_radius; forward without coords_in only */
    const float* coords_in;        /* forward: optional [N,2] (as pnr_background_args); backward: the forward's coords_out */
    const void* embeddings;        /* encoder_bg table [table_rows, 2] fp32 */
    int table_dtype;               /* PNR_DTYPE_F32 */
    const int32_t* offsets;        /* device int32[num_levels + 1] */
    uint32_t table_rows;
    uint32_t num_levels, level_dim;
    float S;                       /* log2(per_level_scale) */
    uint32_t H;                    /* base_resolution */
    uint32_t gridtype;             /* 0 hash, 1 tiled */
    int align_corners;
    uint32_t sh_degree, num_layers, hidden_dim;
    const float* w0;               /* bg_net.0.weight [64, 24], row-major [out][in], device fp32 */
    const float* w1;               /* bg_net.1.weight [3, 64] */
    /* forward */
    float* out;                    /* [N,3] fp32 */
    float* coords_out;             /* [N,2] */
    /* backward */
    const float* grad_rgb;         /* [N,3] */
    float* grad_w0;                /* [64, 24] */
    float* grad_w1;                /* [3, 64] */
    float* grad_table;             /* [table_rows, 2], zeroed by the caller; optional */
    void* workspace;
    uint64_t workspace_bytes;
} pnr_background_train_args;
int pnr_background_train_forward(const pnr_background_train_args* args, pnr_stream_t stream);
uint64_t pnr_background_backward_workspace_bytes(uint32_t N);
int pnr_background_backward(const pnr_background_train_args* args, pnr_stream_t stream);

/* ---- launch geometry of the entries that cap their grid (host only; additive, ABI 10) ----
 * These entries launch min(ceil(rows / rows_per_trip), cap) workgroups and let each walk tiles `for (t = blockIdx.x; t < ntiles; t += gridDim.x)`.
 * pnr_launch_geometry reports, from the function the launcher itself forms its grid with, the workgroups the named entry launches for `rows`
 * rows and the rows one workgroup handles per trip of its tile loop.  A workgroup takes a second trip iff rows > workgroups * rows_per_trip.
 * Names: pnr_palette_heads_forward / _backward, pnr_palette_smooth_forward / _backward, pnr_palette_smooth_points,
 * pnr_palette_train_shade_forward / _backward, pnr_nerf_field_forward, pnr_nerf_density_forward, pnr_mlp_forward, pnr_mlp_backward (the _lm
 * forms launch as their plain twins).  `rows` is the entry's M or B, except for pnr_palette_smooth_points: there it counts what one lane handles
 * per trip -- float4 groups, floor(3 M / 4), when xyzs, noise and xyzs_diff all start on a 16-byte boundary, else single elements, 3 M.
 * pnr_lattice_density (below) answers too: `rows` = the lattice points of one chunk, min(chunk, nx ny nz).
 * PNR_ERR_INVALID for a name that has no capped grid, a null pointer, or more rows than the entry's own 32-bit count can express. */
int pnr_launch_geometry(const char* entry, uint64_t rows, uint32_t* workgroups, uint32_t* rows_per_trip);

/* ---- mesh export: density lattice and marching cubes on the device (additive, ABI 10) ----
 * What the reference's Trainer.save_mesh does on the host (nerf/utils.py:187-217, :633-653: extract_fields builds 128^3 blocks of points with
 * linspace / meshgrid / cat and reads every block back, PyMCubes runs on the CPU over the volume) as device work: the lattice points, the
 * density volume and the surface never leave the GPU; the host reads back two counts.
 *
 * Lattice (nerf/utils.py:187-217: torch.linspace per axis): coordinate i of n >= 2 on [min, max], step = (max - min) / (n - 1) in fp32,
 *     i < n / 2:  min + step * i        otherwise:  max - step * (n - 1 - i)        (a product and a sum, each rounded: no contraction)
 * -- the two-sided form torch.linspace documents; the last point is exactly max, so a lattice over the field's whole box never steps past
 * `bound` (where the encoder would read zero).  Points are numbered in C order, z fastest: index = (x * ny + y) * nz + z.
 *
 * pnr_lattice_points   points first .. first + count of the lattice as [count, 3] fp32 (for a field evaluated by the caller).
 *                      n[d] in 2 .. 512, first + count <= nx ny nz, null pointer: PNR_ERR_INVALID.  count = 0 is PNR_OK.
 *                      The caller evaluates its field there (density()['sigma'], nerf/utils.py:642-648) and hands the volume to pnr_mesh_count.
 * pnr_lattice_density  nerf/utils.py:187-217 with the query of :642-648 for the shipped field (16-level x 2 fp32 hash grid -> sigma_net 32 -> 64 -> 16,
 *                      the field of pnr_occupancy_update): u[x, y, z] = exp(sigma_net(encoder(p))[0]) at every lattice point -- density()['sigma'], no
 *                      density scale -- by the occupancy sweep's lookup kernel and its exact-fp32 matrix-core sigma_net, `chunk` points at a time
 *                      through workspace = pnr_lattice_density_workspace_bytes(chunk) bytes (256-byte aligned; chunk >= 256, rounded up to a multiple
 *                      of 256, at most 2^22 are used).  Another architecture is PNR_ERR_UNSUPPORTED; a null pointer, an n[d] outside 2 .. 512 or a
 *                      workspace below 256 points PNR_ERR_INVALID -- before any launch. */
int pnr_lattice_points(const float* box_min, const float* box_max, const uint32_t* n, uint64_t first, uint32_t count, float* points, pnr_stream_t stream);
typedef struct pnr_lattice_density_args {
    float box_min[3], box_max[3];
    uint32_t n[3];
    float bound;                       /* of the encoder: its inputs are (p + bound) / (2 bound) */
    const float* embeddings;           /* fp32 hash table [rows, 2] */
    const int32_t* offsets;
    uint32_t num_levels;
    float S;
    uint32_t base_resolution, gridtype;
    const float* packed_sigma_net;     /* a PNR_FIELD_FP32 blob of pnr_nerf_field_pack (its sigma_net part) */
    void* workspace;
    uint64_t workspace_bytes;
    float* u;                          /* [nx, ny, nz] out */
} pnr_lattice_density_args;
uint64_t pnr_lattice_density_workspace_bytes(uint32_t chunk);
int pnr_lattice_density(const pnr_lattice_density_args* args, pnr_stream_t stream);

/* Marching cubes over a device volume u[nx, ny, nz] (replaces mcubes.marching_cubes, nerf/utils.py:211).  A lattice point is inside when
 * u > threshold (strict; NaN is outside).  Case table: csrc/mc_tables.inc, generated by csrc/gen_mc_tables.py -- corner c = x + 2y + 4z,
 * cube edge e = axis * 4 + (offsets of the other two axes, lower axis in bit 0), ambiguous faces cut off each inside corner on its own (the
 * same way from both cells of a face: watertight for any field), triangles counter-clockwise seen from the low-density side.
 *   vertices  one per lattice edge (p, axis) whose ends differ, shared by the cells around it, ascending by ((x ny + y) nz + z) * 3 + axis;
 *             [nv, 3] fp32 in lattice-index coordinates: p, with p[axis] + t,  t = (threshold - u0) / (u1 - u0), 0.5 when that is not finite,
 *             clamped to [0, 1]  (u0 = u[p], u1 = u[p + axis]).
 *   triangles by cell in C order, then in table order; [nt, 3] int32 vertex indices.
 * The order is part of the contract: the output is reproducible bit for bit.
 *   pnr_mesh_case_triangles  host only: the triangles of a case (0 .. 5) and, when edges is not NULL, their 3 * n cube edges (255-padded);
 *                            PNR_ERR_INVALID for case > 255.
 *   pnr_mesh_count           classifies every lattice edge and cell, scans, leaves counts[0] = nv, counts[1] = nt (device int32[2]) and the
 *                            per-point vertex ranks in the workspace (pnr_mesh_workspace_bytes(nx, ny, nz) bytes, 256-byte aligned).
 *   pnr_mesh_emit            after pnr_mesh_count on the same u, threshold and workspace: writes the vertices and triangles; rows at or past
 *                            cap_vertices / cap_triangles are not written (the caller sized the arrays from the counts).
 * PNR_ERR_INVALID before any launch: a null pointer, an axis < 2 or > 512 (3 * 512^3 fits the 29-bit ranks), a short or misaligned workspace. */
int pnr_mesh_case_triangles(uint32_t mc_case, uint8_t* edges /* [15] or NULL */);
uint64_t pnr_mesh_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int pnr_mesh_count(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* workspace, uint64_t workspace_bytes, int32_t* counts,
                   pnr_stream_t stream);
int pnr_mesh_emit(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, const void* workspace, uint64_t workspace_bytes,
                  float* vertices, uint32_t cap_vertices, int32_t* triangles, uint32_t cap_triangles, pnr_stream_t stream);

/* ---- evaluate and test loops: palette sheets and meters on the device (additive, ABI 10; csrc/evaluate.hip) ----
 * pnr_palette_sheets replaces the host half of PaletteTrainer.test, palette/utils.py:993-1038, and of the save_images block of
 * evaluate_one_epoch, palette/utils.py:852-909 (nerf/utils.py:716-731 for a NeRF model: rgb and depth only): every `.cpu().numpy()` of an fp32
 * map followed by `(x.clip(0, 1) * 255).astype(np.uint8)` and the np.concatenate(axis=1) of the per-basis images -- ONE launch, the frame leaves
 * the device as bytes.  Inputs are fp32 maps of H*W rays, each with its own row stride in floats (>= its column count): columns of the frame
 * call's aux_map are passed as they are.  A NULL input: that sheet is not written.  An output is written only when it is not NULL; an output
 * given without its input is PNR_ERR_INVALID.  `image` and `depth` are required.
 *   out_rgb [H,W,3]                   (uint8)(int)(clamp(s(image), 0, 1) * 255.0f), s = linear_to_srgb (nerf/utils.py:43-44, pnr_image_to_uint8's
 *                                     expression) when asked, the identity otherwise                                    (palette/utils.py:993-999)
 *   out_depth [H,W]                   (uint8)(int)(depth * 255.0f), no clamp                      (:1001-1002, as pnr_image_to_uint8 does)
 *   out_view_dep, out_direct [H,W,3]  (uint8)(int)(clamp(v, 0, 1) * 255.0f)                                         (:1006-1008, :861-866)
 *   out_basis_img, out_unscaled_basis_img [H, nb W, 3]   pixel (y, i W + x) = basis i of ray y W + x, columns 3i .. 3i + 2   (:1015-1024, :885-898)
 *   out_basis_acc [H, nb W]           pixel (y, i W + x) = basis_acc[y W + x, i]                                        (:1017-1025)
 *   out_weights_guide [H, nb W]       the same from gt_weights: gt_weights.transpose(0, 2, 1).reshape(H, -1)                 (:852-855)
 *   out_basis_color [100, 100 nb, 3]  the palette swatches, basis_color [nb,3] clamped to [0, 1]                        (:1019-1026)
 * Bytes are stored four at a time where the output's address allows, singly at ragged heads and tails (any base pointer works).
 * H * W == 0 is PNR_OK; num_basis outside 1 .. PNR_SHEET_MAX_BASIS with a per-basis input, a stride below the column count or a NULL required
 * pointer is PNR_ERR_INVALID; 3 nb H W >= 2^32 is PNR_ERR_UNSUPPORTED. */
#define PNR_SHEET_MAX_BASIS 8
typedef struct pnr_sheet_args {
    uint32_t H, W, num_basis;
    int linear_to_srgb;                 /* out_rgb only */
    const float* image;                 /* [H W, 3] */
    const float* depth;                 /* [H W] */
    const float* view_dep_rgb;          /* [H W, 3]    optional */
    const float* direct_rgb;            /* [H W, 3]    optional */
    const float* basis_rgb;             /* [H W, 3 nb] optional */
    const float* unscaled_basis_rgb;    /* [H W, 3 nb] optional */
    const float* basis_acc;             /* [H W, nb]   optional */
    const float* gt_weights;            /* [H W, nb]   optional */
    const float* basis_color;           /* [nb, 3] contiguous, optional */
    uint32_t image_stride, depth_stride, view_dep_stride, direct_stride, basis_rgb_stride, unscaled_stride, basis_acc_stride, gt_weights_stride;   /* floats per row */
    uint8_t* out_rgb;
    uint8_t* out_depth;
    uint8_t* out_view_dep;
    uint8_t* out_direct;
    uint8_t* out_basis_img;
    uint8_t* out_unscaled_basis_img;
    uint8_t* out_basis_acc;
    uint8_t* out_weights_guide;
    uint8_t* out_basis_color;
} pnr_sheet_args;
int pnr_palette_sheets(const pnr_sheet_args* args, pnr_stream_t stream);

/* pnr_frame_metrics replaces eval_step's ground truth and loss (palette/utils.py:610-638) and the meters' update() of evaluate_one_epoch
 * (:825-830): PSNRMeter (nerf/utils.py:220-252), SSIMMeter (:297-330, kornia's ssim_loss(window_size=11)), SparsityMeter and TVMeter
 * (palette/utils.py:52-114) of ONE H x W view in ONE launch, added to running totals on the device; nothing is read back per frame.
 *   truth [H W, C], C = 3 or 4, fp32 in [0, 1]; with srgb_to_linear_truth its colour channels first go through nerf/utils.py:48-49 (:617-618);
 *   gt = rgb a + 1 (1 - a) for C = 4 (:621-625), rgb otherwise; truth_rgb_out (optional, [H W, 3] contiguous) receives it as fp32.
 *   mse       mean((pred - gt)^2) over the 3 H W values (the criterion of :636)           psnr  -10 log10(mse)  (nerf/utils.py:242)
 *   sparsity  mean over pixels of sum_i w_i / (sum_i w_i^2 + 1e-6) - 1   (:69)
 *   tv        100 (mean((w[:, :-1] - w[:, 1:])^2) + mean((w[:-1] - w[1:])^2)) over [H, W, nb]   (:101-104)
 *   ssim      1 - 2 mean(clamp((1 - S) / 2, 0, 1)),  S = ((2 m1 m2 + C1)(2 s12 + C2)) / ((m1^2 + m2^2 + C1)(s1 + s2 + C2) + 1e-12) per channel
 *             and pixel, m / E[.] from the 11 x 11 normalised Gaussian (sigma 1.5), border reflected without repeating the edge sample (pad 5,
 *             "same" size), s1 = E[p^2] - m1^2, s2 = E[t^2] - m2^2, s12 = E[p t] - m1 m2, C1 = 0.01^2, C2 = 0.03^2  (nerf/utils.py:317-318).
 *             This is kornia's ssim_loss(window_size=11) with its documented defaults as read from its documentation: kornia is not installed
 *             where this library is developed, so nobody has run it against this statement; the float64 statement in tests/evaluate_reference.py
 *             is the yardstick.
 * One launch does all five (a second launch for SSIM alone was not needed: the meters other than SSIM ride on the tile load SSIM needs anyway).
 * Arithmetic: fp32 inputs, everything after them -- the ground truth, the separable window sums, S, every sum -- in double, so E[p^2] - m^2
 * keeps its bits on flat regions.  Reductions run in a fixed order (per-workgroup partials in double, the last workgroup, found by a ticket the
 * kernel resets itself, adds them by index): two runs give the same bits; no atomics go into a result.
 *   totals    device double[8], caller-owned, zero it to clear: [0] += 1 (frames), [1] += mse, [2] += psnr, [3] += ssim, [4] += sparsity, [5] += tv
 *   frame_out optional device double[8]: this frame's values alone ([0] = 1)
 *   workspace pnr_frame_metrics_workspace_bytes(H, W) bytes, 8-byte aligned, its first 64 bytes ZERO before the first call (the ticket)
 * Values that `want` leaves out are 0 (PSNR implies MSE).  basis_acc == NULL: no palette meters (their bits are ignored).
 * PNR_ERR_INVALID: a NULL pointer, C not 3 or 4, a stride below the column count, num_basis outside 1 .. PNR_MAX_BASIS with basis_acc,
 * H or W < 6 with SSIM wanted, H or W < 2 with TV wanted, a workspace that is too small.  H * W == 0 is PNR_OK and touches nothing. */
#define PNR_METRIC_MSE 1
#define PNR_METRIC_PSNR 2
#define PNR_METRIC_SSIM 4
#define PNR_METRIC_SPARSITY 8
#define PNR_METRIC_TV 16
typedef struct pnr_metrics_args {
    uint32_t H, W;
    const float* pred;                  /* [H W, 3] rows of pred_stride floats */
    uint32_t pred_stride;
    const float* truth;                 /* [H W, C] contiguous */
    uint32_t truth_channels;            /* 3 or 4 */
    int srgb_to_linear_truth;
    const float* basis_acc;             /* [H W, nb] rows of basis_acc_stride floats, or NULL */
    uint32_t basis_acc_stride, num_basis;
    uint32_t want;                      /* PNR_METRIC_* bits */
    float* truth_rgb_out;               /* optional [H W, 3] */
    double* totals;                     /* [8] in/out */
    double* frame_out;                  /* optional [8] out */
    void* workspace;
    uint64_t workspace_bytes;
} pnr_metrics_args;
uint64_t pnr_frame_metrics_workspace_bytes(uint32_t H, uint32_t W);
int pnr_frame_metrics(const pnr_metrics_args* args, pnr_stream_t stream);

/* ---- training batches: gather, blend, weight guide, error map on the device (additive, ABI 10; csrc/train_batch.hip) ----
 * pnr_train_batch replaces what a training step does in front of model.render: NeRFDataset.collate (palette/provider.py:356-410: the pose
 * lookup, get_rays' ray arithmetic, the torch.gather of the pixels and of the feature pixels) and the head of PaletteTrainer.train_step
 * (palette/utils.py:450-478; nerf/utils.py:507-525 likewise: srgb_to_linear, the alpha blend over the background, get_palette_weight_with_hist,
 * palette/utils.py:117-124) -- ONE launch for B views of N rays each, one lane per ray; ray r = b N + n.  The random draws (pixel ids, the
 * per-pixel background) stay torch's and come in as arrays; the view is chosen by an index ON THE DEVICE, nothing is read back to pick it.
 *   images [V,H,W,C], C = 3 or 4, stored as image_format: fp32, fp16 (converted exactly) or uint8 (u / 255.0f, the loader's
 *   astype(float32) / 255 for an 8-bit source); feat_images [V,H,W,D] fp32 or fp16 (the --pred_clip target); poses [V,4,4] fp32 row-major
 *   cam2world with fx, fy, cx, cy as pnr_get_rays takes them; view_index [B], inds [B,N] int64 flat pixel ids; hist_weights [nb,Sr,Sg,Sb]
 *   fp32 (the extraction's LUT without its leading 1: any sizes, r first), element (k, ir, ig, ib) at the dot product with hist_stride -- the
 *   reference holds the table as a permuted view of an [R,G,B,nb] array, which is read where it lies, without a copy per step.
 * Outputs, each optional by a NULL pointer, fp32:
 *   rays_o, rays_d [B N,3]   pnr_get_rays' arithmetic on poses[view_index[b]], the same bits (both or neither)
 *   pixels [B N,C]           the gathered pixel as fp32: collate's `images`
 *   gt_rgb [B N,3]           c = srgb_to_linear ? (x < 0.04045 ? x / 12.92 : ((x + 0.055) / 1.055)^2.4) : x per colour channel (nerf/utils.py:48-49,
 *                            the device library's powf), then for C = 4: c a + bg (1 - a) in fp32 as torch evaluates it -- two products, one
 *                            difference, one sum, nothing fused; bg by bg_mode: 0 = bg_const, 1 = bg_color[3], 2 = bg_color[B N,3] (the
 *                            trainer's rand_like draw).  C = 3: gt_rgb = c, bg is not read.
 *   gt_weights [B N,nb]      sum over the 8 corners of hist[k, ir, ig, ib] w, read at x = gt_rgb (S - 1) per channel: i = floor(x), the corner
 *                            weights (i + 1) - x and x - i, a corner with an index outside [0, S) counts as zero -- grid_sample(bilinear,
 *                            padding_mode='zeros', align_corners=True) behind the reference's [2,1,0] swizzle; summed in grid_sample's corner order
 *   gt_clip [B N,D]          the gathered feature pixel as fp32
 * All addresses are formed in 64 bits (V H W C passes 2^32 on large sets).  A view index outside [0, V) or a pixel id outside [0, H W) is the
 * caller's error; it is clamped into range, so nothing outside the stacks is read.
 * B N == 0 is PNR_OK.  PNR_ERR_INVALID: a NULL required pointer, V, H or W of 0, C not 3 or 4 with a pixel output, rays_o without rays_d, fx or fy of
 * 0 with rays, bg_mode outside 0..2 or without its array (C = 4 with a colour output), a table size of 0 or above 1024, D of 0 with gt_clip;
 * PNR_ERR_UNSUPPORTED: an unknown format, num_basis outside 1 .. PNR_MAX_BASIS with gt_weights, H W >= 2^32. */
#define PNR_IMAGE_FP32 0
#define PNR_IMAGE_FP16 1
#define PNR_IMAGE_UINT8 2
typedef struct pnr_train_batch_args {
    uint32_t V, H, W, C;
    const void* images;                 /* [V,H,W,C] */
    int image_format;                   /* PNR_IMAGE_* */
    const void* feat_images;            /* [V,H,W,D] fp32 or fp16, optional */
    int feat_format;                    /* PNR_IMAGE_FP32 or PNR_IMAGE_FP16 */
    uint32_t D;
    const float* poses;                 /* [V,4,4] */
    float fx, fy, cx, cy;
    const int64_t* view_index;          /* [B] on the device */
    const int64_t* inds;                /* [B,N] */
    uint32_t B, N;
    int bg_mode;                        /* 0: bg_const, 1: bg_color [3], 2: bg_color [B N,3] */
    float bg_const;
    const float* bg_color;
    const float* hist_weights;          /* [num_basis,Sr,Sg,Sb], optional */
    uint32_t num_basis, Sr, Sg, Sb;
    uint64_t hist_stride[4];            /* floats between neighbours along (basis, r, g, b); all 0 = contiguous in that order */
    int srgb_to_linear;
    float* rays_o;                      /* [B N,3] */
    float* rays_d;                      /* [B N,3] */
    float* pixels;                      /* [B N,C] */
    float* gt_rgb;                      /* [B N,3] */
    float* gt_weights;                  /* [B N,num_basis] */
    float* gt_clip;                     /* [B N,D] */
} pnr_train_batch_args;
int pnr_train_batch(const pnr_train_batch_args* args, pnr_stream_t stream);

/* The error map's update at the end of train_step (palette/utils.py:578-599, nerf/utils.py:556-580), in place on a device-resident map
 * [V, cells] (cells = 128 * 128 in the reference) -- ONE launch, no copy of the rows out and back, no host synchronisation:
 *   map[view_index[b], inds_coarse[b, n]] = 0.1f * map[...] + 0.9f * loss_ray[b, n]      (:595-596; two products and a sum, nothing fused)
 * view_index [B], inds_coarse [B,N] int64 on the device, loss_ray [B,N] fp32.  The rows of inds_coarse come from multinomial(replacement=False)
 * and are unique; duplicates within a view (or one view twice in view_index) give an unspecified winner, as torch's scatter_ does.
 * A cell id outside [0, cells) is clamped; the number of views is not an argument, so view_index < V is the caller's to guarantee (a negative one
 * is taken as 0).  B N == 0 is PNR_OK; a NULL pointer or cells of 0 is PNR_ERR_INVALID. */
int pnr_error_map_update(float* error_map, uint32_t cells, const int64_t* view_index, const int64_t* inds_coarse, const float* loss_ray, uint32_t B,
                         uint32_t N, pnr_stream_t stream);

/* ---- Stylizer fit: the GUI's "optimize" step as one launch (additive, ABI 10; csrc/stylizer.hip) ----
 * pnr_stylizer_fit replaces the optimisation loop of palette/gui.py:153-194: `iters` steps of SGD with momentum on the Stylizer's dI [nb],
 * dP [nb,3] and ddelta [nb,3,3] (palette/renderer.py:150-183) against M picked colours -- ONE launch of one wave, the parameters on chip for
 * the whole run, every sum over the points in a fixed order (bit-for-bit reproducible).  All arrays fp32 on the device.  Per iteration:
 *   s_n = softplus(radiance_n)  (log1p(exp(r)), r itself past 20),   I_np = max(s_n + dI_p, 0),   C_npj = palette_pj + dP_pj + sum_i offsets_npi ddelta_pij
 *   rgb_nj = sum_p omega_np clamp(I_np C_npj, 0, 1) (+ view_dep_nj),   e = rgb - target
 *   loss = sum e^2 + lambda_arap (sum_p |D_p D_p^T - 1|_F^2 + sum dP^2)            (D_p = ddelta_p)
 *   the gradient of loss as torch's autograd takes it (clamp: bounds inclusive; max(., 0): zero included)
 *   buf = momentum buf + grad  (the first step of a run without momentum buffers: buf = grad),   x -= lr[t] buf
 *   radiance [M] raw; omega [M,nb]; offsets [M,nb,3]; palette [nb,3], the caller's basis_color.clamp(0,1); target [M,3]; view_dep [M,3] optional,
 *   added to the colour as a constant; lr [iters], the learning rate of every iteration (the scheduler's values, narrowed to fp32 by the caller).
 *   dI, dP, ddelta: in/out.  mom_dI, mom_dP, mom_ddelta: optional (all three or none), written back when given; has_momentum != 0 continues from them.
 *   trace [iters,2], optional: (total loss, regulariser) at the parameters BEFORE that iteration's update, as the reference prints them.
 * PNR_ERR_UNSUPPORTED: num_basis outside 4 .. PNR_MAX_BASIS, M > PNR_STYLIZER_MAX_POINTS, iters > PNR_STYLIZER_MAX_ITERS (a longer run is several
 * launches, continued through the momentum buffers: no single kernel runs for long).  Then M == 0 or iters == 0 is PNR_OK and nothing is touched.
 * PNR_ERR_INVALID: a NULL struct or required pointer, one or two of the three momentum buffers, has_momentum without them.  All before any launch. */
#define PNR_STYLIZER_MAX_POINTS 512
#define PNR_STYLIZER_MAX_ITERS 10000
typedef struct pnr_stylizer_fit_args {
    uint32_t M, num_basis, iters;
    const float* radiance;
    const float* omega;
    const float* offsets;
    const float* palette;
    const float* target;
    const float* view_dep;
    float* dI;
    float* dP;
    float* ddelta;
    float* mom_dI;
    float* mom_dP;
    float* mom_ddelta;
    int has_momentum;
    const float* lr;
    float momentum, lambda_arap;
    float* trace;
} pnr_stylizer_fit_args;
int pnr_stylizer_fit(const pnr_stylizer_fit_args* args, pnr_stream_t stream);

/* ---- coloured mesh export: analytic normals and the vertex block on the device (additive, ABI 10; csrc/normals.hip) ----
 * MI355X-first addition, no counterpart in the reference (its save_mesh writes bare geometry).
 *
 * pnr_density_gradient: for n world-space points of the shipped density field (the field of pnr_lattice_density: 16 levels x 2 features, fp32
 * table, D = 3, hash or tiled, align_corners false; sigma_net 32 -> 64 (ReLU) -> 16, bias-free)
 *   logit [n]     sigma_net(encoder((p + bound) / (2 bound)))[0]: density()['sigma'] = exp(logit)
 *   grad [n,3]    d logit / d p in world coordinates (the 1 / (2 bound) of the encoder's input folded in).  The gradient of the LOGIT: grad sigma =
 *                 sigma grad logit has the same direction, and nothing overflows.
 *   normal [n,3]  -grad / |grad|: out of the dense region, the side pnr_mesh_emit's triangles are counter-clockwise from.
 * Each output is optional by a NULL pointer; at least one must be given.  sigma0 [64,32] and sigma1 [16,64] are the RAW row-major weight
 * matrices (only row 0 of sigma1 is read): an optimiser step or an EMA swap needs no pack launch and invalidates nothing.
 *   Cell path     the cell of a point on each level is grid_core.hpp's: unit_cube_of, grid_cell<3>, corner_rows<3, 1>, and the level's value is
 *                 cell_interp's chain -- the gradient belongs to the trilinear piece the forward value comes from everywhere else in the library.
 *                 Along axis d on level l:  scale_l * sum over the four corner pairs (x-lowest first) of w(other two axes) * (right - left),
 *                 w = the product of the other two axes' factors, lower axis first; an fmaf chain from 0.
 *   sigma_net     hidden pre-activations z_k are plain fp32 fmaf chains over the 32 inputs in order (not the split-fp16 path, not the matrix
 *                 cores); the ReLU derivative is z_k > 0 (strict), as torch's.  logit = the chain over k of w1[0][k] * max(z_k, 0).
 *                 `logit` is therefore NOT promised bit-equal to the matrix-core density path (nerf_density_tile<0>: pnr_lattice_density,
 *                 pnr_nerf_density_forward): the same products, another order of the sums.
 *   Outside       a point outside the box reads zero from the encoder: logit = 0, grad = 0, normal = 0.  |grad| zero or not finite: normal = 0.
 *   Order         one lane per point, every sum in a fixed order, no atomics, no scratch, no workspace: a row's result does not depend on n, on
 *                 its position in the batch or on how the caller chunks the call -- reproducible bit for bit.  The [n, 16 * 3 * 2] Jacobian
 *                 never goes to memory.  ONE launch of ceil(n / 256) workgroups, whatever n is (no capped grid, no tile loop).
 * PNR_ERR_UNSUPPORTED: another architecture (num_levels != 16, gridtype > 1, bound <= 0).  PNR_ERR_INVALID: a NULL struct or required pointer
 * (with n > 0: points), all three outputs NULL.  n = 0 is PNR_OK.  All before any launch. */
typedef struct pnr_density_gradient_args {
    const float* points;               /* [n,3] world space */
    uint32_t n;
    float bound;
    const float* embeddings;           /* fp32 hash table [rows, 2] */
    const int32_t* offsets;
    uint32_t num_levels;
    float S;
    uint32_t base_resolution, gridtype;
    const float* sigma0;               /* [64,32] row-major, raw */
    const float* sigma1;               /* [16,64] row-major, raw; row 0 is read */
    float* logit;                      /* [n]   optional */
    float* grad;                       /* [n,3] optional */
    float* normal;                     /* [n,3] optional */
} pnr_density_gradient_args;
int pnr_density_gradient(const pnr_density_gradient_args* args, pnr_stream_t stream);

/* pnr_mesh_vertex_records: the vertex block of a binary little-endian PLY on the device -- the host reads back final bytes.
 *   vertices [nv,3]   pnr_mesh_emit's lattice-index vertices
 *   world [nv,3]      fp32( (double)v / (n - 1) * (double)(box_max - box_min) + (double)box_min ), box_max - box_min subtracted in fp32 first:
 *                     extract_geometry's float64 vertices rounded once to fp32, the rounding write_ply applies -- a coloured file's x y z equal
 *                     the plain file's bit for bit.  Optional.
 *   records [nv, record_bytes]   x y z (f4) | nx ny nz (f4, with `normal`) | red green blue alpha (u1, alpha 255, with `rgb`) | extra[0 .. extra_channels) (f4)
 *                     record_bytes = 12 + (normal ? 12 : 0) + (rgb ? 4 : 0) + 4 extra_channels.  Optional.
 *   colour bytes      (uint8)(int)(s(clamp(c, 0, 1)) * 255.0f), s = the linear -> sRGB curve of pnr_image_to_uint8 when linear_to_srgb, else the identity.
 * normal [nv,3], rgb [nv,3] contiguous; extra rows of extra_stride floats (>= extra_channels).  One lane per 32-bit word of the output.
 * nv = 0 is PNR_OK.  PNR_ERR_INVALID: a NULL struct or vertex pointer, an n[d] < 2, neither output, extra_channels without `extra` or a stride below the
 * channel count, records not 4-byte aligned; PNR_ERR_UNSUPPORTED: 2^32 or more output words.  All before any launch.
 * pnr_mesh_vertex_record_bytes: host only, the record_bytes above. */
typedef struct pnr_vertex_records_args {
    const float* vertices;             /* [nv,3] */
    uint32_t nv;
    float box_min[3], box_max[3];
    uint32_t n[3];
    const float* normal;               /* [nv,3] optional */
    const float* rgb;                  /* [nv,3] optional */
    int linear_to_srgb;
    const float* extra;                /* [nv, extra_channels] optional */
    uint32_t extra_channels, extra_stride;
    float* world;                      /* [nv,3] out, optional */
    uint8_t* records;                  /* [nv, record_bytes] out, optional; 4-byte aligned */
} pnr_vertex_records_args;
uint32_t pnr_mesh_vertex_record_bytes(int has_normal, int has_rgb, uint32_t extra_channels);
int pnr_mesh_vertex_records(const pnr_vertex_records_args* args, pnr_stream_t stream);

/* ---- palette extraction, front end: histograms and k-means on the device (additive, ABI 10; csrc/extract.hip) ----
 * PaletteTrainer.extract_palette (palette/utils.py:1135-1200) into palette_extraction as far as run_kmeans' return (:167-226).  The hull
 * simplification stays with the reference's CPU package; `centers` / `center_weights` below are exactly its input.  The weight LUT of the
 * palette it returns is pnr_lut_weights, further down.  (The hull simplification on the device has a header of its own: include/pnr_hull.h.)
 *
 * pnr_extract_accumulate: ONE launch folds one rendered view of H x W pixels into both colour histograms.  Per pixel i (row-major):
 *   valid = weights_sum[i] > thresh            strict; a NaN is not valid (:1185)
 *   p     = the first three channels of the ground-truth pixel (alpha is not read), srgb_to_linear'ed first when `linear` (:1169-1170;
 *           pnr_train_batch's curve and pixel conversion: fp32 as stored, fp16 exactly, uint8 as u / 255)
 *   c     = p + 0.05f;  c = c / sqrtf((c0 c0 + c1 c1) + c2 c2)                                   (:1172-1173)
 *   bin   = the reference's RGB_to_bin_index at 3 and at 5 bits per channel from the same c (palette/src/bindings.cpp:40-50):
 *           per channel uint32(fmaxf(0, fminf(0.999f, c)) * 2^bpc), r most significant
 * counts_coarse [512], counts_fine [32 768] and total [1] are 64-bit integer counts and are ACCUMULATED into: the caller zeroes them once.
 * The extraction's sample weights are all 1 (:190), so the counts are exact, independent of arrival order and of the launch shape:
 * bit-reproducible (integer atomics only).  Launch shape: min(256, ceil(H W / 1024)) workgroups of 1024 lanes striding over the view, both
 * tables private in LDS, one 64-bit atomic per non-zero bin and workgroup at the end (pnr_launch_geometry("pnr_extract_accumulate", H W)).
 * pixels: the view's first pixel; row_stride_bytes between rows (0 = W * channels * element size).
 * Order of the checks, all before any launch: NULL args -> PNR_ERR_INVALID; an unknown image_format or channels other than 3 or 4 ->
 * PNR_ERR_UNSUPPORTED; H W == 0 -> PNR_OK, nothing touched; a NULL pointer, a row stride below the row or not a multiple of the element size,
 * a base not aligned to the element -> PNR_ERR_INVALID. */
#define PNR_EXTRACT_COARSE_BINS 512
#define PNR_EXTRACT_FINE_BINS 32768
typedef struct pnr_extract_accumulate_args {
    uint32_t H, W;
    const float* weights_sum;           /* [H W]: the frame call's output, read where it lies */
    const void* pixels;                 /* [H, W, channels] with a row stride */
    int image_format;                   /* PNR_IMAGE_* */
    uint32_t channels;                  /* 3 or 4 */
    uint64_t row_stride_bytes;
    int linear;
    float thresh;                       /* the reference's 0.5 */
    uint64_t* counts_coarse;            /* [512]    in/out */
    uint64_t* counts_fine;              /* [32768]  in/out */
    uint64_t* total;                    /* [1]      in/out: valid samples */
} pnr_extract_accumulate_args;
int pnr_extract_accumulate(const pnr_extract_accumulate_args* args, pnr_stream_t stream);

/* pnr_extract_kmeans: the rest of palette_extraction up to run_kmeans' return, ONE launch of one workgroup.
 *   points    the P non-empty fine bins in ascending code order, (code_channel + 0.5) / 32; weight count / total       (:217-222)
 *   init      the centres (code_channel + 0.5) / 8 of the K coarse bins with count / total > tau, ascending             (:209-215)
 *   Lloyd     scikit-learn's _kmeans_single_lloyd for KMeans(n_clusters=K, init=array): labels = argmin over the CURRENT centres of
 *             ((x0-c0)^2 + (x1-c1)^2) + (x2-c2)^2, a tie to the lowest index; new centres = weighted sums times 1 / weight; stop when the
 *             labels equal the previous iteration's (PNR_EXTRACT_STOP_LABELS), else when the summed squared centre shift is
 *             <= tol * mean(var(points, axis=0)) (unweighted; PNR_EXTRACT_STOP_SHIFT), else after max_iter iterations (PNR_EXTRACT_STOP_CAP);
 *             unless the labels stopped it, one more labelling with the final centres.  center_weights[k] = the weight labelled k.
 *   out       centers [K,3] and center_weights [K] by descending weight, ties to the lower cluster index (:159-165); both buffers hold
 *             PNR_EXTRACT_MAX_K rows.  labels [P] (optional, a debug output): the final label of every point, BEFORE the sort.
 *   info [8]  K, P, iterations run, the stop rule, the status, 0, 0, 0.
 * float64 throughout, no atomics, every sum in a fixed order (csrc/extract.hip): two runs give the same bits.  scikit-learn's float32
 * rounding (it works in the dtype of bin_centers_fine) and its centring of the points are not imitated.
 * K and P are known on the device only, so what depends on them is answered in info[4], not in the return value:
 *   PNR_EXTRACT_NO_CENTER (K = 0), PNR_EXTRACT_TOO_MANY (K > PNR_EXTRACT_MAX_K), PNR_EXTRACT_FEW_POINTS (P < K): nothing else is written.
 *   PNR_EXTRACT_EMPTIED: a cluster lost all its points in iteration info[2] (0-based).  scikit-learn's relocation is NOT done here: centers
 *   holds the centres that iteration started from, in cluster order, center_weights zeros, and the caller finishes on the host.
 * PNR_ERR_INVALID before any launch: a NULL struct or pointer (labels excepted), a workspace below pnr_extract_kmeans_workspace_bytes() or
 * not 8-byte aligned, max_iter == 0, tau or tol negative or NaN. */
#define PNR_EXTRACT_MAX_K 128
#define PNR_EXTRACT_STOP_CAP 0
#define PNR_EXTRACT_STOP_LABELS 1
#define PNR_EXTRACT_STOP_SHIFT 2
#define PNR_EXTRACT_OK 0
#define PNR_EXTRACT_EMPTIED 1
#define PNR_EXTRACT_NO_CENTER 2
#define PNR_EXTRACT_TOO_MANY 3
#define PNR_EXTRACT_FEW_POINTS 4
typedef struct pnr_extract_kmeans_args {
    const uint64_t* counts_coarse;      /* [512] */
    const uint64_t* counts_fine;        /* [32768] */
    const uint64_t* total;              /* [1] */
    double tau;                         /* the reference's 8e-3 */
    double tol;                         /* scikit-learn's 1e-4 */
    uint32_t max_iter;                  /* scikit-learn's 300 */
    void* workspace;
    uint64_t workspace_bytes;
    double* centers;                    /* [PNR_EXTRACT_MAX_K,3] out */
    double* center_weights;             /* [PNR_EXTRACT_MAX_K]   out */
    int32_t* info;                      /* [8] out */
    int32_t* labels;                    /* [32768] out, optional */
} pnr_extract_kmeans_args;
uint64_t pnr_extract_kmeans_workspace_bytes(void);
int pnr_extract_kmeans(const pnr_extract_kmeans_args* args, pnr_stream_t stream);

/* ---- palette extraction, weight LUT: hull projection and barycentrics on the device (additive, ABI 10; csrc/lut.hip) ----
 * What palette_extraction does after the hull simplification (palette/utils.py:235-245): the Tan-2016/2018 "ASAP" weights of the 32 768
 * five-bit colour bins against the palette -- Get_ASAP_weights_using_Tan_2016_triangulation_and_then_barycentric_coordinates
 * (rgbsg/fastLayerDecomposition/Additive_mixing_layers_extraction.py:397-547) -- the `hist_weights` table that initialize_palette, every
 * training batch's weights_guide and the guide sheet read.  The hull simplification itself (the palette) stays with the reference's CPU package.
 *
 * pnr_lut_weights: the weights of N colours against a palette of M colours, PNR_LUT_MIN_M <= M <= PNR_LUT_MAX_M, ONE launch, float64:
 *   order     the palette rows by L1 distance to black (|r| + |g|) + |b|, a tie to the lower row (:404-406): V[0] is the darkest row
 *   hull      the faces are the triples i < j < k of V whose plane has every other row on one side by more than 1e-9, in ascending
 *             (i, j, k), each with its unit normal pointing outwards; a row inside the hull belongs to no face and gets weight 0
 *   project   a point is outside iff its signed distance to some face plane exceeds 1e-8 (the reference's find_simplex(tol=1e-8)); it is
 *             replaced by the closest point of the hull surface: the nearest over the faces of the closest point on the triangle
 *             (:426-437), a tie to the lower face (the closest point of a convex body is unique, so a tie does not change it)
 *   star      for every face without V[0] the tetrahedron (V[0], Vi, Vj, Vk) (:463-486); the point takes its four barycentric
 *             coordinates from the tetrahedron in which its smallest coordinate is largest, a tie to the lower face: on a shared face
 *             both neighbours give the same weights, so this is the reference's "first tetrahedron that contains it" without the
 *             dependence on qhull's face order.  All other columns are 0.
 *   out       the columns in the caller's palette order (:541-543)
 * points: PNR_LUT_POINTS_FP32 / _FP64: [N,3] on the device with point_stride elements between rows (>= 3: a frame's columns are read in
 * place); PNR_LUT_POINTS_BINS: points NULL, N = 32 768, point n = ((code + 0.5) / 32 per channel, r most significant) of code n -- the
 * fp32 bin centres of compute_RGB_histogram, exact -- nothing is uploaded.  normalize_input: every point becomes (c + 0.05) / |c + 0.05|
 * in float64 first, the norm as sqrt((c0 c0 + c1 c1) + c2 c2) (palette/utils.py:237-240: --use_normalized_palette).
 * weights64 [N,M] float64 and lut32 fp32 are both optional, one is required.  lut32 holds the float64 results rounded once, as [N,M] for
 * an array of points and as element (k, ir, ig, ib) of [1,M,32,32,32] for PNR_LUT_POINTS_BINS: bit for bit what initialize_palette forms
 * from the [32,32,32,M] float64 table.
 * info [4]: the status, the hull's faces, its star tetrahedra, 0.  The palette is known on the device only, so its refusals are answered
 * in info[0], not in the return value, and then NO weight is written:
 *   PNR_LUT_FLAT      no triple has a row off its plane by more than 1e-9 (fewer than four non-coplanar rows): there is no hull
 *   PNR_LUT_COPLANAR  a supporting plane carries a fourth row within 1e-9: the triangulation of that facet is a choice, and so are the
 *                     weights (the reference's answer depends on qhull there) -- refused rather than picked
 * Launch shape: min(1024, ceil(N / 128)) workgroups of 128 lanes, one point per lane, a workgroup walking contiguous runs of 128 points
 * (pnr_launch_geometry("pnr_lut_weights", N)); every workgroup rebuilds the hull in LDS itself.  No atomics, every sum and minimum in a
 * fixed order: two runs give the same bits, and a row's result does not depend on the batch it came in.
 * Order of the checks, all before any launch: a NULL struct, palette or info, neither output, M outside 4..16 -> PNR_ERR_INVALID; an
 * unknown points_format -> PNR_ERR_UNSUPPORTED; PNR_LUT_POINTS_BINS with points or N != 32 768, an array without points, with a stride
 * below 3 or a base not aligned to its element, a misaligned palette or output -> PNR_ERR_INVALID. */
#define PNR_LUT_MIN_M 4
#define PNR_LUT_MAX_M 16
#define PNR_LUT_MAX_FACES 28
#define PNR_LUT_POINTS_BINS 0
#define PNR_LUT_POINTS_FP32 1
#define PNR_LUT_POINTS_FP64 2
#define PNR_LUT_OK 0
#define PNR_LUT_FLAT 1
#define PNR_LUT_COPLANAR 2
typedef struct pnr_lut_weights_args {
    const double* palette;              /* [M,3] on the device, the caller's order */
    uint32_t M;
    const void* points;                 /* [N,3] with a row stride, or NULL (PNR_LUT_POINTS_BINS) */
    int points_format;                  /* PNR_LUT_POINTS_* */
    uint64_t point_stride;              /* elements between rows */
    uint32_t N;
    int normalize_input;
    double* weights64;                  /* [N,M] out, optional */
    float* lut32;                       /* [N,M], or [M,32,32,32] for the bins; out, optional */
    int32_t* info;                      /* [4] out */
} pnr_lut_weights_args;
int pnr_lut_weights(const pnr_lut_weights_args* args, pnr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PNR_H_ */
