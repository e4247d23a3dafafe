// adam.hip -- the optimiser step of the training path as ONE launch over every parameter tensor.
//
// The reference trains with torch.optim.Adam(lr, betas=(0.9, 0.99), eps=1e-15) (main_nerf.py:113, main_palette.py:223); torch runs it as
// seven elementwise kernels per parameter tensor (lerp, mul, addcmul, sqrt, mul, add, addcdiv): ~75 launches and seven passes over the
// 50 MB hash tables per step.  Here every element of every tensor makes one trip: read p, g, m, v -- write p, m, v.
// The arithmetic is torch's, operation for operation and rounding for rounding (torch/optim/adam.py:_multi_tensor_adam, what
// torch.optim.Adam runs by default on the GPU; the forms its kernels use on this build were measured with profiles/micro/adam_probe.py:
// lerp = fma(w, g - m, m); addcmul = fma(alpha, g * g, v); division by the fp32 scalar; addcdiv = fma(alpha, m / denom, p)), so that a
// training run is bit-identical to one driven by torch.optim.Adam (tests/test_gpu_ops.py).
#include "pnr_common.hpp"
#include <type_traits>

namespace pnr {

constexpr int kAdamMaxTensors = 32;
constexpr uint32_t kAdamThreads = 256, kAdamPerThread = 8, kAdamChunk = kAdamThreads * kAdamPerThread;

struct AdamTensor { float* p; const float* g; float* m; float* v; uint64_t n; };
struct AdamTable {
    AdamTensor t[kAdamMaxTensors];
    uint32_t first_chunk[kAdamMaxTensors + 1];   // chunk index at which every tensor starts (prefix sum of ceil(n / kAdamChunk))
    int count;
};
struct AdamScalars { float w1, beta2, c2, bc2_sqrt, inv_bc2_sqrt, eps, neg_step_size; float inv_grad_scale; int variant; };

// The loss-scaled (-O) step: GradScaler.step without its read-back.  `rows` are the host scalars of the step for every number of steps the device
// may have skipped since the host last looked (row r: r unobserved skips, i.e. a true step count r lower); `state` = {skipped, skipped, error}: the
// number of skipped steps so far as a ping-pong pair -- every workgroup of every launch of one step reads state[cur], and the first thread of each
// launch writes state[cur ^ 1] = state[cur] + (found_inf != 0), the same value from every launch of the step -- and an error word.
constexpr int kAdamAmpRows = 8;
struct AdamAmp {
    AdamScalars rows[kAdamAmpRows];
    const float* scale; const float* found_inf; int32_t* state;
    int32_t skipped_base, n_rows, cur;
};

template <bool kAmp>
__global__ void __launch_bounds__(kAdamThreads) k_adam(AdamTable tab, std::conditional_t<kAmp, AdamAmp, AdamScalars> a) {
    AdamScalars amp_row;
    if constexpr (kAmp) {
        const int32_t skipped = a.state[a.cur];
        const bool overflow = *a.found_inf != 0.0f;
        const int32_t r = skipped - a.skipped_base;
        const bool bad = !overflow && (r < 0 || r >= a.n_rows);              // never: the host bounds its run-ahead by the number of rows
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.state[a.cur ^ 1] = skipped + (overflow ? 1 : 0);
            if (bad) a.state[2] = 1;
        }
        if (overflow || bad) return;                                          // a skipped step: no store to any tensor
        amp_row = a.rows[r];
        amp_row.inv_grad_scale = (float)(1.0 / (double)*a.scale);            // torch: _scale.double().reciprocal().float()
    }
    const AdamScalars& s = [&]() -> const AdamScalars& { if constexpr (kAmp) return amp_row; else return a; }();
    int ti = 0;
    while (ti + 1 < tab.count && blockIdx.x >= tab.first_chunk[ti + 1]) ti++;   // <= 32 scalar compares
    const AdamTensor t = tab.t[ti];
    const uint64_t base = (uint64_t)(blockIdx.x - tab.first_chunk[ti]) * kAdamChunk;
#pragma unroll
    for (uint32_t k = 0; k < kAdamPerThread; k++) {
        const uint64_t i = base + (uint64_t)k * kAdamThreads + threadIdx.x;
        if (i >= t.n) break;
        float g = t.g[i];
        if (s.inv_grad_scale != 1.0f) g *= s.inv_grad_scale;        // GradScaler.unscale_ folded in (a separate torch kernel otherwise)
        float m = t.m[i], v = t.v[i];
        // exp_avg.lerp_(grad, 1 - beta1): |weight| < 0.5 -> self + weight * (end - self)           (ATen/native/Lerp.h)
        m = fmaf(s.w1, g - m, m);
        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2): a + alpha * (b * c), the product b * c rounded first
        // (PointwiseOpsKernel.cu; which of the candidate forms torch's build uses was measured: profiles/micro/adam_probe.py)
        v = v * s.beta2;
        v = (s.variant & 2) ? fmaf(s.c2 * g, g, v) : fmaf(s.c2, g * g, v);
        // denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps).  torch's default (foreach) implementation divides by the fp32 scalar;
        // its single-tensor kernels turn a division by a host scalar into a multiplication by the fp32 reciprocal -- variant bit 0
        const float denom = ((s.variant & 1) ? sqrtf(v) * s.inv_bc2_sqrt : sqrtf(v) / s.bc2_sqrt) + s.eps;
        // param.addcdiv_(exp_avg, denom, value = -step_size): a + alpha * (b / c)
        const float q = m / denom;
        t.p[i] = (s.variant & 4) ? t.p[i] + s.neg_step_size * q : fmaf(s.neg_step_size, q, t.p[i]);
        t.m[i] = m; t.v[i] = v;
    }
}

// GradScaler's finite check on the scaled gradients (torch._amp_foreach_non_finite_check_and_unscale_'s test, without its write pass): every
// element read once; the only store is *found_inf = 1 -- the same value from whichever lanes find one, so no atomic -- and never a clear.
__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ void __launch_bounds__(kAdamThreads) k_grad_check(AdamTable tab, float* found_inf) {
    int ti = 0;
    while (ti + 1 < tab.count && blockIdx.x >= tab.first_chunk[ti + 1]) ti++;
    const float* g = tab.t[ti].g;
    const uint64_t n = tab.t[ti].n;
    const uint64_t base = (uint64_t)(blockIdx.x - tab.first_chunk[ti]) * kAdamChunk + threadIdx.x;
    bool bad = false;
    if (base - threadIdx.x + kAdamChunk <= n) {                               // a whole chunk: eight loads in flight
        float x[kAdamPerThread];
#pragma unroll
        for (uint32_t k = 0; k < kAdamPerThread; k++) x[k] = g[base + (uint64_t)k * kAdamThreads];
#pragma unroll
        for (uint32_t k = 0; k < kAdamPerThread; k++) bad |= not_finite(x[k]);
    } else {
        for (uint32_t k = 0; k < kAdamPerThread; k++) {
            const uint64_t i = base + (uint64_t)k * kAdamThreads;
            if (i >= n) break;
            bad |= not_finite(g[i]);
        }
    }
    if (bad) *found_inf = 1.0f;
}

// The weights' average (torch_ema's ExponentialMovingAverage, which every recipe of the reference keeps: main_nerf.py:151, main_palette.py:228)
// on its own, over the same kind of chunk table: kSwap = false is torch_ema's update -- tmp = s - p; tmp.mul_(w); s.sub_(tmp), three launches and
// eight passes per tensor there -- as one trip, read p and s, write s, with its roundings: the product and the subtraction are NOT one fma (the intrinsics
// say so whatever the unit's contraction setting; grid_core.hpp: half_of_product is the precedent).  kSwap = true exchanges p and s in place: what
// store + copy_to and, called again, restore do around an evaluation, without their third copy of every table.
struct EmaTensor { float* p; float* s; uint64_t n; };
struct EmaTable {
    EmaTensor t[kAdamMaxTensors];
    uint32_t first_chunk[kAdamMaxTensors + 1];
    int count;
};

__device__ __forceinline__ float ema_next(float s, float p, float w) { return __fsub_rn(s, __fmul_rn(__fsub_rn(s, p), w)); }

template <bool kSwap>
__global__ void __launch_bounds__(kAdamThreads) k_ema(EmaTable tab, float w) {
    int ti = 0;
    while (ti + 1 < tab.count && blockIdx.x >= tab.first_chunk[ti + 1]) ti++;
    const EmaTensor t = tab.t[ti];
    const uint64_t base = (uint64_t)(blockIdx.x - tab.first_chunk[ti]) * kAdamChunk + threadIdx.x;
    if (base - threadIdx.x + kAdamChunk <= t.n) {                             // a whole chunk: sixteen loads in flight
        float p[kAdamPerThread], s[kAdamPerThread];
#pragma unroll
        for (uint32_t k = 0; k < kAdamPerThread; k++) { p[k] = t.p[base + (uint64_t)k * kAdamThreads]; s[k] = t.s[base + (uint64_t)k * kAdamThreads]; }
#pragma unroll
        for (uint32_t k = 0; k < kAdamPerThread; k++) {
            if constexpr (kSwap) { t.p[base + (uint64_t)k * kAdamThreads] = s[k]; t.s[base + (uint64_t)k * kAdamThreads] = p[k]; }
            else t.s[base + (uint64_t)k * kAdamThreads] = ema_next(s[k], p[k], w);
        }
    } else {
        for (uint32_t k = 0; k < kAdamPerThread; k++) {
            const uint64_t i = base + (uint64_t)k * kAdamThreads;
            if (i >= t.n) break;
            const float p = t.p[i], s = t.s[i];
            if constexpr (kSwap) { t.p[i] = s; t.s[i] = p; }
            else t.s[i] = ema_next(s, p, w);
        }
    }
}

}  // namespace pnr

using namespace pnr;

template <bool kSwap>
static int ema_launch(const pnr_ema_tensor* tensors, uint32_t count, float w, pnr_stream_t stream) {
    if (count == 0) return PNR_OK;
    if (!tensors) return PNR_ERR_INVALID;
    if (count > (uint32_t)kAdamMaxTensors) return PNR_ERR_UNSUPPORTED;
    EmaTable tab;
    uint64_t chunks = 0;
    int used = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (tensors[i].n == 0) continue;
        if (!tensors[i].param || !tensors[i].shadow) return PNR_ERR_INVALID;
        tab.t[used] = EmaTensor{tensors[i].param, tensors[i].shadow, tensors[i].n};
        tab.first_chunk[used] = (uint32_t)chunks;
        chunks += (tensors[i].n + kAdamChunk - 1) / kAdamChunk;
        used++;
    }
    if (chunks > 0x7fffffffull) return PNR_ERR_UNSUPPORTED;
    if (chunks == 0) return PNR_OK;
    tab.first_chunk[used] = (uint32_t)chunks;
    tab.count = used;
    hipLaunchKernelGGL(k_ema<kSwap>, dim3((uint32_t)chunks), dim3(kAdamThreads), 0, as_stream(stream), tab, w);
    return check_launch();
}

extern "C" {

uint32_t pnr_adam_max_tensors(void) { return kAdamMaxTensors; }

// the chunk table of the tensors with n > 0 (grads_only: pnr_grad_check's, which needs no other pointer); PNR_OK with *chunks == 0 = nothing to launch
static int adam_table(const pnr_adam_tensor* tensors, uint32_t count, bool grads_only, AdamTable& tab, uint64_t* chunks_out) {
    uint64_t chunks = 0;
    int used = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (tensors[i].n == 0) continue;
        if (!tensors[i].grad || (!grads_only && (!tensors[i].param || !tensors[i].exp_avg || !tensors[i].exp_avg_sq))) return PNR_ERR_INVALID;
        tab.t[used] = AdamTensor{tensors[i].param, tensors[i].grad, tensors[i].exp_avg, tensors[i].exp_avg_sq, tensors[i].n};
        tab.first_chunk[used] = (uint32_t)chunks;
        chunks += (tensors[i].n + kAdamChunk - 1) / kAdamChunk;
        used++;
    }
    if (chunks > 0x7fffffffull) return PNR_ERR_UNSUPPORTED;
    tab.first_chunk[used] = (uint32_t)chunks;
    tab.count = used;
    *chunks_out = chunks;
    return PNR_OK;
}

static AdamScalars adam_scalars(const pnr_adam_scalars* sc) {
    AdamScalars s;
    s.w1 = sc->one_minus_beta1; s.beta2 = sc->beta2; s.c2 = sc->one_minus_beta2; s.bc2_sqrt = sc->bias_correction2_sqrt; s.inv_bc2_sqrt = 1.0f / sc->bias_correction2_sqrt; s.eps = sc->eps;
    s.neg_step_size = sc->neg_step_size;
    s.inv_grad_scale = sc->inv_grad_scale > 0.0f ? sc->inv_grad_scale : 1.0f;
    s.variant = g_opt_adam_variant;
    return s;
}

int pnr_adam_step(const pnr_adam_tensor* tensors, uint32_t count, const pnr_adam_scalars* sc, pnr_stream_t stream) {
    if (count == 0) return PNR_OK;
    if (!tensors || !sc) return PNR_ERR_INVALID;
    if (count > (uint32_t)kAdamMaxTensors) return PNR_ERR_UNSUPPORTED;
    AdamTable tab;
    uint64_t chunks = 0;
    if (int rc = adam_table(tensors, count, false, tab, &chunks)) return rc;
    if (chunks == 0) return PNR_OK;
    hipLaunchKernelGGL(k_adam<false>, dim3((uint32_t)chunks), dim3(kAdamThreads), 0, as_stream(stream), tab, adam_scalars(sc));
    return check_launch();
}

int pnr_grad_check(const pnr_adam_tensor* tensors, uint32_t count, float* found_inf, pnr_stream_t stream) {
    if (count == 0) return PNR_OK;
    if (!tensors || !found_inf) return PNR_ERR_INVALID;
    if (count > (uint32_t)kAdamMaxTensors) return PNR_ERR_UNSUPPORTED;
    AdamTable tab;
    uint64_t chunks = 0;
    if (int rc = adam_table(tensors, count, true, tab, &chunks)) return rc;
    if (chunks == 0) return PNR_OK;
    hipLaunchKernelGGL(k_grad_check, dim3((uint32_t)chunks), dim3(kAdamThreads), 0, as_stream(stream), tab, found_inf);
    return check_launch();
}

int pnr_adam_step_amp(const pnr_adam_tensor* tensors, uint32_t count, const pnr_adam_scalars* rows, uint32_t n_rows, const pnr_adam_amp_ctl* ctl,
                      pnr_stream_t stream) {
    if (count == 0) return PNR_OK;
    if (!tensors || !rows || !ctl || !ctl->scale || !ctl->found_inf || !ctl->state) return PNR_ERR_INVALID;
    if (count > (uint32_t)kAdamMaxTensors || n_rows == 0 || n_rows > (uint32_t)kAdamAmpRows) return PNR_ERR_UNSUPPORTED;
    AdamTable tab;
    uint64_t chunks = 0;
    if (int rc = adam_table(tensors, count, false, tab, &chunks)) return rc;
    if (chunks == 0) return PNR_OK;
    AdamAmp a;
    for (uint32_t r = 0; r < (uint32_t)kAdamAmpRows; r++) a.rows[r] = adam_scalars(&rows[r < n_rows ? r : n_rows - 1]);
    a.scale = ctl->scale; a.found_inf = ctl->found_inf; a.state = ctl->state;
    a.skipped_base = ctl->skipped_base; a.n_rows = (int32_t)n_rows; a.cur = ctl->parity & 1;
    hipLaunchKernelGGL(k_adam<true>, dim3((uint32_t)chunks), dim3(kAdamThreads), 0, as_stream(stream), tab, a);
    return check_launch();
}

int pnr_ema_update(const pnr_ema_tensor* tensors, uint32_t count, float one_minus_decay, pnr_stream_t stream) {
    return ema_launch<false>(tensors, count, one_minus_decay, stream);
}

int pnr_ema_swap(const pnr_ema_tensor* tensors, uint32_t count, pnr_stream_t stream) { return ema_launch<true>(tensors, count, 0.0f, stream); }

}  // extern "C"
