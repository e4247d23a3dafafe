// stylizer.hip -- the GUI's "optimize" step for gfx950 (palette/gui.py:153-194): fit a Stylizer (palette/renderer.py:150-183) to M picked points.
//
// The reference evaluates the field at the M clicked points once and then runs 1000 iterations of SGD with momentum on dI [nb], dP [nb,3] and
// ddelta [nb,3,3] against the clicked colours -- 40-50 small launches per iteration, all serially dependent.  The arithmetic is a few kFLOP per
// iteration, so the whole optimisation is ONE launch of ONE wave:
//   s_n   = softplus(r_n)                      I_np  = max(s_n + dI_p, 0)
//   C_npj = P_pj + dP_pj + sum_i off_npi ddelta_pij
//   rgb_nj = sum_p omega_np clamp(I_np C_npj, 0, 1) (+ view_dep_nj)          e = rgb - target
//   loss  = sum e^2 + lambda (sum_p |D_p D_p^T - 1|_F^2 + sum dP^2)
//   g_npj = 2 e_nj omega_np [0 <= I_np C_npj <= 1]                             (torch's clamp gradient: bounds inclusive)
//   grad dP_pj = sum_n g_npj I_np + 2 lambda dP_pj        grad ddelta_pij = sum_n off_npi g_npj I_np + 4 lambda ((D_p D_p^T - 1) D_p)_ij
//   grad dI_p  = sum_n [s_n + dI_p >= 0] sum_j g_npj C_npj
//   buf = momentum buf + grad (the first step without buffers: buf = grad);   x -= lr[t] buf
// Shape: points stride over the 64 lanes (point n on lane n % 64, trip n / 64); their constants, softplus applied, are staged in LDS once
// and so is the learning-rate table, so that the loop touches global memory only for the optional trace.  The 13 nb + 1 sums over points (the
// gradients and the data loss) are taken in a fixed order: a lane adds its trips in turn, lanes l and l + 32 are added in-register, the 32
// partials of a sum are laid out as an LDS row, and the lane that OWNS the parameter (lane k % 64 owns parameter k) adds its row in four
// strided chains and combines them.  The owner keeps the parameter and its momentum buffer in registers, adds the regulariser's gradient,
// steps, and publishes the new value in LDS, from where every lane reads all parameters at one address each (a broadcast).  No atomics, one
// workgroup whatever M is: a run is reproducible bit for bit.  All fp32, nothing contracted.
#include "pnr_common.hpp"

namespace pnr {

constexpr uint32_t kStyMaxPoints = PNR_STYLIZER_MAX_POINTS;
constexpr uint32_t kStyMaxIters = PNR_STYLIZER_MAX_ITERS;
constexpr uint32_t kStyMinBasis = 4;
constexpr uint32_t kStyRedStride = 36;       // floats per row of the reduction image: 32 partials + 4, so that rows start 16-byte aligned and
                                             // the owners' ds_read_b128 of 16 neighbouring rows fall on 16 distinct 4-bank slots
constexpr uint32_t kStyLdsLimit = 160 * 1024;

// F.softplus, beta 1, threshold 20, as the training kernels write it (palette_train.hip).  The frame kernels' __logf(1 + __expf(x)) rounds 1 + e^x
// to an ulp of 1, a relative error of 1e-6 in a small s_n; once, before the loop, the exact form costs nothing, and with the fast one the gradient
// at (M, nb) = (3, 4) missed its bound against float64 (3.8e-7 against 4 x 6.0e-8).
__device__ __forceinline__ float sty_softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }

template <int NB>
struct StyShape {
    static constexpr int kParams = 13 * NB;            // dI | dP | ddelta, flat in that order
    static constexpr int kRows = kParams + 1;          // + the data loss
    static constexpr int kSlots = (kRows + 63) / 64;   // rows a lane owns
    static constexpr int kFields = 4 * NB + 7;         // per point: s | omega | offsets | target | view_dep
    static constexpr int kPrm = 16 * NB;               // LDS: dI | P + dP | ddelta (read by every lane) | dP (for the regulariser)
};

// floats of dynamic LDS (host and device agree through this one function)
__host__ __device__ inline uint32_t sty_lds_floats(uint32_t nb, uint32_t M, uint32_t iters) {
    const uint32_t mpad = (M + 63) / 64 * 64;
    return 16 * nb + 32 + (13 * nb + 1) * kStyRedStride + ((iters + 3) & ~3u) + (4 * nb + 7) * mpad;
}
static_assert((16 * PNR_MAX_BASIS + 32 + (13 * PNR_MAX_BASIS + 1) * kStyRedStride + kStyMaxIters + (4 * PNR_MAX_BASIS + 7) * kStyMaxPoints) * 4 <= kStyLdsLimit,
              "the largest supported fit has to fit the LDS of one CU");

enum { kStyDI = 0, kStyDP = 1, kStyDD = 2, kStyLoss = 3, kStyNone = 4 };

template <int NB>
__global__ void __launch_bounds__(64) k_stylizer_fit(const pnr_stylizer_fit_args a) {
    typedef StyShape<NB> S;
    extern __shared__ __align__(16) float sty_lds[];
    const uint32_t lane = threadIdx.x, M = a.M, iters = a.iters;
    const uint32_t trips = (M + 63) / 64, mpad = trips * 64;
    float* prm = sty_lds;                                  // [16 NB]
    float* regt = prm + S::kPrm;                           // [32]: per basis |D D^T - 1|^2, then per basis sum_j dP^2
    float* red = regt + 32;                                // [kRows][kStyRedStride]
    float* lrs = red + S::kRows * kStyRedStride;           // [iters]
    float* pts = lrs + ((iters + 3) & ~3u);                // [kFields][mpad]

    // ---- once: the points' constants and the learning rates into LDS; a point past M is all zeros and contributes exact zeros ----
    for (uint32_t n = lane; n < mpad; n += 64) {
        const bool in = n < M;
        pts[n] = in ? sty_softplus(a.radiance[n]) : 0.0f;
        for (int p = 0; p < NB; p++) pts[(1 + p) * mpad + n] = in ? a.omega[(size_t)n * NB + p] : 0.0f;
        for (int c = 0; c < 3 * NB; c++) pts[(1 + NB + c) * mpad + n] = in ? a.offsets[(size_t)n * 3 * NB + c] : 0.0f;
        for (int j = 0; j < 3; j++) {
            pts[(1 + 4 * NB + j) * mpad + n] = in ? a.target[(size_t)n * 3 + j] : 0.0f;
            pts[(4 + 4 * NB + j) * mpad + n] = in && a.view_dep ? a.view_dep[(size_t)n * 3 + j] : 0.0f;
        }
    }
    for (uint32_t t = lane; t < iters; t += 64) lrs[t] = a.lr[t];

    // ---- the rows this lane owns ----
    int kind[S::kSlots];
    uint32_t dbase[S::kSlots], di[S::kSlots], dj[S::kSlots];   // ddelta: LDS index of D_p, row, column
    float x[S::kSlots], buf[S::kSlots], pal[S::kSlots];
#pragma unroll
    for (int s = 0; s < S::kSlots; s++) {
        const uint32_t k = lane + 64 * s;
        kind[s] = k < NB ? kStyDI : k < 4 * NB ? kStyDP : k < 13 * NB ? kStyDD : k == 13 * NB ? kStyLoss : kStyNone;
        x[s] = buf[s] = pal[s] = 0.0f;
        dbase[s] = di[s] = dj[s] = 0;
        if (kind[s] == kStyDI) {
            x[s] = a.dI[k];
            if (a.has_momentum) buf[s] = a.mom_dI[k];
        } else if (kind[s] == kStyDP) {
            x[s] = a.dP[k - NB];
            pal[s] = a.palette[k - NB];
            if (a.has_momentum) buf[s] = a.mom_dP[k - NB];
        } else if (kind[s] == kStyDD) {
            const uint32_t q = k - 4 * NB, p = q / 9, r = q - 9 * p;
            x[s] = a.ddelta[q];
            if (a.has_momentum) buf[s] = a.mom_ddelta[q];
            dbase[s] = 4 * NB + 9 * p;
            di[s] = r / 3;
            dj[s] = r - 3 * di[s];
        }
        if (kind[s] == kStyDI || kind[s] == kStyDD) prm[k] = x[s];
        if (kind[s] == kStyDP) { prm[k] = pal[s] + x[s]; prm[13 * NB + (k - NB)] = x[s]; }
    }
    __syncthreads();

    const float lambda = a.lambda_arap, mu = a.momentum;
    for (uint32_t t = 0; t < iters; t++) {
        // ---- every lane: all parameters (one address per read: a broadcast), then its points ----
        float P[S::kParams];
#pragma unroll
        for (int k = 0; k < S::kParams; k++) P[k] = prm[k];
        float acc[S::kRows];
#pragma unroll
        for (int k = 0; k < S::kRows; k++) acc[k] = 0.0f;
        for (uint32_t trip = 0; trip < trips; trip++) {
            const float* pt = pts + trip * 64 + lane;
            const float sp = pt[0];
            float inten[NB], col[NB][3], rgb[3] = {0.0f, 0.0f, 0.0f};
            bool inside[NB][3];
#pragma unroll
            for (int p = 0; p < NB; p++) {
                inten[p] = fmaxf(sp + P[p], 0.0f);
                const float om = pt[(1 + p) * mpad];
                const float o0 = pt[(1 + NB + 3 * p) * mpad], o1 = pt[(2 + NB + 3 * p) * mpad], o2 = pt[(3 + NB + 3 * p) * mpad];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float* D = P + 4 * NB + 9 * p;
                    col[p][j] = P[NB + 3 * p + j] + ((o0 * D[j] + o1 * D[3 + j]) + o2 * D[6 + j]);
                    const float b = inten[p] * col[p][j];
                    inside[p][j] = b >= 0.0f && b <= 1.0f;
                    rgb[j] += om * fminf(fmaxf(b, 0.0f), 1.0f);
                }
            }
            float e2[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float e = (rgb[j] + pt[(4 + 4 * NB + j) * mpad]) - pt[(1 + 4 * NB + j) * mpad];
                acc[S::kParams] += e * e;
                e2[j] = 2.0f * e;
            }
#pragma unroll
            for (int p = 0; p < NB; p++) {
                const float om = pt[(1 + p) * mpad];
                const float o0 = pt[(1 + NB + 3 * p) * mpad], o1 = pt[(2 + NB + 3 * p) * mpad], o2 = pt[(3 + NB + 3 * p) * mpad];
                float gi = 0.0f;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float g = inside[p][j] ? e2[j] * om : 0.0f;
                    const float h = g * inten[p];
                    gi += g * col[p][j];
                    acc[NB + 3 * p + j] += h;
                    acc[4 * NB + 9 * p + j] += o0 * h;
                    acc[4 * NB + 9 * p + 3 + j] += o1 * h;
                    acc[4 * NB + 9 * p + 6 + j] += o2 * h;
                }
                acc[p] += sp + P[p] >= 0.0f ? gi : 0.0f;
            }
        }
        // ---- the sums over lanes: l + (l + 32) in registers, then one LDS row of 32 per sum ----
#pragma unroll
        for (int k = 0; k < S::kRows; k++) {
            const float v = acc[k] + __shfl_xor(acc[k], 32, 64);
            if (lane < 32) red[k * kStyRedStride + lane] = v;
        }
        __syncthreads();
        float g[S::kSlots];
#pragma unroll
        for (int s = 0; s < S::kSlots; s++) {
            g[s] = 0.0f;
            if (kind[s] == kStyNone) continue;
            const f32x4* row = reinterpret_cast<const f32x4*>(red + (lane + 64 * s) * kStyRedStride);
            f32x4 c = row[0];
#pragma unroll
            for (int i = 1; i < 8; i++) c += row[i];
            g[s] = (c[0] + c[1]) + (c[2] + c[3]);
            if (kind[s] == kStyDP) g[s] += (2.0f * lambda) * x[s];
            if (kind[s] == kStyDD) {
                const float* D = prm + dbase[s];     // E = D D^T - 1, row i of it; (E D)_ij
                float ed = 0.0f;
#pragma unroll
                for (int m = 0; m < 3; m++) {
                    float em = (D[3 * di[s]] * D[3 * m] + D[3 * di[s] + 1] * D[3 * m + 1]) + D[3 * di[s] + 2] * D[3 * m + 2];
                    if ((int)di[s] == m) em -= 1.0f;
                    ed += em * D[3 * m + dj[s]];
                }
                g[s] += (4.0f * lambda) * ed;
            }
        }
        if (a.trace) {     // (total loss, regulariser) at the parameters before this update
            if (lane < NB) {
                const float* D = prm + 4 * NB + 9 * lane;
                float ar = 0.0f, dp = 0.0f;
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int m = 0; m < 3; m++) {
                        const float em = ((D[3 * i] * D[3 * m] + D[3 * i + 1] * D[3 * m + 1]) + D[3 * i + 2] * D[3 * m + 2]) - (i == m ? 1.0f : 0.0f);
                        ar += em * em;
                    }
#pragma unroll
                for (int j = 0; j < 3; j++) dp += prm[13 * NB + 3 * lane + j] * prm[13 * NB + 3 * lane + j];
                regt[lane] = ar;
                regt[16 + lane] = dp;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < S::kSlots; s++)
                if (kind[s] == kStyLoss) {
                    float ar = 0.0f, dp = 0.0f;
                    for (int p = 0; p < NB; p++) { ar += regt[p]; dp += regt[16 + p]; }
                    const float reg = ar * lambda + dp * lambda;
                    a.trace[2 * (size_t)t] = g[s] + reg;
                    a.trace[2 * (size_t)t + 1] = reg;
                }
        }
        __syncthreads();       // every read of the old parameters is done
        const float lr = lrs[t];
        const bool first = t == 0 && !a.has_momentum;
#pragma unroll
        for (int s = 0; s < S::kSlots; s++) {
            if (kind[s] > kStyDD) continue;
            const uint32_t k = lane + 64 * s;
            buf[s] = first ? g[s] : mu * buf[s] + g[s];
            x[s] = x[s] - lr * buf[s];
            if (kind[s] == kStyDP) { prm[k] = pal[s] + x[s]; prm[13 * NB + (k - NB)] = x[s]; }
            else prm[k] = x[s];
        }
        __syncthreads();
    }

#pragma unroll
    for (int s = 0; s < S::kSlots; s++) {
        const uint32_t k = lane + 64 * s;
        if (kind[s] == kStyDI) { a.dI[k] = x[s]; if (a.mom_dI) a.mom_dI[k] = buf[s]; }
        if (kind[s] == kStyDP) { a.dP[k - NB] = x[s]; if (a.mom_dP) a.mom_dP[k - NB] = buf[s]; }
        if (kind[s] == kStyDD) { a.ddelta[k - 4 * NB] = x[s]; if (a.mom_ddelta) a.mom_ddelta[k - 4 * NB] = buf[s]; }
    }
}

template <int NB>
int stylizer_launch(const pnr_stylizer_fit_args& a, uint32_t bytes, hipStream_t stream) {
    if (!raise_lds<k_stylizer_fit<NB>>(kStyLdsLimit)) return PNR_ERR_LAUNCH;
    hipLaunchKernelGGL(k_stylizer_fit<NB>, dim3(1), dim3(64), bytes, stream, a);
    return check_launch();
}

}  // namespace pnr

using namespace pnr;

extern "C" int pnr_stylizer_fit(const pnr_stylizer_fit_args* args, pnr_stream_t stream) {
    if (!args) return PNR_ERR_INVALID;
    const pnr_stylizer_fit_args& a = *args;
    if (a.num_basis < kStyMinBasis || a.num_basis > PNR_MAX_BASIS || a.M > kStyMaxPoints || a.iters > kStyMaxIters) return PNR_ERR_UNSUPPORTED;
    if (a.M == 0 || a.iters == 0) return PNR_OK;
    if (!a.radiance || !a.omega || !a.offsets || !a.palette || !a.target || !a.dI || !a.dP || !a.ddelta || !a.lr) return PNR_ERR_INVALID;
    const int n_mom = (a.mom_dI != nullptr) + (a.mom_dP != nullptr) + (a.mom_ddelta != nullptr);
    if ((n_mom != 0 && n_mom != 3) || (a.has_momentum && n_mom != 3)) return PNR_ERR_INVALID;
    const uint32_t bytes = sty_lds_floats(a.num_basis, a.M, a.iters) * 4;
    if (bytes > kStyLdsLimit) return PNR_ERR_UNSUPPORTED;
    hipStream_t s = as_stream(stream);
    switch (a.num_basis) {
        case 4: return stylizer_launch<4>(a, bytes, s);
        case 5: return stylizer_launch<5>(a, bytes, s);
        case 6: return stylizer_launch<6>(a, bytes, s);
        case 7: return stylizer_launch<7>(a, bytes, s);
        case 8: return stylizer_launch<8>(a, bytes, s);
        case 9: return stylizer_launch<9>(a, bytes, s);
        case 10: return stylizer_launch<10>(a, bytes, s);
    }
    return PNR_ERR_UNSUPPORTED;
}
