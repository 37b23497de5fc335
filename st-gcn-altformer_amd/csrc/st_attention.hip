// ST-TR's spatial self-attention unit, gcn_unit_attention (model/ST_TR/gcn_attention.py:25-156 with
// spatial_transformer.py:17-195 of the reference), in the configuration every reference script builds: only_attention,
// no relative / adjacency / more_channels, data_bn, skip connection, BatchNorm2d, drop-connect, Nh heads, dk = Cout/4,
// dv = Cout, 1x1 projections.  With x (N,Cin,T,V), every one of the B = N*T frames is a set of V joint tokens:
//
//   xn   = data_bn(x)                     BatchNorm1d over the (c,v) channels of the (N, Cin*V, T) view
//   qkv  = Wqkv . xn + bqkv               (2dk+dv, V) per frame; q, k, v and the heads are contiguous channel blocks
//   w    = softmax_j( (q_h*dkh^-0.5)^T k_h )          per (frame, head): V x V, soft-max over the KEY axis
//          (training, drop-connect: w = w*m[j] / (sum_j w*m[j] + 1e-8), m one Bernoulli(0.5) draw per (frame, head, key))
//   o_h  = w . v_h^T                      heads concatenated back to dv channels
//   z    = Wout . o + bout (+ x when Cin == Cout)
//   y    = relu(BatchNorm2d(z))
//
// Layout: every intermediate keeps the (clip, channel, frame, joint) order of x, so the two projections are plain per-clip
// GEMMs on the strided fp32-MFMA GEMM (gemm_f32.hip, v_mfma_f32_32x32x2_f32) or, with STGCN_MATH_BF16X3 in the flags, on the
// three-term bf16 kernel of wx_bf16.hip (the weight gradients stay on the former), and the heads' channels are rows of V floats.
// The V x V part runs in one workgroup (one wave) per (frame, head): lane i owns query row i; the head's keys and values
// are staged in LDS and read as broadcasts; logits, soft-max and o_h are exact fp32 FMAs in registers, and the V x V
// weights never leave the chip.  The training forward saves per row (max, sum of exponentials, drop-connect sum) and the
// backward recomputes the weights from them (P would be N*T*Nh*V^2 floats: 650 MB at the LMDHG layer-3 shape).
//
// Both BatchNorms use the training helpers of train_bn.hip / tcn_backward.hip.  data_bn's per-(c,v) statistics are summed
// in a fixed order (fp32 inside a (clip, thread) strip, fp64 across, parts added in order), BatchNorm2d's with the fp64
// atomics of bn_batch_stats (order-dependent only in the last fp64 bits).
#include <stdarg.h>

#include <cmath>

#include "common.h"

namespace stgcn {

namespace {

constexpr int kVP = 64;        // joints a wave covers (lane = joint)
constexpr float kDropEps = 1e-8f;

// ----------------------------------------------------------------------------------------------------------------------
// forward: one wave per (frame, head).  grid = (N*T, H)
// ----------------------------------------------------------------------------------------------------------------------
template <int DKH, int DVH>
__global__ __launch_bounds__(64) void sta_fwd_kernel(const float *__restrict__ qkv, const float *__restrict__ mask,
                                                     float *__restrict__ o, float *__restrict__ rowstats, int T, int V,
                                                     int H, float qscale) {
    __shared__ __attribute__((aligned(16))) float kT[kVP * DKH];   // [j][d]
    __shared__ __attribute__((aligned(16))) float vT[kVP * DVH];   // [j][e]
    __shared__ float msk[kVP];
    const int bt = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int n = bt / T, t = bt - n * T;
    const int dk = H * DKH, dv = H * DVH, Cq = 2 * dk + dv;
    const size_t TV = (size_t)T * V;
    const float *base = qkv + (size_t)n * Cq * TV + (size_t)t * V;   // + channel * TV + joint
    const float *qb = base + (size_t)(h * DKH) * TV;
    const float *kb = base + (size_t)(dk + h * DKH) * TV;
    const float *vb = base + (size_t)(2 * dk + h * DVH) * TV;
    for (int e = lane; e < DKH * V; e += 64) {
        const int d = e / V, j = e - d * V;
        kT[j * DKH + d] = kb[(size_t)d * TV + j];
    }
    for (int e = lane; e < DVH * V; e += 64) {
        const int c = e / V, j = e - c * V;
        vT[j * DVH + c] = vb[(size_t)c * TV + j];
    }
    const size_t row0 = ((size_t)bt * H + h) * V;                     // (frame, head) block of the mask / row statistics
    if (mask) msk[lane] = lane < V ? mask[row0 + lane] : 0.f;
    __syncthreads();
    if (lane >= V) return;
    float q[DKH];
#pragma unroll
    for (int d = 0; d < DKH; ++d) q[d] = qb[(size_t)d * TV + lane] * qscale;
    float s[kVP];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kVP; ++j) {
        if (j < V) {
            float a = 0.f;
#pragma unroll
            for (int d = 0; d < DKH; ++d) a = fmaf(q[d], kT[j * DKH + d], a);
            s[j] = a;
            mx = fmaxf(mx, a);
        }
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < kVP; ++j)
        if (j < V) {
            s[j] = __expf(s[j] - mx);
            l += s[j];
        }
    const float rl = 1.f / l;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < kVP; ++j)
        if (j < V) {
            float w = s[j] * rl;
            if (mask) {
                w *= msk[j];
                ss += w;
            }
            s[j] = w;
        }
    const float rs = mask ? 1.f / (ss + kDropEps) : 1.f;
    float acc[DVH];
#pragma unroll
    for (int e = 0; e < DVH; ++e) acc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < kVP; ++j) {
        if (j < V) {
            const float w = mask ? s[j] * rs : s[j];
#pragma unroll
            for (int e4 = 0; e4 < DVH / 4; ++e4) {
                const float4 v4 = *reinterpret_cast<const float4 *>(vT + j * DVH + 4 * e4);
                acc[4 * e4] = fmaf(w, v4.x, acc[4 * e4]);
                acc[4 * e4 + 1] = fmaf(w, v4.y, acc[4 * e4 + 1]);
                acc[4 * e4 + 2] = fmaf(w, v4.z, acc[4 * e4 + 2]);
                acc[4 * e4 + 3] = fmaf(w, v4.w, acc[4 * e4 + 3]);
            }
        }
    }
    float *ob = o + ((size_t)n * dv + h * DVH) * TV + (size_t)t * V + lane;
#pragma unroll
    for (int e = 0; e < DVH; ++e) ob[(size_t)e * TV] = acc[e];
    if (rowstats) {
        float4 *rsp = reinterpret_cast<float4 *>(rowstats) + row0 + lane;
        *rsp = make_float4(mx, l, ss, 0.f);
    }
}

// ----------------------------------------------------------------------------------------------------------------------
// backward of the V x V part: one wave per (frame, head).  From do_h and the saved row statistics: the weights are
// recomputed (same instructions as the forward: same bits), then
//   dw = do^T v;   drop-connect: dw1 = (dw - <dw, w>) / (ss + 1e-8), dw0 = dw1 * m;   dS = w0 * (dw0 - <w0, dw0>)
//   dq = dkh^-0.5 * dS k^T,   dk = (q*dkh^-0.5) dS,   dv = do w      (the last two: sums over query rows, through LDS)
// grid = (N*T, H)
// ----------------------------------------------------------------------------------------------------------------------
template <int DKH, int DVH>
__global__ __launch_bounds__(64) void sta_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ dout,
                                                     const float *__restrict__ mask, const float *__restrict__ rowstats,
                                                     float *__restrict__ dqkv, int T, int V, int H, float qscale) {
    extern __shared__ __attribute__((aligned(16))) float sta_lds[];
    float *kT = sta_lds;                      // [j][d]
    float *vT = kT + kVP * DKH;               // [j][e]
    float *qT = vT + kVP * DVH;               // [i][d]   (scaled q)
    float *doT = qT + kVP * DKH;              // [i][e]
    float *Pm = doT + kVP * DVH;              // [i][j], pitch kVP + 1: w, then dS
    float *msk = Pm + kVP * (kVP + 1);
    constexpr int PP = kVP + 1;
    const int bt = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int n = bt / T, t = bt - n * T;
    const int dk = H * DKH, dv = H * DVH, Cq = 2 * dk + dv;
    const size_t TV = (size_t)T * V;
    const size_t fo = (size_t)n * Cq * TV + (size_t)t * V;
    const float *qb = qkv + fo + (size_t)(h * DKH) * TV;
    const float *kb = qkv + fo + (size_t)(dk + h * DKH) * TV;
    const float *vb = qkv + fo + (size_t)(2 * dk + h * DVH) * TV;
    const float *db = dout + ((size_t)n * dv + h * DVH) * TV + (size_t)t * V;
    for (int e = lane; e < DKH * V; e += 64) {
        const int d = e / V, j = e - d * V;
        kT[j * DKH + d] = kb[(size_t)d * TV + j];
        qT[j * DKH + d] = qb[(size_t)d * TV + j] * qscale;
    }
    for (int e = lane; e < DVH * V; e += 64) {
        const int c = e / V, j = e - c * V;
        vT[j * DVH + c] = vb[(size_t)c * TV + j];
        doT[j * DVH + c] = db[(size_t)c * TV + j];
    }
    const size_t row0 = ((size_t)bt * H + h) * V;
    if (mask) msk[lane] = lane < V ? mask[row0 + lane] : 0.f;
    __syncthreads();
    float *gq = dqkv + fo + (size_t)(h * DKH) * TV;
    float *gk = dqkv + fo + (size_t)(dk + h * DKH) * TV;
    float *gv = dqkv + fo + (size_t)(2 * dk + h * DVH) * TV;
    const bool on = lane < V;
    float w0[kVP], dw[kVP];                          // this lane's query row: soft-max weights, then dS
#pragma unroll
    for (int j = 0; j < kVP; ++j) w0[j] = dw[j] = 0.f;
    if (on) {
        const float4 st = reinterpret_cast<const float4 *>(rowstats)[row0 + lane];
        const float mx = st.x, rl = 1.f / st.y, rs = mask ? 1.f / (st.z + kDropEps) : 1.f;
        float q[DKH];
#pragma unroll
        for (int d = 0; d < DKH; ++d) q[d] = qT[lane * DKH + d];
#pragma unroll
        for (int j = 0; j < kVP; ++j) {
            if (j < V) {
                float a = 0.f;
#pragma unroll
                for (int d = 0; d < DKH; ++d) a = fmaf(q[d], kT[j * DKH + d], a);
                w0[j] = __expf(a - mx) * rl;
                float g = 0.f;
#pragma unroll
                for (int e4 = 0; e4 < DVH / 4; ++e4) {
                    const float4 v4 = *reinterpret_cast<const float4 *>(vT + j * DVH + 4 * e4);
                    const float4 d4 = *reinterpret_cast<const float4 *>(doT + lane * DVH + 4 * e4);
                    g = fmaf(d4.x, v4.x, g);
                    g = fmaf(d4.y, v4.y, g);
                    g = fmaf(d4.z, v4.z, g);
                    g = fmaf(d4.w, v4.w, g);
                }
                dw[j] = g;
            }
        }
        if (mask) {                                  // w = w0*m*rs: dw1 = (dw - <dw, w>) * rs, dw0 = dw1 * m
            float c = 0.f;
#pragma unroll
            for (int j = 0; j < kVP; ++j)
                if (j < V) c = fmaf(dw[j], w0[j] * msk[j] * rs, c);
#pragma unroll
            for (int j = 0; j < kVP; ++j)
                if (j < V) dw[j] = (dw[j] - c) * rs * msk[j];
        }
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < kVP; ++j)
            if (j < V) dot = fmaf(w0[j], dw[j], dot);
        float gqa[DKH];
#pragma unroll
        for (int d = 0; d < DKH; ++d) gqa[d] = 0.f;
#pragma unroll
        for (int j = 0; j < kVP; ++j) {
            if (j < V) {
                Pm[lane * PP + j] = mask ? w0[j] * msk[j] * rs : w0[j];
                const float ds = w0[j] * (dw[j] - dot);
                dw[j] = ds;
#pragma unroll
                for (int d = 0; d < DKH; ++d) gqa[d] = fmaf(ds, kT[j * DKH + d], gqa[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < DKH; ++d) gq[(size_t)d * TV + lane] = gqa[d] * qscale;
    }
    __syncthreads();
    if (on) {                                        // dv[e][j] = sum_i w[i][j] do[i][e]   (lane = key j)
        float a[DVH];
#pragma unroll
        for (int e = 0; e < DVH; ++e) a[e] = 0.f;
        for (int i = 0; i < V; ++i) {
            const float w = Pm[i * PP + lane];
#pragma unroll
            for (int e4 = 0; e4 < DVH / 4; ++e4) {
                const float4 d4 = *reinterpret_cast<const float4 *>(doT + i * DVH + 4 * e4);
                a[4 * e4] = fmaf(w, d4.x, a[4 * e4]);
                a[4 * e4 + 1] = fmaf(w, d4.y, a[4 * e4 + 1]);
                a[4 * e4 + 2] = fmaf(w, d4.z, a[4 * e4 + 2]);
                a[4 * e4 + 3] = fmaf(w, d4.w, a[4 * e4 + 3]);
            }
        }
#pragma unroll
        for (int e = 0; e < DVH; ++e) gv[(size_t)e * TV + lane] = a[e];
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int j = 0; j < kVP; ++j)
            if (j < V) Pm[lane * PP + j] = dw[j];
    }
    __syncthreads();
    if (on) {                                        // dk[d][j] = sum_i dS[i][j] qs[i][d]
        float a[DKH];
#pragma unroll
        for (int d = 0; d < DKH; ++d) a[d] = 0.f;
        for (int i = 0; i < V; ++i) {
            const float ds = Pm[i * PP + lane];
#pragma unroll
            for (int d = 0; d < DKH; ++d) a[d] = fmaf(ds, qT[i * DKH + d], a[d]);
        }
#pragma unroll
        for (int d = 0; d < DKH; ++d) gk[(size_t)d * TV + lane] = a[d];
    }
}

// ----------------------------------------------------------------------------------------------------------------------
// data_bn: BatchNorm1d over the (c, v) channels of x (N,C,T,V), normalised over (n, t)
// ----------------------------------------------------------------------------------------------------------------------
// parts[(s*2 + k)*C*V + c*V + v], s = split over clips:  k = 0: sum a, k = 1: sum a^2 (g == NULL) or sum g*(a-mean)*invstd
// grid = (C, splits), 256 threads: v = tid & 63, frame phase tq = tid >> 6.  Fixed order throughout.
__global__ __launch_bounds__(256) void cv_stats_kernel(const float *__restrict__ a, const float *__restrict__ g,
                                                       const float *__restrict__ mean, const float *__restrict__ invstd,
                                                       double *__restrict__ parts, int N, int C, int T, int V) {
    __shared__ double red[2][4][kVP];
    const int c = blockIdx.x, s = blockIdx.y, splits = gridDim.y;
    const int v = threadIdx.x & 63, tq = threadIdx.x >> 6;
    const int per = (N + splits - 1) / splits, n_lo = s * per, n_hi = min(N, n_lo + per);
    const int cv = c * V + v;
    const bool on = v < V;
    const float m = (g && on) ? mean[cv] : 0.f, is = (g && on) ? invstd[cv] : 0.f;
    double d0 = 0.0, d1 = 0.0;
    if (on) {
        for (int n = n_lo; n < n_hi; ++n) {
            const float *ar = a + ((size_t)n * C + c) * T * V + v;
            const float *gr = g ? g + ((size_t)n * C + c) * T * V + v : nullptr;
            float f0 = 0.f, f1 = 0.f;
            for (int t = tq; t < T; t += 4) {
                const float x = ar[(size_t)t * V];
                if (gr) {
                    const float gg = gr[(size_t)t * V];
                    f0 += gg;
                    f1 = fmaf(gg, (x - m) * is, f1);
                } else {
                    f0 += x;
                    f1 = fmaf(x, x, f1);
                }
            }
            d0 += (double)f0;
            d1 += (double)f1;
        }
    }
    red[0][tq][v] = d0;
    red[1][tq][v] = d1;
    __syncthreads();
    if (tq == 0 && on) {
        const size_t CV = (size_t)C * V;
        parts[((size_t)s * 2) * CV + cv] = ((red[0][0][v] + red[0][1][v]) + red[0][2][v]) + red[0][3][v];
        parts[((size_t)s * 2 + 1) * CV + cv] = ((red[1][0][v] + red[1][1][v]) + red[1][2][v]) + red[1][3][v];
    }
}

// sums[k*CV + i] = sum_s parts[(s*2 + k)*CV + i] in the order s = 0, 1, ...
__global__ void cv_sum_parts_kernel(const double *__restrict__ parts, double *__restrict__ sums, int splits, int CV) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * CV) return;
    const int k = i / CV, r = i - k * CV;
    double acc = 0.0;
    for (int s = 0; s < splits; ++s) acc += parts[((size_t)s * 2 + k) * CV + r];
    sums[i] = acc;
}

// out = x*scale[cv] + shift[cv];  grid = (N*C rows, chunks of the T*V plane)
__global__ __launch_bounds__(256) void cv_apply_kernel(const float *__restrict__ x, const float *__restrict__ scale,
                                                       const float *__restrict__ shift, float *__restrict__ out, int C, int T,
                                                       int V) {
    const int row = blockIdx.x, c = row % C;
    const int TV = T * V;
    const int p = blockIdx.y * 256 + threadIdx.x;
    if (p >= TV) return;
    const int cv = c * V + p % V;
    const size_t e = (size_t)row * TV + p;
    out[e] = fmaf(x[e], scale[cv], shift[cv]);
}

// dx = coef[cv]*(g - coef[CV+cv] - (x - mean[cv])*invstd[cv]*coef[2CV+cv]) (+ res)
__global__ __launch_bounds__(256) void cv_bwd_apply_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ coef, const float *__restrict__ res,
                                                           float *__restrict__ dx, int C, int T, int V) {
    const int row = blockIdx.x, c = row % C;
    const int TV = T * V, CV = C * V;
    const int p = blockIdx.y * 256 + threadIdx.x;
    if (p >= TV) return;
    const int cv = c * V + p % V;
    const size_t e = (size_t)row * TV + p;
    float d = coef[cv] * (g[e] - coef[CV + cv] - (x[e] - mean[cv]) * invstd[cv] * coef[2 * CV + cv]);
    if (res) d += res[e];
    dx[e] = d;
}

// ----------------------------------------------------------------------------------------------------------------------
// launchers.  Every shape limit of a launch is one host predicate next to it: the launcher asks it, and so does
// plan_st_attention below, which refuses a call before its first launch.
// ----------------------------------------------------------------------------------------------------------------------
void say(Refusal &r, stgcn_status status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof(r.msg), fmt, ap);
    va_end(ap);
    r.status = status;
}

// sta_*: the instantiated per-head widths; one wave per (frame, head), lane = joint
bool sta_widths_covered(int dkh, int dvh) { return (dkh == 4 && dvh == 16) || (dkh == 8 && dvh == 32) || (dkh == 16 && dvh == 64); }
bool sta_covers(int N, int T, int V, int H) { return V >= 1 && V <= kVP && H >= 1 && H <= 65535 && grid_fits((long long)N * T, 64); }

size_t bwd_lds_bytes(int DKH, int DVH) {
    return sizeof(float) * ((size_t)2 * kVP * DKH + (size_t)2 * kVP * DVH + (size_t)kVP * (kVP + 1) + kVP);
}

int launch_sta_fwd(const float *qkv, const float *mask, float *o, float *rowstats, int N, int T, int V, int H, int dkh,
                   int dvh, hipStream_t st) {
    if (!sta_widths_covered(dkh, dvh) || !sta_covers(N, T, V, H))
        return fail(STGCN_ERR_UNSUPPORTED, "sta_fwd_kernel: N=%d T=%d V=%d heads=%d dkh=%d dvh=%d", N, T, V, H, dkh, dvh);
    const dim3 grid((unsigned)(N * T), (unsigned)H);
    const float qscale = (float)std::pow((double)dkh, -0.5);   // (the reference's Python scalar dkh ** -0.5)
    if (dkh == 4) hipLaunchKernelGGL((sta_fwd_kernel<4, 16>), grid, dim3(64), 0, st, qkv, mask, o, rowstats, T, V, H, qscale);
    else if (dkh == 8) hipLaunchKernelGGL((sta_fwd_kernel<8, 32>), grid, dim3(64), 0, st, qkv, mask, o, rowstats, T, V, H, qscale);
    else hipLaunchKernelGGL((sta_fwd_kernel<16, 64>), grid, dim3(64), 0, st, qkv, mask, o, rowstats, T, V, H, qscale);
    STGCN_LAUNCH_CHECK("sta_fwd_kernel");
    return STGCN_OK;
}

int launch_sta_bwd(const float *qkv, const float *dout, const float *mask, const float *rowstats, float *dqkv, int N, int T,
                   int V, int H, int dkh, int dvh, hipStream_t st) {
    if (!sta_widths_covered(dkh, dvh) || !sta_covers(N, T, V, H))
        return fail(STGCN_ERR_UNSUPPORTED, "sta_bwd_kernel: N=%d T=%d V=%d heads=%d dkh=%d dvh=%d", N, T, V, H, dkh, dvh);
    const dim3 grid((unsigned)(N * T), (unsigned)H);
    const float qscale = (float)std::pow((double)dkh, -0.5);
    const size_t lds = bwd_lds_bytes(dkh, dvh);
#define STA_BWD(A, B)                                                                                            \
    do {                                                                                                         \
        STGCN_HIP_CHECK(allow_lds(sta_bwd_kernel<A, B>, lds));                                                   \
        hipLaunchKernelGGL((sta_bwd_kernel<A, B>), grid, dim3(64), lds, st, qkv, dout, mask, rowstats, dqkv, T, V, H, \
                           qscale);                                                                              \
    } while (0)
    if (dkh == 4) STA_BWD(4, 16);
    else if (dkh == 8) STA_BWD(8, 32);
    else STA_BWD(16, 64);
#undef STA_BWD
    STGCN_LAUNCH_CHECK("sta_bwd_kernel");
    return STGCN_OK;
}

// cv_*: a grid row per (clip, channel) and 256 pixels of its plane a workgroup along grid.y; T*V and 2*C*V are ints in the kernels
bool cv_covers(int N, int C, int T, int V) {
    return N >= 1 && C >= 1 && T >= 1 && V >= 1 && V <= kVP && grid_fits((long long)N * C, 256) &&
           (long long)T * V <= 65535LL * 256 && 2LL * C * V <= 0x7fffffffLL;
}
int cv_refused(const char *kernel, int N, int C, int T, int V) {
    return fail(STGCN_ERR_UNSUPPORTED, "%s: N=%d C=%d T=%d V=%d exceed the grid", kernel, N, C, T, V);
}

int cv_splits(int N) { return N < 16 ? N : 16; }

int launch_cv_stats(const float *a, const float *g, const float *mean, const float *invstd, double *parts, double *sums,
                    int N, int C, int T, int V, hipStream_t st) {
    if (!cv_covers(N, C, T, V)) return cv_refused("cv_stats_kernel", N, C, T, V);
    const int splits = cv_splits(N);
    hipLaunchKernelGGL(cv_stats_kernel, dim3(C, splits), dim3(256), 0, st, a, g, mean, invstd, parts, N, C, T, V);
    STGCN_LAUNCH_CHECK("cv_stats_kernel");
    hipLaunchKernelGGL(cv_sum_parts_kernel, dim3(ceil_div(2 * C * V, 256)), dim3(256), 0, st, parts, sums, splits, C * V);
    STGCN_LAUNCH_CHECK("cv_sum_parts_kernel");
    return STGCN_OK;
}

int launch_cv_apply(const float *x, const float *scale, const float *shift, float *out, int N, int C, int T, int V,
                    hipStream_t st) {
    if (!cv_covers(N, C, T, V)) return cv_refused("cv_apply_kernel", N, C, T, V);
    hipLaunchKernelGGL(cv_apply_kernel, dim3(N * C, ceil_div(T * V, 256)), dim3(256), 0, st, x, scale, shift, out, C, T, V);
    STGCN_LAUNCH_CHECK("cv_apply_kernel");
    return STGCN_OK;
}

int launch_cv_bwd_apply(const float *g, const float *x, const float *mean, const float *invstd, const float *coef,
                        const float *res, float *dx, int N, int C, int T, int V, hipStream_t st) {
    if (!cv_covers(N, C, T, V)) return cv_refused("cv_bwd_apply_kernel", N, C, T, V);
    hipLaunchKernelGGL(cv_bwd_apply_kernel, dim3(N * C, ceil_div(T * V, 256)), dim3(256), 0, st, g, x, mean, invstd, coef, res,
                       dx, C, T, V);
    STGCN_LAUNCH_CHECK("cv_bwd_apply_kernel");
    return STGCN_OK;
}

// ----------------------------------------------------------------------------------------------------------------------
// One W . X product: C[n] = W . X[n] (+ bias) (+ R[n]), W (M,K) row-major (or (K,M): the input gradient through the weights)
// shared by the N clips, X[n] (K,TV), C[n] (M,TV).  Its plan serves the unit's four products and stgcn_wx_product*.
// ----------------------------------------------------------------------------------------------------------------------
// extents and strides of the product on the strided f32 GEMM; the pointers are the launcher's
GemmArgs wx_gemm(int M, int K, long long TV, bool w_transposed) {
    GemmArgs g{};
    if (w_transposed) { g.a_sm = 1; g.a_sk = M; }
    else { g.a_sm = K; g.a_sk = 1; }
    g.a_sb = 0;
    g.b_sk = TV; g.b_sn = 1; g.b_sb = (long long)K * TV;
    g.c_sm = TV; g.c_sn = 1; g.c_sb = (long long)M * TV;
    g.M = M; g.N = (int)TV; g.K = K;
    g.alpha = 1.f;
    return g;
}

struct WxPlan {
    enum Kernel { none, gemm_f32, bf16x3 } kernel = none;
    int M = 0, K = 0, N = 0;
    long long TV = 0;
    bool transposed = false;
    Refusal why;
};

// The arithmetic comes from the low 4 bits of `flags`.  Inside the unit (`alone` false) a product is covered where its own
// kernel is: the f32 GEMM up to 65535 * 64 columns, the bf16x3 kernel up to 65535 * 128.  The stand-alone entry point covers
// what BOTH kernels do and holds a clip to 2^31 - 1 elements, whichever arithmetic is asked for (include/stgcn_hip.h).
WxPlan plan_wx(const char *fn, int M, int K, long long TV, int N, bool w_transposed, unsigned flags, bool alone) {
    WxPlan p;
    p.M = M, p.K = K, p.N = N, p.TV = TV, p.transposed = w_transposed;
    if (N < 1 || M < 1 || K < 1 || TV < 1)
        return say(p.why, STGCN_ERR_ARG, "%s: non-positive dimension (N=%d M=%d K=%d TV=%lld)", fn, N, M, K, TV), p;
    const unsigned m = flags & STGCN_MATH_MASK;
    if (m != STGCN_MATH_F32 && m != STGCN_MATH_BF16X3) {
        const char *name = m == STGCN_MATH_BF16 ? "STGCN_MATH_BF16" : m == STGCN_MATH_F32_VALU ? "STGCN_MATH_F32_VALU" : "unknown";
        return say(p.why, STGCN_ERR_UNSUPPORTED, "%s: arithmetic %u (%s) is not implemented for this product; STGCN_MATH_F32 and "
                   "STGCN_MATH_BF16X3 are", fn, m, name), p;
    }
    const bool f32 = TV <= 0x7fffffffLL && gemm_f32_spans_fit(wx_gemm(M, K, TV, w_transposed)) &&
                     gemm_f32_grid_fits(wx_gemm(M, K, TV, w_transposed), N);
    const bool b3 = wx_bf16x3_covers(M, K, TV, N);
    const bool ok = alone ? f32 && b3 && (long long)(M > K ? M : K) * TV <= 0x7fffffffLL : (m == STGCN_MATH_F32 ? f32 : b3);
    if (!ok)
        return say(p.why, STGCN_ERR_UNSUPPORTED, "%s: N=%d M=%d K=%d TV=%lld exceed the grid or 2^31 elements a clip (%s product)", fn,
                   N, M, K, TV, m == STGCN_MATH_F32 ? "f32" : "bf16x3"), p;
    p.kernel = m == STGCN_MATH_F32 ? WxPlan::gemm_f32 : WxPlan::bf16x3;
    return p;
}

// f32: R is copied into C and the product accumulated onto it (the skip connection as it always ran); bf16x3: R is read in
// the kernel's epilogue.
int launch_wx(const WxPlan &p, const float *W, const float *X, float *Cm, const float *bias, const float *R, hipStream_t st) {
    if (p.kernel == WxPlan::none) return refused(p.why);
    if (p.kernel == WxPlan::bf16x3) return launch_wx_bf16x3(W, X, bias, R, Cm, p.N, p.M, p.K, p.TV, p.transposed, st);
    if (R && R != Cm)
        STGCN_HIP_CHECK(hipMemcpyAsync(Cm, R, (size_t)p.N * p.M * p.TV * sizeof(float), hipMemcpyDeviceToDevice, st));
    GemmArgs g = wx_gemm(p.M, p.K, p.TV, p.transposed);
    g.A = W; g.B = X; g.C = Cm; g.bias = bias;
    g.accumulate = R ? 1 : 0;
    return launch_gemm_f32(g, p.N, st);
}

// dW = sum_n G[n] . X[n]^T  (G[n] (M, TV), X[n] (K, TV)): per-clip f32 products into `part`, summed in clip order
GemmArgs wgrad_gemm(int M, int K, long long TV) {
    GemmArgs g{};
    g.a_sm = TV; g.a_sk = 1; g.a_sb = (long long)M * TV;
    g.b_sk = 1; g.b_sn = TV; g.b_sb = (long long)K * TV;
    g.c_sm = K; g.c_sn = 1; g.c_sb = (long long)M * K;
    g.M = M; g.N = K; g.K = (int)TV;
    g.alpha = 1.f;
    return g;
}
bool wgrad_covers(int M, int K, long long TV, int N) {
    return TV <= 0x7fffffffLL && gemm_f32_spans_fit(wgrad_gemm(M, K, TV)) && gemm_f32_grid_fits(wgrad_gemm(M, K, TV), N) &&
           sum_parts_covers(N, (size_t)M * K);
}
int gemm_wgrad(const float *G, const float *X, float *part, float *dW, int M, int K, long long TV, int N, hipStream_t st) {
    GemmArgs g = wgrad_gemm(M, K, TV);
    g.A = G; g.B = X; g.C = part;
    int rc = launch_gemm_f32(g, N, st);
    if (rc) return rc;
    return launch_sum_parts(part, dW, N, (size_t)M * K, st);
}

bool bias_grad_covers(int M, long long TV, int N) { return row_sum_covers((long long)N * M, TV) && sum_parts_covers(N, (size_t)M); }
int bias_grad(const float *G, float *part, float *db, int M, long long TV, int N, hipStream_t st) {
    int rc = launch_row_sum(G, part, N * M, (int)TV, st);
    if (rc) return rc;
    return launch_sum_parts(part, db, N, (size_t)M, st);
}

// ----------------------------------------------------------------------------------------------------------------------
// The plan of one call of the unit.  Every entry point and every query reads it: whether the pass is covered (else the
// status and text of the refusal), the head widths, the plan of each W . X product of the pass, and the workspace.
// ----------------------------------------------------------------------------------------------------------------------
enum { kEval = 0, kTrain = 1, kBackward = 2 };      // `pass` of stgcn_st_attention_ws_bytes
const char *const kEntry[3] = {"st_attention_forward", "st_attention_forward_train", "st_attention_backward"};

struct FwdWs {      // eval / training forward (the latter writes qkv and o to the caller's save_* tensors)
    float *xn, *qkv, *o, *dscale, *dshift, *bscale, *bshift;
    double *parts, *sums;
};
struct BwdWs {
    float *xn, *dz, *dout, *dqkv, *dxn, *part, *coef, *bscale, *bshift, *dcoef;
    double *sums, *parts;
};

struct StAttentionPlan {
    bool covered = false;
    Refusal why;
    int pass = 0, N = 0, Cin = 0, Cout = 0, dk = 0, T = 0, V = 0, H = 0;
    int dkh = 0, dvh = 0, Cq = 0, CV = 0;      // per-head widths, rows of Wqkv, channels of data_bn
    size_t TV = 0;
    bool frozen = false;
    // forward passes: qkv = Wqkv . xn and z = Wout . o (+ x);  backward: d(xn) = Wqkv^T . dqkv and d(o) = Wout^T . dz
    WxPlan qkv, out;
    size_t ws_bytes = 0;                       // 0: a non-positive dimension or no such pass; else the pass's, covered or not

    size_t act(int C) const { return (size_t)N * C * TV; }
    // the workspace, carved in 256-byte aligned pieces (base NULL: sizes it)
    FwdWs fwd_ws(void *base, size_t *bytes = nullptr) const {
        Carve c(base);
        FwdWs w;
        const bool train = pass == kTrain;
        w.xn = c.take<float>(act(Cin));
        w.qkv = train ? nullptr : c.take<float>(act(Cq));
        w.o = train ? nullptr : c.take<float>(act(Cout));
        w.dscale = c.take<float>(CV);
        w.dshift = c.take<float>(CV);
        w.bscale = c.take<float>(Cout);
        w.bshift = c.take<float>(Cout);
        w.parts = c.take<double>((size_t)cv_splits(N) * 2 * CV);
        w.sums = c.take<double>((size_t)2 * (CV > Cout ? CV : Cout));
        if (bytes) *bytes = c.off;
        return w;
    }
    BwdWs bwd_ws(void *base, size_t *bytes = nullptr) const {
        Carve c(base);
        BwdWs w;
        w.xn = c.take<float>(act(Cin));
        w.dz = c.take<float>(act(Cout));
        w.dout = c.take<float>(act(Cout));
        w.dqkv = c.take<float>(act(Cq));
        w.dxn = c.take<float>(act(Cin));
        const size_t wparts = (size_t)N * ((size_t)Cout * Cout > (size_t)Cq * Cin ? (size_t)Cout * Cout : (size_t)Cq * Cin);
        w.part = c.take<float>(wparts);
        w.coef = c.take<float>((size_t)3 * Cout);
        w.bscale = c.take<float>(Cout);
        w.bshift = c.take<float>(Cout);
        w.dcoef = c.take<float>((size_t)3 * CV);
        w.sums = c.take<double>((size_t)3 * (CV > Cout ? CV : Cout));
        w.parts = c.take<double>((size_t)cv_splits(N) * 2 * CV);
        if (bytes) *bytes = c.off;
        return w;
    }
};

StAttentionPlan plan_st_attention(int pass, int N, int Cin, int Cout, int dk, int T, int V, int H, unsigned flags) {
    StAttentionPlan p;
    p.pass = pass, p.N = N, p.Cin = Cin, p.Cout = Cout, p.dk = dk, p.T = T, p.V = V, p.H = H;
    p.frozen = (flags & STGCN_BN_FROZEN) != 0;
    const char *fn = kEntry[pass >= kEval && pass <= kBackward ? pass : kEval];
    if (pass < kEval || pass > kBackward || N < 1 || Cin < 1 || Cout < 1 || dk < 1 || T < 1 || V < 1 || H < 1)
        return say(p.why, STGCN_ERR_ARG, "%s: non-positive dimension (N=%d Cin=%d Cout=%d dk=%d T=%d V=%d heads=%d)", fn, N, Cin,
                   Cout, dk, T, V, H), p;
    p.dkh = dk / H, p.dvh = Cout / H, p.Cq = 2 * dk + Cout, p.CV = Cin * V, p.TV = (size_t)T * V;
    if (pass == kBackward) p.bwd_ws(nullptr, &p.ws_bytes);
    else p.fwd_ws(nullptr, &p.ws_bytes);
    // the V x V part
    if (dk % H || Cout % H || !sta_widths_covered(p.dkh, p.dvh))
        return say(p.why, STGCN_ERR_UNSUPPORTED, "%s: Cout=%d dk=%d heads=%d give per-head widths (%d, %d); covered: (4,16), (8,32), "
                   "(16,64)", fn, Cout, dk, H, p.dkh, p.dvh), p;
    if (V > kVP) return say(p.why, STGCN_ERR_UNSUPPORTED, "%s: V=%d joints; the attention kernels cover V <= %d", fn, V, kVP), p;
    if (!sta_covers(N, T, V, H))
        return say(p.why, STGCN_ERR_UNSUPPORTED, "%s: N*T=%lld frames of %d heads exceed the grid", fn, (long long)N * T, H), p;
    // data_bn's launches have a grid row per (clip, input channel); the unit has always held Cout to the same bound
    if (!cv_covers(N, Cin > Cout ? Cin : Cout, T, V) || !bn_rows_fit(N, Cout))
        return say(p.why, STGCN_ERR_UNSUPPORTED, "%s: N=%d clips of %d channels and %zu pixels exceed the grid", fn, N,
                   Cin > Cout ? Cin : Cout, p.TV), p;
    // the products, in the arithmetic of `flags`
    const long long TV = (long long)p.TV;
    const bool back = pass == kBackward;
    p.qkv = back ? plan_wx(fn, Cin, p.Cq, TV, N, true, flags, false) : plan_wx(fn, p.Cq, Cin, TV, N, false, flags, false);
    p.out = plan_wx(fn, Cout, Cout, TV, N, back, flags, false);
    for (const WxPlan *x : {&p.qkv, &p.out})
        if (x->kernel == WxPlan::none) return p.why = x->why, p;
    // the weight and bias gradients stay on the f32 GEMM and the row sums
    if (back && !(wgrad_covers(Cout, Cout, TV, N) && wgrad_covers(p.Cq, Cin, TV, N) && bias_grad_covers(Cout, TV, N) &&
                  bias_grad_covers(p.Cq, TV, N)))
        return say(p.why, STGCN_ERR_UNSUPPORTED, "%s: N=%d Cin=%d Cout=%d TV=%lld exceed the grid or 2^31 elements a clip of the "
                   "weight gradients", fn, N, Cin, Cout, TV), p;
    p.covered = true;
    return p;
}

// what (Cin, Cout, dk, V, heads) and the arithmetic decide without N and T: every pass of one clip of one frame
bool unit_covered(int Cin, int Cout, int dk, int V, int heads, unsigned flags) {
    for (int pass = kEval; pass <= kBackward; ++pass)
        if (!plan_st_attention(pass, 1, Cin, Cout, dk, 1, V, heads, flags & STGCN_MATH_MASK).covered) return false;
    return true;
}

// BatchNorm2d + ReLU of both forward passes' tail
int bn_relu(const StAttentionPlan &p, const float *z, const float *scale, const float *shift, float *y, hipStream_t st) {
    return launch_bn_apply(z, scale, shift, nullptr, nullptr, nullptr, y, p.act(p.Cout), p.Cout, p.TV, st);
}

}  // namespace

}  // namespace stgcn

using namespace stgcn;

extern "C" {

int stgcn_st_attention_supported(int Cin, int Cout, int dk, int V, int heads) {
    return unit_covered(Cin, Cout, dk, V, heads, STGCN_MATH_F32) ? 1 : 0;
}

int stgcn_st_attention_math_supported(int Cin, int Cout, int dk, int V, int heads, unsigned flags) {
    return unit_covered(Cin, Cout, dk, V, heads, flags) ? 1 : 0;
}

size_t stgcn_st_attention_ws_bytes(int N, int Cin, int Cout, int dk, int T, int V, int heads, int pass) {
    return plan_st_attention(pass, N, Cin, Cout, dk, T, V, heads, STGCN_MATH_F32).ws_bytes;     // (the same in both arithmetics)
}

int stgcn_wx_product_supported(int M, int K, long long TV, unsigned flags) {
    return plan_wx("wx_product", M, K, TV, 1, false, flags, true).kernel != WxPlan::none ? 1 : 0;
}

const char *stgcn_wx_product_kernel_name(int M, int K, long long TV, unsigned flags) {
    const WxPlan p = plan_wx("wx_product", M, K, TV, 1, false, flags, true);
    return p.kernel == WxPlan::bf16x3 ? wx_bf16x3_kernel_name(M) : p.kernel == WxPlan::gemm_f32 ? "gemm_f32_kernel" : "";
}

size_t stgcn_wx_product_ws_bytes(int M, int K, unsigned flags) {
    (void)M; (void)K; (void)flags;
    return 0;        // both kernels of plan_wx split or read their operands in place
}

int stgcn_wx_product(const float *W, const float *X, const float *bias, const float *R, float *C, void *ws, size_t ws_bytes,
                     int N, int M, int K, long long TV, int w_transposed, unsigned flags, void *stream) {
    REQUIRE_PTR(W); REQUIRE_PTR(X); REQUIRE_PTR(C);
    (void)ws; (void)ws_bytes;
    if (R == C) return fail(STGCN_ERR_ARG, "wx_product: R may not be C");
    const WxPlan p = plan_wx("wx_product", M, K, TV, N, w_transposed != 0, flags, true);
    if (p.kernel == WxPlan::none) return refused(p.why);
    return launch_wx(p, W, X, C, bias, R, (hipStream_t)stream);
}

int stgcn_st_attention_forward_math(const float *x, const float *dbn_scale, const float *dbn_shift, const float *Wqkv,
                                    const float *bqkv, const float *Wout, const float *bout, const float *bn_scale,
                                    const float *bn_shift, void *ws, size_t ws_bytes, float *y, int N, int Cin, int Cout,
                                    int dk, int T, int V, int heads, unsigned flags, void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(dbn_scale); REQUIRE_PTR(dbn_shift); REQUIRE_PTR(Wqkv); REQUIRE_PTR(bqkv);
    REQUIRE_PTR(Wout); REQUIRE_PTR(bout); REQUIRE_PTR(bn_scale); REQUIRE_PTR(bn_shift); REQUIRE_PTR(ws); REQUIRE_PTR(y);
    REQUIRE_ALIGNED(ws, kBlobAlign);
    const StAttentionPlan p = plan_st_attention(kEval, N, Cin, Cout, dk, T, V, heads, flags);
    if (!p.covered) return refused(p.why);
    if (ws_bytes < p.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "st_attention_forward: workspace %zu < %zu bytes", ws_bytes, p.ws_bytes);
    const FwdWs w = p.fwd_ws(ws);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = launch_cv_apply(x, dbn_scale, dbn_shift, w.xn, N, Cin, T, V, st))) return rc;
    if ((rc = launch_wx(p.qkv, Wqkv, w.xn, w.qkv, bqkv, nullptr, st))) return rc;
    if ((rc = launch_sta_fwd(w.qkv, nullptr, w.o, nullptr, N, T, V, heads, p.dkh, p.dvh, st))) return rc;
    if ((rc = launch_wx(p.out, Wout, w.o, y, bout, Cin == Cout ? x : nullptr, st))) return rc;
    return bn_relu(p, y, bn_scale, bn_shift, y, st);
}

int stgcn_st_attention_forward(const float *x, const float *dbn_scale, const float *dbn_shift, const float *Wqkv,
                               const float *bqkv, const float *Wout, const float *bout, const float *bn_scale,
                               const float *bn_shift, void *ws, size_t ws_bytes, float *y, int N, int Cin, int Cout,
                               int dk, int T, int V, int heads, void *stream) {
    return stgcn_st_attention_forward_math(x, dbn_scale, dbn_shift, Wqkv, bqkv, Wout, bout, bn_scale, bn_shift, ws, ws_bytes, y,
                                           N, Cin, Cout, dk, T, V, heads, STGCN_MATH_F32, stream);
}

int stgcn_st_attention_forward_train(const float *x, const float *dbn_weight, const float *dbn_bias, float *dbn_running_mean,
                                     float *dbn_running_var, const float *Wqkv, const float *bqkv, const float *Wout,
                                     const float *bout, const float *bn_weight, const float *bn_bias,
                                     float *bn_running_mean, float *bn_running_var, const float *mask, float momentum,
                                     float eps, void *ws, size_t ws_bytes, float *y, float *save_qkv, float *save_o,
                                     float *save_z, float *save_rowstats, float *save_stats, int N, int Cin, int Cout,
                                     int dk, int T, int V, int heads, unsigned flags, void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(dbn_weight); REQUIRE_PTR(dbn_bias); REQUIRE_PTR(dbn_running_mean);
    REQUIRE_PTR(dbn_running_var); REQUIRE_PTR(Wqkv); REQUIRE_PTR(bqkv); REQUIRE_PTR(Wout); REQUIRE_PTR(bout);
    REQUIRE_PTR(bn_weight); REQUIRE_PTR(bn_bias); REQUIRE_PTR(bn_running_mean); REQUIRE_PTR(bn_running_var);
    REQUIRE_PTR(ws); REQUIRE_PTR(y); REQUIRE_PTR(save_qkv); REQUIRE_PTR(save_o); REQUIRE_PTR(save_z);
    REQUIRE_PTR(save_rowstats); REQUIRE_PTR(save_stats);
    REQUIRE_ALIGNED(ws, kBlobAlign);     // fp64 atomic sums
    const StAttentionPlan p = plan_st_attention(kTrain, N, Cin, Cout, dk, T, V, heads, flags);
    if (!p.covered) return refused(p.why);      // before the first launch: nothing is written, the running statistics included
    if (ws_bytes < p.ws_bytes)
        return fail(STGCN_ERR_WORKSPACE, "st_attention_forward_train: workspace %zu < %zu bytes", ws_bytes, p.ws_bytes);
    const FwdWs w = p.fwd_ws(ws);
    hipStream_t st = (hipStream_t)stream;
    float *dmean = save_stats, *dinv = save_stats + p.CV, *bmean = save_stats + 2 * p.CV, *binv = bmean + Cout;
    int rc;
    // data_bn
    if (p.frozen) {
        rc = launch_bn_frozen_finalize(dbn_weight, dbn_bias, dbn_running_mean, dbn_running_var, eps, w.dscale, w.dshift, p.CV,
                                       st, dmean, dinv);
    } else {
        if ((rc = launch_cv_stats(x, nullptr, nullptr, nullptr, w.parts, w.sums, N, Cin, T, V, st))) return rc;
        rc = launch_bn_train_finalize(w.sums, (double)N * T, dbn_weight, dbn_bias, dbn_running_mean, dbn_running_var, momentum,
                                      eps, w.dscale, w.dshift, p.CV, st, dmean, dinv);
    }
    if (rc) return rc;
    if ((rc = launch_cv_apply(x, w.dscale, w.dshift, w.xn, N, Cin, T, V, st))) return rc;
    // attention
    if ((rc = launch_wx(p.qkv, Wqkv, w.xn, save_qkv, bqkv, nullptr, st))) return rc;
    if ((rc = launch_sta_fwd(save_qkv, mask, save_o, save_rowstats, N, T, V, heads, p.dkh, p.dvh, st))) return rc;
    if ((rc = launch_wx(p.out, Wout, save_o, save_z, bout, Cin == Cout ? x : nullptr, st))) return rc;
    // BatchNorm2d + ReLU
    if (p.frozen) {
        rc = launch_bn_frozen_finalize(bn_weight, bn_bias, bn_running_mean, bn_running_var, eps, w.bscale, w.bshift, Cout, st,
                                       bmean, binv);
    } else {
        if ((rc = launch_bn_batch_stats(save_z, w.sums, N, Cout, p.TV, st))) return rc;
        rc = launch_bn_train_finalize(w.sums, (double)N * p.TV, bn_weight, bn_bias, bn_running_mean, bn_running_var, momentum,
                                      eps, w.bscale, w.bshift, Cout, st, bmean, binv);
    }
    if (rc) return rc;
    return bn_relu(p, save_z, w.bscale, w.bshift, y, st);
}

int stgcn_st_attention_backward(const float *x, const float *dbn_weight, const float *dbn_bias, const float *Wqkv,
                                const float *Wout, const float *bn_weight, const float *bn_bias, const float *mask,
                                const float *save_qkv, const float *save_o, const float *save_z, const float *save_rowstats,
                                const float *save_stats, const float *dy, float *dx, float *ddbn_weight, float *ddbn_bias,
                                float *dWqkv, float *dbqkv, float *dWout, float *dbout, float *dbn_weight_grad,
                                float *dbn_bias_grad, void *ws, size_t ws_bytes, int N, int Cin, int Cout, int dk, int T,
                                int V, int heads, unsigned flags, void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(dbn_weight); REQUIRE_PTR(dbn_bias); REQUIRE_PTR(Wqkv); REQUIRE_PTR(Wout);
    REQUIRE_PTR(bn_weight); REQUIRE_PTR(bn_bias); REQUIRE_PTR(save_qkv); REQUIRE_PTR(save_o); REQUIRE_PTR(save_z);
    REQUIRE_PTR(save_rowstats); REQUIRE_PTR(save_stats); REQUIRE_PTR(dy); REQUIRE_PTR(ddbn_weight); REQUIRE_PTR(ddbn_bias);
    REQUIRE_PTR(dWqkv); REQUIRE_PTR(dbqkv); REQUIRE_PTR(dWout); REQUIRE_PTR(dbout); REQUIRE_PTR(dbn_weight_grad);
    REQUIRE_PTR(dbn_bias_grad); REQUIRE_PTR(ws);
    REQUIRE_ALIGNED(ws, kBlobAlign);
    const StAttentionPlan p = plan_st_attention(kBackward, N, Cin, Cout, dk, T, V, heads, flags);
    if (!p.covered) return refused(p.why);
    if (ws_bytes < p.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "st_attention_backward: workspace %zu < %zu bytes", ws_bytes, p.ws_bytes);
    const BwdWs w = p.bwd_ws(ws);
    hipStream_t st = (hipStream_t)stream;
    const float *dmean = save_stats, *dinv = save_stats + p.CV, *bmean = save_stats + 2 * p.CV, *binv = bmean + Cout;
    int rc;
    // BatchNorm2d + ReLU -> dz
    if ((rc = launch_bn_scale_shift(bn_weight, bn_bias, bmean, binv, w.bscale, w.bshift, Cout, st))) return rc;
    if ((rc = launch_bn_relu_bwd_stats(save_z, w.bscale, w.bshift, bmean, binv, nullptr, nullptr, nullptr, nullptr, nullptr, dy,
                                       w.sums, N, Cout, p.TV, st))) return rc;
    if ((rc = launch_bn_bwd_finalize(w.sums, 1, (double)N * p.TV, bn_weight, binv, dbn_weight_grad, dbn_bias_grad, w.coef, Cout,
                                     st, p.frozen))) return rc;
    if ((rc = launch_bn_relu_bwd_apply(save_z, w.bscale, w.bshift, bmean, binv, nullptr, nullptr, nullptr, nullptr, nullptr, dy,
                                       w.coef, nullptr, w.dz, nullptr, nullptr, N, Cout, p.TV, st))) return rc;
    // output projection
    if ((rc = gemm_wgrad(w.dz, save_o, w.part, dWout, Cout, Cout, p.TV, N, st))) return rc;
    if ((rc = bias_grad(w.dz, w.part, dbout, Cout, p.TV, N, st))) return rc;
    if ((rc = launch_wx(p.out, Wout, w.dz, w.dout, nullptr, nullptr, st))) return rc;
    // attention
    if ((rc = launch_sta_bwd(save_qkv, w.dout, mask, save_rowstats, w.dqkv, N, T, V, heads, p.dkh, p.dvh, st))) return rc;
    // qkv projection (on data_bn's output, rebuilt from x and the saved statistics)
    if ((rc = launch_bn_scale_shift(dbn_weight, dbn_bias, dmean, dinv, w.dcoef, w.dcoef + p.CV, p.CV, st))) return rc;
    if ((rc = launch_cv_apply(x, w.dcoef, w.dcoef + p.CV, w.xn, N, Cin, T, V, st))) return rc;
    if ((rc = gemm_wgrad(w.dqkv, w.xn, w.part, dWqkv, p.Cq, Cin, p.TV, N, st))) return rc;
    if ((rc = bias_grad(w.dqkv, w.part, dbqkv, p.Cq, p.TV, N, st))) return rc;
    if ((rc = launch_wx(p.qkv, Wqkv, w.dqkv, w.dxn, nullptr, nullptr, st))) return rc;
    // data_bn backward: its parameter gradients need d(xn) whether or not x wants a gradient ...
    if ((rc = launch_cv_stats(x, w.dxn, dmean, dinv, w.parts, w.sums, N, Cin, T, V, st))) return rc;
    if ((rc = launch_bn_bwd_finalize(w.sums, 1, (double)N * T, dbn_weight, dinv, ddbn_weight, ddbn_bias, w.dcoef, p.CV, st,
                                     p.frozen))) return rc;
    if (dx == nullptr) return STGCN_OK;
    // ... dx (+ the skip connection's dz)
    return launch_cv_bwd_apply(w.dxn, x, dmean, dinv, w.dcoef, Cin == Cout ? w.dz : nullptr, dx, N, Cin, T, V, st);
}

}  // extern "C"
