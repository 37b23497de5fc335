// Training mode of unit_agcn: the plans and launch sequences of its forward and backward entry points (bottom of the file),
// and the forward WITHOUT materialising its two pre-BatchNorm branches (stem shape class:
// C_in = 3, 3 subsets, down branch).
//
// Both branches are linear in a handful of per-pixel features,
//     zm[o] = sum_f Wm[o][f] * u[f] + bm[o]     (u = the 9 aggregated values x P_s,  Wm = [Wd_0|Wd_1|Wd_2],  bm = sum_s bd_s)
//     zd[o] = sum_k Wdown[o][k] * x[k] + bdown[o]
// so the batch statistics nn.BatchNorm2d takes over (N,T,V) (model/unit_agcn.py:91-92, 54-55 with self.training)
// follow from the first and second moments of u (9 + 45 numbers) and x (3 + 6):
//     E[zm[o]] = Wm[o].E[u] + bm[o],    E[zm[o]^2] = Wm[o]^T E[u u^T] Wm[o] + 2 bm[o] Wm[o].E[u] + bm[o]^2 .
// One pass over x and P accumulates the 63 moments (fp32 within a clip, fp64 across clips), a one-workgroup kernel turns
// them into every channel's (scale, shift), saved mean / invstd and running-buffer update, and the eval-mode expansion
// kernel then writes the module output directly.  Against the materialising path this drops two full-size tensors
// (2 x 4*C*T*V bytes per clip written, read twice) and three elementwise passes.
#include <algorithm>

#include "common.h"

namespace stgcn {

namespace {

constexpr int NMOM = 9 + 45 + 3 + 6;   // u, uu^T (upper triangle), x, xx^T (upper triangle)
constexpr int MOM_NT = 1024;           // threads of the moments kernel: four waves per SIMD hide the LDS latency of the u loop
                                       // (with 256 threads — one wave per SIMD — the same code took 73 us for 256 clips)

template <int CIN, int S>
__global__ __launch_bounds__(MOM_NT) void agcn_moments_kernel(const float *__restrict__ x, const float *__restrict__ P,
                                                           double *__restrict__ part /* [grid][NMOM] */, int N, int T,
                                                           int V, int TF) {
    constexpr int SC = S * CIN;
    static_assert(SC == 9 && CIN == 3, "moment layout is written for 3 channels x 3 subsets");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *Ps = sm;                    // [S][V][V]
    float *Xs = Ps + S * V * V;        // [CIN][TF*V]
    __shared__ float red[MOM_NT / 64][NMOM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int PXM = TF * V;
    double total = 0.0;                // thread tid < NMOM: moment `tid` summed over this workgroup's clips
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        __syncthreads();
        const float *Pn = P + (size_t)n * S * V * V;
        for (int e = tid; e < S * V * V; e += MOM_NT) Ps[e] = Pn[e];
        const float *xn = x + (size_t)n * CIN * T * V;
        float m[NMOM];
#pragma unroll
        for (int i = 0; i < NMOM; ++i) m[i] = 0.f;
        for (int t0 = 0; t0 < T; t0 += TF) {
            const int px = min(TF, T - t0) * V;
            __syncthreads();
            for (int e = tid; e < CIN * px; e += MOM_NT) {
                const int k = e / px, p = e - k * px;
                Xs[k * PXM + p] = xn[((size_t)k * T + t0) * V + p];
            }
            __syncthreads();
            for (int p = tid; p < px; p += MOM_NT) {
                const int tt = p / V, w = p - tt * V;
                float u[SC];
#pragma unroll
                for (int f = 0; f < SC; ++f) u[f] = 0.f;
                for (int v = 0; v < V; ++v) {   // same order of operations as agcn_expand_small_kernel
                    float xv[CIN];
#pragma unroll
                    for (int k = 0; k < CIN; ++k) xv[k] = Xs[k * PXM + tt * V + v];
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const float pv = Ps[(s * V + v) * V + w];
#pragma unroll
                        for (int k = 0; k < CIN; ++k) u[s * CIN + k] = fmaf(xv[k], pv, u[s * CIN + k]);
                    }
                }
#pragma unroll
                for (int i = 0; i < SC; ++i) m[i] += u[i];
#pragma unroll
                for (int i = 0; i < SC; ++i)
#pragma unroll
                    for (int j = i; j < SC; ++j) {
                        const int q = SC + i * SC - i * (i - 1) / 2 + (j - i);      // upper triangle, row-major
                        m[q] = fmaf(u[i], u[j], m[q]);
                    }
                float xp[CIN];
#pragma unroll
                for (int k = 0; k < CIN; ++k) xp[k] = Xs[k * PXM + p];
#pragma unroll
                for (int i = 0; i < CIN; ++i) m[SC + 45 + i] += xp[i];
#pragma unroll
                for (int i = 0; i < CIN; ++i)
#pragma unroll
                    for (int j = i; j < CIN; ++j) {
                        const int q = SC + 45 + CIN + i * CIN - i * (i - 1) / 2 + (j - i);
                        m[q] = fmaf(xp[i], xp[j], m[q]);
                    }
            }
        }
        // block reduction of the clip's 63 moments
#pragma unroll
        for (int i = 0; i < NMOM; ++i) {
            float v = m[i];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) red[wave][i] = v;
        }
        __syncthreads();
        if (tid < NMOM) {                  // fixed order
            double c = 0.0;
#pragma unroll
            for (int w8 = 0; w8 < MOM_NT / 64; ++w8) c += (double)red[w8][tid];
            total += c;
        }
    }
    if (tid < NMOM) part[(size_t)blockIdx.x * NMOM + tid] = total;
}

// moments -> per-channel batch statistics of both BatchNorms -> (scale, shift), saved mean/invstd, running buffers
template <int CIN, int S>
__global__ __launch_bounds__(1024) void agcn_moments_finalize_kernel(
    const double *__restrict__ part, int parts, double count, const float *__restrict__ Wd, const float *__restrict__ bd,
    const float *__restrict__ Wdown, const float *__restrict__ bdown, const float *__restrict__ bn_w,
    const float *__restrict__ bn_b, float *__restrict__ bn_rm, float *__restrict__ bn_rv, const float *__restrict__ dbn_w,
    const float *__restrict__ dbn_b, float *__restrict__ dbn_rm, float *__restrict__ dbn_rv, float momentum, float eps,
    float *__restrict__ s_m, float *__restrict__ t_m, float *__restrict__ s_d, float *__restrict__ t_d,
    float *__restrict__ save_stats /* 4*Cout + 128 floats, or NULL */, int Cout) {
    constexpr int SC = S * CIN;
    __shared__ double mom[NMOM];
    __shared__ double sub[16][64];
    const int tid = threadIdx.x;
    {   // 16 groups of partials per moment (16 waves: the loads of a group are a chain of round trips), then a
        // fixed-order sum of the 16 sub-sums
        const int i = tid & 63, grp = tid >> 6;
        double s = 0.0;
        if (i < NMOM)
            for (int p = grp; p < parts; p += 16) s += part[(size_t)p * NMOM + i];
        sub[grp][i] = s;
    }
    __syncthreads();
    if (tid < NMOM) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += sub[g][tid];
        mom[tid] = s / count;
        // the backward's moment form (agcn_backward.hip) reads the feature moments back: 63 doubles behind the 4*Cout floats
        if (save_stats) reinterpret_cast<double *>(save_stats + 4 * Cout)[tid] = mom[tid];
        if (save_stats && tid == 0)   // validity mark for the moment-form backward (it used to trust the caller)
            reinterpret_cast<unsigned *>(save_stats)[STGCN_MOMENTS_MARK_SLOT(Cout)] = STGCN_MOMENTS_MAGIC;
    }
    __syncthreads();
    const double *mu = mom, *muu = mom + SC, *mx = mom + SC + 45, *mxx = mom + SC + 45 + CIN;
    for (int o = tid; o < Cout; o += 1024) {
        double w[SC], b = 0.0;
        for (int s = 0; s < S; ++s) {
            b += (double)bd[s * Cout + o];
            for (int k = 0; k < CIN; ++k) w[s * CIN + k] = (double)Wd[((size_t)s * Cout + o) * CIN + k];
        }
        double lin = 0.0, quad = 0.0;
        int q = 0;
        for (int i = 0; i < SC; ++i) lin += w[i] * mu[i];
        for (int i = 0; i < SC; ++i)
            for (int j = i; j < SC; ++j, ++q) quad += (i == j ? 1.0 : 2.0) * w[i] * w[j] * muu[q];
        const double mean_m = lin + b;
        double var_m = quad + 2.0 * b * lin + b * b - mean_m * mean_m;
        double wd[CIN];
        for (int k = 0; k < CIN; ++k) wd[k] = (double)Wdown[o * CIN + k];
        const double bdn = (double)bdown[o];
        double lind = 0.0, quadd = 0.0;
        q = 0;
        for (int i = 0; i < CIN; ++i) lind += wd[i] * mx[i];
        for (int i = 0; i < CIN; ++i)
            for (int j = i; j < CIN; ++j, ++q) quadd += (i == j ? 1.0 : 2.0) * wd[i] * wd[j] * mxx[q];
        const double mean_d = lind + bdn;
        double var_d = quadd + 2.0 * bdn * lind + bdn * bdn - mean_d * mean_d;
        if (var_m < 0.0) var_m = 0.0;
        if (var_d < 0.0) var_d = 0.0;
        const double unb = count > 1.0 ? count / (count - 1.0) : 1.0;
        {
            const float inv = 1.f / sqrtf((float)var_m + eps), s = bn_w[o] * inv;
            s_m[o] = s;
            t_m[o] = bn_b[o] - (float)mean_m * s;
            if (save_stats) { save_stats[o] = (float)mean_m; save_stats[Cout + o] = inv; }
            bn_rm[o] = (1.f - momentum) * bn_rm[o] + momentum * (float)mean_m;
            bn_rv[o] = (1.f - momentum) * bn_rv[o] + momentum * (float)(var_m * unb);
        }
        {
            const float inv = 1.f / sqrtf((float)var_d + eps), s = dbn_w[o] * inv;
            s_d[o] = s;
            t_d[o] = dbn_b[o] - (float)mean_d * s;
            if (save_stats) { save_stats[2 * Cout + o] = (float)mean_d; save_stats[3 * Cout + o] = inv; }
            dbn_rm[o] = (1.f - momentum) * dbn_rm[o] + momentum * (float)mean_d;
            dbn_rv[o] = (1.f - momentum) * dbn_rv[o] + momentum * (float)(var_d * unb);
        }
    }
}

inline int moments_grid(int N) { return N < 256 ? N : 256; }

}  // namespace

static bool agcn_moments_supported(int Cin, int V, int S) {
    return agcn_stem_class(Cin, S) && ((size_t)S * V * V + (size_t)Cin * (MOM_NT / V > 0 ? MOM_NT / V : 1) * V) * 4 <= (size_t)kLdsBytes && V <= MOM_NT;
}

// part: moments_grid(N) * NMOM doubles of scratch.  Writes s_m, t_m, s_d, t_d (Cout each) and updates the running buffers.
static int launch_agcn_moments(const float *x, const float *P, double *part, const float *Wd, const float *bd, const float *Wdown,
                        const float *bdown, const float *bn_w, const float *bn_b, float *bn_rm, float *bn_rv,
                        const float *dbn_w, const float *dbn_b, float *dbn_rm, float *dbn_rv, float momentum, float eps,
                        float *s_m, float *t_m, float *s_d, float *t_d, float *save_stats, int N, int Cin, int Cout, int T,
                        int V, int S, hipStream_t st) {
    if (!agcn_moments_supported(Cin, V, S))
        return fail(STGCN_ERR_UNSUPPORTED, "agcn moments: covers Cin=3, 3 subsets (got %d, %d, V=%d)", Cin, S, V);
    int TF = MOM_NT / V;
    if (TF < 1) TF = 1;
    if (TF > T) TF = T;
    const size_t lds = ((size_t)S * V * V + (size_t)Cin * TF * V) * 4;
    const int grid = moments_grid(N);
    STGCN_HIP_CHECK(allow_lds((agcn_moments_kernel<3, 3>), lds));
    hipLaunchKernelGGL((agcn_moments_kernel<3, 3>), dim3(grid), dim3(MOM_NT), lds, st, x, P, part, N, T, V, TF);
    STGCN_LAUNCH_CHECK("agcn_moments_kernel");
    hipLaunchKernelGGL((agcn_moments_finalize_kernel<3, 3>), dim3(1), dim3(1024), 0, st, part, grid, (double)N * T * V, Wd, bd,
                       Wdown, bdown, bn_w, bn_b, bn_rm, bn_rv, dbn_w, dbn_b, dbn_rm, dbn_rv, momentum, eps, s_m, t_m, s_d, t_d,
                       save_stats, Cout);
    STGCN_LAUNCH_CHECK("agcn_moments_finalize_kernel");
    return STGCN_OK;
}

// ---- training forward: plan, workspace, launch sequence ------------------------------------------------------------
namespace {

struct AgcnTrainWs {
    TrainSmall v;
    double *part;        // moments path: the per-workgroup partial moments
    float *zm, *zd;      // materialising path: the two pre-BatchNorm branches
    size_t bytes;
};
AgcnTrainWs carve_agcn_train(void *base, bool moments, int N, int Cout, int T, int V) {
    Carve c(base);
    AgcnTrainWs w{};
    w.v = carve_train_small(c, Cout);
    if (moments) {
        w.part = c.packed<double>((size_t)moments_grid(N) * NMOM);
    } else {
        w.zm = c.packed<float>((size_t)N * Cout * T * V);
        w.zd = c.packed<float>((size_t)N * Cout * T * V);
    }
    w.bytes = c.off;
    return w;
}

}  // namespace

AgcnTrainPlan plan_agcn_train(int N, int Cin, int Cout, int T, int V, int S, bool materialise, bool has_down, bool frozen) {
    AgcnTrainPlan p;
    p.frozen = frozen;
    p.has_down = has_down;
    p.moments = !materialise && agcn_moments_supported(Cin, V, S);
    // Outside Cin = 3 the residual rows are left out of the main branch's contraction altogether (no Wdown: "identity" with
    // EXPAND_NO_RESIDUAL) and conv_down runs as one plain product — the expansion kernel run a second time with the main scales
    // at zero did the whole work of both branches again (2 x 208 us at 64 -> 128 channels, 64 clips).  This is NOT "no folded
    // expansion kernel serves the shape" (!expand_is_folded(p.down.kernel)): Cin = 3 with S != 3, V > 256 or a folded weight image
    // beyond LDS has no folded kernel either and still runs the generic expansion twice; taking the plan's answer there would
    // move the bits of zd, its statistics and y, so the shape test stays.
    p.down_as_gemm = has_down && Cin != 3;
    p.down = plan_agcn_expand(N, Cin, Cout, T, V, S, true);
    p.main = p.down_as_gemm || !has_down ? plan_agcn_expand(N, Cin, Cout, T, V, S, false) : p.down;
    p.ws_bytes = carve_agcn_train(nullptr, p.moments, N, Cout, T, V).bytes;
    return p;
}

// P: the attention matrices of this call (launch_attention).  save_zm / save_zd (optional) receive the branches in place of
// the workspace's; save_stats (4*Cout + 128, optional): batch mean, invstd of the main BatchNorm, then of the down BatchNorm,
// then the feature-moment block.
int launch_agcn_forward_train(const AgcnTrainPlan &p, const float *x, const float *P, const float *Wd, const float *bd,
                              const float *Wdown, const float *bdown, const float *bn_weight, const float *bn_bias,
                              float *bn_running_mean, float *bn_running_var, const float *dbn_weight, const float *dbn_bias,
                              float *dbn_running_mean, float *dbn_running_var, float momentum, float eps, void *ws, float *y,
                              float *save_zm, float *save_zd, float *save_stats, int N, int Cin, int Cout, int T, int V, int S,
                              hipStream_t st) {
    const AgcnTrainWs w = carve_agcn_train(ws, p.moments, N, Cout, T, V);
    float *ones = w.v.ones, *zeros = w.v.zeros, *s1 = w.v.s1, *t1 = w.v.t1, *s2 = w.v.s2, *t2 = w.v.t2;
    int rc;
    if (p.moments) {   // batch statistics from the moments of the 12 per-pixel features; the branches are never written
        if ((rc = launch_agcn_moments(x, P, w.part, Wd, bd, Wdown, bdown, bn_weight, bn_bias, bn_running_mean, bn_running_var,
                                      dbn_weight, dbn_bias, dbn_running_mean, dbn_running_var, momentum, eps, s1, t1, s2, t2,
                                      save_stats, N, Cin, Cout, T, V, S, st)))
            return rc;
        return launch_agcn_expand(p.main, x, P, Wd, bd, Wdown, bdown, s1, t1, s2, t2, y, 0, st);
    }
    float *zm = save_zm ? save_zm : w.zm, *zd = save_zd ? save_zd : w.zd;
    const size_t plane = (size_t)T * V, total = (size_t)N * Cout * plane;
    // (scale, shift) of one BatchNorm over z, from its running statistics (frozen) or from the batch's; sv: its mean and invstd
    auto finalize = [&](const float *z, double *sums, const float *weight, const float *bias, float *rm, float *rv, float *s,
                        float *t, float *sv) {
        float *sv_inv = sv ? sv + Cout : nullptr;
        if (p.frozen) return launch_bn_frozen_finalize(weight, bias, rm, rv, eps, s, t, Cout, st, sv, sv_inv);
        if (int r = launch_bn_batch_stats(z, sums, N, Cout, plane, st)) return r;
        return launch_bn_train_finalize(sums, (double)N * plane, weight, bias, rm, rv, momentum, eps, s, t, Cout, st, sv, sv_inv);
    };
    if (save_stats)   // no feature moments on this path: clear their block incl. the validity mark the moment-form backward checks
        STGCN_HIP_CHECK(hipMemsetAsync(save_stats + 4 * Cout, 0, 128 * sizeof(float), st));
    if ((rc = launch_fill_ones_zeros(ones, zeros, Cout, st))) return rc;
    // main branch, pre-BN: sum_s conv_d_s(x P_s)   (unit scale on the main path, zero on the residual path, no ReLU)
    const bool with_down = p.has_down && !p.down_as_gemm;
    rc = launch_agcn_expand(p.main, x, P, Wd, bd, with_down ? Wdown : nullptr, with_down ? bdown : nullptr, ones, zeros,
                            with_down ? zeros : nullptr, with_down ? zeros : nullptr, zm, EXPAND_RAW | EXPAND_NO_RESIDUAL, st);
    if (rc != STGCN_OK) return rc;
    if ((rc = finalize(zm, w.v.sums1, bn_weight, bn_bias, bn_running_mean, bn_running_var, s1, t1, save_stats))) return rc;
    if (!p.has_down) return launch_bn_apply(zm, s1, t1, x, nullptr, nullptr, y, total, Cout, plane, st);  // identity residual: + x
    if (p.down_as_gemm) {     // residual branch, pre-BN: zd[n] = Wdown x[n] + bdown
        const long long Pl = (long long)plane;
        GemmArgs g{Wdown, x, zd, bdown, Cout, (int)plane, Cin, Cin, 1, 0, Pl, 1, (long long)Cin * Pl, Pl, 1, (long long)Cout * Pl, 1.f, 0};
        rc = launch_gemm_f32(g, N, st);
    } else {
        rc = launch_agcn_expand(p.down, x, P, Wd, bd, Wdown, bdown, zeros, zeros, ones, zeros, zd, EXPAND_RAW, st);
    }
    if (rc != STGCN_OK) return rc;
    if ((rc = finalize(zd, w.v.sums2, dbn_weight, dbn_bias, dbn_running_mean, dbn_running_var, s2, t2,
                       save_stats ? save_stats + 2 * Cout : nullptr)))
        return rc;
    return launch_bn_apply(zm, s1, t1, zd, s2, t2, y, total, Cout, plane, st);
}

// ---- training backward: plan, workspace, launch sequence -------------------------------------------------------------
namespace {

struct AgcnBackwardWs {   // of the generic GEMM chain (the moment form lays out its own: agcn_backward.hip)
    double *sums;
    float *coefm, *coefd, *sm, *tm, *sd, *td, *ones, *zeros;
    float *dzm, *dzd, *chain;   // both pre-BatchNorm gradients, launch_agcn_bwd_generic's scratch
    float *zm, *zd;             // recompute: the rebuilt branches
    size_t bytes;
};
AgcnBackwardWs carve_agcn_backward(void *base, const AgcnBackwardPlan &p, int N, int Cin, int Cout, int T, int V, int S) {
    Carve c(base);
    AgcnBackwardWs w{};
    const size_t C = Cout, total = (size_t)N * Cout * T * V;
    w.sums = c.packed<double>(3 * C);
    w.coefm = c.packed<float>(3 * C); w.coefd = c.packed<float>(3 * C);
    w.sm = c.packed<float>(C); w.tm = c.packed<float>(C); w.sd = c.packed<float>(C); w.td = c.packed<float>(C);
    w.ones = c.packed<float>(C); w.zeros = c.packed<float>(C);
    c.pad();
    w.dzm = c.packed<float>(total); w.dzd = c.packed<float>(total);
    w.chain = c.packed<float>(agcn_bwd_generic_ws_floats(N, Cin, Cout, T, V, p.inter_c_max, S));
    c.pad();
    if (p.recompute) { w.zm = c.packed<float>(total); w.zd = c.packed<float>(total); }
    w.bytes = c.off;
    return w;
}

}  // namespace

// The moment-form backward (agcn_backward.hip) serves the stem's shape class after a moments-path forward when no input
// gradient is wanted; everything else (any Cin / Cout / subsets, identity residual, dx, saved branches) takes the generic
// GEMM chain.  The moment form is the closed form of the BATCH-statistics BatchNorm: frozen statistics take the chain too.
AgcnBackwardPlan plan_agcn_backward(int N, int Cin, int Cout, int T, int V, int S, bool recompute, bool generic, bool has_down,
                                    bool frozen) {
    AgcnBackwardPlan p;
    p.frozen = frozen;
    p.has_down = has_down;
    if (V > kAttentionMaxV) return p;
    const size_t fused_bytes = agcn_bwd_ws_bytes(N, Cin, Cout, T, V, S);      // 0: the moment form does not cover the shape
    p.fused = !generic && fused_bytes != 0;
    p.ws_bytes = fused_bytes;                                                 // the moment form needs neither branch
    if (p.fused) return p;
    p.recompute = recompute;
    if (recompute) p.expand = plan_agcn_expand(N, Cin, Cout, T, V, S, has_down);
    p.inter_c_max = Cout / 4 > 0 ? Cout / 4 : 1;   // upper bound used for sizing: unit_agcn's coff_embedding = 4
    // (a workspace sized for the chain also serves the moment form, should the entry point take that after all)
    p.ws_bytes = std::max(carve_agcn_backward(nullptr, p, N, Cin, Cout, T, V, S).bytes, fused_bytes);
    return p;
}

int launch_agcn_backward_train(const AgcnBackwardPlan &p, const float *x, const float *A_eff, const float *Wa, const float *ba,
                               const float *Wb, const float *bb, const float *Wd, const float *bd, const float *Wdown,
                               const float *bdown, const float *P, const float *zm, const float *zd, const float *bn_weight,
                               const float *bn_bias, const float *dbn_weight, const float *dbn_bias, const float *save_stats,
                               const float *y, const float *dy, float *dWa, float *dba, float *dWb, float *dbb, float *dWd,
                               float *dbd, float *dWdown, float *dbdown, float *dgamma, float *dbeta, float *ddgamma,
                               float *ddbeta, float *dPA, float *dx, void *ws, int N, int Cin, int Cout, int T, int V,
                               int inter_c, int S, hipStream_t st) {
    if (p.fused)
        return launch_agcn_bwd(x, P, A_eff, y, dy, Wa, ba, Wb, bb, Wd, bd, Wdown, bdown, bn_weight, dbn_weight, save_stats, ws,
                               dWa, dba, dWb, dbb, dWd, dbd, dWdown, dbdown, dgamma, dbeta, ddgamma, ddbeta, dPA, N, Cin, Cout,
                               T, V, inter_c, S, st);
    const AgcnBackwardWs w = carve_agcn_backward(ws, p, N, Cin, Cout, T, V, S);
    const bool has_down = p.has_down;
    const size_t plane = (size_t)T * V;
    const double count = (double)N * plane;
    int rc;
    if (p.recompute) {   // the forward kept no branches (moments path): rebuild them with the raw-mode expansion kernel
        if ((rc = launch_fill_ones_zeros(w.ones, w.zeros, Cout, st))) return rc;
        if ((rc = launch_agcn_expand(p.expand, x, P, Wd, bd, Wdown, bdown, w.ones, w.zeros, has_down ? w.zeros : nullptr,
                                     has_down ? w.zeros : nullptr, w.zm, EXPAND_RAW | EXPAND_NO_RESIDUAL, st)))
            return rc;
        zm = w.zm;
        if (has_down) {
            if ((rc = launch_agcn_expand(p.expand, x, P, Wd, bd, Wdown, bdown, w.zeros, w.zeros, w.ones, w.zeros, w.zd, EXPAND_RAW, st)))
                return rc;
            zd = w.zd;
        }
    }
    const float *mean_m = save_stats, *inv_m = save_stats + Cout, *mean_d = save_stats + 2 * Cout, *inv_d = save_stats + 3 * Cout;
    if ((rc = launch_bn_scale_shift(bn_weight, bn_bias, mean_m, inv_m, w.sm, w.tm, Cout, st))) return rc;
    if (has_down && (rc = launch_bn_scale_shift(dbn_weight, dbn_bias, mean_d, inv_d, w.sd, w.td, Cout, st))) return rc;
    // side b of the ReLU's argument: the second BatchNorm, or (scale == NULL) the identity residual x itself
    const float *zb = has_down ? zd : x, *sb = has_down ? w.sd : nullptr, *tb = has_down ? w.td : nullptr;
    const float *mb = has_down ? mean_d : nullptr, *ib = has_down ? inv_d : nullptr;
    if ((rc = launch_bn_relu_bwd_stats(zm, w.sm, w.tm, mean_m, inv_m, zb, sb, tb, mb, ib, dy, w.sums, N, Cout, plane, st))) return rc;
    if ((rc = launch_bn_bwd_finalize(w.sums, 1, count, bn_weight, inv_m, dgamma, dbeta, w.coefm, Cout, st, p.frozen))) return rc;
    if (has_down && (rc = launch_bn_bwd_finalize(w.sums, 2, count, dbn_weight, inv_d, ddgamma, ddbeta, w.coefd, Cout, st, p.frozen)))
        return rc;
    // materialise both pre-BatchNorm gradients, then the GEMM chain
    // (identity residual, unit_agcn.py:57-58,92: dL/dx of the "+ x" term is the masked cotangent itself — written by the same
    //  pass as dx's first term; it was a kernel of its own re-reading zm, x and dy)
    const bool dx_from_g = dx != nullptr && !has_down;
    if ((rc = launch_bn_relu_bwd_apply(zm, w.sm, w.tm, mean_m, inv_m, zb, sb, tb, mb, ib, dy, w.coefm, has_down ? w.coefd : nullptr,
                                       w.dzm, has_down ? w.dzd : nullptr, nullptr, N, Cout, plane, st, dx_from_g ? dx : nullptr)))
        return rc;
    return launch_agcn_bwd_generic(x, P, A_eff, w.dzm, has_down ? w.dzd : nullptr, Wa, ba, Wb, bb, Wd, Wdown, w.chain, dWa, dba,
                                   dWb, dbb, dWd, dbd, dWdown, dbdown, dPA, dx, dx_from_g ? 1 : 0, N, Cin, Cout, T, V, inter_c, S,
                                   st);
}

}  // namespace stgcn
