// Backward kernels of the AltFormer heads' transformer block (vit.h, "backward"): the weight / bias gradient of a linear,
// the LayerNorm backward, the attention backward and the weight transpose that turns a dgrad into a forward linear.
// Nothing here uses atomics: every output element has one owner and a fixed summation order, and reductions over the
// tokens are written as partial slabs that launch_sum_parts (gemm_f32.hip) adds in slab order, so two runs are bit-identical.
//
// wgrad: dW (Nout, K) = dY^T A is a product whose contraction index (the token) is the slow index of both operands, so a
//   chunk of 32 tokens of dY (32 x 128) and of A (32 x 128) goes to LDS exactly as it lies in memory and the MFMA fragments
//   are read along the rows (32 consecutive floats per half-wave: no transpose, no bank conflict; the two halves of a wave
//   take the two tokens of one v_mfma_f32_32x32x2_f32, and the row stride of 160 floats puts them 32 banks apart).
//   A workgroup of 4 waves owns a 128 x 128 tile of dW for one range of tokens; the column sums of dY (the bias gradient)
//   ride in the workgroups of the first K tile, summed by the threads that stage dY.
//   (The kernel itself is in vit_wgrad_kernel.h: the ST-ViT head's patch embedding runs it on rows of its own.)
//   A second form of the same code owns a 64 x 64 tile (one accumulator block per wave, chunks of 32 x 64, a dense LDS image):
//   four times the workgroups per split, for calls whose tokens cannot supply them.  plan_wgrad (vit.h) picks the form and
//   the cut; where it says one split and the call does not accumulate, the slab the kernel writes is dW itself.
//
// attention backward: built from vit_attention_common.h, which describes the layout it shares with the forward.  One
//   workgroup per (sequence, head) pair as there (several pairs for L <= 64), two phases:
//   (a) K and V in LDS, a wave per 32 queries with its Q (pre-scaled) and dO rows in registers: S^T = K Q^T, the soft-max
//       row maximum and sum, P, delta = rowsum(dO * O), dP^T = V dO^T, dS = P (dP - delta), and dQ^T = K^T dS^T with the
//       accumulator registers of dS^T as the B operand (the forward's O^T = V^T P^T form).  Row maximum, 1 / sum and delta
//       of every query go to LDS (12 bytes per query).
//   (b) LDS reloaded with scale * Q and dO, a wave per 32 keys with its K and V rows in registers: S = Q K^T (the same
//       products in the same order as in (a), so P is bit-identical), P from the row statistics, dP = dO V^T, dS, then
//       dV^T = dO^T P and dK^T = (scale Q)^T dS, again with the accumulators as the B operand.
//   Seven products instead of five; no sum across waves, no L x L matrix outside registers.
//   LDS: ceil(L/32)*32 * (2 (hd + 1) + 4) * 4 bytes = 134 KiB at L = 256, hd 64.
#include "vit_attention_common.h"
#include "vit_wgrad_kernel.h"

namespace stgcn {
namespace vit {

namespace {

// ---- transpose ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_pad_kernel(const float *__restrict__ W, float *__restrict__ Wt, int rows,
                                                           int cols, int rows_pad) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        t[ty + 8 * i][tx] = r < rows && c < cols ? W[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (c < cols && r < rows_pad) Wt[(size_t)c * rows_pad + r] = t[tx][ty + 8 * i];
    }
}

// ---- masked gradient --------------------------------------------------------------------------------------------------------
// out = a * m over n4 float4s, a grid-stride loop: one 16-byte load of each operand and one 16-byte store per step.
__global__ __launch_bounds__(256) void mask_mul_kernel(const float4 *__restrict__ a, const float4 *__restrict__ m,
                                                       float4 *__restrict__ out, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 va = a[i], vm = m[i];
        out[i] = make_float4(va.x * vm.x, va.y * vm.y, va.z * vm.z, va.w * vm.w);
    }
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------------
// vit_wgrad_kernel.h holds the kernel: vit_patch_backward.hip runs it too, on the patch embedding's rows.
using namespace wgrad_kernel;

// ---- LayerNorm backward -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per row; the row (D floats, at most 16 KiB) is read three times, from the cache after the first
__global__ __launch_bounds__(256) void vit_ln_backward_kernel(const float *x, const float *dn, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, float eps, const float *dres,
                                                             float *dx, float *a, float *stats, int M, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float4 *xp = reinterpret_cast<const float4 *>(x + (size_t)row * D);
    const float4 *gp = reinterpret_cast<const float4 *>(dn + (size_t)row * D);
    const float4 *wp = reinterpret_cast<const float4 *>(gamma);
    const int nv = D >> 2;
    float s = 0.f;
    for (int j = lane; j < nv; j += 64) {
        const float4 v = xp[j];
        s += (v.x + v.y) + (v.z + v.w);
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f, s1 = 0.f, s2 = 0.f;
    for (int j = lane; j < nv; j += 64) {
        const float4 v = xp[j], g = gp[j], w = wp[j];
        const float cx = v.x - mean, cy = v.y - mean, cz = v.z - mean, cw = v.w - mean;
        const float gx = g.x * w.x, gy = g.y * w.y, gz = g.z * w.z, gw = g.w * w.w;
        q += (cx * cx + cy * cy) + (cz * cz + cw * cw);
        s1 += (gx + gy) + (gz + gw);
        s2 += (gx * cx + gy * cy) + (gz * cz + gw * cw);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) * rstd / (float)D;
    // every lane has read the whole row before any lane writes: dx may alias dn or dres
    const float4 *rp = reinterpret_cast<const float4 *>(dres != nullptr ? dres + (size_t)row * D : nullptr);
    const float4 *bp = reinterpret_cast<const float4 *>(beta);
    float4 *op = reinterpret_cast<float4 *>(dx + (size_t)row * D);
    float4 *ap = reinterpret_cast<float4 *>(a != nullptr ? a + (size_t)row * D : nullptr);
    for (int j = lane; j < nv; j += 64) {
        const float4 v = xp[j], g = gp[j], w = wp[j];
        const float hx = (v.x - mean) * rstd, hy = (v.y - mean) * rstd, hz = (v.z - mean) * rstd, hw = (v.w - mean) * rstd;
        float4 o;
        o.x = rstd * (g.x * w.x - m1 - hx * m2);
        o.y = rstd * (g.y * w.y - m1 - hy * m2);
        o.z = rstd * (g.z * w.z - m1 - hz * m2);
        o.w = rstd * (g.w * w.w - m1 - hw * m2);
        if (rp != nullptr) {
            const float4 r = rp[j];
            o.x += r.x, o.y += r.y, o.z += r.z, o.w += r.w;
        }
        op[j] = o;
        if (ap != nullptr) {
            const float4 b = bp[j];
            ap[j] = make_float4(hx * w.x + b.x, hy * w.y + b.y, hz * w.z + b.z, hw * w.w + b.w);
        }
    }
    if (lane == 0 && stats != nullptr) {
        stats[2 * (size_t)row] = mean;
        stats[2 * (size_t)row + 1] = rstd;
    }
}

constexpr int kLnRows = 64;    // rows per partial of the LayerNorm parameter gradients (256 left a slab with 128 workgroups of
                               // one dependent chain per thread: 97 us per call; the loads of four rows are now in flight together)

// part[0][split][c] = sum over the split's rows of dn xhat, part[1][split][c] = sum of dn; a thread owns a column
__global__ __launch_bounds__(256) void vit_ln_param_kernel(const float *__restrict__ x, const float *__restrict__ dn,
                                                          const float *__restrict__ stats, float *__restrict__ part, int M,
                                                          int D) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int r_lo = blockIdx.y * kLnRows, r_hi = min(M, r_lo + kLnRows);
    if (c >= D) return;
    float sg = 0.f, sb = 0.f;
    int r = r_lo;
    for (; r + 3 < r_hi; r += 4) {   // four rows' loads issued together, added in row order
        float g[4], h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            g[i] = dn[(size_t)(r + i) * D + c];
            h[i] = (x[(size_t)(r + i) * D + c] - stats[2 * (size_t)(r + i)]) * stats[2 * (size_t)(r + i) + 1];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sg += g[i] * h[i];
            sb += g[i];
        }
    }
    for (; r < r_hi; ++r) {
        const float g = dn[(size_t)r * D + c];
        sg += g * ((x[(size_t)r * D + c] - stats[2 * (size_t)r]) * stats[2 * (size_t)r + 1]);
        sb += g;
    }
    part[(size_t)blockIdx.y * D + c] = sg;
    part[((size_t)gridDim.y + blockIdx.y) * D + c] = sb;
}

// ---- attention backward -------------------------------------------------------------------------------------------------------
template <int HD, int NT>
__global__ __launch_bounds__(512) void vit_attention_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ out,
                                                               const float *__restrict__ dout, float *__restrict__ dqkv,
                                                               int pairs, int L, int H, float scale, int G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ROWS = NT * 32, KS = HD + kPadF32, HH = HD / 2;
    float *As = lds;                              // [G][ROWS][KS]: K in phase (a), scale * Q in phase (b)
    float *Bs = lds + (size_t)G * ROWS * KS;      // [G][ROWS][KS]: V in phase (a), dO in phase (b)
    float *Ss = lds + (size_t)2 * G * ROWS * KS;  // [G][ROWS][4]: row maximum, 1 / row sum, delta of every query
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD, otok = (size_t)H * HD;
    const int nvec = G * ROWS * (HD / 4);

    for (int e = tid; e < nvec; e += blockDim.x) {
        const int d4 = e % (HD / 4), j = (e / (HD / 4)) % ROWS, g = e / ((HD / 4) * ROWS);
        const int p = blockIdx.x * G + g;
        float4 k = make_float4(0.f, 0.f, 0.f, 0.f), v = k;
        if (p < pairs && j < L) {
            const float *base = qkv + ((size_t)(p / H) * L + j) * tok + (size_t)(p % H) * HD + d4 * 4;
            k = *reinterpret_cast<const float4 *>(base + (size_t)H * HD);
            v = *reinterpret_cast<const float4 *>(base + (size_t)2 * H * HD);
        }
        float *kd = As + ((size_t)g * ROWS + j) * KS + d4 * 4, *vd = Bs + ((size_t)g * ROWS + j) * KS + d4 * 4;
        kd[0] = k.x, kd[1] = k.y, kd[2] = k.z, kd[3] = k.w;
        vd[0] = v.x, vd[1] = v.y, vd[2] = v.z, vd[3] = v.w;
    }
    __syncthreads();

    const int g = wave / NT, t = wave % NT;
    const int p = blockIdx.x * G + g;
    const bool active = p < pairs && t * 32 < L;  // wave-uniform
    const int b = active ? p / H : 0, h = active ? p % H : 0;
    const int ri = t * 32 + l31;                  // the lane's query in phase (a), its key in phase (b)
    const float *Ag = As + (size_t)g * ROWS * KS, *Bg = Bs + (size_t)g * ROWS * KS;
    float *Sg = Ss + (size_t)g * ROWS * 4;

    // ---- phase (a): a wave per 32 queries ----
    if (active) {
        float qf[HH], df[HH];
        float delta = 0.f;
        if (ri < L) {
            const float4 *qp = reinterpret_cast<const float4 *>(qkv + ((size_t)b * L + ri) * tok + (size_t)h * HD + half * HH);
            const float4 *dp = reinterpret_cast<const float4 *>(dout + ((size_t)b * L + ri) * otok + (size_t)h * HD + half * HH);
            const float4 *op = reinterpret_cast<const float4 *>(out + ((size_t)b * L + ri) * otok + (size_t)h * HD + half * HH);
#pragma unroll
            for (int s = 0; s < HH / 4; ++s) {
                const float4 v = qp[s], d = dp[s], o = op[s];
                qf[4 * s] = v.x * scale, qf[4 * s + 1] = v.y * scale, qf[4 * s + 2] = v.z * scale, qf[4 * s + 3] = v.w * scale;
                df[4 * s] = d.x, df[4 * s + 1] = d.y, df[4 * s + 2] = d.z, df[4 * s + 3] = d.w;
                delta += (d.x * o.x + d.y * o.y) + (d.z * o.z + d.w * o.w);
            }
        } else {
#pragma unroll
            for (int s = 0; s < HH; ++s) qf[s] = 0.f, df[s] = 0.f;
        }
        delta += __shfl_xor(delta, 32, 64);

        f32x16 sc[NT];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
            const float *kp = Ag + (size_t)(kt * 32 + l31) * KS + half * HH;
#pragma unroll
            for (int s = 0; s < HH; ++s) sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[s], qf[s], sc[kt], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = ACC_KEY(kt * 32, i, half);
                if (key >= L) sc[kt][i] = -INFINITY;
                mx = fmaxf(mx, sc[kt][i]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float e = __expf(sc[kt][i] - mx);
                sc[kt][i] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
        if (half == 0) {
            Sg[ri * 4] = ri < L ? mx : 0.f;
            Sg[ri * 4 + 1] = ri < L ? inv : 0.f;
            Sg[ri * 4 + 2] = ri < L ? delta : 0.f;
        }
        // dP^T = V dO^T per key tile, dS^T = P^T (dP^T - delta) in place of P^T
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            f32x16 dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) dp[i] = 0.f;
            const float *vp = Bg + (size_t)(kt * 32 + l31) * KS + half * HH;
#pragma unroll
            for (int s = 0; s < HH; ++s) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[s], df[s], dp, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) sc[kt][i] = sc[kt][i] * inv * (dp[i] - delta);
        }
        // dQ^T = K^T dS^T
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt) {
            f32x16 o;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = ACC_KEY(kt * 32, i, half);
                    o = __builtin_amdgcn_mfma_f32_32x32x2f32(Ag[(size_t)key * KS + dt * 32 + l31], sc[kt][i], o, 0, 0, 0);
                }
            if (ri < L) {
                float *qo = dqkv + ((size_t)b * L + ri) * tok + (size_t)h * HD + dt * 32 + 4 * half;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    *reinterpret_cast<float4 *>(qo + 8 * r) =
                        make_float4(o[4 * r] * scale, o[4 * r + 1] * scale, o[4 * r + 2] * scale, o[4 * r + 3] * scale);
            }
        }
    }
    __syncthreads();

    // ---- phase (b): LDS <- scale * Q and dO, a wave per 32 keys ----
    for (int e = tid; e < nvec; e += blockDim.x) {
        const int d4 = e % (HD / 4), j = (e / (HD / 4)) % ROWS, gg = e / ((HD / 4) * ROWS);
        const int pp = blockIdx.x * G + gg;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), d = q;
        if (pp < pairs && j < L) {
            const size_t row = (size_t)(pp / H) * L + j;
            q = *reinterpret_cast<const float4 *>(qkv + row * tok + (size_t)(pp % H) * HD + d4 * 4);
            d = *reinterpret_cast<const float4 *>(dout + row * otok + (size_t)(pp % H) * HD + d4 * 4);
        }
        float *qd = As + ((size_t)gg * ROWS + j) * KS + d4 * 4, *dd = Bs + ((size_t)gg * ROWS + j) * KS + d4 * 4;
        qd[0] = q.x * scale, qd[1] = q.y * scale, qd[2] = q.z * scale, qd[3] = q.w * scale;
        dd[0] = d.x, dd[1] = d.y, dd[2] = d.z, dd[3] = d.w;
    }
    __syncthreads();
    if (!active) return;

    float kf[HH], vf[HH];
    if (ri < L) {
        const float *base = qkv + ((size_t)b * L + ri) * tok + (size_t)h * HD + half * HH;
        const float4 *kp = reinterpret_cast<const float4 *>(base + (size_t)H * HD);
        const float4 *vp = reinterpret_cast<const float4 *>(base + (size_t)2 * H * HD);
#pragma unroll
        for (int s = 0; s < HH / 4; ++s) {
            const float4 k = kp[s], v = vp[s];
            kf[4 * s] = k.x, kf[4 * s + 1] = k.y, kf[4 * s + 2] = k.z, kf[4 * s + 3] = k.w;
            vf[4 * s] = v.x, vf[4 * s + 1] = v.y, vf[4 * s + 2] = v.z, vf[4 * s + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < HH; ++s) kf[s] = 0.f, vf[s] = 0.f;
    }
    f32x16 dk[HD / 32], dv[HD / 32];
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dk[dt][i] = 0.f, dv[dt][i] = 0.f;
#pragma unroll 1
    for (int qt = 0; qt < NT; ++qt) {
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
        const float *qp = Ag + (size_t)(qt * 32 + l31) * KS + half * HH, *op = Bg + (size_t)(qt * 32 + l31) * KS + half * HH;
#pragma unroll
        for (int c = 0; c < HH; ++c) {
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(qp[c], kf[c], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(op[c], vf[c], dp, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = ACC_KEY(qt * 32, i, half);
            const float4 st = *reinterpret_cast<const float4 *>(&Sg[q * 4]);   // (max, 1 / sum, delta, -); 1 / sum = 0 past L
            const float pr = ri < L ? __expf(s[i] - st.x) * st.y : 0.f;
            s[i] = pr;
            dp[i] = pr * (dp[i] - st.z);
        }
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = ACC_KEY(qt * 32, i, half);
                dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Bg[(size_t)q * KS + dt * 32 + l31], s[i], dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ag[(size_t)q * KS + dt * 32 + l31], dp[i], dk[dt], 0, 0, 0);
            }
    }
    if (ri < L) {
        float *base = dqkv + ((size_t)b * L + ri) * tok + (size_t)h * HD + 4 * half;
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                *reinterpret_cast<float4 *>(base + (size_t)H * HD + dt * 32 + 8 * r) =
                    make_float4(dk[dt][4 * r], dk[dt][4 * r + 1], dk[dt][4 * r + 2], dk[dt][4 * r + 3]);
                *reinterpret_cast<float4 *>(base + (size_t)2 * H * HD + dt * 32 + 8 * r) =
                    make_float4(dv[dt][4 * r], dv[dt][4 * r + 1], dv[dt][4 * r + 2], dv[dt][4 * r + 3]);
            }
    }
}

struct AttentionBackward {
    static constexpr const char *what = "vit attention backward", *kernel_name = "vit_attention_bwd_kernel";
    static constexpr size_t lds_bytes(int nt, int hd) { return attention_bwd_f32_lds_bytes(nt, hd); }
    template <int HD, int NT>
    static auto kernel() { return vit_attention_bwd_kernel<HD, NT>; }
};

}  // namespace

// partial slabs -> dst, or dst += their sum
int reduce_parts(const float *part, int parts, size_t n, float *dst, float *tmp, bool accumulate, hipStream_t st) {
    int rc;
    if (!accumulate) return launch_sum_parts(part, dst, parts, n, st);
    if ((rc = launch_sum_parts(part, tmp, parts, n, st))) return rc;
    return launch_add_inplace(dst, tmp, n, st);
}

int launch_transpose_pad(const float *W, float *Wt, int rows, int cols, int rows_pad, hipStream_t st) {
    transpose_pad_kernel<<<dim3(ceil_div(cols, 32), ceil_div(rows_pad, 32)), dim3(256), 0, st>>>(W, Wt, rows, cols, rows_pad);
    STGCN_LAUNCH_CHECK("transpose_pad_kernel");
    return STGCN_OK;
}

int launch_mask_mul(const float *a, const float *m, float *out, size_t n, hipStream_t st) {
    if (n == 0 || n % 4 != 0 || (((uintptr_t)a | (uintptr_t)m | (uintptr_t)out) & 15) != 0)
        return fail(STGCN_ERR_ARG, "vit mask: %zu elements, or an operand that is not 16-byte aligned", n);
    const size_t n4 = n / 4, want = (n4 + 255) / 256;
    mask_mul_kernel<<<dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, st>>>(
        reinterpret_cast<const float4 *>(a), reinterpret_cast<const float4 *>(m), reinterpret_cast<float4 *>(out), n4);
    STGCN_LAUNCH_CHECK("mask_mul_kernel");
    return STGCN_OK;
}

// About 512 workgroups (two per CU) where the rows allow it, a split at least 256 rows long, ranges multiples of the chunk.
// (The default cut of every weight gradient; plan_wgrad in vit.h builds STGCN_VIT_WGRAD_SMALL's rule next to it.)
int wgrad_rows_per_split(int M, int K, int Nout) {
    const int tiles = ceil_div(Nout, WT) * ceil_div(K, WT);
    int splits = ceil_div(512, tiles);
    const int most = ceil_div(M, 256);
    if (splits > most) splits = most;
    return ceil_div(ceil_div(M, splits), WC) * WC;
}

// The one launcher of both forms of the fp32 kernel.  Where the plan says one split and the caller does not accumulate, the
// kernel's slab IS dW (and its bias slab db): no launch_sum_parts.
int launch_wgrad(const WgradPlan &wp, const float *dY, const float *A, const float *rowscale, int L, float *dW, float *db,
                 float *part, float *tmp, int M, int K, int Nout, bool accumulate, hipStream_t st) {
    const bool direct = wp.direct(accumulate);
    const int tiles_n = ceil_div(Nout, wp.tile), tiles_k = ceil_div(K, wp.tile);
    float *slab = direct ? dW : part;
    float *bpart = db == nullptr ? nullptr : direct ? db : part + (size_t)wp.splits * Nout * K;
    const dim3 grid((unsigned)(tiles_n * tiles_k * wp.splits));
    if (wp.tile == 64)
        vit_wgrad_kernel<DenseWgradRows, 64><<<grid, dim3(256), 0, st>>>(dY, A, rowscale, L, slab, bpart, M, K, Nout, tiles_n, tiles_k,
                                                                         wp.cps, wp.long_splits, DenseWgradRows{});
    else
        vit_wgrad_kernel<DenseWgradRows, 128><<<grid, dim3(256), 0, st>>>(dY, A, rowscale, L, slab, bpart, M, K, Nout, tiles_n, tiles_k,
                                                                          wp.cps, wp.long_splits, DenseWgradRows{});
    STGCN_LAUNCH_CHECK("vit_wgrad_kernel");
    if (direct) return STGCN_OK;
    int rc;
    if ((rc = reduce_parts(part, wp.splits, (size_t)Nout * K, dW, tmp, accumulate, st))) return rc;
    if (db != nullptr && (rc = reduce_parts(bpart, wp.splits, (size_t)Nout, db, tmp, accumulate, st))) return rc;
    return STGCN_OK;
}

int launch_ln_backward(const float *x, const float *dn, const float *gamma, const float *beta, float eps, const float *dres,
                       float *dx, float *a, float *stats, int M, int D, hipStream_t st) {
    if (!grid_fits(ceil_div(M, 4), 256)) return fail(STGCN_ERR_UNSUPPORTED, "vit layernorm backward: %d rows exceed the grid", M);
    vit_ln_backward_kernel<<<dim3(ceil_div(M, 4)), dim3(256), 0, st>>>(x, dn, gamma, beta, eps, dres, dx, a, stats, M, D);
    STGCN_LAUNCH_CHECK("vit_ln_backward_kernel");
    return STGCN_OK;
}

int ln_param_splits(int M) { return ceil_div(M, kLnRows); }

int launch_ln_param_grad(const float *x, const float *dn, const float *stats, float *dgamma, float *dbeta, float *part,
                         float *tmp, int M, int D, bool accumulate, hipStream_t st) {
    const int splits = ln_param_splits(M);
    if (splits > 65535) return fail(STGCN_ERR_UNSUPPORTED, "vit layernorm backward: %d row ranges", splits);
    vit_ln_param_kernel<<<dim3(ceil_div(D, 256), splits), dim3(256), 0, st>>>(x, dn, stats, part, M, D);
    STGCN_LAUNCH_CHECK("vit_ln_param_kernel");
    int rc;
    if ((rc = reduce_parts(part, splits, (size_t)D, dgamma, tmp, accumulate, st))) return rc;
    return reduce_parts(part + (size_t)splits * D, splits, (size_t)D, dbeta, tmp, accumulate, st);
}

int launch_attention_backward(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L, int H, int hd,
                              float scale, hipStream_t st) {
    return launch_resident<AttentionBackward>(B, L, H, hd, scale, st, qkv, out, dout, dqkv);
}

}  // namespace vit
}  // namespace stgcn
