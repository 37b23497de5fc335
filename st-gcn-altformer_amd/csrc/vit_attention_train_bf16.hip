// Multi-head attention of the AltFormer heads' blocks for TRAINING on bf16 matrix operands (STGCN_VIT_TRAIN_ATTN_BF16 of
// stgcn_vit_block_forward_train / stgcn_vit_block_backward): forward and backward of
//     qkv (B, L, 3, H, hd) fp32 as the qkv linear stores it  ->  out (B, L, H*hd) fp32,  dout -> dqkv (packed as qkv, fp32)
// on v_mfma_f32_32x32x16_bf16, resident form (L <= 256), head_dim 32 / 64, built from vit_attention_common.h, which describes the
// layout.  Everything in memory is fp32; operands are split or rounded (r = round to nearest-even bf16) while they are staged,
// every sum is fp32.
//
// The arithmetic (DESIGN section 15 "bf16 attention"), per (sequence, head):
//   s  = scale * (qh kh^T + qh kl^T + ql kh^T),  qh = r(q), ql = r(q - qh), kh, kl alike, of the UNSCALED q and k.  A rounded q
//        or k is multiplied by the size of the scores before the exponential, so the score product alone takes three terms.
//        Order into the fp32 accumulator, the same wherever a score is computed (forward, backward phase (a) and (b)):
//        per key tile of 32, per k-step of 16 channels in ascending order: kl * qh, then kh * ql, then kh * qh (score_step).
//        The products are exact in fp32 and the matrix core adds a k-step's 16 products in one order whichever operand is A
//        and which is B, so the three places agree bit for bit.  fp contraction is OFF in this file, the shared pieces
//        included below the pragma with it: s * scale - m is a multiply and a subtract everywhere.
//   m  = max s,  p = exp(s - m),  l = sum p (of the unrounded fp32 p);  keys past L are zero-filled in LDS and score -inf.
//   forward : out = (r(p) r(v)) / l
//   backward: P = p / l,  dP = r(dO) r(v)^T,  delta_i = sum_j P_ij dP_ij (fp32, of the unrounded P and the kernel's own dP: each
//             row of dS then sums to zero up to fp32 rounding; `out` is not read),  dS = P (dP - delta),
//             dV = r(P)^T r(dO),  dQ = scale * r(dS) r(k),  dK = scale * r(dS)^T r(q).
//
// Forward: vit_attention_bf16.hip with fp32 memory on both sides.  A pair gets NT = ceil(L / 32) waves, a wave 32 queries as hi
//   and lo B fragments; K is staged as a hi and a lo tile [keys][hd + 8], V transposed and permuted [hd][keys + 8];
//   the score accumulators, exponentiated, rounded and packed in place, are the B operand of O^T = V^T P^T.
// Backward: the two phases of vit_attention_bwd_kernel (vit_backward.hip), a workgroup per pair (several for L <= 64):
//   (a) LDS: K hi, K lo, V as rows [keys][hd + 8], K hi transposed and permuted [hd][keys + 8].  A wave per 32 queries: S^T, the
//       statistics, dP^T = V dO^T (B = the wave's dO rows from memory, rounded), delta, dS^T in the score registers, and
//       dQ^T = K^T dS^T with the packed dS^T as B operand.  (m, 1 / l, delta) per query go to LDS.
//   (b) LDS reloaded: Q hi, Q lo, dO as rows, Q hi and dO transposed and permuted.  A wave per 32 keys with its K (hi, lo) and V
//       rows as B fragments: S = Q K^T, P from the statistics, dP = dO V^T, dS, then dV^T = dO^T P and dK^T = Q^T dS with the
//       packed accumulators as B operand.
//   At L > 224 with hd = 64 the five tiles of (b) are 178 KiB, more than the 160 there are: that one instantiation (SPLIT)
//   walks the query tiles twice.  The first walk has dO^T staged and computes S, P and dV^T; then, between two barriers, Q^T
//   is written over dO^T (from the Q hi rows in LDS), and the second walk computes S and P again, dP, dS and dK^T.  Every
//   output sees the same products in the same order as in the other instantiations; the price is the score product twice.
// LDS reads and writes, banks: a fragment read is 16 bytes per lane, lane = row; the hardware serves it in four groups of 16
//   lanes of one lane half (256 bytes = all 64 banks once), and the rows of a group are one of each residue mod 16.  The
//   strides are 20, 36 and 16 NT + 4 dwords = 4 x an odd number, so the 16 rows of a group start at 16 distinct multiples of 4
//   banks and their four-bank spans do not overlap: conflict-free.  Row tiles are written 16 bytes per thread, consecutive
//   threads consecutive pieces of a row: 8 lanes cover 128 contiguous bytes at hd = 64 (conflict-free); at hd = 32 they cover
//   two rows 80 bytes apart, whose last and first pieces share a bank (2-way on one pair of 8).
//   The transposed tiles are NOT conflict-free to write: 2 bytes per thread and channel row, and the threads of one token
//   are 8 channel rows = 128 NT + 32 dwords = 0 mod 32 banks apart, so the hd / 8 threads of a token collide, and four
//   neighbouring tokens share two dwords: up to 16-way.  The scatter runs once per tile (one tile in a forward, three in a
//   backward), not in the product loops.
#include <type_traits>

#include "bf16_common.h"
#include "vit.h"

#pragma clang fp contract(off)

#include "vit_attention_common.h"

namespace stgcn {
namespace vit {

namespace {

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <int HD, int NT>
__global__ __launch_bounds__(512) void vit_attention_train_bf16_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                                      int pairs, int L, int H, float scale, int G) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds16[];
    constexpr int ROWS = NT * 32, KS = HD + kPad16, VS = ROWS + kPad16, KST = HD / 16;
    unsigned short *Kh = lds16;                              // [G][ROWS][KS]
    unsigned short *Kl = Kh + (size_t)G * ROWS * KS;         // [G][ROWS][KS]
    unsigned short *Vt = Kl + (size_t)G * ROWS * KS;         // [G][HD][VS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD;

    const int nvec = G * ROWS * (HD / 8);
    for (int e = tid; e < nvec; e += blockDim.x) {
        const StageSlot s = stage_slot<HD, ROWS, 8>(e, G, pairs, L, H);
        float k[8], v[8];
        zero8(k);
        zero8(v);
        if (s.live) {
            const float *base = qkv + s.tok * tok + s.col;
            load8(base + (size_t)H * HD, k);
            load8(base + (size_t)2 * H * HD, v);
        }
        uint4 hi, lo;
        split8(k, hi, lo);
        *reinterpret_cast<uint4 *>(Kh + ((size_t)s.g * ROWS + s.j) * KS + s.d0) = hi;
        *reinterpret_cast<uint4 *>(Kl + ((size_t)s.g * ROWS + s.j) * KS + s.d0) = lo;
        scatter8(Vt + ((size_t)s.g * HD + s.d0) * VS, VS, perm16(s.j), round8(v));
    }
    __syncthreads();

    const int g = wave / NT, qt = wave % NT;
    const int p = blockIdx.x * G + g;
    if (p >= pairs || qt * 32 >= L) return;   // wave-uniform, after the only barrier
    const int b = p / H, h = p % H;
    const int qi = qt * 32 + l31;

    uint4 qh[KST], ql[KST];
    {
        const float *qp = qkv + ((size_t)b * L + (qi < L ? qi : 0)) * tok + (size_t)h * HD + half * 8;
#pragma unroll
        for (int s = 0; s < KST; ++s) {
            float q[8];
            zero8(q);
            if (qi < L) load8(qp + 16 * s, q);
            split8(q, qh[s], ql[s]);
        }
    }

    const unsigned short *Khg = Kh + (size_t)g * ROWS * KS, *Klg = Kl + (size_t)g * ROWS * KS, *Vg = Vt + (size_t)g * HD * VS;
    f32x16 sc[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
        const size_t ko = (size_t)(kt * 32 + l31) * KS + half * 8;
#pragma unroll
        for (int s = 0; s < KST; ++s) sc[kt] = score_step(lds16B(Khg + ko + 16 * s), lds16B(Klg + ko + 16 * s), qh[s], ql[s], sc[kt], true);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sc[kt][i] *= scale;
            if (kt == NT - 1 && ACC_KEY(kt * 32, i, half) >= L) sc[kt][i] = -INFINITY;
            mx = fmaxf(mx, sc[kt][i]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // key 0 is always valid: mx is finite
    float sum = 0.f;
    uint4 pk[NT][2];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        float e[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            e[i] = __expf(sc[kt][i] - mx);    // exp(-inf) = 0: masked keys
            sum += e[i];
        }
        pk[kt][0] = pack8(e, 0);
        pk[kt][1] = pack8(e, 1);
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt) {
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
        const unsigned short *vp = Vg + (size_t)(dt * 32 + l31) * VS + half * 8;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int gk = 0; gk < 2; ++gk) o = mfma(lds16B(vp + kt * 32 + gk * 16), pk[kt][gk], o);
        if (qi < L) store_rows(out + ((size_t)b * L + qi) * ((size_t)H * HD) + (size_t)h * HD + dt * 32 + 4 * half, o, inv);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
template <int HD, int NT, bool SPLIT>
__global__ __launch_bounds__(512) void vit_attention_bwd_bf16_kernel(const float *__restrict__ qkv, const float *__restrict__ dout,
                                                                    float *__restrict__ dqkv, int pairs, int L, int H,
                                                                    float scale, int G) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds16[];
    constexpr int ROWS = NT * 32, KS = HD + kPad16, VS = ROWS + kPad16, KST = HD / 16;
    const size_t rt = (size_t)G * ROWS * KS, tt = (size_t)G * HD * VS;   // elements of a row tile, of a transposed tile
    unsigned short *R0 = lds16;          // [G][ROWS][KS]: K hi in (a), Q hi in (b)
    unsigned short *R1 = R0 + rt;        // K lo, Q lo
    unsigned short *R2 = R1 + rt;        // V, dO
    unsigned short *T0 = R2 + rt;        // [G][HD][VS]: K hi^T in (a); dO^T in (b), then Q hi^T if SPLIT
    unsigned short *T1 = T0 + tt;        // Q hi^T in (b) unless SPLIT
    float *Ss = reinterpret_cast<float *>(T0 + (SPLIT ? 1 : 2) * tt);   // [G][ROWS][4]: row maximum, 1 / row sum, delta
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD, otok = (size_t)H * HD;
    const int nvec = G * ROWS * (HD / 8);

    for (int e = tid; e < nvec; e += blockDim.x) {
        const StageSlot s = stage_slot<HD, ROWS, 8>(e, G, pairs, L, H);
        float k[8], v[8];
        zero8(k);
        zero8(v);
        if (s.live) {
            const float *base = qkv + s.tok * tok + s.col;
            load8(base + (size_t)H * HD, k);
            load8(base + (size_t)2 * H * HD, v);
        }
        uint4 hi, lo;
        split8(k, hi, lo);
        const size_t ro = ((size_t)s.g * ROWS + s.j) * KS + s.d0;
        *reinterpret_cast<uint4 *>(R0 + ro) = hi;
        *reinterpret_cast<uint4 *>(R1 + ro) = lo;
        *reinterpret_cast<uint4 *>(R2 + ro) = round8(v);
        scatter8(T0 + ((size_t)s.g * HD + s.d0) * VS, VS, perm16(s.j), hi);
    }
    __syncthreads();

    const int g = wave / NT, t = wave % NT;
    const int p = blockIdx.x * G + g;
    const bool active = p < pairs && t * 32 < L;   // wave-uniform
    const int b = active ? p / H : 0, h = active ? p % H : 0;
    const int ri = t * 32 + l31;                   // the lane's query in phase (a), its key in phase (b)
    const unsigned short *R0g = R0 + (size_t)g * ROWS * KS, *R1g = R1 + (size_t)g * ROWS * KS, *R2g = R2 + (size_t)g * ROWS * KS;
    const unsigned short *T0g = T0 + (size_t)g * HD * VS, *T1g = T1 + (size_t)g * HD * VS;
    float *Sg = Ss + (size_t)g * ROWS * 4;

    // ---- phase (a): a wave per 32 queries ----
    if (active) {
        f32x16 sc[NT];
        float mx = -INFINITY;
        {
            uint4 qh[KST], ql[KST];
            const float *qp = qkv + ((size_t)b * L + (ri < L ? ri : 0)) * tok + (size_t)h * HD + half * 8;
#pragma unroll
            for (int s = 0; s < KST; ++s) {
                float q[8];
                zero8(q);
                if (ri < L) load8(qp + 16 * s, q);
                split8(q, qh[s], ql[s]);
            }
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
                const size_t ko = (size_t)(kt * 32 + l31) * KS + half * 8;
#pragma unroll
                for (int s = 0; s < KST; ++s)
                    sc[kt] = score_step(lds16B(R0g + ko + 16 * s), lds16B(R1g + ko + 16 * s), qh[s], ql[s], sc[kt], true);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sc[kt][i] *= scale;
                    if (kt == NT - 1 && ACC_KEY(kt * 32, i, half) >= L) sc[kt][i] = -INFINITY;
                    mx = fmaxf(mx, sc[kt][i]);
                }
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

        // dP^T = V dO^T per key tile; P in place of p, delta = sum P dP in register order, then across the two lane halves
        uint4 df[KST];
        {
            const float *dp = dout + ((size_t)b * L + (ri < L ? ri : 0)) * otok + (size_t)h * HD + half * 8;
#pragma unroll
            for (int s = 0; s < KST; ++s) {
                float d[8];
                zero8(d);
                if (ri < L) load8(dp + 16 * s, d);
                df[s] = round8(d);
            }
        }
        // The dP accumulators of all key tiles do not fit next to the scores, so delta takes one pass over the tiles and dS a
        // second one that computes the same dP again (same operands, same order: the same bits).
        float delta = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            f32x16 dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) dp[i] = 0.f;
            const size_t vo = (size_t)(kt * 32 + l31) * KS + half * 8;
#pragma unroll
            for (int s = 0; s < KST; ++s) dp = mfma(lds16B(R2g + vo + 16 * s), df[s], dp);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                sc[kt][i] = sc[kt][i] * inv;
                delta += sc[kt][i] * dp[i];
            }
        }
        delta += __shfl_xor(delta, 32, 64);
        if (half == 0) {
            Sg[ri * 4] = ri < L ? mx : 0.f;
            Sg[ri * 4 + 1] = ri < L ? inv : 0.f;
            Sg[ri * 4 + 2] = ri < L ? delta : 0.f;
        }
        uint4 dsp[NT][2];                         // dS^T, rounded and packed: the B operand of dQ^T = K^T dS^T
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            f32x16 dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) dp[i] = 0.f;
            const size_t vo = (size_t)(kt * 32 + l31) * KS + half * 8;
#pragma unroll
            for (int s = 0; s < KST; ++s) dp = mfma(lds16B(R2g + vo + 16 * s), df[s], dp);
            float ds[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) ds[i] = sc[kt][i] * (dp[i] - delta);
            dsp[kt][0] = pack8(ds, 0);
            dsp[kt][1] = pack8(ds, 1);
        }
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt) {
            f32x16 o;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] = 0.f;
            const unsigned short *kp = T0g + (size_t)(dt * 32 + l31) * VS + half * 8;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                for (int gk = 0; gk < 2; ++gk) o = mfma(lds16B(kp + kt * 32 + gk * 16), dsp[kt][gk], o);
            if (ri < L) {
                float *qo = dqkv + ((size_t)b * L + ri) * tok + (size_t)h * HD + dt * 32 + 4 * half;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    *reinterpret_cast<float4 *>(qo + 8 * r) =
                        make_float4(o[4 * r] * scale, o[4 * r + 1] * scale, o[4 * r + 2] * scale, o[4 * r + 3] * scale);
            }
        }
    } else if (half == 0) {                        // rows nobody computed: statistics that make P = 0
        Sg[ri * 4] = 0.f, Sg[ri * 4 + 1] = 0.f, Sg[ri * 4 + 2] = 0.f;
    }
    __syncthreads();

    // ---- phase (b): LDS <- Q hi, Q lo, dO, dO^T (and Q hi^T), a wave per 32 keys ----
    for (int e = tid; e < nvec; e += blockDim.x) {
        const StageSlot s = stage_slot<HD, ROWS, 8>(e, G, pairs, L, H);
        float q[8], d[8];
        zero8(q);
        zero8(d);
        if (s.live) {
            load8(qkv + s.tok * tok + s.col, q);
            load8(dout + s.tok * otok + s.col, d);
        }
        uint4 hi, lo;
        split8(q, hi, lo);
        const uint4 dr = round8(d);
        const size_t ro = ((size_t)s.g * ROWS + s.j) * KS + s.d0;
        *reinterpret_cast<uint4 *>(R0 + ro) = hi;
        *reinterpret_cast<uint4 *>(R1 + ro) = lo;
        *reinterpret_cast<uint4 *>(R2 + ro) = dr;
        scatter8(T0 + ((size_t)s.g * HD + s.d0) * VS, VS, perm16(s.j), dr);
        if constexpr (!SPLIT) scatter8(T1 + ((size_t)s.g * HD + s.d0) * VS, VS, perm16(s.j), hi);
    }
    __syncthreads();

    f32x16 dk[HD / 32], dv[HD / 32];
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dk[dt][i] = 0.f, dv[dt][i] = 0.f;
    uint4 kh[KST], kl[KST], vf[KST];               // the lane's key: K hi, K lo and V as B fragments
    {
        const bool valid = active && ri < L;
        const float *base = qkv + ((size_t)b * L + (valid ? ri : 0)) * tok + (size_t)h * HD + half * 8;
#pragma unroll
        for (int s = 0; s < KST; ++s) {
            float k[8], v[8];
            zero8(k);
            zero8(v);
            if (valid) {
                load8(base + (size_t)H * HD + 16 * s, k);
                load8(base + (size_t)2 * H * HD + 16 * s, v);
            }
            split8(k, kh[s], kl[s]);
            vf[s] = round8(v);
        }
    }
    // one tile of 32 queries against the lane's key: S, P (and dP, dS), then the dV^T and / or dK^T products of the tile
    auto tile = [&](int qt, auto want_dv, auto want_dk) {
        constexpr bool DV = decltype(want_dv)::value, DK = decltype(want_dk)::value;
        {
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
            const size_t qo = (size_t)(qt * 32 + l31) * KS + half * 8;
#pragma unroll
            for (int c = 0; c < KST; ++c) {
                s = score_step(lds16B(R0g + qo + 16 * c), lds16B(R1g + qo + 16 * c), kh[c], kl[c], s, false);
                if constexpr (DK) dp = mfma(lds16B(R2g + qo + 16 * c), vf[c], dp);
            }
            float pr[16], ds[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int q = ACC_KEY(qt * 32, i, half);
                const float4 st = *reinterpret_cast<const float4 *>(&Sg[q * 4]);   // (max, 1 / sum, delta, -); 1 / sum = 0 past L
                pr[i] = ri < L ? __expf(s[i] * scale - st.x) * st.y : 0.f;
                ds[i] = pr[i] * (dp[i] - st.z);
            }
            const uint4 pp[2] = {pack8(pr, 0), pack8(pr, 1)}, dd[2] = {pack8(ds, 0), pack8(ds, 1)};
            const unsigned short *Qt = SPLIT ? T0g : T1g;   // where Q hi^T lies when the dK products run
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                for (int gk = 0; gk < 2; ++gk) {
                    const size_t to = (size_t)(dt * 32 + l31) * VS + half * 8 + qt * 32 + gk * 16;
                    if constexpr (DV) dv[dt] = mfma(lds16B(T0g + to), pp[gk], dv[dt]);
                    if constexpr (DK) dk[dt] = mfma(lds16B(Qt + to), dd[gk], dk[dt]);
                }
        }
    };
    using yes = std::true_type;
    using no = std::false_type;
    if (active) {
#pragma unroll 1
        for (int qt = 0; qt < NT; ++qt) {
            if constexpr (SPLIT) tile(qt, yes{}, no{});
            else tile(qt, yes{}, yes{});
        }
    }
    if constexpr (SPLIT) {
        __syncthreads();                           // every wave is done with dO^T
        for (int e = tid; e < nvec; e += blockDim.x) {
            const StageSlot s = stage_slot<HD, ROWS, 8>(e, G, pairs, L, H);
            scatter8(T0 + ((size_t)s.g * HD + s.d0) * VS, VS, perm16(s.j), lds16B(R0 + ((size_t)s.g * ROWS + s.j) * KS + s.d0));
        }
        __syncthreads();
        if (active) {
#pragma unroll 1
            for (int qt = 0; qt < NT; ++qt) tile(qt, no{}, yes{});
        }
    }
    if (active && ri < L) {
        float *base = dqkv + ((size_t)b * L + ri) * tok + (size_t)h * HD + 4 * half;
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                *reinterpret_cast<float4 *>(base + (size_t)H * HD + dt * 32 + 8 * r) =
                    make_float4(dk[dt][4 * r] * scale, dk[dt][4 * r + 1] * scale, dk[dt][4 * r + 2] * scale, dk[dt][4 * r + 3] * scale);
                *reinterpret_cast<float4 *>(base + (size_t)2 * H * HD + dt * 32 + 8 * r) =
                    make_float4(dv[dt][4 * r], dv[dt][4 * r + 1], dv[dt][4 * r + 2], dv[dt][4 * r + 3]);
            }
    }
}

struct ForwardTrainBf16 {
    static constexpr const char *what = "vit attention (train bf16)", *kernel_name = "vit_attention_train_bf16_kernel";
    static constexpr size_t lds_bytes(int nt, int hd) { return attention_bf16_lds_bytes(nt, hd, 2); }
    template <int HD, int NT>
    static auto kernel() { return vit_attention_train_bf16_kernel<HD, NT>; }
};
struct BackwardBf16 {
    static constexpr const char *what = "vit attention backward (bf16)", *kernel_name = "vit_attention_bwd_bf16_kernel";
    static constexpr size_t lds_bytes(int nt, int hd) { return attention_bwd_bf16_lds_bytes(nt, hd); }
    template <int HD, int NT>
    static auto kernel() { return vit_attention_bwd_bf16_kernel<HD, NT, attention_bwd_bf16_split(NT, HD)>; }
};

}  // namespace

int launch_attention_train_bf16(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st) {
    return launch_resident<ForwardTrainBf16>(B, L, H, hd, scale, st, qkv, out);
}

int launch_attention_backward_bf16(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L, int H, int hd,
                                   float scale, hipStream_t st) {
    (void)out;   // delta is sum P dP of the kernel's own products, not rowsum(dO * out)
    return launch_resident<BackwardBf16>(B, L, H, hd, scale, st, qkv, dout, dqkv);
}

}  // namespace vit
}  // namespace stgcn
