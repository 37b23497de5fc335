// extern "C" surface of libstgcn_hip.so (declared in include/stgcn_hip.h): argument validation,
// thread-local error text, and dispatch to the kernel launchers.  No allocation, no sync.
#include <stdarg.h>
#include <string.h>

#include "common.h"

namespace stgcn {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int fail(stgcn_status st, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return (int)st;
}

namespace {

__global__ void bn_fold_kernel(const float *__restrict__ w, const float *__restrict__ b,
                               const float *__restrict__ rm, const float *__restrict__ rv,
                               const float *__restrict__ cb, float eps, float *__restrict__ scale,
                               float *__restrict__ shift, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    // same operation order as ATen's CPU batch-norm transform: w / sqrt(var + eps)
    const float s = w[c] / sqrtf(rv[c] + eps);
    const float centre = (cb ? cb[c] : 0.f) - rm[c];
    scale[c] = s;
    shift[c] = fmaf(centre, s, b[c]);
}

// per-rank reductions for the data-parallel harness: stats = [clips, sum(probe), sum(probe^2), correct] with
// probe[n][c] = out[n][c][0][0]; one workgroup, one launch (replaces ~6 tiny torch kernels per step).
// correct = #{n : argmax_c logits[n][c] == labels[n]} — get_acc of SHREC/ST_TS/train_sttran.py:105-109 (np.argmax on the
// host there).  np.argmax semantics: the LOWEST index among equal maxima, and a NaN counts as the maximum (first NaN wins).
__device__ inline int argmax_row(const float *__restrict__ row, int classes) {
    float best = row[0];
    int arg = 0;
    if (best != best) return 0;
    for (int c = 1; c < classes; ++c) {
        const float v = row[c];
        if (v != v) return c;          // NaN: np.argmax / torch.argmax return its index
        if (v > best) { best = v; arg = c; }
    }
    return arg;
}

template <bool BF16>
__global__ __launch_bounds__(256) void step_stats_kernel(const void *__restrict__ out, float *__restrict__ stats,
                                                          int N, int C, size_t clip_stride, size_t chan_stride,
                                                          float n_local,
                                                          const float *__restrict__ logits,
                                                          const long long *__restrict__ labels,
                                                          long long *__restrict__ pred, int n_logits, int classes) {
    __shared__ float red[3][4];
    float s1 = 0.f, s2 = 0.f, hit = 0.f;
    if (out != nullptr)
        for (int e = threadIdx.x; e < N * C; e += 256) {
            const size_t at = (size_t)(e / C) * clip_stride + (size_t)(e % C) * chan_stride;   // element (n, c, 0, 0)
            float v;
            if constexpr (BF16) v = __uint_as_float((unsigned)reinterpret_cast<const unsigned short *>(out)[at] << 16);
            else v = reinterpret_cast<const float *>(out)[at];
            s1 += v;
            s2 = fmaf(v, v, s2);
        }
    if (logits != nullptr)
        for (int n = threadIdx.x; n < n_logits; n += 256) {
            const int a = argmax_row(logits + (size_t)n * classes, classes);
            if (pred != nullptr) pred[n] = a;
            if (labels != nullptr && labels[n] == (long long)a) hit += 1.f;
        }
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o, 64);
        s2 += __shfl_down(s2, o, 64);
        hit += __shfl_down(hit, o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = s1; red[1][w] = s2; red[2][w] = hit; }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[0] = n_local;
        stats[1] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        stats[2] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        stats[3] = red[2][0] + red[2][1] + red[2][2] + red[2][3];   // exact: a count below 2^24
    }
}

}  // namespace

int launch_bn_fold(const float *w, const float *b, const float *rm, const float *rv, const float *cb,
                   float eps, float *scale, float *shift, int C, hipStream_t st) {
    hipLaunchKernelGGL(bn_fold_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, w, b, rm, rv, cb, eps, scale,
                       shift, C);
    STGCN_LAUNCH_CHECK("bn_fold_kernel");
    return STGCN_OK;
}

}  // namespace stgcn

using namespace stgcn;

extern "C" {

int stgcn_version(void) { return STGCN_ABI_VERSION; }

const char *stgcn_last_error(void) { return g_err; }

int stgcn_bn_fold(const float *weight, const float *bias, const float *running_mean,
                  const float *running_var, const float *conv_bias, float eps, float *scale, float *shift,
                  int C, void *stream) {
    REQUIRE_PTR(weight); REQUIRE_PTR(bias); REQUIRE_PTR(running_mean); REQUIRE_PTR(running_var);
    REQUIRE_PTR(scale); REQUIRE_PTR(shift); REQUIRE_POS(C);
    return launch_bn_fold(weight, bias, running_mean, running_var, conv_bias, eps, scale, shift, C,
                          (hipStream_t)stream);
}

// what the three graph-conv forwards check of their attention's arguments before they plan it
#define REQUIRE_ATTENTION_ARGS(P)                                                                                          \
    REQUIRE_PTR(x); REQUIRE_PTR(A_eff); REQUIRE_PTR(Wa); REQUIRE_PTR(ba); REQUIRE_PTR(Wb); REQUIRE_PTR(bb); REQUIRE_PTR(P); \
    REQUIRE_POS(N); REQUIRE_POS(Cin); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(inter_c); REQUIRE_POS(subsets)

int stgcn_agcn_attention(const float *x, const float *A_eff, const float *Wa, const float *ba,
                         const float *Wb, const float *bb, float *P, int N, int Cin, int T, int V,
                         int inter_c, int subsets, void *stream) {
    REQUIRE_ATTENTION_ARGS(P);
    return launch_attention(plan_attention(N, Cin, T, V, inter_c, subsets, AttentionOut{}), AttentionIO{x, false, P}, A_eff, Wa, ba,
                            Wb, bb, (hipStream_t)stream);
}

const char *stgcn_agcn_attention_kernel_name(int N, int Cin, int T, int V, int inter_c, int subsets, int extra) {
    if (N <= 0 || Cin <= 0 || T <= 0 || V <= 0 || inter_c <= 0 || subsets <= 0 || extra < 0 || extra > 3) return "";
    AttentionOut want;
    want.kind = extra == 0 ? AttentionOut::none : extra == 1 ? AttentionOut::features : AttentionOut::frags;
    want.split = extra == 3 ? stem_wide_split(V) : 0;
    return attention_kernel_name(plan_attention(N, Cin, T, V, inter_c, subsets, want));
}

const char *stgcn_agcn_expand_kernel_name(int N, int Cin, int Cout, int T, int V, int subsets, int has_down) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || T <= 0 || V <= 0 || subsets <= 0) return "";
    return expand_kernel_name(plan_agcn_expand(N, Cin, Cout, T, V, subsets, has_down != 0));
}

int stgcn_agcn_forward(const float *x, const float *A_eff, const float *Wa, const float *ba,
                       const float *Wb, const float *bb, const float *Wd, const float *bd,
                       const float *Wdown, const float *bdown, const float *bn_scale,
                       const float *bn_shift, const float *down_scale, const float *down_shift, float *P_ws,
                       float *y, int N, int Cin, int Cout, int T, int V, int inter_c, int subsets,
                       void *stream) {
    REQUIRE_PTR(Wd); REQUIRE_PTR(bd); REQUIRE_PTR(bn_scale); REQUIRE_PTR(bn_shift); REQUIRE_PTR(y);
    REQUIRE_POS(Cout);
    if ((Wdown == nullptr) != (bdown == nullptr) || (Wdown == nullptr) != (down_scale == nullptr) ||
        (Wdown == nullptr) != (down_shift == nullptr))
        return fail(STGCN_ERR_ARG, "agcn_forward: Wdown/bdown/down_scale/down_shift must be all set or all NULL");
    if (Wdown == nullptr && Cin != Cout)
        return fail(STGCN_ERR_ARG, "agcn_forward: identity residual needs Cin == Cout (got %d, %d)", Cin, Cout);
    REQUIRE_ATTENTION_ARGS(P_ws);
    const AttentionPlan at = plan_attention(N, Cin, T, V, inter_c, subsets, AttentionOut{});
    const ExpandPlan ex = plan_agcn_expand(N, Cin, Cout, T, V, subsets, Wdown != nullptr);
    if (at.kernel == AttentionKernel::none) return refused(at.why);     // (both before the first launch: a refused call
    if (ex.kernel == ExpandKernel::none) return refused(ex.why);        //  writes nothing, P included)
    int rc = launch_attention(at, AttentionIO{x, false, P_ws}, A_eff, Wa, ba, Wb, bb, (hipStream_t)stream);
    if (rc != STGCN_OK) return rc;
    return launch_agcn_expand(ex, x, P_ws, Wd, bd, Wdown, bdown, bn_scale, bn_shift, down_scale, down_shift, y, 0,
                              (hipStream_t)stream);
}

size_t stgcn_tcn_packed_bytes(int Cin, int Cout, int K, unsigned flags) {
    if (Cin <= 0 || Cout <= 0 || K <= 0) return 0;
    return plan_tcn_pack(Cin, Cout, K, flags).bytes;
}

int stgcn_tcn_supported(int Cin, int Cout, int T, int V, int K, int stride, unsigned flags) {
    if (Cin <= 0 || Cout <= 0 || T <= 0 || V <= 0 || K <= 0 || stride <= 0) return 0;
    return tcn_on_matrix_cores(plan_tcn(Cin, Cout, T, V, K, stride, flags).kernel) ? 1 : 0;
}

const char *stgcn_tcn_kernel_name(int Cin, int Cout, int T, int V, int K, int stride, unsigned flags) {
    if (Cin <= 0 || Cout <= 0 || T <= 0 || V <= 0 || K <= 0 || stride <= 0) return "";
    return tcn_kernel_name(plan_tcn(Cin, Cout, T, V, K, stride, flags).kernel);
}

int stgcn_stem_supported(int Cin, int C, int T, int V, int K, int subsets, unsigned flags) {
    if (Cin <= 0 || C <= 0 || T <= 0 || V <= 0 || K <= 0 || subsets <= 0) return 0;
    return plan_stem(1, Cin, C, T, V, K, subsets, flags).kernel != StemKernel::none ? 1 : 0;
}

int stgcn_tcn_pack(const float *W, const float *scale, void *Wp, int Cin, int Cout, int K, unsigned flags,
                   void *stream) {
    REQUIRE_PTR(W); REQUIRE_PTR(scale); REQUIRE_PTR(Wp);
    REQUIRE_POS(Cin); REQUIRE_POS(Cout); REQUIRE_POS(K);
    REQUIRE_ALIGNED(Wp, kBlobAlign);
    return launch_tcn_pack(plan_tcn_pack(Cin, Cout, K, flags), W, scale, Wp, Cin, Cout, K, (hipStream_t)stream);
}

int stgcn_tcn_forward_packed(const float *x, const void *Wp, const float *shift, void *y, int N, int Cin,
                             int Cout, int T, int V, int K, int stride, unsigned flags, void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(Wp); REQUIRE_PTR(shift); REQUIRE_PTR(y);
    REQUIRE_POS(N); REQUIRE_POS(Cin); REQUIRE_POS(Cout); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(K);
    REQUIRE_POS(stride);
    REQUIRE_ALIGNED(Wp, kBlobAlign);     // the matrix-core kernels stage it by LDS-DMA
    return launch_tcn(plan_tcn(Cin, Cout, T, V, K, stride, flags), x, Wp, shift, y, N, Cin, Cout, T, V, K, stride, flags,
                      (hipStream_t)stream);
}

int stgcn_tcn_forward(const float *x, const float *W, const float *scale, const float *shift, void *y, int N,
                      int Cin, int Cout, int T, int V, int K, int stride, void *ws, size_t ws_bytes,
                      unsigned flags, void *stream) {
    REQUIRE_PTR(ws);
    REQUIRE_POS(Cin); REQUIRE_POS(Cout); REQUIRE_POS(K);
    REQUIRE_ALIGNED(ws, kBlobAlign);
    const size_t need = plan_tcn_pack(Cin, Cout, K, flags).bytes;
    if (ws_bytes < need)
        return fail(STGCN_ERR_WORKSPACE, "tcn_forward: workspace %zu B < %zu B", ws_bytes, need);
    int rc = stgcn_tcn_pack(W, scale, ws, Cin, Cout, K, flags, stream);
    if (rc != STGCN_OK) return rc;
    return stgcn_tcn_forward_packed(x, ws, shift, y, N, Cin, Cout, T, V, K, stride, flags, stream);
}

size_t stgcn_stem_prep_bytes(int Cin, int C, int K, int subsets, unsigned flags) {
    if (Cin <= 0 || C <= 0 || K <= 0 || subsets <= 0) return 0;
    return plan_stem_prep(C, K, flags).bytes;
}

int stgcn_stem_prepare(const float *Wd, const float *bd, const float *Wdown, const float *bdown,
                       const float *bn_scale, const float *bn_shift, const float *down_scale,
                       const float *down_shift, const float *Wt, const float *t_scale, void *prep, int Cin,
                       int C, int K, int subsets, unsigned flags, void *stream) {
    REQUIRE_PTR(Wd); REQUIRE_PTR(bd); REQUIRE_PTR(Wdown); REQUIRE_PTR(bdown); REQUIRE_PTR(bn_scale);
    REQUIRE_PTR(bn_shift); REQUIRE_PTR(down_scale); REQUIRE_PTR(down_shift); REQUIRE_PTR(Wt);
    REQUIRE_PTR(t_scale); REQUIRE_PTR(prep);
    REQUIRE_POS(Cin); REQUIRE_POS(C); REQUIRE_POS(K); REQUIRE_POS(subsets);
    REQUIRE_ALIGNED(prep, kBlobAlign);
    return launch_stem_prepare(Wd, bd, Wdown, bdown, bn_scale, bn_shift, down_scale, down_shift, Wt, t_scale,
                               prep, Cin, C, K, subsets, flags, (hipStream_t)stream);
}

size_t stgcn_stem_ws_bytes(int N, int Cin, int C, int T, int V, int K, int subsets, unsigned flags) {
    if (N <= 0 || Cin <= 0 || C <= 0 || T <= 0 || V <= 0 || K <= 0 || subsets <= 0) return 0;
    return plan_stem(N, Cin, C, T, V, K, subsets, flags).ws_bytes;
}

const char *stgcn_stem_kernel_name(int Cin, int C, int T, int V, int K, int subsets, unsigned flags) {
    if (Cin <= 0 || C <= 0 || T <= 0 || V <= 0 || K <= 0 || subsets <= 0) return "";
    return stem_kernel_name(plan_stem(1, Cin, C, T, V, K, subsets, flags).kernel);
}

int stgcn_stem_short_tile_blocks(int C, int T, int V, int K) {
    if (C <= 0 || T <= 0 || V <= 0 || K <= 0) return 0;
    return stem_v6_short_tile_blocks(C, T, V, K);
}

int stgcn_stem_walk_run(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *first, int *end) {
    REQUIRE_PTR(first); REQUIRE_PTR(end);
    REQUIRE_POS(num_wg); REQUIRE_POS(nclips); REQUIRE_POS(tiles_per_clip);
    if (wg < 0) return fail(STGCN_ERR_ARG, "%s: wg = %d must not be negative", __func__, wg);
    stem_v6_walk_run(wg, num_wg, nclips, tiles_per_clip, short_last, first, end);
    return STGCN_OK;
}

int stgcn_stem_walk_order(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *tiles, int cap, int *count) {
    REQUIRE_PTR(count);
    REQUIRE_POS(num_wg); REQUIRE_POS(nclips); REQUIRE_POS(tiles_per_clip);
    if (wg < 0) return fail(STGCN_ERR_ARG, "%s: wg = %d must not be negative", __func__, wg);
    if (cap < 0 || (cap > 0 && !tiles)) return fail(STGCN_ERR_ARG, "%s: cap = %d tiles at %p", __func__, cap, (void *)tiles);
    *count = stem_v6_walk_order(wg, num_wg, nclips, tiles_per_clip, short_last, tiles, cap);
    return STGCN_OK;
}

int stgcn_stem_features_used(int Cin, int C, int T, int V, int K, int subsets, unsigned flags) {
    if (Cin <= 0 || C <= 0 || T <= 0 || V <= 0 || K <= 0 || subsets <= 0) return 0;
    const StemPart part = plan_stem(1, Cin, C, T, V, K, subsets, flags).part;
    return part == StemPart::features || part == StemPart::frags ? 1 : 0;
}

int stgcn_stem_attention(const float *x, const float *A_eff, const float *Wa, const float *ba, const float *Wb,
                         const float *bb, void *ws, size_t ws_bytes, int N, int Cin, int C, int T, int V,
                         int inter_c, int subsets, int K, unsigned flags, void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(A_eff); REQUIRE_PTR(Wa); REQUIRE_PTR(ba); REQUIRE_PTR(Wb); REQUIRE_PTR(bb);
    REQUIRE_PTR(ws);
    REQUIRE_POS(N); REQUIRE_POS(Cin); REQUIRE_POS(C); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(inter_c);
    REQUIRE_POS(subsets); REQUIRE_POS(K);
    REQUIRE_ALIGNED(ws, kBlobAlign);     // the fused kernels read its features / fragments by LDS-DMA
    const StemPlan pl = plan_stem(N, Cin, C, T, V, K, subsets, flags);
    if (ws_bytes < pl.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "stem: workspace %zu B < %zu B", ws_bytes, pl.ws_bytes);
    char *w = (char *)ws;
    float *part = (float *)(w + pl.part_off);
    AttentionOut want;
    want.kind = pl.part == StemPart::features ? AttentionOut::features : pl.part == StemPart::frags ? AttentionOut::frags : AttentionOut::none;
    want.split = pl.split, want.bounds = pl.bounds_off != 0;
    const AttentionIO io{x, (flags & STGCN_IN_NTVC) != 0, (float *)ws, pl.part == StemPart::features ? part : nullptr,
                         pl.part == StemPart::frags ? part : nullptr, pl.part == StemPart::xcopy ? part : nullptr,
                         want.bounds ? (float *)(w + pl.bounds_off) : nullptr};
    return launch_attention(plan_attention(N, Cin, T, V, inter_c, subsets, want), io, A_eff, Wa, ba, Wb, bb, (hipStream_t)stream);
}

int stgcn_stem_tail_prepared(const float *x, const void *ws, size_t ws_bytes, const void *prep, const float *t_shift,
                             void *out, int N, int Cin, int C, int T, int V, int subsets, int K, unsigned flags,
                             void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(ws); REQUIRE_PTR(prep); REQUIRE_PTR(t_shift); REQUIRE_PTR(out);
    REQUIRE_POS(N); REQUIRE_POS(Cin); REQUIRE_POS(C); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(subsets);
    REQUIRE_POS(K);
    REQUIRE_ALIGNED(ws, kBlobAlign); REQUIRE_ALIGNED(prep, kBlobAlign);
    const StemPlan pl = plan_stem(N, Cin, C, T, V, K, subsets, flags);
    if (ws_bytes < pl.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "stem: workspace %zu B < %zu B", ws_bytes, pl.ws_bytes);
    return launch_stem(pl, x, ws, prep, t_shift, out, N, Cin, C, T, V, subsets, K, flags, (hipStream_t)stream);
}

int stgcn_stem_forward_prepared(const float *x, const float *A_eff, const float *Wa, const float *ba,
                                const float *Wb, const float *bb, const void *prep, const float *t_shift, void *ws,
                                size_t ws_bytes, void *out, int N, int Cin, int C, int T, int V, int inter_c,
                                int subsets, int K, unsigned flags, void *stream) {
    REQUIRE_PTR(prep); REQUIRE_PTR(t_shift); REQUIRE_PTR(out);      // (what the tail would refuse, before the attention writes)
    REQUIRE_ALIGNED(prep, kBlobAlign);
    int rc = stgcn_stem_attention(x, A_eff, Wa, ba, Wb, bb, ws, ws_bytes, N, Cin, C, T, V, inter_c, subsets, K, flags,
                                  stream);
    if (rc != STGCN_OK) return rc;
    return stgcn_stem_tail_prepared(x, ws, ws_bytes, prep, t_shift, out, N, Cin, C, T, V, subsets, K, flags, stream);
}

// ---- training entry points: each reads one plan (common.h) for its path and its workspace ---------------------------
// materialise != 0: room for the two pre-BatchNorm branches (needed when they are to be saved, or for shapes the
// moments path does not cover); 0: the moments path's scratch only
size_t stgcn_agcn_train_ws_bytes(int N, int Cin, int Cout, int T, int V, int subsets, int materialise) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || T <= 0 || V <= 0 || subsets <= 0) return 0;
    return plan_agcn_train(N, Cin, Cout, T, V, subsets, materialise != 0, true, false).ws_bytes;
}

int stgcn_agcn_forward_train(const float *x, const float *A_eff, const float *Wa, const float *ba, const float *Wb,
                             const float *bb, const float *Wd, const float *bd, const float *Wdown,
                             const float *bdown, const float *bn_weight, const float *bn_bias, float *bn_running_mean,
                             float *bn_running_var, const float *dbn_weight, const float *dbn_bias,
                             float *dbn_running_mean, float *dbn_running_var, float momentum, float eps, float *P_ws,
                             void *ws, size_t ws_bytes, float *y, float *save_zm, float *save_zd, float *save_stats,
                             int N, int Cin, int Cout, int T, int V, int inter_c, int subsets, unsigned flags, void *stream) {
    REQUIRE_PTR(Wd); REQUIRE_PTR(bd); REQUIRE_PTR(bn_weight); REQUIRE_PTR(bn_bias); REQUIRE_PTR(bn_running_mean);
    REQUIRE_PTR(bn_running_var); REQUIRE_PTR(ws); REQUIRE_PTR(y); REQUIRE_POS(Cout);
    REQUIRE_ALIGNED(ws, kBlobAlign);     // fp64 atomic sums
    REQUIRE_ALIGNED(save_stats, 8);      // the 63 feature moments are doubles
    const bool has_down = Wdown != nullptr;
    if (has_down && (!bdown || !dbn_weight || !dbn_bias || !dbn_running_mean || !dbn_running_var))
        return fail(STGCN_ERR_ARG, "agcn_forward_train: down branch given without its bias / BatchNorm tensors");
    if (!has_down && Cin != Cout)
        return fail(STGCN_ERR_ARG, "agcn_forward_train: identity residual needs Cin == Cout (got %d, %d)", Cin, Cout);
    REQUIRE_ATTENTION_ARGS(P_ws);
    const bool frozen = (flags & STGCN_BN_FROZEN) != 0;     // running statistics: the branches are materialised
    const AgcnTrainPlan pl = plan_agcn_train(N, Cin, Cout, T, V, subsets, frozen || !has_down || save_zm || save_zd, has_down, frozen);
    // (before the attention launch: a refused call writes nothing, P included)
    if (ws_bytes < pl.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "agcn_forward_train: workspace %zu B too small", ws_bytes);
    const AttentionPlan at = plan_attention(N, Cin, T, V, inter_c, subsets, AttentionOut{});
    if (at.kernel == AttentionKernel::none) return refused(at.why);
    if (pl.main.kernel == ExpandKernel::none) return refused(pl.main.why);
    int rc = launch_attention(at, AttentionIO{x, false, P_ws}, A_eff, Wa, ba, Wb, bb, (hipStream_t)stream);
    if (rc != STGCN_OK) return rc;
    return launch_agcn_forward_train(pl, x, P_ws, Wd, bd, Wdown, bdown, bn_weight, bn_bias, bn_running_mean, bn_running_var,
                                     dbn_weight, dbn_bias, dbn_running_mean, dbn_running_var, momentum, eps, ws, y, save_zm,
                                     save_zd, save_stats, N, Cin, Cout, T, V, subsets, (hipStream_t)stream);
}

// recompute: bit 0 = the two pre-BatchNorm branches are not supplied (rebuilt in the workspace); bit 1 = size for the
// generic path (input gradient wanted / identity residual / a shape outside the stem class).  Never 0 for valid sizes.
size_t stgcn_agcn_backward_ws_bytes(int N, int Cin, int Cout, int T, int V, int subsets, int recompute) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || T <= 0 || V <= 0 || subsets <= 0) return 0;
    return plan_agcn_backward(N, Cin, Cout, T, V, subsets, (recompute & 1) != 0, (recompute & 2) != 0, true, false).ws_bytes;
}

int stgcn_agcn_backward_train(const float *x, const float *A_eff, const float *Wa, const float *ba, const float *Wb,
                              const float *bb, const float *Wd, const float *bd, const float *Wdown, const float *bdown,
                              const float *P, const float *zm, const float *zd, const float *bn_weight,
                              const float *bn_bias, const float *dbn_weight, const float *dbn_bias,
                              const float *save_stats, const float *y, const float *dy, float *dWa, float *dba, float *dWb,
                              float *dbb,
                              float *dWd, float *dbd, float *dWdown, float *dbdown, float *dgamma, float *dbeta,
                              float *ddgamma, float *ddbeta, float *dPA, float *dx, void *ws, size_t ws_bytes, int N, int Cin,
                              int Cout, int T, int V, int inter_c, int subsets, unsigned flags, void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(A_eff); REQUIRE_PTR(Wa); REQUIRE_PTR(ba); REQUIRE_PTR(Wb); REQUIRE_PTR(bb); REQUIRE_PTR(Wd);
    REQUIRE_PTR(bd); REQUIRE_PTR(P); REQUIRE_PTR(bn_weight); REQUIRE_PTR(bn_bias);
    REQUIRE_PTR(save_stats); REQUIRE_PTR(dy); REQUIRE_PTR(dWa); REQUIRE_PTR(dba);
    REQUIRE_PTR(dWb); REQUIRE_PTR(dbb); REQUIRE_PTR(dWd); REQUIRE_PTR(dbd);
    REQUIRE_PTR(dgamma); REQUIRE_PTR(dbeta); REQUIRE_PTR(dPA); REQUIRE_PTR(ws);
    REQUIRE_POS(N); REQUIRE_POS(Cin); REQUIRE_POS(Cout); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(inter_c); REQUIRE_POS(subsets);
    REQUIRE_ALIGNED(ws, kBlobAlign); REQUIRE_ALIGNED(save_stats, 8);
    const bool has_down = Wdown != nullptr;
    if (has_down) {
        REQUIRE_PTR(bdown); REQUIRE_PTR(dbn_weight); REQUIRE_PTR(dbn_bias); REQUIRE_PTR(dWdown); REQUIRE_PTR(dbdown);
        REQUIRE_PTR(ddgamma); REQUIRE_PTR(ddbeta);
    } else if (Cin != Cout) {
        return fail(STGCN_ERR_ARG, "agcn_backward: identity residual needs Cin == Cout (got %d, %d)", Cin, Cout);
    }
    if (V > kAttentionMaxV) return fail(STGCN_ERR_UNSUPPORTED, "agcn_backward: V=%d > %d", V, kAttentionMaxV);
    if (N > kMaxGridClips) return fail(STGCN_ERR_UNSUPPORTED, "agcn_backward: N=%d > %d clips per call", N, kMaxGridClips);
    // the moment form wants what a moments-path forward leaves (no saved branches, the output y, the moments), batch
    // statistics, a down branch and no input gradient
    const bool frozen = (flags & STGCN_BN_FROZEN) != 0;
    const bool generic = frozen || !has_down || dx != nullptr || zm != nullptr || y == nullptr;
    const AgcnBackwardPlan pl = plan_agcn_backward(N, Cin, Cout, T, V, subsets, zm == nullptr, generic, has_down, frozen);
    // the GEMM chain runs one batch entry per (clip, subset) pair on a 16-bit grid axis: refuse here, not at its first
    // product - the expansion and the BatchNorm gradient have been launched by then
    if (!pl.fused && (long long)N * subsets > kMaxGridClips)
        return fail(STGCN_ERR_UNSUPPORTED, "agcn_backward: the GEMM chain covers N * subsets <= %d (N=%d, %d subsets)", kMaxGridClips,
                    N, subsets);
    if (!pl.fused && inter_c > pl.inter_c_max)
        return fail(STGCN_ERR_UNSUPPORTED, "agcn_backward: inter_c=%d > Cout/4 (workspace is sized for coff_embedding >= 4)", inter_c);
    if (has_down ? ((zm == nullptr) != (zd == nullptr)) : (zd != nullptr))
        return fail(STGCN_ERR_ARG, "agcn_backward: give both saved branches or neither (zd only with a down branch)");
    if (ws_bytes < pl.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "agcn_backward: workspace %zu B < %zu B", ws_bytes, pl.ws_bytes);
    if (pl.recompute && pl.expand.kernel == ExpandKernel::none) return refused(pl.expand.why);
    return launch_agcn_backward_train(pl, x, A_eff, Wa, ba, Wb, bb, Wd, bd, Wdown, bdown, P, zm, zd, bn_weight, bn_bias, dbn_weight,
                                      dbn_bias, save_stats, y, dy, dWa, dba, dWb, dbb, dWd, dbd, dWdown, dbdown, dgamma, dbeta,
                                      ddgamma, ddbeta, dPA, dx, ws, N, Cin, Cout, T, V, inter_c, subsets, (hipStream_t)stream);
}

size_t stgcn_tcn_train_ws_bytes(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || T <= 0 || V <= 0 || K <= 0 || stride <= 0) return 0;
    return plan_tcn_train(N, Cin, Cout, T, V, K, stride, flags).ws_bytes;
}

int stgcn_tcn_forward_train(const float *x, const float *W, const float *conv_bias, const float *bn_weight,
                            const float *bn_bias, float *bn_running_mean, float *bn_running_var, float momentum,
                            float eps, void *ws, size_t ws_bytes, float *y, float *save_z, float *save_mean,
                            float *save_invstd, int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags,
                            void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(W); REQUIRE_PTR(bn_weight); REQUIRE_PTR(bn_bias); REQUIRE_PTR(bn_running_mean);
    REQUIRE_PTR(bn_running_var); REQUIRE_PTR(ws); REQUIRE_PTR(y);
    REQUIRE_POS(N); REQUIRE_POS(Cin); REQUIRE_POS(Cout); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(K); REQUIRE_POS(stride);
    REQUIRE_ALIGNED(ws, kBlobAlign);     // packed weights (LDS-DMA) and fp64 atomic sums
    const TcnTrainPlan pl = plan_tcn_train(N, Cin, Cout, T, V, K, stride, flags);
    if (pl.ws_bytes == 0) return fail(STGCN_ERR_ARG, "tcn_forward_train: T=%d K=%d stride=%d gives no output frame", T, K, stride);
    if (ws_bytes < pl.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "tcn_forward_train: workspace %zu B < %zu B", ws_bytes, pl.ws_bytes);
    if (flags & STGCN_OUT_BF16) return fail(STGCN_ERR_UNSUPPORTED, "tcn_forward_train: fp32 output only");
    return launch_tcn_forward_train(pl, x, W, conv_bias, bn_weight, bn_bias, bn_running_mean, bn_running_var, momentum, eps, ws, y,
                                    save_z, save_mean, save_invstd, N, Cin, Cout, T, V, K, stride, (hipStream_t)stream);
}

size_t stgcn_tcn_backward_ws_bytes(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || T <= 0 || V <= 0 || K <= 0 || stride <= 0) return 0;
    return plan_tcn_backward(N, Cin, Cout, T, V, K, stride, flags).ws_bytes;
}

int stgcn_tcn_backward_train(const float *x, const float *W, const float *z, const float *bn_weight,
                             const float *bn_bias, const float *save_mean, const float *save_invstd, const float *dy,
                             float *dx, float *dW, float *dbias, float *dgamma, float *dbeta, void *ws, size_t ws_bytes,
                             int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags, void *stream) {
    REQUIRE_PTR(x); REQUIRE_PTR(W); REQUIRE_PTR(z); REQUIRE_PTR(bn_weight); REQUIRE_PTR(bn_bias); REQUIRE_PTR(save_mean);
    REQUIRE_PTR(save_invstd); REQUIRE_PTR(dy); REQUIRE_PTR(dW); REQUIRE_PTR(dgamma); REQUIRE_PTR(dbeta); REQUIRE_PTR(ws);
    REQUIRE_POS(N); REQUIRE_POS(Cin); REQUIRE_POS(Cout); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(K); REQUIRE_POS(stride);
    REQUIRE_ALIGNED(ws, kBlobAlign);
    const TcnBackwardPlan pl = plan_tcn_backward(N, Cin, Cout, T, V, K, stride, flags);
    if (pl.ws_bytes == 0) return fail(STGCN_ERR_ARG, "tcn_backward: T=%d K=%d stride=%d gives no output frame", T, K, stride);
    if (ws_bytes < pl.ws_bytes) return fail(STGCN_ERR_WORKSPACE, "tcn_backward: workspace %zu B < %zu B", ws_bytes, pl.ws_bytes);
    if (N > 65535) return fail(STGCN_ERR_UNSUPPORTED, "tcn_backward: N=%d > 65535 clips per call", N);
    return launch_tcn_backward_train(pl, x, W, z, bn_weight, bn_bias, save_mean, save_invstd, dy, dx, dW, dbias, dgamma, dbeta, ws,
                                     N, Cin, Cout, T, V, K, (hipStream_t)stream);
}

int stgcn_patch_embed(const float *z, const float *W, const float *b, const float *pos, float *out, int N, int C, int E,
                      int T, int V, unsigned flags, void *stream) {
    REQUIRE_PTR(z); REQUIRE_PTR(W); REQUIRE_PTR(b); REQUIRE_PTR(out);
    REQUIRE_POS(N); REQUIRE_POS(C); REQUIRE_POS(E); REQUIRE_POS(T); REQUIRE_POS(V);
    if (flags & ~(STGCN_IN_NTVC | STGCN_EMBED_TS)) return fail(STGCN_ERR_ARG, "patch_embed: unknown flag bits 0x%x", flags);
    if (N > 65535) return fail(STGCN_ERR_UNSUPPORTED, "patch_embed: N=%d > 65535 clips per call", N);
    return launch_patch_embed(z, W, b, pos, out, N, C, E, T, V, flags, (hipStream_t)stream);
}

int stgcn_step_stats(const void *out, int out_is_bf16, float *stats, int N, int C, long clip_stride, long chan_stride,
                     float n_local,
                     const float *logits, const long long *labels, long long *pred, int n_logits, int classes,
                     void *stream) {
    REQUIRE_PTR(stats);
    if (out != nullptr) { REQUIRE_POS(N); REQUIRE_POS(C); REQUIRE_POS(clip_stride); REQUIRE_POS(chan_stride); }
    if (logits != nullptr) {
        REQUIRE_POS(n_logits); REQUIRE_POS(classes);
        if (n_logits >= (1 << 24)) return fail(STGCN_ERR_UNSUPPORTED, "step_stats: %d rows of logits per call", n_logits);
    } else if (labels != nullptr || pred != nullptr) {
        return fail(STGCN_ERR_ARG, "step_stats: labels / pred given without logits");
    }
    if (out == nullptr && logits == nullptr) return fail(STGCN_ERR_ARG, "step_stats: neither out nor logits given");
    if (out_is_bf16)
        hipLaunchKernelGGL(step_stats_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, out, stats, N, C,
                           (size_t)clip_stride, (size_t)chan_stride, n_local, logits, labels, pred, n_logits, classes);
    else
        hipLaunchKernelGGL(step_stats_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, out, stats, N, C,
                           (size_t)clip_stride, (size_t)chan_stride, n_local, logits, labels, pred, n_logits, classes);
    STGCN_LAUNCH_CHECK("step_stats_kernel");
    return STGCN_OK;
}

}  // extern "C"
