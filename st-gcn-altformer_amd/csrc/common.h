// Shared host/device helpers for libstgcn_hip (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/stgcn_hip.h"

// save_stats[4*Cout + 126] (one of the two spare floats behind the 63 moment doubles): written by the moments-path forward,
// cleared by the materialising path, checked by the moment-form backward (which poisons its outputs with NaN without it).
#define STGCN_MOMENTS_MAGIC 0x4D4F4D31u   /* "MOM1" */
#define STGCN_MOMENTS_MARK_SLOT(Cout) (4 * (Cout) + 126)

namespace stgcn {

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kLdsBytes = 160 * 1024;  // LDS per CU (and max per workgroup) on gfx950

// thread-local last-error text (stgcn_last_error)
void set_error(const char *fmt, ...);
int fail(stgcn_status st, const char *fmt, ...);

#define STGCN_HIP_CHECK(expr)                                                              \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            return stgcn::fail(STGCN_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

#define STGCN_LAUNCH_CHECK(name)                                                           \
    do {                                                                                   \
        hipError_t _e = hipGetLastError();                                                 \
        if (_e != hipSuccess)                                                              \
            return stgcn::fail(STGCN_ERR_HIP, "launch of %s failed: %s", name,             \
                               hipGetErrorString(_e));                                     \
    } while (0)

// argument checks of the extern "C" entry points
#define REQUIRE_PTR(p)                                                                     \
    do {                                                                                   \
        if ((p) == nullptr) return stgcn::fail(STGCN_ERR_ARG, "%s: %s is NULL", __func__, #p); \
    } while (0)
#define REQUIRE_POS(v)                                                                     \
    do {                                                                                   \
        if ((v) <= 0) return stgcn::fail(STGCN_ERR_ARG, "%s: %s = %d must be positive", __func__, #v, (int)(v)); \
    } while (0)

// The alignment contract (include/stgcn_hip.h, "Alignment"): a blob or workspace that is an LDS-DMA source or the target of an
// fp64 atomic is refused off 256 bytes, an operand an entry point lists by name off its listed demand; NULL (an optional
// operand) passes.  Before anything is launched, and the message names the operand.
static inline bool aligned_to(const void *p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
constexpr int kBlobAlign = 256;
#define REQUIRE_ALIGNED(p, bytes)                                                          \
    do {                                                                                   \
        if (!stgcn::aligned_to((p), (bytes)))                                              \
            return stgcn::fail(STGCN_ERR_ARG, "%s: %s must be %d-byte aligned", __func__, #p, (int)(bytes)); \
    } while (0)

// phases switched off by a diagnostic build (see tcn_conv.hip); always 0 in the shipped library
// kernel option bits that travel in the high half of the kernels' `abl` argument (the low half is the ablation mask)
constexpr int OPT_OUT_NTVC = 1 << 16;  // store the output as (N,T,V,C) instead of (N,C,T,V)

static inline int ablate_mask() {
#ifdef STGCN_ABLATION
    const char *e = getenv("STGCN_ABLATE");
    return e ? atoi(e) : 0;
#else
    return 0;
#endif
}

// diagnostic builds: device buffer for in-kernel cycle stamps (address in env STGCN_DBG_PTR), else NULL
static inline unsigned long long *debug_buffer() {
#ifdef STGCN_ABLATION
    const char *e = getenv("STGCN_DBG_PTR");
    return e ? reinterpret_cast<unsigned long long *>(strtoull(e, nullptr, 0)) : nullptr;
#else
    return nullptr;
#endif
}

// max(x, lo) that keeps a NaN (torch.relu's rule): one v_maximum3_f32 on gfx950.  fmaxf and v_max_f32 return the operand that
// is not a NaN, so a ReLU written with them stores a NaN pre-activation as 0 (as -inf in the raw mode, lo = -inf).  Every
// ReLU, raw-mode clamp and max-pool of the library goes through here; lo = -inf returns x unchanged.  On finite inputs the
// result differs from fmaxf's in nothing but the sign of a zero (max_nan(-0, +0) = +0).
__device__ __forceinline__ float max_nan(float x, float lo) { return __builtin_elementwise_maximum(x, lo); }

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// Workspace carving.  A layout is written once, as a function that takes pieces from a Carve in order: run on a NULL base it
// sizes the workspace (`off` is the total, every piece NULL), run on the caller's pointer it places the pieces.
struct Carve {
    char *p;
    size_t off = 0;
    explicit Carve(void *base) : p((char *)base) {}
    template <typename T>
    T *take(size_t n, size_t align = 256) {        // n elements; the piece occupies a multiple of `align` bytes
        T *r = p ? reinterpret_cast<T *>(p + off) : nullptr;
        off += align_up(n * sizeof(T), align);
        return r;
    }
    template <typename T>
    T *packed(size_t n) { return take<T>(n, sizeof(T)); }   // no padding behind the piece (blocks of small vectors)
    void pad(size_t align = 256) { off = align_up(off, align); }
};

// output frames of the temporal conv: pad (K-1)/2 on both sides (an even K drops a frame at stride 1)
static inline int tcn_out_frames(int T, int K, int stride) { return (T + 2 * ((K - 1) / 2) - K) / stride + 1; }

// Opt a kernel in to more than 64 KiB of dynamic LDS.
template <typename K>
static inline hipError_t allow_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// A launch carries its size along an axis in work-items, a 32-bit number: gridDim.x * blockDim.x must stay below 2^32.  This
// runtime does not reject a larger one: it runs the product modulo 2^32, and the workgroups past it never start (22.4 M
// workgroups of 256 threads of the streaming attention left three quarters of their result unwritten: DESIGN, "Large
// extents").  Every launch whose grid grows with the batch asks this before it goes; 2^31 - 1 workgroups bound nothing.
static inline bool grid_fits(long long blocks, int threads) { return blocks >= 0 && blocks * threads <= 0xffffffffLL; }

// Iteration shared by the elementwise kernels: workgroup (blockIdx.x, c = blockIdx.y) owns clips
// [n_lo, n_hi) of channel c; a clip's plane of the channel is contiguous, so there is no division in the loop and,
// when the plane is a multiple of 4 floats, every access is a 16-byte one.
struct ChannelRows {
    int n_lo, n_hi;
    bool vec;
    __device__ ChannelRows(int N, size_t plane) {
        const int per = (N + (int)gridDim.x - 1) / (int)gridDim.x;
        n_lo = blockIdx.x * per;
        n_hi = min(N, n_lo + per);
        vec = (plane & 3) == 0;
    }
};

// grid.x of those kernels: ~64 K elements per workgroup and channel, at most one workgroup per clip; tensors too small to
// give a thousand workgroups that way (the deeper layers' 64-clip steps: 64 - 128 workgroups of 256 threads for the whole
// chip, 0.5 TB/s) are cut finer, down to 8 K elements per workgroup and channel.
static inline int bn_chunks(int N, size_t plane, int C = 0) {
    int chunks = (int)(((size_t)N * plane + 65535) / 65536);
    if (C > 0 && chunks * C < 1024) {
        const int fine = (int)(((size_t)N * plane + 8191) / 8192);
        chunks = (1024 + C - 1) / C;
        if (chunks > fine) chunks = fine;
    }
    if (chunks > N) chunks = N;
    if (chunks > 64) chunks = 64;
    return chunks < 1 ? 1 : chunks;
}
// ... and their grid.y: the channel rides on a 16-bit axis.  Asked by every launcher of them (train_bn.hip, tcn_backward.hip)
static inline bool bn_rows_fit(int N, int C) { return N >= 1 && C >= 1 && C <= 65535; }

// ---------------------------------------------------------------------------------------
// launchers implemented in the kernel translation units (all enqueue on `st`, return status)
// ---------------------------------------------------------------------------------------
int launch_bn_fold(const float *w, const float *b, const float *rm, const float *rv,
                   const float *cb, float eps, float *scale, float *shift, int C, hipStream_t st);

// graph conv forward (unit_agcn): the plans every entry point reads (agcn.hip) — which kernel and instantiation serve a
// shape, its launch geometry and, where none does, the status and text of the refusal
constexpr int kMaxGridClips = 65535;   // the clip index rides in a 16-bit grid dimension
constexpr int kAttentionMaxV = 64;     // joints the attention kernels (and with them the graph conv) cover
static inline bool agcn_stem_class(int Cin, int S) { return Cin == 3 && S == 3; }   // what the folded forms are written for
struct Refusal { stgcn_status status = STGCN_OK; char msg[160] = ""; };   // of a plan whose kernel is `none`
static inline int refused(const Refusal &r) { return fail(r.status, "%s", r.msg); }

enum class AttentionKernel { none, folded, generic_mfma, generic_valu };
struct AttentionOut {                  // what a call produces besides P
    enum Kind { none, features, frags } kind = none;   // features: (N, T*V, 16); frags: P as bf16 hi/lo MFMA B fragments
    int split = 0;                     // frags of wide frames: (N,48,64) x 16 B for the joint split V0 | V - V0, else (N,12,64)
    bool bounds = false;               // (N,4): max|x| and max|x| * largest column abs-sum of P_s per clip (KF7's scales)
};
struct AttentionTile {                 // the chosen kernel's geometry: written by its *_covers, read by launch_attention
    int maxb = 0, nw = 0, ks = 0, mb = 0, maxit = 0;   // folded<MAXB,NW>, generic_mfma<KS,MAXB>, generic_valu<MAXIT>
    int TC = 0, pitch = 0, slice_off = 0, sq_behind = 0, gx = 0, gy = 0;
    size_t lds = 0;
};
struct AttentionPlan {
    AttentionKernel kernel = AttentionKernel::none;
    AttentionTile tile;
    AttentionOut out;
    int N = 0, Cin = 0, T = 0, V = 0, inter_c = 0, S = 0;
    Refusal why;
};
AttentionPlan plan_attention(int N, int Cin, int T, int V, int inter_c, int S, AttentionOut want);
const char *attention_kernel_name(const AttentionPlan &p);   // with its template arguments; "" for none
bool attention_emits_features(int Cin, int V, int S);
struct AttentionIO {                   // x is (N,Cin,T,V), or (N,T,V,Cin) with x_ntvc; the outputs AttentionOut names, or NULL;
    const float *x;                    // xcopy (optional): channel-major copy of x for kernels downstream
    bool x_ntvc;
    float *P, *feat = nullptr;
    void *pfrag = nullptr;
    float *xcopy = nullptr, *ybound = nullptr;
};
// its kernels (agcn_attention.hip): one coverage predicate each, called by plan_attention only, and the launcher
bool attention_folded_covers(int N, int Cin, int T, int V, int inter_c, int S, bool features, AttentionTile &t);
bool attention_generic_mfma_covers(int N, int Cin, int T, int V, int inter_c, int S, AttentionTile &t);
bool attention_generic_valu_covers(int N, int Cin, int T, int V, int inter_c, int S, AttentionTile &t);
int launch_attention(const AttentionPlan &p, const AttentionIO &io, const float *A_eff, const float *Wa, const float *ba,
                     const float *Wb, const float *bb, hipStream_t st);

enum class ExpandKernel { none, small4, small, mfma, generic };
struct ExpandTile { int now = 0, npb = 0, TF = 0, gx = 0, gy = 0; size_t lds = 0; };   // mfma<NOW,NPB>
struct ExpandPlan {
    ExpandKernel kernel = ExpandKernel::none;
    ExpandTile tile;
    int N = 0, Cin = 0, Cout = 0, T = 0, V = 0, S = 0;
    Refusal why;
};
ExpandPlan plan_agcn_expand(int N, int Cin, int Cout, int T, int V, int S, bool has_down);
const char *expand_kernel_name(const ExpandPlan &p);
constexpr int EXPAND_RAW = 1;           // `mode` of the expansion: no ReLU (the pre-activation value) ...
constexpr int EXPAND_NO_RESIDUAL = 2;   // ... and the identity residual left out
// its kernels (agcn_expand.hip), as above; has_down (Wdown is given) only decides between the folded forms and the rest
bool agcn_expand_small4_covers(int N, int Cin, int Cout, int T, int V, int S, bool has_down, ExpandTile &t);
bool agcn_expand_small_covers(int N, int Cin, int Cout, int T, int V, int S, bool has_down, ExpandTile &t);
bool agcn_expand_mfma_covers(int N, int Cin, int Cout, int T, int V, int S, ExpandTile &t);
bool agcn_expand_generic_covers(int N, int Cin, int T, int V, int S, ExpandTile &t);
int launch_agcn_expand(const ExpandPlan &p, const float *x, const float *P, const float *Wd, const float *bd,
                       const float *Wdown, const float *bdown, const float *bn_scale, const float *bn_shift,
                       const float *down_scale, const float *down_shift, float *y, int mode, hipStream_t st);

// temporal conv (Unit2D): the plan every entry point reads (tcn.hip; the packed blob's layout is described there)
enum class TcnKernel { none, valu, valu_joint_axis, mfma_f32, bf16_small, v4, v6 };
enum class TcnLayout { none, valu, f32_frags, bf16 };
struct TcnPack {   // depends on (Cin, Cout, K, math) only.  bytes: all of it; single: the first layout alone; pairs: offset of the
    TcnLayout layout = TcnLayout::none;                                                     // pair-order copy (0: it has none)
    size_t bytes = 0, single = 0, pairs = 0;
};
struct TcnTile { int rows = 0, n = 0; size_t lds = 0; };   // the chosen kernel's tile: written by its *_covers, read by its launch
struct TcnPlan {
    TcnKernel kernel = TcnKernel::none;
    TcnPack pack;
    TcnTile tile;
    int Tout = 0;                    // output frames (joint axis: T)
    bool stats_in_conv_ok = false;   // launch_tcn may be given `stats`
};
TcnPack plan_tcn_pack(int Cin, int Cout, int K, unsigned flags);
TcnPlan plan_tcn(int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
static inline bool tcn_on_matrix_cores(TcnKernel k) { return k >= TcnKernel::mfma_f32; }
const char *tcn_kernel_name(TcnKernel k);
int launch_tcn_pack(const TcnPack &p, const float *W, const float *scale, void *Wp, int Cin, int Cout, int K, hipStream_t st);
// stats (optional, 2*Cout doubles ZEROED by the caller): per-channel sum and sum of squares of the stored output
int launch_tcn(const TcnPlan &p, const float *x, const void *Wp, const float *shift, void *y, int N, int Cin, int Cout, int T,
               int V, int K, int stride, unsigned flags, hipStream_t st, double *stats = nullptr);
// its kernels, one coverage predicate and one launcher each (the predicates are called by plan_tcn[_pack] only): VALU and f32
// matrix cores (tcn_conv.hip) ...
int launch_tcn_pack_f32(bool frags, const float *W, const float *scale, void *Wp, int Cin, int Cout, int K, hipStream_t st);
int launch_tcn_valu(bool joint_axis, const float *x, const void *Wp, const float *shift, void *y, int N, int Cin, int Cout, int T,
                    int V, int K, int stride, int Lout, unsigned flags, hipStream_t st);
bool tcn_mfma_f32_covers(int Cin, int Cout, int V, int K, int stride, int Tout, TcnTile &t);
int launch_tcn_mfma_f32(const TcnTile &t, const float *x, const void *Wp, const float *shift, void *y, int N, int Cin, int Cout,
                        int T, int V, int K, int stride, int Tout, unsigned flags, hipStream_t st);
// ... the 128-pixel tile on the bf16 matrix cores (tcn_bf16.hip) ...
int launch_tcn_pack_bf16(const float *W, const float *scale, void *Wp, int Cin, int Cout, int K, hipStream_t st);
bool tcn_bf16_small_covers(int Cin, int Cout, int V, int K, int stride, int Tout, int terms, TcnTile &t);
int launch_tcn_bf16_small(const TcnTile &t, const float *x, const void *Wp, const float *shift, void *y, int N, int Cin, int Cout,
                          int T, int V, int K, int stride, int Tout, unsigned flags, hipStream_t st);
// ... the large-tile persistent form (stem_bf16_v4.hip): K = 9, stride 1 ...
bool tcn_v4_covers(int Cin, int Cout, int T, int V, int K, int stride, int terms, TcnTile &t);
int launch_tcn_v4(const TcnTile &t, const float *x, const void *Wp, const float *shift, void *y, int N, int Cin, int Cout, int T,
                  int V, unsigned flags, hipStream_t st);
// ... and the same in KF6's form (tcn_bf16_v6.hip): one wave per SIMD, on the pair-order copy of the weights
bool tcn_v6_takes_weights(int Cin, int Cout, int K);   // the blob carries the pair-order copy
bool tcn_v6_covers(int Cin, int Cout, int T, int V, int K, int stride, int terms, TcnTile &t, bool &stats_ok);
int launch_tcn_pack_pairs_padded(const float *W, const float *scale, void *Wq, int Cin, int Cout, hipStream_t st);
int launch_tcn_v6(const TcnTile &t, const float *x, const void *Wq, const float *shift, void *y, int N, int Cin, int Cout, int T,
                  int V, unsigned flags, hipStream_t st, double *stats = nullptr);

// the 128-pixel fused stem on the bf16 matrix cores: reads x (channel-major) and P, computes the features per tile
bool stem_bf16_small_supported(int C, int T, int V, int K, unsigned flags);
int launch_stem_bf16_small(const float *x, const float *P, const float *W12, const void *Wp, const float *shift, void *out, int N,
                           int C, int T, int V, int K, unsigned flags, hipStream_t st);

// large-tile persistent bf16 stem, eight waves (stem_bf16_v4.hip); *frags: the 256-pixel tile (features from fragments)
bool stem_v4_supported(int Cin, int C, int T, int V, int K, int S, unsigned flags, bool *frags = nullptr);
int launch_stem_v4(const float *x, bool x_ntvc, const float *feat, const void *prep_w12, const void *Wp, const float *shift,
                   void *out, int N, int C, int T, int V, int K, unsigned flags, hipStream_t st);  // honours STGCN_OUT_NTVC

// the same tile with ONE WAVE PER SIMD on v_mfma_f32_16x16x32_bf16 (kernel in kf6.h, narrow form instantiated by
// stem_bf16_v6.hip: 256 threads, a wave owns all 128 channels of 64 pixels), on pair-order temporal weights
bool stem_v6_supported(int C, int T, int V, int K, unsigned flags);
// KF6's narrow three-term form (kf6.h): blocks the short form of a clip's last tile reads (0: the shape has none), and the run
// [first, end) of tiles that workgroup wg of num_wg walks
int stem_v6_short_tile_blocks(int C, int T, int V, int K);
void stem_v6_walk_run(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *first, int *end);
int stem_v6_walk_order(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *tiles, int cap);
// ... and for wide frames (32 < V <= 64, V even: the two-hand graph) the same kernel over the two joint halves [0, V0) and
// [V0, V), each handled like a narrow clip (stem_bf16_v6w.hip)
static inline int stem_wide_split(int V) {     // V0 (a multiple of 4: 16-byte aligned half rows), or 0 when V does not split
    if (V <= 32 || V > 64 || (V & 1)) return 0;
    const int v0 = (V / 2 + 3) / 4 * 4;
    return (v0 <= 32 && V - v0 >= 1) ? v0 : 0;
}
bool stem_v6w_supported(int C, int T, int V, int K, unsigned flags);
// ... and KF7 (stem_f16mx.hip, STGCN_STEM_F16MX): KF6 with fp16 x fp16 + two scaled-e4m3 residual products per k-step group
bool stem_f16mx_supported(int C, int T, int V, int K, unsigned flags);
size_t stem_f16mx_prep_bytes(int C, int K);
int launch_stem_f16mx_prepare(const float *W12, const float *Wt, const float *t_scale, void *dst, int C, hipStream_t st);
int launch_stem_f16mx(const float *x, bool x_ntvc, const void *pfrag, const void *bounds, const void *prep_w12, const void *mx_blob,
                      const float *shift, void *out, int N, int C, int T, int V, int K, unsigned flags, hipStream_t st);
int launch_stem_v6w(const float *x, bool x_ntvc, const void *pfrag, const void *prep_w12, const void *Wq, const float *shift,
                    void *out, int N, int C, int T, int V, int K, unsigned flags, hipStream_t st);
int launch_tcn_pack_bf16_pairs(const float *W, const float *scale, void *Wq, int Cin, int Cout, hipStream_t st);
int launch_stem_v6(const float *x, bool x_ntvc, const void *pfrag, const void *prep_w12, const void *Wq, const float *shift,
                   void *out, int N, int C, int T, int V, int K, unsigned flags, hipStream_t st);

// training-mode BatchNorm helpers (train_bn.hip)
int launch_fill_ones_zeros(float *ones, float *zeros, int C, hipStream_t st);
int launch_bn_batch_stats(const float *z, double *sums, int N, int C, size_t plane, hipStream_t st);
int launch_bn_train_finalize(const double *sums, double count, const float *weight, const float *bias,
                             float *running_mean, float *running_var, float momentum, float eps, float *scale,
                             float *shift, int C, hipStream_t st, float *save_mean = nullptr,
                             float *save_invstd = nullptr);
int launch_bn_frozen_finalize(const float *weight, const float *bias, const float *running_mean, const float *running_var,
                              float eps, float *scale, float *shift, int C, hipStream_t st, float *save_mean = nullptr,
                              float *save_invstd = nullptr);
int launch_bn_scale_shift(const float *weight, const float *bias, const float *mean, const float *invstd, float *scale,
                          float *shift, int C, hipStream_t st);
int launch_bn_apply(const float *za, const float *sa, const float *ta, const float *zb, const float *sb,
                    const float *tb, float *y, size_t total, int C, size_t plane, hipStream_t st);

// backward of the training-mode blocks (tcn_backward.hip)
int launch_bn_relu_bwd_stats(const float *za, const float *sa, const float *ta, const float *ma, const float *ia,
                             const float *zb, const float *sb, const float *tb, const float *mb, const float *ib,
                             const float *dy, double *sums, int N, int C, size_t plane, hipStream_t st);
int launch_bn_bwd_finalize(const double *sums, int which, double count, const float *gamma, const float *invstd,
                           float *dgamma, float *dbeta, float *coef, int C, hipStream_t st, bool frozen = false);
int launch_upsample2(const float *dz, float *dzu, size_t rows, int Tout, int T, int V, hipStream_t st);
int launch_bn_relu_bwd_apply(const float *za, const float *sa, const float *ta, const float *ma, const float *ia,
                             const float *zb, const float *sb, const float *tb, const float *mb, const float *ib,
                             const float *dy, const float *coefa, const float *coefb, float *dza, float *dzb, double *bsum,
                             int N, int C, size_t plane, hipStream_t st,
                             float *gout = nullptr);   // optional: the masked cotangent g itself (identity residual: dL/dx of "+ x")
int launch_doubles_to_floats(const double *src, float *dst, int n, hipStream_t st);
int launch_weight_flip(const float *W, float *Wf, int Cout, int Cin, int K, hipStream_t st);
int launch_tcn_dgrad_valu(const float *dz, const float *W, float *dx, int N, int Cin, int Cout, int T, int V, int K,
                          int stride, int Tout, hipStream_t st);
size_t tcn_wgrad_ws_bytes(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
// one wave per SIMD, input tile as a ring (tcn_wgrad_v6.hip): 17 <= V <= 24
bool tcn_wgrad_v6_supported(int N, int Cin, int Cout, int T, int V, int K, int stride);
int tcn_wgrad_v6_splits(int N, int Cin, int Cout, int T);
int launch_tcn_wgrad_v6(const float *dz, const float *x, float *part, int N, int Cin, int Cout, int T, int V, int K, unsigned flags,
                        hipStream_t st);
int launch_tcn_wgrad(const float *dz, const float *x, float *dW, float *part, int N, int Cin, int Cout, int T, int V, int K,
                     int stride, int Tout, unsigned flags, hipStream_t st);

// The per-channel vectors of a training forward, one block at the head of its workspace: unit / zero vectors for the
// raw-mode kernels, (scale, shift) and the fp64 sums of two BatchNorms.  The temporal conv has one BatchNorm and leaves
// s2, t2 and sums2 unused.
struct TrainSmall {
    float *ones, *zeros, *s1, *t1, *s2, *t2;
    double *sums1, *sums2;      // 2*C each: sum, sum of squares
};
static inline TrainSmall carve_train_small(Carve &c, int C) {
    TrainSmall w;
    w.ones = c.packed<float>(C); w.zeros = c.packed<float>(C);
    w.s1 = c.packed<float>(C); w.t1 = c.packed<float>(C); w.s2 = c.packed<float>(C); w.t2 = c.packed<float>(C);
    w.sums1 = c.packed<double>(2 * (size_t)C); w.sums2 = c.packed<double>(2 * (size_t)C);
    c.pad();
    return w;
}

// training-mode temporal conv block (tcn_train.hip): the plan both the size query and the entry point read — the path
// choice and, through the carve over it, every region of the workspace.  `flags` may carry STGCN_BN_FROZEN (no size depends
// on it).  ws_bytes == 0: T, K and stride leave no output frame.
struct TcnTrainPlan {
    bool frozen = false, stats_in_conv = false;   // stats_in_conv: the one-wave kernel sums the batch statistics in its epilogue
    unsigned cflags = 0;                          // the raw convolution's flags ...
    TcnPlan conv;                                 // ... and its plan
    int Tout = 0;
    size_t ws_bytes = 0;
};
TcnTrainPlan plan_tcn_train(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
int launch_tcn_forward_train(const TcnTrainPlan &p, const float *x, const float *W, const float *conv_bias,
                             const float *bn_weight, const float *bn_bias, float *bn_running_mean, float *bn_running_var,
                             float momentum, float eps, void *ws, float *y, float *save_z, float *save_mean,
                             float *save_invstd, int N, int Cin, int Cout, int T, int V, int K, int stride, hipStream_t st);
struct TcnBackwardPlan {
    bool frozen = false;
    bool upsampled = false;         // stride 2, odd K: run as the stride-1 block's backward on dz upsampled with zero frames
    bool dgrad_by_forward = false;  // dx = the forward kernels on the flipped weights:
    unsigned flags = 0, dgrad_flags = 0;
    TcnPlan dgrad;                  // the plan of that convolution (Cout input, Cin output channels), run with dgrad_flags
    int Tout = 0, stride = 0, Tz = 0;   // stride and frames of the gradient tensor the two conv gradients read (after upsampling)
    size_t wgrad_bytes = 0;             // partials of the matrix-core wgrad (0: it does not serve the shape)
    size_t ws_bytes = 0;
};
TcnBackwardPlan plan_tcn_backward(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
int launch_tcn_backward_train(const TcnBackwardPlan &p, const float *x, const float *W, const float *z, const float *bn_weight,
                              const float *bn_bias, const float *save_mean, const float *save_invstd, const float *dy, float *dx,
                              float *dW, float *dbias, float *dgamma, float *dbeta, void *ws, int N, int Cin, int Cout, int T,
                              int V, int K, hipStream_t st);

// training-mode graph conv (agcn_train.hip): the plans of its two entry points, read by the size queries and the entry points alike
struct AgcnTrainPlan {
    bool frozen = false, has_down = false;
    bool moments = false;        // batch statistics from the feature moments: the two pre-BatchNorm branches are never written
    bool down_as_gemm = false;   // materialising path: conv_down as one plain product (outside Cin = 3)
    ExpandPlan main, down;       // the expansion that writes y (moments) or the main branch; the one that writes the down branch
    size_t ws_bytes = 0;
};
// materialise: the branches are to be saved, the statistics are frozen or there is no down branch (the size query's hint)
AgcnTrainPlan plan_agcn_train(int N, int Cin, int Cout, int T, int V, int S, bool materialise, bool has_down, bool frozen);
int launch_agcn_forward_train(const AgcnTrainPlan &p, const float *x, const float *P, const float *Wd, const float *bd,
                              const float *Wdown, const float *bdown, const float *bn_weight, const float *bn_bias,
                              float *bn_running_mean, float *bn_running_var, const float *dbn_weight, const float *dbn_bias,
                              float *dbn_running_mean, float *dbn_running_var, float momentum, float eps, void *ws, float *y,
                              float *save_zm, float *save_zd, float *save_stats, int N, int Cin, int Cout, int T, int V, int S,
                              hipStream_t st);
struct AgcnBackwardPlan {
    bool frozen = false, has_down = false;
    bool fused = false;          // the moment form (agcn_backward.hip); else the generic GEMM chain
    bool recompute = false;      // generic: the forward kept no branches, they are rebuilt in the workspace
    int inter_c_max = 0;         // generic: the embedding width the workspace is sized for
    ExpandPlan expand;           // recompute: the expansion that rebuilds either branch
    size_t ws_bytes = 0;         // 0: V > kAttentionMaxV
};
// generic: the caller wants the GEMM chain (input gradient, identity residual, saved branches, frozen statistics)
AgcnBackwardPlan plan_agcn_backward(int N, int Cin, int Cout, int T, int V, int S, bool recompute, bool generic, bool has_down,
                                    bool frozen);
int launch_agcn_backward_train(const AgcnBackwardPlan &p, const float *x, const float *A_eff, const float *Wa, const float *ba,
                               const float *Wb, const float *bb, const float *Wd, const float *bd, const float *Wdown,
                               const float *bdown, const float *P, const float *zm, const float *zd, const float *bn_weight,
                               const float *bn_bias, const float *dbn_weight, const float *dbn_bias, const float *save_stats,
                               const float *y, const float *dy, float *dWa, float *dba, float *dWb, float *dbb, float *dWd,
                               float *dbd, float *dWdown, float *dbdown, float *dgamma, float *dbeta, float *ddgamma,
                               float *ddbeta, float *dPA, float *dx, void *ws, int N, int Cin, int Cout, int T, int V,
                               int inter_c, int S, hipStream_t st);

// backward of the training-mode graph conv (agcn_backward.hip)
size_t agcn_bwd_ws_bytes(int N, int Cin, int Cout, int T, int V, int S);   // 0: the moment form does not cover the shape
int launch_agcn_bwd(const float *x, const float *P, const float *A_eff, const float *y, const float *dy, const float *Wa,
                    const float *ba, const float *Wb, const float *bb, const float *Wd, const float *bd, const float *Wdown,
                    const float *bdown, const float *bn_w, const float *dbn_w, const float *stats, void *ws, float *dWa,
                    float *dba, float *dWb, float *dbb, float *dWd, float *dbd, float *dWdown, float *dbdown, float *dgamma,
                    float *dbeta, float *ddgamma, float *ddbeta, float *dPA, int N, int Cin, int Cout, int T, int V, int inter_c,
                    int S, hipStream_t st);

// strided batched fp32 GEMM + small helpers (gemm_f32.hip): C[b][m][n] (+)= alpha * sum_k A[b][m][k] B[b][k][n] (+ bias[m])
struct GemmArgs {
    const float *A, *B;
    float *C;
    const float *bias;                 // per output row m, or NULL
    int M, N, K;
    long long a_sm, a_sk, a_sb;        // element strides: row, contraction index, batch
    long long b_sk, b_sn, b_sb;
    long long c_sm, c_sn, c_sb;
    float alpha;
    int accumulate;                    // 0: C = ..., 1: C += ...
    // optional two-level ROW index: row i = q*m_inner + r addresses A at q*a_sm + r*a_sm2 and C at q*c_sm + r*c_sm2
    // (m_inner = 0: single level, i*a_sm / i*c_sm).  nbias (optional): per column n.  cbias (optional) adds
    // cbias[q*cb_sq + r*cb_sr + n*cb_sn].
    int m_inner = 0;
    long long a_sm2 = 0, c_sm2 = 0;
    const float *nbias = nullptr;
    const float *cbias = nullptr;
    long long cb_sq = 0, cb_sr = 0, cb_sn = 0;
    // optional split of the contraction index: part j of ksplit covers k in [j*kc, (j+1)*kc) (kc a multiple of the K chunk)
    // and writes C + j*c_ss — the caller sums the parts in a fixed order (launch_sum_parts).  For products with a long K
    // and a small C (the per-clip weight-gradient slices, the joint Gram matrices) whose one tile per clip left most CUs idle.
    int ksplit = 1;
    long long c_ss = 0;
    // optional two-level BATCH index (the chain's (clip, subset) products): b = bq*b_inner + br addresses A at
    // bq*a_sb + br*a_sb2, B and C alike (b_inner = 0: single level)
    int b_inner = 0;
    long long a_sb2 = 0, b_sb2 = 0, c_sb2 = 0;
    // optional two-level CONTRACTION index ((subset, joint) in dx += sum_s du_s P_s^T): k = kq*k_inner + kr addresses A at
    // kq*a_sk + kr*a_sk2 and B at kq*b_sk + kr*b_sk2 (k_inner = 0: single level)
    int k_inner = 0;
    long long a_sk2 = 0, b_sk2 = 0;
};
// The shape limits of the launchers below, one host predicate each: the launcher asks it and refuses with
// STGCN_ERR_UNSUPPORTED, and a plan that wants to refuse before its first launch asks it too (pointers are not read).
bool gemm_f32_spans_fit(const GemmArgs &g);              // every operand of one batch entry within 32-bit offsets
bool gemm_f32_grid_fits(const GemmArgs &g, int batch);   // column tiles and batch entries on 16-bit grid axes
bool sum_parts_covers(int parts, size_t n);
bool row_sum_covers(long long rows, long long cols);
int launch_gemm_f32(const GemmArgs &g, int batch, hipStream_t st);
// out[rep*rep_stride + e] = sum_p part[p*n + e] in a fixed order, written `reps` times (one bias gradient shared by the subsets)
int launch_sum_parts(const float *part, float *out, int parts, size_t n, hipStream_t st, int reps = 1, size_t rep_stride = 0);
int launch_add_inplace(float *dst, const float *src, size_t n, hipStream_t st);
int launch_row_sum(const float *in, float *out, int rows, int cols, hipStream_t st);
// out[b][r][:] (+)= sum_{i < nsum} in[b][i][r][:] . M[b][i]  (rows of V floats times V x V matrices; gemm_f32.hip)
int launch_rowmix(const float *in, const float *M, float *out, int R, int V, int nsum, int accumulate, long long in_sb,
                  long long in_sb2, long long in_ss, long long m_sb, long long m_sb2, long long m_ss, bool m_transposed,
                  long long out_sb, long long out_sb2, int batch, int b_inner, hipStream_t st);
int launch_softmax_bwd(const float *P, const float *A_eff, const float *dP, float *dS, int N, int V, int S, float alpha,
                       hipStream_t st);

// weights times channel-first activations in the three-term split arithmetic (wx_bf16.hip):
// C[n] = W . X[n] (+ bias per row) (+ R[n]); W (M,K), or (K,M) with w_transposed; X[n] (K,TV); C[n], R[n] (M,TV); R may not overlap C
bool wx_bf16x3_covers(int M, int K, long long TV, int N);   // asked by its launcher and by plan_wx (st_attention.hip)
int wx_bf16x3_tile_rows(int M);              // rows of the tile form that serves M: 128 or 64
const char *wx_bf16x3_kernel_name(int M);
int launch_wx_bf16x3(const float *W, const float *X, const float *bias, const float *R, float *C, int N, int M, int K,
                     long long TV, bool w_transposed, hipStream_t st);

// first patch embedding of the transformer heads on the stem output (gemm_f32.hip: one strided GEMM per clip)
int launch_patch_embed(const float *z, const float *W, const float *b, const float *pos, float *out, int N, int C, int E,
                       int T, int V, unsigned flags, hipStream_t st);

// generic backward of the training-mode graph conv: any Cin / Cout / subsets, identity or conv residual, optional dx
// (agcn_backward_generic.hip)
size_t agcn_bwd_generic_ws_floats(int N, int Cin, int Cout, int T, int V, int inter_c, int S);
int launch_agcn_bwd_generic(const float *x, const float *P, const float *A_eff, const float *dzm, const float *dzd,
                            const float *Wa, const float *ba, const float *Wb, const float *bb, const float *Wd,
                            const float *Wdown, float *ws, float *dWa, float *dba, float *dWb, float *dbb, float *dWd,
                            float *dbd, float *dWdown, float *dbdown, float *dPA, float *dx, int dx_initialised, int N,
                            int Cin, int Cout, int T, int V, int inter_c, int S, hipStream_t st);

// fused stem: the f32 kernel and the graph-conv fold (tcn_conv.hip) ...
size_t stem_w12_bytes(int C);
int launch_stem_fold(const float *Wd, const float *bd, const float *Wdown, const float *bdown, const float *bn_scale,
                     const float *bn_shift, const float *down_scale, const float *down_shift, float *W12, int Cin, int C, int S,
                     hipStream_t st);
bool stem_f32_supported(int C, int T, int V, int K);   // Cin = 3, 3 subsets
int launch_stem_f32(const float *x, const float *P, const float *W12, const void *Wp, const float *shift, void *out, int N, int C,
                    int T, int V, int K, unsigned flags, hipStream_t st);   // (the same signature as launch_stem_bf16_small)

// ... and the plan every stem entry point reads (stem.hip; the layouts are described there)
enum class StemKernel { none, f32, bf16_small, kf4_features, kf4_frags, kf6, kf6w, kf7 };
enum class StemPart { none, features, frags, xcopy };   // the workspace part behind P
struct StemPrep { size_t bytes = 0, single = 0, pairs = 0, f16mx = 0; };   // prep blob: bytes, offsets of its parts (0: absent)
struct StemPlan {
    StemKernel kernel = StemKernel::none;
    StemPrep prep;
    StemPart part = StemPart::none;
    size_t ws_bytes = 0, part_off = 0, bounds_off = 0;  // P at 0; bounds_off: KF7's per-clip bounds (0: not written)
    int split = 0;                                      // frags of wide frames: V0 of the joint halves, else 0
};
StemPrep plan_stem_prep(int C, int K, unsigned flags);
StemPlan plan_stem(int N, int Cin, int C, int T, int V, int K, int S, unsigned flags);
const char *stem_kernel_name(StemKernel k);
int launch_stem_prepare(const float *Wd, const float *bd, const float *Wdown, const float *bdown,
                        const float *bn_scale, const float *bn_shift, const float *down_scale,
                        const float *down_shift, const float *Wt, const float *t_scale, void *prep,
                        int Cin, int C, int K, int S, unsigned flags, hipStream_t st);
int launch_stem(const StemPlan &p, const float *x, const void *ws, const void *prep, const float *t_shift, void *out, int N,
                int Cin, int C, int T, int V, int S, int K, unsigned flags, hipStream_t st);

}  // namespace stgcn
