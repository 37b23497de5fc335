// Temporal conv of Unit2D (conv_t + folded BatchNorm + ReLU, or raw), host side: the plan every entry point reads — which
// kernel serves a shape (the kernels' coverage predicates are called here only) and what the packed weight blob holds —
// the packing and the launch.
#include "common.h"

namespace stgcn {

// packed blob: [ the weights in ONE of the layouts below, `single` bytes ]
//   valu      : (Cout,Cin,K) floats, scale folded in                                    whatever the others do not take
//   f32_frags : the same floats in fp32 MFMA A-fragment order (tcn_conv.hip)           STGCN_MATH_F32, Cin % 16 == 0, Cout % 128 == 0
//   bf16      : bf16 hi and lo images in 32x32x16 fragment order (tcn_bf16.hip);       bf16 / bf16x3, Cin % 16 == 0,
//               64 output channels are padded to 128 rows, the upper 64 zero           Cout % 128 == 0 or Cout == 64
//             [ the bf16 weights again in KF6's pair order (tcn_bf16_v6.hip), at `pairs` ]   where K3v6 takes the weights
// every part 256-B aligned.  It depends on (Cin, Cout, K, math) only.  The fused stem's prep blob takes its sizes and offsets
// from here (stem.hip).
// An unknown math mode has no layout; its size is the VALU layout's.
TcnPack plan_tcn_pack(int Cin, int Cout, int K, unsigned flags) {
    const unsigned math = flags & STGCN_MATH_MASK;
    const bool bf16 = math == STGCN_MATH_BF16X3 || math == STGCN_MATH_BF16;
    TcnPack p;
    p.layout = bf16 && Cin % 16 == 0 && (Cout % 128 == 0 || Cout == 64)            ? TcnLayout::bf16
               : math == STGCN_MATH_F32 && Cin % 16 == 0 && Cout % 128 == 0        ? TcnLayout::f32_frags
               : math <= STGCN_MATH_F32_VALU                                       ? TcnLayout::valu
                                                                                   : TcnLayout::none;
    const int rows = p.layout == TcnLayout::bf16 ? (Cout + 127) / 128 * 128 : Cout;
    p.bytes = p.single = align_up((size_t)Cin * rows * K * sizeof(float), 256);   // one float per weight, or two bf16 images
    if (p.layout == TcnLayout::bf16 && tcn_v6_takes_weights(Cin, Cout, K)) p.pairs = p.single, p.bytes += p.single;
    return p;
}

// Kernels, first that covers.  The joint axis (STGCN_CONV_ALONG_V) has the VALU kernel only.  On the bf16 layout: K3v6 (one
// wave per SIMD), K3v4 (eight waves), the 128-pixel tile — or none: a bf16 blob is never read by the VALU kernel.  On the
// f32 fragments the fp32 MFMA kernel or none.  On the VALU layout the VALU kernel, whatever the math mode asked for.
// Diagnostic builds: ablation bit 8192 keeps K3v4 where K3v6 would run.
TcnPlan plan_tcn(int Cin, int Cout, int T, int V, int K, int stride, unsigned flags) {
    const unsigned math = flags & STGCN_MATH_MASK;
    const int terms = math == STGCN_MATH_BF16X3 ? 3 : 1;
    TcnPlan p;
    p.pack = plan_tcn_pack(Cin, Cout, K, flags);
    if (flags & STGCN_CONV_ALONG_V) {
        p.Tout = T;
        if (math == STGCN_MATH_F32_VALU && tcn_out_frames(V, K, stride) >= 1) p.kernel = TcnKernel::valu_joint_axis;
        return p;
    }
    p.Tout = tcn_out_frames(T, K, stride);
    if (p.Tout < 1) return p;
    bool stats_ok = false;
    switch (p.pack.layout) {
    case TcnLayout::bf16:
        if (p.pack.pairs && !(ablate_mask() & 8192) && tcn_v6_covers(Cin, Cout, T, V, K, stride, terms, p.tile, stats_ok)) {
            p.kernel = TcnKernel::v6;
            p.stats_in_conv_ok = stats_ok && !(flags & (STGCN_OUT_BF16 | STGCN_OUT_NTVC));
        } else if (tcn_v4_covers(Cin, Cout, T, V, K, stride, terms, p.tile)) {
            p.kernel = TcnKernel::v4;
        } else if (tcn_bf16_small_covers(Cin, Cout, V, K, stride, p.Tout, terms, p.tile)) {
            p.kernel = TcnKernel::bf16_small;
        }
        break;
    case TcnLayout::f32_frags:
        if (tcn_mfma_f32_covers(Cin, Cout, V, K, stride, p.Tout, p.tile)) p.kernel = TcnKernel::mfma_f32;
        break;
    case TcnLayout::valu: p.kernel = TcnKernel::valu; break;
    case TcnLayout::none: break;
    }
    return p;
}

const char *tcn_kernel_name(TcnKernel k) {
    static const char *const names[] = {"", "tcn_valu_kernel", "tcn_valu_joint_axis_kernel", "tcn_mfma_f32_kernel",
                                        "tcn_mfma_bf16_kernel", "tcn_bf16_v4_kernel", "tcn_bf16_v6_kernel"};
    return names[(int)k];
}

int launch_tcn_pack(const TcnPack &p, const float *W, const float *scale, void *Wp, int Cin, int Cout, int K, hipStream_t st) {
    switch (p.layout) {
    case TcnLayout::bf16: {
        const int rc = launch_tcn_pack_bf16(W, scale, Wp, Cin, Cout, K, st);
        if (rc != STGCN_OK || !p.pairs) return rc;
        return launch_tcn_pack_pairs_padded(W, scale, (char *)Wp + p.pairs, Cin, Cout, st);
    }
    case TcnLayout::f32_frags:
    case TcnLayout::valu: return launch_tcn_pack_f32(p.layout == TcnLayout::f32_frags, W, scale, Wp, Cin, Cout, K, st);
    default: return fail(STGCN_ERR_UNSUPPORTED, "tcn_pack: math mode not built");
    }
}

int launch_tcn(const TcnPlan &p, const float *x, const void *Wp, const float *shift, void *y, int N, int Cin, int Cout, int T,
               int V, int K, int stride, unsigned flags, hipStream_t st, double *stats) {
    const unsigned math = flags & STGCN_MATH_MASK;
    if (flags & STGCN_CONV_ALONG_V) {      // Unit2D(dim=3): the joint axis
        if (math != STGCN_MATH_F32_VALU) return fail(STGCN_ERR_UNSUPPORTED, "tcn: STGCN_CONV_ALONG_V goes with STGCN_MATH_F32_VALU");
        if (p.kernel == TcnKernel::none) return fail(STGCN_ERR_ARG, "tcn: V=%d K=%d stride=%d gives no output joint", V, K, stride);
    } else if (p.Tout < 1) {
        return fail(STGCN_ERR_ARG, "tcn: T=%d K=%d stride=%d gives no output frame", T, K, stride);
    }
    if (stats != nullptr && !p.stats_in_conv_ok)
        return fail(STGCN_ERR_UNSUPPORTED, "tcn: no kernel sums the channel statistics of this shape and output");
    // (the statistics form is the training forward's: a persistent kernel, no clip index in its grid)
    if (N > 65535 && stats == nullptr) return fail(STGCN_ERR_UNSUPPORTED, "tcn: N=%d > 65535 clips per call", N);
    switch (p.kernel) {
    case TcnKernel::valu_joint_axis:
        return launch_tcn_valu(true, x, Wp, shift, y, N, Cin, Cout, T, V, K, stride, tcn_out_frames(V, K, stride), flags, st);
    case TcnKernel::valu: return launch_tcn_valu(false, x, Wp, shift, y, N, Cin, Cout, T, V, K, stride, p.Tout, flags, st);
    case TcnKernel::mfma_f32:
    case TcnKernel::bf16_small:
        return (p.kernel == TcnKernel::mfma_f32 ? launch_tcn_mfma_f32 : launch_tcn_bf16_small)(
            p.tile, x, Wp, shift, y, N, Cin, Cout, T, V, K, stride, p.Tout, flags, st);
    case TcnKernel::v4: return launch_tcn_v4(p.tile, x, Wp, shift, y, N, Cin, Cout, T, V, flags, st);
    case TcnKernel::v6:
        return launch_tcn_v6(p.tile, x, (const char *)Wp + p.pack.pairs, shift, y, N, Cin, Cout, T, V, flags, st, stats);
    case TcnKernel::none: break;
    }
    if (p.pack.layout == TcnLayout::none) return fail(STGCN_ERR_ARG, "tcn: unknown math mode %u", math);
    if (p.pack.layout == TcnLayout::bf16)
        return fail(STGCN_ERR_UNSUPPORTED,
                    "bf16 MFMA kernel does not cover Cin=%d Cout=%d V=%d K=%d stride=%d T=%d (needs Cin%%16==0, "
                    "Cout%%128==0, tile rows that fit LDS)", Cin, Cout, V, K, stride, T);
    return fail(STGCN_ERR_UNSUPPORTED,
                "tcn: f32 MFMA kernel needs a tile row <= 768 floats (V=%d K=%d stride=%d); use STGCN_MATH_F32_VALU", V, K, stride);
}

}  // namespace stgcn
