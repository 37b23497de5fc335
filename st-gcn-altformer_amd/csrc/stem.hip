// Fused stem (tcn0(gcn0(x))), host side: the plan every stem entry point reads — which kernel serves a shape (the kernels'
// coverage predicates are called here only), where its operands sit in the prep blob and the workspace — and the launch.
#include "common.h"

namespace stgcn {

// prep blob: [ W12 : C x 16 floats ][ temporal weights, single packing (the temporal conv's, tcn.hip) ]
//            [ the same weights in KF6's pair order ]   where the temporal conv's blob has its pair-order copy and C % 128 == 0
//            [ KF7's header + weights ]                 STGCN_STEM_F16MX with bf16x3, behind the pair-order copy
// every part 256-B aligned.  It depends on (C, K, flags) only: one blob serves every batch shape.  The two weight parts have
// the sizes and offsets of the temporal conv's packed blob (plan_tcn_pack); the pair-order part is written by KF6's own pack
// kernel (stem_bf16_v6.hip), whose lo image differs from K3v6's in a last bit here and there.
StemPrep plan_stem_prep(int C, int K, unsigned flags) {
    const TcnPack t = plan_tcn_pack(C, C, K, flags);
    // (the fused kernels take C % 128 == 0 only and launch_stem_prepare refuses the rest; the size query answers for C = 64
    //  without the pair-order part, as it always has)
    const bool pairs = t.pairs && C % 128 == 0;
    StemPrep p;
    p.single = stem_w12_bytes(C);
    p.pairs = pairs ? p.single + t.pairs : 0;
    p.bytes = p.single + (pairs ? t.bytes : t.single);
    if (p.pairs && (flags & STGCN_STEM_F16MX) && (flags & STGCN_MATH_MASK) == STGCN_MATH_BF16X3) {
        p.f16mx = p.bytes;
        p.bytes += align_up(stem_f16mx_prep_bytes(C, K), 256);
    }
    return p;
}

// workspace: [ P : N*S*V*V floats ] then, 256-B aligned, ONE of
//   features : N*T*V x 64 B (16 features as bf16 hi + lo), written by the attention kernel   KF4 on 128-pixel tiles
//   frags    : N x 12 KiB (the attention matrices as bf16 hi/lo MFMA B fragments; 48 KiB      KF4 on 256-pixel tiles,
//              for wide frames, split at stem_wide_split(V)); the kernel computes features   KF6, KF6w, KF7
//   xcopy    : N*Cin*T*V floats, channel-major, with STGCN_IN_NTVC                           the kernels that read x
// and, where KF7 covers the shape, (N,4) floats of per-clip bounds behind the large-tile part.
// Kernels, first that covers: KF7 (STGCN_STEM_F16MX) on fragments; KF6, the 256-pixel tile with one wave per SIMD; KF6w,
// the same kernel over the two joint halves of a wide frame; KF4 (eight waves); then the 128-pixel bf16 or the f32 kernel.
// Diagnostic builds: ablation bit 256 keeps KF4 where KF6 / KF6w would run, 512 keeps KF4 / KF6 where KF7 would.
StemPlan plan_stem(int N, int Cin, int C, int T, int V, int K, int S, unsigned flags) {
    const unsigned math = flags & STGCN_MATH_MASK;
    StemPlan p;
    p.prep = plan_stem_prep(C, K, flags);
    p.ws_bytes = align_up((size_t)N * S * V * V * sizeof(float), 256);
    bool frags = false;   // the 256-pixel tile: KF4 computes the features itself from the fragments
    if (stem_v4_supported(Cin, C, T, V, K, S, flags, &frags)) {
        const bool v6 = frags && stem_v6_supported(C, T, V, K, flags) && !(ablate_mask() & 256);
        const bool v6w = !frags && stem_v6w_supported(C, T, V, K, flags) && !(ablate_mask() & 256);
        const bool f16mx = stem_f16mx_supported(C, T, V, K, flags);
        frags = frags || v6w;
        p.kernel = frags && f16mx && !(ablate_mask() & 512) ? StemKernel::kf7
                   : v6                                     ? StemKernel::kf6
                   : v6w                                    ? StemKernel::kf6w
                   : frags                                  ? StemKernel::kf4_frags
                                                            : StemKernel::kf4_features;
        p.part = frags ? StemPart::frags : StemPart::features;
        p.part_off = p.ws_bytes;
        p.ws_bytes += frags ? (size_t)N * (V > 32 ? 48 : 12) * 1024 : (size_t)N * T * V * 16 * sizeof(float);
        p.split = frags ? stem_wide_split(V) : 0;
        if (f16mx) {   // (the room is there whenever KF7 covers the shape; the attention kernel fills it with fragments)
            p.bounds_off = frags ? p.ws_bytes : 0;
            p.ws_bytes += align_up((size_t)N * 4 * sizeof(float), 256);
        }
        return p;
    }
    if (flags & STGCN_IN_NTVC) {
        p.part = StemPart::xcopy;
        p.part_off = p.ws_bytes;
        p.ws_bytes += (size_t)N * Cin * T * V * sizeof(float);
    }
    if (!agcn_stem_class(Cin, S) || T < 1) return p;
    if (math == STGCN_MATH_BF16X3 || math == STGCN_MATH_BF16) {
        if (stem_bf16_small_supported(C, T, V, K, flags)) p.kernel = StemKernel::bf16_small;
    } else if (math == STGCN_MATH_F32 && stem_f32_supported(C, T, V, K)) {
        p.kernel = StemKernel::f32;
    }
    return p;
}

const char *stem_kernel_name(StemKernel k) {   // (both forms of KF4, and KF6 and KF6w, share a kernel name)
    static const char *const names[] = {"", "stem_mfma_f32_kernel", "stem_mfma_bf16_kernel", "stem_bf16_v4_kernel",
                                        "stem_bf16_v4_kernel", "stem_bf16_v6_kernel", "stem_bf16_v6_kernel", "stem_f16mx_kernel"};
    return names[(int)k];
}

int launch_stem_prepare(const float *Wd, const float *bd, const float *Wdown, const float *bdown,
                        const float *bn_scale, const float *bn_shift, const float *down_scale,
                        const float *down_shift, const float *Wt, const float *t_scale, void *prep, int Cin,
                        int C, int K, int S, unsigned flags, hipStream_t st) {
    const unsigned math = flags & STGCN_MATH_MASK;
    if (math != STGCN_MATH_F32 && math != STGCN_MATH_BF16X3 && math != STGCN_MATH_BF16)
        return fail(STGCN_ERR_UNSUPPORTED, "stem: no fused kernel for math mode %u", math);
    if (Cin != 3 || S != 3 || C % 128 != 0)
        return fail(STGCN_ERR_UNSUPPORTED, "stem: fused kernel covers Cin=3, 3 subsets, C%%128==0 (got Cin=%d S=%d C=%d)",
                    Cin, S, C);
    const StemPrep p = plan_stem_prep(C, K, flags);
    char *const blob = (char *)prep;
    int rc = launch_stem_fold(Wd, bd, Wdown, bdown, bn_scale, bn_shift, down_scale, down_shift, (float *)blob, Cin, C, S, st);
    TcnPack single = plan_tcn_pack(C, C, K, flags);
    single.bytes = single.single, single.pairs = 0;   // the single packing alone: the pair-order part is KF6's own
    if (rc == STGCN_OK) rc = launch_tcn_pack(single, Wt, t_scale, blob + p.single, C, C, K, st);
    if (rc == STGCN_OK && p.pairs) rc = launch_tcn_pack_bf16_pairs(Wt, t_scale, blob + p.pairs, C, C, st);
    if (rc == STGCN_OK && p.f16mx) rc = launch_stem_f16mx_prepare((const float *)blob, Wt, t_scale, blob + p.f16mx, C, st);
    return rc;
}

int launch_stem(const StemPlan &p, const float *x, const void *ws, const void *prep, const float *t_shift, void *out, int N,
                int Cin, int C, int T, int V, int S, int K, unsigned flags, hipStream_t st) {
    if (N > kMaxGridClips) return fail(STGCN_ERR_UNSUPPORTED, "stem: N=%d > %d clips per call", N, kMaxGridClips);
    const char *w = (const char *)ws, *b = (const char *)prep;
    const float *part = (const float *)(w + p.part_off), *P = (const float *)ws;
    const bool x_ntvc = (flags & STGCN_IN_NTVC) != 0;
    switch (p.kernel) {
    case StemKernel::f32:          // (these two read x channel-major: the workspace's copy of it with STGCN_IN_NTVC)
    case StemKernel::bf16_small:
        return (p.kernel == StemKernel::f32 ? launch_stem_f32 : launch_stem_bf16_small)(
            p.part == StemPart::xcopy ? part : x, P, (const float *)prep, b + p.prep.single, t_shift, out, N, C, T, V, K, flags, st);
    case StemKernel::kf4_features:
    case StemKernel::kf4_frags:
        return launch_stem_v4(x, x_ntvc, part, prep, b + p.prep.single, t_shift, out, N, C, T, V, K, flags, st);
    case StemKernel::kf6:
    case StemKernel::kf6w:
        return (p.kernel == StemKernel::kf6 ? launch_stem_v6 : launch_stem_v6w)(x, x_ntvc, part, prep, b + p.prep.pairs, t_shift,
                                                                               out, N, C, T, V, K, flags, st);
    case StemKernel::kf7:
        return launch_stem_f16mx(x, x_ntvc, part, w + p.bounds_off, prep, b + p.prep.f16mx, t_shift, out, N, C, T, V, K, flags,
                                 st);
    default:
        return fail(STGCN_ERR_UNSUPPORTED,
                    "stem: no fused kernel covers Cin=%d S=%d C=%d T=%d V=%d K=%d in math mode %u; call the two-stage path", Cin,
                    S, C, T, V, K, flags & STGCN_MATH_MASK);
    }
}

}  // namespace stgcn
