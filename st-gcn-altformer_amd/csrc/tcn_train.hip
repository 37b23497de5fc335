// Training mode of the temporal conv block (Unit2D: conv_t + BatchNorm + ReLU): the plans, workspaces and launch sequences
// of its forward and backward entry points.  The kernels are the eval-mode convolutions run raw (tcn_conv.hip,
// tcn_bf16*.hip), the BatchNorm pieces of train_bn.hip and the gradients of tcn_backward.hip / tcn_wgrad_v6.hip.
#include "common.h"

namespace stgcn {

namespace {

struct TcnTrainWs {
    TrainSmall v;
    char *packed;     // the weights in the convolution's layout, unit scale
    float *z;         // conv_t(x) + b
    size_t bytes;
};
TcnTrainWs carve_tcn_train(void *base, const TcnTrainPlan &p, int N, int Cin, int Cout, int V, int K) {
    Carve c(base);
    TcnTrainWs w{};
    w.v = carve_train_small(c, Cout);
    w.packed = c.packed<char>(p.conv.pack.bytes);
    w.z = c.packed<float>((size_t)N * Cout * p.Tout * V);
    w.bytes = c.off;
    return w;
}

}  // namespace

TcnTrainPlan plan_tcn_train(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags) {
    TcnTrainPlan p;
    p.frozen = (flags & STGCN_BN_FROZEN) != 0;
    p.cflags = (flags & STGCN_MATH_MASK) | STGCN_RAW;
    p.conv = plan_tcn(Cin, Cout, T, V, K, stride, p.cflags);
    p.Tout = p.conv.Tout;
    if (p.Tout < 1) return p;
#ifndef STGCN_NO_CONV_STATS    /* A/B builds: the separate statistics pass */
    p.stats_in_conv = !p.frozen && p.conv.stats_in_conv_ok;
#endif
    p.ws_bytes = carve_tcn_train(nullptr, p, N, Cin, Cout, V, K).bytes;
    return p;
}

int launch_tcn_forward_train(const TcnTrainPlan &p, const float *x, const float *W, const float *conv_bias,
                             const float *bn_weight, const float *bn_bias, float *bn_running_mean, float *bn_running_var,
                             float momentum, float eps, void *ws, float *y, float *save_z, float *save_mean,
                             float *save_invstd, int N, int Cin, int Cout, int T, int V, int K, int stride, hipStream_t st) {
    const TcnTrainWs w = carve_tcn_train(ws, p, N, Cin, Cout, V, K);
    float *z = save_z ? save_z : w.z;
    double *sums = w.v.sums1;
    const size_t plane = (size_t)p.Tout * V, total = (size_t)N * Cout * plane;
    int rc;
    if ((rc = launch_fill_ones_zeros(w.v.ones, w.v.zeros, Cout, st))) return rc;
    if ((rc = launch_tcn_pack(p.conv.pack, W, w.v.ones, w.packed, Cin, Cout, K, st))) return rc;   // unit scale: the raw convolution
    const float *bias = conv_bias ? conv_bias : w.v.zeros;
    // stats_in_conv: the one-wave kernel sums the batch statistics in its epilogue (no separate pass over z)
    if (p.stats_in_conv) STGCN_HIP_CHECK(hipMemsetAsync(sums, 0, sizeof(double) * 2 * Cout, st));
    if ((rc = launch_tcn(p.conv, x, w.packed, bias, z, N, Cin, Cout, T, V, K, stride, p.cflags, st, p.stats_in_conv ? sums : nullptr)))
        return rc;
    if (p.frozen) {
        rc = launch_bn_frozen_finalize(bn_weight, bn_bias, bn_running_mean, bn_running_var, eps, w.v.s1, w.v.t1, Cout, st,
                                       save_mean, save_invstd);
    } else {
        if (!p.stats_in_conv && (rc = launch_bn_batch_stats(z, sums, N, Cout, plane, st))) return rc;
        rc = launch_bn_train_finalize(sums, (double)N * plane, bn_weight, bn_bias, bn_running_mean, bn_running_var, momentum,
                                      eps, w.v.s1, w.v.t1, Cout, st, save_mean, save_invstd);
    }
    if (rc != STGCN_OK) return rc;
    return launch_bn_apply(z, w.v.s1, w.v.t1, nullptr, nullptr, nullptr, y, total, Cout, plane, st);
}

// ---- backward ------------------------------------------------------------------------------------------------------
namespace {

struct TcnBackwardWs {
    double *sums, *bsum;             // 3*Cout, 2*Cout
    float *coef, *scale, *shift;     // 3*Cout, Cout, Cout
    float *ones, *zeros;             // Cin each: the dgrad's unit scale and zero bias
    float *dz, *dzu;                 // gradient before the BatchNorm; the same upsampled with zero frames
    float *Wf;                       // dgrad by forward: the flipped weights ...
    void *packed;                    // ... in the convolution's layout
    float *part;                     // matrix-core wgrad partials (NULL: it does not serve the shape)
    size_t bytes;
};
TcnBackwardWs carve_tcn_backward(void *base, const TcnBackwardPlan &p, int N, int Cin, int Cout, int T, int V, int K) {
    Carve c(base);
    TcnBackwardWs w{};
    w.sums = c.packed<double>(3 * (size_t)Cout); w.bsum = c.packed<double>(2 * (size_t)Cout);
    w.coef = c.packed<float>(3 * (size_t)Cout); w.scale = c.packed<float>(Cout); w.shift = c.packed<float>(Cout);
    w.ones = c.packed<float>(Cin); w.zeros = c.packed<float>(Cin);
    c.pad();
    w.dz = c.take<float>((size_t)N * Cout * p.Tout * V);
    if (p.upsampled) w.dzu = c.take<float>((size_t)N * Cout * T * V);
    if (p.dgrad_by_forward) {
        w.Wf = c.take<float>((size_t)Cout * Cin * K);
        w.packed = c.take<char>(p.dgrad.pack.bytes);
    }
    if (p.wgrad_bytes) w.part = c.packed<float>(p.wgrad_bytes / sizeof(float));
    w.bytes = c.off;
    return w;
}

}  // namespace

TcnBackwardPlan plan_tcn_backward(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags) {
    TcnBackwardPlan p;
    p.frozen = (flags & STGCN_BN_FROZEN) != 0;
    p.flags = flags & ~STGCN_BN_FROZEN;
    p.Tout = tcn_out_frames(T, K, stride);
    if (p.Tout < 1) return p;
    // A stride-2 block with an odd K (TCN_GCN_unit's downsampling layers, model/ST_TR/ST_TR_new.py:362-372) runs its backward as
    // the stride-1 block's on dz upsampled with zero frames (launch_upsample2): matrix-core wgrad and dgrad instead of plain FMAs.
    p.upsampled = stride == 2 && (K & 1) == 1;
    p.stride = p.upsampled ? 1 : stride;
    p.Tz = p.upsampled ? T : p.Tout;
    // The input gradient of a stride-1 block is the forward kernel on the flipped weights ONLY for odd K: the transposed
    // conv pads K-1-pad frames, which equals the forward's pad = (K-1)/2 when K is odd.  With an even K the forward drops a
    // frame (Tout = T-1) and that shortcut would write T-2 misaligned frames: even K runs the general VALU dgrad instead.
    p.dgrad_by_forward = p.stride == 1 && (K & 1) == 1;
    if (p.dgrad_by_forward) {   // dgrad = forward conv with Cout input and Cin output channels, on the VALU where no
        p.dgrad_flags = (p.flags & STGCN_MATH_MASK) | STGCN_RAW;                        // matrix-core kernel takes it
        p.dgrad = plan_tcn(Cout, Cin, p.Tz, V, K, 1, p.dgrad_flags);
        if (!tcn_on_matrix_cores(p.dgrad.kernel)) {
            p.dgrad_flags = STGCN_MATH_F32_VALU | STGCN_RAW;
            p.dgrad = plan_tcn(Cout, Cin, p.Tz, V, K, 1, p.dgrad_flags);
        }
    }
    p.wgrad_bytes = tcn_wgrad_ws_bytes(N, Cin, Cout, T, V, K, p.stride, p.flags);
    p.ws_bytes = carve_tcn_backward(nullptr, p, N, Cin, Cout, T, V, K).bytes;
    return p;
}

int launch_tcn_backward_train(const TcnBackwardPlan &p, const float *x, const float *W, const float *z, const float *bn_weight,
                              const float *bn_bias, const float *save_mean, const float *save_invstd, const float *dy, float *dx,
                              float *dW, float *dbias, float *dgamma, float *dbeta, void *ws, int N, int Cin, int Cout, int T,
                              int V, int K, hipStream_t st) {
    const TcnBackwardWs w = carve_tcn_backward(ws, p, N, Cin, Cout, T, V, K);
    const size_t plane = (size_t)p.Tout * V;
    int rc;
    if ((rc = launch_bn_scale_shift(bn_weight, bn_bias, save_mean, save_invstd, w.scale, w.shift, Cout, st))) return rc;
    if ((rc = launch_bn_relu_bwd_stats(z, w.scale, w.shift, save_mean, save_invstd, nullptr, nullptr, nullptr, nullptr, nullptr, dy,
                                       w.sums, N, Cout, plane, st)))
        return rc;
    if ((rc = launch_bn_bwd_finalize(w.sums, 1, (double)N * plane, bn_weight, save_invstd, dgamma, dbeta, w.coef, Cout, st, p.frozen)))
        return rc;
    if ((rc = launch_bn_relu_bwd_apply(z, w.scale, w.shift, save_mean, save_invstd, nullptr, nullptr, nullptr, nullptr, nullptr, dy,
                                       w.coef, nullptr, w.dz, nullptr, dbias ? w.bsum : nullptr, N, Cout, plane, st)))
        return rc;
    if (dbias && (rc = launch_doubles_to_floats(w.bsum, dbias, Cout, st))) return rc;
    const float *dz = w.dz;         // the gradient tensor the two conv gradients read: p.Tz frames at p.stride
    if (p.upsampled) {
        if ((rc = launch_upsample2(w.dz, w.dzu, (size_t)N * Cout, p.Tout, T, V, st))) return rc;
        dz = w.dzu;
    }
    if (dx != nullptr && p.dgrad_by_forward) {   // dx = conv_t(dz, flipped W): the forward kernels, raw output
        if ((rc = launch_fill_ones_zeros(w.ones, w.zeros, Cin, st))) return rc;
        if ((rc = launch_weight_flip(W, w.Wf, Cout, Cin, K, st))) return rc;
        if ((rc = launch_tcn_pack(p.dgrad.pack, w.Wf, w.ones, w.packed, Cout, Cin, K, st))) return rc;
        if ((rc = launch_tcn(p.dgrad, dz, w.packed, w.zeros, dx, N, Cout, Cin, p.Tz, V, K, 1, p.dgrad_flags, st))) return rc;
    } else if (dx != nullptr) {
        if ((rc = launch_tcn_dgrad_valu(dz, W, dx, N, Cin, Cout, T, V, K, p.stride, p.Tz, st))) return rc;
    }
    return launch_tcn_wgrad(dz, x, dW, w.part, N, Cin, Cout, T, V, K, p.stride, p.Tz, p.flags, st);
}

}  // namespace stgcn
