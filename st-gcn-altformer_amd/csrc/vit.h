// Launchers of the AltFormer heads' transformer-block kernels (vit_linear.hip, vit_attention.hip), shared with the
// block entry point in vit_block.hip.  All enqueue on `st` and return a stgcn_status.
#pragma once

#include "common.h"

namespace stgcn {
namespace vit {

constexpr int kMaxL = 256;      // longest sequence the attention kernel keeps on chip

// Y (M, Nout) = act(LN?(X) W^T + bias) (+ R).  X (M, K), W (Nout, K), K % 32 == 0.  gamma / beta / eps: LayerNorm of X's
// rows applied while the A tile is staged (gamma == nullptr: none).  math: STGCN_MATH_F32 or STGCN_MATH_BF16X3.
// Y may alias R (each element is read and written by one thread); it must not alias X.
int launch_linear(const float *X, const float *W, const float *bias, const float *R, const float *gamma, const float *beta,
                  float eps, float *Y, int M, int K, int Nout, bool gelu, unsigned math, hipStream_t st);

// out (B, L, H*hd) = softmax(scale * q k^T) v per (sequence, head) of the packed qkv (B, L, 3, H, hd); hd in {32, 64},
// L <= kMaxL.
int launch_attention_packed(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st);

}  // namespace vit
}  // namespace stgcn
