// Token-major linear layer of the AltFormer heads' transformer blocks (model/AltFormer/model_ST.py:18-88):
//     Y (M, Nout) = act(LN?(X) W^T + b) (+ R),   X (M, K) and W (Nout, K) both K-contiguous (nn.Linear.weight as stored).
// These are plain large GEMMs (M = 126,720 tokens at batch 32, K = 256 or 512), so the tiling is the usual one and not
// gemm_f32.hip's small strided-batched one: a workgroup of 4 waves owns a 128 x 128 tile of Y, each wave a 64 x 64 quarter
// (2 x 2 MFMA blocks of 32 x 32, 64 accumulator registers), K in chunks of 32 through LDS with the next chunk's global
// loads in flight while the current one multiplies.  Tiles are numbered with the Nout tiles fastest, so the workgroups
// that share a 128-row slab of X run together and the slab is read from HBM once.
//
// Three arithmetics (STGCN_MATH_*):
//   f32    : v_mfma_f32_32x32x2_f32 on the fp32 tiles (exact products, fp32 accumulate);
//   bf16x3 : both tiles are split into bf16 hi + lo while they are staged (the weights too: the split of a 128 x 32 weight
//            chunk is 16 values per thread and hides under the 24 MFMAs of the chunk, so there is no packed weight format
//            and nothing to cache on the host), then lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_bf16;
//   bf16   : (the block's STGCN_VIT_BF16 and STGCN_VIT_TRAIN_BF16 modes) both operands rounded to nearest-even bf16 while
//            they are staged, one LDS tile per operand, one v_mfma_f32_32x32x16_bf16 per k-step and block, fp32 accumulate.
//            X is fp32 (rounded after the LayerNorm) or already bf16 in memory (XB: 8-byte loads that go to LDS as they
//            are), Y is stored as fp32 or as bf16 (YB); bias, GELU and residual stay fp32.  The k pairs, instructions and
//            their order do not depend on the tile form here either, so the three forms agree bit for bit.
// The k index inside a chunk is permuted the same way for both operands (a dot product does not care): lanes 0-31 of an
// MFMA take the first half of the chunk / k-step and lanes 32-63 the second, so every fragment is a run of consecutive
// LDS bytes read with 16-byte loads.  Row strides (36 floats, 40 bf16) make those loads bank-conflict free.
//
// LayerNorm: every workgroup first takes the (mean, rstd) of its 128 rows (see the kernel) and applies them to the A tile
// between the global load and the LDS store, so the normalised tensor never exists in memory.
// No atomics anywhere: one thread owns each output element and sums in a fixed order.
// Training (vit_block_train.hip) runs this kernel too: the forward with LinearExtra's pre-activation store and row factor,
// the dgrads as this linear on a transposed weight with the GELU' and row-factor steps of the epilogue (vit.h).
//
// Tile forms (Form below; vit.h's linear_tile chooses): the kernel is one template over the waves of a workgroup and the
// 32 x 32 blocks of a wave.  128 x 128 is the form described above; 64 x 64 (4 waves, one block each) and 32 x 64 (2 waves,
// one block each) exist for calls too small to fill the part with 128 x 128 tiles (one clip: 62 of them in a proj linear).
// A form only changes which workgroup and wave owns a 32 x 32 block of Y: the block's accumulator sees the same k pairs in
// the same MFMA instructions in the same order, and a row's LayerNorm statistics are the same 8-thread sums and three
// exchanges, so every form's result is bit-identical to the 128 x 128 form's.
#include "vit_linear_kernel.h"

namespace stgcn {
namespace vit {

namespace {

using namespace linear_kernel;

template <int MATH, class F, bool XB = false, bool YB = false>
int launch_form(const void *X, const float *W, const float *bias, const float *R, const float *gamma, const float *beta, float eps,
                void *Y, int M, int K, int Nout, bool gelu, const LinearExtra &ex, hipStream_t st) {
    const int tiles_n = ceil_div(Nout, F::BN);
    const long long tiles = (long long)tiles_n * ceil_div(M, F::BM);
    if (!grid_fits(tiles, F::THREADS)) return fail(STGCN_ERR_UNSUPPORTED, "vit linear: %lld tiles", tiles);
    vit_linear_kernel<MATH, F, XB, YB><<<dim3((unsigned)tiles), dim3(F::THREADS), 0, st>>>(X, W, bias, R, gamma, beta, eps, Y, M, K, Nout,
                                                                                 tiles_n, gelu, ex, DenseRows{});
    STGCN_LAUNCH_CHECK("vit_linear_kernel");
    return STGCN_OK;
}

template <int MATH, bool XB = false, bool YB = false>
int launch_math(const LinearTile t, const void *X, const float *W, const float *bias, const float *R, const float *gamma,
                const float *beta, float eps, void *Y, int M, int K, int Nout, bool gelu, const LinearExtra &ex, hipStream_t st) {
    static_assert(Form128::BM == 128 && Form128::BN == 128 && Form64::BM == 64 && Form64::BN == 64 && Form32::BM == 32 &&
                  Form32::BN == 64, "the forms linear_tile (vit.h) plans with");
    if (t.bm == Form128::BM) return launch_form<MATH, Form128, XB, YB>(X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st);
    if (t.bm == Form64::BM) return launch_form<MATH, Form64, XB, YB>(X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st);
    return launch_form<MATH, Form32, XB, YB>(X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st);
}

}  // namespace

int launch_linear(const void *X, const float *W, const float *bias, const float *R, const float *gamma, const float *beta,
                  float eps, void *Y, int M, int K, int Nout, bool gelu, unsigned mode, hipStream_t st, const LinearExtra &ex) {
    const unsigned math = mode & STGCN_MATH_MASK;
    const bool xb = (mode & STGCN_VIT_X_BF16) != 0, yb = (mode & STGCN_VIT_Y_BF16) != 0;
    if ((xb || yb) && math != STGCN_MATH_BF16) return fail(STGCN_ERR_UNSUPPORTED, "vit linear: bf16 storage needs the bf16 arithmetic");
    if (xb && gamma != nullptr) return fail(STGCN_ERR_UNSUPPORTED, "vit linear (bf16): LayerNorm needs fp32 rows");
    const LinearTile t = linear_tile(M, K, Nout, mode);
    if (math == STGCN_MATH_F32) return launch_math<STGCN_MATH_F32>(t, X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st);
    if (math != STGCN_MATH_BF16) return launch_math<STGCN_MATH_BF16X3>(t, X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st);
    constexpr int B = STGCN_MATH_BF16;   // fp32 or bf16 storage on either side
    if (xb)
        return yb ? launch_math<B, true, true>(t, X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st)
                  : launch_math<B, true, false>(t, X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st);
    return yb ? launch_math<B, false, true>(t, X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st)
              : launch_math<B, false, false>(t, X, W, bias, R, gamma, beta, eps, Y, M, K, Nout, gelu, ex, st);
}

}  // namespace vit
}  // namespace stgcn
