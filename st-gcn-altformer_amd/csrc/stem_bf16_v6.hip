// KF6, narrow frames (V <= 32): the headline fused stem.  The kernel, its plan and its launcher live in kf6.h (read that
// first); this translation unit instantiates the narrow form and holds KF6's weight packing.
#include "kf6.h"

namespace stgcn {

namespace {

// weight packing for KF6: Wq (bf16) index ((((ob*npairs + q)*2 + img)*64 + lane)*8 + j
//   o = ob*16 + (lane&15); step f = 2q + (lane>>5); chunk f/9, tap f%9; c = chunk*16 + 8*((lane>>4)&1) + j
// (the order of tcn_pack_pairs_padded_kernel, tcn_bf16_v6.hip, but NOT its bytes: here the compiler contracts the lo image's
//  residual scale*W - hi into one fma, there the product is rounded first, and one lo value in a few hundred differs in its last
//  bit.  The fused stem keeps this packing so that KF6 / KF6w read the bytes they always have.)
__global__ void tcn_pack_bf16_pairs_kernel(const float *__restrict__ W, const float *__restrict__ scale,
                                           unsigned short *__restrict__ Wq, int Cin, int Cout) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;  // one thread per (weight, img)
    if (e >= (size_t)Cout * Cin * KT6 * 2) return;
    const int j = (int)(e & 7);
    const int lane = (int)((e >> 3) & 63);
    size_t r = e >> 9;
    const int img = (int)(r & 1);
    r >>= 1;
    const int npairs = Cin / CCB * KT6 / 2;
    const int q = (int)(r % npairs);
    const int ob = (int)(r / npairs);
    const int o = ob * 16 + (lane & 15);
    const int f = 2 * q + (lane >> 5);
    const int c = (f / KT6) * CCB + 8 * ((lane >> 4) & 1) + j, tap = f % KT6;
    const float w = scale[o] * W[((size_t)o * Cin + c) * KT6 + tap];
    const unsigned h = pack_bf16x2(w, 0.f) & 0xffffu;
    const unsigned l = pack_bf16x2(w - bf16_lo_to_f32(h), 0.f) & 0xffffu;
    Wq[e] = (unsigned short)(img ? l : h);
}

}  // namespace

bool stem_v6_supported(int C, int T, int V, int K, unsigned flags) { return stem_v6_form_supported<false>(C, T, V, K, flags); }

int stem_v6_short_tile_blocks(int C, int T, int V, int K) {
    V6Plan pl;
    return T >= 1 && plan_v6_narrow(C, T, V, K, 3, pl) && pl.short_last ? pl.short_blocks : 0;
}

void stem_v6_walk_run(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *first, int *end) {
    const int ntiles = nclips * tiles_per_clip, G = ntiles < num_wg ? ntiles : num_wg;   // (the launch's grid)
    const V6Run r = wg < G ? v6_run(wg, G, nclips, tiles_per_clip, short_last) : V6Run{ntiles, ntiles};
    *first = r.first;
    *end = r.end;
}

// the tiles of workgroup wg in the order the kernel walks them (v6_order: two store phases); returns their number and writes
// the first `cap` of them
int stem_v6_walk_order(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *tiles, int cap) {
    const int ntiles = nclips * tiles_per_clip, G = ntiles < num_wg ? ntiles : num_wg;   // (the launch's grid)
    const V6Run r = wg < G ? v6_run(wg, G, nclips, tiles_per_clip, short_last) : V6Run{ntiles, ntiles};
#ifndef V6_ONE_STORE_PHASE
    const V6Order o = v6_order(wg, r, tiles_per_clip, short_last);
#else
    const V6Order o = V6Order{-1};
#endif
    int n = 0;
    for (int t = v6_order_start(r, o); t < r.end; t = v6_order_next(t, r.first, o.ts), ++n)
        if (n < cap) tiles[n] = t;
    return n;
}

// temporal weights (Cout,Cin,9) * scale -> KF6's pair order (same size as the 32x32x16 packing)
int launch_tcn_pack_bf16_pairs(const float *W, const float *scale, void *Wq, int Cin, int Cout, hipStream_t st) {
    const size_t total = (size_t)Cin * Cout * KT6 * 2;
    hipLaunchKernelGGL(tcn_pack_bf16_pairs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, scale,
                       (unsigned short *)Wq, Cin, Cout);
    STGCN_LAUNCH_CHECK("tcn_pack_bf16_pairs_kernel");
    return STGCN_OK;
}

int launch_stem_v6(const float *x, bool x_ntvc, const void *pfrag, const void *prep_w12, const void *Wq, const float *shift,
                   void *out, int N, int C, int T, int V, int K, unsigned flags, hipStream_t st) {
    return launch_stem_v6_form<false>(x, x_ntvc, pfrag, prep_w12, Wq, shift, out, N, C, T, V, K, flags, st);
}

}  // namespace stgcn
