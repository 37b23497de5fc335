// KF6 for wide frames (32 < V <= 64 joints, the two-hand graph): the kernel of kf6.h instantiated with the joint axis split
// into two halves (see the WIDE notes at the head of KF6 there).  A translation unit of its own so that the wide
// instantiation and the headline kernel do not share a register-allocation context.
#include "kf6.h"

namespace stgcn {

bool stem_v6w_supported(int C, int T, int V, int K, unsigned flags) { return stem_v6_form_supported<true>(C, T, V, K, flags); }

int launch_stem_v6w(const float *x, bool x_ntvc, const void *pfrag, const void *prep_w12, const void *Wq, const float *shift,
                    void *out, int N, int C, int T, int V, int K, unsigned flags, hipStream_t st) {
    return launch_stem_v6_form<true>(x, x_ntvc, pfrag, prep_w12, Wq, shift, out, N, C, T, V, K, flags, st);
}

}  // namespace stgcn
