// Graph conv (unit_agcn) forward, host side: the two plans every entry point and size query reads — which kernel and
// instantiation compute the attention matrices (K1, agcn_attention.hip) and the aggregation + expansion (K2,
// agcn_expand.hip) of a shape, with what geometry, or why none does.  The kernels' coverage predicates are called here only.
#include <stdarg.h>
#include <string.h>

#include "common.h"

namespace stgcn {

template <class Plan>
static Plan refuse(Plan p, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.why.msg, sizeof(p.why.msg), fmt, ap);
    va_end(ap);
    p.why.status = STGCN_ERR_UNSUPPORTED;
    p.kernel = decltype(p.kernel)::none;
    return p;
}

// Kernels, first that covers: the folded form (Cin <= 4: the stem), the only one with outputs besides P; the generic form on
// the matrix cores; the generic VALU form.  Diagnostic builds: ablation bit 2048 keeps the VALU form where the MFMA one would run.
AttentionPlan plan_attention(int N, int Cin, int T, int V, int inter_c, int S, AttentionOut want) {
    AttentionPlan p;
    p.out = want, p.N = N, p.Cin = Cin, p.T = T, p.V = V, p.inter_c = inter_c, p.S = S;
    const bool features = want.kind == AttentionOut::features, frags = want.kind == AttentionOut::frags;
    const int v0 = want.split, v1 = V - want.split;
    if (N > kMaxGridClips) return refuse(p, "attention: N=%d > %d clips per call", N, kMaxGridClips);
    if (V > kAttentionMaxV) return refuse(p, "attention: V=%d too large (max %d)", V, kAttentionMaxV);
    if (frags && (!agcn_stem_class(Cin, S) || (v0 == 0 && V > 32)))
        return refuse(p, "attention: fragment output covers Cin=3, 3 subsets, V<=32 (got %d, %d, %d)", Cin, S, V);
    if (frags && v0 != 0 && (v0 < 1 || v0 > 32 || v1 < 1 || v1 > 32))
        return refuse(p, "attention: joint split %d | %d outside 1..32 per half", v0, v1);
    if (features && !agcn_stem_class(Cin, S))
        return refuse(p, "attention: the feature pass covers Cin=3, 3 subsets (got %d, %d)", Cin, S);
    if (attention_folded_covers(N, Cin, T, V, inter_c, S, features, p.tile)) {
        if (want.bounds && S * V > 512) return refuse(p, "attention: no bound output for V=%d", V);
        p.kernel = AttentionKernel::folded;
        return p;
    }
    if (features) return refuse(p, "attention: V=%d too large for the feature pass", V);
    if (frags) return refuse(p, "attention: V=%d outside the folded kernel", V);
    if (want.bounds) return refuse(p, "attention: no bound output for V=%d", V);
    if (!(ablate_mask() & 2048) && attention_generic_mfma_covers(N, Cin, T, V, inter_c, S, p.tile)) {
        p.kernel = AttentionKernel::generic_mfma;
        return p;
    }
    if (!attention_generic_valu_covers(N, Cin, T, V, inter_c, S, p.tile))
        return refuse(p, "attention: Cin=%d inter_c=%d V=%d needs %zu B of LDS", Cin, inter_c, V, p.tile.lds);
    p.kernel = AttentionKernel::generic_valu;
    return p;
}

// Kernels, first that covers: the two folded forms of the stem class with a down branch (16-byte stores, else scalar), the
// matrix-core form (Cin % 16 == 0, 64 / 128 / 256 output channels), the generic VALU form.  Diagnostic builds: ablation bit
// 4096 keeps the VALU form where the MFMA one would run.
ExpandPlan plan_agcn_expand(int N, int Cin, int Cout, int T, int V, int S, bool has_down) {
    ExpandPlan p;
    p.N = N, p.Cin = Cin, p.Cout = Cout, p.T = T, p.V = V, p.S = S;
    if (N > kMaxGridClips) return refuse(p, "agcn: N=%d > %d clips per call", N, kMaxGridClips);
    p.kernel = agcn_expand_small4_covers(N, Cin, Cout, T, V, S, has_down, p.tile)  ? ExpandKernel::small4
               : agcn_expand_small_covers(N, Cin, Cout, T, V, S, has_down, p.tile) ? ExpandKernel::small
               : !(ablate_mask() & 4096) && agcn_expand_mfma_covers(N, Cin, Cout, T, V, S, p.tile) ? ExpandKernel::mfma
               : agcn_expand_generic_covers(N, Cin, T, V, S, p.tile)                ? ExpandKernel::generic
                                                                                     : ExpandKernel::none;
    if (p.kernel == ExpandKernel::none) return refuse(p, "agcn: Cin=%d V=%d does not fit LDS", Cin, V);
    return p;
}

// every (kernel, instantiation) the two plans can name: 6 + 6 + 4 of the attention, 6 of the expansion
static const char *const kKernelNames[] = {
    "attention_folded_kernel<1,16>", "attention_folded_kernel<2,16>", "attention_folded_kernel<4,16>",
    "attention_folded_kernel<2,8>", "attention_folded_kernel<6,8>", "attention_folded_kernel<12,8>",
    "attention_generic_mfma_kernel<16,1>", "attention_generic_mfma_kernel<32,1>", "attention_generic_mfma_kernel<64,1>",
    "attention_generic_mfma_kernel<16,2>", "attention_generic_mfma_kernel<32,2>", "attention_generic_mfma_kernel<64,2>",
    "attention_generic_kernel<2>", "attention_generic_kernel<4>", "attention_generic_kernel<9>", "attention_generic_kernel<16>",
    "agcn_expand_small4_kernel<3,3>", "agcn_expand_small_kernel<3,3>", "agcn_expand_mfma_kernel<1,8>",
    "agcn_expand_mfma_kernel<1,16>", "agcn_expand_mfma_kernel<2,16>", "agcn_expand_generic_kernel"};

static const char *listed(const char *name) {
    for (const char *n : kKernelNames)
        if (strcmp(n, name) == 0) return n;
    return "";
}

const char *attention_kernel_name(const AttentionPlan &p) {
    const AttentionTile &t = p.tile;
    char b[64] = "";
    switch (p.kernel) {
    case AttentionKernel::folded: snprintf(b, sizeof(b), "attention_folded_kernel<%d,%d>", t.maxb, t.nw); break;
    case AttentionKernel::generic_mfma: snprintf(b, sizeof(b), "attention_generic_mfma_kernel<%d,%d>", t.ks, t.mb); break;
    case AttentionKernel::generic_valu: snprintf(b, sizeof(b), "attention_generic_kernel<%d>", t.maxit); break;
    case AttentionKernel::none: break;
    }
    return listed(b);
}

const char *expand_kernel_name(const ExpandPlan &p) {
    char b[64] = "";
    switch (p.kernel) {
    case ExpandKernel::small4: return listed("agcn_expand_small4_kernel<3,3>");
    case ExpandKernel::small: return listed("agcn_expand_small_kernel<3,3>");
    case ExpandKernel::mfma: snprintf(b, sizeof(b), "agcn_expand_mfma_kernel<%d,%d>", p.tile.now, p.tile.npb); break;
    case ExpandKernel::generic: return listed("agcn_expand_generic_kernel");
    case ExpandKernel::none: break;
    }
    return listed(b);
}

// True when the attention can also emit the (N, T*V, 16) feature tensor.  T does not enter: each folded form fits LDS for
// every T or for none (its frame chunk is cut to the room the Gram and weight images leave).  inter_c does, above 1360 (the
// LDS copy of the embedding weights outgrows the 512-thread form); the fused stem's plan has no inter_c, so this asks for
// unit_agcn's 32 as it always has, and plan_attention refuses the wider call.
bool attention_emits_features(int Cin, int V, int S) {
    AttentionOut want;
    want.kind = AttentionOut::features;
    return plan_attention(1, Cin, 1, V, 32, S, want).kernel == AttentionKernel::folded;
}

}  // namespace stgcn
