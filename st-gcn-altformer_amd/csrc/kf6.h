// The one-wave-per-SIMD form: 256 threads, 4 waves, a wave owns all 128 output channels of 64 pixels of a 256-pixel tile, on
// v_mfma_f32_16x16x32_bf16 with a slot-structured main loop and a weight ring filled by LDS-DMA.  KF6 (the headline fused
// stem, below), KF7 (stem_f16mx.hip), K3v6 (tcn_bf16_v6.hip) and the temporal conv's weight gradient (tcn_wgrad_v6.hip)
// are built in this form.  This header holds:
//   * what they share: the tile constants, the LDS-DMA helper, the vmcnt waits, FragB6, TileInfo6, relu1 and
//     the cycle-stamp macros of the diagnostic builds (static_for comes from bf16_common.h);
//   * the KF6 kernel template and the host plans of the fused stem (narrow and wide frames; KF7 runs the narrow plan with
//     three terms).  stem_bf16_v6.hip instantiates KF6's narrow form, stem_bf16_v6w.hip its wide form: one translation
//     unit per form, so that neither perturbs the other's code generation.
// Included once per translation unit (it includes bf16_common.h); everything sits in an anonymous namespace.
#pragma once

#include <type_traits>

#include "bf16_common.h"

namespace stgcn {

namespace {

using namespace bf16k;

constexpr int NP6 = 256;   // output pixels per tile
constexpr int NT6 = 256;   // threads per workgroup: one wave per SIMD
constexpr int KT6 = 9;     // temporal taps
constexpr int FRAG6 = 1024;
constexpr int PAIR6 = 16 * FRAG6;   // weights of one pair: 8 blocks of 16 channels x (hi, lo)
constexpr int RING6 = 3 * PAIR6;
constexpr int EPI6 = 4096; // epilogue staging per wave: 16 channels x 64 pixels fp32

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __attribute__((address_space(3))) void *lptr6_t;

__device__ __forceinline__ void dma16v6(const void *g, unsigned lds_addr) {
    // M0 = LDS destination (wave-uniform).  M0 is declared clobbered instead of saved and restored around every transfer:
    // nothing else in these kernels lives in M0, and the three extra scalar instructions per transfer are not free when a
    // single wave owns the SIMD (they sit in the MFMA stream).
    const unsigned lds = __builtin_amdgcn_readfirstlane(lds_addr);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(g), "s"(lds) : "memory", "m0");
}
// wait until at most N vector-memory operations (LDS-DMAs and loads, in issue order) are in flight
template <int N>
__device__ __forceinline__ void vm_wait_keep() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

struct FragB6 { uint4 hi[4], lo[4]; };     // activations of one pair: 4 pixel blocks of 16

struct TileInfo6 {
    int n, Vh, j0, half;
    TileGeomB g;
};

// max(x, 0) as ONE instruction in the producer's slots, and one that keeps a NaN (common.h: max_nan): v_maximum3_f32 x, 0, 0
__device__ __forceinline__ float relu1(float x) { return max_nan(x, 0.f); }

// ---- the balanced walk of KF6's narrow three-term form --------------------------------------------------------------------
// A clip whose last tile holds at most 128 pixels ends in a SHORT tile (half the pixel blocks per wave, see the kernel).  With
// the grid-stride walk and tiles_per_clip dividing the grid, workgroup b only ever sees tile position b % tiles_per_clip: a
// few workgroups would get nothing but short tiles and the others none, and the kernel ends with the others.  So such shapes
// are walked in contiguous, clip-major runs balanced by cost: a full tile costs 2 units, a short one 1, a clip P = 2 tpc - 1,
// and tile L = k * tpc + r starts at cost position k * P + 2 r (the "boundaries": the positions q with (q mod P) even).
// Workgroup b of G takes the tiles between boundaries B(b) and B(b + 1), with B(0) = 0, B(G) = the total, and in between by
// bisection: the middle workgroup of a range starts at the boundary nearest to the range's cost-proportional split point.
// Rounding each B(b) on its own from b * total / G (the tiles that start in the workgroup's 1/G share) leaves runs up to 1.5
// tiles apart in cost, because a full tile that straddles a target moves it by a whole unit at either end of a run; halving
// the range first keeps every workgroup within one full tile of every other (tests/test_stem_walk_host.py holds it to that),
// and whole clips per workgroup (the headline: one each) come out exactly.  With ntiles <= G (the launch then has G = ntiles)
// it is one tile each.  short_last = 0: every tile costs 2, the same rule gives equal counts.  Scalar code, at most
// log2(G) steps, twice per workgroup, in front of the tile loop; the host test reaches the same function through
// stgcn_stem_walk_run.
constexpr int OPT_V6_SHORT = 1 << 17;   // (kernel option bit beside OPT_OUT_NTVC) the clip's last tile takes the short form
struct V6Run { int first, end; };
// I: int where 2 * total * G fits it (every real shape), else long long
template <typename I>
__host__ __device__ inline I v6_walk_bound(int b, int G, I total, int P) {
    int lo = 0, hi = G;
    I plo = 0, phi = total;
    while (true) {
        if (b == lo) return plo;
        if (b == hi) return phi;
        const int m = hi - lo;
        const I span = phi - plo;
        // whole clips per workgroup from a clip's start: the split points are boundaries all the way down
        if (plo % P == 0 && span % ((I)m * P) == 0) return plo + (I)(b - lo) * (span / m);
        const int mid = (lo + hi) >> 1;
        const I num = span * (mid - lo);                       // split point: plo + num / m
        I off = (2 * num + m) / (2 * m);                       // ... rounded to a position,
        if (((plo + off) % P) & 1) off += num <= off * m ? -1 : 1;   // ... from inside a full tile to its nearer end
        if (b < mid) { hi = mid; phi = plo + off; }
        else { lo = mid; plo = plo + off; }
    }
}
__host__ __device__ inline V6Run v6_run(int b, int G, int nclips, int tpc, int short_last) {
    if (nclips * tpc <= G) return V6Run{b, b + 1};
    const int P = 2 * tpc - (short_last ? 1 : 0);             // cost of a clip
    const long long total = (long long)nclips * P;
    long long q0, q1;
    if (total <= (0x7fffffffLL - G) / (2 * G)) {
        q0 = v6_walk_bound<int>(b, G, (int)total, P);
        q1 = v6_walk_bound<int>(b + 1, G, (int)total, P);
    } else {
        q0 = v6_walk_bound<long long>(b, G, total, P);
        q1 = v6_walk_bound<long long>(b + 1, G, total, P);
    }
    // position -> tile: clip q / P, tile (q mod P) / 2 of it
    return V6Run{(int)(q0 / P * tpc + q0 % P / 2), (int)(q1 / P * tpc + q1 % P / 2)};
}

// ---- the ORDER in which a workgroup walks its run: two store phases ---------------------------------------------------------
// Every full tile costs every workgroup the same, so walked alike all workgroups reach their epilogues together and the chip
// takes their result stores as one burst per tile ("Two store phases").  The workgroups are therefore split
// into two classes, cls = (b >> 3) & 1: workgroups are dealt round-robin over the 8 XCDs, b and b + 8 share one, so a class that
// is a function of b mod 2 / 4 / 8 would give all workgroups of an XCD the same phase; bit 3 puts half of every XCD's workgroups
// into each class wherever workgroup 0 lands.  Class 0 walks its run in order.  Class 1 walks the first SHORT tile of its run
// first and then the rest in order: a short tile costs 0.75 of a full one, so from its second tile on a class-1 workgroup stores
// a quarter of a tile ahead of class 0, and both classes do the same work (no delay, no idle time, the same tiles, each with
// its own accumulation order and bits).  A run without a short tile, or one that begins with it, is walked in order.
// V6Order::ts = the short tile walked first, -1 where the run is walked in order; the walk is
//     t = v6_order_start(run, o);  while (t < run.end) { ...; t = v6_order_next(t, run.first, o.ts); }
// (next(ts) = first, next(ts - 1) = ts + 1, else t + 1: the walk always ends at exactly run.end).  The kernel and the host test
// (stgcn_stem_walk_order) share these functions.
struct V6Order { int ts; };
__host__ __device__ inline int v6_store_class(int b) { return (b >> 3) & 1; }
__host__ __device__ inline V6Order v6_order(int b, V6Run run, int tpc, int short_last) {
    if (!short_last || !v6_store_class(b)) return V6Order{-1};
    const int ts = run.first + (tpc - 1 - run.first % tpc);   // the first tile at or behind run.first that ends a clip
    return V6Order{ts > run.first && ts < run.end ? ts : -1};
}
__host__ __device__ inline int v6_order_start(V6Run run, V6Order o) { return o.ts >= 0 ? o.ts : run.first; }
__host__ __device__ inline int v6_order_next(int t, int first, int ts) { return t == ts ? first : (t == ts - 1 ? ts + 1 : t + 1); }

#ifdef STGCN_ABLATION  // in-kernel cycle stamps of KF6 and KF7 (diagnostic builds only; dbg == NULL otherwise)
#define V6_STAMP(var) unsigned long long var = 0; if (dbg) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory"); }
#define V6_ACC(slot, a, b) if (dbg) { tsum[slot] += (b) - (a); }
#else
#define V6_STAMP(var)
#define V6_ACC(slot, a, b)
#endif

// ---- KF6 ------------------------------------------------------------------------------------------------------------------
// KF6 — the fused stem on the bf16 matrix cores with ONE WAVE PER SIMD (256 threads, 4 waves, up to 512 registers each) on
// v_mfma_f32_16x16x32_bf16.  Headline kernel for V <= ~25 (the 256-pixel tile); KF4 (stem_bf16_v4.hip) keeps the rest.
//
// Same tile, LDS images, in-kernel feature computation and producer as KF4's FK form — what changes:
//   * ownership: a wave owns ALL 128 output channels of its 64-pixel quarter (8 x 4 accumulator blocks of 16 x 16 = 128
//     registers).  Every weight fragment is read once by each of 4 waves instead of twice by 8, an activation fragment feeds
//     eight channel blocks: LDS read traffic per MFMA is halved; and there is no second wave on the SIMD to lose matrix-pipe
//     arbitration to (KF4's older waves ran ahead and then waited 23 % of their time at the stage barriers).
//   * with nothing else on the SIMD, clumps of other instructions between MFMAs are no longer hidden, so the loop is written
//     as SLOTS: one MFMA followed by at most a couple of fillers (compile-time loop over the slots, sched_barrier(0) after
//     each; the `filler` lambda says which filler sits in which slot), no branches, as little scalar work as possible
//     (division-free ring counters, M0 clobbered rather than saved around an LDS-DMA).  The first version of this kernel
//     with KF4's fenced phases was 2.7 % SLOWER than KF4 (hipcc gathers 30-40 instructions between groups of MFMAs); a
//     uniform branch per producer piece cost 5 %.
//   * the MFMA shape: the kernel runs at the rate the chip sustains for issued bf16 MFMA on random operands (power-limited,
//     DESIGN.md section 3), so what is left is energy per FLOP: the 16x16x32 form delivers ~1.12-1.15x the FLOP/s of
//     32x32x16 under that limit (MI355X_MICROARCH.md "DVFS give-back" (7); this pool: 1,836 vs 1,644 TFLOP/s with this
//     kernel's LDS operand traffic, tools/micro/mfma_shape.hip) — measured here as an 11 % higher clock at equal wall time
//     before the scalar work was trimmed, 2.8 % faster than the same kernel on 32x32x16 after.
//
// K = 32 of one MFMA = 16 channels x TWO consecutive k-steps of the flat (16-channel chunk, tap) sequence.  A tile has
// nch * 9 steps (72: even), so steps pair up without padding; every second chunk boundary falls inside a pair
// (tap 8 of chunk c with tap 0 of chunk c+1: the two lane halves of a B fragment then read different image buffers).
// The loop is written per PERIOD of 9 pairs = 2 chunks (static taps, static buffers), periods in a dynamic loop:
//   pairs 0-2 produce chunk 2p+1 into buf1, pair 4 straddles, pairs 5-7 produce chunk 2p+2 into buf0 — one pair before
//   the chunk's first reader, so that the reader's activation fragments can be prefetched across the barrier.
//   A wave produces 3 + 3 + 2 sixteen-pixel blocks per window from the image's first row or, where the host plan has shown
//   that no tile's taps read more than 28 blocks (v6_blocks_read), 3 + 2 + 2 from the block of the tile's first pixel (NPBW).
// Weights: repacked per pair ([16-channel block][pair][hi|lo][lane] x 16 B, stgcn_stem_prepare), ring of 3 pair slots
// (16 KiB each) filled by LDS-DMA two pairs ahead — issued early in a pair, waited for (vmcnt(0)) at its end, so that at a
// pair's start BOTH the current and the next pair are resident and published: the next pair's first fragments are read
// before the barrier, no pair opens with an exposed LDS read.  A wave keeps only the current and the next 16-channel
// block's weight fragments in registers (read one block ahead of use).
// Per-tile tail: epilogue staged 16 channels x 64 pixels at a time through LDS (16-byte stores, scalar base + one per-lane
// term), next tile's x loads in flight during the stores, feature phase, chunk-0 production.
//
// WIDE (stem_bf16_v6w.hip): frames of 32 < V <= 64 joints (the two-hand graph, V = 46).
// The temporal conv never mixes joints, so the joint axis is cut into two halves [0, V0) and [V0, V) (V0 a multiple of 4,
// both halves <= 32 joints) and each (clip, half) is walked like a narrow clip of Vh joints: same tile, images, producer
// and main loop.  What differs sits in the per-tile tail only: the aggregation u_s = x P_s sums over ALL V joints (two
// k-steps of 32 per feature MFMA; 24 attention fragments per half, which live in the idle second image buffer between
// the main loops instead of a region of their own), and the epilogue maps a half-space pixel (t, v') to the clip's
// (t, j0 + v'): pairs of pixels stay 8-byte aligned (V, V0 even), so rows go out as 8-byte stores.

// Result stores of the NARROW kernel's epilogue: NON-TEMPORAL (round 3).  The 0.5 GB of output per launch pass through the same
// 4 MiB L2s that serve the weight ring (2.4 GB per launch, re-read by every tile); streamed as `nt` whole 128-byte lines displace
// less of it.  Round 3 measured 0.9-1.7 % off the kernel in same-box A/Bs of two libraries (tools/ab_libs.sh; write-through
// `sc1` stores instead: 11 % slower) — on an epilogue in which every 16-channel block still waited for the previous block's
// stores; DESIGN section 3 ("The narrow kernel's tile tail") records where that A/B stands on the straight-line epilogue.
// The WIDE form keeps plain stores: its 8-byte pair stores fill a line from two workgroups a tile apart, and pushed out early
// as `nt` halves they measured 3 % slower.  -DV6_PLAIN_STORES builds the plain form for that A/B.
template <bool NT>
__device__ __forceinline__ void st_out4(float *p, const float4 &v) {
#ifndef V6_PLAIN_STORES
    if constexpr (NT) {
        using f32x4v = __attribute__((ext_vector_type(4))) float;
        __builtin_nontemporal_store(f32x4v{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4v *>(p));
        return;
    }
#endif
    *reinterpret_cast<float4 *>(p) = v;
}

// WIDE: V0 = joints of the first half, tpc1 = tiles of a clip's second half (tiles_per_clip counts both halves)
// NPBW: producer blocks per wave and chunk.  8 (3 + 3 + 2 per window) covers every image the plan admits, counted from the
// image's first row; 7 (3 + 2 + 2) counts from the first block a tap of the tile reads (pb0) and is chosen by the host plan
// for the shapes in which no tile's taps read more than 28 blocks from there on (v6_blocks_read): what the frame-aligned image
// holds behind them is then not produced either.
// PIXROWS (narrow three-term form, (N,C,T,V) output; launch_v6 chooses it): the consumer MFMAs take the activations as their A
// and the weights as their B operand, from the same registers.  A lane then ends up with four consecutive pixels of one
// channel instead of four channels of one pixel, and the epilogue stores them as they are (kf6_tile.h, "PIXROWS").
template <int TERMS, bool BF16OUT, bool WIDE, int NPBW = 8, bool PIXROWS = false>
__global__ __launch_bounds__(NT6) void stem_bf16_v6_kernel(
    const uint4 *__restrict__ pfrag, const float *__restrict__ x, int xsc, int xsp, const float *__restrict__ W12,
    const uint4 *__restrict__ Wp, const float *__restrict__ shift, void *y, int C, int T, int V, int ROWS,
    int tiles_per_clip, int ntiles, int abl, unsigned long long *dbg, int V0, int tpc1) {
#ifdef STGCN_ABLATION
    unsigned long long tsum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // [8 ..]: the short form's tiles
#endif
    extern __shared__ __attribute__((aligned(16))) char smem6[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // = pixel quarter of the tile
    const int TV = T * V;
    const int nch = C / CCB;                 // channel chunks (C = 128 -> 8)
    const int npairs = nch * KT6 / 2;        // K = 32 steps per tile (nch even: host side)
    const int img_bytes = ROWS * PXB;
    const int buf_bytes = img_bytes * (TERMS == 3 ? 2 : 1);
    // LDS carve: W12 (bf16 hi/lo) | weight ring (3 pairs) | images buf0, buf1 (= epilogue staging, 4 x 4 KiB) | Fs | Pf
    uint4 *W12q = reinterpret_cast<uint4 *>(smem6);
    char *ring = smem6 + C * W12P * 4;
    char *buf0 = ring + RING6;
    char *buf1 = buf0 + buf_bytes;
    uint4 *Fs = reinterpret_cast<uint4 *>(buf0 + max(2 * buf_bytes, 4 * EPI6));
    // WIDE, three-term arithmetic: the half's 24 fragments (24 KiB) sit in the second image buffer, which is idle from the
    // end of a tile's main loop to the next tile's first period (the budget has no 24 KiB of its own)
    const uint4 *Pf = (WIDE && TERMS == 3) ? reinterpret_cast<const uint4 *>(buf1) : Fs + 4 * ROWS;
    const unsigned lds0 = (unsigned)(size_t)(lptr6_t)smem6;
    const unsigned ring_lds = lds0 + (unsigned)(ring - smem6);
    const unsigned pf_lds = lds0 + (unsigned)(reinterpret_cast<const char *>(Pf) - smem6);

    const int cg = blockIdx.y;               // 128-channel group of the output
    // the four weight fragments this wave DMAs per pair: 16-channel blocks 2*wave, 2*wave+1, images hi and lo
    const uint4 *wsrc = Wp + ((size_t)(cg * 8 + 2 * wave) * npairs * 2) * 64 + lane;
    // fragment d = (block-in-wave, image) of weight pair `qsrc` (index within a tile's pairs) -> ring slot `slot`
    auto dma_frag = [&](int qsrc, int slot, int d) {
        const int bw = d >> 1, img = d & 1;
        dma16v6(wsrc + ((size_t)(bw * npairs + qsrc) * 2 + img) * 64, ring_lds + slot * PAIR6 + ((2 * wave + bw) * 2 + img) * FRAG6);
    };
    // tile -> clip, joint half and geometry.  WIDE: a clip's tiles alternate between the halves (half-0 tile i, half-1 tile i,
    // ...; the first half may own one more), so that the two column halves of a frame range are written close in time
    auto tile_info = [&](int tile) {
        TileInfo6 ti;
        ti.n = tile / tiles_per_clip;
        const int r = tile - ti.n * tiles_per_clip;
        int idx;
        if (r < 2 * tpc1) { ti.half = r & 1; idx = r >> 1; }
        else { ti.half = 0; idx = r - tpc1; }
        ti.Vh = ti.half ? V - V0 : V0;
        ti.j0 = ti.half ? V0 : 0;
        ti.g = tile_geom_b(idx, ti.Vh, KT6, 1, T, NP6);
        return ti;
    };
    auto dma_pfrag = [&](int tile) {         // 12 KiB: the clip's attention fragments -> Pf  (WIDE: the half's 24 KiB)
        if constexpr (WIDE) {
            const TileInfo6 ti = tile_info(tile);
            const uint4 *src = pfrag + ((size_t)ti.n * 48 + ti.half * 24) * 64 + lane;
#pragma unroll
            for (int i = 0; i < 6; ++i) dma16v6(src + (wave + 4 * i) * 64, pf_lds + (wave + 4 * i) * FRAG6);
        } else {
            const int n = tile / tiles_per_clip;
            const uint4 *src = pfrag + (size_t)n * 12 * 64 + lane;
#pragma unroll
            for (int i = 0; i < 3; ++i) dma16v6(src + (wave + 4 * i) * 64, pf_lds + (wave + 4 * i) * FRAG6);
        }
    };

    // ---- features of a tile from x and the clip's attention fragments (see stem_bf16_v4.hip, FK form) -------------
    struct XRegs { float xa[WIDE ? 16 : 8]; float xp[3]; };
    auto load_x = [&](XRegs &xr, int tile, int u) {
        int ln = tid & 63;                   // opaque per call: keeps lane-only address terms from being hoisted and spilled
        asm volatile("" : "+v"(ln));
        const int mb = u >> 1, hh = u & 1;
        TileInfo6 ti;
        if constexpr (WIDE) ti = tile_info(tile);
        else {
            ti.n = tile / tiles_per_clip;
            ti.g = tile_geom_b(tile - ti.n * tiles_per_clip, V, KT6, 1, T, NP6);
        }
        const int n = ti.n;
        const TileGeomB g = ti.g;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float *>(x + (size_t)n * 3 * TV), 0, (unsigned)(3 * TV * 4), 0x00020000);
        const int tf = g.t_first - (KT6 - 1) / 2 + 4 * mb;
        if constexpr (WIDE) {
            // (every offset is computed unconditionally and made opaque before the select: with the product inside the
            //  conditional hipcc turns each of the 19 selects into a branch around its load)
            const int k = ln & 3, t = tf + ((ln & 15) >> 2), v0 = 8 * (ln >> 4);
            const bool okr = (k < 3) & (t >= 0) & (t < T);
            unsigned base = (unsigned)((k * xsc + (t * V + v0) * xsp) * 4);
            asm volatile("" : "+v"(base));
#pragma unroll
            for (int j = 0; j < 16; ++j) {     // joints 0-31 and 32-63: the two k-steps of the aggregation
                const int dv = (j & 7) + 32 * (j >> 3);
                const unsigned off = (okr & (v0 + dv < V)) ? base + (unsigned)(dv * xsp * 4) : 0x7ffffff0u;   // (&: no short-circuit branch)
                xr.xa[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
            }
            const int t2 = tf + (ln >> 4), w = 16 * hh + (ln & 15);        // w: column within the half
            const bool ok = (t2 >= 0) & (t2 < T) & (w < ti.Vh);
            unsigned base2 = (unsigned)(((t2 * V + ti.j0 + w) * xsp) * 4);
            asm volatile("" : "+v"(base2));
#pragma unroll
            for (int k2 = 0; k2 < 3; ++k2) {
                const unsigned off = ok ? base2 + (unsigned)(k2 * xsc * 4) : 0x7ffffff0u;
                xr.xp[k2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
            }
        } else {
            {
                const int k = ln & 3, t = tf + ((ln & 15) >> 2), v0 = 8 * (ln >> 4);
                const bool okr = k < 3 && t >= 0 && t < T;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned off = (okr && v0 + j < V) ? (unsigned)((k * xsc + (t * V + v0 + j) * xsp) * 4) : 0x7ffffff0u;
                    xr.xa[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
                }
            }
            {
                const int t = tf + (ln >> 4), w = 16 * hh + (ln & 15);
                const bool ok = t >= 0 && t < T && w < V;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const unsigned off = ok ? (unsigned)((k * xsc + (t * V + w) * xsp) * 4) : 0x7ffffff0u;
                    xr.xp[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
                }
            }
        }
    };
    auto feature_unit = [&](const TileInfo6 &ti, int u, const XRegs &xr) {
        const TileGeomB &g = ti.g;
        int ln = tid & 63;
        asm volatile("" : "+v"(ln));
        const int mb = u >> 1, hh = u & 1;
        f32x4 d[3];
        if constexpr (WIDE) {
            float xk[2][8];
#pragma unroll
            for (int j = 0; j < 16; ++j) xk[j >> 3][j & 7] = xr.xa[j];
#pragma unroll
            for (int s = 0; s < 3; ++s) d[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint4 xh, xl;
                split8(xk[ks], xh, xl);
                const bf16x8 ah = __builtin_bit_cast(bf16x8, xh), al = __builtin_bit_cast(bf16x8, xl);
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int f = ((s * 2 + hh) * 2 + ks) * 2;
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, Pf[(f + 0) * 64 + ln]);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, Pf[(f + 1) * 64 + ln]);
                    d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bl, d[s], 0, 0, 0);
                    d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, d[s], 0, 0, 0);
                    d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, d[s], 0, 0, 0);
                    d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, d[s], 0, 0, 0);
                }
            }
        } else {
            uint4 xh, xl;
            split8(xr.xa, xh, xl);
            const bf16x8 ah = __builtin_bit_cast(bf16x8, xh), al = __builtin_bit_cast(bf16x8, xl);
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const bf16x8 bh = __builtin_bit_cast(bf16x8, Pf[((s * 2 + hh) * 2 + 0) * 64 + ln]);
                const bf16x8 bl = __builtin_bit_cast(bf16x8, Pf[((s * 2 + hh) * 2 + 1) * 64 + ln]);
                d[s] = f32x4{0.f, 0.f, 0.f, 0.f};
                d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bl, d[s], 0, 0, 0);
                d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, d[s], 0, 0, 0);
                d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, d[s], 0, 0, 0);
                d[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, d[s], 0, 0, 0);
            }
        }
        const int Vh = ti.Vh;                                 // joints of this tile's pixel space (= V unless WIDE)
        const int w = 16 * hh + (ln & 15);
        const int p = (4 * mb + (ln >> 4)) * Vh + w;         // pixel row of the tile
        const int gi = g.origin + p;
        const bool valid = p < g.span && gi >= 0 && gi < T * Vh; // else: the temporal conv's zero padding
        const float one = valid ? 1.f : 0.f;
        const float fa[8] = {d[0][0] * one, d[0][1] * one, d[0][2] * one, d[1][0] * one,
                             d[1][1] * one, d[1][2] * one, d[2][0] * one, d[2][1] * one};
        const float fb[8] = {d[2][2] * one, xr.xp[0] * one, xr.xp[1] * one, xr.xp[2] * one, one, 0.f, 0.f, 0.f};
        uint4 ha, la, hb, lb;
        split8(fa, ha, la);
        split8(fb, hb, lb);
        if (w < Vh && p < ROWS) {
            Fs[p] = ha;
            Fs[(size_t)ROWS + p] = hb;
            Fs[(size_t)2 * ROWS + p] = la;
            Fs[(size_t)3 * ROWS + p] = lb;
        }
    };
    // units wave, wave+4, wave+8 arrive prefetched; any further ones (narrow frames only) are loaded here
    auto feature_phase = [&](int tile, const XRegs &x0, const XRegs &x1, const XRegs &x2) {
        TileInfo6 ti;
        if constexpr (WIDE) ti = tile_info(tile);
        else {
            ti.n = tile / tiles_per_clip;
            ti.Vh = V;
            ti.j0 = ti.half = 0;
            ti.g = tile_geom_b(tile - ti.n * tiles_per_clip, V, KT6, 1, T, NP6);
        }
        const TileGeomB &g = ti.g;
        const int need = min(ROWS, ((g.span + 15) >> 4) << 4);       // rows the producer will read
        const int nun = (((need + ti.Vh - 1) / ti.Vh + 3) >> 2) * 2; // M-blocks x 2 joint halves
        const bool two = ti.Vh > 16;
        for (int u = wave; u < nun; u += 4) {
            if (!two && (u & 1)) continue;
            if (u == wave) feature_unit(ti, u, x0);
            else if (u == wave + 4) feature_unit(ti, u, x1);
            else if (u == wave + 8) feature_unit(ti, u, x2);
            else {
                XRegs xr;
                load_x(xr, tile, u);
                feature_unit(ti, u, xr);
            }
        }
    };

    // ---- producer: one 16-pixel block of chunk `ch` -> hi/lo images of `buf` (see stem_bf16_v4.hip) -----------------
    const int pl = lane & 15, pg = lane >> 4;
    struct Prod { uint4 wh, wl, fb; f32x4 d; int p; };
    auto prod_load = [&](Prod &pr, int ch, int bi) {
        pr.p = bi * 16 + pl;
        pr.wh = W12q[(size_t)(pg & 1) * C + ch * CCB + pl];
        pr.wl = W12q[(size_t)(2 + (pg & 1)) * C + ch * CCB + pl];
        pr.fb = Fs[(size_t)pg * ROWS + pr.p];
    };
    auto prod_mfma = [&](Prod &pr) {
        const bf16x8 f = __builtin_bit_cast(bf16x8, pr.fb);
        pr.d = f32x4{0.f, 0.f, 0.f, 0.f};
        pr.d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pr.wh), f, pr.d, 0, 0, 0);
        pr.d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pr.wl), f, pr.d, 0, 0, 0);
    };
    // The same inside the slot-structured loop, with a VGPR destination: the result feeds VALU work, and through the
    // builtin hipcc computed it in AGPRs and copied it out (4 v_accvgpr_read + an s_nop 6 per block).  As inline asm the
    // hazard recogniser does not see the matrix-core write: the consumer sits four slots (>= 4 main MFMAs, 64+ cycles)
    // further down, far beyond the 7 wait states a 4-pass MFMA result needs; the second MFMA accumulates onto the first
    // with identical vDst / SrcC (back-to-back forwarding).
    auto prod_mfma_slots = [&](Prod &pr) {
        using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
        const u32x4 wh = __builtin_bit_cast(u32x4, pr.wh), wl = __builtin_bit_cast(u32x4, pr.wl), fb = __builtin_bit_cast(u32x4, pr.fb);
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(pr.d) : "v"(wh), "v"(fb));
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(pr.d) : "v"(wl), "v"(fb));
    };
    auto prod_finish = [&](char *buf, const Prod &pr) {
        const float v0 = relu1(pr.d[0]), v1 = relu1(pr.d[1]), v2 = relu1(pr.d[2]), v3 = relu1(pr.d[3]);
        const unsigned h0 = pack_bf16x2(v0, v1), h1 = pack_bf16x2(v2, v3);
        const int off = lds_off(pr.p, pg >> 1) + (pg & 1) * 8;
        *reinterpret_cast<uint2 *>(buf + off) = make_uint2(h0, h1);
        if constexpr (TERMS == 3) {
            const unsigned l0 = pack_bf16x2(v0 - bf16_lo_to_f32(h0), v1 - bf16_hi_to_f32(h0));
            const unsigned l1 = pack_bf16x2(v2 - bf16_lo_to_f32(h1), v3 - bf16_hi_to_f32(h1));
            *reinterpret_cast<uint2 *>(buf + img_bytes + off) = make_uint2(l0, l1);
        }
    };

    // ---- one-time setup ----------------------------------------------------------------------
    for (int e = tid; e < C * 2; e += NT6) {   // W12 -> bf16 hi/lo planes [hi k0-7][hi k8-15][lo k0-7][lo k8-15] of [C] x 16 B
        const int c = e >> 1, kh = e & 1;
        float w8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w8[i] = W12[c * W12P + kh * 8 + i];
        uint4 hi, lo;
        split8(w8, hi, lo);
        W12q[(size_t)kh * C + c] = hi;
        W12q[(size_t)(2 + kh) * C + c] = lo;
    }
    // Folded-BN shift of this workgroup's 128 output channels (narrow form), read ONCE: lane l keeps channels l and 64 + l in
    // two registers, and the epilogue fetches a lane's four channel rows of a 16-channel block from them through the LDS
    // crossbar (ds_bpermute: counts in lgkmcnt, touches no memory).  A per-block global load of the shift shares vmcnt with
    // the result stores: it made every block wait for the previous block's stores to complete (eight store round trips in
    // series per tile).  Eight float4 per lane instead would not fit every instantiation (the wide bf16 form holds 252
    // AGPRs, K3v6 with statistics 256), and 512 B of LDS would take the kernel from C = 256 shapes that fill the budget.
    // Three-term narrow form only: its main loop comes out instruction for instruction as without them.  The one-term form
    // and the WIDE form keep their per-block load (see their epilogues and DESIGN section 3).
    float sh_lo = 0.f, sh_hi = 0.f;
    if constexpr (!WIDE && TERMS == 3) {
        sh_lo = shift[cg * 128 + lane];
        sh_hi = shift[cg * 128 + 64 + lane];
    }
    // the workgroup's tiles: tile, tile_next(tile), ... below tile_end.  Grid-stride over all tiles, or (narrow three-term form
    // of a shape with short last tiles) the contiguous run of v6_run in the order of v6_order
    int tile = blockIdx.x;
    int tile_end = ntiles;
    unsigned run_step = 0;                    // 1 on a contiguous run, else 0: the stride is gridDim.x, read where it is used (the
                                              // other forms then keep their prologue and scalar registers as they were)
    // ... walked in the order of v6_order: run_first / ord_ts are what v6_order_next needs (ord_ts = -1: in order)
    [[maybe_unused]] int run_first = 0, ord_ts = -1;
    if constexpr (TERMS == 3 && !WIDE) {
        if (abl & OPT_V6_SHORT) {
            const V6Run run = v6_run(blockIdx.x, gridDim.x, ntiles / tiles_per_clip, tiles_per_clip, 1);
            tile = run.first;
            tile_end = run.end;
            run_step = 1u;
#ifndef V6_ONE_STORE_PHASE   // (A/B variant: every workgroup walks its run in order, as before the two store phases)
            const V6Order ord = v6_order(blockIdx.x, run, tiles_per_clip, 1);
            run_first = run.first;
            ord_ts = ord.ts;
            tile = v6_order_start(run, ord);
#endif
        }
    }
    auto tile_step = [&]() -> unsigned {
        if constexpr (TERMS == 3 && !WIDE) return run_step ? run_step : gridDim.x;
        else return gridDim.x;
    };
    // the tile behind tile t of the walk (a few scalar instructions per tile, outside the main loop's slots)
    auto tile_next = [&](int t) -> int {
#ifndef V6_ONE_STORE_PHASE
        if constexpr (TERMS == 3 && !WIDE)
            if (run_step) return v6_order_next(t, run_first, ord_ts);
#endif
        return t + tile_step();
    };
    {
        XRegs x0 = {}, x1 = {}, x2 = {};
        if (tile < tile_end) {
            dma_pfrag(tile);
            load_x(x0, tile, wave);
            load_x(x1, tile, wave + 4);
            load_x(x2, tile, wave + 8);
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) { dma_frag(0, 0, d); dma_frag(1, 1, d); }
        vm_wait_keep<0>();
        __syncthreads();                      // W12q, Pf(tile), weight pairs 0 and 1 landed
        if (tile < tile_end) feature_phase(tile, x0, x1, x2);
        __syncthreads();
    }

    // ring bookkeeping without divisions: slot of the current pair gq (the comments' running pair index), and (slot,
    // source index) of pair gq + 2
    int slot0 = 0, slot2 = 2, q2 = 2 % npairs;
    const int sel = lane >> 5, chh = (lane >> 4) & 1;   // B fragment lane groups: step of the pair, channel half
    // One tile, generic in the 16-pixel blocks a wave owns: 4 (the 256-pixel tile) or 2 (SHORT: the narrow three-term form on a
    // clip's last tile of at most 128 pixels — a wave owns all 128 channels of 32 pixels, 16 * TERMS MFMAs per pair with two
    // fillers per slot, five producer blocks per wave and chunk counted from the tile's first block, bounds-checked stores).
    // LDS carve, images, weight ring and its DMA schedule, MFMA and term order are the same; so is every stored value.
    // The body is kf6_tile.h, included once per form (it says why it is text and not a generic lambda).
    for (; tile < tile_end; tile = tile_next(tile)) {
        if constexpr (TERMS == 3 && !WIDE) {
            // (scalar) the clip's last tile of a shape with short last tiles: one uniform branch per tile
            if ((abl & OPT_V6_SHORT) && (tile + 1) % tiles_per_clip == 0) {
#define V6_TILE_NB 2
#include "kf6_tile.h"
#undef V6_TILE_NB
            } else {
#define V6_TILE_NB 4
#include "kf6_tile.h"
#undef V6_TILE_NB
            }
        } else {
#define V6_TILE_NB 4
#include "kf6_tile.h"
#undef V6_TILE_NB
        }
    }
#ifdef STGCN_ABLATION
    if (dbg && lane == 0 && blockIdx.x < 16 && blockIdx.y == 0)   // (16 workgroups x 8 rows x 8 slots: the tools size the buffer)
        for (int i = 0; i < 8; ++i) {         // rows 0-3 of a workgroup's eight: the waves' full tiles, rows 4-7: their short tiles
            dbg[(blockIdx.x * 8 + wave) * 8 + i] = tsum[i];
            dbg[(blockIdx.x * 8 + 4 + wave) * 8 + i] = tsum[8 + i];
        }
#endif
}

// ---- host: plans and launch ---------------------------------------------------------------------------------------------
struct V6Plan {
    int rows = 0, tiles_per_clip = 0;
    size_t lds = 0;
    int v0 = 0, tpc1 = 0;                     // wide form: joints of the first half, tiles of a clip's second half
    int npbw = 8;                             // producer blocks per wave and chunk (narrow three-term KF6: 7 where v6_blocks_read allows)
    // narrow three-term KF6: the clip's last tile takes the short form and the tiles are walked in balanced runs (v6_run)
    bool short_last = false;
    int short_blocks = 0;                     // 16-row blocks the taps of that tile read (v6_short_blocks), at most 20
};

// rows of the image one (pixel space of Vh joints) tile needs; 0 when the producer cannot cover it
inline int v6_rows(int T, int Vh, int K) {
    int dt = ceil_div(NP6 - 1, Vh);
    if (dt > T - 1) dt = T - 1;
    const int span = (dt + K) * Vh;
    if (ceil_div(ceil_div(span, 16), 4) > 8) return 0;       // producer: at most 3 + 3 + 2 blocks per wave and chunk
    return (span + 15) / 16 * 16;
}

// The most 16-row blocks of its image from which the taps of one tile of a (T, V) clip read: the image starts at frame
// t_first - 4 (tile_geom_b), the tile's first pixel sits s = q0 - t_first * V rows into it, and the pixels that are stored read
// the rows s .. s + (q_last - q0) + (K - 1) V — blocks s >> 4 (the kernel's pb0) up to that row's.  Blocks in front of pb0, and
// what the frame-aligned span holds behind the last row read, feed no result.  Full tiles repeat with s = 256 i mod V, a period
// of at most V tiles; the clip's last tile is walked as it is.  At most 28: seven producer blocks per wave and chunk, counted
// from pb0, cover every tile.
inline int v6_blocks_read(int T, int V, int K) {
    const int TV = T * V, tpc = ceil_div(TV, NP6);
    int most = 0;
    for (int i = 0; i < tpc; ++i) {
        if (i >= V && i < tpc - 1) i = tpc - 1;              // (the full tiles' geometry has come round)
        const int q0 = i * NP6, q_last = (q0 + NP6 < TV ? q0 + NP6 : TV) - 1, s = q0 % V;
        const int n = ((s + q_last - q0 + (K - 1) * V) >> 4) - (s >> 4) + 1;
        if (n > most) most = n;
    }
    return most;
}

// The same count for the SHORT form of a clip's last tile: 0 unless that tile holds 1 .. 128 pixels, else the blocks from the one
// of its first pixel (row s = q0 mod V of the image) to the one of the last row a tap reads, s + (pixels - 1) + (K - 1) V.  The short
// form produces five blocks per wave and chunk from there on: the plan admits it up to 20 (V = 22, T = 180: exactly 20).
inline int v6_short_blocks(int T, int V, int K) {
    const int TV = T * V, tpc = ceil_div(TV, NP6), q0 = (tpc - 1) * NP6, npx = TV - q0;
    if (npx < 1 || npx > NP6 / 2) return 0;
    const int s = q0 % V;
    return ((s + npx - 1 + (K - 1) * V) >> 4) - (s >> 4) + 1;
}

// narrow frames (V <= 32); terms = 3: two images per chunk buffer (KF6 bf16 hi + lo; KF7 fp16 + two e4m3 = 64 B per row)
inline bool plan_v6_narrow(int C, int T, int V, int K, int terms, V6Plan &pl) {
    if (K != KT6 || C % 128 != 0 || V > 32) return false;    // (C % 32 == 0: an even number of 16-channel chunks)
    const int rows = v6_rows(T, V, K);
    if (rows == 0) return false;
    const size_t buf = (size_t)rows * PXB * (terms == 3 ? 2 : 1);
    const size_t img = 2 * buf > (size_t)4 * EPI6 ? 2 * buf : (size_t)4 * EPI6;
    pl.lds = (size_t)C * W12P * 4 + RING6 + img + (size_t)rows * 64 + 12 * FRAG6;
    if (pl.lds > (size_t)kLdsBytes) return false;
    pl.rows = rows;
    pl.tiles_per_clip = ceil_div(T * V, NP6);
    pl.npbw = v6_blocks_read(T, V, K) <= 28 ? 7 : 8;         // (read by KF6's three-term launch only)
    pl.short_blocks = v6_short_blocks(T, V, K);              // (likewise)
    pl.short_last = pl.short_blocks >= 1 && pl.short_blocks <= 20;
    return true;
}

// wide frames: the two joint halves of stem_wide_split
inline bool plan_v6_wide(int C, int T, int V, int K, int terms, V6Plan &pl) {
    const int v0 = stem_wide_split(V);
    if (K != KT6 || C % 128 != 0 || v0 == 0) return false;
    const int r0 = v6_rows(T, v0, K), r1 = v6_rows(T, V - v0, K);
    if (r0 == 0 || r1 == 0) return false;
    const int rows = r0 > r1 ? r0 : r1;
    const size_t buf = (size_t)rows * PXB * (terms == 3 ? 2 : 1);
    const size_t img = 2 * buf > (size_t)4 * EPI6 ? 2 * buf : (size_t)4 * EPI6;
    // the half's 24 fragments: inside the second image buffer with three terms (it must hold them), else behind Fs
    if (terms == 3 && buf < (size_t)24 * FRAG6) return false;
    pl.lds = (size_t)C * W12P * 4 + RING6 + img + (size_t)rows * 64 + (terms == 3 ? 0 : 24 * FRAG6);
    if (pl.lds > (size_t)kLdsBytes) return false;
    pl.rows = rows;
    pl.v0 = v0;
    pl.tpc1 = ceil_div(T * (V - v0), NP6);
    pl.tiles_per_clip = ceil_div(T * v0, NP6) + pl.tpc1;
    return pl.tiles_per_clip - pl.tpc1 >= pl.tpc1;           // (the interleaved tile order assumes it: V0 >= V - V0)
}

template <bool WIDE>
bool stem_v6_form_supported(int C, int T, int V, int K, unsigned flags) {
    const unsigned math = flags & STGCN_MATH_MASK;
    if (math != STGCN_MATH_BF16X3 && math != STGCN_MATH_BF16) return false;
    const int terms = math == STGCN_MATH_BF16X3 ? 3 : 1;
    V6Plan pl;
    return T >= 1 && (WIDE ? plan_v6_wide(C, T, V, K, terms, pl) : plan_v6_narrow(C, T, V, K, terms, pl));
}

template <int TERMS, bool WIDE>
int launch_v6(const uint4 *pf, const float *x, int xsc, int xsp, const float *W12, const uint4 *Wq, const float *shift, void *y,
              int N, int C, int T, int V, const V6Plan &pl, bool bf16out, int opt, int num_cu, hipStream_t st) {
    const int ntiles = N * pl.tiles_per_clip;
    const dim3 grid(ntiles < num_cu ? ntiles : num_cu, C / 128, 1);
    auto kern = bf16out ? stem_bf16_v6_kernel<TERMS, true, WIDE> : stem_bf16_v6_kernel<TERMS, false, WIDE>;
    if constexpr (TERMS == 3 && !WIDE)        // (the one-term and the wide forms stay on 8 blocks: not measured on 7)
        if (pl.npbw == 7) kern = bf16out ? stem_bf16_v6_kernel<3, true, false, 7> : stem_bf16_v6_kernel<3, false, false, 7>;
    if constexpr (TERMS == 3 && !WIDE)        // (N,C,T,V): results leave the accumulators as rows of pixels (PIXROWS)
        if (!(opt & OPT_OUT_NTVC)) {
            if (pl.npbw == 7) kern = bf16out ? stem_bf16_v6_kernel<3, true, false, 7, true> : stem_bf16_v6_kernel<3, false, false, 7, true>;
            else kern = bf16out ? stem_bf16_v6_kernel<3, true, false, 8, true> : stem_bf16_v6_kernel<3, false, false, 8, true>;
        }
    if constexpr (TERMS == 3 && !WIDE)
        if (pl.short_last) opt |= OPT_V6_SHORT;
    STGCN_HIP_CHECK(allow_lds(kern, pl.lds));
    hipLaunchKernelGGL(kern, grid, dim3(NT6), pl.lds, st, pf, x, xsc, xsp, W12, Wq, shift, y, C, T, V, pl.rows,
                       pl.tiles_per_clip, ntiles, opt, debug_buffer(), pl.v0, pl.tpc1);
    STGCN_LAUNCH_CHECK("stem_bf16_v6_kernel");
    return STGCN_OK;
}

template <bool WIDE>
int launch_stem_v6_form(const float *x, bool x_ntvc, const void *pfrag, const void *prep_w12, const void *Wq, const float *shift,
                        void *out, int N, int C, int T, int V, int K, unsigned flags, hipStream_t st) {
    const unsigned math = flags & STGCN_MATH_MASK;
    const int terms = math == STGCN_MATH_BF16X3 ? 3 : 1;
    const bool bf16out = (flags & STGCN_OUT_BF16) != 0;
    const int opt = (flags & STGCN_OUT_NTVC) ? OPT_OUT_NTVC : 0;
    V6Plan pl;
    if (!(WIDE ? plan_v6_wide(C, T, V, K, terms, pl) : plan_v6_narrow(C, T, V, K, terms, pl)))
        return fail(STGCN_ERR_UNSUPPORTED, "stem v6 kernel does not cover C=%d T=%d V=%d K=%d", C, T, V, K);
    if ((size_t)3 * T * V * 4 >= ((size_t)1 << 31) || (size_t)T * V * C >= ((size_t)1 << 31))
        return fail(STGCN_ERR_UNSUPPORTED, "stem v6: clip of T=%d V=%d exceeds a buffer resource", T, V);
    int dev = 0, num_cu = 256;
    STGCN_HIP_CHECK(hipGetDevice(&dev));
    STGCN_HIP_CHECK(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const int xsc = x_ntvc ? 1 : T * V, xsp = x_ntvc ? 3 : 1;
    const uint4 *pf = (const uint4 *)pfrag;
    const float *W12 = (const float *)prep_w12;
    const uint4 *wq = (const uint4 *)Wq;
    return terms == 3 ? launch_v6<3, WIDE>(pf, x, xsc, xsp, W12, wq, shift, out, N, C, T, V, pl, bf16out, opt, num_cu, st)
                      : launch_v6<1, WIDE>(pf, x, xsc, xsp, W12, wq, shift, out, N, C, T, V, pl, bf16out, opt, num_cu, st);
}

}  // namespace
}  // namespace stgcn
