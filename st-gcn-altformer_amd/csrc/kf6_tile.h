// One tile of KF6's tile loop (kf6.h), as text (a header only in name, so that what hashes and tracks the sources by their
// suffix sees it): included inside the loop's body, inside braces of its own, with V6_TILE_NB
// = the 16-pixel blocks a wave owns.  The kernel includes it for 4 and, in the narrow three-term form, for 2, so that each form is
// plain code of the loop body: wrapped in a generic lambda instead, the same text moved hipcc's allocation in the kernels that
// only ever run the full form (KF6-wide: 2,004 -> 2,020 instructions and 100 -> 112 v_accvgpr_* per period).
        constexpr int NB = V6_TILE_NB;
        constexpr bool SHORT = NB != 4;
        constexpr int NPW = SHORT ? 5 : NPBW;     // producer blocks per wave and chunk
        [[maybe_unused]] constexpr int SB = SHORT ? 8 : 0;        // (diagnostic builds: the short form's cycle stamps have slots of their own)
        // SHORT: the lane, opaque per tile — the lane-only address terms of its epilogue are then computed where they are used;
        // hoisted out of the tile loop beside the full form's they do not fit the register file (13 spilled registers)
        // (PIXROWS: likewise in both forms, so that its epilogue's per-lane term stays out of the main loop's registers)
        int lane_t = lane;
        if constexpr (SHORT || PIXROWS) asm volatile("" : "+v"(lane_t));
        TileInfo6 ti;
        if constexpr (WIDE) ti = tile_info(tile);
        else {
            ti.n = tile / tiles_per_clip;
            ti.Vh = V;
            ti.j0 = ti.half = 0;
            ti.g = tile_geom_b(tile - ti.n * tiles_per_clip, V, KT6, 1, T, NP6);
        }
        const int n = ti.n;
        const TileGeomB g = ti.g;
        const int Vh = ti.Vh;
        const int nblk = (g.span + 15) >> 4;
        const int next_tile = tile_next(tile);    // (the walk's order: the prefetches below and the loop's end test follow it)
        // NPBW == 7: the wave's first producer block.  The image starts at the tile's first FRAME, the tile's first pixel sits
        // s = q0 - t_first * Vh rows into it (0 <= s < Vh) and no tap reads a row in front of it: blocks below s >> 4 are not
        // produced (their rows keep the previous tile's data), nor are blocks behind pb0 + 27, which the host plan has shown to
        // lie behind the last row read.  The wave's k-th block is pbw + 4k, clamped to the image's last one.
        // SHORT: counted from the tile's first block as well, whatever NPBW: the host plan admits the short form only where the
        // taps of a short tile read at most 20 blocks from there on (v6_short_blocks).
        const int pbw = (NPBW == 8 && !SHORT) ? wave : ((g.q0 - g.t_first * Vh) >> 4) + wave;

        V6_STAMP(t_0)
        // chunk 0 of this tile
        if constexpr (NPBW == 8 && !SHORT) {
            for (int b = wave; b < nblk; b += 4) {
                Prod pr;
                prod_load(pr, 0, b);
                prod_mfma(pr);
                prod_finish(buf0, pr);
            }
        } else {
#ifdef V6_CHUNK0_SERIAL   // (A/B variant: one block after the other, as the 8-block form)
            for (int b = pbw; b < nblk; b += 4) {
                Prod pr;
                prod_load(pr, 0, b);
                prod_mfma(pr);
                prod_finish(buf0, pr);
            }
#else
            // the wave's blocks as loads, then MFMAs, then finishes: one LDS round trip and one MFMA latency per tile instead of
            // one per block (a clamped slot produces the last block again: same rows, same values)
            Prod pr[NPW];
#pragma unroll
            for (int k = 0; k < NPW; ++k) prod_load(pr[k], 0, min(pbw + 4 * k, nblk - 1));
#pragma unroll
            for (int k = 0; k < NPW; ++k) prod_mfma(pr[k]);
#pragma unroll
            for (int k = 0; k < NPW; ++k) prod_finish(buf0, pr[k]);
#endif
        }
        // LDS offsets of this lane's activation rows per tap, for the wave's FIRST 16-pixel block: block nb sits exactly
        // nb * 16 * PXB bytes further (16 more pixels leave the swizzle bit (row >> 3) & 1 alone), which rides in the
        // ds_read immediate — 9 offset registers instead of 36 (the kernel is at 256 VGPRs + copies through AGPRs).
        // Pixels past the clip's last one (last tile only) read rows of the image that exist but hold stale data: their
        // results are never stored.
        unsigned boff[KT6];
        {
            const int q = g.q0 + wave * (16 * NB) + (lane & 15);
            const int prow = q - g.t_first * Vh;
#pragma unroll
            for (int tap = 0; tap < KT6; ++tap) boff[tap] = (unsigned)lds_off(prow + tap * Vh, chh);
        }
        f32x4 acc[8][NB];
#pragma unroll
        for (int mb = 0; mb < 8; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();                      // chunk 0 visible
        V6_STAMP(t_1)
        V6_ACC(SB + 0, t_0, t_1)

        auto rd = [&](const char *p) { return *reinterpret_cast<const uint4 *>(p); };
        // activation fragments of the pair with local steps l0 = 2*pi, l1 = l0 + 1 (0 .. 17 within a period: chunk l/9 in
        // buffer l/9, tap l%9); lanes 0-31 carry step l0, lanes 32-63 step l1
        auto load_b = [&](FragB6 &b, auto l0_c, auto nb_c, auto lo_c) {
            constexpr int l0 = decltype(l0_c)::value, l1 = l0 + 1, nb = decltype(nb_c)::value;
            constexpr bool lo_img = decltype(lo_c)::value;
            const char *b0 = (l0 >= KT6 ? buf1 : buf0), *b1 = (l1 >= KT6 ? buf1 : buf0);
            const unsigned o0 = boff[l0 % KT6], o1 = boff[l1 % KT6];
            const char *p = (sel ? b1 : b0) + (sel ? o1 : o0) + (nb * 16 * PXB) + (lo_img ? img_bytes : 0);
            if constexpr (lo_img) b.lo[nb] = rd(p); else b.hi[nb] = rd(p);
        };
        using IC0 = std::integral_constant<int, 0>;
        FragB6 b_cur = {}, b_nxt = {};
        uint4 ah0n = rd(ring + slot0 * PAIR6 + lane * 16), al0n = rd(ring + slot0 * PAIR6 + lane * 16 + FRAG6);
        static_for<0, NB>([&](auto nb_c) {      // pair 0 of the tile (chunk 0 is complete)
            load_b(b_cur, IC0{}, nb_c, std::false_type{});
            if constexpr (TERMS == 3) load_b(b_cur, IC0{}, nb_c, std::true_type{});
        });
        const int nper = nch / 2;
        for (int per = 0; per < nper; ++per) {
            if constexpr (!WIDE)
                if (per + 1 == nper && next_tile < tile_end) dma_pfrag(next_tile);   // Pf is idle after the tile's feature phase
            static_for<0, 9>([&](auto pi_c) {
                constexpr int pi = decltype(pi_c)::value;
                constexpr int l0 = 2 * pi;
                // production: pairs 0-2 -> chunk 2per+1 into buf1; pairs 5-7 -> chunk 2per+2 into buf0 (3, 3, 2 blocks per
                // wave; NPBW == 7: 3, 2, 2; SHORT: 2, 2, 1): NPW / 3 each, the first NPW % 3 pairs one more
                constexpr int win = pi <= 2 ? 0 : (pi >= 5 && pi <= 7 ? 1 : -1);
                constexpr int wpi = win == 0 ? pi : pi - 5;
                constexpr int npb = win < 0 ? 0 : NPW / 3 + (wpi < NPW % 3 ? 1 : 0);
                constexpr int pk0 = NPW / 3 * wpi + (wpi < NPW % 3 ? wpi : NPW % 3);   // the pair's first block among the wave's NPW
                char *pbuf = win == 0 ? buf1 : buf0;
                const int pch = min(2 * per + 1 + (win == 1 ? 1 : 0), nch - 1);
                const int slot1 = slot0 == 2 ? 0 : slot0 + 1;
                const char *aslot = ring + slot0 * PAIR6 + lane * 16;
                const char *anext = ring + slot1 * PAIR6 + lane * 16;
                // weight fragments: current / next 16-channel block.  Block 0 of THIS pair was read during the previous one
                // (ah0n / al0n): pairs gq and gq+1 are both resident and published at a pair's start (their DMAs are issued
                // early in a pair and waited for at its end), so no pair opens with an exposed LDS read.
                V6_STAMP(t_p0)                // (diagnostic builds: time per kind of pair, slots 4-7 of the stamp buffer)
                uint4 ah[2], al[2];
                ah[0] = ah0n;
                if constexpr (TERMS == 3) al[0] = al0n;
                Prod pr = {};
                unsigned ph0 = 0, ph1 = 0;
                float pv0 = 0.f, pv1 = 0.f, pv2 = 0.f, pv3 = 0.f;
                int poff = 0;
                constexpr int NM = 8 * NB * TERMS;            // MFMAs of the pair
                // filler v (0 .. 95; with TERMS == 1 three share a slot, in the SHORT form two)
                auto filler = [&](auto v_c) {
                    constexpr int v = decltype(v_c)::value;
                    // next block's weight fragments, one block ahead: block mb+1 at fillers 12*mb + 2, + 3
                    if constexpr (v % 12 == 2 && v / 12 < 7) ah[(v / 12 + 1) & 1] = rd(aslot + ((v / 12 + 1) * 2) * FRAG6);
                    if constexpr (TERMS == 3 && v % 12 == 3 && v / 12 < 7) al[(v / 12 + 1) & 1] = rd(aslot + ((v / 12 + 1) * 2 + 1) * FRAG6);
                    // next pair's activation fragments (its chunk was published one pair ago at the latest)
                    if constexpr (v >= 40 && v < 40 + 2 * NB) {
                        constexpr int nb = (v - 40) / 2;
                        constexpr int ln = (l0 + 2) % 18;     // (pair 8 -> pair 0 of the next period / tile: chunk in buf0)
                        using LN = std::integral_constant<int, ln>;
                        using NBc = std::integral_constant<int, nb>;
                        if constexpr (v % 2 == 0) load_b(b_nxt, LN{}, NBc{}, std::false_type{});
                        else if constexpr (TERMS == 3) load_b(b_nxt, LN{}, NBc{}, std::true_type{});
                    }
                    // producer blocks: block b of this pair occupies fillers 8 + 28*b ...
                    if constexpr (npb > 0 && v >= 8 && (v - 8) / 28 < npb) {
                        constexpr int b = (v - 8) / 28, w = (v - 8) % 28;
                        auto piece = [&]() {
                            if constexpr (w == 0) {
                                pr.p = min(pbw + 4 * (pk0 + b), nblk - 1) * 16 + pl;
                                pr.wh = W12q[(size_t)(pg & 1) * C + pch * CCB + pl];
                            }
                            if constexpr (w == 1) pr.wl = W12q[(size_t)(2 + (pg & 1)) * C + pch * CCB + pl];
                            if constexpr (w == 2) pr.fb = Fs[(size_t)pg * ROWS + pr.p];
                            if constexpr (w == 10) { if constexpr (TERMS == 3 && !SHORT) prod_mfma_slots(pr); else prod_mfma(pr); }   // (TERMS == 1 packs three fillers per slot, SHORT two: too close to the consumer for the unchecked form)
                            if constexpr (w == 14) {
                                pv0 = relu1(pr.d[0]); pv1 = relu1(pr.d[1]); pv2 = relu1(pr.d[2]); pv3 = relu1(pr.d[3]);
                            }
                            if constexpr (w == 15) { ph0 = pack_bf16x2(pv0, pv1); ph1 = pack_bf16x2(pv2, pv3); }
                            if constexpr (w == 16) poff = lds_off(pr.p, pg >> 1) + (pg & 1) * 8;
                            if constexpr (w == 17) *reinterpret_cast<uint2 *>(pbuf + poff) = make_uint2(ph0, ph1);
                            if constexpr (TERMS == 3 && w == 18) { pv0 -= bf16_lo_to_f32(ph0); pv1 -= bf16_hi_to_f32(ph0); }
                            if constexpr (TERMS == 3 && w == 19) { pv2 -= bf16_lo_to_f32(ph1); pv3 -= bf16_hi_to_f32(ph1); }
                            if constexpr (TERMS == 3 && w == 20) { ph0 = pack_bf16x2(pv0, pv1); ph1 = pack_bf16x2(pv2, pv3); }
                            if constexpr (TERMS == 3 && w == 21) *reinterpret_cast<uint2 *>(pbuf + img_bytes + poff) = make_uint2(ph0, ph1);
                        };
                        constexpr bool has_work = w <= 2 || w == 10 || (w >= 14 && w <= 17) || (TERMS == 3 && w >= 18 && w <= 21);
                        // (no branch around it: in the tile's last period the second window re-produces the last chunk
                        //  into the idle buffer — a uniform branch per piece cost more than the redundant work)
                        if constexpr (has_work) piece();
                    }
                    // weights of pair gq + 2 -> the slot pair gq - 1 occupied (its readers passed the last barrier); issued
                    // early so that they have landed by the end of the pair
                    if constexpr (v >= 4 && v < 8) dma_frag(q2, slot2, v - 4);
                    // block 0 of the next pair
                    if constexpr (v == 88) ah0n = rd(anext);
                    if constexpr (TERMS == 3 && v == 89) al0n = rd(anext + FRAG6);
                };
                static_for<0, NM>([&](auto i_c) {
                    constexpr int i = decltype(i_c)::value;
                    // (the three terms of a block back to back on one accumulator: interleaving the pixel blocks instead
                    //  measured 2 % slower)
                    constexpr int mb = i / (NB * TERMS), nb = (i / TERMS) % NB, term = i % TERMS;
                    const bf16x8 a_h = __builtin_bit_cast(bf16x8, ah[mb & 1]), b_h = __builtin_bit_cast(bf16x8, b_cur.hi[nb]);
                    if constexpr (TERMS == 3 && PIXROWS) {
                        // operands exchanged: the MFMA takes its A and B fragments in one lane layout (row or column lane & 15,
                        // k-group lane >> 4), so the same registers give the transposed block D[row = pixel][col = channel],
                        // every element the same sum of the same products over the same k (see the PIXROWS epilogue)
                        const bf16x8 a_l = __builtin_bit_cast(bf16x8, al[mb & 1]), b_l = __builtin_bit_cast(bf16x8, b_cur.lo[nb]);
                        if constexpr (term == 0) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b_l, a_h, acc[mb][nb], 0, 0, 0);
                        else if constexpr (term == 1) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b_h, a_l, acc[mb][nb], 0, 0, 0);
                        else acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b_h, a_h, acc[mb][nb], 0, 0, 0);
                    } else if constexpr (TERMS == 3) {
                        const bf16x8 a_l = __builtin_bit_cast(bf16x8, al[mb & 1]), b_l = __builtin_bit_cast(bf16x8, b_cur.lo[nb]);
                        if constexpr (term == 0) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_h, b_l, acc[mb][nb], 0, 0, 0);
                        else if constexpr (term == 1) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_l, b_h, acc[mb][nb], 0, 0, 0);
                        else acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_h, b_h, acc[mb][nb], 0, 0, 0);
                    } else {
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_h, b_h, acc[mb][nb], 0, 0, 0);
                    }
                    // (the accumulators' home is the AGPR file: without this hint hipcc kept 16 of the 32 blocks in VGPRs and
                    //  copied each through an AGPR quad around its MFMAs — 64 v_accvgpr_write per period)
                    if constexpr (term == TERMS - 1) asm volatile("" : "+a"(acc[mb][nb]));
#ifndef V6_NOFILL   // (diagnostic variant: the MFMA stream alone; results are wrong)
                    static_for<i * (96 / NM), (i + 1) * (96 / NM)>(filler);
#endif
                    __builtin_amdgcn_sched_barrier(0);
                });
                b_cur = b_nxt;
                V6_STAMP(t_s1)
                V6_ACC(SB + (pi == 4 ? 6 : (pi == 0 ? 7 : (pi == 3 ? 5 : 4))), t_p0, t_s1)
                vm_wait_keep<0>();                  // pair gq+2's weights (issued ~1,500 cycles ago) have landed
                __syncthreads();              // ... and are visible; produced image rows are visible; slot gq%3 is free
                V6_STAMP(t_s2)
                V6_ACC(SB + 2, t_s1, t_s2)
                slot0 = slot1;
                slot2 = slot2 == 2 ? 0 : slot2 + 1;
                q2 = q2 + 1 == npairs ? 0 : q2 + 1;
            });
        }
        vm_wait_keep<0>();                          // (the next tile's attention fragments)
        V6_STAMP(t_2)
        V6_ACC(SB + 1, t_1, t_2)

        // ---- epilogue: each 16-channel x 64-pixel block (SHORT: x 32 pixels, half of the slice's rows' width) through this wave's
        // 4 KiB staging slice, 16 B per lane
        // D[row = channel 4*(lane>>4) + r][col = pixel lane&15] per 16x16 block.  Store addresses = scalar base + one
        // per-lane term; the last tile of a clip keeps per-lane bounds checks.
        // WIDE: the second image buffer is idle from here on (every wave is past the last pair's barrier): the next tile's
        // attention fragments go there now, land during the stores and are waited for in front of the feature phase
        if constexpr (WIDE)
            if (next_tile < tile_end) dma_pfrag(next_tile);
        XRegs xn0, xn1, xn2;                  // next tile's x: in flight while this tile's results are stored
        load_x(xn0, min(next_tile, ntiles - 1), wave);
        load_x(xn1, min(next_tile, ntiles - 1), wave + 4);
        load_x(xn2, min(next_tile, ntiles - 1), wave + 8);
        __builtin_amdgcn_sched_barrier(0);
        [[maybe_unused]] float *stg = reinterpret_cast<float *>(buf0 + wave * EPI6);   // (PIXROWS stores without staging)
        const int qw = g.q0 + wave * (16 * NB);
        const bool full = !SHORT && g.q0 + NP6 - 1 <= g.q_last;            // (scalar) every pixel of the tile lies inside the clip
        if constexpr (WIDE) {
            // half-space pixel q = t*Vh + v'  ->  pixel t*V + j0 + v' of the clip
            auto clip_pixel = [&](int q) { const int t = q / Vh; return t * V + ti.j0 + (q - t * Vh); };
            if (abl & OPT_OUT_NTVC) {
                // (N,T,V,C): as the narrow form, with the four pixels a lane stores mapped one by one
                unsigned pt[4];
                bool pok[4];
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int q = qw + it * 16 + (lane >> 2);
                    pok[it] = q <= g.q_last;
                    pt[it] = (unsigned)(clip_pixel(min(q, g.q_last)) * C + 4 * (lane & 3));
                }
#pragma unroll
                for (int mb = 0; mb < 8; ++mb) {
                    const int ob = cg * 128 + mb * 16;
                    const float4 sh4 = *reinterpret_cast<const float4 *>(shift + ob + 4 * (lane >> 4));
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) {
                        const int px = nb * 16 + (lane & 15);
                        const float4 v = make_float4(max_nan(acc[mb][nb][0] + sh4.x, 0.f), max_nan(acc[mb][nb][1] + sh4.y, 0.f),
                                                     max_nan(acc[mb][nb][2] + sh4.z, 0.f), max_nan(acc[mb][nb][3] + sh4.w, 0.f));
                        *reinterpret_cast<float4 *>(stg + px * 16 + (((lane >> 4) ^ (px & 3)) << 2)) = v;
                    }
                    const size_t tbase = (size_t)n * TV * C + ob;            // scalar
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int idx = it * 64 + lane, px = idx >> 2, sl = idx & 3;
                        const float4 v = *reinterpret_cast<const float4 *>(stg + px * 16 + ((sl ^ (px & 3)) << 2));
                        if (pok[it]) {
                            if constexpr (BF16OUT)
                                *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(y) + tbase + pt[it]) =
                                    make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                            else
                                st_out4<false>(reinterpret_cast<float *>(y) + tbase + pt[it], v);
                        }
                    }
                }
            } else {
                // (N,C,T,V): a lane owns ONE pair of pixels of the wave's 64 (2*(lane&31), +1: V, V0 and Vh are even, so a
                // pair never straddles a frame or the halves and sits 8-byte aligned in the clip) and walks the 16 channel
                // rows of a block two at a time: eight 8-byte stores per block
                const int qp = qw + 2 * (lane & 31);
                const bool pok = qp <= g.q_last;
                const unsigned lterm = (unsigned)((lane >> 5) * TV + clip_pixel(min(qp, g.q_last)));
#pragma unroll
                for (int mb = 0; mb < 8; ++mb) {
                    const int ob = cg * 128 + mb * 16;
                    const float4 sh4 = *reinterpret_cast<const float4 *>(shift + ob + 4 * (lane >> 4));
                    const float shv[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            stg[(4 * (lane >> 4) + r) * 64 + nb * 16 + (lane & 15)] = max_nan(acc[mb][nb][r] + shv[r], 0.f);
                    const size_t tbase = ((size_t)n * C + ob) * TV;           // scalar
#pragma unroll
                    for (int it = 0; it < 8; ++it) {
                        const float2 v = *reinterpret_cast<const float2 *>(stg + (it * 2 + (lane >> 5)) * 64 + 2 * (lane & 31));
                        const size_t sbase = tbase + (size_t)(it * 2) * TV;    // scalar
                        if (pok) {
                            if constexpr (BF16OUT)
                                *reinterpret_cast<unsigned *>(reinterpret_cast<unsigned short *>(y) + sbase + lterm) = pack_bf16x2(v.x, v.y);
                            else
                                *reinterpret_cast<float2 *>(reinterpret_cast<float *>(y) + sbase + lterm) = v;
                        }
                    }
                }
            }
        } else {
            if constexpr (TERMS == 1) {
                // One term: the epilogue as it was (per-block shift load, a branch per store).  With the two-form epilogue below
                // hipcc's allocation moved in this instantiation's MAIN LOOP (1,045 -> 1,073 instructions per period, 24 more AGPR
                // copies; with the shift re-read per tile just the same), which its contract does not allow.
                if (abl & OPT_OUT_NTVC) {
                    // (N,T,V,C): staged pixel-major [64 px][16 ch]: a lane's four channels of a pixel are one 16-byte slot
                    // (slot XOR-swizzled by the pixel: conflict-free b128 accesses); a store then writes 16 pixels x 64 B
                    const unsigned lterm = (unsigned)((lane >> 2) * C + 4 * (lane & 3));
#pragma unroll
                    for (int mb = 0; mb < 8; ++mb) {
                        const int ob = cg * 128 + mb * 16;
                        const float4 sh4 = *reinterpret_cast<const float4 *>(shift + ob + 4 * (lane >> 4));
#pragma unroll
                        for (int nb = 0; nb < 4; ++nb) {
                            const int px = nb * 16 + (lane & 15);
                            const float4 v = make_float4(max_nan(acc[mb][nb][0] + sh4.x, 0.f), max_nan(acc[mb][nb][1] + sh4.y, 0.f),
                                                         max_nan(acc[mb][nb][2] + sh4.z, 0.f), max_nan(acc[mb][nb][3] + sh4.w, 0.f));
                            *reinterpret_cast<float4 *>(stg + px * 16 + (((lane >> 4) ^ (px & 3)) << 2)) = v;
                        }
                        const size_t tbase = ((size_t)n * TV + qw) * C + ob;      // scalar
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int idx = it * 64 + lane, px = idx >> 2, sl = idx & 3;
                            const float4 v = *reinterpret_cast<const float4 *>(stg + px * 16 + ((sl ^ (px & 3)) << 2));
                            if (full || qw + px <= g.q_last) {
                                if constexpr (BF16OUT) {
                                    unsigned short *yb = reinterpret_cast<unsigned short *>(y) + tbase + (size_t)(it * 16) * C;
                                    *reinterpret_cast<uint2 *>(yb + lterm) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                                } else {
                                    float *yb = reinterpret_cast<float *>(y) + tbase + (size_t)(it * 16) * C;
                                    st_out4<true>(yb + lterm, v);
                                }
                            }
                        }
                    }
                } else {
                    // element offset of (row = idx>>4, 4-pixel group c4 = 4*(idx&15)) for idx = it*64 + lane
                    const unsigned lterm = (unsigned)((lane >> 4) * TV + 4 * (lane & 15));
                    const int c4l = 4 * (lane & 15);
#pragma unroll
                    for (int mb = 0; mb < 8; ++mb) {
                        const int ob = cg * 128 + mb * 16;
                        const float4 sh4 = *reinterpret_cast<const float4 *>(shift + ob + 4 * (lane >> 4));
                        const float shv[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
#pragma unroll
                        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                stg[(4 * (lane >> 4) + r) * 64 + nb * 16 + (lane & 15)] = max_nan(acc[mb][nb][r] + shv[r], 0.f);
                        const size_t tbase = ((size_t)n * C + ob) * TV + qw;      // scalar
                        const bool al16 = ((tbase & 3) == 0) && (TV % 4 == 0);    // 16-byte (8-byte for bf16) aligned rows
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const float4 v = *reinterpret_cast<const float4 *>(stg + (it * 4 + (lane >> 4)) * 64 + c4l);
                            const size_t sbase = tbase + (size_t)(it * 4) * TV;    // scalar
                            if (full && al16) {
                                if constexpr (BF16OUT)
                                    *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(y) + sbase + lterm) =
                                        make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                                else
                                    st_out4<true>(reinterpret_cast<float *>(y) + sbase + lterm, v);
                            } else {                                     // last tile of a clip / unaligned rows: element by element
                                const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (qw + c4l + e <= g.q_last) store_out<BF16OUT>(y, sbase + lterm + e, e4[e]);
                            }
                        }
                    }
                }
            } else if constexpr (PIXROWS) {
                // PIXROWS, (N,C,T,V) only (launch_v6): D[row = pixel 4*(lane>>4) + r][col = channel lane&15] per 16x16 block — a
                // lane holds FOUR CONSECUTIVE PIXELS OF ONE CHANNEL, which is what a row of the output wants: one 16-byte store
                // straight from the accumulators, no staging slice, no ds_write / ds_read, one shift value per block (the lane's
                // channel, from lane (mb & 3) * 16 + (lane & 15) of sh_lo / sh_hi).  A store instruction writes 16 channel rows x
                // 64 B; the four pixel blocks of a wave complete a row's 256 B within four consecutive stores.  The same three
                // forms as the staged epilogue below, chosen by the same uniform branch per tile.
                const int cl = lane_t & 15, p4 = 4 * (lane_t >> 4);
                const unsigned lterm = (unsigned)(cl * TV + p4);            // the one per-lane address term
                const size_t tb0 = ((size_t)n * C + cg * 128) * TV + qw;    // scalar: the wave's pixels in channel row 0 of the group
                // 16-byte (8-byte for bf16) aligned rows, the same for all eight blocks, and a result that sits on them
                const bool al16 = ((tb0 & 3) == 0) && (TV % 4 == 0) && (reinterpret_cast<size_t>(y) & (BF16OUT ? 7 : 15)) == 0;
                auto blocks = [&](auto form_c) {
                    constexpr int FORM = decltype(form_c)::value;  // 1: every store 16 B; 0: element by element; 2: whole groups 16 B
                    float shv[8];
#pragma unroll
                    for (int mb = 0; mb < 8; ++mb)         // all eight up front: one lgkmcnt wait per tile
                        shv[mb] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * ((mb & 3) * 16 + cl),
                                                                                         __builtin_bit_cast(int, mb < 4 ? sh_lo : sh_hi)));
                    // FORM 1: a block's four stores issue as soon as its 16 values exist (left alone, hipcc computes most of
                    // the tile's 128 values first and issues the stores behind them in one clump)
                    if constexpr (FORM == 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int mb = 0; mb < 8; ++mb) {
                        const size_t tbase = tb0 + (size_t)(mb * 16) * TV;        // scalar
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) {
                            const float4 v = make_float4(max_nan(acc[mb][nb][0] + shv[mb], 0.f), max_nan(acc[mb][nb][1] + shv[mb], 0.f),
                                                         max_nan(acc[mb][nb][2] + shv[mb], 0.f), max_nan(acc[mb][nb][3] + shv[mb], 0.f));
                            const size_t sbase = tbase + nb * 16;                 // scalar
                            auto store16 = [&]() {
                                if constexpr (BF16OUT)
                                    *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(y) + sbase + lterm) =
                                        make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                                else
                                    st_out4<true>(reinterpret_cast<float *>(y) + sbase + lterm, v);
                            };
                            auto store_elements = [&]() {               // element by element, each under its bounds check
                                const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (qw + nb * 16 + p4 + e <= g.q_last) store_out<BF16OUT>(y, sbase + lterm + e, e4[e]);
                            };
                            if constexpr (FORM == 1) store16();
                            else if constexpr (FORM == 2) { if (qw + nb * 16 + p4 + 3 <= g.q_last) store16(); else store_elements(); }
                            else store_elements();                       // last tile of a clip / unaligned rows
                        }
                        if constexpr (FORM == 1) __builtin_amdgcn_sched_barrier(0);
                    }
                };
#ifdef V6_SHORT_ELEMENT_STORES
                if constexpr (SHORT) blocks(std::integral_constant<int, 0>{});
#else
                if constexpr (SHORT) { if (al16) blocks(std::integral_constant<int, 2>{}); else blocks(std::integral_constant<int, 0>{}); }
#endif
                else if (full && al16) blocks(std::integral_constant<int, 1>{}); else blocks(std::integral_constant<int, 0>{});
            } else {
                // The narrow forms below exist twice, chosen by ONE uniform branch per tile: FAST (every pixel inside the clip, rows
                // aligned) is straight-line code whose stores issue back to back — nothing between a tile's first and last store
                // waits on vmcnt, so the next tile's x loads (issued above) and the stores all stay in flight; the other keeps the
                // per-lane / per-element bounds checks for a clip's last tile and unaligned rows.
                const int bpa = 16 * (lane_t >> 4);                        // ds_bpermute byte address of source lane 4 * (lane >> 4)
                // shift of channel rows 4*(lane>>4) + r, r = 0 .. 3, of 16-channel block mb
                auto block_shift = [&](int mb, float (&shv)[4]) {
                    const int src = __builtin_bit_cast(int, mb < 4 ? sh_lo : sh_hi);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        shv[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(bpa + 4 * ((mb & 3) * 16 + r), src));
                };
                if (abl & OPT_OUT_NTVC) {
                    // (N,T,V,C): staged pixel-major [64 px][16 ch]: a lane's four channels of a pixel are one 16-byte slot
                    // (slot XOR-swizzled by the pixel: conflict-free b128 accesses); a store then writes 16 pixels x 64 B
                    const unsigned lterm = (unsigned)((lane_t >> 2) * C + 4 * (lane_t & 3));
                    auto blocks = [&](auto fast_c) {
                        constexpr bool FAST = decltype(fast_c)::value;
#pragma unroll
                        for (int mb = 0; mb < 8; ++mb) {
                            const int ob = cg * 128 + mb * 16;
                            float shv[4];
                            block_shift(mb, shv);
#pragma unroll
                            for (int nb = 0; nb < NB; ++nb) {
                                const int px = nb * 16 + (lane_t & 15);
                                const float4 v = make_float4(max_nan(acc[mb][nb][0] + shv[0], 0.f), max_nan(acc[mb][nb][1] + shv[1], 0.f),
                                                             max_nan(acc[mb][nb][2] + shv[2], 0.f), max_nan(acc[mb][nb][3] + shv[3], 0.f));
                                *reinterpret_cast<float4 *>(stg + px * 16 + (((lane_t >> 4) ^ (px & 3)) << 2)) = v;
                            }
                            const size_t tbase = ((size_t)n * TV + qw) * C + ob;      // scalar
#pragma unroll
                            for (int it = 0; it < NB; ++it) {
                                const int idx = it * 64 + lane_t, px = idx >> 2, sl = idx & 3;
                                const float4 v = *reinterpret_cast<const float4 *>(stg + px * 16 + ((sl ^ (px & 3)) << 2));
                                if (FAST || qw + px <= g.q_last) {
                                    if constexpr (BF16OUT) {
                                        unsigned short *yb = reinterpret_cast<unsigned short *>(y) + tbase + (size_t)(it * 16) * C;
                                        *reinterpret_cast<uint2 *>(yb + lterm) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                                    } else {
                                        float *yb = reinterpret_cast<float *>(y) + tbase + (size_t)(it * 16) * C;
                                        st_out4<true>(yb + lterm, v);
                                    }
                                }
                            }
                        }
                    };
                    if constexpr (SHORT) blocks(std::false_type{});
                    else if (full) blocks(std::true_type{}); else blocks(std::false_type{});
                } else {
                    // A staged row holds the wave's 16 * NB pixels: LPR lanes read it back four pixels each, a pass covers RPI rows.
                    // element offset of (row = idx / LPR, 4-pixel group c4 = 4 * (idx % LPR)) for idx = it*64 + lane
                    constexpr int LPR = 4 * NB, RPI = 64 / LPR;
                    const unsigned lterm = (unsigned)((lane_t / LPR) * TV + 4 * (lane_t % LPR));
                    const int c4l = 4 * (lane_t % LPR);
                    const size_t tb0 = ((size_t)n * C + cg * 128) * TV + qw;      // scalar: the wave's pixels in channel row 0 of the group
                    // 16-byte (8-byte for bf16) aligned rows: the same for all eight blocks (a block is 16 rows of TV further)
                    const bool al16 = ((tb0 & 3) == 0) && (TV % 4 == 0);
                    // SHORT, aligned rows: a lane whose four pixels all lie inside the clip stores them as 16 bytes under its own
                    // predicate (at T = 180, V = 22 all 30 groups of the 120 pixels are whole); a ragged last group and unaligned
                    // rows keep the element form.  -DV6_SHORT_ELEMENT_STORES builds the element form alone (A/B).
                    [[maybe_unused]] const bool whole = qw + c4l + 3 <= g.q_last;
                    auto blocks = [&](auto form_c) {
                        constexpr int FORM = decltype(form_c)::value;  // 1: every store 16 B; 0: element by element; 2: whole groups 16 B
                        constexpr bool FAST = FORM == 1;
#pragma unroll
                        for (int mb = 0; mb < 8; ++mb) {
                            float shv[4];
                            block_shift(mb, shv);
#pragma unroll
                            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    stg[(4 * (lane_t >> 4) + r) * 64 + nb * 16 + (lane_t & 15)] = max_nan(acc[mb][nb][r] + shv[r], 0.f);
                            const size_t tbase = tb0 + (size_t)(mb * 16) * TV;        // scalar
#pragma unroll
                            for (int it = 0; it < 16 / RPI; ++it) {
                                const float4 v = *reinterpret_cast<const float4 *>(stg + (it * RPI + lane_t / LPR) * 64 + c4l);
                                const size_t sbase = tbase + (size_t)(it * RPI) * TV;  // scalar
                                auto store16 = [&]() {
                                    if constexpr (BF16OUT)
                                        *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(y) + sbase + lterm) =
                                            make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                                    else
                                        st_out4<true>(reinterpret_cast<float *>(y) + sbase + lterm, v);
                                };
                                auto store_elements = [&]() {               // element by element, each under its bounds check
                                    const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                                    for (int e = 0; e < 4; ++e)
                                        if (qw + c4l + e <= g.q_last) store_out<BF16OUT>(y, sbase + lterm + e, e4[e]);
                                };
                                if constexpr (FAST) store16();
                                else if constexpr (FORM == 2) { if (whole) store16(); else store_elements(); }
                                else store_elements();                       // last tile of a clip / unaligned rows
                            }
                        }
                    };
#ifdef V6_SHORT_ELEMENT_STORES
                    if constexpr (SHORT) blocks(std::integral_constant<int, 0>{});
#else
                    if constexpr (SHORT) { if (al16) blocks(std::integral_constant<int, 2>{}); else blocks(std::integral_constant<int, 0>{}); }
#endif
                    else if (full && al16) blocks(std::integral_constant<int, 1>{}); else blocks(std::integral_constant<int, 0>{});
                }
            }
        }
        V6_STAMP(t_3)
        V6_ACC(SB + 3, t_2, t_3)
        if (next_tile < tile_end) {           // its fragments landed at the last stage barrier, its x during the stores;
            if constexpr (WIDE) {             // (WIDE: fragments issued at the head of this epilogue — landed, then visible)
                vm_wait_keep<0>();
                __syncthreads();
            }
            feature_phase(next_tile, xn0, xn1, xn2);   // Fs lies behind the staging area: no barrier needed in front
            V6_STAMP(t_4)
            __syncthreads();                  // Fs complete, every wave's staging reads done (chunk 0 overwrites buf0)
        }
        V6_STAMP(t_5)
