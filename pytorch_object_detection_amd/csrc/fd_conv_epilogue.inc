// fd_conv_epilogue.inc -- the fused epilogue of the conv kernels, included TEXTUALLY at the end of each kernel body (as a
// function taking the accumulator arrays by reference the compiler spills them: 508 bytes of scratch per lane on the tower kernel).
//   y = act(acc * scale + shift (+ / mask) res), transposed through a per-wave LDS stage so a lane owns 4 consecutive channels of
//   one pixel (16-byte residual loads / output stores).
// In scope: ConvArgs a; f32x16 acc[TM][TN], cor[..][..]; char* smem (free for reuse: the K loop ended in a workgroup barrier);
//   float* ybase; int m0, n0, wm, wn, wave, lane, l31, lh; constexpr TM, TN, SPLIT, GNS (GNS: also write the row-group statistics of the
//   stored output, fd_gn_rowstats -- compiled into dedicated instantiations only: inside the four-sub-tile kernels it pushes the
//   accumulators into scratch).
#ifndef FD_EPI_RES_PREFETCHED
#include "fd_conv_res_prefetch.inc"     // (kernels without a peeled last K-tile: the same prefetch, at the head of the epilogue)
#endif
    // ---- epilogue: acc reg e of lane l is C[row = (e&3) + 8*(e>>2) + 4*(l>>5)][col = l&31] ----
    // Vector path: each 32x32 sub-tile is transposed through a per-wave LDS stage so that a lane owns 4 consecutive
    // channels of one pixel: residual loads / output stores are 16 B per lane, 8 full 128-B lines per instruction
    // (4x fewer memory instructions than storing straight from the accumulator layout).
    if constexpr (SPLIT) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] += cor[i][j] * (1.0f / FD_SPLIT_SCALE);
    }
    float* stage = reinterpret_cast<float*>(smem) + wave * 1024;
    // The WHOLE wave tile on the fast path (full sub-tiles inside the output, rows at a fixed stride, no activation or ReLU / SiLU on every channel): a loop of its
    // own -- the four sub-tiles' ~100 instructions each then lie next to each other instead of ~7 000 instructions (the general and the scalar path) apart
    // (DESIGN 4.1n: instruction fetch; strided 3x3 layers -9 ... -10 %, the 1x1 layers -2 ... -4 %).
    // epi_buf (uniform; host: fd_conv_epi_extents): the output view fits 32-bit byte offsets -- the fast loop stores through a raw buffer descriptor over the view
    // (of this split-K slice).  Rows past M then lie behind the descriptor's extent and are dropped by the range check, so the ragged last M tile is on the fast
    // path too; the column condition stays (channels past Cout_epi lie inside a view's row).  GNS keeps the row condition: its statistics store wants the predicate.
    const bool epi_buf = !SPLIT && a.y_bytes != 0;
    const bool wave_fast = !SPLIT && a.vec_epi && !a.sc_on && ((!GNS && epi_buf) || m0 + (wm * TM + TM) * 32 <= a.M) && n0 + (wn * TN + TN) * 32 <= a.Cout_epi &&
                           (a.act == FD_ACT_NONE || (a.act_c0 <= n0 + wn * TN * 32 && (a.act == FD_ACT_RELU || a.act == FD_ACT_SILU)));
    if (wave_fast && epi_buf) {
        // ONE uniform decision per wave, outside the j / i / p loops: {no residual, add, mask} x {none, ReLU, SiLU}, each a straight-line copy of the store loop
        // (between two stores: the residual, the activation, one 32-bit add, the store -- no branch, no 64-bit address arithmetic).  A launch runs one copy, so the executed
        // footprint shrinks (DESIGN 4.1n) although the kernel grows.  The four ds_read_b128 of a sub-tile are issued together and waited for once.
        const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)ybase, (short)0, (int)a.y_bytes, 0x00020000);
        const int c4 = (lane & 7) * 4;
        const int mw = m0 + wm * TM * 32 + (lane >> 3), nw = n0 + wn * TN * 32 + c4;          // this lane's first row / channel of the wave tile
        const unsigned y_off = ((unsigned)mw * (unsigned)a.y_cs + (unsigned)(a.y_co + nw)) * 4u;
        const int ystep8 = a.y_cs * 32;                                                       // bytes between rows r and r + 8
        const float* sp = stage + (lane >> 3) * 32 + c4;
        auto store_wave_tile = [&](auto res_c, auto act_c) {
            constexpr int RES = (RUP && decltype(res_c)::value == 2) ? 1 : decltype(res_c)::value;   // 0 none, 1 addend, 2 ReLU mask (the upsampled map of RUP is always an addend)
            constexpr int ACT = decltype(act_c)::value;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float sc = esc[j], sf = esf[j];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        stage[((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + l31] = acc[i][j][e] * sc + sf;
                    wave_lds_sync();
                    float4 vv[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) vv[p] = *reinterpret_cast<const float4*>(sp + p * 256);
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        float4 v = vv[p];
                        if constexpr (RES != 0 && !RUP) {
                            const float4 r = rres[SPLIT ? 0 : i][SPLIT ? 0 : j][p];
                            if constexpr (RES == 2) {
                                v.x = r.x > 0.f ? v.x : 0.f; v.y = r.y > 0.f ? v.y : 0.f;
                                v.z = r.z > 0.f ? v.z : 0.f; v.w = r.w > 0.f ? v.w : 0.f;
                            } else {
                                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                            }
                        }
                        if constexpr (ACT == FD_ACT_RELU) {
                            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                        } else if constexpr (ACT == FD_ACT_SILU) {
                            v.x = fd_act(v.x, FD_ACT_SILU, 0.f); v.y = fd_act(v.y, FD_ACT_SILU, 0.f);
                            v.z = fd_act(v.z, FD_ACT_SILU, 0.f); v.w = fd_act(v.w, FD_ACT_SILU, 0.f);
                        }
                        if constexpr (RES != 0 && RUP) {          // the upsampled map joins AFTER the activation (HISFcos.py:155-165: relu(gn(tf(c))) + Up_sample(...))
                            const float4 r = rres[SPLIT ? 0 : i][SPLIT ? 0 : j][p];
                            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                        }
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(f32x4, v), yrsrc, (int)(y_off + (unsigned)((4 * i + p) * ystep8) + 128u * j), 0, 0);
                        // (row step: one add of a scalar; column block: the immediate offset.  NOT the instruction's scalar offset: the compiler's hazard table
                        // exempts a 16-byte buffer store with an SGPR offset from "VALU write of the store's data registers", and on gfx950 such a store
                        // followed two instructions later by the next sub-tile's staging multiply-add in one of its data registers stored the NEW value --
                        // seen in the copies without a residual, where nothing else stands between.  With the immediate 0 the compiler inserts the wait states.)
                        if constexpr (GNS) fd_gn_rowstats(a.gn_stats, a.gn_G, a.gn_cg, v, (size_t)(mw + 32 * i + 8 * p), nw + 32 * j, lane, true);
                    }
                    wave_lds_sync();
                }
            }
        };
        using std::integral_constant;
        switch ((a.res ? (a.res_mask ? 2 : 1) : 0) * 3 + a.act) {      // (wave_fast: a.act is NONE = 0, RELU = 1 or SILU = 2)
            case 0: store_wave_tile(integral_constant<int, 0>{}, integral_constant<int, FD_ACT_NONE>{}); break;
            case 1: store_wave_tile(integral_constant<int, 0>{}, integral_constant<int, FD_ACT_RELU>{}); break;
            case 2: store_wave_tile(integral_constant<int, 0>{}, integral_constant<int, FD_ACT_SILU>{}); break;
            case 3: store_wave_tile(integral_constant<int, 1>{}, integral_constant<int, FD_ACT_NONE>{}); break;
            case 4: store_wave_tile(integral_constant<int, 1>{}, integral_constant<int, FD_ACT_RELU>{}); break;
            case 5: store_wave_tile(integral_constant<int, 1>{}, integral_constant<int, FD_ACT_SILU>{}); break;
            case 6: store_wave_tile(integral_constant<int, 2>{}, integral_constant<int, FD_ACT_NONE>{}); break;
            case 7: store_wave_tile(integral_constant<int, 2>{}, integral_constant<int, FD_ACT_RELU>{}); break;
            default: store_wave_tile(integral_constant<int, 2>{}, integral_constant<int, FD_ACT_SILU>{}); break;
        }
    } else if (wave_fast) {
        // the same wave tile with 64-bit pointers and the variants behind uniform branches: views too large for 32-bit byte offsets, and the last-but-ragged tiles of GNS
        const int act_u = a.act;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nb = n0 + (wn * TN + j) * 32;
            const float sc = esc[j], sf = esf[j];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mb = m0 + (wm * TM + i) * 32;
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    stage[((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + l31] = acc[i][j][e] * sc + sf;
                wave_lds_sync();
                const int c4 = (lane & 7) * 4, nn = nb + c4;
                {
                    float* yp = ybase + (size_t)(mb + (lane >> 3)) * a.y_cs + a.y_co + nn;
                    const size_t ystep = (size_t)8 * a.y_cs;
                    const float* sp = stage + (lane >> 3) * 32 + c4;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        float4 v = *reinterpret_cast<const float4*>(sp + p * 256);
                        if (!RUP && a.res) {
                            const float4 r = rres[SPLIT ? 0 : i][SPLIT ? 0 : j][p];
                            if (a.res_mask) {
                                v.x = r.x > 0.f ? v.x : 0.f; v.y = r.y > 0.f ? v.y : 0.f;
                                v.z = r.z > 0.f ? v.z : 0.f; v.w = r.w > 0.f ? v.w : 0.f;
                            } else {
                                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                            }
                        }
                        if (act_u == FD_ACT_RELU) {
                            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                        } else if (act_u == FD_ACT_SILU) {
                            v.x = fd_act(v.x, FD_ACT_SILU, 0.f); v.y = fd_act(v.y, FD_ACT_SILU, 0.f);
                            v.z = fd_act(v.z, FD_ACT_SILU, 0.f); v.w = fd_act(v.w, FD_ACT_SILU, 0.f);
                        }
                        if (RUP && a.res) {          // the upsampled map joins AFTER the activation (HISFcos.py:155-165: relu(gn(tf(c))) + Up_sample(...))
                            const float4 r = rres[SPLIT ? 0 : i][SPLIT ? 0 : j][p];
                            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                        }
                        if (H1 && a.y16) fd_st_h4(reinterpret_cast<_Float16*>(a.y) + ((size_t)(mb + (lane >> 3) + 8 * p) * a.y_cs + a.y_co + nn), v);   // (uniform) f16 output map
                        else
                        *reinterpret_cast<float4*>(yp + p * ystep) = v;
                        if constexpr (GNS) fd_gn_rowstats(a.gn_stats, a.gn_G, a.gn_cg, v, (size_t)(mb + (lane >> 3) + 8 * p), nn, lane, true);
                    }
                }
                wave_lds_sync();
            }
        }
    } else
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nb = n0 + (wn * TN + j) * 32;
        const int n = nb + l31;
        const bool n_ok = n < a.Cout_epi;
        const float sc = esc[j], sf = esf[j];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = m0 + (wm * TM + i) * 32;
            if (a.vec_epi) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    stage[((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + l31] = acc[i][j][e] * sc + sf;
                wave_lds_sync();     // the stage is private to this wave: no workgroup barrier needed
                // The loop below is instruction-issue bound, not memory bound (a per-workgroup timeline showed 10 us between the end of
                // the K loop and the last store being ISSUED, with or without a residual, while a store-only kernel writes the same
                // pattern at 6.7 TB/s): everything uniform is decided once per sub-tile -- one switch on the activation per float4
                // instead of one per component, the common "ReLU / SiLU on every channel" cases branch-free.
                const int c4 = (lane & 7) * 4, nn = nb + c4;
                const bool col_ok = nn < a.Cout_epi;
                const bool act_all = a.act_c0 <= nb;            // (uniform) every channel of this sub-tile takes the activation
                const int act_u = a.act;
                // fast path (uniform test): a full 32 x 32 sub-tile inside the output, rows at a fixed stride (no scatter), activation
                // none / ReLU / SiLU on every channel, residual already in registers: ~15 instructions per 16-byte store
                const bool simple_act = act_u == FD_ACT_NONE || (act_all && (act_u == FD_ACT_RELU || act_u == FD_ACT_SILU));
                if (!SPLIT && !a.sc_on && mb + 32 <= a.M && nb + 32 <= a.Cout_epi && simple_act) {
                    float* yp = ybase + (size_t)(mb + (lane >> 3)) * a.y_cs + a.y_co + nn;
                    const size_t ystep = (size_t)8 * a.y_cs;
                    const float* sp = stage + (lane >> 3) * 32 + c4;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        float4 v = *reinterpret_cast<const float4*>(sp + p * 256);
                        if (!RUP && a.res) {
                            const float4 r = rres[SPLIT ? 0 : i][SPLIT ? 0 : j][p];
                            if (a.res_mask) {
                                v.x = r.x > 0.f ? v.x : 0.f; v.y = r.y > 0.f ? v.y : 0.f;
                                v.z = r.z > 0.f ? v.z : 0.f; v.w = r.w > 0.f ? v.w : 0.f;
                            } else {
                                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                            }
                        }
                        if (act_u == FD_ACT_RELU) {
                            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                        } else if (act_u == FD_ACT_SILU) {
                            v.x = fd_act(v.x, FD_ACT_SILU, 0.f); v.y = fd_act(v.y, FD_ACT_SILU, 0.f);
                            v.z = fd_act(v.z, FD_ACT_SILU, 0.f); v.w = fd_act(v.w, FD_ACT_SILU, 0.f);
                        }
                        if (RUP && a.res) {          // the upsampled map joins AFTER the activation (HISFcos.py:155-165: relu(gn(tf(c))) + Up_sample(...))
                            const float4 r = rres[SPLIT ? 0 : i][SPLIT ? 0 : j][p];
                            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                        }
                        if (H1 && a.y16) fd_st_h4(reinterpret_cast<_Float16*>(a.y) + ((size_t)(mb + (lane >> 3) + 8 * p) * a.y_cs + a.y_co + nn), v);   // (uniform) f16 output map
                        else
                        *reinterpret_cast<float4*>(yp + p * ystep) = v;
                        if constexpr (GNS) fd_gn_rowstats(a.gn_stats, a.gn_G, a.gn_cg, v, (size_t)(mb + (lane >> 3) + 8 * p), nn, lane, true);
                    }
                } else
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int row = (lane >> 3) + 8 * p;
                    const int m = mb + row;
                    float4 v = *reinterpret_cast<const float4*>(stage + row * 32 + c4);
                    const bool st_ok = m < a.M && col_ok;
                    if (st_ok) {
                        const size_t mo = (size_t)out_row(a, m);
                        float4 rup = make_float4(0.f, 0.f, 0.f, 0.f);
                        if constexpr (RUP && !SPLIT) { if (a.res) rup = rres[i][j][p]; }
                        if (!RUP && a.res) {
                            float4 r;
                            if constexpr (SPLIT) {
                                if (H1 && a.res16) r = fd_ld_h4(reinterpret_cast<const _Float16*>(a.res) + mo * a.res_cs + a.res_co + nn);
                                else r = *reinterpret_cast<const float4*>(a.res + mo * a.res_cs + a.res_co + nn);
                            } else r = rres[i][j][p];
                            if (a.res_mask) {
                                v.x = r.x > 0.f ? v.x : 0.f; v.y = r.y > 0.f ? v.y : 0.f;
                                v.z = r.z > 0.f ? v.z : 0.f; v.w = r.w > 0.f ? v.w : 0.f;
                            } else {
                                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                            }
                        }
                        if (act_u == FD_ACT_RELU && act_all) {
                            v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f;
                            v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
                        } else if (act_u == FD_ACT_SILU && act_all) {
                            v.x = fd_act(v.x, FD_ACT_SILU, 0.f); v.y = fd_act(v.y, FD_ACT_SILU, 0.f);
                            v.z = fd_act(v.z, FD_ACT_SILU, 0.f); v.w = fd_act(v.w, FD_ACT_SILU, 0.f);
                        } else if (act_u != FD_ACT_NONE) {
                            // the level's ScaleExp parameter by a select chain over UNIFORM kernel-argument reads (a per-lane index
                            // into the argument block is a vector-memory load, and its s_waitcnt vmcnt(0) also waits for every
                            // earlier store of the wave: one in-order counter on gfx9)
                            float prm = a.seg_param[0];
                            if (act_u == FD_ACT_EXP) {
#pragma unroll
                                for (int t = 1; t < FD_MAX_SEG; ++t)
                                    prm = (t < a.nseg && m >= a.m_out[t]) ? a.seg_param[t] : prm;
                            }
                            if (nn + 0 >= a.act_c0) v.x = fd_act(v.x, act_u, prm);
                            if (nn + 1 >= a.act_c0) v.y = fd_act(v.y, act_u, prm);
                            if (nn + 2 >= a.act_c0) v.z = fd_act(v.z, act_u, prm);
                            if (nn + 3 >= a.act_c0) v.w = fd_act(v.w, act_u, prm);
                        }
                        if constexpr (RUP) { v.x += rup.x; v.y += rup.y; v.z += rup.z; v.w += rup.w; }
                        if (H1 && a.y16) fd_st_h4(reinterpret_cast<_Float16*>(a.y) + mo * a.y_cs + a.y_co + nn, v);
                        else
                        *reinterpret_cast<float4*>(ybase + mo * a.y_cs + a.y_co + nn) = v;
                    }
                    if constexpr (GNS) fd_gn_rowstats(a.gn_stats, a.gn_G, a.gn_cg, v, (size_t)m, nn, lane, st_ok);     // (host: no scatter with gn_stats)
                }
                wave_lds_sync();
            } else {
                const int act = (n >= a.act_c0) ? a.act : FD_ACT_NONE;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = mb + 4 * lh + (e & 3) + 8 * (e >> 2);
                    if (n_ok && m < a.M) {
                        const size_t mo = (size_t)out_row(a, m);
                        float v = acc[i][j][e] * sc + sf;
                        if (a.res) {
                            const float r = a.res[mo * a.res_cs + a.res_co + n];
                            v = a.res_mask ? (r > 0.f ? v : 0.f) : v + r;
                        }
                        float prm = a.seg_param[0];
                        if (act == FD_ACT_EXP) {
#pragma unroll
                            for (int t = 1; t < FD_MAX_SEG; ++t)
                                prm = (t < a.nseg && m >= a.m_out[t]) ? a.seg_param[t] : prm;
                        }
                        ybase[mo * a.y_cs + a.y_co + n] = fd_act(v, act, prm);
                    }
                }
            }
        }
    }
