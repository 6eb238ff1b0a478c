// fd_conv_res_prefetch.inc -- residual tile prefetch of the vector epilogue (see fd_conv_epilogue.inc), included textually BEFORE the
// last K-tile's MFMAs by kernels that define FD_EPI_RES_PREFETCHED: the 16-byte residual loads fly under the matrix work instead
// of being waited for at the head of the epilogue.  (Kernels that do not define it get the same text at the head of the epilogue.)
    float4 rres[SPLIT ? 1 : TM][SPLIT ? 1 : TN][4];
    if (!SPLIT && a.res && a.vec_epi) {
        if (!RUP && a.res_bytes != 0) {
            // (uniform) rows at a fixed stride, the view within 32-bit byte offsets (host: fd_conv_epi_extents): one raw buffer descriptor over the VIEW, one per-lane
            // offset per 32-channel column of the wave tile, the sub-tile / row step in the instruction's scalar offset.  Rows past M lie behind the descriptor's
            // extent and read as zero by the range check; channels past Cout_epi lie INSIDE a channel view's row, so those lanes take the out-of-range offset
            // (a select per column, not an exec mask per load).  No 64-bit address arithmetic, no predicate, no branch between the loads.
            constexpr unsigned R_OOB = 0xC0000000u;
            const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, (short)0, (int)a.res_bytes, 0x00020000);
            const int rstep8 = a.res_cs * 32;      // bytes between rows r and r + 8
            const unsigned r_row =(unsigned)(m0 + wm * TM * 32 + (lane >> 3)) * (unsigned)a.res_cs + (unsigned)a.res_co;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int nn = n0 + (wn * TN + j) * 32 + (lane & 7) * 4;
                const unsigned r_off = nn < a.Cout_epi ? (r_row + (unsigned)nn) * 4u : R_OOB;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        rres[SPLIT ? 0 : i][SPLIT ? 0 : j][p] =
                            __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, (int)r_off, (4 * i + p) * rstep8, 0));
            }
        } else {
            // scatter launches (out_row decodes the row: two integer divisions), the half-resolution addend of the RUP kernels (rows not at a fixed stride), f16
            // residual maps and views too large for 32-bit byte offsets: 64-bit pointers and a predicate per load
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int m = m0 + (wm * TM + i) * 32 + (lane >> 3) + 8 * p;
                    const int nn = n0 + (wn * TN + j) * 32 + (lane & 7) * 4;
                    const size_t ro_ = (size_t)(RUP ? res_row_up(a, m) : out_row(a, m)) * a.res_cs + a.res_co + nn;
                    if (H1 && a.res16)       // (uniform) the residual / mask source is an f16 map
                        rres[i][j][p] = (m < a.M && nn < a.Cout_epi) ? fd_ld_h4(reinterpret_cast<const _Float16*>(a.res) + ro_) : make_float4(0.f, 0.f, 0.f, 0.f);
                    else
                    rres[i][j][p] = (m < a.M && nn < a.Cout_epi) ? *reinterpret_cast<const float4*>(a.res + ro_) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
        }
    }
    // per-channel scale / shift of this lane's output columns, requested with the residual (their L2 latency used to sit at the head of every
    // sub-tile column of the epilogue)
    float esc[TN], esf[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
        const bool n_ok = n < a.Cout_epi;
        esc[j] = (a.scale && n_ok) ? a.scale[n] : 1.0f;
        esf[j] = (a.shift && n_ok) ? a.shift[n] : 0.0f;
    }
