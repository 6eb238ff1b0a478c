// fd_stem_bwd.hip -- weight gradient of the ResNet stem (7x7 stride-2 pad-3 convolution 3 -> 64 on the [N][H][W][4] image layout): the one layer of the
// trainable detectors that had no HIP backward (the image needs no gradient, so there is no data-gradient kernel).
//
//   dW[co][ci][ky][kx] = scale[co] * sum over (n, oy, ox) of g[n][oy][ox][co] * x[n][2 oy - 3 + ky][2 ox - 3 + kx][ci],   g = dy, or dy where y > 0 (ReLU mask)
//
// As a GEMM: M = 64 output channels, N = 147 tap x channel columns, K = every output pixel.  The columns are laid out like the forward kernel's K
// (fd_stem.hip): column c = 22 ky + 3 kx + ci, 22 per filter row (c % 22 == 21 unused), 7 x 22 = 154, padded to 160 = 5 MFMA blocks of 32 (92 % of
// the MFMAs are real work); the padding columns accumulate whatever the patch holds next to the window and are never read back.
//   * fp32 MFMA 32x32x2 (exact fp32 products): one instruction sums TWO output pixels.  A = g[pixel lh][co l31], B = patch value of pixel lh at column l31.
//   * A workgroup (4 waves) owns a SPLIT: SB_TPS consecutive 8 x 32-pixel output tiles in (image, tile row, tile column) order -- a function of
//     (N, H, W) alone.  Per tile the 21 x 69-pixel input patch is staged once in LDS with the zero channel dropped; wave w takes output rows 2w, 2w + 1
//     of the tile, 8 pixels at a time: dy (and y) arrive by 16-byte loads -- the next 8 pixels are in flight under the current MFMAs --, the ReLU mask
//     is applied in registers and the 8 x 64 block goes to a wave-private LDS stage, from which the A operand is read as single floats.
//   * LDS banks: the patch row pitch is 214 = 22 + 6 * 32 floats, so column c of filter row ky sits at c + 192 ky: the 32 lanes of a half wave read 32
//     consecutive banks whatever filter rows their columns fall in (ds_read_b32: a lane group is a 32-lane half, conflict-free); the other half reads
//     the next pixel, 6 floats on.  The A reads are 32 consecutive floats per half.
//   * Every wave keeps the whole 64 x 160 product in 10 accumulators (160 registers); at the end of the split the four waves' accumulators are added in
//     wave order through LDS and the slab [64][160] is written to the workspace.  A second launch adds the slabs in index order in fp64, applies
//     `scale` and writes torch's [64][3][7][7].  No atomics, no dependence on the device: two runs are bit-identical.
#include "fd_conv_common.h"

#define SB_TH 8
#define SB_TW 32
#define SB_PR (2 * SB_TH + 5)        // 21 patch rows
#define SB_PC (2 * SB_TW + 5)        // 69 patch pixels per row
#define SB_PITCH 214                 // floats per patch row: 22 + 6 * 32 (>= 208 = the last pixel pair's unused column 21)
#define SB_KR 22                     // columns per filter row: 7 taps x 3 channels + 1 unused
#define SB_NC 160                    // GEMM columns: 7 * 22 = 154 padded to 5 x 32
#define SB_NB (SB_NC / 32)
#define SB_CO 64
#define SB_TPS 8                     // output tiles per split (fixed: the partition is a function of the geometry alone)
#define SB_SLAB (SB_CO * SB_NC)      // floats per partial slab
#define SB_GS 4496                   // float offset of the dy stages behind the patch (21 * 214 = 4494, rounded up to 16 bytes)

struct StemWgradArgs {
    const float4* x; const float* dy; const float* y; float* ws;
    int dy_cs, dy_co, y_cs, y_co, N, H, W, Ho, Wo, tiles_h, tiles_w, ntile;
};

template <bool MASK>
__global__ __launch_bounds__(256, 2) void stem7x7_wgrad_kernel(StemWgradArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[SB_SLAB];      // 40 KB: patch [21][214] + 4 dy stages [8][64]; the cross-wave sum [64][160] at the end
    float* Ps = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    float* Gs = smem + SB_GS + wave * 512;
    // this lane's five GEMM columns c = 32 jb + l31 as patch offsets (filter row ky = c / 22, ky * pitch + c % 22); columns >= 154 read offset 0
    int offB[SB_NB];
#pragma unroll
    for (int jb = 0; jb < SB_NB; ++jb) {
        const int c = 32 * jb + l31, ky = c / SB_KR;
        offB[jb] = (c < 7 * SB_KR ? ky * SB_PITCH + (c - ky * SB_KR) : 0) + lh * 6;
    }
    if (tid < SB_PR)
        for (int i = SB_PC * 3; i < SB_PITCH; ++i) Ps[tid * SB_PITCH + i] = 0.f;

    f32x16 acc[2][SB_NB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < SB_NB; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int t0 = blockIdx.x * SB_TPS, t1 = min(a.ntile, t0 + SB_TPS);
    auto tile_pos = [&](int t, int& n, int& ho0, int& wo0) {
        const int tw = t % a.tiles_w; t /= a.tiles_w;
        const int th = t % a.tiles_h;
        n = t / a.tiles_h; ho0 = th * SB_TH; wo0 = tw * SB_TW;
    };
    // chunk ch of a tile = 8 consecutive pixels of this wave's output row 2 wave + (ch >> 2), column quarter ch & 3; lane -> pixel (lane >> 4) + 4 u, channels 4 (lane & 15) ..
    // The loads are unconditional (a pixel outside the image reads the clamped pixel and is zeroed when it is staged: bit u of dok), so that nothing but
    // their first use waits for them.
    float4 dv[2], yv[2];
    int dok = 0;
    auto load_chunk = [&](int t, int ch) {
        int n, ho0, wo0;
        tile_pos(t, n, ho0, wo0);
        const int oy = ho0 + 2 * wave + (ch >> 2);
        dok = 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ox = wo0 + 8 * (ch & 3) + (lane >> 4) + 4 * u;
            if (oy < a.Ho && ox < a.Wo) dok |= 1 << u;
            const size_t row = ((size_t)n * a.Ho + min(oy, a.Ho - 1)) * a.Wo + min(ox, a.Wo - 1);
            dv[u] = *reinterpret_cast<const float4*>(a.dy + row * a.dy_cs + a.dy_co + 4 * (lane & 15));
            if constexpr (MASK) yv[u] = *reinterpret_cast<const float4*>(a.y + row * a.y_cs + a.y_co + 4 * (lane & 15));
        }
    };
    load_chunk(t0, 0);
    const float* Aop = Gs + lh * SB_CO + l31;
    constexpr int NPX = (SB_PR * SB_PC + 255) / 256;          // patch pixels per thread (6)
    for (int t = t0; t < t1; ++t) {
        int n, ho0, wo0;
        tile_pos(t, n, ho0, wo0);
        {   // the tile's input patch: all of a thread's loads in flight together (clamped address, zero outside the image), then LDS with channel 3 dropped
            const float4* xin = a.x + (size_t)n * a.H * a.W;
            float4 pv[NPX];
#pragma unroll
            for (int u = 0; u < NPX; ++u) {
                const int i = min(tid + 256 * u, SB_PR * SB_PC - 1);
                const int pr = i / SB_PC, pc = i - pr * SB_PC;
                const int hi = 2 * ho0 - 3 + pr, wi = 2 * wo0 - 3 + pc;
                pv[u] = xin[(size_t)min(max(hi, 0), a.H - 1) * a.W + min(max(wi, 0), a.W - 1)];
                if ((unsigned)hi >= (unsigned)a.H || (unsigned)wi >= (unsigned)a.W) pv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            __syncthreads();                   // every wave is done with the previous tile's patch
#pragma unroll
            for (int u = 0; u < NPX; ++u) {
                const int i = tid + 256 * u;
                if (i < SB_PR * SB_PC) {
                    const int pr = i / SB_PC, pc = i - pr * SB_PC;
                    float* d = Ps + pr * SB_PITCH + pc * 3;
                    d[0] = pv[u].x; d[1] = pv[u].y; d[2] = pv[u].z;
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int ch = 0; ch < 8; ++ch) {
            // this chunk: registers -> the wave's stage, masked by the forward output
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float4 g = dv[u];
                const bool ok = (dok >> u) & 1;
                if constexpr (MASK) {
                    g.x = (ok && yv[u].x > 0.f) ? g.x : 0.f; g.y = (ok && yv[u].y > 0.f) ? g.y : 0.f;
                    g.z = (ok && yv[u].z > 0.f) ? g.z : 0.f; g.w = (ok && yv[u].w > 0.f) ? g.w : 0.f;
                } else {
                    g.x = ok ? g.x : 0.f; g.y = ok ? g.y : 0.f; g.z = ok ? g.z : 0.f; g.w = ok ? g.w : 0.f;
                }
                *reinterpret_cast<float4*>(Gs + ((lane >> 4) + 4 * u) * SB_CO + 4 * (lane & 15)) = g;
            }
            const bool live = (ho0 + 2 * wave + (ch >> 2) < a.Ho) && (wo0 + 8 * (ch & 3) < a.Wo);      // (wave-uniform)
            // the next chunk travels under this chunk's MFMAs (after the split's last chunk: the same chunk again, unused)
            {
                const bool more = ch < 7 || t + 1 < t1;
                load_chunk(more ? (ch < 7 ? t : t + 1) : t, more ? ((ch + 1) & 7) : ch);
            }
            wave_lds_sync();
            if (live) {
                const float* Bp = Ps + (2 * (2 * wave + (ch >> 2))) * SB_PITCH + 6 * 8 * (ch & 3);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {          // pixel pair (2 tt, 2 tt + 1) of the chunk: lane half lh carries the second pixel
                    const float a0 = Aop[tt * 2 * SB_CO], a1 = Aop[tt * 2 * SB_CO + 32];
                    float b[SB_NB];
#pragma unroll
                    for (int jb = 0; jb < SB_NB; ++jb) b[jb] = Bp[offB[jb] + 12 * tt];
#pragma unroll
                    for (int jb = 0; jb < SB_NB; ++jb) {
                        acc[0][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[jb], acc[0][jb], 0, 0, 0);
                        acc[1][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[jb], acc[1][jb], 0, 0, 0);
                    }
                }
            }
            wave_lds_sync();                   // the stage is free for the next chunk
        }
    }
    // ---- the four waves' partial products, added in wave order: acc[i][jb] reg e of lane l is D[co 32 i + (e & 3) + 8 (e >> 2) + 4 lh][column 32 jb + l31] ----
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jb = 0; jb < SB_NB; ++jb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        float* d = smem + (32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh) * SB_NC + 32 * jb + l31;
                        *d = (w == 0) ? acc[i][jb][e] : *d + acc[i][jb][e];
                    }
        }
    }
    __syncthreads();
    float4* out = reinterpret_cast<float4*>(a.ws + (size_t)blockIdx.x * SB_SLAB);
    for (int i = tid; i < SB_SLAB / 4; i += 256) out[i] = reinterpret_cast<const float4*>(smem)[i];
}

// dw[co][ci][ky][kx] = scale[co] * (slab 0 + slab 1 + ...), summed in fp64 in slab order: 16 columns x 16 consecutive slab ranges per workgroup, the ranges' sums added in range order
__global__ __launch_bounds__(256) void stem7x7_wgrad_final_kernel(const float* __restrict__ ws, int nsplit, const float* __restrict__ scale, float* __restrict__ dw) {
    __shared__ double part[16][16];
    const int tid = threadIdx.x, el = tid & 15, r = tid >> 4;
    const int e = blockIdx.x * 16 + el;                   // (co, column) of the 64 x 154 real block: 9 856 = 616 x 16
    const int co = e / (7 * SB_KR), c = e - co * (7 * SB_KR);
    const int L = (nsplit + 15) / 16, s0 = r * L, s1 = min(nsplit, s0 + L);
    double sum = 0.0;
    const float* p = ws + co * SB_NC + c;
#pragma unroll 4
    for (int s = s0; s < s1; ++s) sum += (double)p[(size_t)s * SB_SLAB];
    part[r][el] = sum;
    __syncthreads();
    const int ky = c / SB_KR, kk = c - ky * SB_KR;
    if (r == 0 && kk < 21) {
        double tot = 0.0;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) tot += part[rr][el];
        if (scale) tot *= (double)scale[co];
        const int kx = kk / 3, ci = kk - 3 * kx;
        dw[((co * 3 + ci) * 7 + ky) * 7 + kx] = (float)tot;
    }
}

static int64_t stem_wgrad_splits(int32_t N, int32_t H, int32_t W) {
    if (N < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return -1;
    const int64_t Ho = H / 2, Wo = W / 2;
    const int64_t ntile = (int64_t)N * ((Ho + SB_TH - 1) / SB_TH) * ((Wo + SB_TW - 1) / SB_TW);
    if (ntile >= (1LL << 31) - SB_TPS) return -1;
    return (ntile + SB_TPS - 1) / SB_TPS;
}

extern "C" int64_t fd_stem7x7_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    const int64_t ns = stem_wgrad_splits(N, H, W);
    return ns < 0 ? -1 : ns * (int64_t)SB_SLAB * 4;
}

extern "C" int32_t fd_stem7x7_bwd_weight_nhwc4(const float* x4, const float* dy, int32_t dy_cs, int32_t dy_co, const float* y, int32_t y_cs, int32_t y_co,
                                               const float* scale, float* dw, void* workspace, int64_t workspace_bytes, int32_t N, int32_t H, int32_t W,
                                               fd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FD_REQUIRE(x4 && dy && dw && workspace, FD_E_INVAL, "fd_stem7x7_bwd_weight_nhwc4: x4, dy, dw and workspace must not be NULL");
    const int64_t nsplit = stem_wgrad_splits(N, H, W);
    FD_REQUIRE(nsplit > 0, FD_E_INVAL, "fd_stem7x7_bwd_weight_nhwc4: N >= 1 and even H, W >= 2 (got N=%d H=%d W=%d)", N, H, W);
    FD_REQUIRE(dy_cs % 4 == 0 && dy_co % 4 == 0 && dy_co >= 0 && dy_cs >= dy_co + SB_CO, FD_E_INVAL,
               "fd_stem7x7_bwd_weight_nhwc4: dy must be a 64-channel view with cs % 4 == 0, co % 4 == 0, cs >= co + 64 (cs=%d co=%d)", dy_cs, dy_co);
    FD_REQUIRE(!y || (y_cs % 4 == 0 && y_co % 4 == 0 && y_co >= 0 && y_cs >= y_co + SB_CO), FD_E_INVAL,
               "fd_stem7x7_bwd_weight_nhwc4: y must be a 64-channel view with cs % 4 == 0, co % 4 == 0, cs >= co + 64 (cs=%d co=%d)", y_cs, y_co);
    FD_REQUIRE((((uintptr_t)x4 | (uintptr_t)dy | (uintptr_t)y | (uintptr_t)workspace) & 15) == 0 && (((uintptr_t)dw | (uintptr_t)scale) & 3) == 0, FD_E_INVAL,
               "fd_stem7x7_bwd_weight_nhwc4: x4, dy, y and workspace must be 16-byte aligned (dw, scale: 4-byte)");
    FD_REQUIRE(workspace_bytes >= nsplit * (int64_t)SB_SLAB * 4, FD_E_INVAL, "fd_stem7x7_bwd_weight_nhwc4: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)(nsplit * (int64_t)SB_SLAB * 4));
    StemWgradArgs a;
    a.x = reinterpret_cast<const float4*>(x4); a.dy = dy; a.y = y; a.ws = reinterpret_cast<float*>(workspace);
    a.dy_cs = dy_cs; a.dy_co = dy_co; a.y_cs = y_cs; a.y_co = y_co; a.N = N; a.H = H; a.W = W; a.Ho = H / 2; a.Wo = W / 2;
    a.tiles_h = (a.Ho + SB_TH - 1) / SB_TH; a.tiles_w = (a.Wo + SB_TW - 1) / SB_TW; a.ntile = N * a.tiles_h * a.tiles_w;
    if (y) hipLaunchKernelGGL((stem7x7_wgrad_kernel<true>), dim3((unsigned)nsplit), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((stem7x7_wgrad_kernel<false>), dim3((unsigned)nsplit), dim3(256), 0, stream, a);
    FD_CHECK_LAUNCH("fd_stem7x7_bwd_weight_nhwc4");
    hipLaunchKernelGGL(stem7x7_wgrad_final_kernel, dim3(SB_CO * 7 * SB_KR / 16), dim3(256), 0, stream, a.ws, (int)nsplit, scale, dw);
    FD_CHECK_LAUNCH("fd_stem7x7_bwd_weight_nhwc4 (final sum)");
    return FD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Weight gradient of the EfficientNet stem (_conv_stem: 3x3 stride-2 convolution 3 -> Cout, Cout in {32 ... 64}, static "SAME" padding) on the same image
// layout and by the same scheme as the 7x7 kernel above:
//
//   dW[co][ci][ky][kx] = scale[co] * sum over (n, oy, ox) of dy[n][oy][ox][co] * x[n][2 oy - pad_top + ky][2 ox - pad_left + kx][ci]
//
// GEMM: M = Cout (two MFMA row blocks of 32; the second is skipped when Cout <= 32 and its rows >= Cout see zeros), N = 27 tap x channel columns
// c = 9 ky + 3 kx + ci padded to ONE block of 32 (columns 27 ... 31 accumulate the patch's first floats and are never read back), K = every output pixel.
// Tile 8 x 32 output pixels, patch 17 rows x 65 pixels with the zero channel dropped; the row pitch is 201 = 9 + 6 * 32 floats, so column c of filter row ky
// sits at c + 192 ky and the 32 lanes of a half wave read 32 consecutive banks.  A workgroup owns S3_TPS consecutive tiles in (image, tile row, tile column)
// order -- a function of (N, Ho, Wo) alone -- and leaves its [64][32] slab in the workspace; the second launch adds the slabs in index order in fp64,
// applies `scale` and writes torch's [Cout][3][3][3].  No mask variant: the swish behind this stem is an act_rows node that keeps the pre-activation.
#define S3_TH 8
#define S3_TW 32
#define S3_PR (2 * S3_TH + 1)        // 17 patch rows
#define S3_PC (2 * S3_TW + 1)        // 65 patch pixels per row
#define S3_PITCH 201                 // floats per patch row: 9 + 6 * 32 (>= 195)
#define S3_KR 9                      // columns per filter row: 3 taps x 3 channels
#define S3_NCOL 27
#define S3_CO 64
#define S3_TPS 8
#define S3_SLAB (S3_CO * 32)         // floats per partial slab
#define S3_GS 3420                   // float offset of the dy stages behind the patch (17 * 201 = 3417, rounded up to 16 bytes)

struct Stem3WgradArgs {
    const float4* x; const float* dy; float* ws;
    int dy_cs, dy_co, N, H, W, Cout, pad_top, pad_left, Ho, Wo, tiles_h, tiles_w, ntile;
};

__global__ __launch_bounds__(256, 2) void stem3x3_wgrad_kernel(Stem3WgradArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[S3_GS + 4 * 512];      // patch [17][201] + 4 dy stages [8][64]; the cross-wave sum [64][32] at the end
    float* Ps = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    float* Gs = smem + S3_GS + wave * 512;
    const int kyB = l31 / S3_KR;
    const int offB = (l31 < S3_NCOL ? kyB * S3_PITCH + (l31 - kyB * S3_KR) : 0) + lh * 6;
    const bool two = a.Cout > 32;                            // (uniform) the second row block holds channels 32 ...
    if (tid < S3_PR)
        for (int i = S3_PC * 3; i < S3_PITCH; ++i) Ps[tid * S3_PITCH + i] = 0.f;

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    const int t0 = blockIdx.x * S3_TPS, t1 = min(a.ntile, t0 + S3_TPS);
    auto tile_pos = [&](int t, int& n, int& ho0, int& wo0) {
        const int tw = t % a.tiles_w; t /= a.tiles_w;
        const int th = t % a.tiles_h;
        n = t / a.tiles_h; ho0 = th * S3_TH; wo0 = tw * S3_TW;
    };
    // chunk ch of a tile = 8 consecutive pixels of this wave's output row 2 wave + (ch >> 2), column quarter ch & 3; lane -> pixel (lane >> 4) + 4 u, channels 4 (lane & 15) ..
    // Unconditional loads from a clamped pixel and a clamped channel quad (inside the Cout-channel view); what is outside is zeroed when it is staged.
    float4 dv[2];
    int dok = 0;
    const int cq = min(4 * (lane & 15), a.Cout - 4);
    const bool cok = 4 * (lane & 15) < a.Cout;
    auto load_chunk = [&](int t, int ch) {
        int n, ho0, wo0;
        tile_pos(t, n, ho0, wo0);
        const int oy = ho0 + 2 * wave + (ch >> 2);
        dok = 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ox = wo0 + 8 * (ch & 3) + (lane >> 4) + 4 * u;
            if (cok && oy < a.Ho && ox < a.Wo) dok |= 1 << u;
            const size_t row = ((size_t)n * a.Ho + min(oy, a.Ho - 1)) * a.Wo + min(ox, a.Wo - 1);
            dv[u] = *reinterpret_cast<const float4*>(a.dy + row * a.dy_cs + a.dy_co + cq);
        }
    };
    load_chunk(t0, 0);
    const float* Aop = Gs + lh * S3_CO + l31;
    constexpr int NPX = (S3_PR * S3_PC + 255) / 256;          // patch pixels per thread (5)
    for (int t = t0; t < t1; ++t) {
        int n, ho0, wo0;
        tile_pos(t, n, ho0, wo0);
        {
            const float4* xin = a.x + (size_t)n * a.H * a.W;
            float4 pv[NPX];
#pragma unroll
            for (int u = 0; u < NPX; ++u) {
                const int i = min(tid + 256 * u, S3_PR * S3_PC - 1);
                const int pr = i / S3_PC, pc = i - pr * S3_PC;
                const int hi = 2 * ho0 - a.pad_top + pr, wi = 2 * wo0 - a.pad_left + pc;
                pv[u] = xin[(size_t)min(max(hi, 0), a.H - 1) * a.W + min(max(wi, 0), a.W - 1)];
                if ((unsigned)hi >= (unsigned)a.H || (unsigned)wi >= (unsigned)a.W) pv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            __syncthreads();                   // every wave is done with the previous tile's patch
#pragma unroll
            for (int u = 0; u < NPX; ++u) {
                const int i = tid + 256 * u;
                if (i < S3_PR * S3_PC) {
                    const int pr = i / S3_PC, pc = i - pr * S3_PC;
                    float* d = Ps + pr * S3_PITCH + pc * 3;
                    d[0] = pv[u].x; d[1] = pv[u].y; d[2] = pv[u].z;
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int ch = 0; ch < 8; ++ch) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float4 g = dv[u];
                const bool ok = (dok >> u) & 1;
                g.x = ok ? g.x : 0.f; g.y = ok ? g.y : 0.f; g.z = ok ? g.z : 0.f; g.w = ok ? g.w : 0.f;
                *reinterpret_cast<float4*>(Gs + ((lane >> 4) + 4 * u) * S3_CO + 4 * (lane & 15)) = g;
            }
            const bool live = (ho0 + 2 * wave + (ch >> 2) < a.Ho) && (wo0 + 8 * (ch & 3) < a.Wo);      // (wave-uniform)
            {
                const bool more = ch < 7 || t + 1 < t1;
                load_chunk(more ? (ch < 7 ? t : t + 1) : t, more ? ((ch + 1) & 7) : ch);
            }
            wave_lds_sync();
            if (live) {
                const float* Bp = Ps + (2 * (2 * wave + (ch >> 2))) * S3_PITCH + 6 * 8 * (ch & 3);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {          // pixel pair (2 tt, 2 tt + 1) of the chunk: lane half lh carries the second pixel
                    const float b = Bp[offB + 12 * tt];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Aop[tt * 2 * S3_CO], b, acc[0], 0, 0, 0);
                    if (two) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Aop[tt * 2 * S3_CO + 32], b, acc[1], 0, 0, 0);
                }
            }
            wave_lds_sync();                   // the stage is free for the next chunk
        }
    }
    // ---- the four waves' partial products, added in wave order: acc[i] reg e of lane l is D[co 32 i + (e & 3) + 8 (e >> 2) + 4 lh][column l31] ----
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float* d = smem + (32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + l31;
                    *d = (w == 0) ? acc[i][e] : *d + acc[i][e];
                }
        }
    }
    __syncthreads();
    float4* out = reinterpret_cast<float4*>(a.ws + (size_t)blockIdx.x * S3_SLAB);
    for (int i = tid; i < S3_SLAB / 4; i += 256) out[i] = reinterpret_cast<const float4*>(smem)[i];
}

// dw[co][ci][ky][kx] = scale[co] * (slab 0 + slab 1 + ...), summed in fp64 in slab order: 16 (co, column) elements x 16 consecutive slab ranges per workgroup
__global__ __launch_bounds__(256) void stem3x3_wgrad_final_kernel(const float* __restrict__ ws, int nsplit, int Cout, const float* __restrict__ scale,
                                                                   float* __restrict__ dw) {
    __shared__ double part[16][16];
    const int tid = threadIdx.x, el = tid & 15, r = tid >> 4;
    const int e = blockIdx.x * 16 + el;
    const bool ok = e < Cout * S3_NCOL;
    const int co = ok ? e / S3_NCOL : 0, c = ok ? e - co * S3_NCOL : 0;
    const int L = (nsplit + 15) / 16, s0 = r * L, s1 = min(nsplit, s0 + L);
    double sum = 0.0;
    const float* p = ws + co * 32 + c;
#pragma unroll 4
    for (int s = s0; s < s1; ++s) sum += (double)p[(size_t)s * S3_SLAB];
    part[r][el] = sum;
    __syncthreads();
    if (r == 0 && ok) {
        double tot = 0.0;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) tot += part[rr][el];
        if (scale) tot *= (double)scale[co];
        const int ky = c / S3_KR, kk = c - ky * S3_KR, kx = kk / 3, ci = kk - 3 * kx;
        dw[((co * 3 + ci) * 3 + ky) * 3 + kx] = (float)tot;
    }
}

static int64_t stem3_wgrad_splits(int32_t N, int32_t H, int32_t W, int32_t Ho, int32_t Wo) {
    if (N < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || (int64_t)N * H * W >= (1LL << 31) || (int64_t)N * Ho * Wo >= (1LL << 31)) return -1;
    const int64_t ntile = (int64_t)N * ((Ho + S3_TH - 1) / S3_TH) * ((Wo + S3_TW - 1) / S3_TW);
    return (ntile + S3_TPS - 1) / S3_TPS;
}

extern "C" int64_t fd_stem_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t Ho, int32_t Wo) {
    if (Cout < 4 || Cout > S3_CO || Cout % 4) return -1;
    const int64_t ns = stem3_wgrad_splits(N, H, W, Ho, Wo);
    return ns < 0 ? -1 : ns * (int64_t)S3_SLAB * 4;
}

extern "C" int32_t fd_stem_conv_bwd_weight_nhwc4(const float* x4, const float* dy, int32_t dy_cs, int32_t dy_co, const float* scale, float* dw,
                                                 void* workspace, int64_t workspace_bytes, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t K,
                                                 int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, fd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FD_REQUIRE(K == 3 && stride == 2 && Cout >= 4 && Cout <= S3_CO && Cout % 4 == 0, FD_E_UNSUPPORTED,
               "fd_stem_conv_bwd_weight_nhwc4: K = 3, stride = 2, Cout %% 4 == 0, Cout <= 64 supported (got K=%d stride=%d Cout=%d)", K, stride, Cout);
    FD_REQUIRE(x4 && dy && dw && workspace, FD_E_INVAL, "fd_stem_conv_bwd_weight_nhwc4: x4, dy, dw and workspace must not be NULL");
    const int64_t nsplit = stem3_wgrad_splits(N, H, W, Ho, Wo);
    FD_REQUIRE(nsplit > 0 && pad_top >= 0 && pad_top < 3 && pad_left >= 0 && pad_left < 3 && 2 * ((int64_t)Ho - 1) - pad_top < H && 2 * ((int64_t)Wo - 1) - pad_left < W,
               FD_E_INVAL, "fd_stem_conv_bwd_weight_nhwc4: bad geometry (N=%d H=%d W=%d pad=(%d, %d) Ho=%d Wo=%d)", N, H, W, pad_top, pad_left, Ho, Wo);
    FD_REQUIRE(dy_cs % 4 == 0 && dy_co % 4 == 0 && dy_co >= 0 && dy_cs >= dy_co + Cout, FD_E_INVAL,
               "fd_stem_conv_bwd_weight_nhwc4: dy must be a Cout-channel view with cs %% 4 == 0, co %% 4 == 0, cs >= co + Cout (cs=%d co=%d)", dy_cs, dy_co);
    FD_REQUIRE((((uintptr_t)x4 | (uintptr_t)dy | (uintptr_t)workspace) & 15) == 0 && (((uintptr_t)dw | (uintptr_t)scale) & 3) == 0, FD_E_INVAL,
               "fd_stem_conv_bwd_weight_nhwc4: x4, dy and workspace must be 16-byte aligned (dw, scale: 4-byte)");
    FD_REQUIRE(workspace_bytes >= nsplit * (int64_t)S3_SLAB * 4, FD_E_INVAL, "fd_stem_conv_bwd_weight_nhwc4: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)(nsplit * (int64_t)S3_SLAB * 4));
    Stem3WgradArgs a;
    a.x = reinterpret_cast<const float4*>(x4); a.dy = dy; a.ws = reinterpret_cast<float*>(workspace);
    a.dy_cs = dy_cs; a.dy_co = dy_co; a.N = N; a.H = H; a.W = W; a.Cout = Cout; a.pad_top = pad_top; a.pad_left = pad_left; a.Ho = Ho; a.Wo = Wo;
    a.tiles_h = (Ho + S3_TH - 1) / S3_TH; a.tiles_w = (Wo + S3_TW - 1) / S3_TW; a.ntile = N * a.tiles_h * a.tiles_w;
    hipLaunchKernelGGL(stem3x3_wgrad_kernel, dim3((unsigned)nsplit), dim3(256), 0, stream, a);
    FD_CHECK_LAUNCH("fd_stem_conv_bwd_weight_nhwc4");
    hipLaunchKernelGGL(stem3x3_wgrad_final_kernel, dim3((Cout * S3_NCOL + 15) / 16), dim3(256), 0, stream, (const float*)a.ws, (int)nsplit, Cout, scale, dw);
    FD_CHECK_LAUNCH("fd_stem_conv_bwd_weight_nhwc4 (final sum)");
    return FD_OK;
}
