// fd_mbconv_bwd.hip — backward of the MBConv depthwise conv (fd_dwconv2d_nhwc, fd_mbconv.hip) on NHWC fp32 channel views (gfx950):
// depthwise k x k, k in {3, 5}, stride in {1, 2}, asymmetric (TensorFlow "SAME", static) zero padding -- the caller states the top / left padding and the
// output size, as for the forward.
//   * fd_dwconv2d_bwd_data_nhwc    dx[n,h,w,c] = scale[c] * sum_{r,s} dy[n,ho,wo,c] * w[r,s,c] over the taps with (h + pad_top - r) = stride * ho, ho in [0, Ho)
//                                  (and the same along w).  Gather form: EVERY dx pixel of the view is written, the rows / columns no window reaches as 0.
//   * fd_dwconv2d_bwd_weight_nhwc  dw[r,s,c] = scale[c] * sum_{n,ho,wo} dy[n,ho,wo,c] * x[n, ho*stride - pad_top + r, wo*stride - pad_left + s, c], two phases
//                                  (fixed-partition partial sums, then dw_wgrad_final_kernel): deterministic, no float atomics.
// Both are HBM-bound: 16 bytes per lane, the data gradient with dwconv_kxk_kernel's access pattern (S adjacent pixels per thread, the weights of a kernel row
// read once per S outputs), the weight gradient with dwconv_dilated_wgrad_partial_kernel's partition (fd_layers.hip) over strips of S adjacent dy pixels.
#include "fd_common.h"
#include "fd_dw_wgrad_final.inc"

#define FD_GRID_CAP 16384

static inline unsigned grid_for(long work, int block) {
    long g = (work + block - 1) / block;
    if (g > FD_GRID_CAP) g = FD_GRID_CAP;
    if (g < 1) g = 1;
    return (unsigned)g;
}

static inline bool view_ok(const void* p, int cs, int co, int C) {
    return p && C >= 4 && C % 4 == 0 && cs % 4 == 0 && co >= 0 && co % 4 == 0 && cs >= co + C && ((uintptr_t)p & 15) == 0;
}

// what both entries ask of the geometry: the forward's own conditions (fd_dwconv2d_nhwc)
static inline bool geom_ok(int N, int H, int W, int Ho, int Wo, int K, int stride, int pad_top, int pad_left) {
    return N >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 && pad_top >= 0 && pad_left >= 0 && pad_top < K && pad_left < K &&
           (long)(Ho - 1) * stride - pad_top < H && (long)(Wo - 1) * stride - pad_left < W;
}

// ------------------------------------------------------------------------------ data gradient
// One thread = S adjacent dx pixels of one row x one channel quad.  Along a row the S pixels start at w0 = S * strip (even: S is), so with A = w0 + pad_left
// = 2a + PL (PL = the parity of pad_left, a template parameter at stride 2) pixel j meets tap s where PL + j - s is even, at dy column a + (PL + j - s) / 2:
// the window of dy columns [a - (K-1)/2, ...) is loaded once per visited kernel row and every index into it is a compile-time constant.  Along the rows only the
// kernel rows of the matching parity are visited.  At stride 1 every tap is met and the window is the forward's with the taps reversed.
template <int K, int STRIDE, int PL, int S>
__global__ __launch_bounds__(256) void dwconv_kxk_dgrad_kernel(const float* __restrict__ dy, int dy_cs, int dy_co, const float* __restrict__ wt,
                                                                const float* __restrict__ scale, float* __restrict__ dx, int dx_cs, int dx_co, int C,
                                                                int H, int W, int Ho, int Wo, int pad_t, int pad_l, long total) {
    constexpr int HALF = (K - 1) / 2;
    constexpr int NW = STRIDE == 1 ? S - 1 + K : (PL + S - 1) / 2 + HALF + 1;       // dy columns a thread's S pixels touch
    const int C4 = C >> 2;
    const int spr = (W + S - 1) / S;           // strips per dx row
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int q;
        long t = fd_div(i, C4, q);
        int sx; t = fd_div(t, spr, sx);
        int h;
        const long n = fd_div(t, H, h);
        const int w0 = sx * S;
        // first dy column of the window: stride 1: w0 + pad_l - (K - 1); stride 2: (w0 + pad_l - PL) / 2 - HALF
        const int b = STRIDE == 1 ? w0 + pad_l - (K - 1) : ((w0 + pad_l - PL) >> 1) - HALF;
        const float* gb = dy + (n * Ho * (long)Wo) * dy_cs + dy_co + 4 * q;
        float4 acc[S];
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int hr = h + pad_t - r;
            if (STRIDE == 2 && (hr & 1)) continue;                        // the other parity: no output row meets this tap
            const int ho = STRIDE == 1 ? hr : hr >> 1;
            if ((unsigned)ho >= (unsigned)Ho) continue;
            float4 u[NW];
#pragma unroll
            for (int c = 0; c < NW; ++c) {
                const int wo = b + c;
                u[c] = (unsigned)wo < (unsigned)Wo ? *reinterpret_cast<const float4*>(gb + ((long)ho * Wo + wo) * dy_cs)
                                                  : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const float4 k = *reinterpret_cast<const float4*>(wt + (r * K + s) * C + 4 * q);
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    if (STRIDE == 1 || ((PL + j - s) & 1) == 0) {         // (compile-time: j and s are unrolled)
                        const int idx = STRIDE == 1 ? j - s + K - 1 : (PL + j - s + 2 * HALF) / 2;
                        if ((unsigned)(b + idx) < (unsigned)Wo) {         // a tap outside dy adds nothing (not even +0*w)
                            const float4 v = u[idx];
                            acc[j].x = fmaf(v.x, k.x, acc[j].x); acc[j].y = fmaf(v.y, k.y, acc[j].y);
                            acc[j].z = fmaf(v.z, k.z, acc[j].z); acc[j].w = fmaf(v.w, k.w, acc[j].w);
                        }
                    }
                }
            }
        }
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
        if (scale) sc = *reinterpret_cast<const float4*>(scale + 4 * q);
        float* xb = dx + ((n * H + h) * (long)W) * dx_cs + dx_co + 4 * q;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if (w0 + j >= W) break;
            *reinterpret_cast<float4*>(xb + (long)(w0 + j) * dx_cs) = make_float4(acc[j].x * sc.x, acc[j].y * sc.y, acc[j].z * sc.z, acc[j].w * sc.w);
        }
    }
}

extern "C" int32_t fd_dwconv2d_bwd_data_nhwc(const float* dy, int32_t dy_cs, int32_t dy_co, const float* w, const float* scale, float* dx,
                                             int32_t dx_cs, int32_t dx_co, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride,
                                             int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, fd_stream_t stream) {
    FD_REQUIRE((K == 3 || K == 5) && (stride == 1 || stride == 2), FD_E_UNSUPPORTED,
               "fd_dwconv2d_bwd_data: kernel %d stride %d has no kernel (k in {3,5}, stride in {1,2})", K, stride);
    FD_REQUIRE(view_ok(dy, dy_cs, dy_co, C) && view_ok(dx, dx_cs, dx_co, C) && w && ((uintptr_t)w & 15) == 0 && ((uintptr_t)scale & 15) == 0, FD_E_INVAL,
               "fd_dwconv2d_bwd_data: channel views must be 4-aligned, pointers 16-byte aligned (C=%d)", C);
    FD_REQUIRE(geom_ok(N, H, W, Ho, Wo, K, stride, pad_top, pad_left), FD_E_INVAL,
               "fd_dwconv2d_bwd_data: output %dx%d reaches past the %dx%d input (k=%d s=%d pad %d/%d)", Ho, Wo, H, W, K, stride, pad_top, pad_left);
    FD_REQUIRE((long)N * H * W * dx_cs < (1L << 31) * 4 && (long)N * Ho * Wo * dy_cs < (1L << 31) * 4, FD_E_UNSUPPORTED,
               "fd_dwconv2d_bwd_data: tensor too large");
    constexpr int S = 4;
    const long total = (long)N * H * ((W + S - 1) / S) * (C / 4);
    hipStream_t st = (hipStream_t)stream;
#define FD_DWB_LAUNCH(KK, SS, PP)                                                                                                         \
    hipLaunchKernelGGL((dwconv_kxk_dgrad_kernel<KK, SS, PP, S>), dim3(grid_for(total, 256)), dim3(256), 0, st, dy, dy_cs, dy_co, w, scale, \
                       dx, dx_cs, dx_co, C, H, W, Ho, Wo, pad_top, pad_left, total)
    const int pl = pad_left & 1;
    if (K == 3 && stride == 1) FD_DWB_LAUNCH(3, 1, 0);
    else if (K == 5 && stride == 1) FD_DWB_LAUNCH(5, 1, 0);
    else if (K == 3 && pl == 0) FD_DWB_LAUNCH(3, 2, 0);
    else if (K == 3) FD_DWB_LAUNCH(3, 2, 1);
    else if (pl == 0) FD_DWB_LAUNCH(5, 2, 0);
    else FD_DWB_LAUNCH(5, 2, 1);
#undef FD_DWB_LAUNCH
    FD_CHECK_LAUNCH("fd_dwconv2d_bwd_data_nhwc");
    return FD_OK;
}

// ------------------------------------------------------------------------------ weight gradient
// Phase 1, dwconv_dilated_wgrad_partial_kernel's scheme on the strided geometry: one workgroup = (chunk of dy STRIPS, kernel row r); a strip is S adjacent dy
// pixels of one output row.  A thread owns one channel quad and every R-th strip of the chunk and keeps the K tap sums of kernel row r: per strip it loads the
// S dy quads and the (S - 1) * STRIDE + K window of x once (a pixel-per-thread form reads x K times per kernel row: 25 L2 reads per input pixel at k = 5).
// The row lanes are added in lane order through LDS -> part[chunk][K*K][C].  The K workgroups of a chunk have block ids congruent mod 8 (they read the same
// dy rows: an L2 hint, the result does not depend on it).  A chunk past the last strip writes zeros: the final kernel adds every chunk.
template <int K, int STRIDE, int S>
__global__ __launch_bounds__(256) void dwconv_kxk_wgrad_partial_kernel(const float* __restrict__ x, int x_cs, int x_co, const float* __restrict__ dy,
                                                                        int dy_cs, int dy_co, int C, int QW, int pad_t, int pad_l, int H, int W, int Ho,
                                                                        int Wo, long strips, long chunk_strips, int nchunk, float* __restrict__ part) {
    constexpr int WIN = (S - 1) * STRIDE + K;
    __shared__ float4 red[256];
    const int id = blockIdx.x;
    const int r = (id >> 3) % K;                                 // kernel row of this workgroup
    const int chunk = ((id >> 3) / K) * 8 + (id & 7);
    if (chunk >= nchunk) return;                                 // (the grid is rounded up to 8 chunks; uniform per workgroup)
    const int tid = threadIdx.x;
    const int R = 256 / QW;                                      // row lanes
    const int ql = tid % QW, rl = tid / QW;
    const int q = blockIdx.y * QW + ql;                          // channel quad
    const bool live = 4 * q < C;
    const int spr = (Wo + S - 1) / S;                            // strips per dy row
    const long m0 = (long)chunk * chunk_strips;
    const long m1 = min(strips, m0 + chunk_strips);
    float4 acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (long m = m0 + rl; m < m1; m += R) {
            int sx, ho;
            long t = fd_div(m, spr, sx);
            const long n = fd_div(t, Ho, ho);
            const int hi = ho * STRIDE - pad_t + r;
            if ((unsigned)hi >= (unsigned)H) continue;
            const int wo0 = sx * S, wi0 = wo0 * STRIDE - pad_l;
            const float* grow = dy + ((n * Ho + ho) * (long)Wo) * dy_cs + dy_co + 4 * q;
            const float* xrow = x + ((n * H + hi) * (long)W) * x_cs + x_co + 4 * q;
            float4 g[S], u[WIN];
#pragma unroll
            for (int j = 0; j < S; ++j)
                g[j] = wo0 + j < Wo ? *reinterpret_cast<const float4*>(grow + (long)(wo0 + j) * dy_cs) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int c = 0; c < WIN; ++c) {
                const int wi = wi0 + c;
                u[c] = (unsigned)wi < (unsigned)W ? *reinterpret_cast<const float4*>(xrow + (long)wi * x_cs) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (wo0 + j >= Wo) break;
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    if ((unsigned)(wi0 + j * STRIDE + c) >= (unsigned)W) continue;       // a tap outside the input adds nothing (not even +0*dy)
                    const float4 v = u[j * STRIDE + c];
                    float4& a = acc[c];
                    a.x = fmaf(v.x, g[j].x, a.x); a.y = fmaf(v.y, g[j].y, a.y);
                    a.z = fmaf(v.z, g[j].z, a.z); a.w = fmaf(v.w, g[j].w, a.w);
                }
            }
        }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        red[tid] = acc[c];
        __syncthreads();
        if (rl == 0 && live) {
            float4 v = red[ql];
            for (int j = 1; j < R; ++j) {
                const float4 u = red[j * QW + ql];
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
            *reinterpret_cast<float4*>(part + ((long)chunk * (K * K) + r * K + c) * C + 4 * q) = v;
        }
        __syncthreads();
    }
}

extern "C" int64_t fd_dwconv2d_wgrad_workspace_bytes(int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t K) {
    if (N < 1 || Ho < 1 || Wo < 1 || C < 4 || C % 4 || !(K == 3 || K == 5)) return -1;
    return (int64_t)dw_wgrad_chunks((long)N * Ho * Wo) * K * K * C * 4;
}

extern "C" int32_t fd_dwconv2d_bwd_weight_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co, float* dw,
                                               int32_t C, int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t N, int32_t H, int32_t W,
                                               int32_t Ho, int32_t Wo, const float* scale, int32_t layout, void* workspace, fd_stream_t stream) {
    FD_REQUIRE((K == 3 || K == 5) && (stride == 1 || stride == 2), FD_E_UNSUPPORTED,
               "fd_dwconv2d_bwd_weight: kernel %d stride %d has no kernel (k in {3,5}, stride in {1,2})", K, stride);
    FD_REQUIRE(view_ok(x, x_cs, x_co, C) && view_ok(dy, dy_cs, dy_co, C) && dw && workspace && ((uintptr_t)workspace & 15) == 0, FD_E_INVAL,
               "fd_dwconv2d_bwd_weight: channel views must be 4-aligned, dw and a 16-byte aligned workspace given (C=%d)", C);
    FD_REQUIRE(layout == 0 || layout == 1, FD_E_INVAL, "fd_dwconv2d_bwd_weight: layout 0 ([K*K][C]) or 1 ([C][1][K][K]) (got %d)", layout);
    FD_REQUIRE(geom_ok(N, H, W, Ho, Wo, K, stride, pad_top, pad_left), FD_E_INVAL,
               "fd_dwconv2d_bwd_weight: output %dx%d reaches past the %dx%d input (k=%d s=%d pad %d/%d)", Ho, Wo, H, W, K, stride, pad_top, pad_left);
    FD_REQUIRE((long)N * H * W * x_cs < (1L << 31) * 4 && (long)N * Ho * Wo * dy_cs < (1L << 31) * 4, FD_E_UNSUPPORTED,
               "fd_dwconv2d_bwd_weight: tensor too large");
    const int C4 = C / 4;
    // channel quads per workgroup: a power of two <= 64, the other 256 / QW >= 4 thread groups are row lanes.  (Up to 256 quads, as the dilated kernel takes them,
    // left one row lane at C = 816: 64 dependent rows per thread and 320 workgroups for the 16 x 16^2 map, 0.08 of the HBM rate.)
    int QW = 1;
    while (QW < C4 && QW < 64) QW *= 2;
    constexpr int S = 4;
    const int nchunk = dw_wgrad_chunks((long)N * Ho * Wo);       // (the workspace query's count)
    const long strips = (long)N * Ho * ((Wo + S - 1) / S);
    const long chunk_strips = (strips + nchunk - 1) / nchunk;
    const dim3 grid((nchunk + 7) / 8 * 8 * K, (C4 + QW - 1) / QW);
    hipStream_t st = (hipStream_t)stream;
#define FD_DWW_LAUNCH(KK, SS)                                                                                                                 \
    hipLaunchKernelGGL((dwconv_kxk_wgrad_partial_kernel<KK, SS, S>), grid, dim3(256), 0, st, x, x_cs, x_co, dy, dy_cs, dy_co, C, QW, pad_top, pad_left, \
                       H, W, Ho, Wo, strips, chunk_strips, nchunk, (float*)workspace)
    if (K == 3 && stride == 1) FD_DWW_LAUNCH(3, 1);
    else if (K == 3) FD_DWW_LAUNCH(3, 2);
    else if (stride == 1) FD_DWW_LAUNCH(5, 1);
    else FD_DWW_LAUNCH(5, 2);
#undef FD_DWW_LAUNCH
    FD_CHECK_LAUNCH("fd_dwconv2d_bwd_weight_nhwc (partial)");
    hipLaunchKernelGGL(dw_wgrad_final_kernel, dim3((K * K * C + 15) / 16), dim3(256), 0, st, (const float*)workspace, dw, K * K * C, nchunk, scale, layout, C,
                       K * K);
    FD_CHECK_LAUNCH("fd_dwconv2d_bwd_weight_nhwc (final)");
    return FD_OK;
}
