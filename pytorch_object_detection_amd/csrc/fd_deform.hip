// fd_deform.hip — modulated deformable convolution ("DCNv2", the reference's DeformableConv2d, model/modules/modules.py:219-277) as a sampler in front
// of the dense-conv GEMM: fd_deform_im2col_nhwc writes the bilinearly sampled, mask-weighted columns [B*Ho*Wo][K*K*C] (tap major, then channel),
// fd_deform_bwd_nhwc turns the gradient of those columns into the gradients of the offsets, the mask and (scattered) the input map.
// The sampling rule is the project's own statement of the published algorithm (include/fcosdet.h).
#include "fd_common.h"

#define FD_GRID_CAP 16384

static inline unsigned grid_for(long work, int block) {
    long g = (work + block - 1) / block;
    if (g > FD_GRID_CAP) g = FD_GRID_CAP;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// maps read / written four channels at a time
static inline int view4_ok(const void* p, int cs, int co, int C) {
    return p && ((uintptr_t)p & 15) == 0 && C >= 4 && (C & 3) == 0 && (cs & 3) == 0 && (co & 3) == 0 && co >= 0 && cs >= co + C;
}
// maps read / written one float at a time (offset: 2*K*K channels, mask: K*K channels -- 18 and 9 for a 3x3 layer)
static inline int view1_ok(const void* p, int cs, int co, int C) {
    return p && ((uintptr_t)p & 3) == 0 && C >= 1 && co >= 0 && cs >= co + C;
}

struct DeformGeom {
    int H, W, Ho, Wo, C, K, stride, pad, dil;
};

// One (output pixel, tap) item: the four bilinear corner weights (0 where the corner lies outside the map), the corner addresses and the mask.
struct DeformTap {
    long r00, r01, r10, r11;     // input-map rows of the four corners, clamped into the map: always readable when `inside`, the true rows where the corner is valid
    float w00, w01, w10, w11;
    float ly, lx, mask;
    bool v00, v01, v10, v11, inside;
};

// Written so that a NaN / infinite offset counts as outside: the corner rows below are then never formed.
__device__ __forceinline__ DeformTap deform_tap(const DeformGeom& g, long m, int t, const float* __restrict__ off, int off_cs, int off_co,
                                                const float* __restrict__ mask, int mask_cs, int mask_co, int mask_act) {
    DeformTap s;
    int wo, ho;
    long b = fd_div(m, g.Wo, wo);
    b = fd_div(b, g.Ho, ho);
    const int i = t / g.K, j = t - i * g.K;
    const float* o = off + m * off_cs + off_co + 2 * t;
    const float y = (float)(ho * g.stride - g.pad + i * g.dil) + o[0];
    const float x = (float)(wo * g.stride - g.pad + j * g.dil) + o[1];
    s.inside = y > -1.0f && y < (float)g.H && x > -1.0f && x < (float)g.W;
    s.mask = 1.0f;
    if (mask) {
        const float v = mask[m * mask_cs + mask_co + t];
        s.mask = mask_act ? 2.0f * fd_sigmoid(v) : v;
    }
    s.v00 = s.v01 = s.v10 = s.v11 = false;
    s.w00 = s.w01 = s.w10 = s.w11 = s.ly = s.lx = 0.f;
    s.r00 = s.r01 = s.r10 = s.r11 = 0;
    if (!s.inside) return s;
    const float fy = floorf(y), fx = floorf(x);
    const int y0 = (int)fy, x0 = (int)fx;            // in [-1, H - 1] x [-1, W - 1]
    s.ly = y - fy;
    s.lx = x - fx;
    const bool ya = y0 >= 0, yb = y0 + 1 < g.H, xa = x0 >= 0, xb = x0 + 1 < g.W;
    s.v00 = ya && xa; s.v01 = ya && xb; s.v10 = yb && xa; s.v11 = yb && xb;
    s.w00 = (1.0f - s.ly) * (1.0f - s.lx);
    s.w01 = (1.0f - s.ly) * s.lx;
    s.w10 = s.ly * (1.0f - s.lx);
    s.w11 = s.ly * s.lx;
    const int yc0 = y0 < 0 ? 0 : y0, yc1 = yb ? y0 + 1 : g.H - 1, xc0 = x0 < 0 ? 0 : x0, xc1 = xb ? x0 + 1 : g.W - 1;
    const long ra = (b * g.H + yc0) * g.W, rb = (b * g.H + yc1) * g.W;
    s.r00 = ra + xc0; s.r01 = ra + xc1; s.r10 = rb + xc0; s.r11 = rb + xc1;
    return s;
}

// v or zero, component by component (a select between two float4 objects is compiled through scratch memory)
__device__ __forceinline__ float4 keep4(bool keep, const float4& v) {
    return make_float4(keep ? v.x : 0.f, keep ? v.y : 0.f, keep ? v.z : 0.f, keep ? v.w : 0.f);
}

// Lanes of a wave are split into groups of `lpi` lanes (64, or the channel-chunk count when that is a smaller power of two); a group owns one item.
static inline int lanes_per_item(int chunks) {
    return (chunks < 64 && (64 % chunks) == 0) ? chunks : 64;
}

// ---- forward: a lane group owns one (pixel, tap); its lanes run over the channel quads, so each corner is one contiguous read
__global__ __launch_bounds__(256) void deform_im2col_kernel(const float* __restrict__ x, int x_cs, int x_co, const float* __restrict__ off, int off_cs,
                                                             int off_co, const float* __restrict__ mask, int mask_cs, int mask_co, int mask_act,
                                                             float* __restrict__ cols, int cols_cs, int cols_co, DeformGeom g, int lpi, long items) {
    const int KK = g.K * g.K, C4 = g.C >> 2;
    const int per_block = 256 / lpi;
    const int sub = threadIdx.x / lpi, q0 = threadIdx.x - sub * lpi;
    for (long it = (long)blockIdx.x * per_block + sub; it < items; it += (long)gridDim.x * per_block) {
        int t;
        const long m = fd_div(it, KK, t);
        const DeformTap s = deform_tap(g, m, t, off, off_cs, off_co, mask, mask_cs, mask_co, mask_act);
        float* dst = cols + m * cols_cs + cols_co + (long)t * g.C;
        if (!s.inside) {            // fully outside: zeros, x is not touched
            for (int q = q0; q < C4; q += lpi) *reinterpret_cast<float4*>(dst + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float a00 = s.w00 * s.mask, a01 = s.w01 * s.mask, a10 = s.w10 * s.mask, a11 = s.w11 * s.mask;
        const float* p00 = x + s.r00 * x_cs + x_co;
        const float* p01 = x + s.r01 * x_cs + x_co;
        const float* p10 = x + s.r10 * x_cs + x_co;
        const float* p11 = x + s.r11 * x_cs + x_co;
        for (int q = q0; q < C4; q += lpi) {
            // the four corner reads are unconditional (clamped rows) so that they are in flight together; a corner outside the map is replaced by zero afterwards
            float4 v00 = *reinterpret_cast<const float4*>(p00 + 4 * q);
            float4 v01 = *reinterpret_cast<const float4*>(p01 + 4 * q);
            float4 v10 = *reinterpret_cast<const float4*>(p10 + 4 * q);
            float4 v11 = *reinterpret_cast<const float4*>(p11 + 4 * q);
            v00 = keep4(s.v00, v00); v01 = keep4(s.v01, v01); v10 = keep4(s.v10, v10); v11 = keep4(s.v11, v11);
            float4 acc;
            acc.x = fmaf(a11, v11.x, fmaf(a10, v10.x, fmaf(a01, v01.x, a00 * v00.x)));
            acc.y = fmaf(a11, v11.y, fmaf(a10, v10.y, fmaf(a01, v01.y, a00 * v00.y)));
            acc.z = fmaf(a11, v11.z, fmaf(a10, v10.z, fmaf(a01, v01.z, a00 * v00.z)));
            acc.w = fmaf(a11, v11.w, fmaf(a10, v10.w, fmaf(a01, v01.w, a00 * v00.w)));
            *reinterpret_cast<float4*>(dst + 4 * q) = acc;
        }
    }
}

// ---- backward: a lane group owns one (pixel, tap); its lanes run over single channels, so that every atomic wave-instruction of the d_x scatter adds
// to contiguous floats of one input row (256 bytes at C >= 64).  The three channel sums (d_offset y / x, d_mask) are folded inside the group by a
// butterfly of a fixed shape: bit-identical from run to run.  d_x is added with fp32 atomics in arrival order: not bit-reproducible.
__global__ __launch_bounds__(256) void deform_bwd_kernel(const float* __restrict__ dcols, int dc_cs, int dc_co, const float* __restrict__ x, int x_cs, int x_co,
                                                          const float* __restrict__ off, int off_cs, int off_co, const float* __restrict__ mask, int mask_cs,
                                                          int mask_co, int mask_act, float* __restrict__ d_off, int do_cs, int do_co,
                                                          float* __restrict__ d_mask, int dm_cs, int dm_co, float* __restrict__ d_x, int dx_cs, int dx_co,
                                                          DeformGeom g, int lpi, long items) {
    const int KK = g.K * g.K;
    const int per_block = 256 / lpi;
    const int sub = threadIdx.x / lpi, c0 = threadIdx.x - sub * lpi;
    const long span = (long)gridDim.x * per_block;
    const long rounds = (items + span - 1) / span;      // every lane takes part in every butterfly: idle groups run on with a zero contribution
    for (long r = 0; r < rounds; ++r) {
        const long it = r * span + (long)blockIdx.x * per_block + sub;
        const bool live = it < items;
        int t = 0;
        const long m = live ? fd_div(it, KK, t) : 0;
        DeformTap s;
        s.inside = false;
        if (live) s = deform_tap(g, m, t, off, off_cs, off_co, mask, mask_cs, mask_co, mask_act);
        float sy = 0.f, sx = 0.f, sm = 0.f;
        if (live && s.inside) {
            const float* gp = dcols + m * dc_cs + dc_co + (long)t * g.C;
            const long o00 = s.r00, o01 = s.r01, o10 = s.r10, o11 = s.r11;
            const float a00 = s.w00 * s.mask, a01 = s.w01 * s.mask, a10 = s.w10 * s.mask, a11 = s.w11 * s.mask;
            // a corner of weight zero (an integer coordinate) gets no add
            const bool s00 = s.v00 && a00 != 0.f, s01 = s.v01 && a01 != 0.f, s10 = s.v10 && a10 != 0.f, s11 = s.v11 && a11 != 0.f;
            for (int c = c0; c < g.C; c += lpi) {
                const float gv = gp[c];
                // unconditional reads at the clamped rows (in flight together), a corner outside the map replaced by zero afterwards
                float v00 = x[o00 * x_cs + x_co + c], v01 = x[o01 * x_cs + x_co + c], v10 = x[o10 * x_cs + x_co + c], v11 = x[o11 * x_cs + x_co + c];
                v00 = s.v00 ? v00 : 0.f; v01 = s.v01 ? v01 : 0.f; v10 = s.v10 ? v10 : 0.f; v11 = s.v11 ? v11 : 0.f;
                sm = fmaf(gv, s.w00 * v00 + s.w01 * v01 + s.w10 * v10 + s.w11 * v11, sm);
                sy = fmaf(gv, (1.0f - s.lx) * (v10 - v00) + s.lx * (v11 - v01), sy);
                sx = fmaf(gv, (1.0f - s.ly) * (v01 - v00) + s.ly * (v11 - v10), sx);
                if (d_x) {
                    if (s00) atomicAdd(d_x + o00 * dx_cs + dx_co + c, gv * a00);
                    if (s01) atomicAdd(d_x + o01 * dx_cs + dx_co + c, gv * a01);
                    if (s10) atomicAdd(d_x + o10 * dx_cs + dx_co + c, gv * a10);
                    if (s11) atomicAdd(d_x + o11 * dx_cs + dx_co + c, gv * a11);
                }
            }
        }
        for (int d = lpi >> 1; d > 0; d >>= 1) {
            sy += __shfl_xor(sy, d);
            sx += __shfl_xor(sx, d);
            sm += __shfl_xor(sm, d);
        }
        if (live && c0 == 0) {
            float* o = d_off + m * do_cs + do_co + 2 * t;
            o[0] = sy * s.mask;
            o[1] = sx * s.mask;
            if (d_mask) d_mask[m * dm_cs + dm_co + t] = mask_act ? sm * s.mask * (1.0f - 0.5f * s.mask) : sm;     // d(2 sigmoid(v)) / dv = mask (1 - mask / 2)
        }
    }
}

static int deform_geom(DeformGeom& g, int B, int H, int W, int C, int K, int stride, int pad, int dil) {
    if (B < 1 || H < 1 || W < 1 || K < 1 || K > 7 || stride < 1 || stride > 4 || pad < 0 || pad > 7 || dil < 1 || dil > 4) return 0;
    g.H = H; g.W = W; g.C = C; g.K = K; g.stride = stride; g.pad = pad; g.dil = dil;
    const int eh = H + 2 * pad - dil * (K - 1) - 1, ew = W + 2 * pad - dil * (K - 1) - 1;
    if (eh < 0 || ew < 0) return 0;
    g.Ho = eh / stride + 1;
    g.Wo = ew / stride + 1;
    // rows and column elements are indexed in 64 bits; the pixel decode of deform_tap and the integer coordinates need the map in 31
    return (long)B * H * W < (1l << 31) && (long)B * g.Ho * g.Wo < (1l << 31);
}

extern "C" int32_t fd_deform_im2col_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* offset, int32_t off_cs, int32_t off_co,
                                         const float* mask, int32_t mask_cs, int32_t mask_co, int32_t mask_act, float* cols, int32_t cols_cs,
                                         int32_t cols_co, int32_t B, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride, int32_t pad,
                                         int32_t dil, fd_stream_t stream) {
    DeformGeom g;
    FD_REQUIRE(deform_geom(g, B, H, W, C, K, stride, pad, dil), FD_E_INVAL,
               "fd_deform_im2col: 1 <= K <= 7, 1 <= stride <= 4, 0 <= pad <= 7, 1 <= dil <= 4 and a non-empty output expected (B=%d H=%d W=%d K=%d stride=%d pad=%d dil=%d)",
               B, H, W, K, stride, pad, dil);
    FD_REQUIRE(C > 0 && C % 4 == 0, FD_E_INVAL, "fd_deform_im2col: C %% 4 == 0 expected (C=%d)", C);
    FD_REQUIRE((long)K * K * C < (1l << 31), FD_E_INVAL, "fd_deform_im2col: K*K*C too large");
    FD_REQUIRE(view4_ok(x, x_cs, x_co, C) && view4_ok(cols, cols_cs, cols_co, K * K * C), FD_E_INVAL,
               "fd_deform_im2col: x and cols must be 4-aligned channel views (C=%d)", C);
    FD_REQUIRE(view1_ok(offset, off_cs, off_co, 2 * K * K) && (!mask || view1_ok(mask, mask_cs, mask_co, K * K)), FD_E_INVAL,
               "fd_deform_im2col: offset must be a view of 2*K*K channels, mask (optional) one of K*K");
    FD_REQUIRE(mask_act == 0 || mask_act == 1, FD_E_INVAL, "fd_deform_im2col: mask_act 0 (mask values) or 1 (logits, 2 * sigmoid) (got %d)", mask_act);
    const long items = (long)B * g.Ho * g.Wo * K * K;
    const int lpi = lanes_per_item(C / 4);
    hipLaunchKernelGGL(deform_im2col_kernel, dim3(grid_for(items, 256 / lpi)), dim3(256), 0, (hipStream_t)stream, x, x_cs, x_co, offset, off_cs, off_co,
                       mask, mask_cs, mask_co, mask_act, cols, cols_cs, cols_co, g, lpi, items);
    FD_CHECK_LAUNCH("fd_deform_im2col_nhwc");
    return FD_OK;
}

extern "C" int32_t fd_deform_bwd_nhwc(const float* dcols, int32_t dcols_cs, int32_t dcols_co, const float* x, int32_t x_cs, int32_t x_co,
                                      const float* offset, int32_t off_cs, int32_t off_co, const float* mask, int32_t mask_cs, int32_t mask_co,
                                      int32_t mask_act, float* d_offset, int32_t doff_cs, int32_t doff_co, float* d_mask, int32_t dmask_cs,
                                      int32_t dmask_co, float* d_x, int32_t dx_cs, int32_t dx_co, int32_t B, int32_t H, int32_t W, int32_t C,
                                      int32_t K, int32_t stride, int32_t pad, int32_t dil, fd_stream_t stream) {
    DeformGeom g;
    FD_REQUIRE(deform_geom(g, B, H, W, C, K, stride, pad, dil), FD_E_INVAL,
               "fd_deform_bwd: 1 <= K <= 7, 1 <= stride <= 4, 0 <= pad <= 7, 1 <= dil <= 4 and a non-empty output expected (B=%d H=%d W=%d K=%d stride=%d pad=%d dil=%d)",
               B, H, W, K, stride, pad, dil);
    FD_REQUIRE(C > 0 && C % 4 == 0, FD_E_INVAL, "fd_deform_bwd: C %% 4 == 0 expected (C=%d)", C);
    FD_REQUIRE((long)K * K * C < (1l << 31), FD_E_INVAL, "fd_deform_bwd: K*K*C too large");
    FD_REQUIRE(view4_ok(x, x_cs, x_co, C) && view4_ok(dcols, dcols_cs, dcols_co, K * K * C) && (!d_x || view4_ok(d_x, dx_cs, dx_co, C)), FD_E_INVAL,
               "fd_deform_bwd: x, dcols and d_x (optional) must be 4-aligned channel views (C=%d)", C);
    FD_REQUIRE(view1_ok(offset, off_cs, off_co, 2 * K * K) && view1_ok(d_offset, doff_cs, doff_co, 2 * K * K), FD_E_INVAL,
               "fd_deform_bwd: offset and d_offset must be views of 2*K*K channels");
    FD_REQUIRE((mask == nullptr) == (d_mask == nullptr) && (!mask || (view1_ok(mask, mask_cs, mask_co, K * K) && view1_ok(d_mask, dmask_cs, dmask_co, K * K))),
               FD_E_INVAL, "fd_deform_bwd: mask and d_mask come together, each a view of K*K channels");
    FD_REQUIRE(mask_act == 0 || mask_act == 1, FD_E_INVAL, "fd_deform_bwd: mask_act 0 (mask values) or 1 (logits, 2 * sigmoid) (got %d)", mask_act);
    const long items = (long)B * g.Ho * g.Wo * K * K;
    const int lpi = lanes_per_item(C);
    hipLaunchKernelGGL(deform_bwd_kernel, dim3(grid_for(items, 256 / lpi)), dim3(256), 0, (hipStream_t)stream, dcols, dcols_cs, dcols_co, x, x_cs, x_co,
                       offset, off_cs, off_co, mask, mask_cs, mask_co, mask_act, d_offset, doff_cs, doff_co, d_mask, dmask_cs, dmask_co, d_x, dx_cs, dx_co,
                       g, lpi, items);
    FD_CHECK_LAUNCH("fd_deform_bwd_nhwc");
    return FD_OK;
}
