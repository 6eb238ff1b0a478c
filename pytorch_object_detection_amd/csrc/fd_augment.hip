// fd_augment.hip — the training-side augmentations on the device (gfx950): the reference's flip (dataset/voc.py:12-20),
// Transforms (data/augment.py: colorJitter, random_rotation, random_crop_resize), preprocess_img_boxes and collate_fn for a
// whole batch of RAW uint8 images in one launch.  The random decisions and the box arithmetic stay on the
// host (data/augment.py of this package); the device receives one parameter record per image (FD_AUG_* in fcosdet.h).
//   * Every pixel step before the resize is pointwise (colour) or a nearest-neighbour gather (crop, rotation, flip), so it
//     is folded into the four taps of the bilinear resize: tap in crop space -> + crop origin -> PIL's 16.16 fixed-point
//     inverse rotation (black outside) -> mirrored column -> three raw bytes -> colour chain -> blend -> Normalize.
//   * Colour: PIL's ImageEnhance Brightness / Contrast / Color, clip(trunc(deg + f * (pix - deg))) in fp32, and the HSV hue
//     shift; exact against PIL (tests/augment_ref.py restates all of it in numpy).  Compiled with -ffp-contract=off.
//   * Contrast needs int(mean(L) + 0.5) of the image at that point of the chain: fd_jitter_l_sums reduces it in integers.
//   * Mosaic: fd_mosaic_collate_u8 tiles four such images around a centre per output; per canvas pixel it picks
//     the tile, then runs the same per-pixel function (aug_pixel) as the fused launch.
// Whatever a record holds, a tap is read only after its final (row, column) has been checked against [h][w], and only
// canvas pixels are written.
#include "fd_resize_taps.h"

#define AUG_MAX_ROT_SIDE 16384

__device__ __forceinline__ unsigned aug_luma(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

__device__ __forceinline__ unsigned aug_blend1(float deg, unsigned pix, float f) {
    const float v = deg + f * ((float)pix - deg);        // pix, deg integers <= 255: the difference is exact
    return (unsigned)min(max((int)v, 0), 255);           // (int): truncation toward zero, as PIL's cast
}

__device__ __forceinline__ unsigned aug_round8(float v) { return (unsigned)min(max((int)floorf(v + 0.5f), 0), 255); }

// RGB -> HSV, H += shift (mod 256), HSV -> RGB: PIL's conversions.  The hue sums with the constants 2.0 / 4.0 / 6.0 / 1.0 / 255.0
// are fp64 there (C double literals), the ratios fp32.
__device__ __forceinline__ void aug_hue(unsigned& r, unsigned& g, unsigned& b, unsigned shift) {
    const unsigned maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    unsigned uh = 0, us = 0;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        double hd = (double)h / 6.0 + 1.0;               // in (0, 2): fmod(hd, 1.0) is hd or hd - 1.0, both exact
        if (hd >= 1.0) hd -= 1.0;
        h = (float)hd;
        uh = (unsigned)min(max((int)((double)h * 255.0), 0), 255);
        us = (unsigned)min(max((int)((double)s * 255.0), 0), 255);
    }
    uh = (uh + shift) & 255u;
    if (us == 0) { r = g = b = maxc; return; }
    const float v = (float)maxc;
    const float x = (float)uh * 6.0f / 255.0f;
    const float fi = floorf(x);
    const float f = x - fi;
    const float fs = (float)us / 255.0f;
    const unsigned p = aug_round8(v * (1.0f - fs));
    const unsigned q = aug_round8(v * (1.0f - fs * f));
    const unsigned t = aug_round8(v * (1.0f - fs * (1.0f - f)));
    const int i = (int)fi % 6;
    r = (i == 0 || i == 5) ? maxc : (i == 1) ? q : (i == 4) ? t : p;
    g = (i == 1 || i == 2) ? maxc : (i == 0) ? t : (i == 3) ? q : p;
    b = (i == 3 || i == 4) ? maxc : (i == 2) ? t : (i == 5) ? q : p;
}

// Operations [0, stop) of the record's chain on one pixel; each rounds to uint8, as PIL does between operations.
__device__ __forceinline__ void aug_chain(const int* __restrict__ rec, int stop, unsigned& r, unsigned& g, unsigned& b) {
#pragma unroll 1
    for (int k = 0; k < stop; ++k) {
        const int op = rec[FD_AUG_OP0 + k], arg = rec[FD_AUG_ARG0 + k];
        if (op == FD_AUG_OP_HUE) { aug_hue(r, g, b, (unsigned)arg & 255u); continue; }
        if (op != FD_AUG_OP_BRIGHTNESS && op != FD_AUG_OP_CONTRAST && op != FD_AUG_OP_SATURATION) continue;
        const float f = __int_as_float(arg);
        const float deg = op == FD_AUG_OP_BRIGHTNESS ? 0.f : op == FD_AUG_OP_CONTRAST ? (float)(rec[FD_AUG_MEAN_L] & 255) : (float)aug_luma(r, g, b);
        r = aug_blend1(deg, r, f); g = aug_blend1(deg, g, f); b = aug_blend1(deg, b, f);
    }
}

__device__ __forceinline__ int aug_chain_len(const int* __restrict__ rec) { return min(max(rec[FD_AUG_NOPS], 0), FD_AUG_MAX_OPS); }

// The pixel of the rotated image at (y, x): PIL's affine_fixed.  Sides <= 16384 and |d| < 90 keep every |coordinate| below
// 19 778 * 65536 < 2^31 (centre-relative: (w/2) * (1 + |cos| + |sin|)); the sums are formed in 64 bits, so no record can overflow them.
__device__ __forceinline__ void aug_rot_map(const int* __restrict__ fx, int y, int x, int& sy, int& sx) {
    const long xx = (long)fx[2] + (long)fx[0] * x + (long)fx[1] * y;
    const long yy = (long)fx[5] + (long)fx[3] * x + (long)fx[4] * y;
    const long qx = xx >> 16, qy = yy >> 16;
    sx = (qx < -1 || qx > 0x7fffffff) ? -1 : (int)qx;
    sy = (qy < -1 || qy > 0x7fffffff) ? -1 : (int)qy;
}

// One resized pixel (ly, lx) of the record's NH x NW image: the four taps of the CROP_H x CROP_W -> NH x NW resize, each through
// crop offset -> rotation map -> mirrored column -> raw bytes -> colour chain, blended.  The caller has checked 0 <= ly < nh,
// 0 <= lx < nw and h, w, cw, ch >= 1.  Shared by the fused launch and the mosaic launch so that there is one definition.
__device__ __forceinline__ void aug_pixel(const int* __restrict__ rec, const unsigned char* __restrict__ img, int ly, int lx, int h, int w, int nh, int nw,
                                          int cw, int ch, unsigned& r, unsigned& g, unsigned& b) {
    const int cx = rec[FD_AUG_CROP_X], cy = rec[FD_AUG_CROP_Y], flip = rec[FD_AUG_FLIP], rot = rec[FD_AUG_ROT_ON];
    const int nops = aug_chain_len(rec);
    int y0, y1, x0, x1;
    unsigned cy0, cy1, cx0, cx1;
    resize_axis(ly, ch, nh, y0, y1, cy0, cy1);
    resize_axis(lx, cw, nw, x0, x1, cx0, cx1);
    unsigned ar = 0, ag = 0, ab = 0;
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
        int sy = ((t & 2) ? y1 : y0) + cy, sx = ((t & 1) ? x1 : x0) + cx;
        const unsigned wt = ((t & 2) ? cy1 : cy0) * ((t & 1) ? cx1 : cx0);
        if (rot) {
            const bool in_rot = (unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w;
            aug_rot_map(rec + FD_AUG_ROT0, sy, sx, sy, sx);
            if (!in_rot) sy = -1;
        }
        if (flip) sx = w - 1 - sx;
        unsigned pr = 0, pg = 0, pb = 0;
        if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {      // the only gate in front of the loads
            const unsigned char* p = img + ((long)sy * w + sx) * 3;
            pr = p[0]; pg = p[1]; pb = p[2];
            aug_chain(rec, nops, pr, pg, pb);
        }
        ar += pr * wt; ag += pg * wt; ab += pb * wt;
    }
    constexpr unsigned half = 1u << (2 * FD_RESIZE_COEF_BITS - 1);
    r = (ar + half) >> (2 * FD_RESIZE_COEF_BITS);
    g = (ag + half) >> (2 * FD_RESIZE_COEF_BITS);
    b = (ab + half) >> (2 * FD_RESIZE_COEF_BITS);
}

// ------------------------------------------------------------------------------ the fused launch
__global__ __launch_bounds__(256) void augment_resize_collate_u8_kernel(const unsigned char* const* __restrict__ src, const int* __restrict__ recs,
                                                                         float* __restrict__ y, int H, int W, float m0, float m1, float m2,
                                                                         float s0, float s1, float s2) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)H * (unsigned)W) return;
    const int n = blockIdx.z;
    const int* __restrict__ rec = recs + (long)n * FD_AUG_WORDS;
    const unsigned dy = i / (unsigned)W, dx = i - dy * (unsigned)W;
    const int h = rec[FD_AUG_H], w = rec[FD_AUG_W], nh = rec[FD_AUG_NH], nw = rec[FD_AUG_NW];
    const int cw = rec[FD_AUG_CROP_W], ch = rec[FD_AUG_CROP_H];
    unsigned r = 0, g = 0, b = 0;
    if ((int)dy < nh && (int)dx < nw && h >= 1 && w >= 1 && cw >= 1 && ch >= 1) aug_pixel(rec, src[n], (int)dy, (int)dx, h, w, nh, nw, cw, ch, r, g, b);
    const long per = (long)H * W;
    float* o = y + (long)n * 3 * per + i;
    o[0] = ((float)r / 255.0f - m0) / s0;
    o[per] = ((float)g / 255.0f - m1) / s1;
    o[2 * per] = ((float)b / 255.0f - m2) / s2;
}

extern "C" int32_t fd_augment_resize_collate_u8(const uint8_t* const* images_dev, const int32_t* recs_dev, float* y, int32_t N, int32_t H, int32_t W,
                                                const float* mean3, const float* std3, fd_stream_t stream) {
    FD_REQUIRE(images_dev && recs_dev && y && mean3 && std3, FD_E_INVAL, "fd_augment_resize_collate_u8: null pointer");
    FD_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= FD_RESIZE_MAX_SIDE && W <= FD_RESIZE_MAX_SIDE && (long)H * W < (1l << 31), FD_E_INVAL,
               "fd_augment_resize_collate_u8: bad batch %d or canvas %d x %d", N, H, W);
    FD_REQUIRE(((uintptr_t)y & 3) == 0 && ((uintptr_t)recs_dev & 3) == 0, FD_E_INVAL, "fd_augment_resize_collate_u8: y / records not 4-byte aligned");
    FD_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, FD_E_INVAL, "fd_augment_resize_collate_u8: zero std");
    const long per = (long)H * W;
    hipLaunchKernelGGL(augment_resize_collate_u8_kernel, dim3((unsigned)((per + 255) / 256), 1, (unsigned)N), dim3(256), 0, (hipStream_t)stream,
                       images_dev, recs_dev, y, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    FD_CHECK_LAUNCH("fd_augment_resize_collate_u8");
    return FD_OK;
}

// ------------------------------------------------------------------------------ the mosaic launch
// Four sources per output: canvas pixel (dy, dx) of output n belongs to tile t = 2 * (dy >= YC) + (dx >= XC) and is pixel
// (dy - PYt, dx - PXt) of the NH x NW image of record 4n + t, or the FILL level when that lies outside it (or the record's sizes
// are not positive).  XC, YC, PX, PY are only compared and subtracted in 64 bits: any 32-bit value is safe.  The record is chosen
// per lane, so its words come through vector loads here; everything behind the choice is aug_pixel, the fused launch's arithmetic.
__global__ __launch_bounds__(256) void mosaic_collate_u8_kernel(const unsigned char* const* __restrict__ src, const int* __restrict__ recs,
                                                                 const int* __restrict__ place, float* __restrict__ y, int H, int W, float m0, float m1,
                                                                 float m2, float s0, float s1, float s2) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)H * (unsigned)W) return;
    const int n = blockIdx.z;
    const int* __restrict__ pl = place + (long)n * FD_MOSAIC_WORDS;
    const unsigned dy = i / (unsigned)W, dx = i - dy * (unsigned)W;
    const int t = ((int)dy >= pl[FD_MOSAIC_YC] ? 2 : 0) + ((int)dx >= pl[FD_MOSAIC_XC] ? 1 : 0);
    const long slot = (long)n * 4 + t;
    const int* __restrict__ rec = recs + slot * FD_AUG_WORDS;
    const long ly = (long)dy - (long)pl[FD_MOSAIC_PX0 + 2 * t + 1], lx = (long)dx - (long)pl[FD_MOSAIC_PX0 + 2 * t];
    const int h = rec[FD_AUG_H], w = rec[FD_AUG_W], nh = rec[FD_AUG_NH], nw = rec[FD_AUG_NW];
    const int cw = rec[FD_AUG_CROP_W], ch = rec[FD_AUG_CROP_H];
    const unsigned fill = (unsigned)pl[FD_MOSAIC_FILL];
    unsigned r = fill & 255u, g = (fill >> 8) & 255u, b = (fill >> 16) & 255u;
    if (ly >= 0 && ly < (long)nh && lx >= 0 && lx < (long)nw && h >= 1 && w >= 1 && cw >= 1 && ch >= 1)
        aug_pixel(rec, src[slot], (int)ly, (int)lx, h, w, nh, nw, cw, ch, r, g, b);
    const long per = (long)H * W;
    float* o = y + (long)n * 3 * per + i;
    o[0] = ((float)r / 255.0f - m0) / s0;
    o[per] = ((float)g / 255.0f - m1) / s1;
    o[2 * per] = ((float)b / 255.0f - m2) / s2;
}

extern "C" int32_t fd_mosaic_collate_u8(const uint8_t* const* images_dev, const int32_t* recs_dev, const int32_t* place_dev, float* y, int32_t N, int32_t H,
                                        int32_t W, const float* mean3, const float* std3, fd_stream_t stream) {
    FD_REQUIRE(images_dev && recs_dev && place_dev && y && mean3 && std3, FD_E_INVAL, "fd_mosaic_collate_u8: null pointer");
    FD_REQUIRE(N >= 1 && N <= FD_MOSAIC_MAX_N && H >= 1 && W >= 1 && H <= FD_RESIZE_MAX_SIDE && W <= FD_RESIZE_MAX_SIDE && (long)H * W < (1l << 31), FD_E_INVAL,
               "fd_mosaic_collate_u8: bad batch %d or canvas %d x %d", N, H, W);
    FD_REQUIRE(((uintptr_t)y & 3) == 0 && ((uintptr_t)recs_dev & 3) == 0 && ((uintptr_t)place_dev & 3) == 0 && ((uintptr_t)images_dev & 7) == 0, FD_E_INVAL,
               "fd_mosaic_collate_u8: y / records / placements not 4-byte or pointers not 8-byte aligned");
    FD_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, FD_E_INVAL, "fd_mosaic_collate_u8: zero std");
    const long per = (long)H * W;
    hipLaunchKernelGGL(mosaic_collate_u8_kernel, dim3((unsigned)((per + 255) / 256), 1, (unsigned)N), dim3(256), 0, (hipStream_t)stream, images_dev,
                       recs_dev, place_dev, y, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    FD_CHECK_LAUNCH("fd_mosaic_collate_u8");
    return FD_OK;
}

// ------------------------------------------------------------------------------ sum of L in front of the contrast operation
// Images whose chain holds contrast: sum over the RAW image of L after the operations that precede contrast (flip, rotation
// and crop come later in the reference's order and do not enter).  Integer sums: exact and order-independent.  Each lane
// strides over the pixels of its image, a wave reduces by shuffles, the four waves meet in LDS, lane 0 issues ONE 64-bit
// vector atomic add on HBM per workgroup.
#define AUG_SUM_BLOCKS_MAX 256

__device__ __forceinline__ int aug_contrast_at(const int* __restrict__ rec) {
    const int n = aug_chain_len(rec);
    for (int k = 0; k < n; ++k)
        if (rec[FD_AUG_OP0 + k] == FD_AUG_OP_CONTRAST) return k;
    return -1;
}

__global__ __launch_bounds__(256) void jitter_l_sums_kernel(const unsigned char* const* __restrict__ src, const int* __restrict__ recs,
                                                             unsigned long long* __restrict__ sums) {
    const int n = blockIdx.z;
    const int* __restrict__ rec = recs + (long)n * FD_AUG_WORDS;
    const int at = aug_contrast_at(rec);
    const int h = rec[FD_AUG_H], w = rec[FD_AUG_W];
    if (at < 0 || h < 1 || w < 1) return;                 // uniform over the workgroup
    const unsigned long total = (unsigned long)h * (unsigned long)w;
    const unsigned char* __restrict__ img = src[n];
    unsigned long long acc = 0;
    for (unsigned long i = (unsigned long)blockIdx.x * 256u + threadIdx.x; i < total; i += (unsigned long)gridDim.x * 256u) {
        const unsigned char* p = img + i * 3;
        unsigned r = p[0], g = p[1], b = p[2];
        aug_chain(rec, at, r, g, b);
        acc += aug_luma(r, g, b);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + n, part[0] + part[1] + part[2] + part[3]);
}

// One lane per image: int(sum / (h * w) + 0.5) in doubles, PIL's ImageStat mean, into the record's FD_AUG_MEAN_L word.
__global__ void jitter_l_mean_kernel(int* __restrict__ recs, const unsigned long long* __restrict__ sums, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int* rec = recs + (long)n * FD_AUG_WORDS;
    const int h = rec[FD_AUG_H], w = rec[FD_AUG_W];
    if (aug_contrast_at(rec) < 0 || h < 1 || w < 1) return;
    const double mean = (double)sums[n] / (double)((long)h * (long)w);
    rec[FD_AUG_MEAN_L] = (int)(mean + 0.5);
}

extern "C" int32_t fd_jitter_l_sums(const uint8_t* const* images_dev, int32_t* recs_dev, uint64_t* sums_dev, int32_t N, int64_t max_pixels,
                                    fd_stream_t stream) {
    FD_REQUIRE(images_dev && recs_dev && sums_dev, FD_E_INVAL, "fd_jitter_l_sums: null pointer");
    FD_REQUIRE(N >= 1 && N <= 65535 && max_pixels >= 1 && max_pixels <= (int64_t)FD_RESIZE_MAX_SIDE * FD_RESIZE_MAX_SIDE, FD_E_INVAL,
               "fd_jitter_l_sums: bad batch %d or pixel count %lld", N, (long long)max_pixels);
    FD_REQUIRE(((uintptr_t)sums_dev & 7) == 0 && ((uintptr_t)recs_dev & 3) == 0, FD_E_INVAL, "fd_jitter_l_sums: sums not 8-byte / records not 4-byte aligned");
    if (hipMemsetAsync(sums_dev, 0, sizeof(uint64_t) * (size_t)N, (hipStream_t)stream) != hipSuccess) {
        fd_set_error("fd_jitter_l_sums: clearing the sums failed");
        return FD_E_LAUNCH;
    }
    // ~8 pixels per lane, capped: 256 workgroups per image already cover the device for a batch
    long blocks = (max_pixels + 2047) / 2048;
    if (blocks > AUG_SUM_BLOCKS_MAX) blocks = AUG_SUM_BLOCKS_MAX;
    hipLaunchKernelGGL(jitter_l_sums_kernel, dim3((unsigned)blocks, 1, (unsigned)N), dim3(256), 0, (hipStream_t)stream, images_dev, recs_dev,
                       (unsigned long long*)sums_dev);
    FD_CHECK_LAUNCH("fd_jitter_l_sums");
    hipLaunchKernelGGL(jitter_l_mean_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, recs_dev,
                       (const unsigned long long*)sums_dev, N);
    FD_CHECK_LAUNCH("fd_jitter_l_sums (mean)");
    return FD_OK;
}

// ------------------------------------------------------------------------------ single steps: one image -> uint8
__global__ __launch_bounds__(256) void color_jitter_u8_kernel(const unsigned char* __restrict__ x, const int* __restrict__ rec, unsigned char* __restrict__ y,
                                                               long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    unsigned r = x[i * 3], g = x[i * 3 + 1], b = x[i * 3 + 2];
    aug_chain(rec, aug_chain_len(rec), r, g, b);
    y[i * 3] = (unsigned char)r; y[i * 3 + 1] = (unsigned char)g; y[i * 3 + 2] = (unsigned char)b;
}

extern "C" int32_t fd_color_jitter_u8(const uint8_t* x, int32_t h, int32_t w, uint8_t* y, const int32_t* rec_dev, fd_stream_t stream) {
    FD_REQUIRE(x && y && rec_dev, FD_E_INVAL, "fd_color_jitter_u8: null pointer");
    FD_REQUIRE(h >= 1 && w >= 1 && h <= FD_RESIZE_MAX_SIDE && w <= FD_RESIZE_MAX_SIDE, FD_E_INVAL, "fd_color_jitter_u8: sides must be in 1 .. %d (got %d x %d)",
               FD_RESIZE_MAX_SIDE, h, w);
    const long total = (long)h * w;
    hipLaunchKernelGGL(color_jitter_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, rec_dev, y, total);
    FD_CHECK_LAUNCH("fd_color_jitter_u8");
    return FD_OK;
}

struct aug_rot6 { int v[6]; };

__global__ __launch_bounds__(256) void rotate_u8_kernel(const unsigned char* __restrict__ x, int h, int w, unsigned char* __restrict__ y, aug_rot6 fx) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)h * (unsigned)w) return;
    const int dy = (int)(i / (unsigned)w), dx = (int)(i - (unsigned)dy * (unsigned)w);
    int sy, sx;
    aug_rot_map(fx.v, dy, dx, sy, sx);
    unsigned r = 0, g = 0, b = 0;
    if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
        const unsigned char* p = x + ((long)sy * w + sx) * 3;
        r = p[0]; g = p[1]; b = p[2];
    }
    unsigned char* o = y + (long)i * 3;
    o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)b;
}

extern "C" int32_t fd_rotate_u8(const uint8_t* x, int32_t h, int32_t w, uint8_t* y, const int32_t* fixed6, fd_stream_t stream) {
    FD_REQUIRE(x && y && fixed6, FD_E_INVAL, "fd_rotate_u8: null pointer");
    FD_REQUIRE(h >= 1 && w >= 1 && h <= AUG_MAX_ROT_SIDE && w <= AUG_MAX_ROT_SIDE, FD_E_INVAL, "fd_rotate_u8: sides must be in 1 .. %d (got %d x %d)",
               AUG_MAX_ROT_SIDE, h, w);
    FD_REQUIRE(x != y, FD_E_INVAL, "fd_rotate_u8: in-place rotation is not supported");
    aug_rot6 fx;
    for (int k = 0; k < 6; ++k) fx.v[k] = fixed6[k];
    const long total = (long)h * w;
    hipLaunchKernelGGL(rotate_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, h, w, y, fx);
    FD_CHECK_LAUNCH("fd_rotate_u8");
    return FD_OK;
}
