// fd_resize.hip — the input pipeline's resize on the device (gfx950): the cv2.resize call of the reference's
// preprocess_img_boxes (dataset/voc.py:110-139, Test_coco.py:76-105) and the box scaling that goes with it
// (voc.py:137-138 boxes * scale, Test_coco.py:147-151 boxes / scale).
//   * bilinear resize of raw uint8 [h][w][3] images with half-pixel geometry and 11-bit integer blending,
//     alone (-> uint8) or fused with pad-to-canvas + ToTensor + Normalize for a whole mixed-size batch (-> the stem's
//     fp32 [N][H][W][4] input) in one launch;
//   * per-image scaling of padded detections / ground-truth boxes.
// The arithmetic is this project's own definition, UNPINNED AGAINST cv2 (cv2 is third-party and absent): it uses the
// geometry of cv2.INTER_LINEAR / torch bilinear (align_corners=False), no antialiasing.  Compiled with -ffp-contract=off:
// the coordinate arithmetic is plain fp32 (one rounding per operation), tests/resize_ref.py restates it in numpy bit for bit.
// Write-dominated and HBM-bound: one lane per output pixel, one 16-byte store, four cache-resident taps.
#include "fd_resize_taps.h"      // resize_axis: the tap arithmetic, shared with fd_augment.hip

// One output pixel (dy, dx) of the h x w -> nh x nw resize: three integer levels 0..255.
__device__ __forceinline__ void resize_pixel(const unsigned char* __restrict__ src, int h, int w, int nh, int nw, int dy, int dx,
                                             unsigned& r, unsigned& g, unsigned& b) {
    int y0, y1, x0, x1;
    unsigned cy0, cy1, cx0, cx1;
    resize_axis(dy, h, nh, y0, y1, cy0, cy1);
    resize_axis(dx, w, nw, x0, x1, cx0, cx1);
    const unsigned char* p00 = src + ((long)y0 * w + x0) * 3;
    const unsigned char* p01 = src + ((long)y0 * w + x1) * 3;
    const unsigned char* p10 = src + ((long)y1 * w + x0) * 3;
    const unsigned char* p11 = src + ((long)y1 * w + x1) * 3;
    const unsigned w00 = cx0 * cy0, w01 = cx1 * cy0, w10 = cx0 * cy1, w11 = cx1 * cy1;     // sum = 2^22
    constexpr unsigned half = 1u << (2 * FD_RESIZE_COEF_BITS - 1);
    r = (p00[0] * w00 + p01[0] * w01 + p10[0] * w10 + p11[0] * w11 + half) >> (2 * FD_RESIZE_COEF_BITS);
    g = (p00[1] * w00 + p01[1] * w01 + p10[1] * w10 + p11[1] * w11 + half) >> (2 * FD_RESIZE_COEF_BITS);
    b = (p00[2] * w00 + p01[2] * w01 + p10[2] * w10 + p11[2] * w11 + half) >> (2 * FD_RESIZE_COEF_BITS);
}

// ------------------------------------------------------------------------------ one image -> uint8 (the cv2.resize drop-in)
__global__ __launch_bounds__(256) void resize_u8_kernel(const unsigned char* __restrict__ x, int h, int w, unsigned char* __restrict__ y,
                                                         int nh, int nw) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)nh * (unsigned)nw) return;
    const unsigned dy = i / (unsigned)nw, dx = i - dy * (unsigned)nw;
    unsigned r, g, b;
    resize_pixel(x, h, w, nh, nw, (int)dy, (int)dx, r, g, b);
    unsigned char* o = y + (long)i * 3;
    o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)b;
}

extern "C" int32_t fd_resize_u8(const uint8_t* x, int32_t h, int32_t w, uint8_t* y, int32_t nh, int32_t nw, fd_stream_t stream) {
    FD_REQUIRE(x && y, FD_E_INVAL, "fd_resize_u8: null pointer");
    FD_REQUIRE(h >= 1 && w >= 1 && nh >= 1 && nw >= 1 && h <= FD_RESIZE_MAX_SIDE && w <= FD_RESIZE_MAX_SIDE && nh <= FD_RESIZE_MAX_SIDE &&
               nw <= FD_RESIZE_MAX_SIDE, FD_E_INVAL, "fd_resize_u8: sizes must be in 1 .. %d (got %d x %d -> %d x %d)", FD_RESIZE_MAX_SIDE, h, w, nh, nw);
    FD_REQUIRE((long)nh * nw < (1l << 31), FD_E_INVAL, "fd_resize_u8: more than 2^31 output pixels");
    const long total = (long)nh * nw;
    hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, h, w, y, nh, nw);
    FD_CHECK_LAUNCH("fd_resize_u8");
    return FD_OK;
}

// ------------------------------------------------------------------------------ mixed-size batch: resize + pad + normalise
// One launch per batch, image index in blockIdx.z: `src` is a device array of N pointers to the RAW uint8 [h_n][w_n][3]
// images, src_hw / dst_hw device int32 [N][2] = (h_n, w_n) / (nh_n, nw_n).  Canvas pixels outside nh_n x nw_n are uint8 zero
// BEFORE Normalize, channel 3 = 0, the normalisation is collate_u8_kernel's expression (fd_mbconv.hip) on the integer level.
// The tables live in device memory, so the host cannot see them: an entry with a side < 1 makes its image all padding, and
// only canvas pixels are ever written (a destination larger than the canvas is cut, never written past it).
__global__ __launch_bounds__(256) void resize_collate_u8_kernel(const unsigned char* const* __restrict__ src, const int* __restrict__ src_hw,
                                                                 const int* __restrict__ dst_hw, float4* __restrict__ y, int H, int W,
                                                                 float m0, float m1, float m2, float s0, float s1, float s2) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)H * (unsigned)W) return;
    const int n = blockIdx.z;
    const unsigned dy = i / (unsigned)W, dx = i - dy * (unsigned)W;
    const int h = src_hw[2 * n], w = src_hw[2 * n + 1], nh = dst_hw[2 * n], nw = dst_hw[2 * n + 1];
    unsigned r = 0, g = 0, b = 0;
    if ((int)dy < nh && (int)dx < nw && h >= 1 && w >= 1) resize_pixel(src[n], h, w, nh, nw, (int)dy, (int)dx, r, g, b);
    y[(long)n * H * W + i] = make_float4(((float)r / 255.0f - m0) / s0, ((float)g / 255.0f - m1) / s1, ((float)b / 255.0f - m2) / s2, 0.f);
}

extern "C" int32_t fd_resize_collate_u8_nhwc4(const uint8_t* const* images_dev, const int32_t* src_hw_dev, const int32_t* dst_hw_dev, float* y,
                                              int32_t N, int32_t H, int32_t W, const float* mean3, const float* std3, fd_stream_t stream) {
    FD_REQUIRE(images_dev && src_hw_dev && dst_hw_dev && y && mean3 && std3, FD_E_INVAL, "fd_resize_collate_u8: null pointer");
    FD_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= FD_RESIZE_MAX_SIDE && W <= FD_RESIZE_MAX_SIDE && (long)H * W < (1l << 31), FD_E_INVAL,
               "fd_resize_collate_u8: bad batch %d or canvas %d x %d", N, H, W);
    FD_REQUIRE(((uintptr_t)y & 15) == 0, FD_E_INVAL, "fd_resize_collate_u8: y not 16-byte aligned");
    FD_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, FD_E_INVAL, "fd_resize_collate_u8: zero std");
    const long per = (long)H * W;
    hipLaunchKernelGGL(resize_collate_u8_kernel, dim3((unsigned)((per + 255) / 256), 1, (unsigned)N), dim3(256), 0, (hipStream_t)stream, images_dev,
                       src_hw_dev, dst_hw_dev, (float4*)y, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    FD_CHECK_LAUNCH("fd_resize_collate_u8_nhwc4");
    return FD_OK;
}

// ------------------------------------------------------------------------------ boxes between resized and source coordinates
// In place on padded [B][K][4]: image b uses scales[b] (device fp32).  invert: IEEE fp32 division, as boxes_to_xywh_kernel
// (fd_layers.hip) and numpy's boxes /= scale; else the fp32 product of voc.py:137-138.  Rows >= counts[b] are not touched.
__global__ __launch_bounds__(256) void boxes_scale_batch_kernel(float4* boxes, const int* __restrict__ counts, const float* __restrict__ scales,
                                                                 long total, int K, int invert, int xywh) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int k;
    const int bi = (int)fd_div(i, K, k);
    if (counts && k >= counts[bi]) return;
    const float s = scales[bi];
    float4 b = boxes[i];
    if (invert) { b.x = b.x / s; b.y = b.y / s; b.z = b.z / s; b.w = b.w / s; }
    else { b.x = b.x * s; b.y = b.y * s; b.z = b.z * s; b.w = b.w * s; }
    if (xywh) { b.z = b.z - b.x; b.w = b.w - b.y; }
    boxes[i] = b;
}

extern "C" int32_t fd_boxes_scale_batch(float* boxes, const int32_t* counts, const float* scales_dev, int32_t B, int32_t K, int32_t invert,
                                        int32_t xywh, fd_stream_t stream) {
    FD_REQUIRE(boxes && ((uintptr_t)boxes & 15) == 0 && scales_dev && B >= 0 && K >= 0, FD_E_INVAL, "fd_boxes_scale_batch: bad argument");
    const long total = (long)B * K;
    if (total == 0) return FD_OK;
    hipLaunchKernelGGL(boxes_scale_batch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (float4*)boxes, counts,
                       scales_dev, total, K, invert != 0, xywh != 0);
    FD_CHECK_LAUNCH("fd_boxes_scale_batch");
    return FD_OK;
}
