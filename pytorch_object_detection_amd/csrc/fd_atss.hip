// fd_atss.hip — ATSS target assignment (Adaptive Training Sample Selection, Zhang et al., CVPR 2020) beside
// fd_fcos_gen_targets (fd_loss.hip): same level table, same location order, same three outputs.  DESIGN 4.3o states the
// definition; tests/atss_ref.py restates it in numpy.  Built with -ffp-contract=off: every fp32 / fp64 operation rounds once.
//
//   memset(workspace)                        one 64-bit claim word per (image, location), 0 = unclaimed
//   atss_select_kernel   grid (M, B)         per ground-truth row: per-level top-k by (d2, pix), IoU, fp64 mean + std,
//                                            positives published with a 64-bit atomicMax (iou bits : ~row)
//   atss_output_kernel   grid (L / 256, B)   per location: claim word -> cls / cnt / reg, as gen_targets_kernel writes them
#include "fd_common.h"
#include <math.h>

#define ATSS_THREADS 256
#define ATSS_WAVES (ATSS_THREADS / 64)
#define ATSS_MAX_CAND (FD_MAX_SEG * FD_ATSS_MAX_TOPK)

struct AtssArgs {
    const float* gt; const long long* labels;
    int B, M, L, nseg, topk;
    int H[FD_MAX_SEG], W[FD_MAX_SEG], stride[FD_MAX_SEG], loc_start[FD_MAX_SEG + 1];
    float anchor_scale, inside_eps;
    unsigned long long* claim;      // [B][L]
    double* gt_thr; int* gt_npos;   // [B][M], optional
    long long* cls_t; float* cnt_t; float* reg_t;
};

// centre of location (px, py) of a level with stride st: the expression of gen_targets_kernel
__device__ __forceinline__ float atss_centre(int p, int st) { return (float)(p * st) + (float)(st / 2); }

__device__ __forceinline__ unsigned long long atss_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(ATSS_THREADS) void atss_select_kernel(AtssArgs a) {
    __shared__ unsigned long long s_red[2][ATSS_WAVES];
    __shared__ int s_pix[ATSS_MAX_CAND];
    __shared__ int s_lvl[ATSS_MAX_CAND];
    __shared__ float s_iou[ATSS_MAX_CAND];
    __shared__ double s_thr;
    __shared__ int s_npos;
    const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long row = (long)b * a.M + m;
    const float4 g = reinterpret_cast<const float4*>(a.gt)[row];
    const bool valid = a.labels[row] >= 0 && isfinite(g.x) && isfinite(g.y) && isfinite(g.z) && isfinite(g.w) && g.z > g.x && g.w > g.y;
    if (!valid) {                                        // uniform over the workgroup: padding takes no part
        if (tid == 0) {
            if (a.gt_thr) a.gt_thr[row] = __builtin_nan("");
            if (a.gt_npos) a.gt_npos[row] = 0;
        }
        return;
    }
    const float gx = (g.x + g.z) / 2.0f, gy = (g.y + g.w) / 2.0f;

    // 1. candidates: per level k_l rounds of arg-min over (d2, pix); round r takes the smallest key above round r-1's, so
    //    nothing has to be marked as taken.  d2 >= +0 (or +inf), so its bits order as the floats do.
    int n = 0, parity = 0;
    for (int s = 0; s < a.nseg; ++s) {
        const int W = a.W[s], HW = a.H[s] * W, st = a.stride[s];
        const int k = a.topk < HW ? a.topk : HW;
        unsigned long long prev = 0ull;
        for (int r = 0; r < k; ++r) {
            unsigned long long best = ~0ull;
            for (int pix = tid; pix < HW; pix += ATSS_THREADS) {
                const int py = (int)((unsigned)pix / (unsigned)W), px = pix - py * W;
                const float dx = atss_centre(px, st) - gx, dy = atss_centre(py, st) - gy;
                const float d2 = dx * dx + dy * dy;
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)pix;
                if ((r == 0 || key > prev) && key < best) best = key;
            }
            best = atss_wave_min(best);
            if ((tid & 63) == 0) s_red[parity][tid >> 6] = best;
            __syncthreads();
            best = s_red[parity][0];
#pragma unroll
            for (int w = 1; w < ATSS_WAVES; ++w) best = s_red[parity][w] < best ? s_red[parity][w] : best;
            parity ^= 1;                                 // the next round writes the other buffer: one barrier per round
            prev = best;
            if (tid == 0) {                              // r < k <= HW: a key above prev always exists, so the low word is a pixel of the level
                const unsigned pix = (unsigned)(best & 0xFFFFFFFFull);
                s_pix[n + r] = (int)(pix < (unsigned)HW ? pix : (unsigned)HW - 1u);
                s_lvl[n + r] = s;
            }
        }
        n += k;
    }
    if (tid == 0) s_npos = 0;
    __syncthreads();

    // 2. IoU of the candidate's anchor (a square of side anchor_scale * stride) and the GT box: fd_pairwise_iou(plus_one = 0)
    float cx = 0.f, cy = 0.f, iou = 0.f;
    int loc = 0;
    if (tid < n) {
        const int s = s_lvl[tid], pix = s_pix[tid], W = a.W[s], st = a.stride[s];
        const int py = (int)((unsigned)pix / (unsigned)W), px = pix - py * W;
        loc = a.loc_start[s] + pix;
        cx = atss_centre(px, st); cy = atss_centre(py, st);
        const float rad = (a.anchor_scale * (float)st) / 2.0f;
        const float ax1 = cx - rad, ay1 = cy - rad, ax2 = cx + rad, ay2 = cy + rad;
        const float ltx = fmaxf(ax1, g.x), lty = fmaxf(ay1, g.y);
        const float rbx = fminf(ax2, g.z), rby = fminf(ay2, g.w);
        const float w = fmaxf(rbx - ltx, 0.0f), h = fmaxf(rby - lty, 0.0f);
        const float inter = w * h;
        const float a1 = (ax2 - ax1) * (ay2 - ay1);
        const float a2 = (g.z - g.x) * (g.w - g.y);
        iou = inter / ((a1 + a2) - inter);
        s_iou[tid] = iou;
    }
    __syncthreads();

    // 3. threshold in fp64, sequentially in candidate order, in one lane
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += (double)s_iou[i];
        const double mean = sum / (double)n;
        double ss = 0.0;
        for (int i = 0; i < n; ++i) {
            const double d = (double)s_iou[i] - mean;
            ss += d * d;
        }
        const double sd = n > 1 ? sqrt(ss / (double)(n - 1)) : 0.0;
        s_thr = mean + sd;
    }
    __syncthreads();

    // 4. + 5. positives claim their location: larger iou wins, equal iou goes to the lower row (larger ~m).  The low word
    //    ~m is never 0 for m < M, so a claim differs from the memset's 0 even when iou underflows to +0.
    if (tid < n) {
        const float inside = fminf(fminf(cx - g.x, cy - g.y), fminf(g.z - cx, g.w - cy));
        if ((double)iou >= s_thr && inside > a.inside_eps) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)~(unsigned)m;
            atomicMax(&a.claim[(long)b * a.L + loc], key);
            atomicAdd(&s_npos, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (a.gt_thr) a.gt_thr[row] = s_thr;
        if (a.gt_npos) a.gt_npos[row] = s_npos;
    }
}

__global__ __launch_bounds__(256) void atss_output_kernel(AtssArgs a) {
    const int b = blockIdx.y;
    const int loc = blockIdx.x * 256 + threadIdx.x;
    if (loc >= a.L) return;
    const long o = (long)b * a.L + loc;
    const unsigned m = ~(unsigned)(a.claim[o] & 0xFFFFFFFFull);   // unclaimed: 0xFFFFFFFF, never < M
    if (m < (unsigned)a.M) {
        int s = 0;
#pragma unroll
        for (int t = 1; t < FD_MAX_SEG; ++t)
            if (t < a.nseg && loc >= a.loc_start[t]) s = t;
        const int pix = loc - a.loc_start[s];
        const int W = a.W[s], st = a.stride[s];
        const int py = (int)((unsigned)pix / (unsigned)W), px = pix - py * W;
        const float x = atss_centre(px, st), y = atss_centre(py, st);
        const float4 g = reinterpret_cast<const float4*>(a.gt)[(long)b * a.M + m];
        const float4 off = make_float4(x - g.x, y - g.y, g.z - x, g.w - y);
        const float lr_min = fminf(off.x, off.z), lr_max = fmaxf(off.x, off.z);
        const float tb_min = fminf(off.y, off.w), tb_max = fmaxf(off.y, off.w);
        a.cls_t[o] = a.labels[(long)b * a.M + m];
        a.cnt_t[o] = sqrtf((lr_min * tb_min) / (lr_max * tb_max + 1e-10f));
        reinterpret_cast<float4*>(a.reg_t)[o] = off;
    } else {
        a.cls_t[o] = 0;
        a.cnt_t[o] = -1.0f;
        reinterpret_cast<float4*>(a.reg_t)[o] = make_float4(-1.f, -1.f, -1.f, -1.f);
    }
}

extern "C" int64_t fd_atss_workspace_bytes(int32_t B, int32_t L) {
    if (B < 1 || L < 1) return -1;
    return (int64_t)B * L * 8;
}

extern "C" int32_t fd_atss_gen_targets(const float* gt_boxes, const int64_t* labels, int32_t M, const fd_segs* segs,
                                       const int32_t* strides, int32_t topk, float anchor_scale, float inside_eps,
                                       int64_t* cls_target, float* cnt_target, float* reg_target, double* gt_thr,
                                       int32_t* gt_npos, void* workspace, fd_stream_t stream) {
    FD_REQUIRE(M >= 0, FD_E_INVAL, "fd_atss_gen_targets: M=%d", M);
    FD_REQUIRE(strides && cls_target && cnt_target && reg_target && workspace && (M == 0 || (gt_boxes && labels)), FD_E_INVAL,
               "fd_atss_gen_targets: null pointer");
    FD_REQUIRE(fd_segs_ok(segs) && segs->batch <= 65535, FD_E_INVAL, "fd_atss_gen_targets: bad level table");
    FD_REQUIRE(topk >= 1, FD_E_INVAL, "fd_atss_gen_targets: topk=%d", topk);
    FD_REQUIRE(topk <= FD_ATSS_MAX_TOPK, FD_E_UNSUPPORTED, "fd_atss_gen_targets: topk=%d > %d not supported", topk, FD_ATSS_MAX_TOPK);
    FD_REQUIRE(isfinite(anchor_scale) && anchor_scale > 0.f, FD_E_INVAL, "fd_atss_gen_targets: anchor_scale must be finite and > 0");
    FD_REQUIRE(isfinite(inside_eps) && inside_eps >= 0.f, FD_E_INVAL, "fd_atss_gen_targets: inside_eps must be finite and >= 0");
    FD_REQUIRE((((uintptr_t)gt_boxes | (uintptr_t)reg_target) & 15) == 0 && ((uintptr_t)workspace & 7) == 0, FD_E_INVAL,
               "fd_atss_gen_targets: gt_boxes / reg_target not 16-byte or workspace not 8-byte aligned");
    AtssArgs a;
    a.gt = gt_boxes; a.labels = (const long long*)labels; a.B = segs->batch; a.M = M; a.nseg = segs->nseg; a.topk = topk;
    int64_t L = 0;
    for (int s = 0; s < FD_MAX_SEG; ++s) {
        a.loc_start[s] = (int)L;
        if (s < segs->nseg) {
            // the centre expression multiplies a pixel index by the stride in int32
            FD_REQUIRE(strides[s] >= 1 && (int64_t)segs->H[s] * strides[s] <= INT32_MAX && (int64_t)segs->W[s] * strides[s] <= INT32_MAX,
                       FD_E_INVAL, "fd_atss_gen_targets: bad level table (stride %d of level %d)", strides[s], s);
            a.H[s] = segs->H[s]; a.W[s] = segs->W[s]; a.stride[s] = strides[s];
            L += (int64_t)segs->H[s] * segs->W[s];
            FD_REQUIRE(L <= INT32_MAX, FD_E_INVAL, "fd_atss_gen_targets: bad level table (too many locations)");
        } else { a.H[s] = a.W[s] = a.stride[s] = 1; }
    }
    a.loc_start[FD_MAX_SEG] = (int)L; a.L = (int)L;
    a.anchor_scale = anchor_scale; a.inside_eps = inside_eps;
    a.claim = (unsigned long long*)workspace; a.gt_thr = gt_thr; a.gt_npos = gt_npos;
    a.cls_t = (long long*)cls_target; a.cnt_t = cnt_target; a.reg_t = reg_target;
    if (hipMemsetAsync(workspace, 0, (size_t)a.B * (size_t)a.L * 8, (hipStream_t)stream) != hipSuccess) {
        fd_set_error("fd_atss_gen_targets: clearing the workspace failed");
        return FD_E_LAUNCH;
    }
    if (M > 0) {
        hipLaunchKernelGGL(atss_select_kernel, dim3(M, a.B), dim3(ATSS_THREADS), 0, (hipStream_t)stream, a);
        FD_CHECK_LAUNCH("fd_atss_gen_targets");
    }
    hipLaunchKernelGGL(atss_output_kernel, dim3((a.L + 255) / 256, a.B), dim3(256), 0, (hipStream_t)stream, a);
    FD_CHECK_LAUNCH("fd_atss_gen_targets");
    return FD_OK;
}
