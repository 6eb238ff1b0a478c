// fd_simota.hip — SimOTA target assignment (Ge et al., OTA, CVPR 2021; YOLOX) beside fd_fcos_gen_targets (fd_loss.hip) and
// fd_atss_gen_targets (fd_atss.hip): same level table, same location order, same three outputs, but ranked by what the network
// currently predicts.  DESIGN 4.3p states the definition; tests/simota_ref.py restates it in numpy.  Built with
// -ffp-contract=off: every fp32 operation rounds once.
//
//   simota_pairs_kernel   grid (L / 256, B)    per location: its 64-bit claim word = all ones (unclaimed); q, N, then per row iou
//                                              and cost -> workspace (iou, -1 for a non-candidate; key word = not-preferred bit :
//                                              cost bits, all ones for a non-candidate) and the optional pair_iou / pair_cost
//   simota_select_kernel  grid (M, B)          per ground-truth row: <= top_q arg-max rounds over (iou, ~loc) for the dynamic k,
//                                              then k arg-min rounds over (not preferred, cost, loc); every positive published
//                                              with one 64-bit atomicMin (not preferred : cost bits : row)
//   simota_output_kernel  grid (L / 256, B)    per location: claim word -> cls / cnt / reg, as gen_targets_kernel writes them
#include "fd_common.h"
#include <float.h>
#include <math.h>

#define SIMOTA_THREADS 256
#define SIMOTA_WAVES (SIMOTA_THREADS / 64)
#define SIMOTA_NO_KEY 0xFFFFFFFFu

struct SimotaArgs {
    const float* cls; const float* cnt; const float* reg;     // [B][L][C], [B][L], [B][L][4]
    const float* gt; const long long* labels;                 // [B][M][4], [B][M]
    int B, M, L, C, nseg, top_q, quality;
    int W[FD_MAX_SEG], stride[FD_MAX_SEG], loc_start[FD_MAX_SEG + 1];
    float centre_radius, iou_weight, inside_eps;
    unsigned long long* claim;      // [B][L]
    float* w_iou; unsigned* w_key;  // [B][M][L] each
    float* pair_iou; float* pair_cost; int* gt_k; int* gt_ncand;   // optional
    long long* cls_t; float* cnt_t; float* reg_t;
};

// centre of location (px, py) of a level with stride st: the expression of gen_targets_kernel
__device__ __forceinline__ float simota_centre(int p, int st) { return (float)(p * st) + (float)(st / 2); }

// -log(x), at most 100: log(0) and NaN both give 100 (the clamp of binary_cross_entropy)
__device__ __forceinline__ float simota_nl(float x) {
    const float v = -logf(x);
    return v < 100.0f ? v : 100.0f;
}

__device__ __forceinline__ bool simota_row_valid(const float4 g, long long label, int C) {
    return label >= 1 && label <= (long long)C && isfinite(g.x) && isfinite(g.y) && isfinite(g.z) && isfinite(g.w) && g.z > g.x && g.w > g.y;
}

// loc < L -> its level; pix, px, py inside the level
__device__ __forceinline__ void simota_locate(const SimotaArgs& a, int loc, int& st, float& cx, float& cy) {
    int s = 0;
#pragma unroll
    for (int t = 1; t < FD_MAX_SEG; ++t)
        if (t < a.nseg && loc >= a.loc_start[t]) s = t;
    const int pix = loc - a.loc_start[s];
    const int W = a.W[s];
    const int py = (int)((unsigned)pix / (unsigned)W), px = pix - py * W;
    st = a.stride[s];
    cx = simota_centre(px, st); cy = simota_centre(py, st);
}

__global__ __launch_bounds__(256) void simota_pairs_kernel(SimotaArgs a) {
    const int b = blockIdx.y;
    const int loc = blockIdx.x * 256 + threadIdx.x;
    if (loc >= a.L) return;
    int st; float cx, cy;
    simota_locate(a, loc, st, cx, cy);
    const size_t o = (size_t)b * a.L + loc;
    a.claim[o] = ~0ull;                                         // unclaimed: above every claim of simota_select_kernel
    const float z = fd_sigmoid(a.cnt[o]);
    const float* cl = a.cls + o * (size_t)a.C;
    float N = 0.0f;
    for (int c = 0; c < a.C; ++c) N = N + simota_nl(1.0f - sqrtf(fd_sigmoid(cl[c]) * z));
    const float4 d = reinterpret_cast<const float4*>(a.reg)[o];
    const float bx1 = cx - d.x, by1 = cy - d.y, bx2 = cx + d.z, by2 = cy + d.w;
    const float a1 = (bx2 - bx1) * (by2 - by1);
    const float radius = a.centre_radius * (float)st;
    for (int m = 0; m < a.M; ++m) {
        const size_t row = (size_t)b * a.M + m;                 // uniform over the workgroup
        const size_t idx = row * a.L + loc;
        const float4 g = reinterpret_cast<const float4*>(a.gt)[row];
        const long long label = a.labels[row];
        float iou = 0.0f, cost = INFINITY;
        if (simota_row_valid(g, label, a.C)) {
            float wv = -1.0f;
            unsigned key = SIMOTA_NO_KEY;
            const float inside = fminf(fminf(cx - g.x, cy - g.y), fminf(g.z - cx, g.w - cy));
            if (inside > a.inside_eps) {
                const float gx = (g.x + g.z) / 2.0f, gy = (g.y + g.w) / 2.0f;
                const bool pref = fmaxf(fabsf(cx - gx), fabsf(cy - gy)) < radius;
                // predicted box against the row: fd_pairwise_iou(plus_one = 0)
                const float ltx = fmaxf(bx1, g.x), lty = fmaxf(by1, g.y);
                const float rbx = fminf(bx2, g.z), rby = fminf(by2, g.w);
                const float w = fmaxf(rbx - ltx, 0.0f), h = fmaxf(rby - lty, 0.0f);
                const float inter = w * h;
                const float a2 = (g.z - g.x) * (g.w - g.y);
                iou = inter / ((a1 + a2) - inter);
                if (!(iou > 0.0f)) iou = 0.0f;
                if (iou > 1.0f) iou = 1.0f;
                const float qg = sqrtf(fd_sigmoid(cl[(int)label - 1]) * z);
                cost = ((N - simota_nl(1.0f - qg)) + simota_nl(qg)) + a.iou_weight * (0.0f - logf(iou + 1e-8f));
                if (!(cost < FLT_MAX)) cost = FLT_MAX;
                // +0 <= cost <= FLT_MAX: the sign bit is free for the preference, and the bits order as the floats do
                key = (pref ? 0u : 0x80000000u) | (__float_as_uint(cost) & 0x7FFFFFFFu);
                wv = iou;
            }
            a.w_iou[idx] = wv;
            a.w_key[idx] = key;
        }
        if (a.pair_iou) a.pair_iou[idx] = iou;
        if (a.pair_cost) a.pair_cost[idx] = cost;
    }
}

__device__ __forceinline__ unsigned long long simota_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long simota_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(SIMOTA_THREADS) void simota_select_kernel(SimotaArgs a) {
    __shared__ unsigned long long s_red[2][SIMOTA_WAVES];
    __shared__ int s_cnt[SIMOTA_WAVES];
    const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t row = (size_t)b * a.M + m;
    const float4 g = reinterpret_cast<const float4*>(a.gt)[row];
    if (!simota_row_valid(g, a.labels[row], a.C)) {      // uniform over the workgroup: padding takes no part
        if (tid == 0) {
            if (a.gt_k) a.gt_k[row] = 0;
            if (a.gt_ncand) a.gt_ncand[row] = 0;
        }
        return;
    }
    const float* iou = a.w_iou + row * a.L;
    const unsigned* keys = a.w_key + row * a.L;
    int parity = 0;

    // 3. dynamic k: round r takes the largest (iou, ~loc) below round r-1's, so nothing has to be marked as taken; equal IoUs
    //    are separate keys, and which of them comes first does not change the sum.  0 <= iou <= 1, so its bits order as the
    //    floats do; ~loc is never 0 for loc < L, so key 0 means "none left".
    float sum = 0.0f;
    int n = 0;
    unsigned long long prev = ~0ull;
    for (int r = 0; r < a.top_q; ++r) {
        unsigned long long best = 0ull;
        int cnt = 0;
        for (int p = tid; p < a.L; p += SIMOTA_THREADS) {
            const float v = iou[p];
            if (v >= 0.0f) {
                ++cnt;
                const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)~(unsigned)p;
                if (key < prev && key > best) best = key;
            }
        }
        best = simota_wave_max(best);
        if (r == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        }
        if ((tid & 63) == 0) {
            s_red[parity][tid >> 6] = best;
            if (r == 0) s_cnt[tid >> 6] = cnt;
        }
        __syncthreads();
        best = s_red[parity][0];
#pragma unroll
        for (int w = 1; w < SIMOTA_WAVES; ++w) best = s_red[parity][w] > best ? s_red[parity][w] : best;
        if (r == 0) {
#pragma unroll
            for (int w = 0; w < SIMOTA_WAVES; ++w) n += s_cnt[w];
        }
        parity ^= 1;                                     // the next round writes the other buffer: one barrier per round
        if (best == 0ull) break;                         // fewer than top_q candidates (uniform: every thread read the same words)
        sum = sum + __uint_as_float((unsigned)(best >> 32));
        prev = best;
    }
    int k = (int)sum;
    k = k < 1 ? 1 : k;
    k = k < n ? k : n;
    if (tid == 0) {
        if (a.gt_k) a.gt_k[row] = k;
        if (a.gt_ncand) a.gt_ncand[row] = n;
    }

    // 4. + 5. the k smallest (not preferred, cost, loc) claim their location: the smallest (not preferred, cost, row) wins.
    //    A claim is below 2^40, the all-ones word simota_pairs_kernel left above every claim, and atomicMin keeps the minimum in
    //    any order.
    prev = 0ull;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = ~0ull;
        for (int p = tid; p < a.L; p += SIMOTA_THREADS) {
            const unsigned hi = keys[p];
            if (hi != SIMOTA_NO_KEY) {
                const unsigned long long key = ((unsigned long long)hi << 32) | (unsigned)p;
                if ((r == 0 || key > prev) && key < best) best = key;
            }
        }
        best = simota_wave_min(best);
        if ((tid & 63) == 0) s_red[parity][tid >> 6] = best;
        __syncthreads();
        best = s_red[parity][0];
#pragma unroll
        for (int w = 1; w < SIMOTA_WAVES; ++w) best = s_red[parity][w] < best ? s_red[parity][w] : best;
        parity ^= 1;
        if (best == ~0ull) break;                        // r < k <= n: does not happen; never index with the sentinel
        prev = best;
        if (tid == 0) {
            const unsigned p = (unsigned)(best & 0xFFFFFFFFull);
            if (p < (unsigned)a.L) atomicMin(&a.claim[(size_t)b * a.L + p], ((best >> 32) << 8) | (unsigned long long)m);
        }
    }
}

__global__ __launch_bounds__(256) void simota_output_kernel(SimotaArgs a) {
    const int b = blockIdx.y;
    const int loc = blockIdx.x * 256 + threadIdx.x;
    if (loc >= a.L) return;
    const size_t o = (size_t)b * a.L + loc;
    const unsigned long long word = a.M > 0 ? a.claim[o] : ~0ull;      // M == 0: nothing wrote the claim words
    const unsigned m = (unsigned)(word & 0xFFull);
    if (word != ~0ull && m < (unsigned)a.M) {
        int st; float x, y;
        simota_locate(a, loc, st, x, y);
        const size_t row = (size_t)b * a.M + m;
        const float4 g = reinterpret_cast<const float4*>(a.gt)[row];
        const float4 off = make_float4(x - g.x, y - g.y, g.z - x, g.w - y);
        a.cls_t[o] = a.labels[row];
        if (a.quality) {
            a.cnt_t[o] = a.w_iou[row * a.L + loc];
        } else {
            const float lr_min = fminf(off.x, off.z), lr_max = fmaxf(off.x, off.z);
            const float tb_min = fminf(off.y, off.w), tb_max = fmaxf(off.y, off.w);
            a.cnt_t[o] = sqrtf((lr_min * tb_min) / (lr_max * tb_max + 1e-10f));
        }
        reinterpret_cast<float4*>(a.reg_t)[o] = off;
    } else {
        a.cls_t[o] = 0;
        a.cnt_t[o] = -1.0f;
        reinterpret_cast<float4*>(a.reg_t)[o] = make_float4(-1.f, -1.f, -1.f, -1.f);
    }
}

// claim words [B][L] (8 bytes), then the iou and the key word of every pair [B][M][L] (4 bytes each)
extern "C" int64_t fd_simota_workspace_bytes(int32_t B, int32_t M, int32_t L) {
    if (B < 1 || L < 1 || M < 0 || B > 65535 || M > FD_SIMOTA_MAX_GT) return -1;      // beyond what fd_simota_gen_targets accepts
    return (int64_t)B * L * 8 + (int64_t)B * M * L * 8;
}

extern "C" int32_t fd_simota_gen_targets(const float* cls_logits, const float* cnt_logits, const float* reg_pred, int32_t C,
                                         const float* gt_boxes, const int64_t* labels, int32_t M, const fd_segs* segs,
                                         const int32_t* strides, int32_t top_q, float centre_radius, float iou_weight,
                                         float inside_eps, int32_t quality, int64_t* cls_target, float* cnt_target,
                                         float* reg_target, float* pair_iou, float* pair_cost, int32_t* gt_k, int32_t* gt_ncand,
                                         void* workspace, fd_stream_t stream) {
    FD_REQUIRE(M >= 0, FD_E_INVAL, "fd_simota_gen_targets: M=%d", M);
    FD_REQUIRE(cls_logits && cnt_logits && reg_pred && strides && cls_target && cnt_target && reg_target && workspace &&
               (M == 0 || (gt_boxes && labels)), FD_E_INVAL, "fd_simota_gen_targets: null pointer");
    FD_REQUIRE(fd_segs_ok(segs) && segs->batch <= 65535, FD_E_INVAL, "fd_simota_gen_targets: bad level table");
    FD_REQUIRE(C >= 1, FD_E_INVAL, "fd_simota_gen_targets: C=%d", C);
    FD_REQUIRE(top_q >= 1, FD_E_INVAL, "fd_simota_gen_targets: top_q=%d", top_q);
    FD_REQUIRE(top_q <= FD_SIMOTA_MAX_TOPQ, FD_E_UNSUPPORTED, "fd_simota_gen_targets: top_q=%d > %d not supported", top_q, FD_SIMOTA_MAX_TOPQ);
    FD_REQUIRE(M <= FD_SIMOTA_MAX_GT, FD_E_UNSUPPORTED, "fd_simota_gen_targets: M=%d > %d not supported", M, FD_SIMOTA_MAX_GT);
    FD_REQUIRE(isfinite(centre_radius) && centre_radius >= 0.f, FD_E_INVAL, "fd_simota_gen_targets: centre_radius must be finite and >= 0");
    FD_REQUIRE(isfinite(iou_weight) && iou_weight >= 0.f, FD_E_INVAL, "fd_simota_gen_targets: iou_weight must be finite and >= 0");
    FD_REQUIRE(isfinite(inside_eps) && inside_eps >= 0.f, FD_E_INVAL, "fd_simota_gen_targets: inside_eps must be finite and >= 0");
    FD_REQUIRE(quality == 0 || quality == 1, FD_E_INVAL, "fd_simota_gen_targets: quality must be 0 (centre-ness) or 1 (IoU)");
    FD_REQUIRE((((uintptr_t)gt_boxes | (uintptr_t)reg_pred | (uintptr_t)reg_target) & 15) == 0 && ((uintptr_t)workspace & 7) == 0, FD_E_INVAL,
               "fd_simota_gen_targets: gt_boxes / reg_pred / reg_target not 16-byte or workspace not 8-byte aligned");
    SimotaArgs a;
    a.cls = cls_logits; a.cnt = cnt_logits; a.reg = reg_pred; a.gt = gt_boxes; a.labels = (const long long*)labels;
    a.B = segs->batch; a.M = M; a.C = C; a.nseg = segs->nseg; a.top_q = top_q; a.quality = quality;
    int64_t L = 0;
    for (int s = 0; s < FD_MAX_SEG; ++s) {
        a.loc_start[s] = (int)L;
        if (s < segs->nseg) {
            // the centre expression multiplies a pixel index by the stride in int32
            FD_REQUIRE(strides[s] >= 1 && (int64_t)segs->H[s] * strides[s] <= INT32_MAX && (int64_t)segs->W[s] * strides[s] <= INT32_MAX,
                       FD_E_INVAL, "fd_simota_gen_targets: bad level table (stride %d of level %d)", strides[s], s);
            a.W[s] = segs->W[s]; a.stride[s] = strides[s];
            L += (int64_t)segs->H[s] * segs->W[s];
            FD_REQUIRE(L <= INT32_MAX, FD_E_INVAL, "fd_simota_gen_targets: bad level table (too many locations)");
        } else { a.W[s] = a.stride[s] = 1; }
    }
    a.loc_start[FD_MAX_SEG] = (int)L; a.L = (int)L;
    a.centre_radius = centre_radius; a.iou_weight = iou_weight; a.inside_eps = inside_eps;
    const size_t BL = (size_t)a.B * (size_t)a.L;
    a.claim = (unsigned long long*)workspace;
    a.w_iou = (float*)((char*)workspace + BL * 8);
    a.w_key = (unsigned*)(a.w_iou + BL * (size_t)M);
    a.pair_iou = pair_iou; a.pair_cost = pair_cost; a.gt_k = gt_k; a.gt_ncand = gt_ncand;
    a.cls_t = (long long*)cls_target; a.cnt_t = cnt_target; a.reg_t = reg_target;
    const dim3 per_loc((a.L + 255) / 256, a.B);
    if (M > 0) {
        hipLaunchKernelGGL(simota_pairs_kernel, per_loc, dim3(256), 0, (hipStream_t)stream, a);
        FD_CHECK_LAUNCH("fd_simota_gen_targets");
        hipLaunchKernelGGL(simota_select_kernel, dim3(M, a.B), dim3(SIMOTA_THREADS), 0, (hipStream_t)stream, a);
        FD_CHECK_LAUNCH("fd_simota_gen_targets");
    }
    hipLaunchKernelGGL(simota_output_kernel, per_loc, dim3(256), 0, (hipStream_t)stream, a);
    FD_CHECK_LAUNCH("fd_simota_gen_targets");
    return FD_OK;
}
