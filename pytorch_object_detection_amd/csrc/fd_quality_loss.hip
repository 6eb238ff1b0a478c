// fd_quality_loss.hip — IoU-aware classification losses from logits, forward + backward (gfx950): Quality Focal Loss
// (Li et al., Generalized Focal Loss, NeurIPS 2020; beta = 2) and Varifocal Loss (Zhang et al., VarifocalNet, CVPR 2021;
// gamma = 2).  The soft target of element (b, l, c) is q[b][l] where labels[b][l] == c + 1 and 0 elsewhere; q comes from
// fd_ltrb_quality (the IoU of the predicted and the assigned box, fd_loss.hip's ltrb_terms() restated) or from the caller.
// DESIGN 4.3q states the definitions; tests/quality_loss_ref.py restates them in numpy.
//
// Work is laid out per location: a wave owns 64 consecutive locations (one label and one q per lane, read once), walks their
// 64 * C contiguous logits in 16 / 8 / 4-byte pieces and fetches the owning location's label and q across lanes.  The piece ->
// (location, class) mapping of a lane is the same in every tile, so the kernels hold no division in their loops.
#include "fd_common.h"

#define QL_MAXCHUNK 64       // double partials per image (loss, qsum pairs)
#define QL_TILE 64           // locations per wave tile
#define QL_WAVES 4           // waves per workgroup

// ---------------------------------------------------------------------------------------------- quality
__global__ __launch_bounds__(256) void ltrb_quality_kernel(const float4* __restrict__ pred, const float4* __restrict__ tgt,
                                                            const long long* __restrict__ labels, long total,
                                                            float* __restrict__ q) {
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        float v = 0.f;
        if (labels[o] > 0) {
            const float4 p = pred[o], t = tgt[o];
            // ltrb_terms() of fd_loss.hip, operation for operation (this file is compiled with -ffp-contract=off too)
            const float wi = fmaxf(fminf(p.z, t.z) + fminf(p.x, t.x), 0.f);
            const float hi = fmaxf(fminf(p.w, t.w) + fminf(p.y, t.y), 0.f);
            const float ov = wi * hi;
            const float a1 = (p.z + p.x) * (p.w + p.y);
            const float a2 = (t.z + t.x) * (t.w + t.y);
            const float U = (a1 + a2) - ov;
            const float iou = ov / U;
            v = (iou > 0.f) ? fminf(iou, 1.0f) : 0.f;      // NaN (0 / 0) and negative values compare false
        }
        q[o] = v;
    }
}

extern "C" int32_t fd_ltrb_quality(const float* pred, const float* target, const int64_t* labels, int32_t B, int32_t L,
                                   float* q_out, fd_stream_t stream) {
    FD_REQUIRE(pred && target && labels && q_out, FD_E_INVAL, "fd_ltrb_quality: null pointer");
    FD_REQUIRE(B >= 1 && L >= 1, FD_E_INVAL, "fd_ltrb_quality: bad shape B=%d L=%d", B, L);
    FD_REQUIRE((((uintptr_t)pred | (uintptr_t)target) & 15) == 0, FD_E_INVAL, "fd_ltrb_quality: not 16-byte aligned");
    const long total = (long)B * L;
    long g = (total + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(ltrb_quality_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, (const float4*)pred,
                       (const float4*)target, (const long long*)labels, total, q_out);
    FD_CHECK_LAUNCH("fd_ltrb_quality");
    return FD_OK;
}

// ---------------------------------------------------------------------------------------------- the two terms
// e = exp(-|x|) never overflows; s and 1 - s are both formed from it, so neither cancels at a saturated logit.
// bce(x, y) = max(x, 0) - x*y + log1p(e).  GRAD: also d loss / d x.
template <bool GRAD>
__device__ __forceinline__ float quality_term(float x, float y, int kind, float alpha, float* dldx) {
    const float e = expf(-fabsf(x));
    const float sp = log1pf(e);
    const float inv = 1.0f / (1.0f + e);
    const float s = (x >= 0.f) ? inv : e * inv;
    const float oms = (x >= 0.f) ? e * inv : inv;
    if (kind == 0) {                                   // QFL: (y - s)^2 * bce(x, y)
        const float b = (fmaxf(x, 0.f) - x * y) + sp;
        const float d = y - s;
        if (GRAD) *dldx = ((-2.0f * d) * (s * oms)) * b + (d * d) * (s - y);
        return (d * d) * b;
    }
    if (y > 0.f) {                                     // VFL, positive: y * bce(x, y)
        const float b = (fmaxf(x, 0.f) - x * y) + sp;
        if (GRAD) *dldx = y * (s - y);
        return y * b;
    }
    const float b0 = fmaxf(x, 0.f) + sp;               // VFL, negative: alpha * s^2 * bce(x, 0)
    if (GRAD) *dldx = alpha * (((2.0f * s) * (s * oms)) * b0 + (s * s) * s);
    return (alpha * (s * s)) * b0;
}

template <int W> struct QVec;
template <> struct QVec<4> { typedef float4 T; };
template <> struct QVec<2> { typedef float2 T; };
template <> struct QVec<1> { typedef float T; };

// where a lane's pieces lie: piece j = lane + 64 k of a tile belongs to location j / V, class (j % V) * W, V = C / W pieces per row
struct QWalk {
    int loc, rem, a, r, V;
    __device__ __forceinline__ QWalk(int lane, int V_) : loc(lane / V_), rem(lane - (lane / V_) * V_), a(QL_TILE / V_), r(QL_TILE - (QL_TILE / V_) * V_), V(V_) {}
    __device__ __forceinline__ void next() {
        loc += a; rem += r;
        if (rem >= V) { rem -= V; ++loc; }
    }
};

// the label (as a class index, -1 = no class of [0, C)) and q of the wave's 64 locations, one per lane
__device__ __forceinline__ void tile_targets(const long long* __restrict__ labels, const float* __restrict__ q, long row0, int l0,
                                             int lane, int nvalid, int C, int& cls, float& qv) {
    cls = -1; qv = 0.f;
    if (lane < nvalid) {
        const long long lb = labels[row0 + l0 + lane];
        qv = q[row0 + l0 + lane];
        if (lb >= 1 && lb <= (long long)C) cls = (int)lb - 1;
    }
}

template <int W>
__global__ __launch_bounds__(256) void quality_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ labels,
                                                           const float* __restrict__ q, int L, int C, int kind, float alpha,
                                                           int ntiles, int nchunk, double* __restrict__ part) {
    typedef typename QVec<W>::T VT;
    __shared__ double s_sum[256], s_q[256];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = C / W;
    const int per = (ntiles + nchunk - 1) / nchunk;
    const int lo = chunk * per, hi = min(ntiles, lo + per);
    const long row0 = (long)b * L;
    double acc = 0.0, qacc = 0.0;
    for (int tile = lo + wave; tile < hi; tile += QL_WAVES) {
        const int l0 = tile * QL_TILE;
        int cls; float qv;
        const int nvalid = min(QL_TILE, L - l0);       // locations of this tile inside the image
        tile_targets(labels, q, row0, l0, lane, nvalid, C, cls, qv);
        qacc += (double)qv;
        const VT* base = reinterpret_cast<const VT*>(x + (row0 + l0) * C);
        QWalk w(lane, V);
        for (int k = 0; k < V; ++k) {                  // V is the same in every lane: the cross-lane reads are not under divergence
            const int c_l = __shfl(cls, w.loc);
            const float q_l = __shfl(qv, w.loc);
            if (w.loc < nvalid) {
                const VT v = base[lane + QL_TILE * k];
                const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const float y = (w.rem * W + e == c_l) ? q_l : 0.f;
                    acc += (double)quality_term<false>(f[e], y, kind, alpha, nullptr);
                }
            }
            w.next();
        }
    }
    s_sum[tid] = acc; s_q[tid] = qacc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { s_sum[tid] += s_sum[tid + s]; s_q[tid] += s_q[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        part[((long)b * QL_MAXCHUNK + chunk) * 2] = s_sum[0];
        part[((long)b * QL_MAXCHUNK + chunk) * 2 + 1] = s_q[0];
    }
}

__global__ void quality_final_kernel(const double* __restrict__ part, int nchunk, float* __restrict__ loss, float* __restrict__ qsum) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        double a = 0.0, s = 0.0;
        for (int k = 0; k < nchunk; ++k) {
            a += part[((long)b * QL_MAXCHUNK + k) * 2];
            s += part[((long)b * QL_MAXCHUNK + k) * 2 + 1];
        }
        loss[b] = (float)a;
        qsum[b] = (float)s;
    }
}

template <int W>
__global__ __launch_bounds__(256) void quality_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ labels,
                                                           const float* __restrict__ q, const float* __restrict__ gscale, int L,
                                                           int C, int kind, float alpha, int ntiles, float* __restrict__ grad) {
    typedef typename QVec<W>::T VT;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = C / W;
    const long row0 = (long)b * L;
    const float gs = gscale[b];
    for (int tile = blockIdx.x * QL_WAVES + wave; tile < ntiles; tile += gridDim.x * QL_WAVES) {
        const int l0 = tile * QL_TILE;
        int cls; float qv;
        const int nvalid = min(QL_TILE, L - l0);       // locations of this tile inside the image
        tile_targets(labels, q, row0, l0, lane, nvalid, C, cls, qv);
        const VT* base = reinterpret_cast<const VT*>(x + (row0 + l0) * C);
        VT* out = reinterpret_cast<VT*>(grad + (row0 + l0) * C);
        QWalk w(lane, V);
        for (int k = 0; k < V; ++k) {
            const int c_l = __shfl(cls, w.loc);
            const float q_l = __shfl(qv, w.loc);
            if (w.loc < nvalid) {
                const VT v = base[lane + QL_TILE * k];
                const float* f = reinterpret_cast<const float*>(&v);
                VT g;
                float* gf = reinterpret_cast<float*>(&g);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const float y = (w.rem * W + e == c_l) ? q_l : 0.f;
                    float d;
                    quality_term<true>(f[e], y, kind, alpha, &d);
                    gf[e] = d * gs;
                }
                out[lane + QL_TILE * k] = g;
            }
            w.next();
        }
    }
}

// the widest piece the row length and the buffers' alignment allow
static inline int quality_width(int C, uintptr_t bits) {
    if (C % 4 == 0 && (bits & 15) == 0) return 4;
    if (C % 2 == 0 && (bits & 7) == 0) return 2;
    return 1;
}

extern "C" int64_t fd_quality_loss_workspace_bytes(int32_t B) {
    return B < 1 ? -1 : (int64_t)B * QL_MAXCHUNK * 2 * (int64_t)sizeof(double);
}

static int quality_args_ok(const char* who, int32_t B, int32_t L, int32_t C, int32_t kind, float alpha, float gamma, int32_t* code) {
    *code = FD_E_INVAL;
    if (!(B >= 1 && B <= 65535 && L >= 1 && C >= 1)) { fd_set_error("%s: bad shape B=%d L=%d C=%d", who, B, L, C); return 0; }
    if (!(kind == 0 || kind == 1)) { fd_set_error("%s: kind=%d is neither 0 (QFL) nor 1 (VFL)", who, kind); return 0; }
    if (kind == 1 && !(alpha >= 0.f && alpha <= 3.0e38f)) { fd_set_error("%s: alpha must be finite and >= 0", who); return 0; }
    if (gamma != 2.0f) {
        *code = FD_E_UNSUPPORTED;
        fd_set_error("%s: only beta = 2 (QFL) / gamma = 2 (VFL) is built", who);
        return 0;
    }
    return 1;
}

extern "C" int32_t fd_quality_loss_fwd(const float* logits, const int64_t* labels, const float* q, int32_t B, int32_t L, int32_t C,
                                       int32_t kind, float alpha, float gamma, float* loss_per_image, float* qsum_per_image,
                                       void* workspace, fd_stream_t stream) {
    FD_REQUIRE(logits && labels && q && loss_per_image && qsum_per_image && workspace, FD_E_INVAL, "fd_quality_loss_fwd: null pointer");
    int32_t code;
    if (!quality_args_ok("fd_quality_loss_fwd", B, L, C, kind, alpha, gamma, &code)) return code;
    FD_REQUIRE(((uintptr_t)workspace & 7) == 0, FD_E_INVAL, "fd_quality_loss_fwd: workspace not 8-byte aligned");
    const int ntiles = (L + QL_TILE - 1) / QL_TILE;
    const int nchunk = max(1, min(QL_MAXCHUNK, (ntiles + QL_WAVES - 1) / QL_WAVES));
    const dim3 grid(nchunk, B), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const long long* lb = (const long long*)labels;
    double* part = (double*)workspace;
    switch (quality_width(C, (uintptr_t)logits)) {
        case 4: hipLaunchKernelGGL(quality_fwd_kernel<4>, grid, block, 0, st, logits, lb, q, L, C, kind, alpha, ntiles, nchunk, part); break;
        case 2: hipLaunchKernelGGL(quality_fwd_kernel<2>, grid, block, 0, st, logits, lb, q, L, C, kind, alpha, ntiles, nchunk, part); break;
        default: hipLaunchKernelGGL(quality_fwd_kernel<1>, grid, block, 0, st, logits, lb, q, L, C, kind, alpha, ntiles, nchunk, part); break;
    }
    FD_CHECK_LAUNCH("fd_quality_loss_fwd");
    hipLaunchKernelGGL(quality_final_kernel, dim3(B), dim3(64), 0, st, (const double*)part, nchunk, loss_per_image, qsum_per_image);
    FD_CHECK_LAUNCH("fd_quality_loss_fwd (final)");
    return FD_OK;
}

extern "C" int32_t fd_quality_loss_bwd(const float* logits, const int64_t* labels, const float* q, const float* gscale, int32_t B,
                                       int32_t L, int32_t C, int32_t kind, float alpha, float gamma, float* grad_logits,
                                       fd_stream_t stream) {
    FD_REQUIRE(logits && labels && q && gscale && grad_logits, FD_E_INVAL, "fd_quality_loss_bwd: null pointer");
    int32_t code;
    if (!quality_args_ok("fd_quality_loss_bwd", B, L, C, kind, alpha, gamma, &code)) return code;
    const int ntiles = (L + QL_TILE - 1) / QL_TILE;
    const dim3 grid(min(1024, (ntiles + QL_WAVES - 1) / QL_WAVES), B), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const long long* lb = (const long long*)labels;
    switch (quality_width(C, (uintptr_t)logits | (uintptr_t)grad_logits)) {
        case 4: hipLaunchKernelGGL(quality_bwd_kernel<4>, grid, block, 0, st, logits, lb, q, gscale, L, C, kind, alpha, ntiles, grad_logits); break;
        case 2: hipLaunchKernelGGL(quality_bwd_kernel<2>, grid, block, 0, st, logits, lb, q, gscale, L, C, kind, alpha, ntiles, grad_logits); break;
        default: hipLaunchKernelGGL(quality_bwd_kernel<1>, grid, block, 0, st, logits, lb, q, gscale, L, C, kind, alpha, ntiles, grad_logits); break;
    }
    FD_CHECK_LAUNCH("fd_quality_loss_bwd");
    return FD_OK;
}
