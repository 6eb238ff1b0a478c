// fd_grad_norm.hip — the global gradient norm and the clip coefficient of the optimizer step (include/fcosdet.h "Optimizer step"):
// fd_grad_sumsq_slots, fd_grad_sumsq_f32, fd_grad_norm_workspace_bytes, fd_grad_clip_finish.
//
// One extra read of the gradients (4 B per element) and no write to them.  Every block of a sum-of-squares launch stores ONE fp64 partial into a slot
// of its own, and one workgroup adds the slots in index order: no floating-point atomics, no "last block" counter, so the result does not depend on
// the order in which blocks run and two runs on the same inputs give the same bits.  The square of an fp32 value is exact in fp64 (48 significant
// bits), so the only rounding is that of the fp64 additions; an fp32 accumulator would overflow at elements near 1e20.
#include "fd_common.h"

#include <cmath>

#define GN_THREADS 256
#define GN_WAVES (GN_THREADS / 64)
#define GN_UNROLL 4                                        // 16-byte loads in flight per lane
#define GN_BLOCK_ELEMS ((long)GN_THREADS * 4 * GN_UNROLL)  // elements one block covers per sweep
#define GN_MAX_BLOCKS_X 128                                // 128 x 4096 elements = 2 MiB per sweep and tensor, as the update kernels
#define GN_FINISH_THREADS 1024                             // one workgroup

__device__ __forceinline__ double gn_sq(float v) { return (double)v * (double)v; }

// wave butterfly, then the four waves through LDS; every lane of the block gets the same order of additions whatever the data
__device__ __forceinline__ double gn_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_kernel(const fd_grad_chunk c, double* __restrict__ slots) {
    __shared__ double wave_sum[GN_WAVES];
    const int t = blockIdx.y;
    const long n = c.numel[t];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    // The grid's x extent follows the chunk's largest tensor; a shorter tensor is shared among the first `live` blocks only, one per GN_BLOCK_ELEMS
    // elements, so that every lane that works has GN_UNROLL loads in flight.  The other blocks (and all of an empty tensor, whose pointer is not
    // looked at) store 0.0.
    long live = (n + GN_BLOCK_ELEMS - 1) / GN_BLOCK_ELEMS;
    if (live > (long)gridDim.x) live = gridDim.x;
    if ((long)blockIdx.x < live) {
        const float* g = c.g[t];
        const long tid = (long)blockIdx.x * GN_THREADS + threadIdx.x, stride = live * GN_THREADS;
        long head = (long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);      // fp32 tensors: the address is a multiple of 4
        if (head > n) head = n;
        const long nvec = (n - head) >> 2, tail0 = head + (nvec << 2);
        const float4* g4 = reinterpret_cast<const float4*>(g + head);
        long i = tid;
        for (; i + (GN_UNROLL - 1) * stride < nvec; i += GN_UNROLL * stride) {
            float4 v[GN_UNROLL];
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) v[u] = g4[i + u * stride];
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) {
                a0 += gn_sq(v[u].x);
                a1 += gn_sq(v[u].y);
                a2 += gn_sq(v[u].z);
                a3 += gn_sq(v[u].w);
            }
        }
        for (; i < nvec; i += stride) {
            const float4 v = g4[i];
            a0 += gn_sq(v.x);
            a1 += gn_sq(v.y);
            a2 += gn_sq(v.z);
            a3 += gn_sq(v.w);
        }
        // head and tail: at most 3 elements each, the first lanes of the tensor's first block
        if (blockIdx.x == 0) {
            const long k = threadIdx.x;
            if (k < head) a0 += gn_sq(g[k]);
            else if (k >= 4 && k - 4 < n - tail0) a0 += gn_sq(g[tail0 + (k - 4)]);
        }
    }
    const double w = gn_wave_sum((a0 + a1) + (a2 + a3));
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
#pragma unroll
        for (int k = 1; k < GN_WAVES; ++k) s += wave_sum[k];
        slots[(long)t * gridDim.x + blockIdx.x] = s;
    }
}

// One workgroup: lane l adds slots l, l + 1024, ... in index order (four loads in flight), then a fixed LDS tree; lane 0 writes the clip block.
__global__ __launch_bounds__(GN_FINISH_THREADS) void grad_clip_finish_kernel(const double* __restrict__ partials, int n_slots, const float* grad_scale,
                                                                             const float* found_inf, double max_norm, fd_grad_clip* out) {
    __shared__ double tree[GN_FINISH_THREADS];
    double acc = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * GN_FINISH_THREADS < n_slots; i += 4 * GN_FINISH_THREADS) {
        const double p0 = partials[i], p1 = partials[i + GN_FINISH_THREADS], p2 = partials[i + 2 * GN_FINISH_THREADS], p3 = partials[i + 3 * GN_FINISH_THREADS];
        acc += p0;
        acc += p1;
        acc += p2;
        acc += p3;
    }
    for (; i < n_slots; i += GN_FINISH_THREADS) acc += partials[i];
    tree[threadIdx.x] = acc;
    __syncthreads();
    for (int w = GN_FINISH_THREADS / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double sumsq = tree[0];
    const double scale = grad_scale != nullptr ? (double)*grad_scale : 1.0;
    const double total_norm = sqrt(sumsq) / scale;
    const bool found = !isfinite(sumsq) || (found_inf != nullptr && *found_inf != 0.0f);
    double coef = 1.0;
    if (!found) coef = fmin(1.0, max_norm / (total_norm + 1e-6));
    out->sumsq = sumsq;
    out->total_norm = total_norm;
    out->clip_coef = coef;
    out->eff_scale = coef == 1.0 ? (float)scale : (float)(scale / coef);
    out->found = found ? 1.0f : 0.0f;
    out->total_norm_f32 = (float)total_norm;
    out->reserved0 = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
static int grad_chunk_check(const char* who, const fd_grad_chunk* c, long* max_numel) {
    FD_REQUIRE(c, FD_E_INVAL, "%s: null chunk", who);
    FD_REQUIRE(c->n >= 1 && c->n <= FD_OPTIM_MAX_TENSORS, FD_E_INVAL, "%s: n = %d outside [1, %d]", who, c->n, FD_OPTIM_MAX_TENSORS);
    long mx = 0;
    for (int i = 0; i < c->n; ++i) {
        FD_REQUIRE(c->numel[i] >= 0, FD_E_INVAL, "%s: tensor %d has a negative numel", who, i);
        if (c->numel[i] == 0) continue;
        FD_REQUIRE(c->g[i], FD_E_INVAL, "%s: tensor %d has a null g", who, i);
        FD_REQUIRE(((uintptr_t)c->g[i] & 3u) == 0, FD_E_INVAL, "%s: tensor %d is not 4-byte aligned", who, i);
        if (c->numel[i] > mx) mx = c->numel[i];
    }
    *max_numel = mx;
    return FD_OK;
}

static long grad_blocks_x(long max_numel) {
    long bx = (max_numel + GN_BLOCK_ELEMS - 1) / GN_BLOCK_ELEMS;
    if (bx > GN_MAX_BLOCKS_X) bx = GN_MAX_BLOCKS_X;
    if (bx < 1) bx = 1;
    return bx;
}

extern "C" int32_t fd_grad_sumsq_slots(const fd_grad_chunk* chunk) {
    long mx = 0;
    if (grad_chunk_check("fd_grad_sumsq_slots", chunk, &mx) != FD_OK) return -1;
    return (int32_t)(grad_blocks_x(mx) * chunk->n);
}

extern "C" int64_t fd_grad_norm_workspace_bytes(int32_t n_chunks) {
    if (n_chunks < 0) return -1;
    return (int64_t)n_chunks * FD_OPTIM_MAX_TENSORS * GN_MAX_BLOCKS_X * (int64_t)sizeof(double);
}

extern "C" int32_t fd_grad_sumsq_f32(const fd_grad_chunk* chunk, double* partials, int32_t first_slot, fd_stream_t stream) {
    long mx = 0;
    const int rc = grad_chunk_check("fd_grad_sumsq_f32", chunk, &mx);
    if (rc != FD_OK) return rc;
    FD_REQUIRE(partials, FD_E_INVAL, "fd_grad_sumsq_f32: null partials");
    FD_REQUIRE(((uintptr_t)partials & 7u) == 0, FD_E_INVAL, "fd_grad_sumsq_f32: partials are not 8-byte aligned");
    FD_REQUIRE(first_slot >= 0, FD_E_INVAL, "fd_grad_sumsq_f32: first_slot = %d is negative", first_slot);
    // A chunk of empty tensors still launches: its slots must hold 0.0, the workspace is never cleared.
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)grad_blocks_x(mx), (unsigned)chunk->n, 1), dim3(GN_THREADS), 0, (hipStream_t)stream, *chunk,
                       partials + first_slot);
    FD_CHECK_LAUNCH("fd_grad_sumsq_f32");
    return FD_OK;
}

extern "C" int32_t fd_grad_clip_finish(const double* partials, int32_t n_slots, const float* grad_scale, const float* found_inf, double max_norm,
                                       fd_grad_clip* out, fd_stream_t stream) {
    FD_REQUIRE(partials, FD_E_INVAL, "fd_grad_clip_finish: null partials");
    FD_REQUIRE(out, FD_E_INVAL, "fd_grad_clip_finish: null clip block");
    FD_REQUIRE(n_slots >= 0, FD_E_INVAL, "fd_grad_clip_finish: n_slots = %d is negative", n_slots);
    FD_REQUIRE(std::isfinite(max_norm) && max_norm > 0.0, FD_E_INVAL, "fd_grad_clip_finish: max_norm = %g must be positive and finite", max_norm);
    hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(GN_FINISH_THREADS), 0, (hipStream_t)stream, partials, (int)n_slots, grad_scale, found_inf,
                       max_norm, out);
    FD_CHECK_LAUNCH("fd_grad_clip_finish");
    return FD_OK;
}
