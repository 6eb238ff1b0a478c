// fd_avg.hip — averaging the model's weights on the device (include/fcosdet.h "Averaging the model's weights"):
// fd_avg_begin, fd_avg_update_f32, fd_avg_copy_bytes.
//
// Built with -ffp-contract=off: avg + (p - avg) * w rounds as written (the float64 restatement in tests/avg_ref.py), and an element with
// p == avg comes back unchanged whatever w is.
//
// Streaming kernels: 12 B per element (update) / 2 B per byte (copy), no LDS, no atomics.  Every element is read and written by exactly one
// lane of one launch; the state block is written by the begin launch alone and only read here.
#include "fd_common.h"

#include <cmath>

#define AVG_THREADS 256
#define AVG_MAX_BLOCKS_X 512   // 512 x 256 lanes x 16 B = 2 MiB per sweep and tensor, as the optimizer kernels

// ---------------------------------------------------------------------------------------------------------------------------------------
// begin: one lane.  The only writer of fd_avg_state and, among these launches, of *n_averaged.
__global__ void avg_begin_kernel(fd_avg_state* st, int64_t* n_averaged, const int64_t* skip, const int64_t* global_step, const fd_avg_begin_params bp) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bool apply = !(skip != nullptr && *skip != 0);
    if (apply && global_step != nullptr) {
        const int64_t G = *global_step;
        apply = G >= bp.start_step && (G - bp.start_step) % bp.every == 0;
    }
    double w = 0.0;
    if (apply) {
        const int64_t n = *n_averaged;
        w = n == 0 ? 1.0 : (bp.mode == FD_AVG_SWA ? 1.0 / (double)(n + 1) : 1.0 - bp.decay);
        *n_averaged = n + 1;
    }
    st->apply = apply ? 1 : 0;
    st->weight = w;
    st->weight_f32 = (float)w;
    st->reserved0 = 0.0f;
    st->reserved1 = 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// update: COPY = the weight is 1 (no arithmetic: the bits of p, NaN payloads included)
template <bool COPY>
__device__ __forceinline__ float avg_one(float a, float p, float w) {
    if (COPY) return p;
    return a + (p - a) * w;
}

// One tensor of the chunk: elements [0, head) scalar up to the 16-byte boundary, then float4, then the scalar tail; all scalar when the
// two pointers do not share one alignment.
template <bool COPY>
__device__ __forceinline__ void avg_tensor(float* a, const float* p, long n, float w) {
    const long tid = (long)blockIdx.x * AVG_THREADS + threadIdx.x, stride = (long)gridDim.x * AVG_THREADS;
    const unsigned aa = (unsigned)((uintptr_t)a & 15u);
    if ((unsigned)((uintptr_t)p & 15u) != aa) {
        for (long i = tid; i < n; i += stride) a[i] = avg_one<COPY>(COPY ? 0.f : a[i], p[i], w);
        return;
    }
    long head = (long)(((16u - aa) & 15u) >> 2);     // fp32 tensors: aa is a multiple of 4
    if (head > n) head = n;
    const long nvec = (n - head) >> 2, tail0 = head + (nvec << 2);
    float4* a4 = reinterpret_cast<float4*>(a + head);
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    for (long i = tid; i < nvec; i += stride) {
        const float4 pv = p4[i];
        float4 av = pv;
        if (!COPY) {
            av = a4[i];
            av.x = avg_one<false>(av.x, pv.x, w);
            av.y = avg_one<false>(av.y, pv.y, w);
            av.z = avg_one<false>(av.z, pv.z, w);
            av.w = avg_one<false>(av.w, pv.w, w);
        }
        a4[i] = av;
    }
    // head and tail: at most 3 elements each, the first lanes of the tensor's first block
    if (blockIdx.x == 0) {
        const long t = threadIdx.x;
        if (t < head) a[t] = avg_one<COPY>(COPY ? 0.f : a[t], p[t], w);
        else if (t >= 4 && t - 4 < n - tail0) a[tail0 + (t - 4)] = avg_one<COPY>(COPY ? 0.f : a[tail0 + (t - 4)], p[tail0 + (t - 4)], w);
    }
}

__global__ __launch_bounds__(AVG_THREADS) void avg_update_kernel(const fd_avg_chunk c, const fd_avg_state* st) {
    if (st->apply == 0) return;
    const int t = blockIdx.y;
    const long n = c.numel[t];
    if ((long)blockIdx.x * AVG_THREADS >= n) return;   // a block past a short tensor's end (the grid follows the chunk's largest); covers n == 0
    const float w = st->weight_f32;
    if (w == 1.0f) avg_tensor<true>(c.avg[t], c.p[t], n, w);
    else avg_tensor<false>(c.avg[t], c.p[t], n, w);
}

// copy: bytes [0, head) up to dst's 16-byte boundary, then 16 bytes per lane, then the byte tail; all bytes when dst and src do not share
// one alignment (such buffers are BatchNorm statistics and counters: a few KB at most).
__global__ __launch_bounds__(AVG_THREADS) void avg_copy_kernel(const fd_avg_copy_chunk c, const fd_avg_state* st) {
    if (st->apply == 0) return;
    const int t = blockIdx.y;
    const long n = c.nbytes[t];
    if ((long)blockIdx.x * AVG_THREADS >= n) return;
    unsigned char* d = static_cast<unsigned char*>(c.dst[t]);
    const unsigned char* s = static_cast<const unsigned char*>(c.src[t]);
    const long tid = (long)blockIdx.x * AVG_THREADS + threadIdx.x, stride = (long)gridDim.x * AVG_THREADS;
    const unsigned ad = (unsigned)((uintptr_t)d & 15u);
    if ((unsigned)((uintptr_t)s & 15u) != ad) {
        for (long i = tid; i < n; i += stride) d[i] = s[i];
        return;
    }
    long head = (long)((16u - ad) & 15u);
    if (head > n) head = n;
    const long nvec = (n - head) >> 4, tail0 = head + (nvec << 4);
    uint4* d4 = reinterpret_cast<uint4*>(d + head);
    const uint4* s4 = reinterpret_cast<const uint4*>(s + head);
    for (long i = tid; i < nvec; i += stride) d4[i] = s4[i];
    // head and tail: at most 15 bytes each, lanes 0 .. 15 and 16 .. 31 of the buffer's first block
    if (blockIdx.x == 0) {
        const long k = threadIdx.x;
        if (k < head) d[k] = s[k];
        else if (k >= 16 && k - 16 < n - tail0) d[tail0 + (k - 16)] = s[tail0 + (k - 16)];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
static unsigned avg_blocks_x(long max_units16) {   // max_units16: the largest tensor in 16-byte units
    long bx = (max_units16 + AVG_THREADS - 1) / AVG_THREADS;
    if (bx > AVG_MAX_BLOCKS_X) bx = AVG_MAX_BLOCKS_X;
    if (bx < 1) bx = 1;
    return (unsigned)bx;
}

extern "C" int32_t fd_avg_begin(fd_avg_state* state, int64_t* n_averaged, const int64_t* skip, const int64_t* global_step,
                                const fd_avg_begin_params* bp, fd_stream_t stream) {
    FD_REQUIRE(state, FD_E_INVAL, "fd_avg_begin: null state block");
    FD_REQUIRE(n_averaged, FD_E_INVAL, "fd_avg_begin: null n_averaged");
    FD_REQUIRE(bp, FD_E_INVAL, "fd_avg_begin: null params");
    FD_REQUIRE(bp->mode == FD_AVG_SWA || bp->mode == FD_AVG_EMA, FD_E_INVAL, "fd_avg_begin: unknown mode %d", bp->mode);
    FD_REQUIRE(std::isfinite(bp->decay) && bp->decay >= 0.0 && bp->decay <= 1.0, FD_E_INVAL, "fd_avg_begin: decay = %g outside [0, 1]", bp->decay);
    FD_REQUIRE(bp->every >= 1, FD_E_INVAL, "fd_avg_begin: every = %lld must be >= 1", (long long)bp->every);
    FD_REQUIRE(global_step || (bp->start_step == 0 && bp->every == 1), FD_E_INVAL,
               "fd_avg_begin: start_step = %lld / every = %lld need a global_step to gate on", (long long)bp->start_step, (long long)bp->every);
    hipLaunchKernelGGL(avg_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, n_averaged, skip, global_step, *bp);
    FD_CHECK_LAUNCH("fd_avg_begin");
    return FD_OK;
}

extern "C" int32_t fd_avg_update_f32(const fd_avg_chunk* c, const fd_avg_state* state, fd_stream_t stream) {
    FD_REQUIRE(c, FD_E_INVAL, "fd_avg_update_f32: null chunk");
    FD_REQUIRE(state, FD_E_INVAL, "fd_avg_update_f32: null state block");
    FD_REQUIRE(c->n >= 1 && c->n <= FD_OPTIM_MAX_TENSORS, FD_E_INVAL, "fd_avg_update_f32: n = %d outside [1, %d]", c->n, FD_OPTIM_MAX_TENSORS);
    long mx = 0;
    for (int i = 0; i < c->n; ++i) {
        FD_REQUIRE(c->numel[i] >= 0, FD_E_INVAL, "fd_avg_update_f32: tensor %d has a negative numel", i);
        if (c->numel[i] == 0) continue;
        FD_REQUIRE(c->avg[i] && c->p[i], FD_E_INVAL, "fd_avg_update_f32: tensor %d has a null avg / p", i);
        FD_REQUIRE((((uintptr_t)c->avg[i] | (uintptr_t)c->p[i]) & 3u) == 0, FD_E_INVAL, "fd_avg_update_f32: tensor %d is not 4-byte aligned", i);
        if (c->numel[i] > mx) mx = c->numel[i];
    }
    if (mx == 0) return FD_OK;
    hipLaunchKernelGGL(avg_update_kernel, dim3(avg_blocks_x((mx + 3) / 4), (unsigned)c->n, 1), dim3(AVG_THREADS), 0, (hipStream_t)stream, *c, state);
    FD_CHECK_LAUNCH("fd_avg_update_f32");
    return FD_OK;
}

extern "C" int32_t fd_avg_copy_bytes(const fd_avg_copy_chunk* c, const fd_avg_state* state, fd_stream_t stream) {
    FD_REQUIRE(c, FD_E_INVAL, "fd_avg_copy_bytes: null chunk");
    FD_REQUIRE(state, FD_E_INVAL, "fd_avg_copy_bytes: null state block");
    FD_REQUIRE(c->n >= 1 && c->n <= FD_OPTIM_MAX_TENSORS, FD_E_INVAL, "fd_avg_copy_bytes: n = %d outside [1, %d]", c->n, FD_OPTIM_MAX_TENSORS);
    long mx = 0;
    for (int i = 0; i < c->n; ++i) {
        FD_REQUIRE(c->nbytes[i] >= 0, FD_E_INVAL, "fd_avg_copy_bytes: buffer %d has a negative nbytes", i);
        if (c->nbytes[i] == 0) continue;
        FD_REQUIRE(c->dst[i] && c->src[i], FD_E_INVAL, "fd_avg_copy_bytes: buffer %d has a null dst / src", i);
        if (c->nbytes[i] > mx) mx = c->nbytes[i];
    }
    if (mx == 0) return FD_OK;
    hipLaunchKernelGGL(avg_copy_kernel, dim3(avg_blocks_x((mx + 15) / 16), (unsigned)c->n, 1), dim3(AVG_THREADS), 0, (hipStream_t)stream, *c, state);
    FD_CHECK_LAUNCH("fd_avg_copy_bytes");
    return FD_OK;
}
