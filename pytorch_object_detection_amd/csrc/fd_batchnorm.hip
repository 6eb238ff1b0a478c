// fd_batchnorm.hip -- BatchNorm2d on BATCH STATISTICS at any width C % 4 == 0, 4 <= C <= 4096 (the EfficientNet trunk: 16 ... 2304 channels, ResNet layer4:
// 2048), forward and backward on fp32 NHWC channel views, and the per-sample scale-add of drop-connect.
//
// The GroupNorm-with-G-=-C route of fd_layers.hip (fd_groupnorm_*, fd_batchnorm_sync_*) maps a thread to one channel quad of the WHOLE width and therefore
// takes only widths whose quad count divides 256.  Here the width is cut into `ntile` channel tiles of QT <= 64 quads and the rows into `nchunk` row chunks;
// a workgroup owns one (tile, chunk), thread t the quad t % QT on the row lane t / QT (RT = 256 / QT lanes; the 256 - QT * RT threads left over idle):
//     ntile = ceil(C/4 / 64),  QT = ceil(C/4 / ntile),  nchunk = min(1024, ceil(rows / 32)) re-derived so that no chunk is empty
// -- a function of (rows, C) alone.  Every sum is fp64: per thread over its rows in row order, the RT lanes in lane order (LDS), the chunks in index order by
// a second launch (4 interleaved chunk lanes, added in lane order).  No atomics: two runs are bit-identical.  Statistics and apply are separate launches.
//   forward    partial (sum x, sum x^2) -> final (mean, rstd, running statistics) -> apply y = act((x - mean) * rstd * gamma + beta)
//              residual form (fd_batchnorm_train_res_fwd_nhwc, the ResNet bottleneck's output): apply y = act((x - mean) * rstd * gamma + beta + res), act in
//              {NONE, RELU}; statistics of x alone, so everything but the apply launch is the plain form's.  Its backward is the plain one with act NONE on
//              g = dy * [y > 0] (g is the residual's gradient too): no kernel of its own.
//   backward   partial (sum dz, sum dz * xhat; dz = dy * act'(z), z recomputed from x exactly as the forward computed it) -> final (dgamma, dbeta and the two
//              per-channel constants c1 = rstd * gamma * mean(dz), c2 = rstd * gamma * mean(dz * xhat)) -> apply dx = rstd * gamma * dz - c1 - xhat * c2
// workspace (both directions, fd_batchnorm_train_workspace_bytes): double [2][C] then double [nchunk][2][C].  The forward leaves mean[C], rstd[C] in the first
// block (rstd rounded to fp32 first: the value the apply kernels multiply by); the backward leaves c1[C], c2[C] there.
// The same kernels serve nn.SyncBatchNorm (fd_batchnorm_train_sync_*, below): each direction in two phases around an all-reduce the caller issues.
// Every forward has a `_cma` sibling for nn.BatchNorm2d(momentum=None): the blend factor 1 / num_batches_tracked, read from the counter on the device.
// Every entry point with a float momentum, and both backwards, have an `_h` sibling on f16 MAPS (AMP: x, res, y, dy, dx as _Float16, 8-byte aligned views):
// the same kernels instantiated on the element type, so the same partition, operations and order -- y / dx are the fp32 kernel's rounded to f16 once, and
// the statistics, coefficients, running statistics, dgamma / dbeta and phase-1 sums are the fp32 kernel's bits on the upcast inputs.
#include "fd_common.h"

#define BN_MAXCHUNK 1024
#define BN_MAXC 4096

struct BnPart { int ntile, QT, RT, nchunk; long rows_per; };

static BnPart bn_partition(int64_t rows, int32_t C) {
    BnPart p;
    const int C4 = C / 4;
    p.ntile = (C4 + 63) / 64;
    p.QT = (C4 + p.ntile - 1) / p.ntile;
    p.RT = 256 / p.QT;
    const int64_t want = (rows + 31) / 32 < BN_MAXCHUNK ? (rows + 31) / 32 : BN_MAXCHUNK;
    p.rows_per = (long)((rows + want - 1) / want);
    p.nchunk = (int)((rows + p.rows_per - 1) / p.rows_per);
    return p;
}

// four elements per access: 16-byte aligned fp32 views, 8-byte aligned f16 views (half)
static inline bool bn_view_ok(const void* p, int cs, int co, int C, bool half = false) {
    return p && cs % 4 == 0 && co % 4 == 0 && co >= 0 && cs >= co + C && ((uintptr_t)p & (half ? 7 : 15)) == 0;
}

__device__ __forceinline__ float bn_act_grad(float z, int act) {
    if (act == FD_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == FD_ACT_SILU) { const float sg = fd_sigmoid(z); return sg * (1.f + z * (1.f - sg)); }
    return 1.f;
}

// The MAPS (x, dy / res, y / dx) hold fp32 or, in the `_h` entry points, _Float16 elements: the kernels are templates on the element type T.  Four elements
// are one access (16 bytes of fp32, 8 bytes of f16); an f16 element converts to fp32 exactly, every operation after the load is the fp32 kernel's in its
// order, and the result is rounded to f16 ONCE at the store (to nearest even; what exceeds 65504 becomes inf).  Parameters, statistics and sums do not change.
typedef _Float16 bn_h4_t __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ void bn_load4(const void* base, long i, float v[4]) {
    if constexpr (sizeof(T) == 4) {
        const float4 v4 = *reinterpret_cast<const float4*>((const float*)base + i);
        v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
    } else {
        const bn_h4_t h = *reinterpret_cast<const bn_h4_t*>((const _Float16*)base + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)h[e];
    }
}

template <typename T> __device__ __forceinline__ void bn_store4(void* base, long i, const float o[4]) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>((float*)base + i) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        bn_h4_t h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (_Float16)o[e];
        *reinterpret_cast<bn_h4_t*>((_Float16*)base + i) = h;
    }
}

struct BnArgs {                                         // (dy: the incoming gradient of the backward; the residual of the forward's residual form)
    const void* x; const void* dy; const float* gamma; const float* beta; void* out;     // x, dy, out: elements of the kernel's T
    int x_cs, x_co, dy_cs, dy_co, out_cs, out_co, C, QT, RT, act;
    long rows, rows_per;
};

// per (tile, chunk): forward (sum x, sum x^2), backward (sum dz, sum dz * xhat) -> part[chunk][2][C]
template <bool BWD, typename T = float>
__global__ __launch_bounds__(256) void bn_partial_kernel(BnArgs a, const double* __restrict__ stat, double* __restrict__ part) {
    __shared__ double s_a[1024], s_b[1024];          // [row lane][quad of the tile][4], at most 256 x 4
    const int tid = threadIdx.x, ql = tid % a.QT, rt = tid / a.QT;
    const int q = blockIdx.x * a.QT + ql, chunk = blockIdx.y;
    const bool lane_ok = rt < a.RT, live = lane_ok && q < a.C / 4;
    double sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
    if (live) {
        float mean[4], rstd[4], gm[4], bt[4];
        if constexpr (BWD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                mean[e] = (float)stat[4 * q + e]; rstd[e] = (float)stat[a.C + 4 * q + e]; gm[e] = a.gamma[4 * q + e]; bt[e] = a.beta[4 * q + e];
            }
        }
        const long r_begin = (long)chunk * a.rows_per, r_end = min(a.rows, r_begin + a.rows_per);
#pragma unroll 4
        for (long r = r_begin + rt; r < r_end; r += a.RT) {
            float v[4];
            bn_load4<T>(a.x, r * a.x_cs + a.x_co + 4 * q, v);
            if constexpr (BWD) {
                float g[4];
                bn_load4<T>(a.dy, r * a.dy_cs + a.dy_co + 4 * q, g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (v[e] - mean[e]) * rstd[e];
                    const float dz = g[e] * bn_act_grad(xh * gm[e] + bt[e], a.act);
                    sa[e] += (double)dz; sb[e] += (double)dz * (double)xh;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) { sa[e] += (double)v[e]; sb[e] += (double)v[e] * (double)v[e]; }
            }
        }
    }
    if (lane_ok) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { s_a[(rt * a.QT + ql) * 4 + e] = sa[e]; s_b[(rt * a.QT + ql) * 4 + e] = sb[e]; }
    }
    __syncthreads();
    const int TC = a.QT * 4;
    for (int i = tid; i < TC; i += 256) {
        const int c = blockIdx.x * TC + i;
        if (c >= a.C) continue;
        double sum_a = 0, sum_b = 0;
        for (int r = 0; r < a.RT; ++r) { sum_a += s_a[r * TC + i]; sum_b += s_b[r * TC + i]; }
        part[((long)chunk * 2) * a.C + c] = sum_a;
        part[((long)chunk * 2 + 1) * a.C + c] = sum_b;
    }
}

// the chunk sums of 64 channels per workgroup: 4 chunk lanes walk the chunks 4 apart in index order and are added in lane order
__device__ __forceinline__ bool bn_chunk_sums(const double* __restrict__ part, int nchunk, int C, double* s_a, double* s_b, int& c, double& A, double& B) {
    const int tid = threadIdx.x, cl = tid & 63, kl = tid >> 6;
    c = blockIdx.x * 64 + cl;
    double a = 0, b = 0;
    if (c < C)
        for (int k = kl; k < nchunk; k += 4) { a += part[((long)k * 2) * C + c]; b += part[((long)k * 2 + 1) * C + c]; }
    s_a[tid] = a; s_b[tid] = b;
    __syncthreads();
    if (kl != 0 || c >= C) return false;
    A = ((a + s_a[64 + cl]) + s_a[128 + cl]) + s_a[192 + cl];
    B = ((b + s_b[64 + cl]) + s_b[128 + cl]) + s_b[192 + cl];
    return true;
}

// channel c's statistics from its two sums over `count` rows (one rank's, or all ranks' behind an all-reduce): shared by the unsynchronised final kernel and
// the synchronised one, so that one rank gives the same bits through either
// nbt (or null): the layer's num_batches_tracked on the device, already incremented for this batch -- the cumulative moving average of momentum=None,
// momentum = (float)(1 / n), read here by the lane that blends; n < 1 writes neither running tensor
__device__ __forceinline__ void bn_fwd_stats(int c, int C, double A, double B, double count, float eps, float momentum, const int64_t* __restrict__ nbt,
                                             double* __restrict__ stat, float* __restrict__ rmean, float* __restrict__ rvar) {
    const double mean = A / count;
    double var = B / count - mean * mean;               // the biased batch variance
    if (var < 0) var = 0;
    stat[c] = mean;
    stat[C + c] = (double)(float)(1.0 / sqrt(var + (double)eps));
    if (rmean) {                                        // nn.BatchNorm2d: momentum update with the UNBIASED variance
        if (nbt) {
            const int64_t n = *nbt;
            if (n < 1) return;
            momentum = (float)(1.0 / (double)n);
        }
        const double unbiased = var * count / (count - 1.0);
        rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mean);
        rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * unbiased);
    }
}

// the two per-channel constants of the backward apply from (sum dz, sum dz * xhat) over `count` rows
__device__ __forceinline__ void bn_bwd_coef(int c, int C, double A, double B, double count, const float* __restrict__ gamma, const double* __restrict__ stat,
                                            double* __restrict__ coef) {
    const double k = stat[C + c] * (double)gamma[c] / count;
    coef[c] = k * A;
    coef[C + c] = k * B;
}

__global__ __launch_bounds__(256) void bn_fwd_final_kernel(const double* __restrict__ part, int nchunk, int C, double count, float eps, float momentum,
                                                            const int64_t* __restrict__ nbt, double* __restrict__ stat, float* __restrict__ rmean,
                                                            float* __restrict__ rvar) {
    __shared__ double s_a[256], s_b[256];
    int c; double A, B;
    if (!bn_chunk_sums(part, nchunk, C, s_a, s_b, c, A, B)) return;
    bn_fwd_stats(c, C, A, B, count, eps, momentum, nbt, stat, rmean, rvar);
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const double* __restrict__ part, int nchunk, int C, double count, const float* __restrict__ gamma,
                                                            const double* __restrict__ stat, double* __restrict__ coef, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
    __shared__ double s_a[256], s_b[256];
    int c; double A, B;
    if (!bn_chunk_sums(part, nchunk, C, s_a, s_b, c, A, B)) return;
    dbeta[c] = (float)A;
    dgamma[c] = (float)B;
    bn_bwd_coef(c, C, A, B, count, gamma, stat, coef);
}

// forward: y = act(xhat * gamma + beta), RES: y = act(xhat * gamma + beta + res), one float4 of res (a.dy) per float4 of x; backward: dx = rstd * gamma * dz
// - c1 - xhat * c2.  Same (tile, chunk) ownership as the partial kernel.
template <bool BWD, bool RES = false, typename T = float>
__global__ __launch_bounds__(256) void bn_apply_kernel(BnArgs a, const double* __restrict__ stat, const double* __restrict__ coef) {
    const int tid = threadIdx.x, ql = tid % a.QT, rt = tid / a.QT;
    const int q = blockIdx.x * a.QT + ql, chunk = blockIdx.y;
    if (rt >= a.RT || q >= a.C / 4) return;
    float mean[4], rstd[4], gm[4], bt[4], k1[4], c1[4], c2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mean[e] = (float)stat[4 * q + e]; rstd[e] = (float)stat[a.C + 4 * q + e]; gm[e] = a.gamma[4 * q + e]; bt[e] = a.beta[4 * q + e];
        if constexpr (BWD) { k1[e] = rstd[e] * gm[e]; c1[e] = (float)coef[4 * q + e]; c2[e] = (float)coef[a.C + 4 * q + e]; }
    }
    const long r_begin = (long)chunk * a.rows_per, r_end = min(a.rows, r_begin + a.rows_per);
#pragma unroll 4
    for (long r = r_begin + rt; r < r_end; r += a.RT) {
        float v[4], o[4];
        bn_load4<T>(a.x, r * a.x_cs + a.x_co + 4 * q, v);
        if constexpr (BWD) {
            float g[4];
            bn_load4<T>(a.dy, r * a.dy_cs + a.dy_co + 4 * q, g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (v[e] - mean[e]) * rstd[e];
                const float dz = g[e] * bn_act_grad(xh * gm[e] + bt[e], a.act);
                o[e] = (k1[e] * dz - c1[e]) - xh * c2[e];
            }
        } else if constexpr (RES) {
            float u[4];
            bn_load4<T>(a.dy, r * a.dy_cs + a.dy_co + 4 * q, u);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fd_act1(((v[e] - mean[e]) * rstd[e] * gm[e] + bt[e]) + u[e], a.act, 0.f);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fd_act1((v[e] - mean[e]) * rstd[e] * gm[e] + bt[e], a.act, 0.f);
        }
        bn_store4<T>(a.out, r * a.out_cs + a.out_co + 4 * q, o);
    }
}

// a rank of the synchronised form may hold ONE row: only the global count must reach 2
static bool bn_shape_ok(int64_t rows, int32_t C, int64_t min_rows) { return C >= 4 && C <= BN_MAXC && C % 4 == 0 && rows >= min_rows && rows < (1LL << 31); }
// the global count: a host value >= this rank's rows (and >= 2), or <= 0 = "read sums[2C] on the device"
static bool bn_sync_count_ok(double total_rows, int64_t rows) { return total_rows <= 0.0 || (total_rows >= (double)rows && total_rows >= 2.0); }

static int64_t bn_workspace_bytes(int64_t rows, int32_t C, int64_t min_rows) {
    if (!bn_shape_ok(rows, C, min_rows)) return -1;
    const BnPart p = bn_partition(rows, C);
    return ((int64_t)2 * C + (int64_t)p.nchunk * 2 * C) * (int64_t)sizeof(double);
}

extern "C" int64_t fd_batchnorm_train_workspace_bytes(int64_t rows, int32_t C) { return bn_workspace_bytes(rows, C, 2); }
extern "C" int64_t fd_batchnorm_train_sync_workspace_bytes(int64_t rows, int32_t C) { return bn_workspace_bytes(rows, C, 1); }

// What every entry point below starts with: the argument checks, the partition, the kernels' arguments and the workspace split.  rc != FD_OK: rejected
// (fd_last_error is set), nothing else is valid.  stat: mean[C], rstd[C] -- the head of the forward's own workspace, the forward's workspace in the backward.
struct BnLaunch {
    int32_t rc;
    BnArgs a;
    BnPart p;
    bool half;                                          // the maps hold _Float16 (the `_h` entry points)
    const double* stat;
    double* head;                                       // [2][C] in front of the workspace: the forward's statistics, the backward's c1, c2
    double* part;                                       // [nchunk][2][C] behind it
    hipStream_t st;
};

#define BN_REQUIRE(cond, code, ...)                                          \
    do {                                                                     \
        if (!(cond)) { fd_set_error(__VA_ARGS__); L.rc = (code); return L; } \
    } while (0)

// bwd: the backward (g = dy, out = dx; else out = y and g = the residual view of the residual form `res`, otherwise unused).  sync: one phase of the
// synchronised form -- rows from 1, and a call needs only what its phase touches (phase 1: the sums, and dgamma / dbeta in the backward; phase 2: out, and
// gamma / beta / res in the forward), where the unsynchronised call runs both halves and needs all of it.  `who` names the entry point in the messages.
// half: x, g and out hold _Float16 (8-byte aligned views); every check, its code and their order are the fp32 form's.
static BnLaunch bn_prologue(const char* who, bool half, bool bwd, bool sync, bool res, const void* x, int32_t x_cs, int32_t x_co, const void* g, int32_t g_cs,
                            int32_t g_co, const float* gamma, const float* beta, void* out, int32_t out_cs, int32_t out_co, const float* dgamma,
                            const float* dbeta, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, const double* sums, double total_rows,
                            const float* running_mean, const float* running_var, const void* fwd_workspace, void* workspace, int64_t workspace_bytes,
                            fd_stream_t stream) {
    BnLaunch L;
    L.rc = FD_OK;
    L.half = half;
    BN_REQUIRE(bn_shape_ok(rows, C, sync ? 1 : 2), FD_E_UNSUPPORTED, "%s: rows=%lld C=%d unsupported (C %% 4 == 0, 4 <= C <= %d, %d <= rows < 2^31)", who,
               (long long)rows, C, BN_MAXC, sync ? 1 : 2);
    BN_REQUIRE(act == FD_ACT_NONE || act == FD_ACT_RELU || (!res && act == FD_ACT_SILU), FD_E_UNSUPPORTED,
               bwd ? "%s: activation %d has no backward" : "%s: activation %d unsupported", who, act);
    BN_REQUIRE(!sync || phase == 1 || phase == 2, FD_E_UNSUPPORTED,
               bwd ? "%s: phase %d (1: this rank's sums, dgamma, dbeta; 2: dx)" : "%s: phase %d (1: this rank's sums, 2: statistics + apply)", who, phase);
    const bool first = !sync || phase == 1, second = !sync || phase == 2;
    const bool in_ok = bn_view_ok(x, x_cs, x_co, C, half) && (!bwd || (bn_view_ok(g, g_cs, g_co, C, half) && gamma && beta));
    const bool phase_ok = (!second || (bn_view_ok(out, out_cs, out_co, C, half) && gamma && beta && (!res || bn_view_ok(g, g_cs, g_co, C, half)))) &&
                          (!(bwd && first) || (dgamma && dbeta));
    if (!sync) {
        BN_REQUIRE(in_ok && phase_ok, FD_E_INVAL, "%s: bad pointer / channel view (C=%d)", who, C);
    } else {
        BN_REQUIRE(in_ok && sums && ((uintptr_t)sums & 7) == 0, FD_E_INVAL, "%s: bad pointer / channel view (C=%d; sums: [2C + 1] doubles)", who, C);
        if (bwd) BN_REQUIRE(phase_ok, FD_E_INVAL, "%s: phase 1 needs dgamma and dbeta, phase 2 needs dx (C=%d)", who, C);
        else BN_REQUIRE(phase_ok, FD_E_INVAL, "%s: phase 2 needs y, gamma and beta%s (C=%d)", who, res ? " and res" : "", C);
        BN_REQUIRE(bn_sync_count_ok(total_rows, rows), FD_E_INVAL,
                   "%s: total_rows=%g: the global row count (>= this rank's %lld rows, >= 2), or -1: read from sums[2C] on the device", who, total_rows,
                   (long long)rows);
    }
    const int64_t need = bn_workspace_bytes(rows, C, 1);
    if (!bwd) {                                         // (the backward takes no running tensors, and its rstd comes from the forward's workspace)
        BN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), FD_E_INVAL, "%s: running_mean and running_var go together", who);
        BN_REQUIRE(eps >= 0.f, FD_E_INVAL, "%s: eps must not be negative", who);
        BN_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need, FD_E_INVAL,
                   "%s: workspace of %lld bytes, %lld needed (8-byte aligned)", who, (long long)workspace_bytes, (long long)need);
    } else {
        BN_REQUIRE(fwd_workspace && ((uintptr_t)fwd_workspace & 7) == 0 && workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need,
                   FD_E_INVAL, "%s: the forward's workspace and a workspace of %lld bytes needed (got %lld; 8-byte aligned)", who, (long long)need,
                   (long long)workspace_bytes);
    }
    L.p = bn_partition(rows, C);
    BnArgs& a = L.a;
    a.x = x; a.dy = g; a.gamma = gamma; a.beta = beta; a.out = out;
    a.x_cs = x_cs; a.x_co = x_co; a.dy_cs = g_cs; a.dy_co = g_co; a.out_cs = out_cs; a.out_co = out_co; a.C = C; a.QT = L.p.QT; a.RT = L.p.RT; a.act = act;
    a.rows = (long)rows; a.rows_per = L.p.rows_per;
    L.head = (double*)workspace;
    L.part = L.head + 2 * (long)C;
    L.stat = bwd ? (const double*)fwd_workspace : L.head;
    L.st = (hipStream_t)stream;
    return L;
}
#undef BN_REQUIRE

// the two kinds of launch over the maps, on the element type of the entry point (same grid, same ownership)
static void bn_launch_partial(const BnLaunch& L, bool bwd) {
    const dim3 grid(L.p.ntile, L.p.nchunk);
    if (!L.half) {
        if (bwd) hipLaunchKernelGGL((bn_partial_kernel<true, float>), grid, dim3(256), 0, L.st, L.a, L.stat, L.part);
        else hipLaunchKernelGGL((bn_partial_kernel<false, float>), grid, dim3(256), 0, L.st, L.a, L.stat, L.part);
    } else {
        if (bwd) hipLaunchKernelGGL((bn_partial_kernel<true, _Float16>), grid, dim3(256), 0, L.st, L.a, L.stat, L.part);
        else hipLaunchKernelGGL((bn_partial_kernel<false, _Float16>), grid, dim3(256), 0, L.st, L.a, L.stat, L.part);
    }
}

template <typename T> static void bn_launch_apply_t(const BnLaunch& L, bool bwd, bool res) {
    const dim3 grid(L.p.ntile, L.p.nchunk);
    if (bwd) hipLaunchKernelGGL((bn_apply_kernel<true, false, T>), grid, dim3(256), 0, L.st, L.a, L.stat, (const double*)L.head);
    else if (res) hipLaunchKernelGGL((bn_apply_kernel<false, true, T>), grid, dim3(256), 0, L.st, L.a, L.stat, (const double*)nullptr);
    else hipLaunchKernelGGL((bn_apply_kernel<false, false, T>), grid, dim3(256), 0, L.st, L.a, L.stat, (const double*)nullptr);
}

static void bn_launch_apply(const BnLaunch& L, bool bwd, bool res) {
    if (!L.half) bn_launch_apply_t<float>(L, bwd, res);
    else bn_launch_apply_t<_Float16>(L, bwd, res);
}

// the forward's launches; the residual form (`res` a fourth channel view, act in {NONE, RELU}) differs in the apply kernel alone
static int32_t bn_fwd_launches(const BnLaunch& L, bool res, float eps, float momentum, const int64_t* nbt, float* running_mean, float* running_var) {
    const int C = L.a.C;
    bn_launch_partial(L, false);
    FD_CHECK_LAUNCH("fd_batchnorm_train_fwd (partial)");
    hipLaunchKernelGGL(bn_fwd_final_kernel, dim3((C + 63) / 64), dim3(256), 0, L.st, (const double*)L.part, L.p.nchunk, C, (double)L.a.rows, eps, momentum,
                       nbt, L.head, running_mean, running_var);
    FD_CHECK_LAUNCH("fd_batchnorm_train_fwd (statistics)");
    bn_launch_apply(L, false, res);
    FD_CHECK_LAUNCH("fd_batchnorm_train_fwd (apply)");
    return FD_OK;
}

// Each entry point with a float momentum exists twice: on fp32 maps and, `_h`, on f16 maps.  One body serves both (half: the maps' element type;
// res_form false: the plain form, `res` unused).
static int32_t bn_train_fwd(const char* who, bool half, bool res_form, const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta,
                            const void* res, int32_t res_cs, int32_t res_co, void* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                            int32_t act, float momentum, float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                            fd_stream_t stream) {
    const BnLaunch L = bn_prologue(who, half, false, false, res_form, x, x_cs, x_co, res, res_cs, res_co, gamma, beta, y, y_cs, y_co, nullptr, nullptr, rows,
                                   C, eps, act, 0, nullptr, 0.0, running_mean, running_var, nullptr, workspace, workspace_bytes, stream);
    return L.rc != FD_OK ? L.rc : bn_fwd_launches(L, res_form, eps, momentum, nullptr, running_mean, running_var);
}

extern "C" int32_t fd_batchnorm_train_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y, int32_t y_cs,
                                               int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, float momentum, float* running_mean,
                                               float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    return bn_train_fwd("fd_batchnorm_train_fwd", false, false, x, x_cs, x_co, gamma, beta, nullptr, 0, 0, y, y_cs, y_co, rows, C, eps, act, momentum,
                        running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, void* y, int32_t y_cs,
                                                 int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, float momentum, float* running_mean,
                                                 float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    return bn_train_fwd("fd_batchnorm_train_fwd_h", true, false, x, x_cs, x_co, gamma, beta, nullptr, 0, 0, y, y_cs, y_co, rows, C, eps, act, momentum,
                        running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_res_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const float* res,
                                                   int32_t res_cs, int32_t res_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                                                   int32_t act, float momentum, float* running_mean, float* running_var, void* workspace,
                                                   int64_t workspace_bytes, fd_stream_t stream) {
    return bn_train_fwd("fd_batchnorm_train_res_fwd", false, true, x, x_cs, x_co, gamma, beta, res, res_cs, res_co, y, y_cs, y_co, rows, C, eps, act, momentum,
                        running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_res_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const void* res,
                                                     int32_t res_cs, int32_t res_co, void* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                                                     int32_t act, float momentum, float* running_mean, float* running_var, void* workspace,
                                                     int64_t workspace_bytes, fd_stream_t stream) {
    return bn_train_fwd("fd_batchnorm_train_res_fwd_h", true, true, x, x_cs, x_co, gamma, beta, res, res_cs, res_co, y, y_cs, y_co, rows, C, eps, act,
                        momentum, running_mean, running_var, workspace, workspace_bytes, stream);
}

// ---- The cumulative moving average (nn.BatchNorm2d(momentum=None)): the `_cma` siblings take the layer's num_batches_tracked in DEVICE memory where the
// plain forms take `float momentum`, and are bit for bit the plain form called with momentum = (float)(1.0 / n) for a counter holding n >= 1; n < 1 writes
// neither running tensor.  The counter is read by the statistics launch the plain form has anyway: no launch more, nothing read on the host.
static int32_t bn_counter_check(const char* who, const int64_t* nbt, const float* running_mean, const float* running_var) {
    FD_REQUIRE((!running_mean && !running_var) || (nbt && ((uintptr_t)nbt & 7) == 0), FD_E_INVAL,
               "%s: running tensors need num_batches_tracked, one int64 on the device (8-byte aligned)", who);
    return FD_OK;
}

extern "C" int32_t fd_batchnorm_train_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y, int32_t y_cs,
                                                   int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, const int64_t* num_batches_tracked,
                                                   float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    const BnLaunch L = bn_prologue("fd_batchnorm_train_fwd_cma", false, false, false, false, x, x_cs, x_co, nullptr, 0, 0, gamma, beta, y, y_cs, y_co, nullptr,
                                   nullptr, rows, C, eps, act, 0, nullptr, 0.0, running_mean, running_var, nullptr, workspace, workspace_bytes, stream);
    if (L.rc != FD_OK) return L.rc;
    const int32_t rc = bn_counter_check("fd_batchnorm_train_fwd_cma", num_batches_tracked, running_mean, running_var);
    return rc != FD_OK ? rc : bn_fwd_launches(L, false, eps, 0.f, num_batches_tracked, running_mean, running_var);
}

extern "C" int32_t fd_batchnorm_train_res_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const float* res,
                                                       int32_t res_cs, int32_t res_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C,
                                                       float eps, int32_t act, const int64_t* num_batches_tracked, float* running_mean, float* running_var,
                                                       void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    const BnLaunch L = bn_prologue("fd_batchnorm_train_res_fwd_cma", false, false, false, true, x, x_cs, x_co, res, res_cs, res_co, gamma, beta, y, y_cs, y_co,
                                   nullptr, nullptr, rows, C, eps, act, 0, nullptr, 0.0, running_mean, running_var, nullptr, workspace, workspace_bytes,
                                   stream);
    if (L.rc != FD_OK) return L.rc;
    const int32_t rc = bn_counter_check("fd_batchnorm_train_res_fwd_cma", num_batches_tracked, running_mean, running_var);
    return rc != FD_OK ? rc : bn_fwd_launches(L, true, eps, 0.f, num_batches_tracked, running_mean, running_var);
}

static int32_t bn_train_bwd(const char* who, bool half, const void* x, int32_t x_cs, int32_t x_co, const void* dy, int32_t dy_cs, int32_t dy_co,
                            const float* gamma, const float* beta, void* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows, int32_t C,
                            float eps, int32_t act, const void* fwd_workspace, void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    const BnLaunch L = bn_prologue(who, half, true, false, false, x, x_cs, x_co, dy, dy_cs, dy_co, gamma, beta, dx, dx_cs, dx_co, dgamma, dbeta,
                                   rows, C, eps, act, 0, nullptr, 0.0, nullptr, nullptr, fwd_workspace, workspace, workspace_bytes, stream);
    if (L.rc != FD_OK) return L.rc;
    bn_launch_partial(L, true);
    FD_CHECK_LAUNCH("fd_batchnorm_train_bwd (partial)");
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + 63) / 64), dim3(256), 0, L.st, (const double*)L.part, L.p.nchunk, C, (double)rows, gamma, L.stat, L.head,
                       dgamma, dbeta);
    FD_CHECK_LAUNCH("fd_batchnorm_train_bwd (sums)");
    bn_launch_apply(L, true, false);
    FD_CHECK_LAUNCH("fd_batchnorm_train_bwd (apply)");
    return FD_OK;
}

extern "C" int32_t fd_batchnorm_train_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co, const float* gamma,
                                               const float* beta, float* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows,
                                               int32_t C, float eps, int32_t act, const void* fwd_workspace, void* workspace, int64_t workspace_bytes,
                                               fd_stream_t stream) {
    return bn_train_bwd("fd_batchnorm_train_bwd", false, x, x_cs, x_co, dy, dy_cs, dy_co, gamma, beta, dx, dx_cs, dx_co, dgamma, dbeta, rows, C, eps, act,
                        fwd_workspace, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_bwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const void* dy, int32_t dy_cs, int32_t dy_co, const float* gamma,
                                                 const float* beta, void* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows,
                                                 int32_t C, float eps, int32_t act, const void* fwd_workspace, void* workspace, int64_t workspace_bytes,
                                                 fd_stream_t stream) {
    return bn_train_bwd("fd_batchnorm_train_bwd_h", true, x, x_cs, x_co, dy, dy_cs, dy_co, gamma, beta, dx, dx_cs, dx_co, dgamma, dbeta, rows, C, eps, act,
                        fwd_workspace, workspace, workspace_bytes, stream);
}

// ---- The synchronised form (nn.SyncBatchNorm at these widths): each direction cut in two around ONE all-reduce that the CALLER issues.
//   forward   phase 1: partial -> sums[c], sums[C + c] = this rank's sum x, sum x^2                         -> all-reduce(sums[0 .. 2C], the row count in sums[2C])
//             phase 2: (mean, rstd, running statistics) from the global sums and the global count -> apply on this rank's rows
//   backward  phase 1: partial (global mean / rstd from the forward's workspace) -> sums[c], sums[C + c] = this rank's sum dz, sum dz * xhat, and
//                      dgamma / dbeta from THESE local sums (DDP averages them, as with torch's SyncBatchNorm)  -> all-reduce(sums[0 .. 2C))
//             phase 2: (c1, c2) from the global sums and the global count -> apply
// The partial and apply kernels are the ones above; the chunk reduction is bn_chunk_sums and the per-channel finals are bn_fwd_stats / bn_bwd_coef, so one rank
// whose sums pass from phase 1 to phase 2 untouched gives the unsynchronised launch's bits.  count <= 0: the global count is read from sums[2C] on the device.
__global__ __launch_bounds__(256) void bn_wide_sync_sums_kernel(const double* __restrict__ part, int nchunk, int C, double* __restrict__ sums,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double s_a[256], s_b[256];
    int c; double A, B;
    if (!bn_chunk_sums(part, nchunk, C, s_a, s_b, c, A, B)) return;
    sums[c] = A;
    sums[C + c] = B;
    if (dgamma) { dbeta[c] = (float)A; dgamma[c] = (float)B; }
}

__global__ __launch_bounds__(256) void bn_wide_sync_fwd_final_kernel(const double* __restrict__ sums, int C, double count, float eps, float momentum,
                                                                 const int64_t* __restrict__ nbt, double* __restrict__ stat, float* __restrict__ rmean,
                                                                 float* __restrict__ rvar) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    if (count <= 0.0) count = sums[2 * C];
    bn_fwd_stats(c, C, sums[c], sums[C + c], count, eps, momentum, nbt, stat, rmean, rvar);
}

__global__ __launch_bounds__(256) void bn_wide_sync_bwd_coef_kernel(const double* __restrict__ sums, int C, double count, const float* __restrict__ gamma,
                                                                const double* __restrict__ stat, double* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    if (count <= 0.0) count = sums[2 * C];
    bn_bwd_coef(c, C, sums[c], sums[C + c], count, gamma, stat, coef);
}

// one phase of the synchronised forward; the residual form adds the `res` view in phase 2's apply kernel (act in {NONE, RELU}), phase 1 never reads it
static int32_t bn_sync_fwd_launches(const BnLaunch& L, bool res, int32_t phase, double* sums, double total_rows, float eps, float momentum,
                                    const int64_t* nbt, float* running_mean, float* running_var) {
    const int C = L.a.C;
    if (phase == 1) {
        bn_launch_partial(L, false);
        FD_CHECK_LAUNCH("fd_batchnorm_train_sync_fwd (partial)");
        hipLaunchKernelGGL(bn_wide_sync_sums_kernel, dim3((C + 63) / 64), dim3(256), 0, L.st, (const double*)L.part, L.p.nchunk, C, sums, (float*)nullptr,
                           (float*)nullptr);
        FD_CHECK_LAUNCH("fd_batchnorm_train_sync_fwd (sums)");
        return FD_OK;
    }
    hipLaunchKernelGGL(bn_wide_sync_fwd_final_kernel, dim3((C + 255) / 256), dim3(256), 0, L.st, (const double*)sums, C, total_rows, eps, momentum, nbt,
                       L.head, running_mean, running_var);
    FD_CHECK_LAUNCH("fd_batchnorm_train_sync_fwd (statistics)");
    bn_launch_apply(L, false, res);
    FD_CHECK_LAUNCH("fd_batchnorm_train_sync_fwd (apply)");
    return FD_OK;
}

static int32_t bn_train_sync_fwd(const char* who, bool half, bool res_form, const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta,
                                 const void* res, int32_t res_cs, int32_t res_co, void* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                                 int32_t act, int32_t phase, double* sums, double total_rows, float momentum, float* running_mean, float* running_var,
                                 void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    const BnLaunch L = bn_prologue(who, half, false, true, res_form, x, x_cs, x_co, res, res_cs, res_co, gamma, beta, y, y_cs, y_co, nullptr, nullptr, rows, C,
                                   eps, act, phase, sums, total_rows, running_mean, running_var, nullptr, workspace, workspace_bytes, stream);
    return L.rc != FD_OK ? L.rc : bn_sync_fwd_launches(L, res_form, phase, sums, total_rows, eps, momentum, nullptr, running_mean, running_var);
}

extern "C" int32_t fd_batchnorm_train_sync_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y, int32_t y_cs,
                                                    int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums,
                                                    double total_rows, float momentum, float* running_mean, float* running_var, void* workspace,
                                                    int64_t workspace_bytes, fd_stream_t stream) {
    return bn_train_sync_fwd("fd_batchnorm_train_sync_fwd", false, false, x, x_cs, x_co, gamma, beta, nullptr, 0, 0, y, y_cs, y_co, rows, C, eps, act, phase,
                             sums, total_rows, momentum, running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_sync_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, void* y, int32_t y_cs,
                                                      int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums,
                                                      double total_rows, float momentum, float* running_mean, float* running_var, void* workspace,
                                                      int64_t workspace_bytes, fd_stream_t stream) {
    return bn_train_sync_fwd("fd_batchnorm_train_sync_fwd_h", true, false, x, x_cs, x_co, gamma, beta, nullptr, 0, 0, y, y_cs, y_co, rows, C, eps, act, phase,
                             sums, total_rows, momentum, running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_sync_res_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const float* res,
                                                        int32_t res_cs, int32_t res_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C,
                                                        float eps, int32_t act, int32_t phase, double* sums, double total_rows, float momentum,
                                                        float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                                                        fd_stream_t stream) {
    return bn_train_sync_fwd("fd_batchnorm_train_sync_res_fwd", false, true, x, x_cs, x_co, gamma, beta, res, res_cs, res_co, y, y_cs, y_co, rows, C, eps, act,
                             phase, sums, total_rows, momentum, running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_sync_res_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const void* res,
                                                          int32_t res_cs, int32_t res_co, void* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C,
                                                          float eps, int32_t act, int32_t phase, double* sums, double total_rows, float momentum,
                                                          float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                                                          fd_stream_t stream) {
    return bn_train_sync_fwd("fd_batchnorm_train_sync_res_fwd_h", true, true, x, x_cs, x_co, gamma, beta, res, res_cs, res_co, y, y_cs, y_co, rows, C, eps,
                             act, phase, sums, total_rows, momentum, running_mean, running_var, workspace, workspace_bytes, stream);
}

// the `_cma` siblings of the two synchronised forwards; phase 1 does not look at the counter, as it does not look at the momentum
extern "C" int32_t fd_batchnorm_train_sync_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y,
                                                        int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase,
                                                        double* sums, double total_rows, const int64_t* num_batches_tracked, float* running_mean,
                                                        float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    const BnLaunch L = bn_prologue("fd_batchnorm_train_sync_fwd_cma", false, false, true, false, x, x_cs, x_co, nullptr, 0, 0, gamma, beta, y, y_cs, y_co, nullptr,
                                   nullptr, rows, C, eps, act, phase, sums, total_rows, running_mean, running_var, nullptr, workspace, workspace_bytes,
                                   stream);
    if (L.rc != FD_OK) return L.rc;
    const int32_t rc = bn_counter_check("fd_batchnorm_train_sync_fwd_cma", num_batches_tracked, running_mean, running_var);
    return rc != FD_OK ? rc : bn_sync_fwd_launches(L, false, phase, sums, total_rows, eps, 0.f, num_batches_tracked, running_mean, running_var);
}

extern "C" int32_t fd_batchnorm_train_sync_res_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta,
                                                            const float* res, int32_t res_cs, int32_t res_co, float* y, int32_t y_cs, int32_t y_co,
                                                            int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums, double total_rows,
                                                            const int64_t* num_batches_tracked, float* running_mean, float* running_var, void* workspace,
                                                            int64_t workspace_bytes, fd_stream_t stream) {
    const BnLaunch L = bn_prologue("fd_batchnorm_train_sync_res_fwd_cma", false, false, true, true, x, x_cs, x_co, res, res_cs, res_co, gamma, beta, y, y_cs, y_co,
                                   nullptr, nullptr, rows, C, eps, act, phase, sums, total_rows, running_mean, running_var, nullptr, workspace,
                                   workspace_bytes, stream);
    if (L.rc != FD_OK) return L.rc;
    const int32_t rc = bn_counter_check("fd_batchnorm_train_sync_res_fwd_cma", num_batches_tracked, running_mean, running_var);
    return rc != FD_OK ? rc : bn_sync_fwd_launches(L, true, phase, sums, total_rows, eps, 0.f, num_batches_tracked, running_mean, running_var);
}

static int32_t bn_train_sync_bwd(const char* who, bool half, const void* x, int32_t x_cs, int32_t x_co, const void* dy, int32_t dy_cs, int32_t dy_co,
                                 const float* gamma, const float* beta, void* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows,
                                 int32_t C, float eps, int32_t act, int32_t phase, double* sums, double total_rows, const void* fwd_workspace, void* workspace,
                                 int64_t workspace_bytes, fd_stream_t stream) {
    const BnLaunch L = bn_prologue(who, half, true, true, false, x, x_cs, x_co, dy, dy_cs, dy_co, gamma, beta, dx, dx_cs, dx_co, dgamma, dbeta,
                                   rows, C, eps, act, phase, sums, total_rows, nullptr, nullptr, fwd_workspace, workspace, workspace_bytes, stream);
    if (L.rc != FD_OK) return L.rc;
    if (phase == 1) {
        bn_launch_partial(L, true);
        FD_CHECK_LAUNCH("fd_batchnorm_train_sync_bwd (partial)");
        hipLaunchKernelGGL(bn_wide_sync_sums_kernel, dim3((C + 63) / 64), dim3(256), 0, L.st, (const double*)L.part, L.p.nchunk, C, sums, dgamma, dbeta);
        FD_CHECK_LAUNCH("fd_batchnorm_train_sync_bwd (sums)");
        return FD_OK;
    }
    hipLaunchKernelGGL(bn_wide_sync_bwd_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, L.st, (const double*)sums, C, total_rows, gamma, L.stat, L.head);
    FD_CHECK_LAUNCH("fd_batchnorm_train_sync_bwd (coefficients)");
    bn_launch_apply(L, true, false);
    FD_CHECK_LAUNCH("fd_batchnorm_train_sync_bwd (apply)");
    return FD_OK;
}

extern "C" int32_t fd_batchnorm_train_sync_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co,
                                                    const float* gamma, const float* beta, float* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta,
                                                    int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums, double total_rows,
                                                    const void* fwd_workspace, void* workspace, int64_t workspace_bytes, fd_stream_t stream) {
    return bn_train_sync_bwd("fd_batchnorm_train_sync_bwd", false, x, x_cs, x_co, dy, dy_cs, dy_co, gamma, beta, dx, dx_cs, dx_co, dgamma, dbeta, rows, C, eps,
                             act, phase, sums, total_rows, fwd_workspace, workspace, workspace_bytes, stream);
}

extern "C" int32_t fd_batchnorm_train_sync_bwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const void* dy, int32_t dy_cs, int32_t dy_co,
                                                      const float* gamma, const float* beta, void* dx, int32_t dx_cs, int32_t dx_co, float* dgamma,
                                                      float* dbeta, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums,
                                                      double total_rows, const void* fwd_workspace, void* workspace, int64_t workspace_bytes,
                                                      fd_stream_t stream) {
    return bn_train_sync_bwd("fd_batchnorm_train_sync_bwd_h", true, x, x_cs, x_co, dy, dy_cs, dy_co, gamma, beta, dx, dx_cs, dx_co, dgamma, dbeta, rows, C,
                             eps, act, phase, sums, total_rows, fwd_workspace, workspace, workspace_bytes, stream);
}

// ---- drop-connect: y = a * s[n] + r on [N][HW][C] channel views, s one fp32 per sample ON THE DEVICE (0 or 1 / (1 - p)), r may be NULL (the backward of the
// branch: the incoming gradient times s).  Elementwise with two roundings like the torch expression a * s + r; y may alias a.
__global__ __launch_bounds__(256) void sample_scale_add_kernel(const float* a, int a_cs, int a_co, const float* __restrict__ s, const float* r, int r_cs,
                                                                int r_co, float* y, int y_cs, int y_co, int HW, int C4, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int q, px;
        const long m = fd_div(i, C4, q);
        const long n = fd_div(m, HW, px);
        const float sc = s[n];
        const float4 v = *reinterpret_cast<const float4*>(a + m * a_cs + a_co + 4 * q);
        float4 o = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
        if (r) {
            const float4 u = *reinterpret_cast<const float4*>(r + m * r_cs + r_co + 4 * q);
            o.x += u.x; o.y += u.y; o.z += u.z; o.w += u.w;
        }
        *reinterpret_cast<float4*>(y + m * y_cs + y_co + 4 * q) = o;
    }
}

extern "C" int32_t fd_sample_scale_add_nhwc(const float* a, int32_t a_cs, int32_t a_co, const float* s, const float* r, int32_t r_cs, int32_t r_co, float* y,
                                            int32_t y_cs, int32_t y_co, int32_t N, int32_t HW, int32_t C, fd_stream_t stream) {
    FD_REQUIRE(N >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && (int64_t)N * HW < (1LL << 31), FD_E_INVAL,
               "fd_sample_scale_add: N >= 1, HW >= 1, N * HW < 2^31, C %% 4 == 0 (got N=%d HW=%d C=%d)", N, HW, C);
    FD_REQUIRE(bn_view_ok(a, a_cs, a_co, C) && bn_view_ok(y, y_cs, y_co, C) && (!r || bn_view_ok(r, r_cs, r_co, C)) && s && ((uintptr_t)s & 3) == 0, FD_E_INVAL,
               "fd_sample_scale_add: bad pointer / channel view (C=%d)", C);
    const long total = (long)N * HW * (C / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(sample_scale_add_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream, a, a_cs, a_co, s, r, r_cs,
                       r_co, y, y_cs, y_co, HW, C / 4, total);
    FD_CHECK_LAUNCH("fd_sample_scale_add_nhwc");
    return FD_OK;
}
