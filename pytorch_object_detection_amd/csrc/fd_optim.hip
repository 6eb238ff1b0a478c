// fd_optim.hip — the optimizer step (include/fcosdet.h "Optimizer step"): fd_optim_begin, fd_optim_sgd_f32, fd_optim_adam_f32.
//
// Built with -ffp-contract=off: the update rules round as written (the float64 restatement in tests/optim_ref.py is compared against torch's own
// kernels, and an FMA the source does not show would move the result by an ulp per step).
//
// Streaming kernels: 20 B per element (SGD with momentum) / 28 B (Adam), no LDS, no atomics.  Every element is read and written by exactly one
// lane of one launch; the state block is written by the begin launch alone and only read here, so no block reads a word another block of the
// same launch writes.
#include "fd_common.h"

#define OPT_THREADS 256
#define OPT_MAX_BLOCKS_X 512   // 512 x 256 lanes x 16 B = 2 MiB per sweep and tensor: the 2.4 M-element weights take five sweeps

// ---------------------------------------------------------------------------------------------------------------------------------------
// begin: one lane.  The only writer of fd_optim_state.
__global__ void optim_begin_kernel(fd_optim_state* st, const float* found_inf, const fd_optim_begin_params bp) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t G = st->global_step + 1;
    st->global_step = G;
    const bool skip = found_inf != nullptr && *found_inf != 0.0f;
    st->skip = skip ? 1 : 0;

    bool have = false;      // the rule assigned a rate at this step
    double lr = 0.0;
    if (bp.rule == FD_OPTIM_LR_TRAIN_PY) {
        if (G < bp.warmup_steps) {
            lr = (double)G / (double)bp.warmup_steps * bp.lr_init;
            have = true;
        }
        for (int i = 0; i < bp.n_drops; ++i)
            if (G == bp.drop_step[i]) {
                lr = bp.lr_init * bp.drop_factor[i];
                have = true;
            }
    } else if (bp.rule == FD_OPTIM_LR_TRAIN_NEW) {
        lr = bp.lr_init;
        have = true;
        if (G < bp.warmup_steps) {
            const double alpha = (double)G / (double)bp.warmup_steps;
            const double wf = bp.warmup_factor * (1.0 - alpha) + alpha;
            lr = lr * wf;
        } else {
            for (int i = 0; i < bp.n_drops; ++i) {
                if (G < bp.drop_step[i]) break;
                lr *= bp.gamma;
            }
        }
    }
    for (int g = 0; g < bp.n_groups; ++g) {
        if (bp.rule == FD_OPTIM_LR_NONE) {
            if (bp.lr_ptr[g] != nullptr)
                st->lr[g] = bp.lr_ptr_f64[g] ? *(const double*)bp.lr_ptr[g] : (double)*(const float*)bp.lr_ptr[g];
            else
                st->lr[g] = bp.lr_value[g];
        } else if (have) {
            st->lr[g] = lr;
        }
        int64_t t = st->applied[g];
        if (!skip && bp.active[g]) {
            t += 1;
            st->applied[g] = t;
        }
        if (bp.adam) {
            st->bc1[g] = 1.0 - pow(bp.beta1[g], (double)t);
            st->bc2[g] = 1.0 - pow(bp.beta2[g], (double)t);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// update rules on one element; the same functions serve the 16-byte and the scalar path
struct SgdRule {
    float lr, momentum, wd, inv_scale;
    bool nesterov, has_buf;
    __device__ __forceinline__ void one(float& p, float g, float& buf, float& /*unused*/) const {
        float d = g * inv_scale;
        d = d + wd * p;
        if (has_buf) {
            buf = momentum * buf + d;
            d = nesterov ? d + momentum * buf : buf;
        }
        p = p - lr * d;
    }
};

struct AdamRule {
    float lr_wd_keep;        // 1 - lr * wd (AdamW)
    float wd, inv_scale, one_m_b1, b2, one_m_b2, step_size, bc2_sqrt, eps;
    bool decoupled;
    __device__ __forceinline__ void one(float& p, float g, float& m, float& v) const {
        g = g * inv_scale;
        if (decoupled) p = p * lr_wd_keep;
        else g = g + wd * p;
        m = m + (g - m) * one_m_b1;
        v = b2 * v + one_m_b2 * g * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = p - (step_size * m) / denom;
    }
};

template <int NSTATE, class Rule>
__device__ __forceinline__ void optim_scalar(const Rule& r, float* p, const float* g, float* s0, float* s1, long i) {
    float pv = p[i], a = 0.f, b = 0.f;
    if (NSTATE >= 1) a = s0[i];
    if (NSTATE >= 2) b = s1[i];
    r.one(pv, g[i], a, b);
    p[i] = pv;
    if (NSTATE >= 1) s0[i] = a;
    if (NSTATE >= 2) s1[i] = b;
}

// One tensor of the chunk: elements [0, head) scalar up to the 16-byte boundary, then float4, then the scalar tail; all scalar when the
// pointers do not share one alignment (DDP's bucket views are 4-byte aligned, the parameters 256).  NSTATE: state tensors in use.
template <int NSTATE, class Rule>
__device__ __forceinline__ void optim_tensor(const Rule& r, float* p, const float* g, float* s0, float* s1, long n) {
    const long tid = (long)blockIdx.x * OPT_THREADS + threadIdx.x, stride = (long)gridDim.x * OPT_THREADS;
    const unsigned ap = (unsigned)((uintptr_t)p & 15u);
    bool same = ((unsigned)((uintptr_t)g & 15u) == ap);
    if (NSTATE >= 1) same = same && ((unsigned)((uintptr_t)s0 & 15u) == ap);
    if (NSTATE >= 2) same = same && ((unsigned)((uintptr_t)s1 & 15u) == ap);
    if (!same) {
        for (long i = tid; i < n; i += stride) optim_scalar<NSTATE>(r, p, g, s0, s1, i);
        return;
    }
    long head = (long)(((16u - ap) & 15u) >> 2);     // fp32 tensors: ap is a multiple of 4
    if (head > n) head = n;
    const long nvec = (n - head) >> 2, tail0 = head + (nvec << 2);
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    float4* a4 = NSTATE >= 1 ? reinterpret_cast<float4*>(s0 + head) : nullptr;
    float4* b4 = NSTATE >= 2 ? reinterpret_cast<float4*>(s1 + head) : nullptr;
    for (long i = tid; i < nvec; i += stride) {
        float4 pv = p4[i], a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        const float4 gv = g4[i];
        if (NSTATE >= 1) a = a4[i];
        if (NSTATE >= 2) b = b4[i];
        r.one(pv.x, gv.x, a.x, b.x);
        r.one(pv.y, gv.y, a.y, b.y);
        r.one(pv.z, gv.z, a.z, b.z);
        r.one(pv.w, gv.w, a.w, b.w);
        p4[i] = pv;
        if (NSTATE >= 1) a4[i] = a;
        if (NSTATE >= 2) b4[i] = b;
    }
    // head and tail: at most 3 elements each, the first lanes of the tensor's first block
    if (blockIdx.x == 0) {
        const long t = threadIdx.x;
        if (t < head) optim_scalar<NSTATE>(r, p, g, s0, s1, t);
        else if (t >= 4 && t - 4 < n - tail0) optim_scalar<NSTATE>(r, p, g, s0, s1, tail0 + (t - 4));
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sgd_kernel(const fd_optim_chunk c, const fd_optim_hyper h, const fd_optim_state* st, const float* grad_scale) {
    if (st->skip) return;
    const int t = blockIdx.y;
    const long n = c.numel[t];
    if ((long)blockIdx.x * OPT_THREADS >= n) return;   // a block past a short tensor's end (the grid follows the chunk's largest); holds on the scalar path too, and covers n == 0
    SgdRule r;
    r.lr = (float)st->lr[h.group];
    r.momentum = (float)h.momentum;
    r.wd = (float)h.weight_decay;
    r.inv_scale = grad_scale ? 1.0f / *grad_scale : 1.0f;
    r.nesterov = h.nesterov != 0;
    r.has_buf = true;
    if (h.momentum != 0.0) {
        optim_tensor<1>(r, c.p[t], c.g[t], c.s0[t], nullptr, n);
    } else {
        r.has_buf = false;
        optim_tensor<0>(r, c.p[t], c.g[t], nullptr, nullptr, n);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_adam_kernel(const fd_optim_chunk c, const fd_optim_hyper h, const fd_optim_state* st, const float* grad_scale) {
    if (st->skip) return;
    const int t = blockIdx.y;
    const long n = c.numel[t];
    if ((long)blockIdx.x * OPT_THREADS >= n) return;
    const double lr = st->lr[h.group];
    AdamRule r;
    r.lr_wd_keep = (float)(1.0 - lr * h.weight_decay);
    r.wd = (float)h.weight_decay;
    r.inv_scale = grad_scale ? 1.0f / *grad_scale : 1.0f;
    r.one_m_b1 = (float)(1.0 - h.beta1);
    r.b2 = (float)h.beta2;
    r.one_m_b2 = (float)(1.0 - h.beta2);
    r.step_size = (float)(lr / st->bc1[h.group]);
    r.bc2_sqrt = (float)sqrt(st->bc2[h.group]);
    r.eps = (float)h.eps;
    r.decoupled = h.decoupled_wd != 0;
    optim_tensor<2>(r, c.p[t], c.g[t], c.s0[t], c.s1[t], n);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host
static int optim_check(const char* who, const fd_optim_chunk* c, const fd_optim_hyper* h, const fd_optim_state* st, int nstate, long* max_numel) {
    FD_REQUIRE(c && h, FD_E_INVAL, "%s: null chunk / hyper", who);
    FD_REQUIRE(st, FD_E_INVAL, "%s: null state block", who);
    FD_REQUIRE(c->n >= 1 && c->n <= FD_OPTIM_MAX_TENSORS, FD_E_INVAL, "%s: n = %d outside [1, %d]", who, c->n, FD_OPTIM_MAX_TENSORS);
    FD_REQUIRE(h->group >= 0 && h->group < FD_OPTIM_MAX_GROUPS, FD_E_INVAL, "%s: group %d outside [0, %d)", who, h->group, FD_OPTIM_MAX_GROUPS);
    long mx = 0;
    for (int i = 0; i < c->n; ++i) {
        FD_REQUIRE(c->numel[i] >= 0, FD_E_INVAL, "%s: tensor %d has a negative numel", who, i);
        if (c->numel[i] == 0) continue;
        FD_REQUIRE(c->p[i] && c->g[i], FD_E_INVAL, "%s: tensor %d has a null p / g", who, i);
        FD_REQUIRE(nstate < 1 || c->s0[i], FD_E_INVAL, "%s: tensor %d has a null s0 (the rule needs it)", who, i);
        FD_REQUIRE(nstate < 2 || c->s1[i], FD_E_INVAL, "%s: tensor %d has a null s1 (the rule needs it)", who, i);
        FD_REQUIRE((((uintptr_t)c->p[i] | (uintptr_t)c->g[i] | (uintptr_t)(nstate >= 1 ? c->s0[i] : nullptr) | (uintptr_t)(nstate >= 2 ? c->s1[i] : nullptr)) & 3u) == 0,
                   FD_E_INVAL, "%s: tensor %d is not 4-byte aligned", who, i);
        if (c->numel[i] > mx) mx = c->numel[i];
    }
    *max_numel = mx;
    return FD_OK;
}

static dim3 optim_grid(const fd_optim_chunk* c, long max_numel) {
    long bx = (max_numel + (long)OPT_THREADS * 4 - 1) / ((long)OPT_THREADS * 4);
    if (bx > OPT_MAX_BLOCKS_X) bx = OPT_MAX_BLOCKS_X;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)c->n, 1);
}

extern "C" int32_t fd_optim_begin(fd_optim_state* state, const float* found_inf, const fd_optim_begin_params* bp, fd_stream_t stream) {
    FD_REQUIRE(state, FD_E_INVAL, "fd_optim_begin: null state block");
    FD_REQUIRE(bp, FD_E_INVAL, "fd_optim_begin: null params");
    FD_REQUIRE(bp->n_groups >= 1 && bp->n_groups <= FD_OPTIM_MAX_GROUPS, FD_E_INVAL, "fd_optim_begin: n_groups = %d outside [1, %d]", bp->n_groups, FD_OPTIM_MAX_GROUPS);
    FD_REQUIRE(bp->rule == FD_OPTIM_LR_NONE || bp->rule == FD_OPTIM_LR_TRAIN_PY || bp->rule == FD_OPTIM_LR_TRAIN_NEW, FD_E_INVAL, "fd_optim_begin: unknown rule %d", bp->rule);
    FD_REQUIRE(bp->n_drops >= 0 && bp->n_drops <= FD_OPTIM_MAX_DROPS, FD_E_INVAL, "fd_optim_begin: n_drops = %d outside [0, %d]", bp->n_drops, FD_OPTIM_MAX_DROPS);
    FD_REQUIRE(bp->rule == FD_OPTIM_LR_NONE || bp->warmup_steps >= 1, FD_E_INVAL, "fd_optim_begin: warmup_steps must be >= 1");
    hipLaunchKernelGGL(optim_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, found_inf, *bp);
    FD_CHECK_LAUNCH("fd_optim_begin");
    return FD_OK;
}

extern "C" int32_t fd_optim_sgd_f32(const fd_optim_chunk* chunk, const fd_optim_hyper* hyper, const fd_optim_state* state, const float* grad_scale,
                                    fd_stream_t stream) {
    long mx = 0;
    const int nstate = (hyper && hyper->momentum != 0.0) ? 1 : 0;
    const int rc = optim_check("fd_optim_sgd_f32", chunk, hyper, state, nstate, &mx);
    if (rc != FD_OK) return rc;
    if (mx == 0) return FD_OK;
    hipLaunchKernelGGL(optim_sgd_kernel, optim_grid(chunk, mx), dim3(OPT_THREADS), 0, (hipStream_t)stream, *chunk, *hyper, state, grad_scale);
    FD_CHECK_LAUNCH("fd_optim_sgd_f32");
    return FD_OK;
}

extern "C" int32_t fd_optim_adam_f32(const fd_optim_chunk* chunk, const fd_optim_hyper* hyper, const fd_optim_state* state, const float* grad_scale,
                                     fd_stream_t stream) {
    long mx = 0;
    const int rc = optim_check("fd_optim_adam_f32", chunk, hyper, state, 2, &mx);
    if (rc != FD_OK) return rc;
    if (mx == 0) return FD_OK;
    hipLaunchKernelGGL(optim_adam_kernel, optim_grid(chunk, mx), dim3(OPT_THREADS), 0, (hipStream_t)stream, *chunk, *hyper, state, grad_scale);
    FD_CHECK_LAUNCH("fd_optim_adam_f32");
    return FD_OK;
}
