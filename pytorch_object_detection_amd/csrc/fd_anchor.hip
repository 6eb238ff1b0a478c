// fd_anchor.hip — the anchor side of the reference's DataEncoder on the device (gfx950): _get_anchor_boxes, encode
// (ground truth -> per-anchor regression / class targets) and decode (per-anchor predictions -> boxes and labels after
// NMS), utill/utills.py:100-199.  DESIGN §4.2f.
//   * every kernel derives its anchors from the row index and the small fd_anchor_params struct (a kernel argument the
//     host fills): no [A][4] anchor table is read from memory;
//   * encode: one launch per batch, the image's boxes staged once in LDS, one lane per anchor loops over them -- the
//     reference's [A][M] temporaries never exist; 16 + 8 bytes written per anchor;
//   * decode: one pass over the [B][A][C] logits with coalesced (float4 where C % 4 == 0) loads, G lanes per anchor row and
//     a cross-lane first-maximum over the fp32 SIGMOID values; then fd_fcos_topk, fd_box_nms_plus1 and a gather.
// Compiled with -ffp-contract=off: IoU, the divisions and the multiply-adds round once per operation, as on the CPU, so every
// decision and loc_xy are bit-exact against the reference; logf / expf are within 1 ulp on each side.
#include "fd_common.h"
#include <math.h>

// Anchor row r -> (cx, cy, w, h).  Row order: level, y, x, k (utills.py:121-136).
__device__ __forceinline__ float4 anchor_row(const fd_anchor_params& p, int r) {
    int start = 0, fmw = p.fm_w[0], lvl = 0;
    float gw = p.grid_w[0], gh = p.grid_h[0];
    int acc = 0;
#pragma unroll
    for (int l = 0; l < FD_ANCHOR_LEVELS - 1; ++l) {
        acc += FD_ANCHOR_PER_CELL * p.fm_w[l] * p.fm_h[l];
        if (r >= acc) { start = acc; lvl = l + 1; fmw = p.fm_w[l + 1]; gw = p.grid_w[l + 1]; gh = p.grid_h[l + 1]; }
    }
    const unsigned q = (unsigned)(r - start);
    const unsigned cell = q / FD_ANCHOR_PER_CELL, k = q - cell * FD_ANCHOR_PER_CELL;
    const unsigned y = cell / (unsigned)fmw, x = cell - y * (unsigned)fmw;
    const float* wh = &p.wh[0][0][0] + (lvl * FD_ANCHOR_PER_CELL + (int)k) * 2;
    return make_float4(((float)x + 0.5f) * gw, ((float)y + 0.5f) * gh, wh[0], wh[1]);
}

static bool anchor_params_ok(const fd_anchor_params* p, long* total) {
    long a = 0;
    for (int l = 0; l < FD_ANCHOR_LEVELS; ++l) {
        if (p->fm_w[l] < 1 || p->fm_h[l] < 1 || p->fm_w[l] > 65536 || p->fm_h[l] > 65536) return false;
        if (!(p->grid_w[l] > 0.f) || !(p->grid_h[l] > 0.f) || !isfinite(p->grid_w[l]) || !isfinite(p->grid_h[l])) return false;
        for (int k = 0; k < FD_ANCHOR_PER_CELL; ++k)
            for (int c = 0; c < 2; ++c)
                if (!(p->wh[l][k][c] > 0.f) || !isfinite(p->wh[l][k][c])) return false;
        a += (long)FD_ANCHOR_PER_CELL * p->fm_w[l] * p->fm_h[l];
    }
    *total = a;
    return a < (1l << 28);
}

#define FD_ANCHOR_CHECK_PARAMS(name)                                                                                                 \
    do {                                                                                                                             \
        FD_REQUIRE(p, FD_E_INVAL, name ": null parameter struct");                                                                   \
        long total__ = 0;                                                                                                            \
        FD_REQUIRE(anchor_params_ok(p, &total__), FD_E_INVAL, name ": bad fd_anchor_params (sizes >= 1, grid and wh finite and > 0, fewer than 2^28 anchors)"); \
        FD_REQUIRE(total__ == (long)p->num_anchors && (long)A == total__, FD_E_INVAL,                                                 \
                   name ": A=%d, num_anchors=%d, but the feature-map sizes give %ld anchors", A, p->num_anchors, total__);            \
    } while (0)

// ------------------------------------------------------------------------------------------------------ anchors
__global__ __launch_bounds__(256) void anchor_boxes_kernel(fd_anchor_params p, float4* __restrict__ out, int A) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < A) out[r] = anchor_row(p, r);
}

extern "C" int32_t fd_anchor_boxes(const fd_anchor_params* p, float* anchors, int32_t A, fd_stream_t stream) {
    FD_ANCHOR_CHECK_PARAMS("fd_anchor_boxes");
    FD_REQUIRE(anchors, FD_E_INVAL, "fd_anchor_boxes: null pointer");
    FD_REQUIRE(((uintptr_t)anchors & 15) == 0, FD_E_INVAL, "fd_anchor_boxes: anchors not 16-byte aligned");
    hipLaunchKernelGGL(anchor_boxes_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *p, (float4*)anchors, A);
    FD_CHECK_LAUNCH("fd_anchor_boxes");
    return FD_OK;
}

// ------------------------------------------------------------------------------------------------------ encode
// Block (x, b): 256 anchors of image b.  The image's valid boxes (label >= 0) are compacted in row order into LDS as the
// reference forms them: (centre, b - a + 1), then corners c -/+ wh/2 (half a pixel larger than the input) and the "+1" area.
__global__ __launch_bounds__(256) void anchor_encode_kernel(fd_anchor_params p, const float4* __restrict__ gt, const long long* __restrict__ labels,
                                                             int M, int A, float4* __restrict__ loc, long long* __restrict__ cls) {
    __shared__ float4 s_box[FD_ANCHOR_MAX_GT];     // x1, y1, x2, y2
    __shared__ float4 s_cw[FD_ANCHOR_MAX_GT];      // cx, cy, w, h
    __shared__ float s_area[FD_ANCHOR_MAX_GT];
    __shared__ long long s_label[FD_ANCHOR_MAX_GT];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y;
    long long lab = -1;
    if (tid < M) lab = labels[(long)b * M + tid];
    const bool valid = lab >= 0;
    const unsigned long long bal = __ballot(valid);
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int slot = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) slot += s_wave[w];
    const int n = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (valid) {
        const float4 g = gt[(long)b * M + tid];
        const float cx = (g.x + g.z) / 2.0f, cy = (g.y + g.w) / 2.0f;
        const float w = (g.z - g.x) + 1.0f, h = (g.w - g.y) + 1.0f;
        const float x1 = cx - w / 2.0f, y1 = cy - h / 2.0f, x2 = cx + w / 2.0f, y2 = cy + h / 2.0f;
        s_box[slot] = make_float4(x1, y1, x2, y2);
        s_cw[slot] = make_float4(cx, cy, w, h);
        s_area[slot] = ((x2 - x1) + 1.0f) * ((y2 - y1) + 1.0f);
        s_label[slot] = lab;
    }
    __syncthreads();
    const int r = blockIdx.x * 256 + tid;
    if (r >= A) return;
    const long o = (long)b * A + r;
    if (n == 0) {                                  // (the reference raises on an empty image)
        loc[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        cls[o] = 0;
        return;
    }
    const float4 a = anchor_row(p, r);
    const float ax1 = a.x - a.z / 2.0f, ay1 = a.y - a.w / 2.0f, ax2 = a.x + a.z / 2.0f, ay2 = a.y + a.w / 2.0f;
    const float a1 = ((ax2 - ax1) + 1.0f) * ((ay2 - ay1) + 1.0f);
    float best = 0.f;
    int bj = 0;
    for (int j = 0; j < n; ++j) {                  // every lane reads the same LDS address: a broadcast
        const float4 y = s_box[j];
        const float ltx = fmaxf(ax1, y.x), lty = fmaxf(ay1, y.y);
        const float rbx = fminf(ax2, y.z), rby = fminf(ay2, y.w);
        const float w = fmaxf((rbx - ltx) + 1.0f, 0.0f), h = fmaxf((rby - lty) + 1.0f, 0.0f);
        const float inter = w * h;
        const float iou = inter / ((a1 + s_area[j]) - inter);
        if (j == 0 || iou > best) { best = iou; bj = j; }      // first maximum (torch.max)
    }
    const float4 g = s_cw[bj];
    loc[o] = make_float4((g.x - a.x) / a.z, (g.y - a.y) / a.w, logf(g.z / a.z), logf(g.w / a.w));
    long long c = 1 + s_label[bj];
    if (best < 0.5f) c = 0;
    if (best > 0.4f && best < 0.5f) c = -1;
    cls[o] = c;
}

extern "C" int32_t fd_anchor_encode(const fd_anchor_params* p, const float* gt, const int64_t* labels, int32_t B, int32_t M, int32_t A,
                                    float* loc, int64_t* cls, fd_stream_t stream) {
    FD_ANCHOR_CHECK_PARAMS("fd_anchor_encode");
    FD_REQUIRE(loc && cls, FD_E_INVAL, "fd_anchor_encode: null output pointer");
    FD_REQUIRE(B >= 1 && B <= 65535, FD_E_INVAL, "fd_anchor_encode: B=%d outside 1 .. 65535", B);
    FD_REQUIRE(M >= 0, FD_E_INVAL, "fd_anchor_encode: M=%d < 0", M);
    FD_REQUIRE(M <= FD_ANCHOR_MAX_GT, FD_E_UNSUPPORTED, "fd_anchor_encode: M=%d > %d boxes per image not supported", M, FD_ANCHOR_MAX_GT);
    FD_REQUIRE(M == 0 || (gt && labels), FD_E_INVAL, "fd_anchor_encode: null gt / labels with M=%d", M);
    FD_REQUIRE((((uintptr_t)gt | (uintptr_t)loc) & 15) == 0 && (((uintptr_t)labels | (uintptr_t)cls) & 7) == 0, FD_E_INVAL,
               "fd_anchor_encode: gt / loc must be 16-byte aligned, labels / cls 8-byte");
    hipLaunchKernelGGL(anchor_encode_kernel, dim3((unsigned)((A + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, *p,
                       (const float4*)gt, (const long long*)labels, M, A, (float4*)loc, (long long*)cls);
    FD_CHECK_LAUNCH("fd_anchor_encode");
    return FD_OK;
}

// ------------------------------------------------------------------------------------------------------ decode
// G consecutive lanes share one anchor row; lane g takes units g, g + G, ... of it (a unit = a float4 of 4 classes when VEC,
// else one class), so a wave's load instruction covers 64 / G consecutive rows: one contiguous run of memory.  Each lane keeps
// the first maximum of its own sigmoid values; the xor-butterfly then prefers the larger value and, on equal values, the lower
// class index -- torch.max(1) over the sigmoid tensor (utills.py:175).  Lane 0 of the group writes score (0 unless > thr),
// label and box; candidates are counted with one atomic per wave.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void anchor_decode_kernel(fd_anchor_params p, const float4* __restrict__ loc, const float* __restrict__ cls, int A,
                                                             int C, float thr, float* __restrict__ scores, int* __restrict__ classes,
                                                             float4* __restrict__ boxes, int* __restrict__ n_cand) {
    const int tid = threadIdx.x;
    const int g = tid % G;
    const int r0 = blockIdx.x * (256 / G) + tid / G;
    const int b = blockIdx.y;
    const bool live = r0 < A;
    const int r = live ? r0 : A - 1;               // dead lanes shadow the last row: loads stay in range, shuffles stay whole
    const long o = (long)b * A + r;
    const float* row = cls + o * C;
    float best = -1.0f;
    int besti = 0x7fffffff;
    if (VEC) {
        const float4* row4 = reinterpret_cast<const float4*>(row);
        const int Q = C >> 2;
        for (int q = g; q < Q; q += G) {
            const float4 v = row4[q];
            const float s0 = fd_sigmoid(v.x), s1 = fd_sigmoid(v.y), s2 = fd_sigmoid(v.z), s3 = fd_sigmoid(v.w);
            if (s0 > best) { best = s0; besti = 4 * q; }
            if (s1 > best) { best = s1; besti = 4 * q + 1; }
            if (s2 > best) { best = s2; besti = 4 * q + 2; }
            if (s3 > best) { best = s3; besti = 4 * q + 3; }
        }
    } else {
        for (int c = g; c < C; c += G) {
            const float s = fd_sigmoid(row[c]);
            if (s > best) { best = s; besti = c; }
        }
    }
#pragma unroll
    for (int of = G >> 1; of > 0; of >>= 1) {
        const float ob = __shfl_xor(best, of);
        const int oi = __shfl_xor(besti, of);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    const bool writer = live && g == 0;
    const bool cand = writer && best > thr;
    const unsigned long long bal = __ballot(cand);
    if ((tid & 63) == 0 && bal) atomicAdd(&n_cand[b], (int)__popcll(bal));
    if (!writer) return;
    const float4 a = anchor_row(p, r);
    const float4 l = loc[o];
    const float x = l.x * a.z + a.x, y = l.y * a.w + a.y;
    const float w = expf(l.z) * a.z, h = expf(l.w) * a.w;
    scores[o] = cand ? best : 0.0f;
    classes[o] = besti == 0x7fffffff ? 0 : besti;          // (a row of NaNs: no maximum, score 0)
    boxes[o] = make_float4(x - w / 2.0f, y - h / 2.0f, x + w / 2.0f, y + h / 2.0f);
}

__global__ __launch_bounds__(256) void anchor_valid_kernel(const int* __restrict__ n_cand, int* __restrict__ n_valid, int B, int K) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) n_valid[b] = min(n_cand[b], K);
}

// rows kept by the NMS (keep = index into the K sorted candidates), padded with box 0 / label -1 / score 0
__global__ __launch_bounds__(256) void anchor_gather_kernel(const float4* __restrict__ top_boxes, const long long* __restrict__ top_classes,
                                                             const float* __restrict__ top_scores, const int* __restrict__ keep,
                                                             const int* __restrict__ counts, int K, float4* __restrict__ boxes,
                                                             long long* __restrict__ labels, float* __restrict__ scores) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= K) return;
    const long base = (long)b * K;
    const int k = keep[base + r];
    const bool ok = r < counts[b] && k >= 0 && k < K;
    boxes[base + r] = ok ? top_boxes[base + k] : make_float4(0.f, 0.f, 0.f, 0.f);
    labels[base + r] = ok ? top_classes[base + k] : -1ll;
    scores[base + r] = ok ? top_scores[base + k] : 0.0f;
}

struct AnchorDecodeLayout { long scores, classes, boxes, top_scores, top_classes, top_boxes, keep, n_valid, total; };
static long anchor_up256(long v) { return (v + 255) & ~255l; }
static AnchorDecodeLayout anchor_decode_layout(long B, long A, long K) {
    AnchorDecodeLayout l;
    long o = 0;
    l.scores = o;      o += anchor_up256(B * A * 4);
    l.classes = o;     o += anchor_up256(B * A * 4);
    l.boxes = o;       o += anchor_up256(B * A * 16);
    l.top_scores = o;  o += anchor_up256(B * K * 4);
    l.top_classes = o; o += anchor_up256(B * K * 8);
    l.top_boxes = o;   o += anchor_up256(B * K * 16);
    l.keep = o;        o += anchor_up256(B * K * 4);
    l.n_valid = o;     o += anchor_up256(B * 4);
    l.total = o;
    return l;
}

extern "C" int64_t fd_anchor_decode_workspace_bytes(int32_t B, int32_t A, int32_t max_candidates) {
    if (B < 1 || B > 65535 || A < 1 || A >= (1 << 28) || max_candidates < 1 || max_candidates > FD_ANCHOR_MAX_CAND) return -1;
    return anchor_decode_layout(B, A, max_candidates < A ? max_candidates : A).total;
}

template <int G, bool VEC>
static void anchor_decode_launch(const fd_anchor_params* p, const float* loc, const float* cls, int B, int A, int C, float thr, float* scores,
                                 int* classes, float* boxes, int* n_cand, hipStream_t st) {
    constexpr int rows = 256 / G;
    hipLaunchKernelGGL((anchor_decode_kernel<G, VEC>), dim3((unsigned)((A + rows - 1) / rows), (unsigned)B), dim3(256), 0, st, *p,
                       (const float4*)loc, cls, A, C, thr, scores, classes, (float4*)boxes, n_cand);
}

extern "C" int32_t fd_anchor_decode(const fd_anchor_params* p, const float* loc, const float* cls, int32_t B, int32_t A, int32_t C,
                                    float cls_thresh, float nms_thresh, int32_t max_candidates, float* boxes, int64_t* labels,
                                    float* scores, int32_t* counts, int32_t* n_candidates, void* workspace, fd_stream_t stream) {
    FD_ANCHOR_CHECK_PARAMS("fd_anchor_decode");
    FD_REQUIRE(loc && cls && boxes && labels && scores && counts && n_candidates && workspace, FD_E_INVAL, "fd_anchor_decode: null pointer");
    FD_REQUIRE(B >= 1 && B <= 65535, FD_E_INVAL, "fd_anchor_decode: B=%d outside 1 .. 65535", B);
    FD_REQUIRE(C >= 1, FD_E_INVAL, "fd_anchor_decode: C=%d < 1", C);
    FD_REQUIRE(C <= FD_ANCHOR_MAX_CLASSES, FD_E_UNSUPPORTED, "fd_anchor_decode: C=%d > %d classes not supported", C, FD_ANCHOR_MAX_CLASSES);
    FD_REQUIRE(max_candidates >= 1, FD_E_INVAL, "fd_anchor_decode: max_candidates=%d < 1", max_candidates);
    FD_REQUIRE(max_candidates <= FD_ANCHOR_MAX_CAND, FD_E_UNSUPPORTED, "fd_anchor_decode: max_candidates=%d > %d not supported", max_candidates,
               FD_ANCHOR_MAX_CAND);
    FD_REQUIRE(cls_thresh >= 0.f && cls_thresh < 1.f && nms_thresh >= 0.f, FD_E_INVAL,
               "fd_anchor_decode: cls_thresh must be in [0, 1) and nms_thresh >= 0 (a score of 0 marks a non-candidate)");
    FD_REQUIRE((((uintptr_t)loc | (uintptr_t)boxes) & 15) == 0 && ((uintptr_t)cls & 3) == 0 && ((uintptr_t)labels & 7) == 0 &&
               ((uintptr_t)workspace & 255) == 0, FD_E_INVAL,
               "fd_anchor_decode: loc / boxes must be 16-byte aligned, labels 8-byte, the workspace 256-byte");
    const int K = max_candidates < A ? max_candidates : A;
    const AnchorDecodeLayout lay = anchor_decode_layout(B, A, K);
    char* ws = (char*)workspace;
    float* d_scores = (float*)(ws + lay.scores);
    int* d_classes = (int*)(ws + lay.classes);
    float* d_boxes = (float*)(ws + lay.boxes);
    float* t_scores = (float*)(ws + lay.top_scores);
    int64_t* t_classes = (int64_t*)(ws + lay.top_classes);
    float* t_boxes = (float*)(ws + lay.top_boxes);
    int* keep = (int*)(ws + lay.keep);
    int* n_valid = (int*)(ws + lay.n_valid);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n_candidates, 0, (size_t)B * 4, st) != hipSuccess) {
        fd_set_error("fd_anchor_decode: hipMemsetAsync failed");
        return FD_E_LAUNCH;
    }
    const bool vec = (C & 3) == 0 && ((uintptr_t)cls & 15) == 0;
    const int units = vec ? C / 4 : C;
    // G = the power of two >= units, at most 32 (C = 128 scalar: four units per lane)
#define FD_ANCHOR_GO(G_)                                                                                                          \
    do {                                                                                                                          \
        if (vec) anchor_decode_launch<G_, true>(p, loc, cls, B, A, C, cls_thresh, d_scores, d_classes, d_boxes, n_candidates, st); \
        else anchor_decode_launch<G_, false>(p, loc, cls, B, A, C, cls_thresh, d_scores, d_classes, d_boxes, n_candidates, st);    \
    } while (0)
    if (units <= 1) FD_ANCHOR_GO(1);
    else if (units <= 2) FD_ANCHOR_GO(2);
    else if (units <= 4) FD_ANCHOR_GO(4);
    else if (units <= 8) FD_ANCHOR_GO(8);
    else if (units <= 16) FD_ANCHOR_GO(16);
    else FD_ANCHOR_GO(32);
#undef FD_ANCHOR_GO
    FD_CHECK_LAUNCH("fd_anchor_decode (scores)");
    int32_t rc = fd_fcos_topk(d_scores, d_classes, d_boxes, B, A, K, t_scores, t_classes, t_boxes, nullptr, nullptr, stream);
    if (rc != FD_OK) return rc;
    hipLaunchKernelGGL(anchor_valid_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, n_candidates, n_valid, B, K);
    FD_CHECK_LAUNCH("fd_anchor_decode (valid rows)");
    rc = fd_box_nms_plus1(t_boxes, t_scores, n_valid, B, K, nms_thresh, 0, keep, counts, stream);
    if (rc != FD_OK) return rc;
    hipLaunchKernelGGL(anchor_gather_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)B), dim3(256), 0, st, (const float4*)t_boxes,
                       (const long long*)t_classes, t_scores, keep, counts, K, (float4*)boxes, (long long*)labels, scores);
    FD_CHECK_LAUNCH("fd_anchor_decode (gather)");
    return FD_OK;
}
