// fd_eval.hip — VOC average precision on the device: the arithmetic of the reference's evaluation
// (test.py:15-20 sort_by_score, 23-53 iou_2d, 56-82 _compute_ap, 85-162 eval_ap_2d, 225-238 evaluate).  The second half of
// the file is COCO bbox evaluation (fd_eval_coco), which reuses the count / scan / radix-sort kernels of the first.
//
//   count    one wave per image: detections with a label in 1 .. num_cls-1 (rows < det_counts)
//   scan     one workgroup: exclusive scan of those counts = each image's output offset; zeroes the counters
//   match    one workgroup per image: detections and GT rows ranked in LDS by (label, score desc, row); one wave per label
//            walks the label's detections in score order, lanes across the label's GT boxes (fp32 IoU, first-max / first-NaN
//            argmax), one "assigned" bit per (GT box, threshold); writes (key = label:score, value = TP bitmask) per detection
//   hist     digit histograms of the 39-bit keys (5 passes of 8 bits), LDS-privatised
//   plan     digit bases per pass; a pass whose digit is constant over the input is skipped (its launches return at once)
//   5 x (blkcount, blkscan, scatter)   stable LSD radix sort: per tile digit counts, a scan across tiles per digit, a
//            stable scatter (ballot peer ranks in (tile, wave, lane) order)
//   ap       one workgroup per label, the thresholds in turn: TP positions compacted with their running precision, a
//            right-to-left max (the precision envelope), and one lane sums the change-point terms in numpy's pairwise order.
//
// Compiled with -ffp-contract=off (Makefile): every IoU, recall, precision and AP term is one IEEE operation in the
// reference's order, so the per-label AP is bit-identical to numpy on inputs without exactly equal scores.
#include "fd_common.h"

#define EV_MAXK 1024
#define EV_MAXG 512
#define EV_MAXCLS 128
#define EV_MAXTHR 16
#define EV_THREADS 256
#define EV_TILE 1024          // entries per radix-sort tile (EV_THREADS x 4)
#define EV_PASSES 5           // 39-bit key: label (7 bits) above the 32-bit descending score key

struct EvThr {
    float t[EV_MAXTHR];
};

struct EvLayout {
    size_t offs, keys0, keys1, vals0, vals1, blk, hist, ctl, total;
    long emax, nb;
};

static inline size_t ev_align(size_t v) { return (v + 255) & ~(size_t)255; }

static EvLayout ev_layout(int N, int K) {
    EvLayout L;
    L.emax = (long)N * K;
    L.nb = (L.emax + EV_TILE - 1) / EV_TILE;
    size_t o = 0;
    L.offs = o;  o = ev_align(o + (size_t)(N + 1) * 4);
    L.keys0 = o; o = ev_align(o + (size_t)L.emax * 8);
    L.keys1 = o; o = ev_align(o + (size_t)L.emax * 8);
    L.vals0 = o; o = ev_align(o + (size_t)L.emax * 4);
    L.vals1 = o; o = ev_align(o + (size_t)L.emax * 4);
    L.blk = o;   o = ev_align(o + (size_t)L.nb * 256 * 4);
    L.hist = o;  o = ev_align(o + (size_t)EV_PASSES * 256 * 4);
    L.ctl = o;   o = ev_align(o + 16 * 4);
    L.total = o;
    return L;
}

// ctl words: [0, 5) skip flag per pass, [5, 11) input buffer of pass p (sel[5] = buffer holding the sorted result)
#define EV_CTL_SKIP 0
#define EV_CTL_SEL 5

// Descending-orderable key of an fp32 score: larger score -> smaller key; -0 == +0; NaN last (numpy's argsort puts NaN at the end)
__device__ __forceinline__ unsigned ev_desc_key(float s) {
    if (s != s) return 0xFFFFFFFFu;
    if (s == 0.0f) s = 0.0f;
    const unsigned u = __float_as_uint(s);
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}

// np.minimum / np.maximum: a NaN operand gives NaN (fminf / fmaxf would return the other operand)
__device__ __forceinline__ float ev_min(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
__device__ __forceinline__ float ev_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

// iou_2d (test.py:23-53) of one GT box against one prediction, fp32, no "+1": the reference's operation order; a NaN coordinate
// gives a NaN IoU, as there
__device__ __forceinline__ float ev_iou(const float4 g, const float4 d) {
    const float w = ev_max(0.0f, ev_min(g.z, d.z) - ev_max(g.x, d.x));
    const float h = ev_max(0.0f, ev_min(g.w, d.w) - ev_max(g.y, d.y));
    const float overlap = w * h;
    const float area_g = (g.z - g.x) * (g.w - g.y);
    const float area_d = (d.z - d.x) * (d.w - d.y);
    return overlap / ((area_g + area_d) - overlap);
}

// np.argmax order: does candidate (v, i) beat the current best (b, j)?  NaN beats any number, the first NaN / first max wins;
// index EV_NONE (a lane without a GT box) loses to everything
#define EV_NONE 0x7FFFFFFF
__device__ __forceinline__ bool ev_beats(float v, int i, float b, int j) {
    if (i == EV_NONE) return false;
    if (j == EV_NONE) return true;
    const bool vn = v != v, bn = b != b;
    if (vn || bn) return vn && (!bn || i < j);
    return v > b || (v == b && i < j);
}

__device__ __forceinline__ int ev_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ unsigned long long ev_lt_mask() { return (1ull << ev_lane()) - 1ull; }

// exclusive scan over the 256 threads of a workgroup; `sh` holds 4 words; every thread must call it
__device__ __forceinline__ unsigned ev_block_excl_scan(unsigned v, unsigned* sh, unsigned& total) {
    const int lane = ev_lane(), w = threadIdx.x >> 6;
    unsigned x = v;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    unsigned pre = 0;
    for (int i = 0; i < w; ++i) pre += sh[i];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return pre + x - v;
}

// ---------------------------------------------------------------------------------------------------------------
// count: valid detections per image (one wave per image)
__global__ __launch_bounds__(64) void ev_count_kernel(const int64_t* __restrict__ det_classes, const int32_t* __restrict__ det_counts,
                                                      int K, int num_cls, int* __restrict__ img_cnt) {
    const long img = blockIdx.x;
    int c = det_counts ? det_counts[img] : K;
    c = max(0, min(c, K));
    unsigned n = 0;
    for (int i = threadIdx.x; i < K; i += 64) {
        const int64_t l = det_classes[img * K + i];
        n += (i < c && l >= 1 && l < num_cls) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (threadIdx.x == 0) img_cnt[img] = (int)n;
}

// scan: image offsets (offs[N] = number of entries); zeroes the histogram and the per-label counters
__global__ __launch_bounds__(EV_THREADS) void ev_scan_kernel(int N, int num_cls, int* __restrict__ offs, unsigned* __restrict__ hist,
                                                             int32_t* __restrict__ n_gt, int32_t* __restrict__ n_pred) {
    __shared__ unsigned sh[4];
    const int tid = threadIdx.x;
    for (int i = tid; i < EV_PASSES * 256; i += EV_THREADS) hist[i] = 0u;
    for (int i = tid; i < num_cls; i += EV_THREADS) {
        n_gt[i] = 0;
        n_pred[i] = 0;
    }
    unsigned carry = 0;
    for (int base = 0; base < N; base += EV_THREADS) {
        const int i = base + tid;
        const unsigned v = i < N ? (unsigned)offs[i] : 0u;
        unsigned total;
        const unsigned ex = ev_block_excl_scan(v, sh, total);
        if (i < N) offs[i] = (int)(carry + ex);
        carry += total;
    }
    if (tid == 0) offs[N] = (int)carry;
}

// ---------------------------------------------------------------------------------------------------------------
// match: one workgroup per image
struct EvMatchSh {
    unsigned long long dkey[EV_MAXK];   // (label << 42) | (descending score key << 10) | row; ~0 = not taking part
    float4 dbox[EV_MAXK];               // by row
    unsigned short dperm[EV_MAXK];      // rank -> row
    unsigned short dmask[EV_MAXK];      // rank -> TP bitmask over thresholds
    float4 gbox[EV_MAXG];               // by row
    unsigned gkey[EV_MAXG];             // (label << 9) | row; ~0 = not taking part
    unsigned short gperm[EV_MAXG];      // rank -> row
    unsigned short taken[EV_MAXG];      // rank -> assigned bit per threshold
    unsigned short dstart[EV_MAXCLS], dend[EV_MAXCLS], gstart[EV_MAXCLS], gend[EV_MAXCLS];
};

__global__ __launch_bounds__(EV_THREADS) void ev_match_kernel(
    const float* __restrict__ det_scores, const int64_t* __restrict__ det_classes, const float* __restrict__ det_boxes,
    const int32_t* __restrict__ det_counts, int K, const float* __restrict__ gt_boxes, const int64_t* __restrict__ gt_classes,
    const int32_t* __restrict__ gt_counts, int G, int num_cls, EvThr thr, int n_thr, int input_order, const int* __restrict__ offs,
    unsigned long long* __restrict__ out_keys, unsigned* __restrict__ out_vals, int32_t* __restrict__ n_gt, int32_t* __restrict__ n_pred) {
    __shared__ EvMatchSh sh;
    const int tid = threadIdx.x;
    const long img = blockIdx.x;
    const int off = offs[img], nd = offs[img + 1] - off;
    int c = det_counts ? det_counts[img] : K;
    c = max(0, min(c, K));
    int gc = gt_counts ? gt_counts[img] : G;
    gc = max(0, min(gc, G));

    for (int l = tid; l < EV_MAXCLS; l += EV_THREADS) sh.dstart[l] = sh.dend[l] = sh.gstart[l] = sh.gend[l] = 0;
    for (int i = tid; i < K; i += EV_THREADS) {
        const int64_t l = det_classes[img * K + i];
        unsigned long long key = ~0ull;
        if (i < c && l >= 1 && l < num_cls) {
            const unsigned sk = input_order ? 0u : ev_desc_key(det_scores[img * K + i]);
            key = ((unsigned long long)l << 42) | ((unsigned long long)sk << 10) | (unsigned long long)i;
            sh.dbox[i] = reinterpret_cast<const float4*>(det_boxes)[img * K + i];
        }
        sh.dkey[i] = key;
    }
    int ng = 0;
    for (int base = 0; base < G; base += EV_THREADS) {
        const int g = base + tid;
        bool valid = false;
        if (g < G) {
            const int64_t l = gt_classes[img * G + g];
            valid = g < gc && l >= 1 && l < num_cls;
            sh.gkey[g] = valid ? (((unsigned)l << 9) | (unsigned)g) : ~0u;
            if (valid) sh.gbox[g] = reinterpret_cast<const float4*>(gt_boxes)[img * G + g];
            sh.taken[g] = 0;
        }
        ng += __syncthreads_count(valid);
    }
    __syncthreads();

    // rank = number of smaller keys (keys are unique: the row is part of them)
    for (int i0 = tid; i0 < K; i0 += 4 * EV_THREADS) {
        unsigned long long k4[4];
        int r4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; ++u) k4[u] = (i0 + u * EV_THREADS < K) ? sh.dkey[i0 + u * EV_THREADS] : ~0ull;
        for (int j = 0; j < K; ++j) {
            const unsigned long long kj = sh.dkey[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) r4[u] += kj < k4[u] ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k4[u] != ~0ull) sh.dperm[r4[u]] = (unsigned short)(i0 + u * EV_THREADS);
    }
    for (int g = tid; g < G; g += EV_THREADS) {
        const unsigned kg = sh.gkey[g];
        if (kg == ~0u) continue;
        int r = 0;
        for (int j = 0; j < G; ++j) r += sh.gkey[j] < kg ? 1 : 0;
        sh.gperm[r] = (unsigned short)g;
    }
    __syncthreads();

    // label ranges, the output keys (label above the descending score key) and the label counters
    for (int p = tid; p < nd; p += EV_THREADS) {
        const int row = sh.dperm[p];
        const int l = (int)(sh.dkey[row] >> 42);
        if (p == 0 || (int)(sh.dkey[sh.dperm[p - 1]] >> 42) != l) sh.dstart[l] = (unsigned short)p;
        if (p == nd - 1 || (int)(sh.dkey[sh.dperm[p + 1]] >> 42) != l) sh.dend[l] = (unsigned short)(p + 1);
        out_keys[off + p] = ((unsigned long long)l << 32) | ev_desc_key(det_scores[img * K + row]);
        sh.dmask[p] = 0;
    }
    for (int p = tid; p < ng; p += EV_THREADS) {
        const int l = (int)(sh.gkey[sh.gperm[p]] >> 9);
        if (p == 0 || (int)(sh.gkey[sh.gperm[p - 1]] >> 9) != l) sh.gstart[l] = (unsigned short)p;
        if (p == ng - 1 || (int)(sh.gkey[sh.gperm[p + 1]] >> 9) != l) sh.gend[l] = (unsigned short)(p + 1);
    }
    __syncthreads();
    for (int l = 1 + tid; l < num_cls; l += EV_THREADS) {
        if (sh.dend[l] > sh.dstart[l]) atomicAdd(&n_pred[l], (int)(sh.dend[l] - sh.dstart[l]));
        if (sh.gend[l] > sh.gstart[l]) atomicAdd(&n_gt[l], (int)(sh.gend[l] - sh.gstart[l]));
    }

    // greedy matching, one wave per label: detections in rank order, lanes across the label's GT boxes (row order)
    const int wave = tid >> 6, lane = ev_lane();
    for (int l = 1 + wave; l < num_cls; l += EV_THREADS / 64) {
        const int ds = sh.dstart[l], de = sh.dend[l], gs = sh.gstart[l], ge = sh.gend[l];
        if (ds == de || gs == ge) continue;    // no GT of this label in the image: every detection is a false positive
        for (int p = ds; p < de; ++p) {
            const float4 d = sh.dbox[sh.dperm[p]];
            float best = 0.0f;
            int bi = EV_NONE;
            for (int q = gs + lane; q < ge; q += 64) {
                const float v = ev_iou(sh.gbox[sh.gperm[q]], d);
                if (ev_beats(v, q, best, bi)) {
                    best = v;
                    bi = q;
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o);
                const int oi = __shfl_xor(bi, o);
                if (ev_beats(ov, oi, best, bi)) {
                    best = ov;
                    bi = oi;
                }
            }
            if (lane == 0) {
                const unsigned tk = sh.taken[bi];
                unsigned m = 0;
#pragma unroll
                for (int t = 0; t < EV_MAXTHR; ++t)
                    if (t < n_thr && best >= thr.t[t] && !((tk >> t) & 1u)) m |= 1u << t;    // taken GT box: false positive, no fall-back
                sh.taken[bi] = (unsigned short)(tk | m);
                sh.dmask[p] = (unsigned short)m;
            }
        }
    }
    __syncthreads();
    for (int p = tid; p < nd; p += EV_THREADS) out_vals[off + p] = sh.dmask[p];
}

// ---------------------------------------------------------------------------------------------------------------
// radix sort of (key, value) pairs: LSD, 8-bit digits, stable
__global__ __launch_bounds__(EV_THREADS) void ev_hist_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ offs, int N,
                                                             unsigned* __restrict__ hist) {
    __shared__ unsigned h[EV_PASSES * 256];
    const int E = offs[N];
    const long base = (long)blockIdx.x * EV_TILE;
    if (base >= E) return;
    for (int i = threadIdx.x; i < EV_PASSES * 256; i += EV_THREADS) h[i] = 0u;
    __syncthreads();
    for (int r = 0; r < EV_TILE / EV_THREADS; ++r) {
        const long idx = base + r * EV_THREADS + threadIdx.x;
        if (idx < E) {
            const unsigned long long k = keys[idx];
            for (int p = 0; p < EV_PASSES; ++p) atomicAdd(&h[p * 256 + (int)((k >> (8 * p)) & 255u)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < EV_PASSES * 256; i += EV_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// digit bases per pass (in place over the histogram), skip flags, and which buffer each pass reads
__global__ __launch_bounds__(64) void ev_plan_kernel(const int* __restrict__ offs, int N, unsigned* __restrict__ hist, int* __restrict__ ctl) {
    const unsigned E = (unsigned)offs[N];
    const int p = threadIdx.x;
    if (p < EV_PASSES) {
        unsigned s = 0;
        int skip = 0;
        for (int d = 0; d < 256; ++d) {
            const unsigned v = hist[p * 256 + d];
            if (v == E) skip = 1;                 // one digit value holds every entry (E == 0 included)
            hist[p * 256 + d] = s;
            s += v;
        }
        ctl[EV_CTL_SKIP + p] = skip;
    }
    __syncthreads();
    if (p == 0) {
        int sel = 0;
        for (int q = 0; q < EV_PASSES; ++q) {
            ctl[EV_CTL_SEL + q] = sel;
            if (!ctl[EV_CTL_SKIP + q]) sel ^= 1;
        }
        ctl[EV_CTL_SEL + EV_PASSES] = sel;
    }
}

// peers of this lane (same digit, valid) within the wave, and its rank among them
__device__ __forceinline__ unsigned long long ev_peers(unsigned d, bool valid) {
    unsigned long long m = __ballot(valid);
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

__global__ __launch_bounds__(EV_THREADS) void ev_blkcount_kernel(const unsigned long long* __restrict__ keys0, const unsigned long long* __restrict__ keys1,
                                                                 const int* __restrict__ offs, int N, const int* __restrict__ ctl, int pass,
                                                                 unsigned* __restrict__ blk) {
    __shared__ unsigned h[256];
    if (ctl[EV_CTL_SKIP + pass]) return;
    const int E = offs[N];
    const long base = (long)blockIdx.x * EV_TILE;
    if (base >= E) return;
    const unsigned long long* keys = ctl[EV_CTL_SEL + pass] ? keys1 : keys0;
    h[threadIdx.x] = 0u;
    __syncthreads();
    for (int r = 0; r < EV_TILE / EV_THREADS; ++r) {
        const long idx = base + r * EV_THREADS + threadIdx.x;
        const bool valid = idx < E;
        const unsigned d = valid ? (unsigned)((keys[idx] >> (8 * pass)) & 255u) : 0u;
        const unsigned long long peers = ev_peers(d, valid);
        if (valid && (peers & ev_lt_mask()) == 0ull) atomicAdd(&h[d], (unsigned)__popcll(peers));
    }
    __syncthreads();
    blk[(long)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// per digit (one workgroup each): exclusive scan over the tiles, plus the digit's base
__global__ __launch_bounds__(EV_THREADS) void ev_blkscan_kernel(const int* __restrict__ offs, int N, const int* __restrict__ ctl, int pass,
                                                                const unsigned* __restrict__ hist, unsigned* __restrict__ blk) {
    __shared__ unsigned sh[4];
    if (ctl[EV_CTL_SKIP + pass]) return;
    const int E = offs[N];
    const long nb = ((long)E + EV_TILE - 1) / EV_TILE;
    const int d = blockIdx.x;
    unsigned carry = hist[pass * 256 + d];
    for (long b0 = 0; b0 < nb; b0 += EV_THREADS) {
        const long b = b0 + threadIdx.x;
        const unsigned v = b < nb ? blk[b * 256 + d] : 0u;
        unsigned total;
        const unsigned ex = ev_block_excl_scan(v, sh, total);
        if (b < nb) blk[b * 256 + d] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(EV_THREADS) void ev_scatter_kernel(unsigned long long* __restrict__ keys0, unsigned long long* __restrict__ keys1,
                                                                unsigned* __restrict__ vals0, unsigned* __restrict__ vals1,
                                                                const int* __restrict__ offs, int N, const int* __restrict__ ctl, int pass,
                                                                const unsigned* __restrict__ blk) {
    __shared__ unsigned wcnt[EV_THREADS / 64][256];
    __shared__ unsigned run[256], boff[256];
    if (ctl[EV_CTL_SKIP + pass]) return;
    const int E = offs[N];
    const long base = (long)blockIdx.x * EV_TILE;
    if (base >= E) return;
    const bool from1 = ctl[EV_CTL_SEL + pass] != 0;
    const unsigned long long* ik = from1 ? keys1 : keys0;
    const unsigned* iv = from1 ? vals1 : vals0;
    unsigned long long* ok = from1 ? keys0 : keys1;
    unsigned* ov = from1 ? vals0 : vals1;
    const int tid = threadIdx.x, w = tid >> 6;
    run[tid] = 0u;
    boff[tid] = blk[(long)blockIdx.x * 256 + tid];
    for (int r = 0; r < EV_TILE / EV_THREADS; ++r) {     // tile order = (r, wave, lane): ranks keep input order
        for (int q = 0; q < EV_THREADS / 64; ++q) wcnt[q][tid] = 0u;
        __syncthreads();
        const long idx = base + r * EV_THREADS + tid;
        const bool valid = idx < E;
        unsigned long long k = 0ull;
        unsigned v = 0u;
        if (valid) {
            k = ik[idx];
            v = iv[idx];
        }
        const unsigned d = (unsigned)((k >> (8 * pass)) & 255u);
        const unsigned long long peers = ev_peers(d, valid);
        const unsigned lr = (unsigned)__popcll(peers & ev_lt_mask());
        if (valid && lr == 0u) wcnt[w][d] = (unsigned)__popcll(peers);
        __syncthreads();
        unsigned s = run[tid];
        for (int q = 0; q < EV_THREADS / 64; ++q) {
            const unsigned c = wcnt[q][tid];
            wcnt[q][tid] = s;
            s += c;
        }
        run[tid] = s;
        __syncthreads();
        if (valid) {
            const unsigned pos = boff[d] + wcnt[w][d] + lr;
            ok[pos] = k;
            ov[pos] = v;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// AP: one workgroup per label
#define EV_PW_BLOCK 128
#define EV_PW_STACK 40

struct EvTerms {
    const double* q;     // suffix-max precision at the j-th TP
    double g;            // total GT boxes of the label
    int ntp;
    __device__ __forceinline__ double operator()(long j) const {
        if (j < ntp) return ((double)(j + 1) / g - (double)j / g) * q[j];      // (mrec[i+1] - mrec[i]) * mpre[i+1] at a recall step
        return (1.0 - (double)ntp / g) * 0.0;                                  // the closing step to the sentinel recall 1, precision 0
    }
};

// numpy's pairwise_sum (float64): < 8 terms in order; <= 128 terms in 8 accumulators folded ((0+1)+(2+3))+((4+5)+(6+7)), then the
// remainder in order; above that the halves at n/2 rounded down to a multiple of 8
__device__ double ev_pw_leaf(const EvTerms& T, long a, long n) {
    if (n < 8) {
        double res = 0.0;
        for (long i = 0; i < n; ++i) res += T(a + i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = T(a + k);
    long i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += T(a + i + k);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += T(a + i);
    return res;
}

struct EvPwStack {
    long start[EV_PW_STACK], len[EV_PW_STACK];
    double left[EV_PW_STACK];
    int stage[EV_PW_STACK];
};

__device__ double ev_pairwise(const EvTerms& T, long n, EvPwStack& st) {
    if (n <= EV_PW_BLOCK) return ev_pw_leaf(T, 0, n);
    int sp = 0;
    st.start[0] = 0;
    st.len[0] = n;
    st.stage[0] = 0;
    sp = 1;
    double ret = 0.0;
    while (sp > 0) {
        const int f = sp - 1;
        const long a = st.start[f], m = st.len[f];
        if (m <= EV_PW_BLOCK) {
            ret = ev_pw_leaf(T, a, m);
            --sp;
            continue;
        }
        long n2 = m / 2;
        n2 -= n2 % 8;
        if (st.stage[f] == 0) {
            st.stage[f] = 1;
            st.start[sp] = a;
            st.len[sp] = n2;
            st.stage[sp] = 0;
            ++sp;
        } else if (st.stage[f] == 1) {
            st.left[f] = ret;
            st.stage[f] = 2;
            st.start[sp] = a + n2;
            st.len[sp] = m - n2;
            st.stage[sp] = 0;
            ++sp;
        } else {
            ret = st.left[f] + ret;
            --sp;
        }
    }
    return ret;
}

__global__ __launch_bounds__(EV_THREADS) void ev_ap_kernel(const unsigned* __restrict__ vals0, const unsigned* __restrict__ vals1,
                                                           const int* __restrict__ ctl, int num_cls, int n_thr, const int32_t* __restrict__ n_gt,
                                                           const int32_t* __restrict__ n_pred, double* __restrict__ qbuf, double* __restrict__ ap,
                                                           int32_t* __restrict__ n_tp) {
    __shared__ unsigned shc[4];
    __shared__ double shd[4];
    __shared__ EvPwStack stk;
    const int l = blockIdx.x, tid = threadIdx.x, lane = ev_lane(), w = tid >> 6;
    if (l == 0) {
        for (int t = tid; t < n_thr; t += EV_THREADS) {
            ap[(long)t * num_cls] = 0.0;
            n_tp[(long)t * num_cls] = 0;
        }
        return;
    }
    long seg = 0;
    for (int i = 1; i < l; ++i) seg += n_pred[i];
    const int n = n_pred[l], g = n_gt[l];
    const unsigned* vals = (ctl[EV_CTL_SEL + EV_PASSES] ? vals1 : vals0) + seg;
    double* q = qbuf + seg;
    for (int t = 0; t < n_thr; ++t) {
        // TP positions k_j in score order, stored as the running precision there: tp / (tp + fp) = (j + 1) / (k_j + 1)
        unsigned carry = 0;
        for (long c = 0; c < n; c += EV_THREADS) {
            const long k = c + tid;
            const bool bit = k < n && ((vals[k] >> t) & 1u);
            const unsigned long long m = __ballot(bit);
            if (lane == 0) shc[w] = (unsigned)__popcll(m);
            __syncthreads();
            unsigned pre = carry;
            for (int i = 0; i < w; ++i) pre += shc[i];
            const unsigned tot = shc[0] + shc[1] + shc[2] + shc[3];
            if (bit) {
                const unsigned j = pre + (unsigned)__popcll(m & ev_lt_mask());
                q[j] = (double)(j + 1) / (double)(k + 1);
            }
            carry += tot;
            __syncthreads();
        }
        const int ntp = (int)carry;
        // precision envelope: running max from the right (the FP rows between TPs and the sentinel only lower it)
        double cm = 0.0;
        for (long c = ((long)(ntp - 1) / EV_THREADS) * EV_THREADS; ntp > 0 && c >= 0; c -= EV_THREADS) {
            const long j = c + tid;
            double x = j < ntp ? q[j] : 0.0;
            for (int o = 1; o < 64; o <<= 1) {
                const double y = __shfl_down(x, o);
                if (lane + o < 64) x = fmax(x, y);
            }
            if (lane == 0) shd[w] = x;
            __syncthreads();
            double add = cm;
            for (int i = w + 1; i < 4; ++i) add = fmax(add, shd[i]);
            x = fmax(x, add);
            if (j < ntp) q[j] = x;
            cm = fmax(cm, fmax(fmax(shd[0], shd[1]), fmax(shd[2], shd[3])));
            __syncthreads();
        }
        __threadfence_block();
        __syncthreads();
        if (tid == 0) {
            double a;
            if (g == 0) {
                a = n > 0 ? __longlong_as_double(0x7FF8000000000000ll) : 0.0;   // recall 0/0: NaN; no rows at all: 0
            } else {
                EvTerms T{q, (double)g, ntp};
                const bool closing = (double)ntp / (double)g != 1.0;
                a = 0.0 + ev_pairwise(T, (long)ntp + (closing ? 1 : 0), stk);
            }
            ap[(long)t * num_cls + l] = a;
            n_tp[(long)t * num_cls + l] = ntp;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
static int ev_args_ok(int32_t N, int32_t K, int32_t G, int32_t num_cls, int32_t n_thr) {
    if (N < 1 || K < 0 || G < 0 || num_cls < 2 || n_thr < 1) {
        fd_set_error("fd_eval_ap: bad sizes N=%d K=%d G=%d num_cls=%d n_thr=%d", N, K, G, num_cls, n_thr);
        return FD_E_INVAL;
    }
    if (K > EV_MAXK || G > EV_MAXG || num_cls > EV_MAXCLS || n_thr > EV_MAXTHR) {
        fd_set_error("fd_eval_ap: limits are K <= %d detections and G <= %d GT boxes per image, num_cls <= %d, n_thr <= %d "
                     "(got K=%d G=%d num_cls=%d n_thr=%d)", EV_MAXK, EV_MAXG, EV_MAXCLS, EV_MAXTHR, K, G, num_cls, n_thr);
        return FD_E_UNSUPPORTED;
    }
    if ((long)N * K > 0x7FFFFFFFl - EV_TILE) {
        fd_set_error("fd_eval_ap: N * K = %ld detection rows exceeds 2^31", (long)N * K);
        return FD_E_UNSUPPORTED;
    }
    return FD_OK;
}

extern "C" int64_t fd_eval_ap_workspace_bytes(int32_t N, int32_t K, int32_t G, int32_t num_cls, int32_t n_thr) {
    if (ev_args_ok(N, K, G, num_cls, n_thr) != FD_OK) return -1;
    return (int64_t)ev_layout(N, K).total;
}

extern "C" int32_t fd_eval_ap(const float* det_scores, const int64_t* det_classes, const float* det_boxes, const int32_t* det_counts,
                              int32_t N, int32_t K, const float* gt_boxes, const int64_t* gt_classes, const int32_t* gt_counts, int32_t G,
                              int32_t num_cls, const float* thresholds, int32_t n_thr, int32_t flags, double* ap, int32_t* n_gt,
                              int32_t* n_pred, int32_t* n_tp, void* workspace, fd_stream_t stream) {
    const int rc = ev_args_ok(N, K, G, num_cls, n_thr);
    if (rc != FD_OK) return rc;
    FD_REQUIRE(thresholds && ap && n_gt && n_pred && n_tp && workspace, FD_E_INVAL, "fd_eval_ap: null pointer");
    FD_REQUIRE(K == 0 || (det_scores && det_classes && det_boxes), FD_E_INVAL, "fd_eval_ap: null detection pointer");
    FD_REQUIRE(G == 0 || (gt_boxes && gt_classes), FD_E_INVAL, "fd_eval_ap: null GT pointer");
    FD_REQUIRE((((uintptr_t)det_boxes | (uintptr_t)gt_boxes) & 15) == 0, FD_E_INVAL, "fd_eval_ap: boxes not 16-byte aligned");
    FD_REQUIRE(((uintptr_t)workspace & 255) == 0, FD_E_INVAL, "fd_eval_ap: workspace not 256-byte aligned");
    FD_REQUIRE((flags & ~FD_EVAL_INPUT_ORDER) == 0, FD_E_INVAL, "fd_eval_ap: unknown flags 0x%x", flags);
    EvThr thr;
    for (int t = 0; t < EV_MAXTHR; ++t) thr.t[t] = t < n_thr ? thresholds[t] : 0.0f;

    const EvLayout L = ev_layout(N, K);
    char* ws = (char*)workspace;
    int* offs = (int*)(ws + L.offs);
    unsigned long long* keys0 = (unsigned long long*)(ws + L.keys0);
    unsigned long long* keys1 = (unsigned long long*)(ws + L.keys1);
    unsigned* vals0 = (unsigned*)(ws + L.vals0);
    unsigned* vals1 = (unsigned*)(ws + L.vals1);
    unsigned* blk = (unsigned*)(ws + L.blk);
    unsigned* hist = (unsigned*)(ws + L.hist);
    int* ctl = (int*)(ws + L.ctl);
    hipStream_t st = (hipStream_t)stream;

    if (K > 0) {
        hipLaunchKernelGGL(ev_count_kernel, dim3(N), dim3(64), 0, st, det_classes, det_counts, K, num_cls, offs);
        FD_CHECK_LAUNCH("fd_eval_ap (count)");
    } else {
        if (hipMemsetAsync(offs, 0, (size_t)N * 4, st) != hipSuccess) {
            fd_set_error("fd_eval_ap: hipMemsetAsync failed");
            return FD_E_LAUNCH;
        }
    }
    hipLaunchKernelGGL(ev_scan_kernel, dim3(1), dim3(EV_THREADS), 0, st, N, num_cls, offs, hist, n_gt, n_pred);
    FD_CHECK_LAUNCH("fd_eval_ap (scan)");
    hipLaunchKernelGGL(ev_match_kernel, dim3(N), dim3(EV_THREADS), 0, st, det_scores, det_classes, det_boxes, det_counts, K, gt_boxes,
                       gt_classes, gt_counts, G, num_cls, thr, n_thr, (flags & FD_EVAL_INPUT_ORDER) ? 1 : 0, offs, keys0, vals0, n_gt, n_pred);
    FD_CHECK_LAUNCH("fd_eval_ap (match)");
    const unsigned nb = (unsigned)(L.nb > 0 ? L.nb : 1);
    hipLaunchKernelGGL(ev_hist_kernel, dim3(nb), dim3(EV_THREADS), 0, st, keys0, offs, N, hist);
    FD_CHECK_LAUNCH("fd_eval_ap (hist)");
    hipLaunchKernelGGL(ev_plan_kernel, dim3(1), dim3(64), 0, st, offs, N, hist, ctl);
    FD_CHECK_LAUNCH("fd_eval_ap (plan)");
    for (int p = 0; p < EV_PASSES; ++p) {
        hipLaunchKernelGGL(ev_blkcount_kernel, dim3(nb), dim3(EV_THREADS), 0, st, keys0, keys1, offs, N, ctl, p, blk);
        FD_CHECK_LAUNCH("fd_eval_ap (sort: count)");
        hipLaunchKernelGGL(ev_blkscan_kernel, dim3(256), dim3(EV_THREADS), 0, st, offs, N, ctl, p, hist, blk);
        FD_CHECK_LAUNCH("fd_eval_ap (sort: scan)");
        hipLaunchKernelGGL(ev_scatter_kernel, dim3(nb), dim3(EV_THREADS), 0, st, keys0, keys1, vals0, vals1, offs, N, ctl, p, blk);
        FD_CHECK_LAUNCH("fd_eval_ap (sort: scatter)");
    }
    // the keys are dead after the sort: the first key buffer holds the AP kernel's per-TP precision (E doubles)
    hipLaunchKernelGGL(ev_ap_kernel, dim3(num_cls), dim3(EV_THREADS), 0, st, vals0, vals1, ctl, num_cls, n_thr, n_gt, n_pred,
                       (double*)keys0, ap, n_tp);
    FD_CHECK_LAUNCH("fd_eval_ap (ap)");
    return FD_OK;
}

// ===============================================================================================================
// COCO bbox evaluation (pycocotools COCOeval, iouType 'bbox', useCats, default Params): fd_eval_coco.  Shares the count / scan /
// radix-sort machinery above.
//
//   count    one workgroup per image position: sum over labels of min(detections of the label, cut = maxDets[-1])
//   scan     ev_scan_kernel: image offsets of the kept detections
//   match    one workgroup per image position: detections and GT rows ranked in LDS by (label, score desc, row) / (label, row); one
//            wave per label walks its first `cut` detections in score order, lanes across its GT rows (fp64 bbIou); per area range
//            and threshold, the last maximum >= t over the eligible non-ignored GT rows, else over the ignored ones.  Writes per
//            kept detection the sort key (label : descending score), its entry index and one word per area range (matched bits,
//            ignored bits, rank within (image, label)); atomically counts the non-ignored GT per (label, area) and entries per label
//   sort     the stable LSD radix sort above over the (image position, rank) ordered entries: pycocotools' mergesort tie order
//   gather   the per-area words in sorted order
//   accum    one workgroup per (label, area, maxDet), every threshold in one pass: TP positions compacted with their running FP
//            count, fp64 precision at each TP folded into the 101 recall bins (LDS atomic max: the envelope), then a suffix max.
#define CC_MAXT 10            // thresholds: matched / ignored bits 0..9 / 10..19 of an area word
#define CC_MAXA 4
#define CC_MAXM 4
#define CC_MAXR 128
#define CC_MAXCAT 128
#define CC_MAXDET 1024        // rank (bits 20..29 of an area word) < maxDets[-1] <= 1024

struct CcParams {
    double thr[CC_MAXT];      // min(t, 1 - 1e-10)
    double alo[CC_MAXA], ahi[CC_MAXA];
    double rec[CC_MAXR];
    int maxdet[CC_MAXM];
    int T, A, R, M, cut;
};

struct CcLayout {
    size_t offs, keys0, keys1, vals0, vals1, rec, srec, npred, blk, hist, ctl, total;
    long emax, nb;
};

static CcLayout cc_layout(int N, int K) {
    CcLayout L;
    L.emax = (long)N * K;
    if (L.emax < 1) L.emax = 1;
    L.nb = (L.emax + EV_TILE - 1) / EV_TILE;
    size_t o = 0;
    L.offs = o;  o = ev_align(o + (size_t)(N + 1) * 4);
    L.keys0 = o; o = ev_align(o + (size_t)L.emax * 8);
    L.keys1 = o; o = ev_align(o + (size_t)L.emax * 8);
    L.vals0 = o; o = ev_align(o + (size_t)L.emax * 4);
    L.vals1 = o; o = ev_align(o + (size_t)L.emax * 4);
    L.rec = o;   o = ev_align(o + (size_t)L.emax * 4 * CC_MAXA);
    L.srec = o;  o = ev_align(o + (size_t)L.emax * 4 * CC_MAXA);
    L.npred = o; o = ev_align(o + (size_t)(CC_MAXCAT + 1) * 4);
    L.blk = o;   o = ev_align(o + (size_t)L.nb * 256 * 4);
    L.hist = o;  o = ev_align(o + (size_t)EV_PASSES * 256 * 4);
    L.ctl = o;   o = ev_align(o + 16 * 4);
    L.total = o;
    return L;
}

__device__ __forceinline__ int cc_image(const int32_t* __restrict__ order, int p, int N) {
    const int img = order ? order[p] : p;
    return (img >= 0 && img < N) ? img : -1;
}

// count: kept detections per image position (the first `cut` of each label)
__global__ __launch_bounds__(EV_THREADS) void cc_count_kernel(const int64_t* __restrict__ det_labels, const int32_t* __restrict__ det_counts,
                                                              const int32_t* __restrict__ order, int N, int K, int C, int cut,
                                                              int* __restrict__ img_cnt) {
    __shared__ unsigned h[CC_MAXCAT + 1];
    __shared__ unsigned sh[4];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int img = cc_image(order, p, N);
    for (int l = tid; l <= C; l += EV_THREADS) h[l] = 0u;
    __syncthreads();
    if (img >= 0) {
        int c = det_counts ? det_counts[img] : K;
        c = max(0, min(c, K));
        for (int i = tid; i < c; i += EV_THREADS) {
            const int64_t l = det_labels[(long)img * K + i];
            if (l >= 1 && l <= C) atomicAdd(&h[l], 1u);
        }
    }
    __syncthreads();
    unsigned n = 0;
    for (int l = 1 + tid; l <= C; l += EV_THREADS) n += min(h[l], (unsigned)cut);
    unsigned total;
    ev_block_excl_scan(n, sh, total);
    if (tid == 0) img_cnt[p] = (int)total;
}

// ---------------------------------------------------------------------------------------------------------------
// match: one workgroup per image position
struct CcBox {
    double x, y, w, h;
};

struct CcMatchSh {
    unsigned long long dkey[EV_MAXK];   // (label << 42) | (descending score key << 10) | row; ~0 = not taking part
    float4 dbox[EV_MAXK];               // by row, xywh
    CcBox gbox[EV_MAXG];                // by row, xywh
    unsigned long long taken[EV_MAXG];  // GT rank -> bit a * T + t: matched at area a, threshold t
    unsigned gkey[EV_MAXG];             // (label << 9) | row; ~0 = not taking part
    unsigned short dperm[EV_MAXK];      // rank -> row
    unsigned short gperm[EV_MAXG];      // rank -> row
    unsigned char gflag[EV_MAXG];       // by row: bit a = ignored at area a (crowd, or annotation area outside the range); bit 7 = crowd
    unsigned short dstart[CC_MAXCAT + 1], dend[CC_MAXCAT + 1], gstart[CC_MAXCAT + 1], gend[CC_MAXCAT + 1];
    int ostart[CC_MAXCAT + 1];          // label -> first kept entry within the image
};

// maskApi.c bbIou of one detection (x, y, w, h, area da) against one GT box, fp64 in its operation order; crowd: u = da
__device__ __forceinline__ double cc_iou(const CcBox& g, double dx, double dy, double dw, double dh, double da, bool crowd) {
    const double w = fmin(dw + dx, g.w + g.x) - fmax(dx, g.x);
    if (w <= 0) return 0.0;
    const double h = fmin(dh + dy, g.h + g.y) - fmax(dy, g.y);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : (da + g.w * g.h) - i;
    return i / u;
}

// wave-wide last maximum: (v, q) beats (b, j) when v > b, or v == b and q > j; every lane ends with the result
__device__ __forceinline__ void cc_wave_lastmax(double& v, int& q) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oq = __shfl_xor(q, o);
        if (ov > v || (ov == v && oq > q)) {
            v = ov;
            q = oq;
        }
    }
}

__device__ __forceinline__ int cc_wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

#define CC_LANE_G (EV_MAXG / 64)   // GT ranks per lane

__global__ __launch_bounds__(EV_THREADS) void cc_match_kernel(
    const float* __restrict__ det_scores, const int64_t* __restrict__ det_labels, const float* __restrict__ det_boxes,
    const int32_t* __restrict__ det_counts, int K, const double* __restrict__ gt_boxes, const double* __restrict__ gt_area,
    const uint8_t* __restrict__ gt_crowd, const int64_t* __restrict__ gt_labels, int G, const int32_t* __restrict__ order, int N, int C,
    CcParams P, long emax, const int* __restrict__ offs, unsigned long long* __restrict__ out_keys, unsigned* __restrict__ out_vals,
    unsigned* __restrict__ rec, int32_t* __restrict__ n_gt, int32_t* __restrict__ npred) {
    __shared__ CcMatchSh sh;
    const int tid = threadIdx.x, p = blockIdx.x;
    const int img = cc_image(order, p, N);
    if (img < 0) return;        // not a permutation: the image takes no part (count wrote 0 for it)
    const long off = offs[p];
    int c = det_counts ? det_counts[img] : K;
    c = max(0, min(c, K));
    const int A = P.A, T = P.T, cut = P.cut;

    for (int l = tid; l <= C; l += EV_THREADS) sh.dstart[l] = sh.dend[l] = sh.gstart[l] = sh.gend[l] = 0;
    for (int i = tid; i < K; i += EV_THREADS) {
        unsigned long long key = ~0ull;
        if (i < c) {
            const int64_t l = det_labels[(long)img * K + i];
            if (l >= 1 && l <= C) {
                key = ((unsigned long long)l << 42) | ((unsigned long long)ev_desc_key(det_scores[(long)img * K + i]) << 10) | (unsigned long long)i;
                sh.dbox[i] = reinterpret_cast<const float4*>(det_boxes)[(long)img * K + i];
            }
        }
        sh.dkey[i] = key;
    }
    int ng = 0;
    for (int base = 0; base < G; base += EV_THREADS) {
        const int g = base + tid;
        bool valid = false;
        if (g < G) {
            const int64_t l = gt_labels[(long)img * G + g];
            valid = l >= 1 && l <= C;
            sh.gkey[g] = valid ? (((unsigned)l << 9) | (unsigned)g) : ~0u;
            if (valid) {
                const double* b = gt_boxes + ((long)img * G + g) * 4;
                sh.gbox[g] = CcBox{b[0], b[1], b[2], b[3]};
                const double ar = gt_area[(long)img * G + g];
                const bool crowd = gt_crowd[(long)img * G + g] != 0;
                unsigned f = crowd ? 0x80u : 0u;
                for (int a = 0; a < A; ++a)
                    if (crowd || ar < P.alo[a] || ar > P.ahi[a]) f |= 1u << a;
                sh.gflag[g] = (unsigned char)f;
            }
            sh.taken[g] = 0ull;
        }
        ng += __syncthreads_count(valid);
    }
    __syncthreads();

    // rank = number of smaller keys (unique: the row is part of them)
    for (int i0 = tid; i0 < K; i0 += 4 * EV_THREADS) {
        unsigned long long k4[4];
        int r4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; ++u) k4[u] = (i0 + u * EV_THREADS < K) ? sh.dkey[i0 + u * EV_THREADS] : ~0ull;
        for (int j = 0; j < K; ++j) {
            const unsigned long long kj = sh.dkey[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) r4[u] += kj < k4[u] ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k4[u] != ~0ull) sh.dperm[r4[u]] = (unsigned short)(i0 + u * EV_THREADS);
    }
    for (int g = tid; g < G; g += EV_THREADS) {
        const unsigned kg = sh.gkey[g];
        if (kg == ~0u) continue;
        int r = 0;
        for (int j = 0; j < G; ++j) r += sh.gkey[j] < kg ? 1 : 0;
        sh.gperm[r] = (unsigned short)g;
    }
    __syncthreads();
    int ndet = 0;       // detections taking part
    for (int base = 0; base < K; base += EV_THREADS) ndet += __syncthreads_count(base + tid < K && sh.dkey[base + tid] != ~0ull);

    // label ranges over the ranked detections / GT rows
    for (int q = tid; q < ndet; q += EV_THREADS) {
        const int l = (int)(sh.dkey[sh.dperm[q]] >> 42);
        if (q == 0 || (int)(sh.dkey[sh.dperm[q - 1]] >> 42) != l) sh.dstart[l] = (unsigned short)q;
        if (q == ndet - 1 || (int)(sh.dkey[sh.dperm[q + 1]] >> 42) != l) sh.dend[l] = (unsigned short)(q + 1);
    }
    for (int q = tid; q < ng; q += EV_THREADS) {
        const int l = (int)(sh.gkey[sh.gperm[q]] >> 9);
        if (q == 0 || (int)(sh.gkey[sh.gperm[q - 1]] >> 9) != l) sh.gstart[l] = (unsigned short)q;
        if (q == ng - 1 || (int)(sh.gkey[sh.gperm[q + 1]] >> 9) != l) sh.gend[l] = (unsigned short)(q + 1);
    }
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int l = 1; l <= C; ++l) {
            sh.ostart[l] = s;
            s += min((int)sh.dend[l] - (int)sh.dstart[l], cut);
        }
    }
    __syncthreads();

    const int wave = tid >> 6, lane = ev_lane();
    for (int l = 1 + wave; l <= C; l += EV_THREADS / 64) {
        const int ds = sh.dstart[l], de = sh.dend[l], gs = sh.gstart[l], ge = sh.gend[l];
        // non-ignored GT rows of the label per area range
        for (int a = 0; a < A; ++a) {
            int n = 0;
            for (int q0 = gs; q0 < ge; q0 += 64) {
                const int q = q0 + lane;
                n += __popcll(__ballot(q < ge && !((sh.gflag[sh.gperm[q < ge ? q : gs]] >> a) & 1u)));
            }
            if (lane == 0 && n) atomicAdd(&n_gt[(l - 1) * A + a], n);
        }
        const int nkeep = min(de - ds, cut);
        if (nkeep <= 0) continue;
        if (lane == 0) atomicAdd(&npred[l], nkeep);
        const long obase = off + sh.ostart[l];
        if (gs == ge) {     // no GT of the label in the image: every detection unmatched, ignored where its area is outside the range
            for (int r = lane; r < nkeep; r += 64) {
                const int row = sh.dperm[ds + r];
                const float4 d = sh.dbox[row];
                const double da = (double)d.z * (double)d.w;
                const long e = obase + r;
                out_keys[e] = ((unsigned long long)l << 32) | ev_desc_key(det_scores[(long)img * K + row]);
                out_vals[e] = (unsigned)e;
                for (int a = 0; a < A; ++a) {
                    const unsigned ib = (da < P.alo[a] || da > P.ahi[a]) ? ((1u << T) - 1u) : 0u;
                    rec[a * emax + e] = (ib << 10) | ((unsigned)r << 20);
                }
            }
            continue;
        }
        for (int r = 0; r < nkeep; ++r) {
            const int row = sh.dperm[ds + r];
            const float4 d = sh.dbox[row];
            const double dx = d.x, dy = d.y, dw = d.z, dh = d.w;
            const double da = dw * dh;
            double iou[CC_LANE_G];
#pragma unroll
            for (int k = 0; k < CC_LANE_G; ++k) {
                const int q = gs + lane + 64 * k;
                iou[k] = 0.0;
                if (q < ge) {
                    const int g = sh.gperm[q];
                    iou[k] = cc_iou(sh.gbox[g], dx, dy, dw, dh, da, (sh.gflag[g] >> 7) != 0);
                }
            }
            const long e = obase + r;
            for (int a = 0; a < A; ++a) {
                // per group (0 = non-ignored, 1 = ignored): last maximum over every row of the group, whatever is taken
                double bv[2];
                int bq[2];
                bool bnan[2];
#pragma unroll
                for (int grp = 0; grp < 2; ++grp) {
                    double v = -1.0;
                    int qq = -1;
                    bool nan = false;
#pragma unroll
                    for (int k = 0; k < CC_LANE_G; ++k) {
                        const int q = gs + lane + 64 * k;
                        if (q < ge && (int)((sh.gflag[sh.gperm[q]] >> a) & 1u) == grp) {
                            if (iou[k] != iou[k]) nan = true;
                            else if (iou[k] >= v) {
                                v = iou[k];
                                qq = q;
                            }
                        }
                    }
                    cc_wave_lastmax(v, qq);
                    bv[grp] = v;
                    bq[grp] = qq;
                    bnan[grp] = __ballot(nan) != 0ull;
                }
                unsigned mb = 0, ib = 0;
                for (int t = 0; t < T; ++t) {
                    const int bit = a * T + t;
                    const double th = P.thr[t];
                    int m = -1, mg = 0;
#pragma unroll
                    for (int grp = 0; grp < 2; ++grp) {
                        if (m >= 0) break;
                        int mm;
                        const int j = bq[grp];
                        if (!bnan[grp] && (j < 0 || !(bv[grp] >= th))) {
                            mm = -1;        // nothing of the group reaches the threshold
                        } else if (!bnan[grp] && (((sh.gflag[sh.gperm[j]] >> 7) != 0) || !((sh.taken[j] >> bit) & 1ull))) {
                            mm = j;         // the group's last maximum is still available: it is also the eligible rows' last maximum
                        } else {
                            // full pass over the eligible rows (untaken, or crowd): pycocotools' loop keeps the last row not below the
                            // running best; a NaN IoU is never below it, nor is any eligible row after it
                            double v = -1.0;
                            int qq = -1, last = -1;
                            bool nan = false;
#pragma unroll
                            for (int k = 0; k < CC_LANE_G; ++k) {
                                const int q = gs + lane + 64 * k;
                                if (q < ge) {
                                    const unsigned f = sh.gflag[sh.gperm[q]];
                                    if ((int)((f >> a) & 1u) == grp && (((f >> 7) != 0) || !((sh.taken[q] >> bit) & 1ull))) {
                                        last = q;
                                        if (iou[k] != iou[k]) nan = true;
                                        else if (iou[k] >= v) {
                                            v = iou[k];
                                            qq = q;
                                        }
                                    }
                                }
                            }
                            cc_wave_lastmax(v, qq);
                            if (__ballot(nan) != 0ull) mm = cc_wave_max(last);
                            else mm = (qq >= 0 && v >= th) ? qq : -1;
                        }
                        m = mm;
                        mg = grp;
                    }
                    if (m >= 0) {
                        mb |= 1u << t;
                        if (mg) ib |= 1u << t;              // matched to an ignored GT row: ignored
                        if (lane == 0) sh.taken[m] |= 1ull << bit;
                    } else if (da < P.alo[a] || da > P.ahi[a]) {
                        ib |= 1u << t;                      // unmatched and outside the area range: ignored
                    }
                }
                if (lane == 0) rec[a * emax + e] = mb | (ib << 10) | ((unsigned)r << 20);
            }
            if (lane == 0) {
                out_keys[e] = ((unsigned long long)l << 32) | ev_desc_key(det_scores[(long)img * K + row]);
                out_vals[e] = (unsigned)e;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// gather: the area words in sorted entry order
__global__ __launch_bounds__(EV_THREADS) void cc_gather_kernel(const unsigned* __restrict__ vals0, const unsigned* __restrict__ vals1,
                                                               const int* __restrict__ ctl, const int* __restrict__ offs, int N, int A, long emax,
                                                               const unsigned* __restrict__ rec, unsigned* __restrict__ srec) {
    const long E = offs[N];
    const unsigned* vals = ctl[EV_CTL_SEL + EV_PASSES] ? vals1 : vals0;
    for (long i = (long)blockIdx.x * EV_THREADS + threadIdx.x; i < E; i += (long)gridDim.x * EV_THREADS) {
        const long v = vals[i];
        for (int a = 0; a < A; ++a) srec[a * emax + i] = rec[a * emax + v];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// accumulate: one workgroup per (label, area, maxDet), all thresholds in one pass over the label's sorted entries
__global__ __launch_bounds__(EV_THREADS) void cc_accum_kernel(const unsigned* __restrict__ srec, long emax, const int32_t* __restrict__ npred,
                                                              const int32_t* __restrict__ n_gt, CcParams P, int C, double* __restrict__ precision,
                                                              double* __restrict__ recall) {
    __shared__ int jr[CC_MAXR];
    __shared__ unsigned long long bmax[CC_MAXT][CC_MAXR];
    __shared__ unsigned cnt[EV_THREADS / 64][CC_MAXT][2];
    __shared__ unsigned ntp[CC_MAXT];
    const int l = blockIdx.x + 1, a = blockIdx.y, mi = blockIdx.z, k = l - 1;
    const int tid = threadIdx.x, lane = ev_lane(), w = tid >> 6;
    const int T = P.T, A = P.A, R = P.R, M = P.M;
    const int npig = n_gt[k * A + a];
    const long cell = ((long)k * A + a) * M + mi;               // (k, a, m) within one [K][A][M] slice
    const long tstride = (long)C * A * M;
    if (npig == 0) {        // no non-ignored GT: -1, as pycocotools leaves it
        for (int i = tid; i < T * R; i += EV_THREADS) precision[(long)i * tstride + cell] = -1.0;
        for (int t = tid; t < T; t += EV_THREADS) recall[t * tstride + cell] = -1.0;
        return;
    }
    const double g = (double)npig;
    // jr[r] = np.searchsorted(rc, recThrs[r], 'left') in TP terms: the first TP j with rc = (j + 1) / npig >= recThrs[r] (npig: none)
    for (int r = tid; r < R; r += EV_THREADS) {
        const double rt = P.rec[r];
        long j = 0;
        if (rt == rt && rt > 0.0) j = max(0l, min((long)npig, (long)ceil(rt * g) - 2));
        while (j > 0 && (double)j / g >= rt) --j;
        while (j < npig && !((double)(j + 1) / g >= rt)) ++j;
        jr[r] = (int)j;
    }
    for (int i = tid; i < CC_MAXT * CC_MAXR; i += EV_THREADS) (&bmax[0][0])[i] = 0ull;
    long seg = 0;
    for (int i = 1; i < l; ++i) seg += npred[i];
    const long n = npred[l];
    const unsigned* words = srec + a * emax + seg;
    const unsigned maxdet = (unsigned)P.maxdet[mi];
    unsigned ctp[CC_MAXT], cfp[CC_MAXT];
#pragma unroll
    for (int t = 0; t < CC_MAXT; ++t) ctp[t] = cfp[t] = 0u;
    __syncthreads();
    for (long c0 = 0; c0 < n; c0 += EV_THREADS) {
        const long i = c0 + tid;
        unsigned wv = 0u;
        bool valid = false;
        if (i < n) {
            wv = words[i];
            valid = (wv >> 20) < maxdet;
        }
        unsigned long long btp[CC_MAXT], bfp[CC_MAXT];
#pragma unroll
        for (int t = 0; t < CC_MAXT; ++t) {
            if (t < T) {
                const bool m = (wv >> t) & 1u, ig = (wv >> (10 + t)) & 1u;
                btp[t] = __ballot(valid && m && !ig);
                bfp[t] = __ballot(valid && !m && !ig);
                if (lane == 0) {
                    cnt[w][t][0] = (unsigned)__popcll(btp[t]);
                    cnt[w][t][1] = (unsigned)__popcll(bfp[t]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < CC_MAXT; ++t) {
            if (t < T) {
                unsigned ptp = ctp[t], pfp = cfp[t], stp = 0u, sfp = 0u;
                for (int q = 0; q < EV_THREADS / 64; ++q) {
                    if (q < w) {
                        ptp += cnt[q][t][0];
                        pfp += cnt[q][t][1];
                    }
                    stp += cnt[q][t][0];
                    sfp += cnt[q][t][1];
                }
                if ((btp[t] >> lane) & 1ull) {
                    const unsigned j = ptp + (unsigned)__popcll(btp[t] & ev_lt_mask());
                    const unsigned f = pfp + (unsigned)__popcll(bfp[t] & ev_lt_mask());
                    const double tp = (double)(j + 1u);
                    const double pr = tp / (((double)f + tp) + 0x1p-52);     // tp / (fp + tp + np.spacing(1))
                    // the TP serves every recall bin r with jr[r] <= j: record it at the last one, the suffix max spreads it
                    int lo = 0, hi = R;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (jr[mid] <= (int)j) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo > 0) atomicMax(&bmax[t][lo - 1], (unsigned long long)__double_as_longlong(pr));   // pr > 0: bits order as values
                }
                ctp[t] += stp;
                cfp[t] += sfp;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int t = 0; t < CC_MAXT; ++t)
            if (t < T) ntp[t] = ctp[t];
    }
    __syncthreads();
    for (int t = tid; t < T; t += EV_THREADS) {
        unsigned long long cm = 0ull;
        for (int r = R - 1; r >= 0; --r) {
            cm = max(cm, bmax[t][r]);
            precision[((long)t * R + r) * tstride + cell] = __longlong_as_double((long long)cm);
        }
        recall[t * tstride + cell] = (double)ntp[t] / g;
    }
}

// ---------------------------------------------------------------------------------------------------------------
static int cc_args_ok(int32_t N, int32_t K, int32_t G, int32_t num_cats) {
    if (N < 1 || K < 0 || G < 0 || num_cats < 1) {
        fd_set_error("fd_eval_coco: bad sizes N=%d K=%d G=%d num_cats=%d", N, K, G, num_cats);
        return FD_E_INVAL;
    }
    if (K > EV_MAXK || G > EV_MAXG || num_cats > CC_MAXCAT) {
        fd_set_error("fd_eval_coco: limits are K <= %d detections and G <= %d GT rows per image, num_cats <= %d (got K=%d G=%d num_cats=%d)",
                     EV_MAXK, EV_MAXG, CC_MAXCAT, K, G, num_cats);
        return FD_E_UNSUPPORTED;
    }
    if ((long)N * K > 0x7FFFFFFFl - EV_TILE) {
        fd_set_error("fd_eval_coco: N * K = %ld detection rows exceeds 2^31", (long)N * K);
        return FD_E_UNSUPPORTED;
    }
    return FD_OK;
}

extern "C" int64_t fd_eval_coco_workspace_bytes(int32_t N, int32_t K, int32_t G, int32_t num_cats) {
    if (cc_args_ok(N, K, G, num_cats) != FD_OK) return -1;
    return (int64_t)cc_layout(N, K).total;
}

extern "C" int32_t fd_eval_coco(const float* det_scores, const int64_t* det_labels, const float* det_boxes, const int32_t* det_counts, int32_t N,
                                int32_t K, const double* gt_boxes, const double* gt_area, const uint8_t* gt_crowd, const int64_t* gt_labels,
                                int32_t G, const int32_t* image_order, int32_t num_cats, const double* iou_thrs, int32_t n_thr,
                                const double* rec_thrs, int32_t n_rec, const double* area_rng, int32_t n_area, const int32_t* max_dets,
                                int32_t n_maxdet, double* precision, double* recall, int32_t* n_gt, void* workspace, fd_stream_t stream) {
    const int rc = cc_args_ok(N, K, G, num_cats);
    if (rc != FD_OK) return rc;
    FD_REQUIRE(iou_thrs && rec_thrs && area_rng && max_dets && precision && recall && n_gt && workspace, FD_E_INVAL,
               "fd_eval_coco: null pointer");
    FD_REQUIRE(K == 0 || (det_scores && det_labels && det_boxes), FD_E_INVAL, "fd_eval_coco: null detection pointer");
    FD_REQUIRE(G == 0 || (gt_boxes && gt_area && gt_crowd && gt_labels), FD_E_INVAL, "fd_eval_coco: null GT pointer");
    FD_REQUIRE(((uintptr_t)det_boxes & 15) == 0 && ((uintptr_t)gt_boxes & 7) == 0, FD_E_INVAL, "fd_eval_coco: boxes not aligned");
    FD_REQUIRE(((uintptr_t)workspace & 255) == 0, FD_E_INVAL, "fd_eval_coco: workspace not 256-byte aligned");
    if (n_thr < 1 || n_thr > CC_MAXT || n_rec < 1 || n_rec > CC_MAXR || n_area < 1 || n_area > CC_MAXA || n_maxdet < 1 || n_maxdet > CC_MAXM) {
        fd_set_error("fd_eval_coco: limits are 1..%d IoU thresholds, 1..%d recall thresholds, 1..%d area ranges, 1..%d maxDets "
                     "(got %d, %d, %d, %d)", CC_MAXT, CC_MAXR, CC_MAXA, CC_MAXM, n_thr, n_rec, n_area, n_maxdet);
        return FD_E_UNSUPPORTED;
    }
    CcParams P = {};
    P.T = n_thr;
    P.R = n_rec;
    P.A = n_area;
    P.M = n_maxdet;
    for (int t = 0; t < n_thr; ++t) P.thr[t] = fmin(iou_thrs[t], 1.0 - 1e-10);     // COCOeval.evaluateImg: min([t, 1 - 1e-10])
    for (int r = 0; r < n_rec; ++r) {
        P.rec[r] = rec_thrs[r];
        FD_REQUIRE(r == 0 || rec_thrs[r] >= rec_thrs[r - 1], FD_E_INVAL, "fd_eval_coco: recall thresholds must ascend");
    }
    for (int a = 0; a < n_area; ++a) {
        P.alo[a] = area_rng[2 * a];
        P.ahi[a] = area_rng[2 * a + 1];
    }
    for (int m = 0; m < n_maxdet; ++m) {
        P.maxdet[m] = max_dets[m];
        FD_REQUIRE(max_dets[m] >= 1 && max_dets[m] <= CC_MAXDET && (m == 0 || max_dets[m] >= max_dets[m - 1]), FD_E_INVAL,
                   "fd_eval_coco: maxDets must ascend within 1..%d", CC_MAXDET);
    }
    P.cut = max_dets[n_maxdet - 1];

    const CcLayout L = cc_layout(N, K);
    char* ws = (char*)workspace;
    int* offs = (int*)(ws + L.offs);
    unsigned long long* keys0 = (unsigned long long*)(ws + L.keys0);
    unsigned long long* keys1 = (unsigned long long*)(ws + L.keys1);
    unsigned* vals0 = (unsigned*)(ws + L.vals0);
    unsigned* vals1 = (unsigned*)(ws + L.vals1);
    unsigned* rec = (unsigned*)(ws + L.rec);
    unsigned* srec = (unsigned*)(ws + L.srec);
    int32_t* npred = (int32_t*)(ws + L.npred);
    unsigned* blk = (unsigned*)(ws + L.blk);
    unsigned* hist = (unsigned*)(ws + L.hist);
    int* ctl = (int*)(ws + L.ctl);
    hipStream_t st = (hipStream_t)stream;

    if (hipMemsetAsync(npred, 0, (size_t)(CC_MAXCAT + 1) * 4, st) != hipSuccess ||
        hipMemsetAsync(n_gt, 0, (size_t)num_cats * n_area * 4, st) != hipSuccess) {
        fd_set_error("fd_eval_coco: hipMemsetAsync failed");
        return FD_E_LAUNCH;
    }
    hipLaunchKernelGGL(cc_count_kernel, dim3(N), dim3(EV_THREADS), 0, st, det_labels, det_counts, image_order, N, K, num_cats, P.cut, offs);
    FD_CHECK_LAUNCH("fd_eval_coco (count)");
    hipLaunchKernelGGL(ev_scan_kernel, dim3(1), dim3(EV_THREADS), 0, st, N, 0, offs, hist, (int32_t*)nullptr, (int32_t*)nullptr);
    FD_CHECK_LAUNCH("fd_eval_coco (scan)");
    hipLaunchKernelGGL(cc_match_kernel, dim3(N), dim3(EV_THREADS), 0, st, det_scores, det_labels, det_boxes, det_counts, K, gt_boxes, gt_area,
                       gt_crowd, gt_labels, G, image_order, N, num_cats, P, L.emax, offs, keys0, vals0, rec, n_gt, npred);
    FD_CHECK_LAUNCH("fd_eval_coco (match)");
    const unsigned nb = (unsigned)(L.nb > 0 ? L.nb : 1);
    hipLaunchKernelGGL(ev_hist_kernel, dim3(nb), dim3(EV_THREADS), 0, st, keys0, offs, N, hist);
    FD_CHECK_LAUNCH("fd_eval_coco (hist)");
    hipLaunchKernelGGL(ev_plan_kernel, dim3(1), dim3(64), 0, st, offs, N, hist, ctl);
    FD_CHECK_LAUNCH("fd_eval_coco (plan)");
    for (int p = 0; p < EV_PASSES; ++p) {
        hipLaunchKernelGGL(ev_blkcount_kernel, dim3(nb), dim3(EV_THREADS), 0, st, keys0, keys1, offs, N, ctl, p, blk);
        FD_CHECK_LAUNCH("fd_eval_coco (sort: count)");
        hipLaunchKernelGGL(ev_blkscan_kernel, dim3(256), dim3(EV_THREADS), 0, st, offs, N, ctl, p, hist, blk);
        FD_CHECK_LAUNCH("fd_eval_coco (sort: scan)");
        hipLaunchKernelGGL(ev_scatter_kernel, dim3(nb), dim3(EV_THREADS), 0, st, keys0, keys1, vals0, vals1, offs, N, ctl, p, blk);
        FD_CHECK_LAUNCH("fd_eval_coco (sort: scatter)");
    }
    hipLaunchKernelGGL(cc_gather_kernel, dim3(nb * (EV_TILE / EV_THREADS)), dim3(EV_THREADS), 0, st, vals0, vals1, ctl, offs, N, n_area, L.emax,
                       rec, srec);
    FD_CHECK_LAUNCH("fd_eval_coco (gather)");
    hipLaunchKernelGGL(cc_accum_kernel, dim3(num_cats, n_area, n_maxdet), dim3(EV_THREADS), 0, st, srec, L.emax, npred, n_gt, P, num_cats,
                       precision, recall);
    FD_CHECK_LAUNCH("fd_eval_coco (accum)");
    return FD_OK;
}
