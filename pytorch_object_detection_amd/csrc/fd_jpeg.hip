// fd_jpeg.hip — baseline JPEG decoding for the device (gfx950), DESIGN §4.2h: what the reference does with
// Image.open(path).convert('RGB') (dataset/voc.py:69, dataset/pascalvoc.py:28, data/dataload.py:35).
//   * host (fd_jpeg_host.h, compiled in here): marker parsing and Huffman decoding, the serial part;
//   * fd_jpeg_idct_u8: dequantise + libjpeg's jpeg_idct_islow for every component of every image, ONE launch;
//   * fd_jpeg_color_u8: libjpeg-turbo's fancy chroma upsampling + YCbCr -> RGB for every image, ONE launch.
// Integer arithmetic only (built with -ffp-contract=off like its neighbours all the same); exact against Pillow, restated in
// numpy by tests/jpeg_ref.py.  Both launches read a job table in device memory; the host validates an identical host copy
// first, so every offset a kernel forms lies inside the buffers it was given.
#define FD_JPEG_API __attribute__((used, visibility("default")))
#include "fd_jpeg_host.h"
#include "fd_common.h"

#define JPEG_MAX_GRID_SIDE 8192          // blocks per side: (65535 + 15) / 8 rounded up
#define JPEG_BLOCKS_PER_WG 32
#define JPEG_WS_STRIDE 72                // dwords per block in LDS: 64 + 8, so the column-pass stores of the four blocks of a 32-lane half hit 32 banks

// ------------------------------------------------------------------------------ dequantise + jpeg_idct_islow
#define JC_BITS 13
#define JP1_BITS 2
#define JDESCALE(x, n) (((x) + (1l << ((n) - 1))) >> (n))

// One 1-D pass of jidctint.c's 8-point inverse DCT (Loeffler-Ligtenberg-Moshovitz), libjpeg's variable names.  JLONG is 64 bits on
// LP64: |coef * q| <= 32768 * 255 < 2^23, a column sum * 25172 < 2^41, a row pass on those another 2^17 on top: no overflow.
__device__ __forceinline__ void jpeg_idct_1d(const long in[8], long out[8], int shift) {
    long z2 = in[2], z3 = in[6];
    long z1 = (z2 + z3) * 4433l;
    long tmp2 = z1 + z3 * -15137l;
    long tmp3 = z1 + z2 * 6270l;
    z2 = in[0]; z3 = in[4];
    long tmp0 = (z2 + z3) * (1l << JC_BITS);
    long tmp1 = (z2 - z3) * (1l << JC_BITS);
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    long z4 = tmp1 + tmp3;
    const long z5 = (z3 + z4) * 9633l;
    tmp0 *= 2446l; tmp1 *= 16819l; tmp2 *= 25172l; tmp3 *= 12299l;
    z1 *= -7373l; z2 *= -20995l; z3 *= -16069l; z4 *= -3196l;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = JDESCALE(tmp10 + tmp3, shift); out[7] = JDESCALE(tmp10 - tmp3, shift);
    out[1] = JDESCALE(tmp11 + tmp2, shift); out[6] = JDESCALE(tmp11 - tmp2, shift);
    out[2] = JDESCALE(tmp12 + tmp1, shift); out[5] = JDESCALE(tmp12 - tmp1, shift);
    out[3] = JDESCALE(tmp13 + tmp0, shift); out[4] = JDESCALE(tmp13 - tmp0, shift);
}

// libjpeg's range_limit table read at (v & RANGE_MASK): clamp(v + 128) on [-512, 511], its wrap-around outside
__device__ __forceinline__ unsigned jpeg_range_limit(long v) {
    const unsigned i = (unsigned)v & 1023u;
    return i < 128u ? i + 128u : i < 512u ? 255u : i < 896u ? 0u : i - 896u;
}

__global__ __launch_bounds__(256) void jpeg_idct_u8_kernel(const fd_jpeg_idct_job* __restrict__ jobs, const short* __restrict__ coefs,
                                                           const unsigned short* __restrict__ qtabs, unsigned char* __restrict__ planes) {
    __shared__ int ws[JPEG_BLOCKS_PER_WG * JPEG_WS_STRIDE];
    const fd_jpeg_idct_job job = jobs[blockIdx.y];
    const unsigned nblk = (unsigned)job.bw * (unsigned)job.bh;       // <= 8192^2 = 2^26
    const unsigned lb = threadIdx.x >> 3, j = threadIdx.x & 7u;       // block of the workgroup; column, then row, of the block
    const unsigned blk = blockIdx.x * JPEG_BLOCKS_PER_WG + lb;
    const bool live = blk < nblk;
    int* w = ws + lb * JPEG_WS_STRIDE;
    if (live) {
        const short* __restrict__ c = coefs + job.coef_off + (long)blk * 64;
        const unsigned short* __restrict__ q = qtabs + (long)job.qt * 64;
        long in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = (long)((int)c[k * 8 + j] * (int)q[k * 8 + j]);      // DEQUANTIZE: an int product, as libjpeg's
        jpeg_idct_1d(in, out, JC_BITS - JP1_BITS);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * 8 + j] = (int)out[k];                                 // the int workspace of jpeg_idct_islow
    }
    __syncthreads();
    if (live) {
        long in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = (long)w[j * 8 + k];
        jpeg_idct_1d(in, out, JC_BITS + JP1_BITS + 3);
        const unsigned by = blk / (unsigned)job.bw, bx = blk - by * (unsigned)job.bw;
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= jpeg_range_limit(out[k]) << (8 * k);
            hi |= jpeg_range_limit(out[k + 4]) << (8 * k);
        }
        // row 8 * by + j of a plane 8 * bw bytes wide, bytes 8 * bx .. 8 * bx + 7: 8-byte aligned (plane_off is)
        uint2* o = reinterpret_cast<uint2*>(planes + job.plane_off + ((long)(by * 8u + j) * (unsigned)job.bw + bx) * 8);
        *o = make_uint2(lo, hi);
    }
}

extern "C" int32_t fd_jpeg_idct_u8(const fd_jpeg_idct_job* jobs_host, const fd_jpeg_idct_job* jobs_dev, int32_t n_jobs, const int16_t* coefs,
                                   int64_t coef_elems, const uint16_t* qtabs, int32_t n_qtabs, uint8_t* planes, int64_t planes_bytes,
                                   fd_stream_t stream) {
    FD_REQUIRE(jobs_host && jobs_dev && coefs && qtabs && planes, FD_E_INVAL, "fd_jpeg_idct_u8: null pointer");
    FD_REQUIRE(n_jobs >= 1 && n_jobs <= 65535 && coef_elems >= 64 && n_qtabs >= 1 && planes_bytes >= 64, FD_E_INVAL,
               "fd_jpeg_idct_u8: bad job count %d, coefficient count %lld, table count %d or plane bytes %lld", n_jobs, (long long)coef_elems, n_qtabs,
               (long long)planes_bytes);
    FD_REQUIRE(((uintptr_t)jobs_dev & 7) == 0 && ((uintptr_t)coefs & 1) == 0 && ((uintptr_t)qtabs & 1) == 0 && ((uintptr_t)planes & 7) == 0, FD_E_INVAL,
               "fd_jpeg_idct_u8: jobs / planes not 8-byte or coefs / qtabs not 2-byte aligned");
    int64_t max_blocks = 0;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const fd_jpeg_idct_job& jb = jobs_host[i];
        FD_REQUIRE(jb.bw >= 1 && jb.bh >= 1 && jb.bw <= JPEG_MAX_GRID_SIDE && jb.bh <= JPEG_MAX_GRID_SIDE, FD_E_INVAL,
                   "fd_jpeg_idct_u8: job %d: block grid %d x %d outside 1 .. %d", i, jb.bh, jb.bw, JPEG_MAX_GRID_SIDE);
        const int64_t blocks = (int64_t)jb.bw * jb.bh;
        FD_REQUIRE(jb.coef_off >= 0 && jb.coef_off <= coef_elems - blocks * 64, FD_E_INVAL, "fd_jpeg_idct_u8: job %d: coefficients outside the buffer", i);
        FD_REQUIRE(jb.qt >= 0 && jb.qt < n_qtabs, FD_E_INVAL, "fd_jpeg_idct_u8: job %d: quantisation table %d outside 0 .. %d", i, jb.qt, n_qtabs - 1);
        FD_REQUIRE(jb.plane_off >= 0 && (jb.plane_off & 7) == 0 && jb.plane_off <= planes_bytes - blocks * 64, FD_E_INVAL,
                   "fd_jpeg_idct_u8: job %d: plane outside the buffer or not 8-byte aligned", i);
        if (blocks > max_blocks) max_blocks = blocks;
    }
    const unsigned gx = (unsigned)((max_blocks + JPEG_BLOCKS_PER_WG - 1) / JPEG_BLOCKS_PER_WG);
    hipLaunchKernelGGL(jpeg_idct_u8_kernel, dim3(gx, (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, jobs_dev, (const short*)coefs,
                       (const unsigned short*)qtabs, (unsigned char*)planes);
    FD_CHECK_LAUNCH("fd_jpeg_idct_u8");
    return FD_OK;
}

// ------------------------------------------------------------------------------ chroma upsampling + YCbCr -> RGB
__device__ __forceinline__ int jpeg_sample(const unsigned char* __restrict__ p, int stride, int r, int c, int dh, int dw) {
    return ((unsigned)r < (unsigned)dh && (unsigned)c < (unsigned)dw) ? (int)p[(long)r * stride + c] : 0;      // the only gate in front of the loads
}

// One chroma sample at full resolution (jdsample.c: h2v1_fancy_upsample, h2v2_fancy_upsample; replication for dw <= 2).
__device__ __forceinline__ int jpeg_chroma(const unsigned char* __restrict__ p, int stride, int y, int x, int hs, int vs, int dh, int dw) {
    if (hs == 1) return jpeg_sample(p, stride, y, x, dh, dw);
    const int i = x >> 1, r = vs == 2 ? y >> 1 : y;
    if (dw <= 2) return jpeg_sample(p, stride, r, i, dh, dw);
    const bool odd = x & 1;
    const int ni = odd ? i + 1 : i - 1;                      // the horizontal neighbour; outside [0, dw): the edge rule
    const bool edge = (unsigned)ni >= (unsigned)dw;
    if (vs == 1) {
        const int a = jpeg_sample(p, stride, r, i, dh, dw);
        if (edge) return a;
        return (3 * a + jpeg_sample(p, stride, r, ni, dh, dw) + (odd ? 2 : 1)) >> 2;
    }
    const int nr = min(max((y & 1) ? r + 1 : r - 1, 0), dh - 1);        // rows beyond the top / bottom replicate the first / last
    const int cs = 3 * jpeg_sample(p, stride, r, i, dh, dw) + jpeg_sample(p, stride, nr, i, dh, dw);
    const int bias = odd ? 7 : 8;
    if (edge) return (4 * cs + bias) >> 4;
    const int ns = 3 * jpeg_sample(p, stride, r, ni, dh, dw) + jpeg_sample(p, stride, nr, ni, dh, dw);
    return (3 * cs + ns + bias) >> 4;
}

__device__ __forceinline__ unsigned jpeg_clamp8(int v) { return (unsigned)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_color_u8_kernel(const fd_jpeg_color_job* __restrict__ jobs, const unsigned char* __restrict__ planes) {
    const fd_jpeg_color_job job = jobs[blockIdx.z];
    const unsigned total = (unsigned)job.width * (unsigned)job.height;       // < 2^32: both sides <= 65535
    const unsigned long first = ((unsigned long)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= total) return;
    const int w = job.width, h = job.height, hs = job.h_samp, vs = job.v_samp;
    const int dw = (w + hs - 1) / hs, dh = (h + vs - 1) / vs;
    const unsigned char* __restrict__ py = planes + job.plane_off[0];
    const unsigned char* __restrict__ pcb = planes + job.plane_off[1];
    const unsigned char* __restrict__ pcr = planes + job.plane_off[2];
    unsigned y = (unsigned)first / (unsigned)w, x = (unsigned)first - y * (unsigned)w;
    const unsigned npix = min(4u, total - (unsigned)first);
    unsigned char px[12];
#pragma unroll
    for (unsigned k = 0; k < 4; ++k) {
        unsigned r = 0, g = 0, b = 0;
        if (k < npix) {
            const int Y = jpeg_sample(py, job.stride[0], (int)y, (int)x, h, w);
            if (job.ncomp == 1) {
                r = g = b = (unsigned)Y;
            } else {
                const int cb = jpeg_chroma(pcb, job.stride[1], (int)y, (int)x, hs, vs, dh, dw) - 128;
                const int cr = jpeg_chroma(pcr, job.stride[2], (int)y, (int)x, hs, vs, dh, dw) - 128;
                r = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
                g = jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                b = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
            }
            if (++x == (unsigned)w) { x = 0; ++y; }
        }
        px[3 * k] = (unsigned char)r; px[3 * k + 1] = (unsigned char)g; px[3 * k + 2] = (unsigned char)b;
    }
    unsigned char* o = job.out + first * 3u;                 // 12 * lane bytes into a 4-byte aligned image: dword stores
    if (npix == 4) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
        for (int d = 0; d < 3; ++d) o4[d] = (unsigned)px[4 * d] | ((unsigned)px[4 * d + 1] << 8) | ((unsigned)px[4 * d + 2] << 16) | ((unsigned)px[4 * d + 3] << 24);
    } else {
        for (unsigned k = 0; k < 3 * npix; ++k) o[k] = px[k];   // the image's last one to three pixels
    }
}

extern "C" int32_t fd_jpeg_color_u8(const fd_jpeg_color_job* jobs_host, const fd_jpeg_color_job* jobs_dev, int32_t n_jobs, const uint8_t* planes,
                                    int64_t planes_bytes, fd_stream_t stream) {
    FD_REQUIRE(jobs_host && jobs_dev && planes, FD_E_INVAL, "fd_jpeg_color_u8: null pointer");
    FD_REQUIRE(n_jobs >= 1 && n_jobs <= 65535 && planes_bytes >= 1, FD_E_INVAL, "fd_jpeg_color_u8: bad job count %d or plane bytes %lld", n_jobs,
               (long long)planes_bytes);
    FD_REQUIRE(((uintptr_t)jobs_dev & 7) == 0, FD_E_INVAL, "fd_jpeg_color_u8: jobs not 8-byte aligned");
    int64_t max_pixels = 0;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const fd_jpeg_color_job& jb = jobs_host[i];
        FD_REQUIRE(jb.out && ((uintptr_t)jb.out & 3) == 0, FD_E_INVAL, "fd_jpeg_color_u8: job %d: null or not 4-byte aligned out", i);
        FD_REQUIRE(jb.width >= 1 && jb.height >= 1 && jb.width <= 65535 && jb.height <= 65535, FD_E_INVAL, "fd_jpeg_color_u8: job %d: sides %d x %d outside 1 .. 65535",
                   i, jb.height, jb.width);
        FD_REQUIRE(jb.ncomp == 1 || jb.ncomp == 3, FD_E_INVAL, "fd_jpeg_color_u8: job %d: %d components (1 or 3)", i, jb.ncomp);
        const bool samp_ok = (jb.h_samp == 1 && jb.v_samp == 1) || (jb.ncomp == 3 && jb.h_samp == 2 && (jb.v_samp == 1 || jb.v_samp == 2));
        FD_REQUIRE(samp_ok, FD_E_INVAL, "fd_jpeg_color_u8: job %d: luma sampling %d x %d (1x1, 2x1 or 2x2)", i, jb.h_samp, jb.v_samp);
        for (int c = 0; c < jb.ncomp; ++c) {
            const int64_t dw = c ? (jb.width + jb.h_samp - 1) / jb.h_samp : jb.width, dh = c ? (jb.height + jb.v_samp - 1) / jb.v_samp : jb.height;
            FD_REQUIRE(jb.stride[c] >= dw && jb.rows[c] >= dh, FD_E_INVAL, "fd_jpeg_color_u8: job %d: plane %d of %d x %d is smaller than the component", i, c,
                       jb.rows[c], jb.stride[c]);
            FD_REQUIRE(jb.plane_off[c] >= 0 && jb.plane_off[c] <= planes_bytes - (int64_t)jb.stride[c] * jb.rows[c], FD_E_INVAL,
                       "fd_jpeg_color_u8: job %d: plane %d outside the buffer", i, c);
        }
        const int64_t pixels = (int64_t)jb.width * jb.height;
        if (pixels > max_pixels) max_pixels = pixels;
    }
    const unsigned gx = (unsigned)((max_pixels + 1023) / 1024);
    hipLaunchKernelGGL(jpeg_color_u8_kernel, dim3(gx, 1, (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, jobs_dev, planes);
    FD_CHECK_LAUNCH("fd_jpeg_color_u8");
    return FD_OK;
}
