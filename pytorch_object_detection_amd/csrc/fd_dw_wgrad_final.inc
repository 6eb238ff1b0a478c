// fd_dw_wgrad_final.inc -- second phase of every depthwise weight gradient (fd_layers.hip: 3x3 and dilated k x k; fd_mbconv_bwd.hip: strided k x k):
// the fixed-order fp64 sum of the per-chunk partial sums part[chunk][T][C] -> dw, and the fixed row partition the first phases share.  Included by each
// translation unit that launches it (the library is built without relocatable device code, so a kernel cannot be launched across objects).
static __global__ __launch_bounds__(256) void dw_wgrad_final_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                     int n, int nchunk, const float* __restrict__ scale,
                                                                     int layout, int C, int T) {
    // 16 outputs x 16 chunk lanes per workgroup: lane j adds chunks j, j+16, ... in order, lanes are combined in order
    __shared__ double red[256];
    const int o = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + o;
    double s = 0.0;
    if (i < n)
        for (int k = j; k < nchunk; k += 16) s += (double)part[(long)k * n + i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (j == 0 && i < n) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += red[q * 16 + o];
        const int tap = i / C, c = i - tap * C;
        float v = (float)t;
        if (scale) v *= scale[c];
        dw[layout ? c * T + tap : i] = v;
    }
}

static inline int dw_wgrad_chunks(long rows) {
    long n = (rows + 63) / 64;
    if (n > 1024) n = 1024;
    if (n < 1) n = 1;
    return (int)n;
}

