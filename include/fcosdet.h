/*
 * fcosdet.h — C-ABI of libfcosdet_hip.so, the MI355X (gfx950) FCOS / HISFCOS hot path.
 *
 * Every entry point replaces a stock ATen / cuDNN / torchvision call the reference makes on its
 * detection hot path (citations are file:line under the reference repo root).  Conventions:
 *   - plain C, no torch types: every pointer is a DEVICE pointer owned by the caller
 *     (tensor.data_ptr()), sizes are int32, the last argument is the hipStream_t to enqueue on
 *     (torch.cuda.current_stream().cuda_stream on ROCm);
 *   - the library never allocates or frees user-visible memory; scratch comes from a caller
 *     workspace whose size the matching fd_*_workspace_bytes() call returns;
 *   - every call only enqueues work (no hidden synchronisation) and returns FD_OK or a negative
 *     error code; the message is available through fd_last_error() (thread local);
 *   - activations are fp32 NHWC ("rows x channels"): row m of a level is pixel
 *     (n, h, w) = (m / (H*W), (m / W) % H, m % W); a tensor may be a channel slice of a wider
 *     buffer, described by (ptr, channel stride cs, channel offset co):  elem = ptr[m*cs + co + c].
 *   - a pyramid (the 5 FCOS levels sharing head weights) is ONE buffer, levels concatenated along
 *     the row axis and described by fd_segs; a plain feature map is a pyramid with one segment.
 */
#ifndef FCOSDET_H_
#define FCOSDET_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_OK 0
#define FD_E_INVAL (-1)       /* bad argument (shape, alignment, null pointer)        */
#define FD_E_UNSUPPORTED (-2) /* valid request this build has no kernel for            */
#define FD_E_LAUNCH (-3)      /* hipLaunch / hipGetLastError failure                   */

#define FD_MAX_SEG 8

/* activation ids for conv / depthwise / groupnorm epilogues */
#define FD_ACT_NONE 0
#define FD_ACT_RELU 1
#define FD_ACT_SILU 2
#define FD_ACT_EXP 3 /* exp(v * seg_param[level])  — ScaleExp, reference model/modules/modules.py:170-176 */
#define FD_ACT_SIGMOID 4

typedef void* fd_stream_t; /* hipStream_t */

/* Pyramid-level table.  Rows of level s are [m_start[s], m_start[s+1]); m_start[s+1]-m_start[s] = batch*H[s]*W[s]. */
typedef struct fd_segs {
    int32_t nseg;
    int32_t batch;
    int32_t H[FD_MAX_SEG];
    int32_t W[FD_MAX_SEG];
    int32_t m_start[FD_MAX_SEG + 1];
} fd_segs;

/* ------------------------------------------------------------------------------------------- */
/* library                                                                                       */
int32_t fd_version(void);
const char* fd_last_error(void);

/* ------------------------------------------------------------------------------------------- */
/* Convolution = implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32), fused epilogue
 *     y = act( conv(x, w) * scale[c] + shift[c] + res )
 * replaces nn.Conv2d + (frozen) nn.BatchNorm2d + ReLU/SiLU (+ residual add) of
 *   torchvision resnet50 bottlenecks (reference model/backbone/resnet50.py:68-80),
 *   HalfInvertedStageFPN / HisBlock (model/od/HISFcos.py:77-179), HISFCOSHead (HISFcos.py:182-229),
 *   FeaturePyramidNetwork / HeadFCOS (model/od/Fcos.py:61-133).
 * w is packed [Cout][ceil(Cin/32)][KH][KW][32] (K contiguous, 32-channel chunk major, then filter tap; input
 * channels beyond Cin are zero).  Cin % 4 == 0 (a last partial chunk is read as zeros: EfficientNet widths such
 * as 24, 40, 48, 136, 144, 232, 816, 1392), x_cs % 4 == 0, x_co % 4 == 0.
 * in.nseg > 1 requires stride 1 and "same" padding (pad == dil*(K-1)/2).
 * mode FD_CONV_STEM: x is [N][H][W][4] (3 channels + zero pad), 7x7 stride 2 pad 3,
 *   w packed [Cout][7][8][4] (zeros at kw=7 and c=3).
 */
#define FD_CONV_GENERIC 0
#define FD_CONV_STEM 1

/* Arithmetic of the conv kernel.
 *  FD_PREC_F32   : v_mfma_f32_32x32x2_f32, bit-for-bit an fp32 fma chain (default, the parity baseline).
 *  FD_PREC_F16X3 : every fp32 operand is split x = hi + lo*2^-11 (hi, lo f16) and a product is three
 *                  v_mfma_f32_32x32x16_f16 (hi*hi + hi*lo + lo*hi, fp32 accumulation): error ~2^-22 per product,
 *                  operands must stay below f16's range (|x| < 65504).  Activations stay fp32 in HBM (split in the
 *                  loader); w is the pre-split packing [Cout][Cin/32][KH][KW][2][32] f16 (hi plane, lo plane). */
#define FD_PREC_F32 0
#define FD_PREC_F16X3 1
#define FD_PREC_F16 2   /* single-plane f16: operands rounded to f16 once (activations in the loader, weights at pack time: the hi plane of the
                           FD_PREC_F16X3 packing), ONE v_mfma_f32_32x32x16_f16 per product, fp32 accumulation and epilogue, fp32 output -- the
                           arithmetic of a convolution under torch.autocast(float16), which is how the reference trains (train.py:33,175-181).
                           Operands must stay inside f16's range.  Tiles: AUTO, 128x128(_SB), 128x64, 64x128, 64x64, 128x32, 128x96. */

/* block tiles (output pixels x output channels) of the conv kernel */
#define FD_TILE_AUTO 0
#define FD_TILE_128x128 1
#define FD_TILE_128x64 2
#define FD_TILE_64x128 3
#define FD_TILE_64x64 4
#define FD_TILE_128x32 5
#define FD_TILE_128x96 6
#define FD_TILE_128x128_SB 7 /* _SB: single LDS buffer (half the LDS, two barriers per K-tile) */
#define FD_TILE_128x64_SB 8
#define FD_TILE_64x128_SB 9
#define FD_TILE_256x128 10   /* 8 waves (512 threads), 4 x 2 wave tiles of 64 x 64 */
#define FD_TILE_256x128_SB 11
#define FD_TILE_128x96_SB 12
#define FD_TILE_128x128_PATCH 13 /* 3x3 stride-1 'same' convs only: the (128-row tile + halo) input patch is staged ONCE per
                                    32-channel chunk in LDS and the 9 taps are formed from it (9x less L2 -> LDS traffic for
                                    the activations); needs 128 + 2*dil*(W + 1) <= 320 rows, no split-K; FD_PREC_F32 / FD_PREC_F16X3
                                    (FD_PREC_F16 has no patch kernel: FD_E_UNSUPPORTED) */
#define FD_TILE_WINOGRAD 14 /* 3x3 stride-1 'same' convs (dilation 1 or 2), fp32: Winograd F(2x2, 3x3) on the fp32 MFMA -- 16 multiplies
                               per (cin, cout) and 2x2 output tile instead of 36 (fd_conv_wino.hip).  `w` must be the
                               fd_wino_pack_weights_f32 packing; Cin % 8 == 0, Cout % 4 == 0, 16-byte addressable y / res / scale /
                               shift; same epilogue contract incl. ksplit (chunk loop split over workgroups, combined in slice
                               order); the result differs from the direct kernel's fma chain by fp32 rounding (~1e-5 relative),
                               deterministically */
#define FD_TILE_WAVE64 15   /* GEMM-addressed layers (1x1, stride 1, no padding; Cin % 32 == 0, fp32): wave-autonomous 64 x 64 tiles, one wave per
                               workgroup, no barrier in the K loop (fd_conv_wave.hip) -- needs fd_conv_params.w_frag (fd_pack_conv_weight_wave_f32) */
#define FD_TILE_WINOGRAD4 16 /* 3x3 stride-1 'same' convs (dilation 1 or 2), fp32: Winograd F(4x4, 3x3) on the fp32 MFMA -- 36 multiplies per 4x4 output tile and
                                channel pair (2.25 per output: 1.78x fewer than F(2x2), 4x fewer than direct); needs the fd_wino4_pack_weights_f32 packing in `w`;
                                ksplit as FD_TILE_WINOGRAD; no gate / gn_stats.  Rounding error ~2x F(2x2)'s, inside the 1e-4 parity bar */
#define FD_TILE_NARROW 17    /* 3x3 stride-1 pad-1 convs with Cout <= 8 (the centre-ness + box-distance predictor, HISFcos.py:207-209), fp32, Cin % 16 == 0, no
                                residual / gn_stats / split-K: exact fp32 FMA chains on the VECTOR unit, one thread per output pixel (fd_conv_narrow.hip).
                                `gate` + `gate_b` (+ gate_act): the preceding GroupNorm's affine + activation applied to the patch on its way to LDS, zero
                                padding AFTER it as in the reference (any number of levels; coefficient rows as documented at gate_b below).
                                `w` = [Cin / 16][3 r][4 quads][3 q][4 k][8 couts] fp32: channel 16 chunk + 4 quad + k, filter tap (r, q); zero filters past Cout */
#define FD_TILE_F16K64 18    /* FD_PREC_F16 only (the AMP training step, train.py:175-181): f16 operands on K-tiles of 64 channels -- twice the matrix work per LDS tile of the
                                single-plane f16 instantiations of the other tiles, and activation maps stored as f16 (io_f16) go to LDS unconverted, 16 bytes per lane.  `w` = the
                                fd_pack_conv_weight_f32 mode | 16 packing; Cin % 64 == 0, x_cs / x_co multiples of 8, 4-channel aligned output / residual views; ReLU / SiLU / none;
                                any stride / dilation / pyramid / scatter; no split-K, gate, gn_stats, x2.  The library picks the block tile. */
#define FD_TILE_COUNT 19

typedef struct fd_conv_params {
    const float* x;
    const float* w;
    const float* scale; /* [Cout] or NULL (=1) */
    const float* shift; /* [Cout] or NULL (=0) */
    const float* res;   /* optional residual in output geometry, or NULL */
    float* y;
    int32_t x_cs, x_co;
    int32_t res_cs, res_co;
    int32_t y_cs, y_co;
    int32_t Cin, Cout, KH, KW, stride, pad, dil;
    int32_t act;    /* FD_ACT_* applied to output channels >= act_c0; channels below get identity */
    int32_t act_c0;
    int32_t mode;   /* FD_CONV_GENERIC | FD_CONV_STEM */
    int32_t tile;   /* 0 = built-in heuristic; FD_TILE_* forces a block tile (plan-time autotuning) */
    int32_t tag;    /* 1 = launch under a separate kernel symbol (<..., TAG=1>) so a profiler can isolate this layer */
    int32_t ksplit; /* <= 1: off.  > 1: split the K loop over `ksplit` workgroups per tile (finer work units for maps
                       with fewer tiles than CU slots); partial sums go to `workspace`, a second launch combines them
                       in slice order (deterministic) and applies the epilogue */
    void* workspace;           /* split-K scratch, fd_conv_workspace_bytes(out_rows, Cout, ksplit) bytes, 16-B aligned */
    int64_t workspace_bytes;
    int32_t precision; /* FD_PREC_F32 (exact fp32 MFMA) | FD_PREC_F16X3 (opt-in split-f16 products, see below) */
    int32_t res_mode;  /* what `res` does: 0 = added (residual connection); 1 = ReLU mask: y = res > 0 ? v : 0 -- the data
                          gradient of a layer whose input came out of a ReLU is masked in the epilogue that produces it
                          (train step: removes the separate threshold pass); 2 = `res` is a HALF-resolution map [N][H / 2][W / 2] added
                          AFTER the activation, y[n, i, j] = act(conv * scale + shift) + res[n, i / 2, j / 2]: an FPN lateral with the x2 nearest-
                          neighbour upsampling of the coarser level and the add folded into its epilogue (HISFcos.py:155-165, Fcos.py:77-91:
                          no upsample-add pass over the finer map).  fp32 1x1 stride-1 unpadded single-level convs with even H, W, Cin % 32 == 0,
                          16-byte views, no split-K / scatter / gate / gn_stats / x2; tiles AUTO, 64x64, 128x64_SB, 64x128_SB */
    float seg_param[FD_MAX_SEG]; /* per-level scalar for FD_ACT_EXP */
    fd_segs in;     /* input geometry */
    /* Data gradient of a STRIDED conv as parity classes (train.py:175-181; the 3x3 s2 / 1x1 s2 layers of the ResNet trunk):
     * dX pixels with (h % s, w % s) = (a, b) only see the filter taps r = (a + pad) % s + s*t, so each class is a stride-1
     * conv over dY with those taps (KH x KW may differ) whose outputs interleave into dX.  Single-level input only.
     *   out_H, out_W > 0: explicit output size (instead of the size derived from pad / K): taps past the input read zero;
     *   sc_H, sc_W > 0:   output pixel (n, i, j) is written to pixel (sc_sy*i + sc_oy, sc_sx*j + sc_ox) of an
     *                     [N][sc_H][sc_W] map at y (and `res` is read there); y_cs / y_co / res_* describe that map. */
    int32_t out_H, out_W;
    int32_t sc_sy, sc_sx, sc_oy, sc_ox, sc_H, sc_W;
    /* Per-(image, input channel) gate applied to the INPUT in the loader: y = act(conv(x * gate[n][c], w) * scale + shift + res).
     * The squeeze-excitation gate of an MBConv block (efficientnet_pytorch MBConvBlock: x * sigmoid(se_expand(...)), then _project_conv)
     * folded into the project conv: the scaling pass over the expanded map (a read and a write of it) disappears.  1x1 stride-1
     * unpadded convs on a single level, FD_PREC_F32, no split-K; gate is [batch][gate_cs] floats, gate_cs >= Cin, 16-byte aligned rows.
     * The library picks the block tile (tile / tag are ignored).  NULL = off. */
    const float* gate;
    int32_t gate_cs;
    int32_t reserved0;
    /* FD_TILE_WAVE64 only: the SAME weights as `w` in MFMA fragment order (fd_pack_conv_weight_wave_f32); NULL: that tile is unavailable.
     * A caller that holds both packings can switch tiles per launch (plan-time autotuning). */
    const float* w_frag;
    /* GroupNorm fused around the conv (HISFCOSHead, HISFcos.py:216-225: pw1 -> GN -> ReLU -> dw1 -> GN -> SiLU -> pw2; towers -> GN -> ReLU):
     *   gn_stats != NULL: the epilogue also writes, per output row m and channel group g of `gn_groups` groups over Cout, the fp32 pair
     *     (sum, sum of squares) of the group's STORED values to gn_stats[m][g] (float2; rows x gn_groups x 8 bytes) in a fixed summation order;
     *     fd_groupnorm_from_rowstats turns them into the per-(level, image, group) statistics -- the statistics pass over the map disappears.
     *     Needs Cout % 32 == 0, (Cout / gn_groups) in {4, 8, 16, 32}, 16-byte output views, no split-K, no output scatter.
     *   gate_b != NULL (with `gate`): the loader applies x' = act(x * gate[img][c] + gate_b[img][c]), gate_act in {NONE, RELU, SILU}, img =
     *     level * batch + image -- the GroupNorm affine + activation of the PRECEDING layer applied on the way to LDS (coefficients from
     *     fd_groupnorm_from_rowstats), so the normalise pass over the map disappears too.  `gate` alone keeps meaning x * gate (MBConv SE).
     *     Consumers: the 1x1 GEMM layers (above) and FD_TILE_NARROW (3x3, padded: the padding stays zero). */
    float* gn_stats;
    int32_t gn_groups;
    int32_t gate_act;
    const float* gate_b;
    /* A SECOND input whose channels continue the reduction (K-concatenation; 1x1 unpadded fp32 layers on a single level, no split-K / gate):
     *     y = act((x . W[:, :Cin]^T  +  x2' . W[:, Cin:]^T) * scale + shift (+ res)),   x2'[n, i, j] = x2[n, x2_stride * i, x2_stride * j]
     * with `w` the [Cout][Cin + x2_Cin] bank in the plain packing.  A ResNet bottleneck that changes resolution / width ends in
     * relu(bn3(conv3(o2)) + bn_d(downsample(x))) (torchvision Bottleneck.forward behind model/backbone/resnet50.py:68-80): with the BatchNorm scales
     * folded into the two filter banks this is ONE GEMM over K = planes + inplanes, and the 4 * planes wide identity map (420 MB per 16 images in
     * layer1) is neither written nor read back.  x2 is an [batch][x2_H][x2_W] NHWC map; Cin % 32 == 0, x2_Cin % 32 == 0.  NULL = off. */
    const float* x2;
    int32_t x2_cs, x2_co, x2_Cin, x2_stride, x2_H, x2_W;
    /* FD_TILE_WINOGRAD4 only: launch the workgroups [wg_first, wg_first + wg_count) of the layer's grid (fd_conv_workgroups(p) in all; wg_first % 8 == 0;
     * no split-K) instead of all of them -- the layer as several launches whose union is the layer.  One workgroup of that kernel owns a CU, so a grid that
     * is no multiple of the CU count ends in a round with most of the chip idle (the HISFCOS head tower at 16 x 640 x 640: 2 152 workgroups = 8.4 rounds
     * on 256 CUs); launched as whole rounds + a tail, the caller can schedule other work beside the tail (pipeline.TwoLanePipeline).  wg_count = 0: all. */
    int32_t wg_first, wg_count;
    /* FD_TILE_WINOGRAD4 only: the PERSISTENT stream-K form of the launch.  sk_wgs > 0 (a multiple of 8, at most the CU count: 256 on MI355X): that many workgroups, each
     * walks a contiguous, equally long range of the layer's (tile block, 8-channel chunk) units; an item cut by a range boundary is finished by the workgroup that holds its
     * first chunks, which adds the other parts' partial outputs (workspace slots, signalled through flags) in a fixed order -- deterministic, and bit-identical to the plain
     * launch for every item that is not cut.  The layer then takes total-work / CUs instead of whole rounds of workgroups (HISFCOS cls_logits, HISFcos.py:207: 538 items on
     * 256 CUs = 2.1 rounds that ran as 3), and a CU's items follow each other without a dispatch in between.  `workspace` = fd_conv_sk_workspace_bytes(sk_wgs) bytes,
     * 256-byte aligned, its first 8192 bytes (slot flags + the XCDs' queue heads: a fixed header, so launches with different sk_wgs may share a workspace that is large
     * enough for the largest) ZERO before the first launch (every launch leaves them zero); one workspace per concurrently running launch.  No split-K,
     * no wg_first / wg_count.  0: off. */
    int32_t sk_wgs;
    /* FD_PREC_F16 only: AMP activations stored as f16 in HBM (train.py:33,175-181 trains under torch.autocast: its convolutions read and write fp16 tensors).
     * Bit 0: `x` holds _Float16 elements, bit 1: `y`, bit 2: `res` (added or used as ReLU mask).  Channel strides / offsets stay in ELEMENTS; the loader fetches a
     * lane's four channels as 8 bytes and stores them to LDS unconverted, the epilogue rounds the fp32 accumulator result once (round to nearest even).  Plain
     * implicit-GEMM tiles (incl. split-K and the output scatter of strided data gradients); no gate / gn_stats / x2 / Winograd / narrow / wave / patch tiles.  0: fp32 maps. */
    int32_t io_f16;
} fd_conv_params;
/* Workspace bytes of the persistent stream-K form (flags + one 128 KB slot per workgroup); -1: sk_wgs not a multiple of 8 in 8 .. 1024. */
int64_t fd_conv_sk_workspace_bytes(int32_t sk_wgs);

int32_t fd_conv2d_nhwc_f32(const fd_conv_params* p, fd_stream_t stream);
/* Workgroups (grid.x) of the launch `p` describes -- FD_TILE_WINOGRAD4 only (FD_E_UNSUPPORTED otherwise): the range wg_first / wg_count index. */
int32_t fd_conv_workgroups(const fd_conv_params* p);
/* ... and how many workgroups of the slice `p` names (wg_count = 0: of the whole grid) own a tile -- the grid is padded to 8 XCD shares of equal size, the
 * padding workgroups exit at once: the work a slice does is live(slice) / live(all) of the layer's. */
int32_t fd_conv_workgroups_live(const fd_conv_params* p);
/* Two GEMM-addressed (1x1, stride 1, unpadded) layers back to back in ONE launch -- a ResNet bottleneck's conv3 + BN + residual + ReLU and the next
 * block's conv1 + BN + ReLU (torchvision Bottleneck.forward behind model/backbone/resnet50.py:68-80):
 *     y = act1(x . W1^T * scale1 + shift1 + res)   [rows][N1]   written to HBM (it is the next block's residual)
 *     z = act2(y . W2^T * scale2 + shift2)         [rows][N2]   computed from the rows of y while they are still on chip: y is not read back
 * w1_frag / w2_frag: the [N1][K1] / [N2][N1] filter banks in MFMA fragment order (fd_pack_conv_weight_wave_f32).  K1 % 32 == 0, N1 % 64 == 0,
 * N2 in {64, 128}; activations NONE / RELU / SILU; all views 16-byte addressable.  y and z are bit-identical to two fd_conv2d_nhwc_f32 launches. */
typedef struct fd_b2b_params {
    const float* x; const float* w1_frag; const float* scale1; const float* shift1; const float* res; float* y;
    const float* w2_frag; const float* scale2; const float* shift2; float* z;
    int32_t x_cs, x_co, res_cs, res_co, y_cs, y_co, z_cs, z_co;
    int32_t K1, N1, N2, act1, act2, reserved0;
    int64_t rows;
} fd_b2b_params;
int32_t fd_conv1x1_b2b_f32(const fd_b2b_params* p, fd_stream_t stream);
/* Accumulators per output pixel the FD_TILE_NARROW kernel instantiation of a Cout-channel layer carries (4, 5 or 8); -1: Cout not in 1..8. */
int32_t fd_conv_narrow_nco(int32_t Cout);
int64_t fd_conv_workspace_bytes(int64_t out_rows, int32_t Cout, int32_t ksplit);

/* Weights for FD_TILE_WINOGRAD4: OIHW fp32 [Cout][Cin][3][3] -> U = G g G^T (6x6 per filter, computed in double, rounded once) packed
 * [ceil(Cout/32)][Cin/8][36 frequencies][32 cout][8 cin] (fd_wino4_weight_bytes(Cout, Cin) bytes, zero rows past Cout). */
int64_t fd_wino4_weight_bytes(int32_t N, int32_t K);
/* mode 0: forward weights (N = Cout, K = Cin).  mode 1: data-gradient weights (N = Cin, K = Cout: taps flipped, channel roles swapped,
 * times scale[Cout] when given) -- as fd_wino_pack_weights_f32. */
int32_t fd_wino4_pack_weights_f32(const float* w, const float* scale, float* out, int32_t Cout, int32_t Cin, int32_t mode, fd_stream_t stream);

/* Weights for FD_TILE_WAVE64: [Cout][Cin] fp32 (an OIHW 1x1 filter bank, Cin % 32 == 0) -> MFMA fragment order
 * [ceil(Cout/64)][Cin/32][2 sub-tiles][4 k-steps][64 lanes][4 floats] (fd_conv_weight_wave_bytes bytes, zero rows past Cout): lane
 * (l & 31, l >> 5) of sub-tile j, k-step s, K-tile kt holds w[64 nt + 32 j + (l & 31)][32 kt + 8 s + 4 (l >> 5) + 0..3]. */
int64_t fd_conv_weight_wave_bytes(int32_t Cout, int32_t Cin);
int32_t fd_pack_conv_weight_wave_f32(const float* w, float* out, int32_t Cout, int32_t Cin, fd_stream_t stream);

/* Weights for FD_TILE_WINOGRAD: OIHW fp32 [Cout][Cin][3][3] -> U = G g G^T (computed in double, rounded once) packed
 * [ceil(Cout/32)][Cin/8][16 frequencies][32 cout][8 cin] (fd_wino_weight_bytes(Cout, Cin) bytes, zero rows past Cout).
 * mode 0: forward weights.  mode 1: weights of the stride-1 data-gradient conv (output channels = Cin, reduction over Cout,
 * Cout % 8 == 0): g'[ci][co][r][q] = g[co][ci][2-r][2-q] * (scale ? scale[co] : 1); buffer of fd_wino_weight_bytes(Cin, Cout). */
int64_t fd_wino_weight_bytes(int32_t Cout, int32_t Cin);
int32_t fd_wino_pack_weights_f32(const float* w, const float* scale, float* out, int32_t Cout, int32_t Cin, int32_t mode,
                                 fd_stream_t stream);

/* Convolution backward for the train step (reference train.py:175-181: scaler.scale(loss).backward() runs torch's
 * convolution_backward through cuDNN / MIOpen).
 *  - weight gradient: fd_conv2d_bwd_weight_f32, a pixel-reduction GEMM on the fp32 MFMA:
 *        dw[co][r][q][ci] = sum_m dy[m][co] * x[pix(m, r, q)][ci]          (dw is [Cout][KH][KW][Cin], OHWI)
 *    any stride / padding / dilation, pyramids included; Cin % 4 == 0, Cout % 4 == 0.
 *  - data gradient of a stride-1 layer: fd_conv2d_nhwc_f32 itself on dy with the weights flipped and transposed
 *    (w'[ci][co][r][q] = w[co][ci][KH-1-r][KW-1-q], pad' = dil*(K-1) - pad); needs Cout % 32 == 0.
 */
typedef struct fd_conv_wgrad_params {
    const float* x;  /* forward input rows  */
    const float* dy; /* gradient w.r.t. the forward output rows */
    float* dw;       /* [Cout][KH][KW][Cin] */
    int32_t x_cs, x_co, dy_cs, dy_co;
    int32_t Cin, Cout, KH, KW, stride, pad, dil;
    void* workspace; /* fd_conv_wgrad_workspace_bytes(out_rows, Cin, Cout, KH, KW) bytes, 16-B aligned */
    int64_t workspace_bytes;
    int32_t nsplit;  /* 0 = library chooses; else the pixel-range split count (workspace >= (nsplit + 8) * |dw| * 4 bytes:
                        ranges never cross a pyramid level, so every level adds at most one) */
    int32_t layout;  /* dw layout: 0 = [Cout][KH][KW][Cin] (OHWI), 1 = [Cout][Cin][KH][KW] (OIHW, torch's parameter layout) */
    const float* scale; /* optional [Cout]: dw[co] *= scale[co] (a frozen BatchNorm folded into the forward epilogue) */
    fd_segs in;      /* forward INPUT geometry */
    int32_t precision; /* FD_PREC_F32 (exact, default) | FD_PREC_F16: x and dy rounded to f16 on their way to LDS, v_mfma_f32_32x32x16_f16, fp32
                          accumulation -- the weight gradient of a convolution under torch.autocast(float16) (train.py:175-181) */
    int32_t io_f16;    /* FD_PREC_F16 only: bit 0: `x` holds _Float16 elements, bit 1: `dy` (AMP activations / gradients stored as f16: fetched as 8 bytes
                          per lane and staged without conversion; strides / offsets stay in elements).  0: fp32 maps */
} fd_conv_wgrad_params;

int64_t fd_conv_wgrad_workspace_bytes(int64_t out_rows, int32_t Cin, int32_t Cout, int32_t KH, int32_t KW);
int32_t fd_conv2d_bwd_weight_f32(const fd_conv_wgrad_params* p, fd_stream_t stream);
/* OIHW fp32 weights -> the [N][K/32][KH][KW][32] layout fd_conv2d_nhwc_f32 reads, in one pass (the per-step weight
 * preparation of the train step; plans pack once at build time).  mode 0: forward weights (N = Cout, K = Cin, Cin % 32
 * == 0).  mode 1: weights of the stride-1 data-gradient conv (N = Cin, K = Cout, Cout % 32 == 0):
 * w'[ci][co][r][q] = w[co][ci][KH-1-r][KW-1-q] * (scale ? scale[co] : 1).
 * mode | 4: the same weights in the FD_PREC_F16X3 / FD_PREC_F16 operand format [N][K/32][KH][KW][2][32] f16 (hi = f16(w) round-to-nearest,
 * lo = f16((w - hi) * 2^11)); the output buffer has the same byte size as the fp32 packing.
 * mode | 16 (not with | 4): FD_TILE_F16K64's operand -- f16 [N][K/64][KH][KW][64], K % 64 == 0; HALF the byte size of the fp32 packing. */
int32_t fd_pack_conv_weight_f32(const float* w, const float* scale, float* out, int32_t Cout, int32_t Cin, int32_t KH,
                                int32_t KW, int32_t mode, fd_stream_t stream);

/* The same for many weight tensors in ONE launch (a train step re-packs every layer after the optimizer update).
 * `jobs_dev` is a DEVICE array of n_jobs descriptors (pointers are device pointers; the caller checks the divisibility
 * rules of fd_pack_conv_weight_f32); max_elems = the largest Cout*Cin*KH*KW among them (sizes the grid). */
typedef struct fd_pack_job {
    const float* w;      /* [Cout][Cin][KH][KW] */
    const float* scale;  /* [Cout] or NULL (mode 1 only) */
    float* out;
    int32_t Cout, Cin, KH, KW, mode, reserved; /* mode: 0 / 1 (| 4 or | 16) as fd_pack_conv_weight_f32; 2 / 3 = the Winograd packing of fd_wino_pack_weights_f32 (mode 0 / 1), 8 / 9 = that of fd_wino4_pack_weights_f32; 3x3 only */
} fd_pack_job;
int32_t fd_pack_conv_weights_batch_f32(const fd_pack_job* jobs_dev, int32_t n_jobs, int64_t max_elems, fd_stream_t stream);

/* The ResNet stem as its own kernel: y = act(conv7x7_s2_p3(x) * scale + shift), 3 -> 64 channels, on the [N][H][W][4] image layout
 * (torchvision resnet50 conv1 + bn1 + relu behind the reference's model/backbone/resnet50.py:68-80).  The workgroup's input patch and
 * the filter bank are staged once in LDS, K = 7 x 22 (5 % padding; FD_CONV_STEM of fd_conv2d_nhwc_f32 pads 147 to 224).
 * w packed [7 filter rows][22][64]: k = 3 * (filter column) + (input channel), k = 21 zero.  Output [N][H/2][W/2] rows, 64 channels. */
int32_t fd_stem7x7_nhwc4(const float* x4, const float* w, const float* scale, const float* shift, float* y, int32_t y_cs, int32_t y_co,
                         int32_t N, int32_t H, int32_t W, int32_t act, fd_stream_t stream);

/* The stem WITH the max-pool that follows it (torchvision resnet50: conv1 + bn1 + relu + maxpool(3, stride 2, padding 1)) in one launch:
 * y_pooled [N][Hp][Wp] rows, 64 channels, Hp = (H/2 - 1) / 2 + 1.  The 64-channel stride-2 map is never written.  Windows that straddle two workgroups
 * are combined by integer atomicMax on the bits of the (non-negative, post-ReLU) values, starting from zeros that a first small launch of the same call
 * writes to exactly those pixels (two launches on `stream`; nothing outside y_pooled's 64-channel view is touched).  Bitwise reproducible. */
int32_t fd_stem7x7_pool_nhwc4(const float* x4, const float* w, const float* scale, const float* shift, float* y_pooled, int32_t y_cs, int32_t y_co,
                              int32_t N, int32_t H, int32_t W, fd_stream_t stream);

/* Both stem kernels reading the reference's own input tensor -- fp32 [N][3][H][W] (NCHW, dataset/voc.py:141-173), 4-byte aligned -- in their patch
 * loaders: no fd_nchw3_to_nhwc4 pass.  pool != 0: conv1 + bn1 + relu + maxpool as fd_stem7x7_pool_nhwc4 (y = the pooled map, act ignored); pool == 0:
 * as fd_stem7x7_nhwc4.  Same arithmetic and summation order: bit-identical to the nhwc4 entry points on the converted input. */
int32_t fd_stem7x7_nchw3(const float* x, const float* w, const float* scale, const float* shift, float* y, int32_t y_cs, int32_t y_co,
                         int32_t N, int32_t H, int32_t W, int32_t act, int32_t pool, fd_stream_t stream);

/* Weight gradient of the stem above (the image needs no gradient: there is no data-gradient kernel):
 *   dw[co][ci][ky][kx] = scale[co] * sum over (n, oy, ox) of g[n][oy][ox][co] * x4[n][2 oy - 3 + ky][2 ox - 3 + kx][ci],  taps outside the image contribute zero,
 * g = dy when y is NULL, else dy where y > 0 and 0 elsewhere (y = the forward output after ReLU: the mask is applied in the dy loader, no separate pass).
 * x4: the [N][H][W][4] image (channel 3 ignored).  dy and y: [N][H/2][W/2] rows, each a 64-CHANNEL VIEW of a rows buffer -- channel stride cs, first channel co,
 * cs % 4 == 0, co % 4 == 0, cs >= co + 64, base pointer 16-byte aligned; only those 64 channels of a row are read.  scale: optional [64] (a frozen BatchNorm folded
 * into the forward).  dw: [64][3][7][7], torch's OIHW layout.  H and W even and >= 2.  An fp32-MFMA GEMM (M = 64, N = 154 padded to 160, K = the output pixels);
 * the pixels are partitioned by (N, H, W) alone, every part's fp32 partial slab goes to `workspace`, and a second launch adds the slabs in index order in fp64:
 * two runs are bit-identical.  Two launches on `stream`, no host synchronisation, no allocation (safe under graph capture); nothing outside dw and the first
 * fd_stem7x7_wgrad_workspace_bytes(N, H, W) bytes of the 16-byte aligned workspace is written (-1: N < 1, or H / W odd or < 2).  A violated contract returns
 * FD_E_INVAL before any launch. */
int64_t fd_stem7x7_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W);
int32_t fd_stem7x7_bwd_weight_nhwc4(const float* x4, const float* dy, int32_t dy_cs, int32_t dy_co, const float* y, int32_t y_cs, int32_t y_co,
                                    const float* scale, float* dw, void* workspace, int64_t workspace_bytes, int32_t N, int32_t H, int32_t W,
                                    fd_stream_t stream);

/* [N][3][H][W] fp32 (NCHW, the reference's input layout, dataset/voc.py:141-173) -> [N][H][W][4] (c=3 zero) */
int32_t fd_nchw3_to_nhwc4(const float* x, float* y, int32_t N, int32_t H, int32_t W, fd_stream_t stream);
/* Input pipeline tail on the device: uint8 [N][H][W][3] images, already resized and zero padded
 * (dataset/voc.py:110-139; on the host, or by fd_resize_u8 below) -> normalised fp32
 * [N][H][W][4] = ((u8/255) - mean) / std per channel (transforms.ToTensor + Normalize, voc.py:57-58,104,155),
 * channel 3 = 0: the stem conv's input, no NCHW detour.  mean3 / std3 are HOST pointers to 3 floats. */
int32_t fd_preprocess_u8_nhwc4(const uint8_t* x, float* y, int32_t N, int32_t H, int32_t W, const float* mean3,
                               const float* std3, fd_stream_t stream);
/* Output pipeline tail (Test_coco.py:147-151): boxes /= scale, then xyxy -> xywh (COCO), in place on [n][4]. */
int32_t fd_boxes_rescale_xywh(float* boxes, int64_t n_boxes, float scale, fd_stream_t stream);
/* NHWC rows -> NCHW copy (only for callers that insist on contiguous NCHW); any channel view with x_cs >= x_co + C (scalar loads) */
int32_t fd_nhwc_to_nchw(const float* x, int32_t x_cs, int32_t x_co, float* y, int32_t N, int32_t HW,
                        int32_t C, fd_stream_t stream);

/* ------------------------------------------------------------------------------------------- */
/* Bandwidth-bound layer ops                                                                     */
/* Channel views (ptr, cs, co, C) of fd_maxpool[_bwd]_nhwc, fd_upsample2x_add_nhwc / fd_upsample2x_bwd_nhwc, fd_dwconv3x3[_gn]_nhwc,
 * fd_dwconv_dilated_nhwc, fd_dwconv2d_nhwc, fd_dwconv2d_bwd_data_nhwc / fd_dwconv2d_bwd_weight_nhwc, the other two depthwise weight gradients, fd_groupnorm_act / _apply / _stats / _act_bwd_nhwc,
 * fd_coef_apply_nhwc, fd_se_scale[_bwd]_nhwc, fd_act[_bwd]_nhwc[_h] and fd_batchnorm_sync_fwd / _bwd_nhwc are accessed four channels at a
 * time: C, cs and co are multiples of 4, cs >= co + C, ptr is 16-byte aligned (8-byte for the f16 maps of fd_act_bwd_nhwc_h); a view
 * that breaks this returns FD_E_INVAL before any launch (a width the kernel does not cover: FD_E_UNSUPPORTED).  In these entry points cs
 * and co enter the address computation only: a result does not depend, bit for bit, on the view geometry, nothing outside an output
 * view is written, and an output may be another channel slice of an input's buffer (tests/test_layer_views_gpu.py). */

/* nn.MaxPool2d(k, s, pad) on NHWC; k=3,s=2,pad=1 is the ResNet stem pool, k=2,s=2,pad=0 the FPN
 * down_sample{1..6} (HISFcos.py:131-136); optional fused "+ add" of a tensor in output geometry
 * (torch.add(p5_2, p4), HISFcos.py:168-177). */
int32_t fd_maxpool_nhwc(const float* x, int32_t x_cs, int32_t x_co, float* y, int32_t y_cs, int32_t y_co,
                        const float* add, int32_t add_cs, int32_t add_co, int32_t N, int32_t H, int32_t W,
                        int32_t C, int32_t k, int32_t s, int32_t pad, fd_stream_t stream);

/* y = nearest_upsample_x2(x) + lat      (nn.Upsample(scale_factor=2) + torch.add, HISFcos.py:155-165) */
int32_t fd_upsample2x_add_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* lat, int32_t lat_cs,
                               int32_t lat_co, float* y, int32_t y_cs, int32_t y_co, int32_t N, int32_t H,
                               int32_t W, int32_t C, fd_stream_t stream);

/* Depthwise 3x3, stride 1, pad 1 (DepthWiseConv2d, modules.py:40-49): y = act(dw(x)*scale + shift).
 * w packed [9][C]. */
int32_t fd_dwconv3x3_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* w, const float* scale,
                          const float* shift, float* y, int32_t y_cs, int32_t y_co, int32_t C, int32_t act,
                          const fd_segs* segs, fd_stream_t stream);

/* Weight gradient of the depthwise 3x3 conv above (stride 1, pad 1): dw[t][c] = sum_m x[pix(m, t)][c] * dy[m][c],
 * t = 3*r + q, same [9][C] layout as `w` (layout 0) or torch's [C][1][3][3] (layout 1); optional scale[C] multiplies
 * the result per channel (a frozen BatchNorm folded into the forward).  Replaces the depthwise half of torch's convolution_backward in the
 * reference's train step (train.py:175-181, modules.py:40-49).  The data gradient is fd_dwconv3x3_nhwc itself with the
 * taps reversed (w'[t] = w[8-t]).  Deterministic: fixed row partition, fixed-order fp64 final sum.
 * workspace: fd_dwconv3x3_wgrad_workspace_bytes(segs, C).  C/4 must divide 256 or be a multiple of 256. */
int64_t fd_dwconv3x3_wgrad_workspace_bytes(const fd_segs* segs, int32_t C);
int32_t fd_dwconv3x3_bwd_weight_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs,
                                     int32_t dy_co, float* dw, int32_t C, const float* scale, int32_t layout,
                                     const fd_segs* segs, void* workspace, fd_stream_t stream);

/* Dilated depthwise k x k convolution, stride 1, 'same' zero padding (pad = dil * (k - 1) / 2), y = act(dw(x) * scale + shift), over any
 * pyramid: MNBlock.DilatedDepthWiseConv + BN of the reference's model/modules/modules.py:195-216 (MNFCOS: model/od/MNFcos.py:222-297;
 * as shipped MNBlock pads with `dilation`, which keeps the size only for k = 3 -- its residual add raises for k = 5 / 7 -- the
 * 'same' padding is the repaired behaviour).  k in {3, 5, 7}; w packed [K*K][C] (tap major); C % 4 == 0. */
int32_t fd_dwconv_dilated_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* w, const float* scale, const float* shift,
                               float* y, int32_t y_cs, int32_t y_co, int32_t C, int32_t K, int32_t dil, int32_t act,
                               const fd_segs* segs, fd_stream_t stream);

/* Weight gradient of the dilated depthwise conv above: dw[t][c] = sum_m x[pix(m, t; dil)][c] * dy[m][c], t = K*r + q, over every level of the
 * segment table; k in {3, 5, 7}, 1 <= dil <= 8, C % 4 == 0.  layout 0 = [K*K][C] (the layout of `w`), 1 = torch's [C][1][K][K]; optional scale[C]
 * multiplies the result per channel (a frozen BatchNorm folded into the forward).  The data gradient is fd_dwconv_dilated_nhwc itself with the taps
 * reversed (w'[t] = w[K*K-1-t]: k is odd, the padding symmetric).  The backward of MNBlock.DilatedDepthWiseConv (modules.py:195-216) in the reference's
 * train step (train.py:175-181).  Deterministic: fixed row partition, fixed-order fp64 final sum of the chunk partials.  Allocates nothing:
 * workspace = fd_dwconv_dilated_wgrad_workspace_bytes(segs, C, K) bytes, 16-byte aligned (-1: bad table, C or K). */
int64_t fd_dwconv_dilated_wgrad_workspace_bytes(const fd_segs* segs, int32_t C, int32_t K);
int32_t fd_dwconv_dilated_bwd_weight_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co,
                                          float* dw, int32_t C, int32_t K, int32_t dil, const float* scale, int32_t layout,
                                          const fd_segs* segs, void* workspace, fd_stream_t stream);

/* Modulated deformable convolution ("DCNv2"): the sampler of the reference's DeformableConv2d (model/modules/modules.py:219-277, which calls
 * torchvision.ops.deform_conv2d) in front of the dense-conv GEMM.  groups = offset_groups = 1, square kernel, single level, fp32 maps.
 *   Ho = (H + 2*pad - dil*(K-1) - 1) / stride + 1, Wo likewise; tap t = i*K + j; offset rows [B*Ho*Wo][2*K*K]: channel 2t = dy, 2t+1 = dx;
 *   y = ho*stride - pad + i*dil + dy,  x = wo*stride - pad + j*dil + dx
 *   s_c(y, x) = 0 unless -1 < y < H and -1 < x < W (a NaN or infinite offset counts as outside); else with y0 = floor(y), x0 = floor(x), ly = y - y0, lx = x - x0:
 *               (1-ly)(1-lx) x[y0][x0] + (1-ly) lx x[y0][x0+1] + ly (1-lx) x[y0+1][x0] + ly lx x[y0+1][x0+1], a corner outside the map contributing 0
 *   cols[m][t*C + c] = mask[m][t] * s_c(y, x)      (mask = NULL: 1; mask_act = 1: `mask` holds logits v and the factor is 2 * sigmoid(v))
 * so that the layer is the 1x1 conv of `cols` (K*K*C channels, tap major then channel) with weight.permute(0, 2, 3, 1), and fd_conv2d_bwd_weight_f32 on
 * `cols` gives the weight gradient as [Cout][K][K][C].  This rule is the project's own statement of torchvision's published algorithm; it is not pinned
 * against torchvision (absent from this stack) but against the float64 reference tests/deform_ref.py.
 * x, cols (and dcols, d_x below) are channel views read four channels at a time (C % 4 == 0, cs and co multiples of 4, 16-byte aligned); offset and
 * mask (d_offset, d_mask) are channel views read one float at a time: any co >= 0 with cs >= co + 2*K*K (K*K) -- two slices of one side-conv output.
 * 1 <= K <= 7, 1 <= stride <= 4, 0 <= pad <= 7, 1 <= dil <= 4.  A bad argument returns FD_E_INVAL before any launch. */
int32_t fd_deform_im2col_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* offset, int32_t off_cs, int32_t off_co,
                              const float* mask, int32_t mask_cs, int32_t mask_co, int32_t mask_act, float* cols, int32_t cols_cs,
                              int32_t cols_co, int32_t B, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride, int32_t pad,
                              int32_t dil, fd_stream_t stream);
/* Backward of the sampler above from dcols (the gradient of `cols`): the exact derivatives of the piecewise-bilinear rule with floor() held constant
 * (at an integer coordinate: the ly = 0 / lx = 0 side); a fully outside sample gives zero to offset, mask and input.
 *   d_offset rows [B*Ho*Wo][2*K*K], d_mask rows [B*Ho*Wo][K*K] (with mask_act = 1: the gradient of the logits); mask and d_mask are both given or both NULL.
 *   Sums over the channels in a fixed order: deterministic, bit-identical from run to run.
 *   d_x (optional, NULL skips it) rows [B*H*W][C]: the caller zeroes it, the kernel ADDS each sample's four corner shares with fp32 atomic adds
 *   (one hardware add each).  They arrive in no fixed order: d_x is the one result of this layer that is not bit-reproducible. */
int32_t fd_deform_bwd_nhwc(const float* dcols, int32_t dcols_cs, int32_t dcols_co, const float* x, int32_t x_cs, int32_t x_co,
                           const float* offset, int32_t off_cs, int32_t off_co, const float* mask, int32_t mask_cs, int32_t mask_co,
                           int32_t mask_act, float* d_offset, int32_t doff_cs, int32_t doff_co, float* d_mask, int32_t dmask_cs,
                           int32_t dmask_co, float* d_x, int32_t dx_cs, int32_t dx_co, int32_t B, int32_t H, int32_t W, int32_t C,
                           int32_t K, int32_t stride, int32_t pad, int32_t dil, fd_stream_t stream);

/* Depthwise k x k convolution with stride and asymmetric zero padding, y = act(dw(x)*scale + shift): the depthwise
 * stage of an EfficientNet MBConv block (efficientnet_pytorch 0.7.1 MBConvBlock._depthwise_conv + _bn1 + swish, wrapped by
 * the reference's model/backbone/efficientnetv1.py:11-26; Conv2dStaticSamePadding pads (pad//2, pad - pad//2), i.e. more at
 * the bottom / right).  k in {3, 5, 7}, stride in {1, 2}; the caller states the top / left padding and the output size,
 * every tap outside the H x W input reads as zero.  w packed [K*K][C] (tap major).  Single level (no pyramid). */
int32_t fd_dwconv2d_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* w, const float* scale,
                         const float* shift, float* y, int32_t y_cs, int32_t y_co, int32_t N, int32_t H, int32_t W,
                         int32_t C, int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo,
                         int32_t act, fd_stream_t stream);
/* Backward of fd_dwconv2d_nhwc for the MBConv depthwise conv in the train step: k in {3, 5}, stride in {1, 2} (anything else: FD_E_UNSUPPORTED), the
 * same top / left padding and output size as the forward call, fp32 channel views under the contract above.  Any stream, no host synchronisation, no
 * float atomics, bitwise reproducible.  Bad views, a missing / misaligned workspace or an Ho x Wo that reaches past the input return FD_E_INVAL before
 * any launch.
 *   data gradient    dx[n,h,w,c] = scale[c] * sum_{r,s} dy[n,ho,wo,c] * w[r,s,c] over the taps with h + pad_top - r = stride * ho, 0 <= ho < Ho (same
 *                    along w); w [K*K][C] as the forward took it, scale optional (a folded frozen BatchNorm).  EVERY pixel of the dx view is written:
 *                    input rows / columns that no output window reaches come back 0.
 *   weight gradient  dw[r,s,c] = scale[c] * sum_{n,ho,wo} dy[n,ho,wo,c] * x[n, ho*stride - pad_top + r, wo*stride - pad_left + s, c] over the taps
 *                    inside the input; layout 0 = [K*K][C], 1 = [C][1][K][K]; workspace = fd_dwconv2d_wgrad_workspace_bytes(N, Ho, Wo, C, K)
 *                    bytes, 16-byte aligned (-1: bad size, C or K). */
int32_t fd_dwconv2d_bwd_data_nhwc(const float* dy, int32_t dy_cs, int32_t dy_co, const float* w, const float* scale, float* dx,
                                  int32_t dx_cs, int32_t dx_co, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride,
                                  int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, fd_stream_t stream);
int64_t fd_dwconv2d_wgrad_workspace_bytes(int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t K);
int32_t fd_dwconv2d_bwd_weight_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co, float* dw,
                                    int32_t C, int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t N, int32_t H, int32_t W,
                                    int32_t Ho, int32_t Wo, const float* scale, int32_t layout, void* workspace, fd_stream_t stream);
/* MBConv expand -> depthwise in ONE kernel (efficientnet_pytorch 0.7.1 MBConvBlock.forward behind model/backbone/efficientnetv1.py:11-26):
 *     y = swish(bn1(dwconv_kxk(swish(bn0(conv1x1(x, W_expand))))))   k in {3, 5}, stride in {1, 2}, static "SAME" padding (pad_top / pad_left; zeros on every side)
 * without the expanded map (six times the block input) ever reaching HBM: a workgroup stages the input patch of one TO x TO output tile in LDS, computes the expand
 * GEMM of the patch on the fp32 MFMA 32 expanded channels at a time and runs the depthwise conv from LDS.  It also writes the squeeze-excitation pooling's partial
 * sums -- pool[n][tile][c], fd_mbconv_pool_bytes() bytes -- so fd_se_gate_from_pool needs no pass over y.  Cin % 8 == 0 in 8 .. 48, mid % 4 == 0.
 * w_expand_frag: [ceil(mid / 32)][Cin / 8][2][32][4] floats, element (cb, g, h, l, jj) = W_expand[32 cb + l][h * (Cin / 2) + 4 g + jj] (rows >= mid zero); w_dw: [K * K][mid].
 * Results equal the separate launches up to the summation order of the expand GEMM. */
int64_t fd_mbconv_pool_bytes(int32_t N, int32_t Ho, int32_t Wo, int32_t mid, int32_t K, int32_t stride);
int32_t fd_mbconv_expand_dw_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* w_expand_frag, const float* scale0, const float* shift0,
                                 const float* w_dw, const float* scale1, const float* shift1, float* y, int32_t y_cs, int32_t y_co, float* pool,
                                 int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t mid, int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left,
                                 int32_t Ho, int32_t Wo, fd_stream_t stream);
/* The SE gates (fd_se_scale_nhwc with y = NULL) from those per-tile partial sums: T = tiles per image; workspace = fd_se_workspace_bytes(N, HW, C). */
int32_t fd_se_gate_from_pool(const float* pool, int32_t T, const float* w1, const float* b1, const float* w2, const float* b2, int32_t N, int32_t HW,
                             int32_t C, int32_t Cr, void* workspace, fd_stream_t stream);

/* 3-channel stem convolution (EfficientNet._conv_stem 3x3 stride 2 + _bn0 + swish) on the [N][H][W][4] image layout
 * fd_nchw3_to_nhwc4 / fd_preprocess_u8_nhwc4 / fd_collate_u8_nhwc4 produce: y = act(conv(x)*scale + shift).
 * w packed [K*K][4][Cout] (tap, input channel, output channel; input channel 3 is ignored).  K = 3, stride in {1, 2},
 * Cout % 4 == 0; padding as for fd_dwconv2d_nhwc. */
int32_t fd_stem_conv_nhwc4(const float* x4, const float* w, const float* scale, const float* shift, float* y,
                           int32_t y_cs, int32_t y_co, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t K,
                           int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, int32_t act,
                           fd_stream_t stream);

/* Weight gradient of the 3-channel stem convolution fd_stem_conv_nhwc4 (EfficientNet._conv_stem): K = 3, stride = 2, Cout % 4 == 0, Cout <= 64 (anything else:
 * FD_E_UNSUPPORTED).  dw[co][ci][ky][kx] = scale[co] * sum dy[n][oy][ox][co] * x4[n][2 oy - pad_top + ky][2 ox - pad_left + kx][ci]; taps outside the
 * image contribute zero, channel 3 of x4 is ignored, scale may be NULL.  dy: a Cout-channel view of the [N][Ho][Wo] rows.  dw: torch's [Cout][3][3][3].
 * Exact-fp32 MFMA over a fixed split of the output tiles (a function of the geometry alone); the slabs in `workspace`
 * (fd_stem_conv_wgrad_workspace_bytes, -1 for an unsupported shape) are added in index order in fp64 by a second launch: no atomics, bit-identical repeats. */
int64_t fd_stem_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t Ho, int32_t Wo);
int32_t fd_stem_conv_bwd_weight_nhwc4(const float* x4, const float* dy, int32_t dy_cs, int32_t dy_co, const float* scale, float* dw, void* workspace,
                                      int64_t workspace_bytes, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t K, int32_t stride,
                                      int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, fd_stream_t stream);

/* Mixed-aspect batch assembly on the device (dataset/voc.py:128-132 pad-to-32, :141-156 collate_fn):
 * N resized uint8 images of different sizes -> ONE normalised fp32 [N][H][W][4] batch (the stem's input layout).
 * images_dev: DEVICE array of N device pointers to [h_n][w_n][3] uint8; hw_dev: DEVICE int32 [N][2] = (h_n, w_n);
 * H, W >= every (h_n, w_n): the batch canvas (the host picks max over n of h_n + 32 - h_n % 32, as the reference does).
 * Pixels outside an image are uint8 zeros BEFORE normalisation, i.e. (0 - mean) / std, exactly what the reference's
 * zero-pad-then-Normalize produces.  The images are ALREADY resized (on the host, or by fd_resize_u8); raw images go
 * through fd_resize_collate_u8_nhwc4 below.  mean3 / std3 are HOST pointers to 3 floats. */
int32_t fd_collate_u8_nhwc4(const uint8_t* const* images_dev, const int32_t* hw_dev, float* y, int32_t N, int32_t H,
                            int32_t W, const float* mean3, const float* std3, fd_stream_t stream);

/* The resize of the input pipeline on the device: the cv2.resize call of preprocess_img_boxes
 * (dataset/voc.py:110-139, Test_coco.py:76-105).  Bilinear, half-pixel geometry (that of cv2.INTER_LINEAR and of torch's
 * align_corners=False), no antialiasing, 11-bit integer blending; per axis (source length S, destination length D, index d),
 * in fp32 without FMA contraction:
 *     x = (d + 0.5f) * ((float)S / (float)D) - 0.5f;  i0 = floor(x);  f = x - i0;
 *     i0 < 0: i0 = 0, f = 0;   i0 >= S - 1: i0 = S - 1, f = 0;   i1 = min(i0 + 1, S - 1);
 *     c1 = (int)floor(f * 2048.0f + 0.5f);  c0 = 2048 - c1;
 *     level = (p00*cx0*cy0 + p01*cx1*cy0 + p10*cx0*cy1 + p11*cx1*cy1 + (1 << 21)) >> 22          (uint32, per channel)
 * D == S is the identity.  The definition is this library's own and is unpinned against cv2 (third-party, absent here:
 * bit parity with cv2.resize is not claimed); it stays within 0.875 levels of exact bilinear interpolation
 * and tests/resize_ref.py restates it in numpy bit for bit.  The size rule (scale, int(scale * w), pad to 32) is host
 * arithmetic in doubles and stays with the caller (utill.utills.resize_rule).
 *
 * fd_resize_u8: one uint8 [h][w][3] image -> uint8 [nh][nw][3]; every side in 1 .. 65536. */
int32_t fd_resize_u8(const uint8_t* x, int32_t h, int32_t w, uint8_t* y, int32_t nh, int32_t nw, fd_stream_t stream);
/* Resize + pad-to-canvas + ToTensor + Normalize of a whole mixed-size batch in ONE launch: N RAW uint8 images ->
 * normalised fp32 [N][H][W][4], the stem's input layout.  images_dev: DEVICE array of N device pointers to [h_n][w_n][3]
 * uint8, as for fd_collate_u8_nhwc4; src_hw_dev / dst_hw_dev: DEVICE int32 [N][2] = (h_n, w_n) / (nh_n, nw_n), the
 * resized size of image n.  The output equals fd_collate_u8_nhwc4 on the images fd_resize_u8 produces, bit for bit:
 * pixels outside nh_n x nw_n are uint8 zero BEFORE normalisation, i.e. (0 - mean) / std, channel 3 = 0.
 * Checked here (FD_E_INVAL): pointers, alignment of y, N in 1 .. 65535, canvas sides in 1 .. 65536, non-zero std.  The
 * size tables are device memory and are not read by the host: the caller guarantees h_n, w_n >= 1 and nh_n <= H, nw_n <= W
 * (the Python wrapper checks); whatever they hold, the kernel reads inside [h_n][w_n][3] and writes inside the canvas only
 * (an entry with a side < 1 yields an all-padding image).  mean3 / std3 are HOST pointers to 3 floats. */
int32_t fd_resize_collate_u8_nhwc4(const uint8_t* const* images_dev, const int32_t* src_hw_dev, const int32_t* dst_hw_dev,
                                   float* y, int32_t N, int32_t H, int32_t W, const float* mean3, const float* std3,
                                   fd_stream_t stream);
/* Boxes between resized and source coordinates, in place on padded detections [B][K][4] (16-byte aligned): image b uses
 * scales_dev[b] (DEVICE fp32 [B]).  invert = 1: boxes / scale, IEEE fp32 division as fd_boxes_rescale_xywh and as
 * `boxes /= scale` of Test_coco.py:147; invert = 0: boxes * scale, the ground-truth side (dataset/voc.py:137-138).
 * xywh = 1: then xyxy -> xywh (Test_coco.py:150-151).  counts: DEVICE int32 [B] or NULL (all K rows); rows at or
 * beyond counts[b] are left untouched. */
int32_t fd_boxes_scale_batch(float* boxes, const int32_t* counts, const float* scales_dev, int32_t B, int32_t K,
                             int32_t invert, int32_t xywh, fd_stream_t stream);

/* The training-side augmentations on the device: the reference's flip (dataset/voc.py:12-20), Transforms
 * (data/augment.py: colorJitter, random_rotation, random_crop_resize), preprocess_img_boxes and collate_fn of a batch of
 * RAW uint8 [h][w][3] images.  The random decisions and the box arithmetic are host work (data/augment.py of the Python
 * package); the device gets one PARAMETER RECORD of FD_AUG_WORDS 32-bit words per image, in device memory:
 *
 *   FD_AUG_H, FD_AUG_W          raw image size
 *   FD_AUG_FLIP                 1: the image is mirrored left-right first (column x -> w - 1 - x)
 *   FD_AUG_ROT_ON               1: rotated by PIL's img.rotate (NEAREST, no expand, centre (w/2, h/2)) with the six 16.16
 *   FD_AUG_ROT0 .. +5           fixed-point integers (A0, A1, X0, A3, A4, Y0): destination (x, y) takes source pixel
 *                               ((X0 + A0*x + A1*y) >> 16, (Y0 + A3*x + A4*y) >> 16), black when that is outside.  The host
 *                               forms them in doubles as PIL does: angle = -radians(d mod 360), cos / sin rounded to 15
 *                               digits, a2 = cx - a0*cx - a1*cy (same for a5), FIX(v) = (int)(v * 65536 + (v < 0 ? -0.5 : 0.5)),
 *                               X0 = FIX(a2 + a0/2 + a1/2).  Sides <= 16384 and |d| < 90 keep every coordinate below 2^31 in
 *                               magnitude; the device forms the sums in 64-bit integers.
 *   FD_AUG_CROP_X, _Y, _W, _H   crop rectangle inside the (rotated) image; the whole image when there is no crop
 *   FD_AUG_NH, FD_AUG_NW        size the crop is resized to (bilinear, the arithmetic of fd_resize_u8)
 *   FD_AUG_NOPS                 length 0 .. FD_AUG_MAX_OPS of the colour chain, applied to the raw pixel in this order:
 *   FD_AUG_OP0 .. +3            FD_AUG_OP_* of each operation
 *   FD_AUG_ARG0 .. +3           its argument: the bits of the fp32 factor f, or for FD_AUG_OP_HUE the uint8 added to H
 *   FD_AUG_MEAN_L               the contrast operation's grey level int(mean(L) + 0.5); fd_jitter_l_sums fills it in
 *   remaining words             reserved, zero
 *
 * Colour arithmetic (each operation rounds to uint8, as PIL does between operations; fp32, no FMA contraction):
 *   brightness / contrast / saturation: level = clip((int)(deg + f * (pix - deg)), 0, 255) with deg = 0 / FD_AUG_MEAN_L /
 *   L of the pixel, L = (19595 R + 38470 G + 7471 B + 32768) >> 16 -- PIL's ImageEnhance.Brightness / Contrast / Color;
 *   hue: RGB -> HSV, H = (H + shift) & 255, HSV -> RGB with PIL's conversions.  All four are exact against PIL
 *   (tests/augment_ref.py restates them; checked over the whole 2^24 colour cube).
 *
 * fd_augment_resize_collate_u8: ONE launch per batch.  images_dev: DEVICE array of N device pointers; recs_dev: DEVICE
 * int32 [N][FD_AUG_WORDS]; y: PLANAR fp32 [N][3][H][W], what collate_fn returns and a model takes in train() mode.  Canvas
 * pixel (dy, dx) inside NH x NW: the four taps and 11-bit weights of the CROP_H x CROP_W -> NH x NW resize; each tap
 * + (CROP_Y, CROP_X) -> rotation map -> mirrored column -> raw bytes -> colour chain; blended, then Normalize with the
 * expression of fd_collate_u8_nhwc4.  Outside NH x NW: level 0 before Normalize.  The host side cannot read the records:
 * the caller validates them (the Python wrapper does); whatever they hold, a tap is loaded only after its final (row,
 * column) has been checked against [h][w] and only canvas pixels are written.  mean3 / std3 are HOST pointers.
 *
 * fd_jitter_l_sums: for every image whose chain holds FD_AUG_OP_CONTRAST, sums_dev[n] (DEVICE uint64 [N], cleared here) =
 * sum over the raw image of L after the operations that PRECEDE contrast, and FD_AUG_MEAN_L of its record =
 * (int)((double)sum / (h*w) + 0.5), PIL's ImageStat mean.  Integer sums, one 64-bit vector atomic per workgroup: exact
 * and order-independent.  max_pixels: the largest h*w of the batch (sizes the grid).  Run it before the fused launch when
 * any chain holds contrast.  Allocates nothing.
 *
 * fd_color_jitter_u8: one image through the chain of ONE record (device) -> uint8 [h][w][3]; x == y is allowed.
 * fd_rotate_u8: one image -> uint8 [h][w][3] by the six integers (HOST pointer); sides in 1 .. 16384, x != y. */
#define FD_AUG_WORDS 32
#define FD_AUG_H 0
#define FD_AUG_W 1
#define FD_AUG_FLIP 2
#define FD_AUG_ROT_ON 3
#define FD_AUG_ROT0 4
#define FD_AUG_CROP_X 10
#define FD_AUG_CROP_Y 11
#define FD_AUG_CROP_W 12
#define FD_AUG_CROP_H 13
#define FD_AUG_NH 14
#define FD_AUG_NW 15
#define FD_AUG_NOPS 16
#define FD_AUG_OP0 17
#define FD_AUG_ARG0 21
#define FD_AUG_MEAN_L 25
#define FD_AUG_MAX_OPS 4
#define FD_AUG_OP_BRIGHTNESS 1
#define FD_AUG_OP_CONTRAST 2
#define FD_AUG_OP_SATURATION 3
#define FD_AUG_OP_HUE 4
int32_t fd_augment_resize_collate_u8(const uint8_t* const* images_dev, const int32_t* recs_dev, float* y, int32_t N,
                                     int32_t H, int32_t W, const float* mean3, const float* std3, fd_stream_t stream);
int32_t fd_jitter_l_sums(const uint8_t* const* images_dev, int32_t* recs_dev, uint64_t* sums_dev, int32_t N,
                         int64_t max_pixels, fd_stream_t stream);
int32_t fd_color_jitter_u8(const uint8_t* x, int32_t h, int32_t w, uint8_t* y, const int32_t* rec_dev, fd_stream_t stream);
int32_t fd_rotate_u8(const uint8_t* x, int32_t h, int32_t w, uint8_t* y, const int32_t* fixed6, fd_stream_t stream);

/* Mosaic on the device: four augmented sources tiled around a centre on one H x W canvas per output, ONE launch
 * per batch, nothing allocated.  images_dev: DEVICE array of 4*N device pointers, tile t of output n at [4n + t] (a source
 * used several times is simply repeated); recs_dev: DEVICE int32 [4*N][FD_AUG_WORDS], the record above, one per tile;
 * place_dev: DEVICE int32 [N][FD_MOSAIC_WORDS]:
 *
 *   FD_MOSAIC_XC, FD_MOSAIC_YC    the centre: canvas pixel (dy, dx) belongs to tile t = 2 * (dy >= YC) + (dx >= XC)
 *                                 (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right)
 *   FD_MOSAIC_FILL                the level of pixels no tile covers, packed 0x00BBGGRR
 *   FD_MOSAIC_PX0 + 2t, + 2t + 1  (PXt, PYt): canvas position of tile t's pixel (0, 0); may be negative
 *   last word                     reserved, zero
 *
 * With ly = dy - PYt, lx = dx - PXt: when 0 <= ly < NH and 0 <= lx < NW of record 4n + t (and its H, W, CROP_W, CROP_H are
 * >= 1) the pixel is exactly what fd_augment_resize_collate_u8 produces at (ly, lx) for that record and source -- the same
 * taps, weights, crop / rotation / mirror maps, colour chain, blend and rounding (one shared device function); otherwise it is
 * FILL.  Then the same Normalize expression.  y: PLANAR fp32 [N][3][H][W].  A record's FD_AUG_MEAN_L is filled in by
 * fd_jitter_l_sums run on the same 4*N pointers and records.  Refused with FD_E_INVAL: a null pointer, y / records /
 * placements not 4-byte or the pointer table not 8-byte aligned, N outside 1 .. FD_MOSAIC_MAX_N (4*N must fit fd_jitter_l_sums),
 * canvas sides outside 1 .. 65536 or H*W >= 2^31, a zero std.  The tables cannot be read by the host; whatever they hold, a tap
 * is loaded only after its final (row, column) has been checked against the record's [h][w], only canvas pixels are written,
 * and XC, YC, PX, PY are only compared and subtracted in 64 bits.  mean3 / std3 are HOST pointers. */
#define FD_MOSAIC_WORDS 12
#define FD_MOSAIC_XC 0
#define FD_MOSAIC_YC 1
#define FD_MOSAIC_FILL 2
#define FD_MOSAIC_PX0 3
#define FD_MOSAIC_MAX_N 16383
int32_t fd_mosaic_collate_u8(const uint8_t* const* images_dev, const int32_t* recs_dev, const int32_t* place_dev, float* y,
                             int32_t N, int32_t H, int32_t W, const float* mean3, const float* std3, fd_stream_t stream);

/* GroupNorm(G, C) + activation (nn.GroupNorm in HISFCOSHead / HeadFCOS, HISFcos.py:190-204, Fcos.py:102-109).
 * Two launches: partial moments (fp64 accumulation, fixed order) then normalise+affine+act.
 * workspace: fd_groupnorm_workspace_bytes(segs, G). x and y may alias. */
int64_t fd_groupnorm_workspace_bytes(const fd_segs* segs, int32_t G);
int32_t fd_groupnorm_act_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta,
                              float* y, int32_t y_cs, int32_t y_co, int32_t C, int32_t G, float eps, int32_t act,
                              const fd_segs* segs, void* workspace, fd_stream_t stream);

/* Backward of the call above for the train step (reference train.py:175-181 differentiates nn.GroupNorm + ReLU / SiLU,
 * HISFcos.py:190-222): given dy (gradient w.r.t. the activated output) writes dx, dgamma[C], dbeta[C].
 * `fwd_workspace` is the forward call's workspace, unmodified (its partial moments give mean / rstd);
 * `workspace`: fd_groupnorm_bwd_workspace_bytes(segs, C).  act in {NONE, RELU, SILU}.  dx may alias dy.
 * fp64 partial sums in fixed order: deterministic. */
int64_t fd_groupnorm_bwd_workspace_bytes(const fd_segs* segs, int32_t C);
int32_t fd_groupnorm_act_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs,
                                  int32_t dy_co, const float* gamma, const float* beta, float* dx, int32_t dx_cs,
                                  int32_t dx_co, float* dgamma, float* dbeta, int32_t C, int32_t G, float eps,
                                  int32_t act, const fd_segs* segs, const void* fwd_workspace, void* workspace,
                                  fd_stream_t stream);

/* Squeeze-excitation (SEBlock, modules.py:107-121; also the SE stage of an EfficientNet MBConv block, whose middle
 * activation is the same swish): y = x * sigmoid(W2 silu(W1 mean_hw(x) + b1) + b2).
 * w1 [Cr][C], w2 [C][Cr]; C % 4 == 0, C <= 4096, Cr <= 1024.  workspace: fd_se_workspace_bytes(N, HW, C).  x and y may alias. */
int64_t fd_se_workspace_bytes(int32_t N, int32_t HW, int32_t C);
/* (y == NULL: compute the gates only -- they are left as [N][C] floats at byte offset fd_se_workspace_bytes(N, HW, C) - N * C * 4 of the
 *  workspace -- for a consumer that applies them itself: fd_conv_params.gate) */
int32_t fd_se_scale_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* w1, const float* b1,
                         const float* w2, const float* b2, float* y, int32_t y_cs, int32_t y_co, int32_t N,
                         int32_t HW, int32_t C, int32_t Cr, void* workspace, fd_stream_t stream);

/* Backward of the call above for the train step (train.py:175-181 differentiates HisBlock.conv1_2): dx and the gradients of
 * both 1x1 convs (dw1 [Cr][C], db1 [Cr], dw2 [C][Cr], db2 [C]).  `fwd_workspace` = the forward call's workspace, untouched
 * since (pooled sums, gates); `workspace`: fd_se_bwd_workspace_bytes(N, HW, C).  Deterministic (fixed-order sums). */
int64_t fd_se_bwd_workspace_bytes(int32_t N, int32_t HW, int32_t C);
int32_t fd_se_scale_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co,
                             const float* w1, const float* b1, const float* w2, const float* b2, float* dx, int32_t dx_cs,
                             int32_t dx_co, float* dw1, float* db1, float* dw2, float* db2, int32_t N, int32_t HW, int32_t C,
                             int32_t Cr, const void* fwd_workspace, void* workspace, fd_stream_t stream);

/* Elementwise activation y = act(x) on a channel view and its backward dx = dy * act'(x) (x = the saved INPUT):
 * nn.SiLU / nn.ReLU after a BatchNorm (HISFcos.py:100,112), ScaleExp (modules.py:170-176: FD_ACT_EXP, param = scale). */
int32_t fd_act_nhwc(const float* x, int32_t x_cs, int32_t x_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C,
                    int32_t act, float param, fd_stream_t stream);
int32_t fd_act_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co, float* dx,
                        int32_t dx_cs, int32_t dx_co, int64_t rows, int32_t C, int32_t act, float param, fd_stream_t stream);
/* The same pass over f16 maps (x, dy, dx hold _Float16 elements; 8-byte aligned views): AMP activations / gradients stored as f16 (train.py:175-181);
 * the derivative is evaluated in fp32 and the product rounded once. */
int32_t fd_act_bwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const void* dy, int32_t dy_cs, int32_t dy_co, void* dx,
                          int32_t dx_cs, int32_t dx_co, int64_t rows, int32_t C, int32_t act, float param, fd_stream_t stream);

/* Backward of fd_maxpool_nhwc (x = the forward input): dx[p] = sum of dy over the windows whose first maximum is p (the
 * argmax torch's max_pool2d keeps).  Gather form, deterministic.  The fused "+ add" passes dy through unchanged.
 * Backward of fd_upsample2x_add_nhwc w.r.t. its low-resolution input: dx = sum of the 2x2 block of dy (dy: [N][2H][2W]). */
int32_t fd_maxpool_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co, float* dx,
                            int32_t dx_cs, int32_t dx_co, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s,
                            int32_t pad, fd_stream_t stream);
int32_t fd_upsample2x_bwd_nhwc(const float* dy, int32_t dy_cs, int32_t dy_co, float* dx, int32_t dx_cs, int32_t dx_co, int32_t N,
                               int32_t H, int32_t W, int32_t C, fd_stream_t stream);

/* GroupNorm fused into its neighbours (HISFCOSHead, HISFcos.py:216-225).  A producer (fd_conv_params.gn_stats, fd_dwconv3x3_gn_nhwc) leaves
 * rowstats[m][g] = (sum, sum of squares) of group g's channels of row m (fp32 float2).  fd_groupnorm_from_rowstats reduces them per
 * (level, image, group) in fp64 in a fixed order into `workspace` (fd_groupnorm_workspace_bytes(segs, G): the layout fd_groupnorm_act_nhwc
 * leaves, so fd_groupnorm_apply_nhwc and fd_groupnorm_act_bwd_nhwc work on it) and, with coef != NULL, writes the affine a consumer applies
 * in its loader: coef[(level * batch + image)][0][c] = rstd * gamma[c], [..][1][c] = beta[c] - mean * rstd * gamma[c]  ([imgs][2][C] floats).
 * 2 * G must divide 256.  fd_groupnorm_apply_nhwc: y = act(x * a + b) from statistics already in `workspace` (one pass over the map).
 * fd_dwconv3x3_gn_nhwc: depthwise 3x3 (stride 1, pad 1, no bias) that reads its input as in_act(x * a + b) (in_coef as above, NULL: plain;
 * the zero padding is applied AFTER the normalisation, as in the reference) and writes gn_stats of its output (NULL: none). */
int32_t fd_groupnorm_from_rowstats(const float* rowstats, int32_t C, int32_t G, float eps, const float* gamma, const float* beta,
                                   const fd_segs* segs, void* workspace, float* coef, fd_stream_t stream);
int32_t fd_groupnorm_apply_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y,
                                int32_t y_cs, int32_t y_co, int32_t C, int32_t G, float eps, int32_t act, const fd_segs* segs,
                                const void* workspace, fd_stream_t stream);
/* The statistics steps of fd_groupnorm_act_nhwc alone (`workspace` as there) + optionally the affine `coef` [imgs][2][C] of
 * fd_groupnorm_from_rowstats: for a map whose consumers normalise it themselves (fd_conv_params.gate_b, fd_coef_apply_nhwc). */
int32_t fd_groupnorm_stats_nhwc(const float* x, int32_t x_cs, int32_t x_co, int32_t C, int32_t G, float eps, const float* gamma, const float* beta,
                                const fd_segs* segs, void* workspace, float* coef, fd_stream_t stream);
/* y = act(x * coef_a[img][c] + coef_b[img][c]) over a C-channel view, img = level * batch + image, coefficient rows coef_cs floats apart
 * (views into fd_groupnorm_from_rowstats' coef: a CHANNEL SLICE of a map whose statistics were reduced together with other channels -- the
 * class half of the head tower, whose box half is normalised inside the FD_TILE_NARROW predictor's loader).  C / 4 must divide 256. */
int32_t fd_coef_apply_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* coef_a, const float* coef_b, int32_t coef_cs, float* y,
                           int32_t y_cs, int32_t y_co, int32_t C, int32_t act, const fd_segs* segs, fd_stream_t stream);
int32_t fd_dwconv3x3_gn_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* w, const float* in_coef, int32_t in_act,
                             float* y, int32_t y_cs, int32_t y_co, int32_t C, float* gn_stats, int32_t gn_groups,
                             const fd_segs* segs, fd_stream_t stream);

/* nn.BatchNorm2d in TRAINING mode (the FPN BatchNorms under the reference's model.train(), train.py:151) runs on the
 * GroupNorm entry points: batch statistics per channel = GroupNorm statistics of ONE image of (batch*H) x W pixels with
 * G = C groups (fd_segs{nseg 1, batch 1, H = batch*H, W}); forward / backward are fd_groupnorm_act_nhwc /
 * fd_groupnorm_act_bwd_nhwc.  This call then folds the batch statistics the forward left in its workspace into the running
 * statistics (momentum update with the unbiased variance, as nn.BatchNorm2d). rows = batch*H*W. */
int32_t fd_batchnorm_update_running(const void* gn_workspace, int64_t rows, int32_t C, float momentum, float eps,
                                    float* running_mean, float* running_var, fd_stream_t stream);
/* The same with the row count in DEVICE memory (one double): nn.SyncBatchNorm's global count is the result of an all-reduce and differs
 * per step when the ranks' batches are padded to different H x W (dataset/voc.py:141-171); reading it here costs no host synchronisation. */
int32_t fd_batchnorm_update_running_dev(const void* gn_workspace, const double* count_dev, int32_t C, float momentum, float eps,
                                        float* running_mean, float* running_var, fd_stream_t stream);

/* nn.SyncBatchNorm in TRAINING mode (train.py:101-103: SyncBatchNorm.convert_sync_batchnorm after the DDP wrap; SURVEY 2.1 collective C3):
 * batch statistics over ALL ranks' rows.  Forward and backward are each cut in two around ONE all-reduce that the CALLER issues
 * (torch.distributed / RCCL; the library owns no communicator):
 *   forward   phase 1: sums[2c], sums[2c+1] = this rank's sum x, sum x^2 of channel c (fp64, fixed order)      -> all-reduce(sums, rows)
 *             phase 2: y = act((x - mean) * rstd * gamma + beta) with mean / rstd from the global sums and total_rows; (mean, rstd) stay in
 *                      `workspace` (fd_groupnorm_workspace_bytes of {1 image of rows x 1, G = C}) for the backward and for
 *                      fd_batchnorm_update_running(workspace, total_rows, ...)
 *   backward  phase 1: sums[c], sums[C+c] = this rank's sum dz, sum dz * xhat (dz = dy * act'); dgamma / dbeta from THESE local sums
 *                      (DDP averages them with the other gradients, as torch's SyncBatchNorm does)               -> all-reduce(sums)
 *             phase 2: dx = rstd * (gamma * dz - mean_global(gamma dz) - xhat * mean_global(gamma dz xhat))
 *   `workspace` of the backward: fd_groupnorm_bwd_workspace_bytes of the same segment table.  rows = this rank's batch*H*W.
 *   total_rows (phase 2): the GLOBAL row count as a host value, or <= 0: it is read on the device from sums[2C] -- the caller lets its own
 *   row count ride behind the 2C sums of the forward all-reduce ([2C + 1] doubles) and hands the backward a [2C + 1] buffer whose last word
 *   it copies from there (device to device): ranks whose batches are padded to different H x W (dataset/voc.py:141-171) then need no host
 *   round trip, and no rank assumes rows * world_size. */
int32_t fd_batchnorm_sync_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y,
                                   int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase,
                                   double* sums, double total_rows, void* workspace, fd_stream_t stream);
int32_t fd_batchnorm_sync_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co,
                                   const float* gamma, const float* beta, float* dx, int32_t dx_cs, int32_t dx_co, float* dgamma,
                                   float* dbeta, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums,
                                   double total_rows, const void* fwd_workspace, void* workspace, fd_stream_t stream);

/* nn.BatchNorm2d on BATCH statistics at any width: C % 4 == 0, 4 <= C <= 4096, 2 <= rows < 2^31, act in {NONE, RELU, SILU}, fp32 channel views under the layer
 * kernels' view contract (nothing outside the C-channel views is read or written).  The fd_groupnorm_* / fd_batchnorm_sync_* route above serves only the
 * widths whose quad count divides 256; these entry points serve every width (the EfficientNet trunk: 16 ... 2304; ResNet layer4: 2048).
 *   forward   y = act((x - mean) * rstd * gamma + beta) with the biased batch variance; running_mean / running_var (both or neither) are updated as
 *             nn.BatchNorm2d does (momentum, unbiased variance).  workspace = fd_batchnorm_train_workspace_bytes(rows, C) bytes, 8-byte aligned; the
 *             forward leaves double mean[C], double rstd[C] (rstd rounded to fp32) at its start for the backward.
 *   backward  dz = dy * act'(z) with z recomputed from x; dgamma = sum dz * xhat, dbeta = sum dz,
 *             dx = rstd * (gamma * dz - mean(gamma * dz) - xhat * mean(gamma * dz * xhat)).  fwd_workspace: the forward's; workspace: another of the same size.
 * Sums run in fp64 over a partition of the rows that is a function of (rows, C) alone and are added in index order: no atomics, two runs are bit-identical;
 * no host synchronisation, no allocation.  Statistics and apply are separate launches.  Wrong shapes / activations: FD_E_UNSUPPORTED, bad pointers, views or
 * workspaces: FD_E_INVAL, both before any launch.  The workspace query returns -1 for an unsupported shape. */
int64_t fd_batchnorm_train_workspace_bytes(int64_t rows, int32_t C);
int32_t fd_batchnorm_train_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y, int32_t y_cs,
                                    int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, float momentum, float* running_mean,
                                    float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream);
int32_t fd_batchnorm_train_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co, const float* gamma,
                                    const float* beta, float* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows,
                                    int32_t C, float eps, int32_t act, const void* fwd_workspace, void* workspace, int64_t workspace_bytes,
                                    fd_stream_t stream);

/* The same kernels for nn.SyncBatchNorm (statistics over ALL ranks' rows), each direction cut in two around ONE all-reduce that the CALLER issues, with the
 * argument conventions of fd_batchnorm_sync_*: phase in {1, 2}; sums = double[2C + 1], the global row count riding in sums[2C]; total_rows = the global row
 * count as a host value (>= this rank's rows, >= 2), or -1: read from sums[2C] on the device (ranks with different row counts need no host round trip).
 *   forward   phase 1: sums[c], sums[C + c] = this rank's sum x, sum x^2 of channel c; NOTHING else is written (not sums[2C], not the workspace's first
 *                      [2][C] block, not the running statistics, not y); gamma, beta, y may be NULL                         -> all-reduce(sums, count in sums[2C])
 *             phase 2: mean / rstd from the global sums and count into the workspace's first [2][C] block (the backward reads them there), the running
 *                      statistics updated with the global count, y = act((x - mean) * rstd * gamma + beta) on this rank's rows
 *   backward  phase 1: sums[c], sums[C + c] = this rank's sum dz, sum dz * xhat (global mean / rstd from fwd_workspace); dgamma / dbeta from THESE local sums
 *                      (DistributedDataParallel averages them, as with torch's SyncBatchNorm); dx may be NULL                        -> all-reduce(sums[0 .. 2C))
 *             phase 2: c1, c2 from the global sums and count into the workspace's first [2][C] block, then dx; dgamma, dbeta may be NULL
 * Both phases of a direction take the SAME workspace (fd_batchnorm_train_sync_workspace_bytes: the layout of fd_batchnorm_train_workspace_bytes, for
 * rows >= 1 -- a rank may hold one row, only the global count must reach 2).  At most two launches per phase, no atomics, no host synchronisation, no
 * allocation.  ONE rank (rows >= 2, sums handed from phase 1 to phase 2 untouched, total_rows = rows in either form) gives bit for bit what
 * fd_batchnorm_train_fwd_nhwc / _bwd_nhwc give: y, the statistics block, the running statistics, dx, dgamma, dbeta, the coefficient block.
 * FD_E_UNSUPPORTED: C % 4 != 0, C < 4, C > 4096, rows < 1, an activation outside {NONE, RELU, SILU}, phase outside {1, 2}.  FD_E_INVAL: 0 < total_rows < rows
 * (or < 2), bad pointers / views / alignment, a short workspace, running_mean without running_var.  Both before any launch. */
int64_t fd_batchnorm_train_sync_workspace_bytes(int64_t rows, int32_t C);
int32_t fd_batchnorm_train_sync_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y, int32_t y_cs,
                                         int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums, double total_rows,
                                         float momentum, float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                                         fd_stream_t stream);
int32_t fd_batchnorm_train_sync_bwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* dy, int32_t dy_cs, int32_t dy_co, const float* gamma,
                                         const float* beta, float* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows, int32_t C,
                                         float eps, int32_t act, int32_t phase, double* sums, double total_rows, const void* fwd_workspace, void* workspace,
                                         int64_t workspace_bytes, fd_stream_t stream);

/* The residual form of the two forwards above (the ResNet bottleneck's output relu(bn3(conv3(y2)) + identity) in one apply pass):
 *   y = act((x - mean) * rstd * gamma + beta + res),  act in {NONE, RELU}  (SILU: FD_E_UNSUPPORTED -- the backward takes its mask from y)
 * `res` is a fourth fp32 channel view under the same view rules; one float4 of it is read per float4 of x.  The statistics are those of x alone, so the
 * partition, the fp64 sums and their order, the statistics block, the running-statistics update, the workspace (fd_batchnorm_train_workspace_bytes /
 * fd_batchnorm_train_sync_workspace_bytes) and every error code are the plain forms'; phase 1 of the synchronised form does not read res (it may be NULL) and
 * writes exactly what the plain phase 1 writes.  y must not alias x or res.  There is no backward of its own: with g = dy * [y > 0] (fd_act_bwd_nhwc on the
 * saved output; g = dy for act NONE), g is the residual's gradient and fd_batchnorm_train_bwd_nhwc / _sync_bwd_nhwc with act NONE on g give dx, dgamma, dbeta. */
int32_t fd_batchnorm_train_res_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const float* res, int32_t res_cs,
                                        int32_t res_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act,
                                        float momentum, float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                                        fd_stream_t stream);
int32_t fd_batchnorm_train_sync_res_fwd_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const float* res,
                                             int32_t res_cs, int32_t res_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                                             int32_t act, int32_t phase, double* sums, double total_rows, float momentum, float* running_mean,
                                             float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream);

/* The six entry points above on f16 MAPS (torch.autocast(float16) with f16-stored activations and gradients, train.py:175-181): x, res, y, dy and dx hold
 * _Float16 elements on channel views that are 8-byte aligned, cs and co multiples of 4 (the rule of fd_act_bwd_nhwc_h); every other argument is the fp32
 * entry point's -- gamma, beta, dgamma, dbeta and the running statistics fp32, sums fp64, the same workspace (fd_batchnorm_train_workspace_bytes /
 * fd_batchnorm_train_sync_workspace_bytes) with mean / rstd and c1 / c2 as doubles in its first block, the same error codes in the same order, all before
 * any launch (SILU in the residual form: FD_E_UNSUPPORTED).  No atomics, no host synchronisation, no allocation; cs / co enter the address computation only
 * and nothing outside an output view is written.
 * The arithmetic is the fp32 kernels': the same kernel code instantiated on the element type, four halves per 8-byte access where the fp32 form moves a
 * float4.  An f16 element converts to fp32 exactly, the fp32 / fp64 operations run in the same order over the same (tile, chunk) partition, and y / dx are
 * rounded to f16 ONCE at the store, to nearest even, a value beyond 65504 becoming inf (not saturated: a GradScaler must see the overflow).  So for f16
 * inputs and their exact fp32 upcasts, y and dx equal round_f16(fp32 entry point's y / dx) bit for bit, and the statistics block, the coefficient block, the
 * running statistics, dgamma, dbeta and the phase-1 sums equal the fp32 entry point's bit for bit (tests/test_bn_f16_kernels_gpu.py).
 * The `_cma` forms below and the narrow route (fd_batchnorm_sync_*, fd_groupnorm_*) have no f16 form: these serve every width. */
int32_t fd_batchnorm_train_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, void* y, int32_t y_cs, int32_t y_co,
                                      int64_t rows, int32_t C, float eps, int32_t act, float momentum, float* running_mean, float* running_var,
                                      void* workspace, int64_t workspace_bytes, fd_stream_t stream);
int32_t fd_batchnorm_train_res_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const void* res, int32_t res_cs,
                                          int32_t res_co, void* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act,
                                          float momentum, float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                                          fd_stream_t stream);
int32_t fd_batchnorm_train_bwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const void* dy, int32_t dy_cs, int32_t dy_co, const float* gamma,
                                      const float* beta, void* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows, int32_t C,
                                      float eps, int32_t act, const void* fwd_workspace, void* workspace, int64_t workspace_bytes, fd_stream_t stream);
int32_t fd_batchnorm_train_sync_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, void* y, int32_t y_cs,
                                           int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums, double total_rows,
                                           float momentum, float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                                           fd_stream_t stream);
int32_t fd_batchnorm_train_sync_res_fwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const void* res,
                                               int32_t res_cs, int32_t res_co, void* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                                               int32_t act, int32_t phase, double* sums, double total_rows, float momentum, float* running_mean,
                                               float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream);
int32_t fd_batchnorm_train_sync_bwd_nhwc_h(const void* x, int32_t x_cs, int32_t x_co, const void* dy, int32_t dy_cs, int32_t dy_co, const float* gamma,
                                           const float* beta, void* dx, int32_t dx_cs, int32_t dx_co, float* dgamma, float* dbeta, int64_t rows, int32_t C,
                                           float eps, int32_t act, int32_t phase, double* sums, double total_rows, const void* fwd_workspace,
                                           void* workspace, int64_t workspace_bytes, fd_stream_t stream);

/* The cumulative moving average, nn.BatchNorm2d(momentum=None): every entry point above that takes `float momentum` has a `_cma` sibling that takes the
 * layer's num_batches_tracked in DEVICE memory instead (one int64, 8-byte aligned, already incremented for this batch: the host enqueues add_(1) before the
 * call).  The lanes that blend the running statistics read it and use momentum = (float)(1.0 / (double)n): no launch more, nothing read on the host, so a
 * captured forward follows the counter.  CONTRACT: for a counter holding n >= 1 a `_cma` call is BIT FOR BIT its plain sibling called with
 * momentum = (float)(1.0 / n) -- y, the statistics block, both running tensors.  n < 1 writes neither running tensor; y and the statistics block are written
 * as always.  Everything else (shapes, partition, fp64 sums, workspaces, error codes) is the plain sibling's.  FD_E_INVAL before any launch: running tensors
 * with a null or misaligned counter, one running tensor without the other.  Null running tensors (the counter may then be null too) update no statistics.
 * Phase 1 of the synchronised forms does not look at the counter.  The backwards are the plain ones. */
int32_t fd_batchnorm_update_running_cma(const void* gn_workspace, int64_t rows, int32_t C, const int64_t* num_batches_tracked, float eps,
                                        float* running_mean, float* running_var, fd_stream_t stream);
int32_t fd_batchnorm_update_running_dev_cma(const void* gn_workspace, const double* count_dev, int32_t C, const int64_t* num_batches_tracked, float eps,
                                            float* running_mean, float* running_var, fd_stream_t stream);
int32_t fd_batchnorm_train_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y, int32_t y_cs,
                                        int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, const int64_t* num_batches_tracked,
                                        float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream);
int32_t fd_batchnorm_train_res_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const float* res,
                                            int32_t res_cs, int32_t res_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                                            int32_t act, const int64_t* num_batches_tracked, float* running_mean, float* running_var, void* workspace,
                                            int64_t workspace_bytes, fd_stream_t stream);
int32_t fd_batchnorm_train_sync_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, float* y, int32_t y_cs,
                                             int32_t y_co, int64_t rows, int32_t C, float eps, int32_t act, int32_t phase, double* sums,
                                             double total_rows, const int64_t* num_batches_tracked, float* running_mean, float* running_var,
                                             void* workspace, int64_t workspace_bytes, fd_stream_t stream);
int32_t fd_batchnorm_train_sync_res_fwd_cma_nhwc(const float* x, int32_t x_cs, int32_t x_co, const float* gamma, const float* beta, const float* res,
                                                 int32_t res_cs, int32_t res_co, float* y, int32_t y_cs, int32_t y_co, int64_t rows, int32_t C, float eps,
                                                 int32_t act, int32_t phase, double* sums, double total_rows, const int64_t* num_batches_tracked,
                                                 float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes, fd_stream_t stream);

/* Drop-connect (stochastic depth) on [N][HW][C] fp32 channel views: y = a * s[n] + r, s = N floats on the device, r may be NULL; y may alias a.
 * Two roundings, like the torch expression a * s + r. */
int32_t fd_sample_scale_add_nhwc(const float* a, int32_t a_cs, int32_t a_co, const float* s, const float* r, int32_t r_cs, int32_t r_co, float* y,
                                 int32_t y_cs, int32_t y_co, int32_t N, int32_t HW, int32_t C, fd_stream_t stream);

/* ------------------------------------------------------------------------------------------- */
/* Detection post-processing (reference model/modules/head.py:8-102,152-162, utill/utills.py:58-73)   */

/* Per location: score = sqrt(max_c sigmoid(cls) * sigmoid(cnt)), class = argmax_c + 1 (first max),
 * box = (cx - l, cy - t, cx + r, cy + b), (cx, cy) = (x*s + s/2, y*s + s/2).
 * cls/cnt/reg are pyramid buffers (rows x C / 1 / 4 with channel strides).  Outputs are per image,
 * levels concatenated in segment order, row-major inside a level: scores [N][L], classes [N][L]
 * (int32), boxes [N][L][4], L = sum H*W. */
int32_t fd_fcos_decode(const float* cls, int32_t cls_cs, int32_t cls_co, const float* cnt, int32_t cnt_cs,
                       int32_t cnt_co, const float* reg, int32_t reg_cs, int32_t reg_co, int32_t num_classes,
                       const fd_segs* segs, const int32_t* strides, float* scores, int32_t* classes,
                       float* boxes, fd_stream_t stream);

/* torch.topk(score, K, dim=1, largest=True, sorted=True) + gathers (head.py:69-80).  Ties: lower
 * location index first.  Outputs [N][K]; top_idx (int32 location index) may be NULL.  K <= 1024 runs in LDS / registers with no
 * workspace (fd_topk_workspace_bytes = 0); any larger K <= L (FCOSHead accepts any max_detection_box, head.py:41-50) sorts its candidate
 * list in `workspace` (fd_topk_workspace_bytes bytes, 8-byte aligned). */
int64_t fd_topk_workspace_bytes(int32_t N, int32_t L, int32_t K);
int32_t fd_fcos_topk(const float* scores, const int32_t* classes, const float* boxes, int32_t N, int32_t L,
                     int32_t K, float* top_scores, int64_t* top_classes, float* top_boxes, int32_t* top_idx,
                     void* workspace, fd_stream_t stream);

/* score >= score_thr mask + torchvision.ops.batched_nms (coordinate-offset trick) + gathers
 * (FCOSHead.post_process, head.py:84-102).  Input rows must be score-descending (fd_fcos_topk
 * output).  Greedy rule: suppress j when (double)iou(i,j) > iou_thr, iou on class-offset boxes
 * without the "+1" pixel convention.  Outputs padded to [N][K] (rows >= counts[n] zero-filled),
 * keep_idx[n][r] = index into the K input rows.  K <= 1024: two launches, the suppression bitmask is built by
 * K/64 workgroups per image into `workspace` (fd_nms_workspace_bytes), one workgroup per image then scans it in LDS.  K > 1024
 * (up to 262144): the same rule with the class-offset boxes and bitmask rows of ceil(K/64) words in the workspace (three launches).
 * Outputs must not alias inputs. */
int64_t fd_nms_workspace_bytes(int32_t N, int32_t K);
int32_t fd_batched_nms(const float* scores, const int64_t* classes, const float* boxes, int32_t N, int32_t K,
                       float score_thr, double iou_thr, float* out_scores, int64_t* out_classes,
                       float* out_boxes, int32_t* keep_idx, int32_t* counts, void* workspace, fd_stream_t stream);

/* Class-agnostic greedy NMS with the "+1" pixel convention, keep while ovr <= (float)thr
 * (DataEncoder._box_nms, utill/utills.py:221-255; mode 0 = 'union', 1 = 'min').
 * One problem per call-row: boxes [N][K][4], scores [N][K] (any order; sorted internally,
 * ties by lower index), n_valid [N] or NULL (=K).  keep_idx [N][K] (original indices, score
 * descending), counts [N].  K <= 1024. */
int32_t fd_box_nms_plus1(const float* boxes, const float* scores, const int32_t* n_valid, int32_t N, int32_t K,
                         float thr, int32_t mode, int32_t* keep_idx, int32_t* counts, fd_stream_t stream);

/* Pairwise IoU [Na][Nb]; plus_one=1: DataEncoder._box_iou (utills.py:201-218); 0: test.py:23-53 */
int32_t fd_pairwise_iou(const float* a, const float* b, int32_t Na, int32_t Nb, int32_t plus_one, float* out,
                        fd_stream_t stream);

/* ClipBoxes (head.py:152-162): clamp(min 0), x <= W-1, y <= H-1, in place on [n_boxes][4] */
int32_t fd_clip_boxes(float* boxes, int64_t n_boxes, int32_t img_h, int32_t img_w, fd_stream_t stream);

/* Detection records for the ONE collective of image-sharded multi-GPU inference: the padded
 * outputs of fd_batched_nms of B images as one fp32 message records[B][K+1][6]:
 *   records[b][0] = (counts[b], 0, 0, 0, 0, 0);  records[b][1+r] = (x1, y1, x2, y2, score, class), r < K.
 * Counts and class ids are < 2^24, exact in fp32.  fd_unpack_detections is the inverse (on the gathered [W*B] images). */
int32_t fd_pack_detections(const float* scores, const int64_t* classes, const float* boxes, const int32_t* counts,
                           int32_t B, int32_t K, float* records, fd_stream_t stream);
int32_t fd_unpack_detections(const float* records, int32_t B, int32_t K, float* scores, int64_t* classes, float* boxes,
                             int32_t* counts, fd_stream_t stream);

/* ------------------------------------------------------------------------------------------- */
/* VOC average precision (reference test.py:15-20 sort_by_score + 23-162 iou_2d / _compute_ap / eval_ap_2d, the mAP of
 * evaluate 225-238), whole computation on the device.  Inputs (device memory): detections scores [N][K] fp32, classes [N][K]
 * int64 (1-based, as FCOSHead emits), boxes [N][K][4] fp32 xyxy, det_counts [N] int32 or NULL (= K: rows >= count are ignored);
 * GT boxes [N][G][4] fp32, classes [N][G] int64, gt_counts [N] or NULL (= G).  Rows whose label is outside 1 .. num_cls-1 never
 * take part (class 0, the collate's -1 padding, labels >= num_cls).  thresholds: HOST array of n_thr fp32 IoU thresholds.
 * Semantics, per label 1 .. num_cls-1 and threshold:
 *   - each image's detections in descending score order (ties: lower row first); flags & FD_EVAL_INPUT_ORDER: in row order
 *     instead (eval_ap_2d takes its lists as given, sort_by_score is a separate step);
 *   - no GT box of the label in the image: false positive.  Else IoU against each GT box of the label in row order, fp32 without
 *     the "+1" convention: w = max(0, min(x2) - max(x1)), h alike, overlap = w * h, iou = overlap / ((area_gt + area_det) - overlap);
 *     min / max propagate NaN as np.minimum / np.maximum do (a NaN coordinate gives a NaN IoU);
 *     j = argmax, first maximum, a NaN wins (first NaN; zero-area GT against a zero-area detection);
 *   - TP iff iou[j] >= thr (fp32 compare; NaN never) and GT box j of the image is not yet assigned; a TP assigns j.  An assigned
 *     j makes the detection a false positive: there is no fall-back to the next-best box;
 *   - the label's detections of all images in (image, rank) order, sorted by descending score, STABLE (the reference's
 *     np.argsort is an unstable quicksort: the only intended difference, visible only on exactly equal scores);
 *   - fp64 running tp / fp, recall = tp / n_gt, precision = tp / max(tp + fp, eps); AP = sum over the recall change points of
 *     (mrec[i+1] - mrec[i]) * envelope(mpre)[i+1] with sentinels mrec = [0, r.., 1], mpre = [0, p.., 0], summed in numpy's
 *     pairwise order (8 accumulators, blocks of 128, halves rounded to multiples of 8): bit-identical to numpy;
 *   - n_gt > 0 and no detection: 0.0; detections but n_gt == 0: NaN (recall 0 / 0); neither: 0.0.
 * Outputs (device): ap [n_thr][num_cls] fp64, n_gt [num_cls], n_pred [num_cls], n_tp [n_thr][num_cls] int32; column 0 (background)
 * is 0.  Limits: K <= 1024, G <= 512, 2 <= num_cls <= 128, n_thr <= 16, N * K < 2^31 (FD_E_UNSUPPORTED names the limit).
 * Deterministic: no output depends on the order of atomics.  Boxes 16-byte aligned; workspace (fd_eval_ap_workspace_bytes:
 * about 25 bytes per detection row, linear in N * K) 256-byte aligned.  21 launches on `stream`, no host synchronisation. */
#define FD_EVAL_INPUT_ORDER 1
int64_t fd_eval_ap_workspace_bytes(int32_t N, int32_t K, int32_t G, int32_t num_cls, int32_t n_thr);
int32_t fd_eval_ap(const float* det_scores, const int64_t* det_classes, const float* det_boxes, const int32_t* det_counts, int32_t N,
                   int32_t K, const float* gt_boxes, const int64_t* gt_classes, const int32_t* gt_counts, int32_t G, int32_t num_cls,
                   const float* thresholds, int32_t n_thr, int32_t flags, double* ap, int32_t* n_gt, int32_t* n_pred, int32_t* n_tp,
                   void* workspace, fd_stream_t stream);

/* ------------------------------------------------------------------------------------------- */
/* COCO bbox evaluation: pycocotools COCOeval (iouType 'bbox', useCats) evaluate() + accumulate(), whole computation on the device.
 * Inputs (device memory): detections scores [N][K] fp32, labels [N][K] int64 (1 .. num_cats; anything else takes no part), boxes
 * [N][K][4] fp32 xywh, det_counts [N] int32 or NULL (= K); GT boxes [N][G][4] fp64 xywh, annotation area [N][G] fp64, iscrowd [N][G]
 * uint8, labels [N][G] int64 (1 .. num_cats; -1 = padding); image_order [N] int32 or NULL: position p evaluates image image_order[p]
 * (a permutation; positions order score ties across images).  HOST arrays: iou_thrs [n_thr] fp64, rec_thrs [n_rec] fp64 (ascending),
 * area_rng [n_area][2] fp64 (inclusive), max_dets [n_maxdet] int32 (ascending).  Semantics, per (image, label):
 *   - detections by descending score, stable over rows; only the first max_dets[-1] take part (the cut is per (image, label));
 *   - IoU fp64 in maskApi bbIou's order: w = fmin(dx+dw, gx+gw) - fmax(dx, gx), h alike, <= 0 gives 0; u = da + ga - i with
 *     w * h box areas, u = da for a crowd GT;
 *   - per area range a GT row is ignored if crowd or its annotation area is outside the range; per threshold t (as min(t, 1-1e-10))
 *     each detection in score order takes the LAST GT row with the maximal IoU >= t among the non-ignored rows not yet taken (crowd
 *     rows are never taken), else among the ignored ones; matched to an ignored row, or unmatched with w * h outside the range:
 *     ignored;
 * then per (label, area, maxDet): each image's first maxDet detections in position order, stably sorted by descending score; fp64
 * tp / fp cumulative sums over the non-ignored, rc = tp / npig, pr = tp / (fp + tp + 2^-52), the right-to-left envelope,
 * precision[r] = pr at searchsorted(rc, rec_thrs[r], 'left') (0 past the end), recall = rc[-1] (0 without detections); npig == 0
 * leaves -1 in both.
 * Outputs (device): precision [n_thr][n_rec][num_cats][n_area][n_maxdet] fp64, recall [n_thr][num_cats][n_area][n_maxdet] fp64 (the
 * layout of COCOeval.eval), n_gt [num_cats][n_area] int32 (npig).  Limits: K <= 1024, G <= 512, num_cats <= 128, n_thr <= 10, n_rec
 * <= 128, n_area <= 4, n_maxdet <= 4, max_dets <= 1024, N * K < 2^31 (FD_E_UNSUPPORTED names the limit).  Deterministic.  det boxes
 * 16-byte aligned, GT boxes 8-byte; workspace (fd_eval_coco_workspace_bytes: about 56 bytes per detection row) 256-byte aligned.
 * 22 launches and 2 memsets on `stream`, no host synchronisation. */
int64_t fd_eval_coco_workspace_bytes(int32_t N, int32_t K, int32_t G, int32_t num_cats);
int32_t fd_eval_coco(const float* det_scores, const int64_t* det_labels, const float* det_boxes, const int32_t* det_counts, int32_t N,
                     int32_t K, const double* gt_boxes, const double* gt_area, const uint8_t* gt_crowd, const int64_t* gt_labels, int32_t G,
                     const int32_t* image_order, int32_t num_cats, const double* iou_thrs, int32_t n_thr, const double* rec_thrs,
                     int32_t n_rec, const double* area_rng, int32_t n_area, const int32_t* max_dets, int32_t n_maxdet, double* precision,
                     double* recall, int32_t* n_gt, void* workspace, fd_stream_t stream);

/* ------------------------------------------------------------------------------------------- */
/* LTRB IoU / GIoU regression loss (reference model/loss.py:116-177), fused masked forward + backward.
 * pred/target [B][L][4], mask [B][L] (uint8, positives).  mode 0 = 'iou', 1 = 'giou'.
 * loss_per_image [B] = sum over positives (NOT yet divided by num_pos), num_pos [B] int32.
 * backward: grad_pred [B][L][4] = d(sum_b loss_b * gscale[b]) / d pred  (gscale = upstream/num_pos). */
int32_t fd_ltrb_iou_loss_fwd(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t L,
                             int32_t mode, float* loss_per_image, int32_t* num_pos, fd_stream_t stream);
int32_t fd_ltrb_iou_loss_bwd(const float* pred, const float* target, const uint8_t* mask, const float* gscale,
                             int32_t B, int32_t L, int32_t mode, float* grad_pred, fd_stream_t stream);

/* Focal classification loss from logits (model/loss.py:6-28,180-193), alpha 0.25 / gamma 2 in the reference.
 * logits [B][L][C], labels [B][L] int64 (1..C, 0 = background).  loss_per_image [B] = sum over [L][C]
 * (not yet divided by num_pos).  backward: grad [B][L][C] = dloss_b/dlogits * gscale[b].  Only gamma == 2 is built.
 * workspace: fd_focal_workspace_bytes(B). */
int64_t fd_focal_workspace_bytes(int32_t B);
int32_t fd_focal_loss_fwd(const float* logits, const int64_t* labels, int32_t B, int32_t L, int32_t C, float alpha,
                          float gamma, float* loss_per_image, void* workspace, fd_stream_t stream);
int32_t fd_focal_loss_bwd(const float* logits, const int64_t* labels, const float* gscale, int32_t B, int32_t L, int32_t C,
                          float alpha, float gamma, float* grad_logits, fd_stream_t stream);

/* IoU-aware classification losses from logits (the project's own definitions): Quality Focal Loss (kind 0,
 * beta = 2; alpha ignored) and Varifocal Loss (kind 1, gamma = 2, alpha 0.75 as published).  With s = sigmoid(x),
 * bce(x, y) = max(x, 0) - x*y + log1p(exp(-|x|)) and the soft target y = q[b][l] where labels[b][l] == c + 1, else 0:
 *   QFL   (y - s)^2 * bce(x, y)
 *   VFL   y * bce(x, y) where y > 0, alpha * s^2 * bce(x, 0) elsewhere
 * fd_ltrb_quality: q_out [B][L] = 0 where labels <= 0, else iou of pred / target [B][L][4] (LTRB distances, 16-byte
 * aligned) exactly as the LTRB loss computes it, then (iou > 0) ? min(iou, 1) : 0 (NaN and negative values give 0).
 * q is a target: the backward has no gradient for it; a caller may pass any q [B][L] of its own instead.
 * fd_quality_loss_fwd: logits [B][L][C], labels [B][L] int64 (a label outside 1..C matches no class) ->
 * loss_per_image [B] = sum over [L][C], qsum_per_image [B] = sum over [L] of q; both summed in doubles in a fixed order
 * (no atomics: equal inputs give equal bits).  Two launches.  workspace: fd_quality_loss_workspace_bytes(B) bytes,
 * 8-byte aligned; it may hold anything.  fd_quality_loss_bwd: grad_logits [B][L][C] = dloss_b/dlogits * gscale[b], one
 * launch.  Rows are read in 16-, 8- or 4-byte pieces as C and the alignment of logits / grad_logits allow.  B <= 65535.
 * beta / gamma other than 2: FD_E_UNSUPPORTED; other bad arguments: FD_E_INVAL; nothing is enqueued on a refusal. */
int32_t fd_ltrb_quality(const float* pred, const float* target, const int64_t* labels, int32_t B, int32_t L, float* q_out,
                        fd_stream_t stream);
int64_t fd_quality_loss_workspace_bytes(int32_t B);
int32_t fd_quality_loss_fwd(const float* logits, const int64_t* labels, const float* q, int32_t B, int32_t L, int32_t C,
                            int32_t kind, float alpha, float gamma, float* loss_per_image, float* qsum_per_image,
                            void* workspace, fd_stream_t stream);
int32_t fd_quality_loss_bwd(const float* logits, const int64_t* labels, const float* q, const float* gscale, int32_t B,
                            int32_t L, int32_t C, int32_t kind, float alpha, float gamma, float* grad_logits,
                            fd_stream_t stream);

/* Centerness loss: binary_cross_entropy_with_logits(reduction='sum') over positives (model/loss.py:31-57).
 * x / target / mask [B][L]; loss_per_image [B] (sum), num_pos [B]; backward grad [B][L] = (sigmoid(x)-t)*gscale[b]. */
int32_t fd_bce_logits_loss_fwd(const float* x, const float* target, const uint8_t* mask, int32_t B, int32_t L,
                               float* loss_per_image, int32_t* num_pos, fd_stream_t stream);
int32_t fd_bce_logits_loss_bwd(const float* x, const float* target, const uint8_t* mask, const float* gscale, int32_t B,
                               int32_t L, float* grad, fd_stream_t stream);

/* FCOS target assignment (FCOSGenTargets, model/modules/head.py:211-316): gt_boxes [B][M][4] xyxy (pad -1),
 * labels [B][M] int64 (pad -1); per level: stride, (range_lo, range_hi]; centre-sampling radius = stride*radius_ratio
 * (1.5 in the reference).  Outputs per image, levels concatenated: cls_target [B][L] int64 (0 = negative),
 * cnt_target [B][L] (-1 = negative), reg_target [B][L][4] LTRB (-1 = negative).  segs->batch = B. */
int32_t fd_fcos_gen_targets(const float* gt_boxes, const int64_t* labels, int32_t M, const fd_segs* segs,
                            const int32_t* strides, const int32_t* range_lo, const int32_t* range_hi, float radius_ratio,
                            int64_t* cls_target, float* cnt_target, float* reg_target, fd_stream_t stream);

/* ATSS target assignment (Adaptive Training Sample Selection, Zhang et al., CVPR 2020) on the level table,
 * location order and outputs of fd_fcos_gen_targets.  A row is valid when label >= 0, its coordinates are finite and
 * x2 > x1, y2 > y1; M == 0 is accepted with NULL gt_boxes / labels.  Per valid row, fp32 without FMA contraction:
 *   candidates  per level the min(topk, H*W) locations with the smallest (d2, pix), d2 the squared distance of the
 *               location centre (px*s + s/2, py*s + s/2) to the box centre ((x1+x2)/2, (y1+y2)/2); equal d2: lower pix
 *   iou         fd_pairwise_iou(plus_one = 0) of the square anchor centre -/+ (anchor_scale * s) / 2 and the box
 *   thr         mean + sample standard deviation of the candidates' iou, in fp64, summed in candidate order
 *   positive    (double)iou >= thr and min(cx-x1, cy-y1, x2-cx, y2-cy) > inside_eps
 * A location positive for several rows goes to the largest iou, then to the lowest row.  gt_thr [B][M] (thr, NaN for
 * padding) and gt_npos [B][M] (positives of the row before the contest) are optional (NULL).  workspace:
 * fd_atss_workspace_bytes(B, L) bytes, 8-byte aligned; gt_boxes / reg_target 16-byte aligned.  One memset and two
 * launches, no host synchronisation.  topk > FD_ATSS_MAX_TOPK: FD_E_UNSUPPORTED; other bad arguments: FD_E_INVAL. */
#define FD_ATSS_MAX_TOPK 16
int64_t fd_atss_workspace_bytes(int32_t B, int32_t L);
int32_t fd_atss_gen_targets(const float* gt_boxes, const int64_t* labels, int32_t M, const fd_segs* segs,
                            const int32_t* strides, int32_t topk, float anchor_scale, float inside_eps,
                            int64_t* cls_target, float* cnt_target, float* reg_target, double* gt_thr, int32_t* gt_npos,
                            void* workspace, fd_stream_t stream);

/* SimOTA target assignment (Ge et al., OTA, CVPR 2021; YOLOX) on the level table, location order and outputs
 * of fd_fcos_gen_targets, ranked by the current predictions: cls_logits [B][L][C], cnt_logits [B][L], reg_pred [B][L][4]
 * (l, t, r, b) distances in pixels, all fp32.  A row is valid when 1 <= label <= C (its class is column label - 1), its
 * coordinates are finite and x2 > x1, y2 > y1; M == 0 is accepted with NULL gt_boxes / labels.  fp32 without FMA
 * contraction; c = (px*s + s/2, py*s + s/2) the centre of location p, nl(x) = -logf(x) where that is < 100, else 100:
 *   per location  q_c = sqrtf(sigmoid(cls_c) * sigmoid(cnt)); N = sum_c nl(1 - q_c), sequentially, c ascending
 *   candidate     min(cx-x1, cy-y1, x2-cx, y2-cy) > inside_eps
 *   preferred     a candidate with max(|cx-gx|, |cy-gy|) < centre_radius * (float)s, g = ((x1+x2)/2, (y1+y2)/2)
 *   iou           fd_pairwise_iou(plus_one = 0) of (cx-l, cy-t, cx+r, cy+b) and the row; !(iou > 0) -> 0, iou > 1 -> 1
 *   cost          ((N - nl(1 - q_g)) + nl(q_g)) + iou_weight * (0.0f - logf(iou + 1e-8f)), g the row's class;
 *                 !(cost < FLT_MAX) -> FLT_MAX
 *   k             n = number of candidates; sum of the min(top_q, n) largest iou, descending; k = min(max((int)sum, 1), n)
 *   positive      the k candidates with the smallest (not preferred, cost, p), p the location index in [0, L)
 * A location positive for several rows goes to the smallest (not preferred, cost, row).  cnt_target is the centre-ness
 * of fd_fcos_gen_targets (quality 0) or the winning pair's iou (quality 1).  Optional (NULL): pair_iou / pair_cost
 * [B][M][L] (0 / +inf for non-candidates and padding rows), gt_k / gt_ncand [B][M] (k and n, 0 for padding).
 * workspace: fd_simota_workspace_bytes(B, M, L) bytes, 8-byte aligned; gt_boxes / reg_pred / reg_target 16-byte
 * aligned; it may hold anything.  Three launches (M == 0: one), no memset, no host synchronisation.  top_q > FD_SIMOTA_MAX_TOPQ or
 * M > FD_SIMOTA_MAX_GT: FD_E_UNSUPPORTED; other bad arguments: FD_E_INVAL. */
#define FD_SIMOTA_MAX_TOPQ 16
#define FD_SIMOTA_MAX_GT 256
int64_t fd_simota_workspace_bytes(int32_t B, int32_t M, int32_t L);
int32_t fd_simota_gen_targets(const float* cls_logits, const float* cnt_logits, const float* reg_pred, int32_t C,
                              const float* gt_boxes, const int64_t* labels, int32_t M, const fd_segs* segs,
                              const int32_t* strides, int32_t top_q, float centre_radius, float iou_weight,
                              float inside_eps, int32_t quality, int64_t* cls_target, float* cnt_target,
                              float* reg_target, float* pair_iou, float* pair_cost, int32_t* gt_k, int32_t* gt_ncand,
                              void* workspace, fd_stream_t stream);

/* ------------------------------------------------------------------------------------------- */
/* Anchor targets and detections (DataEncoder.encode / decode, utill/utills.py:100-199).
 *
 * fd_anchor_params describes the anchor set of one input size; the HOST fills it (DataEncoder._anchor_params of the Python
 * package) and every kernel derives its anchors from the row index -- no anchor table is read from memory:
 *   fm_w / fm_h [level]    feature-map size ceil(input / 2^(level+3)), >= 1
 *   grid_w / grid_h        fp32 input / fm (NOT the stride: 100 / 13 = 7.69... at level 0)
 *   wh [level][k][2]       the 9 (w, h) pairs of the level, computed in doubles and rounded once to fp32
 *   num_anchors            A = 9 * sum fm_w * fm_h, checked against the `A` argument of every call
 * Row order: level, y, x, k.  Anchor row = (cx, cy, w, h) with cx = ((float)x + 0.5f) * grid_w, cy alike. */
#define FD_ANCHOR_LEVELS 5
#define FD_ANCHOR_PER_CELL 9
#define FD_ANCHOR_MAX_GT 256      /* fd_anchor_encode: ground-truth rows per image, padding included */
#define FD_ANCHOR_MAX_CLASSES 128 /* fd_anchor_decode */
#define FD_ANCHOR_MAX_CAND 1024   /* fd_anchor_decode: max_candidates (the limit of fd_box_nms_plus1) */
typedef struct fd_anchor_params {
    int32_t fm_w[FD_ANCHOR_LEVELS];
    int32_t fm_h[FD_ANCHOR_LEVELS];
    float grid_w[FD_ANCHOR_LEVELS];
    float grid_h[FD_ANCHOR_LEVELS];
    float wh[FD_ANCHOR_LEVELS][FD_ANCHOR_PER_CELL][2];
    int32_t num_anchors;
} fd_anchor_params;

/* anchors [A][4] = (cx, cy, w, h), 16-byte aligned (DataEncoder._get_anchor_boxes, bit for bit). */
int32_t fd_anchor_boxes(const fd_anchor_params* p, float* anchors, int32_t A, fd_stream_t stream);

/* DataEncoder.encode for B images in one launch.  gt [B][M][4] xyxy fp32 (16-byte aligned), labels [B][M] int64; a row
 * with label < 0 is padding (the convention of fd_fcos_gen_targets); 0 <= M <= FD_ANCHOR_MAX_GT (FD_E_UNSUPPORTED above;
 * gt / labels may be NULL when M == 0).  Outputs loc [B][A][4] fp32 (16-byte aligned), cls [B][A] int64.  Per anchor, fp32
 * without FMA contraction: each box becomes (centre, b - a + 1), both sides go back to corners as c -/+ wh/2, IoU with the
 * "+1" convention exactly as fd_pairwise_iou(plus_one = 1), first maximum over the image's boxes in row order;
 * loc = ((gt_xy - a_xy) / a_wh, log(gt_wh / a_wh)); cls = 1 + label, 0 where max_iou < 0.5, then -1 where
 * 0.4f < max_iou < 0.5.  An image without a valid box gets cls = 0, loc = 0 (the reference raises). */
int32_t fd_anchor_encode(const fd_anchor_params* p, const float* gt, const int64_t* labels, int32_t B, int32_t M, int32_t A,
                         float* loc, int64_t* cls, fd_stream_t stream);

/* DataEncoder.decode for B images.  loc [B][A][4] fp32 (16-byte aligned), cls [B][A][C] fp32 logits, 1 <= C <=
 * FD_ANCHOR_MAX_CLASSES (float4 loads when C % 4 == 0 and cls is 16-byte aligned, scalar loads otherwise).  Per anchor:
 * xy = loc_xy * a_wh + a_xy, wh = exp(loc_wh) * a_wh, box = xy -/+ wh / 2; score, label = first maximum over the fp32
 * SIGMOID values (not over the logits: saturated logits tie at 1.0f and the lowest class wins); candidate when
 * score > cls_thresh.  The top K = min(max_candidates, A) candidates by score (ties: lower anchor row first;
 * 1 <= max_candidates <= FD_ANCHOR_MAX_CAND) go through fd_box_nms_plus1(nms_thresh, 'union').  Outputs, all [B][K] and
 * score-descending: boxes [B][K][4] xyxy (16-byte aligned), labels int64 (0-based; -1 in the padding), scores; counts [B]
 * int32 = rows kept; n_candidates [B] int32 = anchors that passed cls_thresh (> K: the image was truncated to the K best).
 * workspace: fd_anchor_decode_workspace_bytes(B, A, max_candidates) bytes (-1: bad arguments), 256-byte aligned.
 * Five launches and one memset on `stream`, no host synchronisation. */
int64_t fd_anchor_decode_workspace_bytes(int32_t B, int32_t A, int32_t max_candidates);
int32_t fd_anchor_decode(const fd_anchor_params* p, const float* loc, const float* cls, int32_t B, int32_t A, int32_t C,
                         float cls_thresh, float nms_thresh, int32_t max_candidates, float* boxes, int64_t* labels,
                         float* scores, int32_t* counts, int32_t* n_candidates, void* workspace, fd_stream_t stream);

/* ------------------------------------------------------------------------------------------- */
/* Optimizer step (train.py:160-182: the learning-rate lines, scaler.step(optimizer)).
 *
 * One step is ONE begin launch followed by one update launch per chunk of tensors.  A chunk is a list of up to
 * FD_OPTIM_MAX_TENSORS tensors whose pointers travel BY VALUE in the kernel arguments: nothing on the device outlives the
 * launch, so gradients may move between steps (zero_grad(set_to_none=True), a graph's private pool) and a capture records
 * the arguments as they are.  The host fills every chunk from the live tensors of the step it launches.
 *
 * fd_optim_state is the optimizer's own block of device memory (allocated once, zero-filled: its address must not move
 * between a capture and its replays).  Only the begin launch writes it; the update launches only read it.
 *   global_step   pre-incremented by every begin (the reference's GLOBAL_STEPS)
 *   skip          1 when *found_inf != 0 at begin: the update launches of the step then write nothing
 *   lr[group]     fp64 rate of the step, written by every begin from the rule, a device scalar or a value
 *   applied[group]  steps actually applied (not skipped); Adam's t
 *   bc1 / bc2     1 - beta1^t, 1 - beta2^t in fp64 (Adam) */
#define FD_OPTIM_MAX_TENSORS 64 /* chunk capacity: 64 * 40 B + 8 B = 2568 B of the 4 KB kernel-argument segment */
#define FD_OPTIM_MAX_GROUPS 8
#define FD_OPTIM_MAX_DROPS 4
#define FD_OPTIM_LR_NONE 0     /* lr[group] = *lr_ptr[group] if given, else lr_value[group] */
#define FD_OPTIM_LR_TRAIN_PY 1 /* train.py:160-173 */
#define FD_OPTIM_LR_TRAIN_NEW 2 /* train_new.py:79-90 */

typedef struct fd_optim_state {
    int64_t global_step;
    int64_t skip;
    double lr[FD_OPTIM_MAX_GROUPS];
    int64_t applied[FD_OPTIM_MAX_GROUPS];
    double bc1[FD_OPTIM_MAX_GROUPS];
    double bc2[FD_OPTIM_MAX_GROUPS];
} fd_optim_state;

typedef struct fd_optim_chunk {
    int32_t n; /* tensors in use, 1 .. FD_OPTIM_MAX_TENSORS */
    int32_t reserved0;
    float* p[FD_OPTIM_MAX_TENSORS];       /* parameter */
    const float* g[FD_OPTIM_MAX_TENSORS]; /* gradient (still multiplied by *grad_scale) */
    float* s0[FD_OPTIM_MAX_TENSORS];      /* SGD momentum buffer (NULL when momentum == 0) / Adam exp_avg */
    float* s1[FD_OPTIM_MAX_TENSORS];      /* Adam exp_avg_sq (NULL for SGD) */
    int64_t numel[FD_OPTIM_MAX_TENSORS];  /* 0 is legal: the tensor is skipped and its pointers are not looked at */
} fd_optim_chunk;

/* Hyper-parameters of one param group; the rate is NOT here, every update reads state->lr[group]. */
typedef struct fd_optim_hyper {
    int32_t group;        /* 0 .. FD_OPTIM_MAX_GROUPS - 1 */
    int32_t nesterov;     /* SGD */
    int32_t decoupled_wd; /* Adam: 1 = AdamW */
    int32_t reserved0;
    double momentum;      /* SGD */
    double weight_decay;
    double beta1, beta2, eps; /* Adam */
} fd_optim_hyper;

/* What the begin launch evaluates.  The rule works in fp64 in the reference's operation order:
 *   TRAIN_PY:  G < warmup_steps: lr = G / warmup_steps * lr_init; then, for each drop in order, G == drop_step[i]:
 *              lr = lr_init * drop_factor[i]; a step that meets neither keeps the rate of the step before.
 *   TRAIN_NEW: lr = lr_init; G < warmup_steps: a = G / warmup_steps, lr = lr * (warmup_factor * (1 - a) + a);
 *              else for each milestone drop_step[i] in order: stop at the first G < drop_step[i], else lr = lr * gamma.
 * Every group gets the rule's rate.  active[group] = 0: the group has no tensor this step, its applied count stays. */
typedef struct fd_optim_begin_params {
    int32_t n_groups; /* 1 .. FD_OPTIM_MAX_GROUPS */
    int32_t adam;     /* 1: write bc1 / bc2 */
    int32_t rule;     /* FD_OPTIM_LR_* */
    int32_t n_drops;  /* 0 .. FD_OPTIM_MAX_DROPS */
    double lr_init, warmup_factor, gamma;
    int64_t warmup_steps;
    int64_t drop_step[FD_OPTIM_MAX_DROPS];
    double drop_factor[FD_OPTIM_MAX_DROPS];
    double lr_value[FD_OPTIM_MAX_GROUPS];
    const void* lr_ptr[FD_OPTIM_MAX_GROUPS]; /* device scalar, fp64 when lr_ptr_f64[group] else fp32; NULL: lr_value */
    int32_t lr_ptr_f64[FD_OPTIM_MAX_GROUPS];
    int32_t active[FD_OPTIM_MAX_GROUPS];
    double beta1[FD_OPTIM_MAX_GROUPS], beta2[FD_OPTIM_MAX_GROUPS];
} fd_optim_begin_params;

/* One launch, one lane: global_step += 1; skip = found_inf && *found_inf != 0 (found_inf: device fp32 scalar or NULL);
 * lr[group]; unless skipped applied[group] += 1 for the active groups; bc1 / bc2 from applied (Adam). */
int32_t fd_optim_begin(fd_optim_state* state, const float* found_inf, const fd_optim_begin_params* params, fd_stream_t stream);

/* One chunk of fp32 tensors, blockIdx.y = tensor, blockIdx.x grid-strides over its elements.  g is multiplied by
 * 1 / *grad_scale on load (grad_scale: device fp32 scalar or NULL); nothing is written when state->skip is set.
 * 16-byte accesses where the tensor's pointers share one alignment (scalar head up to the boundary, scalar tail), scalar
 * accesses where they do not.  Arithmetic is fp32 without FMA contraction, in the order written here.
 *   SGD  (torch.optim.SGD, dampening 0):  d = g + wd * p;  momentum != 0: buf = momentum * buf + d,
 *        d = nesterov ? d + momentum * buf : buf;  p -= lr * d.   Buffers start as zeros.
 *   Adam (torch.optim.Adam / AdamW, no AMSGrad):  decoupled_wd ? p *= 1 - lr * wd : g += wd * p;
 *        m += (g - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g * g;
 *        p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).
 * FD_E_INVAL: n outside [1, FD_OPTIM_MAX_TENSORS], a negative numel, a null p / g / needed state pointer of a tensor
 * with numel > 0, a null state block, a group outside the table. */
int32_t fd_optim_sgd_f32(const fd_optim_chunk* chunk, const fd_optim_hyper* hyper, const fd_optim_state* state,
                         const float* grad_scale, fd_stream_t stream);
int32_t fd_optim_adam_f32(const fd_optim_chunk* chunk, const fd_optim_hyper* hyper, const fd_optim_state* state,
                          const float* grad_scale, fd_stream_t stream);

/* Clipping the global gradient norm inside the step.  The gradients are read once more and never written:
 * the clip coefficient becomes one more factor of the scalar the update launches already divide every gradient by.
 *   1. fd_grad_sumsq_f32 per chunk of gradients: every block stores ONE fp64 partial into a slot of its own;
 *   2. fd_grad_clip_finish: one workgroup adds the slots in index order and writes fd_grad_clip;
 *   3. fd_optim_begin with found_inf = &clip->found;  4. the update launches with grad_scale = &clip->eff_scale.
 * No floating-point atomics and no block counter: the result does not depend on the order in which blocks run. */
typedef struct fd_grad_chunk {
    int32_t n; /* tensors in use, 1 .. FD_OPTIM_MAX_TENSORS */
    int32_t reserved0;
    const float* g[FD_OPTIM_MAX_TENSORS]; /* gradient, 4-byte aligned (still multiplied by *grad_scale) */
    int64_t numel[FD_OPTIM_MAX_TENSORS];  /* 0 is legal: the tensor adds 0.0 and its pointer is not looked at */
} fd_grad_chunk;

/* The clip block: device memory allocated once (its address must not move between a capture and its replays), written
 * by fd_grad_clip_finish alone.  fp64 throughout; the three floats are what other launches and the host's logging read. */
typedef struct fd_grad_clip {
    double sumsq;         /* sum of g * g over every slot (of the gradients as they are: still scaled) */
    double total_norm;    /* sqrt(sumsq) / scale, scale = *grad_scale or 1 */
    double clip_coef;     /* min(1, max_norm / (total_norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s; 1 when found */
    float eff_scale;      /* (float)(scale / clip_coef): the update launches' grad_scale; the scale itself, bit for bit,
                             when clip_coef == 1 */
    float found;          /* 1 when sumsq is not finite or *found_inf != 0, else 0: fd_optim_begin's found_inf */
    float total_norm_f32; /* (float)total_norm */
    float reserved0;
} fd_grad_clip;

/* Slots a chunk's launch writes: n * (blocks per tensor; follows the chunk's largest tensor).  -1: a chunk that
 * fd_grad_sumsq_f32 refuses.  Host only. */
int32_t fd_grad_sumsq_slots(const fd_grad_chunk* chunk);

/* Bytes of partials that n_chunks launches can need at most (-1: n_chunks < 0); 8-byte aligned, never cleared. */
int64_t fd_grad_norm_workspace_bytes(int32_t n_chunks);

/* One chunk: blockIdx.y = tensor, blockIdx.x grid-strides over it with 16-byte loads after a scalar head up to the
 * boundary, scalar tail; each lane accumulates (double)g * g in fp64; fixed reduction across the wave, then across the
 * four waves through LDS; block (x, tensor) stores partials[first_slot + tensor * blocks_x + x], 0.0 when it met no
 * element (blocks_x follows the chunk's largest tensor, one block per 4096 elements up to 128; a shorter tensor is
 * shared among its first ceil(numel / 4096) blocks).  Writes fd_grad_sumsq_slots(chunk) slots from first_slot on.
 * FD_E_INVAL: a null chunk / partials, n outside [1, FD_OPTIM_MAX_TENSORS], a negative numel, a null or not 4-byte
 * aligned g of a tensor with numel > 0, a negative first_slot. */
int32_t fd_grad_sumsq_f32(const fd_grad_chunk* chunk, double* partials, int32_t first_slot, fd_stream_t stream);

/* One workgroup over partials[0 .. n_slots) (n_slots == 0: no gradient, a norm of 0).  grad_scale / found_inf: device
 * fp32 scalars or NULL.  FD_E_INVAL: null partials / out, n_slots < 0, max_norm not positive or not finite. */
int32_t fd_grad_clip_finish(const double* partials, int32_t n_slots, const float* grad_scale, const float* found_inf,
                            double max_norm, fd_grad_clip* out, fd_stream_t stream);

/* Averaging the model's weights (torch.optim.swa_utils.AveragedModel: SWA, the equal average, and EMA).
 *
 * One update is ONE begin launch, one fd_avg_update_f32 launch per chunk of averaged fp32 tensors and one
 * fd_avg_copy_bytes launch per chunk of buffers that are copied instead.  As in the optimizer step the tensor lists
 * travel BY VALUE in the kernel arguments: nothing on the device outlives the launch, a capture records the arguments as
 * they are, and no launch makes the host read the device.
 *
 * fd_avg_state is the averager's own block of device memory (allocated once: its address must not move between a capture
 * and its replays).  Only the begin launch writes it; the update and copy launches only read it. */
#define FD_AVG_SWA 0 /* equal average: weight = 1 / (n_averaged + 1) */
#define FD_AVG_EMA 1 /* exponential moving average: weight = 1 - decay */

typedef struct fd_avg_state {
    int64_t apply;    /* 1: this call averages; 0: its update / copy launches write nothing */
    double weight;    /* blend factor of this call (0 when apply == 0) */
    float weight_f32; /* (float)weight: what the update launches multiply by */
    float reserved0;
    int64_t reserved1; /* up to a multiple of 16 bytes */
} fd_avg_state;

typedef struct fd_avg_begin_params {
    int32_t mode; /* FD_AVG_SWA / FD_AVG_EMA */
    int32_t reserved0;
    double decay;       /* EMA, in [0, 1] */
    int64_t start_step; /* the gate on *global_step: averages when *global_step >= start_step ... */
    int64_t every;      /* ... and (*global_step - start_step) % every == 0; >= 1 */
} fd_avg_begin_params;

/* One launch, one lane.  n_averaged: the module's int64 device scalar.  skip / global_step: device pointers into an
 * optimizer's fd_optim_state, &state->skip and &state->global_step (the step the optimizer evaluated LAST, so the update
 * follows the optimizer's step), or NULL.
 *   apply = !(skip && *skip) && (global_step == NULL || (*global_step >= start_step && (*global_step - start_step) % every == 0))
 *   apply:  weight = *n_averaged == 0 ? 1.0 : (mode == FD_AVG_SWA ? 1.0 / (double)(*n_averaged + 1) : 1.0 - decay);
 *           weight_f32 = (float)weight;  *n_averaged += 1.
 *   else:   weight = 0, *n_averaged untouched.
 * FD_E_INVAL: a null state / n_averaged / params, a mode outside the two, decay outside [0, 1] or not finite,
 * every < 1, global_step == NULL with start_step != 0 or every != 1. */
int32_t fd_avg_begin(fd_avg_state* state, int64_t* n_averaged, const int64_t* skip, const int64_t* global_step,
                     const fd_avg_begin_params* params, fd_stream_t stream);

typedef struct fd_avg_chunk {
    int32_t n; /* tensors in use, 1 .. FD_OPTIM_MAX_TENSORS */
    int32_t reserved0;
    float* avg[FD_OPTIM_MAX_TENSORS];     /* the averaged copy */
    const float* p[FD_OPTIM_MAX_TENSORS]; /* the model's tensor */
    int64_t numel[FD_OPTIM_MAX_TENSORS];  /* 0 is legal: the tensor is skipped and its pointers are not looked at */
} fd_avg_chunk;                           /* 64 * 24 B + 8 B = 1544 B of the 4 KB kernel-argument segment */

/* One chunk of fp32 tensors, blockIdx.y = tensor, blockIdx.x grid-strides over its elements, 256 lanes; the grid's x extent
 * follows the chunk's largest tensor (capped as in the optimizer kernels), a block past a shorter tensor's end exits.
 * 16-byte accesses where avg and p share one alignment (scalar head up to the boundary, scalar tail), scalar accesses where
 * they do not.  12 B per element, no LDS, no atomics.
 *   state->apply == 0:          nothing is written.
 *   state->weight_f32 == 1.0f:  avg = p bit for bit, NaN payloads included (the first update; decay == 0).
 *   otherwise:                  avg = avg + (p - avg) * weight_f32 in fp32, in that order, without FMA contraction.
 * So an element with p == avg comes back unchanged ((p - avg) is 0): tensors that never train stay identical to the
 * model's (a -0.0 comes back as +0.0, the sum of two zeros of opposite sign).
 * FD_E_INVAL: a null chunk / state, n outside [1, FD_OPTIM_MAX_TENSORS], a negative numel, a null or not 4-byte aligned
 * avg / p of a tensor with numel > 0. */
int32_t fd_avg_update_f32(const fd_avg_chunk* chunk, const fd_avg_state* state, fd_stream_t stream);

typedef struct fd_avg_copy_chunk {
    int32_t n; /* buffers in use, 1 .. FD_OPTIM_MAX_TENSORS */
    int32_t reserved0;
    void* dst[FD_OPTIM_MAX_TENSORS];
    const void* src[FD_OPTIM_MAX_TENSORS];
    int64_t nbytes[FD_OPTIM_MAX_TENSORS]; /* 0 is legal */
} fd_avg_copy_chunk;

/* Buffers that are copied, not averaged (integer buffers such as BatchNorm's 0-dim int64 num_batches_tracked; every buffer
 * without use_buffers): dst = src exactly, at any alignment, gated by the same state->apply.  The launch shape is
 * fd_avg_update_f32's: 16-byte accesses where dst and src share one alignment (byte head and tail), bytes where not.
 * FD_E_INVAL: a null chunk / state, n outside [1, FD_OPTIM_MAX_TENSORS], a negative nbytes, a null dst / src of a buffer
 * with nbytes > 0. */
int32_t fd_avg_copy_bytes(const fd_avg_copy_chunk* chunk, const fd_avg_state* state, fd_stream_t stream);

/* Baseline JPEG decoding (the reference's Image.open(path).convert('RGB'), dataset/voc.py:69, dataset/pascalvoc.py:28,
 * data/dataload.py:35).  The serial half stays on the host: fd_jpeg_parse reads the markers up to SOS,
 * fd_jpeg_entropy_decode undoes the Huffman coding into dense quantised coefficients.  The data-parallel half is two launches
 * per batch: fd_jpeg_idct_u8 (dequantise + libjpeg's jpeg_idct_islow, one job per image component) and fd_jpeg_color_u8
 * (libjpeg-turbo's fancy chroma upsampling + YCbCr -> RGB, one job per image).  Integer arithmetic throughout; the result is
 * bit for bit what Pillow returns.
 *
 * The two host functions touch no GPU, keep no state between calls, never set the fd_last_error text and may run on any number
 * of threads at once: what went wrong is their return value (FD_JPEG_E_*), what is merely not handled is info->reason. */
#define FD_JPEG_MAX_COMP 3

/* info->reason when info->supported == 0: a well-formed stream this decoder does not take */
#define FD_JPEG_R_NONE 0
#define FD_JPEG_R_PROGRESSIVE 1 /* SOF2 (and every other frame type but SOF0 / SOF1 / the arithmetic ones) */
#define FD_JPEG_R_ARITHMETIC 2  /* SOF9 .. SOF15 */
#define FD_JPEG_R_PRECISION 3   /* 12-bit samples, or 16-bit quantisation tables */
#define FD_JPEG_R_COMPONENTS 4  /* a component count other than 1 or 3 (CMYK / YCCK) */
#define FD_JPEG_R_RGB 5         /* Adobe transform 0, or component ids 'R','G','B': no YCbCr -> RGB step applies */
#define FD_JPEG_R_SAMPLING 6    /* luma not 1x1 / 2x1 / 2x2, or chroma not 1x1 */
#define FD_JPEG_R_MULTISCAN 7   /* the first scan does not hold every component of the frame */
#define FD_JPEG_R_DNL 8         /* height 0 in the frame header: the height follows in a DNL segment */

/* return codes of the two host functions: FD_OK, or what is wrong with the stream / the call */
#define FD_JPEG_E_TRUNCATED (-16)  /* the stream ends (or a marker interrupts the scan) before the data does */
#define FD_JPEG_E_MARKER (-17)     /* no SOI, a malformed segment, SOS before SOF, a missing or wrong RSTn */
#define FD_JPEG_E_HUFFMAN (-18)    /* bits that match no code of the table, or an impossible table */
#define FD_JPEG_E_COEF_INDEX (-19) /* a run that carries the coefficient index past 63 */
#define FD_JPEG_E_TABLE (-20)      /* the scan names a Huffman or quantisation table nothing defines */
#define FD_JPEG_E_BUFFER (-21)     /* coef_bytes below info->coef_bytes, or a null argument */
#define FD_JPEG_E_UNSUPPORTED (-22) /* fd_jpeg_entropy_decode on an info with supported == 0 */

typedef struct fd_jpeg_info {
    int32_t width, height;
    int32_t ncomp;            /* 1 or 3 when supported */
    int32_t supported;        /* 1: fd_jpeg_entropy_decode and the two launches take this stream */
    int32_t reason;           /* FD_JPEG_R_* */
    int32_t restart_interval; /* MCUs between RSTn markers, 0: none */
    int32_t h_samp[FD_JPEG_MAX_COMP], v_samp[FD_JPEG_MAX_COMP]; /* a single component counts as 1 x 1, as its scan does */
    int32_t h_max, v_max;
    int32_t mcus_x, mcus_y;
    int32_t bw[FD_JPEG_MAX_COMP], bh[FD_JPEG_MAX_COMP]; /* 8 x 8 blocks per row / column, padded to whole MCUs */
    int32_t dc_tab[FD_JPEG_MAX_COMP], ac_tab[FD_JPEG_MAX_COMP]; /* Huffman table selectors of the scan */
    int32_t reserved0[2]; /* up to a multiple of 8 bytes */
    int64_t scan_offset;  /* first entropy-coded byte */
    int64_t coef_bytes;  /* sum over components of bh * bw * 64 * sizeof(int16_t) */
    uint16_t qt[FD_JPEG_MAX_COMP][64]; /* the quantisation table OF EACH COMPONENT, natural (row-major) order */
    uint8_t huff_defined[2][4];        /* [0]: DC, [1]: AC */
    uint8_t huff_bits[2][4][16];       /* codes of length 1 .. 16 */
    uint8_t huff_vals[2][4][256];
} fd_jpeg_info;

/* Reads data[0 .. n) up to and including the SOS header.  FD_OK with info->supported == 0 and a reason for a well-formed
 * stream of another kind; FD_JPEG_E_* for a stream that is not well formed that far.  Never reads outside data[0 .. n). */
int32_t fd_jpeg_parse(const uint8_t* data, int64_t n, fd_jpeg_info* info);

/* Huffman-decodes the scan of a parsed, supported stream into coefs: component c at element offset
 * sum over c' < c of bh[c'] * bw[c'] * 64, as [bh][bw][64] int16 in natural order, zero where the stream codes nothing.
 * Byte stuffing and RSTn (byte alignment, DC predictors back to 0) are undone; the DC predictor is 32 bits wide and the stored
 * value its low 16 bits, libjpeg's JCOEF.  Writes coefs[0 .. info->coef_bytes / 2) and nothing else; on an error the contents
 * are unspecified.  Never reads outside data[0 .. n). */
int32_t fd_jpeg_entropy_decode(const uint8_t* data, int64_t n, const fd_jpeg_info* info, int16_t* coefs, int64_t coef_bytes);

typedef struct fd_jpeg_idct_job {
    int64_t coef_off;  /* int16 elements into coefs: the component's [bh][bw][64] */
    int64_t plane_off; /* bytes into planes, a multiple of 8: the component's uint8 [8 * bh][8 * bw] */
    int32_t bw, bh;
    int32_t qt;        /* which 64-entry table of qtabs */
    int32_t reserved0;
} fd_jpeg_idct_job;

/* ONE launch for every component of every image of a batch.  The job table exists twice with the same contents: jobs_host
 * is validated here before anything is enqueued, jobs_dev (device memory) is what the kernel reads.  coefs: device int16
 * [coef_elems]; qtabs: device uint16 [n_qtabs][64]; planes: device uint8 [planes_bytes].
 * blockIdx.y = job; eight lanes per 8 x 8 block (one column, then one row each, transposed through LDS), 32 blocks per
 * workgroup.  out = range_limit(DESCALE(row pass(DESCALE(column pass(coef * q), 11)), 18)), 64-bit intermediates.
 * FD_E_INVAL: a null pointer, n_jobs outside [1, 65535], a job whose grid is empty or above 8192 blocks a side, whose
 * coefficients, table or plane lie outside the three buffers, or whose plane_off is not a multiple of 8. */
int32_t fd_jpeg_idct_u8(const fd_jpeg_idct_job* jobs_host, const fd_jpeg_idct_job* jobs_dev, int32_t n_jobs, const int16_t* coefs,
                        int64_t coef_elems, const uint16_t* qtabs, int32_t n_qtabs, uint8_t* planes, int64_t planes_bytes,
                        fd_stream_t stream);

typedef struct fd_jpeg_color_job {
    uint8_t* out;                        /* device uint8 [height][width][3], 4-byte aligned */
    int64_t plane_off[FD_JPEG_MAX_COMP]; /* bytes into planes */
    int32_t stride[FD_JPEG_MAX_COMP];    /* bytes per plane row (8 * bw) */
    int32_t rows[FD_JPEG_MAX_COMP];      /* plane rows (8 * bh) */
    int32_t width, height;
    int32_t ncomp;          /* 1: the plane three times; 3: Y, Cb, Cr */
    int32_t h_samp, v_samp; /* of the luma: 1 x 1, 2 x 1 or 2 x 2; the chroma is 1 x 1 */
    int32_t reserved0;
} fd_jpeg_color_job;

/* ONE launch for every image of a batch, blockIdx.z = job; a lane produces four consecutive pixels of the [h * w] pixel
 * sequence, 12 contiguous bytes.  Chroma of true size dw x dh = ceil(w / h_samp) x ceil(h / v_samp): libjpeg-turbo's fancy
 * (triangle) upsampling for dw > 2, plain replication for dw <= 2; then libjpeg's 16.16 YCbCr -> RGB and a clamp to
 * [0, 255].  Only bytes of [h][w][3] are written; a plane sample is read only after its row and column passed
 * (unsigned) < dh / dw.  jobs_host / jobs_dev as above.
 * FD_E_INVAL: a null pointer, n_jobs outside [1, 65535], a job with a null or unaligned out, sides outside [1, 65535],
 * ncomp not 1 or 3, sampling outside the three, a plane smaller than dw x dh or outside planes[0 .. planes_bytes). */
int32_t fd_jpeg_color_u8(const fd_jpeg_color_job* jobs_host, const fd_jpeg_color_job* jobs_dev, int32_t n_jobs, const uint8_t* planes,
                         int64_t planes_bytes, fd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FCOSDET_H_ */
