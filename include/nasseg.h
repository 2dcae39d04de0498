/* nasseg.h - C ABI of libnasseg_hip.so: the MI355X (gfx950) kernels behind the
 * NAS inner loop of DrSleep/nas-segm-pytorch.
 *
 * The reference has no FFI for this path: its boundary is the Python op
 * registry OPS / AGG_OPS (src/nn/layer_factory.py:27-91), the decoder classes
 * (src/nn/micro_decoders.py:142,257) and one Cython module
 * (src/helpers/miou_utils.pyx).  Underneath, every op is an ATen call; the
 * entry points below are the from-scratch gfx950 replacements of exactly those
 * ATen calls, one group per reference call site.  The host side
 * (nas-segm-pytorch_amd/) binds them with ctypes and re-creates the reference's
 * registry / decoder / engine API on top.
 *
 * Conventions
 *  - plain C types only; every pointer except `const int64_t* cm` in
 *    nasseg_compute_ius_accs is a DEVICE pointer owned by the caller (PyTorch's
 *    caching allocator); the library allocates nothing and keeps no state apart
 *    from a per-thread error string;
 *  - activations are fp32 NHWC ("channels_last"): element (b,y,x,c) of a tensor
 *    with pixel stride ld is at ((b*H + y)*W + x)*ld + c; weights arrive in the
 *    PyTorch layouts ((C,1,k,k) depthwise, (N,K,kh,kw) dense) and are re-packed
 *    by the pack entry points;
 *  - `stream` is a hipStream_t passed as void* (0 = default stream); calls are
 *    asynchronous on that stream, re-entrant and thread-safe;
 *  - return value 0 = ok, negative = error; nasseg_last_error() then returns a
 *    message valid until the same thread's next failing call.  The Python
 *    binding raises RuntimeError, which the reference's try_except decorator
 *    (src/helpers/utils.py:172-187) turns into reward 0 for that candidate;
 *  - act codes: 0 none, 1 ReLU, 2 ReLU6.
 */
#ifndef NASSEG_H
#define NASSEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* nasseg_last_error(void);
int nasseg_abi_version(void);
int nasseg_device_count(void);

/* ---- depthwise convolution ------------------------------------------------
 * replaces nn.Conv2d(C, C, k, stride, padding, dilation, groups=C, bias=False)
 * in SepConv / DilConv (layer_factory.py:198-265) and InvertedResidual
 * (layer_factory.py:125-158). */
int nasseg_dw_pack_weight(const float* w, float* wt, int C, int K, int flip, void* stream);
int nasseg_dwconv(const float* x, const float* wt, float* y, const float* in_scale,
                  const float* in_shift, int in_act, const float* scale, const float* shift, int act,
                  int B, int H, int W, int C, int Ho, int Wo, int K, int stride, int pad, int dil,
                  int transposed, float* stats, void* stream);
int nasseg_dwconv_strip_ok(int K, int stride, int dil);
int64_t nasseg_dwconv_stats_blocks(int B, int C, int Ho, int Wo, int K, int stride, int dil);
/* backward-data fused with the first half of the backward of the BatchNorm whose
 * normalised output act(scale*z+shift) the conv read (normalise-on-read chains): writes
 * g = act'(..) * dwconv_backward_data(dy) and per-workgroup rows of {sum g, sum g*xhat} */
int nasseg_dwconv_bwd_data_bn(const float* dy, const float* wt, float* g, const float* z,
                              const float* scale, const float* shift, const float* mean,
                              const float* invstd, int act, int B, int H, int W, int C, int Ho,
                              int Wo, int K, int stride, int pad, int dil, int transposed,
                              float* stats, void* stream);
int64_t nasseg_dwconv_bwd_data_bn_blocks(int B, int C, int Ho, int Wo, int K, int stride, int pad,
                                         int dil, int transposed);
/* the whole backward of a 3x3 depthwise conv between two BatchNorms of a chain (InvertedResidual, layer_factory.py:
 * 139-152) in one kernel: BatchNorm backward behind the conv on load, weight gradient, input gradient masked with
 * the activation of the BatchNorm in front (in_*) and that BatchNorm's backward partial sums; xz, g, z read once,
 * ge written once.  rows = workgroups = partial rows of ws [rows][9][C] and stats [rows][2][C]; 0 = not served */
int64_t nasseg_dwconv_bwd_bn_rows(int B, int C, int H, int W, int K, int stride, int pad, int dil);
int nasseg_dwconv_bwd_bn(const float* xz, const float* g, const float* z, const float* wt, int wt_flipped, float* ge,
                         float* dw, float* ws, const float* in_scale, const float* in_shift, const float* in_mean,
                         const float* in_invstd, int in_act, const float* bn_scale, const float* bn_shift,
                         const float* bn_mean, const float* bn_invstd, const float* bn_sums, int bn_train, int bn_act,
                         int B, int H, int W, int C, int Ho, int Wo, int K, int stride, int pad, int dil, float* stats,
                         void* stream);
int64_t nasseg_dwconv_wgrad_workspace(int B, int C, int Ho, int Wo, int K);
int nasseg_dwconv_wgrad(const float* x, const float* dy, float* dw, float* ws,
                        const float* in_scale, const float* in_shift, int in_act, int B, int H, int W,
                        int C, int Ho, int Wo, int K, int stride, int pad, int dil, void* stream);

/* backward-weight of stride-1 5x5 depthwise layers (any dilation that divides the padding): 1 (initial) a kernel that
 * stages its tiles in LDS - the prologue applied once per element, the 5x8 window of a thread read from LDS, a dilated
 * conv cut into its dil^2 pixel classes; 0: the strip kernel of the other geometries.  v < 0 only queries.  Returns
 * the previous setting.  Partial rows (nasseg_dwconv_wgrad_workspace) have the same count and layout either way. */
int nasseg_dw_wgrad_lds(int v);

/* ---- one SepConv stage in one kernel: depthwise k x k -> pointwise 1x1 (+ BN statistics) -----
 * replaces the Conv2d(C, C, k, groups=C) -> Conv2d(C, N, 1) pair of SepConv / DilConv
 * (layer_factory.py:207-218,241-262): the depthwise output tile stays in LDS and feeds the
 * matrix cores directly; zdw (optional) receives the depthwise output for the backward pass. */
int64_t nasseg_sepconv_blocks(int B, int C, int Ho, int Wo, int N, int K, int stride, int dil);
int nasseg_sepconv_fwd(const float* x, const float* wdw, const float* wpw, float* zdw, float* y,
                       const float* in_scale, const float* in_shift, int in_act,
                       const float* out_scale, const float* out_shift, int out_act, int B, int H,
                       int W, int C, int Ho, int Wo, int N, int K, int stride, int pad, int dil,
                       float* stats, void* stream);

/* ---- InvertedResidual with its expansion never stored (layer_factory.py:125-158) ---------------------------
 * The 1x1 expansion K -> C = 6 K + BatchNorm + ReLU6 in front of the 3x3 depthwise conv is six times wider than the
 * block's input; its raw output z1 = W1 x is K / 4 MFMA steps per 16 x 16 tile.  Statistics of z1: a nasseg_conv_fwd
 * call with y == NULL (nothing stored).  nasseg_irdw_fwd: z2 = dwconv3x3(act1(bn1_scale * (W1 pro(x)) + bn1_shift)),
 * pad 1, stride 1 | 2, with statistics rows of z2; nasseg_irdw_bwd: nasseg_dwconv_bwd_bn with z1 rebuilt from x.
 * w1: (C, K, 1, 1) as PyTorch stores it; wdw: packed [9][C] (nasseg_dw_pack_weight; wdw_flipped != 0: its rotated
 * packing); pro(x) = in_act(in_scale * x + in_shift) (null: none).  Rows (workgroups) of statistics [r][2][C] and of
 * weight-gradient partials [r][9][C]: nasseg_irdw_rows(.., backward); 0 = geometry not served.  These two kernels serve
 * K % 4 == 0, 4 <= K <= 32, C % 16 == 0, 16 <= C <= 192, stride 1 | 2 (MobileNetV2's 16 -> 96, 24 -> 144, 32 -> 192
 * among them).  That is NOT the envelope of the whole form: the expansion's own backward must rebuild z1 as well -
 * nasseg_conv_pw_bwd_kernel_id(.., z_null = 1) >= 0 - which excludes 32 -> 192, for one.
 * nasseg_irdw_config: how the two kernels are launched, 1000 waves + 10 groups + kt (workgroups of 64 * waves threads,
 * waves = 4 | 3 | 2 | 1 by the divisibility of C / 16; grid (rows, groups = C / 16 / waves); kt = 1 | 2 16-wide tiles
 * of K); 0 = not served.  For tests: together with the stride and the prologue it names the kernel that runs. */
int64_t nasseg_irdw_rows(int B, int H, int W, int K, int C, int stride, int backward);
int64_t nasseg_irdw_config(int B, int H, int W, int K, int C, int stride, int backward);
/* Training-mode BatchNorm statistics of z1 = W1 pro(x) WITHOUT computing z1: z1 is linear in pro(x), so its first and
 * second moments per output channel follow from the K-vector and K x K matrix of moments of pro(x) (one pass over the
 * block's input).  The moments are taken about a pivot - per input channel pro(x) of the block's first pixel where
 * sixteen pixels spread over the block keep to one side of 0, and 0 otherwise (the sums are then the raw ones); the
 * same in every workgroup - so that the variance is not the difference of two sums |mean|^2 / var times its size: with
 * |mean| = 200 std it is within 1e-4 of the float64 value, as from every other statistics producer.  Writes what
 * nasseg_bn_finalize writes for the stored map (to the rounding of the centred sums: fp32 per workgroup, fp64 after).
 * ws: nasseg_irdw_stats_workspace(K) floats. */
int64_t nasseg_irdw_stats_workspace(int K);
int nasseg_irdw_stats(const float* x, const float* w1, const float* in_scale, const float* in_shift, int in_act, int B,
                      int H, int W, int K, int C, float eps, float momentum, const float* gamma, const float* beta,
                      float* mean, float* invstd, float* scale, float* shift, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, float* ws, void* stream);
int nasseg_irdw_fwd(const float* x, const float* w1, const float* wdw, float* z2, const float* in_scale,
                    const float* in_shift, int in_act, const float* bn1_scale, const float* bn1_shift, int act1,
                    int B, int H, int W, int K, int C, int Ho, int Wo, int stride, float* stats, void* stream);
int nasseg_irdw_bwd(const float* x, const float* w1, const float* g, const float* z2, const float* wdw,
                    int wdw_flipped, float* ge, float* dw, float* ws, const float* in_scale, const float* in_shift,
                    int in_act, const float* bn1_scale, const float* bn1_shift, const float* bn1_mean,
                    const float* bn1_invstd, int act1, const float* bn2_scale, const float* bn2_shift,
                    const float* bn2_mean, const float* bn2_invstd, const float* bn2_sums, int bn2_train, int bn2_act,
                    int B, int H, int W, int K, int C, int Ho, int Wo, int stride, float* stats, void* stream);

/* ---- dense convolution on the fp32 matrix cores ----------------------------
 * replaces conv1x1 / conv3x3 / conv_bn / conv_bn_relu (layer_factory.py:7-24,
 * 94-122), every pointwise stage (:125-382) and the classifier heads
 * (micro_decoders.py:210-227,360-363); fused input affine+act prologue and
 * output affine/bias+act(+residual) epilogue. */
int nasseg_conv_pack_weight(const float* w, float* wp, int N, int K, int kh, int kw, int mode,
                            void* stream);
/* several weights (dense and depthwise) re-packed by one launch: dims[7*i..] =
 * N, K, kh, kw, kind, Ksrc, koff; kind 0/1/2 as mode above, 3 / 4 = depthwise plain / flipped,
 * 5 = mode 1 with flipped taps (backward-data of a stride-1 conv as a forward conv over dy);
 * Ksrc > 0 packs only input channels [koff, koff+K) of a weight with Ksrc input channels */
int nasseg_pack_weights(int count, const float* const* w, float* const* wp, const int* dims,
                        void* stream);
int nasseg_conv_fwd_pack_mode(int K, int kh, int kw);
/* y == NULL with stats != NULL: only the statistics rows are produced, nothing is stored - for a pointwise conv the
 * N-split persistent kernel serves (nasseg_conv_pointwise_kernel == 2), else an error. */
int nasseg_conv_fwd(const float* x, int ldx, const float* wp, float* y, int ldy,
                    const float* in_scale, const float* in_shift, int in_act,
                    const float* out_scale, const float* out_shift, int out_act, const float* res,
                    int ldres, int B, int Hs, int Ws, int K, int Ho, int Wo, int N, int kh, int kw,
                    int stride, int pad, int dil, int transposed, float* stats, void* stream);
/* rows of statistics a call with N output channels over B*Ho*Wo output pixels writes; K = its reduction
 * channels; pointwise: 0 = any other geometry, 1 = a 1x1, stride-1, unpadded nasseg_conv_fwd call, 2 = such a
 * nasseg_conv_bwd_data_bn call - those may take the persistent pointwise kernel (weight in LDS, inputs
 * prefetched, one statistics row per workgroup of a grid that depends on K) */
int64_t nasseg_conv_fwd_stats_blocks(int B, int Ho, int Wo, int N, int K, int pointwise);
/* ... of a FORWARD call with any kernel size: nasseg_conv_fwd_stats_blocks for 1x1 and strided forms, the tile count of
 * the LDS-tiled kernel for the stride-1 3x3 forms it takes (dilation 1 ... 3, N <= 64, maps of at least 8 x 32 pixels:
 * conv3x3 / conv3x3_dil3 of the CVPR cells, layer_factory.py:56-75).  The tile is picked per map (tiles of 64 to 256
 * pixels: whole waves of the 512 workgroups that run at once, small tiles on small maps), so the count is NOT
 * B * ceil(Ho / 8) * ceil(Wo / 32) in general.  A forward call that passes `stats` for a 3x3 geometry must size them
 * with THIS query. */
int64_t nasseg_conv_fwd_stats_rows(int B, int Ho, int Wo, int N, int K, int kh, int kw, int stride, int pad, int dil);
/* tuning / testing knob: which pointwise calls take the persistent kernel.  -2 (initial): where it measured
 * faster; v >= 0: every call it supports over at least v output pixels (0 = all, a huge value = none);
 * v == -1 only queries.  Returns the previous setting.  Outputs are bit-identical either way; BatchNorm
 * statistics differ in the rounding of their partial sums.  Row counts from nasseg_conv_fwd_stats_blocks are
 * valid for the setting they were asked under. */
int64_t nasseg_conv_pw_min_pixels(int64_t v);
/* tuning / testing knob: which pointwise calls take the N-split persistent kernel (csrc/conv_pwn.hip: input streamed
 * through an LDS ring with four 16-channel blocks in flight per workgroup, the waves of a workgroup split the output
 * channels, statistics reduced across lanes once per kernel).  0: none; 1 (initial): where it measured faster;
 * 2: every call it supports (N, K multiples of 4, N <= 256, K <= 512); v < 0 only queries.  Returns the previous
 * setting.  It is asked BEFORE nasseg_conv_pw_min_pixels' kernel.  Outputs are bit-identical either way; BatchNorm
 * statistics differ in the rounding of their partial sums; row counts from nasseg_conv_fwd_stats_blocks are valid
 * for the setting they were asked under. */
int nasseg_conv_pwn_mode(int v);
/* The general MFMA kernel on maps of at most 8192 pixels (the 11 x 11 ... 21 x 21 maps of the CVPR decoders and of the
 * MobileNetV2 tail at 321 x 321): 1 (initial) four 16-channel steps of the reduction per memory round trip instead of
 * one - with a workgroup per CU or fewer there is no other wave to hide it (960 -> 160 at 16 x 11 x 11: 60 round trips,
 * 78 us for 0.6 GFLOP); 0: one step, as on large maps.  v < 0 only queries.  Returns the previous setting.
 * Bit-identical results. */
int nasseg_conv_deep_k(int v);
/* stride-1 3x3 max pooling (nasseg_maxpool_bn_fwd / _bwd) on the strip kernels - a thread owns four rows of a column
 * and loads the 6 x 3 values their windows touch once: 1 (initial) / 0.  v < 0 only queries.  Returns the previous
 * setting.  Identical outputs. */
int nasseg_pool_strip(int v);
/* which kernel a 1x1, stride-1, unpadded call with these sizes takes under the current settings: 0 the general MFMA
 * kernel, 1 the persistent kernel whose waves own all output channels, 2 the N-split persistent kernel.  pointwise
 * as for nasseg_conv_fwd_stats_blocks (1 forward, 2 backward-data).  For measurement tools (bench.py names kernel
 * families by it). */
int64_t nasseg_conv_pointwise_kernel(int B, int Ho, int Wo, int N, int K, int pointwise);
/* 1 when a plain (not transposed, no input prologue) nasseg_conv_fwd call of this geometry takes the LDS-tiled 3x3
 * kernel (conv3x3_lds_kernel): stride 1, dilation <= 3, at least one 8 x 32 tile, N <= 64; with_stats: the call asks for
 * statistics rows (served there when N % 4 == 0).  For measurement tools, like nasseg_conv_pointwise_kernel. */
int64_t nasseg_conv_fwd_lds3x3(int B, int Ho, int Wo, int N, int K, int kh, int kw, int stride, int pad, int dil,
                               int with_stats);
/* dense twin of nasseg_dwconv_bwd_data_bn (arguments as nasseg_conv_fwd, transposed) */
int nasseg_conv_bwd_data_bn(const float* dy, int lddy, const float* wp, float* g, int ldg,
                            const float* z, int ldz, const float* scale, const float* shift,
                            const float* mean, const float* invstd, int act, int B, int Hs, int Ws,
                            int K, int Ho, int Wo, int N, int kh, int kw, int stride, int pad,
                            int dil, float* stats, void* stream);
/* 1: nasseg_conv_wgrad runs this call on its LDS-tiled 3x3 kernel (stride 1, dilation <= 2, N <= 32,
 * K % 16 == 0, maps of at least 64 tiles of 8 x 32 pixels: the class heads, src/nn/micro_decoders.py:215,226,363),
 * whose summation order differs from the generic kernel that nasseg_conv_wgrad_many always uses */
int nasseg_conv_wgrad_lds3x3(int B, int Hs, int Ws, int K, int Ho, int Wo, int N, int kh, int kw, int stride,
                             int pad, int dil);
int64_t nasseg_conv_wgrad_workspace(int B, int Ho, int Wo, int N, int K, int kh, int kw);
/* weight gradients are read by the optimiser only: nasseg_conv_wgrad / nasseg_dwconv_wgrad called
 * with dw == NULL leave their per-slab partial sums in ws, and this call finalises many layers
 * with one launch per 16: dims[5*i..] = partial rows, taps, N, K, flat (depthwise: N = C, K = 1) */
int nasseg_wgrad_finalize_many(int count, const float* const* partial, float* const* dw,
                               const int* dims, void* stream);
/* first stage of `count` small layers in launches of up to 8 layers of one kernel specialisation
 * running side by side: desc[20*i..] = the arguments of nasseg_conv_wgrad from x to dil (without
 * dw), pointers as integers; equals nasseg_conv_wgrad(..., dw = NULL, ...) per layer */
int nasseg_conv_wgrad_many(int count, const int64_t* desc, void* stream);
/* the depthwise twin: desc[16*i..] = the arguments of nasseg_dwconv_wgrad from x to dil, without dw */
int nasseg_dwconv_wgrad_many(int count, const int64_t* desc, void* stream);

/* Weight gradient fused with the second half of a BatchNorm backward (replaces one nasseg_bn_bwd_apply pass
 * per layer; autograd of BatchNorm2d + Conv2d at src/nn/layer_factory.py:96-98,117-122,125-158,243-255).
 * The conv's output z went through BatchNorm (+ activation); g is the gradient w.r.t. that output with the
 * activation mask applied (bn_act == 0: as nasseg_conv_bwd_data_bn / nasseg_dwconv_bwd_data_bn leave it, or no
 * activation) or still to be applied here (bn_act != 0: g' = g * act'(scale*z + shift), g' for g below);
 * sums[2][N] = {sum g, sum g*xhat} over the M pixels (nasseg_bn_bwd_reduce / nasseg_rows_sum).  On load
 *   dz = scale*(g - sums0/M - xhat*sums1/M)   (bn_train; else dz = scale*g),  xhat = (z - mean)*invstd,
 * from which the weight gradient is computed AND which is written to dz for the backward-data call.
 * nasseg_conv_wgrad_bn: pointwise convs (1x1, stride 1), K % 4 == 0, N % 4 == 0, workspace of
 * nasseg_conv_wgrad_workspace(B,H,W,N,K,1,1).  nasseg_dwconv_wgrad_bn: nasseg_dwconv_strip_ok geometries.
 * dw == NULL: first stage only (nasseg_wgrad_finalize_many). */
int nasseg_conv_wgrad_bn(const float* x, int ldx, const float* g, int ldg, const float* z, int ldz, float* dz,
                         int lddz, float* dw, float* ws, const float* in_scale, const float* in_shift, int in_act,
                         const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd,
                         const float* bn_sums, int bn_train, int bn_act, int B, int H, int W, int K, int N, void* stream);
/* nasseg_conv_wgrad_bn for a small-K k x k conv (kh*kw*K <= 64: nasseg_conv_fwd_pack_mode == 2 - MobileNetV2's
 * stem, the first op of its chain) whose input needs no gradient: the BatchNorm backward is applied to g on load and dz is
 * never written (instead of nasseg_bn_bwd_apply + nasseg_conv_wgrad).  Geometry as nasseg_conv_wgrad. */
int nasseg_conv_wgrad_bn_flat(const float* x, int ldx, const float* g, int ldg, const float* z, int ldz, float* dw,
                              float* ws, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                              const float* bn_invstd, const float* bn_sums, int bn_train, int bn_act, int B, int Hs,
                              int Ws, int K, int Ho, int Wo, int N, int kh, int kw, int stride, int pad, int dil,
                              void* stream);
int nasseg_dwconv_wgrad_bn(const float* x, const float* g, const float* z, float* dz, float* dw, float* ws,
                           const float* in_scale, const float* in_shift, int in_act, const float* bn_scale, const float* bn_shift,
                           const float* bn_mean, const float* bn_invstd, const float* bn_sums, int bn_train, int bn_act,
                           int B, int H, int W, int C, int Ho, int Wo, int K, int stride, int pad, int dil,
                           void* stream);
/* The whole backward of a pointwise conv followed by BatchNorm in one kernel: BatchNorm backward on load (as
 * nasseg_conv_wgrad_bn), weight gradient AND input gradient; dz never reaches HBM.  wb = the weight packed for
 * backward-data ([K][N], pack mode 1); dx [B][H][W][K]; ws: nasseg_conv_pw_bwd_slabs(...) * N * K floats (0 slabs:
 * no fused kernel for these channel counts - N*K <= 6144 with K <= 64, or N <= 64 with K <= 384); dx_act != 0
 * (= in_act): dx additionally multiplied by in_act'(in_scale*x + in_shift), i.e. the gradient w.r.t. the affine's
 * output (w.r.t. x itself for a bare activation); dw == NULL: partial rows only.  dx_stats != NULL (K <= 64; x is the
 * raw output of a BatchNorm with statistics in_mean / in_invstd, dx_act = in_act): also that BatchNorm's backward
 * sums {sum dx, sum dx*xhat} per slab, rows [slabs][2][K] for nasseg_rows_sum (buffer: slabs + 64 rows).
 * dx_res != NULL (K % 4 == 0, no dx_stats): a [P][K] map added to dx after the mask - the gradient of a skip connection
 * that x feeds as well (InvertedResidual, src/nn/layer_factory.py:276-321: autograd then has nothing to accumulate). */
int64_t nasseg_conv_pw_bwd_slabs(int B, int H, int W, int K, int N);
/* 1: nasseg_conv_pw_bwd_bn loads z for this geometry; 0: it rebuilds z = W x from the input tile it stages anyway (the
 * narrow kernel with its weight in LDS: same operand mapping and accumulation order as the forward kernels, the same
 * bits) and z is not read.  A z that is passed must BE the conv's raw output; z == NULL says it was never stored
 * (nasseg_irdw_fwd) and forces the rebuild - an error where no kernel can: ask nasseg_conv_pw_bwd_kernel_id with
 * z_null = 1.  For measurement tools and tests. */
int64_t nasseg_conv_pw_bwd_reads_z(int B, int H, int W, int K, int N);
/* The kernel nasseg_conv_pw_bwd_bn launches for this geometry under the current nasseg_conv_pw_bwd_rz_min_pixels; -1:
 * none, the call fails.  10000 + KC: the wide kernel, KC = 2 .. 6 chunks of 64 input channels; otherwise
 * 100 nt + 10 kt + rz: the narrow kernel holding nt x kt 16-wide tiles of N x K per wave, rz = 1: it rebuilds z,
 * rz = 0: it loads z.  z_null != 0: what a call with z == NULL launches - a kernel that rebuilds z (rz = 1) or none.
 * Kernels that rebuild z exist for K <= 32 with N <= 96 (nt <= 6) and for 16 < K <= 32 with 96 < N <= 144 (nt = 9,
 * kt = 2: 24 -> 144) - not for K <= 16 with N > 96, nor for N > 144.  Whoever drops z (functional._irdw_ok) asks here
 * first.  The launch itself selects through the same table. */
int64_t nasseg_conv_pw_bwd_kernel_id(int B, int H, int W, int K, int N, int z_null);
/* pixels from which nasseg_conv_pw_bwd_bn rebuilds z (where it can: K <= 32, N <= 96): 2^18 initially; 0: every
 * supported geometry, a huge value: none.  v < 0 only queries.  Returns the previous setting. */
int64_t nasseg_conv_pw_bwd_rz_min_pixels(int64_t v);
int nasseg_conv_pw_bwd_bn(const float* x, const float* g, const float* z, const float* wb, float* dx, float* dw,
                          float* ws, const float* in_scale, const float* in_shift, int in_act, int dx_act,
                          const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_invstd,
                          const float* bn_sums, int bn_train, int bn_act, int B, int H, int W, int K, int N,
                          const float* in_mean, const float* in_invstd, float* dx_stats, const float* dx_res,
                          void* stream);
int nasseg_conv_wgrad(const float* x, int ldx, const float* dy, int lddy, float* dw, float* ws,
                      const float* in_scale, const float* in_shift, int in_act, int B, int Hs,
                      int Ws, int K, int Ho, int Wo, int N, int kh, int kw, int stride, int pad,
                      int dil, void* stream);

/* ---- per-channel reductions / BatchNorm ------------------------------------
 * replaces nn.BatchNorm2d (layer_factory.py:56-75,94-158,369-382), x.mean(2).mean(3)
 * in GAPConv1x1 (:181-195), bias / ParamSum coefficient gradients (:353-366). */
int64_t nasseg_colred_workspace(int S, int64_t R, int C);
int nasseg_colred(int mode, const float* a, int64_t lda, const float* b, int64_t ldb,
                  const float* c, int64_t ldc, float* out, float* ws, int S, int64_t R, int C,
                  float mul, void* stream);
int nasseg_bn_stats(const float* x, int64_t ldx, int64_t M, int C, float eps, float momentum,
                    const float* gamma, const float* beta, float* mean, float* invstd,
                    float* scale, float* shift, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked, float* ws, void* stream);
/* partial: rows [nblk, nblk + 64) of the buffer are scratch of the two-level reduction (hence not const) */
int nasseg_bn_finalize(float* partial, int nblk, int64_t M, int C, float eps, float momentum,
                       const float* gamma, const float* beta, float* mean, float* invstd,
                       float* scale, float* shift, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, void* stream);
int nasseg_bn_eval_params(int C, float eps, const float* gamma, const float* beta,
                          const float* running_mean, const float* running_var, float* mean,
                          float* invstd, float* scale, float* shift, void* stream);
int nasseg_bn_bwd_reduce(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M,
                         int C, const float* scale, const float* shift, const float* mean,
                         const float* invstd, int act, float* sums, float* ws, void* stream);
/* sums[cols] = sum of the rows of partial[nblk][cols] (buffer needs nblk + 64 rows: scratch of the two-level
 * reduction, written - hence not const) */
int nasseg_rows_sum(float* partial, int nblk, int cols, float* out, void* stream);
int nasseg_bn_bwd_apply(const float* dy, const float* x, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* sums, int64_t M,
                        int C, int train, int act, float* dx, void* stream);
/* BatchNorm backward whose consumer adds up the partial rows of the sums itself (the small maps of the CVPR cells,
 * micro_decoders.py:54-121: a row-summing launch in front of every BatchNorm backward costs a dependent ~5 us).
 * nasseg_bn_bwd_reduce_rows: the first stage of nasseg_bn_bwd_reduce only - rows [nasseg_colred_rows(1, M, C)][2][C] in
 * a buffer of nasseg_colred_workspace(1, M, C) floats.  nasseg_bn_bwd_apply_rows: nasseg_bn_bwd_apply from such rows
 * (or the statistics rows of a fused backward-data kernel): every workgroup adds them in fp64 in a fixed order; sums_out
 * (null or [2][C]) receives {sum g, sum g*xhat}.  Meant for nrows * 2 * C * 4 <= nasseg_bn_bwd_apply_rows_max_bytes(). */
int64_t nasseg_colred_rows(int S, int64_t R, int C);
int64_t nasseg_bn_bwd_apply_rows_max_bytes(void);
int nasseg_bn_bwd_reduce_rows(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int C,
                              const float* scale, const float* shift, const float* mean, const float* invstd, int act,
                              float* rows, void* stream);
int nasseg_bn_bwd_apply_rows(const float* dy, const float* x, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const float* rows, int nrows, float* sums_out, int64_t M, int C,
                             int train, int act, float* dx, void* stream);

/* ---- elementwise / copies ----------------------------------------------------
 * BN apply + ReLU/ReLU6 + residual (layer_factory.py:94-158), cell sums
 * (micro_decoders.py:48-51,110-121), ParamSum (:353-366), Skip / Zero (:268-297),
 * torch.cat (+F.relu) (micro_decoders.py:11-25,251; layer_factory.py:369-382). */
int nasseg_affine_act(const float* x, const float* scale, const float* shift, const float* res,
                      float* y, int64_t n, int C, int act, void* stream);
int nasseg_axpby(const float* a, const float* b, const float* alpha, const float* beta, float* y,
                 int64_t n, int C, int act, void* stream);
/* y = ca[c] * act_a(xa*sa[c] + ha[c]) + cb[c] * act_b(xb*sb[c] + hb[c]): the sum of two op outputs (cell sums,
 * micro_decoders.py:48-51,110-121; ParamSum's coefficients, layer_factory.py:353-366) whose last BatchNorm +
 * activation is applied as they are loaded - the normalised maps are never written.  Null vectors: scale /
 * coefficient 1, shift 0. */
int nasseg_add_act2(const float* xa, const float* sa, const float* ha, int act_a, const float* ca, const float* xb,
                    const float* sb, const float* hb, int act_b, const float* cb, float* y, int64_t n, int C,
                    void* stream);
int nasseg_act_bwd(const float* dy, const float* ref, float* dx, int64_t n, int act, void* stream);
int nasseg_fill(float* y, int64_t n, float v, void* stream);
int nasseg_chan_copy(const float* x, int64_t ldx, int xoff, float* y, int64_t ldy, int yoff,
                     const float* mref, int64_t ldm, int moff, int64_t P, int C, int act, int mact,
                     void* stream);
int nasseg_chan_fold(const float* dy, float* dx, int64_t P, int C, int rep, void* stream);
/* dst[i] = src[idx[i]], rows of row_bytes bytes, idx an int64 DEVICE array clamped to [0, n_src):
 * the batch of the task0 feature cache (Xy_train[k][indices], src/engine/trainer.py:128-137) */
int nasseg_gather_rows(const void* src, const int64_t* idx, void* dst, int n, int64_t row_bytes,
                       int64_t n_src, void* stream);

/* ---- pooling: Pool (layer_factory.py:161-178); mode 0 max, 1 avg ------------- */
int nasseg_pool_fwd(int mode, const float* x, float* y, uint8_t* idx, int B, int H, int W, int C,
                    int Ho, int Wo, int K, int stride, int pad, void* stream);
int nasseg_pool_bwd(int mode, const float* dy, const uint8_t* idx, float* dx, int B, int H, int W,
                    int C, int Ho, int Wo, int K, int stride, int pad, void* stream);
/* Pool's 1x1 conv + BatchNorm followed by 3x3 max pooling (src/nn/layer_factory.py:161-178) without the
 * normalised map: the pooling applies scale*z + shift to the conv's raw output as it loads; backward gives
 * the gradient w.r.t. the BatchNorm's output together with the per-workgroup sums of its backward. */
int64_t nasseg_maxpool_bn_bwd_blocks(int B, int H, int W, int C, int K, int stride, int pad);
int nasseg_maxpool_bn_fwd(const float* z, const float* scale, const float* shift, float* y, uint8_t* idx,
                          int B, int H, int W, int C, int Ho, int Wo, int stride, int pad, void* stream);
int nasseg_maxpool_bn_bwd(const float* dy, const uint8_t* idx, const float* z, const float* mean,
                          const float* invstd, float* g, float* stats, int B, int H, int W, int C, int Ho,
                          int Wo, int stride, int pad, void* stream);

/* ---- resize: nn.Upsample / F.interpolate bilinear, align_corners=False
 * (layer_factory.py:190-194,338-350; micro_decoders.py:11-25,46-51; trainer.py:141-143,
 * 236-238,245-247; inference.py:58-60) and nearest label resize (trainer.py:43-49,236-238). */
/* One input of ConcatReduce's torch.cat (src/nn/layer_factory.py:369-382, after Adapt's resize :316-350)
 * written into its channel slice of the slab: resized when its size differs, the producer's still pending
 * BatchNorm + activation applied as the source is loaded, and the slab's own BatchNorm statistics emitted
 * as per-workgroup rows for nasseg_bn_finalize (the slab is not read again for them).  Backward
 * (nasseg_cat_src_bwd): the slab BatchNorm's backward applied to one input's slice, masked with the pending
 * activation's derivative, with the producer's BatchNorm-backward sums as per-workgroup rows. */
int64_t nasseg_cat_src_blocks(int B, int Ho, int Wo, int C);
/* Backward of ParamSum (a[c]*x + b[c]*y, layer_factory.py:353-366) for both operands from one read of the gradient:
 * an operand may be a conv chain's raw output with its BatchNorm + activation pending (ts*: mean | invstd | scale |
 * shift; null: a finished map).  g* = c* dy act'(...) - masked, with the producer's BatchNorm-backward sums as rows
 * part* [nasseg_cat_src_blocks(B, H, W, C) + 64][2][C] - and cpart [blocks + 64][2][C]: rows of the coefficient
 * gradients {sum dy*x, sum dy*y} (nasseg_rows_sum finishes them). */
int nasseg_psum_bwd(const float* dy, const float* za, const float* tsa, int act_a, const float* ca, float* ga,
                    float* part_a, const float* zb, const float* tsb, int act_b, const float* cb, float* gb,
                    float* part_b, float* cpart, int B, int H, int W, int C, void* stream);
/* Gradient junction of a node with several consumers (a cell's node read by several ops, a block's output read by
 * later blocks and collect_all: micro_decoders.py:95-121,380-398; torch's autograd adds such gradients pairwise, one
 * launch and three tensor passes per add): out = g0 + g1 + ... + g(n-1), 1 <= n <= 8, added in that order, all dense
 * [B*H*W][C]; unused pointers null.  With z / tstats (the node is a conv chain's raw output whose BatchNorm + activation
 * is pending; tstats: mean | invstd | scale | shift) out is also multiplied by act'(scale*z + shift) and part
 * [nasseg_cat_src_blocks(B, H, W, C) + 64][2][C] (null: none) receives that BatchNorm's backward sums {sum out,
 * sum out * xhat} as rows. */
int nasseg_grad_junction(const float* g0, const float* g1, const float* g2, const float* g3, const float* g4,
                         const float* g5, const float* g6, const float* g7, int n, const float* z, const float* tstats,
                         int act, float* out, float* part, int B, int H, int W, int C, void* stream);
int nasseg_cat_src_fwd(const float* x, const float* scale, const float* shift, int act, float* y, int64_t ldy,
                       int yoff, float* stats, int B, int Hi, int Wi, int C, int Ho, int Wo, void* stream);
int nasseg_cat_src_bwd(const float* du, const float* slab, int64_t ld, int off, const float* sscale,
                       const float* smean, const float* sinvstd, const float* sums, int train, const float* z,
                       const float* tstats, int act, float* g, float* part, int B, int Ho, int Wo, int C, int Hi,
                       int Wi, void* stream);
/* nasseg_bilinear_bwd with the result multiplied by act'(scale*z + shift) at the source's size: the gradient of a
 * resized pending input, masked for its producer (its sums come from nasseg_cat_src_bwd). */
int nasseg_bilinear_bwd_act(const float* dy, int64_t lddy, int dyoff, const float* z, const float* scale,
                            const float* shift, int act, float* dx, int B, int Hi, int Wi, int C, int Ho, int Wo,
                            float* ws, void* stream);
int nasseg_bilinear_fwd(const float* x, float* y, int64_t ldy, int yoff, int B, int Hi, int Wi,
                        int C, int Ho, int Wo, int act, void* stream);
/* nn.Upsample(size, mode="bilinear", align_corners=True) - src/kd/rf_lw/model_lw_v2.py:258,266,274 (the
 * distillation teacher's decoder); forward only, C % 4 == 0, dense output [B][Ho][Wo][C] */
int nasseg_bilinear_ac_fwd(const float* x, float* y, int B, int Hi, int Wi, int C, int Ho, int Wo,
                           void* stream);
int64_t nasseg_bilinear_bwd_workspace(int B, int Hi, int Wi, int C, int Ho, int Wo);
int nasseg_bilinear_bwd(const float* dy, int64_t lddy, int dyoff, float* dx, int B, int Hi, int Wi,
                        int C, int Ho, int Wo, float* ws, void* stream);
int nasseg_nearest_label(const void* x, int elem_size, int64_t* y, int B, int Hi, int Wi, int Ho,
                         int Wo, void* stream);

/* ---- loss: nn.LogSoftmax() + nn.NLLLoss2d(ignore_index=255)
 * (main_search.py:435; trainer.py:144-146,239-241) -------------------------------- */
int64_t nasseg_ce_workspace(void);
int nasseg_ce_fwd(const float* logits, const void* target, int elem_size, int64_t P, int C,
                  int ignore, float* out, float* ws, void* stream);
int nasseg_ce_bwd(const float* logits, const void* target, int elem_size, const float* stats,
                  const float* gscale, int64_t P, int C, int ignore, float* dlogits, void* stream);
/* The same loss plus the distillation term kd_crit = nn.MSELoss() of the decoder-only step
 * (main_search.py:455-458; trainer.py:147-149: loss + kd_coeff * kd_crit(output, kd_y)) from one pass over the
 * logits.  teacher: fp32 [P][C] like the logits, whatever their storage.  Forward: ce = the NLL, bit-identical to
 * nasseg_ce_fwd's out[0]; mse = sum((x - t)^2) / (P*C) over ALL elements (ignored pixels included: MSELoss has no
 * ignore index); stats = nasseg_ce_fwd's out; ws: nasseg_ce_mse_workspace() floats.  ce and mse are two separate
 * device scalars.  Backward: dlogits = g_ce * dNLL + g_mse * 2 (x - t) / (P*C), written once (g_ce, g_mse: device
 * scalars, null = 1); with g_mse = 0 it is bit-identical to nasseg_ce_bwd's.  Deterministic: per-block partials,
 * fixed-order fp64 finalize. */
int64_t nasseg_ce_mse_workspace(void);
int nasseg_ce_mse_fwd(const float* logits, const void* target, int elem_size, const float* teacher, int64_t P,
                      int C, int ignore, float* ce, float* mse, float* stats, float* ws, void* stream);
int nasseg_ce_mse_bwd(const float* logits, const void* target, int elem_size, const float* teacher,
                      const float* stats, const float* g_ce, const float* g_mse, int64_t P, int C, int ignore,
                      float* dlogits, void* stream);

/* Class-weighted cross-entropy with hard-example selection: what a caller gets who hands the reference's call
 * sites - segm_crit of src/main_search.py:435, used at src/engine/trainer.py:144-146,239-250 - a criterion with
 * class weights (nn.NLLLoss2d(weight=w)) or with online hard-example mining (absent from the reference).
 * Pixel p is valid iff its label t != ignore and 0 <= t < C; l_p = logsumexp(x_p) - x_p[t], computed exactly as
 * nasseg_ce_fwd computes it.  select != 0 (needs min_kept >= 1, 0 <= keep_fraction <= 1): n = valid pixels,
 * k = min(n, max(min_kept, ceil(keep_fraction * n))) (in double), tau = min(t_loss, k-th largest l_p); a valid pixel
 * is kept iff l_p >= tau on the fp32 values (ties at tau are all kept; t_loss = +inf: top-k only).  select == 0:
 * every valid pixel is kept, tau = -inf.  Selection ignores the weights.
 *   loss = sum_kept w[t_p] l_p / sum_kept w[t_p]      (weight: fp32 [C], null = ones; nothing kept: NaN)
 *   stats = {sum_kept w, tau};  counts = {k, n, pixels kept};  pixel_loss[p] = l_p, -1 where p is not valid
 * Backward (tau and the kept set are constants): dlogits = gscale * w[t_p] * (softmax(x_p) - onehot(t_p)) / stats[0]
 * on kept pixels, exact zeros on all others, written once (gscale: device scalar, null = 1).  With unit weights
 * and no selection loss and dlogits are bit-identical to nasseg_ce_fwd's / nasseg_ce_bwd's.
 * nasseg_ohem_threshold is the selection alone, over any fp32 array: entries < 0 do not take part; counts[2] =
 * entries >= tau among those that do.  An exact radix select (11 + 11 + 10 bits of the fp32 pattern) on the device:
 * no host synchronisation, no allocation, integer atomics only - deterministic, capturable.
 * ws: nasseg_ohem_workspace() 4-byte words / nasseg_ce_sel_workspace() floats.  P < 2^32. */
int64_t nasseg_ohem_workspace(void);
int nasseg_ohem_threshold(const float* pixel_loss, int64_t P, float t_loss, int64_t min_kept, double keep_fraction,
                          float* tau, int64_t* counts, void* ws, void* stream);
int64_t nasseg_ce_sel_workspace(void);
int nasseg_ce_sel_fwd(const float* logits, const void* target, int elem_size, const float* weight, int64_t P, int C,
                      int ignore, int select, float t_loss, int64_t min_kept, double keep_fraction, float* loss,
                      float* stats, int64_t* counts, float* pixel_loss, float* ws, void* stream);
int nasseg_ce_sel_bwd(const float* logits, const void* target, int elem_size, const float* weight,
                      const float* pixel_loss, const float* stats, const float* gscale, int64_t P, int C, int ignore,
                      float* dlogits, void* stream);

/* The same cross-entropy plus a region-overlap term (soft Jaccard / Dice / Tversky; absent from the reference, whose
 * reward is the mean IoU this term is the differentiable form of), computed in the two passes over the logits the
 * cross-entropy makes anyway.  Valid pixels as above; q_p = softmax(x_p) in fp32 from the cross-entropy's own max
 * and exp values.  Over ALL valid pixels (selection does not thin the term, class weights do not enter it):
 *   I_c = sum_p q_pc [t_p == c],  S_c = sum_p q_pc,  N_c = sum_p [t_p == c]
 *   D_c = (1 - alpha - beta) I_c + alpha S_c + beta N_c + smooth,  T_c = (I_c + smooth) / D_c
 *   K = {c : N_c > 0} (all_classes != 0: every class; needs smooth > 0)
 *   loss_region = 1 - sum_{c in K} T_c / |K|   (K empty: exactly 0, and an exactly zero gradient)
 *   loss = loss_ce + region_weight * loss_region   (with_ce == 0: region_weight * loss_region; weight, stats, counts,
 *                                                   pixel_loss may then be null and select must be 0)
 * alpha = beta = 1: Jaccard; 0.5, 0.5: Dice; alpha, beta, smooth >= 0, alpha + beta > 0.  loss_ce, stats, counts,
 * pixel_loss: bit-identical to nasseg_ce_sel_fwd's loss, stats, counts, pixel_loss.  The sums come from
 * per-workgroup fp64 rows added in fp64 in a fixed order by one finalize launch (no atomics), which also writes
 *   sums = {I_c} | {S_c} (fp32 [2C]);  ncls = {N_c} | |K| (int64 [C + 1])
 *   coef = {-a_c / |K|} | {-b_c / |K| - m} (fp32 [2C]; a_c = b_c = 0 outside K),  a_c = dT_c/dI_c = (D_c -
 *   (I_c + smooth) (1 - alpha - beta)) / D_c^2,  b_c = dT_c/dS_c = -(I_c + smooth) alpha / D_c^2,  m = the mean of the
 *   -b_c / |K| over the C classes: a constant added to every G_pc leaves the gradient below as it is (sum_c q_pc
 *   = 1), and without their mean the fp32 terms have less to cancel.
 * Backward, with G_pc = coef[C + c] + [t_p == c] coef[c]:
 *   dlogits = gscale * (cross-entropy part as nasseg_ce_sel_bwd, kept pixels only
 *                       + region_weight * q_pj (G_pj - sum_c G_pc q_pc), every valid pixel)
 * exact zeros on invalid pixels, written once; at region_weight = 0 bit-identical to nasseg_ce_sel_bwd's.
 * The logits are read once per direction.  Any C (C <= 63 and 16-byte aligned logits: the LDS-tiled kernels).
 * No host synchronisation, no allocation: capturable.  ws: nasseg_ce_region_workspace(C) floats, 8-byte aligned. */
int64_t nasseg_ce_region_workspace(int C);
int nasseg_ce_region_fwd(const float* logits, const void* target, int elem_size, const float* weight, int64_t P,
                         int C, int ignore, int with_ce, int select, float t_loss, int64_t min_kept,
                         double keep_fraction, double alpha, double beta, double smooth, int all_classes,
                         double region_weight, float* loss, float* loss_ce, float* loss_region, float* stats,
                         int64_t* counts, float* pixel_loss, float* coef, float* sums, int64_t* ncls, float* ws,
                         void* stream);
int nasseg_ce_region_bwd(const float* logits, const void* target, int elem_size, const float* weight,
                         const float* pixel_loss, const float* stats, const float* coef, const float* gscale,
                         int with_ce, double region_weight, int64_t P, int C, int ignore, float* dlogits,
                         void* stream);

/* Full-size cross-entropy: the criterion of nasseg_ce_sel_fwd taken at the LABELS' size, the bilinear up-sampling of
 * the logits fused in.  It replaces, for a caller who asks for it, the label resize of src/engine/trainer.py:141-143,
 * 236-238 (labels nearest-resized down to the logits) and the up-sampling of the auxiliary heads of :245-250 - the
 * loss is then taken where validate() (src/engine/inference.py:55-66) scores: on the logits resized to the labels.
 * logits [B][h][w][C], labels [B][H][W] (uint8 / int64) at ANY size, larger than, equal to or smaller than (h, w), per
 * axis.  For label pixel (b, Y, X): ly = lin_coeff(Y, h/H, h, H), lx = lin_coeff(X, w/W, w, W) (bilinear,
 * align_corners = False, torch's source index in fp32) and for every channel
 *   top = l0x x00 + l1x x01,  bot = l0x x10 + l1x x11,  v_c = l0y top + l1y bot
 * with every product and every sum rounded to fp32 on its own - bit for bit the row nasseg_argmax_cm takes its argmax
 * of; equal sizes are the identity.  A label pixel is valid iff t != ignore and 0 <= t < C;
 * l_p = logsumexp(v) - v_t with max, expf and logf as nasseg_ce_fwd.  Selection, loss, stats, counts and the NaN rule
 * are literally nasseg_ce_sel_fwd's over the P = B*H*W label pixels (the selection IS nasseg_ohem_threshold run over
 * pixel_loss).  Per pixel nothing but pixel_loss[p] (-1 where not valid) and lse[p] = logsumexp(v) is written: no
 * tensor of B*H*W*C elements exists in either direction.
 * Backward (tau and the kept set are constants): with g_pc = gscale * w[t_p] * (exp(v_pc - lse_p) - [c == t_p]) /
 * stats[0] on kept pixels and 0 elsewhere,
 *   dlogits[b][i][j][c] = sum_{Y, X} Wy(Y, i) Wx(X, j) g_(b,Y,X),c,   Wy(Y, i) = l0y [i0(Y) == i] + l1y [i1(Y) == i]
 * (Wx alike), a gather in a fixed order (Y, then X, ascending) in fp32; a logit no label pixel touches gets an exact
 * zero; stored in the logits' type, written once.  Sums over pixels: per-workgroup partial rows added in fp64 in a
 * fixed order by one finalize launch.  No float atomics, no host synchronisation, no allocation, a launch geometry
 * that depends on the shapes alone: capturable and bit-reproducible.
 * B*H*W < 2^32, B*h*w*C < 2^31, C >= 2, and B * ceil(h/8) * ceil(w/8) * ceil(C/64) < 2^24 (the backward's workgroups:
 * one per 8 x 8 tile of logits and 64 channels - a limit that only maps thinner than a tile can reach before the others).
 * ws: nasseg_ce_up_workspace floats (0: bad shape) - a function of the grid alone, not of the pixel count. */
int64_t nasseg_ce_up_workspace(int B, int h, int w, int C, int H, int W);
int nasseg_ce_up_fwd(const float* logits, const void* target, int elem_size, const float* weight, int B, int h, int w,
                     int C, int H, int W, int ignore, int select, float t_loss, int64_t min_kept, double keep_fraction,
                     float* loss, float* stats, int64_t* counts, float* pixel_loss, float* lse, float* ws,
                     void* stream);
int nasseg_ce_up_bwd(const float* logits, const void* target, int elem_size, const float* weight,
                     const float* pixel_loss, const float* lse, const float* stats, const float* gscale, int B, int h,
                     int w, int C, int H, int W, int ignore, float* dlogits, void* stream);

/* Row-indexed twins of the two entry points above, for labels that live in a cache (the task0 cache's full-size
 * labels, engine/trainer.py: populate_task0(full_size_labels=True)): target is the WHOLE cache, uint8 / int64
 * [n_rows][H][W], and rows a DEVICE array of B cache rows - the index nasseg_gather_rows takes; image b of the logits
 * meets target[clamp(rows[b], 0, n_rows - 1)] (the clamp is a memory-safety net only: the host checks the range).
 * Repeated and unordered rows are legal.  pixel_loss and lse stay the batch's, [B][H][W]; the workspace is
 * nasseg_ce_up_workspace(B, h, w, C, H, W).  Everything else - validity, selection, loss, stats, counts, the NaN rule,
 * the backward - is as above, and so is every bit: the result is that of the un-indexed entry point on a gathered copy
 * target[rows] (the same kernels, launch geometry, order of sums and finalize; only the address of an image's labels
 * differs - in the forward, in the weighted sum pass and in the backward's gather), which is never written.  The
 * limits above bound the BATCH; the cache may be larger (rows[b]*H*W is 64-bit).  Neither the cache nor the table is
 * written. */
int nasseg_ce_up_rows_fwd(const float* logits, const void* target, int elem_size, const int64_t* rows, int64_t n_rows,
                          const float* weight, int B, int h, int w, int C, int H, int W, int ignore, int select,
                          float t_loss, int64_t min_kept, double keep_fraction, float* loss, float* stats,
                          int64_t* counts, float* pixel_loss, float* lse, float* ws, void* stream);
int nasseg_ce_up_rows_bwd(const float* logits, const void* target, int elem_size, const int64_t* rows, int64_t n_rows,
                          const float* weight, const float* pixel_loss, const float* lse, const float* stats,
                          const float* gscale, int B, int h, int w, int C, int H, int W, int ignore, float* dlogits,
                          void* stream);

/* Full-size cross-entropy plus the region-overlap term (soft Jaccard / Dice / Tversky), both taken at the LABELS'
 * size with the bilinear up-sampling of the logits fused in: the differentiable form of the mean IoU where
 * validate() (src/engine/inference.py:55-66) measures it - on the logits resized up to the labels - instead of on the
 * labels resized down to the logits (src/engine/trainer.py:141-146,236-250).  Notation: "Full-size cross-entropy" and
 * the region-overlap term above; nothing about either changes.
 * logits [B][h][w][C], labels [B][H][W] (uint8 / int64) at any size per axis.  For label pixel p = (b, Y, X) the row
 * v_p is the interpolated row of nasseg_ce_up_fwd, bit for bit (the same lin_coeff, top / bot / v, every product and
 * sum rounded on its own); p is valid iff t_p != ignore and 0 <= t_p < C; lse_p = logsumexp(v_p) and pixel_loss[p]
 * are exactly what nasseg_ce_up_fwd writes (pixel_loss and lse are written - and needed by the backward - also with
 * with_ce == 0).
 * Forward: q_pc = expf(v_pc - lse_p) in fp32 - the value the full-size backward uses, and the one definition of q in
 * every pass here.  Over ALL valid label pixels (selection does not thin the term, class weights do not enter it):
 *   I_c = sum_p q_pc [t_p == c],  S_c = sum_p q_pc,  N_c = sum_p [t_p == c]
 * and D_c, T_c, K, loss_region, coef, sums and ncls are literally those of nasseg_ce_region_fwd (alpha, beta, smooth,
 * all_classes, "K empty: exactly 0 and an exactly zero gradient", the mean-removed coef[C + c]): the same finalize
 * kernel runs on this path's partial rows.  loss = loss_ce + region_weight * loss_region; with_ce == 0: region_weight *
 * loss_region, select must be 0, and weight, stats and counts may be null.  loss_ce, stats, counts, pixel_loss and lse
 * are bit-identical to nasseg_ce_up_fwd's on the same input, selection included.  Class sums: fp32 within a tile of
 * 256 label pixels, fp64 across a workgroup's tiles, one fp64 row per workgroup (at most 1024), the rows added in a
 * fixed order by the finalize launch.  One more launch after the finalize interpolates every valid pixel's row once
 * more and writes
 *   gdot[p] = sum_c G_pc q_pc,  G_pc = coef[C + c] + [t_p == c] coef[c]   (fp32 [B][H][W]; 0 where p is not valid)
 * so that per label pixel three fp32 values are kept - pixel_loss, lse, gdot - and nothing of B*H*W*C elements exists
 * in either direction.
 * Backward:
 *   dlogits[b][i][j][c] = sum_{Y, X} Wy(Y, i) Wx(X, j) ( [p kept] gscale w[t_p] (q_pc - [c == t_p]) / stats[0]
 *                                                        + gscale region_weight q_pc (G_pc - gdot_p) )
 * over the valid label pixels in the gather order of nasseg_ce_up_bwd (Y, then X, ascending), in fp32: a valid pixel
 * the selection did not keep still contributes its region part.  A logit no valid label pixel reaches gets an exact
 * zero; written once, in the logits' type; at region_weight = 0 (with_ce != 0) bit-identical to nasseg_ce_up_bwd's -
 * the launch is then that entry point's own.
 * No float atomics, no host synchronisation, no allocation, a launch geometry that depends on the shapes alone:
 * capturable and bit-reproducible.  Shape limits: those of nasseg_ce_up_fwd.  ws: nasseg_ce_up_region_workspace
 * floats, 8-byte aligned (0: bad shape) - a function of the grid and of C, not of the pixel count.
 * The _rows_ twins read a label cache [n_rows][H][W] through a device table of B rows exactly as
 * nasseg_ce_up_rows_fwd / _bwd do: the result is that of the un-indexed call on target[rows], bit for bit; neither the
 * cache nor the table is written. */
int64_t nasseg_ce_up_region_workspace(int B, int h, int w, int C, int H, int W);
int nasseg_ce_up_region_fwd(const float* logits, const void* target, int elem_size, const float* weight, int B, int h,
                            int w, int C, int H, int W, int ignore, int with_ce, int select, float t_loss,
                            int64_t min_kept, double keep_fraction, double alpha, double beta, double smooth,
                            int all_classes, double region_weight, float* loss, float* loss_ce, float* loss_region,
                            float* stats, int64_t* counts, float* pixel_loss, float* lse, float* coef, float* sums,
                            int64_t* ncls, float* gdot, float* ws, void* stream);
int nasseg_ce_up_region_bwd(const float* logits, const void* target, int elem_size, const float* weight,
                            const float* pixel_loss, const float* lse, const float* stats, const float* coef,
                            const float* gdot, const float* gscale, int with_ce, double region_weight, int B, int h,
                            int w, int C, int H, int W, int ignore, float* dlogits, void* stream);
int nasseg_ce_up_region_rows_fwd(const float* logits, const void* target, int elem_size, const int64_t* rows,
                                 int64_t n_rows, const float* weight, int B, int h, int w, int C, int H, int W,
                                 int ignore, int with_ce, int select, float t_loss, int64_t min_kept,
                                 double keep_fraction, double alpha, double beta, double smooth, int all_classes,
                                 double region_weight, float* loss, float* loss_ce, float* loss_region, float* stats,
                                 int64_t* counts, float* pixel_loss, float* lse, float* coef, float* sums,
                                 int64_t* ncls, float* gdot, float* ws, void* stream);
int nasseg_ce_up_region_rows_bwd(const float* logits, const void* target, int elem_size, const int64_t* rows,
                                 int64_t n_rows, const float* weight, const float* pixel_loss, const float* lse,
                                 const float* stats, const float* coef, const float* gdot, const float* gscale,
                                 int with_ce, double region_weight, int B, int h, int w, int C, int H, int W,
                                 int ignore, float* dlogits, void* stream);

/* Lovasz-Softmax term (Berman, Triggs, Blaschko, CVPR 2018; absent from the reference): the convex extension of the
 * Jaccard loss, the surrogate of the mean IoU the reward is built from.  Logits [P][C], labels [P]; pixel p is valid
 * iff its label t != ignore and 0 <= t < C; n = valid pixels, y_pc = [t_p == c], N_c = sum_p y_pc.
 * q_p = softmax(x_p) in fp32 exactly as the region term and nasseg_ce_fwd compute it (the same max, the same expf
 * values, the same 1 / s): a function of the pixel's own row alone.
 *   errors  e_pc = fabsf(y_pc - q_pc) in fp32 on valid pixels (written as -1 on the others)
 *   order   per class c: the valid pixels by e_pc DESCENDING on the fp32 values, ties by ASCENDING flat index p - a
 *           total order, so every result is a function of the inputs alone.  Position i = 1 .. n; F_i = foreground
 *           (y = 1) pixels among the first i, B_i = i - F_i.
 *   Lovasz gradient of position i, in double from those integers, U = N_c + B_i:
 *           foreground: g = 1 / U;  background: g = (N_c - F_i) / ((U - 1) U), and g = 1 where U - 1 = 0 (N_c = 0,
 *           i = 1) - that is J_i - J_(i-1) with J_i = 1 - (N_c - F_i) / (N_c + B_i), J_0 = 0
 *   loss_c = sum_i e_(i) g_i in double, per-workgroup partials added in index order (no float atomics)
 *   K = {c : N_c > 0} (all_classes != 0: every class; an absent class then costs max_p q_pc, by the formulas alone)
 *   L = sum_{c in K} loss_c / |K|;  exactly 0 with an exactly zero gradient when n = 0
 * Gradient, the order and the g held constant: G_pc = s_pc g_(c, rank(p)) / |K|, s = -1 on foreground and +1 on
 * background (by label, also at e = 0), G_pc = 0 for c outside K and on invalid pixels;
 *   dL/dx_pj = q_pj (G_pj - sum_c G_pc q_pc) on valid pixels, exact zeros on all others.
 * nasseg_lovasz_coef is the sort-and-scan half over ANY non-negative fp32 error array [P][C] (validity from the
 * labels): loss = L, coef = G [P][C], rank [P][C] = the 0-based position of every valid pixel in its class's order
 * (-1 on invalid pixels and for classes outside K; rank may be null), ncls = {N_c} | |K| (int64 [C + 1]).
 * nasseg_lovasz_fwd makes the errors from the logits, then runs the above;
 *   loss = base_loss[0] + lovasz_weight * L (base_loss null: lovasz_weight * L), loss_lovasz = L (may be null).
 * nasseg_lovasz_bwd: dlogits = gscale * lovasz_weight * q (G - sum_c G_c q_c), q recomputed from the logits
 * (gscale: device scalar, null = 1); accumulate != 0: added onto what dlogits holds - the gradient nasseg_ce_sel_bwd /
 * nasseg_ce_region_bwd has just written there - instead of written (invalid pixels are then left as they are).
 * The order comes from a stable least-significant-digit radix sort on the device (4 passes of 8 bits over the
 * complemented bit pattern, classes as grid rows, ranks from wave ballots - never from the arrival order of
 * atomics), F_i from an integer scan.  The caller owns all memory; no allocation, no host synchronisation, no float
 * atomics, a launch geometry that depends on (P, C) alone: capturable, and bit-reproducible.
 * 2 <= C <= 65535, P * C < 2^31.  ws: nasseg_lovasz_workspace(P, C) 4-byte words, 8-byte aligned (0: bad shape). */
int64_t nasseg_lovasz_workspace(int64_t P, int C);
int nasseg_lovasz_coef(const float* errors, const void* target, int elem_size, int64_t P, int C, int ignore,
                       int all_classes, float* loss, float* coef, int* rank, int64_t* ncls, float* ws, void* stream);
int nasseg_lovasz_fwd(const float* logits, const void* target, int elem_size, int64_t P, int C, int ignore,
                      int all_classes, double lovasz_weight, const float* base_loss, float* loss, float* loss_lovasz,
                      float* errors, float* coef, int* rank, int64_t* ncls, float* ws, void* stream);
int nasseg_lovasz_bwd(const float* logits, const void* target, int elem_size, const float* coef, const float* gscale,
                      double lovasz_weight, int accumulate, int64_t P, int C, int ignore, float* dlogits,
                      void* stream);

/* berHu loss of the depth head (BASELINE config 5; absent from the reference - Laina et al.
 * 2016 eq. 2, "parity unpinned") */
int nasseg_berhu_fwd(const float* pred, const float* target, int64_t n, float* out, float* ws,
                     void* stream);
int nasseg_berhu_bwd(const float* pred, const float* target, const float* stats,
                     const float* gscale, int64_t n, float* dpred, void* stream);

/* masked berHu of the depth head against a FULL-SIZE target with holes (absent from the reference - its depth
 * networks are inference only; "parity unpinned").  pred: dense one-channel map [B][h][w]; target: fp32 [B][H][W]
 * in both builds; prediction pixel (y, x) is compared with target[b][sy][sx], (sy, sx) = the source index of
 * F.interpolate(mode="nearest") - the resized target is never written.  A pixel is valid iff its target t is finite
 * and valid_min < t <= valid_max.  d = |pred - t| over valid pixels, c = 0.2 * max d, loss = sum B(d) / n_valid,
 * B(d) = d if d <= c else (d*d + c*c) / (2c); out = {loss, c, n_valid}; no valid pixel: loss 0, gradient 0.
 * Backward (c constant): dpred = gscale / n_valid * (sign(diff) if d <= c else diff / c), exactly 0 on invalid
 * pixels.  ws: nasseg_berhu_masked_workspace() floats.  No host synchronisation. */
int64_t nasseg_berhu_masked_workspace(void);
int nasseg_berhu_masked_fwd(const float* pred, const float* target, int B, int h, int w, int H, int W,
                            float valid_min, float valid_max, float* out, float* ws, void* stream);
int nasseg_berhu_masked_bwd(const float* pred, const float* target, const float* stats, const float* gscale,
                            int B, int h, int w, int H, int W, float valid_min, float valid_max, float* dpred,
                            void* stream);

/* Full-size berHu: the criterion of nasseg_berhu_masked_fwd taken at the TARGET's size, the bilinear up-sampling of the
 * prediction fused in (absent from the reference, "parity unpinned").  It replaces, for a caller who asks for it, the
 * nearest sampling of the target by nasseg_berhu_masked_fwd - and the composition nasseg_bilinear_fwd +
 * nasseg_berhu_masked_fwd at equal sizes (with nasseg_bilinear_bwd behind it), which writes and re-reads a [B][H][W]
 * map in each direction: the loss is then taken where validate_depth (nasseg_depth_metrics) scores, on the prediction
 * resized to the ground truth.
 * pred [B][h][w] (one channel, fp32 or bf16 storage), target fp32 [B][H][W] at ANY size, larger than, equal to or
 * smaller than (h, w), per axis.  For target pixel P = (b, Y, X): P is valid iff target[P] is finite and
 * valid_min < target[P] <= valid_max; ly = lin_coeff(Y, h/H, h, H), lx = lin_coeff(X, w/W, w, W) (bilinear,
 * align_corners = False, torch's source index in fp32) and
 *   top = l0x x00 + l1x x01,  bot = l0x x10 + l1x x11,  v(P) = l0y top + l1y bot
 * with every product and every sum rounded to fp32 on its own - bit for bit the value nasseg_depth_metrics scores
 * (before its clamp); equal sizes are the identity.  d(P) = |v(P) - target[P]|, c = 0.2 * max d over the valid pixels,
 * loss = sum B(d) / n_valid, B(d) = d if d <= c else (d*d + c*c) / (2c); out = {loss, c, n_valid}; no valid pixel:
 * loss 0, gradient 0.  Sums over pixels: per-workgroup partials added in fp64 in a fixed order by one finalize launch.
 * Backward (c constant): with r(P) = sign(v - t) if d <= c else (v - t) / c on valid pixels,
 *   dpred[b][y][x] = gscale / n_valid * sum_P r(P) Wy(P, y) Wx(P, x),   Wy(P, y) = l0y [i0(Y) == y] + l1y [i1(Y) == y]
 * (Wx alike), a gather in fp32 over the target range that can reach (y, x): a group of `group` lanes shares the range of
 * one prediction pixel in a fixed interleaving and adds its partial sums in a fixed tree.  group = 0: chosen from
 * (h, w, H, W) alone - the smallest of 1, 4, 16, 64, 256 that leaves a lane at most 16 of the (2H/h) x (2W/w) targets;
 * 1, 4, 16, 64 or 256: that group (every value is correct at every shape; they differ in speed and in the order of the
 * sum).  A prediction pixel whose range holds no valid target gets an exact zero; dpred is stored in the prediction's
 * type, written once.  No float atomics, no host synchronisation, no allocation, a launch geometry that depends on
 * the shapes alone: capturable and bit-reproducible.
 * B*H*W < 2^32, B*h*w < 2^31.  ws: nasseg_berhu_up_workspace floats (0: bad shape) - a function of the grid alone,
 * not of the pixel count. */
int64_t nasseg_berhu_up_workspace(int B, int h, int w, int H, int W);
int nasseg_berhu_up_fwd(const float* pred, const float* target, int B, int h, int w, int H, int W, float valid_min,
                        float valid_max, float* out, float* ws, void* stream);
int nasseg_berhu_up_bwd(const float* pred, const float* target, const float* stats, const float* gscale, int B, int h,
                        int w, int H, int W, float valid_min, float valid_max, int group, float* dpred, void* stream);

/* Row-indexed twins of the four entry points above, for targets that live in a cache (the task0 depth cache,
 * engine/trainer.py: populate_task0(task="depth")): target is the WHOLE cache, fp32 [n_rows][H][W], and rows a DEVICE
 * array of B cache rows - the index nasseg_gather_rows takes; image b of the prediction is compared with
 * target[clamp(rows[b], 0, n_rows - 1)] (the clamp is a memory-safety net only: the host checks the range).  Repeated
 * and unordered rows are legal.  Everything else - validity, c, out = {loss, c, n_valid}, the backward with c constant,
 * group, the workspaces nasseg_berhu_masked_workspace() / nasseg_berhu_up_workspace(B, h, w, H, W) - is as above, and
 * so is every bit: the result is that of the un-indexed entry point on a gathered copy target[rows] (the same kernels,
 * launch geometry, order of sums and finalize; only the address of an image's target differs), which is never
 * written.  B*H*W < 2^32 and B*h*w < 2^31 bound the BATCH; the cache may be larger (rows[b]*H*W is 64-bit).  Neither
 * the cache nor the table is written. */
int nasseg_berhu_masked_rows_fwd(const float* pred, const float* target, const int64_t* rows, int64_t n_rows, int B,
                                 int h, int w, int H, int W, float valid_min, float valid_max, float* out, float* ws,
                                 void* stream);
int nasseg_berhu_masked_rows_bwd(const float* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                 const float* stats, const float* gscale, int B, int h, int w, int H, int W,
                                 float valid_min, float valid_max, float* dpred, void* stream);
int nasseg_berhu_up_rows_fwd(const float* pred, const float* target, const int64_t* rows, int64_t n_rows, int B, int h,
                             int w, int H, int W, float valid_min, float valid_max, float* out, float* ws,
                             void* stream);
int nasseg_berhu_up_rows_bwd(const float* pred, const float* target, const int64_t* rows, int64_t n_rows,
                             const float* stats, const float* gscale, int B, int h, int w, int H, int W,
                             float valid_min, float valid_max, int group, float* dpred, void* stream);

/* Depth terms: the scale-invariant log term (Eigen et al. 2014, eq. 4, without a square root) and the multi-scale
 * gradient-matching term (MegaDepth, Li & Snavely 2018; MiDaS, Ranftl et al. 2020) on top of the masked berHu - the
 * surrogates of what validate_depth (nasseg_depth_metrics) scores, which are all functions of ln p - ln g (absent from
 * the reference, "parity unpinned").  At the PREDICTION's size only.
 * pred [B][h][w] (one channel, fp32 or bf16 storage), target fp32 [B][H][W] at any size.  Sampling and validity are
 * exactly nasseg_berhu_masked_fwd's: prediction pixel i = (b, y, x) meets t_i = target[b][nearest_src(y)][nearest_src(x)]
 * and is valid iff t_i is finite and valid_min < t_i <= valid_max; V = the valid pixels, n = |V|.  valid_min >= 0 and
 * pred_min > 0 are required (every logarithm is defined).
 *   residual   r_i = logf(max(p_i, pred_min)) - logf(t_i) on V, fp32, each logf on its own; written to resid, fp32
 *              [B][h][w] - the only per-pixel tensor the forward writes; an invalid pixel carries a NaN.
 *   D          = mean_V(r^2) - silog_lambda * mean_V(r)^2, 0 <= silog_lambda <= 1.  The silog score is sqrt(D) at
 *              silog_lambda = 1; the root is left out so that the gradient stays finite at a perfect prediction.
 *   L_gm       = sum_{k < scales} S_k / M_k, s = 2^k; G_k = the pixels with y % s == 0 and x % s == 0 within each image,
 *              M_k = the valid pixels of G_k over the batch,
 *              S_k = sum_{i in G_k} ( [i, i+(0,s) valid] |r_{i+(0,s)} - r_i| + [i, i+(s,0) valid] |r_{i+(s,0)} - r_i| ),
 *              a neighbour counting only inside the same image; M_k == 0: the scale contributes 0.  0 <= scales <= 8
 *              (0: no such term, L_gm = 0, the stencil pass is not launched).
 *   total      = berhu_weight * berhu[0] + silog_weight * D + grad_weight * L_gm, berhu = out of nasseg_berhu_masked_fwd
 *              on the same arguments (null: taken as 0).  n == 0: D = L_gm = 0, gradient 0.
 * out (16 floats) = total | D | L_gm | n | m = mean_V(r) | M_0..M_7 | 3 unused.  Pass 1 writes resid and the workgroup
 * sums of r, r^2 and the count; pass 2 is one stencil sweep over resid for all scales; one finalize launch adds the
 * workgroup partials in fp64 in a fixed order.  ws: nasseg_depth_terms_workspace() floats.
 * Backward (m and the M_k are functions of the mask; c of the berHu constant): resid, terms = resid, out of the forward,
 * gscale = the device scalar upstream gradient of the total (null = 1); the three weights are arguments by value.
 * ONE kernel writes dpred once, in the prediction's type (bf16 storage: one rounding of the sum of all three terms):
 *   dpred_i = gscale * [ berhu_weight * (berHu's gradient, as nasseg_berhu_masked_bwd)
 *             + [p_i > pred_min] / p_i * ( silog_weight * (2/n)(r_i - silog_lambda m)
 *               + grad_weight * sum_k [i in G_k] / M_k * sum_{j in {i+-(0,s), i+-(s,0)}, j valid, in the image} sign(r_i - r_j) ) ]
 * on valid pixels, exactly 0 on invalid ones; sign(0) = 0.  A pixel with p_i <= pred_min gets no gradient from the two
 * terms - the berHu, which they sit on top of, still pulls it up.
 * No float atomics, no host synchronisation, no allocation, a launch geometry that depends on the shapes (and scales)
 * alone: capturable and bit-reproducible.  n and the M_k reach the backward as fp32 (out[3], out[5 + k]), as n_valid of
 * nasseg_berhu_masked_fwd does (its out[2]): above 2^24 valid pixels a count is rounded, and 2/n and 1/M_k with it.
 * _rows_: target is the cache [n_rows][H][W] read in place through the B cache
 * rows, as nasseg_berhu_masked_rows_fwd - bit for bit the un-indexed call on target[rows]. */
int64_t nasseg_depth_terms_workspace(void);
int nasseg_depth_terms_fwd(const float* pred, const float* target, int B, int h, int w, int H, int W, float valid_min,
                           float valid_max, float pred_min, float silog_lambda, int scales, const float* berhu,
                           float berhu_weight, float silog_weight, float grad_weight, float* resid, float* out,
                           float* ws, void* stream);
int nasseg_depth_terms_bwd(const float* pred, const float* target, const float* resid, const float* berhu,
                           const float* terms, const float* gscale, int B, int h, int w, int H, int W,
                           float valid_min, float valid_max, float pred_min, float silog_lambda, int scales,
                           float berhu_weight, float silog_weight, float grad_weight, float* dpred, void* stream);
int nasseg_depth_terms_rows_fwd(const float* pred, const float* target, const int64_t* rows, int64_t n_rows, int B,
                                int h, int w, int H, int W, float valid_min, float valid_max, float pred_min,
                                float silog_lambda, int scales, const float* berhu, float berhu_weight,
                                float silog_weight, float grad_weight, float* resid, float* out, float* ws,
                                void* stream);
int nasseg_depth_terms_rows_bwd(const float* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                const float* resid, const float* berhu, const float* terms, const float* gscale,
                                int B, int h, int w, int H, int W, float valid_min, float valid_max, float pred_min,
                                float silog_lambda, int scales, float berhu_weight, float silog_weight,
                                float grad_weight, float* dpred, void* stream);

/* ---- mean-IoU reward: helpers/miou_utils.pyx fast_cm :7-30, compute_iu :32-57,
 * compute_ius_accs :59-90; argmax + up-sampling of engine/inference.py:58-66 ------ */
int nasseg_fast_cm(const uint8_t* preds, const uint8_t* gt, int64_t P, int n, int64_t* cm,
                   void* stream);
int nasseg_argmax_cm(const float* logits, const uint8_t* gt, uint8_t* preds, int B, int h, int w,
                     int C, int H, int W, int n, int64_t* cm, void* stream);
/* host-side (cm, iu, n_pixels, accs are HOST pointers) */
int nasseg_compute_ius_accs(const int64_t* cm, int n, double* iu, int64_t* n_pixels, double* accs);

/* ---- depth metrics: the depth counterpart of nasseg_argmax_cm (absent from the reference, "parity unpinned").
 * Channel 0 of the NHWC prediction [B][h][w] (pixel stride ldp elements) is up-sampled bilinearly
 * (align_corners=False, fp32) to the ground truth's (H, W); pixels whose gt is finite and in
 * (min_depth, max_depth] are kept, the prediction is clamped to [min_depth, max_depth] (min_depth > 0 required);
 * from the fp32 p and g, in double, acc[0..10] += n, sum|p-g|, sum(p-g)^2, sum|p-g|/g, sum(p-g)^2/g,
 * sum|log10 p - log10 g|, sum(ln p - ln g), sum(ln p - ln g)^2, #{max(p/g, g/p) < 1.25, 1.25^2, 1.25^3};
 * acc[11] is reserved and left untouched.  acc: 12 doubles on the device, ACCUMULATED into; ws:
 * nasseg_depth_metrics_workspace(B, H, W) doubles.  Fixed-order sums: the same inputs give the same bits. */
int64_t nasseg_depth_metrics_workspace(int B, int H, int W);
int nasseg_depth_metrics(const float* pred, int64_t ldp, int B, int h, int w, const float* gt, int H, int W,
                         float min_depth, float max_depth, double* acc, double* ws, void* stream);


/* ---- clip_grad_norm_ + optimiser steps: src/engine/trainer.py:163-166,258-268 on the torch.optim.SGD /
 * torch.optim.Adam objects of src/utils/solvers.py:6-52 - two launches for every parameter of the step.
 *   tensors  DEVICE int64 [n_tensors][8]: parameter, gradient, state 1 (SGD momentum_buffer | Adam exp_avg; 0: SGD
 *            without momentum), state 2 (Adam exp_avg_sq; else 0) addresses, numel, clip set (-1: none), hyper
 *            group, flags (bit 0: all four addresses are 16-byte aligned).  fp32, dense, gradient laid out like
 *            the parameter.
 *   chunks   DEVICE int32 [n_chunks][2] = {tensor, first element}: nasseg_optim_chunk() elements each; the chunks of
 *            one clip set are consecutive.
 *   hyper    HOST double [n_hyper][6] = {kind (0 SGD, 1 Adam), lr, weight_decay, momentum | beta1, beta2, eps};
 *            SGD: no nesterov, no dampening; Adam: no amsgrad; neither maximises.  n_hyper <= 8.
 *   clips    HOST double [n_clip][3] = {max_norm, first chunk, chunk count}, n_clip <= 8: L2 norm over the set,
 *            gradients scaled in place by min(1, max_norm / (norm + 1e-6)); norms[n_clip] receives the norms.
 *   dstep    DEVICE float [n_tensors]: steps taken per tensor, advanced by the call (Adam's bias correction reads
 *            it on the device: the call can be replayed from a hipGraph).
 *   partial  DEVICE double [n_chunks] workspace. */
int64_t nasseg_optim_chunk(void);
int nasseg_optim_step(const int64_t* tensors, int n_tensors, const int* chunks, int n_chunks, const double* hyper,
                      int n_hyper, const double* clips, int n_clip, float* dstep, double* partial, float* norms,
                      void* stream);
/* ---- Polyak averaging: src/engine/trainer.py:167-169,270-272 (avg_p.mul_(d).add_(1 - d, p) for every parameter
 * after every step) - one launch for all of them.
 *   tensors  DEVICE int64 [n_tensors][4]: parameter (read) and average (written) addresses, numel, flags (bit 0: both
 *            addresses are 16-byte aligned).  fp32, dense, average laid out like the parameter.  The kernel writes
 *            through this table: a caller recording the call must name the averages it writes (graph_dag).
 *   chunks   DEVICE int32 [n_chunks][2] = {tensor, first element}: nasseg_optim_chunk() elements each.
 *   decay, alpha: (float)d and (float)(1 - d), 1 - d computed in double - the scalars ATen receives.
 * Rounded as avg.mul_(decay).add_(param, alpha=alpha) is on this platform: fmaf(alpha, p, avg * decay). */
int nasseg_polyak(const int64_t* tensors, int n_tensors, const int* chunks, int n_chunks, float decay, float alpha,
                  void* stream);

/* ---- the search controller: src/rl/micro_controllers.py (MicroController.forward :148-265, TemplateController.forward
 * :442-571, evaluate_actions :267-274 / :573-580), sampling and log-probabilities of src/rl/utils.py:7-27, the PPO
 * surrogate of src/rl/gradient_estimators.py:170-187 (REINFORCE :42-57 needs the rollout and its backward only).
 * In both controllers the LSTM's next input is its own previous output and enc_op is never read, so every step's
 * distribution is independent of the actions: B action rows are ONE T-step rollout plus B T gathers, n samples one
 * rollout plus n T inverse-CDF look-ups.  fp32 only; the dependent chain runs in one workgroup; no atomics: results
 * repeat bit for bit, host-launched or replayed from a hipGraph.
 *   params   DEVICE int64 [1 + 4L + 2 n_heads] addresses, torch's own layouts (nothing is re-packed): g_emb (H);
 *            per LSTM layer k weight_ih_l{k} (4H, H), weight_hh_l{k} (4H, H), bias_ih_l{k}, bias_hh_l{k} (4H), gates
 *            i, f, g, o; per head its Linear's weight (n, H) and bias (n).
 *   steps    DEVICE int32 [T][3] = {head (-1: a warm-up step, the enc_num_layers loop), choices n, position of the
 *            step's action in an action row (-1: none)}; the kernels clamp n to max_choices and ignore heads >=
 *            n_heads and positions >= A.
 *   actions  DEVICE int32 [n_rows][A]; rows DEVICE int32 [B] picks the B rows to evaluate (null: rows 0..B-1); row
 *            indices and actions are clamped into range.  B = 0: no log-probabilities.
 *   u        DEVICE fp32 [n_samples][T] uniforms in [0, 1) (null with n_samples = 0): sampled int32 [n_samples][A]
 *            receives, at every step's position, the first index i with u < p_0 + .. + p_i (the CDF accumulated in
 *            ascending order, the last index catches the rest); positions without a step are set to 0.  sampled_lp
 *            [n_samples]: their log-probabilities, the sums nasseg_ctrl_rollout's log_prob gives for those rows.
 *   saved    DEVICE fp32 [nasseg_ctrl_saved_floats(T, H, L)], written for nasseg_ctrl_backward: activated gates, cell
 *            states, layer outputs, per-step probabilities / log-probabilities / centred logits.
 *   entropy  DEVICE fp32 [1] = sum_t -sum_i p log p (a head with one choice adds 0); log_prob [B] = sum_t
 *            log p_t[a[b, t]], t ascending.
 * Limits (refused with NASSEG_ERR_ARG): H <= 256, L <= 4, T <= 128, max_choices <= 64, n_heads <= 64, B <= 1024,
 * n_samples <= 1024.
 * nasseg_ctrl_backward: from d_log_prob [B] (null: zeros) and d_entropy [1] (null: zero),
 *   dlogits_t = sum_b d_log_prob[b] (onehot(a[b, t]) - p_t) + d_entropy (-p_t (log p_t + H_t)), b ascending,
 * (log p_t + H_t taken as the logits centred on their mean under p_t, which the rollout saved: no cancellation),
 * back through the heads, the layers and time (layer 0's input at t + 1 is the top layer's output at t) in one
 * workgroup, then the parameter gradients in a second launch, one thread per element, t ascending: grads + gtab[e][0]
 * receives entry e's gradient, laid out like the parameter; gtab DEVICE int32 [1 + 4L + 2 n_heads][2] = {offset in
 * floats, rows (heads: n)}.  bias_ih and bias_hh receive the same sums; g_emb layer 0's input gradient at t = 0.
 * work: DEVICE fp32 [nasseg_ctrl_work_floats(T, H, L)].
 * nasseg_ctrl_ppo_seed: log_prob [B] against old_log_prob / adv [n_rows] at rows[B] (null: 0..B-1).  As the reference
 * subtracts a (B, 1) array from a (B,) tensor, ratio_ij = exp(log_prob[j] - old[i]) over B x B pairs (B = 1, the
 * search's setting: the usual formula): action_loss = -mean_ij min(ratio_ij adv_i, clamp(ratio_ij, clip_lo, clip_hi)
 * adv_i); acc[0] += action_loss, acc[1] += entropy[0]; d_log_prob [B] and d_entropy [1] = -entropy_coef are the
 * gradients of action_loss - entropy_coef entropy (min and clamp pass gradients as torch's do: a tie splits, the
 * clamp's bounds are inside). */
int64_t nasseg_ctrl_saved_floats(int T, int H, int L);
int64_t nasseg_ctrl_work_floats(int T, int H, int L);
int nasseg_ctrl_rollout(const int64_t* params, const int* steps, int T, int H, int L, int n_heads, int max_choices,
                        const int* actions, const int* rows, int n_rows, int B, int A, const float* u, int n_samples,
                        int* sampled, float* sampled_lp, float* saved, float* entropy, float* log_prob,
                        void* stream);
int nasseg_ctrl_backward(const int64_t* params, const int* steps, int T, int H, int L, int n_heads, int max_choices,
                         const int* actions, const int* rows, int n_rows, int B, int A, const float* d_log_prob,
                         const float* d_entropy, const float* saved, float* work, const int* gtab, float* grads,
                         void* stream);
int nasseg_ctrl_ppo_seed(const float* log_prob, const float* entropy, const float* old_log_prob, const float* adv,
                         const int* rows, int n_rows, int B, float clip_lo, float clip_hi, float entropy_coef,
                         float* acc, float* d_log_prob, float* d_entropy, void* stream);

/* ---- hipGraph scheduling of a captured step (reference src/nn/micro_decoders.py:54-139: the five
 * ops of a ContextualCell read one input, the two cells of a MergeCell share nothing) ---------------------------------
 * A step recorded from one stream is a line of nodes.  The host side (engine/graph_dag.py) knows from this header
 * which pointers every entry point reads (const) and writes (non-const) and with which address ranges it was called;
 * these host-only calls let it attribute the recorded nodes to calls and replace the line's edges by the real
 * dependencies (kept in a few lanes), so that independent branches replay side by side.
 *   nasseg_graph_capture_nodes: nodes recorded so far by the capture `stream` belongs to; -1: not capturing.
 *   nasseg_graph_node_kinds:    kinds[i] of the i-th recorded node: 0 kernel, 1 memcpy, 2 memset, 3 other.
 *   nasseg_graph_rewire:        graph = hipGraph_t recorded from ONE stream with n_nodes nodes; its edges are replaced
 *                               by edges[2*e] -> edges[2*e+1] (indices in recording order, pointing forward).  The
 *                               caller guarantees they cover every read/write hazard of the recorded launches. */
int nasseg_graph_capture_nodes(void* stream);
int nasseg_graph_node_kinds(void* graph, int n_nodes, int* kinds);
int nasseg_graph_rewire(void* graph, int n_nodes, int n_edges, const int* edges);
/* Stages and lanes.  A dependency between two branches INSIDE one hipGraph costs this runtime about as much as a small
 * kernel, and a graph with branches is no longer replayed from pre-built packets; so the host side cuts the recorded
 * line into STAGES whose LANES share nothing, every (stage, lane) a line graph of its own, and orders them with events:
 *   nasseg_graph_split:  part[i] = the part of the i-th recorded node (kernel and memset nodes only, else
 *                        NASSEG_ERR_UNSUPPORTED); execs[p] receives a hipGraphExec_t holding part p's nodes in
 *                        recording order (0: empty part).  The recorded graph is not modified.
 *   nasseg_graph_run:    one replay - ops[3*i..] = {kind, a, b}: 0 launch executable graph a on stream b, 1 record
 *                        event a on stream b, 2 stream b waits for event a; b == 0 means `stream`.  Asynchronous.
 *   nasseg_lane_*:       the non-blocking streams / timing-free events those ops name (handles as void*). */
int nasseg_graph_split(void* graph, int n_nodes, const int* part, int n_parts, void** execs);
int nasseg_graph_exec_destroy(void* exec);
int nasseg_lane_stream_create(void** stream);
int nasseg_lane_event_create(void** event);
int nasseg_lane_destroy(void* stream, void* event);
int nasseg_graph_run(int n_ops, const int64_t* ops, void* stream);

/* ---- sample augmentation: the training / validation pipelines of data/datasets.py (data/device.py) ------
 * One launch per batch of B samples, every output Ho x Wo.  src: packed uint8 source windows (HxWx3 images,
 * HxW masks) of src_bytes bytes; desc int64 [B][8] = {image offset, mask offset, window height, window width,
 * image row stride, mask row stride (bytes), image fill (3 bytes, channel 0 lowest), mask fill}; taps int32
 * [B][9 (Ho + Wo)] = rows [Ho][4 indices, 4 coefficients], columns [Wo][4, 4] (OpenCV's 11-bit INTER_CUBIC
 * coefficients; index -1: a fill pixel), mask rows [Ho], mask columns [Wo] (nearest index, -1: fill), indices
 * into the window; lut [3][256]: output value of channel c for the uint8 result v.  Writes image [B][Ho][Wo][3]
 * (NHWC) and mask uint8 [B][Ho][Wo] (mask null: no mask is written).  A window - image, mask or counts, of e bytes
 * per element - lies inside src when h > 0, w > 0, 0 <= offset <= src_bytes, e w <= stride <= src_bytes and offset +
 * (h - 1) stride + e w <= src_bytes, so a single-row window whose stride exceeds src_bytes is read as fill too. */
int nasseg_augment(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps, const float* lut,
                   float* image, uint8_t* mask, int B, int Ho, int Wo, void* stream);
/* The same launch for a metric depth target instead of a label map (data/device.py: run_depth_batch).  The image
 * half - src, desc, taps, lut, image - is nasseg_augment's, bit for bit.  The "mask" windows of src hold LITTLE-ENDIAN
 * 16-BIT COUNTS: h rows of w counts, the mask row stride of desc in BYTES and at least 2 w; desc's mask fill is not
 * read.  params fp32 [B][2] = {zoom, fill} per sample; depth_scale: metres per count, one value per launch.  Writes
 * target fp32 [B][Ho][Wo] whatever the image's storage type:
 *   both nearest indices >= 0:  target = fdiv_rn(fmul_rn((float)count, depth_scale), zoom[b]) - two correctly rounded
 *                               fp32 operations, no contraction, no reciprocal: numpy's float32 product and quotient
 *                               (data/datasets.py: _load_depth, DepthResizeScale), bit for bit; zoom 1.0 is exact;
 *   a fill pixel (an index -1, or a window that does not lie inside src):  target = fill[b], written as it is and NOT
 *                               divided (host pipelines pad after the resize).
 * Every load stays inside src whatever desc holds.  A packed target window may start at an odd byte (after an image
 * of odd 3 h w bytes): the kernel reads a count as two byte loads, so offsets and strides need no alignment and no
 * 16-bit load of a count is ever issued.  One thread per output pixel, blockIdx.y = sample, 256 threads. */
int nasseg_augment_depth(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                         const float* lut, const float* params, float depth_scale, float* image, float* target,
                         int B, int Ho, int Wo, void* stream);
/* The two launches above with a photometric jitter between the resampling and lut (data/datasets.py: ColourJitter;
 * data/device.py plans it).  Everything else - arguments, grid, the mask / target half, fills - is the sibling's.
 * colour int32 [B][12] = {q[0][0..2], q[1][0..2], q[2][0..2], apply, 0, 0}: the sample's colour matrix in 12-bit fixed
 * point (4096 = 1.0) and whether to apply it; ctab uint8 [B][3][256], 4-byte aligned: the sample's point table per
 * channel.  A live pixel's resampled uint8 triple v becomes
 *   m[c] = apply ? clip((q[c][0] v[0] + q[c][1] v[1] + q[c][2] v[2] + 2048) >> 12, 0, 255) : v[c]   (arithmetic shift)
 *   image value of channel c = lut[c][ctab[b][c][m[c]]].
 * A fill pixel (an index -1, or a window that does not lie inside src) is lut[c][fill byte c]: neither the matrix nor
 * ctab touches it - the host passes the fill its pipeline ends with.  The sum is int32 with every coefficient clamped
 * to |q| <= 2^15 as it is read (|sum| < 2^25; data/device.py refuses larger coefficients, ColourJitter's stay below
 * 2^14.1), and every table index is a value clipped to 0..255: all loads stay in bounds whatever colour and ctab hold.
 * With apply = 0 and ctab the identity ramp the image is the sibling's, bit for bit.  Both tables sit in LDS; the 12
 * words are uniform per workgroup. */
int nasseg_augment_colour(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                          const int32_t* colour, const uint8_t* ctab, const float* lut, float* image, uint8_t* mask,
                          int B, int Ho, int Wo, void* stream);
int nasseg_augment_depth_colour(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                                const int32_t* colour, const uint8_t* ctab, const float* lut, const float* params,
                                float depth_scale, float* image, float* target, int B, int Ho, int Wo, void* stream);

/* ---- prediction post-processing: cv2.resize(logits, dsize, interpolation=INTER_CUBIC) (float branch) of the
 * reference's inference notebooks, then argmax for segmentation (engine/predict.py) ------------------------------
 * x: NHWC [B][h][w][C], any C >= 1.  taps int32 / coef float32 [4 (H + W)]: per output row, then per output
 * column, the four clipped source indices and the four Keys weights (A = -0.75) of data/datasets._cubic_taps(n_src,
 * n_dst, n_dst / n_src).  Horizontal pass over the four source rows, then vertical, each summed in tap order from
 * zero without FMA contraction: bit-identical to that host restatement (datasets.resize_cubic_to).
 *   nasseg_resize_cubic:        y fp32 NHWC [B][H][W][C];
 *   nasseg_resize_cubic_argmax: labels uint8 [B][H][W] = argmax over C of the resized values (not stored), lowest
 *                               index wins ties; C <= 256. */
int nasseg_resize_cubic(const float* x, int B, int h, int w, int C, const int* taps, const float* coef, float* y,
                        int H, int W, void* stream);
int nasseg_resize_cubic_argmax(const float* x, int B, int h, int w, int C, const int* taps, const float* coef,
                               uint8_t* labels, int H, int W, void* stream);
/* Test-time ensemble over scales and mirroring: what a user of the notebooks' pipeline (examples/inference/) or of
 * validate() (src/engine/inference.py:58-66) does by hand on the host - run the network on resized and mirrored
 * images, bring every result back to the image's size, soft-max, average, argmax - without a full-resolution
 * tensor per view.
 *   nasseg_view_image: x NHWC [B][Hi][Wi][C] (any C >= 1) -> y [B][Ho][Wo][C], resized bilinearly with
 *     align_corners=False (the arithmetic of nasseg_bilinear_fwd) and, mirror != 0, with its columns reversed.
 *   nasseg_fuse_views: n_views <= 16 logit maps views[v] (HOST array of device addresses), NHWC [B][h_v][w_v][C];
 *     dims (HOST) [n_views][3] = {h_v, w_v, offset of the view's block in taps / coef}.  The arrays are copied into
 *     the kernel's arguments: a recorded call reads no device-side table of them.  taps int32 / coef float32
 *     (device): per view a block of n_taps (H + W) entries, n_taps = 4 (the cubic tables above) or 2 (bilinear,
 *     align_corners=False) - per output row, then per output column, n_taps source indices and weights; a mirrored
 *     view is un-mirrored by its column indices (t -> w_v - 1 - t), the kernel has no mirror logic.  Per output
 *     pixel and view: r_v[c] = the horizontal pass over the n_taps source rows, then the vertical pass, each summed
 *     in tap order from zero without FMA contraction (n_taps = 4, un-mirrored: nasseg_resize_cubic bit for bit);
 *     p_v = softmax_c(r_v) in fp32 with the maximum subtracted; P = sum_v p_v in view order.  Outputs, each may be
 *     null: labels uint8 [B][H][W] = argmax_c P (lowest index wins ties, so does the first NaN); probs fp32 NHWC
 *     [B][H][W][C] = P / n_views; cm int64 [n][n] += the histogram of (gt, label) over pixels with gt < n, as
 *     nasseg_argmax_cm (gt uint8 [B][H][W]; integer atomics: exact and reproducible); mean fp32 NHWC [B][H][W][C]
 *     = (sum_v r_v) / n_views, no softmax (depth).  labels / probs / cm need C <= 64; n <= 256. */
int nasseg_view_image(const float* x, float* y, int B, int Hi, int Wi, int C, int Ho, int Wo, int mirror,
                      void* stream);
int nasseg_fuse_views(int n_views, const float* const* views, const int* dims, const int* taps, const float* coef,
                      int n_taps, int B, int C, int H, int W, const uint8_t* gt, int n, uint8_t* labels, float* probs,
                      int64_t* cm, float* mean, void* stream);

/* ---- bfloat16 activation storage --------------------------------------------
 * Every entry point above that reads or writes ACTIVATIONS (feature maps and their gradients)
 * has a twin nasseg_bf16_<op> with the same arguments in which those tensors are stored as
 * bfloat16 (BASELINE config 5).  Only storage changes: values are widened to fp32 on load and
 * rounded to nearest-even on store; arithmetic, MFMA accumulation, BatchNorm statistics,
 * parameters, parameter gradients, workspaces and every per-channel vector stay fp32, and the
 * size / workspace queries are shared with the fp32 entry points.
 * nasseg_bf16_t is one stored value: the upper 16 bits of the IEEE-754 binary32 it stands for, in a struct
 * with the size and alignment of uint16_t (2 bytes, no padding), so that an array of them is an array of
 * uint16_t in memory and a stored value is never taken for a number by accident. */
typedef struct nasseg_bf16_t {
  uint16_t v;
} nasseg_bf16_t;
/* fp32 -> bf16 (round to nearest even) / bf16 -> fp32 of n values: the (B, C, 1, 1) maps on either side of
 * GAPConv1x1's fp32 island (layer_factory.py:181-195) in a bf16-storage network */
int nasseg_to_bf16(const float* x, nasseg_bf16_t* y, int64_t n, void* stream);
int nasseg_from_bf16(const nasseg_bf16_t* x, float* y, int64_t n, void* stream);
int nasseg_bf16_irdw_stats(const nasseg_bf16_t* x, const float* w1, const float* in_scale, const float* in_shift,
                           int in_act, int B, int H, int W, int K, int C, float eps, float momentum, const float* gamma,
                           const float* beta, float* mean, float* invstd, float* scale, float* shift,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, float* ws,
                           void* stream);
int nasseg_bf16_irdw_fwd(const nasseg_bf16_t* x, const float* w1, const float* wdw, nasseg_bf16_t* z2,
                         const float* in_scale, const float* in_shift, int in_act, const float* bn1_scale,
                         const float* bn1_shift, int act1, int B, int H, int W, int K, int C, int Ho, int Wo, int stride,
                         float* stats, void* stream);
int nasseg_bf16_irdw_bwd(const nasseg_bf16_t* x, const float* w1, const nasseg_bf16_t* g, const nasseg_bf16_t* z2,
                         const float* wdw, int wdw_flipped, nasseg_bf16_t* ge, float* dw, float* ws,
                         const float* in_scale, const float* in_shift, int in_act, const float* bn1_scale,
                         const float* bn1_shift, const float* bn1_mean, const float* bn1_invstd, int act1,
                         const float* bn2_scale, const float* bn2_shift, const float* bn2_mean,
                         const float* bn2_invstd, const float* bn2_sums, int bn2_train, int bn2_act, int B, int H, int W,
                         int K, int C, int Ho, int Wo, int stride, float* stats, void* stream);
int nasseg_bf16_dwconv_bwd_bn(const nasseg_bf16_t* xz, const nasseg_bf16_t* g, const nasseg_bf16_t* z, const float* wt,
                              int wt_flipped, nasseg_bf16_t* ge, float* dw, float* ws, const float* in_scale, const float* in_shift,
                              const float* in_mean, const float* in_invstd, int in_act, const float* bn_scale,
                              const float* bn_shift, const float* bn_mean, const float* bn_invstd, const float* bn_sums,
                              int bn_train, int bn_act, int B, int H, int W, int C, int Ho, int Wo, int K, int stride,
                              int pad, int dil, float* stats, void* stream);
int nasseg_bf16_conv_pw_bwd_bn(const nasseg_bf16_t* x, const nasseg_bf16_t* g, const nasseg_bf16_t* z, const float* wb,
                               nasseg_bf16_t* dx, float* dw, float* ws, const float* in_scale, const float* in_shift,
                               int in_act, int dx_act, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                               const float* bn_invstd, const float* bn_sums, int bn_train, int bn_act, int B, int H,
                               int W, int K, int N, const float* in_mean, const float* in_invstd, float* dx_stats,
                               const nasseg_bf16_t* dx_res, void* stream);
int nasseg_bf16_sepconv_fwd(const nasseg_bf16_t* x, const float* wdw, const float* wpw, nasseg_bf16_t* zdw,
                            nasseg_bf16_t* y, const float* in_scale, const float* in_shift, int in_act,
                            const float* out_scale, const float* out_shift, int out_act, int B, int H, int W, int C,
                            int Ho, int Wo, int N, int K, int stride, int pad, int dil, float* stats, void* stream);
int nasseg_bf16_affine_act(const nasseg_bf16_t* x, const float* scale, const float* shift, const nasseg_bf16_t* res,
                      nasseg_bf16_t* y, int64_t n, int C, int act, void* stream);
int nasseg_bf16_psum_bwd(const nasseg_bf16_t* dy, const nasseg_bf16_t* za, const float* tsa, int act_a, const float* ca,
                         nasseg_bf16_t* ga, float* part_a, const nasseg_bf16_t* zb, const float* tsb, int act_b,
                         const float* cb, nasseg_bf16_t* gb, float* part_b, float* cpart, int B, int H, int W, int C,
                         void* stream);
int nasseg_bf16_add_act2(const nasseg_bf16_t* xa, const float* sa, const float* ha, int act_a, const float* ca,
                         const nasseg_bf16_t* xb, const float* sb, const float* hb, int act_b, const float* cb,
                         nasseg_bf16_t* y, int64_t n, int C, void* stream);
int nasseg_bf16_bn_bwd_apply(const nasseg_bf16_t* dy, const nasseg_bf16_t* x, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* sums, int64_t M,
                        int C, int train, int act, nasseg_bf16_t* dx, void* stream);
int nasseg_bf16_bn_bwd_reduce_rows(const nasseg_bf16_t* dy, int64_t lddy, const nasseg_bf16_t* x, int64_t ldx, int64_t M,
                                   int C, const float* scale, const float* shift, const float* mean, const float* invstd,
                                   int act, float* rows, void* stream);
int nasseg_bf16_bn_bwd_apply_rows(const nasseg_bf16_t* dy, const nasseg_bf16_t* x, const float* scale, const float* shift,
                                  const float* mean, const float* invstd, const float* rows, int nrows, float* sums_out,
                                  int64_t M, int C, int train, int act, nasseg_bf16_t* dx, void* stream);
int nasseg_bf16_grad_junction(const nasseg_bf16_t* g0, const nasseg_bf16_t* g1, const nasseg_bf16_t* g2,
                              const nasseg_bf16_t* g3, const nasseg_bf16_t* g4, const nasseg_bf16_t* g5,
                              const nasseg_bf16_t* g6, const nasseg_bf16_t* g7, int n, const nasseg_bf16_t* z,
                              const float* tstats, int act, nasseg_bf16_t* out, float* part, int B, int H, int W, int C,
                              void* stream);
int nasseg_bf16_axpby(const nasseg_bf16_t* a, const nasseg_bf16_t* b, const float* alpha, const float* beta, nasseg_bf16_t* y,
                 int64_t n, int C, int act, void* stream);
int nasseg_bf16_act_bwd(const nasseg_bf16_t* dy, const nasseg_bf16_t* ref, nasseg_bf16_t* dx, int64_t n, int act, void* stream);
int nasseg_bf16_fill(nasseg_bf16_t* y, int64_t n, float v, void* stream);
int nasseg_bf16_chan_copy(const nasseg_bf16_t* x, int64_t ldx, int xoff, nasseg_bf16_t* y, int64_t ldy, int yoff,
                     const nasseg_bf16_t* mref, int64_t ldm, int moff, int64_t P, int C, int act, int mact,
                     void* stream);
int nasseg_bf16_chan_fold(const nasseg_bf16_t* dy, nasseg_bf16_t* dx, int64_t P, int C, int rep, void* stream);
int nasseg_bf16_pool_fwd(int mode, const nasseg_bf16_t* x, nasseg_bf16_t* y, uint8_t* idx, int B, int H, int W, int C,
                    int Ho, int Wo, int K, int stride, int pad, void* stream);
int nasseg_bf16_pool_bwd(int mode, const nasseg_bf16_t* dy, const uint8_t* idx, nasseg_bf16_t* dx, int B, int H, int W,
                    int C, int Ho, int Wo, int K, int stride, int pad, void* stream);
int nasseg_bf16_bilinear_fwd(const nasseg_bf16_t* x, nasseg_bf16_t* y, int64_t ldy, int yoff, int B, int Hi, int Wi,
                        int C, int Ho, int Wo, int act, void* stream);
int nasseg_bf16_maxpool_bn_fwd(const nasseg_bf16_t* z, const float* scale, const float* shift, nasseg_bf16_t* y, uint8_t* idx,
                               int B, int H, int W, int C, int Ho, int Wo, int stride, int pad, void* stream);
int nasseg_bf16_maxpool_bn_bwd(const nasseg_bf16_t* dy, const uint8_t* idx, const nasseg_bf16_t* z, const float* mean,
                               const float* invstd, nasseg_bf16_t* g, float* stats, int B, int H, int W, int C, int Ho,
                               int Wo, int stride, int pad, void* stream);
int nasseg_bf16_cat_src_fwd(const nasseg_bf16_t* x, const float* scale, const float* shift, int act, nasseg_bf16_t* y,
                            int64_t ldy, int yoff, float* stats, int B, int Hi, int Wi, int C, int Ho, int Wo,
                            void* stream);
int nasseg_bf16_cat_src_bwd(const nasseg_bf16_t* du, const nasseg_bf16_t* slab, int64_t ld, int off, const float* sscale,
                            const float* smean, const float* sinvstd, const float* sums, int train,
                            const nasseg_bf16_t* z, const float* tstats, int act, nasseg_bf16_t* g, float* part, int B,
                            int Ho, int Wo, int C, int Hi, int Wi, void* stream);
int nasseg_bf16_bilinear_bwd_act(const nasseg_bf16_t* dy, int64_t lddy, int dyoff, const nasseg_bf16_t* z,
                                 const float* scale, const float* shift, int act, nasseg_bf16_t* dx, int B, int Hi, int Wi,
                                 int C, int Ho, int Wo, float* ws, void* stream);
int nasseg_bf16_bilinear_ac_fwd(const nasseg_bf16_t* x, nasseg_bf16_t* y, int B, int Hi, int Wi, int C, int Ho, int Wo,
                                void* stream);
int nasseg_bf16_bilinear_bwd(const nasseg_bf16_t* dy, int64_t lddy, int dyoff, nasseg_bf16_t* dx, int B, int Hi, int Wi,
                        int C, int Ho, int Wo, float* ws, void* stream);
int nasseg_bf16_ce_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, int64_t P, int C,
                  int ignore, float* out, float* ws, void* stream);
int nasseg_bf16_ce_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* stats,
                  const float* gscale, int64_t P, int C, int ignore, nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_ce_mse_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* teacher,
                           int64_t P, int C, int ignore, float* ce, float* mse, float* stats, float* ws, void* stream);
int nasseg_bf16_ce_mse_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* teacher,
                           const float* stats, const float* g_ce, const float* g_mse, int64_t P, int C, int ignore,
                           nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_ce_sel_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight,
                           int64_t P, int C, int ignore, int select, float t_loss, int64_t min_kept,
                           double keep_fraction, float* loss, float* stats, int64_t* counts, float* pixel_loss,
                           float* ws, void* stream);
int nasseg_bf16_ce_sel_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight,
                           const float* pixel_loss, const float* stats, const float* gscale, int64_t P, int C,
                           int ignore, nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_ce_region_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight,
                              int64_t P, int C, int ignore, int with_ce, int select, float t_loss, int64_t min_kept,
                              double keep_fraction, double alpha, double beta, double smooth, int all_classes,
                              double region_weight, float* loss, float* loss_ce, float* loss_region, float* stats,
                              int64_t* counts, float* pixel_loss, float* coef, float* sums, int64_t* ncls, float* ws,
                              void* stream);
int nasseg_bf16_ce_region_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight,
                              const float* pixel_loss, const float* stats, const float* coef, const float* gscale,
                              int with_ce, double region_weight, int64_t P, int C, int ignore,
                              nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_ce_up_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight, int B,
                          int h, int w, int C, int H, int W, int ignore, int select, float t_loss, int64_t min_kept,
                          double keep_fraction, float* loss, float* stats, int64_t* counts, float* pixel_loss,
                          float* lse, float* ws, void* stream);
int nasseg_bf16_ce_up_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight,
                          const float* pixel_loss, const float* lse, const float* stats, const float* gscale, int B,
                          int h, int w, int C, int H, int W, int ignore, nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_ce_up_rows_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const int64_t* rows,
                               int64_t n_rows, const float* weight, int B, int h, int w, int C, int H, int W,
                               int ignore, int select, float t_loss, int64_t min_kept, double keep_fraction,
                               float* loss, float* stats, int64_t* counts, float* pixel_loss, float* lse, float* ws,
                               void* stream);
int nasseg_bf16_ce_up_rows_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const int64_t* rows,
                               int64_t n_rows, const float* weight, const float* pixel_loss, const float* lse,
                               const float* stats, const float* gscale, int B, int h, int w, int C, int H, int W,
                               int ignore, nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_ce_up_region_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight,
                                 int B, int h, int w, int C, int H, int W, int ignore, int with_ce, int select,
                                 float t_loss, int64_t min_kept, double keep_fraction, double alpha, double beta,
                                 double smooth, int all_classes, double region_weight, float* loss, float* loss_ce,
                                 float* loss_region, float* stats, int64_t* counts, float* pixel_loss, float* lse,
                                 float* coef, float* sums, int64_t* ncls, float* gdot, float* ws, void* stream);
int nasseg_bf16_ce_up_region_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* weight,
                                 const float* pixel_loss, const float* lse, const float* stats, const float* coef,
                                 const float* gdot, const float* gscale, int with_ce, double region_weight, int B,
                                 int h, int w, int C, int H, int W, int ignore, nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_ce_up_region_rows_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size,
                                      const int64_t* rows, int64_t n_rows, const float* weight, int B, int h, int w,
                                      int C, int H, int W, int ignore, int with_ce, int select, float t_loss,
                                      int64_t min_kept, double keep_fraction, double alpha, double beta, double smooth,
                                      int all_classes, double region_weight, float* loss, float* loss_ce,
                                      float* loss_region, float* stats, int64_t* counts, float* pixel_loss, float* lse,
                                      float* coef, float* sums, int64_t* ncls, float* gdot, float* ws, void* stream);
int nasseg_bf16_ce_up_region_rows_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size,
                                      const int64_t* rows, int64_t n_rows, const float* weight,
                                      const float* pixel_loss, const float* lse, const float* stats, const float* coef,
                                      const float* gdot, const float* gscale, int with_ce, double region_weight, int B,
                                      int h, int w, int C, int H, int W, int ignore, nasseg_bf16_t* dlogits,
                                      void* stream);
int nasseg_bf16_lovasz_fwd(const nasseg_bf16_t* logits, const void* target, int elem_size, int64_t P, int C,
                           int ignore, int all_classes, double lovasz_weight, const float* base_loss, float* loss,
                           float* loss_lovasz, float* errors, float* coef, int* rank, int64_t* ncls, float* ws,
                           void* stream);
int nasseg_bf16_lovasz_bwd(const nasseg_bf16_t* logits, const void* target, int elem_size, const float* coef,
                           const float* gscale, double lovasz_weight, int accumulate, int64_t P, int C, int ignore,
                           nasseg_bf16_t* dlogits, void* stream);
int nasseg_bf16_berhu_fwd(const nasseg_bf16_t* pred, const nasseg_bf16_t* target, int64_t n, float* out, float* ws,
                     void* stream);
int nasseg_bf16_berhu_bwd(const nasseg_bf16_t* pred, const nasseg_bf16_t* target, const float* stats,
                     const float* gscale, int64_t n, nasseg_bf16_t* dpred, void* stream);
int nasseg_bf16_berhu_masked_fwd(const nasseg_bf16_t* pred, const float* target, int B, int h, int w, int H, int W,
                                 float valid_min, float valid_max, float* out, float* ws, void* stream);
int nasseg_bf16_berhu_masked_bwd(const nasseg_bf16_t* pred, const float* target, const float* stats,
                                 const float* gscale, int B, int h, int w, int H, int W, float valid_min,
                                 float valid_max, nasseg_bf16_t* dpred, void* stream);
int nasseg_bf16_berhu_up_fwd(const nasseg_bf16_t* pred, const float* target, int B, int h, int w, int H, int W,
                             float valid_min, float valid_max, float* out, float* ws, void* stream);
int nasseg_bf16_berhu_up_bwd(const nasseg_bf16_t* pred, const float* target, const float* stats, const float* gscale,
                             int B, int h, int w, int H, int W, float valid_min, float valid_max, int group,
                             nasseg_bf16_t* dpred, void* stream);
int nasseg_bf16_berhu_masked_rows_fwd(const nasseg_bf16_t* pred, const float* target, const int64_t* rows,
                                      int64_t n_rows, int B, int h, int w, int H, int W, float valid_min,
                                      float valid_max, float* out, float* ws, void* stream);
int nasseg_bf16_berhu_masked_rows_bwd(const nasseg_bf16_t* pred, const float* target, const int64_t* rows,
                                      int64_t n_rows, const float* stats, const float* gscale, int B, int h, int w,
                                      int H, int W, float valid_min, float valid_max, nasseg_bf16_t* dpred,
                                      void* stream);
int nasseg_bf16_berhu_up_rows_fwd(const nasseg_bf16_t* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                  int B, int h, int w, int H, int W, float valid_min, float valid_max, float* out,
                                  float* ws, void* stream);
int nasseg_bf16_berhu_up_rows_bwd(const nasseg_bf16_t* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                  const float* stats, const float* gscale, int B, int h, int w, int H, int W,
                                  float valid_min, float valid_max, int group, nasseg_bf16_t* dpred, void* stream);
int nasseg_bf16_depth_terms_fwd(const nasseg_bf16_t* pred, const float* target, int B, int h, int w, int H, int W,
                                float valid_min, float valid_max, float pred_min, float silog_lambda, int scales,
                                const float* berhu, float berhu_weight, float silog_weight, float grad_weight,
                                float* resid, float* out, float* ws, void* stream);
int nasseg_bf16_depth_terms_bwd(const nasseg_bf16_t* pred, const float* target, const float* resid,
                                const float* berhu, const float* terms, const float* gscale, int B, int h, int w,
                                int H, int W, float valid_min, float valid_max, float pred_min, float silog_lambda,
                                int scales, float berhu_weight, float silog_weight, float grad_weight,
                                nasseg_bf16_t* dpred, void* stream);
int nasseg_bf16_depth_terms_rows_fwd(const nasseg_bf16_t* pred, const float* target, const int64_t* rows,
                                     int64_t n_rows, int B, int h, int w, int H, int W, float valid_min,
                                     float valid_max, float pred_min, float silog_lambda, int scales,
                                     const float* berhu, float berhu_weight, float silog_weight, float grad_weight,
                                     float* resid, float* out, float* ws, void* stream);
int nasseg_bf16_depth_terms_rows_bwd(const nasseg_bf16_t* pred, const float* target, const int64_t* rows,
                                     int64_t n_rows, const float* resid, const float* berhu, const float* terms,
                                     const float* gscale, int B, int h, int w, int H, int W, float valid_min,
                                     float valid_max, float pred_min, float silog_lambda, int scales,
                                     float berhu_weight, float silog_weight, float grad_weight, nasseg_bf16_t* dpred,
                                     void* stream);
int nasseg_bf16_depth_metrics(const nasseg_bf16_t* pred, int64_t ldp, int B, int h, int w, const float* gt, int H,
                              int W, float min_depth, float max_depth, double* acc, double* ws, void* stream);
int nasseg_bf16_colred(int mode, const nasseg_bf16_t* a, int64_t lda, const nasseg_bf16_t* b, int64_t ldb,
                  const nasseg_bf16_t* c, int64_t ldc, float* out, float* ws, int S, int64_t R, int C,
                  float mul, void* stream);
int nasseg_bf16_bn_stats(const nasseg_bf16_t* x, int64_t ldx, int64_t M, int C, float eps, float momentum,
                    const float* gamma, const float* beta, float* mean, float* invstd,
                    float* scale, float* shift, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked, float* ws, void* stream);
int nasseg_bf16_bn_bwd_reduce(const nasseg_bf16_t* dy, int64_t lddy, const nasseg_bf16_t* x, int64_t ldx, int64_t M,
                         int C, const float* scale, const float* shift, const float* mean,
                         const float* invstd, int act, float* sums, float* ws, void* stream);
int nasseg_bf16_dwconv(const nasseg_bf16_t* x, const float* wt, nasseg_bf16_t* y, const float* in_scale,
                  const float* in_shift, int in_act, const float* scale, const float* shift, int act,
                  int B, int H, int W, int C, int Ho, int Wo, int K, int stride, int pad, int dil,
                  int transposed, float* stats, void* stream);
int nasseg_bf16_dwconv_bwd_data_bn(const nasseg_bf16_t* dy, const float* wt, nasseg_bf16_t* g, const nasseg_bf16_t* z,
                              const float* scale, const float* shift, const float* mean,
                              const float* invstd, int act, int B, int H, int W, int C, int Ho,
                              int Wo, int K, int stride, int pad, int dil, int transposed,
                              float* stats, void* stream);
int nasseg_bf16_dwconv_wgrad(const nasseg_bf16_t* x, const nasseg_bf16_t* dy, float* dw, float* ws,
                        const float* in_scale, const float* in_shift, int in_act, int B, int H, int W,
                        int C, int Ho, int Wo, int K, int stride, int pad, int dil, void* stream);
int nasseg_bf16_conv_fwd(const nasseg_bf16_t* x, int ldx, const float* wp, nasseg_bf16_t* y, int ldy,
                    const float* in_scale, const float* in_shift, int in_act,
                    const float* out_scale, const float* out_shift, int out_act, const nasseg_bf16_t* res,
                    int ldres, int B, int Hs, int Ws, int K, int Ho, int Wo, int N, int kh, int kw,
                    int stride, int pad, int dil, int transposed, float* stats, void* stream);
int nasseg_bf16_conv_bwd_data_bn(const nasseg_bf16_t* dy, int lddy, const float* wp, nasseg_bf16_t* g, int ldg,
                            const nasseg_bf16_t* z, int ldz, const float* scale, const float* shift,
                            const float* mean, const float* invstd, int act, int B, int Hs, int Ws,
                            int K, int Ho, int Wo, int N, int kh, int kw, int stride, int pad,
                            int dil, float* stats, void* stream);
int nasseg_bf16_conv_wgrad_many(int count, const int64_t* desc, void* stream);
int nasseg_bf16_dwconv_wgrad_many(int count, const int64_t* desc, void* stream);
int nasseg_bf16_conv_wgrad_bn(const nasseg_bf16_t* x, int ldx, const nasseg_bf16_t* g, int ldg,
                              const nasseg_bf16_t* z, int ldz, nasseg_bf16_t* dz, int lddz, float* dw, float* ws,
                              const float* in_scale, const float* in_shift, int in_act, const float* bn_scale, const float* bn_shift,
                              const float* bn_mean, const float* bn_invstd, const float* bn_sums, int bn_train, int bn_act,
                              int B, int H, int W, int K, int N, void* stream);
int nasseg_bf16_conv_wgrad_bn_flat(const nasseg_bf16_t* x, int ldx, const nasseg_bf16_t* g, int ldg,
                                   const nasseg_bf16_t* z, int ldz, float* dw, float* ws, const float* bn_scale,
                                   const float* bn_shift, const float* bn_mean, const float* bn_invstd,
                                   const float* bn_sums, int bn_train, int bn_act, int B, int Hs, int Ws, int K, int Ho,
                                   int Wo, int N, int kh, int kw, int stride, int pad, int dil, void* stream);
int nasseg_bf16_dwconv_wgrad_bn(const nasseg_bf16_t* x, const nasseg_bf16_t* g, const nasseg_bf16_t* z,
                                nasseg_bf16_t* dz, float* dw, float* ws, const float* in_scale,
                                const float* in_shift, int in_act, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                const float* bn_invstd, const float* bn_sums, int bn_train, int bn_act, int B, int H, int W,
                                int C, int Ho, int Wo, int K, int stride, int pad, int dil, void* stream);
int nasseg_bf16_conv_wgrad(const nasseg_bf16_t* x, int ldx, const nasseg_bf16_t* dy, int lddy, float* dw, float* ws,
                      const float* in_scale, const float* in_shift, int in_act, int B, int Hs,
                      int Ws, int K, int Ho, int Wo, int N, int kh, int kw, int stride, int pad,
                      int dil, void* stream);

int nasseg_bf16_augment(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                        const nasseg_bf16_t* lut, nasseg_bf16_t* image, uint8_t* mask, int B, int Ho, int Wo,
                        void* stream);
int nasseg_bf16_augment_depth(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                              const nasseg_bf16_t* lut, const float* params, float depth_scale, nasseg_bf16_t* image,
                              float* target, int B, int Ho, int Wo, void* stream);
int nasseg_bf16_augment_colour(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                               const int32_t* colour, const uint8_t* ctab, const nasseg_bf16_t* lut,
                               nasseg_bf16_t* image, uint8_t* mask, int B, int Ho, int Wo, void* stream);
int nasseg_bf16_augment_depth_colour(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                                     const int32_t* colour, const uint8_t* ctab, const nasseg_bf16_t* lut,
                                     const float* params, float depth_scale, nasseg_bf16_t* image, float* target,
                                     int B, int Ho, int Wo, void* stream);
int nasseg_bf16_resize_cubic(const nasseg_bf16_t* x, int B, int h, int w, int C, const int* taps, const float* coef,
                             float* y, int H, int W, void* stream);
int nasseg_bf16_resize_cubic_argmax(const nasseg_bf16_t* x, int B, int h, int w, int C, const int* taps,
                                    const float* coef, uint8_t* labels, int H, int W, void* stream);
int nasseg_bf16_view_image(const nasseg_bf16_t* x, nasseg_bf16_t* y, int B, int Hi, int Wi, int C, int Ho, int Wo,
                           int mirror, void* stream);
int nasseg_bf16_fuse_views(int n_views, const nasseg_bf16_t* const* views, const int* dims, const int* taps,
                           const float* coef, int n_taps, int B, int C, int H, int W, const uint8_t* gt, int n,
                           uint8_t* labels, float* probs, int64_t* cm, float* mean, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NASSEG_H */
