/* dcvc_amd.h - C ABI of libdcvc_amd.so: the MI355X (gfx950) implementation of the DCVC-RT
 * per-frame encode / decode hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; device
 * pointers are raw HIP device addresses (e.g. torch.Tensor.data_ptr()), `stream` is a
 * hipStream_t passed as void*.  Every function returns 0 on success or a negative code
 * (-1 bad argument, -2 HIP runtime error, -3 out of memory, -4 stream/decoder error) and never
 * throws; dcvc_last_error() returns a thread-local message.  No function allocates device
 * memory on the per-frame path: weights are packed at *_create, scratch is handed in by the
 * caller.  All kernels are deterministic (no atomics, fixed reduction order).
 *
 * Data layout inside the path: activations are "HWC" row-major [pixel][channel] with an explicit
 * row stride `ld` in ELEMENTS (so a producer can write into a slice of a channel-concat buffer);
 * element type is selected per object by `dtype` (DCVC_F16: _Float16 storage, fp32 MFMA
 * accumulate; DCVC_F32: float storage, fp32-input MFMA - bit-reproducible on a CPU).  Logical
 * channel counts must be multiples of 16 (outputs) / 32 (reduction dims); the Python host pads
 * 368 -> 384 and 514 -> 544 with zero weights.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root).  INTEGRATION.md shows the reference-side binding for each seam.
 */
#ifndef DCVC_AMD_H
#define DCVC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCVC_ABI_VERSION 1

enum {
    DCVC_F16 = 0,
    DCVC_F32 = 1,
    DCVC_U8 = 2, /* uint8 planes: an element type of the metric entries (dcvc_sse, dcvc_msssim_stats) ONLY */
    DCVC_U16 = 3 /* uint16 planes (samples above 8 bits, value in the LOW bits): the same two entries ONLY */
};

enum {              /* epilogue of dcvc_conv_forward */
    DCVC_EPI_BIAS = 0,      /* out = conv + bias                                       */
    DCVC_EPI_BIAS_QUANT = 1,/* out = (conv + bias) * q[c]     bias_quant, cuda_inference.py:196 */
    DCVC_EPI_SHUFFLE2 = 2,  /* out = PixelShuffle(2)(conv + bias), SubpelConv2x layers.py:29-52 */
    DCVC_EPI_WSILU = 3      /* out = wsilu(conv + bias)                                 */
};

int dcvc_abi_version(void);
const char* dcvc_last_error(void);
/* number of HIP devices visible; <0 on error (used by the host code to fail loudly). */
int dcvc_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Fused DepthConvBlock.
 * Replaces: DepthConvProxy (src/layers/extensions/inference/def.h:53-91, impl.cpp:7-121) and
 * DepthConvBlock.forward_torch (src/layers/layers.py:92-106), whose arithmetic order it follows
 * (adaptor not pre-multiplied into conv1; depthwise bias added before conv2).
 * Weights are HOST float32 pointers in the reference's torch layouts:
 *   adaptor_w [C][Cin] (NULL: no adaptor, then Cin == C), w1 [C][C], wd [C][3][3], w2 [C][C],
 *   w3 [4C][C], w4 [C][2C], biases [C] / [4C].
 * C and Cin are LOGICAL sizes; rows of the activation buffers hold round_up(.,32) channels. */
typedef struct dcvc_dcb dcvc_dcb;
typedef struct dcvc_conv dcvc_conv;   /* dense convolution layer, declared below */
int dcvc_dcb_create(int dtype, int cin, int c, int shortcut, const float* adaptor_w,
                    const float* adaptor_b, const float* w1, const float* b1, const float* wd,
                    const float* bd, const float* w2, const float* b2, const float* w3,
                    const float* b3, const float* w4, const float* b4, dcvc_dcb** out);
void dcvc_dcb_destroy(dcvc_dcb* h);
/* bytes of scratch dcvc_dcb_forward needs for an H x W input */
size_t dcvc_dcb_scratch_bytes(const dcvc_dcb* h, int H, int W);
/* x = concat(x0[:, :c0], x1[:, :c1]) (x1 may be NULL, c1 = 0); quant: device float[C] or NULL
 * (forward_with_quant_step, impl.cpp:91-97); out row stride ldo (forward_with_cat, impl.cpp:99-121:
 * the caller points `out` at the channel offset inside the concat buffer).
 * Sources and outputs of every forward entry below (blocks and convolutions) are read and written in 16-byte vectors:
 * x0, x1, out 16-byte aligned, ld0, ld1, ldo a multiple of 16 bytes and at least the channels they hold - any channel
 * slice of a wider map that keeps to this is taken; anything else is an argument error and launches nothing. */
int dcvc_dcb_forward(const dcvc_dcb* h, const void* x0, int64_t ld0, int c0, const void* x1,
                     int64_t ld1, int c1, int H, int W, const float* quant, void* out, int64_t ldo,
                     void* scratch, void* stream);
/* The same block inside a run of DepthConvBlocks that feed each other directly (the Sequential stacks of
 * video_model.py / image_model.py): the first 1x1 conv + WSiLU of a block is pointwise, so the PREVIOUS block
 * can compute it on its output tile before that tile leaves the CU.
 *   next != NULL : also produce next's pre-depthwise activation (needs: same width and type, next without
 *                  adaptor, this block without shortcut and without quant step); results are bit-identical
 *                  to calling the two blocks separately.
 *   head_done    : this block's own pre-depthwise activation was produced that way by the previous call.
 *   a_slot       : 0 / 1, alternating along the run (which half of the scratch holds this block's activation).
 * All calls of a run use the same scratch.  dcvc_dcb_forward(...) == (..., 0, 0, NULL). */
int dcvc_dcb_forward_chained(const dcvc_dcb* h, const void* x0, int64_t ld0, int c0, const void* x1,
                             int64_t ld1, int c1, int H, int W, const float* quant, void* out,
                             int64_t ldo, void* scratch, void* stream, int head_done, int a_slot,
                             const dcvc_dcb* next);

/* A run of DepthConvBlocks that ends in a 1x1 convolution of the same width (decoder.conv2 video_model.py:109, the
 * last layer of y_prior_fusion :199 and y_spatial_prior :212): the last block also computes that convolution
 * (bias, or bias * quant as dcvc_conv_forward would) on its output tile while the tile is still on the CU and writes
 * ONLY the convolution's output (conv_out, row stride ldco) - one launch and two passes over the feature map less;
 * the values are bit-identical to dcvc_dcb_forward_chained(..., next = NULL) followed by dcvc_conv_forward.
 * Needs: block without shortcut, conv 1x1 / stride 1 / cin = cout = the block's width. */
int dcvc_dcb_forward_then_conv(const dcvc_dcb* h, const void* x0, int64_t ld0, int c0, const void* x1,
                               int64_t ld1, int c1, int H, int W, void* scratch, void* stream,
                               int head_done, int a_slot, const dcvc_conv* conv, const float* conv_quant,
                               void* conv_out, int64_t ldco);

/* Measurement aid (bench.py roofline leg): runs the block `iters` times on `stream` with HIP events
 * recorded on that stream around each of its two kernels; returns the mean durations in ms. */
int dcvc_dcb_profile(const dcvc_dcb* h, const void* x0, int64_t ld0, int c0, int H, int W, void* out,
                     int64_t ldo, void* scratch, void* stream, int iters, float* head_ms, float* tail_ms);
/* The same for the second kernel (dcb_tail_kernel) alone: one head + tail launch, then `iters` back-to-back launches of
 * the tail between ONE pair of HIP events on `stream` (an event between two kernels costs 3-5 us of dispatch gap that a
 * per-launch bracket charges to the kernel); returns the mean time per launch in ms.  Blocks without adaptor only. */
int dcvc_dcb_profile_tail(const dcvc_dcb* h, const void* x0, int64_t ld0, int c0, int H, int W, void* out,
                          int64_t ldo, void* scratch, void* stream, int iters, float* tail_ms);

/* ------------------------------------------------------------------------------------------
 * Dense convolutions (implicit GEMM): 1x1, 3x3 (stride 1 or 2, pad 1), 2x2 stride 2.
 * Replaces: the at::conv2d calls of impl.cpp:61-80,133,148, video_model.py:63,127,162 and the
 * epilogue kernels bias_quant_cuda / bias_pixel_shuffle_2_cuda (kernel.cu:534,697).
 * w: HOST float32 [Cout][Cin][KH][KW]; b: HOST float32 [Cout].  For DCVC_EPI_SHUFFLE2 `cout` is
 * the conv's channel count (4 x the shuffled channel count). */
int dcvc_conv_create(int dtype, int cin, int cout, int kh, int kw, int stride, int pad, int epilogue,
                     const float* w, const float* b, dcvc_conv** out);
void dcvc_conv_destroy(dcvc_conv* h);
int dcvc_conv_forward(const dcvc_conv* h, const void* x0, int64_t ld0, int c0, const void* x1,
                      int64_t ld1, int c1, int H, int W, const float* quant, void* out, int64_t ldo,
                      void* stream);
/* The same with a per-input-channel factor applied while the input tile is staged: conv(x * in_scale[c]), the product
 * rounded to the element type exactly as dcvc_scale_channels would store it (so the values equal scale_channels followed
 * by dcvc_conv_forward; in_scale: DEVICE float32 [cin], NULL = plain forward).  Replaces the `ctx_t = conv1(x) * q_feature`
 * tensor of FeatureExtractor.forward (video_model.py:43-47), whose only reader is temporal_prior_encoder (:238, :311). */
int dcvc_conv_forward_scaled(const dcvc_conv* h, const void* x0, int64_t ld0, int c0, const void* x1,
                             int64_t ld1, int c1, int H, int W, const float* in_scale, const float* quant,
                             void* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frame <-> feature layout kernels (dtype = element type of both sides).
 * pixel_unshuffle(8) of an NCHW frame into HWC features: video_model.py:68,276, image_model.py:33 */
int dcvc_unshuffle8(int dtype, const void* x_nchw, int C, int H, int W, void* out_hwc, int64_t ldo,
                    void* stream);
/* bias + PixelShuffle(8) + clamp[0,1] from HWC [H*W][C*64] to NCHW [C][8H][8W]:
 * bias_pixel_shuffle_8 (cuda_inference.py:182-193, kernel.cu:763); bias may be NULL. */
int dcvc_shuffle8_clamp(int dtype, const void* x_hwc, int64_t ld, const float* bias, int C, int H,
                        int W, int do_clamp, void* out_nchw, void* stream);
/* Frame I/O fused into one pass each.
 * Planar 8-bit YUV 4:2:0 -> the padded YCbCr 4:4:4 model input [3][H+pad_b][W+pad_r]: nearest chroma
 * upsampling (src/utils/transforms.py:13-24), /255 and cast (test_video.py:60-63,90), replicate pad
 * (test_video.py:179). */
int dcvc_yuv420_to_frame(int dtype, const uint8_t* y, const uint8_t* u, const uint8_t* v, int H, int W,
                         int pad_b, int pad_r, void* out_nchw, void* stream);
/* Reconstruction [3][Hp][Wp] -> planar 8-bit YUV 4:2:0 of the HxW picture (test_video.py:307-311):
 * crop, chroma 2x2 mean (transforms.py:56-63), clamp(x*255, 0, 255); Y rounded, U/V truncated like
 * the reference's `.to(uint8)` unless round_uv. */
int dcvc_frame_to_yuv420(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, int round_uv,
                         uint8_t* y, uint8_t* u, uint8_t* v, void* stream);
/* PNG (RGB) sources of the reference harness: uint8 planar RGB [3][H][W] -> the padded YCbCr model input (/255, BT.709
 * rgb2ycbcr in fp32 + clamp: src/utils/transforms.py:27-38, test_video.py:84-90, replicate pad :179) ... */
int dcvc_rgb_to_frame(int dtype, const uint8_t* rgb, int H, int W, int pad_b, int pad_r, void* out_nchw,
                      void* stream);
/* ... and a reconstruction [3][Hp][Wp] -> clamp(ycbcr2rgb(x) * 255, 0, 255) of the HxW picture, [3][H][W] in the
 * storage type (transforms.py:41-53, test_video.py:118-119; every operation rounded to the storage type like the
 * reference's fp16 tensors): the values its RGB PSNR, MS-SSIM and PNG writer read. */
int dcvc_frame_to_rgb(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_chw, void* stream);
/* right/bottom edge replication on HWC: replicate_pad (cuda_inference.py:174-179), pad_for_y */
int dcvc_replicate_pad_hwc(int dtype, const void* x, int64_t ldx, int H, int W, int C, int pad_b,
                           int pad_r, void* out, int64_t ldo, void* stream);
/* out[p][c] = x[p][c] * q[c]      (ctx_t = x1 * quant, video_model.py:46) */
int dcvc_scale_channels(int dtype, const void* x, int64_t ldx, const float* q, int64_t P, int C,
                        void* out, int64_t ldo, void* stream);
/* strided 2-D copy of a channel slice (torch.cat halves, crops) */
int dcvc_copy_channels(int dtype, const void* x, int64_t ldx, int64_t P, int C, void* out,
                       int64_t ldo, void* stream);
/* crop HWC [H][W] -> [H2][W2] (hierarchical_params[:, :, :H, :W], video_model.py:283) */
int dcvc_crop_hwc(int dtype, const void* x, int64_t ldx, int W, int H2, int W2, int C, void* out,
                  int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * Entropy-model glue, HWC pipeline form (masks are computed from (h, w, c), never stored).
 *
 * z quantiser: z_hat = clamp(round(z)) in place + int8 copy in the reference's CHW order.
 * round_and_to_int8 (cuda_inference.py:26-33, kernel.cu:828). */
int dcvc_round_z(int dtype, void* z, int64_t ld, int H, int W, int C, int8_t* z_chw, void* stream);
/* int8 CHW -> HWC (get_z, entropy_models.py:221-224) */
int dcvc_z_from_int8(int dtype, const int8_t* z_chw, int H, int W, int C, void* out, int64_t ldo,
                     void* stream);

/* One checkerboard step of the ENCODER prior loop.  n_groups = 2 (video, compress_prior_2x,
 * common_model.py:143-161) or 4 (intra, compress_prior_4x, :206-256); `step` selects mask_step.
 *   q_mode 0: yq = y * (1 / max(qdec, 0.5)) per element      (separate_prior_for_video_encoding)
 *   q_mode 1: yq = y * q_enc[p] with q_enc = sigmoid(qraw[p][0]) * 1.5 + 0.5  (separate_prior :70-71)
 * Computes process_with_mask (cuda_inference.py:58-74), collapses the n_groups channel groups
 * (single_part_for_writing_*), builds the packed int16 symbol (build_index_enc :146-171) and
 * writes it in CHW order of the collapsed tensor; skipped symbols (scale <= thres) get the
 * sentinel low byte 0xFF, which dcvc_rans_encode_y drops (= the reference's boolean-mask
 * compaction `out[skip_cond]`).  y_hat accumulates:  yhat_out = (step == 0 ? 0 : yhat_in) + y_hat.
 * thres < 0 disables skipping. */
int dcvc_prior_enc_step(int dtype, int n_groups, int step, int q_mode, const void* y, int64_t ldy,
                        const void* qsrc, int64_t ldq, const void* scales, int64_t lds_,
                        const void* means, int64_t ldm, int H, int W, int C, float thres,
                        const void* yhat_in, int64_t ldhi, void* yhat_out, int64_t ldho,
                        int16_t* packed_chw, void* stream);
/* DECODER side: indexes for one step (combine_for_reading_* + build_index_dec, :77-143);
 * uint8 in CHW order of the collapsed tensor, 0xFF = skipped. */
int dcvc_prior_dec_index(int dtype, int n_groups, int step, const void* scales, int64_t lds_, int H,
                         int W, int C, float thres, uint8_t* idx_chw, void* stream);
/* DECODER side: restore_y_2x / restore_y_4x (+ running sum):
 *   yhat_out = (step == 0 ? 0 : yhat_in) + (sym + means) * mask_step   (common_model.py:196-203,270-292) */
int dcvc_prior_dec_restore(int dtype, int n_groups, int step, const int8_t* sym_chw,
                           const void* means, int64_t ldm, int H, int W, int C, const void* yhat_in,
                           int64_t ldhi, void* yhat_out, int64_t ldho, void* stream);
/* DECODER hand-off with the kept entries compacted on the device (no reference counterpart: the reference gathers the kept
 * indexes with a boolean mask, copies them with .cpu() and scatters the decoded symbols back, entropy_models.py:330-341 -
 * same stream order; the round-3 path copied the whole index / symbol arrays, ~96 % sentinels).
 *   dcvc_prior_dec_index_compact: as dcvc_prior_dec_index (idx_chw stays on the DEVICE), then the kept indexes in CHW order
 *     are written by a kernel into idx_host[0 .. *count_host) and their number into *count_host - both dcvc_host_alloc
 *     buffers (idx_host: one byte per position rounded up to 16), valid for the host once the stream has passed this point.
 *   host: dcvc_rans_dec_decode_compact decodes exactly *count_host symbols into a pinned int8 buffer (16-byte aligned,
 *     capacity as idx_host).
 *   dcvc_prior_dec_restore_compact: fetches those symbols (coalesced 16-byte reads over the host link) and restores y_hat as
 *     dcvc_prior_dec_restore does; idx_chw and workspace must be the ones of the step's index call.
 * workspace: device, 16-byte aligned, dcvc_prior_dec_compact_ws_bytes(H, W, C, n_groups) bytes. */
int64_t dcvc_prior_dec_compact_ws_bytes(int H, int W, int C, int n_groups);
int dcvc_prior_dec_index_compact(int dtype, int n_groups, int step, const void* scales, int64_t lds_, int H, int W, int C,
                                 float thres, uint8_t* idx_chw, void* workspace, uint8_t* idx_host,
                                 int32_t* count_host, void* stream);
int dcvc_prior_dec_restore_compact(int dtype, int n_groups, int step, const int8_t* sym_host, const uint8_t* idx_chw,
                                   void* workspace, const void* means, int64_t ldm, int H, int W, int C,
                                   const void* yhat_in, int64_t ldhi, void* yhat_out, int64_t ldho, void* stream);
/* The same two calls with the hand-off left in DEVICE memory (the device entropy coder, dcvc_rans_dev_decode_y, sits between
 * them): idx_dev receives the kept indexes (one byte per position rounded up to 16), *count_dev their number; sym_dev holds
 * the decoded symbols in the same order.  Nothing crosses the host link and the host never learns the count. */
int dcvc_prior_dec_index_compact_dev(int dtype, int n_groups, int step, const void* scales, int64_t lds_, int H, int W, int C,
                                     float thres, uint8_t* idx_chw, void* workspace, uint8_t* idx_dev,
                                     int32_t* count_dev, void* stream);
int dcvc_prior_dec_restore_compact_dev(int dtype, int n_groups, int step, const int8_t* sym_dev, const uint8_t* idx_chw,
                                       void* workspace, const void* means, int64_t ldm, int H, int W, int C,
                                       const void* yhat_in, int64_t ldhi, void* yhat_out, int64_t ldho, void* stream);
/* y_hat = y_hat * q   q_mode 0: max(qdec,0.5) per element; q_mode 1: sigmoid(qraw[p][1])*1.5+0.5
 * add_and_multiply (cuda_inference.py:48-55), common_model.py:246,294 */
int dcvc_prior_finish(int dtype, int q_mode, void* yhat, int64_t ldh, const void* qsrc, int64_t ldq,
                      int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Operator-module seam (inference_extensions_cuda, bind.cpp:7-36): flat NCHW-contiguous
 * elementwise kernels with the reference's own signatures (def.h:6-51).  n = element count. */
int dcvc_op_process_with_mask(int dtype, const void* y, const void* scales, const void* means,
                              const void* mask, float thres, void* y_res, void* y_q, void* y_hat,
                              void* s_hat, int64_t n, void* stream);
int dcvc_op_combine_for_reading_2x(int dtype, void* out, const void* x, const void* mask,
                                   int64_t half_n, void* stream);
int dcvc_op_restore_y_2x(int dtype, void* out, const void* y, const void* means, const void* mask,
                         int64_t half_n, void* stream);
int dcvc_op_restore_y_4x(int dtype, void* out, const void* y, const void* means, const void* mask,
                         int64_t quarter_n, void* stream);
int dcvc_op_build_index_dec(int dtype, uint8_t* out, uint8_t* cond_out, const void* scales,
                            float scale_min, float scale_max, float log_scale_min,
                            float log_step_recip, float skip_thres, int64_t n, void* stream);
int dcvc_op_build_index_enc(int dtype, int16_t* out, uint8_t* cond_out, const void* symbols,
                            const void* scales, float scale_min, float scale_max,
                            float log_scale_min, float log_step_recip, float skip_thres, int64_t n,
                            void* stream);
int dcvc_op_round_and_to_int8(int dtype, void* z, int8_t* z_int8, int64_t n, void* stream);
int dcvc_op_clamp_reciprocal_with_quant(int dtype, const void* q_dec, void* y, float min_val,
                                        void* q_out, int64_t n, void* stream);
int dcvc_op_add_and_multiply(int dtype, void* x0, const void* x1, const void* q, int64_t n,
                             void* stream);
int dcvc_op_bias_quant(int dtype, void* x, const void* bias, const void* quant, int C, int64_t HW,
                       void* stream);
int dcvc_op_bias_pixel_shuffle_8(int dtype, void* out, const void* x, const void* bias, int C, int H,
                                 int W, int do_clamp, void* stream);
int dcvc_op_replicate_pad(int dtype, const void* x, int C, int H, int W, int pad_b, int pad_r,
                          void* out, void* stream);
int dcvc_op_bias_wsilu_depthwise_conv2d(int dtype, const void* x, const void* weight,
                                        const void* bias, int C, int H, int W, void* out,
                                        void* stream);
/* NCHW <-> HWC transposes used by the operator-seam proxies */
int dcvc_nchw_to_hwc(int dtype, const void* x, int C, int64_t HW, void* out, int64_t ldo, void* stream);
int dcvc_hwc_to_nchw(int dtype, const void* x, int64_t ldx, int C, int64_t HW, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Host entropy coder (rANS).  Replaces MLCodec_extensions_cpp (src/cpp/py_rans/py_rans.cpp:14-393,
 * rans.cpp:60-534); the byte stream is identical to the reference's.  One worker thread per
 * coder half, like RansEncoderLibMultiThread / RansDecoderLibMultiThread; calls enqueue and
 * return, dcvc_rans_get_* block.  Input buffers are copied on entry unless the entry point says
 * otherwise (*_borrowed, decode_and_get_y). */
typedef struct dcvc_rans_enc dcvc_rans_enc;
typedef struct dcvc_rans_dec dcvc_rans_dec;
dcvc_rans_enc* dcvc_rans_enc_create(void);
void dcvc_rans_enc_destroy(dcvc_rans_enc*);
/* cdf [n][stride] int32, sizes [n], offsets [n] -> group index (add_cdf, py_rans.cpp:69-95) */
int dcvc_rans_enc_add_cdf(dcvc_rans_enc*, const int32_t* cdf, int n, int stride,
                          const int32_t* sizes, const int32_t* offsets);
/* forgets every table group; the next add_cdf returns 0 again (empty_cdf_buffer, py_rans.cpp:97-101) */
int dcvc_rans_enc_empty_cdf(dcvc_rans_enc*);
void dcvc_rans_enc_set_use_two(dcvc_rans_enc*, int two);
int dcvc_rans_enc_reset(dcvc_rans_enc*);
/* symbols: (int8 symbol << 8) + uint8 cdf index (encode_y, py_rans.cpp:20-41).
 * Entries whose low byte is 0xFF are dropped first (see dcvc_prior_enc_step). */
int dcvc_rans_enc_encode_y(dcvc_rans_enc*, const int16_t* symbols, int64_t n, int group);
/* same, without the copy: `symbols` must stay valid and unchanged until dcvc_rans_enc_get_stream
 * has returned (the pinned staging buffer of the D2H hand-off qualifies) */
int dcvc_rans_enc_encode_y_borrowed(dcvc_rans_enc*, const int16_t* symbols, int64_t n, int group);
int dcvc_rans_enc_encode_z(dcvc_rans_enc*, const int8_t* symbols, int64_t n, int group,
                           int start_offset, int per_channel_size);
int dcvc_rans_enc_flush(dcvc_rans_enc*);
/* blocks until the flush completed; returns the stream length, *data valid until next reset */
int64_t dcvc_rans_enc_get_stream(dcvc_rans_enc*, const uint8_t** data);

dcvc_rans_dec* dcvc_rans_dec_create(void);
void dcvc_rans_dec_destroy(dcvc_rans_dec*);
int dcvc_rans_dec_add_cdf(dcvc_rans_dec*, const int32_t* cdf, int n, int stride,
                          const int32_t* sizes, const int32_t* offsets);
int dcvc_rans_dec_empty_cdf(dcvc_rans_dec*);   /* py_rans.cpp:291-295 */
void dcvc_rans_dec_set_use_two(dcvc_rans_dec*, int two);
int dcvc_rans_dec_set_stream(dcvc_rans_dec*, const uint8_t* data, int64_t n);
/* indexes: uint8 cdf index per symbol, 0xFF = skipped (decodes nothing, yields 0).
 * The result has one int8 per index (decode_y + the scatter-back of get_y,
 * entropy_models.py:330-341). */
int dcvc_rans_dec_decode_y(dcvc_rans_dec*, const uint8_t* indexes, int64_t n, int group);
int dcvc_rans_dec_decode_z(dcvc_rans_dec*, int64_t total, int group, int start_offset,
                           int per_channel_size);
/* blocks; copies the decoded int8 symbols of the last decode_* call into out[0..n) */
int64_t dcvc_rans_dec_get(dcvc_rans_dec*, int8_t* out, int64_t capacity);
/* decode_and_get_y (py_rans.cpp:175-262 decode_y + get_decoded_tensor in one call): synchronous,
 * no staging copies - reads `indexes` and writes out[0..n) directly; the first coder runs on the
 * calling thread, the second on its worker. */
int dcvc_rans_dec_decode_and_get_y(dcvc_rans_dec*, const uint8_t* indexes, int64_t n, int group,
                                   int8_t* out);
/* The compacted form of decode_and_get_y: `indexes` holds ONLY the kept entries (count of them, stream order, as
 * dcvc_prior_dec_index_compact writes them); out[0..count) receives one int8 each.  Same coder split as above (the first
 * coder takes floor(count / 2) symbols): the two forms consume a stream identically. */
int dcvc_rans_dec_decode_compact(dcvc_rans_dec*, const uint8_t* indexes, int64_t count, int group, int8_t* out);
/* Integrity check after the LAST symbol of a frame has been decoded (no reference counterpart: the reference decodes a
 * corrupt or truncated payload into garbage, rans.cpp:356-429): a rANS decoder that has undone every encoder step is back
 * in the encoder's initial state and has consumed every byte; returns 0, or -4 with dcvc_last_error() set. */
int dcvc_rans_dec_check_end(dcvc_rans_dec*);
/* Chunked y units: this project's stream extension (docs/chunked_stream.md; NOT readable by the reference).  A unit codes
 * `count` KEPT symbols (no sentinels) in chunks of S = 1 << log2_s (8 .. 12) symbols: ceil(count / S) little-endian uint16
 * chunk byte lengths, then the chunk bodies, each an independent stream of the coder above (what reset(); encode_y(chunk);
 * flush() of one coder writes).  The coder objects only supply their table groups; set_use_two does not apply.
 *   encode: symbols (sym << 8) | index -> out[0 .. capacity); returns the unit's bytes, or a negative error code.
 *   decode: out[0 .. count) from the unit and the symbols' table indexes; -4 (dcvc_last_error() set) if the length table
 *     does not match unit_bytes / count or a chunk does not end on its last byte in the coder's initial state. */
int64_t dcvc_rans_chunked_encode_y(dcvc_rans_enc*, const int16_t* symbols, int64_t count, int group, int log2_s,
                                   uint8_t* out, int64_t capacity);
int dcvc_rans_chunked_decode_y(dcvc_rans_dec*, const uint8_t* unit, int64_t unit_bytes, const uint8_t* indexes,
                               int64_t count, int group, int log2_s, int8_t* out);
/* pmf_to_quantized_cdf (py_rans.cpp:307-364); out holds n+1 entries */
int dcvc_pmf_to_quantized_cdf(const float* pmf, int n, int precision, uint32_t* out);

/* pinned host staging buffers for the device <-> coder hand-off (hipHostMalloc / hipHostFree) */
void* dcvc_host_alloc(size_t bytes);
void dcvc_host_free(void* p);
/* the device address of a dcvc_host_alloc buffer (kernels may read / write pinned host memory in place) */
void* dcvc_host_device_ptr(void* host);
/* Encoder symbol hand-off without a copy command (replaces the reference's boolean-mask compaction + .cpu(),
 * src/layers/cuda_inference.py:159, src/models/entropy_models.py:46-52, and its device synchronisation for the size):
 * `packed` = n_parts arrays of n_per_part int16 (sym << 8 | index, low byte 0xFF = skipped, as dcvc_prior_enc_step writes
 * them).  The kept entries of part p are written IN ORDER to out_host[p * n_per_part ...] and their number to
 * counts_host[p]; both are dcvc_host_alloc buffers that the kernels write in place over the host link.  workspace: device,
 * DCVC_COMPACT_BLOCKS * n_parts int32.  The host may read the buffers once the stream has passed this point. */
#define DCVC_COMPACT_BLOCKS 256
int dcvc_compact_symbols(const int16_t* packed, int n_per_part, int n_parts, int16_t* out_host, int32_t* counts_host,
                         int32_t* workspace, void* stream);
/* dcvc_compact_symbols with the output left in DEVICE memory (input of dcvc_rans_dev_encode_y) */
int dcvc_compact_symbols_dev(const int16_t* packed, int n_per_part, int n_parts, int16_t* out_dev, int32_t* counts_dev,
                             int32_t* workspace, void* stream);
/* ------------------------------------------------------------------------------------------
 * Device entropy coder of the chunked y units (csrc/dcvc_rans_dev.hip): one lane codes one chunk, so a unit is encoded
 * and decoded by kernels enqueued on the caller's stream, with no host step and no host read of the symbol count.
 * Bytes and symbols are exactly those of dcvc_rans_chunked_encode_y / _decode_y.
 *   create: device tables of one cdf group (arguments as dcvc_rans_enc_add_cdf).  n a multiple of 4 and
 *     n * (stride + 21) <= 6144: 24 KB of tables beside the decoder's 40 KB of staged input in LDS; the 128 Gaussian
 *     tables take 20 KB.
 *   encode: sym_dev[0 .. *count_dev) (count <= max_symbols, both device) -> the unit in pinned host memory at
 *     unit_host + 16, preceded by int32 info[4] = {unit bytes, overflow flag, count, chunks}.  A chunk is built in a
 *     scratch slot of slot_bytes (a multiple of 4; 0 = the default, 2 * S + 64: two bytes is the worst case of a
 *     table-coded symbol, 4 of the 64 are the flush); a chunk that does not fit its slot, or a unit that does not fit
 *     unit_capacity, raises the overflow flag instead of writing - the unit bytes are then undefined and the caller
 *     encodes on the host.
 *     workspace: device, 16-byte aligned, dcvc_rans_dev_enc_ws_bytes(max_symbols, log2_s, slot_bytes) bytes.
 *   decode: the unit at payload_dev + unit_desc_dev[0], unit_desc_dev[1] bytes long (device int32 pair, so a captured
 *     launch serves every frame), must lie inside payload_dev[0 .. payload_capacity) (4-byte aligned).
 *     idx_dev[0 .. *count_dev) are the symbols' table indexes; sym_dev receives the symbols.  No byte outside a
 *     lane's chunk is ever used (a read past its end yields zero and marks the chunk); a damaged unit ORs
 *     DCVC_RANS_DEV_E_* bits into *error_host (pinned, the caller clears and reads it) and writes nothing else.
 *     workspace: device, 16-byte aligned, dcvc_rans_dev_dec_ws_bytes(max_symbols, log2_s) bytes. */
#define DCVC_RANS_DEV_E_COUNT 1   /* the symbol count needs a longer length table than the unit has */
#define DCVC_RANS_DEV_E_TABLE 2   /* the length table does not add up to the unit's bytes */
#define DCVC_RANS_DEV_E_CHUNK 4   /* a chunk does not end on its last byte in the coder's initial state */
#define DCVC_RANS_DEV_E_RANGE 8   /* the unit lies outside the payload buffer / a table index outside the group */
typedef struct dcvc_rans_dev dcvc_rans_dev;
int dcvc_rans_dev_create(const int32_t* cdf, int n, int stride, const int32_t* sizes, const int32_t* offsets,
                         dcvc_rans_dev** out);
void dcvc_rans_dev_destroy(dcvc_rans_dev*);
int64_t dcvc_rans_dev_enc_ws_bytes(int64_t max_symbols, int log2_s, int slot_bytes);
int dcvc_rans_dev_encode_y(const dcvc_rans_dev*, const int16_t* sym_dev, const int32_t* count_dev, int64_t max_symbols,
                           int log2_s, int slot_bytes, void* workspace, uint8_t* unit_host, int64_t unit_capacity,
                           void* stream);
int64_t dcvc_rans_dev_dec_ws_bytes(int64_t max_symbols, int log2_s);
int dcvc_rans_dev_decode_y(const dcvc_rans_dev*, const uint8_t* payload_dev, int64_t payload_capacity,
                           const int32_t* unit_desc_dev, const uint8_t* idx_dev, const int32_t* count_dev,
                           int64_t max_symbols, int log2_s, void* workspace, int8_t* sym_dev, int32_t* error_host,
                           void* stream);
/* ------------------------------------------------------------------------------------------
 * Distortion metrics of a decoded frame on the device (the reference computes them on the host from copied planes:
 * test_video.py:94-127 get_distortion, src/utils/metrics.py).  fp64 arithmetic, fixed reduction order.  Results are
 * written by a kernel into a dcvc_host_alloc buffer and are valid for the host once the stream has passed that point;
 * no call waits for the device, so all planes of a frame can be enqueued before ONE synchronisation.
 *
 * The planes get_distortion compares for a YUV 4:2:0 source (test_video.py:96-101), NOT rounded, in the storage type:
 * crop to H x W, Y = clamp(x * 255, 0, 255) [H][W], U / V = clamp(avg_pool2d(x, 2) * 255, 0, 255) [H/2][W/2] - exactly
 * the values dcvc_frame_to_yuv420 rounds / truncates to uint8.  (RGB sources: dcvc_frame_to_rgb.) */
int dcvc_frame_to_yuv420_planes(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* y, void* u, void* v,
                                void* stream);
/* *out_host = sum over i < n of ((double)a[i] - (double)b[i])^2 (calc_psnr, metrics.py:81-96, before the mean and the
 * logarithm).  a_type / b_type: DCVC_F16, DCVC_F32, DCVC_U8 or DCVC_U16.  workspace: device, DCVC_SSE_BLOCKS doubles. */
#define DCVC_SSE_BLOCKS 1024
int dcvc_sse(int a_type, const void* a, int b_type, const void* b, int64_t n, void* workspace, double* out_host,
             void* stream);
/* MS-SSIM statistics of two H x W planes (calc_msssim + calc_ssim, metrics.py:15-68; the 11x11 Gaussian window, sigma
 * 1.5, is applied directly as a row and a column pass instead of by FFT): levels = 5, or 4 if H < 176 or W < 176;
 * H < 88 or W < 88 is an argument error.  Per level l: out_host[2 l] = mean of the ssim map, out_host[2 l + 1] = mean
 * of the cs map over the 'valid' (h - 10) x (w - 10) positions; between levels the 2 x 2 box at even positions
 * (ndimage.convolve mode='reflect', then [::2, ::2]).  *levels_out (host, may be NULL) is set on return.  The final
 * prod(cs[:L-1] ** weight[:L-1]) * ssim[L-1] ** weight[L-1] is the caller's (a negative contrast mean gives NaN there, as in
 * the reference).  workspace: device, 8-byte aligned, dcvc_msssim_ws_bytes(H, W) bytes (< 0: bad size). */
int64_t dcvc_msssim_ws_bytes(int H, int W);
int dcvc_msssim_stats(int a_type, const void* a, int b_type, const void* b, int H, int W, double data_range,
                      void* workspace, double* out_host, int* levels_out, void* stream);
/* ------------------------------------------------------------------------------------------
 * Frame I/O for the other raw formats (csrc/dcvc_pixfmt.hip): bit depths 8 .. 16, 4:2:0 and 4:4:4, planar and
 * semi-planar planes, rows with a pitch.  dcvc_yuv420_to_frame / dcvc_frame_to_yuv420 above keep the reference
 * harness's 8-bit arithmetic; these entries follow the reference family's YUVReader / YUVWriter (DCVC-FM
 * src/utils/video_reader.py:130-181, video_writer.py:85-128, src/transforms/functional.py:98-131) for every format.
 *
 * A pixel format is four integers: chroma (420 or 444), bit_depth (8 .. 16; above 8 a sample is a little-endian 16-bit
 * word), semi_planar (0: planes y, u, v; 1: y and ONE plane of interleaved (U, V) pairs, v is ignored and may be
 * NULL - NV12 / P010, 4:2:0 only), msb_aligned (the value sits in the TOP bit_depth bits of its word, as in P010; not
 * with 8 bits).  max_val = (1 << bit_depth) - 1.  4:2:0 needs an even H and W.  y_stride / c_stride: distance between
 * two rows of the luma plane / of a chroma plane in SAMPLES, at least the row length (W; W / 2 for planar 4:2:0
 * chroma; W for an interleaved row), so that a surface with a pitch needs no repacking; an interleaved plane and its
 * stride are aligned to a pair.  The kernels use the widest access (up to 16 bytes per lane) the planes' addresses and
 * strides allow.  The model frame is 16-byte aligned and its row length a multiple of 8.
 * All argument checks come before any launch and need no device.
 *
 * planes -> the padded YCbCr 4:4:4 model input [3][H+pad_b][W+pad_r]: (float)sample / (float)max_val as one fp32
 * division, one rounding to the storage type, nearest chroma up-sampling for 4:2:0, replicate pad. */
int dcvc_planes_to_frame(int dtype, int chroma, int bit_depth, int semi_planar, int msb_aligned, const void* y,
                         const void* u_or_uv, const void* v, int64_t y_stride, int64_t c_stride, int H, int W, int pad_b,
                         int pad_r, void* out_nchw, void* stream);
/* reconstruction [3][Hp][Wp] -> the planes of the H x W picture: crop, every sample to fp32, 4:2:0 chroma
 * ((a + b) + (d + e)) * 0.25f over the 2x2 block, clip(., 0, 1) * max_val, round to nearest even, clip to [0, max_val],
 * shifted up if msb_aligned - luma and chroma alike. */
int dcvc_frame_to_planes(int dtype, int chroma, int bit_depth, int semi_planar, int msb_aligned, const void* x_nchw, int Hp,
                         int Wp, int H, int W, void* y, void* u_or_uv, void* v, int64_t y_stride, int64_t c_stride,
                         void* stream);
/* the values dcvc_frame_to_planes rounds, NOT rounded: clip(., 0, 1) * max_val as fp32 planes y [H][W], u / v [H/2][W/2]
 * (4:2:0) or [H][W] (4:4:4), whatever the storage type - what PSNR and MS-SSIM (data_range = max_val) compare with the
 * source's samples (DCVC_U8 / DCVC_U16 operands of dcvc_sse / dcvc_msssim_stats).  chroma = 422: the values
 * dcvc_frame_to_yuv422 rounds, u / v [H][W/2] (an even W). */
int dcvc_frame_to_metric_planes(int dtype, int chroma, int max_val, const void* x_nchw, int Hp, int Wp, int H, int W,
                                float* y, float* u, float* v, void* stream);
/* ------------------------------------------------------------------------------------------
 * 4:2:2 frame I/O (csrc/dcvc_pix422.hip, docs/pixel_formats_422.md): what SDI capture and mezzanine files deliver.  The
 * arithmetic continues the entries above: load (float)sample / (float)max_val as one fp32 division, one rounding to the
 * storage type, chroma columns doubled (nearest), replicate pad to [3][H+pad_b][W+pad_r]; store fp32 chroma
 * (a + b) * 0.5f over the pixel pair, clip(., 0, 1) * max_val, round to nearest even, clip.  W is even, H any positive
 * number.  The model frame is 16-byte aligned and its row length a multiple of 8.
 *   DCVC_422_PLANAR  planes y [H][W], u / v [H][W/2], 8 .. 16 bits, value in the low bits; strides in SAMPLES
 *   DCVC_422_UYVY    8 bits, ONE surface (u, v and c_stride are ignored), bytes U Y0 V Y1 per pixel pair; y_stride is the
 *   DCVC_422_YUYV    pitch in BYTES, at least 2 W; bytes Y0 U Y1 V.  Base and pitch are multiples of 4 (one macropixel)
 *   DCVC_422_V210    10 bits, ONE surface, pitch in BYTES, at least dcvc_v210_row_bytes(W); base and pitch are multiples
 *                    of 16.  Six pixels are four little-endian 32-bit words, bits 30 and 31 zero:
 *                      w0 = Cb0 | Y0 << 10 | Cr0 << 20     w1 = Y1 | Cb1 << 10 | Y2 << 20
 *                      w2 = Cr1 | Y3 << 10 | Cb2 << 20     w3 = Y4 | Cr2 << 10 | Y5 << 20      (Cbk / Crk: pixels 2k, 2k + 1)
 * The writer writes a v210 row for exactly dcvc_v210_row_bytes(W) bytes: samples of pixels at or beyond W, the filler
 * groups up to the 128-byte multiple and bits 30 and 31 are zero; nothing of a pitch gap is touched by any layout.  The
 * loader lets nothing of a row past pixel W - 1 reach the frame.
 * All argument checks come before any launch and need no device. */
enum { DCVC_422_PLANAR = 0, DCVC_422_UYVY = 1, DCVC_422_YUYV = 2, DCVC_422_V210 = 3 };
int64_t dcvc_v210_row_bytes(int W);          /* ((W + 47) / 48) * 128; <= 0 for W <= 0 */
int dcvc_yuv422_to_frame(int dtype, int layout, int bit_depth, const void* y_or_packed, const void* u, const void* v,
                         int64_t y_stride, int64_t c_stride, int H, int W, int pad_b, int pad_r, void* out_nchw, void* stream);
int dcvc_frame_to_yuv422(int dtype, int layout, int bit_depth, const void* x_nchw, int Hp, int Wp, int H, int W,
                         void* y_or_packed, void* u, void* v, int64_t y_stride, int64_t c_stride, void* stream);
/* ------------------------------------------------------------------------------------------
 * Separable polyphase resampler on model frames (csrc/dcvc_resize.hip, docs/reduced_resolution.md; no reference
 * counterpart): the scaler of a reduced-resolution run.  x_nchw [3][Hp][Wp] with the valid region H x W at its top left ->
 * out_nchw [3][HOp][WOp] with the valid region HO x WO, one launch for the three planes.  The tables are device memory made
 * by the caller (opendcvc_amd/resize.py): first_h [WO] / coef_h [WO][taps_h] give, per output column, the first source
 * column of its window and the window's weights; first_v [HO] / coef_v [HO][taps_v] the same per output row.  The kernel
 * knows no filter.  fp32 multiply and add in tap order, no fused multiply-add:
 *   t[y][j]   = coef_h[j][0] * x[y][i_0],  then for k = 1 .. taps_h - 1:  t = t + coef_h[j][k] * x[y][i_k]
 *   out[i][j] = coef_v[i][0] * t[y_0][j],  then for k = 1 .. taps_v - 1:  o = o + coef_v[i][k] * t[y_k][j]
 *   i_k = min(max(first_h[j] + k, 0), W - 1),  y_k = min(max(first_v[i] + k, 0), H - 1)
 * x is read in its storage type and widened; t stays fp32 (in LDS, never in memory); ONE rounding to the storage type at
 * the end, no clamp to [0, 1].  Rows and columns of the output past HO x WO are the replicate pad of the valid region.
 * The index clamps are part of the contract: whatever the tables hold, nothing outside the valid H x W region of the
 * source is read - its padding may hold anything.
 * Argument errors (checked before any device work; nothing is launched and out stays untouched): dtype; a size that is
 * not positive, Hp < H, Wp < W, HOp < HO, WOp < WO; taps outside 1 .. 64; a NULL pointer; x not aligned to its element,
 * out not 16-byte aligned or WOp no multiple of 8 (the output is stored 16 bytes per access; the source is gathered
 * element by element), a table not 4-byte aligned. */
int dcvc_resize_frame(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_nchw, int HOp, int WOp, int HO,
                      int WO, const int32_t* first_h, const float* coef_h, int taps_h, const int32_t* first_v,
                      const float* coef_v, int taps_v, void* stream);
/* ------------------------------------------------------------------------------------------
 * Active-area coding (csrc/dcvc_bars.hip; docs/active_area.md is the normative text; no reference counterpart): the
 * letterbox / pillarbox bars of a sequence are found on the device, the encoder codes the window between them and the
 * decode side pastes the window back.  Frames are model frames [3][Hp][Wp] (DCVC_F16 / DCVC_F32), the picture H x W at the
 * top left.  Every comparison runs on the ORDERED KEY of a sample: u = the bits of (float)x, key = u ^ 0x80000000 if the
 * sign bit is clear, else ~u - monotonic over all non-NaN floats (-0 below +0); a NaN is the largest or the smallest key
 * of its line and fails every test below.
 *
 * Envelope (workspace: device, 4-byte aligned, dcvc_bars_ws_bytes(H, W) = 24 (H + W) bytes, < 0: bad size): uint32 keys
 * rowmin[3][H], colmin[3][W], rowmax[3][H], colmax[3][W] in that order.  dcvc_bars_reset fills the mins with 0xFF bytes and
 * the maxes with 0x00 bytes; dcvc_bars_scan folds the valid H x W region of one frame into it with integer atomicMin /
 * atomicMax (order independent: the result is exact), any number of frames, no read-back.  Each sample is read once, 16
 * bytes per access where the tensor's address and row length allow it; nothing outside H x W is read.
 *
 * dcvc_bars_extent: one workgroup on the stream writes 8 int32 words into out8 (dcvc_host_alloc memory, valid for the host
 * once the stream has passed that point; the call does not wait): {found, top, bottom, left, right, c0, c1, c2}, c as fp32
 * bits.  With min / max decoded from the keys and every operation in fp32: a line (row or column) is FLAT iff on all three
 * planes max - min <= tol.  The candidates are row 0, row H - 1, column 0, column W - 1 in that order; the first flat one
 * sets c_p = its min_p and found = 1; none flat: found = 0 and every other word 0.  A line is a BAR iff on all planes
 * max_p <= c_p + tol and min_p >= c_p - tol.  top / bottom / left / right: the numbers of leading / trailing bar rows /
 * columns, 0 .. H or 0 .. W (an all-bar picture: top = bottom = H).
 *
 * dcvc_frame_window: the valid HO x WO region of out is x[top : top + HO, left : left + WO], the rest of out its replicate
 * pad.  dcvc_frame_paste: every element of out is written once - x where the H x W window lies at (top, left) of the
 * HO x WO picture, (T)colour[p] elsewhere inside HO x WO, the replicate pad of that beyond.  Stores are 16 bytes per
 * access, loads the widest (16 bytes .. one element) that the source's address, its row length and `left` allow.
 * Argument errors (checked before any device work, nothing is launched): dtype; a size that is not positive or a tensor
 * that does not hold its picture; a NULL or misaligned pointer; H or W above 2^20 (envelope entries); tol < 0 or NaN;
 * the window not inside the picture; out not 16-byte aligned or WOp no multiple of 8; paste: x and out overlap. */
int64_t dcvc_bars_ws_bytes(int H, int W);
int dcvc_bars_reset(void* workspace, int H, int W, void* stream);
int dcvc_bars_scan(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* workspace, void* stream);
int dcvc_bars_extent(const void* workspace, int H, int W, float tol, int32_t* out8, void* stream);
int dcvc_frame_window(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, int top, int left, void* out_nchw, int HOp,
                      int WOp, int HO, int WO, void* stream);
int dcvc_frame_paste(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_nchw, int HOp, int WOp, int HO,
                     int WO, int top, int left, const float* colour, void* stream);
/* ------------------------------------------------------------------------------------------
 * Repeated-frame coding (csrc/dcvc_repeat.hip; docs/frame_repeat.md is the normative text; no reference counterpart): is a
 * frame the same picture as another one, within a tolerance?  a and b are model frames [3][Hp][Wp] of one dtype (DCVC_F16 /
 * DCVC_F32) and one shape, the picture H x W at the top left.  For every sample of the valid H x W region of plane p:
 *   d = fabsf((float)a - (float)b)   one fp32 subtraction, no fused multiply-add
 *   key = the bits of d as uint32
 * out4[p] = the maximum key over plane p, out4[3] = 0.  The keys of non-negative floats are monotonic, so the integer max is
 * order independent and exact; +0 against -0 gives key 0; a NaN on either side, or inf - inf, gives a key above 0x7f800000,
 * which no tolerance passes (the rule of the active-area entries).  Nothing outside H x W is read.  Each sample of both
 * frames is read once, 16 bytes per access where BOTH addresses and the row length allow it, else element by element (chosen
 * on the host); wave shuffles, LDS, then one integer atomicMax per plane and workgroup (at most 96 workgroups per plane,
 * each striding over the plane's 256 x 32 tiles).
 * workspace: device memory, 4-byte aligned, dcvc_frame_maxdiff_ws_bytes() = 32 bytes, ZERO before its first use; the kernel
 * leaves it zero again (the workgroup that finishes last in a plane moves the plane's maximum to out4), so consecutive
 * compares on one stream need no memset.  One compare at a time per workspace.  out4: dcvc_host_alloc memory, 4-byte aligned, valid for the host
 * once the stream has passed that point; the call does not wait.  a == b is allowed (all zero unless a NaN is present).
 * Argument errors (checked before any device work, nothing is launched): dtype; a size that is not positive or a frame that
 * does not hold its picture; a NULL or misaligned pointer. */
int64_t dcvc_frame_maxdiff_ws_bytes(void);
int dcvc_frame_maxdiff(int dtype, const void* a_nchw, const void* b_nchw, int Hp, int Wp, int H, int W, void* workspace,
                       uint32_t* out4, void* stream);
/* ------------------------------------------------------------------------------------------
 * Deinterlacing in front of the encoder (csrc/dcvc_deint.hip; docs/deinterlace.md is the normative text, which states every
 * operation; no reference counterpart).  cur, prev and out are model frames [3][Hp][Wp] of one dtype (DCVC_F16 / DCVC_F32) and
 * one shape, the picture H x W at the top left.  keep_parity: 0 keeps the even lines (top field first), 1 the odd ones.
 * Lines are counted per plane in units of L rows: 1 for luma, chroma_lines (1 or 2) for the two chroma planes; row y is kept
 * iff (y / L) % 2 == keep_parity.  H must be a multiple of 2 * chroma_lines.
 * dcvc_deinterlace: a kept row of out is the bits of cur.  A sample of a missing row is the edge-directed mean of the lines
 * above and below it (directions -2 .. 2, the straight one preferred by 1 / 255; row offsets that leave the picture are
 * reflected, columns clamped) and, with prev not NULL, is held to d +- diff around the temporal mean d = (prev + cur) / 2, diff
 * from the differences of the two frames on the five lines around it.  fp32 on widened samples, no fused multiply-add, one
 * rounding to the dtype.  Output rows and columns past H x W are the replicate pad of the result.  Nothing outside H x W of
 * cur or prev is read.  decision: NULL, or a word of device memory read ON THE DEVICE when the kernel runs (the call does
 * not wait for it): 0 - out is cur's picture and its replicate pad, bit for bit; anything else - the filter.  One launch for
 * the three planes; 16-byte accesses where cur, prev, out and the row length allow it (chosen on the host).
 * dcvc_comb_detect: is the luma picture interlaced?  q = clamp(rint(x * 1023), 0, 1023) (a NaN counts as 0); over the kept rows
 * 1 <= y <= H - 2 and all columns, 64-bit integer sums  dc = sum |2 q_cur[y] - q_cur[y-1] - q_cur[y+1]|,  with prev
 * dp = sum |2 q_cur[y] - q_prev[y-1] - q_prev[y+1]|,  without  ds = sum |2 q_cur[y] - q_cur[y-2] - q_cur[y+2]| (offsets
 * reflected).  *decision = with prev: 8 * dc < 7 * dp ? 0 : 1;  without: dc > ds ? 1 : 0  (1: interlaced).  Integer atomics only:
 * exact whatever the order.  workspace: device memory, 8-byte aligned, dcvc_comb_ws_bytes() = 64 bytes, ZERO before its first
 * use, eight 64-bit words: [0 .. 2] the sums and the count of finished workgroups, zero again when the kernel ends (no memset
 * between two calls); [3] frames judged, [4] frames found interlaced, both running.  One call at a time per workspace;
 * decision: device memory, 4-byte aligned.  H must be even.
 * Argument errors (checked before any device work, nothing is launched): dtype; a size that is not positive or a frame that
 * does not hold its picture; keep_parity outside 0 / 1; chroma_lines outside 1 / 2; H no multiple of 2 * chroma_lines (of 2:
 * dcvc_comb_detect); a NULL cur, out, workspace or decision (dcvc_comb_detect); a pointer not aligned to its element size; out
 * overlapping cur or prev. */
int dcvc_deinterlace(int dtype, const void* cur_nchw, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity,
                     int chroma_lines, const uint32_t* decision, void* out_nchw, void* stream);
int64_t dcvc_comb_ws_bytes(void);
int dcvc_comb_detect(int dtype, const void* cur_nchw, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity,
                     void* workspace, uint32_t* decision, void* stream);
/* Field-rate output (csrc/dcvc_deint_field.hip; docs/deinterlace.md, "Field-rate output", is the normative text).  Frames,
 * keep_parity (the SOURCE's: the entry flips it itself) and chroma_lines as above.  out is B_n, the picture of cur's second
 * field with its replicate pad: dcvc_deinterlace's filter with the other parity kept, on the field-shifted frame S_n - per
 * plane the rows with (y / L) % 2 != keep_parity from cur, the others from after - with S_(n-1), the same of before and cur,
 * as its previous frame.  Neither is materialised: one launch, the frame a staged row is read from chosen by the row's parity.
 * The rows of cur's second field arrive bit for bit.  before or after NULL: the spatial predictor alone, from cur's second
 * field; then neither neighbour is read.  Nothing outside H x W is read; of before only the second field's rows are, of after
 * only the first field's.  16-byte accesses where every frame given, out and the row length allow it (chosen on the host).
 * Argument errors (checked before any device work, nothing is launched): dtype; a size that is not positive or a frame that
 * does not hold its picture; keep_parity outside 0 / 1; chroma_lines outside 1 / 2; H no multiple of 2 * chroma_lines; a NULL
 * cur or out; a pointer not aligned to its element size; out overlapping before, cur or after. */
int dcvc_deinterlace_field(int dtype, const void* before_nchw, const void* cur_nchw, const void* after_nchw, int Hp, int Wp, int H,
                           int W, int keep_parity, int chroma_lines, void* out_nchw, void* stream);
/* Film mode: field matching (csrc/dcvc_fieldmatch.hip; docs/deinterlace.md, "Film mode", is the normative text).  Frames,
 * keep_parity and chroma_lines as above.  The kept field of cur is completed by one of two candidates: c, the other field of
 * cur, or p, the other field of prev.
 * dcvc_field_match: luma only, q as dcvc_comb_detect's.  For candidate m with o = cur (c) or prev (p), over the rows y that are
 * not kept with 2 <= y <= H - 3 and all columns: a = o[y-2], b = cur[y-1], s = o[y], d = cur[y+1], e = o[y+2]; the sample is
 * combed iff (s - b and s - d are both > T or both < -T) and |a + 4 s + e - 3 (b + d)| > 6 T, T = 36.  max_m: the largest number
 * of combed samples in one 16 x 16 block (y / 16, x / 16); m is combed iff max_m > 20.  decision2[0] = filter, decision2[1] =
 * weave:  c not combed: (0, 0), the frame passes;  else prev given and p not combed: (0, 1);  else (1, 0).  Without prev, or
 * with H < 5, max_p = 0 resp. both are 0.  One launch; integer atomics only: exact whatever the order.  workspace: device memory,
 * 8-byte aligned, dcvc_field_match_ws_bytes() = 64 bytes, ZERO before its first use, sixteen 32-bit words: [0 .. 2] the two
 * maxima and the count of finished workgroups, zero again when the kernel ends (no memset between two calls); running:
 * [4] frames judged, [5] passed, [6] woven, [7] filtered; [8], [9] max_c and max_p of the last call.  One call at a time per
 * workspace; decision2: two words of device memory, 4-byte aligned, written on the device - the call does not wait.  H must
 * be even.  Nothing outside H x W is read.
 * dcvc_field_weave: in place on out.  *weave is read ON THE DEVICE: 0 - nothing is written; else in every plane every row of the
 * picture that is not kept takes prev's W samples, and out's replicate pad follows (to the right of those rows from
 * prev[y][W-1]; the rows below the picture where row H - 1 is not kept).  A copy of bits: a NaN arrives as it is.  One launch
 * for the three planes; 16-byte accesses where prev, out and the row length allow it (chosen on the host).
 * Argument errors (checked before any device work, nothing is launched): dtype; a size that is not positive or a frame that
 * does not hold its picture; keep_parity outside 0 / 1; chroma_lines outside 1 / 2; H no multiple of 2 (dcvc_field_match) or of
 * 2 * chroma_lines (dcvc_field_weave); a NULL cur, out, workspace, decision2 or weave, a NULL prev (dcvc_field_weave); a
 * pointer not aligned to its element size (workspace: 8 bytes, the words: 4); out overlapping prev. */
int64_t dcvc_field_match_ws_bytes(void);
int dcvc_field_match(int dtype, const void* cur_nchw, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity,
                     void* workspace, uint32_t* decision2, void* stream);
int dcvc_field_weave(int dtype, const void* prev_nchw, int Hp, int Wp, int H, int W, int keep_parity, int chroma_lines,
                     const uint32_t* weave, void* out_nchw, void* stream);
/* ------------------------------------------------------------------------------------------
 * Film-grain synthesis and estimation on model frames (csrc/dcvc_grain.hip; docs/film_grain.md is the normative text; no
 * reference counterpart).  The parameters of a grain unit, passed by value: strengths are standard deviations in units of
 * 2^-11 of full scale, scale_y[k] the luma strength at intensity band k (centred at (k + 0.5) / 8). */
typedef struct dcvc_grain_params {
    uint16_t seed;
    uint8_t corr;               /* 0, 1, 2: white, 3 x 3 binomial, 5 x 5 binomial */
    uint8_t scale_y[8];
    uint8_t scale_cb;
    uint8_t scale_cr;
} dcvc_grain_params;
/* x_nchw [3][Hp][Wp] with the picture H x W at its top left -> out_nchw, the same layout: inside the picture
 *   out = v + float(g * gain * s) * 2^-30   (g: the shaped noise of (seed, t, plane, row, column), an integer; s: the strength
 *   at the sample - luma: interpolated between the bands from the sample itself; ONE fp32 add, ONE rounding to the storage
 *   type, no clamp; where the product is 0 or v is a NaN, out has the bits of v),
 * outside it a bit copy.  One launch for the three planes; no sample's neighbours are read, so out_nchw may be x_nchw.  t:
 * the frame's counter since the grain unit.  Nothing is allocated and nothing waited for.
 * Argument errors (checked before any device work): dtype; a size that is not positive, Hp < H, Wp < W; a NULL pointer; a
 * tensor not aligned to its element (16-byte alignment and rows of a multiple of 16 bytes are used where present, not
 * required); corr above 2. */
int dcvc_grain_apply(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, void* out_nchw, dcvc_grain_params params,
                     uint32_t t, void* stream);
/* The estimator's table of a (noisy, clean) pair of such frames: over every whole 16 x 16 block of the H x W picture whose
 * clean luma is flat, table [12][2] int64 (device memory, 8-byte aligned; zeroed by the call) = (count, sum) per line - the
 * eight luma bands' residual variance numerators, Cb's, Cr's, and the horizontal and vertical lag-1 sums.  Integer
 * arithmetic behind the two roundings dq = rint((noisy - clean) * 4096), cq = rint(clean * 4096): the table does not
 * depend on the order of summation.  A picture smaller than a block gives the zero table.  Argument errors as above, and a
 * table that is NULL or misaligned. */
int dcvc_grain_stats(int dtype, const void* noisy_nchw, const void* clean_nchw, int Hp, int Wp, int H, int W, int64_t* table,
                     void* stream);
/* ------------------------------------------------------------------------------------------
 * Motion-compensated temporal pre-filter of the encoder's input (csrc/dcvc_tf.hip; docs/temporal_filter.md is the normative
 * text; no reference counterpart).  Frames are model frames [3][Hp][Wp] with the picture H x W at its top left; every sample
 * fetch clamps its coordinates to the picture, the padding is never read.  Nothing is allocated and nothing waited for.
 * Common argument errors (checked before any device work; nothing is launched and no output is touched): dtype; a size that
 * is not positive, Hp < H, Wp < W; a NULL pointer; a pointer not aligned to its element.
 *
 * The integer pyramid of the luma plane: Q0 [H][W] | Q1 [ceil(H/2)][ceil(W/2)] | Q2 (the halves of Q1), uint16, rows
 * contiguous, dcvc_tf_pyramid_bytes(H, W) bytes.  Q0 = dcvc_frame_analyze's 10-bit quantiser, Q(l+1) = (a + b + c + d + 2) >> 2
 * over 2 x 2 with clamped source coordinates.  One launch. */
int64_t dcvc_tf_pyramid_bytes(int H, int W);
int dcvc_tf_pyramid(int dtype, const void* x_nchw, int Hp, int Wp, int H, int W, uint16_t* pyramid, void* stream);
/* Block motion search of the current pyramid against nref (1 .. 4) reference pyramids, 8 x 8 blocks, level 2 (+-4 around 0),
 * level 1 and level 0 (+-2 around twice the parent's vector), the winner the minimum of (SAD, |dy| + |dx|, dy, dx):
 * mv [nref][gh][gw][2] int16 as (y, x), err [nref][gh][gw] uint32 (the level-0 SAD), gh = ceil(H/8), gw = ceil(W/8).
 * ws: dcvc_tf_motion_ws_bytes(H, W) bytes of device memory (the coarser levels' vectors).  Three launches.
 * Further argument errors: nref outside 1 .. 4; err not 4-byte aligned. */
int64_t dcvc_tf_motion_ws_bytes(int H, int W);
int dcvc_tf_motion(const uint16_t* cur_pyramid, const uint16_t* const* ref_pyramids, int nref, int H, int W, int16_t* mv,
                   uint32_t* err, void* ws, void* stream);
/* The weighted blend of the current frame with nref (0 .. 4) reference frames gathered at their blocks' vectors, for the
 * three planes in one launch.  refs_nchw / dists: host arrays; dists[r] is +-1 or +-2 (base weight 102 or 77 of 256), the
 * references are accumulated in the order given.  level 1 .. 5: T = 4 << level.  Per sample, fp32, multiply and add never
 * fused:  acc = 256 c;  acc = acc + float(w_r) * r  per reference;  out = acc * rcp(256 + sum w_r), ONE rounding to the
 * storage type, no clamp; where no reference has weight the bits of c.  Elements outside the picture: the replicate pad of
 * the filtered picture.  weight_sum (device memory, 8-byte aligned): the sum over the luma samples of (Wsum - 256) is ADDED
 * to it (integer vector atomics: independent of order); the caller zeroes it.
 * Further argument errors: level outside 1 .. 5; nref above 4; a distance that is not +-1 / +-2; out overlapping the current
 * frame or a reference (neighbours are read); mv, err or weight_sum misaligned. */
int dcvc_tf_blend(int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp, int H,
                  int W, const int16_t* mv, const uint32_t* err, int level, void* out_nchw, uint64_t* weight_sum, void* stream);
/* The level chosen from the picture (docs/temporal_filter.md, "Choosing the level from the picture"): one value per 8 x 8
 * block in up to three tables - the Laplacian sum of the current Q0 (S >> 2) and the level-0 SADs of the references passed
 * with distance +-1 (at most two), all clipped to 4095 - each table's lower quartile of its positive values (0 where fewer
 * than an eighth are positive), N the minimum, and the level rule.  cur_pyramid: dcvc_tf_pyramid's; err / dists: those
 * given to dcvc_tf_motion / dcvc_tf_blend (host array dists); nref 0 .. 4 - with none, or none at distance +-1, only the
 * spatial table is formed.  ws: dcvc_tf_noise_ws_bytes() bytes of device memory (three 4096-bin uint32 histograms, cleared
 * by the call).  result (device memory, 4 x int32): {level 0 .. 5, N, the smallest temporal figure or -1, the spatial
 * figure}.  totals (device memory, 8 x int64, 8-byte aligned) or NULL: totals[level] += 1, totals[6] += N, totals[7] += 1;
 * the caller zeroes it.  A memset and two launches on the stream; integer atomics only: independent of order.
 * Further argument errors: nref outside 0 .. 4; a distance that is not +-1 / +-2. */
int64_t dcvc_tf_noise_ws_bytes(void);
/* A developer's knob, not for callers: at most n (1 .. 65535) workgroups share the tiles of dcvc_tf_noise's spatial pass from
 * now on (512 as built; the result does not depend on it); any other n changes nothing.  Returns the count before the call. */
int dcvc_tf_noise_workgroups(int n);
int dcvc_tf_noise(const uint16_t* cur_pyramid, const uint32_t* err, const int* dists, int nref, int H, int W, void* ws,
                  int32_t* result, int64_t* totals, void* stream);
/* dcvc_tf_blend with its level in device memory (result of dcvc_tf_noise): the kernel reads the word once.  Level 0 gives
 * every block the weight 0: the bits of the current picture and its replicate pad, nothing added to weight_sum.  A word
 * outside 0 .. 5 counts as 0 (the host cannot check it).  The same kernel, checks and launch shape as dcvc_tf_blend.
 * Further argument errors: those of dcvc_tf_blend but the level's; level_dev NULL or not 4-byte aligned. */
int dcvc_tf_blend_auto(int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp,
                       int H, int W, const int16_t* mv, const uint32_t* err, const int32_t* level_dev, void* out_nchw,
                       uint64_t* weight_sum, void* stream);
/* Quarter-pel motion (csrc/dcvc_tf_subpel.hip; docs/temporal_filter.md, "Quarter-pel motion"), opt-in: a caller that does not
 * want it calls neither entry.  dcvc_tf_refine refines dcvc_tf_motion's level-0 vectors of nref (1 .. 4) references on the two
 * frames' Q0 (the pyramids given to dcvc_tf_motion; mv / err: its outputs, read only): stage H tries the nine vectors
 * 4 * mv + (dy, dx), dy and dx in {-2, 0, 2} quarter pels, and with subpel 2 stage Q the nine around H's winner with
 * {-1, 0, 1}; reference samples are interpolated in integers with the HEVC luma taps, a candidate ranks by its SAD, plus an
 * eighth of it unless it is the stage's centre, ties by (|dy| + |dx|, dy, dx).  mvq [nref][gh][gw][2] int16 as (y, x) in
 * quarter pels; errq [nref][gh][gw] uint32: the winner's own SAD, which takes err's place in dcvc_tf_noise and in the blend.
 * One launch, no workspace.  Further argument errors: nref outside 1 .. 4; subpel that is not 1 or 2; err or errq not 4-byte
 * aligned; mvq or errq overlapping mv, err or each other. */
int dcvc_tf_refine(const uint16_t* cur_pyramid, const uint16_t* const* ref_pyramids, int nref, int H, int W, int subpel,
                   const int16_t* mv, const uint32_t* err, int16_t* mvq, uint32_t* errq, void* stream);
/* dcvc_tf_blend with quarter-pel vectors: the reference sample is interpolated in fp32 with the same taps, rows first, each
 * sum in rising tap order over the non-zero taps and scaled by 1 / 64, multiply and add never fused, no clamp; a whole
 * component is not filtered, so a whole vector gives dcvc_tf_blend's bits.  level_dev NULL: the fixed level 1 .. 5; otherwise
 * the level is the device word, with dcvc_tf_blend_auto's meaning, and level is not looked at.  One launch for the three
 * planes.  Argument errors: those of dcvc_tf_blend (dcvc_tf_blend_auto where level_dev is given). */
int dcvc_tf_blend_subpel(int dtype, const void* cur_nchw, const void* const* refs_nchw, const int* dists, int nref, int Hp, int Wp,
                         int H, int W, const int16_t* mvq, const uint32_t* errq, int level, const int32_t* level_dev, void* out_nchw,
                         uint64_t* weight_sum, void* stream);
/* ------------------------------------------------------------------------------------------
 * Frame analysis for the encoder's scene-cut decision (csrc/dcvc_analysis.hip; no reference counterpart: the reference
 * harness places I frames by fi % intra_period only).  luma: H x W samples of the model input (DCVC_F16 / DCVC_F32), row
 * stride ld elements, read in place.  Per sample q = (int)fminf(fmaxf(rintf(v * 1023.0f), 0.0f), 1023.0f) (one fp32
 * multiply, ties to even, a NaN counts as 0); everything after it is integer arithmetic, so the result does not depend
 * on the reduction order:
 *   lowres_out[by][bx] = sum of q over the 8 x 8 block (uint16, at most 65472), shape [H/8][W/8]
 *   inter = sum |L - L_prev| over all blocks (0 if lowres_prev is NULL)
 *   intra = sum over the blocks of min(|L - left|, |L - top|); first row: |L - left|, first column: |L - top|,
 *           block (0, 0): 0
 *   total = sum L
 * out_host (dcvc_host_alloc memory, 4 words): inter, intra, total, number of blocks - written by the last of the three
 * kernels, valid for the host once the stream has passed that point; the call does not wait for the device.
 * H and W: multiples of 8, at least 8 (anything else is an argument error and launches nothing).  The luma pass reads 16
 * bytes per access where ld and the base address allow it, narrower otherwise.  workspace: device, 8-byte aligned,
 * dcvc_frame_analysis_ws_bytes(H, W) bytes (< 0: bad size).  lowres_prev and lowres_out must differ. */
int64_t dcvc_frame_analysis_ws_bytes(int H, int W);
int dcvc_frame_analyze(int dtype, const void* luma, int64_t ld, int H, int W, const uint16_t* lowres_prev,
                       uint16_t* lowres_out, void* workspace, uint64_t* out_host, void* stream);
/* ------------------------------------------------------------------------------------------
 * Pair cost of the frame lookahead (csrc/dcvc_lookahead.hip; docs/lookahead.md is the normative text; no reference
 * counterpart).  cur, ref: two low-resolution planes as dcvc_frame_analyze writes them, uint16 [bh][bw], rows contiguous
 * (any uint16 values are taken).  Integers throughout, so the result does not depend on the reduction order.  With
 * n = bh * bw, per plane mean = (sum L + n / 2) / n and ac = sum |L - mean|;
 *   w = ac_ref == 0 ? 64 : clamp((64 * ac_cur + ac_ref / 2) / ac_ref, 0, 255)
 *   o = mean_cur - ((mean_ref * w + 32) >> 6)
 *   wp(r) = clamp(((r * w + 32) >> 6) + o, 0, 65535)
 * Tiles are 8 x 8 plane samples (partial at the right and bottom edge: the samples that exist), candidates (dy, dx) in
 * [-3, 3]^2 with the reference coordinates clamped to the plane:
 *   mc = sum over the tiles of the smallest over the candidates of sum |cur[y][x] - ref[y + dy][x + dx]|
 *   wp = the same with wp(ref[..]) in place of ref[..]
 * out_host (dcvc_host_alloc memory, 8 words): mc, wp, w, o (two's complement), mean_cur, ac_cur, mean_ref, ac_ref - written
 * by the last of the three kernels, valid for the host once the stream has passed that point; the call does not wait for the
 * device, and w and o are derived on the device (no host read between the moments and the search).  workspace: device, 8-byte
 * aligned, dcvc_lookahead_ws_bytes(bh, bw) bytes (< 0: bad size).  cur and ref may be the same plane.  Argument errors
 * (checked before any device work, nothing is launched; the message names the operand): bh or bw below 1 or more than
 * 2^24 samples in all; a null or misaligned cur, ref, workspace or out_host. */
int64_t dcvc_lookahead_ws_bytes(int bh, int bw);
int dcvc_lookahead_cost(const uint16_t* cur, const uint16_t* ref, int bh, int bw, void* workspace, uint64_t* out_host,
                        void* stream);
/* ------------------------------------------------------------------------------------------
 * Payload size estimate for rate control (csrc/dcvc_rate.hip; no reference counterpart).  The sum of the code lengths of
 * one frame's symbols under the quantised CDF tables, in Q16 bits, all in integer arithmetic (independent of the
 * reduction order).  Cost tables (device, uint32, built on the host in fp64 - entropy.cost_table):
 *   row t = { meta, cost[0 .. stride - 2] },  meta = (max_value << 16) | (offset & 0xffff),  max_value = sizes[t] - 2,
 *   cost[v] = rint(65536 * (16 - log2(cdf[t][v + 1] - cdf[t][v]))) for v = 0 .. max_value (max_value: the escape symbol)
 * packed [parts][nsym] int16 (sym << 8) | idx: an entry with idx >= g_n (0xFF, the sentinel of a skipped entry) is not
 * coded; value = sym - offset; inside the table (0 <= value < max_value) it costs cost[value], otherwise
 * cost[max_value] + 2 * 65536 * (n_bypass / 3 + 1 + n_bypass) with raw / n_bypass formed as the host coder's
 * encode_symbol does.  z8 [nz] int8: the same against row z_start + i / zhw of zcost.
 * out_host (dcvc_host_alloc memory, 3 * parts + 2 words): per part {Q16 bits, kept symbols, escapes}, then z's
 * {Q16 bits, escapes} - written by the second of two kernels, valid for the host once the stream has passed that point;
 * the call does not wait for the device.  nsym: a multiple of 8, packed 16-byte aligned (read 16 bytes per access);
 * parts 1 .. 8; g_n <= 255 and g_n * g_stride <= 12288 (the Gaussian rows are staged in LDS).  workspace: device, 8-byte
 * aligned, dcvc_rate_estimate_ws_bytes(nsym, parts, nz) bytes (< 0: bad size). */
int64_t dcvc_rate_estimate_ws_bytes(int nsym, int parts, int nz);
int dcvc_rate_estimate(const int16_t* packed, int nsym, int parts, const uint32_t* gcost, int g_n, int g_stride,
                       const int8_t* z8, int nz, int zhw, const uint32_t* zcost, int z_n, int z_stride, int z_start,
                       void* workspace, uint64_t* out_host, void* stream);
/* ------------------------------------------------------------------------------------------
 * Decoder-state digest (csrc/dcvc_digest.hip, docs/state_digest.md; no reference counterpart).  data: nbytes = 8 m bytes
 * of device memory, read where they lie as m little-endian uint64 words w_0 .. w_{m-1}; all arithmetic mod 2^64:
 *   G = 0x9E3779B97F4A7C15
 *   mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   digest = sum over j of mix(w_j + (j + 1) * G)  +  mix(nbytes * G)
 * The sum is commutative, so the result does not depend on the reduction order (no atomics).  mix is a bijection and the
 * position term is fixed per word: a change confined to one word always changes the digest.  A drift and damage check,
 * not a cryptographic hash.
 * out_host (dcvc_host_alloc memory, 2 words): the digest and a status - 0 not compared (have_expected == 0), 1 equal to
 * `expected`, 2 differs - written by the second of two kernels, valid for the host once the stream has passed that point;
 * the call does not wait for the device.  nbytes <= 0, nbytes % 8 != 0 and a data pointer that is not 8-byte aligned are
 * argument errors and launch nothing (all argument checks need no device).  The buffer is read 16 bytes per access; a base
 * that is 8- but not 16-byte aligned and an odd word count are handled by the same kernel.  One grid-stride pass of the
 * full grid covers DCVC_DIGEST_PASS_WORDS words.  workspace: device, 8-byte aligned,
 * dcvc_state_digest_ws_bytes(nbytes) bytes (< 0: bad size; never more than 8 * DCVC_DIGEST_PASS_WORDS / 512). */
#define DCVC_DIGEST_PASS_WORDS 1048576
int64_t dcvc_state_digest_ws_bytes(int64_t nbytes);
int dcvc_state_digest(const void* data, int64_t nbytes, void* workspace, uint64_t expected, int have_expected,
                      uint64_t* out_host, void* stream);
/* dst[0..n) = src[0..n) on the device by a kernel (the per-frame row of the quantisation tables: src/models/video_model.py:303-305
 * slices them per call; a runtime copy command costs an order of magnitude more than the kernel) */
int dcvc_copy_f32(float* dst, const float* src, int n, void* stream);
/* stream-ordered copies (hipMemcpyAsync) and event-free host wait for a stream */
int dcvc_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int dcvc_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int dcvc_stream_sync(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCVC_AMD_H */
