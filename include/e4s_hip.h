/* libe4s_hip.so — C ABI of the MI355X (gfx950) kernels behind the E4S regional-GAN-inversion
 * hot path.  Plain pointers and sizes only: every pointer is a DEVICE pointer to fp32 data
 * (unless the name says otherwise), every tensor is dense NCHW, the caller owns all buffers
 * and passes the HIP stream to launch on (`stream` = hipStream_t, 0 = default stream).
 * Every entry point returns 0 on success, E4S_ERR_ARG (-1) for a rejected argument, or the
 * positive hipError_t of a failed launch; e4s_last_error() returns the message (thread-local).
 * Nothing here synchronises the device, allocates device memory or keeps global state.
 *
 * Each entry point names the reference interface (paths relative to the reference tree) it
 * replaces; INTEGRATION.md shows the Python/ctypes binding a maintainer would add there.
 */
#ifndef E4S_HIP_H
#define E4S_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E4S_API __attribute__((visibility("default")))
#define E4S_ABI_VERSION 1
#define E4S_ERR_ARG (-1)
#define E4S_MAX_REGIONS 16 /* regions (segmentation classes) a masked layer can mix; the reference uses 12 */
#define E4S_LABEL_NONE 255 /* label of a pixel whose one-hot column is all zero (output of the masked sum is 0) */

E4S_API int e4s_abi_version(void);
E4S_API const char* e4s_last_error(void);

/* ------------------------------------------------------------------------------------ a1
 * Replaces `fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)` —
 * models/stylegan2/op/fused_bias_act.cpp:11-21, kernel fused_bias_act_kernel.cu:18-49, launcher :52-99.
 *   out[i] = f(x[i] + bias[(i / step_b) % size_b]) * scale,  selector act*10+grad:
 *   10/11 linear, 12 zero, 30 leaky-relu, 31 leaky-relu backward (slope chosen by sign of ref[i]), 32 zero.
 * bias may be NULL (size_b = 0), ref may be NULL (treated as 0). In-place (out == x) is allowed. */
E4S_API int e4s_fused_bias_act(float* out, const float* x, const float* bias, const float* ref,
                       int act, int grad, float alpha, float scale,
                       int64_t size_x, int64_t step_b, int64_t size_b, void* stream);

/* ------------------------------------------------------------------------------------ a2
 * Replaces `upfirdn2d_op.upfirdn2d(input[major,H,W,minor], kernel[kh,kw], up_x, up_y, down_x, down_y,
 * pad_x0, pad_x1, pad_y0, pad_y1)` — models/stylegan2/op/upfirdn2d.cpp:12-23, kernel
 * upfirdn2d_kernel.cu:52-137, launcher :140-272.  minor must be 1 (the only layout the reference's
 * Python wrapper produces: op/upfirdn2d.py:96).  out is [major, out_h, out_w] with
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh)/down_y + 1 (op/upfirdn2d.py:100-101); kh,kw <= 32. */
E4S_API int e4s_upfirdn2d(float* out, const float* in, const float* kernel,
                  int major, int in_h, int in_w, int kh, int kw,
                  int up_x, int up_y, int down_x, int down_y,
                  int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* --------------------------------------------------------------------------- a3 - a6
 * Region-aware modulated synthesis.  The reference evaluates a masked layer as
 *   out = sum_c ModulatedConv2d(x, style[:, c]) * nearest(mask)[:, c]      (models/stylegan2/model.py:385-400, 442-456)
 * i.e. 12 full convolutions.  With one-hot masks this equals, per output pixel p of class c(p),
 *   out[b,o,p] = d[b,c(p),o] * sum_{i,k} (W[o,i,k]/sqrt(Cin k^2)) * s[b,c(p),i] * x[b,i,p+k]
 * which the kernels below evaluate ONCE per layer.  */

/* One-hot mask [bs, ncls, h, w] (values 0/1, utils/torch_utils.py:207-213) -> uint8 labels [bs, h, w].
 * A pixel with no class set gets E4S_LABEL_NONE.  *flag (device int, caller zeroes it) is OR-ed with
 * 1 if any value is neither 0 nor 1, with 2 if a pixel has more than one class set. */
E4S_API int e4s_onehot_to_labels(uint8_t* labels, int* flag, const float* mask, int bs, int ncls, int h, int w, void* stream);

/* Weight preparation, once per parameter version (replaces the per-call weight materialisation of
 * models/stylegan2/model.py:277-294).
 *   weight : [cout, cin, k, k]  (the ModulatedConv2d parameter without its leading 1), k = 3 or 1
 *   blur   : [4,4] FIR of the layer's Blur (model.py:212-213) when up != 0, else NULL
 *   wt     : out, [npar, cin, k*k, cout] = weight / sqrt(cin k^2), K-major; npar = 4 when up: the stride-2
 *            transposed 3x3 conv (model.py:295-297) composed with the blur (upfirdn2d pad (1,1), model.py:300)
 *            is, for each output parity (y&1, x&1), a 3x3 correlation over the INPUT grid; parity index = 2*(y&1)+(x&1)
 *   wsq    : out, [cin, cout] = sum_k (weight/sqrt(cin k^2))^2 for the demodulation table (may be NULL) */
E4S_API int e4s_modconv_prep_weights(float* wt, float* wsq, const float* weight, const float* blur,
                             int cout, int cin, int k, int up, void* stream);

/* Style and demodulation tables of one layer (model.py:276-281 for every (sample, region) at once).
 *   styles : W+ codes for this layer, element (b, r, j) at styles[b*stride_b + r*stride_r + j], j < sdim
 *   s      : out, [bs, nreg, cin]  = styles @ (mod_weight/sqrt(sdim))^T + mod_bias      (EqualLinear, model.py:154-162)
 *   d      : out, [bs, nreg, cout] = rsqrt(sum_i s^2 * wsq[i, o] + 1e-8); pass d = NULL / wsq = NULL for demodulate=False */
E4S_API int e4s_style_demod(float* s, float* d, const float* styles, int64_t stride_b, int64_t stride_r,
                    const float* mod_weight, const float* mod_bias, const float* wsq,
                    int bs, int nreg, int cin, int cout, int sdim, void* stream);

/* The same for up to E4S_MAX_STYLE_JOBS layers in two launches (all 26 modulated convs of a 1024x1024 generator: their W+ codes
 * are known before the first layer runs).  jobs is a HOST array; every pointer inside is a device pointer with the meaning of the
 * e4s_style_demod argument of the same name (d/wsq NULL for demodulate=False). */
#define E4S_MAX_STYLE_JOBS 32
typedef struct E4sStyleJob {
    float* s;
    float* d;
    const float* styles;
    int64_t stride_b, stride_r;
    const float* mod_weight;
    const float* mod_bias;
    const float* wsq;
    int nreg, cin, cout, _pad;
} E4sStyleJob;
E4S_API int e4s_style_demod_batched(const E4sStyleJob* jobs, int n_jobs, int bs, int sdim, void* stream);

/* StyledConv forward in one pass (model.py:382-423): 3x3 modulated conv (same resolution, or x2 up-conv
 * + blur when up != 0) with per-pixel region modulation, demodulation, noise injection, bias, leaky-relu*sqrt2.
 *   x       : [bs, cin, h, w]            out : [bs, cout, ho, wo]  (ho = h, or 2h when up)
 *   wt, s, d: from the two calls above (d may be NULL: no demodulation)
 *   labels  : uint8 [bs, lh, lw] region map, sampled nearest at the OUTPUT pixel (model.py:389-391); NULL = every pixel is
 *             region 0 (unmasked layer, nreg must be 1)
 *   noise   : [noise_bs (1 or bs), 1, ho, wo] or NULL;  noise_weight: device pointer to the NoiseInjection scalar (model.py:335)
 *   act_bias: [cout] FusedLeakyReLU bias or NULL; act != 0 applies leaky_relu(0.2)*sqrt(2) (model.py:421)
 *   workspace: optional scratch of workspace_floats floats (NULL/0 = none).  Feature maps too small to fill 256 CUs (4x4..32x32)
 *             are then reduced split-K over input channels: K-slices write raw partial sums to the workspace and a second
 *             launch sums them in a fixed order and applies the epilogue (deterministic; 16*bs*cout*ho*wo floats is always enough) */
E4S_API int e4s_region_modconv3x3(float* out, const float* x, const float* wt, const float* s, const float* d,
                          const uint8_t* labels, int lh, int lw,
                          const float* noise, int noise_bs, const float* noise_weight, const float* act_bias, int act,
                          int bs, int cin, int cout, int h, int w, int nreg, int up,
                          float* workspace, int64_t workspace_floats, void* stream);

/* Split-bf16 variant of the two calls above (the default fast path; numerics in DESIGN.md §4): every fp32 operand is split into
 * bf16 hi + bf16 lo and a*b is evaluated as hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32 accumulation — 3 MFMAs at 16x the fp32
 * MFMA rate.  whi / wlo : out, bf16 (as uint16) [npar][ceil(cin/16)][9][2][cout][8]: element (par, chunk, tap, half, co, e) holds input
 * channel chunk*16 + half*8 + e (zero beyond cin).  k = 3 only.  All other arguments as e4s_modconv_prep_weights / e4s_region_modconv3x3. */
E4S_API int e4s_modconv_prep_weights_sb(uint16_t* whi, uint16_t* wlo, float* wsq, const float* weight, const float* blur,
                                        int cout, int cin, int up, void* stream);
/* Layout flags OR-ed into the `up` argument of e4s_region_modconv3x3_sb (and the `act` argument of e4s_modconv_up_fused_sb): the activation
 * is channel-blocked, [bs, c/8, h, w, 8] instead of [bs, c, h, w] — a pixel's 8 channels are 32 contiguous bytes and consecutive pixels
 * follow, so a tile's halo columns share their cache lines with all 8 channels and both producer and consumer move contiguous bytes.
 * cin % 16 == 0 / cout % 8 == 0, w >= 32, single-region layers (input) / any layer (output). */
#define E4S_X_NHWC 2
#define E4S_OUT_NHWC 4
/* ... or a split-plane tensor (see "The single-region chain" below): E4S_X_SP (e4s_modconv_up_fused_sb) = x is split planes already carrying
 * this layer's modulation (s is then not applied again); E4S_OUT_SP = out is written as split planes modulated by s_next[bs][cout]. */
#define E4S_X_SP 8
#define E4S_OUT_SP 16
E4S_API int e4s_region_modconv3x3_sb(float* out, const float* x, const uint16_t* whi, const uint16_t* wlo, const float* s, const float* d,
                                     const uint8_t* labels, int lh, int lw,
                                     const float* noise, int noise_bs, const float* noise_weight, const float* act_bias, int act,
                                     int bs, int cin, int cout, int h, int w, int nreg, int up,
                                     float* workspace, int64_t workspace_floats,
                                     float* rgb_out, const float* rgb_wt, const float* rgb_s, const float* rgb_bias,
                                     const float* rgb_skip, const float* rgb_up_kernel, const float* s_next,
                                     const uint8_t* uniform_blocks, const int* uniform_ctrl, void* stream);

/* Round 3: the same masked layer on a DMA-fed kernel (csrc/modconv_mx.hip; masked layers of width >= 32, cout >= 128, cin % 16 == 0, channels-first
 * activations): the weights arrive as ready-to-DMA row slots (one kernel row of a 16-channel chunk for 128 output channels: 24-25 KB) from
 * e4s_modconv_prep_weights_mx.  arith 0 = the split-bf16 arithmetic above, bit-identical results; arith 1 = a1*w1 on the f16 MFMA plus the two cross
 * terms fp6(a)*fp6(w - w1) and fp6(a - a1)*fp6(w1) on the block-scaled MX fp6 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4): about half the matrix-pipe
 * time, 2-3x the split-bf16 error (1.9e-4 max-abs on the 1024^2 generator against 8e-5; bar 1e-3).  flags (optional, arith 1; int[2]): a wave that sees a
 * modulated activation >= 65520 (what f16 rounds to infinity) does flags[0] |= 1 and flags[1] += 1 — the result is then not to be trusted.  The library does not
 * fall back by itself (no host synchronisation in the ABI): the host layer snapshots flags[1] before and after a forward pass and re-runs a pass that moved
 * it with arith 0 (e4s2024_amd/ops.py MxGuard; the reference computes these layers in fp32, models/stylegan2/model.py:276-320).
 * e4s_modconv_mx_weight_bytes: size of the prepared copy.  All other arguments as e4s_region_modconv3x3_sb. */
E4S_API int e4s_modconv_mx_weight_bytes(int cout, int cin, int up, int arith, int64_t* bytes);
E4S_API int e4s_modconv_prep_weights_mx(void* dst, const float* weight, const float* blur, int cout, int cin, int up, int arith, void* stream);
E4S_API int e4s_region_modconv3x3_mx(float* out, const float* x, const void* wmx, int arith, int* flags, const float* s, const float* d,
                                     const uint8_t* labels, int lh, int lw,
                                     const float* noise, int noise_bs, const float* noise_weight, const float* act_bias, int act,
                                     int bs, int cin, int cout, int h, int w, int nreg, int up,
                                     float* workspace, int64_t workspace_floats,
                                     float* rgb_out, const float* rgb_wt, const float* rgb_s, const float* rgb_bias, const float* rgb_skip,
                                     const float* rgb_up_kernel, const float* s_next, const uint8_t* uniform_blocks, const int* uniform_ctrl,
                                     void* stream);
/* Round 4: the masked up layer (models/stylegan2/model.py:287-300 with the per-region mixing of :385-400) with the four output parities of a position in ONE workgroup
 * (csrc/modconv_mx4.hip): where the 2 x 2 outputs of every position of a 32 x 8-position tile share a region, the modulated / split / fp6-converted activation operand
 * is prepared once for the four composed 3x3 kernels; the other tiles are computed, inside the same launch, exactly as e4s_region_modconv3x3_mx (arith 1) computes them.
 * The result is bit-identical to that call on every map.  f16 + 2 x MX fp6 arithmetic; wmx4 from e4s_modconv_prep_weights_mx4 (weight [1,cout,cin,3,3], blur [4,4];
 * size e4s_modconv_mx4_weight_bytes), wmx from e4s_modconv_prep_weights_mx(up = 1, arith = 1); cin % 16 == 0, cout % 128 == 0, w >= 32, out 16-byte aligned, noise
 * 8-byte aligned; flags and all other arguments as for e4s_region_modconv3x3_mx. */
E4S_API int e4s_modconv_mx4_weight_bytes(int cout, int cin, int64_t* bytes);
E4S_API int e4s_modconv_prep_weights_mx4(void* dst, const float* weight, const float* blur, int cout, int cin, void* stream);
E4S_API int e4s_region_upconv_mx4(float* out, const float* x, const void* wmx4, const void* wmx, int* flags, const float* s, const float* d, const uint8_t* labels,
                                  int lh, int lw, const float* noise, int noise_bs, const float* noise_weight, const float* act_bias, int act, int bs, int cin,
                                  int cout, int h, int w, int nreg, void* stream);
/* Round 5: the region-uniform 16 x 16 output blocks of a masked up layer (models/stylegan2/model.py:287-300, 385-400; the map: e4s_uniform_blocks) on the f16 + 2 x MX-fp6
 * arithmetic with operands prepared once at staging (csrc/modconv_upblock_mx.hip): x * s[region] -> f16 + two fp6 terms per patch pixel and 32-channel chunk, weights as
 * tap-pair units by LDS-DMA, the same 1x transposed-conv form and blur epilogue.  wmx from e4s_modconv_prep_weights_upblock_mx (weight [cout,cin,3,3] or [1,cout,cin,3,3],
 * NOT blur-composed; size e4s_upblock_mx_weight_bytes); cin % 32 == 0, cin <= 512; blocks / ctrl from e4s_uniform_blocks (want_quad = 0); flags as for
 * e4s_region_modconv3x3_mx; s [bs][nreg][cin], d [bs][nreg][cout], blur [4][4], out fp32 [bs][cout][2h][2w] (only the blocks < nreg are written); w % 16 == 0. */
E4S_API int e4s_upblock_mx_weight_bytes(int cout, int cin, int64_t* bytes);
E4S_API int e4s_modconv_prep_weights_upblock_mx(void* dst, const float* weight, int cout, int cin, void* stream);
E4S_API int e4s_masked_upconv_blocks_mx(float* out, const float* x, const void* wmx, int* flags, const float* s, const float* d, const uint8_t* blocks, const int* ctrl,
                                        const float* blur, const float* noise, int noise_bs, const float* noise_weight, const float* act_bias, int act, int bs, int cin,
                                        int cout, int h, int w, int nreg, void* stream);
/* The regional-style encoder's stride-1, pad-1 3x3 convolutions (models/encoders/helpers.py:128-139) on the same kernel in its plain-convolution mode:
 *   out[bs,cout,h,w] = PReLU( conv3x3( (x - in_mean[b,ci]) * in_rstd[b,ci], W ) )          in_mean / in_rstd (together) and prelu_slope optional
 * cin % 16 == 0; padding is exactly 0 (the normalisation applies to in-image pixels only).  wmx from e4s_conv_prep_weights_mx (weight [cout,cin,3,3],
 * no scale; size: e4s_modconv_mx_weight_bytes(cout, cin, 0, arith)).  arith and flags as above. */
E4S_API int e4s_conv_prep_weights_mx(void* dst, const float* weight, int cout, int cin, int arith, void* stream);
E4S_API int e4s_conv3x3_mx(float* out, const float* x, const void* wmx, int arith, int* flags, const float* in_mean, const float* in_rstd,
                           const float* prelu_slope, int bs, int cin, int cout, int h, int w, void* stream);

/* The same operator (f16 + 2 x MX fp6 only) on the two-phase kernel of csrc/conv_mx3.hip: 32-channel chunks (cin % 32 == 0, cin <= 512), activations converted
 * to fp6 once per staged value, waves 4-7 half a unit behind waves 0-3 so that every SIMD always has a wave on the matrix pipe.  Replaces the same reference
 * statements (models/encoders/helpers.py:128-139).  wmx3 from e4s_conv_prep_weights_mx3 (weight [cout,cin,3,3]; size: e4s_conv3x3_mx3_weight_bytes);
 * flags as for e4s_region_modconv3x3_mx (flags[0] |= 1, flags[1] += 1 when a normalised activation leaves the f16 range). */
E4S_API int e4s_conv3x3_mx3_weight_bytes(int cout, int cin, int64_t* bytes);
E4S_API int e4s_conv_prep_weights_mx3(void* dst, const float* weight, int cout, int cin, void* stream);
E4S_API int e4s_conv3x3_mx3(float* out, const float* x, const void* wmx3, int* flags, const float* in_mean, const float* in_rstd, const float* prelu_slope,
                            int bs, int cin, int cout, int h, int w, void* stream);
/* The stride-2 form on the same kernel: out [bs,cout,h/2,w/2] = PReLU(conv3x3(norm(x), W, stride 2, pad 1)), h and w even — the second convolution of a stage's
 * first bottleneck_IR_SE_Ours unit (models/encoders/helpers.py:128-139 with stride = 2, psp_encoders.py get_blocks).  The input is read as its four phase planes
 * (x[2y+py][2x+px]), each a stride-1 operand of a subset of the nine taps; wmx3 from e4s_conv_prep_weights_mx3_s2 (same size as the stride-1 copy). */
E4S_API int e4s_conv_prep_weights_mx3_s2(void* dst, const float* weight, int cout, int cin, void* stream);
E4S_API int e4s_conv3x3_s2_mx3(float* out, const float* x, const void* wmx3, int* flags, const float* in_mean, const float* in_rstd, const float* prelu_slope,
                               int bs, int cin, int cout, int h, int w, int in_phased, void* stream);
/* e4s_conv3x3_mx3 with its result stored as PHASE PLANES: out[b][c][2 py + px][h/2][w/2] = result[b][c][2y+py][2x+px] (h, w even) — the hand-over between the two
 * convolutions of a stride-2 unit (helpers.py:128-139): e4s_conv3x3_s2_mx3(in_phased = 1) then reads consecutive floats with consecutive lanes, where the plain
 * map costs it two cache lines per useful one. */
E4S_API int e4s_conv3x3_mx3_phased(float* out, const float* x, const void* wmx3, int* flags, const float* in_mean, const float* in_rstd, const float* prelu_slope,
                                   int bs, int cin, int cout, int h, int w, void* stream);
/* e4s_conv3x3_mx3 with explicit memory layouts (round 5): a layout word's bit 0 (1) = phase planes as above, bit 1 (2) = CHANNEL-BLOCKED — the map is
 * [bs][c/4][plane layout][4 floats], a pixel's four channels one 16-byte element (c % 4 == 0, 16-byte aligned).  It is the hand-over between the two convolutions
 * of a bottleneck_IR_SE_Ours unit (models/encoders/helpers.py:128-139: Conv2d -> PReLU -> Conv2d with nothing between them and no other reader): the producer
 * stores 16 bytes per request, the consumer's patch threads request 8 elements per 32-channel chunk instead of 32 floats.
 * Bit 2 (4) = PREPARED OPERANDS (4, or 5 = in phase-plane pixel order; not combined with bit 1): the map is stored as what the consuming convolution's staging would
 * compute from it — per image and 32-channel block 116 h w bytes: f16 part [slot 4][pixel] x 16 B (slot s = channels 8s..8s+7) | MX-fp6 codes of the f16 part and of the
 * residual, first 16 B [term 2][pixel] | their last 8 B each [pixel] x 16 B | the two E8M0 block scales [pixel] x 4 B (bytes 0, 1) — made once per pixel in the
 * producer's epilogue (cout % 32 == 0, h w % 4 == 0; the producer raises the f16 flag for an output beyond the f16 range); as an input it takes no in_mean / in_rstd.
 * in_layout: 0, 2 or 4; out_layout: 0..5; e4s_conv3x3_s2_mx3's in_phased argument is such a word too (0..5).  Values do not depend on the layouts (bit for bit those
 * of e4s_conv3x3_mx3). */
E4S_API int e4s_conv3x3_mx3_ex(float* out, const float* x, const void* wmx3, int* flags, const float* in_mean, const float* in_rstd, const float* prelu_slope,
                               int bs, int cin, int cout, int h, int w, int in_layout, int out_layout, void* stream);
/* Masked up-sampling layers, region-uniform output blocks (model.py:287-300 per region == one transposed conv + blur where a block of output
 * pixels has ONE region):
 *   e4s_uniform_blocks: sub[b][2by+sy][2bx+sx] = the region of an 8 x 8 output sub-block (labels uint8 [bs][lh][lw] sampled 'nearest' at
 *   ho x wo), 255 = mixed / no region; blocks[b][by][bx] = the region of a 16 x 16 block if its four sub-blocks share one, 254 if each of
 *   them is uniform but they differ (only with want_quad), 255 otherwise — and 255 for a
 *   whole row of four blocks (one tile of the composed kernel) unless all four qualify; ctrl: four ints, [0] and [1] zero on entry (every launch leaves them zero again: one buffer per stream serves all layers), ctrl[2] becomes 1
 *   if at least min_percent of those rows qualify, else 0 (both consumers then leave the layer in the composed form);
 *   e4s_masked_upconv_blocks_mx (above) computes exactly the blocks < nreg in the transposed-conv form; e4s_region_modconv3x3_mx / _upconv_mx4(..., uniform_blocks = the
 *   same block map) compute the remaining blocks in the composed form.  (want_quad = 1 additionally marks blocks of four uniform 8 x 8 sub-blocks with 254: the round-2
 *   sub-block kernel that consumed them was measured slower than the composed form and deleted in round 5 — pass 0.) */
E4S_API int e4s_uniform_blocks(uint8_t* blocks, uint8_t* sub, int* ctrl, const uint8_t* labels, int bs, int lh, int lw, int ho, int wo, int nreg,
                               int want_quad, int min_percent, void* stream);
/* rgb_* (all NULL = off): fuse the single-region ToRGB that follows this layer (model.py:439-479) into the epilogue — allowed for
 * same-resolution layers of width >= 32 whose Cout fits one workgroup tile (<= 64, or <= 128 on masked layers): rgb_out [bs,3,h,w] =
 * sum_co out[co] * rgb_wt[co][o] * rgb_s[b][co] + rgb_bias[o] + upfirdn2d(rgb_skip, rgb_up_kernel, up=2, pad=(2,1)), so the layer's
 * output is not read back for the 1x1 conv.  rgb_wt from e4s_modconv_prep_weights(k=1), rgb_s = the ToRGB's s table [bs,1,cout].
 * With rgb_out given, out may be NULL: the layer's own activation is then not written at all (the last layer of the generator, whose
 * output only feeds its ToRGB). */

/* Single-region (unmasked) up layer at 1x the transposed conv's MACs, in two launches (the parity-composed kernel above spends 4x):
 *   e4s_modconv_tconv_sb : z[bs,cout,2h+1,2w+1] = conv_transpose2d(x * s, W/sqrt(9 cin), stride 2)   (model.py:287-299; raw sums)
 *                          whi/wlo from e4s_modconv_prep_weights_sb(up = 0) on the layer's 3x3 weight; s [bs,1,cin]
 *   e4s_blur_epilogue    : out[bs,cout,ho,wo] = act( d * upfirdn2d(z, blur 4x4, pad (1,1)) + noise_weight*noise + act_bias )
 *                          (model.py:300 + 419-421); d [bs,1,cout] or NULL; ho = 2h, wo = 2w */
E4S_API int e4s_modconv_tconv_sb(float* z, const float* x, const uint16_t* whi, const uint16_t* wlo, const float* s,
                                 int bs, int cin, int cout, int h, int w, void* stream);
E4S_API int e4s_blur_epilogue(float* out, const float* z, const float* blur, const float* d,
                              const float* noise, int noise_bs, const float* noise_weight, const float* act_bias, int act,
                              int bs, int cout, int ho, int wo, void* stream);

/* The same single-region up layer in ONE launch: the transposed conv's pre-blur tile stays in LDS and the 4x4 blur, demodulation,
 * noise, bias and activation are applied before the only write (no [bs,cout,2h+1,2w+1] round trip).  Arguments as the pair above. */
E4S_API int e4s_modconv_up_fused_sb(float* out, const float* x, const uint16_t* whi, const uint16_t* wlo, const float* s, const float* d,
                                    const float* blur, const float* noise, int noise_bs, const float* noise_weight,
                                    const float* act_bias, int act, int bs, int cin, int cout, int h, int w, const float* s_next, void* stream);

/* ---- The single-region chain (layers past remaining_layer_idx) on split planes.
 * A single-region layer's modulation s[b][ci] belongs to the INPUT channel alone (model.py:276-283 with one style per sample) and all
 * tables are known up front, so the producer of an activation applies the CONSUMER's modulation and the bf16 hi/lo split in its epilogue
 * and writes "split planes":  sp[plane hi|lo][bs][c/8][h][w][8 x bf16]  (c % 16 == 0; same bytes as the fp32 tensor), whose 16-byte
 * element is one lane's MFMA B fragment.  A split-plane buffer carries 16 more bytes behind the second plane, written as zeros by whoever
 * produces it (the padding source of the consumers' LDS-DMA): allocate 2 * bs * c * h * w * 2 + 16 bytes.  Consumers stage them with LDS-DMA only (no registers, no VALU) from persistent workgroups.
 * Arithmetic is that of e4s_region_modconv3x3_sb / e4s_modconv_up_fused_sb on the fp32 tensor (fl(x * s), RNE split).
 *   e4s_to_split_planes : fp32 [bs,c,h,w] (or channel-blocked [bs,c/8,h,w,8] when x_nhwc) times s[bs][c] -> split planes
 *   e4s_chain_conv3x3   : StyledConv (same resolution) reading split planes; out_sp (optional) = its activation as split planes modulated
 *                         by s_next[bs][cout]; rgb_* (optional) = the following single-region ToRGB fused as in e4s_region_modconv3x3_sb.
 *                         h % 16 == 0, w % 32 == 0; built for 32 -> 32 and 64 -> 64 channels (the 1024 / 512 stages of Generator(1024)).
 *   (the chain's up-sampling layers: e4s_modconv_up_hc below; a rank-1 blur kernel is required there, anything else takes e4s_modconv_up_fused_sb)
 * L is a HOST struct; every pointer inside is a device pointer.  whi / wlo from e4s_modconv_prep_weights_sb(up = 0). */
typedef struct E4sChainLayer {
    const uint16_t* x_sp;
    const uint16_t* whi;
    const uint16_t* wlo;
    const float* d;            /* [bs][cout] demodulation or NULL */
    const float* noise;        /* [noise_bs (1 or bs)][ho*wo] or NULL */
    const float* noise_weight;
    const float* act_bias;     /* [cout] or NULL */
    uint16_t* out_sp;          /* or NULL */
    const float* s_next;       /* [bs][cout], required with out_sp */
    float* rgb_out;            /* [bs,3,h,w] or NULL (e4s_chain_conv3x3 only) */
    const float* rgb_wt;       /* [cout][3]  (e4s_modconv_prep_weights, k = 1) */
    const float* rgb_s;        /* [bs][cout] */
    const float* rgb_bias;     /* [3] */
    const float* rgb_skip;     /* [bs,3,h/2,w/2] or NULL */
    const float* rgb_up_kernel;/* [4,4] */
    int noise_bs, act, bs, cin, cout, h, w, _pad;
} E4sChainLayer;
E4S_API int e4s_to_split_planes(uint16_t* out_sp, const float* x, const float* s, int bs, int c, int h, int w, int x_nhwc, void* stream);
E4S_API int e4s_chain_conv3x3(const E4sChainLayer* L, void* stream);

/* The chain's up layer in the HALF-COMPOSED form (csrc/modconv_uphc.hip; model.py:287-301 + 417-421, single-region case).  The 4 x 4 blur of the
 * reference is an outer product kv x kh (model.py:23-31 make_kernel of a 1-D list): its VERTICAL factor is composed into the weights — two output-row
 * parities x 9 taps over the input rows m-1, m, m+1 (2x the MACs of the bare transposed conv, no vertical tile overlap) — and its HORIZONTAL factor is
 * applied to the MFMA accumulators in registers (three DPP row shifts per register), so the epilogue needs no LDS round trip and no barrier; outputs leave
 * as 16-byte stores of split planes.
 *   e4s_modconv_prep_weights_hc : whi / wlo, bf16 (as uint16) [2 row parities][cin/16][9 = (dy+1)*3 + kx][2][cout][8] from the layer's 3x3 weight
 *                                 [1,cout,cin,3,3] (equalised-lr scale folded in) and the blur kernel [4,4]
 *   e4s_modconv_up_hc           : x_sp [2][bs][cin/8][h][w][8] split planes carrying this layer's modulation -> out_sp [2][bs][cout/8][2h][2w][8]
 *                                 (+ 16 zero bytes) modulated by s_next[bs][cout]; d [bs][cout]; cin % 16 == 0, cout % 32 == 0.
 * `blur` MUST be rank 1 (blur[r][c] == rowsum[r] * colsum[c] / sum): the caller checks that on the host (e4s2024_amd/ops.py PreparedHc) and keeps
 * e4s_modconv_up_fused_sb for any other kernel. */
E4S_API int e4s_modconv_prep_weights_hc(uint16_t* whi, uint16_t* wlo, const float* weight, const float* blur, int cout, int cin, void* stream);
E4S_API int e4s_modconv_up_hc(uint16_t* out_sp, const uint16_t* x_sp, const uint16_t* whi, const uint16_t* wlo, const float* d, const float* blur,
                              const float* noise, int noise_bs, const float* noise_weight, const float* act_bias, int act,
                              int bs, int cin, int cout, int h, int w, const float* s_next, void* stream);

/* ToRGB forward in one pass (model.py:439-479): 1x1 modulated conv without demodulation, + bias, + upsampled skip.
 *   x : [bs, cin, h, w]   wt : [cin, 3] from e4s_modconv_prep_weights(k=1)   s : [bs, nreg, cin]   bias : [3]
 *   skip : previous RGB [bs, 3, h/2, w/2] or NULL; up_kernel : [4,4] FIR of Upsample (model.py:34-53; up=2, pad=(2,1))
 *   out : [bs, 3, h, w] */
E4S_API int e4s_region_torgb(float* out, const float* x, const float* wt, const float* s,
                     const uint8_t* labels, int lh, int lw, const float* bias,
                     const float* skip, const float* up_kernel,
                     int bs, int cin, int h, int w, int nreg, void* stream);

/* ------------------------------------------------------------------------------------ a7
 * Grouped equalised linear: for g < groups, out[b,g,:] = act(x[b,g,:] @ (W[g]*scale)^T + bias[g]*bias_mul) (+ addend)
 * Replaces the 12 LocalMLP layers of models/networks.py:32-36, 226-230 (groups = 12) and EqualLinear
 * (models/stylegan2/model.py:154-164, groups = 1).
 *   x   : element (b,g,i) at x[b*x_stride_b + g*x_stride_g + i], i < in_dim
 *   W   : HOST array of `groups` (<= 16) device pointers, W[g] -> [out_dim, in_dim] (the 12 MLPs are separate parameters);
 *   bias: HOST array of `groups` device pointers to [out_dim] (entries may be NULL), or NULL
 *   act : 0 none, 1 leaky_relu(slope), 2 leaky_relu(slope) * sqrt(2) (fused_lrelu)
 *   addend : [out_dim] added to every (b,g) row, or NULL (latent_avg, networks.py:247)
 *   out : element (b,g,o) at out[b*out_stride_b + g*out_stride_g + o] */
E4S_API int e4s_grouped_linear(float* out, int64_t out_stride_b, int64_t out_stride_g,
                       const float* x, int64_t x_stride_b, int64_t x_stride_g,
                       const float* const* W, const float* const* bias, const float* addend,
                       float scale, float bias_mul, int act, float slope,
                       int bs, int groups, int in_dim, int out_dim, void* stream);

/* Backward of e4s_grouped_linear for dense [bs][groups][...] tensors (f1: PTI trains the LocalMLPs, training/video_swap_ft_coach.py:297-299).
 * gy = dL/d(pre-activation) [bs][groups][out_dim].  dW [groups][out_dim][in_dim] = scale * sum_b gy x^T and db [groups][out_dim] =
 * bias_mul * sum_b gy (either may be NULL);  dx [bs][groups][in_dim] = scale * W^T gy, times leaky_relu'(h_prev) when h_prev (the previous
 * layer's OUTPUT, same shape as dx) is given — or NULL for no input gradient.  scratch: osplit * bs * groups * in_dim floats (the sum over
 * out_dim is split over osplit workgroups and finished in a fixed order).  bs <= 8, in_dim % 4 == 0. */
E4S_API int e4s_grouped_linear_bwd(float* dW, float* db, float* dx, float* scratch, const float* gy, const float* x, const float* const* W,
                                   const float* h_prev, float scale, float bias_mul, float slope, int bs, int groups, int in_dim, int out_dim,
                                   int osplit, void* stream);

/* out[j][n] = sum_k T[j][k] w[n][k] (trans = 0; w [N][K], out [J][N]) or its transpose dw[n][k] = sum_j T[j][k] g[j][n] (trans = 1): a constant
 * J x K map (J, K <= 36) along a long axis — the composition of an up layer's 3x3 weight with its blur kernel into the four parity weights
 * (J = 36, K = 9, N = cout * cin; models/stylegan2/model.py:287-300 composed) and its gradient.  grouped != 0 (J = 36, K = 9 only):
 * the J side is stored [4][N][9] — out[g][n][t] for j = 9 g + t — i.e. the four parity weights as [4][cout][cin][3][3]. */
E4S_API int e4s_small_map(float* out, const float* T, const float* in, int J, int K, int64_t N, int trans, int grouped, void* stream);

/* ------------------------------------------------------------------------------------ a8 / a9: plain convolutions
 * Replaces the F.conv2d calls of the regional-style encoder (models/encoders/psp_encoders.py:334, helpers.py:128-139)
 * and of BiSeNet / ResNet-18 (swap_face_fine/face_parsing/model.py:23-35, resnet.py:15-49) with one implicit-GEMM kernel on
 * fp32 MFMA.  Weights are first re-laid out K-major (once per parameter version):
 *   wt[ci][tap][co] = weight[co][ci][tap] * g[co];  bias_out[co] = beta - mean*g (+ conv_bias*g);  g = gamma/sqrt(var+eps)
 * (BatchNorm2d in eval mode folds into the bias-free conv in front of it; pass bn_* = NULL for a plain conv). */
E4S_API int e4s_conv_prep_weights(float* wt, float* bias_out, const float* weight,
                                  const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                                  const float* conv_bias, int cout, int cin, int kh, int kw, void* stream);

/* out[bs,cout,ho,wo] = act( conv(x', wt) + bias + residual ),  ho = (h + 2*pad - ks)/stride + 1.
 *   x0 / x1 : input channels [0,cin0) come from x0 [bs,cin0,h,w], [cin0,cin) from x1 [bs,cin-cin0,h,w] (x1 = NULL: all from x0) —
 *             the channel concatenation of FeatureFusionModule (face_parsing/model.py:207) without a copy
 *   in_mean / in_rstd : [bs,cin] or NULL — InstanceNorm2d of the INPUT applied while staging, x' = (x - mean)*rstd inside the
 *             image and 0 in the padding (helpers.py:134: InstanceNorm2d -> Conv2d)
 *   act : 0 none, 1 ReLU, 2 PReLU(prelu_slope[cout]);  residual : [bs,cout,ho,wo] added before the activation (resnet.py:46-48)
 *   ks/stride : (3,1) (3,2) (1,1) (1,2) (7,2) */
E4S_API int e4s_conv2d(float* out, const float* x0, const float* x1, int cin0, const float* wt, const float* bias,
                       const float* in_mean, const float* in_rstd, const float* prelu_slope, const float* residual, int act,
                       int bs, int cin, int cout, int h, int w, int ks, int stride, int pad, void* stream);

/* Split-bf16 variants (3 bf16 MFMAs per fp32 product, fp32 accumulate) of the two calls above, for 3x3 / 1x1
 * kernels.  whi / wlo: bf16 (as uint16) [ceil(cin/16)][kh*kw][2][cout][8] — element (chunk, tap, half, co, e) is input channel
 * chunk*16 + half*8 + e.  Same fusions as e4s_conv2d. */
E4S_API int e4s_conv_prep_weights_sb(uint16_t* whi, uint16_t* wlo, float* bias_out, const float* weight,
                                     const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                                     const float* conv_bias, int cout, int cin, int kh, int kw, void* stream);
E4S_API int e4s_conv2d_sb(float* out, const float* x0, const float* x1, int cin0, const uint16_t* whi, const uint16_t* wlo, const float* bias,
                          const float* in_mean, const float* in_rstd, const float* prelu_slope, const float* residual, int act,
                          int bs, int cin, int cout, int h, int w, int ks, int stride, int pad, void* stream);
/* Three-way split (w = w0 + w1 + w2, x likewise; 6 bf16 MFMAs per 16-deep step: a0b0 + a0b1 + a1b0 + a0b2 + a2b0 + a1b1, fp32
 * accumulate): fp32-class error (~2^-24 per product) at 2.7x less matrix-pipe time than the exact fp32 kernel.  Meant for the face
 * parser (swap_face_fine/face_parsing/model.py:20-260), whose argmax must not move.  Slabs from e4s_conv_prep_weights_sb3. */
E4S_API int e4s_conv_prep_weights_sb3(uint16_t* w0, uint16_t* w1, uint16_t* w2, float* bias_out, const float* weight,
                                      const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                                      float bn_eps, const float* conv_bias, int cout, int cin, int kh, int kw, void* stream);
E4S_API int e4s_conv2d_sb3(float* out, const float* x0, const float* x1, int cin0, const uint16_t* w0, const uint16_t* w1,
                           const uint16_t* w2, const float* bias, const float* in_mean, const float* in_rstd,
                           const float* prelu_slope, const float* residual, int act, int bs, int cin, int cout, int h, int w,
                           int ks, int stride, int pad, void* stream);
/* Round 3: the fp32-class convolution at half the MFMAs of the three-way bf16 split — TWO f16 terms per operand (11 significand bits each where bf16 has 8),
 * a1*b1 + a1*b2 + a2*b1 on v_mfma_f32_32x32x16_f16, ~2^-23 per product.  w1 / w2: f16 (as uint16) slabs of weight * 2^wscale_log2 in the layout of
 * e4s_conv_prep_weights_sb — the power of two keeps the second term a normal f16; pick it so that the largest (BatchNorm-folded) weight lands near 2^10 and
 * pass the same value to e4s_conv2d_f16x3, which takes it out again.  Activations are used as they are (|x| < 65520 — a wave that stages a larger one raises
 * flags[0] bit 0 and bumps the counter flags[1] (flags may be NULL), the result is then invalid and the caller re-runs the pass on e4s_conv2d_sb3; their second term loses bits below
 * |x| ~ 2^-3, harmless next to the O(1) activations of the networks on this path).  Same fusions as e4s_conv2d. */
E4S_API int e4s_conv_prep_weights_f16x3(uint16_t* w1, uint16_t* w2, float* bias_out, const float* weight,
                                        const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                                        const float* conv_bias, int cout, int cin, int kh, int kw, int wscale_log2, void* stream);
E4S_API int e4s_conv2d_f16x3(float* out, const float* x0, const float* x1, int cin0, const uint16_t* w1, const uint16_t* w2, const float* bias,
                             const float* in_mean, const float* in_rstd, const float* prelu_slope, const float* residual, int act,
                             int bs, int cin, int cout, int h, int w, int ks, int stride, int pad, int wscale_log2, int* flags, void* stream);

/* Per-plane statistics of x [planes = bs*C, hw]: mean, rstd = 1/sqrt(biased var + eps) (InstanceNorm2d without affine / running
 * stats, helpers.py:133,138), nmean = mean of the normalised plane (what SEModule's avg_pool sees, helpers.py:66).  rstd and nmean
 * may be NULL (plain global average pooling: face_parsing/model.py:83, 116, 209). */
E4S_API int e4s_plane_stats(float* mean, float* rstd, float* nmean, const float* x, int planes, int hw, float eps, void* stream);

/* y[bs,cout] = act( bn( x[bs,cin] @ W[cout,cin]^T ) ), bn optional (eval BatchNorm), act: 0 none, 1 ReLU, 3 sigmoid.
 * The 1x1 convolutions on pooled vectors: SEModule fc1/fc2 (helpers.py:67-71), ARM attention (face_parsing/model.py:84-86),
 * FFM attention (:210-213), conv_avg (:117). */
E4S_API int e4s_vec_fc(float* y, const float* x, const float* W, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                       const float* bn_var, float bn_eps, int act, int bs, int cin, int cout, void* stream);

/* out = prelu( ((x - mean)*rstd) * gate + shortcut' ),  every modifier optional (NULL):
 *   mean,rstd,gate,sc_mean,sc_rstd : [bs,C];  shortcut : [bs,C,h*sc_stride,w*sc_stride] sampled at (y*sc_stride, x*sc_stride)
 *   (MaxPool2d(1,stride), helpers.py:126) and instance-normalised when sc_mean is given (helpers.py:128-131);  prelu : [C].
 * Tail of bottleneck_IR_SE_Ours.forward (helpers.py:141-144) and InstanceNorm+PReLU of the input layer (psp_encoders.py:335-336). */
E4S_API int e4s_norm_gate_add(float* out, const float* x, const float* mean, const float* rstd, const float* gate,
                              const float* shortcut, const float* sc_mean, const float* sc_rstd, int sc_stride, const float* prelu,
                              int bs, int C, int h, int w, void* stream);
/* SEModule's gate (helpers.py:56-72) in one launch: gate[b, o] = sigmoid(fc2 . relu(fc1 . pooled[b])), fc1 [H, C], fc2 [C, H], no biases, H <= 64;
 * value for value what two e4s_vec_fc calls give. */
E4S_API int e4s_se_gate(float* gate, const float* pooled, const float* w1, const float* w2, int bs, int C, int H, void* stream);
/* e4s_norm_gate_add that also returns InstanceNorm statistics (mean, 1/sqrt(var + eps), as e4s_plane_stats computes them) of its OUTPUT planes:
 * the next bottleneck_IR_SE unit (helpers.py:122-144) normalises exactly that tensor.  Planes of at most 16384 pixels, a multiple of 4. */
E4S_API int e4s_norm_gate_add_stats(float* out, float* out_mean, float* out_rstd, const float* x, const float* mean, const float* rstd,
                                    const float* gate, const float* shortcut, const float* sc_mean, const float* sc_rstd, int sc_stride,
                                    const float* prelu, int bs, int C, int h, int w, float eps, void* stream);
/* The same with the InstanceNorm statistics of the INPUT x computed in the launch as well (mean and 1 / sqrt(var + in_eps) of every plane, exactly e4s_plane_stats' sums):
 * out = prelu( IN(x) * gate + shortcut' ) and the statistics of out — InstanceNorm2d(depth) + SEModule + the shortcut add of bottleneck_IR_SE_Ours (helpers.py:128-144) in one
 * launch, for a gate that does not depend on x (the host passes the constant 1/2: see ops.SE_GATE_IS_HALF). */
E4S_API int e4s_norm_self_gate_add_stats(float* out, float* out_mean, float* out_rstd, const float* x, float in_eps, const float* gate, const float* shortcut,
                                         const float* sc_mean, const float* sc_rstd, int sc_stride, const float* prelu, int bs, int C, int h, int w, float eps,
                                         void* stream);

/* Masked average pooling per region (psp_encoders.py:355-375): out[bs,nreg,C] = mean of feats[bs,C,h,w] over the pixels whose
 * label (uint8 [bs,lh,lw], sampled nearest at h x w) equals the region, zeros for an empty region. */
E4S_API int e4s_masked_avg_pool(float* out, const float* feats, const uint8_t* labels, int lh, int lw,
                                int bs, int C, int h, int w, int nreg, void* stream);

/* F.interpolate(mode='bilinear', align_corners=...) on [planes, ih, iw] -> [planes, oh, ow], no antialias
 * (models/networks.py:217 uses align_corners=False; face_parsing/model.py:257-259 uses True). */
E4S_API int e4s_bilinear_resize(float* out, const float* in, int planes, int ih, int iw, int oh, int ow, int align_corners, void* stream);

/* ------------------------------------------------------------------------------------ a9 / a10: parser glue */
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on [planes,h,w] (resnet.py:65, 75). */
E4S_API int e4s_maxpool3x3s2(float* out, const float* in, int planes, int h, int w, void* stream);

/* out[p,Y,X] = feat[p,Y/up,X/up]*gate[p] + add_map[p,Y/up,X/up] + add_vec[p]  (gate/add_map/add_vec optional), planes = bs*C:
 * ARM gating + context add + nearest upsample of ContextPath (face_parsing/model.py:118-128) and FFM's feat*atten+feat (:214-215). */
E4S_API int e4s_gate_add_upsample(float* out, const float* feat, const float* gate, const float* add_map, const float* add_vec,
                                  int planes, int h, int w, int up, void* stream);

/* The face parser's ResNet stem, Conv2d(3, 64, 7, stride 2, pad 3) + folded BatchNorm + ReLU (swap_face_fine/face_parsing/resnet.py:57-58, 66), as an implicit
 * GEMM over the flattened (channel, ky, kx) axis (K = 147 in ten 16-deep steps) in the two-term f16 split of e4s_conv2d_f16x3:
 *   out [bs,64,ho,wo] = act(conv(x [bs,3,h,w]) * 2^-wscale_log2 + bias);  w = the two f16 terms of W * 2^wscale_log2 as [term 2][K step 10][K half 2][co 64][8],
 *   K = (c*7 + ky)*7 + kx zero-padded to 160; bias [64] or NULL; relu 0 / 1. */
E4S_API int e4s_conv7x7s2_stem_f16x3(float* out, const float* x, const void* w, const float* bias, int bs, int h, int wd, int relu, int wscale_log2, void* stream);

/* labels[bs,oh,ow] (uint8) = lut[ argmax_c bilinear_align_corners(logits[bs,ncls,ih,iw]) ] — fuses F.interpolate(..., align_corners=True)
 * (face_parsing/model.py:257), torch.argmax (face_parsing_demo.py:170) and, through the optional 256-entry lut, the 19->12 remap
 * (datasets/dataset.py:58-108).  First maximum wins ties. */
E4S_API int e4s_bilinear_argmax(uint8_t* labels, const float* logits, const uint8_t* lut, int bs, int ncls, int ih, int iw, int oh, int ow,
                                void* stream);

/* BicubicDownSample(factor) + clamp(0,1) + (x-mean)/std of FaceParser.preprocess_img (face_parsing_demo.py:46-84, 151-156):
 * in [bs,C,h,w] in [0,1] -> out [bs,C,h/factor,w/factor]; taps = the 4*factor normalised 1-D weights; mean/std [C] or NULL
 * (NULL: plain down-sample, no clamp).  factor 2 or 4; factor 1 = clamp + normalise only (taps ignored). */
E4S_API int e4s_bicubic_down_normalize(float* out, const float* in, const float* taps, const float* mean, const float* stdv,
                                       int bs, int C, int h, int w, int factor, void* stream);
/* The same on an image in [-1, 1] (what the swap pipeline holds): the [0, 1] image the parser is given there
 * (face_swap_video_pipeline.py:217-219: PIL frames -> ToTensor, face_parsing_demo.py:151-156) is (v + 1) * 0.5, applied on load — value for value
 * what ``e4s_bicubic_down_normalize`` computes from ``(img + 1) / 2``.  factor 2 or 4. */
E4S_API int e4s_bicubic_down_normalize_pm1(float* out, const float* in, const float* taps, const float* mean, const float* stdv,
                                           int bs, int C, int h, int w, int factor, void* stream);

/* tensor2im (utils/torch_utils.py:64-76): img [bs,3,h,w] in ~[-1,1] -> uint8 [bs,h,w,3] = trunc(clamp((x+1)/2, 0, 1) * 255). */
E4S_API int e4s_tensor2im_u8(uint8_t* out, const float* img, int bs, int h, int w, void* stream);

/* ---- f2 / f3: mask surgery between face parsing and synthesis (integer maps, exact) --------------------------------------------
 * e4s_swap_head_mask: swap_head_mask_hole_first(source, target) (swap_face_fine/swap_face_mask.py:194-333) for a batch.
 *   source, target : uint8 [bs, h, w] 12-class maps (driven face, target face)
 *   res            : uint8 [bs, h, w] swapped map;  hole_mask : uint8 {0,1};  hole_map : res with 17 on the hole
 *   lines          : int32 [bs, 2] = (eye_line, nose_line) as computed at :232-239
 *   scratch        : int32 [bs * (3 + w)] work buffer
 * e4s_foreground_masks: foreground = not {0, 11, 7, 4, 8} or hole (face_swap_video_pipeline.py:456-461), then
 *   create_masks(foreground, 'expansion', radius) (gradio_utils/face_swapping.py:203-221; flat (2r+1)^2 dilation / erosion with the
 *   'geodesic' border of utils/morphology.py): content = foreground, full = dilation, border = clip(dilation - erosion, 0, 1).
 *   content (may be NULL), border, full : float32 [bs, 1, h, w] in {0, 1};  hole_mask may be NULL. */
E4S_API int e4s_swap_head_mask(uint8_t* res, uint8_t* hole_mask, uint8_t* hole_map, int32_t* lines, const uint8_t* source,
                               const uint8_t* target, int32_t* scratch, int bs, int h, int w, void* stream);
/* One pass of Pillow's 8-bit image resampler (PIL.Image.resize, src/libImaging/Resample.c) — the reference softens every swapped face with
 * `.resize((512, 512)).resize((1024, 1024))` (face_swap_video_pipeline.py:447, default filter BICUBIC) — on uint8 [bs, h, w, c] images:
 * along axis 1 (width) or 0 (height), out[o] = clip8((2^21 + sum_{j < count[o]} coeffs[o*ksize + j] * in[xmin[o] + j]) >> 22).
 * The tables are Pillow's precompute_coeffs + normalize_coeffs_8bpc (22-bit fixed point), computed by the host (ops.pil_resize). */
E4S_API int e4s_resample_u8(uint8_t* out, const uint8_t* in, const int32_t* xmin, const int32_t* count, const int32_t* coeffs, int ksize,
                            int bs, int h, int w, int c, int out_size, int axis, void* stream);
/* The two pyramid steps of the multi-band blend (swap_face_fine/multi_band_blending.py:5-48; cv2.pyrDown / cv2.pyrUp, OpenCV
 * modules/imgproc/src/pyramids.cpp) on float planes [planes, h, w]:
 *   e4s_pyr_down : out [planes, (h+1)/2, (w+1)/2] = 5x5 kernel [1 4 6 4 1]^2 / 256 at the even pixels, BORDER_REFLECT_101;
 *                  round_u8 != 0 = the 8-bit variant's rounding, floor((sum + 128) / 256) (the reference's pyramid of the uint8 frame)
 *   e4s_pyr_up   : out [planes, 2h, 2w] = up(in), or minuend - up(in) (a Laplacian level), or up(in) + addend (reconstruction);
 *                  up = zero insertion convolved with 4x the same kernel (OpenCV's border rule for the last source pixel) */
E4S_API int e4s_pyr_down(float* out, const float* in, int planes, int h, int w, int round_u8, void* stream);
E4S_API int e4s_pyr_up(float* out, const float* in, const float* minuend, const float* addend, int planes, int h, int w, void* stream);
/* One level of the blend (multi_band_blending.py:27-46) in one pass over [planes, 2h, 2w]: with la = a_hi - up(a_lo), lb = b_hi - up(b_lo),
 * out = up(prev) + la*m_hi + lb*(1 - m_hi);  *_lo and prev are [planes, h, w], *_hi [planes, 2h, 2w]. */
E4S_API int e4s_pyr_blend_level(float* out, const float* prev, const float* a_hi, const float* a_lo, const float* b_hi, const float* b_lo,
                                const float* m_hi, int planes, int h, int w, void* stream);
/* uint8 frames [bs, h, w, 3] -> the network's input [bs, 3, h, w] = (x / 255 - 0.5) / 0.5: transforms.Compose([ToTensor(), Normalize(.5, .5)])
 * of datasets/dataset.py:32, 45 as used at face_swap_video_pipeline.py:338-339 (float32, true division like torchvision). */
E4S_API int e4s_frames_to_tensor(float* out, const uint8_t* frames_u8, int bs, int h, int w, void* stream);
/* erode_mask(mask, img, radius) of the PTI loop (training/video_swap_ft_coach.py:64-93) on uint8 [bs, h, w] 12-class maps: the face mask
 * (every class whose bit is NOT set in bg_class_bits; the reference's background set {0, 4, 11} = 0x811) is eroded with a (2r+1)^2 box,
 * pixels outside the image counting as not-face (cv2.erode, BORDER_CONSTANT 0); out = label where the eroded mask holds, 0 elsewhere. */
E4S_API int e4s_erode_labels(uint8_t* out, const uint8_t* labels, int bs, int h, int w, int radius, unsigned bg_class_bits, void* stream);
E4S_API int e4s_foreground_masks(float* content, float* border, float* full, const uint8_t* swapped, const uint8_t* hole_mask,
                                 int bs, int h, int w, int radius, void* stream);

/* ---- f6: the two-image caller's paste-back (Face_swap_with_two_imgs.py:159-219, 775-794, 909-924): soft paste masks and uint8 blends ------
 * e4s_soft_erosion: SoftErosion.forward (utils/paste_back_tricks.py:17-43) for `planes` independent float32 planes [planes, h, w]:
 *   (iterations - 1) x  x = min(x, conv(x));  c = conv(x)  (kernel_size^2 cone weights, zero padding kernel_size / 2);
 *   hard = c >= threshold (uint8 {0,1}; may be NULL);  soft = 1 where hard, else c / max(c over the not-hard pixels of THIS plane).
 *   weights_t : float32 [kernel_size, kernel_size], the module's `weight` buffer TRANSPOSED (weights_t[kx][ky]), built on the host exactly as the
 *               constructor builds it ((dist.max() - dist) / sum in float32)
 *   scratch   : e4s_soft_erosion_scratch_bytes(planes, h, w, iterations) bytes: the per-workgroup partial maxima and, for iterations > 1, the
 *               intermediate planes.  soft must not alias x.
 *   kernel_size odd, 3..33; iterations >= 1.  No host synchronisation (capturable); the maximum is reduced in a fixed order and holds for any finite input.
 *   Where the reference misbehaves: a plane in which every pixel passes the threshold is all ones (the reference raises on max() of an empty
 *   tensor); a plane whose below-threshold maximum is 0 (an all-zero mask) gives 0 at those pixels (the reference: 0 / 0 = NaN).
 * e4s_blend_u8: Trick.blending_two_images_with_mask (:131-147): out = trunc(clamp(bottom * (1 - m) + up * m, 0, 255)), m = nan_to_0(mask) * up_ratio,
 *   in float32 with every product and sum rounded on its own (numpy's arithmetic).  bottom, up, out: uint8 [n, h, w, 3]; mask: float32
 *   [n, mask_channels, h, w], mask_channels 1 or 3; up_ratio in [0, 1].  With bottom = T, up = swapped, up_ratio = 1 it is the crop paste
 *   np.uint8(swapped * content + T * (1 - content)) of Face_swap_with_two_imgs.py:216-217. */
E4S_API int e4s_soft_erosion_scratch_bytes(int planes, int h, int w, int iterations, int64_t* bytes);
E4S_API int e4s_soft_erosion(float* soft, uint8_t* hard, const float* x, const float* weights_t, float* scratch, int planes, int h, int w,
                             int kernel_size, float threshold, int iterations, void* stream);
E4S_API int e4s_blend_u8(uint8_t* out, const uint8_t* bottom, const uint8_t* up, const float* mask, float up_ratio, int n, int h, int w,
                         int mask_channels, void* stream);

/* ---- f5: crop-align of a video frame and the paste back into it (utils/alignment.py:101-147 crop_image; face_swap_video_pipeline.py:181-210,
 * 474-483).  Pillow's Image.transform(..., BILINEAR) on uint8 RGB, bit for bit (src/libImaging/Geometry.c): output pixel (x, y) is sampled at
 * (x + 0.5, y + 0.5) mapped through the transform in plain double arithmetic; a sample outside the source window is not taken; otherwise the
 * bilinear blend of the four neighbours (columns and the first row clamped to the window, the second row used only inside it) is truncated to
 * 8 bits.  The coefficients are `const void*` = double[n][8] in DEVICE memory (e4s2024_amd/align.py builds them).  The boxes are HOST
 * int32[n][4] = (x0, y0, x1, y1), checked against the frame before anything is launched; they size the launches (one per 32 frames).
 *   e4s_warp_quad_u8              : out uint8 [n, size, size, 3] = Image.transform((size, size), QUAD, data, BILINEAR) of the window
 *                                   `windows[i]` of frames uint8 [n, h, w, 3] (the crop box; Pillow's image.crop(box)); unsampled pixels 0.
 *                                   xi = a0 + a1 x + a2 y + a3 x y,  yi = a4 + a5 x + a6 y + a7 x y.
 *   e4s_warp_perspective_paste_u8 : faces uint8 [n, size, size, 3] pasted IN PLACE into frames uint8 [n, h, w, 3]: every frame pixel of
 *                                   boxes[i] that samples the face under PERSPECTIVE data gets the sample, every other pixel is left alone
 *                                   (= transform to RGBA + alpha_composite onto the frame).  xi = (a0 x + a1 y + a2) / (a6 x + a7 y + 1),
 *                                   yi = (a3 x + a4 y + a5) / (a6 x + a7 y + 1). */
E4S_API int e4s_warp_quad_u8(uint8_t* out, const uint8_t* frames, const int32_t* windows, const void* coeffs, int n, int h, int w, int size,
                             void* stream);
E4S_API int e4s_warp_perspective_paste_u8(uint8_t* frames, const uint8_t* faces, const int32_t* boxes, const void* coeffs, int n, int h, int w,
                                          int size, void* stream);

/* ---- f1: gradients of the one-pass region-modulated convolution (PTI tuning, training/video_swap_ft_coach.py:242-299) -----------
 *     z[b,o,p] = sum_{i,k} W[o,i,k] * s[b,c(p),i] * x[b,i,p+k-pad],   y = d[b,c(p),o] * z        (model.py:389-398, 447-454)
 *     out = leaky_relu(y + noise_weight*noise + act_bias, 0.2) * sqrt(2)                          (model.py:335, 421)
 * The two GEMMs of the backward (U_g = W_g^T gz_g, dW_g = gz_g cols_g^T) are library fp32 GEMMs on the host side; these are the passes
 * around them.  x [bs,cin,h,w], s [bs,nreg,cin], d [bs,nreg,cout] (NULL = no demodulation), ks 1 or 3 (pad ks/2, stride 1).
 * up = 1: labels uint8 [bs,h,w], one group.  up = 2 (the up-sampling layers in their composed form): labels
 * [bs,2h,2w] at the OUTPUT resolution, four groups g = 2a+b, one per output parity: output pixel (2qy+a, 2qx+b) is a 3x3 correlation
 * of x around q with the composed weight W_g under c_g(q) = labels[2qy+a][2qx+b].  A label >= nreg is no region (zero, no gradient).
 *   e4s_mconv_unfold : cols[G, bs, cin*ks*ks, h*w] = s[c_g(q),i] * x[i, q+k-pad]
 *   e4s_mconv_scale  : from gy = dL/d(out) [bs,cout,up*h,up*w] and the forward output `out`:  g' = gy * act'(out);
 *                      gz[G,bs,cout,h*w] = g' * d[c(p),o] (parity-planar);  per pixel chunk (nchunk = ceil(up*h*up*w / chunk_px), the
 *                      caller adds the chunks up): q[nchunk,bs,nreg,cout] = per-region sums of g'*y (dL/dd = q / d),
 *                      dbias[nchunk,bs,cout] = sum g',  dnw[nchunk,bs,cout] = sum g'*noise.  q, dbias, dnw, out, noise, act_bias optional;
 *                      with act = 0 and no noise / bias, `out` is y itself.  noise [noise_bs, up*h*up*w], noise_bs 1 or bs.
 *   labels NULL (all three) = one region, every pixel is region 0: the single-region layers of the generator (nreg = 1).
 *   e4s_mconv_fold   : from U[G, bs, cin*ks*ks, h*w]:  dx[b,i,t] = sum_g sum_k s[c_g(t-k+pad),i] * U[g,b,(i,k),t-k+pad]  (may be NULL)
 *                      ds_part[nchunk, bs, nreg, cin] = per pixel-chunk partial sums of sum_g sum_k U[g,b,(i,k),q] * x[i,q+k-pad] over
 *                      each region's pixels (may be NULL), nchunk = ceil(h*w / chunk_px); dL/ds = ds_part.sum(0) */
/* Gradient of a layer's style tables (EqualLinear modulation + demodulation, model.py:150-161, 276-281, in the one-pass form):
 *     s = styles (mod_w*mod_scale)^T + mod_b*mod_lr,   ws = weight_scale*weight,   d = rsqrt(s^2 wsq + 1e-8),  wsq[i,o] = sum_k ws[o,i,k]^2 ([cin,cout], as e4s_modconv_prep_weights writes it)
 * gs [rows,cin], gd [rows,cout], gws [cout,cin,kk] = dL/ds, dL/dd, dL/dws (each may be NULL; gd needs d and wsq), rows = bs*nreg.
 * Outputs: g_styles [rows,sdim], g_mod_w [cin,sdim], g_mod_b [cin] (written when gs or gd is given), g_weight [cout,cin,kk] w.r.t. the
 * unscaled weight (written when gws or gd is given).  scratch: rows*(cout+cin) floats. */
E4S_API int e4s_style_tables_bwd(float* g_styles, float* g_mod_w, float* g_mod_b, float* g_weight, float* scratch, const float* gs,
                                 const float* gd, const float* gws, const float* styles, const float* mod_w, const float* s, const float* d,
                                 const float* weight, const float* wsq, float weight_scale, float mod_scale, float mod_lr, int rows, int sdim,
                                 int cin, int cout, int kk, void* stream);
E4S_API int e4s_mconv_unfold(float* cols, const float* x, const float* s, const uint8_t* labels, int bs, int cin, int h, int w, int ks,
                             int nreg, int up, void* stream);
E4S_API int e4s_mconv_scale(float* gz, float* q, float* dbias, float* dnw, const float* gy, const float* out, const float* d,
                            const uint8_t* labels, const float* noise, int noise_bs, const float* noise_weight, const float* act_bias,
                            int act, int bs, int cout, int h, int w, int nreg, int up, int chunk_px, void* stream);
/* cols[bs, C*ks*ks, ho*wo] = x[bs, C, stride*qy + ky - pad, stride*qx + kx - pad] (0 outside): the unfolded operand of a plain convolution's
 * weight gradient as a library GEMM — the single-region layers past remaining_layer_idx (conv: dW = g' cols(x)^T, stride 1 pad 1;
 * transposed conv, model.py:296-306: dW = x cols(gT)^T with stride 2 pad 0). */
E4S_API int e4s_unfold2d(float* cols, const float* x, int bs, int C, int hi, int wi, int ho, int wo, int ks, int stride, int pad, void* stream);
E4S_API int e4s_mconv_fold(float* dx, float* ds_part, const float* U, const float* x, const float* s, const uint8_t* labels, int bs, int cin,
                           int h, int w, int ks, int nreg, int up, int chunk_px, void* stream);


/* The contractions of the backward (f1) — replaces the library GEMMs (torch.matmul) behind the reference's autograd of
 * ModulatedConv2d (models/stylegan2/model.py:276-320 differentiated by PyTorch; training/video_swap_ft_coach.py:268-299 is the loop):
 *   C[b] (M x N, row-major, dense [batch][M][N] at stride_c) = opA(A[b]) (M x K) * opB(B[b]) (K x N),  fp32 in / out,
 * each product as three bf16 MFMAs (hi*hi + hi*lo + lo*hi, fp32 accumulation).  a_kc != 0: A is stored [M][K] with row stride lda,
 * else [K][M]; b_kc != 0: B is stored [N][K] with row stride ldb, else [K][N].  K-contiguous operands need 16-byte aligned rows and
 * K % 4 == 0.  Batch strides in floats (0 = one matrix for all b).  workspace (may be NULL): scratch of workspace_floats floats for
 * the split of a long K over workgroups; partial sums are added in a fixed order. */
E4S_API int e4s_gemm_sb(float* c, const float* a, const float* b, int M, int N, int K, int a_kc, int b_kc, int lda, int ldb, int64_t stride_a,
                        int64_t stride_b, int64_t stride_c, int batch, float* workspace, int64_t workspace_floats, void* stream);

/* Weight gradient of the (masked) modulated convolution as one implicit GEMM — the modulated im2col operand of e4s_mconv_unfold is produced
 * while it is staged, never stored:  dW[g][b][co][(ci, k)] = sum_p gz[g][b][co][p] * s[b][c_g(p)][ci] * x[b][ci][p + k - pad],
 * g < up * up (composed weights of the four output parities for up = 2, labels at the output resolution).  s == NULL: no modulation;
 * labels == NULL: one region.  dw: dense [up * up * bs][cout][cin * ks * ks].  w % 16 == 0.  workspace as for e4s_gemm_sb. */
E4S_API int e4s_mconv_wgrad(float* dw, const float* gz, const float* x, const float* s, const uint8_t* labels, int bs, int cin, int cout, int h,
                            int w, int ks, int nreg, int up, float* workspace, int64_t workspace_floats, void* stream);

/* Data and style gradient of the masked modulated 3x3 convolution in one kernel — e4s_gemm_sb (U = W^T gz) + e4s_mconv_fold without U in memory
 * (same reference path: autograd through ModulatedConv2d.forward, models/stylegan2/model.py:276-320):
 *     dx[b,i,q]            = sum_g sum_k s[b,c_g(q-k+1),i] * sum_o wg[g,o,i,k] * gz[g,b,o,q-k+1]               (may be NULL)
 *     ds_part[t,b,r,i]     = tile t's part of sum_g sum_{p: c_g(p) = r} sum_k (sum_o wg[g,o,i,k] gz[g,b,o,p]) * x[b,i,p+k-1]   (may be NULL)
 * gz [up*up, bs, cout, h*w] (e4s_mconv_scale), wg [up*up, cout, cin, 3, 3] fp32, labels as for e4s_mconv_fold (NULL = one region), w >= 32.
 * t < e4s_mconv_dgrad_tiles(h, w); dL/ds = ds_part.sum(0).  Every product as three bf16 MFMAs with fp32 accumulation; sums in a fixed order. */
E4S_API int e4s_mconv_dgrad_tiles(int h, int w);
E4S_API int e4s_mconv_dgrad(float* dx, float* ds_part, const float* gz, const float* wg, const float* x, const float* s, const uint8_t* labels,
                            int bs, int cin, int cout, int h, int w, int nreg, int up, void* stream);

/* Winograd F(2x2, 3x3) pieces around e4s_gemm_sb(batch = 16) for stride-1, pad-1 3x3 convolutions (the regional-style encoder's IR-SE units,
 * models/encoders/helpers.py:122-144: Conv2d(c, d, 3, 1, 1) after InstanceNorm2d / before PReLU):
 *   e4s_wino_weight : U[16][cout][cin] = G g G^T of w [cout][cin][3][3]
 *   e4s_wino_input  : V[16][C][T]      = B^T d B of every 4x4 patch (stride 2) of x [bs][C][H][W], T = bs * H/2 * W/2, tile t = (b * H/2 + ty) * W/2 + tx;
 *                     mean / rstd [bs][C] (both or neither): the patch is taken from (x - mean) * rstd, zero beyond the border
 *   then M[k] (cout x T) = U[k] (cout x cin) * V[k] (cin x T) for k < 16 — e4s_gemm_sb(M, U, V, cout, T, cin, 1, 0, cin, T, cout*cin, cin*T, cout*T, 16, ...)
 *   e4s_wino_output : y [bs][cout][H][W] = act(A^T m A) of m = M[.][co][t]; prelu [cout] or NULL (no activation)
 * H, W even. */
E4S_API int e4s_wino_weight(float* U, const float* w, int cout, int cin, void* stream);
E4S_API int e4s_wino_input(float* V, const float* x, const float* mean, const float* rstd, int bs, int C, int H, int W, void* stream);
E4S_API int e4s_wino_output(float* y, const float* M, const float* prelu, int bs, int cout, int H, int W, void* stream);

/* LPIPS-AlexNet (criteria/lpips; csrc/lpips.hip) — forward and input gradient; conv2 - conv5 run on e4s_conv2d_sb3 (forward) and e4s_conv2d_sb (data
 * gradient on the flipped, transposed weights; 5x5 stride 1 is supported there for conv2).  All tensors fp32 NCHW on the device.
 *   e4s_lpips_conv1        : out [bs][64][ho][wo] = relu(conv(z, w, stride 4, pad 2) + bias), z = (boxmean_f(x) - mean[c]) / std[c], x [bs][3][h][w],
 *                            f in {1, 2, 4} dividing h and w, ho = (h / f - 7) / 4 + 1; wt [3][11][11][64] (the weight [64][3][11][11] with co innermost)
 *   e4s_lpips_conv1_dgrad  : gx [bs][3][h][w] = d/dx of sum(g1 * conv1 pre-activation) (g1 already ReLU-masked), the box mean's backward included (written)
 *   e4s_lpips_maxpool      : MaxPool2d(3, 2), no padding, over planes of h x w (h, w >= 3)
 *   e4s_lpips_maxpool_bwd_relu : g [planes][h][w] = (add + gather of gpool over the windows whose first maximum is the pixel) * (a > 0); add may be NULL
 *   e4s_lpips_head         : partial[b * ceil(hw / 32) + i] = scale * (32-pixel block i's sum over pixels of sum_c lin[c] (fx / |fx| - fy / |fy|)^2),
 *                            |f| = sqrt(sum_c f^2 + 1e-16) + 1e-10; fx, fy [bs][c][hw]
 *   e4s_lpips_sum          : loss[0] = sum of partial[0 .. n) in a fixed order (one workgroup)
 *   e4s_lpips_head_bwd     : gx (and gy unless NULL) = d/dfx (d/dfy) of gout[0] * scale * sum over pixels of the same quantity
 *   e4s_lpips_relu_mask    : g[i] = 0 where a[i] <= 0
 * No float atomics: the same inputs give the same bits. */
E4S_API int e4s_lpips_conv1(float* out, const float* x, const float* mean, const float* std, const float* wt, const float* bias, int bs, int h, int w,
                            int f, void* stream);
E4S_API int e4s_lpips_conv1_dgrad(float* gx, const float* g1, const float* std, const float* wt, int bs, int h, int w, int f, void* stream);
E4S_API int e4s_lpips_maxpool(float* out, const float* a, int planes, int h, int w, void* stream);
E4S_API int e4s_lpips_maxpool_bwd_relu(float* g, const float* gpool, const float* add, const float* a, int planes, int h, int w, void* stream);
E4S_API int e4s_lpips_head(float* partial, const float* fx, const float* fy, const float* lin, int bs, int c, int hw, float scale, void* stream);
E4S_API int e4s_lpips_sum(float* loss, const float* partial, int n, void* stream);
E4S_API int e4s_lpips_head_bwd(float* gx, float* gy, const float* fx, const float* fy, const float* lin, const float* gout, int bs, int c, int hw,
                               float scale, void* stream);
E4S_API int e4s_lpips_relu_mask(float* g, const float* a, int64_t n, void* stream);

/* ArcFace IR-SE50 identity loss (criteria/id_loss.py; csrc/idloss.hip) — forward and input gradient.  The convolutions run on e4s_conv2d_sb3 (forward)
 * and e4s_conv2d_sb (stride-1 data gradients on flipped, transposed weights); the stride-2 3x3 data gradient on e4s_modconv_tconv_sb (s = 1, the weight
 * pre-scaled by sqrt(9 cin)).  All tensors fp32 NCHW on the device.
 *   e4s_id_resample         : out [planes][no][no] = A_y x A_x^T, x [planes][h][w], ay [no][h], ax [no][w]; ry [no][2], rx [no][2] = [lo, hi) of each row's band
 *   e4s_id_resample_adjoint : gx [planes][h][w] (+)= A_y^T g A_x; cy [h][2], cx [w][2] = [lo, hi) of each column's band (empty: 0)
 *   e4s_id_affine           : out = x * scale[c] + shift[c] (scale, shift NULL: x), then PReLU with slope[c] unless slope is NULL; x [bs][C][hw]
 *   e4s_id_prelu_bwd        : g [bs][C][h][w] = src[bs][C][y + off][x + off] (planes sh x sw) * (pre > 0 ? 1 : slope[c])
 *   e4s_id_se_bwd           : SEModule backward for r * gate: s = sum_hw g r, v = fc1^T ((fc1 pooled > 0) fc2^T (s gate (1 - gate))) / hw, dr = g gate + v;
 *                             s, v [bs][C] scratch; fc1 [H][C], fc2 [C][H]; C <= 1024, H <= 64
 *   e4s_id_scatter_add      : gx [planes][h][w] at (2y, 2x) += src [planes][(h + 1) / 2][(w + 1) / 2]
 *   e4s_id_linear           : y [bs][N] = x [bs][K] W^T + bias (bias may be NULL); W [N][K]
 *   e4s_id_linear_t         : gx [bs][K] = g [bs][N] W
 *   e4s_id_head_partial     : part [bs][ceil(D / 8192)][3] = block sums of fx^2, fy^2, fx fy; fx, fy [bs][D]
 *   e4s_id_head_sum         : over taps t < ntap (partials concatenated in tap order, nb_t blocks each): stats [ntap][bs][3] = (|x|, |y|, cos),
 *                             loss[0] = sum_t mean_b (1 - cos), sim[0] = sum_t mean_b (cos - |y|^2 / (|y| |y|))
 *   e4s_id_head_bwd         : gx [bs][D] (+)= -gout[0] scale (fy / |y| - cos fx / |x|) / |x| with the stats of the tap
 * No float atomics: the same inputs give the same bits. */
E4S_API int e4s_id_resample(float* out, const float* x, const float* ay, const float* ax, const int* ry, const int* rx, int planes, int h, int w, int no,
                            void* stream);
E4S_API int e4s_id_resample_adjoint(float* gx, const float* g, const float* ay, const float* ax, const int* cy, const int* cx, int planes, int h, int w,
                                    int no, int accumulate, void* stream);
E4S_API int e4s_id_affine(float* out, const float* x, const float* scale, const float* shift, const float* slope, int bs, int C, int hw, void* stream);
E4S_API int e4s_id_prelu_bwd(float* g, const float* src, const float* pre, const float* slope, int bs, int C, int h, int w, int sh, int sw, int off,
                             void* stream);
E4S_API int e4s_id_se_bwd(float* dr, float* s, float* v, const float* g, const float* r, const float* pooled, const float* gate, const float* fc1,
                          const float* fc2, int bs, int C, int H, int hw, void* stream);
E4S_API int e4s_id_scatter_add(float* gx, const float* src, int planes, int h, int w, void* stream);
E4S_API int e4s_id_linear(float* y, const float* x, const float* W, const float* bias, int bs, int K, int N, void* stream);
E4S_API int e4s_id_linear_t(float* gx, const float* g, const float* W, int bs, int K, int N, void* stream);
E4S_API int e4s_id_head_partial(float* part, const float* fx, const float* fy, int bs, int64_t D, void* stream);
E4S_API int e4s_id_head_sum(float* loss, float* sim, float* stats, const float* part, int bs, int ntap, int nb0, int nb1, int nb2, int nb3, int nb4,
                            void* stream);
E4S_API int e4s_id_head_bwd(float* gx, const float* fx, const float* fy, const float* stats, const float* gout, int bs, int64_t D, float scale,
                            int accumulate, void* stream);

/* Face-parsing feature loss (criteria/face_parsing/face_parsing_loss.py on the unet encoder; csrc/fploss.hip) — forward and input gradient.  The input
 * pooling and its adjoint run on e4s_id_resample(_adjoint) (no = 512), the heads on e4s_id_head_partial / e4s_id_head_sum, the convolutions on
 * e4s_conv2d (3 input channels, fp32), e4s_conv2d_sb3 (forward) and e4s_conv2d_sb (data gradients); the first convolution's ReLU mask on
 * e4s_lpips_relu_mask.  All tensors fp32 NCHW on the device.
 *   e4s_fp_maxpool2 : out [planes][h / 2][w / 2] = MaxPool2d(2) of a [planes][h][w] (h, w even; a 8-byte aligned)
 *   e4s_fp_tap_bwd  : g [bs][C][h][w] = (-gout[0] scale (fy / |y| - cos fx / |x|) / |x| + gpool routed to the first maximum (row-major) of each 2 x 2
 *                     window of fx) * (fx > 0); fx, fy [bs][C][h][w] the block output (ReLU'd) of y_hat and y, stats [bs][3] = (|x|, |y|, cos) of
 *                     the tap (e4s_id_head_sum), gpool [bs][C][h / 2][w / 2] the gradient of the next block's input or NULL (h, w even; g, fx, fy
 *                     8-byte aligned)
 * No float atomics: the same inputs give the same bits. */
E4S_API int e4s_fp_maxpool2(float* out, const float* a, int planes, int h, int w, void* stream);
E4S_API int e4s_fp_tap_bwd(float* g, const float* fx, const float* fy, const float* stats, const float* gout, const float* gpool, int bs, int C, int h,
                           int w, float scale, void* stream);

/* Multi-target loss heads (csrc/lpips.hip, idloss.hip, fploss.hip, pixloss.hip): one reconstruction against k (1 .. E4S_MAX_TARGETS) targets, target j weighted by tw[j]
 * — the driven and the recoloured frame of the PTI objective share the reconstruction's forward pass and input gradient.  ys [k] and tw [k] are HOST
 * arrays (device pointers, weights), read at the call.  Target j of sample b starts at ys[j] + f * fstride + b * (per-sample size) with f = *frame (a
 * device int32, e.g. written before a graph replay to pick a frame of a clip-wide feature cache, clamped to [0, nframes)), or f = 0 when frame is NULL.
 *   e4s_lpips_head_multi      : partial [bs][ceil(hw / 32)] as e4s_lpips_head, the per-pixel distance summed over the targets with their weights
 *   e4s_lpips_head_multi_bwd  : gx [bs][c][hw] = d/dfx of that sum times gout[0] (no target gradient)
 *   e4s_id_head_partial_multi : part [bs][ceil(D / 8192)][9] = block sums of fx^2, then (fy_j^2, fx fy_j) per target (unused targets 0)
 *   e4s_id_head_sum_multi     : stats [ntap][bs][9] = |x|, then (|y_j|, cos_j); loss[0] = sum_t sum_j tw[j] mean_b (1 - cos_j)
 *   e4s_id_head_bwd_multi     : gx [bs][D] (+)= -gout[0] scale sum_j tw[j] (fy_j / |y_j| - cos_j fx / |x|) / |x|
 *   e4s_fp_tap_bwd_multi      : e4s_fp_tap_bwd with that summed head gradient; stats [bs][9] of the tap (targets 8-byte aligned, fstride even)
 *   e4s_pix_mse_multi         : partial [bs C][ceil(hw / 4096)], summing (e4s_lpips_sum) to sum_j tw[j] mean((x fg - y_j)^2); x, y_j [bs][C][hw], the
 *                               targets already weighted (y fg), fg [bs][1][hw] or NULL (1); bs C <= 65535
 *   e4s_pix_mse_multi_bwd     : gx [bs][C][hw] = gout[0] 2 / (bs C hw) sum_j tw[j] (x fg - y_j) fg
 * No float atomics: the same inputs give the same bits; k = 1 with weight 1 gives the single-target heads' values. */
#define E4S_MAX_TARGETS 4
E4S_API int e4s_lpips_head_multi(float* partial, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                 const float* lin, int bs, int c, int hw, float scale, void* stream);
E4S_API int e4s_lpips_head_multi_bwd(float* gx, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                     const float* lin, const float* gout, int bs, int c, int hw, float scale, void* stream);
E4S_API int e4s_id_head_partial_multi(float* part, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                      int bs, int64_t D, void* stream);
E4S_API int e4s_id_head_sum_multi(float* loss, float* stats, const float* part, const float* tw, int k, int bs, int ntap, int nb0, int nb1, int nb2,
                                  int nb3, int nb4, void* stream);
E4S_API int e4s_id_head_bwd_multi(float* gx, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                  const float* stats, const float* gout, int bs, int64_t D, float scale, int accumulate, void* stream);
E4S_API int e4s_fp_tap_bwd_multi(float* g, const float* fx, const float* const* ys, const float* tw, int k, const int* frame, int64_t fstride, int nframes,
                                 const float* stats, const float* gout, const float* gpool, int bs, int C, int h, int w, float scale, void* stream);
E4S_API int e4s_pix_mse_multi(float* partial, const float* x, const float* fg, const float* const* ys, const float* tw, int k, const int* frame,
                              int64_t fstride, int nframes, int bs, int C, int64_t hw, void* stream);
E4S_API int e4s_pix_mse_multi_bwd(float* gx, const float* x, const float* fg, const float* const* ys, const float* tw, int k, const int* frame,
                                  int64_t fstride, int nframes, const float* gout, int bs, int C, int64_t hw, void* stream);

/* f7: the two-image caller's skin colour transfer for ct_mode 'lct' / 'mkl' (Face_swap_with_two_imgs.py:537-572, swap_face_fine/color_transfer.py:218-246,
 * 345-381, utils/morphology.py:23-198; csrc/colortransfer.hip).
 *   e4s_grey_morph   : out [planes][h][w] = flat (2 radius + 1)^2 maximum (op 0, dilation) or minimum (op 1, erosion) of x, pixels outside the image ignored
 *                      (the 'geodesic' border); radius 0 .. 16, 0 = a copy; any h, w >= 1.  Exact.  out must not alias x.
 *   e4s_ct_moments   : partial [bs][nchunk][9] doubles = per pixel chunk the sums of v_0, v_1, v_2, v_0 v_0, v_0 v_1, v_0 v_2, v_1 v_1, v_1 v_2, v_2 v_2 with
 *                      v_c = (float(frame[b][p][c]) * mask[b][p]) / 255.0f in float32 (a true division); frame uint8 [bs][h][w][3], mask float [bs][1][h][w];
 *                      nchunk = ceil(h w / 4096).  e4s_ct_moments_scratch_bytes: the size of `partial` for one call.
 *   e4s_ct_solve     : coef [bs][15] doubles = (A row-major [3][3], mu_src [3], mu_trg [3]) from the two partial buffers, summed in a fixed order:
 *                      mode 0 (lct, 'pca'):  C = cov / N + 1e-5 I,  A = sqrtm(C_trg) inv(sqrtm(C_src))
 *                      mode 1 (mkl):         a, b = cov / (N - 1) of src, trg, eigenvalues clipped to DBL_EPSILON,
 *                                            A^T = a^-1/2 (a^1/2 b a^1/2)^1/2 a^-1/2
 *                      by cyclic Jacobi sweeps in float64, so that y = A (v - mu_src) + mu_trg.  One wave per image, no host round trip.
 *   e4s_ct_apply     : per pixel and channel v as above, y in float64 rounded to float32 and clipped to [0, 1], q = trunc(y * 255.0f);
 *                      composed [bs][3][h][w] = float(frame) * (1 - mask) + float(q) * mask in float32 without contraction; q_u8 [bs][h][w][3] or NULL.
 * partial and coef hold doubles (8-byte aligned; void* in this header).  No float atomics: the same inputs give the same bits. */
E4S_API int e4s_grey_morph(float* out, const float* x, int planes, int h, int w, int radius, int op, void* stream);
E4S_API int e4s_ct_moments_scratch_bytes(int bs, int h, int w, int64_t* bytes);
E4S_API int e4s_ct_moments(void* partial, const uint8_t* frame, const float* mask, int bs, int h, int w, void* stream);
E4S_API int e4s_ct_solve(void* coef, const void* partial_src, const void* partial_trg, int bs, int h, int w, int mode, void* stream);
E4S_API int e4s_ct_apply(float* composed, uint8_t* q_u8, const uint8_t* frame, const float* mask, const void* coef, int bs, int h, int w, void* stream);

/* f8: Blender recolouring, stage 1 — the semantic colour reference `get_color_refer` (swap_face_fine/Blender/model_center/semantic_tools.py:50-167) and the
 * reference channels of `Referencer.forward`'s packages (referencer.py:73-81; csrc/colorref.hip).  Nine parts p (skin hair eye nose lip tooth ear brow
 * inpainting); parts_a / parts_t uint8 [bs][9][H][W] 0/1 masks; feats float [bs][256][h][w] with h * w <= 4096; img_t float [bs][3][H][W], ImageNet-normalised.
 * Maps are brought to h x w by the nearest pick floor(i * (float(H) / h)).  Every sample is processed on its own.
 *   e4s_colorref_scratch_bytes : the size of `scratch` (counts, pixel lists, unit rows, rgb_T); 16-byte aligned, shared by the calls below.
 *   e4s_colorref_lists   : per (sample, part) the ascending pixel lists of A and T and their counts; present uint8 [bs][9] = both counts > 0.
 *   e4s_colorref_rows    : per pixel the 256 channels minus their mean, divided by max(norm, 1e-8); rgb_T = clamp(img_t * std + mean, 0, 1);
 *                          inv_target float [bs][3][h][w] = rgb_T * nearest(sum of the nine T masks), or NULL.  D must be 256.
 *   e4s_colorref_attend  : refs float [bs][9][3][h][w] (the caller zeroes it): at A's pixels a of a present part
 *                              sum_t softmax_t(tau c[a][t]) rgb_T[t],  c = the rows' dot product, a T row counting as zero where A's mask of the part is 0
 *                          by an online softmax with a running maximum (any tau); tau is *tau_dev when tau_dev is not NULL (read on the device).
 *                          inv_parts float [bs][9][3][h][w] (zeroed by the caller) or NULL: at T's pixels t, sum_a softmax_a(tau c[a][t]) refs[p][a].
 *   e4s_colorref_sum_parts : inv [bs][3][h][w] = inv_parts summed over the parts in ascending order.
 *   e4s_colorref_package : out float [bs][6][H][W] = bilinear (align_corners) resize of (sum of refs 0..7, refs 8), zero where fewer than two parts are present.
 * No atomics, no host synchronisation; grids depend on the shapes alone: the same inputs give the same bits, and the calls can be captured in a graph. */
E4S_API int e4s_colorref_scratch_bytes(int bs, int h, int w, int64_t* bytes);
E4S_API int e4s_colorref_lists(void* scratch, uint8_t* present, const uint8_t* parts_a, const uint8_t* parts_t, int bs, int H, int W, int h, int w, void* stream);
E4S_API int e4s_colorref_rows(void* scratch, float* inv_target, const float* feats_a, const float* feats_t, const float* img_t, const uint8_t* parts_t,
                              int bs, int D, int H, int W, int h, int w, void* stream);
E4S_API int e4s_colorref_attend(float* refs, float* inv_parts, const void* scratch, float tau, const float* tau_dev, int bs, int h, int w, void* stream);
E4S_API int e4s_colorref_sum_parts(float* inv, const float* inv_parts, int bs, int h, int w, void* stream);
E4S_API int e4s_colorref_package(float* out, const float* refs, const uint8_t* present, int bs, int H, int W, int h, int w, void* stream);

/* f9: Blender recolouring, stage 2 — the glue of the Res-U-Net (swap_face_fine/Blender/model_center/res_u_net.py; csrc/resunet.hip) between its convolutions,
 * which run on e4s_conv2d_sb3.  fp32 NCHW, eval BatchNorm as (scale, shift) per channel.
 *   e4s_resunet_preact        : act [bs][C][hw] = max(x * scale[c] + shift[c], 0), the bn1 -> relu at the head of a ResBlock (x itself feeds the shortcut).
 *                               Not e4s_id_affine with a zero slope: that writes -0.0 for a negative value.
 *   e4s_resunet_up_cat_preact : u = bilinear x2 of low [bs][c_low][h][w] with align_corners (F.upsample_bilinear; e4s_bilinear_resize's float32 coordinates,
 *                               scale (h - 1) / (2h - 1), 0 when h == 1); up [bs][c_low][2h][2w] = u (up may be NULL);
 *                               act [bs][c_low + c_skip][2h][2w] = max(cat(u, skip) * scale[c] + shift[c], 0), skip [bs][c_skip][2h][2w].
 *   e4s_resunet_head          : out [bs][3][hw] = sigmoid(w[3][C] . x[bs][C][hw] + b[3]) with the full-precision exponential; C is 64 or 16.
 * 16-byte accesses along the pixel axis where the pointers (and, for preact / head, hw % 4 == 0) allow, one element per lane otherwise.  No atomics, no host
 * synchronisation, grids depend on the shapes alone: the same inputs give the same bits, and the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_resunet_preact(float* act, const float* x, const float* scale, const float* shift, int bs, int C, int hw, void* stream);
E4S_API int e4s_resunet_up_cat_preact(float* act, float* up, const float* low, const float* skip, const float* scale, const float* shift, int bs, int c_low,
                                      int c_skip, int h, int w, void* stream);
E4S_API int e4s_resunet_head(float* out, const float* x, const float* w, const float* b, int bs, int C, int hw, void* stream);

/* f10: Blender recolouring, stage 3 — the glue of the feature network (swap_face_fine/Blender/model_center/backbone.py, cmodules/architecture.py,
 * cmodules/normalization.py; csrc/spade.hip) between its convolutions, which run on e4s_conv2d_sb3.  That kernel pads with zeros only; the SPADE blocks pad by
 * reflection, so both calls can write reflection-padded planes [C][h + 2][w + 2] (index -1 is 1, index n is n - 2) for a convolution with pad = 0.
 *   e4s_spade_shared   : the first layer of nnorms SPADE norms in one launch.  seg = nearest pick of img [bs][3][H][W] at h x w (F.interpolate mode='nearest':
 *                        floor(dst * (H / h)) in float32, clamped), actv = relu(conv3x3(reflpad1(seg)) + bias) with weight [nnorms * 128][3][3][3] and bias
 *                        [nnorms * 128], written padded as actv [nnorms][bs][128][h + 2][w + 2] (one norm's slice is a contiguous batch).  Each output sums
 *                        bias, then 27 fused multiply-adds in (input channel, row, column) order.  h, w >= 2.
 *   e4s_spade_modulate : out = act((x - mean) * rstd * (1 + gamma) + beta) for x [bs][C][h][w], mean / rstd [bs * C] (e4s_plane_stats), gamma_beta
 *                        [bs][2C][h][w] = gamma | beta (NULL: the plain InstanceNorm (x - mean) * rstd); act = v > 0 ? v : 0.2 v with leaky, identity
 *                        without; out [bs][C][h][w], or with padded [bs][C][h + 2][w + 2] (then h, w >= 2).  Every operation is rounded on its own: the
 *                        difference, the product with rstd, 1 + gamma, the product, the sum, the activation's product.  16-byte loads along a row when
 *                        w % 4 == 0 and the pointers allow, one element per lane otherwise: the same bits.
 * No atomics, no host synchronisation, grids depend on the shapes alone: the same inputs give the same bits, and the calls can be captured in a graph.
 * bs == 0 returns at once. */
E4S_API int e4s_spade_shared(float* actv, const float* img, const float* weight, const float* bias, int bs, int nnorms, int H, int W, int h, int w, void* stream);
E4S_API int e4s_spade_modulate(float* out, const float* x, const float* mean, const float* rstd, const float* gamma_beta, int bs, int C, int h, int w, int leaky,
                               int padded, void* stream);

/* f11: the Real-ESRGAN step of the recolouring (swap_face_fine/realesr/image_infer.py: RealESRBatchInfer around RRDBNet(3, 3, 64, 23, 32, scale=4); csrc/rrdb.hip),
 * the glue between the network's convolutions, which run on e4s_conv2d_sb3.
 *   e4s_esr_input     : uint8 img [bs][H][W][3] -> out [bs][3][oh][ow]: u = clamp((v / 127.5 - 1) * 0.5 + 0.5, 0, 1) per colour value, every operation rounded on
 *                       its own ("/ 127.5" as PyTorch divides by a host scalar on the device: times the float32 reciprocal), then the align_corners=True bilinear
 *                       pick with e4s_bilinear_resize's coordinates and blend.
 *   e4s_esr_scale_add : y [planes][hw] = t * 0.2 + x, the product rounded, then the sum (PyTorch's t * 0.2 + x bit for bit).  y may be x or t.
 *   e4s_esr_up2       : out [planes][2h][2w] = in [planes][h][w] at (y >> 1, x >> 1): F.interpolate(scale_factor=2, mode='nearest').
 *   e4s_esr_tail      : r = conv3x3(x [bs][64][H][W], weight [3][64][3][3], zero pad 1) + bias [3] in exact float32: each sum is bias, then 576 fused
 *                       multiply-adds in (input channel, row, column) order.  out_u8 [bs][H][W][3] = uint8(clamp(clamp(r * 2 - 1, -1, 1) * 127.5 + 127.5, 0, 255)),
 *                       every operation rounded on its own, truncating; out_f [bs][3][H][W] = r when out_f is not NULL.
 * 16-byte accesses along a row where the pointers and the row length allow, single elements otherwise: the same bits.  No atomics, no host synchronisation,
 * grids depend on the shapes alone: the same inputs give the same bits, and the calls can be captured in a graph.  bs == 0 (planes == 0) returns at once. */
E4S_API int e4s_esr_input(float* out, const uint8_t* img, int bs, int H, int W, int oh, int ow, void* stream);
E4S_API int e4s_esr_scale_add(float* y, const float* t, const float* x, int planes, int hw, void* stream);
E4S_API int e4s_esr_up2(float* out, const float* in, int planes, int h, int w, void* stream);
E4S_API int e4s_esr_tail(uint8_t* out_u8, float* out_f, const float* x, const float* weight, const float* bias, int bs, int H, int W, void* stream);

/* f12: GPEN face enhancement, stage 1 — what the GAN-prior generator (swap_face_fine/gpen/face_model/gpen_model.py:628-690 FullGenerator, between the tensor ends of
 * face_gan.py:49-62; csrc/gpen.hip) needs beside e4s_upfirdn2d, e4s_conv2d(_sb), e4s_grouped_linear, e4s_style_demod_batched, the single-region modulated
 * convolutions and e4s_region_torgb.
 *   e4s_gpen_stem       : ecd0 (gpen_model.py:658, ConvLayer(3, C0, 1)): out [bs][C0][H][W] = lrelu(bias[co] + sum_c weight[co][c] x[c]) * sqrt(2) in exact float32:
 *                         bias, then one fused multiply-add per input channel in channel order, then v > 0 ? v : 0.2 v, then the scale.  weight [C0][3] carries the
 *                         equalised-lr scale.  Exactly one input: x float [bs][3][H][W], or x_u8 uint8 [bs][H][W][3] (RGB) taken through FaceGAN.img2tensor first
 *                         (v / 255 as a true division, - 0.5, / 0.5, each rounded on its own).
 *   e4s_gpen_noise_half : the concatenated half of a StyledConv (gpen_model.py:294-302, 350-356): out_k[b * out_stride_b + c * hw + p] =
 *                         lrelu(fl(w_k[0] * f[b][c][p]) + bias_k[c]) * sqrt(2) for k = 0 and, when out1 is not NULL, k = 1: f [bs][C][hw] is read once for both
 *                         layers of a resolution.  out_k aims at plane C of a [bs][2C][hw] buffer (out_stride_b = 2 C hw), bias_k at entry C of the activation bias,
 *                         w_k at the device scalar noise.weight.  The bits of scale * F.leaky_relu(cat(out, w * noise) + bias, 0.2).
 *   e4s_gpen_to_u8      : FaceGAN.tensor2img without its channel flip: out uint8 [bs][H][W][3] = uint8(clip(x * 0.5 + 0.5, 0, 1) * 255) of x [bs][3][H][W], every
 *                         operation rounded on its own, truncating.
 * 16-byte accesses along a row (12 bytes of uint8 pixels) where the pointers and the row length allow, single elements otherwise: the same bits.  No atomics, no
 * host synchronisation, grids depend on the shapes alone: the same inputs give the same bits, and the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_gpen_stem(float* out, const float* x, const uint8_t* x_u8, const float* weight, const float* bias, int bs, int C0, int H, int W, void* stream);
E4S_API int e4s_gpen_noise_half(float* out0, float* out1, const float* f, const float* w0, const float* w1, const float* bias0, const float* bias1,
                                int bs, int C, int hw, int64_t out_stride_b, void* stream);
E4S_API int e4s_gpen_to_u8(uint8_t* out, const float* x, int bs, int H, int W, void* stream);

/* f13: GPEN face enhancement, stage 2 — what the face mask's network (swap_face_fine/gpen/face_parse/parse_model.py:21-75 ParseNet, blocks.py:72-125 ConvLayer and
 * ResidualBlock, between the tensor ends of face_parsing.py:39-79; csrc/parsenet.hip) needs around its 3 x 3 convolutions, which run on e4s_conv2d_sb3 with
 * pad = 0 on planes that e4s_parsenet_pad wrote: that kernel pads with zeros only, every ConvLayer pads by reflection (index -1 is 1, index n is n - 2) and the
 * decoder's put a nearest x 2 in front.
 *   e4s_parsenet_stem : encoder.0 = ConvLayer(3, C0, 3) (parse_model.py:46; reflection pad 1, bias, no norm, no activation): out [bs][C0][H][W] in exact float32,
 *                       each output bias[co], then 27 fused multiply-adds in (input channel, row, column) order over weight [C0][3][3][3]; the reflection is index
 *                       arithmetic.  Exactly one input: x float [bs][3][H][W], or x_u8 uint8 [bs][H][W][3] taken through FaceParse.img2tensor first
 *                       (face_parsing.py:59-63): with bgr = 1 colour c is byte 2 - c (the [..., ::-1] flip), with bgr = 0 byte c, and the value is lut[byte] with
 *                       lut [256] the float32 of numpy's float64 v / 255. * 2 - 1, made on the host with that expression.  H, W >= 2.
 *   e4s_parsenet_pad  : the input of a reflection-padded convolution in one pass: out [planes][u h + 2][u w + 2] = reflection pad 1 of the nearest x u of
 *                       v = x + add, x and add [planes][h][w], the sum rounded once (add may be NULL: v = x); u = 1, or 2 with the source at (y >> 1, x >> 1)
 *                       (F.interpolate(scale_factor=2, mode='nearest'), blocks.py:84).  add carries feat + body(feat) (parse_model.py:71), which is never a pass
 *                       of its own.  Every output cell is computed from the one source element its index names, so a border cell holds the bits of the
 *                       interior cell it mirrors.  h, w >= 2 when u = 1, h, w >= 1 when u = 2.
 * The mask (face_parsing.py:65-79: argmax over the 19 classes, then MASK_COLORMAP) is e4s_bilinear_argmax at equal size with the colour map as its table: at
 * ih == oh, iw == ow the scale (ih - 1) / (oh - 1) is exactly 1, the coordinates are integers and the blend is 1 * q + 0 * q', which is q for finite logits, so the
 * call is argmax + table (first maximum wins, as torch.argmax).
 * 16-byte accesses where the pointers and the row length allow (the stem along a row when W % 4 == 0, 12 bytes of uint8 pixels; the pad kernel over the flat
 * output, whose rows are not 16-byte aligned one by one), single elements otherwise: the same bits.  No atomics, no host synchronisation, grids depend on the
 * shapes alone: the same inputs give the same bits, and the calls can be captured in a graph.  bs == 0 (planes == 0) returns at once. */
E4S_API int e4s_parsenet_stem(float* out, const float* x, const uint8_t* x_u8, const float* lut, int bgr, const float* weight, const float* bias, int bs, int C0,
                              int H, int W, void* stream);
E4S_API int e4s_parsenet_pad(float* out, const float* x, const float* add, int planes, int h, int w, int u, void* stream);

/* f14: GPEN face enhancement, stage 3 — the RetinaFace detector (swap_face_fine/gpen/face_detect/retinaface_detection.py:61-131 detect, facemodels/retinaface.py,
 * facemodels/net.py, layers/functions/prior_box.py, utils/box_utils.py decode and decode_landm, utils/nms/py_cpu_nms.py; csrc/retinaface.hip): the glue between the
 * network's convolutions (conv.hip, stem and pooling as the face parser's ResNet) and the detection tail on the device.
 *   e4s_retina_input   : out [bs][3][H][W] = pixel - (104, 117, 123) in BGR plane order from img_u8 [bs][H][W][3] (bgr = 1: byte c is plane c; bgr = 0: byte 2 - c).
 *                        Exact; the mean cannot go into the stem's bias, because the zero padding comes behind the subtraction.
 *   e4s_retina_up_add  : out [planes][h][w] = a + b[min(floor(y * (float)hb / h), hb - 1)][min(floor(x * (float)wb / w), wb - 1)], b [planes][hb][wb]:
 *                        F.interpolate(size=..., mode="nearest") + add of FPN.forward (net.py:89-94) in one pass, ATen's legacy index rule, any size pair.
 *   e4s_retina_cat_relu: out [bs][ca + cb + cc][hw] = relu(cat(a, b, c)) of SSH.forward (net.py:64-65) for any batch.
 *   e4s_retina_decode  : head_l [bs][32][ceil(H / s)][ceil(W / s)], s = 8, 16, 32: channels 0-7 BboxHead (anchor, coordinate), 8-11 ClassHead (anchor, class), 12-31
 *                        LandmarkHead (anchor, value) of level l.  Anchor (y w + x) 2 + a, levels concatenated, N in all.  Writes, each group optional as a whole,
 *                        the dense loc [bs][N][4], conf [bs][N][2] (softmax) and landms [bs][N][10] of RetinaFace.forward, and score [bs][N] (class 1),
 *                        boxes [bs][N][4] and lmk [bs][N][10]: decode / decode_landm with variances (0.1, 0.2) on priors from index arithmetic (a correctly rounded
 *                        float32 division of the exact numerator: PriorBox.forward's values), times (W, H, ...), every operation rounded on its own.
 *   e4s_retina_priors  : out [N][4] = those priors (cx, cy, s_kx, s_ky).
 *   e4s_retina_compact : keys [bs][cap] (int64) = (score bits << 32) | (0xFFFFFFFF - anchor) of every anchor with score > threshold in anchor order, -1 behind them;
 *                        counts [bs][2] = (anchors above the threshold, candidates kept).  With more than cap the cap highest scores are kept (ties at the cut: the
 *                        lower anchors).  Sorting the keys descending orders the candidates by score, equal scores by anchor.  cap <= 16384.
 *   e4s_retina_nms     : py_cpu_nms on keys sorted descending: (x2 - x1 + 1)(y2 - y1 + 1) areas, ovr = inter / (a_i + a_j - inter) in float32, greedy, ovr <= thresh
 *                        stays; dets [bs][keep_top_k][5] (box, score), landms_out [bs][keep_top_k][10] as (x0..x4, y0..y4), keep [bs][keep_top_k] (positions in the
 *                        sorted list), nkeep [bs], all cut to keep_top_k; rows behind nkeep are not written.  cbox [bs][cap][4] is workspace.
 * 16-byte accesses where pointers and lengths allow, single elements otherwise: the same bits.  No float atomics, no host synchronisation, grids from shapes and
 * capacities alone: the same inputs give the same bits, and the calls can be captured in a graph.  bs == 0 (planes == 0) returns at once. */
E4S_API int e4s_retina_input(float* out, const uint8_t* img_u8, int bgr, int bs, int H, int W, void* stream);
E4S_API int e4s_retina_up_add(float* out, const float* a, const float* b, int planes, int h, int w, int hb, int wb, void* stream);
E4S_API int e4s_retina_cat_relu(float* out, const float* a, const float* b, const float* c, int bs, int ca, int cb, int cc, int hw, void* stream);
E4S_API int e4s_retina_priors(float* out, int H, int W, void* stream);
E4S_API int e4s_retina_decode(float* loc, float* conf, float* landms, float* score, float* boxes, float* lmk, const float* head0, const float* head1,
                              const float* head2, int bs, int H, int W, void* stream);
E4S_API int e4s_retina_compact(int64_t* keys, int* counts, const float* score, int bs, int N, int cap, float threshold, void* stream);
E4S_API int e4s_retina_nms(float* dets, float* landms_out, int* keep, int* nkeep, float* cbox, int64_t* sorted_keys, const int* counts, const float* boxes,
                           const float* lmk, int bs, int N, int cap, int keep_top_k, float nms_threshold, void* stream);

/* f15: GPEN face enhancement, stage 4 — what FaceEnhancement.process(aligned=False) (swap_face_fine/gpen/face_enhancement.py:68-108, align_faces.py:25-93, 210-266;
 * csrc/gpen_paste.hip) does between its three networks, in OpenCV's arithmetic as tests/gpen_paste_model.py restates it.  Float64 arrays travel as void pointers.
 *   transforms [n][2][2][3] (float64): per face the 2 x 3 forward matrix (frame -> crop) and the 2 x 3 inverse (crop -> frame).  flags [n]: bit 0 = skip the face,
 *   bit 1 = a small face.  "warpAffine(src, M, (w, h))" below is cv2's with flags=3: M inverted in float64, the map in fixed point (10 fractional bits, sampled on
 *   its 1/32 grid after + 16), bilinear, constant-0 border; uint8 with the integer weights (32 - ax)(32 - ay) ... and (sum + 512) >> 10.
 *   e4s_gpen_face_transforms : dets [n][5] (x1, y1, x2, y2, score), landms [n][10] (x0..x4, y0..y4), ref_points [5][2] (float64, cast to float32 first as the
 *                              reference does): the least-squares similarity pair of warp_and_crop_face in float64 closed form (no SVD), and the flags: skip if
 *                              score < threshold, if a landmark is not finite or if the landmarks coincide (the matrices are then zero); small if
 *                              min(y2 - y1, x2 - x1) < small_face, in float32.  One lane per face.
 *   e4s_gpen_warp_crop_u8    : out [n][S][S][3] = warpAffine(frames[frame_of_face[i]] [H][W][3], forward_i, (S, S)); a frame index outside 0 .. bs - 1 gives zeros.
 *   e4s_gpen_smooth3_u8      : out [n][S][S][3] = cv2.filter2D(face, -1, [[1,2,1],[2,4,2],[1,2,1]] / 16) (BORDER_REFLECT_101, the sum / 16 rounded half to even) of
 *                              the faces whose small flag is set, a copy of the others.  out must not be faces.
 *   e4s_gpen_mask_feather    : out [n][S][S] (float32) = mask_postprocess(masks / 255): `thres` rows and columns at each edge zeroed, then twice the separable
 *                              k-tap blur (rows, then columns, BORDER_REFLECT_101) with the float64 taps [k], float64 sums and intermediates in scratch
 *                              (e4s_gpen_mask_feather_scratch_bytes).  k odd, k / 2 < S, k <= 129, thres >= 1.
 *   e4s_gpen_paste_u8        : per frame b and its faces face_begin[b] .. face_begin[b + 1] - 1 in order, skipped ones left out: m_i = warpAffine(masks_i,
 *                              inverse_i, (W, H)) in float32 (weights (1 - fx)(1 - fy) ..., ((v00 w0 + v01 w1) + v10 w2) + v11 w3), p_i the uint8 warpAffine of
 *                              faces_i; where m_i - full_mask > 0: full_mask = m_i, full_img = p_i; out [bs][H][W][3] = convertScaleAbs(base (1 - full_mask) +
 *                              full_img full_mask) in float32, every operation rounded on its own.  One pass, no full-frame intermediate; full_mask [bs][H][W]
 *                              is optional output.  out may be base itself (each lane reads its own pixels before it writes them), no other overlap.  n == 0
 *                              copies base to out.
 * No host synchronisation, no atomics, grids from shapes and counts alone: the same inputs give the same bits, and the calls can be captured in a graph.  n == 0
 * returns without a launch. */
E4S_API int e4s_gpen_face_transforms(void* transforms, int* flags, const float* dets, const float* landms, const void* ref_points, float threshold,
                                     float small_face, int n, void* stream);
E4S_API int e4s_gpen_warp_crop_u8(uint8_t* out, const uint8_t* frames, const int* frame_of_face, const void* transforms, int n, int bs, int H, int W, int S,
                                  void* stream);
E4S_API int e4s_gpen_smooth3_u8(uint8_t* out, const uint8_t* faces, const int* flags, int n, int S, void* stream);
E4S_API int e4s_gpen_mask_feather_scratch_bytes(int n, int S, int64_t* bytes);
E4S_API int e4s_gpen_mask_feather(float* out, const uint8_t* masks, const void* taps, void* scratch, int n, int S, int k, int thres, void* stream);
E4S_API int e4s_gpen_paste_u8(uint8_t* out, float* full_mask, const uint8_t* base, const uint8_t* faces, const float* masks, const void* transforms,
                              const int* flags, const int* face_begin, int n, int bs, int H, int W, int S, void* stream);

/* f16: GPEN face enhancement, stage 5 — the ends of the RealESRNet pass (swap_face_fine/gpen/sr_model/real_esrnet.py:26-60 RealESRNet.process around
 * rrdbnet_arch.py:64-116 RRDBNet; csrc/gpen_sr.hip, the tail on csrc/rrdb.hip) and the resize of the frame to the super-resolved size (face_enhancement.py:66).  The network's convolutions run
 * on e4s_conv2d_sb3, its glue on e4s_esr_scale_add and e4s_esr_up2.
 *   e4s_gsr_input           : uint8 img [bs][H][W][3] -> out [bs][3 r r][(H + ph) / r][(W + pw) / r], r = 1, 2 or 4: v / 255 as a correctly rounded float32 division,
 *                             colour c from byte 2 - c with bgr (byte c without), the reflect pad of ph = (-H) mod r rows and pw = (-W) mod r columns at the
 *                             bottom / right (F.pad(..., 'reflect'): index n + i is n - 2 - i; needs H > ph, W > pw) and pixel_unshuffle by r (arch_util.py:109-125:
 *                             channel c r r + dy r + dx) in one pass.  r = 1: no pad, no unshuffle.
 *   e4s_gsr_tail            : q = conv3x3(x [bs][C][H][W], weight [3][C][3][3], zero pad 1) + bias [3] in exact float32 as e4s_esr_tail forms it: bias, then C * 9 fused
 *                             multiply-adds in (input channel, row, column) order; C a multiple of 8 up to 64.  out_u8 [bs][Ho][Wo][3] = uint8(rint(clamp(q, 0, 1) *
 *                             255.0f)) of the first Ho x Wo pixels, the product rounded on its own, rint to even (numpy's .round()), channel o at byte 2 - o with bgr;
 *                             out_f [bs][3][H][W] = q, uncropped, when out_f is not NULL.
 *   e4s_cv_resize_linear_u8 : out [bs][Ho][Wo][3] = cv2.resize(img [bs][H][W][3], (Wo, Ho)) at INTER_LINEAR in OpenCV's portable fixed-point arithmetic: per axis
 *                             scale = src / dst (double), f = float((d + 0.5) scale - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= src - 1: s = src - 1,
 *                             f = 0; coefficients short(rint((1 - f) 2048)), short(rint(f 2048)) (1 - f in float32); h = S[s] a0 + S[s + 1] a1 in int32 per row, then
 *                             (((b0 (h0 >> 4)) >> 16) + ((b1 (h1 >> 4)) >> 16) + 2) >> 2.  H == 2 Ho with W == 2 Wo (cv2 takes INTER_AREA there) is refused.  Not run
 *                             against OpenCV by anyone: tests/gpen_sr_model.py restates it and is the pin.
 * 16-byte accesses along a row (12 bytes of uint8 pixels) where the pointers and the row length allow, single elements otherwise: the same bits; the resize is a
 * byte gather.  No atomics, no host synchronisation, grids depend on the shapes alone: the same inputs give the same bits, and the calls can be captured in a graph.
 * bs == 0 returns at once. */
E4S_API int e4s_gsr_input(float* out, const uint8_t* img, int bs, int H, int W, int r, int bgr, void* stream);
E4S_API int e4s_gsr_tail(uint8_t* out_u8, float* out_f, const float* x, const float* weight, const float* bias, int bs, int C, int H, int W, int Ho, int Wo, int bgr,
                         void* stream);
E4S_API int e4s_cv_resize_linear_u8(uint8_t* out, const uint8_t* img, int bs, int H, int W, int Ho, int Wo, void* stream);

/* f17: face-vid2vid reenactment, stage 1 — keypoints and head pose (swap_face_fine/face_vid2vid/modules/keypoint_detector.py:9-178, modules/util.py:55-103, 175-213,
 * 335-418, drive_demo.py:67-180; csrc/conv3d.hip, csrc/vid2vid.hip).  The 2-D convolutions of both networks run on e4s_conv2d / e4s_conv2d_sb3.
 *   e4s_conv3d_prep_weights_sb3 : a Conv3d weight [cout][cin][3][3][3] (times the folded BatchNorm scale) as three bf16 slabs [ceil(cin / 16)][27][2][cout][8], the
 *                                 chunk layout of e4s_conv_prep_weights_sb3 with the 27 taps in (kd, kh, kw) order; bias_out as there.
 *   e4s_conv3d_sb3              : out [bs][cout][D][H][W] = act(conv3d(x', w, stride 1, zero pad 1) + bias + residual), x' [bs][cin][D][H][W] =
 *                                 x [bs][cin][D][H / up_hw][W / up_hw] read at (d, y / up_hw, x / up_hw): the nearest (1, 2, 2) upsampling of UpBlock3d folded into
 *                                 the gather (up_hw 1 or 2; H and W multiples of it).  D, H, W are the OUTPUT extents.  Implicit GEMM with K = 27 cin on the three-way
 *                                 bf16 split (six v_mfma_f32_32x32x16_bf16 per 16-deep step, fp32 accumulation: fp32-class).  act: 0 none, 1 ReLU.  bias [cout] and
 *                                 residual [bs][cout][D][H][W] optional.  Any cin and cout >= 1, no padding on the caller's side.  Scalar loads of x: any 4-byte alignment
 *                                 gives the same bits.
 *   e4s_v2v_antialias_down      : out [planes][ceil(h / s)][ceil(w / s)] = AntiAliasInterpolation2d: zero pad k / 2, the k x k kernel `taps` (k odd, <= 33; the
 *                                 module's normalised Gaussian buffer), then [::s, ::s], only the kept outputs evaluated: k k fused multiply-adds in (row, column)
 *                                 order from 0, exact float32.
 *   e4s_avgpool2x2              : nn.AvgPool2d(2) on [planes][h][w] -> [planes][h / 2][w / 2] (an odd last row / column is dropped): (((a + b) + c) + d) * 0.25 in row order.
 *   e4s_v2v_heatmap_kp          : per (sample, keypoint) one workgroup: m = max(logit / temperature) over the D H W positions (a float32 division, as the reference divides), e = exp(logit / temperature - m), then
 *                                 value [bs][K][3] = (sum e x, sum e y, sum e z) / sum e on the grid 2 i / (n - 1) - 1 in (x, y, z) order (each extent >= 2);
 *                                 with jac_planes [bs][9 K][D][H][W]: jacobian [bs][K][3][3] = sum e J_j / sum e; heatmap [bs][K][D][H][W] = e / sum e when wanted.
 *                                 Each lane sums its strided positions in order, the 256 partial sums are added in a fixed tree: the same inputs give the same bits.
 *   e4s_v2v_kp_transform        : per sample: degrees (yaw, pitch, roll) = sum softmax(row) idx * 3 - 99 of the three [bs][nbins] logit rows (summed in float64, rounded once), or deg_in [bs][3]
 *                                 itself when logits are NULL (free_view); radians = deg / 180 * 3.14; rot = pitch_mat yaw_mat roll_mat (drive_demo.py:107-133);
 *                                 value_out [bs][K][3] = rot kp + t + exp (kp [kp_bs][K][3] with kp_bs == bs or 1: one canonical set for every frame);
 *                                 jac_out [bs][K][3][3] = rot jac (einsum 'bmp,bkps->bkms') when jac is given; deg_out [bs][3] and rot_out [bs][3][3] optional.
 * No atomics, no host synchronisation, grids from shapes alone: the calls can be captured in a graph.  bs == 0 (planes == 0) returns at once. */
E4S_API int e4s_conv3d_prep_weights_sb3(uint16_t* w0, uint16_t* w1, uint16_t* w2, float* bias_out, const float* weight, const float* bn_gamma,
                                        const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps, const float* conv_bias, int cout, int cin,
                                        void* stream);
E4S_API int e4s_conv3d_sb3(float* out, const float* x, const uint16_t* w0, const uint16_t* w1, const uint16_t* w2, const float* bias, const float* residual,
                           int act, int up_hw, int bs, int cin, int cout, int D, int H, int W, void* stream);
E4S_API int e4s_v2v_antialias_down(float* out, const float* x, const float* taps, int planes, int h, int w, int k, int s, void* stream);
E4S_API int e4s_avgpool2x2(float* out, const float* x, int planes, int h, int w, void* stream);
E4S_API int e4s_v2v_heatmap_kp(float* value, float* jacobian, float* heatmap, const float* logits, const float* jac_planes, float temperature, int bs, int K, int D,
                               int H, int W, void* stream);
E4S_API int e4s_v2v_kp_transform(float* value_out, float* jac_out, float* deg_out, float* rot_out, const float* yaw, const float* pitch, const float* roll,
                                 const float* deg_in, const float* t, const float* exp, const float* kp, const float* jac, int bs, int kp_bs, int K, int nbins,
                                 void* stream);

/* f18: face-vid2vid reenactment, stage 2 — the dense-motion network (swap_face_fine/face_vid2vid/modules/dense_motion.py:9-128, modules/util.py:13-71, 175-332;
 * csrc/conv3d_k7.hip, csrc/conv3d.hip, csrc/vid2vid.hip).  `compress` runs on e4s_conv2d_sb3 as a 1 x 1, the hourglass on the strided 3 x 3 x 3 kernel.
 *   e4s_conv3d_k7_prep_weights_sb3 : a weight [cout][cin][kd][7][7] (kd 7 or 1; the Conv2d [cout][cin][7][7] is kd 1) as three bf16 slabs
 *                                    [ceil(cin / 16)][49 kd][2][cout][8], the chunk layout of e4s_conv_prep_weights_sb3 with the taps in (kd, kh, kw) order.
 *   e4s_conv3d_k7_sb3              : out [bs][cout][D][H][W] = act(conv(x, w, stride 1, zero pad (kd / 2, 3, 3)) + bias) on x [bs][cin][D][H][W] float32, kd 7 or 1,
 *                                    1 <= cout <= 32, any cin >= 1; act 0 none, 3 sigmoid; bias optional.  Implicit GEMM on the three-way bf16 split
 *                                    (six v_mfma_f32_16x16x32_bf16 per 32-deep step: two (kh, kw) taps of a 16-channel chunk), fp32 accumulation.  Depth steps
 *                                    that lie in the padding are skipped as a whole.  kd 1 with D 1 is a 7 x 7 Conv2d on [bs][cin][H][W].  Scalar loads of x: any
 *                                    4-byte alignment gives the same bits.
 *   e4s_conv3d_sb3_strided         : the 3 x 3 x 3 kernel above with element batch strides: sample b of x starts at x + b x_bstride, of out at out + b out_bstride,
 *                                    of residual at residual + b res_bstride, so a channel slice of a wider buffer is read or written in place (the decoder's
 *                                    concatenations are never copied).  With the dense strides it is the unstrided entry point, bit for bit.
 *   e4s_avgpool2x2_strided         : the 2 x 2 average pool above on x [bs][planes][h][w] (dense) into out + b out_bstride + [planes][h / 2][w / 2]: the same arithmetic.
 *   e4s_v2v_motion_input           : the hourglass input in one pass: out + b out_bstride + [(K + 1)(c + 1)][D][H][W], channel k (c + 1) the heatmap
 *                                    exp(-0.5 |g - kp_d|^2 / 0.01) - exp(-0.5 |g - kp_s|^2 / 0.01) (exactly 0 for k = 0), channel k (c + 1) + 1 + j feature j of
 *                                    feature [bs][c][D][H][W] sampled as F.grid_sample's defaults do (trilinear, zero padding, align_corners = False; the eight taps in
 *                                    ATen's CPU order) at the sparse motion of (b, k, position): k = 0 the identity grid g = 2 i / (n - 1) - 1 in (x, y, z) order,
 *                                    otherwise J (g - kp_d[k - 1]) + kp_s[k - 1] with J = jac_s inv(jac_d) when both Jacobians [bs][K][3][3] are given (the inverse
 *                                    from the adjugate in float64, rounded once), J = I without.  kp_d, kp_s [bs][K][3].  Every extent >= 2.
 *   e4s_v2v_motion_combine         : mask [bs][K + 1][D][H][W] = softmax over the K + 1 channels of logits (maximum first, then exp, the sum in channel order) and
 *                                    deformation [bs][D][H][W][3] = sum_k mask_k sparse_motion_k in channel order, the sparse motions from the device function of
 *                                    e4s_v2v_motion_input: the same bits.  K + 1 <= 32.
 * No atomics, no host synchronisation, no scratch memory, grids from shapes alone: the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_conv3d_k7_prep_weights_sb3(uint16_t* w0, uint16_t* w1, uint16_t* w2, const float* weight, int cout, int cin, int kd, void* stream);
E4S_API int e4s_conv3d_k7_sb3(float* out, const float* x, const uint16_t* w0, const uint16_t* w1, const uint16_t* w2, const float* bias, int act, int kd, int bs,
                              int cin, int cout, int D, int H, int W, void* stream);
E4S_API int e4s_conv3d_sb3_strided(float* out, const float* x, const uint16_t* w0, const uint16_t* w1, const uint16_t* w2, const float* bias,
                                   const float* residual, int act, int up_hw, int bs, int cin, int cout, int D, int H, int W, int64_t x_bstride,
                                   int64_t out_bstride, int64_t res_bstride, void* stream);
E4S_API int e4s_avgpool2x2_strided(float* out, const float* x, int bs, int planes, int h, int w, int64_t out_bstride, void* stream);
E4S_API int e4s_v2v_motion_input(float* out, const float* feature, const float* kp_d, const float* kp_s, const float* jac_d, const float* jac_s, int bs, int K,
                                 int c, int D, int H, int W, int64_t out_bstride, void* stream);
E4S_API int e4s_v2v_motion_combine(float* mask, float* deformation, const float* logits, const float* kp_d, const float* kp_s, const float* jac_d,
                                   const float* jac_s, int bs, int K, int D, int H, int W, void* stream);

/* f19: face-vid2vid reenactment, stage 3 — the generator's feature warp (swap_face_fine/face_vid2vid/modules/generator.py:161-244, modules/util.py:131-153,
 * 196-259; csrc/vid2vid.hip).  The appearance encoder runs on the 2-D convolutions and the 2 x 2 pool above, `resblocks_3d` on the 3 x 3 x 3 kernel (norm2 folded
 * into conv1, the block's input as conv2's residual), `third` and `fourth` on the split-bf16 2-D convolution.
 *   v2v_deform  : deform_input: out + b out_bstride + [C D][H][W] = F.grid_sample(feature, deformation) at its defaults (trilinear, zero padding, align_corners =
 *                 False), feature sample b at feature + b feat_bstride + [C][D][H][W], deformation [bs][D][H][W][3] in (x, y, z) order.  Unnormalisation, floor,
 *                 the eight weights and the order in which the taps join the sum are the device function of the motion-input kernel above: the same bits on the
 *                 same coordinates, and exactly 0 where all eight taps are outside.  A position's taps are computed once per 4 channels.  feat_bstride 0: one
 *                 feature serves every sample (the source's, for all driving frames of a launch); otherwise at least a sample.  One position per lane, so a
 *                 wave gathers from neighbouring addresses and stores 256 contiguous bytes; any 4-byte alignment gives the same bits.  (Four positions per
 *                 lane with 16-byte stores were measured 1.7x slower on a smooth deformation: every gather of a wave then spreads over four times the cache
 *                 lines; tools/probes/deform_forms_probe.hip holds both forms.)
 *   v2v_bn_relu : out [bs][C][n] = max(fma(x, scale[c], shift[c]), 0): an eval-mode BatchNorm and ReLU that stand in front of a zero-padded convolution
 *                 (ResBlock3d's norm1), which no fold into the weights can express.  out may be x.  A NaN input gives 0 (fmaxf returns its other
 *                 operand), where F.relu would hand the NaN on.
 *   v2v_occlude : out [bs][C][hw] = x * occ [bs][1][hw]; out may be x.
 * The last two take 16-byte accesses where the plane size is a multiple of 4 and the pointers are aligned.  fp32, no atomics, no host synchronisation, no
 * scratch memory, grids from shapes alone: the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_v2v_deform(float* out, const float* feature, const float* deformation, int bs, int C, int D, int H, int W, int64_t feat_bstride,
                           int64_t out_bstride, void* stream);
E4S_API int e4s_v2v_bn_relu(float* out, const float* x, const float* scale, const float* shift, int bs, int C, int n, void* stream);
E4S_API int e4s_v2v_occlude(float* out, const float* x, const float* occ, int bs, int C, int hw, void* stream);

/* f20: face-vid2vid reenactment, stage 4 — the glue of the SPADEDecoder (swap_face_fine/face_vid2vid/modules/generator.py:120-158, modules/util.py:421-481;
 * csrc/vid2vid.hip).  The decoder's convolutions (fc, mlp_shared + ReLU, mlp_gamma | mlp_beta as one convolution, conv_0, conv_1 with the shortcut as residual,
 * conv_s) run on e4s_conv2d_sb3, the instance norms' statistics on e4s_plane_stats, the nearest picks of the label map on e4s_esr_up2.
 *   v2v_spade_norm : the modulation of one or two SPADE norms that normalise the same x, with the decoder's nearest x2 folded into the read:
 *                    out_a [bs][C][h][w] = leaky_0.2((x - mean) rstd (1 + gamma_a) + beta_a) and, when gb_s and out_s are given (together, or both NULL),
 *                    out_s = (x - mean) rstd (1 + gamma_s) + beta_s without an activation (the norm_s of a learned shortcut); x is read once for both.
 *                    x [bs][C][h / up][w / up] is read at (y / up, x / up), up 1 or 2 dividing h and w; mean / rstd [bs * C] are e4s_plane_stats' of that
 *                    low-resolution plane: a nearest x2 plane has exactly the statistics of the plane it repeats, so the upsampled x is never formed.
 *                    gb_* [bs][2 C][h][w] = gamma | beta, the two halves of one convolution's output.  Every operation is rounded on its own by the device
 *                    function e4s_spade_modulate runs (csrc/spade_value.h): the same bits as that call on x upsampled by e4s_esr_up2.  16-byte accesses when w % 4 == 0
 *                    and every pointer is 16-byte aligned, one element per lane otherwise: the same bits.
 *   v2v_image_head : out [bs][3][H][W] = sigmoid(conv3x3(leaky_0.2(x [bs][cin][H][W]), weight [3][cin][3][3], zero pad 1) + bias [3]): conv_img behind its
 *                    activation.  Exact float32 in the form of e4s_esr_tail: every sum starts at the bias and takes 9 cin fused multiply-adds in (input
 *                    channel, row, column) order; the sigmoid is 1 / (1 + expf(-v)).  16-byte accesses when W % 4 == 0 and x and out are 16-byte aligned.
 * fp32, no atomics, no host synchronisation, no scratch memory, grids from shapes alone: the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_v2v_spade_norm(float* out_a, float* out_s, const float* x, const float* mean, const float* rstd, const float* gb_a, const float* gb_s, int bs,
                               int C, int h, int w, int up, void* stream);
E4S_API int e4s_v2v_image_head(float* out, const float* x, const float* weight, const float* bias, int bs, int cin, int H, int W, void* stream);

/* f21: CodeFormer face restoration, stage 1 — what CodeFormer.forward needs up to quant_feat between its convolutions (swap_face_fine/archs/codeformer_arch.py:
 * 12-43, 99-134, 161-262, archs/vqgan_arch.py:14-20, 72-84, 117-273; csrc/codeformer.hip).  Every 3 x 3 and 1 x 1 convolution and every linear of the transformer
 * runs on e4s_conv2d_sb3, conv_in (3 channels) and the logits head on the exact e4s_conv2d.  "Channel-major": a
 * tensor [bs][C][T] with the tokens innermost, which is NCHW with T = H W.
 *   cf_group_stats: stats [runs][3] = (mean, corr, rstd) of each of the `runs` contiguous runs of `run` floats in x: in NCHW a GroupNorm group of one sample is
 *                   such a run of C / groups hw floats.  Two launches: part [runs][chunks][2] (scratch the caller provides) takes the mean and the sum of squares
 *                   about that mean of each of the `chunks` equal pieces of a run (the last one shorter; two passes per piece, so a run whose mean is a hundred
 *                   times its deviation keeps its variance); one thread per run then merges its pieces in piece order in float64: mean is the float32 rounding
 *                   of the merged mean, corr what that rounding left, rstd = 1 / sqrt(var + eps) with the biased variance.  1 .. 64 chunks, a function of the
 *                   shapes alone (the host layer: one per 16384 floats).
 *   cf_group_norm : out = s sigmoid(s) (swish != 0) or s, s = ((x - mean_g) - corr_g) rstd_g gamma[c] + beta[c] for x [bs][C][hw] and stats = cf_group_stats'
 *                   output over the bs groups runs.  The sigmoid is 1 / (1 + expf(-s)).  bs C <= 65535.
 *   cf_attention  : out[b][h d + c][i] = sum_j softmax_j(scale q_i . k_j) v[c][j] on channel-major q, k, v, out with `heads` heads of d channels; sample b of an
 *                   operand starts b * its batch stride (elements) behind the pointer, so q, k, v may be slices of one convolution's output.  T = 1 .. 1024, d a
 *                   multiple of 16 up to 512.  Exact float32: the scores are fmaf chains in channel order, the row maximum is subtracted, the row sum and the
 *                   output sums run over the keys in a fixed order.
 *   cf_layer_norm : y[b][c][t] = (x - mean_t) rstd_t gamma[c] + beta[c] over the C <= 512 channels of a token (biased variance, eps inside the root) and, when
 *                   pos [C][T] and y_pos are given (together), y_pos = y + pos.
 *   cf_gelu       : out = 0.5 x (1 + erf(x / sqrt 2)) over n elements; out may be x.
 *   cf_pad_rb     : out [planes][h + 1][w + 1] = x with one zero column on the right and one zero row below (Downsample's F.pad (0, 1, 0, 1)).
 *   cf_argmax     : idx[b][t] (int64) = the lowest n at which logits[b b_stride + t t_stride + n n_stride] is largest, n < K.
 *   cf_quant      : out[b][c][t] = emb[idx[b][t]][c] (idx int64 [bs][T]; emb [K][C]; an index outside 0 .. K - 1 is clamped) and, with adain != 0, adaptive_instance_normalization
 *                   of it against style [bs][C][T]: (q - mean_q) / sqrt(var_q + eps) * sqrt(var_s + eps) + mean_s per plane, var unbiased.  T <= 1024, and
 *                   T >= 2 with adain.
 * fp32, no atomics, no host synchronisation, no scratch memory, grids from shapes alone: the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_cf_group_stats(float* stats, float* part, const float* x, int runs, int run, int chunks, float eps, void* stream);
E4S_API int e4s_cf_group_norm(float* out, const float* x, const float* stats, const float* gamma, const float* beta, int bs, int C, int groups, int hw, int swish,
                              void* stream);
E4S_API int e4s_cf_attention(float* out, const float* q, const float* k, const float* v, int64_t q_bstride, int64_t k_bstride, int64_t v_bstride,
                             int64_t out_bstride, int bs, int heads, int d, int T, float scale, void* stream);
E4S_API int e4s_cf_layer_norm(float* y, float* y_pos, const float* x, const float* gamma, const float* beta, const float* pos, int bs, int C, int T, float eps,
                              void* stream);
E4S_API int e4s_cf_gelu(float* out, const float* x, int64_t n, void* stream);
E4S_API int e4s_cf_pad_rb(float* out, const float* x, int planes, int h, int w, void* stream);
E4S_API int e4s_cf_argmax(int64_t* idx, const float* logits, int bs, int T, int K, int64_t b_stride, int64_t t_stride, int64_t n_stride, void* stream);
E4S_API int e4s_cf_quant(float* out, const void* idx, const float* emb, const float* style, int bs, int C, int T, int K, int adain, float eps, void* stream);

/* f22: CodeFormer face restoration, stage 2 — what CodeFormer.forward needs from quant_feat to out beyond block f21 (swap_face_fine/archs/codeformer_arch.py:
 * 136-157, 264-276, archs/vqgan_arch.py:60-70, 276-323; csrc/codeformer_gen.hip), and the caller's uint8 tail (inference_codeformer.py: tensor2img with
 * min_max = (-1, 1)).  The generator's GroupNorms and AttnBlocks run on block f21's entry points, its Upsample on e4s_esr_up2, every convolution on
 * e4s_conv2d_sb3 (the last one, 64 -> 3, included); a Fuse_sft_block's concatenation is the two-input form of that convolution and two GroupNorm calls with 16
 * groups each.
 *   cf_sft      : out = dec + w (dec scale + shift) for four contiguous [planes][hw] tensors, rounded as t = dec * scale; t = t + shift; t = w * t; out = dec + t.
 *                 16-byte accesses when hw % 4 == 0 and all four pointers are 16-byte aligned.
 *   cf_image_u8 : out (uint8) = rint(((min(max(x, -1), 1) - (-1)) / 2) * 255) over n elements, every step a float32 rounding, rint half to even.  16-byte reads
 *                 and 4-byte stores when n % 4 == 0, x is 16-byte and out 4-byte aligned.
 * fp32, no atomics, no host synchronisation, no scratch memory, grids from shapes alone: the calls can be captured in a graph.  An empty tensor returns at once. */
E4S_API int e4s_cf_sft(float* out, const float* dec, const float* scale, const float* shift, float w, int planes, int hw, void* stream);
E4S_API int e4s_cf_image_u8(uint8_t* out, const float* x, int64_t n, void* stream);

/* f23: CodeFormer face restoration, stage 3 — the tile ends of RealESRGANer.enhance (swap_face_fine/realesrgan_utils.py:69-172 pre_process, tile_process,
 * post_process around RRDBNet x4plus at half=False) and its cv2.resize(..., INTER_LANCZOS4) on uint8 (:243-248); csrc/esrgan_tile.hip.  The network between
 * the ends is block f11 / f16's (e4s_conv2d_sb3, e4s_esr_scale_add, e4s_esr_up2).
 *   e4s_esrt_input            : out [bs][3][th][tw] = float(v) / 255.0f (a correctly rounded float32 division, numpy's img.astype(float32) / 255) of the window
 *                               rows y0 .. y0 + th, columns x0 .. x0 + tw of the PRE-PADDED image [Hp][Wp] (Hp = H + pre_pad, Wp = W + pre_pad, which is never
 *                               formed: row H + i reads row H - 2 - i, F.pad(..., 'reflect'); Hp - H < H, Wp - W < W).  img uint8 [bs][H][W][3] (chw 0) or
 *                               [bs][3][H][W] (chw 1); the channel order is kept.
 *   e4s_esrt_tail             : q = conv3x3(x [bs][C][H][W], weight [3][C][3][3], zero pad 1) + bias [3] in exact float32 as e4s_esr_tail forms it (bias, then C * 9
 *                               fused multiply-adds per output in (input channel, row, column) order; C a multiple of 8 up to 64), evaluated ONLY on the window rows
 *                               oy0 .. oy1, columns ox0 .. ox1 of the tile's output; then clamp(q, 0, 1), * 255.0f, round half to even, uint8, stored at row Y0, column
 *                               X0 of canvas [bs][CH] rows of `pitch` bytes holding CW pixels of three bytes.  No byte outside the window is written; out_f must be null
 *                               (the argument keeps the shape of the other tails).  Plain vector stores.
 *   e4s_cv_resize_lanczos4_u8 : out [bs][Ho][Wo][3] = cv2.resize(img [bs][H][W][3], (Wo, Ho), interpolation=INTER_LANCZOS4) in OpenCV's portable fixed-point
 *                               arithmetic, given the tables of the rule, made on the host: per axis ofs int32 [dst] = s - 3 with s = floor(float((d + 0.5) scale
 *                               - 0.5)), scale = 1.0 / (double(dst) / src), and coef int16 [dst][8] = short(rint(c[k] 2048)) of interpolateLanczos4 at the fraction
 *                               (not reset at the borders; no fix-up of the sum); the taps read index clamp(ofs + k, 0, src - 1).  h = sum S[x_k] a_k in int32,
 *                               v = sum h_k b_k in int32, out = saturate_u8((v + (1 << 21)) >> 22).  A workgroup owns 16 x 64 output pixels; where their source window
 *                               is at most 40 rows by 136 columns it is staged through LDS and every source row filtered once, otherwise the pixels are formed directly.
 *                               Both forms give the same bits; no table content makes an access leave a tensor.  The coef tables are 16-byte aligned.
 * No atomics, no host synchronisation, no scratch memory, grids from shapes alone: the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_esrt_input(float* out, const uint8_t* img, int bs, int H, int W, int Hp, int Wp, int chw, int y0, int x0, int th, int tw, void* stream);
E4S_API int e4s_esrt_tail(uint8_t* canvas, float* out_f, const float* x, const float* weight, const float* bias, int bs, int C, int H, int W, int oy0, int oy1,
                          int ox0, int ox1, int Y0, int X0, int CH, int CW, int64_t pitch, void* stream);
E4S_API int e4s_cv_resize_lanczos4_u8(uint8_t* out, const uint8_t* img, const int* yofs, const void* ycoef, const int* xofs, const void* xcoef, int bs, int H,
                                      int W, int Ho, int Wo, void* stream);

/* f24: the two ends of the whole-clip reenactment chain (face_swap_video_pipeline.py:248-253) — skimage.transform.resize on a float64 image in front of
 * make_animation and (pred * 255).astype(np.uint8) behind it; csrc/skresize.hip.
 *   e4s_sk_resize_u8 : out = float32(skimage.transform.resize(img / 255.0, (Ho, Wo))) at skimage 0.19 / 0.20's defaults (order 1, mode 'reflect', clip,
 *                      anti_aliasing where a side shrinks) for img uint8 [bs][H][W][3]; out float32 [bs][3][Ho][Wo] (chw 1) or [bs][Ho][Wo][3] (chw 0).  Both
 *                      of skimage's steps (scipy.ndimage.gaussian_filter at sigma = max(0, (in / out - 1) / 2), truncate 4, mode 'mirror'; scipy.ndimage.zoom
 *                      at order 1, mode 'mirror', grid_mode=True) are linear and separable: the caller passes their product per axis, made on the host in
 *                      float64, as start int32 [dst], count int32 [dst], weight float64 [dst][T] (T = Ty, Tx: the widest count of the axis, 1 ..
 *                      E4S_SK_MAX_TAPS; rows padded with zeros).  v = double(byte) / 255.0; tmp[r][x] = sum_k xweight[x][k] v[r][xstart[x] + k], then
 *                      out[y][x] = sum_k yweight[y][k] tmp[ystart[y] + k][x]: float64, one rounding per product and per sum, ascending k from 0.0; clipped
 *                      to [min, max] / 255.0 of the sample's own bytes (all channels together); one conversion to float32.  part uint8 [bs][64][2] is
 *                      written by the call's first kernel (the byte range in 64 pieces) and read by its second.  A workgroup owns 16 x 32 output pixels;
 *                      where their source rows number at most 80 every source row is filtered along x once into LDS, otherwise the pixels are formed
 *                      directly in the same order: both forms give the same bits.  start and count are clamped to the source on the device: no table
 *                      content makes an access leave a tensor.  The weight tables (float64 behind a void pointer) are 8-byte aligned.
 *   e4s_frames_u8    : out uint8 [n][H][W][3] = the truncation toward zero of the float32 product x * 255.0f clamped to 0 .. 255 (a NaN gives 0), for x
 *                      float32 [n][3][H][W]: numpy's (pred * 255).astype(np.uint8) on values in [0, 1].  flip != 0 stores the channels reversed.
 * Plain vector loads and stores, no atomics, no host synchronisation, no scratch memory, grids from shapes alone: the calls can be captured in a graph.
 * bs == 0 / n == 0 returns at once. */
#define E4S_SK_MAX_TAPS 1024 /* composite taps per destination index a resize table may hold: a shrink of about 255 : 1 */
E4S_API int e4s_sk_resize_u8(float* out, uint8_t* part, const uint8_t* img, const int* ystart, const int* ycount, const void* yweight, int Ty,
                             const int* xstart, const int* xcount, const void* xweight, int Tx, int bs, int H, int W, int Ho, int Wo, int chw, void* stream);
E4S_API int e4s_frames_u8(uint8_t* out, const float* x, int n, int H, int W, int flip, void* stream);

/* f25: face inpainting, stage 1 — what FaceInpaintingArch.forward (swap_face_fine/gcfsr_arch.py:1347-1540) and the ends of inpainting()
 * (swap_face_fine/face_inpainting.py:21-51) need beside e4s_upfirdn2d, e4s_conv2d(_sb), e4s_grouped_linear, e4s_style_demod_batched, the single-region modulated
 * convolutions and e4s_region_torgb; csrc/gcfsr.hip.
 *   e4s_gcfsr_input           : x [bs][4][S][S]: planes 0 .. 2 = float32(double(byte) / 255.0) * (1 - m) of img uint8 [bs][S][S][3], plane 3 = m, for the hole mask
 *                               uint8 [bs][S][S] (0 = keep, anything else = hole).  count [bs] = the hole pixels of a sample, summed in two levels of integers
 *                               (part int32 [bs][64] is written by the call's first kernel and read by its second); in_size [bs] = float(count) / float(S S), one
 *                               correctly rounded division of two exact operands (S <= 4096).
 *   e4s_gcfsr_condition       : for every level l (w1, b1, w2, b2: HOST arrays of `levels` device pointers to condition_scale1/2[l].weight [C_l][1] and .bias [C_l];
 *                               channels: HOST int [levels]) and sample b: s1 = fl(w1 c) + b1, s2 = fl(w2 c) + b2 with c = in_size[b]; n = fl(fl(fl(s1 s1) + fl(s2 s2))
 *                               + 1e-8f); r = 1 / sqrt(n) (IEEE square root, then IEEE division); s1n = s1 r, s2n = s2 r.  The tables are [bs][sum C_l], the levels
 *                               side by side in the order given.  Norm2Scale (gcfsr_arch.py:702-705) up to rsqrt's last bit.  At most 8 levels.
 *   e4s_gcfsr_scale_shift_act : y [bs][C][hw] <- lrelu(fl(fl(fl(y s1n[b][c]) + fl(shift[b][c][p] s2n[b][c])) + bias[c]), 0.2) * float32(sqrt 2) in place: the tail
 *                               of StyleConv_norm_scale_shift.forward (:741-744) behind the modulated convolution and the noise.  s1n / s2n point at the level's
 *                               first channel in the tables above, table_stride is the tables' row length.  16-byte accesses when hw % 4 == 0 and y and shift are
 *                               16-byte aligned, single elements otherwise, the same bits both ways.
 *   e4s_gcfsr_tail            : out uint8 [bs][S][S][3] = rint(v * 255.0f), half to even, with v = float32(double(byte) / 255.0) outside the hole and
 *                               clamp(img, 0, 1) inside it (x (1 - m) + o m for m in {0, 1}); img float32 [bs][3][S][S], in_u8 [bs][S][S][3], mask [bs][S][S].
 *   e4s_cv_mask_support       : out uint8 [bs][S][S] = 1 where any mask value of source rows ystart[y] .. ystart[y] + ycount[y] - 1 and columns xstart[x] ..
 *                               xstart[x] + xcount[x] - 1 is > 0, else 0: (cv2.resize(mask.astype(float64), (S, S)) > 0) for a non-negative mask [bs][H][W]
 *                               (float32: is_f32 != 0, else uint8), given the taps with a non-zero weight, made on the host (e4s2024_amd/ops_inpaint.py).  start is
 *                               clamped to the mask and count to 1 .. 2 on the device: no table content makes an access leave a tensor.
 * Plain vector loads and stores, no atomics, no host synchronisation, grids from shapes alone: the calls can be captured in a graph.  bs == 0 returns at once. */
E4S_API int e4s_gcfsr_input(float* x, int* count, float* in_size, int* part, const uint8_t* img, const uint8_t* mask, int bs, int S, void* stream);
E4S_API int e4s_gcfsr_condition(float* s1n, float* s2n, const float* in_size, const float* const* w1, const float* const* b1, const float* const* w2,
                                const float* const* b2, const int* channels, int levels, int bs, void* stream);
E4S_API int e4s_gcfsr_scale_shift_act(float* y, const float* shift, const float* s1n, const float* s2n, const float* bias, int bs, int C, int hw,
                                      int64_t table_stride, void* stream);
E4S_API int e4s_gcfsr_tail(uint8_t* out, const float* img, const uint8_t* in_u8, const uint8_t* mask, int bs, int S, void* stream);
E4S_API int e4s_cv_mask_support(uint8_t* out, const void* mask, int is_f32, const int* ystart, const int* ycount, const int* xstart, const int* xcount, int bs,
                                int H, int W, int S, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* E4S_HIP_H */
