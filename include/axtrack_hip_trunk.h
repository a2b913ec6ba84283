/* axtrack_hip_trunk.h -- included by axtrack_hip.h, which declares axt_conv_trainer and the integer types; not for inclusion
 * on its own. Same conventions: AXT_OK or a negative AXT_E* code, axt_last_error() for the text, `stream` a hipStream_t. */
#ifndef AXTRACK_HIP_TRUNK_H
#define AXTRACK_HIP_TRUNK_H

/* ------------------------------------------------------------------------------------------
 * Fine-tuning of every conv block, the stride-2 front included.
 *
 * axt_conv_trainer_create_strided: an axt_conv_trainer for Conv2d(Ci, Co, 3, stride, padding 1) + BatchNorm2d +
 *   LeakyReLU(0.1) on input maps of Hin x Win; the output map is Hout = (Hin - 1) / stride + 1 (floored), the same for W.
 *   The handle is the type axt_conv_trainer_create makes: _forward, _step, _input_grad, _set_batch_stats, _read_* and
 *   _destroy work on it unchanged, with rows of Ci*Hin*Win floats in (d_in, d_dx) and Co*Hout*Wout out (d_feat, d_dfeat).
 *   Limits: stride 1 or 2; 1 <= Ci, Co <= 512; 1 <= Hin, Win <= 512; Hout, Wout <= 256 with stride 2 and <= 128 with
 *   stride 1; 1 <= max_batch <= 64. Anything else, or a null pointer: AXT_EINVAL before any device call, with this
 *   function's name in axt_last_error(). With stride 1 on a map axt_conv_trainer_create takes, the handle is the one that
 *   call makes: the same kernels, the same split of the weight gradient, the same bytes.
 *   Forward and weight gradient read x[b, ci, h*stride + ky - 1, w*stride + kx - 1], 0 outside the input map. The input
 *   gradient at stride 2: d_dx[b, ci, hi, wi] = sum over (co, ky, kx) ascending of weight[co, ci, ky, kx] *
 *   dz[b, co, (hi - ky + 1) / 2, (wi - kx + 1) / 2] for those taps where both numerators are even and the position lies in
 *   the output map; the other taps enter the same FMA chains of 16 as +0.0, so every sum keeps one order that depends on
 *   the sizes and B only. No atomics. On maps beyond 64 x 64 the weight gradient's sum over (b, h, w) is split into more
 *   runs (up to Hout*Wout / 64, at most 1024, the slabs within 16 M floats); the split depends on the sizes and B only.
 *
 * axt_tile_stacks: the input of conv block 0 for a batch of items, gathered from the frames. d_index i32 [B] holds item
 *   numbers item = f*n_tiles + k in the order of axt_cnn_features_frames (frame t0 + f, tile k of h_tile_yx); d_out f32
 *   [B, 5, 512, 512]: channel c of item (f, k) is frames[t0 + f + c], rows from tile_yx[2k]*512, columns from
 *   tile_yx[2k+1]*512, +0.0 beyond H or W. One thread per float4 where W is a multiple of 4 and both pointers are 16-byte
 *   aligned, else per float. Asynchronous on `stream`, no copy, nothing allocated. d_frames, T_all, H, W, t0, n_frames,
 *   h_tile_yx, n_tiles as axt_cnn_features_frames takes them (1 <= n_frames <= 2^22, 1 <= H, W <= 32768, every tile's
 *   origin inside the frame: the products with 512 are formed in 64 bits), 1 <= B <= 1024, else AXT_EINVAL. The item
 *   numbers are on the device, so the call cannot refuse one: an item outside [0, n_frames*n_tiles) gives a stack of +0.0
 *   and reads nothing.
 *
 * axt_cnn_block_features_frames (axtrack_hip.h) also takes block = 2: d_feat f32 [n_frames*n_tiles, 327680] is
 *   [item, 80, 64, 64] NCHW, the output of ConvBlock_2 after its max-pool, copied from the detector's own buffer after every
 *   chunk; conv blocks 3..7 do not run.
 * ------------------------------------------------------------------------------------------ */
int axt_conv_trainer_create_strided(int Ci, int Co, int Hin, int Win, int stride, const float *h_weight, const float *h_bias,
                                    const float *h_gamma, const float *h_beta, const float *h_mean, const float *h_var,
                                    int max_batch, axt_conv_trainer **out);
int axt_tile_stacks(const float *d_frames, int T_all, int H, int W, int t0, int n_frames, const int32_t *h_tile_yx,
                    int n_tiles, const int32_t *d_index, int B, float *d_out, void *stream);

#endif
