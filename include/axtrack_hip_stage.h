/* axtrack_hip_stage.h -- included by axtrack_hip.h, which declares axt_conv_trainer and the integer types; not for inclusion
 * on its own. Same conventions: AXT_OK or a negative AXT_E* code, axt_last_error() for the text, `stream` a hipStream_t. */
#ifndef AXTRACK_HIP_STAGE_H
#define AXTRACK_HIP_STAGE_H

/* ------------------------------------------------------------------------------------------
 * Fine-tuning of the whole last conv stage (conv blocks 5, 6, the max-pool, conv block 7) with the head.
 *
 * axt_conv_trainer_input_grad: the gradient of the loss with respect to the rows _forward read. From d_dfeat
 *   [B, Co*H*W] (the gradient with respect to _forward's output of the same batch, same B), the z stashed by that _forward
 *   and the parameters as they stand: dz = dF * (y > 0 ? 1 : 0.1) * gamma / sqrt(var + 1e-5) with y recomputed from z by
 *   the forward's own expression (y == 0 takes 0.1), d_dx[b, ci, h, w] = sum_{co,ky,kx} dz[b, co, h-ky+1, w-kx+1]
 *   weight[co, ci, ky, kx] (positions outside the map contribute nothing), d_dx [B, Ci*H*W] in the order ci*H*W + h*W + w.
 *   Per output FMA chains of 16 terms in ascending (co, ky, kx), their sums added in ascending order; no atomics:
 *   byte-identical from call to call. Call it before _step, which moves gamma and the weights. dz is formed while the
 *   kernel stages its tiles and the sums stay in registers: it writes d_dx only and allocates nothing (_device_bytes
 *   stays), so calling it before _step leaves _step's results byte-identical. A B other than the last _forward's:
 *   AXT_EINVAL, as _step.
 *
 * axt_maxpool2_forward / _backward: nn.MaxPool2d(2, 2) on n_maps maps of H x W (2 <= H, W <= 32768, n_maps * H * W <=
 *   2^38, else AXT_EINVAL; n_maps = 0 does nothing), d_out [n_maps, H/2, W/2] (floored). _backward recomputes each window's winner from d_in -- the first maximum in the order
 *   (0,0), (0,1), (1,0), (1,1) under a strict >, so -0.0 and +0.0 tie and the first wins, as torch's CPU backward
 *   decides -- and writes every element of d_din [n_maps, H, W]: the window's d_dout at the winner, +0.0 elsewhere and in
 *   a trailing odd row or column. One thread per input element; no atomics, no scatter.
 * ------------------------------------------------------------------------------------------ */
int axt_conv_trainer_input_grad(axt_conv_trainer *tr, const float *d_dfeat, int B, float *d_dx, void *stream);
int axt_maxpool2_forward(const float *d_in, int64_t n_maps, int H, int W, float *d_out, void *stream);
int axt_maxpool2_backward(const float *d_in, const float *d_dout, int64_t n_maps, int H, int W, float *d_din, void *stream);

#endif
