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

/* ------------------------------------------------------------------------------------------
 * Train-mode BatchNorm for a conv trainer: batch statistics. Off unless switched on.
 *
 * axt_conv_trainer_set_batch_stats: on != 0 makes the following _forward calls normalise with the statistics of their own
 *   batch; 0 returns to the running statistics as they then stand. momentum in (0, 1], else AXT_EINVAL (torch's default:
 *   0.1). The first switch on allocates 4 * Co floats (_device_bytes grows then); a handle that never asks holds what it
 *   held and launches what it launched. _step and _input_grad follow the mode of the _forward whose stash they read.
 * With the mode on, per channel over the n = B*H*W values of z = conv3x3(x) + bias:
 *   _forward: mu = sum z / n; var = sum (z - mu)^2 / n in a second pass over z (biased; not E[z^2] - mu^2);
 *     zhat = (z - mu) / sqrt(var + 1e-5), y = gamma zhat + beta, d_feat = y > 0 ? y : 0.1 y. Then, once per _forward:
 *     running_mean = (1 - momentum) running_mean + momentum mu, running_var = (1 - momentum) running_var + momentum var
 *     n / (n - 1), and the count of such forwards grows by one. n < 2: AXT_EINVAL before anything is launched.
 *   _step: dy = dF * (y > 0 ? 1 : 0.1), dbeta = sum dy, dgamma = sum dy zhat,
 *     dz = gamma / sqrt(var + 1e-5) * (dy - dbeta / n - zhat dgamma / n); dW from this dz as before. dbias is 0 by
 *     definition (sum dz vanishes identically), so conv.bias takes Adam steps of its weight decay alone.
 *   _input_grad: d_dx from the same dz, which it writes into the handle's dz scratch (no parameter, moment or statistic
 *     changes; _step forms the same dz again): calling it before _step leaves _step's results byte-identical.
 *   One workgroup per channel; thread t sums r = t, t + 256, ... of r = b*H*W + h*W + w, the 256 partial sums meet in a
 *   fixed binary tree. No atomics: byte-identical from run to run.
 * axt_conv_trainer_read_stats: device -> host, synchronous; any pointer may be NULL. running_mean, running_var [Co] as
 *   they stand, the number of forwards that ran with batch statistics (what num_batches_tracked has grown by), and the
 *   mean and biased variance [Co] of the last such forward (AXT_EINVAL when asked for before there was one).
 * ------------------------------------------------------------------------------------------ */
int axt_conv_trainer_set_batch_stats(axt_conv_trainer *tr, int on, double momentum);
int axt_conv_trainer_read_stats(const axt_conv_trainer *tr, float *h_running_mean, float *h_running_var,
                                int64_t *num_batches_tracked, float *h_batch_mean, float *h_batch_var);
int axt_maxpool2_forward(const float *d_in, int64_t n_maps, int H, int W, float *d_out, void *stream);
int axt_maxpool2_backward(const float *d_in, const float *d_dout, int64_t n_maps, int H, int W, float *d_din, void *stream);

#endif
