/* axtrack_hip_repack.h -- included by axtrack_hip.h, which declares axt_detector, axt_conv_trainer and axt_head_trainer; not
 * for inclusion on its own. Same conventions: AXT_OK or a negative AXT_E* code, axt_last_error() for the text, `stream` a
 * hipStream_t. */
#ifndef AXTRACK_HIP_REPACK_H
#define AXTRACK_HIP_REPACK_H

/* ------------------------------------------------------------------------------------------
 * Weights into a live detector without leaving the device (csrc/repack.hip).
 *
 * What axt_detector_create does on the host for all tensors at once -- fold BatchNorm into the convolution in f64, lay the
 * result out for each conv kernel, transpose the linear layers -- these calls do on the device for one block from f32
 * tensors in state-dict layout that are already in device memory. The images they write are byte for byte the ones
 * axt_detector_create would have uploaded for the same tensors: sc = gamma / sqrt(var + 1e-5), weight' = weight * sc,
 * bias' = (bias - mean) * sc + beta, every operation in f64 and rounded on its own, one rounding to f32.
 *
 * All four are asynchronous on `stream` and make no copy to or from the host; a forward pass issued on the same stream
 * afterwards reads the new weights. A pass on another stream must be ordered against the load by the caller. A null
 * pointer or an index out of range: AXT_EINVAL with the function's name in axt_last_error(), before any launch.
 *
 * axt_detector_load_conv_block: conv block li (0..7 of the package's numbering) from d_weight [Co, Ci, 3, 3], d_bias,
 *   d_gamma, d_beta, d_mean, d_var [Co] (conv.weight, conv.bias, batchnorm.weight, batchnorm.bias, running_mean,
 *   running_var). Rewrites the block's folded bias, its direct-convolution image and whichever of its Winograd and bf16x3
 *   images exist. The block's first load allocates a device copy of its folded weights (Co*Ci*9 floats, counted in
 *   axt_detector_device_bytes) and drops the host copy; an image that a later axt_detector_set_arith has to allocate is
 *   packed from that device copy by the same kernels, so after a load the detector is at every moment the one
 *   axt_detector_create would have made from the same tensors. That first allocation is the only thing that is not
 *   stream-ordered. A detector that never sees a load keeps the host packers.
 * axt_detector_load_linear: linear layer 0..2 (fcs.1, fcs.3, fcs.5) from d_weight [out, in] and d_bias [out]: the
 *   transpose [in][out padded to the GEMM's tile] with zeros in the padded columns, and the bias. Both pointers 16-byte
 *   aligned.
 * axt_conv_trainer_export: axt_detector_load_conv_block(det, li, ...) from the trainer's own device tensors as they stand
 *   on `stream`: the four trained tensors and the running statistics, the moved ones once batch statistics were switched
 *   on. The trainer's Ci, Co and stride must be block li's, else AXT_EINVAL. A trainer that never ran with batch
 *   statistics keeps running_var on the host; its first export uploads it once (Co floats, counted in
 *   axt_conv_trainer_device_bytes).
 * axt_head_trainer_export: axt_detector_load_linear for the three layers from the trainer's master weights; its K0, H1,
 *   H2, NOUT must be the detector's 40960, 1024, 1024, 432, else AXT_EINVAL.
 * ------------------------------------------------------------------------------------------ */
int axt_detector_load_conv_block(axt_detector *det, int li, const float *d_weight, const float *d_bias, const float *d_gamma,
                                 const float *d_beta, const float *d_mean, const float *d_var, void *stream);
int axt_detector_load_linear(axt_detector *det, int layer, const float *d_weight, const float *d_bias, void *stream);
int axt_conv_trainer_export(axt_conv_trainer *tr, axt_detector *det, int li, void *stream);
int axt_head_trainer_export(axt_head_trainer *tr, axt_detector *det, void *stream);

#endif
