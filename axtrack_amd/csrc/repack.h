// Device-side weight packing (repack.hip): the launchers behind axt_detector_load_conv_block / _load_linear and the
// lazy packing of axt_detector_set_arith after a device load. Internal to libaxtrack_hip.so.
//
// Every launcher writes the WHOLE image it names, padding included, from f32 tensors in device memory, asynchronously on
// `st`, and allocates nothing. The layouts are the host packers' in cnn.hip (pack_conv, pack_wino, pack_bf16x3, the
// linear transpose of axt_detector_create), and the values are theirs byte for byte: f64 where they use f64, every
// product and sum rounded on its own (no contraction), rounded once to f32.
#pragma once
#include "axt_common.h"

// sizes of the images in elements, as the host packers size them (cnn.hip asserts them against its kernels' geometry)
constexpr int kRepackWinoChunk = 16 * 5 * 64 * 2;     // floats per (group of 80 output channels, chunk of 8 input channels)
constexpr int kRepackB3Chunk = 5 * 3 * 4 * 80 * 8;    // bf16 per chunk of 16 input channels
inline size_t axt_repack_s2_floats(int cin, int cout) { return (size_t)cin * 9 * 4 * ((cout / 4 + 3) / 4 * 4); }
inline size_t axt_repack_s1_floats(int cin, int cch, int npadw, int ngroups) { return (size_t)ngroups * (cin / cch) * 9 * cch * npadw; }
inline size_t axt_repack_wino_floats(int cin, int cout) { return (size_t)(cout / 80) * (cin / 8) * kRepackWinoChunk; }
inline size_t axt_repack_b3_bf16(int cin) { return (size_t)((cin + 15) / 16) * kRepackB3Chunk; }

// BatchNorm fold of one block: wfold [cout][cin][3][3] = w * sc, bias [cout] = (b - mean) * sc + beta,
// sc = gamma / sqrt(var + 1e-5)
int axt_repack_fold(const float *w, const float *b, const float *gamma, const float *beta, const float *mean, const float *var,
                    int cin, int cout, float *wfold, float *bias, hipStream_t st);
// wfold -> [ci*9 + ky*3 + kx][co % 4][ngp] (stride-2 blocks), axt_repack_s2_floats floats
int axt_repack_direct_s2(const float *wfold, int cin, int cout, float *out, hipStream_t st);
// wfold -> [group of nt*16 output channels][chunk of cch input channels][krow][npadw] (stride-1 blocks)
int axt_repack_direct_s1(const float *wfold, int cin, int cout, int cch, int nt, int npadw, int ngroups, float *out,
                         hipStream_t st);
// wfold -> U = G g G^T in pack_wino's LDS order; cin a multiple of 8, cout of 80
int axt_repack_wino(const float *wfold, int cin, int cout, float *out, hipStream_t st);
// wfold [80][cin][3][3] -> hi | mid | lo bf16 planes in pack_bf16x3's LDS order; out 16-byte aligned
int axt_repack_b3(const float *wfold, int cin, unsigned *out, hipStream_t st);
// w [fout][fin] -> out [fin][fpad], columns fout..fpad-1 zero; fin and fpad multiples of 64, 16-byte aligned pointers
int axt_repack_linear(const float *w, int fin, int fout, int fpad, float *out, hipStream_t st);

// cnn.hip: what the trainers' exports check their own sizes against
int axt_detector_conv_spec(int li, int *cin, int *cout, int *stride);       // li 0..7, else AXT_EINVAL
int axt_detector_linear_spec(int layer, int *fin, int *fout);               // layer 0..2, else AXT_EINVAL
