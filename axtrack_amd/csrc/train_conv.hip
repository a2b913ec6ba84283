// train_conv.hip -- fine-tuning of one convolutional block (Conv2d 3x3 pad 1 + BatchNorm2d + LeakyReLU(0.1), model.py:5-18)
// together with the linear head of train.hip: the block's forward pass in training form (unfolded BatchNorm, f32, the
// weights change every step), its backward pass from the head's input gradient, and torch.optim.Adam with L2 weight decay
// on conv.weight, conv.bias, batchnorm.weight and batchnorm.bias. BatchNorm uses its running statistics and leaves them
// alone, or, after axt_conv_trainer_set_batch_stats, the statistics of each batch as nn.BatchNorm2d does in train mode (the
// kernels at the end of the list). DESIGN.md 6.8e.
//
// Both products run over the im2col matrix X(q, r) of the batch, never stored:
//   q = ci*9 + ky*3 + kx (the order of conv.weight's last three dimensions), r = b*H*W + h*W + w,
//   X(q, r) = x[row(b)][ci][h*s+ky-1][w*s+kx-1], 0 outside the input map, with the stride s = 1 or 2 a template parameter
//   of the three products (s = 1 is the code it was) and (h, w) on the output map of (Hin - 1) / s + 1 rows.
// Kernels
//   conv_fwd_k       z[co][r] = sum_q W[co][q] X(q, r) + bias in ascending q (ci, ky, kx): every run of 16 q is one f32 FMA
//                    chain from zero, the runs' sums are added in ascending order. Then y = gamma (z - mean) inv_sigma + beta,
//                    F = y > 0 ? y : 0.1 y. 64 co x 64 r per workgroup from LDS tiles 16 deep, 4 x 4 outputs per thread.
//                    Writes z (the stash) and F.
//   conv_bn_back_k   one workgroup per output channel: dy = dF * (y > 0 ? 1 : 0.1) with y recomputed from the stashed z by
//                    the forward's own expression (the sign information), dz = dy * gamma * inv_sigma stored for the
//                    weight gradient, and dgamma = sum dy zhat, dbeta = sum dy, dbias = sum dz; then Adam on the three
//                    per-channel parameters. Thread t sums r = t, t+256, ... of r = b*H*W + h*W + w in that order (b
//                    ascending); the 256 partial sums meet in a fixed binary tree.
//   conv_wgrad_k     slab[s][co][q] = sum over the s-th run of r of dz[co][r] X(q, r): the same tiles with the roles of q
//                    and r exchanged, in ascending r (b, h, w): chains of 16 from zero, their sums added in ascending order.
//                    The split of r into runs depends on the sizes and B only (plan_wgrad).
//   conv_adam_w_k    per weight: g = slab[0] + slab[1] + ... in ascending s, then the Adam update of w, m, v in place
// For a stage of several blocks (conv blocks 5, 6, the max-pool, conv block 7), the gradient handed to the block in front:
//   conv_dgrad_k     dx[ci][r] = sum_q W[co][ci][ky][kx] dz(q, r) with q = co*9 + ky*3 + kx and dz(q, r) =
//                    dz[b][co][h-ky+1][w-kx+1], 0 outside the map: conv_fwd_k's product with Co*9 as the depth, the weights
//                    read transposed and flipped where they lie. dz is formed while staging, from dF, the stashed z and
//                    gamma as it stands, by conv_bn_back_k's expressions (DzFromDF), or with batch statistics read from
//                    the dz buffer that bn_batch_back_k<false> filled (DzStored): one kernel, templated on that source;
//                    the same chains of 16 in ascending q. 64 ci x 64 r per workgroup. Reads nothing that the step
//                    writes except the parameters: it runs before the step. At stride 2 r walks the input map and a tap
//                    contributes where (h-ky+1, w-kx+1) are both even and their halves lie in the output map; every other q
//                    of the ascending walk is staged as +0.0, so the chains keep their order and nothing is scattered.
//   maxpool2_fwd_k   nn.MaxPool2d(2, 2), one thread per output element
//   maxpool2_bwd_k   one thread per input element recomputes its window's winner (the first maximum under a strict >) and
//                    writes the window's gradient or +0.0: every element is written, nothing is scattered
//   tile_stacks_k    the raw [B][5][512][512] stacks of a batch of (frame, tile) items gathered from the frames, the input of
//                    conv block 0: one thread per float4 (per float where the rows are not 16-byte aligned)
// Batch statistics (train-mode BatchNorm), n = B*H*W elements per channel, one workgroup per output channel each:
//   bn_batch_fwd_k   from the z that conv_fwd_k stashed: mu = sum z / n, then var = sum (z - mu)^2 / n in a second pass (never
//                    E[z^2] - mu^2), inv = 1 / sqrt(var + 1e-5); running_mean and running_var move by the momentum (var
//                    times n / (n - 1)), and the eval-mode 1 / sqrt(running_var + 1e-5) follows; a third pass overwrites F
//                    with leaky(bn_y(z, mu, inv, gamma, beta)).
//   bn_batch_back_k  pass 1: dbeta = sum dy, dgamma = sum dy zhat with dy and zhat from bn_y on (mu, inv); pass 2:
//                    dz = gamma inv (dy - dbeta / n - zhat dgamma / n) into the dz buffer. With kAdam: Adam on gamma and
//                    beta, and on conv.bias with the gradient 0 that sum dz is by definition. Without: dz only, for
//                    conv_dgrad_k<DzStored>. The sums follow conv_bn_back_k: thread t takes r = t, t + 256, ..., the 256
//                    partial sums meet in a fixed binary tree (sum256, which all three per-channel kernels share).
// Determinism: no atomics; every sum has one fixed order that depends on Ci, Co, H, W and B only.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "adam.h"
#include "axt_common.h"
#include "repack.h"

namespace {

constexpr int kMaxB = 64, kMaxC = 512, kMaxHW = 64;     // the limits include/axtrack_hip.h states
constexpr int TM = 64, TN = 64, TK = 16, TPAD = 68;     // output channels and columns per workgroup, tile depth, LDS pitch
constexpr int kMaxPoolHW = 32768;                       // the max-pool's limits: a map's side, and the elements of a call
constexpr int64_t kMaxPoolElems = (int64_t)1 << 38;     // (one thread each, 256 per workgroup, below 2^31 workgroups)
constexpr float kSlope = 0.1f;
constexpr double kBnEps = 1e-5;

// H, W: the output map, on which z, dz and the per-channel kernels work. Hi, Wi: the input map, which only the three
// products see: H = (Hi - 1) / stride + 1, so with stride 1 the two are one
struct Geom { int Ci, Co, H, W, HW, K9, Hi, Wi, HWi, stride; };
constexpr int kMaxInHW = 512, kMaxOutS1 = 128, kMaxOutS2 = 256;   // the limits of axt_conv_trainer_create_strided

// y of BatchNorm in the one form both passes use, so that the backward pass sees the forward's sign
__device__ inline float bn_y(float z, float mean, float inv_sigma, float gamma, float beta, float *zhat)
{
    const float zh = __fmul_rn(__fsub_rn(z, mean), inv_sigma);
    *zhat = zh;
    return fmaf(gamma, zh, beta);
}

__device__ inline float leaky(float y) { return y > 0.f ? y : kSlope * y; }

// the gradient with respect to y from dF, the gradient with respect to leaky(y): y recomputed from the stashed z by bn_y, so
// the sign test is the forward's (y == 0 takes the slope)
__device__ inline float leaky_back(float z, float dF, float mean, float inv_sigma, float gamma, float beta, float *zhat)
{
    const float y = bn_y(z, mean, inv_sigma, gamma, beta, zhat);
    return y > 0.f ? dF : kSlope * dF;
}

// the offset of element r = b*HW + p of channel c in an array [B][C][HW]. The per-channel kernels walk it with thread t on
// r = t, t + 256, ... (b ascending)
__device__ inline size_t chan_off(int r, int C, int HW, int c)
{
    const int b = r / HW, p = r - b * HW;
    return ((size_t)b * C + c) * HW + p;
}

// the sums of v[0..N-1] over the workgroup's 256 threads in one fixed binary tree (one set of barriers for all N), handed to
// every thread; red may be used again afterwards
template <int N>
__device__ inline void sum256(float (&v)[N], float (*red)[256], int tid)
{
    for (int q = 0; q < N; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            for (int q = 0; q < N; ++q) red[q][tid] += red[q][tid + w];
        __syncthreads();
    }
    for (int q = 0; q < N; ++q) v[q] = red[q][0];
    __syncthreads();
}

__device__ inline float sum256(float v, float (*red)[256], int tid)
{
    float s[1] = {v};
    sum256(s, red, tid);
    return s[0];
}

// threads 0..2: Adam on conv.bias, batchnorm.weight, batchnorm.bias of channel co with the gradients grad[0..2] (p, m, v:
// [3][Co] in that order). Every thread of the workgroup has read the parameters it needs by the time this is called.
__device__ inline void adam_bias_gamma_beta(int tid, int co, int Co, const float (&grad)[3], float *__restrict__ bias,
                                            float *__restrict__ gamma, float *__restrict__ beta, float *__restrict__ mom_m,
                                            float *__restrict__ mom_v, const AdamArgs &a)
{
    if (tid >= 3) return;
    float *param = tid == 0 ? bias : tid == 1 ? gamma : beta;
    float w = param[co], m = mom_m[tid * Co + co], v = mom_v[tid * Co + co];
    adam1(tid == 0 ? grad[0] : tid == 1 ? grad[1] : grad[2], w, m, v, a);
    param[co] = w;
    mom_m[tid * Co + co] = m;
    mom_v[tid * Co + co] = v;
}

// x[row][ci][h*S+ky-1][w*S+kx-1] with q = ci*9 + ky*3 + kx; (b, h, w) of the output map already split; 0 outside the
// input map. S: the stride, 1 or 2, at compile time: S = 1 is the code it was.
template <int S>
__device__ inline float im2col(const float *__restrict__ x, size_t row, const Geom &g, int q, int h, int w)
{
    const int ci = q / 9, tap = q - ci * 9, ky = tap / 3, kx = tap - ky * 3;
    if (S == 1) {
        const int hh = h + ky - 1, ww = w + kx - 1;
        if (hh < 0 || hh >= g.H || ww < 0 || ww >= g.W) return 0.f;
        return x[(row * g.Ci + ci) * g.HW + hh * g.W + ww];
    }
    const int hh = h * S + ky - 1, ww = w * S + kx - 1;
    if (hh < 0 || hh >= g.Hi || ww < 0 || ww >= g.Wi) return 0.f;
    return x[(row * g.Ci + ci) * g.HWi + hh * g.Wi + ww];
}

// acc[i][j] += (sum_k As[k][tm*4+i] * Bs[k][tn*4+j]): the tile's 16 products in one FMA chain from zero, k ascending, and
// that sum added to the running total -- a two-level sum whose error grows with sqrt(K / 16) + 4 instead of sqrt(K)
__device__ inline void tile_fma(const float (*As)[TPAD], const float (*Bs)[TPAD], int tm, int tn, float (&total)[4][4])
{
    float acc[4][4] = {};
#pragma unroll
    for (int k = 0; k < TK; ++k) {
        const float4 a4 = *reinterpret_cast<const float4 *>(&As[k][tm * 4]);
        const float4 b4 = *reinterpret_cast<const float4 *>(&Bs[k][tn * 4]);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) total[i][j] += acc[i][j];
}

// grid (r tiles, co tiles). x: table [., Ci*Hi*Wi], rows picked by index (NULL: 0..B-1). z, F: [B][Co][H*W].
template <int S>
__global__ __launch_bounds__(256) void conv_fwd_k(const float *__restrict__ x, const int *__restrict__ index, int B, Geom g,
                                                  const float *__restrict__ Wt, const float *__restrict__ bias,
                                                  const float *__restrict__ gamma, const float *__restrict__ beta,
                                                  const float *__restrict__ mean, const float *__restrict__ inv_sigma,
                                                  float *__restrict__ z, float *__restrict__ F)
{
    __shared__ __attribute__((aligned(16))) float As[TK][TPAD];      // W[co][q] as [q][co]
    __shared__ __attribute__((aligned(16))) float Bs[TK][TPAD];      // X(q, r) as [q][r]
    const int tid = threadIdx.x, tm = tid / 16, tn = tid % 16;
    const int r0 = blockIdx.x * TN, co0 = blockIdx.y * TM, R = B * g.HW;
    // the column this thread stages: r is fixed, q walks
    const int rl = tid % TN, r = r0 + rl;
    const bool r_ok = r < R;
    const int b = r_ok ? r / g.HW : 0, p = r - b * g.HW, h = p / g.W, w = p - h * g.W;
    const size_t row = r_ok ? (size_t)(index ? index[b] : b) : 0;
    float acc[4][4] = {};
    for (int q0 = 0; q0 < g.K9; q0 += TK) {
        for (int i = tid; i < TM * TK; i += 256) {
            const int k = i % TK, c = i / TK;
            As[k][c] = (co0 + c < g.Co && q0 + k < g.K9) ? Wt[(size_t)(co0 + c) * g.K9 + q0 + k] : 0.f;
        }
        for (int k = tid / TN; k < TK; k += 256 / TN)
            Bs[k][rl] = (r_ok && q0 + k < g.K9) ? im2col<S>(x, row, g, q0 + k, h, w) : 0.f;
        __syncthreads();
        tile_fma(As, Bs, tm, tn, acc);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + tm * 4 + i;
        if (co >= g.Co) continue;
        const float bi = bias[co], ga = gamma[co], be = beta[co], me = mean[co], is = inv_sigma[co];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rr = r0 + tn * 4 + j;
            if (rr >= R) continue;
            const size_t o = chan_off(rr, g.Co, g.HW, co);
            const float zz = acc[i][j] + bi;
            float zh;
            z[o] = zz;
            F[o] = leaky(bn_y(zz, me, is, ga, be, &zh));
        }
    }
}

// grid (Co). dF, z, dz: [B][Co][H*W]. Updates bias, gamma, beta and their moments (p, m, v: [3][Co] in that order).
__global__ __launch_bounds__(256) void conv_bn_back_k(const float *__restrict__ dF, const float *__restrict__ z, int B, Geom g,
                                                      float *__restrict__ bias, float *__restrict__ gamma,
                                                      float *__restrict__ beta, const float *__restrict__ mean,
                                                      const float *__restrict__ inv_sigma, float *__restrict__ mom_m,
                                                      float *__restrict__ mom_v, float *__restrict__ dz, AdamArgs a)
{
    __shared__ float red[3][256];
    const int tid = threadIdx.x, co = blockIdx.x;
    const float ga = gamma[co], be = beta[co], me = mean[co], is = inv_sigma[co];
    const float fold = ga * is;
    float s[3] = {};                                                   // dbias, dgamma, dbeta
    for (int r = tid; r < B * g.HW; r += 256) {
        const size_t o = chan_off(r, g.Co, g.HW, co);
        float zh;
        const float dy = leaky_back(z[o], dF[o], me, is, ga, be, &zh);
        const float d = dy * fold;
        s[1] = fmaf(dy, zh, s[1]);
        s[2] += dy;
        s[0] += d;
        dz[o] = d;
    }
    sum256(s, red, tid);
    adam_bias_gamma_beta(tid, co, g.Co, s, bias, gamma, beta, mom_m, mom_v, a);
}

// grid (q tiles, co tiles, splits). slab [splits][Co][K9].
template <int S>
__global__ __launch_bounds__(256) void conv_wgrad_k(const float *__restrict__ x, const int *__restrict__ index, int B, Geom g,
                                                    const float *__restrict__ dz, int rchunk, float *__restrict__ slab)
{
    __shared__ __attribute__((aligned(16))) float As[TK][TPAD];      // dz[co][r] as [r][co]
    __shared__ __attribute__((aligned(16))) float Bs[TK][TPAD];      // X(q, r) as [r][q]
    const int tid = threadIdx.x, tm = tid / 16, tn = tid % 16;
    const int q0 = blockIdx.x * TN, co0 = blockIdx.y * TM, R = B * g.HW;
    const int r_begin = blockIdx.z * rchunk, r_end = min(R, r_begin + rchunk);
    const int kl = tid % TK;                                          // the r this thread stages within a tile
    float acc[4][4] = {};
    for (int r0 = r_begin; r0 < r_end; r0 += TK) {
        const int r = r0 + kl;
        const bool r_ok = r < r_end;
        const int b = r_ok ? r / g.HW : 0, p = r - b * g.HW, h = p / g.W, w = p - h * g.W;
        const size_t row = r_ok ? (size_t)(index ? index[b] : b) : 0;
        for (int c = tid / TK; c < TM; c += 256 / TK) {
            As[kl][c] = (r_ok && co0 + c < g.Co) ? dz[((size_t)b * g.Co + co0 + c) * g.HW + p] : 0.f;
            Bs[kl][c] = (r_ok && q0 + c < g.K9) ? im2col<S>(x, row, g, q0 + c, h, w) : 0.f;
        }
        __syncthreads();
        tile_fma(As, Bs, tm, tn, acc);
        __syncthreads();
    }
    float *dst = slab + (size_t)blockIdx.z * g.Co * g.K9;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + tm * 4 + i;
        if (co >= g.Co) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = q0 + tn * 4 + j;
            if (q < g.K9) dst[(size_t)co * g.K9 + q] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void conv_adam_w_k(float *__restrict__ W, float *__restrict__ M, float *__restrict__ V, int n,
                                                     const float *__restrict__ slab, int S, AdamArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float gsum = slab[i];
    for (int s = 1; s < S; ++s) gsum += slab[(size_t)s * n + i];
    float w = W[i], m = M[i], v = V[i];
    adam1(gsum, w, m, v, a);
    W[i] = w; M[i] = m; V[i] = v;
}

// The two sources of dz for conv_dgrad_k: dz at offset o of a [B][Co][H*W] array, in channel co.
// Formed from the stashed z and dF by conv_bn_back_k's expressions and from gamma as it stands (running statistics):
struct DzFromDF {
    const float *__restrict__ dF, *__restrict__ z, *__restrict__ gamma, *__restrict__ beta, *__restrict__ mean,
        *__restrict__ inv_sigma;
    __device__ float operator()(size_t o, int co) const
    {
        const float ga = gamma[co], is = inv_sigma[co];
        const float fold = ga * is;
        float zh;
        const float dy = leaky_back(z[o], dF[o], mean[co], is, ga, beta[co], &zh);
        return dy * fold;
    }
};
// Read from the dz buffer that bn_batch_back_k wrote (batch statistics):
struct DzStored {
    const float *__restrict__ dz;
    __device__ float operator()(size_t o, int) const { return dz[o]; }
};

// grid (r tiles, ci tiles). dx[b][ci][h][w] = sum_q Wt[co][ci][ky][kx] dz[b][co][h-ky+1][w-kx+1] in ascending q = co*9 + ky*3
// + kx, 0 outside the map: conv_fwd_k's product with Co*9 as the depth and the weights read transposed and flipped where they
// lie. dz: one of the two sources above; dx: [B][Ci][Hi*Wi].
// S = 2: r walks the input map, and tap (ky, kx) reaches output (ho, wo) = ((h - ky + 1) / 2, (w - kx + 1) / 2) where both
// numerators are even and (ho, wo) lies in the output map; every other q of the ascending walk is staged as +0.0, so the
// chains and their order are those of S = 1 and each dx has one writer.
template <class Dz, int S>
__global__ __launch_bounds__(256) void conv_dgrad_k(Dz dz, int B, Geom g, const float *__restrict__ Wt, float *__restrict__ dx)
{
    const int HWx = S == 1 ? g.HW : g.HWi, Wx = S == 1 ? g.W : g.Wi;
    __shared__ __attribute__((aligned(16))) float As[TK][TPAD];      // W[co][ci][tap] as [q][ci]
    __shared__ __attribute__((aligned(16))) float Bs[TK][TPAD];      // dz of the shifted position as [q][r]
    const int tid = threadIdx.x, tm = tid / 16, tn = tid % 16;
    const int r0 = blockIdx.x * TN, ci0 = blockIdx.y * TM, R = B * HWx, K = g.Co * 9;
    const int rl = tid % TN, r = r0 + rl;
    const bool r_ok = r < R;
    const int b = r_ok ? r / HWx : 0, p = r - b * HWx, h = p / Wx, w = p - h * Wx;
    float acc[4][4] = {};
    for (int q0 = 0; q0 < K; q0 += TK) {
        for (int i = tid; i < TM * TK; i += 256) {
            const int k = i % TK, c = i / TK, q = q0 + k, co = q / 9;
            As[k][c] = (ci0 + c < g.Ci && q < K) ? Wt[((size_t)co * g.Ci + ci0 + c) * 9 + (q - co * 9)] : 0.f;
        }
        for (int k = tid / TN; k < TK; k += 256 / TN) {
            const int q = q0 + k, co = q / 9, tap = q - co * 9, ky = tap / 3, kx = tap - ky * 3;
            int hh = h - ky + 1, ww = w - kx + 1;
            bool ok = r_ok && q < K;
            if (S == 2) {
                ok = ok && hh >= 0 && ww >= 0 && !((hh | ww) & 1);
                hh >>= 1;
                ww >>= 1;
            }
            ok = ok && hh >= 0 && hh < g.H && ww >= 0 && ww < g.W;
            Bs[k][rl] = ok ? dz(((size_t)b * g.Co + co) * g.HW + hh * g.W + ww, co) : 0.f;
        }
        __syncthreads();
        tile_fma(As, Bs, tm, tn, acc);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ci = ci0 + tm * 4 + i;
        if (ci >= g.Ci) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rr = r0 + tn * 4 + j;
            if (rr < R) dx[chan_off(rr, g.Ci, HWx, ci)] = acc[i][j];
        }
    }
}

// the winner of a 2 x 2 window as torch's CPU max_pool2d picks it: the first maximum in the order (0,0), (0,1), (1,0), (1,1)
// under a strict > (-0.0 and +0.0 tie), a NaN taking over. p: the window's top left element, W: the row pitch.
__device__ inline int pool_winner(const float *__restrict__ p, int W, float *value)
{
    const float v[4] = {p[0], p[1], p[W], p[W + 1]};
    int win = 0;
    float m = v[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (v[k] > m || v[k] != v[k]) { m = v[k]; win = k; }
    *value = m;
    return win;
}

// one thread per output element. in [n_maps][H][W], out [n_maps][H/2][W/2].
__global__ __launch_bounds__(256) void maxpool2_fwd_k(const float *__restrict__ in, size_t n_out, int H, int W,
                                                      float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int Ho = H / 2, Wo = W / 2;
    const size_t n = i / ((size_t)Ho * Wo);
    const int rem = (int)(i - n * Ho * Wo), ho = rem / Wo, wo = rem - ho * Wo;
    float m;
    (void)pool_winner(in + (n * H + 2 * ho) * W + 2 * wo, W, &m);
    out[i] = m;
}

// one thread per input element: it recomputes its window's winner and takes the window's gradient if that is itself
__global__ __launch_bounds__(256) void maxpool2_bwd_k(const float *__restrict__ in, const float *__restrict__ dout,
                                                      size_t n_in, int H, int W, float *__restrict__ din)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_in) return;
    const int Ho = H / 2, Wo = W / 2;
    const size_t n = i / ((size_t)H * W);
    const int rem = (int)(i - n * H * W), h = rem / W, w = rem - h * W;
    const int ho = h / 2, wo = w / 2;
    float g = 0.f;
    if (ho < Ho && wo < Wo) {                                       // not in a trailing odd row or column
        float m;
        const int win = pool_winner(in + (n * H + 2 * ho) * W + 2 * wo, W, &m);
        if (win == (h - 2 * ho) * 2 + (w - 2 * wo)) g = dout[(n * Ho + ho) * Wo + wo];
    }
    din[i] = g;
}

// The input of conv block 0 for a batch: out[b][c][y][x] = frames[t0 + f + c][ty*512 + y][tx*512 + x] with item index[b] =
// f*n_tiles + k and (ty, tx) tile k's, +0.0 beyond H or W and for an item outside [0, n_items). One thread per V output
// floats: V = 4 where W is a multiple of 4 (a tile's columns start at a multiple of 512, so a float4 lies wholly inside or
// wholly outside a row and is aligned), else 1.
constexpr int kStackC = AXT_IN_CH, kStackT = AXT_TILE;
template <int V>
__global__ __launch_bounds__(256) void tile_stacks_k(const float *__restrict__ frames, int H, int W, int t0, int n_items,
                                                     int n_tiles, TileList tl, const int *__restrict__ index, int B,
                                                     float *__restrict__ out)
{
    constexpr int per_row = kStackT / V, per_item = kStackC * kStackT * per_row;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * per_item) return;
    const int b = (int)(i / per_item), rem = (int)(i - (size_t)b * per_item);
    const int c = rem / (kStackT * per_row), y = rem / per_row % kStackT, x = rem % per_row * V;
    const int item = index[b];
    float v[V] = {};
    if (item >= 0 && item < n_items) {
        const int f = item / n_tiles, k = item - f * n_tiles;
        const int yy = tl.yx[2 * k] * kStackT + y, xx = tl.yx[2 * k + 1] * kStackT + x;
        if (yy < H && xx < W) {
            const float *src = frames + ((size_t)(t0 + f + c) * H + yy) * W + xx;
            if constexpr (V == 4) {
                const float4 s = *reinterpret_cast<const float4 *>(src);
                v[0] = s.x; v[1] = s.y; v[2] = s.z; v[3] = s.w;
            } else {
                v[0] = *src;
            }
        }
    }
    float *dst = out + i * V;
    if constexpr (V == 4) *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[0] = v[0];
}

// ---- batch statistics (train-mode BatchNorm) ----
struct BnUpdate { float one_minus_m, m, unbias; };             // formed in f64 on the host and rounded once

// grid (Co). z, F: [B][Co][H*W]. stats [3][Co]: the batch's mean, biased variance and 1 / sqrt(var + eps). Moves
// running_mean and running_var, and run_inv = 1 / sqrt(running_var + eps) for the eval-mode kernels with them.
__global__ __launch_bounds__(256) void bn_batch_fwd_k(const float *__restrict__ z, int B, Geom g,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      float *__restrict__ run_mean, float *__restrict__ run_var,
                                                      float *__restrict__ run_inv, float *__restrict__ stats, BnUpdate u,
                                                      float *__restrict__ F)
{
    __shared__ float red[1][256];
    const int tid = threadIdx.x, co = blockIdx.x, n = B * g.HW;
    float s = 0.f;
    for (int r = tid; r < n; r += 256) s += z[chan_off(r, g.Co, g.HW, co)];
    const float mu = __fdiv_rn(sum256(s, red, tid), (float)n);
    s = 0.f;
    for (int r = tid; r < n; r += 256) {
        const float d = __fsub_rn(z[chan_off(r, g.Co, g.HW, co)], mu);
        s = fmaf(d, d, s);
    }
    const float var = __fdiv_rn(sum256(s, red, tid), (float)n);
    const float inv = __fdiv_rn(1.f, __fsqrt_rn(__fadd_rn(var, (float)kBnEps)));
    if (tid == 0) {
        stats[co] = mu;
        stats[g.Co + co] = var;
        stats[2 * g.Co + co] = inv;
        run_mean[co] = __fadd_rn(__fmul_rn(u.one_minus_m, run_mean[co]), __fmul_rn(u.m, mu));
        const float rv = __fadd_rn(__fmul_rn(u.one_minus_m, run_var[co]), __fmul_rn(u.m, __fmul_rn(var, u.unbias)));
        run_var[co] = rv;
        run_inv[co] = (float)(1.0 / sqrt((double)rv + kBnEps));
    }
    const float ga = gamma[co], be = beta[co];
    for (int r = tid; r < n; r += 256) {
        const size_t o = chan_off(r, g.Co, g.HW, co);
        float zh;
        F[o] = leaky(bn_y(z[o], mu, inv, ga, be, &zh));
    }
}

// grid (Co). dF, z, dz: [B][Co][H*W]; stats as bn_batch_fwd_k wrote it. kAdam: updates bias, gamma, beta and their moments
// (p, m, v: [3][Co] in that order) as conv_bn_back_k does, bias with the gradient 0.
template <bool kAdam>
__global__ __launch_bounds__(256) void bn_batch_back_k(const float *__restrict__ dF, const float *__restrict__ z, int B, Geom g,
                                                       float *__restrict__ bias, float *__restrict__ gamma,
                                                       float *__restrict__ beta, const float *__restrict__ stats,
                                                       float *__restrict__ mom_m, float *__restrict__ mom_v,
                                                       float *__restrict__ dz, AdamArgs a)
{
    __shared__ float red[1][256];
    const int tid = threadIdx.x, co = blockIdx.x, n = B * g.HW;
    const float ga = gamma[co], be = beta[co], mu = stats[co], is = stats[2 * g.Co + co];
    const float fold = ga * is;
    float s_gamma = 0.f, s_beta = 0.f;
    for (int r = tid; r < n; r += 256) {
        const size_t o = chan_off(r, g.Co, g.HW, co);
        float zh;
        const float dy = leaky_back(z[o], dF[o], mu, is, ga, be, &zh);
        s_gamma = fmaf(dy, zh, s_gamma);
        s_beta += dy;
    }
    const float dgamma = sum256(s_gamma, red, tid), dbeta = sum256(s_beta, red, tid);
    const float mg = __fdiv_rn(dgamma, (float)n), mb = __fdiv_rn(dbeta, (float)n);
    for (int r = tid; r < n; r += 256) {
        const size_t o = chan_off(r, g.Co, g.HW, co);
        float zh;
        const float dy = leaky_back(z[o], dF[o], mu, is, ga, be, &zh);
        dz[o] = fold * ((dy - mb) - zh * mg);
    }
    if (kAdam) adam_bias_gamma_beta(tid, co, g.Co, {0.f, dgamma, dbeta}, bias, gamma, beta, mom_m, mom_v, a);
}

// split of the reduction over r = B*H*W for the weight gradient: about 1024 workgroups, runs a multiple of the tile depth
// A map beyond 64 x 64 (axt_conv_trainer_create_strided alone makes one) has so many r that 64 runs would leave a
// few workgroups with very long chains of tiles: there the runs may number up to H*W / 64, at most 1024, while the slabs
// stay within 16 M floats. Every shape axt_conv_trainer_create accepts keeps the split it had.
int wgrad_max_split(const Geom &g)
{
    const int base = std::max(1, std::min(64, 1024 / (axt_cdiv(g.K9, TN) * axt_cdiv(g.Co, TM))));
    if (g.H <= kMaxHW && g.W <= kMaxHW) return base;
    const int by_slab = (int)(((int64_t)1 << 24) / ((int64_t)g.Co * g.K9));
    return std::max(base, std::min(std::min(1024, g.HW / 64), by_slab));
}

void plan_wgrad(const Geom &g, int B, int *S, int *rchunk)
{
    const int R = B * g.HW;
    const int chunk = axt_cdiv(axt_cdiv(R, wgrad_max_split(g)), TK) * TK;
    *rchunk = chunk;
    *S = axt_cdiv(R, chunk);
}

}  // namespace

struct axt_conv_trainer {
    Geom g = {};
    int max_batch = 0;
    long step = 0;
    float *w = nullptr, *mw = nullptr, *vw = nullptr;       // conv.weight [Co][Ci][3][3] and its moments
    float *p3 = nullptr, *m3 = nullptr, *v3 = nullptr;      // [3][Co]: conv.bias, batchnorm.weight, batchnorm.bias
    float *mean = nullptr, *inv_sigma = nullptr;            // running_mean, 1 / sqrt(running_var + 1e-5)
    float *z = nullptr, *dz = nullptr, *slab = nullptr;     // stash of the last forward batch; scratch
    int last_B = 0;
    size_t bytes = 0;
    std::vector<void *> allocs;
    // batch statistics (axt_conv_trainer_set_batch_stats): the device buffers exist from the first switch on
    bool batch_stats = false, last_batch_stats = false;
    double momentum = 0.1;
    int64_t forwards = 0;                                   // forwards in batch mode: what num_batches_tracked grows by
    std::vector<float> var0;                                // running_var as created, until run_var takes over
    float *run_var = nullptr, *bstats = nullptr;            // [Co]; [3][Co]: the last batch's mean, biased variance, inv
    float *var_dev = nullptr;                               // var0 on the device for axt_conv_trainer_export while run_var is not there
};

namespace {

int ct_alloc(axt_conv_trainer *t, float **p, size_t floats, bool zero)
{
    const size_t bytes = floats * sizeof(float);
    if (hipMalloc((void **)p, bytes) != hipSuccess) {
        axt_set_error("axt_conv_trainer: hipMalloc of %zu bytes failed", bytes);
        return AXT_ENOMEM;
    }
    t->allocs.push_back(*p);
    t->bytes += bytes;
    if (zero) AXT_CHECK_HIP(hipMemset(*p, 0, bytes));
    return AXT_OK;
}

// what _step and _input_grad ask of their batch: in range, and the one the last forward stashed
int ct_check_stashed(const axt_conv_trainer *t, int B, const char *fn)
{
    AXT_REQUIRE(B >= 1 && B <= t->max_batch, "%s: batch %d not in [1,%d]", fn, B, t->max_batch);
    AXT_REQUIRE(B == t->last_B, "%s: the stashed activations are of a batch of %d, not %d: call axt_conv_trainer_forward on "
                "this batch first", fn, t->last_B, B);
    return AXT_OK;
}

// kAdam: the step's form. Without: dz only; the parameters and the moments are left alone.
template <bool kAdam>
void launch_bn_batch_back(axt_conv_trainer *t, const float *d_dfeat, int B, const AdamArgs &a, hipStream_t st)
{
    const Geom &g = t->g;
    hipLaunchKernelGGL(bn_batch_back_k<kAdam>, dim3(g.Co), dim3(256), 0, st, d_dfeat, t->z, B, g, t->p3, t->p3 + g.Co,
                       t->p3 + 2 * g.Co, t->bstats, t->m3, t->v3, t->dz, a);
}

// what both max-pool entry points ask of their sizes
int pool_check(int64_t n_maps, int H, int W, const char *fn)
{
    AXT_REQUIRE(H >= 2 && H <= kMaxPoolHW && W >= 2 && W <= kMaxPoolHW, "%s: map %d x %d not in [2,%d]", fn, H, W, kMaxPoolHW);
    AXT_REQUIRE(n_maps >= 0 && n_maps <= kMaxPoolElems / ((int64_t)H * W), "%s: %lld maps of %d x %d exceed %lld elements", fn,
                (long long)n_maps, H, W, (long long)kMaxPoolElems);
    return AXT_OK;
}

}  // namespace

extern "C" {

void axt_conv_trainer_destroy(axt_conv_trainer *t)
{
    if (!t) return;
    for (void *p : t->allocs) (void)hipFree(p);
    delete t;
}

// what both create entry points do once their arguments are checked. Hi, Wi: the input map.
static int ct_create(const char *fn, int Ci, int Co, int Hi, int Wi, int stride, const float *h_weight, const float *h_bias,
                     const float *h_gamma, const float *h_beta, const float *h_mean, const float *h_var, int max_batch,
                     axt_conv_trainer **out)
{
    axt_conv_trainer *t = new (std::nothrow) axt_conv_trainer;
    if (!t) {
        axt_set_error("%s: out of host memory", fn);
        return AXT_ENOMEM;
    }
    const int H = (Hi - 1) / stride + 1, W = (Wi - 1) / stride + 1;
    t->g = Geom{Ci, Co, H, W, H * W, Ci * 9, Hi, Wi, Hi * Wi, stride};
    t->max_batch = max_batch;
    t->var0.assign(h_var, h_var + Co);
    const size_t nw = (size_t)Co * Ci * 9, nz = (size_t)max_batch * Co * H * W;
    std::vector<float> p3((size_t)3 * Co), is(Co);
    for (int c = 0; c < Co; ++c) {
        p3[c] = h_bias[c];
        p3[Co + c] = h_gamma[c];
        p3[2 * Co + c] = h_beta[c];
        is[c] = (float)(1.0 / std::sqrt((double)h_var[c] + kBnEps));
    }
    int rc;
    auto fail = [&](int code) { axt_conv_trainer_destroy(t); return code; };
    if ((rc = ct_alloc(t, &t->w, nw, false)) || (rc = ct_alloc(t, &t->mw, nw, true)) || (rc = ct_alloc(t, &t->vw, nw, true)) ||
        (rc = ct_alloc(t, &t->p3, p3.size(), false)) || (rc = ct_alloc(t, &t->m3, p3.size(), true)) ||
        (rc = ct_alloc(t, &t->v3, p3.size(), true)) || (rc = ct_alloc(t, &t->mean, Co, false)) ||
        (rc = ct_alloc(t, &t->inv_sigma, Co, false)) || (rc = ct_alloc(t, &t->z, nz, true)) ||
        (rc = ct_alloc(t, &t->dz, nz, true)) || (rc = ct_alloc(t, &t->slab, (size_t)wgrad_max_split(t->g) * nw, false)))
        return fail(rc);
    if (hipMemcpy(t->w, h_weight, nw * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t->p3, p3.data(), p3.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t->mean, h_mean, Co * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t->inv_sigma, is.data(), Co * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        axt_set_error("%s: weight upload failed", fn);
        return fail(AXT_EHIP);
    }
    *out = t;
    return AXT_OK;
}

int axt_conv_trainer_create(int Ci, int Co, int H, int W, const float *h_weight, const float *h_bias, const float *h_gamma,
                            const float *h_beta, const float *h_mean, const float *h_var, int max_batch,
                            axt_conv_trainer **out)
{
    AXT_REQUIRE(out && h_weight && h_bias && h_gamma && h_beta && h_mean && h_var, "null argument");
    AXT_REQUIRE(Ci >= 1 && Ci <= kMaxC && Co >= 1 && Co <= kMaxC, "axt_conv_trainer_create: channels %d -> %d not in [1,%d]",
                Ci, Co, kMaxC);
    AXT_REQUIRE(H >= 1 && H <= kMaxHW && W >= 1 && W <= kMaxHW, "axt_conv_trainer_create: map %d x %d not in [1,%d]", H, W,
                kMaxHW);
    AXT_REQUIRE(max_batch >= 1 && max_batch <= kMaxB, "axt_conv_trainer_create: max_batch %d not in [1,%d]", max_batch, kMaxB);
    return ct_create("axt_conv_trainer_create", Ci, Co, H, W, 1, h_weight, h_bias, h_gamma, h_beta, h_mean, h_var, max_batch,
                     out);
}

int axt_conv_trainer_create_strided(int Ci, int Co, int Hin, int Win, int stride, const float *h_weight, const float *h_bias,
                                    const float *h_gamma, const float *h_beta, const float *h_mean, const float *h_var,
                                    int max_batch, axt_conv_trainer **out)
{
    static const char fn[] = "axt_conv_trainer_create_strided";
    AXT_REQUIRE(out && h_weight && h_bias && h_gamma && h_beta && h_mean && h_var, "%s: null argument", fn);
    AXT_REQUIRE(stride == 1 || stride == 2, "%s: stride %d is neither 1 nor 2", fn, stride);
    AXT_REQUIRE(Ci >= 1 && Ci <= kMaxC && Co >= 1 && Co <= kMaxC, "%s: channels %d -> %d not in [1,%d]", fn, Ci, Co, kMaxC);
    AXT_REQUIRE(Hin >= 1 && Hin <= kMaxInHW && Win >= 1 && Win <= kMaxInHW, "%s: input map %d x %d not in [1,%d]", fn, Hin, Win,
                kMaxInHW);
    const int H = (Hin - 1) / stride + 1, W = (Win - 1) / stride + 1, lim = stride == 2 ? kMaxOutS2 : kMaxOutS1;
    AXT_REQUIRE(H <= lim && W <= lim, "%s: output map %d x %d of stride %d exceeds %d", fn, H, W, stride, lim);
    AXT_REQUIRE(max_batch >= 1 && max_batch <= kMaxB, "%s: max_batch %d not in [1,%d]", fn, max_batch, kMaxB);
    return ct_create(fn, Ci, Co, Hin, Win, stride, h_weight, h_bias, h_gamma, h_beta, h_mean, h_var, max_batch, out);
}

size_t axt_conv_trainer_device_bytes(const axt_conv_trainer *t) { return t ? t->bytes : 0; }

int axt_conv_trainer_read_weights(const axt_conv_trainer *t, float *h_weight, float *h_bias, float *h_gamma, float *h_beta)
{
    AXT_REQUIRE(t && h_weight && h_bias && h_gamma && h_beta, "null argument");
    const size_t nc = (size_t)t->g.Co * sizeof(float);
    AXT_CHECK_HIP(hipDeviceSynchronize());
    AXT_CHECK_HIP(hipMemcpy(h_weight, t->w, (size_t)t->g.Co * t->g.K9 * sizeof(float), hipMemcpyDeviceToHost));
    AXT_CHECK_HIP(hipMemcpy(h_bias, t->p3, nc, hipMemcpyDeviceToHost));
    AXT_CHECK_HIP(hipMemcpy(h_gamma, t->p3 + t->g.Co, nc, hipMemcpyDeviceToHost));
    AXT_CHECK_HIP(hipMemcpy(h_beta, t->p3 + 2 * t->g.Co, nc, hipMemcpyDeviceToHost));
    return AXT_OK;
}

int axt_conv_trainer_read_moments(const axt_conv_trainer *t, int tensor, float *h_m, float *h_v, int64_t *step)
{
    AXT_REQUIRE(t && tensor >= 0 && tensor < 4, "axt_conv_trainer_read_moments: bad handle or tensor");
    const size_t n = (tensor == 0 ? (size_t)t->g.Co * t->g.K9 : (size_t)t->g.Co) * sizeof(float);
    const float *m = tensor == 0 ? t->mw : t->m3 + (size_t)(tensor - 1) * t->g.Co;
    const float *v = tensor == 0 ? t->vw : t->v3 + (size_t)(tensor - 1) * t->g.Co;
    AXT_CHECK_HIP(hipDeviceSynchronize());
    if (h_m) AXT_CHECK_HIP(hipMemcpy(h_m, m, n, hipMemcpyDeviceToHost));
    if (h_v) AXT_CHECK_HIP(hipMemcpy(h_v, v, n, hipMemcpyDeviceToHost));
    if (step) *step = t->step;
    return AXT_OK;
}

int axt_conv_trainer_forward(axt_conv_trainer *t, const float *d_in, const int32_t *d_index, int B, float *d_feat,
                             void *stream)
{
    AXT_REQUIRE(t && d_in && d_feat, "null argument");
    AXT_REQUIRE(B >= 1 && B <= t->max_batch, "axt_conv_trainer_forward: batch %d not in [1,%d]", B, t->max_batch);
    const Geom &g = t->g;
    const int n = B * g.HW;
    AXT_REQUIRE(!t->batch_stats || n >= 2, "axt_conv_trainer_forward: batch statistics need more than %d value per channel "
                "(B * H * W >= 2)", n);
    const dim3 grid(axt_cdiv(B * g.HW, TN), axt_cdiv(g.Co, TM));
    hipLaunchKernelGGL(g.stride == 2 ? conv_fwd_k<2> : conv_fwd_k<1>, grid, dim3(256), 0, (hipStream_t)stream, d_in, d_index, B,
                       g, t->w, t->p3, t->p3 + g.Co, t->p3 + 2 * g.Co, t->mean, t->inv_sigma, t->z, d_feat);
    AXT_LAUNCH_CHECK();
    if (t->batch_stats) {
        const double m = t->momentum;
        const BnUpdate u = {(float)(1.0 - m), (float)m, (float)((double)n / (n - 1))};
        hipLaunchKernelGGL(bn_batch_fwd_k, dim3(g.Co), dim3(256), 0, (hipStream_t)stream, t->z, B, g, t->p3 + g.Co,
                           t->p3 + 2 * g.Co, t->mean, t->run_var, t->inv_sigma, t->bstats, u, d_feat);
        AXT_LAUNCH_CHECK();
        t->forwards += 1;
    }
    t->last_B = B;
    t->last_batch_stats = t->batch_stats;
    return AXT_OK;
}

int axt_conv_trainer_step(axt_conv_trainer *t, const float *d_in, const int32_t *d_index, int B, const float *d_dfeat,
                          double lr, double beta1, double beta2, double eps, double weight_decay, void *stream)
{
    AXT_REQUIRE(t && d_in && d_dfeat, "null argument");
    if (int rc = ct_check_stashed(t, B, "axt_conv_trainer_step")) return rc;
    AXT_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0 && weight_decay >= 0,
                "axt_conv_trainer_step: bad Adam parameters");
    hipStream_t st = (hipStream_t)stream;
    const Geom &g = t->g;
    t->step += 1;
    const AdamArgs a = adam_args(lr, beta1, beta2, eps, weight_decay, t->step);
    // dz from gamma as it stands: each workgroup reads its channel's gamma before it updates it
    if (t->last_batch_stats)
        launch_bn_batch_back<true>(t, d_dfeat, B, a, st);
    else
        hipLaunchKernelGGL(conv_bn_back_k, dim3(g.Co), dim3(256), 0, st, d_dfeat, t->z, B, g, t->p3, t->p3 + g.Co,
                           t->p3 + 2 * g.Co, t->mean, t->inv_sigma, t->m3, t->v3, t->dz, a);
    AXT_LAUNCH_CHECK();
    int S, rchunk;
    plan_wgrad(g, B, &S, &rchunk);
    hipLaunchKernelGGL(g.stride == 2 ? conv_wgrad_k<2> : conv_wgrad_k<1>, dim3(axt_cdiv(g.K9, TN), axt_cdiv(g.Co, TM), S),
                       dim3(256), 0, st, d_in, d_index, B, g, t->dz, rchunk, t->slab);
    AXT_LAUNCH_CHECK();
    const int nw = g.Co * g.K9;
    hipLaunchKernelGGL(conv_adam_w_k, dim3(axt_cdiv(nw, 256)), dim3(256), 0, st, t->w, t->mw, t->vw, nw, t->slab, S, a);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

// dz is formed while staging and the sums stay in registers: nothing of the handle is written, and nothing is allocated
int axt_conv_trainer_input_grad(axt_conv_trainer *t, const float *d_dfeat, int B, float *d_dx, void *stream)
{
    AXT_REQUIRE(t && d_dfeat && d_dx, "null argument");
    if (int rc = ct_check_stashed(t, B, "axt_conv_trainer_input_grad")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geom &g = t->g;
    const dim3 grid(axt_cdiv(B * g.HWi, TN), axt_cdiv(g.Ci, TM));
    const bool s2 = g.stride == 2;
    if (t->last_batch_stats) {
        // batch form: dz goes through the handle's dz buffer, which _step writes again with the same values from the same
        // inputs
        launch_bn_batch_back<false>(t, d_dfeat, B, AdamArgs{}, st);
        AXT_LAUNCH_CHECK();
        const auto kernel = s2 ? conv_dgrad_k<DzStored, 2> : conv_dgrad_k<DzStored, 1>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, DzStored{t->dz}, B, g, t->w, d_dx);
    } else {
        const DzFromDF dz = {d_dfeat, t->z, t->p3 + g.Co, t->p3 + 2 * g.Co, t->mean, t->inv_sigma};
        const auto kernel = s2 ? conv_dgrad_k<DzFromDF, 2> : conv_dgrad_k<DzFromDF, 1>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, dz, B, g, t->w, d_dx);
    }
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_conv_trainer_set_batch_stats(axt_conv_trainer *t, int on, double momentum)
{
    AXT_REQUIRE(t, "null argument");
    AXT_REQUIRE(momentum > 0 && momentum <= 1, "axt_conv_trainer_set_batch_stats: momentum %g not in (0,1]", momentum);
    if (on && !t->run_var) {
        const size_t Co = t->g.Co;
        float *rv = nullptr, *bs = nullptr;
        int rc;
        if ((rc = ct_alloc(t, &rv, Co, false)) || (rc = ct_alloc(t, &bs, 3 * Co, true))) return rc;
        AXT_CHECK_HIP(hipMemcpy(rv, t->var0.data(), Co * sizeof(float), hipMemcpyHostToDevice));
        t->run_var = rv;
        t->bstats = bs;
    }
    t->batch_stats = on != 0;
    t->momentum = momentum;
    return AXT_OK;
}

int axt_conv_trainer_read_stats(const axt_conv_trainer *t, float *h_running_mean, float *h_running_var,
                                int64_t *num_batches_tracked, float *h_batch_mean, float *h_batch_var)
{
    AXT_REQUIRE(t, "null argument");
    AXT_REQUIRE(t->forwards > 0 || (!h_batch_mean && !h_batch_var), "axt_conv_trainer_read_stats: no forward has run with "
                "batch statistics yet");
    const size_t nc = (size_t)t->g.Co * sizeof(float);
    AXT_CHECK_HIP(hipDeviceSynchronize());
    if (h_running_mean) AXT_CHECK_HIP(hipMemcpy(h_running_mean, t->mean, nc, hipMemcpyDeviceToHost));
    if (h_running_var) {
        if (t->run_var) AXT_CHECK_HIP(hipMemcpy(h_running_var, t->run_var, nc, hipMemcpyDeviceToHost));
        else std::copy(t->var0.begin(), t->var0.end(), h_running_var);
    }
    if (num_batches_tracked) *num_batches_tracked = t->forwards;
    if (h_batch_mean) AXT_CHECK_HIP(hipMemcpy(h_batch_mean, t->bstats, nc, hipMemcpyDeviceToHost));
    if (h_batch_var) AXT_CHECK_HIP(hipMemcpy(h_batch_var, t->bstats + t->g.Co, nc, hipMemcpyDeviceToHost));
    return AXT_OK;
}

int axt_maxpool2_forward(const float *d_in, int64_t n_maps, int H, int W, float *d_out, void *stream)
{
    AXT_REQUIRE(d_in && d_out, "null argument");
    if (int rc = pool_check(n_maps, H, W, "axt_maxpool2_forward")) return rc;
    if (n_maps == 0) return AXT_OK;
    const size_t n_out = (size_t)n_maps * (H / 2) * (W / 2);
    hipLaunchKernelGGL(maxpool2_fwd_k, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_in, n_out, H,
                       W, d_out);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_tile_stacks(const float *d_frames, int T_all, int H, int W, int t0, int n_frames, const int32_t *h_tile_yx,
                    int n_tiles, const int32_t *d_index, int B, float *d_out, void *stream)
{
    static const char fn[] = "axt_tile_stacks";
    AXT_REQUIRE(d_frames && h_tile_yx && d_index && d_out, "%s: null argument", fn);
    AXT_REQUIRE(H >= 1 && W >= 1 && H <= kMaxPoolHW && W <= kMaxPoolHW, "%s: frames of %d x %d not in [1,%d]", fn, H, W,
                kMaxPoolHW);
    AXT_REQUIRE(t0 >= 0 && n_frames >= 1 && n_frames <= (1 << 22) && (int64_t)t0 + n_frames + (kStackC - 1) <= T_all,
                "%s: frames [%d,%d) + context exceed T_all=%d", fn, t0, t0 + n_frames, T_all);
    AXT_REQUIRE(B >= 1 && B <= 1024, "%s: batch %d not in [1,1024]", fn, B);
    TileList tl;
    if (int rc = axt_tile_list(fn, h_tile_yx, n_tiles, axt_last_tile(H, kStackT), axt_last_tile(W, kStackT), &tl)) return rc;
    const bool vec = W % 4 == 0 && (uintptr_t)d_frames % 16 == 0 && (uintptr_t)d_out % 16 == 0;
    const size_t n = (size_t)B * kStackC * kStackT * kStackT / (vec ? 4 : 1);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(tile_stacks_k<4>, grid, dim3(256), 0, (hipStream_t)stream, d_frames, H, W, t0, n_frames * n_tiles,
                           n_tiles, tl, d_index, B, d_out);
    else
        hipLaunchKernelGGL(tile_stacks_k<1>, grid, dim3(256), 0, (hipStream_t)stream, d_frames, H, W, t0, n_frames * n_tiles,
                           n_tiles, tl, d_index, B, d_out);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_maxpool2_backward(const float *d_in, const float *d_dout, int64_t n_maps, int H, int W, float *d_din, void *stream)
{
    AXT_REQUIRE(d_in && d_dout && d_din, "null argument");
    if (int rc = pool_check(n_maps, H, W, "axt_maxpool2_backward")) return rc;
    if (n_maps == 0) return AXT_OK;
    const size_t n_in = (size_t)n_maps * H * W;
    hipLaunchKernelGGL(maxpool2_bwd_k, dim3((unsigned)((n_in + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_in, d_dout,
                       n_in, H, W, d_din);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_conv_trainer_export(axt_conv_trainer *t, axt_detector *det, int li, void *stream)
{
    static const char fn[] = "axt_conv_trainer_export";
    AXT_REQUIRE(t && det, "%s: null argument", fn);
    AXT_REQUIRE(li >= 0 && li < 8, "%s: conv block %d not in 0..7", fn, li);
    int cin, cout, stride;
    if (int rc = axt_detector_conv_spec(li, &cin, &cout, &stride)) return rc;
    const Geom &g = t->g;
    AXT_REQUIRE(g.Ci == cin && g.Co == cout && g.stride == stride, "%s: the trainer is %d -> %d channels at stride %d, conv "
                "block %d is %d -> %d at stride %d", fn, g.Ci, g.Co, g.stride, li, cin, cout, stride);
    if (!t->run_var && !t->var_dev) {
        float *v = nullptr;
        if (int rc = ct_alloc(t, &v, g.Co, false)) return rc;
        AXT_CHECK_HIP(hipMemcpy(v, t->var0.data(), (size_t)g.Co * sizeof(float), hipMemcpyHostToDevice));
        t->var_dev = v;
    }
    return axt_detector_load_conv_block(det, li, t->w, t->p3, t->p3 + g.Co, t->p3 + 2 * g.Co, t->mean,
                                        t->run_var ? t->run_var : t->var_dev, stream);
}

}  // extern "C"
