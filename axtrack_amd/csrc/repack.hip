// Device-side weight packing for gfx950 (MI355X): a block's tensors in state-dict layout, f32 in device memory, into every
// packed image the inference kernels of cnn.hip / cnn_front.hip read. What axt_detector_create does on the
// host with pack_conv, pack_wino, pack_bf16x3 and the linear transposes, without the device -> host -> device round trip.
//
//   fold_k          BatchNorm fold in f64, rounded once to f32 (pack_conv's formulas)
//   direct_s2_k     [ci*9+ky*3+kx][co%4][ngp]                      conv blocks 0, 1 (conv3x3_s2_k1, conv_s2_fused)
//   direct_s1_k     [group][chunk][krow][NPADW]                    conv blocks 2..7 (conv3x3_mfma)
//   wino_k          U = G g G^T in pack_wino's LDS order           conv blocks 2..7 (conv3x3_wino)
//   b3_k            hi | mid | lo bf16 in pack_bf16x3's LDS order  conv blocks 2..6 (conv3x3_bf16x3)
//   transpose_k     [out][in] -> [in][out_padded] through LDS      the three linear layers (gemm_mfma)
//
// Every kernel is a gather: one thread per element (or per 16 bytes) of the IMAGE, which computes where its value comes
// from. So the whole image is written on every call, padding lanes as zeros, and nothing depends on what the buffer held.
//
// Byte identity with the host packers is the contract (tests/test_repack_gpu.py): the same operations in the same order
// and the same formats, and no contraction -- hipcc fuses a*b+c into an FMA on the device by default, the host build
// does not -- so every kernel that multiplies and adds sits under `#pragma clang fp contract(off)`. f64 sqrt and division
// are correctly rounded on the device (OCML follows OpenCL's rules for double).
#include "repack.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void fold_k(const float *__restrict__ w, const float *__restrict__ b,
                                                   const float *__restrict__ gamma, const float *__restrict__ beta,
                                                   const float *__restrict__ mean, const float *__restrict__ var, int k9,
                                                   int cout, float *__restrict__ wfold, float *__restrict__ bias)
{
#pragma clang fp contract(off)
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= cout * k9) return;
    const int co = idx / k9;
    const double sc = (double)gamma[co] / sqrt((double)var[co] + 1e-5);
    wfold[idx] = (float)((double)w[idx] * sc);
    if (idx < cout) {
        const double sb = (double)gamma[idx] / sqrt((double)var[idx] + 1e-5);
        const double d = (double)b[idx] - (double)mean[idx];
        const double p = d * sb;
        bias[idx] = (float)(p + (double)beta[idx]);
    }
}

__global__ __launch_bounds__(kThreads) void direct_s2_k(const float *__restrict__ wfold, int k9, int cout, int ngp,
                                                        float *__restrict__ out, int n)
{
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n) return;
    const int g = idx % ngp, j = (idx / ngp) % 4, k = idx / (ngp * 4);
    const int co = 4 * g + j;
    out[idx] = co < cout ? wfold[co * k9 + k] : 0.f;
}

__global__ __launch_bounds__(kThreads) void direct_s1_k(const float *__restrict__ wfold, int cin, int cout, int cch, int nt,
                                                        int npadw, float *__restrict__ out, int n)
{
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n) return;
    const int krows = 9 * cch, nchunk = cin / cch;
    const int col = idx % npadw, r = idx / npadw;
    const int krow = r % krows, r2 = r / krows;
    const int chunk = r2 % nchunk, grp = r2 / nchunk;
    const int co = grp * nt * 16 + col;
    // krow = ((ky*3 + kx) * cch/4 + c/4) * 4 + c%4
    const int tap = krow / cch, c = krow % cch;
    const int ci = chunk * cch + c;
    out[idx] = (col < nt * 16 && co < cout) ? wfold[(co * cin + ci) * 9 + tap] : 0.f;
}

__global__ __launch_bounds__(kThreads) void wino_k(const float *__restrict__ wfold, int cin, int cout, float *__restrict__ out,
                                                   int n)
{
#pragma clang fp contract(off)
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n) return;
    // image order: [group of 80][chunk of 8][pos 16][channel block 5][lane = q*16 + p][k-step 2]
    const int nchunk = cin / 8;
    const int s = idx % 2, lane = (idx / 2) % 64, nb = (idx / 128) % 5, pos = (idx / 640) % 16, ch = idx / kRepackWinoChunk;
    const int q = lane / 16, p = lane % 16;
    const int ci = (ch % nchunk) * 8 + s * 4 + q, co = (ch / nchunk) * 80 + nb * 16 + p;
    const int i = pos / 4, j = pos % 4;
    const double Gm[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const float *g = wfold + ((size_t)co * cin + ci) * 9;
    double tmp[3];
    for (int b = 0; b < 3; ++b) tmp[b] = Gm[i][0] * g[0 * 3 + b] + Gm[i][1] * g[1 * 3 + b] + Gm[i][2] * g[2 * 3 + b];
    const double u = tmp[0] * Gm[j][0] + tmp[1] * Gm[j][1] + tmp[2] * Gm[j][2];
    out[idx] = (float)u;
}

// f32 -> bf16, round to nearest even, and back: pack_bf16x3's own integer steps
__device__ inline unsigned bf16_rne(float x)
{
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ inline float bf16_to_f32(unsigned h) { return __uint_as_float(h << 16); }

// one thread per 8 bf16 (16 bytes) of the image: [chunk][k-step 5][plane 3][q 4][n 80][8]
__global__ __launch_bounds__(kThreads) void b3_k(const float *__restrict__ wfold, int cin, uint4 *__restrict__ out, int n8)
{
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n8) return;
    const int nn = idx % 80, q = (idx / 80) % 4, plane = (idx / 320) % 3, s = (idx / 960) % 5, chunk = idx / 4800;
    const int j = 4 * s + q;
    unsigned h[8] = {};
    if (j < 18) {
        const int tap = j >> 1, half = j & 1;
        for (int i = 0; i < 8; ++i) {
            const int c = chunk * 16 + 8 * half + i;
            if (c >= cin) continue;
            const float v = wfold[((size_t)nn * cin + c) * 9 + tap];
            const unsigned hi = bf16_rne(v);
            const float r1 = v - bf16_to_f32(hi);
            const unsigned mid = bf16_rne(r1);
            const unsigned lo = bf16_rne(r1 - bf16_to_f32(mid));
            h[i] = plane == 0 ? hi : plane == 1 ? mid : lo;
        }
    }
    out[idx] = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
}

// [fout][fin] -> [fin][fpad] in 64 x 64 tiles through LDS: float4 loads along `in`, float4 stores along `out`, so both
// sides move whole 256-byte rows. blockIdx.x: tile along in, blockIdx.y: tile along out (covers fpad).
constexpr int TT = 64;
__global__ __launch_bounds__(kThreads) void transpose_k(const float *__restrict__ w, int fin, int fout, int fpad,
                                                        float *__restrict__ out)
{
    __shared__ float tile[TT][TT + 1];
    const int i0 = blockIdx.x * TT, o0 = blockIdx.y * TT;
    const int t = threadIdx.x;
    for (int e = t; e < TT * TT / 4; e += kThreads) {
        const int row = e / (TT / 4), c4 = (e % (TT / 4)) * 4;       // row: out, c4: in
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o0 + row < fout) v = *reinterpret_cast<const float4 *>(w + (size_t)(o0 + row) * fin + i0 + c4);
        tile[row][c4 + 0] = v.x;
        tile[row][c4 + 1] = v.y;
        tile[row][c4 + 2] = v.z;
        tile[row][c4 + 3] = v.w;
    }
    __syncthreads();
    for (int e = t; e < TT * TT / 4; e += kThreads) {
        const int row = e / (TT / 4), c4 = (e % (TT / 4)) * 4;       // row: in, c4: out
        const float4 v = make_float4(tile[c4 + 0][row], tile[c4 + 1][row], tile[c4 + 2][row], tile[c4 + 3][row]);
        *reinterpret_cast<float4 *>(out + (size_t)(i0 + row) * fpad + o0 + c4) = v;
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int axt_repack_fold(const float *w, const float *b, const float *gamma, const float *beta, const float *mean, const float *var,
                    int cin, int cout, float *wfold, float *bias, hipStream_t st)
{
    AXT_REQUIRE(w && b && gamma && beta && mean && var && wfold && bias, "axt_repack_fold: null argument");
    AXT_REQUIRE(cin >= 1 && cin <= 512 && cout >= 1 && cout <= 512, "axt_repack_fold: channels %d -> %d not in [1,512]", cin, cout);
    const int n = cout * cin * 9;
    hipLaunchKernelGGL(fold_k, dim3(axt_cdiv(n, kThreads)), dim3(kThreads), 0, st, w, b, gamma, beta, mean, var, cin * 9, cout,
                       wfold, bias);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_repack_direct_s2(const float *wfold, int cin, int cout, float *out, hipStream_t st)
{
    AXT_REQUIRE(wfold && out, "axt_repack_direct_s2: null argument");
    AXT_REQUIRE(cin >= 1 && cin <= 512 && cout >= 1 && cout <= 512, "axt_repack_direct_s2: channels %d -> %d not in [1,512]", cin,
                cout);
    const int ngp = (cout / 4 + 3) / 4 * 4;
    AXT_REQUIRE(cout % 4 == 0, "axt_repack_direct_s2: %d output channels are not a multiple of 4", cout);
    const int n = (int)axt_repack_s2_floats(cin, cout);
    hipLaunchKernelGGL(direct_s2_k, dim3(axt_cdiv(n, kThreads)), dim3(kThreads), 0, st, wfold, cin * 9, cout, ngp, out, n);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_repack_direct_s1(const float *wfold, int cin, int cout, int cch, int nt, int npadw, int ngroups, float *out,
                         hipStream_t st)
{
    AXT_REQUIRE(wfold && out, "axt_repack_direct_s1: null argument");
    AXT_REQUIRE(cin >= 1 && cin <= 512 && cout >= 1 && cout <= 512 && cch >= 4 && cch % 4 == 0 && cin % cch == 0 && nt >= 1 &&
                npadw >= nt * 16 && ngroups >= 1 && ngroups * nt * 16 >= cout,
                "axt_repack_direct_s1: %d -> %d channels do not fit chunks of %d and %d groups of %d", cin, cout, cch, ngroups,
                nt * 16);
    const int n = (int)axt_repack_s1_floats(cin, cch, npadw, ngroups);
    hipLaunchKernelGGL(direct_s1_k, dim3(axt_cdiv(n, kThreads)), dim3(kThreads), 0, st, wfold, cin, cout, cch, nt, npadw, out, n);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_repack_wino(const float *wfold, int cin, int cout, float *out, hipStream_t st)
{
    AXT_REQUIRE(wfold && out, "axt_repack_wino: null argument");
    AXT_REQUIRE(cin >= 8 && cin <= 512 && cin % 8 == 0 && cout >= 80 && cout <= 480 && cout % 80 == 0,
                "axt_repack_wino: %d -> %d channels are not multiples of 8 and 80", cin, cout);
    const int n = (int)axt_repack_wino_floats(cin, cout);
    hipLaunchKernelGGL(wino_k, dim3(axt_cdiv(n, kThreads)), dim3(kThreads), 0, st, wfold, cin, cout, out, n);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_repack_b3(const float *wfold, int cin, unsigned *out, hipStream_t st)
{
    AXT_REQUIRE(wfold && out && aligned16(out), "axt_repack_b3: null or unaligned argument");
    AXT_REQUIRE(cin >= 1 && cin <= 512, "axt_repack_b3: %d input channels not in [1,512]", cin);
    const int n8 = (int)(axt_repack_b3_bf16(cin) / 8);
    hipLaunchKernelGGL(b3_k, dim3(axt_cdiv(n8, kThreads)), dim3(kThreads), 0, st, wfold, cin, reinterpret_cast<uint4 *>(out), n8);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_repack_linear(const float *w, int fin, int fout, int fpad, float *out, hipStream_t st)
{
    AXT_REQUIRE(w && out && aligned16(w) && aligned16(out), "axt_repack_linear: null or unaligned argument");
    AXT_REQUIRE(fin >= TT && fin % TT == 0 && fpad >= TT && fpad % TT == 0 && fout >= 1 && fout <= fpad && fpad / TT <= 65535,
                "axt_repack_linear: [%d][%d] -> [%d][%d] is not in 64 x 64 tiles", fout, fin, fin, fpad);
    hipLaunchKernelGGL(transpose_k, dim3(fin / TT, fpad / TT), dim3(kThreads), 0, st, w, fin, fout, fpad, out);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
