// train.hip -- fine-tuning of the detector's linear head (fcs.1/3/5 of model.py:105-117) with the convolutional trunk
// frozen: YOLO targets from labels, head forward on cached trunk features, the YOLO_AXTrack loss with its gradient, and
// the backward pass fused with Adam (torch.optim.Adam with L2 weight decay, core_functionality.py:81). DESIGN.md 6.8e.
//
// Kernels
//   yolo_targets_k   one thread per (frame, kept tile, cell) scans the frame's labels: the last label of a cell wins
//   head_gemm        out_slab[s][b][j] = sum over the s-th run of r of In[row(b)][r] * W(j, r): plain f32 FMAs on
//                    LDS tiles, split over r so that a skinny product (B <= 64) fills the machine. WT: W is [J][R]
//                    (forward, state_dict layout), else [R][J] (backward: dA = dZ W).
//   head_reduce      sums the slabs in ascending s (+ bias, + Sigmoid | * a(1-a) for the backward pass)
//   head_sum_slabs   sums the slabs in ascending s and nothing else (the input gradient dZ1 W1)
//   yolo_loss_k      one workgroup: the five loss components in f64 through a fixed tree, and dY
//   adam_fused       per weight element: g = sum_b dZ[b,n] In[b,k] in ascending b (never stored), then the Adam update
//                    of w, m, v in place. The hot path: streams w, m, v once in and once out.
//   adam_bias        the same for a bias vector
// Determinism: no atomics; every sum has one fixed order that depends on the layer sizes and B only.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "axt_common.h"
#include "repack.h"

namespace {

constexpr int kMaxB = 64;

// ------------------------------------------------------------------------------------------------ targets
__global__ __launch_bounds__(256) void yolo_targets_k(const int *__restrict__ lx, const int *__restrict__ ly,
                                                      const int *__restrict__ lcount, int F, int cap, TileList tl,
                                                      float *__restrict__ out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)F * tl.n * AXT_CELLS;
    if (i >= total) return;
    const int cell = (int)(i % AXT_CELLS);
    const int tile = (int)(i / AXT_CELLS % tl.n);
    const int f = (int)(i / AXT_CELLS / tl.n);
    const int cx = cell / AXT_S, cy = cell % AXT_S;           // dim 2 is the x cell, dim 3 the y cell
    const int y0 = tl.yx[2 * tile] * AXT_TILE, x0 = tl.yx[2 * tile + 1] * AXT_TILE;
    int n = lcount[f];
    n = n < cap ? n : cap;
    int win = -1;
    float wx = 0.f, wy = 0.f;
    for (int l = 0; l < n; ++l) {
        const int x = lx[(long)f * cap + l], y = ly[(long)f * cap + l];
        if (x < x0 || x >= x0 + AXT_TILE || y < y0 || y >= y0 + AXT_TILE) continue;       // (negative = no label)
        const float vx = (float)AXT_S * ((float)(x - x0) / (float)AXT_TILE);
        const float vy = (float)AXT_S * ((float)(y - y0) / (float)AXT_TILE);
        const int bx = (int)vx, by = (int)vy;
        if (bx == cx && by == cy) {
            win = l;
            wx = vx - (float)bx;
            wy = vy - (float)by;
        }
    }
    const float4 v = win >= 0 ? make_float4(1.f, wx, wy, (float)win) : make_float4(0.f, 0.f, 0.f, 0.f);
    reinterpret_cast<float4 *>(out)[i] = v;
}

// ------------------------------------------------------------------------------------------------ skinny GEMM
constexpr int GJ = 64, GR = 32, GPAD = 68;      // output columns per workgroup, reduction depth per tile, LDS row pitch

// four consecutive floats of a row (zero beyond `len`); vec: the row start and len are multiples of 4
__device__ inline float4 load4(const float *__restrict__ row, int i, int len, bool vec)
{
    if (vec && i + 3 < len) return *reinterpret_cast<const float4 *>(row + i);
    float4 v;
    v.x = i < len ? row[i] : 0.f;
    v.y = i + 1 < len ? row[i + 1] : 0.f;
    v.z = i + 2 < len ? row[i + 2] : 0.f;
    v.w = i + 3 < len ? row[i + 3] : 0.f;
    return v;
}

__device__ inline void store4(float *__restrict__ row, int i, int len, bool vec, float4 v)
{
    if (vec && i + 3 < len) {
        *reinterpret_cast<float4 *>(row + i) = v;
        return;
    }
    if (i < len) row[i] = v.x;
    if (i + 1 < len) row[i + 1] = v.y;
    if (i + 2 < len) row[i + 2] = v.z;
    if (i + 3 < len) row[i + 3] = v.w;
}

// slab[s][b][j], b < B, j < J; In row of b: index ? In + index[b]*ldin : In + b*ldin. Workgroup (x: j tile, y: split).
// Thread (tb = tid / 16, tj = tid % 16) owns rows tb*RB .. +RB-1 and columns tj*4 .. +3 of the 16*RB x 64 tile.
template <int RB, bool WT>
__global__ __launch_bounds__(256) void head_gemm(const float *__restrict__ In, const int *__restrict__ index, int ldin,
                                                 const float *__restrict__ W, int J, int R, int rchunk, int B,
                                                 float *__restrict__ slab)
{
    constexpr int BT = 16 * RB;
    __shared__ __attribute__((aligned(16))) float Xs[GR][BT + 4];
    __shared__ __attribute__((aligned(16))) float Ws[GR][GPAD];
    const int tid = threadIdx.x, tb = tid / 16, tj = tid % 16;
    const int j0 = blockIdx.x * GJ;
    const int r_begin = blockIdx.y * rchunk, r_end = min(R, r_begin + rchunk);
    const bool vin = ldin % 4 == 0, vw = (WT ? R : J) % 4 == 0;
    float acc[RB][4] = {};
    for (int r0 = r_begin; r0 < r_end; r0 += GR) {
        // In tile [BT][GR] -> Xs[r][b]
        for (int i = tid; i < BT * (GR / 4); i += 256) {
            const int b = i / (GR / 4), r = r0 + (i % (GR / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b < B) {
                const float *row = In + (size_t)(index ? index[b] : b) * ldin;
                v = load4(row, r, r_end, vin);
            }
            const int rr = r - r0;
            Xs[rr][b] = v.x; Xs[rr + 1][b] = v.y; Xs[rr + 2][b] = v.z; Xs[rr + 3][b] = v.w;
        }
        if (WT) {       // W [J][R]: tile [GJ][GR] -> Ws[r][j]
            for (int i = tid; i < GJ * (GR / 4); i += 256) {
                const int j = i / (GR / 4), r = r0 + (i % (GR / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j0 + j < J) v = load4(W + (size_t)(j0 + j) * R, r, r_end, vw);
                const int rr = r - r0;
                Ws[rr][j] = v.x; Ws[rr + 1][j] = v.y; Ws[rr + 2][j] = v.z; Ws[rr + 3][j] = v.w;
            }
        } else {        // W [R][J]: tile [GR][GJ] -> Ws[r][j]
            for (int i = tid; i < GR * (GJ / 4); i += 256) {
                const int rr = i / (GJ / 4), j = (i % (GJ / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r0 + rr < r_end) v = load4(W + (size_t)(r0 + rr) * J, j0 + j, J, vw);
                *reinterpret_cast<float4 *>(&Ws[rr][j]) = v;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < GR; ++r) {
            const float4 w = *reinterpret_cast<const float4 *>(&Ws[r][tj * 4]);
            float x[RB];
#pragma unroll
            for (int q = 0; q < RB; ++q) x[q] = Xs[r][tb * RB + q];
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                acc[q][0] = fmaf(x[q], w.x, acc[q][0]);
                acc[q][1] = fmaf(x[q], w.y, acc[q][1]);
                acc[q][2] = fmaf(x[q], w.z, acc[q][2]);
                acc[q][3] = fmaf(x[q], w.w, acc[q][3]);
            }
        }
        __syncthreads();
    }
    float *dst = slab + (size_t)blockIdx.y * B * J;
#pragma unroll
    for (int q = 0; q < RB; ++q) {
        const int b = tb * RB + q;
        if (b >= B) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tj * 4 + c;
            if (j < J) dst[(size_t)b * J + j] = acc[q][c];
        }
    }
}

// out[b][j] = f(sum_s slab[s][b][j]); mode 0: + bias, 1: Sigmoid(+ bias), 2: * a (1 - a) with a = act[b][j]
__global__ __launch_bounds__(256) void head_reduce(const float *__restrict__ slab, int S, int B, int J,
                                                   const float *__restrict__ bias, const float *__restrict__ act,
                                                   int mode, float *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * J) return;
    float s = slab[i];
    for (int k = 1; k < S; ++k) s += slab[(size_t)k * B * J + i];
    if (mode == 2) {
        const float a = act[i];
        s = s * (a * (1.f - a));
    } else {
        s += bias[i % J];
        if (mode == 1) s = 1.f / (1.f + expf(-s));
    }
    out[i] = s;
}

// out[i] = sum_s slab[s][i] in ascending s, nothing else (axt_head_trainer_input_grad)
__global__ __launch_bounds__(256) void head_sum_slabs(const float *__restrict__ slab, int S, size_t n, float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = slab[i];
    for (int k = 1; k < S; ++k) s += slab[(size_t)k * n + i];
    out[i] = s;
}

// ------------------------------------------------------------------------------------------------ loss
// pred [B,144,3], target table [.,144,4] gathered by index. comp f64 [5]: no_object, object, xy, summed, pos rate.
__global__ __launch_bounds__(256) void yolo_loss_k(const float *__restrict__ pred, const float *__restrict__ target,
                                                   const int *__restrict__ index, int B, double l_obj, double l_noobj,
                                                   double l_coord, double *__restrict__ comp, float *__restrict__ dy)
{
    __shared__ double red[4][256];
    const int tid = threadIdx.x;
    double s_no = 0, s_obj = 0, s_xy = 0, s_pos = 0;
    const double inv_bs = 1.0 / (double)B;
    for (int i = tid; i < B * AXT_CELLS; i += 256) {
        const int b = i / AXT_CELLS, c = i % AXT_CELLS;
        const float4 t = reinterpret_cast<const float4 *>(target)[(size_t)(index ? index[b] : b) * AXT_CELLS + c];
        const double obj = t.x, p = pred[3 * i], px = pred[3 * i + 1], py = pred[3 * i + 2];
        const double e_no = p * (1.0 - obj), e_obj = p * obj - obj;
        const double ex = px * obj - (double)t.y, ey = py * obj - (double)t.z;
        s_no += e_no * e_no;
        s_obj += e_obj * e_obj;
        s_xy += ex * ex + ey * ey;
        s_pos += obj;
        if (dy) {
            // d/dp of (p obj - obj)^2 is 2 obj (p obj - obj); of (p (1-obj))^2 is 2 (1-obj)^2 p; obj is 0 or 1 in a target
            dy[3 * i] = (float)((2.0 * l_obj * obj * e_obj + 2.0 * l_noobj * (1.0 - obj) * e_no) * inv_bs);
            dy[3 * i + 1] = (float)(2.0 * l_coord * obj * ex * inv_bs);
            dy[3 * i + 2] = (float)(2.0 * l_coord * obj * ey * inv_bs);
        }
    }
    red[0][tid] = s_no; red[1][tid] = s_obj; red[2][tid] = s_xy; red[3][tid] = s_pos;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double no = l_noobj * red[0][0] * inv_bs, ob = l_obj * red[1][0] * inv_bs, xy = l_coord * red[2][0] * inv_bs;
        comp[0] = no;
        comp[1] = ob;
        comp[2] = xy;
        comp[3] = no + ob + xy;
        comp[4] = red[3][0] / ((double)B * AXT_CELLS);
    }
}

// ------------------------------------------------------------------------------------------------ backward + Adam
// every factor is formed in f64 on the host and rounded once (1.f - 0.999f is off by 5e-5 of itself)
struct AdamArgs { float beta1, beta2, one_minus_beta1, one_minus_beta2, step_size, bc2_sqrt, eps, weight_decay; };

__device__ inline void adam1(float g, float &w, float &m, float &v, const AdamArgs &a)
{
    g = fmaf(a.weight_decay, w, g);
    m = a.beta1 * m + a.one_minus_beta1 * g;
    v = a.beta2 * v + a.one_minus_beta2 * (g * g);
    w = w - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

constexpr int UN = 32, UK = 256;        // weight rows and columns per workgroup: a wave owns 8 rows x 256 columns

// W, M, V [N][K]; dZ [B][N]; In rows [.][K] (gathered by index if given). Dynamic LDS: B * (UK + UN) floats.
__global__ __launch_bounds__(256) void adam_fused(float *__restrict__ W, float *__restrict__ M, float *__restrict__ V,
                                                  int N, int K, const float *__restrict__ dZ,
                                                  const float *__restrict__ In, const int *__restrict__ index, int B,
                                                  AdamArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Xs = lds;                    // [B][UK]
    float *Ds = lds + (size_t)B * UK;   // [B][UN]
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int k0 = blockIdx.x * UK, n0 = blockIdx.y * UN;
    const bool vec = K % 4 == 0;
    for (int i = tid; i < B * (UK / 4); i += 256) {
        const int b = i / (UK / 4), k = (i % (UK / 4)) * 4;
        const float *row = In + (size_t)(index ? index[b] : b) * K;
        *reinterpret_cast<float4 *>(Xs + b * UK + k) = load4(row, k0 + k, K, vec);
    }
    for (int i = tid; i < B * UN; i += 256) {
        const int b = i / UN, n = i % UN;
        Ds[i] = n0 + n < N ? dZ[(size_t)b * N + n0 + n] : 0.f;
    }
    __syncthreads();
    const int k = k0 + lane * 4;
    if (k >= K) return;
    const int nb = n0 + wave * 8;
    float4 w[8], m[8], v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        if (nb + q < N) {
            const size_t off = (size_t)(nb + q) * K;
            w[q] = load4(W + off, k, K, vec);
            m[q] = load4(M + off, k, K, vec);
            v[q] = load4(V + off, k, K, vec);
        }
    }
    float4 g[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) g[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < B; ++b) {
        const float4 x = *reinterpret_cast<const float4 *>(Xs + b * UK + lane * 4);
        const float4 d0 = *reinterpret_cast<const float4 *>(Ds + b * UN + wave * 8);
        const float4 d1 = *reinterpret_cast<const float4 *>(Ds + b * UN + wave * 8 + 4);
        const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            g[q].x = fmaf(d[q], x.x, g[q].x);
            g[q].y = fmaf(d[q], x.y, g[q].y);
            g[q].z = fmaf(d[q], x.z, g[q].z);
            g[q].w = fmaf(d[q], x.w, g[q].w);
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        if (nb + q < N) {
            adam1(g[q].x, w[q].x, m[q].x, v[q].x, a);
            adam1(g[q].y, w[q].y, m[q].y, v[q].y, a);
            adam1(g[q].z, w[q].z, m[q].z, v[q].z, a);
            adam1(g[q].w, w[q].w, m[q].w, v[q].w, a);
            const size_t off = (size_t)(nb + q) * K;
            store4(W + off, k, K, vec, w[q]);
            store4(M + off, k, K, vec, m[q]);
            store4(V + off, k, K, vec, v[q]);
        }
    }
}

__global__ __launch_bounds__(256) void adam_bias(float *__restrict__ Wb, float *__restrict__ M, float *__restrict__ V,
                                                 int N, const float *__restrict__ dZ, int B, AdamArgs a)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float g = 0.f;
    for (int b = 0; b < B; ++b) g += dZ[(size_t)b * N + n];
    float w = Wb[n], m = M[n], v = V[n];
    adam1(g, w, m, v, a);
    Wb[n] = w; M[n] = m; V[n] = v;
}

// split of a reduction of length R for an output of J columns: about 1024 workgroups, runs a multiple of the tile depth
void plan_split(int J, int R, int *S, int *rchunk)
{
    const int jt = axt_cdiv(J, GJ);
    int s = std::max(1, std::min(64, 1024 / jt));
    int chunk = axt_cdiv(axt_cdiv(R, s), GR) * GR;
    *rchunk = chunk;
    *S = axt_cdiv(R, chunk);
}

}  // namespace

struct axt_head_trainer {
    int dims[4] = {};                   // K0, H1, H2, NOUT
    int max_batch = 0;
    long step = 0;
    float *w[3] = {}, *b[3] = {};       // master weights [out][in], biases
    float *mw[3] = {}, *vw[3] = {}, *mb[3] = {}, *vb[3] = {};
    float *a1 = nullptr, *a2 = nullptr;             // Sigmoid outputs of the last forward batch
    float *dz1 = nullptr, *dz2 = nullptr;
    float *slab = nullptr;
    float *ig_dz1 = nullptr, *ig_dz2 = nullptr, *ig_slab = nullptr;    // axt_head_trainer_input_grad's own scratch, allocated by its first call
    double *d_comp = nullptr;
    int last_B = 0;                     // batch of the stashes
    size_t bytes = 0;
    std::vector<void *> allocs;
};

namespace {

AxtOncePerDevice g_adam_once;

int tr_alloc(axt_head_trainer *t, void **p, size_t bytes, bool zero)
{
    if (hipMalloc(p, bytes) != hipSuccess) {
        axt_set_error("axt_head_trainer: hipMalloc of %zu bytes failed", bytes);
        return AXT_ENOMEM;
    }
    t->allocs.push_back(*p);
    t->bytes += bytes;
    if (zero) AXT_CHECK_HIP(hipMemset(*p, 0, bytes));
    return AXT_OK;
}

template <bool WT>
int launch_head_gemm(const float *In, const int *index, int ldin, const float *W, int J, int R, int B, float *slab,
                     int *S_out, hipStream_t st)
{
    int S, rchunk;
    plan_split(J, R, &S, &rchunk);
    *S_out = S;
    const dim3 grid(axt_cdiv(J, GJ), S);
    if (B <= 16)
        hipLaunchKernelGGL((head_gemm<1, WT>), grid, dim3(256), 0, st, In, index, ldin, W, J, R, rchunk, B, slab);
    else if (B <= 32)
        hipLaunchKernelGGL((head_gemm<2, WT>), grid, dim3(256), 0, st, In, index, ldin, W, J, R, rchunk, B, slab);
    else
        hipLaunchKernelGGL((head_gemm<4, WT>), grid, dim3(256), 0, st, In, index, ldin, W, J, R, rchunk, B, slab);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int launch_head_reduce(const float *slab, int S, int B, int J, const float *bias, const float *act, int mode, float *out,
                       hipStream_t st)
{
    hipLaunchKernelGGL(head_reduce, dim3(axt_cdiv(B * J, 256)), dim3(256), 0, st, slab, S, B, J, bias, act, mode, out);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int launch_adam(axt_head_trainer *t, int layer, const float *dZ, const float *In, const int *index, int B,
                const AdamArgs &a, hipStream_t st)
{
    const int K = t->dims[layer], N = t->dims[layer + 1];
    const int lds = B * (UK + UN) * (int)sizeof(float);
    hipLaunchKernelGGL(adam_fused, dim3(axt_cdiv(K, UK), axt_cdiv(N, UN)), dim3(256), lds, st, t->w[layer], t->mw[layer],
                       t->vw[layer], N, K, dZ, In, index, B, a);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(adam_bias, dim3(axt_cdiv(N, 256)), dim3(256), 0, st, t->b[layer], t->mb[layer], t->vb[layer], N, dZ,
                       B, a);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

}  // namespace

extern "C" {

int axt_yolo_targets(const int32_t *d_lx, const int32_t *d_ly, const int32_t *d_lcount, int F, int cap,
                     const int32_t *h_tile_yx, int n_tiles, float *d_target, void *stream)
{
    AXT_REQUIRE(d_lx && d_ly && d_lcount && h_tile_yx && d_target, "axt_yolo_targets: null argument");
    AXT_REQUIRE(F >= 0 && cap >= 1, "axt_yolo_targets: F=%d cap=%d", F, cap);
    TileList tl;
    if (int rc = axt_tile_list("axt_yolo_targets", h_tile_yx, n_tiles, 32766, 32766, &tl)) return rc;
    const long total = (long)F * n_tiles * AXT_CELLS;
    if (total == 0) return AXT_OK;
    AXT_REQUIRE(total < (1l << 31) * 256, "axt_yolo_targets: %d frames x %d tiles: too many cells (2^39 at most)", F, n_tiles);
    hipLaunchKernelGGL(yolo_targets_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_lx, d_ly,
                       d_lcount, F, cap, tl, d_target);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

void axt_head_trainer_destroy(axt_head_trainer *t)
{
    if (!t) return;
    for (void *p : t->allocs) (void)hipFree(p);
    delete t;
}

int axt_head_trainer_create(int K0, int H1, int H2, int NOUT, const float *h_w1, const float *h_b1, const float *h_w2,
                            const float *h_b2, const float *h_w3, const float *h_b3, int max_batch,
                            axt_head_trainer **out)
{
    AXT_REQUIRE(out && h_w1 && h_b1 && h_w2 && h_b2 && h_w3 && h_b3, "null argument");
    AXT_REQUIRE(K0 >= 1 && H1 >= 1 && H2 >= 1, "axt_head_trainer_create: bad sizes %d %d %d", K0, H1, H2);
    AXT_REQUIRE(NOUT == AXT_YOLO_FLOATS, "axt_head_trainer_create: NOUT must be %d, got %d", AXT_YOLO_FLOATS, NOUT);
    AXT_REQUIRE(max_batch >= 1 && max_batch <= kMaxB, "axt_head_trainer_create: max_batch %d not in [1,%d]", max_batch, kMaxB);
    axt_head_trainer *t = new (std::nothrow) axt_head_trainer;
    if (!t) {
        axt_set_error("axt_head_trainer_create: out of host memory");
        return AXT_ENOMEM;
    }
    t->dims[0] = K0; t->dims[1] = H1; t->dims[2] = H2; t->dims[3] = NOUT;
    t->max_batch = max_batch;
    const float *hw[3] = {h_w1, h_w2, h_w3}, *hb[3] = {h_b1, h_b2, h_b3};
    int rc = AXT_OK;
    auto fail = [&](int code) { axt_head_trainer_destroy(t); return code; };
    size_t slab_floats = 0;
    for (int l = 0; l < 3 && !rc; ++l) {
        const size_t nw = (size_t)t->dims[l] * t->dims[l + 1] * sizeof(float), nb = (size_t)t->dims[l + 1] * sizeof(float);
        if ((rc = tr_alloc(t, (void **)&t->w[l], nw, false))) break;
        if ((rc = tr_alloc(t, (void **)&t->mw[l], nw, true))) break;
        if ((rc = tr_alloc(t, (void **)&t->vw[l], nw, true))) break;
        if ((rc = tr_alloc(t, (void **)&t->b[l], nb, false))) break;
        if ((rc = tr_alloc(t, (void **)&t->mb[l], nb, true))) break;
        if ((rc = tr_alloc(t, (void **)&t->vb[l], nb, true))) break;
        if (hipMemcpy(t->w[l], hw[l], nw, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(t->b[l], hb[l], nb, hipMemcpyHostToDevice) != hipSuccess) {
            axt_set_error("axt_head_trainer_create: weight upload failed");
            rc = AXT_EHIP;
            break;
        }
        int S, chunk;
        plan_split(t->dims[l + 1], t->dims[l], &S, &chunk);                 // forward: J = out, R = in
        slab_floats = std::max(slab_floats, (size_t)S * max_batch * t->dims[l + 1]);
        if (l > 0) {
            plan_split(t->dims[l], t->dims[l + 1], &S, &chunk);             // backward: J = in, R = out
            slab_floats = std::max(slab_floats, (size_t)S * max_batch * t->dims[l]);
        }
    }
    if (rc) return fail(rc);
    if ((rc = tr_alloc(t, (void **)&t->a1, (size_t)max_batch * H1 * sizeof(float), true))) return fail(rc);
    if ((rc = tr_alloc(t, (void **)&t->a2, (size_t)max_batch * H2 * sizeof(float), true))) return fail(rc);
    if ((rc = tr_alloc(t, (void **)&t->dz1, (size_t)max_batch * H1 * sizeof(float), true))) return fail(rc);
    if ((rc = tr_alloc(t, (void **)&t->dz2, (size_t)max_batch * H2 * sizeof(float), true))) return fail(rc);
    if ((rc = tr_alloc(t, (void **)&t->slab, slab_floats * sizeof(float), false))) return fail(rc);
    if ((rc = tr_alloc(t, (void **)&t->d_comp, 5 * sizeof(double), true))) return fail(rc);
    if (hipDeviceSynchronize() != hipSuccess) {
        axt_set_error("axt_head_trainer_create: device synchronisation failed");
        return fail(AXT_EHIP);
    }
    *out = t;
    return AXT_OK;
}

size_t axt_head_trainer_device_bytes(const axt_head_trainer *t) { return t ? t->bytes : 0; }

int axt_head_trainer_read_weights(const axt_head_trainer *t, float *h_w1, float *h_b1, float *h_w2, float *h_b2,
                                  float *h_w3, float *h_b3)
{
    AXT_REQUIRE(t && h_w1 && h_b1 && h_w2 && h_b2 && h_w3 && h_b3, "null argument");
    float *hw[3] = {h_w1, h_w2, h_w3}, *hb[3] = {h_b1, h_b2, h_b3};
    AXT_CHECK_HIP(hipDeviceSynchronize());
    for (int l = 0; l < 3; ++l) {
        AXT_CHECK_HIP(hipMemcpy(hw[l], t->w[l], (size_t)t->dims[l] * t->dims[l + 1] * sizeof(float), hipMemcpyDeviceToHost));
        AXT_CHECK_HIP(hipMemcpy(hb[l], t->b[l], (size_t)t->dims[l + 1] * sizeof(float), hipMemcpyDeviceToHost));
    }
    return AXT_OK;
}

int axt_head_trainer_read_moments(const axt_head_trainer *t, int layer, float *h_mw, float *h_vw, float *h_mb, float *h_vb,
                                  int64_t *step)
{
    AXT_REQUIRE(t && layer >= 0 && layer < 3, "axt_head_trainer_read_moments: bad handle or layer");
    const size_t nw = (size_t)t->dims[layer] * t->dims[layer + 1] * sizeof(float), nb = (size_t)t->dims[layer + 1] * sizeof(float);
    AXT_CHECK_HIP(hipDeviceSynchronize());
    if (h_mw) AXT_CHECK_HIP(hipMemcpy(h_mw, t->mw[layer], nw, hipMemcpyDeviceToHost));
    if (h_vw) AXT_CHECK_HIP(hipMemcpy(h_vw, t->vw[layer], nw, hipMemcpyDeviceToHost));
    if (h_mb) AXT_CHECK_HIP(hipMemcpy(h_mb, t->mb[layer], nb, hipMemcpyDeviceToHost));
    if (h_vb) AXT_CHECK_HIP(hipMemcpy(h_vb, t->vb[layer], nb, hipMemcpyDeviceToHost));
    if (step) *step = t->step;
    return AXT_OK;
}

int axt_head_trainer_forward(axt_head_trainer *t, const float *d_feat, const int32_t *d_index, int B, float *d_yolo,
                             void *stream)
{
    AXT_REQUIRE(t && d_feat && d_yolo, "null argument");
    AXT_REQUIRE(B >= 1 && B <= t->max_batch, "axt_head_trainer_forward: batch %d not in [1,%d]", B, t->max_batch);
    hipStream_t st = (hipStream_t)stream;
    const int K0 = t->dims[0], H1 = t->dims[1], H2 = t->dims[2], NOUT = t->dims[3];
    int S, rc;
    if ((rc = launch_head_gemm<true>(d_feat, d_index, K0, t->w[0], H1, K0, B, t->slab, &S, st))) return rc;
    if ((rc = launch_head_reduce(t->slab, S, B, H1, t->b[0], nullptr, 1, t->a1, st))) return rc;
    if ((rc = launch_head_gemm<true>(t->a1, nullptr, H1, t->w[1], H2, H1, B, t->slab, &S, st))) return rc;
    if ((rc = launch_head_reduce(t->slab, S, B, H2, t->b[1], nullptr, 1, t->a2, st))) return rc;
    if ((rc = launch_head_gemm<true>(t->a2, nullptr, H2, t->w[2], NOUT, H2, B, t->slab, &S, st))) return rc;
    if ((rc = launch_head_reduce(t->slab, S, B, NOUT, t->b[2], nullptr, 0, d_yolo, st))) return rc;
    t->last_B = B;
    return AXT_OK;
}

int axt_head_trainer_loss(axt_head_trainer *t, const float *d_yolo, const float *d_target, const int32_t *d_index, int B,
                          double lambda_obj, double lambda_noobj, double lambda_coord, double *h_components, float *d_dy,
                          void *stream)
{
    AXT_REQUIRE(t && d_yolo && d_target, "null argument");
    AXT_REQUIRE(B >= 1 && B <= t->max_batch, "axt_head_trainer_loss: batch %d not in [1,%d]", B, t->max_batch);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(yolo_loss_k, dim3(1), dim3(256), 0, st, d_yolo, d_target, d_index, B, lambda_obj, lambda_noobj,
                       lambda_coord, t->d_comp, d_dy);
    AXT_LAUNCH_CHECK();
    if (h_components) {
        AXT_CHECK_HIP(hipMemcpyAsync(h_components, t->d_comp, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
        AXT_CHECK_HIP(hipStreamSynchronize(st));
    }
    return AXT_OK;
}

int axt_head_trainer_step(axt_head_trainer *t, const float *d_feat, const int32_t *d_index, int B, const float *d_dy,
                          double lr, double beta1, double beta2, double eps, double weight_decay, void *stream)
{
    AXT_REQUIRE(t && d_feat && d_dy, "null argument");
    AXT_REQUIRE(B >= 1 && B <= t->max_batch, "axt_head_trainer_step: batch %d not in [1,%d]", B, t->max_batch);
    AXT_REQUIRE(B == t->last_B, "axt_head_trainer_step: the stashed activations are of a batch of %d, not %d: call "
                "axt_head_trainer_forward on this batch first", t->last_B, B);
    AXT_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0 && weight_decay >= 0,
                "axt_head_trainer_step: bad Adam parameters");
    hipStream_t st = (hipStream_t)stream;
    const int lds_max = kMaxB * (UK + UN) * (int)sizeof(float);
    int rc;
    if ((rc = axt_max_dynamic_lds(adam_fused, lds_max, g_adam_once))) return rc;
    const int H1 = t->dims[1], H2 = t->dims[2], NOUT = t->dims[3];
    int S;
    // every dZ from the weights as they stand, before any of them moves
    if ((rc = launch_head_gemm<false>(d_dy, nullptr, NOUT, t->w[2], H2, NOUT, B, t->slab, &S, st))) return rc;
    if ((rc = launch_head_reduce(t->slab, S, B, H2, nullptr, t->a2, 2, t->dz2, st))) return rc;
    if ((rc = launch_head_gemm<false>(t->dz2, nullptr, H2, t->w[1], H1, H2, B, t->slab, &S, st))) return rc;
    if ((rc = launch_head_reduce(t->slab, S, B, H1, nullptr, t->a1, 2, t->dz1, st))) return rc;
    t->step += 1;
    const double bc1 = 1.0 - std::pow(beta1, (double)t->step), bc2 = 1.0 - std::pow(beta2, (double)t->step);
    AdamArgs a;
    a.beta1 = (float)beta1;
    a.beta2 = (float)beta2;
    a.one_minus_beta1 = (float)(1.0 - beta1);
    a.one_minus_beta2 = (float)(1.0 - beta2);
    a.step_size = (float)(lr / bc1);
    a.bc2_sqrt = (float)std::sqrt(bc2);
    a.eps = (float)eps;
    a.weight_decay = (float)weight_decay;
    if ((rc = launch_adam(t, 2, d_dy, t->a2, nullptr, B, a, st))) return rc;
    if ((rc = launch_adam(t, 1, t->dz2, t->a1, nullptr, B, a, st))) return rc;
    if ((rc = launch_adam(t, 0, t->dz1, d_feat, d_index, B, a, st))) return rc;
    return AXT_OK;
}

// dFeat = dZ1 W1 from the stashes of the last _forward and the weights as they stand, in scratch of its own (allocated by
// the first call): nothing that _forward, _loss or _step read or write is touched.
int axt_head_trainer_input_grad(axt_head_trainer *t, const float *d_dy, int B, float *d_dfeat, void *stream)
{
    AXT_REQUIRE(t && d_dy && d_dfeat, "null argument");
    AXT_REQUIRE(B >= 1 && B <= t->max_batch, "axt_head_trainer_input_grad: batch %d not in [1,%d]", B, t->max_batch);
    AXT_REQUIRE(B == t->last_B, "axt_head_trainer_input_grad: the stashed activations are of a batch of %d, not %d: call "
                "axt_head_trainer_forward on this batch first", t->last_B, B);
    hipStream_t st = (hipStream_t)stream;
    const int K0 = t->dims[0], H1 = t->dims[1], H2 = t->dims[2], NOUT = t->dims[3];
    int S, chunk, rc;
    if (!t->ig_slab) {
        size_t floats = 0;
        for (int l = 0; l < 3; ++l) {
            plan_split(t->dims[l], t->dims[l + 1], &S, &chunk);             // J = in, R = out
            floats = std::max(floats, (size_t)S * t->max_batch * t->dims[l]);
        }
        if ((rc = tr_alloc(t, (void **)&t->ig_dz1, (size_t)t->max_batch * H1 * sizeof(float), false))) return rc;
        if ((rc = tr_alloc(t, (void **)&t->ig_dz2, (size_t)t->max_batch * H2 * sizeof(float), false))) return rc;
        if ((rc = tr_alloc(t, (void **)&t->ig_slab, floats * sizeof(float), false))) return rc;
    }
    if ((rc = launch_head_gemm<false>(d_dy, nullptr, NOUT, t->w[2], H2, NOUT, B, t->ig_slab, &S, st))) return rc;
    if ((rc = launch_head_reduce(t->ig_slab, S, B, H2, nullptr, t->a2, 2, t->ig_dz2, st))) return rc;
    if ((rc = launch_head_gemm<false>(t->ig_dz2, nullptr, H2, t->w[1], H1, H2, B, t->ig_slab, &S, st))) return rc;
    if ((rc = launch_head_reduce(t->ig_slab, S, B, H1, nullptr, t->a1, 2, t->ig_dz1, st))) return rc;
    plan_split(K0, H1, &S, &chunk);
    if (S == 1) return launch_head_gemm<false>(t->ig_dz1, nullptr, H1, t->w[0], K0, H1, B, d_dfeat, &S, st);  // one slab is the sum
    if ((rc = launch_head_gemm<false>(t->ig_dz1, nullptr, H1, t->w[0], K0, H1, B, t->ig_slab, &S, st))) return rc;
    const size_t n = (size_t)B * K0;
    hipLaunchKernelGGL(head_sum_slabs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t->ig_slab, S, n, d_dfeat);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

int axt_head_trainer_export(axt_head_trainer *t, axt_detector *det, void *stream)
{
    static const char fn[] = "axt_head_trainer_export";
    AXT_REQUIRE(t && det, "%s: null argument", fn);
    for (int l = 0; l < 3; ++l) {
        int fin, fout;
        if (int rc = axt_detector_linear_spec(l, &fin, &fout)) return rc;
        AXT_REQUIRE(t->dims[l] == fin && t->dims[l + 1] == fout, "%s: the trainer's layer %d is %d -> %d, the detector's %d -> %d",
                    fn, l, t->dims[l], t->dims[l + 1], fin, fout);
    }
    for (int l = 0; l < 3; ++l)
        if (int rc = axt_detector_load_linear(det, l, t->w[l], t->b[l], stream)) return rc;
    return AXT_OK;
}

}  // extern "C"
