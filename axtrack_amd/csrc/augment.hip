// augment.hip -- the training augmentation of a whole timelapse as ONE bandwidth-bound pass on gfx950:
// translate, then flip, then rotate, as data_utils.transform_X applies them (three passes through sparse / dense
// conversions and the host in the reference), plus the per-frame tile occupancy of the warped frames.
//
// The kernel is a gather: an output pixel (y, x) applies the inverses in reverse order.
//   1. rotation   torchvision's TF.rotate(img, angle) for tensors (nearest, no expand, fill 0), i.e. grid_sample(nearest,
//                 zeros, align_corners=False) on the affine grid of the inverse matrix. In f32 and in this order:
//                   bx = x - W/2 + 0.5, by = y - H/2 + 0.5                    (the grid's base coordinates, exact)
//                   gx = bx * t00 + by * t01,  gy = bx * t10 + by * t11       (t = matrix / (0.5 W | 0.5 H), from the host;
//                                                                              two rounded products, one rounded sum)
//                   ix = ((gx + 1) * W - 1) / 2, iy likewise with H
//                   sx = rintf(ix), sy = rintf(iy)                            (round half to even); outside the frame: 0
//   2. flip       sy = H-1-sy and / or sx = W-1-sx
//   3. translate  sy -= dy, sx -= dx; outside the frame: 0
// The source index of a pixel is the same for every frame: a thread forms the indices of its 4 neighbouring pixels once
// and loops over the kAugFrameChunk frames of its blockIdx.z. No LDS, no MFMA, no atomics.
//
// Launch: block (64, 4) = one wave per row, 4 rows; grid (ceil(W / 256), ceil(H / 4), ceil(T / kAugFrameChunk)).
// A wave covers 256 neighbouring pixels of one row, which never straddle a 512-tile: the occupancy of (frame, tile) is a
// wave ballot of "one of my pixels is > 0" and one plain byte store of 1 from lane 0. Many waves may store the same 1.
// Stores are 16 bytes per lane where W % 4 == 0 and d_out is 16-byte aligned (every row then starts aligned); otherwise
// scalar, the last lane of a row writing the tail. Without rotation the loads of a wave are 1 KiB contiguous (descending
// under flip_x); with rotation they follow a line of slope tan(angle) through the source rows.
#include "axt_common.h"

namespace {

constexpr int kAugFrameChunk = 6;
constexpr int kAugPx = 4;            // pixels per lane
constexpr int kAugRows = 4;          // rows (waves) per block

struct AugXform {
    long long dy, dx;
    int flip_y, flip_x;
    float t00, t01, t10, t11;
};

typedef float aug_f32x4 __attribute__((ext_vector_type(4)));

// offset of the source pixel of output (y, x) inside a frame, or -1 where the output is zero
template <bool ROT>
__device__ __forceinline__ int aug_source(int y, int x, int H, int W, const AugXform &p)
{
    long long sy = y, sx = x;
    if (ROT) {
        const float bx = __fadd_rn(__fsub_rn((float)x, __fmul_rn(0.5f, (float)W)), 0.5f);
        const float by = __fadd_rn(__fsub_rn((float)y, __fmul_rn(0.5f, (float)H)), 0.5f);
        const float gx = __fadd_rn(__fmul_rn(bx, p.t00), __fmul_rn(by, p.t01));
        const float gy = __fadd_rn(__fmul_rn(bx, p.t10), __fmul_rn(by, p.t11));
        const float ix = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.0f), (float)W), 1.0f), 2.0f);
        const float iy = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.0f), (float)H), 1.0f), 2.0f);
        const float rx = rintf(ix), ry = rintf(iy);
        if (!(rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H)) return -1;       // (also NaN)
        sx = (long long)rx;
        sy = (long long)ry;
    }
    if (p.flip_y) sy = H - 1 - sy;
    if (p.flip_x) sx = W - 1 - sx;
    sy -= p.dy;
    sx -= p.dx;
    if (sy < 0 || sy >= H || sx < 0 || sx >= W) return -1;
    return (int)(sy * W + sx);
}

template <bool ROT, bool VEC>
__global__ __launch_bounds__(64 * kAugRows) void augment_frames_k(const float *__restrict__ in, float *__restrict__ out,
                                                                uint8_t *__restrict__ occ, int T, int H, int W, int ntx,
                                                                int n_tiles, AugXform p)
{
    const int y = blockIdx.y * kAugRows + threadIdx.y;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * kAugPx;
    const bool live = y < H && x0 < W;                         // (no early return: every lane takes part in the ballot)
    int src[kAugPx];
#pragma unroll
    for (int j = 0; j < kAugPx; ++j) src[j] = (live && x0 + j < W) ? aug_source<ROT>(y, x0 + j, H, W, p) : -1;
    const size_t frame = (size_t)H * W;
    const size_t o = (size_t)(live ? y : 0) * W + (live ? x0 : 0);
    const int tile = live ? (y / AXT_TILE) * ntx + x0 / AXT_TILE : 0;          // wave-uniform
    const int t0 = blockIdx.z * kAugFrameChunk, t1 = min(T, t0 + kAugFrameChunk);
    for (int t = t0; t < t1; ++t) {
        const float *f = in + (size_t)t * frame;
        float v[kAugPx];
#pragma unroll
        for (int j = 0; j < kAugPx; ++j) v[j] = src[j] >= 0 ? f[src[j]] : 0.f;
        if (live) {
            float *dst = out + (size_t)t * frame + o;
            if (VEC) {
                aug_f32x4 q = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<aug_f32x4 *>(dst) = q;
            } else {
#pragma unroll
                for (int j = 0; j < kAugPx; ++j)
                    if (x0 + j < W) dst[j] = v[j];
            }
        }
        if (occ) {
            const bool any = v[0] > 0.f || v[1] > 0.f || v[2] > 0.f || v[3] > 0.f;       // (a dead pixel holds 0)
            if (__ballot(any) != 0ull && threadIdx.x == 0) occ[(size_t)t * n_tiles + tile] = 1;
        }
    }
}

}  // namespace

extern "C" int axt_augment_frame_chunk(void) { return kAugFrameChunk; }

extern "C" int axt_augment_frames(const float *d_in, int T, int H, int W, int dy, int dx, int flip_y, int flip_x,
                                  int rotate, float m00, float m01, float m10, float m11, float *d_out, uint8_t *d_occ,
                                  void *stream)
{
    AXT_REQUIRE(d_in && d_out, "axt_augment_frames: null argument");
    AXT_REQUIRE(T >= 1 && H >= 1 && W >= 1, "axt_augment_frames: bad shape T=%d H=%d W=%d", T, H, W);
    AXT_REQUIRE((long long)H * W <= 0x7fffffffLL, "axt_augment_frames: a frame of %d x %d pixels: the pixel index must fit 31 bits", H, W);
    AXT_REQUIRE(!rotate || (std::isfinite(m00) && std::isfinite(m01) && std::isfinite(m10) && std::isfinite(m11)),
                "axt_augment_frames: the rotation matrix (%g %g / %g %g) is not finite", (double)m00, (double)m01, (double)m10, (double)m11);
    const dim3 block(64, kAugRows), grid(axt_cdiv(W, 64 * kAugPx), axt_cdiv(H, kAugRows), axt_cdiv(T, kAugFrameChunk));
    AXT_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "axt_augment_frames: timelapse too large for one launch (H <= %d, T <= %d)",
                65535 * kAugRows, 65535 * kAugFrameChunk);
    const size_t n = (size_t)T * H * W;
    AXT_REQUIRE(d_out + n <= d_in || d_in + n <= d_out, "axt_augment_frames: d_out overlaps d_in: the warp is a gather and cannot run in place");
    hipStream_t st = (hipStream_t)stream;
    const int nty = axt_cdiv(H, AXT_TILE), ntx = axt_cdiv(W, AXT_TILE);
    if (d_occ) AXT_CHECK_HIP(hipMemsetAsync(d_occ, 0, (size_t)T * nty * ntx, st));
    AugXform p;
    p.dy = dy, p.dx = dx, p.flip_y = flip_y != 0, p.flip_x = flip_x != 0;
    // rescaled_theta of torchvision's _gen_affine_grid: the f32 matrix entries divided by 0.5 W (x row) and 0.5 H (y row)
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    p.t00 = m00 / hw, p.t01 = m01 / hw, p.t10 = m10 / hh, p.t11 = m11 / hh;
    const bool vec = W % 4 == 0 && ((uintptr_t)d_out & 15) == 0;
#define AXT_AUG_LAUNCH(ROT, VEC)                                                                                        \
    hipLaunchKernelGGL((augment_frames_k<ROT, VEC>), grid, block, 0, st, d_in, d_out, d_occ, T, H, W, ntx, nty * ntx, p)
    if (rotate) {
        if (vec) AXT_AUG_LAUNCH(true, true); else AXT_AUG_LAUNCH(true, false);
    } else {
        if (vec) AXT_AUG_LAUNCH(false, true); else AXT_AUG_LAUNCH(false, false);
    }
#undef AXT_AUG_LAUNCH
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
