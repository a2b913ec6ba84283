// Timelapse preprocessing as ONE fused, HBM-bound pass on gfx950 (the step in front of the
// hot path): reference Timelapse._read_tiff / _clip_image_values / _log_adjust_image / _standardize
// (axtrack/Timelapse.py:205-326), which the reference runs as five numpy passes over the dense timelapse plus a
// scipy.sparse round trip.
//
//   x = u16 * (1/65535)          skimage.util.img_as_float32 (Timelapse.py:207)
//   x = mask ? x : 0             :217
//   x = max(x - offset, 0)       :219-223     (offset already divided by 2^16 by the caller)
//   x = x < clip ? 0 : x         :245-249
//   x = log2(1 + x)              skimage.exposure.adjust_log(x, gain=1) (:255-258)
//   x = x / scale                :312 (the mean is not subtracted)
//
// skimage is absent from the reference tree and from this image (TIFF files are read by tiff.py / tiff.hip, not tifffile): img_as_float32 and adjust_log are
// restated from their published behaviour -- PARITY UNPINNED for those two steps.
// Algorithmic traffic: 2 B in (+ 1 B of mask, cache-resident) and 4 B out per pixel; 8 pixels per lane
// (16-byte load, two 16-byte stores).
//
// Two more passes over the same arithmetic serve the labelled-dataset side:
//   axt_preprocess_stats_u16      the statistics Timelapse._standardize takes of the preprocessed frames before it
//                                 scales them (:286-302: np.mean / np.std / np.max of each frame's non-zero values), as
//                                 per-frame (n, sum, sumsq, max) of the values at scale 1, without writing a frame:
//                                 2 B of traffic per pixel. Deterministic: lane -> wave -> block partials in a scratch
//                                 buffer, a second launch adds each frame's partials in a fixed order; no atomics.
//   axt_preprocess_u16_framewise  axt_preprocess_u16 with one scale per frame (STANDARDIZE_FRAMEWISE, :309-312).
#include "axt_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float prep_one(float x, bool m, float offset, float clip, int log_correct, float scale)
{
    x = m ? x : 0.f;
    if (offset != 0.f) {
        x = __fsub_rn(x, offset);
        x = x < 0.f ? 0.f : x;
    }
    if (clip != 0.f) x = x < clip ? 0.f : x;
    if (log_correct) x = log2f(__fadd_rn(1.0f, x));
    return __fdiv_rn(x, scale);
}

__global__ __launch_bounds__(256) void preprocess_u16_kernel(const unsigned short *__restrict__ raw,
                                                             const unsigned char *__restrict__ mask, long n_px,
                                                             long frame_px, float offset, float clip, int log_correct,
                                                             float scale, float *__restrict__ out)
{
    const float inv = 1.0f / 65535.0f;
    const long stride = (long)gridDim.x * blockDim.x * 8;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n_px; i += stride) {
        if (i + 8 <= n_px && (frame_px % 8 == 0)) {
            const u16x8 v = *reinterpret_cast<const u16x8 *>(raw + i);
            const long mp = i % frame_px;
            f32x4 o0, o1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool m = mask ? mask[mp + j] != 0 : true;
                const float r = prep_one(__fmul_rn((float)v[j], inv), m, offset, clip, log_correct, scale);
                if (j < 4) o0[j] = r; else o1[j - 4] = r;
            }
            *reinterpret_cast<f32x4 *>(out + i) = o0;
            *reinterpret_cast<f32x4 *>(out + i + 4) = o1;
        } else {
            for (long k = i; k < n_px && k < i + 8; ++k) {
                const bool m = mask ? mask[k % frame_px] != 0 : true;
                out[k] = prep_one(__fmul_rn((float)raw[k], inv), m, offset, clip, log_correct, scale);
            }
        }
    }
}

// axt_preprocess_u16 with the scale of the frame a pixel lies in. With frame_px % 8 == 0 the 8 pixels of a lane share a frame.
__global__ __launch_bounds__(256) void preprocess_u16_framewise_kernel(const unsigned short *__restrict__ raw,
                                                                       const unsigned char *__restrict__ mask, long n_px,
                                                                       long frame_px, float offset, float clip,
                                                                       int log_correct, const float *__restrict__ scale,
                                                                       float *__restrict__ out)
{
    const float inv = 1.0f / 65535.0f;
    const long stride = (long)gridDim.x * blockDim.x * 8;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n_px; i += stride) {
        if (i + 8 <= n_px && (frame_px % 8 == 0)) {
            const u16x8 v = *reinterpret_cast<const u16x8 *>(raw + i);
            const long mp = i % frame_px;
            const float sc = scale[i / frame_px];
            f32x4 o0, o1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool m = mask ? mask[mp + j] != 0 : true;
                const float r = prep_one(__fmul_rn((float)v[j], inv), m, offset, clip, log_correct, sc);
                if (j < 4) o0[j] = r; else o1[j - 4] = r;
            }
            *reinterpret_cast<f32x4 *>(out + i) = o0;
            *reinterpret_cast<f32x4 *>(out + i + 4) = o1;
        } else {
            for (long k = i; k < n_px && k < i + 8; ++k) {
                const bool m = mask ? mask[k % frame_px] != 0 : true;
                out[k] = prep_one(__fmul_rn((float)raw[k], inv), m, offset, clip, log_correct, scale[k / frame_px]);
            }
        }
    }
}

// ---- per-frame statistics of the preprocessed values (scale 1) ------------------------------------------------------------
struct StatsAcc {
    long long n = 0;
    double sum = 0.0, sumsq = 0.0;
    float mx = 0.f;                       // the values are >= 0 (u16 counts, clamped at 0 after the offset, log2(1 + x))
    __device__ __forceinline__ void take(float v)
    {
        const double d = (double)v;       // f32 -> f64 is exact, and so is the square of an f32 in f64
        n += v != 0.f;
        sum += d;
        sumsq += d * d;
        mx = fmaxf(mx, v);
    }
    __device__ __forceinline__ void merge(long long n2, double s2, double q2, float m2)
    {
        n += n2; sum += s2; sumsq += q2; mx = fmaxf(mx, m2);
    }
    // sum over the 64 lanes of a wave in a fixed tree order; lane 0 holds the result
    __device__ __forceinline__ void wave_reduce()
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            merge(__shfl_down(n, o, 64), __shfl_down(sum, o, 64), __shfl_down(sumsq, o, 64), __shfl_down(mx, o, 64));
    }
    __device__ __forceinline__ void store(axt_frame_stats *dst) const
    {
        dst->n = n; dst->sum = sum; dst->sumsq = sumsq; dst->max = mx; dst->reserved = 0.f;
    }
};

// Block b works on frame b / bpf alone, as part b % bpf of it (grid-stride over the frame's pixels): which pixels a lane
// adds, and in which order, depends on (H*W, bpf) only. partials [T * bpf].
__global__ __launch_bounds__(256) void preprocess_stats_kernel(const unsigned short *__restrict__ raw,
                                                               const unsigned char *__restrict__ mask, long frame_px,
                                                               int bpf, float offset, float clip, int log_correct,
                                                               axt_frame_stats *__restrict__ partials)
{
    const float inv = 1.0f / 65535.0f;
    const int frame = blockIdx.x / bpf, part = blockIdx.x % bpf;
    const unsigned short *fr = raw + (long)frame * frame_px;
    const bool vec = frame_px % 8 == 0;   // then every frame starts 16-byte aligned and i + 8 <= frame_px below
    const long stride = (long)bpf * blockDim.x * 8;
    StatsAcc a;
    for (long i = ((long)part * blockDim.x + threadIdx.x) * 8; i < frame_px; i += stride) {
        if (vec) {
            const u16x8 v = *reinterpret_cast<const u16x8 *>(fr + i);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool m = mask ? mask[i + j] != 0 : true;
                a.take(prep_one(__fmul_rn((float)v[j], inv), m, offset, clip, log_correct, 1.0f));
            }
        } else {
            for (long k = i; k < frame_px && k < i + 8; ++k) {
                const bool m = mask ? mask[k] != 0 : true;
                a.take(prep_one(__fmul_rn((float)fr[k], inv), m, offset, clip, log_correct, 1.0f));
            }
        }
    }
    a.wave_reduce();
    __shared__ long long s_n[4];
    __shared__ double s_sum[4], s_sumsq[4];
    __shared__ float s_mx[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_n[wave] = a.n; s_sum[wave] = a.sum; s_sumsq[wave] = a.sumsq; s_mx[wave] = a.mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) a.merge(s_n[w], s_sum[w], s_sumsq[w], s_mx[w]);
        a.store(partials + blockIdx.x);
    }
}

// One wave per frame: lane l adds partials l, l + 64, ... in that order, then the wave tree.
__global__ __launch_bounds__(64) void preprocess_stats_finish_kernel(const axt_frame_stats *__restrict__ partials, int bpf,
                                                                     axt_frame_stats *__restrict__ stats)
{
    const axt_frame_stats *p = partials + (long)blockIdx.x * bpf;
    StatsAcc a;
    for (int k = threadIdx.x; k < bpf; k += 64) a.merge(p[k].n, p[k].sum, p[k].sumsq, p[k].max);
    a.wave_reduce();
    if (threadIdx.x == 0) a.store(stats + blockIdx.x);
}

// Blocks per frame: what the frame fills at 8 pixels per lane, bounded so that T frames stay under the block cap of
// axt_preprocess_u16 (frames beyond the cap get one block each).
static int stats_blocks_per_frame(int T, long frame_px)
{
    long bpf = (frame_px / 8 + 255) / 256;
    const long cap = (256 * 8) / T;
    if (bpf > cap) bpf = cap;
    return bpf < 1 ? 1 : (int)bpf;
}

// the arguments the three entry points share: T frames of H x W pixels (a frame's pixels are counted in 31 bits, as
// everywhere in the package, so that T * H * W fits a long), offset and clip_lower finite
static int prep_args_check(const char *fn, int T, int H, int W, float offset, float clip_lower)
{
    AXT_REQUIRE(T > 0 && H > 0 && W > 0 && (long)H * W <= 0x7fffffffL, "%s: bad shape %d x %d x %d", fn, T, H, W);
    AXT_REQUIRE(std::isfinite(offset) && std::isfinite(clip_lower), "%s: offset %g or clip_lower %g is not finite", fn, (double)offset,
                (double)clip_lower);
    return AXT_OK;
}

}  // namespace

extern "C" int axt_preprocess_stats_u16(const uint16_t *d_raw, const uint8_t *d_mask, int T, int H, int W, float offset,
                                        float clip_lower, int log_correct, axt_frame_stats *d_stats, void *d_scratch,
                                        size_t *scratch_bytes, void *stream)
{
    AXT_REQUIRE(scratch_bytes, "axt_preprocess_stats_u16: null argument");
    if (int rc = prep_args_check("axt_preprocess_stats_u16", T, H, W, offset, clip_lower)) return rc;
    const long frame = (long)H * W;
    const int bpf = stats_blocks_per_frame(T, frame);
    const size_t have = *scratch_bytes, need = (size_t)T * bpf * sizeof(axt_frame_stats);
    *scratch_bytes = need;
    if (!d_scratch) return AXT_OK;                    // size query
    AXT_REQUIRE(d_raw && d_stats, "axt_preprocess_stats_u16: null argument");
    AXT_REQUIRE(have >= need, "axt_preprocess_stats_u16: scratch of %zu bytes, %zu needed", have, need);
    axt_frame_stats *partials = static_cast<axt_frame_stats *>(d_scratch);
    hipLaunchKernelGGL(preprocess_stats_kernel, dim3((unsigned)(T * bpf)), dim3(256), 0, (hipStream_t)stream, d_raw, d_mask,
                       frame, bpf, offset, clip_lower, log_correct, partials);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(preprocess_stats_finish_kernel, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, partials, bpf,
                       d_stats);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

extern "C" int axt_preprocess_u16_framewise(const uint16_t *d_raw, const uint8_t *d_mask, int T, int H, int W, float offset,
                                            float clip_lower, int log_correct, const float *d_scale, float *d_out,
                                            void *stream)
{
    AXT_REQUIRE(d_raw && d_out && d_scale, "axt_preprocess_u16_framewise: null argument");
    if (int rc = prep_args_check("axt_preprocess_u16_framewise", T, H, W, offset, clip_lower)) return rc;
    const long n = (long)T * H * W, frame = (long)H * W;
    long blocks = (n / 8 + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(preprocess_u16_framewise_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_raw,
                       d_mask, n, frame, offset, clip_lower, log_correct, d_scale, d_out);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

extern "C" int axt_preprocess_u16(const uint16_t *d_raw, const uint8_t *d_mask, int T, int H, int W, float offset,
                                  float clip_lower, int log_correct, float scale, float *d_out, void *stream)
{
    AXT_REQUIRE(d_raw && d_out, "axt_preprocess_u16: null argument");
    if (int rc = prep_args_check("axt_preprocess_u16", T, H, W, offset, clip_lower)) return rc;
    AXT_REQUIRE(scale > 0.f, "axt_preprocess_u16: scale %g is not above 0", (double)scale);
    const long n = (long)T * H * W, frame = (long)H * W;
    long blocks = (n / 8 + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(preprocess_u16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_raw, d_mask, n,
                       frame, offset, clip_lower, log_correct, scale, d_out);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
