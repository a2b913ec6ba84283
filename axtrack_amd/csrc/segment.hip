// Microchannel segmentation on gfx950: from a transmission image to the mask everything else in the package reads.
//
// The reference makes the mask in a notebook (data_prep_nbs/00_segment_bg.ipynb) with napari and scikit-image:
//   prewitt      = filters.prewitt(transm_chnl)
//   prewitt_g    = filters.gaussian(prewitt, sigma=gaussion_sigma)
//   prewitt_bin  = prewitt > threshold_otsu(prewitt_g)        (threshold of the smoothed image on the unsmoothed one)
//   initial_mask = morphology.binary_closing(prewitt_bin, morphology.square(bin_closing_dim))
//   final_mask   = flood(initial_mask, floodpoint)
// The stages are defined in DESIGN.md 6.8d in terms of SciPy and numpy, which tests/segment_reference.py restates.
//
// axt_segment_edges (stages 1 + 2, one launch): a workgroup of 256 threads owns a 32 x 64 output tile. With
//   R = int(4 sigma + 0.5) it loads the u16 tile with a halo of R + 1 into LDS (reflect, d c b a | a b c d, applied to
//   the index at load), computes the Prewitt magnitude P over the tile plus R -- a cell outside the image takes P of
//   the nearest image cell, which is what mode='nearest' of the smoothing means -- then runs the row pass and the column
//   pass of the Gaussian in LDS. It writes P and G of its tile and folds min(G), max(G) of the tile into two words with
//   one atomic each: G >= 0, so the order of the f32 bit patterns as unsigned integers is the order of the values.
//   LDS at R = 16: (32+34)(64+34) u16 + (32+32)(64+32) f32 + (32+32) 64 f32 = 12.6 + 24 + 16 = 52.6 KiB (3 workgroups
//   per CU); at R = 4 (sigma = 1): 6.1 + 11.3 + 10 = 27.4 KiB (5 per CU). The raw image is read once per tile (the halo
//   again by the neighbours: (66 * 98) / (32 * 64) = 3.2 x at R = 16, 1.5 x at R = 4, from L2).
// axt_segment_histogram (stage 3): 256 LDS bins per workgroup, the 257 f64 edges of np.histogram in LDS; the bin is
//   guessed by one multiply and corrected against the edges (both loops run 256 steps at most), so that the count of
//   every bin is the number of pixels with e_i <= v < e_i+1 (the last bin closed). Integer atomics: the order of the
//   additions does not matter.
// axt_segment_close (stage 4): P > thr as bit-packed rows (one __ballot word per 64 pixels), dilation (OR over the
//   window, 0 outside) and erosion (AND, 1 outside) on the words -- neighbouring words supply the carries of the
//   shifts, k <= 32 < 64 so one word on each side is enough -- and an unpack to bytes.
// axt_segment_flood (stage 5): tiled reachability search in the manner of target.hip. The image becomes two bit planes
//   (open = cells with the seed's value, reach). A tile is 64 x 64 cells: one u64 word per row, one wave per tile, the
//   lane is the row. A sweep is reach |= n & open with n = the horizontal fill of reach inside open (six doubling
//   steps each way) and the rows above and below (__shfl, for 8 neighbours OR-ed with their own left and right
//   shifts), the halo (the neighbour tiles' border bits, read once per visit) entering at lanes 0 and 63 and bits 0
//   and 63. Every sweep but the last reaches at least one more of the tile's 4096 cells. Rounds, worklists, flags and
//   the three counters in rotation are tile_worklist.h's; so is the argument that the result is the unique fixed point:
//   reach only grows, a word has one writer (its tile) and is read and written whole, a tile whose border grew marks
//   the neighbours that have those cells in their halo (for 8 neighbours a corner cell also marks the diagonal tile),
//   so when a round marks nothing every tile has been swept against the final halo. A cell connected to the seed
//   by a path that crosses k tile borders is reached after round k; a path minimal in crossings enters no tile twice
//   through the same one of its 4 * 64 - 4 border cells, so at most n_tiles * 4 * 64 rounds can do work.
#include "axt_common.h"
#include "grid.h"
#include "tile_worklist.h"

namespace {

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------ stages 1 + 2
constexpr int ETY = 32, ETX = 64;            // output tile of segment_edges
constexpr int ENT = 256;
constexpr int MAX_RADIUS = 16;

struct GaussTaps { float w[2 * MAX_RADIUS + 1]; };

__device__ __forceinline__ int reflect_clamp(int i, int n)
{
    if (i < 0) i = -1 - i;
    else if (i >= n) i = 2 * n - 1 - i;
    return min(max(i, 0), n - 1);               // (beyond one reflection: cells no output reads)
}

__global__ __launch_bounds__(64) void minmax_init_kernel(unsigned *__restrict__ mm)
{
    if (threadIdx.x == 0) { mm[0] = 0x7f800000u; mm[1] = 0u; }
}

__global__ __launch_bounds__(ENT) void segment_edges_kernel(const unsigned short *__restrict__ img, int H, int W, int R,
                                                            int tiles_x, GaussTaps taps, float *__restrict__ P,
                                                            float *__restrict__ G, unsigned *__restrict__ minmax)
{
    extern __shared__ unsigned char s_raw[];
    const int IW = ETX + 2 * R + 2, IH = ETY + 2 * R + 2;      // raw tile with its halo
    const int PW = ETX + 2 * R, PH = ETY + 2 * R;              // P over the tile plus R
    float *s_P = reinterpret_cast<float *>(s_raw);
    float *s_row = s_P + PH * PW;                              // [PH][ETX]
    unsigned short *s_img = reinterpret_cast<unsigned short *>(s_row + PH * ETX);
    __shared__ unsigned s_mm[2];
    const int tid = threadIdx.x;
    const int ty0 = (int)(blockIdx.x / tiles_x) * ETY, tx0 = (int)(blockIdx.x % tiles_x) * ETX;
    if (tid == 0) { s_mm[0] = 0x7f800000u; s_mm[1] = 0u; }
    for (int e = tid; e < IH * IW; e += ENT) {
        const int r = e / IW, c = e - r * IW;
        const int gy = reflect_clamp(ty0 - R - 1 + r, H), gx = reflect_clamp(tx0 - R - 1 + c, W);
        s_img[e] = img[(long)gy * W + gx];
    }
    __syncthreads();
    for (int e = tid; e < PH * PW; e += ENT) {
        const int r = e / PW, c = e - r * PW;
        const int gy = ty0 - R + r, gx = tx0 - R + c;
        const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);      // nearest
        // (cy, cx) lies in the tile plus R whenever an output of the image reads this cell, so its 3 x 3 is in s_img
        const int li = min(max(cy - (ty0 - R - 1), 1), IH - 2), lj = min(max(cx - (tx0 - R - 1), 1), IW - 2);
        const unsigned short *q = s_img + li * IW + lj;
        const int a00 = q[-IW - 1], a01 = q[-IW], a02 = q[-IW + 1];
        const int a10 = q[-1], a12 = q[1];
        const int a20 = q[IW - 1], a21 = q[IW], a22 = q[IW + 1];
        const int sy = (a20 + a21 + a22) - (a00 + a01 + a02);             // |.| <= 3 * 65535: exact in f32
        const int sx = (a02 + a12 + a22) - (a00 + a10 + a20);
        const float fy = (float)sy / 3.0f, fx = (float)sx / 3.0f;
        const float p = sqrtf((fy * fy + fx * fx) * 0.5f);
        s_P[e] = p;
        if (r >= R && r < R + ETY && c >= R && c < R + ETX && gy < H && gx < W) P[(long)gy * W + gx] = p;
    }
    __syncthreads();
    const int nt = 2 * R + 1;
    for (int e = tid; e < PH * ETX; e += ENT) {
        const int r = e / ETX, c = e - r * ETX;
        const float *q = s_P + r * PW + c;
        float acc = 0.0f;
        for (int k = 0; k < nt; ++k) acc = fmaf(taps.w[k], q[k], acc);
        s_row[e] = acc;
    }
    __syncthreads();
    unsigned lo = 0x7f800000u, hi = 0u;
    for (int e = tid; e < ETY * ETX; e += ENT) {
        const int r = e / ETX, c = e - r * ETX;
        const int gy = ty0 + r, gx = tx0 + c;
        if (gy >= H || gx >= W) continue;
        const float *q = s_row + r * ETX + c;
        float acc = 0.0f;
        for (int k = 0; k < nt; ++k) acc = fmaf(taps.w[k], q[k * ETX], acc);
        G[(long)gy * W + gx] = acc;
        const unsigned b = __float_as_uint(acc);
        lo = min(lo, b);
        hi = max(hi, b);
    }
    for (int s = 32; s >= 1; s >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, s));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, s));
    }
    if ((tid & 63) == 0) { atomicMin(&s_mm[0], lo); atomicMax(&s_mm[1], hi); }
    __syncthreads();
    if (tid == 0) { atomicMin(&minmax[0], s_mm[0]); atomicMax(&minmax[1], s_mm[1]); }
}

// ------------------------------------------------------------------------------------------------ stage 3
constexpr int HNT = 256, HBINS = 256, HMAX_BLOCKS = 1024;

struct HistEdges { double e[HBINS + 1]; };

__global__ __launch_bounds__(HNT) void segment_histogram_kernel(const float *__restrict__ G, long n, HistEdges edges,
                                                                double scale, int flat, u64 *__restrict__ hist)
{
    __shared__ double s_e[HBINS + 1];
    __shared__ unsigned s_bin[HBINS];             // (a workgroup counts fewer than 2^31 pixels)
    const int tid = threadIdx.x;
    for (int i = tid; i <= HBINS; i += HNT) s_e[i] = edges.e[i];
    s_bin[tid] = 0;
    __syncthreads();
    const double mn = s_e[0], mx = s_e[HBINS];
    for (long i = (long)blockIdx.x * HNT + tid; i < n; i += (long)gridDim.x * HNT) {
        const double v = (double)G[i];
        if (!(v >= mn && v <= mx)) continue;      // (np.histogram drops what lies outside the range, NaN included)
        int b = 0;
        if (!flat) {
            b = min(max((int)((v - mn) * scale), 0), HBINS - 1);
            for (int s = 0; s < HBINS && b > 0 && v < s_e[b]; ++s) --b;
            for (int s = 0; s < HBINS && b < HBINS - 1 && v >= s_e[b + 1]; ++s) ++b;
        }
        atomicAdd(&s_bin[b], 1u);
    }
    __syncthreads();
    const unsigned c = s_bin[tid];
    if (c) atomicAdd(&hist[tid], (u64)c);
}

// ------------------------------------------------------------------------------------------------ stage 4
// bit x & 63 of word x >> 6 of a row is pixel x; bits at and beyond W are 0 in what binarise writes
__global__ __launch_bounds__(256) void binarise_kernel(const float *__restrict__ P, int H, int W, int WW, double thr,
                                                       u64 *__restrict__ bits)
{
    const int bx = (W + 255) / 256;                                       // blocks per row; a wave is one word
    const int y = blockIdx.x / bx, x = (blockIdx.x % bx) * 256 + threadIdx.x;
    const bool on = x < W && (double)P[(long)y * W + x] > thr;
    const u64 word = __ballot(on);
    if ((threadIdx.x & 63) == 0 && (x >> 6) < WW) bits[(long)y * WW + (x >> 6)] = word;
}

// bits of pixels at and beyond W in the last word of a row
__device__ __forceinline__ u64 tail_mask(int W, int WW, int wx)
{
    const int used = W - 64 * (WW - 1);
    return (wx == WW - 1 && used < 64) ? ~0ull << used : 0ull;
}

// DILATE: out[y][x] = OR in[y-b .. y+a][x-b .. x+a], 0 outside. ERODE: out[y][x] = AND in[y-a .. y+b][x-a .. x+b], 1
// outside (the image border and the unused bits of a row's last word). a = k / 2, b = k - 1 - a. One thread per word.
template <bool DILATE>
__global__ __launch_bounds__(256) void morph_kernel(const u64 *__restrict__ in, int H, int W, int WW, int k, u64 *__restrict__ out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)H * WW) return;
    const int y = (int)(i / WW), wx = (int)(i - (long)y * WW);
    const int a = k / 2, b = k - 1 - a;
    const int before = DILATE ? b : a, after = DILATE ? a : b;            // window [-before, +after] on both axes
    const u64 outside = DILATE ? 0ull : ~0ull;
    const u64 tail = DILATE ? 0ull : tail_mask(W, WW, wx);
    u64 prev = outside, cur = outside, next = outside;
    for (int d = -before; d <= after; ++d) {
        const int yy = y + d;
        u64 p = outside, c = outside, nx = outside;
        if (yy >= 0 && yy < H) {
            const u64 *row = in + (long)yy * WW;
            c = row[wx] | tail;
            if (wx > 0) p = row[wx - 1];
            if (wx + 1 < WW) nx = row[wx + 1] | (DILATE ? 0ull : tail_mask(W, WW, wx + 1));
        }
        if (DILATE) { prev |= p; cur |= c; next |= nx; }
        else { prev &= p; cur &= c; next &= nx; }
    }
    u64 acc = cur;
    for (int s = 1; s <= after; ++s) {                                   // pixel x + s
        const u64 v = (cur >> s) | (next << (64 - s));
        acc = DILATE ? acc | v : acc & v;
    }
    for (int s = 1; s <= before; ++s) {                                  // pixel x - s
        const u64 v = (cur << s) | (prev >> (64 - s));
        acc = DILATE ? acc | v : acc & v;
    }
    out[i] = acc;
}

__global__ __launch_bounds__(256) void unpack_kernel(const u64 *__restrict__ bits, int H, int W, int WW, unsigned char *__restrict__ out)
{
    const int bx = (W + 255) / 256;
    const int y = blockIdx.x / bx, x = (blockIdx.x % bx) * 256 + threadIdx.x;
    if (x < W) out[(long)y * W + x] = (unsigned char)(bits[(long)y * WW + (x >> 6)] >> (x & 63) & 1ull);
}

// ------------------------------------------------------------------------------------------------ stage 5
constexpr int FTS = 64;                      // tile edge: a row of a tile is one word, a tile is one wave

__device__ __forceinline__ u64 word_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// open = cells with the seed's value, reach = 0 but for the seed; the worklist state of tile_worklist.h, the seed's tile
// being the worklist of round 0
__global__ __launch_bounds__(256) void flood_init_kernel(const unsigned char *__restrict__ img, int H, int W, int WW, int seed_y,
                                                         int seed_x, u64 *__restrict__ open, u64 *__restrict__ reach,
                                                         int *__restrict__ ctrl, int *__restrict__ flags, int *__restrict__ lists,
                                                         int n_tiles)
{
    const int bx = (W + 255) / 256;
    const int y = blockIdx.x / bx, x = (blockIdx.x % bx) * 256 + threadIdx.x;
    const unsigned char sv = img[(long)seed_y * W + seed_x] ? 1 : 0;
    const bool on = x < W && (img[(long)y * W + x] ? 1 : 0) == sv;
    const u64 word = __ballot(on);
    const int wx = x >> 6;
    if ((threadIdx.x & 63) == 0 && wx < WW) {
        open[(long)y * WW + wx] = word;
        reach[(long)y * WW + wx] = (y == seed_y && wx == (seed_x >> 6)) ? 1ull << (seed_x & 63) : 0ull;
    }
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (long j = i; j < 2L * n_tiles; j += (long)gridDim.x * 256) flags[j] = 0;
    if (i == 0) {
        const int t = (seed_y / FTS) * WW + (seed_x >> 6);
        ctrl[0] = 1; ctrl[1] = 0; ctrl[2] = 0; ctrl[3] = 0;
        lists[0] = t;
    }
}

// One round: wave b sweeps tile lists[par][b] to its fixed point for the halo it read (see the top). flags
// [2][n_tiles], lists [2][n_tiles]. The flag of the seed's tile for round 0 is never set: nothing marks for round 0.
__global__ __launch_bounds__(64) void flood_round_kernel(const u64 *__restrict__ open, u64 *__restrict__ reach, int H, int WW,
                                                         int tiles_y, int conn8, int round, int *__restrict__ ctrl,
                                                         int *__restrict__ flags, int *__restrict__ lists)
{
    const int lane = threadIdx.x, tiles_x = WW;
    const int t = axt_worklist_take(round, tiles_x * tiles_y, ctrl, flags, lists);
    if (t < 0) return;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y = ty * FTS + lane;
    const bool in = y < H;
    const long at = (long)y * WW + tx;
    const u64 op = in ? open[at] : 0ull;
    const u64 first = in ? word_load(&reach[at]) : 0ull;
    // the halo: bit 63 of the word to the left, bit 0 of the word to the right, the rows above and below (lanes 0, 63)
    u64 hl = (in && tx > 0) ? word_load(&reach[at - 1]) >> 63 : 0ull;
    u64 hr = (in && tx + 1 < tiles_x) ? word_load(&reach[at + 1]) & 1ull : 0ull;
    u64 top = 0ull, bot = 0ull, cl = 0ull, cr = 0ull;  // (lane 0 / lane 63 only; cl, cr: the corner cells)
    if (lane == 0 && y > 0 && in) {
        const long up = at - WW;
        top = word_load(&reach[up]);
        if (conn8 && tx > 0) cl = word_load(&reach[up - 1]) >> 63;
        if (conn8 && tx + 1 < tiles_x) cr = word_load(&reach[up + 1]) & 1ull;
    }
    if (lane == FTS - 1 && y + 1 < H) {
        const long dn = at + WW;
        bot = word_load(&reach[dn]);
        if (conn8 && tx > 0) cl = word_load(&reach[dn - 1]) >> 63;
        if (conn8 && tx + 1 < tiles_x) cr = word_load(&reach[dn + 1]) & 1ull;
    }
    if (conn8) {                                      // a halo cell also touches the rows above and below its own
        const u64 l_up = __shfl_up(hl, 1), l_dn = __shfl_down(hl, 1), r_up = __shfl_up(hr, 1), r_dn = __shfl_down(hr, 1);
        hl |= (lane > 0 ? l_up : 0ull) | (lane < FTS - 1 ? l_dn : 0ull) | cl;
        hr |= (lane > 0 ? r_up : 0ull) | (lane < FTS - 1 ? r_dn : 0ull) | cr;
    }
    const u64 halo = hl | hr << 63;
    u64 r = first;
    for (int sweep = 0; sweep <= FTS * FTS; ++sweep) {
        const u64 s_up = __shfl_up(r, 1), s_dn = __shfl_down(r, 1);
        u64 v = (lane > 0 ? s_up : top) | (lane < FTS - 1 ? s_dn : bot);
        if (conn8) v |= v << 1 | v >> 1;
        u64 g = r | ((v | halo) & op);
        // horizontal fill of g inside op, to the left (<<) and to the right (>>)
        u64 gl = g, pl = op, gr = g, pr = op;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            gl |= pl & (gl << s); pl &= pl << s;
            gr |= pr & (gr >> s); pr &= pr >> s;
        }
        g = gl | gr;
        const bool changed = g != r;
        r = g;
        if (!__any(changed)) break;
    }
    const u64 grown = r & ~first;
    if (grown) __hip_atomic_store(&reach[at], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (in: op = 0 below H)
    const u64 any_l = __ballot((grown & 1ull) != 0), any_r = __ballot((grown >> 63) != 0);
    const u64 g_top = __shfl(grown, 0), g_bot = __shfl(grown, FTS - 1);
    int dirs = (g_top ? 1 : 0) | (g_bot ? 2 : 0) | (any_l ? 4 : 0) | (any_r ? 8 : 0);       // (bits in the neighbour order)
    if (conn8) dirs |= ((g_top & 1ull) ? 16 : 0) | ((g_top >> 63) ? 32 : 0) | ((g_bot & 1ull) ? 64 : 0) | ((g_bot >> 63) ? 128 : 0);
    __threadfence();                                  // the words before the marks
    axt_worklist_mark(dirs, t, tiles_x, tiles_y, round, ctrl, flags, lists);
}

int radius_of(double sigma) { return (int)(4.0 * sigma + 0.5); }

}  // namespace

extern "C" int axt_segment_tile_size(void) { return FTS; }

extern "C" int axt_segment_edges(const uint16_t *d_img, int H, int W, double sigma, float *d_P, float *d_G, float *d_minmax,
                                 void *stream)
{
    AXT_REQUIRE(H > 0 && W > 0 && (long)H * W <= 0x7fffffffL, "axt_segment_edges: bad image size %d x %d", H, W);
    AXT_REQUIRE(sigma > 0.0 && sigma <= MAX_RADIUS && radius_of(sigma) <= MAX_RADIUS,
                "axt_segment_edges: sigma %g needs a radius int(4 sigma + 0.5) in [0, %d]", sigma, MAX_RADIUS);
    const int R = radius_of(sigma);
    AXT_REQUIRE(H >= 2 * R + 2 && W >= 2 * R + 2, "axt_segment_edges: a %d x %d image is smaller than %d (2 radius + 2)", H, W,
                2 * R + 2);
    AXT_REQUIRE(d_img && d_P && d_G && d_minmax, "axt_segment_edges: null argument");
    hipStream_t st = (hipStream_t)stream;
    // scipy.ndimage._filters._gaussian_kernel1d: exp(-x^2 / 2 sigma^2), normalised, in f64; then rounded to f32
    GaussTaps taps;
    double w[2 * MAX_RADIUS + 1], sum = 0.0;
    // (the centre tap is 1 by definition: for a sigma whose square underflows, -0.5 / 0 * 0 would be NaN)
    for (int k = 0; k <= 2 * R; ++k) { const double x = k - R; w[k] = k == R ? 1.0 : exp(-0.5 / (sigma * sigma) * x * x); sum += w[k]; }
    for (int k = 0; k <= 2 * MAX_RADIUS; ++k) taps.w[k] = k <= 2 * R ? (float)(w[k] / sum) : 0.0f;
    const size_t lds = sizeof(float) * ((size_t)(ETY + 2 * R) * (ETX + 2 * R) + (size_t)(ETY + 2 * R) * ETX) +
                       sizeof(unsigned short) * (size_t)(ETY + 2 * R + 2) * (ETX + 2 * R + 2);      // <= 53.9 KB
    const int tiles_x = axt_cdiv(W, ETX);
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned *>(d_minmax));
    hipLaunchKernelGGL(segment_edges_kernel, dim3((unsigned)((long)tiles_x * axt_cdiv(H, ETY))), dim3(ENT), lds, st, d_img, H, W, R,
                       tiles_x, taps, d_P, d_G, reinterpret_cast<unsigned *>(d_minmax));
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

extern "C" int axt_segment_histogram(const float *d_G, int64_t n, double mn, double mx, int64_t *d_hist, void *stream)
{
    AXT_REQUIRE(n >= 1 && n <= 0x7fffffffL, "axt_segment_histogram: bad pixel count %lld", (long long)n);
    AXT_REQUIRE(mn <= mx && mx - mn <= 3.5e38 && mn >= -3.5e38, "axt_segment_histogram: bad range [%g, %g]", mn, mx);
    AXT_REQUIRE(d_G && d_hist, "axt_segment_histogram: null argument");
    hipStream_t st = (hipStream_t)stream;
    // np.linspace(mn, mx, 257): arange(257) * step + mn with step = (mx - mn) / 256, the last edge = mx; two roundings
    // per edge (the volatile keeps the product from being fused into the sum)
    HistEdges edges;
    const double step = (mx - mn) / HBINS;
    for (int i = 0; i < HBINS; ++i) { volatile double p = (double)i * step; edges.e[i] = p + mn; }
    edges.e[HBINS] = mx;
    const int flat = !(mx > mn);
    const double scale = flat ? 0.0 : HBINS / (mx - mn);
    AXT_CHECK_HIP(hipMemsetAsync(d_hist, 0, sizeof(int64_t) * HBINS, st));
    const long blocks = (n + HNT - 1) / HNT;
    hipLaunchKernelGGL(segment_histogram_kernel, dim3((unsigned)(blocks < HMAX_BLOCKS ? blocks : HMAX_BLOCKS)), dim3(HNT), 0, st,
                       d_G, (long)n, edges, scale, flat, reinterpret_cast<u64 *>(d_hist));
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

extern "C" int axt_segment_close(const float *d_P, int H, int W, double thr, int k, uint8_t *d_out, void *stream)
{
    AXT_REQUIRE(H > 0 && W > 0 && (long)H * W <= 0x7fffffffL, "axt_segment_close: bad image size %d x %d", H, W);
    AXT_REQUIRE(k >= 2 && k <= 32, "axt_segment_close: bin_closing_dim %d is outside [2, 32]", k);
    AXT_REQUIRE(thr == thr, "axt_segment_close: the threshold is not a number");
    AXT_REQUIRE(d_P && d_out, "axt_segment_close: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int WW = axt_cdiv(W, 64);
    const size_t words = (size_t)H * WW;
    u64 *bits = nullptr;
    AXT_CHECK_HIP(hipMallocAsync((void **)&bits, 2 * words * sizeof(u64), st));
    u64 *b0 = bits, *b1 = bits + words;
    const dim3 px((unsigned)((long)H * axt_cdiv(W, 256)));
    const unsigned nb = (unsigned)((words + 255) / 256);
    hipLaunchKernelGGL(binarise_kernel, px, dim3(256), 0, st, d_P, H, W, WW, thr, b0);
    hipLaunchKernelGGL(morph_kernel<true>, dim3(nb), dim3(256), 0, st, (const u64 *)b0, H, W, WW, k, b1);
    hipLaunchKernelGGL(morph_kernel<false>, dim3(nb), dim3(256), 0, st, (const u64 *)b1, H, W, WW, k, b0);
    hipLaunchKernelGGL(unpack_kernel, px, dim3(256), 0, st, (const u64 *)b0, H, W, WW, d_out);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(bits, st);
    if (e != hipSuccess) { axt_set_error("axt_segment_close: %s", hipGetErrorString(e)); return AXT_EHIP; }
    return AXT_OK;
}

extern "C" int axt_segment_flood(const uint8_t *d_img, int H, int W, int seed_y, int seed_x, int conn8, uint8_t *d_out,
                                 int *rounds_out, void *stream)
{
    AXT_REQUIRE(H > 0 && W > 0 && (long)H * W <= 0x7fffffffL, "axt_segment_flood: bad image size %d x %d", H, W);
    AXT_REQUIRE(seed_y >= 0 && seed_y < H && seed_x >= 0 && seed_x < W, "axt_segment_flood: the seed (%d, %d) is outside %d x %d",
                seed_y, seed_x, H, W);
    AXT_REQUIRE(d_img && d_out, "axt_segment_flood: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int WW = axt_cdiv(W, 64), tiles_y = axt_cdiv(H, FTS);
    const long n_tiles_l = (long)WW * tiles_y;
    const int n_tiles = (int)n_tiles_l;
    const size_t words = (size_t)H * WW;
    // scratch: open u64 [H][WW], reach u64 [H][WW], then i32: ctrl [4], flags [2][n_tiles], lists [2][n_tiles]
    AxtScratch raw(st, 2 * words * sizeof(u64) + sizeof(int) * (4 + 4 * (size_t)n_tiles));
    AXT_CHECK_HIP(raw.err);
    u64 *open = raw.as<u64>(), *reach = open + words;
    int *ctrl = reinterpret_cast<int *>(reach + words);
    int *flags = ctrl + 4, *lists = flags + 2 * (size_t)n_tiles;
    const dim3 px((unsigned)((long)H * axt_cdiv(W, 256)));
    hipLaunchKernelGGL(flood_init_kernel, px, dim3(256), 0, st, d_img, H, W, WW, seed_y, seed_x, open, reach, ctrl, flags, lists,
                       n_tiles);
    int rounds = 0;
    int rc = axt_worklist_run("axt_segment_flood", [&](int r) {
        hipLaunchKernelGGL(flood_round_kernel, dim3(n_tiles), dim3(64), 0, st, (const u64 *)open, reach, H, WW, tiles_y,
                           conn8 ? 1 : 0, r, ctrl, flags, lists);
    }, ctrl, n_tiles_l, FTS, st, &rounds);
    if (rc == AXT_OK) {
        hipLaunchKernelGGL(unpack_kernel, px, dim3(256), 0, st, (const u64 *)reach, H, W, WW, d_out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { axt_set_error("axt_segment_flood: %s", hipGetErrorString(e)); rc = AXT_EHIP; }
    }
    if (rounds_out) *rounds_out = rc == AXT_OK ? rounds : 0;
    return rc;
}
