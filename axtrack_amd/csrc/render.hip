// Annotated RGB frames of a tracking result on gfx950 (video_plotting.py draw_all / setup_frame_drawing / draw_frame /
// draw_detections; DESIGN.md 6.8b has the rules).
//
// One workgroup per (64 x 64 output tile, run of output frames). It walks its frames in order:
//   * trails: the tile's trail canvas (max key per pixel) stays in LDS across the frames of the run; each frame adds the
//     5 x 5 squares of the cells whose segment ends at or before it (the tile's cell list is sorted by frame, so the
//     history is splatted once per workgroup, not once per frame);
//   * target paths and target cells (kind 4 rectangles, key 1 = path, 2 = target): a byte plane per frame, the paths
//     first, the target cells after a barrier, so that the target wins wherever both fall (every writer of a pass
//     stores the same value);
//   * boxes, labels, header: one LDS key plane per frame, filled from the (frame, tile) primitive list with LDS max
//     atomics: key = layer << 24 | (n + 1), so the upper layer wins and, within a layer, the larger n; ground-truth
//     outlines set a flag plane (the same value from every writer);
//   * brightened background: the weight map of the tile with a 12-pixel halo (3 passes x radius 4) in LDS, three
//     horizontal and three vertical 9-tap box passes, each clamped at the FRAME edges, so a slice is an exact crop;
//   * one thread per 16 consecutive pixels of a row resolves the layers and writes 48 bytes (three 16-byte stores when
//     the row start is aligned).
// Every pixel is written by one thread and every overlap is decided by a max: the output does not depend on scheduling.
// The binned lists (trail cells, primitives) are built by axtrack_amd/render.py.
#include <algorithm>

#include "axt_common.h"

namespace {
constexpr int RT = 64;               // output tile edge
constexpr int HALO = 12;             // 3 box passes of radius 4
constexpr int BW = RT + 2 * HALO;    // 88: blur window edge
constexpr int NT = 256;              // 64 rows x 4 groups of 16 pixels
constexpr int GLYPHS = 95;           // printable ASCII 32..126

// one drawing primitive in output coordinates (axtrack_amd/render.py:_PRIM_FIELDS)
struct Prim { int x0, y0, kind, a, b, key, pad0, pad1; };
enum { P_DASHED = 0, P_SOLID = 1, P_GLYPH = 2, P_RECT = 3, P_TARGET = 4 };
enum { TGT_PATH = 1, TGT_CELL = 2 };

struct RenderArgs {
    const float *frames;        // detection frame t at frames + t * H * W (the context frames are skipped by the caller)
    const uint8_t *mask;        // mask of detection frame t at mask + t * mask_stride; NULL = all ones
    long long mask_stride;
    const int32_t *ts;          // [n_out] detection frame of each output frame, ascending
    int n_out, H, W, ymin, xmin, Ho, Wo, ntx, nty, chunk, grid, bg;
    const int32_t *trail_ptr;   // [ntiles + 1]
    const int32_t *trail;       // [n, 4] frame, key, x, y (output coordinates), per tile sorted by frame
    const uint8_t *trail_col;   // [keys + 1] palette index of each trail key
    const int32_t *prim_ptr;    // [n_out * ntiles + 1]
    const Prim *prims;
    const uint8_t *tables;      // palette u8 [20, 3], then glyph rows u8 [95, 7] (bit 4 = leftmost column)
    uint8_t *out;               // [n_out, Ho, Wo, 3]
};

__device__ __forceinline__ int r8_of(float v) { return (int)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }
__device__ __forceinline__ int blend(int a, int C, int c) { return (a * C + (256 - a) * c + 128) >> 8; }

__global__ __launch_bounds__(NT) void render_tiles(RenderArgs a)
{
    __shared__ uint16_t bufA[BW * BW], bufB[BW * BW];
    __shared__ uint32_t trail[RT * RT], over[RT * RT];
    __shared__ uint8_t gt[RT * RT], tgt[RT * RT];
    const int ntiles = a.ntx * a.nty;
    const int tile = blockIdx.x % ntiles, run = blockIdx.x / ntiles;
    const int oy0 = (tile / a.ntx) * RT, ox0 = (tile % a.ntx) * RT;
    const int fy0 = oy0 + a.ymin, fx0 = ox0 + a.xmin;
    const int i0 = run * a.chunk, i1 = min(i0 + a.chunk, a.n_out);
    const int tid = threadIdx.x;
    const long long HW = (long long)a.H * a.W;
    const uint8_t *pal = a.tables, *glyph = a.tables + 60;

    for (int k = tid; k < RT * RT; k += NT) trail[k] = 0u;
    int p = a.trail_ptr[tile];
    const int pend = a.trail_ptr[tile + 1];
    for (int i = i0; i < i1; ++i) {
        const int f = a.ts[i];
        __syncthreads();                                      // (the previous frame's reads of the planes are done)
        for (int k = tid; k < RT * RT; k += NT) { over[k] = 0u; gt[k] = 0; tgt[k] = 0; }
        // trail cells of segments ending at or before f: [p, q)
        int lo = p, hi = pend;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.trail[4 * mid] <= f) lo = mid + 1; else hi = mid;
        }
        __syncthreads();
        for (int j = p + tid; j < lo; j += NT) {
            const uint32_t key = (uint32_t)a.trail[4 * j + 1];
            const int lx = a.trail[4 * j + 2] - ox0, ly = a.trail[4 * j + 3] - oy0;
            for (int dy = -2; dy <= 2; ++dy) {
                const int yy = ly + dy;
                if (yy < 0 || yy >= RT) continue;
                for (int dx = -2; dx <= 2; ++dx) {
                    const int xx = lx + dx;
                    if (xx >= 0 && xx < RT) atomicMax(&trail[yy * RT + xx], key);
                }
            }
        }
        p = lo;
        const int q0 = a.prim_ptr[(long long)i * ntiles + tile], q1 = a.prim_ptr[(long long)i * ntiles + tile + 1];
        for (int j = q0 + tid; j < q1; j += NT) {
            const Prim pr = a.prims[j];
            const int x0 = pr.x0 - ox0, y0 = pr.y0 - oy0;
            const uint32_t key = (uint32_t)pr.key;
            if (pr.kind == P_DASHED || pr.kind == P_SOLID) {
                const int b = pr.a;
                const bool dashed = pr.kind == P_DASHED;
                // the border pixels (u, v) of the square, u = x - x0, v = y - y0: rows v = 0, b-1; columns u = 0, b-1
                for (int e = 0; e < 4; ++e) {
                    const bool row = e < 2;
                    const int fixed = (e & 1) ? b - 1 : 0;
                    const int from = row ? 0 : 1, to = row ? b : b - 1;
                    int lo_t = from, hi_t = to;                   // clip the running coordinate to the tile
                    const int base = row ? x0 : y0;
                    lo_t = max(lo_t, -base);
                    hi_t = min(hi_t, RT - base);
                    const int yy_or_xx = (row ? y0 : x0) + fixed;
                    if (yy_or_xx < 0 || yy_or_xx >= RT) continue;
                    for (int s = lo_t; s < hi_t; ++s) {
                        if (dashed && (((s + fixed) >> 2) & 1)) continue;
                        const int xx = row ? x0 + s : yy_or_xx, yy = row ? yy_or_xx : y0 + s;
                        if (dashed) atomicMax(&over[yy * RT + xx], key);
                        else gt[yy * RT + xx] = 1;
                    }
                }
            } else if (pr.kind == P_GLYPH) {
                const int ch = pr.a, s = pr.b;
                if (ch < 0 || ch >= GLYPHS) continue;
                for (int gy = 0; gy < 7; ++gy) {
                    const int bits = glyph[ch * 7 + gy];
                    for (int gx = 0; gx < 5; ++gx) {
                        if (!((bits >> (4 - gx)) & 1)) continue;
                        for (int v = 0; v < s; ++v) {
                            const int yy = y0 + gy * s + v;
                            if (yy < 0 || yy >= RT) continue;
                            for (int u = 0; u < s; ++u) {
                                const int xx = x0 + gx * s + u;
                                if (xx >= 0 && xx < RT) atomicMax(&over[yy * RT + xx], key);
                            }
                        }
                    }
                }
            } else if (pr.kind == P_RECT) {
                const int ya = max(y0, 0), yb = min(y0 + pr.b, RT), xa = max(x0, 0), xb = min(x0 + pr.a, RT);
                for (int yy = ya; yy < yb; ++yy)
                    for (int xx = xa; xx < xb; ++xx) atomicMax(&over[yy * RT + xx], key);
            } else if (pr.kind == P_TARGET && pr.key == TGT_PATH) {
                const int ya = max(y0, 0), yb = min(y0 + pr.b, RT), xa = max(x0, 0), xb = min(x0 + pr.a, RT);
                for (int yy = ya; yy < yb; ++yy)
                    for (int xx = xa; xx < xb; ++xx) tgt[yy * RT + xx] = TGT_PATH;
            }
        }
        __syncthreads();                                      // (the paths are down: the target cells go over them)
        for (int j = q0 + tid; j < q1; j += NT) {
            if (a.prims[j].kind != P_TARGET || a.prims[j].key != TGT_CELL) continue;
            const Prim pr = a.prims[j];
            const int x0 = pr.x0 - ox0, y0 = pr.y0 - oy0;
            const int ya = max(y0, 0), yb = min(y0 + pr.b, RT), xa = max(x0, 0), xb = min(x0 + pr.a, RT);
            for (int yy = ya; yy < yb; ++yy)
                for (int xx = xa; xx < xb; ++xx) tgt[yy * RT + xx] = TGT_CELL;
        }
        const float *frame = a.frames + (long long)f * HW;
        const uint8_t *mask = a.mask ? a.mask + (long long)f * a.mask_stride : nullptr;
        if (a.bg) {
            // weight map of the window [fy0 - HALO, +BW) x [fx0 - HALO, +BW), in-frame entries only
            const int wy0 = fy0 - HALO, wx0 = fx0 - HALO;
            for (int k = tid; k < BW * BW; k += NT) {
                const int gy = wy0 + k / BW, gx = wx0 + k % BW;
                if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) continue;
                const int r = r8_of(frame[(long long)gy * a.W + gx]);
                bufA[k] = (r > 0 && r <= 30) ? 26 : 256;
            }
            __syncthreads();
            // three horizontal passes (A -> B -> A -> B) over columns [4p, BW - 4p), every row of the window
            for (int pass = 1; pass <= 3; ++pass) {
                const uint16_t *src = (pass & 1) ? bufA : bufB;
                uint16_t *dst = (pass & 1) ? bufB : bufA;
                const int w = BW - 8 * pass;
                for (int k = tid; k < BW * w; k += NT) {
                    const int ly = k / w, lx = 4 * pass + k % w;
                    const int gy = wy0 + ly, gx = wx0 + lx;
                    if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) continue;
                    int sum = 0;
#pragma unroll
                    for (int d = -4; d <= 4; ++d) sum += src[ly * BW + min(max(gx + d, 0), a.W - 1) - wx0];
                    dst[ly * BW + lx] = (uint16_t)((sum + 4) / 9);
                }
                __syncthreads();
            }
            // three vertical passes (B -> A -> B -> A) over rows [4p, BW - 4p), the tile's columns
            for (int pass = 1; pass <= 3; ++pass) {
                const uint16_t *src = (pass & 1) ? bufB : bufA;
                uint16_t *dst = (pass & 1) ? bufA : bufB;
                const int h = BW - 8 * pass;
                for (int k = tid; k < h * RT; k += NT) {
                    const int ly = 4 * pass + k / RT, lx = HALO + k % RT;
                    const int gy = wy0 + ly, gx = wx0 + lx;
                    if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) continue;
                    int sum = 0;
#pragma unroll
                    for (int d = -4; d <= 4; ++d) sum += src[(min(max(gy + d, 0), a.H - 1) - wy0) * BW + lx];
                    dst[ly * BW + lx] = (uint16_t)((sum + 4) / 9);
                }
                __syncthreads();
            }
        } else {
            __syncthreads();
        }
        // resolve: 16 pixels of one row per thread
        const int ly = tid >> 2, lx0 = (tid & 3) * 16;
        const int oy = oy0 + ly, ox = ox0 + lx0;
        if (oy < a.Ho && ox < a.Wo) {
            const int gy = fy0 + ly;
            uint32_t wds[12];
#pragma unroll
            for (int w = 0; w < 12; ++w) wds[w] = 0u;
            const int n = min(16, a.Wo - ox);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j < n) {
                    const int lx = lx0 + j, gx = fx0 + lx;
                    int r = r8_of(frame[(long long)gy * a.W + gx]), g = 0, b = 0;
                    if (a.bg) {
                        const int wt = bufA[(HALO + ly) * BW + HALO + lx];
                        const int m = (!mask || mask[(long long)gy * a.W + gx]) ? 255 : 0;
                        r = blend(wt, r, m);
                        g = b = blend(wt, 0, m);
                    }
                    if (a.grid && (gx % a.grid == 0 || gy % a.grid == 0)) {
                        r = blend(38, 255, r); g = blend(38, 255, g); b = blend(38, 255, b);
                    }
                    const int tg = tgt[ly * RT + lx];
                    if (tg) r = g = b = (tg == TGT_CELL) ? 255 : 217;
                    const uint32_t tk = trail[ly * RT + lx];
                    if (tk) {
                        const uint8_t *c = pal + 3 * a.trail_col[tk];
                        r = c[0]; g = c[1]; b = c[2];
                    }
                    if (gt[ly * RT + lx]) {
                        r = blend(154, 255, r); g = blend(154, 255, g); b = blend(154, 255, b);
                    }
                    const uint32_t ok = over[ly * RT + lx];
                    if (ok >> 24 == 3u) {
                        r = g = b = 107;
                    } else if (ok) {
                        const uint8_t *c = pal + 3 * (int)(((ok & 0xFFFFFFu) - 1u) % 20u);
                        r = c[0]; g = c[1]; b = c[2];
                    }
                    wds[(3 * j) >> 2] |= (uint32_t)r << (8 * ((3 * j) & 3));
                    wds[(3 * j + 1) >> 2] |= (uint32_t)g << (8 * ((3 * j + 1) & 3));
                    wds[(3 * j + 2) >> 2] |= (uint32_t)b << (8 * ((3 * j + 2) & 3));
                }
            }
            uint8_t *dst = a.out + (((long long)i * a.Ho + oy) * a.Wo + ox) * 3;
            if (n == 16 && ((uintptr_t)dst & 15) == 0) {
                uint4 *d4 = reinterpret_cast<uint4 *>(dst);
                d4[0] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
                d4[1] = make_uint4(wds[4], wds[5], wds[6], wds[7]);
                d4[2] = make_uint4(wds[8], wds[9], wds[10], wds[11]);
            } else {
#pragma unroll
                for (int k = 0; k < 48; ++k)
                    if (k < 3 * n) dst[k] = (uint8_t)(wds[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}
}  // namespace

extern "C" int axt_render_tile_size(void) { return RT; }

extern "C" int axt_render_frames(const float *d_frames, const uint8_t *d_mask, int64_t mask_stride, const int32_t *d_ts,
                                 int n_out, int H, int W, int ymin, int xmin, int Ho, int Wo, int grid, int bg,
                                 const int32_t *d_trail_ptr, const int32_t *d_trail, const uint8_t *d_trail_col,
                                 const int32_t *d_prim_ptr, const int32_t *d_prims, const uint8_t *d_tables, uint8_t *d_out,
                                 void *stream)
{
    AXT_REQUIRE(d_frames && d_ts && d_trail_ptr && d_trail_col && d_prim_ptr && d_tables && d_out,
                "axt_render_frames: null pointer");
    AXT_REQUIRE(H > 0 && W > 0 && Ho > 0 && Wo > 0 && ymin >= 0 && xmin >= 0 && Ho <= H && Wo <= W && ymin <= H - Ho && xmin <= W - Wo,
                "axt_render_frames: slice of %d x %d from (%d, %d) outside the %d x %d frame", Ho, Wo, ymin, xmin, H, W);
    AXT_REQUIRE((long)H * W <= 0x7fffffffL, "axt_render_frames: a frame of %d x %d pixels exceeds 2^31 - 1", H, W);
    AXT_REQUIRE(grid >= 0 && mask_stride >= 0, "axt_render_frames: grid and mask_stride must be >= 0");
    AXT_REQUIRE(n_out >= 0, "axt_render_frames: n_out %d is negative", n_out);
    // prim_ptr is indexed by output frame x tile in int, and one launch takes every (run of frames, tile) as a workgroup
    AXT_REQUIRE((long)n_out * axt_cdiv(Wo, RT) * axt_cdiv(Ho, RT) < 0x7fffffffL,
                "axt_render_frames: %d output frames x %d tiles exceed 2^31 - 2", n_out, axt_cdiv(Wo, RT) * axt_cdiv(Ho, RT));
    if (n_out == 0) return AXT_OK;
    RenderArgs a;
    a.frames = d_frames; a.mask = d_mask; a.mask_stride = mask_stride; a.ts = d_ts;
    a.n_out = n_out; a.H = H; a.W = W; a.ymin = ymin; a.xmin = xmin; a.Ho = Ho; a.Wo = Wo;
    a.ntx = axt_cdiv(Wo, RT); a.nty = axt_cdiv(Ho, RT);
    a.grid = grid; a.bg = bg ? 1 : 0;
    a.trail_ptr = d_trail_ptr; a.trail = d_trail; a.trail_col = d_trail_col;
    a.prim_ptr = d_prim_ptr; a.prims = reinterpret_cast<const Prim *>(d_prims); a.tables = d_tables; a.out = d_out;
    // runs of frames: about 512 workgroups (two per CU), so that each re-splats the trail history of its tile rarely
    const int ntiles = a.ntx * a.nty;
    const int runs = std::max(1, std::min(n_out, 512 / ntiles));
    a.chunk = axt_cdiv(n_out, runs);
    const int blocks = ntiles * axt_cdiv(n_out, a.chunk);
    hipLaunchKernelGGL(render_tiles, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, a);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
