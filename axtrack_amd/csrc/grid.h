// The masked grid (axt_grid) and the conventions every search on it shares. Internal; include after axt_common.h.
//
// Cost convention. Path lengths on a masked grid: weights {1 on mask, 65536 off} (reference AxonDetections.py:598), the
// A* of utils.py:379 (pyastar2d, absent from the reference tree -- convention in DESIGN.md). On the whole grid, find the
// minimum-cost 4-/8-connected path to each target, cost of a move = weight of the cell moved into. With weights
// {1, 65536} and fewer than 65536 on-mask moves the cost order equals the lexicographic order of
// (off-mask cells entered, moves), packed as a key:
//   64 bits, off << 32 | moves: the whole-grid searches (moves can exceed 16 bits in a 1001^2 window);
//   32 bits, off << 16 | moves: the searches confined to a window of fewer than 65536 cells.
// A path has moves + 1 cells. Where several paths are equally cheap the one returned is fixed by the neighbour order
// below: a walk back steps to the FIRST neighbour in that order that continues an optimal path.
#pragma once

typedef unsigned long long axt_u64;
constexpr axt_u64 AXT_KEY64_INF = ~0ull, AXT_KEY64_OFF = 1ull << 32, AXT_KEY64_MOVES = 0xffffffffull;
constexpr unsigned int AXT_KEY32_INF = 0xffffffffu, AXT_KEY32_OFF = 1u << 16, AXT_KEY32_MOVES = 0xffffu;

// The neighbour order: up, down, left, right, then the diagonals. The first 4 entries are the 4-connected grid. The
// order is part of the results (see above), and of the bit numbering of the tile worklists' `dirs` (tile_worklist.h).
constexpr int AXT_NB_DY[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
constexpr int AXT_NB_DX[8] = {0, 0, -1, 1, -1, 1, -1, 1};

// The first neighbour (ny, nx) of (cy, cx) in that order, among the first nn, that lies inside [0, h) x [0, w) and
// satisfies ok(ny, nx): its index in the order, or -1.
template <typename Pred>
__host__ __device__ __forceinline__ int axt_first_neighbour(int cy, int cx, int h, int w, int nn, Pred ok)
{
    for (int q = 0; q < nn; ++q) {
        const int ny = cy + AXT_NB_DY[q], nx = cx + AXT_NB_DX[q];
        if (ny < 0 || ny >= h || nx < 0 || nx >= w) continue;
        if (ok(ny, nx)) return q;
    }
    return -1;
}

struct axt_grid {
    int H = 0, W = 0, Ww = 0, conn8 = 0;
    unsigned char *d_mask = nullptr;     // [H][W] 0/1
    unsigned int *d_bits = nullptr;      // [H][Ww] bit x%32 of word x/32, zero-padded
    int *d_label = nullptr;              // [H][W] connected-component label >= 1 on the mask, 0 off it
    // [n_comp][H][W] u8: fewest off-mask cells any path from component `label` has to enter to reach the cell (the
    // cell itself included when it is off the mask), saturated at 255; NULL when the mask has too many components
    unsigned char *d_off = nullptr;
    int n_comp = 0;
    bool has_fields = false;             // d_off covers every component (trivially so for an empty mask)
    // [n_comp][4 or 8][H][Ww] bit rows: bit x of row y of direction d is set iff stepping INTO (y,x) from its
    // neighbour (y+AXT_NB_DY[d], x+AXT_NB_DX[d]) keeps the off-cell count minimal:
    // d_off[A][(y,x)] == d_off[A][neighbour] + [cell off]
    unsigned int *d_tight = nullptr;
};

// grid == NULL stands for the all-ones mask: no mask array, every cell on the mask
static inline const uint8_t *axt_grid_mask(const axt_grid *g) { return g ? g->d_mask : nullptr; }

// exclusive prefix sum of value(in[k]) over k < n into out[0..n] (out[n] = the total); one workgroup of 1024 threads
template <typename T, typename F>
__global__ __launch_bounds__(1024) void axt_scan_kernel(const int *__restrict__ in, long n, T *__restrict__ out, F value)
{
    __shared__ T s_part[1024];
    const int tid = threadIdx.x;
    const long per = (n + 1023) / 1024;
    const long a = min(n, tid * per), b = min(n, a + per);
    T sum = 0;
    for (long k = a; k < b; ++k) sum += value(in[k]);
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        T run = 0;
        for (int k = 0; k < 1024; ++k) { const T v = s_part[k]; s_part[k] = run; run += v; }
        out[n] = run;
    }
    __syncthreads();
    T run = s_part[tid];
    for (long k = a; k < b; ++k) {
        out[k] = run;
        run += value(in[k]);
    }
}

// ---- the internal functions one file defines and another calls (their only prototypes)
// path_bfs.hip: the exact whole-grid search, every source against every target (D [na, nb]; d_cells, when given,
// [na, nb, max_dist]) ...
int axt_path_cost_masked(const int32_t *d_xa, const int32_t *d_ya, int na, const int32_t *d_xb, const int32_t *d_yb,
                         int nb, const uint8_t *d_mask, int H, int W, int max_dist, int conn8, int32_t *d_D,
                         hipStream_t st, int32_t *d_cells);
// ... and for a list of (source, target) pairs (D [n], cells [n, max_dist])
int axt_path_cells_pairs(const int32_t *d_xa, const int32_t *d_ya, const int32_t *d_xb, const int32_t *d_yb, int n,
                         const uint8_t *d_mask, int H, int W, int max_dist, int conn8, int32_t *d_D, int32_t *d_cells,
                         hipStream_t st);
// path_bfs.hip: the arc builder's path-length table of every source detection
int axt_masked_distance_table(const axt_grid *g, const int32_t *d_x, const int32_t *d_y, const int32_t *d_count,
                              const int32_t *d_src_count, int n_frames, int cap, int max_dist, int max_gap,
                              const int32_t *h_dmax, const int32_t *d_dmax, int16_t *d_Dtmp, hipStream_t st);
// assoc.hip: d_off[0..n_frames] = exclusive prefix sum of min(count, cap)
int axt_frame_offsets(const int32_t *d_count, int n_frames, int cap, int32_t *d_off, hipStream_t st);
