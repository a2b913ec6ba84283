// Target screens on gfx950: the distance of every grid cell to a set of target cells, measured through the structure.
//
// The reference's drawing code reads a "StructureScreen" it never shipped (video_plotting.py:170-177,308-309:
// get_trg_path(t, ymin, ymax) and structure_outputchannel_coo): how far is a growth cone from the output channel of the
// microstructure, along the structure? That is one field over the whole grid per mask, from which every detection of
// every frame reads its distance -- the opposite shape of path_bfs.hip / recon.hip, which answer pair questions inside
// the 500-cell association gate with one workgroup per source.
//
// Definition (the package's path convention, grid.h): weights {1 on mask, 65536 off}, a move costs the weight of
// the cell moved INTO, 4- or 8-connected (a diagonal move counts 1). Minimum cost is the lexicographic order of
// (off-mask cells entered, moves), packed as the 64-bit key off << 32 | moves. For target cells T, key(c) is the
// minimum over all paths from c to any cell of T (the cells entered after c count, the target cell included); key = 0
// on T. In the reverse direction the cell being LEFT is the one paid for: key(v) <= key(u) + w(u) for neighbours u, v
// with w(u) = (mask[u] ? 0 : 1) << 32 | 1. Off-mask cells are passable, so every cell has a finite key.
//
// axt_target_field: tiled label-correcting search.
//   * The grid is cut into TS x TS tiles (TS = 32). A workgroup (256 threads, 4 cells each) loads one tile and its
//     one-cell halo -- 34 x 34 keys of 8 bytes and one weight byte each, 10.4 KB of LDS -- and relaxes the tile's cells in
//     place (pull: key(v) = min over neighbours u of key(u) + w(u); one writer per cell, keys only decrease) until a
//     sweep changes nothing: the tile's fixed point for the halo it read. It writes back the cells it improved and, for
//     every border (corner) whose cells improved, marks the neighbour tile that has them in its halo.
//   * Rounds, worklists, per-tile flags and the three counters in rotation: tile_worklist.h. Every loop in the kernel
//     is bounded.
//   * Within a round a workgroup may read a neighbour's border cell before or after that neighbour improves it: either
//     value is the cost of a real path (an upper bound), 8-byte keys are read and written whole, and the neighbour marks
//     this tile whenever its border changed, whatever this tile saw. So when a round marks nothing every tile has been
//     relaxed against the final values of its halo: the keys satisfy key(v) = min_u key(u) + w(u) with positive
//     weights and key = 0 on T, whose only solution reached from above is the shortest-path key. The result does not
//     depend on scheduling: byte-identical from run to run.
//   * After round k every cell whose optimal path crosses at most k tile borders is final, so the number of rounds
//     grows with the tiles a path crosses, not with its cells (the bound at which the host stops: tile_worklist.h).
//   * Sweeps per tile visit: every sweep finalises at least one more cell of the tile, so TS * TS + 1 bounds them.
// axt_target_sample: (off, moves) of every detection slot; -1 for empty slots and detections outside the grid (the
//   decode does not clamp). A per-frame field index serves time-varying masks (one field per distinct mask).
// axt_target_paths: the target path of a detection starts at its cell and steps to the first neighbour n (up, down,
//   left, right, then the diagonals: grid.h's order) with key(c) == key(n) + w(n); it has moves + 1 cells and
//   ends in T. CSR like axt_link_cells: cell_ptr = scan of moves + 1 (no count pass), one thread per detection.
#include "axt_common.h"
#include "grid.h"
#include "tile_worklist.h"

namespace {

typedef axt_u64 u64;

constexpr int TS = 32;                       // tile edge
constexpr int TH = TS + 2;                   // with the halo
constexpr int NT = 256;                      // threads per workgroup
constexpr int CPT = TS * TS / NT;            // cells per thread
constexpr u64 KEY_INF = AXT_KEY64_INF;
constexpr u64 W_ON = 1ull, W_OFF = AXT_KEY64_OFF | 1ull;

// a key is read and written whole (one 8-byte LDS access) while other threads of the workgroup relax their cells
__device__ __forceinline__ u64 lds_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ctrl, flags, lists: the worklist state of tile_worklist.h
__global__ __launch_bounds__(256) void field_init_kernel(u64 *__restrict__ key, long n, int *__restrict__ ctrl,
                                                         int *__restrict__ flags, int n_tiles)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) key[i] = KEY_INF;
    if (i < 2L * n_tiles) flags[i] = 0;
    if (i < 4) ctrl[i] = 0;
}

__global__ __launch_bounds__(256) void field_seed_kernel(const int *__restrict__ targets, int n_targets, int H, int W, int tiles_x,
                                                         u64 *__restrict__ key, int *__restrict__ ctrl, int *__restrict__ flags,
                                                         int *__restrict__ list)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_targets) return;
    const int c = targets[i];
    if (c < 0 || (long)c >= (long)H * W) return;
    key[c] = 0;
    const int t = (c / W / TS) * tiles_x + (c % W) / TS;
    if (atomicExch(&flags[t], 1) == 0) {              // (flags of parity 0: the worklist of round 0)
        const int k = atomicAdd(&ctrl[0], 1);
        if (k < tiles_x * ((H + TS - 1) / TS)) list[k] = t;
    }
}

// One round: workgroup b relaxes tile list_cur[b] (see the top). flags [2][n_tiles], lists [2][n_tiles].
__global__ __launch_bounds__(NT) void field_round_kernel(const unsigned char *__restrict__ mask, int H, int W, int tiles_x,
                                                         int tiles_y, int conn8, int round, u64 *__restrict__ key,
                                                         int *__restrict__ ctrl, int *__restrict__ flags, int *__restrict__ lists)
{
    __shared__ u64 s_key[TH * TH];
    __shared__ unsigned char s_off[TH * TH];          // 1 = the cell is off the mask
    __shared__ int s_dirs;
    const int tid = threadIdx.x;
    const int t = axt_worklist_take(round, tiles_x * tiles_y, ctrl, flags, lists);
    if (t < 0) return;
    const int ty0 = (t / tiles_x) * TS, tx0 = (t % tiles_x) * TS;
    if (tid == 0) s_dirs = 0;
    for (int e = tid; e < TH * TH; e += NT) {
        const int r = e / TH, c = e - r * TH;
        const int gy = ty0 - 1 + r, gx = tx0 - 1 + c;
        u64 k = KEY_INF;
        unsigned char off = 1;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long g = (long)gy * W + gx;
            k = __hip_atomic_load(&key[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            off = (mask == nullptr || mask[g] == 1) ? 0 : 1;
        }
        s_key[e] = k;
        s_off[e] = off;
    }
    __syncthreads();
    const int nn = conn8 ? 8 : 4;
    int pos[CPT];
    u64 first[CPT];
    for (int q = 0; q < CPT; ++q) {
        const int e = tid + q * NT, r = e / TS, c = e - r * TS;
        const bool in = ty0 + r < H && tx0 + c < W;
        pos[q] = in ? (r + 1) * TH + (c + 1) : -1;
        first[q] = in ? s_key[(r + 1) * TH + (c + 1)] : 0;
    }
    for (int sweep = 0; sweep <= TS * TS; ++sweep) {
        int changed = 0;
        for (int q = 0; q < CPT; ++q) {
            const int p = pos[q];
            if (p < 0) continue;
            const u64 mine = lds_load(&s_key[p]);
            u64 best = mine;
            for (int d = 0; d < nn; ++d) {
                const int pn = p + AXT_NB_DY[d] * TH + AXT_NB_DX[d];
                const u64 kn = lds_load(&s_key[pn]);
                if (kn == KEY_INF) continue;
                const u64 cand = kn + (s_off[pn] ? W_OFF : W_ON);
                if (cand < best) best = cand;
            }
            if (best < mine) { lds_store(&s_key[p], best); changed = 1; }      // (one writer per cell; keys only decrease)
        }
        if (!__syncthreads_or(changed)) break;
    }
    int dirs = 0;
    for (int q = 0; q < CPT; ++q) {
        const int p = pos[q];
        if (p < 0) continue;
        const u64 k = s_key[p];
        if (k >= first[q]) continue;
        const int e = tid + q * NT, r = e / TS, c = e - r * TS;
        __hip_atomic_store(&key[(long)(ty0 + r) * W + (tx0 + c)], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool up = r == 0, down = r == TS - 1, left = c == 0, right = c == TS - 1;
        dirs |= (up ? 1 : 0) | (down ? 2 : 0) | (left ? 4 : 0) | (right ? 8 : 0);
        if (conn8) dirs |= (up && left ? 16 : 0) | (up && right ? 32 : 0) | (down && left ? 64 : 0) | (down && right ? 128 : 0);
    }
    if (dirs) atomicOr(&s_dirs, dirs);
    __threadfence();                                  // the keys before the marks
    __syncthreads();
    axt_worklist_mark(s_dirs, t, tiles_x, tiles_y, round, ctrl, flags, lists);
}

__global__ __launch_bounds__(256) void field_unpack_kernel(const u64 *__restrict__ key, long n, int *__restrict__ off,
                                                           int *__restrict__ moves)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    off[i] = k == KEY_INF ? -1 : (int)(k >> 32);
    moves[i] = k == KEY_INF ? -1 : (int)(k & 0xffffffffull);
}

__global__ __launch_bounds__(256) void sample_kernel(const int *__restrict__ off, const int *__restrict__ moves, int n_fields,
                                                     const int *__restrict__ field_index, int H, int W, const int *__restrict__ x,
                                                     const int *__restrict__ y, const int *__restrict__ count, int n_frames,
                                                     int cap, int *__restrict__ det_off, int *__restrict__ det_moves)
{
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= (long)n_frames * cap) return;
    const int f = (int)(s / cap), i = (int)(s - (long)f * cap);
    int o = -1, m = -1;
    const int fi = field_index ? field_index[f] : 0;
    if (i < count[f] && fi >= 0 && fi < n_fields) {
        const int cx = x[s], cy = y[s];
        if (cx >= 0 && cx < W && cy >= 0 && cy < H) {
            const long c = (long)fi * H * W + (long)cy * W + cx;
            o = off[c];
            m = moves[c];
        }
    }
    det_off[s] = o;
    det_moves[s] = m;
}

// the cells of a detection's target path: moves + 1, none where moves < 0 (cell_ptr = their exclusive prefix sum)
struct PathCells {
    __device__ int operator()(int moves) const { return moves < 0 ? 0 : moves + 1; }
};

// one thread per detection slot: the walk over the field (see the top); a step that finds no neighbour -- impossible
// on a field of axt_target_field for this mask -- leaves -1 in the rest of the path
__global__ __launch_bounds__(64) void path_walk_kernel(const unsigned char *__restrict__ mask, const int *__restrict__ off,
                                                       const int *__restrict__ moves, int H, int W, int conn8,
                                                       const int *__restrict__ x, const int *__restrict__ y, long n_slots, int cap,
                                                       const int *__restrict__ det_moves, const int *__restrict__ field_index,
                                                       int group, const long long *__restrict__ cell_ptr, long long n_cells,
                                                       int *__restrict__ cells)
{
    const long s = (long)blockIdx.x * 64 + threadIdx.x;
    if (s >= n_slots) return;
    const int m0 = det_moves[s];
    if (m0 < 0) return;
    if (field_index && field_index[s / cap] != group) return;
    const long long p = cell_ptr[s];
    if (p < 0 || p + m0 + 1 > n_cells) return;
    int cx = x[s], cy = y[s];
    if (cx < 0 || cx >= W || cy < 0 || cy >= H) return;
    const int nn = conn8 ? 8 : 4;
    for (int k = 0; k <= m0; ++k) {
        const long c = (long)cy * W + cx;
        cells[p + k] = (int)c;
        if (k == m0) break;
        const int oc = off[c], mc = moves[c];
        const int found = axt_first_neighbour(cy, cx, H, W, nn, [=](int ny, int nx) {
            const long g = (long)ny * W + nx;
            const int wn = (mask == nullptr || mask[g] == 1) ? 0 : 1;
            return off[g] + wn == oc && moves[g] + 1 == mc;
        });
        if (found < 0) {
            for (int r = k + 1; r <= m0; ++r) cells[p + r] = -1;
            break;
        }
        cy += AXT_NB_DY[found];
        cx += AXT_NB_DX[found];
    }
}

int grid_matches(const axt_grid *grid, int H, int W) { return !grid || (grid->H == H && grid->W == W); }

}  // namespace

extern "C" int axt_target_tile_size(void) { return TS; }

extern "C" int axt_target_field(const axt_grid *grid, int H, int W, int conn8, const int32_t *d_target_cells, int n_targets,
                                int32_t *d_off, int32_t *d_moves, int *n_rounds, void *stream)
{
    AXT_REQUIRE(H > 0 && W > 0 && (long)H * W <= 0x7fffffffL, "axt_target_field: bad grid size %d x %d", H, W);
    AXT_REQUIRE(n_targets >= 1, "axt_target_field: needs at least one target cell");
    AXT_REQUIRE(d_target_cells && d_off && d_moves, "axt_target_field: null argument");
    AXT_REQUIRE(grid_matches(grid, H, W), "axt_target_field: the grid is not %d x %d", H, W);
    hipStream_t st = (hipStream_t)stream;
    const unsigned char *mask = axt_grid_mask(grid);
    const long n = (long)H * W;
    const int tiles_x = axt_cdiv(W, TS), tiles_y = axt_cdiv(H, TS);
    const long n_tiles_l = (long)tiles_x * tiles_y;
    const int n_tiles = (int)n_tiles_l;
    // scratch: keys u64 [H*W], then i32: ctrl [4], flags [2][n_tiles], lists [2][n_tiles]
    const size_t key_bytes = sizeof(u64) * (size_t)n;
    AxtScratch raw(st, key_bytes + sizeof(int) * (4 + 4 * (size_t)n_tiles));
    AXT_CHECK_HIP(raw.err);
    u64 *key = raw.as<u64>();
    int *ctrl = reinterpret_cast<int *>(raw.as<unsigned char>() + key_bytes);
    int *flags = ctrl + 4, *lists = flags + 2 * (size_t)n_tiles;
    const unsigned nb = (unsigned)((n + 255) / 256);
    long n_init = n > 2 * n_tiles_l ? n : 2 * n_tiles_l;      // (a tiny grid has fewer cells than flags or counters)
    if (n_init < 4) n_init = 4;
    const unsigned nb_init = (unsigned)((n_init + 255) / 256);
    hipLaunchKernelGGL(field_init_kernel, dim3(nb_init), dim3(256), 0, st, key, n, ctrl, flags, n_tiles);
    hipLaunchKernelGGL(field_seed_kernel, dim3((unsigned)((n_targets + 255) / 256)), dim3(256), 0, st, d_target_cells, n_targets,
                       H, W, tiles_x, key, ctrl, flags, lists);
    int rounds = 0;
    int rc = axt_worklist_run("axt_target_field", [&](int r) {
        hipLaunchKernelGGL(field_round_kernel, dim3(n_tiles), dim3(NT), 0, st, mask, H, W, tiles_x, tiles_y, conn8 ? 1 : 0, r, key,
                           ctrl, flags, lists);
    }, ctrl, n_tiles_l, TS, st, &rounds);
    if (rc == AXT_OK) {
        hipLaunchKernelGGL(field_unpack_kernel, dim3(nb), dim3(256), 0, st, (const u64 *)key, n, d_off, d_moves);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { axt_set_error("axt_target_field: %s", hipGetErrorString(e)); rc = AXT_EHIP; }
    }
    if (n_rounds) *n_rounds = rc == AXT_OK ? rounds : 0;
    return rc;
}

extern "C" int axt_target_sample(const int32_t *d_off, const int32_t *d_moves, int n_fields, const int32_t *d_field_index, int H,
                                 int W, const int32_t *d_x, const int32_t *d_y, const int32_t *d_count, int n_frames, int cap,
                                 int32_t *d_det_off, int32_t *d_det_moves, void *stream)
{
    AXT_REQUIRE(H > 0 && W > 0 && (long)H * W <= 0x7fffffffL && n_fields >= 1 && n_frames >= 0 && cap >= 1,
                "axt_target_sample: bad argument (grid %d x %d, %d fields, %d frames, cap %d)", H, W, n_fields, n_frames, cap);
    AXT_REQUIRE((long)n_frames * cap <= 0x7fffffffL, "axt_target_sample: n_frames %d x cap %d exceeds 2^31 - 1 slots", n_frames, cap);
    if (n_frames == 0) return AXT_OK;
    AXT_REQUIRE(d_off && d_moves && d_x && d_y && d_count && d_det_off && d_det_moves, "axt_target_sample: null argument");
    AXT_REQUIRE(n_fields == 1 || d_field_index, "axt_target_sample: %d fields need a field index per frame", n_fields);
    const long slots = (long)n_frames * cap;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_off, d_moves,
                       n_fields, d_field_index, H, W, d_x, d_y, d_count, n_frames, cap, d_det_off, d_det_moves);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

extern "C" int axt_target_paths(const axt_grid *grid, const int32_t *d_off, const int32_t *d_moves, int H, int W, int conn8,
                                const int32_t *d_x, const int32_t *d_y, int n_frames, int cap, const int32_t *d_det_moves,
                                const int32_t *d_field_index, int group, int64_t *d_cell_ptr, int32_t *d_cells,
                                int64_t *n_cells, void *stream)
{
    AXT_REQUIRE(H > 0 && W > 0 && (long)H * W <= 0x7fffffffL && n_frames >= 0 && cap >= 1,
                "axt_target_paths: bad argument (grid %d x %d, %d frames, cap %d)", H, W, n_frames, cap);
    AXT_REQUIRE((long)n_frames * cap <= 0x7fffffffL, "axt_target_paths: n_frames %d x cap %d exceeds 2^31 - 1 slots", n_frames, cap);
    AXT_REQUIRE(d_cell_ptr && n_cells, "axt_target_paths: null argument");
    AXT_REQUIRE(n_frames == 0 || d_det_moves, "axt_target_paths: null argument");
    hipStream_t st = (hipStream_t)stream;
    const long slots = (long)n_frames * cap;
    if (!d_cells) {
        hipLaunchKernelGGL((axt_scan_kernel<long long, PathCells>), dim3(1), dim3(1024), 0, st, d_det_moves, slots, (long long *)d_cell_ptr,
                           PathCells{});
        AXT_LAUNCH_CHECK();
        long long total = 0;
        AXT_CHECK_HIP(hipMemcpyAsync(&total, d_cell_ptr + slots, sizeof(total), hipMemcpyDeviceToHost, st));
        AXT_CHECK_HIP(hipStreamSynchronize(st));
        *n_cells = total;
        return AXT_OK;
    }
    AXT_REQUIRE(*n_cells >= 0, "axt_target_paths: bad cell count");
    if (slots == 0 || *n_cells == 0) return AXT_OK;
    AXT_REQUIRE(d_off && d_moves && d_x && d_y, "axt_target_paths: null argument");
    AXT_REQUIRE(grid_matches(grid, H, W), "axt_target_paths: the grid is not %d x %d", H, W);
    hipLaunchKernelGGL(path_walk_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, st, axt_grid_mask(grid), d_off, d_moves,
                       H, W, conn8 ? 1 : 0, d_x, d_y, slots, cap, d_det_moves, d_field_index, group,
                       (const long long *)d_cell_ptr, (long long)*n_cells, d_cells);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
