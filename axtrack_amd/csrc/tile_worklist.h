// The round protocol of the tiled searches (target.hip, segment.hip). Internal; include after axt_common.h and grid.h.
//
// A round is one launch over the worklist of marked tiles, one workgroup per tile of the grid; those beyond the
// worklist's end leave at once. The marks of round r are the worklist of round r + 1. Device state, all i32:
//   ctrl  [4]           [0..2] worklist counters in rotation (round r reads r % 3, fills (r + 1) % 3 and resets
//                       (r + 2) % 3, so no launch resets the counter it reads), [3] rounds that had work;
//   flags [2][n_tiles]  by round parity: the tile is in that round's worklist already (a tile enters once);
//   lists [2][n_tiles]  by round parity: the worklist.
// The caller's init / seed kernels zero ctrl and flags and write the worklist of round 0 (lists[0], ctrl[0]).
// No grid-wide barrier, no spinning, no cooperative launch.
#pragma once

// Head of a round, called by every thread of the workgroup: the tile of workgroup blockIdx.x in this round, or -1 when
// it has none (the workgroup leaves).
__device__ __forceinline__ int axt_worklist_take(int round, int n_tiles, int *__restrict__ ctrl, int *__restrict__ flags,
                                                 const int *__restrict__ lists)
{
    const int par = round & 1;
    const int n_cur = min(ctrl[round % 3], n_tiles);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctrl[(round + 2) % 3] = 0;                    // (nobody reads or writes that counter in this round)
        if (n_cur > 0) ctrl[3] += 1;                  // (launches of a stream run one after the other)
    }
    if ((int)blockIdx.x >= n_cur) return -1;
    const int t = lists[par * n_tiles + blockIdx.x];
    if (t < 0 || t >= n_tiles) return -1;
    if (threadIdx.x == 0) flags[par * n_tiles + t] = 0;
    return t;
}

// Tail of a round, called by (at least) threads 0..7 after a __threadfence() behind the tile's writes: thread q marks
// the neighbour tile of t in direction q of the neighbour order (grid.h) if bit q of dirs is set, and enlists it for
// the next round unless it is listed already.
__device__ __forceinline__ void axt_worklist_mark(int dirs, int t, int tiles_x, int tiles_y, int round, int *__restrict__ ctrl,
                                                  int *__restrict__ flags, int *__restrict__ lists)
{
    const int q = threadIdx.x, n_tiles = tiles_x * tiles_y, par = round & 1;
    if (q >= 8 || !(dirs >> q & 1)) return;
    const int ny = t / tiles_x + AXT_NB_DY[q], nx = t % tiles_x + AXT_NB_DX[q];
    if (ny < 0 || ny >= tiles_y || nx < 0 || nx >= tiles_x) return;
    const int nt = ny * tiles_x + nx;
    if (atomicExch(&flags[(par ^ 1) * n_tiles + nt], 1) == 0) {
        const int k = atomicAdd(&ctrl[(round + 1) % 3], 1);      // (< n_tiles: a tile enters a worklist once)
        if (k < n_tiles) lists[(par ^ 1) * n_tiles + k] = nt;
    }
}

// The host loop: launch_round(r) launches round r (it gets r % 6: the kernels need r % 2 and r % 3) on stream st.
// Every round with work lets some optimal path cross one more tile border, a path is simple and every crossing enters
// a tile through one of its 4 * tile_edge - 4 border cells: at most n_tiles * 4 * tile_edge rounds can do work, and the
// loop stops at that bound with an error instead of going on. It reads ctrl back every CHECK_EVERY rounds. Launch errors
// of the caller's init kernels, still pending, are reported here too. *n_rounds = the rounds that had work.
constexpr int AXT_WORKLIST_CHECK_EVERY = 16;

template <typename Launch>
static int axt_worklist_run(const char *who, Launch launch_round, const int *d_ctrl, long n_tiles, int tile_edge, hipStream_t st,
                            int *n_rounds)
{
    hipError_t e = hipGetLastError();
    const long max_rounds = n_tiles * 4 * tile_edge + 2;
    int h_ctrl[4] = {0, 0, 0, 0};
    bool done = false;
    long round = 0;
    while (e == hipSuccess && !done && round < max_rounds) {
        for (int k = 0; k < AXT_WORKLIST_CHECK_EVERY; ++k, ++round) launch_round((int)(round % 6));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_ctrl, d_ctrl, sizeof(h_ctrl), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        done = h_ctrl[round % 3] == 0;                       // the worklist of the round that would come next
    }
    *n_rounds = h_ctrl[3];
    if (e != hipSuccess) {
        axt_set_error("%s: %s", who, hipGetErrorString(e));
        return AXT_EHIP;
    }
    if (!done) {
        axt_set_error("%s: no fixed point after %ld rounds (bound for %d tiles)", who, max_rounds, (int)n_tiles);
        return AXT_ERUNTIME;
    }
    return AXT_OK;
}
