// Axon reconstructions on gfx950: the links of the tracks and one minimum-cost path per link.
//
// The reference names the API and never built it (AxonDetections._reconstruct_axons / get_axon_reconstructions,
// AxonDetections.py:924-934, read by video_plotting.py:164-168,301-304 as "the A* paths between associated
// detections"). A reconstruction needs only the links the tracker chose -- about one per detection -- not the paths of
// every (t_bef, t) pair that astar_dets_paths() materialises.
//
// axt_track_links: from the track table alone (i32 [F, cap], -1 = none), so that the flow tracker, the frame-to-frame
// variant and identities adopted from a cache are served alike. Slot (f, i) with id k links to the first detection of
// k in frames f+1 .. f+max_gap (ids never repeat within a frame). One workgroup per frame finds the heads, one scan
// over the per-frame counts, one ordered compaction per frame: links come out in ascending tail order, no atomics.
//
// axt_link_paths: the cells of each link's path, the SAME cells in the same order as the package returns for that pair:
//   * all-ones mask (grid == NULL): the closed-form staircase of AxonDetections._open_dets_paths -- 4-connected:
//     columns first, then rows; 8-connected: the diagonal first, then straight. One thread per link.
//   * masked grid: what axt_path_cells gives (path_bfs.hip): key order (off-mask cells entered, moves), then the walk
//     back from the target, at each step to the first neighbour (up, down, left, right, diagonals) whose key is the
//     current key minus the current cell's weight. Here:
//       - A path of L cells stays within Chebyshev radius L-1 of its source, so a breadth-first search confined to the
//         window of radius R around the source finds every cell's exact BFS distance up to R.
//       - If the target is on the mask and reachable over on-mask cells, the optimum enters 0 off-mask cells (the
//         source is never entered, so an off-mask source is fine) and its key is (0, BFS distance over the mask).
//       - The cells with key (0, m) are exactly the on-mask cells at on-mask BFS distance m, and the source (m = 0):
//         any other cell enters at least one off-mask cell. So the walk back over the BFS distance field, with the
//         same neighbour order, picks the same neighbour at every step as the walk over the keys.
//     One workgroup per link keeps the window's u16 distance field in LDS (pull BFS, layer by layer, stopping at the
//     layer that reaches the target) in two buckets: radius 31 (8 KB) for the short steps that are almost all links,
//     then radius 127 (127 KB) for the rest. A target in the same component as an on-mask source that is not reached
//     within max_dist-2 moves has no path (D = max_dist): key order puts on-mask paths first.
//   * Links the breadth-first windows cannot decide (a target off the mask, a target in another component than an
//     on-mask source, a target not reached within the largest window) first try the keys themselves in a window
//     (radius 31, then 63; u32 key off << 16 | moves in LDS, label-correcting sweeps to the fixed point). The window
//     optimum (o, m) is the grid's optimum when m <= R and o equals a lower bound of the off-mask cells of EVERY path:
//     d_off[A][T] of the grid's component fields for a source in component A; for an off-mask source the smaller of
//     min_A (d_off[A][S] - 1 + d_off[A][T]) (paths that first touch the mask in A) and the 4-/8-metric distance S->T
//     (paths that do not touch it: every cell they enter is off the mask). A path that leaves the window has more than R moves, so none beats (o, m). Every
//     cell the walk back tests for equality with the wanted key lies on an optimal prefix of fewer than m moves, so its
//     window key is its grid key, and a cell whose grid key is larger has a window key at least as large: the walk takes
//     the same neighbours as over the grid's keys. What is still undecided (no certificate, no component fields)
//     takes the exact whole-grid search and walk-back of axt_path_cells on a list of (source, target) pairs.
//   * The same gate as axt_path_cost: end points inside the grid, dx^2 + dy^2 < max_dist^2, fewer than max_dist cells;
//     otherwise len = max_dist ("none") and no cells.
// axt_link_cells: the lengths' prefix sum (cell_ptr), the cells as CSR, and the interpolation anchors of the frames a
// gap link skips: frame tail+k (k = 1 .. g-1) at cell index (2k(L-1) + g) / (2g) (round half up).
#include "axt_common.h"
#include "grid.h"

#include <stdlib.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int LINK_PENDING = -1;      // d_len: the window searches still have to look at this link
constexpr int LINK_EXACT = -2;        // d_len: the exact whole-grid search decides this link

// ------------------------------------------------------------------------------------------------ links of the tracks
constexpr int LT = 256;

// exclusive scan of v over the workgroup (LT threads); returns the total in *total
__device__ int block_exclusive_scan(int v, int *s_buf, int *total)
{
    const int tid = threadIdx.x;
    s_buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < LT; off <<= 1) {
        const int add = tid >= off ? s_buf[tid - off] : 0;
        __syncthreads();
        s_buf[tid] += add;
        __syncthreads();
    }
    const int incl = s_buf[tid];
    *total = s_buf[LT - 1];
    __syncthreads();
    return incl - v;
}

// per slot (f, i): head slot (f2*cap + j) or -1, and the gap; per frame: the number of links
__global__ __launch_bounds__(LT) void links_find_kernel(const int *__restrict__ track, const int *__restrict__ count,
                                                        int n_frames, int cap, int max_gap, int *__restrict__ head,
                                                        int *__restrict__ gap, int *__restrict__ frame_cnt)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    __shared__ int s_buf[LT];
    const int nf = min(count[f], cap);
    int mine = 0;
    for (int i = tid; i < nf; i += LT) {
        const int k = track[(long)f * cap + i];
        int h = -1, g = 0;
        if (k >= 0) {
            for (int gg = 1; gg <= max_gap && h < 0; ++gg) {
                const int f2 = f + gg;
                if (f2 >= n_frames) break;
                const int n2 = min(count[f2], cap);
                const int *row = track + (long)f2 * cap;
                for (int j = 0; j < n2; ++j)
                    if (row[j] == k) { h = f2 * cap + j; g = gg; break; }
            }
        }
        head[(long)f * cap + i] = h;
        gap[(long)f * cap + i] = g;
        mine += h >= 0;
    }
    int total;
    block_exclusive_scan(mine, s_buf, &total);
    if (tid == 0) frame_cnt[f] = total;
}

// what an entry adds to a prefix sum (axt_scan_kernel): itself; nothing when negative or, with clamp_from > 0, when
// >= clamp_from (path lengths: max_dist = no path)
struct ClampedCount {
    int clamp_from;
    __device__ int operator()(int v) const { return (v < 0 || (clamp_from > 0 && v >= clamp_from)) ? 0 : v; }
};

__global__ __launch_bounds__(LT) void links_emit_kernel(const int *__restrict__ count, int cap,
                                                        const int *__restrict__ head, const int *__restrict__ gap,
                                                        const int *__restrict__ frame_off, int *__restrict__ links)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    __shared__ int s_buf[LT];
    const int nf = min(count[f], cap);
    int base = frame_off[f];
    for (int i0 = 0; i0 < nf; i0 += LT) {                  // (uniform trip count: every thread reaches the barriers)
        const int i = i0 + tid;
        const long s = (long)f * cap + i;
        const int h = i < nf ? head[s] : -1;
        int total;
        const int pos = base + block_exclusive_scan(h >= 0, s_buf, &total);
        if (h >= 0) {
            links[3 * (long)pos] = (int)s;
            links[3 * (long)pos + 1] = h;
            links[3 * (long)pos + 2] = gap[s];
        }
        base += total;
    }
}

// ------------------------------------------------------------------------------------------------ paths of the links
__device__ __forceinline__ bool link_selected(const int *__restrict__ links, int l, int cap,
                                              const int *__restrict__ head_group, int group)
{
    return head_group == nullptr || head_group[links[3 * (long)l + 1] / cap] == group;
}

// all-ones mask: the staircase of _open_dets_paths, straight into the link's stage row
__global__ __launch_bounds__(256) void link_open_kernel(const int *__restrict__ links, int n_links, const int *__restrict__ x,
                                                        const int *__restrict__ y, int cap, const int *__restrict__ head_group,
                                                        int group, int H, int W, int max_dist, int conn8,
                                                        int *__restrict__ len, int *__restrict__ stage)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_links || !link_selected(links, l, cap, head_group, group)) return;
    const int a = links[3 * (long)l], b = links[3 * (long)l + 1];
    const int xa = x[a], ya = y[a], xb = x[b], yb = y[b];
    const int adx = abs(xb - xa), ady = abs(yb - ya);
    const long d2 = (long)adx * adx + (long)ady * ady;
    const int L = (conn8 ? max(adx, ady) : adx + ady) + 1;
    const bool inb = xa >= 0 && xa < W && ya >= 0 && ya < H && xb >= 0 && xb < W && yb >= 0 && yb < H;
    if (!(d2 < (long)max_dist * max_dist && L < max_dist && inb)) { len[l] = max_dist; return; }
    len[l] = L;
    int *out = stage + (long)l * max_dist;
    const int sx = xb >= xa ? 1 : -1, sy = yb >= ya ? 1 : -1;
    int k = 0;
    if (conn8) {                                            // diagonal first, then straight
        const int m = min(adx, ady);
        for (int q = 0; q <= m; ++q) out[k++] = (ya + sy * q) * W + (xa + sx * q);
        for (int q = 1; q <= adx - m; ++q) out[k++] = (ya + sy * m) * W + (xa + sx * (m + q));
        for (int q = 1; q <= ady - m; ++q) out[k++] = (ya + sy * (m + q)) * W + xb;
    } else {                                                // columns first, then rows
        for (int q = 0; q <= adx; ++q) out[k++] = ya * W + (xa + sx * q);
        for (int q = 1; q <= ady; ++q) out[k++] = (ya + sy * q) * W + xb;
    }
}

// masked grid: the gate, and which links the windows can decide
__global__ __launch_bounds__(256) void link_classify_kernel(const int *__restrict__ links, int n_links, const int *__restrict__ x,
                                                            const int *__restrict__ y, int cap, const int *__restrict__ head_group,
                                                            int group, const unsigned char *__restrict__ mask,
                                                            const int *__restrict__ label, int H, int W, int max_dist,
                                                            int *__restrict__ len)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_links || !link_selected(links, l, cap, head_group, group)) return;
    const int a = links[3 * (long)l], b = links[3 * (long)l + 1];
    const int xa = x[a], ya = y[a], xb = x[b], yb = y[b];
    const long dx = xb - xa, dy = yb - ya;
    const bool inb = xa >= 0 && xa < W && ya >= 0 && ya < H && xb >= 0 && xb < W && yb >= 0 && yb < H;
    if (!inb || dx * dx + dy * dy >= (long)max_dist * max_dist) { len[l] = max_dist; return; }
    const long cs = (long)ya * W + xa, ct = (long)yb * W + xb;
    int v = LINK_PENDING;
    if (cs != ct) {
        if (mask[ct] != 1) v = LINK_EXACT;                                      // target off the mask
        else if (mask[cs] == 1 && label[cs] != label[ct]) v = LINK_EXACT;       // another component
    }
    len[l] = v;
}

constexpr unsigned short D_UNSEEN = 0xfffe, D_BLOCKED = 0xffff;

// One workgroup per link still pending: breadth-first search over on-mask cells in the window of radius R around the
// source (distance field u16 in LDS), stopped at the layer that reaches the target, then the walk back (see the top).
template <int R, int NT>
__global__ __launch_bounds__(NT) void link_bfs_kernel(const int *__restrict__ links, const int *__restrict__ x,
                                                      const int *__restrict__ y, const unsigned char *__restrict__ mask,
                                                      int H, int W, int max_dist, int conn8, int last_bucket,
                                                      int *__restrict__ len, int *__restrict__ stage)
{
    constexpr int WD = 2 * R + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned short dist[];       // [WD][WD]
    const int l = blockIdx.x, tid = threadIdx.x;
    if (len[l] != LINK_PENDING) return;                     // (the same answer for every thread of the workgroup)
    const int a = links[3 * (long)l], b = links[3 * (long)l + 1];
    const int sx = x[a], sy = y[a], tx = x[b], ty = y[b];
    const bool src_on = mask[(long)sy * W + sx] == 1;
    const int limit = min(R, max_dist - 2);                 // moves; paths have fewer than max_dist cells
    const int cheb = max(abs(tx - sx), abs(ty - sy));
    // the path needs >= cheb moves: beyond the window (and within the same component for an on-mask source: beyond
    // max_dist-2 moves means no path)
    const int undecided = (limit == max_dist - 2 && src_on) ? max_dist : (last_bucket ? LINK_EXACT : LINK_PENDING);
    if (cheb > limit) {
        if (tid == 0) len[l] = undecided;
        return;
    }
    const int wy0 = sy - R, wx0 = sx - R;
    for (int e = tid; e < WD * WD; e += NT) {
        const int r = e / WD, c = e - r * WD;
        const int gy = wy0 + r, gx = wx0 + c;
        const bool on = gy >= 0 && gy < H && gx >= 0 && gx < W && mask[(long)gy * W + gx] == 1;
        dist[e] = on ? D_UNSEEN : D_BLOCKED;
    }
    __syncthreads();
    if (tid == 0) dist[R * WD + R] = 0;
    __syncthreads();
    const int tr = ty - wy0, tc = tx - wx0;
    const int nn = conn8 ? 8 : 4;
    int found = (tr == R && tc == R) ? 0 : -1;
    for (int s = 1; s <= limit && found < 0; ++s) {
        // after s moves only the box of radius s around the source can be reached
        const int side = 2 * s + 1, lo = R - s;
        int any = 0;
        for (int e = tid; e < side * side; e += NT) {
            const int r = lo + e / side, c = lo + e % side;
            if (dist[r * WD + c] != D_UNSEEN) continue;
            bool hit = false;                               // (a plain loop: axt_first_neighbour costs a register here)
            for (int q = 0; q < nn && !hit; ++q) {
                const int rr = r + AXT_NB_DY[q], cc = c + AXT_NB_DX[q];
                if (rr < 0 || rr >= WD || cc < 0 || cc >= WD) continue;
                hit = dist[rr * WD + cc] == (unsigned short)(s - 1);
            }
            if (hit) { dist[r * WD + c] = (unsigned short)s; any = 1; }
        }
        const int moved = __syncthreads_or(any);
        if (dist[tr * WD + tc] == (unsigned short)s) found = s;
        else if (!moved) break;                             // the on-mask cells the source reaches are exhausted
    }
    if (tid != 0) return;
    if (found < 0) {
        // every layer up to the limit ran (or the reachable cells ran out): for an on-mask source the target is in its
        // component (link_classify_kernel), so with limit == max_dist-2 there is no path
        len[l] = undecided;
        return;
    }
    int *out = stage + (long)l * max_dist;
    int r = tr, c = tc;
    for (int k = found; k >= 0; --k) {
        out[k] = (wy0 + r) * W + (wx0 + c);
        if (k == 0) break;
        const int q = axt_first_neighbour(r, c, WD, WD, nn, [=](int rr, int cc) {
            return dist[rr * WD + cc] == (unsigned short)(k - 1);
        });
        if (q < 0) {                                        // cannot happen (cell k-1 of a shortest path is a neighbour)
            len[l] = LINK_EXACT;
            return;
        }
        r += AXT_NB_DY[q];
        c += AXT_NB_DX[q];
    }
    len[l] = found + 1;
}

constexpr unsigned int KEY_INF = AXT_KEY32_INF;
constexpr unsigned int KEY_OFF = AXT_KEY32_OFF;     // one off-mask cell entered

// One workgroup per link the breadth-first windows left undecided: the keys (off-mask cells entered, moves) of every
// window cell, label-correcting sweeps over the window until nothing changes; accepted only with the certificate
// above, else the link stays with the exact search.
template <int R, int NT>
__global__ __launch_bounds__(NT) void link_key_kernel(const int *__restrict__ links, const int *__restrict__ x,
                                                      const int *__restrict__ y, const unsigned char *__restrict__ mask,
                                                      const int *__restrict__ label, const unsigned char *__restrict__ off_field,
                                                      int n_comp, int H, int W, int max_dist, int conn8,
                                                      int *__restrict__ len, int *__restrict__ stage)
{
    constexpr int WD = 2 * R + 1;
    static_assert((long)WD * WD < 65536, "moves within the window must fit 16 bits");
    extern __shared__ __attribute__((aligned(16))) unsigned int key[];          // [WD][WD]
    const int l = blockIdx.x, tid = threadIdx.x;
    if (len[l] != LINK_EXACT) return;
    const int a = links[3 * (long)l], b = links[3 * (long)l + 1];
    const int sx = x[a], sy = y[a], tx = x[b], ty = y[b];
    const int adx = abs(tx - sx), ady = abs(ty - sy);
    if (max(adx, ady) > R) return;
    // lower bound of the off-mask cells any path S -> T enters
    const long ct = (long)ty * W + tx;
    const int ls = label[(long)sy * W + sx];
    int lb;
    if (ls > 0) {
        lb = off_field[(long)(ls - 1) * H * W + ct];
    } else {
        // a path that first touches the mask in component q enters >= d_off[q][S] - 1 off-mask cells before that
        // (the source itself is not entered) and >= d_off[q][T] after it
        const long cs = (long)sy * W + sx;
        lb = conn8 ? max(adx, ady) : adx + ady;
        for (int q = 0; q < n_comp; ++q)
            lb = min(lb, (int)off_field[(long)q * H * W + cs] - 1 + (int)off_field[(long)q * H * W + ct]);
    }
    const int wy0 = sy - R, wx0 = sx - R;
    for (int e = tid; e < WD * WD; e += NT) key[e] = (e == R * WD + R) ? 0u : KEY_INF;
    __syncthreads();
    const int nn = conn8 ? 8 : 4;
    for (int sweep = 0; sweep < WD * WD; ++sweep) {
        int changed = 0;
        for (int e = tid; e < WD * WD; e += NT) {
            const int r = e / WD, c = e - r * WD;
            const int gy = wy0 + r, gx = wx0 + c;
            if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
            const unsigned int w = mask[(long)gy * W + gx] == 1 ? 1u : KEY_OFF + 1u;
            unsigned int best = key[e];
            for (int q = 0; q < nn; ++q) {
                const int rr = r + AXT_NB_DY[q], cc = c + AXT_NB_DX[q];
                if (rr < 0 || rr >= WD || cc < 0 || cc >= WD) continue;
                const unsigned int kn = key[rr * WD + cc];
                if (kn != KEY_INF && kn + w < best) best = kn + w;
            }
            if (best < key[e]) { key[e] = best; changed = 1; }      // (one writer per cell; keys only decrease)
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (tid != 0) return;
    const int tr = ty - wy0, tc = tx - wx0;
    const unsigned int kt = key[tr * WD + tc];
    if (kt == KEY_INF) return;
    const int o = (int)(kt >> 16), m = (int)(kt & AXT_KEY32_MOVES);
    if (m > R || o != lb) return;                           // no certificate: the exact search decides
    if (m + 1 >= max_dist) { len[l] = max_dist; return; }
    int *out = stage + (long)l * max_dist;
    int r = tr, c = tc;
    for (int k = m; k >= 0; --k) {
        out[k] = (wy0 + r) * W + (wx0 + c);
        if (k == 0) break;
        const unsigned int kc = key[r * WD + c];
        const unsigned int want = kc - (mask[(long)(wy0 + r) * W + (wx0 + c)] == 1 ? 1u : KEY_OFF + 1u);
        const int q = axt_first_neighbour(r, c, WD, WD, nn, [=](int rr, int cc) { return key[rr * WD + cc] == want; });
        if (q < 0) return;                                  // cannot happen at the fixed point; the exact search decides
        r += AXT_NB_DY[q];
        c += AXT_NB_DX[q];
    }
    len[l] = m + 1;
}

// the links left for the exact search: their end points as (source, target) pair lists
__global__ __launch_bounds__(256) void link_exact_list_kernel(const int *__restrict__ links, int n_links,
                                                              const int *__restrict__ x, const int *__restrict__ y,
                                                              int *__restrict__ len, int *__restrict__ n_exact,
                                                              int *__restrict__ which, int *__restrict__ xy4)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_links || len[l] != LINK_EXACT) return;
    // (the order of the list does not matter: every result goes back to its own link)
    const int k = atomicAdd(n_exact, 1);
    const int a = links[3 * (long)l], b = links[3 * (long)l + 1];
    which[k] = l;
    xy4[k] = x[a];
    xy4[n_links + k] = y[a];
    xy4[2 * (long)n_links + k] = x[b];
    xy4[3 * (long)n_links + k] = y[b];
}

__global__ __launch_bounds__(64) void link_exact_scatter_kernel(const int *__restrict__ which, const int *__restrict__ D,
                                                                const int *__restrict__ cells, int max_dist,
                                                                int *__restrict__ len, int *__restrict__ stage)
{
    const int k = blockIdx.x, l = which[k];
    const int d = D[k];
    if (threadIdx.x == 0) len[l] = d;
    if (d >= max_dist) return;
    for (int q = threadIdx.x; q < d; q += 64) stage[(long)l * max_dist + q] = cells[(long)k * max_dist + q];
}

// CSR cells and interpolation anchors
__global__ __launch_bounds__(64) void link_fill_kernel(const int *__restrict__ links, const int *__restrict__ len,
                                                       const int *__restrict__ stage, const long long *__restrict__ cell_ptr,
                                                       int max_dist, int max_gap, int *__restrict__ cells,
                                                       int *__restrict__ interp)
{
    const int l = blockIdx.x;
    const int L = len[l];
    const bool has = L > 0 && L < max_dist;
    if (has) {
        const long long p = cell_ptr[l];
        for (int q = threadIdx.x; q < L; q += 64) cells[p + q] = stage[(long)l * max_dist + q];
    }
    if (max_gap > 1 && threadIdx.x < max_gap - 1) {
        const int k = threadIdx.x + 1, g = links[3 * (long)l + 2];
        int v = -1;
        if (has && k < g) v = stage[(long)l * max_dist + (2 * k * (L - 1) + g) / (2 * g)];
        interp[(long)l * (max_gap - 1) + k - 1] = v;
    }
}

// AXT_PATH_DEBUG only: how many of the selected links each stage of axt_link_paths decided ("none" included), counted on
// the host from a copy of d_len read back after the stage's launch. A selected link is undecided while its d_len is
// LINK_PENDING or LINK_EXACT; what a stage decided is by how many the undecided ones fell.
struct StageCounts {
    std::vector<char> selected;
    std::vector<int> len;
    int n_selected = 0, undecided = 0;
    int decided[6] = {0, 0, 0, 0, 0, 0};      // gate, bfs31, bfs127, key31, key63, exact

    int init(const int *d_links, int n_links, int cap, const int *d_head_group, int group, hipStream_t st)
    {
        std::vector<int> links(3 * (size_t)n_links), head_group;
        AXT_CHECK_HIP(hipMemcpyAsync(links.data(), d_links, sizeof(int) * links.size(), hipMemcpyDeviceToHost, st));
        AXT_CHECK_HIP(hipStreamSynchronize(st));
        if (d_head_group) {
            int frames = 0;
            for (int l = 0; l < n_links; ++l) frames = std::max(frames, links[3 * (size_t)l + 1] / cap + 1);
            head_group.resize(frames);
            AXT_CHECK_HIP(hipMemcpyAsync(head_group.data(), d_head_group, sizeof(int) * frames, hipMemcpyDeviceToHost, st));
            AXT_CHECK_HIP(hipStreamSynchronize(st));
        }
        selected.resize(n_links);
        len.resize(n_links);
        for (int l = 0; l < n_links; ++l) {
            selected[l] = !d_head_group || head_group[links[3 * (size_t)l + 1] / cap] == group;
            n_selected += selected[l];
        }
        undecided = n_selected;
        return AXT_OK;
    }

    int after(int stage, const int *d_len, hipStream_t st)
    {
        AXT_CHECK_HIP(hipMemcpyAsync(len.data(), d_len, sizeof(int) * len.size(), hipMemcpyDeviceToHost, st));
        AXT_CHECK_HIP(hipStreamSynchronize(st));
        int left = 0;
        for (size_t l = 0; l < len.size(); ++l) left += selected[l] && len[l] < 0;
        decided[stage] = undecided - left;
        undecided = left;
        return AXT_OK;
    }
};

}  // namespace

extern "C" int axt_track_links(const int32_t *d_track, const int32_t *d_count, int n_frames, int cap, int max_gap,
                               int32_t *d_links, int32_t *d_work, int64_t *n_links, void *stream)
{
    AXT_REQUIRE(n_links, "axt_track_links: null argument");
    AXT_REQUIRE(n_frames >= 0 && cap >= 1 && (long)n_frames * cap <= 0x3fffffffL,
                "axt_track_links: n_frames %d negative, cap %d below 1, or more than 2^30 - 1 slots", n_frames, cap);
    AXT_REQUIRE(max_gap >= 1 && max_gap <= 255, "axt_track_links: max_gap %d out of range (1..255)", max_gap);
    AXT_REQUIRE(n_frames == 0 || (d_track && d_count && d_links && d_work), "axt_track_links: null argument");
    *n_links = 0;
    if (n_frames == 0) return AXT_OK;
    hipStream_t st = (hipStream_t)stream;
    const long slots = (long)n_frames * cap;
    int *head = d_work, *gap = d_work + slots, *frame_cnt = d_work + 2 * slots, *frame_off = frame_cnt + n_frames;
    hipLaunchKernelGGL(links_find_kernel, dim3(n_frames), dim3(LT), 0, st, d_track, d_count, n_frames, cap, max_gap, head,
                       gap, frame_cnt);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL((axt_scan_kernel<int, ClampedCount>), dim3(1), dim3(1024), 0, st, (const int *)frame_cnt, (long)n_frames, frame_off,
                       ClampedCount{0});
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(links_emit_kernel, dim3(n_frames), dim3(LT), 0, st, d_count, cap, (const int *)head, (const int *)gap,
                       (const int *)frame_off, d_links);
    AXT_LAUNCH_CHECK();
    int n = 0;
    AXT_CHECK_HIP(hipMemcpyAsync(&n, frame_off + n_frames, sizeof(int), hipMemcpyDeviceToHost, st));
    AXT_CHECK_HIP(hipStreamSynchronize(st));
    *n_links = n;
    return AXT_OK;
}

extern "C" int axt_link_paths(const axt_grid *grid, const int32_t *d_x, const int32_t *d_y, int cap, const int32_t *d_links,
                              int n_links, const int32_t *d_head_group, int group, int H, int W, int max_dist, int conn8,
                              int32_t *d_len, int32_t *d_stage, void *stream)
{
    AXT_REQUIRE(n_links >= 0 && cap >= 1, "axt_link_paths: n_links %d negative or cap %d below 1", n_links, cap);
    AXT_REQUIRE(H > 0 && W > 0 && (long)H * W <= 0x7fffffffL, "axt_link_paths: bad grid size %d x %d", H, W);
    AXT_REQUIRE(max_dist > 1 && max_dist < 32768, "axt_link_paths: max_dist %d out of range (2..32767)", max_dist);
    AXT_REQUIRE(!grid || (grid->H == H && grid->W == W), "axt_link_paths: the grid is not %d x %d", H, W);
    if (n_links == 0) return AXT_OK;
    AXT_REQUIRE(d_x && d_y && d_links && d_len && d_stage, "axt_link_paths: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int nb = (n_links + 255) / 256;
    if (!grid) {
        hipLaunchKernelGGL(link_open_kernel, dim3(nb), dim3(256), 0, st, d_links, n_links, d_x, d_y, cap, d_head_group, group,
                           H, W, max_dist, conn8, d_len, d_stage);
        AXT_LAUNCH_CHECK();
        return AXT_OK;
    }
    const uint8_t *mask = grid->d_mask, *off_field = grid->d_off;
    const int32_t *label = grid->d_label;
    const int n_comp = grid->n_comp;
    AxtScratch counters(st, sizeof(int));     // links left for the exact search
    AXT_CHECK_HIP(counters.err);
    AXT_CHECK_HIP(hipMemsetAsync(counters.p, 0, sizeof(int), st));
    const bool debug = getenv("AXT_PATH_DEBUG") != nullptr;
    StageCounts stages;
    if (debug)
        if (int rc = stages.init(d_links, n_links, cap, d_head_group, group, st)) return rc;
    hipLaunchKernelGGL(link_classify_kernel, dim3(nb), dim3(256), 0, st, d_links, n_links, d_x, d_y, cap, d_head_group, group,
                       mask, label, H, W, max_dist, d_len);
    AXT_LAUNCH_CHECK();
    if (debug)
        if (int rc = stages.after(0, d_len, st)) return rc;
    constexpr int R1 = 31, R2 = 127;
    const size_t lds1 = sizeof(unsigned short) * (2 * R1 + 1) * (2 * R1 + 1);
    const size_t lds2 = sizeof(unsigned short) * (2 * R2 + 1) * (2 * R2 + 1);
    static AxtOncePerDevice once;             // (per device: see axt_common.h)
    if (int rc = axt_max_dynamic_lds(link_bfs_kernel<R2, 1024>, (int)lds2, once)) return rc;
    hipLaunchKernelGGL((link_bfs_kernel<R1, 256>), dim3(n_links), dim3(256), lds1, st, d_links, d_x, d_y, mask, H, W, max_dist,
                       conn8, 0, d_len, d_stage);
    AXT_LAUNCH_CHECK();
    if (debug)
        if (int rc = stages.after(1, d_len, st)) return rc;
    hipLaunchKernelGGL((link_bfs_kernel<R2, 1024>), dim3(n_links), dim3(1024), lds2, st, d_links, d_x, d_y, mask, H, W, max_dist,
                       conn8, 1, d_len, d_stage);
    AXT_LAUNCH_CHECK();
    if (debug)
        if (int rc = stages.after(2, d_len, st)) return rc;
    if (off_field && n_comp >= 1) {
        constexpr int K1 = 31, K2 = 63;
        hipLaunchKernelGGL((link_key_kernel<K1, 256>), dim3(n_links), dim3(256), sizeof(unsigned int) * (2 * K1 + 1) * (2 * K1 + 1),
                           st, d_links, d_x, d_y, mask, label, off_field, n_comp, H, W, max_dist, conn8, d_len, d_stage);
        AXT_LAUNCH_CHECK();
        if (debug)
            if (int rc = stages.after(3, d_len, st)) return rc;
        hipLaunchKernelGGL((link_key_kernel<K2, 1024>), dim3(n_links), dim3(1024), sizeof(unsigned int) * (2 * K2 + 1) * (2 * K2 + 1),
                           st, d_links, d_x, d_y, mask, label, off_field, n_comp, H, W, max_dist, conn8, d_len, d_stage);
        AXT_LAUNCH_CHECK();
        if (debug)
            if (int rc = stages.after(4, d_len, st)) return rc;
    }
    AxtScratch lists(st, sizeof(int) * 5 * (size_t)n_links);
    AXT_CHECK_HIP(lists.err);
    int *which = lists.as<int>(), *xy4 = which + n_links;
    hipLaunchKernelGGL(link_exact_list_kernel, dim3(nb), dim3(256), 0, st, d_links, n_links, d_x, d_y, d_len, counters.as<int>(),
                       which, xy4);
    AXT_LAUNCH_CHECK();
    int n_exact = 0;
    AXT_CHECK_HIP(hipMemcpyAsync(&n_exact, counters.p, sizeof(int), hipMemcpyDeviceToHost, st));
    AXT_CHECK_HIP(hipStreamSynchronize(st));
    if (debug) {
        fprintf(stderr, "link paths: %d of %d links by the exact search\n", n_exact, n_links);
        // (whatever the windows left undecided is the exact search's)
        fprintf(stderr, "link paths: %d links selected: %d gate, %d bfs31, %d bfs127, %d key31, %d key63, %d exact\n",
                stages.n_selected, stages.decided[0], stages.decided[1], stages.decided[2], stages.decided[3],
                stages.decided[4], stages.undecided);
    }
    if (n_exact == 0) return AXT_OK;
    AxtScratch exact(st, sizeof(int) * ((size_t)n_exact * (max_dist + 1)));
    AXT_CHECK_HIP(exact.err);
    int *D = exact.as<int>(), *cells = D + n_exact;
    if (int rc = axt_path_cells_pairs(xy4, xy4 + n_links, xy4 + 2 * (long)n_links, xy4 + 3 * (long)n_links, n_exact, mask, H, W,
                                      max_dist, conn8, D, cells, st))
        return rc;
    hipLaunchKernelGGL(link_exact_scatter_kernel, dim3(n_exact), dim3(64), 0, st, (const int *)which, (const int *)D,
                       (const int *)cells, max_dist, d_len, d_stage);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}

extern "C" int axt_link_cells(const int32_t *d_links, int n_links, const int32_t *d_len, const int32_t *d_stage,
                              int max_dist, int max_gap, int64_t *d_cell_ptr, int32_t *d_cells, int32_t *d_interp,
                              int64_t *n_cells, void *stream)
{
    AXT_REQUIRE(d_cell_ptr && n_cells, "axt_link_cells: null argument");
    AXT_REQUIRE(n_links >= 0, "axt_link_cells: n_links %d is negative", n_links);
    AXT_REQUIRE(max_dist > 1 && max_dist < 32768, "axt_link_cells: max_dist %d out of range (2..32767)", max_dist);
    AXT_REQUIRE(max_gap >= 1 && max_gap <= 255, "axt_link_cells: max_gap %d out of range (1..255)", max_gap);
    AXT_REQUIRE(n_links == 0 || d_len, "axt_link_cells: null argument");
    AXT_REQUIRE(!d_cells || n_links == 0 || (d_links && d_stage && (max_gap == 1 || d_interp)), "axt_link_cells: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (!d_cells) {
        hipLaunchKernelGGL((axt_scan_kernel<long long, ClampedCount>), dim3(1), dim3(1024), 0, st, d_len, (long)n_links,
                           (long long *)d_cell_ptr, ClampedCount{max_dist});
        AXT_LAUNCH_CHECK();
        long long total = 0;
        AXT_CHECK_HIP(hipMemcpyAsync(&total, d_cell_ptr + n_links, sizeof(total), hipMemcpyDeviceToHost, st));
        AXT_CHECK_HIP(hipStreamSynchronize(st));
        *n_cells = total;
        return AXT_OK;
    }
    AXT_REQUIRE(max_gap == 1 || d_interp, "null argument");
    if (n_links == 0) return AXT_OK;
    hipLaunchKernelGGL(link_fill_kernel, dim3(n_links), dim3(64), 0, st, d_links, d_len, d_stage,
                       (const long long *)d_cell_ptr, max_dist, max_gap, d_cells, d_interp);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
