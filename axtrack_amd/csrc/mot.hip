// Tracking scores (MOTChallenge metrics) of K associations of the same detections against labelled identities, on the
// device: the counts behind axtrack_amd/mot_metrics.py (accumulate + summarize), DESIGN.md 6.8g.
//
// THE DEFINITION (stated here and in DESIGN.md 6.8g, nowhere else)
// Inputs per frame: the labels (dense identity g in [0, no), x, y) and the IDed detections = the slots j < count[f] with
// 0 <= track[j] < nh ("hypotheses"; identities are unique within a frame on both sides; labels with an identity outside
// [0, no) and slots with a track outside [0, nh) take no part). d2 = dx^2 + dy^2 on the integer anchors; a pair is
// admissible when d2 <= max_dist^2 (inclusive, as mot_metrics.sq_distances).
// CLEAR-MOT pass, frame after frame, with a partner table (label identity -> track identity, -1 = none) carried along:
//   1. A label whose remembered partner is present and admissible keeps it: MATCH. If two labels remember the same
//      partner, the lower label slot wins and the other goes on to step 2. The partner table is not changed here.
//   2. The remaining labels and hypotheses are assigned with as many admissible pairs as possible first, then the
//      smallest sum of the 64-bit integer costs  (d2 << 26) | hash16(kind 4, label identity, track identity)  -- the
//      splitmix hash of axt_arc_cost_int, whose kinds 0-3 are taken. At most 1024 labels and 1024 hypotheses per frame
//      (cap, gcap <= 1024) and max_dist <= 255: 1024 hashes sum to < 2^26, so the low bits never outweigh one unit of
//      d2 -- the result is one of the true optima, and always the same one. A pair whose label remembers another
//      partner is a SWITCH, otherwise a MATCH; the partner table takes the new partner.
//   3. Unassigned labels are MISS, unassigned hypotheses are FP. A MISS does not clear the partner.
// Cardinality first, by an integer penalty that fits: every row of step 2 may instead take a private dummy column at
// P = (min(rows, cols) + 1) << 42. A pair costs < 2^42 (d2 <= 255^2 < 2^16, shifted by 26, hash below), a matching has at
// most min(rows, cols) pairs, so P exceeds every admissible total and one more pair always pays. P <= 1025 * 2^42; see
// lsap_wave for the bound on every intermediate of the solver (all below 2^63).
// Identity scores: co[g, h] = number of frames in which label identity g and track identity h are both present and
// admissible; idtp = max over matchings M of sum_M co (DESIGN.md 6.8g derives this from summarize's padded problem);
// idfn = n_obj - idtp, idfp = n_pred - idtp. Only the optimum's VALUE is used, so ties need no perturbation.
// Per label identity: frames present, frames not missed; a fragmentation is a run of misses that lies between two
// non-miss events of the identity. motp = (exact integer sum of matched d2) / (matches + switches).
//
// Kernels: co-occurrence -- one workgroup per (frame, association), integer atomics, order-free; CLEAR pass -- one
// wavefront per association walks the frames in order (serial by definition; the parallelism is K and the lanes inside a
// frame); identity matching -- one wavefront per association, exact assignment on co (no x nh).
#include "axt_common.h"

namespace {

constexpr long MINF = 0x7fffffffffffffffL;       // "not admitted": never takes part in arithmetic
constexpr int MOT_MAX_SIDE = 1024;               // labels / hypotheses per frame
constexpr int MOT_MAX_DIST = 255;

__device__ __forceinline__ long mot_pair_cost(long d2, long label, long track)
{
    unsigned long x = (4ul << 60) ^ ((unsigned long)label << 30) ^ (unsigned long)track;
    x += 0x9E3779B97F4A7C15ul;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ul;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBul;
    x ^= x >> 31;
    return (d2 << 26) | (long)(x & 0xFFFFul);
}

// wave-wide minima: DPP inside the rows of 16 lanes, v_readlane across the four rows (the idiom of hungarian.hip; here the
// key needs all 64 bits -- the penalty P -- so the index follows in a second, 32-bit reduction)
#define MOT_DPP_MIN64(v, ctrl)                                                                            \
    {                                                                                                     \
        const unsigned lo_ = (unsigned)(v), hi_ = (unsigned)((v) >> 32);                                  \
        const unsigned ol_ = __builtin_amdgcn_update_dpp(lo_, lo_, ctrl, 0xF, 0xF, false);                \
        const unsigned oh_ = __builtin_amdgcn_update_dpp(hi_, hi_, ctrl, 0xF, 0xF, false);                \
        const unsigned long o_ = ((unsigned long)oh_ << 32) | ol_;                                        \
        (v) = o_ < (v) ? o_ : (v);                                                                        \
    }
#define MOT_DPP_MIN32(v, ctrl)                                                             \
    {                                                                                      \
        const unsigned o_ = __builtin_amdgcn_update_dpp(v, v, ctrl, 0xF, 0xF, false);      \
        v = o_ < v ? o_ : v;                                                               \
    }
__device__ __forceinline__ unsigned long mot_wave_min_u64(unsigned long v)
{
    MOT_DPP_MIN64(v, 0xB1);       // quad_perm [1,0,3,2]
    MOT_DPP_MIN64(v, 0x4E);       // quad_perm [2,3,0,1]
    MOT_DPP_MIN64(v, 0x141);      // row_half_mirror
    MOT_DPP_MIN64(v, 0x140);      // row_mirror
    unsigned long best = ~0ul;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, r * 16), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), r * 16);
        const unsigned long o = ((unsigned long)hi << 32) | lo;
        best = o < best ? o : best;
    }
    return best;
}
__device__ __forceinline__ unsigned mot_wave_min_u32(unsigned v)
{
    MOT_DPP_MIN32(v, 0xB1);
    MOT_DPP_MIN32(v, 0x4E);
    MOT_DPP_MIN32(v, 0x141);
    MOT_DPP_MIN32(v, 0x140);
    unsigned best = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned o = __builtin_amdgcn_readlane(v, r * 16);
        best = o < best ? o : best;
    }
    return best;
}
// smallest key (>= 0), ties to the smallest index; all lanes MINF: key stays MINF, idx is meaningless
__device__ __forceinline__ void mot_wave_argmin(long &key, int &idx)
{
    const unsigned long best = mot_wave_min_u64((unsigned long)key);
    idx = (int)mot_wave_min_u32((unsigned long)key == best ? (unsigned)idx : 0xffffffffu);
    key = (long)best;
}

// Exact rectangular assignment by shortest augmenting paths (Jonker-Volgenant / Crouse 2016, Alg. 1) for ONE wavefront:
// rows 0..n-1, columns 0..m-1, cost(i, j) >= 0 or MINF (not admitted); every row may take a private dummy column at
// `dummy` instead. Minimises sum of the chosen costs; on return col4row[i] >= 0 (a column) or -2 (the dummy).
// Lanes own the columns j = lane, lane + 64, ...; the state may live in LDS or in global memory (generic pointers).
// Ranges (CLEAR pass: n, m <= 1024, costs < 2^42 < dummy <= 1025 * 2^42): a search's distance minVal never exceeds the
// reduced cost of the start row's own dummy (that row's u is still 0), so minVal <= dummy; a row dual only grows, by at
// most minVal per search: 0 <= u <= n * dummy; a column dual only falls, by at most minVal per search:
// -n * dummy <= v <= 0. Hence every r = minVal + c - u - v below is < (n + 2) * dummy <= 1026 * 1025 * 2^42 < 2^63.
// The identity matching (dummy = n_frames, n <= 2^24) is far below that.
struct LsapState {
    long *u, *v, *spc;
    int *row4col, *col4row, *pred, *sr;
    unsigned char *in_sc;
};

template <class Cost>
__device__ __forceinline__ void lsap_wave(int n, int m, long dummy, Cost cost, const LsapState &s, int lane)
{
    for (int j = lane; j < m; j += 64) { s.v[j] = 0; s.row4col[j] = -1; }
    for (int i = lane; i < n; i += 64) { s.u[i] = 0; s.col4row[i] = -1; }
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        for (int j = lane; j < m; j += 64) { s.spc[j] = MINF; s.in_sc[j] = 0; }
        __syncthreads();
        long minVal = 0, best_dummy = MINF;
        int cur = i, dummy_row = -1, n_sr = 0, sink = -1;             // sink >= 0: real column; -2: dummy of dummy_row
        for (;;) {
            if (lane == 0) s.sr[n_sr] = cur;
            ++n_sr;
            const long ucur = s.u[cur];
            const long rd = minVal + dummy - ucur;
            if (rd < best_dummy) { best_dummy = rd; dummy_row = cur; }
            long bkey = MINF;
            int bidx = 0x7fffffff;
            for (int j = lane; j < m; j += 64) {
                if (s.in_sc[j]) continue;
                const long c = cost(cur, j);
                long d = s.spc[j];
                if (c != MINF) {
                    const long r = minVal + c - ucur - s.v[j];
                    if (r < d) { d = r; s.spc[j] = r; s.pred[j] = cur; }
                }
                if (d < bkey) { bkey = d; bidx = j; }
            }
            mot_wave_argmin(bkey, bidx);
            if (best_dummy <= bkey) { sink = -2; minVal = best_dummy; break; }
            minVal = bkey;
            if (lane == 0) s.in_sc[bidx] = 1;
            __syncthreads();
            if (s.row4col[bidx] < 0) { sink = bidx; break; }
            cur = s.row4col[bidx];
        }
        __syncthreads();
        // dual update: rows of SR, columns of SC
        for (int k = lane; k < n_sr; k += 64) {
            const int r = s.sr[k];
            s.u[r] += (k == 0) ? minVal : minVal - s.spc[s.col4row[r]];
        }
        for (int j = lane; j < m; j += 64)
            if (s.in_sc[j] && j != sink) s.v[j] -= minVal - s.spc[j];
        __syncthreads();
        // augment back to row i
        if (lane == 0) {
            int r, jnew;
            if (sink == -2) { r = dummy_row; jnew = -2; }
            else { r = s.pred[sink]; jnew = sink; }
            for (;;) {
                const int jprev = s.col4row[r];
                s.col4row[r] = jnew;
                if (jnew >= 0) s.row4col[jnew] = r;
                if (r == i) break;
                jnew = jprev;
                r = s.pred[jnew];
            }
        }
        __syncthreads();
    }
}

// carve the solver's state for n rows and m columns out of p (8-byte aligned); returns the bytes used
__host__ __device__ inline size_t lsap_bytes(size_t n, size_t m)
{
    return 8 * n + 8 * m + 8 * m + 4 * (m + (m & 1)) + 4 * (n + (n & 1)) + 4 * (m + (m & 1)) + 4 * (n + (n & 1)) + ((m + 7) & ~(size_t)7);
}
__device__ __forceinline__ LsapState lsap_carve(unsigned char *p, size_t n, size_t m)
{
    LsapState s;
    s.u = reinterpret_cast<long *>(p);
    s.v = s.u + n;
    s.spc = s.v + m;
    s.row4col = reinterpret_cast<int *>(s.spc + m);
    s.col4row = s.row4col + (m + (m & 1));
    s.pred = s.col4row + (n + (n & 1));
    s.sr = s.pred + (m + (m & 1));
    s.in_sc = reinterpret_cast<unsigned char *>(s.sr + (n + (n & 1)));
    return s;
}

// ---- co-occurrence: co[k, g, h] += 1 for every admissible (label, hypothesis) pair of frame f. grid (F, K).
__global__ __launch_bounds__(256) void mot_cooc_kernel(
    const int *__restrict__ track, const int *__restrict__ x, const int *__restrict__ y, const int *__restrict__ count,
    int n_frames, int cap, const int *__restrict__ gid, const int *__restrict__ gx, const int *__restrict__ gy,
    const int *__restrict__ gcount, int gcap, int no, int nh, int md2, int *__restrict__ scratch, size_t per_k_ints)
{
    const int f = blockIdx.x, k = blockIdx.y;
    const int nd = max(min(count[f], cap), 0), ng = max(min(gcount[f], gcap), 0);
    const long d0 = (long)f * cap, g0 = (long)f * gcap;
    const int *tr = track + ((long)k * n_frames + f) * cap;
    int *co = scratch + (size_t)k * per_k_ints;
    for (int p = threadIdx.x; p < ng * nd; p += 256) {
        const int i = p / nd, j = p - i * nd;
        const int g = gid[g0 + i], t = tr[j];
        if (g < 0 || g >= no || t < 0 || t >= nh) continue;
        const int dx = x[d0 + j] - gx[g0 + i], dy = y[d0 + j] - gy[g0 + i];
        const long d2 = (long)dx * dx + (long)dy * dy;
        if (d2 <= md2) atomicAdd(&co[(size_t)g * nh + t], 1);
    }
}

// ---- CLEAR pass: one wavefront per association, frames in order.
__global__ __launch_bounds__(64) void mot_clear_kernel(
    const int *__restrict__ track, const int *__restrict__ x, const int *__restrict__ y, const int *__restrict__ count,
    int n_frames, int cap, const int *__restrict__ gid, const int *__restrict__ gx, const int *__restrict__ gy,
    const int *__restrict__ gcount, int gcap, int no, int nh, int md2, int *__restrict__ partner_all,
    unsigned char *__restrict__ fstate_all, size_t per_k_bytes, long *__restrict__ counts, int *__restrict__ tallies_all,
    unsigned char *__restrict__ ev_kind, int *__restrict__ ev_partner, unsigned char *__restrict__ ev_fp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
    const int k = blockIdx.x, lane = threadIdx.x;
    const size_t gc2 = gcap + (gcap & 1), c2 = cap + (cap & 1);
    LsapState S = lsap_carve(msm, gcap, cap);
    int *lg = reinterpret_cast<int *>(msm + lsap_bytes(gcap, cap));      // [gcap] label identity (-1: takes no part)
    int *lx = lg + gc2, *ly = lx + gc2;                 // [gcap] label anchors
    int *cand = ly + gc2;                               // [gcap] step 1: the hypothesis holding the remembered partner
    int *lpart = cand + gc2;                            // [gcap] partner slot of the label's event
    int *rows = lpart + gc2;                            // [gcap] step 2: label slots still open
    int *hx = rows + gc2, *hy = hx + c2;                // [cap] hypothesis anchors
    int *htr = hy + c2, *hslot = htr + c2;              // [cap] track identity, detection slot
    int *claim = hslot + c2;                            // [cap] step 1: lowest claiming label slot
    int *cols = claim + c2;                             // [cap] step 2: hypotheses still open
    unsigned char *lkind = reinterpret_cast<unsigned char *>(cols + c2);     // [gcap] 0 none, 1 MATCH, 2 SWITCH
    unsigned char *hdone = lkind + ((gcap + 7) & ~7);   // [cap]
    unsigned char *slotfp = hdone + ((cap + 7) & ~7);   // [cap] FP flag per detection slot

    int *partner = reinterpret_cast<int *>(reinterpret_cast<unsigned char *>(partner_all) + (size_t)k * per_k_bytes);
    unsigned char *fstate = fstate_all + (size_t)k * per_k_bytes;    // 0 never tracked, 1 tracked last, 2 in a miss run after it
    int *tallies = tallies_all + (size_t)k * no * 2;
    for (int g = lane; g < no; g += 64) { partner[g] = -1; fstate[g] = 0; tallies[2 * g] = 0; tallies[2 * g + 1] = 0; }
    for (int j = lane; j < cap; j += 64) slotfp[j] = 0;
    __syncthreads();

    long n_match = 0, n_switch = 0, n_miss = 0, n_fp = 0, sum_d2 = 0, n_obj = 0, n_pred = 0, n_frag = 0;
    const unsigned long lt_mask = (1ul << lane) - 1;
    for (int f = 0; f < n_frames; ++f) {
        const int nd = max(min(count[f], cap), 0), ng = max(min(gcount[f], gcap), 0);
        const long d0 = (long)f * cap, g0 = (long)f * gcap;
        const int *tr = track + ((long)k * n_frames + f) * cap;
        for (int i = lane; i < ng; i += 64) {
            const int g = gid[g0 + i];
            lg[i] = (g >= 0 && g < no) ? g : -1;
            lx[i] = gx[g0 + i];
            ly[i] = gy[g0 + i];
            lkind[i] = 0;
            lpart[i] = -1;
            cand[i] = -1;
        }
        int nhyp = 0;                                    // the slots with an identity, in slot order
        for (int base = 0; base < nd; base += 64) {
            const int j = base + lane;
            const int t = j < nd ? tr[j] : -1;
            const bool ok = t >= 0 && t < nh;
            const unsigned long m = __ballot(ok);
            if (ok) {
                const int pos = nhyp + __popcll(m & lt_mask);
                hx[pos] = x[d0 + j];
                hy[pos] = y[d0 + j];
                htr[pos] = t;
                hslot[pos] = j;
                claim[pos] = 0x7fffffff;
                hdone[pos] = 0;
            }
            nhyp += __popcll(m);
        }
        __syncthreads();
        if (lane == 0) n_pred += nhyp;
        // 1. remembered partners, lowest label slot per hypothesis
        for (int i = lane; i < ng; i += 64) {
            const int g = lg[i];
            if (g < 0) continue;
            n_obj += 1;
            atomicAdd(&tallies[2 * g], 1);
            const int p = partner[g];
            if (p < 0) continue;
            for (int j = 0; j < nhyp; ++j)
                if (htr[j] == p) {
                    const int dx = hx[j] - lx[i], dy = hy[j] - ly[i];
                    if ((long)dx * dx + (long)dy * dy <= md2) { cand[i] = j; atomicMin(&claim[j], i); }
                    break;
                }
        }
        __syncthreads();
        for (int i = lane; i < ng; i += 64) {
            const int j = cand[i];
            if (j >= 0 && claim[j] == i) {
                const int dx = hx[j] - lx[i], dy = hy[j] - ly[i];
                lkind[i] = 1;
                lpart[i] = hslot[j];
                hdone[j] = 1;
                n_match += 1;
                sum_d2 += (long)dx * dx + (long)dy * dy;
            }
        }
        __syncthreads();
        // 2. the rest: compact the open labels and hypotheses, assign exactly
        int nr = 0, nc = 0;
        for (int base = 0; base < ng; base += 64) {
            const int i = base + lane;
            const bool open = i < ng && lg[i] >= 0 && lkind[i] == 0;
            const unsigned long m = __ballot(open);
            if (open) rows[nr + __popcll(m & lt_mask)] = i;
            nr += __popcll(m);
        }
        for (int base = 0; base < nhyp; base += 64) {
            const int j = base + lane;
            const bool open = j < nhyp && !hdone[j];
            const unsigned long m = __ballot(open);
            if (open) cols[nc + __popcll(m & lt_mask)] = j;
            nc += __popcll(m);
        }
        __syncthreads();
        if (nr > 0 && nc > 0) {
            const long penalty = (long)(min(nr, nc) + 1) << 42;
            lsap_wave(nr, nc, penalty, [&](int r, int c) -> long {
                const int i = rows[r], j = cols[c];
                const int dx = hx[j] - lx[i], dy = hy[j] - ly[i];
                const long d2 = (long)dx * dx + (long)dy * dy;
                return d2 <= md2 ? mot_pair_cost(d2, lg[i], htr[j]) : MINF;
            }, S, lane);
            for (int r = lane; r < nr; r += 64) {
                const int c = S.col4row[r];
                if (c < 0) continue;
                const int i = rows[r], j = cols[c], g = lg[i];
                const int dx = hx[j] - lx[i], dy = hy[j] - ly[i];
                const int p = partner[g];
                const bool sw = p >= 0 && p != htr[j];
                lkind[i] = sw ? 2 : 1;
                lpart[i] = hslot[j];
                hdone[j] = 1;
                partner[g] = htr[j];
                n_switch += sw;
                n_match += !sw;
                sum_d2 += (long)dx * dx + (long)dy * dy;
            }
            __syncthreads();
        }
        // 3. misses and false positives; the per-identity tallies and the fragmentation state
        for (int i = lane; i < gcap; i += 64) {
            int kind = 0, part = -1;
            if (i < ng && lg[i] >= 0) {
                const int g = lg[i];
                kind = lkind[i] ? lkind[i] : 3;
                part = lpart[i];
                const unsigned char st = fstate[g];
                if (kind == 3) {
                    n_miss += 1;
                    if (st == 1) fstate[g] = 2;
                } else {
                    tallies[2 * g + 1] += 1;
                    n_frag += st == 2;
                    fstate[g] = 1;
                }
            }
            if (ev_kind) ev_kind[((long)k * n_frames + f) * gcap + i] = (unsigned char)kind;
            if (ev_partner) ev_partner[((long)k * n_frames + f) * gcap + i] = part;
        }
        for (int j = lane; j < nhyp; j += 64)
            if (!hdone[j]) { n_fp += 1; slotfp[hslot[j]] = 1; }
        __syncthreads();
        for (int j = lane; j < cap; j += 64) {
            if (ev_fp) ev_fp[((long)k * n_frames + f) * cap + j] = slotfp[j];
            slotfp[j] = 0;
        }
        __syncthreads();
    }
    long n_unique = 0;
    for (int g = lane; g < no; g += 64) n_unique += tallies[2 * g] > 0;
    for (int o = 32; o > 0; o >>= 1) {
        n_match += __shfl_xor(n_match, o); n_switch += __shfl_xor(n_switch, o); n_miss += __shfl_xor(n_miss, o);
        n_fp += __shfl_xor(n_fp, o); sum_d2 += __shfl_xor(sum_d2, o); n_obj += __shfl_xor(n_obj, o);
        n_pred += __shfl_xor(n_pred, o); n_frag += __shfl_xor(n_frag, o); n_unique += __shfl_xor(n_unique, o);
    }
    if (lane == 0) {
        long *c = counts + (long)k * 10;
        c[0] = n_match; c[1] = n_switch; c[2] = n_miss; c[3] = n_fp; c[4] = sum_d2;
        c[5] = n_obj; c[6] = n_pred; c[7] = n_unique; c[8] = n_frag;
    }
}

// ---- identity matching: idtp = max-weight matching of label identities to track identities on co[k] (no x nh).
// As an assignment: cost W - co where co > 0 (W = n_frames >= co), not admitted where co == 0; the dummy (cost W) stands
// for "matched to nobody". min sum = no * W - max sum co. State in LDS (use_lds) or in the association's scratch.
__global__ __launch_bounds__(64) void mot_identity_kernel(const int *__restrict__ scratch, size_t per_k_ints, int no, int nh,
                                                          int n_frames, unsigned char *__restrict__ state_all,
                                                          size_t per_k_bytes, int use_lds, long *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ism[];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int *co = scratch + (size_t)k * per_k_ints;
    LsapState S = lsap_carve(use_lds ? ism : state_all + (size_t)k * per_k_bytes, no, nh);
    const long W = n_frames;
    lsap_wave(no, nh, W, [&](int o, int h) -> long {
        const int c = co[(size_t)o * nh + h];
        return c > 0 ? W - c : MINF;
    }, S, lane);
    long idtp = 0;
    for (int o = lane; o < no; o += 64) {
        const int h = S.col4row[o];
        if (h >= 0) idtp += co[(size_t)o * nh + h];
    }
    for (int o = 32; o > 0; o >>= 1) idtp += __shfl_xor(idtp, o);
    if (lane == 0) counts[(long)k * 10 + 9] = idtp;
}

size_t clear_lds_bytes(int gcap, int cap)
{
    const size_t gc2 = gcap + (gcap & 1), c2 = cap + (cap & 1);
    return lsap_bytes(gcap, cap) + 4 * (6 * gc2 + 6 * c2) + ((gcap + 7) & ~7) + 2 * ((cap + 7) & ~7);
}

}  // namespace

// Scratch per association (8-byte aligned pieces): co i32 [no, nh] | partner i32 [no] + fragmentation state u8 [no] |
// the identity matching's solver state.
extern "C" int axt_mot_scores(const int32_t *d_track, int n_assoc, const int32_t *d_x, const int32_t *d_y,
                              const int32_t *d_count, int n_frames, int cap, const int32_t *d_gid, const int32_t *d_gx,
                              const int32_t *d_gy, const int32_t *d_gcount, int gcap, int no, int nh, int max_dist,
                              int64_t *d_counts, int32_t *d_tallies, uint8_t *d_ev_kind, int32_t *d_ev_partner,
                              uint8_t *d_ev_fp, void *d_scratch, size_t *scratch_bytes, void *stream)
{
    AXT_REQUIRE(scratch_bytes, "axt_mot_scores: null argument");
    AXT_REQUIRE(n_assoc >= 1 && n_assoc <= 65535 && n_frames >= 1, "axt_mot_scores: bad shape (%d associations, %d frames)", n_assoc, n_frames);
    AXT_REQUIRE(cap >= 1 && cap <= MOT_MAX_SIDE && gcap >= 1 && gcap <= MOT_MAX_SIDE,
                "axt_mot_scores: cap %d / gcap %d out of range [1,%d]", cap, gcap, MOT_MAX_SIDE);
    AXT_REQUIRE(no >= 1 && no <= (1 << 24) && nh >= 1 && nh <= (1 << 24), "axt_mot_scores: no %d / nh %d out of range [1,2^24]", no, nh);
    AXT_REQUIRE(max_dist >= 0 && max_dist <= MOT_MAX_DIST, "axt_mot_scores: max_dist %d out of range [0,%d]", max_dist, MOT_MAX_DIST);
    const size_t co_bytes = ((size_t)no * nh * 4 + 7) & ~(size_t)7;
    const size_t tab_bytes = (((size_t)no * 4 + 7) & ~(size_t)7) + (((size_t)no + 7) & ~(size_t)7);
    const size_t id_bytes = lsap_bytes(no, nh);
    const bool id_lds = id_bytes <= 64 * 1024;
    const size_t per_k = co_bytes + tab_bytes + (id_lds ? 0 : id_bytes);
    const size_t have = *scratch_bytes, need = per_k * (size_t)n_assoc;
    *scratch_bytes = need;
    if (!d_scratch) return AXT_OK;                    // size query
    AXT_REQUIRE(d_track && d_x && d_y && d_count && d_gid && d_gx && d_gy && d_gcount && d_counts && d_tallies,
                "axt_mot_scores: null argument");
    AXT_REQUIRE(have >= need, "axt_mot_scores: scratch of %zu bytes, %zu needed", have, need);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *base = static_cast<unsigned char *>(d_scratch);
    const int md2 = max_dist * max_dist;
    const size_t lds = clear_lds_bytes(gcap, cap);
    static AxtOncePerDevice once;
    int rc = axt_max_dynamic_lds(mot_clear_kernel, 160 * 1024, once);
    if (rc) return rc;
    AXT_CHECK_HIP(hipMemsetAsync(base, 0, need, st));
    hipLaunchKernelGGL(mot_cooc_kernel, dim3(n_frames, n_assoc), dim3(256), 0, st, d_track, d_x, d_y, d_count, n_frames, cap,
                       d_gid, d_gx, d_gy, d_gcount, gcap, no, nh, md2, reinterpret_cast<int *>(base), per_k / 4);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(mot_clear_kernel, dim3(n_assoc), dim3(64), lds, st, d_track, d_x, d_y, d_count, n_frames, cap, d_gid,
                       d_gx, d_gy, d_gcount, gcap, no, nh, md2, reinterpret_cast<int *>(base + co_bytes),
                       base + co_bytes + (((size_t)no * 4 + 7) & ~(size_t)7), per_k, (long *)d_counts, d_tallies, d_ev_kind,
                       d_ev_partner, d_ev_fp);
    AXT_LAUNCH_CHECK();
    hipLaunchKernelGGL(mot_identity_kernel, dim3(n_assoc), dim3(64), id_lds ? id_bytes : 0, st,
                       reinterpret_cast<const int *>(base), per_k / 4, no, nh, n_frames, base + co_bytes + tab_bytes, per_k,
                       (int)id_lds, (long *)d_counts);
    AXT_LAUNCH_CHECK();
    return AXT_OK;
}
