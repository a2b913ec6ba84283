// axt_grid_create / axt_grid_destroy: what a mask needs once per timelapse, computed on the host and uploaded (the
// struct and its conventions: grid.h). Connected-component labels, the per-component off-cell fields d_off and their
// tight-step rows d_tight; the searches that read them are in path_bfs.hip and recon.hip.
#include "axt_common.h"
#include "grid.h"

#include <new>
#include <stdlib.h>
#include <vector>

extern "C" int axt_grid_create(const uint8_t *h_mask, int H, int W, int conn8, axt_grid **out)
{
    AXT_REQUIRE(h_mask && out && H > 0 && W > 0, "bad argument");
    axt_grid *g = new (std::nothrow) axt_grid();
    if (!g) return AXT_ENOMEM;
    g->H = H; g->W = W; g->Ww = (W + 31) / 32; g->conn8 = conn8 ? 1 : 0;
    std::vector<unsigned int> bits((size_t)H * g->Ww, 0u);
    std::vector<int> label((size_t)H * W, 0);
    std::vector<unsigned char> m01((size_t)H * W);
    for (long k = 0; k < (long)H * W; ++k) m01[k] = h_mask[k] == 1;          // AxonDetections.py:598: mask == 1
    for (int yy = 0; yy < H; ++yy)
        for (int xx = 0; xx < W; ++xx)
            if (m01[(size_t)yy * W + xx]) bits[(size_t)yy * g->Ww + (xx >> 5)] |= 1u << (xx & 31);
    // connected components by flood fill
    std::vector<int> stack;
    int next = 0;
    const int nn = conn8 ? 8 : 4;
    for (long k = 0; k < (long)H * W; ++k) {
        if (!m01[k] || label[k]) continue;
        label[k] = ++next;
        stack.push_back((int)k);
        while (!stack.empty()) {
            const int c = stack.back();
            stack.pop_back();
            const int cy = c / W, cx = c % W;
            for (int d = 0; d < nn; ++d) {
                const int ny = cy + AXT_NB_DY[d], nx = cx + AXT_NB_DX[d];
                if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                const int n = ny * W + nx;
                if (m01[n] && !label[n]) { label[n] = next; stack.push_back(n); }
            }
        }
    }
    // fewest off-mask cells from every component to every cell (0-1 breadth-first search per component)
    g->n_comp = next;
    std::vector<unsigned char> off;
    constexpr int kMaxComp = 64;
    if (next >= 1 && next <= kMaxComp && (size_t)next * H * W <= ((size_t)256 << 20)) {
        off.assign((size_t)next * H * W, 255);
        std::vector<int> dist((size_t)H * W);
        std::vector<int> level, later, work;
        for (int L = 1; L <= next; ++L) {
            std::fill(dist.begin(), dist.end(), INT32_MAX);
            level.clear();
            for (long k = 0; k < (long)H * W; ++k)
                if (label[k] == L) { dist[k] = 0; level.push_back((int)k); }
            // Dial's buckets for weights {0, 1}: close the current level over the zero-weight (on-mask) moves, collect
            // the off-mask cells one level up; 255 levels are all a path of <= 251 cells can use
            for (int d = 0; d < 255 && !level.empty(); ++d) {
                work.swap(level);
                later.clear();
                while (!work.empty()) {
                    const int c = work.back();
                    work.pop_back();
                    if (dist[c] != d) continue;
                    const int cy = c / W, cx = c % W;
                    for (int q = 0; q < nn; ++q) {
                        const int ny = cy + AXT_NB_DY[q], nx = cx + AXT_NB_DX[q];
                        if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
                        const int n = ny * W + nx;
                        const int nd = d + (m01[n] ? 0 : 1);
                        if (nd < dist[n]) {
                            dist[n] = nd;
                            if (nd == d) work.push_back(n); else later.push_back(n);
                        }
                    }
                }
                level.clear();
                for (int n : later)
                    if (dist[n] == d + 1) level.push_back(n);
            }
            unsigned char *o = off.data() + (size_t)(L - 1) * H * W;
            for (long k = 0; k < (long)H * W; ++k)
                if (dist[k] < 255) o[k] = (unsigned char)dist[k];
        }
    }
    g->has_fields = next == 0 || !off.empty();
    std::vector<unsigned int> tightv;
    if (!off.empty()) {
        const int Ww = g->Ww;
        tightv.assign((size_t)next * nn * H * Ww, 0u);
        for (int L = 0; L < next; ++L) {
            const unsigned char *o = off.data() + (size_t)L * H * W;
            for (int d = 0; d < nn; ++d) {
                unsigned int *tb = tightv.data() + ((size_t)L * nn + d) * H * Ww;
                for (int yy = 0; yy < H; ++yy) {
                    const int py = yy + AXT_NB_DY[d];
                    if (py < 0 || py >= H) continue;
                    for (int xx = 0; xx < W; ++xx) {
                        const int px = xx + AXT_NB_DX[d];
                        if (px < 0 || px >= W) continue;
                        const int kc = o[(size_t)yy * W + xx], kp = o[(size_t)py * W + px];
                        if (kc < 255 && kp < 255 && kc == kp + (m01[(size_t)yy * W + xx] ? 0 : 1))
                            tb[(size_t)yy * Ww + (xx >> 5)] |= 1u << (xx & 31);
                    }
                }
            }
        }
    }
    int rc = AXT_OK;
    if (!off.empty() && (hipMalloc((void **)&g->d_off, off.size()) != hipSuccess ||
                         hipMemcpy(g->d_off, off.data(), off.size(), hipMemcpyHostToDevice) != hipSuccess)) {
        axt_set_error("axt_grid_create: device allocation for the component distance fields failed");
        axt_grid_destroy(g);
        return AXT_ENOMEM;
    }
    if (!tightv.empty() && (hipMalloc((void **)&g->d_tight, tightv.size() * 4) != hipSuccess ||
                            hipMemcpy(g->d_tight, tightv.data(), tightv.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        axt_set_error("axt_grid_create: device allocation for the tight-step rows failed");
        axt_grid_destroy(g);
        return AXT_ENOMEM;
    }
    if (hipMalloc((void **)&g->d_mask, (size_t)H * W) != hipSuccess || hipMalloc((void **)&g->d_bits, bits.size() * 4) != hipSuccess ||
        hipMalloc((void **)&g->d_label, label.size() * 4) != hipSuccess) {
        axt_set_error("axt_grid_create: device allocation failed");
        rc = AXT_ENOMEM;
    } else if (hipMemcpy(g->d_mask, m01.data(), m01.size(), hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(g->d_bits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(g->d_label, label.data(), label.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        axt_set_error("axt_grid_create: upload failed");
        rc = AXT_EHIP;
    }
    if (rc) { axt_grid_destroy(g); return rc; }
    *out = g;
    return AXT_OK;
}

extern "C" void axt_grid_destroy(axt_grid *g)
{
    if (!g) return;
    (void)hipFree(g->d_mask);
    (void)hipFree(g->d_bits);
    (void)hipFree(g->d_label);
    (void)hipFree(g->d_off);
    (void)hipFree(g->d_tight);
    delete g;
}
