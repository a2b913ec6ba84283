// Shared helpers for libaxtrack_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <stdio.h>
#include <string.h>

#include "../../include/axtrack_hip.h"

void axt_set_error(const char *fmt, ...);

#define AXT_CHECK_HIP(expr)                                                                   \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            axt_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
            return AXT_EHIP;                                                                  \
        }                                                                                     \
    } while (0)

#define AXT_REQUIRE(cond, ...)                      \
    do {                                            \
        if (!(cond)) {                              \
            axt_set_error(__VA_ARGS__);             \
            return AXT_EINVAL;                      \
        }                                           \
    } while (0)

#define AXT_LAUNCH_CHECK() AXT_CHECK_HIP(hipGetLastError())

static inline int axt_cdiv(int a, int b) { return (a + b - 1) / b; }

// Stream-ordered scratch that every return path gives back: hipMallocAsync on construction (0 bytes: nothing, p stays
// NULL), hipFreeAsync on the same stream in the destructor. Check with AXT_CHECK_HIP(buf.err) before use.
struct AxtScratch {
    void *p = nullptr;
    hipStream_t st;
    hipError_t err = hipSuccess;
    AxtScratch(hipStream_t stream, size_t bytes) : st(stream)
    {
        if (bytes && (err = hipMallocAsync(&p, bytes, st)) != hipSuccess) p = nullptr;
    }
    ~AxtScratch() { if (p) (void)hipFreeAsync(p, st); }
    AxtScratch(const AxtScratch &) = delete;
    AxtScratch &operator=(const AxtScratch &) = delete;
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// Launch attributes (hipFuncSetAttribute) and occupancy answers belong to the CURRENT device, not to the process: a
// second device in one process (Detector(device='cuda:1')) must get its own. One of these per launcher remembers, per
// device index, that the launcher's kernels are set up there (a bit per device; devices beyond 63 are set up on every
// call). No other state survives a call, as include/axtrack_hip.h promises.
struct AxtOncePerDevice {
    std::atomic<uint64_t> done{0};
    int dev = 0;
    // true: the kernels of this launcher still need their attributes on the current device (call mark() afterwards)
    bool pending()
    {
        if (hipGetDevice(&dev) != hipSuccess) dev = 64;
        return dev < 0 || dev >= 64 || !(done.load(std::memory_order_acquire) >> dev & 1);
    }
    void mark() { if (dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_release); }
};
template <typename K>
static inline int axt_max_dynamic_lds(K kernel, int bytes, AxtOncePerDevice &once)
{
    if (!once.pending()) return AXT_OK;
    AXT_CHECK_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    once.mark();
    return AXT_OK;
}

// the kept tiles of a frame (tile row, tile column), passed to the kernels by value
struct TileList { int n; short yx[2 * 256]; };

// the last tile row (column) that begins inside a frame of `extent` pixels; -1: no tile does
static inline int axt_last_tile(int extent, int tile) { return extent >= 1 ? (extent - 1) / tile : -1; }

// The TileList of an entry point `fn` from its host array h_tile_yx [n_tiles][2]. AXT_EINVAL for n_tiles outside 1..256
// and for a row index outside 0..max_ty or a column index outside 0..max_tx; both limits are capped at 32767, what the
// short holds. The index itself is compared, never a product of it, so no index can wrap its way past the check.
static inline int axt_tile_list(const char *fn, const int32_t *h_tile_yx, int n_tiles, int max_ty, int max_tx, TileList *tl)
{
    AXT_REQUIRE(n_tiles >= 1 && n_tiles <= 256, "%s: n_tiles %d out of range [1,256]", fn, n_tiles);
    if (max_ty > 32767) max_ty = 32767;
    if (max_tx > 32767) max_tx = 32767;
    tl->n = n_tiles;
    for (int k = 0; k < n_tiles; ++k) {
        const int ty = h_tile_yx[2 * k], tx = h_tile_yx[2 * k + 1];
        AXT_REQUIRE(ty >= 0 && ty <= max_ty && tx >= 0 && tx <= max_tx, "%s: tile %d (%d,%d) outside rows 0..%d, columns 0..%d", fn, k,
                    ty, tx, max_ty, max_tx);
        tl->yx[2 * k] = (short)ty;
        tl->yx[2 * k + 1] = (short)tx;
    }
    return AXT_OK;
}

// cnn_front.hip: conv blocks 0 + 1 in one launch: frames -> block 1's output [B,40,128,128]
int axt_launch_conv_fused01(const float *in, const float *w0, const float *b0, const float *w1, const float *b1, float *out,
                            int B, hipStream_t st, int Hf, int Wf, int t0, int tstep, int item0, int n_tiles, const TileList &tl);
