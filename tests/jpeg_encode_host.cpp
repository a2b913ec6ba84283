// Stand-alone host program for tests/test_jpeg_cpu.py::test_encoder_core_on_the_host: the encoder's arithmetic of
// csrc/jpeg_encode.h, the very functions the kernels of csrc/jpeg.hip run, on the case file tests/jpeg_cases.py writes.
// Built with -fsanitize=address,undefined; the pixels and the output of every frame live in heap blocks of exactly their
// size, so a read or a write one byte outside ends the program. Every frame is encoded twice: into a block of exactly
// the expected length (the bytes must equal the reference's), and into one a byte shorter (the count must still be
// right, and nothing may be written past the end). Usage: jpeg_encode_host <case file>. Exit status 0 = no failure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpeg_encode.h"

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s <case file>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    int failures = 0, frames = 0;
    int32_t n_cases = 0;
    if (!get(f, &n_cases, 4)) return 2;
    for (int c = 0; c < n_cases; ++c) {
        int32_t h[4];
        if (!get(f, h, sizeof h)) return 2;
        const int n_frames = h[0], H = h[1], W = h[2], quality = h[3];
        for (int k = 0; k < n_frames; ++k, ++frames) {
            const size_t px = (size_t)3 * H * W;
            int64_t want_len = 0;
            uint8_t *rgb = (uint8_t *)malloc(px);
            if (!rgb || !get(f, rgb, px) || !get(f, &want_len, 8)) return 2;
            uint8_t *want = (uint8_t *)malloc(want_len ? (size_t)want_len : 1);
            uint8_t *out = (uint8_t *)malloc(want_len ? (size_t)want_len : 1);
            uint8_t *tight = (uint8_t *)malloc(want_len > 1 ? (size_t)want_len - 1 : 1);
            if (!want || !out || !tight || !get(f, want, (size_t)want_len)) return 2;
            const int64_t n = axt_jpeg_encode_frame_serial(rgb, H, W, quality, out, want_len);
            const int64_t n_tight = axt_jpeg_encode_frame_serial(rgb, H, W, quality, tight, want_len - 1);
            const bool ok = n == want_len && n_tight == want_len && memcmp(out, want, (size_t)want_len) == 0 &&
                            n <= axt_jpeg_scan_bound_hw(H, W);
            printf("case %d frame %d: %d x %d quality %d: %lld bytes, expected %lld: %s\n", c, k, H, W, quality, (long long)n,
                   (long long)want_len, ok ? "ok" : "FAILED");
            failures += !ok;
            free(rgb), free(want), free(out), free(tight);
        }
    }
    fclose(f);
    printf("%d cases, %d frames, %d failures\n", n_cases, frames, failures);
    return failures ? 1 : 0;
}
