// Stand-alone host program for tests/test_tiff_deflate_cpu.py::test_deflate_core_on_the_host (and the source of the
// streams tests/test_tiff_deflate_gpu.py compares the kernel's with): the deflate core of csrc/tiff_deflate.h, the very
// functions the kernel of csrc/tiff_deflate.hip runs, on the case file tests/tiff_deflate_cases.py writes. Built with
// -fsanitize=address,undefined. Every strip lives in a heap block of exactly its size, so a read one sample outside it
// ends the program; the slot, of axt_tiff_deflate_bound_bytes bytes, stands between two runs of guard bytes that are
// checked after the case. Every case is encoded twice (the streams must agree) and a third time into a slot one byte
// shorter than the stream, which must end as status 3 with the guards intact.
// Usage: tiff_deflate_host <case file> <result file>. The result file: per case int32 status, int64 length, int64 batches,
// the stream. Exit status 0 = no case failed these checks; whether the streams inflate to the strips is Python's to check.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tiff_deflate.h"

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) {
        perror(argv[1]);
        return 2;
    }
    const size_t guard = 64;
    int failures = 0;
    int32_t n_cases = 0;
    if (!get(f, &n_cases, 4)) return 2;
    axt_tiff_deflate_work *work = (axt_tiff_deflate_work *)malloc(sizeof(axt_tiff_deflate_work));
    if (!work) return 2;
    for (int c = 0; c < n_cases; ++c) {
        int32_t h[3];
        if (!get(f, h, sizeof h)) return 2;
        const int predictor = h[0], rows = h[1], W = h[2];
        const size_t samples = (size_t)rows * W;
        const int64_t bound = axt_tiff_deflate_bound_bytes((int64_t)samples * 2);
        uint16_t *in = (uint16_t *)malloc(samples ? samples * 2 : 1);
        uint8_t *block[3];
        for (int k = 0; k < 3; ++k) block[k] = (uint8_t *)malloc((size_t)bound + 2 * guard);
        if (!in || !block[0] || !block[1] || !block[2] || !get(f, in, samples * 2)) return 2;
        int64_t bytes[3] = {-1, -1, -1}, batches = 0;
        int status[3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            memset(block[k], 0xa5, (size_t)bound + 2 * guard);
            memset(work, k == 1 ? 0x00 : 0xff, sizeof *work);     // nothing of an earlier case, no zeros to lean on
            const int64_t cap = k < 2 ? bound : bytes[0] - 1;
            status[k] = axt_tiff_deflate_segment(in, rows, W, predictor, block[k] + guard, cap, *work, 0, 1, &bytes[k], k == 0 ? &batches : nullptr);
            for (size_t q = 0; q < guard; ++q) ok = ok && block[k][q] == 0xa5 && block[k][guard + (size_t)cap + q] == 0xa5;
        }
        ok = ok && status[0] == 0 && status[1] == 0 && bytes[0] == bytes[1] && bytes[0] <= bound && bytes[0] >= 8;
        ok = ok && memcmp(block[0] + guard, block[1] + guard, (size_t)bytes[0]) == 0;
        ok = ok && status[2] == AXT_TIFF_OVERRUN && bytes[2] == 0;
        ok = ok && batches <= axt_tiff_deflate_max_batches((int64_t)samples * 2);
        const int32_t st = status[0];
        if (fwrite(&st, 4, 1, g) != 1 || fwrite(&bytes[0], 8, 1, g) != 1 || fwrite(&batches, 8, 1, g) != 1) return 2;
        if (bytes[0] > 0 && fwrite(block[0] + guard, 1, (size_t)bytes[0], g) != (size_t)bytes[0]) return 2;
        printf("case %d: predictor %d rows %d W %d: status %d %d %d, %lld bytes of at most %lld, %lld batches of %lld: %s\n", c, predictor,
               rows, W, status[0], status[1], status[2], (long long)bytes[0], (long long)bound, (long long)batches,
               (long long)axt_tiff_deflate_max_batches((int64_t)samples * 2), ok ? "ok" : "FAILED");
        failures += !ok;
        free(in);
        for (int k = 0; k < 3; ++k) free(block[k]);
    }
    free(work);
    fclose(f);
    fclose(g);
    printf("%d cases, %d failures\n", n_cases, failures);
    return failures ? 1 : 0;
}
