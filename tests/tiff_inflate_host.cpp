// Stand-alone host program for tests/test_tiff_inflate_cpu.py::test_inflate_core_on_the_host: the inflate core of
// csrc/tiff_inflate.h, the very functions the kernel of csrc/tiff_inflate.hip runs, on the case file
// tests/tiff_inflate_cases.py writes. Built with -fsanitize=address,undefined. The input of every case lives in a heap
// block of exactly its size, so a read one byte outside it ends the program; the output stands between two runs of guard
// bytes that are checked after the case. Usage: tiff_inflate_host <case file>. Exit status 0 = every case gave the
// expected status and, where that is 0, the expected samples, within axt_tiff_inflate_max_steps steps, guards intact.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tiff_inflate.h"

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
    const size_t guard = 64;                                  // samples on either side of the output
    int failures = 0;
    int32_t n_cases = 0;
    if (!get(f, &n_cases, 4)) return 2;
    axt_tiff_inflate_tables *tables = (axt_tiff_inflate_tables *)malloc(sizeof(axt_tiff_inflate_tables));
    if (!tables) return 2;
    for (int c = 0; c < n_cases; ++c) {
        int32_t h[5];
        int64_t src_bytes = 0;
        if (!get(f, h, sizeof h) || !get(f, &src_bytes, 8)) return 2;
        const int predictor = h[0], big_endian = h[1], rows = h[2], W = h[3], expected = h[4];
        const size_t samples = (size_t)rows * W;
        uint8_t *src = (uint8_t *)malloc(src_bytes ? (size_t)src_bytes : 1);
        uint16_t *block = (uint16_t *)malloc((samples + 2 * guard) * 2);
        uint16_t *want = (uint16_t *)malloc(samples ? samples * 2 : 1);
        if (!src || !block || !want || !get(f, src, (size_t)src_bytes)) return 2;
        if (expected == 0 && !get(f, want, samples * 2)) return 2;
        memset(block, 0xa5, (samples + 2 * guard) * 2);
        memset(tables, 0xff, sizeof *tables);                 // nothing of an earlier case, no zeros to lean on
        uint16_t *out = block + guard;
        int64_t steps = 0;
        int status = axt_tiff_check_segment(0, src_bytes, 0, rows, W, src_bytes, (int64_t)samples);
        if (status == AXT_TIFF_OK)
            status = axt_tiff_inflate_segment_serial(src, src_bytes, rows, W, predictor, big_endian, out, *tables, &steps);
        bool ok = status == expected && steps <= axt_tiff_inflate_max_steps(src_bytes);
        if (ok && expected == 0) ok = memcmp(out, want, samples * 2) == 0;
        for (size_t g = 0; g < guard; ++g) ok = ok && block[g] == 0xa5a5 && block[guard + samples + g] == 0xa5a5;
        printf("case %d: predictor %d big_endian %d rows %d W %d src_bytes %lld: status %d, expected %d, %lld steps of %lld: %s\n", c,
               predictor, big_endian, rows, W, (long long)src_bytes, status, expected, (long long)steps,
               (long long)axt_tiff_inflate_max_steps(src_bytes), ok ? "ok" : "FAILED");
        failures += !ok;
        free(src), free(block), free(want);
    }
    free(tables);
    fclose(f);
    printf("%d cases, %d failures\n", n_cases, failures);
    return failures ? 1 : 0;
}
