// Stand-alone host program for tests/test_tiff_cpu.py::test_decoder_core_on_the_host: the decoder core of csrc/tiff_decode.h,
// the very functions the kernels of csrc/tiff.hip run, on the case file tests/tiff_cases.py writes. Built with
// -fsanitize=address,undefined; input and output of every case live in heap blocks of exactly their size, so a read or a
// write one byte outside a segment ends the program. Usage: tiff_decode_host <case file>. Exit status 0 = every case
// gave the expected status and, where that is 0, the expected samples.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tiff_decode.h"

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
    int failures = 0;
    int32_t n_cases = 0;
    if (!get(f, &n_cases, 4)) return 2;
    std::vector<uint32_t> tbl_off(AXT_TIFF_LZW_ENTRIES);
    std::vector<uint16_t> tbl_len(AXT_TIFF_LZW_ENTRIES);
    for (int c = 0; c < n_cases; ++c) {
        int32_t h[6];
        int64_t src_bytes = 0;
        if (!get(f, h, sizeof h) || !get(f, &src_bytes, 8)) return 2;
        const int compression = h[0], predictor = h[1], big_endian = h[2], rows = h[3], W = h[4], expected = h[5];
        const size_t samples = (size_t)rows * W;
        // exact-size heap blocks (malloc(0) may be NULL: one byte then, with the length still passed as 0)
        uint8_t *src = (uint8_t *)malloc(src_bytes ? (size_t)src_bytes : 1);
        uint16_t *out = (uint16_t *)malloc(samples ? samples * 2 : 1);
        uint16_t *want = (uint16_t *)malloc(samples ? samples * 2 : 1);
        if (!src || !out || !want || !get(f, src, (size_t)src_bytes)) return 2;
        if (expected == 0 && !get(f, want, samples * 2)) return 2;
        memset(out, 0xa5, samples * 2);
        int status = axt_tiff_check_segment(0, src_bytes, 0, rows, W, src_bytes, (int64_t)samples);
        if (status == AXT_TIFF_OK)
            status = axt_tiff_decode_segment_serial(src, src_bytes, rows, W, compression, predictor, big_endian, out, tbl_off.data(),
                                                    tbl_len.data());
        bool ok = status == expected;
        if (ok && expected == 0) ok = memcmp(out, want, samples * 2) == 0;
        printf("case %d: compression %d predictor %d big_endian %d rows %d W %d src_bytes %lld: status %d, expected %d: %s\n", c,
               compression, predictor, big_endian, rows, W, (long long)src_bytes, status, expected, ok ? "ok" : "FAILED");
        failures += !ok;
        free(src), free(out), free(want);
    }
    int32_t n_desc = 0;
    if (!get(f, &n_desc, 4)) return 2;
    for (int c = 0; c < n_desc; ++c) {
        int64_t d[7];
        int32_t expected = 0;
        if (!get(f, d, sizeof d) || !get(f, &expected, 4)) return 2;
        const int status = axt_tiff_check_segment(d[0], d[1], d[2], (int32_t)d[3], (int)d[4], d[5], d[6]);
        const bool ok = status == expected;
        printf("descriptor %d: status %d, expected %d: %s\n", c, status, expected, ok ? "ok" : "FAILED");
        failures += !ok;
    }
    fclose(f);
    printf("%d cases, %d descriptors, %d failures\n", n_cases, n_desc, failures);
    return failures ? 1 : 0;
}
