// Host-side check of the stage-training entry points (axt_conv_trainer_input_grad, axt_maxpool2_forward, axt_maxpool2_backward)
// under AddressSanitizer and UndefinedBehaviorSanitizer: their argument checks and size arithmetic, which run before any
// device call, so the program needs no GPU and never reaches a launch. Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
//       profiles/experiments/asan_train_stage_args.cpp axtrack_amd/csrc/train_conv.hip axtrack_amd/csrc/api.cpp \
//       -o /tmp/asan_train_stage_args && /tmp/asan_train_stage_args
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "axtrack_hip.h"

static int failures = 0;

static void expect(int got, int want, const char *what, const char *in_message)
{
    const char *msg = axt_last_error();
    const bool ok = got == want && (!in_message || (msg && std::strstr(msg, in_message)));
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: returned %d (want %d), message \"%s\"\n", what, got, want, msg ? msg : "");
    }
}

int main()
{
    float buf[16] = {};
    float *p = buf;                                     // never dereferenced: every call below is refused, or has no maps
    const int EINVAL_ = -22;
    expect(axt_conv_trainer_input_grad(nullptr, p, 1, p, nullptr), EINVAL_, "input_grad(null trainer)", "null");
    const int sides[][2] = {{1, 2}, {2, 1}, {0, 4}, {-2, 4}, {4, -2}, {32769, 2}, {2, 32769}, {INT32_MAX, INT32_MAX},
                            {INT32_MIN, 2}};
    for (const auto &s : sides) {
        expect(axt_maxpool2_forward(p, 1, s[0], s[1], p, nullptr), EINVAL_, "maxpool2_forward(side)", "axt_maxpool2_forward");
        expect(axt_maxpool2_backward(p, p, 1, s[0], s[1], p, nullptr), EINVAL_, "maxpool2_backward(side)", "axt_maxpool2_backward");
    }
    // n_maps * H * W against 2^38, at the smallest and the largest map: one past the limit, and far past it
    const int64_t limit = (int64_t)1 << 38;
    const int hw[][2] = {{2, 2}, {32768, 32768}, {3, 5}};
    for (const auto &s : hw) {
        const int64_t most = limit / ((int64_t)s[0] * s[1]);
        for (int64_t n : {most + 1, (int64_t)-1, INT64_MAX, INT64_MIN}) {
            expect(axt_maxpool2_forward(p, n, s[0], s[1], p, nullptr), EINVAL_, "maxpool2_forward(n_maps)", "axt_maxpool2_forward");
            expect(axt_maxpool2_backward(p, p, n, s[0], s[1], p, nullptr), EINVAL_, "maxpool2_backward(n_maps)",
                   "axt_maxpool2_backward");
        }
        expect(axt_maxpool2_forward(p, 0, s[0], s[1], p, nullptr), 0, "maxpool2_forward(no maps)", nullptr);
        expect(axt_maxpool2_backward(p, p, 0, s[0], s[1], p, nullptr), 0, "maxpool2_backward(no maps)", nullptr);
    }
    expect(axt_maxpool2_forward(nullptr, 1, 2, 2, p, nullptr), EINVAL_, "maxpool2_forward(null in)", "null");
    expect(axt_maxpool2_forward(p, 1, 2, 2, nullptr, nullptr), EINVAL_, "maxpool2_forward(null out)", "null");
    expect(axt_maxpool2_backward(nullptr, p, 1, 2, 2, p, nullptr), EINVAL_, "maxpool2_backward(null in)", "null");
    expect(axt_maxpool2_backward(p, nullptr, 1, 2, 2, p, nullptr), EINVAL_, "maxpool2_backward(null dout)", "null");
    expect(axt_maxpool2_backward(p, p, 1, 2, 2, nullptr, nullptr), EINVAL_, "maxpool2_backward(null din)", "null");
    std::printf(failures ? "%d checks failed\n" : "all argument checks held (%d failures)\n", failures);
    return failures ? 1 : 0;
}
