// Stand-alone host check of vc_gauss_mix_lse_f64's argument contract (include/vaecap.h): links the HOST code of csrc/latent_mi.hip and
// calls the entry with every invalid argument combination and with N == 0, all of which return BEFORE any launch, so it needs no GPU;
// built with -fsanitize=address,undefined on the host side and run on the CPU (make -C vae_captioning_amd/csrc mi-hostcheck).
// Nothing here touches a device: the pointers are host blocks that are never dereferenced.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vaecap.h"

namespace vc {
char* last_error_buf() {   // (api.hip's, which is not linked here)
    static thread_local char buf[512];
    return buf;
}
}  // namespace vc

static int failures = 0;
static void expect(const char* what, int rc, int want) {
    const char* msg = vc::last_error_buf();
    const bool text_ok = want == 0 ? msg[0] == 0 : strstr(msg, "vc_gauss_mix_lse_f64: invalid argument") != nullptr;
    if (rc != want || !text_ok) {
        ++failures;
        fprintf(stderr, "FAIL %s: returned %d, expected %d (%s)\n", what, rc, want, msg);
    } else {
        printf("ok   %-58s -> %d  %s\n", what, rc, msg);
    }
    vc::last_error_buf()[0] = 0;
}

int main() {
    const int EINVAL_ = 10001;   // VC_EINVAL (csrc/common.h)
    float* z = (float*)aligned_alloc(16, 64);
    float* mean = (float*)aligned_alloc(16, 64);
    float* std_ = (float*)aligned_alloc(16, 64);
    double* blk = (double*)aligned_alloc(16, 64);
    double* full = (double*)aligned_alloc(16, 64);
    auto call = [&](long N, long M, int S, int L, const float* a, const float* b, const float* c, double* d, double* e) {
        return vc_gauss_mix_lse_f64(nullptr, N, M, S, L, a, b, c, d, e);
    };
    // N == 0: a successful no-op, whatever else is passed -- no pointer and no other size is looked at
    expect("N == 0", call(0, 4, 2, 3, z, mean, std_, blk, full), 0);
    expect("N == 0, every pointer null", call(0, 4, 2, 3, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
    expect("N == 0, M == S == L == 0", call(0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
    // sizes
    expect("N < 0", call(-1, 4, 2, 3, z, mean, std_, blk, full), EINVAL_);
    expect("N < 0, every pointer null", call(-5, 4, 2, 3, nullptr, nullptr, nullptr, nullptr, nullptr), EINVAL_);
    expect("M == 0", call(2, 0, 2, 3, z, mean, std_, blk, full), EINVAL_);
    expect("M < 0", call(2, -4, 2, 3, z, mean, std_, blk, full), EINVAL_);
    expect("S == 0", call(2, 4, 0, 3, z, mean, std_, blk, full), EINVAL_);
    expect("S < 0", call(2, 4, -2, 3, z, mean, std_, blk, full), EINVAL_);
    expect("L == 0", call(2, 4, 2, 0, z, mean, std_, blk, full), EINVAL_);
    expect("L < 0", call(2, 4, 2, -3, z, mean, std_, blk, full), EINVAL_);
    expect("S == 129: above the rows a workgroup keeps", call(2, 4, 129, 3, z, mean, std_, blk, full), EINVAL_);
    expect("S == INT32_MAX", call(2, 4, INT32_MAX, 3, z, mean, std_, blk, full), EINVAL_);
    expect("N == 2^31", call(1L << 31, 4, 2, 3, z, mean, std_, blk, full), EINVAL_);
    expect("M == 2^31", call(2, 1L << 31, 2, 3, z, mean, std_, blk, full), EINVAL_);
    // pointers, N > 0
    expect("z == NULL", call(2, 4, 2, 3, nullptr, mean, std_, blk, full), EINVAL_);
    expect("mean == NULL", call(2, 4, 2, 3, z, nullptr, std_, blk, full), EINVAL_);
    expect("std_ == NULL", call(2, 4, 2, 3, z, mean, nullptr, blk, full), EINVAL_);
    expect("lse_block == NULL", call(2, 4, 2, 3, z, mean, std_, nullptr, full), EINVAL_);
    expect("lse_full == NULL", call(2, 4, 2, 3, z, mean, std_, blk, nullptr), EINVAL_);
    expect("every pointer null", call(2, 4, 2, 3, nullptr, nullptr, nullptr, nullptr, nullptr), EINVAL_);
    free(z); free(mean); free(std_); free(blk); free(full);
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("gauss mix lse argument checks: all passed\n");
    return 0;
}
