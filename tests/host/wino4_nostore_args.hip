// Stand-alone host check of the y == NULL contract of the pooled F(4x4,3x3) forward (include/vaecap.h): links the HOST code of
// csrc/conv_wino4.hip -- argument checks, planners, the image-range loop -- and calls the entries with y == NULL and arguments that
// fail validation BEFORE any launch, so it needs no GPU; built with -fsanitize=address,undefined on the host side and run on the CPU
// (make -C vae_captioning_amd/csrc wino4-hostcheck).  Nothing here touches a device: every call must return VC_EINVAL.
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
    if (rc != want) {
        ++failures;
        fprintf(stderr, "FAIL %s: returned %d, expected %d (%s)\n", what, rc, want, vc::last_error_buf());
    } else {
        printf("ok   %-78s -> %d  %s\n", what, rc, rc ? vc::last_error_buf() : "");
    }
    vc::last_error_buf()[0] = 0;
}

int main() {
    const int EINVAL_ = 10001;   // VC_EINVAL (csrc/common.h)
    // never dereferenced: validation fails first.  16-byte aligned host blocks stand in for device pointers
    float* x = (float*)aligned_alloc(16, 64);
    float* wp = (float*)aligned_alloc(16, 64);
    float* pool = (float*)aligned_alloc(16, 64);
    float* vws = (float*)aligned_alloc(16, 64);
    uint32_t* codes = (uint32_t*)aligned_alloc(16, 64);
    // y == NULL and no pooled tensor: nothing to leave
    expect("wino4_fwd_pool: y == NULL && ypool == NULL", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 2, 16, 16, 64, 32, x, wp, nullptr, nullptr, nullptr, codes), EINVAL_);
    expect("wino4v_fwd_pool: y == NULL && ypool == NULL", vc_conv3x3_wino4v_fwd_pool_f32(nullptr, 2, 16, 16, 64, 32, x, wp, nullptr, nullptr, nullptr, codes, vws, 64), EINVAL_);
    expect("wino4_fwd: y == NULL && ypool == NULL", vc_conv3x3_wino4_fwd_f32(nullptr, 2, 16, 16, 64, 32, x, wp, nullptr, nullptr, nullptr, 1), EINVAL_);
    expect("wino4v_fwd: y == NULL && ypool == NULL", vc_conv3x3_wino4v_fwd_f32(nullptr, 2, 16, 16, 64, 32, x, wp, nullptr, nullptr, nullptr, 1, vws, 64), EINVAL_);
    // y == NULL with a pooled tensor, but the codes missing (this entry requires them)
    expect("wino4_fwd_pool: y == NULL, pool_bits == NULL", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 2, 16, 16, 64, 32, x, wp, nullptr, nullptr, pool, nullptr), EINVAL_);
    // y == NULL, everything else present, shapes the planner refuses: channels, odd sizes, a call no launch can address
    expect("wino4_fwd_pool: y == NULL, Cout % 32 != 0", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 2, 16, 16, 64, 48, x, wp, nullptr, nullptr, pool, codes), EINVAL_);
    expect("wino4_fwd_pool: y == NULL, Cin % 8 != 0", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 2, 16, 16, 4, 64, x, wp, nullptr, nullptr, pool, codes), EINVAL_);
    expect("wino4_fwd_pool: y == NULL, odd H", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 2, 15, 16, 64, 32, x, wp, nullptr, nullptr, pool, codes), EINVAL_);
    expect("wino4_fwd_pool: y == NULL, B == 0", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 0, 16, 16, 64, 32, x, wp, nullptr, nullptr, pool, codes), EINVAL_);
    expect("wino4_fwd_pool: y == NULL, H < 4", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 2, 2, 2, 64, 32, x, wp, nullptr, nullptr, pool, codes), EINVAL_);
    expect("wino4_fwd_pool: y == NULL, one image over 2 GiB", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 1, 4096, 4096, 64, 64, x, wp, nullptr, nullptr, pool, codes), EINVAL_);
    expect("wino4_fwd_pool: y == NULL, misaligned ypool", vc_conv3x3_wino4_fwd_pool_f32(nullptr, 2, 16, 16, 64, 32, x, wp, nullptr, nullptr, pool + 1, codes), EINVAL_);
    expect("wino4v_fwd_pool: y == NULL, square-block shape (32 wide)", vc_conv3x3_wino4v_fwd_pool_f32(nullptr, 2, 32, 32, 64, 96, x, wp, nullptr, nullptr, pool, codes, vws, 1 << 30), EINVAL_);
    expect("wino4v_fwd_pool: y == NULL, workspace too small", vc_conv3x3_wino4v_fwd_pool_f32(nullptr, 3, 28, 28, 64, 64, x, wp, nullptr, nullptr, pool, codes, vws, 64), EINVAL_);
    expect("wino4v_fwd_pool: y == NULL, workspace missing", vc_conv3x3_wino4v_fwd_pool_f32(nullptr, 3, 28, 28, 64, 64, x, wp, nullptr, nullptr, pool, codes, nullptr, 1 << 30), EINVAL_);
    expect("wino4v_fwd_pool: y == NULL, odd W", vc_conv3x3_wino4v_fwd_pool_f32(nullptr, 3, 28, 27, 64, 64, x, wp, nullptr, nullptr, pool, codes, vws, 1 << 30), EINVAL_);
    // the host-only queries the callers plan with
    expect("wino4_supported(3, 28, 28, 64, 64)", vc_conv3x3_wino4_supported(3, 28, 28, 64, 64, 0), 1);
    expect("wino4v_supported(2, 32, 32, 64, 96)", vc_conv3x3_wino4v_supported(2, 32, 32, 64, 96, 0), 0);
    expect("wino4v_workspace_bytes(3, 28, 28, 64) == 10 blocks x 64 x 2304", (int)vc_conv3x3_wino4v_workspace_bytes(3, 28, 28, 64), 10 * 64 * 2304);
    free(x); free(wp); free(pool); free(vws); free(codes);
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("wino4 no-store argument checks: all passed\n");
    return 0;
}
