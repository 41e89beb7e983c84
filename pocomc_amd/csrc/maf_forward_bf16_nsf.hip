// The spline instances of the bf16 matrix-core forward kernel (maf_forward_bf16.h): neural spline flows of 4, 8 and 16
// bins (n_out = 3 K - 1 = 11, 23, 47), reached through pmc_maf_forward_bf16.  A translation unit of their own: thirteen
// instances (five launch shapes x three bin counts, less the two sixteen-wave shapes of 16 bins, which would spill) compile
// next to the affine ones instead of behind them; the Makefile checks the compiler's remarks: none uses scratch.
#include "maf_forward_bf16.h"

int pmc_launch_forward_bf16_nsf(const pmc_maf_t* m, const uint16_t* image, int64_t per_t, const float* x, float* z, float* ladj,
                                float* log_prob, int64_t n, const int64_t* idx, hipStream_t st) {
    if (m->n_out == RQS_NOUT_OF(8)) return dispatch_fwd_bf16<8>(m, image, per_t, x, z, ladj, log_prob, n, idx, st);
    if (m->n_out == RQS_NOUT_OF(4)) return dispatch_fwd_bf16<4>(m, image, per_t, x, z, ladj, log_prob, n, idx, st);
    if (m->n_out == RQS_NOUT_OF(16)) return dispatch_fwd_bf16<16>(m, image, per_t, x, z, ladj, log_prob, n, idx, st);
    return pmc_fail("pmc_maf_forward_bf16: spline flows are built for 4, 8 or 16 bins");
}
