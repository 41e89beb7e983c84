// A finished run's flow and scaler as a prior (pocomc_amd/prior.py: FlowPrior):
//   log p(x) = flow.log_prob(u(x)) - log|dx/du|,   u = Reparameterize.forward(x).
// Two launches around the flow's own forward kernel: flow_prior_pre_kernel maps the rows (u as float32 for the flow, the
// scaler's log-determinant, the support test), flow_prior_post_kernel joins the flow's float32 log-density with them.
#include "pmc_internal.h"
#include "flow_prior_body.h"

static inline size_t flow_prior_lds_bytes(int D) {
    return (size_t)FP_ROWS * (D | 1) * sizeof(double) + (size_t)FP_ROWS * D * sizeof(float) + FP_ROWS * sizeof(int);
}

// One block: 64 rows through LDS.  x is read with element strides: (row_stride, col_stride) = (1, n) -- the step's
// column-major view -- is walked rows first, everything else features first ((D, 1): the C-contiguous array), so that
// consecutive lanes read consecutive doubles in both.  A thread keeps ONE feature, as in scaler_inverse_kernel.  The
// tile's row length is odd (D | 1 doubles): the rows-first stores and the row sums (one lane per row) spread over the banks.
// The Jacobian term of an element replaces its x in the tile; a row's terms are added by one lane, j = 0, 1, ..., D - 1:
// the row's bits do not depend on the layout, on n or on the row's place in the block.
// Every barrier is reached by every thread: no branch around one depends on the data.
__global__ __launch_bounds__(FP_THREADS) void flow_prior_pre_kernel(
    pmc_scaler_t s, const double* __restrict__ x, int64_t row_stride, int64_t col_stride, int64_t n,
    float* __restrict__ u32, double* __restrict__ ldj, int32_t* __restrict__ inside) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int D = s.D, LD = D | 1;
    double* T = sm;                                                       // [FP_ROWS][LD]: x, then J
    float* U = reinterpret_cast<float*>(sm + (size_t)FP_ROWS * LD);       // [FP_ROWS][D]
    int* rowin = reinterpret_cast<int*>(U + (size_t)FP_ROWS * D);         // [FP_ROWS]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * FP_ROWS;
    const int rows = (int)min((int64_t)FP_ROWS, n - row0);
    if (tid < FP_ROWS) rowin[tid] = 1;
    const int rpp = FP_THREADS / D;                                       // (D <= 157 < FP_THREADS)
    const int r0 = tid / D, j = tid - r0 * D;
    const bool act = r0 < rpp;
    ScalerFeat f;
    if (act) scaler_feat_request(f, s, (const pmc_prior_un_t*)nullptr, j);
    if (col_stride == 1) {
        int r = tid / D, c = tid - r * D;                                 // element e = r * D + c, stepped without a division
        const int dr = FP_THREADS / D, dc = FP_THREADS - dr * D;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[r * LD + c] = x[(row0 + r) * row_stride + c];
            r += dr; c += dc;
            if (c >= D) { c -= D; ++r; }
        }
    } else {
        int c = tid / rows, r = tid - c * rows;                           // element e = c * rows + r
        const int dc = FP_THREADS / rows, dr = FP_THREADS - dc * rows;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[r * LD + c] = x[(row0 + r) * row_stride + (int64_t)c * col_stride];
            c += dc; r += dr;
            if (r >= rows) { r -= rows; ++c; }
        }
    }
    __syncthreads();
    if (act) {
        scaler_feat_finish(f, s, false);
        flow_prior_feature(f, s, T, U, rowin, r0, rpp, rows, j, j, D, LD);      // (a loop per kind: flow_prior_body.h)
    }
    __syncthreads();
    if (tid < rows) {
        const double* a = T + (size_t)tid * LD;
        double l = 0.0;
        for (int k = 0; k < D; ++k) l += a[k];
        if (s.scale) l = s.sum_log_sigma + l;
        ldj[row0 + tid] = l;
        inside[row0 + tid] = rowin[tid];
    }
    // the block's rows are one contiguous piece of u32; a row outside the support goes out as zeros
    float* out = u32 + row0 * D;
    {
        int r = tid / D, c = tid - r * D;
        const int dr = FP_THREADS / D, dc = FP_THREADS - dr * D;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            out[e] = rowin[r] ? U[e] : 0.0f;
            r += dr; c += dc;
            if (c >= D) { c -= D; ++r; }
        }
    }
}

__global__ __launch_bounds__(256) void flow_prior_post_kernel(const float* __restrict__ lp32, const double* __restrict__ ldj,
                                                              const int32_t* __restrict__ inside, double* __restrict__ logp,
                                                              int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    logp[r] = flow_prior_join(lp32[r], ldj[r], inside[r]);
}

extern "C" int pmc_flow_prior_pre(const pmc_scaler_t* s, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                                  float* u32, double* ldj, int32_t* inside, void* stream) {
    if (!s || !s->low || !s->high || !s->kind || !s->log_width || s->D < 1) return pmc_fail("pmc_flow_prior_pre: bad descriptor");
    if (s->scale && (!s->mu || !s->sigma)) return pmc_fail("pmc_flow_prior_pre: scale=1 needs mu and sigma");
    if (s->D > FP_MAX_D) return pmc_fail("pmc_flow_prior_pre: n_dim too large (D <= 157)");
    if (n == 0) return 0;
    if (!x || !u32 || !ldj || !inside || n < 0 || row_stride < 0 || col_stride < 0)
        return pmc_fail("pmc_flow_prior_pre: bad argument");
    if ((n + FP_ROWS - 1) / FP_ROWS > 0x7fffffffLL) return pmc_fail("pmc_flow_prior_pre: too many rows for one launch");
    const size_t lds = flow_prior_lds_bytes(s->D);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(flow_prior_pre_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(flow_prior_pre_kernel)");
    }
    hipLaunchKernelGGL(flow_prior_pre_kernel, dim3((unsigned)((n + FP_ROWS - 1) / FP_ROWS)), dim3(FP_THREADS), lds,
                       (hipStream_t)stream, *s, x, row_stride, col_stride, n, u32, ldj, inside);
    return pmc_check_launch("flow_prior_pre_kernel");
}

extern "C" int pmc_flow_prior_post(const float* lp32, const double* ldj, const int32_t* inside, double* logp, int64_t n,
                                   void* stream) {
    if (n == 0) return 0;
    if (!lp32 || !ldj || !inside || !logp || n < 0) return pmc_fail("pmc_flow_prior_post: bad argument");
    if ((n + 255) / 256 > 0x7fffffffLL) return pmc_fail("pmc_flow_prior_post: too many rows for one launch");
    hipLaunchKernelGGL(flow_prior_post_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       lp32, ldj, inside, logp, n);
    return pmc_check_launch("flow_prior_post_kernel");
}
