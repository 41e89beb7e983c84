// A mixture of C correlated normals on dim columns of x and an optional table of scipy factors on others
// (pocomc_amd/prior.py: GaussianMixturePrior, and the mixture blocks of JointPrior):
//   log p(x) = start + log sum_c w_c N(x_cols; mean_c, cov_c),   start = base[r], the table's sum, or nothing.
// Per component the arithmetic is gauss_prior.hip's (g_c = -0.5 |Linv_c (x - mean_c)|^2 - logc_c, the same order, the same
// bits); the components are closed by a two-pass log-sum-exp in c order.  One launch, float64 VALU, one pass over x.  The
// order of every addition is fixed (include/pocomc_amd.h, tests/gauss_mix_model.py) and nothing is contracted into an FMA:
// the t_c = g_c + logw_c of a row are the numpy model's bits, and the value differs from the model's by what exp and log
// differ by.
#include "gauss_body.h"
#include "prior_body.h"

#pragma clang fp contract(off)

// What the kernel takes of the host's pmc_gauss_mix_t: everything by value.
struct GaussMixArgs {
    const int32_t* cols;
    const double* logw;
    const double* mean;
    const double* linv;
    const double* logc;
    int32_t n_comp;
    int32_t dim;
    int32_t D;
    int32_t Dr;                                    // 0: no table
    pmc_prior_t rest;
    const int32_t* rest_cols;
};

// The x tile, the work tile, the t_c of every component and row, one flag per row:
// 64 (D | 1) 8 + 64 (dim | 1) 8 + 64 n_comp 8 + 256 bytes; 80384 + 33280 + 16384 + 256 = 130304 at D = 157, dim = 64, C = 32.
static inline size_t gauss_mix_lds_bytes(int D, int dim, int n_comp) {
    return ((size_t)FP_ROWS * (D | 1) + (size_t)FP_ROWS * (dim | 1) + (size_t)FP_ROWS * n_comp) * sizeof(double)
           + FP_ROWS * sizeof(int);
}

// gauss_blocks_kernel's tile, stride contract and thread mapping (lane = row of the tile, wavefront w = tid / 64 picks the
// column or the row of Linv; every constant sits at an address the wavefront shares and is read with scalar loads).  The x
// tile T stays as it was read across the component loop -- only the table's columns, which no component reads, become
// their factors' terms -- and the components take turns on a work tile W[64][dim | 1]:
//   0. every table column's x becomes its factor's term; a row with a block or table x that is not finite or a table term
//      that is NaN is marked in rowin, and so are the rows of a tile with a column outside [0, D), which is not followed.
//   per component c = 0 .. C - 1 (mean_c, Linv_c, logc_c, logw_c at c's offset into the descriptor's arrays):
//   1. W[r][j] = d_j = x[cols[j]] - mean_c[j].
//   2. i from dim - 1 down in steps of 8 * GP_ACC: wavefront w forms y_i of i = top - GP_ACC w - u in ONE walk over
//      d_0 .. d_i, y_i = ((0.0 + Linv[i,0] d_0) + Linv[i,1] d_1) + ...; behind a barrier y_i * y_i replaces d_i (y_i reads d_j
//      with j <= i only, and every later step forms smaller i: one barrier per step is enough).
//   3. one lane per row: q = ((0.0 + y_0 y_0) + y_1 y_1) + ..., g = -0.5 q - logc_c, t_c = g + logw_c (-inf where g is NaN
//      or -inf) into S[c][r].
//   4. one lane per row: m = max_c t_c; all -inf: the row is -inf and no difference is formed; else
//      s = ((0.0 + exp(t_0 - m)) + exp(t_1 - m)) + ..., v = m + log(s), logp = start + v.
// The bits of a row depend on its values alone.  Every barrier is reached by every thread: the trip counts depend on the
// descriptor alone.
//   Measured at 1e4 rows x 32 columns, dim = 24, C = 8 (profiles/gauss_mix_prior.txt): 25.6 us per call where one component
//   through gauss_blocks_kernel takes 13.3, about 1.5 us per component -- four barriers and one walk whose scalar loads of
//   Linv_c start behind a barrier, so the components' load latencies do not overlap (read from the code: the parts have not
//   been timed separately).  Keeping each wavefront's tile columns
//   in registers across the components (instead of reading cols once per component) measured 26.4 us: not kept.  Giving each
//   wavefront components of its own (no barrier between components, no work tile) has not been measured.
__global__ __launch_bounds__(FP_THREADS) void gauss_mix_kernel(GaussMixArgs a, const double* __restrict__ x,
                                                               int64_t row_stride, int64_t col_stride, int64_t n,
                                                               const double* base, double* logp) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int C = a.n_comp, k = a.dim, D = a.D, Dr = a.Dr, LD = D | 1, LW = k | 1;
    double* T = sm;                                                       // [FP_ROWS][LD]
    double* W = T + (size_t)FP_ROWS * LD;                                 // [FP_ROWS][LW]
    double* S = W + (size_t)FP_ROWS * LW;                                 // [C][FP_ROWS]
    int* rowin = reinterpret_cast<int*>(S + (size_t)FP_ROWS * C);         // [FP_ROWS]
    const int tid = threadIdx.x;
    const int r = tid & (FP_ROWS - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / FP_ROWS);
    const int64_t row0 = (int64_t)blockIdx.x * FP_ROWS;
    const int rows = (int)min((int64_t)FP_ROWS, n - row0);
    const gp_i32 cols = (gp_i32)a.cols;
    if (tid < FP_ROWS) rowin[tid] = 1;
    gauss_load_tile(T, x, row_stride, col_stride, row0, rows, D, LD, tid);
    __syncthreads();
    double* Tr = T + r * LD;
    double* Wr = W + r * LW;
    const bool live = r < rows;
    // 0. the table's terms, and the rows no component has a value for
    for (int j = w; j < k; j += GP_WAVES) {
        const int c = cols[j];
        const bool col_ok = (unsigned)c < (unsigned)D;
        if (!live) continue;
        if (!col_ok || !isfinite(Tr[c])) rowin[r] = 0;
    }
    for (int m = w; m < Dr; m += GP_WAVES) {
        const int c = a.rest_cols[m];
        const bool col_ok = (unsigned)c < (unsigned)D;
        if (!live) continue;
        if (!col_ok) { rowin[r] = 0; continue; }
        const double xv = Tr[c];
        const double term = prior_term_any(a.rest, m, xv);
        Tr[c] = term;
        if (!isfinite(xv) || isnan(term)) rowin[r] = 0;
    }
    const int tri = k * (k + 1) / 2;
    for (int cc = 0; cc < C; ++cc) {
        const gp_f64 mean = (gp_f64)a.mean + (int64_t)cc * k;
        const gp_f64 linv = (gp_f64)a.linv + (int64_t)cc * tri;
        // 1. d = x - mean_c
        if (live) {
            for (int j = w; j < k; j += GP_WAVES) Wr[j] = Tr[gauss_col(cols, j, D)] - mean[j];
        }
        __syncthreads();
        // 2. y = Linv_c d, from the last rows of Linv up
        for (int top = k - 1; top >= 0; top -= GP_WAVES * GP_ACC) {
            int iu[GP_ACC];
            gp_f64 Lu[GP_ACC];
            double y[GP_ACC];
#pragma unroll
            for (int u = 0; u < GP_ACC; ++u) {
                iu[u] = top - GP_ACC * w - u;                                 // (below 0: nothing to form)
                const int i = max(iu[u], 0);
                Lu[u] = linv + (i * (i + 1)) / 2;
                y[u] = 0.0;
            }
            if (live) {
                // four d at a time while every y_i of the lane still takes them, then the ragged end; the order of a y_i's
                // additions is j = 0, 1, ..., i either way
                int j = 0;
                for (; j + 3 <= iu[GP_ACC - 1]; j += 4) {
                    const double d0 = Wr[j], d1 = Wr[j + 1], d2 = Wr[j + 2], d3 = Wr[j + 3];
#pragma unroll
                    for (int u = 0; u < GP_ACC; ++u) {
                        gp_f64 L = Lu[u] + j;
                        y[u] = (((y[u] + L[0] * d0) + L[1] * d1) + L[2] * d2) + L[3] * d3;
                    }
                }
                for (; j <= iu[0]; ++j) {
                    const double d = Wr[j];
#pragma unroll
                    for (int u = 0; u < GP_ACC; ++u)
                        if (j <= iu[u]) y[u] = y[u] + Lu[u][j] * d;
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int u = 0; u < GP_ACC; ++u)
                    if (iu[u] >= 0) Wr[iu[u]] = y[u] * y[u];
            }
        }
        __syncthreads();
        // 3. t_c
        if (tid < rows) {
            double q = 0.0;
            for (int i = 0; i < k; ++i) q += Wr[i];
            const double g = -0.5 * q - ((gp_f64)a.logc)[cc];
            const double t = g + ((gp_f64)a.logw)[cc];
            S[cc * FP_ROWS + tid] = (isnan(g) || g == -INFINITY) ? -INFINITY : t;
        }
        __syncthreads();                                                      // (the next component writes W)
    }
    // 4. the log-sum-exp and the row's value
    if (tid < rows) {
        double m = -INFINITY;
        for (int cc = 0; cc < C; ++cc) {
            const double t = S[cc * FP_ROWS + tid];
            m = t > m ? t : m;
        }
        double v = -INFINITY;
        if (m != -INFINITY) {
            double s = 0.0;
            for (int cc = 0; cc < C; ++cc) s = s + exp(S[cc * FP_ROWS + tid] - m);
            v = m + log(s);
        }
        if (base) {
            v = base[row0 + tid] + v;
        } else if (Dr > 0) {
            double lp = 0.0;
            for (int mm = 0; mm < Dr; ++mm) lp += Tr[gauss_col((gp_i32)a.rest_cols, mm, D)];
            v = lp + v;
        }
        logp[row0 + tid] = (rowin[tid] && isfinite(v)) ? v : -INFINITY;
    }
}

extern "C" int pmc_gauss_mix_logpdf(const pmc_gauss_mix_t* g, const double* x, int64_t row_stride, int64_t col_stride,
                                    int64_t n, const double* base, double* logp, void* stream) {
#define GM_FAIL(text) return pmc_fail("pmc_gauss_mix_logpdf: " text)
    if (!g) GM_FAIL("bad descriptor");
    if (!g->cols || !g->logw || !g->mean || !g->linv || !g->logc) GM_FAIL("bad mixture descriptor (a NULL array)");
    if (g->n_comp < 1 || g->n_comp > PMC_GAUSS_MIX_MAX_COMPONENTS) GM_FAIL("n_comp must lie in 1 .. 32");
    if (g->dim < 1 || g->dim > PMC_GAUSS_MIX_MAX_DIM) GM_FAIL("dim must lie in 1 .. 64");
    if (g->D > FP_MAX_D) GM_FAIL("n_dim too large (D <= 157)");
    const pmc_prior_t* rest = g->rest;
    if ((rest == nullptr) != (g->rest_cols == nullptr)) GM_FAIL("rest and rest_cols go together (both, or both NULL)");
    if (rest && (!rest->family || !rest->loc || !rest->scale || rest->n_extended < 0 || rest->D < 1))
        GM_FAIL("bad prior descriptor");
    const int64_t Dr = rest ? rest->D : 0;
    if ((int64_t)g->dim + Dr > g->D) GM_FAIL("the mixture and the rest have more columns than x (D)");
    if (rest && rest->n_extended > 0 && !rest->par)
        GM_FAIL("factors other than uniform / normal need the parameter table (par)");
    if (base && rest) GM_FAIL("base and rest exclude each other");
    if (n == 0) return 0;
    if (!x || !logp) GM_FAIL("bad argument (a NULL x or logp)");
    if (n < 0 || row_stride < 0 || col_stride < 0) GM_FAIL("bad argument (a negative count or stride)");
    if ((n + FP_ROWS - 1) / FP_ROWS > 0x7fffffffLL) GM_FAIL("too many rows for one launch");
#undef GM_FAIL
    GaussMixArgs a = {};
    a.cols = g->cols;
    a.logw = g->logw;
    a.mean = g->mean;
    a.linv = g->linv;
    a.logc = g->logc;
    a.n_comp = g->n_comp;
    a.dim = g->dim;
    a.D = g->D;
    a.Dr = (int32_t)Dr;
    if (rest) a.rest = *rest;
    a.rest_cols = g->rest_cols;
    const size_t lds = gauss_mix_lds_bytes(g->D, g->dim, g->n_comp);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gauss_mix_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(gauss_mix_kernel)");
    }
    const dim3 grid((unsigned)((n + FP_ROWS - 1) / FP_ROWS)), block(FP_THREADS);
    hipLaunchKernelGGL(gauss_mix_kernel, grid, block, lds, (hipStream_t)stream, a, x, row_stride, col_stride, n, base, logp);
    return pmc_check_launch("gauss_mix_kernel");
}
