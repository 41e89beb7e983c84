// Correlated normal blocks on some columns of x and an optional table of scipy factors on others (pocomc_amd/prior.py:
// GaussianPrior, and the Gaussian blocks of JointPrior):
//   log p(x) = start + sum_b [-0.5 |Linv_b (x_{C_b} - mean_b)|^2 - logc_b],   start = base[r], the table's sum, or nothing,
// Linv_b the inverse of the lower Cholesky factor of block b's covariance, packed by rows.  One launch, float64 VALU, one
// pass over x.  The order of every addition is fixed (include/pocomc_amd.h, tests/gauss_prior_model.py) and nothing is
// contracted into an FMA: a row's bits are those of the numpy model.
// With a box (TruncatedGaussianPrior, pmc_gauss_box_logpdf) a block's columns are also held to lo_j <= x_j <= hi_j: a row
// outside gets -inf, every other row keeps its bits (the caller has put the box's log mass into logc).
#include "gauss_body.h"
#include "prior_body.h"

#pragma clang fp contract(off)

// What the kernel takes of the host's pmc_gauss_blocks_t: everything by value.
struct GaussBlocksArgs {
    const int32_t* cols[PMC_GAUSS_BLOCKS_MAX];
    const double* mean[PMC_GAUSS_BLOCKS_MAX];
    const double* linv[PMC_GAUSS_BLOCKS_MAX];
    double logc[PMC_GAUSS_BLOCKS_MAX];
    int32_t dim[PMC_GAUSS_BLOCKS_MAX];
    int32_t n_blocks;
    int32_t D;
    int32_t Dr;                                    // 0: no table
    pmc_prior_t rest;
    const int32_t* rest_cols;
};
// The boxes of pmc_gauss_box_t, by value as well; a block without a box has a NULL pair.
struct GaussBoxArgs {
    const double* lo[PMC_GAUSS_BLOCKS_MAX];
    const double* hi[PMC_GAUSS_BLOCKS_MAX];
};

static inline size_t gauss_blocks_lds_bytes(int D) {
    return (size_t)FP_ROWS * (D | 1) * sizeof(double) + FP_ROWS * sizeof(int);
}

// Block bb's constants (read through the constant address space, gauss_body.h), picked in a chain of selects over constant
// indices (the kernel arguments are never indexed with a run-time value); bb is the same in every lane, so these stay scalars.
struct GaussBlock {
    gp_i32 cols;
    gp_f64 mean;
    gp_f64 linv;
    double logc;
    int k;
};
struct GaussBox {
    gp_f64 lo;
    gp_f64 hi;
};
__device__ __forceinline__ GaussBox gauss_box(const GaussBoxArgs& a, int bb) {
    GaussBox g = {(gp_f64)a.lo[0], (gp_f64)a.hi[0]};
#pragma unroll
    for (int b = 1; b < PMC_GAUSS_BLOCKS_MAX; ++b) {
        if (b == bb) {
            g.lo = (gp_f64)a.lo[b];
            g.hi = (gp_f64)a.hi[b];
        }
    }
    return g;
}
__device__ __forceinline__ GaussBlock gauss_block(const GaussBlocksArgs& a, int bb) {
    GaussBlock g = {(gp_i32)a.cols[0], (gp_f64)a.mean[0], (gp_f64)a.linv[0], a.logc[0], a.dim[0]};
#pragma unroll
    for (int b = 1; b < PMC_GAUSS_BLOCKS_MAX; ++b) {
        if (b == bb) {
            g.cols = (gp_i32)a.cols[b];
            g.mean = (gp_f64)a.mean[b];
            g.linv = (gp_f64)a.linv[b];
            g.logc = a.logc[b];
            g.k = a.dim[b];
        }
    }
    return g;
}

// joint_prior_pre_kernel's tile and stride contract (64 rows of all D columns through LDS, row length D | 1, the same two
// coalesced walks) with another thread mapping behind it: lane = row of the tile, wavefront w = tid / 64 picks the column,
// so that every constant -- a column index, a mean, an entry of Linv, a table factor's family -- sits at an address the
// whole wavefront shares, and the lanes of a wavefront walk the tile at an odd stride.
//   1. every block column's x becomes d = x - mean in place, every table column's x its factor's term; a row with an x
//      that is not finite or a table term that is NaN is marked in rowin.  BOX: so is a row with a block column's x outside
//      [lo_j, hi_j] (a NaN fails the test as written); lo and hi are read like mean, with scalar loads, and a block with a
//      NULL pair has no box.  The instance without BOX never looks at the box argument.
//   2. block after block, i from k - 1 down in steps of 8 * GP_ACC: wavefront w forms y_i of i = top - GP_ACC w - u,
//      u = 0 .. GP_ACC - 1, in ONE walk over d_0 .. d_i (each y_i = ((0.0 + Linv[i,0] d_0) + Linv[i,1] d_1) + ..., every
//      product and every sum rounded).  The lane's rows are neighbours: their walks end within three entries of each
//      other, so nearly all of a walk takes four d and sixteen entries of Linv at a time.  Behind a barrier y_i * y_i
//      replaces d_i.  y_i reads d_j with j <= i only, and every later step forms smaller i: what is overwritten is never
//      read again, so one barrier per step is enough.
//   Linv is read straight from global memory with scalar loads (the packed factor, 99 KB at k = 157, does not fit LDS next
//   to the tile).  Measured at 1e4 rows, us per call at k = 64 / 128 / 157: 27 / 67 / 92 with vector loads of one address
//   and rows 8 apart per lane, 21 / 45 / 59 with scalar loads, 14 / 33 / 44 with neighbouring rows as well (k <= 32: 13,
//   the launch itself).  A staging of Linv through LDS in row chunks has not been measured.
//   3. one lane per row adds the table's terms from 0.0 in factor order, then block after block's squares in i order:
//      q = ((0.0 + y_0 y_0) + y_1 y_1) + ..., g = -0.5 q - logc, v = start + g_0 + g_1 + ... left to right.
// The bits of a row depend on its values alone.  A column outside [0, D) is not followed: the rows of its tile are marked.
// Every barrier is reached by every thread: the trip counts depend on the descriptor alone.
template <bool BOX>
__global__ __launch_bounds__(FP_THREADS) void gauss_blocks_kernel(GaussBlocksArgs a, const double* __restrict__ x,
                                                                  int64_t row_stride, int64_t col_stride, int64_t n,
                                                                  const double* base, double* logp, GaussBoxArgs box) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int B = a.n_blocks, D = a.D, Dr = a.Dr, LD = D | 1;
    double* T = sm;                                                       // [FP_ROWS][LD]
    int* rowin = reinterpret_cast<int*>(sm + (size_t)FP_ROWS * LD);       // [FP_ROWS]
    const int tid = threadIdx.x;
    const int r = tid & (FP_ROWS - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / FP_ROWS);
    const int64_t row0 = (int64_t)blockIdx.x * FP_ROWS;
    const int rows = (int)min((int64_t)FP_ROWS, n - row0);
    if (tid < FP_ROWS) rowin[tid] = 1;
    gauss_load_tile(T, x, row_stride, col_stride, row0, rows, D, LD, tid);
    __syncthreads();
    double* Tr = T + r * LD;
    const bool live = r < rows;
    // 1. the elements
    for (int bb = 0; bb < B; ++bb) {
        const GaussBlock g = gauss_block(a, bb);
        GaussBox bx = {nullptr, nullptr};
        if (BOX) bx = gauss_box(box, bb);
        for (int j = w; j < g.k; j += GP_WAVES) {
            const int c = g.cols[j];
            const bool col_ok = (unsigned)c < (unsigned)D;
            if (!live) continue;
            if (!col_ok) { rowin[r] = 0; continue; }
            const double xv = Tr[c];
            Tr[c] = xv - g.mean[j];
            if (!isfinite(xv)) rowin[r] = 0;
            if (BOX && bx.lo) {
                if (!(xv >= bx.lo[j] && xv <= bx.hi[j])) rowin[r] = 0;
            }
        }
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
    __syncthreads();
    // 2. y = Linv d, from the last rows of Linv up
    for (int bb = 0; bb < B; ++bb) {
        const GaussBlock g = gauss_block(a, bb);
        for (int top = g.k - 1; top >= 0; top -= GP_WAVES * GP_ACC) {
            int iu[GP_ACC];
            gp_f64 Lu[GP_ACC];
            double y[GP_ACC];
#pragma unroll
            for (int u = 0; u < GP_ACC; ++u) {
                iu[u] = top - GP_ACC * w - u;                             // (below 0: nothing to form)
                const int i = max(iu[u], 0);
                Lu[u] = g.linv + ((int64_t)i * (i + 1)) / 2;
                y[u] = 0.0;
            }
            if (live) {
                // four d at a time while every y_i of the lane still takes them (their constants are fetched together),
                // then the ragged end; the order of a y_i's additions is j = 0, 1, ..., i either way
                int j = 0;
                for (; j + 3 <= iu[GP_ACC - 1]; j += 4) {
                    const double d0 = Tr[gauss_col(g.cols, j, D)], d1 = Tr[gauss_col(g.cols, j + 1, D)];
                    const double d2 = Tr[gauss_col(g.cols, j + 2, D)], d3 = Tr[gauss_col(g.cols, j + 3, D)];
#pragma unroll
                    for (int u = 0; u < GP_ACC; ++u) {
                        gp_f64 L = Lu[u] + j;
                        y[u] = (((y[u] + L[0] * d0) + L[1] * d1) + L[2] * d2) + L[3] * d3;
                    }
                }
                for (; j <= iu[0]; ++j) {
                    const double d = Tr[gauss_col(g.cols, j, D)];
#pragma unroll
                    for (int u = 0; u < GP_ACC; ++u)
                        if (j <= iu[u]) y[u] = y[u] + Lu[u][j] * d;
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int u = 0; u < GP_ACC; ++u)
                    if (iu[u] >= 0) Tr[gauss_col(g.cols, iu[u], D)] = y[u] * y[u];
            }
        }
    }
    __syncthreads();
    // 3. the row sums
    if (tid < rows) {
        double v = 0.0;
        if (base) {
            v = base[row0 + tid];
        } else if (Dr > 0) {
            for (int m = 0; m < Dr; ++m) v += Tr[gauss_col((gp_i32)a.rest_cols, m, D)];
        }
        for (int bb = 0; bb < B; ++bb) {
            const GaussBlock g = gauss_block(a, bb);
            double q = 0.0;
            for (int i = 0; i < g.k; ++i) q += Tr[gauss_col(g.cols, i, D)];
            const double gb = -0.5 * q - g.logc;
            v = (base || Dr > 0 || bb > 0) ? v + gb : gb;
        }
        logp[row0 + tid] = (rowin[tid] && isfinite(v)) ? v : -INFINITY;
    }
}

// Both entries: the checks (the texts under the entry's name), the arguments by value, the launch of one instance.
static int gauss_blocks_launch(const char* who, const pmc_gauss_blocks_t* g, const pmc_gauss_box_t* box, bool with_box,
                               const double* x, int64_t row_stride, int64_t col_stride, int64_t n, const double* base,
                               double* logp, void* stream) {
    char msg[192];
#define GP_FAIL(text) return (snprintf(msg, sizeof msg, "%s: " text, who), pmc_fail(msg))
    if (!g) GP_FAIL("bad descriptor");
    if (g->n_blocks < 1 || g->n_blocks > PMC_GAUSS_BLOCKS_MAX) GP_FAIL("n_blocks must lie in 1 .. 8");
    int64_t K = 0;
    for (int b = 0; b < g->n_blocks; ++b) {
        if (!g->cols[b] || !g->mean[b] || !g->linv[b]) GP_FAIL("bad block descriptor");
        if (g->dim[b] < 1) GP_FAIL("every block needs at least 1 column (dim >= 1)");
        K += g->dim[b];
    }
    if (g->D > FP_MAX_D) GP_FAIL("n_dim too large (D <= 157)");
    const pmc_prior_t* rest = g->rest;
    if ((rest == nullptr) != (g->rest_cols == nullptr)) GP_FAIL("rest and rest_cols go together (both, or both NULL)");
    if (rest && (!rest->family || !rest->loc || !rest->scale || rest->n_extended < 0 || rest->D < 1))
        GP_FAIL("bad prior descriptor");
    const int64_t Dr = rest ? rest->D : 0;
    if (K + Dr > g->D) GP_FAIL("the blocks and the rest have more columns than x (D)");
    if (rest && rest->n_extended > 0 && !rest->par)
        GP_FAIL("factors other than uniform / normal need the parameter table (par)");
    if (base && rest) GP_FAIL("base and rest exclude each other");
    if (with_box) {
        if (!box) GP_FAIL("bad box descriptor (NULL)");
        for (int b = 0; b < g->n_blocks; ++b)
            if ((box->lo[b] == nullptr) != (box->hi[b] == nullptr))
                GP_FAIL("lo and hi of a block go together (both, or both NULL: no box)");
    }
    if (n == 0) return 0;
    if (!x || !logp || n < 0 || row_stride < 0 || col_stride < 0) GP_FAIL("bad argument");
    if ((n + FP_ROWS - 1) / FP_ROWS > 0x7fffffffLL) GP_FAIL("too many rows for one launch");
#undef GP_FAIL
    GaussBlocksArgs a = {};
    GaussBoxArgs bx = {};
    a.n_blocks = g->n_blocks;
    a.D = g->D;
    for (int b = 0; b < PMC_GAUSS_BLOCKS_MAX; ++b) {
        const int s = b < g->n_blocks ? b : 0;                            // (entries behind n_blocks: block 0's, never used)
        a.cols[b] = g->cols[s];
        a.mean[b] = g->mean[s];
        a.linv[b] = g->linv[s];
        a.logc[b] = g->logc[s];
        a.dim[b] = g->dim[s];
        if (with_box) {
            bx.lo[b] = box->lo[s];
            bx.hi[b] = box->hi[s];
        }
    }
    a.Dr = (int32_t)Dr;
    if (rest) a.rest = *rest;
    a.rest_cols = g->rest_cols;
    const size_t lds = gauss_blocks_lds_bytes(g->D);
    const void* kernel = with_box ? reinterpret_cast<const void*>(gauss_blocks_kernel<true>)
                                  : reinterpret_cast<const void*>(gauss_blocks_kernel<false>);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(gauss_blocks_kernel)");
    }
    const dim3 grid((unsigned)((n + FP_ROWS - 1) / FP_ROWS)), block(FP_THREADS);
    if (with_box)
        hipLaunchKernelGGL(gauss_blocks_kernel<true>, grid, block, lds, (hipStream_t)stream, a, x, row_stride, col_stride, n,
                           base, logp, bx);
    else
        hipLaunchKernelGGL(gauss_blocks_kernel<false>, grid, block, lds, (hipStream_t)stream, a, x, row_stride, col_stride, n,
                           base, logp, bx);
    return pmc_check_launch("gauss_blocks_kernel");
}

extern "C" int pmc_gauss_blocks_logpdf(const pmc_gauss_blocks_t* g, const double* x, int64_t row_stride, int64_t col_stride,
                                       int64_t n, const double* base, double* logp, void* stream) {
    return gauss_blocks_launch("pmc_gauss_blocks_logpdf", g, nullptr, false, x, row_stride, col_stride, n, base, logp, stream);
}

extern "C" int pmc_gauss_box_logpdf(const pmc_gauss_blocks_t* g, const pmc_gauss_box_t* box, const double* x,
                                    int64_t row_stride, int64_t col_stride, int64_t n, const double* base, double* logp,
                                    void* stream) {
    return gauss_blocks_launch("pmc_gauss_box_logpdf", g, box, true, x, row_stride, col_stride, n, base, logp, stream);
}
