// The scaler-forward elements of a flow prior: one feature of a tile of rows in LDS, shared by flow_prior_pre_kernel
// (flow_prior.hip: the feature sits in its own tile column) and joint_prior_pre_kernel (joint_prior.hip: the feature sits in
// the column the prior's column map names).  One source: both produce the same bits.
#ifndef PMC_FLOW_PRIOR_BODY_H
#define PMC_FLOW_PRIOR_BODY_H

#include "scaler_body.h"

#define FP_ROWS 64
#define FP_THREADS 512
#define FP_MAX_D 157                              // the widest MCMC step

// The elements of one thread: feature ju of the rows r0, r0 + rpp, ..., read from tile column jt; KIND / LOGIT: the
// feature's kind and the transform, as constants.  x in T is replaced by the Jacobian term, u goes to U ([rows][DU]) as
// float32, a row with an element outside the support is marked in rowin.
template <int KIND, int LOGIT>
__device__ __forceinline__ void flow_prior_elements(const ScalerFeat& feat, int scale, double* T, float* U, int* rowin,
                                                    int r0, int rpp, int rows, int jt, int ju, int DU, int LD) {
    ScalerFeat f = feat;
    f.kind = KIND;
#pragma unroll 1
    for (int r = r0; r < rows; r += rpp) {
        const double xv = T[r * LD + jt];
        // Reparameterize.forward: the bounded -> unbounded map, then the affine part; the Jacobian term is that of the
        // inverse map at the unscaled value just computed
        const double t = bound_forward(f, LOGIT, 0, xv);
        double xb, J;
        bound_inverse(f, LOGIT, t, xb, J);
        const double u = scale ? (t - f.mu) / f.sigma : t;
        const float uf = (float)u;
        bool in = isfinite(xv) && isfinite(uf);
        if (KIND == 1 || KIND == 3) in = in && xv > f.low;
        if (KIND == 2 || KIND == 3) in = in && xv < f.high;
        T[r * LD + jt] = J;
        U[r * DU + ju] = uf;
        if (!in) rowin[r] = 0;
    }
}

// (a loop per kind: with the kind a run-time value inside one loop the compiler keeps the polynomial constants of
//  erfinv, log and exp in registers all at once, and spills)
__device__ __forceinline__ void flow_prior_feature(const ScalerFeat& f, const pmc_scaler_t& s, double* T, float* U,
                                                   int* rowin, int r0, int rpp, int rows, int jt, int ju, int DU, int LD) {
    if (f.kind == 0) flow_prior_elements<0, 0>(f, s.scale, T, U, rowin, r0, rpp, rows, jt, ju, DU, LD);
    else if (f.kind == 1) flow_prior_elements<1, 0>(f, s.scale, T, U, rowin, r0, rpp, rows, jt, ju, DU, LD);
    else if (f.kind == 2) flow_prior_elements<2, 0>(f, s.scale, T, U, rowin, r0, rpp, rows, jt, ju, DU, LD);
    else if (s.logit) flow_prior_elements<3, 1>(f, s.scale, T, U, rowin, r0, rpp, rows, jt, ju, DU, LD);
    else flow_prior_elements<3, 0>(f, s.scale, T, U, rowin, r0, rpp, rows, jt, ju, DU, LD);
}

// The join of a row: the flow's float32 log-density with the scaler's log-determinant (and the table factors' sum), -inf
// outside the support and for a value that is not finite.  One statement of it for the post kernels of flow_prior.hip /
// joint_prior.hip and for the step's closing kernel (step.hip), which must give their bits.
__device__ __forceinline__ double flow_prior_join(float lp32, double ldj, int inside) {
    const double v = (double)lp32 - ldj;
    return (inside && isfinite(v)) ? v : -INFINITY;
}
__device__ __forceinline__ double joint_prior_join(float lp32, double ldj, double rest_logp, int inside) {
    const double v = ((double)lp32 - ldj) + rest_logp;
    return (inside && isfinite(v)) ? v : -INFINITY;
}
// Several flow blocks (lp32 / ldj: [n_blocks][n], block b's row r at [b * n + r]) and an optional table (rest_logp NULL:
// none): the blocks' terms added left to right, then the table's.  One block: joint_prior_join with a table,
// flow_prior_join without one.
__device__ __forceinline__ double joint_blocks_join(int n_blocks, const float* lp32, const double* ldj,
                                                    const double* rest_logp, int inside, int64_t n, int64_t r) {
    double v = (double)lp32[r] - ldj[r];
    for (int b = 1; b < n_blocks; ++b) v = v + ((double)lp32[(int64_t)b * n + r] - ldj[(int64_t)b * n + r]);
    if (rest_logp) v = v + rest_logp[r];
    return (inside && isfinite(v)) ? v : -INFINITY;
}

#endif
