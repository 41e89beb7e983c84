// What the correlated normal kernels share (gauss_prior.hip: gauss_blocks_kernel; gauss_mix_prior.hip: gauss_mix_kernel): the
// thread mapping's constants, the constant address space of the blocks' constants, and the 64-row tile of x in LDS.
#pragma once
#include "pmc_internal.h"
#include "flow_prior_body.h"

#define GP_WAVES (FP_THREADS / FP_ROWS)            // 8: a wavefront's lane is a row of the tile, its number picks i
#define GP_ACC 4                                   // rows of Linv a lane carries through one walk over d

// The blocks' constants live in the constant address space for the kernel: nobody writes them during the launch, and a load
// at an address the wavefront shares is then a scalar load (through the scalar cache, into SGPRs) where a generic pointer
// makes it a vector load of 64 equal addresses.
typedef const double __attribute__((address_space(4))) * gp_f64;
typedef const int32_t __attribute__((address_space(4))) * gp_i32;

// a column of the caller's map, never followed outside the tile
__device__ __forceinline__ int gauss_col(gp_i32 cols, int j, int D) {
    const int c = cols[j];
    return (unsigned)c < (unsigned)D ? c : 0;
}

// joint_prior_pre_kernel's tile and stride contract: rows row0 .. row0 + rows - 1 of all D columns of x into T[rows][LD],
// LD = D | 1, by all FP_THREADS threads; col_stride == 1 walks a row's columns, anything else a column's rows -- the two
// coalesced layouts (D, 1) and (1, n), other strides correctly and slowly.  The caller's barrier follows.
__device__ __forceinline__ void gauss_load_tile(double* T, const double* __restrict__ x, int64_t row_stride,
                                                int64_t col_stride, int64_t row0, int rows, int D, int LD, int tid) {
    if (col_stride == 1) {
        int rr = tid / D, cc = tid - rr * D;                              // element e = rr * D + cc, stepped without a division
        const int dr = FP_THREADS / D, dc = FP_THREADS - dr * D;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[rr * LD + cc] = x[(row0 + rr) * row_stride + cc];
            rr += dr; cc += dc;
            if (cc >= D) { cc -= D; ++rr; }
        }
    } else {
        int cc = tid / rows, rr = tid - cc * rows;                        // element e = cc * rows + rr
        const int dc = FP_THREADS / rows, dr = FP_THREADS - dc * rows;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[rr * LD + cc] = x[(row0 + rr) * row_stride + (int64_t)cc * col_stride];
            cc += dc; rr += dr;
            if (rr >= rows) { rr -= rows; ++cc; }
        }
    }
}
