// The accepted walkers' blob rows from a host likelihood's pinned buffer into the walkers' device buffer
// (pmc_blob_rows_move, pmc_step_t.blob_host): the launch behind the accept.  A header so that the micro benchmark
// (scripts/micro/blob_move.hip) times the very kernel the library launches, at other numbers of loads in flight.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BLOB_MOVE_ROWS 64            // rows per block in x: the accept's row block, so narrow rows still fill a block
#define BLOB_MOVE_THREADS 256
// loads in flight per thread.  A load from pinned host memory is a PCIe round trip, but the launch hides it with blocks,
// not with a thread's own loads: the grid's second dimension shrinks as a thread takes more dwords.  Measured on an MI355X
// (scripts/micro/blob_move.hip; 1e4 rows, one in four accepted; us per launch at 1 / 2 / 4 / 8 / 16 loads in flight):
//     16-byte rows, pinned    5.55  5.58  5.57  5.57  5.62        HBM  3.88  3.96  3.79  3.64  3.78
//     64-byte rows, pinned    8.38  8.50  8.67  8.70  8.65        HBM  3.66  3.53  3.92  3.93  5.09
//   1040-byte rows, pinned   52.46 51.84 51.89 51.82 52.12        HBM  5.11  4.59  4.47  4.82  5.87
// -- no difference beyond the noise for the pinned source (the wide rows run at the link's 50 GB/s), so the accept's own
// four (accept_kernel<true>) stay.
#define BLOB_MOVE_INFLIGHT 4

// grid (ceil(n / BLOB_MOVE_ROWS), ceil(BLOB_MOVE_ROWS * row_dwords / (BLOB_MOVE_THREADS * U))): block (bx, by) owns the
// rows [bx * 64, bx * 64 + 64) and, of the flattened (row, dword) index over them, the by-th chunk of 256 * U dwords --
// rows are contiguous in both buffers, so narrow rows (a few dwords) and wide ones alike move in coalesced dwords.
// A rejected row is neither read nor written; a block without an accepted row in its chunk issues no load at all.
template <int U>
__global__ __launch_bounds__(BLOB_MOVE_THREADS) void blob_rows_move_kernel(const int32_t* __restrict__ accept,
                                                                           const uint32_t* __restrict__ src,
                                                                           uint32_t* __restrict__ dst, int64_t n, int rw) {
    __shared__ int flag[BLOB_MOVE_ROWS];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * BLOB_MOVE_ROWS;
    const int rows = (int)min((int64_t)BLOB_MOVE_ROWS, n - row0);
    if (tid < BLOB_MOVE_ROWS) flag[tid] = (tid < rows) ? accept[row0 + tid] : 0;
    __syncthreads();
    const uint32_t* __restrict__ s = src + (size_t)row0 * rw;
    uint32_t* __restrict__ d = dst + (size_t)row0 * rw;
    const int total = rows * rw;                                    // <= 64 * 2^18 dwords
    const int i0 = blockIdx.y * (BLOB_MOVE_THREADS * U) + tid;
    uint32_t v[U];
    bool a[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int i = i0 + k * BLOB_MOVE_THREADS;
        a[k] = i < total && flag[i / rw];
        v[k] = a[k] ? s[i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < U; ++k)
        if (a[k]) d[i0 + k * BLOB_MOVE_THREADS] = v[k];
}

template <int U>
static inline void blob_rows_move_launch(const int32_t* accept, const void* src, void* dst, int64_t n, int row_dwords,
                                         hipStream_t st) {
    const int64_t per_block = (int64_t)BLOB_MOVE_ROWS * row_dwords;
    const dim3 grid((unsigned)((n + BLOB_MOVE_ROWS - 1) / BLOB_MOVE_ROWS),
                    (unsigned)((per_block + BLOB_MOVE_THREADS * U - 1) / (BLOB_MOVE_THREADS * U)));
    hipLaunchKernelGGL(blob_rows_move_kernel<U>, grid, dim3(BLOB_MOVE_THREADS), 0, st, accept, (const uint32_t*)src,
                       (uint32_t*)dst, n, row_dwords);
}
