// How many loads from pinned host memory should a thread of the blob move kernel keep in flight?
// (pocomc_amd/csrc/blob_move.h, pmc_blob_rows_move: the accepted walkers' blob rows from a host likelihood's pinned buffer
// into HBM.)  Times the library's kernel itself at 1, 2, 4, 8, 16 loads in flight per thread: n rows (default 10000), one
// row in four accepted, rows of 16, 64 and 1040 bytes; source in pinned host memory and, for comparison, in HBM.
// Time = HIP events around 50 back-to-back launches, divided by 50 (the launch overhead is hidden behind the queue).
// Measurement only.
// build: hipcc --offload-arch=gfx950 -O3 -I../../pocomc_amd/csrc blob_move.hip -o blob_move
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "blob_move.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int U>
static float time_move(const int32_t* acc, const void* src, void* dst, int64_t n, int rw, hipEvent_t e0, hipEvent_t e1) {
    const int reps = 50;
    for (int i = 0; i < 5; ++i) blob_rows_move_launch<U>(acc, src, dst, n, rw, 0);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < reps; ++i) blob_rows_move_launch<U>(acc, src, dst, n, rw, 0);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms * 1e3f / reps;
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? atoll(argv[1]) : 10000;
    if (n < 1 || n > (1 << 22)) { printf("n out of range\n"); return 1; }
    const int widths[3] = {16, 64, 1040};
    const size_t max_bytes = (size_t)n * 1040;
    std::vector<int32_t> h_acc(n);
    for (int64_t r = 0; r < n; ++r) h_acc[r] = (r * 2654435761u >> 7) % 4 == 0;
    int32_t* acc; CK(hipMalloc(&acc, n * sizeof(int32_t)));
    CK(hipMemcpy(acc, h_acc.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    uint32_t *pinned, *hbm, *dst;
    CK(hipHostMalloc(&pinned, max_bytes, hipHostMallocDefault));
    CK(hipMalloc(&hbm, max_bytes));
    CK(hipMalloc(&dst, max_bytes));
    for (size_t i = 0; i < max_bytes / 4; ++i) pinned[i] = (uint32_t)i * 2246822519u;
    CK(hipMemcpy(hbm, pinned, max_bytes, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<uint32_t> back(max_bytes / 4);
    for (int w : widths) {
        const int rw = w / 4;
        for (int where = 0; where < 2; ++where) {
            const void* src = where == 0 ? (const void*)pinned : (const void*)hbm;
            float us[5];
            us[0] = time_move<1>(acc, src, dst, n, rw, e0, e1);
            us[1] = time_move<2>(acc, src, dst, n, rw, e0, e1);
            us[2] = time_move<4>(acc, src, dst, n, rw, e0, e1);
            us[3] = time_move<8>(acc, src, dst, n, rw, e0, e1);
            us[4] = time_move<16>(acc, src, dst, n, rw, e0, e1);
            // the result of the library's own instance: accepted rows moved, the others untouched
            CK(hipMemset(dst, 0xff, (size_t)n * w));
            blob_rows_move_launch<BLOB_MOVE_INFLIGHT>(acc, src, dst, n, rw, 0);
            CK(hipMemcpy(back.data(), dst, (size_t)n * w, hipMemcpyDeviceToHost));
            long long bad = 0;
            for (int64_t r = 0; r < n; ++r)
                for (int j = 0; j < rw; ++j)
                    if (back[r * rw + j] != (h_acc[r] ? pinned[r * rw + j] : 0xffffffffu)) ++bad;
            printf("n %lld  row %4d B  source %-6s  us per launch at 1 / 2 / 4 / 8 / 16 loads in flight: %7.2f %7.2f %7.2f %7.2f %7.2f   wrong dwords: %lld\n",
                   (long long)n, w, where == 0 ? "pinned" : "HBM", us[0], us[1], us[2], us[3], us[4], bad);
        }
    }
    return 0;
}
