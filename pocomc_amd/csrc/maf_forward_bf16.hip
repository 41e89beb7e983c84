// Flow.forward / Flow.log_prob (pocomc/flow.py:99-114, :134-147) on the bf16 matrix cores: v_mfma_f32_16x16x32_bf16, fp32
// accumulate, fp32 master weights (the bf16 fragment image is derived from them by pmc_maf_pack_bf16), fp32 univariate map
// and log-determinant.  BASELINE config 5 names this precision ("8-layer MAF bf16"); it is an opt-in of Flow
// (precision="bf16"), the float32 kernels stay the default and the parity reference.
//
// The kernel and its launch rule are in maf_forward_bf16.h; this file holds the entry point, the image's pack kernel and
// the affine instances, maf_forward_bf16_nsf.hip the spline instances.
#include "maf_forward_bf16.h"

// image[i] = bf16(flat[idx[i]]) or 0
__global__ void maf_pack_bf16_kernel(const float* __restrict__ flat, const int32_t* __restrict__ idx,
                                     unsigned short* __restrict__ img, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t j = idx[i];
        img[i] = j >= 0 ? fbf::to_bf16(flat[j]) : (unsigned short)0;
    }
}

extern "C" int pmc_maf_pack_bf16(const float* flat, const int32_t* pack_idx, uint16_t* image, int64_t n, void* stream) {
    if (!flat || !pack_idx || !image || n <= 0) return pmc_fail("pmc_maf_pack_bf16: bad argument");
    int64_t grid = (n + 255) / 256; if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(maf_pack_bf16_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, flat, pack_idx, image, n);
    return pmc_check_launch("maf_pack_bf16_kernel");
}

extern "C" int pmc_maf_forward_bf16(const pmc_maf_t* m, const uint16_t* image, int64_t image_per_transform, const float* x,
                                    float* z, float* ladj, float* log_prob, int64_t n, const int64_t* idx, void* stream) {
    if (!m || !m->packed || !m->meta || !image || image_per_transform <= 0) return pmc_fail("pmc_maf_forward_bf16: null descriptor field");
    const bool spline = m->n_out == RQS_NOUT_OF(4) || m->n_out == RQS_NOUT_OF(8) || m->n_out == RQS_NOUT_OF(16);
    if (m->n_out != 2 && !spline) return pmc_fail("pmc_maf_forward_bf16: n_out must be 2 (affine) or 11, 23, 47 (splines of 4, 8, 16 bins)");
    // the image MAFSpec.bf16_layout describes: what the kernel's fragment pointers assume
    const int64_t nX2 = (m->Dp + 31) / 32, nK2 = (m->Hp + 31) / 32;
    if (image_per_transform != 512 * ((int64_t)m->nT * (nX2 + 2 * nK2) + (int64_t)m->nOT * nK2))
        return pmc_fail("pmc_maf_forward_bf16: image_per_transform is not this flow's bf16 layout");
    if (spline && m->nOT != m->n_out * m->nXT) return pmc_fail("pmc_maf_forward_bf16: a spline flow has n_out output tiles per 16 ranks");
    if (n == 0) return 0;
    if (!x || n < 0) return pmc_fail("pmc_maf_forward_bf16: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (spline) return pmc_launch_forward_bf16_nsf(m, image, image_per_transform, x, z, ladj, log_prob, n, idx, st);
    return dispatch_fwd_bf16<0>(m, image, image_per_transform, x, z, ladj, log_prob, n, idx, st);
}
