// LDS layouts of the flow-inverse sweeps: the words the kernels carve their dynamic shared memory with, and the one size
// function per sweep that the plan (inverse_plan.hip) holds against the 160 KiB a workgroup can have.
#ifndef PMC_INVERSE_LDS_H
#define PMC_INVERSE_LDS_H

#include "pmc_internal.h"

#define PMC_LDS_CAP ((size_t)160 * 1024)

// ---- register-chain sweeps of the affine flows (maf_inverse_tri4.hip)
#define DG_WORDS(m) ((m)->nT * 4 + 8)      // LDS words of the tiles' degree table (4 per tile, padded)
// + the two-wave sweep's permutation / rank-0 tables and its second x array (with alignment slack)
#define TRI5_TT_WORDS(m) (((m)->nT + 2) * 16)  // the two-wave sweep's per-tile table (16 words per hidden tile, two rows of "no groups" behind)
#define TRI5_YT_WORDS(m) ((m)->T * (((m)->nT + 2) * 4 + 1))   // per transform: the y offsets of every tile's groups, of rank 0
#define TRI5_TABLE_WORDS(m) (((TRI5_TT_WORDS(m) + (m)->Dp + 2 * (m)->T + 3) & ~3) + (m)->Dp * 16 + ((TRI5_YT_WORDS(m) + 3) & ~3))
#define TRI5_LDS_FLOATS(m, maxo) (2 * (m)->Dp * 16 + 2 * (m)->Hp * 16 + 2 * 256 + 2 * (3 + (maxo)) * 256 + TRI5_TABLE_WORDS(m))
#define OOB_VOFF 0x40000000        // a lane offset beyond every image: the bounds-checked load returns zeros

static inline size_t pmc_lds_solo(const pmc_maf_t* m, int maxo) { return (size_t)(2 * m->Dp * 16 + 2 * m->Hp * 16 + 3 * 256 + maxo * 256 + DG_WORDS(m)) * sizeof(float); }
static inline size_t pmc_lds_duo(const pmc_maf_t* m, int maxo) { return (size_t)TRI5_LDS_FLOATS(m, maxo) * sizeof(float); }

// ---- lane-per-walker sweep (maf_inverse_tri6.hip)
#define TRI6_SPAD 20               // floats per walker row of a staging tile (16 + 4: conflict-free b128)
#define TRI6_FLAG_WORDS 8          // tri6::F_COUNT

// ns walker subsets per workgroup; hb: 0 float32 helpers, 1 / 2 the 16-bit ones
static inline size_t pmc_lds_lane(const pmc_maf_t* m, int ns, int hb) {
    const int h_floats = hb ? ((m->nT + 1) >> 1) * 256 : m->nT * 256;       // (Ops<HB>::act_floats: one activation array of a subset)
    const int x_floats = hb ? m->Dp * 16 + ((m->nXT + 1) >> 1) * 256 : 2 * m->Dp * 16;   // y, x by rank (16-bit helpers: x over y in place + the helper's copy)
    return (size_t)(ns * (x_floats + 3 * h_floats) + 3 * 2 * ns * 16 * TRI6_SPAD + 2 * 2 * 16 * ns * TRI6_SPAD) * sizeof(float)
           + (TRI6_FLAG_WORDS + 8) * sizeof(int);        // (+ 8: the wavefronts' SIMD ids of the five-wave variant)
}

// ---- two-wave spline sweep (maf_inverse_nsf2.hip)
#define NSF2_PK 10                 // K tiles of the hidden bursts held in registers; the static burst tile covers flows of <= NSF2_PK + 1 live tiles
#define NSF2_OOB 0x40000000        // a lane offset beyond every image: the bounds-checked load returns zeros
#define NSF2_STAGE_FLOATS (3 * 256)                 // hidden staging S0 | S1 | S2 (transposed, [lane][4])
#define NSF2_PART_FLOATS (4 * 2 * 256)              // output staging [group][half][lane][4]
#define NSF2_TT_WORDS(m) (((m)->nT + 2) * 8)        // per-tile table: ranks (word 0 also the pattern), x / y byte offsets
#define NSF2_YT_WORDS(m) ((m)->T * (((m)->nT + 2) * 4 + 1))   // per transform: the y offsets of every tile's groups, of rank 0
#define NSF2_LDS_BASE_FLOATS(m) (3 * (m)->Dp * 16 + 3 * (m)->Hp * 16 + 2 * NSF2_STAGE_FLOATS + 2 * NSF2_PART_FLOATS + 16 * 32 + \
                                 ((NSF2_TT_WORDS(m) + (m)->Dp + NSF2_YT_WORDS(m) + 3) & ~3))
// EAGER PARTIALS (round 4).  The burst wave's work for tile T1 grows with T1 (40 (T1 - 1) MFMAs at 32 cycles each against a
// chain that takes ~9 k cycles per tile whatever the tile): from the seventh tile on the chain waited for it (barrier
// stamps, docs/LAB_NOTEBOOK.md: 0.5 / 2.1 / 3.1 k cycles at tiles 5 - 7 of a nine-tile flow) while on tiles 1 - 4 the burst wave waited
// 2 - 4 k cycles for the chain.  The output partials of the LAST TWO live tiles therefore start early: their ranks' products
// against h2 tiles 0, 1, 2 (last tile) and 0, 1 (the one before) are formed at steps 2, 3, 4 -- in the burst wave's idle
// time -- into two more partial buffers in LDS that only the burst wave touches; the two tiles' own steps start from those
// and run K = 3 .. / 2 .. only (nsf_burst_tile<T1, KS>).  Flows of >= 8 live tiles on the static path whose LDS stays within
// half a CU's (two workgroups per CU).
#define NSF2_EAGER_FLOATS (2 * NSF2_PART_FLOATS)
#define NSF2_EAGER_OK(m) ((m)->nT >= 8 && (m)->nT <= NSF2_PK + 1 && \
                          (size_t)(NSF2_LDS_BASE_FLOATS(m) + NSF2_EAGER_FLOATS) * sizeof(float) <= 80 * 1024)
#define NSF2_LDS_FLOATS(m) (NSF2_LDS_BASE_FLOATS(m) + (NSF2_EAGER_OK(m) ? NSF2_EAGER_FLOATS : 0))

static inline size_t pmc_lds_nsf_duo(const pmc_maf_t* m) { return (size_t)NSF2_LDS_FLOATS(m) * sizeof(float); }

// ---- lone-wave spline sweep (maf_inverse_tri_nsf.hip) and the affine D-pass kernel (maf_kernels.hip)
static inline size_t pmc_lds_nsf_solo(const pmc_maf_t* m) { return (size_t)(2 * m->Dp * 16 + 3 * m->Hp * 16 + 16 * 32 + 16 * 24) * sizeof(float); }
static inline size_t pmc_lds_dense(const pmc_maf_t* m, int n_rank_arrays) { return (size_t)(n_rank_arrays * m->Dp * 16 + 3 * m->Hp * 16) * sizeof(float); }

// ---- workgroup kernel of the forward pass and of the spline flows' D-pass inverse (maf_forward_wg.hip): nw wavefronts, the
// univariate map's panel, the inverse's iterate.  lean: the instance whose third activation array aliases the first
static inline size_t pmc_lds_wg(const pmc_maf_t* m, int nw, int panel_tiles, int inverse, int lean = 0) {
    return (size_t)(2 * m->Dp * 16 + (lean ? 2 : 3) * m->Hp * 16 + 16 * nw + panel_tiles * 256 + (inverse ? m->Dp * 16 : 0)) * sizeof(float);
}
static inline int pmc_wg_panel_tiles(const pmc_maf_t* m) { return m->n_out == 2 ? 0 : m->n_out; }
// Which instance of the workgroup kernel a call takes: the full one wherever it fits (what every flow that ran before the
// lean instances existed keeps launching), the lean one where only that fits or PMC_MAF_VARIANT_LEAN_LDS asks for it.
// Returns the launch's LDS bytes and sets *lean, or 0: neither fits
static inline size_t pmc_wg_instance(const pmc_maf_t* m, int nw, int inverse, int* lean) {
    const size_t full = pmc_lds_wg(m, nw, pmc_wg_panel_tiles(m), inverse, 0), small = pmc_lds_wg(m, nw, pmc_wg_panel_tiles(m), inverse, 1);
    *lean = (m->reserved & PMC_MAF_VARIANT_LEAN_LDS) || full > PMC_LDS_CAP;
    const size_t lds = *lean ? small : full;
    return lds <= PMC_LDS_CAP ? lds : 0;
}

// ---- workgroup sweep of the affine flows (maf_inverse_wg.hip): x and y by rank, the partial pre-activations of hidden layers
// 1 and 2, the partial output rows, the current hidden tile's h0 | h1 | h2, the log-determinant words of 8 wavefronts
#define WGS_NW 8
static inline size_t pmc_lds_wg_sweep(const pmc_maf_t* m) {
    return (size_t)(2 * m->Dp * 16 + 2 * m->Hp * 16 + m->nOT * 256 + 3 * 256 + 16 * WGS_NW) * sizeof(float);
}

// ---- workgroup sweep of the spline flows (maf_inverse_wg_nsf.hip): x and y by rank, the partial pre-activations of hidden
// layer 1, the array that holds layer 2's partial pre-activations beyond the current tile and the final h2 up to it, the
// current tile's h0 | h1 | h2, one output-partial tile per wavefront, the rank's parameter panel [16][32] and knot tables
// [16][24], the log-determinant words
static inline size_t pmc_lds_wg_nsf_sweep(const pmc_maf_t* m) {
    return (size_t)(2 * m->Dp * 16 + 2 * m->Hp * 16 + 3 * 256 + WGS_NW * 256 + 16 * 32 + 16 * 24 + 16 * WGS_NW) * sizeof(float);
}

// A launch with dynamic LDS: hipFuncSetAttribute first when it is more than 48 KiB (every such launch: nothing is remembered)
template <typename K, typename... A>
static int pmc_launch_lds(K kernel, const char* name, dim3 grid, dim3 block, size_t lds, hipStream_t stream, A... args) {
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return pmc_fail_hip(e, name);
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return 0;
}

#endif
