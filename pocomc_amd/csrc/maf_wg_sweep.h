// The skeleton of the WORKGROUP inverse sweeps (maf_inverse_wg.hip: affine flows, maf_inverse_wg_nsf.hip: 8-bin spline flows):
// eight wavefronts per 16 rows, a triangular sweep with two hidden-width arrays in LDS.  The description of the skeleton and
// the synchronisation contract stand here once for both kernels, with the constants they share.  The steps themselves are
// written out in each kernel: shared as inline functions they compiled to another instruction order and another place for the
// wait on the degree words, and both kernels lost 1 - 2 % (profiles/wide_sweep_skeleton.md has the measurements).  A change to
// a step of the skeleton is therefore made in BOTH .hip files.
//
// The other sweeps keep three hidden-width activation arrays; at the default width they exceed 160 KiB of LDS around n_dim 100
// (51 hidden tiles at D = 102), and those flows fell to the D-pass algorithm: D + 1 full passes of the hyper-network per
// transform.  These sweeps keep no activation array.  Units are sorted by degree and hidden tile T reads tiles <= T only, so
// once tile J is final its whole contribution to every later tile can be added at once -- what stays in LDS is the PARTIAL
// pre-activation of every unit:
//
//   X, Y   [Dp][16]       x found so far by rank (zeros where unknown), the transform's input by rank
//   H1acc  [Hp][16]       b1 + sum_{K<J} W1[., K] h0[K]
//   H2     [Hp][16]       b2 + sum_{K<J} W2[., K] h1[K]   (the spline kernel reuses the slots <= J, see there)
//   HT     3 x [16][16]   h0 | h1 | h2 of the current hidden tile J;   RED [NW][16] log-determinant words
//
// all in the 16-row MFMA operand layout of maf_common.h (lidx / store_rows), which is also how an accumulator tile is
// read back (rows_of).  Layer 0 has no array: h0[J] = relu(b0 + W0[J, :] X) is formed when tile J is reached.
//
// Per transform (last to first), per live hidden tile J:
//   REQUEST, all wavefronts: the fragments of the wavefront's update of tile J (U1, U2, the kernel's own output
//     fragments).  Nothing a tile loads from global memory depends on data, and the diagonal phase is spent waiting at the
//     barrier anyway.  Wavefront 0's diagonal fragments, layer-0 fragments, bias and W0 columns of tile J + 1 are requested
//     INSIDE the diagonal phase of tile J, each after the tile's use of the registers it refills.
//   DIAGONAL phase, wavefront 0: one mini-pass per distinct degree g of the tile (the quad meta words), each
//       h0[J] (the product over X once per tile; every later mini-pass adds the one rank the last one found,
//       a column of w0n), h1[J] = relu(H1acc[J] + W1[J, J] h0[J] + h0[J]),  h2[J] likewise,
//       then the kernel's output stage solves rank g: X[g] = x, ladj -= l.
//     Masked weights are exact zeros: the units of a higher degree in the tile are finite garbage until their own mini-pass
//     and enter as 0 * finite.  A dependent chain of one wavefront's LDS round trips and MFMAs; the other seven wait.
//   barrier
//   UPDATE phase, all wavefronts: H1acc[T] += W1[T, J] h0[J], H2[T] += W2[T, J] h1[J] for the tiles T > J, dealt by
//     T mod NW (every accumulator tile has one owner), then the kernel's output update.
//   barrier
//
// SYNCHRONISATION: lds_barrier() and nothing else.  Every wavefront reaches every barrier: no early return (rows past n
// are zeros on the way in and masked on the way out), every loop bound and every branch around a barrier comes from
// the descriptor and the meta words, none from a value computed from z.  Every register array is indexed by unrolled constants (the
// objects are built under check_resources.py --no-scratch).
#ifndef PMC_MAF_WG_SWEEP_H
#define PMC_MAF_WG_SWEEP_H

#include "maf_wg.h"
#include "inverse_lds.h"

#define WGS_PX 8                   // x tiles whose layer-0 fragments wavefront 0 requests one tile ahead (D <= 128; beyond: in place)
#define WGS_NU 7                   // hidden tiles of a wavefront's update whose fragments are requested before the diagonal phase
                                   // (flows of <= 8 WGS_NU + 1 = 57 hidden tiles; beyond: in place)

#endif
