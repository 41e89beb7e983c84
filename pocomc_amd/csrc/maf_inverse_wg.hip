// Workgroup inverse sweep of the affine flows (PMC_INVERSE_TRIANGULAR_WG -> PMC_SWEEP_WG; an opt-in, AUTO never takes it).
// The skeleton, the LDS arrays it works on and the synchronisation contract are in maf_wg_sweep.h: read that first.  Here:
// the kernel, its LDS carve-up and its output stage, which is RIGHT-looking like the hidden layers --
//
//   Oacc   [nOT 16][16]   b3 + sum_{K<J} W3[., K] h2[K]          (shift, raw log-scale) rows, behind X | Y | H1acc | H2acc
//
//   DIAGONAL phase, after a mini-pass's hidden chain: (shift, raw) of rank g = Oacc rows + W3[rows, J] h2[J] from ONE
//     output tile, x = (y - shift) / exp(soft_ls(raw)),  ladj -= soft_ls(raw).
//   UPDATE phase: Oacc[O] += W3[O, J] h2[J] for the output tiles with a rank still to come, dealt by O mod NW.  The
//     fragments of a wavefront's first WGS_NUO output tiles are requested with those of its hidden update.
#include "maf_wg_sweep.h"

#define WGS_NUO 3                  // output tiles of a wavefront's update whose fragments are requested before the diagonal
                                   // phase (D <= 192; beyond: in place)

template <int NW>
__global__ __launch_bounds__(64 * NW) void maf_inverse_wg_sweep_kernel(pmc_maf_t m, const float* __restrict__ in,
                                                                       float* __restrict__ out,
                                                                       float* __restrict__ ladj_out, int64_t n) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, p = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    const int D = m.D, Dp = m.Dp, Hp = m.Hp, T = m.T, nT = m.nT, nOT = m.nOT, nXT = m.nXT;
    const int nTl = min(m.meta[7], nT);                  // live hidden tiles (the padding tiles trail)
    const int nOeff = min(nOT, (D + 7) / 8);             // output tiles with a rank < D
    float* X = smem;
    float* Y = X + Dp * 16;
    float* H1acc = Y + Dp * 16;
    float* H2acc = H1acc + Hp * 16;
    float* Oacc = H2acc + Hp * 16;
    float* HT0 = Oacc + nOT * 256;
    float* HT1 = HT0 + 256;
    float* HT2 = HT1 + 256;
    float* RED = HT2 + 256;                              // [NW][16]
    const int* feat_of_rank = m.meta + 8;
    const int* rank_of_feat = m.meta + 8 + T * D;
    const int* quad_meta = m.meta + 8 + 2 * T * D;

    {
        const int* ford = feat_of_rank + (T - 1) * D;
        for (int e = tid; e < Dp * 16; e += 64 * NW) {
            const int r = e >> 4, pp = e & 15;
            float v = 0.0f;
            if (r < D && row0 + pp < n) v = in[(row0 + pp) * D + ford[r]];
            Y[lidx(r, pp)] = v;
            X[lidx(r, pp)] = 0.0f;
        }
    }
    float ladj = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const MafView w = maf_view(m, t);
        // the accumulators start from the biases (a thread: one unit, four rows)
        for (int e = tid; e < Hp * 4; e += 64 * NW) {
            const int s = e >> 2, p0 = (e & 3) << 2;
            const float v1 = w.b1[s], v2 = w.b2[s];
#pragma unroll
            for (int j = 0; j < 4; ++j) { H1acc[lidx(s, p0 + j)] = v1; H2acc[lidx(s, p0 + j)] = v2; }
        }
        for (int e = tid; e < nOT * 64; e += 64 * NW) {
            const int o = e >> 2, p0 = (e & 3) << 2;
            const float v = w.b3[o];
#pragma unroll
            for (int j = 0; j < 4; ++j) Oacc[lidx(o, p0 + j)] = v;
        }
        lds_barrier();
        if (wv == 0 && q == 0) {
            // rank 0 reads nothing: bias only
            const float shift = w.b3[0], ls = soft_ls(w.b3[1]);
            X[lidx(0, p)] = (Y[lidx(0, p)] - shift) / expf(ls);
            ladj -= ls;
        }
        // Nothing a tile loads from global memory depends on data: the degree words, wavefront 0's diagonal fragments, layer-0
        // fragments and bias of tile J + 1 are requested while tile J runs, and every wavefront requests the fragments of its
        // update of tile J before the diagonal phase, which it spends waiting at the barrier anyway
        int dgn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dgn[i] = quad_meta[i];
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 nfr1 = zero4, nfr2 = zero4, nb0 = zero4, pf0[WGS_PX];
#pragma unroll
        for (int k = 0; k < WGS_PX; ++k) pf0[k] = zero4;
        // per group of the tile: its output fragment, and the column of W0 of the rank it finds (for the next mini-pass)
        float4 fr3[4], col[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { fr3[i] = zero4; col[i] = zero4; }
        if (wv == 0) {
            nfr1 = w.f1[lane]; nfr2 = w.f2[lane];
            nb0 = *reinterpret_cast<const float4*>(w.b0 + 4 * q);
#pragma unroll
            for (int k = 0; k < WGS_PX; ++k) pf0[k] = w.f0[(size_t)min(k, nXT - 1) * 64 + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = __builtin_amdgcn_readfirstlane(dgn[i] & 0xffff), gi = d < D ? d : 0;
                fr3[i] = w.f3[(size_t)(gi >> 3) * nT * 64 + lane];
                col[i] = *reinterpret_cast<const float4*>(w.w0n + (size_t)gi * Hp + 4 * q);
            }
        }
        for (int J = 0; J < nTl; ++J) {
            // the ranks the tile's degree groups produce (D: a padding quad), in slot order
            int dg[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dg[i] = __builtin_amdgcn_readfirstlane(dgn[i] & 0xffff);
            const int Jn = min(J + 1, nT - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) dgn[i] = quad_meta[4 * Jn + i];
            int gmax = -1;                               // the last rank that is known once this tile is final
#pragma unroll
            for (int i = 0; i < 4; ++i) if (dg[i] < D) gmax = max(gmax, dg[i]);

            // ---- the update's fragments: tiles T > J with T mod NW == wv, output tiles O mod NW == wv with a rank to come
            const int Tf = J + 1 + ((wv - (J + 1)) & (NW - 1));
            const int Olo = (gmax + 1) >> 3;             // (output tiles below it are finished)
            const int Of = Olo + ((wv - Olo) & (NW - 1));
            float4 U1[WGS_NU], U2[WGS_NU], U3[WGS_NUO];
#pragma unroll
            for (int k = 0; k < WGS_NU; ++k) {
                const size_t at = ((size_t)min(Tf + k * NW, nT - 1) * nT + J) * 64 + lane;
                U1[k] = w.f1[at];
                U2[k] = w.f2[at];
            }
#pragma unroll
            for (int k = 0; k < WGS_NUO; ++k) U3[k] = w.f3[((size_t)min(Of + k * NW, nOT - 1) * nT + J) * 64 + lane];

            // ---- diagonal phase
            if (wv == 0) {
                const f32x4 p1 = rows_of(H1acc, J, q, p), p2 = rows_of(H2acc, J, q, p);
                f32x4 a0 = {nb0.x, nb0.y, nb0.z, nb0.w}, a0b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < WGS_PX; ++k) {
                    if (k < nXT) {
                        if (k & 1) a0b = frag_mac(a0b, pf0[k], X + (k << 8), lane);
                        else a0 = frag_mac(a0, pf0[k], X + (k << 8), lane);
                    }
                }
                a0 += a0b;
                a0 = mac_range<4>(a0, w.f0 + (size_t)J * nXT * 64, X, WGS_PX, nXT, lane);
                nb0 = *reinterpret_cast<const float4*>(w.b0 + 16 * Jn + 4 * q);
#pragma unroll
                for (int k = 0; k < WGS_PX; ++k) pf0[k] = w.f0[((size_t)Jn * nXT + min(k, nXT - 1)) * 64 + lane];
                int g_prev = -1;
                float4 c_prev = zero4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int g = dg[i];
                    const bool group = g < D && (i == 0 || g != dg[i - 1]);
                    if (!group && !(i == 3 && g_prev < 0)) continue;        // (a tile without a group: its units once)
                    const int O = group ? (g >> 3) : 0;
                    if (g_prev >= 0) {
                        // the rank the last mini-pass found enters layer 0: one column of W0
                        const float xv = X[lidx(g_prev, p)];
                        a0[0] += c_prev.x * xv; a0[1] += c_prev.y * xv; a0[2] += c_prev.z * xv; a0[3] += c_prev.w * xv;
                    }
                    f32x4 h0, a1, a2;
#pragma unroll
                    for (int r = 0; r < 4; ++r) h0[r] = fmaxf(a0[r], 0.0f);
                    store_rows(HT0, 0, q, p, h0);
                    a1 = frag_mac(p1, nfr1, HT0, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) a1[r] = fmaxf(a1[r] + h0[r], 0.0f);
                    store_rows(HT1, 0, q, p, a1);
                    a2 = frag_mac(p2, nfr2, HT1, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) a2[r] = fmaxf(a2[r] + a1[r], 0.0f);
                    store_rows(HT2, 0, q, p, a2);
                    if (group) {
                        f32x4 o = rows_of(Oacc, O, q, p);
                        o = frag_mac(o, fr3[i], HT2, lane);
                        // rows 2 (g & 7), + 1 of the output tile: quad (g & 7) >> 1 holds them
                        if (q == ((g & 7) >> 1)) {
                            const float shift = (g & 1) ? o[2] : o[0];
                            const float ls = soft_ls((g & 1) ? o[3] : o[1]);
                            X[lidx(g, p)] = (Y[lidx(g, p)] - shift) / expf(ls);
                            ladj -= ls;
                        }
                        g_prev = g;
                        c_prev = col[i];
                    }
                }
                nfr1 = w.f1[((size_t)Jn * nT + Jn) * 64 + lane];
                nfr2 = w.f2[((size_t)Jn * nT + Jn) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = __builtin_amdgcn_readfirstlane(dgn[i] & 0xffff), gi = d < D ? d : 0;
                    fr3[i] = w.f3[((size_t)(gi >> 3) * nT + Jn) * 64 + lane];
                    col[i] = *reinterpret_cast<const float4*>(w.w0n + (size_t)gi * Hp + 16 * Jn + 4 * q);
                }
            }
            lds_barrier();

            // ---- update phase: tile J is final
#pragma unroll
            for (int k = 0; k < WGS_NU; ++k) {
                const int Tt = Tf + k * NW;
                if (Tt < nTl) {
                    f32x4 a1 = rows_of(H1acc, Tt, q, p), a2 = rows_of(H2acc, Tt, q, p);
                    a1 = frag_mac(a1, U1[k], HT0, lane);
                    a2 = frag_mac(a2, U2[k], HT1, lane);
                    store_rows(H1acc, Tt, q, p, a1);
                    store_rows(H2acc, Tt, q, p, a2);
                }
            }
            for (int Tt = Tf + WGS_NU * NW; Tt < nTl; Tt += NW) {            // (flows of more than 8 WGS_NU + 1 hidden tiles)
                const size_t at = ((size_t)Tt * nT + J) * 64 + lane;
                f32x4 a1 = rows_of(H1acc, Tt, q, p), a2 = rows_of(H2acc, Tt, q, p);
                a1 = frag_mac(a1, w.f1[at], HT0, lane);
                a2 = frag_mac(a2, w.f2[at], HT1, lane);
                store_rows(H1acc, Tt, q, p, a1);
                store_rows(H2acc, Tt, q, p, a2);
            }
#pragma unroll
            for (int k = 0; k < WGS_NUO; ++k) {
                const int O = Of + k * NW;
                if (O < nOeff) {
                    f32x4 o = rows_of(Oacc, O, q, p);
                    o = frag_mac(o, U3[k], HT2, lane);
                    store_rows(Oacc, O, q, p, o);
                }
            }
            for (int O = Of + WGS_NUO * NW; O < nOeff; O += NW) {
                f32x4 o = rows_of(Oacc, O, q, p);
                o = frag_mac(o, w.f3[((size_t)O * nT + J) * 64 + lane], HT2, lane);
                store_rows(Oacc, O, q, p, o);
            }
            lds_barrier();
        }
        // x of this transform is the next one's input (by that transform's ranks), or the result; X starts from zero again
        {
            const int* ford = feat_of_rank + t * D;
            const int* rnext = t > 0 ? rank_of_feat + (t - 1) * D : nullptr;
            for (int e = tid; e < Dp * 16; e += 64 * NW) {
                const int r = e >> 4, pp = e & 15;
                if (r < D) {
                    const float v = X[lidx(r, pp)];
                    const int feat = ford[r];
                    if (rnext) Y[lidx(rnext[feat], pp)] = v;
                    else if (row0 + pp < n) out[(row0 + pp) * D + feat] = v;
                }
                X[lidx(r, pp)] = 0.0f;
            }
        }
    }
    const float l = quad_sum(ladj);
    if (lane < 16) RED[wv * 16 + lane] = l;
    lds_barrier();
    if (wv == 0) {
        float lt = 0.0f;
#pragma unroll
        for (int k = 0; k < NW; ++k) lt += RED[16 * k + p];
        if (ladj_out && lane < 16 && row0 + p < n) ladj_out[row0 + p] = lt;
    }
}

// The instance the plan names (inverse_plan.hip: PMC_SWEEP_WG): the plain inverse of z only
int pmc_launch_inverse_wg_sweep(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z,
                                float* x, float* ladj, int64_t n, hipStream_t stream) {
    const size_t lds = pmc_lds_wg_sweep(m);
    if (plan->sweep != PMC_SWEEP_WG || pa || m->n_out != 2 || !m->tri_ok || lds > PMC_LDS_CAP || (size_t)plan->lds_bytes != lds)
        return pmc_fail("pmc_launch_inverse_wg_sweep: not this sweep's plan");
    if (int e = pmc_launch_lds(maf_inverse_wg_sweep_kernel<WGS_NW>, "hipFuncSetAttribute(maf_inverse_wg_sweep_kernel)",
                               dim3((unsigned)((n + 15) / 16)), dim3(64 * WGS_NW), lds, stream, *m, z, x, ladj, n)) return e;
    return pmc_check_launch("maf_inverse_wg_sweep_kernel");
}
