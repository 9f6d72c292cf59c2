// trk_mosaic.hip -- prancSTR's per-call model as a device pass, for gfx950: for every called sample at every locus the
// mosaic allele C and the mosaic fraction f that maximise the likelihood of the call's reads, and the likelihood-ratio
// test of f = 0.
//
// Reference (trtools/prancSTR/prancSTR.py): one Python loop per call that alternates a search over candidate alleles
// (Just_C_Pred, :119-155) with a bounded 1-D maximisation by scipy's SLSQP (Just_F_Pred, :158-189), at most 101 rounds
// (MaximizeMosaicLikelihoodBoth, :56-117), then ComputePvalue (:357-385).  The semantics are stated in include/trk.h
// (trk_mosaic_fit).  The f step here is NOT SLSQP: both branches of the likelihood are sums of logs of affine functions
// of f, hence concave, so the maximiser on [0, 0.5] is an end point or the root of a monotone derivative, and that root
// is bracketed to the last bit.  The pass returns the optimum SLSQP approximates.
//
//   k_mosaic_select<0>  a thread per call of the dense [L, S] grid: the call's status (prancSTR.py:549-562) from A, B
//                       and the call's slice of the CSR read arrays; the outputs of a skipped call; per workgroup the
//                       numbers of calls to fit, those with at most MOS_CAP distinct read values and the others.
//   (k_scan_u32)        the exclusive scan of the 2 x workgroups counts: small calls first, then large.
//   k_mosaic_select<1>  the ordered scatter: a call's place is its workgroup's offset plus its rank inside the workgroup
//                       (ballots and a prefix over the four waves).  No atomics: the list is row-major and the same on
//                       every run.
//   k_mosaic_fit<LDS>   over the compact list.  A group of 16 lanes (one DPP row) per call, four calls per wave, a wave
//                       per workgroup (the groups of a wave meet only in the wave's LDS: no workgroup barrier).  A lane
//                       is an EVALUATION POINT, never the owner of a read value:
//                         C step: a lane owns one candidate allele, 16 candidates at a time; both branches' log
//                           likelihoods are summed serially over the call's R read values, which every lane of the group
//                           reads from the same LDS address (a broadcast) -- {r, n, P[r-A], P[r-B]}, filled once per
//                           call -- plus its own P[r-C] from the locus's stutter table.  The argmax over candidates is
//                           four xor-shuffle steps inside the row on {LL, candidate}, ties to the smaller candidate
//                           (the reference's first maximum).
//                         f step: a lane owns one probe point.  One evaluation puts f = 0 and f = 0.5 on alternate
//                           lanes (the end-point rule); then 13 rounds, each of which probes the 16 interior points
//                           of both branches' brackets at once: the derivative is monotone, so the number of lanes
//                           on which it is positive names the sub-interval that holds the root, and the bracket
//                           shrinks 17 times a round: 17^13 > 2^53.  No convergence test.
//                       The 201-entry stutter table P[-100 .. 100] of a group's locus is built in LDS from (u, d, rho)
//                       by repeated multiplication; the list is row-major, so the groups of a wave mostly share a locus
//                       and then share the table of the first of them.
//                       LDS = true: calls with R <= MOS_CAP.  LDS = false: any R, the reads come from global memory
//                       (the table still from LDS).
// Every loop is bounded by R, the candidate span (<= TRK_MOSAIC_MAX_SPAN, checked by the select pass), 13 or 101.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/trk.h"
#include "trk_internal.h"

namespace {

constexpr int WAVE = 64;
constexpr int ROW = 16;                  // lanes per call
constexpr int GROUPS = WAVE / ROW;       // calls per wave
constexpr int SEL_THREADS = 256;
constexpr int MOS_CAP = 64;              // distinct read values of a call served from LDS
constexpr int MOS_D = 100;               // deltas are confined to +-100 (Likelihood_mosaic, prancSTR.py:314-326)
constexpr int MOS_NP = 2 * MOS_D + 1;
constexpr int F_ROUNDS = 13;
constexpr int MAX_PAIRS = 100;           // maxiter of MaximizeMosaicLikelihoodBoth
constexpr double MOS_ZERO = 10e-200;     // the reference's ZERO

struct MosArgs {
    int L, S;
    int64_t n_calls;
    int64_t n_reads;
    int output_all, fit_all;
    const int32_t* ab;
    const int32_t* off;
    const int32_t* val;
    const int32_t* cnt;
    const double* stutter;
    int32_t* out_c;
    double* out_f;
    double* out_pval;
    double* out_llf;
    double* out_ll0;
    int32_t* out_sup;
    uint8_t* out_status;
    uint32_t* counts;   // [2 * nwg]: small calls per select workgroup, then large; after the scan their offsets
    uint32_t* total;    // calls to fit
    uint32_t* list;     // [n_calls] the calls to fit: small ones in row-major order, then the large ones
    int nwg;
};

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int confine(int64_t d) { return (int)(d < -MOS_D ? -MOS_D : d > MOS_D ? MOS_D : d); }

// the status of call c (include/trk.h); R: its number of distinct read values
__device__ int mosaic_status(const MosArgs& a, int64_t c, int& R) {
    const int64_t o0 = a.off[c], o1 = a.off[c + 1];
    R = 0;
    if (o0 < 0 || o1 < o0 || o1 > a.n_reads) return TRK_MOSAIC_BAD;
    R = (int)(o1 - o0);
    const int32_t A = a.ab[2 * c], B = a.ab[2 * c + 1];
    if (A == TRK_MOSAIC_NOCALL_AB || B == TRK_MOSAIC_NOCALL_AB || R == 0) return TRK_MOSAIC_NOCALL;
    bool has_a = false, has_b = false, bad = false;
    int32_t prev = 0;
    for (int j = 0; j < R; ++j) {
        const int32_t r = a.val[o0 + j];
        bad |= a.cnt[o0 + j] <= 0 || (j > 0 && r <= prev) || r < -TRK_MOSAIC_MAX_ABS || r > TRK_MOSAIC_MAX_ABS;
        has_a |= r == A;
        has_b |= r == B;
        prev = r;
    }
    if (bad || (int64_t)prev - (int64_t)a.val[o0] + 7 > TRK_MOSAIC_MAX_SPAN) return TRK_MOSAIC_BAD;
    if (a.fit_all) return TRK_MOSAIC_FIT;
    // "A not in reads or B not in reads and not output_all" (prancSTR.py:558) as Python reads it
    if (!has_a || (!has_b && !a.output_all)) return TRK_MOSAIC_UNSUPPORTED;
    if (R == 1 && !a.output_all) return TRK_MOSAIC_SINGLE;
    return TRK_MOSAIC_FIT;
}

// PHASE 0: statuses, the outputs of the skipped calls, the workgroup's counts.  PHASE 1: the ordered scatter.
template <int PHASE>
__global__ __launch_bounds__(SEL_THREADS) void k_mosaic_select(const MosArgs a) {
    __shared__ uint32_t w_small[SEL_THREADS / WAVE], w_large[SEL_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid >> 6;
    const int64_t c = (int64_t)blockIdx.x * SEL_THREADS + tid;
    int cls = 0;   // 1: fitted from LDS, 2: fitted from global memory
    if (c < a.n_calls) {
        int R;
        if (PHASE == 0) {
            const int st = mosaic_status(a, c, R);
            a.out_status[c] = (uint8_t)st;
            if (st != TRK_MOSAIC_FIT) {
                a.out_c[c] = 0;
                a.out_sup[c] = 0;
                a.out_f[c] = a.out_pval[c] = a.out_llf[c] = a.out_ll0[c] = __builtin_nan("");
            } else
                cls = R <= MOS_CAP ? 1 : 2;
        } else if (a.out_status[c] == TRK_MOSAIC_FIT)
            cls = a.off[c + 1] - a.off[c] <= MOS_CAP ? 1 : 2;
    }
    const uint64_t m_small = __ballot(cls == 1), m_large = __ballot(cls == 2);
    if (lane == 0) {
        w_small[wid] = (uint32_t)__popcll(m_small);
        w_large[wid] = (uint32_t)__popcll(m_large);
    }
    __syncthreads();
    if (PHASE == 0) {
        if (tid == 0) {
            a.counts[blockIdx.x] = (w_small[0] + w_small[1]) + (w_small[2] + w_small[3]);
            a.counts[a.nwg + blockIdx.x] = (w_large[0] + w_large[1]) + (w_large[2] + w_large[3]);
        }
    } else if (cls) {
        const uint32_t* w = cls == 1 ? w_small : w_large;
        uint32_t at = a.counts[(cls == 1 ? 0 : a.nwg) + blockIdx.x];
        for (int k = 0; k < wid; ++k) at += w[k];
        at += (uint32_t)__popcll((cls == 1 ? m_small : m_large) & ((1ull << lane) - 1ull));
        a.list[at] = (uint32_t)c;
    }
}

// one call's reads as the lanes of its group see them
template <bool LDS>
struct Reads {
    int R;
    int32_t A, B;
    const double* tab;      // LDS: the locus's P[-100 .. 100]
    const int32_t* r;       // LDS records (LDS) or the call's slice of the global arrays
    const double* n;
    const double* pa;
    const double* pb;
    const int32_t* cnt;
    __device__ __forceinline__ void get(int j, int32_t& rj, double& nj, double& paj, double& pbj) const {
        rj = r[j];
        if (LDS) {
            nj = n[j];
            paj = pa[j];
            pbj = pb[j];
        } else {
            nj = (double)cnt[j];
            paj = tab[MOS_D + confine((int64_t)rj - A)];
            pbj = tab[MOS_D + confine((int64_t)rj - B)];
        }
    }
};

// LL_1(C, f) and LL_2(C, f) of the definition, the terms in the reference's order
template <bool LDS>
__device__ __forceinline__ void ll_both(const Reads<LDS>& rd, int32_t C, double f, double& l1, double& l2) {
    const bool is_ab = C == rd.A || C == rd.B;
    l1 = l2 = 0.0;
    for (int j = 0; j < rd.R; ++j) {
        int32_t r;
        double n, pa, pb;
        rd.get(j, r, n, pa, pb);
        const double pc = rd.tab[MOS_D + confine((int64_t)r - C)];
        const double v1 = is_ab ? MOS_ZERO : (0.5 * pa + (0.5 - f) * pb) + f * pc;
        const double v2 = is_ab ? MOS_ZERO : ((0.5 - f) * pa + 0.5 * pb) + f * pc;
        l1 = l1 + n * log(v1);
        l2 = l2 + n * log(v2);
    }
}

// d LL_k / d f at f: sum n b_k / L_k(f), b_1 = P[r-C] - P[r-B], b_2 = P[r-C] - P[r-A]; L_k in the likelihood's own form
// (a + b_k f would cancel to 0 where P[r-B] dwarfs the other two)
template <bool LDS>
__device__ __forceinline__ void g_both(const Reads<LDS>& rd, int32_t C, double f1, double f2, double& g1, double& g2) {
    const bool is_ab = C == rd.A || C == rd.B;
    g1 = g2 = 0.0;
    for (int j = 0; j < rd.R; ++j) {
        int32_t r;
        double n, pa, pb;
        rd.get(j, r, n, pa, pb);
        const double pc = rd.tab[MOS_D + confine((int64_t)r - C)];
        const double b1 = is_ab ? 0.0 : pc - pb, b2 = is_ab ? 0.0 : pc - pa;
        g1 = g1 + n * b1 / ((0.5 * pa + (0.5 - f1) * pb) + f1 * pc);
        g2 = g2 + n * b2 / (((0.5 - f2) * pa + 0.5 * pb) + f2 * pc);
    }
}

__device__ __forceinline__ double bracket_point(double lo, double w, int i) { return lo + w * ((double)i / 17.0); }

template <bool LDS>
__global__ __launch_bounds__(WAVE) void k_mosaic_fit(const MosArgs a) {
    __shared__ double s_tab[GROUPS][MOS_NP + 7];
    __shared__ double s_n[GROUPS][MOS_CAP], s_pa[GROUPS][MOS_CAP], s_pb[GROUPS][MOS_CAP];
    __shared__ int32_t s_r[GROUPS][MOS_CAP];
    const int lane = threadIdx.x, g = lane >> 4, li = lane & (ROW - 1), row0 = lane & ~(ROW - 1);
    const uint32_t n_small = a.counts[a.nwg], total = *a.total;
    const uint32_t begin = LDS ? 0u : n_small, end = LDS ? n_small : total;
    for (uint64_t base = (uint64_t)begin + (uint64_t)blockIdx.x * GROUPS; base < end; base += (uint64_t)gridDim.x * GROUPS) {
        const bool live = base + g < end;
        const int64_t c = live ? (int64_t)a.list[base + g] : 0;
        const int locus = live ? (int)(c / a.S) : -1 - g;
        // the table of the first group of the wave with this locus (the list is row-major: equal loci are neighbours)
        // (every lane of the wave shuffles, then compares: a shuffle reads only lanes that take part in it)
        int slot = g;
#pragma unroll
        for (int k = GROUPS - 1; k >= 0; --k) {
            const int locus_k = __shfl(locus, k * ROW, WAVE);
            if (k < g && locus_k == locus) slot = k;
        }
        wave_fence();   // the readers of the tables and records before are done
        if (live && slot == g && li < 3) {
            const double u = a.stutter[3 * (int64_t)locus], d = a.stutter[3 * (int64_t)locus + 1],
                         rho = a.stutter[3 * (int64_t)locus + 2];
            if (li == 2)
                s_tab[g][MOS_D] = 1 - u - d;
            else {   // lane 0: the expansions, lane 1: the deletions; (x * rho) * (1 - rho)^(k - 1) as StutterProb
                const double head = (li == 0 ? u : d) * rho, q = 1 - rho;
                double pw = 1.0;
                for (int k = 1; k <= MOS_D; ++k) {
                    s_tab[g][li == 0 ? MOS_D + k : MOS_D - k] = head * pw;
                    pw = pw * q;
                }
            }
        }
        wave_fence();
        Reads<LDS> rd;
        rd.tab = s_tab[slot];
        rd.R = 0;
        rd.A = rd.B = 0;
        int64_t o0 = 0;
        if (live) {
            o0 = a.off[c];
            rd.R = a.off[c + 1] - a.off[c];
            rd.A = a.ab[2 * c];
            rd.B = a.ab[2 * c + 1];
        }
        if (LDS) {
            for (int j = li; j < rd.R; j += ROW) {
                const int32_t r = a.val[o0 + j];
                s_r[g][j] = r;
                s_n[g][j] = (double)a.cnt[o0 + j];
                s_pa[g][j] = rd.tab[MOS_D + confine((int64_t)r - rd.A)];
                s_pb[g][j] = rd.tab[MOS_D + confine((int64_t)r - rd.B)];
            }
            rd.r = s_r[g];
            rd.n = s_n[g];
            rd.pa = s_pa[g];
            rd.pb = s_pb[g];
            rd.cnt = nullptr;
            wave_fence();
        } else {
            rd.r = a.val + o0;
            rd.cnt = a.cnt + o0;
            rd.n = rd.pa = rd.pb = nullptr;
        }
        if (!live) continue;   // (the lanes of a row leave together: every shuffle and ballot below is row-wide)
        const int32_t c_lo = rd.r[0] - 3, c_hi = rd.r[rd.R - 1] + 3;   // at most TRK_MOSAIC_MAX_SPAN candidates (select)

        auto c_step = [&](double f) -> int32_t {
            double best = -INFINITY;
            int32_t bc = INT32_MAX;
            for (int32_t c0 = c_lo; c0 <= c_hi; c0 += ROW) {
                const int32_t cand = c0 + li;
                double l1, l2;
                ll_both(rd, cand, f, l1, l2);
                const double ll = l2 > l1 ? l2 : l1;
                if (cand <= c_hi && ll > best) {
                    best = ll;
                    bc = cand;
                }
            }
#pragma unroll
            for (int o = 1; o < ROW; o <<= 1) {
                const double ob = __shfl_xor(best, o, ROW);
                const int32_t oc = __shfl_xor(bc, o, ROW);
                if (ob > best || (ob == best && oc < bc)) {
                    best = ob;
                    bc = oc;
                }
            }
            return bc == INT32_MAX ? 0 : bc;   // no candidate above -inf: the reference's c_final = 0
        };

        auto f_step = [&](int32_t C) -> double {
            double g1, g2;
            const double fe = (li & 1) ? 0.5 : 0.0;
            g_both(rd, C, fe, fe, g1, g2);
            const double g1_0 = __shfl(g1, row0, WAVE), g1_h = __shfl(g1, row0 + 1, WAVE);
            const double g2_0 = __shfl(g2, row0, WAVE), g2_h = __shfl(g2, row0 + 1, WAVE);
            const bool in1 = !(g1_0 <= 0.0) && !(g1_h >= 0.0), in2 = !(g2_0 <= 0.0) && !(g2_h >= 0.0);
            double f1 = g1_0 <= 0.0 ? 0.0 : 0.5, f2 = g2_0 <= 0.0 ? 0.0 : 0.5;
            if (in1 || in2) {
                double lo1 = 0.0, hi1 = 0.5, lo2 = 0.0, hi2 = 0.5;
                for (int it = 0; it < F_ROUNDS; ++it) {
                    const double w1 = hi1 - lo1, w2 = hi2 - lo2;
                    g_both(rd, C, bracket_point(lo1, w1, li + 1), bracket_point(lo2, w2, li + 1), g1, g2);
                    const int k1 = __popc((uint32_t)(__ballot(g1 > 0.0) >> row0) & 0xffffu);
                    const int k2 = __popc((uint32_t)(__ballot(g2 > 0.0) >> row0) & 0xffffu);
                    const double nlo1 = k1 ? bracket_point(lo1, w1, k1) : lo1, nhi1 = k1 < ROW ? bracket_point(lo1, w1, k1 + 1) : hi1;
                    const double nlo2 = k2 ? bracket_point(lo2, w2, k2) : lo2, nhi2 = k2 < ROW ? bracket_point(lo2, w2, k2 + 1) : hi2;
                    lo1 = nlo1;
                    hi1 = nhi1;
                    lo2 = nlo2;
                    hi2 = nhi2;
                }
                if (in1) f1 = 0.5 * (lo1 + hi1);
                if (in2) f2 = 0.5 * (lo2 + hi2);
            }
            double l1, l2;
            ll_both(rd, C, (li & 1) ? f2 : f1, l1, l2);
            const double best1 = __shfl(l1, row0, WAVE), best2 = __shfl(l2, row0 + 1, WAVE);
            return best2 > best1 ? f2 : f1;   // branch 1 wins ties
        };

        double f = 0.01;
        int32_t C = c_step(f);
        f = f_step(C);
        bool nonconv = false;
        for (int pair = 2; pair <= MAX_PAIRS + 1; ++pair) {
            const int32_t c_prev = C;
            const double f_prev = f;
            C = c_step(f);
            f = f_step(C);
            if (pair > MAX_PAIRS) {
                nonconv = true;
                break;
            }
            if (fabs(f - f_prev) < 0.01 && (f < 0.000001 || C == c_prev)) break;
        }
        double l1, l2;
        ll_both(rd, C, (li & 1) ? 0.0 : f, l1, l2);
        const double lmax = l2 > l1 ? l2 : l1;
        const double ll_null = __shfl(lmax, row0 + 1, WAVE);
        double ll_fit = __shfl(lmax, row0, WAVE);
        const bool no_c = f == 0.0;
        double pval = 1.0;
        int32_t sup = 0;
        if (no_c) {
            ll_fit = ll_null;
            C = 0;
        } else {
            const double t = -2 * (ll_null - ll_fit);
            pval = (t <= 0.0 ? 0.5 : 0.0) + 0.5 * exp(-(t > 0.0 ? t : 0.0) / 2);   // chi2.sf(t, 2), 1 below 0
            for (int j = 0; j < rd.R; ++j)
                if (rd.r[j] == C) sup = rd.cnt ? rd.cnt[j] : (int32_t)rd.n[j];
        }
        if (li == 0) {
            a.out_c[c] = C;
            a.out_f[c] = f;
            a.out_pval[c] = pval;
            a.out_llf[c] = ll_fit;
            a.out_ll0[c] = ll_null;
            a.out_sup[c] = sup;
            a.out_status[c] = (uint8_t)(TRK_MOSAIC_FIT | (no_c ? TRK_MOSAIC_NO_C : 0) | (nonconv ? TRK_MOSAIC_NONCONV : 0));
        }
    }
}

}  // namespace

namespace trk {

static int mosaic_select_wgs(int64_t n_calls) { return (int)((n_calls + SEL_THREADS - 1) / SEL_THREADS); }

size_t mosaic_workspace_bytes(int64_t n_calls) {
    return ((size_t)2 * mosaic_select_wgs(n_calls) + 4 + (size_t)n_calls) * sizeof(uint32_t);
}

hipError_t launch_mosaic_fit(const trk_mosaic_in& in, const trk_mosaic_out& out, void* workspace, int n_cu,
                             hipStream_t stream) {
    MosArgs a = {};
    a.L = in.n_loci;
    a.S = in.n_samples;
    a.n_calls = (int64_t)in.n_loci * in.n_samples;
    a.n_reads = in.n_reads;
    a.output_all = (in.flags & TRK_MOSAIC_OUTPUT_ALL) ? 1 : 0;
    a.fit_all = (in.flags & TRK_MOSAIC_FIT_ALL) ? 1 : 0;
    a.ab = in.ab;
    a.off = in.read_off;
    a.val = in.read_val;
    a.cnt = in.read_cnt;
    a.stutter = in.stutter;
    a.out_c = out.c;
    a.out_f = out.f;
    a.out_pval = out.pval;
    a.out_llf = out.ll_fit;
    a.out_ll0 = out.ll_null;
    a.out_sup = out.support;
    a.out_status = out.status;
    a.nwg = mosaic_select_wgs(a.n_calls);
    a.counts = static_cast<uint32_t*>(workspace);
    a.total = a.counts + 2 * (size_t)a.nwg;
    a.list = a.total + 4;
    hipLaunchKernelGGL(k_mosaic_select<0>, dim3(a.nwg), dim3(SEL_THREADS), 0, stream, a);
    hipError_t err = launch_scan_u32(a.counts, 2 * a.nwg, a.total, stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_mosaic_select<1>, dim3(a.nwg), dim3(SEL_THREADS), 0, stream, a);
    // the fit kernels size themselves from the scan's totals on the device: no host round trip.  A wave per workgroup,
    // walked with a grid stride so that calls of unequal cost spread over the CUs.
    const int64_t waves = (a.n_calls + GROUPS - 1) / GROUPS;
    const int grid_s = (int)(waves < (int64_t)n_cu * 32 ? waves : (int64_t)n_cu * 32);
    const int grid_l = (int)(waves < (int64_t)n_cu * 8 ? waves : (int64_t)n_cu * 8);
    hipLaunchKernelGGL(k_mosaic_fit<true>, dim3(grid_s), dim3(WAVE), 0, stream, a);
    hipLaunchKernelGGL(k_mosaic_fit<false>, dim3(grid_l), dim3(WAVE), 0, stream, a);
    return hipGetLastError();
}

}  // namespace trk
