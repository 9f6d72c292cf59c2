// trk_assoc_logit.hip -- associaTR logistic regression of a 0/1 outcome for gfx950 (trk_assoc_scan_logistic).
//
// The linear scan reduces a locus to cross-products in one streaming pass; the logistic weights mu (1 - mu) depend on
// the locus and change with every Newton step, so here a locus keeps its workgroup for the whole fit:
//
//   k_assoc_logit<RESIDENT>   one workgroup (8 waves) per locus that the scan + k_assoc_finalize left at TRK_AS_OK.
//     decode     every wave decodes ITS contiguous share of the locus's row (any ploidy, any alignment), standardises
//                the summed length with the finaliser's mean / std and -- RESIDENT -- leaves it in LDS as float64
//                (nan: not tested) for every later pass; it also counts the cases (sum y) for the start value and the
//                constant-outcome exit.  Rows beyond the LDS budget take <false>: the same code decodes again from
//                HBM in every pass, same order, same bits.
//     pass       64 samples per wave step.  Sample per lane: the 16 doubles of the sample's row of the sample-major
//                vector block (k_assoc_vect: [y, c_1..c_K, 1, 0..], 128 contiguous bytes, L2-resident across loci),
//                eta = x . b (b broadcast from LDS), ONE f64 exp, mu, w = mu (1 - mu), y - mu, log-likelihood term in
//                the last pass.  w, y - mu (and g when it is not resident) go to a wave-private LDS strip, lane ->
//                slot `lane`: 64 consecutive doubles, no bank conflict.  Then 16 x v_mfma_f64_16x16x4_f64, four
//                samples each: lane i reads sample 4 ks + i / 16, column i % 16 -- one coalesced 512-byte line of the
//                vector block, with column 0 (y) REPLACED by g, so the tile rows are [g, c_1..c_K, 1, 0..]; A = x,
//                B = w x in columns 0..14 and y - mu in column 15: D[:, 0..14] = X' W X, D[:, 15] = X' (y - mu) in
//                one accumulation.  The strip reads are four consecutive doubles, each broadcast to 16 lanes:
//                conflict-free as well.  (MFMA lane layout: trk_assoc.hip, k_assoc_scan_mfma.)
//     reduce     the 8 partial tiles are summed through LDS in wave order: no float atomics, a rerun gives the same
//                bits.
//     solve      wave 0: packed lower triangle of [1, c_1..c_K, g] + the gradient as one more row, left-looking
//                Cholesky as k_assoc_regress_wave<1> (same dropped-column rule; which columns are kept is decided in
//                the FIRST factorisation, where W is a constant times I), back-substitution lane-parallel, the step,
//                the convergence test; b and the decision go back to every wave through LDS.
//   After convergence one more pass at the final b gives the Hessian behind SE and the log-likelihood.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/trk.h"
#include "trk_internal.h"

namespace {

constexpr int WAVE = 64;
constexpr int LG_WAVES = 8;     // (16 waves leave 128 registers a lane: the pass spilled ~200 bytes a lane to scratch)
constexpr int LG_THREADS = WAVE * LG_WAVES;
constexpr int LG_MAX_STEPS = 30;
constexpr int LG_TRI = 16 * 17 / 2;                              // packed triangle of 15 design rows + the gradient row
constexpr int LG_FIXED = LG_WAVES * 256 + LG_TRI + 16 + 16 + 16 + 8;   // doubles in front of the strips
constexpr size_t LG_LDS_BUDGET = 160 * 1024;
typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

enum { LG_ITERATE = 0, LG_LAST_PASS = 1, LG_DONE = 2 };

struct LogitArgs {
    trk_batch b;
    const double* vect;        // [n64 * 64 rows at least][16]: y, c_1..c_K, 1, zeros; zero rows beyond S
    const uint8_t* sample_in;  // [S] or null
    const double* allele_len;  // [sumA]
    int32_t* locus_int;
    double* locus_f64;
    int K;                     // covariates
    int n64;                   // 64-sample steps of a row
};

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ double uniform_f64(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
    return v;
}

template <bool RESIDENT>
__global__ __launch_bounds__(LG_THREADS) void k_assoc_logit(const LogitArgs a) {
    extern __shared__ double lg_lds[];
    const int l = blockIdx.x;
    int32_t* li = a.locus_int + (size_t)l * TRK_AI_COLS;
    double* lf = a.locus_f64 + (size_t)l * TRK_AF_COLS;
    if (li[TRK_AI_STATUS] != TRK_AS_OK || li[TRK_AI_RANK] != -1) return;   // filtered by the scan: the whole workgroup leaves
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid >> 6;
    const int S = a.b.n_samples, K = a.K, P = K + 2;       // design columns [1, c_1..c_K, g]
    constexpr int HW = RESIDENT ? 2 : 3;                   // strips of a wave: w, y - mu (, g)
    double* red = lg_lds;                                  // [LG_WAVES][256]
    double* tri = red + LG_WAVES * 256;                    // packed lower triangle, rows 0..P
    double* b_sh = tri + LG_TRI;                           // [16] b in TILE order: g, c_1..c_K, 1, zeros
    double* sy_sh = b_sh + 16;                             // [16] per wave: cases
    double* ll_sh = sy_sh + 16;                            // [16] per wave: log-likelihood
    int* ctrl = reinterpret_cast<int*>(ll_sh + 16);        // [0] what the next pass is
    double* hand = lg_lds + LG_FIXED + (size_t)wid * HW * WAVE;
    double* g_lds = lg_lds + LG_FIXED + (size_t)LG_WAVES * HW * WAVE;   // RESIDENT: [n64 * 64]
#define AT(i, k) tri[(i) * ((i) + 1) / 2 + (k)]

    const double n_d = (double)li[TRK_AI_N_TESTED];
    const double mean = lf[TRK_AF_COLS - 1], sd = lf[TRK_AF_GT_STD];   // the pivoted mean k_assoc_finalize left for the regression
    const int ploidy = a.b.ploidy;
    const int pl = a.b.locus_ploidy ? a.b.locus_ploidy[l] : ploidy;
    const int off = a.b.allele_off[l];
    const int A = a.b.allele_off[l + 1] - off;
    const double pivot = a.allele_len[off];
    // standardised summed length of sample s as the scan sums it (k_assoc_scan_any); nan: not among the tested samples
    auto decode = [&](int s) -> double {
        if (s >= S || (a.sample_in && !a.sample_in[s])) return __builtin_nan("");
        const int16_t* cell = a.b.gt + ((int64_t)l * S + s) * ploidy;
        bool miss = false;
        double g = 0.0;
        for (int p = 0; p < pl; ++p) {
            const int al = cell[p];
            miss |= al == -1;
            if (al == -2) g += -2.0 - pivot;
            else if (al >= 0 && al < A) g += a.allele_len[off + al] - pivot;
        }
        return miss ? __builtin_nan("") : (g - mean) / sd;
    };
    const int per = (a.n64 + LG_WAVES - 1) / LG_WAVES;     // this wave's contiguous share of the 64-sample steps
    const int st0 = wid * per, st1 = st0 + per < a.n64 ? st0 + per : a.n64;

    // ---- decode pass: g into LDS, cases per wave ----------------------------------------------
    {
        double sy = 0.0;
        for (int st = st0; st < st1; ++st) {
            const int s = st * WAVE + lane;
            const double gz = decode(s);
            if (RESIDENT) g_lds[s] = gz;
            if (gz == gz) sy += a.vect[(size_t)s * 16];
        }
        sy = wave_sum_f64(sy);        // a sum of zeros and ones: exact in any order
        if (lane == 0) sy_sh[wid] = sy;
    }
    __syncthreads();
    double n_case = 0.0;
    for (int w = 0; w < LG_WAVES; ++w) n_case += sy_sh[w];
    if (n_case == 0.0 || n_case == n_d) {                  // no maximum-likelihood fit exists
        if (tid == 0) {
            li[TRK_AI_STATUS] = TRK_AS_CONSTANT_OUTCOME;
            li[TRK_AI_RANK] = 0;
            lf[TRK_AF_LOGLIK] = NAN;
        }
        return;
    }

    // ---- wave 0 keeps the fit's state: lane j < P holds b_j in DESIGN order [1, c_1..c_K, g] ----
    const int tile_of = lane == 0 ? K + 1 : (lane == P - 1 ? 0 : lane);    // design column `lane` -> tile row
    double b_l = 0.0;
    uint32_t kept = 0;
    int rank = 0, n_steps = 0;
    if (wid == 0) {
        const double ybar = n_case / n_d;
        if (lane == 0) b_l = log(ybar / (1.0 - ybar));
        if (lane < 16) b_sh[lane] = 0.0;
        wave_fence();
        if (lane == 0) {
            b_sh[K + 1] = b_l;
            ctrl[0] = LG_ITERATE;
        }
    }

    for (;;) {
        __syncthreads();              // b and the decision are visible; `red` is free again
        const int mode = ctrl[0];
        if (mode == LG_DONE) break;
        // ---- pass over this wave's share ------------------------------------------------------
        double bt[16];                // the same in every lane: kept in scalar registers
#pragma unroll
        for (int j = 0; j < 16; ++j) bt[j] = uniform_f64(b_sh[j]);
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
        double ll = 0.0;
        for (int st = st0; st < st1; ++st) {
            const int s = st * WAVE + lane;
            // sample per lane
            const double gz = RESIDENT ? g_lds[s] : decode(s);
            const bool tested = gz == gz;
            const double g0 = tested ? gz : 0.0;
            const d2* vr = reinterpret_cast<const d2*>(a.vect + (size_t)s * 16);
            double v[16];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const d2 t = vr[j];
                v[2 * j] = t[0];
                v[2 * j + 1] = t[1];
            }
            double eta = bt[0] * g0;
#pragma unroll
            for (int j = 1; j < 16; ++j) eta = __builtin_fma(bt[j], v[j], eta);
            const double e = exp(-fabs(eta));
            const double inv = 1.0 / (1.0 + e);
            const double small = e * inv;                       // the smaller of mu and 1 - mu
            const double mu = eta >= 0.0 ? inv : small;
            const double omu = eta >= 0.0 ? small : inv;        // 1 - mu without cancellation
            const double w = tested ? mu * omu : 0.0;
            const double r = tested ? (v[0] != 0.0 ? omu : -mu) : 0.0;
            if (mode == LG_LAST_PASS && tested) ll += v[0] * eta - (fmax(eta, 0.0) + log1p(e));
            hand[lane] = w;
            hand[WAVE + lane] = r;
            if (!RESIDENT) hand[2 * WAVE + lane] = g0;
            wave_fence();
            // four samples per matrix instruction
            const unsigned long long tm = __ballot(tested);
            const double* line = a.vect + (size_t)st * WAVE * 16 + lane;
#pragma unroll 4
            for (int ks = 0; ks < 16; ++ks) {
                const int src = 4 * ks + (lane >> 4);
                const double wk = hand[src], rk = hand[WAVE + src];
                const double gk = RESIDENT ? g_lds[st * WAVE + src] : hand[2 * WAVE + src];
                double x = line[ks * 64];
                x = (lane & 15) == 0 ? gk : x;
                x = ((tm >> src) & 1ull) ? x : 0.0;            // (a covariate of a sample outside the set may be anything)
                const double bv = (lane & 15) == 15 ? rk : wk * x;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, bv, acc, 0, 0, 0);
            }
            wave_fence();             // the strips are read: the next step may overwrite them
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wid * 256 + lane * 4 + r] = acc[r];
        ll = wave_sum_f64(ll);
        if (lane == 0) ll_sh[wid] = ll;
        __syncthreads();
        if (wid != 0) continue;

        // ---- wave 0: tiles in wave order -> packed triangle -------------------------------------
        double loglik = 0.0;
        for (int w = 0; w < LG_WAVES; ++w) loglik += ll_sh[w];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double sum = 0.0;
            for (int w = 0; w < LG_WAVES; ++w) sum += red[w * 256 + lane * 4 + r];
            // D[ti][tj], tile order [g, c_1..c_K, 1]; column 15 the gradient
            const int ti = 4 * r + (lane >> 4), tj = lane & 15;
            if (ti <= K + 1) {
                const int di = ti == 0 ? P - 1 : (ti == K + 1 ? 0 : ti);
                if (tj == 15) {
                    AT(P, di) = sum;
                } else if (tj <= K + 1) {
                    const int dj = tj == 0 ? P - 1 : (tj == K + 1 ? 0 : tj);
                    if (di >= dj) AT(di, dj) = sum;
                }
            }
        }
        wave_fence();
        // ---- left-looking Cholesky, rows j..P (row P: the gradient) updated for column j ---------
        const bool first = n_steps == 0 && mode == LG_ITERATE;
        bool lost = false;            // a kept column failed the pivot rule
        for (int j = 0; j < P; ++j) {
            double v = 0.0;
            if (lane >= j && lane <= P) {
                v = AT(lane, j);
                for (int k = 0; k < j; ++k) v -= AT(lane, k) * AT(j, k);
            }
            const double ajj = AT(j, j);
            const double d = __shfl(v, j, WAVE);
            wave_fence();
            const bool ok = d > 1e-11 * ajj;
            if (first) {
                if (ok) {
                    kept |= 1u << j;
                    ++rank;
                }
            } else if (((kept >> j) & 1u) && !ok) {
                lost = true;
            }
            if (ok && ((kept >> j) & 1u)) {
                const double ljj = sqrt(d);
                if (lane == j) AT(lane, j) = ljj;
                else if (lane > j && lane <= P) AT(lane, j) = v / ljj;
            } else if (lane >= j && lane <= P) {
                AT(lane, j) = 0.0;    // column in the span of the previous ones: out for good
            }
            wave_fence();
        }
        int status = -1;              // -1: go on
        if (first && !((kept >> (P - 1)) & 1u)) status = TRK_AS_COLLINEAR;
        else if (lost) status = TRK_AS_NOT_CONVERGED;
        double coef = NAN, se = NAN;
        if (status < 0 && mode == LG_LAST_PASS) {
            coef = __shfl(b_l, P - 1, WAVE);
            se = 1.0 / AT(P - 1, P - 1);                       // sqrt((H^-1)_gg) with g last
            status = TRK_AS_OK;
        } else if (status < 0) {
            // back-substitution L' delta = z: delta_k in lane k, lanes below k take their share of it
            double accv = 0.0, delta = 0.0;
            for (int k = P - 1; k >= 0; --k) {
                double mine = 0.0;
                if (lane == k && ((kept >> k) & 1u)) mine = (AT(P, k) - accv) / AT(k, k);
                const double dk = __shfl(mine, k, WAVE);
                if (lane == k) delta = dk;
                if (lane < k) accv += AT(k, lane) * dk;
            }
            b_l += delta;
            ++n_steps;
            const bool mine_in = lane < P;
            const double maxd = wave_max_f64(mine_in ? fabs(delta) : 0.0);
            const double maxb = wave_max_f64(mine_in ? fabs(b_l) : 0.0);
            const bool finite = __all(!mine_in || (b_l - b_l == 0.0));
            if (!finite) status = TRK_AS_NOT_CONVERGED;
            else if (maxd <= 1e-9 * fmax(1.0, maxb)) ctrl[0] = LG_LAST_PASS;   // every lane writes the same value
            else if (n_steps == LG_MAX_STEPS) status = TRK_AS_NOT_CONVERGED;
            if (mine_in) b_sh[tile_of] = b_l;
        }
        if (status >= 0) {
            if (lane == 0) {
                li[TRK_AI_STATUS] = status;
                li[TRK_AI_RANK] = rank;
                li[TRK_AI_N_ITER] = n_steps;
                lf[TRK_AF_LOGLIK] = NAN;
                if (status == TRK_AS_OK) {
                    const double z = coef / se;
                    lf[TRK_AF_COEF] = coef;
                    lf[TRK_AF_SE] = se;
                    lf[TRK_AF_TVALUE] = z;
                    lf[TRK_AF_PVAL] = erfc(fabs(z) * 0.70710678118654752440);
                    lf[TRK_AF_DF_RESID] = n_d - (double)rank;
                    lf[TRK_AF_LOGLIK] = loglik;
                }
            }
            ctrl[0] = LG_DONE;
        }
    }
#undef AT
}

}  // namespace

namespace trk {

// samples (rounded up to whole 64-sample steps) whose standardised genotypes fit in LDS beside the fixed areas
static int logit_resident_max() {
    return (int)((LG_LDS_BUDGET / 8 - LG_FIXED - (size_t)LG_WAVES * 2 * WAVE) / WAVE) * WAVE;
}

hipError_t launch_assoc_logit(const trk_batch& b, const trk_assoc_params& prm, const trk_assoc_out& out, const double* vect,
                              hipStream_t stream) {
    if (b.n_loci == 0) return hipSuccess;
    LogitArgs a{};
    a.b = b;
    a.vect = vect;
    a.sample_in = prm.sample_in;
    a.allele_len = prm.allele_len;
    a.locus_int = out.locus_int;
    a.locus_f64 = out.locus_f64;
    a.K = prm.n_vec - 1;
    a.n64 = (b.n_samples + WAVE - 1) / WAVE;
    const bool resident = a.n64 * WAVE <= logit_resident_max() && !trk_opt("TRK_AS_LOGIT_STREAM");
    const size_t lds = resident ? ((size_t)LG_FIXED + (size_t)LG_WAVES * 2 * WAVE + (size_t)a.n64 * WAVE) * 8
                                : ((size_t)LG_FIXED + (size_t)LG_WAVES * 3 * WAVE) * 8;
    void (*kern)(const LogitArgs) = resident ? &k_assoc_logit<true> : &k_assoc_logit<false>;
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kern, dim3(b.n_loci), dim3(LG_THREADS), lds, stream, a);
    return hipGetLastError();
}

}  // namespace trk
