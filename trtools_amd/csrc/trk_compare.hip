// trk_compare.hip -- compareSTR's per-record body over a batch of matched record pairs, for gfx950.
//
// Reference loop (one Python iteration per pair of records, trtools/compareSTR/compareSTR.py:508-693, a dozen numpy
// temporaries each): both-called mask (:550-554), ploidy check (:568-572), phasedness (:578-584), sequence and length
// concordance of the (sorted or ordered) haplotype tuples (:586-604), the sums of allele lengths relative to the
// reference and their moments (:606-607, :633-640), FORMAT-bin stratification (:642-693).  The semantics are stated in
// include/trk.h (trk_compare).  Here: ONE pass over the two genotype tensors (8 B per call, + 4 B per stratify plane);
// with phase planes a pre-pass reads both tensors once more beside the planes (8 + 2 B per call: the pass then moves 18).
//
//   k_cmp_mode      pre-pass, only with phase planes and without ignore_phasing: a workgroup per locus decides sorted /
//                   ordered / mixed.  The mode of a locus is known only after its whole row; the per-sample counters
//                   depend on it; so the main kernel reads it as an input instead of carrying both hypotheses.
//   k_cmp_scan<V>   column-owner tiling (k_qc_scan4's): a thread owns V consecutive samples (4: diploid, S % 4 == 0, one
//                   nontemporal 16-byte load per side and locus; 1: any ploidy, any S), a workgroup owns 256 * V columns
//                   x a contiguous range of loci, launched through the XCD-aware 1-D map.  The range is walked in LDS
//                   blocks of up to CMP_LB loci: the JOINT allele tables of both sides packed {seq_id:16, len_id:16}
//                   (one ds_read_b32 per haplotype) with dlen beside them; a locus whose alleles do not fit is served
//                   from the global tables (uniform branch).  Diploid: the sorted compare of two packed pairs is
//                   {a,b} against {a,b} or {b,a}; decisions become 64-bit lane masks, per-locus counts popcounts of
//                   ballots; the per-sample counters stay in registers over the whole range and leave once.  The five
//                   moments of a wave go through LDS transposed (k_qc_scan4's reduction: eight lanes per moment add
//                   eight columns each, three butterfly steps), the waves' results of a block of loci are staged in LDS,
//                   added in wave order and leave as whole 64-byte rows, one per (column tile, locus).  Stratified
//                   sums: accumulators in LDS, (bin, 8) per wave for the CURRENT period slot -- per present bin a masked
//                   butterfly, eight lanes add the totals; when the slot changes and at the end the four waves' copies
//                   are added in wave order into the workgroup's OWN row of the partial table (no atomics: program
//                   order, reproducible).  The block's allele offsets are staged in LDS (one load each).
//   k_cmp_finish_*  partials added in a fixed order into the outputs: per sample (added INTO the caller's int64
//                   accumulators), per locus, and per (slot, bin) (bin 0 = no FORMAT stratification, from the per-locus
//                   totals in locus order).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/trk.h"
#include "../../include/trk_test.h"
#include "trk_internal.h"

namespace {

constexpr int WAVE = 64;
constexpr int CMP_THREADS = 256;
constexpr int CMP_WAVES = CMP_THREADS / WAVE;
static_assert(CMP_WAVES == 4, "flush_bins and store_block add the four waves' copies by name");
constexpr int CMP_LB = 16;      // loci per LDS block
constexpr int CMP_CAP = 2048;   // allele entries (both sides) per LDS block: 8 KB packed ids + 16 KB dlen
constexpr int CMP_EDGES = TRK_CMP_MAX_BINS + TRK_CMP_MAX_FIELDS;
constexpr uint32_t ENT_ABSENT = 0xffffffffu;   // a -2 haplotype: ',' / -2 on both sides (tr_harmonizer.py:969-971, :1239)
constexpr uint32_t ENT_BAD = 0xfffefffeu;      // an allele index outside the record's alleles (the locus is flagged)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct CmpArgs {
    int L, S, P;
    int s_pad, gx, gy, lpw;
    const int16_t* gt[2];
    const int32_t* aoff[2];
    const uint16_t* sid[2];
    const uint16_t* lid[2];
    const double* dlen[2];
    const uint8_t* ph[2];
    const double* dabs;      // [L] dlen of a -2 haplotype
    const uint8_t* mode;     // [L] 0 sorted, 1 ordered, 2 mixed (flagged; compared as sorted); null: all sorted
    const uint8_t* slot;     // [L] or null
    int n_slots, n_fields, nbf;
    const void* pl[TRK_CMP_MAX_FIELDS][2];
    int is_f32[TRK_CMP_MAX_FIELDS], sfile[TRK_CMP_MAX_FIELDS], e0[TRK_CMP_MAX_FIELDS], ne[TRK_CMP_MAX_FIELDS],
        bin0[TRK_CMP_MAX_FIELDS];
    double edges[CMP_EDGES];
    float edges_f[CMP_EDGES];
    uint32_t* p_samp;   // [gy][3][s_pad]
    uint32_t* l_int;    // [gx][L]: flags of the column tile
    double* l_f64;      // [gx][L][8]: numcalls, conc_seq, conc_len (exact in float64), sums of x, y, xx, xy, yy
    double* b_part;     // [gy * gx][n_slots][nbf][8]: n, conc_seq, conc_len, x, y, xx, xy, yy per workgroup
};

// the sum over the wave, the same bits on every lane (a + b == b + a at every level of the butterfly)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the bin [e_i, e_{i+1}) that holds v, the last one closed on both ends (compareSTR.py:646-664); -1: none (nan fails
// every comparison).  T is the type numpy compares in: float32 for a float32 plane, float64 for an int32 plane.
template <class T>
__device__ __forceinline__ int find_bin(T v, const T* e, int n_edges) {
    int r = -1;
    for (int i = 0; i + 1 < n_edges; ++i) {
        const bool hi = (i + 2 == n_edges) ? (v <= e[i + 1]) : (v < e[i + 1]);
        if (v >= e[i] && hi) r = i;
    }
    return r;
}

struct Tab {              // where a locus's joint tables are
    bool lds;
    const uint32_t* ent;  // LDS: packed entries of the block
    const double* dl;     // LDS: dlen of the block
    int o[2];             // LDS: first entry of each side's alleles of this locus
    int64_t g[2];         // global: allele_off[l] of each side
    int A[2];
    double dabs;
};

__device__ __forceinline__ void look(const CmpArgs& a, const Tab& t, int side, int idx, uint32_t& ent, double& d) {
    if (idx == -2) {
        ent = ENT_ABSENT;
        d = t.dabs;
    } else if (idx < 0 || idx >= t.A[side]) {
        ent = ENT_BAD;
        d = 0.0;
    } else if (t.lds) {
        ent = t.ent[t.o[side] + idx];
        d = t.dl[t.o[side] + idx];
    } else {
        const int64_t at = t.g[side] + idx;
        ent = (uint32_t)a.sid[side][at] | ((uint32_t)a.lid[side][at] << 16);
        d = a.dlen[side][at];
    }
}

// one sample's stratified contribution, wave-wide: for every bin present among the lanes a masked butterfly, then lanes
// 0..7 add the eight totals into this wave's row
__device__ __forceinline__ void strat_add(int bin, bool cs, bool cl, double x, double y, double* dst, int lane) {
    uint64_t rem = __ballot(bin >= 0);
    while (rem) {
        const int first = __ffsll((unsigned long long)rem) - 1;
        const int b = __shfl(bin, first, WAVE);
        const bool in = bin == b;
        const uint64_t m = __ballot(in);
        rem &= ~m;
        const double vx = in ? x : 0.0, vy = in ? y : 0.0;
        const double sx = wave_sum(vx), sy = wave_sum(vy), sxx = wave_sum(vx * vx), sxy = wave_sum(vx * vy),
                     syy = wave_sum(vy * vy);
        const double n = (double)__popcll(m), ns = (double)__popcll(__ballot(in && cs)),
                     nl = (double)__popcll(__ballot(in && cl));
        if (lane < 8) {
            const double v = lane == 0 ? n : lane == 1 ? ns : lane == 2 ? nl : lane == 3 ? sx : lane == 4 ? sy
                           : lane == 5 ? sxx : lane == 6 ? sxy : syy;
            dst[(size_t)b * 8 + lane] += v;
        }
    }
}

template <int V>
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_scan(const CmpArgs a) {
    __shared__ uint32_t t_ent[CMP_CAP];
    __shared__ double t_dl[CMP_CAP];
    __shared__ alignas(16) double r_mom[CMP_WAVES][5][WAVE];        // a wave's five moments of one locus, transposed for the column sums
    __shared__ double stage[CMP_WAVES][CMP_LB][8];      // a block's per-locus results per wave: n, conc_seq, conc_len, 5 moments
    __shared__ uint32_t stage_fl[CMP_WAVES][CMP_LB];
    extern __shared__ double acc[];                     // [CMP_WAVES][nbf * 8]: the FORMAT bins of the CURRENT slot, per wave (dynamic)
    __shared__ int sh_off[2][CMP_LB + 1];               // allele_off of the block's loci
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid >> 6;
    const int S = a.S, L = a.L, P = a.P;
    // 1-D launch, XCD-aware (k_qc_scan4's map): the column tiles of a range of loci run on one XCD
    const int bslot = (int)blockIdx.x >> 3;
    const int bx = bslot % a.gx, by = ((int)blockIdx.x & 7) + 8 * (bslot / a.gx);
    if (by >= a.gy) return;
    const int64_t s0 = ((int64_t)bx * CMP_THREADS + tid) * V;
    const bool live = s0 < S;   // V == 4: S % 4 == 0, a thread's samples are all in range or all out
    const int l_begin = by * a.lpw, l_end = min(L, l_begin + a.lpw);
    const int64_t col4 = live ? (s0 >> 2) : 0, row4 = (int64_t)(S >> 2);
    uint32_t nc[V], ncs[V], ncl[V];
#pragma unroll
    for (int j = 0; j < V; ++j) nc[j] = ncs[j] = ncl[j] = 0;
    double* my_bins = a.nbf ? a.b_part + ((size_t)by * a.gx + bx) * a.n_slots * a.nbf * 8 : nullptr;
    int cur_slot = 0;
    const int nb8 = a.nbf * 8;
    for (int i = tid; i < CMP_WAVES * nb8; i += CMP_THREADS) acc[i] = 0.0;
    // the workgroup's bins of the current slot leave for its row of the partial table: the four waves in wave order (the
    // workgroup is the row's only writer: plain adds in program order)
    auto flush_bins = [&]() {
        __syncthreads();
        for (int i = tid; i < a.nbf * 8; i += CMP_THREADS) {
            const double v = ((acc[i] + acc[nb8 + i]) + acc[2 * nb8 + i]) + acc[3 * nb8 + i];
            if (v != 0.0) my_bins[(size_t)cur_slot * nb8 + i] += v;
            acc[i] = acc[nb8 + i] = acc[2 * nb8 + i] = acc[3 * nb8 + i] = 0.0;
        }
        __syncthreads();
    };

    auto locus = [&](int l, int li, const Tab& t) {
        const bool ordered = a.mode && a.mode[l] == 1;
        bool called[V], cs[V], cl[V], mism = false, bad = false;
        double x[V], y[V];
        if (V == 4) {
            u32x4 w1 = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, w2 = w1;
            if (live) {
                w1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.gt[0]) + (int64_t)l * row4 + col4);
                w2 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.gt[1]) + (int64_t)l * row4 + col4);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int a0 = (int16_t)(w1[j] & 0xffffu), a1 = (int16_t)(w1[j] >> 16);
                const int b0 = (int16_t)(w2[j] & 0xffffu), b1 = (int16_t)(w2[j] >> 16);
                called[j] = a0 != -1 && a1 != -1 && b0 != -1 && b1 != -1;
                uint32_t ea0, ea1, eb0, eb1;
                double da0, da1, db0, db1;
                look(a, t, 0, a0, ea0, da0);
                look(a, t, 0, a1, ea1, da1);
                look(a, t, 1, b0, eb0, db0);
                look(a, t, 1, b1, eb1, db1);
                mism |= called[j] && ((a0 == -2) + (a1 == -2) != (b0 == -2) + (b1 == -2));
                bad |= called[j] && (ea0 == ENT_BAD || ea1 == ENT_BAD || eb0 == ENT_BAD || eb1 == ENT_BAD);
                // sorted tuples are equal exactly when {a,b} == {a,b} or {a,b} == {b,a}: ids alone, no order needed
                const uint32_t d00 = ea0 ^ eb0, d11 = ea1 ^ eb1, d01 = ea0 ^ eb1, d10 = ea1 ^ eb0;
                const bool s_str = ((d00 | d11) & 0xffffu) == 0, s_swp = ((d01 | d10) & 0xffffu) == 0;
                const bool l_str = ((d00 | d11) >> 16) == 0, l_swp = ((d01 | d10) >> 16) == 0;
                cs[j] = called[j] && (s_str || (!ordered && s_swp));
                cl[j] = called[j] && (l_str || (!ordered && l_swp));
                x[j] = called[j] ? da0 + da1 : 0.0;
                y[j] = called[j] ? db0 + db1 : 0.0;
            }
        } else {
            called[0] = cs[0] = cl[0] = false;
            x[0] = y[0] = 0.0;
            if (live) {
                uint16_t sq[2][TRK_MAX_PLOIDY], ln[2][TRK_MAX_PLOIDY];
                double sum[2] = {0.0, 0.0};
                int absent[2] = {0, 0};
                bool c = true, bd = false;
                for (int k = 0; k < 2; ++k) {
                    const int16_t* g = a.gt[k] + ((int64_t)l * S + s0) * P;
                    for (int p = 0; p < P; ++p) {
                        const int idx = g[p];
                        uint32_t e;
                        double d;
                        look(a, t, k, idx, e, d);
                        c &= idx != -1;
                        bd |= e == ENT_BAD;
                        absent[k] += idx == -2;
                        sq[k][p] = (uint16_t)(e & 0xffffu);
                        ln[k][p] = (uint16_t)(e >> 16);
                        sum[k] += d;
                    }
                }
                called[0] = c;
                mism = c && absent[0] != absent[1];
                bad = c && bd;
                if (c) {
                    if (!ordered) {   // any total order sorts: equal sorted tuples == equal multisets
                        for (int k = 0; k < 2; ++k)
                            for (int p = 1; p < P; ++p)
                                for (int q = p; q > 0; --q) {
                                    if (sq[k][q] < sq[k][q - 1]) {
                                        const uint16_t u = sq[k][q];
                                        sq[k][q] = sq[k][q - 1];
                                        sq[k][q - 1] = u;
                                    }
                                    if (ln[k][q] < ln[k][q - 1]) {
                                        const uint16_t u = ln[k][q];
                                        ln[k][q] = ln[k][q - 1];
                                        ln[k][q - 1] = u;
                                    }
                                }
                    }
                    bool es = true, el = true;
                    for (int p = 0; p < P; ++p) {
                        es &= sq[0][p] == sq[1][p];
                        el &= ln[0][p] == ln[1][p];
                    }
                    cs[0] = es;
                    cl[0] = el;
                    x[0] = sum[0];
                    y[0] = sum[1];
                }
            }
        }
        uint32_t n = 0, nseq = 0, nlen = 0;
        double lx = 0.0, ly = 0.0, lxx = 0.0, lxy = 0.0, lyy = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            nc[j] += called[j];
            ncs[j] += cs[j];
            ncl[j] += cl[j];
            n += (uint32_t)__popcll(__ballot(called[j]));
            nseq += (uint32_t)__popcll(__ballot(cs[j]));
            nlen += (uint32_t)__popcll(__ballot(cl[j]));
            lx += x[j];
            ly += y[j];
            lxx += x[j] * x[j];
            lxy += x[j] * y[j];
            lyy += y[j] * y[j];
        }
        const uint32_t flags = (__ballot(mism) ? TRK_CMP_F_PLOIDY : 0u) | (__ballot(bad) ? TRK_CMP_F_BAD : 0u);
        // the five sums over the wave in a fixed order: transposed through LDS, eight lanes per moment add eight
        // consecutive lanes' values each, three butterfly steps add the eight column sums (k_qc_scan4's reduction)
        r_mom[wid][0][lane] = lx;
        r_mom[wid][1][lane] = ly;
        r_mom[wid][2][lane] = lxx;
        r_mom[wid][3][lane] = lxy;
        r_mom[wid][4][lane] = lyy;
        wave_fence();
        const int mk = min(lane >> 3, 4), p8 = lane & 7;
        const double2* rp = reinterpret_cast<const double2*>(&r_mom[wid][mk][p8 * 8]);
        const double2 q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3];
        double msum = ((q0.x + q0.y) + (q1.x + q1.y)) + ((q2.x + q2.y) + (q3.x + q3.y));
        msum += __shfl_xor(msum, 1, WAVE);
        msum += __shfl_xor(msum, 2, WAVE);
        msum += __shfl_xor(msum, 4, WAVE);
        wave_fence();
        if (lane < 40 && p8 == 0) stage[wid][li][3 + mk] = msum;
        if (lane < 24 && p8 == 1) stage[wid][li][mk] = (double)(mk == 0 ? n : mk == 1 ? nseq : nlen);
        if (lane == 63) stage_fl[wid][li] = flags;
        if (a.nbf) {
            const int sl = a.slot ? min((int)a.slot[l], a.n_slots - 1) : 0;   // (uniform over the workgroup)
            if (sl != cur_slot) {
                flush_bins();
                cur_slot = sl;
            }
        }
        if (a.nbf && n) {   // (uniform over the wave)
            double* dst = acc + wid * nb8;
            for (int f = 0; f < a.n_fields; ++f) {
                int bin[2][V];
                for (int k = 0; k < 2; ++k) {
#pragma unroll
                    for (int j = 0; j < V; ++j) bin[k][j] = -1;
                    if (!a.pl[f][k] || !live) continue;
                    if (a.is_f32[f]) {
                        float v[V];
                        if (V == 4) {
                            const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.pl[f][k]) + (int64_t)l * row4 + col4);
#pragma unroll
                            for (int j = 0; j < V; ++j) v[j] = q[j];
                        } else
                            v[0] = static_cast<const float*>(a.pl[f][k])[(int64_t)l * S + s0];
#pragma unroll
                        for (int j = 0; j < V; ++j) bin[k][j] = find_bin<float>(v[j], a.edges_f + a.e0[f], a.ne[f]);
                    } else {
                        int32_t v[V];
                        if (V == 4) {
                            const i32x4 q = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(a.pl[f][k]) + (int64_t)l * row4 + col4);
#pragma unroll
                            for (int j = 0; j < V; ++j) v[j] = q[j];
                        } else
                            v[0] = static_cast<const int32_t*>(a.pl[f][k])[(int64_t)l * S + s0];
#pragma unroll
                        for (int j = 0; j < V; ++j) bin[k][j] = find_bin<double>((double)v[j], a.edges + a.e0[f], a.ne[f]);
                    }
                }
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    // stratify_file 0: both sides in the same bin (:648-649); 1 / 2: that side alone (:651, :653)
                    int b = a.sfile[f] == 1 ? bin[0][j] : a.sfile[f] == 2 ? bin[1][j] : (bin[0][j] == bin[1][j] ? bin[0][j] : -1);
                    b = (called[j] && b >= 0) ? a.bin0[f] + b : -1;
                    strat_add(b, cs[j], cl[j], x[j], y[j], dst, lane);
                }
            }
        }
    };

    int lb = l_begin;
    while (lb < l_end) {
        __syncthreads();   // the readers of the block before are done
        const int nmax = min(CMP_LB, l_end - lb);
        if (tid < 2 * (CMP_LB + 1)) {   // the block's offsets: one load each, then every thread sizes the block from LDS
            const int k = tid / (CMP_LB + 1), i = tid % (CMP_LB + 1);
            if (i <= nmax) sh_off[k][i] = a.aoff[k][lb + i];
        }
        __syncthreads();
        int n = 0, tot = 0;
        while (n < nmax) {
            const int na = (sh_off[0][n + 1] - sh_off[0][n]) + (sh_off[1][n + 1] - sh_off[1][n]);
            if (na < 0 || tot + na > CMP_CAP) break;
            tot += na;
            ++n;
        }
        // the block's per-locus results: the four waves added in wave order, whole 64-byte rows stored side by side
        auto store_block = [&](int cnt) {
            __syncthreads();
            if (tid < cnt * 8) {
                const int li = tid >> 3, k = tid & 7;
                a.l_f64[((size_t)bx * L + lb + li) * 8 + k] = ((stage[0][li][k] + stage[1][li][k]) + stage[2][li][k]) + stage[3][li][k];
            } else if (tid >= 128 && tid < 128 + cnt) {
                const int li = tid - 128;
                a.l_int[(size_t)bx * L + lb + li] = stage_fl[0][li] | stage_fl[1][li] | stage_fl[2][li] | stage_fl[3][li];
            }
        };
        Tab t;
        t.ent = t_ent;
        t.dl = t_dl;
        if (n == 0) {   // this locus's alleles do not fit: the global tables
            t.lds = false;
            for (int k = 0; k < 2; ++k) {
                t.g[k] = sh_off[k][0];
                t.A[k] = sh_off[k][1] - sh_off[k][0];
                t.o[k] = 0;
            }
            t.dabs = a.dabs[lb];
            locus(lb, 0, t);
            store_block(1);
            ++lb;
            continue;
        }
        const int base0 = sh_off[0][0], cnt0 = sh_off[0][n] - base0;
        const int base1 = sh_off[1][0], cnt1 = sh_off[1][n] - base1;
        for (int i = tid; i < cnt0; i += CMP_THREADS) {
            t_ent[i] = (uint32_t)a.sid[0][base0 + i] | ((uint32_t)a.lid[0][base0 + i] << 16);
            t_dl[i] = a.dlen[0][base0 + i];
        }
        for (int i = tid; i < cnt1; i += CMP_THREADS) {
            t_ent[cnt0 + i] = (uint32_t)a.sid[1][base1 + i] | ((uint32_t)a.lid[1][base1 + i] << 16);
            t_dl[cnt0 + i] = a.dlen[1][base1 + i];
        }
        __syncthreads();
        t.lds = true;
        for (int li = 0; li < n; ++li) {
            t.o[0] = sh_off[0][li] - base0;
            t.o[1] = cnt0 + sh_off[1][li] - base1;
            t.A[0] = sh_off[0][li + 1] - sh_off[0][li];
            t.A[1] = sh_off[1][li + 1] - sh_off[1][li];
            t.g[0] = t.g[1] = 0;
            t.dabs = a.dabs[lb + li];
            locus(lb + li, li, t);
        }
        store_block(n);
        lb += n;
    }
    if (a.nbf) flush_bins();
    if (live) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const size_t at = (size_t)by * 3 * a.s_pad + s0 + j;
            a.p_samp[at] = nc[j];
            a.p_samp[at + a.s_pad] = ncs[j];
            a.p_samp[at + 2 * (size_t)a.s_pad] = ncl[j];
        }
    }
}

// phasedness of a locus over its both-called samples (compareSTR.py:578-584): a workgroup per locus
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_mode(const CmpArgs a, uint8_t* mode) {
    const int l = blockIdx.x, P = a.P;
    int any_un = 0, any_ph = 0;
    for (int s = threadIdx.x; s < a.S; s += CMP_THREADS) {
        const int64_t c = (int64_t)l * a.S + s;
        bool called = true;
        if (P == 2) {   // a diploid call is one aligned 32-bit word: coalesced 4-byte loads
            const uint32_t u = reinterpret_cast<const uint32_t*>(a.gt[0])[c], v = reinterpret_cast<const uint32_t*>(a.gt[1])[c];
            called = (u & 0xffffu) != 0xffffu && (u >> 16) != 0xffffu && (v & 0xffffu) != 0xffffu && (v >> 16) != 0xffffu;
        } else
            for (int p = 0; p < P; ++p) called &= a.gt[0][c * P + p] != -1 && a.gt[1][c * P + p] != -1;
        if (!called) continue;
        const bool un = a.ph[0][c] == 0 && a.ph[1][c] == 0;
        any_un |= un;
        any_ph |= !un;
    }
    any_un = __syncthreads_or(any_un);
    any_ph = __syncthreads_or(any_ph);
    if (threadIdx.x == 0) mode[l] = (any_un && any_ph) ? 2 : any_ph ? 1 : 0;
}

__global__ void k_cmp_zero(double* p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.0;
}

// sample_int[c][s] += the ranges' partial counters, in range order
__global__ __launch_bounds__(256) void k_cmp_finish_sample(const CmpArgs a, int n_real, int64_t* out) {
    const int s = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (s >= n_real) return;
    int64_t v = 0;
    for (int r = 0; r < a.gy; ++r) v += a.p_samp[((size_t)r * 3 + c) * a.s_pad + s];
    out[(size_t)c * n_real + s] += v;
}

// per locus: the column tiles added in tile order
__global__ __launch_bounds__(256) void k_cmp_finish_locus(const CmpArgs a, const uint8_t* mode, int32_t* li, double* lf) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= a.L) return;
    uint32_t n = 0, ns = 0, nl = 0, fl = (mode && mode[l] == 2) ? TRK_CMP_F_PHASE : 0u;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < a.gx; ++r) {
        const size_t at = (size_t)r * a.L + l;
        n += (uint32_t)a.l_f64[at * 8];
        ns += (uint32_t)a.l_f64[at * 8 + 1];
        nl += (uint32_t)a.l_f64[at * 8 + 2];
        fl |= a.l_int[at];
#pragma unroll
        for (int k = 0; k < 5; ++k) m[k] += a.l_f64[at * 8 + 3 + k];
    }
    li[(size_t)l * 4] = (int32_t)n;
    li[(size_t)l * 4 + 1] = (int32_t)ns;
    li[(size_t)l * 4 + 2] = (int32_t)nl;
    li[(size_t)l * 4 + 3] = (int32_t)(n ? fl : 0u);
#pragma unroll
    for (int k = 0; k < 5; ++k) lf[(size_t)l * 5 + k] = m[k];
}

// bin 0 of a slot (no FORMAT stratification, compareSTR.py:632-640): the per-locus totals of the slot's loci, 256
// contiguous chunks in locus order, the chunk sums in chunk order.  A workgroup per slot.
__global__ __launch_bounds__(256) void k_cmp_finish_all(const CmpArgs a, const int32_t* li, const double* lf, int NB,
                                                         int64_t* bi, double* bf) {
    __shared__ double sh[8][256];
    const int sl = blockIdx.x, tid = threadIdx.x;
    const int per = (a.L + 255) / 256, l0 = tid * per, l1 = min(a.L, l0 + per);
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int l = l0; l < l1; ++l) {
        const int s = a.slot ? min((int)a.slot[l], a.n_slots - 1) : 0;
        if (s != sl) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] += (double)li[(size_t)l * 4 + k];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[3 + k] += lf[(size_t)l * 5 + k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k][tid] = v[k];
    __syncthreads();
    if (tid >= 8) return;
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += sh[tid][i];
    if (tid < 3) bi[((size_t)sl * NB) * 3 + tid] += (int64_t)t;
    else bf[((size_t)sl * NB) * 5 + tid - 3] += t;
}

// the FORMAT bins: the workgroups' rows, four slices of them each in (range, tile) order, the slices in slice order
__global__ __launch_bounds__(256) void k_cmp_finish_bins(const CmpArgs a, int NB, int64_t* bi, double* bf) {
    __shared__ double sh[4][64];
    const int col = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + col;
    const int per = a.n_slots * a.nbf * 8;
    const int np = a.gy * a.gx, each = (np + 3) / 4, p0 = slice * each, p1 = min(np, p0 + each);
    double part = 0.0;
    if (i < per)
        for (int p = p0; p < p1; ++p) part += a.b_part[(size_t)p * per + i];
    sh[slice][col] = part;
    __syncthreads();
    if (slice || i >= per) return;
    const double t = ((sh[0][col] + sh[1][col]) + sh[2][col]) + sh[3][col];
    const int k = i & 7, b = (i >> 3) % a.nbf, sl = (i >> 3) / a.nbf;
    if (k < 3) bi[((size_t)sl * NB + 1 + b) * 3 + k] += (int64_t)t;
    else bf[((size_t)sl * NB + 1 + b) * 5 + k - 3] += t;
}

}  // namespace

namespace trk {

static int cmp_total_bins(const trk_compare_in& in) {
    int nb = 0;
    for (int f = 0; f < in.n_fields; ++f) nb += in.field[f].n_edges - 1;
    return nb;
}

static void cmp_geometry(const trk_compare_in& in, int n_cu, int& V, int& gx, int& gy, int& lpw) {
    bool al = in.ploidy == 2 && (in.n_samples % 4) == 0;
    for (int k = 0; k < 2; ++k) al = al && (reinterpret_cast<uintptr_t>(in.side[k].gt) & 15) == 0;
    for (int f = 0; f < in.n_fields; ++f)
        for (int k = 0; k < 2; ++k) al = al && (reinterpret_cast<uintptr_t>(in.field[f].plane[k].data) & 15) == 0;
    if (trk_opt("TRK_CMP_GENERAL")) al = false;
    V = al ? 4 : 1;
    gx = (in.n_samples + CMP_THREADS * V - 1) / (CMP_THREADS * V);
    int wgcu = 8;
    if (const char* o = trk_opt("TRK_CMP_WGCU")) wgcu = atoi(o) > 0 ? atoi(o) : wgcu;
    gy = n_cu * wgcu / gx;
    const int max_gy = (in.n_loci + 63) / 64;
    if (gy > max_gy) gy = max_gy;
    if (gy < 1) gy = 1;
    lpw = (in.n_loci + gy - 1) / gy;
    lpw = (lpw + CMP_LB - 1) / CMP_LB * CMP_LB;
    gy = (in.n_loci + lpw - 1) / lpw;
}

size_t compare_workspace_bytes(const trk_compare_in& in, int n_cu) {
    int V, gx, gy, lpw;
    cmp_geometry(in, n_cu, V, gx, gy, lpw);
    const size_t s_pad = (size_t)gx * CMP_THREADS * V;
    const size_t nbf = (size_t)cmp_total_bins(in);
    return (size_t)gx * in.n_loci * (64 + 4) + (size_t)gy * gx * in.n_slots * nbf * 64 + (size_t)gy * 3 * s_pad * 4 +
           (size_t)in.n_loci + 512;
}

hipError_t launch_compare(const trk_compare_in& in, const trk_compare_out& out, void* workspace, int n_cu,
                          hipStream_t stream) {
    int V, gx, gy, lpw;
    cmp_geometry(in, n_cu, V, gx, gy, lpw);
    CmpArgs a = {};
    a.L = in.n_loci;
    a.S = in.n_samples;
    a.P = in.ploidy;
    a.gx = gx;
    a.gy = gy;
    a.lpw = lpw;
    a.s_pad = gx * CMP_THREADS * V;
    for (int k = 0; k < 2; ++k) {
        a.gt[k] = in.side[k].gt;
        a.aoff[k] = in.side[k].allele_off;
        a.sid[k] = in.side[k].seq_id;
        a.lid[k] = in.side[k].len_id;
        a.dlen[k] = in.side[k].dlen;
        a.ph[k] = in.side[k].phased;
    }
    a.dabs = in.dlen_absent;
    a.slot = in.slot;
    a.n_slots = in.n_slots;
    a.n_fields = in.n_fields;
    int e = 0, b = 0;
    for (int f = 0; f < in.n_fields; ++f) {
        const trk_compare_field& fl = in.field[f];
        a.is_f32[f] = fl.plane[fl.stratify_file == 2 ? 1 : 0].dtype == TRK_DT_F32;
        a.sfile[f] = fl.stratify_file;
        // only the side(s) the rule reads (compareSTR.py:647-653)
        a.pl[f][0] = fl.stratify_file != 2 ? fl.plane[0].data : nullptr;
        a.pl[f][1] = fl.stratify_file != 1 ? fl.plane[1].data : nullptr;
        a.e0[f] = e;
        a.ne[f] = fl.n_edges;
        a.bin0[f] = b;
        for (int i = 0; i < fl.n_edges; ++i) {
            a.edges[e + i] = fl.edges[i];
            a.edges_f[e + i] = (float)fl.edges[i];
        }
        e += fl.n_edges;
        b += fl.n_edges - 1;
    }
    a.nbf = b;
    const int NB = 1 + b;
    unsigned char* w = static_cast<unsigned char*>(workspace);
    const size_t nl = (size_t)gx * a.L, nbp = (size_t)gy * gx * a.n_slots * a.nbf * 8;
    a.l_f64 = reinterpret_cast<double*>(w);
    a.b_part = a.l_f64 + nl * 8;
    a.l_int = reinterpret_cast<uint32_t*>(a.b_part + nbp);
    a.p_samp = a.l_int + nl;
    uint8_t* mode = reinterpret_cast<uint8_t*>(a.p_samp + (size_t)gy * 3 * a.s_pad);
    const bool phase = in.side[0].phased && in.side[1].phased && !in.ignore_phasing;
    if (phase) {
        hipLaunchKernelGGL(k_cmp_mode, dim3(a.L), dim3(CMP_THREADS), 0, stream, a, mode);
        a.mode = mode;
    }
    if (nbp) hipLaunchKernelGGL(k_cmp_zero, dim3(512), dim3(256), 0, stream, a.b_part, nbp);
    const dim3 grid(gx * ((gy + 7) / 8 * 8));
    if (V == 4)
        hipLaunchKernelGGL(k_cmp_scan<4>, grid, dim3(CMP_THREADS), (size_t)CMP_WAVES * a.nbf * 64, stream, a);
    else
        hipLaunchKernelGGL(k_cmp_scan<1>, grid, dim3(CMP_THREADS), (size_t)CMP_WAVES * a.nbf * 64, stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int n_real = in.n_samples - in.n_pad_samples;
    hipLaunchKernelGGL(k_cmp_finish_sample, dim3((n_real + 255) / 256, 3), dim3(256), 0, stream, a, n_real, out.sample_int);
    hipLaunchKernelGGL(k_cmp_finish_locus, dim3((a.L + 255) / 256), dim3(256), 0, stream, a, a.mode, out.locus_int,
                       out.locus_f64);
    hipLaunchKernelGGL(k_cmp_finish_all, dim3(a.n_slots), dim3(256), 0, stream, a, out.locus_int, out.locus_f64, NB,
                       out.bin_int, out.bin_f64);
    if (a.nbf)
        hipLaunchKernelGGL(k_cmp_finish_bins, dim3((a.n_slots * a.nbf * 8 + 63) / 64), dim3(256), 0, stream, a, NB,
                           out.bin_int, out.bin_f64);
    return hipGetLastError();
}

}  // namespace trk
