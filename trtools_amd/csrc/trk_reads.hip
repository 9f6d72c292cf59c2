// trk_reads.hip -- prancSTR's read vectors parsed ON THE DEVICE: the 'bp|count;bp|count' field of every call of a batch
// of HipSTR records (MALLREADS) becomes the CSR arrays trk_mosaic_fit reads -- per call the distinct values bp // period
// in ascending order with their summed counts -- and the genotype indices become (A, B) in repeat units.
//
// What it replaces: ExtractReadVector + np.unique + ExtractAB per call in Python (prancSTR.py:220-247 of the reference;
// trtools_amd/prancSTR/prancSTR.py: mosaic_fit_records).  k_parse_samples cannot serve: its planes are scalars, a token
// longer than its 256 staged bytes is the host's, and its outputs are dense.
//
// The output is ragged, so there are two passes (trk_format_samples' protocol):
//   pass 1  k_reads_index         one workgroup per record: where every call's field starts and how long it is
//           k_reads_build<false>  sixteen lanes per call: the number of distinct values
//           k_reads_recsum / k_reads_recscan / k_reads_offsets: record flags, then the exclusive scan of the counts
//   pass 2  k_reads_build<true>   the same parse, the entries stored at read_off[c]
//           k_reads_ab            (A, B) from gt and the per-allele table
// No atomics anywhere: every output byte has one writer and every sum one order.
//
// k_reads_index walks the sample region in tiles of 16 KB like k_parse_samples, but keeps no text in LDS: per 16-byte
// chunk the tab mask (for the token starts) and the COLON mask, both from the same load.  A lane owns a token and finds
// its read_idx-th colon by hopping from chunk to chunk on the popcounts of the colon masks, then the next colon (the
// field's end).  A token that runs over the tile's edge leaves {colons still to find, field start, field end} in LDS and
// the first lane of the next tile goes on from there: no token is too long.  22 KB of LDS, seven workgroups per CU.
//
// k_reads_build gives a call a row of sixteen lanes (four calls per wave, k_mosaic_fit's row shape).  The lanes load the
// field sixteen bytes each into LDS; the ';' mask of each chunk and a prefix popcount across the row give every entry's
// first byte; lane e parses entries e, e + 16, ... (-?d{1,9}|d{1,9}) and floor-divides; the row ranks its entries by
// all-pairs comparison through LDS (value, then position: ranks are distinct), stores them in rank order, finds the first
// entry of every run of equal values with a ballot and sums each run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/trk.h"
#include "trk_internal.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_TILE = 16384;                 // bytes of text per tile of the index pass
constexpr int RD_CHUNKS = RD_TILE / 16;        // four per lane
constexpr int RD_MAXSEG = RD_TILE / 2 + 2;     // tokens that can start in a tile (one byte + a tab each) + the one carried in
constexpr int RB_ROW = 16;                     // lanes per call of the build pass
constexpr int RB_ROWS = RD_THREADS / RB_ROW;   // calls per workgroup
constexpr int RB_E = TRK_READS_MAX_ENTRIES;
constexpr int RB_CH = (TRK_READS_MAX_FIELD + 15 + 15) / 16 + 1;   // chunks a field can touch (it starts anywhere in its first)
constexpr int RB_ROUNDS = (RB_CH + RB_ROW - 1) / RB_ROW;
constexpr uint32_t RB_BAD = 0xffffffffu;       // a call's count: outside the device grammar
enum { ENT_OK = 0, ENT_STOP = 1, ENT_BAD = 2 };
static_assert(RB_E % RB_ROW == 0 && RB_E >= 64, "entries per row");

struct ReadsArgs {
    trk_reads_in in;
    trk_reads_out out;
};

// the caller's workspace (TRK_READS_WS_BYTES): what pass 1 leaves for pass 2, and the scan's intermediates
struct ReadsWs {
    int64_t* fstart;     // [L*S] offset in text of the call's field
    int32_t* flen;       // [L*S] its length, 0: no reads
    uint32_t* cnt;       // [L*S] distinct values, RB_BAD
    int64_t* rec_tot;    // [L]
    int64_t* rec_base;   // [L]
    int64_t* total;      // [1]
};

__host__ __device__ inline ReadsWs carve(void* ws, int64_t L, int64_t S) {
    ReadsWs w;
    char* p = static_cast<char*>(ws);
    w.fstart = reinterpret_cast<int64_t*>(p);
    p += 8 * L * S;
    w.rec_tot = reinterpret_cast<int64_t*>(p);
    p += 8 * L;
    w.rec_base = reinterpret_cast<int64_t*>(p);
    p += 8 * L;
    w.total = reinterpret_cast<int64_t*>(p);
    p += 16;
    w.flen = reinterpret_cast<int32_t*>(p);
    p += 4 * L * S;
    w.cnt = reinterpret_cast<uint32_t*>(p);
    return w;
}

__device__ __forceinline__ bool is_digit(unsigned char c) { return (unsigned)(c - '0') <= 9u; }

// bit i of the result: byte i of the 16-byte chunk equals the byte repeated in `pat`
__device__ __forceinline__ uint32_t eq_mask(const uint4 v, const uint32_t pat) {
    uint32_t m = 0;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = w[k] ^ pat;                                // a zero byte where the text has the byte
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 in every zero byte, carry-free
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
    }
    return m;
}

// The r-th (r >= 1) colon of the tile's bytes [pos, b): its position, or -1 with r reduced by the colons that are there.
// Whole chunks are stepped over on the popcount of their mask.
__device__ __forceinline__ int nth_colon(const uint16_t* col, int pos, const int b, int& r) {
    if (pos >= b) return -1;
    int ci = pos >> 4;
    uint32_t m = (uint32_t)col[ci] & (0xffffu << (pos & 15)) & 0xffffu;
    for (;;) {
        const int cb = ci << 4;
        if (b - cb < 16) m &= (1u << (b - cb)) - 1u;
        const int n = __popc(m);
        if (n >= r) {
            for (; r > 1; --r) m &= m - 1;
            return cb + __ffs((int)m) - 1;
        }
        r -= n;
        ++ci;
        if ((ci << 4) >= b) return -1;
        m = col[ci];
    }
}

__global__ __launch_bounds__(RD_THREADS) void k_reads_index(const ReadsArgs a) {
    __shared__ uint16_t s_cnt[RD_CHUNKS];          // tabs per chunk, then the tabs of the tile before the chunk
    __shared__ uint16_t s_col[RD_CHUNKS];          // colon mask per chunk
    __shared__ uint16_t s_seg[RD_MAXSEG + 1];      // s_seg[k], k >= 1: the byte after the tile's k-th tab
    __shared__ uint32_t s_wsum[RD_THREADS / 64];
    // the token that runs over the tile's edge: 0 looking for the field (s_crem colons to go), 1 inside it, 2 behind it
    __shared__ int32_t s_cph, s_crem;
    __shared__ int64_t s_cfs, s_cfe;
    const int rec = blockIdx.x;
    const int tid = threadIdx.x;
    const int S = a.in.n_samples;
    const int64_t r0 = a.in.smp_off[rec], r1 = a.in.line_end[rec];
    const int ridx = a.in.read_idx[rec];
    if (ridx < 0 || r1 <= r0) {                    // the record lacks the field: no reads, no flag; no sample columns at all
        if (tid == 0) a.out.flags[rec] = ridx < 0 ? 0 : TRK_PARSE_COLUMNS;
        return;
    }
    const ReadsWs ws = carve(a.out.workspace, a.in.n_records, S);
    const unsigned char* reg = a.in.text + r0;
    const int64_t n = r1 - r0;                               // bytes of the region; reg[n] is the newline
    const int64_t lead = (int64_t)((uintptr_t)reg & 15u);    // tiles start on 16-byte boundaries of the address
    const int64_t span = n + lead;
    if (tid == 0) {
        s_cph = 0;
        s_crem = ridx;
        s_cfs = 0;
        s_cfe = 0;
    }
    int64_t base = 0;                              // tabs of the tiles before this one = the sample of its segment 0
    uint32_t rflags = 0;
    for (int64_t t0 = 0; t0 < span; t0 += RD_TILE) {
        uint32_t mk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = tid + q * RD_THREADS;
            const int64_t o = t0 + (int64_t)c * 16 - lead;   // the chunk's first byte from the region's start
            uint32_t m = 0, cm = 0;
            if (o < n && o + 16 > 0) {
                const uint4 v = *reinterpret_cast<const uint4*>(reg + o);
                m = eq_mask(v, 0x09090909u);
                cm = eq_mask(v, 0x3a3a3a3au);                // (bytes outside the region are never looked at: segments end at n)
                if (o < 0) m &= ~((1u << (int)(-o)) - 1u);
                if (o + 16 > n) m &= (1u << (int)(n - o)) - 1u;
            }
            mk[q] = m;
            s_cnt[c] = (uint16_t)__popc(m);
            s_col[c] = (uint16_t)cm;
        }
        __syncthreads();
        // exclusive scan of the 1024 tab counts: lane t owns chunks 4t .. 4t + 3
        uint32_t own[4], sum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            own[q] = s_cnt[4 * tid + q];
            sum += own[q];
        }
        uint32_t incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
            if ((tid & 63) >= o) incl += y;
        }
        if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t wbase = 0;
        for (int w = 0; w < (tid >> 6); ++w) wbase += s_wsum[w];
        const uint32_t tile_tabs = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
        uint32_t run = wbase + incl - sum;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s_cnt[4 * tid + q] = (uint16_t)run;
            run += own[q];
        }
        __syncthreads();
        // segment k >= 1 starts behind the tile's k-th tab; segment 0 is the region's first token or the one carried in
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = tid + q * RD_THREADS;
            uint32_t m = mk[q];
            uint32_t k = 1u + s_cnt[c];
            while (m) {
                const int b = __ffs((int)m) - 1;
                m &= m - 1;
                if (k <= (uint32_t)RD_MAXSEG) s_seg[k] = (uint16_t)(c * 16 + b + 1);
                ++k;
            }
        }
        const int32_t cph = s_cph, crem = s_crem;            // read before this tile's last segment overwrites them
        const int64_t cfs = s_cfs, cfe = s_cfe;
        __syncthreads();
        const uint32_t nseg = 1u + tile_tabs;
        if (nseg > (uint32_t)RD_MAXSEG) {          // (uniform) more empty tokens than any record has: the host's
            rflags |= TRK_PARSE_HOST;
            base = (int64_t)S - 1;                 // (columns not counted to the end: no word on them)
            break;
        }
        const bool last_tile = t0 + RD_TILE >= span;
        const int tile_end = (int)(span - t0 < (int64_t)RD_TILE ? span - t0 : (int64_t)RD_TILE);
        const int64_t tile_abs = r0 - lead + t0;             // offset in text of the tile's first byte
        uint32_t lflags = 0;
        for (uint32_t k = tid; k < nseg; k += RD_THREADS) {
            const int64_t s = base + k;
            if (s >= S) {
                lflags |= TRK_PARSE_COLUMNS;
                continue;
            }
            int pos = k == 0 ? (t0 == 0 ? (int)lead : 0) : (int)s_seg[k];
            const int b = k + 1 < nseg ? (int)s_seg[k + 1] - 1 : tile_end;    // the token's tab, the newline or the tile's edge
            const bool closed = k + 1 < nseg || last_tile;
            const bool cont = k == 0 && t0 > 0;
            int ph = cont ? cph : 0, rem = cont ? crem : ridx;
            int64_t fs = cont ? cfs : 0, fe = cont ? cfe : 0;
            if (ph == 0) {
                if (rem == 0) {
                    fs = tile_abs + pos;
                    ph = 1;
                } else {
                    const int p = nth_colon(s_col, pos, b, rem);
                    if (p >= 0) {
                        pos = p + 1;
                        fs = tile_abs + pos;
                        ph = 1;
                    }
                }
            }
            if (ph == 1) {
                int one = 1;
                const int p = nth_colon(s_col, pos, b, one);
                if (p >= 0) {
                    fe = tile_abs + p;
                    ph = 2;
                }
            }
            if (closed) {
                if (ph == 1) fe = tile_abs + b;
                int64_t len = ph == 0 ? 0 : fe - fs;         // (a token that ends before the field: no reads)
                if (len > TRK_READS_MAX_FIELD) {
                    lflags |= TRK_PARSE_HOST;
                    len = 0;
                }
                ws.fstart[(int64_t)rec * S + s] = fs;
                ws.flen[(int64_t)rec * S + s] = (int32_t)len;
            } else {
                s_cph = ph;
                s_crem = rem;
                s_cfs = fs;
                s_cfe = fe;
            }
        }
        rflags |= (uint32_t)__syncthreads_or((int)lflags);
        base += tile_tabs;
    }
    if (tid == 0) {
        if (base + 1 != S) rflags |= TRK_PARSE_COLUMNS;      // fewer (or more) sample columns than the header announces
        a.out.flags[rec] = (uint8_t)rflags;
    }
}

// One field of the call's text t[p0, p1): an entry -?d{1,9}|d{1,9} (value = floor(bp / period)), a field without '|'
// (the vector ends before it), or something with a '|' that the device does not read.
__device__ __forceinline__ int parse_entry(const unsigned char* t, const int p0, const int p1, const int period, int& val, int& num) {
    int i = p0;
    const bool neg = i < p1 && t[i] == '-';
    if (neg) ++i;
    const int d0 = i;
    uint32_t u = 0;
    while (i < p1 && i - d0 < 10 && is_digit(t[i])) u = u * 10u + (uint32_t)(t[i++] - '0');
    bool ok = i > d0 && i - d0 <= 9 && i < p1 && t[i] == '|';
    if (ok) {
        const int d1 = ++i;
        uint32_t w = 0;
        while (i < p1 && i - d1 < 10 && is_digit(t[i])) w = w * 10u + (uint32_t)(t[i++] - '0');
        ok = i > d1 && i - d1 <= 9 && i == p1;
        if (ok) {
            const int bp = neg ? -(int)u : (int)u;
            int q = bp / period;
            if (bp % period != 0 && bp < 0) --q;             // Python's //: towards minus infinity (period >= 1)
            val = q;
            num = (int)w;
            return ENT_OK;
        }
    }
    for (i = p0; i < p1; ++i)
        if (t[i] == '|') return ENT_BAD;
    return ENT_STOP;
}

template <bool EMIT>
__global__ __launch_bounds__(RD_THREADS) void k_reads_build(const ReadsArgs a) {
    __shared__ uint4 s_text[RB_ROWS][RB_CH];       // the field's chunks as they lie in memory
    __shared__ uint16_t s_ent[RB_ROWS][RB_E + 2];  // first byte of field e in the row's text; field e ends at s_ent[e + 1] - 1
    __shared__ int32_t s_val[RB_ROWS][RB_E], s_num[RB_ROWS][RB_E];     // entries as parsed (num 0: not one)
    __shared__ int32_t s_sv[RB_ROWS][RB_E], s_sn[RB_ROWS][RB_E];       // in rank order
    const int tid = threadIdx.x;
    const int row = tid >> 4, lane = tid & 15;
    const int S = a.in.n_samples;
    const int64_t n_calls = (int64_t)a.in.n_records * S;
    const int64_t c = (int64_t)blockIdx.x * RB_ROWS + row;
    const ReadsWs ws = carve(a.out.workspace, a.in.n_records, S);
    int len = 0, period = 1;
    int64_t fs = 0;
    if (c < n_calls) {
        const int rec = (int)(c / S);
        if (a.out.flags[rec] == 0 && a.in.read_idx[rec] >= 0) {
            len = ws.flen[c];
            fs = ws.fstart[c];
            period = a.in.period[rec];
        }
    }
    const bool live = len > 0;
    if (!__syncthreads_or(live ? 1 : 0)) {         // (uniform) sixteen calls without reads
        if (!EMIT && lane == 0 && c < n_calls) ws.cnt[c] = 0;
        return;
    }
    // ---- the field into LDS, the start of every ';'-separated field of it ------------------------------------------
    const int lead = (int)(fs & 15);
    const int tot = lead + len;                    // the field is bytes [lead, tot) of the row's text
    const unsigned char* src = a.in.text + (fs - lead);
    int nsemi = 0;
#pragma unroll
    for (int r = 0; r < RB_ROUNDS; ++r) {
        const int j = r * RB_ROW + lane;
        uint32_t sm = 0;
        if (live && j * 16 < tot && j < RB_CH) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + j * 16);
            s_text[row][j] = v;
            sm = eq_mask(v, 0x3b3b3b3bu);
            if (j == 0) sm &= ~((1u << lead) - 1u);
            if (tot - j * 16 < 16) sm &= (1u << (tot - j * 16)) - 1u;
        }
        const int cnt = __popc(sm);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < RB_ROW; o <<= 1) {
            const int y = __shfl_up(incl, o, RB_ROW);
            if (lane >= o) incl += y;
        }
        int k = nsemi + incl - cnt + 1;            // the field that starts behind this lane's first ';'
        while (sm) {
            const int b = __ffs((int)sm) - 1;
            sm &= sm - 1;
            if (k <= RB_E + 1) s_ent[row][k] = (uint16_t)(j * 16 + b + 1);
            ++k;
        }
        nsemi += __shfl(incl, RB_ROW - 1, RB_ROW);
    }
    const int nf = nsemi + 1;                      // fields of the text
    if (live && lane == 0) {
        s_ent[row][0] = (uint16_t)lead;
        if (nf <= RB_E + 1) s_ent[row][nf] = (uint16_t)(tot + 1);
    }
    __syncthreads();
    // ---- lane e parses fields e, e + 16, ..; lane 0 also looks at field RB_E: one entry too many? -------------------
    const unsigned char* t = reinterpret_cast<const unsigned char*>(s_text[row]);
    int val[RB_E / RB_ROW], num[RB_E / RB_ROW];
    int first_stop = RB_E + 1, first_bad = RB_E + 1;
#pragma unroll
    for (int it = 0; it <= RB_E / RB_ROW; ++it) {
        const int e = it * RB_ROW + lane;
        int v = 0, m = 0;
        if (live && e < nf && e <= RB_E) {
            const int kind = parse_entry(t, s_ent[row][e], (int)s_ent[row][e + 1] - 1, period, v, m);
            if (kind == ENT_STOP) first_stop = e < first_stop ? e : first_stop;
            if (kind == ENT_BAD) first_bad = e < first_bad ? e : first_bad;
            if (kind != ENT_OK) m = 0;
        }
        if (it < RB_E / RB_ROW) {
            val[it] = v;
            num[it] = m;
        }
    }
#pragma unroll
    for (int o = 1; o < RB_ROW; o <<= 1) {
        const int x = __shfl_xor(first_stop, o, RB_ROW), y = __shfl_xor(first_bad, o, RB_ROW);
        first_stop = x < first_stop ? x : first_stop;
        first_bad = y < first_bad ? y : first_bad;
    }
    const int n_ent = first_stop < nf ? first_stop : nf;     // the fields before the first one without a '|'
    bool bad = live && (first_bad < n_ent || n_ent > RB_E);
    const int n_in = (!live || bad) ? 0 : n_ent;
#pragma unroll
    for (int it = 0; it < RB_E / RB_ROW; ++it) {
        const int e = it * RB_ROW + lane;
        if (e >= n_in) num[it] = 0;
        s_val[row][e] = val[it];
        s_num[row][e] = num[it];
    }
    __syncthreads();
    // ---- rank = the entries that sort before this one (value, then position); stored in rank order -------------------
    const int wrow = (tid & 63) >> 4;              // the row's place in its wave
    int n_valid = 0;
#pragma unroll
    for (int it = 0; it < RB_E / RB_ROW; ++it) {
        const int e = it * RB_ROW + lane;
        const bool valid = num[it] > 0;
        if (valid) {
            int rank = 0;
            for (int j = 0; j < n_in; ++j) {
                const int vj = s_val[row][j];
                rank += (s_num[row][j] > 0 && (vj < val[it] || (vj == val[it] && j < e))) ? 1 : 0;
            }
            s_sv[row][rank] = val[it];
            s_sn[row][rank] = num[it];
        }
        n_valid += __popc((uint32_t)(__ballot(valid) >> (16 * wrow)) & 0xffffu);
    }
    __syncthreads();
    // ---- the first entry of every run of equal values sums its run and stores it -----------------------------------
    const int64_t off = (EMIT && live) ? (int64_t)a.out.read_off[c] : 0;
    int nd = 0;
    bool over = false;
#pragma unroll
    for (int it = 0; it < RB_E / RB_ROW; ++it) {
        const int r = it * RB_ROW + lane;
        const bool head = r < n_valid && (r == 0 || s_sv[row][r] != s_sv[row][r - 1]);
        const uint32_t heads = (uint32_t)(__ballot(head) >> (16 * wrow)) & 0xffffu;
        if (head) {
            const int v = s_sv[row][r];
            int64_t sum = 0;
            for (int j = r; j < n_valid && s_sv[row][j] == v; ++j) sum += s_sn[row][j];
            if (sum > INT32_MAX) over = true;
            if (EMIT) {
                const int64_t o = off + nd + __popc(heads & ((1u << lane) - 1u));
                a.out.read_val[o] = v;
                a.out.read_cnt[o] = (int32_t)sum;
            }
        }
        nd += __popc(heads);
    }
    if (!EMIT) {
        bad = bad || ((uint32_t)(__ballot(over) >> (16 * wrow)) & 0xffffu) != 0;
        if (lane == 0 && c < n_calls) ws.cnt[c] = bad ? RB_BAD : (uint32_t)nd;
    }
}

// sum over the workgroup, known to every lane (s_w: one slot per wave)
__device__ __forceinline__ int64_t block_sum(int64_t x, int64_t* s_w) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// exclusive scan over the workgroup; total: the sum
__device__ __forceinline__ int64_t block_excl_scan(const int64_t x, int64_t* s_w, int64_t& total) {
    int64_t incl = x;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(incl, o, 64);
        if ((int)(threadIdx.x & 63) >= o) incl += y;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    int64_t wbase = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) wbase += s_w[w];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return wbase + incl - x;
}

// a record with a call outside the grammar is the host's; the others' number of entries
__global__ __launch_bounds__(RD_THREADS) void k_reads_recsum(const ReadsArgs a) {
    __shared__ int64_t s_w[RD_THREADS / 64];
    const int rec = blockIdx.x, S = a.in.n_samples;
    const ReadsWs ws = carve(a.out.workspace, a.in.n_records, S);
    const uint32_t f0 = a.out.flags[rec];
    int64_t sum = 0;
    int bad = 0;
    if (f0 == 0 && a.in.read_idx[rec] >= 0) {
        for (int s = threadIdx.x; s < S; s += RD_THREADS) {
            const uint32_t v = ws.cnt[(int64_t)rec * S + s];
            if (v == RB_BAD) bad = 1;
            else sum += v;
        }
    }
    bad = __syncthreads_or(bad);
    sum = block_sum(sum, s_w);
    if (threadIdx.x == 0) {
        const uint32_t f = f0 | (bad ? (uint32_t)TRK_PARSE_HOST : 0u);
        a.out.flags[rec] = (uint8_t)f;
        ws.rec_tot[rec] = f ? 0 : sum;
    }
}

// one workgroup: where every record's entries start, and the total
__global__ __launch_bounds__(RD_THREADS) void k_reads_recscan(const ReadsArgs a) {
    __shared__ int64_t s_w[RD_THREADS / 64];
    const int L = a.in.n_records;
    const ReadsWs ws = carve(a.out.workspace, L, a.in.n_samples);
    int64_t run = 0;
    for (int l0 = 0; l0 < L; l0 += RD_THREADS) {
        const int l = l0 + (int)threadIdx.x;
        int64_t total;
        const int64_t ex = block_excl_scan(l < L ? ws.rec_tot[l] : 0, s_w, total);
        if (l < L) ws.rec_base[l] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) {
        ws.total[0] = run;
        a.out.read_off[(int64_t)L * a.in.n_samples] = (int32_t)(run < INT32_MAX ? run : INT32_MAX);
    }
}

__global__ __launch_bounds__(RD_THREADS) void k_reads_offsets(const ReadsArgs a) {
    __shared__ int64_t s_w[RD_THREADS / 64];
    const int rec = blockIdx.x, S = a.in.n_samples;
    const ReadsWs ws = carve(a.out.workspace, a.in.n_records, S);
    const bool none = a.out.flags[rec] != 0 || a.in.read_idx[rec] < 0;
    int64_t run = ws.rec_base[rec];
    for (int s0 = 0; s0 < S; s0 += RD_THREADS) {
        const int s = s0 + (int)threadIdx.x;
        int64_t total;
        const int64_t ex = block_excl_scan((s < S && !none) ? (int64_t)ws.cnt[(int64_t)rec * S + s] : 0, s_w, total);
        if (s < S) a.out.read_off[(int64_t)rec * S + s] = (int32_t)(run + ex);
        run += total;
    }
}

// ab = floor(allele_bp[gt] / period) per haplotype (ExtractAB's numbers in repeat units), both NOCALL_AB without a full call
__global__ __launch_bounds__(RD_THREADS) void k_reads_ab(const ReadsArgs a) {
    const int S = a.in.n_samples;
    const int64_t n_calls = (int64_t)a.in.n_records * S;
    const int64_t c = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x;
    if (c >= n_calls) return;
    const int rec = (int)(c / S);
    const int32_t a0 = a.in.allele_off[rec], na = a.in.allele_off[rec + 1] - a0;
    const int g0 = a.in.gt[2 * c], g1 = a.in.gt[2 * c + 1];
    int32_t A = TRK_MOSAIC_NOCALL_AB, B = TRK_MOSAIC_NOCALL_AB;
    if (a.out.flags[rec] == 0 && g0 >= 0 && g1 >= 0 && g0 < na && g1 < na) {
        const int period = a.in.period[rec];
        const int x = a.in.allele_bp[a0 + g0], y = a.in.allele_bp[a0 + g1];
        A = x / period - ((x % period != 0 && x < 0) ? 1 : 0);
        B = y / period - ((y % period != 0 && y < 0) ? 1 : 0);
    }
    a.out.ab[2 * c] = A;
    a.out.ab[2 * c + 1] = B;
}

}  // namespace

namespace trk {

hipError_t launch_parse_reads(const trk_reads_in& in, const trk_reads_out& out, int pass, hipStream_t stream, int64_t** total_dev) {
    const ReadsArgs a{in, out};
    const int64_t n_calls = (int64_t)in.n_records * in.n_samples;
    const dim3 per_rec((unsigned)in.n_records), per_row((unsigned)((n_calls + RB_ROWS - 1) / RB_ROWS)), blk(RD_THREADS);
    if (pass == 1) {
        hipLaunchKernelGGL(k_reads_index, per_rec, blk, 0, stream, a);
        hipLaunchKernelGGL(k_reads_build<false>, per_row, blk, 0, stream, a);
        hipLaunchKernelGGL(k_reads_recsum, per_rec, blk, 0, stream, a);
        hipLaunchKernelGGL(k_reads_recscan, dim3(1), blk, 0, stream, a);
        hipLaunchKernelGGL(k_reads_offsets, per_rec, blk, 0, stream, a);
        *total_dev = carve(out.workspace, in.n_records, in.n_samples).total;
    } else {
        hipLaunchKernelGGL(k_reads_build<true>, per_row, blk, 0, stream, a);
        if (in.gt) hipLaunchKernelGGL(k_reads_ab, dim3((unsigned)((n_calls + RD_THREADS - 1) / RD_THREADS)), blk, 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace trk
