// potential.hip — the first half of Johnson's algorithm: Bellman-Ford potentials of a
// graph with signed weights, negative-cycle detection, the reweighting of the edge list
// and the back-transform of a solved row (no reference counterpart: the reference
// hard-codes w = 1, ParallelJohnson.cpp:147).
//
// h[v] = min(0, min over u of d(u, v)): the Bellman-Ford fixpoint from h = 0 everywhere
// (a virtual source with a zero-weight edge to every vertex). It is unique, and
// w'(u, v) = w(u, v) + h[u] - h[v] >= 0 for every edge, so the non-negative solvers
// (delta.hip) run unchanged on w' and give d'(s, v) = d(s, v) + h[s] - h[v].
//
// The rounds run on a temporary CSR by source of (dst | w << 32) records, built from
// the device COO before the graph's own CSR (whose rows are weight-sorted, so they
// must be built from the reduced weights). State per vertex: one u64 key
// (h biased by 2^31) << 32 | pred, so that distance and predecessor change in one
// 64-bit atomic. The frontier is a bitmap; the first one holds the tails of the negative
// edges (from h = 0 nothing else can improve anything). Round r reads bitmap r % 3,
// marks improved targets in bitmap (r + 1) % 3 and clears bitmap (r + 2) % 3; a ring of
// three flags (the scheme of tree.hip's zero-weight levels) says whether round r's
// frontier holds anything, so that the rounds enqueued past the fixpoint exit at once
// and read nothing. All of it is allocated and initialised by the load itself.
//
// An improvement must be STRICT (cand < h[v]) and is applied by a compare-and-swap on
// the key: a plain atomicMin on the packed key would also replace the predecessor of an
// EQUAL h by a smaller id, and a predecessor set without a strict improvement can close
// a zero-weight cycle in the predecessor graph, which the check below would report as
// negative. With strict updates every cycle of the predecessor graph has negative
// weight (the edge that closes it had h[v] > h[u] + w, all others h[v] >= h[u] + w).
//
// Negative cycles: after every batch of PT_BATCH rounds that leaves a frontier, pointer
// jumping over pred (ceil(log2 n) + 1 steps, as validate_tree's bad_cycle) finds the
// chains that do not end at a vertex without a predecessor; the vertex such a chain is
// stuck on lies on a predecessor cycle. n rounds without a fixpoint is the backstop.
#include "devutil.h"

namespace pj {

namespace {

constexpr int PT_LONG_ROW = 32;  // rows longer than this are walked by the whole wave
constexpr int PT_BATCH = 32;     // rounds enqueued per host check (and per cycle check)
constexpr i64 PT_H_MIN = -((i64)1 << 30);
constexpr u32 PT_NONE = 0xffffffffu;
constexpr u64 PT_KEY0 = ((u64)0x80000000u << 32) | PT_NONE;  // h = 0, no predecessor

struct PotCnt {
    u64 relaxed;    // edge records read by the rounds
    u64 rounds;     // rounds that had a frontier
    u64 negative;   // input entries with w < 0
    u64 bad;        // reweighted entries below 0 or above u32 (none, by the fixpoint)
    u32 range;      // a candidate fell below -2^30
    u32 cyc;        // min vertex a predecessor chain is stuck on (PT_NONE: none)
    int32_t hmin;   // min h
    u32 flags[3];   // ring: flags[r % 3] != 0 <=> round r's frontier holds a vertex
};

__device__ __forceinline__ int32_t key_h(u64 k) { return (int32_t)((u32)(k >> 32) ^ 0x80000000u); }
__device__ __forceinline__ u64 make_key(int32_t h, u32 pred) {
    return ((u64)((u32)h ^ 0x80000000u) << 32) | pred;
}

// negative entries: count them and mark their tails in the first frontier
__global__ void pot_init_k(const u32* __restrict__ src, const u32* __restrict__ w, i64 nnz, u64* __restrict__ f0,
                           PotCnt* __restrict__ c) {
    u64 neg = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (i64)gridDim.x * blockDim.x)
        if ((int32_t)w[i] < 0) {
            const u32 u = src[i];
            atomicOr(&f0[u >> 6], 1ull << (u & 63));
            ++neg;
        }
    neg = wave_sum(neg);
    if (lane_id() == 0 && neg) atomicAdd(&c->negative, neg);
}

__global__ void pot_fill_k(u64* __restrict__ key, i64 n) {
    for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (i64)gridDim.x * blockDim.x) key[v] = PT_KEY0;
}

__global__ void pot_pack_k(const u32* __restrict__ src, const u32* __restrict__ dst, const u32* __restrict__ w,
                           u32* __restrict__ key, u64* __restrict__ rec, i64 nnz) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (i64)gridDim.x * blockDim.x) {
        key[i] = src[i];
        rec[i] = (u64)dst[i] | ((u64)w[i] << 32);
    }
}

// one relaxation u -> v; true when v improved (and was marked in the next frontier)
__device__ __forceinline__ bool pot_relax(u32 u, int32_t hu, u64 r, u64* __restrict__ key, u64* __restrict__ fnext,
                                          u32& range) {
    const u32 v = (u32)r;
    const i64 cand = (i64)hu + (i64)(int32_t)(u32)(r >> 32);  // (64-bit: no int32 overflow)
    if (cand >= 0) return false;                              // (h never exceeds 0)
    if (cand < PT_H_MIN) {
        range = 1;
        return false;
    }
    u64 cur = key[v];
    const u64 nk = make_key((int32_t)cand, u);
    while (cand < (i64)key_h(cur)) {
        const u64 old = atomicCAS(&key[v], cur, nk);
        if (old == cur) {
            atomicOr(&fnext[v >> 6], 1ull << (v & 63));
            return true;
        }
        cur = old;
    }
    return false;
}

// Round r: the vertices of frontier word i are the lanes of one wave. Short rows are
// walked by their lane, long rows by the whole wave (tree.hip for_reached_edges).
template <typename Off>
__global__ __launch_bounds__(256) void pot_round_k(const Off* __restrict__ row, const u64* __restrict__ rec, i64 n,
                                                   i64 nwords, u32 r, u64* __restrict__ key, u64* __restrict__ fb,
                                                   PotCnt* __restrict__ c) {
    if (blockIdx.x == 0 && threadIdx.x == 0) c->flags[(r + 2) % 3] = 0;  // (round r + 2's; set by round r + 1)
    if (c->flags[r % 3] == 0) return;  // (block-uniform: this frontier is empty, and so is every later one)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&c->rounds, 1ull);
    const u64* fcur = fb + (size_t)(r % 3) * (size_t)nwords;
    u64* fnext = fb + (size_t)((r + 1) % 3) * (size_t)nwords;
    u64* fclr = fb + (size_t)((r + 2) % 3) * (size_t)nwords;
    const int lane = lane_id();
    const i64 wstride = ((i64)gridDim.x * blockDim.x) >> 6;
    u64 scanned = 0;
    u32 any = 0, range = 0;
    for (i64 wi = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wi < nwords; wi += wstride) {
        const u64 bits = fcur[wi];
        if (lane == 0) fclr[wi] = 0;
        if (!bits) continue;  // (wave-uniform)
        const i64 u = wi * 64 + lane;
        const bool ok = ((bits >> lane) & 1ull) && u < n;
        const int32_t hu = ok ? key_h(key[u]) : 0;
        const Off b = ok ? row[u] : 0, e = ok ? row[u + 1] : 0;
        const bool lng = ok && e - b > (Off)PT_LONG_ROW;
        if (ok && !lng) {
            for (Off k = b; k < e; ++k) any |= pot_relax((u32)u, hu, rec[k], key, fnext, range);
            scanned += (u64)(e - b);
        }
        u64 m = __ballot(lng);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const Off kb = __shfl(b, l, 64), ke = __shfl(e, l, 64);
            const i64 ul = __shfl(u, l, 64);
            const int32_t hl = __shfl(hu, l, 64);
            for (Off k = kb + (Off)lane; k < ke; k += WAVE) {
                any |= pot_relax((u32)ul, hl, rec[k], key, fnext, range);
                ++scanned;
            }
        }
    }
    scanned = wave_sum(scanned);
    if (lane == 0 && scanned) atomicAdd(&c->relaxed, scanned);
    if (__ballot(any) && lane == 0) atomicOr(&c->flags[(r + 1) % 3], 1u);
    if (__ballot(range) && lane == 0) atomicOr(&c->range, 1u);
}

__global__ void pot_anc_k(const u64* __restrict__ key, i64 n, u32* __restrict__ anc) {
    for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (i64)gridDim.x * blockDim.x)
        anc[v] = (u32)key[v];
}

// one pointer-jumping step in place (any ancestor stays an ancestor; PT_NONE = the chain ended)
__global__ void pot_jump_k(u32* __restrict__ anc, i64 n) {
    for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (i64)gridDim.x * blockDim.x) {
        const u32 a = anc[v];
        if (a != PT_NONE) anc[v] = anc[a];
    }
}

__global__ void pot_stuck_k(const u32* __restrict__ anc, i64 n, PotCnt* __restrict__ c) {
    u32 m = PT_NONE;
    for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (i64)gridDim.x * blockDim.x) m = min(m, anc[v]);
    m = ~wave_max(~m);
    if (lane_id() == 0 && m != PT_NONE) atomicMin(&c->cyc, m);
}

__global__ void pot_out_k(const u64* __restrict__ key, i64 n, int32_t* __restrict__ h, PotCnt* __restrict__ c) {
    int32_t m = 0;
    for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (i64)gridDim.x * blockDim.x) {
        const int32_t x = key_h(key[v]);
        h[v] = x;
        m = min(m, x);
    }
    m = -wave_max(-m);
    if (lane_id() == 0 && m < 0) atomicMin(&c->hmin, m);
}

// w := w + h[src] - h[dst] as u32
__global__ void pot_reweight_k(const u32* __restrict__ src, const u32* __restrict__ dst, u32* __restrict__ w,
                               const int32_t* __restrict__ h, i64 nnz, PotCnt* __restrict__ c) {
    u64 bad = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (i64)gridDim.x * blockDim.x) {
        const i64 x = (i64)(int32_t)w[i] + (i64)h[src[i]] - (i64)h[dst[i]];
        bad += x < 0 || x > 0xFFFFFFFFll;
        w[i] = (u32)x;
    }
    bad = wave_sum(bad);
    if (lane_id() == 0 && bad) atomicAdd(&c->bad, bad);
}

// out[v] of a solved row in reduced space (pj.h, "signed graphs"): in place when out == dred
__global__ void signed_correct_k(const int32_t* dred, const int32_t* __restrict__ h, i64 n, i64 source,
                                 int32_t* out, u64* __restrict__ capped) {
    const i64 hs = (source >= 0 && source < n) ? (i64)h[source] : 0;
    u64 cap = 0;
    for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (i64)gridDim.x * blockDim.x) {
        const int32_t dr = dred[v];
        int32_t o = INT_INF;
        if (dr < INT_INF) {
            const i64 d = (i64)dr - hs + (i64)h[v];
            if (d < (i64)INT_INF) o = (int32_t)d;
            else ++cap;
        }
        out[v] = o;
    }
    if (capped) {
        cap = wave_sum(cap);
        if (lane_id() == 0 && cap) atomicAdd(capped, cap);
    }
}

int key_bits(i64 n) {
    int b = 0;
    while (b < 32 && ((u64)1 << b) < (u64)n) ++b;
    return b;
}

// the rounds; returns PJ_OK, PJ_ERR_NEGCYCLE or PJ_ERR_RANGE
template <typename Off>
int pot_rounds(Ctx& ctx, const u32* src, const u32* dst, const u32* w, i64 nnz, i64 n, u64* key, u64* fb, i64 nwords,
               PotCnt* cnt, PotCnt& hc, i64& cycle_checks, hipEvent_t e0) {
    hipStream_t s = ctx.stream;
    const unsigned cap = (unsigned)ctx.cu_count * 8u;
    DevBuf<Off> row((size_t)n + 1);
    DevBuf<u64> rec((size_t)nnz), ralt((size_t)nnz);
    u64* rr = rec.p;
    {
        DevBuf<u32> k((size_t)nnz), kalt((size_t)nnz);
        SortWs ws;
        pot_pack_k<<<grid_for(nnz, 256, 8192), 256, 0, s>>>(src, dst, w, k.p, rec.p, nnz);
        PJ_LAUNCH_CHECK();
        u32* kr = k.p;
        radix_sort_pairs<u64>(k.p, kalt.p, rec.p, ralt.p, nnz, key_bits(n), ws, s, &kr, &rr);
        csr_bounds<Off>(kr, nnz, n, row.p, s);
        PJ_HIP(hipStreamSynchronize(s));  // (the keys and the sort workspace are freed here)
    }
    (rr == rec.p ? ralt : rec).release();
    DevBuf<u32> anc;
    const unsigned rgrid = grid_for(nwords * 64, 256, cap);
    int jumps = 1;
    while (((i64)1 << (jumps - 1)) < n) ++jumps;  // ceil(log2 n) + 1
    PJ_HIP(hipEventRecord(e0, s));  // (kernel_ms: the rounds and the reweighting, not the sort)
    for (u32 r = 0;;) {
        for (int b = 0; b < PT_BATCH; ++b, ++r) {
            pot_round_k<Off><<<rgrid, 256, 0, s>>>(row.p, rr, n, nwords, r, key, fb, cnt);
            PJ_LAUNCH_CHECK();
        }
        PJ_HIP(hipMemcpyAsync(&hc, cnt, sizeof(PotCnt), hipMemcpyDeviceToHost, s));
        PJ_HIP(hipStreamSynchronize(s));
        const bool open = hc.flags[r % 3] != 0;
        if (!open && !hc.range) break;
        // a frontier is left (or a potential fell out of range): look for a predecessor cycle
        anc.ensure((size_t)n);
        const unsigned g = grid_for(n, 256, cap);
        pot_anc_k<<<g, 256, 0, s>>>(key, n, anc.p);
        PJ_LAUNCH_CHECK();
        for (int j = 0; j < jumps; ++j) {
            pot_jump_k<<<g, 256, 0, s>>>(anc.p, n);
            PJ_LAUNCH_CHECK();
        }
        pot_stuck_k<<<g, 256, 0, s>>>(anc.p, n, cnt);
        PJ_LAUNCH_CHECK();
        ++cycle_checks;
        PJ_HIP(hipMemcpyAsync(&hc, cnt, sizeof(PotCnt), hipMemcpyDeviceToHost, s));
        PJ_HIP(hipStreamSynchronize(s));
        if (hc.cyc != PT_NONE) return PJ_ERR_NEGCYCLE;
        if (hc.range) return PJ_ERR_RANGE;
        if ((i64)hc.rounds >= n) return PJ_ERR_NEGCYCLE;  // backstop: n rounds reach the fixpoint of any graph without one
    }
    return PJ_OK;
}

}  // namespace

// Potentials of the device COO (w: int32 bit patterns) into h (n entries), then
// w := w + h[src] - h[dst] >= 0 in place. st is always filled. Returns PJ_OK,
// PJ_ERR_NEGCYCLE (st.cycle_vertex names a vertex on the cycle) or PJ_ERR_RANGE (a
// potential below -2^30); w is rewritten only on PJ_OK.
int signed_potentials(Ctx& ctx, const u32* src, const u32* dst, u32* w, i64 nnz, i64 n, DevBuf<int32_t>& h,
                      pj_potential_stats& st) {
    hipStream_t s = ctx.stream;
    st = pj_potential_stats{};
    st.cycle_vertex = -1;
    h.alloc((size_t)std::max<i64>(n, 1));
    PJ_HIP(hipMemsetAsync(h.p, 0, h.bytes(), s));
    if (n == 0 || nnz == 0) {
        PJ_HIP(hipStreamSynchronize(s));
        return PJ_OK;
    }
    const unsigned cap = (unsigned)ctx.cu_count * 8u;
    const i64 nwords = (n + 63) / 64;
    DevBuf<u64> fb((size_t)(3 * nwords));
    DevBuf<PotCnt> cnt(1);
    PotCnt hc{};
    hc.cyc = PT_NONE;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    PJ_HIP(hipEventCreate(&e0));
    PJ_HIP(hipEventCreate(&e1));
    struct EvGuard {
        hipEvent_t a, b;
        ~EvGuard() {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
        }
    } guard{e0, e1};
    PJ_HIP(hipMemcpyAsync(cnt.p, &hc, sizeof(PotCnt), hipMemcpyHostToDevice, s));
    PJ_HIP(hipMemsetAsync(fb.p, 0, fb.bytes(), s));
    pot_init_k<<<grid_for(nnz, 256, cap), 256, 0, s>>>(src, w, nnz, fb.p, cnt.p);
    PJ_LAUNCH_CHECK();
    PJ_HIP(hipMemcpyAsync(&hc, cnt.p, sizeof(PotCnt), hipMemcpyDeviceToHost, s));
    PJ_HIP(hipStreamSynchronize(s));
    st.negative_edges = (int64_t)hc.negative;
    int rc = PJ_OK;
    if (hc.negative) {
        DevBuf<u64> key((size_t)n);
        pot_fill_k<<<grid_for(n, 256, cap), 256, 0, s>>>(key.p, n);
        PJ_LAUNCH_CHECK();
        const u32 one = 1;
        PJ_HIP(hipMemcpyAsync(&cnt.p->flags[0], &one, sizeof(u32), hipMemcpyHostToDevice, s));
        i64 checks = 0;
        rc = (u64)nnz > 0xFFFFFFFFull
                 ? pot_rounds<u64>(ctx, src, dst, w, nnz, n, key.p, fb.p, nwords, cnt.p, hc, checks, e0)
                 : pot_rounds<u32>(ctx, src, dst, w, nnz, n, key.p, fb.p, nwords, cnt.p, hc, checks, e0);
        st.cycle_checks = (int64_t)checks;
        st.rounds = (int64_t)hc.rounds;
        st.relaxed_edges = (int64_t)hc.relaxed;
        if (rc == PJ_ERR_NEGCYCLE && hc.cyc != PT_NONE) st.cycle_vertex = (int64_t)hc.cyc;
        if (rc == PJ_OK) {
            pot_out_k<<<grid_for(n, 256, cap), 256, 0, s>>>(key.p, n, h.p, cnt.p);
            PJ_LAUNCH_CHECK();
            pot_reweight_k<<<grid_for(nnz, 256, cap), 256, 0, s>>>(src, dst, w, h.p, nnz, cnt.p);
            PJ_LAUNCH_CHECK();
            PJ_HIP(hipMemcpyAsync(&hc, cnt.p, sizeof(PotCnt), hipMemcpyDeviceToHost, s));
        }
    } else {
        PJ_HIP(hipEventRecord(e0, s));
    }
    PJ_HIP(hipEventRecord(e1, s));
    PJ_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    PJ_HIP(hipEventElapsedTime(&ms, e0, e1));
    st.kernel_ms = (double)ms;
    if (rc == PJ_OK && hc.negative) {
        st.min_potential = hc.hmin;
        if (hc.bad) throw Error(PJ_ERR_HIP, "signed load: a reduced weight is negative (the potentials are no fixpoint)");
    }
    return rc;
}

void signed_correct(const int32_t* dred, const int32_t* h, i64 n, i64 source, int32_t* out, u64* capped,
                    unsigned grid_cap, hipStream_t s) {
    if (n == 0) return;
    signed_correct_k<<<grid_for(n, 256, grid_cap), 256, 0, s>>>(dred, h, n, source, out, capped);
    PJ_LAUNCH_CHECK();
}

}  // namespace pj
