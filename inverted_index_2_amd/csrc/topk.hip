// topk.hip — the ranked query (ii2_topk_ranges): "the k docs that lie in the most of these groups, and in how many".  The host
// (setop.cpp: topk_count) runs the counting form of ii2_atleast_ranges up to its last step - per window of the doc range every
// required group marked into the per-context doc bitmap G (union_many.hip: k_um_mark) and added into B = bit_width(n') bit planes
// (atleast.hip: k_thr_add, never saturating at that width), then the excluded lists marked into G - and, instead of collapsing the
// counters to one bit, keeps them:
//   pass 1  k_top_hist   one wave per summary word (2048 bitmap words), as k_thr_select walks them: per word the eligible docs -
//                        counter >= min_match, not in G, not in the tombstone word - are tallied by score into a 256-entry
//                        histogram in LDS, one per workgroup, flushed with one 64-bit global add per non-zero entry.
//           k_top_base   one workgroup: base[s] = the eligible docs of a higher score than s - where class s starts in the result.
//           The host reads the histogram back and cuts it for k (topk_count.h: top_cut).
//   pass 2  k_top_count  per summary word and score class cut_score .. max_score, the eligible docs of that class: a class-major
//                        (class x summary word) table, scanned once (scan.hip);
//           k_top_emit   the docs of class s go to base[s] + (those of the class in earlier windows) + (the table's prefix)
//                        + (their rank inside the word's wave), in doc order - the result is in rank order without a sort, and
//                        the cut class stops at its quota n_cut, which its smallest ids fill.  It zeroes everything it read.
// A word's docs are tallied class by class: the class of the lowest doc left is read from the planes (top_score), an equality
// mask names every doc of that class in the wave's 64 words (top_eq_word), they are counted / placed by one wave scan, and the
// loop goes on with what is left - as many rounds as the 2048 docs hold distinct scores, whatever n' is.
// The weighted form (ii2_topk_weighted_ranges) puts its own add behind every mark, k_top_add: the walk of the counting form's add
// kernel (atleast.hip), but the group's weight w is added to its docs' counters (topk_count.h: top_add_weighted), and only the
// planes ctz(w) .. B - 1 are loaded and stored - an even weight moves fewer bytes (the kernel is instantiated on their number).  Late mode is the counting form's: a chunk
// that S_acc does not name is cleared, not added (topk_count.h: top_late_set says for which groups that loses no eligible doc).
// A summary word and its 2048 x 32 docs belong to one wave; no kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "dv1_device.h"
#include "internal.h"
#include "topk_count.h"

namespace ii2 {

// orders the wave's own LDS traffic (one wave reads what its lane 0 wrote) and keeps the compiler from caching across it
__device__ __forceinline__ void top_wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ uint32_t top_tomb(const TopParams &p, uint32_t word) {
    return (p.tomb && word < p.tomb_nwords) ? p.tomb[word] : 0u;
}

// f(s, m) once per distinct score s among the docs e of the wave's 64 words: m = this lane's docs of that score (wave-uniform
// control flow: every lane calls f)
template <uint32_t B, class F> __device__ __forceinline__ void top_classes(const uint32_t (&pl)[B], uint32_t e, F f) {
    uint32_t rem = e;
    for (;;) {
        const uint64_t live = __ballot(rem != 0u);
        if (!live) break;
        const int leader = (int)__builtin_ctzll(live);
        const uint32_t mine = rem ? top_score<B>(pl, (uint32_t)__builtin_ctz(rem)) : 0u;
        const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)mine, leader, 64));
        const uint32_t m = top_eq_word<B>(pl, s) & rem;
        rem &= ~m;
        f(s, m);
    }
}

// the eligible docs of bitmap word wi with a score >= lo, and their planes in pl; clear: the planes and the G word are zeroed
template <uint32_t B>
__device__ __forceinline__ uint32_t top_load_word(const TopParams &p, uint32_t wi, bool counted, bool marked, uint32_t lo, bool clear, uint32_t (&pl)[B]) {
    uint32_t ge = 0u;
#pragma unroll
    for (uint32_t b = 0; b < B; b++) pl[b] = 0u;
    if (counted) {                                                        // (else the chunk holds excluded ids only: its planes are zero)
#pragma unroll
        for (uint32_t b = 0; b < B; b++) pl[b] = p.planes[(size_t)b * p.plane_words + wi];
        ge = thr_ge_word<B>(pl, lo);
        if (clear) {
#pragma unroll
            for (uint32_t b = 0; b < B; b++)
                if (pl[b]) p.planes[(size_t)b * p.plane_words + wi] = 0u;
        }
    }
    uint32_t g = 0u;
    if (marked) {
        g = p.bitmap[wi];
        if (clear && g) p.bitmap[wi] = 0u;
    }
    if (!ge) return 0u;
    return ge & ~g & ~top_tomb(p, p.win_lo / 32u + wi);
}

template <uint32_t B> __global__ __launch_bounds__(256) void k_top_hist(TopParams p) {
    __shared__ uint32_t sh[TOPK_SCORES];
    sh[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    const bool clear = p.clear != 0u;
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves) {
        const uint32_t acc = p.acc[sw], marked = p.summary[sw];
        uint32_t bits = clear ? acc | marked : acc;
        if (!bits) continue;                                              // (wave-uniform)
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            uint32_t pl[B];
            const uint32_t e = top_load_word<B>(p, wi, (acc >> chunk) & 1u, (marked >> chunk) & 1u, p.min_match, clear, pl);
            top_classes<B>(pl, e, [&](uint32_t s, uint32_t m) {
                const uint32_t total = wave_sum((uint32_t)__popc(m));
                if (l == 0) atomicAdd(&sh[s & (TOPK_SCORES - 1u)], total);
            });
        }
        if (clear && l == 0) {
            if (acc) p.acc[sw] = 0u;
            if (marked) p.summary[sw] = 0u;
        }
    }
    __syncthreads();
    const uint32_t c = sh[threadIdx.x];
    if (c) atomicAdd((unsigned long long *)&p.hist[threadIdx.x], (unsigned long long)c);
}

// base[s] = the docs of a score above s
__global__ __launch_bounds__(256) void k_top_base(TopParams p) {
    __shared__ uint64_t h[TOPK_SCORES];
    h[threadIdx.x] = p.hist[threadIdx.x];
    __syncthreads();
    uint64_t above = 0;
    for (uint32_t t = threadIdx.x + 1u; t < TOPK_SCORES; t++) above += h[t];
    p.base[threadIdx.x] = above;
}

template <uint32_t B> __global__ __launch_bounds__(256) void k_top_count(TopParams p) {
    __shared__ uint32_t wc[4][TOPK_SCORES];
    const uint32_t l = threadIdx.x & 63u;
    uint32_t *w = wc[threadIdx.x >> 6];
    for (uint32_t i = l; i < TOPK_SCORES; i += 64u) w[i] = 0u;
    top_wave_lds_sync();
    if (blockIdx.x == 0 && threadIdx.x == 0) p.cnt[(size_t)p.n_cls * p.n_sum] = 0u;      // the scan's closing entry
    const uint32_t n_waves = gridDim.x * 4u;
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves) {
        const uint32_t acc = p.acc[sw], marked = p.summary[sw];
        uint32_t bits = acc;
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            uint32_t pl[B];
            const uint32_t e = top_load_word<B>(p, wi, true, (marked >> chunk) & 1u, p.cut_score, false, pl);
            top_classes<B>(pl, e, [&](uint32_t s, uint32_t m) {
                const uint32_t total = wave_sum((uint32_t)__popc(m));
                const uint32_t ci = s - p.cut_score;
                if (l == 0 && ci < p.n_cls) w[ci] += total;
            });
        }
        top_wave_lds_sync();
        for (uint32_t ci = l; ci < p.n_cls; ci += 64u) {
            p.cnt[(size_t)ci * p.n_sum + sw] = w[ci];
            w[ci] = 0u;
        }
        top_wave_lds_sync();
    }
}

template <uint32_t B> __global__ __launch_bounds__(256) void k_top_emit(TopParams p) {
    __shared__ uint32_t wr[4][TOPK_SCORES];           // per wave and class: the docs of the class before the wave's next one, in this window
    __shared__ uint64_t s_base[TOPK_SCORES], s_prev[TOPK_SCORES];   // per class: where it starts in the result; its docs in earlier windows
    const uint32_t l = threadIdx.x & 63u;
    uint32_t *r = wr[threadIdx.x >> 6];
    if (threadIdx.x < p.n_cls) {
        const uint32_t ci = threadIdx.x;
        const uint64_t prev = p.window ? p.run[(p.window & 1u) * TOPK_SCORES + ci] : 0ull;
        s_base[ci] = p.base[p.cut_score + ci];
        s_prev[ci] = prev;
        if (blockIdx.x == 0)
            p.run[((p.window + 1u) & 1u) * TOPK_SCORES + ci] = prev + (p.off[(size_t)(ci + 1u) * p.n_sum] - p.off[(size_t)ci * p.n_sum]);
    }
    __syncthreads();
    const uint32_t n_waves = gridDim.x * 4u;
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves) {
        const uint32_t acc = p.acc[sw], marked = p.summary[sw];
        uint32_t bits = acc | marked;
        if (!bits) continue;                                              // (wave-uniform)
        for (uint32_t ci = l; ci < p.n_cls; ci += 64u) r[ci] = (uint32_t)(p.off[(size_t)ci * p.n_sum + sw] - p.off[(size_t)ci * p.n_sum]);
        top_wave_lds_sync();
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            uint32_t pl[B];
            uint32_t e = top_load_word<B>(p, wi, (acc >> chunk) & 1u, (marked >> chunk) & 1u, p.cut_score, true, pl);
            if (!p.n_cls) e = 0u;                                         // nothing is returned: the call only cleans up
            const uint32_t doc0 = p.win_lo + wi * 32u;
            top_classes<B>(pl, e, [&](uint32_t s, uint32_t m) {
                const uint32_t ci = s - p.cut_score;
                const uint32_t c = (uint32_t)__popc(m);
                const uint32_t incl = wave_incl_scan(c);
                const uint32_t total = wave_bcast(incl, 63);
                if (ci >= p.n_cls) return;                                // (wave-uniform; cannot happen: the histogram saw the same docs)
                const uint32_t r0 = r[ci];
                uint64_t rank = s_prev[ci] + r0 + (incl - c);             // among the docs of this class, in doc order
                const uint64_t quota = ci ? ~0ull : p.n_cut;
                const uint64_t at0 = s_base[ci];
                uint32_t v = m;
                while (v) {
                    const uint32_t bit = (uint32_t)__builtin_ctz(v);
                    v &= v - 1u;
                    const uint64_t at = at0 + rank;
                    if (rank < quota && at < p.k) {
                        p.ids[at] = doc0 + bit;
                        if (p.scores) p.scores[at] = s;
                    }
                    rank++;
                }
                top_wave_lds_sync();
                if (l == 0) r[ci] = r0 + total;
                top_wave_lds_sync();
            });
        }
        if (l == 0) {
            if (acc) p.acc[sw] = 0u;
            if (marked) p.summary[sw] = 0u;
        }
    }
}

// behind a group's mark: w added to the counters of the docs in G, G and its summary zeroed, the chunks named in S_acc.  One wave
// per summary word; every access is 64 lanes x one dword, consecutive; the weight and late are wave-uniform.  NP = B - ctz(w) planes
// take part: the launch hands the kernel plane ctz(w) as its plane 0 and w >> ctz(w), an odd weight, so the loads and stores of
// the NP planes stand side by side without a branch between them.
template <uint32_t NP> __global__ __launch_bounds__(256) void k_top_add(TopAddParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    const uint32_t w = p.weight | 1u;                                     // (odd already: the add is known to start at plane 0)
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves) {
        const uint32_t set = p.summary[sw];
        if (!set) continue;                                               // (wave-uniform)
        const uint32_t acc = p.acc[sw];
        uint32_t bits = set;
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            const uint32_t g = p.bitmap[wi];
            if (!g) continue;
            p.bitmap[wi] = 0u;
            if (p.late && !((acc >> chunk) & 1u)) continue;               // no doc of this chunk was seen in an early group
            uint32_t pl[NP];
#pragma unroll
            for (uint32_t b = 0; b < NP; b++) pl[b] = p.planes[(size_t)b * p.plane_words + wi];
            top_add_weighted<NP>(pl, g, w);
#pragma unroll
            for (uint32_t b = 0; b < NP; b++) p.planes[(size_t)b * p.plane_words + wi] = pl[b];
        }
        if (l == 0) {
            if (!p.late) p.acc[sw] = acc | set;
            p.summary[sw] = 0u;
        }
    }
}

template <uint32_t NP> static void top_add_launch(const TopAddParams &p, uint32_t grid, hipStream_t s) {
    hipLaunchKernelGGL(k_top_add<NP>, dim3(grid), dim3(256), 0, s, p);
}

hipError_t launch_top_add(const TopAddParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (p.n_planes < 1u || p.n_planes > THR_MAX_PLANES || !grid || !p.weight || (p.weight >> p.n_planes)) return hipErrorInvalidValue;
    // the planes below ctz(weight) are neither read nor written: the kernel sees the others as planes 0 .. NP - 1
    const uint32_t z = (uint32_t)__builtin_ctz(p.weight);
    TopAddParams q = p;
    q.planes = p.planes + (size_t)z * p.plane_words;
    q.n_planes = p.n_planes - z;
    q.weight = p.weight >> z;
    if (ev0) (void)hipEventRecord(ev0, s);
    switch (q.n_planes) {
        case 1: top_add_launch<1>(q, grid, s); break;
        case 2: top_add_launch<2>(q, grid, s); break;
        case 3: top_add_launch<3>(q, grid, s); break;
        case 4: top_add_launch<4>(q, grid, s); break;
        case 5: top_add_launch<5>(q, grid, s); break;
        case 6: top_add_launch<6>(q, grid, s); break;
        case 7: top_add_launch<7>(q, grid, s); break;
        default: top_add_launch<8>(q, grid, s); break;
    }
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

enum TopKernel { TOP_HIST, TOP_COUNT, TOP_EMIT };

template <uint32_t B> static void top_launch(TopKernel k, const TopParams &p, uint32_t grid, hipStream_t s) {
    if (k == TOP_HIST) hipLaunchKernelGGL(k_top_hist<B>, dim3(grid), dim3(256), 0, s, p);
    else if (k == TOP_COUNT) hipLaunchKernelGGL(k_top_count<B>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_top_emit<B>, dim3(grid), dim3(256), 0, s, p);
}

static hipError_t top_dispatch(TopKernel k, const TopParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (p.n_planes < 1u || p.n_planes > THR_MAX_PLANES || !grid || p.n_cls > TOPK_SCORES || p.cut_score + p.n_cls > TOPK_SCORES) return hipErrorInvalidValue;
    if (ev0) (void)hipEventRecord(ev0, s);
    switch (p.n_planes) {
        case 1: top_launch<1>(k, p, grid, s); break;
        case 2: top_launch<2>(k, p, grid, s); break;
        case 3: top_launch<3>(k, p, grid, s); break;
        case 4: top_launch<4>(k, p, grid, s); break;
        case 5: top_launch<5>(k, p, grid, s); break;
        case 6: top_launch<6>(k, p, grid, s); break;
        case 7: top_launch<7>(k, p, grid, s); break;
        default: top_launch<8>(k, p, grid, s); break;
    }
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

hipError_t launch_top_hist(const TopParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    return top_dispatch(TOP_HIST, p, grid, s, ev0, ev1);
}

hipError_t launch_top_base(const TopParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_top_base, dim3(1), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_top_count(const TopParams &p, uint32_t grid, hipStream_t s) { return top_dispatch(TOP_COUNT, p, grid, s, nullptr, nullptr); }

hipError_t launch_top_emit(const TopParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    return top_dispatch(TOP_EMIT, p, grid, s, ev0, ev1);
}

}  // namespace ii2
