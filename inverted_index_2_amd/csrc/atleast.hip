// atleast.hip — the counting form of the threshold query (ii2_atleast_ranges): "docs in at least m of n groups" for any number
// of groups and lists.  Per window of the doc range the host (setop.cpp: atleast_count) marks one group after the other into the
// per-context doc bitmap G with the block-wise union's mark kernel (union_many.hip: k_um_mark - the union is what counts an id
// once per group), and the two kernels here keep one small counter per doc in B = bit_width(m) bit planes laid out as G is:
//   k_thr_add     behind every group's mark: one wave per summary word (2048 bitmap words), as k_um_count walks them.  Per set
//                 2048-doc chunk each lane adds its word of G into its words of the planes (ripple carry, saturating:
//                 atleast_count.h), stores them and zeroes the G word; then the chunk bits go into the accumulated summary S_acc
//                 and the G summary word is zeroed.  In late mode - the groups behind the first n' - m + 1, in ascending order
//                 of postings: a doc first seen there cannot reach m - chunks that S_acc does not name are cleared, not added.
//   k_thr_select  behind the last group (and the mark of the excluded lists, which leaves them in G): over the chunks of
//                 S_acc | S_G it compares the counters with m, most significant plane first, zeroes the planes, writes
//                 G = ge & ~G, clears S_acc and names every chunk it visited in the G summary - k_um_count, the scan and
//                 k_um_compact then produce the ids as they do for a union and zero what the summary names.
// A summary word and its 2048 x 32 docs belong to one wave: no atomics, and no kernel waits for another workgroup.  Every
// access is 64 lanes x one dword, consecutive.
#include <hip/hip_runtime.h>

#include "atleast_count.h"
#include "internal.h"

namespace ii2 {

template <uint32_t B> __global__ __launch_bounds__(256) void k_thr_add(ThrParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
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
            uint32_t pl[B];
#pragma unroll
            for (uint32_t b = 0; b < B; b++) pl[b] = p.planes[(size_t)b * p.plane_words + wi];
            thr_add_word<B>(pl, g);
#pragma unroll
            for (uint32_t b = 0; b < B; b++) p.planes[(size_t)b * p.plane_words + wi] = pl[b];
        }
        if (l == 0) {
            if (!p.late) p.acc[sw] = acc | set;
            p.summary[sw] = 0u;
        }
    }
}

template <uint32_t B> __global__ __launch_bounds__(256) void k_thr_select(ThrParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves) {
        const uint32_t acc = p.acc[sw];
        const uint32_t set = acc | p.summary[sw];
        if (!set) continue;                                               // (wave-uniform)
        uint32_t bits = set;
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            uint32_t ge = 0u;
            if ((acc >> chunk) & 1u) {                                    // (else the chunk holds excluded ids only: its planes are zero)
                uint32_t pl[B];
#pragma unroll
                for (uint32_t b = 0; b < B; b++) pl[b] = p.planes[(size_t)b * p.plane_words + wi];
                ge = thr_ge_word<B>(pl, p.min_match);
#pragma unroll
                for (uint32_t b = 0; b < B; b++)
                    if (pl[b]) p.planes[(size_t)b * p.plane_words + wi] = 0u;
            }
            const uint32_t g = p.bitmap[wi];
            const uint32_t keep = ge & ~g;
            if (keep != g) p.bitmap[wi] = keep;
        }
        if (l == 0) {
            if (acc) p.acc[sw] = 0u;
            p.summary[sw] = set;
        }
    }
}

template <uint32_t B> static void thr_launch(bool select, const ThrParams &p, uint32_t grid, hipStream_t s) {
    if (select) hipLaunchKernelGGL(k_thr_select<B>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_thr_add<B>, dim3(grid), dim3(256), 0, s, p);
}

static hipError_t thr_dispatch(bool select, const ThrParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (p.n_planes < 1u || p.n_planes > THR_MAX_PLANES || !grid) return hipErrorInvalidValue;
    if (ev0) (void)hipEventRecord(ev0, s);
    switch (p.n_planes) {
        case 1: thr_launch<1>(select, p, grid, s); break;
        case 2: thr_launch<2>(select, p, grid, s); break;
        case 3: thr_launch<3>(select, p, grid, s); break;
        case 4: thr_launch<4>(select, p, grid, s); break;
        case 5: thr_launch<5>(select, p, grid, s); break;
        case 6: thr_launch<6>(select, p, grid, s); break;
        case 7: thr_launch<7>(select, p, grid, s); break;
        default: thr_launch<8>(select, p, grid, s); break;
    }
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

hipError_t launch_thr_add(const ThrParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    return thr_dispatch(false, p, grid, s, ev0, ev1);
}

hipError_t launch_thr_select(const ThrParams &p, uint32_t grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    return thr_dispatch(true, p, grid, s, ev0, ev1);
}

}  // namespace ii2
