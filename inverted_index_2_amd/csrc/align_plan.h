// align_plan.h — the shape of the alignment's ranking kernel (align.hip: k_align_rank), for the device and for the host
// alike: how many terms a workgroup takes, how many entries of another dictionary it stages in LDS, and where a workgroup's
// stretch of terms begins and ends in another dictionary.  The kernel and the host-only ii2_align_plan use these constants
// and this function and no others.
#pragma once
#include "term_device.h"

namespace ii2 {

constexpr uint32_t AL_THREADS = 256;      // threads per workgroup of the ranking kernel
constexpr uint32_t AL_T = 1024;           // terms per workgroup (the brackets in the other dictionaries are searched once per workgroup)
constexpr uint32_t AL_LCAP = 2048;        // bracket entries staged per dictionary (larger brackets: bisection in global memory)

// workgroups of a dictionary of n terms
__host__ __device__ __forceinline__ uint64_t align_workgroups(uint64_t n) { return (n + AL_T - 1) / AL_T; }

// One end of the bracket that a workgroup's stretch of terms has in dictionary d of n terms.  end = false, x the stretch's
// first term: the terms of d before x.  end = true, x its last term: the terms of d up to and including x.
__host__ __device__ __forceinline__ uint32_t align_bracket(const TermDict &d, uint32_t n, const TermRef &x, bool end, bool long_terms) {
    return term_bound(d, 0u, n, x, end, long_terms);
}

}  // namespace ii2
