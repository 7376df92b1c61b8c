// lookback_check.hip — the look-back protocol of lookback.h, run WITHOUT a payload (tests and diagnostics: ii2_lookback_check).
//
// The kernels that use the protocol (k_and2_fused, k_enc_stream) take whichever of its branches the timing of a launch gives
// them, and a wrong offset there faults nowhere: it shifts output.  Here a workgroup does with the protocol exactly what
// k_enc_stream does - the same functions of lookback.h in the same order, nothing of them restated - with an amount the host
// chose, on the context's own records, and reports what came out: its prefix, whether a wait ran out, and how the walk over the
// group records went.  The host may fill the records of the workgroups and groups before the launched ones (g_base) with any
// state it likes, so every branch of the walk is taken on purpose instead of by chance.
#include "dv1_device.h"
#include "internal.h"
#include "lookback.h"

namespace ii2 {

// Workgroup g = g_base + blockIdx.x of a logical grid of n_wg; wave 0 asks, wave 1 collects the group's amount (as in k_enc_stream)
__global__ __launch_bounds__(LB_CHECK_THREADS) void k_lb_check(LbCheckParams p) {
    __shared__ uint32_t wg_err;
    const int l = lane_id();
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = p.g_base + blockIdx.x;
    const unsigned long long own = p.amount[g];
    if (threadIdx.x == 0) wg_err = 0u;
    lds_barrier();
    if (threadIdx.x == 0) {
        for (uint32_t i = p.delay ? p.delay[g] : 0u; i != 0u; i--) __builtin_amdgcn_s_sleep(16);      // (a late publisher: the others really poll)
        lb_publish(p.lb, g, own);
    }
    if (wv == 1u && lb_is_leader(g, p.n_wg)) {
        if (!lb_group_publish(p.lb, g, own) && l == 0) { atomicOr(&wg_err, LB_CHECK_GAVE_UP_GROUP); lb_fail(p.lb); }
    }
    unsigned long long pre = 0ull;
    uint32_t polls = 0u, pm = 0u, windows = 0u, dist = LB_CHECK_NO_PREFIX;
    if (wv == 0u) {
        const bool ok = lb_prefix(p.lb, g, p.n_wg, own, &pre, &polls, &pm, &windows, &dist);
        if (!ok && l == 0) { atomicOr(&wg_err, LB_CHECK_GAVE_UP_PREFIX); lb_fail(p.lb); }
    }
    lds_barrier();
    if (threadIdx.x == 0) {
        const uint32_t i = blockIdx.x;
        const uint32_t err = wg_err;
        p.prefix[i] = (err & LB_CHECK_GAVE_UP_PREFIX) ? 0ull : pre;
        p.state[i] = err;
        p.walk[i] = (windows & 0xFFFFFFu) | (dist << 24);
        p.polls[i] = polls;
    }
}

hipError_t launch_lb_check(const LbCheckParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_lb_check, dim3(p.n_wg - p.g_base), dim3(LB_CHECK_THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace ii2
