// topk_batch_run.h — the rule of the batched ranked query (ii2_topk_batch: k_topk_batch in topk_batch.hip) over one run of equal ids,
// ss_group_run's sibling (small_set_device.h).  The device kernel and the host-only export ii2_topk_batch_run call the same code.
#pragma once
#include <stdint.h>

#include "atleast_count.h"

namespace ii2 {

constexpr uint32_t TB_RUN_END = 0xFFFFFFFFu;

// One run of equal ids among the ascending ids of a query: tag_at(k) is the group tag of its k-th entry, TB_RUN_END behind its last
// one (a run is at most MAX_LISTS long: a list holds an id once).  The required groups are tags 0 .. n_req - 1, the excluded lists
// tag n_req; lists are in tag order, so the tags inside a run ascend.  The doc's score is the sum of weight_of(t) over the distinct
// required tags t of the run - a repeated tag (two lists of one group that hold the id) counts once - and the doc is excluded when
// the run's last tag is not a required one.
template <class TagAt, class WeightOf> II2_HD uint32_t tb_run_score(TagAt tag_at, WeightOf weight_of, uint32_t n_req, bool *excluded) {
    uint32_t score = 0, last = TB_RUN_END;
    for (uint32_t k = 0;; k++) {
        const uint32_t t = tag_at(k);
        if (t == TB_RUN_END) break;
        if (t != last && t < n_req) score += weight_of(t);
        last = t;
    }
    *excluded = last != TB_RUN_END && last >= n_req;
    return score;
}

// what a query's doc needs to be eligible, the tombstone test aside
II2_HD bool tb_run_eligible(uint32_t score, bool excluded, uint32_t min_score) { return score >= min_score && !excluded; }

}  // namespace ii2
