// search_budget.hpp — the LDS budget policy of the search: the data words per view a tick group's k_search gets in LDS, and how many of
// its workgroups the chip then holds at once.  Host only, pure arithmetic: no HIP, no handle, no device (exported as pp_search_budget).
#pragma once
#include <algorithm>
#include <cstddef>

namespace dmpp {

// LDS of one CU as the search sees it: 160 KB, handed out in 128 granules of 1,280 bytes (measured: 54,000 bytes per workgroup are
// two per CU, 52,976 three, 26,864 six); 4 waves per workgroup while it sets up: <= 8 workgroups per CU.
constexpr size_t kLdsPerCu = 160u * 1024u;
constexpr size_t kLdsGranule = 1280;
constexpr size_t kSearchWgsPerCu = 8;

// Workgroups per CU that the hardware grants at per_wg bytes of LDS each: the size rounded up to the granule.
inline int search_wgs_per_cu(size_t per_wg) { return (int)std::min(kSearchWgsPerCu, kLdsPerCu / ((per_wg + kLdsGranule - 1) / kLdsGranule * kLdsGranule)); }
// ... and what search_slots is counted with: the size NOT rounded to the granule, so it OVER-COUNTS (54,000 bytes: three per CU
// here, two in fact).  search_slots feeds the group size and the launch-order decision: making it agree with the count above
// changes scheduling - a performance change, to be measured on its own.
inline int search_wgs_per_cu_unrounded(size_t per_wg) { return (int)std::max<size_t>(1, std::min(kSearchWgsPerCu, kLdsPerCu / per_wg)); }

struct SearchBudget { int budget; bool from_need; int slots; };      // data words per view; budget follows a measured need; workgroup slots

// The budget of a group of G ticks of n scenes, from the one in force (`budget`, 0: none yet; `from_need`: it came from a need).
// static_lds, meta_bytes, gbm_lds: the search kernel's static LDS, its per-line metas, the LDS of its dense form; need: what the
// densest scene of an earlier group needed, -1: nothing has landed yet; fixed: the budget is pinned (DMPP_LDS_BUDGET) and stays;
// dense: every scene takes the dense form in HBM (DMPP_SEARCH_GBM).  First tick: from the obstacle density; afterwards from the need (+ 1/8).
inline SearchBudget search_budget(size_t static_lds, int meta_bytes, int gbm_lds, int budget_max, int n_cus,
                                  int n, int G, int n_obs_total, int need, int budget, bool from_need, bool fixed, bool dense)
{
    const int cus = std::max(1, n_cus);
    if (dense) return { budget, from_need, search_wgs_per_cu_unrounded(static_lds + 64 + (size_t)gbm_lds) * cus };
    if (!fixed) {
        const int items = G * n;
        int want = budget;
        if (need >= 0) {
            const int fit = std::min(budget_max, (need + need / 8 + 64 + 63) / 64 * 64);
            // When the work items outnumber the workgroup slots and a smaller - still safe - slack over the need lets one more
            // searching workgroup onto every CU, the largest budget that does is taken: 256 moving obstacles need ~4,650 words,
            // 5,312 with the usual eighth on top = two workgroups of 55 KB per CU; three fit at <= 5,120 (configs[3]: 1.14 -> 1.23 M
            // ticks/s); 4096 scenes of 64 obstacles: six of 26.9 KB instead of five of 27.9 (5.17 -> 5.30 M).  With a slot for every
            // item the eighth stays: the room it leaves on the CU is what the front kernels start in.  A scene that outgrows the
            // budget takes the dense form in HBM.
            const size_t fixed_lds = static_lds + 64 + (size_t)meta_bytes;
            auto wgs_at = [&](int b) { return search_wgs_per_cu(fixed_lds + 8 * (size_t)b); };
            int target = fit;
            const int tight = std::min(budget_max, (need + std::max(need / 32, 96) + 63) / 64 * 64);
            if (tight < fit && wgs_at(tight) > wgs_at(fit) && items > wgs_at(fit) * cus) {
                const size_t room = kLdsPerCu / (size_t)wgs_at(tight) / kLdsGranule * kLdsGranule;
                const int lim = room > fixed_lds ? (int)((room - fixed_lds) / 8 / 64 * 64) : 0;
                target = std::max(tight, std::min(lim, fit));
            }
            // (the first need that arrives replaces the first tick's guess outright: 64 obstacles were guessed at 2,048 words, need
            // 1,635, and the hysteresis kept the guess - 28.2 KB per workgroup, 18.8 KB free beside five of them, 0.5 KB short of
            // a k_decision workgroup; at 1,920 it fits: +1 % at 1024 scenes, +3 % at 4096)
            if (!from_need || target > budget || target < budget - budget / 4 || (budget > 0 && wgs_at(target) > wgs_at(budget))) want = target;
            from_need = true;
        }
        if (want <= 0) {
            const long long per_scene = ((long long)n_obs_total + n - 1) / n;
            want = (int)std::min<long long>(budget_max, (28 * per_scene + 256 + 63) / 64 * 64);
        }
        budget = std::max(64, std::min(want, budget_max));
    }
    const size_t per_wg = static_lds + 64 + std::max((size_t)meta_bytes + 8 * (size_t)budget, (size_t)gbm_lds);
    return { budget, from_need, search_wgs_per_cu_unrounded(per_wg) * cus };
}

// LDS granules a workgroup of `bytes` holds, and those that stay free on a CU beside `wgs` workgroups of per_wg bytes
constexpr int lds_granules(size_t bytes) { return (int)((bytes + kLdsGranule - 1) / kLdsGranule); }
constexpr int lds_granules_free(int wgs, size_t per_wg) { return (int)(kLdsPerCu / kLdsGranule) - wgs * lds_granules(per_wg); }

// The co-residency step behind the policy: the budget a group's search is LAUNCHED with, given the one search_budget() chose.
// While the work items outnumber the slots every CU holds `wgs` searching workgroups all the time, and a front or scoring
// workgroup starts only in what they leave free.  When that is less than a workgroup of `beside_lds` bytes needs (the larger of
// k_planning's and k_score<4>'s) and a smaller budget - not below the tight one, need + max(need / 32, 96), and with the same
// `wgs` - leaves enough, the largest such multiple of 64 words is taken: 64 obstacles at 512 x 512 need 1,498 words, the policy
// keeps 1,792 = 21 granules, six per CU, 2 free; at 1,600 a workgroup is 19 granules and 14 stay free beside six of them.
// Nothing changes with a slot for every item, a fixed or dense budget, no need yet, or when no such budget exists.  The caller
// keeps the policy's budget for its next call of search_budget(): the hysteresis there must not see this step's output.
inline int coresident_budget(size_t static_lds, int meta_bytes, int gbm_lds, int budget_max, int n_cus, int items, int need, int budget,
                             bool fixed, bool dense, size_t beside_lds)
{
    if (fixed || dense || need < 0 || budget <= 0) return budget;
    auto per_wg = [&](int b) { return static_lds + 64 + std::max((size_t)meta_bytes + 8 * (size_t)b, (size_t)gbm_lds); };
    const int wgs = search_wgs_per_cu(per_wg(budget)), want = lds_granules(beside_lds);
    if (items <= wgs * std::max(1, n_cus) || lds_granules_free(wgs, per_wg(budget)) >= want) return budget;
    const int tight = std::min(budget_max, (need + std::max(need / 32, 96) + 63) / 64 * 64);
    for (int b = budget / 64 * 64; b >= tight && b > 0; b -= 64) {
        if (b == budget) continue;
        if (search_wgs_per_cu(per_wg(b)) != wgs) break;              // (a smaller budget never holds fewer workgroups)
        if (lds_granules_free(wgs, per_wg(b)) >= want) return b;
    }
    return budget;
}

}  // namespace dmpp
