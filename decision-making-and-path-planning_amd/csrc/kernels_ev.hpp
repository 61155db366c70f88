// kernels_ev.hpp — scenario schedule (build-defined): while pp_set_episode_schedule is in force, k_respawn_sched runs in
// the place of k_respawn_spawn - same point of the upload stream, same shape: one 64-lane wave per scene, four scenes per 256-thread
// block, wave-uniform scene index, no LDS, no barrier - and draws the first choice k0 of §4l 3a. by weights computed from outcome
// counts per start record.  Every other step is the device function k_respawn_spawn calls, one copy of each: contact, the clearance
// walk and the restart in kernels_es.hpp (spawn_episode_end, spawn_restart), the steps of §4k under them in kernels_ep.hpp.
//
// Integers only.  Lane k < M computes the weight of record k from its two counts (one 64-bit division per lane, side by side); the sum
// and the running sum are at most 16 scalar iterations each over v_readlane.  Every draw of a launch reads the rows as the launch
// found them: in scope 0 a scene reads and - lane 0, behind the draw - folds its OWN row only; in scope 1 no thread of
// k_respawn_sched writes the handle's row: an ending scene leaves one word, and k_fold_schedule - ONE workgroup, directly behind, in
// front of k_log_episodes - sums the words into 32 LDS counters and applies them.  Integer sums do not depend on their order, so the
// pooled row is reproducible.  No global atomics.
#pragma once
#include "kernels_es.hpp"

namespace dmpp {

static_assert(sizeof(EpisodeSchedule) == 40 && sizeof(EpisodeScheduleRow) == 128 && offsetof(EpisodeScheduleRow, n_fail) == 64, "schedule records (DESIGN.md §4p)");
static_assert(DMPP_EPISODE_MAX_STARTS == 16, "a row is 16 + 16 counts; k_prev fits the low byte of the fold word");

// §4p 1.: the weight of a record with n counted episodes, f of them failures (0 <= f <= n); 1 <= w <= 131070
__host__ __device__ inline int32_t schedule_weight(const EpisodeSchedule& m, int32_t n, int32_t f)
{
    const unsigned long long r = n >= m.min_samples ? ((unsigned long long)f << 16) / (unsigned long long)n : (unsigned long long)m.prior;
    const unsigned long long t = (unsigned long long)m.target, d = r > t ? r - t : t - r;
    return m.floor_w + (int32_t)(((unsigned long long)m.gain * (65536ull - d)) >> 16);
}
// §4p 4.: is an episode that ended with cause word c a failure
__host__ __device__ inline int schedule_fails(const EpisodeSchedule& m, int c) { return (c & m.fail_mask) != 0 && (c & m.pass_mask) == 0 ? 1 : 0; }
// §4p 4.: counts of one record behind `add` endings, `fail` of them failures
__host__ __device__ inline void schedule_fold(int window, int add, int fail, int32_t& n_end, int32_t& n_fail)
{
    int ne = n_end + add, nf = n_fail + fail;
    while (window > 0 && ne >= window) { ne >>= 1; nf >>= 1; }
    n_end = ne; n_fail = nf;
}

// The arguments of k_respawn_spawn, and: the schedule, its rows (scope 0: one per scene; scope 1: one) and - scope 1 only - one word
// per scene for k_fold_schedule.
__global__ void __launch_bounds__(kBlock)
k_respawn_sched(EpisodeModel em, EpisodeSpawn sp, EpisodeSchedule sm, double hw, int n_scenes, int stride, const SceneIn* __restrict__ prev, const ObPoint* __restrict__ obs,
                int n_obs, SceneIn* __restrict__ staged, SceneState* __restrict__ state, const SceneIn* __restrict__ pool_in, const SceneState* __restrict__ pool_state,
                const int32_t* __restrict__ world_first, const int32_t* __restrict__ world_of, int32_t* __restrict__ flags,
                EpisodeStats* __restrict__ stats, EpisodeSpawnStats* __restrict__ sstats, EgoTrace* __restrict__ trace, RolloutScore* __restrict__ score,
                EpisodeScheduleRow* __restrict__ rows, int32_t* __restrict__ fold_word)
{
    const int lane = threadIdx.x & 63;
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kEpScenes + (threadIdx.x >> 6)));
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    SpawnEnd E;
    spawn_episode_end(em, sp, hw, s, lane, prev, obs, n_obs, staged, flags, stats, E);
    if (E.c == 0) { episode_go_on(s, lane, E, stats); return; }
    // §4p 1. weights: lane k holds w_k
    const int M = sp.n_starts;
    const int e = stats[s].n_episodes + 1;
    EpisodeScheduleRow* row = rows + (sm.scope == 0 ? s : 0);
    int w = 0;
    if (lane < M) w = schedule_weight(sm, row->n_end[lane], row->n_fail[lane]);
    // §4p 2. draw: the lowest k whose running sum is greater than t
    unsigned W = 0;
    for (int k = 0; k < M; k++) W += (unsigned)__builtin_amdgcn_readlane(w, k);
    const unsigned t = (unsigned)(((spawn_hash(sp, s, e) >> 32) * (unsigned long long)W) >> 32);
    int k0 = M - 1;
    unsigned run = 0;
    for (int k = 0; k < M; k++) {
        run += (unsigned)__builtin_amdgcn_readlane(w, k);
        if (run > t) { k0 = k; break; }
    }
    const int k_prev = sstats[s].cur_start & (DMPP_EPISODE_MAX_STARTS - 1);      // the record the ENDED episode ran on (written by this kernel: 0 .. M - 1)
    spawn_restart(sp, hw, s, lane, stride, k0, E, prev, staged, state, pool_in, pool_state, world_first, world_of, flags, stats, sstats, trace, score);
    if (lane != 0) return;
    // §4p 4. fold: the scene's own row here, the handle's row in k_fold_schedule
    const int fail = schedule_fails(sm, E.c);
    if (sm.scope == 0) schedule_fold(sm.window, 1, fail, row->n_end[k_prev], row->n_fail[k_prev]);
    else fold_word[s] = k_prev | fail << 8;
}

constexpr int kFoldBlock = 1024;      // one workgroup; a chunk of scenes per pass

// Scope 1: the endings of one advance into the handle's row.  stats: EpisodeStats behind the episode step (age == 0: the scene ended
// an episode in this advance and k_respawn_sched left its word).  128 B of LDS, one barrier pair, no scratch.
__global__ void __launch_bounds__(kFoldBlock)
k_fold_schedule(int n_scenes, int window, const EpisodeStats* __restrict__ stats, const int32_t* __restrict__ fold_word, EpisodeScheduleRow* __restrict__ row)
{
    __shared__ int cnt[2 * DMPP_EPISODE_MAX_STARTS];      // endings per record, then failures per record
    const int tid = threadIdx.x;
    if (tid < 2 * DMPP_EPISODE_MAX_STARTS) cnt[tid] = 0;
    __syncthreads();
    for (int base = 0; base < n_scenes; base += kFoldBlock) {
        const int s = base + tid;
        if (s < n_scenes && stats[s].age == 0) {
            const int word = fold_word[s], k = word & (DMPP_EPISODE_MAX_STARTS - 1);
            atomicAdd(&cnt[k], 1);                                        // (LDS integer adds: any order, one sum)
            if ((word >> 8) & 1) atomicAdd(&cnt[DMPP_EPISODE_MAX_STARTS + k], 1);
        }
    }
    __syncthreads();
    if (tid < DMPP_EPISODE_MAX_STARTS && cnt[tid] > 0) schedule_fold(window, cnt[tid], cnt[DMPP_EPISODE_MAX_STARTS + tid], row->n_end[tid], row->n_fail[tid]);
}

}  // namespace dmpp
