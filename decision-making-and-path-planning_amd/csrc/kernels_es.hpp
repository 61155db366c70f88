// kernels_es.hpp — episode spawn model (build-defined): k_respawn_spawn runs in the place of k_respawn_egos while
// pp_set_episode_spawn is in force - same point of the upload stream, same shape: one 64-lane wave per scene, four scenes per
// 256-thread block, no LDS, no barrier.  On top of §4k it ends an episode on contact with an obstacle of the scene's slice, draws
// the start record of a restart from a pool of M per scene and skips the candidates that are not clear of the slice and of the
// egos of the scene's world.
//
// The scene index is wave-uniform (readfirstlane), so everything up to the cause word is scalar but the contact scan: there the
// lanes stride the slice and one ballot per pass of 64 entries tells the wave whether any of them touches (only the predicate is
// needed: subtraction is monotone, so "some d_j - hw <= 0" needs no minimum).  A scene that goes on costs lane 0 two stores.  The
// candidate loop is wave-uniform too: per candidate the lanes stride the slice, then the member range of the world, one ballot per
// pass, and the loop leaves on the first clear candidate.  The pool holds record k of scene s at k * stride + s with an even
// stride: a record of the pool and the staged record it replaces share their phase within 16 bytes (wave_copy_record).
#pragma once
#include "kernels_ep.hpp"

namespace dmpp {

static_assert(sizeof(EpisodeSpawn) == 32 && sizeof(EpisodeSpawnStats) == 80 && offsetof(EpisodeSpawnStats, n_used) == 16, "spawn records (DESIGN.md §4l)");
static_assert(DMPP_EGO_CONTACT == 128, "cause bit of §4l");

// §4l 3a. mix: uint64 arithmetic mod 2^64
__device__ __forceinline__ unsigned long long spawn_mix(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// some entry j of obs[0 .. n) has (sqrt(dx dx + dy dy) - (double)radius) - hw <= lim (a NaN compares false); wave-uniform result
__device__ __forceinline__ bool wave_slice_within(const ObPoint* __restrict__ obs, int n, double x, double y, double hw, double lim, int lane)
{
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        bool hit = false;
        if (j < n) {
            const double dx = obs[j].x - x, dy = obs[j].y - y;
            hit = (sqrt(dx * dx + dy * dy) - (double)obs[j].radius) - hw <= lim;
        }
        if (wave_ballot(hit)) return true;
    }
    return false;
}

// some scene t != s of [p0, p1) has (sqrt(dx dx + dy dy) - hw) - hw <= lim at the pose the advance read
__device__ __forceinline__ bool wave_world_within(const SceneIn* __restrict__ prev, int p0, int p1, int s, double x, double y, double hw, double lim, int lane)
{
    for (int base = p0; base < p1; base += 64) {
        const int t = base + lane;
        bool hit = false;
        if (t < p1 && t != s) {
            const double dx = prev[t].loc.globalpoint.x - x, dy = prev[t].loc.globalpoint.y - y;
            hit = (sqrt(dx * dx + dy * dy) - hw) - hw <= lim;
        }
        if (wave_ballot(hit)) return true;
    }
    return false;
}

// What steps 1 - 2 of §4l leave for the steps behind them: what §4k's leave (EpisodeEnd; c with CONTACT on top) and the scene's slice
// of the pool the advance read.
struct SpawnEnd : EpisodeEnd { int on; const ObPoint* slice; };

// The steps of §4l as device functions: k_respawn_spawn and k_respawn_sched (kernels_ev.hpp, §4p) are made of the same ones, and differ
// in how k0 is drawn.  Steps 1., 2., 3., 5. and 6. are §4k's and live in kernels_ep.hpp (episode_age_dist, episode_cause / episode_go_on,
// episode_close, episode_start_words); 1a. and 3a. are here.
// §4l 1., 1a., 2.: age and distance of the running episode, contact, cause word
__device__ __forceinline__ void spawn_episode_end(const EpisodeModel& em, const EpisodeSpawn& sp, double hw, int s, int lane, const SceneIn* prev, const ObPoint* obs,
                                                  int n_obs, const SceneIn* staged, const int32_t* flags, const EpisodeStats* stats, SpawnEnd& E)
{
    E.f = flags[s];
    const double px = prev[s].loc.globalpoint.x, py = prev[s].loc.globalpoint.y;
    episode_age_dist(stats[s], px, py, staged[s].loc.globalpoint.x, staged[s].loc.globalpoint.y, E);
    // the slice of the record the advance read (a sanitised record: inside the pool; anything else is taken as empty)
    int off = prev[s].obs_off, on = prev[s].obs_n;
    if (on <= 0 || off < 0 || (long long)off + on > (long long)n_obs) { off = 0; on = 0; }
    E.slice = obs + off; E.on = on;
    // 1a. contact
    const bool touch = sp.contact != 0 && wave_slice_within(E.slice, on, px, py, hw, 0.0, lane);
    E.c = episode_cause(em, E.f, E.age) | (touch ? DMPP_EGO_CONTACT : 0);
}

// §4l 3a.: the hash of scene s for its e-th ended episode
__device__ __forceinline__ unsigned long long spawn_hash(const EpisodeSpawn& sp, int s, int e)
{
    return spawn_mix(spawn_mix(sp.seed + (unsigned long long)s) + (unsigned long long)e);
}

// §4l 3. - 6. behind the walk: the restart onto record k, stats, the words of the walk, trace and scorecard words (lane 0).  Shared with
// k_respawn_world (kernels_ew.hpp, §4s), whose walk is the world's
__device__ __forceinline__ void spawn_take_record(int s, int lane, int stride, int k, int rejected, int blocked, const SpawnEnd& E,
                                                  SceneIn* staged, SceneState* state, const SceneIn* pool_in, const SceneState* pool_state, int32_t* flags,
                                                  EpisodeStats* stats, EpisodeSpawnStats* sstats, EgoTrace* trace, RolloutScore* score)
{
    // 4. restart: SceneIn and SceneState of the scene become start record k, every byte
    const SceneIn* start_in = pool_in + (size_t)k * stride;
    wave_copy_record(&staged[s], &start_in[s], lane);
    wave_copy_record(&state[s], &pool_state[(size_t)k * stride + s], lane);
    if (lane != 0) return;
    episode_close(stats[s], E);
    flags[s] = 0;
    EpisodeSpawnStats& S = sstats[s];
    if (E.c & DMPP_EGO_CONTACT) S.n_contact = S.n_contact + 1;
    S.n_blocked = S.n_blocked + blocked; S.n_rejected = S.n_rejected + rejected;
    S.cur_start = k; S.n_used[k] = S.n_used[k] + 1;
    episode_start_words(start_in[s].loc, E, s, trace, score);
}

// §4l 3a. from k0 on, 3. - 6.: the clearance walk and the restart onto the record it took
__device__ __forceinline__ void spawn_restart(const EpisodeSpawn& sp, double hw, int s, int lane, int stride, int k0, const SpawnEnd& E,
                                              const SceneIn* prev, SceneIn* staged, SceneState* state, const SceneIn* pool_in, const SceneState* pool_state,
                                              const int32_t* world_first, const int32_t* world_of, int32_t* flags,
                                              EpisodeStats* stats, EpisodeSpawnStats* sstats, EgoTrace* trace, RolloutScore* score)
{
    const int M = sp.n_starts;
    int p0 = 0, p1 = 0;
    if ((sp.check & 2) && world_of) { const int w = world_of[s]; p0 = world_first[w]; p1 = world_first[w + 1]; }
    int k = k0, rejected = M, blocked = 1;
    for (int i = 0; i < M; i++) {
        const int cand = (k0 + i) % M;
        const GlobalPoint3D P = pool_in[(size_t)cand * stride + s].loc.globalpoint;
        if ((sp.check & 1) && wave_slice_within(E.slice, E.on, P.x, P.y, hw, sp.clearance, lane)) continue;
        if (wave_world_within(prev, p0, p1, s, P.x, P.y, hw, sp.clearance, lane)) continue;
        k = cand; rejected = i; blocked = 0;
        break;
    }
    spawn_take_record(s, lane, stride, k, rejected, blocked, E, staged, state, pool_in, pool_state, flags, stats, sstats, trace, score);
}

// prev / obs: the SceneIn records and the obstacle pool (n_obs entries) of the input set the advance read; staged, state, flags, stats,
// trace, score: as k_respawn_egos.  pool_in / pool_state: the start records, record k of scene s at k * stride + s.  world_first /
// world_of: the fleet's tables, or null without a fleet.  hw = 0.5 * Vehicle_Width (rounded once, on the host: exact).
__global__ void __launch_bounds__(kBlock)
k_respawn_spawn(EpisodeModel em, EpisodeSpawn sp, double hw, int n_scenes, int stride, const SceneIn* __restrict__ prev, const ObPoint* __restrict__ obs, int n_obs,
                SceneIn* __restrict__ staged, SceneState* __restrict__ state, const SceneIn* __restrict__ pool_in, const SceneState* __restrict__ pool_state,
                const int32_t* __restrict__ world_first, const int32_t* __restrict__ world_of, int32_t* __restrict__ flags,
                EpisodeStats* __restrict__ stats, EpisodeSpawnStats* __restrict__ sstats, EgoTrace* __restrict__ trace, RolloutScore* __restrict__ score)
{
    const int lane = threadIdx.x & 63;
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kEpScenes + (threadIdx.x >> 6)));
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    SpawnEnd E;
    spawn_episode_end(em, sp, hw, s, lane, prev, obs, n_obs, staged, flags, stats, E);
    if (E.c == 0) { episode_go_on(s, lane, E, stats); return; }
    // 3a. start record
    const int M = sp.n_starts;
    const int e = stats[s].n_episodes + 1;
    int k0;
    if (sp.order == 0) k0 = (int)(((spawn_hash(sp, s, e) >> 32) * (unsigned long long)M) >> 32);
    else k0 = e % M;
    spawn_restart(sp, hw, s, lane, stride, k0, E, prev, staged, state, pool_in, pool_state, world_first, world_of, flags, stats, sstats, trace, score);
}

// obs_off / obs_n of start records 1 .. M - 1 become those of the scene's record 0 (one thread per record)
__global__ void __launch_bounds__(kBlock)
k_spawn_pin_slices(int n_scenes, int M, int stride, SceneIn* __restrict__ pool_in)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_scenes * (M - 1)) return;
    const int k = 1 + i / n_scenes, s = i % n_scenes;
    SceneIn& r = pool_in[(size_t)k * stride + s];
    r.obs_off = pool_in[s].obs_off; r.obs_n = pool_in[s].obs_n;
}

}  // namespace dmpp
