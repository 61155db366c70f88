// kernels_ew.hpp — world episodes (build-defined): k_respawn_world runs in the place of k_respawn_spawn while
// pp_set_episode_worlds is in force.  The WORLD is the unit of an episode: when any ego of a world ends, every ego of that world
// restarts on this advance, on one start record index drawn for the world.
//
// One 256-thread workgroup per world, its four waves striding the members (wave v takes members a + v, a + v + 4, ..), so a
// member is handled by the same wave in every phase and a world of any size fits.  Without a fleet a world is one scene.
//   phase 1  own causes: spawn_episode_end per member (all of it from what stood BEFORE this step), (f, age, c, dist) into the
//            per-scene scratch array `ends` (worlds may have thousands of members), the wave's count of enders into LDS;
//   barrier  - behind it nobody reads a member's EpisodeStats / flag word again but the wave that owns the member;
//   verdict  no ender: episode_go_on per member and out.  Else
//   phase 2  the candidate walk, uniform over the workgroup: per candidate the waves test their members' OWN entries against record
//            k of that member, a wave that finds one within the clearance stores 1 into the candidate's LDS word, one barrier, and
//            the walk leaves on the first word that stayed 0;
//   phase 3  the restarts: wave_copy_record of record k, episode_close with the world's cause word, the spawn-stats words (the same
//            in every member), episode_start_words.
// Barriers are reached by whole workgroups only: the world index is uniform per block and every trip count between two barriers
// depends on LDS words read behind a barrier.  No scratch memory, no atomics: the LDS words are written with plain stores (a 1 by
// lane 0 of whichever wave found a blocker - every writer writes the same value).
#pragma once
#include "kernels_es.hpp"
#include "kernels_f.hpp"

namespace dmpp {

static_assert(DMPP_EGO_WORLD == 256, "cause bit of §4s");
constexpr int kWorldWaves = kBlock / 64;     // waves of a world's workgroup

// what phase 1 leaves of a member for phase 3
struct alignas(8) WorldEnd { int32_t f, age, c, _pad; double dist; };      // 24 B

// the OWN entries of member m (§4s 4.): with a fleet the pinned slice without its peer slots, without one the slice of the record
// the advance read; a slice that does not lie inside the pool is empty
__device__ __forceinline__ const ObPoint* world_own_slice(const SceneIn* __restrict__ prev, const FleetPin* __restrict__ fpin, const ObPoint* __restrict__ obs, int n_obs, int m, int& on)
{
    int off, n;
    if (fpin) { off = fpin[m].obs_off; n = fpin[m].n_own; }
    else { off = prev[m].obs_off; n = prev[m].obs_n; }
    if (n <= 0 || off < 0 || (long long)off + n > (long long)n_obs) { off = 0; n = 0; }
    on = n;
    return obs + off;
}

// n_worlds blocks.  world_first: the fleet's table, or null without a fleet (world w is scene w); fpin: the fleet's pinned slices,
// or null.  ends: n_scenes records of scratch.  Everything else as k_respawn_spawn.
__global__ void __launch_bounds__(kBlock)
k_respawn_world(EpisodeModel em, EpisodeSpawn sp, double hw, int stride, const SceneIn* __restrict__ prev, const ObPoint* __restrict__ obs, int n_obs,
                SceneIn* __restrict__ staged, SceneState* __restrict__ state, const SceneIn* __restrict__ pool_in, const SceneState* __restrict__ pool_state,
                const int32_t* __restrict__ world_first, const FleetPin* __restrict__ fpin, int32_t* __restrict__ flags,
                EpisodeStats* __restrict__ stats, EpisodeSpawnStats* __restrict__ sstats, EgoTrace* __restrict__ trace, RolloutScore* __restrict__ score,
                WorldEnd* __restrict__ ends)
{
    __shared__ int s_enders[kWorldWaves];
    __shared__ int s_blocked[DMPP_EPISODE_MAX_STARTS];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = blockIdx.x;
    const int a = world_first ? world_first[w] : w, b = world_first ? world_first[w + 1] : w + 1;
    if (a >= b) return;                                 // (pp_set_fleet refuses an empty world: never taken; the whole workgroup would leave)
    if (threadIdx.x < DMPP_EPISODE_MAX_STARTS) s_blocked[threadIdx.x] = 0;
    const int e = stats[a].n_episodes + 1;              // (read in front of the barrier: behind it the wave of member a closes the record)
    // phase 1: own causes
    int mine = 0;
    for (int m = a + wv; m < b; m += kWorldWaves) {
        SpawnEnd E;
        spawn_episode_end(em, sp, hw, m, lane, prev, obs, n_obs, staged, flags, stats, E);
        if (lane == 0) { WorldEnd r; r.f = E.f; r.age = E.age; r.c = E.c; r._pad = 0; r.dist = E.dist; ends[m] = r; }
        mine += E.c != 0;
    }
    if (lane == 0) s_enders[wv] = mine;
    __syncthreads();
    int enders = 0;
    for (int v = 0; v < kWorldWaves; v++) enders += s_enders[v];
    // 2. verdict
    if (enders == 0) {
        for (int m = a + wv; m < b; m += kWorldWaves) {
            const WorldEnd r = ends[m];
            EpisodeEnd E; E.f = r.f; E.age = r.age; E.c = 0; E.dist = r.dist;
            episode_go_on(m, lane, E, stats);
        }
        return;
    }
    // 3a. one draw per world: the world's first scene stands for the world
    const int M = sp.n_starts;
    int k0;
    if (sp.order == 0) k0 = (int)(((spawn_hash(sp, a, e) >> 32) * (unsigned long long)M) >> 32);
    else k0 = e % M;
    int k = k0, rejected = 0, blocked = 0;
    if (sp.check & 1) {                                 // phase 2 (check bit 1 is ignored: every ego of the world moves in this step)
        rejected = M; blocked = 1;
        for (int i = 0; i < M; i++) {
            const int cand = (k0 + i) % M;
            bool hit = false;
            for (int m = a + wv; m < b && !hit; m += kWorldWaves) {
                int on;
                const ObPoint* own = world_own_slice(prev, fpin, obs, n_obs, m, on);
                const GlobalPoint3D P = pool_in[(size_t)cand * stride + m].loc.globalpoint;
                hit = wave_slice_within(own, on, P.x, P.y, hw, sp.clearance, lane);
            }
            if (hit && lane == 0) s_blocked[i] = 1;
            __syncthreads();
            if (s_blocked[i] == 0) { k = cand; rejected = i; blocked = 0; break; }      // (the same word in every thread: the workgroup leaves together)
        }
    }
    // phase 3: 3. - 6. for every member, with record k of that member
    for (int m = a + wv; m < b; m += kWorldWaves) {
        const WorldEnd r = ends[m];
        SpawnEnd E;
        E.f = r.f; E.age = r.age; E.dist = r.dist; E.on = 0; E.slice = nullptr;
        E.c = r.c | (enders - (r.c != 0) > 0 ? DMPP_EGO_WORLD : 0);      // some OTHER member ended
        spawn_take_record(m, lane, stride, k, rejected, blocked, E, staged, state, pool_in, pool_state, flags, stats, sstats, trace, score);
    }
}

}  // namespace dmpp
