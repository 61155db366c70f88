// kernels_ep.hpp — episodic rollouts: k_respawn_egos puts an ego whose episode ended back on its start records (DESIGN.md §4k;
// build-defined).  It runs on the upload stream directly behind k_advance_egos / k_advance_route, in front of the traffic
// kernels, k_couple_fleet, k_resolve_map and k_sanitise_scenes, and is launched only while episodes are on.
//
// One 64-lane wave per scene, four scenes per 256-thread block, no LDS, no barrier (the shape of k_advance_egos).  The scene
// index is made wave-uniform for the compiler (readfirstlane), so the flag word, the age, the two positions and the cause are
// scalar loads / scalar arithmetic and the wave branches once on the cause.  A scene that goes on costs one wave two stores;
// only an ending scene copies its SceneIn (248 B) and its SceneState (3424 B), the lanes striding over 16-byte pieces.  Lane 0
// writes the stats, the flag word, the trace record and the two scorecard fields with plain stores.
#pragma once
#include "dev_geom.hpp"

namespace dmpp {

constexpr int kEpScenes = 4;           // scenes (waves) per block of k_respawn_egos

// Record s of an array of T copied over record s of another: both arrays start on a 16-byte boundary (every device allocation
// does) and hold the record at the same byte offset, so source and destination share their phase within 16 bytes.  A record
// whose size is an odd multiple of 8 starts on an odd multiple of 8 in every second slot: then 8 bytes go first, the 16-byte
// pieces follow, and whatever is left - 8 bytes or nothing - goes last.
template <class T>
__device__ __forceinline__ void wave_copy_record(T* __restrict__ dst, const T* __restrict__ src, int lane)
{
    static_assert(sizeof(T) % 8 == 0 && alignof(T) == 8, "records are copied as one optional 8-byte head, 16-byte pieces and one optional 8-byte tail");
    static_assert(sizeof(uint4) == 16 && sizeof(unsigned long long) == 8, "piece sizes");
    char* d = reinterpret_cast<char*>(dst);
    const char* q = reinterpret_cast<const char*>(src);
    const int head = (int)(reinterpret_cast<uintptr_t>(d) & 8);                      // 0 or 8: bytes in front of the first 16-byte boundary
    const int body = ((int)sizeof(T) - head) >> 4;                                   // whole 16-byte pieces
    const int tail = (int)sizeof(T) - head - (body << 4);                            // 0 or 8
    if (head && lane == 0) *reinterpret_cast<unsigned long long*>(d) = *reinterpret_cast<const unsigned long long*>(q);
    for (int i = lane; i < body; i += 64)
        reinterpret_cast<uint4*>(d + head)[i] = reinterpret_cast<const uint4*>(q + head)[i];
    if (tail && lane == 63) {
        const int o = head + (body << 4);
        *reinterpret_cast<unsigned long long*>(d + o) = *reinterpret_cast<const unsigned long long*>(q + o);
    }
}

static_assert(sizeof(EpisodeStats) == 80 && offsetof(EpisodeStats, ticks_total) == 48 && offsetof(EpisodeStats, dist) == 56, "EpisodeStats layout (DESIGN.md §4k)");
static_assert(DMPP_EGO_PATH_END == 1 && DMPP_EGO_BAD_PATH == 2 && DMPP_EGO_LANE_END == 4 && DMPP_EGO_OFF_GRID == 8 && DMPP_EGO_ROUTE_END == 16 &&
              DMPP_EGO_TIMEOUT == 64, "n_end[b] counts bit b of the cause word, TIMEOUT in n_end[5]");

// What steps 1 - 2 leave for the steps behind them: the flag word the advance left, the age and the metres of the running episode
// and its cause word.
struct EpisodeEnd { int f, age, c; double dist; };

// The numbered steps of §4k as device functions: k_respawn_egos, k_respawn_spawn (kernels_es.hpp, §4l) and k_respawn_sched
// (kernels_ev.hpp, §4p) are made of the same ones.  (The pointers are the kernels' own __restrict__ arguments.  The test E.c == 0 and
// the early return stay in the kernel: folded into a function that also stores, the compiler merges the uniform test with the lane
// test into one divergent branch.)
// §4k 1.: age and distance of the running episode, from the pose the advance read (px, py) and the one it staged (qx, qy)
__device__ __forceinline__ void episode_age_dist(const EpisodeStats& e, double px, double py, double qx, double qy, EpisodeEnd& E)
{
    E.age = e.age + 1;
    const double ex = qx - px, ey = qy - py;
    E.dist = e.dist + sqrt(ex * ex + ey * ey);
}
// §4k 2.: the base of the cause word (§4l ORs CONTACT on top)
__device__ __forceinline__ int episode_cause(const EpisodeModel& em, int f, int age)
{
    return (f & em.end_mask) | ((em.max_ticks > 0 && age >= em.max_ticks) ? DMPP_EGO_TIMEOUT : 0);
}
// §4k 2., cause word 0: a scene that goes on costs lane 0 two stores
__device__ __forceinline__ void episode_go_on(int s, int lane, const EpisodeEnd& E, EpisodeStats* stats)
{
    if (lane == 0) { stats[s].age = E.age; stats[s].dist = E.dist; }
}
// §4k 3.: the running episode is closed in the scene's stats (one lane)
__device__ __forceinline__ void episode_close(EpisodeStats& stats, const EpisodeEnd& E)
{
    const int c = E.c, age = E.age;
    EpisodeStats e = stats;
    e.n_episodes = e.n_episodes + 1;
    for (int b = 0; b < 5; b++) if (c & (1 << b)) e.n_end[b] = e.n_end[b] + 1;
    if (c & DMPP_EGO_TIMEOUT) e.n_end[5] = e.n_end[5] + 1;
    e.last_cause = c; e.last_age = age;
    if (e.min_age < 0 || age < e.min_age) e.min_age = age;
    if (e.max_age < 0 || age > e.max_age) e.max_age = age;
    e.ticks_total = e.ticks_total + (int64_t)age;
    e.last_dist = E.dist; e.dist_total = e.dist_total + E.dist;
    e.age = 0; e.dist = 0;
    stats = e;
}
// §4k 5. trace of the start record L   6. the scorecard's last ego is the one of the start record (one lane).  The mask names
// CONTACT for §4l: pp_set_episodes refuses an end_mask outside 31, so without the spawn model a cause word never holds bit 128 and
// the wider mask gives k_respawn_egos the bytes of TIMEOUT alone.
__device__ __forceinline__ void episode_start_words(const LocationOut& L, const EpisodeEnd& E, int s, EgoTrace* trace, RolloutScore* score)
{
    if (trace) {
        EgoTrace t;
        t.pose = L.globalpoint; t.velocity = L.velocity;
        t.id_cur = L.id[clampi(L.lane_num - 1, 0, DMPP_LANESUM - 1)]; t.lane_num = L.lane_num;
        t.flags = E.f | DMPP_EGO_RESPAWNED | (E.c & (DMPP_EGO_TIMEOUT | DMPP_EGO_CONTACT)); t._pad = 0;
        trace[s] = t;
    }
    if (score) { score[s].last_pos.x = L.globalpoint.x; score[s].last_pos.y = L.globalpoint.y; score[s].last_speed = L.velocity; }
}

// prev: the SceneIn records the advance read; staged: the ones it wrote (restored here for an ending scene); trace: the trace
// of this advance or null; score: the scorecard records while scoring is on, else null.
__global__ void __launch_bounds__(kBlock)
k_respawn_egos(EpisodeModel em, int n_scenes, const SceneIn* __restrict__ prev, SceneIn* __restrict__ staged, SceneState* __restrict__ state,
               const SceneIn* __restrict__ start_in, const SceneState* __restrict__ start_state, int32_t* __restrict__ flags,
               EpisodeStats* __restrict__ stats, EgoTrace* __restrict__ trace, RolloutScore* __restrict__ score)
{
    const int lane = threadIdx.x & 63;
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kEpScenes + (threadIdx.x >> 6)));
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    EpisodeEnd E;
    E.f = flags[s];
    episode_age_dist(stats[s], prev[s].loc.globalpoint.x, prev[s].loc.globalpoint.y, staged[s].loc.globalpoint.x, staged[s].loc.globalpoint.y, E);
    E.c = episode_cause(em, E.f, E.age);
    if (E.c == 0) { episode_go_on(s, lane, E, stats); return; }
    // 4. restart: SceneIn and SceneState of the scene become its start records, every byte
    wave_copy_record(&staged[s], &start_in[s], lane);
    wave_copy_record(&state[s], &start_state[s], lane);
    if (lane != 0) return;
    episode_close(stats[s], E);
    flags[s] = 0;
    episode_start_words(start_in[s].loc, E, s, trace, score);
}

// the starting values of the stats (-1, -1 for min_age / max_age: not all zero bits)
__global__ void __launch_bounds__(kBlock)
k_episode_reset(int n_scenes, EpisodeStats* __restrict__ stats)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_scenes) return;
    EpisodeStats e;
    e.n_episodes = 0; e.age = 0;
    for (int b = 0; b < 6; b++) e.n_end[b] = 0;
    e.last_cause = 0; e.last_age = 0; e.min_age = -1; e.max_age = -1;
    e.ticks_total = 0; e.dist = 0; e.last_dist = 0; e.dist_total = 0;
    stats[s] = e;
}

}  // namespace dmpp
