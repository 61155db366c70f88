// rollout_features.hpp — which rollout features a successful set call switches off, and what must hold between the features that
// stay on.  A feature holds data captured from what another call replaces (start records from the resident scenes, start states from
// the actors, ...): the call that replaces it RETIRES the feature.  Host only, pure: no HIP, no handle, no device (exported as
// pp_feature_retires / pp_feature_consistent; DESIGN.md §7 has the table in prose).
#pragma once

namespace dmpp {

// One bit per feature with an `on` flag on the handle.  kTraffic is traffic per scene (pp_set_traffic), kWorldTraffic traffic per
// world (pp_set_world_traffic): one TrafficState serves both, so at most one of the two is on.  kSchedule (pp_set_episode_schedule),
// kWorldEpisodes (pp_set_episode_worlds) and kWorldReset (pp_set_episode_world_traffic) have no cause: their set calls retire nothing.
enum Feature : unsigned {
    kFleet = 1, kRoute = 2, kTraffic = 4, kWorldTraffic = 8, kFollow = 16, kEpisodes = 32, kSpawn = 64, kTrafficReset = 128, kEpisodeLog = 256,
    kSchedule = 512, kWorldEpisodes = 1024, kWorldReset = 2048,
    kFeatureCount = 12, kAllFeatures = 4095
};
// What a successful call did, its off / NULL / zero form included.  kSetFleet + i is the set call of feature bit i, i < 9.
enum Cause : int {
    kResidentReplaced,          // pp_set_scenes, pp_set_egos, pp_set_n_scenes
    kMapReplaced,               // pp_set_map (also when a later allocation or copy in the call fails)
    kSetFleet, kSetRoute, kSetTraffic, kSetWorldTraffic, kSetFollow, kSetEpisodes, kSetSpawn, kSetTrafficReset, kSetEpisodeLog,
    kTrafficOff,                // pp_set_traffic / pp_set_world_traffic with no actors
    kSetGridFollow, kScoreBeginEnd, kCauseCount
};
constexpr int set_cause_of(int bit) { return bit < 9 ? kSetFleet + bit : -1; }      // -1: no cause, retires() is 0

// The features a cause retires.  Never retired by another call: the follow MODEL, the grid-follow model, the scorecard (it restarts
// instead) and every `ever` flag with the stats behind it.
constexpr unsigned retires(int cause)
{
    constexpr unsigned in_spawn = kSchedule | kWorldEpisodes | kWorldReset;      // part of the spawn model in force (§4p, §4s, §4t): gone with it, and with a new pool
    switch (cause) {
    case kResidentReplaced: return kFleet | kRoute | kTraffic | kWorldTraffic | kEpisodes | kSpawn | kTrafficReset | kEpisodeLog | in_spawn;
    case kMapReplaced:      return kRoute;                                    // the routes named roads of the old map
    case kSetFleet:         return kWorldTraffic | kWorldReset;               // pinned to the worlds the call replaces (§4j); n_worlds = 0 on a handle with a fleet included
    case kSetTraffic:
    case kSetWorldTraffic:  return kTrafficReset | kWorldReset;               // start states captured from the actors the call replaces (§4m, §4t)
    case kTrafficOff:       return kTraffic | kWorldTraffic | kTrafficReset | kWorldReset;
    case kSetFollow:        return kTrafficReset | kWorldReset;               // ... captured under the model the call replaces; also on a handle whose traffic is off
    case kSetEpisodes:      return kSpawn | kTrafficReset | kEpisodeLog | in_spawn;      // record 0 of the pool, set 0 of the reset, the episodes the log numbered
    case kSetSpawn:         return kTrafficReset | kEpisodeLog | in_spawn;    // the first two read cur_start of the model in force
    default:                return 0;                                         // pp_set_route, pp_set_episode_traffic, pp_set_episode_log, pp_set_grid_follow, pp_score_begin / _end
    }
}

// What holds between the features of a handle after every set call.
constexpr bool consistent(unsigned m, bool have_map, int resident_mode)
{
    const bool episodes = (m & kEpisodes) != 0;
    if ((m & kTraffic) && (m & kWorldTraffic)) return false;                  // (one traffic set per handle)
    if ((m & kSpawn) && !episodes) return false;
    if ((m & kTrafficReset) && !((m & kTraffic) && !(m & kWorldTraffic) && episodes)) return false;
    if ((m & kEpisodeLog) && !episodes) return false;
    if ((m & kWorldTraffic) && !(m & kFleet)) return false;
    if ((m & kRoute) && !(have_map && resident_mode == 1)) return false;
    if ((m & kSchedule) && !(m & kSpawn)) return false;
    if ((m & kWorldEpisodes) && !(m & kSpawn)) return false;
    if ((m & kSchedule) && (m & kWorldEpisodes)) return false;                // (a schedule keeps rows per scene, a world draws once)
    if ((m & kWorldReset) && !((m & kWorldTraffic) && episodes && (m & kSpawn) && (m & kWorldEpisodes))) return false;
    return true;
}

// The features that are on in no consistent mask without `feature`: what the off form of its set call takes off with it.
constexpr unsigned dependants(unsigned feature)
{
    unsigned free = 0;
    for (unsigned m = 0; m <= kAllFeatures; m++) if (!(m & feature) && consistent(m, true, 1)) free |= m;
    return kAllFeatures & ~free & ~feature;
}
static_assert(dependants(kWorldEpisodes) == kWorldReset && dependants(kSchedule) == 0 && dependants(kWorldReset) == 0, "the features without a cause");

// The masks are transitively closed: a cause that retires X retires every Y that the set call of X retires - X's dependants -,
// unless X and Y are never on together (world traffic and the traffic reset: the reset holds nothing of world traffic).
constexpr bool together(unsigned x, unsigned y)
{
    for (unsigned m = 0; m <= kAllFeatures; m++) if ((m & x) && (m & y) && consistent(m, true, 1)) return true;
    return false;
}
constexpr bool closed()
{
    for (int c = 0; c < kCauseCount; c++)
        for (int i = 0; i < kFeatureCount; i++)
            for (int j = 0; j < kFeatureCount; j++)
                if ((retires(c) >> i & 1) && (retires(set_cause_of(i)) >> j & 1) && !(retires(c) >> j & 1) && together(1u << i, 1u << j)) return false;
    return true;
}
static_assert(closed(), "a cause retires a feature and not what depends on it");
// ... and what every cause leaves of a consistent state is consistent
constexpr bool kept()
{
    for (unsigned m = 0; m <= kAllFeatures; m++)
        if (consistent(m, true, 1))
            for (int c = 0; c < kCauseCount; c++) if (!consistent(m & ~retires(c), true, 1)) return false;
    return true;
}
static_assert(kept(), "a cause leaves a feature on without what it needs");

}  // namespace dmpp
