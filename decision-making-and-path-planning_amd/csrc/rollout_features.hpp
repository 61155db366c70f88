// rollout_features.hpp — which rollout features a successful set call switches off, and what must hold between the features that
// stay on.  A feature holds data captured from what another call replaces (start records from the resident scenes, start states from
// the actors, ...): the call that replaces it RETIRES the feature.  Host only, pure: no HIP, no handle, no device (exported as
// pp_feature_retires / pp_feature_consistent; DESIGN.md §7 has the table in prose).
#pragma once

namespace dmpp {

// One bit per feature with an `on` flag on the handle.  kTraffic is traffic per scene (pp_set_traffic), kWorldTraffic traffic per
// world (pp_set_world_traffic): one TrafficState serves both, so at most one of the two is on.
enum Feature : unsigned {
    kFleet = 1, kRoute = 2, kTraffic = 4, kWorldTraffic = 8, kFollow = 16, kEpisodes = 32, kSpawn = 64, kTrafficReset = 128, kEpisodeLog = 256,
    kFeatureCount = 9, kAllFeatures = 511
};
// What a successful call did, its off / NULL / zero form included.  kSetFleet + i is the set call of feature bit i.
enum Cause : int {
    kResidentReplaced,          // pp_set_scenes, pp_set_egos, pp_set_n_scenes
    kMapReplaced,               // pp_set_map (also when a later allocation or copy in the call fails)
    kSetFleet, kSetRoute, kSetTraffic, kSetWorldTraffic, kSetFollow, kSetEpisodes, kSetSpawn, kSetTrafficReset, kSetEpisodeLog,
    kTrafficOff,                // pp_set_traffic / pp_set_world_traffic with no actors
    kSetGridFollow, kScoreBeginEnd, kCauseCount
};

// The features a cause retires.  Never retired by another call: the follow MODEL, the grid-follow model, the scorecard (it restarts
// instead) and every `ever` flag with the stats behind it.
constexpr unsigned retires(int cause)
{
    switch (cause) {
    case kResidentReplaced: return kFleet | kRoute | kTraffic | kWorldTraffic | kEpisodes | kSpawn | kTrafficReset | kEpisodeLog;
    case kMapReplaced:      return kRoute;                                    // the routes named roads of the old map
    case kSetFleet:         return kWorldTraffic;                             // pinned to the worlds the call replaces (§4j); n_worlds = 0 on a handle with a fleet included
    case kSetTraffic:
    case kSetWorldTraffic:  return kTrafficReset;                             // start states captured from the actors the call replaces (§4m)
    case kTrafficOff:       return kTraffic | kWorldTraffic | kTrafficReset;
    case kSetFollow:        return kTrafficReset;                             // ... captured under the model the call replaces; also on a handle whose traffic is off
    case kSetEpisodes:      return kSpawn | kTrafficReset | kEpisodeLog;      // record 0 of the pool, set 0 of the reset, the episodes the log numbered
    case kSetSpawn:         return kTrafficReset | kEpisodeLog;               // both read cur_start of the model in force
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
    return true;
}

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
                if ((retires(c) >> i & 1) && (retires(kSetFleet + i) >> j & 1) && !(retires(c) >> j & 1) && together(1u << i, 1u << j)) return false;
    return true;
}
static_assert(closed(), "a cause retires a feature and not what depends on it");

}  // namespace dmpp
