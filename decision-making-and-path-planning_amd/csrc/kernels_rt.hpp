// kernels_rt.hpp — route following: k_advance_route is k_advance_egos for a handle with routes set (build-defined: the
// simulated localisation module of a rollout).  The frame - record load, pose, grid test, stores - is adv_scene of kernels_a.hpp, the
// id searches its device functions; a scene that follows no route takes §4c 4. - 5. through them unchanged.  For a routed scene §4f stands in the place
// of those two steps: the ego goes road -> pre-junction (pos 1) -> junction (pos 2) -> next road (pos 0) on the junction table and
// the polylines of the resident map.
//
// The shape of k_advance_egos: one 64-lane wave per scene, four scenes per block, the record as one 32-bit word per lane, ids from
// wave_first_min, no LDS, no barrier.  The junction lookup is a wave scan of the table: 64 entries per pass, the first match of a
// pass by ballot, so the lowest index wins.  Every branch below depends on values that are the same in all lanes of the wave.
#pragma once
#include "kernels_a.hpp"

namespace dmpp {

constexpr int kPosWord = (int)(offsetof(LocationOut, pos) / 4), kRoadWord = (int)(offsetof(LocationOut, road_num) / 4);
constexpr int kLastRoadWord = (int)(offsetof(LocationOut, last_roadnum) / 4), kNextRoadWord = (int)(offsetof(LocationOut, next_roadnum) / 4);
constexpr int kLastLaneWord = (int)(offsetof(LocationOut, last_lanenum) / 4), kNextLaneWord = (int)(offsetof(LocationOut, next_lanenum) / 4);
constexpr int kPathNumWord = (int)(offsetof(LocationOut, path_num) / 4);
constexpr int kStubWord = (int)(offsetof(SceneIn, stub_attribute) / 4), kOutLaneWord = (int)(offsetof(SceneIn, out_lane_no) / 4);
constexpr int kOutLaneWords = (int)(sizeof(uint16_t) * DMPP_LANESUM / 4);
static_assert(offsetof(SceneIn, out_lane_no) % 4 == 0 && (sizeof(uint16_t) * DMPP_LANESUM) % 4 == 0, "out_lane_no travels as whole words");
static_assert(sizeof(RouteLeg) == 8 + sizeof(uint16_t) * DMPP_LANESUM && offsetof(RouteLeg, stub_attribute) == 4 && offsetof(RouteLeg, out_lane_no) == 8,
              "a leg is read as words: road_num, stub_attribute, out_lane_no");

// J(road, next_road, lane) of §4f: the lowest index of the junction table with these three keys, -1 if there is none
__device__ __forceinline__ int wave_find_junction(const MapJunction* __restrict__ J, int n, int road, int next_road, int last_lane, int lane)
{
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool hit = false;
        if (i < n) { const MapJunction q = J[i]; hit = q.last_road == road && q.next_road == next_road && q.last_lane == last_lane; }
        const unsigned long long b = wave_ballot(hit);
        if (b) return base + __ffsll((long long)b) - 1;
    }
    return -1;
}

__device__ __forceinline__ void rt_zero_ids(int& w, int lane) { if (lane >= kIdWord && lane < kIdWord + DMPP_LANESUM) w = 0; }

// §4f in the place of §4c 4. - 5. for one scene at its new pose p (a scene that follows no route takes those two steps unchanged)
__device__ __forceinline__ void rt_route_step(const RouteModel& rm, int window, int s, const SceneIn& si, int ln, const AdvPose& p,
                                              const GlobalPoint3D* __restrict__ lane_pool, const GlobalPoint2D* __restrict__ ref_pool, int n_junctions,
                                              const MapJunction* __restrict__ junctions, const RouteLeg* __restrict__ legs, const int32_t* __restrict__ route_first,
                                              int lane, int& w, int& f, int& ln_new)
{
    const int pos = si.loc.pos, leg = si.loc.path_num;
    const int r0 = route_first[s], n_legs = route_first[s + 1] - r0;
    const bool routed = n_legs > 0 && leg >= 0 && leg < n_legs && pos >= 0 && pos <= 2;
    if (!routed) adv_lane_step(lane_pool, si.lanes, ln, window, 1, p.x, p.y, lane, w, f, ln_new);       // (routes live on a resident map)
    else if (pos != 2) {
        // ---- on a lane: ids as §4c 4.; the lane number as §4c 5. on the road, held in the pre-junction ----
        const LaneView& lv = si.lanes;
        const AdvIds r = adv_search_ids(lane_pool, lv, ln, window, p.x, p.y, lane, w);
        adv_store_ids(w, lane, ln, r);
        if (pos == 0 && r.ic >= 0) {
            ln_new = adv_lane_number(lv, ln, r);
            if (lane == kLaneNumWord) w = ln_new;
        }
        if (r.has_c) {
            const int idc = r.ic >= 0 ? r.ic : adv_get_id(w, ln - 1);
            const bool has_next = leg + 1 < n_legs;
            int next_road = 0, jn = -1, jn_next_lane = 0;
            if (has_next && !(pos == 1 && si.ref_n <= 0)) {
                next_road = legs[r0 + leg + 1].road_num;
                jn = wave_find_junction(junctions, n_junctions, si.loc.road_num, next_road, ln_new, lane);
                if (jn >= 0) jn_next_lane = junctions[jn].next_lane;
            }
            if (adv_lane_ends(lv, idc, window)) {
                if (!has_next) f |= DMPP_EGO_LANE_END | DMPP_EGO_ROUTE_END;       // the last leg: arrived
                else if (jn < 0) f |= DMPP_EGO_LANE_END;                          // missed its exit lane
            }
            if (pos == 0 && jn >= 0 && (long long)lv.cur_n - 1 - idc <= (long long)rm.pre_points) {      // 0 -> 1
                if (lane == kPosWord) w = 1;
                if (lane == kLastRoadWord) w = si.loc.road_num;
                if (lane == kNextRoadWord) w = next_road;
                if (lane == kLastLaneWord) w = ln_new;
                if (lane == kNextLaneWord) w = jn_next_lane;
            }
            if (pos == 1 && idc == lv.cur_n - 1 && si.ref_n > 0) {                                         // 1 -> 2
                double d2; int jid;
                wave_view_nearest(ref_pool + si.ref_off, si.ref_n, 0, window, p.x, p.y, lane, d2, jid);
                rt_zero_ids(w, lane);
                adv_set_id(w, lane, clampi(si.loc.last_lanenum - 1, 0, DMPP_LANESUM - 1), jid >= 0 ? jid : 0);
                ln_new = si.loc.next_lanenum;
                if (lane == kPosWord) w = 2;
                if (lane == kRoadWord) w = si.loc.next_roadnum;
                if (lane == kLaneNumWord) w = ln_new;
            }
        }
    } else {
        // ---- in the junction: the id of the polyline; no lane ids, no lane-end test, the lane number is held ----
        const int slot = clampi(si.loc.last_lanenum - 1, 0, DMPP_LANESUM - 1);
        const int j = adv_get_id(w, slot);
        double d2; int jid;
        wave_view_nearest(ref_pool + si.ref_off, si.ref_n, j, window, p.x, p.y, lane, d2, jid);
        const int jn = jid >= 0 ? jid : j;
        adv_set_id(w, lane, slot, jn);
        if (jn >= si.ref_n - 1) {                                                                          // 2 -> 0
            if (leg + 1 >= n_legs) f |= DMPP_EGO_ROUTE_END;       // (a caller error: a junction behind the last leg; everything is held)
            else {
                const int* __restrict__ L = reinterpret_cast<const int*>(&legs[r0 + leg + 1]);
                if (lane == kPosWord) w = 0;
                if (lane == kPathNumWord) w = leg + 1;
                if (lane == kStubWord) w = L[1];
                if (lane >= kOutLaneWord && lane < kOutLaneWord + kOutLaneWords) w = L[2 + lane - kOutLaneWord];
                rt_zero_ids(w, lane);
                const AdvIds r = adv_search_ids(lane_pool, si.lanes, ln, window, p.x, p.y, lane, w);     // (the views are those of the new road)
                adv_store_ids(w, lane, ln, r);
            }
        }
    }
}

template <bool kTrack>
__global__ void __launch_bounds__(kBlock)
k_advance_route(PlannerConfig c, EgoModel m, RouteModel rm, GridFollow gf, int n_scenes, const SceneIn* __restrict__ in, SceneIn* __restrict__ out,
                const PlanOut* __restrict__ plan, const SceneState* __restrict__ state, const GlobalPoint3D* __restrict__ lane_pool,
                const GlobalPoint2D* __restrict__ ref_pool, int n_junctions, const MapJunction* __restrict__ junctions,
                const RouteLeg* __restrict__ legs, const int32_t* __restrict__ route_first, int32_t* __restrict__ flags, EgoTrace* __restrict__ trace,
                typename AdvTrackArg<kTrack>::type trk)
{
    adv_scene<kTrack>(c, m, gf, n_scenes, in, out, plan, state, flags, trace, trk,
                      [&](int s, const SceneIn& si, int ln, const AdvPose& p, int lane, int& w, int& f, int& ln_new) {
                          rt_route_step(rm, m.window, s, si, ln, p, lane_pool, ref_pool, n_junctions, junctions, legs, route_first, lane, w, f, ln_new);
                      });
}

}  // namespace dmpp
