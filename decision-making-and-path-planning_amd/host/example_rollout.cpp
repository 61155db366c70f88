// example_rollout.cpp — closed-loop evaluation through the C-ABI: 256 generated scenes, every ego follows what the planner
// tells it for 50 ticks (pp_rollout: advance + tick on the device, no host wait, no per-tick PCIe traffic), then the host looks
// at where they ended up: how many scenes carry which rollout flag and how far the egos travelled.  The rollout is scored on the
// device (pp_score_begin: one RolloutScore record per scene, nothing fetched per tick): collisions, worst clearance, distance.
// With --fleet the egos share one world (pp_set_fleet): every scene keeps 8 free pool entries behind its own
// obstacles, the nearest egos are written there after every advance, and the scorecard tells ego-ego contact from the rest.
// Exit code 0 = ran on the GPU.
#include "../../include/dmpp_planner.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(expr) do { int rc__ = (expr); if (rc__) { std::fprintf(stderr, "%s: %s\n", #expr, pp_last_error()); return 2; } } while (0)

int main(int argc, char** argv)
{
    const bool fleet = argc > 1 && std::strcmp(argv[1], "--fleet") == 0;
    const int n = 256, n_obs = 24, ticks = 50;
    PlannerConfig cfg; pp_default_config(&cfg, 256, 256);
    PlannerCaps caps{}; caps.max_scenes = n; caps.max_obs_total = n * n_obs; caps.max_lane_pts_total = n * 3 * PP_GEN_LANE_PTS; caps.max_ref_pts_total = n * PP_GEN_REF_PTS;
    std::vector<SceneIn> in(n); std::vector<SceneState> st(n);
    std::vector<GlobalPoint3D> lanes((size_t)n * 3 * PP_GEN_LANE_PTS); std::vector<uint8_t> attr(lanes.size());
    std::vector<GlobalPoint2D> ref((size_t)n * PP_GEN_REF_PTS); std::vector<ObPoint> obs((size_t)n * n_obs); std::vector<ObMotion> mot(obs.size());
    CHECK(pp_gen_scenes(&cfg, 300, n, n_obs, 8, in.data(), lanes.data(), attr.data(), ref.data(), obs.data(), mot.data(), st.data()));
    FleetModel fm; pp_default_fleet_model(&fm);
    if (fleet) {                                      // the slices move apart: n_obs own entries, then fm.max_peers free peer slots
        const int stride = n_obs + fm.max_peers;
        std::vector<ObPoint> wide((size_t)n * stride);
        for (int s = 0; s < n; s++) {
            for (int j = 0; j < n_obs; j++) wide[(size_t)s * stride + j] = obs[(size_t)in[(size_t)s].obs_off + j];
            in[(size_t)s].obs_off = s * stride; in[(size_t)s].obs_n = n_obs;
        }
        obs.swap(wide); caps.max_obs_total = n * stride;
    }
    pp_handle h = nullptr;
    CHECK(pp_create(&cfg, 0, &caps, &h));
    CHECK(pp_set_scenes(h, n, in.data(), lanes.data(), attr.data(), (int)lanes.size(), ref.data(), (int)ref.size(), obs.data(), nullptr, (int)obs.size()));
    CHECK(pp_set_state(h, st.data(), n));
    if (fleet) { const int32_t world_first[2] = { 0, n }; CHECK(pp_set_fleet(h, 1, world_first, &fm)); }      // one world of all egos

    EgoModel model; pp_default_ego_model(&model);
    EgoTrace* trace = (EgoTrace*)pp_host_alloc(sizeof(EgoTrace) * (size_t)ticks * n);      // pinned: the kernel writes it over PCIe
    if (!trace) { std::fprintf(stderr, "pp_host_alloc: %s\n", pp_last_error()); return 2; }
    long long last = 0;
    CHECK(pp_score_begin(h, model.dt));
    CHECK(pp_rollout(h, ticks, &model, trace, &last));
    CHECK(pp_sync(h));
    std::vector<int32_t> flags(n);
    CHECK(pp_get_ego_flags(h, flags.data(), n));

    int n_end = 0, n_bad = 0, n_lane = 0, n_grid = 0, n_free = 0;
    double dist = 0;
    for (int s = 0; s < n; s++) {
        const int f = flags[(size_t)s];
        n_end += (f & DMPP_EGO_PATH_END) != 0; n_bad += (f & DMPP_EGO_BAD_PATH) != 0; n_lane += (f & DMPP_EGO_LANE_END) != 0;
        n_grid += (f & DMPP_EGO_OFF_GRID) != 0; n_free += f == 0;
        GlobalPoint3D p = in[(size_t)s].loc.globalpoint;               // odometer: the steps of the trace, one after the other
        for (int t = 0; t < ticks; t++) {
            const GlobalPoint3D q = trace[(size_t)t * n + s].pose;
            dist += std::sqrt((q.x - p.x) * (q.x - p.x) + (q.y - p.y) * (q.y - p.y));
            p = q;
        }
    }
    std::printf("rolled %d scenes out for %d ticks (last tick id %lld): %d free, PATH_END %d, BAD_PATH %d, LANE_END %d, OFF_GRID %d; mean distance travelled %.2f m\n",
                n, ticks, last, n_free, n_end, n_bad, n_lane, n_grid, dist / n);
    std::vector<RolloutScore> score(n);
    CHECK(pp_score_end(h));
    CHECK(pp_get_rollout_score(h, score.data(), n));
    int n_hit = 0, hit_ticks = 0, worst = 0; double sdist = 0;
    for (int s = 0; s < n; s++) {
        const RolloutScore& r = score[(size_t)s];
        n_hit += r.n_collision_ticks > 0; hit_ticks += r.n_collision_ticks; sdist += r.dist;
        if (r.min_clearance < score[(size_t)worst].min_clearance) worst = s;
    }
    std::printf("scorecard: %d of %d scenes touched an obstacle (%d collision ticks of %d scored per scene)\n", n_hit, n, hit_ticks, score[0].n_ticks);
    std::printf("scorecard: worst clearance %.3f m, scene %d, tick %d, obstacle %d\n", score[(size_t)worst].min_clearance, worst,
                score[(size_t)worst].min_clearance_tick, score[(size_t)worst].min_clearance_obs);
    std::printf("scorecard: mean distance %.2f m (the trace's odometer above: %.2f m)\n", sdist / n, dist / n);
    if (fleet) {
        // Ego-ego contact: a nearest obstacle at or beyond the scene's own entries is a peer slot.  The scorecard keeps ONE nearest
        // obstacle per scene (where its smallest clearance occurred), so the ticks counted are those of the scenes whose closest
        // call was with another ego.  pp_gen_scenes places its scenes as unrelated synthetic roads in one coordinate frame: the
        // numbers show the mechanism, they are not traffic.
        int near_peer = 0, hit_scenes = 0, hit_ticks_peer = 0;
        for (int s = 0; s < n; s++) {
            const RolloutScore& r = score[(size_t)s];
            if (r.min_clearance_obs < n_obs) continue;
            near_peer++;
            if (r.n_collision_ticks > 0) { hit_scenes++; hit_ticks_peer += r.n_collision_ticks; }
        }
        std::printf("fleet: one world of %d egos, %d peer slots each, range %.0f m: closest call with another ego in %d scenes; ego-ego collision ticks: %d in %d scenes\n",
                    n, fm.max_peers, fm.range, near_peer, hit_ticks_peer, hit_scenes);
    }
    pp_host_free(trace);
    pp_destroy(h);
    std::printf("example_rollout ok\n");
    return 0;
}
