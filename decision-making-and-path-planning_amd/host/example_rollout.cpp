// example_rollout.cpp — closed-loop evaluation through the C-ABI: 256 generated scenes, every ego follows what the planner
// tells it for 50 ticks (pp_rollout: advance + tick on the device, no host wait, no per-tick PCIe traffic), then the host looks
// at where they ended up: how many scenes carry which rollout flag and how far the egos travelled.  The rollout is scored on the
// device (pp_score_begin: one RolloutScore record per scene, nothing fetched per tick): collisions, worst clearance, distance.
// With --fleet the egos share one world (pp_set_fleet): every scene keeps 8 free pool entries behind its own
// obstacles, the nearest egos are written there after every advance, and the scorecard tells ego-ego contact from the rest.
// With --route the egos drive a ring of four roads on the map store (pp_set_map + pp_set_egos) along a route each (pp_set_route,
// DESIGN.md §4f): the advance step takes them road -> pre-junction -> junction -> next road, and the host prints the legs completed.
// With --follow the grid follows the ego (pp_set_grid_follow): the advance step re-centres grid_origin and goal.
// Combined with --route the ring is driven with the grid stage ON, on a grid of 64 m, and the host prints how many egos carry
// OFF_GRID at the end (without --follow a routed run keeps the grid stage off: every ego would leave its grid on its first road).
// With --track [BIAS] the egos do not sit on their planned paths: every ego keeps a pose of its own and steers a bicycle model along
// the plan (pp_set_ego_tracker with the default model and curv_bias BIAS); the host prints how hard the egos steered
// and how often the planner replanned.  It works with --route and every other flag.
// With --route --traffic every ring ego has a slower vehicle 20 m ahead of it (pp_set_traffic): a scripted actor at
// 1.5 m/s on the closed track of the ego's lane, written into the ego's one obstacle entry on every staged input set; the run is
// scored, and the host prints how many egos saw their vehicle, the worst clearance and the distance travelled.
// With --route --traffic --react the vehicle starts 15 m BEHIND its ego at a desired 8 m/s instead and the car-following law is on
// (pp_set_traffic_follow with the default model): it closes up, finds the ego as its leader and keeps a gap; the host
// prints the smallest ego-actor clearance of the run and the vehicles' mean speed at the end.
// With --route --traffic [--react] --cut-in every vehicle starts 9 m ahead on the NEIGHBOURING lane and carries one manoeuvre (pp_set_traffic_manoeuvres,
// DESIGN.md §4v): when its ego is within 12 m behind it, it changes onto the ego's lane in 20 advances - the planner sees it arrive and brakes.
// With --route --fleet --traffic --shared (and --react for following) the 64 egos form 8 worlds of 8 - each world a platoon on one lane,
// 12 m apart, 4 peer slots per scene - and there is ONE vehicle per world in the place of one per scene (pp_set_world_traffic,
// DESIGN.md §4j): it is written into slot 0 of all 8 member scenes and follows the nearest of the world's 8 egos.
// With --route --episodes every ego gets a route of ONE leg and episodes are on (pp_set_episodes with the default model):
// an ego that arrives restarts on the device from its start records, and the host prints episodes, causes and mean age per ego.
// With --route --episodes --starts M --contact the spawn model is on as well (pp_set_episode_spawn): every ego has M start
// records - record k is 5 k lane points behind its first one -, --contact puts a vehicle 20 m ahead of every ego that drives TOWARDS it at
// 3 m/s and lets contact end an episode, and a restart skips the start records the vehicle stands on (the default clearance, 2 m); the
// host prints episodes, contacts, blocked restarts and the use of each start record.
// With --route --episodes --traffic --reset-traffic (or --contact for the traffic) the vehicle of a restarted ego goes back to a start state
// (pp_set_episode_traffic): with --contact the run of §4l loses its episodes of age 1 - no ego restarts into the vehicle
// that drove on over its start pose -, and with --starts M every start record has its own set: the vehicle at its offset from THAT record.
// The host prints the resets and the shortest episode.
// With --route --episodes --log N the episode log is on (pp_set_episode_log): a ring of N records on the device, one
// record appended per ended episode, drained once behind the run; the scorecard is on, so every record carries its episode's own.
// The host prints an outcome table per start record: episodes, causes, mean age and metres, worst clearance, episodes with a collision.
// With --route --fleet --traffic --shared [--react] --episodes [--starts M] --contact --worlds [--reset-traffic] the WORLD is the unit of an episode
// (pp_set_episode_worlds): whenever one ego of a world ends its episode, all 8 egos of the world restart on that advance on one
// start record index; --reset-traffic puts the world's vehicle back as well (pp_set_episode_world_traffic, §4t), so every world episode
// repeats.  The routes of this example have one leg: the front ego of a platoon arrives (LANE_END | ROUTE_END) after 7 - 10 advances, before it
// reaches the oncoming vehicle 20 m ahead, so the episodes the run prints end on arrival, not on contact - contact ends a world in the closed
// loop of tests/test_episode_world_loop.py.
// With --route --episodes --starts M --schedule [pooled|scene] a scenario schedule is on (pp_set_episode_schedule with the default model in
// that scope): the start record of a restart is drawn by weights from the outcome counts per record that the device keeps -
// with --contact the records whose episodes meet the vehicle about half the time get the most restarts.  The host prints the rows - counted
// episodes, failures and the weight of the next draw per record - beside the restarts per record of the spawn statistics.
// With --score-trace DEPTH[,POST] the score trace is on (pp_set_score_trace with the default model): every scene keeps its
// last DEPTH scored ticks in a ring on the device, which freezes POST ticks behind the scene's first contact; behind the run the host
// prints every frozen scene's triggering tick and, for the first three, the records before it.  Any mode; a routed run gets the scorecard.
// With --conflict [WARN[,CRIT]] the conflict score is on (pp_set_conflict_score with the default model, ttc_warn / ttc_crit replaced; DESIGN.md
// §4u): the device differences the obstacle snapshots of consecutive scored ticks and keeps every scene's smallest time to collision and largest
// braking demand; behind the run the host prints min_ttc, n_crit_ticks and max_drac per scene, and the worst scene.  Any mode; a routed run gets
// the scorecard.
// With --perception [RANGE[,CONFIRM]] the planner reads what a sensor would report (pp_set_perception with the default model, range / confirm
// replaced) while the scorecard and the conflict score keep the truth; behind the run the host prints the entry-ticks by cause
// and by output and the closest thing no planner saw, beside the scorecard.  Any mode.
// Exit code 0 = ran on the GPU.
#include "../../include/dmpp_planner.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(expr) do { int rc__ = (expr); if (rc__) { std::fprintf(stderr, "%s: %s\n", #expr, pp_last_error()); return 2; } } while (0)

// --conflict [WARN[,CRIT]]: the conflict score on with the default model, its two thresholds replaced (0: the default)
struct ConflictArg { bool on = false; double warn = 0, crit = 0; };
static int set_conflict(pp_handle h, const ConflictArg& a)
{
    ConflictModel cm; pp_default_conflict(&cm);
    if (a.warn > 0) { cm.ttc_warn = a.warn; if (cm.ttc_crit > a.warn) cm.ttc_crit = a.warn; }
    if (a.crit > 0) cm.ttc_crit = a.crit;
    CHECK(pp_set_conflict_score(h, &cm));
    return 0;
}

// --perception [RANGE[,CONFIRM]]: the perception model on with the default model, range (m, 0: the default) and confirm (-1: the default) replaced
struct PerceptArg { bool on = false; double range = 0; int confirm = -1; };
static PerceptArg g_percept;
static int set_percept(pp_handle h)
{
    if (!g_percept.on) return 0;
    PerceptionModel pm; pp_default_perception(&pm);
    if (g_percept.range > 0) pm.range = g_percept.range;
    if (g_percept.confirm >= 0) pm.confirm = g_percept.confirm;
    CHECK(pp_set_perception(h, &pm));
    return 0;
}
// ... and behind the run: the totals over the scenes, and the scene with the closest hidden entry
static int print_percept(pp_handle h, int n)
{
    if (!g_percept.on) return 0;
    std::vector<PerceptionStats> ps((size_t)n);
    CHECK(pp_get_perception_stats(h, ps.data(), n));
    PerceptionStats t = {}; int worst = -1;
    for (int s = 0; s < n; s++) {
        const PerceptionStats& p = ps[(size_t)s];
        t.n_entries += p.n_entries; t.n_out += p.n_out; t.n_occluded += p.n_occluded; t.n_missed += p.n_missed; t.n_detected += p.n_detected;
        t.n_fresh += p.n_fresh; t.n_coasted += p.n_coasted; t.n_hidden += p.n_hidden;
        if (p.min_hidden_obs >= 0 && (worst < 0 || p.min_hidden_clearance < ps[(size_t)worst].min_hidden_clearance)) worst = s;
    }
    std::printf("perception: %lld entry-ticks over %lld ticks: %lld out of view, %lld occluded, %lld missed, %lld detected; %lld fresh, %lld coasted, %lld hidden\n",
                (long long)t.n_entries, (long long)ps[0].n_ticks, (long long)t.n_out, (long long)t.n_occluded, (long long)t.n_missed, (long long)t.n_detected,
                (long long)t.n_fresh, (long long)t.n_coasted, (long long)t.n_hidden);
    if (worst < 0) { std::printf("perception: no entry was ever hidden\n"); return 0; }
    const PerceptionStats& w = ps[(size_t)worst];
    std::printf("perception: the closest thing no planner saw: scene %d, entry %d (type %d) at %.3f m clearance on tick %lld\n", worst, w.min_hidden_obs, w.min_hidden_type,
                w.min_hidden_clearance, (long long)w.min_hidden_tick);
    return 0;
}

// ... and behind the run: every scene's record in short, and the worst scene
static int print_conflict(pp_handle h, int n)
{
    std::vector<ConflictScore> cs((size_t)n);
    CHECK(pp_get_conflict_score(h, cs.data(), n));
    int worst = -1;
    for (int s = 0; s < n; s++) {
        const ConflictScore& c = cs[(size_t)s];
        std::printf("conflict: scene %d  min_ttc %.3f s  n_crit_ticks %d  max_drac %.3f m/s^2  (%d of %d ticks with a conflict, %d without history)\n", s, c.min_ttc,
                    c.n_crit_ticks, c.max_drac, c.n_conflict_ticks, c.n_ticks, c.n_no_history_ticks);
        if (c.min_ttc_tick >= 0 && (worst < 0 || c.min_ttc < cs[(size_t)worst].min_ttc)) worst = s;
    }
    if (worst < 0) { std::printf("conflict: no scene had a conflict\n"); return 0; }
    const ConflictScore& c = cs[(size_t)worst];
    std::printf("conflict: worst scene %d: min_ttc %.3f s on scored tick %d against entry %d (type %d), first critical tick %d, time-integrated TTC %.3f s^2, max_drac %.3f m/s^2 on tick %d\n",
                worst, c.min_ttc, c.min_ttc_tick, c.min_ttc_obs, c.min_ttc_type, c.first_crit_tick, c.tit_warn, c.max_drac, c.max_drac_tick);
    return 0;
}

// --score-trace DEPTH[,POST]: the recorder on with the default model (a ring freezes POST ticks behind its first contact)
static int set_score_trace(pp_handle h, int depth, int post)
{
    ScoreTraceModel tm; pp_default_score_trace(&tm);
    tm.depth = depth; tm.post = post >= 0 ? post : (tm.post < depth ? tm.post : depth - 1);
    CHECK(pp_set_score_trace(h, &tm));
    return 0;
}

// ... and behind the run: every frozen scene's triggering tick, and - for the first three - the records before it
static int print_score_trace(pp_handle h, int n, int depth)
{
    std::vector<ScoreTraceInfo> info((size_t)n); std::vector<ScoreTick> ring((size_t)depth);
    CHECK(pp_get_score_trace_info(h, info.data(), n));
    int frozen = 0, shown = 0;
    for (int s = 0; s < n; s++) frozen += info[(size_t)s].state == 2;
    std::printf("score trace: %d of %d rings frozen (depth %d)\n", frozen, n, depth);
    for (int s = 0; s < n; s++) {
        if (info[(size_t)s].state != 2) continue;
        ScoreTraceInfo hd;
        const int got = pp_read_score_trace(h, s, ring.data(), depth, &hd, 0);
        if (got < 0) { std::fprintf(stderr, "pp_read_score_trace: %s\n", pp_last_error()); return 2; }
        for (int i = 0; i < got; i++) {
            const ScoreTick& r = ring[(size_t)i];
            if (r.k != hd.trigger_k) continue;
            std::printf("score trace:   scene %d froze on scored tick %d (tick id %lld, cause %d): clearance %.3f m to obstacle %d (type %d) at %.1f km/h, %d records in the ring\n",
                        s, r.k, (long long)r.tick, hd.trigger, r.clearance, r.obs, r.ob_type, r.v, got);
        }
        if (shown++ >= 3) continue;
        for (int i = 0; i < got && ring[(size_t)i].k <= hd.trigger_k; i++) {
            const ScoreTick& r = ring[(size_t)i];
            std::printf("score trace:     k %d  (%.2f, %.2f)  %.1f km/h  clearance %.3f m  behavior %d  marks %d%s\n", r.k, r.x, r.y, r.v, r.clearance, r.behavior,
                        r.marks & 255, (r.marks & DMPP_TICK_START) ? "  (start record)" : "");
        }
    }
    return 0;
}

// --track [BIAS]: the ego tracker, set right behind the resident scenes; read back after the rollout
static bool g_track = false; static double g_track_bias = 0;
static int set_tracker(pp_handle h)
{
    if (!g_track) return 0;
    EgoTracker tk; pp_default_ego_tracker(&tk); tk.curv_bias = g_track_bias;
    CHECK(pp_set_ego_tracker(h, &tk));
    return 0;
}
static int print_tracker(pp_handle h, int n)
{
    if (!g_track) return 0;
    std::vector<EgoTrackState> ts((size_t)n);
    CHECK(pp_get_ego_track_state(h, ts.data(), n));
    double max_kappa = 0; long long n_init = 0, n_sat = 0;
    for (const EgoTrackState& t : ts) { max_kappa = std::max(max_kappa, t.max_kappa); n_init += t.n_init; n_sat += t.n_sat; }
    std::printf("track: %d egos steered a bicycle model along their plans (curv_bias %g 1/m): largest |curvature| %.4f 1/m, %lld advances met max_curv, %lld states derived\n",
                n, g_track_bias, max_kappa, n_sat, n_init);
    return 0;
}

// --route: a ring of four left-hand arcs of 70 degrees (two lanes, 260 points, lane 2 at 0.5 m) joined by junction arcs of 20
// degrees (40-point polylines), 64 obstacle-free egos with routes of 3 .. 6 legs, 1200 ticks with the grid stage off - or, with
// follow, on: 256 x 256 cells that follow the ego.
// --cut-in (with --route --traffic [--react]): every vehicle starts 9 m ahead of its ego on the NEIGHBOURING lane's track at the
// planner's cruising speed and carries one manoeuvre: once the ego is within 12 m behind it, onto the ego's lane in 20 advances
static bool g_cut_in = false;

static int run_route(bool follow, bool traffic, bool react, bool shared, bool episodes, int starts, bool contact, bool reset, int log_cap, int trace_depth, int trace_post, int sched, bool worlds, const ConflictArg& conflict)
{
    const bool spawn = starts > 0 || contact; const int M = starts > 0 ? starts : 1;
    if (contact) traffic = true;                      // (the vehicle to touch)
    const int W = 8, K = shared ? 4 : 0, stride = 1 + K;      // --shared: worlds of W scenes, K peer slots behind every scene's one own entry
    const int n = 64, ticks = 1200, P = 260, JP = 40, n_lanes = 2;
    const double kPi = 3.14159265358979323846, step = 0.5, w = 3.75;
    const double kr = (70.0 * kPi / 180.0) / ((P - 1) * step), kj = (20.0 * kPi / 180.0) / ((JP + 1) * step);
    std::vector<GlobalPoint3D> pts; std::vector<GlobalPoint2D> jpts; std::vector<MapLane> lanes; std::vector<MapJunction> junc;
    std::vector<int32_t> first = { 0 };
    auto arc = [](double x0, double y0, double th0, double k, double s, double d, double* x, double* y, double* th) {
        *th = th0 + k * s;
        *x = x0 + (std::sin(*th) - std::sin(th0)) / k - d * std::sin(*th); *y = y0 - (std::cos(*th) - std::cos(th0)) / k + d * std::cos(*th);
    };
    double x0 = 300, y0 = 200, th0 = 0;
    for (int r = 0; r < 4; r++) {
        double ex, ey, eth;
        for (int l = 0; l < n_lanes; l++) {
            lanes.push_back({ (int32_t)pts.size(), P, n_lanes, 0 });
            for (int i = 0; i < P; i++) { GlobalPoint3D q; arc(x0, y0, th0, kr, step * i, w * (1 - l), &q.x, &q.y, &eth); q.dir = std::fmod(eth * 180.0 / kPi, 360.0); pts.push_back(q); }
        }
        first.push_back((int32_t)lanes.size());
        arc(x0, y0, th0, kr, step * (P - 1), 0, &ex, &ey, &eth);
        for (int l = 0; l < n_lanes; l++) {
            junc.push_back({ r + 1, (r + 1) % 4 + 1, l + 1, l + 1, (int32_t)jpts.size(), JP });
            for (int i = 0; i < JP; i++) { GlobalPoint2D q; double t; arc(ex, ey, eth, kj, step * (i + 1), w * (1 - l), &q.x, &q.y, &t); jpts.push_back(q); }
        }
        arc(ex, ey, eth, kj, step * (JP + 1), 0, &x0, &y0, &th0);
    }
    std::vector<uint8_t> attr(pts.size(), 0); std::vector<uint16_t> width(pts.size(), 375);
    MapDesc map{}; map.n_roads = 4; map.n_lanes = (int32_t)lanes.size(); map.n_points = (int32_t)pts.size(); map.n_junctions = (int32_t)junc.size(); map.n_jpoints = (int32_t)jpts.size();
    map.road_first_lane = first.data(); map.lanes = lanes.data(); map.points = pts.data(); map.lanechg_attribute = attr.data(); map.lane_width_cm = width.data();
    map.junctions = junc.data(); map.jpoints = jpts.data();

    PlannerConfig cfg; pp_default_config(&cfg, follow ? 256 : 128, follow ? 256 : 128);
    if (!follow) cfg.grid_stage = 0;                  // (a grid that does not follow the ego bounds the run: DESIGN.md §4c 6., §4g)
    PlannerCaps caps{}; caps.max_scenes = n; caps.max_obs_total = traffic ? n * stride : 1; caps.max_lane_pts_total = (int32_t)pts.size(); caps.max_ref_pts_total = (int32_t)jpts.size();
    std::vector<SceneIn> in(n); std::vector<SceneState> st(n);
    {   // generated records for everything the map does not decide (DecisionOut, state), then the egos onto the ring
        std::vector<GlobalPoint3D> gl((size_t)n * 3 * PP_GEN_LANE_PTS); std::vector<uint8_t> ga(gl.size()); std::vector<GlobalPoint2D> gr((size_t)n * PP_GEN_REF_PTS);
        std::vector<ObPoint> go(1); std::vector<ObMotion> gm(1);
        CHECK(pp_gen_scenes(&cfg, 0, n, 0, 0, in.data(), gl.data(), ga.data(), gr.data(), go.data(), gm.data(), st.data()));
    }
    std::vector<RouteLeg> legs; std::vector<int32_t> route_first = { 0 };
    for (int s = 0; s < n; s++) {
        int road = s % 4 + 1, lane = (s / 4) % n_lanes + 1, id = 100 + (s * 7) % 80; const int n_legs = episodes ? 1 : 3 + s % 4;
        if (shared) { const int w = s / W; road = w % 4 + 1; lane = (w / 4) % n_lanes + 1; id = 60 + 24 * (s % W); }      // a platoon per world: member 0 at the rear
        const GlobalPoint3D& q = pts[(size_t)lanes[(size_t)first[(size_t)road - 1] + lane - 1].point_off + id];
        SceneIn& e = in[(size_t)s];
        e.loc.globalpoint = q; e.loc.velocity = 20; e.loc.pos = 0; e.loc.road_num = road; e.loc.lane_num = lane; e.loc.path_num = 0;
        e.loc.last_roadnum = road; e.loc.next_roadnum = road % 4 + 1; e.loc.last_lanenum = lane; e.loc.next_lanenum = lane;
        for (int k = 0; k < DMPP_LANESUM; k++) { e.loc.id[k] = id; e.out_lane_no[k] = k < n_lanes ? (uint16_t)(k + 1) : 0; }
        e.lanes = LaneView{}; e.ref_off = e.ref_n = e.obs_off = e.obs_n = 0; e.stub_attribute = 1; e.period_last = 100;
        const double half = 0.5 * cfg.grid_w * cfg.cell, th = q.dir * kPi / 180.0;      // the first tick's frame: the ego in the middle, the goal 15 m ahead
        e.grid_origin.x = q.x - half; e.grid_origin.y = q.y - half; e.goal.x = q.x + 15.0 * std::cos(th); e.goal.y = q.y + 15.0 * std::sin(th);
        st[(size_t)s].z_target_lanenum = lane; st[(size_t)s].d_his_target_lanenum = lane;
        for (int k = 0; k < n_legs; k++) { RouteLeg g{}; g.road_num = (road - 1 + k) % 4 + 1; g.stub_attribute = 1; for (int l = 0; l < n_lanes; l++) g.out_lane_no[l] = (uint16_t)(l + 1); legs.push_back(g); }
        route_first.push_back((int32_t)legs.size());
    }
    // --traffic: one closed track per lane number - the lane's points on road 1, its junction polyline, road 2 ... - and one vehicle
    // per ego, 20 m ahead of it along that track, in the ego's single obstacle entry
    std::vector<TrafficTrack> tracks; std::vector<GlobalPoint2D> tpts; std::vector<TrafficActor> actors; std::vector<ObPoint> obs((size_t)n * stride, ObPoint{ -500, -500, 0, 0.5f });
    const int per_road = P + JP;
    auto arc_of = [&](int lane, int road, int id) {      // arc length of lane point `id` of `road` along the closed track of `lane`
        const GlobalPoint2D* T = tpts.data() + tracks[(size_t)lane - 1].point_off;
        double here = 0;
        for (int i = 0, at = per_road * (road - 1) + id; i < at; i++) here += std::sqrt((T[i + 1].x - T[i].x) * (T[i + 1].x - T[i].x) + (T[i + 1].y - T[i].y) * (T[i + 1].y - T[i].y));
        return here;
    };
    const double ahead = react ? -15.0 : 20.0;           // where a vehicle starts along its track, seen from its ego
    if (traffic) {
        for (int l = 0; l < n_lanes; l++) {
            tracks.push_back({ (int32_t)tpts.size(), 4 * per_road, 1, 0 });
            for (int r = 0; r < 4; r++) {
                const MapLane& L = lanes[(size_t)first[(size_t)r] + l];
                for (int i = 0; i < P; i++) tpts.push_back({ pts[(size_t)L.point_off + i].x, pts[(size_t)L.point_off + i].y });
                const MapJunction& J = junc[(size_t)r * n_lanes + l];
                for (int i = 0; i < JP; i++) tpts.push_back(jpts[(size_t)J.point_off + i]);
            }
        }
        for (int s = 0; s < n; s++) {
            SceneIn& e = in[(size_t)s];
            const int lane = e.loc.lane_num;
            const double here = arc_of(lane, e.loc.road_num, e.loc.id[lane - 1]);      // arc length of the ego's lane point along its track
            e.obs_off = s * stride; e.obs_n = 1;
            obs[(size_t)s * stride] = ObPoint{ 0, 0, 0, 0.9f };    // (placed by pp_set_traffic / pp_set_world_traffic)
            if (shared) {                                 // one vehicle per world: behind its rear ego (member 0), or ahead of its front ego (member W - 1)
                if (contact) { if (s % W == W - 1) actors.push_back(TrafficActor{ here + 20.0, -3.0, s / W, 0, lane - 1, 1, 0.9f, 0 }); continue; }      // --worlds: oncoming, ahead of the front ego
                if (react && s % W == 0) actors.push_back(TrafficActor{ here - 15.0, 8.0, s / W, 0, lane - 1, 1, 0.9f, 0 });
                if (!react && s % W == W - 1) actors.push_back(TrafficActor{ here + 20.0, 1.5, s / W, 0, lane - 1, 1, 0.9f, 0 });
                continue;
            }
            if (g_cut_in) {
                const int other = lane == 1 ? 2 : 1;
                actors.push_back(TrafficActor{ arc_of(other, e.loc.road_num, e.loc.id[lane - 1]) + 9.0, 10.0 / 3.6, s, 0, other - 1, 1, 0.9f, 0 });
            }
            else if (react) actors.push_back(TrafficActor{ here - 15.0, 8.0, s, 0, lane - 1, 1, 0.9f, 0 });      // (a closed track: a negative s0 wraps)
            else actors.push_back(TrafficActor{ here + 20.0, contact ? -3.0 : 1.5, s, 0, lane - 1, 1, 0.9f, 0 });
        }
    }
    pp_handle h = nullptr;
    CHECK(pp_create(&cfg, 0, &caps, &h));
    CHECK(pp_set_map(h, &map));
    CHECK(pp_set_egos(h, n, in.data(), traffic ? obs.data() : nullptr, nullptr, traffic ? n * stride : 0));
    CHECK(pp_set_state(h, st.data(), n));
    RouteModel rm; CHECK(pp_default_route_model(&rm));
    CHECK(pp_set_route(h, (int)legs.size(), legs.data(), route_first.data(), &rm));
    if (follow) { GridFollow gf; pp_default_grid_follow(&gf); CHECK(pp_set_grid_follow(h, &gf)); }
    if (set_tracker(h)) return 2;
    EgoModel model; pp_default_ego_model(&model);
    if (traffic) {
        if (shared) {
            std::vector<int32_t> world_first; for (int s = 0; s <= n; s += W) world_first.push_back(s);
            FleetModel fm; pp_default_fleet_model(&fm); fm.max_peers = K;
            CHECK(pp_set_fleet(h, n / W, world_first.data(), &fm));
            CHECK(pp_set_world_traffic(h, (int)tracks.size(), tracks.data(), tpts.data(), (int)tpts.size(), (int)actors.size(), actors.data()));
        } else
        CHECK(pp_set_traffic(h, (int)tracks.size(), tracks.data(), tpts.data(), (int)tpts.size(), n, actors.data()));
        if (react) { TrafficFollow tf; pp_default_traffic_follow(&tf); CHECK(pp_set_traffic_follow(h, &tf)); }
        if (g_cut_in) {                                   // one record per vehicle: EGO_DIST, the ego behind it (side 1), onto the ego's lane, no offset at the end
            std::vector<TrafficManoeuvre> mv;
            for (int s = 0; s < n; s++) mv.push_back(TrafficManoeuvre{ 12.0, 0.0, 0.0, NAN, s, DMPP_TRIG_EGO_DIST | 1 << 8, 0, in[(size_t)s].loc.lane_num - 1, 20, 0 });
            if (pp_check_traffic_manoeuvres(n, (int)tracks.size(), n, mv.data()) != -1) { std::fprintf(stderr, "the cut-in list is not legal\n"); return 2; }
            CHECK(pp_set_traffic_manoeuvres(h, n, mv.data()));
        }
        CHECK(pp_score_begin(h, model.dt));
    }
    if ((log_cap || trace_depth || conflict.on) && !traffic) CHECK(pp_score_begin(h, model.dt));      // (the records carry their episode's scorecard; the trace and the conflict score see scored ticks)
    if (episodes) { EpisodeModel em; pp_default_episode_model(&em); CHECK(pp_set_episodes(h, &em)); }      // last: it captures what the calls above set up
    if (spawn) {                                      // M start records per ego: record k stands 5 k lane points behind record 0, on the same lane
        EpisodeSpawn sp; pp_default_episode_spawn(&sp); sp.n_starts = M; sp.contact = contact ? 1 : 0;
        std::vector<SceneIn> in_k; std::vector<SceneState> st_k;
        for (int k = 1; k < M; k++) for (int s = 0; s < n; s++) {
            SceneIn e = in[(size_t)s]; const int id = e.loc.id[0] > 5 * k ? e.loc.id[0] - 5 * k : 0;      // (the egos start at point 100 or later: never clamped here)
            const GlobalPoint3D& q = pts[(size_t)lanes[(size_t)first[(size_t)e.loc.road_num - 1] + e.loc.lane_num - 1].point_off + id];
            e.loc.globalpoint = q; for (int l = 0; l < DMPP_LANESUM; l++) e.loc.id[l] = id;
            in_k.push_back(e); st_k.push_back(st[(size_t)s]);
        }
        CHECK(pp_set_episode_spawn(h, &sp, M > 1 ? in_k.data() : nullptr, M > 1 ? st_k.data() : nullptr));
    }
    if (worlds) CHECK(pp_set_episode_worlds(h, 1));   // (part of the spawn model in force: behind pp_set_episode_spawn; the worlds are those of the fleet)
    if (reset && shared) {                            // the world reset of §4t: set k puts a world's vehicle at its offset from start record k of the world's front ego
        std::vector<TrafficStart> sets;
        for (int k = 1; k < M; k++) for (int a = 0; a < n / W; a++) {
            const SceneIn& e = in[(size_t)a * W + W - 1]; const int lane = e.loc.lane_num, id = e.loc.id[0] > 5 * k ? e.loc.id[0] - 5 * k : 0;
            sets.push_back(TrafficStart{ arc_of(lane, e.loc.road_num, id) + 20.0, 0.0 });
        }
        CHECK(pp_set_episode_world_traffic(h, M, M > 1 ? sets.data() : nullptr));
    } else
    if (reset) {                                      // last of all: set 0 is captured here; set k puts the vehicle at its offset from start record k (5 k points back)
        std::vector<TrafficStart> sets;
        for (int k = 1; k < M; k++) for (int s = 0; s < n; s++) {
            const SceneIn& e = in[(size_t)s]; const int lane = e.loc.lane_num, id = e.loc.id[0] > 5 * k ? e.loc.id[0] - 5 * k : 0;
            sets.push_back(TrafficStart{ arc_of(lane, e.loc.road_num, id) + ahead, actors[(size_t)s].speed > 0 ? actors[(size_t)s].speed : 0.0 });
        }
        CHECK(pp_set_episode_traffic(h, M, M > 1 ? sets.data() : nullptr));
    }
    if (log_cap) CHECK(pp_set_episode_log(h, log_cap));      // last of all
    EpisodeSchedule sm; pp_default_episode_schedule(&sm); sm.scope = sched == 2 ? 0 : 1;
    if (sched) CHECK(pp_set_episode_schedule(h, &sm));       // (part of the spawn model in force: it retires nothing, anywhere behind pp_set_episode_spawn)
    if (trace_depth && set_score_trace(h, trace_depth, trace_post)) return 2;      // (no feature: anywhere)
    if (conflict.on && set_conflict(h, conflict)) return 2;                        // (likewise)
    if (set_percept(h)) return 2;                                                  // (likewise: the model belongs to the handle)
    long long last = 0;
    CHECK(pp_rollout(h, ticks, &model, nullptr, &last));
    CHECK(pp_sync(h));
    if (trace_depth && print_score_trace(h, n, trace_depth)) return 2;
    if (conflict.on && print_conflict(h, n)) return 2;
    if (print_percept(h, n)) return 2;
    if (log_cap) {
        std::vector<EpisodeRecord> rec((size_t)log_cap);
        long long lost = 0, total = 0;
        const int got = pp_read_episode_log(h, rec.data(), log_cap, &lost);
        if (got < 0) { std::fprintf(stderr, "pp_read_episode_log: %s\n", pp_last_error()); return 2; }
        CHECK(pp_get_episode_log_info(h, &total, nullptr));
        std::printf("log: %lld records appended to a ring of %d, %d read, %lld overwritten unread; per start record:\n", total, log_cap, got, lost);
        static const char* const bit[8] = { "PATH_END", "BAD_PATH", "LANE_END", "OFF_GRID", "ROUTE_END", "-", "TIMEOUT", "CONTACT" };
        for (int k = 0; k < M; k++) {
            long long eps = 0, by[8] = {}, age = 0, hit = 0; double metres = 0, worst = INFINITY;
            for (int i = 0; i < got; i++) {
                const EpisodeRecord& r = rec[(size_t)i];
                if (r.start != k) continue;
                eps++; age += r.age; metres += r.dist; hit += r.score.n_collision_ticks > 0;
                if (r.score.min_clearance < worst) worst = r.score.min_clearance;
                for (int b = 0; b < 8; b++) by[b] += (r.cause >> b) & 1;
            }
            std::printf("log:   start %d: %lld episodes", k, eps);
            if (eps) {
                std::printf(", mean age %.1f advances, mean %.1f m, worst clearance %.2f m, %lld with a collision; causes:", (double)age / eps, metres / eps, worst, hit);
                for (int b = 0; b < 8; b++) if (by[b]) std::printf(" %s %lld", bit[b], by[b]);
            }
            std::printf("\n");
        }
    }
    if (episodes) {
        static const char* const cause[6] = { "PATH_END", "BAD_PATH", "LANE_END", "OFF_GRID", "ROUTE_END", "TIMEOUT" };
        std::vector<EpisodeStats> es(n);
        CHECK(pp_get_episode_stats(h, es.data(), n));
        long long total = 0, by[6] = { 0, 0, 0, 0, 0, 0 }; double metres = 0;
        std::printf("episodes: ended per ego (mean age in advances):");
        for (int s = 0; s < n; s++) {
            const EpisodeStats& e = es[(size_t)s];
            std::printf(" %d (%.1f)", e.n_episodes, e.n_episodes ? (double)e.ticks_total / e.n_episodes : 0.0);
            total += e.n_episodes; metres += e.dist_total;
            for (int b = 0; b < 6; b++) by[b] += e.n_end[b];
        }
        std::printf("\nepisodes: %lld ended in %d advances of %d egos, %.1f m driven in them; causes:", total, ticks, n, metres);
        for (int b = 0; b < 6; b++) if (by[b]) std::printf(" %s %lld", cause[b], by[b]);
        std::printf("\n");
    }
    if (spawn) {
        std::vector<EpisodeSpawnStats> ss(n);
        CHECK(pp_get_episode_spawn_stats(h, ss.data(), n));
        long long nc = 0, nb = 0, nr = 0, used[DMPP_EPISODE_MAX_STARTS] = {};
        for (int s = 0; s < n; s++) {
            nc += ss[(size_t)s].n_contact; nb += ss[(size_t)s].n_blocked; nr += ss[(size_t)s].n_rejected;
            for (int k = 0; k < M; k++) used[k] += ss[(size_t)s].n_used[k];
        }
        std::printf("spawn: %d start records per ego, contact %s: %lld episodes ended on contact, %lld restarts found no clear record, %lld records rejected; restarts per record:",
                    M, contact ? "ends an episode" : "off", nc, nb, nr);
        for (int k = 0; k < M; k++) std::printf(" %lld", used[k]);
        std::printf("\n");
    }
    if (sched) {                                      // the rows (per-scene scope: summed over the scenes for the print) and the weights of the next draw
        std::vector<EpisodeScheduleRow> rows(sm.scope == 1 ? 1 : (size_t)n);
        CHECK(pp_get_episode_schedule(h, rows.data(), (int)rows.size()));
        EpisodeScheduleRow sum = {};
        for (const EpisodeScheduleRow& r : rows) for (int k = 0; k < M; k++) { sum.n_end[k] += r.n_end[k]; sum.n_fail[k] += r.n_fail[k]; }
        int32_t wt[DMPP_EPISODE_MAX_STARTS];
        CHECK(pp_episode_schedule_weights(&sm, &rows[0], M, wt));
        std::printf("schedule (%s): counted episodes / failures per record%s:", sm.scope == 1 ? "pooled" : "per scene", sm.scope == 1 ? "" : ", all scenes");
        for (int k = 0; k < M; k++) std::printf(" %d/%d", sum.n_end[k], sum.n_fail[k]);
        std::printf("; weights of the next draw%s:", sm.scope == 1 ? "" : " of scene 0");
        for (int k = 0; k < M; k++) std::printf(" %d", wt[k]);
        std::printf("\n");
    }
    if (worlds) {
        std::vector<EpisodeStats> es(n);
        CHECK(pp_get_episode_stats(h, es.data(), n));
        int with_world = 0, together = 0;
        for (int s = 0; s < n; s++) with_world += (es[(size_t)s].last_cause & DMPP_EGO_WORLD) != 0;
        for (int a = 0; a < n / W; a++) { bool same = true; for (int j = 1; j < W; j++) same = same && es[(size_t)a * W + j].n_episodes == es[(size_t)a * W].n_episodes; together += same; }
        std::printf("worlds: the world is the unit of an episode: %d of %d worlds have the same episode count in every member, %d egos last ended because a partner did (DMPP_EGO_WORLD)\n",
                    together, n / W, with_world);
    }
    if (reset && shared) {
        const int nv = (int)actors.size();
        std::vector<int32_t> nr((size_t)nv);
        CHECK(pp_get_episode_world_traffic_resets(h, nr.data(), nv));
        long long resets = 0; for (int a = 0; a < nv; a++) resets += nr[(size_t)a];
        std::printf("reset-traffic: %d set(s) of start states per world vehicle, %lld vehicle resets\n", M, resets);
    } else
    if (reset) {
        std::vector<int32_t> nr(n); std::vector<EpisodeStats> es(n);
        CHECK(pp_get_episode_traffic_resets(h, nr.data(), n));
        CHECK(pp_get_episode_stats(h, es.data(), n));
        long long resets = 0; int shortest = -1;
        for (int s = 0; s < n; s++) {
            resets += nr[(size_t)s];
            if (es[(size_t)s].min_age >= 0 && (shortest < 0 || es[(size_t)s].min_age < shortest)) shortest = es[(size_t)s].min_age;
        }
        std::printf("reset-traffic: %d set(s) of start states per vehicle, %lld vehicle resets; the shortest episode of the run took %d advances\n", M, resets, shortest);
    }
    if (traffic) {
        const int nv = (int)actors.size();
        std::vector<RolloutScore> score(n); std::vector<double> arc((size_t)nv);
        CHECK(pp_get_rollout_score(h, score.data(), n));
        CHECK(pp_get_traffic_state(h, arc.data(), nv));
        if (shared) std::printf("shared: %d worlds of %d egos, one vehicle per world in slot 0 of every member scene (%d records in the place of %d)\n", n / W, W, nv, n);
        int saw = 0, hit = 0; double worst = INFINITY, dist = 0, driven = 0;
        for (int s = 0; s < n; s++) {
            const RolloutScore& r = score[(size_t)s];
            saw += r.n_ob_flag > 0; hit += r.n_collision_ticks > 0; dist += r.dist; if (r.min_clearance < worst) worst = r.min_clearance;
        }
        for (int a = 0; a < nv; a++) driven += arc[(size_t)a];
        if (g_cut_in) {
            std::vector<TrafficManoeuvreState> ms((size_t)nv); int done = 0, home = 0;
            CHECK(pp_get_traffic_manoeuvre_state(h, ms.data(), nv));
            for (int a = 0; a < nv; a++) { done += ms[(size_t)a].n_done; home += ms[(size_t)a].track == in[(size_t)a].loc.lane_num - 1 && ms[(size_t)a].lat == 0; }
            std::printf("cut-in: %d vehicles 9 m ahead on the neighbouring lane at %.2f m/s%s: %d moves finished, %d vehicles on their ego's lane with no offset; %d of %d egos saw "
                        "theirs (ob_flag), %d touched it, worst clearance %.2f m, mean distance travelled %.1f m\n", nv, actors[0].speed, react ? ", following on" : "", done, home, saw, n, hit, worst, dist / n);
        } else if (react) {
            std::vector<double> v((size_t)nv); double vsum = 0;
            CHECK(pp_get_traffic_speed(h, v.data(), nv));
            for (int a = 0; a < nv; a++) vsum += v[(size_t)a];
            std::printf("react: %d vehicles that want %.1f m/s, 15 m behind their egos, following on: %d egos were touched, smallest ego-actor clearance of the run %.2f m, "
                        "mean distance travelled by the egos %.1f m, mean vehicle speed now %.2f m/s\n", nv, actors[0].speed, hit, worst, dist / n, vsum / nv);
        } else
        std::printf("traffic: %d vehicles at %.1f m/s, 20 m ahead of their egos: %d of %d egos saw theirs (ob_flag), %d touched it, worst clearance %.2f m, "
                    "mean distance travelled %.1f m (a vehicle covers %.1f m; mean arc length now %.1f m)\n",
                    nv, actors[0].speed, saw, n, hit, worst, dist / n, actors[0].speed * model.dt * ticks, driven / nv);
    }
    std::vector<int32_t> flags(n); std::vector<SceneIn> end(n);
    CHECK(pp_get_ego_flags(h, flags.data(), n));
    CHECK(pp_get_scene_in(h, end.data(), n));
    int arrived = 0, missed = 0, other = 0, legs_done = 0, off_grid = 0;
    std::printf("route: legs completed per ego (of its route):");
    for (int s = 0; s < n; s++) {
        const int f = flags[(size_t)s], total = route_first[(size_t)s + 1] - route_first[(size_t)s];
        const int done = end[(size_t)s].loc.path_num + ((f & DMPP_EGO_ROUTE_END) ? 1 : 0);
        std::printf(" %d/%d", done, total);
        legs_done += done; arrived += (f & DMPP_EGO_ROUTE_END) != 0; missed += f == DMPP_EGO_LANE_END; off_grid += (f & DMPP_EGO_OFF_GRID) != 0; other += (f & ~(DMPP_EGO_LANE_END | DMPP_EGO_ROUTE_END)) != 0;
    }
    std::printf("\nroute: %d egos on a ring of 4 roads for %d ticks (last tick id %lld): %d legs completed, %d arrived (ROUTE_END), %d missed an exit, %d with another flag\n",
                n, ticks, last, legs_done, arrived, missed, other);
    if (follow) std::printf("follow: the grid stage ran on %d x %d cells that followed the ego: %d of %d egos carry OFF_GRID\n", cfg.grid_w, cfg.grid_h, off_grid, n);
    if (print_tracker(h, n)) return 2;
    pp_destroy(h);
    std::printf("example_rollout ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    bool fleet = false, route = false, follow = false, traffic = false, react = false, shared = false, episodes = false, contact = false, reset = false, worlds = false; int starts = 0, log_cap = 0, trace_depth = 0, trace_post = -1, sched = 0;
    ConflictArg conflict;
    for (int a = 1; a < argc; a++) {
        if (std::strcmp(argv[a], "--fleet") == 0) fleet = true;
        else if (std::strcmp(argv[a], "--route") == 0) route = true;
        else if (std::strcmp(argv[a], "--follow") == 0) follow = true;
        else if (std::strcmp(argv[a], "--track") == 0) {
            g_track = true;                               // a number behind it is the steering bias
            char* e = nullptr;
            if (a + 1 < argc) { const double b = std::strtod(argv[a + 1], &e); if (e != argv[a + 1] && *e == 0) { g_track_bias = b; a++; } }
        }
        else if (std::strcmp(argv[a], "--traffic") == 0) traffic = true;
        else if (std::strcmp(argv[a], "--react") == 0) react = true;
        else if (std::strcmp(argv[a], "--cut-in") == 0) g_cut_in = true;
        else if (std::strcmp(argv[a], "--shared") == 0) shared = true;
        else if (std::strcmp(argv[a], "--episodes") == 0) episodes = true;
        else if (std::strcmp(argv[a], "--contact") == 0) contact = true;
        else if (std::strcmp(argv[a], "--reset-traffic") == 0) reset = true;
        else if (std::strcmp(argv[a], "--worlds") == 0) worlds = true;
        else if (std::strcmp(argv[a], "--starts") == 0 && a + 1 < argc) starts = std::atoi(argv[++a]);
        else if (std::strcmp(argv[a], "--schedule") == 0) {
            sched = 1;                                    // pooled unless the next word says otherwise
            if (a + 1 < argc && std::strcmp(argv[a + 1], "scene") == 0) { sched = 2; a++; }
            else if (a + 1 < argc && std::strcmp(argv[a + 1], "pooled") == 0) a++;
        }
        else if (std::strcmp(argv[a], "--log") == 0 && a + 1 < argc) log_cap = std::atoi(argv[++a]);
        else if (std::strcmp(argv[a], "--score-trace") == 0 && a + 1 < argc) { if (std::sscanf(argv[++a], "%d,%d", &trace_depth, &trace_post) < 1) trace_depth = -1; }
        else if (std::strcmp(argv[a], "--conflict") == 0) {
            conflict.on = true;
            if (a + 1 < argc && argv[a + 1][0] != '-' && std::sscanf(argv[++a], "%lf,%lf", &conflict.warn, &conflict.crit) < 1) conflict.warn = -1;
        }
        else if (std::strcmp(argv[a], "--perception") == 0) {
            g_percept.on = true;
            if (a + 1 < argc && argv[a + 1][0] != '-' && std::sscanf(argv[++a], "%lf,%d", &g_percept.range, &g_percept.confirm) < 1) g_percept.range = -1;
        }
        else { std::fprintf(stderr, "usage: example_rollout [--fleet | --route [--episodes [--starts M] [--contact] [--schedule [pooled|scene]] [--reset-traffic] [--log N]] [--traffic [--react] [--cut-in] | --fleet --traffic --shared [--react] [--episodes [--starts M] --contact --worlds [--reset-traffic]]]] [--follow] [--track [BIAS]] [--score-trace DEPTH[,POST]] [--conflict [WARN[,CRIT]]] [--perception [RANGE[,CONFIRM]]]\n"); return 2; }
    }
    if (traffic && !route) { std::fprintf(stderr, "--traffic drives the ring: use it with --route\n"); return 2; }
    if (g_cut_in && !(route && traffic && !shared && !contact)) { std::fprintf(stderr, "--cut-in scripts the per-scene traffic: use it with --route --traffic [--react]\n"); return 2; }
    if (react && !traffic) { std::fprintf(stderr, "--react makes the traffic follow: use it with --traffic\n"); return 2; }
    if (shared && !(route && fleet && traffic)) { std::fprintf(stderr, "--shared puts one vehicle into every world: use it with --route --fleet --traffic\n"); return 2; }
    if (episodes && !route) { std::fprintf(stderr, "--episodes restarts egos that arrive: use it with --route\n"); return 2; }
    if ((starts || contact) && !episodes) { std::fprintf(stderr, "--starts / --contact shape the restarts: use them with --route --episodes\n"); return 2; }
    if (starts < 0 || starts > DMPP_EPISODE_MAX_STARTS) { std::fprintf(stderr, "--starts takes 1 .. %d\n", DMPP_EPISODE_MAX_STARTS); return 2; }
    if (worlds && !(shared && episodes && contact)) { std::fprintf(stderr, "--worlds restarts a world as a whole: use it with --route --fleet --traffic --shared --episodes --contact\n"); return 2; }
    if (worlds && sched) { std::fprintf(stderr, "--worlds draws once per world: not with --schedule\n"); return 2; }
    if (contact && ((react && !worlds) || (shared && !worlds))) { std::fprintf(stderr, "--contact brings its own oncoming vehicle: not with --react / --shared\n"); return 2; }
    if (starts && shared && !worlds) { std::fprintf(stderr, "--starts places its records behind each ego on its lane: not with the platoons of --shared\n"); return 2; }
    if (sched && !(route && episodes && starts > 0)) { std::fprintf(stderr, "--schedule draws among start records: use it with --route --episodes --starts M\n"); return 2; }
    if (reset && !(route && episodes && (traffic || contact))) { std::fprintf(stderr, "--reset-traffic puts a restarted ego's vehicle back: use it with --route --episodes --traffic (or --contact)\n"); return 2; }
    if (reset && shared && !worlds) { std::fprintf(stderr, "--reset-traffic resets per-scene traffic: a vehicle of --shared belongs to a whole world\n"); return 2; }
    if (log_cap && !(route && episodes)) { std::fprintf(stderr, "--log records how episodes ended: use it with --route --episodes\n"); return 2; }
    if (log_cap < 0 || log_cap > DMPP_EPISODE_LOG_MAX) { std::fprintf(stderr, "--log takes 1 .. %d records\n", DMPP_EPISODE_LOG_MAX); return 2; }
    if (trace_depth < 0 || trace_depth > DMPP_SCORE_TRACE_MAX || (trace_depth && trace_post >= trace_depth)) { std::fprintf(stderr, "--score-trace takes DEPTH 1 .. %d and POST 0 .. DEPTH - 1\n", DMPP_SCORE_TRACE_MAX); return 2; }
    if (conflict.on && (conflict.warn < 0 || conflict.crit < 0 || !std::isfinite(conflict.warn) || !std::isfinite(conflict.crit) || (conflict.warn > 0 && conflict.crit > conflict.warn)))
        { std::fprintf(stderr, "--conflict takes WARN > 0 and 0 < CRIT <= WARN, in seconds\n"); return 2; }
    if (g_percept.on && (!(g_percept.range >= 0) || g_percept.confirm > 255))
        { std::fprintf(stderr, "--perception takes RANGE > 0 in metres (0: the default) and CONFIRM 0 .. 255\n"); return 2; }
    if (route) return run_route(follow, traffic, react, shared, episodes, starts, contact, reset, log_cap, trace_depth, trace_post, sched, worlds, conflict);
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
    if (follow) { GridFollow gf; pp_default_grid_follow(&gf); CHECK(pp_set_grid_follow(h, &gf)); }              // OFF_GRID below: the egos the frame could not hold
    if (set_tracker(h)) return 2;

    EgoModel model; pp_default_ego_model(&model);
    EgoTrace* trace = (EgoTrace*)pp_host_alloc(sizeof(EgoTrace) * (size_t)ticks * n);      // pinned: the kernel writes it over PCIe
    if (!trace) { std::fprintf(stderr, "pp_host_alloc: %s\n", pp_last_error()); return 2; }
    long long last = 0;
    CHECK(pp_score_begin(h, model.dt));
    if (trace_depth && set_score_trace(h, trace_depth, trace_post)) return 2;
    if (conflict.on && set_conflict(h, conflict)) return 2;
    if (set_percept(h)) return 2;
    CHECK(pp_rollout(h, ticks, &model, trace, &last));
    CHECK(pp_sync(h));
    if (trace_depth && print_score_trace(h, n, trace_depth)) return 2;
    if (conflict.on && print_conflict(h, n)) return 2;
    if (print_percept(h, n)) return 2;
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
    if (print_tracker(h, n)) return 2;
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
