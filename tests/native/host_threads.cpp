// host_threads.cpp - the class surface used the way the reference uses it: CDecision on one thread, CPlanning on another
// (Decision.cpp:45, Planning.cpp:27 start one thread per module), plus a third thread calling helper methods on the planning
// object.  Built twice by tests/test_host_threads.py: with -fsanitize=thread (host build, no GPU needed: every device call
// fails fast and the host-side state is what the sanitizer watches) and plain (GPU box: the results of the concurrent run
// must equal those of the same calls made one thread at a time).
#include "../../decision-making-and-path-planning_amd/host/dmpp_decision.hpp"
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>

struct Inputs {
    SceneIn in; SceneState st; LaneMap map;
    std::vector<ObPoint> obs;
};

static Inputs make_inputs()
{
    Inputs I;
    PlannerConfig cfg = CShare::Config();
    std::vector<GlobalPoint3D> lanes(3 * PP_GEN_LANE_PTS);
    std::vector<uint8_t> attr(3 * PP_GEN_LANE_PTS);
    std::vector<GlobalPoint2D> ref(PP_GEN_REF_PTS);
    std::vector<ObMotion> mot(64);
    I.obs.resize(64);
    pp_gen_scenes(&cfg, 2, 1, 64, 0, &I.in, lanes.data(), attr.data(), ref.data(), I.obs.data(), mot.data(), &I.st);
    I.map.cur.assign(lanes.begin(), lanes.begin() + PP_GEN_LANE_PTS);
    if (I.in.lanes.left_n) I.map.left.assign(lanes.begin() + PP_GEN_LANE_PTS, lanes.begin() + 2 * PP_GEN_LANE_PTS);
    if (I.in.lanes.right_n) I.map.right.assign(lanes.begin() + 2 * PP_GEN_LANE_PTS, lanes.end());
    I.map.lane_sum = I.in.lanes.lane_sum; I.map.lanechg_attribute = I.in.lanes.lanechg_attribute; I.map.lane_width = I.in.lanes.lane_width;
    I.map.cur_lanechg_attribute.assign(attr.begin(), attr.begin() + PP_GEN_LANE_PTS);
    for (int i = 0; i < DMPP_LANESUM; i++) I.map.out_lane_no[i] = I.in.out_lane_no[i];
    return I;
}

struct Trace { std::vector<DecisionOutPod> dec; std::vector<PlanningOut> res; std::vector<double> helper; int errors = 0; };

static void decision_thread(const Inputs& I, int n, Trace& T)
{
    CDecision& d = CDecision::Instance();
    for (int t = 0; t < n; t++) {
        LocationOut loc = I.in.loc;
        loc.globalpoint.x += 0.01 * t;
        DecisionOut o = d.decide(loc, I.obs);
        if (CShare::LastStatus().code) T.errors++;
        T.dec.push_back(o);
    }
}
static void planning_thread(const Inputs& I, int n, Trace& T)
{
    CPlanning& p = CPlanning::Instance();
    DecisionOut dec; dec.behavior = 1; dec.target_lanenum = I.in.loc.lane_num; dec.velocity_expect = 10;
    PlanningOut result{}; PlanningStatus show{};
    for (int t = 0; t < n; t++) {
        LocationOut loc = I.in.loc;
        loc.globalpoint.y += 0.002 * t;
        p.plan(dec, loc, VehStatus{}, I.obs, result, show);
        if (CShare::LastStatus().code) T.errors++;
        T.res.push_back(result);
    }
}
// CalcDistance, and GetVhclLocalState - a whole tick on a scratch copy of the planning object's state - while plan() runs on the
// other thread: its five outputs depend on its arguments alone, whatever state the copy was taken from.
static void helper_thread(const Inputs& I, int n, Trace& T)
{
    CPlanning& p = CPlanning::Instance();
    GlobalPoint2D path[DMPP_PATH_POINTS];
    for (int i = 0; i < DMPP_PATH_POINTS; i++) path[i] = GlobalPoint2D{I.in.loc.globalpoint.x - 5 + 0.25 * i, I.in.loc.globalpoint.y + 0.01 * i};
    for (int t = 0; t < n; t++) {
        GlobalPoint2D a{0, 0}, b{1.0 + t, 1};
        T.helper.push_back(p.CalcDistance(a, b));
        if (CShare::LastStatus().code) T.errors++;
        LocationOut loc = I.in.loc;
        loc.globalpoint.x += 0.3 * t;
        double lat = 0, dir_err = 0, remain = 0; int near_id = 0, front_id = 0;
        p.GetVhclLocalState(loc, path, lat, dir_err, near_id, front_id, remain);
        if (CShare::LastStatus().code) T.errors++;
        for (double v : {lat, dir_err, (double)near_id, (double)front_id, remain}) T.helper.push_back(v);
    }
}

int main(int argc, char** argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 50;
    PlannerConfig& cfg = CShare::Config();
    cfg.grid_stage = 0;
    Inputs I = make_inputs();
    CDecision::Instance().SetMap(I.map); CPlanning::Instance().SetMap(I.map);
    const bool have_gpu = CDecision::Instance().startCDecisionThread() && CPlanning::Instance().startCPlanningThread();
    // reference: the same calls, one thread at a time
    Trace ref;
    if (have_gpu) {
        decision_thread(I, n, ref); planning_thread(I, n, ref); helper_thread(I, n, ref);
        CDecision::Instance().Reset(); CPlanning::Instance().Reset();
    }
    Trace a, b, c;
    std::thread t1(decision_thread, std::cref(I), n, std::ref(a));
    std::thread t2(planning_thread, std::cref(I), n, std::ref(b));
    std::thread t3(helper_thread, std::cref(I), n, std::ref(c));
    t1.join(); t2.join(); t3.join();
    if (!have_gpu) {
        // no GPU: every call must have failed cleanly (and the sanitizer has watched the host side)
        const bool ok = a.errors == n && b.errors == n && c.errors == 2 * n;      // the helper thread makes two calls per round
        std::printf(ok ? "host_threads ok (no GPU: %d + %d + %d calls refused)\n" : "host_threads FAILED (no GPU) %d %d %d\n", a.errors, b.errors, c.errors);
        return ok ? 0 : 1;
    }
    bool ok = a.errors == 0 && b.errors == 0 && c.errors == 0 && ref.errors == 0;
    ok = ok && a.dec.size() == ref.dec.size() && std::memcmp(a.dec.data(), ref.dec.data(), a.dec.size() * sizeof(DecisionOutPod)) == 0;
    ok = ok && b.res.size() == ref.res.size() && std::memcmp(b.res.data(), ref.res.data(), b.res.size() * sizeof(PlanningOut)) == 0;
    ok = ok && c.helper == ref.helper;
    std::printf(ok ? "host_threads ok (%d concurrent decide / plan / helper calls equal the sequential run)\n" : "host_threads FAILED: concurrent results differ (errors %d %d %d)\n",
                ok ? n : a.errors, b.errors, c.errors);
    return ok ? 0 : 1;
}
