"""Known answers for the functions whose bodies ARE in the reference, with expected values derived by hand from the
cited source lines (the reference ships no tests or vectors, and cannot be built here - these are analytic answers, not
reference outputs: parity stays "unpinned").

Every answer runs on two backends: the CPU oracle, and the HIP library on the device (the `backend` fixture; the answers
that predate it keep their test ids on the oracle and run on the device as *_hip).  The oracle
and the kernels were written from the same reading of Planning.cpp / Decision.cpp, so the device-vs-oracle parity tests
cannot see a misreading they share; these answers can.  Scene-level answers are observed through whole ticks and run
once on one scene and once on a batch of 300 copies of it (tests/kat_backends.py: the device's piped, grouped path).

The scenes are the straight lanes of tests/lanechange_scenes.py: lanes along +x, points 0.5 m apart, lane 1 at y = 200,
lane 2 at 196.25, lane 3 at 192.5, the ego on point 50 (x = 125) unless moved, so arc lengths are exact binary
fractions.  Default config: ROAD_FARAIM_MIN 10 / MAX 40, PRE_INTER_FARAIM 15, INTER_FARAIM 10, Vehicle_Width 1.8
(windows +-0.9), NO_OBSTACLE_DIS 999, ID_MORE 0."""
import math

import numpy as np
import pytest

import kat_backends as kb
import lanechange_scenes as lcs

Y1, Y2, Y3 = 200.0, 196.25, 192.5          # lane centres
COPIES = pytest.mark.parametrize("copies", [1, 300], ids=["x1", "x300"])
MISS = (0, 999.0, 999.0)                    # corridor searched, nothing found: NO_OBSTACLE_DIS in both distances
EMPTY = (0, 0.0, 0.0)                       # corridor without points: never searched, the zeroed record (Decision.cpp:794-806)


@pytest.fixture(scope="module")
def backends(dm, oracle):
    """backends("oracle") / backends("hip"): one of each per module (the device one keeps its handles)."""
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = kb.OracleBackend(oracle) if kind == "oracle" else kb.HipBackend()
        return made[kind]
    return get


@pytest.fixture(scope="module", params=["oracle", pytest.param("hip", marks=pytest.mark.gpu)])
def backend(request, backends):
    return backends(request.param)


@pytest.fixture(scope="module")
def cfg(dm):
    c = dm.default_config(128)
    c["grid_stage"] = 0
    return c


@pytest.fixture(scope="module")
def cfg_off(cfg):
    """Decision stage off: the scene's own DecisionOut (SceneIn.dec) and refpath-pool slice are used as they are."""
    c = cfg.copy()
    c["decision_stage"] = 0
    return c


def lane_x(k):
    return 100.0 + 0.5 * k


def ahead_of(k):
    """metres from the ego (point 50) to lane point k"""
    return (k - lcs.EGO_ID) * 0.5


def own_decision(sc, behavior=1, target=None, refpath_n=0):
    d = sc["scene_in"]["dec"]
    d["behavior"], d["refpath_n"], d["velocity_expect"] = behavior, refpath_n, 10.0
    d["target_lanenum"] = sc["scene_in"]["loc"]["lane_num"][0] if target is None else target


def move_ego(sc, k):
    """the ego on point k of its lane (every lane's id = k)"""
    loc = sc["scene_in"]["loc"]
    loc["id"][:] = k
    loc["globalpoint"]["x"] = lane_x(k)


def mark_aims(st):
    """distinct stale values in both aim points, to see which ones a tick writes"""
    st["aimpoint_far"]["Aim_point"]["x"], st["aimpoint_far"]["Aim_point"]["y"] = 1234.5, -7.25
    st["aimpoint_far"]["Aim_point"]["dir"], st["aimpoint_far"]["Aim_id"] = 33.0, 17
    st["aimpoint_near"]["Aim_point"]["x"], st["aimpoint_near"]["Aim_point"]["y"] = 4321.5, 7.25
    st["aimpoint_near"]["Aim_point"]["dir"], st["aimpoint_near"]["Aim_id"] = 11.0, 71
    return (1234.5, -7.25, 33.0, 17), (4321.5, 7.25, 11.0, 71)


def tick(backend, cfg, sc, copies, st=None, ticks=1):
    st = sc["state"].copy() if st is None else st
    return backend.run(cfg, sc, st, ticks, copies)


def ticks_each(backend, cfg, sc, st, n, copies):
    """Results after each of n ticks from st (st is left at the state after the last).  A batch queues its ticks without a
    host wait, so each prefix is its own queued run from the same start."""
    if copies == 1:
        return [backend.run(cfg, sc, st, 1, 1) for _ in range(n)]
    start, out = st.copy(), []
    for k in range(1, n + 1):
        s = start.copy()
        out.append(backend.run(cfg, sc, s, k, copies))
    st[:] = s
    return out


# ---- scalar functions ----------------------------------------------------------------------------------------------
def kat_GetRoadAngle_quadrants(backend, cfg):       # Planning.cpp:719-750: degrees CCW from east, [0,360)
    A = lambda b: backend.road_angle(cfg, (0.0, 0.0), b)
    assert A((1.0, 0.0)) == 0.0
    assert A((1.0, 1.0)) == pytest.approx(45.0, abs=1e-12)
    assert A((0.0, 2.0)) == pytest.approx(90.0, abs=1e-12)            # |dx| < EPSILON, dy > 0  (:726-728)
    assert A((-1.0, 1.0)) == pytest.approx(135.0, abs=1e-12)          # bx < ax: + PI           (:739-741)
    assert A((-1.0, 0.0)) == pytest.approx(180.0, abs=1e-12)
    assert A((-1.0, -1.0)) == pytest.approx(225.0, abs=1e-12)
    assert A((0.0, -3.0)) == pytest.approx(270.0, abs=1e-12)          # |dx| < EPSILON, dy < 0  (:730-732)
    assert A((1.0, -1.0)) == pytest.approx(315.0, abs=1e-12)          # 4th quadrant: + 2 PI    (:743-746)
    assert A((1e-7, 1e-7)) == 0.0                                     # both below EPSILON      (:722-723)
    assert A((1e-7, 1.0)) == pytest.approx(90.0, abs=1e-12)           # EPSILON branch, not atan


def kat_GetAngleErr_wrap(backend):                  # Planning.cpp:760-786: (-180, 180]
    E = backend.angle_err
    assert E(10.0, 30.0) == 20.0
    assert E(350.0, 10.0) == 20.0                       # dir1 >= 180, diff = -340 <= -180 -> +360
    assert E(10.0, 350.0) == -20.0                      # dir1 < 180, diff = 340 > 180 -> -360
    assert E(0.0, 180.0) == 180.0                       # diff == 180 stays (<=)
    assert E(180.0, 0.0) == 180.0                       # diff == -180 is not > -180 -> +360
    assert E(200.0, 100.0) == -100.0


def kat_GetLatDis_sign_and_epsilon(backend, cfg):   # Planning.cpp:686-709: left of the path is positive
    L = lambda cur, pt, nxt: backend.lat_dis(cfg, cur, pt, nxt)
    assert L((5.0, 2.0), (0.0, 0.0), (10.0, 0.0)) == pytest.approx(2.0, abs=1e-15)      # left of +x heading
    assert L((5.0, -3.0), (0.0, 0.0), (10.0, 0.0)) == pytest.approx(-3.0, abs=1e-15)
    assert L((2.0, 5.0), (0.0, 0.0), (0.0, 10.0)) == -2.0      # vertical segment branch (:697): right of +y heading
    assert L((-2.0, 5.0), (0.0, 0.0), (0.0, 10.0)) == 2.0
    assert L((5.0, 1e-7), (0.0, 0.0), (10.0, 0.0)) == 0.0      # below EPSILON -> exactly 0 (:699-702)
    assert L((0.0, 1.0), (0.0, 0.0), (1.0, 1.0)) == pytest.approx(math.sqrt(0.5), rel=1e-15)


def kat_CalculateRadius(backend, dm):               # Planning.cpp:1000-1019
    pts = np.zeros(200, dm.GlobalPoint2D)
    th = np.arange(200) * 0.01
    R = 25.0
    pts["x"], pts["y"] = R * np.sin(th), R * (1 - np.cos(th))
    assert backend.radius(pts, 10, 18) == pytest.approx(R, rel=1e-9)     # circumradius of 3 points on a circle
    pts["x"], pts["y"] = np.arange(200) * 0.5, 0.0
    assert backend.radius(pts, 10, 18) == 1000.0                          # sinA < 0.001 (:1010-1012)
    assert backend.radius(pts, 195, 203) == 1000.0                        # front id 203 fenced to 199
    # middle index uses integer division before round(): (10+19)/2 = 14, not round(14.5) = 15 (:1003).  Point 14 lifted by
    # 1 m: the triangle (5,0) (7,1) (9.5,0) has area 2.25 and circumradius |am||mf||af| / (4 * 2.25) = sqrt(36.25) / 2;
    # with point 15 the three points would be collinear (radius 1000)
    pts["y"] = (np.arange(200) == 14) * 1.0
    assert backend.radius(pts, 10, 19) == pytest.approx(0.5 * math.sqrt(36.25), rel=1e-9)


def kat_SpeedPlanning_branches(backend):            # Planning.cpp:888-990
    S = lambda flag, lon, far=30.0, pos=0: backend.speed(pos, flag, lon, far, 10.0)
    for pos in (0, 1, 2):                                                 # the three cases are the same body
        assert S(0, 999.0, pos=pos) == (10.0, 0, 0.0)                     # no obstacle -> expected speed (:917-921)
        assert S(1, 20.0, pos=pos) == (3 + (20.0 - 9) / (30.0 - 9) * (10.0 - 3), 0, 0.0)   # lon-4 > 9 (:898)
    assert S(1, 12.0) == (3.0, 0, 0.0)                                    # 5 < lon-4 <= 9 (:903-907)
    assert S(1, 9.0) == (0.0, 1, -3.0)                                    # lon-4 == 5 is not > 5: AEB (:909-913)
    assert S(1, 9.5) == (3.0, 0, 0.0)
    assert S(1, 13.0) == (3.0, 0, 0.0) and S(1, 13.000001)[0] > 3.0       # boundary lon-4 > 9 is strict
    assert math.isinf(S(1, 20.0, far=9.0)[0])                             # division by (faraim-9), quirk :898
    assert backend.speed(5, 1, 1.0, 30.0, 10.0, init=(7.0, 1, -1.0)) == (7.0, 1, -1.0)   # default: untouched


def test_UpdatePlanJudge_order_and_strict_bounds(backend, cfg):      # Planning.cpp:797-832
    J = lambda hb, b, pos, lat, derr, rem: backend.plan_judge(cfg, hb, b, pos, lat, derr, rem)
    assert J(1, 2, 0, 0.5, 90.0, 0.0) == (1, 1)          # behaviour changed: first test wins (:803-806)
    assert J(1, 1, 0, -0.25, 90.0, 0.0) == (1, 2)        # |lat| > 0.2 (:810-813)
    assert J(1, 1, 0, 0.2, 50.0, 0.0) == (1, 3)          # lat == 0.2 is not > 0.2; |dir err| > 45 (:815-818)
    assert J(1, 1, 0, 0.2, -45.0, 9.5) == (1, 4)         # pos 0: remain < ROAD_REMAIN_DISTANCE 10 (:821-824)
    assert J(1, 1, 0, 0.2, 45.0, 10.0) == (0, 0)         # strict <
    assert J(1, 1, 1, 0.0, 0.0, 4.5) == (1, 4)           # pos != 0: remain < INTER_REMAIN_DISTANCE 5 (:826-829)
    assert J(1, 1, 2, 0.0, 0.0, 5.0) == (0, 0)
    assert J(1, 1, 2, 0.0, 0.0, 9.5) == (0, 0)           # the road distance does not apply off the road


# ---- Planning: Calculate_aim_dis, GetVhclLocalState, the tick counter (through ticks) ------------------------------
def kat_Calculate_aim_dis(backend, dm, cfg_off, copies):     # Planning.cpp:242-290; FLOAT members (Planning.h:20-21)
    def aim_dis(v, pos):
        sc = lcs.make_scene(dm, cfg_off, map_attr=0)
        own_decision(sc)
        sc["scene_in"]["loc"]["velocity"], sc["scene_in"]["loc"]["pos"] = v, pos
        st = tick(backend, cfg_off, sc, copies).st
        return float(st["faraim_dis"]), float(st["nearaim_dis"])
    for v, want in ((0.0, 10.0), (60.0, 40.0), (18.0, float(np.float32(18.0 / 3.6 * 5 + 4)))):
        assert aim_dis(v, 0) == (want, want)                  # clamped to [MIN, MAX] (:258-266)
    assert aim_dis(60.0, 1) == (15.0, 15.0)                   # PRE_INTER_FARAIM (:273-277)
    assert aim_dis(60.0, 2) == (10.0, 10.0)                   # INTER_FARAIM (:281-285)
    assert aim_dis(60.0, 7) == (0.0, 0.0)                     # default: stays at the initial 0 (:250-251,287)


def kat_GetVhclLocalState_and_UpdatePlanJudge(backend, dm, cfg_off, copies):     # Planning.cpp:623-676, run on last_Bpoints of a later tick
    def local(x, y=0.3, near_id=0):
        sc = lcs.make_scene(dm, cfg_off, map_attr=0)
        own_decision(sc)
        g = sc["scene_in"]["loc"]["globalpoint"]
        g["x"], g["y"], g["dir"] = x, y, 20.0
        st = sc["state"].copy()
        st["count"] = 1                                        # not the first tick: no InitialPlanning (:124-128)
        st["last_Bpoints"]["x"], st["last_Bpoints"]["y"] = np.arange(200) * 0.5, 0.0
        st["path_near_id"] = near_id
        s = tick(backend, cfg_off, sc, copies, st).st
        return (float(s["path_lat_dis"]), float(s["path_dir_err"]), int(s["path_near_id"]), int(s["path_front_near_id"]),
                float(s["remain_dis"]))
    lat, derr, mid, fid, rem = local(10.1)
    assert (mid, fid) == (20, 28)                                        # nearest point, +8 (:649)
    assert lat == pytest.approx(0.3, abs=1e-12) and derr == 20.0         # left of the path; heading error (:666,673-675)
    assert rem == (199 - 28) * 0.5                                       # arc length from the front id (:668-671)
    assert local(10.25)[2] == 20                                         # tie between points 20 and 21: strict < keeps the first (:645)
    assert local(1e5, near_id=7)[2] == 7                                 # farther than 9999 from every point: id keeps its old value
    assert local(99.4)[2:4] == (199, 207)                                # last point: index 199 -> segment 198-199 (:656-659)
    assert local(99.4)[4] == 0.0                                         # front id 207: the remain loop never runs


def kat_tick_counters_and_first_tick(backend, dm, copies):    # Planning.cpp:124-128, 189-223
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    sc = dm.gen_scenes(cfg, 0, 1, 8, junction_every=0)
    st = sc["state"].copy()
    r = backend.run(cfg, sc, st, 1, copies)
    assert int(r.st["count"]) == 1 and int(r.plan["result"]["cnt"]) == 0       # cnt = count % 100 before the increment
    r = backend.run(cfg, sc, st, 1, copies)
    assert int(r.st["count"]) == 2 and int(r.plan["result"]["cnt"]) == 1
    # the published points are every 2nd path point (:180-183) and their WGS84 image (:205-212)
    plan = r.plan
    assert plan["show"]["path_points"].tobytes() == plan["road_points"][::2].tobytes()
    lat = cfg["wgs_lat0"][0] + plan["road_points"]["y"][::2] * cfg["wgs_deg_per_m_lat"][0]
    assert np.array_equal(plan["result"]["pnts"]["x"], lat)
    r = backend.run(cfg, sc, st, 1, copies)
    assert int(r.st["count"]) == 3 and int(r.plan["result"]["cnt"]) == 2
    r = backend.run(cfg, sc, st, 97, copies)
    assert int(r.st["count"]) == 100 and int(r.plan["result"]["cnt"]) == 99
    r = backend.run(cfg, sc, st, 1, copies)
    assert int(r.st["count"]) == 1 and int(r.plan["result"]["cnt"]) == 0       # BYTE count wraps 101 -> 1 (:219-223)
    r = backend.run(cfg, sc, st, 1, copies)
    assert int(r.st["count"]) == 2 and int(r.plan["result"]["cnt"]) == 1


# ---- the answers above predate the backend fixture: their tests keep their ids on the oracle, the device and the
# 300-copy batch run them as *_hip / *_hip_and_batch
OTHER_RUNS = pytest.mark.parametrize("kind,copies", [
    pytest.param("oracle", 300, id="oracle-x300"),
    pytest.param("hip", 1, id="hip-x1", marks=pytest.mark.gpu),
    pytest.param("hip", 300, id="hip-x300", marks=pytest.mark.gpu),
])


def test_GetRoadAngle_quadrants(backends, cfg):
    kat_GetRoadAngle_quadrants(backends("oracle"), cfg)


@pytest.mark.gpu
def test_GetRoadAngle_quadrants_hip(backends, cfg):
    kat_GetRoadAngle_quadrants(backends("hip"), cfg)


def test_GetAngleErr_wrap(backends):
    kat_GetAngleErr_wrap(backends("oracle"))


@pytest.mark.gpu
def test_GetAngleErr_wrap_hip(backends):
    kat_GetAngleErr_wrap(backends("hip"))


def test_GetLatDis_sign_and_epsilon(backends, cfg):
    kat_GetLatDis_sign_and_epsilon(backends("oracle"), cfg)


@pytest.mark.gpu
def test_GetLatDis_sign_and_epsilon_hip(backends, cfg):
    kat_GetLatDis_sign_and_epsilon(backends("hip"), cfg)


def test_CalculateRadius(backends, dm):
    kat_CalculateRadius(backends("oracle"), dm)


@pytest.mark.gpu
def test_CalculateRadius_hip(backends, dm):
    kat_CalculateRadius(backends("hip"), dm)


def test_SpeedPlanning_branches(backends):
    kat_SpeedPlanning_branches(backends("oracle"))


@pytest.mark.gpu
def test_SpeedPlanning_branches_hip(backends):
    kat_SpeedPlanning_branches(backends("hip"))


def test_Calculate_aim_dis(backends, dm, cfg_off):
    kat_Calculate_aim_dis(backends("oracle"), dm, cfg_off, 1)


@OTHER_RUNS
def test_Calculate_aim_dis_hip_and_batch(backends, dm, cfg_off, kind, copies):
    kat_Calculate_aim_dis(backends(kind), dm, cfg_off, copies)


def test_GetVhclLocalState_and_UpdatePlanJudge(backends, dm, cfg_off):
    kat_GetVhclLocalState_and_UpdatePlanJudge(backends("oracle"), dm, cfg_off, 1)


@OTHER_RUNS
def test_GetVhclLocalState_and_UpdatePlanJudge_hip_and_batch(backends, dm, cfg_off, kind, copies):
    kat_GetVhclLocalState_and_UpdatePlanJudge(backends(kind), dm, cfg_off, copies)


def test_tick_counters_and_first_tick(backends, dm):
    kat_tick_counters_and_first_tick(backends("oracle"), dm, 1)


@OTHER_RUNS
def test_tick_counters_and_first_tick_hip_and_batch(backends, dm, kind, copies):
    kat_tick_counters_and_first_tick(backends(kind), dm, copies)


# ---- SearchAimPoint, road (Planning.cpp:401-434) --------------------------------------------------------------------
@COPIES
def test_aim_road_first_point_past_faraim(backend, dm, cfg_off, copies):
    # behaviour 1 in the ego lane (:401-407).  Velocity 0 -> faraim 10 (MIN).  After step i the walk from point 50 has
    # summed (i - 49) * 0.5 m (:413-414); sum - 4 > 10 first at sum = 14.5, i = 78.  At i = 77 sum - 4 == 10: strict > (:416).
    sc = lcs.make_scene(dm, cfg_off, map_attr=0)
    own_decision(sc)
    sc["scene_in"]["loc"]["velocity"] = 0.0
    r = tick(backend, cfg_off, sc, copies)
    assert r.aim() == (lane_x(78), Y2, 0.0, 78)                           # :418-421
    assert r.aim("near") == r.aim()                                        # :434
    # velocity 60 -> faraim 40 (MAX): sum - 4 > 40 first at sum = 44.5 = 89 steps, i = 138
    sc["scene_in"]["loc"]["velocity"] = 60.0
    r = tick(backend, cfg_off, sc, copies)
    assert r.aim() == (lane_x(138), Y2, 0.0, 138) and r.aim("near") == r.aim()


@COPIES
def test_aim_road_lane_end_default(backend, dm, cfg_off, copies):
    # ego on point 300 of 320: the walk sums 19 * 0.5 = 9.5 m, never past faraim 10 + 4; every step writes the default
    # Aim_id = cur_n - 1 with the lane's last point (:426-429), and near follows (:434)
    sc = lcs.make_scene(dm, cfg_off, map_attr=0)
    move_ego(sc, 300)
    own_decision(sc)
    sc["scene_in"]["loc"]["velocity"] = 0.0
    r = tick(backend, cfg_off, sc, copies)
    assert r.aim() == (lane_x(319), Y2, 0.0, 319) and r.aim("near") == r.aim()


# ---- SearchAimPoint, left / right lane change (Planning.cpp:443-499) ----------------------------------------------
@COPIES
def test_aim_left_walk_and_default_on_current_lane(backend, dm, cfg_off, copies):
    sc = lcs.make_scene(dm, cfg_off, map_attr=0)          # ego lane 2, left lane 1 (y 200)
    own_decision(sc, behavior=2, target=1)
    sc["scene_in"]["loc"]["velocity"] = 0.0
    st = sc["state"].copy()
    _, near = mark_aims(st)
    r = tick(backend, cfg_off, sc, copies, st)
    assert r.aim() == (lane_x(78), Y1, 0.0, 78)           # the left lane's own point past faraim (:448-461)
    assert r.aim("near") == near                          # only behaviour 1 and the junction copy far to near (:434,539)
    # left lane of 60 points: the walk from 50 sums 4.5 m; the default reads the CURRENT lane at leftpoint_sum - 2 = 58
    # (y of lane 2) and sets Aim_id = leftpoint_sum - 1 = 59 (:464-467)
    sc["scene_in"]["lanes"]["left_n"] = 60
    r = tick(backend, cfg_off, sc, copies)
    assert r.aim() == (lane_x(58), Y2, 0.0, 59)


@COPIES
def test_aim_right_loop_bound_is_left_sum(backend, dm, cfg_off, copies):
    sc = lcs.make_scene(dm, cfg_off, map_attr=0)          # ego lane 2, right lane 3 (y 192.5)
    own_decision(sc, behavior=3, target=3)
    sc["scene_in"]["loc"]["velocity"] = 0.0
    r = tick(backend, cfg_off, sc, copies)
    assert r.aim() == (lane_x(78), Y3, 0.0, 78)           # both lanes 320 points: the right lane's point past faraim
    # left lane of 70 points: the loop stops at leftpoint_sum - 1 = 69 (:478), 9.5 m walked, so the default takes the
    # right lane's last point (:494-497) although the right lane would reach faraim at point 78
    sc["scene_in"]["lanes"]["left_n"] = 70
    r = tick(backend, cfg_off, sc, copies)
    assert r.aim() == (lane_x(319), Y3, 0.0, 319)


@COPIES
def test_aim_right_without_left_lane_stays_stale(backend, dm, cfg_off, copies):
    # lane 1 has no left lane: leftpoint_sum = 0 (:366-368), the loop of :478 never runs and nothing writes either aim
    # point - both keep the previous tick's values (Planning.h:22-23)
    sc = lcs.make_scene(dm, cfg_off, lane_num=1, map_attr=0)
    own_decision(sc, behavior=3, target=2)
    st = sc["state"].copy()
    far, near = mark_aims(st)
    r = tick(backend, cfg_off, sc, copies, st)
    assert r.aim() == far and r.aim("near") == near


# ---- SearchAimPoint, pos 1 / 2 on the refpath (Planning.cpp:505-578) -----------------------------------------------
JUNCTION_AIMS = {
    # id: (pos, refpath, (x, y, dir, Aim_id)).  faraim: pos 1 -> 15, pos 2 -> 10; the walk stops at the first i with
    # sum(0..i+1) - 4 > faraim (:509-512).
    # n = 3: the unsigned test i < size - 4 of :517 is always true -> dir = GetRoadAngle(p[i], p[i+2]) (:519)
    "n3_i0_pos1": (1, [(0, 0), (20, 0), (20, 20)], (0.0, 0.0, 45.0, 0)),
    "n3_i0_pos2": (2, [(0, 0), (20, 0), (20, 20)], (0.0, 0.0, 45.0, 0)),
    # n = 3, i = 1: p[3] does not exist - fence: index clamped to p[2]: (10,0) -> (10,10) is 90 degrees
    "n3_i1_fenced": (2, [(0, 0), (10, 0), (10, 10)], (10.0, 0.0, 90.0, 1)),
    # n = 3, 4 m in all: default = last point, dir p[n-3] -> p[n-1] (:529-536)
    "n3_default": (2, [(0, 0), (2, 0), (2, 2)], (2.0, 2.0, 45.0, 2)),
    # n = 4: n - 4 = 0, the else branch GetRoadAngle(p[i-2], p[i]) (:523) with i - 2 < 0 clamped to 0
    "n4_i0_fenced": (2, [(0, 0), (20, 0), (20, 20), (40, 20)], (0.0, 0.0, 0.0, 0)),      # p0 -> p0: both below EPSILON
    "n4_i1_fenced": (2, [(0, 0), (0, 10), (20, 10), (20, 30)], (0.0, 10.0, 90.0, 1)),    # p0 -> p1
    # n = 5: i = 0 < 1 takes p[0] -> p[2]; i = 1 takes p[-1] clamped, p0 -> p1 = atan(3/4)
    "n5_i0": (2, [(0, 0), (20, 0), (20, 20), (20, 30), (20, 40)], (0.0, 0.0, 45.0, 0)),
    "n5_i1_fenced": (2, [(0, 0), (4, 3), (4, 23), (4, 33), (4, 43)], (4.0, 3.0, math.atan(3 / 4) * 180 / math.pi, 1)),
    # 2.5 m steps along +x to the corner (12.5, 0), then +y: sum = 15 first at i = 5.  n = 12: 5 < 8, forward p5 -> p7
    # (up, 90); n = 9: 5 < 5 fails, backward p3 -> p5 (along x, 0); n = 10: 5 < 6, 90
    "n12_forward": (2, [(2.5 * k, 0) for k in range(6)] + [(12.5, 2.5 * k) for k in range(1, 7)], (12.5, 0.0, 90.0, 5)),
    "n10_forward": (2, [(2.5 * k, 0) for k in range(6)] + [(12.5, 2.5 * k) for k in range(1, 5)], (12.5, 0.0, 90.0, 5)),
    "n9_backward": (2, [(2.5 * k, 0) for k in range(6)] + [(12.5, 2.5 * k) for k in range(1, 4)], (12.5, 0.0, 0.0, 5)),
}


@COPIES
@pytest.mark.parametrize("case", sorted(JUNCTION_AIMS))
def test_aim_junction(backend, dm, cfg_off, copies, case):
    pos, pts, (x, y, d, aim_id) = JUNCTION_AIMS[case]
    sc = lcs.make_scene(dm, cfg_off, map_attr=0)
    sc["scene_in"]["loc"]["pos"] = pos
    lcs.set_polyline(dm, sc, [(float(a), float(b)) for a, b in pts])
    own_decision(sc, refpath_n=len(pts))
    r = tick(backend, cfg_off, sc, copies)
    gx, gy, gd, gid = r.aim()
    assert (gx, gy, gid) == (x, y, aim_id)
    assert gd == pytest.approx(d, rel=1e-9, abs=1e-12)      # an atan result
    assert r.aim("near") == r.aim()                          # :539,577


@COPIES
@pytest.mark.parametrize("n", [0, 1, 2])
def test_aim_junction_short_refpath_untouched(backend, dm, cfg_off, copies, n):
    # fewer than 3 points: the walk is skipped (fence for the unsigned size()-1 and p[n-3]); far keeps its
    # stale value and near is still set from it (:539)
    sc = lcs.make_scene(dm, cfg_off, map_attr=0)
    sc["scene_in"]["loc"]["pos"] = 2
    lcs.set_polyline(dm, sc, [(0.0, 0.0), (20.0, 0.0)][:n])
    own_decision(sc, refpath_n=n)
    st = sc["state"].copy()
    far, _ = mark_aims(st)
    r = tick(backend, cfg_off, sc, copies, st)
    assert r.aim() == far and r.aim("near") == far


# ---- PreStubDecision / StubDecision speed rule (Decision.cpp:370-382, :455-467) --------------------------------------
@COPIES
@pytest.mark.parametrize("pos", [1, 2])
@pytest.mark.parametrize("ahead,flag,dis,v,dlg", [
    (12.5, 1, 12.5, 9.5, 13),          # dis_lng < 13: v = dis - 3 (:373-377)
    (13.0, 1, 13.0, 10.0, 1),          # not < 13 (:378-382)
    (2.0, 1, 2.0, 0.0, 13),            # dis - 3 < 0 -> 0
    (None, 0, 999.0, 10.0, 1),         # nothing on the path: NO_OBSTACLE_DIS
])
def test_stub_speed_rule(backend, dm, cfg, copies, pos, ahead, flag, dis, v, dlg):
    # the front refpath of pos 1 is the ego lane from the ego point on, then the junction polyline (:352-367); of pos 2 the
    # junction polyline from the ego's point on, then the exit lane (:438-452): a straight line in 0.5 m steps either way
    sc = lcs.make_junction_scene(dm, cfg, pos, obstacles=[] if ahead is None else [(ahead, 0.0)])
    r = tick(backend, cfg, sc, copies)
    assert r.around(0) == ((1, 0.0, dis) if flag else MISS)
    assert float(r.dec["velocity_expect"]) == v and int(r.dec["behavior_to_dlg"]) == dlg
    assert (int(r.dec["behavior"]), int(r.dec["light"])) == (1, 0)      # :385-399, stub_attribute 0
    assert int(r.dec["refpath_n"]) == (270 + 40 if pos == 1 else 40 + 60)


# ---- lateral sweep and its counters (Decision.cpp:915-1016), map attribute 0 ----------------------------------------
def sweep_scene(dm, cfg, width):
    # ego lane 2, one obstacle 10 m ahead (< 15, :922) and 0.25 m left of the lane centre.  The candidate paths are the
    # front path moved 0.3 i left (CreateNewPath offset -0.3 i, :942) or right (+0.3 i, :961): relative to left candidate i
    # the obstacle sits at 0.25 - 0.3 i, to right candidate i at 0.25 + 0.3 i; a candidate is taken when nothing lies in
    # its [-0.9, 0.9] window within 25 m (:944).  Left clears first at i = 4 (-0.95), right at i = 3 (1.15).
    # Candidates: BYTE i < (W - 1.8) / 0.6 (:940).  W 4.2: 4.000000000000001 -> i = 0..4;  W 3.75: 3.25 -> i = 0..3.
    sc = lcs.make_scene(dm, cfg, map_attr=0, obstacles=[(2, 10.0, 0.25)])
    sc["scene_in"]["lanes"]["lane_width"] = width
    return sc


def state_of(r):
    """(behavior, light, behavior_to_dlg, obsavoid_status, velocity_expect, obsavoid_time, no_obsaviod_time)"""
    s = r.st
    return (int(s["z_behavior"]), int(s["z_light_status"]), int(s["z_behavior_to_dlg"]), int(s["z_segment_obsavoid_status"]),
            float(r.dec["velocity_expect"]), int(s["obsavoid_time"]), int(s["no_obsaviod_time"]))


@COPIES
def test_sweep_fires_on_third_tick_left(backend, dm, cfg, copies):
    assert (420 / 100.0 - 1.8) / 0.6 == 4.000000000000001          # the quotient of :940 just above 4: five candidates
    sc = sweep_scene(dm, cfg, 420 / 100.0)
    st = sc["state"].copy()
    seq = ticks_each(backend, cfg, sc, st, 3, copies)
    assert state_of(seq[0]) == (1, 0, 1, 0, 10.0, 1, 0)           # obsavoid_time 1, 2: keep lane (:977-983)
    assert state_of(seq[1]) == (1, 0, 1, 0, 10.0, 2, 0)
    assert state_of(seq[2]) == (4, 1, 11, 1, 5.0, 3, 0)           # > 2 (:936): left avoid (:944-952), 5 km/h (:1781-1793)
    assert (int(seq[2].plan["sweep_side"]), int(seq[2].plan["sweep_index"])) == (-1, 4)
    assert int(seq[2].st["z_target_lanenum"]) == 2
    assert seq[0].around(0) == (1, 0.25, 10.0)


@COPIES
def test_sweep_right_when_no_left_candidate_clears(backend, dm, cfg, copies):
    sc = sweep_scene(dm, cfg, 3.75)
    st = sc["state"].copy()
    r = ticks_each(backend, cfg, sc, st, 3, copies)[2]
    assert state_of(r) == (5, 2, 12, 1, 5.0, 3, 0)                 # right avoid (:957-973)
    assert (int(r.plan["sweep_side"]), int(r.plan["sweep_index"])) == (1, 3)


@COPIES
def test_sweep_release_and_retrigger(backend, dm, cfg, copies):
    sc = sweep_scene(dm, cfg, 420 / 100.0)
    st = sc["state"].copy()
    assert state_of(ticks_each(backend, cfg, sc, st, 3, copies)[2])[:3] == (4, 1, 11)
    clear = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sc.items()}
    clear["scene_in"]["obs_n"] = 0
    seq = ticks_each(backend, cfg, clear, st, 4, copies)
    # clear ticks (:985-1009): no_obsaviod_time counts, the avoidance holds until it is > 3, dlg is 1 on every one (:1008);
    # obsavoid_time is not reset here
    assert [state_of(r) for r in seq] == [(4, 1, 1, 1, 5.0, 3, 1), (4, 1, 1, 1, 5.0, 3, 2), (4, 1, 1, 1, 5.0, 3, 3),
                                          (1, 0, 1, 0, 10.0, 3, 4)]
    # the obstacle is back: obsavoid_time 3 -> 4 > 2, the sweep fires on its first tick (:922-936)
    r = ticks_each(backend, cfg, sc, st, 1, copies)[0]
    assert state_of(r) == (4, 1, 11, 1, 5.0, 4, 0)
    # only a non-zero map attribute resets both counters (:1014-1015)
    attr = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sc.items()}
    attr["scene_in"]["lanes"]["lanechg_attribute"] = 1
    r = ticks_each(backend, cfg, attr, st, 1, copies)[0]
    assert (int(r.st["obsavoid_time"]), int(r.st["no_obsaviod_time"])) == (0, 0)
    seq = ticks_each(backend, cfg, sc, st, 3, copies)
    assert [state_of(x)[5] for x in seq] == [1, 2, 3] and state_of(seq[1])[:3] == (1, 0, 1) and state_of(seq[2])[:3] == (4, 1, 11)


# ---- LoadRefPath windows (Decision.cpp:553-673), observed through the published refpath and the corridors ------------


def window_scene(dm, cfg, lane_pt, ego=lcs.EGO_ID, **kw):
    """an obstacle on lane point `lane_pt` of the ego lane (map attribute 0 unless given)"""
    sc = lcs.make_scene(dm, cfg, **dict(dict(map_attr=0), **kw), obstacles=[(2, ahead_of(lane_pt))])
    move_ego(sc, ego)
    return sc


@COPIES
@pytest.mark.parametrize("id_more", [0, 3])
def test_loadrefpath_front_and_rear_slices(backend, dm, cfg, copies, id_more):
    c = cfg.copy()
    c["ID_MORE"] = id_more
    e = lcs.EGO_ID + id_more
    # front [Id+ID_MORE, Id+ID_MORE+120) (:581-587): published as the refpath of behaviour 1 (:1801-1816)
    r = tick(backend, c, window_scene(dm, c, e + 119), copies)
    assert int(r.dec["refpath_n"]) == 120
    assert (r.refpath[0]["x"], r.refpath[-1]["x"]) == (lane_x(e), lane_x(e + 119)) and (r.refpath["y"] == Y2).all()
    assert r.around(0) == (1, 0.0, 59.5)                                         # on the last front point
    assert tick(backend, c, window_scene(dm, c, e + 120), copies).around(0) == MISS    # one point beyond
    # rear: descending from Id+ID_MORE while > Id+ID_MORE-40 (:590-596): 40 points, the last one Id+ID_MORE-39
    assert tick(backend, c, window_scene(dm, c, e - 39), copies).around(1) == (1, 0.0, 19.5)
    assert tick(backend, c, window_scene(dm, c, e - 40), copies).around(1) == MISS


@COPIES
def test_loadrefpath_lane_end(backend, dm, cfg, copies):
    # ego on point 318 of 320, ID_MORE 3: the front slice [min(320, 321), min(320, 441)) is empty, the rear loop starts at
    # 320 - one past the lane, read as point 319 (fence) - and runs down to 282: 39 points, the first two equal
    c = cfg.copy()
    c["ID_MORE"] = 3
    r = tick(backend, c, window_scene(dm, c, 282, ego=318), copies)
    assert int(r.dec["refpath_n"]) == 0 and r.around(0) == EMPTY
    assert r.around(1) == (1, 0.0, 37 * 0.5)                                     # 0 m from 320 to 319, then 37 steps
    assert tick(backend, c, window_scene(dm, c, 281, ego=318), copies).around(1) == MISS


@COPIES
def test_loadrefpath_lane_start(backend, dm, cfg, copies):
    # ego on point 5: the rear loop runs 5, 4, ..., 1 - the bound is > max(0, 5 - 40) = 0, strict (:590)
    assert tick(backend, cfg, window_scene(dm, cfg, 1, ego=5), copies).around(1) == (1, 0.0, 2.0)
    assert tick(backend, cfg, window_scene(dm, cfg, 0, ego=5), copies).around(1) == MISS


@COPIES
def test_loadrefpath_left_neighbour_id_guard(backend, dm, cfg, copies):
    # map allows left (attribute 1), ego lane 2; an obstacle on point 30 of the left lane.  Left id 0: the guard
    # Id_LeftLane > 0 is strict (:606), no LF / LR at all.  Left id 1: LF = left points 1..120 (obstacle at 29 * 0.5 m),
    # LR = the single point 1 (searched, a path of one point finds nothing)
    def run(left_id):
        sc = lcs.make_scene(dm, cfg, map_attr=1, obstacles=[(1, ahead_of(30))])
        sc["scene_in"]["loc"]["id"][0, 0] = left_id
        return tick(backend, cfg, sc, copies)
    r = run(0)
    assert (r.around(2), r.around(3)) == (EMPTY, EMPTY)
    r = run(1)
    assert (r.around(2), r.around(3)) == ((1, 0.0, 14.5), MISS)


@COPIES
def test_loadrefpath_no_left_lane_shifts_front(backend, dm, cfg, copies):
    # lane 1 with left changes allowed: LF = CreateNewPath(F, -W) (:626-632), the front path moved one lane width to the
    # left (negative offset = left): y = 200 + 3.75.  An obstacle 10 m ahead, 0.5 m left of that line.
    sc = lcs.make_scene(dm, cfg, lane_num=1, map_attr=1, obstacles=[(1, 10.0, lcs.LANE_W + 0.5)])
    r = tick(backend, cfg, sc, copies)
    assert r.around(2) == (1, 0.5, 10.0)
    assert r.around(4) == EMPTY and r.around(5) == EMPTY                 # attribute 1 loads no right paths (:636)


# ---- AroundObstacle lateral windows (Decision.cpp:811-842) ---------------------------------------------------------
HW, HL = 0.9, lcs.LANE_W / 2       # half the vehicle width; half the lane width (1.875)
CORRIDORS = {
    # k: (name, lane, front?, map attribute, (lo, hi))
    0: ("F", 2, True, 1, (-HW, HW)), 1: ("R", 2, False, 1, (-HW, HW)),
    2: ("LF", 1, True, 1, (-HW, HL)), 3: ("LR", 1, False, 1, (-HW, HL)),
    4: ("RF", 3, True, 2, (-HL, HW)), 5: ("RR", 3, False, 2, (-HL, HW)),
}
INSIDE = {HW: 0.8125, -HW: -0.8125, HL: 1.75, -HL: -1.75}          # exact binary fractions 0.0875 / 0.125 inside
OUTSIDE = {HW: 1.0, -HW: -1.0, HL: 2.0, -HL: -2.0}                 # 0.1 / 0.125 outside


@COPIES
@pytest.mark.parametrize("bound", ["lo", "hi"])
@pytest.mark.parametrize("k", sorted(CORRIDORS), ids=[CORRIDORS[k][0] for k in sorted(CORRIDORS)])
def test_around_lateral_windows(backend, dm, cfg, copies, k, bound):
    # two obstacles per corridor, lateral offsets in the corridor's own frame (left of its direction positive; the rear
    # corridors run backwards, so their left is world -y): one just outside the bound and nearer, one just inside and
    # farther.  The corridor reports the inside one: the nearer one was dropped by the window.
    name, lane, front, attr, (lo, hi) = CORRIDORS[k]
    b = lo if bound == "lo" else hi
    lat_in, lat_out = INSIDE[b], OUTSIDE[b]
    d_out, d_in = (8.0, 12.0) if front else (6.0, 9.0)
    sgn = 1.0 if front else -1.0
    sc = lcs.make_scene(dm, cfg, map_attr=attr, obstacles=[(lane, sgn * d_out, sgn * lat_out), (lane, sgn * d_in, sgn * lat_in)])
    r = tick(backend, cfg, sc, copies)
    assert r.around(k) == (1, lat_in, d_in), name
