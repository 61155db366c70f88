"""Lane traffic (pp_set_traffic / pp_get_traffic_state / k_move_traffic): scripted vehicles that drive a track.

CPU: the ABI mirrors, hand-derived known answers of the numpy model (tests/traffic_model.py) with their arithmetic, the ring
track helper, and a closed loop of oracle tick + route model + traffic model in which every ego follows a slower vehicle.
GPU: the known answers on k_move_traffic (alone, batched, at the block edge), the device against the model after every advance
of a routed rollout BYTE FOR BYTE (§4h specifies every operation), with a motion pool, with a fleet in both call orders, through
pp_update_async, traffic off against a handle that never had it, the error paths, and the closed loop against the CPU loop."""
import numpy as np
import pytest

import fleet_model as fl
import map_scenes as ms
import rollout_score_model as sm
import route_model as rmod
import route_scenes as rs
import traffic_backends as tb
import traffic_model as tm
import traffic_scenes as ts
from parity_util import compare

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirrors(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(26) == dm.TrafficTrack.itemsize == 16
    assert lib.pp_sizeof(27) == dm.TrafficActor.itemsize == 40
    assert hasattr(lib, "pp_set_traffic") and hasattr(lib, "pp_get_traffic_state")
    assert dm.TrafficActor.fields["scene"][1] == 16 and dm.TrafficActor.fields["radius"][1] == 32


def _runner(dm, name, log=None):
    return tb.Runner(dm, tb.ModelBackend() if name == "model" else tb.DeviceBackend(), log)


# The known answers are written once against a runner of tests/traffic_backends.py: run(polylines, rows, steps) - rows are
# (s0, speed, track, type, radius), one actor each - gives s and the ObPoint of every actor after the set call (stage 0) and after
# every step (stage k).  Every case takes the same two steps of 1 s, so that the device can replay them all in one launch; an actor
# with speed 0 stays where the set call put it.
STEPS = [1.0, 1.0]
TRI = [(0.0, 0.0), (4.0, 0.0), (4.0, 3.0)]          # the 3-4-5 triangle: segments of 4, 3 and - closing, (4, 3) -> (0, 0) - 5


def _kat_triangle_closed(dm, run):
    # cum = 0, 4, 7, 12: L = 12.  s = 2: segment 0, t = 2 / 4 -> (2, 0).  s = 5.5: segment 1 (4 <= 5.5 < 7), t = 1.5 / 3 = 0.5 ->
    # (4, 0 + 0.5 * 3) = (4, 1.5).  s = 9.5: the closing segment 2 (7 <= 9.5), d = 12 - 7 = 5, t = 2.5 / 5 = 0.5, Q = P[0] ->
    # (4 + 0.5 * (0 - 4), 3 + 0.5 * (0 - 3)) = (2, 1.5).  type and radius travel into the slot.
    r = run([(ts.polyline(dm, TRI), True)], [(2.0, 0.0, 0, 7, 0.75), (5.5, 0.0, 0, 8, 1.0), (9.5, 0.0, 0, 9, 0.0)], STEPS)
    assert [r.at(0, a) for a in range(3)] == [(2.0, 2.0, 0.0), (5.5, 4.0, 1.5), (9.5, 2.0, 1.5)]
    assert [r.at(2, a) for a in range(3)] == [r.at(0, a) for a in range(3)]
    assert r.ob[0]["type"].tolist() == [7, 8, 9] and r.ob[0]["radius"].tolist() == [0.75, 1.0, 0.0]
    assert tm.cumulative(np.array([0.0, 4.0, 4.0]), np.array([0.0, 0.0, 3.0]), True).tolist() == [0.0, 4.0, 7.0, 12.0]


def _kat_s_on_a_vertex(dm, run):
    # s = 4 = cum[1] exactly: the largest i with cum[i] <= 4 is 1 - the LATER segment - and t = 0 -> P[1] = (4, 0); s = 7 = cum[2]:
    # i = 2, t = 0 -> P[2] = (4, 3); s = 0: i = 0, t = 0 -> P[0].  The same on the open triangle (nseg = 2, L = 7) for s = 4.
    r = run([(ts.polyline(dm, TRI), True), (ts.polyline(dm, TRI), False)], [(4.0, 0.0, 0, 0, 0.5), (7.0, 0.0, 0, 0, 0.5), (0.0, 0.0, 0, 0, 0.5), (4.0, 0.0, 1, 0, 0.5)], STEPS)
    assert [r.at(0, a) for a in range(4)] == [(4.0, 4.0, 0.0), (7.0, 4.0, 3.0), (0.0, 0.0, 0.0), (4.0, 4.0, 0.0)]
    cum = tm.cumulative(np.array([0.0, 4.0, 4.0]), np.array([0.0, 0.0, 3.0]), True)
    assert [tm.locate(cum, s) for s in (0.0, 4.0, 7.0)] == [tm.locate_walk(cum, s) for s in (0.0, 4.0, 7.0)] == [0, 1, 2]


def _kat_end_of_an_open_track(dm, run):
    # (0, 0), (2, 0), (2, 2): cum = 0, 2, 4, nseg = 2, L = 4.  s = L = 4: i ranges over [0, 2), the largest with cum[i] <= 4 is 1, and
    # t = (4 - 2) / 2 = 1 on the LAST segment -> (2, 0 + 1 * 2) = (2, 2).
    r = run([(ts.polyline(dm, [(0.0, 0.0), (2.0, 0.0), (2.0, 2.0)]), False)], [(4.0, 0.0, 0, 0, 0.5)], STEPS)
    assert r.at(0, 0) == (4.0, 2.0, 2.0)
    assert tm.point_at(np.array([0.0, 2.0, 2.0]), np.array([0.0, 0.0, 2.0]), np.array([0.0, 2.0, 4.0]), 4.0)[:2] == (1, 1.0)


def _kat_open_track_clamps_both_ways(dm, run):
    # (0, 0) -> (10, 0), L = 10.  From s = 9 at +3 m/s: 9 + 3 * 1 = 12 > L -> 10, (10, 0), and it stays.  From s = 1 at -3 m/s:
    # 1 + (-3) = -2, not >= 0 -> 0, (0, 0), and it stays.  An s0 outside the track is clamped by the set call: 25 -> 10, -1 -> 0.
    r = run([(ts.polyline(dm, [(0.0, 0.0), (10.0, 0.0)]), False)], [(9.0, 3.0, 0, 0, 0.5), (1.0, -3.0, 0, 0, 0.5), (25.0, 0.0, 0, 0, 0.5), (-1.0, 0.0, 0, 0, 0.5)], STEPS)
    assert [r.at(0, a) for a in range(4)] == [(9.0, 9.0, 0.0), (1.0, 1.0, 0.0), (10.0, 10.0, 0.0), (0.0, 0.0, 0.0)]
    assert [r.at(1, a) for a in range(2)] == [(10.0, 10.0, 0.0), (0.0, 0.0, 0.0)]
    assert [r.at(2, a) for a in range(2)] == [(10.0, 10.0, 0.0), (0.0, 0.0, 0.0)]


def _kat_closed_track_wraps_both_ways(dm, run):
    # The triangle, L = 12.  Forwards from 11 at +2: 13, q = floor(13 / 12) = 1, 13 - 1 * 12 = 1 -> (1, 0); then 3 -> (3, 0).
    # Backwards from 0.5 at -3: -2.5, q = floor(-2.5 / 12) = -1, -2.5 - (-1 * 12) = 9.5 -> (2, 1.5) (the closing segment, as above);
    # then 6.5 -> segment 1, t = 2.5 / 3.  An s0 of 12 = L is wrapped by the set call: q = 1, 12 - 12 = 0 -> P[0].
    r = run([(ts.polyline(dm, TRI), True)], [(11.0, 2.0, 0, 0, 0.5), (0.5, -3.0, 0, 0, 0.5), (12.0, 0.0, 0, 0, 0.5)], STEPS)
    assert [r.at(0, a) for a in range(3)] == [(11.0, 4.0 + (4.0 / 5.0) * (0.0 - 4.0), 3.0 + (4.0 / 5.0) * (0.0 - 3.0)), (0.5, 0.5, 0.0), (0.0, 0.0, 0.0)]
    assert [r.at(1, a) for a in range(2)] == [(1.0, 1.0, 0.0), (9.5, 2.0, 1.5)]
    assert [r.at(2, a) for a in range(2)] == [(3.0, 3.0, 0.0), (6.5, 4.0, 0.0 + (2.5 / 3.0) * 3.0)]


def _kat_several_laps_in_one_step(dm, run):
    # From 2 at +25 m/s: 27, q = floor(27 / 12) = 2 (> 1), 27 - 2 * 12 = 3 -> (3, 0); then 28, q = 2, 4 -> the vertex (4, 0).
    # From 2 at -37: -35, q = floor(-35 / 12) = -3, -35 + 36 = 1 -> (1, 0).
    r = run([(ts.polyline(dm, TRI), True)], [(2.0, 25.0, 0, 0, 0.5), (2.0, -37.0, 0, 0, 0.5)], STEPS)
    assert [r.at(1, a) for a in range(2)] == [(3.0, 3.0, 0.0), (1.0, 1.0, 0.0)]
    assert r.at(2, 0) == (4.0, 4.0, 0.0) and r.at(2, 1) == (0.0, 0.0, 0.0)          # 1 - 37 = -36, q = -3, -36 + 36 = 0


def _kat_zero_length_segments(dm, run):
    # (0, 0), (2, 0), (2, 0), (4, 0), (4, 0): cum = 0, 2, 2, 4, 4 - a zero-length segment in the middle (1) and at the end (3).
    # s = 2: the largest i with cum[i] <= 2 is 2 (past the empty segment), t = 0 -> (2, 0).  s = 3: i = 2, t = 1 / 2 -> (3, 0).
    # s = 4 = L: i = 3, d = cum[4] - cum[3] = 0 -> t = 0 (no division) -> P[3] = (4, 0).  s = 1: i = 0, t = 0.5 -> (1, 0).
    p = ts.polyline(dm, [(0.0, 0.0), (2.0, 0.0), (2.0, 0.0), (4.0, 0.0), (4.0, 0.0)])
    r = run([(p, False)], [(2.0, 0.0, 0, 0, 0.5), (3.0, 0.0, 0, 0, 0.5), (4.0, 0.0, 0, 0, 0.5), (1.0, 1.0, 0, 0, 0.5)], STEPS)
    assert [r.at(0, a) for a in range(4)] == [(2.0, 2.0, 0.0), (3.0, 3.0, 0.0), (4.0, 4.0, 0.0), (1.0, 1.0, 0.0)]
    assert r.at(1, 3) == (2.0, 2.0, 0.0) and r.at(2, 3) == (3.0, 3.0, 0.0)          # it drives across the empty segment
    cum = tm.cumulative(p["x"], p["y"], False)
    assert cum.tolist() == [0.0, 2.0, 2.0, 4.0, 4.0] and [tm.locate(cum, s) for s in (2.0, 4.0)] == [tm.locate_walk(cum, s) for s in (2.0, 4.0)] == [2, 3]


def _kat_two_point_tracks(dm, run):
    # (1, 1), (4, 5): one segment of sqrt(9 + 16) = 5.  Open, s = 2.5: t = 0.5 -> (2.5, 3).  Closed: nseg = 2, L = 10, the closing
    # segment runs back; s = 7.5: i = 1, t = 2.5 / 5, Q = P[0] -> (4 + 0.5 * (1 - 4), 5 + 0.5 * (1 - 5)) = (2.5, 3) again.
    p = ts.polyline(dm, [(1.0, 1.0), (4.0, 5.0)])
    r = run([(p, False), (p, True)], [(2.5, 0.0, 0, 0, 0.5), (7.5, 0.0, 1, 0, 0.5), (2.5, 5.0, 1, 0, 0.5)], STEPS)
    assert [r.at(0, a) for a in range(3)] == [(2.5, 2.5, 3.0), (7.5, 2.5, 3.0), (2.5, 2.5, 3.0)]
    assert r.at(1, 2) == (7.5, 2.5, 3.0) and r.at(2, 2) == (2.5, 2.5, 3.0)           # 12.5 -> q = 1 -> 2.5: a lap of the two-point loop


KATS = [_kat_triangle_closed, _kat_s_on_a_vertex, _kat_end_of_an_open_track, _kat_open_track_clamps_both_ways, _kat_closed_track_wraps_both_ways,
        _kat_several_laps_in_one_step, _kat_zero_length_segments, _kat_two_point_tracks]


@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, kat):
    kat(dm, _runner(dm, "model"))


def test_ring_track_helper(dm):
    """Lane 2 of the four ring roads and their junction polylines as one closed track: 4 * (260 + 40) points, every segment - the
    closing one included - between 0.45 and 0.55 m, and the lap as long as the ring says (4 * (129.5 + 20.5) m)."""
    m = rs.build_ring(dm)
    p = ts.ring_track(dm, m, 2)
    cum = tm.cumulative(p["x"], p["y"], True)
    seg = np.diff(cum)
    assert len(p) == 4 * ts.SEG == 1200 and len(seg) == 1200
    assert 0.45 < seg.min() and seg.max() < 0.55
    assert abs(cum[-1] - 4 * (rs.ROAD_LEN + rs.JUNC_LEN)) < 0.05
    inner = ts.ring_track(dm, m, 1)                      # the inside lane: shorter
    assert tm.cumulative(inner["x"], inner["y"], True)[-1] < cum[-1]


# ---- the followers: every ego has a slower vehicle ahead on its lane's ring track -------------------------------------------------
F_N, F_TICKS = 16, 300
F_GAP, F_SPEED, F_RADIUS, F_TYPE = 20.0, 1.5, 0.9, 7
_CPU = {}


def _followers(dm):
    """16 ring egos of the closed loop of tests/test_route.py (lanes 1 / 2, 120 .. 170 points into their first road; grid stage off)
    that do not start on lane 2 of the two-lane road 3.  Chosen on the CPU loop: an ego there answers the slower vehicle with the
    reference's lane change to lane 1 and drives on at a HIGHER speed (85.6 m in 300 ticks against 81.8 m on the empty ring) - a
    reaction, but not the following this test is about.  Every ego owns one obstacle entry: a vehicle F_GAP = 20 m ahead of it on
    the closed track of its own lane at F_SPEED = 1.5 m/s (5.4 km/h; the planner drives the empty ring at 10 km/h)."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, 2 * F_N, seed=3, lanes=(1, 2), ids=(120, 170), legs=(6, 10), n_obs=1)
    loc = sc["scene_in"]["loc"]
    keep = np.flatnonzero(~((loc["road_num"] == 3) & (loc["lane_num"] == 2)))[:F_N]
    assert len(keep) == F_N
    legs = np.concatenate([legs[rf[k]:rf[k + 1]] for k in keep])
    rf = np.concatenate([[0], np.cumsum([rf[k + 1] - rf[k] for k in keep])]).astype(np.int32)
    sc = dict(sc, scene_in=sc["scene_in"][keep].copy(), state=sc["state"][keep].copy(), obs_pool=np.zeros(F_N, dm.ObPoint), mot_pool=None)
    sc["obs_pool"]["radius"] = 0.5                        # (the empty run: obs_n = 0, nobody reads it)
    sc["scene_in"]["obs_off"] = np.arange(F_N)
    polylines = [(ts.ring_track(dm, m, 1), True), (ts.ring_track(dm, m, 2), True)]
    tracks, pts = ts.pack(dm, polylines)
    rows = []
    for s in range(F_N):
        loc = sc["scene_in"]["loc"][s]
        lane = int(loc["lane_num"])
        p = polylines[lane - 1][0]
        here = tm.cumulative(p["x"], p["y"], True)[ts.SEG * (int(loc["road_num"]) - 1) + int(loc["id"][lane - 1])]
        rows.append((here + F_GAP, F_SPEED, s, 0, lane - 1, F_TYPE, F_RADIUS))
    return cfg, m, sc, legs, rf, tracks, pts, ts.actors(dm, rows)


def _cpu_loop(dm, oracle, traffic):
    if traffic in _CPU:
        return _CPU[traffic]
    cfg, m, sc, legs, rf, tracks, pts, act = _followers(dm)
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt = float(model["dt"][0])
    raw = sc["scene_in"].copy()
    raw["obs_n"] = 1 if traffic else 0
    si, st, flags, obs = ms.resolve(dm, m, raw), sc["state"].copy(), np.zeros(F_N, np.int32), sc["obs_pool"].copy()
    tr = None
    if traffic:
        tr = tm.Traffic(tracks, pts, act, si["obs_off"])
        obs, _ = tr.place(obs, None, 0.0)
    scores = sm.new_scores(dm.RolloutScore, F_N)
    sins, pools, ss, ob_ticks = [si], [obs], [None if tr is None else tr.s.copy()], np.zeros(F_N, np.int64)
    for t in range(F_TICKS + 1):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        sm.fold(scores, cfg, dt, si, plan, st, obs, flags)
        ob_ticks += plan["ob_flag"] != 0
        if t < F_TICKS:
            si, flags, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
            if tr is not None:
                obs, _ = tr.place(obs, None, dt)
            sins.append(si), pools.append(obs), ss.append(None if tr is None else tr.s.copy())
    _CPU[traffic] = dict(cfg=cfg, m=m, sc=dict(sc, scene_in=raw), legs=legs, rf=rf, tracks=tracks, pts=pts, act=act, sins=sins, pools=pools, s=ss,
                         scores=scores, ob_ticks=ob_ticks, flags=flags)
    return _CPU[traffic]


def test_followers_closed_loop_on_the_cpu(dm, oracle):
    """Oracle tick + route model + traffic model, 301 scored ticks.  Established here, on the CPU alone: every ego sees its vehicle
    (PlanOut.ob_flag != 0 on at least 209 of the ticks), travels less than on the empty ring (about 30 m against 71 .. 82 m: it falls
    in behind at the vehicle's 1.5 m/s) and never touches it (the smallest clearance of the run is 8.4 m: the reference's speed plan
    keeps its distance)."""
    r, e = _cpu_loop(dm, oracle, True), _cpu_loop(dm, oracle, False)
    print("ob_flag ticks", r["ob_ticks"].tolist(), "\ndist", np.round(r["scores"]["dist"], 1).tolist(), "\nempty ring", np.round(e["scores"]["dist"], 1).tolist(),
          "\nmin clearance", np.round(r["scores"]["min_clearance"], 2).tolist())
    assert (r["ob_ticks"] > 0).all() and not e["ob_ticks"].any()
    assert (r["scores"]["dist"] < e["scores"]["dist"]).all()
    assert (r["scores"]["n_collision_ticks"] == 0).all() and (r["scores"]["min_clearance"] > 0).all()
    assert not r["flags"].any() and (r["scores"]["n_ticks"] == F_TICKS + 1).all()
    # the vehicles drove on: 300 steps of 1.5 * 0.1 m along the track
    assert np.allclose(r["s"][-1] - r["s"][0], F_TICKS * F_SPEED * 0.1, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, kat):
    """The known answers above on k_move_traffic (pp_set_traffic, then two advances), each also held byte for byte against the model."""
    kat(dm, _runner(dm, "device"))


_LOG = []


def _kat_log(dm):
    if not _LOG:
        run = _runner(dm, "model", _LOG)
        for kat in KATS:
            kat(dm, run)
    return _LOG


@gpu
@pytest.mark.parametrize("count", [None, 1, 255, 256, 257])
def test_kat_batch_and_block_edge(dm, count):
    """All known answers as actors of ONE launch (count None: the 24 of them), and repeated cyclically to 1, 255, 256 and 257 actors -
    the edge of the 256-thread block.  Every actor gives the bytes its case gave alone, and the device the model's."""
    log = _kat_log(dm)
    n = tb.batched(dm, tb.DeviceBackend(), log, repeat_to=count)
    assert n == (count if count is not None else sum(len(c["rows"]) for c in log))


def _planner(dm, cfg, m, sc, n_obs, slack=0, motion=False):
    pl = dm.Planner(cfg, device=0, **rs.caps(m, len(sc["scene_in"]), n_obs, slack))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=motion)
    pl.set_state(sc["state"])
    return pl


S_N, S_TICKS, S_OBS = 64, 120, 3


def _step_scene(dm, n=S_N, n_obs=S_OBS, stride=None, seed=5):
    """Routed ring egos with n_obs own obstacle entries each: entry 0 static (well off the road), entry 1 a vehicle on the closed ring
    track of lane 1 or 2, entry 2 one on the OPEN track of lane 3 of road 1 - mixed speeds, some negative, fast enough that closed
    tracks wrap and the open one clamps at both ends within the run."""
    stride = stride or n_obs
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, n, seed=seed, legs=(3, 6), n_obs=stride)
    rng = np.random.default_rng(seed)
    sc["scene_in"]["obs_n"] = n_obs
    pool = sc["obs_pool"]
    pool["x"], pool["y"], pool["radius"], pool["type"] = rng.uniform(0.0, 50.0, len(pool)), rng.uniform(0.0, 50.0, len(pool)), 0.5, 1
    polylines = [(ts.ring_track(dm, m, 1), True), (ts.ring_track(dm, m, 2), True), (ts.lane_track(dm, m, 1, 3), False)]
    tracks, pts = ts.pack(dm, polylines)
    rows = []
    for s in range(n):
        rows.append((rng.uniform(-100.0, 1500.0), rng.choice([-40.0, -3.0, 0.0, 2.5, 8.0, 55.0]), s, 1, s % 2, 100 + s, 0.9))
        rows.append((rng.uniform(0.0, 129.5), rng.choice([-12.0, 0.75, 12.0]), s, 2, 2, 200 + s, 1.1))
    return cfg, m, sc, legs, rf, tracks, pts, ts.actors(dm, rows)


def _slices(pl, n):
    return [pl.get_obstacles(s) for s in range(n)]


@gpu
def test_step_check_against_the_model(dm):
    """The primary criterion: 120 ticks on 64 routed ring egos with two vehicles each.  After every advance the model, applied to the
    previous pool and state, gives the staged pool (read back once the next tick has adopted it), every scene's slice and the state
    array byte for byte; the static entries never change and obs_off / obs_n are those of the same run without traffic."""
    cfg, m, sc, legs, rf, tracks, pts, act = _step_scene(dm)
    n, model = S_N, dm.default_ego_model()
    dt = float(model["dt"][0])
    plain = _planner(dm, cfg, m, sc, S_OBS)
    plain.set_route(legs, rf)
    pl = _planner(dm, cfg, m, sc, S_OBS)
    pl.set_route(legs, rf)
    pl.set_traffic(tracks, pts, act)
    tr = tm.Traffic(tracks, pts, act, sc["scene_in"]["obs_off"])
    want, _ = tr.place(sc["obs_pool"], None, 0.0)
    assert pl.traffic_state().tobytes() == tr.s.tobytes()
    assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * S_OBS).tobytes() == want.tobytes()
    wrapped = clamped = 0
    for t in range(S_TICKS):
        pl.tick(), plain.tick()
        if t > 0:                                                   # the set the last advance staged is the current one now
            assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * S_OBS).tobytes() == want.tobytes(), f"tick {t}: pool"
        pl.advance_async(model), plain.advance_async(model)
        before = tr.s.copy()
        want, _ = tr.place(want, None, dt)
        wrapped += int((np.abs(tr.s - before) > 100.0).sum())
        clamped += int(((tr.s == 0.0) | (tr.s == tr.length(2)))[1::2].sum())
        got = pl.traffic_state()
        assert got.tobytes() == tr.s.tobytes(), f"tick {t}: state of actors {np.flatnonzero(got != tr.s).tolist()}"
        sin, sin0 = pl.get_scene_in(), plain.get_scene_in()
        assert np.array_equal(sin["obs_off"], sin0["obs_off"]) and np.array_equal(sin["obs_n"], sin0["obs_n"]) and (sin["obs_n"] == S_OBS).all()
        for s, sl in enumerate(_slices(pl, n)):
            assert sl.tobytes() == want[s * S_OBS:(s + 1) * S_OBS].tobytes(), f"tick {t}, scene {s}: slice"
        assert want[0::S_OBS].tobytes() == sc["obs_pool"][0::S_OBS].tobytes()
    pl.tick(), plain.tick()
    assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * S_OBS).tobytes() == want.tobytes()
    assert plain.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * S_OBS).tobytes() == sc["obs_pool"].tobytes()
    print(f"wraps {wrapped}, actor-ticks at an end of the open track {clamped}")
    assert wrapped > 5 and clamped > 100
    pl.close(), plain.close()


@gpu
def test_motion_pool_and_dynamic_obstacles(dm):
    """With a motion pool and dynamic_obstacles = 1 a traffic entry gets a zero ObMotion - whatever velocity the caller's pool gave
    it - and the tick's snapshot (§5 G4) shows it where k_move_traffic put it, while an own entry with a velocity still drifts: the
    scorecard, which folds the snapshot's clearances, equals the model fed the model's snapshots byte for byte."""
    n, n_obs, ticks = 8, 3, 6
    cfg = dm.default_config(128)
    cfg["grid_stage"], cfg["dynamic_obstacles"] = 0, 1
    sc = dm.gen_scenes(cfg, 0, n, n_obs, junction_every=0)
    ego = sc["scene_in"]["loc"]["globalpoint"]
    pool, mot = sc["obs_pool"].reshape(n, n_obs), sc["mot_pool"].reshape(n, n_obs)
    pool["radius"], pool["x"], pool["y"] = 0.5, ego["x"][:, None] + 300.0, ego["y"][:, None] + 300.0
    pool["x"][:, 0], pool["y"][:, 0] = ego["x"] + 30.0, ego["y"] + 2.0          # entry 0: own, approaching at 2 m/s
    mot["vx"], mot["vy"] = 0.0, 0.0
    mot["vx"][:, 0] = -2.0
    sc["state"]["tick"] = 10                                                     # (§5 G4 moves by v * dyn_dt * tick: from the first tick on)
    mot["vx"][:, 1], mot["vy"][:, 1] = 500.0, -500.0                             # entry 1: the vehicle's slot, with rubbish motion
    polylines = [(ts.polyline(dm, [(float(ego["x"][s]) - 20.0, float(ego["y"][s]) + 12.0), (float(ego["x"][s]) + 80.0, float(ego["y"][s]) + 12.0)]), False) for s in range(n)]
    tracks, pts = ts.pack(dm, polylines)
    act = ts.actors(dm, [(20.0, 2.0 if s % 2 else 0.0, s, 1, s, 5, 0.9) for s in range(n)])
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
    pl.set_scenes(sc, with_motion=True)
    pl.set_state(sc["state"])
    pl.set_traffic(tracks, pts, act)
    pl.score_begin()
    model = dm.default_ego_model()
    dt = float(model["dt"][0])
    tr = tm.Traffic(tracks, pts, act, sc["scene_in"]["obs_off"])
    wpool, wmot = tr.place(sc["obs_pool"], sc["mot_pool"], 0.0)
    assert wmot.reshape(n, n_obs)[:, 1].tobytes() == bytes(16 * n) and wmot.reshape(n, n_obs)[:, 0].tobytes() == mot[:, 0].tobytes()
    scores, flags = sm.new_scores(dm.RolloutScore, n), np.zeros(n, np.int32)
    plan_p = dm.pinned_empty(n, dm.PlanOut)
    drift = 0.0
    for t in range(ticks):
        sin, st_before = pl.get_scene_in(), pl.get_state()
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * n_obs).tobytes() == wpool.tobytes(), f"tick {t}: pool"
        assert pl.read_device(dm.BUF_MOT_POOL, dm.ObMotion, n * n_obs).tobytes() == wmot.tobytes(), f"tick {t}: motion pool"
        now = sm.snapshot(cfg, sin, st_before, wpool, wmot)
        assert now.reshape(n, n_obs)[:, 1].tobytes() == wpool.reshape(n, n_obs)[:, 1].tobytes()            # the vehicle: not moved again
        drift = max(drift, float(np.abs(now["x"].reshape(n, n_obs)[:, 0] - wpool["x"].reshape(n, n_obs)[:, 0]).max()))
        sm.fold(scores, cfg, dt, sin, np.array(plan_p), pl.get_state(), now, flags)
        pl.advance_async(model)
        flags = pl.ego_flags()
        wpool, wmot = tr.place(wpool, wmot, dt)
    got = pl.rollout_score()
    for k in ("min_clearance", "min_clearance_tick", "min_clearance_obs", "n_collision_ticks", "n_ticks"):
        assert got[k].tobytes() == scores[k].tobytes(), (k, got[k].tolist(), scores[k].tolist())
    # the vehicle, 12 m to the side where it was put, is the nearest obstacle (with the 500 m/s of the caller's pool it would be
    # half a kilometre away on the first tick); the own entry, 28 m ahead, did drift
    assert drift > 1.9 and (scores["min_clearance_obs"] == 1).all() and (scores["min_clearance"] < 12.0).all()
    pl.close()


@gpu
@pytest.mark.parametrize("fleet_first", [True, False])
def test_with_the_fleet_in_both_call_orders(dm, fleet_first):
    """Fleet and traffic on one handle, set in either order: after every advance the peer slots are what fleet_model.couple gives and
    the traffic entries what the traffic model gives, on the same staged set.  A slot that is a peer slot (>= n_own) is PP_ERR_ARG."""
    n, own, K, ticks = 32, 2, 3, 20
    cfg, m, sc, legs, rf, tracks, pts, act = _step_scene(dm, n=n, n_obs=own, stride=own + K, seed=9)
    act = act[0::2].copy()                                           # the vehicle of entry 1 only
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"] = 40.0, K
    worlds = [0, 5, n]
    pl = _planner(dm, cfg, m, sc, own + K)
    pl.set_route(legs, rf)
    if fleet_first:
        pl.set_fleet(worlds, fm)
        pl.set_traffic(tracks, pts, act)
    else:
        pl.set_traffic(tracks, pts, act)
        pl.set_fleet(worlds, fm)
    bad = act.copy()
    bad["slot"][3] = own                                             # the first peer slot of scene 3
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_traffic(tracks, pts, bad)
    off, n_own = sc["scene_in"]["obs_off"].copy(), sc["scene_in"]["obs_n"].copy()
    tr = tm.Traffic(tracks, pts, act, off)
    pool, _ = tr.place(sc["obs_pool"], None, 0.0)
    model = dm.default_ego_model()
    dt, peers = float(model["dt"][0]), 0
    for t in range(ticks + 1):
        got = pl.get_scene_in()
        want, pool, _ = fl.couple(fm, worlds, off, n_own, got, pool)          # (reads only the poses of `got`; writes obs_off / obs_n)
        assert np.array_equal(got["obs_off"], want["obs_off"]) and np.array_equal(got["obs_n"], want["obs_n"]), f"stage {t}"
        for s, sl in enumerate(_slices(pl, n)):
            a, c = int(want["obs_off"][s]), int(want["obs_n"][s])
            assert sl.tobytes() == pool[a:a + c].tobytes(), f"stage {t}, scene {s}: slice"
        assert pl.traffic_state().tobytes() == tr.s.tobytes()
        peers += int((got["obs_n"] - own).sum())
        if t < ticks:
            pl.tick()
            pl.advance_async(model)
            pool, _ = tr.place(pool, None, dt)
    assert peers > ticks * n // 4
    pl.close()


@gpu
def test_update_async_places_the_actors_unstepped(dm):
    """A caller-uploaded pool with rubbish in the traffic entries comes out with the actors at the current s - no step - and so does an
    update that brings only SceneIn records; a pool that stops short of a pinned entry is PP_ERR_ARG."""
    cfg, m, sc, legs, rf, tracks, pts, act = _step_scene(dm, n=16, seed=11)
    n, model = 16, dm.default_ego_model()
    pl = _planner(dm, cfg, m, sc, S_OBS)
    pl.set_route(legs, rf)
    pl.set_traffic(tracks, pts, act)
    tr = tm.Traffic(tracks, pts, act, sc["scene_in"]["obs_off"])
    pool, _ = tr.place(sc["obs_pool"], None, 0.0)
    for _ in range(3):
        pl.tick()
        pl.advance_async(model)
        pool, _ = tr.place(pool, None, float(model["dt"][0]))
    pl.tick()
    s_now = tr.s.copy()
    up = dm.pinned_copy(np.frombuffer(bytes([0x5A]) * (n * S_OBS * dm.ObPoint.itemsize), dm.ObPoint))
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.update_async(obs_pool=up, n_obs_total=n * S_OBS - 1)
    pl.update_async(obs_pool=up)
    assert pl.traffic_state().tobytes() == s_now.tobytes()
    pl.tick()
    want, _ = tr.place(np.array(up), None, 0.0)
    assert tr.s.tobytes() == s_now.tobytes()
    assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * S_OBS).tobytes() == want.tobytes()
    assert want[0::S_OBS].tobytes() == bytes([0x5A]) * (n * 24)                      # the other entries are the caller's
    sin = dm.pinned_copy(pl.get_scene_in())
    pl.update_async(scene_in=sin)                                                    # obstacles carried over
    pl.tick()
    assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * S_OBS).tobytes() == want.tobytes()
    assert pl.traffic_state().tobytes() == s_now.tobytes()
    pl.advance_async(model)                                                          # ... and the next advance steps from there
    want, _ = tr.place(want, None, float(model["dt"][0]))
    assert pl.traffic_state().tobytes() == tr.s.tobytes()
    assert np.concatenate(_slices(pl, n)).tobytes() == want.tobytes()
    pl.close()


def _rollout_record(dm, pl, n, n_obs, ticks):
    pl.rollout(ticks)
    pl.sync()
    return pl.get_scene_in(), pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * n_obs), pl.get_plan(), pl.ego_flags()


@gpu
def test_off_means_off(dm):
    """After set_traffic(None) 40 ticks of a routed rollout give SceneIn, pool, PlanOut and flags identical to a handle that never
    made the call (started from the pool the set call left: switching off leaves the entries where they are); pp_set_egos switches
    traffic off as well."""
    cfg, m, sc, legs, rf, tracks, pts, act = _step_scene(dm, n=32, seed=13)
    n = 32
    placed, _ = tm.Traffic(tracks, pts, act, sc["scene_in"]["obs_off"]).place(sc["obs_pool"], None, 0.0)
    sc_placed = dict(sc, obs_pool=placed)
    outs = []
    for mode in ("never", "off", "set_egos"):
        pl = _planner(dm, cfg, m, sc_placed if mode == "never" else sc, S_OBS)
        if mode != "never":
            pl.set_traffic(tracks, pts, act)
            assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * S_OBS).tobytes() == placed.tobytes()
        if mode == "off":
            pl.set_traffic(None)
        if mode == "set_egos":
            pl.set_egos(sc_placed, with_motion=False)
            pl.set_state(sc["state"])
        if mode != "never":
            with pytest.raises(dm.PlannerError, match="error -4:"):
                pl.traffic_state()
        pl.set_route(legs, rf)
        outs.append(_rollout_record(dm, pl, n, S_OBS, 40))
        pl.close()
    for k in (1, 2):
        for a, b, name in zip(outs[k], outs[0], ("SceneIn", "pool", "PlanOut", "flags")):
            assert a.tobytes() == b.tobytes(), (("never", "off", "set_egos")[k], name)
    assert outs[0][1].tobytes() == placed.tobytes()
    # ... and it was not a run that could not tell: with traffic left on, the pool has moved
    pl = _planner(dm, cfg, m, sc, S_OBS)
    pl.set_traffic(tracks, pts, act)
    pl.set_route(legs, rf)
    assert _rollout_record(dm, pl, n, S_OBS, 40)[1].tobytes() != placed.tobytes()
    pl.close()


@gpu
def test_errors_leave_the_traffic_as_it_was(dm):
    """Every refused call leaves the previous traffic running: the advance after it matches the model."""
    cfg, m, sc, legs, rf, tracks, pts, act = _step_scene(dm, n=8, seed=17)
    n, model = 8, dm.default_ego_model()
    dt = float(model["dt"][0])
    empty = dm.Planner(cfg, device=0, **rs.caps(m, n, S_OBS))
    with pytest.raises(dm.PlannerError, match="error -4:"):                    # no resident scenes
        empty.set_traffic(tracks, pts, act)
    empty.close()
    pl = _planner(dm, cfg, m, sc, S_OBS)
    pl.set_route(legs, rf)
    pl.set_traffic(tracks, pts, act)
    tr = tm.Traffic(tracks, pts, act, sc["scene_in"]["obs_off"])
    pool, _ = tr.place(sc["obs_pool"], None, 0.0)

    def edit(arr, field, k, v):
        out = arr.copy()
        out[field][k] = v
        return out

    two = ts.actors(dm, [(0.0, 1.0, 0, 1, 0, 0, 0.5), (5.0, 1.0, 0, 1, 1, 0, 0.5)])          # the same (scene, slot) twice
    flat, flat_pts = ts.pack(dm, [(ts.polyline(dm, [(1.0, 1.0), (1.0, 1.0), (1.0, 1.0)]), True)])
    cases = [
        ("track slice outside points", (edit(tracks, "point_off", 2, len(pts) - 10), pts, act)),
        ("negative point_off", (edit(tracks, "point_off", 0, -1), pts, act)),
        ("n_points < 2", (edit(tracks, "n_points", 1, 1), pts, act)),
        ("non-finite point", (tracks, edit(pts, "y", 700, np.nan), act)),
        ("infinite point", (tracks, edit(pts, "x", 3, np.inf), act)),
        ("non-finite s0", (tracks, pts, edit(act, "s0", 2, np.nan))),
        ("non-finite speed", (tracks, pts, edit(act, "speed", 5, -np.inf))),
        ("negative radius", (tracks, pts, edit(act, "radius", 1, -0.5))),
        ("non-finite radius", (tracks, pts, edit(act, "radius", 1, np.nan))),
        ("scene out of range", (tracks, pts, edit(act, "scene", 0, n))),
        ("negative scene", (tracks, pts, edit(act, "scene", 0, -1))),
        ("track out of range", (tracks, pts, edit(act, "track", 4, len(tracks)))),
        ("slot outside the own entries", (tracks, pts, edit(act, "slot", 6, S_OBS))),
        ("negative slot", (tracks, pts, edit(act, "slot", 6, -1))),
        ("two actors on one slot", (tracks, pts, two)),
        ("closed track without length", (flat, flat_pts, ts.actors(dm, [(0.0, 1.0, 0, 1, 0, 0, 0.5)]))),
    ]
    for what, args in cases:
        pl.tick()                                                              # (adopts what the last advance staged: nothing is staged now)
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_traffic(*args)
        pl.advance_async(model)
        with pytest.raises(dm.PlannerError, match="error -4:"):                # an update is staged - for a new set and for off alike
            pl.set_traffic(tracks, pts, act)
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.set_traffic(None)
        pool, _ = tr.place(pool, None, dt)
        assert pl.traffic_state().tobytes() == tr.s.tobytes(), what
        assert np.concatenate(_slices(pl, n)).tobytes() == pool.tobytes(), what
    pl.close()


@gpu
def test_followers_closed_loop_agrees_with_the_cpu_loop(dm, oracle):
    """The end-to-end run on the device: the CPU loop's scene, 300 advances with scoring on.  The staged records agree with the CPU
    loop's within the bounds tests/test_route.py uses for its closed loop (parity_util.compare); the vehicles' arc lengths and pool
    entries are equal byte for byte; the scorecard's integer fields are equal."""
    r = _cpu_loop(dm, oracle, True)
    pl = _planner(dm, r["cfg"], r["m"], r["sc"], 1)
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    pl.score_begin()
    model = dm.default_ego_model()
    assert pl.traffic_state().tobytes() == r["s"][0].tobytes()
    worst = 0.0
    for t in range(F_TICKS):
        pl.tick()
        pl.advance_async(model)
        got, want = pl.get_scene_in(), r["sins"][t + 1]
        worst = max(worst, float(np.abs(got["loc"]["globalpoint"]["x"] - want["loc"]["globalpoint"]["x"]).max()),
                    float(np.abs(got["loc"]["globalpoint"]["y"] - want["loc"]["globalpoint"]["y"]).max()))
        bad = compare(got, want, "scene_in")
        assert not bad, f"tick {t} (largest position difference so far {worst!r} m)\n" + "\n".join(bad[:10])
        assert pl.traffic_state().tobytes() == r["s"][t + 1].tobytes(), f"tick {t}: arc lengths"
        assert np.concatenate(_slices(pl, F_N)).tobytes() == r["pools"][t + 1].tobytes(), f"tick {t}: vehicles"
    pl.tick()
    score, want = pl.rollout_score(), r["scores"]
    print(f"largest position difference over {F_TICKS} ticks: {worst!r} m; ob_flag ticks {score['n_ob_flag'].tolist()}")
    for k, (dt_, _) in dm.RolloutScore.fields.items():
        if dt_.base.kind == "i":
            assert np.array_equal(score[k], want[k]), (k, score[k].tolist(), want[k].tolist())
    assert (score["n_ob_flag"] > 0).all() and (score["n_collision_ticks"] == 0).all() and not pl.ego_flags().any()
    pl.close()
