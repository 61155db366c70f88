"""Traffic manoeuvres in the closed loop: a vehicle cuts in front of every ego of a routed ring, and a pedestrian steps
off the kerb when the ego is three seconds away.

The CPU loop is the one of tests/test_traffic_follow.py - oracle tick + route model + traffic model - with the manoeuvre model in the
place of the traffic model, the scorecard (tests/rollout_score_model.py) and the conflict score (tests/conflict_model.py) on.  The
device is held to it as that file holds its closed loop: the staged records through parity_util.compare, the scorecard's integer
fields equal, no tolerance added.  The assertions are structural; the magnitudes the loop shows stand in DESIGN.md §4v."""
import numpy as np
import pytest

import conflict_model as cm
import route_scenes as rs
import traffic_manoeuvre_model as mm
import traffic_model as tm
import traffic_scenes as ts

gpu = pytest.mark.gpu
N, TICKS = 16, 120
GAP, DIST, STEPS = 9.0, 12.0, 20          # the vehicle starts GAP m ahead on lane 1 and cuts in once the ego is within DIST m behind it
SPEED, RADIUS, TYPE = 10.0 / 3.6, 0.9, 7          # the planner cruises the empty ring at 10 km/h
_CPU = {}


def _scene(dm):
    """16 ring egos on lane 2 (the starts of §4i's scene A: 120 .. 170 points into their first road, grid stage off, the two-lane
    road 3 left out), one own obstacle entry each: a vehicle on the lane-1 ring track GAP m ahead of the ego's abscissa at SPEED."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, 4 * N, seed=3, lanes=(2,), ids=(120, 170), legs=(6, 10), n_obs=1)
    loc = sc["scene_in"]["loc"]
    keep = np.flatnonzero((loc["road_num"] != 3) & (loc["lane_num"] == 2))[:N]
    assert len(keep) == N
    legs = np.concatenate([legs[rf[k]:rf[k + 1]] for k in keep])
    rf = np.concatenate([[0], np.cumsum([rf[k + 1] - rf[k] for k in keep])]).astype(np.int32)
    sc = dict(sc, scene_in=sc["scene_in"][keep].copy(), state=sc["state"][keep].copy(), obs_pool=np.zeros(N, dm.ObPoint), mot_pool=None)
    sc["obs_pool"]["radius"] = 0.5
    sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"] = np.arange(N), 1
    polylines = [(ts.ring_track(dm, m, 1), True), (ts.ring_track(dm, m, 2), True)]
    tracks, pts = ts.pack(dm, polylines)
    cum1 = tm.cumulative(polylines[0][0]["x"], polylines[0][0]["y"], True)
    rows = []
    for s in range(N):
        loc = sc["scene_in"]["loc"][s]
        rows.append((cum1[ts.SEG * (int(loc["road_num"]) - 1) + int(loc["id"][1])] + GAP, SPEED, s, 0, 0, TYPE, RADIUS))
    recs = mm.records(*[mm.record(a, mm.EGO_DIST, 1, dist=DIST, track=1, lat_end=0.0, n_steps=STEPS) for a in range(N)])
    return cfg, m, sc, legs, rf, tracks, pts, ts.actors(dm, rows), recs


def _cpu_loop(dm, oracle, cut_in):
    import map_scenes as ms
    import rollout_score_model as sm
    import route_model as rmod
    if cut_in in _CPU:
        return _CPU[cut_in]
    cfg, m, sc, legs, rf, tracks, pts, act, recs = _scene(dm)
    model, rm, conflict = dm.default_ego_model(), dm.default_route_model(), dm.default_conflict()
    dt = float(model["dt"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"].copy()), sc["state"].copy(), np.zeros(N, np.int32)
    tr = mm.Manoeuvres(tracks, pts, act, si["obs_off"], recs if cut_in else recs[:0])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    scores, conf, prev = sm.new_scores(dm.RolloutScore, N), cm.new_scores(dm.ConflictScore, N), cm.new_prev(dm.ObPoint)
    sins, ss, sts, ob_ticks = [si], [tr.s.copy()], [tr.st.copy()], np.zeros(N, np.int64)
    for t in range(TICKS + 1):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        prev = cm.step(conf, prev, conflict, cfg, dt, si, obs)
        sm.fold(scores, cfg, dt, si, plan, st, obs, flags)
        ob_ticks += plan["ob_flag"] != 0
        if t < TICKS:
            si, flags, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
            obs, _ = tr.advance(obs, None, dt, None, si, flags)
            sins.append(si), ss.append(tr.s.copy()), sts.append(tr.st.copy())
    _CPU[cut_in] = dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, tracks=tracks, pts=pts, act=act, recs=recs, sins=sins, s=ss, st=sts, scores=scores, conf=conf,
                        flags=flags, ob_ticks=ob_ticks)
    return _CPU[cut_in]


def _structure(st, scores_with, scores_without):
    assert st["n_done"].tolist() == [1] * N and st["track"].tolist() == [1] * N and st["lat"].tolist() == [0.0] * N and st["k"].tolist() == [0] * N
    assert any(scores_with[k].tobytes() != scores_without[k].tobytes() for k in scores_with.dtype.names), "the cut-in changes the scorecard"


def test_cut_in_closed_loop_on_the_cpu(dm, oracle):
    """Every vehicle fires once, ends on the lane-2 track with no offset, and no ego is touched; the scorecard differs from the run
    without the records.  (Figures: printed here, written into DESIGN.md §4v.)"""
    on, off = _cpu_loop(dm, oracle, True), _cpu_loop(dm, oracle, False)
    for name, r in (("cut-in", on), ("none", off)):
        print(name, "ob_flag ticks", r["ob_ticks"].tolist(), "\n  min clearance", np.round(r["scores"]["min_clearance"], 2).tolist(), "obs", r["scores"]["min_clearance_obs"].tolist(),
              "\n  min_ttc", np.round(r["conf"]["min_ttc"], 2).tolist(), "\n  collision ticks", r["scores"]["n_collision_ticks"].tolist(), "dist", np.round(r["scores"]["dist"], 1).tolist())
    fired = [next(t for t in range(TICKS + 1) if on["st"][t]["k"][a] > 0) for a in range(N)]
    print("fired at advance", fired)
    _structure(on["st"][-1], on["scores"], off["scores"])
    assert not off["st"][-1]["n_done"].any() and (off["st"][-1]["track"] == 0).all()
    assert (on["scores"]["n_collision_ticks"] == 0).all() and (on["scores"]["first_collision_tick"] == -1).all() and not on["flags"].any()


def test_pedestrian_steps_off_the_kerb_on_the_cpu(dm, oracle):
    """A parked actor on a polyline that crosses the ego's lane, EGO_TIME 3 s, speed 1.5: it stands until the ego is three seconds away at
    its own speed, then walks across; the run with the record differs from the run without it, where the pedestrian never moves."""
    import map_scenes as ms
    import route_model as rmod
    cfg, m, sc, legs, rf, _, _, _, _ = _scene(dm)
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt = float(model["dt"][0])
    si0 = ms.resolve(dm, m, sc["scene_in"].copy())
    lane2 = ts.ring_track(dm, m, 2)
    polylines, rows = [], []
    for s in range(N):          # the crossing: 4 m either side of the point 25 m (50 points) ahead of the ego, along the lane's normal there
        loc = si0["loc"][s]
        i = ts.SEG * (int(loc["road_num"]) - 1) + int(loc["id"][1]) + 50
        ax, ay, bx, by = lane2["x"][i], lane2["y"][i], lane2["x"][i + 1], lane2["y"][i + 1]
        ln = float(np.hypot(bx - ax, by - ay))
        nx, ny = -(by - ay) / ln, (bx - ax) / ln
        polylines.append((ts.polyline(dm, [(ax - 4.0 * nx + 0.5 * k * nx, ay - 4.0 * ny + 0.5 * k * ny) for k in range(17)]), False))
        rows.append((0.0, 0.0, s, 0, s, 2, 0.4))
    tracks, pts = ts.pack(dm, polylines)
    recs = mm.records(*[mm.record(a, mm.EGO_TIME, time=3.0, speed=1.5) for a in range(N)])
    out = {}
    for with_rec in (True, False):
        si, st, flags = si0.copy(), sc["state"].copy(), np.zeros(N, np.int32)
        tr = mm.Manoeuvres(tracks, pts, ts.actors(dm, rows), si["obs_off"], recs if with_rec else recs[:0])
        obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
        fired, ob_ticks = np.full(N, -1), np.zeros(N, np.int64)
        for t in range(TICKS):
            plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
            ob_ticks += plan["ob_flag"] != 0
            si, flags, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
            obs, _ = tr.advance(obs, None, dt, None, si, flags)
            fired = np.where((fired < 0) & np.array([i.fired for i in tr.minfo]), t, fired)
        out[with_rec] = (tr.s.copy(), tr.st.copy(), fired, ob_ticks)
    s, st, fired, ob = out[True]
    print("pedestrian: fired at advance", fired.tolist(), "walked", s.tolist(), "ob_flag ticks with", ob.tolist(), "without", out[False][3].tolist())
    assert (fired >= 0).all() and st["n_done"].tolist() == [1] * N and (st["v0"] == 1.5).all() and (s > 0).all()
    assert (fired > 0).all(), "nobody steps off before the ego is three seconds away"
    assert not out[False][0].any() and not out[False][1]["n_done"].any()


@gpu
def test_cut_in_closed_loop_agrees_with_the_cpu_loop(dm, oracle):
    """The cut-in scene on the device, 120 advances with the scorecard and the conflict score on, against the CPU loop: the staged
    records within parity_util.compare's bounds, the integer fields of the scorecard and of the conflict score equal; then the structure."""
    from parity_util import compare
    r, off = _cpu_loop(dm, oracle, True), _cpu_loop(dm, oracle, False)
    pl = dm.Planner(r["cfg"], device=0, **rs.caps(r["m"], N, 1, 0))
    pl.set_map(r["m"])
    pl.set_egos(r["sc"], with_motion=False)
    pl.set_state(r["sc"]["state"])
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    pl.set_traffic_manoeuvres(r["recs"].astype(dm.TrafficManoeuvre))
    pl.score_begin()
    pl.set_conflict_score(dm.default_conflict())
    model = dm.default_ego_model()
    assert pl.traffic_state().tobytes() == r["s"][0].tobytes()
    for t in range(TICKS):
        pl.tick()
        pl.advance_async(model)
        bad = compare(pl.get_scene_in(), r["sins"][t + 1], "scene_in")
        assert not bad, f"tick {t}\n" + "\n".join(bad[:10])
        st = pl.get_traffic_manoeuvre_state()
        for k in ("track", "next", "k", "clock", "n_done"):
            assert np.array_equal(st[k], r["st"][t + 1][k]), (t, k, st[k].tolist(), r["st"][t + 1][k].tolist())
    pl.tick()
    score, conf, st = pl.rollout_score(), pl.conflict_score(), pl.get_traffic_manoeuvre_state()
    pl.close()
    for got, want in ((score, r["scores"]), (conf, r["conf"])):
        for k, (dt_, _) in got.dtype.fields.items():
            if dt_.base.kind == "i":
                assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    _structure(st, score, off["scores"])
    assert (score["n_collision_ticks"] == 0).all()
