"""The perception model in the closed loop: planners read the perceived snapshot, judges the truth.

The CPU loop is the one of tests/test_traffic.py / tests/test_traffic_manoeuvre_loop.py - oracle tick + route model + traffic (manoeuvre)
model, scorecard and conflict models - with tests/perception_model.py between the truth and the oracle tick: the oracle plans on the
perceived pool, the scorecard and the conflict score fold the truth.  The device is held to it as those files hold their loops: the staged
records through parity_util.compare, the integer fields of the scorecard and of the conflict score and ALL perception counters equal.

  followers : §4h's 16 ring egos, each behind a vehicle at 1.5 m/s on its own lane.  The range is 0.9 of the smallest centre distance of
              the clean run (taken from the clean CPU run): no ego sees its vehicle before it is closer than it ever came - every ego
              comes strictly closer, and min_hidden_clearance names the vehicle's entry and type.
  cut-in    : §4v's scene, the default model with confirm = 5 and no position noise (see _cut_in_model): the first ob_flag tick is not earlier than in the clean run, and the
              conflict score - which reads the truth - has its first critical tick unchanged or earlier.

The assertions are structural; the magnitudes are printed here and stand in DESIGN.md §4w."""
import numpy as np
import pytest

import conflict_model as cm
import perception_backends as pb
import perception_model as pcm
import traffic_manoeuvre_model as mm
import traffic_model as tm

gpu = pytest.mark.gpu
_CPU = {}


def _scene(dm, kind):
    import test_traffic as tt
    import test_traffic_manoeuvre_loop as tml
    if kind == "followers":
        cfg, m, sc, legs, rf, tracks, pts, act = tt._followers(dm)
        raw = sc["scene_in"].copy()
        raw["obs_n"] = 1
        return dict(cfg=cfg, m=m, sc=dict(sc, scene_in=raw), legs=legs, rf=rf, tracks=tracks, pts=pts, act=act, recs=None, n=tt.F_N, ticks=tt.F_TICKS, type=tt.F_TYPE)
    cfg, m, sc, legs, rf, tracks, pts, act, recs = tml._scene(dm)
    return dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, tracks=tracks, pts=pts, act=act, recs=recs, n=tml.N, ticks=tml.TICKS, type=tml.TYPE)


def _cpu_loop(dm, oracle, kind, pm):
    """pm None: the clean run.  Returns the scene and, per tick, the staged records; the records of the three judges; per ego the first
    ob_flag tick (-1: never) and the smallest centre distance to its vehicle."""
    import map_scenes as ms
    import rollout_score_model as sm
    import route_model as rmod
    key = (kind, None if pm is None else np.array(pm).tobytes())
    if key in _CPU:
        return _CPU[key]
    r = _scene(dm, kind)
    cfg, sc, n, ticks = r["cfg"], r["sc"], r["n"], r["ticks"]
    model, rm, conflict = dm.default_ego_model(), dm.default_route_model(), dm.default_conflict()
    dt = float(model["dt"][0])
    si, st, flags = ms.resolve(dm, r["m"], sc["scene_in"].copy()), sc["state"].copy(), np.zeros(n, np.int32)
    tr = tm.Traffic(r["tracks"], r["pts"], r["act"], si["obs_off"]) if r["recs"] is None else mm.Manoeuvres(r["tracks"], r["pts"], r["act"], si["obs_off"], r["recs"])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    scores, conf, prev = sm.new_scores(dm.RolloutScore, n), cm.new_scores(dm.ConflictScore, n), cm.new_prev(dm.ObPoint)
    tracks, pstats = pcm.new_tracks(dm.PerceptTrack, len(obs)), pcm.new_stats(dm.PerceptionStats, n)
    sins, first_ob, centre = [si], np.full(n, -1), np.full(n, np.inf)
    for t in range(ticks + 1):
        seen = obs if pm is None else pcm.step(tracks, pstats, pm, cfg, t + 1, si, obs)[0]
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=seen, mot_pool=None), st, n_threads=8, want_grid=False)
        prev = cm.step(conf, prev, conflict, cfg, dt, si, obs)          # the judges read the truth
        sm.fold(scores, cfg, dt, si, plan, st, obs, flags)
        first_ob = np.where((first_ob < 0) & (plan["ob_flag"] != 0), t, first_ob)
        g, o = si["loc"]["globalpoint"], obs[si["obs_off"]]
        centre = np.minimum(centre, np.hypot(o["x"] - g["x"], o["y"] - g["y"]))
        if t < ticks:
            si, flags, _ = rmod.advance(dm, cfg, model, rm, r["legs"], r["rf"], r["m"], si, plan, st, flags)
            obs, _ = tr.place(obs, None, dt) if r["recs"] is None else tr.advance(obs, None, dt, None, si, flags)
            sins.append(si)
    _CPU[key] = dict(r, sins=sins, scores=scores, conf=conf, pstats=pstats, first_ob=first_ob, centre=centre, s0=tr.s.copy())
    return _CPU[key]


def _followers_model(dm, oracle):
    clean = _cpu_loop(dm, oracle, "followers", None)
    return clean, pb.model(range=0.9 * float(clean["centre"].min()))


def _cut_in_model(dm):
    """The default model with confirm = 5 and the position noise off.  "Not earlier than in the clean run" is a statement about the
    confirmation alone: with the default noise (0.1 m + 0.005 d) a report can stand inside the corridor one tick before the vehicle does -
    on the CPU loop one ego of the 16 is flagged on tick 12 against 13 - which is the noise at work, not a track confirmed early."""
    pm = dm.default_perception()
    pm["confirm"], pm["sigma0"], pm["sigma_gain"] = 5, 0.0, 0.0
    return pm


def _check_followers(clean, r):
    n = r["n"]
    assert (r["centre"] < clean["centre"]).all(), "every ego comes strictly closer than in the clean run"
    assert r["pstats"]["min_hidden_obs"].tolist() == [0] * n and r["pstats"]["min_hidden_type"].tolist() == [r["type"]] * n
    assert (r["pstats"]["n_hidden"] > 0).all() and (r["pstats"]["n_fresh"] > 0).all(), "hidden first, seen once inside the range"
    assert (r["first_ob"] >= clean["first_ob"]).all() and (clean["first_ob"] >= 0).all()


def _never_is_last(a):
    return np.where(a < 0, np.iinfo(np.int64).max, a)


def _check_cut_in(clean, r):
    assert (_never_is_last(r["first_ob"]) >= _never_is_last(clean["first_ob"])).all(), "the first ob_flag tick is not earlier than in the clean run"
    assert (_never_is_last(r["conf"]["first_crit_tick"]) <= _never_is_last(clean["conf"]["first_crit_tick"])).all(), "the first critical tick: unchanged or earlier"
    st = r["pstats"]
    assert (st["n_out"] + st["n_occluded"] + st["n_missed"] + st["n_detected"] == st["n_entries"]).all() and (st["n_entries"] == r["ticks"] + 1).all()


def test_followers_see_their_vehicle_late_on_the_cpu(dm, oracle):
    clean, pm = _followers_model(dm, oracle)
    r = _cpu_loop(dm, oracle, "followers", pm)
    print("range", float(pm["range"][0]), "\nclean: smallest centre distance", np.round(clean["centre"], 2).tolist(), "first ob_flag tick", clean["first_ob"].tolist(),
          "\nperceived: smallest centre distance", np.round(r["centre"], 2).tolist(), "first ob_flag tick", r["first_ob"].tolist(),
          "\nmin_hidden_clearance", np.round(r["pstats"]["min_hidden_clearance"], 2).tolist(), "collision ticks", r["scores"]["n_collision_ticks"].tolist())
    _check_followers(clean, r)


def test_cut_in_confirmed_late_on_the_cpu(dm, oracle):
    clean, r = _cpu_loop(dm, oracle, "cut-in", None), _cpu_loop(dm, oracle, "cut-in", _cut_in_model(dm))
    print("clean: first ob_flag tick", clean["first_ob"].tolist(), "first_crit_tick", clean["conf"]["first_crit_tick"].tolist(), "min_ttc", np.round(clean["conf"]["min_ttc"], 2).tolist(),
          "\nconfirm 5: first ob_flag tick", r["first_ob"].tolist(), "first_crit_tick", r["conf"]["first_crit_tick"].tolist(), "min_ttc", np.round(r["conf"]["min_ttc"], 2).tolist(),
          "\nmin clearance clean", np.round(clean["scores"]["min_clearance"], 2).tolist(), "confirm 5", np.round(r["scores"]["min_clearance"], 2).tolist())
    _check_cut_in(clean, r)


def _device_loop(dm, r, pm):
    """The scene on the device with the model set; returns (scorecard, conflict score, perception stats)."""
    import route_scenes as rs
    from parity_util import compare
    pl = dm.Planner(r["cfg"], device=0, **rs.caps(r["m"], r["n"], 1, 0))
    pl.set_map(r["m"])
    pl.set_egos(r["sc"], with_motion=False)
    pl.set_state(r["sc"]["state"])
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    if r["recs"] is not None:
        pl.set_traffic_manoeuvres(r["recs"].astype(dm.TrafficManoeuvre))
    pl.score_begin()
    pl.set_conflict_score(dm.default_conflict())
    pl.set_perception(pm)
    model = dm.default_ego_model()
    for t in range(r["ticks"]):
        pl.tick()
        pl.advance_async(model)
        bad = compare(pl.get_scene_in(), r["sins"][t + 1], "scene_in")
        assert not bad, f"tick {t}\n" + "\n".join(bad[:10])
    pl.tick()
    out = pl.rollout_score(), pl.conflict_score(), pl.perception_stats()
    pl.close()
    for got, want in ((out[0], r["scores"]), (out[1], r["conf"]), (out[2], r["pstats"])):
        for k, (dt_, _) in got.dtype.fields.items():
            if dt_.base.kind == "i":
                assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    return out


@gpu
def test_followers_loop_agrees_with_the_cpu_loop(dm, oracle):
    clean, pm = _followers_model(dm, oracle)
    r = _cpu_loop(dm, oracle, "followers", pm)
    score, _, st = _device_loop(dm, r, pm)
    assert st["min_hidden_obs"].tolist() == [0] * r["n"] and st["min_hidden_type"].tolist() == [r["type"]] * r["n"]
    assert (score["min_clearance"] < clean["scores"]["min_clearance"]).all(), "the scorecard, which reads the truth, shows every ego closer than in the clean run"


@gpu
def test_cut_in_loop_agrees_with_the_cpu_loop(dm, oracle):
    pm = _cut_in_model(dm)
    clean, r = _cpu_loop(dm, oracle, "cut-in", None), _cpu_loop(dm, oracle, "cut-in", pm)
    _, conf, _ = _device_loop(dm, r, pm)
    assert (_never_is_last(conf["first_crit_tick"]) <= _never_is_last(clean["conf"]["first_crit_tick"])).all()
