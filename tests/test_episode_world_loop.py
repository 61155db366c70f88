"""World episodes with the world traffic reset in closed loop (pp_set_episode_worlds, pp_set_episode_world_traffic).

The set-up is §4j's platoon (tests/test_world_traffic.py): worlds of routed ring egos 15 m apart with 4 peer slots and ONE shared vehicle
per world, here turned round to drive towards its world as §4l's followers have it (speed -3 m/s: it steps as §4h whether following is on
or not).  contact = 1: the front ego meets the vehicle, its episode ends with CONTACT, and with world episodes its partner's ends on the
same advance with exactly DMPP_EGO_WORLD; both restart on the captured records and the world reset puts the vehicle back on set 0, so
every later world episode repeats the first byte for byte.

CPU: the loop of oracle tick + route model + world-episode model + world-traffic model + world reset + fleet model, its structure, and
the control run with world episodes off.  GPU: the device against that loop on every advance (SceneIn every byte but an advanced
heading, flags, s, v, the integer stats, the counters), on the platoons with following on and off, and on worlds of 1 | 2 | 65 members
with n_sets = M; pp_rollout against its parts; the error paths and the life cycle of both set calls."""
import numpy as np
import pytest

import episode_model as epm
import episode_spawn_backends as esb
import episode_spawn_model as esm
import episode_world_model as ewm
import fleet_model as fl
import map_scenes as ms
import route_model as rmod
import route_scenes as rs
import test_episodes as te
import test_world_traffic as twt
import traffic_scenes as ts
import world_traffic_model as wm

gpu = pytest.mark.gpu
WORLD, CONTACT = 256, 128
V_SPEED, V_RADIUS, V_TYPE = -3.0, 0.9, 7
_CPU, _DEV = {}, {}

# name: (worlds as (leader, members) - members > 0: a platoon 15 m apart; members < 0: that many egos on ONE pose, no peer slots -, peer slots, gap of
# the vehicle in front of the front ego - negative: BEHIND the rear ego -, following, M, advances, the vehicle's speed, max_ticks, the advance in
# front of which pp_set_episode_world_traffic is called)
SETUPS = {
    "platoons": (2, 2, 4, 30.0, True, 1, 200, -3.0, 0, 0),
    "platoons_move": (2, 2, 4, 30.0, False, 1, 80, -3.0, 0, 0),
    "sizes": (3, (1, 2, 65), 0, 8.0, True, 3, 90, -3.0, 0, 0),
    "near": (2, 2, 4, 8.0, False, 1, 40, -3.0, 0, 0),
    # §4j's chased platoons: the vehicle 12 m behind the rear ego wants 6 m/s and follows (speed > 0: v' = v* of §4t 3.); every world ends on
    # TIMEOUT.  The reset is set 10 advances into the run, so the v captured into set 0 is the car-following v of that moment, not the speed
    "chased": (2, 2, 4, -12.0, True, 1, 100, 6.0, 30, 10),
    "chased_sets": (2, 2, 4, -12.0, True, 3, 100, 6.0, 30, 10),
}


def _scene(dm, name):
    leaders, size, K, gap, follow, M, ticks, speed, max_ticks, warm = SETUPS[name]
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    if isinstance(size, int):
        sc, legs, rf, wf, off, polylines, rows = twt._platoons(dm, cfg, m, leaders, size, 1, K)
        front = 15.0 * (size - 1)
    else:                                                                      # every leader alone, then `size[w]` copies of it on its pose
        sc, legs, rf, wf, off, polylines, rows = twt._platoons(dm, cfg, m, leaders, 1, 1, K)
        idx = np.repeat(np.arange(leaders), size)
        n = len(idx)
        si = sc["scene_in"][idx].copy()
        off = np.arange(n, dtype=np.int64) * (1 + K)
        si["obs_off"] = off
        legs = np.concatenate([legs[rf[k]:rf[k + 1]] for k in idx])
        rf = np.concatenate([[0], np.cumsum([rf[k + 1] - rf[k] for k in idx])]).astype(np.int32)
        pool = np.concatenate([sc["obs_pool"][:1 + K]] * n)
        sc = dict(sc, scene_in=si, state=sc["state"][idx].copy(), obs_pool=pool, n_obs=1 + K)
        wf, front = np.concatenate([[0], np.cumsum(size)]).astype(np.int32), 0.0
    tracks, pts = ts.pack(dm, polylines)
    act = ts.actors(dm, [(here + (front + gap if gap > 0 else gap), speed, w, 0, lane - 1, V_TYPE, V_RADIUS) for w, lane, here in rows])
    fmod = dm.default_fleet_model()
    fmod["max_peers"] = K
    sp = esb.neutral(dm.EpisodeSpawn)
    sp["contact"], sp["n_starts"], sp["order"] = 1, M, 1
    n = len(sc["scene_in"])
    starts, tstarts = None, None
    if M > 1:                                                                  # the records of every index are the capture's; the vehicles' sets differ: 4 m further away per index
        starts = (np.concatenate([sc["scene_in"]] * (M - 1)), np.concatenate([sc["state"]] * (M - 1)))
        tstarts = np.zeros((M - 1) * len(act), dm.TrafficStart)
        tstarts["s"] = np.concatenate([act["s0"] + (4.0 if gap > 0 else -4.0) * k for k in range(1, M)])
        tstarts["v"] = np.repeat(2.0 + np.arange(1, M), len(act))
    return dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, wf=wf, off=off, own=np.ones(n, np.int64), tracks=tracks, pts=pts, act=act, fmod=fmod, K=K,
                em=te._em(dm, 31, max_ticks), sp=sp, follow=follow, M=M, ticks=ticks, n=n, starts=starts, tstarts=tstarts, warm=warm)


def _cpu_loop(dm, oracle, name, worlds=True):
    """sins[t], flags[t], s[t], v[t]: what tick t reads; causes[t]: the cause words of the advance behind tick t."""
    if (name, worlds) in _CPU:
        return _CPU[name, worlds]
    r = _scene(dm, name)
    cfg, m, sc, n, wf, off, own, M = r["cfg"], r["m"], r["sc"], r["n"], r["wf"], r["off"], r["own"], r["M"]
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt, width = float(model["dt"][0]), float(cfg["Vehicle_Width"][0])
    tr = wm.World(r["tracks"], r["pts"], r["act"], wf, off, own)
    si, st, flags = ms.resolve(dm, m, sc["scene_in"].copy()), sc["state"].copy(), np.zeros(n, np.int32)
    si, obs, _ = fl.couple(r["fmod"], wf, off, own, si, sc["obs_pool"].copy())
    obs, _ = tr.place(obs, None, 0.0)
    # pp_set_episodes captures the resident records as they stand: coupled; start records k >= 1 are resolved and take record 0's slice
    pin, pst = [si.copy()], [st.copy()]
    for k in range(1, M):
        rec = ms.resolve(dm, m, r["starts"][0][(k - 1) * n:k * n].copy())
        rec["obs_off"], rec["obs_n"] = si["obs_off"], si["obs_n"]
        pin.append(rec), pst.append(r["starts"][1][(k - 1) * n:k * n].copy())
    stats, sstats = epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n)
    reset = None
    out = dict(r, sins=[si], flags=[flags], s=[tr.s.copy()], v=[tr.v.copy()], causes=[])
    for t in range(r["ticks"]):
        if worlds and t == r["warm"]:                                          # pp_set_episode_world_traffic: set 0 is captured from the traffic as it stands
            reset = ewm.WorldReset(tr, M, r["tstarts"], follow=r["follow"])
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        q, f, _ = rmod.advance(dm, cfg, model, rm, r["legs"], r["rf"], m, si, plan, st, flags)
        if worlds:
            si, st, flags, _, c = ewm.step(r["em"], r["sp"], stats, sstats, pin, pst, si, q, f, st, obs, 0.5 * width, wf, (off, own))
        else:
            si, st, flags, _, c = esm.step(r["em"], r["sp"], stats, sstats, pin, pst, si, q, f, st, obs, 0.5 * width, wf)
        if r["follow"]:
            obs, _ = tr.step(obs, None, dt, None, si, flags, width)
        else:
            obs, _ = tr.place(obs, None, dt)
        if reset is not None:
            obs, _ = reset.step(tr, obs, None, stats["age"], sstats["cur_start"], wf)
        si, obs, _ = fl.couple(r["fmod"], wf, off, own, si, obs)
        out["sins"].append(si), out["flags"].append(flags), out["s"].append(tr.s.copy()), out["v"].append(tr.v.copy()), out["causes"].append(c)
    out.update(causes=np.array(out["causes"]), stats=stats, sstats=sstats, n_resets=None if reset is None else reset.n_resets.copy(), reset=reset)
    _CPU[name, worlds] = out
    return out


def _episodes(causes, a, b):
    """The advances on which world [a, b) ended."""
    return np.flatnonzero(causes[:, a:b].any(axis=1)).tolist()


def test_platoons_restart_together_and_replay_on_the_cpu(dm, oracle):
    r = _cpu_loop(dm, oracle, "platoons")
    causes, stats, wf = r["causes"], r["stats"], r["wf"]
    print("episodes", stats["n_episodes"].tolist(), "ages", stats["min_age"].tolist(), stats["max_age"].tolist(), "contacts", r["sstats"]["n_contact"].tolist(),
          "resets", r["n_resets"].tolist())
    for w, (a, b) in enumerate(zip(wf[:-1], wf[1:])):
        ends = _episodes(causes, a, b)
        assert len(ends) >= 3, (w, ends)
        for t in ends:
            # both members end on the same advance: the touched ego with CONTACT, its partner with exactly 256
            assert sorted(causes[t, a:b].tolist()) == [CONTACT, WORLD], (w, t, causes[t, a:b].tolist())
        assert (stats["min_age"][a:b] == stats["max_age"][a:b]).all() and (stats["n_episodes"][a:b] == len(ends)).all()
        assert int(r["n_resets"][w]) == len(ends) and not stats["n_end"][a:b].any()
        # every later world episode stages the SceneIn sequence of both members and the vehicle's (s, v) sequence of the first, byte for byte
        first, age = ends[0] + 1, int(stats["min_age"][a])
        for t0 in ends[:-1]:
            for j in range(age):
                assert r["sins"][t0 + 1 + j][a:b].tobytes() == r["sins"][j][a:b].tobytes(), (w, t0, j)
                assert r["s"][t0 + 1 + j][w] == r["s"][j][w] and r["v"][t0 + 1 + j][w] == r["v"][j][w], (w, t0, j)
        assert first == age
    # the worlds started elsewhere on the ring: they do not end on the same advances
    assert _episodes(causes, 0, 2) != _episodes(causes, 2, 4)


def test_control_without_world_episodes_does_not_repeat(dm, oracle):
    """pp_set_episode_worlds off: only the touched ego restarts, its partner drives on, the vehicle is never put back: no later episode
    repeats the first."""
    r = _cpu_loop(dm, oracle, "platoons", worlds=False)
    causes, stats = r["causes"], r["stats"]
    assert set(causes[causes != 0].tolist()) == {CONTACT}
    for a in (0, 2):
        ends = _episodes(causes, a, a + 2)
        assert ends and not (causes[ends[0], a:a + 2] != 0).all()              # only the touched ego ended
        t0, touched = ends[0], a + int(np.flatnonzero(causes[ends[0], a:a + 2])[0])
        assert r["s"][t0 + 2][a // 2] != r["s"][1][a // 2]                     # the vehicle stays where the episode left it
        assert any(r["sins"][t0 + 1 + j][touched].tobytes() != r["sins"][j][touched].tobytes() for j in range(1, min(10, r["ticks"] - t0)))


def test_sizes_loop_restarts_every_member_on_the_cpu(dm, oracle):
    """Worlds of 1 | 2 | 65 egos on one pose each, M = 3 round robin with the vehicles' sets 4 m further away per index: every member touches on
    the same advance (CONTACT, with WORLD beside it but in the world of one), cur_start cycles and the vehicle goes to the set it names."""
    r = _cpu_loop(dm, oracle, "sizes")
    causes, wf, act = r["causes"], r["wf"], r["act"]
    for w, (a, b) in enumerate(zip(wf[:-1], wf[1:])):
        ends = _episodes(causes, a, b)
        assert len(ends) >= 3, (w, ends)
        for e, t in enumerate(ends):
            assert set(causes[t, a:b].tolist()) == {CONTACT | (WORLD if b - a > 1 else 0)}
            k = (e + 1) % 3
            assert float(r["s"][t + 1][w]) == float(act["s0"][w]) + 4.0 * k
        assert int(r["n_resets"][w]) == len(ends)


@pytest.mark.parametrize("name", ["chased", "chased_sets"])
def test_chased_vehicles_take_v_of_their_set_on_the_cpu(dm, oracle, name):
    """Following on, speed > 0: a restarted world's vehicle takes v' = v* of its set (§4t 3.).  Set 0 was captured 10 advances into the run: its v
    is the car-following v of that moment, which is not the speed; sets 1 and 2 carry v = 3 and 4.  Every world ends on TIMEOUT, both members
    with a cause of their own: 64 | 256."""
    r = _cpu_loop(dm, oracle, name)
    causes, wf, reset, M = r["causes"], r["wf"], r["reset"], r["M"]
    assert (reset.v[0] != r["act"]["speed"]).all() and (reset.v[0] > 0).all(), reset.v[0].tolist()
    for w, (a, b) in enumerate(zip(wf[:-1], wf[1:])):
        ends = _episodes(causes, a, b)
        assert ends == [29, 59, 89], ends
        for e, t in enumerate(ends):
            assert causes[t, a:b].tolist() == [64 | WORLD] * 2
            k = (e + 1) % M
            assert r["v"][t + 1][w] == reset.v[k][w] and r["s"][t + 1][w] == reset.s[k][w] and r["v"][t][w] != r["v"][t + 1][w], (w, e)
        assert int(r["n_resets"][w]) == 3
    if M > 1:
        assert reset.v[1].tolist() == [3.0, 3.0] and reset.v[2].tolist() == [4.0, 4.0]


# ---------------------------------------------------------------------------------------------------------------
# GPU
def _planner(dm, r, worlds=True, reset=True):
    pl = dm.Planner(r["cfg"], device=0, **rs.caps(r["m"], r["n"], 1 + r["K"], 0))
    pl.set_map(r["m"])
    pl.set_egos(r["sc"], with_motion=False)
    pl.set_state(r["sc"]["state"])
    pl.set_route(r["legs"], r["rf"])
    pl.set_fleet(r["wf"], r["fmod"])
    if r["follow"]:
        pl.set_traffic_follow(dm.default_traffic_follow())
    pl.set_world_traffic(r["tracks"], r["pts"], r["act"])
    pl.set_episodes(r["em"])
    pl.set_episode_spawn(r["sp"], *(r["starts"] if r["starts"] is not None else (None, None)))
    if worlds:
        pl.set_episode_worlds()
        if reset:
            pl.set_episode_world_traffic(r["M"], r["tstarts"])
    return pl


def _speeds(pl, r):
    return pl.traffic_speed() if r["follow"] else np.ascontiguousarray(r["act"]["speed"], np.float64).copy()


def _last(pl, r):
    return (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), pl.episode_stats(), pl.episode_spawn_stats(), pl.traffic_state(), _speeds(pl, r),
            pl.episode_world_traffic_resets())


_LAST = ("PlanOut", "SceneState", "flags", "SceneIn", "EpisodeStats", "EpisodeSpawnStats", "s", "v", "n_resets")


def _device_loop(dm, oracle, name):
    if name in _DEV:
        return _DEV[name]
    r = _cpu_loop(dm, oracle, name)
    pl, model = _planner(dm, r, reset=r["warm"] == 0), dm.default_ego_model()
    run = dict(sins=[pl.get_scene_in()], flags=[np.zeros(r["n"], np.int32)], s=[pl.traffic_state()], v=[_speeds(pl, r)])
    for t in range(r["ticks"]):
        pl.tick()
        if r["warm"] and t == r["warm"]:                                       # (behind the tick that adopted the last advance: nothing is staged)
            pl.set_episode_world_traffic(r["M"], r["tstarts"])
        pl.advance_async(model)
        run["sins"].append(pl.get_scene_in()), run["flags"].append(pl.ego_flags()), run["s"].append(pl.traffic_state()), run["v"].append(_speeds(pl, r))
    pl.tick()
    pl.sync()
    run["last"] = _last(pl, r)
    pl.close()
    _DEV[name] = run
    return run


@gpu
@pytest.mark.parametrize("name", ["platoons", "platoons_move", "sizes", "chased", "chased_sets"])
def test_device_agrees_with_the_cpu_loop(dm, oracle, name):
    """Every advance of the device against the CPU loop: the staged records - every byte but an advanced heading -, the flag words, s and v of
    every vehicle (a vehicle of a world that went on: as the traffic kernel wrote it; of a world that restarted: on its start state), and at
    the end the integer stats, the spawn-stats words and the reset counters."""
    r, d = _cpu_loop(dm, oracle, name), _device_loop(dm, oracle, name)
    for t in range(r["ticks"] + 1):
        assert np.array_equal(d["flags"][t], r["flags"][t]), f"set {t}: flags"
        te._assert_records(d["sins"][t], r["sins"][t], f"set {t}")
        assert d["s"][t].tobytes() == r["s"][t].tobytes(), f"set {t}: s {d['s'][t].tolist()} against {r['s'][t].tolist()}"
        assert d["v"][t].tobytes() == r["v"][t].tobytes(), f"set {t}: v"
    got, sgot = d["last"][4], d["last"][5]
    for f in te._INT_FIELDS:
        assert np.array_equal(got[f], r["stats"][f]), f
    for f in ("n_contact", "n_blocked", "n_rejected", "cur_start", "n_used"):
        assert np.array_equal(sgot[f], r["sstats"][f]), f
    assert np.array_equal(d["last"][8], r["n_resets"]) and (r["n_resets"] >= 1).all()
    assert (got["min_age"] == got["max_age"]).all() or name == "sizes"


@gpu
def test_the_score_trace_marks_the_start_of_every_member(dm, oracle):
    """The score trace (§4o) behind world episodes, on the platoons with the vehicle 8 m ahead: rings that never freeze (trigger 0), 40 ticks.
    The trace model is stepped over the device's own per-tick records and the device's headers and rings must equal it on every tick
    (tests/test_score_trace.py::_follow); and the tick behind an advance that ended a world carries DMPP_TICK_START in the ring of EVERY
    member - the touched ego and the partner that ended with exactly 256 -, and no other tick but the first does.  The RolloutScore records
    equal the scorecard model folded over the same per-tick records, every byte (a restart moves last_pos / last_speed to the start record)."""
    import rollout_score_model as rsm
    import score_trace_backends as stb
    import score_trace_model as stm
    import test_score_trace as tst
    r = _cpu_loop(dm, oracle, "near")
    n, ticks, adv = r["n"], r["ticks"], dm.default_ego_model()
    model = tst._tm(dm, depth=64, post=2, trigger=0)
    pl = _planner(dm, r)
    pl.set_score_trace(model)
    pl.score_begin(float(adv["dt"][0]))
    scores, (rings, info) = rsm.new_scores(dm.RolloutScore, n), stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, 64)
    recs = tst._follow(dm, pl, r["cfg"], model, n, ticks, rings, info, scores, adv, True)
    last, (_, got_rings), got_score = pl.episode_stats(), stb.read_all(pl, n), pl.rollout_score()
    pl.close()
    assert got_score.tobytes() == scores.tobytes(), "the scorecard words of every member, every byte, behind 40 scored ticks and the world restarts among them"
    ended = np.array([recs[t + 1]["stats"]["n_episodes"] > recs[t]["stats"]["n_episodes"] for t in range(ticks - 1)])          # [t, s]: the advance behind tick t ended scene s
    assert np.array_equal(ended, r["causes"][:ticks - 1] != 0) and ended.any(axis=0).all()
    assert sorted(last["last_cause"][:2].tolist()) == sorted(last["last_cause"][2:].tolist()) == [CONTACT, WORLD]
    for s in range(n):
        ring = got_rings[s]
        assert ring["k"].tolist() == list(range(ticks))
        start = (ring["marks"] & stm.TICK_START) != 0
        assert np.flatnonzero(start).tolist() == [0] + (np.flatnonzero(ended[:, s]) + 1).tolist(), (s, np.flatnonzero(start).tolist())


@gpu
def test_rollout_gives_the_bytes_of_its_parts(dm, oracle):
    r, d = _cpu_loop(dm, oracle, "platoons_move"), _device_loop(dm, oracle, "platoons_move")
    pl = _planner(dm, r)
    last = pl.rollout(r["ticks"])
    pl.sync()
    got = _last(pl, r)
    pl.close()
    assert last == r["ticks"] + 1
    for a, b, what in zip(got, d["last"], _LAST):
        assert a.tobytes() == b.tobytes(), what


@gpu
def test_control_on_the_device(dm, oracle):
    """World episodes off on the same handle set-up: the world reset is refused, only touched egos restart - the bytes of the control loop."""
    r = _cpu_loop(dm, oracle, "platoons", worlds=False)
    pl = _planner(dm, r, worlds=False)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_world_traffic(1)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.episode_world_traffic_resets()
    pl.rollout(r["ticks"])
    pl.sync()
    got = pl.episode_stats()
    for f in te._INT_FIELDS:
        assert np.array_equal(got[f], r["stats"][f]), f
    assert pl.traffic_state().tobytes() == r["s"][-1].tobytes()
    assert not (got["last_cause"] & WORLD).any()
    pl.close()


@gpu
def test_per_scene_traffic_resets_in_every_member(dm, oracle):
    """Per-scene traffic (one copy of the vehicle in every member scene) with §4m's reset behind world episodes: the front ego touches its
    copy, the world restarts, and the actors of BOTH members go back - the reset keys on age == 0, which every member of the world now has."""
    r = _cpu_loop(dm, oracle, "platoons_move")
    act = np.repeat(r["act"], 2)
    act["scene"] = np.arange(4)
    pl = _planner(dm, r, worlds=False)
    pl.set_traffic(r["tracks"], r["pts"], act)
    pl.set_episode_worlds()
    pl.set_episode_traffic(1)
    pl.rollout(r["ticks"])
    pl.sync()
    st, n = pl.episode_stats(), pl.episode_traffic_resets()
    assert (st["n_episodes"] > 0).all() and np.array_equal(n, st["n_episodes"]), (st["n_episodes"].tolist(), n.tolist())
    assert sorted(st["last_cause"][:2].tolist()) == sorted(st["last_cause"][2:].tolist()) == [CONTACT, WORLD]
    pl.close()


def _behaves(pl, ticks=45):
    """(a member of a world of several ended with the WORLD bit, the reset counters went up) over the next advances, in which something
    must end."""
    before = pl.episode_stats()["n_episodes"].copy()
    c0 = pl.episode_world_traffic_resets().copy()
    pl.rollout(ticks)
    pl.sync()
    st = pl.episode_stats()
    ended = st["n_episodes"] > before
    assert ended.any(), "the probe is too short: nothing ended"
    return bool((st["last_cause"][ended] & WORLD).any()), bool((pl.episode_world_traffic_resets() > c0).any())


def _worlds_on(dm, pl):
    """World episodes are on iff the world reset is accepted (world traffic on): the call switches the reset on."""
    try:
        pl.set_episode_world_traffic(1)
        return True
    except dm.PlannerError as e:
        assert "error -4:" in str(e)
        return False


@gpu
def test_error_paths_change_nothing(dm, oracle):
    r = _cpu_loop(dm, oracle, "sizes")
    M, bad = r["M"], r["tstarts"].copy()
    # the spawn model off
    pl = _planner(dm, r, worlds=False)
    pl.set_episode_spawn(None)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_worlds()
    pl.close()
    # a schedule in force refuses world episodes; world episodes refuse a schedule
    sp0 = r["sp"].copy()
    sp0["order"] = 0
    pl = _planner(dm, dict(r, sp=sp0), worlds=False)
    pl.set_episode_schedule(dm.default_episode_schedule())
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_worlds()
    pl.set_episode_schedule(off=True)
    pl.set_episode_worlds()
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_schedule(dm.default_episode_schedule())
    pl.set_episode_world_traffic(M, r["tstarts"])
    assert _behaves(pl) == (True, True)                                        # (the refused schedule changed nothing)
    pl.close()
    # the world reset: a bad n_sets / s / v, world episodes off, per-scene traffic in the place of world traffic; a staged update
    pl, ref = _planner(dm, r), _planner(dm, r)
    for n_sets, st in ((2, r["tstarts"][:len(r["act"])]), (-1, None), (M, None)):
        with pytest.raises((dm.PlannerError, ValueError)):
            pl.set_episode_world_traffic(n_sets, st)
    for field, v in (("s", np.nan), ("s", np.inf), ("v", -1.0), ("v", np.nan)):
        bad[:] = r["tstarts"]
        bad[field][1] = v
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_episode_world_traffic(M, bad)
    for p in (pl, ref):
        p.tick()
        p.advance_async()
    for call in (lambda: pl.set_episode_worlds(False), lambda: pl.set_episode_worlds(), lambda: pl.set_episode_world_traffic(M, r["tstarts"]),
                 lambda: pl.set_episode_world_traffic(0)):
        with pytest.raises(dm.PlannerError, match="error -4:"):               # an update is staged
            call()
    for p in (pl, ref):
        p.tick()
        p.rollout(50)
        p.sync()
    for a, b, what in zip(_last(pl, r), _last(ref, r), _LAST):
        assert a.tobytes() == b.tobytes(), what                                # none of it changed anything: the run goes on like the reference run
    assert (pl.episode_world_traffic_resets() > 0).all()
    ref.close()
    pl.set_episode_worlds(False)
    with pytest.raises(dm.PlannerError, match="error -4:"):                    # world episodes off
        pl.set_episode_world_traffic(1)
    pl.set_episode_worlds()
    pl.set_world_traffic()                                                     # no world traffic
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_world_traffic(1)
    pl.close()


@gpu
def test_a_refused_spawn_model_puts_world_episodes_and_the_reset_back(dm, oracle):
    """pp_set_episode_spawn retires world episodes and the world reset before it knows whether its records are on the map; a start record off
    the map is refused and both are back: the run goes on like the reference run, byte for byte, and the reset goes on counting."""
    r = _scene(dm, "sizes")
    pl, ref = _planner(dm, r), _planner(dm, r)
    off_map = (r["starts"][0].copy(), r["starts"][1])
    off_map[0]["loc"]["road_num"][r["n"] + 3] = 99
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_episode_spawn(r["sp"], *off_map)
    c0 = pl.episode_world_traffic_resets().copy()
    for p in (pl, ref):
        p.rollout(40)
        p.sync()
    for a, b, what in zip(_last(pl, r), _last(ref, r), _LAST):
        assert a.tobytes() == b.tobytes(), what
    ref.close()
    assert (pl.episode_world_traffic_resets() > c0).all()
    assert _worlds_on(dm, pl)
    pl.close()


@gpu
@pytest.mark.parametrize("call", ["spawn", "episodes", "fleet", "world_traffic", "follow", "egos", "worlds_off"])
def test_life_cycle(dm, oracle, call):
    """What each set call leaves (§4s, §4t): world episodes go with the spawn model; the world reset goes with everything its table was
    captured from and with pp_set_episode_worlds(h, 0); its counters stay readable."""
    r = _cpu_loop(dm, oracle, "sizes")
    pl = _planner(dm, r)
    pl.rollout(40)
    pl.sync()
    counted = pl.episode_world_traffic_resets()
    assert (counted > 0).all()
    starts = r["starts"]
    if call == "spawn":
        pl.set_episode_spawn(r["sp"], *starts)
        want = (False, False)
    elif call == "episodes":
        pl.set_episodes(r["em"])
        with pytest.raises(dm.PlannerError, match="error -4:"):               # the spawn model went with it
            pl.set_episode_worlds()
        pl.set_episode_spawn(r["sp"], *starts)
        want = (False, False)
    elif call == "fleet":
        # other worlds while world episodes stay on: the next advance follows them (the reset went with world traffic, which went with the fleet)
        pl.set_fleet(np.array([0, 3, r["n"]], np.int32), r["fmod"])
        act = r["act"][:2].copy()
        pl.set_world_traffic(r["tracks"], r["pts"], act)
        want = (True, False)
    elif call == "world_traffic":
        pl.set_world_traffic(r["tracks"], r["pts"], r["act"])
        want = (True, False)
    elif call == "follow":
        pl.set_traffic_follow(dm.default_traffic_follow())
        want = (True, False)
    elif call == "egos":
        pl.set_egos(r["sc"], with_motion=False)
        pl.set_state(r["sc"]["state"])
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.set_episode_worlds()
        assert pl.episode_world_traffic_resets().tobytes() == counted.tobytes()
        pl.close()
        return
    else:
        pl.set_episode_worlds(False)
        want = (False, False)
    assert pl.episode_world_traffic_resets().tobytes() == counted.tobytes()  # readable, as they were
    if call in ("fleet", "world_traffic"):                                     # (the vehicles are back in front of their worlds: something ends)
        assert _behaves(pl) == want
        if call == "fleet":
            assert (pl.episode_stats()["last_cause"][:3] & WORLD).any()        # scenes 1 and 2 end with scene 0 now
    else:
        pl.rollout(45)
        pl.sync()
    assert pl.episode_world_traffic_resets().tobytes() == counted.tobytes()  # ... and nothing counts any more
    assert _worlds_on(dm, pl) == want[0]
    if not want[0]:
        pl.set_episode_worlds()
        pl.set_episode_world_traffic(1)
    assert not pl.episode_world_traffic_resets().any()                         # a new table, new counters
    pl.close()
