"""Traffic manoeuvres around the advance itself: a list that never fires against a handle without one, pp_update_async
between advances, the episode reset (k_reset_manoeuvres behind k_reset_traffic), and every call's refusals and switch-off sites.
The cases and the device loop are those of tests/manoeuvre_scenes.py; the model is tests/traffic_manoeuvre_model.py."""
import numpy as np
import pytest

import manoeuvre_scenes as ms
import traffic_follow_backends as fb
import traffic_manoeuvre_model as mm
import traffic_scenes as ts

gpu = pytest.mark.gpu
FAR = ms.FAR
R, T = 0.9, 3


def _lanes(dm, n=160):
    return [(ms.line(dm, n), False), (ms.line(dm, n, y=3.5), False)]


def _two_scenes(dm, tf, recs=None, ego=FAR):
    """Two scenes of three vehicles: one 30 m along y = 0 with one 10 m behind it, and one 18 m along y = 3.5; the first of each
    scene (actors 0 and 3) cuts onto y = 3.5 in 4 advances and ends 0.5 m left of it."""
    rows = [(30.0, 5.0, 0, T, R), (20.0, 4.0, 0, T, R), (18.0, 6.0, 1, T, R)]
    recs = [mm.record(0, track=1, lat_end=0.5, n_steps=4), mm.record(3, track=1, lat_end=0.5, n_steps=4)] if recs is None else recs
    return ms.case("two_scenes", _lanes(dm), [dict(ego=ego, actors=rows), dict(ego=ego, actors=rows)], recs, tf)


def _snapshot(dm, pl, act, stride, n, follow):
    return pl.traffic_state().tobytes(), pl.traffic_speed().tobytes() if follow else b"", ms.read_actors(dm, pl, act, stride, n).tobytes()


@gpu
@pytest.mark.parametrize("follow,motion,fleet", [(False, False, None), (True, False, None), (True, True, None), (False, True, "before"), (True, False, "after")],
                         ids=["plain", "follow", "follow-motion", "motion-fleet-before", "follow-fleet-after"])
def test_idle_is_plain_traffic(dm, follow, motion, fleet):
    """A handle whose manoeuvres never come within reach (after = 2^30) against a handle without: the same pool, s and v bytes over
    8 advances - k_manoeuvre_traffic with lat = 0 on the actor's own track gives the bytes of k_move_traffic / k_follow_traffic."""
    tf = {} if follow else None
    c = _two_scenes(dm, tf, [mm.record(0, mm.EGO_DIST, 1, dist=50.0, after=2 ** 30, track=1), mm.record(4, after=2 ** 30, lat_end=1.0)], ego=(40.0, 0.0, 9.0, False))
    fmod = dm.default_fleet_model()
    fmod["range"], fmod["max_peers"] = 40.0, 2

    def fleet_of(pl):
        pl.set_fleet([0, 2], fmod)
    runs = []
    for manoeuvres in (True, False):
        pl, act, stride, model, po = ms.open_device(dm, c, with_motion=motion, manoeuvres=manoeuvres, before=fleet_of if fleet == "before" else None, peers=2 if fleet else 0)
        if fleet == "after":
            fleet_of(pl)
        n, total = len(c.scenes), len(c.scenes) * (stride + (2 if fleet else 0))
        seen = [_snapshot(dm, pl, act, stride, n, follow)]
        for k in range(8):
            fb.staged_step(dm, pl, model, po)
            seen.append(_snapshot(dm, pl, act, stride, n, follow))
        pl.tick()
        seen.append((pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, total).tobytes(), pl.read_device(dm.BUF_MOT_POOL, dm.ObMotion, total).tobytes() if motion else b""))
        if manoeuvres:
            st = pl.get_traffic_manoeuvre_state()
            assert st["clock"].tolist() == [8] * 6 and not st["n_done"].any() and not st["lat"].any()
        pl.close()
        runs.append(seen)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a == b, f"stage {k}: a list out of reach changes the bytes of plain traffic"
    assert runs[0][0] != runs[0][8]


@gpu
@pytest.mark.parametrize("follow", [False, True])
def test_update_async_places_the_offset_pose_and_nothing_else(dm, follow):
    """Two advances into a move, a caller-uploaded pool comes out with every actor at its current (s, lat) on its current track; s, v and
    the states - the clock included - are what they were, and the next advance goes on from there."""
    tf = {} if follow else None
    c = _two_scenes(dm, tf)
    pl, act, stride, model, po = ms.open_device(dm, c)
    n = len(c.scenes)
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    tracks, pts = ts.pack(dm, c.polylines)
    tr = mm.Manoeuvres(tracks, pts, act, np.arange(n) * stride, c.recs)
    pool, _ = tr.place(ts.filled(dm.ObPoint, n * stride), None, 0.0)

    def step(pool):
        si, flags = fb.staged_step(dm, pl, model, po)
        pool, _ = tr.advance(pool, None, ms.DT, tf, si, flags, width)
        assert pl.get_traffic_manoeuvre_state().astype(mm.STATE).tobytes() == tr.st.tobytes() and pl.traffic_state().tobytes() == tr.s.tobytes()
        assert ms.read_actors(dm, pl, act, stride, n).tobytes() == pool[tr.pool_index].tobytes()
        return pool
    for _ in range(2):
        pool = step(pool)
    pl.tick()
    assert tr.st["k"].tolist() == [2, 0, 0, 2, 0, 0] and (tr.st["lat"][[0, 3]] != 0).all() and tr.st["clock"].tolist() == [0, 2, 2, 0, 2, 2]
    before = (pl.get_traffic_manoeuvre_state().tobytes(), pl.traffic_state().tobytes(), pl.traffic_speed().tobytes() if follow else b"")
    up = dm.pinned_copy(np.frombuffer(bytes([0x5A]) * (n * stride * dm.ObPoint.itemsize), dm.ObPoint))
    pl.update_async(obs_pool=up)
    assert before == (pl.get_traffic_manoeuvre_state().tobytes(), pl.traffic_state().tobytes(), pl.traffic_speed().tobytes() if follow else b"")
    pl.tick()
    pool, _ = tr.update(np.array(up))
    got = pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * stride)
    assert got.tobytes() == pool.tobytes()
    assert got["y"][0] == 3.5 + tr.st["lat"][0] and got["y"][1] == 0.0          # the offset pose, left of y = 3.5 by a negative lat
    si, flags = fb.staged_step(dm, pl, model, po)
    pool, _ = tr.advance(pool, None, ms.DT, tf, si, flags, width)
    assert pl.get_traffic_manoeuvre_state().astype(mm.STATE).tobytes() == tr.st.tobytes() and pl.traffic_state().tobytes() == tr.s.tobytes()
    assert ms.read_actors(dm, pl, act, stride, n).tobytes() == pool[tr.pool_index].tobytes()
    pl.close()


@gpu
@pytest.mark.parametrize("follow", [False, True])
def test_episode_reset_puts_the_manoeuvres_back(dm, follow):
    """Episodes + spawn model + §4m's reset + manoeuvres.  Scene 0's ego is flagged in advance 3 - two advances into its vehicle's
    4-advance cut-in - and restarts; scene 1 goes on.  The restarted scene's states are the set call's (n_done kept), its s, v and pool
    entries the start's, and its second episode repeats the first byte for byte, advance by advance; scene 1 is the model's without
    any restart.  Then the move finishes in both and n_done counts on."""
    tf = {} if follow else None
    c = _two_scenes(dm, tf)
    pl, act, stride, model, po = ms.open_device(dm, c)
    n = len(c.scenes)
    em = dm.default_episode_model()
    sp = dm.default_episode_spawn()
    sp["contact"], sp["check"] = 0, 0
    pl.set_episodes(em)
    pl.set_episode_spawn(sp)
    pl.set_episode_traffic(1)
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    tracks, pts = ts.pack(dm, c.polylines)
    tr = mm.Manoeuvres(tracks, pts, act, np.arange(n) * stride, c.recs)
    pool, _ = tr.place(ts.filled(dm.ObPoint, n * stride), None, 0.0)
    s_start, v_start = tr.s.copy(), tr.v.copy()
    flagged = fb.staging_plan(dm, [(FAR[0], FAR[1], FAR[2], True), FAR], ms.DT)
    stages = [(tr.st.copy(), tr.s.copy(), tr.v.copy(), pool[tr.pool_index].copy())]
    for k in range(1, 10):
        si, flags = fb.staged_step(dm, pl, model, flagged if k == 3 else po)
        age = pl.episode_stats()["age"]
        assert (age == 0).tolist() == [k == 3, False], f"advance {k}: ages {age.tolist()}"
        pool, _ = tr.advance(pool, None, ms.DT, tf, si, flags, width)
        if k == 3:          # §4m: s and v of set 0, the plain pose on the initial track; §4v: the state of the set call
            tr.restart([0])
            tr.s[:3], tr.v[:3] = s_start[:3], v_start[:3]
            pool, _ = tr.update(pool)
        got = (pl.get_traffic_manoeuvre_state().astype(mm.STATE), pl.traffic_state(), pl.traffic_speed() if follow else tr.v.copy(), ms.read_actors(dm, pl, act, stride, n))
        want = (tr.st, tr.s, tr.v, pool[tr.pool_index])
        for name, g, w in zip(("states", "s", "v", "pool entries"), got, want):
            assert g.tobytes() == w.tobytes(), f"advance {k}: {name} differ from the model's at actors {np.flatnonzero(g != w).tolist()}"
        stages.append(tuple(x.copy() for x in got))
    assert pl.episode_traffic_resets().tolist() == [1, 1, 1, 0, 0, 0]
    pl.close()
    first = slice(0, 3)
    assert stages[2][0]["k"][0] == 2 and stages[3][0][first].tobytes() == stages[0][0][first].tobytes()          # under way, then the set call's state
    for k in (0, 1, 2):          # the second episode of scene 0, advance by advance (n_done is 0 in both: the move never finished before)
        for a, b in zip(stages[k], stages[k + 3]):
            assert a[first].tobytes() == b[first].tobytes(), f"episode 2, advance {k}"
    assert stages[9][0]["n_done"].tolist() == [1, 0, 0, 1, 0, 0] and stages[9][0]["track"].tolist() == [1, 0, 1, 1, 0, 1] and stages[9][0]["lat"][[0, 3]].tolist() == [0.5, 0.5]


@gpu
@pytest.mark.parametrize("follow", [False, True])
def test_timeout_restarts_mid_move_and_replays(dm, follow):
    """EpisodeModel.max_ticks = 3 against a 4-advance cut-in: every episode ends on DMPP_EGO_TIMEOUT with the move under way.  After
    every advance the device is the model's, the restarted actors have the set call's state, and every later episode repeats the first
    byte for byte, advance by advance - states, s, v and pool entries."""
    tf = {} if follow else None
    c = _two_scenes(dm, tf)
    pl, act, stride, model, po = ms.open_device(dm, c)
    n = len(c.scenes)
    em = dm.default_episode_model()
    em["max_ticks"] = 3
    sp = dm.default_episode_spawn()
    sp["contact"], sp["check"] = 0, 0
    pl.set_episodes(em)
    pl.set_episode_spawn(sp)
    pl.set_episode_traffic(1)
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    tracks, pts = ts.pack(dm, c.polylines)
    tr = mm.Manoeuvres(tracks, pts, act, np.arange(n) * stride, c.recs)
    pool, _ = tr.place(ts.filled(dm.ObPoint, n * stride), None, 0.0)
    s_start, v_start = tr.s.copy(), tr.v.copy()
    stages, restarts = [(tr.st.copy(), tr.s.copy(), tr.v.copy(), pool[tr.pool_index].copy())], []
    for k in range(1, 11):
        si, flags = fb.staged_step(dm, pl, model, po)
        stats = pl.episode_stats()
        pool, _ = tr.advance(pool, None, ms.DT, tf, si, flags, width)
        if (stats["age"] == 0).any():
            assert (stats["age"] == 0).all() and (stats["last_cause"] == dm.EGO_TIMEOUT).all(), stats["last_cause"].tolist()
            assert tr.st["k"][[0, 3]].tolist() == [3, 3] or tr.st["k"][[0, 3]].tolist() == [2, 2], "the move is under way at the restart"
            restarts.append(k)
            tr.restart([0, 1])
            tr.s[:], tr.v[:] = s_start, v_start
            pool, _ = tr.update(pool)
        got = (pl.get_traffic_manoeuvre_state().astype(mm.STATE), pl.traffic_state(), pl.traffic_speed() if follow else tr.v.copy(), ms.read_actors(dm, pl, act, stride, n))
        for name, g, w in zip(("states", "s", "v", "pool entries"), got, (tr.st, tr.s, tr.v, pool[tr.pool_index])):
            assert g.tobytes() == w.tobytes(), f"advance {k}: {name} differ from the model's at actors {np.flatnonzero(g != w).tolist()}"
        stages.append(tuple(x.copy() for x in got))
    pl.close()
    assert len(restarts) >= 2 and restarts[1] - restarts[0] < 4, restarts
    period = restarts[1] - restarts[0]
    assert not stages[-1][0]["n_done"].any()                     # no move ever finished
    for r in restarts:
        for j in range(period):
            if r + j < len(stages):
                for a, b in zip(stages[restarts[0] + j], stages[r + j]):
                    assert a.tobytes() == b.tobytes(), f"the episode from advance {r}, advance {j}"
    for a, b in zip(stages[0], stages[restarts[0]]):
        assert a.tobytes() == b.tobytes(), "a restart is the state behind the set calls"


@gpu
def test_following_off_and_on_again_mid_move(dm):
    """pp_set_traffic_follow(NULL) and (non-NULL) two advances into a move: the states stay, the scripted step runs at v0 while following
    is off, and switching it on again starts every actor at v = v0 - the speed a record may have changed."""
    c = _two_scenes(dm, {}, [mm.record(0, track=1, lat_end=0.5, n_steps=6, speed=7.0), mm.record(3, track=1, lat_end=0.5, n_steps=6, speed=7.0)])
    pl, act, stride, model, po = ms.open_device(dm, c)
    n = len(c.scenes)
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    tracks, pts = ts.pack(dm, c.polylines)
    tr = mm.Manoeuvres(tracks, pts, act, np.arange(n) * stride, c.recs)
    tr.set_follow()
    pool, _ = tr.place(ts.filled(dm.ObPoint, n * stride), None, 0.0)

    def step(pool, tf):
        si, flags = fb.staged_step(dm, pl, model, po)
        pool, _ = tr.advance(pool, None, ms.DT, tf, si, flags, width)
        assert pl.get_traffic_manoeuvre_state().astype(mm.STATE).tobytes() == tr.st.tobytes() and pl.traffic_state().tobytes() == tr.s.tobytes()
        assert tf is None or pl.traffic_speed().tobytes() == tr.v.tobytes()
        assert ms.read_actors(dm, pl, act, stride, n).tobytes() == pool[tr.pool_index].tobytes()
        return pool
    pool = step(pool, {})                                         # (one advance: the current arrays are the second pair)
    pl.tick()
    before = (pl.get_traffic_manoeuvre_state().tobytes(), pl.traffic_state().tobytes())
    pl.set_traffic_follow(None)
    assert before == (pl.get_traffic_manoeuvre_state().tobytes(), pl.traffic_state().tobytes())
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_speed()
    for _ in range(2):
        pool = step(pool, None)
    pl.tick()
    assert tr.st["k"].tolist() == [3, 0, 0, 3, 0, 0] and tr.st["v0"].tolist() == [7.0, 4.0, 6.0] * 2
    before = (pl.get_traffic_manoeuvre_state().tobytes(), pl.traffic_state().tobytes())
    pl.set_traffic_follow(fb.fm_record(dm, {}))
    tr.set_follow()
    assert before == (pl.get_traffic_manoeuvre_state().tobytes(), pl.traffic_state().tobytes())
    assert pl.traffic_speed().tolist() == [7.0, 4.0, 6.0] * 2    # v = v0, not the actors' speed of pp_set_traffic
    for _ in range(4):
        pool = step(pool, {})
    assert tr.st["n_done"].tolist() == [1, 0, 0, 1, 0, 0]
    pl.close()


@gpu
def test_calls_refusals_and_switch_off_sites(dm):
    """Every PP_ERR_STATE / PP_ERR_ARG of the set call with the handle's bytes unchanged after each, the getter, the off form held to the
    model, pp_set_traffic dropping the list, and the order against pp_set_episode_traffic."""
    tf = {}
    c = _two_scenes(dm, tf)
    pl, act, stride, model, po = ms.open_device(dm, c, manoeuvres=False)
    n = len(c.scenes)
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    tracks, pts = ts.pack(dm, c.polylines)
    recs = c.recs.astype(dm.TrafficManoeuvre)
    state, arg = "error -4:", "error -1:"
    with pytest.raises(dm.PlannerError, match=state):
        pl.get_traffic_manoeuvre_state()                          # no list in force
    pl.set_traffic_manoeuvres(None)                               # off while off: nothing to do
    pl.set_traffic_manoeuvres(recs)
    tr = mm.Manoeuvres(tracks, pts, act, np.arange(n) * stride, c.recs)
    tr.set_follow()
    pool, _ = tr.place(ts.filled(dm.ObPoint, n * stride), None, 0.0)

    def same(pool):
        assert pl.get_traffic_manoeuvre_state().astype(mm.STATE).tobytes() == tr.st.tobytes() and pl.traffic_state().tobytes() == tr.s.tobytes()
        assert pl.traffic_speed().tobytes() == tr.v.tobytes() and ms.read_actors(dm, pl, act, stride, n).tobytes() == pool[tr.pool_index].tobytes()

    def step(pool):
        si, flags = fb.staged_step(dm, pl, model, po)
        pool, _ = tr.advance(pool, None, ms.DT, tf, si, flags, width)
        same(pool)
        return pool
    same(pool)
    pool = step(pool)
    # PP_ERR_STATE: an update staged (the advance just made)
    for r in (recs, None):
        with pytest.raises(dm.PlannerError, match=state):
            pl.set_traffic_manoeuvres(r)
        same(pool)
    pl.tick()
    # PP_ERR_ARG: one refused list per rule, the list in force untouched
    def edit(**kw):
        r = recs.copy()
        for k, v in kw.items():
            r[k][1] = v
        return r
    bad = [edit(actor=6), edit(actor=-1), edit(track=2), edit(track=-2), recs[::-1].copy(), np.concatenate([recs[:1]] * 9), edit(trigger=3), edit(trigger=1 | 3 << 8),
           edit(trigger=1 << 8), edit(trigger=1, dist=np.nan), edit(trigger=1, dist=-1.0), edit(trigger=2, time=np.inf), edit(trigger=2, time=-1.0), edit(lat_end=np.nan),
           edit(lat_end=np.inf), edit(speed=np.inf), edit(after=-1), edit(n_steps=0), edit(n_steps=4097), edit(_pad=7)]
    for k, r in enumerate(bad):
        with pytest.raises(dm.PlannerError, match=arg):
            pl.set_traffic_manoeuvres(r)
        same(pool)
    pool = step(pool)                                             # ... and the move goes on as if nothing had been called
    pl.tick()
    # while a list is in force pp_set_episode_traffic needs every actor in the state of the set call
    pl.set_episodes(dm.default_episode_model())
    with pytest.raises(dm.PlannerError, match=state):
        pl.set_episode_traffic(1)
    same(pool)
    # the off form: every actor goes on along the track it is on at the speed it wants; the offset goes at the next staged set
    assert tr.st["track"].tolist() == [1, 0, 1, 1, 0, 1] and (tr.st["lat"][[0, 3]] != 0).all()
    pl.set_traffic_manoeuvres(None)
    with pytest.raises(dm.PlannerError, match=state):
        pl.get_traffic_manoeuvre_state()
    act2 = act.copy()
    act2["track"], act2["speed"] = tr.st["track"], tr.st["v0"]
    plain = fb.fm.Follow(tracks, pts, act2, np.arange(n) * stride)
    plain.s, plain.v = tr.s.copy(), tr.v.copy()
    assert pl.traffic_state().tobytes() == plain.s.tobytes() and pl.traffic_speed().tobytes() == plain.v.tobytes()
    for k in range(3):
        si, flags = fb.staged_step(dm, pl, model, po)
        pool, _ = plain.step(pool, None, ms.DT, tf, si, flags, width)
        assert pl.traffic_state().tobytes() == plain.s.tobytes() and pl.traffic_speed().tobytes() == plain.v.tobytes(), f"advance {k} after the off form"
        assert ms.read_actors(dm, pl, act, stride, n).tobytes() == pool[plain.pool_index].tobytes()
    assert any(i.kind == "actor" and i.leader == 0 for i in plain.info[:3])          # the vehicle that cut in leads on its new track
    pl.tick()
    # a list again, then the reset: the call comes BEFORE pp_set_episode_traffic, and is refused after it
    pl.set_traffic_manoeuvres(recs)
    st = pl.get_traffic_manoeuvre_state()
    assert st["track"].tolist() == [1, 0, 1, 1, 0, 1] and st["v0"].tolist() == act2["speed"].tolist() and not st["k"].any() and not st["lat"].any()
    pl.set_episode_traffic(1)
    s_was, v_was, ob_was = pl.traffic_state().tobytes(), pl.traffic_speed().tobytes(), ms.read_actors(dm, pl, act, stride, n).tobytes()
    for r in (recs, None):
        with pytest.raises(dm.PlannerError, match=state):
            pl.set_traffic_manoeuvres(r)
        assert pl.get_traffic_manoeuvre_state().tobytes() == st.tobytes()
        assert (pl.traffic_state().tobytes(), pl.traffic_speed().tobytes(), ms.read_actors(dm, pl, act, stride, n).tobytes()) == (s_was, v_was, ob_was)
    # whatever replaces the traffic frees the list: pp_set_traffic, its no-actors form, new resident scenes
    pl.set_traffic(tracks, pts, act)
    with pytest.raises(dm.PlannerError, match=state):
        pl.get_traffic_manoeuvre_state()
    pl.set_traffic_manoeuvres(recs)
    pl.set_traffic(None, None, None)
    with pytest.raises(dm.PlannerError, match=state):
        pl.get_traffic_manoeuvre_state()
    ob_was = ms.read_actors(dm, pl, act, stride, n).tobytes()
    with pytest.raises(dm.PlannerError, match=state):
        pl.set_traffic_manoeuvres(recs)                           # no per-scene traffic
    assert ms.read_actors(dm, pl, act, stride, n).tobytes() == ob_was
    with pytest.raises(dm.PlannerError, match=state):
        pl.traffic_state()
    pl.set_traffic(tracks, pts, act)
    pl.set_traffic_manoeuvres(recs)
    pl.set_scenes(pl.scenes, with_motion=False)
    pl.set_state(pl.scenes["state"])
    with pytest.raises(dm.PlannerError, match=state):
        pl.get_traffic_manoeuvre_state()
    # world traffic has no manoeuvres
    fmod = dm.default_fleet_model()
    fmod["max_peers"] = 0
    pl.set_fleet([0, n], fmod)
    wact = act[:3].copy()
    pl.set_world_traffic(tracks, pts, wact)
    s_was, ob_was = pl.traffic_state().tobytes(), np.concatenate([pl.get_obstacles(k, cap=stride) for k in range(n)]).tobytes()
    with pytest.raises(dm.PlannerError, match=state):
        pl.set_traffic_manoeuvres(recs[:1])
    assert (pl.traffic_state().tobytes(), np.concatenate([pl.get_obstacles(k, cap=stride) for k in range(n)]).tobytes()) == (s_was, ob_was)
    with pytest.raises(dm.PlannerError, match=state):
        pl.get_traffic_manoeuvre_state()
    lib = dm.load_library()
    assert lib.pp_feature_retires(14) == -1
    pl.close()
