"""Episode log (pp_set_episode_log): one record per ended episode, appended on the device in the order of the scenes.

CPU: the ABI mirror and its offsets, hand-derived records of the numpy model (tests/episode_log_model.py over the episode models)
for each of the five flags and for TIMEOUT, two episodes in a row, a start record that ends at once, the episode's own scorecard on
the scenario of tests/test_episodes.py::_kat_the_scorecard_does_not_see_the_jump, and the ring arithmetic.
GPU: the same known answers on k_log_episodes; its order and the seams of its scan (wave 64, block and chunk 1024); the ring; the spawn model, and a set call
in the middle of a run under it; pp_score_begin behind the set call and in the middle of an episode; a closed loop on the ring of tests/route_scenes.py with the
scorecard on, and pp_rollout against its parts; the log only observes; the error paths and the lifetime.

The scenes are built from the two egos of tests/test_episodes.py on its small map: the LANE_END ego ends on its first advance -
and, put back on the same record, on every later one -, the other goes on; a boolean mask over the scenes chooses who ends."""
import numpy as np
import pytest

import episode_log_backends as elb
import episode_log_model as elm
import rollout_score_model as rsm
import test_episodes as te

gpu = pytest.mark.gpu
cfg0 = te.cfg0


def _runner(name):
    return elb.Runner(elb.ModelBackend() if name == "model" else elb.DeviceBackend())


def _one(dm, cfg, si, pos, em, legs=None, sts=None, score=False, sp=None, starts=None):
    """A Case of ONE scene, as tests/test_episodes.py::_Ep makes its calls."""
    route = None if legs is None else (legs, np.array([0, len(legs)], np.int32), dm.default_route_model())
    sts = [np.zeros(1, dm.SceneState) for _ in pos] if sts is None else sts
    return elb.Case(cfg, dm.default_ego_model(), em, sp, si, [np.zeros(0, dm.ObPoint)], te._state0(dm), list(zip(pos, sts)), te._world(dm), route, starts, None, score)


def _masked(dm, cfg, mask, n_steps=1, em=None, sp=None, starts=None):
    """len(mask) routed scenes: the LANE_END ego (x = 133, lane 1, ego_id = 60) where the mask is set, else the ego that goes on (x = 110 + k
    at step k, ego_id = 20)."""
    mask = np.asarray(mask, bool)
    n = len(mask)
    si = np.repeat(te._ego(dm, 110.0, ego_id=20), n)
    si[mask] = te._ego(dm, 133.0, y=3.75, lane=1, ego_id=60)[0]
    steps = []
    for k in range(n_steps):
        po = np.repeat(te._path(dm, 110.0 + k), n)
        po[mask] = te._path(dm, 133.0, y=3.75)[0]
        steps.append((po, np.zeros(n, dm.SceneState)))
    route = (np.tile(te._legs(dm), n), np.arange(0, 2 * n + 1, 2, dtype=np.int32), dm.default_route_model())
    return elb.Case(cfg, dm.default_ego_model(), te._em(dm) if em is None else em, sp, si, [np.zeros(0, dm.ObPoint)] * n, np.repeat(te._state0(dm), n), steps,
                    te._world(dm), route, starts)


def _rec(r):
    return dict(scene=int(r["scene"]), episode=int(r["episode"]), start=int(r["start"]), cause=int(r["cause"]), age=int(r["age"]), seq=int(r["seq"]),
                tick=int(r["tick"]), dist=float(r["dist"]), x=float(r["end_pos"]["x"]), y=float(r["end_pos"]["y"]), v=float(r["end_speed"]))


def _unscored(dm, r):
    return r["score"].tobytes() == rsm.new_scores(dm.RolloutScore, 1)[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirror_and_offsets(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(34) == dm.EpisodeRecord.itemsize == 240 and dm.EPISODE_LOG_MAX == 1 << 20
    names = ("scene", "episode", "start", "cause", "age", "seq", "tick", "dist", "end_pos", "end_speed", "score")
    assert [dm.EpisodeRecord.fields[k][1] for k in names] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 56, 64]
    assert dm.EpisodeRecord.fields["score"][0] == dm.RolloutScore and dm.EpisodeRecord.fields["tick"][0] == np.int64
    for sym in ("pp_set_episode_log", "pp_read_episode_log", "pp_get_episode_log_info"):
        getattr(lib, sym)


def _kat_each_flag_and_the_timeout(dm, cfg0, run):
    # the five advances of tests/test_episodes.py::_flag_cases: one record each - episode 0 on start record 0, ended by advance 0, which
    # read tick 1, after 1 advance and d metres, at the pose and speed of the record that advance READ (the start record); no scorecard
    for flag, cfg, si, po, st, legs, d in te._flag_cases(dm, cfg0):
        r = run(_one(dm, cfg, si, [po], te._em(dm), legs, None if st is None else [st]), 4)
        (rec,) = r.records
        loc = si["loc"][0]
        assert _rec(rec) == dict(scene=0, episode=0, start=0, cause=flag, age=1, seq=0, tick=1, dist=d, x=float(loc["globalpoint"]["x"]),
                                 y=float(loc["globalpoint"]["y"]), v=36.0), flag
        assert _unscored(dm, rec) and r.infos == [(1, 0)]
    # max_ticks = 3: advances 0 and 1 log nothing, advance 2 (seq 2, behind tick 3) ends the episode at age 3 after 3 m; it read the record on 112
    r = run(_one(dm, cfg0, te._ego(dm, 110.0, ego_id=20), [te._path(dm, 110.0), te._path(dm, 111.0), te._path(dm, 112.0)], te._em(dm, 31, 3)), 4)
    assert [len(q) for q, _ in r.reads] == [0, 0, 1] and r.infos == [(0, 0), (0, 0), (1, 0)]
    assert _rec(r.records[0]) == dict(scene=0, episode=0, start=0, cause=64, age=3, seq=2, tick=3, dist=3.0, x=112.0, y=0.0, v=36.0)


def _kat_two_episodes_in_a_row(dm, cfg0, run):
    # tests/test_episodes.py::_kat_two_episodes_in_a_row: advance 1 ends episode 0 (age 2, 2 m, read from 133.0), advance 2 ends episode 1 (age 1,
    # the jump of 2.5 m, read from the start record on 132)
    si = te._ego(dm, 132.0, y=3.75, lane=1, ego_id=60)
    r = run(_one(dm, cfg0, si, [te._path(dm, 132.0, y=3.75), te._path(dm, 133.0, y=3.75), te._path(dm, 133.5, y=3.75)], te._em(dm), te._legs(dm)), 4)
    assert [len(q) for q, _ in r.reads] == [0, 1, 1]
    assert _rec(r.records[0]) == dict(scene=0, episode=0, start=0, cause=4, age=2, seq=1, tick=2, dist=2.0, x=133.0, y=3.75, v=36.0)
    assert _rec(r.records[1]) == dict(scene=0, episode=1, start=0, cause=4, age=1, seq=2, tick=3, dist=2.5, x=132.0, y=3.75, v=36.0)


def _kat_a_start_record_that_ends_at_once(dm, cfg0, run):
    # one record per advance, never two; drained once at the end they come out oldest first
    si, po = te._ego(dm, 133.0, y=3.75, lane=1, ego_id=60), te._path(dm, 133.0, y=3.75)
    r = run(_one(dm, cfg0, si, [po, po, po], te._em(dm), te._legs(dm)), 4, "end")
    assert r.infos == [(1, 0), (2, 0), (3, 0)] and [(len(q), lost) for q, lost in r.reads] == [(3, 0)]
    for k, rec in enumerate(r.records):
        assert _rec(rec) == dict(scene=0, episode=k, start=0, cause=4, age=1, seq=k, tick=k + 1, dist=1.0, x=133.0, y=3.75, v=36.0)


def _kat_the_episodes_own_scorecard(dm, cfg0, run):
    # tests/test_episodes.py::_kat_the_scorecard_does_not_see_the_jump, twice in a row: max_ticks = 2, scored ticks (110, 36) and (x1, v1), then the
    # restart.  The record of advance 1 carries n_ticks = 2, dist = x1 - 110, max_dec = 4 and - no patch - the last scored pose x1; the record
    # of advance 3 is the second episode's own: the same two ticks again, not four of them
    v1 = 36.0 - 4.0 * 0.1 * 3.6
    s = 0.5 * (36.0 + v1) / 3.6 * 0.1
    x1 = 110.5 + (s - 0.5) / 0.5 * (111.0 - 110.5)
    dec = -((v1 - 36.0) / 3.6 / 0.1)
    pos = [te._path(dm, 110.0, desspd=30.0), te._path(dm, 111.0, desspd=30.0)] * 2
    r = run(_one(dm, cfg0, te._ego(dm, 110.0, ego_id=20), pos, te._em(dm, 31, 2), score=True), 4)
    assert [len(q) for q, _ in r.reads] == [0, 1, 0, 1]
    for k, rec in enumerate(r.records):
        assert _rec(rec) == dict(scene=0, episode=k, start=0, cause=64, age=2, seq=2 * k + 1, tick=2 * k + 2, dist=r.records[0]["dist"], x=x1, y=0.0, v=v1)
        sc = rec["score"]
        assert (int(sc["n_ticks"]), float(sc["dist"]), float(sc["max_acc"]), float(sc["max_dec"]), float(sc["max_speed"])) == (2, x1 - 110.0, 0.0, dec, 36.0)
        assert (float(sc["last_pos"]["x"]), float(sc["last_pos"]["y"]), float(sc["last_speed"])) == (x1, 0.0, v1)
        assert not sc["n_grid_ticks"] and not sc["grid_status_ticks"].any() and int(sc["behavior_ticks"].sum()) == 2
    assert abs(dec - 4.0) < 1e-12 and abs(x1 - 110.98) < 1e-12
    if run.name == "model":
        assert r.records[0]["score"].tobytes() == r.records[1]["score"].tobytes()


KATS = [_kat_each_flag_and_the_timeout, _kat_two_episodes_in_a_row, _kat_a_start_record_that_ends_at_once, _kat_the_episodes_own_scorecard]


@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, cfg0, kat):
    kat(dm, cfg0, _runner("model"))


def test_ring_arithmetic_on_the_model(dm, cfg0):
    """m = 5 scenes end in one advance, cap = 3: ordinals 0 and 1 are never written, 2, 3, 4 go to slots 2, 0, 1; a read gives scenes 2, 3, 4
    and counts 2 lost.  With one more advance the ordinals 5 .. 9 follow: 7, 8, 9 to slots 1, 2, 0."""
    r = _runner("model")(_masked(dm, cfg0, [True] * 5), 3)
    assert r.infos == [(5, 2)] and [(q["scene"].tolist(), lost) for q, lost in r.reads] == [([2, 3, 4], 2)]
    log = elm.EpisodeLog(dm.EpisodeRecord, 5, 3)
    stats, si = r.data[0].stats, r.data[0].prev_in
    log.append(stats, si, 1)
    assert log.ring["scene"].tolist() == [3, 4, 2] and log.info() == (5, 2)
    log.append(stats, si, 2)
    assert log.ring["scene"].tolist() == [4, 2, 3] and log.ring["seq"].tolist() == [1, 1, 1] and log.info() == (10, 7)
    q, lost = log.read(2)
    assert (q["scene"].tolist(), lost, log.info()) == ([2, 3], 7, (10, 7))
    q, lost = log.read()
    assert (q["scene"].tolist(), lost, log.info()) == ([4], 0, (10, 7))
    # a scene that goes on appends nothing, whatever the others do
    r = _runner("model")(_masked(dm, cfg0, [False, True, False, True, False], 2), 3, "end")
    assert r.infos == [(2, 0), (4, 1)] and [(q["scene"].tolist(), q["seq"].tolist(), lost) for q, lost in r.reads] == [([3, 1, 3], [0, 1, 1], 1)]


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg0, kat):
    """The known answers above on k_log_episodes, every read also held against the model on the device's own records (elb.Runner)."""
    kat(dm, cfg0, _runner("device"))


_ALONE = {}


def _alone(dm, cfg):
    """The record the ending ego gives as the only scene of a launch."""
    if "rec" not in _ALONE:
        (_ALONE["rec"],) = _runner("device")(_masked(dm, cfg, [True]), 4).records
    return _ALONE["rec"]


def _masks(n, which):
    m = np.zeros(n, bool)
    if which == "all":
        m[:] = True
    elif which == "first":
        m[0] = True
    elif which == "last":
        m[-1] = True
    elif which == "last two":
        m[-2:] = True
    elif which == "every other":
        m[::2] = True
    return m


SHAPES = [(5, "all"), (9, "all"), (65, "all"), (65, "none"), (65, "first"), (65, "last"), (65, "last two"), (257, "last two"), (1025, "last two"), (1025, "every other"),
          (2049, "last two"), (3073, "every other"), (3073, "first")]


@gpu
@pytest.mark.parametrize("n, which", SHAPES, ids=lambda v: str(v).replace(" ", "_"))
def test_order_and_the_seams_of_the_scan(dm, cfg0, n, which):
    """One advance of n scenes, a ring that holds them all: the records are the ended scenes in the order of their indices
    - {63, 64} and {255, 256} across two waves of one chunk, {1023, 1024} across two chunks, every other scene of 1025 in both -, equal to the
    model byte for byte, and each equal to the record the scene gives alone but for `scene`.  The kernel's chunk is 1024 scenes and its wave
    totals go through two LDS sets used in turn: {2047, 2048} of 2049 carry the base over two chunks into the third, which writes the first
    set again; every other scene of 3073 fills all four chunks; only scene 0 of 3073 leaves the scan with three chunks unvisited."""
    mask = _masks(n, which)
    r = _runner("device")(_masked(dm, cfg0, mask), n + 3)
    recs = r.records
    assert recs["scene"].tolist() == np.flatnonzero(mask).tolist() and r.infos == [(int(mask.sum()), 0)]
    alone = _alone(dm, cfg0)
    for rec in recs:
        one = rec.copy()
        one["scene"] = 0
        assert one.tobytes() == alone.tobytes(), int(rec["scene"])


@gpu
@pytest.mark.parametrize("n, which", [(9, "every other"), (1029, "every other"), (2051, "every other")], ids=["9", "1029", "2051"])
def test_more_endings_than_the_ring_holds(dm, cfg0, n, which):
    """m scenes end in one advance, cap = m - 1 | m | m + 1, over one chunk of scenes, over two and over three: the last
    min(m, cap) records in order, the others counted as lost; then the same launch again on the ring as it stands."""
    mask = _masks(n, which)
    ended = np.flatnonzero(mask).tolist()
    m = len(ended)
    for cap in (m - 1, m, m + 1):
        r = _runner("device")(_masked(dm, cfg0, mask, 2), cap)
        lost = max(m - cap, 0)
        assert r.infos == [(m, lost), (2 * m, 2 * lost)], cap
        assert [(q["scene"].tolist(), q["seq"].tolist(), k) for q, k in r.reads] == [(ended[lost:], [0] * (m - lost), lost), (ended[lost:], [1] * (m - lost), lost)], cap
        e = _runner("device")(_masked(dm, cfg0, mask, 2), cap, "end")
        keep = (ended + ended)[2 * m - min(cap, 2 * m):]
        assert e.infos == [(m, lost), (2 * m, 2 * m - len(keep))] and [(q["scene"].tolist(), k) for q, k in e.reads] == [(keep, 2 * m - len(keep))], cap


@gpu
def test_ring_of_three_over_four_advances(dm, cfg0):
    """cap = 3, scenes 1 and 3 of five end on every advance.  Drained behind each advance nothing is lost; drained once at the end the ring
    holds the last three of eight and n_lost = 5; a read of at most one record leaves the rest for the next."""
    case = _masked(dm, cfg0, [False, True, False, True, False], 4)
    r = _runner("device")(case, 3)
    assert r.infos == [(2 * k, 0) for k in (1, 2, 3, 4)]
    assert [(q["scene"].tolist(), q["seq"].tolist(), q["episode"].tolist(), lost) for q, lost in r.reads] == [([1, 3], [k, k], [k, k], 0) for k in range(4)]
    e = _runner("device")(case, 3, "end")
    assert e.infos == [(2, 0), (4, 1), (6, 3), (8, 5)]
    assert [(q["scene"].tolist(), q["seq"].tolist(), lost) for q, lost in e.reads] == [([3, 1, 3], [2, 3, 3], 5)]
    p = _runner("device")(case, 3, "end", 1)
    assert [(q["scene"].tolist(), q["seq"].tolist(), lost) for q, lost in p.reads] == [([3], [2], 5), ([1, 3], [3, 3], 0)]
    p = _runner("device")(case, 3, "each", 1)
    assert [(q["scene"].tolist(), lost) for q, lost in p.reads] == [([1], 0), ([3], 0)] * 4


@gpu
def test_start_is_the_record_the_ended_episode_ran_on(dm, cfg0):
    """M = 2, round robin, no contact and no clearance check: the restarts take records 1, 0, 1, 0, so the ENDED episodes ran on 0, 1, 0, 1."""
    si, po = te._ego(dm, 133.0, y=3.75, lane=1, ego_id=60), te._path(dm, 133.0, y=3.75)
    other = si.copy()
    other["period_last"] = 50.0
    sp = dm.default_episode_spawn()
    sp["n_starts"], sp["order"], sp["contact"], sp["check"], sp["clearance"] = 2, 1, 0, 0, 0.0
    case = _one(dm, cfg0, si, [po] * 4, te._em(dm), te._legs(dm), sp=sp, starts=(other, te._state0(dm)))
    for name in ("model", "device"):
        r = _runner(name)(case, 8)
        assert r.records["start"].tolist() == [0, 1, 0, 1] and r.records["episode"].tolist() == [0, 1, 2, 3], name
        assert [int(d.sstats["cur_start"][0]) for d in r.data] == [1, 0, 1, 0], name


@gpu
def test_a_set_call_in_the_middle_of_a_run_takes_the_start_records_in_force(dm, cfg0):
    """M = 2, round robin, scene 1 of three ends on every advance.  Behind the first advance cur_start is 0, 1, 0; a second pp_set_episode_log
    there starts a new log whose start_of is gathered from the spawn stats of every scene, each at its own stride: the next record of scene 1
    says start 1 (its neighbours' 0 would be a gather off by a record), the one after it 0."""
    sp = dm.default_episode_spawn()
    sp["n_starts"], sp["order"], sp["contact"], sp["check"], sp["clearance"] = 2, 1, 0, 0, 0.0
    plain = _masked(dm, cfg0, [False, True, False])
    other = plain.si.copy()
    other["period_last"] = 50.0
    case = _masked(dm, cfg0, [False, True, False], sp=sp, starts=(other, plain.state0.copy()))
    po, st = case.steps[0]
    pl, si, pool = elb.open_planner(case, 8)
    d, si, flags = elb.advance(pl, case, po, st, si, np.zeros(3, np.int32), pool)
    assert d.sstats["cur_start"].tolist() == [0, 1, 0] and pl.read_episode_log()[0]["start"].tolist() == [0]
    pl.tick()                                                                 # (the advance is adopted: nothing is staged)
    pl.set_episode_log(8)
    log = elm.EpisodeLog(dm.EpisodeRecord, 3, 8, d.sstats["cur_start"])
    assert pl.episode_log_info() == (0, 0)
    for k in range(2):
        d, si, flags = elb.advance(pl, case, po, st, si, flags, pool)
        log.append(d.stats, d.prev_in, d.tick, d.sstats)
    got, want = pl.read_episode_log(), log.read()
    pl.close()
    elb.same_reads([got], [want], "the second log")
    assert (got[0]["scene"].tolist(), got[0]["start"].tolist(), got[0]["episode"].tolist(), got[0]["seq"].tolist()) == ([1, 1], [1, 0], [1, 2], [0, 1])


@gpu
def test_score_begin_behind_the_set_call_and_in_the_middle_of_an_episode(dm, cfg0):
    """The log is set on a handle without a scorecard; pp_score_begin behind it gives the log its scorecards.  max_ticks = 3, the ego goes 110 ->
    111 -> 112 and restarts.  A second pp_score_begin behind advance 1 restarts the totals and the running episode's card with them: the
    record of advance 2 has ONE tick in it - the one on 112, no distance -, the record of advance 5 the whole second episode: three ticks, 2 m."""
    pos = [te._path(dm, 110.0 + k % 3) for k in range(6)]
    case = _one(dm, cfg0, te._ego(dm, 110.0, ego_id=20), pos, te._em(dm, 31, 3))
    scored = _one(dm, cfg0, te._ego(dm, 110.0, ego_id=20), pos, te._em(dm, 31, 3), score=True)      # (what elb.advance reads of a scored run)
    dt = float(case.model["dt"][0])
    pl, si, pool = elb.open_planner(case, 4)
    log = elm.EpisodeLog(dm.EpisodeRecord, 1, 4)
    pl.score_begin(dt)
    log.score_begin()
    flags, reads, want = np.zeros(1, np.int32), [], []
    for k, (po, st) in enumerate(case.steps):
        d, si, flags = elb.advance(pl, scored, po, st, si, flags, pool)
        log.fold(case.cfg, dt, d.prev_in, d.plan, d.state, d.pool, d.prev_flags)
        log.append(d.stats, d.prev_in, d.tick)
        reads.append(pl.read_episode_log()), want.append(log.read())
        if k == 1:
            pl.score_begin(dt)                                                # behind a staged advance, in the middle of the first episode
            log.score_begin()
            assert int(pl.rollout_score()["n_ticks"][0]) == 0
    pl.close()
    elb.same_reads(reads, want, "device against the model on its own records")
    assert [len(q) for q, _ in reads] == [0, 0, 1, 0, 0, 1]
    a, b = reads[2][0][0]["score"], reads[5][0][0]["score"]
    assert (int(a["n_ticks"]), float(a["dist"]), float(a["last_pos"]["x"])) == (1, 0.0, 112.0)
    assert (int(b["n_ticks"]), float(b["dist"]), float(b["last_pos"]["x"])) == (3, 2.0, 112.0)


def _ring_handle(dm, cap=None):
    cfg, m, sc, legs, rf = te._ring_scene(dm)
    pl = te._planner(dm, cfg, m, sc)
    pl.set_route(legs, rf)
    pl.score_begin(float(dm.default_ego_model()["dt"][0]))
    pl.set_episodes(te._em(dm))
    if cap is not None:
        pl.set_episode_log(cap)
    return pl, cfg, m, sc, legs, rf


@gpu
def test_closed_loop_on_the_ring_with_the_scorecard(dm):
    """8 egos, 160 advances, the scorecard on, a ring of 16 drained every 10 advances: every record is the model's on the device's own
    per-advance records - PlanOut and SceneState of every tick, SceneIn, flags and EpisodeStats of every advance - byte for byte, scorecard
    included; RolloutScore, which runs across the restarts, is untouched by it.  Every episode of an ego repeats its first, and so does its record."""
    n, ticks = te.RING_N, te.RING_TICKS
    pl, cfg, m, sc, legs, rf = _ring_handle(dm, 16)
    model, dt, none = dm.default_ego_model(), float(dm.default_ego_model()["dt"][0]), np.zeros(1, dm.ObPoint)
    log, want = elm.EpisodeLog(dm.EpisodeRecord, n, 16, None, True), rsm.new_scores(dm.RolloutScore, n)
    sin, flags, plan_p, got = pl.get_scene_in(), np.zeros(n, np.int32), dm.pinned_empty(n, dm.PlanOut), []
    start_in = sin.copy()
    for t in range(ticks):
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        plan, state = np.array(plan_p), pl.get_state()
        rsm.fold(want, cfg, dt, sin, plan, state, none, flags)
        log.fold(cfg, dt, sin, plan, state, none, flags)
        tick = pl.tick_id()
        pl.advance_async(model)
        stats = pl.episode_stats()
        log.append(stats, sin, tick)
        for s in np.flatnonzero(stats["age"] == 0):                       # §4k 6.: the totals' last ego moves to the start record; the episode's own card needs no patch
            want["last_pos"]["x"][s], want["last_pos"]["y"][s] = start_in["loc"]["globalpoint"]["x"][s], start_in["loc"]["globalpoint"]["y"][s]
            want["last_speed"][s] = start_in["loc"]["velocity"][s]
        assert pl.episode_log_info() == log.info(), t
        if t % 10 == 9:
            reads = [pl.read_episode_log()]
            elb.same_reads(reads, [log.read()], f"advance {t}")
            got.append(reads[0][0])
        sin, flags = pl.get_scene_in(), pl.ego_flags()
    assert pl.rollout_score().tobytes() == want.tobytes()
    total, lost = pl.episode_log_info()
    stats = pl.episode_stats()
    pl.close()
    recs = np.concatenate(got)
    assert lost == 0 and total == len(recs) == int(stats["n_episodes"].sum()) and (stats["n_episodes"] >= 3).all()
    assert sorted(set(recs["cause"].tolist())) == [20] and (recs["score"]["n_ticks"] == recs["age"]).all() and (np.diff(recs["seq"]) >= 0).all()
    for s in range(n):                                                    # every episode of an ego repeats its first (tests/test_episodes.py): so does its record
        mine = recs[recs["scene"] == s]
        assert mine["episode"].tolist() == list(range(len(mine))) and len(mine) == int(stats["n_episodes"][s])
        for rec in mine[1:]:
            a, b = rec.copy(), mine[0].copy()
            for f in ("episode", "seq", "tick"):
                a[f] = b[f]
            assert a.tobytes() == b.tobytes(), s


@gpu
def test_rollout_logs_what_its_parts_log(dm):
    """160 x (tick, advance) with a drain every 10 advances against pp_rollout(160) drained once: the same records, byte for byte."""
    n, ticks = te.RING_N, te.RING_TICKS
    pl, *_ = _ring_handle(dm, 16)
    model, parts = dm.default_ego_model(), []
    for t in range(ticks):
        pl.tick()
        pl.advance_async(model)
        if t % 10 == 9:
            q, lost = pl.read_episode_log()
            assert lost == 0
            parts.append(q)
    pl.close()
    parts = np.concatenate(parts)
    pl, *_ = _ring_handle(dm, 256)
    pl.rollout(ticks)
    whole, lost = pl.read_episode_log()
    pl.close()
    assert lost == 0 and len(whole) == len(parts) >= 3 * n and whole.tobytes() == parts.tobytes()


@gpu
def test_the_log_only_observes(dm):
    """60 advances of the ring with the scorecard on - the log on, the log on and then off, the log never set: the staged SceneIn, SceneState,
    EpisodeStats, RolloutScore and the trace are identical byte for byte."""
    outs = []
    for mode in ("on", "off again", "never"):
        pl, *_ = _ring_handle(dm, None if mode == "never" else 16)
        if mode == "off again":
            pl.set_episode_log(0)
        _, trace = pl.rollout(60, trace=True)
        pl.sync()
        outs.append((pl.get_scene_in(), pl.get_state(), pl.episode_stats(), pl.rollout_score(), np.array(trace)))
        if mode != "never":
            total, _ = pl.episode_log_info()
            assert total == (int(outs[-1][2]["n_episodes"].sum()) if mode == "on" else 0) and (mode != "on" or total > 0)
        pl.close()
    for other in outs[1:]:
        for a, b, name in zip(outs[0], other, ("SceneIn", "SceneState", "EpisodeStats", "RolloutScore", "trace")):
            assert a.tobytes() == b.tobytes(), name


@gpu
def test_errors_and_lifetime(dm, cfg0):
    case = _masked(dm, cfg0, [True, False, True], 1)
    po, st = case.steps[0]

    def go(pl, k=1):
        si, flags = pl.get_scene_in(), pl.ego_flags()
        for _ in range(k):
            _, si, flags = elb.advance(pl, case, po, st, si, flags, None)

    # a handle that never set a log, and one without episodes
    pl, _, _ = elb.open_planner(case)
    for call in (pl.read_episode_log, pl.episode_log_info):
        with pytest.raises(dm.PlannerError, match="error -4:"):
            call()
    pl.set_episodes(off=True)
    with pytest.raises(dm.PlannerError, match="error -4:"):                   # PP_ERR_STATE: episodes off
        pl.set_episode_log(4)
    pl.set_episode_log(0)                                                     # (off is off)
    pl.close()
    # every refusal leaves the log as it was: the run goes on like the reference run.  (go() leaves its last advance staged.)
    pl, _, _ = elb.open_planner(case, 8)
    ref, _, _ = elb.open_planner(case, 8)
    go(pl), go(ref)
    for cap in (-1, dm.EPISODE_LOG_MAX + 1):                                  # PP_ERR_ARG
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_episode_log(cap)
    for cap in (4, 0):                                                        # PP_ERR_STATE: an update is staged
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.set_episode_log(cap)
    go(pl, 2), go(ref, 2)
    assert pl.episode_log_info() == ref.episode_log_info() == (6, 0)
    (a, la), (b, lb) = pl.read_episode_log(), ref.read_episode_log()
    assert a.tobytes() == b.tobytes() and la == lb == 0 and a["scene"].tolist() == [0, 2] * 3 and a["seq"].tolist() == [0, 0, 1, 1, 2, 2]
    ref.close()
    # readable after off: the two records of one more advance stay, later advances append nothing
    go(pl)
    pl.tick()
    pl.set_episode_log(0)
    go(pl, 2)
    assert pl.episode_log_info() == (8, 0)
    q, lost = pl.read_episode_log()
    assert (q["scene"].tolist(), q["seq"].tolist(), lost) == ([0, 2], [3, 3], 0) and pl.episode_stats()["n_episodes"][[0, 2]].tolist() == [6, 6]
    # a second set call starts from total = 0, seq = 0, nothing unread - and episode numbers go on: they are the scene's, not the log's
    pl.tick()
    pl.set_episode_log(2)
    assert pl.episode_log_info() == (0, 0) and len(pl.read_episode_log()[0]) == 0
    go(pl, 2)
    q, lost = pl.read_episode_log()
    assert pl.episode_log_info() == (4, 2) and (q["scene"].tolist(), q["seq"].tolist(), q["episode"].tolist(), lost) == ([0, 2], [1, 1], [7, 7], 2)
    # pp_set_episodes, pp_set_episode_spawn (NULL included) and pp_set_egos switch it off
    for off in ("episodes", "spawn", "no spawn", "egos"):
        pl.tick()
        pl.set_episode_log(4)
        go(pl)
        assert pl.episode_log_info() == (2, 0), off
        pl.tick()
        if off == "episodes":
            pl.set_episodes(case.em)
        elif off == "spawn":
            pl.set_episode_spawn(elb.esb.neutral(dm.EpisodeSpawn))
        elif off == "no spawn":
            pl.set_episode_spawn(None)
        else:
            si, pool, W = case.laid_out()
            pl.set_egos(dict(scene_in=si, obs_pool=pool, mot_pool=None, n_obs=W), with_motion=False)
            pl.set_route(*elb.ab._route(case.route, case.n))
            pl.set_state(case.state0)
            pl.set_episodes(case.em)
        before = pl.episode_stats()["n_episodes"][[0, 2]]
        go(pl, 2)
        assert (pl.episode_stats()["n_episodes"][[0, 2]] == before + 2).all() and pl.episode_log_info() == (2, 0), off
    pl.close()
