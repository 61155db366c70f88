"""The score trace: a ring of the last scored ticks per scene, frozen shortly after an incident.

CPU tests: hand-derived known answers on the numpy model (tests/score_trace_model.py), the ABI mirror, the defaults, a null handle.
GPU tests: k_score_ego<., true> inside a real tick against the model, byte for byte (tests/score_trace_backends.py) - the known
answers, the 64-lane stride with the minimum on the last entry, one scene alone and inside batches of 5 and 300, with and without the
episode log, off = the engine without it, the life cycle, the error paths, and the contact loop of §4l.

Every case stands on hw = 1 (Vehicle_Width 2), dt_score = 0.5 and an ego on the x axis, so that clearances and decelerations are
exact: an obstacle at distance D with radius r gives clearance D - r - 1."""
import ctypes as C
import math

import numpy as np
import pytest

import coupling_backends as cb
import rollout_score_model as rsm
import score_trace_backends as stb
import score_trace_model as stm

gpu = pytest.mark.gpu
INF = math.inf
DT = 0.5
COLLISION, NEAR, FLAG, BRAKE = 1, 2, 4, 8
ULP1 = 2.0 ** -52          # nextafter(1, 2) - 1


@pytest.fixture()
def cfg1(dm):
    cfg = cb.config()
    cfg["Vehicle_Width"] = 2.0
    return cfg


def _tm(dm, depth=4, post=1, trigger=15, flag_mask=0, near=0.5, brake=6.0):
    m = np.zeros(1, dm.ScoreTraceModel)
    m["depth"], m["post"], m["trigger"], m["flag_mask"], m["near"], m["brake"] = depth, post, trigger, flag_mask, near, brake
    return m


def _runner(name):
    return (stb.ModelBackend() if name == "model" else stb.DeviceBackend()).run


def _t(cfg, x, v, obs=(), **kw):
    """One scene on the x axis at (x, 0) with v km/h; obs: (distance ahead, radius)."""
    return cb.tick(cfg, [(x, 0.0, v, [(x + d, 0.0, r) for d, r in obs])], **kw)


def _hd(info, s=0):
    return tuple(int(info[f][s]) for f in ("n_written", "state", "trigger_k", "trigger", "post_left", "n_trigger_ticks"))


def _causes(ring):
    return [int(m) >> 8 for m in ring["marks"]]


# ---------------------------------------------------------------------------------------------------------------
# known answers, asserted on both legs
def _kat_three_ticks(dm, cfg, run):
    """depth 4, post 1, every cause armed, near 0.5, brake 6.
    tick 0 (k 0): ego x 100 at 36 km/h, obstacle 10 m ahead, radius 1: clearance 10 - 1 - 1 = 8; k == 0, so no brake.  Cause 0.
                  header (n_written 1, armed, -1, 0, 0, 0 trigger ticks).
    tick 1 (k 1): ego x 101 at 18 km/h: a = (18 - 36) / 3.6 / 0.5 = -10, -a = 10 >= 6: BRAKE; obstacle 2.25 m ahead, radius 1:
                  clearance 0.25 <= 0.5: NEAR, > 0: no collision.  Cause 10.  Armed -> counting: trigger_k 1, trigger 10, post_left 1;
                  header (2, 1, 1, 10, 1, 1).
    tick 2 (k 2): ego x 102 at 18 km/h (a = 0); obstacle 1 m ahead, radius 1: clearance -1: COLLISION | NEAR = 3.  A post tick, not
                  a second trigger: post_left 0, frozen; header (3, 2, 1, 10, 0, 2).
    tick 3 (k 3): the same again: counted (3 trigger ticks), not recorded: header (3, 2, 1, 10, 0, 3), the ring as before."""
    ticks = [_t(cfg, 100.0, 36.0, [(10.0, 1.0)]), _t(cfg, 101.0, 18.0, [(2.25, 1.0)]), _t(cfg, 102.0, 18.0, [(1.0, 1.0)]), _t(cfg, 102.0, 18.0, [(1.0, 1.0)])]
    r = run(cfg, DT, _tm(dm), ticks)
    assert [_hd(i) for i in r.info] == [(1, 0, -1, 0, 0, 0), (2, 1, 1, 10, 1, 1), (3, 2, 1, 10, 0, 2), (3, 2, 1, 10, 0, 3)]
    ring = r.rings[3][0]
    assert r.rings[2][0].tobytes() == ring.tobytes() and len(ring) == 3
    assert ring["k"].tolist() == [0, 1, 2] and ring["tick"].tolist() == [1, 2, 3] and ring["x"].tolist() == [100.0, 101.0, 102.0] and ring["y"].tolist() == [0.0] * 3
    assert ring["v"].tolist() == [36.0, 18.0, 18.0] and ring["clearance"].tolist() == [8.0, 0.25, -1.0] and ring["obs"].tolist() == [0, 0, 0]
    assert _causes(ring) == [0, 10, 3] and ring["behavior"].tolist() == [1, 1, 1] and ring["flags"].tolist() == [0, 0, 0]
    assert [int(s["n_ticks"][0]) for s in r.score] == [1, 2, 3, 4] and int(r.score[3]["n_collision_ticks"][0]) == 2


def _kat_ties_and_one_ulp_beside_them(dm, cfg, run):
    """clearance == 0, clearance == near and -a == brake trigger; one ulp on the other side of each does not.  Distances: sqrt(dx dx)
    is exact, so an obstacle (D ahead, radius r) has d = D - r, exactly representable here."""
    two = lambda second, v1=36.0: [_t(cfg, 0.0, 36.0), _t(cfg, 0.0, v1, second)]
    # collision: D 5, r 4: d = 1, clearance 0.  Beside it: D = 1 + 2^-52, r 0: clearance 2^-52
    r = run(cfg, DT, _tm(dm, trigger=COLLISION, post=0), two([(5.0, 4.0)]))
    assert _hd(r.info[1]) == (2, 2, 1, COLLISION, 0, 1) and r.rings[1][0]["clearance"].tolist() == [INF, 0.0]
    r = run(cfg, DT, _tm(dm, trigger=COLLISION, post=0), two([(1.0 + ULP1, 0.0)]))
    assert _hd(r.info[1]) == (2, 0, -1, 0, 0, 0) and r.rings[1][0]["clearance"].tolist() == [INF, ULP1]
    # near: D 5, r 3.5: clearance 0.5 == near; near one ulp below 0.5: nothing
    r = run(cfg, DT, _tm(dm, trigger=NEAR, post=0, near=0.5), two([(5.0, 3.5)]))
    assert _hd(r.info[1]) == (2, 2, 1, NEAR, 0, 1) and r.rings[1][0]["clearance"].tolist() == [INF, 0.5]
    r = run(cfg, DT, _tm(dm, trigger=NEAR, post=0, near=math.nextafter(0.5, 0.0)), two([(5.0, 3.5)]))
    assert _hd(r.info[1]) == (2, 0, -1, 0, 0, 0)
    # brake: 36 -> 18 km/h in 0.5 s: a = -18 / 3.6 / 0.5 = -10 exactly; brake 10 triggers, one ulp above 10 does not; the first tick (k = 0) never brakes
    assert (18.0 - 36.0) / 3.6 / DT == -10.0
    r = run(cfg, DT, _tm(dm, trigger=BRAKE, post=0, brake=10.0), two([], 18.0))
    assert _hd(r.info[1]) == (2, 2, 1, BRAKE, 0, 1) and _causes(r.rings[1][0]) == [0, BRAKE]
    r = run(cfg, DT, _tm(dm, trigger=BRAKE, post=0, brake=math.nextafter(10.0, INF)), two([], 18.0))
    assert _hd(r.info[1]) == (2, 0, -1, 0, 0, 0) and _causes(r.rings[1][0]) == [0, 0]
    # a cause outside `trigger` is no cause: a collision with only BRAKE armed
    r = run(cfg, DT, _tm(dm, trigger=BRAKE, post=0), two([(1.0, 1.0)]))
    assert _hd(r.info[1]) == (2, 0, -1, 0, 0, 0) and _causes(r.rings[1][0]) == [0, 0] and r.rings[1][0]["clearance"].tolist() == [INF, -1.0]


def _kat_nan_pose_and_no_obstacle(dm, cfg, run):
    """A NaN pose: every d_j is NaN, so the tick has no clearance, and (NaN - v) / 3.6 / dt compares false - in this tick and, through
    last_speed, in the next: no cause, and the record is still written.  A tick with no obstacle: clearance +inf, obs -1, ob_type 0.
    The device leg keeps x finite: a resident record with a NaN POSITION would send the tick's own front kernels through it, which no
    test of this project does (tests/test_traffic_follow.py); its NaN is the speed (tests/test_rollout_score.py: the Planning kernel
    only scales its aim distance by it) and the obstacle's x, which give the same two NaN comparisons and the same missing clearance."""
    x = math.nan if run.__self__.name == "model" else 0.5
    nan = cb.tick(cfg, [(x, 0.0, math.nan, [(math.nan, 0.0, 1.0)])])
    ticks = [_t(cfg, 0.0, 36.0, [(10.0, 1.0)]), nan, _t(cfg, 1.0, 0.0)]
    r = run(cfg, DT, _tm(dm), ticks)
    assert [_hd(i) for i in r.info] == [(1, 0, -1, 0, 0, 0), (2, 0, -1, 0, 0, 0), (3, 0, -1, 0, 0, 0)]
    ring = r.rings[2][0]
    assert (math.isnan(ring["x"][1]) or x == 0.5) and math.isnan(ring["v"][1]) and ring["y"][1] == 0.0
    assert ring["clearance"].tolist() == [8.0, INF, INF] and ring["obs"].tolist() == [0, -1, -1] and ring["ob_type"].tolist() == [0, 0, 0] and _causes(ring) == [0, 0, 0]


def _seven(cfg):
    """Seven ticks of an ego that drives 1 m per tick at 36 km/h towards a wall at x = 9.5 (radius 1): clearance 7.5 - k; k = 7: none."""
    return [_t(cfg, float(k), 36.0, [(9.5 - k, 1.0)]) for k in range(7)]


def _kat_depth_1_2_3_over_seven_ticks(dm, cfg, run):
    """Slot wrap and oldest-first order of a plain ring (trigger 0 never freezes)."""
    for depth in (1, 2, 3):
        r = run(cfg, DT, _tm(dm, depth=depth, post=0, trigger=0), _seven(cfg))
        for k in range(7):
            assert _hd(r.info[k]) == (k + 1, 0, -1, 0, 0, 0)
            assert r.rings[k][0]["k"].tolist() == list(range(max(0, k + 1 - depth), k + 1)), (depth, k)
            assert r.rings[k][0]["clearance"].tolist() == [7.5 - j for j in range(max(0, k + 1 - depth), k + 1)]


def _kat_post_0_and_post_depth_minus_1(dm, cfg, run):
    """The wall's clearance is <= 2.5 from k = 5 on (near 2.5, trigger NEAR).  post 0: frozen on the triggering tick, the newest
    record.  post depth - 1 = 2: ticks 5, 6 and the first tick of a second pass (k 7) fill the ring: the triggering record is the oldest."""
    ticks = _seven(cfg) + _seven(cfg)[:3]
    r = run(cfg, DT, _tm(dm, depth=3, post=0, trigger=NEAR, near=2.5), ticks)
    # (two ticks with the cause: k 5 and - counted on the frozen ring - k 6)
    assert _hd(r.info[9]) == (6, 2, 5, NEAR, 0, 2) and r.rings[9][0]["k"].tolist() == [3, 4, 5] and _causes(r.rings[9][0]) == [0, 0, NEAR]
    r = run(cfg, DT, _tm(dm, depth=3, post=2, trigger=NEAR, near=2.5), ticks)
    assert [_hd(r.info[k]) for k in (5, 6, 7, 9)] == [(6, 1, 5, NEAR, 2, 1), (7, 1, 5, NEAR, 1, 2), (8, 2, 5, NEAR, 0, 2), (8, 2, 5, NEAR, 0, 2)]
    assert r.rings[9][0]["k"].tolist() == [5, 6, 7] and _causes(r.rings[9][0]) == [NEAR, NEAR, 0] and r.rings[9][0]["clearance"].tolist() == [2.5, 1.5, 7.5]


def _kat_second_cause_and_rearm(dm, cfg, run):
    """A second cause while counting post does not re-trigger and is counted.  A re-arming read keeps ring and n_written; the next
    incident triggers with its lead-in."""
    hit, free = lambda x: _t(cfg, x, 36.0, [(1.0, 1.0)]), lambda x: _t(cfg, x, 36.0, [(9.0, 1.0)])
    ticks = [free(0.0), hit(1.0), hit(2.0), free(3.0), free(4.0), free(5.0), hit(6.0), free(7.0)]
    r = run(cfg, DT, _tm(dm, depth=4, post=2, trigger=COLLISION), ticks, rearm={4: [0]})
    assert [_hd(i) for i in r.info] == [(1, 0, -1, 0, 0, 0), (2, 1, 1, 1, 2, 1), (3, 1, 1, 1, 1, 2), (4, 2, 1, 1, 0, 2), (4, 0, -1, 0, 0, 2),
                                        (5, 0, -1, 0, 0, 2), (6, 1, 6, 1, 2, 3), (7, 1, 6, 1, 1, 3)]
    assert r.rings[3][0]["k"].tolist() == [0, 1, 2, 3] and r.rings[4][0].tobytes() == r.rings[3][0].tobytes()      # tick 4 fell on a frozen ring
    assert r.rings[7][0]["k"].tolist() == [3, 5, 6, 7] and _causes(r.rings[7][0]) == [0, 0, 1, 0]                  # k 4 is missing: it was not recorded


KATS = [_kat_three_ticks, _kat_ties_and_one_ulp_beside_them, _kat_nan_pose_and_no_obstacle, _kat_depth_1_2_3_over_seven_ticks,
        _kat_post_0_and_post_depth_minus_1, _kat_second_cause_and_rearm]


@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, cfg1, kat):
    kat(dm, cfg1, _runner("model"))


def test_flag_cause_marks_and_types_on_the_model(dm, cfg1):
    """What only a crafted PlanOut / SceneState / flag word can say (the device leg of these is the closed loops below): the flag cause
    under its mask, the four mark bits, the behaviour as it is (not clamped), the type of the obstacle the minimum named."""
    t0 = _t(cfg1, 0.0, 36.0, [(9.0, 1.0), (5.0, 1.0)], behavior=9, afresh=1, desaccVd=2, flags=4)
    t0.pool["type"][:] = [7, cb.fl.OB_PEER | 3]
    t1 = _t(cfg1, 1.0, 36.0, [(9.0, 1.0)], behavior=-2, ob_flag=1, flags=4 | 16)
    model, n = _tm(dm, depth=2, post=0, trigger=FLAG, flag_mask=16), 1
    scores, (rings, info) = rsm.new_scores(dm.RolloutScore, n), stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, 2)
    stats = np.zeros(1, dm.EpisodeStats)
    for k, (t, age) in enumerate(((t0, 0), (t1, 3))):
        po, st, flags = cb._crafted(t)
        stats["age"] = age
        stm.step(rings, info, model, scores, cfg1, DT, 41 + k, t.si, po, st, t.pool, flags, stats)
        rsm.fold(scores, cfg1, DT, t.si, po, st, t.pool, flags)
    ring = stm.oldest_first(rings, info, 0)
    assert _hd(info) == (2, 2, 1, FLAG, 0, 1) and ring["tick"].tolist() == [41, 42] and ring["flags"].tolist() == [4, 20]
    assert ring["marks"].tolist() == [stm.TICK_REPLAN | stm.TICK_DESACC | stm.TICK_START, stm.TICK_OB_FLAG | FLAG << 8]
    assert ring["behavior"].tolist() == [9, -2] and ring["obs"].tolist() == [1, 0] and ring["ob_type"].tolist() == [cb.fl.OB_PEER | 3, 0]
    assert ring["clearance"].tolist() == [3.0, 7.0]


def test_abi_mirror_defaults_and_null_handle(dm):
    lib = dm.load_library()
    assert [lib.pp_sizeof(k) for k in (35, 36, 37)] == [dm.ScoreTraceModel.itemsize, dm.ScoreTick.itemsize, dm.ScoreTraceInfo.itemsize] == [32, 64, 32]
    assert [dm.ScoreTick.fields[f][1] for f in ("k", "flags", "tick", "x", "y", "v", "clearance", "obs", "ob_type", "behavior", "marks")] == \
        [0, 4, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    d = dm.default_score_trace()[0]
    assert (int(d["depth"]), int(d["post"]), int(d["trigger"]), int(d["flag_mask"]), float(d["near"]), float(d["brake"])) == (64, 8, COLLISION, 0, 0.5, 6.0)
    assert (dm.SCORE_TRACE_MAX, dm.TRACE_COLLISION, dm.TRACE_NEAR, dm.TRACE_FLAG, dm.TRACE_BRAKE) == (256, 1, 2, 4, 8)
    buf, m = np.zeros(4, dm.ScoreTick), dm.default_score_trace()
    assert lib.pp_set_score_trace(None, m.ctypes.data) == dm.PP_ERR_ARG
    assert lib.pp_get_score_trace_info(None, buf.ctypes.data, 1) == dm.PP_ERR_ARG
    assert lib.pp_read_score_trace(None, 0, buf.ctypes.data, 4, None, 0) == dm.PP_ERR_ARG
    lib.pp_default_score_trace(None)


# ---------------------------------------------------------------------------------------------------------------
# the device against the model
@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg1, kat):
    kat(dm, cfg1, _runner("device"))


M_OBS = (0, 1, 63, 64, 65, 128, 129)


def _stride_case(cfg, m):
    """Three ticks of one ego with m obstacles, FAR ones 20 + j m ahead (radius 1) and - the LAST entry - the nearest one: 6, then 2.25
    (near), then 1 m ahead (contact).  Every entry has a type of its own, 100 + j."""
    ticks = []
    for k, last in enumerate((6.0, 2.25, 1.0)):
        obs = [(20.0 + j, 1.0) for j in range(m)]
        if m:
            obs[-1] = (last, 1.0)
        t = _t(cfg, float(k), 36.0, obs)
        t.pool["type"][:m] = 100 + np.arange(m)
        ticks.append(t)
    return ticks


_ALONE = {}


def _alone(dm, cfg):
    """Every obstacle count alone on the device (once per process): the minimum on the last entry, its type loaded from there."""
    if not _ALONE:
        model = _tm(dm, depth=4, post=1, trigger=COLLISION | NEAR)
        for m in M_OBS:
            r = stb.DeviceBackend().run(cfg, DT, model, _stride_case(cfg, m))
            ring = r.rings[2][0]
            if m:
                assert ring["obs"].tolist() == [m - 1] * 3 and ring["ob_type"].tolist() == [100 + m - 1] * 3 and ring["clearance"].tolist() == [4.0, 0.25, -1.0]
                assert _hd(r.info[2]) == (3, 2, 1, NEAR, 0, 2) and _causes(ring) == [0, NEAR, COLLISION | NEAR]
            else:
                assert ring["obs"].tolist() == [-1] * 3 and ring["ob_type"].tolist() == [0] * 3 and ring["clearance"].tolist() == [INF] * 3 and _hd(r.info[2]) == (3, 0, -1, 0, 0, 0)
            _ALONE[m] = r
        _ALONE["model"] = model
    return _ALONE


@gpu
def test_obstacle_counts_with_the_minimum_on_the_last_entry(dm, cfg1):
    """0, 1, 63 | 64 | 65, 128 | 129 obstacles: the 64-lane stride, the last lane of a full pass, the only lane of a short one - and the
    ob_type load of the entry the wave minimum named."""
    assert sorted(k for k in _alone(dm, cfg1) if k != "model") == list(M_OBS)


@gpu
@pytest.mark.parametrize("n", [5, 300])
def test_a_scene_gives_the_same_bytes_alone_and_inside_a_batch(dm, cfg1, n):
    """5: one block of four waves and the first wave of the next; 300: 75 blocks.  Scene s is the case of M_OBS[s % 7]: the waves of a
    block have different trip counts."""
    alone = _alone(dm, cfg1)
    cases = [M_OBS[s % len(M_OBS)] for s in range(n)]
    ticks = stb.batch_ticks([_stride_case(cfg1, m) for m in cases])
    r = stb.DeviceBackend().run(cfg1, DT, alone["model"], ticks)
    for k in range(3):
        for s, m in enumerate(cases):
            a = alone[m]
            assert r.info[k][s].tobytes() == a.info[k][0].tobytes() and r.rings[k][s].tobytes() == a.rings[k][0].tobytes(), (n, k, s, m)
            assert r.score[k][s].tobytes() == a.score[k][0].tobytes(), (n, k, s, m)


def _crafted_run(dm, cfg, ticks, model, after=None):
    """The ticks through one handle; model None: the trace is never set.  after: {tick index: callable(pl)} between two ticks.  Returns
    (RolloutScore behind every tick, (headers, rings) behind every tick or None)."""
    pl = stb.open_planner(cfg, ticks, model, True, DT)
    keep, scores, traces = [], [], []
    for k, t in enumerate(ticks):
        stb.feed(pl, t, keep)
        scores.append(pl.rollout_score())
        traces.append(stb.read_all(pl, len(t.si)) if model is not None else None)
        if after and k in after:
            after[k](pl)
    pl.close()
    return scores, traces


@gpu
def test_off_is_the_engine_without_it(dm, cfg1):
    """The RolloutScore records with the recorder on are those of a handle that never set it, byte for byte; after
    pp_set_score_trace(NULL) headers and rings no longer change while the scorecard runs on; a handle that never set it answers the
    reads with PP_ERR_STATE."""
    ticks = stb.batch_ticks([_stride_case(cfg1, m) + _stride_case(cfg1, m) for m in (65, 0, 1, 129, 64)])
    model = _tm(dm, depth=4, post=1, trigger=COLLISION | NEAR)
    never, _ = _crafted_run(dm, cfg1, ticks, None)
    on, _ = _crafted_run(dm, cfg1, ticks, model)
    off, tr = _crafted_run(dm, cfg1, ticks, model, {1: lambda pl: pl.set_score_trace(off=True)})
    for k in range(len(ticks)):
        assert never[k].tobytes() == on[k].tobytes() == off[k].tobytes(), k
    for k in range(2, len(ticks)):
        assert tr[k][0].tobytes() == tr[1][0].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(tr[k][1], tr[1][1])), k
    assert _hd(tr[1][0], 0) == (2, 1, 1, NEAR, 1, 1)                       # (it was caught counting post, and stays there)
    pl = stb.open_planner(cfg1, ticks, None, True, DT)
    for call in (pl.score_trace_info, lambda: pl.read_score_trace(0, cap=4)):
        with pytest.raises(dm.PlannerError, match="error -4:"):
            call()
    pl.set_score_trace(off=True)                                            # (off is off, and still no set call)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.score_trace_info()
    pl.close()


@gpu
def test_set_before_or_after_score_begin_and_only_while_scoring(dm, cfg1):
    """Legal on either side of pp_score_begin, and it records only while the scorecard is on: ticks before pp_score_begin and behind
    pp_score_end leave headers and rings alone; pp_score_begin resets the headers."""
    ticks = _seven(cfg1)
    model = _tm(dm, depth=3, post=0, trigger=0)
    pl, keep = stb.open_planner(cfg1, ticks, model, False), []
    stb.feed(pl, ticks[0], keep)
    assert _hd(pl.score_trace_info()) == (0, 0, -1, 0, 0, 0) and len(pl.read_score_trace(0)[0]) == 0
    pl.score_begin(DT)
    stb.feed(pl, ticks[1], keep), stb.feed(pl, ticks[2], keep)
    ring, hd = pl.read_score_trace(0)
    assert _hd(hd.reshape(1)) == (2, 0, -1, 0, 0, 0) and ring["k"].tolist() == [0, 1] and ring["tick"].tolist() == [2, 3] and ring["clearance"].tolist() == [6.5, 5.5]
    pl.score_end()
    stb.feed(pl, ticks[3], keep)
    assert pl.read_score_trace(0)[0].tobytes() == ring.tobytes() and _hd(pl.score_trace_info()) == (2, 0, -1, 0, 0, 0)
    pl.score_begin(DT)                                                      # the totals restart, and the headers with them
    assert _hd(pl.score_trace_info()) == (0, 0, -1, 0, 0, 0)
    pl.set_score_trace(_tm(dm, depth=2, post=0, trigger=0))                 # after pp_score_begin, another depth
    for t in ticks[4:7]:
        stb.feed(pl, t, keep)
    ring, hd = pl.read_score_trace(0)
    assert _hd(hd.reshape(1)) == (3, 0, -1, 0, 0, 0) and ring["k"].tolist() == [1, 2] and ring["clearance"].tolist() == [2.5, 1.5]
    pl.close()


@gpu
def test_error_paths_change_nothing(dm, cfg1):
    ticks = stb.batch_ticks([_stride_case(cfg1, m) for m in (1, 65)])
    model = _tm(dm, depth=4, post=1, trigger=COLLISION | NEAR)
    pl, keep = stb.open_planner(cfg1, ticks, model, True, DT), []
    for t in ticks:
        stb.feed(pl, t, keep)
    info, rings = stb.read_all(pl, 2)
    assert _hd(info, 1) == (3, 2, 1, NEAR, 0, 2)
    bad = [dict(depth=0), dict(depth=257), dict(post=-1), dict(post=4), dict(trigger=16), dict(trigger=-1), dict(flag_mask=32), dict(near=INF),
           dict(near=math.nan), dict(brake=0.0), dict(brake=-1.0), dict(brake=INF), dict(brake=math.nan)]
    for kw in bad:
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_score_trace(_tm(dm, **kw))
    for scene in (-1, 2):                                                   # PP_ERR_ARG: no such resident scene
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.read_score_trace(scene, rearm=True)
    with pytest.raises(dm.PlannerError, match="error -3:"):                 # PP_ERR_CAPACITY: three records, room for two - and no re-arm
        pl.read_score_trace(1, rearm=True, cap=2)
    lib, out = dm.load_library(), np.zeros(2, dm.ScoreTraceInfo)
    assert lib.pp_get_score_trace_info(pl.h, None, 1) == dm.PP_ERR_ARG and lib.pp_get_score_trace_info(pl.h, out.ctypes.data, 3) == dm.PP_ERR_ARG
    assert lib.pp_read_score_trace(pl.h, 0, None, 4, None, 0) == dm.PP_ERR_ARG and lib.pp_read_score_trace(pl.h, 0, out.ctypes.data, -1, None, 0) == dm.PP_ERR_ARG
    again, rings2 = stb.read_all(pl, 2)
    assert again.tobytes() == info.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(rings, rings2))
    stb.feed(pl, ticks[2], keep)                                            # the model in force is still the first one: frozen rings stay frozen
    assert _hd(pl.score_trace_info(), 1) == (3, 2, 1, NEAR, 0, 3)
    pl.close()


# ---------------------------------------------------------------------------------------------------------------
# closed loops: the model stepped over the device's own per-tick records
def _follow(dm, pl, cfg, model, n, ticks, rings, info, scores, advance, episodes, between=None, hold=None, t0=0):
    """`ticks` x (tick, advance) on a streamed handle with the scorecard and the trace on; rings / info / scores: the model's, stepped
    in place over PlanOut, SceneState, snapshot, flag words and EpisodeStats of every tick as the device had them.  hold: ticks t at
    which the device must equal the model (default: all).  between: {t: callable(pl)} behind advance t.  Returns the per-tick records."""
    dt, plan_p, recs = float(advance["dt"][0]), dm.pinned_empty(n, dm.PlanOut), []
    for t in range(t0, t0 + ticks):
        sin, flags = pl.get_scene_in(), pl.ego_flags()
        stats = pl.episode_stats() if episodes else None
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        plan, state = np.array(plan_p), pl.get_state()
        total = int((sin["obs_off"] + sin["obs_n"]).max()) if len(sin) else 0
        now = pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, total) if total else np.zeros(1, dm.ObPoint)
        stm.step(rings, info, model, scores, cfg, dt, pl.tick_id(), sin, plan, state, now, flags, stats)
        rsm.fold(scores, cfg, dt, sin, plan, state, now, flags)
        recs.append(dict(sin=sin, plan=plan, state=state, now=now, flags=flags, stats=stats))
        if hold is None or t in hold:
            got_info, got_rings = stb.read_all(pl, n)
            stb.same(got_info, info, f"tick {t}: headers")
            for s in range(n):
                stb.same(got_rings[s], stm.oldest_first(rings, info, s), f"tick {t}, scene {s}: ring")
        pl.advance_async(advance)
        if episodes:                                                        # §4k 6.: a restart moves the totals' last ego to the start record
            after, out = pl.episode_stats(), pl.get_scene_in()
            for s in np.flatnonzero(after["n_episodes"] > stats["n_episodes"]):
                scores["last_pos"]["x"][s], scores["last_pos"]["y"][s] = out["loc"]["globalpoint"]["x"][s], out["loc"]["globalpoint"]["y"][s]
                scores["last_speed"][s] = out["loc"]["velocity"][s]
        if between and t in between:
            between[t](pl)
    return recs


def _contact_handle(dm, r, model, log=False, trace=True):
    import test_episode_spawn as tes
    pl = tes._planner(dm, r)
    if log:
        pl.set_episode_log(64)
    if trace:
        pl.set_score_trace(model)
    pl.score_begin(float(dm.default_ego_model()["dt"][0]))
    return pl


_LOOP = {}


def _contact_loop(dm):
    """§4l's contact scenario, 60 advances, trigger COLLISION, depth 32, post 2, the episode log off and on (once per process)."""
    if not _LOOP:
        import test_episode_spawn as tes
        import test_traffic as tt
        r, n, adv = tes._loop_scene(dm), tt.F_N, dm.default_ego_model()
        model = _tm(dm, depth=32, post=2, trigger=COLLISION)
        for log in (False, True):
            pl = _contact_handle(dm, r, model, log)
            scores, (rings, info) = rsm.new_scores(dm.RolloutScore, n), stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, 32)
            recs = _follow(dm, pl, r["cfg"], model, n, 60, rings, info, scores, adv, True, hold=set(range(0, 60, 7)) | {59})
            got_info, got_rings = stb.read_all(pl, n)
            _LOOP[log] = dict(info=got_info, rings=got_rings, score=pl.rollout_score(), recs=recs, want_score=scores.copy(),
                              log=pl.read_episode_log()[0] if log else None, stats=pl.episode_stats())
            pl.close()
        _LOOP["scene"], _LOOP["model"] = r, model
    return _LOOP


@gpu
def test_contact_loop_freezes_every_ring_behind_its_contact(dm):
    """16 ring followers with their vehicles turned round; first episodes end on contact at ages 37 - 47.  Every scene ends frozen; the
    record at trigger_k has clearance <= 0 and the actor's type; the two records after it are there and no third; every ring is the
    model's on the device's own per-tick records (held inside _follow), and so is the RolloutScore."""
    import test_traffic as tt
    L = _contact_loop(dm)[False]
    info, n = L["info"], tt.F_N
    print("trigger_k", info["trigger_k"].tolist(), "n_written", info["n_written"].tolist(), "trigger ticks", info["n_trigger_ticks"].tolist())
    assert (info["state"] == 2).all() and (info["trigger"] == COLLISION).all() and (info["post_left"] == 0).all()
    assert L["score"].tobytes() == L["want_score"].tobytes()
    assert np.array_equal(info["trigger_k"], L["score"]["first_collision_tick"]) and (info["trigger_k"] >= 36).all() and (info["trigger_k"] <= 46).all()
    for s in range(n):
        ring, k = L["rings"][s], int(info["trigger_k"][s])
        assert int(info["n_written"][s]) == k + 3 and len(ring) == min(k + 3, 32)
        assert ring["k"].tolist() == list(range(k + 3 - len(ring), k + 3))                      # two records behind the triggering one, no third
        hit = ring[ring["k"] == k][0]
        assert float(hit["clearance"]) <= 0 and int(hit["ob_type"]) == tt.F_TYPE and int(hit["obs"]) == 0 and int(hit["marks"]) >> 8 == COLLISION
        assert (ring["clearance"][ring["k"] < k] > 0).all()
        assert int(ring[ring["k"] == k + 1][0]["marks"]) & stm.TICK_START, "the tick behind the ending advance read a start record"
        assert not (ring["marks"][(ring["k"] <= k) & (ring["k"] > 0)] & stm.TICK_START).any()
        assert np.array_equal(np.diff(ring["tick"]), np.ones(len(ring) - 1, np.int64))


@gpu
def test_with_the_episode_log_on_nothing_else_changes(dm):
    """k_score_ego<true, true> against <false, true>: headers and rings byte for byte; RolloutScore - and, with the log on, the
    episodes' own scorecards - byte for byte what the same run gives with the recorder off."""
    import test_traffic as tt
    L = _contact_loop(dm)
    a, b = L[False], L[True]
    assert a["info"].tobytes() == b["info"].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a["rings"], b["rings"]))
    assert a["score"].tobytes() == b["score"].tobytes() and len(b["log"]) >= tt.F_N
    for log in (False, True):                                               # the same run with the recorder never set
        pl, adv = _contact_handle(dm, L["scene"], None, log, trace=False), dm.default_ego_model()
        for _ in range(60):                                                 # (as _follow: 60 scored ticks, an advance behind each)
            pl.tick()
            pl.advance_async(adv)
        assert pl.rollout_score().tobytes() == L[log]["score"].tobytes(), log
        assert pl.episode_stats().tobytes() == L[log]["stats"].tobytes(), log
        if log:
            assert pl.read_episode_log()[0].tobytes() == b["log"].tobytes()
        pl.close()


@gpu
def test_contact_loop_against_the_cpu_loop(dm, oracle):
    """The CPU loop of oracle + route, spawn and traffic models (tests/test_episode_spawn.py) with the trace model beside it, against
    the device's rings: integer fields equal, doubles within 1e-6 (the project's bar for oracle against device)."""
    import test_episode_spawn as tes
    import test_traffic as tt
    import episode_model as epm
    import episode_spawn_model as esm
    import map_scenes as ms
    import route_model as rmod
    import traffic_model as tm
    L = _contact_loop(dm)
    r, model, n = L["scene"], L["model"], tt.F_N
    cfg, m, sc, adv, rm = r["cfg"], r["m"], r["sc"], dm.default_ego_model(), dm.default_route_model()
    dt, hw = float(adv["dt"][0]), 0.5 * float(cfg["Vehicle_Width"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(n, np.int32)
    tr = tm.Traffic(r["tracks"], r["pts"], r["act"], si["obs_off"])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    pin, pst = [si.copy()], [st.copy()]
    stats, sstats, scores = epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n), rsm.new_scores(dm.RolloutScore, n)
    rings, info = stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, 32)
    tick0 = int(L[False]["rings"][0]["tick"][0]) - int(L[False]["rings"][0]["k"][0])
    for t in range(60):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        stm.step(rings, info, model, scores, cfg, dt, tick0 + t, si, plan, st, obs, flags, stats)
        rsm.fold(scores, cfg, dt, si, plan, st, obs, flags)
        q, f, _ = rmod.advance(dm, cfg, adv, rm, r["legs"], r["rf"], m, si, plan, st, flags)
        si, st, flags, _, _ = esm.step(r["em"], r["sp"], stats, sstats, pin, pst, si, q, f, st, obs, hw, None, None, scores)
        obs, _ = tr.place(obs, None, dt)
    got = L[False]
    for f in dm.ScoreTraceInfo.names:
        assert np.array_equal(got["info"][f], info[f]), f
    worst = 0.0
    for s in range(n):
        a, b = got["rings"][s], stm.oldest_first(rings, info, s)
        for f in dm.ScoreTick.names:
            if a.dtype[f].kind == "f":
                d = float(np.max(np.where(a[f] == b[f], 0.0, np.abs(a[f] - b[f]))))
                worst = max(worst, d)
                assert d <= 1e-6, (s, f, d)
            else:
                assert np.array_equal(a[f], b[f]), (s, f, a[f].tolist(), b[f].tolist())
    print("largest difference of a double, device against the CPU loop:", worst)


@gpu
def test_flag_cause_on_the_ring_without_episodes(dm):
    """The flag cause on the device: the 8 one-leg ring egos of tests/test_episodes.py without episodes arrive (LANE_END | ROUTE_END = 20)
    and keep their sticky word; flag_mask 16, post 3: every ring freezes 3 ticks behind the first tick that carried the word."""
    import test_episodes as te
    cfg, m, sc, legs, rf = te._ring_scene(dm)
    pl = te._planner(dm, cfg, m, sc)
    pl.set_route(legs, rf)
    n, adv, model = te.RING_N, dm.default_ego_model(), _tm(dm, depth=8, post=3, trigger=FLAG | BRAKE, flag_mask=16, brake=1000.0)
    pl.score_begin(float(adv["dt"][0]))
    pl.set_score_trace(model)                                               # behind pp_score_begin
    scores, (rings, info) = rsm.new_scores(dm.RolloutScore, n), stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, 8)
    _follow(dm, pl, cfg, model, n, 70, rings, info, scores, adv, False, hold=set(range(0, 70, 9)) | {69})
    info, rings = stb.read_all(pl, n)
    pl.close()
    print("trigger_k", info["trigger_k"].tolist())
    assert (info["state"] == 2).all() and (info["trigger"] == FLAG).all() and (info["n_written"] == info["trigger_k"] + 4).all()
    for s in range(n):
        ring, k = rings[s], int(info["trigger_k"][s])
        assert ring["k"].tolist() == list(range(k - 4, k + 4)) and [int(f) & 16 for f in ring["flags"]] == [0] * 4 + [16] * 4 and _causes(ring) == [0] * 4 + [FLAG] * 4
        assert ring["tick"].tolist() == [j + 1 for j in range(k - 4, k + 4)]
        assert (ring["obs"] == -1).all() and (ring["clearance"] == INF).all() and not (ring["marks"] & stm.TICK_START).any()


@gpu
def test_life_cycle_across_set_calls(dm):
    """pp_set_fleet, pp_set_traffic, pp_set_episodes and pp_set_route do not touch the headers: a 20-tick run with one of them in the
    middle equals the model (which knows nothing of them).  pp_set_egos while scoring resets the headers."""
    import test_episode_spawn as tes
    import test_traffic as tt
    r, n, adv = tes._loop_scene(dm), tt.F_N, dm.default_ego_model()
    model = _tm(dm, depth=6, post=1, trigger=BRAKE, brake=0.05)

    def fleet(pl):
        fm = dm.default_fleet_model()
        fm["max_peers"] = 0
        pl.set_fleet([0, n // 2, n], fm)

    calls = dict(fleet=fleet, traffic=lambda pl: pl.set_traffic(r["tracks"], r["pts"], r["act"]), episodes=lambda pl: pl.set_episodes(r["em"]),
                 route=lambda pl: pl.set_route(r["legs"], r["rf"]))
    for name, call in calls.items():
        pl = tt._planner(dm, r["cfg"], r["m"], r["sc"], 1)
        pl.set_route(r["legs"], r["rf"])
        pl.set_traffic(r["tracks"], r["pts"], r["act"])
        pl.set_score_trace(model)
        pl.score_begin(float(adv["dt"][0]))
        scores, (rings, info) = rsm.new_scores(dm.RolloutScore, n), stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, 6)
        _follow(dm, pl, r["cfg"], model, n, 10, rings, info, scores, adv, False, hold={0, 9})
        # a set call follows a tick, not a staged advance: one more tick adopts the advance - it is scored, and the model steps over it
        sin, flags, dt = pl.get_scene_in(), pl.ego_flags(), float(adv["dt"][0])
        plan_p = dm.pinned_empty(n, dm.PlanOut)
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        plan, state, now = np.array(plan_p), pl.get_state(), pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, n)
        stm.step(rings, info, model, scores, r["cfg"], dt, pl.tick_id(), sin, plan, state, now, flags)
        rsm.fold(scores, r["cfg"], dt, sin, plan, state, now, flags)
        before = pl.score_trace_info()
        stb.same(before, info, f"{name}: in front of the call")
        call(pl)
        stb.same(pl.score_trace_info(), before, f"{name}: behind the call")
        _follow(dm, pl, r["cfg"], model, n, 10, rings, info, scores, adv, name == "episodes", hold={10, 19}, t0=10)
        assert int(info["n_written"].min()) >= 2, name
        if name == "route":                                                 # new egos while scoring: the totals restart, and the headers with them
            pl.tick()
            pl.set_egos(r["sc"], with_motion=False)
            assert all(_hd(pl.score_trace_info(), s) == (0, 0, -1, 0, 0, 0) for s in range(n))
            assert (pl.rollout_score()["n_ticks"] == 0).all()
        pl.close()
