"""Episodic rollouts (pp_set_episodes): ended egos restart on the device from start records.

CPU: the ABI mirrors, hand-derived known answers of the numpy model (tests/episode_model.py) with their arithmetic, and a closed
loop of oracle tick + route model + episode model on the ring of tests/route_scenes.py.
GPU: the known answers on k_respawn_egos alone and as distinct scenes of one launch (batches of 5 and 9), restore completeness on
byte patterns, the closed loop against the CPU loop, pp_rollout against its parts, episodes switched off, the error paths and
lifetime, and the scorecard and a fleet on restarting egos."""
import math

import numpy as np
import pytest

import episode_backends as eb
import episode_model as epm
import fleet_model as fl
import map_scenes as ms
import rollout_score_model as rsm
import route_model as rmod
import route_scenes as rs

gpu = pytest.mark.gpu


@pytest.fixture()
def cfg0(dm):
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    return cfg


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirrors_and_default_model(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(29) == dm.EpisodeModel.itemsize == 8
    assert lib.pp_sizeof(30) == dm.EpisodeStats.itemsize == 80
    assert [dm.EpisodeStats.fields[k][1] for k in ("n_episodes", "age", "n_end", "last_cause", "last_age", "min_age", "max_age", "ticks_total", "dist", "last_dist", "dist_total")] == \
        [0, 4, 8, 32, 36, 40, 44, 48, 56, 64, 72]
    em = dm.default_episode_model()
    assert (int(em["end_mask"][0]), int(em["max_ticks"][0])) == (31, 0)
    assert (dm.EGO_RESPAWNED, dm.EGO_TIMEOUT) == (epm.RESPAWNED, epm.TIMEOUT) == (32, 64)
    assert (epm.PATH_END, epm.BAD_PATH, epm.LANE_END, epm.OFF_GRID, epm.ROUTE_END) == \
        (dm.EGO_PATH_END, dm.EGO_BAD_PATH, dm.EGO_LANE_END, dm.EGO_OFF_GRID, dm.EGO_ROUTE_END)
    s = epm.new_stats(dm.EpisodeStats, 2)
    assert s["min_age"].tolist() == [-1, -1] and s["max_age"].tolist() == [-1, -1] and not s["n_episodes"].any() and not s["dist_total"].any()


# The map of tests/test_route.py, small enough to do by hand.  Road 1: two lanes of 100 points, x = 100 + 0.5 k (k = 0 .. 99, the last
# point at 149.5), lane 1 at y = 3.75, lane 2 at y = 0.  Road 2: one lane of 100 points, x = 155 + 0.5 k, y = 0.  One junction, from
# lane 2 of road 1 to lane 1 of road 2: 10 points, x = 150 + 0.5 k, y = 0.  Lane 1 of road 1 has no junction.
_WORLD = {}


def _world(dm):
    if not _WORLD:
        pts = np.zeros(300, dm.GlobalPoint3D)
        pts["x"][:100], pts["y"][:100] = 100.0 + 0.5 * np.arange(100), 3.75
        pts["x"][100:200], pts["y"][100:200] = 100.0 + 0.5 * np.arange(100), 0.0
        pts["x"][200:], pts["y"][200:] = 155.0 + 0.5 * np.arange(100), 0.0
        jp = np.zeros(10, dm.GlobalPoint2D)
        jp["x"] = 150.0 + 0.5 * np.arange(10)
        _WORLD["map"] = dict(road_first_lane=np.array([0, 2, 3], np.int32),
                             lanes=np.array([(0, 100, 2, 0), (100, 100, 2, 0), (200, 100, 1, 0)], dm.MapLane),
                             points=pts, lanechg_attribute=np.zeros(300, np.uint8), lane_width_cm=np.full(300, 375, np.uint16),
                             junctions=np.array([(1, 2, 2, 1, 0, 10)], dm.MapJunction), jpoints=jp)
    return _WORLD


def _legs(dm, n=2):
    legs = np.zeros(2, dm.RouteLeg)
    legs["road_num"] = [1, 2]
    legs["stub_attribute"] = [1, 2]
    legs["out_lane_no"][0, :1] = [2]
    legs["out_lane_no"][1, :1] = [1]
    return legs[:n]


def _ego(dm, x, y=0.0, pos=0, road=1, lane=2, ego_id=30, four=(0, 0, 0, 0), v=36.0):
    si = np.zeros(1, dm.SceneIn)
    loc = si["loc"]
    loc["pos"], loc["road_num"], loc["lane_num"], loc["velocity"] = pos, road, lane, v
    loc["last_roadnum"], loc["next_roadnum"], loc["last_lanenum"], loc["next_lanenum"] = four
    loc["id"][:] = ego_id
    loc["globalpoint"]["x"], loc["globalpoint"]["y"], loc["globalpoint"]["dir"] = x, y, 77.0
    si["stub_attribute"], si["out_lane_no"][0, 0] = 1, 2
    si["period_last"] = 100.0
    return ms.resolve(dm, _world(dm)["map"], si)


def _path(dm, x0, y=0.0, desspd=36.0):
    """A straight 200-point path along +x from x0 at 0.5 m spacing; at 36 km/h towards 36 km/h the ego goes s = 1 m, to x0 + 1."""
    po = np.zeros(1, dm.PlanOut)
    po["road_points"]["x"][0] = x0 + 0.5 * np.arange(200)
    po["road_points"]["y"][0] = y
    po["result"]["desspd"] = desspd
    return po


def _state0(dm):
    """The state an episode starts from: the constructor values, and two words no advance and no crafted state carries."""
    st = np.zeros(1, dm.SceneState)
    dm.load_library().pp_init_state(st.ctypes.data, 2)
    st["tick"], st["count"] = 7, 3
    return st


def _em(dm, end_mask=31, max_ticks=0):
    em = dm.default_episode_model()
    em["end_mask"], em["max_ticks"] = end_mask, max_ticks
    return em


class _Ep:
    """Advances of one scene on a backend of tests/episode_backends.py: the known answers below are written once against it."""
    def __init__(self, dm, runner):
        self.dm, self.run, self.name = dm, runner, runner.name

    def __call__(self, cfg, si, pos, em, legs=None, sts=None, score=False):
        dm = self.dm
        route = None if legs is None else (legs, np.array([0, len(legs)], np.int32), dm.default_route_model())
        sts = [np.zeros(1, dm.SceneState) for _ in pos] if sts is None else sts
        return self.run(cfg, dm.default_ego_model(), em, si, _state0(dm), list(zip(pos, sts)), _world(dm), route, score)


def _runner(name, log=None):
    return eb.Runner(eb.ModelBackend() if name == "model" else eb.DeviceBackend(), log)


def _stats(r):
    e = r.stats[0]
    return dict(n=int(e["n_episodes"]), age=int(e["age"]), n_end=e["n_end"].tolist(), cause=int(e["last_cause"]), last_age=int(e["last_age"]),
                ages=(int(e["min_age"]), int(e["max_age"])), ticks=int(e["ticks_total"]), dist=float(e["dist"]), last_dist=float(e["last_dist"]),
                total=float(e["dist_total"]))


NONE = dict(n=0, n_end=[0] * 6, cause=0, last_age=0, ages=(-1, -1), ticks=0, last_dist=0.0, total=0.0)


def _restarted(dm, r, si, trace_flags):
    """Step r put the scene back on its start records: every byte of SceneIn and SceneState, no flag, the trace of the start record."""
    assert r.out.tobytes() == si.tobytes() and r.state.tobytes() == _state0(dm).tobytes() and int(r.flags[0]) == 0
    t, loc = r.trace[0], si["loc"][0]
    assert t["pose"].tobytes() == loc["globalpoint"].tobytes() and float(t["velocity"]) == float(loc["velocity"])
    assert (int(t["id_cur"]), int(t["lane_num"]), int(t["flags"])) == (int(loc["id"][int(loc["lane_num"]) - 1]), int(loc["lane_num"]), trace_flags)


def _flag_cases(dm, cfg0):
    """(flag, configuration, ego, plan, state the advance reads, legs, metres the advance moves the ego): each of the five flags alone."""
    st198 = np.zeros(1, dm.SceneState)
    st198["path_near_id"] = 198
    bad = _path(dm, 110.0)
    bad["road_points"]["x"][0, 0] = np.nan
    grid = dm.default_config(128)
    off = _ego(dm, 120.0)
    off["grid_origin"]["x"], off["grid_origin"]["y"], off["goal"]["x"], off["goal"]["y"] = 100.0, 100.0, 116.0, 116.0
    inj = _ego(dm, 154.5, pos=2, road=2, lane=1, ego_id=0, four=(1, 2, 2, 1))
    inj["loc"]["id"][0, 1] = 6
    return [
        # the path is walked from point 198 (199.0): 0.5 m are left of the 1 m step -> PATH_END, the ego stops on point 199 (199.5)
        (epm.PATH_END, cfg0, _ego(dm, 199.0), _path(dm, 100.0), st198, None, 0.5),
        # point k0 = 0 of the path is NaN -> BAD_PATH, the record is carried over: the ego moves 0 m
        (epm.BAD_PATH, cfg0, _ego(dm, 110.0), bad, None, None, 0.0),
        # lane 1 of road 1 has no junction: the ego lands on 134.0 = point 68, 68 + 32 >= 100 -> LANE_END alone (it missed its exit lane)
        (epm.LANE_END, cfg0, _ego(dm, 133.0, y=3.75, lane=1, ego_id=60), _path(dm, 133.0, y=3.75), None, _legs(dm), 1.0),
        # grid stage on, a grid of 32 m at (100, 100): the ego on y = 0 lands on 121.0, outside it -> OFF_GRID
        (epm.OFF_GRID, grid, off, _path(dm, 120.0), None, None, 1.0),
        # inside the junction behind the LAST leg: the ego lands on 155.5, nearest polyline point 9 = the end -> ROUTE_END alone, everything held
        (epm.ROUTE_END, cfg0, inj, _path(dm, 154.5), None, _legs(dm, 1), 1.0),
    ]


def _kat_each_flag_in_the_mask_ends_the_episode(dm, cfg0, ep):
    for flag, cfg, si, po, st, legs, d in _flag_cases(dm, cfg0):
        (r,) = ep(cfg, si, [po], _em(dm), legs, None if st is None else [st])
        _restarted(dm, r, si, flag | 32)
        b = flag.bit_length() - 1
        assert _stats(r) == dict(n=1, age=0, n_end=[int(k == b) for k in range(6)], cause=flag, last_age=1, ages=(1, 1), ticks=1, dist=0.0, last_dist=d, total=d), flag


def _kat_a_flag_outside_the_mask_freezes_as_before(dm, cfg0, ep):
    for flag, cfg, si, po, st, legs, d in _flag_cases(dm, cfg0):
        st = np.zeros(1, dm.SceneState) if st is None else st
        (r,) = ep(cfg, si, [po], _em(dm, 31 & ~flag), legs, [st])
        assert int(r.flags[0]) == flag and int(r.trace["flags"][0]) == flag and r.state.tobytes() == st.tobytes()
        assert float(r.out["loc"]["globalpoint"]["x"][0]) == float(si["loc"]["globalpoint"]["x"][0]) + d
        assert (r.out.tobytes() == si.tobytes()) == (flag == epm.BAD_PATH)
        assert _stats(r) == dict(NONE, age=1, dist=d), flag


def _kat_a_scene_that_goes_on_is_only_counted(dm, cfg0, ep):
    # no flag, no timeout: the staged record is the advance's (111.0), the state the tick's; one advance, one metre - routed or not
    for legs in (None, _legs(dm)):
        si = _ego(dm, 110.0, ego_id=20)
        (r,) = ep(cfg0, si, [_path(dm, 110.0)], _em(dm), legs)
        assert (float(r.out["loc"]["globalpoint"]["x"][0]), int(r.out["loc"]["id"][0, 1]), int(r.flags[0]), int(r.trace["flags"][0])) == (111.0, 22, 0, 0)
        assert r.state.tobytes() == np.zeros(1, dm.SceneState).tobytes() and _stats(r) == dict(NONE, age=1, dist=1.0)


def _kat_two_flags_count_in_both(dm, cfg0, ep):
    # lane 2 of road 1 on a route of ONE leg: point 68 is the lane end of the last leg -> LANE_END | ROUTE_END = 4 | 16 = 20, the ego arrived
    si = _ego(dm, 133.0, ego_id=60)
    (r,) = ep(cfg0, si, [_path(dm, 133.0)], _em(dm), _legs(dm, 1))
    _restarted(dm, r, si, 20 | 32)
    assert _stats(r) == dict(n=1, age=0, n_end=[0, 0, 1, 0, 1, 0], cause=20, last_age=1, ages=(1, 1), ticks=1, dist=0.0, last_dist=1.0, total=1.0)
    # with only ROUTE_END in the mask the cause is 16 and only n_end[4] counts; the trace still carries both flags of the advance
    (r,) = ep(cfg0, si, [_path(dm, 133.0)], _em(dm, 16), _legs(dm, 1))
    _restarted(dm, r, si, 20 | 32)
    assert _stats(r)["n_end"] == [0, 0, 0, 0, 1, 0] and _stats(r)["cause"] == 16


def _kat_timeout_at_max_ticks(dm, cfg0, ep):
    # max_ticks = 3: 110 -> 111 -> 112 (ages 1, 2 = max_ticks - 1: nothing), the third advance reaches age 3 = max_ticks: TIMEOUT alone,
    # 3 m driven; the record it staged (113.0) is replaced by the start record, the trace says 0 | RESPAWNED | TIMEOUT = 96
    si = _ego(dm, 110.0, ego_id=20)
    r = ep(cfg0, si, [_path(dm, 110.0), _path(dm, 111.0), _path(dm, 112.0)], _em(dm, 31, 3))
    assert [float(q.out["loc"]["globalpoint"]["x"][0]) for q in r] == [111.0, 112.0, 110.0]
    assert _stats(r[0]) == dict(NONE, age=1, dist=1.0) and _stats(r[1]) == dict(NONE, age=2, dist=2.0)
    assert [int(q.flags[0]) for q in r] == [0, 0, 0] and [int(q.trace["flags"][0]) for q in r] == [0, 0, 96]
    _restarted(dm, r[2], si, 96)
    assert _stats(r[2]) == dict(n=1, age=0, n_end=[0, 0, 0, 0, 0, 1], cause=64, last_age=3, ages=(3, 3), ticks=3, dist=0.0, last_dist=3.0, total=3.0)


def _kat_flag_and_timeout_on_one_advance(dm, cfg0, ep):
    # max_ticks = 1 and the LANE_END advance: cause 4 | 64 = 68, ONE episode, counted under LANE_END and under TIMEOUT; trace 4 | 32 | 64 = 100
    si = _ego(dm, 133.0, y=3.75, lane=1, ego_id=60)
    (r,) = ep(cfg0, si, [_path(dm, 133.0, y=3.75)], _em(dm, 31, 1), _legs(dm))
    _restarted(dm, r, si, 100)
    assert _stats(r) == dict(n=1, age=0, n_end=[0, 0, 1, 0, 0, 1], cause=68, last_age=1, ages=(1, 1), ticks=1, dist=0.0, last_dist=1.0, total=1.0)


def _kat_a_timeout_rescues_a_scene_frozen_by_an_unmasked_flag(dm, cfg0, ep):
    # LANE_END is not in the mask (27): the first advance freezes the ego on 134.0, the second carries the record over (+0 m, age 2), the
    # third reaches max_ticks = 3: cause = (4 & 27) | 64 = 64 - TIMEOUT alone - while the trace keeps the flag: 4 | 32 | 64 = 100
    si = _ego(dm, 133.0, y=3.75, lane=1, ego_id=60)
    po = _path(dm, 133.0, y=3.75)
    r = ep(cfg0, si, [po, po, po], _em(dm, 27, 3), _legs(dm))
    assert [int(q.flags[0]) for q in r] == [4, 4, 0] and [int(q.trace["flags"][0]) for q in r] == [4, 4, 100]
    assert r[1].out.tobytes() == r[0].out.tobytes() != si.tobytes() and float(r[0].out["loc"]["globalpoint"]["x"][0]) == 134.0
    assert _stats(r[0]) == dict(NONE, age=1, dist=1.0) and _stats(r[1]) == dict(NONE, age=2, dist=1.0)
    _restarted(dm, r[2], si, 100)
    assert _stats(r[2]) == dict(n=1, age=0, n_end=[0, 0, 0, 0, 0, 1], cause=64, last_age=3, ages=(3, 3), ticks=3, dist=0.0, last_dist=1.0, total=1.0)


def _kat_two_episodes_in_a_row(dm, cfg0, ep):
    # episode 1: 132 -> 133.0 (point 66: 66 + 32 < 100) -> 134.0 (point 68: LANE_END), age 2, 2 m.  Episode 2 starts on 132 again; the plan
    # it is given leads from 133.5 to 134.5 (point 69: LANE_END), age 1, and the ego jumped 134.5 - 132 = 2.5 m.
    si = _ego(dm, 132.0, y=3.75, lane=1, ego_id=60)
    r = ep(cfg0, si, [_path(dm, 132.0, y=3.75), _path(dm, 133.0, y=3.75), _path(dm, 133.5, y=3.75)], _em(dm), _legs(dm))
    assert (int(r[0].flags[0]), int(r[0].out["loc"]["id"][0, 0]), _stats(r[0])) == (0, 66, dict(NONE, age=1, dist=1.0))
    _restarted(dm, r[1], si, 36)
    assert _stats(r[1]) == dict(n=1, age=0, n_end=[0, 0, 1, 0, 0, 0], cause=4, last_age=2, ages=(2, 2), ticks=2, dist=0.0, last_dist=2.0, total=2.0)
    _restarted(dm, r[2], si, 36)
    assert _stats(r[2]) == dict(n=2, age=0, n_end=[0, 0, 2, 0, 0, 0], cause=4, last_age=1, ages=(1, 2), ticks=3, dist=0.0, last_dist=2.5, total=4.5)


def _kat_a_start_record_that_ends_at_once(dm, cfg0, ep):
    # the start record sits one step in front of its lane end: every advance ends an episode - one per advance, never two
    si = _ego(dm, 133.0, y=3.75, lane=1, ego_id=60)
    po = _path(dm, 133.0, y=3.75)
    r = ep(cfg0, si, [po, po, po], _em(dm), _legs(dm))
    for k, q in enumerate(r):
        _restarted(dm, q, si, 36)
        assert _stats(q) == dict(n=k + 1, age=0, n_end=[0, 0, k + 1, 0, 0, 0], cause=4, last_age=1, ages=(1, 1), ticks=k + 1, dist=0.0, last_dist=1.0, total=float(k + 1))


def _kat_a_nan_position(dm, cfg0, ep):
    # the start record's x is NaN: ex = 134.0 - NaN -> the episode's distance is NaN, and so is every total it enters; the integers count
    # on, the running distance starts again from 0 and the restored record carries the NaN, bit for bit
    si = _ego(dm, np.nan, y=3.75, lane=1, ego_id=60)
    po = _path(dm, 133.0, y=3.75)
    r = ep(cfg0, si, [po, po], _em(dm), _legs(dm))
    for k, q in enumerate(r):
        _restarted(dm, q, si, 36)
        s = _stats(q)
        assert math.isnan(s.pop("last_dist")) and math.isnan(s.pop("total"))
        assert s == dict(n=k + 1, age=0, n_end=[0, 0, k + 1, 0, 0, 0], cause=4, last_age=1, ages=(1, 1), ticks=k + 1, dist=0.0)


def _kat_the_scorecard_does_not_see_the_jump(dm, cfg0, ep):
    # desspd 30 < 36: v1 = 36 - 4 * 0.1 * 3.6 = 34.56 km/h, s = 0.5 (36 + v1) / 3.6 * 0.1 = 0.98 m: past point 1 (110.5), on to
    # x1 = 110.5 + (s - 0.5) / 0.5 * 0.5.  max_ticks = 2: the second advance ends the episode.  Scored ticks: the start (110, 36), then
    # (x1, v1): dist = x1 - 110, max_dec = (36 - v1) / 3.6 / 0.1 = 4; the restart moves last_pos / last_speed to (110, 36), so the third scored
    # tick - on the start record - adds +0 m and no acceleration: without the patch it would add x1 - 110 again and max_acc = 4
    v1 = 36.0 - 4.0 * 0.1 * 3.6
    s = 0.5 * (36.0 + v1) / 3.6 * 0.1
    x1 = 110.5 + (s - 0.5) / 0.5 * (111.0 - 110.5)
    si = _ego(dm, 110.0, ego_id=20)
    r = ep(cfg0, si, [_path(dm, 110.0, desspd=30.0), _path(dm, 111.0, desspd=30.0)], _em(dm, 31, 2), score=True)
    assert (float(r[0].out["loc"]["globalpoint"]["x"][0]), float(r[0].out["loc"]["velocity"][0])) == (x1, v1)
    _restarted(dm, r[1], si, 96)
    before, patched, after = r[0].score[0], r[1].score[0], r[1].final_score[0]
    assert (int(before["n_ticks"]), float(before["dist"]), float(before["last_pos"]["x"]), float(before["last_speed"])) == (1, 0.0, 110.0, 36.0)
    dec = -((v1 - 36.0) / 3.6 / 0.1)
    assert (int(patched["n_ticks"]), float(patched["dist"]), float(patched["max_acc"]), float(patched["max_dec"])) == (2, x1 - 110.0, 0.0, dec)
    assert (float(patched["last_pos"]["x"]), float(patched["last_pos"]["y"]), float(patched["last_speed"])) == (110.0, 0.0, 36.0)
    assert (int(after["n_ticks"]), float(after["dist"]), float(after["max_acc"]), float(after["max_dec"]), float(after["max_speed"])) == (3, x1 - 110.0, 0.0, dec, 36.0)
    assert abs(dec - 4.0) < 1e-12 and abs(x1 - 110.98) < 1e-12


KATS = [_kat_a_scene_that_goes_on_is_only_counted, _kat_each_flag_in_the_mask_ends_the_episode, _kat_a_flag_outside_the_mask_freezes_as_before, _kat_two_flags_count_in_both, _kat_timeout_at_max_ticks,
        _kat_flag_and_timeout_on_one_advance, _kat_a_timeout_rescues_a_scene_frozen_by_an_unmasked_flag, _kat_two_episodes_in_a_row,
        _kat_a_start_record_that_ends_at_once, _kat_a_nan_position]


@pytest.mark.parametrize("kat", KATS + [_kat_the_scorecard_does_not_see_the_jump], ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, cfg0, kat):
    kat(dm, cfg0, _Ep(dm, _runner("model")))


# ---- the ring ------------------------------------------------------------------------------------------------
RING_N, RING_TICKS = 8, 160
_CPU = {}


def _ring_scene(dm, n_obs=0):
    """8 obstacle-free egos on lanes 1 / 2 of the ring, 190 .. 215 points into a road of 260, each with a route of ONE leg: an ego
    arrives (LANE_END | ROUTE_END) after a few dozen advances."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, RING_N, seed=3, lanes=(1, 2), ids=(190, 215), legs=(1, 1), n_obs=n_obs)
    return cfg, m, sc, legs, rf


def _cpu_loop(dm, oracle, max_ticks=0):
    """Oracle tick + route model + episode model, 160 advances.  sins[t]: the records tick t reads (sins[0] the start records)."""
    if max_ticks in _CPU:
        return _CPU[max_ticks]
    cfg, m, sc, legs, rf = _ring_scene(dm)
    model, rm, em = dm.default_ego_model(), dm.default_route_model(), _em(dm, 31, max_ticks)
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(RING_N, np.int32)
    start_in, start_state, stats = si.copy(), st.copy(), epm.new_stats(dm.EpisodeStats, RING_N)
    sins, fl_, causes = [si], [flags], []
    for t in range(RING_TICKS):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, mot_pool=None), st, n_threads=8, want_grid=False)
        q, f, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
        si, st, flags, _, c = epm.step(em, stats, start_in, start_state, si, q, f, st)
        sins.append(si), fl_.append(flags), causes.append(c)
    _CPU[max_ticks] = dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, em=em, sins=sins, flags=fl_, causes=np.array(causes), stats=stats, state=st)
    return _CPU[max_ticks]


def test_ring_episodes_on_the_cpu(dm, oracle):
    """Every ego arrives at least three times, every episode of an ego has the same age, ends with LANE_END | ROUTE_END and stages the
    records of the ego's first episode byte for byte: SceneIn + SceneState are the whole per-scene memory of the engine."""
    r = _cpu_loop(dm, oracle)
    s, causes = r["stats"], r["causes"]
    print("episodes", s["n_episodes"].tolist(), "ages", s["min_age"].tolist(), "causes", sorted(set(causes[causes != 0].tolist())))
    assert (s["n_episodes"] >= 3).all() and (s["min_age"] == s["max_age"]).all()
    assert (s["n_end"][:, 4] == s["n_episodes"]).all() and (s["n_end"][:, 2] == s["n_episodes"]).all() and not s["n_end"][:, [0, 1, 3, 5]].any()
    assert set(causes[causes != 0].tolist()) == {20} and (s["ticks_total"] == s["n_episodes"] * s["min_age"]).all()
    for k in range(RING_N):
        ends = np.flatnonzero(causes[:, k])                    # advance t ended an episode: sins[t + 1][k] is the start record again
        first = [r["sins"][t + 1][k].tobytes() for t in range(0, ends[0] + 1)]
        for a, b in zip(ends[:-1], ends[1:]):
            assert [r["sins"][t + 1][k].tobytes() for t in range(a + 1, b + 1)] == first, f"ego {k}: the episode ending with advance {b} is not its first one"
        assert first[-1] == r["sins"][0][k].tobytes()


def test_ring_episodes_with_a_timeout_on_the_cpu(dm, oracle):
    """max_ticks = 25 on the same scene: the egos whose route ends sooner still arrive, the others end with TIMEOUT alone at age 25."""
    free, r = _cpu_loop(dm, oracle)["stats"], _cpu_loop(dm, oracle, 25)
    s = r["stats"]
    print("free ages", free["min_age"].tolist(), "with the timeout: episodes", s["n_episodes"].tolist(), "ages", s["min_age"].tolist(), "causes", s["last_cause"].tolist())
    soon = free["min_age"] < 25
    assert soon.sum() == 2 and (free["min_age"] != 25).all()
    assert (s["last_cause"][soon] == 20).all() and np.array_equal(s["min_age"][soon], free["min_age"][soon]) and not s["n_end"][soon, 5].any()
    assert (s["last_cause"][~soon] == 64).all() and (s["min_age"][~soon] == 25).all() and (s["n_end"][~soon, 5] == s["n_episodes"][~soon]).all()
    assert not s["n_end"][~soon, :5].any() and (s["min_age"] == s["max_age"]).all() and (s["n_episodes"] == RING_TICKS // s["min_age"]).all()


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("kat", KATS + [_kat_the_scorecard_does_not_see_the_jump], ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg0, kat):
    """The known answers above on k_respawn_egos behind k_advance_egos / k_advance_route (injected PlanOut / SceneState), each step also
    held against the model on the device's own records: SceneIn, flags, trace, SceneState, EpisodeStats (episode_backends.compare)."""
    kat(dm, cfg0, _Ep(dm, _runner("device")))


@gpu
def test_kat_batches_equal_each_case_alone(dm, cfg0):
    """Every known answer once more on the device, logged, then as distinct scenes of one launch in batches of 5 and of 9 scenes - more
    than one block of four waves, never a multiple of four - with ending scenes first, last and on either side of the block edge
    4 | 5: every scene gives the bytes it gave alone (SceneIn, flags, trace, SceneState, EpisodeStats)."""
    log = []
    ep = _Ep(dm, _runner("device", log))
    for kat in KATS:
        kat(dm, cfg0, ep)
    ran = eb.batched(eb.DeviceBackend(), log)
    print(f"{len(log)} calls; batches (size, ending scenes): {ran}")
    assert {n for n, _ in ran} == {5, 9}
    assert any({0, 3, 4, n - 1} <= set(e) and len(e) < n for n, e in ran if n == 5) and any({0, 3, 4, n - 1} <= set(e) and len(e) < n for n, e in ran if n == 9)


def _pattern(dtype, n, seed):
    """n records of distinct, never-zero bytes."""
    raw = (np.arange(n * dtype.itemsize, dtype=np.int64) * 37 + seed) % 251 + 1
    return np.frombuffer(raw.astype(np.uint8).tobytes(), dtype).copy()


@gpu
def test_restore_brings_every_byte_back(dm, cfg0):
    """9 scenes; the start records are captured from byte patterns: SceneState is a pattern from its first byte to its last, SceneIn
    a pattern in every byte an advance carries over and pp_set_egos does not derive (dec, stub_attribute, _pad, out_lane_no,
    period_last, grid_origin, goal - the last 8 bytes of the record -, the unused ids and junction indices).  The records the step
    runs on arrive later and differ in every one of those bytes.  Scenes 0, 3, 4 and 8 end (first, last, either side of the block
    edge; odd and even indices: SceneIn is 248 B, so every second record starts 8 bytes off a 16-byte boundary): they get every
    byte of their start records back.  The others keep every byte the advance wrote."""
    n, m = 9, _world(dm)["map"]
    ending = [0, 3, 4, 8]
    si = np.concatenate([_ego(dm, 133.0, y=3.75, lane=1, ego_id=60) if k in ending else _ego(dm, 110.0 + k, ego_id=20) for k in range(n)])
    po = np.concatenate([_path(dm, 133.0, y=3.75) if k in ending else _path(dm, 110.0 + k) for k in range(n)])
    cap = _pattern(dm.SceneIn, n, 5)
    for name in ("pos", "road_num", "lane_num", "path_num", "last_roadnum", "next_roadnum", "last_lanenum", "next_lanenum"):
        cap["loc"][name] = si["loc"][name]
    cap["loc"]["id"][:, :2] = si["loc"]["id"][:, :2]
    cap["obs_off"], cap["obs_n"] = 0, 0
    cap_st, st = _pattern(dm.SceneState, n, 11), np.zeros(n, dm.SceneState)
    legs = np.concatenate([_legs(dm)] * n)
    route = (legs, np.arange(0, 2 * n + 1, 2, dtype=np.int32), dm.default_route_model())
    state0 = np.concatenate([_state0(dm)] * n)
    (r,) = _runner("device")(cfg0, dm.default_ego_model(), _em(dm), si, state0, [(po, st)], _world(dm), route, False, (cap, cap_st))
    start = ms.resolve(dm, m, cap)
    assert np.flatnonzero(r.stats["n_episodes"]).tolist() == ending and r.flags.tolist() == [0] * n
    for k in range(n):
        if k in ending:
            assert r.out[k].tobytes() == start[k].tobytes() and r.state[k].tobytes() == cap_st[k].tobytes(), k
        else:
            assert r.state[k].tobytes() == st[k].tobytes() and float(r.out["loc"]["globalpoint"]["x"][k]) == 111.0 + k, k
            diff = np.frombuffer(r.out[k].tobytes(), np.uint8) != np.frombuffer(start[k].tobytes(), np.uint8)
            assert diff[-16:].all() and diff.sum() > 100, k         # (nothing of the start record leaked into it)
    assert 0 not in np.frombuffer(cap_st.tobytes(), np.uint8)


def _planner(dm, cfg, m, sc, n_obs=0, slack=0):
    pl = dm.Planner(cfg, device=0, **rs.caps(m, len(sc["scene_in"]), n_obs, slack))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    return pl


def _assert_records(got, want, what):
    """tests/test_route.py::_assert_records: every byte of the records but the heading (GetRoadAngle of §4c 3., an `atan`), which is
    held to 1e-6 degrees."""
    g, w = got.copy(), want.copy()
    g["loc"]["globalpoint"]["dir"], w["loc"]["globalpoint"]["dir"] = 0.0, 0.0
    assert g.tobytes() == w.tobytes(), what + ": SceneIn bytes, fields " + ", ".join(f for f in g.dtype.names if g[f].tobytes() != w[f].tobytes())
    dd = np.abs(got["loc"]["globalpoint"]["dir"] - want["loc"]["globalpoint"]["dir"])
    assert np.minimum(dd, 360.0 - dd).max() <= 1e-6, what + ": dir"


_RUNS = {}
_INT_FIELDS = ("n_episodes", "age", "n_end", "last_cause", "last_age", "min_age", "max_age", "ticks_total")


def _device_loop(dm, oracle):
    """The ring loop on the device, advance by advance with read-backs in between."""
    if "loop" in _RUNS:
        return _RUNS["loop"]
    r = _cpu_loop(dm, oracle)
    pl = _planner(dm, r["cfg"], r["m"], r["sc"])
    pl.set_route(r["legs"], r["rf"])
    pl.set_episodes(r["em"])
    model, trace = dm.default_ego_model(), dm.pinned_empty(RING_N, dm.EgoTrace)
    run = dict(sins=[pl.get_scene_in()], flags=[np.zeros(RING_N, np.int32)], trace=[])
    for t in range(RING_TICKS):
        pl.tick()
        pl.advance_async(model, trace)
        run["sins"].append(pl.get_scene_in()), run["flags"].append(pl.ego_flags())
        pl.sync()
        run["trace"].append(np.array(trace))
    pl.tick()
    pl.sync()
    run["last"] = (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), pl.episode_stats())
    pl.close()
    _RUNS["loop"] = run
    return run


@gpu
def test_ring_episodes_agree_with_the_cpu_loop(dm, oracle):
    """160 advances of the ring on the device: every staged record and flag word against the CPU loop - every byte but the heading -
    and the stats equal in every integer field."""
    r, d = _cpu_loop(dm, oracle), _device_loop(dm, oracle)
    for t in range(RING_TICKS + 1):
        assert np.array_equal(d["flags"][t], r["flags"][t]), f"set {t}: flags"
        _assert_records(d["sins"][t], r["sins"][t], f"set {t}")
    got, want = d["last"][4], r["stats"]
    print("episodes", got["n_episodes"].tolist(), "ages", got["min_age"].tolist(), "dist_total", got["dist_total"].tolist(), "cpu", want["dist_total"].tolist())
    for name in _INT_FIELDS:
        assert np.array_equal(got[name], want[name]), name
    assert (got["n_episodes"] >= 3).all()


@gpu
def test_rollout_with_episodes_equals_its_parts(dm, oracle):
    """pp_rollout(160) with episodes on = 160 x (advance, tick) with read-backs in between, bit for bit; the trace rows are those of the parts."""
    r, d = _cpu_loop(dm, oracle), _device_loop(dm, oracle)
    pl = _planner(dm, r["cfg"], r["m"], r["sc"])
    pl.set_route(r["legs"], r["rf"])
    pl.set_episodes(r["em"])
    last, trace = pl.rollout(RING_TICKS, trace=True)
    pl.sync()
    got = (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), pl.episode_stats())
    pl.close()
    assert last == RING_TICKS + 1
    for a, b, name in zip(got, d["last"], ("PlanOut", "SceneState", "flags", "SceneIn", "EpisodeStats")):
        assert a.tobytes() == b.tobytes(), name
    trace = np.array(trace)
    for t in range(RING_TICKS):
        assert trace[t].tobytes() == d["trace"][t].tobytes(), f"trace row {t}"
    assert ((trace["flags"] & epm.RESPAWNED) != 0).sum() == int(got[4]["n_episodes"].sum())


@gpu
def test_episodes_off_is_the_engine_without_them(dm, oracle):
    """A handle that sets and unsets episodes gives the bytes of one that never did: flagged egos freeze again."""
    r = _cpu_loop(dm, oracle)
    K, outs = 60, []
    for had in (True, False):
        pl = _planner(dm, r["cfg"], r["m"], r["sc"])
        pl.set_route(r["legs"], r["rf"])
        if had:
            pl.set_episodes(r["em"])
            pl.set_episodes(off=True)
        _, trace = pl.rollout(K, trace=True)
        pl.sync()
        outs.append((pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), np.array(trace)))
        if had:
            s = pl.episode_stats()                                  # the stats stay readable - and untouched
            assert s.tobytes() == epm.new_stats(dm.EpisodeStats, RING_N).tobytes()
        pl.close()
    for a, b, name in zip(outs[0], outs[1], ("PlanOut", "SceneState", "flags", "SceneIn", "trace")):
        assert a.tobytes() == b.tobytes(), name
    first = r["stats"]["min_age"]
    assert np.array_equal(outs[0][2] != 0, first <= K) and (outs[0][2][first <= K] == 20).all() and (first <= K).any()


@gpu
def test_errors_and_lifetime(dm, oracle):
    r = _cpu_loop(dm, oracle, 25)
    cfg, m, sc = r["cfg"], r["m"], r["sc"]
    pl = dm.Planner(cfg, device=0, **rs.caps(m, RING_N))
    with pytest.raises(dm.PlannerError, match="error -4:"):                   # PP_ERR_STATE: no resident scenes
        pl.set_episodes()
    with pytest.raises(dm.PlannerError, match="error -4:"):                   # ... and the stats of a handle that never set episodes
        pl.n = RING_N
        pl.episode_stats()
    pl.close()

    def fresh():
        p = _planner(dm, cfg, m, sc)
        p.set_route(r["legs"], r["rf"])
        p.set_episodes(r["em"])
        p.rollout(30)                                                         # (max_ticks = 25: every ego has restarted once)
        return p
    pl, ref = fresh(), fresh()
    for mask, ticks in ((32, 0), (63, 0), (-1, 0), (31, -1), (0, 0)):         # PP_ERR_ARG
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_episodes(_em(dm, mask, ticks))
    pl.advance_async()
    ref.advance_async()
    for kw in (dict(), dict(off=True)):                                       # PP_ERR_STATE: an update is staged
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.set_episodes(**kw)
    # none of it changed the model, the start records or the stats: the run goes on like the reference run
    for p in (pl, ref):
        p.tick()
        p.rollout(40)
        p.sync()
    for name in ("get_plan", "get_state", "ego_flags", "get_scene_in", "episode_stats"):
        assert getattr(pl, name)().tobytes() == getattr(ref, name)().tobytes(), name
    stats = pl.episode_stats()
    assert (stats["n_episodes"] >= 2).all() and (stats["max_age"] <= 25).all()
    ref.close()
    # a second pp_set_episodes captures again and restarts the stats; pp_get_state behind a staged advance is the restored state
    pl.set_episodes(_em(dm, 31, 1))
    assert pl.episode_stats().tobytes() == epm.new_stats(dm.EpisodeStats, RING_N).tobytes()
    start_in, start_state = pl.get_scene_in(), pl.get_state()
    pl.tick()
    pl.advance_async()
    assert pl.get_state().tobytes() == start_state.tobytes() and pl.get_scene_in().tobytes() == start_in.tobytes()
    assert pl.episode_stats()["n_episodes"].tolist() == [1] * RING_N and ((pl.episode_stats()["last_cause"] & 64) == 64).all()
    # pp_set_egos switches episodes off: flagged egos freeze, the stats stay as they were
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_route(r["legs"], r["rf"])
    before = pl.episode_stats()
    pl.rollout(60)
    pl.sync()
    free = _cpu_loop(dm, oracle)["stats"]["min_age"]
    assert np.array_equal(pl.ego_flags() != 0, free <= 60) and pl.episode_stats().tobytes() == before.tobytes()
    pl.close()


@gpu
def test_scorecard_and_fleet_on_restarting_egos(dm):
    """A fleet, routes, the scorecard and - last - episodes with max_ticks = 22 on the ring, 46 advances: the staged records and
    slices are fleet_model on the episode model's output, so a restarted ego sits in its peers' slots at its START pose in the same
    set; SceneState is the restored one; RolloutScore equals rollout_score_model + the patch of §4k 6., byte for byte."""
    K, ticks, worlds = 3, 46, [0, 3, RING_N]
    cfg, m, sc, legs, rf = _ring_scene(dm, n_obs=K)
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"] = 1000.0, K
    em, model, rm = _em(dm, 31, 22), dm.default_ego_model(), dm.default_route_model()
    dt = float(model["dt"][0])
    pl = _planner(dm, cfg, m, sc, n_obs=K)
    pl.set_fleet(worlds, fm)
    pl.set_route(legs, rf)
    pl.score_begin(dt)
    pl.set_episodes(em)
    off, own = sc["scene_in"]["obs_off"].copy(), sc["scene_in"]["obs_n"].copy()
    sin, pool, _ = fl.couple(fm, worlds, off, own, ms.resolve(dm, m, sc["scene_in"]), sc["obs_pool"].copy())
    assert pl.get_scene_in().tobytes() == sin.tobytes()
    start_in, start_state = sin.copy(), sc["state"].copy()
    stats, want, flags = epm.new_stats(dm.EpisodeStats, RING_N), rsm.new_scores(dm.RolloutScore, RING_N), np.zeros(RING_N, np.int32)
    plan_p, seen = dm.pinned_empty(RING_N, dm.PlanOut), 0
    for t in range(ticks):
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        plan, state = np.array(plan_p), pl.get_state()
        rsm.fold(want, cfg, dt, sin, plan, state, pool, flags)
        pl.advance_async(model)
        got, gflags = pl.get_scene_in(), pl.ego_flags()
        routed, f, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, sin, plan, state, flags)
        out, wstate, wflags, _, causes = epm.step(em, stats, start_in, start_state, sin, routed, f, state, None, want)
        wsin, wpool, _ = fl.couple(fm, worlds, off, own, out, pool)
        assert np.array_equal(gflags, wflags), f"advance {t}: flags"
        _assert_records(got, wsin, f"advance {t}")
        assert pl.get_state().tobytes() == wstate.tobytes(), f"advance {t}: SceneState"
        assert pl.episode_stats().tobytes() == stats.tobytes(), f"advance {t}: EpisodeStats"
        for s in range(RING_N):
            a, c = int(wsin["obs_off"][s]), int(wsin["obs_n"][s])
            sl = pl.get_obstacles(s)
            assert sl.tobytes() == wpool[a:a + c].tobytes(), f"advance {t}, scene {s}: slice"
            for e in np.flatnonzero(causes):                                  # ego e restarted: its peers see it on its start pose
                w = 0 if e < worlds[1] else 1
                if s != e and worlds[w] <= s < worlds[w + 1]:
                    slot = sl[sl["type"] == (fl.OB_PEER | int(e))]                # (a world of 3 has room for both peers; in the world of 5 the nearest 3)
                    assert len(slot) == (1 if w == 0 else len(slot)) <= 1
                    if len(slot):
                        assert (float(slot["x"][0]), float(slot["y"][0])) == (float(start_in["loc"]["globalpoint"]["x"][e]), float(start_in["loc"]["globalpoint"]["y"][e]))
                        seen += 1
        sin, flags, pool = got, gflags, wpool
    pl.tick()
    assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
    rsm.fold(want, cfg, dt, sin, np.array(plan_p), pl.get_state(), pool, flags)
    score = pl.rollout_score()
    pl.close()
    print("episodes", stats["n_episodes"].tolist(), "causes", stats["last_cause"].tolist(), "peer slots that showed a restarted ego:", seen)
    assert score.tobytes() == want.tobytes(), ", ".join(f for f in score.dtype.names if score[f].tobytes() != want[f].tobytes())
    assert (stats["n_episodes"] >= 2).all() and seen > 0
