"""Closed-loop rollout (pp_advance_async / pp_rollout / pp_get_ego_flags).

CPU: the ABI mirrors, and hand-derived known answers of the numpy ego model (tests/ego_model.py) with their arithmetic.
GPU: the device against that model step by step on its own inputs, the closed loop against the open loop and the oracle,
pp_rollout against its parts, a closed-form speed ramp, a lane change on the map store, frozen scenes and state errors."""
import math

import numpy as np
import pytest

import advance_backends as ab
import ego_model as em
import map_scenes as ms
from parity_util import compare

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirrors_and_default_model(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(19) == dm.EgoModel.itemsize == 32
    assert lib.pp_sizeof(20) == dm.EgoTrace.itemsize == 48
    m = dm.default_ego_model()
    for f in ("dt", "max_acc", "max_dec", "window"):
        assert np.isfinite(m[f][0]) and m[f][0] > 0
    assert (em.PATH_END, em.BAD_PATH, em.LANE_END, em.OFF_GRID) == (dm.EGO_PATH_END, dm.EGO_BAD_PATH, dm.EGO_LANE_END, dm.EGO_OFF_GRID)


def _straight(dm, x0=100.0, step=0.5, y=0.0):
    """PlanOut with a straight 200-point path along +x (0.5 m spacing: every arc length is an exact binary fraction)."""
    po = np.zeros(1, dm.PlanOut)
    po["road_points"]["x"][0] = x0 + step * np.arange(200)
    po["road_points"]["y"][0] = y
    return po


def _scene(dm, cfg, lane_num=2, lane_sum=3, n_pts=320, ego_id=50, v=36.0, lane_w=3.75):
    """One SceneIn on three straight lanes (x = 100 + 0.5 k; lane 1 leftmost at y = +lane_w, lane 2 at 0, lane 3 at -lane_w;
    pool: current, left, right view one after the other) and its lane pool."""
    si = np.zeros(1, dm.SceneIn)
    pool = np.zeros(3 * n_pts, dm.GlobalPoint3D)
    for slot, dy in enumerate((0.0, lane_w, -lane_w)):
        pool["x"][slot * n_pts:(slot + 1) * n_pts] = 100.0 + 0.5 * np.arange(n_pts)
        pool["y"][slot * n_pts:(slot + 1) * n_pts] = dy
    lv = si["lanes"]
    lv["cur_off"], lv["cur_n"], lv["left_off"], lv["left_n"], lv["right_off"], lv["right_n"] = 0, n_pts, n_pts, n_pts, 2 * n_pts, n_pts
    lv["lane_sum"], lv["lane_width"] = lane_sum, lane_w
    si["loc"]["lane_num"], si["loc"]["velocity"] = lane_num, v
    si["loc"]["id"][:] = ego_id
    si["loc"]["globalpoint"]["dir"] = 77.0
    return si, pool


def _map3(dm, n_pts=320, lane_w=3.75):
    """The three lanes of _scene as a map store: one road, lane 1 leftmost (y = +lane_w), lane 2 at 0, lane 3 at -lane_w."""
    pts = np.zeros(3 * n_pts, dm.GlobalPoint3D)
    for k, dy in enumerate((lane_w, 0.0, -lane_w)):
        pts["x"][k * n_pts:(k + 1) * n_pts] = 100.0 + 0.5 * np.arange(n_pts)
        pts["y"][k * n_pts:(k + 1) * n_pts] = dy
    return dict(road_first_lane=np.array([0, 3], np.int32), lanes=np.array([(k * n_pts, n_pts, 3, 0) for k in range(3)], dm.MapLane), points=pts,
                lanechg_attribute=np.zeros(3 * n_pts, np.uint8), lane_width_cm=np.full(3 * n_pts, int(round(lane_w * 100)), np.uint16),
                junctions=np.zeros(0, dm.MapJunction), jpoints=np.zeros(1, dm.GlobalPoint2D))


def _state(dm, near_id=10, afresh=0):
    st = np.zeros(1, dm.SceneState)
    st["path_near_id"], st["afresh_planning"] = near_id, afresh
    return st


class _Adv:
    """One advance of one scene on a backend of tests/advance_backends.py: the known answers below are written once against it."""
    def __init__(self, dm, runner):
        self.dm, self.run, self.name = dm, runner, runner.name

    def steps(self, cfg, si, steps, pool, model=None, map_mode=False):
        """steps: (PlanOut, near_id, afresh) one after the other on one handle.  map_mode: `pool` is a map, the views are its."""
        dm = self.dm
        if map_mode:
            si = si.copy()
            si["loc"]["road_num"] = 1
            si = ms.resolve(dm, pool, si)
        res = self.run(cfg, dm.default_ego_model() if model is None else model, si, [(po, _state(dm, k, a)) for po, k, a in steps],
                       dict(map=pool) if map_mode else dict(lane_pool=pool))
        return [(r.out[0], int(r.flags[0])) for r in res]

    def __call__(self, cfg, si, po, pool, near_id=10, afresh=0, map_mode=False, model=None):
        return self.steps(cfg, si, [(po, near_id, afresh)], pool, model, map_mode)[0]


_LOG = []


def _runner(name, log=None):
    return ab.Runner(ab.ModelBackend() if name == "model" else ab.DeviceBackend(), log)


@pytest.fixture()
def cfg0(dm):
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    return cfg


def _kat_speed(dm, cfg0, adv):
    # defaults: dt 0.1 s, max_acc 2, max_dec 4 -> at most 2*0.1*3.6 = 0.72 km/h up, 4*0.1*3.6 = 1.44 km/h down per tick
    assert [float(dm.default_ego_model()[k][0]) for k in ("dt", "max_acc", "max_dec")] == [0.1, 2.0, 4.0]
    si, pool = _scene(dm, cfg0)

    def next_speed(v, desaccVd, desacc, desspd):
        """The speed one advance gives (path from x = 0 at 0.5 m: with k0 = 0 the ego's x is t * 0.5 = s, the length gone, exactly)."""
        si["loc"]["velocity"] = v
        po = _straight(dm, x0=0.0)
        po["result"]["desaccVd"], po["result"]["desacc"], po["result"]["desspd"] = desaccVd, desacc, desspd
        out, f = adv(cfg0, si, po, pool, near_id=0)
        assert f == 0
        return float(out["loc"]["velocity"]), float(out["loc"]["globalpoint"]["x"])
    assert next_speed(36.0, 0, 0.0, 36.0)[0] == 36.0                 # at the target: held
    assert next_speed(0.0, 0, 0.0, 30.0)[0] == 2.0 * 0.1 * 3.6       # rate limit up: 0 + 0.72
    assert next_speed(29.5, 0, 0.0, 30.0)[0] == 30.0                 # 29.5 + 0.72 > 30: the target
    assert next_speed(30.0, 0, 0.0, 0.0)[0] == 30.0 - 4.0 * 0.1 * 3.6   # rate limit down: 30 - 1.44
    assert next_speed(1.0, 0, 0.0, 0.0)[0] == 0.0                    # 1 - 1.44 < 0: the target
    assert next_speed(20.0, 0, 0.0, math.inf)[0] == 20.0             # a non-finite desspd holds v
    assert next_speed(20.0, 0, 0.0, -math.inf)[0] == 20.0
    # desaccVd: v + desacc*dt*3.6, never below 0: 5 - 3*0.1*3.6 = 3.92; 1 - 1.08 < 0 -> 0 (the rate limits do not apply)
    assert next_speed(5.0, 1, -3.0, 99.0)[0] == 5.0 + -3.0 * 0.1 * 3.6
    assert abs(next_speed(5.0, 1, -3.0, 99.0)[0] - 3.92) < 1e-12
    assert next_speed(1.0, 1, -3.0, 99.0)[0] == 0.0
    # distance: mean of the two speeds over dt: (36 + 36)/2 km/h = 10 m/s for 0.1 s = 1 m; braking 1 -> 0 km/h: 0.5/3.6*0.1 m
    assert next_speed(36.0, 0, 0.0, 36.0)[1] == 1.0
    assert abs(next_speed(1.0, 0, 0.0, 0.0)[1] - 0.5 / 36.0) < 1e-15
    if adv.name == "model":                                          # ... and the two functions of the model by themselves
        assert em.next_speed(29.5, 0, 0.0, 30.0, 0.1, 2.0, 4.0) == 30.0 and em.next_speed(1.0, 1, -3.0, 99.0, 0.1, 2.0, 4.0) == 0.0
        assert em.step_length(36.0, 36.0, 0.1) == 1.0 and abs(em.step_length(1.0, 0.0, 0.1) - 0.5 / 36.0) < 1e-15


def _kat_straight_path_lands_on_a_point(dm, cfg0, adv):
    # v = v' = 36 km/h -> s = 1 m.  Start P[10] = (105, 0); segments of 0.5 m: a = 0.5 after segment 10, a + L = 1.0 >= s on
    # segment 11 with t = (1 - 0.5)/0.5 = 1 -> x = 105.5 + 1*0.5 = 106 exactly (the ego ends ON point 12, on segment 11), dir 0
    si, pool = _scene(dm, cfg0)
    po = _straight(dm)
    po["result"]["desspd"] = 36.0
    out, f = adv(cfg0, si, po, pool)
    g = out["loc"]["globalpoint"]
    assert (float(g["x"]), float(g["y"]), float(g["dir"]), float(out["loc"]["velocity"]), f) == (106.0, 0.0, 0.0, 36.0, 0)
    # ids: lane points x = 100 + 0.5 k -> point 12 of every view, searched over [50, 82)?  No: the ids start at 50 = x 125, ahead
    # of the ego; ids never go backwards, the nearest point of [50, 82) to x = 106 is 50 itself
    assert out["loc"]["id"].tolist() == [50, 50, 50, 50, 50, 50, 50, 50]
    # a path that was replanned starts at the ego: k0 = 0 whatever the (old-path) index says -> 100 + 1 = 101
    out, f = adv(cfg0, si, po, pool, near_id=150, afresh=1)
    assert float(out["loc"]["globalpoint"]["x"]) == 101.0 and f == 0
    # between two points: v = 18 -> s = 0.5*(18 + 18)/3.6*0.1 = 0.5 m ... and 27 km/h -> 0.75 m: segment 11, t = 0.5 -> 105.75
    si["loc"]["velocity"] = 27.0
    po["result"]["desspd"] = 27.0
    out, f = adv(cfg0, si, po, pool)
    assert abs(float(out["loc"]["globalpoint"]["x"]) - 105.75) < 1e-12 and f == 0
    # everything else is carried over
    for name in ("dec", "lanes", "ref_off", "ref_n", "obs_off", "obs_n", "stub_attribute", "out_lane_no", "period_last", "grid_origin", "goal"):
        assert out[name].tobytes() == si[0][name].tobytes()


def _kat_zero_length_segment_and_standstill(dm, cfg0, adv):
    si, pool = _scene(dm, cfg0)
    po = _straight(dm)
    po["result"]["desspd"] = 36.0
    # points 11 and 12 coincide (segment 11 has length 0 and is skipped): from P[10] = 105: segment 10 -> a = 0.5, segment 11
    # skipped, segment 12 runs from 105.5 (P[12] moved onto P[11]) to 106.5: L = 1, t = (1 - 0.5)/1 = 0.5 -> x = 106.0
    po["road_points"]["x"][0, 12] = po["road_points"]["x"][0, 11]
    out, f = adv(cfg0, si, po, pool)
    assert float(out["loc"]["globalpoint"]["x"]) == 106.0 and float(out["loc"]["globalpoint"]["dir"]) == 0.0 and f == 0
    # standstill: v = v' = 0 -> s = 0: the ego sits on P[k0] and keeps its heading (no segment)
    si["loc"]["velocity"] = 0.0
    po["result"]["desspd"] = 0.0
    out, f = adv(cfg0, si, po, pool)
    assert (float(out["loc"]["globalpoint"]["x"]), float(out["loc"]["globalpoint"]["dir"]), f) == (105.0, 77.0, 0)


def _kat_path_end_and_bad_path(dm, cfg0, adv):
    si, pool = _scene(dm, cfg0)
    po = _straight(dm)
    po["result"]["desspd"] = 36.0
    # from P[198] = 199 only one segment of 0.5 m is left, s = 1 m: the ego stops on P[199] = 199.5, heading of segment 198
    out, f = adv(cfg0, si, po, pool, near_id=198)
    assert (float(out["loc"]["globalpoint"]["x"]), float(out["loc"]["globalpoint"]["dir"]), f) == (199.5, 0.0, em.PATH_END)
    assert float(out["loc"]["velocity"]) == 36.0
    # from P[197]: a + L = 1.0 >= s on segment 198: the step ENDS on point 199, it does not reach past it
    out, f = adv(cfg0, si, po, pool, near_id=197)
    assert (float(out["loc"]["globalpoint"]["x"]), f) == (199.5, 0)
    # a NaN two points ahead (P[12]) is on the walked part (segment 11 is needed for s = 1): loc untouched, BAD_PATH
    po["road_points"]["y"][0, 12] = np.nan
    out, f = adv(cfg0, si, po, pool)
    assert f == em.BAD_PATH and out["loc"].tobytes() == si[0]["loc"].tobytes()
    # the same NaN beyond the walked part (s = 0.5 m ends on segment 10) does not matter
    si["loc"]["velocity"] = 18.0
    po["result"]["desspd"] = 18.0
    out, f = adv(cfg0, si, po, pool)
    assert (float(out["loc"]["globalpoint"]["x"]), f) == (105.5, 0)
    # a frozen scene is carried over unchanged and keeps its flags.  The flag is reached the honest way: the step of
    # test_kat_lane_end (100 lane points, from 133 to 134 = point 68: 68 + 32 >= 100) sets LANE_END, the next step finds it set
    se, _ = _scene(dm, cfg0, ego_id=60)
    se["lanes"]["cur_n"] = 100
    pe = _straight(dm, x0=133.0)
    pe["result"]["desspd"] = 36.0
    (mid, f0), (out, f) = adv.steps(cfg0, se, [(pe, 0, 0), (_straight(dm), 10, 0)], pool)
    assert (f0, float(mid["loc"]["globalpoint"]["x"]), int(mid["loc"]["id"][1])) == (em.LANE_END, 134.0, 68)
    assert f == em.LANE_END and out.tobytes() == mid.tobytes()
    if adv.name == "model":                                          # the model takes the flag word as it is given
        st = _state(dm)
        o, fl, _ = em.advance(cfg0, dm.default_ego_model(), si, _straight(dm), st, np.array([em.LANE_END], np.int32), pool, False)
        assert int(fl[0]) == em.LANE_END and o[0].tobytes() == si[0].tobytes()


def _kat_ids(dm, cfg0, adv):
    si, pool = _scene(dm, cfg0, ego_id=50, v=36.0)
    # ego to x = 125.25 + 1.0: path from x0 = 125.25, k0 = 0, s = 1 -> x = 126.25, exactly between lane points 52 (126.0) and
    # 53 (126.5): d2 = 0.0625 for both in the current view -> the FIRST minimum, 52.  Left / right views (|dy| = 3.75): 52 too.
    po = _straight(dm, x0=125.25)
    po["result"]["desspd"] = 36.0
    out, f = adv(cfg0, si, po, pool, near_id=0)
    assert float(out["loc"]["globalpoint"]["x"]) == 126.25
    assert out["loc"]["id"].tolist() == [52, 52, 52, 50, 50, 50, 50, 50] and f == 0       # slots 1 (cur), 0 (left), 2 (right)
    # window edge: window 4 searches [50, 54) only; the ego at x = 131 (point 62) gets the last point of the window, 53
    model = dm.default_ego_model()
    model["window"] = 4
    po = _straight(dm, x0=130.0)
    po["result"]["desspd"] = 36.0
    out, f = adv(cfg0, si, po, pool, near_id=0, model=model)
    assert out["loc"]["id"].tolist() == [53, 53, 53, 50, 50, 50, 50, 50]
    # an empty view keeps its id: no right lane (right_n = 0), and an id at / beyond the end of its view
    si2 = si.copy()
    si2["lanes"]["right_n"] = 0
    si2["loc"]["id"][0, 0] = 400                                     # left view: [400, ...) of 320 points is empty
    out, f = adv(cfg0, si2, po, pool, near_id=0)
    assert out["loc"]["id"].tolist() == [400, 62, 50, 50, 50, 50, 50, 50]
    # lane 1 has no left view, lane 3 (= lane_sum) no right view: slots 0 / 1 and 1 / 2 only
    si3, _ = _scene(dm, cfg0, lane_num=1)
    out, f = adv(cfg0, si3, po, pool, near_id=0)
    assert out["loc"]["id"].tolist() == [62, 62, 50, 50, 50, 50, 50, 50]
    si3, _ = _scene(dm, cfg0, lane_num=3)
    out, f = adv(cfg0, si3, po, pool, near_id=0)
    assert out["loc"]["id"].tolist() == [50, 62, 62, 50, 50, 50, 50, 50]


def _kat_lane_end(dm, cfg0, adv):
    # 100 points in the current lane, window 32: LANE_END once id' + 32 >= 100, i.e. from id' = 68 on
    si, pool = _scene(dm, cfg0, ego_id=60)
    si["lanes"]["cur_n"] = 100
    for x0, want_id, want_f in ((132.5, 67, 0), (133.0, 68, em.LANE_END)):      # + 1 m: x = 133.5 = point 67, 134.0 = point 68
        po = _straight(dm, x0=x0)
        po["result"]["desspd"] = 36.0
        out, f = adv(cfg0, si, po, pool, near_id=0)
        assert (int(out["loc"]["id"][1]), f) == (want_id, want_f)


def _kat_lane_switch_margin(dm, cfg0, adv):
    # lane width 3.75 -> margin 0.9375.  The ego at lateral offset e from the current lane (same x as a lane point, so the
    # distances are |e| and 3.75 - |e| exactly): switch when |e| - (3.75 - |e|) > 0.9375, i.e. |e| > 2.34375 (= 75/32, exact).
    # Map mode is a resident map: the three lanes of _scene as one road of a map store (_map3), the views resolved from it
    si, pool = _scene(dm, cfg0, ego_id=50, v=36.0)
    m = _map3(dm)
    for e, want in ((2.34375, 2), (2.375, 1), (-2.34375, 2), (-2.375, 3), (0.0, 2)):
        po = _straight(dm, x0=125.0, y=e)
        po["result"]["desspd"] = 36.0
        out, f = adv(cfg0, si, po, m, near_id=0, map_mode=True)
        assert (int(out["loc"]["lane_num"]), f) == (want, 0), e
        assert int(out["lanes"]["cur_off"]) == 320 * (want - 1)                   # the views are those of the new lane
        out, f = adv(cfg0, si, po, pool, near_id=0, map_mode=False)          # slice mode: held
        assert int(out["loc"]["lane_num"]) == 2
    if adv.name == "model":                                          # the model's map mode on the slices themselves, without a map
        po = _straight(dm, x0=125.0, y=2.375)
        po["result"]["desspd"] = 36.0
        o, fl, _ = em.advance(cfg0, dm.default_ego_model(), si, po, _state(dm, 0), np.zeros(1, np.int32), pool, True)
        assert (int(o["loc"]["lane_num"][0]), int(fl[0])) == (1, 0)
    # off grid: a 128 x 128 grid of 0.25 m cells from the origin (100, -16): x = 126 is cell 104, x = 132.5 would be cell 130
    # (the goal lies on the grid: the tick the device's advance follows searches it)
    cfg = dm.default_config(128)
    si["grid_origin"]["x"], si["grid_origin"]["y"] = 100.0, -16.0
    si["goal"]["x"], si["goal"]["y"] = 128.0, 0.0
    for x0, want in ((125.0, 0), (131.5, em.OFF_GRID)):
        po = _straight(dm, x0=x0)
        po["result"]["desspd"] = 36.0
        assert adv(cfg, si, po, pool, near_id=0)[1] == want


KATS = [_kat_speed, _kat_straight_path_lands_on_a_point, _kat_zero_length_segment_and_standstill, _kat_path_end_and_bad_path, _kat_ids, _kat_lane_end, _kat_lane_switch_margin]


def test_kat_speed(dm, cfg0):
    _kat_speed(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_straight_path_lands_on_a_point(dm, cfg0):
    _kat_straight_path_lands_on_a_point(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_zero_length_segment_and_standstill(dm, cfg0):
    _kat_zero_length_segment_and_standstill(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_path_end_and_bad_path(dm, cfg0):
    _kat_path_end_and_bad_path(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_ids(dm, cfg0):
    _kat_ids(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_lane_end(dm, cfg0):
    _kat_lane_end(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_lane_switch_margin(dm, cfg0):
    _kat_lane_switch_margin(dm, cfg0, _Adv(dm, _runner("model")))


@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg0, kat):
    """The known answers above on k_advance_egos (injected PlanOut / SceneState), each also held against the model step by step."""
    kat(dm, cfg0, _Adv(dm, _runner("device")))


@gpu
def test_kat_batch_equals_each_case_alone(dm, cfg0):
    """Every known answer above once more on the device, logged, then all of them as distinct scenes of one launch per group of
    calls that can share a launch (advance_backends.batched): batch sizes that are no multiple of four, more than one block;
    every scene gives the bytes it gave alone."""
    log = []
    a = _Adv(dm, _runner("device", log))
    for kat in KATS:
        kat(dm, cfg0, a)
    sizes = ab.batched(ab.DeviceBackend(), log)
    print(f"{len(log)} calls in batches of {sizes}; device against model: {ab.STATS}")
    assert sum(sizes) >= len(log) and all(n % 4 != 0 and n > 4 for n in sizes)


# ---------------------------------------------------------------------------------------------------------------
# GPU
TICKS = 30
_RUNS = {}


def _closed_loop(dm, which):
    """30 ticks of advance + tick + pp_fetch_async with pp_get_scene_in after each advance; everything the device read and wrote."""
    if which in _RUNS:
        return _RUNS[which]
    n, first, je = {"c1": (1024, 0, 0), "junc": (256, 5000, 8)}[which]
    cfg = dm.default_config(512)
    n_obs = 64
    sc = dm.gen_scenes(cfg, first, n, n_obs, junction_every=je)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    model = dm.default_ego_model()
    plan_p, grid_p = dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut)
    run = dict(cfg=cfg, sc=sc, n=n, model=model, sin=[pl.get_scene_in()], plan=[], grid=[], state=[], flags=[np.zeros(n, np.int32)])
    for t in range(TICKS + 1):
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p, grid_p)) == 0
        run["plan"].append(np.array(plan_p)), run["grid"].append(np.array(grid_p)), run["state"].append(pl.get_state())
        if t < TICKS:
            pl.advance_async(model)
            run["sin"].append(pl.get_scene_in())
            run["flags"].append(pl.ego_flags())
    pl.close()
    _RUNS[which] = run
    return run


@gpu
@pytest.mark.parametrize("which", ["c1", "junc"])
def test_step_check_against_the_model(dm, which):
    """No compounding: the numpy model applied to the device's own SceneIn_t, PlanOut_t, SceneState_t gives the device's
    SceneIn_{t+1}: integers exact, x / y / velocity within 1e-9, dir within 1e-6 degrees; ties below 1e-9 in squared distance
    may be left out of the id comparison, at most 0.5 % of the scene-ticks."""
    r = _closed_loop(dm, which)
    n, left_out, moved = r["n"], 0, 0
    for t in range(TICKS):
        want, wflags, gaps = em.advance(r["cfg"], r["model"], r["sin"][t], r["plan"][t], r["state"][t], r["flags"][t], r["sc"]["lane_pool"])
        got = r["sin"][t + 1]
        tie = gaps < 1e-9
        left_out += int(tie.sum())
        assert np.array_equal(r["flags"][t + 1], wflags), f"tick {t}: flags"
        assert np.array_equal(got["loc"]["lane_num"], want["loc"]["lane_num"])
        assert np.array_equal(got["loc"]["id"][~tie], want["loc"]["id"][~tie]), f"tick {t}: ids"
        for f in ("x", "y"):
            d = np.abs(got["loc"]["globalpoint"][f] - want["loc"]["globalpoint"][f])
            assert d.max() <= 1e-9, f"tick {t}: {f} off by {d.max()}"
        assert np.abs(got["loc"]["velocity"] - want["loc"]["velocity"]).max() <= 1e-9
        dd = np.abs(got["loc"]["globalpoint"]["dir"] - want["loc"]["globalpoint"]["dir"])
        assert np.minimum(dd, 360.0 - dd).max() <= 1e-6, f"tick {t}: dir"
        rest_g, rest_w = got.copy(), want.copy()
        rest_g["loc"], rest_w["loc"] = 0, 0
        assert rest_g.tobytes() == rest_w.tobytes(), f"tick {t}: the carried-over part"
        for f in ("pos", "road_num", "last_roadnum", "next_roadnum", "last_lanenum", "next_lanenum", "path_num"):
            assert np.array_equal(got["loc"][f], want["loc"][f])
        moved += int((got["loc"]["globalpoint"]["x"] != r["sin"][t]["loc"]["globalpoint"]["x"]).sum())
    share = left_out / float(n * TICKS)
    print(f"{which}: {left_out} of {n * TICKS} scene-ticks left out of the id comparison ({100 * share:.3f} %), {moved} moved, "
          f"flags at the end: {np.bincount(r['flags'][-1], minlength=16).tolist()}")
    assert share <= 0.005
    assert moved > n * TICKS // 4                       # the egos do move


@gpu
@pytest.mark.parametrize("which", ["c1", "junc"])
def test_closed_loop_plans_what_the_open_loop_plans(dm, oracle, which):
    """A second handle fed the traced SceneIn_t through pp_update_async gives the rollout handle's PlanOut, GridOut and
    SceneState bit for bit at every tick; the oracle, given the device's SceneIn_t and state, agrees within the usual bounds."""
    r = _closed_loop(dm, which)
    n, cfg, sc = r["n"], r["cfg"], r["sc"]
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * 64)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    plan_p, grid_p = dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut)
    for t in range(TICKS + 1):
        if t:
            in_t = dm.pinned_copy(r["sin"][t])
            pl.update_async(in_t)
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p, grid_p)) == 0
        assert np.array(plan_p).tobytes() == r["plan"][t].tobytes(), f"tick {t}: PlanOut"
        assert np.array(grid_p).tobytes() == r["grid"][t].tobytes(), f"tick {t}: GridOut"
        assert pl.get_state().tobytes() == r["state"][t].tobytes(), f"tick {t}: SceneState"
    pl.close()
    for t in range(TICKS + 1):
        st_o = (r["state"][t - 1] if t else sc["state"]).copy()
        plan_o, gout_o, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=r["sin"][t], mot_pool=None), st_o, n_threads=16)
        bad = compare(r["plan"][t], plan_o, "plan") + compare(r["state"][t], st_o, "state")
        bad += compare(r["grid"][t]["status"], gout_o["status"], "grid.status")
        keep = (gout_o["status"] != 3) & (gout_o["status"] != 7)      # OVERFLOW / COST_RANGE: only the status is specified
        bad += compare(r["grid"][t][keep], gout_o[keep], "grid")
        assert not bad, f"tick {t}\n" + "\n".join(bad[:20])


@gpu
@pytest.mark.parametrize("n", [128, 1024])
def test_rollout_equals_its_parts(dm, n):
    """pp_rollout(K) = K x (advance, tick), bit for bit, below pipeline_min (one stream) and above it (piped)."""
    K, n_obs = 12, 32
    cfg = dm.default_config(256)
    sc = dm.gen_scenes(cfg, 700, n, n_obs, junction_every=8)
    model = dm.default_ego_model()
    outs = []
    for whole in (False, True):
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
        pl.set_scenes(sc, with_motion=False)
        pl.set_state(sc["state"])
        sins = []
        if whole:
            assert np.array_equal(pl.ego_flags(), np.zeros(n, np.int32))          # a handle that never advanced
            last, trace = pl.rollout(K, model, trace=True)
            assert last == K + 1 == pl.tick_id()
        else:
            pl.tick()
            for t in range(K):
                pl.advance_async(model)
                sins.append(pl.get_scene_in())
                pl.tick()
        pl.sync()
        outs.append((pl.get_plan(), pl.get_grid_out(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), sins, np.array(trace) if whole else None))
        pl.close()
    a, b = outs
    for k, name in enumerate(("PlanOut", "GridOut", "SceneState", "flags", "SceneIn")):
        assert a[k].tobytes() == b[k].tobytes(), name
    trace, sins = b[6], a[5]
    for t in range(K):
        loc = sins[t]["loc"]
        assert trace[t]["pose"].tobytes() == loc["globalpoint"].tobytes() and trace[t]["velocity"].tobytes() == loc["velocity"].tobytes()
        assert np.array_equal(trace[t]["lane_num"], loc["lane_num"])
        assert np.array_equal(trace[t]["id_cur"], loc["id"][np.arange(n), np.clip(loc["lane_num"] - 1, 0, 7)])
    assert np.array_equal(trace[K - 1]["flags"], b[3])
    assert (trace[K - 1]["pose"]["x"] != sc["scene_in"]["loc"]["globalpoint"]["x"]).mean() > 0.5


@gpu
@pytest.mark.parametrize("copies", [1, 300])
def test_known_answer_speed_ramp(dm, copies):
    """One straight three-lane road, no obstacles, velocity_expect 30 km/h (decision stage off: DecisionOut is the caller's),
    start speed 0, default model (0.72 km/h per tick up), 50 rollout ticks, replanning every tick (the path starts at the ego).
    Speeds: v_k = 0.72 k for k <= 41 (29.52), v_42 = min(30, 30.24) = 30, then 30.  Sum of the tick means (v_{k-1} + v_k)/2:
    k = 1..41: 0.72 * sum(k - 1/2) = 0.72 * (861 - 20.5) = 605.16;  k = 42: (29.52 + 30)/2 = 29.76;  k = 43..50: 8 * 30 = 240;
    total 874.92 km/h-ticks = 874.92 / 3.6 * 0.1 = 24.30333... m."""
    import lanechange_scenes as lcs
    from kat_backends import replicate
    cfg = dm.default_config(128)
    cfg["decision_stage"], cfg["force_replan"] = 0, 1
    sc = lcs.make_scene(dm, cfg, lane_num=2, obstacles=())
    sc["scene_in"]["dec"]["velocity_expect"], sc["scene_in"]["dec"]["behavior"], sc["scene_in"]["dec"]["target_lanenum"] = 30.0, 1, 2
    sc["scene_in"]["loc"]["velocity"] = 0.0
    x0 = float(sc["scene_in"]["loc"]["globalpoint"]["x"][0])
    sc["scene_in"]["grid_origin"]["x"] = x0 - 2.0           # the 32 m grid (128 cells of 0.25 m) holds the whole drive and the goal 20 m ahead
    sc = replicate(sc, copies)
    pl = dm.Planner(cfg, device=0, max_scenes=copies, max_obs_total=1)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    _, trace = pl.rollout(50, trace=True)
    pl.sync()
    trace = np.array(trace)
    want = 874.92 / 3.6 * 0.1
    got = trace[-1]["pose"]["x"] - x0
    print(f"copies {copies}: travelled {got[0]!r} m, closed form {want!r} m, final speed {trace[-1]['velocity'][0]!r}, flags {trace[-1]['flags'][0]}")
    assert np.abs(got - want).max() <= 1e-6
    assert (trace[-1]["velocity"] == 30.0).all() and abs(float(trace[40]["velocity"][0]) - 29.52) < 1e-9
    assert np.abs(trace[-1]["pose"]["y"] - (200.0 - lcs.LANE_W)).max() <= 1e-9 and (trace[-1]["flags"] == 0).all()
    assert all(trace[:, k].tobytes() == trace[:, 0].tobytes() for k in range(copies))
    assert int(trace[-1]["id_cur"][0]) == lcs.EGO_ID + 49          # x = 125 + 24.30 -> lane point 50 + 48.6, nearest 99 (x = 149.5)
    pl.close()


@gpu
def test_map_mode_lane_change_is_followed(dm):
    """On the map store an ego whose path leads into the neighbouring lane ends with lane_num changed, and its lane views are
    resolve() of tests/map_scenes.py - and a fresh pp_set_egos - at the traced pose."""
    import map_scenes as ms
    cfg = dm.default_config(128)
    m = ms.build_map(dm, n_roads=5)
    n, n_obs = 96, 16
    sc = ms.make_egos(dm, cfg, m, n, n_obs)
    # placed by hand as well, so that the test does not hang on what the generated egos decide: ego 0 is three quarters of the
    # way through a change to the left - road 1, localised on lane 2 at point 40, but 2.8 m to the left of it (lane 1 is 3.75 m
    # to the left: 0.95 m away against 2.8 m, more than the quarter width 0.94 m closer) - and free of obstacles
    L2 = m["lanes"][int(m["road_first_lane"][0]) + 1]
    p = m["points"][int(L2["point_off"]) + 40]
    loc0 = sc["scene_in"]["loc"][0]
    loc0["pos"], loc0["road_num"], loc0["lane_num"], loc0["velocity"] = 0, 1, 2, 20.0
    loc0["last_roadnum"], loc0["next_roadnum"], loc0["last_lanenum"], loc0["next_lanenum"] = 1, 2, 2, 2
    loc0["id"][:] = 40
    loc0["globalpoint"]["x"], loc0["globalpoint"]["y"], loc0["globalpoint"]["dir"] = float(p["x"]), float(p["y"]) + 2.8, float(p["dir"])
    sc["scene_in"]["obs_n"][0] = 0
    sc["scene_in"]["grid_origin"][0]["x"], sc["scene_in"]["grid_origin"][0]["y"] = float(p["x"]) - 3.0, float(p["y"]) - 16.0
    sc["scene_in"]["goal"][0]["x"], sc["scene_in"]["goal"][0]["y"] = float(p["x"]) + 25.0, float(p["y"])
    caps = dict(max_scenes=n, max_obs_total=n * n_obs, max_lane_pts_total=len(m["points"]), max_ref_pts_total=max(len(m["jpoints"]), 1))
    pl = dm.Planner(cfg, device=0, **caps)
    pl.set_map(m)
    pl.set_egos(sc)
    pl.set_state(sc["state"])
    first = pl.get_scene_in()
    model = dm.default_ego_model()
    model["window"] = 48
    _, trace = pl.rollout(60, model, trace=True)
    pl.sync()
    trace, last = np.array(trace), pl.get_scene_in()
    changed = np.flatnonzero(last["loc"]["lane_num"] != first["loc"]["lane_num"])
    print("lane numbers changed for scenes", changed.tolist(), "flags", np.bincount(pl.ego_flags(), minlength=16).tolist())
    assert len(changed) > 0                                             # generated egos that ended in another lane
    assert int(trace[0]["lane_num"][0]) == 1                            # the hand-placed one is followed at the first advance
    assert any(int(sc["scene_in"]["obs_n"][k]) > 0 for k in changed)
    assert np.array_equal(trace[-1]["lane_num"], last["loc"]["lane_num"])
    assert np.abs(last["loc"]["lane_num"] - first["loc"]["lane_num"]).max() <= 60
    want = ms.resolve(dm, m, last)
    assert not compare(last, want, "scene_in")
    fresh = dm.Planner(cfg, device=0, **caps)
    fresh.set_map(m)
    raw = last.copy()
    raw["lanes"] = 0
    raw["ref_off"], raw["ref_n"] = 0, 0
    fresh.set_egos(dict(sc, scene_in=raw))
    assert fresh.get_scene_in().tobytes() == last.tobytes()
    fresh.close(), pl.close()


@gpu
def test_frozen_scenes_sticky_flags_and_state_errors(dm):
    n, n_obs = 64, 8
    cfg = dm.default_config(128)
    sc = dm.gen_scenes(cfg, 40, n, n_obs, junction_every=0)
    sc["scene_in"]["lanes"]["cur_n"][:8] = 80                 # these are within 32 points of their lane end at once (id 50 or 51: + 32 >= 80)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    model = dm.default_ego_model()
    with pytest.raises(dm.PlannerError, match="-4"):          # PP_ERR_STATE: no tick yet
        pl.advance_async(model)
    pl.tick()
    pl.update_async(dm.pinned_copy(sc["scene_in"]))
    with pytest.raises(dm.PlannerError, match="-4"):          # ... and on top of a staged update
        pl.advance_async(model)
    pl.tick()
    pl.advance_async(model)
    with pytest.raises(dm.PlannerError, match="-4"):          # two advances for one tick
        pl.advance_async(model)
    with pytest.raises(dm.PlannerError, match="-4"):          # new SceneIn records on top of a staged advance
        pl.update_async(dm.pinned_copy(sc["scene_in"]))
    f1, s1 = pl.ego_flags(), pl.get_scene_in()
    assert (f1[:8] & dm.EGO_LANE_END).all()
    assert (s1["loc"]["globalpoint"]["x"][:8] != sc["scene_in"]["loc"]["globalpoint"]["x"][:8]).any()      # flagged by the step that moved them
    flags = [f1]
    for t in range(20):
        pl.tick()
        pl.advance_async(model)
        flags.append(pl.ego_flags())
        s = pl.get_scene_in()
        frozen = flags[-2] != 0
        assert s[frozen].tobytes() == s1[frozen].tobytes() if t == 0 else s[frozen].tobytes() == prev[frozen].tobytes()
        assert ((flags[-1] & flags[-2]) == flags[-2]).all()   # sticky
        prev = s
    pl.tick()
    pl.sync()
    assert pl.get_plan()["result"]["cnt"].max() > 0             # frozen scenes still tick
    pl.set_scenes(sc, with_motion=False)                        # new scenes: flags cleared
    assert not pl.ego_flags().any()
    with pytest.raises(dm.PlannerError, match="-4"):
        pl.advance_async(model)
    pl.close()
