"""A grid that follows the ego (pp_set_grid_follow): the advance step re-centres grid_origin and goal.

CPU: the ABI mirror, hand-written known answers on the numpy model (tests/grid_follow_model.py), and the closed loop of oracle tick
+ models on the ring of tests/route_scenes.py with the grid stage on - every ego stays on its grid through a junction with
following on and is frozen with OFF_GRID without it.
GPU: the same known answers on k_advance_egos (slice mode) and k_advance_route (routed egos on a map), alone and as distinct
scenes of one launch; following switched off is the engine without it, byte for byte; the error paths; the closed loop against the
model step by step on the device's own records with every GridOut against the oracle; the scorecard's grid ticks.

The known answers stand still (0 km/h towards 0 km/h: s = 0, the new position is P[0] to the bit) unless they say otherwise, so the
ego's position and the goal point are whatever the case writes into the path, and every expected word is worked out in the comment
above its assertion at cell = 0.25."""
import numpy as np
import pytest

import ego_model as em
import grid_follow_backends as gb
import grid_follow_model as gfm
import map_scenes as ms
import route_model as rmod
import route_scenes as rs
from parity_util import compare
from test_rollout import _scene
from test_route import _assert_records, _ego, _legs, _path, _planner, _tiny_map

gpu = pytest.mark.gpu
FAR = (1000.0, 1000.0)          # a frame nowhere near the ego: never held


def _cfg(dm, w=128, h=None, grid_stage=1):
    cfg = dm.default_config(128)
    cfg["grid_w"], cfg["grid_h"], cfg["grid_stage"] = w, h or w, grid_stage
    return cfg


def _gf(dm, goal_point=199, margin=32):
    gf = dm.default_grid_follow()
    gf["goal_point"], gf["margin_cells"] = goal_point, margin
    return gf


def _still(dm, ego, goal, goal_point=199):
    """PlanOut of an ego that stands on P[0] = ego: desspd 0; P[goal_point] = goal, every other point one more metre along +x."""
    po = np.zeros(1, dm.PlanOut)
    po["road_points"]["x"][0] = ego[0] + 1.0 * np.arange(200)
    po["road_points"]["y"][0] = ego[1]
    po["road_points"]["x"][0, goal_point], po["road_points"]["y"][0, goal_point] = goal
    return po


def _frame(out):
    o, g = out["grid_origin"], out["goal"]
    return float(o["x"]), float(o["y"]), float(g["x"]), float(g["y"])


def _bits(*v):
    return np.array(v, np.float64).tobytes()


class _Adv:
    """One scene on one kernel: kind "egos": three straight lanes in slice mode (k_advance_egos); kind "route": the routed ego of
    tests/test_route.py on its tiny map (k_advance_route).  Called with the frame the scene starts from and one PlanOut per step."""
    def __init__(self, dm, name, kind, log=None):
        self.dm, self.name, self.kind, self.log = dm, name, kind, log

    def scene(self, cfg, v=0.0):
        dm = self.dm
        if self.kind == "egos":
            si, pool = _scene(dm, cfg, v=v)
            return si, dict(lane_pool=pool), None
        m = _tiny_map(dm)
        legs = _legs(dm)
        return _ego(dm, m, v=v), dict(map=m), (legs, np.array([0, len(legs)], np.int32), None)

    def steps(self, cfg, gf, origin, goal, pos, si=None, v=0.0):
        base, world, route = self.scene(cfg, v)
        si = base if si is None else si
        si = si.copy()
        si["grid_origin"]["x"], si["grid_origin"]["y"] = origin
        si["goal"]["x"], si["goal"]["y"] = goal
        run = gb.Runner(self.name, gf, self.log)
        res = run(cfg, self.dm.default_ego_model(), si, [(po, np.zeros(1, self.dm.SceneState)) for po in pos], world, route)
        return si, [(r.out[0], int(r.flags[0])) for r in res]

    def __call__(self, cfg, gf, origin, goal, po, **kw):
        si, res = self.steps(cfg, gf, origin, goal, [po], **kw)
        return res[0]


# ---------------------------------------------------------------------------------------------------------------
# known answers: 128 x 128 cells of 0.25 m (32 m), margin 32 cells (8 m), goal point 199, the grid stage on
def _kat_mixed_block(dm, adv):
    """Held, re-centred, skipped and frozen, two steps each: the first four scenes of the batched launch."""
    cfg, gf = _cfg(dm), _gf(dm)
    # held twice: ego (8.1, 12) -> cells (32, 48), goal (23.9, 12) -> cells (95, 48): 32 <= all < 96.  The frame stays (0, 0), the
    # goal is the path point; then the goal moves to (20, 13): cells (80, 52), held again
    si, ((a, fa), (b, fb)) = adv.steps(cfg, gf, (0.0, 0.0), (1.0, 1.0), [_still(dm, (8.1, 12.0), (23.9, 12.0)), _still(dm, (8.1, 12.0), (20.0, 13.0))])
    assert (_frame(a), fa) == ((0.0, 0.0, 23.9, 12.0), 0) and (_frame(b), fb) == ((0.0, 0.0, 20.0, 13.0), 0)
    # re-centred, then held in the new frame.  x: 10.3 + 30.1 = 40.4, half 20.2, / 0.25 = 80.8 -> 80, - 64 = 16 cells = 4.0;
    # y: -0.3 + 0.1 = -0.2, half -0.1, / 0.25 = -0.4 -> floor -1, - 64 = -65 cells = -16.25.  In that frame the ego is in cell
    # (25.2, 63.8) -> (25, 63): not OFF_GRID.  Step 2 from there: ego (14, 0) -> cells (40, 65), goal (26, 0) -> (88, 65): held
    si, ((a, fa), (b, fb)) = adv.steps(cfg, gf, FAR, (1.0, 1.0), [_still(dm, (10.3, -0.3), (30.1, 0.1)), _still(dm, (14.0, 0.0), (26.0, 0.0))])
    assert (_frame(a), fa) == ((4.0, -16.25, 30.1, 0.1), 0) and (_frame(b), fb) == ((4.0, -16.25, 26.0, 0.0), 0)
    # skipped twice: a NaN, then an infinite goal point - origin and goal are carried over to the byte; the old test of §4c 6. runs on
    # the held frame (0, 0): the ego at (8.1, 12) is on it
    si, ((a, fa), (b, fb)) = adv.steps(cfg, gf, (0.0, 0.0), (1.0, 1.0), [_still(dm, (8.1, 12.0), (np.nan, 12.0)), _still(dm, (8.1, 12.0), (20.0, -np.inf))])
    assert fa == 0 and fb == 0
    for out in (a, b):
        assert out["grid_origin"].tobytes() + out["goal"].tobytes() == _bits(0.0, 0.0, 1.0, 1.0)
    # OFF_GRID on the new frame, then frozen: the goal 50 m ahead of the ego at (0, 0): x: half of 50 = 25 -> 100 - 64 = 36 cells =
    # 9.0, y: 0 - 64 cells = -16.0; the ego is in cell (-36, 64): OFF_GRID, with the new frame written.  The next advance finds the
    # flag (set by a step of its own) and carries the record over to the byte, whatever the plan says
    si, ((a, fa), (b, fb)) = adv.steps(cfg, gf, (0.0, 0.0), (1.0, 1.0), [_still(dm, (0.0, 0.0), (50.0, 0.0)), _still(dm, (8.1, 12.0), (23.9, 12.0))])
    assert (_frame(a), fa) == ((9.0, -16.0, 50.0, 0.0), em.OFF_GRID)
    assert b.tobytes() == a.tobytes() and fb == em.OFF_GRID


def _kat_hold_against_recentre(dm, adv):
    """Either side of each edge of the hold test, origin (0, 0): x / 0.25 is the cell."""
    cfg, gf = _cfg(dm), _gf(dm)
    held = (0.0, 0.0)
    for ego, goal, want in (
            ((8.1, 12.0), (23.9, 12.0), held),                 # ego cell 32 = M, goal cell 95 = W - M - 1 (the mixed block again, one step)
            ((7.9, 12.0), (23.9, 12.0), (-0.25, -4.0)),        # ego cell 31 = M - 1: x: 31.8 / 2 = 15.9 -> 63.6 -> 63 - 64 = -1 cell; y: 12 -> 48 - 64 = -16 cells
            ((8.1, 12.0), (24.1, 12.0), (0.0, -4.0)),          # goal cell 96 = W - M: x: 32.2 / 2 = 16.1 -> 64.4 -> 64 - 64 = 0
            ((12.0, 8.1), (12.0, 23.9), held),                 # the same in y
            ((12.0, 7.9), (12.0, 23.9), (-4.0, -0.25)),
            ((12.0, 8.1), (12.0, 24.1), (-4.0, 0.0))):
        out, f = adv(cfg, gf, (0.0, 0.0), (1.0, 1.0), _still(dm, ego, goal))
        assert (_frame(out), f) == (want + goal, 0), (ego, goal)
    # margin 0: the whole grid holds.  Ego cell 0 and goal cell 127 are held, ego cell -1 and goal cell 128 are not
    gf0 = _gf(dm, margin=0)
    for ego, goal, want in (
            ((0.1, 12.0), (31.9, 12.0), held),
            ((-0.1, 12.0), (31.9, 12.0), (-0.25, -4.0)),       # x: 31.8 / 2 = 15.9 -> 63 - 64 = -1 cell
            ((0.1, 12.0), (32.1, 12.0), (0.0, -4.0))):         # x: 32.2 / 2 = 16.1 -> 64 - 64 = 0
        out, f = adv(cfg, gf0, (0.0, 0.0), (1.0, 1.0), _still(dm, ego, goal))
        assert (_frame(out), f) == (want + goal, 0), (ego, goal)


def _kat_skipped_goal_takes_the_old_test(dm, adv):
    """A non-finite road_points[goal_point]: the frame is held and OFF_GRID comes from §4c 6. on it: the ego at (40, 12) is in
    cell 160 of the 128 of the frame at (0, 0)."""
    cfg, gf = _cfg(dm), _gf(dm)
    out, f = adv(cfg, gf, (0.0, 0.0), (1.0, 1.0), _still(dm, (40.0, 12.0), (50.0, np.nan)))
    assert f == em.OFF_GRID and out["grid_origin"].tobytes() + out["goal"].tobytes() == _bits(0.0, 0.0, 1.0, 1.0)
    # with a finite goal the same ego is re-centred and stays on: x: 90 / 2 = 45 -> 180 - 64 = 116 cells = 29.0, ego cell 44
    out, f = adv(cfg, gf, (0.0, 0.0), (1.0, 1.0), _still(dm, (40.0, 12.0), (50.0, 12.0)))
    assert (_frame(out), f) == ((29.0, -4.0, 50.0, 12.0), 0)


def _kat_goal_points(dm, adv):
    """goal_point 1 and 199 (and 100): the goal is that point of the path and no other.  P[0] = (10.3, -0.3); P[k] is marked (k, 0.5 k)."""
    cfg = _cfg(dm)
    po = _still(dm, (10.3, -0.3), (0.0, 0.0))
    po["road_points"]["x"][0, 1:] = np.arange(1, 200)
    po["road_points"]["y"][0, 1:] = 0.5 * np.arange(1, 200)
    # 1: goal (1, 0.5): x: 11.3 / 2 = 5.65 -> 22.6 -> 22 - 64 = -42 cells = -10.5; y: 0.2 / 2 = 0.1 -> 0.4 -> 0 - 64 = -16.0
    out, f = adv(cfg, _gf(dm, 1), FAR, (1.0, 1.0), po)
    assert (_frame(out), f) == ((-10.5, -16.0, 1.0, 0.5), 0)
    # 100: goal (100, 50): x: 110.3 / 2 = 55.15 -> 220.6 -> 220 - 64 = 156 cells = 39.0; y: 49.7 / 2 = 24.85 -> 99.4 -> 99 - 64 = 35
    # cells = 8.75; the ego's cell is (10.3 - 39) / 0.25 < 0: OFF_GRID
    out, f = adv(cfg, _gf(dm, 100), FAR, (1.0, 1.0), po)
    assert (_frame(out), f) == ((39.0, 8.75, 100.0, 50.0), em.OFF_GRID)
    # 199: goal (199, 99.5): x: 209.3 / 2 = 104.65 -> 418.6 -> 418 - 64 = 354 cells = 88.5; y: 99.2 / 2 = 49.6 -> 198.4 -> 198 - 64 = 134
    # cells = 33.5
    out, f = adv(cfg, _gf(dm, 199), FAR, (1.0, 1.0), po)
    assert (_frame(out), f) == ((88.5, 33.5, 199.0, 99.5), em.OFF_GRID)


def _kat_bad_path_and_path_end(dm, adv):
    cfg, gf = _cfg(dm), _gf(dm)
    # BAD_PATH: P[0] is not finite - the record is carried over to the byte, the frame included, although the goal point is fine
    po = _still(dm, (np.nan, 12.0), (23.9, 12.0))
    si, ((out, f),) = adv.steps(cfg, gf, FAR, (1.0, 1.0), [po])
    assert f == em.BAD_PATH and out.tobytes() == si[0].tobytes()
    # PATH_END: 36 km/h held is s = 1 m, the path from (10, 0) has 199 segments of 1/1024 m: the ego stops on P[199] = 10 + 199/1024
    # = 10.1943359375, which is the goal too: x: / 0.25 = 40.77.. -> 40 - 64 = -24 cells = -6.0; y: 0 - 64 cells = -16.0
    po = _path(dm, 10.0)
    po["road_points"]["x"][0] = 10.0 + np.arange(200) / 1024.0
    out, f = adv(cfg, gf, FAR, (1.0, 1.0), po, v=36.0)
    assert (_frame(out), f) == ((-6.0, -16.0, 10.1943359375, 0.0), em.PATH_END)
    assert float(out["loc"]["globalpoint"]["x"]) == 10.1943359375


def _kat_small_grid_off_the_new_frame(dm, adv):
    """OFF_GRID on the new frame: a grid of 8 m (32 x 32 cells, the smallest the grid stage takes) whose goal lies 10 m ahead.
    x: 10 / 2 = 5 -> 20 - 16 = 4 cells = 1.0; y: 0 - 16 cells = -4.0; the ego at (0, 0) is in cell (-4, 16)."""
    cfg, gf = _cfg(dm, 32), _gf(dm, margin=4)
    out, f = adv(cfg, gf, (-4.0, -4.0), (1.0, 1.0), _still(dm, (0.0, 0.0), (10.0, 0.0)))
    assert (_frame(out), f) == ((1.0, -4.0, 10.0, 0.0), em.OFF_GRID)
    # 6 m ahead it stays on: x: 3 -> 12 - 16 = -4 cells = -1.0, ego cell (4, 16)
    out, f = adv(cfg, gf, (-4.0, -4.0), (1.0, 1.0), _still(dm, (0.0, 0.0), (6.0, 0.0)))
    assert (_frame(out), f) == ((-1.0, -4.0, 6.0, 0.0), 0)


def _kat_no_grid_stage(dm, adv):
    """grid_stage = 0: the frame is maintained, nothing is tested.  An odd, rectangular grid, W = 127 and H = 64 (W / 2 = 63, H / 2 =
    32): the midpoint of the mixed block, (20.2, -0.1) -> cells (80, -1): x: 80 - 63 = 17 cells = 4.25, y: -1 - 32 = -33 cells = -8.25.
    Non-finite held origins are re-centred (a NaN compares false; -inf / +inf cells lie outside the margins)."""
    cfg, gf = _cfg(dm, 127, 64, grid_stage=0), _gf(dm, margin=31)
    po = _still(dm, (10.3, -0.3), (30.1, 0.1))
    for origin in (FAR, (np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf)):
        out, f = adv(cfg, gf, origin, (1.0, 1.0), po)
        assert (_frame(out), f) == ((4.25, -8.25, 30.1, 0.1), 0), origin
    # held on the odd grid: 31 <= cell < 127 - 31 = 96 in x, 31 <= cell < 64 - 31 = 33 in y.  Origin (0, -8): ego (10.3, -0.3) ->
    # cells (41, 30.8 -> 30): re-centred; ego (10.3, -0.2) and goal (20, 0.2) -> cells (41, 31) and (80, 32): held
    out, f = adv(cfg, gf, (0.0, -8.0), (1.0, 1.0), _still(dm, (10.3, -0.2), (20.0, 0.2)))
    assert (_frame(out), f) == ((0.0, -8.0, 20.0, 0.2), 0)
    # ... and far off the frame with no flag: there is no OFF_GRID test without the grid stage
    out, f = adv(cfg, gf, FAR, (1.0, 1.0), _still(dm, (0.0, 0.0), (500.0, 0.0)))
    assert (_frame(out), f) == (((1000.0 - 63.0) * 0.25, -8.0, 500.0, 0.0), 0)


KATS = [_kat_mixed_block, _kat_hold_against_recentre, _kat_skipped_goal_takes_the_old_test, _kat_goal_points, _kat_bad_path_and_path_end,
        _kat_small_grid_off_the_new_frame, _kat_no_grid_stage]


def _kat_routed_transitions(dm, adv):
    """A routed ego making 0 -> 1 and one making 2 -> 0 (the known answers of tests/test_route.py) with following on, goal point 20
    = 10 m along the 0.5 m path: the route fields and the frame are both right."""
    cfg, gf = _cfg(dm), _gf(dm, goal_point=20)
    m = _tiny_map(dm)
    # 0 -> 1: from 118.5 the ego lands on 119.5 = lane point 39.  Frame (100, -16): ego cell 78, goal 128.5 -> cell 114 >= 96:
    # re-centred.  x: 248 / 2 = 124 -> 496 - 64 = 432 cells = 108.0; y: -16.0.  Ego cell (46, 64): on the grid
    out, f = adv(cfg, gf, (100.0, -16.0), (1.0, 1.0), _path(dm, 118.5), v=36.0)
    assert (int(out["loc"]["pos"]), int(out["loc"]["id"][1]), f) == (1, 39, 0)
    assert tuple(int(out["loc"][k]) for k in ("last_roadnum", "next_roadnum", "last_lanenum", "next_lanenum")) == (1, 2, 2, 1)
    assert (int(out["ref_off"]), int(out["ref_n"])) == (0, 10)
    assert _frame(out) == (108.0, -16.0, 128.5, 0.0)
    # 2 -> 0: in the junction at polyline id 6, from 154.6 the ego lands on 155.6: the polyline's last point -> pos 0 on leg 1.
    # Goal P[20] = 154.6 + 10 = 164.6; x: (155.6 + 164.6) / 2 = 160.1 -> 640.4 -> 640 - 64 = 576 cells = 144.0; ego cell 46
    si = _ego(dm, m, pos=2, road=2, lane=1, ego_id=0, four=(1, 2, 2, 1), v=36.0)
    si["loc"]["id"][0, 1] = 6
    po = _path(dm, 154.6)
    out, f = adv(cfg, gf, FAR, (1.0, 1.0), po, si=si)
    assert (int(out["loc"]["pos"]), int(out["loc"]["path_num"]), f) == (0, 1, 0)
    assert out["loc"]["id"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert (int(out["stub_attribute"]), out["out_lane_no"].tolist()) == (2, [1, 0, 0, 0, 0, 0, 0, 0])
    assert _frame(out) == (144.0, -16.0, 164.6, 0.0) and out["goal"].tobytes() == po["road_points"][0, 20].tobytes()


def test_abi_mirror_and_default_model(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(25) == dm.GridFollow.itemsize == 8
    gf = dm.default_grid_follow()
    assert (int(gf["goal_point"][0]), int(gf["margin_cells"][0])) == (199, 32)
    assert gfm.OFF_GRID == dm.EGO_OFF_GRID


@pytest.mark.parametrize("kind", ["egos", "route"])
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, kat, kind):
    kat(dm, _Adv(dm, "model", kind))


def test_kat_routed_transitions_on_the_model(dm):
    _kat_routed_transitions(dm, _Adv(dm, "model", "route"))


def test_kat_smallest_grid_on_the_model(dm):
    """16 x 16 cells (4 m), the goal 10 m ahead: x: 5 -> 20 - 8 = 12 cells = 3.0; y: 0 - 8 cells = -2.0; the ego at (0, 0) is in cell
    (-12, 8): OFF_GRID.  On the model only: the grid stage of the device takes multiples of 32 cells, so the device runs this known
    answer on 32 x 32 cells (_kat_small_grid_off_the_new_frame)."""
    cfg, gf = _cfg(dm, 16), _gf(dm, margin=4)
    for kind in ("egos", "route"):
        out, f = _Adv(dm, "model", kind)(cfg, gf, (-2.0, -2.0), (1.0, 1.0), _still(dm, (0.0, 0.0), (10.0, 0.0)))
        assert (_frame(out), f) == ((3.0, -2.0, 10.0, 0.0), em.OFF_GRID)


def test_model_with_following_off_is_the_wrapped_model(dm):
    cfg, model = _cfg(dm), dm.default_ego_model()
    st, flags = np.zeros(1, dm.SceneState), np.zeros(1, np.int32)
    for v, po in ((0.0, _still(dm, (40.0, 12.0), (50.0, 12.0))), (36.0, _path(dm, 118.5))):
        si, world, _ = _Adv(dm, "model", "egos").scene(cfg, v)
        want = em.advance(cfg, model, si, po, st, flags, world["lane_pool"], False)
        got = gfm.advance(dm, cfg, model, None, si, po, st, flags, lane_pool=world["lane_pool"])
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and int(want[1][0]) == em.OFF_GRID
        si, world, (legs, rf, _) = _Adv(dm, "model", "route").scene(cfg, v)
        rm = dm.default_route_model()
        want = rmod.advance(dm, cfg, model, rm, legs, rf, world["map"], si, po, st, flags)
        got = gfm.advance(dm, cfg, model, None, si, po, st, flags, route=(rm, legs, rf, world["map"]))
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


@gpu
@pytest.mark.parametrize("kind", ["egos", "route"])
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, kat, kind):
    """The known answers on k_advance_egos / k_advance_route (injected PlanOut / SceneState), each step also held against the model."""
    kat(dm, _Adv(dm, "device", kind))


@gpu
def test_kat_routed_transitions_on_the_device(dm):
    _kat_routed_transitions(dm, _Adv(dm, "device", "route"))


@gpu
@pytest.mark.parametrize("kind", ["egos", "route"])
def test_kat_batch_equals_each_case_alone(dm, kind):
    """Every known answer once more on the device, logged, then as distinct scenes of one launch per group of calls that can share
    one (same configuration, GridFollow model, number of steps): at least five scenes, never a multiple of four, and the first block
    of the two-step group holds a held, a re-centred, a skipped and a frozen scene.  Every scene gives the bytes it gave alone."""
    log = []
    a = _Adv(dm, "device", kind, log)
    for kat in KATS + ([_kat_routed_transitions] if kind == "route" else []):
        kat(dm, a)
    first = log[:4]
    assert all(len(c["steps"]) == 2 and c["cfg"].tobytes() == first[0]["cfg"].tobytes() and c["gf"].tobytes() == first[0]["gf"].tobytes() for c in first)
    origin = [[r.out["grid_origin"][0].tobytes() for r in c["res"]] for c in first]
    assert [o[0] == c["si"]["grid_origin"][0].tobytes() for o, c in zip(origin, first)] == [True, False, True, False]      # held, re-centred, skipped, re-centred
    assert [int(c["res"][0].flags[0]) for c in first] == [0, 0, 0, em.OFF_GRID]                                           # ... which the second step finds frozen
    sizes = gb.batched(log)
    print(f"{len(log)} calls in batches of {sizes}")
    assert sum(sizes) >= len(log) and all(n % 4 != 0 and n > 4 for n in sizes)


# ---------------------------------------------------------------------------------------------------------------
# the ring: 16 routed egos, the grid stage on, 256 x 256 cells, the default model
E2E_N, E2E_TICKS = 16, 300
_CPU = {}


def _e2e_scene(dm):
    """The egos of tests/test_route.py's ring run, 150 .. 200 points into their first road (260 points) with routes of 2 .. 4 legs: at
    0.28 m per tick the slowest leaves its first junction (40 points behind the lane) after about 280 ticks.  A grid of 64 m; the
    planned path ends 32 .. 44 m ahead of the ego, so the midpoint frame keeps both at most 22 m from its centre."""
    cfg = dm.default_config(256)
    assert int(cfg["grid_stage"][0]) == 1
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, E2E_N, seed=3, lanes=(1, 2), ids=(150, 200), legs=(2, 4))
    return cfg, m, sc, legs, rf


def _cpu_loop(dm, oracle, follow):
    if follow in _CPU:
        return _CPU[follow]
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    model, rm, gf = dm.default_ego_model(), dm.default_route_model(), dm.default_grid_follow() if follow else None
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(E2E_N, np.int32)
    status, moved = np.zeros(8, np.int64), 0
    for t in range(E2E_TICKS):
        plan, gout, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, mot_pool=None), st, n_threads=8, want_grid=True)
        status += np.bincount(np.clip(gout["status"], 0, 7), minlength=8)
        new, flags, _ = gfm.advance(dm, cfg, model, gf, si, plan, st, flags, route=(rm, legs, rf, m))
        moved += int((new["grid_origin"].tobytes() != si["grid_origin"].tobytes()))
        si = new
    _CPU[follow] = dict(si=si, flags=flags, status=status, moved=moved)
    return _CPU[follow]


def test_ring_closed_loop_on_the_cpu(dm, oracle):
    """Oracle tick + models, 300 ticks with the grid stage on.  Following on: every ego crosses a junction, none carries OFF_GRID (or
    any other flag), and every tick's search found its goal.  Following off: every ego is frozen with OFF_GRID on its first road."""
    on, off = _cpu_loop(dm, oracle, True), _cpu_loop(dm, oracle, False)
    print("on: legs", on["si"]["loc"]["path_num"].tolist(), "flags", on["flags"].tolist(), "status", on["status"].tolist(), "ticks that moved a frame", on["moved"])
    print("off: legs", off["si"]["loc"]["path_num"].tolist(), "flags", off["flags"].tolist())
    assert (on["si"]["loc"]["path_num"] >= 1).all() and (on["si"]["loc"]["pos"] == 0).all()
    assert not on["flags"].any()
    assert on["status"][dm.G_FOUND] == E2E_N * E2E_TICKS and on["moved"] > 0
    assert (off["flags"] == em.OFF_GRID).all() and (off["si"]["loc"]["path_num"] == 0).all()


def _ring_planner(dm, follow):
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    pl = _planner(dm, cfg, m, sc)
    pl.set_route(legs, rf)
    if follow:
        pl.set_grid_follow(dm.default_grid_follow())
    return pl, (cfg, m, sc, legs, rf)


@gpu
def test_ring_without_following_freezes_every_ego(dm):
    """The run of the closed loop below on a handle that never set following: every ego leaves its grid on its first road."""
    pl, _ = _ring_planner(dm, False)
    pl.rollout(E2E_TICKS)
    pl.sync()
    flags, last = pl.ego_flags(), pl.get_scene_in()["loc"]
    pl.close()
    assert (flags == em.OFF_GRID).all() and (last["path_num"] == 0).all()


@gpu
def test_ring_closed_loop_with_following(dm, oracle):
    """16 ring egos, the grid stage on, following on, 300 ticks: no ego carries OFF_GRID at the end and every one crossed a junction
    (the run that freezes all of them without following: above, and on the parent).  On every tick the staged records equal the model
    applied to the device's own records of the tick before, byte for byte (the heading within 1e-6 degrees, as in test_route.py), and
    the tick's GridOut equals the oracle's on the device's own SceneIn within the tolerances of parity_util."""
    pl, (cfg, m, sc, legs, rf) = _ring_planner(dm, True)
    model, rm, gf = dm.default_ego_model(), dm.default_route_model(), dm.default_grid_follow()
    n = E2E_N
    plan_p, grid_p = dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut)
    sin, flags, n_dir, moved, state = pl.get_scene_in(), np.zeros(n, np.int32), 0, 0, sc["state"].copy()
    for t in range(E2E_TICKS):
        st_o = state.copy()                                    # the state the tick starts from
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p, grid_p)) == 0
        plan, gout, state = np.array(plan_p), np.array(grid_p), pl.get_state()
        _, gout_o, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=sin, mot_pool=None), st_o, n_threads=8, want_grid=True)
        bad = compare(gout, gout_o, "grid")
        assert not bad, f"tick {t}\n" + "\n".join(bad[:10])
        pl.advance_async(model)
        got, gflags = pl.get_scene_in(), pl.ego_flags()
        want, wflags, _ = gfm.advance(dm, cfg, model, gf, sin, plan, state, flags, route=(rm, legs, rf, m))
        assert np.array_equal(gflags, wflags), f"tick {t}: flags {gflags.tolist()} against {wflags.tolist()}"
        n_dir += _assert_records(got, want, f"tick {t}")
        moved += int(got["grid_origin"].tobytes() != sin["grid_origin"].tobytes())
        sin, flags = got, gflags
    pl.close()
    print(f"legs {sin['loc']['path_num'].tolist()}, flags {flags.tolist()}, ticks that moved a frame {moved}, dir words that differ {n_dir}")
    assert not (flags & em.OFF_GRID).any() and not flags.any()
    assert (sin["loc"]["path_num"] >= 1).all() and moved > 0


@gpu
def test_rollout_scorecard_counts_every_grid_tick(dm):
    """A short pp_rollout with the scorecard and following on: every scored tick ran the grid stage on a frame the ego was on."""
    pl, _ = _ring_planner(dm, True)
    pl.score_begin()
    pl.rollout(40)
    pl.sync()
    score, flags = pl.rollout_score(), pl.ego_flags()
    pl.close()
    assert (score["n_ticks"] == 41).all() and np.array_equal(score["n_grid_ticks"], score["n_ticks"])
    assert not flags.any() and (score["ego_flags"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# off, and the error paths
@gpu
def test_following_off_is_the_engine_without_it(dm):
    """Three handles, a few advances of the ring egos with the grid stage on: one that never set following, one that set it and
    switched it off with NULL, one that set it, called pp_set_egos and then switched it off - staged records, flags and traces to the
    byte.  (A fourth that leaves it ON across pp_set_egos differs: the model survives pp_set_egos.)"""
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    K, outs = 12, []
    for mode in ("never", "off", "egos_off", "egos_on"):
        pl = _planner(dm, cfg, m, sc)
        if mode != "never":
            pl.set_grid_follow(dm.default_grid_follow())
        if mode.startswith("egos"):
            pl.set_egos(sc, with_motion=False)
            pl.set_state(sc["state"])
        if mode in ("off", "egos_off"):
            pl.set_grid_follow(None)
        pl.set_route(legs, rf)
        _, trace = pl.rollout(K, trace=True)
        pl.sync()
        outs.append((pl.get_scene_in(), pl.ego_flags(), np.array(trace), pl.get_plan(), pl.get_grid_out()))
        pl.close()
    for other in outs[1:3]:
        for a, b, name in zip(outs[0], other, ("SceneIn", "flags", "trace", "PlanOut", "GridOut")):
            assert a.tobytes() == b.tobytes(), name
    assert outs[0][0]["grid_origin"].tobytes() == ms.resolve(dm, m, sc["scene_in"])["grid_origin"].tobytes()       # carried over, as ever
    assert outs[3][0]["goal"].tobytes() != outs[0][0]["goal"].tobytes()                                             # the model survived pp_set_egos


@gpu
def test_bad_arguments_leave_the_model_as_it_was(dm):
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    good = _gf(dm, goal_point=150, margin=40)
    ref = _planner(dm, cfg, m, sc)
    ref.set_grid_follow(good)
    pl = _planner(dm, cfg, m, sc)
    pl.set_grid_follow(good)
    for gp, mg in ((0, 32), (200, 32), (-1, 32), (199, -1), (199, 128), (199, 1 << 30)):          # 2 * 128 = 256 is not < 256
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_grid_follow(_gf(dm, gp, mg))
    pl.set_grid_follow(_gf(dm, 199, 127))                                                          # 254 < 256: the largest margin
    pl.set_grid_follow(good)
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_grid_follow(_gf(dm, 0, 0))
    small = cfg.copy()
    small["grid_w"], small["grid_h"] = 64, 64                                                      # 2 * 40 >= 64: the margin no longer fits
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_config(small)
    outs = []
    for p in (pl, ref):
        p.set_route(legs, rf)
        p.rollout(8)
        p.sync()
        outs.append((p.get_scene_in(), p.ego_flags()))
        p.close()
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][0]["goal"].tobytes() != ms.resolve(dm, m, sc["scene_in"])["goal"].tobytes()     # ... and it is still on
