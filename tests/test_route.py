"""Route following (pp_set_route): rollout egos cross junctions onto the next road of their route.

CPU: the ABI mirrors, hand-derived known answers of the numpy model (tests/route_model.py) with their arithmetic, and a closed
loop of oracle tick + model on the ring of tests/route_scenes.py.
GPU: the device against the model step by step on its own records (bytes), pp_rollout against its parts, a fresh upload of the
final records, routing switched off, the error paths, a fleet and the scorecard on routed egos, and the closed loop against
the CPU loop."""
import numpy as np
import pytest

import advance_backends as ab
import ego_model as em
import map_scenes as ms
import route_model as rmod
import route_scenes as rs
from parity_util import compare

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
    assert lib.pp_sizeof(23) == dm.RouteLeg.itemsize == 24
    assert lib.pp_sizeof(24) == dm.RouteModel.itemsize == 8
    assert int(dm.default_route_model()["pre_points"][0]) == 60
    assert rmod.ROUTE_END == dm.EGO_ROUTE_END == 16 and rmod.LANE_END == dm.EGO_LANE_END


# A map small enough to do by hand.  Road 1: two lanes of 100 points, x = 100 + 0.5 k (k = 0 .. 99, the last point at 149.5),
# lane 1 at y = 3.75, lane 2 at y = 0.  Road 2: one lane of 100 points, x = 155 + 0.5 k, y = 0.  One junction, from lane 2 of road 1
# to lane 1 of road 2: 10 points, x = 150 + 0.5 k (k = 0 .. 9, the last at 154.5), y = 0.  Lane 1 of road 1 has no junction.
def _tiny_map(dm):
    pts = np.zeros(300, dm.GlobalPoint3D)
    pts["x"][:100], pts["y"][:100] = 100.0 + 0.5 * np.arange(100), 3.75
    pts["x"][100:200], pts["y"][100:200] = 100.0 + 0.5 * np.arange(100), 0.0
    pts["x"][200:], pts["y"][200:] = 155.0 + 0.5 * np.arange(100), 0.0
    jp = np.zeros(10, dm.GlobalPoint2D)
    jp["x"] = 150.0 + 0.5 * np.arange(10)
    return dict(road_first_lane=np.array([0, 2, 3], np.int32),
                lanes=np.array([(0, 100, 2, 0), (100, 100, 2, 0), (200, 100, 1, 0)], dm.MapLane),
                points=pts, lanechg_attribute=np.zeros(300, np.uint8), lane_width_cm=np.full(300, 375, np.uint16),
                junctions=np.array([(1, 2, 2, 1, 0, 10)], dm.MapJunction), jpoints=jp)


def _legs(dm, n=2):
    legs = np.zeros(2, dm.RouteLeg)
    legs["road_num"] = [1, 2]
    legs["stub_attribute"] = [1, 2]
    legs["out_lane_no"][0, :1] = [2]
    legs["out_lane_no"][1, :1] = [1]
    return legs[:n]


def _ego(dm, m, pos=0, road=1, lane=2, ego_id=30, four=(0, 0, 0, 0), path_num=0, v=36.0):
    si = np.zeros(1, dm.SceneIn)
    loc = si["loc"]
    loc["pos"], loc["road_num"], loc["lane_num"], loc["path_num"], loc["velocity"] = pos, road, lane, path_num, v
    loc["last_roadnum"], loc["next_roadnum"], loc["last_lanenum"], loc["next_lanenum"] = four
    loc["id"][:] = ego_id
    loc["globalpoint"]["dir"] = 77.0
    si["stub_attribute"], si["out_lane_no"][0, 0] = 1, 2
    return ms.resolve(dm, m, si)


def _path(dm, x0, y=0.0):
    """A straight 200-point path along +x from x0 at 0.5 m spacing, driven at 36 km/h: the ego goes s = 1 m, to x0 + 1."""
    po = np.zeros(1, dm.PlanOut)
    po["road_points"]["x"][0] = x0 + 0.5 * np.arange(200)
    po["road_points"]["y"][0] = y
    po["result"]["desspd"] = 36.0
    return po


class _Adv:
    """One routed advance of one scene on a backend of tests/advance_backends.py: the known answers below are written once against it."""
    def __init__(self, dm, runner):
        self.dm, self.run, self.name = dm, runner, runner.name

    def steps(self, cfg, m, si, pos, legs, pre_points=60):
        dm = self.dm
        rm = dm.default_route_model()
        rm["pre_points"] = pre_points
        route = None if legs is None else (legs, np.array([0, len(legs)], np.int32), rm)
        res = self.run(cfg, dm.default_ego_model(), si, [(po, np.zeros(1, dm.SceneState)) for po in pos], dict(map=m), route)
        return [(r.out[0], int(r.flags[0])) for r in res]

    def __call__(self, cfg, m, si, po, legs, pre_points=60):
        return self.steps(cfg, m, si, [po], legs, pre_points)[0]


def _runner(name, log=None):
    return ab.Runner(ab.ModelBackend() if name == "model" else ab.DeviceBackend(), log)


def _four(loc):
    return tuple(int(loc[k]) for k in ("last_roadnum", "next_roadnum", "last_lanenum", "next_lanenum"))


def _kat_pre_junction_starts_at_pre_points(dm, cfg0, adv):
    # n_c = 100, pre_points = 60: 0 -> 1 when 99 - id' <= 60, i.e. from id' = 39 (x = 119.5) on.  The ego goes 1 m: from 118.5 it
    # lands on 119.5 = point 39 -> pos 1; from 118.0 on 119.0 = point 38 (99 - 38 = 61 > 60) -> pos 0.  Jn = J(1, 2, lane 2): next_lane 1.
    m = _tiny_map(dm)
    si = _ego(dm, m)
    out, f = adv(cfg0, m, si, _path(dm, 118.5), _legs(dm))
    assert (int(out["loc"]["pos"]), int(out["loc"]["id"][1]), f) == (1, 39, 0)
    assert _four(out["loc"]) == (1, 2, 2, 1)                          # last road, next road (leg 1), last lane, Jn.next_lane
    assert (int(out["loc"]["road_num"]), int(out["loc"]["lane_num"]), int(out["loc"]["path_num"])) == (1, 2, 0)
    assert (int(out["ref_off"]), int(out["ref_n"])) == (0, 10)         # the polyline of the four indices, derived behind the step
    out, f = adv(cfg0, m, si, _path(dm, 118.0), _legs(dm))
    assert (int(out["loc"]["pos"]), int(out["loc"]["id"][1]), f) == (0, 38, 0) and _four(out["loc"]) == (0, 0, 0, 0)
    # pre_points = 61 takes point 38 in; pre_points = 0 only the last point
    assert int(adv(cfg0, m, si, _path(dm, 118.0), _legs(dm), pre_points=61)[0]["loc"]["pos"]) == 1
    assert int(adv(cfg0, m, si, _path(dm, 118.5), _legs(dm), pre_points=0)[0]["loc"]["pos"]) == 0


def _kat_junction_is_entered_on_the_last_lane_point(dm, cfg0, adv):
    # pos 1 on lane 2 of road 1, id 90.  From 149.25 the ego lands on 150.25: the nearest lane point of [90, 100) is the last, 99
    # (149.5) = n_c - 1 -> pos 2, road_num / lane_num = next_roadnum / next_lanenum = 2 / 1, every id 0 except slot
    # last_lanenum - 1 = 1: the nearest polyline point of [0, 10) to 150.25 - 150.0 (0.25 away) and 150.5 (0.25 away) tie, the first wins: 0.
    m = _tiny_map(dm)
    si = _ego(dm, m, pos=1, ego_id=90, four=(1, 2, 2, 1))
    out, f = adv(cfg0, m, si, _path(dm, 149.25), _legs(dm))
    assert float(out["loc"]["globalpoint"]["x"]) == 150.25
    assert (int(out["loc"]["pos"]), int(out["loc"]["road_num"]), int(out["loc"]["lane_num"]), f) == (2, 2, 1, 0)
    assert out["loc"]["id"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0] and _four(out["loc"]) == (1, 2, 2, 1) and int(out["loc"]["path_num"]) == 0
    # from 149.5 it lands on 150.5 = polyline point 1
    out, f = adv(cfg0, m, si, _path(dm, 149.5), _legs(dm))
    assert (int(out["loc"]["pos"]), out["loc"]["id"].tolist(), f) == (2, [0, 1, 0, 0, 0, 0, 0, 0], 0)
    assert (int(out["lanes"]["cur_off"]), int(out["lanes"]["cur_n"])) == (200, 100)        # the views are those of road 2 from here on
    # one point short of the end (from 148.0 to 149.0 = point 98): still pos 1, and no LANE_END although 98 + 32 >= 100 - Jn exists
    out, f = adv(cfg0, m, si, _path(dm, 148.0), _legs(dm))
    assert (int(out["loc"]["pos"]), int(out["loc"]["id"][1]), f) == (1, 98, 0)
    # pos 1 without a polyline (the four indices name no junction): "no Jn" -> LANE_END at the lane end, pos held
    si2 = _ego(dm, m, pos=1, ego_id=90, four=(1, 2, 1, 1))
    out, f = adv(cfg0, m, si2, _path(dm, 149.5), _legs(dm))
    assert (int(out["loc"]["pos"]), int(out["ref_n"]), f) == (1, 0, em.LANE_END)


def _kat_junction_is_left_at_the_end_of_the_polyline(dm, cfg0, adv):
    # pos 2: road 2, lane 1, polyline id in slot last_lanenum - 1 = 1, j = 6; window 32 -> searched [6, 10).  From 154.6 the ego lands
    # on 155.6: nearest polyline point 9 (154.5) = ref_n - 1 -> pos 0, path_num 1, out_lane_no / stub_attribute of leg 1, ids zeroed
    # and the view of lane 1 of road 2 (x = 155 + 0.5 k) searched over [0, 32): 155.5 = point 1 (0.1 away; 156.0 is 0.4 away).
    m = _tiny_map(dm)
    si = _ego(dm, m, pos=2, road=2, lane=1, ego_id=0, four=(1, 2, 2, 1))
    si["loc"]["id"][0, 1] = 6
    out, f = adv(cfg0, m, si, _path(dm, 154.6), _legs(dm))
    assert (int(out["loc"]["pos"]), int(out["loc"]["path_num"]), f) == (0, 1, 0)
    assert out["loc"]["id"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert (int(out["stub_attribute"]), out["out_lane_no"].tolist()) == (2, [1, 0, 0, 0, 0, 0, 0, 0])
    assert (int(out["loc"]["road_num"]), int(out["loc"]["lane_num"])) == (2, 1) and _four(out["loc"]) == (1, 2, 2, 1)
    # from 152.9 it lands on 153.9: polyline point 8 (154.0) < ref_n - 1 -> still in the junction, the leg index has NOT moved
    out, f = adv(cfg0, m, si, _path(dm, 152.9), _legs(dm))
    assert (int(out["loc"]["pos"]), int(out["loc"]["path_num"]), out["loc"]["id"].tolist(), f) == (2, 0, [0, 8, 0, 0, 0, 0, 0, 0], 0)
    assert (int(out["stub_attribute"]), int(out["out_lane_no"][0])) == (1, 2)
    # a junction behind the LAST leg (a caller error): everything is held, ROUTE_END
    out, f = adv(cfg0, m, si, _path(dm, 154.6), _legs(dm, 1))
    assert (int(out["loc"]["pos"]), int(out["loc"]["path_num"]), out["loc"]["id"].tolist(), f) == (2, 0, [0, 9, 0, 0, 0, 0, 0, 0], rmod.ROUTE_END)


def _kat_lane_end_missed_exit_and_arrival(dm, cfg0, adv):
    m = _tiny_map(dm)
    # lane 1 of road 1 has no junction: the ego at id' = 68 (x = 134.0; 68 + 32 >= 100) missed its exit lane -> LANE_END alone
    si = _ego(dm, m, lane=1, ego_id=60)
    out, f = adv(cfg0, m, si, _path(dm, 133.0, y=3.75), _legs(dm))
    assert (int(out["loc"]["pos"]), int(out["loc"]["id"][0]), f) == (0, 68, em.LANE_END)
    # one point before (id' = 67): nothing yet
    assert adv(cfg0, m, si, _path(dm, 132.5, y=3.75), _legs(dm))[1] == 0
    # the same pose on lane 2, which has its junction: no flag, and pos 1 (99 - 68 <= 60)
    si = _ego(dm, m, lane=2, ego_id=60)
    out, f = adv(cfg0, m, si, _path(dm, 133.0), _legs(dm))
    assert (int(out["loc"]["pos"]), f) == (1, 0)
    # the last leg (a route of one leg): LANE_END | ROUTE_END = 4 | 16, the ego arrived
    out, f = adv(cfg0, m, si, _path(dm, 133.0), _legs(dm, 1))
    assert (int(out["loc"]["pos"]), f) == (0, em.LANE_END | rmod.ROUTE_END) and f == 20


def _kat_pre_junction_holds_the_lane_number(dm, cfg0, adv):
    # lane width 3.75 -> margin 0.9375; the ego 2.8 m to the left of lane 2 is 0.95 m from lane 1: 2.8 - 0.95 = 1.85 > 0.9375.
    # On the road (pos 0) the lane number follows (§4c 5.); in the pre-junction it is held - the polyline was chosen by lane
    m = _tiny_map(dm)
    po = _path(dm, 110.0, y=2.8)
    out, f = adv(cfg0, m, _ego(dm, m, pos=0, ego_id=20), po, _legs(dm))
    assert (int(out["loc"]["lane_num"]), int(out["loc"]["pos"]), f) == (1, 0, 0)
    out, f = adv(cfg0, m, _ego(dm, m, pos=1, ego_id=20, four=(1, 2, 2, 1)), po, _legs(dm))
    assert (int(out["loc"]["lane_num"]), int(out["loc"]["pos"]), f) == (2, 1, 0)
    assert out["loc"]["id"].tolist()[:2] == [22, 22]                   # the ids of both views are found all the same (x = 111 = point 22)


def _kat_scenes_without_a_route_take_the_plain_step(dm, cfg0, adv):
    # an unrouted scene, a path_num outside the route, a frozen scene: bytes of ego_model.advance (map mode) + resolve
    m = _tiny_map(dm)
    model = dm.default_ego_model()
    st = np.zeros(1, dm.SceneState)
    for si, legs, flag in ((_ego(dm, m, ego_id=60), None, 0), (_ego(dm, m, ego_id=60, path_num=2), _legs(dm), 0),
                           (_ego(dm, m, ego_id=60, path_num=-1), _legs(dm), 0), (_ego(dm, m, ego_id=60), _legs(dm), em.OFF_GRID)):
        po = _path(dm, 133.0)
        want, wf, _ = em.advance(cfg0, model, si, po, st, np.array([flag], np.int32), m["points"], map_mode=True)
        if flag == 0:
            out, f = adv(cfg0, m, si, po, legs)
        elif adv.name == "model":                                    # the model takes the flag word as it is given
            o, fl, _ = rmod.advance(dm, cfg0, model, dm.default_route_model(), legs, np.array([0, len(legs)], np.int32), m, si, po, st,
                                    np.array([flag], np.int32))
            out, f = o[0], int(fl[0])
        else:
            continue                                                 # (the device reaches a flag by a step of its own: below)
        assert out.tobytes() == ms.resolve(dm, m, want)[0].tobytes() and f == int(wf[0])
        assert f == (flag if flag else em.LANE_END)                  # (§4c: the lane end freezes it)
    # the frozen scene with its flag reached the honest way, on both backends: the grid stage on, a grid of 32 m at the origin
    # (100, 100), far from the road at y = 0 - the routed ego goes from 120 to 121 = point 42 (99 - 42 <= 60: pos 1) and is off the
    # grid; the next step finds OFF_GRID set and is the plain step of a frozen scene: the record as it stands, the flag kept
    cfg = dm.default_config(128)
    si = _ego(dm, m, ego_id=30)
    si["grid_origin"]["x"], si["grid_origin"]["y"], si["goal"]["x"], si["goal"]["y"] = 100.0, 100.0, 116.0, 116.0
    (mid, f0), (out, f) = adv.steps(cfg, m, si, [_path(dm, 120.0), _path(dm, 133.0)], _legs(dm))
    assert (f0, int(mid["loc"]["pos"]), int(mid["loc"]["id"][1]), float(mid["loc"]["globalpoint"]["x"])) == (em.OFF_GRID, 1, 42, 121.0)
    want, wf, _ = em.advance(cfg, model, mid.reshape(1), _path(dm, 133.0), st, np.array([f0], np.int32), m["points"], map_mode=True)
    assert out.tobytes() == ms.resolve(dm, m, want)[0].tobytes() == mid.tobytes() and f == int(wf[0]) == em.OFF_GRID


KATS = [_kat_pre_junction_starts_at_pre_points, _kat_junction_is_entered_on_the_last_lane_point, _kat_junction_is_left_at_the_end_of_the_polyline, _kat_lane_end_missed_exit_and_arrival, _kat_pre_junction_holds_the_lane_number, _kat_scenes_without_a_route_take_the_plain_step]


def test_kat_pre_junction_starts_at_pre_points(dm, cfg0):
    _kat_pre_junction_starts_at_pre_points(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_junction_is_entered_on_the_last_lane_point(dm, cfg0):
    _kat_junction_is_entered_on_the_last_lane_point(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_junction_is_left_at_the_end_of_the_polyline(dm, cfg0):
    _kat_junction_is_left_at_the_end_of_the_polyline(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_lane_end_missed_exit_and_arrival(dm, cfg0):
    _kat_lane_end_missed_exit_and_arrival(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_pre_junction_holds_the_lane_number(dm, cfg0):
    _kat_pre_junction_holds_the_lane_number(dm, cfg0, _Adv(dm, _runner("model")))


def test_kat_scenes_without_a_route_take_the_plain_step(dm, cfg0):
    _kat_scenes_without_a_route_take_the_plain_step(dm, cfg0, _Adv(dm, _runner("model")))


@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg0, kat):
    """The known answers above on k_advance_route / k_advance_egos (injected PlanOut / SceneState), each also held against the model."""
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


# ---- the ring ------------------------------------------------------------------------------------------------
E2E_N, E2E_TICKS = 16, 950
_CPU = {}


def _e2e_scene(dm):
    """16 obstacle-free egos on lanes 1 / 2 of the ring, 120 .. 170 points into their first road, routes of 6 .. 10 legs.  The
    planner drives an obstacle-free ring at 10 km/h (0.28 m = 0.56 points per tick): the slowest start needs about 870 ticks to
    leave its second junction, the fastest is then 50 points further - 950 ticks leave every ego on the open road of its third leg."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, E2E_N, seed=3, lanes=(1, 2), ids=(120, 170), legs=(6, 10))
    return cfg, m, sc, legs, rf


def _cpu_loop(dm, oracle):
    if _CPU:
        return _CPU
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    model, rm = dm.default_ego_model(), dm.default_route_model()
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(E2E_N, np.int32)
    sins, poss = [si], [si["loc"]["pos"].copy()]
    for t in range(E2E_TICKS):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, mot_pool=None), st, n_threads=8, want_grid=False)
        si, flags, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
        sins.append(si), poss.append(si["loc"]["pos"].copy())
    _CPU.update(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, sins=sins, flags=flags, pos=np.array(poss))
    return _CPU


def test_ring_closed_loop_on_the_cpu(dm, oracle):
    """Oracle tick + model, 950 ticks: every ego crosses at least two junctions and is back on the road with no flag other than
    ROUTE_END; on the way every ego was in the pre-junction and in the junction, and the ring is the gentle one it claims to be."""
    r = _cpu_loop(dm, oracle)
    m, last = r["m"], r["sins"][-1]["loc"]
    print("legs", last["path_num"].tolist(), "pos", last["pos"].tolist(), "flags", r["flags"].tolist(), "lanes", last["lane_num"].tolist(),
          "road", last["road_num"].tolist())
    assert (last["path_num"] >= 2).all()                               # two junctions crossed: path_num moves when a junction is left
    assert (last["pos"] == 0).all()
    assert ((r["flags"] & ~rmod.ROUTE_END) == 0).all()
    for k in range(E2E_N):
        seq = r["pos"][:, k]
        changes = seq[np.flatnonzero(np.diff(seq, prepend=seq[0] - 1))].tolist()
        assert changes[:7] == [0, 1, 2, 0, 1, 2, 0], (k, changes)
    want_road = (r["sins"][0]["loc"]["road_num"] - 1 + last["path_num"]) % 4 + 1
    assert np.array_equal(last["road_num"], want_road)
    assert np.array_equal(r["legs"]["road_num"][r["rf"][:-1] + last["path_num"]], last["road_num"])
    # the generator's promises: 4 roads of 2 - 3 lanes and 260 points, 40-point polylines at about 0.5 m, at most 30 degrees per junction
    assert len(m["road_first_lane"]) == 5 and set(np.diff(m["road_first_lane"]).tolist()) == {2, 3} and (m["lanes"]["n_points"] == 260).all()
    for q in m["junctions"]:
        j = m["jpoints"][int(q["point_off"]):int(q["point_off"]) + int(q["n_points"])]
        step = np.hypot(np.diff(j["x"]), np.diff(j["y"]))
        assert len(j) == 40 and 0.45 < step.min() and step.max() < 0.55
        a = m["points"][int(m["lanes"][m["road_first_lane"][q["last_road"] - 1] + q["last_lane"] - 1]["point_off"]) + 259]["dir"]
        b = m["points"][int(m["lanes"][m["road_first_lane"][q["next_road"] - 1] + q["next_lane"] - 1]["point_off"])]["dir"]
        assert (b - a) % 360.0 <= 30.0


# ---------------------------------------------------------------------------------------------------------------
# GPU
STEP_N, STEP_TICKS = 256, 220
_RUNS = {}


def _assert_records(got, want, what):
    """Every byte of the records but the heading must be equal.  loc.globalpoint.dir is GetRoadAngle of §4c 3. - an `atan`, which the
    device's and the host's maths libraries round differently in the last bit (§4c: "`atan` aside") - and is held to the bound
    tests/test_rollout.py sets for it, 1e-6 degrees.  Returns the number of headings that are not bit-equal."""
    g, w = got.copy(), want.copy()
    g["loc"]["globalpoint"]["dir"], w["loc"]["globalpoint"]["dir"] = 0.0, 0.0
    bad = compare(g, w, "scene_in", rtol=0.0, atol=0.0)
    assert not bad, what + "\n" + "\n".join(bad[:10])
    assert g.tobytes() == w.tobytes(), what + ": SceneIn bytes"
    dd = np.abs(got["loc"]["globalpoint"]["dir"] - want["loc"]["globalpoint"]["dir"])
    assert np.minimum(dd, 360.0 - dd).max() <= 1e-6, what + ": dir"
    return int((got["loc"]["globalpoint"]["dir"] != want["loc"]["globalpoint"]["dir"]).sum())


def _planner(dm, cfg, m, sc, n_obs=0, slack=0):
    pl = dm.Planner(cfg, device=0, **rs.caps(m, len(sc["scene_in"]), n_obs, slack))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    return pl


def _step_scene(dm):
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, STEP_N, seed=17, legs=(2, 6), mixed=True)
    rf = rf.copy()
    legs = np.concatenate([legs[:rf[5]], legs[rf[6]:]])                # scene 5 gets no route at all
    rf[6:] -= rf[6] - rf[5]
    sc["scene_in"]["loc"]["path_num"][9] = 40                           # scene 9 a leg index outside its route
    return cfg, m, sc, legs, rf


def _closed_loop(dm):
    """220 ticks of advance + tick with pp_get_scene_in and pp_get_ego_flags after every advance, on 256 egos that start in every
    position of the ring."""
    if "step" in _RUNS:
        return _RUNS["step"]
    cfg, m, sc, legs, rf = _step_scene(dm)
    n = STEP_N
    pl = _planner(dm, cfg, m, sc)
    model, rm = dm.default_ego_model(), dm.default_route_model()
    pl.set_route(legs, rf, rm)
    assert pl.get_scene_in().tobytes() == ms.resolve(dm, m, sc["scene_in"]).tobytes()        # pp_set_route leaves the resident records alone
    plan_p = dm.pinned_empty(n, dm.PlanOut)
    run = dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, n=n, model=model, rm=rm, sin=[pl.get_scene_in()], plan=[], state=[], flags=[np.zeros(n, np.int32)])
    for t in range(STEP_TICKS):
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        run["plan"].append(np.array(plan_p)), run["state"].append(pl.get_state())
        pl.advance_async(model)
        run["sin"].append(pl.get_scene_in()), run["flags"].append(pl.ego_flags())
    pl.tick()
    pl.sync()
    run["last"] = (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in())
    pl.close()
    _RUNS["step"] = run
    return run


@gpu
def test_step_check_against_the_model(dm):
    """The primary criterion: for 220 ticks on 256 ring egos the model applied to the device's own SceneIn_t, PlanOut_t, SceneState_t
    and flags gives the staged SceneIn_{t+1} and the flag words byte for byte - no scene and no tick left out, no tolerance on
    anything §4f specifies.  The one field that is not bit-equal is the heading of §4c 3. (_assert_records): measured on the device,
    5 of the 256 headings of the first advance differ from the host's `atan` in the last bit (46.846632226929856 against 46.84663222692985)."""
    r = _closed_loop(dm)
    n, trans, n_dir = r["n"], np.zeros((3, 3), np.int64), 0
    for t in range(STEP_TICKS):
        want, wflags, _ = rmod.advance(dm, r["cfg"], r["model"], r["rm"], r["legs"], r["rf"], r["m"], r["sin"][t], r["plan"][t], r["state"][t], r["flags"][t])
        got = r["sin"][t + 1]
        assert np.array_equal(r["flags"][t + 1], wflags), f"tick {t}: flags {np.flatnonzero(r['flags'][t + 1] != wflags).tolist()}"
        n_dir += _assert_records(got, want, f"tick {t}")
        np.add.at(trans, (np.clip(r["sin"][t]["loc"]["pos"], 0, 2), np.clip(got["loc"]["pos"], 0, 2)), 1)
    fl = r["flags"][-1]
    print(f"transitions (rows: from pos, columns: to pos):\n{trans}\nflags at the end: {np.bincount(fl, minlength=32).tolist()}, dir words that differ: {n_dir}")
    assert trans[0, 1] > 20 and trans[1, 2] > 20 and trans[2, 0] > 20                     # every transition is exercised ...
    assert (fl == em.LANE_END).any() and (fl == (em.LANE_END | rmod.ROUTE_END)).any() and (fl == 0).any()      # ... and both ends
    assert not (fl & ~(em.LANE_END | rmod.ROUTE_END)).any()
    assert trans[0, 2] == 0 and trans[1, 0] == 0 and trans[2, 1] == 0                      # at most one transition per advance, in order
    assert int(r["sin"][-1]["loc"]["path_num"][9]) == 40 and int(r["flags"][-1][5]) in (0, em.LANE_END)


@gpu
def test_rollout_with_a_route_equals_its_parts(dm):
    """pp_rollout(220) on a routed handle = 220 x (advance, tick) with read-backs in between, bit for bit; the trace is the staged records."""
    r = _closed_loop(dm)
    pl = _planner(dm, r["cfg"], r["m"], r["sc"])
    pl.set_route(r["legs"], r["rf"], r["rm"])
    last, trace = pl.rollout(STEP_TICKS, r["model"], trace=True)
    pl.sync()
    assert last == STEP_TICKS + 1
    got = (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in())
    for a, b, name in zip(got, r["last"], ("PlanOut", "SceneState", "flags", "SceneIn")):
        assert a.tobytes() == b.tobytes(), name
    trace = np.array(trace)
    for t in range(STEP_TICKS):
        loc = r["sin"][t + 1]["loc"]
        assert trace[t]["pose"].tobytes() == loc["globalpoint"].tobytes() and np.array_equal(trace[t]["lane_num"], loc["lane_num"])
        assert np.array_equal(trace[t]["id_cur"], loc["id"][np.arange(r["n"]), np.clip(loc["lane_num"] - 1, 0, 7)])
        assert np.array_equal(trace[t]["flags"], r["flags"][t + 1])
    # a fresh pp_set_egos of the final records (views cleared) reproduces them: the records are what the map gives at these indices
    raw = r["last"][3].copy()
    raw["lanes"] = 0
    raw["ref_off"], raw["ref_n"] = 0, 0
    pl.set_egos(dict(r["sc"], scene_in=raw), with_motion=False)
    assert pl.get_scene_in().tobytes() == r["last"][3].tobytes()
    pl.close()


@gpu
def test_route_off_is_the_engine_without_one(dm):
    """n_legs_total = 0 and a new pp_set_egos: the handle then runs §4c byte for byte like a handle that never had a route."""
    cfg, m, sc, legs, rf = _step_scene(dm)
    K, outs = 40, []
    for routed_before in (True, False):
        pl = _planner(dm, cfg, m, sc)
        if routed_before:
            pl.set_route(legs, rf)
            pl.rollout(30)
            pl.set_route(None)
            pl.set_egos(sc, with_motion=False)
            pl.set_state(sc["state"])
        _, trace = pl.rollout(K, trace=True)
        pl.sync()
        outs.append((pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), np.array(trace)))
        pl.close()
    for a, b, name in zip(outs[0], outs[1], ("PlanOut", "SceneState", "flags", "SceneIn", "trace")):
        assert a.tobytes() == b.tobytes(), name
    assert (outs[0][3]["loc"]["pos"] == sc["scene_in"]["loc"]["pos"]).all()                 # nobody moved on: §4c
    assert (outs[1][2] & em.LANE_END).any() and not (outs[1][2] & rmod.ROUTE_END).any()
    # pp_set_egos alone switches it off as well
    pl = _planner(dm, cfg, m, sc)
    pl.set_route(legs, rf)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.rollout(K)
    pl.sync()
    assert pl.get_scene_in().tobytes() == outs[1][3].tobytes() and pl.ego_flags().tobytes() == outs[1][2].tobytes()
    pl.close()


@gpu
def test_errors_leave_the_route_as_it_was(dm):
    cfg, m, sc, legs, rf = _step_scene(dm)
    n = STEP_N
    # slice-mode scenes: PP_ERR_STATE
    gen = dm.gen_scenes(cfg, 0, 8, 4, junction_every=0)
    pl = dm.Planner(cfg, device=0, max_scenes=8, max_obs_total=32)
    with pytest.raises(dm.PlannerError, match="error -4:"):                   # no resident scenes
        pl.set_route(legs[:8], np.arange(9, dtype=np.int32))
    pl.set_scenes(gen, with_motion=False)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_route(legs[:8], np.arange(9, dtype=np.int32))
    pl.close()
    pl = _planner(dm, cfg, m, sc)
    pl.set_route(legs, rf)
    bad = rf.copy()
    bad[0] = 1
    with pytest.raises(dm.PlannerError, match="error -1:"):                   # PP_ERR_ARG: does not start at 0
        pl.set_route(legs, bad)
    bad = rf.copy()
    bad[-1] -= 1
    with pytest.raises(dm.PlannerError, match="error -1:"):                   # does not end at n_legs_total
        pl.set_route(legs, bad)
    bad = rf.copy()
    bad[3], bad[4] = rf[4], rf[3]
    assert bad[4] < bad[3]
    with pytest.raises(dm.PlannerError, match="error -1:"):                   # decreases
        pl.set_route(legs, bad)
    far = legs.copy()
    far["road_num"][7] = 5
    with pytest.raises(dm.PlannerError, match="error -1:"):                   # a road outside the map
        pl.set_route(far, rf)
    far["road_num"][7] = 0
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_route(far, rf)
    neg = dm.default_route_model()
    neg["pre_points"] = -1
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_route(legs, rf, neg)
    pl.tick()
    pl.advance_async()
    with pytest.raises(dm.PlannerError, match="error -4:"):                   # an update is staged
        pl.set_route(legs, rf)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_route(None)
    # none of it changed the route: the run goes on like the reference run
    r = _closed_loop(dm)
    assert pl.get_scene_in().tobytes() == r["sin"][1].tobytes()
    pl.tick()
    pl.rollout(STEP_TICKS - 1)
    pl.sync()
    assert pl.get_scene_in().tobytes() == r["last"][3].tobytes() and pl.ego_flags().tobytes() == r["last"][2].tobytes()
    pl.close()


@gpu
def test_fleet_and_scorecard_on_routed_egos(dm):
    """With a fleet set the peers are coupled at the ROUTED poses - fleet_model on the model's staged set gives the device's
    records and slices - and the scorecard's ego_flags carries ROUTE_END."""
    import fleet_model as fl
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    n, K, ticks = 128, 4, 60
    sc, legs, rf = rs.make_egos(dm, cfg, m, n, seed=23, legs=(1, 3), mixed=True, n_obs=K)
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"] = 12.0, K
    worlds = [0, 1, 40, n]
    pl = _planner(dm, cfg, m, sc, n_obs=K)
    pl.set_fleet(worlds, fm)
    pl.set_route(legs, rf)
    pl.score_begin()
    model, rm = dm.default_ego_model(), dm.default_route_model()
    off, own = sc["scene_in"]["obs_off"].copy(), sc["scene_in"]["obs_n"].copy()
    plan_p = dm.pinned_empty(n, dm.PlanOut)
    sin, flags, pool, peers = pl.get_scene_in(), np.zeros(n, np.int32), sc["obs_pool"].copy(), 0
    for t in range(ticks):
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        plan, state = np.array(plan_p), pl.get_state()
        pl.advance_async(model)
        got, gflags = pl.get_scene_in(), pl.ego_flags()
        routed, wflags, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, sin, plan, state, flags)
        want, wpool, _ = fl.couple(fm, worlds, off, own, routed, pool)
        assert np.array_equal(gflags, wflags), f"tick {t}: flags"
        _assert_records(got, want, f"tick {t}")
        for s in range(0, n, 5):
            a, c = int(want["obs_off"][s]), int(want["obs_n"][s])
            assert pl.get_obstacles(s).tobytes() == wpool[a:a + c].tobytes(), f"tick {t}, scene {s}: slice"
        peers += int(got["obs_n"].sum())
        sin, flags, pool = got, gflags, wpool
    pl.tick()
    score = pl.rollout_score()
    print("peer slots filled:", peers, "flags:", np.bincount(flags, minlength=32).tolist())
    assert peers > ticks * n // 8
    assert np.array_equal(score["ego_flags"], flags) and (score["ego_flags"] & rmod.ROUTE_END).any()
    pl.close()


@gpu
def test_ring_closed_loop_agrees_with_the_cpu_loop(dm, oracle):
    """The end-to-end run on the device: 950 ticks of the CPU loop's scene.  Every integer field of every staged record equals the CPU
    loop's, pose and velocity agree within the bounds of the closed loop against the oracle in tests/test_rollout.py (parity_util.compare)."""
    r = _cpu_loop(dm, oracle)
    pl = _planner(dm, r["cfg"], r["m"], r["sc"])
    pl.set_route(r["legs"], r["rf"])
    model = dm.default_ego_model()
    worst = 0.0
    for t in range(E2E_TICKS):
        pl.tick()
        pl.advance_async(model)
        got, want = pl.get_scene_in(), r["sins"][t + 1]
        worst = max(worst, float(np.abs(got["loc"]["globalpoint"]["x"] - want["loc"]["globalpoint"]["x"]).max()),
                    float(np.abs(got["loc"]["globalpoint"]["y"] - want["loc"]["globalpoint"]["y"]).max()))
        bad = compare(got, want, "scene_in")
        assert not bad, f"tick {t} (largest position difference so far {worst!r} m)\n" + "\n".join(bad[:10])
    flags = pl.ego_flags()
    last = pl.get_scene_in()["loc"]
    print(f"largest position difference over {E2E_TICKS} ticks: {worst!r} m; legs {last['path_num'].tolist()}")
    assert np.array_equal(flags, r["flags"]) and ((flags & ~rmod.ROUTE_END) == 0).all()
    assert (last["pos"] == 0).all() and (last["path_num"] >= 2).all()
    pl.close()
