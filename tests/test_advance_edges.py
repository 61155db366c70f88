"""Edges of one rollout step (k_advance_egos / k_advance_route) that no generated closed loop reaches: the
second and later 64-segment passes of the path walk and its short last pass, its BAD_PATH / PATH_END / heading-held exits, the
path_near_id clamp and the speed branches; the strided loop of the windowed id search and its tie-breaking across lanes and strides;
junction tables of more than one 64-entry pass; the whole out_lane_no copy; the EgoTrace of out-of-range lane numbers.

Every case has a hand-derived literal and is written once against advance_backends.Runner: asserted on the numpy model (CPU) and
on the device (injected PlanOut / SceneState), where each step is also held against the model (integers and carried-over bytes
exact, x / y / velocity 1e-9, heading 1e-6 degrees) and then run again inside batches of distinct scenes.  All coordinates are
dyadic and the build has -ffp-contract=off, so the pose literals are asserted with == on both backends.  No case is left out for a
tie: where a tie is the point of a case the model leg asserts that it is an exact one (gap 0.0)."""
import math

import numpy as np
import pytest

import advance_backends as ab
import ego_model as em
from test_rollout import _scene, _state, _straight
from test_route import _ego, _four, _legs, _path, _tiny_map

gpu = pytest.mark.gpu


@pytest.fixture()
def cfg0(dm):
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    return cfg


def _model(dm, window=None):
    m = dm.default_ego_model()
    if window is not None:
        m["window"] = window
    return m


def _one(dm, run, cfg, si, po, pool, near_id=0, afresh=0, window=None):
    r = run(cfg, _model(dm, window), si, [(po, _state(dm, near_id, afresh))], dict(lane_pool=pool))[0]
    return r.out[0], int(r.flags[0]), r


def _pose(out):
    g = out["loc"]["globalpoint"]
    return float(g["x"]), float(g["y"]), float(g["dir"])


def _po(dm, x0=100.0, step=0.5, spd=36.0, **kw):
    po = _straight(dm, x0=x0, step=step, **kw)
    po["result"]["desspd"] = spd
    return po


# ---------------------------------------------------------------------------------------------------------------
# the path walk.  36 km/h held: s = 1 m (test_kat_speed); 72 km/h held: s = 2 m
def _edges_walk(dm, cfg0, run):
    si, pool = _scene(dm, cfg0)
    # W1: spacing 1/64 from x = 100, k0 = 0: a = 63/64 after segments 0 .. 62, a + L = 1 >= s on segment 63 - lane 63, the last of
    # pass 1 - with t = (1 - 63/64)/(1/64) = 1: x = P[63] + 1/64 = 101, on point 64
    out, f, _ = _one(dm, run, cfg0, si, _po(dm, step=1 / 64), pool)
    assert (_pose(out), f) == ((101.0, 0.0, 0.0), 0)
    # W2: k0 = 1: segments 1 .. 64 are still one pass (c0 = 1): from P[1] = 100 + 1/64 to 101 + 1/64
    out, f, _ = _one(dm, run, cfg0, si, _po(dm, step=1 / 64), pool, near_id=1)
    assert (_pose(out), f) == ((101.0 + 1 / 64, 0.0, 0.0), 0)
    # W3: spacing 1/128: 128 segments, the step ends on segment 127, the last lane of pass 2
    out, f, _ = _one(dm, run, cfg0, si, _po(dm, step=1 / 128), pool)
    assert (_pose(out), f) == ((101.0, 0.0, 0.0), 0)
    # W4: spacing 1/128, k0 = 5, 72 -> 71 km/h (72 - 1.44 < 71: the target): s = 0.5 * 143 / 3.6 * 0.1 = 1.986 m, but only 194
    # segments = 1.515625 m are left - passes from 5, 69, 133 and 197, the last of 2 segments: PATH_END on P[199] = 100 + 199/128
    s72 = si.copy()
    s72["loc"]["velocity"] = 72.0
    out, f, _ = _one(dm, run, cfg0, s72, _po(dm, step=1 / 128, spd=71.0), pool, near_id=5)
    assert (_pose(out), float(out["loc"]["velocity"]), f) == ((100.0 + 199 / 128, 0.0, 0.0), 71.0, em.PATH_END)
    # W5: points 0 .. 80 coincide at (100, 0), then 0.5 m spacing: pass 1 is all zero-length segments and is skipped, in pass 2
    # segments 64 .. 79 too; segment 80 (100 -> 100.5) gives a = 0.5, segment 81 ends the step with t = 1: x = 101 = point 82
    po = _po(dm)
    po["road_points"]["x"][0] = 100.0 + 0.5 * np.maximum(np.arange(200) - 80, 0)
    out, f, _ = _one(dm, run, cfg0, si, po, pool)
    assert (_pose(out), f) == ((101.0, 0.0, 0.0), 0)
    # W6: all 200 points coincide: no segment at all - PATH_END on P[199], the heading held at 77
    po = _po(dm)
    po["road_points"]["x"][0], po["road_points"]["y"][0] = 123.5, 2.25
    out, f, _ = _one(dm, run, cfg0, si, po, pool)
    assert (_pose(out), float(out["loc"]["velocity"]), f) == ((123.5, 2.25, 77.0), 36.0, em.PATH_END)
    # W7: spacing 1/64 with a NaN at P[70]: at 36 km/h the walk ends in pass 1 (W1) and never looks at it; at 72 km/h (s = 2 m: 128
    # segments) segment 69 is on the walked part: BAD_PATH, loc untouched
    po = _po(dm, step=1 / 64)
    po["road_points"]["y"][0, 70] = np.nan
    out, f, _ = _one(dm, run, cfg0, si, po, pool)
    assert (_pose(out), f) == ((101.0, 0.0, 0.0), 0)
    po["result"]["desspd"] = 72.0
    out, f, _ = _one(dm, run, cfg0, s72, po, pool)
    assert f == em.BAD_PATH and out["loc"].tobytes() == s72[0]["loc"].tobytes()
    # W8: a segment whose squared length overflows (dx = 1e200): its length is infinite - BAD_PATH
    po = _po(dm)
    po["road_points"]["x"][0, 1] = 1e200
    out, f, _ = _one(dm, run, cfg0, si, po, pool)
    assert f == em.BAD_PATH and out["loc"].tobytes() == si[0]["loc"].tobytes()
    # W9: path_near_id is clamped to 0 .. 199: -5 walks from P[0] (100 -> 101); 199 and 250 stand on P[199] = 199.5 with no segment
    # ahead: PATH_END there, the heading held
    out, f, _ = _one(dm, run, cfg0, si, _po(dm), pool, near_id=-5)
    assert (_pose(out), f) == ((101.0, 0.0, 0.0), 0)
    for k in (199, 250):
        out, f, _ = _one(dm, run, cfg0, si, _po(dm), pool, near_id=k)
        assert (_pose(out), float(out["loc"]["velocity"]), f) == ((199.5, 0.0, 77.0), 36.0, em.PATH_END)
    # W10: speed.  desaccVd: v' = v + desacc*dt*3.6 whatever desspd says, never below 0: 1 - 1.08 < 0 -> 0, s = 0.5/36 m along
    # segment 10 from P[10] = 105; 5 - 1.08 = 3.92 is not clamped
    s1 = si.copy()
    s1["loc"]["velocity"] = 1.0
    po = _po(dm, spd=99.0)
    po["result"]["desaccVd"], po["result"]["desacc"] = 1, -3.0
    out, f, _ = _one(dm, run, cfg0, s1, po, pool, near_id=10)
    assert (float(out["loc"]["velocity"]), f) == (0.0, 0) and abs(float(out["loc"]["globalpoint"]["x"]) - (105.0 + 0.5 / 36.0)) < 1e-12
    assert float(out["loc"]["globalpoint"]["dir"]) == 0.0
    s1["loc"]["velocity"] = 5.0
    out, f, _ = _one(dm, run, cfg0, s1, po, pool, near_id=10)
    assert (float(out["loc"]["velocity"]), f) == (5.0 + -3.0 * 0.1 * 3.6, 0)
    # ... a desspd of +-inf holds v (36 km/h: 105 -> 106); a NaN velocity makes the distance NaN: BAD_PATH
    for g in (math.inf, -math.inf):
        out, f, _ = _one(dm, run, cfg0, si, _po(dm, spd=g), pool, near_id=10)
        assert (_pose(out), float(out["loc"]["velocity"]), f) == ((106.0, 0.0, 0.0), 36.0, 0)
    s1["loc"]["velocity"] = np.nan
    out, f, _ = _one(dm, run, cfg0, s1, _po(dm), pool, near_id=10)
    assert f == em.BAD_PATH and out["loc"].tobytes() == s1[0]["loc"].tobytes()


# ---------------------------------------------------------------------------------------------------------------
# the windowed id search
def _hairpin(dm, moved=False):
    """One lane of 128 points that comes back on itself: point j at (100 + 0.5 j, +1), point j + 64 at (100 + 0.5 j, -1), j < 64.
    moved: point 6 is taken away to y = 8 and point 10 put in its place, (103, +1)."""
    si = np.zeros(1, dm.SceneIn)
    pool = np.zeros(128, dm.GlobalPoint3D)
    pool["x"] = 100.0 + 0.5 * (np.arange(128) % 64)
    pool["y"] = np.where(np.arange(128) < 64, 1.0, -1.0)
    if moved:
        pool["y"][6] = 8.0
        pool["x"][10] = 103.0
    si["lanes"]["cur_n"], si["lanes"]["lane_sum"], si["lanes"]["lane_width"] = 128, 1, 3.75
    si["loc"]["lane_num"], si["loc"]["velocity"], si["loc"]["globalpoint"]["dir"] = 1, 36.0, 77.0
    return si, pool


def _edges_window(dm, cfg0, run):
    # the three 320-point lanes of _scene (x = 100 + 0.5 k), the ids of all three views at 50, the ego put on point 200 (199 -> 200 m):
    # [50, 50 + w) holds point 200 only for the largest window; otherwise the last point of the window is the nearest - 50 + w - 1,
    # found in the first stride of the lanes (w <= 64), the second (65, 128) or the third (129).  LANE_END: id' + w >= 320
    si, pool = _scene(dm, cfg0)
    for w, want, want_f in ((1, 50, 0), (64, 113, 0), (65, 114, 0), (128, 177, 0), (129, 178, 0), (2 ** 20, 200, em.LANE_END)):
        out, f, _ = _one(dm, run, cfg0, si, _po(dm, x0=199.0), pool, window=w)
        assert (out["loc"]["id"].tolist(), f) == ([want, want, want, 50, 50, 50, 50, 50], f) and f == want_f, w
        assert _pose(out) == (200.0, 0.0, 0.0)
    # a window cut by the end of the view: [300, 364) of 320 points, the ego beyond the end (299 -> 300 m = where point 400 would be)
    s2 = si.copy()
    s2["loc"]["id"][0, :3] = 300
    out, f, _ = _one(dm, run, cfg0, s2, _po(dm, x0=299.0), pool, window=64)
    assert (out["loc"]["id"].tolist(), f) == ([319, 319, 319, 50, 50, 50, 50, 50], em.LANE_END)
    # a negative id: [-7, 57) is searched from 0: the ego on point 20 (109 -> 110 m); [-70, -6) is empty: the id is kept
    s2["loc"]["id"][0, :3] = -7
    out, f, _ = _one(dm, run, cfg0, s2, _po(dm, x0=109.0), pool, window=64)
    assert (out["loc"]["id"].tolist(), f) == ([20, 20, 20, 50, 50, 50, 50, 50], 0)
    s2["loc"]["id"][0, :3] = -70
    out, f, _ = _one(dm, run, cfg0, s2, _po(dm, x0=109.0), pool, window=64)
    assert (out["loc"]["id"].tolist(), f) == ([-70, -70, -70, 50, 50, 50, 50, 50], 0)
    # an id at the end of its view keeps its value (and 320 + 32 >= 320: LANE_END)
    s2["loc"]["id"][0, :3] = 320
    out, f, _ = _one(dm, run, cfg0, s2, _po(dm, x0=109.0), pool)
    assert (out["loc"]["id"].tolist(), f) == ([320, 320, 320, 50, 50, 50, 50, 50], em.LANE_END)
    # the hairpin, the ego on y = 0 at (103, 0) (102 -> 103 m): points 6 (103, +1) and 70 (103, -1) are both at d2 = 1, every other
    # point at 1.25 or more: an exact tie between i and i + 64 - one lane, two strides - goes to i.  From id 3 the same two points
    # sit in lane 3; from id 0 in lane 6
    hp, hpool = _hairpin(dm)
    for id0 in (0, 3):
        hp["loc"]["id"][0, 0] = id0
        out, f, r = _one(dm, run, cfg0, hp, _po(dm, x0=102.0), hpool, window=128)
        assert (out["loc"]["id"].tolist(), f) == ([6, 0, 0, 0, 0, 0, 0, 0], em.LANE_END)
        assert r.gaps is None or r.gaps[0] == 0.0                        # (the model leg: the tie is exact)
    # ... and with point 10 in the place of point 6: index 10 (lane 10, first stride) ties with index 70 (lane 6, second stride) -
    # the lower index sits in the higher lane and wins
    hp, hpool = _hairpin(dm, moved=True)
    out, f, r = _one(dm, run, cfg0, hp, _po(dm, x0=102.0), hpool, window=128)
    assert (out["loc"]["id"].tolist(), f) == ([10, 0, 0, 0, 0, 0, 0, 0], em.LANE_END)
    assert r.gaps is None or r.gaps[0] == 0.0
    # window 64 sees [0, 64) only: point 10 alone
    out, f, r = _one(dm, run, cfg0, hp, _po(dm, x0=102.0), hpool, window=64)
    assert (out["loc"]["id"].tolist(), f) == ([10, 0, 0, 0, 0, 0, 0, 0], 0)
    assert r.gaps is None or r.gaps[0] == 0.25


# ---------------------------------------------------------------------------------------------------------------
# the junction table
REAL, REAL2, PAD = (1, 2, 2, 1, 0, 10), (1, 2, 2, 2, 10, 6), (2, 1, 1, 1, 0, 10)


def _padded_map(dm, n, entries):
    """_tiny_map with a junction table of n entries: `entries` (index -> record), every other entry a padding record from road 2
    back to road 1, whose keys no ego of these tests has.  REAL2: the keys of the real junction, lane 2 of road 2 as its
    target and a polyline of its own (6 points behind the real one's 10)."""
    m = _tiny_map(dm)
    jp = np.zeros(16, dm.GlobalPoint2D)
    jp["x"][:10], jp["x"][10:] = 150.0 + 0.5 * np.arange(10), 150.0 + 0.5 * np.arange(6)
    m["jpoints"] = jp
    m["junctions"] = np.array([entries.get(k, PAD) for k in range(n)], dm.MapJunction).reshape(n)
    return m


def _routed(dm, run, cfg, m, si, po, legs):
    r = run(cfg, dm.default_ego_model(), si, [(po, np.zeros(1, dm.SceneState))], dict(map=m), (legs, np.array([0, len(legs)], np.int32), None))[0]
    return r.out[0], int(r.flags[0])


def _edges_route(dm, cfg0, run):
    # 0 -> 1 as in test_kat_pre_junction_starts_at_pre_points (118.5 -> 119.5 = point 39: 99 - 39 <= 60), the junction found in the
    # last lane of pass 1, the first lanes of pass 2, the last lane of pass 2 and alone in pass 3, with and without a short tail
    for n, idx in ((64, 63), (65, 63), (65, 64), (128, 64), (128, 65), (128, 127), (129, 127), (129, 128)):
        m = _padded_map(dm, n, {idx: REAL})
        out, f = _routed(dm, run, cfg0, m, _ego(dm, m), _path(dm, 118.5), _legs(dm))
        assert (int(out["loc"]["pos"]), int(out["loc"]["id"][1]), f) == (1, 39, 0), (n, idx)
        assert _four(out["loc"]) == (1, 2, 2, 1) and (int(out["ref_off"]), int(out["ref_n"])) == (0, 10), (n, idx)
    # no entry matches, in tables of 0, 64 and 128 entries: the ego at id' = 68 (133 -> 134 m; 68 + 32 >= 100) missed its exit
    for n in (0, 64, 128):
        m = _padded_map(dm, n, {})
        out, f = _routed(dm, run, cfg0, m, _ego(dm, m, ego_id=60), _path(dm, 133.0), _legs(dm))
        assert (int(out["loc"]["pos"]), int(out["loc"]["id"][1]), f, _four(out["loc"])) == (0, 68, em.LANE_END, (0, 0, 0, 0)), n
    # the same three keys twice: the lowest index wins, in next_lanenum and in the polyline resolved from the four indices - both
    # copies in one pass (3 and 40), and in passes 1 and 2 (5 and 70), either copy first
    for n, first, second in ((64, 3, 40), (128, 5, 70)):
        for lo, want_lane, want_ref in ((REAL, 1, (0, 10)), (REAL2, 2, (10, 6))):
            m = _padded_map(dm, n, {first: lo, second: REAL2 if lo is REAL else REAL})
            out, f = _routed(dm, run, cfg0, m, _ego(dm, m), _path(dm, 118.5), _legs(dm))
            assert (int(out["loc"]["pos"]), f, _four(out["loc"])) == (1, 0, (1, 2, 2, want_lane)), (n, want_lane)
            assert (int(out["ref_off"]), int(out["ref_n"])) == want_ref, (n, want_lane)
    # 2 -> 0 as in test_kat_junction_is_left_at_the_end_of_the_polyline, the next leg with eight distinct out_lane_no: all four words
    m = _tiny_map(dm)
    legs = _legs(dm)
    legs["out_lane_no"][1] = [11, 12, 13, 14, 15, 16, 17, 18]
    si = _ego(dm, m, pos=2, road=2, lane=1, ego_id=0, four=(1, 2, 2, 1))
    si["loc"]["id"][0, 1] = 6
    out, f = _routed(dm, run, cfg0, m, si, _path(dm, 154.6), legs)
    assert (int(out["loc"]["pos"]), int(out["loc"]["path_num"]), f) == (0, 1, 0)
    assert (int(out["stub_attribute"]), out["out_lane_no"].tolist()) == (2, [11, 12, 13, 14, 15, 16, 17, 18])
    assert out["loc"]["id"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------
# the trace (every call above and below is also checked by Runner: the EgoTrace records are the staged records)
def _edges_trace(dm, cfg0, run):
    # lane number 0 has a right view only (slot 0), lane number 9 a left view only (slot 7); id_cur comes from slot
    # clamp(lane_num - 1, 0, 7): 0 and 7.  The ego goes from 130 to 131 m = point 62 of [50, 82)
    for ln, want_ids in ((0, [62, 50, 50, 50, 50, 50, 50, 50]), (9, [50, 50, 50, 50, 50, 50, 50, 62]), (2, [62, 62, 62, 50, 50, 50, 50, 50])):
        si, pool = _scene(dm, cfg0, lane_num=ln, lane_sum=8 if ln == 0 else 3)
        out, f, r = _one(dm, run, cfg0, si, _po(dm, x0=130.0), pool)
        t = r.trace[0]
        assert (out["loc"]["id"].tolist(), f) == (want_ids, 0), ln
        assert (float(t["pose"]["x"]), float(t["pose"]["y"]), float(t["pose"]["dir"]), float(t["velocity"])) == (131.0, 0.0, 0.0, 36.0)
        assert (int(t["id_cur"]), int(t["lane_num"]), int(t["flags"]), int(t["_pad"])) == (62, ln, 0, 0), ln
    # a scene that BAD_PATH stops: the trace is the untouched record and the flag
    si, pool = _scene(dm, cfg0)
    po = _po(dm)
    po["road_points"]["x"][0, 0] = np.inf
    out, f, r = _one(dm, run, cfg0, si, po, pool)
    t = r.trace[0]
    assert (float(t["pose"]["dir"]), float(t["velocity"]), int(t["id_cur"]), int(t["lane_num"]), int(t["flags"])) == (77.0, 36.0, 50, 2, em.BAD_PATH)


EDGES = [_edges_walk, _edges_window, _edges_route, _edges_trace]


def _runner(name, log=None):
    return ab.Runner(ab.ModelBackend() if name == "model" else ab.DeviceBackend(), log)


@pytest.mark.parametrize("edges", EDGES, ids=lambda f: f.__name__[7:])
def test_edges_on_the_model(dm, cfg0, edges):
    edges(dm, cfg0, _runner("model"))


@gpu
@pytest.mark.parametrize("edges", EDGES, ids=lambda f: f.__name__[7:])
def test_edges_on_the_device(dm, cfg0, edges):
    edges(dm, cfg0, _runner("device"))
    print(f"device against model so far: {ab.STATS}")


@gpu
def test_edges_batch_equals_each_case_alone(dm, cfg0):
    """Every edge case once more on the device, logged, then as distinct scenes of one launch per group of calls that can share one
    (advance_backends.batched): the batch sizes are no multiple of four and span more than one block; bytes as alone."""
    log = []
    run = _runner("device", log)
    for edges in EDGES:
        edges(dm, cfg0, run)
    sizes = ab.batched(ab.DeviceBackend(), log)
    print(f"{len(log)} calls in batches of {sizes}; device against model: {ab.STATS}")
    assert sum(sizes) >= len(log) and all(n % 4 != 0 and n > 4 for n in sizes)
