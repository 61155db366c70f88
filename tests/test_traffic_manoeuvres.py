"""Traffic manoeuvres: triggered lane changes, lateral offsets and speed changes of the actors of pp_set_traffic.

CPU: hand-derived known answers on the numpy model (tests/traffic_manoeuvre_model.py, written from the section), the model with every
trigger out of reach against §4h's and §4i's models, and pp_check_traffic_manoeuvres rule by rule.  GPU: k_manoeuvre_traffic held to
the model byte for byte after every advance - states, s, v and the pinned pool entries - on the projection's wave edges, the
scene-wide group scan and the triggers, each case alone and as scenes of one launch of all cases.  Idle-is-plain-traffic,
pp_update_async, the episode reset and the calls: tests/test_traffic_manoeuvre_calls.py.

The track vertices lie every metre on axis-parallel lines and the poses are dyadic, so every literal below is exact."""
import ctypes

import numpy as np
import pytest

import manoeuvre_scenes as ms
import traffic_follow_model as fm
import traffic_manoeuvre_model as mm
import traffic_model as tm
import traffic_scenes as ts

gpu = pytest.mark.gpu
FAR = ms.FAR
R, T = 0.9, 3          # radius and type of every actor


def two_lanes(dm, n=41):
    return [(ms.line(dm, n), False), (ms.line(dm, n, y=3.5), False)]


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirrors(dm):
    lib = dm.load_library()
    assert (lib.pp_sizeof(47), lib.pp_sizeof(48)) == (dm.TrafficManoeuvre.itemsize, dm.TrafficManoeuvreState.itemsize) == (56, 48)
    assert lib.pp_sizeof(42) == 0 and lib.pp_sizeof(49) == 0
    assert dm.TrafficManoeuvre.names == mm.RECORD.names and dm.TrafficManoeuvreState.names == mm.STATE.names
    assert [dm.TrafficManoeuvre.fields[k][1] for k in mm.RECORD.names] == [mm.RECORD.fields[k][1] for k in mm.RECORD.names]
    assert [dm.TrafficManoeuvreState.fields[k][1] for k in mm.STATE.names] == [mm.STATE.fields[k][1] for k in mm.STATE.names]
    assert (dm.MANOEUVRE_MAX, dm.TRIG_ADVANCES, dm.TRIG_EGO_DIST, dm.TRIG_EGO_TIME) == (8, 0, 1, 2)
    lib.pp_feature_retires.argtypes, lib.pp_feature_retires.restype = [ctypes.c_int], ctypes.c_int
    assert lib.pp_feature_retires(14) == -1          # no feature bit, no cause: the table is as it was


def _cut_in_case(dm):
    """Actor 0 on y = 0 at x = 10 cuts onto y = 3.5 (right of it: lat0 = -3.5) in 4 advances, then - one idle advance later - moves 1 m to
    the left in 2 advances at 4 m/s; actor 1 on y = 3.5 cuts onto y = 0 (lat0 = +3.5)."""
    recs = [mm.record(0, track=1, n_steps=4), mm.record(0, after=1, lat_end=1.0, speed=4.0, n_steps=2), mm.record(1, track=0, n_steps=4)]
    return ms.case("cut_in_kat", two_lanes(dm), [dict(ego=FAR, actors=[(10.0, 2.0, 0, T, R), (10.0, 2.0, 1, T, R)])], recs)


def test_known_answers_cut_in_ramp_and_chain(dm):
    r = ms.run_model(dm, _cut_in_case(dm), steps=8)
    st, s, ob = r.st, r.s, r.ob
    assert r.info[1][0].projected == (10, 9) and r.info[1][1].projected == (10, 9)          # vertex 10 lies abreast; segments 9 | 10 tie: the earlier one, t = 1
    # advance 1: the same abscissa on the other track, lat0 = -+3.5 exactly, one step of 2 m/s * 0.5 s, k = 1: w = 1/16 * 2.5
    assert (st[1]["track"].tolist(), st[1]["lat0"].tolist(), s[1].tolist(), st[1]["k"].tolist()) == ([1, 0], [-3.5, 3.5], [11.0, 11.0], [1, 1])
    assert st[1]["lat"].tolist() == [-3.5 + 3.5 * 0.15625, 3.5 - 3.5 * 0.15625]
    assert (ob[1]["x"].tolist(), ob[1]["y"].tolist()) == ([11.0, 11.0], [3.5 - 2.953125, 2.953125])
    # advance 2 = n_steps / 2: w = 0.5, lat = -+1.75 exactly
    assert st[2]["lat"].tolist() == [-1.75, 1.75] and ob[2]["y"].tolist() == [1.75, 1.75] and ob[2]["x"].tolist() == [12.0, 12.0]
    # advance 4 = n_steps: lat = lat_end exactly, idle, clock = 0
    assert st[4]["lat"].tolist() == [0.0, 0.0] and st[4]["k"].tolist() == [0, 0] and st[4]["clock"].tolist() == [0, 0]
    assert st[4]["next"].tolist() == [1, 1] and st[4]["n_done"].tolist() == [1, 1] and ob[4]["y"].tolist() == [3.5, 0.0]
    assert r.info[4][0].finished and r.info[4][1].finished
    # the chain: advance 5 is idle (clock 0 < after 1), advance 6 fires record 1: v0 = 4, lat0 = 0, tau = 1/2: w = 1/2
    assert st[5]["clock"].tolist() == [1, 1] and st[5]["k"].tolist() == [0, 0] and s[5].tolist() == [15.0, 15.0]
    assert r.info[6][0].fired and not r.info[6][1].fired
    assert (st[6]["v0"].tolist(), st[6]["lat"].tolist(), st[6]["k"].tolist(), s[6].tolist()) == ([4.0, 2.0], [0.5, 0.0], [1, 0], [17.0, 16.0])
    assert (st[7]["lat"].tolist(), st[7]["n_done"].tolist(), st[7]["next"].tolist(), st[7]["clock"].tolist()) == ([1.0, 0.0], [2, 1], [2, 1], [0, 3])
    assert (ob[7]["x"].tolist(), ob[7]["y"].tolist()) == ([19.0, 17.0], [4.5, 0.0])
    assert st[8]["clock"].tolist() == [1, 4] and st[8]["track"].tolist() == [1, 0]          # speed = NaN kept v0 = 2 for actor 1 throughout
    assert st[8]["v0"].tolist() == [4.0, 2.0]


def _trigger_case(dm, nan_ego=False):
    """Parked actors at (5, 0) on a line along +x; a record starts them at 1 m/s with an offset of 1 m in 2 advances.
    scene 0, ego (2, -4): d2 = 25, p = 3.  scene 1, ego (5, -4): d2 = 16, p = 0.  scenes 2 / 3: ego (2, -4) at 36 km/h, flagged / not."""
    def rec(a, kind, side=0, **kw):
        return mm.record(a, kind, side, lat_end=1.0, speed=1.0, n_steps=2, **kw)
    below = float(np.nextafter(5.0, 0.0))
    scenes = [dict(ego=(2.0, -4.0, 0.0, False), actors=[(5.0, 0.0, 0, T, R)] * 4),
              dict(ego=(5.0, -4.0, 0.0, False), actors=[(5.0, 0.0, 0, T, R)] * 2),
              dict(ego=(2.0, -4.0, 36.0, True), actors=[(5.0, 0.0, 0, T, R)]),
              dict(ego=(2.0, -4.0, 36.0, False), actors=[(5.0, 0.0, 0, T, R)] * 2)]
    recs = [rec(0, mm.EGO_DIST, dist=5.0), rec(1, mm.EGO_DIST, dist=below), rec(2, mm.EGO_DIST, 1, dist=5.0), rec(3, mm.EGO_DIST, 2, dist=5.0),
            rec(4, mm.EGO_DIST, 1, dist=4.0), rec(5, mm.EGO_DIST, 2, dist=4.0), rec(6, mm.EGO_TIME, time=100.0), rec(7, mm.EGO_TIME, time=1.0),
            rec(8, mm.EGO_TIME, time=0.4)]
    fires = [True, False, True, False, True, True, False, True, False]
    if nan_ego:
        scenes.append(dict(ego=(np.nan, -4.0, 36.0, False), actors=[(5.0, 0.0, 0, T, R)] * 2))
        recs += [rec(9, mm.EGO_DIST, dist=1e300), rec(10, mm.EGO_TIME, time=1e300)]
        fires += [False, False]
    return ms.case("triggers", [(ms.line(dm, 41), False)], scenes, recs, expect=dict(fires=fires))


def _check_triggers(c, r):
    for a, f in enumerate(c.expect["fires"]):
        assert [bool(i[a].fired) for i in r.info[1:]] == [f] + [False] * (len(r.info) - 2), f"actor {a}"
        assert r.st[-1]["n_done"][a] == (1 if f else 0) and r.st[-1]["lat"][a] == (1.0 if f else 0.0) and r.st[-1]["v0"][a] == (1.0 if f else 0.0)
        assert r.s[-1][a] == (5.0 + 0.5 * (len(r.s) - 1) if f else 5.0)


def test_known_answers_triggers(dm):
    """EGO_DIST fires on d2 == dist * dist and not one ulp below; sides 1 and 2 are both taken on p == 0; EGO_TIME never fires for a flagged
    ego; a NaN ego fires nothing."""
    c = _trigger_case(dm, nan_ego=True)
    _check_triggers(c, ms.run_model(dm, c))


def _idle(c):
    r = c.recs.copy()
    r["after"] = 2 ** 30
    return ms.case(c.name + "_idle", c.polylines, c.scenes, [r], c.tf)


@pytest.mark.parametrize("follow", [False, True])
def test_out_of_reach_is_plain_traffic_on_the_model(dm, follow):
    """Every trigger out of reach (after = 2^30): 40 advances give the bytes of tests/traffic_model.py / tests/traffic_follow_model.py."""
    c = _idle(_scene_case(dm, 65, ego=(50.0, 0.0, 10.0, False), tf={} if follow else None))
    act, stride, _, _ = ms.fb._layout(dm, c.scenes, None)
    tracks, pts = ts.pack(dm, c.polylines)
    si, flags = ms.fb._egos(dm, c.scenes)
    a, b = mm.Manoeuvres(tracks, pts, act, np.arange(1) * stride, c.recs), fm.Follow(tracks, pts, act, np.arange(1) * stride)
    pa, _ = a.place(ts.filled(dm.ObPoint, stride), None, 0.0)
    pb, _ = b.place(ts.filled(dm.ObPoint, stride), None, 0.0)
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    kinds = set()
    for k in range(40):
        pa, _ = a.advance(pa, None, ms.DT, c.tf, si, flags, width)
        pb, _ = b.step(pb, None, ms.DT, c.tf, si, flags, width) if follow else b.place(pb, None, ms.DT)
        assert pa.tobytes() == pb.tobytes() and a.s.tobytes() == b.s.tobytes() and (not follow or a.v.tobytes() == b.v.tobytes()), f"advance {k}"
        kinds |= {i.step.kind for i in a.minfo}
    assert a.st["clock"].tolist() == [40] * 65 and not a.st["n_done"].any()
    assert kinds == ({"actor", "ego", "free"} if follow else {"plain"})


def _bad_lists():
    ok = lambda **kw: mm.record(1, mm.EGO_DIST, 1, dist=3.0, n_steps=5, track=1, **kw)          # noqa: E731
    def edit(**kw):
        r = ok()
        for k, v in kw.items():
            r[k] = v
        return r
    nine = [mm.record(1)] * 9
    return {"actor < 0": [edit(actor=-1)], "actor out of range": [edit(actor=4)], "track out of range": [edit(track=3)], "track < -1": [edit(track=-2)],
            "out of order": [ok(), mm.record(0)], "more than 8 for one actor": nine, "unknown kind": [edit(trigger=3)], "unknown side": [edit(trigger=1 | 3 << 8)],
            "a side on ADVANCES": [edit(trigger=0 | 1 << 8)], "negative trigger": [edit(trigger=-255)],
            "dist NaN": [edit(dist=np.nan)], "dist inf": [edit(dist=np.inf)], "dist < 0": [edit(dist=-1.0)],
            "time NaN": [edit(trigger=2, time=np.nan)], "time < 0": [edit(trigger=2, time=-0.5)], "lat_end inf": [edit(lat_end=np.inf)], "lat_end NaN": [edit(lat_end=np.nan)],
            "speed inf": [edit(speed=-np.inf)], "after < 0": [edit(after=-1)], "n_steps 0": [edit(n_steps=0)], "n_steps 4097": [edit(n_steps=4097)], "_pad": [edit(_pad=1)]}


def _lib_check(dm, n_actors, n_tracks, recs):
    r = np.ascontiguousarray(recs, dm.TrafficManoeuvre)
    return dm.load_library().pp_check_traffic_manoeuvres(n_actors, n_tracks, len(r), r.ctypes.data if len(r) else None)


def test_check_refuses_one_record_per_rule(dm):
    legal = mm.records(mm.record(0), mm.record(1, mm.EGO_DIST, 1, dist=0.0, speed=-2.0, track=2, n_steps=4096), mm.record(1, mm.EGO_TIME, 2, time=0.0, after=7),
                       mm.record(1, mm.EGO_TIME, dist=np.nan, time=1.0), mm.record(3, mm.ADVANCES, dist=-1.0, time=np.inf))
    assert mm.check(4, 3, legal) == -1 and _lib_check(dm, 4, 3, legal) == -1          # (dist and time are read by their own kind only)
    assert _lib_check(dm, 4, 3, legal[:0]) == -1
    lib = dm.load_library()
    assert lib.pp_check_traffic_manoeuvres(4, 3, 2, None) == 0 and lib.pp_check_traffic_manoeuvres(4, 3, -1, legal.ctypes.data) == 0
    eight = mm.records(*[mm.record(1)] * 8)
    assert mm.check(4, 3, eight) == -1 and _lib_check(dm, 4, 3, eight) == -1
    for name, bad in _bad_lists().items():
        lst = mm.records(legal[:1], *bad)
        want = len(lst) - 1
        assert mm.check(4, 3, lst) == want, name
        assert _lib_check(dm, 4, 3, lst) == want, name


def test_projection_on_the_model_with_a_nan_vertex(dm):
    """A NaN vertex is never the nearest one and a segment that ends on it is no candidate (pp_set_traffic refuses such a track, so
    this edge exists on the model alone)."""
    px, py = np.arange(6.0), np.full(6, 3.5)
    px[2] = np.nan
    cum = np.arange(6.0)
    s, lat0, j, seg = mm.project(px, py, cum, False, 1.75, 0.0)
    assert (j, seg, s, lat0) == (1, 0, 1.0, -3.5)                # vertex 2 would be nearest; segment 1 ends on it: its foot is a NaN
    assert mm.project(np.full(3, np.nan), py[:3], cum[:3], False, 1.0, 0.0) is None


# ---- the cases of the device tests ------------------------------------------------------------------------------------------------
def _proj_case(dm, name, target, x, expect, closed=False, y=0.0):
    """One actor on the line y (200 vertices from x = -16) at abscissa x, 2 m/s; advance 1 projects it onto `target`."""
    src = ms.line(dm, 200, x0=-16.0, y=y)
    return ms.case(name, [(src, False), (target, closed)], [dict(ego=FAR, actors=[(x + 16.0, 2.0, 0, T, R)])], [mm.record(0, track=1, n_steps=4)],
                   expect=dict(projected=expect))


def _square(dm):
    xy = [(float(k), 0.0) for k in range(10)] + [(10.0, float(k)) for k in range(10)] + [(10.0 - k, 10.0) for k in range(10)] + [(0.0, 10.0 - k) for k in range(10)]
    return ts.polyline(dm, xy)


def _proj_cases(dm):
    up = lambda n: ms.line(dm, n, y=3.5)          # noqa: E731
    dup = ts.polyline(dm, [(0.0, 3.5), (1.0, 3.5), (1.0, 3.5)] + [(float(k), 3.5) for k in range(2, 20)])
    return [
        _proj_case(dm, "n2", up(2), 0.25, (0, 0, 0.25, -3.5)),
        _proj_case(dm, "n63_last_vertex", up(63), 61.75, (62, 61, 61.75, -3.5)),
        _proj_case(dm, "n64_lane63_foot_t1", up(64), 63.0, (63, 62, 63.0, -3.5)),
        _proj_case(dm, "n65_second_pass_lane0", up(65), 63.75, (64, 63, 63.75, -3.5)),
        _proj_case(dm, "n128_tie_across_passes", up(128), 63.5, (63, 63, 63.5, -3.5)),
        _proj_case(dm, "n129_third_pass", up(129), 127.75, (128, 127, 127.75, -3.5)),
        _proj_case(dm, "n129_tie_in_a_pass", up(129), 10.5, (10, 10, 10.5, -3.5)),
        _proj_case(dm, "foot_t0", up(64), 0.0, (0, 0, 0.0, -3.5)),
        _proj_case(dm, "foot_on_vertex_tie_of_segments", up(64), 20.0, (20, 19, 20.0, -3.5)),
        _proj_case(dm, "before_the_start", up(64), -3.0, (0, 0, 0.0, -3.5)),
        _proj_case(dm, "past_the_end", up(64), 66.0, (63, 62, 63.0, -3.5)),
        _proj_case(dm, "closing_segment", _square(dm), -1.0, (0, 39, 39.5, -1.0), closed=True, y=0.5),
        _proj_case(dm, "zero_length_segment", dup, 1.25, (1, 0, 1.0, -3.5)),
    ]


def _check_projection(c, r):
    j, seg, s, lat0 = c.expect["projected"]
    assert r.info[1][0].projected == (j, seg), (c.name, r.info[1][0].projected)
    assert r.st[1]["lat0"][0] == lat0 and r.st[1]["track"][0] == 1, (c.name, r.st[1])
    track = c.polylines[1]
    L = tm.cumulative(track[0]["x"], track[0]["y"], track[1])[-1]
    assert r.s[1][0] == tm.wrap(s + 1.0, L, track[1]), (c.name, r.s[1][0])          # the projected s, then one step of 2 m/s * 0.5 s
    assert r.st[4]["lat"][0] == 0.0 and r.st[4]["n_done"][0] == 1


def _scene_case(dm, n, ego=FAR, tf={}):
    """One scene of n actors on two lines 3.5 m apart, 4 m between neighbours, desired speeds 3 .. 5 m/s: the first n - 32 on y = 0, the
    last 32 on y = 3.5.  Actor 5 cuts from y = 0 onto y = 3.5 in advance 1, the last actor from y = 3.5 onto y = 0 in advance 2."""
    na = n - 32
    rows = [(4.0 * i, 3.0 + i % 3, 0, T, R) for i in range(na)] + [(4.0 * i, 3.0 + (i + 1) % 3, 1, T, R) for i in range(32)]
    recs = [mm.record(5, track=1, n_steps=3), mm.record(n - 1, after=1, track=0, n_steps=3, speed=6.0)]
    return ms.case(f"scene{n}", [(ms.line(dm, 260), False), (ms.line(dm, 260, y=3.5), False)], [dict(ego=ego, actors=rows)], recs, tf)


def _group_cases(dm):
    lanes3 = [(ms.line(dm, 120), False), (ms.line(dm, 120, y=3.5), False), (ms.line(dm, 120, y=7.0), False)]
    cut = ms.case("new_leader_and_group_left_behind", lanes3[:2],
                  [dict(ego=FAR, actors=[(30.0, 5.0, 0, T, R), (20.0, 5.0, 0, T, R), (18.0, 5.0, 1, T, R)])], [mm.record(0, after=1, track=1, n_steps=3)], {},
                  expect=dict(kinds={1: ["free", "actor", "free"], 2: ["free", "actor", "free"], 3: ["free", "free", "actor"]}, leaders={(1, 1): 0, (2, 1): 0, (3, 2): 0}))
    same = ms.case("two_land_on_equal_s", lanes3, [dict(ego=FAR, actors=[(20.0, 5.0, 0, T, R), (20.0, 5.0, 2, T, R)])],
                   [mm.record(0, track=1, n_steps=3), mm.record(1, track=1, n_steps=3)], {},
                   expect=dict(kinds={1: ["free", "free"], 2: ["free", "actor"]}, leaders={(2, 1): 0}, equal_s=1))
    return [cut, same, _scene_case(dm, 64), _scene_case(dm, 65)]


def _check_group(c, r):
    for k, kinds in c.expect.get("kinds", {}).items():
        assert [i.step.kind for i in r.info[k]] == kinds, (c.name, k, [i.step.kind for i in r.info[k]])
    for (k, a), b in c.expect.get("leaders", {}).items():
        assert r.info[k][a].step.leader == b, (c.name, k, a)
    if "equal_s" in c.expect:
        k = c.expect["equal_s"]
        assert r.s[k][0] == r.s[k][1] and r.st[k]["track"].tolist() == [1, 1] and r.st[k]["lat0"].tolist() == [-3.5, 3.5]
        assert r.info[2][1].step.g == 0.0 and r.s[2][1] < r.s[2][0]          # the lower index is ahead: the other one brakes
    if c.name.startswith("scene"):
        n = len(c.scenes[0]["actors"])
        assert r.info[1][5].projected is not None and r.info[2][n - 1].projected is not None and r.st[-1]["n_done"].sum() == 2
        assert all(i.step.kind in ("actor", "free") for i in r.info[3]) and sum(i.step.kind == "actor" for i in r.info[3]) >= n - 4
        if n == 65:          # the follower of the last actor finds it in the second pass over the scene's members
            assert r.info[1][63].step.leader == 64 and r.info[3][63].step.leader != 64


def _all_cases(dm, follow):
    if follow:
        return [(c, _check_group) for c in _group_cases(dm)]
    return [(c, _check_projection) for c in _proj_cases(dm)] + [(_trigger_case(dm), _check_triggers), (_cut_in_case(dm), None)]


N_CASES = {False: 15, True: 4}
_ALONE = {}


def _alone(dm, follow, k):
    if (follow, k) not in _ALONE:
        c, chk = _all_cases(dm, follow)[k]
        r = ms.run_device(dm, c)
        if chk is not None:
            chk(c, r)
        _ALONE[(follow, k)] = r
    return _ALONE[(follow, k)]


@pytest.mark.parametrize("follow,k", [(f, k) for f in (False, True) for k in range(N_CASES[f])])
def test_case_on_the_model(dm, follow, k):
    """What every case expects of the branch record, on the model alone: a case that stops reaching its edge fails without a GPU."""
    assert len(_all_cases(dm, follow)) == N_CASES[follow]
    c, chk = _all_cases(dm, follow)[k]
    if chk is not None:
        chk(c, ms.run_model(dm, c))


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("follow,k", [(f, k) for f in (False, True) for k in range(N_CASES[f])])
def test_case_on_the_device(dm, follow, k):
    """Projection edges and triggers with following off, group edges with following on: every advance byte for byte against the model."""
    _alone(dm, follow, k)


@gpu
@pytest.mark.parametrize("follow", [False, True])
def test_cases_as_scenes_of_one_launch(dm, follow):
    """All cases as the scenes of ONE launch: the device is the model's, and every actor gives the bytes its case gave alone."""
    cases = [c for c, _ in _all_cases(dm, follow)]
    joined, base = ms.join(cases)
    ms.same_alone(ms.run_device(dm, joined), base, cases, [_alone(dm, follow, k) for k in range(len(cases))])
