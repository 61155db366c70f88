"""World traffic (pp_set_world_traffic / k_move_world_traffic / k_follow_world_traffic): one vehicle per world of a
fleet, written into the same own-obstacle slot of every member scene and led by the nearest of all the world's egos.

CPU: hand-derived known answers of the numpy model (tests/world_traffic_model.py) - the leader that lives in another member scene,
the tie rules, the stride edges of the kernel's member loops, the window edges, the world borders, flags, slots and pools, parked
and reversing vehicles -, each alone and replayed as worlds of one launch; worlds of one scene against §4h / §4i's models byte for
byte; a platoon of ring egos in the closed loop of oracle + route model + fleet model + world model against per-scene copies.
GPU: all of those cases on the two kernels, each held to the model BYTE FOR BYTE after the set calls and after every advance
(s, v, the full obstacle slice of every member scene and every byte of both pools: the 0xA5 fill must survive wherever nothing is
pinned; the model is fed the ego poses, velocities and flag words the device itself staged); pp_update_async; worlds of one against
pp_set_traffic on the device; the error paths and the life cycle; a routed fleet rollout against the model.

Every case also asserts, from the model's record of the step, which branch it took.

One known answer runs on the model only: a NaN ego position in a member scene, for the reason §4i gives - the advance never stages
one unflagged, and a resident record with a NaN pose would send the tick's own kernels through it."""
import numpy as np
import pytest

import fleet_model as fl
import route_scenes as rs
import traffic_follow_backends as fb
import traffic_follow_model as fm
import traffic_model as tm
import traffic_scenes as ts
import world_traffic_backends as wb
import world_traffic_model as wm

gpu = pytest.mark.gpu
FAR = (4096.0, 4096.0, 0.0, False)          # an ego nowhere near a track
FILL_OB = bytes([ts.FILL]) * 24
FILL_MOT = bytes([ts.FILL]) * 16


def _runner(dm, name, log=None):
    return wb.Runner(dm, wb.ModelBackend() if name == "model" else wb.DeviceBackend(), log)


def straight(dm, n, step=1.0, y=0.0):
    return ts.polyline(dm, [(k * step, y) for k in range(n)])


def square(dm):
    """40 points, 1 m apart, round the square (0, 0) - (10, 10); closed: L = 40 (tests/test_traffic_follow.py)."""
    xy = [(float(k), 0.0) for k in range(10)] + [(10.0, float(k)) for k in range(10)] + [(10.0 - k, 10.0) for k in range(10)] + [(0.0, 10.0 - k) for k in range(10)]
    return ts.polyline(dm, xy)


def _same_in_every_member(r, stage, a):
    first = r.entry(stage, a, 0).tobytes()
    assert first != FILL_OB
    assert all(r.entry(stage, a, m).tobytes() == first for m in range(len(r.layout.entries[a]))), f"stage {stage}, vehicle {a}: the members' entries differ"


# ---------------------------------------------------------------------------------------------------------------
# The known answers, written once against a runner of tests/world_traffic_backends.py.  Everything is a multiple of a small power
# of two unless a comment says otherwise, so the arithmetic below is exact in binary.
def _kat_leader_lives_in_the_other_scene(dm, run):
    # 1.  A world of two egos on one 1 m track, both at 14.4 km/h = 4 m/s: member 0, the FRONT ego, on vertex 35, member 1, the REAR ego,
    # on vertex 20.  The vehicle at s = 7.5 (v0 = v = 4, radius 0.5): i0 = 7, vertex 20 is k = 13, g = 12.5; vertex 35 is k = 28, g = 27.5.
    # The leader is the nearer ego, member 1, although slot 0 of member 0 holds the vehicle too: net = 12.5 - 0.5 - 0.9, dv = 0,
    # dyn = 4 * 1.5 = 6.  A per-scene copy in member 0 (§4i) would see the front ego only, 15 m further on.
    poly = [(straight(dm, 101), False)]
    row = (7.5, 4.0, 0, 3, 0.5)
    r = run(poly, [dict(egos=[(35.0, 0.0, 14.4, False), (20.0, 0.0, 14.4, False)], actors=[row])])
    i = r.info[1][0]
    assert (i.kind, i.ego_scene, i.ego_candidates, i.kstar, float(i.g), float(i.vl), float(i.dyn)) == ("ego", 1, [0, 1], 13, 12.5, 4.0, 6.0)
    assert float(i.net) == 12.5 - 0.5 - 0.5 * 1.8 and i.n_world == 2
    for stage in (0, 1, 2):
        _same_in_every_member(r, stage, 0)
    assert r.at(0, 0) == (7.5, 4.0, 7.5, 0.0) and r.entry(1, 0, 1)["type"] == 3 and r.entry(1, 0, 1)["radius"] == 0.5
    # against §4i's model: the copy of the rear ego's scene gives these bytes, the copy of the front ego's scene does not
    copies = fb.ModelBackend().run(dm, poly, [dict(ego=(35.0, 0.0, 14.4, False), actors=[row]), dict(ego=(20.0, 0.0, 14.4, False), actors=[row])], fm.params(None), 0.5, 2)
    for stage in (1, 2):
        assert r.s[stage][0].tobytes() == copies.s[stage][1].tobytes() and r.v[stage][0].tobytes() == copies.v[stage][1].tobytes()
        assert r.s[stage][0] < copies.s[stage][0] and r.v[stage][0] < copies.v[stage][0]          # the front ego's copy brakes less


def _kat_tie_neighbouring_lanes(dm, run):
    # 2a.  Six members; the egos of members 3 and 4 have the same nearest vertex, 20, so g_e = 12.5 for both: the lower scene, 3, leads
    # (14.4 km/h: vl = 4) although member 4's ego (standing: vl = 0) is nearer to the vertex (d2 = 0 against 0.25).
    egos = [FAR, FAR, FAR, (20.0, 0.5, 14.4, False), (20.0, 0.0, 0.0, False), FAR]
    r = run([(straight(dm, 101), False)], [dict(egos=egos, actors=[(7.5, 4.0, 0, 0, 0.5)])])
    i = r.info[1][0]
    assert (i.kind, i.ego_scene, i.ego_candidates, float(i.g), float(i.vl), float(i.d2)) == ("ego", 3, [3, 4], 12.5, 4.0, 0.25)
    _same_in_every_member(r, 1, 0)


def _kat_tie_64_members_apart(dm, run):
    # 2b.  66 members; members 1 and 65 - the same lane of the kernel's stride, different passes - tie at g_e = 12.5: member 1 leads.
    egos = [FAR] * 66
    egos[1], egos[65] = (20.0, 0.5, 14.4, False), (20.0, 0.0, 0.0, False)
    r = run([(straight(dm, 101), False)], [dict(egos=egos, actors=[(7.5, 4.0, 0, 0, 0.5)])])
    i = r.info[1][0]
    assert (i.kind, i.ego_scene, i.ego_candidates, float(i.g), float(i.vl), i.n_world) == ("ego", 1, [1, 65], 12.5, 4.0, 66)
    _same_in_every_member(r, 1, 0)


def _kat_tie_ego_wins_against_an_actor(dm, run):
    # 2c.  Member 1's ego on vertex 20 and vehicle 1 at s = 20; the follower at s = 9.5: g_e = 10.5 = g_b.  The ego wins: its radius and speed count.
    r = run([(straight(dm, 101), False)], [dict(egos=[FAR, (20.0, 0.0, 0.0, False)], actors=[(9.5, 4.0, 0, 0, 0.5), (20.0, 2.0, 0, 0, 0.25)])])
    i = r.info[1][0]
    assert (i.kind, i.ego_scene, float(i.actor_g), float(i.ego_g), float(i.vl), float(i.net)) == ("ego", 1, 10.5, 10.5, 0.0, 10.5 - 0.5 - 0.5 * 1.8)


SIZES = [1, 2, 63, 64, 65, 129]


def _kat_stride_edges_of_the_members(dm, run):
    # 3a.  One world per size; the only ego within `lateral` is the LAST member (vertex 20, 4 m/s), every other ego is far away: the
    # leader is found in the last lane of the last pass, and the stores reach the last member's entry.
    worlds = [dict(egos=[FAR] * (n - 1) + [(20.0, 0.0, 14.4, False)], actors=[(7.5, 4.0, 0, 10 + n, 0.5)]) for n in SIZES]
    r = run([(straight(dm, 101), False)], worlds)
    first = 0
    for a, n in enumerate(SIZES):
        i = r.info[1][a]
        assert (i.kind, i.ego_scene, i.ego_candidates, i.n_world, float(i.g), float(i.vl)) == ("ego", first + n - 1, [first + n - 1], n, 12.5, 4.0), n
        for stage in (0, 1, 2):
            _same_in_every_member(r, stage, a)
        last = r.entry(2, a, n - 1)
        assert (float(last["x"]), float(last["y"]), int(last["type"])) == (float(r.s[2][a]), 0.0, 10 + n)
        first += n
    assert r.s[1].tobytes() == np.full(len(SIZES), r.s[1][0]).tobytes()          # every world saw the same thing


def _kat_group_of_65(dm, run):
    # 3b.  A (world, track) group of 65 vehicles in a world of two scenes, twice: vehicle 0 at s = 0 is under test, its leader is vehicle p
    # at s = 5 - p = 63 the last lane of the first pass, p = 64 the first lane of the second -, the others stand at 10 + 0.25 i.
    worlds = [dict(egos=[FAR, FAR], actors=[(0.0 if i == 0 else 5.0 if i == p else 10.0 + 0.25 * i, 3.0, 0, i, 0.125) for i in range(65)]) for p in (63, 64)]
    r = run([(straight(dm, 201), False)], worlds)
    for w, p in enumerate((63, 64)):
        i = r.info[1][65 * w]
        assert (i.kind, i.leader, i.n_members, i.n_actor_candidates, float(i.g)) == ("actor", 65 * w + p, 65, 64, 5.0)
    for a in (0, 63, 64, 65, 129):
        _same_in_every_member(r, 1, a)


def _kat_window_of_120_vertices(dm, run):
    # 4a.  A 0.5 m track, look = 60, the vehicle at s = 0.25: i0 = 0, vertex k has g = 0.5 k - 0.25, so the window has 120 vertices - more
    # than 64.  One world per k*: member 1's ego on vertex k* (member 0 far away) - the first, both sides of the 64th, the last; and
    # on vertex 121, the first one OUTSIDE the window, which is seen from vertex 120 (d2 = 0.25).
    ks = [1, 64, 65, 120]
    worlds = [dict(egos=[FAR, (0.5 * k, 0.0, 0.0, False)], actors=[(0.25, 3.0, 0, 0, 0.5)]) for k in ks + [121]]
    r = run([(straight(dm, 201, step=0.5), False)], worlds)
    for a, k in enumerate(ks):
        i = r.info[1][a]
        assert (i.kind, i.window, i.kstar, float(i.d2), float(i.g), i.ego_scene) == ("ego", 120, k, 0.0, 0.5 * k - 0.25, 2 * a + 1), k
    i = r.info[1][len(ks)]
    assert (i.kind, i.window, i.kstar, float(i.d2), float(i.g)) == ("ego", 120, 120, 0.25, 59.75)


def _kat_window_wraps_and_ends(dm, run):
    # 4b.  The closed square (n = 40, L = 40), the vehicle at s = 37.5: i0 = 37; k = 2 is P[39] (g = 1.5), k = 3 is P[0] (g = 2.5), k = 4 is P[1]
    # (g = 3.5): the window wraps past vertex n - 1.  World 0: member 1's ego on P[1].  World 1: member 0's ego on P[1], member 1's on
    # P[39]: the higher scene is nearer and leads.  World 2: an open track of 11 points, the vehicle at s = 7.5: the window ends at the
    # track's end with 3 vertices although look = 60; member 1's ego on the last vertex: k* = 3, g = 2.5.
    sq = square(dm)
    on = lambda j: (float(sq["x"][j]), float(sq["y"][j]), 0.0, False)
    worlds = [dict(egos=[FAR, on(1)], actors=[(37.5, 3.0, 0, 0, 0.5)]), dict(egos=[on(1), on(39)], actors=[(37.5, 3.0, 0, 0, 0.5)]),
              dict(egos=[FAR, (10.0, 0.0, 0.0, False)], actors=[(7.5, 3.0, 1, 0, 0.5)])]
    r = run([(sq, True), (straight(dm, 11), False)], worlds)
    i = r.info[1]
    assert (i[0].kind, i[0].window, i[0].kstar, float(i[0].g), i[0].ego_scene) == ("ego", 40, 4, 3.5, 1)
    assert (i[1].kind, i[1].kstar, float(i[1].g), i[1].ego_scene, i[1].ego_candidates) == ("ego", 2, 1.5, 3, [2, 3])
    assert (i[2].kind, i[2].window, i[2].kstar, float(i[2].g), i[2].ego_scene) == ("ego", 3, 3, 2.5, 5)


def _kat_world_borders(dm, run):
    # 5.  Two worlds on ONE track.  World 0 (scenes 0, 1): its vehicle at s = 7.5; member 1's ego on vertex 40 (g = 32.5).  World 1 (scenes
    # 2, 3): the ego of scene 2 - the first scene beyond world_first[1] - stands on vertex 10, directly in front of world 0's vehicle,
    # and world 1's parked vehicle at s = 9 stands nearer still: world 0's vehicle sees neither (its group has one member, its
    # candidates are scene 1 alone).  World 1's follower at s = 2 is led by its world's parked vehicle (g = 7; its ego, g = 8, is
    # further) and does not see world 0's vehicle at 7.5 (g = 5.5).
    worlds = [dict(egos=[FAR, (40.0, 0.0, 0.0, False)], actors=[(7.5, 4.0, 0, 0, 0.5)]),
              dict(egos=[(10.0, 0.0, 0.0, False), FAR], actors=[(9.0, 0.0, 0, 1, 0.5), (2.0, 4.0, 0, 2, 0.5)])]
    r = run([(straight(dm, 101), False)], worlds)
    i = r.info[1]
    assert (i[0].kind, i[0].ego_scene, i[0].ego_candidates, i[0].n_members, float(i[0].g), i[0].n_world) == ("ego", 1, [1], 1, 32.5, 2)
    assert i[1].kind == "plain"
    assert (i[2].kind, i[2].leader, float(i[2].g), float(i[2].ego_g), i[2].ego_scene, i[2].n_members) == ("actor", 1, 7.0, 8.0, 2, 2)


def _kat_flagged_ego_in_another_scene(dm, run):
    # 6.  Member 1's ego on vertex 20 at 14.4 km/h, FLAGGED (frozen): it leads with vl = 0 whatever its velocity, dv = 4; world 1 is the same
    # unflagged: vl = 4.
    worlds = [dict(egos=[FAR, (20.0, 0.0, 14.4, flagged)], actors=[(7.5, 4.0, 0, 0, 0.5)]) for flagged in (True, False)]
    r = run([(straight(dm, 101), False)], worlds)
    a, b = r.info[1]
    assert (a.kind, a.ego_scene, float(a.g), float(a.vl)) == ("ego", 1, 12.5, 0.0) and (b.kind, b.ego_scene, float(b.vl), float(b.dyn)) == ("ego", 3, 4.0, 6.0)
    assert float(a.dyn) == 4.0 * 1.5 + (4.0 * 4.0) / (2 * np.sqrt(1.0 * 2.0)) and r.v[1][0] < r.v[1][1] < 4.0


def _kat_slots_and_pools(dm, run):
    # 7.  Three members with 2, 4 and 3 own entries, 1, 0 and 2 unpinned entries behind their slices and K = 2 peer slots each, so every
    # obs_off differs; a motion pool.  Two vehicles own slots 0 and 1.  Egos on vertices 20, 35 and 200: the first two are each other's
    # peers (range 60), the third has none.  The vehicles' entries are identical in every member and carry a zero ObMotion; the own
    # entries beyond slot 1, the unpinned entries, the unused peer slots and all their motions keep the 0xA5 fill; the traffic
    # kernel leaves the peer slots alone and k_couple_fleet fills them as before.
    egos = [(20.0, 0.0, 14.4, False), (35.0, 0.0, 14.4, False), (200.0, 0.0, 0.0, False)]
    r = run([(straight(dm, 301), False)], [dict(egos=egos, actors=[(7.5, 4.0, 0, 3, 0.5), (2.0, 4.0, 0, 4, 0.75)], own=[2, 4, 3], pad=[1, 0, 2])], motion=True, K=2)
    lay = r.layout
    assert lay.off.tolist() == [0, 5, 11] and lay.total == 18
    assert (r.info[1][0].kind, r.info[1][0].ego_scene, r.info[1][1].kind, r.info[1][1].leader) == ("ego", 0, "actor", 0)
    for stage in (0, 1, 2):
        pool, mot = r.pool[stage], r.mot[stage]
        pinned = {int(e) for a in (0, 1) for e in lay.entries[a]}
        assert pinned == {0, 1, 5, 6, 11, 12}
        peers = {2: 1, 9: 0}                                     # member 0 sees scene 1, member 1 sees scene 0; member 2 (entries 14, 15) nobody
        for e in range(lay.total):
            if e in pinned:
                assert mot[e].tobytes() == bytes(16), (stage, e)
            elif e in peers:
                assert int(pool[e]["type"]) == (fl.OB_PEER | peers[e]) and mot[e].tobytes() == bytes(16), (stage, e)
            else:
                assert pool[e].tobytes() == FILL_OB and mot[e].tobytes() == FILL_MOT, (stage, e)
        for a in (0, 1):
            _same_in_every_member(r, stage, a)
        assert [len(x) for x in r.slices[stage]] == [3, 5, 3]


def _kat_parked_and_reversing(dm, run):
    # 8.  Vehicles with !(speed > 0) in a world of three scenes, an ego right in front of them: §4h's step, written to all members, v = speed.
    rows = [(1.0, -3.0, 0, 1, 0.5), (50.0, 0.0, 0, 2, 0.5), (0.5, -3.0, 1, 3, 0.5), (39.0, 0.0, 1, 4, 0.5), (2.0, -0.0, 0, 5, 0.5)]
    polylines = [(straight(dm, 101), False), (square(dm), True)]
    r = run(polylines, [dict(egos=[FAR, (3.0, 0.0, 0.0, False), FAR], actors=rows)], steps=3)
    tracks, pts = ts.pack(dm, polylines)
    plain = tm.Traffic(tracks, pts, ts.actors(dm, [(x[0], x[1], 0, k, x[2], x[3], x[4]) for k, x in enumerate(rows)]), np.zeros(1, np.int64))
    pool, _ = plain.place(np.zeros(len(rows), dm.ObPoint), None, 0.0)
    for k in range(1, 4):
        pool, _ = plain.place(pool, None, 0.5)
        assert r.s[k].tobytes() == plain.s.tobytes() and r.v[k].tolist() == [x[1] for x in rows] and all(i.kind == "plain" for i in r.info[k])
        for m in range(3):
            assert r.slices[k][m].tobytes() == pool.tobytes(), (k, m)


def _kat_following_off(dm, run):
    # Following never set: the vehicles of a world drive at constant speed through everything (k_move_world_traffic with step = dt), in every member.
    r = run([(straight(dm, 101), False), (square(dm), True)],
            [dict(egos=[(20.0, 0.0, 0.0, False)] * 3, actors=[(7.5, 4.0, 0, 1, 0.5), (38.0, 3.0, 1, 2, 0.5)]), dict(egos=[FAR] * 65, actors=[(99.0, 4.0, 0, 1, 0.5)])],
            steps=3, follow=False)
    assert [r.at(k, 0)[0] for k in range(4)] == [7.5, 9.5, 11.5, 13.5] and [r.at(k, 1)[0] for k in range(4)] == [38.0, 39.5, 1.0, 2.5]
    assert [r.at(k, 2)[0] for k in range(4)] == [99.0, 100.0, 100.0, 100.0]
    for a in range(3):
        _same_in_every_member(r, 3, a)


CASES = [_kat_leader_lives_in_the_other_scene, _kat_tie_neighbouring_lanes, _kat_tie_64_members_apart, _kat_tie_ego_wins_against_an_actor,
         _kat_stride_edges_of_the_members, _kat_group_of_65, _kat_window_of_120_vertices, _kat_window_wraps_and_ends, _kat_world_borders,
         _kat_flagged_ego_in_another_scene, _kat_slots_and_pools, _kat_parked_and_reversing, _kat_following_off]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_case_on_the_model(dm, case):
    case(dm, _runner(dm, "model"))


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_case_on_the_device(dm, case):
    """The known answers on k_move_world_traffic / k_follow_world_traffic, each also held byte for byte against the model."""
    case(dm, _runner(dm, "device"))


_LOG = []


def _case_log(dm):
    if not _LOG:
        run = _runner(dm, "model", _LOG)
        for case in CASES:
            case(dm, run)
    return _LOG


def test_cases_batched_on_the_model(dm):
    """Every case as worlds of one launch per (model, dt, steps, follow, motion, K): the worlds do not disturb each other."""
    launches, largest = wb.batched(dm, wb.ModelBackend(), _case_log(dm))
    assert launches >= 4 and largest >= 130


@gpu
def test_cases_batched_on_the_device(dm):
    launches, largest = wb.batched(dm, wb.DeviceBackend(), _case_log(dm))
    assert launches >= 4 and largest >= 130


def test_nan_ego_position_on_the_model(dm):
    """6., model only (see the module docstring): a NaN ego position in a member scene is no candidate - every d2 is NaN, and a NaN is
    never the minimum -, so the other member's ego leads; a world whose only ego is NaN leaves the road free."""
    run = _runner(dm, "model")
    r = run([(straight(dm, 101), False)], [dict(egos=[(np.nan, 0.0, 0.0, False), (20.0, 0.0, 14.4, False)], actors=[(7.5, 4.0, 0, 0, 0.5)]),
                                          dict(egos=[(20.0, np.nan, 0.0, False)], actors=[(7.5, 4.0, 0, 0, 0.5)])])
    a, b = r.info[1]
    assert (a.kind, a.ego_scene, a.ego_candidates, float(a.vl)) == ("ego", 1, [1], 4.0) and (b.kind, b.ego_candidates, b.window) == ("free", [], 60)


# ---- worlds of one scene = scene traffic (10.) ---------------------------------------------------------------------------------------
ONE_STEPS = 40


def _ones(dm):
    """Six scenes, each a world of its own, three vehicles each on an open and a closed track, egos on and off the tracks."""
    sq = square(dm)
    polylines = [(straight(dm, 101), False), (sq, True)]
    egos = [(20.0, 0.0, 14.4, False), FAR, (float(sq["x"][5]), float(sq["y"][5]), 3.6, False), (60.0, 1.0, 7.2, True), (10.0, 4.0, 0.0, False), (35.0, -1.5, 10.8, False)]
    scenes = []
    for c, e in enumerate(egos):
        scenes.append(dict(ego=e, actors=[(2.0 + c, 6.0, 0, 10 + c, 0.5), (30.0 + 3 * c, 1.5, c % 2, 20 + c, 0.75), (7.0 * c, 3.0 if c % 3 else -1.0, 1, 30 + c, 0.5)]))
    return polylines, scenes


@pytest.mark.parametrize("follow", [False, True], ids=["move", "follow"])
def test_worlds_of_one_equal_scene_traffic_on_the_model(dm, follow):
    """The corollary of §4j: the same tracks and actor records through §4h / §4i's models and through the world model with one-scene
    worlds, 40 advances: s, v and the pools are byte-identical."""
    polylines, scenes = _ones(dm)
    r = wb.ModelBackend().run(dm, polylines, [dict(egos=[sc["ego"]], actors=sc["actors"]) for sc in scenes], fm.params(None), 0.5, ONE_STEPS, follow=follow)
    tracks, pts = ts.pack(dm, polylines)
    tr = fm.Follow(tracks, pts, r.layout.act, r.layout.off)          # (worlds of one: the world index IS the scene index)
    si, flags = fb._egos(dm, scenes)
    pool, _ = tr.place(r.layout.filled(dm.ObPoint), None, 0.0)
    kinds = set()
    for k in range(ONE_STEPS + 1):
        if k > 0:
            pool, _ = tr.step(pool, None, 0.5, None, si, flags, 1.8) if follow else tr.place(pool, None, 0.5)
            kinds |= {i.kind for i in tr.info} if follow else set()
        assert r.s[k].tobytes() == tr.s.tobytes() and r.pool[k].tobytes() == pool.tobytes(), k
        assert not follow or r.v[k].tobytes() == tr.v.tobytes(), k
    assert not follow or kinds == {"ego", "actor", "free", "plain"}


def _one_on_the_device(dm, polylines, scenes, follow, world):
    """As wb.DeviceBackend with one-scene worlds, the traffic set through pp_set_world_traffic or - the same records - pp_set_traffic."""
    lay = wb.Layout(dm, [dict(egos=[sc["ego"]], actors=sc["actors"]) for sc in scenes], 0)
    tracks, pts = ts.pack(dm, polylines)
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    sc = dm.gen_scenes(cfg, 0, lay.n, 1, junction_every=0)
    si = sc["scene_in"]
    si["obs_off"], si["obs_n"] = lay.off, lay.own
    for f in ("x", "y"):
        si["loc"]["globalpoint"][f] = lay.si["loc"]["globalpoint"][f]
    si["loc"]["velocity"] = lay.si["loc"]["velocity"]
    pl = dm.Planner(cfg, device=0, max_scenes=lay.n, max_obs_total=lay.total)
    wb.set_scenes(pl, sc, si, lay.filled(dm.ObPoint), None, lay.total)
    pl.set_state(sc["state"])
    pl.set_fleet(lay.world_first, lay.fm)
    (pl.set_world_traffic if world else pl.set_traffic)(tracks, pts, lay.act)
    if follow:
        pl.set_traffic_follow(dm.default_traffic_follow())
    model = dm.default_ego_model()
    model["dt"], model["window"] = 0.5, 1
    po = fb.staging_plan(dm, lay.egos, 0.5)
    out = []
    for k in range(ONE_STEPS + 1):
        if k > 0:
            pl.tick()
            st = pl.get_state()
            st["afresh_planning"] = 1
            pl.write_device(dm.BUF_PLAN_OUT, po)
            pl.write_device(dm.BUF_STATE, st)
            pl.advance_async(model)
        out.append((pl.traffic_state(), pl.traffic_speed() if follow else None, np.concatenate([pl.get_obstacles(c, cap=3) for c in range(lay.n)])))
    pl.close()
    return lay, out


@gpu
@pytest.mark.parametrize("follow", [False, True], ids=["move", "follow"])
def test_worlds_of_one_equal_scene_traffic_on_the_device(dm, follow):
    """The same records through pp_set_traffic and through pp_set_world_traffic with one-scene worlds, 40 advances: s, v and every
    scene's slice are byte-identical, and they are the model's."""
    polylines, scenes = _ones(dm)
    lay, shared = _one_on_the_device(dm, polylines, scenes, follow, True)
    _, copies = _one_on_the_device(dm, polylines, scenes, follow, False)
    want = wb.ModelBackend().run(dm, polylines, [dict(egos=[sc["ego"]], actors=sc["actors"]) for sc in scenes], fm.params(None), 0.5, ONE_STEPS, follow=follow)
    for k in range(ONE_STEPS + 1):
        assert shared[k][0].tobytes() == copies[k][0].tobytes() == want.s[k].tobytes(), f"stage {k}: s"
        assert shared[k][2].tobytes() == copies[k][2].tobytes() == want.pool[k].tobytes(), f"stage {k}: slices"
        assert not follow or shared[k][1].tobytes() == copies[k][1].tobytes() == want.v[k].tobytes(), f"stage {k}: v"


# ---- pp_update_async (9.) and the life cycle (11.) -------------------------------------------------------------------------------------
def _life_scene(dm, K=0):
    """Two worlds of 3 and 2 scenes on one open track; 2 own entries per scene (scene 3: one more) and one unpinned entry behind every slice."""
    polylines = [(straight(dm, 101), False)]
    worlds = [dict(egos=[(20.0, 0.0, 14.4, False), (35.0, 0.0, 14.4, False), FAR], actors=[(7.5, 4.0, 0, 3, 0.5), (2.0, 5.0, 0, 4, 0.5)], pad=[1, 1, 1]),
              dict(egos=[(50.0, 0.0, 7.2, False), FAR], actors=[(30.0, 6.0, 0, 5, 0.5)], own=[3, 2], pad=[1, 1])]
    return polylines, worlds, wb.Layout(dm, worlds, K)


def _life_planner(dm, lay, motion=False):
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    sc = dm.gen_scenes(cfg, 0, lay.n, 1, junction_every=0)
    si = sc["scene_in"]
    si["obs_off"], si["obs_n"] = lay.off, lay.own
    for f in ("x", "y"):
        si["loc"]["globalpoint"][f] = lay.si["loc"]["globalpoint"][f]
    si["loc"]["velocity"] = lay.si["loc"]["velocity"]
    pl = dm.Planner(cfg, device=0, max_scenes=lay.n, max_obs_total=lay.total)
    wb.set_scenes(pl, sc, si, lay.filled(dm.ObPoint), lay.filled(dm.ObMotion) if motion else None, lay.total)
    pl.set_state(sc["state"])
    return pl, cfg, sc, si


def _advance(dm, pl, lay, dt=0.5):
    model = dm.default_ego_model()
    model["dt"], model["window"] = dt, 1
    pl.tick()
    st = pl.get_state()
    st["afresh_planning"] = 1
    pl.write_device(dm.BUF_PLAN_OUT, fb.staging_plan(dm, lay.egos, dt))
    pl.write_device(dm.BUF_STATE, st)
    pl.advance_async(model)


def test_place_with_no_step_leaves_s_on_the_model(dm):
    """9., model: placing at the current s (pp_update_async) changes no s and writes every member's entry into a fresh pool."""
    polylines, worlds, lay = _life_scene(dm)
    tracks, pts = ts.pack(dm, polylines)
    tr = wm.World(tracks, pts, lay.act, lay.world_first, lay.off, lay.own)
    pool, _ = tr.place(lay.filled(dm.ObPoint), None, 0.0)
    for _ in range(3):
        pool, _ = tr.step(pool, None, 0.5, None, lay.si, lay.flags, 1.8)
    s, v = tr.s.copy(), tr.v.copy()
    fresh, _ = tr.place(lay.filled(dm.ObPoint), None, 0.0)
    assert tr.s.tobytes() == s.tobytes() and tr.v.tobytes() == v.tobytes() and fresh.tobytes() == pool.tobytes()


@gpu
def test_update_async_places_every_member(dm):
    """9.  After three following advances a caller-uploaded pool comes out with the vehicles at the current s in EVERY member scene, s and
    v are what they were, every other entry is the caller's; a pool that stops short of the last pinned entry is refused."""
    polylines, worlds, lay = _life_scene(dm)
    tracks, pts = ts.pack(dm, polylines)
    pl, cfg, sc, si = _life_planner(dm, lay)
    pl.set_fleet(lay.world_first, lay.fm)
    pl.set_world_traffic(tracks, pts, lay.act)
    pl.set_traffic_follow(dm.default_traffic_follow())
    tr = wm.World(tracks, pts, lay.act, lay.world_first, lay.off, lay.own)
    want, _ = tr.place(lay.filled(dm.ObPoint), None, 0.0)
    for _ in range(3):
        _advance(dm, pl, lay)
        want, _ = tr.step(want, None, 0.5, None, pl.get_scene_in(), pl.ego_flags(), float(cfg["Vehicle_Width"][0]))
    pl.tick()
    s_now, v_now = tr.s.copy(), tr.v.copy()
    assert pl.traffic_state().tobytes() == s_now.tobytes() and pl.traffic_speed().tobytes() == v_now.tobytes() and (v_now != lay.act["speed"]).any()
    last = max(int(e.max()) for e in lay.entries)                # the last pinned entry: slot 0 of scene 4
    assert last == lay.total - 3
    short = dm.pinned_copy(np.frombuffer(bytes([0x5A]) * (last * dm.ObPoint.itemsize), dm.ObPoint))
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.update_async(obs_pool=short)
    up = dm.pinned_copy(np.frombuffer(bytes([0x5A]) * (lay.total * dm.ObPoint.itemsize), dm.ObPoint))
    pl.update_async(obs_pool=up)
    assert pl.traffic_state().tobytes() == s_now.tobytes() and pl.traffic_speed().tobytes() == v_now.tobytes()
    pl.tick()
    want, _ = tr.place(np.array(up), None, 0.0)
    assert tr.s.tobytes() == s_now.tobytes()
    assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, lay.total).tobytes() == want.tobytes()
    pl.close()


@gpu
def test_errors_and_life_cycle(dm):
    """11.  Every PP_ERR_* of pp_set_world_traffic with nothing changed after the failure; replace semantics between the two set calls;
    off after a successful pp_set_fleet (n_worlds = 0 included) and not after a refused one; following set before and after the traffic."""
    polylines, worlds, lay = _life_scene(dm, K=1)
    tracks, pts = ts.pack(dm, polylines)
    act, tf = lay.act, dm.default_traffic_follow()
    pl, cfg, sc, si = _life_planner(dm, lay)
    width = float(cfg["Vehicle_Width"][0])
    pool = lambda: pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, lay.total)
    assert hasattr(pl.lib, "pp_set_world_traffic")
    # PP_ERR_STATE: no fleet
    with pytest.raises(dm.PlannerError, match="error -4:.*no fleet"):
        pl.set_world_traffic(tracks, pts, act)
    assert pool().tobytes() == lay.filled(dm.ObPoint).tobytes()
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_state()
    pl.set_world_traffic(None, None, None)                       # n_actors = 0 needs no fleet: off is off
    pl.set_fleet(lay.world_first, lay.fm)
    pl.set_traffic_follow(tf)                                    # following BEFORE the traffic: the set call sets v = speed
    pl.set_world_traffic(tracks, pts, act)
    tr = wm.World(tracks, pts, act, lay.world_first, lay.off, lay.own)
    want, _ = tr.place(fl.couple(lay.fm, lay.world_first, lay.off, lay.own, si, lay.filled(dm.ObPoint))[1], None, 0.0)
    assert pool().tobytes() == want.tobytes() and pl.traffic_speed().tobytes() == np.ascontiguousarray(act["speed"]).tobytes()

    def refused(code, tracks=tracks, pts=pts, act=act, match=""):
        with pytest.raises(dm.PlannerError, match=f"error {code}:.*{match}"):
            pl.set_world_traffic(tracks, pts, act)
        assert pl.traffic_state().tobytes() == tr.s.tobytes() and pool().tobytes() == want.tobytes()

    def changed(**kw):
        a = act.copy()
        for k, (row, val) in kw.items():
            a[k][row] = val
        return a

    # PP_ERR_ARG: what §4h checks ...
    for a in (changed(s0=(0, np.nan)), changed(speed=(1, np.inf)), changed(radius=(2, -1.0)), changed(radius=(0, np.nan)), changed(track=(0, 1)), changed(track=(0, -1))):
        refused(-1, act=a)
    t2 = tracks.copy(); t2["n_points"] = 1
    refused(-1, tracks=t2)
    t2 = tracks.copy(); t2["point_off"] = 1
    refused(-1, tracks=t2)
    p2 = pts.copy(); p2["x"][3] = np.nan
    refused(-1, pts=p2)
    p2 = pts.copy(); p2["x"], p2["y"] = 1.0, 1.0
    t2 = tracks.copy(); t2["closed"] = 1
    refused(-1, tracks=t2, pts=p2)
    # ... a world out of range, a slot that is not an own entry of SOME member (scene 4 has 2: slot 2 is one of scene 3's only), a duplicate
    refused(-1, act=changed(scene=(0, 2)), match="world")
    refused(-1, act=changed(scene=(0, -1)), match="world")
    refused(-1, act=changed(slot=(2, 2)), match="scene 4")
    refused(-1, act=changed(slot=(0, 2)), match="scene 0")
    refused(-1, act=changed(slot=(0, -1)), match="scene 0")
    refused(-1, act=changed(slot=(1, 0)), match="two actors on slot 0 of world 0")
    # PP_ERR_STATE: an update staged
    _advance(dm, pl, lay)
    want, _ = tr.step(want, None, 0.5, tf, pl.get_scene_in(), pl.ego_flags(), width)
    want = fl.couple(lay.fm, lay.world_first, lay.off, lay.own, lay.scene_in(pl.get_scene_in()), want)[1]
    with pytest.raises(dm.PlannerError, match="error -4:.*staged"):
        pl.set_world_traffic(tracks, pts, act)
    with pytest.raises(dm.PlannerError, match="error -4:.*staged"):
        pl.set_world_traffic(None, None, None)
    pl.tick()
    assert pl.traffic_state().tobytes() == tr.s.tobytes() and pl.traffic_speed().tobytes() == tr.v.tobytes() and pool().tobytes() == want.tobytes()
    assert any(i.kind == "ego" and i.ego_scene == 0 for i in tr.info)
    # a refused pp_set_fleet changes nothing; a successful one switches world traffic off - the entries keep the last pose
    bad = lay.fm.copy(); bad["range"] = -1.0
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_fleet(lay.world_first, bad)
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_fleet(np.array([0, 3, 3, 5], np.int32), lay.fm)
    assert pl.traffic_state().tobytes() == tr.s.tobytes()
    pl.set_fleet(lay.world_first, lay.fm)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_state()
    assert pool().tobytes() == want.tobytes()
    pl.set_world_traffic(tracks, pts, act)                       # on again (following is still on: v = speed), then fleet off
    assert pl.traffic_speed().tobytes() == np.ascontiguousarray(act["speed"]).tobytes()
    pl.set_fleet(None)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_state()
    with pytest.raises(dm.PlannerError, match="error -4:.*no fleet"):
        pl.set_world_traffic(tracks, pts, act)
    # replace semantics: scene traffic, then world traffic, then scene traffic again; scene traffic survives pp_set_fleet
    pl.set_traffic_follow(None)
    per_scene = ts.actors(dm, [(11.0, 2.0, 4, 1, 0, 9, 0.25)])
    pl.set_traffic(tracks, pts, per_scene)
    assert pl.traffic_state().tolist() == [11.0]
    pl.set_fleet(lay.world_first, lay.fm)
    assert pl.traffic_state().tolist() == [11.0]                 # (per-scene traffic keeps its relation to pp_set_fleet)
    pl.set_world_traffic(tracks, pts, act)
    assert pl.traffic_state().tobytes() == np.ascontiguousarray(act["s0"]).tobytes()
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_speed()
    pl.set_traffic_follow(tf)                                    # following AFTER the traffic: v = speed, grouped by (world, track)
    assert pl.traffic_speed().tobytes() == np.ascontiguousarray(act["speed"]).tobytes()
    tr = wm.World(tracks, pts, act, lay.world_first, lay.off, lay.own)
    want, _ = tr.place(pool(), None, 0.0)
    assert pool().tobytes() == want.tobytes()
    for _ in range(2):
        _advance(dm, pl, lay)
        want, _ = tr.step(want, None, 0.5, tf, pl.get_scene_in(), pl.ego_flags(), width)
        want = fl.couple(lay.fm, lay.world_first, lay.off, lay.own, lay.scene_in(pl.get_scene_in()), want)[1]
        assert pl.traffic_state().tobytes() == tr.s.tobytes() and pl.traffic_speed().tobytes() == tr.v.tobytes()
    pl.tick()
    assert pool().tobytes() == want.tobytes()
    assert tr.info[1].kind == "actor" and tr.info[1].leader == 0
    pl.set_traffic(tracks, pts, per_scene)                       # replaces the world traffic: one vehicle again, stepped per scene
    assert pl.traffic_state().tolist() == [11.0] and pl.traffic_speed().tolist() == [2.0]
    pl.set_traffic(None, None, None)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_state()
    # pp_set_scenes switches it off, as it does scene traffic and the fleet
    pl.set_world_traffic(tracks, pts, act)
    wb.set_scenes(pl, sc, si, lay.filled(dm.ObPoint), None, lay.total)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_state()
    with pytest.raises(dm.PlannerError, match="error -4:.*no fleet"):
        pl.set_world_traffic(tracks, pts, act)
    pl.close()
    # no resident scenes
    pl = dm.Planner(cfg, device=0, max_scenes=4, max_obs_total=8)
    with pytest.raises(dm.PlannerError, match="error -4:.*no resident scenes"):
        pl.set_world_traffic(tracks, pts, act)
    pl.close()


# ---- platoons on the ring (12., 13.) ---------------------------------------------------------------------------------------------------
P_GAP_PTS, P_BEHIND, P_SPEED, P_RADIUS, P_TYPE, P_K, P_TICKS = 30, 12.0, 6.0, 0.9, 7, 4, 300
_CPU = {}


def _platoons(dm, cfg, m, leaders, size, n_own, K, seed=3):
    """`leaders` ring egos (tests/test_traffic_follow.py's scene A: lanes 1 / 2, 120 .. 170 points into their first road, the starts on
    lane 2 of the two-lane road 3 left out), each followed by size - 1 copies of itself P_GAP_PTS points (15 m) further back on its lane:
    scene w * size + j is member j of world w, member 0 in front.  Every scene owns n_own obstacle entries and K peer slots behind them.
    Returns (sc, legs, route_first, world_first, off, the polylines of the two ring tracks, rows of (world, lane, arc length of the rear ego))."""
    sc, legs, rf = rs.make_egos(dm, cfg, m, 4 * leaders, seed=seed, lanes=(1, 2), ids=(120, 170), legs=(6, 10), n_obs=0)
    loc = sc["scene_in"]["loc"]
    keep = np.flatnonzero(~((loc["road_num"] == 3) & (loc["lane_num"] == 2)))[:leaders]
    assert len(keep) == leaders
    idx = np.repeat(keep, size)
    n = len(idx)
    si, st = sc["scene_in"][idx].copy(), sc["state"][idx].copy()
    legs2 = np.concatenate([legs[rf[k]:rf[k + 1]] for k in idx])
    rf2 = np.concatenate([[0], np.cumsum([rf[k + 1] - rf[k] for k in idx])]).astype(np.int32)
    polylines = [(ts.ring_track(dm, m, 1), True), (ts.ring_track(dm, m, 2), True)]
    S = float(cfg["grid_w"][0]) * float(cfg["cell"][0])
    rows = []
    for s in range(n):
        j, l = s % size, si["loc"][s]
        road, lane, pid = int(l["road_num"]), int(l["lane_num"]), int(l["id"][0]) - P_GAP_PTS * (s % size)
        L = m["lanes"][m["road_first_lane"][road - 1] + lane - 1]
        p = m["points"][int(L["point_off"]) + pid]
        l["id"][:] = pid
        l["globalpoint"]["x"], l["globalpoint"]["y"], l["globalpoint"]["dir"] = p["x"], p["y"], p["dir"]
        si["grid_origin"][s]["x"], si["grid_origin"][s]["y"] = float(p["x"]) - 0.5 * S, float(p["y"]) - 0.5 * S
        if j == size - 1:
            q = polylines[lane - 1][0]
            rows.append((s // size, lane, tm.cumulative(q["x"], q["y"], True)[ts.SEG * (road - 1) + pid]))
    stride = n_own + K
    off = np.arange(n, dtype=np.int64) * stride
    si["obs_off"], si["obs_n"] = off, n_own
    pool = np.zeros(n * stride, dm.ObPoint)
    pool["x"], pool["y"], pool["radius"], pool["type"] = -500.0, -500.0, 0.5, 1
    sc = dict(sc, scene_in=si, state=st, obs_pool=pool, mot_pool=None, n_obs=stride)
    return sc, legs2, rf2, np.arange(leaders + 1, dtype=np.int32) * size, off, polylines, rows


def _platoon_loop(dm, oracle, shared):
    """12.  One world of two ring egos 15 m apart, one vehicle 12 m behind the REAR ego (member 1) that wants 6 m/s; oracle tick + route model
    + follow / world model + fleet model.  shared: one vehicle of the world; otherwise one per-scene copy (§4i) in every member."""
    import map_scenes as ms
    import rollout_score_model as sm
    import route_model as rmod
    if shared in _CPU:
        return _CPU[shared]
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf, wf, off, polylines, rows = _platoons(dm, cfg, m, 1, 2, 1, P_K)
    fmod = dm.default_fleet_model()
    fmod["max_peers"] = P_K
    tracks, pts = ts.pack(dm, polylines)
    (w, lane, here), own = rows[0], np.ones(2, np.int64)
    if shared:
        tr = wm.World(tracks, pts, ts.actors(dm, [(here - P_BEHIND, P_SPEED, 0, 0, lane - 1, P_TYPE, P_RADIUS)]), wf, off, own)
    else:
        tr = fm.Follow(tracks, pts, ts.actors(dm, [(here - P_BEHIND, P_SPEED, c, 0, lane - 1, P_TYPE, P_RADIUS) for c in (0, 1)]), off)
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt, width = float(model["dt"][0]), float(cfg["Vehicle_Width"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"].copy()), sc["state"].copy(), np.zeros(2, np.int32)
    si, obs, _ = fl.couple(fmod, wf, off, own, si, sc["obs_pool"].copy())
    obs, _ = tr.place(obs, None, 0.0)
    scores, leaders, ss = sm.new_scores(dm.RolloutScore, 2), [], [tr.s.copy()]
    for t in range(P_TICKS + 1):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=2, want_grid=False)
        sm.fold(scores, cfg, dt, si, plan, st, obs, flags)
        if t < P_TICKS:
            si, flags, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
            obs, _ = tr.step(obs, None, dt, None, si, flags, width)
            leaders.append([(i.kind, getattr(i, "ego_scene", None)) for i in tr.info])
            si, obs, _ = fl.couple(fmod, wf, off, own, si, obs)
            ss.append(tr.s.copy())
    _CPU[shared] = dict(scores=scores, leaders=leaders, s=ss, flags=flags, L=tr.length(lane - 1), obs=obs, si=si)
    return _CPU[shared]


def test_platoon_closed_loop_on_the_cpu(dm, oracle):
    """12.  A platoon of two ring egos in one world and one faster vehicle behind the rear ego, 301 scored ticks.  Shared: no ego's scorecard
    has a collision tick and the vehicle's leader is the rear ego (scene 1) on every step.  Control, one per-scene copy in every member:
    the copy in the front ego's scene sees only the front ego, 15 m further on, so the copies have different leaders from the first
    step and their arc lengths differ at the end - the scenes of the world disagree about where the vehicle is."""
    sh, cp = _platoon_loop(dm, oracle, True), _platoon_loop(dm, oracle, False)
    d = np.abs(np.array([s[0] - s[1] for s in cp["s"]]))
    d = np.minimum(d, cp["L"] - d)
    print("shared: collision ticks", sh["scores"]["n_collision_ticks"].tolist(), "min clearance", np.round(sh["scores"]["min_clearance"], 2).tolist(),
          "ego dist", np.round(sh["scores"]["dist"], 1).tolist(), "vehicle dist", round(float(sh["s"][-1][0] - sh["s"][0][0]), 1),
          "\ncopies: largest difference of s", round(float(d.max()), 2), "at the end", round(float(d[-1]), 2), "collision ticks", cp["scores"]["n_collision_ticks"].tolist(),
          "min clearance", np.round(cp["scores"]["min_clearance"], 2).tolist())
    assert (sh["scores"]["n_collision_ticks"] == 0).all() and (sh["scores"]["first_collision_tick"] == -1).all() and not sh["flags"].any()
    assert all(x == [("ego", 1)] for x in sh["leaders"]) and len(sh["leaders"]) == P_TICKS
    assert cp["leaders"][0] == [("ego", None), ("ego", None)] and cp["s"][1][0] != cp["s"][1][1]          # different leaders from the first step
    assert cp["s"][-1][0] != cp["s"][-1][1]


R_W, R_SIZE, R_OWN, R_K, R_TICKS = 8, 4, 3, 3, 60


@gpu
def test_step_check_on_a_routed_fleet_rollout(dm):
    """13.  32 routed ring egos in 8 worlds of 4 (platoons, 15 m apart), two vehicles per world - one 12 m behind the rear ego and faster, one
    25 m ahead of the front ego and slow -, 60 advances with route + fleet + follow.  After every advance the model, fed the SceneIn
    records and flag words the device staged, gives s, v and every scene's slice - own entries and peers - byte for byte."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf, wf, off, polylines, rows = _platoons(dm, cfg, m, R_W, R_SIZE, R_OWN, R_K, seed=5)
    n, own = R_W * R_SIZE, np.full(R_W * R_SIZE, R_OWN, np.int64)
    tracks, pts = ts.pack(dm, polylines)
    rng = np.random.default_rng(5)
    act = []
    for w, lane, here in rows:
        act.append((here - P_BEHIND, rng.choice([4.0, 6.0, 9.0]), w, 1, lane - 1, 100 + w, 0.9))
        act.append((here + 15.0 * (R_SIZE - 1) + 25.0, rng.choice([0.0, 1.5, 2.5]), w, 2, lane - 1, 200 + w, 0.9))
    act = ts.actors(dm, act)
    fmod = dm.default_fleet_model()
    fmod["max_peers"] = R_K
    model, tf = dm.default_ego_model(), dm.default_traffic_follow()
    dt, width = float(model["dt"][0]), float(cfg["Vehicle_Width"][0])
    pl = dm.Planner(cfg, device=0, **rs.caps(m, n, R_OWN + R_K, 0))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_route(legs, rf)
    pl.set_fleet(wf, fmod)
    pl.set_traffic_follow(tf)
    pl.set_world_traffic(tracks, pts, act)
    tr = wm.World(tracks, pts, act, wf, off, own)

    def slices(si, pool):
        return np.concatenate([pool[int(si["obs_off"][c]):int(si["obs_off"][c]) + int(si["obs_n"][c])] for c in range(n)])

    si, want, _ = fl.couple(fmod, wf, off, own, pl.get_scene_in(), sc["obs_pool"])
    want, _ = tr.place(want, None, 0.0)
    assert pl.traffic_state().tobytes() == tr.s.tobytes() and pl.traffic_speed().tobytes() == tr.v.tobytes()
    assert np.concatenate([pl.get_obstacles(c) for c in range(n)]).tobytes() == slices(si, want).tobytes()
    kinds, rear = {"ego": 0, "actor": 0, "free": 0, "plain": 0}, 0
    for t in range(R_TICKS):
        pl.tick()
        pl.advance_async(model)
        seen = pl.get_scene_in()
        want, _ = tr.step(want, None, dt, tf, seen, pl.ego_flags(), width)
        si, want, _ = fl.couple(fmod, wf, off, own, seen, want)
        for a, i in enumerate(tr.info):
            kinds[i.kind] += 1
            rear += i.kind == "ego" and i.ego_scene % R_SIZE == R_SIZE - 1
        got_s, got_v = pl.traffic_state(), pl.traffic_speed()
        assert got_s.tobytes() == tr.s.tobytes(), f"tick {t}: s of vehicles {np.flatnonzero(got_s != tr.s).tolist()}"
        assert got_v.tobytes() == tr.v.tobytes(), f"tick {t}: v of vehicles {np.flatnonzero(got_v != tr.v).tolist()}"
        assert seen.tobytes() == si.tobytes(), f"tick {t}: the coupled records"
        assert np.concatenate([pl.get_obstacles(c) for c in range(n)]).tobytes() == slices(si, want).tobytes(), f"tick {t}: slices"
        assert want[0::R_OWN + R_K].tobytes() == sc["obs_pool"][0::R_OWN + R_K].tobytes()
    print("leader kinds over the run:", kinds, "rear ego led", rear)
    assert rear > R_TICKS * R_W // 2 and kinds["ego"] >= rear and (kinds["actor"] > 0 or kinds["free"] > 0)
    pl.close()
