"""Car-following traffic (pp_set_traffic_follow / pp_get_traffic_speed / k_follow_traffic): actors keep a gap to the
ego and to each other.

CPU: the ABI mirrors, hand-derived known answers of the numpy model (tests/traffic_follow_model.py) with their arithmetic, the order
and tie rules, the wave edges of the kernel's two strided searches (run on the model, which the device is held to), and three
vehicles of different desired speeds on the ring that queue instead of driving through each other
(scene B); a faster vehicle behind each of 16 ring egos in the closed loop of oracle + route model + follow model, which drives through
its ego with following off and never touches it with following on (scene A).
GPU: all of those cases on k_follow_traffic - alone, and as actors of one launch repeated to a few thousand -, each held to the model
BYTE FOR BYTE after every advance (s, v and every actor's ObPoint; the model is fed the ego pose, velocity and flag word the device
itself staged); a routed rollout with three vehicles per scene against the model; off means off; pp_update_async leaves v alone;
the error paths; scene A against the CPU loop.

Every case also asserts, from the model's record of the step, which branch it took.

Two known answers run on the model only: a NaN ego position and a NaN ego velocity.  The advance never stages either unflagged
(a non-finite pose or distance is DMPP_EGO_BAD_PATH, which freezes the resident record), and a resident record with a NaN pose
would send the tick's own kernels through it, which is not what this file is about."""
import numpy as np
import pytest

import route_scenes as rs
import traffic_follow_backends as fb
import traffic_follow_model as fm
import traffic_model as tm
import traffic_scenes as ts

gpu = pytest.mark.gpu
FAR = (4096.0, 4096.0, 0.0, False)          # an ego nowhere near a track


def _runner(dm, name, log=None):
    return fb.Runner(dm, fb.ModelBackend() if name == "model" else fb.DeviceBackend(), log)


def straight(dm, n, step=1.0, y=0.0):
    return ts.polyline(dm, [(k * step, y) for k in range(n)])


def square(dm):
    """40 points, 1 m apart, round the square (0, 0) - (10, 10); closed: the closing segment runs from (0, 1) to (0, 0), L = 40."""
    xy = [(float(k), 0.0) for k in range(10)] + [(10.0, float(k)) for k in range(10)] + [(10.0 - k, 10.0) for k in range(10)] + [(0.0, 10.0 - k) for k in range(10)]
    return ts.polyline(dm, xy)


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirrors(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(28) == dm.TrafficFollow.itemsize == 64
    assert hasattr(lib, "pp_set_traffic_follow") and hasattr(lib, "pp_get_traffic_speed")
    assert dm.TrafficFollow.names == fm.FIELDS
    tf = dm.default_traffic_follow()
    assert tuple(float(tf[k][0]) for k in fm.FIELDS) == fm.DEFAULT == (60.0, 1.5, 2.0, 1.5, 1.0, 2.0, 6.0, 0.1)


# The known answers are written once against a runner of tests/traffic_follow_backends.py: run(polylines, scenes, tf, dt, steps).
# Everything is a multiple of a small power of two unless a comment says otherwise, so the arithmetic below is exact in binary.
def _kat_free_road_from_standstill(dm, run):
    # max_dec = 32, dt = 0.5.  Actor 0: s = 10, v = v0 = 10, radius 0.5.  Actor 1 reverses at -8 m/s from s = 11, radius 0.5: in
    # step 1 it is 1 m ahead, net = 1 - 0.5 - 0.5 = 0, not > min_net -> 0.1; q = (gap + dyn) / 0.1 >= 20, acc <= 1 - 400 -> clamped to
    # -32; v' = 10 - 16 < 0 -> 0; s' = 10 + 0.5 * (10 + 0) * 0.5 = 12.5.  Actor 1 stepped to 11 - 4 = 7: behind.  Step 2, the free
    # road from standstill: r = 0 / 10 = 0, free = 1, acc = max_acc = 1, v' = 0 + 1 * 0.5 = 0.5, s' = 12.5 + 0.5 * (0 + 0.5) * 0.5 = 12.625.
    r = run([(straight(dm, 101), False)], [dict(ego=FAR, actors=[(10.0, 10.0, 0, 3, 0.5), (11.0, -8.0, 0, 4, 0.5)])], dict(max_dec=32.0))
    assert r.at(1, 0) == (12.5, 0.0, 12.5, 0.0) and r.at(2, 0) == (12.625, 0.5, 12.625, 0.0)
    i1, i2 = r.info[1][0], r.info[2][0]
    assert (i1.kind, i1.leader, i1.floored, i1.clamped, i1.stopped) == ("actor", 1, True, True, True)
    assert (i2.kind, i2.acc, i2.clamped, i2.stopped, i2.wrapped) == ("free", 1.0, False, False, False)
    # the reversing actor moves as §4h - s + speed * dt - and keeps v = speed
    assert r.at(1, 1) == (7.0, -8.0, 7.0, 0.0) and r.at(2, 1) == (3.0, -8.0, 3.0, 0.0) and r.info[1][1].kind == "plain"
    assert r.ob[2]["type"].tolist() == [3, 4] and r.ob[2]["radius"].tolist() == [0.5, 0.5]


def _kat_leader_at_equal_speed(dm, run):
    # headway = 1 (gap 2, max_acc 1, comfort_dec 2), dt = 0.5.  Actor 0: s = 7, v = v0 = 4, radius 0.5; its leader, actor 1: s = 20, v = v0 = 4,
    # radius 0.5.  r = 1, free = 1 - 1 = 0; net = 13 - 0.5 - 0.5 = 12; dv = 0, dyn = 4 * 1 + 0 / c2 = 4, star = 6, q = 0.5,
    # acc = 1 * (0 - 0.25) = -0.25; v' = 4 - 0.125 = 3.875, s' = 7 + 0.5 * 7.875 * 0.5 = 8.96875.  The leader has a free road at its
    # desired speed: acc = 0, it drives on at 4.  (v = speed at set time, so v < v0 needs a step of braking first: _kat_issue_figure.)
    tf = dict(headway=1.0)
    r = run([(straight(dm, 101), False)], [dict(ego=FAR, actors=[(7.0, 4.0, 0, 0, 0.5), (20.0, 4.0, 0, 0, 0.5)])], tf)
    i = r.info[1][0]
    assert (i.kind, i.leader, float(i.g), float(i.net), float(i.dyn), float(i.acc)) == ("actor", 1, 13.0, 12.0, 4.0, -0.25)
    assert r.at(1, 0) == (8.96875, 3.875, 8.96875, 0.0)
    assert r.info[1][1].kind == "free" and r.at(1, 1) == (22.0, 4.0, 22.0, 0.0)          # the leader: r = 1, acc = 0


def _kat_issue_figure(dm, run):
    # The issue's figure: v = vl = 4 under v0 = 8, headway 1, gap 2, net 12 gives acc = 0.6875 max_acc.  max_dec = 8, dt = 0.5.
    # Step 1 brings the follower to v = 4: actor 0 (s = 0, v = v0 = 8, radius 0.5) stands 0.5 m behind the reversing actor 1 (s = 0.5,
    # speed -16, radius 0.5): net floored, acc clamped, v' = 8 - 8 * 0.5 = 4, s' = 0 + 0.5 * (8 + 4) * 0.5 = 3.  Actor 1 clamps at the
    # track's start (0.5 - 8 < 0 -> 0): behind from now on.  Actor 2 (s = 14, v = v0 = 4, radius 0.5) drives free: r = 1, acc = 0, s' = 16.
    # Step 2: g = 16 - 3 = 13, net = 13 - 0.5 - 0.5 = 12; r = 4 / 8 = 0.5, r2 = 0.25, free = 1 - 0.0625 = 0.9375; dv = 0,
    # dyn = 4 * 1 + 0 = 4, star = 6, q = 6 / 12 = 0.5, acc = 1 * (0.9375 - 0.25) = 0.6875; v' = 4 + 0.34375 = 4.34375,
    # s' = 3 + 0.5 * 8.34375 * 0.5 = 5.0859375.
    tf = dict(headway=1.0, max_dec=8.0)
    r = run([(straight(dm, 101), False)], [dict(ego=FAR, actors=[(0.0, 8.0, 0, 0, 0.5), (0.5, -16.0, 0, 0, 0.5), (14.0, 4.0, 0, 0, 0.5)])], tf)
    assert r.at(1, 0) == (3.0, 4.0, 3.0, 0.0) and r.info[1][0].clamped and r.info[1][0].leader == 1 and not r.info[1][0].stopped
    assert r.at(1, 1)[0] == 0.0 and r.info[1][1].wrapped                                   # (the open track clamps the reversing actor at 0)
    i = r.info[2][0]
    assert (i.kind, i.leader, float(i.net), float(i.dyn), float(i.acc), i.clamped) == ("actor", 2, 12.0, 4.0, 0.6875, False)
    assert r.at(2, 0) == (5.0859375, 4.34375, 5.0859375, 0.0)


def _kat_standing_leader_inside_min_net(dm, run):
    # Actor 0: s = 10, v = v0 = 2, radius 0.5; actor 1 PARKED (speed 0) at s = 11, radius 0.5: net = 1 - 1 = 0, not > 0.1 -> 0.1; dv = 2,
    # dyn > 0, q >= 20 -> acc = -max_dec = -6 (clamped); v' = 2 - 3 < 0 -> 0; s' = 10 + 0.5 * 2 * 0.5 = 10.5.  Step 2: v = 0, r = 0, free = 1;
    # net = 0.5 - 1 < 0.1 -> 0.1, dyn = 0, star = 2, q = 20, acc = 1 - 400 -> -6, v' = 0, s' = 10.5.  The parked actor is placed as §4h places it.
    r = run([(straight(dm, 101), False)], [dict(ego=FAR, actors=[(10.0, 2.0, 0, 0, 0.5), (11.0, 0.0, 0, 9, 0.5)])])
    assert r.at(1, 0) == (10.5, 0.0, 10.5, 0.0) and r.at(2, 0) == (10.5, 0.0, 10.5, 0.0)
    for k in (1, 2):
        i = r.info[k][0]
        assert (i.kind, i.leader, i.floored, i.clamped, i.stopped, float(i.vl)) == ("actor", 1, True, True, True, 0.0)
        assert r.at(k, 1) == (11.0, 0.0, 11.0, 0.0) and r.info[k][1].kind == "plain"
    assert float(r.info[2][0].dyn) == 0.0


def _kat_ego_leader_and_flagged_ego(dm, run):
    # Scene 0: the ego on vertex 20 of the track, 14.4 km/h = 4 m/s (14.4 and 3.6 have the same significand: the quotient is exactly 4).
    # Actor 0: s = 7.5, v0 = v = 4, radius 0.5: i0 = 7, the window's vertices 8, 9, .. have g = 0.5, 1.5, ..; vertex 20 is k* = 13, d2 = 0,
    # g_e = 12.5; net = 12.5 - 0.5 - 0.5 * Vehicle_Width (0.9, not exact); dv = 0, dyn = 4 * 1.5 = 6.  Scene 1: the same with the ego FLAGGED:
    # vl = 0 whatever its velocity, dv = 4.
    egos = [(20.0, 0.0, 14.4, False), (20.0, 0.0, 14.4, True)]
    r = run([(straight(dm, 101), False)], [dict(ego=e, actors=[(7.5, 4.0, 0, 0, 0.5)]) for e in egos])
    a, b = r.info[1][0], r.info[1][1]
    assert (a.kind, a.kstar, float(a.d2), float(a.g), float(a.vl), float(a.dyn)) == ("ego", 13, 0.0, 12.5, 4.0, 6.0)
    assert float(a.net) == 12.5 - 0.5 - 0.5 * 1.8
    assert (b.kind, b.kstar, float(b.g), float(b.vl)) == ("ego", 13, 12.5, 0.0)
    assert float(b.dyn) == 4.0 * 1.5 + (4.0 * 4.0) / (2 * np.sqrt(1.0 * 2.0)) and float(b.acc) < float(a.acc)
    assert r.v[1][1] < r.v[1][0] < 4.0


KATS = [_kat_free_road_from_standstill, _kat_leader_at_equal_speed, _kat_issue_figure, _kat_standing_leader_inside_min_net,
        _kat_ego_leader_and_flagged_ego]


# ---- order and tie rules --------------------------------------------------------------------------------------------------------
def _tie_equal_s(dm, run):
    # Two actors at s = 10 (v0 = 2).  Open: the lower index is ahead - actor 1 sees actor 0 at g = 0 (floored, clamped), actor 0 sees
    # nobody.  Closed (the square, L = 40): actor 1 sees actor 0 at g = 0, actor 0 sees actor 1 a lap ahead, g = 0 + L = 40 <= look.
    r = run([(straight(dm, 101), False), (square(dm), True)],
            [dict(ego=FAR, actors=[(10.0, 2.0, 0, 0, 0.5), (10.0, 2.0, 0, 0, 0.5)]), dict(ego=FAR, actors=[(10.0, 2.0, 1, 0, 0.5), (10.0, 2.0, 1, 0, 0.5)])])
    i = r.info[1]
    assert (i[0].kind, i[1].kind, i[1].leader, float(i[1].g), i[1].clamped) == ("free", "actor", 0, 0.0, True)
    assert (i[2].kind, i[2].leader, float(i[2].g), i[3].kind, i[3].leader, float(i[3].g)) == ("actor", 3, 40.0, "actor", 2, 0.0)


def _tie_ego_wins(dm, run):
    # The ego on vertex 20 and actor 1 at s = 20; the follower at s = 9.5: g_e = 20 - 9.5 = g_b.  The ego wins: its radius and speed count.
    r = run([(straight(dm, 101), False)], [dict(ego=(20.0, 0.0, 0.0, False), actors=[(9.5, 4.0, 0, 0, 0.5), (20.0, 2.0, 0, 0, 0.25)])])
    i = r.info[1][0]
    assert (i.kind, float(i.actor_g), float(i.ego_g), float(i.vl), float(i.net)) == ("ego", 10.5, 10.5, 0.0, 10.5 - 0.5 - 0.5 * 1.8)


def _edge_lateral(dm, run):
    # lateral = 1.5: the ego 1.5 m beside vertex 20 has d2 = 2.25 == lateral * lateral: a candidate; one ulp further out it is not.
    out = float(np.nextafter(1.5, 2.0))
    r = run([(straight(dm, 101), False)], [dict(ego=(20.0, y, 0.0, False), actors=[(9.5, 4.0, 0, 0, 0.5)]) for y in (1.5, out, -1.5, -out)])
    i = r.info[1]
    assert [x.kind for x in i] == ["ego", "free", "ego", "free"] and [x.kstar for x in i] == [11] * 4
    assert float(i[0].d2) == 2.25 and float(i[1].d2) > 2.25


def _edge_look(dm, run):
    # look = 60.  An actor exactly 60 m ahead is a leader, one ulp further it is not; the same for the ego's vertex (the follower at
    # s = 0: i0 = 0, vertex 60 has g = 60; from s = -ulp .. the window's edge is moved instead: look one ulp below 60 in a launch of
    # its own, see _edge_look_short).
    over = float(np.nextafter(60.0, 61.0))
    r = run([(straight(dm, 101), False)],
            [dict(ego=FAR, actors=[(0.0, 4.0, 0, 0, 0.5), (60.0, 0.0, 0, 0, 0.5)]), dict(ego=FAR, actors=[(0.0, 4.0, 0, 0, 0.5), (over, 0.0, 0, 0, 0.5)]),
             dict(ego=(60.0, 0.0, 0.0, False), actors=[(0.0, 4.0, 0, 0, 0.5)]), dict(ego=(61.0, 0.0, 0.0, False), actors=[(0.0, 4.0, 0, 0, 0.5)])])
    i = r.info[1]
    assert (i[0].kind, float(i[0].g), i[2].kind, i[2].n_actor_candidates) == ("actor", 60.0, "free", 0)
    assert (i[4].kind, i[4].kstar, i[4].window, float(i[4].g)) == ("ego", 60, 60, 60.0)
    assert (i[5].kind, i[5].kstar, i[5].window, float(i[5].d2)) == ("ego", 60, 60, 1.0)          # vertex 61 is outside: 60 is the nearest that takes part


def _edge_look_short(dm, run):
    # look one ulp below 60: the actor and the vertex at g = 60 are out; the ego on vertex 60 is still seen from vertex 59 (d2 = 1).
    r = run([(straight(dm, 101), False)],
            [dict(ego=FAR, actors=[(0.0, 4.0, 0, 0, 0.5), (60.0, 0.0, 0, 0, 0.5)]), dict(ego=(60.0, 0.0, 0.0, False), actors=[(0.0, 4.0, 0, 0, 0.5)])],
            dict(look=float(np.nextafter(60.0, 0.0))))
    i = r.info[1]
    assert (i[0].kind, i[0].n_actor_candidates) == ("free", 0) and (i[2].kind, i[2].window, i[2].kstar, float(i[2].g)) == ("ego", 59, 59, 59.0)


QUEUE = [(3.0, 6.0), (9.5, 2.0), (17.0, 5.0), (22.25, 1.0), (31.0, 7.0)]


def _jacobi_permutation(dm, run):
    # Five actors with distinct s on the closed square, three steps; launched in two other orders every actor gives the same bytes.
    scenes = [dict(ego=(10.0, 4.0, 3.6, False), actors=[(s, v, 0, 0, 0.5) for s, v in QUEUE])]
    base = run([(square(dm), True)], scenes, steps=3)
    assert sorted(i.kind for i in base.info[1]) == ["actor"] * 4 + ["ego"]
    for order in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        r = run([(square(dm), True)], scenes, steps=3, order=order)
        for k in range(4):
            assert r.s[k].tobytes() == base.s[k].tobytes() and r.v[k].tobytes() == base.v[k].tobytes() and r.ob[k].tobytes() == base.ob[k].tobytes(), (order, k)


# ---- wave edges -----------------------------------------------------------------------------------------------------------------
GROUPS = [(1, None), (2, 1), (63, 62), (64, 63), (65, 63), (65, 64), (129, 63), (129, 64), (129, 127), (129, 128)]


def _wave_groups(dm, run):
    # One scene per (members, p): member 0 at s = 0 is the actor under test, its leader is member p at s = 5 - lane p % 64 of stride
    # step p // 64 - and the others stand at 10 + 0.25 i; 63 | 64 and 127 | 128 are the last lane of a pass and the first of the next.
    scenes = []
    for n, p in GROUPS:
        scenes.append(dict(ego=FAR, actors=[(0.0 if i == 0 else 5.0 if i == p else 10.0 + 0.25 * i, 3.0, 0, i, 0.125) for i in range(n)]))
    r = run([(straight(dm, 201), False)], scenes)
    a = 0
    for n, p in GROUPS:
        i = r.info[1][a]
        assert i.n_members == n and i.n_actor_candidates == n - 1
        assert (i.kind, i.leader) == (("free", -1) if p is None else ("actor", a + p)), (n, p)
        a += n


def _wave_window(dm, W):
    def case(dm, run):
        # The actor at s = 0.5 on a 1 m track: i0 = 0, vertex k has g = k - 0.5, so look = W - 0.5 gives a window of exactly W vertices.
        # One scene per k*: the ego 0.5 m beside vertex k* (d2 = 0.25; its neighbours 1.25) - the first, the last, and both sides of
        # every 64-lane stride step inside the window.
        # The last scene: the ego beside vertex W + 1, the first one OUTSIDE the window, is seen from the last one inside (d2 = 1 + 0.25).
        ks = sorted({1, W} | {k for k in (64, 65, 128, 129) if k <= W})
        r = run([(straight(dm, 201), False)], [dict(ego=(float(k), 0.5, 0.0, False), actors=[(0.5, 3.0, 0, 0, 0.5)]) for k in ks + [W + 1]], dict(look=W - 0.5))
        for a, k in enumerate(ks):
            i = r.info[1][a]
            assert (i.kind, i.window, i.kstar, float(i.d2), float(i.g)) == ("ego", W, k, 0.25, k - 0.5), (W, k)
        i = r.info[1][len(ks)]
        assert (i.kind, i.window, i.kstar, float(i.d2), float(i.g)) == ("ego", W, W, 1.25, W - 0.5), W
    case.__name__ = f"_wave_window_{W}"
    return case


def _closing_segment(dm, run):
    # The closed square (n = 40, L = 40), the actor at s = 37.5: i0 = 37; k = 2 is j = 39 = n - 1 (g = 1.5), k = 3 is j = n: P[0], g = (40 - 37.5) + 0
    # = 2.5, k = 4 is j = n + 1: P[1], g = 3.5.  Scenes 0 - 2: the ego on P[39], P[0], P[1].  Scene 3: an actor leader across the closing
    # segment, at s = 0.5: g = 0.5 - 37.5 = -37 -> + 40 = 3.  Scene 4: look = 60 > L is a one-lap window of n = 40 vertices, the last one
    # P[i0] itself, a lap ahead: the ego on P[30], behind the actor, is seen at g = 32.5.  Scene 5: alone on the lap (it is no candidate
    # for itself), v = v0 = 3: acc = 0, it drives across s = L.
    sq = square(dm)
    egos = [(float(sq["x"][j]), float(sq["y"][j]), 0.0, False) for j in (39, 0, 1)]
    scenes = [dict(ego=e, actors=[(37.5, 3.0, 0, 0, 0.5)]) for e in egos]
    scenes.append(dict(ego=FAR, actors=[(37.5, 3.0, 0, 0, 0.5), (0.5, 1.0, 0, 0, 0.5)]))
    scenes.append(dict(ego=(float(sq["x"][30]), float(sq["y"][30]), 0.0, False), actors=[(37.5, 3.0, 0, 0, 0.5)]))
    scenes.append(dict(ego=FAR, actors=[(39.5, 3.0, 0, 0, 0.5)]))
    r = run([(sq, True)], scenes, steps=3)
    i = r.info[1]
    assert [(x.kind, x.kstar, float(x.g)) for x in i[:3]] == [("ego", 2, 1.5), ("ego", 3, 2.5), ("ego", 4, 3.5)]
    assert all(x.window == 40 for x in i[:3])
    assert (i[3].kind, i[3].leader, float(i[3].g)) == ("actor", 4, 3.0) and (i[4].kind, float(i[4].g)) == ("actor", 37.0)
    assert (i[5].kind, i[5].kstar, i[5].window, float(i[5].g)) == ("ego", 33, 40, 32.5)
    assert (i[6].kind, i[6].n_members, i[6].window, i[6].wrapped) == ("free", 1, 40, True) and r.at(1, 6)[0] == 1.0          # 39.5 + 0.5 * 6 * 0.5 = 41 -> 1


def _open_end_and_zero_segments(dm, run):
    # Scene 0: an open track of 11 points, the actor at s = 7.5: i0 = 7, the window ends at n - 1 = 10 with 3 vertices although look = 60;
    # the ego on the last vertex: k* = 3.  Scene 1: nobody ahead: the actor runs to the end and clamps at L = 10.
    # Scene 2: zero-length segments - points 0, 1, 2, 2, 2, 3, 4 (x), the actor at s = 0.5, the ego on x = 2: vertices 2, 3, 4 tie at d2 = 0
    # and the first, k* = 2, wins; g = 1.5.
    dup = ts.polyline(dm, [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (2.0, 0.0), (2.0, 0.0), (3.0, 0.0), (4.0, 0.0)])
    r = run([(straight(dm, 11), False), (dup, False)],
            [dict(ego=(10.0, 0.0, 0.0, False), actors=[(7.5, 3.0, 0, 0, 0.5)]), dict(ego=FAR, actors=[(7.5, 8.0, 0, 0, 0.5)]),
             dict(ego=(2.0, 0.0, 0.0, False), actors=[(0.5, 3.0, 1, 0, 0.5)])])
    i = r.info[1]
    assert (i[0].kind, i[0].window, i[0].kstar, float(i[0].g)) == ("ego", 3, 3, 2.5)
    assert i[1].kind == "free" and r.info[2][1].wrapped and r.at(2, 1)[0] == 10.0
    assert (i[2].kind, i[2].window, i[2].kstar, float(i[2].d2), float(i[2].g)) == ("ego", 6, 2, 0.0, 1.5)


def _edges(dm):
    return [_tie_equal_s, _tie_ego_wins, _edge_lateral, _edge_look, _edge_look_short, _jacobi_permutation, _wave_groups,
            _wave_window(dm, 63), _wave_window(dm, 64), _wave_window(dm, 65), _wave_window(dm, 129), _closing_segment, _open_end_and_zero_segments]


CASES = KATS + _edges(None)


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[1:])
def test_case_on_the_model(dm, case):
    case(dm, _runner(dm, "model"))


def test_nan_ego_on_the_model(dm):
    """A NaN ego position gives no ego candidate (every d2 is NaN, and a NaN is never the minimum); a NaN ego velocity gives
    dv = NaN, dyn = NaN -> 0: the follower keeps the standstill gap only.  (Model only: see the module docstring.)"""
    run = _runner(dm, "model")
    r = run([(straight(dm, 101), False)], [dict(ego=(np.nan, 0.0, 0.0, False), actors=[(7.5, 4.0, 0, 0, 0.5)]), dict(ego=(20.0, np.nan, 0.0, False), actors=[(7.5, 4.0, 0, 0, 0.5)]),
                                          dict(ego=(20.0, 0.0, np.nan, False), actors=[(7.5, 4.0, 0, 0, 0.5)])])
    i = r.info[1]
    assert (i[0].kind, i[0].kstar, i[1].kind, i[1].kstar) == ("free", -1, "free", -1) and i[0].window == 60
    assert (i[2].kind, float(i[2].dyn), np.isnan(i[2].vl)) == ("ego", 0.0, True)
    # star = gap = 2, net = 12.5 - 0.5 - 0.9, free = 0
    assert float(i[2].acc) == 1.0 * (0.0 - (2.0 / (12.5 - 0.5 - 0.5 * 1.8)) * (2.0 / (12.5 - 0.5 - 0.5 * 1.8)))


def test_parked_and_reversing_actors_step_as_lane_traffic(dm):
    """An actor with !(speed > 0) gives, with following on, the bytes §4h's model gives - on open and closed tracks, wrapping and
    clamping - whatever stands in front of it."""
    rows = [(1.0, -3.0, 0, 1, 0.5), (50.0, 0.0, 0, 2, 0.5), (0.5, -3.0, 1, 3, 0.5), (39.0, 0.0, 1, 4, 0.5), (2.0, -0.0, 0, 5, 0.5)]
    polylines = [(straight(dm, 101), False), (square(dm), True)]
    r = _runner(dm, "model")(polylines, [dict(ego=(3.0, 0.0, 0.0, False), actors=rows)], steps=3)
    tracks, pts = ts.pack(dm, polylines)
    plain = tm.Traffic(tracks, pts, ts.actors(dm, [(x[0], x[1], 0, k, x[2], x[3], x[4]) for k, x in enumerate(rows)]), np.zeros(1, np.int64))
    pool, _ = plain.place(np.zeros(len(rows), dm.ObPoint), None, 0.0)
    for k in range(1, 4):
        pool, _ = plain.place(pool, None, 0.5)
        assert r.s[k].tobytes() == plain.s.tobytes() and r.ob[k].tobytes() == pool.tobytes()
        assert r.v[k].tolist() == [x[1] for x in rows] and all(i.kind == "plain" for i in r.info[k])


# ---- three vehicles on the ring (scene B) ------------------------------------------------------------------------------------------
B_TICKS, B_DT = 400, 0.1
B_ROWS = [(0.0, 9.0), (40.0, 2.5), (90.0, 5.0)]          # (s0, desired speed): the fastest starts behind the slowest
B_RADIUS = 0.9


def _ring_three(dm, follow):
    m = rs.build_ring(dm)
    tracks, pts = ts.pack(dm, [(ts.ring_track(dm, m, 2), True)])
    act = ts.actors(dm, [(s, v, 0, k, 0, 7, B_RADIUS) for k, (s, v) in enumerate(B_ROWS)])
    tr = fm.Follow(tracks, pts, act, np.zeros(1, np.int64))
    si, flags = np.zeros(1, dm.SceneIn), np.zeros(1, np.int32)
    si["loc"]["globalpoint"]["x"], si["loc"]["globalpoint"]["y"] = 1.0e6, 1.0e6          # no ego near
    pool, _ = tr.place(np.zeros(3, dm.ObPoint), None, 0.0)
    L, lap, net_min, orders = tr.length(0), np.zeros(3), np.inf, set()
    for _ in range(B_TICKS):
        before = tr.s.copy()
        if follow:
            pool, _ = tr.step(pool, None, B_DT, None, si, flags, 1.8)
        else:
            pool, _ = tr.place(pool, None, B_DT)
        lap += tr.s < before                                     # (a wrap: s fell)
        total = tr.s + lap * L                                   # unwrapped distance along the ring
        orders.add((tuple(np.argsort(total).tolist()), bool(total.max() - total.min() < L)))          # who is ahead of whom, and nobody lapped
        ahead = np.sort(total)
        gaps = np.diff(np.concatenate([ahead, [ahead[0] + L]]))
        net_min = min(net_min, float(gaps.min() - 2 * B_RADIUS))
    return dict(total=total, net_min=net_min, orders=orders, start=np.array([s for s, _ in B_ROWS]), L=L, v=tr.v.copy())


def test_three_vehicles_queue_on_the_ring(dm):
    """Scene B.  Three vehicles with desired speeds 9, 2.5 and 5 m/s on one closed ring track (lane 2, about 600 m), no ego near,
    400 steps of 0.1 s.  With following on they never pass each other - the unwrapped arc lengths keep their order 0 < 1 < 2 < 0 + L -
    and no net gap goes <= 0; the same vehicles at constant speed (following off) do reorder: 0 drives through 1."""
    on, off = _ring_three(dm, True), _ring_three(dm, False)
    print("following on: travelled", np.round(on["total"] - on["start"], 2).tolist(), "smallest net gap", round(on["net_min"], 3), "speeds", np.round(on["v"], 3).tolist(),
          "\nfollowing off: travelled", np.round(off["total"] - off["start"], 2).tolist(), "smallest net gap", round(off["net_min"], 3))
    t = on["total"]
    assert on["orders"] == {((0, 1, 2), True)} and on["net_min"] > 0          # after every one of the 400 steps: 0 < 1 < 2 < 0 + L
    assert t[0] < t[1] < t[2] < t[0] + on["L"] and len(off["orders"]) > 1
    assert off["total"][0] > off["total"][1] and off["net_min"] <= 0
    assert on["v"][0] < 9.0 and (on["total"] - on["start"] > 50.0).all()          # 0 was held up, and everybody drove


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[1:])
def test_case_on_the_device(dm, case):
    """The known answers, the tie rules and the wave edges on k_follow_traffic, each also held byte for byte against the model."""
    case(dm, _runner(dm, "device"))


_LOG = []


def _case_log(dm):
    if not _LOG:
        run = _runner(dm, "model", _LOG)
        for case in CASES:
            case(dm, run)
    return _LOG


@gpu
@pytest.mark.parametrize("count", [None, 3000])
def test_cases_batched(dm, count):
    """Every case as scenes of one launch per model (count None), and repeated cyclically to 3000 actors and more: every actor gives the
    bytes its case gave alone, and the device the model's."""
    n = fb.batched(dm, fb.DeviceBackend(), _case_log(dm), repeat_to=count)
    assert n >= (count or 1)


def test_cases_batched_on_the_model(dm):
    """The batched replay itself, on the model: the cases do not disturb each other as scenes of one launch."""
    assert fb.batched(dm, fb.ModelBackend(), _case_log(dm)) > 700


R_N, R_OBS, R_TICKS = 32, 4, 60


def _ring_scene(dm, n=R_N, seed=5):
    """Routed ring egos (tests/route_scenes.py) with R_OBS own obstacle entries each: entry 0 static and far away, entries 1 - 3 three
    vehicles on the closed ring track of the ego's own lane: one 12 m behind the ego and faster than it, two ahead at different speeds,
    one of them parked."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, n, seed=seed, lanes=(1, 2), ids=(120, 170), legs=(6, 10), n_obs=R_OBS)
    sc["scene_in"]["obs_n"] = R_OBS
    pool = sc["obs_pool"]
    pool["x"], pool["y"], pool["radius"], pool["type"] = -500.0, -500.0, 0.5, 1
    polylines = [(ts.ring_track(dm, m, 1), True), (ts.ring_track(dm, m, 2), True)]
    tracks, pts = ts.pack(dm, polylines)
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(n):
        loc = sc["scene_in"]["loc"][s]
        lane = int(loc["lane_num"])
        p = polylines[lane - 1][0]
        here = tm.cumulative(p["x"], p["y"], True)[ts.SEG * (int(loc["road_num"]) - 1) + int(loc["id"][lane - 1])]
        rows.append((here - 12.0, rng.choice([4.0, 6.0, 9.0]), s, 1, lane - 1, 100 + s, 0.9))
        rows.append((here + rng.uniform(15.0, 30.0), rng.choice([0.0, 1.5, 2.5]), s, 2, lane - 1, 200 + s, 0.9))
        rows.append((here + rng.uniform(35.0, 55.0), rng.choice([-1.0, 1.0, 3.0]), s, 3, lane - 1, 300 + s, 1.1))
    return cfg, m, sc, legs, rf, tracks, pts, ts.actors(dm, rows)


def _planner(dm, cfg, m, sc, n_obs, motion=False):
    pl = dm.Planner(cfg, device=0, **rs.caps(m, len(sc["scene_in"]), n_obs, 0))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=motion)
    pl.set_state(sc["state"])
    return pl


def _slices(pl, n):
    return np.concatenate([pl.get_obstacles(s) for s in range(n)])


@gpu
def test_step_check_on_a_routed_rollout(dm):
    """60 ticks on 32 routed ring egos with three vehicles each, one of them behind the ego and faster.  After every advance the model,
    fed the SceneIn records and flag words the device staged, gives s, v and every scene's slice byte for byte; the vehicle behind
    finds the ego as its leader, the others each other; the static entries never change."""
    cfg, m, sc, legs, rf, tracks, pts, act = _ring_scene(dm)
    model, tf = dm.default_ego_model(), dm.default_traffic_follow()
    dt = float(model["dt"][0])
    pl = _planner(dm, cfg, m, sc, R_OBS)
    pl.set_route(legs, rf)
    pl.set_traffic_follow(tf)                                    # before the traffic: pp_set_traffic sets v = speed
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_speed()
    pl.set_traffic(tracks, pts, act)
    tr = fm.Follow(tracks, pts, act, sc["scene_in"]["obs_off"])
    want, _ = tr.place(sc["obs_pool"], None, 0.0)
    assert pl.traffic_state().tobytes() == tr.s.tobytes() and pl.traffic_speed().tobytes() == tr.v.tobytes()
    kinds = {"ego": 0, "actor": 0, "free": 0, "plain": 0}
    for t in range(R_TICKS):
        pl.tick()
        pl.advance_async(model)
        want, _ = tr.step(want, None, dt, tf, pl.get_scene_in(), pl.ego_flags(), float(cfg["Vehicle_Width"][0]))
        for i in tr.info:
            kinds[i.kind] += 1
        got_s, got_v = pl.traffic_state(), pl.traffic_speed()
        assert got_s.tobytes() == tr.s.tobytes(), f"tick {t}: s of actors {np.flatnonzero(got_s != tr.s).tolist()}"
        assert got_v.tobytes() == tr.v.tobytes(), f"tick {t}: v of actors {np.flatnonzero(got_v != tr.v).tolist()}"
        assert _slices(pl, R_N).tobytes() == want.tobytes(), f"tick {t}: slices"
        assert want[0::R_OBS].tobytes() == sc["obs_pool"][0::R_OBS].tobytes()
    print("leader kinds over the run:", kinds)
    assert kinds["ego"] > R_TICKS * R_N // 2 and kinds["actor"] > R_TICKS * R_N // 2 and kinds["plain"] > 0
    pl.close()


@gpu
@pytest.mark.parametrize("mode", ["never", "null", "on_then_null", "no_traffic"])
def test_off_means_off(dm, mode):
    """Following never set, set to NULL, switched on and off again before the first advance, and set on a handle without traffic: over
    20 advances the staged pool and pp_get_traffic_state are §4h's model's, byte for byte (no traffic: the pool is the caller's, and
    both getters are PP_ERR_STATE)."""
    cfg, m, sc, legs, rf, tracks, pts, act = _ring_scene(dm, n=16, seed=13)
    n, model = 16, dm.default_ego_model()
    dt = float(model["dt"][0])
    pl = _planner(dm, cfg, m, sc, R_OBS)
    pl.set_route(legs, rf)
    if mode != "no_traffic":
        pl.set_traffic(tracks, pts, act)
    if mode == "null":
        pl.set_traffic_follow(None)
    if mode in ("on_then_null", "no_traffic"):
        pl.set_traffic_follow(dm.default_traffic_follow())
    if mode == "on_then_null":
        assert pl.traffic_speed().tobytes() == np.ascontiguousarray(act["speed"]).tobytes()
        pl.set_traffic_follow(None)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_speed()
    tr = tm.Traffic(tracks, pts, act, sc["scene_in"]["obs_off"])
    want = sc["obs_pool"].copy()
    if mode != "no_traffic":
        want, _ = tr.place(want, None, 0.0)
    for t in range(20):
        pl.tick()
        pl.advance_async(model)
        if mode == "no_traffic":
            with pytest.raises(dm.PlannerError, match="error -4:"):
                pl.traffic_state()
        else:
            want, _ = tr.place(want, None, dt)
            assert pl.traffic_state().tobytes() == tr.s.tobytes(), f"tick {t}: arc lengths"
        assert _slices(pl, n).tobytes() == want.tobytes(), f"tick {t}: pool"
    pl.tick()
    assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * R_OBS).tobytes() == want.tobytes()
    pl.close()


@gpu
def test_switching_off_mid_run_and_surviving_set_egos(dm):
    """Following on for an odd number of advances, then off: the actors go on at constant speed from where they are (§4h's model from
    the s the follow model reached).  The model survives pp_set_egos: traffic set again afterwards follows at once."""
    cfg, m, sc, legs, rf, tracks, pts, act = _ring_scene(dm, n=16, seed=21)
    n, model, tf = 16, dm.default_ego_model(), dm.default_traffic_follow()
    dt = float(model["dt"][0])
    pl = _planner(dm, cfg, m, sc, R_OBS)
    pl.set_route(legs, rf)
    pl.set_traffic(tracks, pts, act)
    pl.set_traffic_follow(tf)
    tr = fm.Follow(tracks, pts, act, sc["scene_in"]["obs_off"])
    want, _ = tr.place(sc["obs_pool"], None, 0.0)
    for t in range(3):
        pl.tick()
        pl.advance_async(model)
        want, _ = tr.step(want, None, dt, tf, pl.get_scene_in(), pl.ego_flags(), float(cfg["Vehicle_Width"][0]))
    pl.tick()
    assert pl.traffic_state().tobytes() == tr.s.tobytes()
    pl.set_traffic_follow(None)
    assert pl.traffic_state().tobytes() == tr.s.tobytes()
    for t in range(3):
        pl.advance_async(model)
        want, _ = tr.place(want, None, dt)
        assert pl.traffic_state().tobytes() == tr.s.tobytes() and _slices(pl, n).tobytes() == want.tobytes(), f"advance {t} after off"
        pl.tick()
    pl.set_traffic_follow(tf)                                    # on again: v = speed
    assert pl.traffic_speed().tobytes() == np.ascontiguousarray(act["speed"]).tobytes()
    pl.set_egos(sc, with_motion=False)                           # traffic off, the model stays
    pl.set_state(sc["state"])
    pl.set_route(legs, rf)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.traffic_speed()
    pl.set_traffic(tracks, pts, act)
    tr = fm.Follow(tracks, pts, act, sc["scene_in"]["obs_off"])
    want, _ = tr.place(sc["obs_pool"], None, 0.0)
    for t in range(2):
        pl.tick()
        pl.advance_async(model)
        want, _ = tr.step(want, None, dt, tf, pl.get_scene_in(), pl.ego_flags(), float(cfg["Vehicle_Width"][0]))
        assert pl.traffic_state().tobytes() == tr.s.tobytes() and pl.traffic_speed().tobytes() == tr.v.tobytes(), f"advance {t} after set_egos"
        assert _slices(pl, n).tobytes() == want.tobytes()
    assert any(i.kind == "ego" for i in tr.info)
    pl.close()


@gpu
def test_update_async_leaves_the_speeds(dm):
    """After some following advances a caller-uploaded pool comes out with the actors at the current s, and v is what it was."""
    cfg, m, sc, legs, rf, tracks, pts, act = _ring_scene(dm, n=16, seed=11)
    n, model, tf = 16, dm.default_ego_model(), dm.default_traffic_follow()
    dt = float(model["dt"][0])
    pl = _planner(dm, cfg, m, sc, R_OBS)
    pl.set_route(legs, rf)
    pl.set_traffic(tracks, pts, act)
    pl.set_traffic_follow(tf)
    tr = fm.Follow(tracks, pts, act, sc["scene_in"]["obs_off"])
    want, _ = tr.place(sc["obs_pool"], None, 0.0)
    for _ in range(3):
        pl.tick()
        pl.advance_async(model)
        want, _ = tr.step(want, None, dt, tf, pl.get_scene_in(), pl.ego_flags(), float(cfg["Vehicle_Width"][0]))
    pl.tick()
    s_now, v_now = tr.s.copy(), tr.v.copy()
    assert (v_now != act["speed"]).any()
    up = dm.pinned_copy(np.frombuffer(bytes([0x5A]) * (n * R_OBS * dm.ObPoint.itemsize), dm.ObPoint))
    pl.update_async(obs_pool=up)
    assert pl.traffic_state().tobytes() == s_now.tobytes() and pl.traffic_speed().tobytes() == v_now.tobytes()
    pl.tick()
    want, _ = tr.place(np.array(up), None, 0.0)
    assert tr.s.tobytes() == s_now.tobytes()
    assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, n * R_OBS).tobytes() == want.tobytes()
    pl.advance_async(model)                                      # ... and the next advance follows from there
    want, _ = tr.step(want, None, dt, tf, pl.get_scene_in(), pl.ego_flags(), float(cfg["Vehicle_Width"][0]))
    assert pl.traffic_state().tobytes() == tr.s.tobytes() and pl.traffic_speed().tobytes() == tr.v.tobytes()
    assert _slices(pl, n).tobytes() == want.tobytes()
    pl.close()


@gpu
def test_errors_leave_the_model_as_it_was(dm):
    """Every refused call leaves the model that was set: the advance after it matches the numpy model with the old parameters."""
    cfg, m, sc, legs, rf, tracks, pts, act = _ring_scene(dm, n=8, seed=17)
    n, model, tf = 8, dm.default_ego_model(), dm.default_traffic_follow()
    dt = float(model["dt"][0])
    assert dm.load_library().pp_sizeof(28) == 64
    pl = _planner(dm, cfg, m, sc, R_OBS)
    pl.set_route(legs, rf)
    pl.set_traffic(tracks, pts, act)
    pl.set_traffic_follow(tf)
    tr = fm.Follow(tracks, pts, act, sc["scene_in"]["obs_off"])
    want, _ = tr.place(sc["obs_pool"], None, 0.0)
    bad = [(k, x) for k in fm.FIELDS for x in (np.nan, np.inf)] + [(k, 0.0) for k in ("look", "gap", "max_acc", "comfort_dec", "max_dec", "min_net")] + \
          [(k, -1.0) for k in fm.FIELDS]
    for k, x in bad:
        t2 = tf.copy()
        t2[k] = x
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_traffic_follow(t2)
    ok = tf.copy()
    ok["lateral"], ok["headway"] = 0.0, 0.0                      # both may be 0
    pl.set_traffic_follow(ok)
    pl.set_traffic_follow(tf)
    for _ in range(2):
        pl.tick()
        pl.advance_async(model)
        for arg in (tf, None):                                   # an update is staged - for a model and for off alike
            with pytest.raises(dm.PlannerError, match="error -4:"):
                pl.set_traffic_follow(arg)
        want, _ = tr.step(want, None, dt, tf, pl.get_scene_in(), pl.ego_flags(), float(cfg["Vehicle_Width"][0]))
        assert pl.traffic_state().tobytes() == tr.s.tobytes() and pl.traffic_speed().tobytes() == tr.v.tobytes()
        assert _slices(pl, n).tobytes() == want.tobytes()
    pl.close()


# ---- a faster vehicle behind every ego (scene A) -------------------------------------------------------------------------------------
A_N, A_TICKS = 16, 300
A_GAP, A_SPEED, A_RADIUS, A_TYPE = 12.0, 6.0, 0.9, 7
_CPU = {}


def _chased(dm):
    """16 ring egos of the closed loop of tests/test_traffic.py (lanes 1 / 2, 120 .. 170 points into their first road, grid stage off;
    starts on lane 2 of the two-lane road 3 left out, as there: those egos answer a vehicle with a lane change).  Every ego owns one
    obstacle entry: a vehicle A_GAP = 12 m BEHIND it on the closed track of its own lane that wants A_SPEED = 6 m/s - the planner drives
    the empty ring at 10 km/h = 2.8 m/s."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, 2 * A_N, seed=3, lanes=(1, 2), ids=(120, 170), legs=(6, 10), n_obs=1)
    loc = sc["scene_in"]["loc"]
    keep = np.flatnonzero(~((loc["road_num"] == 3) & (loc["lane_num"] == 2)))[:A_N]
    assert len(keep) == A_N
    legs = np.concatenate([legs[rf[k]:rf[k + 1]] for k in keep])
    rf = np.concatenate([[0], np.cumsum([rf[k + 1] - rf[k] for k in keep])]).astype(np.int32)
    sc = dict(sc, scene_in=sc["scene_in"][keep].copy(), state=sc["state"][keep].copy(), obs_pool=np.zeros(A_N, dm.ObPoint), mot_pool=None)
    sc["obs_pool"]["radius"] = 0.5
    sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"] = np.arange(A_N), 1
    polylines = [(ts.ring_track(dm, m, 1), True), (ts.ring_track(dm, m, 2), True)]
    tracks, pts = ts.pack(dm, polylines)
    rows = []
    for s in range(A_N):
        loc = sc["scene_in"]["loc"][s]
        lane = int(loc["lane_num"])
        p = polylines[lane - 1][0]
        here = tm.cumulative(p["x"], p["y"], True)[ts.SEG * (int(loc["road_num"]) - 1) + int(loc["id"][lane - 1])]
        rows.append((here - A_GAP, A_SPEED, s, 0, lane - 1, A_TYPE, A_RADIUS))
    return cfg, m, sc, legs, rf, tracks, pts, ts.actors(dm, rows)


def _cpu_loop(dm, oracle, follow):
    import map_scenes as ms
    import rollout_score_model as sm
    import route_model as rmod
    if follow in _CPU:
        return _CPU[follow]
    cfg, m, sc, legs, rf, tracks, pts, act = _chased(dm)
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt = float(model["dt"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"].copy()), sc["state"].copy(), np.zeros(A_N, np.int32)
    tr = fm.Follow(tracks, pts, act, si["obs_off"])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    scores = sm.new_scores(dm.RolloutScore, A_N)
    sins, pools, ss, vs, kinds = [si], [obs], [tr.s.copy()], [tr.v.copy()], {"ego": 0, "free": 0}
    for t in range(A_TICKS + 1):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        sm.fold(scores, cfg, dt, si, plan, st, obs, flags)
        if t < A_TICKS:
            si, flags, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
            if follow:
                obs, _ = tr.step(obs, None, dt, None, si, flags, float(cfg["Vehicle_Width"][0]))
                for i in tr.info:
                    kinds[i.kind] += 1
            else:
                obs, _ = tr.place(obs, None, dt)
            sins.append(si), pools.append(obs), ss.append(tr.s.copy()), vs.append(tr.v.copy())
    _CPU[follow] = dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, tracks=tracks, pts=pts, act=act, sins=sins, pools=pools, s=ss, v=vs, scores=scores, flags=flags, kinds=kinds)
    return _CPU[follow]


def test_chased_egos_closed_loop_on_the_cpu(dm, oracle):
    """Scene A: oracle tick + route model + traffic / follow model, 301 scored ticks.  With following OFF every vehicle drives through
    its ego (n_collision_ticks > 0 for all 16); with following ON none ever touches it (n_collision_ticks == 0, first_collision_tick
    == -1) and every vehicle has the ego as its leader for most of the run."""
    off, on = _cpu_loop(dm, oracle, False), _cpu_loop(dm, oracle, True)
    print("off: collision ticks", off["scores"]["n_collision_ticks"].tolist(), "\non: min clearance", np.round(on["scores"]["min_clearance"], 2).tolist(),
          "\non: ego dist", np.round(on["scores"]["dist"], 1).tolist(), "vehicle dist", np.round(on["s"][-1] - on["s"][0], 1).tolist(), "\nleader kinds", on["kinds"])
    assert (off["scores"]["n_collision_ticks"] > 0).all()
    assert (on["scores"]["n_collision_ticks"] == 0).all() and (on["scores"]["first_collision_tick"] == -1).all()
    assert on["kinds"]["ego"] > A_TICKS * A_N // 2


@gpu
def test_chased_egos_closed_loop_agrees_with_the_cpu_loop(dm, oracle):
    """Scene A on the device, 300 advances with scoring on, against the CPU loop.  The staged records agree within the bounds
    tests/test_route.py uses for its closed loop (parity_util.compare); the scorecard's integer fields are equal - no collision tick.
    The vehicles' s and v depend on the ego's pose, which agrees to about 1e-9 m, not to the bit; the law is smooth in it except where
    the nearest vertex k* changes, and an ego within 1e-9 m of that tie can make one side switch a tick earlier: g_e then differs by one
    0.5 m segment for one tick, which moves acc by at most max_acc * 2 q dq <= 1 * 2 * 3 * 0.15 m/s^2 (q <= 3 at these gaps,
    dq = star * 0.5 / net^2), v by 0.09 m/s and s by less than 0.01 m per event.  The bound on s is 0.05 m; without such an event the
    difference stays near the 1e-9 m of the poses, and the largest one is printed."""
    from parity_util import compare
    r = _cpu_loop(dm, oracle, True)
    pl = _planner(dm, r["cfg"], r["m"], r["sc"], 1)
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    pl.set_traffic_follow(dm.default_traffic_follow())
    pl.score_begin()
    model = dm.default_ego_model()
    assert pl.traffic_state().tobytes() == r["s"][0].tobytes() and pl.traffic_speed().tobytes() == r["v"][0].tobytes()
    worst_s = worst_v = 0.0
    lap = fm.Follow(r["tracks"], r["pts"], r["act"], np.arange(A_N)).cum                    # (a wrap a tick apart is a difference of a lap)
    lap = np.array([lap[int(k)][-1] for k in r["act"]["track"]])
    for t in range(A_TICKS):
        pl.tick()
        pl.advance_async(model)
        bad = compare(pl.get_scene_in(), r["sins"][t + 1], "scene_in")
        assert not bad, f"tick {t}\n" + "\n".join(bad[:10])
        ds = np.abs(pl.traffic_state() - r["s"][t + 1])
        worst_s, worst_v = max(worst_s, float(np.minimum(ds, np.abs(lap - ds)).max())), max(worst_v, float(np.abs(pl.traffic_speed() - r["v"][t + 1]).max()))
        assert worst_s <= 0.05, f"tick {t}: arc lengths off by {worst_s!r} m"
    pl.tick()
    score, want = pl.rollout_score(), r["scores"]
    print(f"largest difference over {A_TICKS} ticks: s {worst_s!r} m, v {worst_v!r} m/s")
    for k, (dt_, _) in dm.RolloutScore.fields.items():
        if dt_.base.kind == "i":
            assert np.array_equal(score[k], want[k]), (k, score[k].tolist(), want[k].tolist())
    assert (score["n_collision_ticks"] == 0).all() and (score["first_collision_tick"] == -1).all() and not pl.ego_flags().any()
    pl.close()
