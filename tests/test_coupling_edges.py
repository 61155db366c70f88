"""Edges of the scorecard's front half (k_score_ego) and of the fleet coupling step (k_couple_fleet; §4e)
that no generated scene reaches.  Both kernels give one 64-lane wave to a scene, stride by 64 over a list of any length and end in
a (value, index) wave minimum whose tie rule - the first index of the smallest - is part of the specification: the cases below put
the minimum, exact ties, NaNs and the range edge on the last lane of a pass, the first lane of the next, the same lane of two
passes, a low index in a high lane against a high index in lane 0, and on both sides of the 4096 members the fleet kernel marks.

Every case has a hand-derived literal and is written once against a runner of tests/coupling_backends.py: asserted on the numpy
model (CPU) and on the device, where every record / every pool byte is also held against the model, and then run again inside
batches of distinct scenes / worlds.  All coordinates are dyadic and every distance is a 3-4-5 triangle or lies along an axis, so
the literals are asserted with ==; where a tie is the point of a case it is asserted to be an exact one.

Left out, with the reason: a fleet range of +inf (pp_set_fleet refuses a range that is not finite: test_errors_leave_the_fleet_as_it_was);
the status clamp of k_score_grid (no API reaches it, one thread per scene: test_kat_counters_and_histograms, model leg)."""
import math

import numpy as np
import pytest

import coupling_backends as cb

gpu = pytest.mark.gpu
INF, NAN = math.inf, math.nan


@pytest.fixture()
def cfg0(dm):
    cfg = cb.config()
    assert 0.5 * float(cfg["Vehicle_Width"][0]) == 0.9
    return cfg


# ---------------------------------------------------------------------------------------------------------------
# k_score_ego.  The ego disc has radius 0.9.  A FAR obstacle j stands 8 + j/4 m to the left of the ego with radius 0.5:
# d_j = 7.5 + j/4.  A NEAR one stands on one of twelve points exactly 5 m from the ego, radius 0.5: d = sqrt(25) - 0.5 = 4.5,
# clearance 4.5 - 0.9.
RING = [(3.0, 4.0), (-3.0, -4.0), (4.0, 3.0), (-4.0, -3.0), (-3.0, 4.0), (3.0, -4.0), (-4.0, 3.0), (4.0, -3.0), (5.0, 0.0), (0.0, -5.0), (-5.0, 0.0), (0.0, 5.0)]
NEAR = 4.5 - 0.9


def _obs(ex, ey, m, near=(), put=None):
    """m obstacles around an ego at (ex, ey): FAR ones, NEAR ones at the indices `near` (each on a ring point of its own), and the
    records of `put` (index -> (x, y, radius), absolute)."""
    obs = [(ex, ey + 8.0 + 0.25 * j, 0.5) for j in range(m)]
    for k, j in enumerate(near):
        obs[j] = (ex + RING[k][0], ey + RING[k][1], 0.5)
    for j, o in (put or {}).items():
        obs[j] = o
    return obs


def _d(ex, ey, o):
    """d_j of §4d 1."""
    dx, dy = o[0] - ex, o[1] - ey
    return math.sqrt(dx * dx + dy * dy) - float(np.float32(o[2]))


def _scored(cfg, run, obs, ex=10.0, ey=0.0, lead=0):
    """One tick of one scene; (min_clearance, min_clearance_tick, min_clearance_obs, first_collision_tick, n_collision_ticks, n_ticks)."""
    r = run(cfg, 0.1, [cb.tick(cfg, [(ex, ey, 36.0, obs)], lead=lead)]).after[0]
    return _clear(r, 0)


def _clear(r, s):
    return (float(r["min_clearance"][s]), int(r["min_clearance_tick"][s]), int(r["min_clearance_obs"][s]), int(r["first_collision_tick"][s]),
            int(r["n_collision_ticks"][s]), int(r["n_ticks"][s]))


M_ALL = (0, 1, 63, 64, 65, 127, 128, 129, 200)


def _edges_score_minimum(dm, cfg0, run):
    # no obstacle: no clearance
    assert _scored(cfg0, run, []) == (INF, -1, -1, -1, 0, 1)
    # the unique minimum on the last obstacle - the last lane of a full pass (m = 64, 128), the only lane of a short last pass
    # (65, 129), the middle of one (200) - and on 63 / 64 / 128: the last lane of pass 1, the first lane of passes 2 and 3
    for m in M_ALL[1:]:
        for j in sorted({m - 1, 63, 64, 128}):
            if j < m:
                assert _scored(cfg0, run, _obs(10.0, 0.0, m, near=[j])) == (NEAR, 0, j, -1, 0, 1), (m, j)
    # without a NEAR one the nearest is FAR obstacle 0: 7.5 - 0.9
    assert _scored(cfg0, run, _obs(10.0, 0.0, 200)) == (7.5 - 0.9, 0, 0, -1, 0, 1)
    # a radius that is not exact in f32, on the only lane of pass 2: 1.7f = 1.7000000476837158 widened; 2.5 m abeam: a collision
    got = _scored(cfg0, run, _obs(10.0, 0.0, 65, put={64: (10.0, 2.5, 1.7)}))
    assert got == (2.5 - float(np.float32(1.7)) - 0.9, 0, 64, 0, 1, 1) and got[0] < -0.1


def _edges_score_ties(dm, cfg0, run):
    # exact ties at d = 4.5 between obstacles on different ring points: the first index, whichever lane or pass holds it.
    # (5, 64): lane 5 of pass 1 against lane 0 of pass 2 - the lower index in the higher lane; (63, 64): neighbours across the pass
    # boundary; (0, 64, 128): one lane, three passes; (64, 1): as (5, 64) with the higher index written first; (128, 3): the only
    # lane of pass 3 against pass 1
    for m, tied, want in ((129, (5, 64), 5), (129, (63, 64), 63), (129, (0, 64, 128), 0), (129, (64, 1), 1), (129, (128, 3), 3), (200, (199, 70, 134), 70),
                          (65, (64, 5), 5)):
        obs = _obs(10.0, 0.0, m, near=tied)
        assert len({obs[j][:2] for j in tied}) == len(tied) and all(_d(10.0, 0.0, obs[j]) == 4.5 for j in tied)          # (distinct obstacles, an exact tie)
        assert _scored(cfg0, run, obs) == (NEAR, 0, want, -1, 0, 1), (m, tied)
    # a tie at -inf (discs of infinite radius): the first index, a collision
    put = {66: (10.0, 3.0, INF), 2: (13.0, 4.0, INF)}
    assert _scored(cfg0, run, _obs(10.0, 0.0, 129, put=put)) == (-INF, 0, 2, 0, 1, 1)


def _edges_score_nan(dm, cfg0, run):
    # a NaN d_j: from x, from the radius, from inf - inf (an obstacle at infinity with an infinite radius)
    nans = [(NAN, 0.0, 0.5), (10.0, 3.0, NAN), (INF, 0.0, INF)]
    assert all(math.isnan(_d(10.0, 0.0, o)) for o in nans)
    # every entry of lane 0 (0, 64, 128) is a NaN, the minimum is elsewhere: lane 0 has nothing to offer, the others are not hidden
    put = {0: nans[0], 64: nans[1], 128: nans[2]}
    assert _scored(cfg0, run, _obs(10.0, 0.0, 129, near=[70], put=put)) == (NEAR, 0, 70, -1, 0, 1)
    assert _scored(cfg0, run, _obs(10.0, 0.0, 129, put=put)) == (7.5 + 0.25 - 0.9, 0, 1, -1, 0, 1)           # (FAR obstacle 1)
    # the whole of pass 1 is NaNs, the minimum is in pass 2: every lane still holds "none" when pass 2 begins
    put = {j: nans[j % 3] for j in range(64)}
    assert _scored(cfg0, run, _obs(10.0, 0.0, 129, near=[100], put=put)) == (NEAR, 0, 100, -1, 0, 1)
    assert _scored(cfg0, run, _obs(10.0, 0.0, 129, put=put)) == (7.5 + 16.0 - 0.9, 0, 64, -1, 0, 1)          # (FAR obstacle 64)
    # all NaN: no clearance - after a tick that had one the three fields and the collision fields stay, the tick is counted
    all_nan = [nans[j % 3] for j in range(129)]
    hit = _obs(10.0, 0.0, 129, put={2: (10.0, 0.5, 0.0)})                        # a point 0.5 m abeam: clearance 0.5 - 0.9
    res = run(cfg0, 0.1, [cb.tick(cfg0, [(10.0, 0.0, 36.0, hit)]), cb.tick(cfg0, [(10.0, 0.0, 36.0, all_nan)])])
    assert _clear(res.after[0], 0) == (0.5 - 0.9, 0, 2, 0, 1, 1) and _clear(res.after[1], 0) == (0.5 - 0.9, 0, 2, 0, 1, 2)
    assert _scored(cfg0, run, all_nan) == (INF, -1, -1, -1, 0, 1)
    # all distances +inf (obstacles at infinity): obstacle 0 is the nearest, the clearance is +inf - and inf < inf is false: nothing
    # is replaced, min_clearance_tick stays -1, no collision
    assert _scored(cfg0, run, [(INF, 0.0, 0.5)] * 70) == (INF, -1, -1, -1, 0, 1)


def _edges_score_waves_of_a_block(dm, cfg0, run):
    # seven scenes of one launch - two blocks, the second partial - with another m in every wave; three entries that belong to
    # nobody (discs of 1000 m on the ego) in front of every slice, so the first obs_off is 3 and the offsets are odd and even
    ms = (65, 0, 129, 1, 64, 200, 63)
    near = ([64], [], [128, 5], [0], [63, 62], [199, 135], [5, 4])
    egos = [(10.0 + 16.0 * k, 2.0 * k, 36.0, _obs(10.0 + 16.0 * k, 2.0 * k, m, near=nr)) for k, (m, nr) in enumerate(zip(ms, near))]
    t = cb.tick(cfg0, egos, lead=3)
    assert t.si["obs_off"].tolist() == [3, 71, 74, 206, 210, 277, 480]
    r = run(cfg0, 0.1, [t]).after[0]
    want = [(NEAR, 0, 64), (INF, -1, -1), (NEAR, 0, 5), (NEAR, 0, 0), (NEAR, 0, 62), (NEAR, 0, 135), (NEAR, 0, 4)]
    assert [_clear(r, s)[:3] for s in range(7)] == want and (r["n_collision_ticks"] == 0).all() and (r["n_ticks"] == 1).all()
    # ... and one scene alone behind a lead of three
    assert _scored(cfg0, run, _obs(10.0, 0.0, 129, near=[128]), lead=3) == (NEAR, 0, 128, -1, 0, 1)


def _edges_score_ticks(dm, cfg0, run):
    # 129 obstacles around a standing ego, tick by tick
    e = (10.0, 0.0)
    ticks = [_obs(*e, 129, near=[128]),                                          # 0: 4.5 - 0.9 on obstacle 128
             _obs(*e, 129, near=[5]),                                            # 1: the same clearance on obstacle 5: strict <, nothing moves
             _obs(*e, 129, put={64: (13.0, 4.0, 4.5)}),                          # 2: a disc of 4.5 m, 5 m away: 0.5 - 0.9, the first collision
             [],                                                                 # 3: no obstacle: only the counters
             _obs(*e, 129, put={127: (7.0, -4.0, 4.75)}),                        # 4: deeper, 0.25 - 0.9: the first collision tick stays
             _obs(*e, 129, put={65: (10.0, 0.9, 0.0)}),                          # 5: a point 0.9 m abeam: sqrt(0.9*0.9) - 0 - 0.9 = 0: touching is a collision
             _obs(*e, 129, put={65: (10.0, math.nextafter(0.9, 1.0), 0.0)})]     # 6: one ulp further it is not
    res = run(cfg0, 0.1, [cb.tick(cfg0, [(e[0], e[1], 36.0, o)]) for o in ticks])
    want = [(NEAR, 0, 128, -1, 0, 1), (NEAR, 0, 128, -1, 0, 2), (0.5 - 0.9, 2, 64, 2, 1, 3), (0.5 - 0.9, 2, 64, 2, 1, 4), (0.25 - 0.9, 4, 127, 2, 2, 5),
            (0.25 - 0.9, 4, 127, 2, 3, 6), (0.25 - 0.9, 4, 127, 2, 3, 7)]
    assert [_clear(r, 0) for r in res.after] == want
    # ... and the same last two ticks on a fresh record: the clearance is 0.0 exactly, then positive
    res = run(cfg0, 0.1, [cb.tick(cfg0, [(e[0], e[1], 36.0, o)]) for o in ticks[6:4:-1]])
    assert _clear(res.after[0], 0)[1:] == (0, 65, -1, 0, 1) and 0.0 < float(res.after[0]["min_clearance"][0]) < 1e-15
    assert _clear(res.after[1], 0) == (0.0, 1, 65, 1, 1, 2)
    # the 3-4-5 ramp among 65 obstacles that move with the ego: (0, 0) at 10 km/h, (3, 4) at 13.6, (9, 12) at 10, dt 0.1 s:
    # dist = 5 + 10, rise and fall (13.6 - 10)/3.6/0.1 m/s^2
    pts = ((0.0, 0.0, 10.0), (3.0, 4.0, 13.6), (9.0, 12.0, 10.0))
    r = run(cfg0, 0.1, [cb.tick(cfg0, [(x, y, v, _obs(x, y, 65, near=[64]))]) for x, y, v in pts]).after[2]
    assert (float(r["dist"][0]), float(r["max_speed"][0]), float(r["max_acc"][0]), float(r["max_dec"][0])) == (15.0, 13.6, (13.6 - 10.0) / 3.6 / 0.1, -((10.0 - 13.6) / 3.6 / 0.1))
    assert (float(r["last_pos"]["x"][0]), float(r["last_pos"]["y"][0]), float(r["last_speed"][0])) == (9.0, 12.0, 10.0)
    assert _clear(r, 0) == (NEAR, 0, 64, -1, 0, 3)


SCORE_EDGES = [_edges_score_minimum, _edges_score_ties, _edges_score_nan, _edges_score_waves_of_a_block, _edges_score_ticks]


# ---------------------------------------------------------------------------------------------------------------
# k_couple_fleet.  A world of n members stands behind p0 scenes of another world; member j of it is scene p0 + j.  Unless a case
# puts it elsewhere a member stands alone, 1000 + 100 j m east of the observer: out of everybody's range.
O = (100.0, 50.0)                                     # the observer


def _world(n, p0, at, o=O):
    """(positions, world_first): p0 scenes of a world of their own (far to the west, 100 m apart), then the n members; at: member ->
    (x, y) relative to the observer at `o`."""
    xy = [(-1000.0 - 100.0 * k, 0.0) for k in range(p0)]
    xy += [(o[0] + at[j][0], o[1] + at[j][1]) if j in at else (o[0] + 1000.0 + 100.0 * j, o[1]) for j in range(n)]
    return xy, ([0, p0, p0 + n] if p0 else [0, n])


def _fm(dm, rng=60.0, K=8, radius=0.9):
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"], fm["radius"] = rng, K, radius
    return fm


def _d2(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return dx * dx + dy * dy


def _edges_fleet_strides(dm, cfg0, run):
    # the observer first, last and at index 64 of worlds of 2 .. 129 members that begin at scene 0, 3 and 61; its peers are the
    # members at 0, 1, 62 .. 65, 127, 128 (the ends of the strides), the one with the highest index nearest: 1 m, 2 m, ... north of it
    for n in (2, 63, 64, 65, 128, 129):
        for obs in sorted({0, n - 1, 64} & set(range(n))):
            near = sorted(({0, 1, 62, 63, 64, 65, 127, 128} & set(range(n))) - {obs}, reverse=True)
            at = {j: (0.0, 1.0 + k) for k, j in enumerate(near)}
            at[obs] = (0.0, 0.0)
            for p0 in (0, 3, 61):
                xy, wf = _world(n, p0, at)
                r = run(cfg0, _fm(dm), wf, xy, n_own=1)
                assert r.peers(p0 + obs) == (len(near), [p0 + j for j in near]), (n, obs, p0)
                assert int(r.out["obs_n"][p0 + obs]) == 1 + len(near) and int(r.out["obs_off"][p0 + obs]) == 9 * (p0 + obs)


def _edges_fleet_ties(dm, cfg0, run):
    # exact ties in d2 = 25 on ring points around the observer (member 10) with fewer slots than tied members: the lower scene
    # index wins.  (5, 64): the lower index in the higher lane; (63, 64): neighbours across the stride step; (1, 65): one lane,
    # consecutive steps.  K = 1 takes the lower one, K = 2 both in order
    for p0 in (0, 3, 61):
        for lo, hi in ((5, 64), (63, 64), (1, 65)):
            for first in (lo, hi):                                   # (either of the two on either ring point)
                at = {10: (0.0, 0.0), first: RING[0], lo + hi - first: RING[1]}
                xy, wf = _world(129, p0, at)
                assert _d2(xy[p0 + lo], xy[p0 + 10]) == _d2(xy[p0 + hi], xy[p0 + 10]) == 25.0 and xy[p0 + lo] != xy[p0 + hi]
                assert run(cfg0, _fm(dm, K=1), wf, xy).peers(p0 + 10) == (1, [p0 + lo]), (p0, lo, hi)
                assert run(cfg0, _fm(dm, K=2), wf, xy).peers(p0 + 10) == (2, [p0 + lo, p0 + hi]), (p0, lo, hi)
        # six tied on six ring points, K = 3: the three lowest, whatever their lanes (64 -> lane 0, 128 -> lane 0, 2 -> lane 2 ...)
        tied = (128, 64, 70, 2, 127, 66)
        at = {j: RING[k] for k, j in enumerate(tied)}
        at[10] = (0.0, 0.0)
        xy, wf = _world(129, p0, at)
        assert all(_d2(xy[p0 + j], xy[p0 + 10]) == 25.0 for j in tied)
        assert run(cfg0, _fm(dm, K=3), wf, xy).peers(p0 + 10) == (3, [p0 + 2, p0 + 64, p0 + 66]), p0


def _edges_fleet_one_spot(dm, cfg0, run):
    # 70 members on one spot, K = 8: every d2 is 0 - the eight lowest indices other than the observer, in order, for every observer:
    # round k takes the smallest (0, p) above the last one taken, across lanes and stride steps
    for p0 in (0, 3):
        xy, wf = _world(70, p0, {j: (0.0, 0.0) for j in range(70)})
        for motion in (True, False):
            r = run(cfg0, _fm(dm), wf, xy, n_own=2, motion=motion)
            assert r.peers(p0 + 0) == (8, [p0 + j for j in range(1, 9)])
            assert r.peers(p0 + 35) == (8, [p0 + j for j in range(8)]) and r.peers(p0 + 69) == (8, [p0 + j for j in range(8)])
            assert r.peers(p0 + 5) == (8, [p0 + j for j in (0, 1, 2, 3, 4, 6, 7, 8)])
            if motion:                      # every written slot has zero motion; the own entries' motion keeps its bytes
                with_motion = r
                for s in (p0, p0 + 35, p0 + 69):
                    a = int(r.off[s])
                    assert r.mot[a:a + 2].tobytes() == bytes([cb.FILL]) * 32 and r.mot[a + 2:a + 10].tobytes() == bytes(8 * 16)
                    assert r.pool[a:a + 2].tobytes() == bytes([cb.FILL]) * 48
            else:                           # no motion pool: the same slices
                assert r.mot is None and r.pool.tobytes() == with_motion.pool.tobytes() and r.out.tobytes() == with_motion.out.tobytes()


def _edges_fleet_slots(dm, cfg0, run):
    # K = 64 (FLEET_MAX_PEERS): every lane keeps a round.  The observer is member 0; member j stands (n - j) / 2 m north of it, so
    # the highest index is the nearest, but members 6 and 7 stand 32 m north and south: tied
    def line(n):
        at = {j: (0.0, 0.5 * (n - j)) for j in range(1, n)}
        at[0] = (0.0, 0.0)
        if n > 7:
            at[6], at[7] = (0.0, 32.0), (0.0, -32.0)
        return _world(n, 3, at)
    # 63 candidates: obs_n = n_own + 63 and slot 63 keeps its bytes
    xy, wf = line(64)
    r = run(cfg0, _fm(dm, K=64), wf, xy, n_own=2)
    # 63 .. 8 stand 0.5 .. 28 m away, 5 .. 1 stand 29.5 .. 31.5 m away, then 6 and 7 at 32 m, the lower index first
    want = [3 + j for j in range(63, 7, -1)] + [3 + j for j in (5, 4, 3, 2, 1, 6, 7)]
    assert r.peers(3) == (63, want) and int(r.out["obs_n"][3]) == 2 + 63
    assert r.slots(3)[63].tobytes() == bytes([cb.FILL]) * 24
    # 64 candidates: every slot; member 1 now stands 32 m north as well, on member 6: three tied, by index
    xy, wf = line(65)
    want = [3 + j for j in range(64, 7, -1)] + [3 + j for j in (5, 4, 3, 2, 1, 6, 7)]
    assert run(cfg0, _fm(dm, K=64), wf, xy, n_own=2).peers(3) == (64, want)
    # 70 candidates: the 64 nearest - 70, 69, .. 8 are nearer than 32 m (63 of them), then 6 and 7 tie for the last slot: 6
    xy, wf = line(71)
    assert _d2(xy[3 + 6], xy[3]) == _d2(xy[3 + 7], xy[3]) == 1024.0
    assert run(cfg0, _fm(dm, K=64), wf, xy, n_own=2).peers(3) == (64, [3 + j for j in range(70, 7, -1)] + [3 + 6])
    # K = 0 with own entries: obs_n = n_own, no pool byte changes
    r = run(cfg0, _fm(dm, K=0), wf, xy, n_own=3)
    assert (r.out["obs_n"] == 3).all() and r.out["obs_off"].tolist() == [3 * s for s in range(74)] and r.pool.tobytes() == r.pool_in.tobytes()
    # a world of one beside it sees nobody: scene 0 alone, scenes 1, 2 a world of two on one spot
    r = run(cfg0, _fm(dm), [0, 1, 3], [(0.0, 0.0), (0.0, 0.0), (0.0, 0.0)])
    assert [r.peers(s) for s in range(3)] == [(0, []), (1, [2]), (1, [1])]


def _edges_fleet_range_and_nan(dm, cfg0, run):
    # range 5 in a world of 65: member 64 at (3, 4) has d2 = 25 = 5*5: in (<=); member 1 at (0, nextafter(5)): out
    y = math.nextafter(5.0, 6.0)
    assert y * y > 25.0
    for p0 in (0, 3):
        xy, wf = _world(65, p0, {0: (0.0, 0.0), 64: (3.0, 4.0), 1: (0.0, y)}, o=(0.0, 0.0))          # (the observer at the origin: y keeps its last bit)
        assert xy[p0 + 1] == (0.0, y)
        r = run(cfg0, _fm(dm, rng=5.0, K=4), wf, xy)
        assert r.peers(p0) == (1, [p0 + 64])
        assert r.peers(p0 + 1) == (1, [p0 + 64]) and r.peers(p0 + 64) == (2, [p0 + 1, p0])          # (1 and 64 are 3 m and y - 4 ~ 1 m apart: d2 ~ 10)
        assert r.slots(p0)[1:].tobytes() == bytes([cb.FILL]) * (3 * 24)
        # 65 members on one spot but member 64 with a NaN x and member 1 with an infinite y: neither is anybody's peer, neither
        # sees anybody - whichever lane and stride step they sit in
        at = {j: (0.0, 0.0) for j in range(65)}
        at[64], at[1] = (NAN, 0.0), (0.0, INF)
        xy, wf = _world(65, p0, at)
        r = run(cfg0, _fm(dm), wf, xy, n_own=1)
        assert r.peers(p0) == (8, [p0 + j for j in range(2, 10)]) and r.peers(p0 + 63) == (8, [p0] + [p0 + j for j in range(2, 9)])
        for s in (p0 + 64, p0 + 1):
            assert r.peers(s) == (0, []) and int(r.out["obs_n"][s]) == 1 and r.slots(s).tobytes() == bytes([cb.FILL]) * (8 * 24)
        for s in range(p0, p0 + 65):
            assert not {p0 + 64, p0 + 1} & set(r.peers(s)[1]), s
        # ... and with the NaN in member 0, the first entry of lane 0: it hides nobody
        at = {j: (0.0, 0.0) for j in range(65)}
        at[0], at[64] = (NAN, 0.0), (0.0, NAN)
        xy, wf = _world(65, p0, at)
        r = run(cfg0, _fm(dm), wf, xy, n_own=1)
        assert r.peers(p0 + 5) == (8, [p0 + j for j in (1, 2, 3, 4, 6, 7, 8, 9)]) and r.peers(p0 + 63) == (8, [p0 + j for j in range(1, 9)])
        assert r.peers(p0) == (0, []) and r.peers(p0 + 64) == (0, [])
        for s in range(p0, p0 + 65):
            assert not {p0, p0 + 64} & set(r.peers(s)[1]), s


def _edges_fleet_4096(dm, cfg0, run):
    # one world of 4161 members: 64 stride steps of 64 lanes are marked (members 0 .. 4095), 65 members form the tail every round
    # looks at again.  K = 5, range 5.  Around member 10 seven members stand on ring points (d2 = 25): 200 and 4031 (marked), 4095
    # (the last marked one), 4096 (the first of the tail), 4097, 4159 and 4160 (lane 0 again, the next step of the tail): the five lowest
    at = {10: (0.0, 0.0)}
    tied = (4096, 4160, 4095, 4097, 200, 4159, 4031)
    at.update({j: RING[k] for k, j in enumerate(tied)})
    # member 4100 - in the tail of its own lane - stands 5000 m north with 4, 4036 (its lane, marked) and 4101 on its spot (d2 = 0) and
    # 4099, 4158 and 68 on ring points around it: the three at 0 in index order, then the two lowest at 25; itself never
    B = (0.0, 5000.0)
    at.update({4100: B, 4: B, 4036: B, 4101: B})
    at.update({j: (B[0] + RING[k][0], B[1] + RING[k][1]) for k, j in enumerate((4099, 4158, 68))})
    xy, wf = _world(4161, 0, at)
    assert all(_d2(xy[j], xy[10]) == 25.0 for j in tied) and all(_d2(xy[j], xy[4100]) == 25.0 for j in (4099, 4158, 68))
    r = run(cfg0, _fm(dm, rng=5.0, K=5), wf, xy, n_own=1, motion=True, batch=False)
    assert r.peers(10) == (5, [200, 4031, 4095, 4096, 4097])
    assert r.peers(4100) == (5, [4, 4036, 4101, 68, 4099])
    assert r.peers(4036) == (5, [4, 4100, 4101, 68, 4099]) and r.peers(4101) == (5, [4, 4036, 4100, 68, 4099])
    assert r.peers(4150) == (0, []) and r.peers(300) == (0, [])
    a = int(r.off[4100])
    assert r.mot[a:a + 1].tobytes() == bytes([cb.FILL]) * 16 and r.mot[a + 1:a + 6].tobytes() == bytes(5 * 16)


FLEET_EDGES = [_edges_fleet_strides, _edges_fleet_ties, _edges_fleet_one_spot, _edges_fleet_slots, _edges_fleet_range_and_nan, _edges_fleet_4096]


# ---------------------------------------------------------------------------------------------------------------
def _score_runner(name, log=None):
    return cb.ScoreRunner(cb.ScoreModelBackend() if name == "model" else cb.ScoreDeviceBackend(), log)


def _fleet_runner(name, log=None):
    return cb.FleetRunner(cb.FleetModelBackend() if name == "model" else cb.FleetDeviceBackend(), log)


@pytest.mark.parametrize("edges", SCORE_EDGES, ids=lambda f: f.__name__[7:])
def test_edges_on_the_model(dm, cfg0, edges):
    edges(dm, cfg0, _score_runner("model"))


@pytest.mark.parametrize("edges", FLEET_EDGES, ids=lambda f: f.__name__[7:])
def test_fleet_edges_on_the_model(dm, cfg0, edges):
    edges(dm, cfg0, _fleet_runner("model"))


@gpu
@pytest.mark.parametrize("edges", SCORE_EDGES, ids=lambda f: f.__name__[7:])
def test_edges_on_the_device(dm, cfg0, edges):
    edges(dm, cfg0, _score_runner("device"))


@gpu
@pytest.mark.parametrize("edges", FLEET_EDGES, ids=lambda f: f.__name__[7:])
def test_fleet_edges_on_the_device(dm, cfg0, edges):
    edges(dm, cfg0, _fleet_runner("device"))


@gpu
def test_edges_batch_equals_each_case_alone(dm, cfg0):
    """Every single-scene scorecard case once more on the device, logged, then as distinct scenes of one launch per group of calls
    that can share one (coupling_backends.score_batched): no multiple of four, more than one block; bytes as alone."""
    log = []
    run = _score_runner("device", log)
    for edges in SCORE_EDGES:
        edges(dm, cfg0, run)
    sizes = cb.score_batched(cb.ScoreDeviceBackend(), log)
    print(f"{len(log)} calls in batches of {sizes}")
    assert sum(sizes) >= len(log) and all(n % 4 != 0 and n > 4 for n in sizes)


@gpu
def test_fleet_edges_batch_equals_each_case_alone(dm, cfg0):
    """Every fleet case but the 4161-member world once more on the device, logged, then the calls that share a FleetModel as worlds
    of one launch (coupling_backends.fleet_batched): most worlds begin at a scene index that is no multiple of 64; bytes as alone."""
    log = []
    run = _fleet_runner("device", log)
    for edges in FLEET_EDGES[:-1]:
        edges(dm, cfg0, run)
    sizes = cb.fleet_batched(cb.FleetDeviceBackend(), log)
    print(f"{len(log)} calls in batches of {sizes} scenes")
    assert sum(sizes) >= sum(len(c["xy"]) for c in log) and all(n % 4 != 0 and n > 4 for n in sizes)
