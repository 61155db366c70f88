"""team_search_obstacle's deferred arc-length sum (csrc/dev_geom.hpp) on crafted scenes: full ticks, device against the oracle.

The search sums the arc length only up to the nearest accepted vertex b*, extends the run of absorbed additions behind it
and, where the rule does not hold (a length that is not finite; a tie run with more than 64 obstacles), runs a second pass
with the full sum.  tests/search_obstacle_rule.py is the rule, tests/test_search_obstacle_rule.py checks it against the
oracle on the CPU; here every branch of the device code is driven through k_decision (corridor F and the five others:
teams of two waves; the junction path: four waves; the lateral sweep) and k_planning (four waves).  Batches of 1 to 8
scenes, 128 x 128 grid, grid stage off; every batch is compared with the oracle field by field over three ticks."""
import numpy as np
import pytest

from parity_util import compare
from test_front_cull import N_TICKS, _cfg, _far, _run, _set_lane, _set_obs, _straight_xy

EGO = 50


def _first(cfg):
    return EGO + int(cfg["ID_MORE"][0])              # lane point of corridor F's vertex 0


def _unit(xy, k):
    a, b = (xy[k], xy[k + 1]) if k + 1 < len(xy) else (xy[k - 1], xy[k])
    t = (b - a) / np.hypot(*(b - a))
    return t, np.array([-t[1], t[0]])


def _beside(xy, k, lat=0.2, along=0.0):
    t, side = _unit(xy, k)
    return tuple(xy[k] + along * t + lat * side)


def _scenes(dm, cfg, seed, n, n_obs, junction_every=0):
    sc = dm.gen_scenes(cfg, seed, n, n_obs, junction_every=junction_every)
    sc["mot_pool"][:] = 0
    return sc


def _pre_junction(sc, s):
    """Scene s becomes a pre-junction scene whose front path is its lane from the ego on (no junction polyline behind it)."""
    sc["scene_in"]["loc"]["pos"][s], sc["scene_in"]["ref_n"][s] = 1, 0


def _absorbed_lane(n, x0, step, at):
    """A lane along +y, `step` between points; point at+1 lies one ulp of x0 beside point `at`, at the same y."""
    y = 100.0 + step * np.arange(n, dtype=np.float64)
    y[at + 1:] -= step
    x = np.full(n, x0)
    x[at + 1:] = np.nextafter(x0, np.inf)
    return np.stack([x, y], axis=1)


@pytest.mark.gpu
def test_winner_vertices(dm, oracle):
    """The winner on F's vertex 0, n-1 and 7, 8, 9, 15, 16, 17 (both sides of serial_sum's eight-wide blocks; the sum runs
    over s[1 .. b*]), each with accepted obstacles farther along that come first in j.  Lane-change attributes 0 to 3; the
    scene on vertex 8 has a wide lane, so the third tick runs the lateral sweep."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(2110)
    verts = (0, 119, 7, 8, 9, 15, 16, 17)
    sc = _scenes(dm, cfg, 5100, len(verts), 24)
    first = _first(cfg)
    for s, v in enumerate(verts):
        xy = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 23.0 * s)
        chg = 0 if v == 8 else s % 4
        _set_lane(dm, sc, s, xy, EGO, lanechg=chg, width=7.0 if v == 8 else 3.75)
        inward = 0.1 if v == 0 else -0.1 if v == 119 else 0.0
        later = [_beside(xy, first + w, -0.3) for w in range(v + 2, min(v + 30, 118), 9)]
        _set_obs(sc, s, _far(rng, 3, xy) + later + _far(rng, 5, xy) + [_beside(xy, first + v, 0.2, inward)] + _far(rng, 2, xy))
    plans, _ = _run(dm, oracle, cfg, sc, "winner vertices")
    a = plans[0]["around"]
    assert a["Obs_flag"][:, 0].tolist() == [1] * len(verts) and a["Ob_Pathid"][:, 0].tolist() == list(verts)
    assert (plans[-1]["sweep_index"] >= 0).any() or (plans[-1]["sweep_side"] != 0).any()          # the sweep ran and chose


@pytest.mark.gpu
def test_planning_path_vertices(dm, oracle):
    """The same vertices on Planning's path: a first tick without obstacles gives the path the oracle plans (it does not
    depend on the obstacles while the behaviour stays), then the obstacles go beside its points."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(2111)
    verts = (0, 199, 7, 8, 9, 15, 16, 17)
    sc = _scenes(dm, cfg, 5200, len(verts), 12)
    for s in range(len(verts)):
        _set_lane(dm, sc, s, _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 31.0 * s), EGO, lanechg=0)
        _set_obs(sc, s, [])
    dry, _, _ = oracle.plan_tick_batch(cfg, sc, sc["state"].copy(), want_grid=False)
    for s, v in enumerate(verts):
        road = np.stack([dry["road_points"]["x"][s], dry["road_points"]["y"][s]], axis=1)
        xy = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 31.0 * s)
        inward = 0.02 if v == 0 else -0.02 if v == 199 else 0.0
        later = [_beside(road, w, -0.2) for w in range(v + 3, min(v + 60, 198), 19)]
        _set_obs(sc, s, _far(rng, 2, xy) + later + [_beside(road, v, 0.05, inward)] + _far(rng, 3, xy))
    plans, _ = _run(dm, oracle, cfg, sc, "planning path vertices")
    assert plans[0]["ob_flag"].tolist() == [1] * len(verts)
    assert plans[0]["ob_pathid"].tolist() == list(verts), plans[0]["ob_pathid"].tolist()


@pytest.mark.gpu
def test_planning_path_counts_and_ties(dm, oracle):
    """On Planning's path (four waves): 1, 63, 64, 65 and 129 obstacles with the winner last in j, an accepted obstacle
    farther along first and, from 65 on, the winner's lane of the wave holding an earlier obstacle on a later vertex; two
    obstacles on one vertex in both j orders, next to each other and 64 apart (one lane).  The absorbed tie and repeated points
    cannot be put there: on a road the path is a Bezier curve of 200 distinct points some 0.1 to 0.5 m apart and 60 m long, so
    no addition of its sum is absorbed; those two families run on corridor F and on the junction path (test_ties)."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(2117)
    sc = _scenes(dm, cfg, 5250, 8, 129)
    for s in range(8):
        _set_lane(dm, sc, s, _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 29.0 * s), EGO, lanechg=0)
        _set_obs(sc, s, [])
    dry, _, _ = oracle.plan_tick_batch(cfg, sc, sc["state"].copy(), want_grid=False)
    want = {}
    for s in range(8):
        road = np.stack([dry["road_points"]["x"][s], dry["road_points"]["y"][s]], axis=1)
        xy = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 29.0 * s)
        if s < 5:
            m, v = (1, 63, 64, 65, 129)[s], 40 + 3 * s
            pts = _far(rng, m, xy)
            pts[m - 1] = _beside(road, v, 0.05)
            if m > 1:
                pts[0] = _beside(road, 150, -0.1)
            if m > 64:
                pts[m - 1 - 64] = _beside(road, 120, 0.1)
            if m > 128:
                pts[m - 1 - 128] = _beside(road, 90, 0.1)
            want[s] = (v, pts[m - 1])
        else:
            v, gap = 60 + s, (0, 63, 70)[s - 5]
            a, b = _beside(road, v, 0.06), _beside(road, v, -0.05)
            pair = (a, b) if s != 6 else (b, a)
            pts = _far(rng, 3, xy) + [pair[0]] + _far(rng, gap, xy) + [pair[1], _beside(road, 170, 0.1)]
            want[s] = (v, pair[0])
        _set_obs(sc, s, pts)
    plans, _ = _run(dm, oracle, cfg, sc, "planning path counts / ties")
    p = plans[0]
    assert p["ob_flag"].tolist() == [1] * 8
    for s, (v, ob) in want.items():
        assert p["ob_pathid"][s] == v and (p["ob"]["x"][s], p["ob"]["y"][s]) == ob, (s, p["ob_pathid"][s], v, ob)


@pytest.mark.gpu
def test_counts_and_nothing_accepted(dm, oracle):
    """1, 63, 64, 65 and 129 obstacles (the 64-lane stride: with 129 a lane holds three, and its later obstacle sits on the
    earlier vertex), and scenes where no corridor and no path accepts anything: no length is computed at all."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(2112)
    sc = _scenes(dm, cfg, 5300, 8, 129)
    first = _first(cfg)
    counts = (1, 63, 64, 65, 129)
    for s, m in enumerate(counts):
        xy = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 47.0 * s)
        _set_lane(dm, sc, s, xy, EGO, lanechg=s % 4)
        pts = _far(rng, m, xy)
        pts[m - 1] = _beside(xy, first + 20 + s, 0.1)                  # the winner: the LAST obstacle
        if m > 1:
            pts[0] = _beside(xy, first + 60, -0.2)                     # accepted, farther, first in j
        if m > 64:
            pts[m - 1 - 64] = _beside(xy, first + 45, 0.3)             # same lane of the wave as the winner, one stride earlier
        if m > 128:
            pts[m - 1 - 128] = _beside(xy, first + 30, 0.3)
        _set_obs(sc, s, pts)
    for s in range(len(counts), 8):
        xy = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 47.0 * s)
        _set_lane(dm, sc, s, xy, EGO, lanechg=s % 4)
        # far away, beside the lanes but outside every limit, and behind the rear corridor
        _set_obs(sc, s, _far(rng, 70 + s, xy) + [_beside(xy, first + 40, 12.0), _beside(xy, first + 70, -12.0), _beside(xy, 0, 0.0, -30.0)])
    plans, _ = _run(dm, oracle, cfg, sc, "counts / nothing accepted")
    a = plans[0]["around"]
    assert a["Obs_flag"][:5, 0].tolist() == [1] * 5 and a["Ob_Pathid"][:5, 0].tolist() == [20, 21, 22, 23, 24]
    assert not a["Obs_flag"][5:].any() and not plans[0]["ob_flag"][5:].any()


@pytest.mark.gpu
def test_ties(dm, oracle):
    """Same-vertex ties in both j orders; ties ACROSS vertices whose arc lengths are equal because the addition between them
    is absorbed (2e-16 m against 2400 m), in both j orders, with at most 64 obstacles (the tie run decides on the device) and
    with more (second pass); repeated lane points at the winner.  On corridor F (two waves) and on a pre-junction path
    (four waves)."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(2113)
    sc = _scenes(dm, cfg, 5400, 8, 90)
    first = _first(cfg)
    at = first + 60                                                       # F's vertex 60: 60 steps of 40 m behind vertex 0
    xy_t = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 15.0)
    xy_a = _absorbed_lane(dm.GEN_LANE_PTS, 1.0, 40.0, at)
    left, right = (1.0 - 0.3, xy_a[at, 1]), (1.0 + 0.3, xy_a[at, 1])       # nearest: point at | point at+1
    beyond = (1.1, xy_a[at + 3, 1] - 0.2)
    want = {}
    # 0, 1: two obstacles on one vertex, j's 1 and 75 apart
    for s, gap in ((0, 0), (1, 74)):
        _set_lane(dm, sc, s, xy_t, EGO, lanechg=s)
        a, b = _beside(xy_t, first + 33, 0.3), _beside(xy_t, first + 33, -0.25)
        pair = (a, b) if s == 0 else (b, a)
        _set_obs(sc, s, _far(rng, 4, xy_t) + [pair[0]] + _far(rng, gap, xy_t) + [pair[1]] + [_beside(xy_t, first + 50, 0.1)])
        want[s] = (33, pair[0])
    # 2 .. 5: the absorbed tie.  (scene, pre-junction?, far obstacles between the two, the larger j on the smaller vertex?)
    # With 63 far obstacles between them the two share a lane of the wave (j and j + 64) and the EARLIER j sits on the later
    # vertex of the run: the lane's pick (first obstacle on its smallest vertex) drops the winner, which is what the second pass
    # on `tie run and m > 64` is for.
    for s, junc, gap, swap in ((2, False, 2, True), (3, False, 63, True), (4, True, 3, False), (5, True, 63, True)):
        _set_lane(dm, sc, s, xy_a, EGO, lanechg=0)
        if junc:
            _pre_junction(sc, s)
        pair = (right, left) if swap else (left, right)
        _set_obs(sc, s, _far(rng, 3, xy_a) + [pair[0]] + _far(rng, gap, xy_a) + [pair[1], beyond])
        v0 = at - (EGO if junc else first)
        want[s] = (v0 + (1 if swap else 0), pair[0])
    # 6, 7: three equal lane points; the winner on the first of them (a tie run without a second obstacle in it)
    xy_r = xy_t.copy()
    xy_r[first + 41] = xy_r[first + 42] = xy_r[first + 40]
    for s, m_far in ((6, 5), (7, 80)):
        _set_lane(dm, sc, s, xy_r, EGO, lanechg=(0, 3)[s - 6])
        hit = tuple(xy_r[first + 40] + [0.01, 0.15])
        _set_obs(sc, s, _far(rng, m_far, xy_r) + [_beside(xy_r, first + 47, 0.1), hit, _beside(xy_r, first + 20, 9.0)])
        want[s] = (40, hit)
    plans, _ = _run(dm, oracle, cfg, sc, "ties")
    f = plans[0]["around"][:, 0]
    assert f["Obs_flag"].tolist() == [1] * 8
    for s, (v, ob) in want.items():
        assert f["Ob_Pathid"][s] == v and (f["Ob_Attr"]["x"][s], f["Ob_Attr"]["y"][s]) == ob, (s, f[s], v, ob)
    assert (f["Ob_Pose"]["dis_lng"][2:6] > 2048).all()


def _junction_path(dm, sc, s):
    """The front path of a (pre-)junction scene as k_decision / the reference build it (Decision.cpp:323-486)."""
    si = sc["scene_in"]
    loc, lv = si["loc"], si["lanes"]
    cur = sc["lane_pool"][int(lv["cur_off"][s]): int(lv["cur_off"][s]) + int(lv["cur_n"][s])]
    ref = sc["ref_pool"][int(si["ref_off"][s]): int(si["ref_off"][s]) + int(si["ref_n"][s])]
    cxy, rxy = np.stack([cur["x"], cur["y"]], axis=1), np.stack([ref["x"], ref["y"]], axis=1)
    if loc["pos"][s] == 1:
        i0 = max(int(loc["id"][s][min(max(int(loc["lane_num"][s]) - 1, 0), 7)]), 0)
        path = np.concatenate([cxy[i0:], rxy])
    else:
        i0 = max(int(loc["id"][s][min(max(int(loc["last_lanenum"][s]) - 1, 0), 7)]), 0)
        path = np.concatenate([rxy[i0:], cxy[:60]])
    return path[:dm.MAX_REFPATH]


@pytest.mark.gpu
def test_junction_paths(dm, oracle):
    """pos 1 and 2 (the whole block on the junction path): winners on its vertices 0, 7, 8, 9, 16, 17 and 40 (the last with
    129 obstacles), each behind an accepted obstacle farther along that comes first in j; one scene with nothing on the path."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(2114)
    sc = _scenes(dm, cfg, 5500, 16, 129, junction_every=2)
    si = sc["scene_in"]
    junc = [s for s in range(16) if si["loc"]["pos"][s] != 0][:8]
    assert {int(si["loc"]["pos"][s]) for s in junc} == {1, 2}
    for s in range(16):
        _set_obs(sc, s, [])
    verts = (0, 7, 8, 9, 16, 17, None, 40)
    for s, v in zip(junc, verts):
        path = _junction_path(dm, sc, s)
        assert len(path) > 70
        far = _far(rng, 127 if v == 40 else 20, path)
        if v is None:
            _set_obs(sc, s, far)
        else:
            _set_obs(sc, s, far[:5] + [_beside(path, 60, -0.2)] + far[5:] + [_beside(path, v, 0.1, 0.05 if v == 0 else 0.0)])
    plans, _ = _run(dm, oracle, cfg, sc, "junction paths")
    a = plans[0]["around"]
    assert a["Obs_flag"][junc, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 1]
    assert [int(a["Ob_Pathid"][s, 0]) for s, v in zip(junc, verts) if v is not None] == [v for v in verts if v is not None]


def _device_ticks(dm, cfg, sc, n_ticks=N_TICKS):
    n = len(sc["scene_in"])
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=max(n * sc["n_obs"], 1))
    st = sc["state"].copy()
    out = []
    for _ in range(n_ticks):
        plan, _ = pl.plan_tick_batch(sc, st, want_grid=False)
        out.append((plan.copy(), st.copy()))
    pl.close()
    return out


@pytest.mark.gpu
def test_same_scene_any_slot(dm, oracle):
    """One crafted scene alone, as scene 0 and as the last scene of a batch of five: its records are byte-identical."""
    cfg = _cfg(dm)
    first = _first(cfg)

    def craft(sc, s):
        rng = np.random.default_rng(2115)
        line = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 63.0)
        xy = line.copy()
        xy[first + 31] = xy[first + 30]                                   # a repeated point behind the winner's vertex
        _set_lane(dm, sc, s, xy, EGO, lanechg=1)
        _set_obs(sc, s, _far(rng, 30, line) + [_beside(line, first + 52, 0.2), _beside(line, first + 30, -0.1), _beside(line, first + 30, 0.3)] + _far(rng, 40, line))

    alone = _scenes(dm, cfg, 5600, 1, 80)
    craft(alone, 0)
    alone["scene_in"]["ref_n"][0] = 0
    want = _device_ticks(dm, cfg, alone)
    ref, _ = _run(dm, oracle, cfg, alone, "alone")
    assert ref[0]["around"]["Obs_flag"][0, 0] == 1 and ref[0]["around"]["Ob_Pathid"][0, 0] == 30
    for slot in (0, 4):
        five = _scenes(dm, cfg, 5601, 5, 80)
        craft(five, slot)
        # the same record and state as the scene alone (the generator draws lights, speeds ... per seed), at this slot's offsets
        si, lv = five["scene_in"], five["scene_in"]["lanes"]
        offs = (int(si["obs_off"][slot]), int(lv["cur_off"][slot]), int(lv["left_off"][slot]), int(lv["right_off"][slot]), int(si["ref_off"][slot]))
        si[slot] = alone["scene_in"][0]
        si["obs_off"][slot], lv["cur_off"][slot], lv["left_off"][slot], lv["right_off"][slot], si["ref_off"][slot] = offs
        si["ref_n"][slot] = 0
        five["state"][slot] = alone["state"][0]
        got = _device_ticks(dm, cfg, five)
        for t in range(N_TICKS):
            assert got[t][0][slot].tobytes() == want[t][0][0].tobytes(), (slot, t, compare(got[t][0][slot:slot + 1], want[t][0][:1]))
            assert got[t][1][slot].tobytes() == want[t][1][0].tobytes(), (slot, t)


@pytest.mark.gpu
def test_nan_lane_points(dm, oracle):
    """A NaN lane point DOES reach the kernels (k_validate_scenes / k_sanitise_scenes test offsets and counts only), so the
    second pass is reachable: a NaN point beyond the winner (two waves, four waves, more than 64 obstacles), a NaN point
    before the only accepted obstacle (its arc length is NaN), a scene with nothing accepted, and one whose answer only the
    second pass gives (see the last case).
    NOT covered, on purpose: accepted obstacles in DIFFERENT lanes of the wave of which one has a NaN arc length and comes
    first in j.  The
    reference then keeps that first one (`lng < NaN` is never true); the second pass is the sequence the kernels always ran,
    and its xor reduction on (lng, j) keeps whichever operand a NaN comparison leaves in place.  Measured on the device with
    this code: obstacles on vertices 60 (j = 3) and 40 (j = 4) behind a NaN point at 20 gave vertex 40, the oracle 60; on 70
    (j = 3) and 30 (j = 4) around a NaN point at 45 gave dis_lng 15.0, the oracle NaN.  That behaviour is older than the
    deferred sum and is left as it is."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(2116)
    sc = _scenes(dm, cfg, 5700, 7, 70)
    first = _first(cfg)
    base = _straight_xy(dm.GEN_LANE_PTS, 300.0, 400.0, 0.0)
    cases = [  # (NaN at path vertex, obstacles as (vertex, lat) in j order, far obstacles in front, pre-junction?)
        (80, [(30, 0.2), (50, -0.1)], 3, False),               # beyond the winner
        (80, [(50, -0.1), (30, 0.2)], 66, False),              # ... more than 64 obstacles
        (80, [(50, 0.1), (30, 0.2)], 2, True),                 # ... four waves
        (20, [(60, 0.2)], 3, False),                           # before it: the arc length is NaN
        (20, [(60, 0.2)], 3, True),
        (100, [], 5, False),                                   # nothing accepted
        # first in j an obstacle BEYOND the NaN point (its arc length is NaN), 64 later - the same lane of the wave - one before
        # it: the reference keeps the first (`lng < NaN` is false), and so does the lane's `first, or strictly smaller`; the
        # first pass alone would answer vertex 30 with a finite length.  This is the scene that needs the second pass.
        (45, [(70, 0.1), None, (30, 0.2)], 3, False),
    ]
    for s, (bad, near, n_far, junc) in enumerate(cases):
        xy = base.copy()
        v0 = EGO if junc else first
        xy[v0 + bad, 1] = np.nan
        _set_lane(dm, sc, s, xy, EGO, lanechg=0)
        sc["scene_in"]["loc"]["globalpoint"]["dir"][s] = 0.0
        if junc:
            _pre_junction(sc, s)
        pts = _far(rng, n_far, base)
        for q in near:                                          # None: 63 far obstacles
            pts += _far(rng, 63, base) if q is None else [_beside(base, v0 + q[0], q[1])]
        _set_obs(sc, s, pts)
    plans, _ = _run(dm, oracle, cfg, sc, "NaN lane points")
    f = plans[0]["around"][:, 0]
    assert f["Obs_flag"].tolist() == [1, 1, 1, 1, 1, 0, 1]
    assert f["Ob_Pathid"].tolist()[:5] == [30, 30, 30, 60, 60] and f["Ob_Pathid"][6] == 70
    assert np.isnan(f["Ob_Pose"]["dis_lng"][[3, 4, 6]]).all() and np.isfinite(f["Ob_Pose"]["dis_lng"][[0, 1, 2]]).all()
