"""The scoring pass with its candidates in registers (`score_body` of csrc/kernels_score.hpp): a lane computes its own point
of a pass and takes the neighbours i - 1 and i + 1 of the curvature term from the lanes beside it, the left-over candidate's
partial sums lie over the obstacle lists.  Crafted scenes that sit on the lane borders of that form - passes of 64 points,
the packed fourth pass, the quarters of the left-over candidate - and on the sizes at which its loads and lists change.

Grid 96 x 64 cells of 0.25 m (24 m x 16 m), default config, static obstacles.  Scenes are built with score_scenes.build (its
padding discs and pool layout) and then moved onto this grid: ego at origin + (2, 8), goal at origin + (22, 8) unless a case
says otherwise.  References: the oracle and the 40-digit model (grid_score_model), with the bars of test_score_edges.py -
integers and cand_prog exact, floats within parity_util.RTOL / ATOL.  GPU: every case alone (sixteen waves), in a batch of
kScoreWideMaxScenes (sixteen waves) and in a batch of one more (four waves), against both references, and the whole GridOut
record byte for byte the same in the three."""
import math

import numpy as np
import pytest

import grid_score_model as gm
import score_scenes as ss
import test_score_edges as tse
from parity_util import compare

GRID_W, GRID_H = 96, 64
EGO, GOAL, HEADING = (2.0, 8.0), (22.0, 8.0), 25.0
HIT_POINTS = (63, 64, 127, 128, 191, 192, 198, 199)
HIT_CANDIDATE = 15                     # lateral offset +2.4 m at the terminal: clear of the pebble that blocks the goal
# Bend scene: the goal 19 cells above and 80 cells right of the ego's cell; the path's one corner lies 19 diagonal steps (or
# 19 straight ones) from the start, and the look-ahead cuts the other leg so that the corner falls between two points
BEND_GOAL = (EGO[0] + 80 * 0.25, EGO[1] + 19 * 0.25)
BEND_BORDERS = (63, 127, 191)          # the corner between points b and b + 1
LATTICES = (0, 1, 3, 4, 5, 15, 16)
PREFIX_POINTS = (1, 2, 3, 8, 9, 64, 65, 121)
SNAPSHOT_SIZES = (0, 1, 255, 256, 257)

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _cfg(dm, n_lattice=16, lookahead=120):
    cfg = dm.default_config(GRID_W, GRID_H)
    cfg["dynamic_obstacles"] = 0
    cfg["n_lattice"], cfg["lookahead_cells"] = n_lattice, lookahead
    return cfg


def _spec(name, discs=(), heading=HEADING, ego=EGO, goal=GOAL):
    return dict(name=name, discs=list(discs), heading=heading, ego=ego, goal=goal)


def _build(dm, cfg, specs, n_obs):
    """One scene per spec, `n_obs` obstacles each: score_scenes' padding discs first, the spec's discs last."""
    sc = ss.build(dm, cfg, ["n_rel_0"] * len(specs), n_obs)
    si = sc["scene_in"]
    for s, sp in enumerate(specs):
        assert len(sp["discs"]) <= n_obs, (sp["name"], len(sp["discs"]), n_obs)
        ox, oy = float(si["grid_origin"]["x"][s]), float(si["grid_origin"]["y"][s])
        ob = sc["obs_pool"][s * n_obs:(s + 1) * n_obs]
        for j, (x, y, r) in enumerate(sp["discs"]):
            q = n_obs - len(sp["discs"]) + j
            ob[q]["x"], ob[q]["y"], ob[q]["radius"], ob[q]["type"] = ox + x, oy + y, r, 0
        gp = si["loc"]["globalpoint"]
        gp["x"][s], gp["y"][s], gp["dir"][s] = ox + sp["ego"][0], oy + sp["ego"][1], sp["heading"]
        si["goal"]["x"][s], si["goal"]["y"][s] = ox + sp["goal"][0], oy + sp["goal"][1]
    return sc


def _reference(dm, oracle, specs, n_obs, n_lattice=16, lookahead=120):
    """Oracle GridOut + path, model and form of one scene per spec (computed once per process, never modified)."""
    def make():
        cfg = _cfg(dm, n_lattice, lookahead)
        sc = _build(dm, cfg, specs, n_obs)
        k = ss.kernel_constants()
        out = []
        for s, sp in enumerate(specs):
            _, go, _, _, path = oracle.plan_tick_one(cfg, sc, s, sc["state"].copy())
            obs = ss.scene_obstacles(sc, s)
            status = int(go["status"])
            path = path[:max(int(go["path_len"]), 0)].copy()
            out.append(dict(name=sp["name"], gout=go.copy(), path=path, model=gm.score_scene(cfg, sc["scene_in"][s], obs, path, status),
                            form=ss.forms(cfg, sc["scene_in"][s], obs, path, status, k)))
        return out
    return _cached(("ref", tuple(sp["name"] for sp in specs), n_obs, n_lattice, lookahead), make)


# ---- the crafted scenes --------------------------------------------------------------------------------------------------
GOAL_PEBBLE = (GOAL[0], GOAL[1], 0.1)           # on the goal: the search ends without a path, the terminal is the goal itself


def _lattice_points(k, nl=16):
    """Candidate k of a scene WITHOUT a grid path (terminal = goal, terminal heading = ego -> goal), float64: for placing discs."""
    pi = math.pi
    thT = math.degrees(math.atan2(GOAL[1] - EGO[1], GOAL[0] - EGO[0]))
    off = (k - (nl - 1) // 2) * 0.3
    ex, ey = GOAL[0] + off * math.sin(thT * pi / 180), GOAL[1] - off * math.cos(thT * pi / 180)
    d = math.hypot(ex - EGO[0], ey - EGO[1]) / 3
    x1, y1 = EGO[0] + d * math.cos(HEADING * pi / 180), EGO[1] + d * math.sin(HEADING * pi / 180)
    x2, y2 = ex - d * math.cos(thT * pi / 180), ey - d * math.sin(thT * pi / 180)
    t = np.arange(200) / 199.0
    u = 1 - t
    return np.stack([u ** 3 * EGO[0] + 3 * u * u * t * x1 + 3 * u * t * t * x2 + t ** 3 * ex,
                     u ** 3 * EGO[1] + 3 * u * u * t * y1 + 3 * u * t * t * y2 + t ** 3 * ey], -1)


def _hit_spec(i):
    """A pebble ahead of point i of HIT_CANDIDATE, half a point spacing inside the contact distance of point i: point i is the
    first one the vehicle's half width reaches (point i - 1 stays ~6 cm clear)."""
    P = _lattice_points(HIT_CANDIDATE)
    a, b = (P[i - 1], P[i + 1]) if i < 199 else (P[i - 1], P[i])
    u = (b - a) / np.hypot(*(b - a))
    spacing = float(np.hypot(*(P[i] - P[i - 1])))
    c = P[i] + u * (0.1 + 0.9 - 0.5 * spacing)
    return _spec(f"hit_{i}", [GOAL_PEBBLE, (float(c[0]), float(c[1]), 0.1)])


def _line(k, y=11.2):
    """k discs of radius 0.1 beside the candidates, x from 4 to 20: all inside the cull box, none touching a candidate."""
    if k == 0:
        return []
    if k == 1:
        return [(12.0, y, 0.1)]
    return [(4.0 + 16.0 * i / (k - 1), y, 0.1) for i in range(k)]


def _clump(k):
    return [(12.0 + 0.01 * i, 10.6, 0.1) for i in range(k)]


# three walls with gaps at alternating ends: a grid path of more than 121 cells with many corners
MAZE = _spec("maze", [(6.0, 0.5 + i, 0.5) for i in range(11)] + [(12.0, 15.5 - i, 0.5) for i in range(11)] + [(18.0, 0.5 + i, 0.5) for i in range(11)],
             heading=90.0, ego=(2.0, 2.0), goal=(22.0, 2.0))
BEND = _spec("bend", [], heading=0.0, goal=BEND_GOAL)
FOUND = _spec("found", _line(7))
BLOCKED = _spec("blocked", _line(7) + [(GOAL[0], GOAL[1], 1.0)])
MAIN_N_OBS = 132
MAIN = [_hit_spec(i) for i in HIT_POINTS] + [_spec(f"line_{k}", _line(k)) for k in (7, 8, 128, 129)] + [_spec("clump_13", _clump(13)), FOUND, BLOCKED]


def _bend_lookaheads(path, W):
    """For each border b of BEND_BORDERS a look-ahead that puts the path's single corner between points b and b + 1 of the
    resampled prefix, well inside (0.1 .. 0.9 of the way; rounding moves it by ~1e-13): {b: lookahead}."""
    cx, cy = path % W, path // W
    step = np.hypot(np.diff(cx), np.diff(cy))                 # 1 or sqrt 2, in cells
    turn = [j for j in range(1, len(step)) if step[j] != step[j - 1]]
    assert len(turn) == 1, ("the bend scene's path has one corner", turn)
    cum = np.concatenate([[0.0], np.cumsum(step)])
    out = {}
    for b in BEND_BORDERS:
        for la in range(turn[0] + 1, len(path)):
            pos = 199.0 * cum[turn[0]] / cum[la]
            if b + 0.1 <= pos <= b + 0.9:
                out[b] = la
                break
    return out


def _bend(dm, oracle):
    def make():
        r = _reference(dm, oracle, [BEND], 4)[0]
        assert int(r["gout"]["status"]) == 0
        return _bend_lookaheads(r["path"].astype(np.int64), GRID_W)
    return _cached("bend", make)


def _prefix_runs(dm, oracle):
    """(lookahead, specs) of the path-prefix group: the maze on every prefix length, the bend on its three look-aheads."""
    runs = [(p - 1, [MAZE, BLOCKED]) for p in PREFIX_POINTS]
    runs += [(la, [BEND, BLOCKED]) for la in sorted(_bend(dm, oracle).values())]
    return runs


def _all_references(dm, oracle):
    refs = [(f"{r['name']}/main", r) for r in _reference(dm, oracle, MAIN, MAIN_N_OBS)]
    for nl in LATTICES:
        refs += [(f"{r['name']}/n_lattice {nl}", r) for r in _reference(dm, oracle, [FOUND, BLOCKED], 16, n_lattice=nl)]
    for la, specs in _prefix_runs(dm, oracle):
        refs += [(f"{r['name']}/lookahead {la}", r) for r in _reference(dm, oracle, specs, 40, lookahead=la)]
    for m in SNAPSHOT_SIZES:
        refs += [(f"{r['name']}/{m} obstacles", r) for r in _reference(dm, oracle, _snapshot_specs(m), m)]
    return refs


def _snapshot_specs(m):
    k = min(m, 129)
    return [_spec(f"snap_{m}", _line(k)), _spec(f"snap_{m}_blocked", _line(max(k - 1, 0)) + ([(GOAL[0], GOAL[1], 1.0)] if m else []))]


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_oracle_scores_equal_the_model(dm, oracle):
    bad, worst = [], 0.0
    for tag, r in _all_references(dm, oracle):
        b, w = tse._against_model(r["gout"], r["model"], tag)
        bad += b
        worst = max(worst, w)
    print(f"oracle against model, largest relative difference: {worst:.3g}")
    assert not bad, "\n".join(bad[:20])


def test_cases_keep_away_from_the_discontinuities(dm, oracle):
    """No point of any case comes near clearance = 0 or the fence sinA = 0.001 (the bars of test_score_edges.py)."""
    bad = []
    for tag, r in _all_references(dm, oracle):
        m = r["model"]
        if m["min_abs_clearance"] < tse.MIN_ABS_CLEARANCE:
            bad.append(f"{tag}: a point with |clearance| = {m['min_abs_clearance']:.3g} m")
        if m["min_fence"] < tse.MIN_FENCE:
            bad.append(f"{tag}: a point {m['min_fence']:.3g} (relative) from the fence sinA = 0.001")
    assert not bad, "\n".join(bad)


def test_first_hits_land_on_the_lane_borders(dm, oracle):
    """Point i of candidate HIT_CANDIDATE is the first one hit, for every i of HIT_POINTS: the last and first lanes of a pass
    (63 | 64, 127 | 128, 191 | 192) and the packed pass's own ends (192, 198, 199).  No grid path: sixteen candidates, four
    whole rounds on four waves and the packed pass."""
    refs = {r["name"]: r for r in _reference(dm, oracle, MAIN, MAIN_N_OBS)}
    for i in HIT_POINTS:
        r = refs[f"hit_{i}"]
        assert int(r["gout"]["status"]) != 0 and r["model"]["n_candidates"] == 16
        assert r["model"]["cand_prog"][HIT_CANDIDATE] == (200 - i) / 200, (i, r["model"]["cand_prog"][HIT_CANDIDATE])
        assert r["model"]["cand_col"][HIT_CANDIDATE] >= 1000.0
    assert ss.schedule(4, 16) == dict(rounds=4, split=0, packed=True)


def test_bend_puts_the_largest_curvature_term_on_the_pass_borders(dm, oracle):
    """The bend scene's path is two straight legs; with the look-aheads of _bend_lookaheads its corner lies between points b and
    b + 1, so the two largest curvature terms of the grid-path candidate are those of b and b + 1 (each reads the other)."""
    las = _bend(dm, oracle)
    assert set(las) == set(BEND_BORDERS), las
    for b, la in las.items():
        r = _reference(dm, oracle, [BEND, BLOCKED], 40, lookahead=la)[0]
        cfg = _cfg(dm, lookahead=la)
        sc = _build(dm, cfg, [BEND], 40)
        gx, gy = float(sc["scene_in"]["grid_origin"]["x"][0]), float(sc["scene_in"]["grid_origin"]["y"][0])
        cells = r["path"][:r["form"]["a"] + 1].astype(np.int64)
        pin = [(gm._num(gx) + (gm._num(int(c % GRID_W)) + gm._num(0.5)) * gm._num(0.25), gm._num(gy) + (gm._num(int(c // GRID_W)) + gm._num(0.5)) * gm._num(0.25)) for c in cells]
        P = np.array([[float(x), float(y)] for x, y in gm.mean_points(cfg, pin)])
        d1, d2, d3 = np.hypot(*(P[1:-1] - P[:-2]).T), np.hypot(*(P[2:] - P[1:-1]).T), np.hypot(*(P[2:] - P[:-2]).T)
        cos_a = (d1 * d1 + d2 * d2 - d3 * d3) / (2 * d1 * d2)
        k2 = (1 - cos_a * cos_a) / (0.25 * d3 * d3)
        top = set((np.argsort(-k2)[:2] + 1).tolist())
        assert top == {b, b + 1}, (b, la, top)
        assert r["form"]["have_path"] and r["model"]["n_candidates"] == 17


def test_case_list_covers_the_sizes_the_register_form_splits_on(dm, oracle):
    k = ss.kernel_constants()
    main = {r["name"]: r for r in _reference(dm, oracle, MAIN, MAIN_N_OBS)}
    # the partial sums of the left-over candidate lie over the lists these scenes read until their last point: a found path
    # (17 candidates: the grid path is left over on four waves and on sixteen) with 7 | 8 and 128 | 129 culled obstacles, a full bucket + 1
    for n in (7, 8, 128, 129):
        f = main[f"line_{n}"]["form"]
        assert f["n_rel"] == n and f["have_path"] and f["nc"] == 17, (n, f["n_rel"], f["nc"])
    assert {main[f"line_{n}"]["form"]["form"] for n in (7, 8, 128, 129)} == {"lds_plain", "lds_buckets", "snapshot_buckets"}
    assert main["clump_13"]["form"]["fullest"] == k["kBucketCap"] + 1 and main["clump_13"]["form"]["nc"] == 17
    assert ss.schedule(4, 17)["split"] == 1 and ss.schedule(16, 17)["split"] == 1
    # candidate counts: found scenes give n_lattice + 1, blocked ones n_lattice
    seen = set()
    for nl in LATTICES:
        found, blocked = _reference(dm, oracle, [FOUND, BLOCKED], 16, n_lattice=nl)
        assert found["form"]["nc"] == nl + 1 and blocked["form"]["nc"] == nl and int(blocked["gout"]["status"]) != 0
        seen |= {found["form"]["nc"], blocked["form"]["nc"]}
    kinds = {(nw, s["rounds"] > 0, s["split"] > 0, s["packed"]) for nw in (4, 16) for nc in seen for s in [ss.schedule(nw, nc)]}
    assert {(4, True, True, True), (4, True, False, True), (4, True, False, False), (4, False, True, False), (4, False, False, False),
            (16, False, True, False), (16, True, True, False), (16, True, False, False), (16, False, False, False)} <= kinds, kinds
    # path prefixes: the maze is long enough for the look-ahead cap
    for p in PREFIX_POINTS:
        r = _reference(dm, oracle, [MAZE, BLOCKED], 40, lookahead=p - 1)[0]
        assert int(r["gout"]["status"]) == 0 and int(r["gout"]["path_len"]) >= 121 and r["form"]["a"] + 1 == p, (p, int(r["gout"]["path_len"]), r["form"]["a"])
    # snapshot sizes: one record per thread up to 256, the first size beyond; both culled and not
    for m in SNAPSHOT_SIZES:
        found, blocked = _reference(dm, oracle, _snapshot_specs(m), m)
        assert found["form"]["m"] == m and int(found["gout"]["status"]) == 0 and (m == 0 or int(blocked["gout"]["status"]) != 0)
    assert {_reference(dm, oracle, _snapshot_specs(m), m)[0]["form"]["form"] for m in (255, 256, 257)} >= {"snapshot_buckets", "hbm_plain"}


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _planner(dm, cfg, n, n_obs):
    return dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=max(n * n_obs, 1))


def _run(pl, sc):
    pl.set_scenes(sc)
    pl.set_state(sc["state"])
    pl.tick(sync=True)
    return pl.get_grid_out()


def _three_schedules(dm, oracle, specs, n_obs, steps, field=None):
    """`specs` alone, in the wide batch and in the narrow batch, one handle per setting, the config stepped through `steps`
    ([(value, specs)] with set_config, or [(None, specs)]): mismatches against oracle and model, and records that are not the
    same bytes in the three settings."""
    bad = []
    widths = dict(alone=1, **tse._widths())
    cfg0 = _cfg(dm)
    pls = {w: _planner(dm, cfg0, n, n_obs) for w, n in widths.items()}
    try:
        for value, sp in steps:
            kw = {} if field is None else {field: value}
            cfg = _cfg(dm, **kw)
            refs = _reference(dm, oracle, sp, n_obs, **kw)
            out = {}
            for w, n in widths.items():
                pls[w].set_config(cfg)
                if w == "alone":
                    out[w] = np.concatenate([_run(pls[w], _build(dm, cfg, [one], n_obs)) for one in sp])
                else:
                    out[w] = _run(pls[w], _build(dm, cfg, tse._fill(sp, n), n_obs))
                bad += tse._check(out[w], refs, f"{w}/{field} {value}")
            for w in ("wide", "narrow"):
                for i in range(len(out[w])):
                    c = i % len(sp)
                    if out[w][i].tobytes() != out["alone"][c].tobytes():
                        bad.append(f"{field} {value} {sp[c]['name']}: record {i} of the {w} batch differs from the scene alone: " +
                                   "; ".join(compare(out[w][i:i + 1], out["alone"][c:c + 1], "", rtol=0.0, atol=0.0)))
    finally:
        for pl in pls.values():
            pl.close()
    return bad


@pytest.mark.gpu
def test_device_lane_borders_and_overlaid_partial_sums(dm, oracle):
    """First hits on the pass borders and in the packed pass, and the left-over candidate beside 7 | 8 and 128 | 129 culled
    obstacles and a bucket of 13."""
    bad = _three_schedules(dm, oracle, MAIN, MAIN_N_OBS, [(None, MAIN)])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
def test_device_candidate_counts(dm, oracle):
    """n_lattice 16 .. 0 with and without a found path: quarter split on and off, packed pass on and off, no candidate at all."""
    bad = _three_schedules(dm, oracle, [FOUND, BLOCKED], 16, [(nl, [FOUND, BLOCKED]) for nl in sorted(LATTICES, reverse=True)], "n_lattice")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
def test_device_path_prefixes_and_bends(dm, oracle):
    """Prefixes of 1 .. 121 points of a path with many corners, and one corner on 63 | 64, 127 | 128 and 191 | 192.  A blocked
    scene rides along in every batch: its path cells are those an earlier tick left behind."""
    bad = _three_schedules(dm, oracle, [MAZE, BLOCKED], 40, _prefix_runs(dm, oracle), "lookahead")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("m", SNAPSHOT_SIZES)
def test_device_snapshot_sizes(dm, oracle, m):
    """0, 1, 255, 256 and 257 obstacles in the scene's snapshot."""
    sp = _snapshot_specs(m)
    bad = _three_schedules(dm, oracle, sp, m, [(None, sp)])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
def test_device_no_path_over_stale_path_cells(dm, oracle):
    """Every scene of a handle finds a path in one tick and none in the next: the path cells of the first tick are still in the
    handle's buffer while the second is scored, and nothing of them shows."""
    bad = []
    cfg = _cfg(dm)
    for w, n in dict(alone=1, **tse._widths()).items():
        pl = _planner(dm, cfg, n, 40)
        try:
            first = _run(pl, _build(dm, cfg, [MAZE] * n, 40))
            assert np.all(first["status"] == 0) and np.all(first["path_len"] >= 121)
            bad += tse._check(_run(pl, _build(dm, cfg, [BLOCKED] * n, 40)), _reference(dm, oracle, [BLOCKED], 40), f"{w}/stale")
        finally:
            pl.close()
    assert not bad, "\n".join(bad[:20])
