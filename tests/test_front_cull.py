"""team_search_obstacle (csrc/dev_geom.hpp) on crafted scenes, and a prior check of the maths of an obstacle cull.

GPU: full ticks of crafted scenes, device against the oracle.  The team splits a corridor's points into one share per wave
(two waves: n/4 | 3n/4, four waves: nothing | three thirds); test_share_boundaries puts an obstacle at every vertex of
front paths and junction paths of 2 to 9 points, so each boundary of each split is the nearest vertex once.  The other GPU
tests are lane shapes and obstacle lists (bends, repeated points, NaN obstacles, ties on the arc length, 0 to 257
obstacles) that any form of the search, brute force or culled, has to get right.
CPU: the kernels do NOT cull obstacles (a cull was built and measured slower, profiles/r17_front_cull.txt).  The two
certificate tests check only the geometry a later cull would rest on: a numpy keep rule (path statistics, enable rule,
radius, chunk boxes) against oracle.SearchObstacle - the answer over the kept obstacles, in original indices, must be the
answer over all of them.  They exercise no device code and say nothing about what the device does."""
import numpy as np
import pytest

from parity_util import compare

CHUNK = 16
# An addition to the enable rule of the cull's design: beyond this magnitude the rule is off (path) or the obstacle is kept.
# The nearest vertex is picked from ROUNDED squared distances; far enough away they tie, the first vertex wins and an
# obstacle on the line of segment 0 is accepted - the geometric bound does not cover that.  Within 1e5 m the rounding moves
# the bound by under 0.05 m, inside the radius' slack of a metre.
COORD_MAX = 1e5


# ---------------------------------------------------------------------------------------------------------------------
# the certificate, in numpy
def cull_keep(eps, px, py, ox, oy, lo, hi):
    """(on, keep[m]) of the keep rule under test."""
    n, m = len(px), len(ox)
    keep_all = np.ones(m, bool)
    if n < 2:
        return False, keep_all
    dx, dy = np.diff(px), np.diff(py)
    with np.errstate(all="ignore"):
        ln = np.sqrt(dx * dx + dy * dy)
        hmax, hmin = ln.max(), ln.min()
        cmin = np.inf
        if n >= 3:
            cmin = ((dx[1:] * dx[:-1] + dy[1:] * dy[:-1]) / (ln[1:] * ln[:-1])).min()
        finite = bool(np.all(np.abs(px) <= COORD_MAX) and np.all(np.abs(py) <= COORD_MAX))
        on = finite and hmin >= 1e-3 and cmin >= 0.5 and eps <= 1e-3 * hmin and np.isfinite(lo) and np.isfinite(hi)
    if not on:
        return False, keep_all
    R = 2 * hmax + 4 * max(abs(lo), abs(hi)) + 1
    keep = ~((np.abs(ox) <= COORD_MAX) & (np.abs(oy) <= COORD_MAX))          # NaN or far beyond the certified range: kept
    for k in range(0, n, CHUNK):
        xmin, xmax = px[k:k + CHUNK].min() - R, px[k:k + CHUNK].max() + R
        ymin, ymax = py[k:k + CHUNK].min() - R, py[k:k + CHUNK].max() + R
        keep |= ~((ox < xmin) | (ox > xmax) | (oy < ymin) | (oy > ymax))
    return True, keep


def chunk_boxes(px, py, lo, hi):
    ln = np.hypot(np.diff(px), np.diff(py))
    R = 2 * ln.max() + 4 * max(abs(lo), abs(hi)) + 1
    return R, [(px[k:k + CHUNK].min(), px[k:k + CHUNK].max(), py[k:k + CHUNK].min(), py[k:k + CHUNK].max())
               for k in range(0, len(px), CHUNK)]


# ---------------------------------------------------------------------------------------------------------------------
# paths
def _wavy(n, rng):
    x = np.cumsum(rng.uniform(0.3, 0.7, n)) + rng.uniform(0, 60)
    return x, rng.uniform(10, 110) + 2.5 * np.sin(x / 7.0)


def _straight(n, heading_deg, x0=64.0, y0=64.0, h=0.5):
    k = np.arange(n, dtype=np.float64)
    if heading_deg == "vertical":
        return np.full(n, x0), y0 + h * k
    if heading_deg == "near-vertical":                  # |dx| of a segment is half of EPSILON: GetLatDis takes it for vertical
        return x0 + 5e-7 * k, y0 + h * k
    if heading_deg == "near-vertical-out":              # ... and twice EPSILON: the slope branch with a huge slope
        return x0 + 2e-6 * k, y0 - h * k
    a = np.radians(heading_deg)
    return x0 + h * np.cos(a) * k, y0 + h * np.sin(a) * k


def _bend(n, at, bend_deg, heading_deg=10.0, h=0.5):
    a0, a1 = np.radians(heading_deg), np.radians(heading_deg + bend_deg)
    x, y = [64.0], [64.0]
    for i in range(1, n):
        a = a0 if i <= at else a1
        x.append(x[-1] + h * np.cos(a)); y.append(y[-1] + h * np.sin(a))
    return np.array(x), np.array(y)


def _adversarial(px, py, lo, hi, bends=()):
    """Obstacles where a wrong certificate would show."""
    pts = []
    n = len(px)
    for k in bends:                                     # backward extension of the segment after the bend
        if 0 < k < n - 1:
            ux, uy = px[k + 1] - px[k], py[k + 1] - py[k]
            u = np.hypot(ux, uy)
            for d in (5.0, 20.0, 100.0):
                pts.append((px[k] - d * ux / u, py[k] - d * uy / u))
    if n >= 2:
        R, boxes = chunk_boxes(px, py, lo, hi)
        if np.isfinite(R):
            for (x0, x1, y0, y1) in boxes:              # both sides of every edge of every inflated box
                cx, cy = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
                for e in (-1e-9, 1e-9):
                    pts += [(x0 - R + e, cy), (x1 + R + e, cy), (cx, y0 - R + e), (cx, y1 + R + e)]
        for (a, b) in ((0, 1), (n - 2, n - 1)):         # on the lines through the two end segments, beyond both ends
            ux, uy = px[b] - px[a], py[b] - py[a]
            u = np.hypot(ux, uy)
            if u > 0:
                for d in (0.2, 3.0, 9.0, 40.0):
                    pts += [(px[a] - d * ux / u, py[a] - d * uy / u), (px[b] + d * ux / u, py[b] + d * uy / u)]
    return pts


def _check_path(dm, oracle, cfg, px, py, rng, lo, hi, bends=(), n_uniform=48):
    """oracle.SearchObstacle over the kept obstacles == over all of them; returns (on, dropped)."""
    eps = float(cfg["EPSILON"][0])
    n = len(px)
    p = np.zeros(n, dm.GlobalPoint2D)
    p["x"], p["y"] = px, py
    adv = _adversarial(px, py, lo, hi, bends)
    m = n_uniform + len(adv) + 1
    o = np.zeros(m, dm.ObPoint)
    o["x"][:n_uniform], o["y"][:n_uniform] = rng.uniform(0, 128, n_uniform), rng.uniform(0, 128, n_uniform)
    if adv:
        o["x"][n_uniform:m - 1], o["y"][n_uniform:m - 1] = np.array(adv).T
    o["x"][m - 1], o["y"][m - 1] = 3.0e5, py[0]                    # beyond the certified range: kept
    order = rng.permutation(m)
    o = o[order]
    o["type"] = np.arange(m)                                       # the original index travels in the record
    o["radius"] = 0.5
    on, keep = cull_keep(eps, px, py, o["x"], o["y"], lo, hi)
    if not on:
        assert keep.all()
    full = oracle.SearchObstacle(cfg, p, o, lo, hi)
    kept = oracle.SearchObstacle(cfg, p, o[keep], lo, hi)
    for f in ("flag", "dis_lat", "dis_lng", "path_id"):
        assert full[f] == kept[f] or (full[f] != full[f] and kept[f] != kept[f]), (f, full, kept, n, lo, hi)     # (NaN: a NaN path point)
    if full["flag"]:
        assert full["ob"].tobytes() == kept["ob"].tobytes(), (full, kept)
    return on, int((~keep).sum())


def test_cull_certificate_friendly_paths(dm, oracle):
    cfg = dm.default_config(128)
    rng = np.random.default_rng(1701)
    total = good = 0
    for k in range(120):                                           # wavy lanes, n from 2 to 200
        n = (2, 3, 15, 16, 17, 200)[k] if k < 6 else int(rng.integers(2, 201))
        px, py = _wavy(n, rng)
        lo, hi = ((-0.9, 0.9), (-0.9, 1.875), (-1.875, 0.9), (-float(rng.uniform(0.5, 2)), float(rng.uniform(0.5, 2))))[k % 4]
        on, dropped = _check_path(dm, oracle, cfg, px, py, rng, lo, hi)
        total += 1; good += bool(on and dropped > 0)
    headings = list(np.arange(0.0, 360.0, 7.5)) + [90.0, 270.0, 89.9999, 90.0001, "vertical", "near-vertical", "near-vertical-out"]
    for k, hd in enumerate(headings):                              # straight lanes at every heading
        n = (2, 40, 120, 200)[k % 4]
        px, py = _straight(n, hd)
        on, dropped = _check_path(dm, oracle, cfg, px, py, rng, -0.9, 0.9)
        total += 1; good += bool(on and dropped > 0)
    # the test proves something only if the cull is on and drops obstacles on nearly all of these
    assert good >= 0.9 * total, (good, total)


def test_cull_certificate_bends_and_bunched_points(dm, oracle):
    cfg = dm.default_config(128)
    rng = np.random.default_rng(1702)
    eps = float(cfg["EPSILON"][0])
    seen = {}
    for bend in (30.0, 59.0, 61.0, 90.0, 150.0, -30.0, -59.0, -61.0, -90.0, -150.0):
        for n, at in ((3, 1), (40, 7), (120, 16), (120, 63), (200, 150)):
            px, py = _bend(n, at, bend, heading_deg=float(rng.uniform(0, 360)))
            on, _ = _check_path(dm, oracle, cfg, px, py, rng, -0.9, 0.9, bends=(at,))
            seen[abs(bend)] = on
            # the obstacle 20 m back on the extension IS accepted by the reference rule past a sharp bend: the fallback matters
            if abs(bend) >= 90:
                p = np.zeros(n, dm.GlobalPoint2D); p["x"], p["y"] = px, py
                ux, uy = px[at + 1] - px[at], py[at + 1] - py[at]
                o = np.zeros(1, dm.ObPoint); o["x"], o["y"] = px[at] - 40 * ux, py[at] - 40 * uy
                assert oracle.SearchObstacle(cfg, p, o, -0.9, 0.9)["flag"] == 1
    assert seen == {30.0: True, 59.0: True, 61.0: False, 90.0: False, 150.0: False}
    # Bezier paths: 200 points bunched towards the ends, from 60 m long down to shorter than the enable rule allows
    for length in (60.0, 20.0, 2.0, 0.5, 0.05):
        for turn in (0.0, 40.0, 170.0):
            s = (20.0, 30.0, float(rng.uniform(0, 360)))
            e = (s[0] + length * np.cos(np.radians(s[2] + 10)), s[1] + length * np.sin(np.radians(s[2] + 10)), s[2] + turn)
            b = oracle.BezierPlanning(cfg, s, e)
            for cut in (0, 57, 198):
                on, _ = _check_path(dm, oracle, cfg, b["x"][cut:].copy(), b["y"][cut:].copy(), rng, -1.1, 1.1)
                if length <= 0.05:
                    assert not on                                   # segments under a millimetre: nothing may be dropped
    # repeated point, NaN point, infinite bound, far-away path: the rule says OFF, nothing dropped
    px, py = _straight(50, 33.0)
    for mut in ("dup", "nan", "inf", "far", "eps"):
        qx, qy, lo, hi, c2 = px.copy(), py.copy(), -0.9, 0.9, cfg
        if mut == "dup": qx[20], qy[20] = qx[19], qy[19]
        if mut == "nan": qy[31] = np.nan
        if mut == "inf": hi = np.inf
        if mut == "far": qx += 2.0e5
        if mut == "eps": c2 = cfg.copy(); c2["EPSILON"] = 1e-3
        on, keep = cull_keep(float(c2["EPSILON"][0]), qx, qy, np.array([0.0]), np.array([0.0]), lo, hi)
        assert not on and keep.all(), mut
        _check_path(dm, oracle, c2, qx, qy, rng, lo, hi)
    assert cull_keep(eps, px, py, np.array([np.nan, 0.0, 0.0]), np.array([0.0, np.nan, 0.0]), -0.9, 0.9)[1].tolist() == [True, True, False]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: full ticks on crafted scenes
N_TICKS = 3          # the sweep needs obsavoid_time + 1 > 2: the third tick


def _lane_points(dm, xy, dirs):
    p = np.zeros(len(xy), dm.GlobalPoint3D)
    p["x"], p["y"], p["dir"] = xy[:, 0], xy[:, 1], dirs
    return p


def _set_lane(dm, sc, s, xy, ego_id, lanechg=0, lane_num=2, width=3.75):
    """Scene s drives the polyline xy (GEN_LANE_PTS points or fewer); its neighbours are the same polyline shifted sideways."""
    n = dm.GEN_LANE_PTS
    k = len(xy)
    assert k <= n
    d = np.diff(xy, axis=0)
    dirs = np.degrees(np.arctan2(d[:, 1], d[:, 0])) % 360.0
    dirs = np.concatenate([dirs, dirs[-1:]])
    dirs = np.where(np.isfinite(dirs), dirs, 0.0)
    si = sc["scene_in"]
    base = s * 3 * n
    for slot, shift in ((0, 0.0), (1, width), (2, -width)):
        sc["lane_pool"][base + slot * n: base + slot * n + k] = _lane_points(dm, xy + np.array([0.0, shift]), dirs)
    lv = si["lanes"]
    lv["cur_off"][s], lv["cur_n"][s] = base, k
    lv["left_off"][s], lv["left_n"][s] = base + n, (k if lane_num > 1 else 0)
    lv["right_off"][s], lv["right_n"][s] = base + 2 * n, (k if lane_num < 3 else 0)
    lv["lanechg_attribute"][s], lv["lane_width"][s], lv["lane_sum"][s] = lanechg, width, 3
    sc["attr_pool"][base: base + 3 * n] = lanechg
    loc = si["loc"]
    loc["pos"][s], loc["lane_num"][s], loc["last_lanenum"][s], loc["next_lanenum"][s] = 0, lane_num, lane_num, lane_num
    loc["id"][s] = ego_id
    e = min(ego_id, k - 1)
    loc["globalpoint"]["x"][s], loc["globalpoint"]["y"][s], loc["globalpoint"]["dir"][s] = xy[e, 0], xy[e, 1], dirs[e]
    loc["velocity"][s] = 12.0
    si["dec"]["target_lanenum"][s] = lane_num
    st = sc["state"]
    st["z_target_lanenum"][s], st["d_his_target_lanenum"][s] = lane_num, lane_num


def _set_obs(sc, s, pts):
    """Scene s sees exactly `pts` (list of (x, y)), in that order."""
    cap = sc["n_obs"]
    assert len(pts) <= cap
    si = sc["scene_in"]
    off = s * cap
    si["obs_off"][s], si["obs_n"][s] = off, len(pts)
    o = sc["obs_pool"][off: off + len(pts)]
    if len(pts):
        a = np.array(pts, dtype=np.float64)
        o["x"], o["y"] = a[:, 0], a[:, 1]
    o["type"], o["radius"] = 0, 0.5


def _straight_xy(n, x0, y0, heading_deg=0.0, h=0.5):
    a = np.radians(heading_deg)
    k = np.arange(n, dtype=np.float64)
    return np.stack([x0 + h * np.cos(a) * k, y0 + h * np.sin(a) * k], axis=1)


def _far(rng, k, xy):
    """k obstacles at least 30 m beside the polyline's bounding box (nowhere near a corridor)."""
    y = np.where(rng.random(k) < 0.5, xy[:, 1].min() - rng.uniform(30, 50, k), xy[:, 1].max() + rng.uniform(30, 50, k))
    return list(zip(rng.uniform(xy[:, 0].min(), xy[:, 0].max(), k), y))


def _run(dm, oracle, cfg, sc, label, n_ticks=N_TICKS):
    """n_ticks of the batch on the device and in the oracle; every tick's PlanOut (around[6], ob_*, ob, sweep_*, dec, result,
    ...) and SceneState must agree: integers and obstacle records exactly, floats within parity_util's tolerances."""
    n = len(sc["scene_in"])
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=max(n * sc["n_obs"], 1))
    st_g, st_o = sc["state"].copy(), sc["state"].copy()
    plans = []
    for t in range(n_ticks):
        plan_g, _ = pl.plan_tick_batch(sc, st_g, want_grid=False)
        plan_o, _, _ = oracle.plan_tick_batch(cfg, sc, st_o, want_grid=False)
        bad = compare(plan_g, plan_o, "plan") + compare(st_g, st_o, "state")
        assert not bad, f"{label} tick {t}\n" + "\n".join(bad[:10])
        ai, ao = plan_g["around"]["Ob_Attr"], plan_o["around"]["Ob_Attr"]
        assert ai.tobytes() == ao.tobytes() or not compare(ai, ao), f"{label} tick {t}: obstacle records"
        plans.append(plan_o)
    pl.close()
    return plans, st_o


def _cfg(dm):
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    return cfg


@pytest.mark.gpu
def test_lane_shapes(dm, oracle):
    cfg = _cfg(dm)
    rng = np.random.default_rng(1710)
    n_lane = dm.GEN_LANE_PTS
    more = int(cfg["ID_MORE"][0])
    sc = dm.gen_scenes(cfg, 4100, 16, 12, junction_every=0)
    sc["mot_pool"][:] = 0
    s = 0
    # straight lanes at several headings, every lane-change attribute, one obstacle in the corridor among far ones
    for hd, chg in ((0.0, 0), (90.0, 1), (37.0, 2), (200.0, 3), (-90.0, 0), (135.0, 0)):
        xy = _straight_xy(n_lane, 300.0, 400.0, hd)
        _set_lane(dm, sc, s, xy, 50, lanechg=chg)
        _set_obs(sc, s, _far(rng, 7, xy) + [tuple(xy[50 + 60] + [0.1, 0.2])] + _far(rng, 4, xy))
        s += 1
    # a 90 degree bend 20 m ahead of the ego and ONE obstacle 30 m back on the extension of the segment after the bend: the
    # reference rule accepts it (nearest vertex = the bend, lateral distance 0), so no cull may drop it
    bend_scene = s
    leg = _straight_xy(91, 300.0, 400.0, 0.0)
    xy = np.concatenate([leg, leg[-1] + np.stack([np.zeros(n_lane - 91), 0.5 * np.arange(1, n_lane - 90)], axis=1)])
    _set_lane(dm, sc, s, xy, 50)
    _set_obs(sc, s, [(xy[90, 0], xy[90, 1] - 30.0)])
    s += 1
    # the same bend with far and near obstacles
    _set_lane(dm, sc, s, xy, 50, lanechg=1)
    _set_obs(sc, s, _far(rng, 5, xy) + [(xy[90, 0] + 0.3, xy[90, 1] - 45.0), tuple(xy[140] + [0.2, 0.0])] + _far(rng, 5, xy))
    s += 1
    # two identical consecutive points ahead of the ego (a zero-length segment)
    xy = _straight_xy(n_lane, 300.0, 400.0, 20.0)
    xy[80] = xy[79]
    _set_lane(dm, sc, s, xy, 50)
    _set_obs(sc, s, _far(rng, 6, xy) + [tuple(xy[100] + [0.0, 0.3])])
    s += 1
    # ego at the lane's end: a 2-point front path, then 1 and 0 points
    for cut in (2, 1, 0):
        xy = _straight_xy(n_lane, 300.0, 400.0, 0.0)
        k = 50 + more + cut
        _set_lane(dm, sc, s, xy[:k], 50)
        _set_obs(sc, s, _far(rng, 3, xy) + [tuple(xy[k - 1] + [0.2, 0.1]), tuple(xy[k - 1] + [1.0, 0.0]), tuple(xy[30] + [0.0, 0.2])])
        s += 1
    # a wavy lane whose chunk boxes are not thin, obstacles just inside and far outside the corridor
    x = 300.0 + 0.5 * np.arange(n_lane)
    xy = np.stack([x, 400.0 + 3.0 * np.sin(x / 9.0)], axis=1)
    for chg in (0, 3):
        _set_lane(dm, sc, s, xy, 50, lanechg=chg)
        _set_obs(sc, s, _far(rng, 4, xy) + [tuple(xy[k] + [0.0, d]) for k, d in ((70, 0.85), (95, -0.95), (130, 0.5), (30, 0.1), (60, 4.0))])
        s += 1
    while s < 16:
        _set_obs(sc, s, [])
        s += 1
    plans, _ = _run(dm, oracle, cfg, sc, "lane shapes")
    f = plans[0]["around"][bend_scene][0]
    assert f["Obs_flag"] == 1 and f["Ob_Attr"]["y"] == 400.0 - 30.0          # today's answer: accepted, 30 m off the path
    assert plans[0]["around"]["Obs_flag"][:6, 0].all()


@pytest.mark.gpu
def test_junction_scenes(dm, oracle):
    """pos 1 / 2: the whole block on the front refpath (team<4>), gentle arcs of up to 400 points."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(1711)
    sc = dm.gen_scenes(cfg, 4200, 16, 70, junction_every=2)
    sc["mot_pool"][:] = 0
    si = sc["scene_in"]
    assert set(si["loc"]["pos"].tolist()) == {0, 1, 2}
    for s in range(16):
        ref = sc["ref_pool"][si["ref_off"][s]: si["ref_off"][s] + si["ref_n"][s]]
        xy = np.stack([ref["x"], ref["y"]], axis=1)
        far = _far(rng, 69, xy)
        hit = (float(ref["x"][60 + s]), float(ref["y"][60 + s]) + 0.2)
        at = (0, 68, 63, 64)[s % 4]
        if s >= 12:
            _set_obs(sc, s, far)                                    # nothing on the junction path
        else:
            _set_obs(sc, s, far[:at] + [hit] + far[at:68] + ([hit] if s % 3 == 0 else far[68:69]))
    plans, _ = _run(dm, oracle, cfg, sc, "junction")
    junc = si["loc"]["pos"] != 0
    assert plans[0]["around"]["Obs_flag"][junc, 0].sum() >= 4


@pytest.mark.gpu
def test_obstacle_lists(dm, oracle):
    """No obstacle near a corridor, every obstacle near it, NaN obstacles first and last, ties on the arc length."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(1712)
    n_lane = dm.GEN_LANE_PTS
    sc = dm.gen_scenes(cfg, 4300, 12, 96, junction_every=0)
    sc["mot_pool"][:] = 0
    x = 300.0 + 0.5 * np.arange(n_lane)
    xy = np.stack([x, 400.0 + 1.5 * np.sin(x / 11.0)], axis=1)
    near = lambda k, lat=2.5: [tuple(xy[int(i)] + [0.0, float(d)]) for i, d in zip(rng.integers(15, 175, k), rng.uniform(-lat, lat, k))]
    nan = (float("nan"), 400.0)
    tie = lambda i: [tuple(xy[i] + [0.0, 0.3]), tuple(xy[i] + [0.0, -0.3]), tuple(xy[i] + [0.01, 0.1])]   # one nearest vertex: one lng
    lists = [
        _far(rng, 96, xy),                                           # nothing near the corridors
        _far(rng, 1, xy),
        near(96),                                                    # every obstacle near the lane (two chunks of 64)
        near(64, 0.5),
        [nan] + _far(rng, 40, xy) + near(5),                         # NaN first: accepted with dis_lng = s[0]
        _far(rng, 40, xy) + near(5) + [nan],                         # NaN last
        [nan] + _far(rng, 94, xy) + [(400.0, float("nan"))],
        _far(rng, 70, xy) + tie(90) + _far(rng, 10, xy),             # ties: the lowest index wins
        _far(rng, 62, xy) + tie(120) + near(3, 0.2),                 # ... across the 64-obstacle boundary
        tie(60)[::-1] + _far(rng, 20, xy) + tie(60),
        near(30) + tie(160) + near(30),
        [],
    ]
    for s, pts in enumerate(lists):
        _set_lane(dm, sc, s, xy, 50, lanechg=(0, 1, 2, 3)[s % 4])
        _set_obs(sc, s, pts)
    plans, _ = _run(dm, oracle, cfg, sc, "obstacle lists")
    a = plans[0]["around"]
    assert not a["Obs_flag"][0].any() and not a["Obs_flag"][1].any()
    assert a["Obs_flag"][4, 0] == 1 and a["Ob_Pose"]["dis_lng"][4, 0] == 0.0 and np.isnan(a["Ob_Attr"]["x"][4, 0])
    assert a["Obs_flag"][7, 0] == 1 and a["Ob_Attr"]["y"][7, 0] == xy[90, 1] + 0.3      # first of the tied three


@pytest.mark.gpu
def test_obstacle_counts(dm, oracle):
    """m = 0, 1, 63, 64, 65, 128, 256, 257 with the only in-corridor obstacle first, last and at 63 | 64."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(1713)
    n_lane = dm.GEN_LANE_PTS
    cases = [(m, at) for m in (0, 1, 63, 64, 65, 128, 256, 257) for at in sorted({0, m - 1, 63, 64}) if 0 <= at < m] + [(0, None)]
    assert 8 <= len(cases) <= 32
    sc = dm.gen_scenes(cfg, 4400, len(cases), 257, junction_every=0)
    sc["mot_pool"][:] = 0
    for s, (m, at) in enumerate(cases):
        xy = _straight_xy(n_lane, 300.0, 400.0, 11.0 * s)
        _set_lane(dm, sc, s, xy, 50, lanechg=(0, 0, 1, 2)[s % 4])
        pts = _far(rng, m, xy)
        if at is not None:
            pts[at] = tuple(xy[50 + 20 + s] + [0.05, 0.05])
        _set_obs(sc, s, pts)
    plans, _ = _run(dm, oracle, cfg, sc, "obstacle counts")
    flag = plans[0]["around"]["Obs_flag"][:, 0]
    assert flag.tolist() == [int(at is not None) for _, at in cases]


@pytest.mark.gpu
def test_sweep_runs(dm, oracle):
    """LaneChg == 0 and a front obstacle nearer than 15 m: on the third tick the lateral sweep searches its candidates."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(1714)
    n_lane = dm.GEN_LANE_PTS
    sc = dm.gen_scenes(cfg, 4500, 8, 20, junction_every=0)
    sc["mot_pool"][:] = 0
    for s in range(8):
        xy = _straight_xy(n_lane, 300.0, 400.0, 45.0 * s)
        _set_lane(dm, sc, s, xy, 50, lanechg=0, width=(3.75, 7.0)[s % 2])
        ahead = xy[50 + 16 + s]                                       # 8 to 12 m ahead of the ego
        side = np.array([-(xy[1] - xy[0])[1], (xy[1] - xy[0])[0]]) / 0.5
        pts = _far(rng, 9, xy) + [tuple(ahead + 0.2 * side)] + _far(rng, 6, xy)
        pts += [tuple(xy[50 + 40] + 1.2 * side), tuple(xy[50 + 30] - 0.7 * side), tuple(xy[50 + 25] + 2.0 * side), tuple(xy[50 + 70])]
        _set_obs(sc, s, pts)
    plans, st = _run(dm, oracle, cfg, sc, "sweep")
    assert (plans[-1]["around"]["Ob_Pose"]["dis_lng"][:, 0] < 15).all() and (st["obsavoid_time"] >= 2).all()
    assert (plans[-1]["sweep_index"] >= 0).any() or (plans[-1]["sweep_side"] != 0).any()


def _share_cases():
    return [(n, v) for n in range(2, 10) for v in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 1])
def test_share_boundaries(dm, oracle, half):
    """Paths of n = 2 .. 9 points with the only near obstacle beside vertex v, for every v: the nearest vertex falls on each
    side of every share boundary (two waves: n/4; four waves: n/3, 2n/3; empty leader shares for n < 4).  Front corridor of
    a road scene (two waves per corridor) and the front path of a pre-junction scene (four waves)."""
    cfg = _cfg(dm)
    rng = np.random.default_rng(1720 + half)
    n_lane = dm.GEN_LANE_PTS
    more = int(cfg["ID_MORE"][0])
    cases = _share_cases()[half::2]
    sc = dm.gen_scenes(cfg, 4600, 2 * len(cases), 4, junction_every=0)
    sc["mot_pool"][:] = 0
    si = sc["scene_in"]
    for k, (n, v) in enumerate(cases):
        xy = _straight_xy(n_lane, 300.0, 400.0, 17.0 * k)
        fwd = (xy[1] - xy[0]) / 0.5
        side = np.array([-fwd[1], fwd[0]])
        inward = 0.1 * fwd * (1 if v == 0 else -1 if v == n - 1 else 0)          # clear of the two end tests, still nearest to v
        # road scene: the lane ends n points after the first front point
        s = 2 * k
        first = 50 + more
        _set_lane(dm, sc, s, xy[:first + n], 50, lanechg=0)
        _set_obs(sc, s, _far(rng, 2, xy) + [tuple(xy[first + v] + 0.1 * side + inward)] + _far(rng, 1, xy))
        # pre-junction scene: the front path is the n lane points from the ego on, no junction polyline behind them
        s = 2 * k + 1
        _set_lane(dm, sc, s, xy[:50 + n], 50, lanechg=0)
        si["loc"]["pos"][s], si["ref_n"][s] = 1, 0
        _set_obs(sc, s, _far(rng, 1, xy) + [tuple(xy[50 + v] - 0.1 * side + inward)] + _far(rng, 2, xy))
    plans, _ = _run(dm, oracle, cfg, sc, f"share boundaries {half}", n_ticks=1)
    a = plans[0]["around"]
    assert a["Obs_flag"][:, 0].tolist() == [1] * (2 * len(cases))
    assert a["Ob_Pathid"][:, 0].tolist() == [v for _, v in cases for _ in (0, 1)]
