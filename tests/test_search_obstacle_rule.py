"""tests/search_obstacle_rule.py (the rule team_search_obstacle answers by: one in-order sum up to the nearest accepted
vertex, plus the run of absorbed additions behind it) against oracle.SearchObstacle: every field, floats by bit pattern.

Each family counts the cases that really have its property - from the reference's s, rebuilt here by the same in-order
additions and checked against the oracle's dis_lng wherever it reports one - and fails if a family has none.  CPU only: no
device code runs here."""
import struct

import numpy as np

from search_obstacle_rule import SLOW_PATH, accepted, cumulative, search_obstacle_rule, segment_lengths, select_by_rule


def _bits(v):
    return struct.pack("<d", float(v))


def _limits(cfg):
    hv, hw = 0.5 * float(cfg["Vehicle_Width"][0]), 0.5 * 3.75
    plan = float(np.float32(1.1))
    return [(-hv, hv), (-hv, hv), (-hv, hw), (-hv, hw), (-hw, hv), (-hw, hv), (-plan, plan)]     # AroundObstacle's six, Planning's


def _check(dm, oracle, cfg, xy, obs, lo, hi):
    """Model == oracle on one query.  Returns None for a slow-path answer, else dict(res, acc, s, d)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    obs = np.asarray(obs, np.float64).reshape(-1, 2)
    p = np.zeros(len(xy), dm.GlobalPoint2D); p["x"], p["y"] = xy[:, 0], xy[:, 1]
    o = np.zeros(len(obs), dm.ObPoint); o["x"], o["y"] = obs[:, 0], obs[:, 1]
    o["type"], o["radius"] = np.arange(len(obs)), 0.5                  # the index travels in the record
    eps, nod = float(cfg["EPSILON"][0]), float(cfg["NO_OBSTACLE_DIS"][0])
    res = search_obstacle_rule(eps, nod, p["x"], p["y"], o["x"], o["y"], lo, hi)
    finite = bool(np.isfinite(xy).all())
    d = segment_lengths(p["x"], p["y"])
    if not finite:
        assert res == SLOW_PATH, "a NaN / inf path coordinate must send the call to the slow path"
        return None
    if np.isfinite(d).all():
        assert res != SLOW_PATH, "finite lengths never need the slow path"
    if res == SLOW_PATH:
        return None
    ref = oracle.SearchObstacle(cfg, p, o, lo, hi)
    ctx = (len(xy), len(obs), lo, hi, res, ref)
    assert res["flag"] == ref["flag"] and res["path_id"] == ref["path_id"], ctx
    assert _bits(res["dis_lat"]) == _bits(ref["dis_lat"]) and _bits(res["dis_lng"]) == _bits(ref["dis_lng"]), ctx
    want = o[res["ob_index"]] if res["flag"] else np.zeros(1, dm.ObPoint)[0]
    assert ref["ob"].tobytes() == want.tobytes(), ctx
    s = cumulative(d)
    if ref["flag"]:
        assert _bits(s[ref["path_id"]]) == _bits(ref["dis_lng"]), ctx      # the s rebuilt here is the oracle's
        assert res["additions"] == min(bi for _, bi, _ in accepted(eps, p["x"], p["y"], o["x"], o["y"], lo, hi))
    return dict(res=res, s=s, d=d, acc=accepted(eps, p["x"], p["y"], o["x"], o["y"], lo, hi), n=len(xy))


def _lane(n, rng, h=0.5):
    """A gently wavy lane of n points, about h apart."""
    x = 300.0 + np.cumsum(rng.uniform(0.8 * h, 1.2 * h, n))
    return np.stack([x, 400.0 + 2.0 * np.sin(x / 9.0) + rng.uniform(-40, 40)], axis=1)


def _beside(xy, k, lat=0.2, along=0.0):
    """A point `lat` to the left of vertex k (and `along` forward)."""
    a, b = (xy[k], xy[k + 1]) if k + 1 < len(xy) else (xy[k - 1], xy[k])
    t = (b - a) / np.hypot(*(b - a))
    return xy[k] + along * t + lat * np.array([-t[1], t[0]])


def _far(rng, k):
    return np.stack([rng.uniform(250, 450, k), rng.uniform(600, 700, k)], axis=1)


def _cat(*parts):
    """Obstacle lists (arrays of points, lists of points, possibly empty) in order, as one (m, 2) array."""
    return np.concatenate([np.asarray(q, np.float64).reshape(-1, 2) for q in parts])


def test_random_paths(dm, oracle):
    cfg = dm.default_config(128)
    rng = np.random.default_rng(2101)
    lims = _limits(cfg)
    found = ties = 0
    for k in range(280):
        n = (2, 3, 240, 64, 65)[k] if k < 5 else int(rng.integers(2, 241))
        m = (0, 1, 130, 64, 65)[k % 5] if k < 10 else int(rng.integers(0, 131))
        xy = _lane(n, rng)
        near = rng.random(m) < 0.3                                     # the others are spread over the map
        obs = np.stack([rng.uniform(xy[:, 0].min() - 5, xy[:, 0].max() + 5, m), rng.uniform(xy[:, 1].min() - 8, xy[:, 1].max() + 8, m)], axis=1)
        for j in np.nonzero(near)[0]:
            obs[j] = _beside(xy, int(rng.integers(0, n)), float(rng.uniform(-2.5, 2.5)), float(rng.uniform(-0.2, 0.2)))
        lo, hi = lims[k % len(lims)]
        r = _check(dm, oracle, cfg, xy, obs, lo, hi)
        found += r["res"]["flag"]
        ties += r["res"]["flag"] and sum(bi == r["res"]["path_id"] for _, bi, _ in r["acc"]) > 1
    assert found >= 100 and ties >= 5, (found, ties)


def test_nothing_accepted(dm, oracle):
    cfg = dm.default_config(128)
    rng = np.random.default_rng(2102)
    count = 0
    for k, (lo, hi) in enumerate(_limits(cfg) * 3):
        n = (2, 9, 120, 200, 240)[k % 5]
        xy = _lane(n, rng)
        # far away; beside the lane but outside the limits; behind the first point and beyond the last
        obs = _cat(_far(rng, 20), [_beside(xy, n // 2, hi + 0.5), _beside(xy, n // 3, lo - 0.5),
                                  _beside(xy, 0, 0.0, -3.0), _beside(xy, n - 1, 0.0, 3.0)])
        r = _check(dm, oracle, cfg, xy, obs, lo, hi)
        count += r["res"]["flag"] == 0 and not r["acc"] and r["res"]["additions"] == 0
    assert count == 21


def test_winner_vertices(dm, oracle):
    """Vertex 0, n-1 and both sides of the eight-wide blocks of serial_sum (the sum of b* lengths starts at index 1)."""
    cfg = dm.default_config(128)
    rng = np.random.default_rng(2103)
    lo, hi = _limits(cfg)[0]
    hit = {}
    for n in (2, 10, 19, 120, 200):
        for v in (0, n - 1, 7, 8, 9, 15, 16, 17):
            if not 0 <= v < n:
                continue
            xy = _lane(n, rng)
            inward = 0.1 if v == 0 else -0.1 if v == n - 1 else 0.0
            later = [_beside(xy, w, -0.3) for w in range(v + 1, min(v + 40, n - 1), 7)]      # accepted too, farther along
            obs = _cat(_far(rng, 5), later, [_beside(xy, v, 0.2, inward)], _far(rng, 3))
            r = _check(dm, oracle, cfg, xy, obs, lo, hi)
            if r["res"]["flag"] and r["res"]["path_id"] == v and r["res"]["ob_index"] == 5 + len(later):
                key = "last" if v == n - 1 else v
                hit[key] = hit.get(key, 0) + 1
                if v == 0:
                    assert r["res"]["dis_lng"] == 0.0 and r["res"]["additions"] == 0
    assert set(hit) == {0, "last", 7, 8, 9, 15, 16, 17}, hit


def test_same_vertex_ties(dm, oracle):
    """Two accepted obstacles whose nearest vertex is the same: the smaller j wins, whichever of the two it is."""
    cfg = dm.default_config(128)
    rng = np.random.default_rng(2104)
    lo, hi = _limits(cfg)[0]
    seen = {"first": 0, "second": 0}
    for n in (2, 40, 120, 240):
        for v in sorted({0, n // 2, n - 1}):
            xy = _lane(n, rng)
            inward = 0.1 if v == 0 else -0.1 if v == n - 1 else 0.0
            a, b = _beside(xy, v, 0.3, inward), _beside(xy, v, -0.25, inward)
            for order in ("first", "second"):
                pair = [a, b] if order == "first" else [b, a]
                obs = _cat(_far(rng, 4), pair[:1], _far(rng, 70), pair[1:], _far(rng, 2))      # across the 64 stride
                r = _check(dm, oracle, cfg, xy, obs, lo, hi)
                on_v = [j for j, bi, _ in r["acc"] if bi == v]
                if len(on_v) == 2 and r["res"]["ob_index"] == 4 and r["res"]["path_id"] == v:
                    seen[order] += 1
    assert seen["first"] >= 6 and seen["second"] >= 6, seen


def test_zero_length_runs(dm, oracle):
    """Repeated points before, at and after the winner's vertex."""
    cfg = dm.default_config(128)
    rng = np.random.default_rng(2105)
    lo, hi = _limits(cfg)[6]
    seen = {"before": 0, "at": 0, "after": 0}
    for n in (30, 120, 200):
        for where in ("before", "at", "after"):
            for run in (1, 2, 5):
                xy = _lane(n, rng)
                v = n // 2
                k0 = {"before": v - 10, "at": v, "after": v + 6}[where]
                xy[k0 + 1: k0 + 1 + run] = xy[k0]                         # points k0 .. k0+run coincide
                w = v if where != "at" else k0                            # (the first of equal points is the nearest vertex)
                nxt = k0 + run + 1 if where == "at" else v + 1
                obs = _cat(_far(rng, 3), [_beside(xy, min(nxt + 3, n - 2), 0.1)], [xy[w] + 0.02 * (xy[nxt] - xy[w]) + [0.0, 0.15]], _far(rng, 3))
                r = _check(dm, oracle, cfg, xy, obs, lo, hi)
                b, d = r["res"]["path_id"], r["d"]
                assert r["res"]["flag"] == 1
                zero = np.nonzero(d[1:] == 0)[0] + 1
                seen["before"] += bool((zero < b).any())
                seen["at"] += bool(((zero == b) | (zero == b + 1)).any())
                seen["after"] += bool((zero > b + 1).any())
    assert min(seen.values()) >= 6, seen


def _absorbed_lane(n, x0, step, at):
    """A lane along +y, `step` between points, except that point at+1 lies one ulp of x0 beside point `at` at the same y."""
    y = 100.0 + step * np.arange(n, dtype=np.float64)
    y[at + 1:] -= step
    x = np.full(n, x0)
    x[at + 1:] = np.nextafter(x0, np.inf)
    return np.stack([x, y], axis=1)


def test_absorbed_ties(dm, oracle):
    """Two accepted obstacles on DIFFERENT vertices with equal arc lengths: the addition between them is absorbed
    (2e-16 m against more than 2048 m).  The smaller j wins, on whichever of the two vertices it sits."""
    cfg = dm.default_config(128)
    rng = np.random.default_rng(2106)
    lo, hi = _limits(cfg)[0]
    seen = {"j on the smaller vertex is larger": 0, "j on the smaller vertex is smaller": 0}
    for n, step, at, x0 in ((240, 10.0, 215, 1.0), (240, 12.0, 200, 1.5), (230, 10.0, 228, 1.0), (120, 40.0, 60, 1.25)):
        xy = _absorbed_lane(n, x0, step, at)
        left, right = np.array([x0 - 0.3, xy[at, 1]]), np.array([x0 + 0.3, xy[at, 1]])     # nearest: point at | point at+1
        for order in seen:
            pair = [right, left] if "larger" in order else [left, right]
            for gap in (0, 70):                                           # both in one 64-stride, and apart
                obs = _cat(_far(rng, 3), pair[:1], _far(rng, gap), pair[1:], [[x0 + 0.1, xy[min(at + 2, n - 1), 1] - 0.2]], _far(rng, 2))
                r = _check(dm, oracle, cfg, xy, obs, lo, hi)
                s, acc = r["s"], {j: bi for j, bi, _ in r["acc"]}
                ja, jb = (3 + gap + 1, 3) if "larger" in order else (3, 3 + gap + 1)       # j of the obstacle on `at`, on at+1
                ok = acc.get(ja) == at and acc.get(jb) == at + 1 and s[at] == s[at + 1] and r["d"][at + 1] > 0 and s[at] > 2048
                if ok:
                    assert r["res"]["ob_index"] == 3 and r["res"]["dis_lng"] == s[at]
                    assert r["res"]["path_id"] == (at + 1 if "larger" in order else at)
                    seen[order] += 1
    assert min(seen.values()) >= 6, seen


def test_sum_overflows_to_inf(dm, oracle):
    """A sum of FINITE lengths that overflows: the tie run from b* then covers every later vertex and the first j wins, as in
    a sequential loop over s = ..., inf, inf.  No path reaches this - a finite length is sqrt(dx*dx + dy*dy), at most
    sqrt(DBL_MAX) = 1.34e154, and 511 of them stay far below DBL_MAX (the first assertion) - so the oracle cannot be asked.
    The rule is checked where it takes lengths: select_by_rule against the reference's selection loop, written out on s."""
    big = np.sqrt(np.finfo(np.float64).max)
    xy = np.array([[-big / 2, 0.0], [big / 2, 0.0]])
    assert np.isfinite(segment_lengths(xy[:, 0], xy[:, 1])[1]) and 511 * big < np.finfo(np.float64).max
    assert np.isinf(segment_lengths(2 * xy[:, 0], xy[:, 1])[1])          # a longer segment is not a finite length any more

    def reference(s, acc):                                                # orc_SearchObstacle's loop over the accepted obstacles
        found, best = False, None
        for j, bi, lat in acc:
            if not found or s[bi] < best[3]:
                found, best = True, (j, bi, lat, s[bi])
        return best

    rng = np.random.default_rng(2107)
    count = 0
    for k in range(60):
        n = int(rng.integers(4, 40))
        d = np.concatenate([[0.0], rng.uniform(0.6, 1.0, n - 1) * 1.0e308])     # s[1] is finite, s[3] and all beyond are inf
        s = cumulative(d)
        assert np.isfinite(d).all() and np.isinf(s[3:]).all()
        lowest = (0, 1, 2, 3)[k % 4]
        bis = rng.integers(lowest, n, int(rng.integers(1, 9)))
        acc = [(int(j), int(bi), 0.1 * j) for j, bi in enumerate(bis)]
        j, bi, lat, S, b = select_by_rule(d, acc)
        want = reference(s, acc)
        assert (j, bi, lat) == want[:3] and _bits(S) == _bits(want[3]), (d, acc, want)
        count += bool(np.isinf(S) and len({bi for _, bi, _ in acc}) > 1)
    assert count >= 6, count


def test_non_finite_points_take_the_slow_path(dm, oracle):
    cfg = dm.default_config(128)
    rng = np.random.default_rng(2108)
    lo, hi = _limits(cfg)[0]
    count = 0
    for n in (2, 30, 120):
        for bad in (np.nan, np.inf, -np.inf):
            for at in sorted({0, n // 2, n - 1}):
                for axis in (0, 1):
                    xy = _lane(n, rng)
                    obs = _cat(_far(rng, 3), [_beside(xy, n // 3, 0.1)], [_beside(xy, min(n - 1, 2 * n // 3), 0.1)])
                    xy[at, axis] = bad
                    assert _check(dm, oracle, cfg, xy, obs, lo, hi) is None
                    assert search_obstacle_rule(1e-6, 9999.0, xy[:, 0], xy[:, 1], [], [], lo, hi) == SLOW_PATH or n < 2
                    count += 1
    # one segment longer than a double holds, from finite coordinates: not a finite length either
    xy = np.array([[-1.5e308, 0.0], [1.5e308, 0.0], [1.5e308, 1.0]])
    assert _check(dm, oracle, cfg, xy, [[1.5e308, 0.9]], lo, hi) is None
    assert count == 48
