"""The rule by which team_search_obstacle (csrc/dev_geom.hpp) names the nearest obstacle WITHOUT the cumulative arc length.

orc_SearchObstacle builds s[0] = 0, s[i] = s[i-1] + |P[i] - P[i-1]| and uses it in two ways only: `lng = s[bi]` is compared
between the accepted obstacles (strict <, so the first j with the smallest lng wins), and the winner's s[bi] is reported.
While every segment length d[i] is finite, s never decreases (d[i] >= 0, and a sum that overflows stays at inf), so

    the winner is the lexicographic minimum of (s[bi], j) over the accepted obstacles.

Let b* be the smallest bi among them, S = s[b*] (the only in-order sum the answer needs: b* additions) and e >= b* the last
index with fl(S + d[k]) == S for every k in (b*, e].  Then s[k] == S exactly for b* <= k <= e and s[k] > S beyond (the
first addition that is not absorbed raises the sum, and it never comes down again), so the obstacles that share the
smallest lng are those with b* <= bi <= e, and the winner is the smallest j among them.  Each test fl(S + d[k]) == S stands
alone: the sequential sum is S at every k of the run, so no test needs the one before it.
An overflow needs nothing of its own: with S = inf every later d[k] is absorbed, the run reaches the last point, and the
first j of the accepted obstacles wins - what a sequential loop over s = inf, inf, ... does.  (No path can get there: a
finite length is sqrt(dx*dx + dy*dy) <= sqrt(DBL_MAX) = 1.34e154, and the longest path has 512 points.  The case exists
for select_by_rule, which takes lengths, and tests/test_search_obstacle_rule.py shows it there.)

A length that is not finite (a NaN or inf coordinate, or coordinates so large that one segment overflows) breaks the
premise: a NaN in s makes every later comparison false, and the FIRST accepted obstacle keeps a NaN lng whatever follows.
The rule does not apply then and the model answers SLOW_PATH; the device runs the full sum and the per-obstacle comparison
for such a call, as it did for every call before.  (The device looks at the lengths only once an obstacle is accepted -
with nothing accepted either path reports "nothing" - while the model answers SLOW_PATH whenever a length is not finite.)

Everything here is sequential IEEE double arithmetic in the order of the reference loop: numpy element-wise products and
sums round once per operation, as the oracle (built without contraction) does.
"""
import numpy as np

SLOW_PATH = "slow path"


def segment_lengths(px, py):
    """d[0] = 0 (unused), d[i] = |P[i] - P[i-1]| as orc_CalcDistance rounds it."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    d = np.zeros(len(px))
    with np.errstate(all="ignore"):
        dx, dy = px[1:] - px[:-1], py[1:] - py[:-1]
        d[1:] = np.sqrt(dx * dx + dy * dy)
    return d


def cumulative(d):
    """The reference's s: additions in index order."""
    s = np.zeros(len(d))
    acc = np.float64(0.0)
    with np.errstate(all="ignore"):
        for i in range(1, len(d)):
            acc = acc + d[i]
            s[i] = acc
    return s


def _sgn(a):
    return 1.0 if a > 0 else -1.0


def lat_dis(eps, cx, cy, ax, ay, bx, by):
    """orc_GetLatDis (Planning.cpp:686-709)."""
    with np.errstate(all="ignore"):
        if np.abs(ax - bx) > eps:
            k = (ay - by) / (ax - bx)
            lat = np.abs((cy - ay) - k * (cx - ax)) / np.sqrt(1 + k * k)
        else:
            lat = np.abs(ax - cx)
        if lat < eps:
            return np.float64(0.0)
        return lat * _sgn((bx - ax) * (cy - ay) - (by - ay) * (cx - ax))


def accepted(eps, px, py, ox, oy, lo, hi):
    """[(j, bi, lat)] of the obstacles the reference loop reaches `lng = s[bi]` with, in j order.  No arc length involved."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    n = len(px)
    out = []
    for j in range(len(ox)):
        x, y = np.float64(ox[j]), np.float64(oy[j])
        with np.errstate(all="ignore"):
            dx, dy = x - px, y - py
            d2 = dx * dx + dy * dy
        d2 = np.where(np.isnan(d2), np.inf, d2)          # `d2 < best` is false for a NaN: it never becomes the minimum
        bi = int(np.argmin(d2))                          # first minimum; all inf: 0, as `inf < inf` is false from best = inf
        idx = n - 2 if bi == n - 1 else bi
        ax, ay, bx, by = px[idx], py[idx], px[idx + 1], py[idx + 1]
        with np.errstate(all="ignore"):
            if bi == 0 and (x - ax) * (bx - ax) + (y - ay) * (by - ay) < 0:
                continue
            if bi == n - 1 and (x - bx) * (bx - ax) + (y - by) * (by - ay) > 0:
                continue
        lat = lat_dis(eps, x, y, ax, ay, bx, by)
        if lat < lo or lat > hi:
            continue
        out.append((j, bi, lat))
    return out


def search_obstacle_rule(eps, no_obstacle_dis, px, py, ox, oy, lo, hi):
    """SLOW_PATH, or dict(flag, dis_lat, dis_lng, path_id, ob_index, additions): the answer by the rule above.
    `additions` counts the in-order additions the rule needed (b*)."""
    n, m = len(px), len(ox)
    none = dict(flag=0, dis_lat=float(no_obstacle_dis), dis_lng=float(no_obstacle_dis), path_id=0, ob_index=-1, additions=0)
    if n < 2:
        return none
    d = segment_lengths(px, py)
    if not np.isfinite(d).all():
        return SLOW_PATH
    acc = accepted(eps, px, py, ox, oy, lo, hi) if m >= 1 else []
    if not acc:
        return none
    j, bi, lat, S, b = select_by_rule(d, acc)
    return dict(flag=1, dis_lat=float(lat), dis_lng=float(S), path_id=bi, ob_index=j, additions=b)


def select_by_rule(d, acc):
    """(j, bi, lat, S, b*) of the winner among acc = [(j, bi, lat)] (not empty), given the FINITE segment lengths d[1 .. n)."""
    n = len(d)
    b = min(bi for _, bi, _ in acc)
    S = np.float64(0.0)
    with np.errstate(all="ignore"):
        for k in range(1, b + 1):                        # the one in-order sum
            S = S + d[k]
        e = b
        while e + 1 < n and S + d[e + 1] == S:           # each test on its own: S is the sum at every index of the run
            e += 1
    j, bi, lat = min(t for t in acc if t[1] <= e)        # smallest j with b* <= bi <= e
    return j, bi, lat, S, b
