"""G3 - the scoring of the lattice candidates and of the grid path - at high precision, written from the specification
(BezierPlanning, MeanPoints; GetRoadAngle of Planning.cpp:719-750), not from the kernel or the oracle.

Arithmetic: mpmath at DPS digits on the EXACT values of the float64 inputs (PI and EPSILON are the config's numbers, as
the specification says); without mpmath, float64 with math.fsum for the sums - `ARITHMETIC` says which one is in use.  At
40 digits the order of a sum does not matter, so the 64-leaf tree of §5 is not restated here: against float64 results it
shows as a relative difference of ~1e-15.

The specification, as this file reads it:
  * have_path = the search FOUND a path; a = min(path_len - 1, lookahead_cells, 199); the terminal point T is the centre of
    path cell a, the terminal heading GetRoadAngle(centre of cell max(a - 4, 0), T), the ego's heading when a = 0;
    without a path T = goal, heading GetRoadAngle(ego, goal), and there is no path candidate.
  * candidate k < n_lattice: BezierPlanning(ego pose -> (T + off * (sin th, -cos th), th)), off = (k - (n_lattice - 1) // 2)
    * lattice_step (whole-number division: with 16 candidates number 7 is the straight one; off > 0 is to the RIGHT of the heading);
    candidate n_lattice: MeanPoints(centres of path cells 0 .. a) with off = 0.  200 points each.
  * per point: clearance = min over the obstacles within r + Vehicle_Width / 2 + d_safe of the point (farther ones cannot
    produce a penalty and are left out) of (distance - r), minus Vehicle_Width / 2; pen = 1000 if clearance <= 0,
    ((d_safe - c) / d_safe)^2 below d_safe, else 0.  Interior points: kappa = 1 / R, R the circumradius expression of
    Planning.cpp:1004-1017 on (p[i-1], p[i], p[i+1]); R = 1000 when two neighbours coincide (0/0), when sinA is not a number,
    and when sinA < 0.001.
  * col = sum pen, curv = sum kappa^2, prog = (200 - first point with clearance <= 0) / 200 (0 without one),
    cost = w_col col + w_curv curv + w_prog prog + w_off |off|; the smallest cost wins, ties to the lowest index; no
    candidate at all: winner 0, 200 zero points.

  * obstacles whose values are not finite or out of range ("Values outside the grid's range"): the plain loop as it
    stands - clearance starts at +inf, an obstacle with d2 > cutoff^2 is skipped, v = d - r replaces the clearance when v < clearance,
    and a comparison with a NaN is false.  So a NaN x, y or radius contributes nothing, an infinite distance is skipped by every
    finite cutoff, radius = +inf gives every point at a finite distance the clearance -inf, radius = -inf gives +inf, and a negative
    cutoff - squared - admits the obstacle within |cutoff| with v = d + |r|.  `collision` evaluates exactly this; nothing is
    decided beforehand (a point whose clearance stays +inf has no penalty).

The specification has two discontinuities - clearance <= 0 and sinA < 0.001 - so every result carries how close the case
comes to them: `min_abs_clearance` (metres, over all points with a finite clearance) and `min_fence` (|sinA - 0.001| / 0.001
over the interior points that have a sinA).  A committed case keeps away from both (tests/test_score_edges.py)."""
import math

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpf
    DPS = 40
    mp.dps = DPS
    ARITHMETIC = f"mpmath {mpmath.__version__} at {DPS} digits"
    _sqrt, _atan, _cos, _sin = mp.sqrt, mp.atan, mp.cos, mp.sin
    _sum = lambda v: mp.fsum(v)
    _num = lambda v: mpf(float(v))
except ImportError:                      # float64: the same text, sums by math.fsum
    mpmath = None
    ARITHMETIC = "float64 with math.fsum (mpmath is not importable)"
    _sqrt, _atan, _cos, _sin = math.sqrt, math.atan, math.cos, math.sin
    _sum = lambda v: math.fsum(v)
    _num = float

N = 200
PREFILTER_MARGIN = 0.01      # metres beyond an obstacle's cutoff: the float64 pre-selection of the obstacles evaluated at high precision


def road_angle(cfg, ax, ay, bx, by):
    """GetRoadAngle: degrees, counter-clockwise from east, [0, 360)."""
    pi, eps = _num(cfg["PI"][0]), _num(cfg["EPSILON"][0])
    dx, dy = bx - ax, by - ay
    if abs(dx) < eps and abs(dy) < eps:
        ang = _num(0)
    elif abs(dx) < eps:
        ang = pi / 2 if by > ay else 3 * pi / 2
    else:
        ang = _atan(dy / dx)
        if bx < ax:
            ang = ang + pi
        elif bx > ax and by < ay:
            ang = ang + 2 * pi
    return ang * 180 / pi


_basis = {}


def _bernstein(i):
    if i not in _basis:
        t = _num(i) / (N - 1)
        u = 1 - t
        _basis[i] = (u * u * u, 3 * u * u * t, 3 * u * t * t, t * t * t)
    return _basis[i]


def bezier(cfg, sx, sy, sdir, ex, ey, edir):
    """BezierPlanning: 200 points of the cubic with arms |P3 - P0| / 3 along the two headings."""
    pi = _num(cfg["PI"][0])
    th0, th1 = sdir * pi / 180, edir * pi / 180
    d = _sqrt((ex - sx) ** 2 + (ey - sy) ** 2) / 3
    x1, y1 = sx + d * _cos(th0), sy + d * _sin(th0)
    x2, y2 = ex - d * _cos(th1), ey - d * _sin(th1)
    pts = []
    for i in range(N):
        b0, b1, b2, b3 = _bernstein(i)
        pts.append((b0 * sx + b1 * x1 + b2 * x2 + b3 * ex, b0 * sy + b1 * y1 + b2 * y2 + b3 * ey))
    return pts


def mean_points(cfg, pin):
    """MeanPoints: 200 points at uniform arc length along the polyline `pin`, linear interpolation."""
    eps = _num(cfg["EPSILON"][0])
    if not pin:
        return [(_num(0), _num(0))] * N
    cum = [_num(0)]
    for i in range(1, len(pin)):
        cum.append(cum[-1] + _sqrt((pin[i][0] - pin[i - 1][0]) ** 2 + (pin[i][1] - pin[i - 1][1]) ** 2))
    L = cum[-1]
    if len(pin) == 1 or L < eps:
        return [pin[0]] * N
    out, j = [], 0
    for k in range(N):
        s = L * k / (N - 1)
        while j < len(pin) - 2 and cum[j + 1] < s:       # the first segment whose end is not before s
            j += 1
        seg = cum[j + 1] - cum[j]
        r = (s - cum[j]) / seg if seg > eps else _num(0)
        out.append((pin[j][0] + r * (pin[j + 1][0] - pin[j][0]), pin[j][1] + r * (pin[j + 1][1] - pin[j][1])))
    return out


def curvature(pts):
    """curv = sum of kappa^2 over the interior points, and the smallest distance from the fence sinA = 0.001."""
    k2s, min_fence = [], math.inf
    seg = [_sqrt((pts[i][0] - pts[i + 1][0]) ** 2 + (pts[i][1] - pts[i + 1][1]) ** 2) for i in range(N - 1)]
    fence = _num(1) / 1000
    for i in range(1, N - 1):
        dis1, dis2 = seg[i - 1], seg[i]
        dis3 = _sqrt((pts[i - 1][0] - pts[i + 1][0]) ** 2 + (pts[i - 1][1] - pts[i + 1][1]) ** 2)
        den = 2 * dis1 * dis2
        R = _num(1000)
        if den > 0:
            cos_a = (dis1 * dis1 + dis2 * dis2 - dis3 * dis3) / den
            rad = 1 - cos_a * cos_a
            sin_a = _sqrt(rad) if rad >= 0 else _num(0)       # exactly straight: the rounding of cos_a may leave -1e-40
            min_fence = min(min_fence, float(abs(sin_a - fence) * 1000))
            if sin_a >= fence:
                R = dis3 / 2 / sin_a
        kappa = 1 / R
        k2s.append(kappa * kappa)
    return _sum(k2s), min_fence


def collision(cfg, pts, P, obs):
    """col, prog, the first colliding point and the smallest |clearance| of one candidate.  `P`: the points in float64, for
    the pre-selection (PREFILTER_MARGIN beyond the cutoff); the decisions themselves are taken at high precision."""
    half_w, d_safe = _num(cfg["Vehicle_Width"][0]) / 2, _num(cfg["d_safe"][0])
    pens, first_hit, min_abs_clear = [], N, math.inf
    if len(obs):
        ox, oy, orad = obs["x"].astype(np.float64), obs["y"].astype(np.float64), obs["radius"].astype(np.float64)
        # The pre-selection only drops what the plain loop certainly skips - a finite or infinite distance beyond |cutoff| + margin
        # (the cutoff is squared in the loop, so its sign does not matter there).  A NaN distance or cutoff, and inf against inf,
        # compare false here and go to the loop below, which is the rule itself: clear starts at +inf, `d2 > thr * thr`
        # skips, `v < clear` replaces - and a comparison with a NaN is false.
        with np.errstate(all="ignore"):
            dist = np.hypot(P[:, 0:1] - ox[None, :], P[:, 1:2] - oy[None, :])
            sel = ~(dist > (np.abs(orad + float(half_w) + float(d_safe)) + PREFILTER_MARGIN)[None, :])
        o_mp = [(_num(ox[j]), _num(oy[j]), _num(orad[j])) for j in range(len(obs))]
        inf = _num(math.inf)
        for i in np.flatnonzero(sel.any(axis=1)):
            x, y = pts[i]
            clear = inf
            for j in np.flatnonzero(sel[i]):
                qx, qy, r = o_mp[j]
                d2 = (x - qx) ** 2 + (y - qy) ** 2
                thr = r + half_w + d_safe
                if d2 > thr * thr:
                    continue
                v = _sqrt(d2) - r
                if v < clear:
                    clear = v
            if clear == inf:
                continue
            clear = clear - half_w
            min_abs_clear = min(min_abs_clear, float(abs(clear)))
            if clear <= 0:
                pens.append(_num(1000))
                first_hit = min(first_hit, int(i))
            elif clear < d_safe:
                pens.append(((d_safe - clear) / d_safe) ** 2)
    prog = _num(0) if first_hit == N else _num(N - first_hit) / N
    return dict(col=_sum(pens) if pens else _num(0), prog=prog, first_hit=first_hit, min_abs_clearance=min_abs_clear)


# The same candidate (the sweeps of n_lattice re-use every offset) among the same near obstacles (the two batches differ in
# their padding alone) is evaluated once per process.
_points_cache, _curv_cache, _col_cache = {}, {}, {}


def _relevant(cfg, P, obs):
    """The obstacles within their cutoff + PREFILTER_MARGIN of any point of the candidate (float64), in list order."""
    if not len(obs):
        return np.ascontiguousarray(obs)
    with np.errstate(all="ignore"):              # (only what the plain loop certainly skips is dropped: see `collision`)
        reach = np.abs(obs["radius"].astype(np.float64) + 0.5 * float(cfg["Vehicle_Width"][0]) + float(cfg["d_safe"][0])) + PREFILTER_MARGIN
        dist = np.hypot(P[:, 0:1] - obs["x"][None, :], P[:, 1:2] - obs["y"][None, :])
        return np.ascontiguousarray(obs[(~(dist > reach[None, :])).any(axis=0)])


def _candidate(cfg, gkey, make, obs):
    if gkey not in _points_cache:
        pts = make()
        _points_cache[gkey] = (pts, np.array([[float(x), float(y)] for x, y in pts]))
        _curv_cache[gkey] = curvature(pts)
    pts, P = _points_cache[gkey]
    rel = _relevant(cfg, P, obs)
    ckey = (gkey, float(cfg["Vehicle_Width"][0]), float(cfg["d_safe"][0]), rel.tobytes())
    if ckey not in _col_cache:
        _col_cache[ckey] = collision(cfg, pts, P, rel)
    r = dict(_col_cache[ckey])
    r["curv"], r["min_fence"] = _curv_cache[gkey]
    return pts, P, r


def score_scene(cfg, si, obs, path, status):
    """cfg: PlannerConfig record array of one; si: one SceneIn record; obs: the scene's effective ObPoint records; path: the grid
    path's cells (start .. goal) and status: the search's status.  Returns n_candidates, best_candidate, the float64 arrays
    cand_col / cand_curv / cand_prog / cand_cost, best_path (200 x 2), margin (runner-up's cost minus the winner's; inf with
    fewer than two candidates), min_abs_clearance and min_fence (the smallest over all candidates)."""
    W, cell = int(cfg["grid_w"][0]), _num(cfg["cell"][0])
    gx, gy = _num(si["grid_origin"]["x"]), _num(si["grid_origin"]["y"])
    ego = tuple(_num(si["loc"]["globalpoint"][f]) for f in ("x", "y", "dir"))
    have_path = int(status) == 0 and path is not None and len(path) >= 1
    nl = min(int(cfg["n_lattice"][0]), 16)
    nc = nl + (1 if have_path else 0)
    centre = lambda c: (gx + (_num(int(c) % W) + _num(0.5)) * cell, gy + (_num(int(c) // W) + _num(0.5)) * cell)
    a = 0
    if have_path:
        a = min(len(path) - 1, int(cfg["lookahead_cells"][0]), N - 1)
        T = centre(path[a])
        a0 = max(a - 4, 0)
        thT = ego[2] if a0 == a else road_angle(cfg, *centre(path[a0]), *T)
    else:
        T = (_num(si["goal"]["x"]), _num(si["goal"]["y"]))
        thT = road_angle(cfg, ego[0], ego[1], T[0], T[1])
    pi = _num(cfg["PI"][0])
    cs, sn = _cos(thT * pi / 180), _sin(thT * pi / 180)
    step = _num(cfg["lattice_step"][0])
    w = [_num(cfg[f][0]) for f in ("w_col", "w_curv", "w_prog", "w_off")]
    pi_f, eps_f = float(cfg["PI"][0]), float(cfg["EPSILON"][0])
    col, curv, prog, cost = (np.zeros(17) for _ in range(4))
    costs, cand_pts = [], []
    min_abs_clear, min_fence = math.inf, math.inf
    for k in range(nc):
        if k < nl:
            off = (k - (nl - 1) // 2) * step
            pts, P, r = _candidate(cfg, ("bezier", pi_f, ego, T, thT, off), lambda: bezier(cfg, ego[0], ego[1], ego[2], T[0] + off * sn, T[1] - off * cs, thT), obs)
        else:
            off = _num(0)
            cells = [int(c) for c in path[:a + 1]]
            pts, P, r = _candidate(cfg, ("path", eps_f, gx, gy, cell, W, tuple(cells)), lambda: mean_points(cfg, [centre(c) for c in cells]), obs)
        c = w[0] * r["col"] + w[1] * r["curv"] + w[2] * r["prog"] + w[3] * abs(off)
        col[k], curv[k], prog[k], cost[k] = float(r["col"]), float(r["curv"]), float(r["prog"]), float(c)
        costs.append(c)
        cand_pts.append(P)
        min_abs_clear, min_fence = min(min_abs_clear, r["min_abs_clearance"]), min(min_fence, r["min_fence"])
    best, best_path, margin = 0, np.zeros((N, 2)), math.inf
    if nc:
        best = min(range(nc), key=lambda k: (costs[k], k))
        best_path = cand_pts[best].copy()
        if nc > 1:
            margin = float(min(costs[k] for k in range(nc) if k != best) - costs[best])
    return dict(n_candidates=nc, best_candidate=best, cand_col=col, cand_curv=curv, cand_prog=prog, cand_cost=cost,
                best_path=best_path, margin=margin, min_abs_clearance=min_abs_clear, min_fence=min_fence)
