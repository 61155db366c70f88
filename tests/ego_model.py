"""The ego model of the closed-loop rollout in plain Python / numpy, written from DESIGN.md §4c (not from the kernel).

`advance` is one pp_advance_async for a batch: SceneIn of tick t, PlanOut of tick t, SceneState after tick t and the flag
words in; SceneIn of tick t + 1 and the new flag words out.  Python floats are IEEE doubles and every expression below is
evaluated left to right as the specification writes it, so the result is meant to equal the device's to the last bits
(`atan` aside).  In map mode the lane views of the result still have to be derived (map_scenes.resolve), as k_resolve_map
does behind the kernel."""
import math

import numpy as np

PATH_END, BAD_PATH, LANE_END, OFF_GRID = 1, 2, 4, 8
N_PATH = 200
LANESUM = 8


def road_angle(cfg, ax, ay, bx, by):
    """GetRoadAngle (Planning.cpp:719-750 as dev_geom.hpp keeps it): degrees CCW from east, atan with the EPSILON branches."""
    PI, EPS = float(cfg["PI"][0]), float(cfg["EPSILON"][0])
    if abs(bx - ax) < EPS and abs(by - ay) < EPS:
        angle = 0.0
    elif abs(bx - ax) < EPS:
        angle = PI / 2 if by > ay else 3 * PI / 2
    else:
        angle = math.atan((by - ay) / (bx - ax))
        if bx < ax:
            angle = angle + PI
        elif bx > ax and by < ay:
            angle = angle + 2 * PI
    return angle * 180 / PI


def next_speed(v, desaccVd, desacc, desspd, dt, max_acc, max_dec):
    """§4c 1.: km/h."""
    if desaccVd != 0:
        vn = v + desacc * dt * 3.6
        if not vn > 0:
            vn = 0.0
        return vn
    g = desspd
    if not math.isfinite(g):
        return v
    if g > v:
        vn = v + max_acc * dt * 3.6
        if vn > g:
            vn = g
    else:
        vn = v - max_dec * dt * 3.6
        if vn < g:
            vn = g
    return vn


def step_length(v, vn, dt):
    """§4c 2.: metres."""
    return 0.5 * (v + vn) / 3.6 * dt


def walk_path(cfg, px, py, k0, s, dir0):
    """§4c 3.: (x, y, dir, flags) - flags is 0, PATH_END or BAD_PATH (then x, y, dir are meaningless)."""
    k0 = min(max(int(k0), 0), N_PATH - 1)
    x, y, d = float(px[k0]), float(py[k0]), dir0
    if not (math.isfinite(s) and math.isfinite(x) and math.isfinite(y)):
        return x, y, d, BAD_PATH
    if not s > 0:
        return x, y, d, 0
    a, last = 0.0, -1
    for i in range(k0, N_PATH - 1):
        x0, y0, x1, y1 = float(px[i]), float(py[i]), float(px[i + 1]), float(py[i + 1])
        dx, dy = x1 - x0, y1 - y0
        q = dx * dx + dy * dy
        L = math.sqrt(q)
        if not math.isfinite(L):
            return x, y, d, BAD_PATH
        if L == 0:
            continue
        last = i
        if a + L >= s:
            t = (s - a) / L
            return x0 + t * dx, y0 + t * dy, road_angle(cfg, x0, y0, x1, y1), 0
        a = a + L
    if last >= 0:
        d = road_angle(cfg, float(px[last]), float(py[last]), float(px[last + 1]), float(py[last + 1]))
    return float(px[N_PATH - 1]), float(py[N_PATH - 1]), d, PATH_END


def nearest_in_window(lx, ly, n, j, window, x, y):
    """§4c 4.: (new id or None, d2 of it, gap to the second smallest d2 in the window or inf).  lx / ly: the view's points."""
    lo, hi = max(int(j), 0), min(int(j) + int(window), int(n))
    if lo >= hi:
        return None, None, math.inf
    ex = lx[lo:hi] - x
    ey = ly[lo:hi] - y
    d2 = ex * ex + ey * ey
    ok = ~np.isnan(d2)
    if not ok.any():
        return None, None, math.inf
    k = int(np.nanargmin(d2))                    # first index of the smallest
    rest = np.delete(d2, k)
    rest = rest[~np.isnan(rest)]
    gap = float(rest.min() - d2[k]) if len(rest) else math.inf
    return lo + k, float(d2[k]), gap


def advance_scene(cfg, model, si, po, st, flag, lane_x, lane_y, map_mode):
    """One scene.  si / po / st: numpy records; returns (new SceneIn record, new flag word, smallest id gap)."""
    out = si.copy()
    if flag != 0:
        return out, int(flag), math.inf
    dt, max_acc, max_dec = float(model["dt"][0]), float(model["max_acc"][0]), float(model["max_dec"][0])
    window = int(model["window"][0])
    R = po["result"]
    v = float(si["loc"]["velocity"])
    vn = next_speed(v, int(R["desaccVd"]), float(R["desacc"]), float(R["desspd"]), dt, max_acc, max_dec)
    s = step_length(v, vn, dt)
    P = po["road_points"]
    k0 = 0 if int(st["afresh_planning"]) != 0 else int(st["path_near_id"])
    x, y, d, f = walk_path(cfg, P["x"], P["y"], k0, s, float(si["loc"]["globalpoint"]["dir"]))
    if f & BAD_PATH:
        return out, BAD_PATH, math.inf
    loc = out["loc"]
    loc["globalpoint"]["x"], loc["globalpoint"]["y"], loc["globalpoint"]["dir"], loc["velocity"] = x, y, d, vn
    n, V = int(si["loc"]["lane_num"]), si["lanes"]
    views = {}
    if 1 <= n <= LANESUM and int(V["cur_n"]) > 0:
        views["cur"] = (n - 1, int(V["cur_off"]), int(V["cur_n"]))
    if 2 <= n <= LANESUM + 1 and int(V["left_n"]) > 0:
        views["left"] = (n - 2, int(V["left_off"]), int(V["left_n"]))
    if 0 <= n < min(int(V["lane_sum"]), LANESUM) and int(V["right_n"]) > 0:
        views["right"] = (n, int(V["right_off"]), int(V["right_n"]))
    found, gap = {}, math.inf
    ids = si["loc"]["id"].copy()
    for name, (slot, off, m) in views.items():
        i, d2, g = nearest_in_window(lane_x[off:off + m], lane_y[off:off + m], m, int(si["loc"]["id"][slot]), window, x, y)
        gap = min(gap, g)
        if i is not None:
            found[name] = d2
            ids[slot] = i
    loc["id"] = ids
    if "cur" in views and int(ids[views["cur"][0]]) + window >= views["cur"][2]:
        f |= LANE_END
    if map_mode and "cur" in found:
        rc, w = math.sqrt(found["cur"]), 0.25 * float(V["lane_width"])
        if "left" in found and rc - math.sqrt(found["left"]) > w:
            loc["lane_num"] = n - 1
        elif "right" in found and rc - math.sqrt(found["right"]) > w:
            loc["lane_num"] = n + 1
    if int(cfg["grid_stage"][0]):
        cell = float(cfg["cell"][0])
        fx = math.floor((x - float(si["grid_origin"]["x"])) / cell)
        fy = math.floor((y - float(si["grid_origin"]["y"])) / cell)
        if not (0 <= fx < int(cfg["grid_w"][0]) and 0 <= fy < int(cfg["grid_h"][0])):
            f |= OFF_GRID
    return out, f, gap


def advance(cfg, model, scene_in, plan, state, flags, lane_pool, map_mode=False):
    """The batch.  Returns (SceneIn of the next tick, flag words, per-scene gap between the two smallest squared distances of
    any id search - a scene with a gap below the comparison's resolution may be left out of an id comparison)."""
    out = scene_in.copy()
    new_flags = np.array(flags, np.int32).copy()
    gaps = np.full(len(scene_in), math.inf)
    lane_x, lane_y = np.ascontiguousarray(lane_pool["x"]), np.ascontiguousarray(lane_pool["y"])
    for k in range(len(scene_in)):
        rec, new_flags[k], gaps[k] = advance_scene(cfg, model, scene_in[k], plan[k], state[k], int(flags[k]), lane_x, lane_y, map_mode)
        out[k] = rec
    return out, new_flags, gaps
