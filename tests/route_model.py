"""The route step of the closed-loop rollout in plain Python / numpy, written from DESIGN.md §4f (not from the kernel).

`advance` is one pp_advance_async on a handle with routes set: the SceneIn records, PlanOut and SceneState of tick t, the
flag words, the routes and the map in; the SceneIn records of tick t + 1 and the new flag words out.  The shared steps (speed,
distance, pose, the windowed nearest-point search) are those of tests/ego_model.py; a scene that follows no route is
ego_model.advance_scene itself.  With resolve=True the lane views and junction slices of the result are derived again
(map_scenes.resolve), as k_resolve_map does behind the kernel, so the result is meant to equal the staged records byte for byte."""
import math

import numpy as np

import ego_model as em
import map_scenes as ms

PATH_END, BAD_PATH, LANE_END, OFF_GRID, ROUTE_END = 1, 2, 4, 8, 16
LANESUM = em.LANESUM


def find_junction(m, road, next_road, lane):
    """J(road, next_road, lane): the lowest-index junction with these three keys, or None."""
    for q in m["junctions"]:
        if int(q["last_road"]) == road and int(q["next_road"]) == next_road and int(q["last_lane"]) == lane:
            return q
    return None


def _views(si, n):
    V = si["lanes"]
    views = {}
    if 1 <= n <= LANESUM and int(V["cur_n"]) > 0:
        views["cur"] = (n - 1, int(V["cur_off"]), int(V["cur_n"]))
    if 2 <= n <= LANESUM + 1 and int(V["left_n"]) > 0:
        views["left"] = (n - 2, int(V["left_off"]), int(V["left_n"]))
    if 0 <= n < min(int(V["lane_sum"]), LANESUM) and int(V["right_n"]) > 0:
        views["right"] = (n, int(V["right_off"]), int(V["right_n"]))
    return views


def _search(views, ids, window, x, y, lane_x, lane_y):
    """§4c 4. from the ids given: (found: view -> d2, ids with the new ids written, smallest gap)."""
    found, gap, ids = {}, math.inf, ids.copy()
    start = ids.copy()
    for name, (slot, off, cnt) in views.items():
        i, d2, g = em.nearest_in_window(lane_x[off:off + cnt], lane_y[off:off + cnt], cnt, int(start[slot]), window, x, y)
        gap = min(gap, g)
        if i is not None:
            found[name] = d2
            ids[slot] = i
    return found, ids, gap


def advance_scene(cfg, model, rm, legs, m, si, po, st, flag, lane_x, lane_y, ref_x, ref_y):
    """One scene; legs: the RouteLeg records of ITS route.  Returns (new SceneIn record, new flag word, smallest id gap)."""
    p, pos, n_legs = int(si["loc"]["path_num"]), int(si["loc"]["pos"]), len(legs)
    if flag != 0 or n_legs == 0 or not 0 <= p < n_legs or pos not in (0, 1, 2):
        return em.advance_scene(cfg, model, si, po, st, flag, lane_x, lane_y, True)
    out = si.copy()
    dt, max_acc, max_dec = float(model["dt"][0]), float(model["max_acc"][0]), float(model["max_dec"][0])
    window, pre_points = int(model["window"][0]), int(np.asarray(rm).reshape(-1)[0]["pre_points"])
    R = po["result"]
    v = float(si["loc"]["velocity"])
    vn = em.next_speed(v, int(R["desaccVd"]), float(R["desacc"]), float(R["desspd"]), dt, max_acc, max_dec)
    s = em.step_length(v, vn, dt)
    P = po["road_points"]
    k0 = 0 if int(st["afresh_planning"]) != 0 else int(st["path_near_id"])
    x, y, d, f = em.walk_path(cfg, P["x"], P["y"], k0, s, float(si["loc"]["globalpoint"]["dir"]))
    if f & BAD_PATH:
        return out, BAD_PATH, math.inf
    loc = out["loc"]
    loc["globalpoint"]["x"], loc["globalpoint"]["y"], loc["globalpoint"]["dir"], loc["velocity"] = x, y, d, vn
    n, V = int(si["loc"]["lane_num"]), si["lanes"]
    ref_off, ref_n = int(si["ref_off"]), int(si["ref_n"])
    gap = math.inf
    if pos in (0, 1):
        views = _views(si, n)
        found, ids, gap = _search(views, si["loc"]["id"], window, x, y, lane_x, lane_y)
        loc["id"] = ids
        lane2 = n
        if pos == 0 and "cur" in found:
            rc, w = math.sqrt(found["cur"]), 0.25 * float(V["lane_width"])
            if "left" in found and rc - math.sqrt(found["left"]) > w:
                lane2 = n - 1
            elif "right" in found and rc - math.sqrt(found["right"]) > w:
                lane2 = n + 1
            loc["lane_num"] = lane2
        if "cur" in views:
            id2, n_c = int(ids[views["cur"][0]]), views["cur"][2]
            has_next = p + 1 < n_legs
            Jn = None
            if has_next and not (pos == 1 and ref_n <= 0):
                Jn = find_junction(m, int(si["loc"]["road_num"]), int(legs[p + 1]["road_num"]), lane2)
            if id2 + window >= n_c:
                if not has_next:
                    f |= LANE_END | ROUTE_END
                elif Jn is None:
                    f |= LANE_END
            if pos == 0 and Jn is not None and n_c - 1 - id2 <= pre_points:
                loc["pos"] = 1
                loc["last_roadnum"], loc["next_roadnum"] = int(si["loc"]["road_num"]), int(legs[p + 1]["road_num"])
                loc["last_lanenum"], loc["next_lanenum"] = lane2, int(Jn["next_lane"])
            if pos == 1 and id2 == n_c - 1 and ref_n > 0:
                loc["pos"] = 2
                loc["road_num"], loc["lane_num"] = int(si["loc"]["next_roadnum"]), int(si["loc"]["next_lanenum"])
                ids = np.zeros(LANESUM, np.int32)
                i, _, g = em.nearest_in_window(ref_x[ref_off:ref_off + ref_n], ref_y[ref_off:ref_off + ref_n], ref_n, 0, window, x, y)
                gap = min(gap, g)
                ids[min(max(int(si["loc"]["last_lanenum"]) - 1, 0), LANESUM - 1)] = 0 if i is None else i
                loc["id"] = ids
    else:
        slot = min(max(int(si["loc"]["last_lanenum"]) - 1, 0), LANESUM - 1)
        j = int(si["loc"]["id"][slot])
        i, _, gap = em.nearest_in_window(ref_x[ref_off:ref_off + ref_n], ref_y[ref_off:ref_off + ref_n], ref_n, j, window, x, y)
        j2 = j if i is None else i
        ids = si["loc"]["id"].copy()
        ids[slot] = j2
        loc["id"] = ids
        if j2 >= ref_n - 1:
            if p + 1 >= n_legs:
                f |= ROUTE_END
            else:
                loc["pos"], loc["path_num"] = 0, p + 1
                out["out_lane_no"] = legs[p + 1]["out_lane_no"]
                out["stub_attribute"] = int(legs[p + 1]["stub_attribute"])
                found, ids, g = _search(_views(si, n), np.zeros(LANESUM, np.int32), window, x, y, lane_x, lane_y)
                gap = min(gap, g)
                loc["id"] = ids
    if int(cfg["grid_stage"][0]):
        cell = float(cfg["cell"][0])
        fx = math.floor((x - float(si["grid_origin"]["x"])) / cell)
        fy = math.floor((y - float(si["grid_origin"]["y"])) / cell)
        if not (0 <= fx < int(cfg["grid_w"][0]) and 0 <= fy < int(cfg["grid_h"][0])):
            f |= OFF_GRID
    return out, f, gap


def advance(dm, cfg, model, rm, legs, route_first, m, scene_in, plan, state, flags, resolve=True):
    """The batch.  legs / route_first: as given to pp_set_route (None: no scene is routed); m: the map dict of pp_set_map.
    Returns (SceneIn of the next tick, flag words, per-scene smallest gap between the two best squared distances of a search)."""
    out = scene_in.copy()
    new_flags = np.array(flags, np.int32).copy()
    gaps = np.full(len(scene_in), math.inf)
    lane_x, lane_y = np.ascontiguousarray(m["points"]["x"]), np.ascontiguousarray(m["points"]["y"])
    ref_x, ref_y = np.ascontiguousarray(m["jpoints"]["x"]), np.ascontiguousarray(m["jpoints"]["y"])
    none = np.zeros(0, dm.RouteLeg)
    for k in range(len(scene_in)):
        R = none if legs is None else legs[int(route_first[k]):int(route_first[k + 1])]
        rec, new_flags[k], gaps[k] = advance_scene(cfg, model, rm, R, m, scene_in[k], plan[k], state[k], int(flags[k]), lane_x, lane_y, ref_x, ref_y)
        out[k] = rec
    if resolve:
        out = ms.resolve(dm, m, out)
    return out, new_flags, gaps
