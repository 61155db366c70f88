"""The rollout scorecard in plain Python / numpy, written from DESIGN.md §4d (not from the kernels).

`fold` is what one scored tick does to the RolloutScore records of a batch: SceneIn the tick read, its PlanOut, SceneState
after it, its obstacle snapshot, the flag words its egos carried and - if it ran the grid stage - its GridOut in; the records
updated in place.  Python floats and numpy float64 are IEEE doubles, every expression is evaluated left to right as the
specification writes it and each numpy operation rounds once, so the records are meant to equal the device's byte for byte."""
import math

import numpy as np

G_STATUS_COUNT, G_INTERNAL, MAX_LATTICE = 8, 6, 17


def new_scores(dtype, n):
    """§4d 0.: the starting values."""
    r = np.zeros(n, dtype)
    r["min_clearance"] = math.inf
    r["min_clearance_tick"], r["min_clearance_obs"], r["first_collision_tick"] = -1, -1, -1
    return r


def snapshot(cfg, scene_in, state_before, obs_pool, mot_pool=None):
    """§5 G4 as k_effective_obstacles applies it: the obstacle pool of the tick, every scene's slice moved by
    v * (dyn_dt * tick) with the SceneState.tick the tick starts from.  Without motion: the pool itself."""
    now = obs_pool.copy()
    if mot_pool is None or not int(cfg["dynamic_obstacles"][0]):
        return now
    dyn_dt = float(cfg["dyn_dt"][0])
    for k in range(len(scene_in)):
        off, m = int(scene_in["obs_off"][k]), int(scene_in["obs_n"][k])
        t = dyn_dt * float(int(state_before["tick"][k]))
        now["x"][off:off + m] = obs_pool["x"][off:off + m] + mot_pool["vx"][off:off + m] * t
        now["y"][off:off + m] = obs_pool["y"][off:off + m] + mot_pool["vy"][off:off + m] * t
    return now


def clearance(x, y, ox, oy, radius, vehicle_width):
    """§4d 1.: (clearance, first index of the nearest obstacle edge), or (None, -1) for a tick without a clearance."""
    if len(ox) == 0:
        return None, -1
    dx = np.asarray(ox, np.float64) - x
    dy = np.asarray(oy, np.float64) - y
    with np.errstate(invalid="ignore", over="ignore"):          # (inf - inf is a NaN d_j, not a warning)
        d = np.sqrt(dx * dx + dy * dy) - np.asarray(radius, np.float32).astype(np.float64)
    ok = ~np.isnan(d)
    if not ok.any():
        return None, -1
    j = int(np.nanargmin(d))                     # first index of the smallest
    return float(d[j]) - 0.5 * vehicle_width, j


def fold_scene(r, cfg, dt_score, si, po, st, ox, oy, radius, flag, go=None):
    """One scene, one tick.  r: its RolloutScore record (a numpy void that writes through)."""
    k = int(r["n_ticks"])
    x, y, v = float(si["loc"]["globalpoint"]["x"]), float(si["loc"]["globalpoint"]["y"]), float(si["loc"]["velocity"])
    cl, j = clearance(x, y, ox, oy, radius, float(cfg["Vehicle_Width"][0]))
    if cl is not None:
        if cl < float(r["min_clearance"]):
            r["min_clearance"], r["min_clearance_tick"], r["min_clearance_obs"] = cl, k, j
        if cl <= 0:
            if int(r["first_collision_tick"]) < 0:
                r["first_collision_tick"] = k
            r["n_collision_ticks"] += 1
    if k > 0:
        ex, ey = x - float(r["last_pos"]["x"]), y - float(r["last_pos"]["y"])
        r["dist"] = float(r["dist"]) + math.sqrt(ex * ex + ey * ey)
        a = (v - float(r["last_speed"])) / 3.6 / dt_score
        if a > float(r["max_acc"]):
            r["max_acc"] = a
        if -a > float(r["max_dec"]):
            r["max_dec"] = -a
    if v > float(r["max_speed"]):
        r["max_speed"] = v
    r["last_pos"]["x"], r["last_pos"]["y"], r["last_speed"] = x, y, v
    if int(st["afresh_planning"]) != 0:
        r["n_replans"] += 1
    if int(po["ob_flag"]) != 0:
        r["n_ob_flag"] += 1
    if int(po["result"]["desaccVd"]) != 0:
        r["n_desacc"] += 1
    r["behavior_ticks"][min(max(int(po["dec"]["behavior"]), 0), 7)] += 1
    r["ego_flags"] = int(flag)
    r["n_ticks"] = k + 1
    if go is not None:
        s = int(go["status"])
        if not 0 <= s < G_STATUS_COUNT:
            s = G_INTERNAL
        r["n_grid_ticks"] += 1
        r["grid_status_ticks"][s] += 1
        nc = int(go["n_candidates"])
        if nc == min(int(cfg["n_lattice"][0]), MAX_LATTICE - 1) + 1 and int(go["best_candidate"]) == nc - 1:
            r["n_grid_path_candidate"] += 1


def fold(scores, cfg, dt_score, scene_in, plan, state, obs_now, flags, grid=None):
    """The batch, in place.  obs_now: the tick's snapshot pool (`snapshot`); grid: GridOut of the tick or None."""
    ox, oy, rad = np.ascontiguousarray(obs_now["x"]), np.ascontiguousarray(obs_now["y"]), np.ascontiguousarray(obs_now["radius"])
    for k in range(len(scene_in)):
        off, m = int(scene_in["obs_off"][k]), int(scene_in["obs_n"][k])
        fold_scene(scores[k], cfg, dt_score, scene_in[k], plan[k], state[k], ox[off:off + m], oy[off:off + m], rad[off:off + m],
                   int(flags[k]), None if grid is None else grid[k])
    return scores
