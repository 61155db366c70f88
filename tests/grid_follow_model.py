"""The grid that follows the ego in plain Python / numpy, written from DESIGN.md §4g (not from the kernel).

`advance` is one pp_advance_async of a handle with a GridFollow model.  It wraps the existing models without editing them:
ego_model.advance / route_model.advance run on a copy of the configuration with grid_stage = 0 (so they make no OFF_GRID test and
carry grid_origin and goal over), then every scene that entered with flag 0 and came out without BAD_PATH takes the follow step on
its new position, and the OFF_GRID test of §4c 6. runs on the new frame when the real grid_stage is on.  With gf None it returns
exactly what the wrapped model returns.  Python floats are IEEE doubles and every expression is evaluated left to right as §4g
writes it, so the eight words of grid_origin and goal are meant to equal the device's bit for bit."""
import math

import numpy as np

import ego_model as em
import route_model as rmod

OFF_GRID, BAD_PATH = em.OFF_GRID, em.BAD_PATH


def _floor(v):
    """floor as IEEE has it: an infinity or a NaN is its own floor."""
    return float(math.floor(v)) if math.isfinite(v) else v


def follow_frame(ox, oy, x, y, gx, gy, W, H, cell, M):
    """§4g 1. - 3. for one scene: (origin'.x, origin'.y, goal'.x, goal'.y), or None when the step is skipped (non-finite goal point)."""
    if not (math.isfinite(gx) and math.isfinite(gy)):
        return None
    ex, cx = _floor((x - ox) / cell), _floor((gx - ox) / cell)
    ey, cy = _floor((y - oy) / cell), _floor((gy - oy) / cell)
    held = M <= ex < W - M and M <= cx < W - M and M <= ey < H - M and M <= cy < H - M          # (a NaN compares false)
    if held:
        return ox, oy, gx, gy
    mx = 0.5 * (x + gx)
    my = 0.5 * (y + gy)
    return (_floor(mx / cell) - float(W // 2)) * cell, (_floor(my / cell) - float(H // 2)) * cell, gx, gy


def off_grid(ox, oy, x, y, W, H, cell):
    """§4c 6. on the frame (ox, oy)."""
    fx, fy = _floor((x - ox) / cell), _floor((y - oy) / cell)
    return not (0 <= fx < W and 0 <= fy < H)


def follow(cfg, gf, scene_in, plan, flags_in, out, flags_out):
    """The follow step on the result (out, flags_out) of a wrapped model that ran with grid_stage = 0.  Returns (out, flags)."""
    out, flags = out.copy(), np.array(flags_out, np.int32).copy()
    W, H, cell = int(cfg["grid_w"][0]), int(cfg["grid_h"][0]), float(cfg["cell"][0])
    grid_stage = int(cfg["grid_stage"][0]) != 0
    k, M = (int(gf["goal_point"][0]), int(gf["margin_cells"][0])) if gf is not None else (0, 0)
    for s in range(len(scene_in)):
        if int(flags_in[s]) != 0 or int(flags[s]) & BAD_PATH:
            continue                                       # frozen on the way in, or BAD_PATH: the record is carried over
        x, y = float(out["loc"]["globalpoint"]["x"][s]), float(out["loc"]["globalpoint"]["y"][s])
        ox, oy = float(scene_in["grid_origin"]["x"][s]), float(scene_in["grid_origin"]["y"][s])
        if k > 0:
            g = plan["road_points"][s][k]
            fr = follow_frame(ox, oy, x, y, float(g["x"]), float(g["y"]), W, H, cell, M)
            if fr is not None:
                ox, oy = fr[0], fr[1]
                out["grid_origin"]["x"][s], out["grid_origin"]["y"][s] = ox, oy
                out["goal"][s] = g                          # (an exact copy)
        if grid_stage and off_grid(ox, oy, x, y, W, H, cell):
            flags[s] |= OFF_GRID
    return out, flags


def advance(dm, cfg, model, gf, scene_in, plan, state, flags, lane_pool=None, map_mode=False, route=None):
    """One advance of the batch.  route None: ego_model.advance on lane_pool (slice mode, or map mode on a map's point pool);
    route = (rm, legs, route_first, map): route_model.advance.  gf None: the wrapped model itself, on the real configuration."""
    def wrapped(c):
        if route is not None:
            rm, legs, rf, m = route
            return rmod.advance(dm, c, model, rm, legs, rf, m, scene_in, plan, state, flags)
        return em.advance(c, model, scene_in, plan, state, flags, lane_pool, map_mode)
    if gf is None:
        return wrapped(cfg)
    c0 = cfg.copy()
    c0["grid_stage"] = 0
    out, f, gaps = wrapped(c0)
    out, f = follow(cfg, gf, scene_in, plan, np.asarray(flags), out, f)
    return out, f, gaps
