"""The conflict score in plain Python / numpy, written from DESIGN.md §4u (not from the kernel).

`step` is what one scored tick does to the ConflictScore records of a batch and to the previous-snapshot buffer: SceneIn the tick
read, its obstacle snapshot and - while episodes are on - EpisodeStats in; the records updated in place, the buffer of the next
tick returned.  It runs IN FRONT of the scorecard's fold of the tick and reads nothing of it.  Python floats are IEEE doubles and
every expression is evaluated left to right as the specification writes it, so the records are meant to equal the device's byte
for byte."""
import math

import numpy as np


def new_scores(dtype, n):
    """§4u 0.: the starting values."""
    r = np.zeros(n, dtype)
    r["min_ttc"] = math.inf
    r["min_ttc_tick"], r["min_ttc_obs"], r["first_crit_tick"], r["max_drac_tick"] = -1, -1, -1, -1
    return r


def new_prev(ob_dtype, cap=0):
    """The previous-snapshot buffer.  What it holds at the start is never read (prev_n = 0): zero here."""
    return np.zeros(cap, ob_dtype)


def _div(a, b):
    """a / b as IEEE does it (Python raises on b == 0)."""
    if b != 0 or b != b:
        return a / b
    if a != a or a == 0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def entry(model, ego_ok, ux, uy, x, y, h, dt, o, p):
    """§4u 2.: (ttc_j or None, drac_j or None) of one entry; o, p: (x, y, type, radius) now and one scored tick ago, p None without one."""
    if not ego_ok or p is None:
        return None, None
    lim = float(model["v_max"]) * dt
    gx, gy = o[0] - p[0], o[1] - p[1]
    if not (p[2] == o[2] and p[3] == o[3] and math.sqrt(gx * gx + gy * gy) <= lim):
        return None, None
    px, py = o[0] - x, o[1] - y
    wx, wy = gx / dt - ux, gy / dt - uy
    R = o[3] + h
    q = px * px + py * py
    c = q - R * R
    if c <= 0:
        return 0.0, None
    dist, b = math.sqrt(q), px * wx + py * wy
    vc = _div(-b, dist)
    if not vc > float(model["min_closing"]):
        return None, None
    a = wx * wx + wy * wy
    disc = b * b - a * c
    if not disc >= 0:
        return None, None
    ttc = _div(c, (-b) + math.sqrt(disc))
    gap = dist - R
    return ttc, (_div(vc * vc, 2 * gap) if gap > 0 else None)


def step_scene(C, model, cfg, dt, si, now, prev, age, obs_cap):
    """One scene, one tick.  C: its record (a numpy void that writes through); now / prev: the whole buffers; age: EpisodeStats.age or
    None while episodes are off.  Returns (off, m): the entries of `now` that go into the buffer of the next tick."""
    k = int(C["n_ticks"])
    x, y = float(si["loc"]["globalpoint"]["x"]), float(si["loc"]["globalpoint"]["y"])
    off, m = int(si["obs_off"]), int(si["obs_n"])
    if off < 0 or m < 0 or off + m > obs_cap:
        m = 0
    h = 0.5 * float(cfg["Vehicle_Width"][0])
    # 1. ego history
    hist = k > 0 and not (age is not None and int(age) == 0)
    ex, ey = x - float(C["last_pos"]["x"]), y - float(C["last_pos"]["y"])
    ego_ok = hist and math.sqrt(ex * ex + ey * ey) <= float(model["v_max"]) * dt
    ux, uy = ex / dt, ey / dt
    if k > 0 and not ego_ok:
        C["n_no_history_ticks"] += 1
    # 2., 3. entries and their reduction
    same, prev_n = int(C["prev_off"]) == off, int(C["prev_n"])
    t_best, j_best, D = None, -1, 0.0
    for j in range(m):
        o = now[off + j]
        o = (float(o["x"]), float(o["y"]), int(o["type"]), float(o["radius"]))          # (float32 -> double is exact)
        p = None
        if same and j < prev_n:
            p = prev[off + j]
            p = (float(p["x"]), float(p["y"]), int(p["type"]), float(p["radius"]))
        ttc, drac = entry(model, ego_ok, ux, uy, x, y, h, dt, o, p)
        if ttc is not None and ttc == ttc and (t_best is None or ttc < t_best):
            t_best, j_best = ttc, j
        if drac is not None and drac > D:
            D = drac
    # 4. fold
    if t_best is not None:
        C["n_conflict_ticks"] += 1
        if t_best < float(C["min_ttc"]):
            C["min_ttc"], C["min_ttc_tick"], C["min_ttc_obs"], C["min_ttc_type"] = t_best, k, j_best, int(now["type"][off + j_best])
        if t_best <= float(model["ttc_warn"]):
            C["n_warn_ticks"] += 1
            C["tit_warn"] = float(C["tit_warn"]) + (float(model["ttc_warn"]) - t_best) * dt
        if t_best <= float(model["ttc_crit"]):
            C["n_crit_ticks"] += 1
            if int(C["first_crit_tick"]) == -1:
                C["first_crit_tick"] = k
        if D > float(C["max_drac"]):
            C["max_drac"], C["max_drac_tick"] = D, k
    # 5. state
    C["last_pos"]["x"], C["last_pos"]["y"], C["prev_off"], C["prev_n"], C["n_ticks"] = x, y, off, m, k + 1
    return off, m


def step(scores, prev, model, cfg, dt_score, scene_in, obs_now, ep_stats=None, obs_cap=None):
    """The batch, records in place; returns the previous-snapshot buffer of the next tick.  Every scene reads `prev` as it stood in
    front of the tick, whatever the other scenes store."""
    model = np.asarray(model).reshape(-1)[0]
    cap = len(obs_now) if obs_cap is None else int(obs_cap)
    nxt = np.zeros(max(len(prev), len(obs_now)), obs_now.dtype)
    nxt[:len(prev)] = prev
    for s in range(len(scene_in)):
        off, m = step_scene(scores[s], model, cfg, float(dt_score), scene_in[s], obs_now, prev, None if ep_stats is None else int(ep_stats["age"][s]), cap)
        nxt[off:off + m] = obs_now[off:off + m]
    return nxt
