"""The ego tracking model in plain Python / numpy, written from DESIGN.md §4q (not from the kernel).

`advance` is one pp_advance_async of a handle with an EgoTracker.  It wraps the existing models without editing them: the pose step
of ego_model / route_model is the one function ego_model.walk_path, and for the length of one call that name is bound to the tracked
pose step below (every unfrozen scene calls it once, in scene order), so speed, distance, ids, lane number, the routed step, the
grid test and - through grid_follow_model - the following grid are the wrapped models' own.  With tk None it returns exactly what
the wrapped model returns.  Python floats are IEEE doubles and every expression is evaluated left to right as §4q writes it, so
every field of EgoTrackState and the staged x, y, velocity are meant to equal the device's bit for bit; `dir` (and with it key_dir,
which is defined as the bits of the dir that was stored) goes through atan."""
import math
import struct
from unittest import mock

import numpy as np

import ego_model as em
import grid_follow_model as gfm

PATH_END, BAD_PATH = em.PATH_END, em.BAD_PATH
N_PATH = em.N_PATH
DEG = 0.017453292519943295          # the double nearest to pi / 180
# 1 / n! for n = 1, 3 .. 17 and n = 0, 2 .. 16, signs alternating: the Taylor coefficients of sin and cos (§4q 1.)
SIN_C = (1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08,
         1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15)
COS_C = (1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
         2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14)


def bits(v):
    """The 64 bits of a double."""
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def heading(d):
    """§4q 1.: the unit heading (hx, hy) of an angle in degrees, by the fixed polynomial."""
    d = float(d)
    if not math.isfinite(d):
        return 1.0, 0.0
    q = float(math.floor((d + 45.0) / 90.0))
    r = d - q * 90.0
    qi = int(q - 4.0 * float(math.floor(q / 4.0)))
    x = r * DEG
    x2 = x * x
    ps = SIN_C[8]
    for k in range(7, -1, -1):
        ps = ps * x2 + SIN_C[k]
    sn = ps * x
    pc = COS_C[8]
    for k in range(7, -1, -1):
        pc = pc * x2 + COS_C[k]
    cs = pc
    ax, ay = ((cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs))[qi]
    n = math.sqrt(ax * ax + ay * ay)
    return _div(ax, n), _div(ay, n)


def walk(px, py, k0, d):
    """The arc walk of §4c 3. as §4q 2. factors it: (x, y, seg, bad, ran_out).  d <= 0 or NaN: P[k0]."""
    x, y, seg = float(px[k0]), float(py[k0]), -1
    if not d > 0:
        return x, y, seg, False, False
    a = 0.0
    for i in range(k0, N_PATH - 1):
        x0, y0, x1, y1 = float(px[i]), float(py[i]), float(px[i + 1]), float(py[i + 1])
        dx, dy = x1 - x0, y1 - y0
        L = math.sqrt(dx * dx + dy * dy)
        if not math.isfinite(L):
            return x, y, seg, True, False
        if L == 0:
            continue
        seg = i
        if a + L >= d:
            t = (d - a) / L
            return x0 + t * dx, y0 + t * dy, seg, False, False
        a = a + L
    return float(px[N_PATH - 1]), float(py[N_PATH - 1]), seg, False, True


def command(px, py, hx, hy, tx, ty, max_curv):
    """§4q 3., first half: (kc after the clamp, 1 if it met a bound)."""
    ex, ey = tx - px, ty - py
    ly = ey * hx - ex * hy
    d2 = ex * ex + ey * ey
    kc = 0.0
    if d2 != 0:
        kc = _div(2.0 * ly, d2)
    if kc != kc:
        kc = 0.0
    sat = 0
    if kc >= max_curv:
        kc, sat = max_curv, 1
    if kc <= -max_curv:
        kc, sat = -max_curv, 1
    return kc, sat


def rate_limit(kappa, kc, curv_rate, dt):
    """§4q 3., second half: kappa moves towards kc by at most curv_rate * dt."""
    dk = curv_rate * dt
    lo, hi = kappa - dk, kappa + dk
    kn = kc
    if kn > hi:
        kn = hi
    if kn < lo:
        kn = lo
    return kn


def move(px, py, hx, hy, ka, s, n_sub):
    """§4q 4.: n_sub substeps of half turn, move, half turn, renormalise.  Returns (x, y, hx, hy)."""
    if not s > 0:
        return px, py, hx, hy
    ds = s / float(n_sub)
    t = 0.25 * ka * ds
    t2 = t * t
    den = 1.0 + t2
    rc, rs = _div(1.0 - t2, den), _div(2.0 * t, den)
    for _ in range(n_sub):
        mx, my = rc * hx - rs * hy, rs * hx + rc * hy
        px, py = px + ds * mx, py + ds * my
        nx, ny = rc * mx - rs * my, rs * mx + rc * my
        n = math.sqrt(nx * nx + ny * ny)
        hx, hy = _div(nx, n), _div(ny, n)
    return px, py, hx, hy


def _tk(tk):
    t = np.asarray(tk).reshape(-1)[0]
    return (float(t["look_min"]), float(t["look_gain"]), float(t["max_curv"]), float(t["curv_rate"]), float(t["curv_bias"]), int(t["n_sub"]))


def track_pose(cfg, tk, dt, S, x, y, d, vn, s, px, py, k0, age0):
    """§4q for one unfrozen scene.  S: its EgoTrackState record; (x, y, d): loc.globalpoint of the record the advance reads; vn, s:
    §4c 1. - 2.  Returns (x', y', dir', flags, S'): flags 0, PATH_END or BAD_PATH - with BAD_PATH S' is S and the pose is meaningless."""
    look_min, look_gain, max_curv, curv_rate, curv_bias, n_sub = _tk(tk)
    k0 = min(max(int(k0), 0), N_PATH - 1)
    if not (math.isfinite(s) and math.isfinite(float(px[k0])) and math.isfinite(float(py[k0]))):
        return x, y, d, BAD_PATH, S
    _, _, _, bad, ran_out = walk(px, py, k0, s)
    if bad:
        return x, y, d, BAD_PATH, S
    ld = look_min + look_gain * vn / 3.6
    tx, ty, _, bad, _ = walk(px, py, k0, ld)
    if bad or not (math.isfinite(tx) and math.isfinite(ty)):
        return x, y, d, BAD_PATH, S
    S = S.copy()
    hx, hy, kappa = float(S["hx"]), float(S["hy"]), float(S["kappa"])
    stale = int(S["valid"]) == 0 or int(S["key_x"]) != bits(x) or int(S["key_y"]) != bits(y) or int(S["key_dir"]) != bits(d) or bool(age0)
    if stale:
        hx, hy = heading(d)
        kappa = 0.0
        S["n_init"] = int(S["n_init"]) + 1
    kc, sat = command(x, y, hx, hy, tx, ty, max_curv)
    kn = rate_limit(kappa, kc, curv_rate, dt)
    S["kappa"], S["n_sat"] = kn, int(S["n_sat"]) + sat
    if abs(kn) > float(S["max_kappa"]):
        S["max_kappa"] = abs(kn)
    ka = kn + curv_bias
    x, y, hx, hy = move(x, y, hx, hy, ka, s, n_sub)
    d = em.road_angle(cfg, 0.0, 0.0, hx, hy)
    S["hx"], S["hy"], S["key_x"], S["key_y"], S["key_dir"], S["valid"], S["_pad"] = hx, hy, bits(x), bits(y), bits(d), 1, 0
    return x, y, d, (PATH_END if ran_out else 0), S


def advance(dm, cfg, model, tk, states, scene_in, plan, state, flags, age0=None, gf=None, lane_pool=None, map_mode=False, route=None):
    """One advance of the batch: gfm.advance (ego_model.advance on lane_pool, or route_model.advance with route = (rm, legs,
    route_first, map); gf: the GridFollow model or None) with the pose step of §4q.  states: EgoTrackState[n]; age0: per scene,
    whether episodes are on and EpisodeStats.age is 0 (None: episodes off).  Returns (SceneIn, flags, gaps, states').  tk None: the
    wrapped model itself, the states unchanged."""
    if tk is None:
        return gfm.advance(dm, cfg, model, gf, scene_in, plan, state, flags, lane_pool, map_mode, route) + (states,)
    new_states = states.copy()
    todo = [k for k in range(len(scene_in)) if int(flags[k]) == 0]
    dt, max_acc, max_dec = float(model["dt"][0]), float(model["max_acc"][0]), float(model["max_dec"][0])

    def tracked(c, px, py, k0, s, dir0):
        k = todo.pop(0)
        si, R = scene_in[k], plan[k]["result"]
        g = si["loc"]["globalpoint"]
        vn = em.next_speed(float(si["loc"]["velocity"]), int(R["desaccVd"]), float(R["desacc"]), float(R["desspd"]), dt, max_acc, max_dec)
        x, y, d, f, S = track_pose(cfg, tk, dt, new_states[k], float(g["x"]), float(g["y"]), float(g["dir"]), vn, s, px, py, k0,
                                   age0 is not None and bool(age0[k]))
        new_states[k] = S
        return x, y, d, f

    with mock.patch.object(em, "walk_path", tracked):
        out, f, gaps = gfm.advance(dm, cfg, model, gf, scene_in, plan, state, flags, lane_pool, map_mode, route)
    assert not todo, "every unfrozen scene takes the pose step once"
    return out, f, gaps, new_states
