"""The perception model in plain Python / numpy, written from DESIGN.md §4w (not from the kernel).

`step` is what k_perceive does on one tick: it takes the tracks (one per POOL entry), the stats (one per scene), the model, the
configuration, the tick id T, the SceneIn records and the TRUTH snapshot of the tick (what BUF_OBS_NOW holds: the pool moved by the
constant-velocity model), and returns the perceived snapshot.  Python floats are IEEE doubles and every expression is evaluated left to
right as the specification writes it; the hash is done in Python integers masked to 64 bits, with the one copy of §4l's mixer
(episode_spawn_model.mix) and of §4q's heading (ego_track_model.heading)."""
import math
import struct

import numpy as np

import ego_track_model as etm
import episode_spawn_model as esm

HIDDEN_XY = 1.0e12
_M64 = (1 << 64) - 1
OUT, OCCLUDED, MISSED, DETECTED = 0, 1, 2, 3          # causes, in the order they are tried
FRESH, COASTED, HIDDEN = 0, 1, 2                      # outputs


def new_tracks(dtype, n):
    return np.zeros(n, dtype)


def new_stats(dtype, n):
    st = np.zeros(n, dtype)
    st["min_hidden_clearance"], st["min_hidden_tick"], st["min_hidden_obs"] = np.inf, -1, -1
    return st


def hash0(seed, s, j, T):
    """§4w 3.: h0 of entry j of scene s on tick T."""
    return esm.mix((esm.mix((esm.mix((int(seed) + int(s)) & _M64) + int(j)) & _M64) + int(T)) & _M64)


def normal(w):
    """§4w 4.: the deviate of one mixed word - its four 16-bit fields summed, centred, scaled."""
    a = (w & 0xFFFF) + ((w >> 16) & 0xFFFF) + ((w >> 32) & 0xFFFF) + ((w >> 48) & 0xFFFF)
    return float(a - 131070) / 37837.0


def _f32bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _mul(a, b):
    return a * b          # (a Python float product is the IEEE product: no exception on overflow or inf * 0)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def in_view(m, x, y, hx, hy, ego_ok, ox, oy):
    """§4w 1.: (in view, dx, dy, d2)."""
    dx, dy = ox - x, oy - y
    d2 = _mul(dx, dx) + _mul(dy, dy)
    rng = float(m["range"])
    ok = ego_ok and d2 <= _mul(rng, rng)
    chf = float(m["cos_half_fov"])
    if ok and not chf <= -1.0:
        ok = _mul(dx, hx) + _mul(dy, hy) >= _mul(chf, math.sqrt(d2)) if d2 >= 0 else False
    return bool(ok), dx, dy, d2


def occluded(x, y, truth, j, dx, dy, d2):
    """§4w 2.: some other entry, strictly nearer, whose disc the sight line to the centre of entry j passes through."""
    for k in range(len(truth)):
        R = float(truth[k]["radius"])
        if not (math.isfinite(R) and R > 0):
            continue
        kdx, kdy = float(truth[k]["x"]) - x, float(truth[k]["y"]) - y
        kd2 = _mul(kdx, kdx) + _mul(kdy, kdy)
        if not kd2 < d2:
            continue
        t = _div(_mul(kdx, dx) + _mul(kdy, dy), d2)
        if not t > 0:
            continue
        t = min(t, 1.0)
        px, py = kdx - _mul(t, dx), kdy - _mul(t, dy)
        if _mul(px, px) + _mul(py, py) <= _mul(R, R):
            return True
    return False


def step_scene(tracks, stats, m, cfg, T, s, si, truth_pool, seen_pool, age0, obs_cap):
    """One scene of one tick; returns [(cause, output)] per entry."""
    x, y, d = (float(si["loc"]["globalpoint"][f]) for f in ("x", "y", "dir"))
    off, n = int(si["obs_off"]), int(si["obs_n"])
    if off < 0 or n < 0 or off + n > obs_cap:
        n = 0
    ego_ok = math.isfinite(x) and math.isfinite(y) and math.isfinite(d)
    hx, hy = etm.heading(d)
    hw = 0.5 * float(cfg["Vehicle_Width"][0])
    truth = truth_pool[off:off + n]
    log = []
    S = stats[s]
    S["n_ticks"] += 1
    S["n_entries"] += n
    best, best_j = 0.0, -1
    for j in range(n):
        o = truth[j]
        ox, oy = float(o["x"]), float(o["y"])
        view, dx, dy, d2 = in_view(m, x, y, hx, hy, ego_ok, ox, oy)
        dist = math.sqrt(d2) if d2 >= 0 else math.nan
        h0 = hash0(m["seed"], s, j, T)
        if not view:
            cause = OUT
        elif int(m["occlusion"]) and occluded(x, y, truth, j, dx, dy, d2):
            cause = OCCLUDED
        elif (h0 >> 32) < int(m["p_miss"]):
            cause = MISSED
        else:
            cause = DETECTED
        S[("n_out", "n_occluded", "n_missed", "n_detected")[cause]] += 1
        tr = tracks[off + j]
        if age0 or int(tr["last"]["type"]) != int(o["type"]) or _f32bits(tr["last"]["radius"]) != _f32bits(o["radius"]):
            tr["last"]["x"], tr["last"]["y"], tr["hits"], tr["misses"], tr["confirmed"] = 0.0, 0.0, 0, 0, 0
        tr["last"]["type"], tr["last"]["radius"] = o["type"], o["radius"]
        out = np.zeros(1, truth_pool.dtype)[0]
        out["x"], out["y"], out["type"], out["radius"] = HIDDEN_XY, HIDDEN_XY, o["type"], 0.0
        kind = HIDDEN
        if cause == DETECTED:
            tr["hits"], tr["misses"] = min(int(tr["hits"]) + 1, 65535), 0
            if int(tr["hits"]) > int(m["confirm"]):
                tr["confirmed"] = 1
            if tr["confirmed"]:
                out = o.copy()
                sigma = float(m["sigma0"]) + _mul(float(m["sigma_gain"]), dist)
                if sigma > 0:
                    out["x"] = ox + _mul(sigma, normal(esm.mix((h0 + 1) & _M64)))
                    out["y"] = oy + _mul(sigma, normal(esm.mix((h0 + 2) & _M64)))
                tr["last"] = out
                kind = FRESH
        else:
            tr["hits"] = 0
            if tr["confirmed"]:
                tr["misses"] = min(int(tr["misses"]) + 1, 65535)
                if int(tr["misses"]) <= int(m["coast"]):
                    out, kind = tr["last"].copy(), COASTED
                else:
                    tr["confirmed"] = 0
        seen_pool[off + j] = out
        S[("n_fresh", "n_coasted", "n_hidden")[kind]] += 1
        if kind == HIDDEN:
            cl = dist - float(o["radius"]) - hw
            if cl == cl and (best_j < 0 or cl < best):
                best, best_j = cl, j
        log.append((cause, kind))
    if best_j >= 0 and best < float(S["min_hidden_clearance"]):
        S["min_hidden_clearance"], S["min_hidden_tick"], S["min_hidden_obs"], S["min_hidden_type"] = best, T, best_j, truth[best_j]["type"]
    return log


def step(tracks, stats, model, cfg, T, scene_in, truth_pool, ep_stats=None, obs_cap=None, seen_pool=None):
    """One tick.  Returns (perceived pool, [[(cause, output)] per scene]); entries no slice covers keep what seen_pool held (zeros)."""
    m = np.array(model).reshape(1)[0]
    seen = np.zeros(len(truth_pool), truth_pool.dtype) if seen_pool is None else seen_pool
    cap = len(truth_pool) if obs_cap is None else int(obs_cap)
    logs = []
    for s in range(len(scene_in)):
        age0 = ep_stats is not None and int(ep_stats[s]["age"]) == 0
        logs.append(step_scene(tracks, stats, m, cfg, int(T), s, scene_in[s], truth_pool, seen, age0, cap))
    return seen, logs
