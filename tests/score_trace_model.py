"""The score trace in plain Python / numpy, written from DESIGN.md §4o (not from the kernel).

`step` is what one scored tick does to the rings and headers of a batch, on the inputs of §4d plus the tick id and - while episodes
are on - EpisodeStats: it must run BEFORE the scorecard's own fold of the tick (rollout_score_model.fold), because it reads n_ticks
and last_speed of the RolloutScore records as they stand in front of it.  Python floats are IEEE doubles and every expression is
evaluated as the specification writes it, so rings and headers are meant to equal the device's byte for byte."""
import math

import numpy as np

import rollout_score_model as sm

TRACE_COLLISION, TRACE_NEAR, TRACE_FLAG, TRACE_BRAKE = 1, 2, 4, 8
TICK_REPLAN, TICK_OB_FLAG, TICK_DESACC, TICK_START = 1, 2, 4, 8
ARMED, POST, FROZEN = 0, 1, 2


def new_trace(tick_dtype, info_dtype, n, depth):
    """§4o 0.: (rings[n, depth], headers[n]) at their starting values.  A ring slot that was never written is not specified: zero here."""
    info = np.zeros(n, info_dtype)
    info["trigger_k"] = -1
    return np.zeros((n, depth), tick_dtype), info


def record(model, score, cfg, dt_score, tick_id, si, po, st, ox, oy, radius, ob_types, flag, age):
    """§4o 1., 2.: the ScoreTick of one scene's tick as a dict, and its cause word.  score: the scene's RolloutScore BEFORE the fold;
    ob_types: ObPoint.type of the slice; age: EpisodeStats.age, or None while episodes are off."""
    k = int(score["n_ticks"])
    x, y, v = float(si["loc"]["globalpoint"]["x"]), float(si["loc"]["globalpoint"]["y"]), float(si["loc"]["velocity"])
    cl, j = sm.clearance(x, y, ox, oy, radius, float(cfg["Vehicle_Width"][0]))
    marks = 0
    if int(st["afresh_planning"]) != 0:
        marks |= TICK_REPLAN
    if int(po["ob_flag"]) != 0:
        marks |= TICK_OB_FLAG
    if int(po["result"]["desaccVd"]) != 0:
        marks |= TICK_DESACC
    if age is not None and int(age) == 0:
        marks |= TICK_START
    c = 0
    if cl is not None and cl <= 0:
        c |= TRACE_COLLISION
    if cl is not None and cl <= float(model["near"]):
        c |= TRACE_NEAR
    if (int(flag) & int(model["flag_mask"])) != 0:
        c |= TRACE_FLAG
    if k > 0:
        a = (v - float(score["last_speed"])) / 3.6 / dt_score
        if -a >= float(model["brake"]):
            c |= TRACE_BRAKE
    c &= int(model["trigger"])
    rec = dict(k=k, flags=int(flag), tick=int(tick_id), x=x, y=y, v=v, clearance=math.inf if cl is None else cl,
               obs=j if cl is not None else -1, ob_type=int(ob_types[j]) if cl is not None else 0,
               behavior=int(po["dec"]["behavior"]), marks=marks | (c << 8))
    return rec, c


def advance_header(model, hd, ring, rec, c):
    """§4o 3., 4.: one scene's header `hd` and ring (numpy voids / rows that write through)."""
    depth, post = int(model["depth"]), int(model["post"])
    if c != 0:
        hd["n_trigger_ticks"] += 1
    state = int(hd["state"])
    if state == FROZEN:
        return
    slot = ring[int(hd["n_written"]) % depth]
    for f, val in rec.items():
        slot[f] = val
    hd["n_written"] += 1
    if state == ARMED and c != 0:
        hd["trigger_k"], hd["trigger"], hd["post_left"], hd["state"] = rec["k"], c, post, POST if post > 0 else FROZEN
    elif state == POST:
        hd["post_left"] -= 1
        if int(hd["post_left"]) == 0:
            hd["state"] = FROZEN


def step(rings, info, model, scores, cfg, dt_score, tick_id, scene_in, plan, state, obs_now, flags, ep_stats=None):
    """The batch, in place; scores: the RolloutScore records BEFORE this tick's fold (left alone)."""
    model = np.asarray(model).reshape(-1)[0]
    ox, oy, rad, typ = (np.ascontiguousarray(obs_now[f]) for f in ("x", "y", "radius", "type"))
    for s in range(len(scene_in)):
        off, m = int(scene_in["obs_off"][s]), int(scene_in["obs_n"][s])
        rec, c = record(model, scores[s], cfg, dt_score, tick_id, scene_in[s], plan[s], state[s], ox[off:off + m], oy[off:off + m], rad[off:off + m],
                        typ[off:off + m], int(flags[s]), None if ep_stats is None else int(ep_stats["age"][s]))
        advance_header(model, info[s], rings[s], rec, c)


def rearm(info, s):
    """pp_read_score_trace(rearm != 0): armed again; the ring and n_written stay."""
    info[s]["state"], info[s]["trigger_k"], info[s]["trigger"], info[s]["post_left"] = ARMED, -1, 0, 0


def oldest_first(rings, info, s):
    """What pp_read_score_trace copies: the min(n_written, depth) records of scene s, oldest first."""
    depth, w = rings.shape[1], int(info["n_written"][s])
    n = min(w, depth)
    return rings[s][[(w - n + i) % depth for i in range(n)]].copy()
