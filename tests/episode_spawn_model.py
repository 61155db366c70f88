"""The episode spawn model in plain Python / numpy, written from DESIGN.md §4l (not from the kernel): contact ends an episode, a
restart draws its start record from a pool of M per scene and skips the candidates that are not clear.

`step` is what the episode step of one pp_advance_async does while pp_set_episode_spawn is in force.  It takes what
episode_model.step takes, and: the spawn model, the EpisodeSpawnStats, the pool of start records - pool_in[k][s] / pool_state[k][s],
record 0 the capture of pp_set_episodes -, the obstacle pool `O` of the input set the advance read (plain entries, no motion),
half the vehicle width and the fleet's world_first (None without a fleet).  Python floats are IEEE doubles and every expression is
evaluated left to right as the specification writes it; the hash is done in Python integers, masked to 64 bits."""
import math

import numpy as np

import episode_model as epm

CONTACT = epm.CONTACT
MAX_STARTS = 16
_M64 = (1 << 64) - 1


def mix(z):
    """§4l 3a.: uint64 arithmetic mod 2^64."""
    z = (int(z) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def hash_u(seed, s, e):
    return mix((mix((int(seed) + int(s)) & _M64) + int(e)) & _M64)


def first_choice(seed, s, e, M, order):
    """k0 of scene s for its e-th ended episode."""
    if int(order) == 1:
        return int(e) % int(M)
    return ((hash_u(seed, s, e) >> 32) * int(M)) >> 32


def new_stats(dtype, n):
    return np.zeros(n, dtype)


def _within(ox, oy, radius, x, y, hw, lim):
    """(sqrt(dx dx + dy dy) - radius) - hw <= lim; a NaN compares false.  radius None: an ego, (… - hw) - hw."""
    dx, dy = float(ox) - float(x), float(oy) - float(y)
    sq = dx * dx + dy * dy
    d = math.sqrt(sq) if sq == sq else float("nan")
    d = d - (hw if radius is None else float(radius))
    return d - hw <= lim


def slice_within(O, off, n, x, y, hw, lim):
    return any(_within(O["x"][j], O["y"][j], np.float32(O["radius"][j]), x, y, hw, lim) for j in range(int(off), int(off) + int(n)))


def world_within(p, members, s, x, y, hw, lim):
    return any(_within(p["loc"]["globalpoint"]["x"][t], p["loc"]["globalpoint"]["y"][t], None, x, y, hw, lim) for t in members if t != s)


def step_scene(em, sp, s, e, se, pool_in, pool_state, p, q, flag, state, O, hw, members, trace=None, score=None):
    """One scene, one advance.  e / se: its EpisodeStats / EpisodeSpawnStats records (numpy voids that write through); p: the whole
    SceneIn array the advance read (the world test reads the other scenes of it); q, state: the scene's staged record and state;
    members: the scenes of its world or None.  Returns (staged SceneIn record, SceneState record, flag word, cause word)."""
    M, order, check, clearance = int(sp["n_starts"][0]), int(sp["order"][0]), int(sp["check"][0]), float(sp["clearance"][0])
    ps = p[s]
    px, py = float(ps["loc"]["globalpoint"]["x"]), float(ps["loc"]["globalpoint"]["y"])
    # 1.
    age, dist = epm.age_dist(e, ps, q)
    off, n = int(ps["obs_off"]), int(ps["obs_n"])
    # 1a.
    touch = int(sp["contact"][0]) != 0 and slice_within(O, off, n, px, py, hw, 0.0)
    # 2.
    c = epm.cause(flag, age, int(em["end_mask"][0]), int(em["max_ticks"][0])) | (CONTACT if touch else 0)
    if c == 0:
        epm.go_on(e, age, dist)
        return q, state, int(flag), 0
    # 3.
    epm.close(e, c, age, dist)
    if c & CONTACT:
        se["n_contact"] += 1
    # 3a.
    k0 = first_choice(int(sp["seed"][0]), s, int(e["n_episodes"]), M, order)
    k = None
    for i in range(M):
        cand = (k0 + i) % M
        X, Y = float(pool_in[cand][s]["loc"]["globalpoint"]["x"]), float(pool_in[cand][s]["loc"]["globalpoint"]["y"])
        blocked = bool(check & 1) and slice_within(O, off, n, X, Y, hw, clearance)
        blocked = blocked or (bool(check & 2) and members is not None and world_within(p, members, s, X, Y, hw, clearance))
        if not blocked:
            k = cand
            se["n_rejected"] += i
            break
    if k is None:
        k = k0
        se["n_rejected"] += M
        se["n_blocked"] += 1
    se["cur_start"] = k
    se["n_used"][k] += 1
    start_in, start_state = pool_in[k][s], pool_state[k][s]
    # 5. 6.
    epm.start_words(start_in, flag, c, trace, s, score)
    # 4.
    return start_in, start_state, 0, c


def step(em, sp, stats, sstats, pool_in, pool_state, p, q, flags, state, O, hw, world_first=None, trace=None, score=None):
    """The batch - a Jacobi step: every scene reads the records `p` the advance READ.  stats, sstats (and score, if given) are
    updated in place; trace, if given, is copied.  Returns (staged SceneIn, SceneState, flag words, trace or None, cause words)."""
    n = len(q)
    out, st, f = q.copy(), state.copy(), np.array(flags, np.int32).copy()
    tr = None if trace is None else trace.copy()
    causes = np.zeros(n, np.int32)
    world_of = None
    if world_first is not None:
        world_of = np.zeros(n, np.int64)
        for w in range(len(world_first) - 1):
            world_of[int(world_first[w]):int(world_first[w + 1])] = w
    for s in range(n):
        members = None if world_of is None else range(int(world_first[world_of[s]]), int(world_first[world_of[s] + 1]))
        with np.errstate(invalid="ignore", over="ignore"):
            rec, srec, f[s], causes[s] = step_scene(em, sp, s, stats[s], sstats[s], pool_in, pool_state, p, q[s], int(flags[s]), state[s], O, hw, members,
                                                    tr, None if score is None else score[s])
        out[s], st[s] = rec, srec
    return out, st, f, tr, causes
