"""Episodic rollouts in plain Python / numpy, written from DESIGN.md §4k (not from the kernel).

`step` is what the episode step of one pp_advance_async does behind the advance kernel: the SceneIn records the advance read
(`p`), the ones it staged (`q`), the flag words it left, the SceneState array, the start records and the stats in; the staged
records, the state, the flag words and - if asked for - the trace records and the scorecard records out.  Python floats are
IEEE doubles and every expression is evaluated left to right as the specification writes it, so the records are meant to equal
the device's byte for byte."""
import math

import numpy as np

PATH_END, BAD_PATH, LANE_END, OFF_GRID, ROUTE_END = 1, 2, 4, 8, 16
RESPAWNED, TIMEOUT, CONTACT = 32, 64, 128
ALL_FLAGS = 31
LANESUM = 8


def new_stats(dtype, n):
    """§4k 0.: the starting values."""
    r = np.zeros(n, dtype)
    r["min_age"], r["max_age"] = -1, -1
    return r


def cause(flag, age, end_mask, max_ticks):
    """§4k 2.: the cause word of a scene whose running episode has `age` advances and whose advance left `flag`."""
    return (int(flag) & int(end_mask)) | (TIMEOUT if int(max_ticks) > 0 and int(age) >= int(max_ticks) else 0)


def trace_record(dtype, rec, flags):
    """The EgoTrace record §4c defines for one SceneIn record: pose, speed, the id of slot clamp(lane_num - 1, 0, 7), lane, flags."""
    t = np.zeros(1, dtype)[0]
    loc = rec["loc"]
    t["pose"], t["velocity"], t["lane_num"], t["flags"] = loc["globalpoint"], loc["velocity"], loc["lane_num"], flags
    t["id_cur"] = loc["id"][min(max(int(loc["lane_num"]) - 1, 0), LANESUM - 1)]
    return t


def age_dist(e, p, q):
    """§4k 1.: age and distance of the running episode of stats record e; p the record the advance read, q the one it staged."""
    ex = float(q["loc"]["globalpoint"]["x"]) - float(p["loc"]["globalpoint"]["x"])
    ey = float(q["loc"]["globalpoint"]["y"]) - float(p["loc"]["globalpoint"]["y"])
    return int(e["age"]) + 1, float(e["dist"]) + math.sqrt(ex * ex + ey * ey)


def go_on(e, age, dist):
    """§4k 2., cause word 0: the episode goes on."""
    e["age"], e["dist"] = age, dist


def close(e, c, age, dist):
    """§4k 3.: the running episode is closed in the stats record e with cause word c."""
    e["n_episodes"] += 1
    for b in range(5):
        if c & (1 << b):
            e["n_end"][b] += 1
    if c & TIMEOUT:
        e["n_end"][5] += 1
    e["last_cause"], e["last_age"] = c, age
    if int(e["min_age"]) < 0 or age < int(e["min_age"]):
        e["min_age"] = age
    if int(e["max_age"]) < 0 or age > int(e["max_age"]):
        e["max_age"] = age
    e["ticks_total"] += age
    e["last_dist"] = dist
    e["dist_total"] = float(e["dist_total"]) + dist
    e["age"], e["dist"] = 0, 0.0


def start_words(start_in, flag, c, trace=None, k=0, score=None):
    """§4k 5. - 6.: the trace record (record k of `trace`) and the scorecard words of a restart onto start_in.  CONTACT is §4l's cause
    bit: §4k's cause word never holds it (end_mask lies inside 31)."""
    if trace is not None:
        trace[k] = trace_record(trace.dtype, start_in, int(flag) | RESPAWNED | (c & (TIMEOUT | CONTACT)))
    if score is not None:
        score["last_pos"]["x"], score["last_pos"]["y"] = start_in["loc"]["globalpoint"]["x"], start_in["loc"]["globalpoint"]["y"]
        score["last_speed"] = start_in["loc"]["velocity"]


def step_scene(em, e, start_in, start_state, p, q, flag, state, trace=None, k=0, score=None):
    """One scene, one advance.  e: its EpisodeStats record, score: its RolloutScore record or None (numpy voids that write
    through); trace: the EgoTrace array of the advance or None, k the scene's index in it.  Returns (staged SceneIn record,
    SceneState record, flag word, cause word)."""
    # 1. 2.
    age, dist = age_dist(e, p, q)
    c = cause(flag, age, int(em["end_mask"][0]), int(em["max_ticks"][0]))
    if c == 0:
        go_on(e, age, dist)
        return q, state, int(flag), 0
    # 3. 5. 6.
    close(e, c, age, dist)
    start_words(start_in, flag, c, trace, k, score)
    # 4.
    return start_in, start_state, 0, c


def step(em, stats, start_in, start_state, p, q, flags, state, trace=None, score=None):
    """The batch.  stats (and score, if given) are updated in place; trace, if given, is the EgoTrace array of the advance and is
    copied.  Returns (staged SceneIn, SceneState, flag words, trace or None, cause words)."""
    n = len(q)
    out, st, f = q.copy(), state.copy(), np.array(flags, np.int32).copy()
    tr = None if trace is None else trace.copy()
    causes = np.zeros(n, np.int32)
    for k in range(n):
        with np.errstate(invalid="ignore", over="ignore"):
            rec, srec, f[k], causes[k] = step_scene(em, stats[k], start_in[k], start_state[k], p[k], q[k], int(flags[k]), state[k],
                                                    tr, k, None if score is None else score[k])
        out[k], st[k] = rec, srec
    return out, st, f, tr, causes
