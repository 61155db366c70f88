"""World episodes and the world traffic reset in plain Python / numpy, written from DESIGN.md §4s and §4t (not from the kernels):
the WORLD is the unit of an episode - when any ego of a world ends, every ego of that world restarts on the same advance and on the
same start-record index, and the world's vehicles go back to that index's start states.

`step` is what the episode step of one pp_advance_async does while pp_set_episode_worlds is in force.  It takes what
episode_spawn_model.step takes and `own`: with a fleet the pinned slices (pin_off, n_own) of every scene - the OWN entries the
clearance walk tests -, None without one (the slice of the record the advance read).  The steps that are §4k's and §4l's are called
from tests/episode_model.py and tests/episode_spawn_model.py; what is written here is the verdict, the world's cause word, the one
draw per world and the walk over every member's own entries.

`WorldReset` is tests/episode_traffic_model.py's Reset for the vehicles of tests/world_traffic_model.py's World: a vehicle resets
when the FIRST scene of its world has age 0, onto the set that scene's cur_start names."""
import numpy as np

import episode_model as epm
import episode_spawn_model as esm
import episode_traffic_model as etm
import traffic_model as tm

WORLD = 256
CONTACT = epm.CONTACT


def worlds_of(n, world_first=None):
    """The member runs [a, b) of every world: the fleet's, or one scene each."""
    if world_first is None:
        return [(s, s + 1) for s in range(n)]
    wf = [int(x) for x in world_first]
    assert wf[0] == 0 and wf[-1] == n
    return list(zip(wf[:-1], wf[1:]))


def own_cause(em, sp, e, p, m, q, flag, O, hw):
    """§4s 1. = §4l 1., 1a., 2. of member m: (age, dist, c_m), all from what stood before the step."""
    pm = p[m]
    px, py = float(pm["loc"]["globalpoint"]["x"]), float(pm["loc"]["globalpoint"]["y"])
    age, dist = epm.age_dist(e, pm, q)
    off, n = _inside(int(pm["obs_off"]), int(pm["obs_n"]), len(O))
    touch = int(sp["contact"][0]) != 0 and esm.slice_within(O, off, n, px, py, hw, 0.0)
    return age, dist, epm.cause(flag, age, int(em["end_mask"][0]), int(em["max_ticks"][0])) | (CONTACT if touch else 0)


def _inside(off, n, n_pool):
    """A slice that does not lie inside the pool is empty."""
    return (0, 0) if n <= 0 or off < 0 or off + n > n_pool else (off, n)


def world_cause(c, m, members):
    """§4s 3.: C_m = c_m | WORLD iff some OTHER member has a cause of its own."""
    return int(c[m]) | (WORLD if any(int(c[t]) != 0 for t in members if t != m) else 0)


def own_entries(p, own, m, n_pool):
    if own is None:
        return _inside(int(p[m]["obs_off"]), int(p[m]["obs_n"]), n_pool)
    return _inside(int(own[0][m]), int(own[1][m]), n_pool)


def blocked(sp, pool_in, cand, members, p, own, O, hw):
    """§4s 4.: candidate `cand` is blocked iff check bit 0 is set and SOME member has an own entry within the clearance of ITS record."""
    if not int(sp["check"][0]) & 1:
        return False
    clearance = float(sp["clearance"][0])
    for m in members:
        X, Y = float(pool_in[cand][m]["loc"]["globalpoint"]["x"]), float(pool_in[cand][m]["loc"]["globalpoint"]["y"])
        off, n = own_entries(p, own, m, len(O))
        if esm.slice_within(O, off, n, X, Y, hw, clearance):
            return True
    return False


def draw(sp, a, e, pool_in, members, p, own, O, hw):
    """§4s 4.: (k, rejected, blocked) of the world whose first scene is a, for its e-th ended episode."""
    M = int(sp["n_starts"][0])
    k0 = esm.first_choice(int(sp["seed"][0]), a, e, M, int(sp["order"][0]))
    for i in range(M):
        cand = (k0 + i) % M
        if not blocked(sp, pool_in, cand, members, p, own, O, hw):
            return cand, i, 0
    return k0, M, 1


def step(em, sp, stats, sstats, pool_in, pool_state, p, q, flags, state, O, hw, world_first=None, own=None, trace=None, score=None):
    """The batch.  stats, sstats (and score) are updated in place; trace is copied.  Returns (staged SceneIn, SceneState, flag words,
    trace or None, cause words C_m)."""
    n = len(q)
    out, st, f = q.copy(), state.copy(), np.array(flags, np.int32).copy()
    tr = None if trace is None else trace.copy()
    causes = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in worlds_of(n, world_first):
            members = range(a, b)
            # 1. own causes (Jacobi: everything from before the step)
            age, dist, c = {}, {}, {}
            for m in members:
                age[m], dist[m], c[m] = own_cause(em, sp, stats[m], p, m, q[m], int(flags[m]), O, hw)
            # 2. verdict
            if not any(c[m] for m in members):
                for m in members:
                    epm.go_on(stats[m], age[m], dist[m])
                continue
            # 3. close
            for m in members:
                causes[m] = world_cause(c, m, members)
                epm.close(stats[m], int(causes[m]), age[m], dist[m])
                if c[m] & CONTACT:
                    sstats[m]["n_contact"] += 1
            # 3a. one draw per world
            k, rejected, blk = draw(sp, a, int(stats[a]["n_episodes"]), pool_in, members, p, own, O, hw)
            for m in members:
                S = sstats[m]
                S["n_rejected"] += rejected
                S["n_blocked"] += blk
                S["cur_start"] = k
                S["n_used"][k] += 1
                # 4. - 6.
                epm.start_words(pool_in[k][m], int(flags[m]), c[m], tr, m, None if score is None else score[m])
                out[m], st[m], f[m] = pool_in[k][m], pool_state[k][m], 0
    return out, st, f, tr, causes


class WorldReset(etm.Reset):
    """§4t: etm.Reset on a world_traffic_model.World (or any traffic whose `scene` is a world and whose `entries` are per member)."""

    def step(self, tr, obs_pool, mot_pool, age, cur_start, world_first):
        obs = obs_pool.copy()
        mot = None if mot_pool is None else mot_pool.copy()
        for a, A in enumerate(tr.actors):
            a0 = int(world_first[int(A["scene"])])
            if int(age[a0]) != 0:                                # 1. the world goes on
                continue
            k = 0 if self.n_sets == 1 else int(cur_start[a0])    # 2.
            t = int(A["track"])
            s1 = tm.wrap(self.s[k][a], tr.cum[t][-1], int(tr.tracks["closed"][t]) != 0)          # 3.
            tr.s[a] = s1                                         # 4.
            if self.follow:
                speed = np.float64(A["speed"])
                tr.v[a] = self.v[k][a] if speed > 0 else speed
            tr._write(obs, mot, a, s1)
            self.n_resets[a] += 1
        return obs, mot
