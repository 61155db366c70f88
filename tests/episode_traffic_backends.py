"""Two backends for the episode traffic reset (pp_set_episode_traffic), in the spirit of episode_spawn_backends.py,
on which this builds: the numpy model (tests/episode_traffic_model.py behind the ego, route, episode, spawn and traffic models)
and the HIP kernel k_reset_traffic behind k_respawn_egos / k_respawn_spawn and k_move_traffic / k_follow_traffic.

A known answer is written once against `Runner` and asserted on both.  One call takes a Case: what episode_spawn_backends.Case
takes - the egos, their obstacle slices, the steps with the PlanOut and SceneState each advance reads, the episode model, the spawn
model or None - and the traffic: polylines, actor rows (s0, speed, scene, slot, track, type, radius; the slot must lie inside the
scene's slice `obs`), the TrafficFollow record or None, whether the input sets carry a motion pool, n_sets (0: pp_set_episode_traffic
is not called) and the TrafficStart records of sets 1 .. n_sets - 1.  It returns one Result per step: what
episode_spawn_backends.Result holds and, behind the advance, the arc lengths, the speeds (None with following off), the whole
obstacle pool as the scenes' slices give it, the reset counters (None without the call) and the motion pool (None without one).
On the device the slices are read through pp_get_obstacles from the staged set and the motion pool from the current set once the
next tick has adopted it."""
import numpy as np

import advance_harness as ah
import dmpp_amd as dm
import episode_spawn_backends as esb
import episode_spawn_model as esm
import episode_traffic_model as etm
import traffic_follow_model as fm
import traffic_model as tm
import traffic_scenes as ts

MOT_FILL = (500.0, -500.0)          # the ObMotion of every entry before traffic is set: a traffic entry must lose it


class Case(esb.Case):
    def __init__(self, cfg, model, em, sp, si, obs, state0, steps, world, route, starts, polylines, rows, n_sets=1, tstarts=None, follow=None, motion=False):
        esb.Case.__init__(self, cfg, model, em, sp, si, obs, state0, steps, world, route, starts)
        self.polylines, self.rows, self.n_sets, self.tstarts, self.follow, self.motion = polylines, rows, n_sets, tstarts, follow, motion
        for r in rows:
            assert 0 <= r[3] < len(obs[r[2]]), "an actor's slot is an own entry of its scene"

    def traffic(self):
        tracks, pts = ts.pack(dm, self.polylines)
        return tracks, pts, ts.actors(dm, self.rows)

    def without_reset(self):
        return Case(self.cfg, self.model, self.em, self.sp, self.si, self.obs, self.state0, self.steps, self.world, self.route, self.starts,
                    self.polylines, self.rows, 0, None, self.follow, self.motion)


class Result(esb.Result):
    def __init__(self, base, s, v, pool, resets, mot=None):
        esb.Result.__init__(self, base.out, base.flags, base.trace, base.state, base.stats, base.sstats)
        self.s, self.v, self.pool, self.resets, self.mot = s, v, pool, resets, mot


def _mot0(case, pool):
    if not case.motion:
        return None
    mot = np.zeros(len(pool), dm.ObMotion)
    mot["vx"], mot["vy"] = MOT_FILL
    return mot


class ModelBackend:
    name = "model"

    def run(self, case):
        n = case.n
        si, pool, pin, pst, stats, sstats = case.start()
        tracks, pts, act = case.traffic()
        tr = (fm.Follow if case.follow is not None else tm.Traffic)(tracks, pts, act, si["obs_off"])
        pool, mot = tr.place(pool, _mot0(case, pool), 0.0)                    # pp_set_traffic
        reset = etm.Reset(tr, case.n_sets, case.tstarts, case.follow is not None) if case.n_sets else None
        flags, res = np.zeros(n, np.int32), []
        dt = float(case.model["dt"][0])
        for po, st in case.steps:
            r = esb.model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags)          # (contact and clearance read the pool the advance READ)
            if case.follow is not None:
                pool, mot = tr.step(pool, mot, dt, case.follow, r.out, r.flags, float(case.cfg["Vehicle_Width"][0]))
            else:
                pool, mot = tr.place(pool, mot, dt)
            if reset is not None:
                pool, mot = reset.step(tr, pool, mot, r.stats["age"], r.sstats["cur_start"])
            res.append(Result(r, tr.s.copy(), tr.v.copy() if case.follow is not None else None, pool.copy(), None if reset is None else reset.n_resets.copy(), mot))
            si, flags = r.out, r.flags
        return res


class DeviceBackend:
    name = "device"

    def run(self, case):
        def then(pl):
            pl.set_traffic(*case.traffic())
            if case.follow is not None:
                pl.set_traffic_follow(case.follow)
            pl.set_episodes(case.em)
            if case.sp is not None:
                esb.set_spawn(pl, case)
            if case.n_sets:
                pl.set_episode_traffic(case.n_sets, case.tstarts)

        def adopted(pl):                                  # the set the last advance staged is the current one now
            if case.motion and res:
                res[-1].mot = pl.read_device(dm.BUF_MOT_POOL, dm.ObMotion, len(pool))
                assert pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, len(pool)).tobytes() == res[-1].pool.tobytes(), "the slices are the pool"
        n = case.n
        pl, si, pool, W = esb.open_case(case, then, _mot0(case, case.laid_out()[1]))
        trace, res = dm.pinned_empty(n, dm.EgoTrace), []
        for po, st in case.steps:
            ah.inject_advance(pl, case.model, po, st, trace, after_tick=adopted)
            out, f, stats = pl.get_scene_in(), pl.ego_flags(), pl.episode_stats()
            sstats = pl.episode_spawn_stats() if case.sp is not None else esm.new_stats(dm.EpisodeSpawnStats, n)
            base = esb.Result(out, f, np.array(trace), pl.get_state(), stats, sstats)
            got = pool.copy()
            for s in range(n):
                sl = pl.get_obstacles(s)
                assert len(sl) == int(si["obs_n"][s])
                got[s * W:s * W + len(sl)] = sl
            res.append(Result(base, pl.traffic_state(), pl.traffic_speed() if case.follow is not None else None, got,
                              pl.episode_traffic_resets() if case.n_sets else None))
        if case.motion:
            pl.tick()
            res[-1].mot = pl.read_device(dm.BUF_MOT_POOL, dm.ObMotion, len(pool))
        pl.close()
        return res


def compare(got, want, what):
    """episode_spawn_backends.compare - the ego's records, flags, trace, state and both stats - and, byte for byte, the arc lengths,
    the speeds, the obstacle pool, the reset counters and the motion pool."""
    esb.compare(got, want, what)
    for name in ("s", "v", "pool", "resets", "mot"):
        g, w = getattr(got, name), getattr(want, name)
        assert (g is None) == (w is None), f"{what}: {name}"
        if g is not None:
            assert g.tobytes() == w.tobytes(), f"{what}: {name} differs at {np.flatnonzero(g != w).tolist()[:8]}: {g[g != w][:4].tolist()} against {w[g != w][:4].tolist()}"


class Runner:
    """What a known answer calls.  The device is held against the model on the same case, every step, and every call is logged
    for batched()."""
    def __init__(self, backend, log=None):
        self.backend, self.name, self.log = backend, backend.name, log

    def __call__(self, case):
        res = self.backend.run(case)
        if self.name == "device":
            for k, (r, w) in enumerate(zip(res, ModelBackend().run(case))):
                compare(r, w, f"step {k}")
        if self.log is not None:
            assert case.n == 1
            self.log.append(ah.Call(case, res))
        return res


def _same_launch(a, b):
    same = lambda x, y: (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes())
    return (esb._same_launch(a, b) and a.n_sets == b.n_sets and same(a.follow, b.follow) and a.motion == b.motion)


def _restarts(res):
    return any(int(r.stats["age"][0]) == 0 for r in res)


def batch_of(cases):
    """Single-scene cases that can share a launch as the scenes of one case: scenes, slices, start records, tracks, actors and
    start states concatenated, track and scene indices moved."""
    c0 = cases[0]
    si, obs, state0, steps, route, starts = esb.joined(cases)
    polylines, rows, first = [], [], []
    for k, c in enumerate(cases):
        first.append(len(rows))
        rows += [(r[0], r[1], k, r[3], r[4] + len(polylines), r[5], r[6]) for r in c.rows]
        polylines += c.polylines
    tstarts = None
    if c0.n_sets > 1:
        tstarts = np.concatenate([np.asarray(c.tstarts).reshape(c0.n_sets - 1, len(c.rows))[k] for k in range(c0.n_sets - 1) for c in cases])
    big = Case(c0.cfg, c0.model, c0.em, c0.sp, si, obs, state0, steps, c0.world, route, starts, polylines, rows, c0.n_sets, tstarts, c0.follow, c0.motion)
    return big, first + [len(rows)], len(cases)


def batched(log, sizes=(5, 9), backend=None):
    """Every logged single-scene call again, as distinct scenes of one launch (episode_spawn_backends.batched): the calls that can
    share a launch form a group, each group runs in batches of every size of `sizes` with a scene that RESTARTS first, last and on
    either side of the respawn kernels' block edge 4 | 5 where the group has both kinds.  The device is held against the model on
    the same batch, and that against the bytes the model gave for every scene alone (`log` is a model runner's) - the start choice
    of the cases logged here is round robin or M = 1, so it does not depend on the scene index.  Returns (size, indices of the
    restarting scenes) per batch."""
    assert all(c.case.sp is None or c.case.M == 1 or int(c.case.sp["order"][0]) == 1 for c in log)
    ran = []
    for n, batch, at in ah.batches(log, _same_launch, _restarts, sizes):
        big, first, _ = batch_of([c.case for c in batch])
        got, want = (backend or DeviceBackend()).run(big), ModelBackend().run(big)
        W = big.laid_out()[2]
        for t, (r, w) in enumerate(zip(got, want)):
            compare(r, w, f"batch of {n}, step {t}")
            ah.same_alone(w, t, batch, ("out",), obs_width=W)          # (the log is the MODEL's: an advanced heading is the host's atan on both sides)
            for k, c in enumerate(batch):
                alone, what, own = c.res[t], f"batch of {n}, scene {k}, step {t}", len(c.case.obs[0])
                assert w.stats[k].tobytes() == alone.stats[0].tobytes() and w.sstats[k].tobytes() == alone.sstats[0].tobytes(), what + ": stats"
                acts = slice(first[k], first[k + 1])
                assert w.s[acts].tobytes() == alone.s.tobytes(), what + ": s"
                assert w.pool[k * W:k * W + own].tobytes() == alone.pool[:own].tobytes(), what + ": slice"
                if alone.v is not None:
                    assert w.v[acts].tobytes() == alone.v.tobytes(), what + ": v"
                if alone.resets is not None:
                    assert w.resets[acts].tobytes() == alone.resets.tobytes(), what + ": n_resets"
        ran.append((n, at))
    return ran
