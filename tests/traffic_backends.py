"""Backends for the lane-traffic known answers (tests/test_traffic.py): one call = some tracks, some actors and a list of steps;
the result = the arc length and the ObPoint of every actor after pp_set_traffic and after every step.

ModelBackend runs tests/traffic_model.py.  DeviceBackend gives every actor a scene of its own with one obstacle entry
(pp_gen_scenes, slice mode), calls pp_set_traffic and then (pp_plan_tick, pp_advance_async with EgoModel.dt = the step) per step,
reading pp_get_traffic_state and every actor's pp_get_obstacles each time - and holds all of it against the model byte for byte."""
import numpy as np

import traffic_model as tm
import traffic_scenes as ts


class Result:
    def __init__(self, s, ob):
        self.s, self.ob = s, ob          # lists over stages (0: after the set call): float64 (n,), ObPoint (n,)

    def at(self, stage, a):
        o = self.ob[stage][a]
        return float(self.s[stage][a]), float(o["x"]), float(o["y"])


class ModelBackend:
    name = "model"

    def run(self, dm, polylines, rows, steps):
        tracks, pts = ts.pack(dm, polylines)
        n = len(rows)
        act = ts.actors(dm, [(r[0], r[1], a, 0, r[2], r[3], r[4]) for a, r in enumerate(rows)])
        tr = tm.Traffic(tracks, pts, act, np.arange(n))
        pool = ts.filled(dm.ObPoint, n)
        s, ob = [], []
        for step in [0.0] + list(steps):
            pool, _ = tr.place(pool, None, step)
            s.append(tr.s.copy()), ob.append(pool.copy())
        return Result(s, ob)


class DeviceBackend:
    name = "device"

    def run(self, dm, polylines, rows, steps):
        want = ModelBackend().run(dm, polylines, rows, steps)
        tracks, pts = ts.pack(dm, polylines)
        n = len(rows)
        act = ts.actors(dm, [(r[0], r[1], a, 0, r[2], r[3], r[4]) for a, r in enumerate(rows)])
        cfg = dm.default_config(128)
        cfg["grid_stage"] = 0
        sc = dm.gen_scenes(cfg, 0, n, 1, junction_every=0)
        sc["obs_pool"] = ts.filled(dm.ObPoint, n)
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n)
        pl.set_scenes(sc, with_motion=False)
        pl.set_state(sc["state"])
        pl.set_traffic(tracks, pts, act)
        s, ob = [], []
        for k, step in enumerate([0.0] + list(steps)):
            if k > 0:
                model = dm.default_ego_model()
                model["dt"] = step
                pl.tick()
                pl.advance_async(model)
            s.append(pl.traffic_state())
            got = np.zeros(n, dm.ObPoint)
            for a in range(n):
                sl = pl.get_obstacles(a)
                assert len(sl) == 1
                got[a] = sl[0]
            ob.append(got)
            assert s[-1].tobytes() == want.s[k].tobytes(), f"stage {k}: arc lengths {s[-1].tolist()} against the model's {want.s[k].tolist()}"
            assert got.tobytes() == want.ob[k].tobytes(), f"stage {k}: pool entries differ from the model's at actors {np.flatnonzero(got != want.ob[k]).tolist()}"
        pl.close()
        return Result(s, ob)


class Runner:
    """run(polylines, rows, steps): rows are (s0, speed, track, type, radius); logs every call for the batched replay."""

    def __init__(self, dm, backend, log=None):
        self.dm, self.backend, self.name, self.log = dm, backend, backend.name, log

    def __call__(self, polylines, rows, steps):
        res = self.backend.run(self.dm, polylines, rows, steps)
        if self.log is not None:
            self.log.append(dict(polylines=polylines, rows=rows, steps=list(steps), res=res))
        return res


def batched(dm, backend, log, repeat_to=None):
    """Every logged call as actors of ONE launch (the calls must share their steps): tracks and actors concatenated, track
    indices moved.  Every actor must give the bytes it gave alone.  repeat_to: the actors are repeated cyclically up to that
    count (identical actors on distinct scenes).  Returns the number of actors."""
    steps = log[0]["steps"]
    assert all(c["steps"] == steps for c in log)
    polylines, rows, alone = [], [], []
    for c in log:
        base = len(polylines)
        polylines += c["polylines"]
        for a, r in enumerate(c["rows"]):
            rows.append((r[0], r[1], r[2] + base, r[3], r[4]))
            alone.append((c["res"], a))
    n0 = len(rows)
    if repeat_to is not None:
        rows = [rows[k % n0] for k in range(repeat_to)]
        alone = [alone[k % n0] for k in range(repeat_to)]
    res = backend.run(dm, polylines, rows, steps)
    for k, (r, a) in enumerate(alone):
        for stage in range(len(steps) + 1):
            assert res.s[stage][k].tobytes() == r.s[stage][a].tobytes(), f"actor {k}, stage {stage}: s"
            assert res.ob[stage][k].tobytes() == r.ob[stage][a].tobytes(), f"actor {k}, stage {stage}: ObPoint"
    return len(rows)
