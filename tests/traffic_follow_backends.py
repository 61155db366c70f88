"""Backends for the car-following known answers (tests/test_traffic_follow.py).

One call = some tracks, some SCENES - each an ego (x, y, velocity in km/h, flagged or not) and the actors of that scene as rows
(s0, speed, track, type, radius) - a TrafficFollow model, dt and a number of steps.  The result = s, v and the ObPoint of every
actor after the set calls (stage 0) and after every advance (stage k), and the model's branch record (`info`) of every step.  The
ego is staged at the same pose, with the same velocity, by every advance.

ModelBackend runs tests/traffic_follow_model.py on those ego values.  DeviceBackend gives every scene the obstacle entries its
actors need (pp_gen_scenes, slice mode), calls pp_set_traffic and pp_set_traffic_follow and then, per step, pp_plan_tick and
pp_advance_async with a PlanOut put in the place of the tick's that makes k_advance_egos stage the wanted pose (path point 0 one
step's distance behind it, point 1 on it; a flagged ego: a NaN path point, which is DMPP_EGO_BAD_PATH and freezes the resident
record).  The model is then fed what the device ITSELF staged - pp_get_scene_in, pp_get_ego_flags - and s, v and every actor's
ObPoint (pp_get_obstacles) are held against it byte for byte."""
import numpy as np

import traffic_follow_model as fm
import traffic_scenes as ts


class Result:
    def __init__(self, s, v, ob, info):
        self.s, self.v, self.ob, self.info = s, v, ob, info          # lists over stages; info[0] is None

    def at(self, stage, a):
        o = self.ob[stage][a]
        return float(self.s[stage][a]), float(self.v[stage][a]), float(o["x"]), float(o["y"])


def _layout(dm, scenes, order):
    """Actor records in launch order.  Flat actor f (scene by scene, row by row) owns slot = its row of its scene, whatever the
    launch order: `order[i]` = the flat actor that is actor i of the launch.  Returns (records, stride, order, inverse)."""
    flat = [(r[0], r[1], c, k, r[2], r[3], r[4]) for c, sc in enumerate(scenes) for k, r in enumerate(sc["actors"])]
    order = np.arange(len(flat)) if order is None else np.asarray(order)
    inv = np.empty(len(flat), np.int64)
    inv[order] = np.arange(len(flat))
    stride = max(max((len(sc["actors"]) for sc in scenes), default=1), 1)
    return ts.actors(dm, [flat[f] for f in order]), stride, order, inv


def _egos(dm, scenes):
    si, flags = np.zeros(len(scenes), dm.SceneIn), np.zeros(len(scenes), np.int32)
    for c, sc in enumerate(scenes):
        x, y, v, flagged = sc["ego"]
        si["loc"]["globalpoint"]["x"][c], si["loc"]["globalpoint"]["y"][c], si["loc"]["velocity"][c] = x, y, v
        flags[c] = dm.EGO_BAD_PATH if flagged else 0
    return si, flags


def _run_model(dm, polylines, act, stride, si_of_step, flags_of_step, tf, dt, steps):
    tracks, pts = ts.pack(dm, polylines)
    n_sc = int(act["scene"].max()) + 1 if len(act) else 0
    n_sc = max(n_sc, len(si_of_step(1)))
    tr = fm.Follow(tracks, pts, act, np.arange(n_sc) * stride)
    pool = ts.filled(dm.ObPoint, n_sc * stride)
    pool, _ = tr.place(pool, None, 0.0)
    s, v, ob, info = [tr.s.copy()], [tr.v.copy()], [pool[tr.pool_index].copy()], [None]
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    for k in range(1, steps + 1):
        pool, _ = tr.step(pool, None, dt, tf, si_of_step(k), flags_of_step(k), width)
        s.append(tr.s.copy()), v.append(tr.v.copy()), ob.append(pool[tr.pool_index].copy()), info.append(tr.info)
    return Result(s, v, ob, info)


def _unpermute(res, inv):
    return Result([x[inv] for x in res.s], [x[inv] for x in res.v], [x[inv] for x in res.ob], [None if i is None else [i[k] for k in inv] for i in res.info])


class ModelBackend:
    name = "model"

    def run(self, dm, polylines, scenes, tf, dt, steps, order=None):
        act, stride, order, inv = _layout(dm, scenes, order)
        si, flags = _egos(dm, scenes)
        return _unpermute(_run_model(dm, polylines, act, stride, lambda k: si, lambda k: flags, tf, dt, steps), inv)


def staging_plan(dm, egos, dt):
    """The PlanOut that makes k_advance_egos stage every ego (x, y, v, flagged) at its pose: vn = v + 0 (desaccVd with desacc = 0),
    dist = 0.5 (v + vn) / 3.6 dt, walked from point 0; a flagged ego: a NaN path point (DMPP_EGO_BAD_PATH)."""
    po = np.zeros(len(egos), dm.PlanOut)
    po["result"]["desaccVd"] = 1
    with np.errstate(all="ignore"):
        for c, (x, y, v, flagged) in enumerate(egos):
            d = np.float64(0.5) * (np.float64(v) + np.float64(v)) / np.float64(3.6) * np.float64(dt)
            d = d if d > 0 else np.float64(0.0)
            po["road_points"]["x"][c] = x + (np.arange(dm.PATH_POINTS) - 1.0) * d
            po["road_points"]["y"][c] = y
            if flagged:
                po["road_points"]["x"][c, 0] = np.nan
    return po


def staged_step(dm, pl, model, po, after_tick=None):
    """One step of the device loop: the tick an advance follows, `po` and a fresh SceneState in the place of what it wrote, the
    advance; returns the SceneIn records and the ego flag words the device staged."""
    pl.tick()
    if after_tick is not None:
        after_tick()
    st = pl.get_state()
    st["afresh_planning"] = 1                                   # (the ego stands on point 0 of the path)
    pl.write_device(dm.BUF_PLAN_OUT, po)
    pl.write_device(dm.BUF_STATE, st)
    pl.advance_async(model)
    return pl.get_scene_in(), pl.ego_flags()


def check_staged_egos(seen_si, seen_flags, want_si, want_flags, steps):
    """The egos came out as the case wants them (else its known answers mean nothing)."""
    for k in range(1, steps + 1):
        for f in ("x", "y"):
            assert seen_si[k]["loc"]["globalpoint"][f].tobytes() == want_si["loc"]["globalpoint"][f].tobytes(), f"step {k}: staged ego {f}"
        assert seen_si[k]["loc"]["velocity"].tobytes() == want_si["loc"]["velocity"].tobytes(), f"step {k}: staged ego velocity"
        assert np.array_equal(seen_flags[k] != 0, want_flags != 0), f"step {k}: ego flags {seen_flags[k].tolist()}"


class DeviceBackend:
    name = "device"

    def run(self, dm, polylines, scenes, tf, dt, steps, order=None):
        act, stride, order, inv = _layout(dm, scenes, order)
        tracks, pts = ts.pack(dm, polylines)
        n, na = len(scenes), len(act)
        want_si, want_flags = _egos(dm, scenes)
        cfg = dm.default_config(128)
        cfg["grid_stage"] = 0
        sc = dm.gen_scenes(cfg, 0, n, stride, junction_every=0)
        sc["obs_pool"] = ts.filled(dm.ObPoint, n * stride)
        sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"] = np.arange(n) * stride, stride
        sc["scene_in"]["loc"]["globalpoint"]["x"], sc["scene_in"]["loc"]["globalpoint"]["y"] = want_si["loc"]["globalpoint"]["x"], want_si["loc"]["globalpoint"]["y"]
        sc["scene_in"]["loc"]["velocity"] = want_si["loc"]["velocity"]
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * stride)
        pl.set_scenes(sc, with_motion=False)
        pl.set_state(sc["state"])
        pl.set_traffic(tracks, pts, act)
        pl.set_traffic_follow(fm_record(dm, tf))
        model = dm.default_ego_model()
        model["dt"], model["window"] = dt, 1                        # (a window of one point: the ids stay, no DMPP_EGO_LANE_END)
        po = staging_plan(dm, [sc["ego"] for sc in scenes], dt)
        seen_si, seen_flags = {}, {}
        s, v, ob = [], [], []
        for k in range(steps + 1):
            if k > 0:
                seen_si[k], seen_flags[k] = staged_step(dm, pl, model, po)
            s.append(pl.traffic_state()), v.append(pl.traffic_speed())
            got = np.zeros(na, dm.ObPoint)
            slices = [pl.get_obstacles(c, cap=stride) for c in range(n)]
            for a in range(na):
                got[a] = slices[int(act["scene"][a])][int(act["slot"][a])]
            ob.append(got)
        pl.close()
        check_staged_egos(seen_si, seen_flags, want_si, want_flags, steps)
        want = _run_model(dm, polylines, act, stride, lambda k: seen_si[k], lambda k: seen_flags[k], tf, dt, steps)
        for k in range(steps + 1):
            assert s[k].tobytes() == want.s[k].tobytes(), f"stage {k}: arc lengths differ from the model's at actors {np.flatnonzero(s[k] != want.s[k]).tolist()[:20]}"
            assert v[k].tobytes() == want.v[k].tobytes(), f"stage {k}: speeds differ from the model's at actors {np.flatnonzero(v[k] != want.v[k]).tolist()[:20]}"
            assert ob[k].tobytes() == want.ob[k].tobytes(), f"stage {k}: pool entries differ from the model's at actors {np.flatnonzero(ob[k] != want.ob[k]).tolist()[:20]}"
        return _unpermute(Result(s, v, ob, want.info), inv)


def fm_record(dm, tf):
    rec = np.zeros(1, dm.TrafficFollow)
    for k, val in fm.params(tf).items():
        rec[k] = val
    return rec


class Runner:
    """run(polylines, scenes, tf=None, dt=0.5, steps=2, order=None); logs every call for the batched replay."""

    def __init__(self, dm, backend, log=None):
        self.dm, self.backend, self.name, self.log = dm, backend, backend.name, log

    def __call__(self, polylines, scenes, tf=None, dt=0.5, steps=2, order=None):
        tf = fm.params(tf)
        res = self.backend.run(self.dm, polylines, scenes, tf, dt, steps, order)
        if self.log is not None and order is None:
            self.log.append(dict(polylines=polylines, scenes=scenes, tf=tf, dt=dt, steps=steps, res=res))
        return res


def batched(dm, backend, log, repeat_to=None):
    """Every logged call as scenes of ONE launch per (model, dt, steps) - a launch has one model -: tracks and scenes
    concatenated, track indices moved.  Every actor must give the bytes it gave alone.  repeat_to: the scenes of a launch are
    repeated cyclically until it has at least that many actors.  Returns the number of actors of the largest launch."""
    keys, largest = {}, 0
    for c in log:
        keys.setdefault((tuple(sorted((k, float(x)) for k, x in c["tf"].items())), c["dt"], c["steps"]), []).append(c)
    for calls in keys.values():
        polylines, scenes, alone = [], [], []
        for c in calls:
            base, a = len(polylines), 0
            polylines += c["polylines"]
            for sc in c["scenes"]:
                scenes.append(dict(ego=sc["ego"], actors=[(r[0], r[1], r[2] + base, r[3], r[4]) for r in sc["actors"]]))
                alone.append([(c["res"], a + k) for k in range(len(sc["actors"]))])
                a += len(sc["actors"])
        n0, count = len(scenes), sum(len(x) for x in alone)
        while repeat_to is not None and count < repeat_to:
            k = len(scenes) % n0
            scenes.append(scenes[k]), alone.append(alone[k])
            count += len(alone[k])
        res = backend.run(dm, polylines, scenes, calls[0]["tf"], calls[0]["dt"], calls[0]["steps"])
        flat = [x for sc in alone for x in sc]
        for k, (r, a) in enumerate(flat):
            for stage in range(calls[0]["steps"] + 1):
                assert res.s[stage][k].tobytes() == r.s[stage][a].tobytes(), f"actor {k}, stage {stage}: s"
                assert res.v[stage][k].tobytes() == r.v[stage][a].tobytes(), f"actor {k}, stage {stage}: v"
                assert res.ob[stage][k].tobytes() == r.ob[stage][a].tobytes(), f"actor {k}, stage {stage}: ObPoint"
        largest = max(largest, len(flat))
    return largest
