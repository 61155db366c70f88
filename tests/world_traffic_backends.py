"""Backends for the world-traffic known answers (tests/test_world_traffic.py).

One call = some tracks, some WORLDS - each a list of member egos (x, y, velocity in km/h, flagged or not), the world's vehicles as
rows (s0, speed, track, type, radius; row k owns slot k of every member) and optionally `own` (own obstacle entries per member,
default: one per vehicle) and `pad` (unpinned entries behind a member's slice, default none) - a TrafficFollow model, dt, a number of
steps, following on or off, a motion pool or not, and K peer slots per scene.  Scene m's slice starts at the sum of
own + K + pad of the scenes before it.  The result = s, v, every scene's obstacle slice (own entries, then the peers k_couple_fleet
wrote) and the WHOLE obstacle and motion pools after the set calls (stage 0) and after every advance (stage k), and the model's
branch record of every step.  Every ego is staged at the same pose, with the same velocity, by every advance.

ModelBackend runs tests/world_traffic_model.py, then tests/fleet_model.py's couple, on those ego values.  DeviceBackend uploads the
scenes (pp_set_scenes, slice mode, pools filled with 0xA5), calls pp_set_fleet, pp_set_world_traffic and pp_set_traffic_follow and
then, per step, pp_plan_tick and pp_advance_async with a PlanOut put in the place of the tick's that makes k_advance_egos stage the
wanted pose (tests/traffic_follow_backends.py).  The model is then fed what the device ITSELF staged - pp_get_scene_in,
pp_get_ego_flags - and s, v, the full slice of every scene (pp_get_obstacles) and, once the next tick has adopted the set, every
byte of both pools are held against it: the 0xA5 fill must survive in every entry that is not pinned."""
import numpy as np

import fleet_model as fl
import traffic_follow_backends as fb
import traffic_follow_model as fm
import traffic_scenes as ts
import world_traffic_model as wm

RANGE = 60.0           # the fleet's range (it matters only with K > 0)
PEER_RADIUS = 0.9


class Result:
    def __init__(self, s, v, slices, pool, mot, info, layout):
        self.s, self.v, self.slices, self.pool, self.mot, self.info, self.layout = s, v, slices, pool, mot, info, layout

    def at(self, stage, a):
        """(s, v, x, y) of vehicle a, the pose read from its entry in the FIRST member scene of its world."""
        o = self.pool[stage][self.layout.entries[a][0]]
        return float(self.s[stage][a]), float(self.v[stage][a]), float(o["x"]), float(o["y"])

    def entry(self, stage, a, member):
        return self.pool[stage][self.layout.entries[a][member]]


class Layout:
    def __init__(self, dm, worlds, K):
        self.K = K
        self.world_first = np.concatenate([[0], np.cumsum([len(w["egos"]) for w in worlds])]).astype(np.int32)
        own, pad, rows, egos = [], [], [], []
        for w, W in enumerate(worlds):
            m = len(W["egos"])
            own += list(W.get("own") or [max(len(W["actors"]), 1)] * m)
            pad += list(W.get("pad") or [0] * m)
            egos += list(W["egos"])
            rows += [(r[0], r[1], w, k, r[2], r[3], r[4]) for k, r in enumerate(W["actors"])]
        self.n = len(egos)
        self.own, self.pad = np.array(own, np.int64), np.array(pad, np.int64)
        block = self.own + K + self.pad
        self.off = np.concatenate([[0], np.cumsum(block)[:-1]]).astype(np.int64)
        self.total = int(block.sum())
        self.act = ts.actors(dm, rows)
        self.si, self.flags = fb._egos(dm, [dict(ego=e) for e in egos])
        self.egos = egos
        self.fm = np.zeros(1, dm.FleetModel)
        self.fm["range"], self.fm["radius"], self.fm["max_peers"] = RANGE, PEER_RADIUS, K
        self.entries = [self.off[self.world_first[int(A["scene"])]:self.world_first[int(A["scene"]) + 1]] + int(A["slot"]) for A in self.act]

    def filled(self, dtype):
        return ts.filled(dtype, max(self.total, 1))

    def scene_in(self, si):
        """The loc fields of `si` on records whose slices are the layout's (what the model's couple starts from)."""
        out = si.copy()
        out["obs_off"], out["obs_n"] = self.off, self.own
        return out


def _slices(lay, si, pool):
    return [pool[int(si["obs_off"][c]):int(si["obs_off"][c]) + int(si["obs_n"][c])].copy() for c in range(lay.n)]


def _run_model(dm, polylines, lay, si_of_step, flags_of_step, tf, dt, steps, follow, motion):
    tracks, pts = ts.pack(dm, polylines)
    tr = wm.World(tracks, pts, lay.act, lay.world_first, lay.off, lay.own)
    pool, mot = lay.filled(dm.ObPoint), lay.filled(dm.ObMotion) if motion else None
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    si0 = lay.scene_in(si_of_step(0))
    si, pool, mot = fl.couple(lay.fm, lay.world_first, lay.off, lay.own, si0, pool, mot)          # pp_set_fleet, then pp_set_world_traffic
    pool, mot = tr.place(pool, mot, 0.0)
    s, v, sl, pl, mo, info = [tr.s.copy()], [tr.v.copy()], [_slices(lay, si, pool)], [pool], [mot], [None]
    for k in range(1, steps + 1):
        if follow:
            pool, mot = tr.step(pool, mot, dt, tf, si_of_step(k), flags_of_step(k), width)
        else:
            pool, mot = tr.place(pool, mot, dt)
        si, pool, mot = fl.couple(lay.fm, lay.world_first, lay.off, lay.own, lay.scene_in(si_of_step(k)), pool, mot)
        s.append(tr.s.copy()), v.append(tr.v.copy()), sl.append(_slices(lay, si, pool)), pl.append(pool), mo.append(mot), info.append(tr.info if follow else None)
    return Result(s, v, sl, pl, mo, info, lay)


class ModelBackend:
    name = "model"

    def run(self, dm, polylines, worlds, tf, dt, steps, follow=True, motion=False, K=0):
        lay = Layout(dm, worlds, K)
        return _run_model(dm, polylines, lay, lambda k: lay.si, lambda k: lay.flags, tf, dt, steps, follow, motion)


def set_scenes(pl, sc, si, obs, mot, n_obs_total):
    rc = pl.lib.pp_set_scenes(pl.h, len(si), si.ctypes.data, sc["lane_pool"].ctypes.data, sc["attr_pool"].ctypes.data, len(sc["lane_pool"]),
                              sc["ref_pool"].ctypes.data, len(sc["ref_pool"]), obs.ctypes.data, None if mot is None else mot.ctypes.data, n_obs_total)
    assert rc == 0, pl.lib.pp_last_error()
    pl.n = len(si)


class DeviceBackend:
    name = "device"

    def run(self, dm, polylines, worlds, tf, dt, steps, follow=True, motion=False, K=0):
        lay = Layout(dm, worlds, K)
        tracks, pts = ts.pack(dm, polylines)
        n, na = lay.n, len(lay.act)
        cfg = dm.default_config(128)
        cfg["grid_stage"] = 0
        sc = dm.gen_scenes(cfg, 0, n, 1, junction_every=0)
        si = sc["scene_in"]
        si["obs_off"], si["obs_n"] = lay.off, lay.own
        for f in ("x", "y"):
            si["loc"]["globalpoint"][f] = lay.si["loc"]["globalpoint"][f]
        si["loc"]["velocity"] = lay.si["loc"]["velocity"]
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=max(lay.total, 1))
        set_scenes(pl, sc, si, lay.filled(dm.ObPoint), lay.filled(dm.ObMotion) if motion else None, lay.total)
        pl.set_state(sc["state"])
        pl.set_fleet(lay.world_first, lay.fm)
        pl.set_world_traffic(tracks, pts, lay.act)
        if follow:
            pl.set_traffic_follow(fb.fm_record(dm, tf))
        model = dm.default_ego_model()
        model["dt"], model["window"] = dt, 1
        po = fb.staging_plan(dm, lay.egos, dt)
        seen_si, seen_flags = {0: pl.get_scene_in()}, {0: np.zeros(n, np.int32)}
        s, v, sl, pools, mots = [], [], [], [], []

        def whole_pools():                                       # of the set the last tick adopted: the stage before
            pools.append(pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, max(lay.total, 1)))
            mots.append(pl.read_device(dm.BUF_MOT_POOL, dm.ObMotion, max(lay.total, 1)) if motion else None)

        for k in range(steps + 1):
            if k > 0:
                seen_si[k], seen_flags[k] = fb.staged_step(dm, pl, model, po, whole_pools)
            s.append(pl.traffic_state()), v.append(pl.traffic_speed() if follow else np.ascontiguousarray(lay.act["speed"]).copy())
            sl.append([pl.get_obstacles(c, cap=int(lay.own[c]) + K) for c in range(n)])
        pl.tick()
        whole_pools()
        pl.close()
        fb.check_staged_egos(seen_si, seen_flags, lay.si, lay.flags, steps)
        want = _run_model(dm, polylines, lay, lambda k: seen_si[k], lambda k: seen_flags[k], tf, dt, steps, follow, motion)
        for k in range(steps + 1):
            assert s[k].tobytes() == want.s[k].tobytes(), f"stage {k}: arc lengths differ from the model's at vehicles {np.flatnonzero(s[k] != want.s[k]).tolist()[:20]}"
            if follow:
                assert v[k].tobytes() == want.v[k].tobytes(), f"stage {k}: speeds differ from the model's at vehicles {np.flatnonzero(v[k] != want.v[k]).tolist()[:20]}"
            for c in range(n):
                assert sl[k][c].tobytes() == want.slices[k][c].tobytes(), f"stage {k}: the slice of scene {c} differs from the model's"
            assert pools[k].tobytes() == want.pool[k].tobytes(), f"stage {k}: pool entries {np.flatnonzero(pools[k] != want.pool[k]).tolist()[:20]} differ from the model's"
            assert not motion or mots[k].tobytes() == want.mot[k].tobytes(), f"stage {k}: the motion pool differs from the model's"
        return Result(s, v, sl, pools, mots, want.info, lay)


class Runner:
    """run(polylines, worlds, tf=None, dt=0.5, steps=2, follow=True, motion=False, K=0); logs every call for the batched replay."""

    def __init__(self, dm, backend, log=None):
        self.dm, self.backend, self.name, self.log = dm, backend, backend.name, log

    def __call__(self, polylines, worlds, tf=None, dt=0.5, steps=2, follow=True, motion=False, K=0):
        tf = fm.params(tf)
        res = self.backend.run(self.dm, polylines, worlds, tf, dt, steps, follow, motion, K)
        if self.log is not None:
            self.log.append(dict(polylines=polylines, worlds=worlds, tf=tf, dt=dt, steps=steps, follow=follow, motion=motion, K=K, res=res))
        return res


def batched(dm, backend, log):
    """Every logged call as worlds of ONE launch per (model, dt, steps, follow, motion, K) - a launch has one of each -: tracks and
    worlds concatenated, track indices moved.  Every vehicle must give the s, v and entry bytes - in every member scene - it gave
    alone.  Returns (launches, vehicles of the largest launch)."""
    keys, largest = {}, 0
    for c in log:
        keys.setdefault((tuple(sorted((k, float(x)) for k, x in c["tf"].items())), c["dt"], c["steps"], c["follow"], c["motion"], c["K"]), []).append(c)
    for calls in keys.values():
        polylines, worlds, alone = [], [], []
        for c in calls:
            base, a = len(polylines), 0
            polylines += c["polylines"]
            for W in c["worlds"]:
                worlds.append(dict(W, actors=[(r[0], r[1], r[2] + base, r[3], r[4]) for r in W["actors"]]))
                alone += [(c["res"], a + k) for k in range(len(W["actors"]))]
                a += len(W["actors"])
        c0 = calls[0]
        res = backend.run(dm, polylines, worlds, c0["tf"], c0["dt"], c0["steps"], c0["follow"], c0["motion"], c0["K"])
        for k, (r, a) in enumerate(alone):
            for stage in range(c0["steps"] + 1):
                assert res.s[stage][k].tobytes() == r.s[stage][a].tobytes(), f"vehicle {k}, stage {stage}: s"
                assert res.v[stage][k].tobytes() == r.v[stage][a].tobytes(), f"vehicle {k}, stage {stage}: v"
                assert len(res.layout.entries[k]) == len(r.layout.entries[a])
                for m in range(len(r.layout.entries[a])):
                    assert res.entry(stage, k, m).tobytes() == r.entry(stage, a, m).tobytes(), f"vehicle {k}, stage {stage}, member {m}: ObPoint"
        largest = max(largest, len(alone))
    return len(keys), largest
