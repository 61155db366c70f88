"""The two backends of tests/advance_backends.py for a handle with an EgoTracker (pp_set_ego_tracker).

The device backend follows advance_backends.DeviceBackend - crafted PlanOut / SceneState injected through a real tick - on a Planner
that sets the tracker as soon as it exists (before set_map / set_egos / set_scenes, which the model must survive), and reads the
EgoTrackState records after every advance.  The model backend is tests/ego_track_model.py around the models advance_backends uses.
The states cannot be handed to the device: a call starts from the zeroed states a set call leaves and chains its own steps.

A step is (PlanOut[n], SceneState[n]) or (PlanOut[n], SceneState[n], SceneIn[n], mask[n]): before that step the records of the
scenes with mask set are replaced the way a caller does it - pp_update_async with the current records patched, one tick that adopts
them - and the advance then reads them.

compare() holds the device against the model on the device's own records of the step before: everything advance_backends.compare
checks, and x, y, velocity and every EgoTrackState byte exactly.  key_dir is by definition the bits of the `dir` that was stored,
and `dir` is an `atan` (advance_backends.DIR_TOL): each side's key_dir is held against its own dir."""
import hashlib

import numpy as np

import advance_backends as ab
import dmpp_amd as dm
import ego_track_model as etm

STATE_EXACT = ("hx", "hy", "kappa", "key_x", "key_y", "max_kappa", "valid", "n_init", "n_sat", "_pad")


def _tk(tk):
    return None if tk is None else np.array(tk, dm.EgoTracker).reshape(1).copy()


class Result(ab.Result):
    def __init__(self, out, flags, trace, track, gaps=None):
        super().__init__(out, flags, trace, gaps)
        self.track = track


def split(step, cur):
    """(po, st, records the advance reads) of a step."""
    if len(step) == 2:
        return step[0], step[1], cur
    po, st, upd, mask = step
    new = cur.copy()
    new[np.asarray(mask, bool)] = upd[np.asarray(mask, bool)]
    return po, st, new


def model_step(cfg, model, tk, track, si, po, st, flags, world, route=None, age0=None):
    n = len(si)
    if "map" in world:
        legs, rf, rm = ab._route(route, n)
        out, f, gaps, track = etm.advance(dm, cfg, model, tk, track, si, po, st, flags, age0=age0, route=(rm, legs, rf, world["map"]))
    else:
        out, f, gaps, track = etm.advance(dm, cfg, model, tk, track, si, po, st, flags, age0=age0, lane_pool=world["lane_pool"], map_mode=False)
    return Result(out, f, ab.trace_of(out, f), track, gaps)


class ModelBackend:
    name = "model"

    def __init__(self, tk):
        self.tk = _tk(tk)

    def run(self, cfg, model, si, steps, world, route=None):
        res, flags, track = [], np.zeros(len(si), np.int32), np.zeros(len(si), dm.EgoTrackState)
        for step in steps:
            po, st, si = split(step, si)
            res.append(model_step(cfg, model, self.tk, track, si, po, st, flags, world, route))
            si, flags, track = res[-1].out, res[-1].flags, res[-1].track
        return res


class DeviceBackend:
    name = "device"

    def __init__(self, tk):
        self.tk = _tk(tk)

    def run(self, cfg, model, si, steps, world, route=None):
        n = len(si)
        sc = dict(scene_in=si, obs_pool=np.zeros(1, dm.ObPoint), mot_pool=np.zeros(1, dm.ObMotion), n_obs=0)
        if "map" in world:
            m = world["map"]
            pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=1, max_lane_pts_total=len(m["points"]), max_ref_pts_total=max(len(m["jpoints"]), 1))
            pl.set_ego_tracker(self.tk)
            pl.set_map(m)
            pl.set_egos(sc, with_motion=False)
            if route is not None:
                legs, rf, rm = ab._route(route, n)
                pl.set_route(legs, rf, rm)
        else:
            pool, ref = world["lane_pool"], world.get("ref_pool", np.zeros(1, dm.GlobalPoint2D))
            sc.update(lane_pool=pool, attr_pool=np.zeros(len(pool), np.uint8), ref_pool=ref)
            pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=1, max_lane_pts_total=len(pool), max_ref_pts_total=len(ref))
            pl.set_ego_tracker(self.tk)
            pl.set_scenes(sc, with_motion=False)
        state = np.zeros(n, dm.SceneState)
        pl.lib.pp_init_state(state.ctypes.data, n)
        pl.set_state(state)
        assert pl.get_scene_in().tobytes() == si.tobytes(), "the resident records are the crafted ones (views resolved, slices inside the pools)"
        if self.tk is not None:
            assert not pl.ego_track_state().tobytes().strip(b"\0"), "a set call leaves zeroed states"
        trace, res, pin = dm.pinned_empty(n, dm.EgoTrace), [], dm.pinned_empty(n, dm.SceneIn)
        for k, step in enumerate(steps):
            if len(step) == 4:                            # the caller's update: adopted by a tick of its own, read by the advance below
                assert k > 0, "an update follows an advance"
                pl.tick()
                pin[:] = split(step, pl.get_scene_in())[2]
                pl.update_async(scene_in=pin)
            pl.tick()                                     # the tick an advance follows; what it wrote is replaced below
            pl.write_device(dm.BUF_PLAN_OUT, step[0])
            pl.write_device(dm.BUF_STATE, step[1])
            pl.advance_async(model, trace)
            out, f = pl.get_scene_in(), pl.ego_flags()
            track = pl.ego_track_state() if self.tk is not None else np.zeros(n, dm.EgoTrackState)
            pl.sync()
            res.append(Result(out, f, np.array(trace), track))
        pl.close()
        return res


def compare(got, want, what, stats=None):
    ab.compare(got, want, what, stats)
    for name in ("x", "y"):
        assert got.out["loc"]["globalpoint"][name].tobytes() == want.out["loc"]["globalpoint"][name].tobytes(), f"{what}: {name} to the bit"
    assert got.out["loc"]["velocity"].tobytes() == want.out["loc"]["velocity"].tobytes(), f"{what}: velocity to the bit"
    for name in STATE_EXACT:
        assert got.track[name].tobytes() == want.track[name].tobytes(), f"{what}: EgoTrackState.{name} {got.track[name]} against {want.track[name]}"
    for r, side in ((got, "device"), (want, "model")):
        stored = r.track["valid"] != 0
        same = r.track["key_dir"] == r.out["loc"]["globalpoint"]["dir"].view(np.uint64)
        moved = r.track["key_x"] == r.out["loc"]["globalpoint"]["x"].view(np.uint64)      # (a scene the advance froze or refused keeps an older key)
        assert (same | ~stored | ~moved).all(), f"{what}: key_dir is not the bits of the dir the {side} stored"


class Runner:
    """advance_backends.Runner with the tracker: what a known answer calls."""
    def __init__(self, name, tk, log=None):
        self.tk, self.name, self.log = _tk(tk), name, log
        self.backend = ModelBackend(tk) if name == "model" else DeviceBackend(tk)

    def __call__(self, cfg, model, si, steps, world, route=None):
        res = self.backend.run(cfg, model, si, steps, world, route)
        cur, flags, track = si, np.zeros(len(si), np.int32), np.zeros(len(si), dm.EgoTrackState)
        for k, r in enumerate(res):
            ab.check_trace(r, f"{self.name} step {k}")
            if self.name == "device":
                po, st, cur = split(steps[k], cur)
                compare(r, model_step(cfg, model, self.tk, track, cur, po, st, flags, world, route), f"step {k}", ab.STATS)
            cur, flags, track = r.out, r.flags, r.track
        if self.log is not None:
            self.log.append(dict(cfg=cfg.copy(), model=model.copy(), si=si.copy(), steps=[tuple(np.copy(a) for a in s) for s in steps], world=world,
                                 route=route, res=res, tk=self.tk))
        return res


def _key(case):
    h = hashlib.sha1()
    h.update(case["cfg"].tobytes() + case["model"].tobytes() + case["tk"].tobytes() + bytes([len(case["steps"])]))
    h.update(b"map" if "map" in case["world"] else b"slice")
    if "map" in case["world"]:
        for k in sorted(case["world"]["map"]):
            h.update(np.ascontiguousarray(case["world"]["map"][k]).tobytes())
        h.update(b"-" if case["route"] is None else ab._route(case["route"], 1)[2].tobytes())
    return h.hexdigest()


def batched(log, sizes_wanted=(5, 7)):
    """Every logged single-scene device call again, as distinct scenes of one launch.  The calls that can share a launch (same
    configuration, ego model, tracker, world kind, map, route model, number of steps) are cut into batches of sizes_wanted scenes in
    turn - never a multiple of four, more than one block - the first calls repeated to fill the last batch.  Slice-mode lane pools
    are laid one behind the other and the views moved by their pool's offset.  Every scene must give the bytes it gave alone: SceneIn,
    flags, trace and EgoTrackState.  Returns the batch sizes."""
    groups = {}
    for case in log:
        assert len(case["si"]) == 1
        groups.setdefault(_key(case), []).append(case)
    sizes = []
    for group in groups.values():
        todo, turn = list(group), 0
        while todo:
            want = sizes_wanted[turn % len(sizes_wanted)]
            turn += 1
            cases, todo = todo[:want], todo[want:]
            k = 0
            while len(cases) < want:
                cases.append(group[k % len(group)])
                k += 1
            sizes.append(_batch(cases))
    sizes.append(_batch(routed_calls()))
    return sizes


def routed_calls():
    """Five routed one-scene calls on the device (k_advance_route<true>), each held against the model by the Runner, as one more
    input of batched(): the inputs of the known answers of tests/test_route.py with the ego ON the start of its path, heading along
    it - road -> pre-junction, pre-junction -> junction, junction -> next road, arrival on the last leg, a missed exit lane."""
    import test_route as tr
    m, tk, log = tr._tiny_map(dm), dm.default_ego_tracker(), []
    tk["curv_bias"] = 0.04
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    in_junction = tr._ego(dm, m, pos=2, road=2, lane=1, ego_id=0, four=(1, 2, 2, 1))
    in_junction["loc"]["id"][0, 1] = 6
    calls = [(tr._ego(dm, m), 118.5, 0.0, 2, (1, 0)), (tr._ego(dm, m, pos=1, ego_id=90, four=(1, 2, 2, 1)), 149.5, 0.0, 2, (2, 0)), (in_junction, 154.6, 0.0, 2, (0, 0)),
             (tr._ego(dm, m, ego_id=60), 133.0, 0.0, 1, (0, ab.em.LANE_END | ab.rmod.ROUTE_END)), (tr._ego(dm, m, lane=1, ego_id=60), 133.0, 3.75, 2, (0, ab.em.LANE_END))]
    run = Runner("device", tk, log)
    for si, x0, y, n_legs, want in calls:
        g = si["loc"]["globalpoint"]
        g["x"], g["y"], g["dir"] = x0, y, 0.0
        legs = tr._legs(dm, n_legs)
        r = run(cfg, dm.default_ego_model(), si, [(tr._path(dm, x0, y), np.zeros(1, dm.SceneState))], dict(map=m), (legs, np.array([0, len(legs)], np.int32), dm.default_route_model()))[0]
        assert (int(r.out["loc"]["pos"][0]), int(r.flags[0])) == want, f"routed call from x = {x0}: pos, flags"
    return log


def _batch(cases):
    n, c0 = len(cases), cases[0]
    assert n % 4 != 0 and n > 4
    route, offs = None, np.zeros(n, np.int64)
    if "map" in c0["world"]:
        world = c0["world"]
        if c0["route"] is not None:
            legs, rf = [], [0]
            for c in cases:
                lg, f1, _ = ab._route(c["route"], 1)
                legs.append(lg[int(f1[0]):int(f1[1])])
                rf.append(rf[-1] + len(legs[-1]))
            route = (np.concatenate(legs), np.array(rf, np.int32), ab._route(c0["route"], 1)[2])
    else:
        pools, where, total = [], {}, 0
        for k, c in enumerate(cases):
            p = c["world"]["lane_pool"]
            d = p.tobytes()
            if d not in where:
                where[d] = total
                pools.append(p)
                total += len(p)
            offs[k] = where[d]
        world = dict(lane_pool=np.concatenate(pools))

    def moved(rec, sign=1):
        rec = rec.copy()
        for name in ("cur_off", "left_off", "right_off"):
            rec["lanes"][name] += sign * offs.astype(np.int32)
        return rec

    si = moved(np.concatenate([c["si"] for c in cases]))
    steps = []
    for t in range(len(c0["steps"])):
        po = np.concatenate([c["steps"][t][0] for c in cases])
        st = np.concatenate([c["steps"][t][1] for c in cases])
        if any(len(c["steps"][t]) == 4 for c in cases):
            upd = moved(np.concatenate([c["steps"][t][2] if len(c["steps"][t]) == 4 else c["si"] for c in cases]))
            mask = np.array([len(c["steps"][t]) == 4 and bool(c["steps"][t][3][0]) for c in cases])
            steps.append((po, st, upd, mask))
        else:
            steps.append((po, st))
    res = DeviceBackend(c0["tk"]).run(c0["cfg"], c0["model"], si, steps, world, route)
    for t, r in enumerate(res):
        out = moved(r.out, -1)
        for k, c in enumerate(cases):
            alone = c["res"][t]
            what = f"batch of {n}, scene {k}, step {t}"
            assert out[k].tobytes() == alone.out[0].tobytes(), what + ": SceneIn"
            assert int(r.flags[k]) == int(alone.flags[0]), what + ": flags"
            assert r.trace[k].tobytes() == alone.trace[0].tobytes(), what + ": trace"
            assert r.track[k].tobytes() == alone.track[0].tobytes(), what + ": EgoTrackState"
    return n
