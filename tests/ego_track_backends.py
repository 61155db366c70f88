"""The two backends of tests/advance_backends.py for a handle with an EgoTracker (pp_set_ego_tracker).

The device backend follows advance_backends.DeviceBackend - crafted PlanOut / SceneState injected through a real tick - on a Planner
that sets the tracker as soon as it exists (the `first` hook of advance_harness.open_planner: before set_map / set_egos /
set_scenes, which the model must survive), and reads the EgoTrackState records after every advance.  The model backend is
tests/ego_track_model.py around the models advance_backends uses.
The states cannot be handed to the device: a call starts from the zeroed states a set call leaves and chains its own steps.

A step is (PlanOut[n], SceneState[n]) or (PlanOut[n], SceneState[n], SceneIn[n], mask[n]): before that step the records of the
scenes with mask set are replaced the way a caller does it - pp_update_async with the current records patched, one tick that adopts
them - and the advance then reads them.

compare() holds the device against the model on the device's own records of the step before: everything advance_backends.compare
checks, and x, y, velocity and every EgoTrackState byte exactly.  key_dir is by definition the bits of the `dir` that was stored,
and `dir` is an `atan` (advance_backends.DIR_TOL): each side's key_dir is held against its own dir."""
import numpy as np

import advance_backends as ab
import advance_harness as ah
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
        pl = ah.open_planner(cfg, si, world, mot_pool=np.zeros(1, dm.ObMotion), route=route, first=lambda pl: pl.set_ego_tracker(self.tk))
        if self.tk is not None:
            assert not pl.ego_track_state().tobytes().strip(b"\0"), "a set call leaves zeroed states"
        trace, res, pin = dm.pinned_empty(n, dm.EgoTrace), [], dm.pinned_empty(n, dm.SceneIn)
        for k, step in enumerate(steps):
            if len(step) == 4:                            # the caller's update: adopted by a tick of its own, read by the advance below
                assert k > 0, "an update follows an advance"
                pl.tick()
                pin[:] = split(step, pl.get_scene_in())[2]
                pl.update_async(scene_in=pin)
            ah.inject_advance(pl, model, step[0], step[1], trace)
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


class Runner(ab.Runner):
    """advance_backends.Runner with the tracker: what a known answer calls."""
    def __init__(self, name, tk, log=None):
        self.tk = tk = _tk(tk)

        def step(cfg, model, cur, s, flags, world, route, track):
            po, st, cur = split(s, cur)
            return model_step(cfg, model, tk, track, cur, po, st, flags, world, route)
        super().__init__(ModelBackend(tk) if name == "model" else DeviceBackend(tk), log, step, lambda r, want, what: compare(r, want, what, ab.STATS),
                         lambda n: dict(track=np.zeros(n, dm.EgoTrackState)), tk=tk)


def _same_launch(a, b):
    return ab.same_launch(a, b) and a.tk.tobytes() == b.tk.tobytes()


def batched(log, sizes_wanted=(5, 7)):
    """Every logged single-scene device call again, as distinct scenes of one launch.  The calls that can share a launch (same
    configuration, ego model, tracker, world kind, map, route model, number of steps) are cut into batches of sizes_wanted scenes in
    turn - never a multiple of four, more than one block - the first calls repeated to fill the last batch.  Slice-mode lane pools
    are laid one behind the other and the views moved by their pool's offset.  Every scene must give the bytes it gave alone: SceneIn,
    flags, trace and EgoTrackState.  Returns the batch sizes."""
    sizes = []
    for group in ah.group_calls(log, _same_launch):
        todo, turn = list(group), 0
        while todo:
            want = sizes_wanted[turn % len(sizes_wanted)]
            turn += 1
            calls, todo = todo[:want], todo[want:]
            k = 0
            while len(calls) < want:
                calls.append(group[k % len(group)])
                k += 1
            sizes.append(_batch(calls))
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


def _join_steps(cases, moved):
    """advance_harness.join_steps, and the update of a step that has one in any case: the other cases' records masked out."""
    steps = ah.join_steps(cases)
    for t, (po, st) in enumerate(steps):
        if any(len(c.steps[t]) == 4 for c in cases):
            upd = moved(np.concatenate([c.steps[t][2] if len(c.steps[t]) == 4 else c.si for c in cases]))
            steps[t] = (po, st, upd, np.array([len(c.steps[t]) == 4 and bool(c.steps[t][3][0]) for c in cases]))
    return steps


def _batch(calls):
    return ab.batch(DeviceBackend(calls[0].case.tk), calls, ("out", "flags", "trace", "track"), _join_steps)
