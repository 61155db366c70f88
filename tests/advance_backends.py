"""Two backends for one step of the closed-loop rollout (pp_advance_async), in the spirit of kat_backends.py:
the numpy model (tests/ego_model.py, tests/route_model.py) and the HIP kernels k_advance_egos / k_advance_route.

A known answer is written once against `Runner` and asserted on both.  One call takes the configuration, the ego model, N SceneIn
records, a list of steps - each the PlanOut[N] and SceneState[N] one advance reads - the world (a lane pool: slice mode; a map:
the map store) and an optional route; it returns one Result per step: the SceneIn records the advance staged, the flag words and
the EgoTrace records.

PlanOut, SceneState and flag words are injected on the device: tests/advance_harness.py (inject_advance) on how and why."""
import numpy as np

import advance_harness as ah
import dmpp_amd as dm
import ego_model as em
import route_model as rmod

X_TOL, DIR_TOL = 1e-9, 1e-6          # x / y / velocity; heading in degrees: the bounds of test_step_check_against_the_model


class Result:
    """One advance: SceneIn records staged for the next tick, flag words, EgoTrace records; gaps: model only (smallest difference
    between the two best squared distances of any id search of the scene: 0.0 is an exact tie)."""
    def __init__(self, out, flags, trace, gaps=None):
        self.out, self.flags, self.trace, self.gaps = out, flags, trace, gaps


def trace_of(out, flags):
    """The EgoTrace records §4c defines for staged records `out`: pose, speed, the id of slot clamp(lane_num - 1, 0, 7), lane, flags."""
    n = len(out)
    tr = np.zeros(n, dm.EgoTrace)
    loc = out["loc"]
    tr["pose"], tr["velocity"], tr["lane_num"], tr["flags"] = loc["globalpoint"], loc["velocity"], loc["lane_num"], flags
    tr["id_cur"] = loc["id"][np.arange(n), np.clip(loc["lane_num"], 1, dm.LANESUM) - 1]
    return tr


_route = ah.route_of


def model_step(cfg, model, si, po, st, flags, world, route=None):
    n = len(si)
    if "map" in world:
        legs, rf, rm = _route(route, n)
        out, f, gaps = rmod.advance(dm, cfg, model, rm, legs, rf, world["map"], si, po, st, flags)      # (resolve: as k_resolve_map behind the kernel)
    else:
        out, f, gaps = em.advance(cfg, model, si, po, st, flags, world["lane_pool"], False)
    return Result(out, f, trace_of(out, f), gaps)


class ModelBackend:
    name = "model"

    def run(self, cfg, model, si, steps, world, route=None):
        res, flags = [], np.zeros(len(si), np.int32)
        for po, st in steps:
            res.append(model_step(cfg, model, si, po, st, flags, world, route))
            si, flags = res[-1].out, res[-1].flags
        return res


class DeviceBackend:
    name = "device"

    def __init__(self, first=None):
        self.first = first          # set calls of a feature that come before the records (advance_harness.open_planner)

    def run(self, cfg, model, si, steps, world, route=None):
        pl = ah.open_planner(cfg, si, world, mot_pool=np.zeros(1, dm.ObMotion), route=route, first=self.first)
        trace, res = dm.pinned_empty(len(si), dm.EgoTrace), []
        for po, st in steps:
            ah.inject_advance(pl, model, po, st, trace)
            out, f = pl.get_scene_in(), pl.ego_flags()
            pl.sync()
            res.append(Result(out, f, np.array(trace)))
        pl.close()
        return res


def _wrap(d):
    return np.minimum(d, 360.0 - d)


def compare(got, want, what, stats=None):
    """Device against model for one advance: integers, flags, ids, lane numbers and every carried-over byte exact, x / y / velocity
    within 1e-9, the heading within 1e-6 degrees, the trace alike.  No scene is left out for a tie."""
    assert np.array_equal(got.flags, want.flags), f"{what}: flags {got.flags.tolist()} against {want.flags.tolist()}"
    g, w = got.out.copy(), want.out.copy()
    diffs = {}
    for name, tol in (("x", X_TOL), ("y", X_TOL), ("dir", DIR_TOL)):
        a, b = g["loc"]["globalpoint"][name], w["loc"]["globalpoint"][name]
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: {name}"
        d = np.nan_to_num(np.abs(a - b), nan=0.0)
        d = np.where(a == b, 0.0, _wrap(d) if name == "dir" else d)          # (equal infinities are equal)
        diffs[name] = float(d.max())
        assert diffs[name] <= tol, f"{what}: {name} off by {diffs[name]!r}"
        g["loc"]["globalpoint"][name], w["loc"]["globalpoint"][name] = 0.0, 0.0
    a, b = g["loc"]["velocity"], w["loc"]["velocity"]
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: velocity"
    diffs["v"] = float(np.where(a == b, 0.0, np.nan_to_num(np.abs(a - b), nan=0.0)).max())
    assert diffs["v"] <= X_TOL, f"{what}: velocity off by {diffs['v']!r}"
    g["loc"]["velocity"], w["loc"]["velocity"] = 0.0, 0.0
    assert np.array_equal(g["loc"]["id"], w["loc"]["id"]), f"{what}: ids {g['loc']['id'].tolist()} against {w['loc']['id'].tolist()}"
    assert g.tobytes() == w.tobytes(), f"{what}: the integers and the carried-over bytes of the records"
    for name in ("id_cur", "lane_num", "flags", "_pad"):
        assert np.array_equal(got.trace[name], want.trace[name]), f"{what}: trace {name}"
    bits = int((got.out["loc"]["globalpoint"].tobytes() != want.out["loc"]["globalpoint"].tobytes()) or
               (got.out["loc"]["velocity"].tobytes() != want.out["loc"]["velocity"].tobytes()))
    if stats is not None:
        for k, v in diffs.items():
            stats[k] = max(stats.get(k, 0.0), v)
        stats["advances"] = stats.get("advances", 0) + 1
        stats["not_bit_equal"] = stats.get("not_bit_equal", 0) + bits


def check_trace(r, what):
    """The trace is the written record (§4c): every byte, the heading included."""
    assert r.trace.tobytes() == trace_of(r.out, r.flags).tobytes(), f"{what}: the EgoTrace records are not the staged records"


STATS = {}


class Runner:
    """What a known answer calls.  On the device every step is also held against the model applied to the device's own records
    of the step before (compare), and every call is logged for batched().  The families on the same call signature (grid follow,
    ego tracker) pass their own step(cfg, model, records, step, flags, world, route, **carried) and check(got, want, what), what the model carries
    from step to step (carried(n)) and what they add to a logged case (feature: gf=..., tk=...)."""
    def __init__(self, backend, log=None, step=None, check=None, carried=None, **feature):
        self.backend, self.name, self.log, self.carried, self.feature = backend, backend.name, log, carried, feature
        self.step = step or (lambda cfg, model, cur, s, flags, world, route: model_step(cfg, model, cur, s[0], s[1], flags, world, route))
        self.check = check or (lambda r, want, what: compare(r, want, what, STATS))

    def __call__(self, cfg, model, si, steps, world, route=None):
        res = self.backend.run(cfg, model, si, steps, world, route)
        ah.hold_run(self.name, res, si, lambda k, cur, flags, **kept: self.step(cfg, model, cur, steps[k], flags, world, route, **kept), self.check,
                    self.carried and self.carried(len(si)), check_trace)
        if self.log is not None:
            self.log.append(ah.Call(ah.case_of(steps, cfg=cfg, model=model, si=si, world=world, route=route, **self.feature), res))
        return res


def same_launch(a, b):
    """Same configuration, ego model, number of steps and world kind; in map mode the same map and route model."""
    if a.cfg.tobytes() != b.cfg.tobytes() or a.model.tobytes() != b.model.tobytes() or len(a.steps) != len(b.steps) or ("map" in a.world) != ("map" in b.world):
        return False
    if "map" not in a.world:
        return True
    ma, mb = a.world["map"], b.world["map"]
    same_map = sorted(ma) == sorted(mb) and all(np.ascontiguousarray(ma[k]).tobytes() == np.ascontiguousarray(mb[k]).tobytes() for k in ma)
    return same_map and ah.same_route_model(a.route, b.route)


def batch(backend, calls, attrs=("out", "flags", "trace"), join_steps=lambda cases, moved: ah.join_steps(cases)):
    """The one-scene calls as the scenes of one launch on `backend` (a DeviceBackend of this family).  Slice-mode lane pools are laid
    one behind the other and the views moved by their pool's offset.  Every scene must give the bytes it gave alone: `attrs`."""
    n, c0 = len(calls), calls[0].case
    assert n % 4 != 0 and n > 4
    world, route, moved = ah.join_world([c.case for c in calls])
    res = backend.run(c0.cfg, c0.model, moved(np.concatenate([c.case.si for c in calls])), join_steps([c.case for c in calls], moved), world, route)
    for t, r in enumerate(res):
        ah.same_alone(r, t, calls, attrs, moved=moved)
    return n


def batched(backend, log, min_scenes=5):
    """Every logged single-scene call again, as distinct scenes of one launch: the calls that can share a launch (same configuration,
    ego model, world kind, map, route model and number of steps) form one batch of at least `min_scenes` scenes - more than one
    block of four - and never a multiple of four (the first calls are repeated to get there).  Slice-mode lane pools are laid one
    behind the other and the views moved by their pool's offset.  Every scene must give the bytes it gave alone.  Returns the batch sizes."""
    sizes = []
    for calls in ah.group_calls(log, same_launch):
        k = 0
        while len(calls) < min_scenes or len(calls) % 4 == 0:
            calls.append(calls[k])
            k += 1
        sizes.append(batch(backend, calls))
    return sizes
