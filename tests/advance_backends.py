"""Two backends for one step of the closed-loop rollout (pp_advance_async), in the spirit of kat_backends.py:
the numpy model (tests/ego_model.py, tests/route_model.py) and the HIP kernels k_advance_egos / k_advance_route.

A known answer is written once against `Runner` and asserted on both.  One call takes the configuration, the ego model, N SceneIn
records, a list of steps - each the PlanOut[N] and SceneState[N] one advance reads - the world (a lane pool: slice mode; a map:
the map store) and an optional route; it returns one Result per step: the SceneIn records the advance staged, the flag words and
the EgoTrace records.

The device cannot be handed PlanOut, SceneState or flag words, so they are injected: the handle ticks once (a tick is what an
advance follows), the host waits, the crafted records are copied over the tick's PlanOut and SceneState buffers
(Planner.write_device) and pp_advance_async runs on them.  A flag word that is set on the way in is reached the honest way: an
earlier step of the same call sets it, the handle ticks, and the next step is injected (the model chains its own steps alike).
The tick's own results are overwritten before anything reads them; the scenes keep every slice inside its pool, so the slice check
behind the advance changes nothing and the model needs no rule for it."""
import hashlib

import numpy as np

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


def _route(route, n):
    if route is None:
        return None, np.zeros(n + 1, np.int32), dm.default_route_model()
    legs, rf, rm = route
    return legs, np.ascontiguousarray(rf, np.int32), dm.default_route_model() if rm is None else rm


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

    def run(self, cfg, model, si, steps, world, route=None):
        n = len(si)
        sc = dict(scene_in=si, obs_pool=np.zeros(1, dm.ObPoint), mot_pool=np.zeros(1, dm.ObMotion), n_obs=0)
        if "map" in world:
            m = world["map"]
            pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=1, max_lane_pts_total=len(m["points"]), max_ref_pts_total=max(len(m["jpoints"]), 1))
            pl.set_map(m)
            pl.set_egos(sc, with_motion=False)
            if route is not None:
                legs, rf, rm = _route(route, n)
                pl.set_route(legs, rf, rm)
        else:
            pool, ref = world["lane_pool"], world.get("ref_pool", np.zeros(1, dm.GlobalPoint2D))
            sc.update(lane_pool=pool, attr_pool=np.zeros(len(pool), np.uint8), ref_pool=ref)
            pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=1, max_lane_pts_total=len(pool), max_ref_pts_total=len(ref))
            pl.set_scenes(sc, with_motion=False)
        state = np.zeros(n, dm.SceneState)
        pl.lib.pp_init_state(state.ctypes.data, n)
        pl.set_state(state)
        assert pl.get_scene_in().tobytes() == si.tobytes(), "the resident records are the crafted ones (views resolved, slices inside the pools)"
        trace, res = dm.pinned_empty(n, dm.EgoTrace), []
        for po, st in steps:
            pl.tick()                                     # the tick an advance follows; what it wrote is replaced below
            pl.write_device(dm.BUF_PLAN_OUT, po)
            pl.write_device(dm.BUF_STATE, st)
            pl.advance_async(model, trace)
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
    of the step before (compare), and every call is logged for batched()."""
    def __init__(self, backend, log=None):
        self.backend, self.name, self.log = backend, backend.name, log

    def __call__(self, cfg, model, si, steps, world, route=None):
        res = self.backend.run(cfg, model, si, steps, world, route)
        cur, flags = si, np.zeros(len(si), np.int32)
        for k, r in enumerate(res):
            check_trace(r, f"{self.name} step {k}")
            if self.name == "device":
                compare(r, model_step(cfg, model, cur, steps[k][0], steps[k][1], flags, world, route), f"step {k}", STATS)
            cur, flags = r.out, r.flags
        if self.log is not None:
            self.log.append(dict(cfg=cfg.copy(), model=model.copy(), si=si.copy(), steps=[(po.copy(), st.copy()) for po, st in steps], world=world,
                                 route=route, res=res))
        return res


def _key(case):
    h = hashlib.sha1()
    h.update(case["cfg"].tobytes() + case["model"].tobytes() + bytes([len(case["steps"])]))
    if "map" in case["world"]:
        for k in sorted(case["world"]["map"]):
            h.update(np.ascontiguousarray(case["world"]["map"][k]).tobytes())
        h.update(b"-" if case["route"] is None else _route(case["route"], 1)[2].tobytes())
    return h.hexdigest()


def batched(backend, log, min_scenes=5):
    """Every logged single-scene call again, as distinct scenes of one launch: the calls that can share a launch (same configuration,
    ego model, world kind, map, route model and number of steps) form one batch of at least `min_scenes` scenes - more than one
    block of four - and never a multiple of four (the first calls are repeated to get there).  Slice-mode lane pools are laid one
    behind the other and the views moved by their pool's offset.  Every scene must give the bytes it gave alone.  Returns the batch sizes."""
    groups = {}
    for case in log:
        assert len(case["si"]) == 1
        groups.setdefault(_key(case), []).append(case)
    sizes = []
    for cases in groups.values():
        cases = list(cases)
        k = 0
        while len(cases) < min_scenes or len(cases) % 4 == 0:
            cases.append(cases[k])
            k += 1
        n, c0 = len(cases), cases[0]
        si = np.concatenate([c["si"] for c in cases])
        steps = [(np.concatenate([c["steps"][t][0] for c in cases]), np.concatenate([c["steps"][t][1] for c in cases])) for t in range(len(c0["steps"]))]
        route, offs = None, np.zeros(n, np.int64)
        if "map" in c0["world"]:
            world = c0["world"]
            if c0["route"] is not None:
                legs, rf = [], [0]
                for c in cases:
                    lg, f1, _ = _route(c["route"], 1)
                    legs.append(lg[int(f1[0]):int(f1[1])])
                    rf.append(rf[-1] + len(legs[-1]))
                route = (np.concatenate(legs), np.array(rf, np.int32), _route(c0["route"], 1)[2])
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
            for name in ("cur_off", "left_off", "right_off"):
                si["lanes"][name] += offs.astype(np.int32)
        res = backend.run(c0["cfg"], c0["model"], si, steps, world, route)
        for t, r in enumerate(res):
            out = r.out.copy()
            for name in ("cur_off", "left_off", "right_off"):
                out["lanes"][name] -= offs.astype(np.int32)
            for k, c in enumerate(cases):
                alone = c["res"][t]
                what = f"batch of {n}, scene {k}, step {t}"
                assert out[k].tobytes() == alone.out[0].tobytes(), what + ": SceneIn"
                assert int(r.flags[k]) == int(alone.flags[0]), what + ": flags"
                assert r.trace[k].tobytes() == alone.trace[0].tobytes(), what + ": trace"
        sizes.append(n)
    return sizes
