"""The two backends of tests/advance_backends.py for a handle with a GridFollow model (pp_set_grid_follow).

Everything is reused by import: the device backend is advance_backends.DeviceBackend - the same injection of crafted PlanOut /
SceneState through a real tick - on a Planner that switches following on as soon as it exists, so before the first advance (and
before set_map / set_egos / set_scenes, which the model must survive); the model backend is tests/grid_follow_model.py around the
models advance_backends uses.  Runner holds every device step against that model on the device's own records of the step before,
as advance_backends.Runner does, and `batched` runs advance_backends.batched once per GridFollow model (a model is a kernel
argument: only calls with the same one can share a launch)."""
from unittest import mock

import numpy as np

import advance_backends as ab
import dmpp_amd as dm
import grid_follow_model as gfm


def _gf(gf):
    return None if gf is None else np.array(gf, dm.GridFollow).reshape(1).copy()


def model_step(cfg, model, gf, si, po, st, flags, world, route=None):
    n = len(si)
    if "map" in world:
        legs, rf, rm = ab._route(route, n)
        out, f, gaps = gfm.advance(dm, cfg, model, gf, si, po, st, flags, route=(rm, legs, rf, world["map"]))
    else:
        out, f, gaps = gfm.advance(dm, cfg, model, gf, si, po, st, flags, lane_pool=world["lane_pool"], map_mode=False)
    return ab.Result(out, f, ab.trace_of(out, f), gaps)


class ModelBackend:
    name = "model"

    def __init__(self, gf):
        self.gf = _gf(gf)

    def run(self, cfg, model, si, steps, world, route=None):
        res, flags = [], np.zeros(len(si), np.int32)
        for po, st in steps:
            res.append(model_step(cfg, model, self.gf, si, po, st, flags, world, route))
            si, flags = res[-1].out, res[-1].flags
        return res


class DeviceBackend(ab.DeviceBackend):
    def __init__(self, gf):
        self.gf = _gf(gf)

    def run(self, cfg, model, si, steps, world, route=None):
        gf = self.gf

        class FollowingPlanner(dm.Planner):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                self.set_grid_follow(gf)

        with mock.patch.object(ab.dm, "Planner", FollowingPlanner):
            return super().run(cfg, model, si, steps, world, route)


class Runner:
    """advance_backends.Runner with the GridFollow model: what a known answer calls."""
    def __init__(self, name, gf, log=None):
        self.gf, self.name, self.log = _gf(gf), name, log
        self.backend = ModelBackend(gf) if name == "model" else DeviceBackend(gf)

    def __call__(self, cfg, model, si, steps, world, route=None):
        res = self.backend.run(cfg, model, si, steps, world, route)
        cur, flags = si, np.zeros(len(si), np.int32)
        for k, r in enumerate(res):
            ab.check_trace(r, f"{self.name} step {k}")
            if self.name == "device":
                want = model_step(cfg, model, self.gf, cur, steps[k][0], steps[k][1], flags, world, route)
                ab.compare(r, want, f"step {k}", ab.STATS)
                for name in ("grid_origin", "goal"):          # §4g: to the last bit
                    assert r.out[name].tobytes() == want.out[name].tobytes(), f"step {k}: {name} {r.out[name]} against {want.out[name]}"
            cur, flags = r.out, r.flags
        if self.log is not None:
            self.log.append(dict(cfg=cfg.copy(), model=model.copy(), si=si.copy(), steps=[(po.copy(), st.copy()) for po, st in steps], world=world,
                                 route=route, res=res, gf=self.gf))
        return res


def batched(log, min_scenes=5):
    """advance_backends.batched on the device, once per GridFollow model of the logged calls.  Returns the batch sizes."""
    by_gf = {}
    for case in log:
        by_gf.setdefault(b"" if case["gf"] is None else case["gf"].tobytes(), []).append(case)
    sizes = []
    for cases in by_gf.values():
        sizes += ab.batched(DeviceBackend(cases[0]["gf"]), cases, min_scenes)
    return sizes
