"""The two backends of tests/advance_backends.py for a handle with a GridFollow model (pp_set_grid_follow).

Everything is reused by import: the device backend is advance_backends.DeviceBackend - the same injection of crafted PlanOut /
SceneState through a real tick - on a Planner that switches following on as soon as it exists (the `first` hook of
advance_harness.open_planner), so before the first advance (and before set_map / set_egos / set_scenes, which the model must
survive); the model backend is tests/grid_follow_model.py around the
models advance_backends uses.  Runner holds every device step against that model on the device's own records of the step before,
as advance_backends.Runner does, and `batched` runs advance_backends.batched once per GridFollow model (a model is a kernel
argument: only calls with the same one can share a launch)."""
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
        super().__init__(lambda pl: pl.set_grid_follow(self.gf))


def compare(got, want, what):
    ab.compare(got, want, what, ab.STATS)
    for name in ("grid_origin", "goal"):          # §4g: to the last bit
        assert got.out[name].tobytes() == want.out[name].tobytes(), f"{what}: {name} {got.out[name]} against {want.out[name]}"


class Runner(ab.Runner):
    """advance_backends.Runner with the GridFollow model: what a known answer calls."""
    def __init__(self, name, gf, log=None):
        self.gf = gf = _gf(gf)
        super().__init__(ModelBackend(gf) if name == "model" else DeviceBackend(gf), log, check=compare, gf=gf,
                         step=lambda cfg, model, cur, s, flags, world, route: model_step(cfg, model, gf, cur, s[0], s[1], flags, world, route))


def batched(log, min_scenes=5):
    """advance_backends.batched on the device, once per GridFollow model of the logged calls.  Returns the batch sizes."""
    by_gf = {}
    for call in log:
        by_gf.setdefault(b"" if call.case.gf is None else call.case.gf.tobytes(), []).append(call)
    sizes = []
    for calls in by_gf.values():
        sizes += ab.batched(DeviceBackend(calls[0].case.gf), calls, min_scenes)
    return sizes
