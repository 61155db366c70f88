"""Two backends for the episode step of the closed-loop rollout (pp_set_episodes), in the spirit of
advance_backends.py: the numpy model (tests/episode_model.py behind tests/ego_model.py / tests/route_model.py) and the HIP kernel
k_respawn_egos behind k_advance_egos / k_advance_route.

A known answer is written once against `Runner` and asserted on both.  One call takes the configuration, the ego model, the
episode model, N SceneIn records, the SceneState the episodes start from, a list of steps - each the PlanOut[N] and SceneState[N]
one advance reads - the world (a map) and an optional route; it returns one Result per step: the SceneIn records staged for the
next tick, the flag words, the EgoTrace records, the SceneState array and the EpisodeStats after the advance - and, with
score=True, the RolloutScore records (the tick before every advance is scored, and one closing tick after the last).

PlanOut and SceneState are injected on the device as advance_backends.py does it (advance_harness.inject_advance): the handle ticks,
the host waits, the crafted records are copied over the tick's buffers and pp_advance_async runs on them.  So the scorecard on the device has folded the
tick's own PlanOut, not the crafted one: a known answer asserts only what the scorecard takes from SceneIn (dist, max_acc, max_dec,
max_speed, last_pos, last_speed, n_ticks); the whole record is held against the model in the closed loop of tests/test_episodes.py.

capture = (SceneIn[N], SceneState[N]): the start records are captured from THESE - pp_set_egos + pp_set_state + pp_set_episodes -
and the records the step runs on arrive afterwards (pp_set_state, pp_update_async), so that a restored record differs from the
staged one in every byte the test chose.  The captured records are never ticked: such a call has one step."""
import numpy as np

import advance_backends as ab
import advance_harness as ah
import dmpp_amd as dm
import episode_model as epm
import map_scenes as ms
import rollout_score_model as rsm


class Result:
    def __init__(self, out, flags, trace, state, stats, score=None):
        self.out, self.flags, self.trace, self.state, self.stats, self.score = out, flags, trace, state, stats, score


def model_step(cfg, model, em, stats, start_in, start_state, si, po, st, flags, world, route=None, score=None):
    """One advance + episode step of the model on records of any origin.  stats / score are updated in place."""
    r = ab.model_step(cfg, model, si, po, st, flags, world, route)
    out, st2, f, tr, _ = epm.step(em, stats, start_in, start_state, si, r.out, r.flags, st, r.trace, score)
    return Result(out, f, tr, st2, stats.copy(), None if score is None else score.copy())


class ModelBackend:
    name = "model"

    def run(self, cfg, model, em, si, state0, steps, world, route=None, score=False, capture=None):
        n = len(si)
        start_in, start_state = (si, state0) if capture is None else (ms.resolve(dm, world["map"], capture[0]), capture[1])
        stats, flags, res = epm.new_stats(dm.EpisodeStats, n), np.zeros(n, np.int32), []
        scores = rsm.new_scores(dm.RolloutScore, n) if score else None
        dt, none = float(model["dt"][0]), np.zeros(1, dm.ObPoint)
        for po, st in steps:
            if score:
                rsm.fold(scores, cfg, dt, si, po, st, none, flags)
            res.append(model_step(cfg, model, em, stats, start_in, start_state, si, po, st, flags, world, route, scores))
            si, flags = res[-1].out, res[-1].flags
        if score:
            rsm.fold(scores, cfg, dt, si, steps[-1][0], steps[-1][1], none, flags)
            res[-1].final_score = scores.copy()
        return res


class DeviceBackend:
    name = "device"

    def run(self, cfg, model, em, si, state0, steps, world, route=None, score=False, capture=None):
        n = len(si)
        first_in, first_state = (si, state0) if capture is None else capture
        pl = ah.open_planner(cfg, first_in, world, mot_pool=np.zeros(1, dm.ObMotion), route=route, state=first_state, then=lambda pl: pl.set_episodes(em),
                             check=capture is None)
        keep, adopted = None, None
        if capture is not None:
            assert len(steps) == 1, "the captured records are never ticked"
            assert pl.get_scene_in().tobytes() == ms.resolve(dm, world["map"], capture[0]).tobytes(), "the captured records are the crafted ones, resolved"
            pl.set_state(state0)
            keep = dm.pinned_copy(si)
            pl.update_async(scene_in=keep)

            def adopted(pl):
                assert pl.get_scene_in().tobytes() == si.tobytes(), "the records of the update are the crafted ones"
        if score:
            pl.score_begin(float(model["dt"][0]))
        trace, res = dm.pinned_empty(n, dm.EgoTrace), []
        for po, st in steps:
            ah.inject_advance(pl, model, po, st, trace, after_tick=adopted)
            out, f, stats = pl.get_scene_in(), pl.ego_flags(), pl.episode_stats()
            state = pl.get_state()                        # behind the staged advance: the restored state
            sco = pl.rollout_score() if score else None
            assert pl.read_device(dm.BUF_STATE, dm.SceneState, n).tobytes() == state.tobytes(), "pp_get_state is the SceneState buffer"
            res.append(Result(out, f, np.array(trace), state, stats, sco))
        if score:
            pl.tick()
            res[-1].final_score = pl.rollout_score()
        pl.close()
        return res


def _but_heading(rec, field):
    """A copy of SceneIn / EgoTrace records with the heading zeroed, and the headings."""
    r = rec.copy()
    d = r[field[0]]["globalpoint"]["dir"] if len(field) == 2 else r[field[0]]["dir"]
    dirs = d.copy()
    d[...] = 0.0
    return r, dirs


def same_stats(got, want):
    """EpisodeStats byte for byte - except that a distance which is a NaN on both sides is equal whatever its sign and payload:
    IEEE 754 leaves both open for the result of an operation on a NaN, §4k specifies "a NaN", and the device's `sqrt` and the
    host's hand back different ones (tests/test_episodes.py::_kat_a_nan_position is the only test that gets there)."""
    g, w = got.copy(), want.copy()
    for name in ("dist", "last_dist", "dist_total"):
        both = np.isnan(g[name]) & np.isnan(w[name])
        g[name][both], w[name][both] = 0.0, 0.0
    return g.tobytes() == w.tobytes()


def compare(got, want, what):
    """Device against model for one advance + episode step, byte for byte: the staged SceneIn records, the flag words, the trace,
    SceneState and EpisodeStats.  The one field that is not held to the bit is the heading of an ADVANCED record - GetRoadAngle of
    §4c 3., an `atan` the device's and the host's maths libraries round differently ("`atan` aside", §4c) - which keeps the bound of
    tests/test_route.py::_assert_records, 1e-6 degrees; a restored record carries the start record's heading, every bit of it."""
    assert np.array_equal(got.flags, want.flags), f"{what}: flags {got.flags.tolist()} against {want.flags.tolist()}"
    restored = (want.trace["flags"] & epm.RESPAWNED) != 0
    for g, w, field, name in ((got.out, want.out, ("loc", "globalpoint"), "SceneIn"), (got.trace, want.trace, ("pose",), "trace")):
        (g0, gd), (w0, wd) = _but_heading(g, field), _but_heading(w, field)
        assert g0.tobytes() == w0.tobytes(), f"{what}: {name} bytes"
        assert np.array_equal(np.isnan(gd), np.isnan(wd)), f"{what}: {name} heading"
        dd = np.where(gd == wd, 0.0, np.nan_to_num(np.abs(gd - wd), nan=0.0))
        assert (np.minimum(dd, 360.0 - dd) <= 1e-6).all(), f"{what}: {name} heading"
        assert gd[restored].tobytes() == wd[restored].tobytes(), f"{what}: {name} heading of a restored record"
    assert got.state.tobytes() == want.state.tobytes(), f"{what}: SceneState"
    assert same_stats(got.stats, want.stats), f"{what}: EpisodeStats {got.stats.tolist()} against {want.stats.tolist()}"


def check_trace(r, what):
    """advance_backends.check_trace with episodes: the trace of a restored record keeps the flag word that ended the episode."""
    restored = (r.trace["flags"] & epm.RESPAWNED) != 0
    want_tr = ab.trace_of(r.out, np.where(restored, r.trace["flags"], r.flags).astype(np.int32))
    assert r.trace.tobytes() == want_tr.tobytes(), f"{what}: the EgoTrace records are not the staged records"


class Runner:
    """What a known answer calls.  On the device every step is also held against the model applied to the device's own records
    of the step before (compare), and every call is logged for batched()."""
    def __init__(self, backend, log=None):
        self.backend, self.name, self.log = backend, backend.name, log

    def __call__(self, cfg, model, em, si, state0, steps, world, route=None, score=False, capture=None):
        res = self.backend.run(cfg, model, em, si, state0, steps, world, route, score, capture)
        start_in, start_state = (si, state0) if capture is None else (ms.resolve(dm, world["map"], capture[0]), capture[1])

        def step(k, cur, flags, stats):
            return model_step(cfg, model, em, stats, start_in, start_state, cur, steps[k][0], steps[k][1], flags, world, route)
        ah.hold_run(self.name, res, si, step, compare, dict(stats=epm.new_stats(dm.EpisodeStats, len(si))), check_trace)
        if self.log is not None:
            assert capture is None and not score
            self.log.append(ah.Call(ah.case_of(steps, cfg=cfg, model=model, em=em, si=si, state0=state0, world=world, route=route), res))
        return res


def _same_launch(a, b):
    return (a.cfg.tobytes() == b.cfg.tobytes() and a.model.tobytes() == b.model.tobytes() and a.em.tobytes() == b.em.tobytes() and
            len(a.steps) == len(b.steps) and a.world is b.world and ah.same_route_model(a.route, b.route))


def batched(backend, log, sizes=(5, 9)):
    """Every logged single-scene call again, as distinct scenes of one launch: the calls that can share a launch (same configuration,
    ego model, episode model, map, route model and number of steps) form a group, and each group runs in batches of every size of
    `sizes` - more than one block of four waves, never a multiple of four.  The group's calls are rotated so that a scene that
    ENDS an episode sits first, last and on either side of the block edge 4 | 5 where the group has both kinds (the filler repeats
    the group's calls).  Every scene must give the bytes it gave alone.  Returns (size, indices of the ending scenes) per batch."""
    ran = []
    for n, batch, at in ah.batches(log, _same_launch, ah.ends_episode, sizes):
        cases = [c.case for c in batch]
        res = backend.run(cases[0].cfg, cases[0].model, cases[0].em, np.concatenate([c.si for c in cases]), np.concatenate([c.state0 for c in cases]),
                          ah.join_steps(cases), cases[0].world, ah.join_routes([c.route for c in cases]))
        for t, r in enumerate(res):
            ah.same_alone(r, t, batch, ("out", "flags", "trace", "state", "stats"))
        ran.append((n, at))
    return ran
