"""Two backends for the score trace, on top of the scorecard backends of coupling_backends.py: the numpy model
tests/score_trace_model.py and k_score_ego<., true> inside a real tick.

One call takes the configuration, dt_score, the ScoreTraceModel, a list of coupling_backends.Tick and - optionally - the scenes to
re-arm behind given ticks; it returns, per tick, the headers, every scene's ring as pp_read_score_trace copies it (oldest first) and
the RolloutScore records.  The model leg folds the crafted PlanOut / SceneState / flag word of a Tick; the device leg cannot be handed
those in front of k_score_ego (coupling_backends.py), so what follows from the crafted inputs alone a case asserts as literals on both
legs, and headers and rings are held byte for byte against the model stepped over the device's own PlanOut, SceneState and flag words
of that tick.  Tick ids: a fresh handle numbers its ticks from 1, and so does the model leg."""
import numpy as np

import coupling_backends as cb
import dmpp_amd as dm
import rollout_score_model as sm
import score_trace_model as stm


class TraceResult:
    """info[k], rings[k][s], score[k]: behind tick k (behind its re-arms too)."""
    def __init__(self):
        self.info, self.rings, self.score = [], [], []


def _model(m):
    return np.array(m, dm.ScoreTraceModel).reshape(1).copy()


class ModelBackend:
    name = "model"

    def run(self, cfg, dt, model, ticks, rearm=None):
        model, n = _model(model), len(ticks[0].si)
        scores = sm.new_scores(dm.RolloutScore, n)
        rings, info = stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, int(model["depth"][0]))
        res = TraceResult()
        for k, t in enumerate(ticks):
            po, st, flags = cb._crafted(t)
            stm.step(rings, info, model, scores, cfg, dt, k + 1, t.si, po, st, t.pool, flags)
            sm.fold(scores, cfg, dt, t.si, po, st, t.pool, flags)
            for s in (rearm or {}).get(k, ()):
                stm.rearm(info, s)
            res.info.append(info.copy()), res.rings.append([stm.oldest_first(rings, info, s) for s in range(n)]), res.score.append(scores.copy())
        return res


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.shape} against {b.shape}"
    assert a.tobytes() == b.tobytes(), what + ": " + ", ".join(f"{f} {a[f].tolist()} / {b[f].tolist()}" for f in a.dtype.names if a[f].tobytes() != b[f].tobytes())


def open_planner(cfg, ticks, model=None, score=True, dt=0.5):
    """A slice-mode handle on the road of coupling_backends with the first tick's records resident; model None: the trace is never set."""
    sc, n = cb.road(cfg), len(ticks[0].si)
    cap = max(len(t.pool) for t in ticks)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=cap, max_lane_pts_total=len(sc["lane_pool"]), max_ref_pts_total=len(sc["ref_pool"]))
    first = np.zeros(cap, dm.ObPoint)
    first[:len(ticks[0].pool)] = ticks[0].pool
    cb._set_scenes(pl, sc, ticks[0].si, first, None, cap)
    pl.set_state(np.repeat(sc["state"][:1], n))
    if model is not None:
        pl.set_score_trace(model)
    if score:
        pl.score_begin(dt)
    return pl


def feed(pl, t, keep):
    """One crafted tick through the handle; returns (SceneIn it read, PlanOut, SceneState behind it)."""
    in_t, obs_t, plan_p = dm.pinned_copy(t.si), dm.pinned_copy(t.pool), dm.pinned_empty(len(t.si), dm.PlanOut)
    keep.append((in_t, obs_t, plan_p))
    pl.update_async(in_t, obs_t)
    pl.tick()
    assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
    sin = pl.get_scene_in()
    assert sin.tobytes() == t.si.tobytes(), "the tick read the crafted records (every slice inside its pool)"
    return sin, np.array(plan_p), pl.get_state()


def read_all(pl, n):
    """(headers, [ring of every scene, oldest first]); every ring is read under the header the batch call gave."""
    info = pl.score_trace_info()
    rings = []
    for s in range(n):
        ring, hd = pl.read_score_trace(s)
        assert hd.tobytes() == info[s].tobytes(), f"scene {s}: the header of the read"
        rings.append(ring)
    return info, rings


class DeviceBackend:
    name = "device"

    def run(self, cfg, dt, model, ticks, rearm=None):
        assert not int(cfg["grid_stage"][0]) and not int(cfg["decision_stage"][0]) and not int(cfg["dynamic_obstacles"][0])
        model, n = _model(model), len(ticks[0].si)
        pl = open_planner(cfg, ticks, model, True, dt)
        want = sm.new_scores(dm.RolloutScore, n)
        wrings, winfo = stm.new_trace(dm.ScoreTick, dm.ScoreTraceInfo, n, int(model["depth"][0]))
        same(pl.score_trace_info(), winfo, "before the first tick")
        res, keep = TraceResult(), []
        for k, t in enumerate(ticks):
            sin, plan, state = feed(pl, t, keep)
            flags = pl.ego_flags()
            stm.step(wrings, winfo, model, want, cfg, dt, pl.tick_id(), sin, plan, state, t.pool, flags)
            sm.fold(want, cfg, dt, sin, plan, state, t.pool, flags)
            for s in (rearm or {}).get(k, ()):
                ring, hd = pl.read_score_trace(s, rearm=True)
                same(hd.reshape(1), winfo[s:s + 1], f"tick {k}, scene {s}: the header of a re-arming read is the one before it")
                same(ring, stm.oldest_first(wrings, winfo, s), f"tick {k}, scene {s}: the ring of a re-arming read")
                stm.rearm(winfo, s)
            info, rings = read_all(pl, n)
            same(info, winfo, f"tick {k}: headers")
            for s in range(n):
                same(rings[s], stm.oldest_first(wrings, winfo, s), f"tick {k}, scene {s}: ring")
            got = pl.rollout_score()
            same(got, want, f"tick {k}: RolloutScore")
            res.info.append(info), res.rings.append(rings), res.score.append(got)
        pl.close()
        return res


def batch_ticks(cases):
    """The ticks of single-scene cases laid side by side as the scenes of one batch: pools one behind the other, obs_off moved."""
    ticks = []
    for t in range(len(cases[0])):
        si, pools, at = [], [], 0
        for c in cases:
            s1 = c[t].si.copy()
            s1["obs_off"] += at
            si.append(s1), pools.append(c[t].pool)
            at += len(c[t].pool)
        ticks.append(cb.Tick(np.concatenate(si), np.concatenate(pools)))
    return ticks
