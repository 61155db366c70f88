"""Two backends for the conflict score, on top of the scorecard backends of coupling_backends.py: the numpy model
tests/conflict_model.py and k_score_ego<., ., true> inside a real tick.

One call takes the configuration, dt_score, the ConflictModel and a list of coupling_backends.Tick; it returns, per tick, the
ConflictScore records and the RolloutScore records.  The device leg is a slice-mode handle on coupling_backends.road, fed every tick's
records and pool through pp_update_async (score_trace_backends.open_planner / feed); a case asserts its known answers as literals on
both legs, and the device's records are held byte for byte against the model stepped over the device's own SceneIn of that tick - and,
in the same run, RolloutScore against the scorecard model: the step changes nothing of it."""
import numpy as np

import conflict_model as cm
import coupling_backends as cb
import dmpp_amd as dm
import rollout_score_model as sm
import score_trace_backends as stb

same = stb.same
batch_ticks = stb.batch_ticks


class ConflictResult:
    """conf[k], score[k]: behind tick k; start: the ConflictScore records before the first tick."""
    def __init__(self):
        self.start, self.conf, self.score = None, [], []


def _model(m):
    return np.array(m, dm.ConflictModel).reshape(1).copy()


class ModelBackend:
    name = "model"

    def run(self, cfg, dt, model, ticks, ep_stats=None):
        """ep_stats: per tick an EpisodeStats array or None (episodes off) - model leg only."""
        model, n = _model(model), len(ticks[0].si)
        scores, conf, prev = sm.new_scores(dm.RolloutScore, n), cm.new_scores(dm.ConflictScore, n), cm.new_prev(dm.ObPoint)
        res = ConflictResult()
        res.start = conf.copy()
        for k, t in enumerate(ticks):
            po, st, flags = cb._crafted(t)
            prev = cm.step(conf, prev, model, cfg, dt, t.si, t.pool, None if ep_stats is None else ep_stats[k])
            sm.fold(scores, cfg, dt, t.si, po, st, t.pool, flags)
            res.conf.append(conf.copy()), res.score.append(scores.copy())
        return res


def open_planner(cfg, ticks, model=None, score=True, dt=0.5):
    """score_trace_backends.open_planner without a trace; model None: the conflict score is never set."""
    pl = stb.open_planner(cfg, ticks, None, False, dt)
    if model is not None:
        pl.set_conflict_score(_model(model))
    if score:
        pl.score_begin(dt)
    return pl


class DeviceBackend:
    name = "device"

    def run(self, cfg, dt, model, ticks, ep_stats=None):
        assert ep_stats is None, "episodes on the device: the closed loops"
        assert not int(cfg["grid_stage"][0]) and not int(cfg["decision_stage"][0]) and not int(cfg["dynamic_obstacles"][0])
        model, n = _model(model), len(ticks[0].si)
        pl = open_planner(cfg, ticks, model, True, dt)
        want, wconf, prev = sm.new_scores(dm.RolloutScore, n), cm.new_scores(dm.ConflictScore, n), cm.new_prev(dm.ObPoint)
        res, keep = ConflictResult(), []
        res.start = pl.conflict_score()
        same(res.start, wconf, "before the first tick")
        for k, t in enumerate(ticks):
            sin, plan, state = stb.feed(pl, t, keep)
            flags = pl.ego_flags()
            prev = cm.step(wconf, prev, model, cfg, dt, sin, t.pool)
            sm.fold(want, cfg, dt, sin, plan, state, t.pool, flags)
            got, score = pl.conflict_score(), pl.rollout_score()
            same(got, wconf, f"tick {k}: ConflictScore")
            same(score, want, f"tick {k}: RolloutScore")
            res.conf.append(got), res.score.append(score)
        pl.close()
        return res
