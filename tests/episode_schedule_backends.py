"""Two backends for the episode step with a scenario schedule in force (pp_set_episode_schedule), built on
tests/episode_spawn_backends.py: the numpy model (tests/episode_schedule_model.py on top of tests/episode_spawn_model.py) and the
HIP kernels k_respawn_sched / k_fold_schedule behind k_advance_egos / k_advance_route.

A Case is an episode_spawn_backends.Case with the schedule `sm` (None: pp_set_episode_schedule is not called - k_respawn_spawn
runs).  A Result is what episode_spawn_backends.Result holds and the EpisodeScheduleRow records behind the advance."""
import numpy as np

import advance_backends as ab
import advance_harness as ah
import dmpp_amd as dm
import episode_schedule_model as evm
import episode_spawn_backends as esb


class Case(esb.Case):
    def __init__(self, sm, *args, **kw):
        esb.Case.__init__(self, *args, **kw)
        self.sm = sm


class Result(esb.Result):
    def __init__(self, r, rows):
        esb.Result.__init__(self, r.out, r.flags, r.trace, r.state, r.stats, r.sstats, r.score)
        self.rows = rows


def model_step(case, rows, stats, sstats, pin, pst, pool, si, po, st, flags):
    """One advance + episode step of the model on records of any origin.  rows / stats / sstats are updated in place."""
    if case.sm is None:
        return Result(esb.model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags), rows.copy())
    r = ab.model_step(case.cfg, case.model, si, po, st, flags, case.world, case.route)
    out, st2, f, tr, _ = evm.step(case.em, case.sp, case.sm, rows, stats, sstats, pin, pst, si, r.out, r.flags, st, pool, 0.5 * float(case.cfg["Vehicle_Width"][0]),
                                  case.world_first, r.trace)
    return Result(esb.Result(out, f, tr, st2, stats.copy(), sstats.copy()), rows.copy())


def _rows(case):
    return np.zeros(1, dm.EpisodeScheduleRow) if case.sm is None else evm.new_rows(dm.EpisodeScheduleRow, case.sm, case.n)


class ModelBackend:
    name = "model"

    def run(self, case):
        assert not case.score
        n = case.n
        (si, pool, pin, pst, stats, sstats), rows, flags, res = case.start(), _rows(case), np.zeros(n, np.int32), []
        for po, st in case.steps:
            res.append(model_step(case, rows, stats, sstats, pin, pst, pool, si, po, st, flags))
            si, flags = res[-1].out, res[-1].flags
        return res


class DeviceBackend:
    name = "device"

    def run(self, case, light=False):
        """light: only flags, stats and rows are fetched per step (the big batches)."""
        def then(pl):                                     # everything of the Case in force, the schedule last
            esb.set_worlds(pl, case)
            pl.set_episodes(case.em)
            esb.set_spawn(pl, case)
            if case.sm is not None:
                pl.set_episode_schedule(case.sm)
        assert not case.score
        n = case.n
        pl = esb.open_case(case, then, check=not light)[0]
        trace, res = dm.pinned_empty(n, dm.EgoTrace), []
        for po, st in case.steps:
            ah.inject_advance(pl, case.model, po, st, trace)
            f, stats, sstats = pl.ego_flags(), pl.episode_stats(), pl.episode_spawn_stats()
            out, state = (None, None) if light else (pl.get_scene_in(), pl.get_state())
            rows = pl.episode_schedule() if case.sm is not None else np.zeros(1, dm.EpisodeScheduleRow)
            res.append(Result(esb.Result(out, f, np.array(trace), state, stats, sstats), rows))
        pl.close()
        return res


def compare(got, want, what):
    """episode_spawn_backends.compare - all of Result, byte for byte but the heading of an ADVANCED record - and the rows."""
    esb.compare(got, want, what)
    assert got.rows.tobytes() == want.rows.tobytes(), f"{what}: rows {got.rows.tolist()} against {want.rows.tolist()}"


class Runner:
    """What a known answer calls.  On the device every step is also held against the model applied to the device's own records of
    the step before."""
    def __init__(self, backend):
        self.backend, self.name = backend, backend.name

    def __call__(self, case):
        res = self.backend.run(case)
        si, pool, pin, pst, stats, sstats = case.start()

        def step(k, cur, flags, rows, stats, sstats):
            return model_step(case, rows, stats, sstats, pin, pst, pool, cur, case.steps[k][0], case.steps[k][1], flags)
        ah.hold_run(self.name, res, si, step, compare, dict(rows=_rows(case), stats=stats, sstats=sstats))
        return res
