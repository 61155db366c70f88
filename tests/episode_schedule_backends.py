"""Two backends for the episode step with a scenario schedule in force (pp_set_episode_schedule), built on
tests/episode_spawn_backends.py: the numpy model (tests/episode_schedule_model.py on top of tests/episode_spawn_model.py) and the
HIP kernels k_respawn_sched / k_fold_schedule behind k_advance_egos / k_advance_route.

A Case is an episode_spawn_backends.Case with the schedule `sm` (None: pp_set_episode_schedule is not called - k_respawn_spawn
runs).  A Result is what episode_spawn_backends.Result holds and the EpisodeScheduleRow records behind the advance."""
import numpy as np

import advance_backends as ab
import dmpp_amd as dm
import episode_model as epm
import episode_schedule_model as evm
import episode_spawn_backends as esb
import episode_spawn_model as esm


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
        si, pool, _ = case.laid_out()
        pin, pst = case.pools(si)
        rows, stats, sstats, flags, res = _rows(case), epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n), np.zeros(n, np.int32), []
        for po, st in case.steps:
            res.append(model_step(case, rows, stats, sstats, pin, pst, pool, si, po, st, flags))
            si, flags = res[-1].out, res[-1].flags
        return res


def planner(case):
    """A handle with everything of the Case in force, the schedule last; and the resident records."""
    n, m = case.n, case.world["map"]
    si, pool, W = case.laid_out()
    sc = dict(scene_in=si, obs_pool=pool, mot_pool=None, n_obs=W)
    pl = dm.Planner(case.cfg, device=0, max_scenes=n, max_obs_total=len(pool), max_lane_pts_total=len(m["points"]), max_ref_pts_total=max(len(m["jpoints"]), 1))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    if case.route is not None:
        legs, rf, rm = ab._route(case.route, n)
        pl.set_route(legs, rf, rm)
    pl.set_state(case.state0)
    if case.world_first is not None:
        fm = dm.default_fleet_model()
        fm["max_peers"] = 0
        pl.set_fleet(case.world_first, fm)
    pl.set_episodes(case.em)
    pl.set_episode_spawn(case.sp, *(case.starts if case.starts is not None else (None, None)))
    if case.sm is not None:
        pl.set_episode_schedule(case.sm)
    return pl, si


class DeviceBackend:
    name = "device"

    def run(self, case, light=False):
        """light: only flags, stats and rows are fetched per step (the big batches)."""
        assert not case.score
        n = case.n
        pl, si = planner(case)
        if not light:
            assert pl.get_scene_in().tobytes() == si.tobytes(), "the resident records are the crafted ones (views resolved, slices inside the pools)"
        trace, res = dm.pinned_empty(n, dm.EgoTrace), []
        for po, st in case.steps:
            pl.tick()                                     # the tick an advance follows; what it wrote is replaced below
            pl.write_device(dm.BUF_PLAN_OUT, po)
            pl.write_device(dm.BUF_STATE, st)
            pl.advance_async(case.model, trace)
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
        if self.name != "device":
            return res
        n = case.n
        si, pool, _ = case.laid_out()
        pin, pst = case.pools(si)
        cur, flags, rows, stats, sstats = si, np.zeros(n, np.int32), _rows(case), epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n)
        for k, r in enumerate(res):
            if k:
                rows, stats, sstats = res[k - 1].rows.copy(), res[k - 1].stats.copy(), res[k - 1].sstats.copy()
            compare(r, model_step(case, rows, stats, sstats, pin, pst, pool, cur, case.steps[k][0], case.steps[k][1], flags), f"step {k}")
            cur, flags = r.out, r.flags
        return res
