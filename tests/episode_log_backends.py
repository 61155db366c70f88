"""Two backends for the episode log (pp_set_episode_log), built on episode_backends.py and - for the Case, which also
carries a spawn model - on episode_spawn_backends.py: the numpy model (tests/episode_log_model.py behind the episode models) and the
HIP kernel k_log_episodes behind k_respawn_egos / k_respawn_spawn.

A run takes an episode_spawn_backends.Case, the ring's capacity and when to drain: after every advance (`each`) or once behind the
last (`end`); with `max_records` every drain is two reads - one of at most max_records, one of the rest.  It returns a Run: per
advance the Data the log step reads (the SceneIn records and flag words the advance read, EpisodeStats and EpisodeSpawnStats
behind it, the tick id, and - scored runs - the PlanOut and SceneState of the tick, which the scorecard folded), the (total,
lost_total) pair behind every advance and the reads in the order they were made, each (records, n_lost).

`replay` is the model of the log alone, applied to such Data of any origin: the model backend feeds it the episode models' records,
and `Runner` holds every read of the device against the replay of the device's OWN per-advance records, byte for byte - the
scorecard included, since the device's records carry the tick's own PlanOut (episode_backends.py on what a crafted PlanOut cannot do)."""
import numpy as np

import advance_backends as ab          # (tests reach ab._route through this module)
import advance_harness as ah
import dmpp_amd as dm
import episode_log_model as elm
import episode_spawn_backends as esb
import episode_spawn_model as esm

Case = esb.Case


class Data:
    def __init__(self, prev_in, prev_flags, stats, sstats, tick, pool, plan=None, state=None):
        self.prev_in, self.prev_flags, self.stats, self.sstats, self.tick, self.pool = prev_in, prev_flags, stats, sstats, tick, pool
        self.plan, self.state = plan, state


class Run:
    def __init__(self, data, infos, reads):
        self.data, self.infos, self.reads = data, infos, reads

    @property
    def records(self):
        """Every record read, in the order of the reads."""
        return np.concatenate([r for r, _ in self.reads]) if self.reads else np.zeros(0, dm.EpisodeRecord)


def _drain(read, drain, last, max_records):
    if drain == "each" or last:
        return [read(max_records)] + ([read(None)] if max_records is not None else [])
    return []


def replay(case, cap, data, drain="each", max_records=None):
    """(infos, reads) of the log model on the per-advance Data."""
    log = elm.EpisodeLog(dm.EpisodeRecord, case.n, cap, None if case.sp is None else np.zeros(case.n, np.int32), case.score)
    dt, infos, reads = float(case.model["dt"][0]), [], []
    for k, d in enumerate(data):
        if case.score:
            log.fold(case.cfg, dt, d.prev_in, d.plan, d.state, d.pool, d.prev_flags)
        log.append(d.stats, d.prev_in, d.tick, None if case.sp is None else d.sstats)
        infos.append(log.info())
        reads += _drain(log.read, drain, k == len(data) - 1, max_records)
    return infos, reads


class ModelBackend:
    name = "model"

    def run(self, case, cap, drain="each", max_records=None):
        n = case.n
        (si, pool, pin, pst, stats, sstats), flags, data = case.start(), np.zeros(n, np.int32), []
        for k, (po, st) in enumerate(case.steps):
            r = esb.model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags)
            data.append(Data(si, flags, r.stats, r.sstats, k + 1, pool, po, st))
            si, flags = r.out, r.flags
        return Run(data, *replay(case, cap, data, drain, max_records))


def open_planner(case, cap=None):
    """The set-up of episode_spawn_backends.DeviceBackend, then - last - pp_set_episode_log.  Returns (planner, SceneIn, pool)."""
    def then(pl):
        pl.set_episodes(case.em)
        if case.sp is not None:
            esb.set_spawn(pl, case)
        if case.score:
            pl.score_begin(float(case.model["dt"][0]))
        if cap is not None:
            pl.set_episode_log(cap)
    return esb.open_case(case, then, check=False)[:3]


def advance(pl, case, po, st, si, flags, pool):
    """One tick and one advance on crafted PlanOut / SceneState records (advance_harness.inject_advance).  Returns (the Data of the
    advance, the staged SceneIn records, the flag words)."""
    seen = dict(plan=None, state=None)
    folded = (lambda pl: seen.update(plan=pl.get_plan(), state=pl.get_state())) if case.score else None      # what the scorecard folded: the tick's own
    ah.inject_advance(pl, case.model, po, st, after_tick=folded, before_advance=lambda pl: seen.update(tick=pl.tick_id()))
    sstats = pl.episode_spawn_stats() if case.sp is not None else esm.new_stats(dm.EpisodeSpawnStats, case.n)
    return Data(si, flags, pl.episode_stats(), sstats, seen["tick"], pool, seen["plan"], seen["state"]), pl.get_scene_in(), pl.ego_flags()


class DeviceBackend:
    name = "device"

    def run(self, case, cap, drain="each", max_records=None):
        pl, si, pool = open_planner(case, cap)
        flags, data, infos, reads = np.zeros(case.n, np.int32), [], [], []
        for k, (po, st) in enumerate(case.steps):
            d, si, flags = advance(pl, case, po, st, si, flags, pool)
            data.append(d)
            infos.append(pl.episode_log_info())
            reads += _drain(pl.read_episode_log, drain, k == len(case.steps) - 1, max_records)
        pl.close()
        return Run(data, infos, reads)


def same_reads(got, want, what):
    assert len(got) == len(want), what
    for k, ((g, gl), (w, wl)) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and len(g) == len(w) and gl == wl, f"{what}, read {k}: {len(g)} records and {gl} lost against {len(w)} and {wl}"
        assert g.tobytes() == w.tobytes(), f"{what}, read {k}: fields " + ", ".join(f for f in g.dtype.names if g[f].tobytes() != w[f].tobytes())


class Runner:
    """What a known answer calls.  On the device every read and every (total, lost_total) pair is also held against the replay of the
    device's own per-advance records."""
    def __init__(self, backend):
        self.backend, self.name = backend, backend.name

    def __call__(self, case, cap, drain="each", max_records=None):
        run = self.backend.run(case, cap, drain, max_records)
        if self.name == "device":
            infos, reads = replay(case, cap, run.data, drain, max_records)
            assert run.infos == infos, f"(total, lost_total): {run.infos} against {infos}"
            same_reads(run.reads, reads, "device against the model on its own records")
        return run
