"""Two backends for the episode step with world episodes in force (pp_set_episode_worlds), built on
tests/episode_spawn_backends.py: the numpy model (tests/episode_world_model.py) and the HIP kernel k_respawn_world behind
k_advance_egos / k_advance_route.

A Case is episode_spawn_backends.Case with `worlds` - pp_set_episode_worlds is called (False: the path of §4l on the same script, for
the neutral comparisons) - and `log` - pp_set_episode_log(cap) is called behind it and every Result carries the records read after
its step.  `peers` = K: the fleet of a Case with world_first has max_peers = K (range 60 m) and every scene's slot is K entries wider:
the pinned slices are the laid-out ones - the OWN entries of the clearance walk -, the peer slots behind them are written by
k_couple_fleet / tests/fleet_model.py, and the records an advance reads carry obs_n = own + peers in range (such a Case has one step: the
pool of the staged set is not carried).  `tk`: an EgoTracker set before the records (pp_set_ego_tracker); every Result carries the
EgoTrackState and the model's advance is tests/ego_track_model.py's with age0 from the EpisodeStats the step finds."""
import numpy as np

import advance_backends as ab
import advance_harness as ah
import dmpp_amd as dm
import episode_backends as eb
import episode_model as epm
import episode_spawn_backends as esb
import episode_spawn_model as esm
import episode_world_model as ewm
import ego_track_backends as etb
import fleet_model as fl
import rollout_score_model as rsm


class Case(esb.Case):
    def __init__(self, *args, worlds=True, log=0, peers=0, tk=None, **kw):
        esb.Case.__init__(self, *args, **kw)
        self.worlds, self.log, self.peers, self.tk = worlds, log, peers, None if tk is None else np.array(tk, dm.EgoTracker).reshape(1).copy()
        assert peers == 0 or (self.world_first is not None and len(self.steps) == 1)

    def fleet_model(self):
        fm = dm.default_fleet_model()
        fm["max_peers"], fm["range"] = self.peers, 60.0
        return fm

    def laid_out(self):
        """esb.Case.laid_out with `peers` free entries behind every scene's own ones."""
        W = max(1, max(len(o) for o in self.obs)) + self.peers
        si, pool = self.si.copy(), np.zeros(self.n * W, dm.ObPoint)
        for s, o in enumerate(self.obs):
            pool[s * W:s * W + len(o)] = o
            si["obs_off"][s], si["obs_n"][s] = s * W, len(o)
        return esb.ms.resolve(dm, self.world["map"], si), pool, W

    def own(self):
        """The fleet's pinned slices: (obs_off, n_own) of every scene, or None without a fleet."""
        si = self.laid_out()[0]
        return None if self.world_first is None else (si["obs_off"].copy(), si["obs_n"].copy())

    def start(self):
        """esb.Case.start; with peer slots the resident records and the pool are the coupled ones (pp_set_fleet), which pp_set_episodes captures."""
        si, pool, _ = self.laid_out()
        if self.peers:
            si, pool, _ = fl.couple(self.fleet_model(), self.world_first, *self.own(), si, pool)
        return (si, pool) + self.pools(si) + (epm.new_stats(dm.EpisodeStats, self.n), esm.new_stats(dm.EpisodeSpawnStats, self.n))


def model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags, score=None, track=None):
    """One advance + episode step of the model on records of any origin.  stats / sstats / score are updated in place."""
    if not case.worlds:
        res = esb.model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags, score)
        res.track = None
        return res
    if case.tk is None:
        r = ab.model_step(case.cfg, case.model, si, po, st, flags, case.world, case.route)
    else:                                                 # §4q: a scene whose EpisodeStats.age is 0 re-derives its state
        r = etb.model_step(case.cfg, case.model, case.tk, track, si, po, st, flags, case.world, case.route, age0=stats["age"] == 0)
    out, st2, f, tr, _ = ewm.step(case.em, case.sp, stats, sstats, pin, pst, si, r.out, r.flags, st, pool, 0.5 * float(case.cfg["Vehicle_Width"][0]),
                                  case.world_first, case.own(), r.trace, score)
    if case.peers:                                        # k_couple_fleet behind the episode step: the peers at the restarted poses
        out, _, _ = fl.couple(case.fleet_model(), case.world_first, *case.own(), out, pool)
    res = esb.Result(out, f, tr, st2, stats.copy(), sstats.copy(), None if score is None else score.copy())
    res.track = None if case.tk is None else r.track
    return res


class ModelBackend:
    name = "model"

    def run(self, case):
        n = case.n
        (si, pool, pin, pst, stats, sstats), flags, res = case.start(), np.zeros(n, np.int32), []
        scores = rsm.new_scores(dm.RolloutScore, n) if case.score else None
        dt, track = float(case.model["dt"][0]), np.zeros(n, dm.EgoTrackState)
        for po, st in case.steps:
            if case.score:
                rsm.fold(scores, case.cfg, dt, si, po, st, pool, flags)
            res.append(model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags, scores, track))
            si, flags, track = res[-1].out, res[-1].flags, res[-1].track
        return res


class DeviceBackend:
    name = "device"

    def run(self, case):
        def then(pl):
            if case.peers:
                pl.set_fleet(case.world_first, case.fleet_model())
            else:
                esb.set_worlds(pl, case)
            pl.set_episodes(case.em)
            esb.set_spawn(pl, case)
            if case.worlds:
                pl.set_episode_worlds()
            if case.log:
                pl.set_episode_log(case.log)
        n = case.n
        si, pool, W = case.laid_out()
        pl = ah.open_planner(case.cfg, si, case.world, (pool, W), None, False, case.route, case.state0,
                             first=None if case.tk is None else (lambda pl: pl.set_ego_tracker(case.tk)), then=then, check=not case.peers)
        if case.peers:
            assert pl.get_scene_in().tobytes() == case.start()[0].tobytes(), "the resident records are the crafted ones, coupled"
        if case.score:
            pl.score_begin(float(case.model["dt"][0]))
        trace, res = dm.pinned_empty(n, dm.EgoTrace), []
        for po, st in case.steps:
            ah.inject_advance(pl, case.model, po, st, trace)
            out, f, stats, sstats = pl.get_scene_in(), pl.ego_flags(), pl.episode_stats(), pl.episode_spawn_stats()
            state = pl.get_state()
            sco = pl.rollout_score() if case.score else None
            res.append(esb.Result(out, f, np.array(trace), state, stats, sstats, sco))
            res[-1].track = pl.ego_track_state() if case.tk is not None else None
            if case.log:
                res[-1].records = pl.read_episode_log()[0]
        pl.close()
        return res


class Runner:
    """What a test calls.  On the device every step is also held against the model applied to the device's own records of the step
    before (episode_spawn_backends.compare: every byte but an advanced heading)."""
    def __init__(self, backend):
        self.backend, self.name = backend, backend.name

    def __call__(self, case):
        res = self.backend.run(case)
        si, pool, pin, pst, stats, sstats = case.start()

        def step(k, cur, flags, stats, sstats, track=None):
            return model_step(case, stats, sstats, pin, pst, pool, cur, case.steps[k][0], case.steps[k][1], flags, None, track)
        carried = dict(stats=stats, sstats=sstats)
        if case.tk is not None:
            carried["track"] = np.zeros(case.n, dm.EgoTrackState)
        ah.hold_run(self.name, res, si, step, compare, carried, eb.check_trace)
        return res


def compare(got, want, what):
    """esb.compare, and with a tracker the EgoTrackState fields that are specified to the bit (ego_track_backends.STATE_EXACT)."""
    esb.compare(got, want, what)
    if want.track is not None:
        for name in etb.STATE_EXACT:
            assert got.track[name].tobytes() == want.track[name].tobytes(), f"{what}: EgoTrackState.{name} {got.track[name]} against {want.track[name]}"


def same_bytes(a, b, what, score=False):
    """Two runs of one script, Result by Result: every array, every byte."""
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for name in ("out", "flags", "trace", "state", "stats", "sstats") + (("score",) if score else ()):
            assert np.asarray(getattr(x, name)).tobytes() == np.asarray(getattr(y, name)).tobytes(), f"{what}: step {t}, {name}"
