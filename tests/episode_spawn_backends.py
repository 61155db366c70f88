"""Two backends for the episode step with the spawn model in force (pp_set_episode_spawn), in the spirit of
episode_backends.py, on which this builds: the numpy model (tests/episode_spawn_model.py behind tests/ego_model.py /
tests/route_model.py) and the HIP kernel k_respawn_spawn behind k_advance_egos / k_advance_route.

A known answer is written once against `Runner` and asserted on both.  One call takes a Case: the configuration, the ego model,
the episode model, the spawn model (None: pp_set_episode_spawn is not called - the path of §4k), N SceneIn records with obs_n
obstacles each (`obs`: a list of N ObPoint arrays; obs_off is laid out by the backend, one slot of equal width per scene), the
SceneState the episodes start from, the steps - each the PlanOut[N] and SceneState[N] one advance reads -, the map, an optional
route, the start records 1 .. M - 1 (`starts`: (SceneIn[(M - 1) N], SceneState[(M - 1) N]), record k of scene s at (k - 1) N + s)
and the fleet's world_first (a fleet of max_peers = 0: worlds only, no peer slots).  It returns one Result per step: what
episode_backends.Result holds and the EpisodeSpawnStats.  PlanOut and SceneState are injected on the device as there."""
import numpy as np

import advance_backends as ab
import advance_harness as ah
import dmpp_amd as dm
import episode_backends as eb
import episode_model as epm
import episode_spawn_model as esm
import map_scenes as ms
import rollout_score_model as rsm


class Case:
    def __init__(self, cfg, model, em, sp, si, obs, state0, steps, world, route=None, starts=None, world_first=None, score=False):
        self.cfg, self.model, self.em, self.sp, self.si, self.obs, self.state0 = cfg, model, em, sp, si, obs, state0
        self.steps, self.world, self.route, self.starts, self.world_first, self.score = steps, world, route, starts, world_first, score
        assert len(obs) == len(si)

    @property
    def n(self):
        return len(self.si)

    @property
    def M(self):
        return 1 if self.sp is None else int(self.sp["n_starts"][0])

    def laid_out(self):
        """(SceneIn with obs_off / obs_n set, the obstacle pool, the slot width): scene s owns pool[s W : (s + 1) W]."""
        W = max(1, max(len(o) for o in self.obs))
        si, pool = self.si.copy(), np.zeros(self.n * W, dm.ObPoint)
        for s, o in enumerate(self.obs):
            pool[s * W:s * W + len(o)] = o
            si["obs_off"][s], si["obs_n"][s] = s * W, len(o)
        return ms.resolve(dm, self.world["map"], si), pool, W

    def start(self):
        """What a model run starts from: (SceneIn laid out, the obstacle pool, the start records of pools(), EpisodeStats and
        EpisodeSpawnStats before the first step)."""
        si, pool, _ = self.laid_out()
        return (si, pool) + self.pools(si) + (epm.new_stats(dm.EpisodeStats, self.n), esm.new_stats(dm.EpisodeSpawnStats, self.n))

    def pools(self, si):
        """The start records as §4l prepares them: record 0 the capture, the others resolved on the map with record 0's slice."""
        pin, pst = [si], [self.state0]
        for k in range(1, self.M):
            r = ms.resolve(dm, self.world["map"], self.starts[0][(k - 1) * self.n:k * self.n])
            r["obs_off"], r["obs_n"] = si["obs_off"], si["obs_n"]
            pin.append(r), pst.append(self.starts[1][(k - 1) * self.n:k * self.n])
        return pin, pst


class Result(eb.Result):
    def __init__(self, out, flags, trace, state, stats, sstats, score=None):
        eb.Result.__init__(self, out, flags, trace, state, stats, score)
        self.sstats = sstats


def neutral(dtype):
    """The spawn model that changes nothing (§4l): M = 1, contact 0, check 0."""
    sp = np.zeros(1, dtype)
    sp["seed"], sp["clearance"], sp["n_starts"] = 1, 0.0, 1
    return sp


def model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags, score=None):
    """One advance + episode step of the model on records of any origin.  stats / sstats / score are updated in place."""
    r = ab.model_step(case.cfg, case.model, si, po, st, flags, case.world, case.route)
    if case.sp is None:
        out, st2, f, tr, _ = epm.step(case.em, stats, pin[0], pst[0], si, r.out, r.flags, st, r.trace, score)
    else:
        out, st2, f, tr, _ = esm.step(case.em, case.sp, stats, sstats, pin, pst, si, r.out, r.flags, st, pool, 0.5 * float(case.cfg["Vehicle_Width"][0]),
                                      case.world_first, r.trace, score)
    return Result(out, f, tr, st2, stats.copy(), sstats.copy(), None if score is None else score.copy())


class ModelBackend:
    name = "model"

    def run(self, case):
        n = case.n
        (si, pool, pin, pst, stats, sstats), flags, res = case.start(), np.zeros(n, np.int32), []
        scores = rsm.new_scores(dm.RolloutScore, n) if case.score else None
        dt = float(case.model["dt"][0])
        for po, st in case.steps:
            if case.score:
                rsm.fold(scores, case.cfg, dt, si, po, st, pool, flags)
            res.append(model_step(case, stats, sstats, pin, pst, pool, si, po, st, flags, scores))
            si, flags = res[-1].out, res[-1].flags
        if case.score:
            rsm.fold(scores, case.cfg, dt, si, case.steps[-1][0], case.steps[-1][1], pool, flags)
            res[-1].final_score = scores.copy()
        return res


def open_case(case, then, mot_pool=None, check=True):
    """advance_harness.open_planner for a Case - its laid-out records and obstacle slots, route and start state - with the feature
    set calls `then(pl)` behind them; a motion pool makes the input sets carry one.  Returns (handle, SceneIn, obstacle pool, slot width)."""
    si, pool, W = case.laid_out()
    return ah.open_planner(case.cfg, si, case.world, (pool, W), mot_pool, mot_pool is not None, case.route, case.state0, then=then, check=check), si, pool, W


def set_worlds(pl, case):
    """The fleet of a Case with world_first: worlds only, no peer slots."""
    if case.world_first is not None:
        fm = dm.default_fleet_model()
        fm["max_peers"] = 0
        pl.set_fleet(case.world_first, fm)


def set_spawn(pl, case):
    pl.set_episode_spawn(case.sp, *(case.starts if case.starts is not None else (None, None)))


class DeviceBackend:
    name = "device"

    def run(self, case):
        def then(pl):
            set_worlds(pl, case)
            pl.set_episodes(case.em)
            if case.sp is not None:
                set_spawn(pl, case)
        n = case.n
        pl = open_case(case, then)[0]
        if case.score:
            pl.score_begin(float(case.model["dt"][0]))
        trace, res = dm.pinned_empty(n, dm.EgoTrace), []
        for po, st in case.steps:
            ah.inject_advance(pl, case.model, po, st, trace)
            out, f, stats = pl.get_scene_in(), pl.ego_flags(), pl.episode_stats()
            sstats = pl.episode_spawn_stats() if case.sp is not None else esm.new_stats(dm.EpisodeSpawnStats, n)
            state = pl.get_state()                        # behind the staged advance: the restored state
            sco = pl.rollout_score() if case.score else None
            res.append(Result(out, f, np.array(trace), state, stats, sstats, sco))
        if case.score:
            pl.tick()
            res[-1].final_score = pl.rollout_score()
        pl.close()
        return res


def compare(got, want, what):
    """episode_backends.compare - SceneIn, flags, trace, SceneState, EpisodeStats byte for byte, the heading of an ADVANCED record
    within 1e-6 degrees - and the EpisodeSpawnStats byte for byte."""
    eb.compare(got, want, what)
    assert got.sstats.tobytes() == want.sstats.tobytes(), f"{what}: EpisodeSpawnStats {got.sstats.tolist()} against {want.sstats.tolist()}"


class Runner:
    """What a known answer calls.  On the device every step is also held against the model applied to the device's own records
    of the step before (compare), and every call is logged for batched()."""
    def __init__(self, backend, log=None):
        self.backend, self.name, self.log = backend, backend.name, log

    def __call__(self, case, log=True):
        res = self.backend.run(case)
        si, pool, pin, pst, stats, sstats = case.start()

        def step(k, cur, flags, stats, sstats):
            return model_step(case, stats, sstats, pin, pst, pool, cur, case.steps[k][0], case.steps[k][1], flags)
        ah.hold_run(self.name, res, si, step, compare, dict(stats=stats, sstats=sstats), eb.check_trace)
        if self.log is not None and log:
            assert case.n == 1 and not case.score and case.world_first is None
            self.log.append(ah.Call(case, res))
        return res


def _same_launch(a, b):
    return eb._same_launch(a, b) and (a.sp is None) == (b.sp is None) and (a.sp is None or a.sp.tobytes() == b.sp.tobytes())


def joined(cases):
    """(SceneIn, obs, state0, steps, route, starts) of one-scene cases as the scenes of one Case."""
    M = cases[0].M
    starts = None if M == 1 else tuple(np.concatenate([c.starts[i][k - 1:k] for k in range(1, M) for c in cases]) for i in (0, 1))
    return (np.concatenate([c.si for c in cases]), [c.obs[0] for c in cases], np.concatenate([c.state0 for c in cases]), ah.join_steps(cases),
            ah.join_routes([c.route for c in cases]), starts)


def batched(log, sizes=(5, 9)):
    """Every logged single-scene call again, as distinct scenes of one launch (episode_backends.batched): the calls that can share
    a launch form a group, each group runs in batches of every size of `sizes` with a scene that ENDS an episode first, last and on
    either side of the block edge 4 | 5 where the group has both kinds.  The hashed start choice of §4l depends on the scene index,
    so a batch is held against the MODEL run on the same batch (compare: every byte but an advanced heading); a scene whose
    choice does not depend on its index (M = 1 or round robin) must also give the bytes it gave alone.  Returns (size, indices of
    the ending scenes) per batch."""
    ran = []
    for n, batch, at in ah.batches(log, _same_launch, ah.ends_episode, sizes):
        c0 = batch[0].case
        si, obs, state0, steps, route, starts = joined([c.case for c in batch])
        big = Case(c0.cfg, c0.model, c0.em, c0.sp, si, obs, state0, steps, c0.world, route, starts)
        got, want = DeviceBackend().run(big), ModelBackend().run(big)
        W = big.laid_out()[2]
        for t, (r, w) in enumerate(zip(got, want)):
            compare(r, w, f"batch of {n}, step {t}")
            if c0.sp is None or c0.M == 1 or int(c0.sp["order"][0]) != 0:
                ah.same_alone(r, t, batch, ("out", "flags", "trace", "state", "stats", "sstats"), obs_width=W)
        ran.append((n, at))
    return ran
