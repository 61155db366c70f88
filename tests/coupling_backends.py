"""Two backends each for the two kernels that couple an ego to what is around it, in the spirit of advance_backends.py:

  the scorecard's front half (k_score_ego)  - numpy model tests/rollout_score_model.py
  the fleet coupling step   (k_couple_fleet)         - numpy model tests/fleet_model.py

A known answer is written once against ScoreRunner / FleetRunner and asserted on both backends.  Both specifications fix every
field to the last bit and the build has -ffp-contract=off: there is no tolerance anywhere in this file.

Scorecard.  One call takes the configuration, dt_score and a list of ticks - each the SceneIn[N] records and the obstacle pool the
tick reads - and returns the RolloutScore[N] records before the first tick and after every tick.  The model folds a crafted PlanOut /
SceneState (zero but for the counters a Tick names).  The device cannot be handed a PlanOut in front of k_score_ego - the kernel runs
inside the tick, behind the Planning kernel - so its leg is a slice-mode handle on the straight road of
lanechange_scenes.make_scene (grid stage, decision stage and moving obstacles off) that is fed every tick's records and pool through
pp_update_async; what follows from the crafted inputs alone (clearance, collisions, distance, speeds, n_ticks - and behavior_ticks,
since with the decision stage off PlanOut.dec is the caller's record) a case asserts as literals on both backends, and the WHOLE
record is held byte for byte against the model folded over the device's own PlanOut and SceneState of that tick.

Fleet.  One call takes the FleetModel, world_first, the positions of N egos, the own entries per scene and whether the set carries a
motion pool; it returns the SceneIn records, the whole obstacle pool and the whole motion pool after the step.  Every pool byte is
0x5A before it, so an untouched slot still holds that.  The device leg is pp_set_scenes + pp_set_fleet on the resident set (no
tick); SceneIn, every slice (pp_get_obstacles) and both pools (Planner.read_device: after pp_set_fleet PP_BUF_OBS_POOL /
PP_BUF_MOT_POOL are the pools of the set pp_get_scene_in reads) are held byte for byte against the model.

batched(): every logged single-scene scorecard call / every logged fleet call again as distinct scenes / worlds of one launch."""
import numpy as np

import dmpp_amd as dm
import fleet_model as fl
import rollout_score_model as sm

FILL = 0x5A          # every byte of the fleet runner's pools before the step


# ===============================================================================================================
# the road both device legs stand on
_ROAD = {}


def road(cfg):
    """lanechange_scenes.make_scene: three straight lanes, the ego's record with DecisionOut as test_known_answer_speed_ramp sets it."""
    if not _ROAD:
        import lanechange_scenes as lcs
        sc = lcs.make_scene(dm, cfg, lane_num=2, obstacles=())
        d = sc["scene_in"]["dec"]
        d["velocity_expect"], d["behavior"], d["target_lanenum"] = 30.0, 1, 2
        _ROAD.update(sc)
    return _ROAD


def config():
    """default_config(128) with the grid stage, the decision stage and moving obstacles off."""
    cfg = dm.default_config(128)
    cfg["grid_stage"], cfg["decision_stage"], cfg["dynamic_obstacles"] = 0, 0, 0
    return cfg


def _set_scenes(pl, sc, si, obs, mot, n_obs_total):
    rc = pl.lib.pp_set_scenes(pl.h, len(si), si.ctypes.data, sc["lane_pool"].ctypes.data, sc["attr_pool"].ctypes.data, len(sc["lane_pool"]),
                              sc["ref_pool"].ctypes.data, len(sc["ref_pool"]), obs.ctypes.data, None if mot is None else mot.ctypes.data, n_obs_total)
    assert rc == 0, pl.lib.pp_last_error()
    pl.n = len(si)


# ===============================================================================================================
# scorecard
class Tick:
    """One scored tick: SceneIn[N], the obstacle pool it reads, and what only a crafted PlanOut / SceneState / GridOut can say (model
    leg only): afresh_planning, ob_flag, desaccVd, the ego flag word, GridOut.  The behaviour is si.dec.behavior on both legs."""
    def __init__(self, si, pool, afresh=0, ob_flag=0, desaccVd=0, flags=0, grid=None):
        self.si, self.pool, self.afresh, self.ob_flag, self.desaccVd, self.flags, self.grid = si, pool, afresh, ob_flag, desaccVd, flags, grid


def tick(cfg, egos, behavior=1, lead=0, **kw):
    """egos: (x, y, v, obstacles) per scene, obstacles (x, y, radius).  The slices lie one behind the other, `lead` entries in front of
    each of them that belong to nobody: discs of radius 1000 on the ego (whoever reads one of them reports a deep collision)."""
    n = len(egos)
    si = np.repeat(road(cfg)["scene_in"][:1], n)
    total = sum(lead + len(e[3]) for e in egos)
    pool = np.zeros(max(total, 1), dm.ObPoint)
    at = 0
    for k, (x, y, v, obs) in enumerate(egos):
        pool[at:at + lead]["x"], pool[at:at + lead]["y"], pool[at:at + lead]["radius"] = x, y, 1000.0
        at += lead
        g = si[k]["loc"]
        g["globalpoint"]["x"], g["globalpoint"]["y"], g["velocity"] = x, y, v
        si[k]["obs_off"], si[k]["obs_n"], si[k]["dec"]["behavior"] = at, len(obs), behavior
        for j, (ox, oy, r) in enumerate(obs):
            pool[at + j]["x"], pool[at + j]["y"], pool[at + j]["radius"] = ox, oy, r
        at += len(obs)
    return Tick(si, pool, **kw)


class ScoreResult:
    """start: the records before the first tick; after[k]: after tick k."""
    def __init__(self, start, after):
        self.start, self.after = start, after


def _crafted(t):
    """The PlanOut / SceneState the model leg folds for a tick: zero but for the counters."""
    n = len(t.si)
    po, st = np.zeros(n, dm.PlanOut), np.zeros(n, dm.SceneState)
    po["dec"]["behavior"], po["ob_flag"], po["result"]["desaccVd"], st["afresh_planning"] = t.si["dec"]["behavior"], t.ob_flag, t.desaccVd, t.afresh
    return po, st, np.full(n, t.flags, np.int32)


class ScoreModelBackend:
    name = "model"

    def run(self, cfg, dt, ticks):
        r = sm.new_scores(dm.RolloutScore, len(ticks[0].si))
        start, after = r.copy(), []
        for t in ticks:
            po, st, flags = _crafted(t)
            sm.fold(r, cfg, dt, t.si, po, st, t.pool, flags, t.grid)
            after.append(r.copy())
        return ScoreResult(start, after)


def _same(a, b, what):
    assert a.tobytes() == b.tobytes(), what + ": " + ", ".join(f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes())


class ScoreDeviceBackend:
    name = "device"

    def run(self, cfg, dt, ticks):
        assert not int(cfg["grid_stage"][0]) and not int(cfg["decision_stage"][0]) and not int(cfg["dynamic_obstacles"][0])
        sc, n = road(cfg), len(ticks[0].si)
        cap = max(len(t.pool) for t in ticks)
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=cap, max_lane_pts_total=len(sc["lane_pool"]), max_ref_pts_total=len(sc["ref_pool"]))
        first = np.zeros(cap, dm.ObPoint)
        first[:len(ticks[0].pool)] = ticks[0].pool
        _set_scenes(pl, sc, ticks[0].si, first, None, cap)
        pl.set_state(np.repeat(sc["state"][:1], n))
        pl.score_begin(dt)
        want = sm.new_scores(dm.RolloutScore, n)
        start = pl.rollout_score()
        _same(start, want, "before the first tick")
        plan_p, after, keep, flags = dm.pinned_empty(n, dm.PlanOut), [], [], np.zeros(n, np.int32)
        for k, t in enumerate(ticks):
            in_t, obs_t = dm.pinned_copy(t.si), dm.pinned_copy(t.pool)
            keep.append((in_t, obs_t))
            pl.update_async(in_t, obs_t)
            pl.tick()
            assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
            sin = pl.get_scene_in()
            assert sin.tobytes() == t.si.tobytes(), f"tick {k}: the tick read the crafted records (every slice inside its pool)"
            sm.fold(want, cfg, dt, sin, np.array(plan_p), pl.get_state(), t.pool, flags)
            got = pl.rollout_score()
            _same(got, want, f"tick {k}")
            after.append(got)
        pl.close()
        return ScoreResult(start, after)


class ScoreRunner:
    """What a scorecard case calls; single-scene calls are logged for score_batched()."""
    def __init__(self, backend, log=None):
        self.backend, self.name, self.log = backend, backend.name, log

    def __call__(self, cfg, dt, ticks):
        res = self.backend.run(cfg, dt, ticks)
        if self.log is not None and len(ticks[0].si) == 1:
            self.log.append(dict(cfg=cfg.copy(), dt=dt, ticks=ticks, res=res))
        return res


def score_batched(backend, log, min_scenes=5):
    """Every logged single-scene call again as distinct scenes of one launch per group of calls that can share one (configuration,
    dt_score, number of ticks): at least `min_scenes` scenes and never a multiple of four (the first calls are repeated to get
    there), so the last block is partial and the waves of a block have different trip counts.  The pools of a tick are laid one
    behind the other and obs_off moved.  Every scene must give the bytes it gave alone.  Returns the batch sizes."""
    groups = {}
    for c in log:
        groups.setdefault((c["cfg"].tobytes(), c["dt"], len(c["ticks"])), []).append(c)
    sizes = []
    for cases in groups.values():
        cases, k = list(cases), 0
        while len(cases) < min_scenes or len(cases) % 4 == 0:
            cases.append(cases[k])
            k += 1
        ticks = []
        for t in range(len(cases[0]["ticks"])):
            si, pools, at = [], [], 0
            for c in cases:
                ct = c["ticks"][t]
                s1 = ct.si.copy()
                s1["obs_off"] += at
                si.append(s1), pools.append(ct.pool)
                at += len(ct.pool)
            ticks.append(Tick(np.concatenate(si), np.concatenate(pools)))
        res = backend.run(cases[0]["cfg"], cases[0]["dt"], ticks)
        for t, got in enumerate(res.after):
            for k, c in enumerate(cases):
                _same(got[k:k + 1], c["res"].after[t], f"batch of {len(cases)}, scene {k}, tick {t}")
        sizes.append(len(cases))
    return sizes


# ===============================================================================================================
# fleet
class FleetResult:
    """out: SceneIn after the step; pool / mot: the whole pools after it (mot None without a motion pool); off / own: the pinned
    slices; si / pool_in: what went in (model leg: obs_off / obs_n of `si` are rubbish, the step must overwrite them)."""
    def __init__(self, out, pool, mot, off, own, si, pool_in):
        self.out, self.pool, self.mot, self.off, self.own, self.si, self.pool_in = out, pool, mot, off, own, si, pool_in

    def peers(self, s):
        """(obs_n - n_own, [peer scene of every filled slot]) of scene s."""
        c = int(self.out["obs_n"][s]) - int(self.own[s])
        a = int(self.off[s]) + int(self.own[s])
        sl = self.pool[a:a + c]
        assert ((sl["type"] & fl.OB_PEER) != 0).all()
        return c, [int(t) & ~fl.OB_PEER for t in sl["type"]]

    def slots(self, s):
        """The K peer slots of scene s, filled or not."""
        a = int(self.off[s]) + int(self.own[s])
        return self.pool[a:a + self.K]


def _filled(count, dtype):
    return np.frombuffer(bytes([FILL]) * (max(count, 1) * np.dtype(dtype).itemsize), dtype).copy()


def fleet_inputs(cfg, fm, xy, n_own, motion):
    """SceneIn records of the road at the positions xy; scene s owns n_own[s] pool entries and the K entries behind them."""
    n, K = len(xy), int(np.asarray(fm).reshape(-1)[0]["max_peers"])
    own = np.broadcast_to(np.asarray(n_own, np.int64), (n,)).copy()
    off = np.concatenate([[0], np.cumsum(own + K)[:-1]]) if n else np.zeros(0, np.int64)
    si = np.repeat(road(cfg)["scene_in"][:1], n)
    si["loc"]["globalpoint"]["x"], si["loc"]["globalpoint"]["y"] = [p[0] for p in xy], [p[1] for p in xy]
    total = int((own + K).sum())
    return si, _filled(total, dm.ObPoint), _filled(total, dm.ObMotion) if motion else None, off, own, total


class FleetModelBackend:
    name = "model"

    def run(self, cfg, fm, wf, xy, n_own, motion):
        si, pool, mot, off, own, _ = fleet_inputs(cfg, fm, xy, n_own, motion)
        si["obs_off"], si["obs_n"] = 12345, -7
        out, p2, m2 = fl.couple(fm, wf, off, own, si, pool, mot)
        return FleetResult(out, p2, m2, off, own, si, pool)


class FleetDeviceBackend:
    name = "device"

    def run(self, cfg, fm, wf, xy, n_own, motion):
        si, pool, mot, off, own, total = fleet_inputs(cfg, fm, xy, n_own, motion)
        si["obs_off"], si["obs_n"] = off, own
        sc, n = road(cfg), len(si)
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=len(pool), max_lane_pts_total=len(sc["lane_pool"]), max_ref_pts_total=len(sc["ref_pool"]))
        _set_scenes(pl, sc, si, pool, mot, total)
        assert pl.get_scene_in().tobytes() == si.tobytes(), "the resident records are the crafted ones"
        pl.set_fleet(wf, fm)
        out = pl.get_scene_in()
        p2 = pl.read_device(dm.BUF_OBS_POOL, dm.ObPoint, len(pool))
        m2 = pl.read_device(dm.BUF_MOT_POOL, dm.ObMotion, len(pool)) if motion else None
        want, wpool, wmot = fl.couple(fm, wf, off, own, si, pool, mot)
        assert np.array_equal(out["obs_off"], want["obs_off"]) and np.array_equal(out["obs_n"], want["obs_n"]), \
            f"obs_n of scenes {np.flatnonzero(out['obs_n'] != want['obs_n'])[:8].tolist()}: {out['obs_n'][out['obs_n'] != want['obs_n']][:8].tolist()}"
        assert out.tobytes() == want.tobytes(), "SceneIn"
        for s in (range(n) if n <= 200 else sorted(set(range(0, n, 9)) | set(range(n - 70, n)) | set(range(16)))):          # (every pool byte is compared below)
            a, c = int(want["obs_off"][s]), int(want["obs_n"][s])
            sl = pl.get_obstacles(s)
            assert sl.tobytes() == wpool[a:a + c].tobytes(), f"scene {s}: slice, peers {[int(t) & ~fl.OB_PEER for t in sl['type'][int(own[s]):]]}"
        pl.close()
        assert p2.tobytes() == wpool.tobytes(), "the obstacle pool, untouched slots included"
        assert m2 is None or m2.tobytes() == wmot.tobytes(), "the motion pool"
        return FleetResult(out, p2, m2, off, own, si, pool)


class FleetRunner:
    """What a fleet case calls; every call is logged for fleet_batched()."""
    def __init__(self, backend, log=None):
        self.backend, self.name, self.log = backend, backend.name, log

    def __call__(self, cfg, fm, world_first, xy, n_own=0, motion=False, batch=True):
        fm = np.array(fm, dm.FleetModel).reshape(1).copy()
        res = self.backend.run(cfg, fm, list(world_first), list(xy), n_own, motion)
        res.K = int(fm["max_peers"][0])
        if self.log is not None and batch:
            self.log.append(dict(cfg=cfg.copy(), fm=fm, wf=list(world_first), xy=list(xy), n_own=res.own.copy(), motion=motion, res=res))
        return res


def fleet_batched(backend, log, max_scenes=320):
    """Every logged call again, its worlds beside those of the other calls in one launch: the calls with the same FleetModel and the
    same kind of set (motion pool or none) are laid one behind the other - scene indices and pool offsets move - in launches of at
    most `max_scenes` scenes (as long as one call fits), at least two calls and five scenes each (the first calls are repeated to get there) and never a
    multiple of four scenes (a world of one is added behind them), so most worlds start at a scene index that is no multiple of 64 and share
    their blocks with other worlds.  Every scene must give the bytes it gave alone: SceneIn but for the moved obs_off, and every
    pool entry - a filled slot names its peer by scene index, moved alike.  Returns the batch sizes (scenes)."""
    groups = {}
    for c in log:
        groups.setdefault((c["cfg"].tobytes(), c["fm"].tobytes(), c["motion"]), []).append(c)
    sizes = []
    for cases in groups.values():
        chunks, cur = [], []
        for c in cases:
            if cur and sum(len(x["xy"]) for x in cur) + len(c["xy"]) > max_scenes:
                chunks.append(cur)
                cur = []
            cur.append(c)
        chunks.append(cur)
        for chunk in chunks:
            chunk, k = list(chunk), 0
            while len(chunk) < 2 or sum(len(x["xy"]) for x in chunk) < 5:
                chunk.append(cases[k % len(cases)])
                k += 1
            xy, wf, own, first = [], [0], [], []
            for c in chunk:
                first.append(len(xy))
                wf += [w + len(xy) for w in c["wf"][1:]]
                xy += c["xy"]
                own += c["n_own"].tolist()
            if len(xy) % 4 == 0:                          # one more scene, a world of its own far from everybody: the last block is partial
                xy, wf, own = xy + [(-1.0e6, -1.0e6)], wf + [len(xy) + 1], own + [0]
            c0 = chunk[0]
            res = backend.run(c0["cfg"], c0["fm"], wf, xy, np.array(own), c0["motion"])
            K = int(c0["fm"]["max_peers"][0])
            for c, p0 in zip(chunk, first):
                alone, m = c["res"], len(c["xy"])
                at = int(res.off[p0]) if m else 0
                got = res.out[p0:p0 + m].copy()
                got["obs_off"] -= at
                assert got.tobytes() == alone.out.tobytes(), f"batch of {len(xy)}, world at {p0}: SceneIn"
                total = int((alone.own + K).sum())
                pool = res.pool[at:at + total].copy()
                for s in range(m):
                    a = int(alone.off[s]) + int(alone.own[s])
                    pool["type"][a:a + int(alone.out["obs_n"][s]) - int(alone.own[s])] -= p0
                assert pool.tobytes() == alone.pool[:total].tobytes(), f"batch of {len(xy)}, world at {p0}: pool"
                assert res.mot is None or res.mot[at:at + total].tobytes() == alone.mot[:total].tobytes(), f"batch of {len(xy)}, world at {p0}: motion pool"
            sizes.append(len(xy))
    return sizes
