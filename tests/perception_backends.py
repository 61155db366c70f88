"""Two backends for the perception model: the numpy model tests/perception_model.py and k_perceive inside a real tick.

One call takes the configuration, the PerceptionModel and a list of coupling_backends.Tick - each the SceneIn[N] records and the
obstacle pool the tick reads - and returns, per tick, the perceived snapshot, the truth snapshot, the tracks and the stats.  The
device leg is a slice-mode handle on coupling_backends.road (grid stage, decision stage and moving obstacles off: the truth snapshot
is the pool), fed every tick's records and pool through pp_update_async; what it reads back - BUF_OBS_SEEN, BUF_OBS_NOW, the tracks and
the stats - is held byte for byte against the model stepped over the device's own SceneIn and tick id, on the entries some slice
covers (the others belong to nobody and are never written).  A case asserts its known answers as literals on both legs."""
import numpy as np

import coupling_backends as cb
import dmpp_amd as dm
import perception_model as pcm
import score_trace_backends as stb

same = stb.same
batch_ticks = stb.batch_ticks
config = cb.config


def model(**kw):
    """The transparent model with the given fields changed."""
    m = dm.transparent_perception()
    for k, v in kw.items():
        m[k] = v
    return m


def scene_tick(cfg, scenes):
    """scenes: (x, y, dir, obstacles) per scene, obstacles (x, y, radius[, type]); the slices lie one behind the other."""
    t = cb.tick(cfg, [(x, y, 0.0, [(o[0], o[1], o[2]) for o in obs]) for x, y, d, obs in scenes])
    for k, (x, y, d, obs) in enumerate(scenes):
        t.si[k]["loc"]["globalpoint"]["dir"] = d
        off = int(t.si[k]["obs_off"])
        for j, o in enumerate(obs):
            t.pool[off + j]["type"] = o[3] if len(o) > 3 else 1
    return t


def covered(si, n_pool):
    keep = np.zeros(n_pool, bool)
    for s in si:
        keep[int(s["obs_off"]):int(s["obs_off"]) + int(s["obs_n"])] = True
    return keep


class PerceptResult:
    """seen[k], now[k], tracks[k], stats[k], log[k][s][j] = (cause, output): behind tick k; T[k]: its id."""
    def __init__(self):
        self.seen, self.now, self.tracks, self.stats, self.log, self.T = [], [], [], [], [], []

    def entry(self, k, s, j, si):
        return self.seen[k][int(si[s]["obs_off"]) + j]


def _step(tracks, stats, m, cfg, T, si, pool, ep, replica):
    """pcm.step; replica: every scene is a copy of scene 0 and the model draws nothing from the hash that depends on the scene
    (p_miss 0 or 0xFFFFFFFF without a survivor, no noise) - scene 0 is stepped and its slice, tracks and stats are laid out n times."""
    if not replica:
        return pcm.step(tracks, stats, m, cfg, T, si, pool, ep)
    n, n1 = len(si), int(si[0]["obs_n"])
    assert all(int(si[s]["obs_off"]) == s * n1 and int(si[s]["obs_n"]) == n1 for s in range(n))
    assert all(pool[s * n1:(s + 1) * n1].tobytes() == pool[:n1].tobytes() for s in range(n)), "copies of scene 0"
    t1, s1 = tracks[:n1].copy(), stats[:1].copy()
    seen1, log1 = pcm.step(t1, s1, m, cfg, T, si[:1], pool[:n1], None if ep is None else ep[:1])
    tracks[:n * n1], stats[:] = np.tile(t1, n), np.tile(s1, n)
    seen = np.zeros(len(pool), pool.dtype)
    seen[:n * n1] = np.tile(seen1, n)
    return seen, log1 * n


class ModelBackend:
    name = "model"

    def run(self, cfg, m, ticks, ep_stats=None, replica=False):
        cap = max(len(t.pool) for t in ticks)
        tracks, stats = pcm.new_tracks(dm.PerceptTrack, cap), pcm.new_stats(dm.PerceptionStats, len(ticks[0].si))
        res = PerceptResult()
        for k, t in enumerate(ticks):
            seen, log = _step(tracks, stats, m, cfg, k + 1, t.si, t.pool, None if ep_stats is None else ep_stats[k], replica)
            res.seen.append(seen), res.now.append(t.pool.copy()), res.tracks.append(tracks.copy()), res.stats.append(stats.copy())
            res.log.append(log), res.T.append(k + 1)
        return res


class DeviceBackend:
    name = "device"

    def run(self, cfg, m, ticks, ep_stats=None, replica=False):
        assert ep_stats is None, "episodes on the device: test_perception.test_episode_restart_on_the_device"
        assert not int(cfg["grid_stage"][0]) and not int(cfg["decision_stage"][0]) and not int(cfg["dynamic_obstacles"][0])
        n, cap = len(ticks[0].si), max(len(t.pool) for t in ticks)
        pl = stb.open_planner(cfg, ticks, None, False)
        pl.set_perception(m)
        wtracks, wstats = pcm.new_tracks(dm.PerceptTrack, cap), pcm.new_stats(dm.PerceptionStats, n)
        same(pl.perception_stats(), wstats, "stats before the first tick")
        same(pl.perception_tracks(0, cap), wtracks, "tracks before the first tick")
        res, keep = PerceptResult(), []
        for k, t in enumerate(ticks):
            sin, _, _ = stb.feed(pl, t, keep)
            T = pl.tick_id()
            wseen, log = _step(wtracks, wstats, m, cfg, T, sin, t.pool, None, replica)
            on = covered(sin, len(t.pool))
            seen, now = pl.read_device(dm.BUF_OBS_SEEN, dm.ObPoint, len(t.pool)), pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, len(t.pool))
            tracks, stats = pl.perception_tracks(0, cap), pl.perception_stats()
            same(now[on], t.pool[on], f"tick {k}: the truth snapshot")
            same(seen[on], wseen[on], f"tick {k}: the perceived snapshot")
            same(tracks[:len(t.pool)][on], wtracks[:len(t.pool)][on], f"tick {k}: tracks")
            same(stats, wstats, f"tick {k}: stats")
            seen[~on] = 0
            res.seen.append(seen), res.now.append(now), res.tracks.append(tracks), res.stats.append(stats), res.log.append(log), res.T.append(T)
        pl.close()
        return res


BACKENDS = {"model": ModelBackend, "device": DeviceBackend}
