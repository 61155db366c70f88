"""The rollout feature table ("Feature life cycle"; tests/test_feature_table.py holds it literally) against the device: for
every (cause, retired feature) cell a handle with everything the cell needs switched on runs a leg, the cause is applied, what the cause
took away is put back - but for the feature under test and what cannot be on without it -, a second leg runs, and the public getters show
that the feature did nothing in it.  For the rows that retire nothing: every feature that was on is still at work.

The traffic-reset column is tests/test_episode_traffic.py::test_every_switch_off_site_and_the_getter, and pp_set_egos -> route is
tests/test_route.py::test_route_off_is_the_engine_without_one; they are not repeated here.

The scene: the 16 followers of tests/test_episode_spawn.py::_loop_scene (the contact loop of tests/test_episode_traffic.py) with a timeout
of 20 advances, 45 advances per leg: wherever the vehicles stand, every ego restarts at least twice in a leg."""
import numpy as np
import pytest

import ego_model as egm
import route_model as rmod
import test_episode_spawn as tes
import test_episodes as te
import test_feature_table as ft
import test_route as trt
import test_traffic as tt

gpu = pytest.mark.gpu
K, N, LOG_CAP = 45, tt.F_N, 4096
NEEDS = {ft.FLEET: ft.WORLD, ft.TRAFFIC: ft.TRESET, ft.EPISODES: ft.SPAWN | ft.TRESET | ft.ELOG}          # what cannot be on without the feature
ORDER = (ft.ROUTE, ft.FLEET, ft.TRAFFIC, ft.WORLD, ft.EPISODES, ft.SPAWN, ft.TRESET, ft.ELOG)              # every feature behind what it needs


def _scene(dm):
    return dict(tes._loop_scene(dm), em=te._em(dm, 31, 20))


def _fleet0(dm):
    fm = dm.default_fleet_model()
    fm["max_peers"] = 0                                          # (worlds of one scene, no peer slots: what pp_set_world_traffic needs)
    return fm


def _switch_on(dm, pl, r, features):
    calls = {ft.ROUTE: lambda: pl.set_route(r["legs"], r["rf"]),
             ft.FLEET: lambda: pl.set_fleet(np.arange(N + 1, dtype=np.int32), _fleet0(dm)),
             ft.TRAFFIC: lambda: pl.set_traffic(r["tracks"], r["pts"], r["act"]),
             ft.WORLD: lambda: pl.set_world_traffic(r["tracks"], r["pts"], r["act"]),
             ft.EPISODES: lambda: pl.set_episodes(r["em"]),
             ft.SPAWN: lambda: pl.set_episode_spawn(r["sp"]),
             ft.TRESET: lambda: pl.set_episode_traffic(1),
             ft.ELOG: lambda: pl.set_episode_log(LOG_CAP)}
    for f in ORDER:
        if features & f:
            calls[f]()


PER_SCENE = ft.ROUTE | ft.FLEET | ft.TRAFFIC | ft.EPISODES | ft.SPAWN | ft.TRESET | ft.ELOG
PER_WORLD = ft.ROUTE | ft.FLEET | ft.WORLD | ft.EPISODES | ft.SPAWN | ft.ELOG


def _handle(dm, r, features):
    pl = tt._planner(dm, r["cfg"], r["m"], r["sc"], 1)
    _switch_on(dm, pl, r, features)
    return pl


def _read(pl, features):
    """What the getters say the features have done so far."""
    out = dict(episodes=pl.episode_stats()["n_episodes"].copy())
    if features & ft.SPAWN:
        out["spawn"] = pl.episode_spawn_stats()["n_used"].copy()
    if features & ft.TRESET:
        out["treset"] = pl.episode_traffic_resets()
    if features & ft.ELOG:
        out["elog"] = pl.episode_log_info()[0]
    if features & (ft.TRAFFIC | ft.WORLD):
        out["traffic"] = pl.traffic_state()
    return out


def _egos(dm, pl, r):
    pl.set_egos(r["sc"], with_motion=False)
    pl.set_state(r["sc"]["state"])


# (cause, how the call is made, the own feature that the call's off form takes away, the own feature whose stats the call's set form restarts)
CAUSES = {
    "set_egos": (ft.RESIDENT, _egos, 0, 0),
    "set_fleet": (ft.SET_FLEET, lambda dm, pl, r: pl.set_fleet(np.arange(N + 1, dtype=np.int32), _fleet0(dm)), 0, 0),
    "set_fleet_off": (ft.SET_FLEET, lambda dm, pl, r: pl.set_fleet(None), ft.FLEET, 0),
    "set_traffic_off": (ft.TRAFFIC_OFF, lambda dm, pl, r: pl.set_traffic(None), 0, 0),
    "set_world_traffic_off": (ft.TRAFFIC_OFF, lambda dm, pl, r: pl.set_world_traffic(None), 0, 0),
    "set_episodes": (ft.SET_EPISODES, lambda dm, pl, r: pl.set_episodes(r["em"]), 0, ft.EPISODES),
    "set_episodes_null": (ft.SET_EPISODES, lambda dm, pl, r: pl.set_episodes(off=True), ft.EPISODES, 0),
    "set_episode_spawn": (ft.SET_SPAWN, lambda dm, pl, r: pl.set_episode_spawn(r["sp"]), 0, ft.SPAWN),
    "set_episode_spawn_null": (ft.SET_SPAWN, lambda dm, pl, r: pl.set_episode_spawn(None), ft.SPAWN, 0),
}
CELLS = [("set_egos", PER_SCENE, ft.TRAFFIC), ("set_egos", PER_SCENE, ft.EPISODES), ("set_egos", PER_SCENE, ft.SPAWN), ("set_egos", PER_SCENE, ft.ELOG),
         ("set_egos", PER_WORLD, ft.WORLD), ("set_fleet", PER_WORLD, ft.WORLD), ("set_fleet_off", PER_WORLD, ft.WORLD),
         ("set_traffic_off", PER_SCENE, ft.TRAFFIC), ("set_world_traffic_off", PER_WORLD, ft.WORLD),
         ("set_episodes", PER_SCENE, ft.SPAWN), ("set_episodes", PER_SCENE, ft.ELOG), ("set_episodes_null", PER_SCENE, ft.SPAWN), ("set_episodes_null", PER_SCENE, ft.ELOG),
         ("set_episode_spawn", PER_SCENE, ft.ELOG), ("set_episode_spawn_null", PER_SCENE, ft.ELOG)]


@gpu
@pytest.mark.parametrize("site,features,x", CELLS, ids=[f"{s}-{ft.NAMES[x].replace(' ', '_')}" for s, _, x in CELLS])
def test_a_retired_feature_does_nothing(dm, site, features, x):
    cause, call, own, restarted = CAUSES[site]
    assert ft.TABLE[cause] & x                                   # (the cell is one of the table)
    r = _scene(dm)
    pl = _handle(dm, r, features)
    pl.rollout(K)
    first = _read(pl, features)
    assert first["episodes"].all() and first["spawn"].sum() and first["elog"] > 0          # (the first leg had all of it at work)
    call(dm, pl, r)
    back = (ft.TABLE[cause] | own) & features & ~(x | NEEDS.get(x, 0))
    if cause == ft.RESIDENT:
        back |= ft.ROUTE & features
    _switch_on(dm, pl, r, back)
    on = (features & ~(ft.TABLE[cause] | own)) | back
    restarted |= back                                            # (a set call starts its feature's stats again)
    if restarted & ft.ELOG:
        first["elog"] = 0
    if restarted & ft.SPAWN:
        first["spawn"][:] = 0
    if restarted & ft.EPISODES:
        first["episodes"][:] = 0
    pl.rollout(K)
    pl.sync()
    if on & ft.EPISODES:                                         # the egos did restart in the second leg ...
        assert (pl.episode_stats()["n_episodes"] > first["episodes"]).all(), "an ego did not restart in the second leg"
    if x == ft.SPAWN:                                            # ... and the feature under test had no part in it
        assert pl.episode_spawn_stats()["n_used"].tobytes() == first["spawn"].tobytes()
    elif x == ft.ELOG:
        assert pl.episode_log_info()[0] == first["elog"]
    elif x == ft.EPISODES:
        assert pl.episode_stats()["n_episodes"].tobytes() == first["episodes"].tobytes()
    else:                                                        # traffic of either kind
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.traffic_state()
    if on & ft.SPAWN and x != ft.SPAWN:                          # what was put back is at work again
        assert pl.episode_spawn_stats()["n_used"].sum() > first["spawn"].sum()
    if on & ft.ELOG and x != ft.ELOG:
        assert pl.episode_log_info()[0] > first["elog"]
    pl.close()


@gpu
def test_new_resident_scenes_retire_the_fleet(dm):
    """pp_set_egos -> fleet, on the same egos with a free pool entry behind every slice and worlds of two: with the fleet every scene's slice
    is its own entry and the peer, behind pp_set_egos the own entry alone."""
    r = _scene(dm)
    sc = dict(r["sc"], scene_in=r["sc"]["scene_in"].copy(), obs_pool=np.zeros(2 * N, dm.ObPoint), n_obs=2)
    sc["scene_in"]["obs_off"] = 2 * np.arange(N)
    sc["obs_pool"]["radius"] = 0.5
    fm = dm.default_fleet_model()
    fm["max_peers"], fm["range"] = 1, 1.0e6                       # (the other ego of the world is always in range)
    pl = tt._planner(dm, r["cfg"], r["m"], sc, 2)
    pl.set_route(r["legs"], r["rf"])
    pl.set_fleet(np.arange(0, N + 1, 2, dtype=np.int32), fm)
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    pl.rollout(K)
    assert [len(pl.get_obstacles(s)) for s in range(N)] == [2] * N
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    pl.rollout(K)
    assert [len(pl.get_obstacles(s)) for s in range(N)] == [1] * N
    pl.close()


@gpu
def test_a_new_map_retires_the_route(dm):
    """pp_set_map -> route, on the scene of tests/test_route.py::test_route_off_is_the_engine_without_one: behind the call the egos run into
    their lane ends like those of a handle whose route was switched off by pp_set_route(0), byte for byte."""
    cfg, m, sc, legs, rf = trt._step_scene(dm)
    outs = []
    for by_map in (True, False):
        pl = trt._planner(dm, cfg, m, sc)
        pl.set_route(legs, rf)
        pl.rollout(30)
        pl.set_map(m) if by_map else pl.set_route(None)
        pl.rollout(40)
        pl.sync()
        outs.append((pl.get_scene_in(), pl.ego_flags(), pl.get_state()))
        pl.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert (outs[0][1] & egm.LANE_END).any()


NOTHING = {"set_route": lambda dm, pl, r: pl.set_route(r["legs"], r["rf"]),
           "set_episode_traffic": lambda dm, pl, r: pl.set_episode_traffic(1),
           "set_episode_log": lambda dm, pl, r: pl.set_episode_log(LOG_CAP),
           "set_grid_follow": lambda dm, pl, r: (pl.set_grid_follow(dm.default_grid_follow()), pl.set_grid_follow(None)),
           "score_begin_end": lambda dm, pl, r: (pl.score_begin(), pl.score_end())}


@gpu
@pytest.mark.parametrize("site", list(NOTHING))
def test_calls_that_retire_nothing_leave_every_feature_at_work(dm, site):
    r = _scene(dm)
    pl = _handle(dm, r, PER_SCENE)
    pl.rollout(K)
    first = _read(pl, PER_SCENE)
    assert first["episodes"].all() and first["treset"].all() and first["elog"] > 0
    NOTHING[site](dm, pl, r)
    if site == "set_episode_traffic":
        first["treset"][:] = 0                                   # (the call restarts its own counters)
    if site == "set_episode_log":
        first["elog"] = 0
    pl.rollout(K)
    pl.sync()
    now = _read(pl, PER_SCENE)
    assert (now["episodes"] > first["episodes"]).all() and (now["treset"] > first["treset"]).all() and now["elog"] > first["elog"]
    assert now["spawn"].sum() > first["spawn"].sum() and now["traffic"].tobytes() != first["traffic"].tobytes()
    assert not (pl.ego_flags() & rmod.ROUTE_END).any()
    pl.close()
