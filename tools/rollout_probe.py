#!/usr/bin/env python3
"""Runs ON THE GPU BOX: ticks/s of the closed loop on the device (pp_rollout: advance + tick, no per-tick PCIe traffic) against
the host-fed streamed loop (pp_update_async of prepared pinned inputs + pp_fetch_published_async, what a host-side vehicle
model needs every tick), same handle size, same build, alternating.
    python tools/rollout_probe.py [scenes] [timed ticks] [warm-up ticks] [runs]
SCORE=1: the rollout leg runs with the scorecard on (pp_score_begin) and prints a summary of the records; SCORE=ab: every run has
a rollout leg without and one with scoring, alternating (the cost of scoring on one build).
FLEET=K: every run has a rollout leg with the fleet on (pp_set_fleet, K peer slots per scene; FLEET_WORLD=<scenes per world>, 0 or
unset: one world of all scenes; FLEET_RANGE=<metres>, default the model's) and one with the fleet off whose scenes carry K far-away
obstacles more - the same obs_n, or the comparison would charge the fleet for longer obstacle lists -, alternating.
ROUTE=1: every run has a rollout leg of obstacle-free egos on the ring of tests/route_scenes.py (map store, grid stage off) with
their routes set (pp_set_route: k_advance_route) and one without (k_advance_egos: the egos freeze at their lane ends), alternating.
FOLLOW=1: every run has a rollout leg of routed ring egos with the grid stage ON (256 x 256 cells) whose grid follows the ego
(pp_set_grid_follow, default model) and one without (the egos leave their grids and freeze with OFF_GRID), alternating.
FOLLOW=trace_on / trace_off: for rocprofv3 --kernel-trace --stats - one such ring rollout (k_advance_route) and one rollout of the
generated scenes (k_advance_egos), both with following on / both with it off, and nothing else.
TRAFFIC=A: every run has a rollout leg with lane traffic on (pp_set_traffic: A actors per scene, default 8 for TRAFFIC=1, in the first
A of the scene's own obstacle entries, driving the scene's current lane as an open track at 1 .. 8 m/s) and one with it off: the same
scenes after the same pp_set_traffic, switched off again, so both legs start from the same pool with the same obs_n - alternating.
MANOEUVRE=1 (with TRAFFIC, and REACT for following): traffic (and following) stay on in both legs; the leg "on" also has a manoeuvre list
(pp_set_traffic_manoeuvres, DESIGN.md §4v: k_manoeuvre_traffic in the place of k_move_traffic / k_follow_traffic) - every actor swings
1 m to the left and back, eight records of 10 advances, the first when the ego is within 60 m.
EPISODES=1: every run has a rollout leg of routed ring egos with ONE-leg routes and episodes on (pp_set_episodes, default model:
k_respawn_egos behind k_advance_route, arrived egos restart) and one with them off on the same scenes (arrived egos freeze),
alternating; with ONE_ROLLOUT one more leg with episodes on alone, for rocprofv3 --kernel-trace --stats.
EPISODES=1 with SPAWN=M and / or CONTACT=1: both legs have episodes on, on the ring with traffic - OBS obstacle entries per scene
(default 1), the first a vehicle that drives the ego's lane towards it at 3 m/s from 20 m ahead (pp_set_traffic), the others far away -
and the second leg has the spawn model on as well (pp_set_episode_spawn, DESIGN.md §4l: k_respawn_spawn in the place of
k_respawn_egos) with M start records per scene - record k of scene s is the start of scene (s + k) mod n - and contact ending an
episode if CONTACT=1; the default clearance and check.
EPISODES=1 RESET=1 (with SPAWN=M and / or CONTACT=1): both legs have that spawn model on, and the second leg the episode traffic reset as
well (pp_set_episode_traffic, DESIGN.md §4m: k_reset_traffic behind k_move_traffic) - with M > 1 one set of start states per start record,
the vehicle 20 m ahead of that record along its own track.  The workloads differ: without the reset the egos spend advances restarting
into the vehicle that drove on over their start pose (the egos with an episode of age 1 are printed); k_reset_traffic's own cost is
what a kernel trace of the ONE_ROLLOUT leg gives.
EPISODES=1 LOG=cap: both legs are the ring rollout with episodes on, and the second leg has the episode log on as well
(pp_set_episode_log(cap), DESIGN.md §4n: k_log_episodes behind k_respawn_egos); it is drained once behind the timed rollout, outside the
timing.  SCORE=1 puts the scorecard on in both legs (k_score_ego<true> in the second).  With ONE_ROLLOUT one more leg with the log on alone.
EPISODES=1 SPAWN=M SCHEDULE=pooled|scene (with CONTACT=1 / RESET=1 as above): both legs have that spawn model on (and the reset, if asked
for), and the second leg the scenario schedule as well (pp_set_episode_schedule, DESIGN.md §4p: k_respawn_sched in the place of
k_respawn_spawn, in pooled scope k_fold_schedule behind it) - the default model in that scope, contact the failure.  The rows are read
behind the timed rollout, outside the timing.  With ONE_ROLLOUT one more leg with the schedule on alone.
EPISODES=1 WORLDS=1 (with FLEET=K, FLEET_WORLD=<scenes per world>, SPAWN=M, CONTACT=1, RESET=1 as above): both legs have the fleet - K peer
slots behind every scene's OBS own entries, worlds of FLEET_WORLD consecutive scenes (0 or unset: 16) - and that spawn model on, and the
second leg world episodes as well (pp_set_episode_worlds, DESIGN.md §4s: k_respawn_world in the place of k_respawn_spawn): when one ego
of a world ends, its whole world restarts.  RESET=1 keeps the per-scene reset of §4m on in both legs.  The workloads differ - a world
restarts as often as ALL its members end -: the episodes ended and the members that ended with DMPP_EGO_WORLD are printed beside the
rates.  With ONE_ROLLOUT one more leg with world episodes on alone.
SCORE=1 TRACE=depth: every run has a scored rollout leg without and one with the score trace (pp_set_score_trace: the default model with
`depth` records per scene, DESIGN.md §4o: k_score_ego<false, true> in the place of <false, false>), alternating; headers and one ring are
read behind the timed rollout, outside the timing.  TRACE_TRIGGER=mask replaces the model's trigger (0: rings that never freeze, so every
scene stores every tick).  With ONE_ROLLOUT one more leg of each, so that one kernel trace holds both kernels.
TRACK=1 [TRACK_BIAS=b]: every run has a rollout leg of routed ring egos (grid stage off, scorecard on for its replan count) without and
one with the ego tracker (pp_set_ego_tracker: the default model with curv_bias b, DESIGN.md §4q: k_advance_route<true> in the place of
<false>), alternating.  The workloads differ once tracked egos replan on lateral error: the replan counts are printed beside the rates.
With ONE_ROLLOUT one more leg of each, so that one kernel trace holds both kernels.
PERCEPT=1: every run has a rollout leg without and one with the default perception model (pp_set_perception), and
prints the entry-ticks by cause and by output.
CONFLICT=1 (implies SCORE=1): every run has a scored rollout leg without and one with the conflict score (pp_set_conflict_score: the default
model, DESIGN.md §4u: k_score_ego<false, false, true> in the place of <false, false, false>), alternating; the records are read behind the
timed rollout, outside the timing.  With ONE_ROLLOUT one more leg of each, so that one kernel trace holds both kernels."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import dmpp_amd as dm
from parity_util import move_ego

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 10
runs = int(sys.argv[4]) if len(sys.argv) > 4 else 3
n_obs, depth = int(os.environ.get("N_OBS", "64")), 4          # N_OBS: obstacles per generated scene
cfg = dm.default_config(512)
model = dm.default_ego_model()


def fresh():
    sc = dm.gen_scenes(cfg, 0, n, n_obs, junction_every=8)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    return pl, sc


CONFLICT = os.environ.get("CONFLICT", "0") == "1"
PERCEPT = os.environ.get("PERCEPT", "0") == "1"          # a rollout leg without and one with the default perception model
SCORE = "1" if CONFLICT else os.environ.get("SCORE", "0")
FLEET = int(os.environ.get("FLEET", "0"))
FLEET_WORLD = int(os.environ.get("FLEET_WORLD", "0"))


def fleet_run(on):
    """n_obs own obstacles and FLEET more entries per scene: the peer slots (fleet on), or obstacles 1e6 m away (fleet off)."""
    K, stride = FLEET, n_obs + FLEET
    sc = dm.gen_scenes(cfg, 0, n, n_obs, junction_every=8)
    pool = np.zeros((n, stride), dm.ObPoint)
    pool[:, :n_obs] = sc["obs_pool"].reshape(n, n_obs)
    pool[:, n_obs:]["x"], pool[:, n_obs:]["y"], pool[:, n_obs:]["radius"] = 1e6, 1e6, 0.5
    sc["obs_pool"], sc["n_obs"] = pool.reshape(-1), stride
    sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"] = np.arange(n) * stride, n_obs if on else stride
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * stride)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    if on:
        fm = dm.default_fleet_model()
        fm["max_peers"] = K
        if os.environ.get("FLEET_RANGE"):
            fm["range"] = float(os.environ["FLEET_RANGE"])
        w = FLEET_WORLD if FLEET_WORLD > 0 else n
        pl.set_fleet(list(range(0, n, w)) + [n], fm)
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    mean_obs = float(pl.get_scene_in()["obs_n"].mean())
    pl.close()
    return n * steps / dt, mean_obs


TRAFFIC = int(os.environ.get("TRAFFIC", "0"))
if TRAFFIC == 1:
    TRAFFIC = 8
REACT = os.environ.get("REACT", "0") == "1"
MANOEUVRE = os.environ.get("MANOEUVRE", "0") == "1"          # with TRAFFIC (and REACT): traffic (and following) stay on in both legs; "on" = a manoeuvre list too


def traffic_run(on):
    pl, sc = fresh()
    lanes = sc["scene_in"]["lanes"]
    tracks, actors = np.zeros(n, dm.TrafficTrack), np.zeros(n * TRAFFIC, dm.TrafficActor)
    tracks["point_off"], tracks["n_points"] = lanes["cur_off"], lanes["cur_n"]
    pts = np.zeros(len(sc["lane_pool"]), dm.GlobalPoint2D)
    pts["x"], pts["y"] = sc["lane_pool"]["x"], sc["lane_pool"]["y"]
    k = np.arange(n * TRAFFIC)
    actors["scene"], actors["slot"], actors["track"] = k // TRAFFIC, k % TRAFFIC, k // TRAFFIC
    actors["s0"], actors["speed"], actors["type"], actors["radius"] = 10.0 + 12.0 * (k % TRAFFIC), 1.0 + (k % 8), 1, 0.9
    pl.set_traffic(tracks, pts, actors)
    if MANOEUVRE:                     # every actor swings 1 m to the left and back, over and over: eight records of 10 advances each, the first when the ego is within 60 m
        if REACT:
            pl.set_traffic_follow(dm.default_traffic_follow())
        if on:
            recs = np.zeros((n * TRAFFIC, dm.MANOEUVRE_MAX), dm.TrafficManoeuvre)
            recs["actor"], recs["track"], recs["n_steps"], recs["speed"] = k[:, None], -1, 10, np.nan
            recs["lat_end"] = np.where(np.arange(dm.MANOEUVRE_MAX) % 2 == 0, 1.0, 0.0)[None, :]
            recs["trigger"][:, 0], recs["dist"][:, 0] = dm.TRIG_EGO_DIST, 60.0
            pl.set_traffic_manoeuvres(recs.reshape(-1))
    elif REACT:                       # REACT=1: traffic stays on in both legs; "on" = the car-following law too
        if on:
            pl.set_traffic_follow(dm.default_traffic_follow())
    elif not on:
        pl.set_traffic(None)          # the entries stay where the set call put them: plain obstacles
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    frozen = int((pl.ego_flags() != 0).sum())
    pl.close()
    return n * steps / dt, frozen


def route_run(on):
    import route_scenes as rs
    rcfg = dm.default_config(128)
    rcfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, rcfg, m, n, seed=5, ids=(10, 250), legs=(6, 10))
    pl = dm.Planner(rcfg, device=0, **rs.caps(m, n))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    if on:
        pl.set_route(legs, rf)
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    frozen = int((pl.ego_flags() != 0).sum())
    pl.close()
    return n * steps / dt, frozen


LOG = int(os.environ.get("LOG", "0"))


def episodes_run(on, log=0):
    import route_scenes as rs
    rcfg = dm.default_config(128)
    rcfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, rcfg, m, n, seed=5, ids=(10, 250), legs=(1, 1))
    pl = dm.Planner(rcfg, device=0, **rs.caps(m, n))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_route(legs, rf)
    if LOG > 0 and SCORE == "1":
        pl.score_begin()
    if on:
        pl.set_episodes()
    if log > 0:
        pl.set_episode_log(log)           # last
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    frozen = int((pl.ego_flags() != 0).sum())
    ended = int(pl.episode_stats()["n_episodes"].sum()) if on else 0
    if log > 0:
        recs, lost = pl.read_episode_log()
        episodes_run.logged = (pl.episode_log_info()[0], len(recs), lost)
    pl.close()
    return n * steps / dt, frozen, ended


SPAWN = int(os.environ.get("SPAWN", "0"))
CONTACT = os.environ.get("CONTACT", "0") == "1"
RESET = os.environ.get("RESET", "0") == "1"
SCHEDULE = os.environ.get("SCHEDULE", "")


WORLDS = os.environ.get("WORLDS", "0") == "1"


def spawn_run(on, reset=False, sched="", worlds=None):
    import route_scenes as rs
    import traffic_model as tm
    import traffic_scenes as ts
    k_obs, M = int(os.environ.get("OBS", "1")), max(SPAWN, 1)
    rcfg = dm.default_config(128)
    rcfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, rcfg, m, n, seed=5, lanes=(1, 2), ids=(10, 250), legs=(1, 1), n_obs=k_obs)
    sc["mot_pool"] = None
    sc["obs_pool"]["x"], sc["obs_pool"]["y"], sc["obs_pool"]["radius"] = 1e6, 1e6, 0.5
    sc["scene_in"]["obs_n"] = k_obs
    stride = k_obs + (FLEET if worlds is not None else 0)
    if stride != k_obs:                   # room for the peer slots behind every scene's own entries
        pool = np.zeros((n, stride), dm.ObPoint)
        pool["x"], pool["y"], pool["radius"] = 1e6, 1e6, 0.5
        sc["obs_pool"], sc["scene_in"]["obs_off"], sc["n_obs"] = pool.reshape(-1), np.arange(n) * stride, stride
    polylines = [(ts.ring_track(dm, m, 1), True), (ts.ring_track(dm, m, 2), True)]
    tracks, pts = ts.pack(dm, polylines)
    cums = [tm.cumulative(p["x"], p["y"], True) for p, _ in polylines]
    rows = []
    for s in range(n):
        loc = sc["scene_in"]["loc"][s]
        lane = int(loc["lane_num"])
        here = cums[lane - 1][ts.SEG * (int(loc["road_num"]) - 1) + int(loc["id"][lane - 1])]
        rows.append((here + 20.0, -3.0, s, 0, lane - 1, 7, 0.9))
    pl = dm.Planner(rcfg, device=0, **rs.caps(m, n, stride))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_route(legs, rf)
    if worlds is not None:
        fm = dm.default_fleet_model()
        fm["max_peers"] = FLEET
        pl.set_fleet(list(range(0, n, FLEET_WORLD if FLEET_WORLD > 0 else 16)) + [n], fm)
    pl.set_traffic(tracks, pts, ts.actors(dm, rows))
    pl.set_episodes()
    if on:
        sp = dm.default_episode_spawn()
        sp["n_starts"], sp["contact"] = M, int(CONTACT)
        roll = lambda a: np.concatenate([np.roll(a, -k, axis=0) for k in range(1, M)]) if M > 1 else None
        pl.set_episode_spawn(sp, roll(sc["scene_in"]), roll(sc["state"]))
    if worlds:
        pl.set_episode_worlds()
    if reset:                             # last: set 0 is captured here; set k puts the vehicle 20 m ahead of start record k along its OWN track
        sets = None
        if on and M > 1:
            sets = np.zeros((M - 1, n), dm.TrafficStart)
            for k in range(1, M):
                for s in range(n):
                    loc = sc["scene_in"]["loc"][(s + k) % n]
                    sets["s"][k - 1, s] = cums[rows[s][4]][ts.SEG * (int(loc["road_num"]) - 1) + int(loc["id"][int(loc["lane_num"]) - 1])] + 20.0
        pl.set_episode_traffic(M if on else 1, sets)
    if sched:
        sm = dm.default_episode_schedule()
        sm["scope"] = 1 if sched == "pooled" else 0
        pl.set_episode_schedule(sm)
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    ended = int(pl.episode_stats()["n_episodes"].sum())
    ss = pl.episode_spawn_stats() if on else None
    spawn_run.resets = int(pl.episode_traffic_resets().sum()) if reset else 0
    spawn_run.age1 = int((pl.episode_stats()["min_age"] == 1).sum())
    spawn_run.world_ends = int(((pl.episode_stats()["last_cause"] & dm.EGO_WORLD) != 0).sum())
    if sched:
        rows = pl.episode_schedule()
        spawn_run.rows = (int(rows["n_end"].sum()), int(rows["n_fail"].sum()))
    pl.close()
    return n * steps / dt, ended, (0, 0, 0) if ss is None else (int(ss["n_contact"].sum()), int(ss["n_blocked"].sum()), int(ss["n_rejected"].sum()))


def follow_run(on):
    import route_scenes as rs
    rcfg = dm.default_config(256)
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, rcfg, m, n, seed=5, ids=(10, 250), legs=(6, 10))
    pl = dm.Planner(rcfg, device=0, **rs.caps(m, n))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_route(legs, rf)
    if on:
        pl.set_grid_follow(dm.default_grid_follow())
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    off_grid = int(((pl.ego_flags() & dm.EGO_OFF_GRID) != 0).sum())
    pl.close()
    return n * steps / dt, off_grid


def track_run(on, bias):
    """The ring of follow_run with the grid stage off and the scorecard on (for its replan count); on: the ego tracker of
    DESIGN.md §4q with the default model and curv_bias = bias."""
    import route_scenes as rs
    rcfg = dm.default_config(128)
    rcfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, rcfg, m, n, seed=5, ids=(10, 250), legs=(6, 10))
    pl = dm.Planner(rcfg, device=0, **rs.caps(m, n))
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_route(legs, rf)
    if on:
        tk = dm.default_ego_tracker()
        tk["curv_bias"] = bias
        pl.set_ego_tracker(tk)
    pl.score_begin()
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    replans, frozen = int(pl.rollout_score()["n_replans"].sum()), int((pl.ego_flags() != 0).sum())
    track_run.max_kappa = float(pl.ego_track_state()["max_kappa"].max()) if on else 0.0
    pl.close()
    return n * steps / dt, replans, frozen


TRACE = int(os.environ.get("TRACE", "0"))


def rollout_run(score=SCORE == "1", follow=False, trace=0, conflict=False, percept=False):
    pl, _ = fresh()
    if follow:
        pl.set_grid_follow(dm.default_grid_follow())
    if score:
        pl.score_begin()
    if trace > 0:
        tm = dm.default_score_trace()
        tm["depth"], tm["post"] = trace, min(int(tm["post"][0]), trace - 1)
        if os.environ.get("TRACE_TRIGGER"):          # TRACE_TRIGGER=0: plain rings that never freeze - every scene stores every tick
            tm["trigger"] = int(os.environ["TRACE_TRIGGER"])
        pl.set_score_trace(tm)
    if conflict:
        pl.set_conflict_score(dm.default_conflict())
    if percept:
        pl.set_perception(dm.default_perception())
    pl.rollout(warm, model)
    pl.sync()
    t0 = time.perf_counter()
    pl.rollout(steps, model)
    pl.sync()
    dt = time.perf_counter() - t0
    frozen = int((pl.ego_flags() != 0).sum())
    if score:
        sc = pl.rollout_score()
        rollout_run.summary = "%d ticks scored, %d scenes with a collision, worst clearance %.3f m, mean distance %.2f m" % (
            int(sc["n_ticks"][0]), int((sc["n_collision_ticks"] > 0).sum()), float(sc["min_clearance"].min()), float(sc["dist"].mean()))
    if trace > 0:                             # outside the timing: the headers, and the ring of the first frozen scene
        info = pl.score_trace_info()
        frozen_rings = np.flatnonzero(info["state"] == 2)
        got = len(pl.read_score_trace(int(frozen_rings[0]))[0]) if len(frozen_rings) else 0
        rollout_run.traced = "%d rings frozen, %d counting, %d armed; %d records written in all; the first frozen ring holds %d" % (
            len(frozen_rings), int((info["state"] == 1).sum()), int((info["state"] == 0).sum()), int(info["n_written"].sum()), got)
    if percept:                               # outside the timing
        c = pl.perception_stats()
        rollout_run.percepts = "%d entry-ticks: %d out, %d occluded, %d missed, %d detected; %d fresh, %d coasted, %d hidden; closest hidden %.3f m" % tuple(
            [int(c[f].sum()) for f in ("n_entries", "n_out", "n_occluded", "n_missed", "n_detected", "n_fresh", "n_coasted", "n_hidden")] + [float(c["min_hidden_clearance"].min())])
    if conflict:                              # outside the timing
        c = pl.conflict_score()
        rollout_run.conflicts = "%d ticks, %d scenes with a conflict, %d with a critical tick, smallest TTC %.3f s, largest DRAC %.3f m/s^2, %d ticks without history" % (
            int(c["n_ticks"][0]), int((c["n_conflict_ticks"] > 0).sum()), int((c["n_crit_ticks"] > 0).sum()), float(c["min_ttc"].min()), float(c["max_drac"].max()),
            int(c["n_no_history_ticks"].sum()))
    pl.close()
    return n * steps / dt, frozen


def streamed_run():
    pl, sc = fresh()
    snaps = []
    for _ in range(depth + 2):
        move_ego(sc, 1)
        snaps.append(dm.pinned_copy(sc["scene_in"]))
    ress = [dm.pinned_empty(n, dm.PlanningOut) for _ in range(depth)]
    shows = [dm.pinned_empty(n, dm.PlanningStatus) for _ in range(depth)]

    def loop(k):
        ids = []
        for t in range(k):
            if len(ids) == depth:
                pl.wait_tick(ids.pop(0))
            pl.update_async(snaps[t % len(snaps)])
            pl.tick()
            ids.append(pl.fetch_published_async(ress[t % depth], shows[t % depth]))
        for i in ids:
            pl.wait_tick(i)
    loop(warm)
    pl.sync()
    t0 = time.perf_counter()
    loop(steps)
    pl.sync()
    dt = time.perf_counter() - t0
    pl.close()
    return n * steps / dt


if os.environ.get("EPISODES", "0") == "1" and WORLDS:
    off, on = [], []
    for r in range(runs):
        a, ea, _ = spawn_run(True, reset=RESET, worlds=False)
        b, eb, (nc, nb, nr) = spawn_run(True, reset=RESET, worlds=True)
        off.append(a), on.append(b)
        print("run %d  %d ring egos with traffic in worlds of %d (K %d), spawn model on (M %d, contact %d, reset %d)  worlds off %.3f M ticks/s (%d episodes ended)   "
              "world episodes on %.3f M ticks/s (%d episodes ended, %d on contact, %d egos whose last cause has WORLD, %d blocked, %d rejected)" %
              (r, n, FLEET_WORLD if FLEET_WORLD > 0 else 16, FLEET, max(SPAWN, 1), int(CONTACT), int(RESET), a / 1e6, ea, b / 1e6, eb, nc, spawn_run.world_ends, nb, nr), flush=True)
    print("median  %d ring egos  world episodes off %.3f M ticks/s (spread %.3f)   on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout of each, so that one trace holds both kernels
        spawn_run(True, reset=RESET, worlds=False)
        spawn_run(True, reset=RESET, worlds=True)
    sys.exit(0)
if FLEET > 0:
    off, on = [], []
    for r in range(runs):
        a, na = fleet_run(False)
        b, nb = fleet_run(True)
        off.append(a), on.append(b)
        print("run %d  %d scenes  fleet off (padded, obs_n %.1f) %.3f M ticks/s   fleet on (K %d, worlds of %d, obs_n %.1f) %.3f M ticks/s" %
              (r, n, na, a / 1e6, FLEET, FLEET_WORLD if FLEET_WORLD > 0 else n, nb, b / 1e6), flush=True)
    print("median  %d scenes  fleet off %.3f M ticks/s (spread %.3f)   fleet on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more fleet rollout alone
        fleet_run(True)
    sys.exit(0)
if TRAFFIC > 0:
    off, on = [], []
    for r in range(runs):
        a, fa = traffic_run(False)
        b, fb = traffic_run(True)
        off.append(a), on.append(b)
        print("run %d  %d scenes, obs_n %d  traffic off %.3f M ticks/s (%d frozen at the end)   traffic on (%d actors per scene) %.3f M ticks/s (%d frozen)" %
              (r, n, n_obs, a / 1e6, fa, TRAFFIC, b / 1e6, fb), flush=True)
    print("median  %d scenes  %s off %.3f M ticks/s (spread %.3f)   %s on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, ("manoeuvres (traffic%s on)" % (" and following" if REACT else "")) if MANOEUVRE else "following (traffic on)" if REACT else "traffic", statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6,
           "manoeuvres" if MANOEUVRE else "following" if REACT else "traffic", statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout with traffic alone
        traffic_run(True)
    sys.exit(0)
if os.environ.get("EPISODES", "0") == "1" and SCHEDULE:
    assert SCHEDULE in ("pooled", "scene") and SPAWN > 0
    off, on = [], []
    for r in range(runs):
        a, ea, _ = spawn_run(True, reset=RESET)
        b, eb, (nc, _, _) = spawn_run(True, reset=RESET, sched=SCHEDULE)
        off.append(a), on.append(b)
        print("run %d  %d ring egos with traffic, spawn model on (M %d, contact %d, reset %d)  schedule off %.3f M ticks/s (%d episodes ended)   "
              "schedule on (%s) %.3f M ticks/s (%d episodes ended, %d on contact; rows: %d counted, %d failures)" %
              ((r, n, SPAWN, int(CONTACT), int(RESET), a / 1e6, ea, SCHEDULE, b / 1e6, eb, nc) + spawn_run.rows), flush=True)
    print("median  %d ring egos  schedule off %.3f M ticks/s (spread %.3f)   schedule on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout with the schedule alone
        spawn_run(True, reset=RESET, sched=SCHEDULE)
    sys.exit(0)
if os.environ.get("EPISODES", "0") == "1" and RESET:
    off, on = [], []
    for r in range(runs):
        a, ea, _ = spawn_run(True)
        a1 = spawn_run.age1
        b, eb, (nc, _, _) = spawn_run(True, reset=True)
        off.append(a), on.append(b)
        print("run %d  %d ring egos with traffic, spawn model on (M %d, contact %d)  reset off %.3f M ticks/s (%d episodes ended, %d egos with an episode of age 1)   "
              "reset on %.3f M ticks/s (%d episodes ended, %d on contact, %d egos with an episode of age 1, %d vehicle resets)" %
              (r, n, max(SPAWN, 1), int(CONTACT), a / 1e6, ea, a1, b / 1e6, eb, nc, spawn_run.age1, spawn_run.resets), flush=True)
    print("median  %d ring egos  reset off %.3f M ticks/s (spread %.3f)   reset on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout with the reset alone
        spawn_run(True, reset=True)
    sys.exit(0)
if os.environ.get("EPISODES", "0") == "1" and (SPAWN > 0 or CONTACT):
    off, on = [], []
    for r in range(runs):
        a, ea, _ = spawn_run(False)
        b, eb, (nc, nb, nr) = spawn_run(True)
        off.append(a), on.append(b)
        print("run %d  %d ring egos with traffic, obs_n %s  episodes alone %.3f M ticks/s (%d episodes ended)   spawn model on (M %d, contact %d) %.3f M ticks/s "
              "(%d episodes ended, %d on contact, %d blocked restarts, %d rejected records)" %
              (r, n, os.environ.get("OBS", "1"), a / 1e6, ea, max(SPAWN, 1), int(CONTACT), b / 1e6, eb, nc, nb, nr), flush=True)
    print("median  %d ring egos  episodes alone %.3f M ticks/s (spread %.3f)   spawn model on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout with the spawn model alone
        spawn_run(True)
    sys.exit(0)
if os.environ.get("EPISODES", "0") == "1" and LOG > 0:
    off, on = [], []
    for r in range(runs):
        a, _, ea = episodes_run(True)
        b, _, eb = episodes_run(True, LOG)
        off.append(a), on.append(b)
        print("run %d  %d ring egos, one-leg routes, episodes on%s  log off %.3f M ticks/s (%d episodes ended)   log on (cap %d) %.3f M ticks/s (%d episodes ended; "
              "%d records appended, %d read, %d lost)" % ((r, n, ", scorecard on" if SCORE == "1" else "", a / 1e6, ea, LOG, b / 1e6, eb) + episodes_run.logged), flush=True)
    print("median  %d ring egos  log off %.3f M ticks/s (spread %.3f)   log on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout with the log alone
        episodes_run(True, LOG)
    sys.exit(0)
if os.environ.get("EPISODES", "0") == "1":
    off, on = [], []
    for r in range(runs):
        a, fa, _ = episodes_run(False)
        b, fb, eb = episodes_run(True)
        off.append(a), on.append(b)
        print("run %d  %d ring egos, one-leg routes  episodes off %.3f M ticks/s (%d frozen at the end)   episodes on %.3f M ticks/s (%d frozen, %d episodes ended)" %
              (r, n, a / 1e6, fa, b / 1e6, fb, eb), flush=True)
    print("median  %d ring egos  episodes off %.3f M ticks/s (spread %.3f)   episodes on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout with episodes alone
        episodes_run(True)
    sys.exit(0)
if os.environ.get("ROUTE", "0") == "1":
    off, on = [], []
    for r in range(runs):
        a, fa = route_run(False)
        b, fb = route_run(True)
        off.append(a), on.append(b)
        print("run %d  %d ring egos  route off %.3f M ticks/s (%d frozen at the end)   route on %.3f M ticks/s (%d frozen)" % (r, n, a / 1e6, fa, b / 1e6, fb), flush=True)
    print("median  %d ring egos  route off %.3f M ticks/s (spread %.3f)   route on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more routed rollout alone
        route_run(True)
    sys.exit(0)
if os.environ.get("TRACK", "0") == "1":
    bias = float(os.environ.get("TRACK_BIAS", "0"))
    off, on = [], []
    for r in range(runs):
        a, ra, fa = track_run(False, bias)
        b, rb, fb = track_run(True, bias)
        off.append(a), on.append(b)
        print("run %d  %d ring egos, scorecard on  tracker off %.3f M ticks/s (%d replans, %d frozen)   tracker on, bias %g: %.3f M ticks/s (%d replans, %d frozen, max |kappa| %.4f)" %
              (r, n, a / 1e6, ra, fa, bias, b / 1e6, rb, fb, track_run.max_kappa), flush=True)
    print("median  %d ring egos  tracker off %.3f M ticks/s (spread %.3f)   tracker on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: k_advance_route<false> and <true> in one trace
        track_run(False, bias)
        track_run(True, bias)
    sys.exit(0)
if os.environ.get("FOLLOW", "0").startswith("trace_"):
    on = os.environ["FOLLOW"] == "trace_on"
    a, fa = follow_run(on)
    b, fb = rollout_run(False, follow=on)
    print("following %s  %d ring egos %.3f M ticks/s (%d OFF_GRID)   %d generated scenes %.3f M ticks/s (%d frozen)" % ("on" if on else "off", n, a / 1e6, fa, n, b / 1e6, fb), flush=True)
    sys.exit(0)
if os.environ.get("FOLLOW", "0") == "1":
    off, on = [], []
    for r in range(runs):
        a, fa = follow_run(False)
        b, fb = follow_run(True)
        off.append(a), on.append(b)
        print("run %d  %d ring egos, grid stage on  follow off %.3f M ticks/s (%d OFF_GRID at the end)   follow on %.3f M ticks/s (%d OFF_GRID)" % (r, n, a / 1e6, fa, b / 1e6, fb), flush=True)
    print("median  %d ring egos  follow off %.3f M ticks/s (spread %.3f)   follow on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more following rollout alone
        follow_run(True)
    sys.exit(0)
if CONFLICT:
    off, on = [], []
    for r in range(runs):
        a, _ = rollout_run(True)
        b, _ = rollout_run(True, conflict=True)
        off.append(a), on.append(b)
        print("run %d  %d scenes, scorecard on  conflict off %.3f M ticks/s   conflict on %.3f M ticks/s (%s)" % (r, n, a / 1e6, b / 1e6, rollout_run.conflicts), flush=True)
    print("median  %d scenes, scorecard on  conflict off %.3f M ticks/s (spread %.3f)   conflict on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: both kernels in one trace
        rollout_run(True)
        rollout_run(True, conflict=True)
    sys.exit(0)
if PERCEPT:
    off, on = [], []
    for r in range(runs):
        a, _ = rollout_run()
        b, _ = rollout_run(percept=True)
        off.append(a), on.append(b)
        print("run %d  %d scenes  perception off %.3f M ticks/s   perception on %.3f M ticks/s (%s)" % (r, n, a / 1e6, b / 1e6, rollout_run.percepts), flush=True)
    print("median  %d scenes  perception off %.3f M ticks/s (spread %.3f)   perception on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: both snapshot kernels in one trace
        rollout_run()
        rollout_run(percept=True)
    sys.exit(0)
if SCORE == "1" and TRACE > 0:
    off, on = [], []
    for r in range(runs):
        a, _ = rollout_run(True)
        b, _ = rollout_run(True, trace=TRACE)
        off.append(a), on.append(b)
        print("run %d  %d scenes, scorecard on  trace off %.3f M ticks/s   trace on (depth %d) %.3f M ticks/s (%s)" % (r, n, a / 1e6, TRACE, b / 1e6, rollout_run.traced), flush=True)
    print("median  %d scenes, scorecard on  trace off %.3f M ticks/s (spread %.3f)   trace on %.3f M ticks/s (spread %.3f)   ratio %.3f" %
          (n, statistics.median(off) / 1e6, (max(off) - min(off)) / 1e6, statistics.median(on) / 1e6, (max(on) - min(on)) / 1e6,
           statistics.median(on) / statistics.median(off)), flush=True)
    if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: both kernels in one trace
        rollout_run(True)
        rollout_run(True, trace=TRACE)
    sys.exit(0)
if SCORE == "ab":
    off, on = [], []
    for r in range(runs):
        a, _ = rollout_run(False)
        b, _ = rollout_run(True)
        off.append(a), on.append(b)
        print("run %d  %d scenes  rollout %.3f M ticks/s   scored rollout %.3f M ticks/s" % (r, n, a / 1e6, b / 1e6), flush=True)
    print("median  %d scenes  rollout %.3f M ticks/s   scored rollout %.3f M ticks/s   ratio %.3f   (%s)" %
          (n, statistics.median(off) / 1e6, statistics.median(on) / 1e6, statistics.median(on) / statistics.median(off), rollout_run.summary), flush=True)
    sys.exit(0)
ro, stv = [], []
for r in range(runs):
    a, frozen = rollout_run()
    b = streamed_run()
    ro.append(a), stv.append(b)
    print("run %d  %d scenes  rollout %.3f M ticks/s (%d scenes frozen at the end)   host-fed streamed %.3f M ticks/s" % (r, n, a / 1e6, frozen, b / 1e6), flush=True)
print("median  %d scenes  rollout %.3f M ticks/s   host-fed streamed %.3f M ticks/s   ratio %.3f" %
      (n, statistics.median(ro) / 1e6, statistics.median(stv) / 1e6, statistics.median(ro) / statistics.median(stv)), flush=True)
if SCORE == "1":
    print("scorecard:", rollout_run.summary, flush=True)
if os.environ.get("ONE_ROLLOUT"):        # for rocprofv3 --kernel-trace --stats: one more rollout alone
    rollout_run()
