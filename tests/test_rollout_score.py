"""Rollout scorecard (pp_score_begin / pp_score_end / pp_get_rollout_score).

CPU: the ABI mirror, hand-derived known answers of the numpy model (tests/rollout_score_model.py) with their arithmetic, and
the collision scene of the device's known answer run as a closed loop on the CPU (oracle tick + ego model + score model).
GPU: the device against that model after every tick of a closed loop, BYTE FOR BYTE (§4d specifies every field exactly);
scoring on against scoring off; pp_rollout against its parts; the collision scene in closed form; ticks without an advance;
the lifecycle of the call group."""
import math

import numpy as np
import pytest

import coupling_backends as cb
import ego_model as em
import rollout_score_model as sm

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirror(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(21) == dm.RolloutScore.itemsize
    assert dm.RolloutScore.itemsize % 8 == 0 and dm.RolloutScore.itemsize > 0
    assert hasattr(lib, "pp_score_begin") and hasattr(lib, "pp_score_end") and hasattr(lib, "pp_get_rollout_score")
    assert (sm.G_STATUS_COUNT, sm.G_INTERNAL, sm.MAX_LATTICE) == (dm.G_STATUS_COUNT, dm.G_INTERNAL, dm.MAX_LATTICE)


def _one(cfg, x, y, v, obs=(), behavior=1, afresh=0, ob_flag=0, desaccVd=0, flags=0, grid=None):
    """One scored tick of one scene (coupling_backends.Tick): ego at (x, y) with speed v, obstacles (x, y, radius)."""
    return cb.tick(cfg, [(x, y, v, list(obs))], behavior=behavior, afresh=afresh, ob_flag=ob_flag, desaccVd=desaccVd, flags=flags, grid=grid)


def _runner(name, log=None):
    return cb.ScoreRunner(cb.ScoreModelBackend() if name == "model" else cb.ScoreDeviceBackend(), log)


@pytest.fixture()
def cfg(dm):
    c = cb.config()                                                          # (grid stage, decision stage, moving obstacles off: the device leg)
    assert float(c["Vehicle_Width"][0]) == 1.8 and 0.5 * 1.8 == 0.9          # the ego disc: radius 0.9 m
    return c


# The known answers are written once against a runner of tests/coupling_backends.py: the numpy model (CPU) and k_score_ego inside a
# tick of crafted records (test_kat_on_the_device), where every record is also held byte for byte against the model folded over
# the device's own PlanOut and SceneState.  run(cfg, dt, ticks) -> .start, .after[k]: the records before the first / after tick k.
def _kat_start_values_and_empty_slice(dm, cfg, run):
    # a tick without obstacles, then one whose only distance is a NaN
    res = run(cfg, 0.1, [_one(cfg, 10.0, 0.0, 36.0), _one(cfg, 10.0, 0.0, 36.0, obs=[(math.nan, 0.0, 0.5)])])
    r = res.start
    assert (float(r["min_clearance"][0]), int(r["min_clearance_tick"][0]), int(r["min_clearance_obs"][0])) == (math.inf, -1, -1)
    assert int(r["first_collision_tick"][0]) == -1 and int(r["n_ticks"][0]) == 0
    # a tick without obstacles has no clearance: the three fields and the collision fields stay, the tick is counted
    r = res.after[0]
    assert (float(r["min_clearance"][0]), int(r["min_clearance_tick"][0]), int(r["min_clearance_obs"][0])) == (math.inf, -1, -1)
    assert (int(r["first_collision_tick"][0]), int(r["n_collision_ticks"][0]), int(r["n_ticks"][0])) == (-1, 0, 1)
    # ... and so has one whose only distance is a NaN
    r = res.after[1]
    assert (float(r["min_clearance"][0]), int(r["min_clearance_tick"][0]), int(r["min_clearance_obs"][0])) == (math.inf, -1, -1)
    assert int(r["n_ticks"][0]) == 2


def _kat_obstacle_abeam_tie_and_nan(dm, cfg, run):
    # straight drive along +x at y = 0, one obstacle of radius 0.5 three metres to the left of x = 10: abeam the centre
    # distance is the offset, d = 3 - 0.5, clearance = offset - radius - 0.9 = 1.6; one metre before it sqrt(1 + 9) - 0.5 - 0.9
    ob = [(10.0, 3.0, 0.5)]
    res = run(cfg, 0.1, [_one(cfg, x, 0.0, 36.0, obs=ob) for x in (9.0, 10.0, 11.0, 10.0)])
    r = res.after[0]
    assert float(r["min_clearance"][0]) == math.sqrt(1.0 * 1.0 + 3.0 * 3.0) - 0.5 - 0.9
    r = res.after[1]
    assert float(r["min_clearance"][0]) == 3.0 - 0.5 - 0.9 and abs(float(r["min_clearance"][0]) - 1.6) < 1e-15
    assert (int(r["min_clearance_tick"][0]), int(r["min_clearance_obs"][0])) == (1, 0)
    r = res.after[2]                                              # past it: the minimum and its tick stay
    assert float(r["min_clearance"][0]) == 3.0 - 0.5 - 0.9 and int(r["min_clearance_tick"][0]) == 1
    assert int(r["n_collision_ticks"][0]) == 0 and int(r["first_collision_tick"][0]) == -1
    # the same clearance again later does not move the tick (strict <)
    r = res.after[3]
    assert int(r["min_clearance_tick"][0]) == 1
    # two obstacles at the same distance (left and right of the ego): the first index; a NaN in front of them is ignored
    r = run(cfg, 0.1, [_one(cfg, 10.0, 0.0, 36.0, obs=[(10.0, 5.0, 0.5), (10.0, 3.0, 0.5), (10.0, -3.0, 0.5)])]).after[0]
    assert (float(r["min_clearance"][0]), int(r["min_clearance_obs"][0])) == (3.0 - 0.5 - 0.9, 1)
    r = run(cfg, 0.1, [_one(cfg, 10.0, 0.0, 36.0, obs=[(math.nan, 0.0, 0.5), (10.0, -3.0, 0.5), (10.0, 3.0, 0.5)])]).after[0]
    assert (float(r["min_clearance"][0]), int(r["min_clearance_obs"][0])) == (3.0 - 0.5 - 0.9, 1)
    # the radius is an f32 widened to double: 1.7f = 1.7000000476837158
    r = run(cfg, 0.1, [_one(cfg, 10.0, 0.0, 36.0, obs=[(10.0, 2.5, 1.7)])]).after[0]
    assert float(r["min_clearance"][0]) == 2.5 - float(np.float32(1.7)) - 0.9 and float(r["min_clearance"][0]) < -0.1


def _kat_collision_exactly_at_zero(dm, cfg, run):
    # a point obstacle (radius 0) exactly 0.9 m beside the ego: sqrt(0*0 + 0.9*0.9) = 0.9 (sqrt(x*x) = |x| in IEEE arithmetic),
    # clearance = 0.9 - 0 - 0.9 = 0: touching counts as a collision (<=); one ulp further away it does not
    res = run(cfg, 0.1, [_one(cfg, 10.0, 0.0, 36.0, obs=[(10.0, y, 0.0)]) for y in (math.nextafter(0.9, 1.0), 0.9, 0.5)])
    r = res.after[0]
    assert float(r["min_clearance"][0]) > 0 and int(r["n_collision_ticks"][0]) == 0 and int(r["first_collision_tick"][0]) == -1
    r = res.after[1]
    assert float(r["min_clearance"][0]) == 0.0
    assert (int(r["first_collision_tick"][0]), int(r["n_collision_ticks"][0]), int(r["min_clearance_tick"][0])) == (1, 1, 1)
    r = res.after[2]                                                              # deeper: counted, the first tick stays
    assert (int(r["first_collision_tick"][0]), int(r["n_collision_ticks"][0]), int(r["min_clearance_tick"][0])) == (1, 2, 2)
    assert float(r["min_clearance"][0]) == 0.5 - 0.0 - 0.9


def _kat_distance_and_speed_ramp(dm, cfg, run):
    # three ticks: (0, 0) at 10 km/h, (3, 4) at 13.6 km/h, (9, 12) at 10 km/h, dt 0.1 s.
    # dist = sqrt(9 + 16) + sqrt(36 + 64) = 5 + 10 = 15 m; rise (13.6 - 10)/3.6/0.1 = 10 m/s^2, fall the same; max speed 13.6
    # ... then a NaN speed (the Planning kernel only scales its aim distance by it: every loop over it is bounded by a count, and
    # the CPU oracle returns for the record: test_crafted_records_pass_the_cpu_oracle) and 5 km/h standing still
    res = run(cfg, 0.1, [_one(cfg, 0.0, 0.0, 10.0), _one(cfg, 3.0, 4.0, 13.6), _one(cfg, 9.0, 12.0, 10.0), _one(cfg, 9.0, 12.0, math.nan),
                         _one(cfg, 9.0, 12.0, 5.0)])
    r = res.after[0]
    assert (float(r["dist"][0]), float(r["max_acc"][0]), float(r["max_dec"][0]), float(r["max_speed"][0])) == (0.0, 0.0, 0.0, 10.0)
    r = res.after[1]
    assert float(r["dist"][0]) == 5.0 and float(r["max_acc"][0]) == (13.6 - 10.0) / 3.6 / 0.1 and float(r["max_dec"][0]) == 0.0
    r = res.after[2]
    assert float(r["dist"][0]) == 15.0 and float(r["max_speed"][0]) == 13.6
    assert float(r["max_acc"][0]) == (13.6 - 10.0) / 3.6 / 0.1 and abs(float(r["max_acc"][0]) - 10.0) < 1e-12
    assert float(r["max_dec"][0]) == -((10.0 - 13.6) / 3.6 / 0.1) and abs(float(r["max_dec"][0]) - 10.0) < 1e-12
    assert (float(r["last_pos"]["x"][0]), float(r["last_pos"]["y"][0]), float(r["last_speed"][0]), int(r["n_ticks"][0])) == (9.0, 12.0, 10.0, 3)
    # a NaN speed never replaces a maximum
    r = res.after[4]
    assert float(r["max_speed"][0]) == 13.6 and abs(float(r["max_acc"][0]) - 10.0) < 1e-12 and abs(float(r["max_dec"][0]) - 10.0) < 1e-12
    assert float(r["dist"][0]) == 15.0                                    # standing still adds 0


def _kat_counters_and_histograms(dm, cfg, run):
    """behavior_ticks holds on both backends: with the decision stage off PlanOut.dec is the caller's record, out-of-range values
    included (kernels_r.hpp, `po.dec = dec`; on the oracle: test_crafted_records_pass_the_cpu_oracle).  Model leg only: the counters
    of a crafted PlanOut / SceneState (n_replans, n_ob_flag, n_desacc, ego_flags) and the grid half with its status clamp - no API
    hands the device such records, and k_score_grid has no wave structure."""
    go = np.zeros(1, dm.GridOut)
    nl = int(cfg["n_lattice"][0])
    assert nl == 16
    # behaviour 1, 6 in their bins; -3 clamps to 0, 11 to 7.  Status 0 and 5 in their bins; 99 and -1 count under G_INTERNAL.
    # The grid path is candidate 16 of 17: it won only on the tick with n_candidates = 17 and best = 16 - with 16 candidates
    # (no path found) the last Bezier candidate, index 15 = n_candidates - 1, is not the grid path.
    ticks = [(1, 0, 17, 16, 1, 0, 0), (6, 5, 17, 3, 0, 1, 1), (-3, 99, 16, 15, 1, 1, 0), (11, -1, 17, 16, 0, 0, 1)]
    crafted = []
    for k, (beh, status, nc, best, afresh, ob_flag, dv) in enumerate(ticks):
        go["status"], go["n_candidates"], go["best_candidate"] = status, nc, best
        crafted.append(_one(cfg, 0.0, 0.0, 0.0, behavior=beh, afresh=afresh, ob_flag=ob_flag, desaccVd=dv, flags=k, grid=go.copy()))
    crafted.append(_one(cfg, 0.0, 0.0, 0.0))
    res = run(cfg, 0.1, crafted)
    r = res.after[3]
    assert r["behavior_ticks"][0].tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
    assert int(r["n_ticks"][0]) == 4
    if run.name == "model":
        want = [0] * dm.G_STATUS_COUNT
        want[dm.G_FOUND], want[dm.G_PATH_TRUNC], want[dm.G_INTERNAL] = 1, 1, 2
        assert r["grid_status_ticks"][0].tolist() == want
        assert (int(r["n_grid_ticks"][0]), int(r["n_grid_path_candidate"][0]), int(r["n_ticks"][0])) == (4, 2, 4)
        assert (int(r["n_replans"][0]), int(r["n_ob_flag"][0]), int(r["n_desacc"][0]), int(r["ego_flags"][0])) == (2, 2, 2, 3)
    # a tick without the grid stage leaves the grid half alone
    r = res.after[4]
    assert int(r["n_ticks"][0]) == 5 and r["behavior_ticks"][0].tolist() == [1, 2, 0, 0, 0, 0, 1, 1]
    if run.name == "model":
        assert (int(r["n_grid_ticks"][0]), int(r["n_ticks"][0])) == (4, 5)


KATS = [_kat_start_values_and_empty_slice, _kat_obstacle_abeam_tie_and_nan, _kat_collision_exactly_at_zero, _kat_distance_and_speed_ramp,
        _kat_counters_and_histograms]


def test_kat_start_values_and_empty_slice(dm, cfg):
    _kat_start_values_and_empty_slice(dm, cfg, _runner("model"))


def test_kat_obstacle_abeam_tie_and_nan(dm, cfg):
    _kat_obstacle_abeam_tie_and_nan(dm, cfg, _runner("model"))


def test_kat_collision_exactly_at_zero(dm, cfg):
    _kat_collision_exactly_at_zero(dm, cfg, _runner("model"))


def test_kat_distance_and_speed_ramp(dm, cfg):
    _kat_distance_and_speed_ramp(dm, cfg, _runner("model"))


def test_kat_counters_and_histograms(dm, cfg):
    _kat_counters_and_histograms(dm, cfg, _runner("model"))


def test_crafted_records_pass_the_cpu_oracle(dm, oracle, cfg):
    """What the device leg sends through a real tick, on the CPU oracle first: a NaN ego speed, behaviours outside 0 .. 7, and
    obstacles that are NaN, infinite or 200 to a scene.  The tick returns, and PlanOut.dec.behavior is the caller's value."""
    inf = math.inf
    odd = [(math.nan, 0.0, 0.5), (inf, 0.0, 0.5), (inf, 0.0, inf), (10.0, 3.0, math.nan), (-inf, inf, 0.0)] + [(10.0 + 0.25 * j, 3.0, 0.5) for j in range(195)]
    sc = cb.road(cfg)
    for t in (_one(cfg, 9.0, 12.0, math.nan), _one(cfg, 0.0, 0.0, 0.0, behavior=-3), _one(cfg, 0.0, 0.0, 0.0, behavior=11), _one(cfg, 10.0, 0.0, 36.0, obs=odd)):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=t.si, obs_pool=t.pool, mot_pool=None, n_obs=len(t.pool)), sc["state"].copy(), want_grid=False)
        assert int(plan["dec"]["behavior"][0]) == int(t.si["dec"]["behavior"][0])


@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg, kat):
    """The known answers above on k_score_ego, each record also held byte for byte against the model (coupling_backends)."""
    kat(dm, cfg, _runner("device"))


@gpu
def test_kat_batch_equals_each_case_alone(dm, cfg):
    """Every known answer once more on the device, logged, then as distinct scenes of one launch per group of calls that can share
    one (coupling_backends.score_batched): more than one block, no multiple of four; every scene gives the bytes it gave alone."""
    log = []
    run = _runner("device", log)
    for kat in KATS:
        kat(dm, cfg, run)
    sizes = cb.score_batched(cb.ScoreDeviceBackend(), log)
    print(f"{len(log)} calls in batches of {sizes}")
    assert sum(sizes) >= len(log) and all(n % 4 != 0 and n > 4 for n in sizes)


# ---- the collision scene: the speed-ramp road with one obstacle beside the lane ----------------------------------
RAMP_TICKS = 50
OB_AHEAD, OB_LEFT, OB_RADIUS = 10.0, 2.5, 1.75          # abeam: 2.5 - 1.75 - 0.9 = -0.15 m; 1.75 is exact in f32


def _ramp_scene(dm):
    """test_known_answer_speed_ramp's road (decision stage off, force_replan, 0 -> 30 km/h) plus one static obstacle 10 m
    ahead of the start, 2.5 m to the left of the lane centre: outside the planner's corridor, inside the ego disc abeam."""
    import lanechange_scenes as lcs
    cfg = dm.default_config(128)
    cfg["decision_stage"], cfg["force_replan"] = 0, 1
    sc = lcs.make_scene(dm, cfg, lane_num=2, obstacles=[(2, OB_AHEAD, OB_LEFT)])
    sc["obs_pool"]["radius"][0] = OB_RADIUS
    sc["scene_in"]["dec"]["velocity_expect"], sc["scene_in"]["dec"]["behavior"], sc["scene_in"]["dec"]["target_lanenum"] = 30.0, 1, 2
    sc["scene_in"]["loc"]["velocity"] = 0.0
    x0 = float(sc["scene_in"]["loc"]["globalpoint"]["x"][0])
    sc["scene_in"]["grid_origin"]["x"] = x0 - 2.0
    return cfg, sc, x0


def _ramp_closed_form():
    """Positions along the lane after k advances, from the closed form of the ramp (default model: dt 0.1 s, 2 m/s^2): the speed
    rises 0.72 km/h per tick to 30 (v_k = min(0.72 k, 30)), a tick covers (v_{k-1} + v_k)/2 / 3.6 * 0.1 m.  For k <= 41 that is
    0.01 k^2 m: 9.00 m at k = 30, 9.61 at 31, 10.24 at 32, 10.89 at 33.  With the obstacle 10 m ahead and 2.5 m to the side,
    radius 1.75 + 0.9: contact while |dx| <= sqrt(2.65^2 - 2.5^2) = 0.8789 m, i.e. at k = 31 (0.39) and k = 32 (0.24) only
    (k = 30: 1.00, k = 33: 0.89)."""
    v = [min(0.72 * k, 30.0) for k in range(RAMP_TICKS + 1)]
    X = [0.0]
    for k in range(1, RAMP_TICKS + 1):
        X.append(X[-1] + 0.5 * (v[k - 1] + v[k]) / 3.6 * 0.1)
    cl = [math.sqrt((OB_AHEAD - xk) * (OB_AHEAD - xk) + OB_LEFT * OB_LEFT) - OB_RADIUS - 0.9 for xk in X]
    return X, cl


def _check_ramp_record(r, n_ticks_scored=RAMP_TICKS + 1):
    """One RolloutScore record of the collision scene against the closed form.  The tick indices and counts are exact.  The ego
    follows Bezier paths that start at its pose, so its positions agree with the closed form to rounding only; the bound is the
    1e-6 m that test_known_answer_speed_ramp holds the same closed form to, and no closed-form clearance is that close to 0."""
    X, cl = _ramp_closed_form()
    assert abs(X[30] - 9.0) < 1e-9 and abs(X[31] - 9.61) < 1e-9 and abs(X[32] - 10.24) < 1e-9 and abs(X[33] - 10.89) < 1e-9
    hits = [k for k, c in enumerate(cl) if c <= 0]
    assert hits == [31, 32] and min(abs(c) for c in cl) > 1e-3
    k_min = int(np.argmin(cl))
    assert k_min == 32 and abs(cl[32] - (math.sqrt(0.24 * 0.24 + 6.25) - 2.65)) < 1e-12
    assert int(r["n_ticks"]) == n_ticks_scored
    assert (int(r["first_collision_tick"]), int(r["n_collision_ticks"])) == (31, 2)
    assert (int(r["min_clearance_tick"]), int(r["min_clearance_obs"])) == (32, 0)
    assert abs(float(r["min_clearance"]) - cl[32]) <= 1e-6
    assert abs(float(r["dist"]) - X[RAMP_TICKS]) <= 1e-6 and abs(X[RAMP_TICKS] - 874.92 / 3.6 * 0.1) < 1e-9
    assert float(r["max_speed"]) == 30.0
    # 0.72 km/h per tick = 2 m/s^2 exactly as the model limits it; the speed never falls
    assert abs(float(r["max_acc"]) - 2.0) < 1e-9 and float(r["max_dec"]) == 0.0
    assert int(r["n_ob_flag"]) == 0 and int(r["n_replans"]) == n_ticks_scored and int(r["ego_flags"]) == 0
    assert r["behavior_ticks"].tolist() == [0, n_ticks_scored, 0, 0, 0, 0, 0, 0]


def test_collision_scene_closed_loop_on_the_cpu(dm, oracle):
    """Oracle tick + ego model + score model, 1 + 50 ticks: the scene does what the device test says - the plan never sees
    the obstacle (ob_flag 0 on every tick), the ego disc overlaps it on ticks 31 and 32."""
    cfg, sc, x0 = _ramp_scene(dm)
    model = dm.default_ego_model()
    st = sc["state"].copy()
    sin, flags = sc["scene_in"].copy(), np.zeros(1, np.int32)
    r = sm.new_scores(dm.RolloutScore, 1)
    for t in range(RAMP_TICKS + 1):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=sin), st, want_grid=False)
        assert int(plan["ob_flag"][0]) == 0, f"tick {t}: the planner sees the obstacle"
        sm.fold(r, cfg, float(model["dt"][0]), sin, plan, st, sc["obs_pool"], flags)
        sin, flags, _ = em.advance(cfg, model, sin, plan, st, flags, sc["lane_pool"])
    assert abs(float(r["last_pos"]["x"][0]) - x0 - 874.92 / 3.6 * 0.1) <= 1e-6
    _check_ramp_record(r[0])


# ---------------------------------------------------------------------------------------------------------------
# GPU
TICKS = 30


def _planner(dm, cfg, sc, n, n_obs, with_motion=False):
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=max(n * n_obs, 1))
    pl.set_scenes(sc, with_motion=with_motion)
    pl.set_state(sc["state"])
    return pl


def _same(a, b, what):
    assert a.tobytes() == b.tobytes(), what + ": " + ", ".join(f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes())


@gpu
@pytest.mark.parametrize("which", ["c1", "dyn"])
def test_step_check_against_the_model(dm, which):
    """A 30-tick closed loop with everything the device read and wrote captured per tick; the model folded over the captured
    ticks equals rollout_score() after EVERY tick, byte for byte."""
    n, first, je, dyn = {"c1": (1024, 0, 0, 0), "dyn": (256, 5000, 8, 1)}[which]
    cfg = dm.default_config(512)
    cfg["dynamic_obstacles"] = dyn
    n_obs = 64
    sc = dm.gen_scenes(cfg, first, n, n_obs, junction_every=je)
    pl = _planner(dm, cfg, sc, n, n_obs, with_motion=bool(dyn))
    model = dm.default_ego_model()
    dt = float(model["dt"][0])
    plan_p, grid_p = dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut)
    pl.score_begin()
    want = sm.new_scores(dm.RolloutScore, n)
    _same(pl.rollout_score(), want, "before the first tick")
    st_before, sin, flags = sc["state"], pl.get_scene_in(), np.zeros(n, np.int32)
    for t in range(TICKS + 1):
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p, grid_p)) == 0
        plan, grid, st = np.array(plan_p), np.array(grid_p), pl.get_state()
        now = sm.snapshot(cfg, sin, st_before, sc["obs_pool"], sc["mot_pool"] if dyn else None)
        sm.fold(want, cfg, dt, sin, plan, st, now, flags, grid)
        _same(pl.rollout_score(), want, f"tick {t}")
        if t < TICKS:
            pl.advance_async(model)
            sin, flags, st_before = pl.get_scene_in(), pl.ego_flags(), st
    got = pl.rollout_score()
    pl.close()
    fin = np.isfinite(got["min_clearance"])
    print(f"{which}: finite clearance in {int(fin.sum())} of {n} scenes, smallest {got['min_clearance'].min()!r}, collisions in "
          f"{int((got['n_collision_ticks'] > 0).sum())}, replans {int(got['n_replans'].sum())}, grid status {got['grid_status_ticks'].sum(axis=0).tolist()}, "
          f"grid path won {int(got['n_grid_path_candidate'].sum())}, moved {float(got['dist'].mean())!r} m on average, flags {np.bincount(got['ego_flags'], minlength=16).tolist()}")
    assert fin.any() and (got["n_replans"] > 0).any() and (got["dist"] > 0).any()
    assert (got["n_ticks"] == TICKS + 1).all() and (got["n_grid_ticks"] == TICKS + 1).all()
    assert (got["grid_status_ticks"].sum(axis=1) == got["n_grid_ticks"]).all()
    assert (got["behavior_ticks"].sum(axis=1) == got["n_ticks"]).all()
    if dyn:                                             # the obstacles did move: the snapshot of a late tick is not the pool
        assert sm.snapshot(cfg, sin, st_before, sc["obs_pool"], sc["mot_pool"])["x"].tobytes() != sc["obs_pool"]["x"].tobytes()


def _rollout_outputs(dm, cfg, sc, n, n_obs, K, score, whole=True, read_mid=False):
    pl = _planner(dm, cfg, sc, n, n_obs)
    model = dm.default_ego_model()
    if score:
        pl.score_begin()
    trace = None
    if whole:
        _, trace = pl.rollout(K, model, trace=True)
    else:
        pl.tick()
        for t in range(K):
            pl.advance_async(model)
            pl.tick()
            if read_mid and score and t % 4 == 1:
                mid = pl.rollout_score()                # a host wait in the middle of the run
                assert (mid["n_ticks"] == t + 2).all()
    pl.sync()
    out = dict(PlanOut=pl.get_plan(), GridOut=pl.get_grid_out(), SceneState=pl.get_state(), SceneIn=pl.get_scene_in(), flags=pl.ego_flags())
    if trace is not None:
        out["EgoTrace"] = np.array(trace)
    if score:
        out["score"] = pl.rollout_score()
    pl.close()
    return out


@gpu
@pytest.mark.parametrize("n", [128, 1024])
def test_scoring_changes_no_output(dm, n):
    """The same rollout with scoring on and off: identical PlanOut, GridOut, SceneState, SceneIn, ego flags and EgoTrace, below
    pipeline_min (one stream) and above it (piped)."""
    K, n_obs = 12, 32
    cfg = dm.default_config(256)
    sc = dm.gen_scenes(cfg, 700, n, n_obs, junction_every=8)
    off = _rollout_outputs(dm, cfg, sc, n, n_obs, K, score=False)
    on = _rollout_outputs(dm, cfg, sc, n, n_obs, K, score=True)
    for name in off:
        assert on[name].tobytes() == off[name].tobytes(), name
    assert (on["score"]["n_ticks"] == K + 1).all() and (on["score"]["n_grid_ticks"] == K + 1).all()
    assert (on["EgoTrace"][K - 1]["pose"]["x"] != sc["scene_in"]["loc"]["globalpoint"]["x"]).mean() > 0.5


@gpu
@pytest.mark.parametrize("n", [128, 1024])
def test_scored_rollout_equals_its_parts(dm, n):
    """pp_rollout(K) with scoring = K x (advance, tick) with scoring, and reading the score in the middle of the run (a host
    wait) does not change the final record."""
    K, n_obs = 12, 32
    cfg = dm.default_config(256)
    sc = dm.gen_scenes(cfg, 700, n, n_obs, junction_every=8)
    whole = _rollout_outputs(dm, cfg, sc, n, n_obs, K, score=True)
    parts = _rollout_outputs(dm, cfg, sc, n, n_obs, K, score=True, whole=False)
    parts_mid = _rollout_outputs(dm, cfg, sc, n, n_obs, K, score=True, whole=False, read_mid=True)
    _same(whole["score"], parts["score"], "rollout against its parts")
    _same(whole["score"], parts_mid["score"], "with reads in the middle")
    assert np.array_equal(whole["score"]["ego_flags"], whole["flags"])
    assert (whole["score"]["dist"] > 0).mean() > 0.5


@gpu
@pytest.mark.parametrize("copies", [1, 300])
def test_known_answer_collision_beside_the_lane(dm, copies):
    """The collision scene on the device, one scene and 300 copies: contact on scored ticks 31 and 32, the worst clearance on
    tick 32, the distance of the ramp - from the closed form (_ramp_closed_form) - and, from the traced poses, byte for byte."""
    from kat_backends import replicate
    cfg, sc, x0 = _ramp_scene(dm)
    rs = replicate(sc, copies)
    pl = dm.Planner(cfg, device=0, max_scenes=copies, max_obs_total=copies)
    pl.set_scenes(rs, with_motion=False)
    pl.set_state(rs["state"])
    pl.score_begin()
    _, trace = pl.rollout(RAMP_TICKS, trace=True)
    pl.sync()
    got, trace = pl.rollout_score(), np.array(trace)
    assert (pl.get_plan()["ob_flag"] == 0).all()
    pl.close()
    print(f"copies {copies}: first collision {int(got['first_collision_tick'][0])}, {int(got['n_collision_ticks'][0])} collision ticks, "
          f"min clearance {float(got['min_clearance'][0])!r} on tick {int(got['min_clearance_tick'][0])}, dist {float(got['dist'][0])!r}")
    _check_ramp_record(got[0])
    assert all(got[k].tobytes() == got[0].tobytes() for k in range(copies))
    # from the traced poses (row t: the ego of scored tick t + 1) the clearance and distance fields follow exactly
    xs = [x0] + [float(v) for v in trace[:, 0]["pose"]["x"]]
    ys = [float(sc["scene_in"]["loc"]["globalpoint"]["y"][0])] + [float(v) for v in trace[:, 0]["pose"]["y"]]
    ob = sc["obs_pool"][:1]
    cls = [sm.clearance(x, y, ob["x"], ob["y"], ob["radius"], 1.8)[0] for x, y in zip(xs, ys)]
    dist = 0.0
    for k in range(1, len(xs)):
        ex, ey = xs[k] - xs[k - 1], ys[k] - ys[k - 1]
        dist = dist + math.sqrt(ex * ex + ey * ey)
    assert float(got["min_clearance"][0]) == min(cls) and int(got["min_clearance_tick"][0]) == cls.index(min(cls))
    assert float(got["dist"][0]) == dist
    assert [k for k, c in enumerate(cls) if c <= 0] == [31, 32]


@gpu
@pytest.mark.parametrize("n", [40, 320])
def test_ticks_without_an_advance_are_scored(dm, n):
    """update_async + tick x 8 (new egos from the host every tick), then 3 ticks on unchanged inputs: every one is scored once,
    against the model, byte for byte after every tick - one-stream ticks (40 scenes) and piped ones (320)."""
    n_obs = 16
    cfg = dm.default_config(256)
    sc = dm.gen_scenes(cfg, 300, n, n_obs, junction_every=8)
    pl = _planner(dm, cfg, sc, n, n_obs)
    plan_p, grid_p = dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut)
    pl.score_begin(0.05)
    want = sm.new_scores(dm.RolloutScore, n)
    flags = np.zeros(n, np.int32)
    keep = []
    for t in range(11):
        if 0 < t <= 8:
            in_t = dm.pinned_copy(sc["scene_in"])
            in_t["loc"]["globalpoint"]["x"] += 0.125 * t
            in_t["loc"]["globalpoint"]["y"] += 0.0625 * (t % 3)
            in_t["loc"]["velocity"] += 1.5 * ((t % 4) - 1.5)
            keep.append(in_t)
            pl.update_async(in_t)
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p, grid_p)) == 0
        sin = pl.get_scene_in()
        sm.fold(want, cfg, 0.05, sin, np.array(plan_p), pl.get_state(), sc["obs_pool"], flags, np.array(grid_p))
        _same(pl.rollout_score(), want, f"tick {t}")
    got = pl.rollout_score()
    pl.close()
    assert (got["n_ticks"] == 11).all() and (got["dist"] > 0).all() and (got["max_acc"] > 0).all() and (got["max_dec"] > 0).all()
    assert (got["ego_flags"] == 0).all()


@gpu
def test_lifecycle(dm):
    n, n_obs = 64, 8
    cfg = dm.default_config(128)
    sc = dm.gen_scenes(cfg, 40, n, n_obs, junction_every=0)
    sc["scene_in"]["lanes"]["cur_n"][:8] = 80                 # within 32 points of their lane end at once: frozen after the first advance
    pl = _planner(dm, cfg, sc, n, n_obs)
    model = dm.default_ego_model()
    with pytest.raises(dm.PlannerError, match="-4"):          # PP_ERR_STATE: never begun
        pl.rollout_score()
    pl.tick()                                                 # not scored
    for bad in (0.0, -0.1, math.inf, math.nan):
        with pytest.raises(dm.PlannerError, match="-1"):      # PP_ERR_ARG
            pl.score_begin(bad)
    with pytest.raises(dm.PlannerError, match="-4"):          # ... and a refused begin allocates nothing
        pl.rollout_score()
    pl.score_begin()
    _same(pl.rollout_score(), sm.new_scores(dm.RolloutScore, n), "after score_begin")
    pl.rollout(5, model)
    a = pl.rollout_score()
    assert (a["n_ticks"] == 5).all() and (a["n_grid_ticks"] == 5).all()          # the unscored tick before is the plan the first advance follows
    assert np.array_equal(a["ego_flags"], pl.ego_flags()) and (a["ego_flags"][:8] & dm.EGO_LANE_END).all() and (a["ego_flags"] == 0).any()
    pl.score_begin()                                          # twice: the totals restart
    _same(pl.rollout_score(), sm.new_scores(dm.RolloutScore, n), "after the second score_begin")
    pl.rollout(3, model)
    b = pl.rollout_score()
    assert (b["n_ticks"] == 3).all() and np.array_equal(b["ego_flags"], pl.ego_flags())
    pl.set_scenes(sc, with_motion=False)                      # new scenes while scoring is on: zeroed
    _same(pl.rollout_score(), sm.new_scores(dm.RolloutScore, n), "after set_scenes")
    pl.set_state(sc["state"])
    pl.rollout(4, model)                                      # 1 initial tick + 4
    c = pl.rollout_score()
    assert (c["n_ticks"] == 5).all()
    pl.score_end()
    pl.rollout(3, model)                                      # scoring off: the records stay as they are, and readable
    pl.tick()
    _same(pl.rollout_score(), c, "after score_end")
    pl.close()
