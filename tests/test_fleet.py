"""Fleet coupling (pp_set_fleet / pp_get_obstacles / k_couple_fleet).

CPU: the ABI mirror, hand-derived known answers of the numpy model (tests/fleet_model.py) with their arithmetic, and a two-ego
platoon run as a closed loop on the CPU (oracle tick + ego model + fleet model), coupled and uncoupled.
GPU: the device against that model after pp_set_fleet and after every advance of a closed loop, BYTE FOR BYTE (§4e specifies
the step exactly); the closed loop against a fleet-less handle fed the traced inputs, and against the oracle; the platoon; the
scorecard over a fleet rollout; pp_rollout against the stepped run; fleet off against a handle that never had one; errors."""
import math

import numpy as np
import pytest

import coupling_backends as cb
import ego_model as em
import fleet_model as fl
import rollout_score_model as sm
from parity_util import compare

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirror_and_default_model(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(22) == dm.FleetModel.itemsize == 16
    assert hasattr(lib, "pp_set_fleet") and hasattr(lib, "pp_get_obstacles") and hasattr(lib, "pp_default_fleet_model")
    fm = dm.default_fleet_model()
    # 60 m: the reach of the front corridor; 0.9f: half the default vehicle width (1.8 m) rounded to float; 8 peers
    assert float(fm["range"][0]) == 60.0 and int(fm["max_peers"][0]) == 8
    assert fm["radius"][0] == np.float32(0.5 * float(dm.default_config(128)["Vehicle_Width"][0])) == np.float32(0.9)
    assert dm.OB_PEER == fl.OB_PEER == 0x40000000 and dm.FLEET_MAX_PEERS == 64


FILL = cb.FILL          # every byte of the pools before the step: an untouched slot still holds it


def _fm(dm, rng=60.0, K=8, radius=0.9):
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"], fm["radius"] = rng, K, radius
    return fm


def _runner(name, log=None):
    return cb.FleetRunner(cb.FleetModelBackend() if name == "model" else cb.FleetDeviceBackend(), log)


@pytest.fixture()
def cfg0(dm):
    return cb.config()


# The known answers are written once against a runner of tests/coupling_backends.py: run(cfg, fm, world_first, positions, n_own,
# motion) puts scene s on pool entries [s (n_own + K), ..) - n_own own entries, K peer slots - and returns SceneIn, the pinned slices
# and the whole pools after the step, from the numpy model (CPU; the incoming obs_off / obs_n are rubbish, the step overwrites
# them with the pinned values) and from pp_set_fleet on a resident set (test_kat_on_the_device), where SceneIn, every slice and
# every pool byte are also held against the model.
def _kat_three_on_a_line(dm, cfg0, run):
    # egos at x = 0, 3, 4 on y = 0, one world, K = 2, range 60.
    # scene 0: d2 to 1 = 3*3 = 9, to 2 = 4*4 = 16 -> slots (1, 2);  scene 1: d2 to 0 = 9, to 2 = 1 -> slots (2, 0);
    # scene 2: d2 to 0 = 16, to 1 = 1 -> slots (1, 0)
    r = run(cfg0, _fm(dm, K=2), [0, 3], [(0.0, 0.0), (3.0, 0.0), (4.0, 0.0)], n_own=1, motion=True)
    out, p2, m2, off = r.out, r.pool, r.mot, r.off
    assert [r.peers(s) for s in range(3)] == [(2, [1, 2]), (2, [2, 0]), (2, [1, 0])]
    assert out["obs_off"].tolist() == [0, 3, 6] and out["obs_n"].tolist() == [3, 3, 3]
    # a slot is the peer's position, OB_PEER | its scene and the model's radius (0.9 rounded to float); its motion is zero;
    # the scene's own entry (index 0 of its slice) and its motion keep their bytes
    o = p2[off[1] + 1]
    assert (float(o["x"]), float(o["y"]), int(o["type"]), o["radius"]) == (4.0, 0.0, 0x40000002, np.float32(0.9))
    assert m2[off[1] + 1].tobytes() == bytes(16) and m2[off[1] + 2].tobytes() == bytes(16)
    for s in range(3):
        assert p2[off[s]].tobytes() == bytes([FILL]) * 24 and m2[off[s]].tobytes() == bytes([FILL]) * 16
    # nothing else of SceneIn changes
    a, b = out.copy(), r.si.copy()
    a["obs_off"], a["obs_n"], b["obs_off"], b["obs_n"] = 0, 0, 0, 0
    assert a.tobytes() == b.tobytes()
    # the inputs are not written (model: the rubbish the records came with; device: the slices that were pinned)
    assert r.pool_in.tobytes() == bytes([FILL]) * r.pool_in.nbytes and int(r.si["obs_n"][0]) == (-7 if run.name == "model" else 1)


def _kat_tie_goes_to_the_lower_scene(dm, cfg0, run):
    # 3-4-5 triangles: scene 1 at the origin, scene 0 at (3, 4), scene 2 at (4, 3), scene 3 at (-5, 0): d2 = 9 + 16 = 16 + 9 =
    # 25 + 0 = 25 for all three, exactly -> order 0, 2, 3 by scene index; with K = 2 scene 3 is left out
    xy = [(3.0, 4.0), (0.0, 0.0), (4.0, 3.0), (-5.0, 0.0)]
    assert run(cfg0, _fm(dm, K=3), [0, 4], xy).peers(1) == (3, [0, 2, 3])
    assert run(cfg0, _fm(dm, K=2), [0, 4], xy).peers(1) == (2, [0, 2])


def _kat_range_edge(dm, cfg0, run):
    # range 5: a peer at (3, 4) has d2 = 25 = 5*5 exactly: in (<=); one at (0, nextafter(5)) has d2 = y*y > 25: out
    y = math.nextafter(5.0, 6.0)
    assert y * y > 25.0
    r = run(cfg0, _fm(dm, rng=5.0, K=4), [0, 3], [(0.0, 0.0), (3.0, 4.0), (0.0, y)])
    assert r.peers(0) == (1, [1])
    # untouched slots c .. K - 1 keep their bytes
    assert r.pool[r.off[0] + 1:r.off[0] + 4].tobytes() == bytes([FILL]) * (3 * 24)
    # from scene 2 the others are sqrt(0 + y*y) = y > 5 and sqrt(9 + (y - 4)^2) ~ 3.16 away: only scene 1
    assert r.peers(2) == (1, [1])


def _kat_fewer_slots_than_candidates_and_none(dm, cfg0, run):
    # five egos 1 m apart on a line, K = 2: scene 2 (the middle) takes 1 and 3 (d2 = 1 both, lower index first), not 0 and 4 (d2 = 4)
    xy = [(float(k), 0.0) for k in range(5)]
    r = run(cfg0, _fm(dm, K=2), [0, 5], xy)
    assert r.peers(2) == (2, [1, 3])
    assert r.peers(0) == (2, [1, 2]) and r.peers(4) == (2, [3, 2])
    # K = 0: no slot, obs_off / obs_n are still the pinned values
    r = run(cfg0, _fm(dm, K=0), [0, 5], xy, n_own=2)
    assert r.out["obs_n"].tolist() == [2] * 5 and r.out["obs_off"].tolist() == [0, 2, 4, 6, 8] and r.pool.tobytes() == r.pool_in.tobytes()


def _kat_nan_peer_and_nan_self(dm, cfg0, run):
    # scene 1 has a NaN x: its d2 is NaN for everyone - no candidate - and it sees nobody itself; the others see each other
    r = run(cfg0, _fm(dm, K=3), [0, 4], [(0.0, 0.0), (math.nan, 0.0), (2.0, 0.0), (0.0, math.inf)])
    assert r.peers(0) == (1, [2]) and r.peers(2) == (1, [0])
    assert r.peers(1) == (0, []) and r.peers(3) == (0, [])      # (inf: not finite either)
    assert int(r.out["obs_off"][1]) == int(r.off[1]) and int(r.out["obs_n"][1]) == 0
    assert r.pool[r.off[1]:r.off[1] + 3].tobytes() == bytes([FILL]) * (3 * 24)


def _kat_worlds_do_not_see_each_other(dm, cfg0, run):
    # scenes 0, 1 | 2, 3: scenes 1 and 2 share a position, scenes 0 and 3 are 1 m from it - each sees only its own world's member
    xy = [(1.0, 0.0), (0.0, 0.0), (0.0, 0.0), (0.0, 1.0)]
    r = run(cfg0, _fm(dm, K=3), [0, 2, 4], xy)
    assert [r.peers(s) for s in range(4)] == [(1, [1]), (1, [0]), (1, [3]), (1, [2])]
    # one world of all four: scene 1 sees 2 (d2 = 0), then 0 and 3 (d2 = 1, lower index first)
    assert run(cfg0, _fm(dm, K=3), [0, 4], xy).peers(1) == (3, [2, 0, 3])
    # a world of one sees nobody
    r = run(cfg0, _fm(dm, K=3), [0, 1, 4], xy)
    assert r.peers(0) == (0, []) and r.peers(1) == (2, [2, 3])


KATS = [_kat_three_on_a_line, _kat_tie_goes_to_the_lower_scene, _kat_range_edge, _kat_fewer_slots_than_candidates_and_none, _kat_nan_peer_and_nan_self,
        _kat_worlds_do_not_see_each_other]


def test_kat_three_on_a_line(dm, cfg0):
    _kat_three_on_a_line(dm, cfg0, _runner("model"))


def test_kat_tie_goes_to_the_lower_scene(dm, cfg0):
    _kat_tie_goes_to_the_lower_scene(dm, cfg0, _runner("model"))


def test_kat_range_edge(dm, cfg0):
    _kat_range_edge(dm, cfg0, _runner("model"))


def test_kat_fewer_slots_than_candidates_and_none(dm, cfg0):
    _kat_fewer_slots_than_candidates_and_none(dm, cfg0, _runner("model"))


def test_kat_nan_peer_and_nan_self(dm, cfg0):
    _kat_nan_peer_and_nan_self(dm, cfg0, _runner("model"))


def test_kat_worlds_do_not_see_each_other(dm, cfg0):
    _kat_worlds_do_not_see_each_other(dm, cfg0, _runner("model"))


@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg0, kat):
    """The known answers above on k_couple_fleet (pp_set_fleet on a resident set), each also held byte for byte against the model."""
    kat(dm, cfg0, _runner("device"))


@gpu
def test_kat_batch_equals_each_case_alone(dm, cfg0):
    """Every known answer once more on the device, logged, then the calls that share a FleetModel as worlds of one launch
    (coupling_backends.fleet_batched): every scene gives the bytes it gave alone, scene indices and pool offsets moved."""
    log = []
    run = _runner("device", log)
    for kat in KATS:
        kat(dm, cfg0, run)
    sizes = cb.fleet_batched(cb.FleetDeviceBackend(), log)
    print(f"{len(log)} calls in batches of {sizes} scenes")
    assert sum(sizes) >= sum(len(c["xy"]) for c in log) and all(n % 4 != 0 and n > 4 for n in sizes)


# ---- the platoon: a standing leader and a follower approaching it in the same lane -------------------------------
P_TICKS, P_GAP, P_SPEED, P_K = 36, 20.0, 20.0, 4
P_FAR = 300.0            # every scene's own obstacle: 300 m to the left, seen by nobody (it makes the peer slot index 1, not 0)


def _platoon(dm, copies=1):
    """`copies` worlds of (leader, follower) on the straight three-lane road of lanechange_scenes.make_scene (x = 100 + 0.5 k, the
    road of test_rollout._scene with its pools, refpath and state filled in), lane 2, decision stage off, replanning every tick
    (the configuration of test_known_answer_speed_ramp).  Leader: standing, expected speed 0, P_GAP m ahead.  Follower: P_SPEED
    km/h, expected speed P_SPEED.  Established on the oracle alone (the CPU test below): at 20 km/h the reference's speed plan,
    seeing the leader 20 m ahead, brakes to a stop about 7 m short of it; blind, the follower covers 20 km/h * 3.6 s = 20 m in
    36 ticks and ends on top of the leader.  Every scene owns one far-away obstacle and P_K peer slots."""
    import lanechange_scenes as lcs
    cfg = dm.default_config(128)
    cfg["decision_stage"], cfg["force_replan"] = 0, 1
    parts = []
    for ahead, vel in ((P_GAP, 0.0), (0.0, P_SPEED)):
        sc = lcs.make_scene(dm, cfg, lane_num=2, obstacles=())
        si = sc["scene_in"]
        si["dec"]["velocity_expect"], si["dec"]["behavior"], si["dec"]["target_lanenum"] = vel, 1, 2
        si["loc"]["velocity"] = vel
        si["loc"]["globalpoint"]["x"] += ahead
        si["loc"]["id"][:] = lcs.EGO_ID + int(round(2 * ahead))
        si["goal"]["x"] += ahead
        si["grid_origin"]["x"] = si["loc"]["globalpoint"]["x"] - 2.0
        parts.append(sc)
    n, stride = 2 * copies, 1 + P_K
    sc = dict(parts[0])
    sc["scene_in"] = np.tile(np.concatenate([p["scene_in"] for p in parts]), copies)
    sc["state"] = np.tile(np.concatenate([p["state"] for p in parts]), copies)
    sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"] = np.arange(n) * stride, 1
    sc["obs_pool"], sc["mot_pool"], sc["n_obs"] = np.zeros(n * stride, dm.ObPoint), np.zeros(n * stride, dm.ObMotion), stride
    own = sc["obs_pool"][::stride]
    own["x"], own["y"], own["radius"] = sc["scene_in"]["loc"]["globalpoint"]["x"], sc["scene_in"]["loc"]["globalpoint"]["y"] + P_FAR, 0.5
    fm = dm.default_fleet_model()
    fm["max_peers"] = P_K
    return cfg, sc, fm, np.arange(copies + 1, dtype=np.int32) * 2


def _contact(fx, fy, lx, ly, radius, width):
    """Clearance of the follower at (fx, fy) to the leader disc at (lx, ly), as rollout_score_model computes a clearance."""
    return sm.clearance(fx, fy, np.array([lx]), np.array([ly]), np.array([radius], np.float32), width)[0]


def _platoon_on_the_cpu(dm, oracle, coupled, ticks=P_TICKS):
    cfg, sc, fm, wf = _platoon(dm)
    model = dm.default_ego_model()
    off, own = sc["scene_in"]["obs_off"].copy(), sc["scene_in"]["obs_n"].copy()
    sin, obs, st, flags = sc["scene_in"].copy(), sc["obs_pool"].copy(), sc["state"].copy(), np.zeros(2, np.int32)
    if coupled:
        sin, obs, _ = fl.couple(fm, wf, off, own, sin, obs)
    cls, ob_flags, types, scores = [], [], [], sm.new_scores(dm.RolloutScore, 2)
    for t in range(ticks + 1):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=sin, obs_pool=obs), st, want_grid=False)
        g = sin["loc"]["globalpoint"]
        cls.append(_contact(float(g["x"][1]), float(g["y"][1]), float(g["x"][0]), float(g["y"][0]), float(fm["radius"][0]), float(cfg["Vehicle_Width"][0])))
        ob_flags.append(int(plan["ob_flag"][1])), types.append(int(plan["ob"]["type"][1]))
        sm.fold(scores, cfg, float(model["dt"][0]), sin, plan, st, obs, flags)
        if t < ticks:
            sin, flags, _ = em.advance(cfg, model, sin, plan, st, flags, sc["lane_pool"])
            if coupled:
                sin, obs, _ = fl.couple(fm, wf, off, own, sin, obs)
    return dict(cls=cls, ob_flags=ob_flags, types=types, scores=scores, sin=sin, flags=flags)


def test_platoon_closed_loop_on_the_cpu(dm, oracle):
    """Coupled, the follower sees the leader from the first tick (ob_flag on every tick, PlanOut.ob is the peer slot), brakes and
    never touches it; uncoupled, the same run ends inside the leader while its own obstacle list - and so its scorecard - shows
    nothing."""
    c = _platoon_on_the_cpu(dm, oracle, True)
    print("coupled: clearance from %.3f to %.3f m, ob_flag ticks %d, final speed %r" %
          (c["cls"][0], c["cls"][-1], sum(c["ob_flags"]), float(c["sin"]["loc"]["velocity"][1])))
    assert min(c["cls"]) > 0 and all(c["ob_flags"]) and not c["flags"].any()
    assert all(t == (fl.OB_PEER | 0) for t in c["types"])                       # the leader is scene 0
    assert float(c["sin"]["loc"]["velocity"][1]) < P_SPEED                      # it is braking ...
    long = _platoon_on_the_cpu(dm, oracle, True, ticks=120)
    assert float(long["sin"]["loc"]["velocity"][1]) == 0.0 and min(long["cls"]) > 0 and long["cls"][:P_TICKS + 1] == c["cls"]      # ... to a stop, short of the leader
    assert float(c["sin"]["loc"]["globalpoint"]["x"][0]) == 125.0 + P_GAP       # ... and the leader never moved
    r = c["scores"][1]
    assert int(r["n_collision_ticks"]) == 0 and int(r["min_clearance_obs"]) == 1 and int(r["n_ob_flag"]) == P_TICKS + 1
    assert float(r["min_clearance"]) == min(c["cls"])                           # the scorecard's clearance IS the clearance to the leader
    u = _platoon_on_the_cpu(dm, oracle, False)
    print("uncoupled: clearance from %.3f to %.3f m, smallest %.3f" % (u["cls"][0], u["cls"][-1], min(u["cls"])))
    assert u["cls"][-1] <= 0 and not any(u["ob_flags"]) and not u["flags"].any()
    r = u["scores"][1]
    assert int(r["n_collision_ticks"]) == 0 and int(r["min_clearance_obs"]) == 0 and float(r["min_clearance"]) > 100.0


# ---------------------------------------------------------------------------------------------------------------
# GPU
TICKS, F_K, F_RANGE = 30, 8, 3.0
_RUN = {}


def _strided(dm, sc, n, n_obs, K):
    """The scenes' obstacle slices moved apart: scene s owns [s (n_obs + K), ..): n_obs own entries, then K free peer slots."""
    stride = n_obs + K
    out = dict(sc, scene_in=sc["scene_in"].copy(), n_obs=stride)
    for k, dt in (("obs_pool", dm.ObPoint), ("mot_pool", dm.ObMotion)):
        p = np.zeros((n, stride), dt)
        p[:, :n_obs] = sc[k][:n * n_obs].reshape(n, n_obs)
        out[k] = p.reshape(-1)
    out["scene_in"]["obs_off"], out["scene_in"]["obs_n"] = np.arange(n) * stride, n_obs
    return out


def _fleet_on_a_map(dm, n=1024, n_obs=16, K=F_K):
    """1024 egos of map_scenes.make_egos on one map: up to ~70 egos per lane within 50 m, so a range of 3 m gives every
    peer count from 0 to K (chosen with the model on the CPU: roughly 10 % of the scenes see nobody, 20 % fill all 8 slots)."""
    import map_scenes as ms
    cfg = dm.default_config(128)
    m = ms.build_map(dm, n_roads=5)
    sc = _strided(dm, ms.make_egos(dm, cfg, m, n, n_obs), n, n_obs, K)
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"] = F_RANGE, K
    caps = dict(max_scenes=n, max_obs_total=n * (n_obs + K), max_lane_pts_total=len(m["points"]), max_ref_pts_total=max(len(m["jpoints"]), 1))
    return cfg, m, sc, fm, caps


WORLDS = [0, 1, 3, 10, 74, 1024]          # worlds of 1, 2, 7, 64 and the rest (950 members: more than one per lane)


def _map_planner(dm, cfg, m, sc, caps, fleet=None):
    pl = dm.Planner(cfg, device=0, **caps)
    pl.set_map(m)
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    if fleet is not None:
        pl.set_fleet(*fleet)
    return pl


def _pool_of(pl, n, base):
    """The obstacle pool of the input set get_scene_in reads, rebuilt from every scene's slice (the slots beyond obs_n, which no
    kernel reads, as in `base`); and the slices."""
    pool, slices = base.copy(), []
    sin = pl.get_scene_in()
    for s in range(n):
        sl = pl.get_obstacles(s)
        assert len(sl) == int(sin["obs_n"][s])
        pool[int(sin["obs_off"][s]):int(sin["obs_off"][s]) + len(sl)] = sl
        slices.append(sl)
    return sin, pool, slices


def _closed_loop(dm):
    """31 scored ticks of a fleet with pp_get_scene_in + pp_get_obstacles after pp_set_fleet and after every advance."""
    if _RUN:
        return _RUN
    cfg, m, sc, fm, caps = _fleet_on_a_map(dm)
    n = len(sc["scene_in"])
    pl = _map_planner(dm, cfg, m, sc, caps)
    raw = pl.get_scene_in()                               # (with the lane views derived: what pp_set_fleet reads)
    pl.set_fleet(WORLDS, fm)
    pl.score_begin()
    model = dm.default_ego_model()
    plan_p, grid_p = dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut)
    sin, pool, slices = _pool_of(pl, n, sc["obs_pool"])
    run = dict(cfg=cfg, m=m, sc=sc, fm=fm, caps=caps, n=n, model=model, raw=[raw], sin=[sin], pool=[pool], slices=[slices], plan=[], grid=[],
               state=[], flags=[np.zeros(n, np.int32)])
    for t in range(TICKS + 1):
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p, grid_p)) == 0
        run["plan"].append(np.array(plan_p)), run["grid"].append(np.array(grid_p)), run["state"].append(pl.get_state())
        if t < TICKS:
            pl.advance_async(model)
            sin, pool, slices = _pool_of(pl, n, run["pool"][-1])
            run["sin"].append(sin), run["pool"].append(pool), run["slices"].append(slices), run["flags"].append(pl.ego_flags())
    run["score"], run["last_sin"] = pl.rollout_score(), pl.get_scene_in()
    pl.close()
    _RUN.update(run)
    return _RUN


@gpu
def test_step_check_against_the_model(dm):
    """The model applied to the device's own SceneIn of a set gives the device's obs_off, obs_n and slice bytes for every
    scene after pp_set_fleet and after every advance: no tolerance, nothing left out."""
    r = _closed_loop(dm)
    n, sc, K = r["n"], r["sc"], F_K
    off, own = sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"]
    hist = np.zeros(K + 1, np.int64)
    for t in range(TICKS + 1):
        got = r["sin"][t]
        base = r["pool"][t - 1] if t else sc["obs_pool"]
        want, wpool, _ = fl.couple(r["fm"], WORLDS, off, own, got, base)
        assert np.array_equal(got["obs_off"], want["obs_off"]) and np.array_equal(got["obs_n"], want["obs_n"]), f"set {t}: obs_off / obs_n"
        assert got.tobytes() == want.tobytes(), f"set {t}: SceneIn"
        for s in range(n):
            a, c = int(want["obs_off"][s]), int(want["obs_n"][s])
            assert r["slices"][t][s].tobytes() == wpool[a:a + c].tobytes(), f"set {t}, scene {s}: slice"
        hist += np.bincount(got["obs_n"] - own, minlength=K + 1)
    print("peers per scene-tick:", hist.tolist())
    assert hist[1:].sum() >= (TICKS + 1) * n // 4 and hist[K] > 0 and hist[0] > 0
    # the own entries never change, and what the advance produced differs from the first set only in loc and the slices
    assert r["pool"][TICKS].reshape(n, -1)[:, :16].tobytes() == sc["obs_pool"].reshape(n, -1)[:, :16].tobytes()
    # before pp_set_fleet the records had the caller's slices
    assert np.array_equal(r["raw"][0]["obs_n"], own) and (r["sin"][0]["obs_n"] > own).any()
    assert int(r["sin"][0]["obs_n"][0]) == int(own[0])                          # scene 0 is a world of its own


@gpu
def test_step_check_long_world(dm):
    """One world of 4200 scenes (more than 64 stride steps of 64 lanes) and worlds of 1 .. 130 beside it, on the resident
    set alone (no tick): pp_set_fleet against the model, bytes."""
    n, K = 4300, 5
    cfg = dm.default_config(32)
    cfg["grid_stage"] = 0
    sc = _strided(dm, dm.gen_scenes(cfg, 0, n, 1, junction_every=0), n, 1, K)
    rng = np.random.default_rng(3)
    g = sc["scene_in"]["loc"]["globalpoint"]
    g["x"], g["y"] = rng.uniform(0.0, 300.0, n), rng.uniform(0.0, 300.0, n)
    g["x"][4000], g["y"][17] = np.nan, np.inf
    g["x"][4100:4104], g["y"][4100:4104] = 7.0, 9.0                            # four egos on one spot: ties at d2 = 0
    wf = [0, 4200, 4201, 4203, 4300]
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"], fm["radius"] = 5.0, K, 1.25
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * (1 + K))
    pl.set_scenes(sc, with_motion=True)
    pl.set_fleet(wf, fm)
    got = pl.get_scene_in()
    want, wpool, wmot = fl.couple(fm, wf, sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"], sc["scene_in"], sc["obs_pool"], sc["mot_pool"])
    assert got.tobytes() == want.tobytes()
    for s in list(range(0, n, 7)) + [17, 4000, 4100, 4101, 4102, 4103, 4200, 4201, 4202]:
        a, c = int(want["obs_off"][s]), int(want["obs_n"][s])
        assert pl.get_obstacles(s).tobytes() == wpool[a:a + c].tobytes(), s
    hist = np.bincount(got["obs_n"] - 1, minlength=K + 1)
    print("peers per scene:", hist.tolist())
    assert hist[K] > 0 and hist[0] > 0 and int(got["obs_n"][4000]) == 1 and int(got["obs_n"][17]) == 1
    pl.close()


@gpu
def test_closed_loop_plans_what_the_open_loop_plans(dm, oracle):
    """A second handle WITHOUT a fleet, fed every tick's traced SceneIn and obstacle pool through pp_update_async, gives the fleet
    handle's PlanOut, GridOut and SceneState bit for bit; the oracle, given the same inputs, agrees within the usual bounds."""
    r = _closed_loop(dm)
    n, cfg, sc = r["n"], r["cfg"], r["sc"]
    pl = _map_planner(dm, cfg, r["m"], sc, r["caps"])
    plan_p, grid_p = dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut)
    keep = []
    for t in range(TICKS + 1):
        in_t, obs_t = dm.pinned_copy(r["sin"][t]), dm.pinned_copy(r["pool"][t])
        keep.append((in_t, obs_t))
        pl.update_async(in_t, obs_t)
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p, grid_p)) == 0
        assert np.array(plan_p).tobytes() == r["plan"][t].tobytes(), f"tick {t}: PlanOut"
        assert np.array(grid_p).tobytes() == r["grid"][t].tobytes(), f"tick {t}: GridOut"
        assert pl.get_state().tobytes() == r["state"][t].tobytes(), f"tick {t}: SceneState"
    pl.close()
    seen = 0
    for t in range(TICKS + 1):
        st_o = (r["state"][t - 1] if t else sc["state"]).copy()
        plan_o, gout_o, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=r["sin"][t], obs_pool=r["pool"][t], mot_pool=None), st_o, n_threads=16)
        bad = compare(r["plan"][t], plan_o, "plan") + compare(r["state"][t], st_o, "state")
        bad += compare(r["grid"][t]["status"], gout_o["status"], "grid.status")
        ok = (gout_o["status"] != 3) & (gout_o["status"] != 7)      # OVERFLOW / COST_RANGE: only the status is specified
        bad += compare(r["grid"][t][ok], gout_o[ok], "grid")
        assert not bad, f"tick {t}\n" + "\n".join(bad[:20])
        seen += int(((r["plan"][t]["ob"]["type"] & dm.OB_PEER) != 0).sum())
    print("scene-ticks whose planning obstacle was a peer:", seen)
    assert seen > 0                                       # the peers do reach the plans


@gpu
def test_scorecard_with_peers(dm):
    """RolloutScore over the fleet rollout = rollout_score_model fed the traced snapshots, peers included, bytes; and some
    scene's nearest obstacle was a peer."""
    r = _closed_loop(dm)
    n = r["n"]
    want = sm.new_scores(dm.RolloutScore, n)
    for t in range(TICKS + 1):
        sm.fold(want, r["cfg"], float(r["model"]["dt"][0]), r["sin"][t], r["plan"][t], r["state"][t], r["pool"][t], r["flags"][t], r["grid"][t])
    got = r["score"]
    assert got.tobytes() == want.tobytes(), ", ".join(f for f in got.dtype.names if got[f].tobytes() != want[f].tobytes())
    by_peer = got["min_clearance_obs"] >= r["sc"]["scene_in"]["obs_n"]
    print(f"nearest obstacle was a peer in {int(by_peer.sum())} of {n} scenes; ego-ego contact in {int(((got['n_collision_ticks'] > 0) & by_peer).sum())}")
    assert by_peer.any() and (got["n_ticks"] == TICKS + 1).all()


@gpu
def test_rollout_needs_no_host_wait(dm):
    """pp_rollout of 30 ticks on a fleet with nothing in between = the stepped run: last PlanOut, final SceneIn, ego flags."""
    r = _closed_loop(dm)
    pl = _map_planner(dm, r["cfg"], r["m"], r["sc"], r["caps"], fleet=(WORLDS, r["fm"]))
    last = pl.rollout(TICKS, r["model"])
    assert last == TICKS + 1
    pl.sync()
    assert pl.get_plan().tobytes() == r["plan"][TICKS].tobytes()
    assert pl.get_grid_out().tobytes() == r["grid"][TICKS].tobytes()
    assert pl.get_state().tobytes() == r["state"][TICKS].tobytes()
    assert pl.get_scene_in().tobytes() == r["last_sin"].tobytes() == r["sin"][TICKS].tobytes()
    assert np.array_equal(pl.ego_flags(), r["flags"][TICKS])
    for s in (0, 1, 5, 40, 100, 1023):
        assert pl.get_obstacles(s).tobytes() == r["slices"][TICKS][s].tobytes()
    pl.close()


def _outputs(pl):
    pl.sync()
    return dict(PlanOut=pl.get_plan(), GridOut=pl.get_grid_out(), SceneState=pl.get_state(), SceneIn=pl.get_scene_in(), flags=pl.ego_flags())


@gpu
def test_fleet_off_is_the_engine_without_one(dm):
    """A rollout with no pp_set_fleet, and one with pp_set_fleet followed by pp_set_fleet(h, 0, ..) before the first advance,
    give identical bytes; switching off restores the slices; and the fleet does change the run (the comparison is not vacuous)."""
    cfg, m, sc, fm, caps = _fleet_on_a_map(dm, n=256)
    K, wf = 12, [0, 100, 256]
    outs = []
    for mode in ("never", "on-off", "on"):
        pl = _map_planner(dm, cfg, m, sc, caps)
        first = pl.get_scene_in()
        if mode != "never":
            pl.set_fleet(wf, fm)
            assert (pl.get_scene_in()["obs_n"] > first["obs_n"]).any()
        if mode == "on-off":
            pl.set_fleet(None)
            assert pl.get_scene_in().tobytes() == first.tobytes()
            pl.set_fleet(None)                             # off twice is fine
        pl.rollout(K, dm.default_ego_model())
        outs.append(_outputs(pl))
        pl.close()
    for name in outs[0]:
        assert outs[0][name].tobytes() == outs[1][name].tobytes(), name
    assert outs[2]["PlanOut"].tobytes() != outs[0]["PlanOut"].tobytes()


@gpu
@pytest.mark.parametrize("copies", [1, 300])
def test_platoon(dm, oracle, copies):
    """The CPU scenario on the device, one world and 300: the follower's ob_flag ticks and PlanOut.ob.type as on the CPU, no
    contact (scorecard: no collision tick, nearest obstacle = its peer slot); with the fleet off its trace runs into the
    leader while its scorecard reports no collision."""
    cfg, sc, fm, wf = _platoon(dm, copies)
    n = 2 * copies
    lead, foll = np.arange(copies) * 2, np.arange(copies) * 2 + 1
    cpu = _platoon_on_the_cpu(dm, oracle, True)
    width, radius = float(cfg["Vehicle_Width"][0]), float(fm["radius"][0])
    for coupled in (True, False):
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=len(sc["obs_pool"]))
        pl.set_scenes(sc, with_motion=False)
        pl.set_state(sc["state"])
        if coupled:
            pl.set_fleet(wf, fm)
        pl.score_begin()
        plan_p = dm.pinned_empty(n, dm.PlanOut)
        trace = dm.pinned_empty(n * P_TICKS, dm.EgoTrace)
        ob_flags, types = [], []
        for t in range(P_TICKS + 1):
            pl.tick()
            assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
            ob_flags.append(np.array(plan_p["ob_flag"])), types.append(np.array(plan_p["ob"]["type"]))
            if t < P_TICKS:
                pl.advance_async(None, trace[t * n:(t + 1) * n])
        pl.sync()
        score, tr, flags = pl.rollout_score(), np.array(trace).reshape(P_TICKS, n), pl.ego_flags()
        pl.close()
        assert not flags.any()
        # contact from the traces, on the host: the follower's pose of every tick against the leader's
        xs = np.vstack([sc["scene_in"]["loc"]["globalpoint"]["x"][None, :], tr["pose"]["x"]])
        ys = np.vstack([sc["scene_in"]["loc"]["globalpoint"]["y"][None, :], tr["pose"]["y"]])
        cls = np.array([[_contact(xs[t, f], ys[t, f], xs[t, f - 1], ys[t, f - 1], radius, width) for f in foll] for t in range(P_TICKS + 1)])
        print(f"copies {copies}, coupled {coupled}: follower clearance from {cls[0, 0]:.3f} to {cls[-1, 0]:.3f} m, ob_flag ticks {int(sum(o[1] for o in ob_flags))}")
        assert (xs[:, lead] == 125.0 + P_GAP).all()                                 # the leaders stand
        for k in range(1, copies):
            assert tr[:, 2 * k:2 * k + 2]["pose"].tobytes() == tr[:, 0:2]["pose"].tobytes()
        if coupled:
            assert [int(o[1]) for o in ob_flags] == cpu["ob_flags"] and all((o[foll] == o[1]).all() for o in ob_flags)
            for t in range(P_TICKS + 1):
                assert np.array_equal(types[t][foll], dm.OB_PEER | lead), f"tick {t}"
            assert cls.min() > 0
            assert (score["n_collision_ticks"][foll] == 0).all() and (score["min_clearance_obs"][foll] == 1).all()
            assert np.abs(cls[:, 0] - np.array(cpu["cls"])).max() <= 1e-6           # the CPU run, to the rounding of the Bezier paths
            assert (score["min_clearance"][foll] == cls.min(axis=0)).all()
        else:
            assert not any(o.any() for o in ob_flags)
            assert (cls[-1] <= 0).all()                                             # inside the leader ...
            assert (score["n_collision_ticks"] == 0).all() and (score["min_clearance_obs"] == 0).all()      # ... and the scorecard cannot see it


def _set_scenes_raw(dm, pl, sc, n_obs_total):
    n = len(sc["scene_in"])
    rc = pl.lib.pp_set_scenes(pl.h, n, sc["scene_in"].ctypes.data, sc["lane_pool"].ctypes.data, sc["attr_pool"].ctypes.data, len(sc["lane_pool"]),
                              sc["ref_pool"].ctypes.data, len(sc["ref_pool"]), sc["obs_pool"].ctypes.data, None, n_obs_total)
    assert rc == 0, pl.lib.pp_last_error()
    pl.n = n


@gpu
def test_errors_leave_the_fleet_as_it_was(dm):
    n, n_obs, K = 64, 8, 8
    cfg = dm.default_config(128)
    tight = dm.gen_scenes(cfg, 40, n, n_obs, junction_every=0)             # slices back to back: no room for a peer slot
    sc = _strided(dm, tight, n, n_obs, K)
    fm, wf = _fm(dm, rng=40.0, K=K), [0, 10, 64]
    model = dm.default_ego_model()

    def planner(scenes=sc, max_obs=n * (n_obs + K)):
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=max_obs)
        _set_scenes_raw(dm, pl, scenes, min(max_obs, len(scenes["obs_pool"])))
        pl.set_state(scenes["state"])
        return pl

    # no resident scenes
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * (n_obs + K))
    with pytest.raises(dm.PlannerError, match="-4"):
        pl.set_fleet(wf, fm)
    pl.close()
    # overlapping extended slices; a pool that ends before the last scene's peer slots
    pl = planner(tight, n * n_obs + 1000)
    with pytest.raises(dm.PlannerError, match="-1"):
        pl.set_fleet(wf, fm)
    pl.set_fleet(wf, _fm(dm, rng=40.0, K=0))                                # K = 0 needs no room
    assert pl.get_scene_in().tobytes() == tight["scene_in"].tobytes()
    pl.close()
    pl = planner(sc, n * (n_obs + K) - 1)
    with pytest.raises(dm.PlannerError, match="-3"):
        pl.set_fleet(wf, fm)
    pl.close()
    # a good fleet, then every bad call: the fleet stays as it was and the rollout is the one of a handle that never saw them
    ref = planner()
    ref.set_fleet(wf, fm)
    ref.rollout(6, model)
    want = _outputs(ref)
    ref.close()
    pl = planner()
    pl.set_fleet(wf, fm)
    coupled = pl.get_scene_in()
    assert (coupled["obs_n"] > n_obs).any()
    for bad_wf in ([1, 10, 64], [0, 10, 10, 64], [0, 30, 20, 64], [0, 10, 63], [0, 10, 65]):
        with pytest.raises(dm.PlannerError, match="-1"):
            pl.set_fleet(bad_wf, fm)
    for bad_fm in (_fm(dm, K=65), _fm(dm, K=-1), _fm(dm, rng=math.nan), _fm(dm, rng=math.inf), _fm(dm, rng=0.0), _fm(dm, radius=-1.0), _fm(dm, radius=math.nan)):
        with pytest.raises(dm.PlannerError, match="-1"):
            pl.set_fleet(wf, bad_fm)
    with pytest.raises(dm.PlannerError, match="-1"):
        pl.get_obstacles(n)
    assert pl.get_scene_in().tobytes() == coupled.tobytes()
    pl.set_fleet(wf, fm)                                                    # the same fleet again starts from the OWN entries
    assert pl.get_scene_in().tobytes() == coupled.tobytes()
    pl.rollout(6, model)
    got = _outputs(pl)
    for name in want:
        assert got[name].tobytes() == want[name].tobytes(), name
    # an update staged for the next tick: PP_ERR_STATE, and the advance goes through
    pl.advance_async(model)
    with pytest.raises(dm.PlannerError, match="-4"):
        pl.set_fleet(wf, fm)
    pl.tick()
    pl.sync()
    # new scenes: the fleet is off, obs_n as uploaded
    _set_scenes_raw(dm, pl, sc, len(sc["obs_pool"]))
    pl.set_state(sc["state"])
    pl.rollout(3, model)
    assert np.array_equal(pl.get_scene_in()["obs_n"], sc["scene_in"]["obs_n"])
    pl.close()


@gpu
def test_set_egos_after_a_fleet_switches_it_off(dm):
    cfg, m, sc, fm, caps = _fleet_on_a_map(dm, n=128)
    pl = _map_planner(dm, cfg, m, sc, caps, fleet=([0, 128], fm))
    assert (pl.get_scene_in()["obs_n"] > 16).any()
    pl.rollout(3, dm.default_ego_model())
    pl.set_egos(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.rollout(3, dm.default_ego_model())
    assert (pl.get_scene_in()["obs_n"] == 16).all()
    ref = _map_planner(dm, cfg, m, sc, caps)
    ref.rollout(3, dm.default_ego_model())
    a, b = _outputs(pl), _outputs(ref)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    pl.close(), ref.close()


@gpu
def test_update_async_on_a_fleet_handle(dm):
    """The third launch site: a fleet handle fed from the host.  SceneIn records alone (with rubbish obs_off / obs_n), SceneIn with
    an obstacle pool that ends before the last peer slots, and an obstacles-only update on top of a staged advance: after each
    the set the tick reads is fleet_model.couple of what was uploaded, byte for byte, nothing is poisoned, and a following
    advance carries the own entries and the slots along."""
    n, n_obs, K = 64, 8, 8
    stride = n_obs + K
    cfg = dm.default_config(128)
    sc = _strided(dm, dm.gen_scenes(cfg, 40, n, n_obs, junction_every=0), n, n_obs, K)
    fm, wf = _fm(dm, rng=1e6, K=K), [0, 10, 64]           # (a range that holds every generated ego: each scene of these worlds of 10 and 54 fills its K slots)
    off, own = sc["scene_in"]["obs_off"].copy(), sc["scene_in"]["obs_n"].copy()
    model = dm.default_ego_model()
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * stride)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_fleet(wf, fm)
    sin0, pool, _ = _pool_of(pl, n, sc["obs_pool"])
    assert (sin0["obs_n"] > own).any() and int(sin0["obs_n"][n - 1]) > n_obs          # the last scene has peers: its slots end the pool
    plan_p = dm.pinned_empty(n, dm.PlanOut)

    def tick():
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0                            # nothing poisoned

    def check(what, uploaded, base):
        got, got_pool, slices = _pool_of(pl, n, base)
        want, wpool, _ = fl.couple(fm, wf, off, own, uploaded, base)
        assert got.tobytes() == want.tobytes(), what + ": SceneIn"
        for s in range(n):
            a, c = int(want["obs_off"][s]), int(want["obs_n"][s])
            assert slices[s].tobytes() == wpool[a:a + c].tobytes(), f"{what}, scene {s}: slice"
        return got, got_pool

    tick()
    # 1. SceneIn records alone: the egos moved, obs_off / obs_n are rubbish
    in1 = dm.pinned_copy(sc["scene_in"])
    in1["loc"]["globalpoint"]["x"] += 0.75
    in1["loc"]["globalpoint"]["y"][::3] += 0.5
    in1["obs_off"], in1["obs_n"] = 12345, -7
    pl.update_async(in1)
    tick()
    got, pool = check("SceneIn only", np.array(in1), pool)
    assert np.array_equal(got["obs_off"], off) and (got["obs_n"] >= own).all() and (got["obs_n"] > own).any()
    # 2. SceneIn and an obstacle pool that stops behind the last scene's OWN entries (below the end of its peer slots)
    in2 = dm.pinned_copy(sc["scene_in"])
    in2["loc"]["globalpoint"]["x"] += 1.5
    in2["obs_off"], in2["obs_n"] = -3, 99999
    short = (n - 1) * stride + n_obs
    obs2 = dm.pinned_copy(sc["obs_pool"][:short])
    obs2["x"] += 0.25
    obs2["type"] = 7
    with pytest.raises(dm.PlannerError, match="-1"):                                  # one entry less would cut the last scene's OWN entries
        pl.update_async(in2, obs2, n_obs_total=short - 1)
    pl.update_async(in2, obs2, n_obs_total=short)
    tick()
    base = pool.copy()
    base[:short] = obs2
    got, pool = check("SceneIn and a short pool", np.array(in2), base)
    assert int(got["obs_n"][n - 1]) > n_obs
    assert all(int(t) == 7 for t in pl.get_obstacles(5)[:n_obs]["type"])            # the own entries are the uploaded ones
    # 3. obstacles only, on top of a staged advance: the egos the advance produced, the obstacles uploaded
    pl.advance_async(model)
    adv = pl.get_scene_in()
    obs3 = dm.pinned_copy(sc["obs_pool"])
    obs3["y"] -= 0.5
    obs3["type"] = 9
    pl.update_async(None, obs3)
    got, pool = check("obstacles on a staged advance", adv, np.array(obs3))
    assert got.tobytes() == adv.tobytes()                                           # (the same egos: the same peers)
    tick()
    # a following advance carries own entries and slots along, and couples again
    pl.advance_async(model)
    nxt = pl.get_scene_in()
    got, pool = check("the advance after", nxt, pool)
    assert all(int(t) == 9 for t in pl.get_obstacles(5)[:n_obs]["type"]) and (got["obs_n"] > own).any()
    assert (got["loc"]["globalpoint"]["x"] != adv["loc"]["globalpoint"]["x"]).any()
    tick()
    pl.close()


@gpu
def test_peer_slots_carry_no_motion(dm):
    """With moving obstacles on (§5 G4) and a motion pool whose PEER SLOTS hold 5 m/s, the platoon runs exactly as with zero
    motion there: the step zeroes a slot's ObMotion.  The same velocity on an own obstacle at the leader's place does change
    the run (the comparison is not vacuous)."""
    cfg, sc, fm, wf = _platoon(dm)
    cfg["dynamic_obstacles"] = 1
    stride = 1 + P_K

    def run(scenes, fleet):
        pl = dm.Planner(cfg, device=0, max_scenes=2, max_obs_total=len(scenes["obs_pool"]))
        pl.set_scenes(scenes, with_motion=True)
        pl.set_state(scenes["state"])
        if fleet:
            pl.set_fleet(wf, fm)
        _, trace = pl.rollout(P_TICKS, trace=True)
        pl.sync()
        out = (np.array(trace), pl.get_plan(), pl.get_state())
        pl.close()
        return out

    moving = dict(sc, mot_pool=sc["mot_pool"].copy())
    for s in range(2):
        moving["mot_pool"]["vx"][s * stride + 1:(s + 1) * stride] = 5.0
        moving["mot_pool"]["vy"][s * stride + 1:(s + 1) * stride] = -1.0
    a, b = run(sc, True), run(moving, True)
    for x, y, name in zip(a, b, ("EgoTrace", "PlanOut", "SceneState")):
        assert x.tobytes() == y.tobytes(), name
    assert float(a[0][-1]["velocity"][1]) < P_SPEED                                  # the follower did react to the leader
    # fleet off, the leader as the follower's OWN obstacle: standing against driving away at 5 m/s
    own = dict(sc, obs_pool=sc["obs_pool"].copy(), mot_pool=sc["mot_pool"].copy())
    o = own["obs_pool"][stride]
    o["x"], o["y"], o["radius"] = sc["scene_in"]["loc"]["globalpoint"]["x"][0], sc["scene_in"]["loc"]["globalpoint"]["y"][0], fm["radius"][0]
    away = dict(own, mot_pool=own["mot_pool"].copy())
    away["mot_pool"]["vx"][stride] = 5.0
    c, d = run(own, False), run(away, False)
    assert c[0].tobytes() != d[0].tobytes()
