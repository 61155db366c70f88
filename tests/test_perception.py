"""Perception model: hand-derived known answers on the numpy model and on k_perceive inside real ticks, the device held
byte for byte against the model over a moving set, the transparent model and the hidden record against a handle without the call, and
the errors of the set call.  Every device case also passes through perception_backends.DeviceBackend, which holds the perceived
snapshot, the truth snapshot, the tracks and the stats against the model after every tick."""
import math
import os

import numpy as np
import pytest

import dmpp_amd as dm
import perception_backends as pb
import perception_model as pcm

BACKENDS = [pytest.param("model"), pytest.param("device", marks=pytest.mark.gpu)]
NEXT10 = math.nextafter(10.0, math.inf)
R_BELOW_1 = float(np.nextafter(np.float32(1), np.float32(0)))


SHAPES = ["alone", "family", "x300"]
SURVIVOR_SEED = 3775741442          # hash0(seed, 0, 0, 1) >> 32 == 0xFFFFFFFF: found by running through all 2^32 seeds


def run(backend, m, ticks, replica=False):
    return pb.BACKENDS[backend]().run(pb.config(), m, ticks, replica=replica)


def copies_tick(cfg, scene, n):
    """n copies of one scene (x, y, dir, obs), their slices one behind the other."""
    t = pb.scene_tick(cfg, [scene])
    m = len(scene[3])
    si = np.repeat(t.si, n)
    si["obs_off"] = np.arange(n) * m
    return pb.cb.Tick(si, np.tile(t.pool[:m], n) if m * n else t.pool)


def laid_out(backend, m, cases, shape, replica=True):
    """cases: per case the list over its ticks of one scene (x, y, dir, obs).  alone: every case on a handle of its own; family: the cases
    as the scenes of one launch (a shorter case repeats its last tick; its checks look at its own ticks only); x300: every case as 300
    copies.  replica: the model of the family draws nothing scene-dependent from the hash, so the model leg steps one copy.
    Returns [(case index, result, ticks, scene)]."""
    cfg = pb.config()
    if shape == "family":
        ticks = [pb.scene_tick(cfg, [c[min(k, len(c) - 1)] for c in cases]) for k in range(max(len(c) for c in cases))]
        res = run(backend, m, ticks)
        return [(i, res, ticks, i) for i in range(len(cases))]
    out, n = [], 1 if shape == "alone" else 300
    for i, c in enumerate(cases):
        ticks = [copies_tick(cfg, sc, n) for sc in c]
        res = run(backend, m, ticks, replica=replica and n > 1)
        out += [(i, res, ticks, s) for s in sorted({0, n // 2, n - 1})]
    return out


def hidden_flags(res, ticks, k, s):
    off, n = int(ticks[k].si[s]["obs_off"]), int(ticks[k].si[s]["obs_n"])
    out = []
    for j in range(n):
        e, t = res.seen[k][off + j], ticks[k].pool[off + j]
        hid = e["x"] == pcm.HIDDEN_XY and e["y"] == pcm.HIDDEN_XY and e["radius"] == 0 and e["type"] == t["type"]
        assert hid or e.tobytes() == t.tobytes(), f"tick {k} scene {s} entry {j}: neither hidden nor the truth's bytes"
        out.append(bool(hid))
    return out


EGO = (0.0, 0.0, 0.0)


def scene(obs, ego=EGO):
    return ego + (obs,)


# ---- range and field of view: ego (0, 0) heading 0, range 10, cos_half_fov 0 ------------------------------------------------------
VIEW_OBS = [(10.0, 0.0, 0.5), (NEXT10, 0.0, 0.5), (6.0, 8.0, 0.5), (0.0, 5.0, 0.5), (-5e-324, 5.0, 0.5), (0.0, 0.0, 0.5), (math.nan, 0.0, 0.5),
            (0.0, -10.0, 0.5), (math.inf, 0.0, 0.5)]
VIEW_HIDDEN = [False, True, False, False, True, False, True, False, True]      # d2 == range^2 seen, one ulp beyond not; dx = 0 seen, one ulp behind not; d2 = 0 seen; NaN, inf not
HW = 0.5 * float(pb.config()["Vehicle_Width"][0])
VIEW_CASES = [      # (scene, hidden flags, n_out, min_hidden_obs, min_hidden_tick, min_hidden_clearance)
    (scene(VIEW_OBS), VIEW_HIDDEN, 4, 4, 1, 5.0 - 0.5 - HW),                                 # the closest hidden entry: entry 4 at distance 5
    (scene(VIEW_OBS[:3], (math.nan, 0.0, 0.0)), [True] * 3, 3, -1, -1, math.inf),          # a NaN ego: nothing in view, every clearance a NaN
    (scene(VIEW_OBS[:3], (0.0, 0.0, math.nan)), [True] * 3, 3, 0, 1, 10.0 - 0.5 - HW),     # a NaN heading: nothing in view
    (scene(VIEW_OBS[:3], (math.inf, 0.0, 0.0)), [True] * 3, 3, 0, 1, math.inf),            # an infinite ego: d2 = inf, and inf < inf never holds
]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_range_and_view_edges(backend, shape):
    for i, res, ticks, s in laid_out(backend, pb.model(range=10.0, cos_half_fov=0.0), [[c[0]] for c in VIEW_CASES], shape):
        _, want, n_out, obs, tick, cl = VIEW_CASES[i]
        assert hidden_flags(res, ticks, 0, s) == want, f"case {i} scene {s}"
        st = res.stats[0][s]
        assert (st["n_out"], st["n_detected"], st["n_entries"], st["n_hidden"], st["n_fresh"]) == (n_out, len(want) - n_out, len(want), n_out, len(want) - n_out)
        if i == 3:          # (no clearance below +inf: the record keeps its start)
            obs, tick = -1, -1
        assert (st["min_hidden_obs"], st["min_hidden_tick"], st["min_hidden_clearance"]) == (obs, tick, cl), f"case {i} scene {s}"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_range_inf_sees_everything_finite(backend, shape):
    cases = [[scene([(1e200, 0.0, 0.5), (-1e150, 3.0, 0.5), (math.nan, 0.0, 0.5)])], [scene([(-0.0, 1e300, 0.5)])]]
    for i, res, ticks, s in laid_out(backend, pb.model(), cases, shape):
        assert hidden_flags(res, ticks, 0, s) == [[False, False, True], [False]][i]          # (d2 = inf <= inf * inf)


# ---- occlusion: ego (0, 0), all round, no range --------------------------------------------------------------------------------------
OCC_SCENES = [
    ([(10.0, 0.0, 0.5), (5.0, 1.0, 1.0)], [True, False]),                      # t = 0.5, foot (0, 1): 1 <= R^2 = 1, the tangent line is occluded
    ([(10.0, 0.0, 0.5), (5.0, 1.0, R_BELOW_1)], [False, False]),               # one float below: R^2 < 1
    ([(10.0, 0.0, 0.5), (-5.0, 0.0, 1.0)], [False, False]),                    # behind the ego: t <= 0
    ([(10.0, 0.0, 0.0), (15.0, 0.0, 1.0)], [False, False]),                    # beyond the target (which has no disc itself)
    ([(10.0, 0.0, 0.0), (6.0, 8.0, 20.0)], [False, False]),                    # equal d2 does not occlude, either way
    ([(10.0, 0.0, 0.5), (5.0, 0.0, 0.0), (4.0, 0.0, math.nan), (3.0, 0.0, math.inf)], [False, False, False, False]),      # R = 0 / NaN / inf: no disc
    ([(10.0, 0.0, 0.5), (12.0, 0.0, 1.0)], [False, True]),                     # the far one lies behind the near disc, the near one behind nothing
]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_occlusion_edges(backend, shape):
    for i, res, ticks, s in laid_out(backend, pb.model(occlusion=1), [[scene(obs)] for obs, _ in OCC_SCENES], shape):
        want = OCC_SCENES[i][1]
        assert hidden_flags(res, ticks, 0, s) == want, f"case {i} scene {s}"
        assert res.stats[0][s]["n_occluded"] == sum(want)


@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("backend", BACKENDS)
def test_block_of_four_edge(backend, n):
    """Four scenes fill one block of k_perceive, the fifth opens the next one."""
    cfg = pb.config()
    for obs, want in (OCC_SCENES[0], (ring(65, 64, 63), [j == 63 for j in range(65)])):
        t = copies_tick(cfg, scene(obs), n)
        res = run(backend, pb.model(occlusion=1), [t])
        for s in range(n):
            assert hidden_flags(res, [t], 0, s) == want


# ---- misses and noise: the draws depend on the scene, so the model leg steps every copy ---------------------------------------------------------
MISS_OBS = [(5.0 + j, 1.0, 0.5) for j in range(70)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_miss_thresholds(backend, shape):
    for i, res, ticks, s in laid_out(backend, pb.model(p_miss=0), [[scene(MISS_OBS)]], shape, replica=False):
        assert hidden_flags(res, ticks, 0, s) == [False] * 70
    # everything is missed but the one crafted survivor: entry 0 of scene 0 on tick 1
    for i, res, ticks, s in laid_out(backend, pb.model(p_miss=0xFFFFFFFF, seed=SURVIVOR_SEED), [[scene(MISS_OBS)]], shape, replica=False):
        assert hidden_flags(res, ticks, 0, s) == [not (s == 0 and j == 0) for j in range(70)], f"scene {s}"
        assert res.stats[0][s]["n_missed"] == (69 if s == 0 else 70)
    for i, res, ticks, s in laid_out(backend, pb.model(p_miss=0x80000000, seed=3), [[scene(MISS_OBS)]], shape, replica=False):
        want = [(pcm.hash0(3, s, j, 1) >> 32) < 0x80000000 for j in range(70)]
        assert hidden_flags(res, ticks, 0, s) == want and 20 < sum(want) < 50


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_noise(backend, shape):
    seen = set()
    for i, res, ticks, s in laid_out(backend, pb.model(sigma0=0.5, sigma_gain=0.01, seed=11), [[scene(MISS_OBS)]], shape, replica=False):
        off = int(ticks[0].si[s]["obs_off"])
        for j in range(70):
            e, o = res.seen[0][off + j], ticks[0].pool[off + j]
            sigma = 0.5 + 0.01 * math.sqrt((5.0 + j) * (5.0 + j) + 1.0)
            h0 = pcm.hash0(11, s, j, 1)
            assert e["x"] == o["x"] + sigma * pcm.normal(pcm.esm.mix(h0 + 1)) and e["y"] == o["y"] + sigma * pcm.normal(pcm.esm.mix(h0 + 2))
            assert abs(e["x"] - o["x"]) <= sigma * 3.47 and abs(e["y"] - o["y"]) <= sigma * 3.47 and (e["x"], e["y"]) != (o["x"], o["y"])
            assert e["type"] == o["type"] and e["radius"] == o["radius"]
        seen.add(res.seen[0][off:off + 70].tobytes())
    assert shape != "x300" or len(seen) == 3, "every scene draws its own noise"
    # sigma = 0 gives the truth's bytes, a -0.0 included
    for i, res, ticks, s in laid_out(backend, pb.model(seed=11), [[scene([(-0.0, 3.0, 0.5), (4.0, -0.0, 0.5)])]], shape):
        assert hidden_flags(res, ticks, 0, s) == [False, False]


# ---- tracks: range 10, the entry steps in (x = 5) and out (x = 20) of it ---------------------------------------------------------------------
F, C, H = pcm.FRESH, pcm.COASTED, pcm.HIDDEN
TRACK_CASES = [      # (confirm, coast, [(in-view pattern, types or None, outputs)])
    (0, 0, [([1, 1, 0, 1], None, [F, F, H, F])]),
    (1, 1, [([1, 1, 0, 1, 0, 0, 1, 1], None, [H, F, C, F, C, H, H, F]), ([1, 0, 1, 1, 0, 0], None, [H, H, H, F, C, H])]),
    (2, 3, [([1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1], None, [H, H, F, C, C, C, F, C, C, C, H, H, H, F]),
            ([1, 1, 1, 1, 1, 1], [1, 1, 1, 3, 3, 3], [H, H, F, H, H, F])]),          # the slot changes hands on the fourth tick: without the restart it would be fresh
    (2, 0, [([1, 1, 0, 1, 1, 1, 0, 1], None, [H, H, H, H, H, F, H, H])]),
]


def track_case(pattern, types=None):
    return [scene([(5.0 if v else 20.0, 0.25 * k, 0.5, 1 if types is None else types[k]), (3.0, -4.0, 0.5, 2)]) for k, v in enumerate(pattern)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_track_confirm_coast_and_slot_change(backend, shape):
    for confirm, coast, fam in TRACK_CASES:
        for i, res, ticks, s in laid_out(backend, pb.model(range=10.0, confirm=confirm, coast=coast), [track_case(p, ty) for p, ty, _ in fam], shape):
            pattern, types, want = fam[i]
            K = len(pattern)
            got = [res.log[k][s][0][1] for k in range(K)]
            assert got == want, f"confirm {confirm} coast {coast} case {i} scene {s}"
            off, last_fresh = int(ticks[0].si[s]["obs_off"]), None
            for k, kind in enumerate(got):
                e = res.seen[k][off]
                if kind == F:
                    assert e.tobytes() == ticks[k].pool[off].tobytes()
                    last_fresh = e.tobytes()
                elif kind == C:
                    assert e.tobytes() == last_fresh, "a coasted record keeps its bytes"
                else:
                    assert (e["x"], e["y"], e["radius"], e["type"]) == (pcm.HIDDEN_XY, pcm.HIDDEN_XY, 0.0, 1 if types is None else types[k])
            if types is not None:
                assert [int(res.tracks[k][off]["hits"]) for k in range(K)] == [1, 2, 3, 1, 2, 3]
            st = res.stats[K - 1][s]
            assert (st["n_ticks"], st["n_entries"]) == (K, 2 * K)
            assert st["n_out"] + st["n_occluded"] + st["n_missed"] + st["n_detected"] == st["n_entries"] == st["n_fresh"] + st["n_coasted"] + st["n_hidden"]
            assert (st["n_fresh"], st["n_coasted"], st["n_hidden"]) == (K - confirm + want.count(F), want.count(C), confirm + want.count(H))          # (the second entry is seen on every tick: hidden for its first `confirm`)


def test_episode_restart_restarts_the_slice_model():
    cfg = pb.config()
    ticks = [pb.scene_tick(cfg, [sc]) for sc in track_case([1, 1, 1, 1, 1, 1])]
    age = [np.array([(a,)], [("age", np.int32)]) for a in (5, 6, 7, 0, 1, 2)]
    res = pb.ModelBackend().run(cfg, pb.model(range=10.0, confirm=2, coast=3), ticks, ep_stats=age)
    assert [res.log[k][0][0][1] for k in range(6)] == [H, H, F, H, H, F]
    assert [res.log[k][0][1][1] for k in range(6)] == [H, H, F, H, H, F]          # the whole slice, not one entry


# ---- wave edges: a ring of m small discs round the ego, entry `occ` moved onto the sight line of entry `tgt` -------------------------------
def ring(m, occ=None, tgt=None):
    obs = []
    for j in range(m):
        a = 2.0 * math.pi * j / 264.0
        obs.append([(50.0 + 0.01 * j) * math.cos(a), (50.0 + 0.01 * j) * math.sin(a), 0.05])
    if occ is not None:
        a = 2.0 * math.pi * tgt / 264.0
        obs[occ] = [10.0 * math.cos(a), 10.0 * math.sin(a), 0.05]
    return [tuple(o) for o in obs]


# sizes on either side of the 64-lane chunk; the occluder in another chunk than the target, in the last partial chunk, at 0 and at m - 1
RING_CASES = [(0, None, None), (1, None, None), (63, 62, 0), (64, 0, 63), (65, 64, 63), (128, 127, 3), (129, 128, 0), (256, 70, 255), (257, 0, 256), (257, 256, 130)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_wave_edges(backend, shape):
    # family: ten scenes with adjacent slices (three blocks of four waves, the last one half empty): none reads its neighbour's entries
    for i, res, ticks, s in laid_out(backend, pb.model(occlusion=1), [[scene(ring(*c))] for c in RING_CASES], shape):
        m, occ, tgt = RING_CASES[i]
        assert hidden_flags(res, ticks, 0, s) == [j == tgt for j in range(m)], f"case {i} scene {s}"
        assert res.stats[0][s]["n_occluded"] == (occ is not None) and res.stats[0][s]["min_hidden_obs"] == (-1 if tgt is None else tgt)


@pytest.mark.parametrize("backend", BACKENDS)
def test_adjacent_slices_do_not_see_each_other(backend):
    # a scene whose only entry would hide the only entry of the next one, were it read across the slices - and the other way round
    t = pb.scene_tick(pb.config(), [scene([(10.0, 0.0, 1.0)]), scene([(100.0, 0.0, 0.5)]), scene([(10.0, 0.0, 1.0)])])
    res = run(backend, pb.model(occlusion=1), [t])
    assert [hidden_flags(res, [t], 0, s) for s in range(3)] == [[False], [False], [False]]


TIE_OBS = [(5.0, 0.0, 0.5)] * 140
for _j in (2, 66, 70):                                  # the same clearance three times: lane 2 twice, lane 6 once
    TIE_OBS[_j] = (0.0, 20.0, 0.5)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_min_hidden_ties(backend, shape):
    for i, res, ticks, s in laid_out(backend, pb.model(range=10.0), [[scene(TIE_OBS)] * 2], shape):
        for k in range(2):                              # the first minimum by tick, then by index
            st = res.stats[k][s]
            assert (st["min_hidden_tick"], st["min_hidden_obs"], st["min_hidden_type"]) == (1, 2, 1)
            assert st["min_hidden_clearance"] == 20.0 - 0.5 - HW


# ---- the device against the model over a moving set ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_against_model_moving_set():
    cfg, rng = pb.config(), np.random.default_rng(5)
    base = [[(float(rng.uniform(-70, 70)), float(rng.uniform(-70, 70)), float(rng.uniform(0.2, 2.5)), int(rng.integers(1, 4))) for _ in range(m)] for m in (70, 3, 0, 130, 64)]
    vel = [[(float(rng.uniform(-6, 6)), float(rng.uniform(-6, 6))) for _ in b] for b in base]
    ticks = []
    for k in range(12):
        ticks.append(pb.scene_tick(cfg, [(2.0 * k, 0.5 * s, 15.0 * s + 3.0 * k, [(o[0] + v[0] * k, o[1] + v[1] * k, o[2], o[3]) for o, v in zip(base[s], vel[s])])
                                         for s in range(5)]))
    res = pb.DeviceBackend().run(cfg, dm.default_perception(), ticks)          # (the backend holds every tick's bytes against the model)
    last = res.stats[-1]
    for f in ("n_out", "n_occluded", "n_missed", "n_detected", "n_fresh", "n_coasted", "n_hidden"):
        assert int(last[f].sum()) > 0, f"the set exercises {f}"


# ---- the transparent model and the hidden record, on handles with the whole tick ---------------------------------------------------------------
def _results(pl):
    return pl.get_plan(), pl.get_state(), pl.get_grid_out()


def _open(cfg, sc, n_obs, env=None):
    """env: read at pp_create (DMPP_PIPELINE_MIN, DMPP_TICK_GROUP), put back behind it."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pl = dm.Planner(cfg, device=0, max_scenes=len(sc["scene_in"]), max_obs_total=max(n_obs, 1))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pl.set_scenes(sc)
    pl.set_state(sc["state"].copy())
    return pl


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ticks", "group", "streamed", "rollout"])
def test_transparent_model_changes_nothing(mode):
    """ticks: one-stream ticks (without the call the snapshot is the head of k_decision<true>); group: piped ticks in groups of three,
    the last group cut short by the getters; streamed: every tick adopts an update; rollout: 30 scored advances."""
    cfg = dm.default_config(128)
    sc = dm.gen_scenes(cfg, 0, 8, 8, junction_every=4)
    got, keep = {}, []
    for name in ("never", "transparent", "set_then_off"):
        pl = _open(cfg, sc, 64, {"DMPP_PIPELINE_MIN": "1", "DMPP_TICK_GROUP": "3"} if mode == "group" else None)
        if name != "never":
            pl.set_perception(dm.transparent_perception())
        if name == "set_then_off":
            pl.set_perception(None)
        if mode == "rollout":
            pl.score_begin()
            pl.rollout(30)
        elif mode == "streamed":
            for k in range(5):
                si = sc["scene_in"].copy()
                si["loc"]["globalpoint"]["x"] += 0.25 * k
                in_t, obs_t = dm.pinned_copy(si), dm.pinned_copy(sc["obs_pool"])
                keep.append((in_t, obs_t))
                pl.update_async(in_t, obs_t)
                pl.tick()
        else:
            for _ in range(5):
                pl.tick()
        got[name] = _results(pl) + ((pl.rollout_score(), pl.get_scene_in()) if mode == "rollout" else ())
        if name == "transparent":
            n = 64
            assert pl.read_device(dm.BUF_OBS_SEEN, dm.ObPoint, n).tobytes() == pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, n).tobytes()
            st = pl.perception_stats()
            assert (st["n_fresh"] == st["n_entries"]).all() and (st["n_ticks"] == (31 if mode == "rollout" else 5)).all()      # (a first pp_rollout plans once in front of its first advance)
        pl.close()
    for name in ("transparent", "set_then_off"):
        for a, b in zip(got[name], got["never"]):
            assert a.tobytes() == b.tobytes(), f"{mode}, {name}: differs from the handle without the call"


@pytest.mark.gpu
@pytest.mark.parametrize("n_obs", [8, 64])
def test_all_missed_is_the_scene_without_obstacles(n_obs):
    """Every entry hidden on the device: PlanOut, SceneState and GridOut of the scenes with obs_n = 0, over three ticks."""
    cfg = dm.default_config(128)
    sc = dm.gen_scenes(cfg, 0, 8, n_obs, junction_every=4)
    pl = _open(cfg, sc, 8 * n_obs)
    pl.set_perception(pb.model(p_miss=0xFFFFFFFF))
    for _ in range(3):
        pl.tick()
    seen, hid, st = _results(pl), pl.read_device(dm.BUF_OBS_SEEN, dm.ObPoint, 8 * n_obs), pl.perception_stats()
    assert (st["n_missed"] == 3 * n_obs).all() and (st["n_hidden"] == 3 * n_obs).all() and (hid["x"] == pcm.HIDDEN_XY).all() and (hid["radius"] == 0).all()
    assert hid["type"].tobytes() == sc["obs_pool"]["type"].tobytes()
    pl.close()
    bare = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    bare["scene_in"]["obs_n"] = 0
    pl = _open(cfg, bare, 8 * n_obs)
    for _ in range(3):
        pl.tick()
    want = _results(pl)
    pl.close()
    for a, b, name in zip(seen, want, ("PlanOut", "SceneState", "GridOut")):
        assert a.tobytes() == b.tobytes(), name


@pytest.mark.gpu
def test_first_tick_window_and_resets_on_set_calls():
    """Between the set call and the first perceived tick PP_BUF_OBS_SEEN and pp_get_grid show what the last tick's search rasterised; the calls
    that replace the resident scenes or move slices restart tracks and stats, whether the model is on or switched off."""
    cfg = dm.default_config(128)
    sc = dm.gen_scenes(cfg, 0, 8, 8, junction_every=4)
    pl = _open(cfg, sc, 64)
    pl.tick()
    grid, now = pl.get_grid(3), pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, 64)
    pl.set_perception(dm.default_perception())
    assert pl.read_device(dm.BUF_OBS_SEEN, dm.ObPoint, 64).tobytes() == now.tobytes() and pl.get_grid(3).tobytes() == grid.tobytes()
    start_s, start_t = pcm.new_stats(dm.PerceptionStats, 8), pcm.new_tracks(dm.PerceptTrack, 64)

    def ticked():
        for _ in range(4):
            pl.tick()
        assert (pl.perception_stats()["n_ticks"] == 4).all() and pl.perception_tracks(0, 64)["hits"].any()

    def restarted(what):
        pb.same(pl.perception_stats(), start_s, what + ": stats")
        pb.same(pl.perception_tracks(0, 64), start_t, what + ": tracks")

    ticked()
    pl.set_scenes(sc)
    restarted("pp_set_scenes")
    ticked()
    rc = pl.lib.pp_set_n_scenes(pl.h, 8, len(sc["lane_pool"]), len(sc["ref_pool"]), 64, 1, 1)
    assert rc == 0, pl.lib.pp_last_error()
    restarted("pp_set_n_scenes")
    ticked()
    pl.set_traffic([], np.zeros(0, dm.GlobalPoint2D), [])          # traffic off: the traffic family restarts them too
    restarted("pp_set_traffic with no actors")
    ticked()
    pl.set_perception(None)                                        # off: the records stay readable, and still never mix two populations
    pl.set_scenes(sc)
    restarted("pp_set_scenes while the model is off")
    pl.close()


@pytest.mark.gpu
def test_episode_restart_on_the_device():
    """§4k's ring egos, one standing disc 20 m ahead of each, episodes of 7 advances: on the tick an ego restarts (EpisodeStats.age == 0, written
    on the upload stream in front of the set the tick adopts) the tracks of its slice restart - two hidden ticks again with confirm 2.  The
    perceived snapshot, tracks and stats are held byte for byte against the model stepped over the device's own SceneIn, truth and EpisodeStats."""
    import test_conflict_score as tcs
    import test_episodes as te
    cfg, m, sc, legs, rf, em = tcs._ring_scene(dm)
    n = te.RING_N
    pl = te._planner(dm, cfg, m, sc, 1)
    pl.set_route(legs, rf)
    pl.set_episodes(em)
    pm = pb.model(confirm=2, coast=3)
    pl.set_perception(pm)
    adv = dm.default_ego_model()
    wtracks, wstats = None, pcm.new_stats(dm.PerceptionStats, n)
    since, restarts = [0] * n, 0
    for t in range(20):
        sin, ages = pl.get_scene_in(), pl.episode_stats()
        pl.tick()
        total = int((sin["obs_off"] + sin["obs_n"]).max())
        now = pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, total)
        if wtracks is None:
            wtracks = pcm.new_tracks(dm.PerceptTrack, total)
        wseen, log = pcm.step(wtracks, wstats, pm, cfg, pl.tick_id(), sin, now, ages)
        on = pb.covered(sin, total)
        pb.same(pl.read_device(dm.BUF_OBS_SEEN, dm.ObPoint, total)[on], wseen[on], f"tick {t}: the perceived snapshot")
        pb.same(pl.perception_tracks(0, total)[on], wtracks[on], f"tick {t}: tracks")
        pb.same(pl.perception_stats(), wstats, f"tick {t}: stats")
        for s in range(n):
            if int(ages["age"][s]) == 0:
                since[s], restarts = 0, restarts + (t > 0)
            assert log[s][0][1] == (H if since[s] < 2 else F), f"tick {t} scene {s}: {since[s]} ticks behind its restart"
            since[s] += 1
        pl.advance_async(adv)
    assert restarts >= n, "every ego restarted at least once inside the loop"
    pl.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_sizes():
    lib = dm.load_library()
    for name in ("pp_default_perception", "pp_set_perception", "pp_get_perception_stats", "pp_get_perception_tracks"):
        assert hasattr(lib, name)
    assert (lib.pp_sizeof(50), lib.pp_sizeof(51), lib.pp_sizeof(52)) == (56, 32, 96) and lib.pp_sizeof(49) == 0
    m = dm.default_perception()[0]
    assert (m["range"], m["cos_half_fov"], m["sigma0"], m["sigma_gain"], m["occlusion"], m["confirm"], m["coast"]) == (60.0, 0.5, 0.1, 0.005, 1, 2, 3)
    assert int(m["p_miss"]) == round(0.02 * 2 ** 32)
    assert lib.pp_set_perception(None, None) == dm.PP_ERR_ARG


@pytest.mark.gpu
def test_errors():
    cfg = pb.config()
    t = pb.scene_tick(cfg, [(0.0, 0.0, 0.0, [(5.0, 0.0, 0.5)])])
    pl = pb.stb.open_planner(cfg, [t], None, False)
    stats, tracks = np.zeros(1, dm.PerceptionStats), np.zeros(1, dm.PerceptTrack)
    assert pl.lib.pp_get_perception_stats(pl.h, stats.ctypes.data, 1) == dm.PP_ERR_STATE          # before a set call: as pp_get_conflict_score
    assert pl.lib.pp_get_perception_tracks(pl.h, tracks.ctypes.data, 0, 1) == dm.PP_ERR_STATE
    assert pl.device_ptr(dm.BUF_OBS_SEEN) == (None, 0)
    bad = [dict(range=0.0), dict(range=-1.0), dict(range=math.nan), dict(cos_half_fov=1.5), dict(cos_half_fov=math.nan), dict(sigma0=-0.1), dict(sigma0=math.inf),
           dict(sigma_gain=math.nan), dict(sigma_gain=-1.0), dict(occlusion=2), dict(confirm=-1), dict(confirm=256), dict(coast=-1), dict(coast=256), dict(_pad=1)]
    for kw in bad:
        m = pb.model(**kw)
        assert pl.lib.pp_set_perception(pl.h, m.ctypes.data) == dm.PP_ERR_ARG, kw
    assert pl.lib.pp_get_perception_stats(pl.h, stats.ctypes.data, 1) == dm.PP_ERR_STATE          # a refused call changes nothing
    keep = []
    in_t, obs_t = dm.pinned_copy(t.si), dm.pinned_copy(t.pool)
    keep.append((in_t, obs_t))
    pl.update_async(in_t, obs_t)
    pl.set_perception(pb.model(range=10.0))             # legal with an update staged: the call reads nothing of the resident set
    pl.tick()
    assert pl.perception_stats()["n_fresh"][0] == 1
    assert pl.lib.pp_get_perception_stats(pl.h, stats.ctypes.data, 2) == dm.PP_ERR_ARG
    assert pl.lib.pp_get_perception_tracks(pl.h, tracks.ctypes.data, 1, 1) == dm.PP_ERR_ARG
    pl.set_perception(pb.model(range=10.0))             # a second call starts again
    assert pl.perception_stats()["n_ticks"][0] == 0 and pl.perception_tracks(0, 1)["hits"][0] == 0
    pl.close()
