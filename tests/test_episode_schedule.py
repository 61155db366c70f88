"""Scenario schedule (pp_set_episode_schedule): the start record of a restart drawn by weights from outcome counts
per start record, kept on the device.

CPU: the ABI mirrors; the known answers of §4p - weights, draws - on the numpy model (tests/episode_schedule_model.py) and on
pp_episode_schedule_weights, which is built from the function the kernel calls; the edges of min_samples, target and window; the
pass mask; gain = 0 against the hashed choice of §4l; scripted known answers on the model; a closed loop of oracle tick + route,
traffic, spawn and schedule models.
GPU: the scripted known answers on k_respawn_sched (+ k_fold_schedule) alone, in batches on either side of the block edge 4 | 5 and
of 300 scenes; the pooled fold on its chunk edges; the two scopes against each other; gain = 0 against k_respawn_spawn; the
clearance walk from a scheduled k0; off / never set; error paths and the life cycle; with the log and the traffic reset on;
pp_rollout against its parts; the closed loop against the CPU loop.

The scripted known answers.  The ego of tests/test_episode_spawn.py on lane 2 with max_ticks = 1: EVERY advance ends an episode
(TIMEOUT, 64), and a step whose injected path starts with a NaN point adds BAD_PATH (2) - the record is carried over, the ego moves
0 m.  With fail_mask = 2 the test scripts, advance by advance, whether the episode failed.  `script` below plays the draws of a
script with the pure functions of the model - no ego, no records -, so a test knows which record every advance starts from (its
path must begin there), and holds cur_start, n_used and the rows of both backends against it.

Which draws of the tables of §4p a scene can reach: u = mix(mix(seed + s) + e) depends on seed + s only, so the three hashes of
§4l are (seed 1, scene 0, e 1), (seed 4, scene 0, e 2) and (seed 3049, scene 0, e 100).  The FIRST draw of a scene always finds
rows of zeros - equal weights, the `[5,5,5,5]` row -; the second finds one counted episode on record 0: `[13,1,1,1]` and `[9,7]`;
the hundredth is reached by a script of 100 advances.  The remaining rows of the tables need counts no play of one scene produces
at e = 1 or 2; they are asserted on the model's draw, and the device is held to the model byte for byte on every step."""
import numpy as np
import pytest

import episode_model as epm
import episode_schedule_backends as evb
import episode_schedule_model as evm
import episode_spawn_backends as esb
import episode_spawn_model as esm
import episode_traffic_model as etm
import map_scenes as ms
import route_model as rmod
import test_episode_spawn as tes
import test_episodes as te
import test_traffic as tt
import traffic_model as tm

gpu = pytest.mark.gpu
U = (0x86D6FD953217AE03, 0xC7EB916392985897, 0xA0DF773B063C2D69)          # the three hashes of §4l
TIMEOUT, BAD_PATH, CONTACT = 64, 2, 128


@pytest.fixture()
def cfg1(dm):
    """Grid stage off, Vehicle_Width 2.0: hw = 1."""
    cfg = dm.default_config(128)
    cfg["grid_stage"], cfg["Vehicle_Width"] = 0, 2.0
    return cfg


def _sm(dm, **kw):
    sm = dm.default_episode_schedule()
    for k, v in kw.items():
        sm[k] = v
    return sm


def _row(dm, pairs):
    row = np.zeros(1, dm.EpisodeScheduleRow)
    for k, (n, f) in enumerate(pairs):
        row["n_end"][0, k], row["n_fail"][0, k] = n, f
    return row


STEEP = dict(min_samples=1, floor_w=1, gain=65535, target=65536, prior=65536)          # the second model of §4p 1.


# ---------------------------------------------------------------------------------------------------------------
# CPU: ABI, known answers, edges
def test_abi_mirrors_and_default_model(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(38) == dm.EpisodeSchedule.itemsize == 40
    assert lib.pp_sizeof(39) == dm.EpisodeScheduleRow.itemsize == 128
    names = ("scope", "fail_mask", "pass_mask", "min_samples", "window", "floor_w", "gain", "target", "prior", "_pad")
    assert dm.EpisodeSchedule.names == names and [dm.EpisodeSchedule.fields[k][1] for k in names] == list(range(0, 40, 4))
    assert [dm.EpisodeScheduleRow.fields[k][1] for k in ("n_end", "n_fail")] == [0, 64]
    assert dm.default_episode_schedule()[0].tolist() == (1, 207, 16, 4, 256, 4096, 61440, 32768, 32768, 0)
    assert [lib.pp_sizeof(k) for k in (31, 32, 34)] == [32, 80, 240]           # (the records of §4l and §4n are as they were)
    assert evm.CAUSES == 31 | dm.EGO_TIMEOUT | dm.EGO_CONTACT


def test_weight_known_answers(dm):
    for kw, pairs, want in ((dict(), [(0, 0), (3, 3), (4, 4), (4, 2), (4, 0), (8, 1)], [65536, 65536, 34816, 65536, 34816, 42496]),
                            (STEEP, [(0, 0), (1, 0), (1, 1), (3, 1), (3, 2), (64, 63)], [65536, 1, 65536, 21845, 43690, 64512])):
        sm, row = _sm(dm, **kw), _row(dm, pairs)
        assert evm.weights(sm, row[0], len(pairs)) == want
        assert dm.episode_schedule_weights(sm, row, len(pairs)).tolist() == want
    # the bounds of a weight: 1 <= w <= 131070
    assert evm.weight(_sm(dm, floor_w=1, gain=65535, target=0, min_samples=1), 5, 5) == 1
    assert evm.weight(_sm(dm, floor_w=65535, gain=65535, target=0, min_samples=1), 5, 0) == 131070


def test_draw_known_answers():
    assert [esm.hash_u(*a) for a in ((1, 0, 1), ((1 << 64) - 1, 5, 2), (2026, 1023, 100))] == list(U)
    assert [esm.hash_u(*a) for a in ((1, 0, 1), (4, 0, 2), (3049, 0, 100))] == list(U)          # ... as one scene reaches them
    for ws, ts, ks in (([1, 1, 1, 13], (8, 12, 10), (3, 3, 3)), ([13, 1, 1, 1], (8, 12, 10), (0, 0, 0)), ([5, 5, 5, 5], (10, 15, 12), (2, 3, 2)),
                       ([8, 1, 7], (8, 12, 10), (1, 2, 2)), ([9, 7], (8, 12, 10), (0, 1, 1))):
        assert [evm.draw(u, ws) for u in U] == list(zip(ts, ks)), ws
    assert evm.draw(U[0], [8, 1, 7]) == (8, 1)          # t equals the running sum 8: record 0 is passed


def test_min_samples_and_target_edges(dm):
    sm = _sm(dm)                                         # min_samples 4, prior = target: an unknown record has the largest weight
    assert evm.weights(sm, _row(dm, [(3, 0), (4, 0)])[0], 2) == [65536, 34816] == dm.episode_schedule_weights(sm, _row(dm, [(3, 0), (4, 0)]), 2).tolist()
    # r on the target, at 0 and at 65536: d = 0, 32768, 32768
    assert evm.weights(sm, _row(dm, [(4, 2), (4, 0), (4, 4)])[0], 3) == [4096 + 61440, 4096 + 30720, 4096 + 30720]
    for target, pairs, want in ((0, [(2, 0), (2, 2), (2, 1)], [1 + 65535, 1, 1 + 32767]), (65536, [(2, 0), (2, 2), (2, 1)], [1, 1 + 65535, 1 + 32767])):
        sm = _sm(dm, **dict(STEEP, target=target))
        assert evm.weights(sm, _row(dm, pairs)[0], 3) == want == dm.episode_schedule_weights(sm, _row(dm, pairs), 3).tolist()


def test_window_halves_both_counts(dm):
    row = _row(dm, [(6, 5), (0, 0)])[0]
    sm = _sm(dm, window=8)
    evm.fold(sm, row, [(0, True)])                      # window - 1: nothing
    assert (int(row["n_end"][0]), int(row["n_fail"][0])) == (7, 6)
    evm.fold(sm, row, [(0, True)])                      # window: one halving
    assert (int(row["n_end"][0]), int(row["n_fail"][0])) == (4, 3)
    evm.fold(sm, row, [(1, k % 2 == 0) for k in range(35)])      # pooled: 35 endings, 18 failures on record 1 in one advance: 35 -> 17 -> 8 -> 4, 18 -> 9 -> 4 -> 2
    assert (int(row["n_end"][1]), int(row["n_fail"][1])) == (4, 2) and int(row["n_end"][0]) == 4
    never = _row(dm, [(1000, 7)])[0]
    evm.fold(_sm(dm, window=0), never, [(0, False)])
    assert (int(never["n_end"][0]), int(never["n_fail"][0])) == (1001, 7)


def test_pass_mask(dm):
    sm = _sm(dm)                                         # fail 207, pass 16: an arrival passes, a missed exit fails
    assert [evm.fails(sm, c) for c in (20, 4, 64, 128, 128 | 16)] == [False, True, True, True, False]
    assert [evm.fails(_sm(dm, fail_mask=2, pass_mask=0), c) for c in (64, 66, 2)] == [False, True, True]


def test_gain_zero_is_the_hashed_order(dm):
    """Equal weights give §4l's k0 for every weight: gain = 0 whatever the counts, and any gain on rows of zeros."""
    rng = np.random.default_rng(7)
    for M in (1, 2, 3, 16):
        row = _row(dm, [(int(n), int(rng.integers(0, n + 1))) for n in rng.integers(0, 50, 16)])
        for sm, r in ((_sm(dm, gain=0, floor_w=int(rng.integers(1, 65536))), row), (_sm(dm), _row(dm, []))):
            ws = evm.weights(sm, r[0], M)
            assert len(set(ws)) == 1
            for seed, s, e in [(1, 0, 1), ((1 << 64) - 1, 5, 2), (2026, 1023, 100)] + [(int(rng.integers(1, 1 << 62)), int(rng.integers(0, 4096)), int(rng.integers(1, 1000))) for _ in range(50)]:
                assert evm.draw(esm.hash_u(seed, s, e), ws)[1] == esm.first_choice(seed, s, e, M, 0), (M, seed, s, e)


def test_host_weights_refuse_what_the_set_call_refuses(dm):
    row = _row(dm, [(1, 1)])
    for kw in (dict(scope=2), dict(fail_mask=256), dict(pass_mask=32), dict(min_samples=0), dict(window=1), dict(window=-1), dict(floor_w=0), dict(floor_w=65536),
               dict(gain=-1), dict(gain=65536), dict(target=65537), dict(prior=-1), dict(_pad=1)):
        with pytest.raises(dm.PlannerError, match="error -1:"):
            dm.episode_schedule_weights(_sm(dm, **kw), row, 1)
    for M in (0, 17):
        with pytest.raises(dm.PlannerError, match="error -1:"):
            dm.episode_schedule_weights(_sm(dm), row, M)
    with pytest.raises(dm.PlannerError, match="error -1:"):
        dm.episode_schedule_weights(_sm(dm), _row(dm, [(1, 2)]), 1)


# ---------------------------------------------------------------------------------------------------------------
# scripts
def script(sm, seed, M, fails):
    """fails[t][s]: does the episode that advance t ends for scene s fail.  Every advance ends an episode of every scene, no clearance
    check.  Returns (ks, rows): ks[t][s] the record scene s stands on when advance t reads it (ks[0] = 0), rows[t] behind advance t."""
    n, scope = len(fails[0]), int(sm["scope"][0])
    rows = np.zeros(n if scope == 0 else 1, [("n_end", np.int32, (16,)), ("n_fail", np.int32, (16,))])
    ks, out = [[0] * n], []
    for t, F in enumerate(fails):
        before = rows.copy()
        ks.append([evm.draw(esm.hash_u(seed, s, t + 1), evm.weights(sm, before[s if scope == 0 else 0], M))[1] for s in range(n)])
        if scope == 0:
            for s in range(n):
                evm.fold(sm, rows[s], [(ks[t][s], F[s])])
        else:
            evm.fold(sm, rows[0], [(ks[t][s], F[s]) for s in range(n)])
        out.append(rows.copy())
    return ks, out


def _po_table(dm, M):
    """PlanOut by [record the advance starts from][failed]: the straight path from the record's pose, its first point NaN for a failure."""
    tab = np.zeros((M, 2), dm.PlanOut)
    for k in range(M):
        tab[k, 0] = te._path(dm, tes._x(k))[0]
        tab[k, 1] = tab[k, 0]
        tab["road_points"]["x"][k, 1, 0] = np.nan
    return tab


def _case(dm, cfg1, sm, seed, M, fails, check=0, obs=None, sp_kw=None):
    """The Case of a script: n scenes of the ego at (110, 0), start records tes._starts, max_ticks = 1."""
    n = len(fails[0])
    ks, rows = script(_sm(dm, gain=0) if sm is None else sm, seed, M, fails)
    tab = _po_table(dm, M)
    steps = [(tab[np.array(ks[t]), np.array(F, int)], np.zeros(n, dm.SceneState)) for t, F in enumerate(fails)]
    one = tes._starts(dm, M)
    starts = None if M == 1 else (np.concatenate([np.repeat(one[0][k:k + 1], n) for k in range(M - 1)]), np.concatenate([np.repeat(one[1][k:k + 1], n) for k in range(M - 1)]))
    sp = tes._sp(dm, seed=seed, n_starts=M, order=0, check=check, **(sp_kw or {}))
    case = evb.Case(sm, cfg1, dm.default_ego_model(), te._em(dm, 31, 1), sp, np.repeat(te._ego(dm, 110.0, ego_id=20), n),
                    [np.zeros(0, dm.ObPoint) if obs is None else obs] * n, np.repeat(te._state0(dm), n), steps, te._world(dm), None, starts)
    return case, ks, rows


def _check_script(res, ks, rows, fails, what=""):
    """Results against the script: the record every advance took, n_used, the rows, the causes and the counts of §4k."""
    n = len(fails[0])
    for t, r in enumerate(res):
        assert r.sstats["cur_start"].tolist() == ks[t + 1], (what, t)
        assert r.rows.tobytes() == rows[t].tobytes(), (what, t, r.rows.tolist(), rows[t].tolist())
        assert r.stats["last_cause"].tolist() == [TIMEOUT | (BAD_PATH if f else 0) for f in fails[t]], (what, t)
        assert (r.stats["n_episodes"] == t + 1).all() and not r.flags.any(), (what, t)
    used = np.zeros((n, 16), np.int32)
    for t in range(1, len(res) + 1):
        used[np.arange(n), ks[t]] += 1
    assert np.array_equal(res[-1].sstats["n_used"], used), what


FM = dict(fail_mask=BAD_PATH, pass_mask=0)


def _kat_first_draw_finds_rows_of_zeros(dm, cfg1, run):
    # seed 1, scene 0, e = 1: u = U[0].  Rows of zeros: every record has the prior's weight - the [5,5,5,5] row: k0 = 2 of 4 - and the hashed
    # choice of §4l for the other M (1 of 2 and 3, 8 of 16).  The episode on record 0 failed: n_end[0] = n_fail[0] = 1 behind the advance
    for M, k in ((4, 2), (2, 1), (3, 1), (16, 8), (1, 0)):
        for scope in (0, 1):
            case, ks, rows = _case(dm, cfg1, _sm(dm, scope=scope, **FM), 1, M, [[True]])
            (r,) = run(case)
            assert ks[1] == [k] and int(r.sstats["cur_start"][0]) == k and r.rows["n_end"][0].tolist() == [1] + [0] * 15 == r.rows["n_fail"][0].tolist(), (M, scope)
            _check_script([r], ks, rows, [[True]])
            tes._is_record(dm, r, k, case.si, None if M == 1 else (case.starts[0], case.starts[1]), f"M {M}")


def _kat_second_draw_tables(dm, cfg1, run):
    # seed 4, scene 0: the SECOND draw has u = U[1] and finds one counted episode on record 0.
    # floor 1, gain 12, target 65536, prior 0, min_samples 1: a failure on record 0 gives r = 65536, w = 13, the unknown records r = 0, w = 1:
    # [13,1,1,1], t = 12 -> record 0.  Had the episode passed: [1,1,1,1], the hashed choice, (a 4) >> 32 = 3.
    sm = _sm(dm, scope=0, min_samples=1, floor_w=1, gain=12, target=65536, prior=0, window=0, **FM)
    for failed, ws, k in ((True, [13, 1, 1, 1], 0), (False, [1, 1, 1, 1], 3)):
        case, ks, rows = _case(dm, cfg1, sm, 4, 4, [[failed], [False]])
        res = run(case)
        assert evm.weights(sm, rows[0][0], 4) == ws and dm.episode_schedule_weights(sm, res[0].rows, 4).tolist() == ws
        assert evm.draw(U[1], ws) == ({13: 12, 1: 3}[ws[0]], k) and ks[2] == [k]
        _check_script(res, ks, rows, [[failed], [False]])
    # floor 1, gain 8, target 65536, prior 49152: record 0 failed: d = 0, w = 9; record 1 unknown: d = 16384, (8 * 49152) >> 16 = 6, w = 7: [9,7], t = 12 -> 1
    sm = _sm(dm, scope=1, min_samples=1, floor_w=1, gain=8, target=65536, prior=49152, window=0, **FM)
    case, ks, rows = _case(dm, cfg1, sm, 4, 2, [[True], [True]])
    res = run(case)
    assert evm.weights(sm, rows[0][0], 2) == [9, 7] and evm.draw(U[1], [9, 7]) == (12, 1) and ks[2] == [1]
    _check_script(res, ks, rows, [[True], [True]])
    assert res[1].rows["n_end"][0, :2].tolist() == [1, 1] and res[1].rows["n_fail"][0, :2].tolist() == [1, 1]          # (ks[1] = 1: the second episode ran on record 1)


def _hundred(dm):
    """100 advances of one scene with seed 3049 - the hundredth draw has u = U[2] -, M = 4, a steep model and a window of 8: every third
    episode and every episode on record 3 fails."""
    sm = _sm(dm, scope=0, window=8, fail_mask=BAD_PATH, pass_mask=0, **STEEP)
    fails, ks = [], [[0]]
    for t in range(100):          # (the failure of advance t depends on the record it runs on: the script is grown step by step)
        fails.append([t % 3 == 0 or ks[t][0] == 3])
        ks, rows = script(sm, 3049, 4, fails)
    return sm, fails, ks, rows


def _kat_hundredth_draw(dm, cfg1, run):
    sm, fails, ks, rows = _hundred(dm)
    case, ks2, rows2 = _case(dm, cfg1, sm, 3049, 4, fails)
    assert ks2 == ks
    res = run(case)
    _check_script(res, ks, rows, fails)
    ws = evm.weights(sm, rows[98][0], 4)
    assert evm.draw(U[2], ws)[1] == ks[100][0] == int(res[99].sstats["cur_start"][0])
    hashed = [esm.first_choice(3049, 0, e, 4, 0) for e in range(1, 101)]
    took = [k[0] for k in ks[1:]]
    # the schedule is at work: it departs from the hashed order, leans towards the failing record 3, and the window halves (no count reaches 8)
    assert sum(a != b for a, b in zip(took, hashed)) >= 10 and took.count(3) > hashed.count(3)
    assert max(int(r["n_end"].max()) for r in rows) == 7 and sum(int(r["n_end"].sum()) < int(q["n_end"].sum()) for q, r in zip(rows, rows[1:])) >= 5


KATS = [_kat_first_draw_finds_rows_of_zeros, _kat_second_draw_tables, _kat_hundredth_draw]


def _runner(name):
    return evb.Runner(evb.ModelBackend() if name == "model" else evb.DeviceBackend())


@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, cfg1, kat):
    kat(dm, cfg1, _runner("model"))


def _batch_fails(n, T):
    return [[(3 * s + 5 * t) % 7 < 3 for s in range(n)] for t in range(T)]


def _batch_case(dm, cfg1, n, scope, T=4):
    sm = _sm(dm, scope=scope, window=6 if scope == 0 else 40, fail_mask=BAD_PATH, pass_mask=0, **STEEP)
    return _case(dm, cfg1, sm, 2026, 4, _batch_fails(n, T)) + (_batch_fails(n, T),)


def test_batch_on_the_model(dm, cfg1):
    for scope in (0, 1):
        case, ks, rows, fails = _batch_case(dm, cfg1, 5, scope)
        _check_script(evb.ModelBackend().run(case), ks, rows, fails, f"scope {scope}")


# ---- the closed loop: the followers of tests/test_episode_spawn.py, record 0 in front of the oncoming vehicle, record 1 a clear start ----
C_TICKS, C_MAX, C_BACK = 200, 50, 80
_CPU = {}


def _loop_scene(dm):
    """tests/test_episode_spawn.py::_loop_scene - every ego with a vehicle 20 m ahead that comes towards it at 3 m/s: contact after 37 .. 47
    advances - with a timeout of 50 advances and a second start record 80 lane points further back, which the vehicle does not reach in
    50 advances.  Traffic reset with one set: the vehicle starts every episode where it started the first."""
    r = tes._loop_scene(dm)
    m, si = r["m"], r["sc"]["scene_in"]
    rec1 = si.copy()
    for s in range(tt.F_N):
        loc = rec1["loc"][s]
        lane, pid = int(loc["lane_num"]), int(loc["id"][int(loc["lane_num"]) - 1]) - C_BACK
        p = m["points"][int(m["lanes"][m["road_first_lane"][int(loc["road_num"]) - 1] + lane - 1]["point_off"]) + pid]
        assert pid >= 0
        rec1["loc"]["id"][s, :] = pid
        for f in ("x", "y", "dir"):
            rec1["loc"]["globalpoint"][f][s] = p[f]
    sp = tes._sp(dm, contact=1, n_starts=2, order=0, seed=11)
    sm = _sm(dm, scope=1, fail_mask=CONTACT, pass_mask=0, min_samples=1, window=0, floor_w=4096, gain=61440, target=65536, prior=65536)
    return dict(r, em=te._em(dm, 31, C_MAX), sp=sp, sm=sm, starts=(rec1, r["sc"]["state"].copy()))


def _cpu_loop(dm, oracle, sched):
    if sched in _CPU:
        return _CPU[sched]
    r = _loop_scene(dm)
    cfg, m, sc, n = r["cfg"], r["m"], r["sc"], tt.F_N
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt, hw = float(model["dt"][0]), 0.5 * float(cfg["Vehicle_Width"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(n, np.int32)
    tr = tm.Traffic(r["tracks"], r["pts"], r["act"], si["obs_off"])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    reset = etm.Reset(tr, 1)
    rec1 = ms.resolve(dm, m, r["starts"][0])
    rec1["obs_off"], rec1["obs_n"] = si["obs_off"], si["obs_n"]
    pin, pst = [si.copy(), rec1], [st.copy(), r["starts"][1]]
    stats, sstats, rows = epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n), evm.new_rows(dm.EpisodeScheduleRow, r["sm"], n)
    sins, fl_, causes = [si], [flags], []
    for t in range(C_TICKS):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        q, f, _ = rmod.advance(dm, cfg, model, rm, r["legs"], r["rf"], m, si, plan, st, flags)
        if sched:
            si, st, flags, _, c = evm.step(r["em"], r["sp"], r["sm"], rows, stats, sstats, pin, pst, si, q, f, st, obs, hw)
        else:
            si, st, flags, _, c = esm.step(r["em"], r["sp"], stats, sstats, pin, pst, si, q, f, st, obs, hw)
        obs, _ = tr.place(obs, None, dt)
        obs, _ = reset.step(tr, obs, None, stats["age"], sstats["cur_start"])
        sins.append(si), fl_.append(flags), causes.append(c)
    _CPU[sched] = dict(r, sins=sins, flags=fl_, causes=np.array(causes), stats=stats, sstats=sstats, rows=rows, state=st, s=tr.s.copy())
    return _CPU[sched]


def test_schedule_leans_towards_the_failing_record_on_the_cpu(dm, oracle):
    """target = 65536: the record whose episodes fail gets the weight.  Record 0 ends in contact, record 1 in a timeout; with the schedule
    record 0 is drawn strictly more often than under the hashed order, and the rows add up to the counts of §4k / §4l."""
    a, b = _cpu_loop(dm, oracle, True), _cpu_loop(dm, oracle, False)
    used, hashed, row = a["sstats"]["n_used"].sum(axis=0), b["sstats"]["n_used"].sum(axis=0), a["rows"][0]
    print("n_used with the schedule", used[:2].tolist(), "hashed", hashed[:2].tolist(), "row", row["n_end"][:2].tolist(), row["n_fail"][:2].tolist())
    for r in (a, b):
        c = r["causes"]
        assert set(c[c != 0].tolist()) == {CONTACT, TIMEOUT}
    assert int(used[0]) > int(hashed[0]) and int(used[1]) > 0 and not used[2:].any()
    assert int(row["n_end"].sum()) == int(a["stats"]["n_episodes"].sum()) == int(used.sum()) and int(row["n_fail"].sum()) == int(a["sstats"]["n_contact"].sum())
    assert row["n_fail"][:2].tolist() == [int(row["n_end"][0]), 0]          # every episode on record 0 met its vehicle, none on record 1 did


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg1, kat):
    """The scripted known answers on k_respawn_sched (+ k_fold_schedule in scope 1) behind k_advance_egos, every step also held against
    the model on the device's own records: all of Result and the rows, byte for byte."""
    kat(dm, cfg1, _runner("device"))


@gpu
@pytest.mark.parametrize("n", [4, 5, 300])
@pytest.mark.parametrize("scope", [0, 1], ids=["scene", "pooled"])
def test_batches(dm, cfg1, n, scope):
    """n distinct scripts as the scenes of one launch - one block, the block edge 4 | 5, 75 blocks -, four advances: against the script and,
    every step, against the model on the same batch."""
    case, ks, rows, fails = _batch_case(dm, cfg1, n, scope)
    res = _runner("device")(case)
    _check_script(res, ks, rows, fails)
    assert len({tuple(k) for k in np.array(ks[1:]).T.tolist()}) > 1 and any(int(r["n_end"].max()) >= 3 for r in rows)


@gpu
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_pooled_fold_on_its_chunk_edges(dm, cfg1, n):
    """Every scene ends an episode in every advance: k_fold_schedule sums n words per launch, in chunks of 1024.  A window of 8 is far below
    the endings per record: many halvings per advance.  Rows, cur_start, n_used and the counts of §4k against the script."""
    sm = _sm(dm, scope=1, window=8, fail_mask=BAD_PATH, pass_mask=0, **STEEP)
    fails = [[(s * 7 + t) % 3 == 0 for s in range(n)] for t in range(3)]
    case, ks, rows = _case(dm, cfg1, sm, 9, 4, fails)
    res = evb.DeviceBackend().run(case, light=True)
    _check_script(res, ks, rows, fails)
    assert all(len(set(k)) == 4 for k in ks[2:])          # (the later advances fold endings of every record)


@gpu
def test_one_scene_gives_the_same_bytes_in_both_scopes(dm, cfg1):
    sm, fails, ks, rows = _hundred(dm)
    out = []
    for scope in (0, 1):
        case, _, _ = _case(dm, cfg1, _sm(dm, **dict({k: int(sm[k][0]) for k in sm.dtype.names}, scope=scope)), 3049, 4, fails[:30])
        out.append(evb.DeviceBackend().run(case))
    for t, (a, b) in enumerate(zip(*out)):
        for name in ("out", "flags", "trace", "state", "stats", "sstats", "rows"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (t, name)
    _check_script(out[1], ks[:31], rows[:30], fails[:30])


@gpu
def test_gain_zero_gives_the_bytes_of_k_respawn_spawn(dm, cfg1):
    """gain = 0 is the neutral model: every byte of §4l with order 0 - 9 scenes, M = 3 and 16, six advances with failures - while the rows
    still count."""
    for M in (3, 16):
        fails = _batch_fails(9, 6)
        out = []
        for sm in (None, _sm(dm, scope=0, gain=0, floor_w=777, window=4, **FM), _sm(dm, scope=1, gain=0, **FM)):
            case, ks, rows = _case(dm, cfg1, sm, 2026, M, fails)
            out.append(evb.DeviceBackend().run(case))
            if sm is not None:
                _check_script(out[-1], ks, rows, fails)
        assert ks[1:] == [[esm.first_choice(2026, s, e, M, 0) for s in range(9)] for e in range(1, 7)]
        for other in out[1:]:
            for t, (a, b) in enumerate(zip(out[0], other)):
                for name in ("out", "flags", "trace", "state", "stats", "sstats"):
                    assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (M, t, name)


@gpu
def test_clearance_walk_starts_from_the_scheduled_record(dm, cfg1):
    """_kat_second_draw_tables with a blocker beside record 0 (the capture at (110, 0); clearance 2: (3.5 - 0.5) - 1 = 2 -> blocked): the second
    draw's k0 = 0 is the SCHEDULED record, the hashed one would be 3; the walk moves on to record 1 with one rejection."""
    sm = _sm(dm, scope=0, min_samples=1, floor_w=1, gain=12, target=65536, prior=0, window=0, **FM)
    case, ks, rows = _case(dm, cfg1, sm, 4, 4, [[True], [False]], check=1, obs=tes._obs(dm, [(110.0, 3.5)]), sp_kw=dict(clearance=2.0))
    assert ks[1] == [2] and ks[2] == [0] and esm.first_choice(4, 0, 2, 4, 0) == 3
    res = _runner("device")(case)
    assert int(res[0].sstats["cur_start"][0]) == 2 and int(res[0].sstats["n_rejected"][0]) == 0
    assert int(res[1].sstats["cur_start"][0]) == 1 and int(res[1].sstats["n_rejected"][0]) == 1 and res[1].sstats["n_used"][0, :4].tolist() == [0, 1, 1, 0]
    assert res[1].rows.tobytes() == rows[1].tobytes()          # (the rows count the record an episode RAN on: 0, then 2)


def _planner(dm, r, sched=True, log=0):
    pl = tes._planner(dm, dict(r, sp=None), spawn=False)
    pl.set_episode_spawn(r["sp"], *r["starts"])
    pl.set_episode_traffic(1)
    if log:
        pl.set_episode_log(log)
    if sched:
        pl.set_episode_schedule(r["sm"])
    return pl


_RUNS = {}


def _device_loop(dm, oracle):
    if "loop" in _RUNS:
        return _RUNS["loop"]
    r = _cpu_loop(dm, oracle, True)
    pl = _planner(dm, r, log=4096)
    n, model = tt.F_N, dm.default_ego_model()
    trace = dm.pinned_empty(n, dm.EgoTrace)
    run = dict(sins=[pl.get_scene_in()], flags=[np.zeros(n, np.int32)], trace=[])
    for t in range(C_TICKS):
        pl.tick()
        pl.advance_async(model, trace)
        run["sins"].append(pl.get_scene_in()), run["flags"].append(pl.ego_flags())
        pl.sync()
        run["trace"].append(np.array(trace))
    pl.tick()
    pl.sync()
    run["last"] = _last(pl)
    run["log"] = pl.read_episode_log()[0]
    pl.close()
    _RUNS["loop"] = run
    return run


_NAMES = ("PlanOut", "SceneState", "flags", "SceneIn", "EpisodeStats", "EpisodeSpawnStats", "traffic", "resets", "rows")


def _last(pl, rows=True):
    return (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), pl.episode_stats(), pl.episode_spawn_stats(), pl.traffic_state(),
            pl.episode_traffic_resets(), pl.episode_schedule() if rows else np.zeros(0))


@gpu
def test_closed_loop_agrees_with_the_cpu_loop(dm, oracle):
    """200 advances of the followers with the schedule, the traffic reset and the episode log on: every staged record against the CPU loop -
    every byte but the heading -, equal flag words, the stats of §4k and §4l equal in every integer field, the row byte for byte; and the
    log tells the same story as the row."""
    r, d = _cpu_loop(dm, oracle, True), _device_loop(dm, oracle)
    for t in range(C_TICKS + 1):
        assert np.array_equal(d["flags"][t], r["flags"][t]), f"set {t}: flags"
        te._assert_records(d["sins"][t], r["sins"][t], f"set {t}")
    got, sgot, rows = d["last"][4], d["last"][5], d["last"][8]
    for name in te._INT_FIELDS:
        assert np.array_equal(got[name], r["stats"][name]), name
    for name in tes._SP_INT:
        assert np.array_equal(sgot[name], r["sstats"][name]), name
    assert rows.tobytes() == r["rows"].tobytes() and d["last"][6].tobytes() == r["s"].tobytes()
    log = d["log"]
    assert len(log) == int(got["n_episodes"].sum()) > 16
    assert [int((log["start"] == k).sum()) for k in range(2)] == rows["n_end"][0, :2].tolist()
    assert [int(((log["start"] == k) & ((log["cause"] & CONTACT) != 0)).sum()) for k in range(2)] == rows["n_fail"][0, :2].tolist()


@gpu
def test_rollout_with_the_schedule_equals_its_parts(dm, oracle):
    r, d = _cpu_loop(dm, oracle, True), _device_loop(dm, oracle)
    pl = _planner(dm, r, log=4096)
    last, trace = pl.rollout(C_TICKS, trace=True)
    pl.sync()
    got, log = _last(pl), pl.read_episode_log()[0]
    pl.close()
    assert last == C_TICKS + 1
    for a, b, name in zip(got, d["last"], _NAMES):
        assert a.tobytes() == b.tobytes(), name
    assert log.tobytes() == d["log"].tobytes() and np.array(trace).tobytes() == np.array(d["trace"]).tobytes()


@gpu
def test_off_means_off(dm, oracle):
    """A handle that sets the schedule and switches it off gives the bytes of one that never set it - k_respawn_spawn runs again - and its
    rows stay readable, untouched; a handle that never set it has none."""
    r = _cpu_loop(dm, oracle, True)
    outs = []
    for had in (True, False):
        pl = _planner(dm, r, sched=had)
        if had:
            pl.rollout(60)
            before = pl.episode_schedule()
            assert int(before["n_end"].sum()) == int(pl.episode_stats()["n_episodes"].sum()) > 0
            pl.close()
            pl = _planner(dm, r, sched=True)
            pl.set_episode_schedule(off=True)
        pl.rollout(120)
        pl.sync()
        outs.append(_last(pl, rows=False))
        if had:
            assert not pl.episode_schedule().tobytes().strip(b"\0")
        else:
            with pytest.raises(dm.PlannerError, match="error -4:"):
                pl.episode_schedule()
        pl.close()
    for a, b, name in zip(outs[0], outs[1], _NAMES):
        assert a.tobytes() == b.tobytes(), name
    assert outs[0][4]["n_episodes"].sum() > 16


@gpu
def test_a_refused_spawn_model_leaves_the_schedule_drawing(dm):
    """pp_set_episode_spawn retires the schedule before it knows whether its records are on the map; a start record off the map is refused and
    the schedule is back: rows (one per scene), spawn stats and the run are those of a reference handle, and the rows go on changing."""
    r = _loop_scene(dm)
    r["sm"] = r["sm"].copy()
    r["sm"]["scope"] = 0

    def fresh():
        p = _planner(dm, r)
        p.rollout(60)
        p.sync()
        return p
    pl, ref = fresh(), fresh()
    before = pl.episode_schedule()
    assert before.shape == (tt.F_N,) and int(before["n_end"].sum()) > 0
    off_map = (r["starts"][0].copy(), r["starts"][1])
    off_map[0]["loc"]["road_num"][1] = 99
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_episode_spawn(r["sp"], *off_map)
    for p in (pl, ref):
        p.rollout(60)
        p.sync()
    for a, b, name in zip(_last(pl), _last(ref), _NAMES):
        assert a.tobytes() == b.tobytes(), name
    ref.close()
    rows = pl.episode_schedule()
    assert rows.tobytes() != before.tobytes() and int(rows["n_end"].sum()) > int(before["n_end"].sum())
    pl.close()


@gpu
def test_errors_and_lifetime(dm, oracle):
    r = _cpu_loop(dm, oracle, True)
    n, sm = tt.F_N, r["sm"]
    # PP_ERR_STATE: no spawn model; a round-robin one; nothing readable on a handle that never set a schedule
    pl = tes._planner(dm, dict(r, sp=None), spawn=False)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_schedule(sm)
    pl.set_episode_spawn(tes._sp(dm, contact=1, n_starts=2, order=1), *r["starts"])
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_schedule(sm)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.episode_schedule()
    pl.close()

    def fresh():
        p = _planner(dm, r, log=512)
        p.rollout(60)
        return p
    pl, ref = fresh(), fresh()
    for kw in (dict(scope=2), dict(scope=-1), dict(fail_mask=256), dict(pass_mask=32), dict(min_samples=0), dict(window=1), dict(window=-3), dict(floor_w=0),
               dict(floor_w=65536), dict(gain=-1), dict(gain=65536), dict(target=-1), dict(target=65537), dict(prior=65537), dict(_pad=5)):
        with pytest.raises(dm.PlannerError, match="error -1:"):                # PP_ERR_ARG
            pl.set_episode_schedule(_sm(dm, **kw))
    pl.advance_async()
    ref.advance_async()
    for kw in (dict(model=sm), dict(off=True)):                                # PP_ERR_STATE: an update is staged
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.set_episode_schedule(**kw)
    # none of it changed the schedule, its rows or anything else: the run goes on like the reference run - and the schedule retired nothing
    for p in (pl, ref):
        p.tick()
        p.rollout(60)
        p.sync()
    for a, b, name in zip(_last(pl), _last(ref), _NAMES):
        assert a.tobytes() == b.tobytes(), name
    assert pl.read_episode_log()[0].tobytes() == ref.read_episode_log()[0].tobytes() and pl.episode_traffic_resets().any()
    ref.close()
    rows = pl.episode_schedule()
    assert int(rows["n_end"].sum()) == int(pl.episode_stats()["n_episodes"].sum()) > 16
    # a second set call zeroes the rows and - in the other scope - reads them per scene; it leaves the log and the reset on
    pl.set_episode_schedule(_sm(dm, scope=0))
    assert pl.episode_schedule().shape == (n,) and not pl.episode_schedule().tobytes().strip(b"\0")
    lib = dm.load_library()
    for bad_n in (-1, n + 1):
        assert lib.pp_get_episode_schedule(pl.h, rows.ctypes.data, bad_n) == dm.PP_ERR_ARG
    pl.rollout(60)
    assert pl.episode_schedule()["n_end"].sum() > 0 and len(pl.read_episode_log()[0]) > 0
    # every successful pp_set_episode_spawn leaves no schedule: the rows stay readable and stand still, k_respawn_spawn runs
    pl.set_episode_spawn(r["sp"], *r["starts"])
    before = pl.episode_schedule()
    pl.rollout(60)
    assert pl.episode_schedule().tobytes() == before.tobytes() and pl.episode_spawn_stats()["n_used"].sum() > 0
    # ... NULL included, and then there is no spawn model to schedule
    pl.set_episode_schedule(sm)
    assert lib.pp_get_episode_schedule(pl.h, rows.ctypes.data, 2) == dm.PP_ERR_ARG          # (pooled scope: n is 1)
    pl.set_episode_spawn(None)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_schedule(sm)
    # pp_set_episodes retires the spawn model and the schedule with it: setting the same spawn model again starts without one
    pl.set_episode_spawn(r["sp"], *r["starts"])
    pl.set_episode_schedule(sm)
    pl.rollout(60)
    pl.set_episodes(r["em"])
    pl.set_episode_spawn(r["sp"], *r["starts"])
    before = pl.episode_schedule()
    pl.rollout(60)
    assert pl.episode_schedule().tobytes() == before.tobytes() and int(before["n_end"].sum()) > 0
    # pp_set_egos retires it through the episodes
    pl.set_episode_schedule(sm)
    pl.set_egos(r["sc"], with_motion=False)
    pl.set_state(r["sc"]["state"])
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_schedule(sm)
    assert not pl.episode_schedule().tobytes().strip(b"\0")
    pl.close()
