"""Episode traffic reset (pp_set_episode_traffic / pp_get_episode_traffic_resets / k_reset_traffic): when an ego
restarts, the actors of its scene go back to a start state - start record k plus traffic set k is scenario k.

CPU: the ABI mirror, hand-derived known answers of the numpy model (tests/episode_traffic_model.py) on the 3-4-5 triangle of
tests/test_traffic.py, and the two closed loops of the issue: the contact loop of tests/test_episode_spawn.py and the chased egos
of tests/test_traffic_follow.py with a timeout, both with the reset - every later episode repeats the first byte for byte - and
the chased loop without it, which does not repeat.
GPU: the known answers on k_reset_traffic alone and as distinct scenes of one launch (batches of 5 and 9), with and without a
motion pool, with following off and on, behind k_respawn_egos and k_respawn_spawn; the thread-per-actor edges (1, 255, 256, 257
and 513 actors, scenes with 0, 1 and 3 actors); both closed loops against their CPU loops; pp_rollout against its parts; off means
off; every refusal; every switch-off site; the getter's error paths.

The geometry of the known answers.  The egos are those of tests/test_episodes.py on its two-road map, routed (k_advance_route): the
ego at (110, 0) on lane 2 drives on ("go"); the ego at (132, 3.75) on lane 1 goes on once and then runs into its lane end
("two": advances 1 and 2 restart it, "back": advance 1 restarts it and the plan of advance 2 leads on from the start record); the
ego at (133, 3.75) ends at once ("once": every advance restarts it).  The tracks lie at the origin, more than 100 m from any ego,
so with following on no ego ever leads.  EgoModel.dt is 0.1 and the scripted speeds are +-10 m/s: 10 * 0.1 rounds to 1.0 exactly,
so an actor moves one metre per advance and every arc length and pose below is exact."""
import itertools

import numpy as np
import pytest

import episode_model as epm
import episode_spawn_model as esm
import episode_traffic_backends as etb
import episode_traffic_model as etm
import map_scenes as ms
import route_model as rmod
import test_episode_spawn as tes
import test_episodes as te
import test_traffic as tt
import test_traffic_follow as tf
import traffic_follow_model as fm
import traffic_model as tm
import traffic_scenes as ts

gpu = pytest.mark.gpu
TRI = tt.TRI
FAR = tes.FAR


# ---------------------------------------------------------------------------------------------------------------
# CPU: ABI
def test_abi_mirror(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(33) == dm.TrafficStart.itemsize == 16
    assert [dm.TrafficStart.fields[k][1] for k in ("s", "v")] == [0, 8]
    assert hasattr(lib, "pp_set_episode_traffic") and hasattr(lib, "pp_get_episode_traffic_resets")
    assert [lib.pp_sizeof(k) for k in range(26, 33)] == [16, 40, 64, 8, 80, 32, 80]          # (the records of §4h - §4l are as they were)
    assert 10.0 * 0.1 == 1.0 and float(dm.default_ego_model()["dt"][0]) == 0.1               # (what the known answers below lean on)


# ---------------------------------------------------------------------------------------------------------------
# the known answers, written once against a Runner of tests/episode_traffic_backends.py
VARIANTS = list(itertools.product((False, True), repeat=3))          # (following, motion pool, k_respawn_spawn with M = 1)


def _vid(v):
    return "-".join(n for n, on in zip(("follow", "motion", "spawn"), v) if on) or "plain"


def _starts(dm, n):
    return np.zeros(n, dm.TrafficStart)


class _Tr:
    """Advances of ONE scene with its actors: rows are (s0, speed, track, type, radius), actor a in slot a of the scene's slice, a static
    entry behind them.  M > 1: a round-robin spawn model whose records all stand on the ego's pose (told apart by period_last)."""
    def __init__(self, dm, runner, follow=False, motion=False, spawn=False):
        self.dm, self.run, self.name, self.follow, self.motion, self.spawn = dm, runner, getattr(runner, "name", None), follow, motion, spawn

    def case(self, kind, polylines, rows, n_sets=1, sets=None, M=1):
        dm, y = self.dm, 3.75
        if kind == "go":
            si, pos = te._ego(dm, 110.0, ego_id=20), [te._path(dm, 110.0), te._path(dm, 111.0), te._path(dm, 112.0)]
        elif kind in ("two", "back"):
            si = te._ego(dm, 132.0, y=y, lane=1, ego_id=60)
            pos = [te._path(dm, 132.0, y=y), te._path(dm, 133.0, y=y), te._path(dm, 133.5 if kind == "two" else 132.0, y=y)]
        else:
            si, pos = te._ego(dm, 133.0, y=y, lane=1, ego_id=60), [te._path(dm, 133.0, y=y)] * 3
        sp, starts = (tes._sp(dm) if self.spawn else None), None
        if M > 1:
            sp, ins, sts = tes._sp(dm, n_starts=M, order=1), [], []
            for k in range(1, M):
                r, s = si.copy(), te._state0(dm)
                r["period_last"], s["tick"] = 100.0 + k, 7 + 10 * k
                ins.append(r), sts.append(s)
            starts = (np.concatenate(ins), np.concatenate(sts))
        tstarts = None
        if sets is not None:                                     # sets[k - 1][a] = (s*, v*) of set k of actor a
            tstarts = _starts(dm, len(sets) * len(rows))
            tstarts["s"], tstarts["v"] = [p[0] for st in sets for p in st], [p[1] for st in sets for p in st]
        obs = tes._obs(dm, [FAR] * (len(rows) + 1))
        cfg = dm.default_config(128)
        cfg["grid_stage"] = 0
        route = (te._legs(dm), np.array([0, 2], np.int32), dm.default_route_model())
        return etb.Case(cfg, dm.default_ego_model(), te._em(dm), sp, si, [obs], te._state0(dm), list(zip(pos, [np.zeros(1, dm.SceneState) for _ in pos])),
                        te._world(dm), route, starts, polylines, [(r[0], r[1], 0, a, r[2], r[3], r[4]) for a, r in enumerate(rows)], n_sets, tstarts,
                        dm.default_traffic_follow() if self.follow else None, self.motion)

    def __call__(self, *args, **kw):
        case = self.case(*args, **kw)
        res = self.run(case)
        for r in res:                                            # the static entry behind the actors: never written
            assert r.pool[len(case.rows)].tobytes() == tes._obs(self.dm, [FAR])[0].tobytes()
            assert r.mot is None or (r.mot[len(case.rows)].tobytes() != bytes(16) and r.mot[:len(case.rows)].tobytes() == bytes(16 * len(case.rows)))
        return res


def _at(r, a):
    return float(r.s[a]), float(r.pool["x"][a]), float(r.pool["y"][a])


def _v(tr, r, want):
    """The speeds, where following is on (without it there are none)."""
    assert (r.v is None) == (not tr.follow)
    return True if r.v is None else r.v.tolist() == want


def _closed(dm):
    return [(ts.polyline(dm, TRI), True)]


def _kat_reset_after_the_actor_moved(dm, tr):
    # the triangle, cum = 0, 4, 7, 12.  The call captures s = 2, v = speed = 10.  Advance 0 (the scene goes on): 2 + 10 * 0.1 = 3 -> (3, 0) - with
    # following: v / speed = 1, free = 1 - 1 = 0, acc = 0, v1 = 10, s = 2 + (0.5 * 20) * 0.1 = 3 as well.  Advance 1 steps to 4 and restarts: the
    # step is discarded, s' = wrap(2) = 2 -> segment 0, t = 2 / 4 -> (2, 0), v' = 10, one reset.  Advance 2 restarts again: 2, two resets.
    r = tr("two", _closed(dm), [(2.0, 10.0, 0, 7, 0.75)])
    assert [_at(q, 0) for q in r] == [(3.0, 3.0, 0.0), (2.0, 2.0, 0.0), (2.0, 2.0, 0.0)]
    assert [q.resets.tolist() for q in r] == [[0], [1], [2]] and [int(q.stats["age"][0]) for q in r] == [1, 0, 0]
    assert all(_v(tr, q, [10.0]) for q in r)
    assert all((int(q.pool["type"][0]), float(q.pool["radius"][0])) == (7, 0.75) for q in r)


def _kat_a_scene_that_goes_on_keeps_the_traffic_kernels_bytes(dm, tr):
    # the ego at 110 never restarts: 3 -> (3, 0), 4 -> the vertex (4, 0), 5 -> segment 1, t = 1 / 3 -> (4, (1 / 3) * 3); no reset is counted and
    # every byte is that of the same run without pp_set_episode_traffic
    case = tr.case("go", _closed(dm), [(2.0, 10.0, 0, 7, 0.75)])
    r, plain = tr.run(case), tr.run(case.without_reset())
    assert [_at(q, 0) for q in r] == [(3.0, 3.0, 0.0), (4.0, 4.0, 0.0), (5.0, 4.0, (1.0 / 3.0) * 3.0)]
    assert [q.resets.tolist() for q in r] == [[0]] * 3 and all(p.resets is None for p in plain)
    for q, p in zip(r, plain):
        assert q.s.tobytes() == p.s.tobytes() and q.pool.tobytes() == p.pool.tobytes() and (q.v is None or q.v.tobytes() == p.v.tobytes())
        assert q.mot is None or q.mot.tobytes() == p.mot.tobytes()


def _kat_start_states_wrap_clamp_and_sit_on_vertices(dm, tr):
    # M = 2, round robin, every advance restarts: advance 0 takes record 1 -> set 1, advance 1 record 0 -> set 0 (the capture), advance 2 set 1.
    # Set 1 on the closed triangle (L = 12): 27 -> q = floor(27 / 12) = 2, 27 - 24 = 3 -> (3, 0); -2.5 -> q = -1, -2.5 + 12 = 9.5 -> the closing
    # segment, t = 2.5 / 5 -> (2, 1.5); on the open track (0, 0) -> (10, 0): 25 -> L = 10 -> (10, 0); -1 -> 0 -> (0, 0).  On a vertex: 4 = cum[1] ->
    # segment 1, t = 0 -> (4, 0); 7 = cum[2] -> (4, 3); 12 = L -> q = 1, 0 -> (0, 0).  v' = 3 for all of them (speed > 0).
    polylines = _closed(dm) + [(ts.polyline(dm, [(0.0, 0.0), (10.0, 0.0)]), False)]
    rows = [(1.0, 10.0, 0, 1, 0.5), (1.0, 10.0, 0, 2, 0.5), (5.0, 10.0, 1, 3, 0.5), (5.0, 10.0, 1, 4, 0.5), (1.0, 10.0, 0, 5, 0.5), (1.0, 10.0, 0, 6, 0.5), (1.0, 10.0, 0, 7, 0.5)]
    set1 = [(27.0, 3.0), (-2.5, 3.0), (25.0, 3.0), (-1.0, 3.0), (4.0, 3.0), (7.0, 3.0), (12.0, 3.0)]
    r = tr("once", polylines, rows, 2, [set1], M=2)
    one = [(3.0, 3.0, 0.0), (9.5, 2.0, 1.5), (10.0, 10.0, 0.0), (0.0, 0.0, 0.0), (4.0, 4.0, 0.0), (7.0, 4.0, 3.0), (0.0, 0.0, 0.0)]
    zero = [(1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (5.0, 5.0, 0.0), (5.0, 5.0, 0.0), (1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (1.0, 1.0, 0.0)]
    assert [[_at(q, a) for a in range(7)] for q in r] == [one, zero, one]
    assert [int(q.sstats["cur_start"][0]) for q in r] == [1, 0, 1] and [q.resets.tolist() for q in r] == [[k] * 7 for k in (1, 2, 3)]
    assert _v(tr, r[0], [3.0] * 7) and _v(tr, r[1], [10.0] * 7) and _v(tr, r[2], [3.0] * 7)


def _kat_parked_and_reversing_actors_keep_their_speed(dm, tr):
    # a parked actor (speed 0) and a reversing one (-10) take s* and keep v = speed whatever the set says (§4i); the driving one takes v* = 4.
    # s* = 5: segment 1, t = 1 / 3 -> (4, (1 / 3) * 3); s* = 6: t = 2 / 3 -> (4, (2 / 3) * 3); s* = 1 -> (1, 0).  Advance 1 takes set 0 again.
    rows = [(5.5, 0.0, 0, 1, 0.5), (9.5, -10.0, 0, 2, 0.5), (2.0, 10.0, 0, 3, 0.5)]
    r = tr("once", _closed(dm), rows, 2, [[(5.0, 3.0), (6.0, 2.5), (1.0, 4.0)]], M=2)
    assert [_at(r[0], a) for a in range(3)] == [(5.0, 4.0, (1.0 / 3.0) * 3.0), (6.0, 4.0, (2.0 / 3.0) * 3.0), (1.0, 1.0, 0.0)]
    assert [_at(r[1], a) for a in range(3)] == [(5.5, 4.0, 1.5), (9.5, 2.0, 1.5), (2.0, 2.0, 0.0)]
    assert _v(tr, r[0], [0.0, -10.0, 4.0]) and _v(tr, r[1], [0.0, -10.0, 10.0]) and _v(tr, r[2], [0.0, -10.0, 4.0])


def _kat_the_next_advance_drives_on_from_the_start_state(dm, tr):
    # advance 1 restarts the scene onto record 1 -> set 1: s = 1, v = 4; the plan of advance 2 leads on from the start record, so the scene goes on
    # and the traffic kernel steps from the start state.  Scripted: 1 + 1 = 2 -> (2, 0).  Following (free road): r = 4 / 10, acc = 1 * (1 - r^2 r^2),
    # v1 = 4 + acc * 0.1, s = 1 + 0.5 * (4 + v1) * 0.1.  The parked actor - on a track of its own: it leads nobody - stays on its s* = 5.
    rows, sets = [(2.0, 10.0, 0, 1, 0.5), (5.5, 0.0, 1, 2, 0.5)], [[(1.0, 4.0), (5.0, 9.0)]]
    polylines = _closed(dm) + [(ts.polyline(dm, [(0.0, 0.0), (10.0, 0.0)]), False)]
    r = tr("back", polylines, rows, 2, sets, M=2)
    assert [int(q.stats["age"][0]) for q in r] == [1, 0, 1] and [q.resets.tolist() for q in r] == [[0, 0], [1, 1], [1, 1]]
    assert _at(r[0], 0) == (3.0, 3.0, 0.0) and _at(r[1], 0) == (1.0, 1.0, 0.0) and [_at(q, 1)[0] for q in r] == [5.5, 5.0, 5.0]
    if tr.follow:
        rr = 4.0 / 10.0
        r2 = rr * rr
        v1 = 4.0 + (1.0 * (1 - r2 * r2)) * 0.1
        assert r[1].v.tolist() == [4.0, 0.0] and r[2].v.tolist() == [v1, 0.0] and float(r[2].s[0]) == 1.0 + 0.5 * (4.0 + v1) * 0.1
    else:
        assert _at(r[2], 0) == (2.0, 2.0, 0.0)
    # the scene beside it that never restarts drives on through all of it
    g = tr("go", polylines, rows, 2, sets, M=2)
    assert [_at(q, 0)[0] for q in g] == [3.0, 4.0, 5.0] and [q.resets.tolist() for q in g] == [[0, 0]] * 3


def _kat_a_start_record_that_ends_at_once(dm, tr):
    # every advance ends an episode: the actor is reset on every advance, stays on its start state, and n_resets counts the advances
    r = tr("once", _closed(dm), [(2.0, 10.0, 0, 7, 0.75)])
    for k, q in enumerate(r):
        assert _at(q, 0) == (2.0, 2.0, 0.0) and q.resets.tolist() == [k + 1] and int(q.stats["n_episodes"][0]) == k + 1 and _v(tr, q, [10.0])


def _kat_the_set_follows_the_start_record(dm, tr):
    # n_sets = M = 3, round robin: the restarts take records 1, 2, 0 and the actor sets 1, 2, 0: 5.5 -> (4, 1.5), 9.5 -> (2, 1.5), the capture 2 -> (2, 0)
    rows, sets = [(2.0, 10.0, 0, 7, 0.75)], [[(5.5, 1.0)], [(9.5, 2.0)]]
    r = tr("once", _closed(dm), rows, 3, sets, M=3)
    assert [int(q.sstats["cur_start"][0]) for q in r] == [1, 2, 0]
    assert [_at(q, 0) for q in r] == [(5.5, 4.0, 1.5), (9.5, 2.0, 1.5), (2.0, 2.0, 0.0)]
    assert _v(tr, r[0], [1.0]) and _v(tr, r[1], [2.0]) and _v(tr, r[2], [10.0])
    g = tr("go", _closed(dm), rows, 3, sets, M=3)
    assert [_at(q, 0)[0] for q in g] == [3.0, 4.0, 5.0] and not g[2].resets.any()


def _kat_one_set_for_every_start_record(dm, tr):
    # n_sets = 1 with M = 3: the restarts take records 1, 2, 0 and the actor set 0 every time
    r = tr("once", _closed(dm), [(2.0, 10.0, 0, 7, 0.75)], 1, None, M=3)
    assert [int(q.sstats["cur_start"][0]) for q in r] == [1, 2, 0]
    assert [_at(q, 0) for q in r] == [(2.0, 2.0, 0.0)] * 3 and r[2].resets.tolist() == [3]
    g = tr("go", _closed(dm), [(2.0, 10.0, 0, 7, 0.75)], 1, None, M=3)
    assert [_at(q, 0)[0] for q in g] == [3.0, 4.0, 5.0] and not g[2].resets.any()


KATS = [_kat_reset_after_the_actor_moved, _kat_a_scene_that_goes_on_keeps_the_traffic_kernels_bytes, _kat_start_states_wrap_clamp_and_sit_on_vertices,
        _kat_parked_and_reversing_actors_keep_their_speed, _kat_the_next_advance_drives_on_from_the_start_state, _kat_a_start_record_that_ends_at_once,
        _kat_the_set_follows_the_start_record, _kat_one_set_for_every_start_record]


def _runner(name, log=None):
    return etb.Runner(etb.ModelBackend() if name == "model" else etb.DeviceBackend(), log)


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, kat, variant):
    kat(dm, _Tr(dm, _runner("model"), *variant))


_LOGS = {}


def _kat_log(dm, variant):
    if variant not in _LOGS:
        log = []
        for kat in KATS:
            kat(dm, _Tr(dm, _runner("model", log), *variant))
        _LOGS[variant] = log
    return _LOGS[variant]


def _check_batches(ran):
    assert {n for n, _ in ran} == {5, 9}
    for size in (5, 9):
        assert any({0, 3, 4, size - 1} <= set(e) and len(e) < size for n, e in ran if n == size)


def test_kat_batches_on_the_model(dm):
    """The batching of tests/episode_traffic_backends.py itself: the model on a batch gives every scene the bytes it gave alone."""
    _check_batches(etb.batched(_kat_log(dm, (True, True, True)), backend=etb.ModelBackend()))


# ---- the closed loops of the issue ------------------------------------------------------------------------------------------------
_CPU = {}
C_EPISODES = [3, 2, 3, 2, 3, 3, 2, 2, 3, 3, 3, 3, 2, 2, 2, 2]
C_AGES = [37, 43, 38, 42, 38, 39, 44, 43, 39, 39, 38, 39, 43, 47, 45, 46]


def _contact_loop(dm, oracle):
    """tests/test_episode_spawn.py::_cpu_loop - 16 followers, the vehicle 20 m ahead at -3 m/s, contact = 1, 120 advances - with the actors
    of a restarted scene put back behind the traffic step.  sins[t] / s[t] / pools[t]: what tick t reads."""
    if "contact" in _CPU:
        return _CPU["contact"]
    r = tes._loop_scene(dm)
    cfg, m, sc, n = r["cfg"], r["m"], r["sc"], tt.F_N
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt, hw = float(model["dt"][0]), 0.5 * float(cfg["Vehicle_Width"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(n, np.int32)
    tr = tm.Traffic(r["tracks"], r["pts"], r["act"], si["obs_off"])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    reset = etm.Reset(tr, 1)
    pin, pst = [si.copy()], [st.copy()]
    stats, sstats = epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n)
    sins, fl_, causes, ss, pools = [si], [flags], [], [tr.s.copy()], [obs]
    for t in range(tes.L_TICKS):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        q, f, _ = rmod.advance(dm, cfg, model, rm, r["legs"], r["rf"], m, si, plan, st, flags)
        si, st, flags, _, c = esm.step(r["em"], r["sp"], stats, sstats, pin, pst, si, q, f, st, obs, hw)
        obs, _ = tr.place(obs, None, dt)
        obs, _ = reset.step(tr, obs, None, stats["age"], sstats["cur_start"])
        sins.append(si), fl_.append(flags), causes.append(c), ss.append(tr.s.copy()), pools.append(obs)
    _CPU["contact"] = dict(r, sins=sins, flags=fl_, causes=np.array(causes), s=ss, pools=pools, stats=stats, sstats=sstats, state=st, resets=reset.n_resets.copy())
    return _CPU["contact"]


def _episodes_repeat(r, names, n):
    """Every later episode of every ego stages the sequences `names` of its first episode byte for byte (the last, unfinished one a prefix)."""
    T = len(r["causes"])
    for k in range(n):
        ends = np.flatnonzero(r["causes"][:, k])                 # advance t ended an episode: set t + 1 holds the start states again
        first = [tuple(r[name][t][k].tobytes() for name in names) for t in range(0, ends[0] + 1)]
        for a, b in zip(list(ends), list(ends[1:]) + [T]):
            later = [tuple(r[name][t][k].tobytes() for name in names) for t in range(a + 1, min(b, T) + 1)]
            assert later == first[:len(later)] and later, f"ego {k}: the episode behind advance {a} is not its first one"


def test_contact_loop_repeats_its_first_episode_on_the_cpu(dm, oracle):
    """With the reset the §4l contact loop has no age-1 episodes: every ego plays its first episode again and again - the same age, the
    only cause DMPP_EGO_CONTACT - and every later episode stages the SceneIn records and the actor's arc lengths of the first byte for byte."""
    r = _contact_loop(dm, oracle)
    s, ss, causes = r["stats"], r["sstats"], r["causes"]
    print("episodes", s["n_episodes"].tolist(), "ages", s["min_age"].tolist(), s["max_age"].tolist())
    assert s["n_episodes"].tolist() == C_EPISODES
    assert s["min_age"].tolist() == C_AGES and s["max_age"].tolist() == C_AGES
    assert set(causes[causes != 0].tolist()) == {tes.CONTACT} and np.array_equal(ss["n_contact"], s["n_episodes"]) and not s["n_end"].any()
    assert r["resets"].tolist() == C_EPISODES                    # (one actor per scene: reset with every restart)
    _episodes_repeat(r, ("sins", "s"), tt.F_N)
    # the loop of tests/test_episode_spawn.py, without the reset, restarts into the vehicle: episodes of age 1
    assert (tes._cpu_loop(dm, oracle)["stats"]["min_age"] == 1).all()


H_TICKS, H_MAX = 200, 60


def _chased_loop(dm, oracle, reset):
    """tests/test_traffic_follow.py::_cpu_loop with following on - the vehicle 12 m behind every ego that wants 6 m/s - and episodes with
    end_mask = 31, max_ticks = 60 over 200 advances; reset: the actors of a restarted scene are put back (s and v)."""
    if ("chased", reset) in _CPU:
        return _CPU[("chased", reset)]
    cfg, m, sc, legs, rf, tracks, pts, act = tf._chased(dm)
    n, model, rm, em = tf.A_N, dm.default_ego_model(), dm.default_route_model(), te._em(dm, 31, H_MAX)
    dt = float(model["dt"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"].copy()), sc["state"].copy(), np.zeros(n, np.int32)
    tr = fm.Follow(tracks, pts, act, si["obs_off"])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    rs_ = etm.Reset(tr, 1, None, True) if reset else None
    start_in, start_state, stats = si.copy(), st.copy(), epm.new_stats(dm.EpisodeStats, n)
    sins, fl_, causes, ss, vs, pools = [si], [flags], [], [tr.s.copy()], [tr.v.copy()], [obs]
    for t in range(H_TICKS):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        q, f, _ = rmod.advance(dm, cfg, model, rm, legs, rf, m, si, plan, st, flags)
        si, st, flags, _, c = epm.step(em, stats, start_in, start_state, si, q, f, st)
        obs, _ = tr.step(obs, None, dt, None, si, flags, float(cfg["Vehicle_Width"][0]))
        if rs_ is not None:
            obs, _ = rs_.step(tr, obs, None, stats["age"])
        sins.append(si), fl_.append(flags), causes.append(c), ss.append(tr.s.copy()), vs.append(tr.v.copy()), pools.append(obs)
    _CPU[("chased", reset)] = dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, tracks=tracks, pts=pts, act=act, em=em, sins=sins, flags=fl_, causes=np.array(causes),
                                   s=ss, v=vs, pools=pools, stats=stats, state=st, resets=None if rs_ is None else rs_.n_resets.copy())
    return _CPU[("chased", reset)]


def test_chased_loop_repeats_with_the_reset_and_not_without_it_on_the_cpu(dm, oracle):
    """3 episodes per ego, each ended by the timeout alone.  With the reset (SceneIn, s, v) of set 60 e + j equal those of set j byte for
    byte: SceneIn + SceneState + (s, v) is the whole memory of a scene.  Without it the vehicles carry on and no ego repeats."""
    on, off = _chased_loop(dm, oracle, True), _chased_loop(dm, oracle, False)
    for r in (on, off):
        assert (r["stats"]["n_episodes"] == 3).all() and set(r["causes"][r["causes"] != 0].tolist()) == {epm.TIMEOUT}
        assert np.flatnonzero(r["causes"].any(axis=1)).tolist() == [59, 119, 179]
    assert on["resets"].tolist() == [3] * tf.A_N
    for t in range(H_MAX, H_TICKS + 1):
        for name in ("sins", "s", "v", "pools"):
            assert on[name][t].tobytes() == on[name][t % H_MAX].tobytes(), f"set {t}: {name} is not that of set {t % H_MAX}"
    for k in range(tf.A_N):
        assert off["sins"][H_MAX][k].tobytes() == off["sins"][0][k].tobytes()                  # (the ego itself is put back on its start record ...)
        assert off["s"][H_MAX][k] != off["s"][0][k]                                              # (... its vehicle is not ...)
        assert any(off["sins"][H_MAX + j][k].tobytes() != off["sins"][j][k].tobytes() for j in range(1, H_MAX)), f"ego {k} repeats without the reset"


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_kat_on_the_device(dm, variant):
    """The known answers above on k_reset_traffic behind k_respawn_egos / k_respawn_spawn and k_move_traffic / k_follow_traffic, each step also
    held against the model byte for byte: the ego's records, both stats, s, v, every slice, the counters and the motion pool."""
    for kat in KATS:
        kat(dm, _Tr(dm, _runner("device"), *variant))


@gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_kat_batches(dm, variant):
    """Every known answer as distinct scenes of one launch, in batches of 5 and of 9 scenes with restarting scenes first, last and on either
    side of the respawn kernels' block edge 4 | 5: the device against the model on the batch, and every scene the bytes it gave alone."""
    ran = etb.batched(_kat_log(dm, variant))
    print(f"batches (size, restarting scenes): {ran}")
    _check_batches(ran)


def _edge_case(dm, total, follow, motion):
    """Scenes with 3, 1 and 0 actors in turn until `total` actors are placed; the 3 sit on two tracks (two on the closed triangle, one
    reversing on an open track).  The scenes that own actors 0, 255, 256 (the last of a block and the first of the next) and the last
    actor, and every 7th scene, restart on every advance ("once"); the others go on.  Two advances."""
    tr = _Tr(dm, None, follow, motion, False)
    kinds, rows_of, owner, a = [], [], [], 0
    while a < total or len(kinds) % 3 != 0:
        cnt = min((3, 1, 0)[len(kinds) % 3], total - a)
        rows_of.append([(1.0, 10.0, 0, 1, 0.5), (6.0, 10.0, 0, 2, 0.5), (5.0, -10.0, 1, 3, 0.5)][:cnt])
        owner += [len(kinds)] * cnt
        kinds.append("go")
        a += cnt
    for k in {0, 255, 256, total - 1}:
        if k < total:
            kinds[owner[k]] = "once"
    for s in range(6, len(kinds), 7):
        kinds[s] = "once"
    polylines = _closed(dm) + [(ts.polyline(dm, [(0.0, 0.0), (10.0, 0.0)]), False)]
    cases = []
    for kind, rows in zip(kinds, rows_of):
        c = tr.case(kind, polylines, rows)
        c.steps = c.steps[:2]
        cases.append(c)
    big, first, _ = etb.batch_of(cases)
    assert len(big.rows) == total
    return big, kinds, owner


@gpu
@pytest.mark.parametrize("follow,motion", [(False, False), (True, True)], ids=["plain", "follow-motion"])
@pytest.mark.parametrize("total", [1, 255, 256, 257, 513])
def test_thread_per_actor_edges(dm, total, follow, motion):
    """1, 255, 256, 257 and 513 actors in scenes of 0, 1 and 3, the restarting scenes' actors first and last of a 256-thread block: the
    device gives the model's bytes, and every actor of a scene that goes on has the s, v, pool entry and counter of the same launch
    without the reset."""
    case, kinds, owner = _edge_case(dm, total, follow, motion)
    got, want, plain = etb.DeviceBackend().run(case), etb.ModelBackend().run(case), etb.DeviceBackend().run(case.without_reset())
    W = case.laid_out()[2]
    on = np.array([kinds[s] == "once" for s in owner])
    entry = np.array([owner[a] * W + case.rows[a][3] for a in range(total)])
    assert on.any() and (total == 1 or (~on).any())
    for t, (r, w, p) in enumerate(zip(got, want, plain)):
        etb.compare(r, w, f"{total} actors, step {t}")
        assert r.resets.tolist() == ((t + 1) * on).tolist()
        assert r.s[~on].tobytes() == p.s[~on].tobytes() and r.pool[entry[~on]].tobytes() == p.pool[entry[~on]].tobytes()
        assert r.v is None or r.v[~on].tobytes() == p.v[~on].tobytes()
        assert r.mot is None or r.mot[entry[~on]].tobytes() == p.mot[entry[~on]].tobytes()
        assert (r.s[on] != p.s[on]).all()                       # (a reset actor stands on its start state, not one step on)


_INT = te._INT_FIELDS
_RUNS = {}


def _contact_planner(dm, r, reset=True):
    pl = tes._planner(dm, r)
    if reset:
        pl.set_episode_traffic(1)
    return pl


def _slices(pl, n):
    return np.concatenate([pl.get_obstacles(s) for s in range(n)])


def _device_loop(dm, key, make, ticks, n, speed):
    """`ticks` x (tick, advance) with read-backs in between on the planner `make()` gives."""
    if key in _RUNS:
        return _RUNS[key]
    pl = make()
    model, trace = dm.default_ego_model(), dm.pinned_empty(n, dm.EgoTrace)
    run = dict(sins=[pl.get_scene_in()], flags=[np.zeros(n, np.int32)], s=[pl.traffic_state()], v=[pl.traffic_speed() if speed else None], pools=[_slices(pl, n)], trace=[])
    for t in range(ticks):
        pl.tick()
        pl.advance_async(model, trace)
        run["sins"].append(pl.get_scene_in()), run["flags"].append(pl.ego_flags()), run["s"].append(pl.traffic_state())
        run["v"].append(pl.traffic_speed() if speed else None), run["pools"].append(_slices(pl, n))
        pl.sync()
        run["trace"].append(np.array(trace))
    pl.tick()
    pl.sync()
    run["last"] = _last(pl, speed)
    pl.close()
    _RUNS[key] = run
    return run


def _last(pl, speed):
    return dict(PlanOut=pl.get_plan(), SceneState=pl.get_state(), flags=pl.ego_flags(), SceneIn=pl.get_scene_in(), EpisodeStats=pl.episode_stats(),
                s=pl.traffic_state(), v=pl.traffic_speed() if speed else np.zeros(0), resets=pl.episode_traffic_resets())


def _agree(d, r, ticks, speed):
    """tests/test_episode_spawn.py::test_followers_agree_with_the_cpu_loop, and the traffic: flag words, staged records but for the advanced
    heading, integer stats; s, v and every slice byte for byte."""
    for t in range(ticks + 1):
        assert np.array_equal(d["flags"][t], r["flags"][t]), f"set {t}: flags"
        te._assert_records(d["sins"][t], r["sins"][t], f"set {t}")
        assert d["s"][t].tobytes() == r["s"][t].tobytes(), f"set {t}: s, largest difference {np.abs(d['s'][t] - r['s'][t]).max()!r}"
        assert not speed or d["v"][t].tobytes() == r["v"][t].tobytes(), f"set {t}: v"
        assert d["pools"][t].tobytes() == r["pools"][t].tobytes(), f"set {t}: slices"
    for name in _INT:
        assert np.array_equal(d["last"]["EpisodeStats"][name], r["stats"][name]), name
    assert d["last"]["resets"].tolist() == r["resets"].tolist()


@gpu
def test_contact_loop_agrees_with_the_cpu_loop(dm, oracle):
    r = _contact_loop(dm, oracle)
    d = _device_loop(dm, "contact", lambda: _contact_planner(dm, r), tes.L_TICKS, tt.F_N, False)
    _agree(d, r, tes.L_TICKS, False)
    got = d["last"]["EpisodeStats"]
    print("episodes", got["n_episodes"].tolist(), "ages", got["min_age"].tolist(), got["max_age"].tolist())
    assert got["n_episodes"].tolist() == C_EPISODES and got["min_age"].tolist() == C_AGES and got["max_age"].tolist() == C_AGES


def _chased_planner(dm, r, reset=True):
    pl = tf._planner(dm, r["cfg"], r["m"], r["sc"], 1)
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    pl.set_traffic_follow(dm.default_traffic_follow())
    pl.set_episodes(r["em"])
    if reset:
        pl.set_episode_traffic(1)
    return pl


@gpu
def test_chased_loop_agrees_with_the_cpu_loop(dm, oracle):
    r = _chased_loop(dm, oracle, True)
    d = _device_loop(dm, "chased", lambda: _chased_planner(dm, r), H_TICKS, tf.A_N, True)
    _agree(d, r, H_TICKS, True)
    for t in range(H_MAX, H_TICKS + 1):                         # the device repeats its own first episode too, every byte (the heading included)
        for name in ("sins", "s", "v", "pools"):
            assert d[name][t].tobytes() == d[name][t % H_MAX].tobytes(), f"set {t}: {name}"


@gpu
@pytest.mark.parametrize("loop", ["contact", "chased"])
def test_rollout_with_the_reset_equals_its_parts(dm, oracle, loop):
    """pp_rollout(K) = K x (advance, tick) with read-backs in between, bit for bit, the traffic and the counters included."""
    if loop == "contact":
        r = _contact_loop(dm, oracle)
        d, pl, K, speed = _device_loop(dm, "contact", lambda: _contact_planner(dm, r), tes.L_TICKS, tt.F_N, False), _contact_planner(dm, r), tes.L_TICKS, False
    else:
        r = _chased_loop(dm, oracle, True)
        d, pl, K, speed = _device_loop(dm, "chased", lambda: _chased_planner(dm, r), H_TICKS, tf.A_N, True), _chased_planner(dm, r), H_TICKS, True
    last, trace = pl.rollout(K, trace=True)
    pl.sync()
    got = _last(pl, speed)
    pl.close()
    assert last == K + 1
    for name, a in got.items():
        assert a.tobytes() == d["last"][name].tobytes(), name
    trace = np.array(trace)
    for t in range(K):
        assert trace[t].tobytes() == d["trace"][t].tobytes(), f"trace row {t}"
    assert got["resets"].sum() == got["EpisodeStats"]["n_episodes"].sum() > 0


def _record(pl, K, speed=False):
    _, trace = pl.rollout(K, trace=True)
    pl.sync()
    return dict(PlanOut=pl.get_plan(), SceneState=pl.get_state(), flags=pl.ego_flags(), SceneIn=pl.get_scene_in(), EpisodeStats=pl.episode_stats(),
                s=pl.traffic_state(), v=pl.traffic_speed() if speed else np.zeros(0), pool=_slices(pl, pl.n), trace=np.array(trace))


def _same(a, b):
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


@gpu
def test_off_means_off(dm, oracle):
    """While no episode ends, the run with the call is the run without it, byte for byte; and after n_sets = 0 the vehicles carry on as in §4k -
    the bytes of a handle that never made the call -, the counters readable and untouched."""
    r = _contact_loop(dm, oracle)
    K = min(C_AGES) - 2                                          # (no ego has touched its vehicle yet)
    with_, without = _contact_planner(dm, r), _contact_planner(dm, r, reset=False)
    a, b = _record(with_, K), _record(without, K)
    _same(a, b)
    assert not a["EpisodeStats"]["n_episodes"].any() and not with_.episode_traffic_resets().any()
    with pytest.raises(dm.PlannerError, match="error -4:"):      # a handle that never made the call has no counters
        without.episode_traffic_resets()
    with_.set_episode_traffic(0)
    a, b = _record(with_, 60), _record(without, 60)
    _same(a, b)
    assert (a["EpisodeStats"]["min_age"] == 1).all()            # (the egos restart into their vehicles again)
    assert not with_.episode_traffic_resets().any()
    with_.close(), without.close()


@gpu
def test_refusals_leave_the_model_in_force_untouched(dm, oracle):
    """Every refusal of §4m's table, on a handle with a reset in force (M = 3, n_sets = 3): the run goes on like the reference run."""
    r = _contact_loop(dm, oracle)
    n = tt.F_N
    sp = tes._sp(dm, n_starts=3, order=1, contact=1)
    starts = (np.concatenate([r["sc"]["scene_in"]] * 2), np.concatenate([r["sc"]["state"]] * 2))
    sets = _starts(dm, 2 * n)
    sets["s"], sets["v"] = np.concatenate([r["act"]["s0"] + 5.0, r["act"]["s0"] - 5.0]), 0.0

    def fresh():
        p = _contact_planner(dm, r, reset=False)
        p.set_episode_spawn(sp, *starts)
        p.set_episode_traffic(3, sets)
        p.rollout(50)                                            # (every ego has met its vehicle once)
        return p
    pl, ref = fresh(), fresh()
    assert pl.episode_traffic_resets().all()
    for n_sets, st in ((-1, None), (2, sets[:n]), (4, np.concatenate([sets, sets[:n]])), (16, None), (3, None)):          # neither 1 nor M; NULL with n_sets > 1
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_episode_traffic(n_sets, st)
    for field, bad in (("s", np.nan), ("s", np.inf), ("s", -np.inf), ("v", np.nan), ("v", np.inf), ("v", -1.0), ("v", -1e-300)):
        b = sets.copy()
        b[field][2 * n - 1] = bad
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_episode_traffic(3, b)
    pl.advance_async()
    ref.advance_async()
    for n_sets, st in ((3, sets), (1, None), (0, None)):        # PP_ERR_STATE: an update is staged
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.set_episode_traffic(n_sets, st)
    for p in (pl, ref):
        p.tick()
    a, b = _record(pl, 40), _record(ref, 40)
    _same(a, b)
    assert pl.episode_traffic_resets().tobytes() == ref.episode_traffic_resets().tobytes() and (pl.episode_spawn_stats()["n_used"][:, 1] > 0).all()
    pl.close(), ref.close()
    # PP_ERR_STATE on a handle that lacks a precondition: no traffic, world traffic, episodes off
    base = tt._planner(dm, r["cfg"], r["m"], r["sc"], 1)
    base.set_route(r["legs"], r["rf"])
    base.set_episodes(r["em"])
    with pytest.raises(dm.PlannerError, match="error -4:"):      # no traffic
        base.set_episode_traffic(1)
    fleet = dm.default_fleet_model()
    fleet["max_peers"] = 0
    base.set_fleet(np.arange(n + 1, dtype=np.int32), fleet)
    base.set_world_traffic(r["tracks"], r["pts"], r["act"])
    base.set_episodes(r["em"])
    with pytest.raises(dm.PlannerError, match="error -4:"):      # world traffic: a reset has no owner
        base.set_episode_traffic(1)
    base.set_traffic(r["tracks"], r["pts"], r["act"])
    base.set_episodes(off=True)
    with pytest.raises(dm.PlannerError, match="error -4:"):      # episodes off
        base.set_episode_traffic(1)
    with pytest.raises(dm.PlannerError, match="error -4:"):      # ... and none of these left counters behind
        base.episode_traffic_resets()
    base.set_episodes(r["em"])
    with pytest.raises(dm.PlannerError, match="error -1:"):      # without a spawn model only 1 is legal
        base.set_episode_traffic(2, sets[:n])
    base.set_episode_traffic(1)
    base.close()


@gpu
def test_every_switch_off_site_and_the_getter(dm, oracle):
    """Every successful pp_set_traffic / pp_set_world_traffic / pp_set_traffic_follow / pp_set_episodes / pp_set_episode_spawn - NULL included -
    and pp_set_egos switch the reset off: no actor is reset in the advances behind it, and the counters stay readable."""
    r = dict(_contact_loop(dm, oracle), em=te._em(dm, 31, 20))
    n, K = tt.F_N, 45                                            # (a timeout of 20 advances: wherever the vehicles stand, every ego restarts at least twice within K)
    sp = tes._sp(dm, contact=1)
    fleet = dm.default_fleet_model()
    fleet["max_peers"] = 0

    def after(site):
        """A handle with the reset in force and resets counted, the site called on it, and the pieces the site took away put back."""
        pl = tt._planner(dm, r["cfg"], r["m"], r["sc"], 1)
        pl.set_route(r["legs"], r["rf"])
        pl.set_fleet(np.arange(n + 1, dtype=np.int32), fleet)    # (worlds of one scene, no peer slots: what pp_set_world_traffic needs)
        pl.set_traffic(r["tracks"], r["pts"], r["act"])
        pl.set_episodes(r["em"])
        pl.set_episode_spawn(sp)
        pl.set_episode_traffic(1)
        pl.rollout(K)
        before = pl.episode_traffic_resets()
        assert before.all()
        site(pl)
        return pl, before

    def again(pl, traffic=True, episodes=True, spawn=True):
        if traffic:
            pl.set_traffic(r["tracks"], r["pts"], r["act"])
        if episodes:
            pl.set_episodes(r["em"])
        if spawn:
            pl.set_episode_spawn(sp)

    def egos(pl):
        pl.set_egos(r["sc"], with_motion=False)
        pl.set_state(r["sc"]["state"])
        pl.set_route(r["legs"], r["rf"])
        again(pl)

    sites = dict(set_traffic=lambda pl: pl.set_traffic(r["tracks"], r["pts"], r["act"]),
                 set_traffic_off=lambda pl: (pl.set_traffic(None), again(pl, episodes=False, spawn=False)),
                 set_world_traffic=lambda pl: (pl.set_world_traffic(r["tracks"], r["pts"], r["act"]), again(pl, episodes=False, spawn=False)),
                 set_traffic_follow=lambda pl: (pl.set_traffic_follow(dm.default_traffic_follow()), pl.set_traffic_follow(None)),
                 set_traffic_follow_null=lambda pl: pl.set_traffic_follow(None),
                 set_episodes=lambda pl: (pl.set_episodes(r["em"]), again(pl, traffic=False, episodes=False)),
                 set_episodes_null=lambda pl: (pl.set_episodes(off=True), again(pl, traffic=False)),
                 set_episode_spawn=lambda pl: pl.set_episode_spawn(sp),
                 set_episode_spawn_null=lambda pl: (pl.set_episode_spawn(None), again(pl, traffic=False, episodes=False)),
                 set_egos=egos)
    for name, site in sites.items():
        pl, before = after(site)
        pl.rollout(K)
        pl.sync()
        assert pl.episode_stats()["n_episodes"].all(), name       # (the egos did restart ...)
        assert pl.episode_traffic_resets().tobytes() == before.tobytes(), f"{name}: the reset is still on"
        # the getter: n outside 0 .. n_actors is PP_ERR_ARG, 0 is accepted
        out = np.zeros(n + 1, np.int32)
        assert pl.lib.pp_get_episode_traffic_resets(pl.h, out.ctypes.data, n + 1) == -1 and pl.lib.pp_get_episode_traffic_resets(pl.h, out.ctypes.data, -1) == -1
        assert pl.lib.pp_get_episode_traffic_resets(pl.h, out.ctypes.data, 0) == 0 and pl.lib.pp_get_episode_traffic_resets(pl.h, out.ctypes.data, 3) == 0
        assert out[:3].tolist() == before[:3].tolist() and not out[3:].any()
        # ... and the call switches it on again, the counters from 0
        pl.set_episode_traffic(1)
        assert not pl.episode_traffic_resets().any()
        pl.rollout(K)
        assert pl.episode_traffic_resets().all(), name
        pl.close()
