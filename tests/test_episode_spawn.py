"""Episode spawn model (pp_set_episode_spawn): start-record pools, spawn clearance and ending on contact.

CPU: the ABI mirrors, the hash's known answers, hand-derived known answers of the numpy model (tests/episode_spawn_model.py) and
a closed loop of oracle tick + route model + traffic model + spawn model on the followers of tests/test_traffic.py with the
vehicles turned round.
GPU: the known answers on k_respawn_spawn alone and as distinct scenes of one launch (batches of 5 and 9), restore completeness
of record k on byte patterns, the world test on worlds of 1 .. 66 members, the neutral model against k_respawn_egos, the closed
loop against the CPU loop, pp_rollout against its parts, the spawn model switched off, the error paths and lifetime.

The geometry of the known answers.  The map is the one of tests/test_episodes.py: lane 2 of road 1 runs along y = 0 from x = 100
to 149.5.  Vehicle_Width is set to 2.0, so hw = 1 exactly, and every obstacle has radius 0.5 (exact as a float): an obstacle at
distance D straight beside a pose (dx = 0, dy = D, both exact) has sqrt(0·0 + D·D) = D exactly (IEEE: sqrt(x·x) = |x|), so
(D − 0.5) − 1 is exact for the D used here: D = 1.5 gives 0 - contact -, D = 3.5 gives 2.0 = the clearance - blocked."""
import numpy as np
import pytest

import episode_model as epm
import episode_spawn_backends as esb
import episode_spawn_model as esm
import map_scenes as ms
import rollout_score_model as rsm
import route_model as rmod
import test_episodes as te
import test_traffic as tt
import traffic_model as tm

gpu = pytest.mark.gpu
CONTACT = 128


@pytest.fixture()
def cfg1(dm):
    """Grid stage off, Vehicle_Width 2.0: hw = 1."""
    cfg = dm.default_config(128)
    cfg["grid_stage"], cfg["Vehicle_Width"] = 0, 2.0
    return cfg


def _sp(dm, **kw):
    sp = esb.neutral(dm.EpisodeSpawn)
    for k, v in kw.items():
        sp[k] = v
    return sp


def _obs(dm, pts, radius=0.5):
    o = np.zeros(len(pts), dm.ObPoint)
    for k, (x, y) in enumerate(pts):
        o["x"][k], o["y"][k], o["type"][k], o["radius"][k] = x, y, 3, radius
    return o


FAR = (500.0, 500.0)          # an obstacle that is near nothing


# ---------------------------------------------------------------------------------------------------------------
# CPU: ABI, hash
def test_abi_mirrors_and_default_model(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(31) == dm.EpisodeSpawn.itemsize == 32
    assert lib.pp_sizeof(32) == dm.EpisodeSpawnStats.itemsize == 80
    assert [dm.EpisodeSpawn.fields[k][1] for k in ("seed", "clearance", "n_starts", "order", "contact", "check")] == [0, 8, 16, 20, 24, 28]
    assert [dm.EpisodeSpawnStats.fields[k][1] for k in ("n_contact", "n_blocked", "n_rejected", "cur_start", "n_used")] == [0, 4, 8, 12, 16]
    sp = dm.default_episode_spawn()[0]
    assert (int(sp["seed"]), float(sp["clearance"]), int(sp["n_starts"]), int(sp["order"]), int(sp["contact"]), int(sp["check"])) == (1, 2.0, 1, 0, 1, 3)
    assert dm.EGO_CONTACT == esm.CONTACT == CONTACT and dm.EPISODE_MAX_STARTS == esm.MAX_STARTS == 16
    assert lib.pp_sizeof(29) == 8 and lib.pp_sizeof(30) == 80           # (the records of §4k are as they were)


def test_hash_known_answers():
    assert esm.mix(0) == 0xE220A8397B1DCDAF and esm.mix(1) == 0x910A2DEC89025CC1
    for (seed, s, e), u, ks in (((1, 0, 1), 0x86D6FD953217AE03, (0, 1, 1, 8)), (((1 << 64) - 1, 5, 2), 0xC7EB916392985897, (0, 1, 2, 12)),
                                ((2026, 1023, 100), 0xA0DF773B063C2D69, (0, 1, 1, 10))):
        assert esm.hash_u(seed, s, e) == u
        assert tuple(esm.first_choice(seed, s, e, M, 0) for M in (1, 2, 3, 16)) == ks
    assert [esm.first_choice(9, 4, e, 3, 1) for e in (1, 2, 3, 4)] == [1, 2, 0, 1]          # round robin: e mod M


def test_hash_draws_every_start_record():
    for M in (2, 3, 4, 16):
        for s in range(8):
            assert {esm.first_choice(1, s, e, M, 0) for e in range(1, 4 * M + 1)} == set(range(M)), (M, s)


# ---------------------------------------------------------------------------------------------------------------
# the known answers, written once against a Runner of tests/episode_spawn_backends.py
class _Sp:
    """Advances of one scene: the ego of tests/test_episodes.py on lane 2 (y = 0), one straight path per step."""
    def __init__(self, dm, runner):
        self.dm, self.run, self.name = dm, runner, runner.name

    def __call__(self, cfg, si, pos, em, sp, obs=None, starts=None, legs=None, sts=None, score=False, state0=None):
        dm = self.dm
        route = None if legs is None else (legs, np.array([0, len(legs)], np.int32), dm.default_route_model())
        sts = [np.zeros(1, dm.SceneState) for _ in pos] if sts is None else sts
        obs = np.zeros(0, dm.ObPoint) if obs is None else obs
        return self.run(esb.Case(cfg, dm.default_ego_model(), em, sp, si, [obs], te._state0(dm) if state0 is None else state0, list(zip(pos, sts)),
                                 te._world(dm), route, starts, None, score))


def _runner(name, log=None):
    return esb.Runner(esb.ModelBackend() if name == "model" else esb.DeviceBackend(), log)


def _sstats(r, k=0):
    e = r.sstats[k]
    used = e["n_used"].tolist()
    return dict(contact=int(e["n_contact"]), blocked=int(e["n_blocked"]), rejected=int(e["n_rejected"]), cur=int(e["cur_start"]),
                used={i: u for i, u in enumerate(used) if u})


S0 = dict(contact=0, blocked=0, rejected=0, cur=0, used={})
UP = float(np.nextafter(1.5, 2.0))           # the next double above 1.5


def _kat_contact_scan_on_its_stride_edges(dm, cfg1, sp_):
    # the ego reads (110, 0); the touching obstacle stands at (110, 1.5): d − hw = (1.5 − 0.5) − 1 = 0 -> contact, whatever its index and
    # however many entries the lanes stride (one pass of 64, two, three); every other entry is far away.  One advance: cause 128 alone.
    si, po, em = te._ego(dm, 110.0, ego_id=20), te._path(dm, 110.0), te._em(dm)
    for n, at in ((1, 0), (63, 0), (63, 62), (64, 63), (65, 63), (65, 64), (128, 64), (128, 127), (129, 0), (129, 63), (129, 64), (129, 128)):
        pts = [FAR] * n
        pts[at] = (110.0, 1.5)
        (r,) = sp_(cfg1, si, [po], em, _sp(dm, contact=1), _obs(dm, pts))
        _is_record(dm, r, 0, si, None, f"n {n} at {at}", n)
        assert (int(r.flags[0]), int(r.trace["flags"][0]), int(r.out["obs_n"][0])) == (0, CONTACT | 32, n)
        assert te._stats(r) == dict(n=1, age=0, n_end=[0] * 6, cause=CONTACT, last_age=1, ages=(1, 1), ticks=1, dist=0.0, last_dist=1.0, total=1.0), (n, at)
        assert _sstats(r) == dict(S0, contact=1, used={0: 1}), (n, at)
        # the same obstacle one ulp further away: d − hw is the next double above 0 -> no contact, the ego drives on to 111
        pts[at] = (110.0, UP)
        (r,) = sp_(cfg1, si, [po], em, _sp(dm, contact=1), _obs(dm, pts))
        assert (float(r.out["loc"]["globalpoint"]["x"][0]), int(r.flags[0]), int(r.trace["flags"][0])) == (111.0, 0, 0), (n, at)
        assert te._stats(r) == dict(te.NONE, age=1, dist=1.0) and _sstats(r) == S0, (n, at)
    # no obstacle at all: nothing to touch
    (r,) = sp_(cfg1, si, [po], em, _sp(dm, contact=1))
    assert te._stats(r) == dict(te.NONE, age=1, dist=1.0) and _sstats(r) == S0


def _kat_contact_ignores_nan_and_infinity(dm, cfg1, sp_):
    # NaN and infinite coordinates give a NaN or infinite d_j: compared false, ignored - also when they stand in front of, between and
    # behind a touching entry, which still ends the episode
    si, po, em = te._ego(dm, 110.0, ego_id=20), te._path(dm, 110.0), te._em(dm)
    odd = [(np.nan, 0.0), (110.0, np.nan), (np.inf, 0.0), (110.0, -np.inf), (np.inf, np.inf), (np.nan, np.inf)]
    (r,) = sp_(cfg1, si, [po], em, _sp(dm, contact=1), _obs(dm, odd * 11))          # 66 entries: two passes
    assert te._stats(r) == dict(te.NONE, age=1, dist=1.0) and _sstats(r) == S0
    (r,) = sp_(cfg1, si, [po], em, _sp(dm, contact=1), _obs(dm, odd * 11 + [(110.0, 1.5)] + odd))
    assert te._stats(r)["cause"] == CONTACT and _sstats(r) == dict(S0, contact=1, used={0: 1})


def _kat_contact_off_ends_nothing(dm, cfg1, sp_):
    # contact == 0 and the ego INSIDE an obstacle (d − hw = −1.5): nothing ends, on the advance and on the next one
    si, em = te._ego(dm, 110.0, ego_id=20), te._em(dm)
    r = sp_(cfg1, si, [te._path(dm, 110.0), te._path(dm, 111.0)], em, _sp(dm, contact=0), _obs(dm, [(110.0, 0.0), (111.0, 0.0)]))
    assert [float(q.out["loc"]["globalpoint"]["x"][0]) for q in r] == [111.0, 112.0] and [int(q.flags[0]) for q in r] == [0, 0]
    assert te._stats(r[1]) == dict(te.NONE, age=2, dist=2.0) and _sstats(r[1]) == S0


def _kat_contact_flag_and_timeout_on_one_advance(dm, cfg1, sp_):
    # the LANE_END advance of tests/test_episodes.py (lane 1, y = 3.75, 133 -> 134) with max_ticks = 1 and an obstacle 1.5 m beside the pose
    # the advance READ (133, 3.75 + 1.5 = 5.25, exact): cause 4 | 64 | 128 = 196, ONE episode, n_end counts LANE_END and TIMEOUT, n_contact 1,
    # the trace carries 4 | 32 | 64 | 128 = 228
    si = te._ego(dm, 133.0, y=3.75, lane=1, ego_id=60)
    (r,) = sp_(cfg1, si, [te._path(dm, 133.0, y=3.75)], te._em(dm, 31, 1), _sp(dm, contact=1), _obs(dm, [(133.0, 5.25)]), legs=te._legs(dm))
    assert int(r.trace["flags"][0]) == 228 and int(r.flags[0]) == 0 and float(r.out["loc"]["globalpoint"]["x"][0]) == 133.0
    assert te._stats(r) == dict(n=1, age=0, n_end=[0, 0, 1, 0, 0, 1], cause=196, last_age=1, ages=(1, 1), ticks=1, dist=0.0, last_dist=1.0, total=1.0)
    assert _sstats(r) == dict(S0, contact=1, used={0: 1})
    # contact is judged at the pose the advance READ: an obstacle 1.5 m beside the pose it WROTE (134) is 1.80 m from the read one - none
    (r,) = sp_(cfg1, si, [te._path(dm, 133.0, y=3.75)], te._em(dm, 31, 0), _sp(dm, contact=1), _obs(dm, [(134.0, 5.25)]), legs=te._legs(dm))
    assert te._stats(r)["cause"] == 4 and int(r.trace["flags"][0]) == 36 and _sstats(r) == dict(S0, used={0: 1})


def _x(k):
    """Where start record k of _starts stands on lane 2 (record 0: the ego of the known answers at 110)."""
    return 110.0 if k == 0 else 100.0 + 2.0 * k


def _starts(dm, M, x0=100.0, dx=2.0, y=0.0):
    """Start records 1 .. M − 1 on lane 2: record k at (x0 + dx k, y), id of its lane point, and fields only record k carries."""
    si, st = [], []
    for k in range(1, M):
        x = x0 + dx * k
        r = te._ego(dm, x, y=y, ego_id=int(round((x - 100.0) / 0.5)))
        r["period_last"], r["goal"]["x"], r["goal"]["y"], r["dec"]["velocity_expect"], r["loc"]["globalpoint"]["dir"] = 100.0 + k, float(k), -float(k), 3.0 * k, 10.0 + k
        s = te._state0(dm)
        s["tick"], s["path_lat_dis"], s["brakespeed"] = 7 + 10 * k, 0.25 * k, 1.0 + k
        si.append(r), st.append(s)
    return (np.concatenate(si), np.concatenate(st)) if M > 1 else None


def _is_record(dm, r, k, si0, starts, what="", n_obs=0):
    """Step r put the scene on start record k: every byte of SceneIn and SceneState; obs_off / obs_n are those of record 0 - the one
    scene of the call owns the pool from entry 0 on and has n_obs obstacles."""
    want_in, want_st = (si0, te._state0(dm)) if k == 0 else (starts[0][k - 1:k].copy(), starts[1][k - 1:k])
    want_in = ms.resolve(dm, te._world(dm)["map"], want_in)
    want_in["obs_off"], want_in["obs_n"] = 0, n_obs
    assert r.out.tobytes() == want_in.tobytes() and r.state.tobytes() == want_st.tobytes(), (what, k)
    assert int(r.sstats["cur_start"][0]) == k, (what, k)


def _kat_round_robin(dm, cfg1, sp_):
    # max_ticks = 1: every advance ends an episode (TIMEOUT alone); order 1: the e-th ended episode restarts on record e mod M, so M + 1
    # restarts visit 1, 2, .., M − 1, 0, 1.  contact 0, check 0: nothing else plays a part.
    si, em = te._ego(dm, 110.0, ego_id=20), te._em(dm, 31, 1)
    for M in (1, 2, 16):
        starts = _starts(dm, M)
        pos = [te._path(dm, 110.0)] + [te._path(dm, _x(t % M)) for t in range(1, M + 1)]          # (every path starts where the ego of that advance stands)
        r = sp_(cfg1, si, pos, em, _sp(dm, n_starts=M, order=1), _obs(dm, [FAR, FAR]), starts)
        used = {}
        for t, q in enumerate(r):
            k = (t + 1) % M
            used[k] = used.get(k, 0) + 1
            _is_record(dm, q, k, si, starts, f"M {M} restart {t}", 2)
            assert int(q.out["obs_n"][0]) == 2 and int(q.trace["flags"][0]) == 96 and _sstats(q) == dict(S0, cur=k, used=used), (M, t)
        assert sorted(used) == list(range(M))


def _kat_round_robin_on_the_record_that_ends_at_once(dm, cfg1, sp_):
    # _kat_a_start_record_that_ends_at_once of tests/test_episodes.py: the start record sits one step in front of its lane end.  Here all M
    # records do (133, 3.75), told apart by the fields only they carry: every advance ends one episode with LANE_END alone (no timeout) and
    # restarts round robin: M + 1 consecutive restarts visit 1, 2, .., M − 1, 0, 1
    si, po = te._ego(dm, 133.0, y=3.75, lane=1, ego_id=60), te._path(dm, 133.0, y=3.75)
    for M in (1, 2, 3, 16):
        ins, sts = [], []
        for k in range(1, M):
            r = si.copy()
            r["period_last"], r["goal"]["x"] = 100.0 + k, float(k)
            s = te._state0(dm)
            s["tick"] = 7 + 10 * k
            ins.append(r), sts.append(s)
        starts = (np.concatenate(ins), np.concatenate(sts)) if M > 1 else None
        r = sp_(cfg1, si, [po] * (M + 1), te._em(dm), _sp(dm, n_starts=M, order=1), None, starts, legs=te._legs(dm))
        used = {}
        for t, q in enumerate(r):
            k = (t + 1) % M
            used[k] = used.get(k, 0) + 1
            _is_record(dm, q, k, si, starts, f"M {M} restart {t}")
            assert int(q.trace["flags"][0]) == 36 and te._stats(q)["n_end"] == [0, 0, t + 1, 0, 0, 0] and te._stats(q)["cause"] == 4, (M, t)
            assert _sstats(q) == dict(S0, cur=k, used=used), (M, t)
        assert sorted(used) == list(range(M))


def _kat_hashed_order(dm, cfg1, sp_):
    # order 0, scene 0: restart e goes to ((u >> 32) M) >> 32 with u = mix(mix(seed + 0) + e).  Seed 1, e = 1: u = 0x86D6FD953217AE03, the known
    # answer of §4l -> record 1 of 2 and 3, record 8 of 16; the later restarts are asked of first_choice, which has the known answers
    si, em = te._ego(dm, 110.0, ego_id=20), te._em(dm, 31, 1)
    for seed, M in ((1, 2), (1, 3), (1, 16), (2026, 16), ((1 << 64) - 1, 3)):
        starts = _starts(dm, M)
        ks = [esm.first_choice(seed, 0, e, M, 0) for e in range(1, 6)]
        r = sp_(cfg1, si, [te._path(dm, 110.0)] + [te._path(dm, _x(k)) for k in ks[:4]], em, _sp(dm, seed=seed, n_starts=M, order=0), None, starts)
        if seed == 1:
            assert ks[0] == {2: 1, 3: 1, 16: 8}[M]
        for t, q in enumerate(r):
            _is_record(dm, q, ks[t], si, starts, f"seed {seed} M {M} restart {t}")
        assert _sstats(r[-1])["used"] == {k: ks.count(k) for k in set(ks)}


def _kat_clearance_threshold(dm, cfg1, sp_):
    # M = 3, round robin, first restart: k0 = 1, record 1 at (102.0, 0).  clearance 2: a blocker at (102.0, 3.5) gives (3.5 − 0.5) − 1 = 2.0 ≤ 2 ->
    # blocked, the choice moves on to record 2 (104, 0) and n_rejected = 1; one ulp further away -> clear, record 1.  The blocker sits at slice
    # index 0, 63, 64 and last of 129; NaN entries in the slice block nothing.
    si, em, M = te._ego(dm, 110.0, ego_id=20), te._em(dm, 31, 1), 3
    starts = _starts(dm, M)
    up = float(np.nextafter(3.5, 4.0))
    for n, at in ((1, 0), (64, 63), (65, 64), (129, 63), (129, 64), (129, 128)):
        for y, k, rej in ((3.5, 2, 1), (up, 1, 0)):
            pts = [FAR if j % 2 else (np.nan, 0.0) for j in range(n)]
            pts[at] = (102.0, y)
            (r,) = sp_(cfg1, si, [te._path(dm, 110.0)], em, _sp(dm, n_starts=M, order=1, clearance=2.0, check=1), _obs(dm, pts), starts)
            _is_record(dm, r, k, si, starts, f"n {n} at {at} y {y!r}", n)
            assert _sstats(r) == dict(S0, rejected=rej, cur=k, used={k: 1}) and int(r.out["obs_n"][0]) == n, (n, at, y)
    # check == 0: the blocked candidate is taken
    (r,) = sp_(cfg1, si, [te._path(dm, 110.0)], em, _sp(dm, n_starts=M, order=1, clearance=2.0, check=0), _obs(dm, [(102.0, 3.5)]), starts)
    _is_record(dm, r, 1, si, starts, n_obs=1)
    assert _sstats(r) == dict(S0, cur=1, used={1: 1})
    # check == 2 (the world alone) and no fleet: the slice is not looked at and the world test is skipped
    (r,) = sp_(cfg1, si, [te._path(dm, 110.0)], em, _sp(dm, n_starts=M, order=1, clearance=2.0, check=2), _obs(dm, [(102.0, 3.5)]), starts)
    _is_record(dm, r, 1, si, starts, n_obs=1)
    assert _sstats(r) == dict(S0, cur=1, used={1: 1})


def _kat_clearance_wraps_and_gives_up(dm, cfg1, sp_):
    # M = 3, round robin, TWO restarts: the second has e = 2, k0 = 2 = M − 1, record 2 at (104, 0).  A blocker on it (104, 3.5): rejected, the
    # choice wraps to record 0 - the capture, the ego at (112, 0) -, which is clear.  Record 1 (102, 0) is clear on restart 1.
    si, em, M = te._ego(dm, 112.0, ego_id=24), te._em(dm, 31, 1), 3
    starts = _starts(dm, M)
    r = sp_(cfg1, si, [te._path(dm, 112.0), te._path(dm, 102.0)], em, _sp(dm, n_starts=M, order=1, clearance=2.0, check=3), _obs(dm, [FAR, (104.0, 3.5)]), starts)
    _is_record(dm, r[0], 1, si, starts, n_obs=2)
    _is_record(dm, r[1], 0, si, starts, n_obs=2)
    assert _sstats(r[1]) == dict(S0, rejected=1, cur=0, used={0: 1, 1: 1})
    # all three blocked (102, 104 and 112, each with a blocker 3.5 m beside it): k0 is taken all the same, n_blocked = 1, n_rejected = M
    pts = [(102.0, 3.5), (104.0, -3.5), (112.0, 3.5)]
    (r,) = sp_(cfg1, si, [te._path(dm, 112.0)], em, _sp(dm, n_starts=M, order=1, clearance=2.0, check=1), _obs(dm, pts), starts)
    _is_record(dm, r, 1, si, starts, n_obs=3)
    assert _sstats(r) == dict(S0, blocked=1, rejected=3, cur=1, used={1: 1})
    # clearance 0 on the same slice: (3.5 − 0.5) − 1 = 2 > 0, nothing is blocked
    (r,) = sp_(cfg1, si, [te._path(dm, 112.0)], em, _sp(dm, n_starts=M, order=1, clearance=0.0, check=1), _obs(dm, pts), starts)
    assert _sstats(r) == dict(S0, cur=1, used={1: 1})


def _kat_the_scorecard_follows_the_chosen_record(dm, cfg1, sp_):
    # the scorecard known answer of tests/test_episodes.py with M = 2, round robin: the second advance ends the episode (max_ticks = 2) and
    # restarts on record 1 at (102.0, 0) with velocity 36: last_pos / last_speed move THERE, so the closing tick - on record 1 - adds +0 m
    v1 = 36.0 - 4.0 * 0.1 * 3.6
    s = 0.5 * (36.0 + v1) / 3.6 * 0.1
    x1 = 110.5 + (s - 0.5) / 0.5 * (111.0 - 110.5)
    si, starts = te._ego(dm, 110.0, ego_id=20), _starts(dm, 2)
    r = sp_(cfg1, si, [te._path(dm, 110.0, desspd=30.0), te._path(dm, 111.0, desspd=30.0)], te._em(dm, 31, 2), _sp(dm, n_starts=2, order=1), None, starts, score=True)
    _is_record(dm, r[1], 1, si, starts)
    patched, after = r[1].score[0], r[1].final_score[0]
    assert (float(patched["last_pos"]["x"]), float(patched["last_pos"]["y"]), float(patched["last_speed"])) == (102.0, 0.0, 36.0)
    dec = -((v1 - 36.0) / 3.6 / 0.1)
    assert (int(patched["n_ticks"]), float(patched["dist"]), float(patched["max_acc"]), float(patched["max_dec"])) == (2, x1 - 110.0, 0.0, dec)
    assert (int(after["n_ticks"]), float(after["dist"]), float(after["max_acc"]), float(after["max_dec"]), float(after["max_speed"])) == (3, x1 - 110.0, 0.0, dec, 36.0)


KATS = [_kat_contact_scan_on_its_stride_edges, _kat_contact_ignores_nan_and_infinity, _kat_contact_off_ends_nothing, _kat_contact_flag_and_timeout_on_one_advance,
        _kat_round_robin, _kat_round_robin_on_the_record_that_ends_at_once, _kat_hashed_order, _kat_clearance_threshold, _kat_clearance_wraps_and_gives_up]


@pytest.mark.parametrize("kat", KATS + [_kat_the_scorecard_follows_the_chosen_record], ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, cfg1, kat):
    kat(dm, cfg1, _Sp(dm, _runner("model")))


# ---- the world test -------------------------------------------------------------------------------------------
WORLDS = [0, 1, 3, 67, 132, 198]          # worlds of 1, 2, 64, 65 and 66 members


def _world_case(dm, cfg1, fleet=True, check=2):
    """198 scenes, scene s at (110, 10 s), record 1 of scene s at (120, 10 s); M = 2, round robin, max_ticks = 1: the one advance restarts every
    scene, first choice record 1.  hw = 1, clearance 2: an ego that stood at distance 4 of a spawn point - (4 − 1) − 1 = 2 - blocks it.  The
    blockers are MOVED to (124, 10 v) - dx = 4 exactly, dy = 0 - for their victim v of the same world; `up` blockers stand one ulp further.
    Returns (Case, {victim: blocker}, the victims whose blocker is one ulp too far)."""
    n = WORLDS[-1]
    ego = lambda x, y: te._ego(dm, x, y=y, ego_id=int(round((x - 100.0) / 0.5)))
    pos = {s: (110.0, 10.0 * s) for s in range(n)}
    # world of 2: its second member blocks its first.  World of 64 (3 .. 66): first and last member.  World of 65 (67 .. 131): members 63 and 64
    # (the last).  World of 66 (132 .. 197): first, members 63, 64 and the last.  victim: blocker
    pairs = {1: 2, 4: 3, 5: 66, 68: 67 + 63, 69: 67 + 64, 133: 132, 134: 132 + 63, 135: 132 + 64, 136: 197}
    up = {140: 132 + 62, 70: 67 + 62}                                          # one ulp too far: clear
    for v, b in list(pairs.items()) + list(up.items()):
        pos[b] = (124.0 if v in pairs else float(np.nextafter(124.0, 200.0)), 10.0 * v)
    pos[0] = (120.0, 10.0 * 150)                                               # the lone scene of world 0 stands ON the spawn point of scene 150: another world
    si = np.concatenate([ego(*pos[s]) for s in range(n)])
    rec1 = np.concatenate([ego(120.0, 10.0 * s) for s in range(n)])
    rec1["period_last"] = 101.0
    st1 = np.concatenate([te._state0(dm)] * n)
    st1["tick"] = 17
    po = np.concatenate([te._path(dm, pos[s][0], y=pos[s][1]) for s in range(n)])
    case = esb.Case(cfg1, dm.default_ego_model(), te._em(dm, 31, 1), _sp(dm, n_starts=2, order=1, clearance=2.0, check=check), si, [np.zeros(0, dm.ObPoint)] * n,
                    np.concatenate([te._state0(dm)] * n), [(po, np.zeros(n, dm.SceneState))], te._world(dm), None, (rec1, st1), WORLDS if fleet else None)
    return case, pairs, up


def _check_worlds(dm, cfg1, run):
    case, pairs, up = _world_case(dm, cfg1)
    (r,) = run(case, log=False)
    cur = r.sstats["cur_start"]
    # a victim takes record 0 - its OWN pose of this advance, on which it stands itself: a scene does not block itself - with one rejection;
    # everybody else takes record 1: the blockers one ulp too far do not block, nor does scene 0 of another world on scene 150's spawn point
    assert np.flatnonzero(cur == 0).tolist() == sorted(pairs) and (r.sstats["n_blocked"] == 0).all()
    assert r.sstats["n_rejected"].tolist() == [int(s in pairs) for s in range(case.n)] and int(cur[150]) == 1 and all(int(cur[v]) == 1 for v in up)
    rec = case.pools(case.laid_out()[0])[0]
    for s in range(case.n):
        k = int(cur[s])
        assert r.out[s].tobytes() == rec[k][s].tobytes(), s
        assert int(r.state["tick"][s]) == (7 if k == 0 else 17), s
    # without a fleet the world test is skipped: every scene takes record 1
    case, _, _ = _world_case(dm, cfg1, fleet=False)
    (r,) = run(case, log=False)
    assert (r.sstats["cur_start"] == 1).all() and not r.sstats["n_rejected"].any()
    # check bit 1 clear: the fleet is there and nobody looks
    case, _, _ = _world_case(dm, cfg1, check=1)
    (r,) = run(case, log=False)
    assert (r.sstats["cur_start"] == 1).all() and not r.sstats["n_rejected"].any()


def test_world_test_on_the_model(dm, cfg1):
    _check_worlds(dm, cfg1, _runner("model"))


# ---- the closed loop: the followers of tests/test_traffic.py with the vehicles turned round ---------------------
L_SPEED, L_TICKS = -3.0, 120
_CPU = {}


def _loop_scene(dm):
    cfg, m, sc, legs, rf, tracks, pts, act = tt._followers(dm)
    assert tt.F_GAP == 20.0
    act = act.copy()
    act["speed"] = L_SPEED
    raw = sc["scene_in"].copy()
    raw["obs_n"] = 1
    em = te._em(dm, 31, 0)
    return dict(cfg=cfg, m=m, sc=dict(sc, scene_in=raw), legs=legs, rf=rf, tracks=tracks, pts=pts, act=act, em=em, sp=_sp(dm, contact=1))


def _cpu_loop(dm, oracle):
    """Oracle tick + route model + spawn model + traffic model, 120 advances; the scorecard model is folded beside it to find every
    ego's first scored contact.  sins[t]: the records tick t reads."""
    if _CPU:
        return _CPU
    r = _loop_scene(dm)
    cfg, m, sc, n = r["cfg"], r["m"], r["sc"], tt.F_N
    model, rm = dm.default_ego_model(), dm.default_route_model()
    dt, hw = float(model["dt"][0]), 0.5 * float(cfg["Vehicle_Width"][0])
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(n, np.int32)
    tr = tm.Traffic(r["tracks"], r["pts"], r["act"], si["obs_off"])
    obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
    pin, pst = [si.copy()], [st.copy()]
    stats, sstats, scores = epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n), rsm.new_scores(dm.RolloutScore, n)
    sins, fl_, causes, hits = [si], [flags], [], []
    for t in range(L_TICKS):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
        before = scores["n_collision_ticks"].copy()
        rsm.fold(scores, cfg, dt, si, plan, st, obs, flags)
        hits.append(scores["n_collision_ticks"] > before)
        q, f, _ = rmod.advance(dm, cfg, model, rm, r["legs"], r["rf"], m, si, plan, st, flags)
        si, st, flags, _, c = esm.step(r["em"], r["sp"], stats, sstats, pin, pst, si, q, f, st, obs, hw)
        obs, _ = tr.place(obs, None, dt)
        sins.append(si), fl_.append(flags), causes.append(c)
    _CPU.update(r, sins=sins, flags=fl_, causes=np.array(causes), hits=np.array(hits), stats=stats, sstats=sstats, state=st)
    return _CPU


def test_contact_ends_the_followers_episodes_on_the_cpu(dm, oracle):
    """Every ego ends its first episode with cause exactly DMPP_EGO_CONTACT, on the advance behind its first scored contact (tick 36 .. 46 of
    the run without episodes, which this one equals until then); no episode ends in any other way: n_contact == n_episodes > 0."""
    r = _cpu_loop(dm, oracle)
    s, ss, causes, hits = r["stats"], r["sstats"], r["causes"], r["hits"]
    first_end = [int(np.flatnonzero(causes[:, k])[0]) for k in range(tt.F_N)]
    first_hit = [int(np.flatnonzero(hits[:, k])[0]) for k in range(tt.F_N)]
    print("first contact ticks", first_hit, "\nfirst ages", [int(a) + 1 for a in first_end], "episodes", s["n_episodes"].tolist(), "ages", s["min_age"].tolist(), s["max_age"].tolist())
    assert first_hit == [36, 42, 37, 41, 37, 38, 43, 42, 38, 38, 37, 38, 42, 46, 44, 45]
    assert first_end == first_hit and all(int(causes[first_end[k], k]) == CONTACT for k in range(tt.F_N))
    assert set(causes[causes != 0].tolist()) == {CONTACT}
    assert np.array_equal(ss["n_contact"], s["n_episodes"]) and (s["n_episodes"] > 0).all() and not s["n_end"].any()
    assert not ss["n_blocked"].any() and not ss["n_rejected"].any() and not ss["cur_start"].any() and np.array_equal(ss["n_used"][:, 0], s["n_episodes"])


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("kat", KATS + [_kat_the_scorecard_follows_the_chosen_record], ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg1, kat):
    """The known answers above on k_respawn_spawn behind k_advance_egos / k_advance_route (injected PlanOut / SceneState), each step also held
    against the model on the device's own records: SceneIn, flags, trace, SceneState, EpisodeStats, EpisodeSpawnStats."""
    kat(dm, cfg1, _Sp(dm, _runner("device")))


@gpu
def test_kat_batches(dm, cfg1):
    """Every known answer once more on the device, logged, then as distinct scenes of one launch in batches of 5 and of 9 scenes with ending
    scenes first, last and on either side of the block edge 4 | 5, against the model on the same batch and - where the start choice does
    not depend on the scene index - against the bytes each scene gave alone."""
    log = []
    sp_ = _Sp(dm, _runner("device", log))
    for kat in KATS:
        kat(dm, cfg1, sp_)
    ran = esb.batched(log)
    print(f"{len(log)} calls; batches (size, ending scenes): {ran}")
    assert {n for n, _ in ran} == {5, 9}
    for size in (5, 9):
        assert any({0, 3, 4, size - 1} <= set(e) and len(e) < size for n, e in ran if n == size)


@gpu
def test_world_test_on_the_device(dm, cfg1):
    _check_worlds(dm, cfg1, _runner("device"))


@gpu
def test_restore_brings_every_byte_of_record_k_back(dm, cfg1):
    """test_restore_brings_every_byte_back of tests/test_episodes.py with a pool of three: 9 scenes, records 1 and 2 of every scene are byte
    patterns (SceneState from its first byte to its last; SceneIn in every byte an advance carries over and the set call does not derive).
    Scenes 0, 3, 4 and 8 end; the hashed choice sends them to records 1 and 2 (a seed is searched for which none of them draws record 0 and
    both others are drawn): they get every byte of THAT record back, obs_off / obs_n of record 0.  The others keep what the advance wrote."""
    n, M, m = 9, 3, te._world(dm)["map"]
    ending = [0, 3, 4, 8]
    seed = next(sd for sd in range(1, 100) if {esm.first_choice(sd, s, 1, M, 0) for s in ending} == {1, 2})
    si = np.concatenate([te._ego(dm, 133.0, y=3.75, lane=1, ego_id=60) if k in ending else te._ego(dm, 110.0 + k, ego_id=20) for k in range(n)])
    po = np.concatenate([te._path(dm, 133.0, y=3.75) if k in ending else te._path(dm, 110.0 + k) for k in range(n)])
    cap = te._pattern(dm.SceneIn, (M - 1) * n, 5)
    for name in ("pos", "road_num", "lane_num", "path_num", "last_roadnum", "next_roadnum", "last_lanenum", "next_lanenum"):
        cap["loc"][name] = np.tile(si["loc"][name], M - 1)
    cap["loc"]["id"][:, :2] = np.tile(si["loc"]["id"][:, :2], (M - 1, 1))
    cap_st = te._pattern(dm.SceneState, (M - 1) * n, 11)
    legs = np.concatenate([te._legs(dm)] * n)
    route = (legs, np.arange(0, 2 * n + 1, 2, dtype=np.int32), dm.default_route_model())
    case = esb.Case(cfg1, dm.default_ego_model(), te._em(dm), _sp(dm, seed=seed, n_starts=M, order=0), si, [_obs(dm, [FAR])] * n,
                    np.concatenate([te._state0(dm)] * n), [(po, np.zeros(n, dm.SceneState))], te._world(dm), route, (cap, cap_st))
    (r,) = _runner("device")(case, log=False)
    start = ms.resolve(dm, m, cap)
    start["obs_off"], start["obs_n"] = np.tile(r.out["obs_off"], M - 1), 1
    assert np.flatnonzero(r.stats["n_episodes"]).tolist() == ending and r.flags.tolist() == [0] * n
    got = set()
    for s in range(n):
        if s in ending:
            k = esm.first_choice(seed, s, 1, M, 0)
            got.add(k)
            assert r.out[s].tobytes() == start[(k - 1) * n + s].tobytes() and r.state[s].tobytes() == cap_st[(k - 1) * n + s].tobytes(), (s, k)
            assert int(r.sstats["cur_start"][s]) == k and r.sstats["n_used"][s].tolist() == [int(j == k) for j in range(16)]
        else:
            assert not r.state[s].tobytes().strip(b"\0") and float(r.out["loc"]["globalpoint"]["x"][s]) == 111.0 + s and not r.sstats[s].tobytes().strip(b"\0"), s
    assert got == {1, 2}


class _Both:
    """A known answer of tests/test_episodes.py on k_respawn_egos and on k_respawn_spawn with the neutral model: the same bytes."""
    name = "device"

    def __init__(self, dm):
        self.dm = dm

    def __call__(self, cfg, si, pos, em, legs=None, sts=None, score=False):
        dm, out = self.dm, []
        for sp in (None, esb.neutral(dm.EpisodeSpawn)):
            run = _Sp(dm, _runner("device"))
            out.append(run(cfg, si, pos, em, sp, None, None, legs, sts, score))
        for t, (a, b) in enumerate(zip(*out)):
            for name in ("out", "flags", "trace", "state", "stats") + (("score",) if score else ()):
                assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (t, name)
            assert not b.sstats["n_contact"].any() and not b.sstats["n_rejected"].any() and int(b.sstats["n_used"][0, 0]) == int(b.stats["n_episodes"][0])
        if score:
            assert out[0][-1].final_score.tobytes() == out[1][-1].final_score.tobytes()
        return out[1]


@gpu
@pytest.mark.parametrize("kat", [k for k in te.KATS if k is not te._kat_a_nan_position] + [te._kat_a_nan_position, te._kat_the_scorecard_does_not_see_the_jump], ids=lambda f: f.__name__[5:])
def test_neutral_model_gives_the_bytes_of_k_respawn_egos(dm, kat):
    cfg0 = dm.default_config(128)
    cfg0["grid_stage"] = 0
    kat(dm, cfg0, _Both(dm))


def _planner(dm, r, spawn=True):
    pl = tt._planner(dm, r["cfg"], r["m"], r["sc"], 1)
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    pl.set_episodes(r["em"])
    if spawn:
        pl.set_episode_spawn(r["sp"])
    return pl


_RUNS = {}
_SP_INT = ("n_contact", "n_blocked", "n_rejected", "cur_start", "n_used")


def _device_loop(dm, oracle):
    if "loop" in _RUNS:
        return _RUNS["loop"]
    r = _cpu_loop(dm, oracle)
    pl = _planner(dm, r)
    n, model = tt.F_N, dm.default_ego_model()
    trace = dm.pinned_empty(n, dm.EgoTrace)
    run = dict(sins=[pl.get_scene_in()], flags=[np.zeros(n, np.int32)], trace=[])
    for t in range(L_TICKS):
        pl.tick()
        pl.advance_async(model, trace)
        run["sins"].append(pl.get_scene_in()), run["flags"].append(pl.ego_flags())
        pl.sync()
        run["trace"].append(np.array(trace))
    pl.tick()
    pl.sync()
    run["last"] = (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), pl.episode_stats(), pl.episode_spawn_stats(), pl.traffic_state())
    pl.close()
    _RUNS["loop"] = run
    return run


@gpu
def test_followers_agree_with_the_cpu_loop(dm, oracle):
    """120 advances of the followers on the device: every staged record against the CPU loop - every byte but the heading -, equal flag words
    and the stats of §4k and §4l equal in every integer field."""
    r, d = _cpu_loop(dm, oracle), _device_loop(dm, oracle)
    for t in range(L_TICKS + 1):
        assert np.array_equal(d["flags"][t], r["flags"][t]), f"set {t}: flags"
        te._assert_records(d["sins"][t], r["sins"][t], f"set {t}")
    got, sgot = d["last"][4], d["last"][5]
    print("episodes", got["n_episodes"].tolist(), "contacts", sgot["n_contact"].tolist(), "ages", got["min_age"].tolist(), got["max_age"].tolist())
    for name in te._INT_FIELDS:
        assert np.array_equal(got[name], r["stats"][name]), name
    for name in _SP_INT:
        assert np.array_equal(sgot[name], r["sstats"][name]), name
    assert (sgot["n_contact"] == got["n_episodes"]).all() and (got["n_episodes"] > 0).all()


@gpu
def test_rollout_with_the_spawn_model_equals_its_parts(dm, oracle):
    r, d = _cpu_loop(dm, oracle), _device_loop(dm, oracle)
    pl = _planner(dm, r)
    last, trace = pl.rollout(L_TICKS, trace=True)
    pl.sync()
    got = (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), pl.episode_stats(), pl.episode_spawn_stats(), pl.traffic_state())
    pl.close()
    assert last == L_TICKS + 1
    for a, b, name in zip(got, d["last"], ("PlanOut", "SceneState", "flags", "SceneIn", "EpisodeStats", "EpisodeSpawnStats", "traffic")):
        assert a.tobytes() == b.tobytes(), name
    trace = np.array(trace)
    for t in range(L_TICKS):
        assert trace[t].tobytes() == d["trace"][t].tobytes(), f"trace row {t}"
    assert ((trace["flags"] & CONTACT) != 0).sum() == int(got[5]["n_contact"].sum()) > 0


def _record(pl, K):
    _, trace = pl.rollout(K, trace=True)
    pl.sync()
    return (pl.get_plan(), pl.get_state(), pl.ego_flags(), pl.get_scene_in(), pl.episode_stats(), np.array(trace))


_NAMES = ("PlanOut", "SceneState", "flags", "SceneIn", "EpisodeStats", "trace")


@gpu
def test_off_means_off(dm, oracle):
    """A handle that sets the spawn model and switches it off gives the bytes of one that never set it - k_respawn_egos runs again, the egos
    drive through their vehicles - and its stats stay readable, untouched; a handle that never set it has none."""
    r = _cpu_loop(dm, oracle)
    outs = []
    for had in (True, False):
        pl = _planner(dm, r, spawn=had)
        if had:
            pl.set_episode_spawn(None)
        outs.append(_record(pl, 60))
        if had:
            assert not pl.episode_spawn_stats().tobytes().strip(b"\0")
        else:
            with pytest.raises(dm.PlannerError, match="error -4:"):
                pl.episode_spawn_stats()
        pl.close()
    for a, b, name in zip(outs[0], outs[1], _NAMES):
        assert a.tobytes() == b.tobytes(), name
    assert not outs[0][4]["n_episodes"].any()                                  # (no flag, no timeout: without the spawn model nothing ends here)


@gpu
def test_errors_and_lifetime(dm, oracle):
    r = _cpu_loop(dm, oracle)
    n = tt.F_N
    pl = tt._planner(dm, r["cfg"], r["m"], r["sc"], 1)
    pl.set_route(r["legs"], r["rf"])
    pl.set_traffic(r["tracks"], r["pts"], r["act"])
    with pytest.raises(dm.PlannerError, match="error -4:"):                    # PP_ERR_STATE: episodes are off
        pl.set_episode_spawn(r["sp"])
    with pytest.raises(dm.PlannerError, match="error -4:"):                    # ... and the stats of a handle that never set a spawn model
        pl.episode_spawn_stats()
    pl.close()
    starts = (np.concatenate([r["sc"]["scene_in"]] * 2), np.concatenate([r["sc"]["state"]] * 2))
    good = _sp(dm, n_starts=3, order=1, contact=1, check=1, clearance=1.0)

    def fresh():
        p = _planner(dm, r, spawn=False)
        p.set_episode_spawn(good, *starts)
        p.rollout(50)                                                          # (every ego has met its vehicle once)
        return p
    pl, ref = fresh(), fresh()
    off_map = (starts[0].copy(), starts[1])
    off_map[0]["loc"]["road_num"][n + 3] = 99
    for kw in (dict(n_starts=0), dict(n_starts=17), dict(clearance=-1.0), dict(clearance=np.nan), dict(clearance=np.inf), dict(order=2), dict(order=-1), dict(check=4)):
        with pytest.raises(dm.PlannerError, match="error -1:"):                # PP_ERR_ARG
            pl.set_episode_spawn(_sp(dm, **dict(dict(n_starts=3), **kw)), *starts)
    with pytest.raises(dm.PlannerError, match="error -1:"):                    # ... NULL arrays with n_starts > 1
        pl.set_episode_spawn(good)
    with pytest.raises(dm.PlannerError, match="error -1:"):                    # ... a start record off the map, as pp_set_egos refuses it
        pl.set_episode_spawn(good, *off_map)
    pl.advance_async()
    ref.advance_async()
    for args in ((good,) + starts, (None,)):                                   # PP_ERR_STATE: an update is staged
        with pytest.raises(dm.PlannerError, match="error -4:"):
            pl.set_episode_spawn(*args)
    # none of it changed the model, the pool or the stats: the run goes on like the reference run
    for p in (pl, ref):
        p.tick()
        p.rollout(40)
        p.sync()
    for name in ("get_plan", "get_state", "ego_flags", "get_scene_in", "episode_stats", "episode_spawn_stats"):
        assert getattr(pl, name)().tobytes() == getattr(ref, name)().tobytes(), name
    ss = pl.episode_spawn_stats()
    assert (ss["n_contact"] > 0).all() and ss["n_used"][:, 1].any()
    ref.close()
    # a second pp_set_episode_spawn zeroes the stats; every successful pp_set_episodes switches the spawn model off - its record 0 is gone - and
    # the stats stay readable: k_respawn_egos runs, contacts end nothing
    pl.set_episode_spawn(good, *starts)
    assert not pl.episode_spawn_stats().tobytes().strip(b"\0")
    pl.rollout(3)
    pl.set_episodes(r["em"])
    before = pl.episode_spawn_stats()
    pl.rollout(60)
    pl.sync()
    assert pl.episode_spawn_stats().tobytes() == before.tobytes() and not pl.episode_stats()["n_episodes"].any()
    pl.set_episode_spawn(r["sp"])
    pl.set_episodes(off=True)                                                  # NULL included
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_spawn(r["sp"])
    # pp_set_egos switches it off through the episodes
    pl.set_episodes(r["em"])
    pl.set_episode_spawn(r["sp"])
    pl.set_egos(r["sc"], with_motion=False)
    pl.set_state(r["sc"]["state"])
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_spawn(r["sp"])
    pl.close()


@gpu
@pytest.mark.parametrize("with_map", [False, True], ids=["no_map", "map_but_pp_set_scenes"])
def test_a_pool_needs_scenes_placed_on_the_map(dm, with_map):
    """n_starts > 1 on scenes that are not resident from pp_set_map + pp_set_egos - scenes with their own slices (pp_set_scenes), with no
    map on the handle or with one the scenes were not placed on - is PP_ERR_STATE: the start records could not be placed.  On a handle
    with no model yet it leaves none (the stats are still those of a handle that never set one); on a handle with a model in force -
    n_starts = 1 is accepted on any resident scenes - it leaves the model, both stats records and the next rollout's bytes as they were."""
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    n, n_obs = 9, 8
    sc = dm.gen_scenes(cfg, 0, n, n_obs, junction_every=4)
    em = te._em(dm, 31, 7)                                                     # (a timeout: every scene restarts several times below)
    one, two = _sp(dm, contact=1, check=1, clearance=1.0), _sp(dm, n_starts=2, order=1, contact=1, check=1, clearance=1.0)
    starts = (sc["scene_in"].copy(), sc["state"].copy())

    def fresh():
        p = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
        if with_map:
            p.set_map(te._world(dm)["map"])
        p.set_scenes(sc, with_motion=False)
        p.set_state(sc["state"])
        p.set_episodes(em)
        return p
    pl, ref = fresh(), fresh()
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_spawn(two, *starts)
    with pytest.raises(dm.PlannerError, match="error -4:"):                    # no model was set: none is readable
        pl.episode_spawn_stats()
    for p in (pl, ref):
        p.set_episode_spawn(one)                                               # M = 1: contact ending and statistics alone, on any resident scenes
        p.rollout(10)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.set_episode_spawn(two, *starts)
    for p in (pl, ref):
        p.rollout(12)
        p.sync()
    for name in ("get_plan", "get_state", "ego_flags", "get_scene_in", "episode_stats", "episode_spawn_stats"):
        assert getattr(pl, name)().tobytes() == getattr(ref, name)().tobytes(), name
    es, ss = pl.episode_stats(), pl.episode_spawn_stats()
    assert (es["n_episodes"] >= 3).all() and np.array_equal(ss["n_used"][:, 0], es["n_episodes"]) and not ss["n_used"][:, 1:].any()
    pl.close()
    ref.close()
