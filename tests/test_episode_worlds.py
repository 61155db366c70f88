"""World episodes (pp_set_episode_worlds): the egos of a world restart together.

CPU: the draw's known answers, the world's cause word, the spawn-stats words, the blocked-by-some-member rule and the neutral model
on tests/episode_world_model.py; the header's declarations.
GPU: k_respawn_world against the model byte for byte (tests/episode_world_backends.py) on worlds of 1 .. 257 members, with the
ender first, in the middle and last, two enders, every world and no world ending, own slices of 0 | 1 | 64 | 65 entries, the candidate
walk for M = 1, 2, 3, 16, both orders, check 0 | 1 | 3, the neutral comparisons against k_respawn_spawn, the episode log and the
scorecard behind it.  The closed loop, the world traffic reset, the error paths and the life cycle: tests/test_episode_world_loop.py.

The scripts.  The map, the ego and the paths are those of tests/test_episodes.py: lane 2 of road 1 along y = 0.  Every scene's ego
reads (110, 0); start record k >= 1 stands at (100 + 3 k, 0).  Vehicle_Width is 2.0 (hw = 1), every obstacle has radius 0.5 and stands
straight beside a pose, so d = (D - 0.5) - 1 is exact: D = 1.5 touches, D = 3.5 is at the clearance 2.0 - blocked.  An ender of its own is
scripted with a NaN in point 0 of its path (BAD_PATH, cause 2: the record is carried over) or with a touching obstacle (CONTACT)."""
import os

import numpy as np
import pytest

import episode_spawn_backends as esb
import episode_spawn_model as esm
import episode_world_backends as ewb
import episode_world_model as ewm
import test_episodes as te

gpu = pytest.mark.gpu
WORLD, CONTACT, BAD_PATH = 256, 128, 2
FAR = (500.0, 500.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _x(k):
    return 110.0 if k == 0 else 100.0 + 3.0 * k


def _starts(dm, M, n):
    """Start records 1 .. M - 1 of n scenes, record k of scene s at (k - 1) n + s: (100 + 3 k, 0) and fields only (k, s) carries."""
    if M == 1:
        return None
    si, st = [], []
    for k in range(1, M):
        r = np.concatenate([te._ego(dm, _x(k), ego_id=6 * k)] * n)
        r["period_last"], r["goal"]["x"], r["goal"]["y"] = 100.0 + k, np.arange(n), -float(k)
        s = np.concatenate([te._state0(dm)] * n)
        s["tick"], s["brakespeed"] = 7 + 10 * k, 1.0 + np.arange(n)
        si.append(r), st.append(s)
    return np.concatenate(si), np.concatenate(st)


def _bad_path(dm, x):
    po = te._path(dm, x)
    po["road_points"]["x"][0, 0] = np.nan
    return po


def _first(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _script(dm, cfg1, sizes, enders, M=2, fleet=True, worlds=True, obs=None, steps=1, em=None, log=0, score=False, peers=0, tk=None, xs=None, **sp):
    """n = sum(sizes) scenes in worlds of `sizes` members; the scenes of `enders` read a NaN path on every step.  obs: {scene: points};
    xs: {scene: x of its ego} (default 110); peers, tk: tests/episode_world_backends.py."""
    n = int(sum(sizes))
    x = [float((xs or {}).get(s, 110.0)) for s in range(n)]
    si = np.concatenate([te._ego(dm, x[s], ego_id=int(round((x[s] - 100.0) / 0.5))) for s in range(n)])
    si["goal"]["x"] = 1000.0 + np.arange(n)
    po = np.concatenate([_bad_path(dm, x[s]) if s in enders else te._path(dm, x[s]) for s in range(n)])
    ob = [_obs(dm, (obs or {}).get(s, [])) for s in range(n)]
    spawn = _sp(dm, n_starts=M, **dict(dict(order=1), **sp))
    return ewb.Case(cfg1, dm.default_ego_model(), te._em(dm) if em is None else em, spawn, si, ob, np.concatenate([te._state0(dm)] * n),
                    [(po, np.zeros(n, dm.SceneState))] * steps, te._world(dm), None, _starts(dm, M, n), _first(sizes) if fleet else None, score,
                    worlds=worlds, log=log, peers=peers, tk=tk)


def _runner(name):
    return ewb.Runner(ewb.ModelBackend() if name == "model" else ewb.DeviceBackend())


def _words(r, s):
    e = r.sstats[s]
    return (int(e["n_blocked"]), int(e["n_rejected"]), int(e["cur_start"]), tuple(e["n_used"].tolist()))


def _hold_structure(case, r, enders, c_own=BAD_PATH):
    """What §4s says of ONE step from fresh stats, whatever the draw: a world with an ender ends as a whole - cause words, no n_end slot
    for WORLD, the same spawn-stats words in every member, every member on ITS record k -, a world without one goes on."""
    rec_in, rec_st = case.pools(case.laid_out()[0])
    wf = case.world_first if case.world_first is not None else np.arange(case.n + 1)
    for a, b in zip(wf[:-1], wf[1:]):
        mine = [s for s in range(a, b) if s in enders]
        for s in range(a, b):
            e = r.stats[s]
            if not mine:
                assert (int(e["n_episodes"]), int(e["age"]), int(e["last_cause"])) == (0, 1, 0), s
                assert not r.sstats[s].tobytes().strip(b"\0") and float(r.out["loc"]["globalpoint"]["x"][s]) == 111.0, s
                continue
            want = (c_own if s in mine else 0) | (WORLD if [t for t in mine if t != s] else 0)
            assert (int(e["n_episodes"]), int(e["age"]), int(e["last_cause"]), int(e["last_age"])) == (1, 0, want, 1), (s, int(e["last_cause"]), want)
            assert e["n_end"].tolist() == [0, int(s in mine and c_own == BAD_PATH), 0, 0, 0, 0], s
            assert _words(r, s) == _words(r, a), (s, a)
            k = int(r.sstats["cur_start"][s])
            assert r.out[s].tobytes() == rec_in[k][s].tobytes() and r.state[s].tobytes() == rec_st[k][s].tobytes() and int(r.flags[s]) == 0, (s, k)
            assert int(r.trace["flags"][s]) == (32 | (BAD_PATH if s in mine and c_own == BAD_PATH else 0) | (CONTACT if s in mine and c_own == CONTACT else 0)), s


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_draw_known_answers():
    """§4s: the world's first scene stands for the world - the known answers are §4l's."""
    for (seed, a, e), ks in (((1, 0, 1), (0, 1, 1, 8)), (((1 << 64) - 1, 5, 2), (0, 1, 2, 12)), ((2026, 1023, 100), (0, 1, 1, 10))):
        assert tuple(esm.first_choice(seed, a, e, M, 0) for M in (1, 2, 3, 16)) == ks
    assert ewm.WORLD == WORLD


def test_header_declares_the_new_symbols(dm):
    with open(os.path.join(ROOT, "include", "dmpp_planner.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "dmpp_types.h")) as f:
        t = f.read()
    for decl in ("int  pp_set_episode_worlds(pp_handle h, int on);", "int  pp_set_episode_world_traffic(pp_handle h, int n_sets, const TrafficStart* starts);",
                 "int  pp_get_episode_world_traffic_resets(pp_handle h, int32_t* n_resets, int n);"):
        assert decl in h, decl
    assert "#define DMPP_EGO_WORLD 256" in t and dm.EGO_WORLD == WORLD
    lib = dm.load_library()
    for sym in ("pp_set_episode_worlds", "pp_set_episode_world_traffic", "pp_get_episode_world_traffic_resets"):
        assert getattr(lib, sym)
    # the feature table has no new cause
    assert lib.pp_feature_retires(14) == -1


def test_world_cause_word():
    members = range(3)
    for c, want in (((2, 0, 0), (2, WORLD, WORLD)), ((2, 0, 128), (2 | WORLD, WORLD, 128 | WORLD)), ((1, 2, 64), (1 | WORLD, 2 | WORLD, 64 | WORLD))):
        assert tuple(ewm.world_cause(c, m, members) for m in members) == want
    assert ewm.world_cause((4,), 0, range(1)) == 4                             # a sole ender carries no WORLD bit


SIZES = [1, 2, 3, 4, 5]
ENDERS = {0, 2, 4, 10, 14}          # world of 1: itself; of 2: its last; of 3: its middle; of 4: none; of 5: first and last


@pytest.mark.parametrize("fleet", [True, False], ids=["fleet", "no_fleet"])
def test_one_two_all_and_no_enders_on_the_model(dm, cfg1, fleet):
    sizes = SIZES if fleet else [1] * 15
    for enders in (ENDERS, set(range(15)), set()):
        case = _script(dm, cfg1, sizes, enders, fleet=fleet)
        (r,) = _runner("model")(case)
        _hold_structure(case, r, enders)
        assert fleet or not any(int(c) & WORLD for c in r.stats["last_cause"])
    # WORLD is never counted in n_end, CONTACT neither: a world of 3 whose middle member touches
    case = _script(dm, cfg1, [3], {1}, obs={1: [(110.0, 1.5)]}, contact=1, em=te._em(dm, 29, 0))          # (BAD_PATH masked out: the NaN path ends nothing)
    (r,) = _runner("model")(case)
    assert r.stats["last_cause"].tolist() == [WORLD, CONTACT, WORLD] and not r.stats["n_end"].any() and r.sstats["n_contact"].tolist() == [0, 1, 0]


def _walk_case(dm, cfg1, M, i, check=1, order=1, fleet=True, last_only=False):
    """A world of 3 (scenes 1 .. 3 of 5) whose first member ends; round robin, first ending: k0 = 1 mod M.  Candidates k0 .. k0 + i - 1 are
    blocked (i = M: all of them), each by ONE entry of ONE member's own slice, the members in rotation (last_only: always the last) -
    the entry stands 3.5 m beside THAT record's pose.  Own slices of 0, 1, 64 and 65 entries."""
    k0 = 1 % M
    obs = {1: [], 2: [FAR], 3: [FAR] * 65, 0: [FAR] * 64}
    for j in range(i):
        k = (k0 + j) % M
        m = 3 if last_only or j % 2 == 0 else 2
        if j == 0:
            obs[3][64] = (_x(k), 3.5)                                         # entry 64 of the last member: the second pass of 64
        else:
            obs[m] = obs[m] + [(_x(k), -3.5)]
    return _script(dm, cfg1, [1, 3, 1], {1}, M=M, obs=obs, check=check, order=order, clearance=2.0, fleet=fleet), k0


WALKS = [(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3), (16, 0), (16, 1), (16, 15), (16, 16)]


def _hold_walk(case, r, M, i, k0, blocked_on=True):
    want = (0, 0, k0) if not blocked_on else ((1, M, k0) if i == M else (0, i, (k0 + i) % M))
    for s in (1, 2, 3):
        used = tuple(int(j == want[2]) for j in range(16))
        assert _words(r, s) == want + (used,), (M, i, s, _words(r, s), want)
    assert not r.sstats[0].tobytes().strip(b"\0") and not r.sstats[4].tobytes().strip(b"\0")
    _hold_structure(case, r, {1})


@pytest.mark.parametrize("M,i", WALKS)
def test_blocked_by_some_member_on_the_model(dm, cfg1, M, i):
    case, k0 = _walk_case(dm, cfg1, M, i)
    (r,) = _runner("model")(case)
    _hold_walk(case, r, M, i, k0)
    # check bit 0 clear: nobody looks; check 3: bit 1 changes nothing
    case0, _ = _walk_case(dm, cfg1, M, i, check=0)
    (r0,) = _runner("model")(case0)
    _hold_walk(case0, r0, M, i, k0, blocked_on=False)
    case3, _ = _walk_case(dm, cfg1, M, i, check=3)
    ewb.same_bytes(_runner("model")(case3), [r], "check 3 against check 1")


def test_a_slice_outside_the_pool_is_empty_on_the_model(dm, cfg1):
    case, k0 = _walk_case(dm, cfg1, 3, 1, last_only=True)
    si, pool, pin, pst, stats, sstats = case.start()
    hw, own = 1.0, (si["obs_off"].copy(), si["obs_n"].copy())
    members = range(1, 4)
    assert ewm.blocked(case.sp, pin, k0, members, si, own, pool, hw)
    own[1][3] = len(pool)                                                      # the last member's slice now ends beyond the pool: read as empty
    assert not ewm.blocked(case.sp, pin, k0, members, si, own, pool, hw)
    own[1][3], own[0][3] = 65, -1
    assert not ewm.blocked(case.sp, pin, k0, members, si, own, pool, hw)


def _peer_case(dm, cfg1, own_blocker):
    """A world of two with K = 2 peer slots, M = 3, round robin: member 0 (scene 0) ends, k0 = 1, its record 1 stands at (103, 0) - and so does
    the EGO of member 1, which k_couple_fleet has written into member 0's first peer slot: an entry of the slice the advance read, at distance 0
    of the candidate, that is NOT an own entry and must not block.  own_blocker: the same candidate blocked by an own entry 3.5 m beside it."""
    obs = {0: [FAR, (103.0, 3.5)] if own_blocker else [FAR, FAR], 1: [FAR]}
    return _script(dm, cfg1, [2], {0}, M=3, obs=obs, check=1, clearance=2.0, peers=2, xs={1: 103.0})


def _hold_peers(run):
    def check(dm, cfg1):
        for own_blocker, want in ((False, (0, 0, 1)), (True, (0, 1, 2))):
            case = _peer_case(dm, cfg1, own_blocker)
            si0, pool0 = case.start()[:2]
            assert si0["obs_n"].tolist() == [3, 2] and case.own()[1].tolist() == [2, 1]          # own entries + one peer in range each
            peer = pool0[int(si0["obs_off"][0]) + 2]
            assert (float(peer["x"]), float(peer["y"])) == (103.0, 0.0)                             # member 1, ON the candidate's pose
            (r,) = _runner(run)(case)
            assert _words(r, 0)[:3] == _words(r, 1)[:3] == want, (own_blocker, _words(r, 0))
            assert r.stats["last_cause"].tolist() == [BAD_PATH, WORLD]
    return check


def test_peer_slots_do_not_block_on_the_model(dm, cfg1):
    _hold_peers("model")(dm, cfg1)
    # a walk that scanned the whole slice the advance read - peer slots included - would reject record 1: the model says so when it is handed that slice
    case = _peer_case(dm, cfg1, False)
    si, pool, pin, pst, stats, sstats = case.start()
    assert not ewm.blocked(case.sp, pin, 1, range(2), si, case.own(), pool, 1.0)
    assert ewm.blocked(case.sp, pin, 1, range(2), si, (si["obs_off"], si["obs_n"]), pool, 1.0)


@gpu
def test_peer_slots_do_not_block_on_the_device(dm, cfg1):
    _hold_peers("device")(dm, cfg1)


def _hold_tracker(dm, cfg1, run):
    """The ego tracker (§4q) behind world episodes: 15 scenes in worlds of 1 .. 5, scene 10 touches an obstacle beside its start pose on each of
    three advances, so its world of 5 restarts three times - scene 10 with CONTACT, its partners with exactly 256.  The advance behind a restart
    finds age 0 in EVERY member and re-derives its state (n_init goes up by one per restart); the other worlds derive once.  Every step: device
    against model, EgoTrackState included."""
    import test_ego_track as tet
    case = _script(dm, cfg1, SIZES, set(), M=1, steps=3, obs={10: [(110.0, 1.5)]}, contact=1, tk=tet._tk(dm, curv_bias=0.04))
    r = _runner(run)(case)
    for t, q in enumerate(r):
        assert q.stats["last_cause"][10:15].tolist() == [CONTACT, WORLD, WORLD, WORLD, WORLD] and q.stats["n_episodes"][10:15].tolist() == [t + 1] * 5
        assert q.track["n_init"][10:15].tolist() == [t + 1] * 5 and q.track["n_init"][:10].tolist() == [1] * 10, (t, q.track["n_init"].tolist())
        assert (q.track["valid"] == 1).all() and not q.stats["n_episodes"][:10].any()


def test_the_tracker_re_derives_in_every_member_on_the_model(dm, cfg1):
    _hold_tracker(dm, cfg1, "model")


@gpu
def test_the_tracker_re_derives_in_every_member_on_the_device(dm, cfg1):
    _hold_tracker(dm, cfg1, "device")


def _neutral_script(dm, cfg1, M, fleet, worlds, check):
    """9 scenes, worlds of one; scenes 0, 3, 4, 8 end on BAD_PATH, scene 5 on CONTACT, scene 6 has a blocker on record 1 mod M; hashed
    order, two steps."""
    obs = {5: [(110.0, 1.5)], 6: [FAR, (_x(1 % M), 3.5)], 7: [FAR]}
    return _script(dm, cfg1, [1] * 9, {0, 3, 4, 6, 8}, M=M, fleet=fleet, worlds=worlds, obs=obs, steps=2, order=0, seed=7, contact=1, check=check, clearance=2.0)


@pytest.mark.parametrize("M", [1, 2, 3, 16])
def test_neutral_model_on_the_model(dm, cfg1, M):
    """Worlds of one - a fleet of singletons or no fleet, check bit 1 set or not -: every byte is §4l's."""
    for fleet in (True, False):
        for check in (1, 3):
            want = esb.ModelBackend().run(_neutral_script(dm, cfg1, M, fleet, False, check))
            got = _runner("model")(_neutral_script(dm, cfg1, M, fleet, True, check))
            ewb.same_bytes(got, want, f"M {M} fleet {fleet} check {check}")
            assert int(got[-1].stats["n_episodes"].sum()) >= 6 and not any(int(c) & WORLD for c in got[-1].stats["last_cause"])


# ---------------------------------------------------------------------------------------------------------------
# GPU
BIG = [1, 2, 3, 4, 5, 63, 64, 65]                                              # 207 scenes
BIG_ENDERS = {0, 2, 4, 10, 14, 15, 15 + 63 + 63, 15 + 63 + 64 + 64}            # ... world of 63: its first; of 64: its last; of 65: its last (member 64)


@gpu
@pytest.mark.parametrize("sizes,enders", [(SIZES, ENDERS), (SIZES, set(range(15))), (SIZES, set()), (BIG, BIG_ENDERS), ([129, 43], {64}), ([257, 43], {256}),
                                          ([1] * 5, {1, 4}), ([100] * 3, {0, 150, 299})],
                         ids=["5_worlds", "all_end", "none_ends", "207_scenes", "world_of_129", "world_of_257", "5_scenes", "300_scenes"])
def test_worlds_end_together_on_the_device(dm, cfg1, sizes, enders):
    """One advance from fresh stats, device against model byte for byte (Runner) and against §4s's structure.  M = 3, hashed: worlds whose
    first scene differs draw differently."""
    case = _script(dm, cfg1, sizes, enders, M=3, order=0, seed=11)
    (r,) = _runner("device")(case)
    _hold_structure(case, r, enders)
    wf = case.world_first
    for a, b in zip(wf[:-1], wf[1:]):
        if any(a <= s < b for s in enders):
            assert int(r.sstats["cur_start"][a]) == esm.first_choice(11, int(a), 1, 3, 0), a


@gpu
def test_a_world_alone_and_inside_the_batch(dm, cfg1):
    """The world of 5 with two enders alone and as the last world of 15 scenes, round robin (the draw does not depend on the scene index)."""
    (alone,) = _runner("device")(_script(dm, cfg1, [5], {0, 4}, M=3))
    (batch,) = _runner("device")(_script(dm, cfg1, SIZES, ENDERS, M=3))
    for name in ("flags", "trace", "stats", "sstats"):
        assert getattr(batch, name)[10:15].tobytes() == getattr(alone, name).tobytes(), name
    for name, fields in (("out", ("obs_off", "goal")), ("state", ("brakespeed",))):          # (the fields the script writes a scene's index into)
        a, b = getattr(alone, name).copy(), getattr(batch, name)[10:15].copy()
        for rec in (a, b):
            for f in fields:
                rec[f] = np.zeros(1, rec.dtype[f])[0]
        assert a.tobytes() == b.tobytes(), name


def test_two_steps_with_contact_and_timeout_on_the_model(dm, cfg1):
    _two_steps(dm, cfg1, "model")


@gpu
def test_two_steps_with_contact_and_timeout_on_the_device(dm, cfg1):
    _two_steps(dm, cfg1, "device")


def _two_steps(dm, cfg1, name):
    """Two advances: a touching obstacle in scene 7 (world of 4) and max_ticks = 2 - on the second advance every world ends on TIMEOUT, every
    member with 64 | 256 but the world of one (64 alone); the world of 4 ended on the first advance and is one tick old: it goes on."""
    case = _script(dm, cfg1, SIZES, set(), M=2, obs={7: [(110.0, 1.5)], 8: [FAR]}, steps=2, contact=1, em=te._em(dm, 31, 2))
    r = _runner(name)(case)
    assert r[0].stats["last_cause"][6:10].tolist() == [WORLD, CONTACT, WORLD, WORLD] and not r[0].stats["last_cause"][:6].any()
    assert r[1].stats["last_cause"].tolist() == [64] + [64 | WORLD] * 5 + [WORLD, CONTACT, WORLD, WORLD] + [64 | WORLD] * 5
    assert r[1].stats["age"][6:10].tolist() == [1] * 4 and r[1].stats["n_end"][:, 5].tolist() == [1] * 6 + [0] * 4 + [1] * 5


@gpu
@pytest.mark.parametrize("M,i", WALKS)
def test_candidate_walk_on_the_device(dm, cfg1, M, i):
    case, k0 = _walk_case(dm, cfg1, M, i)
    (r,) = _runner("device")(case)
    _hold_walk(case, r, M, i, k0)


@gpu
@pytest.mark.parametrize("order", [0, 1])
def test_check_bit_1_changes_nothing_on_the_device(dm, cfg1, order):
    """check 0 | 1 | 3 on the walk whose only blocking entry is entry 64 of the LAST member: 0 takes k0, 1 and 3 give the same bytes."""
    runs = {}
    for check in (0, 1, 3):
        case, k0 = _walk_case(dm, cfg1, 3, 1, check=check, order=order, last_only=True)
        (runs[check],) = _runner("device")(case)
    k0 = esm.first_choice(1, 1, 1, 3, order)
    assert _words(runs[0], 1)[:3] == (0, 0, k0)
    ewb.same_bytes([runs[1]], [runs[3]], "check 1 against check 3")
    blocked = k0 == 1                                                          # (the blocker stands beside record 1 mod 3)
    assert _words(runs[1], 3)[:3] == ((0, 1, 2) if blocked else (0, 0, k0))


@gpu
@pytest.mark.parametrize("M", [1, 2, 3, 16])
def test_worlds_of_one_give_the_bytes_of_k_respawn_spawn(dm, cfg1, M):
    for fleet in (True, False):
        want = esb.DeviceBackend().run(_neutral_script(dm, cfg1, M, fleet, False, 3))
        got = _runner("device")(_neutral_script(dm, cfg1, M, fleet, True, 3))
        ewb.same_bytes(got, want, f"M {M} fleet {fleet}")
    assert int(got[-1].stats["n_episodes"].sum()) >= 6


@gpu
def test_the_episode_log_behind_world_episodes(dm, cfg1):
    """One record per member, by scene index, cause with 256, start the record the ENDED episode ran on (round robin, M = 3: 0, then 1)."""
    case = _script(dm, cfg1, SIZES, {2, 10}, M=3, steps=2, log=64)
    r = _runner("device")(case)
    ended = [1, 2] + list(range(10, 15))
    for t, want_start in ((0, 0), (1, 1)):
        rec = r[t].records
        assert rec["scene"].tolist() == ended and rec["start"].tolist() == [want_start] * 7 and rec["episode"].tolist() == [t] * 7
        assert rec["cause"].tolist() == [WORLD, BAD_PATH, BAD_PATH, WORLD, WORLD, WORLD, WORLD]
        assert rec["age"].tolist() == [1] * 7


@gpu
def test_the_scorecard_follows_the_worlds_record(dm, cfg1):
    case = _script(dm, cfg1, [3], {1}, M=2, score=True)
    (r,) = _runner("device")(case)
    (w,) = ewb.ModelBackend().run(case)
    assert r.score["last_pos"]["x"].tolist() == [_x(1)] * 3 and r.score["last_pos"]["y"].tolist() == [0.0] * 3
    for f in ("last_pos", "last_speed", "n_ticks", "dist", "max_speed", "max_acc", "max_dec"):          # (what §4d derives from the ego alone)
        assert r.score[f].tobytes() == w.score[f].tobytes(), f


@gpu
def test_two_runs_give_the_same_bytes(dm, cfg1):
    case = _script(dm, cfg1, BIG, BIG_ENDERS, M=16, order=0, steps=2, check=1)
    ewb.same_bytes(ewb.DeviceBackend().run(case), ewb.DeviceBackend().run(case), "run 2 against run 1")
