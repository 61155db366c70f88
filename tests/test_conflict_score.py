"""The conflict score: time to collision and braking demand per scene from the snapshots of consecutive scored ticks.

CPU tests: hand-derived known answers and the rules of the step on the numpy model (tests/conflict_model.py), the ABI mirror, the
defaults, a null handle.
GPU tests: k_score_ego<., ., true> inside a real tick against the model, byte for byte (tests/conflict_backends.py) - the same
known answers and rules, the 64-lane stride with the only closing entry the last one, ties across the wave, one scene alone and inside
batches of 5 and 300, off = the engine without it, the life cycle, the error paths, and the closed loops of §4l, §4k and §4j.

Every crafted case stands on hw = 1 (Vehicle_Width 2), radius 0.5 (R = 1.5) and dt_score = 0.5, with ego and obstacle on or beside the
x axis, so that every product, root and quotient below is exact.  An obstacle dead ahead at distance D that closes with vc has
c = D^2 - 2.25, b = -D vc, disc = D^2 vc^2 - vc^2 (D^2 - 2.25) = 2.25 vc^2 and ttc = (D^2 - 2.25) / (D vc + 1.5 vc) = (D - 1.5) / vc."""
import math

import numpy as np
import pytest

import conflict_backends as cfb
import conflict_model as cm
import coupling_backends as cb

gpu = pytest.mark.gpu
INF, NAN = math.inf, math.nan
DT = 0.5
R05 = 0.5


@pytest.fixture()
def cfg1(dm):
    cfg = cb.config()
    cfg["Vehicle_Width"] = 2.0
    return cfg


def _cm(dm, warn=3.0, crit=1.5, v_max=70.0, min_closing=0.0):
    m = np.zeros(1, dm.ConflictModel)
    m["ttc_warn"], m["ttc_crit"], m["v_max"], m["min_closing"] = warn, crit, v_max, min_closing
    return m


def _runner(name):
    return (cfb.ModelBackend() if name == "model" else cfb.DeviceBackend()).run


def _t(cfg, ego, obs=(), **kw):
    """One scene: the ego at `ego` (x, y), obstacles (x, y) of radius 0.5 or (x, y, radius)."""
    return cb.tick(cfg, [(ego[0], ego[1], 36.0, [(o[0], o[1], o[2] if len(o) > 2 else R05) for o in obs])], **kw)


def _c(conf, s=0):
    """(n_ticks, n_conflict_ticks, n_warn_ticks, n_crit_ticks, n_no_history_ticks) of scene s."""
    return tuple(int(conf[f][s]) for f in ("n_ticks", "n_conflict_ticks", "n_warn_ticks", "n_crit_ticks", "n_no_history_ticks"))


def _min(conf, s=0):
    return (float(conf["min_ttc"][s]), int(conf["min_ttc_tick"][s]), int(conf["min_ttc_obs"][s]))


def _drac(conf, s=0):
    return (float(conf["max_drac"][s]), int(conf["max_drac_tick"][s]))


START = dict(min_ttc=INF, max_drac=0.0, tit_warn=0.0, n_ticks=0, n_conflict_ticks=0, n_warn_ticks=0, n_crit_ticks=0, min_ttc_tick=-1, min_ttc_obs=-1,
             min_ttc_type=0, first_crit_tick=-1, max_drac_tick=-1, n_no_history_ticks=0, prev_off=0, prev_n=0)


def _is_start(conf):
    return all((conf[f] == v).all() for f, v in START.items()) and (conf["last_pos"]["x"] == 0).all() and (conf["last_pos"]["y"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# known answers, asserted on both legs
def _kat_head_on_static_obstacle(dm, cfg, run):
    """ego (0, 0) -> (2, 0): u = (4, 0); the obstacle stands at (31.5, 0): w = (-4, 0), p = (29.5, 0), q = 870.25, c = 868, b = -118,
    vc = 4, a = 16, disc = 13924 - 13888 = 36, ttc = 868 / (118 + 6) = 7; gap = 28, drac = 16 / 56.  7 > ttc_warn 3: no warn tick.
    Tick 0 has no tick before it: no conflict and - k = 0 - no missing history either."""
    r = run(cfg, DT, _cm(dm), [_t(cfg, (0.0, 0.0), [(31.5, 0.0)]), _t(cfg, (2.0, 0.0), [(31.5, 0.0)])])
    assert _is_start(r.start)
    assert _c(r.conf[0]) == (1, 0, 0, 0, 0) and _min(r.conf[0]) == (INF, -1, -1) and int(r.conf[0]["prev_n"][0]) == 1
    assert _c(r.conf[1]) == (2, 1, 0, 0, 0) and _min(r.conf[1]) == (7.0, 1, 0) and _drac(r.conf[1]) == (16 / 56, 1)
    assert float(r.conf[1]["tit_warn"][0]) == 0.0 and int(r.conf[1]["first_crit_tick"][0]) == -1
    assert (float(r.conf[1]["last_pos"]["x"][0]), float(r.conf[1]["last_pos"]["y"][0])) == (2.0, 0.0)


def _kat_graze_and_its_twin(dm, cfg, run):
    """ego (-2, 0) -> (0, 0), obstacle at (10, 1.5): q = 102.25, c = 100, b = -40, a = 16, disc = 1600 - 1600 = 0: the discs touch in
    passing, ttc = 100 / 40 = 2.5 <= 3: one warn tick, tit_warn = 0.5 * 0.5.  vc = 40 / sqrt(102.25) as the device rounds it.
    The twin 2^-30 further out: (1.5 + 2^-30)^2 rounds to 2.25 + 3 * 2^-30, c = 100 + 3 * 2^-30, disc = -48 * 2^-30 < 0: a miss."""
    r = run(cfg, DT, _cm(dm), [_t(cfg, (-2.0, 0.0), [(10.0, 1.5)]), _t(cfg, (0.0, 0.0), [(10.0, 1.5)])])
    vc = 40.0 / math.sqrt(102.25)
    assert _c(r.conf[1]) == (2, 1, 1, 0, 0) and _min(r.conf[1]) == (2.5, 1, 0) and float(r.conf[1]["tit_warn"][0]) == 0.25
    assert _drac(r.conf[1]) == (vc * vc / (2 * (math.sqrt(102.25) - 1.5)), 1)
    y = 1.5 + 2.0 ** -30
    r = run(cfg, DT, _cm(dm), [_t(cfg, (-2.0, 0.0), [(10.0, y)]), _t(cfg, (0.0, 0.0), [(10.0, y)])])
    assert _c(r.conf[1]) == (2, 0, 0, 0, 0) and _min(r.conf[1]) == (INF, -1, -1) and _drac(r.conf[1]) == (0.0, -1)


def _kat_contact_perpendicular_and_standstill(dm, cfg, run):
    """Contact: the obstacle 1.5 m ahead of the ego, both driving 1 m per tick (w = 0) and then apart: c = 0, ttc = 0 whatever w is -
    a critical tick - and no DRAC.  Perpendicular: a standing ego and an obstacle that moves (10, -1) -> (10, 0): p = (10, 0),
    w = (0, 2), b = 0: not closing.  Standstill: the same inputs twice: u = 0, w = 0, b = 0: a static obstacle is not closing."""
    ticks = [_t(cfg, (0.0, 0.0), [(1.5, 0.0)]), _t(cfg, (1.0, 0.0), [(2.5, 0.0)]), _t(cfg, (1.0, 0.0), [(2.5, 0.0)]), _t(cfg, (0.0, 0.0), [(1.5, 0.0)])]
    r = run(cfg, DT, _cm(dm), ticks)
    assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 1, 1, 1, 0), (3, 2, 2, 2, 0), (4, 3, 3, 3, 0)]
    assert _min(r.conf[3]) == (0.0, 1, 0) and _drac(r.conf[3]) == (0.0, -1) and int(r.conf[3]["first_crit_tick"][0]) == 1
    assert [float(c["tit_warn"][0]) for c in r.conf] == [0.0, 1.5, 3.0, 4.5]                     # (3 - 0) * 0.5 per tick
    r = run(cfg, DT, _cm(dm), [_t(cfg, (0.0, 0.0), [(10.0, -1.0)]), _t(cfg, (0.0, 0.0), [(10.0, 0.0)])])
    assert _c(r.conf[1]) == (2, 0, 0, 0, 0)
    r = run(cfg, DT, _cm(dm), [_t(cfg, (0.0, 0.0), [(3.0, 0.0)]), _t(cfg, (0.0, 0.0), [(3.0, 0.0)]), _t(cfg, (0.0, 0.0), [(3.0, 0.0)])])
    assert _c(r.conf[2]) == (3, 0, 0, 0, 0) and _min(r.conf[2]) == (INF, -1, -1)


def _head_on(cfg, n):
    """n ticks of the ego driving 2 m per tick from (0, 0) at the obstacle at (31.5, 0): vc = 4, ttc = 7, 6.5, 6, ... from tick 1 on."""
    return [_t(cfg, (2.0 * k, 0.0), [(31.5, 0.0)]) for k in range(n)]


def _kat_closing_speed_tie(dm, cfg, run):
    """vc = 4 exactly: min_closing 4 gives no conflict (strict >), one ulp below 4 gives the TTC of 7."""
    r = run(cfg, DT, _cm(dm, min_closing=4.0), _head_on(cfg, 2))
    assert _c(r.conf[1]) == (2, 0, 0, 0, 0) and _min(r.conf[1]) == (INF, -1, -1)
    r = run(cfg, DT, _cm(dm, min_closing=math.nextafter(4.0, 0.0)), _head_on(cfg, 2))
    assert _c(r.conf[1]) == (2, 1, 0, 0, 0) and _min(r.conf[1]) == (7.0, 1, 0)


def _kat_warn_and_crit_ties(dm, cfg, run):
    """t* = 7 exactly: ttc_warn 7 counts, one ulp below 7 does not; ttc_crit likewise (ttc_warn stays 7)."""
    below = math.nextafter(7.0, 0.0)
    for warn, crit, want in ((7.0, 1.5, (2, 1, 1, 0, 0)), (below, 1.5, (2, 1, 0, 0, 0)), (7.0, 7.0, (2, 1, 1, 1, 0)), (7.0, below, (2, 1, 1, 0, 0))):
        r = run(cfg, DT, _cm(dm, warn=warn, crit=crit), _head_on(cfg, 2))
        assert _c(r.conf[1]) == want, (warn, crit)
        assert int(r.conf[1]["first_crit_tick"][0]) == (1 if want[3] else -1) and float(r.conf[1]["tit_warn"][0]) == 0.0


def _kat_tit_warn_over_three_ticks(dm, cfg, run):
    """ttc 7, 6.5, 6 at ticks 1, 2, 3 (D = 29.5, 27.5, 25.5: disc = 36 each, ttc = 868 / 124, 754 / 116, 648 / 108); ttc_warn 8:
    tit_warn = (1 + 1.5 + 2) * 0.5 = 2.25, summed as 0.5, 1.25, 2.25; ttc_crit 6.5: ticks 2 and 3, the first is 2.  DRAC: 16 / (2 gap),
    gap 28, 26, 24: the largest at tick 3, 16 / 48."""
    r = run(cfg, DT, _cm(dm, warn=8.0, crit=6.5), _head_on(cfg, 4))
    assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 1, 1, 0, 0), (3, 2, 2, 1, 0), (4, 3, 3, 2, 0)]
    assert [float(c["tit_warn"][0]) for c in r.conf] == [0.0, 0.5, 1.25, 2.25]
    assert [_min(c) for c in r.conf[1:]] == [(7.0, 1, 0), (6.5, 2, 0), (6.0, 3, 0)]
    assert int(r.conf[3]["first_crit_tick"][0]) == 2 and _drac(r.conf[3]) == (16 / 48, 3)


def _kat_v_max_ties(dm, cfg, run):
    """A displacement of exactly v_max * dt keeps the velocity, a clearly larger one drops it.  Ego: 2 m per tick, v_max 4 (limit 2):
    ttc 7; v_max 3.9: no history, counted, no conflict.  Entry: a standing ego and an obstacle (13.5, 0) -> (11.5, 0): w = (-4, 0),
    D = 11.5, ttc = 10 / 4 = 2.5 with v_max 4; with v_max 3.9 the entry has no velocity - and the ego's history is not at fault."""
    r = run(cfg, DT, _cm(dm, v_max=4.0), _head_on(cfg, 2))
    assert _c(r.conf[1]) == (2, 1, 0, 0, 0) and _min(r.conf[1]) == (7.0, 1, 0)
    r = run(cfg, DT, _cm(dm, v_max=3.9), _head_on(cfg, 3))
    assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 0, 0, 0, 1), (3, 0, 0, 0, 2)]
    moving = [_t(cfg, (0.0, 0.0), [(13.5, 0.0)]), _t(cfg, (0.0, 0.0), [(11.5, 0.0)])]
    r = run(cfg, DT, _cm(dm, v_max=4.0), moving)
    assert _c(r.conf[1]) == (2, 1, 1, 0, 0) and _min(r.conf[1]) == (2.5, 1, 0) and _drac(r.conf[1]) == (16 / 20, 1)
    r = run(cfg, DT, _cm(dm, v_max=3.9), moving)
    assert _c(r.conf[1]) == (2, 0, 0, 0, 0)


def _approach(cfg, k, extra=(), first=(), **kw):
    """A standing ego at (0, 0) and an obstacle that drives at it with 4 m/s: x = 21.5 - 2 k; from tick 1 on ttc = (20 - 2 k) / 4: 4.5 at k = 1, 4 at k = 2
    (D = 17.5: c = 304, b = -70, disc = 4900 - 4864 = 36, ttc = 304 / 76), drac = 16 / (2 (20 - 2 k)).  first / extra: entries in front of / behind it."""
    return _t(cfg, (0.0, 0.0), list(first) + [(21.5 - 2.0 * k, 0.0)] + list(extra), **kw)


def _kat_one_tick_without_a_velocity(dm, cfg, run):
    """The obstacle of _approach over three ticks: TTCs at ticks 1 (4.5) and 2 (4).  Each of: another type at tick 1, another radius at
    tick 1, the slice moved by one entry from tick 1 on, the entry new at tick 1 behind a list that grew - costs exactly tick 1."""
    r = run(cfg, DT, _cm(dm), [_approach(cfg, k) for k in range(3)])
    assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 1, 0, 0, 0), (3, 2, 0, 0, 0)] and _min(r.conf[1]) == (4.5, 1, 0) and _min(r.conf[2]) == (4.0, 2, 0)
    typed = [_approach(cfg, k) for k in range(3)]
    typed[1].pool["type"][0], typed[2].pool["type"][0] = 5, 5
    radius = [_approach(cfg, 0), _t(cfg, (0.0, 0.0), [(19.75, 0.0, 0.75)]), _t(cfg, (0.0, 0.0), [(17.75, 0.0, 0.75)])]
    # (R = 1.75, D = 17.75: c = 315.0625 - 3.0625 = 312, b = -71, disc = 5041 - 4992 = 49, ttc = 312 / 78 = 4)
    moved = [_approach(cfg, 0), _approach(cfg, 1, lead=1), _approach(cfg, 2, lead=1)]
    grown = [_t(cfg, (0.0, 0.0), [(50.0, 30.0)]), _approach(cfg, 1, first=[(50.0, 30.0)]), _approach(cfg, 2, first=[(50.0, 30.0)])]
    for name, ticks, obs in (("type", typed, 0), ("radius", radius, 0), ("obs_off", moved, 0), ("grown", grown, 1)):
        r = run(cfg, DT, _cm(dm), ticks)
        assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (3, 1, 0, 0, 0)], name
        assert _min(r.conf[2]) == (4.0, 2, obs), name
    assert int(r.conf[2]["prev_n"][0]) == 2 and int(run(cfg, DT, _cm(dm), moved).conf[2]["prev_off"][0]) == 1
    assert int(run(cfg, DT, _cm(dm), typed).conf[2]["min_ttc_type"][0]) == 5


def _kat_nan_infinity_and_no_obstacle(dm, cfg, run):
    """Beside the obstacle of _approach a NaN one and one at infinity: neither has a velocity (NaN - NaN and inf - inf are NaN, and a NaN
    compares false), the record is that of _approach alone.  A scene without obstacles still advances n_ticks, last_pos and prev_n.
    A NaN ego position (model leg only: a resident record with a NaN position would send the tick's own front kernels through it,
    which no test of this project does): no history from then on, counted, no conflict."""
    odd = [(NAN, 0.0), (INF, 0.0)]
    r = run(cfg, DT, _cm(dm), [_approach(cfg, k, first=odd) for k in range(3)])
    assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 1, 0, 0, 0), (3, 2, 0, 0, 0)] and _min(r.conf[2]) == (4.0, 2, 2) and int(r.conf[2]["prev_n"][0]) == 3
    r = run(cfg, DT, _cm(dm), [_approach(cfg, 0), _t(cfg, (1.0, 0.5)), _t(cfg, (2.0, 0.5))])
    assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (3, 0, 0, 0, 0)]
    assert [int(c["prev_n"][0]) for c in r.conf] == [1, 0, 0] and (float(r.conf[2]["last_pos"]["x"][0]), float(r.conf[2]["last_pos"]["y"][0])) == (2.0, 0.5)
    if run.__self__.name == "model":
        r = run(cfg, DT, _cm(dm), [_approach(cfg, 0), _t(cfg, (NAN, 0.0), [(19.5, 0.0)]), _t(cfg, (0.0, 0.0), [(17.5, 0.0)]), _t(cfg, (0.0, 0.0), [(15.5, 0.0)])])
        assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 0, 0, 0, 1), (3, 0, 0, 0, 2), (4, 1, 0, 0, 2)] and _min(r.conf[3]) == (3.5, 3, 0)


KATS = [_kat_head_on_static_obstacle, _kat_graze_and_its_twin, _kat_contact_perpendicular_and_standstill, _kat_closing_speed_tie, _kat_warn_and_crit_ties,
        _kat_tit_warn_over_three_ticks, _kat_v_max_ties, _kat_one_tick_without_a_velocity, _kat_nan_infinity_and_no_obstacle]


@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, cfg1, kat):
    kat(dm, cfg1, _runner("model"))


def test_the_literals_of_the_known_answers():
    """The figures the cases above rest on, in Python floats."""
    assert 868 / (118 + math.sqrt(118.0 * 118.0 - 16 * 868.0)) == 7.0 and 29.5 * 29.5 - 2.25 == 868.0
    assert 100 / (40 + math.sqrt(40.0 * 40.0 - 16 * 100.0)) == 2.5
    y = 1.5 + 2.0 ** -30
    assert (100.0 + y * y) - 2.25 == 100 + 3 * 2.0 ** -30 and 1600.0 - 16 * ((100.0 + y * y) - 2.25) < 0
    y1 = math.nextafter(1.5, 2.0)
    assert (100.0 + y1 * y1) - 2.25 == 100.0, "one ulp of lateral offset is absorbed by the rounding of q: no twin"
    assert 0.5 + 0.75 + 1.0 == 2.25


def test_age_zero_takes_the_history_on_the_model(dm, cfg1):
    """Episodes on and EpisodeStats.age == 0 at tick 2: that tick has no conflict and counts one n_no_history_ticks, the ticks around
    it have theirs; without the stats every tick from 1 on has one."""
    ticks = _head_on(cfg1, 4)
    stats = [np.zeros(1, dm.EpisodeStats) for _ in ticks]
    for k, age in enumerate((0, 1, 0, 1)):                                  # (tick 0: k = 0, nothing to count)
        stats[k]["age"] = age
    r = cfb.ModelBackend().run(cfg1, DT, _cm(dm), ticks, stats)
    assert [_c(c) for c in r.conf] == [(1, 0, 0, 0, 0), (2, 1, 0, 0, 0), (3, 1, 0, 0, 1), (4, 2, 0, 0, 1)] and _min(r.conf[3]) == (6.0, 3, 0)
    r = cfb.ModelBackend().run(cfg1, DT, _cm(dm), ticks)
    assert _c(r.conf[3]) == (4, 3, 0, 0, 0)


def test_abi_mirror_defaults_and_null_handle(dm):
    lib = dm.load_library()
    assert [lib.pp_sizeof(k) for k in (45, 46)] == [dm.ConflictModel.itemsize, dm.ConflictScore.itemsize] == [32, 88]
    names = ("min_ttc", "max_drac", "tit_warn", "last_pos", "n_ticks", "n_conflict_ticks", "n_warn_ticks", "n_crit_ticks", "min_ttc_tick", "min_ttc_obs",
             "min_ttc_type", "first_crit_tick", "max_drac_tick", "n_no_history_ticks", "prev_off", "prev_n")
    assert dm.ConflictScore.names == names
    assert [dm.ConflictScore.fields[f][1] for f in names] == [0, 8, 16, 24, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84]
    assert dm.ConflictModel.names == ("ttc_warn", "ttc_crit", "v_max", "min_closing")
    d = dm.default_conflict()[0]
    assert (float(d["ttc_warn"]), float(d["ttc_crit"]), float(d["v_max"]), float(d["min_closing"])) == (3.0, 1.5, 70.0, 0.0)
    buf = np.zeros(1, dm.ConflictScore)
    assert lib.pp_set_conflict_score(None, dm.default_conflict().ctypes.data) == dm.PP_ERR_ARG
    assert lib.pp_get_conflict_score(None, buf.ctypes.data, 1) == dm.PP_ERR_ARG
    lib.pp_default_conflict(None)
    assert _is_start(cm.new_scores(dm.ConflictScore, 3))


# ---------------------------------------------------------------------------------------------------------------
# the device against the model
@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, cfg1, kat):
    kat(dm, cfg1, _runner("device"))


M_OBS = (0, 1, 63, 64, 65, 128, 129)


def _stride_case(cfg, m):
    """Three ticks of a standing ego with m obstacles: standing ones at (50 + j, 30) and - the LAST entry - the only closing one, the
    obstacle of _approach.  Every entry has a type of its own, 100 + j."""
    ticks = []
    for k in range(3):
        obs = [(50.0 + j, 30.0) for j in range(m)]
        if m:
            obs[-1] = (21.5 - 2.0 * k, 0.0)
        t = _t(cfg, (0.0, 0.0), obs)
        t.pool["type"][:m] = 100 + np.arange(m)
        ticks.append(t)
    return ticks


def _tie_case(cfg, a, b, m):
    """As _stride_case, but entries a and b are the closing obstacle, the same bytes but for the type: the lower index wins."""
    ticks = []
    for k in range(3):
        obs = [(50.0 + j, 30.0) for j in range(m)]
        obs[a] = obs[b] = (21.5 - 2.0 * k, 0.0)
        t = _t(cfg, (0.0, 0.0), obs)
        t.pool["type"][:m] = 100 + np.arange(m)
        ticks.append(t)
    return ticks


def _split_case(cfg):
    """71 entries; entry 2 drives 4 -> 3.5 -> 3 (vc 1: D 3.5: c = 10, b = -3.5, disc = 2.25, ttc = 10 / 5 = 2, drac = 1 / 4), entry 70 drives
    46.5 -> 41.5 -> 36.5 (vc 10: D 41.5: c = 1720, b = -415, disc = 225, ttc = 1720 / 430 = 4, drac = 100 / 80): at tick 1 the smallest TTC
    is on entry 2 and the largest DRAC on entry 70.  Tick 2: entry 2 at D 3: ttc 1.5, drac 1 / 3; entry 70 at D 36.5: ttc 3.5, drac 100 / 70."""
    ticks = []
    for k in range(3):
        obs = [(50.0 + j, 30.0) for j in range(71)]
        obs[2], obs[70] = (4.0 - 0.5 * k, 0.0), (46.5 - 5.0 * k, 0.0)
        t = _t(cfg, (0.0, 0.0), obs)
        t.pool["type"][:71] = 100 + np.arange(71)
        ticks.append(t)
    return ticks


def _edge_cases(cfg):
    cases = {f"m{m}": _stride_case(cfg, m) for m in M_OBS}
    cases.update(tie_0_64=_tie_case(cfg, 0, 64, 65), tie_63_64=_tie_case(cfg, 63, 64, 129), split=_split_case(cfg))
    return cases


_ALONE = {}


def _alone(dm, cfg):
    """Every wave-edge case alone on the device (once per process), with its literals."""
    if not _ALONE:
        for name, ticks in _edge_cases(cfg).items():
            r = cfb.DeviceBackend().run(cfg, DT, _cm(dm), ticks)
            c = r.conf[2]
            if name == "m0":
                assert _c(c) == (3, 0, 0, 0, 0) and _min(c) == (INF, -1, -1) and int(c["prev_n"][0]) == 0
            elif name.startswith("m"):
                m = int(name[1:])
                assert _c(c) == (3, 2, 0, 0, 0) and _min(c) == (4.0, 2, m - 1) and int(c["min_ttc_type"][0]) == 100 + m - 1 and _drac(c) == (16 / 32, 2)
            elif name.startswith("tie"):
                a = int(name.split("_")[1])
                assert _c(c) == (3, 2, 0, 0, 0) and _min(c) == (4.0, 2, a) and int(c["min_ttc_type"][0]) == 100 + a and _min(r.conf[1]) == (4.5, 1, a)
            else:
                assert _min(r.conf[1]) == (2.0, 1, 2) and _drac(r.conf[1]) == (1.25, 1) and _c(r.conf[1]) == (2, 1, 1, 0, 0)
                assert _min(c) == (1.5, 2, 2) and int(c["min_ttc_type"][0]) == 102 and _drac(c) == (100 / 70, 2) and _c(c) == (3, 2, 2, 1, 0)
                assert float(c["tit_warn"][0]) == 0.5 + 0.75 and int(c["first_crit_tick"][0]) == 2
            _ALONE[name] = r
    return _ALONE


@gpu
def test_wave_edges_alone(dm, cfg1):
    """0, 1, 63 | 64 | 65, 128 | 129 obstacles with the only closing entry the last one; an exact tie of the TTC on entries 0 and 64 and on
    63 and 64; the largest DRAC and the smallest TTC on different entries."""
    assert len(_alone(dm, cfg1)) == len(M_OBS) + 3


def _batch_off(ticks, s):
    return int(ticks[0].si["obs_off"][s])


@gpu
@pytest.mark.parametrize("n", [5, 300])
def test_a_scene_gives_the_same_bytes_alone_and_inside_a_batch(dm, cfg1, n):
    """5: one block of four waves and the first wave of the next; 300: 75 blocks.  Scene s is wave-edge case s % 10: the waves of a block
    have different trip counts.  The bytes are those of the scene alone, but for prev_off, which is the moved obs_off."""
    alone, cases = _alone(dm, cfg1), _edge_cases(cfg1)
    names = [list(cases)[(s + 2) % len(cases)] for s in range(n)]
    ticks = cfb.batch_ticks([cases[k] for k in names])
    r = cfb.DeviceBackend().run(cfg1, DT, _cm(dm), ticks)
    for k in range(3):
        for s, name in enumerate(names):
            got = r.conf[k][s:s + 1].copy()
            assert int(got["prev_off"][0]) == _batch_off(ticks, s)
            got["prev_off"] = 0
            assert got.tobytes() == alone[name].conf[k].tobytes(), (n, k, s, name)
            assert r.score[k][s].tobytes() == alone[name].score[k][0].tobytes(), (n, k, s, name)


def _crafted_run(dm, cfg, ticks, model, trace=None, after=None):
    """The ticks through one handle; model None: the conflict score is never set.  Returns, behind every tick, RolloutScore, the trace
    (headers, rings) or None, and the ConflictScore records or None."""
    import score_trace_backends as stb
    pl = cfb.open_planner(cfg, ticks, model, False, DT)
    if trace is not None:
        pl.set_score_trace(trace)
    pl.score_begin(DT)
    keep, scores, traces, confs = [], [], [], []
    on = model is not None
    for k, t in enumerate(ticks):
        stb.feed(pl, t, keep)
        scores.append(pl.rollout_score())
        traces.append(stb.read_all(pl, len(t.si)) if trace is not None else None)
        confs.append(pl.conflict_score() if on else None)
        if after and k in after:
            after[k](pl)
    pl.close()
    return scores, traces, confs


@gpu
def test_off_is_the_engine_without_it(dm, cfg1):
    """RolloutScore and the score-trace rings with the step on are those of a handle that never set it, byte for byte, and those of one
    that switched it off; behind pp_set_conflict_score(NULL) the records stay readable and no longer change; a handle that never set it
    answers the read with PP_ERR_STATE."""
    cases = _edge_cases(cfg1)
    ticks = cfb.batch_ticks([cases[k] + cases[k] for k in ("m65", "m0", "split", "m129", "tie_0_64")])
    tm = np.zeros(1, dm.ScoreTraceModel)
    tm["depth"], tm["post"], tm["trigger"], tm["near"], tm["brake"] = 4, 1, 3, 18.0, 6.0
    never_s, never_t, _ = _crafted_run(dm, cfg1, ticks, None, tm)
    on_s, on_t, on_c = _crafted_run(dm, cfg1, ticks, _cm(dm), tm)
    off_s, off_t, off_c = _crafted_run(dm, cfg1, ticks, _cm(dm), tm, {1: lambda pl: pl.set_conflict_score(None)})
    for k in range(len(ticks)):
        assert never_s[k].tobytes() == on_s[k].tobytes() == off_s[k].tobytes(), k
        for a, b in ((never_t[k], on_t[k]), (never_t[k], off_t[k])):
            assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])), k
    assert (never_t[5][0]["n_trigger_ticks"] > 0).any()                      # (the trace saw something: a clearance of 18 at tick 1)
    assert off_c[1].tobytes() == on_c[1].tobytes() and _c(off_c[1], 2) == (2, 1, 1, 0, 0)
    for k in range(2, len(ticks)):
        assert off_c[k].tobytes() == off_c[1].tobytes(), k
    assert _c(on_c[5], 2) == (6, 4, 4, 2, 0)              # (split twice: at tick 3 both movers jump back, inside v_max * dt: driving away, no conflict)
    pl = cfb.open_planner(cfg1, ticks, None, True, DT)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.conflict_score()
    pl.set_conflict_score(None)                           # (off is off, and still no set call)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.conflict_score()
    pl.close()


@gpu
def test_set_before_or_after_score_begin_and_only_while_scoring(dm, cfg1):
    """Legal on either side of pp_score_begin; the step runs only while the scorecard is on: ticks before pp_score_begin and behind
    pp_score_end leave the records alone; pp_score_begin puts them back on the starting values, and so does a second set call."""
    import score_trace_backends as stb
    ticks = _head_on(cfg1, 9)
    pl, keep = cfb.open_planner(cfg1, ticks, _cm(dm), False), []
    stb.feed(pl, ticks[0], keep)
    assert _is_start(pl.conflict_score())
    pl.score_begin(DT)
    for t in ticks[1:4]:
        stb.feed(pl, t, keep)
    c = pl.conflict_score()
    assert _c(c) == (3, 2, 0, 0, 0) and _min(c) == (6.0, 2, 0)                # (ttc 6.5 and 6 at the ego's x = 4 and 6)
    pl.score_end()
    stb.feed(pl, ticks[4], keep)
    assert pl.conflict_score().tobytes() == c.tobytes()
    pl.score_begin(DT)
    assert _is_start(pl.conflict_score())
    stb.feed(pl, ticks[5], keep), stb.feed(pl, ticks[6], keep)
    assert _min(pl.conflict_score()) == (4.5, 1, 0)                           # (x = 12: D = 19.5)
    pl.set_conflict_score(_cm(dm, warn=8.0, crit=4.0))                        # behind pp_score_begin: starts again, under the new model
    assert _is_start(pl.conflict_score())
    stb.feed(pl, ticks[7], keep), stb.feed(pl, ticks[8], keep)
    c = pl.conflict_score()
    assert _c(c) == (2, 1, 1, 1, 0) and _min(c) == (3.5, 1, 0) and float(c["tit_warn"][0]) == 2.25
    pl.close()


@gpu
def test_error_paths_change_nothing(dm, cfg1):
    import score_trace_backends as stb
    ticks = _head_on(cfg1, 4)
    pl, keep = cfb.open_planner(cfg1, ticks, _cm(dm, warn=8.0, crit=6.5), True, DT), []
    stb.feed(pl, ticks[0], keep), stb.feed(pl, ticks[1], keep)
    before = pl.conflict_score()
    bad = [dict(warn=0.0), dict(warn=-1.0), dict(warn=INF), dict(warn=NAN), dict(crit=0.0), dict(crit=-1.0), dict(crit=NAN), dict(crit=INF), dict(crit=3.5),
           dict(v_max=0.0), dict(v_max=-1.0), dict(v_max=INF), dict(v_max=NAN), dict(min_closing=-0.5), dict(min_closing=INF), dict(min_closing=NAN)]
    for kw in bad:
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_conflict_score(_cm(dm, **kw))
    lib, out = dm.load_library(), np.zeros(2, dm.ConflictScore)
    assert lib.pp_get_conflict_score(pl.h, None, 1) == dm.PP_ERR_ARG and lib.pp_get_conflict_score(pl.h, out.ctypes.data, 2) == dm.PP_ERR_ARG
    assert lib.pp_get_conflict_score(pl.h, out.ctypes.data, -1) == dm.PP_ERR_ARG
    assert pl.conflict_score().tobytes() == before.tobytes()
    stb.feed(pl, ticks[2], keep), stb.feed(pl, ticks[3], keep)                # the model in force is still the first one (warn 8, crit 6.5)
    c = pl.conflict_score()
    assert _c(c) == (4, 3, 3, 2, 0) and float(c["tit_warn"][0]) == 2.25 and int(c["first_crit_tick"][0]) == 2
    pl.close()


# ---------------------------------------------------------------------------------------------------------------
# closed loops: the model stepped over the device's own per-tick records, and the CPU loop of oracle and models
def _follow(dm, pl, cfg, model, n, ticks, conf, prev, scores, advance, episodes):
    """`ticks` x (tick, advance) on a streamed handle with the scorecard and the conflict score on; conf / prev / scores: the model's,
    stepped over SceneIn, snapshot, PlanOut, SceneState, flag words and EpisodeStats of every tick as the device had them; the device's
    records are held against conf behind EVERY tick.  Returns (the device's records behind every tick, EpisodeStats.age in front of every tick)."""
    import rollout_score_model as rsm
    dt, plan_p, got, ages = float(advance["dt"][0]), dm.pinned_empty(n, dm.PlanOut), [], []
    for t in range(ticks):
        sin, flags = pl.get_scene_in(), pl.ego_flags()
        stats = pl.episode_stats() if episodes else None
        pl.tick()
        assert pl.wait_tick(pl.fetch_async(plan_p)) == 0
        plan, state = np.array(plan_p), pl.get_state()
        total = int((sin["obs_off"] + sin["obs_n"]).max()) if len(sin) else 0
        now = pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, total) if total else np.zeros(1, dm.ObPoint)
        prev = cm.step(conf, prev, model, cfg, dt, sin, now, stats)
        rsm.fold(scores, cfg, dt, sin, plan, state, now, flags)
        got.append(pl.conflict_score()), ages.append(None if stats is None else stats["age"].copy())
        cfb.same(got[-1], conf, f"tick {t}: ConflictScore")
        pl.advance_async(advance)
        if episodes:                                                        # §4k 6.: a restart moves the totals' last ego to the start record
            after, out = pl.episode_stats(), pl.get_scene_in()
            for s in np.flatnonzero(after["n_episodes"] > stats["n_episodes"]):
                scores["last_pos"]["x"][s], scores["last_pos"]["y"][s] = out["loc"]["globalpoint"]["x"][s], out["loc"]["globalpoint"]["y"][s]
                scores["last_speed"][s] = out["loc"]["velocity"][s]
    cfb.same(pl.rollout_score(), scores, "RolloutScore behind the loop")
    return got, ages


LOOP_TICKS, APPROACH = 60, 8
_CPU = {}


def _contact_cpu(dm, oracle):
    """§4l's contact scenario on the CPU (tests/test_episode_spawn.py: oracle tick + route, spawn and traffic models), 60 advances, with
    the conflict model beside the scorecard model (once per process).  conf[t]: the records behind tick t."""
    if "contact" not in _CPU:
        import episode_model as epm
        import episode_spawn_model as esm
        import map_scenes as ms
        import rollout_score_model as rsm
        import route_model as rmod
        import test_episode_spawn as tes
        import test_traffic as tt
        import traffic_model as tm
        r, n = tes._loop_scene(dm), tt.F_N
        cfg, m, sc, adv, rm, model = r["cfg"], r["m"], r["sc"], dm.default_ego_model(), dm.default_route_model(), dm.default_conflict()
        dt, hw = float(adv["dt"][0]), 0.5 * float(cfg["Vehicle_Width"][0])
        si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(n, np.int32)
        tr = tm.Traffic(r["tracks"], r["pts"], r["act"], si["obs_off"])
        obs, _ = tr.place(sc["obs_pool"].copy(), None, 0.0)
        pin, pst = [si.copy()], [st.copy()]
        stats, sstats, scores = epm.new_stats(dm.EpisodeStats, n), esm.new_stats(dm.EpisodeSpawnStats, n), rsm.new_scores(dm.RolloutScore, n)
        conf, prev, per_tick = cm.new_scores(dm.ConflictScore, n), cm.new_prev(dm.ObPoint), []
        for t in range(LOOP_TICKS):
            plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
            prev = cm.step(conf, prev, model, cfg, dt, si, obs, stats)
            rsm.fold(scores, cfg, dt, si, plan, st, obs, flags)
            per_tick.append(conf.copy())
            q, f, _ = rmod.advance(dm, cfg, adv, rm, r["legs"], r["rf"], m, si, plan, st, flags)
            si, st, flags, _, _ = esm.step(r["em"], r["sp"], stats, sstats, pin, pst, si, q, f, st, obs, hw, None, None, scores)
            obs, _ = tr.place(obs, None, dt)
        _CPU["contact"] = dict(scene=r, conf=per_tick, scores=scores, stats=stats)
    return _CPU["contact"]


def _check_contact_loop(conf, scores, n, f_type):
    """What §4l's loop must show, on the records behind every tick.  Every ego's vehicle drives at it at 3 m/s.  The egos start at their
    cruising speed - 20 m at some 10 m/s closing: a TTC under 2 s from tick 1 on - and brake behind the vehicle first, so the TTC of a
    tick rises before it falls for good; min_ttc is a running minimum and never rises, and over the APPROACH tick by tick - the last
    APPROACH ticks up to the first contact - every tick brings a new smallest TTC, down to 0 in contact.  The first critical tick
    precedes the scorecard's first collision tick; the minimum names the actor's type; the tick behind the ending advance read a start
    record and has no history."""
    last = conf[-1]
    print("first_crit_tick", last["first_crit_tick"].tolist(), "\nfirst_collision_tick", scores["first_collision_tick"].tolist(), "\nmin_ttc", last["min_ttc"].tolist(),
          "\nmax_drac", np.round(last["max_drac"], 3).tolist(), "\nn_no_history_ticks", last["n_no_history_ticks"].tolist(), "n_conflict_ticks", last["n_conflict_ticks"].tolist())
    for s in range(n):
        hit = int(scores["first_collision_tick"][s])
        assert hit > APPROACH
        whole = [float(c["min_ttc"][s]) for c in conf]
        assert all(b <= a for a, b in zip(whole, whole[1:])), (s, whole)
        series = whole[hit - APPROACH:hit + 1]
        assert all(b < a for a, b in zip(series, series[1:])), (s, series)
        assert [int(conf[t]["min_ttc_tick"][s]) for t in range(hit - APPROACH, hit + 1)] == list(range(hit - APPROACH, hit + 1)), s
        assert series[-1] == 0.0 and series[-2] > 0.0 and float(last["min_ttc"][s]) == 0.0, (s, series)
        assert 0 <= int(last["first_crit_tick"][s]) < hit, (s, int(last["first_crit_tick"][s]), hit)
        assert int(last["min_ttc_type"][s]) == f_type and int(last["min_ttc_obs"][s]) == 0
        assert int(last["n_no_history_ticks"][s]) >= 1 and int(conf[hit]["n_no_history_ticks"][s]) == 0 and int(conf[hit + 1]["n_no_history_ticks"][s]) == 1
        assert float(conf[hit]["max_drac"][s]) > 0 and 0 < int(conf[hit]["max_drac_tick"][s]) < hit          # (in contact: no DRAC)


def test_contact_loop_on_the_cpu(dm, oracle):
    import test_traffic as tt
    L = _contact_cpu(dm, oracle)
    _check_contact_loop(L["conf"], L["scores"], tt.F_N, tt.F_TYPE)


def _against_cpu(got, want, what, tol=1e-6):
    """The device's records against the CPU loop's: every integer field equal, doubles within tol - the bar tests/test_score_trace.py sets
    for the same loop's ScoreTick doubles (the project's bar for oracle against device).  Returns the largest difference of a double."""
    worst = 0.0
    for f in got.dtype.names:
        a, b = got[f], want[f]
        if f == "last_pos":
            a, b = np.stack([a["x"], a["y"]]), np.stack([b["x"], b["y"]])
        if a.dtype.kind == "f":
            d = float(np.max(np.where(a == b, 0.0, np.abs(a - b))))
            worst = max(worst, d)
            assert d <= tol, (what, f, d)
        else:
            assert np.array_equal(a, b), (what, f, a.tolist(), b.tolist())
    return worst


# ---- §4k's ring egos with a timeout: the age = 0 rule ------------------------------------------------------------------------------------
RING_MAX_TICKS, RING_AHEAD_PTS, RING_OB_TYPE = 7, 20, 9


def _ring_scene(dm):
    """tests/test_episodes.py's 8 one-leg ring egos, every one with ONE own obstacle: a standing disc on its lane 40 points (20 m) ahead of
    its start.  Episodes end after 7 advances (TIMEOUT): a restart moves the ego back by what it drove in 0.7 s, 5.4 m at the most -
    inside v_max * dt = 7 m, so only the age = 0 rule takes that tick's history."""
    import route_scenes as rs
    import test_episodes as te
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, te.RING_N, seed=3, lanes=(1, 2), ids=(190, 215), legs=(1, 1), n_obs=1)
    si, pool = sc["scene_in"].copy(), sc["obs_pool"].copy()
    for s in range(te.RING_N):
        l = si["loc"][s]
        L = m["lanes"][m["road_first_lane"][int(l["road_num"]) - 1] + int(l["lane_num"]) - 1]
        p = m["points"][int(L["point_off"]) + int(l["id"][0]) + RING_AHEAD_PTS]
        o = pool[int(si["obs_off"][s])]
        o["x"], o["y"], o["radius"], o["type"] = p["x"], p["y"], 0.5, RING_OB_TYPE
    si["obs_n"] = 1
    return cfg, m, dict(sc, scene_in=si, obs_pool=pool), legs, rf, te._em(dm, 31, RING_MAX_TICKS)


def _ring_cpu(dm, oracle, ticks=30):
    if "ring" not in _CPU:
        import episode_model as epm
        import map_scenes as ms
        import route_model as rmod
        import test_episodes as te
        cfg, m, sc, legs, rf, em = _ring_scene(dm)
        adv, rm, model, n = dm.default_ego_model(), dm.default_route_model(), dm.default_conflict(), te.RING_N
        dt = float(adv["dt"][0])
        si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(n, np.int32)
        start_in, start_state, stats = si.copy(), st.copy(), epm.new_stats(dm.EpisodeStats, n)
        conf, prev, per_tick, ages = cm.new_scores(dm.ConflictScore, n), cm.new_prev(dm.ObPoint), [], []
        for t in range(ticks):
            plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, mot_pool=None), st, n_threads=8, want_grid=False)
            ages.append(stats["age"].copy())
            prev = cm.step(conf, prev, model, cfg, dt, si, sc["obs_pool"], stats)
            per_tick.append(conf.copy())
            q, f, _ = rmod.advance(dm, cfg, adv, rm, legs, rf, m, si, plan, st, flags)
            si, st, flags, _, _ = epm.step(em, stats, start_in, start_state, si, q, f, st)
        _CPU["ring"] = dict(conf=per_tick, ages=ages, ticks=ticks)
    return _CPU["ring"]


def _check_ring(conf, ages, n):
    """Every tick k > 0 that read a start record (age 0) counts one n_no_history_ticks and no conflict; every other tick k > 0 has the
    standing disc dead ahead of a driving ego: a conflict."""
    print("n_no_history_ticks", conf[-1]["n_no_history_ticks"].tolist(), "n_conflict_ticks", conf[-1]["n_conflict_ticks"].tolist(), "min_ttc", np.round(conf[-1]["min_ttc"], 3).tolist())
    for s in range(n):
        for t in range(1, len(conf)):
            d_hist = int(conf[t]["n_no_history_ticks"][s]) - int(conf[t - 1]["n_no_history_ticks"][s])
            d_conf = int(conf[t]["n_conflict_ticks"][s]) - int(conf[t - 1]["n_conflict_ticks"][s])
            assert (d_hist, d_conf) == ((1, 0) if int(ages[t][s]) == 0 else (0, 1)), (s, t, int(ages[t][s]), d_hist, d_conf)
        assert int(conf[-1]["n_no_history_ticks"][s]) == (len(conf) - 1) // RING_MAX_TICKS and int(conf[-1]["min_ttc_type"][s]) == RING_OB_TYPE


def test_ring_timeout_on_the_cpu(dm, oracle):
    import test_episodes as te
    L = _ring_cpu(dm, oracle)
    _check_ring(L["conf"], L["ages"], te.RING_N)


# ---- §4j's platoons under world traffic with following ----------------------------------------------------------------------------------------
PL_W, PL_SIZE, PL_K, PL_GAP, PL_SPEED = 4, 4, 3, 12.0, 1.5


def _platoon_scene(dm):
    """tests/test_world_traffic.py's platoons: 16 routed ring egos in 4 worlds of 4, 15 m apart, 3 peer slots and one own entry each: the
    world's vehicle, the platoon's leader: PL_GAP m ahead of the front ego at PL_SPEED (5.4 km/h; the egos start at 20 .. 30 km/h), following on.
    The gap is chosen on the CPU loop: the ring drives at 10 km/h, so all members brake alike at first and only the front ego, which closes on the
    vehicle, makes the ego behind it close on a peer, and so on down the platoon; at 25 m nothing reaches the rear ego within 60 advances, at 8 m
    the FRONT ego comes within ttc_crit of the vehicle."""
    import route_scenes as rs
    import test_world_traffic as twt
    import traffic_scenes as ts
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    m = rs.build_ring(dm)
    sc, legs, rf, wf, off, polylines, rows = twt._platoons(dm, cfg, m, PL_W, PL_SIZE, 1, PL_K)
    tracks, pts = ts.pack(dm, polylines)
    act = ts.actors(dm, [(here + 15.0 * (PL_SIZE - 1) + PL_GAP, PL_SPEED, w, 0, lane - 1, twt.P_TYPE, twt.P_RADIUS) for w, lane, here in rows])
    fmod = dm.default_fleet_model()
    fmod["max_peers"] = PL_K
    return dict(cfg=cfg, m=m, sc=sc, legs=legs, rf=rf, wf=wf, off=off, tracks=tracks, pts=pts, act=act, fmod=fmod, tf=dm.default_traffic_follow())


def _platoon_cpu(dm, oracle):
    if "platoon" not in _CPU:
        import fleet_model as fl
        import map_scenes as ms
        import rollout_score_model as rsm
        import route_model as rmod
        import world_traffic_model as wm
        r, n = _platoon_scene(dm), PL_W * PL_SIZE
        cfg, m, sc, adv, rm, model = r["cfg"], r["m"], r["sc"], dm.default_ego_model(), dm.default_route_model(), dm.default_conflict()
        dt, width, own = float(adv["dt"][0]), float(cfg["Vehicle_Width"][0]), np.ones(n, np.int64)
        tr = wm.World(r["tracks"], r["pts"], r["act"], r["wf"], r["off"], own)
        si, st, flags = ms.resolve(dm, m, sc["scene_in"].copy()), sc["state"].copy(), np.zeros(n, np.int32)
        si, obs, _ = fl.couple(r["fmod"], r["wf"], r["off"], own, si, sc["obs_pool"].copy())
        obs, _ = tr.place(obs, None, 0.0)
        scores, conf, prev, per_tick = rsm.new_scores(dm.RolloutScore, n), cm.new_scores(dm.ConflictScore, n), cm.new_prev(dm.ObPoint), []
        for t in range(LOOP_TICKS):
            plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, obs_pool=obs, mot_pool=None), st, n_threads=8, want_grid=False)
            prev = cm.step(conf, prev, model, cfg, dt, si, obs)
            rsm.fold(scores, cfg, dt, si, plan, st, obs, flags)
            per_tick.append(conf.copy())
            si, flags, _ = rmod.advance(dm, cfg, adv, rm, r["legs"], r["rf"], m, si, plan, st, flags)
            obs, _ = tr.step(obs, None, dt, r["tf"], si, flags, width)
            si, obs, _ = fl.couple(r["fmod"], r["wf"], r["off"], own, si, obs)
        _CPU["platoon"] = dict(scene=r, conf=per_tick, scores=scores)
    return _CPU["platoon"]


def _check_platoon(conf, scores):
    """The rear ego of every world (member 3) closes on the peer in front of it: its smallest TTC names a peer (DMPP_OB_PEER | scene).  Nobody
    comes within ttc_crit of anything, and nobody touches."""
    last = conf[-1]
    print("min_ttc", np.round(last["min_ttc"], 2).tolist(), "\nmin_ttc_type", [hex(int(t)) for t in last["min_ttc_type"]], "\nn_conflict_ticks", last["n_conflict_ticks"].tolist(),
          "n_warn_ticks", last["n_warn_ticks"].tolist(), "n_crit_ticks", last["n_crit_ticks"].tolist(), "\nmax_drac", np.round(last["max_drac"], 3).tolist())
    assert (last["n_crit_ticks"] == 0).all() and (last["first_crit_tick"] == -1).all() and (scores["n_collision_ticks"] == 0).all()
    assert (last["n_no_history_ticks"] == 0).all() and (last["n_ticks"] == LOOP_TICKS).all()
    for w in range(PL_W):
        rear = w * PL_SIZE + PL_SIZE - 1
        t = int(last["min_ttc_type"][rear])
        assert int(last["n_conflict_ticks"][rear]) > 0 and (t & cb.fl.OB_PEER) != 0 and w * PL_SIZE <= (t & ~cb.fl.OB_PEER) < rear, (w, hex(t))


def test_platoon_loop_on_the_cpu(dm, oracle):
    L = _platoon_cpu(dm, oracle)
    _check_platoon(L["conf"], L["scores"])


# ---- the same loops on the device -----------------------------------------------------------------------------------------------------
def _device_loop(dm, pl, cfg, n, episodes):
    """60 (tick, advance) with the scorecard and the conflict score (default model) on; closes the handle."""
    import rollout_score_model as rsm
    adv, model = dm.default_ego_model(), dm.default_conflict()
    pl.set_conflict_score(model)
    pl.score_begin(float(adv["dt"][0]))
    got, ages = _follow(dm, pl, cfg, model, n, LOOP_TICKS, cm.new_scores(dm.ConflictScore, n), cm.new_prev(dm.ObPoint), rsm.new_scores(dm.RolloutScore, n), adv, episodes)
    score = pl.rollout_score()
    pl.close()
    return got, ages, score


def _all_ticks_against_cpu(got, want, what):
    worst = max(_against_cpu(g, w, f"{what}, tick {t}") for t, (g, w) in enumerate(zip(got, want)))
    print(f"{what}: largest difference of a double, device against the CPU loop, over {len(want)} ticks: {worst}")


@gpu
def test_contact_loop_on_the_device(dm, oracle):
    """§4l's contact loop: the device equals the model on its own per-tick records byte for byte (held inside _follow, RolloutScore too), shows
    what the CPU loop shows, and equals the CPU loop in every integer field and within 1e-6 in every double, behind every tick."""
    import test_episode_spawn as tes
    import test_traffic as tt
    L = _contact_cpu(dm, oracle)
    got, _, score = _device_loop(dm, tes._planner(dm, L["scene"]), L["scene"]["cfg"], tt.F_N, True)
    _check_contact_loop(got, score, tt.F_N, tt.F_TYPE)
    _all_ticks_against_cpu(got, L["conf"], "contact loop")


@gpu
def test_ring_timeout_on_the_device(dm, oracle):
    """§4k's ring egos with max_ticks 7: the age = 0 rule on the device, against the model on the device's own EpisodeStats and against the CPU loop."""
    import test_episodes as te
    cfg, m, sc, legs, rf, em = _ring_scene(dm)
    pl = te._planner(dm, cfg, m, sc, 1)
    pl.set_route(legs, rf)
    pl.set_episodes(em)
    got, ages, _ = _device_loop(dm, pl, cfg, te.RING_N, True)
    L = _ring_cpu(dm, oracle)
    _check_ring(got[:L["ticks"]], ages[:L["ticks"]], te.RING_N)
    _all_ticks_against_cpu(got[:L["ticks"]], L["conf"], "ring with a timeout")


@gpu
def test_platoon_loop_on_the_device(dm, oracle):
    """§4j's platoons behind their leader under world traffic with following, peers and the world's vehicle in one slice."""
    import route_scenes as rs
    L = _platoon_cpu(dm, oracle)
    r, n = L["scene"], PL_W * PL_SIZE
    pl = dm.Planner(r["cfg"], device=0, **rs.caps(r["m"], n, 1 + PL_K, 0))
    pl.set_map(r["m"])
    pl.set_egos(r["sc"], with_motion=False)
    pl.set_state(r["sc"]["state"])
    pl.set_route(r["legs"], r["rf"])
    pl.set_fleet(r["wf"], r["fmod"])
    pl.set_traffic_follow(r["tf"])
    pl.set_world_traffic(r["tracks"], r["pts"], r["act"])
    got, _, score = _device_loop(dm, pl, r["cfg"], n, False)
    _check_platoon(got, score)
    _all_ticks_against_cpu(got, L["conf"], "platoon loop")


@gpu
def test_life_cycle_across_set_calls(dm):
    """pp_set_fleet, pp_set_traffic, pp_set_episodes, pp_set_grid_follow and pp_set_score_trace leave the records alone; pp_set_egos while
    scoring is on puts them back on the starting values, and the scorecard's with them."""
    import test_episode_spawn as tes
    import test_traffic as tt
    r, n, adv = tes._loop_scene(dm), tt.F_N, dm.default_ego_model()

    def fleet(pl):
        fm = dm.default_fleet_model()
        fm["max_peers"] = 0
        pl.set_fleet([0, n // 2, n], fm)

    calls = dict(fleet=fleet, traffic=lambda pl: pl.set_traffic(r["tracks"], r["pts"], r["act"]), episodes=lambda pl: pl.set_episodes(r["em"]),
                 grid_follow=lambda pl: pl.set_grid_follow(dm.default_grid_follow()), score_trace=lambda pl: pl.set_score_trace())
    for name, call in calls.items():
        pl = tt._planner(dm, r["cfg"], r["m"], r["sc"], 1)
        pl.set_route(r["legs"], r["rf"])
        pl.set_traffic(r["tracks"], r["pts"], r["act"])
        pl.set_conflict_score(dm.default_conflict())
        pl.score_begin(float(adv["dt"][0]))
        for _ in range(3):
            pl.tick()
            pl.advance_async(adv)
        pl.tick()                                                           # (a set call follows a tick, not a staged advance)
        before = pl.conflict_score()
        assert (before["n_ticks"] == 4).all() and (before["n_conflict_ticks"] > 0).all(), name
        call(pl)
        cfb.same(pl.conflict_score(), before, f"{name}: behind the call")
        pl.advance_async(adv)
        pl.tick()
        assert (pl.conflict_score()["n_ticks"] == 5).all(), name           # (and the step runs on)
        if name == "score_trace":                                           # new egos while scoring: the totals restart, and the records with them
            pl.set_egos(r["sc"], with_motion=False)
            assert _is_start(pl.conflict_score()) and (pl.rollout_score()["n_ticks"] == 0).all()
        pl.close()
