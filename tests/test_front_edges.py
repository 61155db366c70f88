"""The front chain (k_decision, k_planning) on the block edges of its parallel steps: the aim walk of SearchAimPoint, the
nearest-point reduction of GetVhclLocalState, junction path generation, the remaining-lane-change-length flags, the
junction front path at its 512-point cap and the width of the lateral sweep.

tests/front_scenes.py lists the cases and says which split each sits on and how its expected value follows by hand;
tests/front_model.py is the model (plain Python floats, every sum in index order).

CPU: the model against the hand values, the model against the oracle on every case and on a seeded random sweep.
GPU: every case on the device in three forms - alone in a handle created for one scene, all cases of a family as the scenes of one batch
(the ticks queued without a host wait) and the first case of each family as 300 copies through kat_backends.HipBackend (the
piped, grouped path).  Each form is held to the model (fields that come only from + - * / and sqrt: bit for bit, any NaN
for a NaN - see same()), to the oracle (parity_util.compare with its own tolerances: integers exactly) and to the other
forms (every field of PlanOut and SceneState and the published refpath, byte for byte)."""
import math
import struct

import numpy as np
import pytest

import front_model as fm
import front_scenes as fs
import kat_backends as kb
import lanechange_scenes as lcs
from parity_util import compare

FAMILY_NAMES = list(fs.FAMILIES)
FLAG_INDEX = dict(A60=0, B10=1, B15=2, B50=3)        # which of (A > 60, B > 10, B > 15, B > 50) a combination's decision reads
FLAG_PROBES = dict(A60=(480, 481), B10=(80, 81), B15=(120, 121), B50=(400, 401))    # exact runs either side of the threshold


@pytest.fixture(scope="module")
def cfgs(dm):
    on = dm.default_config(128)
    on["grid_stage"] = 0
    off = on.copy()
    off["decision_stage"] = 0
    return dict(on=on, off=off)


@pytest.fixture(scope="module")
def cases(dm, cfgs):
    return fs.all_cases(dm, cfgs)


def fields(plan, st, refpath):
    """the fields the model produces, from one scene's PlanOut / SceneState records and its published refpath"""
    aim = lambda a: (float(a["Aim_point"]["x"]), float(a["Aim_point"]["y"]), int(a["Aim_id"]))
    a0 = plan["around"][0]
    return dict(aim_far=aim(st["aimpoint_far"]), aim_near=aim(st["aimpoint_near"]), near_id=int(st["path_near_id"]),
                fid=int(st["path_front_near_id"]), remain=float(st["remain_dis"]), cause=int(st["afresh_cause"]),
                road=list(zip(plan["road_points"]["x"].tolist(), plan["road_points"]["y"].tolist())),
                refpath_n=int(plan["dec"]["refpath_n"]), refpath=list(zip(refpath["x"].tolist(), refpath["y"].tolist())),
                around0=(int(a0["Obs_flag"]), float(a0["Ob_Pose"]["dis_lat"]), float(a0["Ob_Pose"]["dis_lng"])),
                sweep=(int(plan["sweep_side"]), int(plan["sweep_index"])),
                outcome=(int(st["z_behavior"]), int(st["z_target_lanenum"]), int(st["z_light_status"]),
                         int(st["z_segment_lanechg_status"]), int(st["z_behavior_to_dlg"])))


def same(a, b):
    """Bit for bit: two floats are the same when their eight bytes are (so -0.0 is not 0.0), with one exception - any NaN
    equals any NaN, since the sign and payload of a NaN are not the reference's to define (the host's 0 * inf is a negative
    NaN, the device's a positive one)."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return (a != a and b != b) or struct.pack("d", a) == struct.pack("d", b)
    return type(a) == type(b) and a == b


def differences(got, want, keys=None):
    bad = []
    for k in (want if keys is None else keys):
        if k in want and k in got and not same(got[k], want[k]):
            g, w = got[k], want[k]
            if isinstance(w, list):
                j = next(i for i in range(max(len(g), len(w))) if i >= min(len(g), len(w)) or not same(g[i], w[i]))
                g, w = f"len {len(g)}, [{j}] = {g[j] if j < len(g) else None}", f"len {len(w)}, [{j}] = {w[j] if j < len(w) else None}"
            bad.append(f"{k}: {g} != {w}")
    return bad


def same_bytes(a, b, path=""):
    """field-by-field byte comparison of two records (padding skipped)"""
    if a.dtype.names:
        return [m for n in a.dtype.names if not n.startswith("_pad") for m in same_bytes(a[n], b[n], path + "." + n)]
    return [] if np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() else [path]


# ---- the oracle on every case (once per module, shared) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs(cases, oracle, cfgs):
    out = {}
    for cs in cases.values():
        for c in cs:
            st = c.st.copy()
            plan, _, _ = oracle.plan_tick_batch(cfgs[c.cfgk], c.sc, st, want_grid=False, n_ticks=c.ticks)
            out[repr(c)] = (plan[0], st[0], oracle.last_refpath())
    return out


@pytest.fixture(scope="module")
def flag_outcomes(cases, oracle_runs):
    """combination -> {False: outcome, True: outcome}: the third tick's behaviour with the combination's flag clear and set,
    taken from the two exact runs either side of its threshold (front_scenes.FLAG_COMBOS)"""
    by_name = {c.name: c for c in cases["flags"]}
    out = {}
    for combo, (lo, hi) in FLAG_PROBES.items():
        out[combo] = {False: fields(*oracle_runs[repr(by_name[f"{combo}_run{lo}"])])["outcome"],
                      True: fields(*oracle_runs[repr(by_name[f"{combo}_run{hi}"])])["outcome"]}
        assert out[combo][False] != out[combo][True], combo                   # the flag does decide go or keep
        assert out[combo][False][0] == 1 and out[combo][True][0] in (2, 3)    # keep lane | change left / right
    return out


def expected(cfgs, case, flag_outcomes):
    """what the model says of a case: the fields of model_tick for a one-tick case, the outcome its flag selects for a
    flags case, the hand-derived sweep for a sweep case"""
    if case.family == "flags":
        if case.combo is None:
            return {}
        return dict(outcome=flag_outcomes[case.combo][fs.model_flags(case)[FLAG_INDEX[case.combo]]])
    if case.family == "sweep":
        W = float(case.sc["scene_in"]["lanes"]["lane_width"][0])
        assert fm.sweep_candidates(W, float(cfgs["on"]["Vehicle_Width"][0])) == case.hand["n_cand"]
        return dict(sweep=case.hand["sweep"])
    return fs.model_tick(cfgs[case.cfgk], case)


# ---- CPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_model_matches_hand_values(cases, cfgs, family):
    n = 0
    for c in cases[family]:
        if c.family == "flags":
            got = dict(flags=fs.model_flags(c))
        elif c.family == "sweep":            # (the model has the candidate count; `sweep` is a known answer for oracle and device)
            got = dict(n_cand=fm.sweep_candidates(float(c.sc["scene_in"]["lanes"]["lane_width"][0]), 1.8))
        else:                                # (`around0` likewise: SearchObstacle has its own model and tests)
            got = fs.model_tick(cfgs[c.cfgk], c)
            if getattr(c, "nan_remain", False):
                assert math.isnan(got["remain"]), c
        keys = [k for k in c.hand if k in got]
        bad = differences(got, c.hand, keys)
        assert not bad, f"{c}: " + "; ".join(bad)
        n += len(keys)
    assert n > 0


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_model_matches_oracle(cases, cfgs, oracle_runs, flag_outcomes, family):
    for c in cases[family]:
        got = fields(*oracle_runs[repr(c)])
        bad = differences(got, expected(cfgs, c, flag_outcomes)) + differences(got, c.hand, ("around0", "sweep"))
        assert not bad, f"{c}: " + "; ".join(bad)


def test_flag_outcomes_follow_the_model_flag_only(cases, oracle_runs, flag_outcomes):
    """Within one out_lanes / map_attr combination the third tick's behaviour is a function of the one flag it reads: every
    case - whatever its other three flags - lands on the outcome of the exact probe with the same flag."""
    seen = {(combo, f): 0 for combo in FLAG_INDEX for f in (False, True)}
    for c in cases["flags"]:
        if c.combo is None:
            continue
        f = fs.model_flags(c)[FLAG_INDEX[c.combo]]
        assert fields(*oracle_runs[repr(c)])["outcome"] == flag_outcomes[c.combo][f], c
        seen[c.combo, f] += 1
    assert all(seen.values()), seen


def _random_lane(rng, n, nan_p):
    step = 0.02 * 100 ** rng.random() * rng.uniform(0.5, 1.0, n)           # log-uniform: as many maps at 5 cm as at 1 m
    heading = np.cumsum(rng.normal(0, 0.01, n))
    xy = np.stack([100.0 + np.cumsum(step * np.cos(heading)), 200.0 + np.cumsum(step * np.sin(heading))], 1)
    if rng.random() < nan_p:
        xy[rng.integers(0, n), rng.integers(0, 2)] = math.nan
    return xy


def test_random_sweep_model_against_oracle(dm, oracle, cfgs, flag_outcomes, capsys):
    """Seeded random lanes and refpaths (spacing 0.02 - 2 m, 2 - 1500 points, NaN points, ids from below 0 to past the end)
    through every model function, against the oracle's whole tick."""
    rng = np.random.default_rng(2222)
    on, off = cfgs["on"], cfgs["off"]
    blocks = {2: 0, 3: 0}                    # lanes whose walk / run reached a second / third block of 256 segments
    hit = dict(road=0, left=0, right=0, junction=0, local=0, mean=0, flags=0, jfront=0, aim_dis=0)

    def reached(n_seg):
        for b in blocks:
            blocks[b] += n_seg > 256 * (b - 1)

    def check(case, cfg, want=None):
        st = case.st.copy()
        plan, _, _ = oracle.plan_tick_batch(cfg, case.sc, st, want_grid=False, n_ticks=case.ticks)
        got = fields(plan[0], st[0], oracle.last_refpath())
        want = fs.model_tick(cfg, case) if want is None else want
        bad = differences(got, want)
        assert not bad, f"{case.name}: " + "; ".join(bad)
        return want

    for k in range(360):
        kind = ("road", "left", "right", "junction", "flags", "jfront")[k % 6]
        n = int(rng.choice([rng.integers(2, 40), rng.integers(40, 600), rng.integers(600, 1501)]))
        if kind in ("road", "left", "right"):
            xy = _random_lane(rng, n, 0.25)
            ident = int(rng.integers(-6, n + 6))
            other = _random_lane(rng, int(rng.integers(2, 1501)), 0.0)
            beh = dict(road=1, left=2, right=3)[kind]
            kw = dict(road=dict(cur_xy=xy), left=dict(cur_xy=None, left=xy, right=other), right=dict(cur_xy=None, right=xy, left=other))[kind]
            sc, st = fs.road_scene(dm, off, behavior=beh, target=dict(road=None, left=1, right=3)[kind], ids=ident, **kw)
            sc["scene_in"]["loc"]["velocity"] = float(rng.choice([0.0, 18.0, 25.0, 60.0]))
            want = check(fs.Case("random", f"{kind}{k} n {n} id {ident}", "off", sc, st), off)
            if want["aim_far"][2] != fs.STALE_FAR[3]:
                reached(want["aim_far"][2] - max(ident, 0) + 1)
            hit[kind] += 1
            hit["aim_dis"] += 1
        elif kind == "junction":
            pos = 1 + k // 6 % 2
            sc = lcs.make_junction_scene(dm, off, pos)
            fs.own_decision(sc)
            fs.put_ref(dm, sc, _random_lane(rng, n, 0.25), refpath_n=int(rng.integers(0, n + 20)))
            st = sc["state"].copy()
            fs.mark_aims(st)
            st["aimpoint_far"]["Aim_id"] = int(rng.integers(-3, 400))
            path = _random_lane(rng, 200, 0.25)
            g = sc["scene_in"]["loc"]["globalpoint"]
            g["x"], g["y"] = path[int(rng.integers(0, 200))] + rng.normal(0, 0.05, 2)
            st["last_Bpoints"]["x"], st["last_Bpoints"]["y"] = path[:, 0], path[:, 1]
            st["count"], st["his_behavior"], st["path_near_id"] = 1, int(rng.integers(0, 2)), int(rng.integers(-5, 260))
            want = check(fs.Case("random", f"junction{k} n {n}", "off", sc, st), off)
            reached(want["aim_far"][2] + 1)
            hit["junction"] += 1
            hit["local"] += 1
            hit["mean"] += "na" in want
        elif kind == "flags":
            combo = list(FLAG_INDEX)[k // 6 % 4]
            # The flag shows only in the third tick's behaviour, and only if the 120-point front corridor reaches the obstacle
            # 10 m ahead: so spacing 0.1 - 2 m here (not from 0.02), NaN points only past the corridor, and a draw whose ego has
            # fewer than 120 points ahead (ids near and past the lane end) is generated but has no outcome to compare.
            step = 0.2 * 10 ** rng.random()
            xs = 100.0 + np.cumsum(step * rng.uniform(0.5, 1.0, n))
            ident = int(rng.integers(-6, n + 6))
            if rng.random() < 0.2 and max(ident, 0) + 125 < n:
                xs[rng.integers(max(ident, 0) + 125, n)] = math.nan
            ahead = np.zeros(n, np.uint8)
            run = int(rng.integers(0, n))
            ahead[:run] = fs.FLAG_COMBOS[combo]["ahead"]
            if rng.random() < 0.5:
                ahead[:int(rng.integers(0, run + 1))] = 1
            sc = fs.flag_scene(dm, on, combo, xs, ahead, id_cur=ident)
            case = fs.Case("random", f"flags{k} {combo} n {n} id {ident} run {run}", "on", sc, ticks=3)
            if n - 1 - max(ident, 0) >= 120:
                flag = fs.model_flags(case)[FLAG_INDEX[combo]]
                check(case, on, dict(outcome=flag_outcomes[combo][flag]))
                reached(min(run, n - 1 - max(ident, 0)))
                hit["flags"] += 1
        else:
            pos = 1 + k // 6 % 2
            sc = lcs.make_junction_scene(dm, on, pos)
            fs.put_lanes(dm, sc, cur=_random_lane(rng, n, 0.1))
            fs.put_ref(dm, sc, _random_lane(rng, int(rng.integers(0, 700)), 0.1))
            sc["scene_in"]["loc"]["id"][:] = int(rng.integers(-6, n + 6))
            sc["scene_in"]["obs_n"] = 0
            want = check(fs.Case("random", f"jfront{k} pos {pos} n {n}", "on", sc), on)
            reached(want["aim_far"][2] + 1 if want["refpath_n"] >= 3 else 0)
            hit["jfront"] += 1
    with capsys.disabled():
        print(f"\nrandom sweep: {hit}; lanes that reached a second block of 256: {blocks[2]}, a third: {blocks[3]}")
    assert all(hit.values()), hit
    assert blocks[2] >= 20 and blocks[3] >= 10


# ---- GPU ---------------------------------------------------------------------------------------------------------------
class Device:
    """Per configuration a one-scene handle and a batch handle (created once per module), kat_backends.HipBackend
    for the 300 copies; every result is computed once and kept."""
    MAX_SCENES = 64

    def __init__(self, dm, cfgs, cases):
        self.dm, self.cfgs, self.cases = dm, cfgs, cases
        self.pl, self.hip, self.done = {}, kb.HipBackend(), {}

    def planner(self, cfgk, n):
        """the handle for n = 1 scene (pools large enough for the longest lanes) or for a batch of up to MAX_SCENES"""
        if (cfgk, n) not in self.pl:
            self.pl[cfgk, n] = self.dm.Planner(self.cfgs[cfgk], device=0, max_scenes=n, max_obs_total=n * 4,
                                               max_lane_pts_total=n * 2400, max_ref_pts_total=n * 700)
        return self.pl[cfgk, n]

    def _read(self, pl, cfgk, k, plan, st):
        n = int(plan["dec"]["refpath_n"][k])
        return plan[k], st[k], pl.get_refpath(k, n) if cfgk == "on" else np.zeros(0, self.dm.GlobalPoint2D)

    def run(self, family, form):
        """{case name: (PlanOut, SceneState, refpath)} of a family in one form"""
        if (family, form) in self.done:
            return self.done[family, form]
        out = {}
        cs = self.cases[family]
        if form == "alone":
            for c in cs:
                pl = self.planner(c.cfgk, 1)
                pl.set_scenes(c.sc)
                pl.set_state(c.st[:1])
                for _ in range(c.ticks):
                    pl.tick(sync=True)
                out[c.name] = self._read(pl, c.cfgk, 0, pl.get_plan(), pl.get_state())
        elif form == "batch":
            for cfgk in ("on", "off"):
                group = [c for c in cs if c.cfgk == cfgk]
                if not group:
                    continue
                assert len(group) <= self.MAX_SCENES and len({c.ticks for c in group}) == 1
                sc = fs.concat_scenes(group)
                pl = self.planner(cfgk, self.MAX_SCENES)
                pl.set_scenes(sc)
                pl.set_state(sc["state"])
                for _ in range(group[0].ticks):
                    pl.tick()                                                  # queued: no host wait between the ticks
                plan, st = pl.get_plan(), pl.get_state()
                for k, c in enumerate(group):
                    out[c.name] = self._read(pl, cfgk, k, plan, st)
        else:
            c = cs[0]
            r = self.hip.run(self.cfgs[c.cfgk], c.sc, c.st.copy(), c.ticks, 300)   # (asserts that the 300 copies agree)
            out[c.name] = (r.plan, r.st, r.refpath if c.cfgk == "on" else np.zeros(0, self.dm.GlobalPoint2D))
        self.done[family, form] = out
        return out


@pytest.fixture(scope="module")
def device(dm, cfgs, cases):
    return Device(dm, cfgs, cases)


FORMS = pytest.mark.parametrize("form", ["alone", "batch", "x300"])
FAMILY = pytest.mark.parametrize("family", FAMILY_NAMES)


@pytest.mark.gpu
@FORMS
@FAMILY
def test_device_matches_model(device, cases, cfgs, flag_outcomes, family, form):
    got = device.run(family, form)
    for c in cases[family]:
        if c.name in got:
            f = fields(*got[c.name])
            bad = differences(f, expected(cfgs, c, flag_outcomes)) + differences(f, c.hand, ("around0", "sweep"))
            assert not bad, f"{c} {form}: " + "; ".join(bad)


@pytest.mark.gpu
@FORMS
@FAMILY
def test_device_matches_oracle(device, cases, oracle_runs, family, form):
    got = device.run(family, form)
    for c in cases[family]:
        if c.name in got:
            plan, st, ref = got[c.name]
            plan_o, st_o, ref_o = oracle_runs[repr(c)]
            bad = compare(plan, plan_o, "plan") + compare(st, st_o, "state")
            if c.cfgk == "on":
                bad += compare(ref, ref_o, "refpath", rtol=0, atol=0)
            assert not bad, f"{c} {form}:\n" + "\n".join(bad[:10])


@pytest.mark.gpu
@FAMILY
def test_forms_agree(device, cases, family):
    alone, batch, x300 = (device.run(family, form) for form in ("alone", "batch", "x300"))
    assert set(alone) == set(batch) == {c.name for c in cases[family]} and list(x300) == [cases[family][0].name]
    for name, other in [(n, batch) for n in alone] + [(n, x300) for n in x300]:
        (p, s, r), (p2, s2, r2) = alone[name], other[name]
        bad = same_bytes(p, p2, "plan") + same_bytes(s, s2, "state") + ([] if r.tobytes() == r2.tobytes() else ["refpath"])
        assert not bad, f"{family}/{name}: alone and {'batch' if other is batch else 'x300'} differ in {bad[:8]}"
