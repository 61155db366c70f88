"""The front chain in two launches per tick ("front chain").

A. The obstacle snapshot at the head of k_decision: where the snapshot and Decision share a stream the tick runs
k_decision<true>, whose workgroups write their scene's snapshot slice themselves, and k_effective_obstacles is not launched.  DMPP_FRONT_SNAPSHOT=0 (read at pp_create) keeps the separate launch on every path.

Every case runs the same ticks on a default handle and on a knob-off handle and compares PlanOut, SceneState, GridOut, the
published refpath and the snapshot set itself (PP_BUF_OBS_NOW) byte for byte; the snapshot is also held to the oracle's
effective_obstacles byte for byte, and the tick to the oracle's tick (parity_util.compare, as tests/test_gpu_parity.py does).
Which form ran is read from the launch counts of the kernel table: the fused form records no k_effective_obstacles.

B. k_planning on a tick that is not a scene's first (count != 0) runs the aim walk of SearchAimPoint and GetVhclLocalState side
by side on two waves; the first tick (count == 0) keeps the serial order.  The cases below sit on what that split can get wrong
(PLAN_CASES); each runs three ticks with the ego moved between them.  CPU: the oracle against tests/front_model.py on every
case and tick.  GPU: the device alone, as one batch and as 300 copies (piped, grid stage on), after every tick against the
oracle (parity_util.compare) and against the model fed the device's own state before that tick, bit for bit."""
import math
import os
import struct

import numpy as np
import pytest

import front_scenes as fs
import kat_backends as kb
import lanechange_scenes as lcs
from parity_util import compare

START_TICK = 7                       # a start state whose tick is not 0: the snapshot is pool + motion * dyn_dt * tick
# strides of the 256-thread copy loop (0, 1, 255 | 256 | 257) and the 512-record LDS cap of the corridor searches (513)
OBS_COUNTS = [0, 1, 255, 256, 257, 513]
FORMS = dict(one=(1, 0), batch=(5, 0), x300=(300, 64))          # scenes, grid side (0: grid stage off)


def _planner(dm, cfg, sc, fused, env=None):
    n = len(sc["scene_in"])
    env = dict(env or {}, **({} if fused else {"DMPP_FRONT_SNAPSHOT": "0"}))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pl = dm.Planner(cfg, max_scenes=n, max_obs_total=max(len(sc["obs_pool"]), 1))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pl.set_profile(1)
    return pl


def _config(dm, grid, dynamic=1, decision=1):
    cfg = dm.default_config(grid or 128)
    cfg["grid_stage"] = 1 if grid else 0
    cfg["dynamic_obstacles"] = dynamic
    cfg["decision_stage"] = decision
    return cfg


def _scenes(dm, cfg, seed, n, n_obs):
    sc = dm.gen_scenes(cfg, seed, n, n_obs, junction_every=3)
    sc["state"]["tick"] = START_TICK
    if n_obs:
        assert float(cfg["dyn_dt"][0]) != 0 and (sc["mot_pool"]["vx"] != 0).any() and (sc["mot_pool"]["vy"] != 0).any()
    return sc


def _covered(sc):
    """the pool slots some scene's slice covers (the others are never written)"""
    m = np.zeros(len(sc["obs_pool"]), bool)
    for off, k in zip(sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"]):
        m[int(off):int(off) + int(k)] = True
    return m


def _results(dm, pl, sc):
    plan, st = pl.get_plan(), pl.get_state()
    out = dict(plan=plan, state=st)
    if pl.cfg["grid_stage"][0]:
        out["grid"] = pl.get_grid_out()
    if pl.cfg["decision_stage"][0]:
        out["refpath"] = np.concatenate([pl.get_refpath(s, int(plan["dec"]["refpath_n"][s])) for s in range(0, pl.n, max(pl.n // 5, 1))])
    out["snapshot"] = pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, len(sc["obs_pool"]))[_covered(sc)]
    return out


def _run(dm, cfg, sc, ticks, fused, env=None):
    pl = _planner(dm, cfg, sc, fused, env)
    pl.set_scenes(sc)
    pl.set_state(sc["state"])
    for _ in range(ticks):
        pl.tick()                                   # queued: no host wait between the ticks
    out = _results(dm, pl, sc)
    out["snapshot_launches"] = pl.kernel_ms()["k_effective_obstacles"][1]
    pl.close()
    return out


def _same_bytes(a, b, tag):
    for k in ("plan", "state", "grid", "refpath", "snapshot"):
        assert (k in a) == (k in b), (tag, k)
        if k in a:
            assert a[k].tobytes() == b[k].tobytes(), f"{tag}: {k} differs between the fused and the separate-launch run: " + "; ".join(compare(a[k], b[k], k, rtol=0, atol=0)[:5])


def _against_oracle(oracle, cfg, sc, ticks, got, tag):
    st = sc["state"].copy()
    grid = bool(cfg["grid_stage"][0])
    plan_o, gout_o, _ = oracle.plan_tick_batch(cfg, sc, st, n_threads=8, want_grid=grid, n_ticks=ticks)
    bad = compare(got["plan"], plan_o, "plan") + compare(got["state"], st, "state")
    if grid:
        bad += compare(got["grid"]["status"], gout_o["status"], "grid.status")
        keep = (gout_o["status"] != 3) & (gout_o["status"] != 7)      # OVERFLOW / COST_RANGE: only the status is specified
        bad += compare(got["grid"][keep], gout_o[keep], "grid")
    assert not bad, tag + "\n" + "\n".join(bad[:20])
    # the snapshot of the last tick: every scene started at START_TICK, so the whole pool moved by the same time
    now = oracle.effective_obstacles(cfg, sc["obs_pool"], sc["mot_pool"], START_TICK + ticks - 1)[_covered(sc)]
    assert got["snapshot"].tobytes() == now.tobytes(), tag + ": snapshot set differs from the oracle's"


def _pair(dm, oracle, cfg, sc, ticks, tag, fused_expected=True, env=None):
    a = _run(dm, cfg, sc, ticks, True, env)
    b = _run(dm, cfg, sc, ticks, False, env)
    assert b["snapshot_launches"] == ticks, tag
    assert a["snapshot_launches"] == (0 if fused_expected else ticks), tag
    _same_bytes(a, b, tag)
    _against_oracle(oracle, cfg, sc, ticks, a, tag)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k,n_obs", list(enumerate(OBS_COUNTS)))
def test_fused_snapshot_equals_separate_launch(dm, oracle, form, k, n_obs):
    n, grid = FORMS[form]
    cfg = _config(dm, grid)
    ticks = 1 + k % 4                              # 1 to 4 ticks: the tick counter moves the obstacles
    sc = _scenes(dm, cfg, 7000 + k, n, n_obs)
    got = _pair(dm, oracle, cfg, sc, ticks, f"{form}, {n_obs} obstacles, {ticks} ticks")
    if n_obs:                                      # the obstacles did move: the snapshot is not the pool
        assert got["snapshot"].tobytes() != sc["obs_pool"][_covered(sc)].tobytes()


def _share_slices(sc, n_obs):
    """scenes 2j and 2j + 1 share one slice; every fourth scene's slice starts half a slice later and overlaps two others partly"""
    k = np.arange(len(sc["scene_in"]))
    sc["scene_in"]["obs_off"] = (k // 2) * n_obs + np.where(k % 4 == 3, n_obs // 2, 0)
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("form,n_obs", [("batch", 40), ("batch", 300), ("x300", 40)])
def test_shared_and_overlapping_slices(dm, oracle, form, n_obs):
    """k_validate_scenes checks bounds only, so slices may overlap: every writer of a slot stores the same bytes (same pool
    entry, same tick), and a workgroup reads only slots it has itself written and waited for."""
    n, grid = FORMS[form]
    cfg = _config(dm, grid)
    sc = _share_slices(_scenes(dm, cfg, 7100, n, n_obs), n_obs)
    off = sc["scene_in"]["obs_off"]
    assert off[0] == off[1] and off[2] < off[3] < off[2] + n_obs < off[3] + n_obs <= len(sc["obs_pool"])
    _pair(dm, oracle, cfg, sc, 3, f"shared slices, {form}, {n_obs} obstacles")


@pytest.mark.gpu
def test_decision_off_keeps_the_separate_launch(dm, oracle):
    cfg = _config(dm, 0, decision=0)
    sc = _scenes(dm, cfg, 7200, 5, 24)
    _pair(dm, oracle, cfg, sc, 2, "decision off", fused_expected=False)


@pytest.mark.gpu
def test_small_batch_with_the_grid_keeps_the_separate_launch(dm, oracle):
    """8 scenes with the grid stage on are not piped: the snapshot stays on the handle's stream, Decision and Planning fork
    beside the grid engine."""
    cfg = _config(dm, 64)
    sc = _scenes(dm, cfg, 7300, 8, 24)
    _pair(dm, oracle, cfg, sc, 3, "8 scenes, grid on", fused_expected=False)


@pytest.mark.gpu
@pytest.mark.parametrize("grid,env", [(0, None), (64, {"DMPP_PIPELINE_MIN": "1"})])
def test_streamed_ticks_snapshot_the_adopted_pool(dm, oracle, grid, env):
    """4 scenes, 3 ticks, a new obstacle pool staged between ticks (pp_update_async): the tick after adoption snapshots the new
    pool, and every tick's fetch equals the knob-off run.  Grid off: one stream; grid on with DMPP_PIPELINE_MIN=1: piped.
    A streamed handle keeps the separate launch (its searches wait for single ticks), so the first tick - enqueued
    with the first update already staged - is the only one the default handle could have fused, and does not."""
    n, n_obs, T = 4, 24, 3
    cfg = _config(dm, grid)
    sc = _scenes(dm, cfg, 7400, n, n_obs)
    rng = np.random.default_rng(74)
    pools = []
    for t in range(T):
        p = sc["obs_pool"].copy()
        p["x"] += rng.uniform(-0.5, 0.5, len(p)) * (t + 1)
        p["y"] += rng.uniform(-0.5, 0.5, len(p)) * (t + 1)
        pools.append(p)
    runs = []
    for fused in (True, False):
        pl = _planner(dm, cfg, sc, fused, env)
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
        plans = [dm.pinned_empty(n, dm.PlanOut) for _ in range(T)]
        grids = [dm.pinned_empty(n, dm.GridOut) if grid else None for _ in range(T)]
        pinned = [dm.pinned_copy(p) for p in pools]
        mot = dm.pinned_copy(sc["mot_pool"])
        ids, snaps = [], []
        for t in range(T):
            pl.update_async(None, pinned[t], mot)
            pl.tick()
            ids.append(pl.fetch_async(plans[t], grids[t]))
            if t == T - 1:
                for i in ids:
                    assert pl.wait_tick(i) == 0
            if t in (0, T - 1):                    # (reading the set is a host wait: after the first tick and after the last)
                snaps.append(pl.read_device(dm.BUF_OBS_NOW, dm.ObPoint, n * n_obs))
        assert pl.kernel_ms()["k_effective_obstacles"][1] == T
        runs.append(dict(plans=[np.array(p) for p in plans], grids=[np.array(g) for g in grids if g is not None],
                         snaps=snaps, state=pl.get_state()))
        pl.close()
    a, b = runs
    for k in ("plans", "grids", "snaps"):
        for t, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.tobytes() == y.tobytes(), f"streamed {k}[{t}] differs between the fused and the separate-launch run"
    assert a["state"].tobytes() == b["state"].tobytes()
    for snap, t in zip(a["snaps"], (0, T - 1)):    # the adopted pool of that tick, moved by that tick's counter
        assert snap.tobytes() == oracle.effective_obstacles(cfg, pools[t], sc["mot_pool"], START_TICK + t).tobytes(), t
    st = sc["state"].copy()
    for t in range(T):
        plan_o, gout_o, _ = oracle.plan_tick_batch(cfg, dict(sc, obs_pool=pools[t]), st, want_grid=bool(grid))
        bad = compare(a["plans"][t], plan_o, "plan")
        if grid:
            bad += compare(a["grids"][t]["status"], gout_o["status"], "grid.status")
        assert not bad, f"streamed tick {t}\n" + "\n".join(bad[:20])
    assert not compare(a["state"], st, "state")


# ---- B: k_planning, the aim walk beside the local state -----------------------------------------------------------------
TICKS = 3
X300 = ("K256", "K513", "lane_end_600", "beh2_default_from_current_lane", "beh3_id_negative", "junction_3_points_found",
        "mid_199", "K257_count_255", "pos1_K256_decision_on")          # the cases that also run as 300 copies


@pytest.fixture(scope="module")
def cfgs(dm):
    on = dm.default_config(128)
    on["grid_stage"] = 0
    off = on.copy()
    off["decision_stage"] = 0
    return dict(on=on, off=off)


def _later_tick(c, y, count=1, behavior=1):
    """a case of front_scenes made a later tick: count != 0 and a last path of 200 points at 0.25 m from the ego along its lane"""
    c.st["count"], c.st["his_behavior"] = count, behavior
    c.st["last_Bpoints"]["x"], c.st["last_Bpoints"]["y"] = fs.X_EGO + 0.25 * np.arange(200), y
    return c


def plan_cases(dm, cfgs):
    """name -> Case.  Every case but the two `decision_on` ones starts with count != 0, i.e. on the side-by-side path."""
    aim = {c.name: c for c in fs.aim_cases(dm, cfgs)}
    side = {c.name: c for c in fs.aim_side_cases(dm, cfgs)}
    local = {c.name: c for c in fs.local_cases(dm, cfgs)}
    gen = {c.name: c for c in fs.gen_cases(dm, cfgs)}
    out = {}
    # the stop on segment 254 | 255 | 256 of the walk (0-based: the last two of the first block of 256 and the first of the
    # second, which the block loop continues after the join), their strict-> twins, and a stop in the third block
    for name in ("K255", "K256", "K257", "K255_twin", "K256_twin", "K257_twin", "K513", "K769"):
        out[name] = _later_tick(aim[name], fs.Y2)
    # never found: the fallback of every branch (current lane's end; the left-lane quirk, read from the current lane and fenced
    # into it; the right lane's end; the refpath's end on a NaN sum)
    for name in ("lane_end_255", "lane_end_256", "lane_end_600", "nan_in_second_block", "nan_one_past_stop"):
        out[name] = _later_tick(aim[name], fs.Y2)
    for name, y in (("beh2_K256", 200.0), ("beh2_default_from_current_lane", 200.0), ("beh2_default_fenced_into_current_lane", 200.0),
                    ("beh3_K256", 192.5), ("beh3_left_n306", 192.5), ("beh3_left_n307", 192.5)):
        out[name] = _later_tick(side[name], y, behavior=int(side[name].sc["scene_in"]["dec"]["behavior"][0]))
    for name in ("pos1_nan_inside_na", "pos2_nan_inside_na", "pos2_na65", "pos1_na300"):
        out[name] = gen[name]                                                     # (count 1 already)
    # i0 < 0 (kinds 1 and 2 walk from 0, kind 3 does not walk and the stale aim stays), i0 = iend and i0 > iend (an empty walk)
    for name in ("id_negative", "id_at_lane_end", "id_past_lane_end"):
        out[name] = _later_tick(aim[name], fs.Y2)
    E = lcs.EGO_ID
    right = fs.line(fs.ego_lane(fs.walk_xs(fs.X_EGO, 30, 3)), 192.5)
    sc, st = fs.road_scene(dm, cfgs["off"], None, 3, 3, right=right, left=fs.line(100.0 + 0.5 * np.arange(E + 31), 200.0), ids=-3)
    out["beh3_id_negative"] = _later_tick(fs.Case("plan", "beh3_id_negative", "off", sc, st,
                                                  hand=dict(aim_far=fs.STALE_FAR[:2] + fs.STALE_FAR[3:])), 192.5, behavior=3)
    # a junction refpath of 2 points (no walk: the stale aim stays), 3 and 4 points, the stop found (pos 2: sum > 14) and not
    for n, xs, hand in ((2, (0.0, 20.0), None), (3, (0.0, 5.0, 25.0), 1), (3, (0.0, 1.0, 2.0), 2), (4, (0.0, 20.0, 21.0, 22.0), 0),
                        (4, (0.0, 1.0, 2.0, 3.0), 3)):
        sc = lcs.make_junction_scene(dm, cfgs["off"], 2)
        fs.own_decision(sc)
        fs.put_ref(dm, sc, fs.line(fs.X_EGO + np.array(xs), 200.0))
        sc["scene_in"]["loc"]["velocity"] = 0.0
        st = sc["state"].copy()
        fs.mark_aims(st)
        found = hand is not None and hand < n - 1
        name = f"junction_{n}_points" + ("" if hand is None else "_found" if found else "_not_found")
        want = dict(aim_far=fs.STALE_FAR[:2] + fs.STALE_FAR[3:]) if hand is None else dict(aim_far=(fs.X_EGO + xs[hand], 200.0, hand))
        out[name] = _later_tick(fs.Case("plan", name, "off", sc, st, hand=want), 200.0)
    # the local state: nearest point 199, fid >= 199 (an empty remain), nothing within 9999 m (the member keeps its value), a NaN
    # point in the last path before / behind the minimum and on either side of fid
    for name in ("mid_199", "mid_198", "mid_192", "mid_191", "mid_190", "mid_0", "all_beyond_9999", "all_nan_prev_250",
                 "nan_30_min_100", "nan_150_min_100", "nan_107_min_100", "nan_108_min_100", "tie_63_64_at_3_4"):
        out[name] = local[name]
    # count 255: this tick is a later one, the next has count 0 (255 + 1 wraps) and takes the serial order again, the third is
    # a later one once more; and first ticks (count 0) at a junction with the decision stage on, which go on to two later ticks
    c = _later_tick({c.name: c for c in fs.aim_cases(dm, cfgs)}["K257"], fs.Y2, count=255)
    c.name = "K257_count_255"
    out[c.name] = c
    for name in ("pos1_K256_decision_on", "pos2_K256_decision_on"):
        out[name] = side[name]
    for name, c in out.items():
        c.name = name
        fs.assert_fenced(c.sc)
    assert set(X300) <= set(out)
    return out


def _moved(sc, t):
    """the scene of tick t: the ego t lane points and (0.25 t, t / 32) m further on"""
    si = sc["scene_in"].copy()
    si["loc"]["id"] += t
    si["loc"]["globalpoint"]["x"] += 0.25 * t
    si["loc"]["globalpoint"]["y"] += 0.03125 * t
    return dict(sc, scene_in=si)


def fields(plan, st, refpath):
    """the fields the model produces, from one scene's PlanOut / SceneState records and its published refpath"""
    aim = lambda a: (float(a["Aim_point"]["x"]), float(a["Aim_point"]["y"]), int(a["Aim_id"]))
    return dict(aim_far=aim(st["aimpoint_far"]), aim_near=aim(st["aimpoint_near"]), near_id=int(st["path_near_id"]),
                fid=int(st["path_front_near_id"]), remain=float(st["remain_dis"]), cause=int(st["afresh_cause"]),
                road=list(zip(plan["road_points"]["x"].tolist(), plan["road_points"]["y"].tolist())),
                refpath_n=int(plan["dec"]["refpath_n"]), refpath=list(zip(refpath["x"].tolist(), refpath["y"].tolist())))


def same(a, b):
    """bit for bit; any NaN equals any NaN (sign and payload of a NaN are not the reference's to define)"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return (a != a and b != b) or struct.pack("d", a) == struct.pack("d", b)
    return type(a) == type(b) and a == b


def differences(got, want, keys):
    bad = []
    for k in keys:
        if k in want and not same(got[k], want[k]):
            g, w = got[k], want[k]
            if isinstance(w, list):
                j = next(i for i in range(max(len(g), len(w))) if i >= min(len(g), len(w)) or not same(g[i], w[i]))
                g, w = f"[{j}] = {g[j] if j < len(g) else None}", f"[{j}] = {w[j] if j < len(w) else None}"
            bad.append(f"{k}: {g} != {w}")
    return bad


def same_bytes(a, b, path=""):
    """field-by-field byte comparison of two records (padding skipped)"""
    if a.dtype.names:
        return [m for n in a.dtype.names if not n.startswith("_pad") for m in same_bytes(a[n], b[n], path + "." + n)]
    return [] if np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() else [path]


MODEL_KEYS = ("aim_far", "aim_near", "near_id", "fid", "remain", "cause", "road", "refpath_n", "refpath")


def _model(cfgs, c, sc_t, st_before):
    """front_model's tick of case c on the scene of that tick from the state before it (a one-record array)"""
    return fs.model_tick(cfgs[c.cfgk], fs.Case(c.family, c.name, c.cfgk, sc_t, st_before))


@pytest.fixture(scope="module")
def pcases(dm, cfgs):
    return plan_cases(dm, cfgs)


@pytest.fixture(scope="module")
def oracle_ticks(pcases, oracle, cfgs):
    """name -> per tick (scene of the tick, oracle state before, PlanOut, state after, refpath), computed once"""
    out = {}
    for name, c in pcases.items():
        st = c.st.copy()
        rows = []
        for t in range(TICKS):
            sc_t, before = _moved(c.sc, t), st.copy()
            plan, _, _ = oracle.plan_tick_batch(cfgs[c.cfgk], sc_t, st, want_grid=False)
            rows.append((sc_t, before, plan[0].copy(), st[0].copy(), oracle.last_refpath().copy()))
        out[name] = rows
    return out


def test_plan_cases_cover_both_orders(pcases, oracle_ticks):
    counts = {name: [int(r[1]["count"][0]) for r in rows] for name, rows in oracle_ticks.items()}
    assert counts["K257_count_255"] == [255, 0, 1]
    assert counts["pos1_K256_decision_on"] == [0, 1, 2] and counts["K256"] == [1, 2, 3]
    assert sum(c[0] != 0 for c in counts.values()) >= 40


def test_oracle_matches_model_and_hand_values(pcases, oracle_ticks, cfgs):
    """CPU: the oracle's own values on every case and tick are the model's, bit for bit, and on the first tick the hand values"""
    for name, c in pcases.items():
        for t, (sc_t, before, plan, after, ref) in enumerate(oracle_ticks[name]):
            got = fields(plan, after, ref)
            want = _model(cfgs, c, sc_t, before)
            bad = differences(got, want, MODEL_KEYS)
            if t == 0:
                bad += differences(got, c.hand, ("aim_far", "aim_near", "near_id", "fid", "remain", "cause", "refpath_n"))
            assert not bad, f"{name} tick {t}: " + "; ".join(bad)
            if getattr(c, "nan_remain", False) and t == 0:
                assert math.isnan(got["remain"]), name


class PlanDevice:
    """every form computed once: name -> per tick (state before, PlanOut, state after, refpath) of scene 0 / the case's scene"""
    def __init__(self, dm, cfgs, pcases):
        self.dm, self.cfgs, self.cases, self.pl, self.done = dm, cfgs, pcases, {}, {}

    def planner(self, cfg, n, n_obs=4):
        key = (cfg.tobytes(), n)
        if key not in self.pl:
            self.pl[key] = self.dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs, max_lane_pts_total=max(n, 4) * 2400,
                                           max_ref_pts_total=max(n, 4) * 700)
        return self.pl[key]

    def _read(self, pl, cfgk, k, plan, st):
        n = int(plan["dec"]["refpath_n"][k])
        return plan[k].copy(), st[k].copy(), pl.get_refpath(k, n) if cfgk == "on" else np.zeros(0, self.dm.GlobalPoint2D)

    def run(self, form):
        if form in self.done:
            return self.done[form]
        out = {}
        if form == "alone":
            for name, c in self.cases.items():
                pl = self.planner(self.cfgs[c.cfgk], 1)
                pl.set_scenes(c.sc)
                pl.set_state(c.st[:1])
                rows = []
                for t in range(TICKS):
                    before = pl.get_state()[:1].copy()
                    pl.set_scenes(_moved(c.sc, t))
                    pl.tick(sync=True)
                    rows.append((before,) + self._read(pl, c.cfgk, 0, pl.get_plan(), pl.get_state()))
                out[name] = rows
        elif form == "batch":
            for cfgk in ("on", "off"):
                group = [c for c in self.cases.values() if c.cfgk == cfgk]
                assert 0 < len(group) <= 64
                pl = self.planner(self.cfgs[cfgk], 64)
                for t in range(TICKS):
                    sc = fs.concat_scenes([fs.Case(c.family, c.name, cfgk, _moved(c.sc, t), c.st) for c in group])
                    pl.set_scenes(sc)
                    if t == 0:
                        pl.set_state(sc["state"])
                    before = pl.get_state()
                    pl.tick()
                    plan, st = pl.get_plan(), pl.get_state()
                    for k, c in enumerate(group):
                        out.setdefault(c.name, []).append((before[k:k + 1].copy(),) + self._read(pl, cfgk, k, plan, st))
        else:
            for name in X300:
                c = self.cases[name]
                cfg = self.cfgs[c.cfgk].copy()
                cfg["grid_stage"] = 1                       # the piped path needs the grid stage (its plan outputs do not)
                pl = self.planner(cfg, 300, max(int(c.sc["n_obs"]), 1))
                rows = []
                for t in range(TICKS):
                    pl.set_scenes(kb.replicate(_moved(c.sc, t), 300))
                    if t == 0:
                        pl.set_state(np.repeat(c.st[:1], 300))
                    before = pl.get_state()
                    pl.tick()
                    plan, st = pl.get_plan(), pl.get_state()
                    for k in (1, 150, 299):                 # the copies agree
                        assert not same_bytes(plan[k], plan[0], "plan") + same_bytes(st[k], st[0], "state"), (name, t, k)
                    rows.append((before[:1].copy(),) + self._read(pl, c.cfgk, 0, plan, st))
                out[name] = rows
        self.done[form] = out
        return out


@pytest.fixture(scope="module")
def pdevice(dm, cfgs, pcases):
    return PlanDevice(dm, cfgs, pcases)


PLAN_FORMS = pytest.mark.parametrize("form", ["alone", "batch", "x300"])


@pytest.mark.gpu
@PLAN_FORMS
def test_planning_matches_model(pdevice, pcases, cfgs, form):
    """after each of the three ticks: the device against the model fed the device's own state before that tick, bit for bit"""
    got = pdevice.run(form)
    assert set(got) == (set(X300) if form == "x300" else set(pcases))
    for name, rows in got.items():
        c = pcases[name]
        for t, (before, plan, after, ref) in enumerate(rows):
            f = fields(plan, after, ref)
            bad = differences(f, _model(cfgs, c, _moved(c.sc, t), before), MODEL_KEYS)
            if t == 0:
                bad += differences(f, c.hand, ("aim_far", "aim_near", "near_id", "fid", "remain", "cause", "refpath_n"))
            assert not bad, f"{name} {form} tick {t}: " + "; ".join(bad)


@pytest.mark.gpu
@PLAN_FORMS
def test_planning_matches_oracle(pdevice, pcases, oracle_ticks, form):
    got = pdevice.run(form)
    for name, rows in got.items():
        for t, (before, plan, after, ref) in enumerate(rows):
            _, _, plan_o, st_o, ref_o = oracle_ticks[name][t]
            bad = compare(plan, plan_o, "plan") + compare(after, st_o, "state")
            if pcases[name].cfgk == "on":
                bad += compare(ref, ref_o, "refpath", rtol=0, atol=0)
            assert not bad, f"{name} {form} tick {t}:\n" + "\n".join(bad[:10])


@pytest.mark.gpu
def test_planning_forms_agree(pdevice, pcases):
    """every field of PlanOut and SceneState and the published refpath, byte for byte, between the three forms"""
    alone, batch, x300 = (pdevice.run(form) for form in ("alone", "batch", "x300"))
    for other, tag in ((batch, "batch"), (x300, "x300")):
        for name, rows in other.items():
            for t, ((_, p, s, r), (_, p2, s2, r2)) in enumerate(zip(alone[name], rows)):
                bad = same_bytes(p, p2, "plan") + same_bytes(s, s2, "state") + ([] if r.tobytes() == r2.tobytes() else ["refpath"])
                assert not bad, f"{name} tick {t}: alone and {tag} differ in {bad[:8]}"
