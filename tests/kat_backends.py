"""Two backends for the hand-derived known answers of tests/test_reference_kat.py: the CPU oracle and the HIP library.

Each known answer is written once against this interface and asserted on both.  Scalar functions go through the
oracle's entry points or the device's stand-alone stages (pp_geom_batch ops 0-2, pp_scalar_stage ops 0-2); everything
else is observed through whole ticks of a scene (plan, state, published refpath).

A scene tick runs `copies` copies of one scene.  With one copy the device runs a handle of one scene, ticked and read
back tick by tick.  With many (300: above the piped threshold of 256 scenes, grid stage on) the ticks are queued without
a host wait and read once at the end, so they go through the piped, grouped path (DMPP_TICK_GROUP); every copy must
agree bit for bit with the first, which the tests then hold to the hand value."""
import numpy as np

import dmpp_amd as dm
from parity_util import compare


def replicate(sc, copies):
    """`copies` copies of scene 0 of `sc`: lane, attribute and refpath pools shared, obstacles and state one set each."""
    if copies == 1:
        return sc
    n_obs = int(sc["n_obs"])
    si = np.repeat(sc["scene_in"][:1], copies)
    si["obs_off"] = np.arange(copies) * n_obs
    out = dict(sc, scene_in=si, state=np.repeat(sc["state"][:1], copies))
    for k in ("obs_pool", "mot_pool"):
        out[k] = np.tile(sc[k][:max(n_obs, 1)], copies)
    return out


def _same_copies(plan, st, tag):
    bad = []
    for k in range(1, len(st)):
        bad += compare(plan[k], plan[0], f"{tag} plan[{k}]", rtol=0, atol=0)
        bad += compare(st[k], st[0], f"{tag} state[{k}]", rtol=0, atol=0)
        if bad:
            break
    assert not bad, "copies of one scene disagree:\n" + "\n".join(bad[:10])


class Result:
    """Scene 0 after the last tick: PlanOut record, SceneState record, published DecisionOut.refpath."""
    def __init__(self, plan, st, refpath):
        self.plan, self.st, self.refpath = plan, st, refpath

    @property
    def dec(self):
        return self.plan["dec"]

    def around(self, k):
        """(Obs_flag, dis_lat, dis_lng) of corridor k: 0 F, 1 R, 2 LF, 3 LR, 4 RF, 5 RR (Decision.cpp:847-880)."""
        a = self.plan["around"][k]
        return int(a["Obs_flag"]), float(a["Ob_Pose"]["dis_lat"]), float(a["Ob_Pose"]["dis_lng"])

    def aim(self, which="far"):
        a = self.st["aimpoint_" + which]
        p = a["Aim_point"]
        return float(p["x"]), float(p["y"]), float(p["dir"]), int(a["Aim_id"])


class OracleBackend:
    name = "oracle"

    def __init__(self, oracle):
        self.o = oracle

    # ---- scalar functions ----
    def lat_dis(self, cfg, cur, pt, nxt):
        return self.o.GetLatDis(cfg, cur, pt, nxt)

    def road_angle(self, cfg, a, b):
        return self.o.GetRoadAngle(cfg, a, b)

    def angle_err(self, d1, d2):
        return self.o.GetAngleErr(d1, d2)

    def plan_judge(self, cfg, last_behavior, behavior, pos, lat, derr, rem):
        dec, loc, st = np.zeros(1, dm.DecisionOutPod), np.zeros(1, dm.LocationOut), np.zeros(1, dm.SceneState)
        dec["behavior"], loc["pos"] = behavior, pos
        st["path_lat_dis"], st["path_dir_err"], st["remain_dis"] = lat, derr, rem
        cause = np.zeros(1, np.int32)
        afresh = self.o.L.orc_UpdatePlanJudge(cfg.ctypes.data, dec.ctypes.data, loc.ctypes.data, last_behavior,
                                              st.ctypes.data, cause.ctypes.data)
        return int(afresh), int(cause[0])

    def speed(self, pos, ob_flag, lon, faraim, velocity_expect, init=(0.0, 0, 0.0)):
        dec, loc = np.zeros(1, dm.DecisionOutPod), np.zeros(1, dm.LocationOut)
        dec["velocity_expect"], loc["pos"] = velocity_expect, pos
        return self.o.SpeedPlanning(ob_flag, dec, loc, lon, 0.0, faraim, init=init)

    def radius(self, pts, near_id, front_id):
        return self.o.CalculateRadius(pts, near_id, front_id)

    # ---- scene ticks ----
    def run(self, cfg, sc, st, ticks=1, copies=1):
        """`ticks` ticks of `copies` copies of scene 0 from state st[0]; st[0] is updated. Returns a Result of scene 0."""
        rs = replicate(sc, copies)
        sts = np.repeat(st[:1], copies)
        plan, _, _ = self.o.plan_tick_batch(cfg, rs, sts, want_grid=False, n_ticks=ticks)
        _same_copies(plan, sts, self.name)
        st[0] = sts[0]
        return Result(plan[0], sts[0].copy(), self.o.last_refpath())    # the thread's last scene: a copy of scene 0


class HipBackend:
    name = "hip"

    def __init__(self):
        self._pl = {}

    def _planner(self, cfg, copies):
        key = (copies, cfg.tobytes())
        if key not in self._pl:
            self._pl[key] = dm.Planner(cfg, max_scenes=copies, max_obs_total=copies * 256)
        return self._pl[key]

    def _one(self, cfg):
        return self._planner(cfg, 1)

    # ---- scalar functions: the device's stand-alone stages ----
    def lat_dis(self, cfg, cur, pt, nxt):
        a, b, c = (np.array([p], dm.GlobalPoint2D) for p in (cur, pt, nxt))
        return float(self._one(cfg).geom_batch(0, a, b, c)[0])

    def road_angle(self, cfg, a, b):
        a, b = (np.array([p], dm.GlobalPoint2D) for p in (a, b))
        return float(self._one(cfg).geom_batch(1, a, b)[0])

    def angle_err(self, d1, d2):
        cfg = dm.default_config(128)
        cfg["grid_stage"] = 0
        return float(self._one(cfg).geom_batch(2, np.array([(d1, d2)], dm.GlobalPoint2D))[0])

    def plan_judge(self, cfg, last_behavior, behavior, pos, lat, derr, rem):
        out = self._one(cfg).scalar_stage(0, [last_behavior, behavior, pos, lat, derr, rem], n_out=2)
        return int(out[0]), int(out[1])

    def speed(self, pos, ob_flag, lon, faraim, velocity_expect, init=(0.0, 0, 0.0)):
        cfg = dm.default_config(128)
        cfg["grid_stage"] = 0
        out = self._one(cfg).scalar_stage(1, [pos, ob_flag, lon, faraim, velocity_expect, init[0], init[1], init[2]], n_out=3)
        return float(out[0]), int(out[1]), float(out[2])

    def radius(self, pts, near_id, front_id):
        cfg = dm.default_config(128)
        cfg["grid_stage"] = 0
        return float(self._one(cfg).scalar_stage(2, [near_id, front_id], last_Bpoints=pts, n_out=1)[0])

    # ---- scene ticks ----
    def run(self, cfg, sc, st, ticks=1, copies=1):
        if copies == 1:
            pl = self._one(cfg)
            pl.set_scenes(sc)
            pl.set_state(st[:1])
            for _ in range(ticks):
                pl.tick(sync=True)
            plan, sts = pl.get_plan(), pl.get_state()
        else:
            cfg = cfg.copy()
            cfg["grid_stage"] = 1                       # the piped path needs the grid stage (its plan outputs do not)
            pl = self._planner(cfg, copies)
            pl.set_scenes(replicate(sc, copies))
            pl.set_state(np.repeat(st[:1], copies))
            for _ in range(ticks):
                pl.tick()                               # queued: no host wait between the ticks
            plan, sts = pl.get_plan(), pl.get_state()
            _same_copies(plan, sts, self.name)
        st[0] = sts[0]
        return Result(plan[0], sts[0].copy(), pl.get_refpath(0, int(plan["dec"]["refpath_n"][0])))
