"""Case-split scenes for the block- and wave-parallel steps of the front chain (k_decision, k_planning), and the adapter
that runs tests/front_model.py on a scene.  Used by tests/test_front_edges.py on the oracle and on the device.

Built on lanechange_scenes.make_scene / make_junction_scene (three straight lanes along +x, lane 2 at y = 196.25) with
lanes and refpaths of their own length placed in the scene's pools.  Every length is an exact binary fraction, so each
expected index follows by hand (stated per family below and kept in Case.hand); the model only confirms it.

family      function / split the cases sit on                                  how the expected value follows
----------  -----------------------------------------------------------------  ------------------------------------------
aim         block_aim_walk: 256 segments per pass, the in-order sum carried     velocity 0 -> faraim 10, stop at the first
            across passes; serial_walk: blocks of eight, its NaN branch.        sum > 14.  Spacing h = 2^-6 after a first
            K = 1 | 7 8 9 (eight-wide block) | 255 256 257 258 (first pass |    segment L0 = 14 - (K-1) h + h/2: the sum on
            second) | 511 512 513 (second | third) | 769 (fourth), each with    segment K is 14 + h/2, Aim_id = i0 + K - 1.
            the twin L0 = 14 - (K-1) h whose sum on segment K is exactly 14     Twin: the > is strict, Aim_id = i0 + K.
            (strict >).  Lane ends after 255 | 256 | 257 | 600 segments         No stop: Aim_id = n - 1 (Planning.cpp:426).
            (default branch), stop on the last segment, i0 < 0, i0 = iend,      i0 >= iend: nothing written, the marked
            i0 > iend, NaN before / after the stop, an infinite coordinate.     stale aims stay.  NaN sum: never > : default.
aim-side    the same walk at its other three call sites: behaviour 2 (left     as above on the left / right lane or the
            lane, default read from the CURRENT lane, Planning.cpp:464-467),    refpath (pos 1: faraim 15, pos 2: 10; i0 = 0
            behaviour 3 (bound min(left_n, right_n), :478), pos 1 / 2 on the    so Aim_id = K - 1); left_n = 50 + K cuts the
            refpath with the decision stage off and once on (k_decision's      right-lane walk one short of its stop:
            published copy).  Stops 255 | 256 | 257.                            default = the right lane's last point.
local       GetVhclLocalState in k_planning: four indices per lane             ego at the origin, path x = 6 + 0.25 i, the
            (lane + 64 k), wave_first_min, serial_sum's blocks of eight.        tied points at distance 5 exactly ((3,4),
            Ties inside one lane (5, 70), (70, 134), (70, 5, 198), across       (4,3), (-3,4)): the lowest index wins.
            lanes (63, 64), (191, 192), a high lane's low index against a low   remain = (199 - fid) * 0.25 for fid <= 199,
            lane's high one (199, 135), ends (0, 199).  mid 0 63 64 | 182 183   else 0 (a single moved point; 9 | 8 | 7 | 2 | 1 | 0
            184 | 189 190 191 192 | 198 199.  A NaN point before / behind the   segments: both sides of the block of eight); NaN
            minimum and on either side of fid; all NaN with path_near_id 7      remain iff the NaN point is >= fid; nothing
            and 250; every point beyond 9999 m.                                 below 9999: the previous id, fenced to 199.
gen         junction PathPlanning: na clamp, wave_cumlen, mean_point's         decision stage off, his_behavior 0 -> cause
            binary search against the specification's linear scan.  na = 0 1    1, always replans.  Stop offset na by the L0
            2 3 | 63 64 65 (one wave) | 199 200, Aim_id 300 clamped to 200,     construction (K = na + 1).  200 points at
            refpath_n below a stale Aim_id; zero-length segments at the         2^-4: s_k = L k / 199 = k / 16 = cum[k]
            start, middle, end; all points equal; cum meeting the resampling    exactly, the scan takes q = k - 1, r = 1:
            abscissa exactly; a NaN point inside the first na.                  road_points = the first 200 refpath points.
flags       the remaining-lane-change-length flags of k_decision: parallel     spacing 2^-3: 10 | 15 | 50 | 60 m are 80 |
            sum, rounding bound, in-order fallback over blocks of 256.  Runs    120 | 400 | 480 segments, sums exact, so the
            479 480 481 (A > 60), 399 400 401 (B > 50), 119 120 121 (B > 15),   parallel sum can equal the threshold and the
            79 80 81 (B > 10); irregular spacing 63 64 65 | 255 256 257 | 511   fallback walks two blocks.  flag = run *
            512 513; A ending in block 0 | 1 | 2 while B runs on; A ended and   2^-3 > threshold, seen as go | keep on the
            attr 1 again on the first segment of the next block; NaN in B's     third tick (period 1600, obstacle 10 m ahead).
            part only; ego 0 1 2 points before the lane end; a run ending on    A ends at 100, attr 1 again at 256: A = 12.5 m
            the lane's last segment after 256 and 512 segments.                 (68 m with the later run).  Irregular triples
                                                                                and the runs to the lane end are scaled so that
                                                                                the threshold falls inside the last segment:
                                                                                one segment fewer clears the flag.  NaN in B
                                                                                after A = 62.5 m: A set, every B flag clear.
jfront      junction branch of k_decision: front path capped at 512 points,    path at 2^-3 from x = 125: n1 = min(cur_n -
            four-wave search, published refpath.  pos 1: cur_n - Id_Cur 400     Id, 512), n2 = min(ref_n, 512 - n1) (pos 2:
            511 512 513 x ref_n 0 1 112 200; pos 2: ref_n - Id_Inter 452 453    n2 = min(60, 512 - n1)); an obstacle on the
            512 600, Id_Inter >= ref_n.  Every case twice: an obstacle on the    last vertex is found at (n - 1) / 8 m, one
            last vertex, and with a second one on vertex 0.                     on vertex 0 at 0 m.
sweep       lateral sweep of k_decision on its third tick: n_cand 0 | 1 | 8.   n_cand = #{i < 8 : i < (W - 1.8) / 0.6}: W
                                                                                1.8 -> 0, 2.1 -> 1, 6.3 -> 8 (left 7 clears)

Index fences (checked in csrc/kernels_r.hpp before any case went to the device): block_aim_walk starts at max(i0, 0) and
reads i + 1 <= iend only; iend is n - 1 of the lane walked (behaviour 3: min(left_n, right_n) - 1); the behaviour-2 default
index is clamped into the current lane; refpath_n is clamped to ref_n and 512 with the decision stage off; na is clamped to
[0, min(200, refpath_n)]; Id_Cur / Id_Inter are floored at 0 and a count max(n - Id, 0) is taken; the remaining-length loop
runs base < cur_n - 1 from max(Id_Cur, 0); path_near_id is clamped to [0, 199], fid to 199 before it indexes.  No case
relies on an unfenced read; assert_fenced() checks that every slice of a scene lies inside the pools it ships."""
import math

import numpy as np

import front_model as fm
import lanechange_scenes as lcs

H = 2.0 ** -6
Y2 = 196.25
X_EGO = 125.0
STALE_FAR, STALE_NEAR = (1234.5, -7.25, 33.0, 17), (4321.5, 7.25, 11.0, 71)


class Case:
    def __init__(self, family, name, cfgk, sc, st=None, ticks=1, hand=None):
        self.family, self.name, self.cfgk, self.sc, self.ticks = family, name, cfgk, sc, ticks
        self.st = sc["state"].copy() if st is None else st
        self.hand = hand or {}

    def __repr__(self):
        return f"{self.family}/{self.name}"


# ---- building blocks ---------------------------------------------------------------------------------------------------
def walk_xs(x0, n_seg, K, limit=14.0, twin=False, h=H):
    """n_seg + 1 abscissae from x0: a first segment L0 = limit - (K - 1) h (+ h / 2 unless twin), then spacing h.  The sum on
    segment K (1-based) is limit + h / 2 (twin: exactly limit).  Every value is a multiple of 2^-7 below 2^9: exact."""
    L0 = limit - (K - 1) * h + (0.0 if twin else h / 2)
    assert L0 > 0
    return np.concatenate([[x0], x0 + L0 + h * np.arange(n_seg)])


def line(xs, y=Y2):
    xs = np.asarray(xs, float)
    return np.stack([xs, np.full(len(xs), y)], 1)


def ego_lane(tail_xs):
    """lane points 0..49 at 0.5 m (x = 100 + 0.5 k) and then tail_xs, whose first value is the ego point 50 (x = 125)"""
    return np.concatenate([100.0 + 0.5 * np.arange(lcs.EGO_ID), tail_xs])


def put_lanes(dm, sc, cur=None, left=None, right=None, attr=None):
    """The scene's three lanes replaced by arrays of (x, y) of any length (None: the 320-point lane stays); attr: the
    current lane's lanechg_attribute bytes.  The pools are rebuilt as cur | left | right."""
    n = dm.GEN_LANE_PTS
    lv = sc["scene_in"]["lanes"]
    old, old_attr = sc["lane_pool"], sc["attr_pool"]
    pts, att, off = [], [], 0
    for slot, (xy, key) in enumerate(((cur, "cur"), (left, "left"), (right, "right"))):
        if xy is None:
            a, b = old[slot * n:(slot + 1) * n].copy(), old_attr[slot * n:(slot + 1) * n].copy()
            cnt = int(lv[key + "_n"][0])
        else:
            a = np.zeros(len(xy), dm.GlobalPoint3D)
            a["x"], a["y"] = xy[:, 0], xy[:, 1]
            b = np.full(len(xy), int(lv["lanechg_attribute"][0]), np.uint8)
            cnt = len(xy)
        if slot == 0 and attr is not None:
            b = np.asarray(attr, np.uint8)
            assert len(b) == len(a)
        pts.append(a), att.append(b)
        lv[key + "_off"], lv[key + "_n"] = off, cnt
        off += len(a)
    sc["lane_pool"], sc["attr_pool"] = np.concatenate(pts), np.concatenate(att)
    return sc


def put_ref(dm, sc, xy, refpath_n=None):
    xy = np.asarray(xy, float).reshape(-1, 2)
    pool = np.zeros(max(len(xy), 1), dm.GlobalPoint2D)
    pool["x"][:len(xy)], pool["y"][:len(xy)] = xy[:, 0], xy[:, 1]
    sc["ref_pool"] = pool
    si = sc["scene_in"]
    si["ref_off"], si["ref_n"] = 0, len(xy)
    si["dec"]["refpath_n"] = len(xy) if refpath_n is None else refpath_n
    return sc


def own_decision(sc, behavior=1, target=None):
    d = sc["scene_in"]["dec"]
    d["behavior"], d["refpath_n"], d["velocity_expect"] = behavior, 0, 10.0
    d["target_lanenum"] = sc["scene_in"]["loc"]["lane_num"][0] if target is None else target


def mark_aims(st):
    for which, (x, y, d, k) in (("aimpoint_far", STALE_FAR), ("aimpoint_near", STALE_NEAR)):
        st[which]["Aim_point"]["x"], st[which]["Aim_point"]["y"], st[which]["Aim_point"]["dir"] = x, y, d
        st[which]["Aim_id"] = k


def assert_fenced(sc):
    """every slice of every scene lies inside the pools the scene ships (reads stay in the pools the scene owns)"""
    nl, nr, no = len(sc["lane_pool"]), len(sc["ref_pool"]), len(sc["obs_pool"])
    assert len(sc["attr_pool"]) == nl
    for si in sc["scene_in"]:
        lv = si["lanes"]
        for k in ("cur", "left", "right"):
            assert 0 <= lv[k + "_off"] and 0 <= lv[k + "_n"] and lv[k + "_off"] + lv[k + "_n"] <= nl
        assert 0 <= si["ref_off"] and 0 <= si["ref_n"] and si["ref_off"] + si["ref_n"] <= nr
        assert 0 <= si["obs_off"] and 0 <= si["obs_n"] <= sc["n_obs"] and si["obs_off"] + si["obs_n"] <= no


def concat_scenes(cases):
    """the scenes of `cases` as one batch: pools concatenated, every offset moved, obstacle slots padded to the largest"""
    n_obs = max(max(int(c.sc["n_obs"]) for c in cases), 1)
    si = np.concatenate([c.sc["scene_in"][:1] for c in cases]).copy()
    lane, attr, ref = [], [], []
    obs = np.zeros(len(cases) * n_obs, cases[0].sc["obs_pool"].dtype)
    mot = np.zeros(len(cases) * n_obs, cases[0].sc["mot_pool"].dtype)
    lo = ro = 0
    for k, c in enumerate(cases):
        for key in ("cur_off", "left_off", "right_off"):
            si["lanes"][key][k] += lo
        si["ref_off"][k] += ro
        m, o = int(c.sc["scene_in"]["obs_n"][0]), int(c.sc["scene_in"]["obs_off"][0])
        obs[k * n_obs:k * n_obs + m], mot[k * n_obs:k * n_obs + m] = c.sc["obs_pool"][o:o + m], c.sc["mot_pool"][o:o + m]
        si["obs_off"][k] = k * n_obs
        lane.append(c.sc["lane_pool"]), attr.append(c.sc["attr_pool"]), ref.append(c.sc["ref_pool"])
        lo, ro = lo + len(c.sc["lane_pool"]), ro + len(c.sc["ref_pool"])
    sc = dict(scene_in=si, lane_pool=np.concatenate(lane), attr_pool=np.concatenate(attr), ref_pool=np.concatenate(ref),
              obs_pool=obs, mot_pool=mot, n_obs=n_obs, state=np.concatenate([c.st[:1] for c in cases]).copy())
    assert_fenced(sc)
    return sc


# ---- the model on a scene -----------------------------------------------------------------------------------------------
def _lane(sc, key):
    lv = sc["scene_in"]["lanes"][0]
    p = sc["lane_pool"][int(lv[key + "_off"]):int(lv[key + "_off"]) + int(lv[key + "_n"])]
    return list(zip(p["x"].tolist(), p["y"].tolist(), p["dir"].tolist()))


def _cfgd(cfg):
    return {k: float(cfg[k][0]) for k in ("ROAD_FARAIM_MAX", "ROAD_FARAIM_MIN", "PRE_INTER_FARAIM", "INTER_FARAIM",
                                          "ROAD_REMAIN_DISTANCE", "INTER_REMAIN_DISTANCE", "EPSILON", "PI", "Vehicle_Width")}


def _aim(a):
    p = a["Aim_point"]
    return float(p["x"]), float(p["y"]), float(p["dir"]), int(a["Aim_id"])


def model_tick(cfg, case):
    """What front_model.py expects of ONE tick of the case: a dict with any of aim_far / aim_near (x, y, Aim_id),
    near_id, fid, remain, cause, road (200 points), refpath_n, refpath.  Junction scenes with the decision stage on and every
    scene with it off; a first tick (count 0) stops at the aim points - its path is a Bezier curve (sin / cos)."""
    c = _cfgd(cfg)
    sc, st = case.sc, case.st[0]
    si = sc["scene_in"][0]
    loc = si["loc"]
    pos, lane_num = int(loc["pos"]), int(loc["lane_num"])
    ids = [int(v) for v in loc["id"]]
    lane_id = lambda k: ids[min(max(k, 0), len(ids) - 1)]
    cur = _lane(sc, "cur")
    inter = sc["ref_pool"][int(si["ref_off"]):int(si["ref_off"]) + int(si["ref_n"])]
    inter = list(zip(inter["x"].tolist(), inter["y"].tolist()))
    out = {}
    if int(cfg["decision_stage"][0]):
        assert pos in (1, 2), "the model covers the decision stage at a junction only"
        id_ = lane_id(lane_num - 1) if pos == 1 else lane_id(int(loc["last_lanenum"]) - 1)
        n1, n2, refpath = fm.junction_front_path(pos, cur, inter, id_)
        out["refpath_n"], out["refpath"], out["n1n2"] = n1 + n2, refpath, (n1, n2)
        behavior, same_lane = 1, True
    else:
        n = min(int(si["dec"]["refpath_n"]), int(si["ref_n"]), fm.MAX_REFPATH)
        refpath = inter[:max(n, 0)]
        behavior, same_lane = int(si["dec"]["behavior"]), int(si["dec"]["target_lanenum"]) == lane_num
    faraim = fm.aim_dis(pos, float(loc["velocity"]), c)
    has_left, has_right = lane_num > 1, lane_num < int(si["lanes"]["lane_sum"])
    far, near = fm.search_aim_point(
        pos, behavior, same_lane, faraim, _aim(st["aimpoint_far"]), _aim(st["aimpoint_near"]),
        cur=cur, cur_id=lane_id(lane_num - 1),
        left=_lane(sc, "left") if has_left else (), left_id=lane_id(lane_num - 2) if has_left else 0,
        right=_lane(sc, "right") if has_right else (), right_id=lane_id(lane_num) if has_right else 0,
        refpath=refpath, eps=c["EPSILON"], pi=c["PI"])
    out["aim_far"], out["aim_near"] = (far[0], far[1], far[3]), (near[0], near[1], near[3])
    if int(st["count"]) == 0:
        return out
    last = list(zip(st["last_Bpoints"]["x"].tolist(), st["last_Bpoints"]["y"].tolist()))
    ego = (float(loc["globalpoint"]["x"]), float(loc["globalpoint"]["y"]))
    mid, fid, remain, index = fm.local_state(last, ego, int(st["path_near_id"]))
    lat = fm.lat_dis(ego, last[index], last[index + 1], c["EPSILON"])
    derr = fm.angle_err(fm.road_angle(last[index], last[index + 1], c["EPSILON"], c["PI"]), float(loc["globalpoint"]["dir"]))
    afresh, cause = fm.update_plan_judge(int(st["his_behavior"]), behavior, pos, lat, derr, remain, c)
    out.update(near_id=mid, fid=fid, remain=remain, cause=cause)
    if not afresh:
        out["road"] = last
    elif pos in (1, 2):
        out["na"] = fm.na_of(far[3], len(refpath))
        out["road"] = fm.mean_points(refpath, out["na"], fm.PATH_POINTS, c["EPSILON"])
    return out


def model_flags(case):
    si = case.sc["scene_in"][0]
    lane = _lane(case.sc, "cur")
    off = int(si["lanes"]["cur_off"])
    attrs = case.sc["attr_pool"][off:off + len(lane)].tolist()
    k = int(si["loc"]["lane_num"]) - 1
    return fm.remaining_flags(lane, attrs, int(si["loc"]["id"][k]))


# ---- family: aim ---------------------------------------------------------------------------------------------------------
AIM_K = (257, 1, 7, 8, 9, 255, 256, 258, 511, 512, 513, 769)      # (the first case of a family also runs as 300 copies)


def road_scene(dm, cfg, cur_xy, behavior=1, target=None, left=None, right=None, ids=None, stale=True):
    sc = lcs.make_scene(dm, cfg, map_attr=0)
    put_lanes(dm, sc, cur=cur_xy, left=left, right=right)
    own_decision(sc, behavior, target)
    sc["scene_in"]["loc"]["velocity"] = 0.0
    if ids is not None:
        sc["scene_in"]["loc"]["id"][:] = ids
    st = sc["state"].copy()
    if stale:
        mark_aims(st)
    return sc, st


def aim_cases(dm, cfgs):
    out = []
    E = lcs.EGO_ID

    def add(name, xs, aim_id, **kw):
        y = kw.pop("y", None)
        xy = line(ego_lane(xs))
        if y is not None:
            xy[:, 1] = y
        sc, st = road_scene(dm, cfgs["off"], xy, **kw)
        if aim_id is None:                                                      # no step: far stays, near still follows it (:434)
            hand = dict(aim_far=STALE_FAR[:2] + STALE_FAR[3:], aim_near=STALE_FAR[:2] + STALE_FAR[3:])
        else:
            hand = dict(aim_far=(float(xy[aim_id, 0]), float(xy[aim_id, 1]), aim_id))
            hand["aim_near"] = hand["aim_far"]                                  # behaviour 1: near follows far (:434)
        out.append(Case("aim", name, "off", sc, st, hand=hand))

    for K in AIM_K:
        add(f"K{K}", walk_xs(X_EGO, K + 12, K), E + K - 1)
        add(f"K{K}_twin", walk_xs(X_EGO, K + 12, K, twin=True), E + K)
    for S in (255, 256, 257, 600):                                             # S segments of h after the ego: 9.4 m at most
        add(f"lane_end_{S}", X_EGO + H * np.arange(S + 1), E + S)
    add("stop_on_last_segment", walk_xs(X_EGO, 257, 257), E + 256)            # cur_n = 50 + 258: the stop is i = cur_n - 2
    add("id_negative", walk_xs(X_EGO, 20, 3), 28, ids=-3)                      # walks from point 0 at 0.5 m: 29 * 0.5 = 14.5
    add("id_at_lane_end", walk_xs(X_EGO, 20, 3), None, ids=E + 20)             # i0 = iend = cur_n - 1
    add("id_past_lane_end", walk_xs(X_EGO, 20, 3), None, ids=E + 26)
    for name, K, at, want in (("nan_in_first_eight", 257, E + 3, "end"), ("nan_in_second_block", 513, E + 300, "end"),
                              ("nan_one_past_stop", 257, E + 258, E + 256), ("inf_before_stop", 257, E + 5, E + 4)):
        xs = walk_xs(X_EGO, K + 12, K)
        xs[at - E] = math.inf if name.startswith("inf") else math.nan
        add(name, xs, E + K + 12 if want == "end" else want)
    xs = walk_xs(X_EGO, 269, 257)
    add("nan_y_in_second_pass", xs, E + 269, y=np.where(np.arange(E + 270) == E + 257, math.nan, Y2))   # the stop segment itself
    return out


def aim_side_cases(dm, cfgs):
    out = []
    E, Y1, Y3 = lcs.EGO_ID, 200.0, 192.5
    for K in (257, 255, 256):
        side = line(ego_lane(walk_xs(X_EGO, K + 12, K)))
        for beh, tgt, key, y in ((2, 1, "left", Y1), (3, 3, "right", Y3)):
            xy = side.copy()
            xy[:, 1] = y
            other = line(100.0 + 0.5 * np.arange(E + K + 13), Y1 if beh == 3 else Y3)      # as long as the lane walked
            sc, st = road_scene(dm, cfgs["off"], None, beh, tgt, **{key: xy, "right" if beh == 2 else "left": other})
            out.append(Case("aim-side", f"beh{beh}_K{K}", "off", sc, st,
                            hand=dict(aim_far=(float(xy[E + K - 1, 0]), y, E + K - 1), aim_near=STALE_NEAR[:2] + STALE_NEAR[3:])))
    # behaviour 2, the left lane ends 256 segments after the ego: the default reads the CURRENT lane at left_n - 2 = 305
    left = line(ego_lane(X_EGO + H * np.arange(257)), Y1)
    sc, st = road_scene(dm, cfgs["off"], None, 2, 1, left=left)
    out.append(Case("aim-side", "beh2_default_from_current_lane", "off", sc, st,
                    hand=dict(aim_far=(100.0 + 0.5 * 305, Y2, 306))))
    # ... and with a current lane of 100 points the index is fenced to its last point
    sc, st = road_scene(dm, cfgs["off"], line(100.0 + 0.5 * np.arange(100)), 2, 1, left=left)
    out.append(Case("aim-side", "beh2_default_fenced_into_current_lane", "off", sc, st, hand=dict(aim_far=(149.5, Y2, 306))))
    # behaviour 3, K = 256 (stop i = 305): left_n = 306 -> iend = 305, the walk ends one short: default = right lane's end
    right = line(ego_lane(walk_xs(X_EGO, 268, 256)), Y3)
    for left_n, want in ((E + 256, len(right) - 1), (E + 257, E + 255)):
        sc, st = road_scene(dm, cfgs["off"], None, 3, 3, right=right, left=line(100.0 + 0.5 * np.arange(left_n), Y1))
        out.append(Case("aim-side", f"beh3_left_n{left_n}", "off", sc, st, hand=dict(aim_far=(float(right[want, 0]), Y3, want))))
    # pos 1 (faraim 15) / pos 2 (faraim 10) on a refpath of its own, decision stage off: i0 = 0, Aim_id = K - 1
    for pos, lim in ((1, 19.0), (2, 14.0)):
        for K in (255, 256, 257):
            xs = walk_xs(X_EGO, K + 12, K, limit=lim)
            sc = lcs.make_junction_scene(dm, cfgs["off"], pos)
            own_decision(sc)
            put_ref(dm, sc, line(xs, 200.0))
            sc["scene_in"]["loc"]["velocity"] = 0.0
            hand = dict(aim_far=(float(xs[K - 1]), 200.0, K - 1))
            hand["aim_near"] = hand["aim_far"]
            out.append(Case("aim-side", f"pos{pos}_K{K}", "off", sc, hand=hand))
    # decision stage on: the walk reads k_decision's published path.  pos 1: 100 lane points from the ego, then the
    # polyline; pos 2: the polyline from Id_Inter = 7 on.  K = 256 falls in the second pass either way.
    xs = walk_xs(X_EGO, 300, 256, limit=19.0)
    sc = lcs.make_junction_scene(dm, cfgs["on"], 1)
    put_lanes(dm, sc, cur=line(ego_lane(xs[:100]), 200.0))
    put_ref(dm, sc, line(xs[100:], 200.0))
    sc["scene_in"]["obs_n"] = 0
    out.append(Case("aim-side", "pos1_K256_decision_on", "on", sc, hand=dict(aim_far=(float(xs[255]), 200.0, 255), refpath_n=301)))
    xs = walk_xs(X_EGO, 300, 256)
    sc = lcs.make_junction_scene(dm, cfgs["on"], 2)
    put_ref(dm, sc, line(np.concatenate([X_EGO - 7 + np.arange(7), xs]), 200.0))
    put_lanes(dm, sc, cur=line(xs[-1] + H * (1 + np.arange(100)), 200.0))
    sc["scene_in"]["loc"]["id"][:] = 7
    out.append(Case("aim-side", "pos2_K256_decision_on", "on", sc, hand=dict(aim_far=(float(xs[255]), 200.0, 255), refpath_n=361)))
    return out


# ---- family: local ---------------------------------------------------------------------------------------------------
TIE_SETS = ((0, 199), (5, 70), (70, 134), (70, 5, 198), (63, 64), (191, 192), (199, 135))
TIE_POINTS = ((3.0, 4.0), (4.0, 3.0), (-3.0, 4.0))
MIDS = (0, 63, 64, 182, 183, 184, 189, 190, 191, 192, 198, 199)


def local_cases(dm, cfgs):
    out = []

    def add(name, put, near_id=0, hand=None, far=False):
        sc = lcs.make_scene(dm, cfgs["off"], map_attr=0, obstacles=())
        own_decision(sc)
        g = sc["scene_in"]["loc"]["globalpoint"]
        g["x"], g["y"], g["dir"] = 0.0, 0.0, 0.0
        st = sc["state"].copy()
        st["count"], st["his_behavior"], st["path_near_id"] = 1, 1, near_id
        x = (20000.0 if far else 6.0) + 0.25 * np.arange(200)
        y = np.zeros(200)
        put(x, y)
        st["last_Bpoints"]["x"], st["last_Bpoints"]["y"] = x, y
        out.append(Case("local", name, "off", sc, st, hand=hand))

    def rem(mid):
        return max(199 - (mid + 8), 0) * 0.25

    for s in TIE_SETS:
        for p in TIE_POINTS:
            def put(x, y, s=s, p=p):
                x[list(s)], y[list(s)] = p
            m = min(s)
            add("tie_" + "_".join(map(str, s)) + f"_at_{p[0]:g}_{p[1]:g}", put, hand=dict(near_id=m, fid=m + 8))
    for m in MIDS:
        def put(x, y, m=m):
            x[m], y[m] = 3.0, 4.0
        add(f"mid_{m}", put, hand=dict(near_id=m, fid=m + 8, remain=rem(m)))
    for nan_at, m, nan_rem in ((30, 100, False), (150, 100, True), (107, 100, False), (108, 100, True), (101, 100, False)):
        def put(x, y, nan_at=nan_at, m=m):
            x[m], y[m] = 3.0, 4.0
            x[nan_at] = math.nan
        add(f"nan_{nan_at}_min_{m}", put, hand=dict(near_id=m, fid=m + 8) if nan_rem else dict(near_id=m, fid=m + 8, remain=rem(m)))
        out[-1].nan_remain = nan_rem
    for near_id, want in ((7, 7), (250, 199)):
        def put(x, y):
            x[:] = math.nan
        add(f"all_nan_prev_{near_id}", put, near_id, hand=dict(near_id=want, fid=want + 8))
    add("all_beyond_9999", lambda x, y: None, 7, hand=dict(near_id=7, fid=15, remain=184 * 0.25), far=True)
    return out


# ---- family: gen -----------------------------------------------------------------------------------------------------
def gen_cases(dm, cfgs):
    out = []

    def add(name, pos, xy, refpath_n=None, hand=None, stale=False):
        sc = lcs.make_junction_scene(dm, cfgs["off"], pos)
        own_decision(sc)
        put_ref(dm, sc, xy, refpath_n)
        st = sc["state"].copy()
        st["count"], st["his_behavior"] = 1, 0                                  # behaviour 1 != 0: cause 1, replans
        st["last_Bpoints"]["x"], st["last_Bpoints"]["y"] = X_EGO + 0.25 * np.arange(200), 200.0
        if stale:
            mark_aims(st)
        out.append(Case("gen", f"pos{pos}_{name}", "off", sc, st, hand=dict(hand or {}, cause=1)))

    for pos, lim in ((1, 19.0), (2, 14.0)):
        for na in (65, 0, 1, 3, 63, 64, 199, 200, 300):
            n = 512 if na == 300 else na + 14
            add(f"na{na}", pos, line(walk_xs(X_EGO, n - 1, na + 1, limit=lim), 200.0), hand=dict(na=min(na, 200)))
        pts = line(walk_xs(X_EGO, 4, 3, limit=lim), 200.0)
        add("na2_stale_aim_n2", pos, pts[:2], hand=dict(na=2, aim_far=(STALE_FAR[0], STALE_FAR[1], 17)), stale=True)
        add("na1_stale_aim_n1", pos, pts[:1], hand=dict(na=1), stale=True)
        add("na0_stale_aim_n0", pos, pts[:0], hand=dict(na=0), stale=True)
        add("refpath_n_below_ref_n", pos, pts, refpath_n=2, hand=dict(na=2), stale=True)
        # 300 points at 0.25 m: the walk stops at i = 56 (pos 2) / 76 (pos 1); runs of six equal points move it on by five
        base = X_EGO + 0.25 * np.arange(300)
        for where, at in (("start", 0), ("middle", 30), ("end_of_na", 50 if pos == 2 else 70)):
            xs = base.copy()
            xs[at:at + 6] = xs[at]
            xs[at + 6:] -= 1.25
            add(f"repeats_{where}", pos, line(xs, 200.0), hand=dict(na=(56 if pos == 2 else 76) + 5))
        add("all_equal", pos, line(np.full(100, X_EGO), 200.0), hand=dict(na=99, road=[(X_EGO, 200.0)] * 200))
        xs = X_EGO + 2.0 ** -4 * np.arange(400)                                 # stop at i = 224 / 304: na = 200, s_k = cum[k]
        add("abscissa_on_vertices", pos, line(xs, 200.0), hand=dict(na=200, road=[(float(v), 200.0) for v in xs[:200]]))
        xs = base.copy()
        xs[20] = math.nan
        add("nan_inside_na", pos, line(xs, 200.0), hand=dict(na=200))           # NaN sum never stops: Aim_id 299, na 200
    return out


# ---- family: flags ---------------------------------------------------------------------------------------------------
FLAG_COMBOS = {      # the out_lanes / map_attr combinations of lanechange_scenes.SCENARIOS whose decision reads the flag
    "A60": dict(lane_num=2, map_attr=1, out_lanes=(2,), ahead=1),
    "B15": dict(lane_num=2, map_attr=1, out_lanes=(1, 2), ahead=1),
    "B50": dict(lane_num=2, map_attr=2, out_lanes=(2,), ahead=3),
    "B10": dict(lane_num=2, map_attr=2, out_lanes=(1, 2), ahead=3),
}
G = 2.0 ** -3


def flag_scene(dm, cfg, combo, xs, attrs_ahead, id_cur=5, obstacle=10.0):
    """Current lane `xs` (lane 2), the ego on point e = id_cur fenced into the lane (the id itself goes to the scene as it is), an
    obstacle `obstacle` m ahead; attrs_ahead[k] is the attribute of point e + 1 + k, i.e. of segment k of the run (zero past its end)."""
    kw = dict(FLAG_COMBOS[combo])
    kw.pop("ahead")
    sc = lcs.make_scene(dm, cfg, period=1600.0, obstacles=[(2, 10.0)], **kw)
    a = np.zeros(len(xs), np.uint8)
    e = min(max(id_cur, 0), len(xs) - 1)
    a[:e + 1] = kw["map_attr"]
    m = min(len(attrs_ahead), len(xs) - e - 1)
    a[e + 1:e + 1 + m] = attrs_ahead[:m]
    put_lanes(dm, sc, cur=line(xs), attr=a)
    si = sc["scene_in"]
    si["loc"]["id"][:] = 5                                                     # the neighbour lanes keep their 320 points
    si["loc"]["id"][0, kw["lane_num"] - 1] = id_cur
    si["loc"]["globalpoint"]["x"] = xs[e]
    sc["obs_pool"]["x"][:] = xs[e] + obstacle
    return sc


def flags_cases(dm, cfgs):
    out = []
    xs = 100.0 + G * np.arange(720)

    def add(name, combo, x, ahead, hand=None, **kw):
        out.append(Case("flags", f"{combo}_{name}", "on", flag_scene(dm, cfgs["on"], combo, x, np.asarray(ahead, np.uint8), **kw),
                        ticks=3, hand=dict(flags=hand) if hand is not None else {}))
        out[-1].combo = combo

    def flags_of(a_seg, b_seg):
        return a_seg * G > 60, b_seg * G > 10, b_seg * G > 15, b_seg * G > 50

    for combo, runs in (("A60", (480, 479, 481)), ("B50", (399, 400, 401)), ("B15", (119, 120, 121)), ("B10", (79, 80, 81))):
        ahead = FLAG_COMBOS[combo]["ahead"]
        for run in runs:
            add(f"run{run}", combo, xs, [ahead] * run, flags_of(run if ahead == 1 else 0, run))
    # irregular spacing (no exact sums), scaled so that the combination's threshold T falls inside segment r of the triple
    # r - 1 | r | r + 1: the first r segments sum to T - 0.3 d, the first r + 1 to T + 0.7 d (d: the length of segment r, 0.06 m at
    # least - far above the rounding of either sum).  A run end miscounted by one segment at a wave or block seam flips the flag.
    rng = np.random.default_rng(22)
    d = rng.uniform(0.5, 1.0, 719)
    for r, combos in ((64, ("B10", "B15")), (256, ("B50", "A60")), (512, ("B50", "A60"))):
        for combo in combos:
            T = float(combo[1:])
            xi = np.concatenate([[100.0], 100.0 + np.cumsum(d * (T / (d[5:5 + r].sum() + 0.3 * d[5 + r])))])
            for run in (r - 1, r, r + 1):
                past = run > r
                hand = dict(B10=(False, past, False, False), B15=(False, True, past, False), B50=(False, True, True, past),
                            A60=(past, True, True, True))[combo]
                add(f"irregular_run{run}", combo, xi, [FLAG_COMBOS[combo]["ahead"]] * run, hand)
    for a_end in (100, 300, 520):                                              # A ends in block 0 | 1 | 2, B runs on to 700
        for combo in ("A60", "B15"):
            add(f"A_ends_{a_end}_B_700", combo, xs, [1] * a_end + [3] * (700 - a_end), flags_of(a_end, 700))
    # A ended in block 0; attribute 1 again from the first segment of block 1: a block-wise count that forgot the run had ended
    # would add 444 more segments (68 m in all) to A's 12.5 m
    for combo in ("A60", "B15"):
        add("A_ends_100_attr1_again_at_256", combo, xs, [1] * 100 + [3] * 156 + [1] * 444, flags_of(100, 700))
        add("A_ends_300_attr1_again_at_512", combo, xs, [1] * 300 + [3] * 212 + [1] * 188, flags_of(300, 700))
    # a NaN point inside B's part only: A = 500 segments = 62.5 m is past its threshold before the NaN and is still decided
    # (the A60 combination changes lane), B's sum is NaN and every B flag false (the B15 combination keeps the lane)
    xn = xs.copy()
    xn[5 + 600] = math.nan
    for combo in ("A60", "B15"):
        add("nan_in_B_only", combo, xn, [1] * 500 + [3] * 200, (True, False, False, False))
    # the ego 0 | 1 | 2 points before the lane end, the last two segments 6 m each: B = 0 | 6 | 12 m, so B > 10 is set only two
    # points before the end.  The obstacle stands on the next lane point, 6 m ahead.  On the last point the front path is a single
    # point and finds no obstacle: the decision never gets to the flag, and that case states no outcome (its flags and its
    # parity with the oracle are still checked).
    xe = np.concatenate([xs[:718], xs[717] + 6.0 * np.arange(1, 3)])
    for back in (0, 1, 2):
        add(f"ego_{back}_before_lane_end", "B10", xe, [3] * 10, (False, back == 2, False, False), id_cur=len(xe) - 1 - back, obstacle=6.0)
    out[-3].combo = None
    # the run ends on the lane's last segment after 256 | 512 segments, at a dyadic spacing g with (run - 1) g < T < run g: the
    # flag is set, and one segment fewer at the lane end would clear it (256: 401 | 481 / 2048, 512: 801 | 961 / 8192; sums exact)
    for run, combo, g in ((256, "B50", 401 / 2048), (256, "A60", 481 / 2048), (512, "B50", 801 / 8192), (512, "A60", 961 / 8192)):
        T = float(combo[1:])
        assert (run - 1) * g < T < run * g
        ahead = FLAG_COMBOS[combo]["ahead"]
        add(f"run{run}_to_lane_end", combo, 100.0 + g * np.arange(720), [ahead] * 720, (ahead == 1, True, True, True),
            id_cur=719 - run)
    return out


# ---- family: jfront --------------------------------------------------------------------------------------------------
def jfront_cases(dm, cfgs):
    out = []

    def finish(name, sc, n1, n2, both):
        n = n1 + n2
        obs = [((n - 1) * G, 0.0)] + ([(0.0, 0.0)] if both else [])
        for j, (ahead, left) in enumerate(obs):
            o = sc["obs_pool"][j]
            o["x"], o["y"], o["type"], o["radius"] = X_EGO + ahead, 200.0 + left, 0, 0.5
        sc["scene_in"]["obs_n"] = len(obs) if n > 0 else 0
        hand = dict(refpath_n=n, n1n2=(n1, n2), refpath=[(X_EGO + G * k, 200.0) for k in range(n)])
        if n >= 2:
            hand["around0"] = (1, 0.0, 0.0 if both else (n - 1) * G)
        out.append(Case("jfront", name + ("_both" if both else "_last"), "on", sc, hand=hand))

    for tail in (512, 400, 511, 513):
        for ref_n in (112, 0, 1, 200):
            for both in (False, True):
                sc = lcs.make_junction_scene(dm, cfgs["on"], 1, obstacles=[(0.0, 0.0), (0.0, 0.0)])
                put_lanes(dm, sc, cur=line(ego_lane(X_EGO + G * np.arange(tail)), 200.0))
                put_ref(dm, sc, line(X_EGO + G * (tail + np.arange(ref_n)), 200.0))
                n1 = min(tail, 512)
                finish(f"pos1_tail{tail}_ref{ref_n}", sc, n1, min(ref_n, 512 - n1), both)
    for tail in (452, 453, 512, 600, 0, -5):                                   # 0 / -5: Id_Inter = ref_n, Id_Inter > ref_n
        for both in (False, True):
            sc = lcs.make_junction_scene(dm, cfgs["on"], 2, obstacles=[(0.0, 0.0), (0.0, 0.0)])
            id_inter = 7 if tail > 0 else 40 - tail
            ref_n = id_inter + tail if tail > 0 else 40
            n1 = min(max(tail, 0), 512)
            put_ref(dm, sc, line(X_EGO + G * (np.arange(ref_n) - id_inter), 200.0))
            put_lanes(dm, sc, cur=line(X_EGO + G * (max(tail, 0) + np.arange(dm.GEN_LANE_PTS)), 200.0))
            sc["scene_in"]["loc"]["id"][:] = id_inter
            finish(f"pos2_tail{tail}", sc, n1, min(60, 512 - n1), both)
    return out


# ---- family: sweep ---------------------------------------------------------------------------------------------------
def sweep_cases(dm, cfgs):
    """Ego lane 2, map attribute 0, obstacles 10 m ahead at 0.25 m and 1.15 m left of the lane centre.  Relative to left
    candidate i they sit at 0.25 - 0.3 i and 1.15 - 0.3 i: one of them is inside [-0.9, 0.9] for i = 0..6, both are outside at
    i = 7 (-1.85, -0.95).  Right candidate i: 0.25 + 0.3 i leaves the window at i = 3.  So W 6.3 (8 candidates) goes left at
    index 7, W 3.75 (4) right at 3, W 2.1 (1: the path itself) and W 1.8 (0) find nothing and keep behaviour 1."""
    out = []
    for W, n_cand, want in ((6.3, 8, (-1, 7)), (1.8, 0, (0, -1)), (2.1, 1, (0, -1)), (3.75, 4, (1, 3)), (9.0, 8, (-1, 7))):
        sc = lcs.make_scene(dm, cfgs["on"], map_attr=0, obstacles=[(2, 10.0, 0.25), (2, 10.0, 1.15)])
        sc["scene_in"]["lanes"]["lane_width"] = W
        out.append(Case("sweep", f"W{W:g}", "on", sc, ticks=3, hand=dict(n_cand=n_cand, sweep=want)))
    return out


FAMILIES = dict(aim=aim_cases, **{"aim-side": aim_side_cases}, local=local_cases, gen=gen_cases, flags=flags_cases,
                jfront=jfront_cases, sweep=sweep_cases)


def all_cases(dm, cfgs):
    """cfgs: {"on": config with the decision stage, "off": without}"""
    cases = {f: build(dm, cfgs) for f, build in FAMILIES.items()}
    for cs in cases.values():
        assert len({c.name for c in cs}) == len(cs)
        for c in cs:
            assert_fenced(c.sc)
    return cases
