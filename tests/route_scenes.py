"""A drivable ring for the route-following tests: four roads, each a left-hand arc of 70 degrees, joined by
junction arcs of 20 degrees - four times 90 degrees, so the ring closes by symmetry and no junction turns the ego by more than
30 degrees.  Roads 1, 2 and 4 have three lanes, road 3 has two; lane 2 is the centreline (260 points at exactly 0.5 m), lane 1 lies
3.75 m to its left (the inside of the ring: ~0.48 m spacing), lane 3 to its right (~0.52 m).  Every lane that exists on both sides
of a junction has a 40-point polyline to the same lane of the next road; its points continue the spacing of the lane, the lane's
last point and the next lane's first are NOT repeated in it.  Lane 3 of road 2 has no junction: an ego that stays there misses its
exit.  (The map of map_scenes.build_map folds back on itself and cannot be lapped.)"""
import math

import numpy as np

LANE_W = 3.75
LANE_W_CM = 375
PTS = 260                     # points per lane
JPTS = 40                     # points per junction polyline
STEP = 0.5
ROAD_TURN = math.radians(70.0)
JUNC_TURN = math.radians(20.0)
ROAD_LEN = (PTS - 1) * STEP                   # 129.5 m along lane 2
JUNC_LEN = (JPTS + 1) * STEP                  # 20.5 m from the last point of a lane to the first of the next
N_LANES = (3, 3, 2, 3)
CENTRE = (400.0, 400.0)


def _arc(x0, y0, th0, k, s, d):
    """Point at arc length s of the arc of curvature k from the pose (x0, y0, th0), moved d to the left; and the heading there."""
    th = th0 + k * s
    x = x0 + (np.sin(th) - math.sin(th0)) / k
    y = y0 - (np.cos(th) - math.cos(th0)) / k
    return x - d * np.sin(th), y + d * np.cos(th), th


def build_ring(dm):
    kr, kj = ROAD_TURN / ROAD_LEN, JUNC_TURN / JUNC_LEN
    # the centreline starts so that the ring is centred on CENTRE: found by walking one lap from the origin first
    def lap(x, y, th):
        poses = []
        for r in range(4):
            poses.append((x, y, th))
            x, y, th = (float(v) for v in _arc(x, y, th, kr, ROAD_LEN, 0.0))
            poses.append((x, y, th))
            x, y, th = (float(v) for v in _arc(x, y, th, kj, JUNC_LEN, 0.0))
        return poses
    p0 = lap(0.0, 0.0, 0.0)
    cx = sum(p[0] for p in p0[0::2]) / 4.0
    cy = sum(p[1] for p in p0[0::2]) / 4.0
    poses = lap(CENTRE[0] - cx, CENTRE[1] - cy, 0.0)
    lanes, first, pts, attr, width, junc, jpts = [], [0], [], [], [], [], []
    for r in range(4):
        x0, y0, th0 = poses[2 * r]
        for l in range(N_LANES[r]):
            d = LANE_W * (1 - l)                                  # lane 1: +3.75 (left), lane 2: 0, lane 3: -3.75
            x, y, th = _arc(x0, y0, th0, kr, STEP * np.arange(PTS), d)
            p = np.zeros(PTS, dm.GlobalPoint3D)
            p["x"], p["y"], p["dir"] = x, y, np.degrees(th) % 360.0
            a = np.full(PTS, 2 if l == 0 else (1 if l == N_LANES[r] - 1 else 3), np.uint8)      # where a change is allowed: away from the edges
            a[:20] = 0
            a[PTS - 40:] = 0
            lanes.append((sum(len(q) for q in pts), PTS, N_LANES[r]))
            pts.append(p), attr.append(a), width.append(np.full(PTS, LANE_W_CM, np.uint16))
        first.append(len(lanes))
    for r in range(4):
        x0, y0, th0 = poses[2 * r + 1]
        nxt = (r + 1) % 4
        for l in range(min(N_LANES[r], N_LANES[nxt])):
            x, y, _ = _arc(x0, y0, th0, kj, STEP * (1 + np.arange(JPTS)), LANE_W * (1 - l))
            jp = np.zeros(JPTS, dm.GlobalPoint2D)
            jp["x"], jp["y"] = x, y
            junc.append((r + 1, nxt + 1, l + 1, l + 1, sum(len(q) for q in jpts), JPTS))
            jpts.append(jp)
    return dict(road_first_lane=np.array(first, np.int32),
                lanes=np.array([(o, n, ls, 0) for o, n, ls in lanes], dm.MapLane),
                points=np.concatenate(pts), lanechg_attribute=np.concatenate(attr), lane_width_cm=np.concatenate(width),
                junctions=np.array(junc, dm.MapJunction), jpoints=np.concatenate(jpts))


def exit_lanes(road):
    """Lanes of `road` (1-based) that have a junction to the next road of the ring."""
    return list(range(1, min(N_LANES[road - 1], N_LANES[road % 4]) + 1))


def make_route(dm, first_road, n_legs):
    """n_legs legs round the ring from first_road (1-based)."""
    legs = np.zeros(n_legs, dm.RouteLeg)
    for k in range(n_legs):
        road = (first_road - 1 + k) % 4 + 1
        legs["road_num"][k] = road
        legs["stub_attribute"][k] = (1, 0, 1, 3)[road - 1]
        ex = exit_lanes(road)
        legs["out_lane_no"][k, :len(ex)] = ex
    return legs


def caps(m, n, n_obs=0, slack=0):
    return dict(max_scenes=n, max_obs_total=max(n * n_obs + slack, 1), max_lane_pts_total=len(m["points"]), max_ref_pts_total=len(m["jpoints"]))


def make_egos(dm, cfg, m, n, seed=3, lanes=(1, 2), ids=(10, 60), legs=(6, 10), mixed=False, speed=(20.0, 30.0), n_obs=0):
    """n obstacle-free egos on the ring with a route each.  Returns (sc, legs, route_first).  lanes: the lanes they start on;
    ids: the range of their start point; legs: the range of their leg count.  mixed: some start in the pre-junction or inside a
    junction, on any lane, near the end of a road or on the last leg of a short route (the step-by-step tests want every branch)."""
    rng = np.random.default_rng(seed)
    sc = dm.gen_scenes(cfg, 0, n, n_obs, junction_every=0)
    si = sc["scene_in"]
    S = float(cfg["grid_w"][0]) * float(cfg["cell"][0])
    all_legs, route_first = [], [0]
    for s in range(n):
        road = int(rng.integers(1, 5))
        pos = int(rng.choice([0, 0, 0, 1, 2])) if mixed else 0
        lane_pool = list(range(1, N_LANES[road - 1] + 1)) if mixed else [l for l in lanes if l <= N_LANES[road - 1]]
        lane = int(rng.choice(lane_pool))
        n_legs = int(rng.integers(legs[0], legs[1] + 1))
        if mixed and s % 7 == 3:
            n_legs = int(rng.integers(1, 3))                  # short routes: the last leg is reached in the run
        loc = si["loc"][s]
        prev = (road - 2) % 4 + 1
        if pos == 2 and (lane > min(N_LANES[prev - 1], N_LANES[road - 1])):
            pos = 0
        if pos == 1 and (lane not in exit_lanes(road) or n_legs < 2):
            pos = 0
        if pos == 2:                                          # in the junction leading INTO this road: the leg is still the last road's
            R = make_route(dm, prev, n_legs + 1)
            J = [q for q in m["junctions"] if q["last_road"] == prev and q["next_road"] == road and q["last_lane"] == lane][0]
            jid = int(rng.integers(1, JPTS - 4))
            p = m["jpoints"][int(J["point_off"]) + jid]
            q = m["jpoints"][int(J["point_off"]) + jid + 1]
            loc["last_roadnum"], loc["next_roadnum"], loc["last_lanenum"], loc["next_lanenum"] = prev, road, lane, lane
            loc["id"][:] = 0
            loc["id"][lane - 1] = jid
            ex, ey, ed = float(p["x"]), float(p["y"]), math.degrees(math.atan2(float(q["y"] - p["y"]), float(q["x"] - p["x"]))) % 360.0
        else:
            R = make_route(dm, road, n_legs)
            L = m["lanes"][m["road_first_lane"][road - 1] + lane - 1]
            if pos == 1:
                pid = int(rng.integers(205, 250))
            elif mixed:
                pid = int(rng.integers(10, 255))
            else:
                pid = int(rng.integers(ids[0], ids[1] + 1))
            p = m["points"][int(L["point_off"]) + pid]
            nxt = road % 4 + 1
            loc["last_roadnum"], loc["next_roadnum"], loc["last_lanenum"], loc["next_lanenum"] = road, nxt, lane, lane
            loc["id"][:] = pid
            ex, ey, ed = float(p["x"]), float(p["y"]), float(p["dir"])
        loc["pos"], loc["road_num"], loc["lane_num"], loc["path_num"] = pos, road, lane, 0
        loc["globalpoint"]["x"], loc["globalpoint"]["y"], loc["globalpoint"]["dir"] = ex, ey, ed
        loc["velocity"] = float(rng.uniform(speed[0], speed[1]))
        si["lanes"][s] = np.zeros(1, dm.LaneView)[0]
        si["ref_off"][s], si["ref_n"][s] = 0, 0
        si["obs_off"][s], si["obs_n"][s] = s * n_obs, 0
        si["out_lane_no"][s] = R["out_lane_no"][0]
        si["stub_attribute"][s] = R["stub_attribute"][0]
        si["period_last"][s] = 100.0
        si["grid_origin"][s]["x"], si["grid_origin"][s]["y"] = ex - 0.5 * S, ey - 0.5 * S
        si["goal"][s]["x"], si["goal"][s]["y"] = ex + 0.3 * S * math.cos(math.radians(ed)), ey + 0.3 * S * math.sin(math.radians(ed))
        st = sc["state"][s]
        st["z_target_lanenum"], st["d_his_target_lanenum"] = lane, lane
        all_legs.append(R)
        route_first.append(route_first[-1] + len(R))
    sc["lane_pool"], sc["attr_pool"], sc["ref_pool"] = m["points"], m["lanechg_attribute"], m["jpoints"]
    return sc, np.concatenate(all_legs), np.array(route_first, np.int32)
