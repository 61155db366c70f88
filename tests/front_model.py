"""A plain model of the front chain's block- and wave-parallel steps, written from DESIGN.md (§3.3 fences, §4 helper
specifications) and the cited lines of Planning.cpp / Decision.cpp - not from the kernels and not from the oracle.

Python floats (IEEE binary64) and math.sqrt, every sum in index order: the same operations in the same order as the
sequential loops of the reference, so every value that comes only from + - * / and sqrt is the bit pattern the reference
would produce.  Pure functions: no device, no oracle, no numpy.  Points are (x, y) tuples, lane points (x, y, dir).

The tests of tests/test_front_edges.py hold the device (k_decision, k_planning) and the oracle to these functions on the
scenes of tests/front_scenes.py."""
import math
import struct

PATH_POINTS = 200
MAX_REFPATH = 512
NAN = float("nan")


def f32(x):
    """the value after an assignment to a FLOAT member (Planning.h:20-21)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def seg_len(a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    return math.sqrt(dx * dx + dy * dy)


# ---- Calculate_aim_dis, Planning.cpp:242-290 ------------------------------------------------------------------------
def aim_dis(pos, velocity, cfg):
    """faraim_dis (= nearaim_dis).  cfg: mapping with ROAD_FARAIM_MAX / MIN, PRE_INTER_FARAIM, INTER_FARAIM."""
    if pos == 0:
        far = f32((velocity / 3.6) * 5 + 4)                     # :256, rounded to float on assignment
        if far > cfg["ROAD_FARAIM_MAX"]:
            far = f32(cfg["ROAD_FARAIM_MAX"])                   # :258-261
        elif far < cfg["ROAD_FARAIM_MIN"]:
            far = f32(cfg["ROAD_FARAIM_MIN"])                   # :262-266
        return far
    if pos == 1:
        return f32(cfg["PRE_INTER_FARAIM"])                     # :273-277
    if pos == 2:
        return f32(cfg["INTER_FARAIM"])                         # :281-285
    return 0.0                                                  # :250-251, 287


# ---- the walk of SearchAimPoint, Planning.cpp:410-432 ------------------------------------------------------------------
def aim_walk(points, i0, iend, faraim):
    """First i in [i0, iend) with  |P[i0] P[i0+1]| + ... + |P[i] P[i+1]| - 4 > faraim, else -1.  A negative i is skipped
    (fence).  Also returns whether any step was taken (the default of :426-429 is written on every step that
    does not stop)."""
    s, stepped = 0.0, False
    for i in range(i0, iend):
        if i < 0:
            continue
        s += seg_len(points[i], points[i + 1])                  # :413-414
        stepped = True
        if s - 4 > faraim:                                      # :416, strict; false for a NaN sum
            return i, True
    return -1, stepped


def road_angle(a, b, eps, pi):
    """GetRoadAngle, Planning.cpp:719-750 (through atan: not a bit-exact field)"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    if abs(dx) < eps and abs(dy) < eps:
        ang = 0.0
    elif abs(dx) < eps:
        ang = pi / 2 if b[1] > a[1] else 3 * pi / 2
    else:
        ang = math.atan(dy / dx)
        if b[0] < a[0]:
            ang = ang + pi
        elif b[0] > a[0] and b[1] < a[1]:
            ang = ang + 2 * pi
    return ang * 180 / pi


def angle_err(dir1, dir2):
    """GetAngleErr, Planning.cpp:760-786"""
    e = dir2 - dir1
    if dir1 < 180:
        if not (e <= 180):
            e = dir2 - dir1 - 360
    elif not (e > -180):
        e = dir2 - dir1 + 360
    return e


def lat_dis(cur, pt, nxt, eps):
    """GetLatDis, Planning.cpp:686-709"""
    if abs(pt[0] - nxt[0]) > eps:
        k = (pt[1] - nxt[1]) / (pt[0] - nxt[0])
        d = abs((cur[1] - pt[1]) - k * (cur[0] - pt[0])) / math.sqrt(1 + k * k)
    else:
        d = abs(pt[0] - cur[0])
    if d < eps:
        return 0.0
    cross = (nxt[0] - pt[0]) * (cur[1] - pt[1]) - (nxt[1] - pt[1]) * (cur[0] - pt[0])
    return d * (1 if cross > 0 else -1)


def search_aim_point(pos, behavior, same_lane, faraim, far, near, cur=(), cur_id=0, left=(), left_id=0, right=(),
                     right_id=0, refpath=(), eps=1e-6, pi=math.pi):
    """SearchAimPoint, Planning.cpp:303-583.  far / near: the previous aim points (x, y, dir, Aim_id); returns the new pair.
    same_lane: DecisionOut.target_lanenum == the ego's lane (:401).  left / right are empty (sum 0, id 0) when the lane
    does not exist (:359-380).  refpath: the DecisionOut.refpath of pos 1 / 2."""
    if pos == 0:
        if same_lane:
            if behavior == 1:                                                     # :404-434
                f, stepped = aim_walk(cur, cur_id, len(cur) - 1, faraim)
                if f >= 0:
                    far = (cur[f][0], cur[f][1], cur[f][2], f)                    # :418-421
                elif stepped:
                    e = cur[len(cur) - 1]
                    far = (e[0], e[1], e[2], len(cur) - 1)                        # :426-429
                near = far                                                        # :434
        elif behavior == 2:                                                       # :443-469
            f, stepped = aim_walk(left, left_id, len(left) - 1, faraim)
            if f >= 0:
                far = (left[f][0], left[f][1], left[f][2], f)
            elif stepped:                                                         # :464-467: the CURRENT lane at left_n - 2
                q = min(max(len(left) - 2, 0), max(len(cur) - 1, 0))              # (index fenced into the current lane)
                far = (cur[q][0], cur[q][1], cur[q][2], len(left) - 1)
        elif behavior == 3:                                                       # :473-499
            # the loop bound is the LEFT lane's sum (:478); fence: i + 1 stays inside the right lane, a negative id
            # never walks
            iend = min(len(left) - 1, len(right) - 1)
            f, stepped = aim_walk(right, right_id, iend, faraim) if right_id >= 0 else (-1, False)
            if f >= 0:
                far = (right[f][0], right[f][1], right[f][2], f)
            elif stepped:
                e = right[len(right) - 1]
                far = (e[0], e[1], e[2], len(right) - 1)                          # :494-497
    elif pos in (1, 2):                                                           # :505-578
        n = len(refpath)
        if n >= 3:                                                                # fence: size() - 1 is unsigned, p[n - 3]
            f, _ = aim_walk(refpath, 0, n - 1, faraim)
            if f >= 0:
                if n < 4 or f < n - 4:                                            # :517 compares unsigned
                    d = road_angle(refpath[f], refpath[min(f + 2, n - 1)], eps, pi)       # :519, i + 2 fenced
                else:
                    d = road_angle(refpath[max(f - 2, 0)], refpath[f], eps, pi)           # :523, i - 2 fenced
                far = (refpath[f][0], refpath[f][1], d, f)
            else:                                                                 # :529-536
                far = (refpath[n - 1][0], refpath[n - 1][1], road_angle(refpath[n - 3], refpath[n - 1], eps, pi), n - 1)
        near = far                                                                # :539, 577
    return far, near


# ---- GetVhclLocalState, Planning.cpp:623-676 --------------------------------------------------------------------------
def local_state(last200, ego, prev_near_id):
    """(path_near_id, path_front_near_id, remain_dis, index): the first minimum of the 200 distances strictly below 9999
    (:640-650; a NaN distance is never smaller), the previous id - fenced to [0, 199] - when nothing qualifies, fid = mid + 8
    (:649), the remaining length from fid in index order (:668-671), index = mid - 1 on the last point (:654-659)."""
    best, mid = 9999.0, min(max(prev_near_id, 0), PATH_POINTS - 1)
    for i in range(PATH_POINTS):
        dx, dy = ego[0] - last200[i][0], ego[1] - last200[i][1]
        d = math.sqrt(dx * dx + dy * dy)
        if d < best:
            best, mid = d, i
    fid = mid + 8
    remain = 0.0
    for i in range(fid, PATH_POINTS - 1):
        remain += seg_len(last200[i], last200[i + 1])
    return mid, fid, remain, (mid - 1 if mid == PATH_POINTS - 1 else mid)


def update_plan_judge(his_behavior, behavior, pos, lat, dir_err, remain, cfg):
    """UpdatePlanJudge, Planning.cpp:797-832: (afresh, cause)"""
    if his_behavior != behavior:
        return 1, 1
    if abs(lat) > 0.2:
        return 1, 2
    if abs(dir_err) > 45:
        return 1, 3
    if pos == 0 and remain < cfg["ROAD_REMAIN_DISTANCE"]:
        return 1, 4
    if pos != 0 and remain < cfg["INTER_REMAIN_DISTANCE"]:
        return 1, 4
    return 0, 0


# ---- PathPlanning at a junction, Planning.cpp:867-872 + MeanPoints --------------------------------------
def na_of(aim_id, refpath_n):
    """How many refpath points PathPlanning hands to MeanPoints: Ref_points[0 .. Aim_id), fenced to the 200 the array
    holds and to the refpath."""
    return max(min(aim_id, 200, refpath_n), 0)


def mean_points(refpath, na, n_out=PATH_POINTS, eps=1e-6):
    """MeanPoints over the first na points: arc-length resampling, the segment found by a LINEAR scan for the first
    cum[q + 1] >= s (so a tie on a vertex and zero-length segments take the smallest q), r = 0 on a segment not longer than
    EPSILON."""
    if na <= 0:
        return [(0.0, 0.0)] * n_out
    cum = [0.0]
    for i in range(1, na):
        cum.append(cum[i - 1] + seg_len(refpath[i - 1], refpath[i]))
    total = cum[na - 1]
    if na == 1 or total < eps:
        return [(refpath[0][0], refpath[0][1])] * n_out
    out = []
    for k in range(n_out):
        s = (total * k) / (n_out - 1) if n_out > 1 else 0.0
        j = na - 2
        for q in range(na - 1):
            if cum[q + 1] >= s:
                j = q
                break
        seg = cum[j + 1] - cum[j]
        r = (s - cum[j]) / seg if seg > eps else 0.0
        out.append((refpath[j][0] + r * (refpath[j + 1][0] - refpath[j][0]),
                    refpath[j][1] + r * (refpath[j + 1][1] - refpath[j][1])))
    return out


# ---- the remaining lane-change length tests, Decision.cpp:1178-1187 and the like ------------------------------------
def remaining_runs(lane, attrs, id_cur):
    """(A, B): the in-order sums  for (i = Id; i < n - 1 && PRED(attr[i + 1]); i++) dis += |p[i] p[i + 1]|  with PRED as the
    compiler parses it: A `attr == 1` (:1179), B `attr & 1` (:1212 and the like).  A negative id starts at 0 (fence)."""
    out = []
    for pred in (lambda a: a == 1, lambda a: (a & 1) != 0):
        s = 0.0
        for i in range(max(id_cur, 0), len(lane) - 1):
            if not pred(attrs[i + 1]):
                break
            s += seg_len(lane[i], lane[i + 1])
        out.append(s)
    return tuple(out)


def remaining_flags(lane, attrs, id_cur):
    """(A > 60, B > 10, B > 15, B > 50); a NaN sum makes its comparisons false"""
    a, b = remaining_runs(lane, attrs, id_cur)
    return a > 60, b > 10, b > 15, b > 50


# ---- PreStubDecision / StubDecision front path, Decision.cpp:323-486 ------------------------------------------------
def junction_front_path(pos, cur, inter, id_):
    """(n1, n2, points): pos 1 - the ego lane from Id_Cur on (:352-358), then the junction polyline (:361-367); pos 2 - the
    polyline from Id_Inter on (:438-444), then the first 60 points of the exit lane (:446-452).  At most 512 points
    (DecisionOut.refpath holds DMPP_MAX_REFPATH); a negative id starts at 0 (fence)."""
    i0 = max(id_, 0)
    if pos == 1:
        first = [(p[0], p[1]) for p in cur[i0:]][:MAX_REFPATH]
        second = [(p[0], p[1]) for p in inter][:MAX_REFPATH - len(first)]
    else:
        first = [(p[0], p[1]) for p in inter[i0:]][:MAX_REFPATH]
        second = [(p[0], p[1]) for p in cur[:60]][:MAX_REFPATH - len(first)]
    return len(first), len(second), first + second


def sweep_candidates(lane_width, vehicle_width, cap=8):
    """number of lateral candidates per side: BYTE i with (double)i < (W - Vehicle_Width) / 0.6 (Decision.cpp:940), at most
    DMPP_MAX_SWEEP"""
    lim = (lane_width - vehicle_width) / 0.6
    n = 0
    while n < cap and float(n) < lim:
        n += 1
    return n
