"""The packed streamed fetch in plain Python floats, written from DESIGN.md §4r (shared by the CPU and GPU tests of
tests/test_packed_fetch.py): how a tick's PlanOut becomes a PackedPlan, and how its GridOut, path cells and SceneIn become a
PackedGrid - the winner's control points included, which this model computes by itself from the rule of DESIGN §5 - and the
cubic Bezier the host evaluates from them.  Python floats are IEEE doubles and every expression below is written in the order
§4r gives, so +, -, *, / and sqrt round as in the library; sin, cos and atan are the C library's.
"""
import math

import numpy as np

# direction code d -> (dx, dy)
STEPS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
CODE = {s: d for d, s in enumerate(STEPS)}
PATH_POINTS = 200
NONE, LATTICE, PATH, BAD = 0, 1, 2, 4
G_FOUND = 0

PLAN_RESULT = ("brakedis", "brake_speed", "desacc", "desspd", "desstr", "radius", "cnt", "APA", "desaccVd", "desstrVd", "light", "road_type", "sstop")
PLAN_SHOW = ("near_ob_dist", "planspeed", "planacc", "afresh_cause", "trafficlight")
GRID_HEAD = ("order_digest", "status", "n_expanded", "n_pushed", "n_rounds", "path_len", "path_cost", "start_cell", "goal_cell", "best_candidate", "n_candidates")


def pack_plan(dm, po):
    """One PlanOut record -> one PackedPlan record."""
    pk = np.zeros(1, dm.PackedPlan)[0]
    for f in PLAN_RESULT:
        pk[f] = po["result"][f]
    for f in PLAN_SHOW:
        pk[f] = po["show"][f]
    pk["ob_flag"] = po["ob_flag"]
    pk["dec"] = po["dec"]
    pk["path_points"] = po["show"]["path_points"]
    return pk


def _road_angle(pi, eps, a, b):
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


def prefix_steps(cfg, status, path_len):
    """a of DESIGN §5: the last cell of the path prefix the scoring pass reads."""
    if status != G_FOUND or path_len < 1:
        return 0
    return min(path_len - 1, int(cfg["lookahead_cells"][0]), PATH_POINTS - 1)


def cell_centre(cfg, org, cell):
    W, size = int(cfg["grid_w"][0]), float(cfg["cell"][0])
    return (org[0] + (float(cell % W) + 0.5) * size, org[1] + (float(cell // W) + 0.5) * size)


def control_points(cfg, si, path, status, path_len, k):
    """x0 y0 x1 y1 x2 y2 x3 y3 of lattice candidate k."""
    pi, eps, step = float(cfg["PI"][0]), float(cfg["EPSILON"][0]), float(cfg["lattice_step"][0])
    nl = min(int(cfg["n_lattice"][0]), 16)
    ex, ey, edir = (float(si["loc"]["globalpoint"][f]) for f in ("x", "y", "dir"))
    org = (float(si["grid_origin"]["x"]), float(si["grid_origin"]["y"]))
    if status == G_FOUND and path_len >= 1:
        a = prefix_steps(cfg, status, path_len)
        a0 = max(a - 4, 0)
        T = cell_centre(cfg, org, int(path[a]))
        th = edir if a0 == a else _road_angle(pi, eps, cell_centre(cfg, org, int(path[a0])), T)
    else:
        T = (float(si["goal"]["x"]), float(si["goal"]["y"]))
        th = _road_angle(pi, eps, (ex, ey), T)
    a0_, aT = edir * pi / 180, th * pi / 180
    c0, s0, cs, sn = math.cos(a0_), math.sin(a0_), math.cos(aT), math.sin(aT)
    off = float(k - (nl - 1) // 2) * step
    x3, y3 = T[0] + off * sn, T[1] + off * (-cs)
    dx, dy = x3 - ex, y3 - ey
    d = math.sqrt(dx * dx + dy * dy) / 3
    return [ex, ey, ex + d * c0, ey + d * s0, x3 - d * cs, y3 - d * sn, x3, y3]


def bezier_points(geo, n=PATH_POINTS):
    """The n points of the cubic Bezier with control points geo, as bezier_point evaluates them: (n, 2) float64."""
    x0, y0, x1, y1, x2, y2, x3, y3 = (float(v) for v in geo)
    out = np.zeros((n, 2))
    for i in range(n):
        t = float(i) / float(n - 1) if n > 1 else 0.0
        u = 1 - t
        b0, b1, b2, b3 = u * u * u, 3 * u * u * t, 3 * u * t * t, t * t * t
        out[i, 0] = b0 * x0 + b1 * x1 + b2 * x2 + b3 * x3
        out[i, 1] = b0 * y0 + b1 * y1 + b2 * y2 + b3 * y3
    return out


def pack_grid(dm, cfg, si, go, path):
    """One GridOut record, the path cells of its search (at least path_len of them) and the SceneIn record the tick read -> one
    PackedGrid record."""
    pk = np.zeros(1, dm.PackedGrid)[0]
    for f in GRID_HEAD:
        pk[f] = go[f]
    nc, best = int(go["n_candidates"]), int(go["best_candidate"])
    status, path_len = int(go["status"]), int(go["path_len"])
    nl = min(int(cfg["n_lattice"][0]), 16)
    W = int(cfg["grid_w"][0])
    if nc <= 0:
        return pk                                                  # kind 0: everything behind the header is 0
    for f in ("cost", "col", "curv", "prog"):
        pk["best_" + f] = go["cand_" + f][best]
    if best < nl:
        pk["kind"] = LATTICE
        pk["geo"] = control_points(cfg, si, path, status, path_len, best)
        return pk
    kind = PATH
    a = prefix_steps(cfg, status, path_len)
    pk["n_steps"] = a
    pk["geo"][0], pk["geo"][1] = si["grid_origin"]["x"], si["grid_origin"]["y"]
    planes = [0] * 12
    if int(path[0]) != int(go["start_cell"]):
        kind |= BAD
    for i in range(a):
        p0, p1 = int(path[i]), int(path[i + 1])
        d = CODE.get((p1 % W - p0 % W, p1 // W - p0 // W))
        if d is None:
            kind |= BAD
            continue
        for b in range(3):
            if (d >> b) & 1:
                planes[3 * (i >> 6) + b] |= 1 << (i & 63)
    pk["kind"] = kind
    pk["planes"] = np.array(planes, np.uint64)
    return pk


def step_codes(pk):
    """The direction codes of a kind-2 record's n_steps steps."""
    pl = [int(v) for v in pk["planes"]]
    return [sum(((pl[3 * (i >> 6) + b] >> (i & 63)) & 1) << b for b in range(3)) for i in range(int(pk["n_steps"]))]


def masked_grid_out(go):
    """GridOut records as pp_unpack_grid delivers them: cand_*[k] = 0 for k != best_candidate (a new 1-D array)."""
    out = np.array(go, copy=True).reshape(-1)
    idx, best, some = np.arange(len(out)), out["best_candidate"].astype(np.int64), out["n_candidates"] > 0
    for f in ("cand_cost", "cand_col", "cand_curv", "cand_prog"):
        keep = np.where(some, out[f][idx, best], 0.0)
        out[f][:] = 0
        out[f][idx, best] = keep
    return out
