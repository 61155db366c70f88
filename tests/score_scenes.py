"""Crafted scenes for the scoring pass (G3; `score_body` of csrc/kernels_score.hpp) and the form the kernel takes
for each of them (shared by the CPU and GPU tests of tests/test_score_edges.py).

Base geometry: 128 x 128 cells of 0.25 m, default config, ego at origin + (3, 16), goal at origin + (29, 16), heading 25
degrees unless a case says otherwise, a line of k discs of radius 0.1 at y = 19.2 with x from 6 to 26.  Obstacles are static
and the motion pool is zero.  Every scene of a batch has the same `n_obs` (the pools are laid out as `gen_scenes` does): the
near obstacles come LAST in a scene's list, behind padding discs that lie outside the grid and outside every cull box.

`forms()` restates the kernel's case split from the rule in the header comment of kernels_score.hpp and DESIGN §7 "k_score in
detail" - which obstacles survive the cull, whether the scene is bucketed and from where, the fullest bucket - with the
kernel's constants read from its sources by pattern (`kernel_constants()`), so that a later change to a constant fails the
coverage test of test_score_edges.py instead of silently hollowing the cases out."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "decision-making-and-path-planning_amd", "csrc")

GRID = 128
EGO = (3.0, 16.0)
GOAL = (29.0, 16.0)
HEADING = 25.0
PAD = (-40.0, -40.0)          # padding discs: from here towards -x, half a metre apart, radius 0.1


def line(k):
    """k discs of radius 0.1 at y = 19.2, x from 6 to 26."""
    if k == 0:
        return []
    if k == 1:
        return [(16.0, 19.2, 0.1)]
    return [(6.0 + 20.0 * i / (k - 1), 19.2, 0.1) for i in range(k)]


def clump(k):
    """k discs 0.01 m apart: all of them land in the same buckets."""
    return [(16.0 + 0.01 * i, 18.6, 0.1) for i in range(k)]


# name -> (ego heading in degrees, near discs (x, y, r) relative to the grid origin, goal relative to the grid origin)
CASES = {
    "n_rel_0":      (HEADING, line(0), GOAL),
    "n_rel_7":      (HEADING, line(7), GOAL),
    "n_rel_8":      (HEADING, line(8), GOAL),
    "n_rel_128":    (HEADING, line(128), GOAL),
    "n_rel_129":    (HEADING, line(129), GOAL),
    "clump_12":     (HEADING, clump(12), GOAL),
    "clump_13":     (HEADING, clump(13), GOAL),
    "tail":         (HEADING, [(29.6, 14.9, 0.1)], GOAL),
    "wall":         (HEADING, [(16.0, 16.0, 1.0)], GOAL),
    "detour":       (0.0, [(16.0, 16.0, 3.0), (16.0, 22.2, 0.1), (16.0, 9.8, 0.1)], GOAL),
    # the detour with its north pebble over the stretch of the path where nothing else is near: the path candidate's penalty there
    # is this pebble's alone, and only the box of the path's cells keeps it in the cull (beside the big disc the pebble above never is
    # the nearest obstacle of a point)
    "detour_west":  (0.0, [(16.0, 16.0, 3.0), (9.0, 22.2, 0.1), (16.0, 9.8, 0.1)], GOAL),
    "blocked_goal": (HEADING, [(29.0, 16.0, 1.0)], GOAL),
    "goal_is_ego":  (HEADING, line(0), EGO),
    "tie":          (0.0, line(9), GOAL),
    # 129 near obstacles of which 100 lie just inside the lower edge of the grown cull box and touch the lowest bucket row alone:
    # not culled, and the buckets the candidates' points read hold 1 .. kBucketCap entries - indices 227 .. 255 of the snapshot
    "light_buckets": (HEADING, [(4.0 + 24.0 * i / 99, 11.8, 0.1) for i in range(100)] + line(29), GOAL),
}
CASE_NAMES = list(CASES)
BASE = "n_rel_7"                       # the scene the n_lattice and lookahead_cells sweeps run on
BATCH_N_OBS = (256, 300)               # 256: a scene that is not culled is bucketed from the snapshot; 300: the plain HBM loop
EDGE_CASE = ("n_rel_129", 257)         # run alone: the first obstacle count beyond the snapshot buckets


def config(dm):
    cfg = dm.default_config(GRID)
    cfg["dynamic_obstacles"] = 0
    return cfg


def build(dm, cfg, names, n_obs):
    """One scene per entry of `names` (a case may repeat), `n_obs` obstacles each: padding first, the case's discs last."""
    n = len(names)
    sc = dm.gen_scenes(cfg, 0, n, n_obs, junction_every=0)
    si = sc["scene_in"]
    sc["mot_pool"][:] = 0
    for s, name in enumerate(names):
        heading, discs, goal = CASES[name]
        assert len(discs) <= n_obs, (name, len(discs), n_obs)
        assert int(si["obs_off"][s]) == s * n_obs and int(si["obs_n"][s]) == n_obs
        ox, oy = float(si["grid_origin"]["x"][s]), float(si["grid_origin"]["y"][s])
        n_pad = n_obs - len(discs)
        rows = [(PAD[0] - 0.5 * i, PAD[1], 0.1) for i in range(n_pad)] + list(discs)
        ob = sc["obs_pool"][s * n_obs:(s + 1) * n_obs]
        for j, (x, y, r) in enumerate(rows):
            ob[j]["x"], ob[j]["y"], ob[j]["radius"], ob[j]["type"] = ox + x, oy + y, r, 0
        gp = si["loc"]["globalpoint"]
        gp["x"][s], gp["y"][s], gp["dir"][s] = ox + EGO[0], oy + EGO[1], heading
        si["goal"]["x"][s], si["goal"]["y"][s] = ox + goal[0], oy + goal[1]
    return sc


def scene_obstacles(sc, s):
    si = sc["scene_in"]
    return sc["obs_pool"][int(si["obs_off"][s]):int(si["obs_off"][s]) + int(si["obs_n"][s])]


# ---- the kernel's constants, read from its sources -------------------------------------------------------------------
def kernel_constants():
    """kMaxRelObs, kBucketN, kBucketCap, kBucketMinObs of kernels_score.hpp and kScoreWideMaxScenes of dmpp_hip.hip."""
    out = {}
    with open(os.path.join(CSRC, "kernels_score.hpp")) as f:
        score = f.read()
    with open(os.path.join(CSRC, "dmpp_hip.hip")) as f:
        host = f.read()
    for name, text in (("kMaxRelObs", score), ("kBucketN", score), ("kBucketCap", score), ("kBucketMinObs", score),
                       ("kScoreWideMaxScenes", host)):
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)\s*[,;]", text)
        if m is None:
            raise AssertionError(f"constant {name} not found in the kernel sources: the form table cannot be computed")
        out[name] = int(m.group(1))
    m = re.search(r"bucketed\s*=\s*culled\s*\?\s*n_rel\s*>=\s*kBucketMinObs\s*:\s*m\s*<=\s*(\d+)\s*;", score)
    if m is None:
        raise AssertionError("the bucketing rule of score_body was not found in kernels_score.hpp")
    out["snapshot_bucket_max"] = int(m.group(1))
    return out


# ---- which form score_body takes for a scene ----------------------------------------------------------------------------
def _road_angle(cfg, a, b):
    pi, eps = float(cfg["PI"][0]), float(cfg["EPSILON"][0])
    dx, dy = b[0] - a[0], b[1] - a[1]
    if abs(dx) < eps and abs(dy) < eps:
        ang = 0.0
    elif abs(dx) < eps:
        ang = pi / 2 if dy > 0 else 3 * pi / 2
    else:
        ang = math.atan(dy / dx)
        if dx < 0:
            ang += pi
        elif dy < 0:
            ang += 2 * pi
    return ang * 180 / pi


def forms(cfg, si, obs, path, status, k=None):
    """The case split of score_body for one scene (float64; the crafted discs keep well away from every box edge, so the
    counts do not hang on a rounding).  `si`: one SceneIn record, `obs`: the scene's effective obstacles, `path` / `status`: the
    search's result.  Returns n_rel, culled, bucketed, fullest (largest bucket fill, 0 when not bucketed), form, and the
    path prefix `a`, `nc`, the cull box and - for the detour's claim - the box of the lattice hulls alone."""
    k = k or kernel_constants()
    W, cell = int(cfg["grid_w"][0]), float(cfg["cell"][0])
    pi = float(cfg["PI"][0])
    half_w, d_safe, step = 0.5 * float(cfg["Vehicle_Width"][0]), float(cfg["d_safe"][0]), float(cfg["lattice_step"][0])
    gx, gy = float(si["grid_origin"]["x"]), float(si["grid_origin"]["y"])
    ex, ey, edir = (float(si["loc"]["globalpoint"][f]) for f in ("x", "y", "dir"))
    have_path = status == 0 and path is not None and len(path) >= 1
    nl = min(int(cfg["n_lattice"][0]), 16)
    nc = nl + (1 if have_path else 0)
    centre = lambda c: (gx + (c % W + 0.5) * cell, gy + (c // W + 0.5) * cell)
    a = 0
    if have_path:
        a = min(len(path) - 1, int(cfg["lookahead_cells"][0]), 199)
        T = centre(int(path[a]))
        a0 = max(a - 4, 0)
        thT = edir if a0 == a else _road_angle(cfg, centre(int(path[a0])), T)
    else:
        T = (float(si["goal"]["x"]), float(si["goal"]["y"]))
        thT = _road_angle(cfg, (ex, ey), T)
    X0 = Y0 = math.inf
    X1 = Y1 = -math.inf
    c0, s0 = math.cos(edir * pi / 180), math.sin(edir * pi / 180)
    cs, sn = math.cos(thT * pi / 180), math.sin(thT * pi / 180)
    for q in range(nl):
        off = (q - (nl - 1) // 2) * step
        x3, y3 = T[0] + off * sn, T[1] - off * cs
        d = math.hypot(x3 - ex, y3 - ey) / 3
        xs = (ex, ex + d * c0, x3 - d * cs, x3)
        ys = (ey, ey + d * s0, y3 - d * sn, y3)
        X0, X1, Y0, Y1 = min(X0, *xs), max(X1, *xs), min(Y0, *ys), max(Y1, *ys)
    hull = (X0, X1, Y0, Y1)
    if have_path:
        cells = np.asarray(path[:a + 1], np.int64)
        cx, cy = cells % W, cells // W
        X0, X1 = min(X0, gx + (cx.min() - 0.5) * cell), max(X1, gx + (cx.max() + 1.5) * cell)
        Y0, Y1 = min(Y0, gy + (cy.min() - 0.5) * cell), max(Y1, gy + (cy.max() + 1.5) * cell)
    m = len(obs)
    ox, oy, r = obs["x"].astype(np.float64), obs["y"].astype(np.float64), obs["radius"].astype(np.float64)
    thr = r + half_w + d_safe
    near = (ox >= X0 - thr) & (ox <= X1 + thr) & (oy >= Y0 - thr) & (oy <= Y1 + thr)
    n_rel = int(near.sum())
    culled = n_rel <= k["kMaxRelObs"]
    bucketed = n_rel >= k["kBucketMinObs"] if culled else m <= k["snapshot_bucket_max"]
    fullest, fill_at = 0, lambda x, y: 0
    if bucketed:
        nb = k["kBucketN"]
        cnt = np.zeros((nb, nb), np.int64)
        ibx = nb / (X1 - X0) if X1 > X0 else 0.0
        iby = nb / (Y1 - Y0) if Y1 > Y0 else 0.0
        def sat(q):                       # the device's conversion: a NaN is 0, beyond int the nearest end - then the clamp
            return 0 if q != q else int(min(max(q, 0.0), nb - 1.0))
        bx = lambda v: sat(math.floor((v - X0) * ibx) if math.isfinite((v - X0) * ibx) else (v - X0) * ibx)
        by = lambda v: sat(math.floor((v - Y0) * iby) if math.isfinite((v - Y0) * iby) else (v - Y0) * iby)
        for j in (np.flatnonzero(near) if culled else range(m)):
            t = thr[j] * (1.0 + 1e-9) + 1e-9
            if not (ox[j] >= X0 - t and ox[j] <= X1 + t and oy[j] >= Y0 - t and oy[j] <= Y1 + t):
                continue
            cnt[by(oy[j] - t):by(oy[j] + t) + 1, bx(ox[j] - t):bx(ox[j] + t) + 1] += 1
        fullest = int(cnt.max())
        fill_at = lambda x, y: int(cnt[by(y), bx(x)])          # entries of the bucket a point at (x, y) reads
    if culled:
        form = "lds_buckets" if bucketed else "lds_plain"
    else:
        form = "snapshot_buckets" if bucketed else "hbm_plain"
    return dict(n_rel=n_rel, m=m, culled=culled, bucketed=bucketed, fullest=fullest, form=form,
                overflow=bucketed and fullest > k["kBucketCap"], a=a, nc=nc, have_path=have_path, box=(X0, X1, Y0, Y1), hull=hull,
                fill_at=fill_at, first_near=int(np.flatnonzero(near)[0]) if n_rel else -1)


def schedule(nw, nc):
    """How score_body deals nc candidates to nw waves: (whole rounds, left-over candidates split by quarters, packed pass)."""
    left = nc % nw
    n_whole = nc - left if 4 * left <= nw else nc
    rounds = (n_whole + nw - 1) // nw
    return dict(rounds=rounds, split=nc - n_whole, packed=nw <= 4 and 2 <= rounds <= 4)
