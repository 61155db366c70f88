"""The fleet coupling step in plain numpy, written from DESIGN.md §4e (not from the kernel).

`couple` is what one k_couple_fleet launch does to one input set: the SceneIn records, the obstacle pool and (if the set
carries one) the motion pool in; copies of them with the peer slots filled and obs_off / obs_n set out.  numpy float64 is the
IEEE double, every expression is evaluated left to right as the specification writes it and each numpy operation rounds
once, and the order (d2, p) is total, so the result is meant to equal the device's byte for byte."""
import numpy as np

OB_PEER = 0x40000000


def candidates(rng, K, x, y, px, py, members, s):
    """§4e 1. - 3. for scene `s`: the scene indices of its peers, nearest first, at most K.  members: the scene indices of
    its world (increasing); px, py: the positions of those members."""
    if K <= 0 or not (np.isfinite(x) and np.isfinite(y)):
        return []
    dx = px - x
    dy = py - y
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = dx * dx + dy * dy
        ok = (d2 <= rng * rng) & (members != s)          # (a NaN compares false)
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return []
    order = np.lexsort((members[idx], d2[idx]))           # by d2, ties by scene index
    return [int(members[idx[k]]) for k in order[:K]]


def couple(fm, world_first, pinned_off, n_own, si, obs_pool, mot_pool=None):
    """fm: a FleetModel record (range, radius, max_peers); world_first: n_worlds + 1 scene indices; pinned_off / n_own: the
    pinned slice of every scene.  Returns (si', obs_pool', mot_pool') - mot_pool' is None without a motion pool."""
    fm = np.asarray(fm).reshape(-1)[0]
    rng, radius, K = float(fm["range"]), np.float32(fm["radius"]), int(fm["max_peers"])
    out, obs = si.copy(), obs_pool.copy()
    mot = None if mot_pool is None else mot_pool.copy()
    X = np.ascontiguousarray(si["loc"]["globalpoint"]["x"], np.float64)
    Y = np.ascontiguousarray(si["loc"]["globalpoint"]["y"], np.float64)
    for w in range(len(world_first) - 1):
        a, b = int(world_first[w]), int(world_first[w + 1])
        members = np.arange(a, b)
        px, py = X[a:b], Y[a:b]
        for s in range(a, b):
            peers = candidates(rng, K, X[s], Y[s], px, py, members, s)
            base = int(pinned_off[s]) + int(n_own[s])
            for k, p in enumerate(peers):
                o = obs[base + k]
                o["x"], o["y"], o["type"], o["radius"] = X[p], Y[p], OB_PEER | p, radius
                if mot is not None:
                    mot[base + k]["vx"], mot[base + k]["vy"] = 0.0, 0.0
            out["obs_off"][s], out["obs_n"][s] = int(pinned_off[s]), int(n_own[s]) + len(peers)
    return out, obs, mot
