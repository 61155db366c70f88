"""Car-following traffic in plain numpy, written from DESIGN.md §4i (not from the kernel).

`Follow` is tests/traffic_model.py's `Traffic` - the tracks, the cumulative lengths, the arc length `s` of every actor and §4h's
`place` (pp_set_traffic, pp_update_async) - plus a speed `v` per actor and `step`: what one k_follow_traffic launch does to one
staged obstacle pool, given the SceneIn records and ego flag words of the set being staged.  numpy float64 is the IEEE double,
every expression is evaluated left to right as the specification writes it and each operation rounds once; the two orders
(g_b, b) and (d2_k, k) are total, so the result is meant to equal the device's byte for byte.

`step` also records, per actor, which branch it took (`info`): the tests assert the branch beside the bytes, so that a case that
silently stops exercising its edge fails."""
import numpy as np

import traffic_model as tm

FIELDS = ("look", "lateral", "gap", "headway", "max_acc", "comfort_dec", "max_dec", "min_net")
DEFAULT = (60.0, 1.5, 2.0, 1.5, 1.0, 2.0, 6.0, 0.1)


def params(tf=None, **kw):
    """The eight fields as a dict of float64: from a TrafficFollow record, a dict (over the defaults), or the defaults; keywords replace fields."""
    if tf is None:
        p = dict(zip(FIELDS, DEFAULT))
    elif isinstance(tf, dict):
        p = dict(zip(FIELDS, DEFAULT), **tf)
    else:
        rec = np.asarray(tf).reshape(-1)[0]
        p = {k: rec[k] for k in FIELDS}
    p.update(kw)
    return {k: np.float64(p[k]) for k in FIELDS}


class Info:
    """What §4i did for one actor in one step.  kind: 'plain' (!(speed > 0): §4h's step), 'free', 'actor', 'ego'."""

    def __init__(self, kind):
        self.kind, self.leader, self.g, self.net, self.dyn, self.acc = kind, -1, None, None, None, None
        self.clamped = self.floored = self.stopped = self.wrapped = False
        self.n_members = self.n_actor_candidates = self.window = 0
        self.kstar, self.d2, self.actor_g, self.ego_g, self.vl = -1, None, None, None, None


def idm(p, v, speed, radius, lead, info):
    """§4i 4.: the acceleration of a follower at speed v that wants `speed`, behind lead = (kind, g, vl, rl, index) or None."""
    r = v / speed
    r2 = r * r
    free = 1 - r2 * r2
    if lead is None:
        acc = p["max_acc"] * free
    else:
        info.kind, g, vl, rl, info.leader = lead
        info.g, info.vl = g, vl
        net = g - radius - rl
        if not (net > p["min_net"]):
            net, info.floored = p["min_net"], True
        dv = v - vl
        c2 = 2 * np.sqrt(p["max_acc"] * p["comfort_dec"])
        dyn = v * p["headway"] + (v * dv) / c2
        if not (dyn > 0):
            dyn = np.float64(0.0)
        star = p["gap"] + dyn
        q = star / net
        acc = p["max_acc"] * (free - q * q)
        info.net, info.dyn = net, dyn
    if not (acc >= -p["max_dec"]):                               # (a NaN brakes)
        acc, info.clamped = -p["max_dec"], True
    info.acc = acc
    return acc


def ego_speed(scene_in, flags, c):
    """§4i 2.: vl_e of scene c's ego - a frozen ego stands."""
    return np.float64(0.0) if int(flags[c]) != 0 else np.float64(scene_in["loc"]["velocity"][c]) / np.float64(3.6)


class Follow(tm.Traffic):
    def __init__(self, tracks, points, actors, obs_off):
        super().__init__(tracks, points, actors, obs_off)
        self.reset_speed()
        groups = {}
        for a, A in enumerate(self.actors):
            groups.setdefault((int(A["scene"]), int(A["track"])), []).append(a)
        self.groups = {k: np.array(v, np.int64) for k, v in groups.items()}          # (indices rise within a group)
        self.info = []

    def reset_speed(self):
        """pp_set_traffic while following is on, pp_set_traffic_follow(non-NULL) while traffic is on: v = speed."""
        self.v = np.ascontiguousarray(self.actors["speed"], np.float64).copy()

    # §4i 1.: (g, b) of the actor leader, or None
    def _actor_leader(self, a, k, closed, L, look, s, info):
        grp = self.groups[(int(self.actors["scene"][a]), k)]
        b = grp[grp != a]
        info.n_members = len(grp)
        if len(b) == 0:
            return None
        with np.errstate(all="ignore"):
            g = s[b] - s[a]
            if closed:
                g = np.where((g < 0) | ((g == 0) & (b > a)), g + L, g)
                cand = np.ones(len(b), bool)
            else:
                cand = (g > 0) | ((g == 0) & (b < a))
            cand &= g <= look                                    # (a NaN compares false)
        info.n_actor_candidates = int(cand.sum())
        if not cand.any():
            return None
        g, b = g[cand], b[cand]
        m = np.lexsort((b, g))[0]                                # the smallest in the total order (g, b)
        return g[m], int(b[m])

    # §4i 2.: (g_e, k*, d2) of the ego candidate, or None
    def _ego(self, a, k, closed, L, look, lateral, s_a, x, y, info):
        cum, px, py = self.cum[k], self.px[k], self.py[k]
        n = len(px)
        i0 = tm.locate(cum, s_a)
        ks = np.arange(1, (n if closed else n - 1 - i0) + 1, dtype=np.int64)
        if len(ks) == 0:
            return None
        j = i0 + ks
        pj = np.where(j <= n - 1, j, j - n)
        with np.errstate(all="ignore"):
            g = np.where(j <= n - 1, cum[pj] - s_a, (L - s_a) + cum[pj])
            part = g <= look
            info.window = int(part.sum())
            assert part[:info.window].all()                      # (g never decreases with k: the vertices that take part are a prefix)
            ex, ey = px[pj] - x, py[pj] - y
            d2 = ex * ex + ey * ey
            ok = np.flatnonzero(part & ~np.isnan(d2))            # (a NaN is never the minimum)
            if len(ok) == 0:
                return None
            m = ok[np.argmin(d2[ok])]                            # (argmin: the FIRST index of the smallest)
            info.kstar, info.d2 = int(ks[m]), d2[m]
            if not (d2[m] <= lateral * lateral):
                return None
        return g[m], int(ks[m]), d2[m]

    # §4i 2. - 3.: (g_e, vl_e) of the ego that may lead actor a - the ego of its own scene - or None
    def _ego_leader(self, a, k, closed, L, p, s_a, scene_in, flags, info):
        c = int(self.actors["scene"][a])
        gp = scene_in["loc"]["globalpoint"][c]
        eg = self._ego(a, k, closed, L, p["look"], p["lateral"], s_a, np.float64(gp["x"]), np.float64(gp["y"]), info)
        return None if eg is None else (eg[0], ego_speed(scene_in, flags, c))

    def step(self, obs_pool, mot_pool, dt, tf, scene_in, flags, vehicle_width):
        """One k_follow_traffic launch on one staged set: returns (obs_pool', mot_pool'), updates self.s, self.v, self.info.
        scene_in: the SceneIn records BEING staged (loc.globalpoint, loc.velocity are read); flags: the ego flag words as staged."""
        p = params(tf)
        dt = np.float64(dt)
        obs = obs_pool.copy()
        mot = None if mot_pool is None else mot_pool.copy()
        s0, v0s = self.s.copy(), self.v.copy()                   # Jacobi: everybody reads the state before this advance
        self.info = []
        half_w = np.float64(0.5) * np.float64(vehicle_width)
        for a, A in enumerate(self.actors):
            k = int(A["track"])
            closed = int(self.tracks["closed"][k]) != 0
            L = self.cum[k][-1]
            speed = np.float64(A["speed"])
            with np.errstate(all="ignore"):
                if not (speed > 0):                              # parked or reversing: §4h's step, v = speed
                    info = Info("plain")
                    (raw, s1), v1 = self._plain(a, s0[a], dt), speed
                else:
                    info = Info("free")
                    v = v0s[a]
                    lead = None
                    al = self._actor_leader(a, k, closed, L, p["look"], s0, info)          # 1.
                    if al is not None:
                        info.actor_g = al[0]
                        lead = ("actor", al[0], v0s[al[1]], np.float64(self.actors["radius"][al[1]]), al[1])
                    el = self._ego_leader(a, k, closed, L, p, s0[a], scene_in, flags, info)          # 2.
                    if el is not None:
                        info.ego_g = el[0]
                        if lead is None or el[0] <= lead[1]:     # 3.: the ego wins a tie
                            lead = ("ego", el[0], el[1], half_w, -1)
                    acc = idm(p, v, speed, np.float64(A["radius"]), lead, info)          # 4.
                    v1 = v + acc * dt                            # 5.
                    if not (v1 > 0):
                        v1, info.stopped = np.float64(0.0), True
                    raw = s0[a] + 0.5 * (v + v1) * dt
                    s1 = tm.wrap(raw, L, closed)
                info.wrapped = bool(s1 != raw)
            self.s[a], self.v[a] = s1, v1
            self.info.append(info)
            self._write(obs, mot, a, s1)
        return obs, mot
