"""Traffic manoeuvres in plain numpy, written from DESIGN.md §4v (not from the kernel).

`Manoeuvres` is tests/traffic_follow_model.py's `Follow` - the tracks, the cumulative lengths, `s` and `v` of every actor - plus one
TrafficManoeuvreState per actor (`st`, a structured array with the fields of the C record) and the record list.  `advance` is what
one k_manoeuvre_traffic launch does to one staged obstacle pool in pp_advance_async, `update` what it does with step = 0
(pp_update_async, the set call), `restart` what k_reset_manoeuvres does behind §4m's reset.  tf None: following off.  numpy float64
is the IEEE double, every expression is evaluated left to right as the section writes it and each operation rounds once; every
order is total, so the result is meant to equal the device's byte for byte.

`advance` records per actor what happened (`info`: fired, projected onto (j*, segment), finished, and the §4i Info of the step), so
that a test can assert that a case reaches the edge it was built for."""
import types

import numpy as np

import traffic_follow_model as fm
import traffic_model as tm

ADVANCES, EGO_DIST, EGO_TIME = 0, 1, 2
STATE = np.dtype([("lat", "<f8"), ("lat0", "<f8"), ("v0", "<f8"), ("track", "<i4"), ("next", "<i4"), ("k", "<i4"), ("clock", "<i4"), ("n_done", "<i4"), ("_pad", "<i4")])
RECORD = np.dtype([("dist", "<f8"), ("time", "<f8"), ("lat_end", "<f8"), ("speed", "<f8"), ("actor", "<i4"), ("trigger", "<i4"), ("after", "<i4"), ("track", "<i4"),
                   ("n_steps", "<i4"), ("_pad", "<i4")])
MANOEUVRE_MAX = 8
I32_MAX = 2 ** 31 - 1


def record(actor, kind=ADVANCES, side=0, dist=0.0, time=0.0, lat_end=0.0, speed=np.nan, after=0, track=-1, n_steps=1):
    r = np.zeros(1, RECORD)
    r["actor"], r["trigger"], r["dist"], r["time"], r["lat_end"], r["speed"] = actor, kind | (side << 8), dist, time, lat_end, speed
    r["after"], r["track"], r["n_steps"] = after, track, n_steps
    return r


def records(*rows):
    return np.concatenate(rows) if rows else np.zeros(0, RECORD)


def check(n_actors, n_tracks, recs):
    """pp_check_traffic_manoeuvres: -1 when the list is legal, else the index of the first record that is not."""
    prev, run = 0, 0
    for i, m in enumerate(recs):
        actor, trig = int(m["actor"]), int(m["trigger"])
        if i > 0 and actor != prev:
            run = 0
        kind, side = trig & 255, trig >> 8
        ok = 0 <= actor < n_actors and actor >= (prev if i else 0) and run < MANOEUVRE_MAX and -1 <= int(m["track"]) < n_tracks
        ok = ok and trig >= 0 and kind <= EGO_TIME and side <= 2 and not (side != 0 and kind == ADVANCES)
        ok = ok and not (kind == EGO_DIST and not (np.isfinite(m["dist"]) and m["dist"] >= 0))
        ok = ok and not (kind == EGO_TIME and not (np.isfinite(m["time"]) and m["time"] >= 0))
        ok = ok and bool(np.isfinite(m["lat_end"])) and not np.isinf(m["speed"]) and int(m["after"]) >= 0 and 1 <= int(m["n_steps"]) <= 4096 and int(m["_pad"]) == 0
        if not ok:
            return i
        prev, run = actor, run + 1
    return -1


def foot(px, py, i, x, y):
    """§4v start: the foot of (x, y) on segment i with the parameter clamped to [0, 1]: (f2, t, lat0), or None for a segment without a length."""
    n = len(px)
    j = i + 1 if i + 1 < n else 0
    with np.errstate(all="ignore"):
        dx, dy = px[j] - px[i], py[j] - py[i]
        l2 = dx * dx + dy * dy
        if not (l2 > 0):
            return None
        ax, ay = x - px[i], y - py[i]
        t = (ax * dx + ay * dy) / l2
        if not (t >= 0):
            t = np.float64(0.0)
        if t > 1:
            t = np.float64(1.0)
        fx, fy = px[i] + t * dx, py[i] + t * dy
        gx, gy = x - fx, y - fy
        return gx * gx + gy * gy, t, (dx * ay - dy * ax) / np.sqrt(l2)


def project(px, py, cum, closed, x, y):
    """§4v start: the pose (x, y) onto a track: (s, lat0, j*, segment or -1), or None when no vertex has a distance."""
    n = len(px)
    nseg = n if closed else n - 1
    with np.errstate(all="ignore"):
        ex, ey = px - x, py - y
        d2 = ex * ex + ey * ey
    ok = np.flatnonzero(~np.isnan(d2))
    if len(ok) == 0:
        return None
    j = int(ok[np.argmin(d2[ok])])                               # (argmin: the FIRST index of the smallest)
    before = j - 1 if j > 0 else (n - 1 if closed else -1)
    behind = j if j < nseg else -1
    best = None
    for i in sorted(k for k in (before, behind) if k >= 0):      # the earlier segment first; the later one only if strictly nearer
        f = foot(px, py, i, x, y)
        if f is not None and not np.isnan(f[0]) and (best is None or f[0] < best[0]):
            best = f + (i,)
    with np.errstate(all="ignore"):
        if best is None:
            s, lat0, seg = cum[j], np.float64(0.0), -1
        else:
            _, t, lat0, seg = best
            s = cum[seg] + t * (cum[seg + 1] - cum[seg])
    return tm.wrap(s, cum[-1], closed), lat0, j, seg


class Manoeuvres(fm.Follow):
    def __init__(self, tracks, points, actors, obs_off, recs):
        super().__init__(tracks, points, actors, obs_off)
        self.records = np.array(recs, RECORD).reshape(-1).copy()
        assert check(len(self.actors), len(self.tracks), self.records) == -1
        self.run = [np.flatnonzero(self.records["actor"] == a) for a in range(len(self.actors))]
        self.set_states()
        self.minfo = []

    def set_states(self):
        """pp_set_traffic_manoeuvres: { 0, 0, speed, pin.track, 0, 0, 0, 0 }."""
        self.st = np.zeros(len(self.actors), STATE)
        self.st["v0"], self.st["track"] = self.actors["speed"], self.actors["track"]

    def set_follow(self):
        """pp_set_traffic_follow(non-NULL): the states stay, v = v0."""
        self.v = self.st["v0"].copy()

    def restart(self, scenes):
        """k_reset_manoeuvres: the actors of the scenes that restarted go back to the state of the set call; n_done is kept."""
        for a in np.flatnonzero(np.isin(self.actors["scene"], scenes)):
            done = self.st["n_done"][a]
            self.st[a] = np.zeros(1, STATE)[0]
            self.st["v0"][a], self.st["track"][a], self.st["n_done"][a] = self.actors["speed"][a], self.actors["track"][a], done

    # §4v pose: (x, y, dx, dy) of arc length s on track k with offset lat
    def pose(self, k, s, lat):
        px, py, cum = self.px[k], self.py[k], self.cum[k]
        i, _, x, y = tm.point_at(px, py, cum, s)
        j = i + 1 if i + 1 < len(px) else 0
        with np.errstate(all="ignore"):
            dx, dy = px[j] - px[i], py[j] - py[i]
            if lat != 0:
                ln = np.sqrt(dx * dx + dy * dy)
                if ln > 0:
                    nx, ny = -dy / ln, dx / ln
                    x, y = x + lat * nx, y + lat * ny
        return x, y, dx, dy

    def _store(self, obs, mot, a, k, s, lat):
        A = self.actors[a]
        x, y, _, _ = self.pose(k, s, lat)
        o = obs[int(self.pool_index[a])]
        o["x"], o["y"], o["type"], o["radius"] = x, y, A["type"], A["radius"]
        if mot is not None:
            mot[int(self.pool_index[a])]["vx"], mot[int(self.pool_index[a])]["vy"] = 0.0, 0.0

    def update(self, obs_pool, mot_pool=None):
        """step = 0: every actor at its current (s, lat) on its current track; no step, no trigger, no clock."""
        obs = obs_pool.copy()
        mot = None if mot_pool is None else mot_pool.copy()
        for a in range(len(self.actors)):
            self._store(obs, mot, a, int(self.st["track"][a]), self.s[a], self.st["lat"][a])
        return obs, mot

    # §4v step, following: §4i 1. with the scene's actors whose current track in the before-state is k
    def _actor_leader(self, a, k, closed, L, look, s_a, s0, st0, info):
        b = np.flatnonzero((self.actors["scene"] == self.actors["scene"][a]) & (st0["track"] == k))
        b = b[b != a]
        info.n_members = len(b) + 1
        if len(b) == 0:
            return None
        with np.errstate(all="ignore"):
            g = s0[b] - s_a
            if closed:
                g = np.where((g < 0) | ((g == 0) & (b > a)), g + L, g)
                cand = np.ones(len(b), bool)
            else:
                cand = (g > 0) | ((g == 0) & (b < a))
            cand &= g <= look
        info.n_actor_candidates = int(cand.sum())
        if not cand.any():
            return None
        g, b = g[cand], b[cand]
        m = np.lexsort((b, g))[0]
        return g[m], int(b[m])

    def advance(self, obs_pool, mot_pool, dt, tf, scene_in, flags, vehicle_width=None):
        """One k_manoeuvre_traffic launch of an advance: returns (obs_pool', mot_pool'), updates s, v (tf not None), st, minfo."""
        p = None if tf is None else fm.params(tf)
        dt = np.float64(dt)
        obs = obs_pool.copy()
        mot = None if mot_pool is None else mot_pool.copy()
        s0, v0s, st0 = self.s.copy(), self.v.copy(), self.st.copy()          # Jacobi: everybody reads the state before this advance
        half_w = None if p is None else np.float64(0.5) * np.float64(vehicle_width)
        self.minfo = []
        for a, A in enumerate(self.actors):
            st = st0[a].copy()
            mi = types.SimpleNamespace(fired=False, projected=None, finished=False, step=None)
            c = int(A["scene"])
            k, s = int(st["track"]), s0[a]
            run = self.run[a]
            have = 0 <= int(st["next"]) < len(run)
            m = self.records[run[int(st["next"])]] if have else None
            with np.errstate(all="ignore"):
                # trigger
                if have and int(st["k"]) == 0 and int(st["clock"]) >= int(m["after"]):
                    kind, side = int(m["trigger"]) & 255, int(m["trigger"]) >> 8
                    xa, ya, dx, dy = self.pose(k, s, st["lat"])
                    if kind == ADVANCES:
                        mi.fired = True
                    else:
                        gp = scene_in["loc"]["globalpoint"][c]
                        ex, ey = xa - np.float64(gp["x"]), ya - np.float64(gp["y"])
                        d2 = ex * ex + ey * ey
                        if kind == EGO_DIST:
                            r2 = m["dist"] * m["dist"]
                        else:
                            r = m["time"] * fm.ego_speed(scene_in, flags, c)
                            r2 = r * r
                        pr = ex * dx + ey * dy
                        mi.fired = bool(d2 <= r2 and (side == 0 or (side == 1 and pr >= 0) or (side == 2 and pr <= 0)))
                    # start of the move
                    if mi.fired:
                        if not np.isnan(m["speed"]):
                            st["v0"] = m["speed"]
                        st["lat0"] = st["lat"]
                        t2 = int(m["track"])
                        if t2 >= 0 and t2 != k:
                            pj = project(self.px[t2], self.py[t2], self.cum[t2], int(self.tracks["closed"][t2]) != 0, xa, ya)
                            if pj is not None:
                                s, st["lat0"], k = pj[0], pj[1], t2
                                st["track"] = t2
                                mi.projected = (pj[2], pj[3])
                # step
                closed, L, want = int(self.tracks["closed"][k]) != 0, self.cum[k][-1], np.float64(st["v0"])
                if p is None or not (want > 0):
                    info = fm.Info("plain")
                    s1, v1 = tm.wrap(s + want * dt, L, closed), want
                else:
                    info = fm.Info("free")
                    v, lead = v0s[a], None
                    al = self._actor_leader(a, k, closed, L, p["look"], s, s0, st0, info)
                    if al is not None:
                        info.actor_g = al[0]
                        lead = ("actor", al[0], v0s[al[1]], np.float64(self.actors["radius"][al[1]]), al[1])
                    gp = scene_in["loc"]["globalpoint"][c]
                    eg = self._ego(a, k, closed, L, p["look"], p["lateral"], s, np.float64(gp["x"]), np.float64(gp["y"]), info)
                    if eg is not None:
                        info.ego_g = eg[0]
                        if lead is None or eg[0] <= lead[1]:
                            lead = ("ego", eg[0], fm.ego_speed(scene_in, flags, c), half_w, -1)
                    acc = fm.idm(p, v, want, np.float64(A["radius"]), lead, info)
                    v1 = v + acc * dt
                    if not (v1 > 0):
                        v1 = np.float64(0.0)
                    s1 = tm.wrap(s + 0.5 * (v + v1) * dt, L, closed)
                mi.step = info
                # ramp
                if have and (mi.fired or int(st["k"]) > 0):
                    st["k"] = int(st["k"]) + 1
                    tau = np.float64(int(st["k"])) / np.float64(int(m["n_steps"]))
                    w = tau * tau * (3 - 2 * tau)
                    st["lat"] = st["lat0"] + (m["lat_end"] - st["lat0"]) * w
                    if int(st["k"]) == int(m["n_steps"]):
                        st["lat"], st["k"], st["clock"] = m["lat_end"], 0, 0
                        st["next"], st["n_done"] = int(st["next"]) + 1, int(st["n_done"]) + 1
                        mi.finished = True
                elif int(st["clock"]) < I32_MAX:
                    st["clock"] = int(st["clock"]) + 1
            self.s[a], self.st[a] = s1, st
            if p is not None:
                self.v[a] = v1
            self.minfo.append(mi)
            self._store(obs, mot, a, k, s1, st["lat"])
        return obs, mot
