"""Lane traffic in plain numpy, written from DESIGN.md §4h (not from the kernel).

`Traffic` holds what pp_set_traffic builds - the cumulative lengths of every track and the arc length `s` of every actor -
and `place` is what one k_move_traffic launch does to one staged obstacle pool: s' = wrap(s + speed * step) (no step for
step = 0), then ObPoint { x, y, type, radius } into the actor's pool entry and a zero ObMotion if the set carries a motion
pool.  numpy float64 is the IEEE double, every expression is evaluated left to right as the specification writes it, each
operation rounds once and the segment index is unique, so the result is meant to equal the device's byte for byte."""
import numpy as np


def cumulative(px, py, closed):
    """§4h cumulative lengths: cum[0] = 0, cum[i + 1] = cum[i] + sqrt(dx dx + dy dy), in order; a closed track has one more
    segment from the last point back to the first."""
    n = len(px)
    nseg = n if closed else n - 1
    cum = np.zeros(nseg + 1, np.float64)
    with np.errstate(over="ignore"):
        for i in range(nseg):
            j = i + 1 if i + 1 < n else 0
            dx = np.float64(px[j]) - np.float64(px[i])
            dy = np.float64(py[j]) - np.float64(py[i])
            cum[i + 1] = cum[i] + np.sqrt(dx * dx + dy * dy)
    return cum


def wrap(s, L, closed):
    """§4h `wrap`."""
    s, L = np.float64(s), np.float64(L)
    with np.errstate(all="ignore"):
        if closed:
            q = np.floor(s / L)
            s = s - q * L
            if not (s >= 0):
                s = np.float64(0.0)
            if s >= L:
                s = np.float64(0.0)
        else:
            if not (s >= 0):
                s = np.float64(0.0)
            if s > L:
                s = L
    return s


def locate(cum, s):
    """§4h place, first line: the largest i in [0, nseg) with cum[i] <= s.  cum is non-decreasing, so that is the number of
    entries of cum[0 .. nseg) that are <= s, less one (locate_walk below is the definition read literally)."""
    nseg = len(cum) - 1
    return min(max(int(np.searchsorted(cum[:nseg], s, side="right")) - 1, 0), nseg - 1)


def locate_walk(cum, s):
    i = 0
    for k in range(len(cum) - 1):
        if cum[k] <= s:
            i = k
    return i


def point_at(px, py, cum, s):
    """§4h place: (i, t, x, y) of arc length s."""
    n = len(px)
    i = locate(cum, s)
    with np.errstate(all="ignore"):
        d = cum[i + 1] - cum[i]
        t = (np.float64(s) - cum[i]) / d if d > 0 else np.float64(0.0)
        j = i + 1 if i + 1 < n else 0
        x = np.float64(px[i]) + t * (np.float64(px[j]) - np.float64(px[i]))
        y = np.float64(py[i]) + t * (np.float64(py[j]) - np.float64(py[i]))
    return i, t, x, y


class Traffic:
    """The state pp_set_traffic builds.  pool_index: the absolute pool entry of every actor, obs_off[scene] + slot of the
    resident records at set time (the pin); entries[a]: the entries actor a is written into (that one)."""

    def __init__(self, tracks, points, actors, obs_off):
        self.tracks, self.actors = np.array(tracks).copy(), np.array(actors).copy()
        self.px, self.py, self.cum = [], [], []
        for T in self.tracks:
            a, n = int(T["point_off"]), int(T["n_points"])
            self.px.append(np.ascontiguousarray(points["x"][a:a + n], np.float64))
            self.py.append(np.ascontiguousarray(points["y"][a:a + n], np.float64))
            self.cum.append(cumulative(self.px[-1], self.py[-1], int(T["closed"]) != 0))
        self.pool_index = np.asarray(obs_off)[self.actors["scene"]].astype(np.int64) + self.actors["slot"]
        self.entries = self.pool_index[:, None]
        self.s = np.ascontiguousarray(self.actors["s0"], np.float64).copy()          # wrapped by the first place(.., 0.0)

    def length(self, k):
        return self.cum[k][-1]

    def _plain(self, a, s, step):
        """§4h 2. - 3.: one step of a scripted actor (none for step = 0); returns (the sum, its wrap)."""
        k = int(self.actors["track"][a])
        with np.errstate(over="ignore"):
            raw = s + np.float64(self.actors["speed"][a]) * step if step != 0 else s          # the product is rounded, then the sum
        return raw, wrap(raw, self.cum[k][-1], int(self.tracks["closed"][k]) != 0)

    def _write(self, obs, mot, a, s):
        """§4h 4. - 5.: the ObPoint of arc length s into the actor's entries, and a zero ObMotion with a motion pool."""
        A = self.actors[a]
        k = int(A["track"])
        _, _, x, y = point_at(self.px[k], self.py[k], self.cum[k], s)
        for e in self.entries[a]:
            o = obs[int(e)]
            o["x"], o["y"], o["type"], o["radius"] = x, y, A["type"], A["radius"]
            if mot is not None:
                mot[int(e)]["vx"], mot[int(e)]["vy"] = 0.0, 0.0

    def place(self, obs_pool, mot_pool=None, step=0.0):
        """One launch on one staged set: returns (obs_pool', mot_pool') and updates self.s.  step = 0: pp_set_traffic and
        pp_update_async (s = wrap(s), which leaves a wrapped s as it is); step = EgoModel.dt: pp_advance_async."""
        obs = obs_pool.copy()
        mot = None if mot_pool is None else mot_pool.copy()
        for a in range(len(self.actors)):
            self.s[a] = self._plain(a, self.s[a], np.float64(step))[1]
            self._write(obs, mot, a, self.s[a])
        return obs, mot
