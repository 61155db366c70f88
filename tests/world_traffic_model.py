"""World traffic in plain numpy, written from DESIGN.md §4j (not from the kernel).

`World` is one vehicle record and one (s, v) state per vehicle PER WORLD of a fleet: `TrafficActor.scene` is the world and
`TrafficActor.slot` an own entry of every member scene.  `place` is what one k_move_world_traffic launch does to one staged obstacle
pool (pp_set_world_traffic, pp_update_async, an advance with following off), `step` what one k_follow_world_traffic launch does,
given the SceneIn records and ego flag words of EVERY scene of the set being staged.  §4h's cumulative lengths, `wrap`, locate and
place and §4i's steps 1 and 2 - per member ego - are taken from tests/traffic_model.py and tests/traffic_follow_model.py, as §4j
takes them over from §4h and §4i; what is new here is who the candidates are, the order (g_e, e) and where the pose is written.
numpy float64 is the IEEE double and every expression is evaluated left to right as the specification writes it, so the result is
meant to equal the device's byte for byte.

`step` records, per vehicle, which branch it took (`info`, tests/traffic_follow_model.Info plus `ego_scene`, the scene of the ego
leader, `ego_candidates`, the member scenes whose ego was a candidate, and `n_world`, the members looked at)."""
import numpy as np

import traffic_follow_model as fm
import traffic_model as tm


class World(fm.Follow):
    def __init__(self, tracks, points, actors, world_first, pin_off, n_own=None):
        """world_first: n_worlds + 1 scene indices; pin_off / n_own: the fleet's pinned slice of every scene."""
        self.world_first = np.asarray(world_first, np.int64)
        super().__init__(tracks, points, actors, np.zeros(len(self.world_first) - 1, np.int64))
        pin_off = np.asarray(pin_off, np.int64)
        self.entries = []                                        # per vehicle: its pool entry in every member scene, in scene order
        for A in self.actors:
            w = int(A["scene"])
            assert 0 <= w < len(self.world_first) - 1
            m = np.arange(self.world_first[w], self.world_first[w + 1])
            if n_own is not None:
                assert (0 <= int(A["slot"])) and (int(A["slot"]) < np.asarray(n_own)[m]).all()
            self.entries.append(pin_off[m] + int(A["slot"]))
        del self.pool_index                                      # (a vehicle has no single entry)

    def members(self, a):
        w = int(self.actors["scene"][a])
        return np.arange(self.world_first[w], self.world_first[w + 1])

    def _write(self, obs, mot, a, s):
        A = self.actors[a]
        k = int(A["track"])
        _, _, x, y = tm.point_at(self.px[k], self.py[k], self.cum[k], s)
        for e in self.entries[a]:                                # the same bytes into every member's entry
            o = obs[int(e)]
            o["x"], o["y"], o["type"], o["radius"] = x, y, A["type"], A["radius"]
            if mot is not None:
                mot[int(e)]["vx"], mot[int(e)]["vy"] = 0.0, 0.0

    def place(self, obs_pool, mot_pool=None, step=0.0):
        obs = obs_pool.copy()
        mot = None if mot_pool is None else mot_pool.copy()
        step = np.float64(step)
        for a, A in enumerate(self.actors):
            k = int(A["track"])
            s = self.s[a]
            if step != 0:
                with np.errstate(over="ignore"):
                    s = s + np.float64(A["speed"]) * step
            s = tm.wrap(s, self.cum[k][-1], int(self.tracks["closed"][k]) != 0)
            self.s[a] = s
            self._write(obs, mot, a, s)
        return obs, mot

    def step(self, obs_pool, mot_pool, dt, tf, scene_in, flags, vehicle_width):
        p = fm.params(tf)
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
                    info = fm.Info("plain")
                    raw = s0[a] + speed * dt
                    s1, v1 = tm.wrap(raw, L, closed), speed
                else:
                    info = fm.Info("free")
                    v = v0s[a]
                    lead = None
                    al = self._actor_leader(a, k, closed, L, p["look"], s0, info)          # 1.: the group is (world, track)
                    if al is not None:
                        info.actor_g = al[0]
                        lead = ("actor", al[0], v0s[al[1]], np.float64(self.actors["radius"][al[1]]), al[1])
                    best, info.ego_candidates, info.ego_scene = None, [], -1
                    mem = self.members(a)
                    info.n_world = len(mem)
                    for e in mem:                                # 2.: every member scene, in index order
                        loc = scene_in["loc"][int(e)]
                        one = fm.Info("free")
                        eg = self._ego(a, k, closed, L, p["look"], p["lateral"], s0[a], np.float64(loc["globalpoint"]["x"]), np.float64(loc["globalpoint"]["y"]), one)
                        info.window = one.window
                        if eg is None:
                            continue
                        info.ego_candidates.append(int(e))
                        if best is None or eg[0] < best[0]:      # the total order (g_e, e): e rises, so a tie keeps the lower scene
                            best = (eg[0], int(e), eg[1], eg[2])
                    if best is not None:
                        info.ego_g, info.ego_scene, info.kstar, info.d2 = best
                        if lead is None or best[0] <= lead[1]:   # 3.: the ego wins a tie against an actor
                            e = best[1]
                            vl = np.float64(0.0) if int(flags[e]) != 0 else np.float64(scene_in["loc"]["velocity"][e]) / np.float64(3.6)
                            lead = ("ego", best[0], vl, half_w, -1)
                    r = v / speed                                # 4.
                    r2 = r * r
                    free = 1 - r2 * r2
                    if lead is None:
                        acc = p["max_acc"] * free
                    else:
                        info.kind, g, vl, rl, info.leader = lead
                        info.g, info.vl = g, vl
                        net = g - np.float64(A["radius"]) - rl
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
                    if not (acc >= -p["max_dec"]):               # (a NaN brakes)
                        acc, info.clamped = -p["max_dec"], True
                    info.acc = acc
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
