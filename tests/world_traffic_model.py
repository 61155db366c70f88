"""World traffic in plain numpy, written from DESIGN.md §4j (not from the kernel).

`World` is one vehicle record and one (s, v) state per vehicle PER WORLD of a fleet: `TrafficActor.scene` is the world and
`TrafficActor.slot` an own entry of every member scene.  `place` (tests/traffic_model.py) is then what one k_move_world_traffic
launch does to one staged obstacle pool (pp_set_world_traffic, pp_update_async, an advance with following off) and `step`
(tests/traffic_follow_model.py) what one k_follow_world_traffic launch does, given the SceneIn records and ego flag words of EVERY
scene of the set being staged: §4j takes §4h and §4i over whole - the groups are (world, track) because `scene` is the world - and
what is new here is who the ego candidates are, the order (g_e, e) and where the pose is written.

`step` records, per vehicle, which branch it took (`info`, tests/traffic_follow_model.Info plus `ego_scene`, the scene of the ego
leader, `ego_candidates`, the member scenes whose ego was a candidate, and `n_world`, the members looked at)."""
import numpy as np

import traffic_follow_model as fm


class World(fm.Follow):
    def __init__(self, tracks, points, actors, world_first, pin_off, n_own=None):
        """world_first: n_worlds + 1 scene indices; pin_off / n_own: the fleet's pinned slice of every scene."""
        self.world_first = np.asarray(world_first, np.int64)
        super().__init__(tracks, points, actors, np.zeros(len(self.world_first) - 1, np.int64))
        pin_off = np.asarray(pin_off, np.int64)
        self.entries = []                                        # per vehicle: its pool entry in every member scene, in scene order: the same bytes into each
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

    # §4j: every member scene's ego is a candidate (§4i 2.), the smallest in the total order (g_e, e) may lead
    def _ego_leader(self, a, k, closed, L, p, s_a, scene_in, flags, info):
        best, info.ego_candidates, info.ego_scene = None, [], -1
        mem = self.members(a)
        info.n_world = len(mem)
        for e in mem:                                            # in index order
            gp = scene_in["loc"]["globalpoint"][int(e)]
            one = fm.Info("free")
            eg = self._ego(a, k, closed, L, p["look"], p["lateral"], s_a, np.float64(gp["x"]), np.float64(gp["y"]), one)
            info.window = one.window
            if eg is None:
                continue
            info.ego_candidates.append(int(e))
            if best is None or eg[0] < best[0]:                  # e rises, so a tie keeps the lower scene
                best = (eg[0], int(e), eg[1], eg[2])
        if best is None:
            return None
        _, info.ego_scene, info.kstar, info.d2 = best
        return best[0], fm.ego_speed(scene_in, flags, best[1])
