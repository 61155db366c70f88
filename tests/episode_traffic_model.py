"""The episode traffic reset in plain Python / numpy, written from DESIGN.md §4m (not from the kernel): when an ego restarts, the
actors of its scene go back to a start state.

`Reset` is what pp_set_episode_traffic builds on top of tests/traffic_model.py's `Traffic` or tests/traffic_follow_model.py's
`Follow` - the table of n_sets start states per actor, set 0 captured from the traffic as it stands, and the counters - and `step`
is what one k_reset_traffic launch does to one staged obstacle pool, behind the episode step and the traffic step of the same
advance: for every actor whose scene has EpisodeStats.age == 0, s' = wrap(s*), v' = v* (speed > 0) or speed, the ObPoint at s'
into the actor's pool entry with a zero ObMotion, and one more reset counted.  numpy float64 is the IEEE double; nothing is
computed here that tests/traffic_model.py does not compute."""
import numpy as np

import traffic_model as tm


class Reset:
    """tr: the Traffic / Follow the table is captured from; follow: following is on (v is captured and written).  starts: records
    with fields s and v, set k (1 ..) of actor a at (k - 1) * n_actors + a; None with n_sets == 1."""

    def __init__(self, tr, n_sets, starts=None, follow=False):
        n = len(tr.actors)
        self.n_sets, self.follow = int(n_sets), bool(follow)
        self.s, self.v = np.zeros((self.n_sets, n), np.float64), np.zeros((self.n_sets, n), np.float64)
        self.s[0] = tr.s                                         # set 0: the capture
        self.v[0] = tr.v if follow else np.ascontiguousarray(tr.actors["speed"], np.float64)
        if self.n_sets > 1:
            st = np.asarray(starts).reshape(-1)
            assert len(st) == (self.n_sets - 1) * n
            self.s[1:] = st["s"].reshape(self.n_sets - 1, n)
            self.v[1:] = st["v"].reshape(self.n_sets - 1, n)
        self.n_resets = np.zeros(n, np.int32)

    def step(self, tr, obs_pool, mot_pool, age, cur_start=None):
        """One launch on the set an advance stages.  age: EpisodeStats.age of every scene behind the episode step; cur_start:
        EpisodeSpawnStats.cur_start of every scene (read only with n_sets > 1).  Updates tr.s, tr.v (following on) and the counters;
        returns (obs_pool', mot_pool')."""
        obs = obs_pool.copy()
        mot = None if mot_pool is None else mot_pool.copy()
        for a, A in enumerate(tr.actors):
            c = int(A["scene"])
            if int(age[c]) != 0:                                 # 1. the scene goes on: the traffic step's bytes stay
                continue
            k = 0 if self.n_sets == 1 else int(cur_start[c])     # 2.
            t = int(A["track"])
            s1 = tm.wrap(self.s[k][a], tr.cum[t][-1], int(tr.tracks["closed"][t]) != 0)          # 3.
            tr.s[a] = s1                                         # 4.
            if self.follow:
                speed = np.float64(A["speed"])
                tr.v[a] = self.v[k][a] if speed > 0 else speed
            tr._write(obs, mot, a, s1)
            self.n_resets[a] += 1
        return obs, mot
