"""The episode log in plain Python / numpy, written from DESIGN.md §4n (not from the kernel), over tests/episode_model.py and
tests/rollout_score_model.py.

`EpisodeLog` is the state pp_set_episode_log creates: the ring, `total`, every scene's start record and the scorecard of its
running episode on the device side; `seq` and the read position on the host side.  `append` is what k_log_episodes does behind the
episode step of one advance, `fold` what a scored tick does to the scorecards of the running episodes, `read` / `info` what
pp_read_episode_log / pp_get_episode_log_info return.  Records are numpy voids of the ABI's layout, so a log is meant to equal
the device's byte for byte."""
import numpy as np

import rollout_score_model as rsm


class EpisodeLog:
    def __init__(self, record_dtype, n, cap, cur_start=None, scored=False):
        """§4n 0.: the state behind pp_set_episode_log(cap).  cur_start: EpisodeSpawnStats.cur_start with a spawn model in force."""
        assert cap > 0
        self.dtype, self.n, self.cap = record_dtype, n, cap
        self.ring = np.zeros(cap, record_dtype)
        self.total, self.seq, self.pos, self.lost = 0, 0, 0, 0
        self.start_of = np.zeros(n, np.int32) if cur_start is None else np.array(cur_start, np.int32).copy()
        self.score_dtype = record_dtype.fields["score"][0]
        self.E = rsm.new_scores(self.score_dtype, n) if scored else None

    def score_begin(self):
        """pp_score_begin (and every call that restarts the totals of §4d): the scorecards of the running episodes restart too."""
        self.E = rsm.new_scores(self.score_dtype, self.n)

    def fold(self, cfg, dt_score, scene_in, plan, state, obs_now, flags):
        """§4n 3.: a scored tick, folded by §4d 2. - 4. into the scorecard of every scene's running episode (no grid half)."""
        rsm.fold(self.E, cfg, dt_score, scene_in, plan, state, obs_now, flags)

    def append(self, stats, prev_in, tick, spawn_stats=None):
        """§4n 2.: one advance.  stats: EpisodeStats behind the episode step; prev_in: the SceneIn records the advance read; tick:
        pp_tick_id of the tick it read; spawn_stats: EpisodeSpawnStats behind the step, or None without a spawn model."""
        ended = np.flatnonzero(stats["age"][:self.n] == 0)
        m = len(ended)
        for rank, s in enumerate(ended):
            o = self.total + rank
            if o >= self.total + m - self.cap:
                r = self.ring[o % self.cap]
                r["scene"], r["episode"], r["start"], r["cause"] = s, int(stats["n_episodes"][s]) - 1, self.start_of[s], stats["last_cause"][s]
                r["age"], r["seq"], r["tick"], r["dist"] = stats["last_age"][s], self.seq, tick, stats["last_dist"][s]
                r["end_pos"]["x"], r["end_pos"]["y"] = prev_in["loc"]["globalpoint"]["x"][s], prev_in["loc"]["globalpoint"]["y"][s]
                r["end_speed"] = prev_in["loc"]["velocity"][s]
                r["score"] = rsm.new_scores(self.score_dtype, 1)[0] if self.E is None else self.E[s]
            if self.E is not None:
                self.E[s] = rsm.new_scores(self.score_dtype, 1)[0]
            self.start_of[s] = 0 if spawn_stats is None else spawn_stats["cur_start"][s]
        self.total += m
        self.seq += 1

    def read(self, max_records=None):
        """§4n 4., pp_read_episode_log: (records, n_lost)."""
        want = self.cap if max_records is None else max_records
        oldest = max(self.pos, self.total - self.cap)
        lost = oldest - self.pos
        n = min(self.total - oldest, want)
        out = np.array([self.ring[(oldest + k) % self.cap] for k in range(n)], self.dtype).reshape(n)
        self.pos, self.lost = oldest + n, self.lost + lost
        return out, lost

    def info(self):
        """pp_get_episode_log_info: (total, lost_total)."""
        return self.total, self.lost + max(0, self.total - self.cap - self.pos)
