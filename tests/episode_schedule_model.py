"""The scenario schedule in plain Python / numpy, written from DESIGN.md §4p (not from the kernels), on top of
tests/episode_spawn_model.py: while pp_set_episode_schedule is in force, the first choice k0 of §4l 3a. is drawn by weights computed
from outcome counts per start record; every other step is §4l.

Python integers throughout: the specification uses int32 counts and uint64 intermediates, none of which can overflow here (a weight
is at most 131070, a sum of 16 of them below 2^22, (u >> 32) * W below 2^54).

`step` is what the episode step of one pp_advance_async does.  It takes what episode_spawn_model.step takes, and the schedule and
its rows - one per scene (scope 0) or one (scope 1) -, which it folds in place."""
import contextlib

import numpy as np

import episode_spawn_model as esm

CAUSES = 31 | 64 | 128


def weight(sm, n, f):
    """§4p 1.: the weight of a record with n counted episodes, f of them failures."""
    n, f = int(n), int(f)
    r = (f * 65536) // n if n >= int(sm["min_samples"][0]) else int(sm["prior"][0])
    d = abs(r - int(sm["target"][0]))
    return int(sm["floor_w"][0]) + ((int(sm["gain"][0]) * (65536 - d)) >> 16)


def weights(sm, row, M):
    return [weight(sm, row["n_end"][k], row["n_fail"][k]) for k in range(int(M))]


def draw(u, ws):
    """§4p 2.: (t, k0) for the hash u and the weights ws."""
    W = sum(int(w) for w in ws)
    t = ((int(u) >> 32) * W) >> 32
    run = 0
    for k, w in enumerate(ws):
        run += int(w)
        if run > t:
            return t, k
    raise AssertionError("t < W: some running sum exceeds it")


def fails(sm, c):
    """§4p 4.: is an episode that ended with cause word c a failure."""
    return (int(c) & int(sm["fail_mask"][0])) != 0 and (int(c) & int(sm["pass_mask"][0])) == 0


def fold(sm, row, endings):
    """§4p 4.: `endings` - (k_prev, failed) of every episode one advance ended for this row - are added, then every touched record
    is halved while its n_end has reached the window."""
    window, touched = int(sm["window"][0]), []
    for k, failed in endings:
        row["n_end"][k] += 1
        row["n_fail"][k] += int(bool(failed))
        touched.append(int(k))
    for k in sorted(set(touched)):
        while window > 0 and int(row["n_end"][k]) >= window:
            row["n_end"][k] >>= 1
            row["n_fail"][k] >>= 1


def new_rows(dtype, sm, n):
    return np.zeros(int(n) if int(sm["scope"][0]) == 0 else 1, dtype)


@contextlib.contextmanager
def _first_choice(choice):
    """episode_spawn_model.step with §4l 3a.'s k0 replaced: the one place where §4p differs from §4l."""
    old = esm.first_choice
    esm.first_choice = choice
    try:
        yield
    finally:
        esm.first_choice = old


def step(em, sp, sm, rows, stats, sstats, pool_in, pool_state, p, q, flags, state, O, hw, world_first=None, trace=None, score=None):
    """The batch - a Jacobi step twice over: every scene reads the records `p` the advance READ, and every draw reads the rows as
    they stood BEFORE this advance's endings are folded.  stats, sstats, rows (and score, if given) are updated in place.  Returns
    what episode_spawn_model.step returns."""
    assert int(sp["order"][0]) == 0, "a schedule replaces the hashed choice"
    scope = int(sm["scope"][0])
    before, k_prev = rows.copy(), sstats["cur_start"].copy()

    def choice(seed, s, e, M, order):
        return draw(esm.hash_u(seed, s, e), weights(sm, before[s if scope == 0 else 0], M))[1]
    with _first_choice(choice):
        out = esm.step(em, sp, stats, sstats, pool_in, pool_state, p, q, flags, state, O, hw, world_first, trace, score)
    causes = out[4]
    ended = [s for s in range(len(q)) if int(causes[s]) != 0]
    if scope == 0:
        for s in ended:
            fold(sm, rows[s], [(int(k_prev[s]), fails(sm, causes[s]))])
    else:
        fold(sm, rows[0], [(int(k_prev[s]), fails(sm, causes[s])) for s in ended])
    return out
