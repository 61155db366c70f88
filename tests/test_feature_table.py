"""The rollout feature table (csrc/rollout_features.hpp through pp_feature_retires / pp_feature_consistent; DESIGN.md §7, "Feature life
cycle"): which features a successful set call switches off, and what holds between the features that are on.  No device needed.

The table and the invariants stand here a second time, literally, as DESIGN.md prints them: a header that drifts from the document
fails."""
import ctypes
import itertools

import pytest

FLEET, ROUTE, TRAFFIC, WORLD, FOLLOW, EPISODES, SPAWN, TRESET, ELOG, SCHEDULE, WORLDS, WRESET = (1 << i for i in range(12))
ALL = (1 << 12) - 1
NAMES = {FLEET: "fleet", ROUTE: "route", TRAFFIC: "traffic", WORLD: "world traffic", FOLLOW: "follow", EPISODES: "episodes", SPAWN: "spawn",
         TRESET: "traffic reset", ELOG: "episode log", SCHEDULE: "schedule", WORLDS: "world episodes", WRESET: "world reset"}
# causes, by number (include/dmpp_planner.h)
(RESIDENT, MAP, SET_FLEET, SET_ROUTE, SET_TRAFFIC, SET_WORLD, SET_FOLLOW, SET_EPISODES, SET_SPAWN, SET_TRESET, SET_ELOG, TRAFFIC_OFF,
 SET_GRID_FOLLOW, SCORE) = range(14)
TABLE = {
    RESIDENT: FLEET | ROUTE | TRAFFIC | WORLD | EPISODES | SPAWN | TRESET | ELOG | SCHEDULE | WORLDS | WRESET,          # pp_set_scenes, pp_set_egos, pp_set_n_scenes
    MAP: ROUTE,
    SET_FLEET: WORLD | WRESET,
    SET_TRAFFIC: TRESET | WRESET,
    SET_WORLD: TRESET | WRESET,
    TRAFFIC_OFF: TRAFFIC | WORLD | TRESET | WRESET,                                        # either traffic call with no actors: traffic itself too
    SET_FOLLOW: TRESET | WRESET,
    SET_EPISODES: SPAWN | TRESET | ELOG | SCHEDULE | WORLDS | WRESET,
    SET_SPAWN: TRESET | ELOG | SCHEDULE | WORLDS | WRESET,
    SET_ROUTE: 0, SET_TRESET: 0, SET_ELOG: 0, SET_GRID_FOLLOW: 0, SCORE: 0,
}
# the nine features with a set cause; the set calls of SCHEDULE, WORLDS and WRESET have none: they retire nothing
SET_CAUSE = {FLEET: SET_FLEET, ROUTE: SET_ROUTE, TRAFFIC: SET_TRAFFIC, WORLD: SET_WORLD, FOLLOW: SET_FOLLOW, EPISODES: SET_EPISODES, SPAWN: SET_SPAWN,
             TRESET: SET_TRESET, ELOG: SET_ELOG}
ENVS = list(itertools.product((0, 1), (0, 1)))          # (have_map, resident_mode)


def want_consistent(m, have_map, mode):
    """The invariants of DESIGN.md §7, one per line."""
    return (not (m & SPAWN) or bool(m & EPISODES)) and \
           (not (m & TRESET) or bool(m & TRAFFIC and not m & WORLD and m & EPISODES)) and \
           (not (m & ELOG) or bool(m & EPISODES)) and \
           (not (m & WORLD) or bool(m & FLEET)) and \
           (not (m & ROUTE) or bool(have_map and mode == 1)) and \
           (not (m & SCHEDULE) or bool(m & SPAWN)) and \
           (not (m & WORLDS) or bool(m & SPAWN)) and \
           not (m & SCHEDULE and m & WORLDS) and \
           (not (m & WRESET) or bool(m & WORLD and m & EPISODES and m & SPAWN and m & WORLDS)) and \
           not (m & TRAFFIC and m & WORLD)          # (one TrafficState: per scene or per world)


@pytest.fixture(scope="module")
def table(dm):
    lib = dm.load_library()
    lib.pp_feature_retires.argtypes, lib.pp_feature_retires.restype = [ctypes.c_int], ctypes.c_int
    lib.pp_feature_consistent.argtypes, lib.pp_feature_consistent.restype = [ctypes.c_uint, ctypes.c_int, ctypes.c_int], ctypes.c_int
    return lib


def test_retire_masks_are_the_documented_table(table):
    assert {c: table.pp_feature_retires(c) for c in range(14)} == TABLE
    assert table.pp_feature_retires(14) == -1 and table.pp_feature_retires(-1) == -1
    assert not any(m & FOLLOW for m in TABLE.values())          # nothing retires the follow model


def test_consistent_is_the_documented_invariants(table):
    n_ok = 0
    for m in range(ALL + 1):
        for have_map, mode in ENVS:
            got = table.pp_feature_consistent(m, have_map, mode)
            assert got == int(want_consistent(m, have_map, mode)), (bin(m), have_map, mode)
            n_ok += got
    assert 0 < n_ok < 4 * (ALL + 1) and table.pp_feature_consistent(0, 0, 0) == 1
    assert table.pp_feature_consistent(ALL & ~(WORLD | WORLDS | WRESET), 1, 1) == 1          # everything per-scene at once is a legal handle
    assert table.pp_feature_consistent(ALL & ~(TRAFFIC | TRESET | SCHEDULE), 1, 1) == 1          # ... and everything per-world


def dependants(table, f):
    """The features that are on in no consistent mask without f."""
    free = 0
    for m in range(ALL + 1):
        if not m & f and table.pp_feature_consistent(m, 1, 1):
            free |= m
    return ALL & ~free & ~f


def test_every_cause_keeps_a_consistent_state_consistent(table):
    """... also when the cause takes the map or resident mode 1 away (pp_set_map that fails half way, pp_set_scenes), and when the call is the
    off form of a set call, which clears its own bit as well."""
    own = {c: f for f, c in SET_CAUSE.items()}
    own[TRAFFIC_OFF] = 0
    deps = {f: dependants(table, f) for f in (SCHEDULE, WORLDS, WRESET)}
    assert deps == {SCHEDULE: 0, WORLDS: WRESET, WRESET: 0}          # pp_set_episode_worlds(h, 0) takes the world reset off
    for m in range(ALL + 1):
        for have_map, mode in ENVS:
            if not table.pp_feature_consistent(m, have_map, mode):
                continue
            for c in range(14):
                after = m & ~table.pp_feature_retires(c)
                envs = [(have_map, mode)] + ([(0, mode)] if c == MAP else []) + ([(have_map, 0), (have_map, 1)] if c == RESIDENT else [])
                for e in envs:
                    assert table.pp_feature_consistent(after, *e), (bin(m), c, e)
                    assert table.pp_feature_consistent(after & ~own.get(c, 0), *e), (bin(m), c, e, "off form")
            for f, d in deps.items():          # no cause: the off form of the set call takes the feature and its dependants off
                assert table.pp_feature_consistent(m & ~(f | d), have_map, mode), (bin(m), NAMES[f])


def test_masks_are_transitively_closed(table):
    """A cause that retires X retires what the set call of X retires - unless the two are never on together: pp_set_fleet retires world traffic,
    pp_set_world_traffic the traffic reset, and the reset is never on beside world traffic."""
    def together(x, y):
        return any(m & x and m & y and table.pp_feature_consistent(m, 1, 1) for m in range(ALL + 1))
    exempt = []
    for c in range(14):
        r = table.pp_feature_retires(c)
        for x in SET_CAUSE:
            for y in NAMES:
                if r & x and table.pp_feature_retires(SET_CAUSE[x]) & y and not r & y:
                    assert not together(x, y), f"cause {c} retires {NAMES[x]} and not {NAMES[y]}"
                    exempt.append((c, x, y))
    assert exempt == [(SET_FLEET, WORLD, TRESET)]


def test_a_set_call_never_retires_its_own_feature(table):
    for f, c in SET_CAUSE.items():
        assert not table.pp_feature_retires(c) & f, NAMES[f]
    assert table.pp_feature_retires(TRAFFIC_OFF) & (TRAFFIC | WORLD) == TRAFFIC | WORLD          # the one exception: no actors
