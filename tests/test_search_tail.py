"""The tail of the jump-point search (`search_core` of csrc/kernels_s.hpp behind the step loop): one pass over the closed-set
hash for the digest and every closed cell's parent slot, the chain of slot numbers from the goal to the start, the hops
expanded to path cells by one lane each, and the wave reductions.

The scenes come from tests/search_scenes.py (bitmaps sent as discs of 0.4 cells).  GPU tests hold the device to the model of
tests/grid_search_model.py in status, counters, digest, `path_len` and every path cell, and to the oracle for the whole tick.
The CPU tests check the case list itself: that every case sits where its name says (hops, runs, max_path, the walk taken),
and that the parents ON the goal's chain are found at every probe distance the parent probe has code for.

The hash of the coverage check is the kernel's: slot `(cell * 2654435761 mod 2^32) >> (32 - kClosedLog)`, linear probing, the
cells in insertion order (per step the entries taken, latest push first; a cell already in the hash is not inserted again).
The entries of the LAST step that lie behind the goal in the batch are inserted too but never expanded (kSeqNone).

Waived, one of five: "a parent found behind a kSeqNone slot".  A kSeqNone cell is inserted in the last step of the search
only; every parent on a chain was inserted in an earlier step, and linear probing never moves a cell, so the slots between a
parent's home slot and its own were all filled BEFORE the parent was - by cells that were expanded.  No scene can place a
kSeqNone slot there - not for the chain's parents, and not for the parent of any other cell the pass probes for.  What can be
had is asserted instead: kSeqNone slots in the hash that the pass reads and whose own parents it probes for (the goal closed
as the first node of a batch of four), and the check itself asserts that no case of the list has a parent behind one."""
import numpy as np
import pytest

import grid_search_model as gm
import search_scenes as ss
from parity_util import compare

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


FIELDS = ("n_expanded", "n_pushed", "n_rounds", "path_cost", "path_len", "order_digest")
HASH_MUL = 2654435761

# ---- the case list -------------------------------------------------------------------------------------------------------
# zigzag_case(21, 96): 64 hops; a start off the corner saves one, a goal one row in from the border adds one
HOPS_63_64_65 = [("hops/63", dict(start=(1, 5))), ("hops/64", {}), ("hops/65", dict(goal_in=1))]
RUNS = [12, 13, 64, 65]                   # kLongRun = 12: the hop's lane | the whole wave; 64 | 65: one and two turns of the wave
TRUNC_CASE = "corner/(0, 0)-(63, 63)"     # 74 cells (search_scenes.MAX_PATH_LEN)
GOAL_FIRST_OF_FOUR = [2, 18]              # random_case(seed, 64, 64): the goal is closed as node 0 of a batch of four (found by scanning)
LIMIT_INSIDE_BATCH = (7, 23)               # random_case(7, 64, 64): expansion 23 is the second node of a batch of four (checked below)
NO_PATH_CASE = "walled_in"
MIN_MAX_PATH = 2                          # pp_create refuses max_path < 2: max_path = 1 is asserted to be refused, and 2 runs in its place
WRAP_ON_CHAIN = [304, 1626]               # random_case(seed, 64, 64): a parent on the goal's chain sits across the wrap 511 -> 0 (found by scanning)


def _small(name):
    return next(c for c in ss.small_cases() if c.name == name)


def _groups():
    """name -> (cases, over): one handle and one launch per group."""
    def make():
        big = dict(max_path=8192)
        G = {}
        c64 = [_small("start_is_goal"), _small("goal_adjacent/0"), _small("goal_adjacent/3"), _small(NO_PATH_CASE), _small(TRUNC_CASE)]
        c64 += [ss.random_case(s, 64, 64, name=f"goal_first/{s}") for s in GOAL_FIRST_OF_FOUR]
        c64 += [ss.random_case(s, 64, 64, name=f"wrap/{s}") for s in WRAP_ON_CHAIN]
        c64 += [ss.random_case(s, 64, 64) for s in (1, 3, 4, 6, 7)]
        G["64x64"] = (c64, {})
        G["64x64/limit"] = ([ss.random_case(LIMIT_INSIDE_BATCH[0], 64, 64)], dict(max_expansions=LIMIT_INSIDE_BATCH[1]))
        for mp in (ss.MAX_PATH_LEN, ss.MAX_PATH_LEN - 1, 2, 1):
            G[f"64x64/max_path={mp}"] = ([_small(TRUNC_CASE), _small("goal_adjacent/1"), _small("start_is_goal")], dict(max_path=mp))
        c96 = [ss.zigzag_case(21, 96, name=n, **kw) for n, kw in HOPS_63_64_65]
        c96 += [ss.plain_case(96, 32, (3, 7), (3 + r, 7), name=f"run/{r}") for r in RUNS]
        c96 += [ss.plain_case(96, 32, (80, 20), (80 - r, 20), cells=[(40, 3)], name=f"run_west/{r}") for r in (12, 13)]
        c96 += [ss.random_case(s, 96, 32) for s in (1, 2, 3)]
        G["96x32"] = (c96, dict(max_path=1024))
        # near-full hashes (374 .. 389 expansions of at most 384): long probe chains and the wrap; those past 380 leave LDS (HBM walk)
        G["128x128"] = ([ss.walled_case(s) for s in ss.NEAR_CLOSED_MAX] + [ss.walled_case(ss.PEAK_513)], {})
        G["544x32"] = ([ss.strip_case(s, 544) for s in (0, 1)], big)                           # the first width of K = 1
        G["1024x32"] = ([ss.zigzag_case(126, 1024), ss.zigzag_case(130, 1024)], big)          # K = 1: LDS walk | the set has left LDS
        G["1056x32"] = ([ss.zigzag_case(170, 1056)] + [ss.zigzag_case(n, 1056, name=f"zigzag/1056x32/{n}+", **kw) for n, kw, _ in ss.ZIGZAG_SPLIT]
                        + [ss.strip_case(0, 1056)], big)                                       # K = 2: 511 | 513 | 512 hops
        return G
    return _cached("groups", make)


GROUP_NAMES = ["64x64", "64x64/limit", "64x64/max_path=74", "64x64/max_path=73", "64x64/max_path=2", "64x64/max_path=1", "96x32", "128x128", "544x32",
               "1024x32", "1056x32"]


def _cell(c, p):
    return p[1] * c.W + p[0]


def _model(dm, case, over):
    def make():
        cfg = ss.config(dm, case.W, case.H, **over)
        m = gm.search(case.bitmap.tobytes(), case.W, case.H, _cell(case, case.start), _cell(case, case.goal),
                      int(cfg["max_expansions"][0]), int(cfg["bucket_cap"][0]), int(cfg["max_path"][0]))
        return m, cfg
    return _cached(("model", case.name, case.W, tuple(sorted(over.items()))), make)


# ---- the kernel's hash, replayed from the model's trace ------------------------------------------------------------------
def hash_replay(m, W, closed_log):
    """(slot of every inserted cell, the kSeqNone cells, (direction, run) of every cell) after the search of model result `m`."""
    T = 1 << closed_log
    ent = m["entries"]
    tab, slot, info, seq_none = [None] * T, {}, {}, set()
    live = [0]
    for i, st in enumerate(m["steps"]):
        taken = list(st["taken"])
        if i == len(m["steps"]) - 1:
            # the device takes the whole batch before it looks at the goal or the limit: the entries behind are inserted, not expanded
            ties = [live[k] for k in st["tie_positions"]]
            taken = ties[::-1][:gm.BATCH]
            assert taken[:len(st["taken"])] == list(st["taken"])
        for e in taken:
            _, cell, d, run = ent[e]
            if cell in slot:
                continue
            h = ((cell * HASH_MUL) & 0xFFFFFFFF) >> (32 - closed_log)
            while tab[h] is not None:
                h = (h + 1) % T
            tab[h], slot[cell], info[cell] = cell, h, (d, run)
            if e not in st["closed"]:
                seq_none.add(cell)
        live = [e for e in live if e not in set(st["taken"])] + list(st["pushed"])
    return tab, slot, info, seq_none


def probe_path(tab, cell, closed_log):
    """The slots the probe for `cell` reads before it finds it: (home slot, [slots passed])."""
    T = 1 << closed_log
    h = ((cell * HASH_MUL) & 0xFFFFFFFF) >> (32 - closed_log)
    passed = []
    while tab[h] != cell:
        assert tab[h] is not None, "the cell is not in the hash"
        passed.append(h)
        h = (h + 1) % T
    return h, passed


def chain_probes(m, W, closed_log):
    """For every hop of the goal's chain: (distance, wrapped, kSeqNone slots passed) of the probe for the hop's parent."""
    tab, slot, info, seq_none = hash_replay(m, W, closed_log)
    start, goal = m["order"][0], m["order"][-1]
    out, c = [], goal
    while c != start:
        d, run = info[c]
        c -= run * (gm.VEC[d][1] * W + gm.VEC[d][0])
        at, passed = probe_path(tab, c, closed_log)
        out.append((len(passed), bool(passed) and at < passed[0], sum(tab[s] in seq_none for s in passed)))
    return out, tab, slot, info, seq_none


def _lds_walk(dm, c, over, k):
    m, cfg = _model(dm, c, over)
    return m["status"] in (gm.FOUND, gm.PATH_TRUNC) and ss.forms(m, cfg, 1, k)["path_walk"] == "lds"


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def test_kernel_constants_are_read():
    """The patterns tests/search_scenes.py reads from kernels_s.hpp still find their lines (the hop-list bound among them)."""
    k = ss.kernel_constants()
    assert k["DMPP_OPEN_CAP"] == 512 and k["closed_log"] == {0: 9, 1: 9, 2: 10}


def test_case_list_sits_on_the_tail_s_edges(dm):
    k = ss.kernel_constants()
    G = _groups()
    assert list(G) == GROUP_NAMES
    M = {}
    for name, (cases, over) in G.items():
        for c in cases:
            m, cfg = _model(dm, c, over)
            f = ss.forms(m, cfg, 1, k) if m["status"] not in (gm.GOAL_BLOCKED,) else None
            M[(name, c.name)] = (m, f)
            print(f"{name:20s} {c.name:26s} {gm.STATUS_NAMES[m['status']]:10s} exp {m.get('n_expanded', -1):4d} hops {m.get('hops', 0):4d} "
                  f"len {m.get('path_len', 0):5d} K {f['K']} walk {f['path_walk']}")
    hops = lambda g, n: M[(g, n)][0]["hops"]
    walk = lambda g, n: M[(g, n)][1]["path_walk"]
    # hops 0, 1, 63 | 64 | 65 (one and two passes of the hop expansion), 511 | 512 | 513 (lds | chunked)
    assert hops("64x64", "start_is_goal") == 0 and M[("64x64", "start_is_goal")][0]["path_len"] == 1
    assert hops("64x64", "goal_adjacent/0") == 1 and hops("64x64", "goal_adjacent/3") == 1
    assert [hops("96x32", n) for n, _ in HOPS_63_64_65] == [63, 64, 65] and all(walk("96x32", n) == "lds" for n, _ in HOPS_63_64_65)
    z = [("zigzag/1056x32/170", 511, "lds"), ("zigzag/1056x32/170+", 512, "lds"), ("zigzag/1056x32/171+", 513, "chunked")]
    assert [(hops("1056x32", n), walk("1056x32", n), M[("1056x32", n)][1]["K"]) for n, _, _ in z] == [(h, w, 2) for _, h, w in z]
    # runs of 12 | 13 and 64 | 65 cells in one hop
    for r in RUNS:
        m = M[("96x32", f"run/{r}")][0]
        assert (m["hops"], m["path_len"]) == (1, r + 1), r
    # max_path = Lc, Lc - 1 and 1 (the specification's answer, the model's; a handle takes max_path >= 2: MIN_MAX_PATH below)
    full = M[("64x64/max_path=74", TRUNC_CASE)][0]
    assert full["status"] == gm.FOUND and full["path_len"] == ss.MAX_PATH_LEN and full["hops"] > 1
    for mp in (ss.MAX_PATH_LEN - 1, 2, 1):
        t = M[(f"64x64/max_path={mp}", TRUNC_CASE)][0]
        assert t["status"] == gm.PATH_TRUNC and t["path"] == full["path"][-mp:]
    assert M[("64x64/max_path=1", "start_is_goal")][0]["status"] == gm.FOUND and M[("64x64/max_path=1", "goal_adjacent/1")][0]["status"] == gm.PATH_TRUNC
    # the goal closed as the first node of a batch of four: three kSeqNone slots in the hash
    for s in GOAL_FIRST_OF_FOUR:
        m = M[("64x64", f"goal_first/{s}")][0]
        last = m["steps"][-1]
        assert m["status"] == gm.FOUND and len(last["closed"]) == 1 and last["closed"][0] == last["taken"][0] and last["n_ties"] >= gm.BATCH, s
        assert len(hash_replay(m, 64, 9)[3]) >= 2, s
    # NO_PATH, and LIMIT with max_expansions inside a batch (digest without a path)
    assert M[("64x64", NO_PATH_CASE)][0]["status"] == gm.NO_PATH
    lim = M[("64x64/limit", ss.random_case(LIMIT_INSIDE_BATCH[0], 64, 64).name)][0]
    assert lim["status"] == gm.LIMIT and lim["n_expanded"] == LIMIT_INSIDE_BATCH[1]
    assert lim["steps"][-1]["n_ties"] > len(lim["steps"][-1]["closed"]) >= 1 and len(lim["steps"][-1]["taken"]) < min(gm.BATCH, lim["steps"][-1]["n_ties"])
    # the closed set leaves LDS (HBM walk), K = 0 and K = 1; a retry through k_search_spill; K = 1 on the LDS walk
    walks128 = {c.name: (M[("128x128", c.name)][1]["path_walk"], M[("128x128", c.name)][1]["retry"]) for c in G["128x128"][0]}
    assert any(w == "hbm" for w, _ in walks128.values()) and any(w == "lds" for w, _ in walks128.values()), walks128
    assert any(r for _, r in walks128.values()), walks128
    assert walk("1024x32", "zigzag/1024x32/126") == "lds" and walk("1024x32", "zigzag/1024x32/130") == "hbm" and M[("1024x32", "zigzag/1024x32/126")][1]["K"] == 1
    assert all(M[("544x32", c.name)][1]["K"] == 1 and M[("544x32", c.name)][0]["status"] == gm.FOUND for c in G["544x32"][0])


def test_parents_on_the_chain_are_found_at_every_probe_distance(dm):
    """Over the cases whose path comes from the parent slots (the LDS walk): parents ON the goal's chain at probe distance 0, 1,
    >= 2 and across the wrap 511 -> 0.  (Behind a kSeqNone slot: waived, see the module docstring; what stands in for it is below.)"""
    k = ss.kernel_constants()
    seen = dict(d0=0, d1=0, d2=0, wrap=0, behind_none=0)
    none_in_hash, none_on_a_walked_path = 0, 0          # kSeqNone cells | closed cells whose parent's probe passes one (none: see the waiver)
    longest = 0
    for name, (cases, over) in _groups().items():
        for c in cases:
            if not _lds_walk(dm, c, over, k):
                continue
            m, cfg = _model(dm, c, over)
            K = ss.forms(m, cfg, 1, k)["K"]
            cl = k["closed_log"][K]
            probes, tab, slot, info, seq_none = chain_probes(m, c.W, cl)
            assert len(probes) == m["hops"]
            for dist, wrapped, nones in probes:
                seen["d0"] += dist == 0
                seen["d1"] += dist == 1
                seen["d2"] += dist >= 2
                seen["wrap"] += wrapped
                seen["behind_none"] += nones > 0
                longest = max(longest, dist)
            none_in_hash += len(seq_none)
            # the pass probes for the parent of EVERY closed cell: a kSeqNone slot on one of those probe paths
            for cell, (d, run) in info.items():
                if d <= 7 and run > 0:
                    p = cell - run * (gm.VEC[d][1] * c.W + gm.VEC[d][0])
                    none_on_a_walked_path += any(tab[s] in seq_none for s in probe_path(tab, p, cl)[1])
    print("parents on goal chains:", seen, "longest probe", longest, "kSeqNone cells", none_in_hash, "on walked probe paths", none_on_a_walked_path)
    assert seen["d0"] and seen["d1"] and seen["d2"] and seen["wrap"], seen
    assert seen["behind_none"] == 0            # (cannot be: the reason for the waiver; if this ever fails, assert it above instead)
    assert none_in_hash >= 4 and none_on_a_walked_path == 0, (none_in_hash, none_on_a_walked_path)


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def _n_obs(cases):
    return max(1, max(int(np.count_nonzero(c.bitmap)) for c in cases))


def _oracle_tick(dm, oracle, name):
    def make():
        cases, over = _groups()[name]
        cfg = _model(dm, cases[0], over)[1]
        sc = ss.build(dm, cfg, [(c.bitmap, c.start, c.goal) for c in cases], _n_obs(cases))
        st = sc["state"].copy()
        plan, gout, _ = oracle.plan_tick_batch(cfg, sc, st, n_threads=8)
        return plan, gout, st
    return _cached(("oracle", name), make)


def _launch(dm, name, items):
    """One launch of the cases `items` (indices into the group): (GridOut, PlanOut, SceneState, paths)."""
    cases, over = _groups()[name]
    cfg = _model(dm, cases[0], over)[1]
    sc = ss.build(dm, cfg, [(cases[i].bitmap, cases[i].start, cases[i].goal) for i in items], _n_obs(cases))
    pl = dm.Planner(cfg, device=0, max_scenes=len(items), max_obs_total=len(items) * sc["n_obs"])
    try:
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
        pl.tick(sync=True)
        gout, plan, state = pl.get_grid_out(), pl.get_plan(), pl.get_state()
        paths = [pl.get_path(s, int(gout["path_len"][s])) if int(gout["path_len"][s]) else np.zeros(0, np.int32) for s in range(len(items))]
    finally:
        pl.close()
    return gout, plan, state, paths


def _check(dm, oracle, name, items, gout, plan, state, paths, tag):
    cases, over = _groups()[name]
    plan_o, gout_o, state_o = _oracle_tick(dm, oracle, name)
    bad = []
    for s, ci in enumerate(items):
        c = cases[ci]
        m, _ = _model(dm, c, over)
        t = f"{tag}[{s}] {c.name}"
        rec = gout[s]
        if int(rec["status"]) != m["status"]:
            bad.append(f"{t}: status {int(rec['status'])} vs model {m['status']} ({gm.STATUS_NAMES[m['status']]})")
            continue
        assert m["status"] not in (gm.OVERFLOW, gm.COST_RANGE, gm.INTERNAL), t          # every case of this file defines every field
        bad += [f"{t}.{f}: {int(rec[f])} vs model {m[f]}" for f in FIELDS if int(rec[f]) != m[f]]
        if paths[s].tolist() != m["path"]:
            k = next((i for i, (a, b) in enumerate(zip(paths[s].tolist(), m["path"])) if a != b), -1)
            bad.append(f"{t}.path: differs from the model's at cell {k} (lengths {len(paths[s])} / {len(m['path'])})")
        bad += compare(gout[s:s + 1], gout_o[ci:ci + 1], t + " grid") + compare(plan[s:s + 1], plan_o[ci:ci + 1], t + " plan")
        bad += compare(state[s:s + 1], state_o[ci:ci + 1], t + " state")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_device_tail_equals_model_and_oracle(dm, oracle, name):
    """Every case of a group in one launch: status, counters, digest, path_len and every path cell against the model; GridOut,
    PlanOut and SceneState against the oracle's tick."""
    items = list(range(len(_groups()[name][0])))
    if _groups()[name][1].get("max_path", MIN_MAX_PATH) < MIN_MAX_PATH:
        with pytest.raises(dm.PlannerError, match="max_path too small"):
            _launch(dm, name, items)
        return
    bad = _check(dm, oracle, name, items, *_launch(dm, name, items), "whole")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [("64x64", "goal_first/2"), ("96x32", "hops/65"), ("128x128", None)])
def test_same_scene_alone_first_and_last_of_129(dm, oracle, name, case):
    """One scene alone (sixteen set-up waves), and first and last in a batch of 129 (four): the same bytes, and the model's."""
    cases, _ = _groups()[name]
    ci = 0 if case is None else [c.name for c in cases].index(case)
    other = (ci + 1) % len(cases)
    alone = _launch(dm, name, [ci])
    items = [ci] + [other] * 127 + [ci]
    batch = _launch(dm, name, items)
    bad = _check(dm, oracle, name, [ci], *alone, "alone") + _check(dm, oracle, name, items, *batch, "129")
    for s in (0, 128):
        if alone[0][0].tobytes() != batch[0][s].tobytes() or alone[3][0].tobytes() != batch[3][s].tobytes() or alone[1][0].tobytes() != batch[1][s].tobytes():
            bad.append(f"{name}/{cases[ci].name}: item {s} of 129 differs from the scene alone")
    assert not bad, "\n".join(bad[:20])
