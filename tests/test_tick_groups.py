"""Tick groups: a piped pp_plan_tick defers its search and scoring until G ticks are enqueued and launches them for all G at
once (one k_search / k_score over G * n work items).  Which ticks share a launch must change no result: every case below runs
the same ticks on a grouped handle and on one with DMPP_TICK_GROUP=1 (one tick per launch, the pipeline before groups) and
compares the outputs bit for bit - with the groups cut short by every kind of call that has to flush an open group.
The first two tests check the group arithmetic and the LDS budget arithmetic of a group's search on the CPU."""
import ctypes
import os

import numpy as np
import pytest

from parity_util import compare, move_ego


def test_group_arithmetic(dm):
    """CPU: the size of a group and the ring sizes (no device needed)."""
    lib = dm.load_library()
    lib.pp_tick_group_size.argtypes = [ctypes.c_int] * 4
    lib.pp_tick_group_cap.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t]
    lib.pp_tick_group_const.argtypes = [ctypes.c_int]
    gmax, nbuf, ring, nobs, gring, ngout = (lib.pp_tick_group_const(k) for k in range(6))
    assert gmax == 4 and nbuf >= 2
    assert ring == 2 * nbuf and nobs == ring * gmax             # snapshot sets: 2 kBuf group positions of gmax slots
    assert gring == 4 * nbuf and ngout == gring * gmax          # GridOut sets: a multiple of kBuf positions (same stream)
    assert lib.pp_tick_group_const(6) == -1
    size = lib.pp_tick_group_size
    # the smallest G with G * n >= 2 * slots, at most gmax and the handle's slots
    assert size(1024, 1536, 4, 0) == 3
    assert size(1024, 1280, 4, 0) == 3
    assert size(1024, 2048, 4, 0) == 4
    assert size(2048, 1536, 4, 0) == 2
    assert size(4096, 1536, 4, 0) == 1
    assert size(256, 1536, 4, 0) == 4
    assert size(1024, 1536, 2, 0) == 2
    assert size(1024, 1536, 1, 0) == 1
    # the knob: forced sizes, capped the same way
    assert size(1024, 1536, 4, 1) == 1
    assert size(4096, 1536, 4, 2) == 2
    assert size(1024, 1536, 4, 9) == 4
    assert size(1024, 1536, 3, 4) == 3
    cap = lib.pp_tick_group_cap
    item = 512 * 512 * 2 + 3 * 512 * 512 // 8          # closed-set spill, closed bits, dense bitmaps of a 512 x 512 scene
    assert cap(1024, 256, 0, item) == 4
    assert cap(1024, 256, 1, item) == 1                 # DMPP_TICK_GROUP=1: no extra memory
    assert cap(128, 256, 0, item) == 1                  # never piped
    assert cap(4096, 256, 0, item) == 1                 # a set of 4 x 4096 work items would exceed the byte cap
    big = 2048 * 2048 * 2 + 3 * 2048 * 2048 // 8
    assert cap(1024, 256, 0, big) == 1


def test_search_budget_arithmetic(dm):
    """CPU: the LDS budget of a group's search and the workgroup slots it gives (pp_search_budget, no device needed).  Every row:
    static LDS 7344, metas 4096, dense-form LDS 8192, at most 8192 words, 256 CUs - the figures of a 512 x 512 grid.  The expected
    values are those of the expressions as they stood inline in pp_plan_tick."""
    lib = dm.load_library()
    i32 = ctypes.c_int32
    lib.pp_search_budget.argtypes = [ctypes.c_int] * 12 + [ctypes.POINTER(i32)] * 3
    FIXED, DENSE = 1, 2
    rows = [  # n, G, n_obs_total, need, budget, from_need, mode -> budget, from_need, slots
        ((1024, 1, 65536, -1, 0, 0, 0), (2048, 0, 1280)),          # first tick, 64 obstacles
        ((1024, 3, 65536, 1635, 2048, 0, 0), (1920, 1, 1536)),     # the first need replaces the guess
        ((1024, 3, 65536, 1500, 1920, 1, 0), (1920, 1, 1536)),     # hysteresis keeps
        ((1024, 3, 65536, 900, 1920, 1, 0), (1088, 1, 2048)),      # shrinks by more than a quarter
        ((1024, 3, 65536, 2500, 1920, 1, 0), (2880, 1, 1024)),     # grows
        ((1024, 2, 262144, 4650, 5312, 1, 0), (5248, 1, 768)),     # 256 obstacles, items outnumber slots: tight slack
        ((256, 1, 65536, 4650, 5312, 1, 0), (5312, 1, 768)),       # ... a slot for every item: the eighth stays (768: the unrounded count; the granule rule gives two per CU)
        ((1024, 1, 262144, -1, 0, 0, 0), (7424, 0, 512)),          # first tick, 256 obstacles
        ((64, 1, 12800, 9000, 2048, 1, 0), (8192, 1, 512)),        # need above the maximum
        ((64, 1, 0, 0, 256, 1, 0), (64, 1, 2048)),                 # need 0
        ((64, 1, 0, -1, 0, 0, 0), (256, 0, 2048)),                 # no obstacles, first tick
        ((96, 1, 6144, 3000, 600, 0, FIXED), (600, 0, 2048)),      # fixed budget
        ((96, 1, 6144, 3000, 0, 0, DENSE), (0, 0, 2048)),          # dense forced
    ]
    for args, want in rows:
        out = [i32(-7) for _ in range(3)]
        assert lib.pp_search_budget(7344, 4096, 8192, 8192, 256, *args, *(ctypes.byref(o) for o in out)) == 0
        assert tuple(o.value for o in out) == want, (args, want)


def _planner(dm, cfg, n, group, n_obs=256, **kw):
    """A handle with DMPP_TICK_GROUP=group (read at pp_create); extra environment (DMPP_PIPELINE_MIN) through kw."""
    env = dict(kw.pop("env", {}), DMPP_TICK_GROUP=str(group))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return dm.Planner(cfg, max_scenes=n, max_obs_total=max(n * max(n_obs, 256), 1), **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pair(dm, cfg, sc, group, **kw):
    n = len(sc["scene_in"])
    pls = [_planner(dm, cfg, n, g, n_obs=int(sc["n_obs"]), **dict(kw)) for g in (group, 1)]
    for pl in pls:
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
    return pls


def _same(pls, tag, paths=(0, 7)):
    a, b = pls
    bad = compare(a.get_plan(), b.get_plan(), "plan") + compare(a.get_state(), b.get_state(), "state")
    ga, gb = a.get_grid_out(), b.get_grid_out()
    bad += compare(ga, gb, "grid")
    assert not bad, tag + "\n" + "\n".join(bad[:20])
    assert ga.tobytes() == gb.tobytes(), tag
    for s in paths:
        if s < a.n:
            k = int(gb["path_len"][s])
            assert (a.get_path(s, k) == b.get_path(s, k)).all(), (tag, s)


def _scenes(dm, cfg, seed, n, n_obs):
    return dm.gen_scenes(cfg, seed, n, n_obs, junction_every=8)


@pytest.mark.gpu
@pytest.mark.parametrize("group,n_ticks", [(3, 7), (4, 5), (2, 3)])
def test_odd_tick_counts(dm, group, n_ticks):
    """Tick counts that leave a partial group: pp_sync launches it."""
    cfg = dm.default_config(256)
    sc = _scenes(dm, cfg, 31, 256, 24)
    pls = _pair(dm, cfg, sc, group)
    for pl in pls:
        for _ in range(n_ticks):
            pl.tick()
        pl.sync()
    _same(pls, f"G={group}, {n_ticks} ticks")


@pytest.mark.gpu
def test_reads_in_the_middle_of_a_group(dm):
    """pp_sync, pp_get_grid_out and pp_get_path after 1, 2, ... ticks of a group of four: each read flushes the open group, and
    the ticks after it start a new one."""
    cfg = dm.default_config(256)
    sc = _scenes(dm, cfg, 32, 300, 32)
    pls = _pair(dm, cfg, sc, 4, order_cap=512)
    for step, k in enumerate((1, 2, 3, 5, 1, 2)):
        for pl in pls:
            for _ in range(k):
                pl.tick()
        if step % 3 == 0:
            for pl in pls:
                pl.sync()
        if step % 3 == 1:                   # the expansion order first, with the group still open: pp_get_order flushes it
            orders = [[pl.get_order(s_, 512) for s_ in (0, 5, 299)] for pl in pls]
            go = pls[1].get_grid_out()
            for i, s_ in enumerate((0, 5, 299)):
                k = min(int(go["n_expanded"][s_]), 512)
                assert (orders[0][i][:k] == orders[1][i][:k]).all(), (step, s_)
        _same(pls, f"after step {step} ({k} ticks)", paths=(0, 5, 299))
        for pl in pls:                      # pp_get_search_info with a group open (dense-scene count only: it must flush too)
            pl.tick()
            dense = ctypes.c_int(-1)
            assert pl.lib.pp_get_search_info(pl.h, None, None, ctypes.byref(dense)) == 0
            assert 0 <= dense.value <= pl.n
        _same(pls, f"after step {step} + 1", paths=(0, 299))


@pytest.mark.gpu
def test_streamed_ticks_fetched_every_tick(dm):
    """New inputs every tick and the results of every tick downloaded without a host sync: the same on both handles."""
    cfg = dm.default_config(256)
    n, n_obs = 256, 16
    sc = _scenes(dm, cfg, 33, n, n_obs)
    pls = _pair(dm, cfg, sc, 4)
    for pl in pls:                          # two grouped ticks before streaming begins (pp_update_async flushes them)
        pl.tick()
        pl.tick()
    rng = np.random.default_rng(5)
    snaps = []
    for t in range(6):
        move_ego(sc, 1)
        sc["obs_pool"]["x"] += rng.uniform(-0.3, 0.3, len(sc["obs_pool"]))
        snaps.append((dm.pinned_copy(sc["scene_in"]), dm.pinned_copy(sc["obs_pool"])))
    outs = []
    for pl in pls:
        plans = [dm.pinned_empty(n, dm.PlanOut) for _ in snaps]
        grids = [dm.pinned_empty(n, dm.GridOut) for _ in snaps]
        ids = []
        for t, (a, b) in enumerate(snaps):
            pl.update_async(a, b)
            pl.tick()
            ids.append(pl.fetch_async(plans[t], grids[t]))
        for i in ids:
            pl.wait_tick(i)
        outs.append([(p.copy(), g.copy()) for p, g in zip(plans, grids)])
    for t, ((pa, ga), (pb, gb)) in enumerate(zip(*outs)):
        bad = compare(pa, pb, "plan") + compare(ga, gb, "grid")
        assert not bad, f"streamed tick {t}\n" + "\n".join(bad[:20])
    _same(pls, "after the streamed ticks")


@pytest.mark.gpu
def test_grid_stage_switch_and_n_change_mid_group(dm):
    """pp_set_config (grid stage off, then on) and a smaller batch (pp_set_scenes) in the middle of a group."""
    cfg = dm.default_config(256)
    sc = _scenes(dm, cfg, 34, 320, 24)
    pls = _pair(dm, cfg, sc, 3)
    off = cfg.copy()
    off["grid_stage"] = 0
    small = _scenes(dm, cfg, 35, 260, 24)
    for pl in pls:
        pl.tick()
        pl.tick()
        pl.set_config(off)
        pl.tick()
        pl.set_config(cfg)
        pl.tick()
        pl.tick()
        pl.set_scenes(small)                 # n changes with a group open
        pl.set_state(small["state"])
        for _ in range(4):
            pl.tick()
        pl.sync()
    _same(pls, "after the switches")


@pytest.mark.gpu
def test_dynamic_obstacles_replanned_every_tick(dm):
    """BASELINE configs[3] in small: moving obstacles, replan every tick."""
    cfg = dm.default_config(256)
    cfg["dynamic_obstacles"] = 1
    cfg["force_replan"] = 1
    sc = _scenes(dm, cfg, 36, 256, 96)
    pls = _pair(dm, cfg, sc, 4)
    for pl in pls:
        for _ in range(6):
            pl.tick()
        pl.sync()
    _same(pls, "dynamic obstacles")


@pytest.mark.gpu
def test_spilling_scene_inside_a_group(dm):
    """A scene whose open list outgrows LDS (k_search_spill searches it again) in groups of three ticks: a one-scene handle
    made to run piped (DMPP_PIPELINE_MIN=1), so that the spill area and the retry list are per work item."""
    from grid_scenes import pebble_field
    cfg = dm.default_config(1024)
    cfg["bucket_cap"] = 16384
    cfg["max_path"] = 32768
    sc = pebble_field(dm, cfg, n_side=40, radius=0.05)
    pls = _pair(dm, cfg, sc, 3, env={"DMPP_PIPELINE_MIN": "1"}, order_cap=1 << 18)
    for pl in pls:
        for _ in range(4):
            pl.tick()
        pl.sync()
    _same(pls, "spilling scene", paths=(0,))
    go = pls[1].get_grid_out()
    assert int(go["status"][0]) == 0
    k = int(go["n_expanded"][0])
    assert (pls[0].get_order(0, k) == pls[1].get_order(0, k)).all()


@pytest.mark.gpu
def test_launch_order_over_a_group(dm):
    """1024 scenes in groups of two: 2048 work items outnumber the search's workgroup slots, so k_order sorts the items of both
    ticks.  Odd tick counts leave a group of one flushed by pp_sync, whose launch order must cover its own items."""
    cfg = dm.default_config(512)
    sc = _scenes(dm, cfg, 37, 1024, 32)
    pls = _pair(dm, cfg, sc, 2)
    for k in (3, 1, 4, 5):
        for pl in pls:
            for _ in range(k):
                pl.tick()
            pl.sync()
        _same(pls, f"{k} ticks", paths=(0, 511, 1023))
