"""The set-up of `k_search` (csrc/kernels_s.hpp, `build_sparse_views` / `build_dense_views`): the footprints of a scene as a
flat list of (obstacle, line) items that the threads of the workgroup take in contiguous runs, the spans of a thread's first
`kRasterKeep` items kept in registers between the two passes, obstacles staged `kRasterChunk` at a time.

Every case is one scene.  `get_grid` (the builder at 4 waves = 256 threads) must equal `oracle.rasterise` cell for cell, and one
tick at n = 1 (the builder at 16 waves = 1024 threads inside `k_search`) must give the oracle's status, expansion count, path
length and digest.  The CPU test restates the item count of an obstacle from the box formula of `footprint_of` and asserts
that the list has a case on either side of every split of the walk, so that a later change of a constant fails there instead
of silently hollowing the cases out."""
import os
import re

import numpy as np
import pytest

import search_scenes as ss
from parity_util import compare

T4, T16 = 256, 1024                     # threads of the set-up: get_grid and batches | a tick of a handful of scenes


def raster_constants():
    with open(os.path.join(ss.CSRC, "kernels_s.hpp")) as f:
        ker = f.read()
    out = {}
    for name in ("kRasterChunk", "kRasterKeep"):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", ker)
        assert m, f"{name} not found in kernels_s.hpp"
        out[name] = int(m.group(1))
    m = re.search(r"kSearchSetupWaves\s*=\s*(\d+)\s*,", ker)
    mw = re.search(r"kSearchSetupWavesWide\s*=\s*(\d+)\s*;", ker)
    assert m and mw and int(m.group(1)) * 64 == T4 and int(mw.group(1)) * 64 == T16
    return out


# ---- discs, in cells relative to the grid origin: (x, y, radius) -----------------------------------------------------
def sub(ix, iy):
    """A sub-cell disc on the centre of cell (ix, iy): a box of 3 lines per axis, one cell occupied."""
    return (ix + 0.5, iy + 0.5, 0.3)


def out(k=0):
    """Far outside the grid on both axes: an empty clipped box."""
    return (-200.0 - 3.0 * k, -200.0, 0.4)


def half_out(ix, k=0):
    """Inside the grid in x, far outside in y: columns but no rows - still no items."""
    return (ix + 0.5, -300.0 - 2.0 * k, 2.0)


def subs(n, W, H, seed):
    """n sub-cell discs on distinct interior cells."""
    rng = np.random.default_rng([seed, W, H])
    cells = rng.choice((W - 4) * (H - 4), n, replace=False)
    return [sub(2 + int(c) % (W - 4), 2 + int(c) // (W - 4)) for c in cells]


def item_counts(W, H, cell, inflate, discs):
    """rows + columns of the clipped box of every disc (0 when the box is empty): the box formula of footprint_of, the disc
    given as it reaches the device (float32 radius)."""
    out_ = []
    for x, y, r in discs:
        R = float(np.float32(r * cell)) + inflate
        X, Y = x * cell, y * cell
        ix0 = max(int(np.floor((X - R) / cell)) - 1, 0)
        ix1 = min(int(np.floor((X + R) / cell)) + 1, W - 1)
        iy0 = max(int(np.floor((Y - R) / cell)) - 1, 0)
        iy1 = min(int(np.floor((Y + R) / cell)) + 1, H - 1)
        out_.append((iy1 - iy0 + 1) + (ix1 - ix0 + 1) if ix1 >= ix0 and iy1 >= iy0 else 0)
    return out_


CELL, INFLATE = 0.25, 0.0               # of ss.config (asserted in _scene)


def padded_to(discs, W, H, target):
    """`discs` followed by sub-cell discs - 6 items each in the interior, 5 on the lower border, 4 in a corner - up to exactly `target` items."""
    discs = list(discs)
    left = target - sum(item_counts(W, H, CELL, INFLATE, discs))
    corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    k = 0
    while left > 0:
        piece = next(p for p in (6, 5, 4) if left - p == 0 or (left - p >= 4 and left - p != 7))       # (1, 2, 3 and 7 items cannot be made up)
        d = sub(3 + 2 * (k % 60), 3 + 2 * (k // 60)) if piece == 6 else (sub(10 + 3 * (k % 35), 0) if piece == 5 else sub(*corners.pop()))
        assert item_counts(W, H, CELL, INFLATE, [d])[0] == piece
        discs.append(d)
        left -= piece
        k += 1
    assert left == 0 and sum(item_counts(W, H, CELL, INFLATE, discs)) == target
    return discs


def cases(k=None):
    k = k or raster_constants()
    C = k["kRasterChunk"]
    rng = np.random.default_rng(2601)
    some = [(30.3, 40.6, 9.1), (90.4, 20.3, 5.5), (64.0, 100.0, 14.2)]
    big40 = [(float(rng.uniform(30, 98)), float(rng.uniform(30, 98)), float(rng.uniform(46, 52))) for _ in range(40)]
    L = []                              # (name, W, H, discs)
    L.append(("m0", 128, 128, []))
    L.append(("m1", 128, 128, [(64.3, 64.6, 10.0)]))
    L.append(("m2", 128, 128, [sub(5, 5), (100.0, 30.0, 7.0)]))
    L.append(("few_items", 128, 128, subs(8, 128, 128, 1)))                                   # 48 items: most threads own nothing
    mid = [(40.3 + 10 * i, 30.4 + 15 * i, 18.0) for i in range(5)]
    L.append(("some_items", 128, 128, mid))                                                   # between 256 and 1024 items
    for target in (T4, 2 * T4, 2 * T4 + 1, T16, T16 + 1):                                     # (one chunk each: fewer than kRasterChunk discs)
        L.append((f"items_{target}", 128, 128, padded_to(some + (mid if target >= T16 else []), 128, 128, target)))
    L.append(("empty_first", 128, 128, [out(i) for i in range(5)] + some))
    L.append(("empty_last", 128, 128, some + [out(i) for i in range(5)]))
    L.append(("empty_runs", 128, 128, [some[0]] + [out(i) for i in range(3)] + [some[1], half_out(20), half_out(90, 1), some[2], out(9), sub(70, 70)]))
    L.append(("empty_all", 128, 128, [out(i) for i in range(10)]))
    L.append(("empty_chunk", 128, 128, subs(C, 128, 128, 2) + [out(i) for i in range(C)] + [(64.0, 64.0, 20.0)]))
    L.append(("whole_grid_disc", 128, 64, [sub(9, 9), (64.0, 32.0, 100.0), sub(100, 50), sub(101, 50), sub(0, 0), sub(127, 63)]))
    for m in (C - 1, C, C + 1, 2 * C + 1):
        L.append((f"chunk_{m}", 96, 64, subs(m - 2, 96, 64, m) + [(20.0, 20.0, 6.0), (70.0, 40.0, 11.0)]))
    L.append(("beyond_keep", 128, 128, big40))                                                # ~ 31 items per thread at 256 threads, ~ 8 at 1024
    L.append(("beyond_keep_chunks", 128, 128, [(float(rng.uniform(10, 118)), float(rng.uniform(10, 118)), 8.0) for _ in range(2 * C + 1)]))
    # positions up to 2047: the packing a | b << 16 of a kept span, and the widest line masks (K = 2)
    L.append(("wide_2048x32", 2048, 32, [(1000.3, 16.2, 740.0), sub(2040, 3), sub(2047, 31), (1900.0, 10.0, 140.0)]))
    return L


DENSE = ["m2", "empty_runs", "beyond_keep", "chunk_%d"]           # also under DMPP_SEARCH_GBM=1 (chunk_%d: 2 C + 1)
OVERFLOW = "beyond_keep"                                           # ... and under a DMPP_LDS_BUDGET it does not fit
OVERFLOW_BUDGET = 16
CASE_NAMES = ["m0", "m1", "m2", "few_items", "some_items", "items_256", "items_512", "items_513", "items_1024", "items_1025", "empty_first",
              "empty_last", "empty_runs", "empty_all", "empty_chunk", "whole_grid_disc", "chunk_C-1", "chunk_C", "chunk_C+1", "chunk_2C+1",
              "beyond_keep", "beyond_keep_chunks", "wide_2048x32"]          # a literal: collecting the tests reads no source file


def _case(i):
    L = cases()
    assert len(L) == len(CASE_NAMES)
    return L[i]


def test_case_list_crosses_every_split_on_both_sides():
    k = raster_constants()
    C, KEEP = k["kRasterChunk"], k["kRasterKeep"]
    assert KEEP >= 11                                             # every scene of the benchmark keeps everything (<= 2,594 items on 256 threads)
    L = cases(k)
    assert [n for n, _, _, _ in L][:16] == CASE_NAMES[:16]
    info = {}
    for name, W, H, discs in L:
        cnt = item_counts(W, H, CELL, INFLATE, discs)
        chunks = [sum(cnt[b:b + C]) for b in range(0, len(cnt), C)]
        info[name] = dict(m=len(discs), cnt=cnt, total=sum(cnt), chunks=chunks, W=W, H=H)
    ms = {v["m"] for v in info.values()}
    assert {0, 1, 2, C - 1, C, C + 1, 2 * C + 1} <= ms
    first = {n: (v["chunks"] or [0])[0] for n, v in info.items()}          # items of the first chunk
    for T in (T4, T16):
        assert any(0 < t < T for t in first.values()) and any(t > T for t in first.values())           # threads that own nothing | all own some
        assert any(t > 0 and t % T == 0 for t in first.values()) and any(t > T and t % T == 1 for t in first.values())
    per = lambda t, T: -(-t // T)
    # kept spans only | spans computed again in pass 2, and the same list on both sides of the split at the two widths
    assert any(0 < per(t, T4) <= KEEP for t in first.values()) and any(per(t, T4) > KEEP for t in first.values())
    assert per(first["beyond_keep"], T4) > 2 * KEEP and per(first["beyond_keep"], T16) <= KEEP
    assert per(first["beyond_keep_chunks"], T4) > KEEP and per(info["beyond_keep_chunks"]["chunks"][1], T4) > 0      # chunk 0 keeps and recomputes, chunk 1 recomputes
    assert info["chunk_%d" % (2 * C + 1)]["chunks"][2] > 0 and len(info["chunk_%d" % (C + 1)]["chunks"]) == 2
    # empty clipped boxes: first, last, in runs between obstacles with items, a whole chunk, a whole scene
    e = lambda n: [c == 0 for c in info[n]["cnt"]]
    assert e("empty_first")[:5] == [True] * 5 and not e("empty_first")[5] and not any(e("empty_last")[:3]) and all(e("empty_last")[3:])
    r = e("empty_runs")
    assert r == [False, True, True, True, False, True, True, False, True, False]
    assert info["empty_all"]["total"] == 0 and info["empty_all"]["m"] > 0
    assert info["empty_chunk"]["chunks"][1] == 0 and info["empty_chunk"]["chunks"][0] > 0 and info["empty_chunk"]["chunks"][2] > 0
    # one obstacle with every line of both axes, beside sub-cell ones; rows != columns
    w = info["whole_grid_disc"]
    assert w["W"] != w["H"] and max(w["cnt"]) == w["W"] + w["H"] and sorted(w["cnt"])[:2] == [4, 4] and w["cnt"].count(6) >= 2
    assert max(info["whole_grid_disc"]["cnt"]) > per(w["total"], T4)           # threads whose whole run lies inside one obstacle
    assert info["wide_2048x32"]["W"] == 2048 and max(info["wide_2048x32"]["cnt"]) > 1400           # spans that end beyond position 1023
    names = set(info)
    assert {d if "%d" not in d else d % (2 * C + 1) for d in DENSE} <= names and OVERFLOW in names


# ---- the GPU side -----------------------------------------------------------------------------------------------------
def _scene(dm, W, H, discs):
    cfg = ss.config(dm, W, H)
    cell = float(cfg["cell"][0])
    assert cell == CELL and float(cfg["inflate"][0]) == INFLATE
    m = len(discs)
    sc = dm.gen_scenes(cfg, 0, 1, m, junction_every=0)
    si = sc["scene_in"]
    sc["mot_pool"][:] = 0
    ox, oy = float(si["grid_origin"]["x"][0]), float(si["grid_origin"]["y"][0])
    ob = sc["obs_pool"]
    for j, (x, y, r) in enumerate(discs):
        ob["x"][j], ob["y"][j], ob["radius"][j], ob["type"][j] = ox + x * cell, oy + y * cell, r * cell, 0
    assert int(si["obs_n"][0]) == m and int(si["obs_off"][0]) == 0
    gp = si["loc"]["globalpoint"]
    gp["x"][0], gp["y"][0] = ox + (0.06 * W + 0.5) * cell, oy + (0.08 * H + 0.5) * cell
    si["goal"]["x"][0], si["goal"]["y"][0] = ox + (0.93 * W + 0.5) * cell, oy + (0.9 * H + 0.5) * cell
    return cfg, sc, (ox, oy)


def _check_one(dm, oracle, pl, cfg, sc, origin, tag, expect_dense=None):
    m = int(sc["scene_in"]["obs_n"][0])
    pl.set_scenes(sc)
    pl.set_state(sc["state"])
    pl.tick(sync=True)
    if expect_dense is not None:
        assert pl.search_info()[2] == expect_dense, (tag, pl.search_info())
    g = pl.get_grid_out()[0]
    _, go, grid_o, _, _ = oracle.plan_tick_one(cfg, sc, 0, sc["state"].copy())
    grid_r = oracle.rasterise(cfg, origin, sc["obs_pool"][:m])
    assert np.array_equal(grid_r, grid_o), tag
    grid_g = pl.get_grid(0)
    assert np.array_equal(grid_g, grid_r), f"{tag}: get_grid differs from the oracle in {int((grid_g != grid_r).sum())} cells"
    assert int(g["status"]) == int(go["status"]), (tag, int(g["status"]), int(go["status"]))
    if int(go["status"]) not in (3, 7):                            # OVERFLOW / COST_RANGE: only the status is specified
        for f in ("n_expanded", "path_len", "order_digest"):
            assert int(g[f]) == int(go[f]), (tag, f, int(g[f]), int(go[f]))


@pytest.fixture(scope="module")
def planner_for(dm):
    made = {}

    def get(cfg, W, H):
        if (W, H) not in made:
            # the largest budget the grid allows, fixed: no case goes the dense way because the adaptive budget started small
            old = os.environ.get("DMPP_LDS_BUDGET")
            os.environ["DMPP_LDS_BUDGET"] = str(W * H // 32)
            try:
                made[(W, H)] = dm.Planner(cfg, device=0, max_scenes=1, max_obs_total=512)
            finally:
                if old is None:
                    os.environ.pop("DMPP_LDS_BUDGET", None)
                else:
                    os.environ["DMPP_LDS_BUDGET"] = old
        return made[(W, H)]
    yield get
    for pl in made.values():
        pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASE_NAMES)), ids=CASE_NAMES)
def test_items_sparse(dm, oracle, planner_for, i):
    name, W, H, discs = _case(i)
    cfg, sc, origin = _scene(dm, W, H, discs)
    _check_one(dm, oracle, planner_for(cfg, W, H), cfg, sc, origin, name, expect_dense=0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gbm", "overflow"])
def test_items_dense(dm, oracle, form):
    """The dense form takes the same walk: forced for every scene, and for a scene that does not fit a tiny budget."""
    C = raster_constants()["kRasterChunk"]
    env = {"DMPP_SEARCH_GBM": "1"} if form == "gbm" else {"DMPP_LDS_BUDGET": str(OVERFLOW_BUDGET)}
    want = [d if "%d" not in d else d % (2 * C + 1) for d in DENSE] if form == "gbm" else [OVERFLOW]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        for name, W, H, discs in cases():
            if name not in want:
                continue
            cfg, sc, origin = _scene(dm, W, H, discs)
            pl = dm.Planner(cfg, device=0, max_scenes=1, max_obs_total=512)
            try:
                _check_one(dm, oracle, pl, cfg, sc, origin, f"{form}/{name}", expect_dense=1)
                if form == "overflow":
                    assert pl.search_info()[0] == OVERFLOW_BUDGET          # (dense == 1 above: the scene did not fit it)
            finally:
                pl.close()
    finally:
        for k_, v in old.items():
            if v is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v


@pytest.mark.gpu
def test_items_batch(dm, oracle):
    """256 generated scenes, 128 x 128, 24 obstacles: the 4-wave set-up inside a real launch of the batch path."""
    cfg = dm.default_config(128)
    n = 256
    sc = dm.gen_scenes(cfg, 2600, n, 24, junction_every=4)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * 24)
    try:
        st_o = sc["state"].copy()
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
        pl.tick(sync=True)
        plan_o, gout_o, grids_o = oracle.plan_tick_batch(cfg, sc, st_o, n_threads=8, want_grid=True, keep_grids=True)
        gout_g = pl.get_grid_out()
        bad = compare(gout_g["status"], gout_o["status"], "grid.status")
        keep = (gout_o["status"] != 3) & (gout_o["status"] != 7)
        bad += compare(gout_g[keep], gout_o[keep], "grid") + compare(pl.get_plan(), plan_o, "plan") + compare(pl.get_state(), st_o, "state")
        assert not bad, "\n".join(bad[:20])
        for s in (0, 97, 255):
            assert np.array_equal(pl.get_grid(s), grids_o[s]), s
    finally:
        pl.close()
