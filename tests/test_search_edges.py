"""The jump-point search (G2; `search_core` of csrc/kernels_s.hpp, run as k_search<K, SW> and k_search_spill) on
bitmaps that sit ON its case splits, against a model written from the specification (tests/grid_search_model.py).

The scenes and the form the kernel takes for each are tests/search_scenes.py: a bitmap reaches the device as one small disc
per occupied cell with `inflate = 0`.  CPU tests: the model against the oracle - on every scene of the case list, on 400
further random bitmaps, on the generated scenes of test_oracle_properties - and the coverage of the case list (every split
crossed on both sides, asserted from the model's trace and `forms()`).  GPU tests: the device against the model in every
field the status defines, against the oracle for the whole tick (PlanOut and SceneState included), `get_grid` against the
bitmap, and a crafted scene's GridOut, expansion order and path the same bytes in every form of the launch: alone, in a batch
of 128 (sixteen set-up waves; every case early and late in the batch), in a batch of 129 (four set-up waves), all cases of a
group in one launch, and with DMPP_SEARCH_GBM=1 (dense views).

All integers: no tolerance anywhere but in the float scores of the whole-tick comparison (parity_util.RTOL).  A scene that
ends OVERFLOW or COST_RANGE is compared on its status alone; such scenes are < 10 % of a random family."""
import os
import time

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
STATUS_ONLY = (gm.OVERFLOW, gm.COST_RANGE)

class _Groups:
    """The case list by group name, built on first use (collecting the tests builds no bitmap and reads no source file)."""

    def __getitem__(self, name):
        return self._all()[name]

    def values(self):
        return self._all().values()

    def _all(self):
        return _cached("groups", lambda: {g.name: g for g in ss.groups()})


GROUPS = _Groups()


def _okey(over):
    return tuple(sorted(over.items()))


def _cell(c, p):
    return p[1] * c.W + p[0]


def _model(dm, case, over):
    """(model result, config) of a case under `over` (once per process, never modified)."""
    def make():
        cfg = ss.config(dm, case.W, case.H, **over)
        m = gm.search(case.bitmap.tobytes(), case.W, case.H, _cell(case, case.start), _cell(case, case.goal),
                      int(cfg["max_expansions"][0]), int(cfg["bucket_cap"][0]), int(cfg["max_path"][0]))
        return m, cfg
    return _cached(("model", case.name, _okey(over)), make)


def _against_model(status, rec, order, path, m, tag):
    """Mismatches of a search result (oracle's or device's) against the model's, in every field the status defines."""
    if status != m["status"]:
        return [f"{tag}: status {status} vs model {m['status']} ({gm.STATUS_NAMES[m['status']]})"]
    if status in STATUS_ONLY:
        return []
    bad = [f"{tag}.{f}: {int(rec[f])} vs model {m[f]}" for f in FIELDS if int(rec[f]) != m[f]]
    if order is not None and list(order) != m["order"]:
        k = next((i for i, (a, b) in enumerate(zip(order, m["order"])) if a != b), min(len(order), len(m["order"])))
        bad.append(f"{tag}.order: differs from the model's at expansion {k} (lengths {len(order)} / {len(m['order'])})")
    if path is not None and list(path) != m["path"]:
        bad.append(f"{tag}.path: differs from the model's (lengths {len(path)} / {len(m['path'])})")
    return bad


def _all_cases():
    for g in GROUPS.values():
        for over in g.overs:
            for c in g.cases:
                yield g, over, c


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_model_constants_are_the_kernels():
    k = ss.kernel_constants()
    assert (gm.BATCH, gm.DIAG_JUMP, gm.F_LIMIT) == (k["DMPP_JPS_BATCH"], k["DMPP_DIAG_JUMP"], k["DMPP_F_LIMIT"])
    assert [gm.FOUND, gm.NO_PATH, gm.LIMIT, gm.OVERFLOW, gm.GOAL_BLOCKED, gm.PATH_TRUNC, gm.INTERNAL, gm.COST_RANGE] == list(range(8))


def test_oracle_equals_model_on_the_case_list(dm, oracle):
    """Status, counters, path cost and length, the whole expansion order, the digest and the path, on every committed scene under
    every config it runs with; the oracle's peak of live entries is the model's.  start == goal on an occupied cell is
    GOAL_BLOCKED in both."""
    bad, hist = [], {}
    for g, over, c in _all_cases():
        m, cfg = _model(dm, c, over)
        out, order, path = oracle.grid_search(cfg, c.bitmap, _cell(c, c.start), _cell(c, c.goal), order_cap=c.W * c.H)
        status = int(out["status"][0])
        hist[status] = hist.get(status, 0) + 1
        tag = f"{g.name}/{c.name}{over or ''}"
        bad += _against_model(status, out[0], order.tolist(), path.tolist(), m, tag)
        if status not in STATUS_ONLY + (gm.GOAL_BLOCKED,) and oracle.last_peak_open() != m["peak_open"]:
            bad.append(f"{tag}: peak of live entries {oracle.last_peak_open()} vs model {m['peak_open']}")
        if status not in STATUS_ONLY and m["order_digest"] != gm.digest_of(m["order"]):
            bad.append(f"{tag}: the model's digest is not the digest of its order")
    print("statuses:", {gm.STATUS_NAMES[s]: n for s, n in sorted(hist.items())})
    assert not bad, "\n".join(bad[:20])
    by_name = {c.name: _model(dm, c, {})[0] for c in GROUPS["small"].cases}
    assert by_name["start_is_goal_occupied"]["status"] == gm.GOAL_BLOCKED and by_name["start_is_goal"]["status"] == gm.FOUND


def test_oracle_equals_model_on_400_random_bitmaps(dm, oracle):
    """64 x 64, 96 x 32 and 32 x 160, densities 0.02 - 0.45, random start and goal, now and then an occupied goal, a small
    max_expansions or bucket_cap = 16."""
    rng = np.random.default_rng(1812)
    bad, hist = [], {}
    for trial in range(400):
        W, H = [(64, 64), (96, 32), (32, 160)][trial % 3]
        cfg = dm.default_config(W, H)
        cfg["bucket_cap"] = 16 if trial % 11 == 0 else 4096
        cfg["max_expansions"] = int(rng.integers(1, 200)) if trial % 9 == 0 else 100000
        grid = (rng.random((H, W)) < float(rng.uniform(0.02, 0.45))).astype(np.uint8)
        st, go = int(rng.integers(0, W * H)), int(rng.integers(0, W * H))
        if trial % 13:
            grid.reshape(-1)[go] = 0
        out, order, path = oracle.grid_search(cfg, grid, st, go, order_cap=W * H)
        m = gm.search(grid.tobytes(), W, H, st, go, int(cfg["max_expansions"][0]), int(cfg["bucket_cap"][0]), int(cfg["max_path"][0]), trace=False)
        status = int(out["status"][0])
        hist[status] = hist.get(status, 0) + 1
        bad += _against_model(status, out[0], order.tolist(), path.tolist(), m, f"trial {trial} ({W}x{H})")
    print("statuses:", {gm.STATUS_NAMES[s]: n for s, n in sorted(hist.items())})
    assert not bad, "\n".join(bad[:20])
    assert sum(hist.get(s, 0) for s in STATUS_ONLY) <= 40, hist               # compared on the status alone: at most 10 %
    assert hist.get(gm.FOUND, 0) >= 250 and all(hist.get(s, 0) >= 3 for s in (gm.LIMIT, gm.OVERFLOW, gm.GOAL_BLOCKED)), hist


def test_oracle_equals_model_on_generated_scenes(dm, oracle):
    """The disc scenes of test_oracle_properties::test_grid_search_is_optimal_and_well_formed, rasterised by the oracle."""
    cfg = dm.default_config(128)
    sc = dm.gen_scenes(cfg, 40, 24, 24, junction_every=0)
    bad = []
    for s in range(24):
        grid = oracle.rasterise(cfg, (0.0, 0.0), sc["obs_pool"][s * 24:(s + 1) * 24])
        si = sc["scene_in"][s]
        st = oracle.cell_of(cfg, (0.0, 0.0), float(si["loc"]["globalpoint"]["x"]), float(si["loc"]["globalpoint"]["y"]))
        go = oracle.cell_of(cfg, (0.0, 0.0), float(si["goal"]["x"]), float(si["goal"]["y"]))
        out, order, path = oracle.grid_search(cfg, grid, st, go, order_cap=128 * 128)
        m = gm.search(grid.tobytes(), 128, 128, st, go, int(cfg["max_expansions"][0]), int(cfg["bucket_cap"][0]), int(cfg["max_path"][0]), trace=False)
        bad += _against_model(int(out["status"][0]), out[0], order.tolist(), path.tolist(), m, f"scene {s}")
    assert not bad, "\n".join(bad[:20])


def test_bitmap_scenes_rasterise_back_to_the_bitmap(dm, oracle):
    """from_bitmap: the discs of a scene give the bitmap back under G1 (`oracle.rasterise` and its brute-force form), and ego and
    goal land on the cells asked for - a random bitmap, the seam bitmap with a start per copy, 2048 x 32 and 32 x 2048."""
    seam = GROUPS["seam"].cases
    picks = [(c.bitmap, c.start, c.goal) for c in (GROUPS["random/64x64"].cases[0], GROUPS["strip/2048"].cases[0], GROUPS["strip/32x2048"].cases[0])]
    picks.append((seam[0].bitmap, [c.start for c in seam[:3]], [c.goal for c in seam[:3]]))
    for bitmap, start, goal in picks:
        H, W = bitmap.shape
        cfg = ss.config(dm, W, H)
        n = len(start) if isinstance(start, list) else 2
        sc = ss.from_bitmap(dm, cfg, bitmap, start, goal, n_copies=n)
        assert len(sc["scene_in"]) == n and sc["n_obs"] == max(1, int(np.count_nonzero(bitmap))) and not sc["mot_pool"]["vx"].any()
        for s in range(n):
            si = sc["scene_in"][s]
            origin = (float(si["grid_origin"]["x"]), float(si["grid_origin"]["y"]))
            obs = sc["obs_pool"][int(si["obs_off"]):int(si["obs_off"]) + int(si["obs_n"])]
            assert np.array_equal(oracle.rasterise(cfg, origin, obs), bitmap)
            assert np.array_equal(oracle.rasterise(cfg, origin, obs, brute=True), bitmap)
            st = start[s] if isinstance(start, list) else start
            go = goal[s] if isinstance(goal, list) else goal
            assert oracle.cell_of(cfg, origin, float(si["loc"]["globalpoint"]["x"]), float(si["loc"]["globalpoint"]["y"])) == st[1] * W + st[0]
            assert oracle.cell_of(cfg, origin, float(si["goal"]["x"]), float(si["goal"]["y"])) == go[1] * W + go[0]


def _rows(dm, names, n_items=1):
    k = ss.kernel_constants()
    rows = []
    for name in names:
        g = GROUPS[name]
        for over in g.overs:
            for c in g.cases:
                m, cfg = _model(dm, c, over)
                rows.append((g, over, c, m, ss.forms(m, cfg, n_items, k)))
    return rows


def _form_line(g, over, c, m, f):
    return (f"{g.name:18s} {c.name:26s} {str(over.get('max_expansions', over.get('bucket_cap', over.get('max_path', '')))):>5s} "
            f"{gm.STATUS_NAMES[m['status']]:12s} exp {m.get('n_expanded', -1):5d} hops {m.get('hops', 0):4d} live {m['peak_open']:4d} slots {f['peak_slots']:4d} "
            f"K {f['K']} spill@ {str(f['closed_spill_step']):>4s} upper {int(f['upper_keys'])} squeezes {len(f['squeezes']):2d} retry {int(f['retry'])} walk {f['path_walk']}")


def test_case_list_crosses_every_split_on_both_sides(dm):
    """Every "so that" of the case list, from the model's records and forms(): a changed constant of the kernel, or a changed
    scene, fails here instead of hollowing the cases out."""
    k = ss.kernel_constants()
    open_cap, cmax = k["DMPP_OPEN_CAP"], k["kClosedMax"]
    assert [g.name for g in GROUPS.values()] == ss.GROUP_NAMES
    CRAFTED = [g.name for g in GROUPS.values() if g.crafted]
    rows = _rows(dm, CRAFTED)
    for r in rows:
        if r[0].name != "seam":
            print(_form_line(*r))
    by = lambda name: [r for r in rows if r[0].name == name]
    F = lambda name: [r[4] for r in by(name)]
    M = lambda name: [r[3] for r in by(name)]

    # -- random families: few scenes compared on the status alone; the 128 x 128 family straddles 256, 384 and 512
    for name in ("random/64x64", "random/96x32", "random/128x128"):
        ms = [r[3] for r in _rows(dm, [name])]
        assert 10 * sum(m["status"] in STATUS_ONLY for m in ms) <= len(ms), name
    fam = _rows(dm, ["random/128x128"])
    assert any(r[4]["retry"] for r in fam) and any(not r[4]["retry"] for r in fam)
    assert any(r[4]["upper_keys"] for r in fam) and all(r[4]["closed_spill_step"] is not None for r in fam)
    assert any(r[4]["closed_spill_step"] is None for r in _rows(dm, ["random/64x64"]))

    # -- word boundaries of the scans (144 starts of a 12 x 12 window across the seam, one launch)
    seam = by("seam")
    assert len(seam) == 144 and len({r[2].start for r in seam}) == 144 and all(r[3]["status"] == gm.FOUND for r in seam)
    x0, y0, n = ss.SEAM_WINDOW
    assert x0 <= 63 < 64 < x0 + n and y0 <= 63 < 64 < y0 + n
    b = ss.seam_bitmap()
    for gx, gy in ss.SEAM_GOALS:                      # the goal lies in a word that holds no obstacle bit, in either view
        assert not b[gy, gx // 32 * 32:gx // 32 * 32 + 32].any() and not b[gy // 32 * 32:gy // 32 * 32 + 32, gx].any()
    for q in (31, 32, 95, 96):                        # obstacles on both sides of a seam, in x and in y
        assert b[:, q].any() and b[q, :].any()
    assert any(b[y, 31] and b[y, 32] for y in range(128)) and any(b[31, x] and b[32, x] for x in range(128))
    alone_at = lambda y, x: b[y, x] and b[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].sum() == 1
    for bit in (0, 31, 32):                           # isolated cells on bits 0, 31 and 32, beside a row and beside a column of the window
        assert any(alone_at(y, x) for y in range(y0 - 1, y0 + n + 1) for x in range(128) if x % 64 == bit), bit
        assert any(alone_at(y, x) for x in range(x0 - 1, x0 + n + 1) for y in range(128) if y % 64 == bit), bit
    J = [j for r in seam for j in r[3]["jumps"]]
    for d in (0, 2, 4, 6):
        jj = [j for j in J if j["dir"] == d]
        assert any(j["bit_start"] == 31 for j in jj) and any(j["bit_start"] == 0 for j in jj), d
        assert any(j["bit_stop"] == 31 for j in jj) and any(j["bit_stop"] == 0 for j in jj), d
        assert any(j["seams"] >= 2 for j in jj), d
    for d in (1, 3, 5, 7):
        jj = [j for j in J if j["dir"] == d]
        assert {j["end"] for j in jj} == {"goal", "forced", "straight", "cap"}, d
        assert any(j["end"] == "cap" and j["run"] == k["DMPP_DIAG_JUMP"] for j in jj), d
        assert any(j["end"] == "straight" and j["run"] == k["DMPP_DIAG_JUMP"] - 1 for j in jj), d

    # -- edges of the grid, the degenerate scenes
    small = {r[2].name: r for r in by("small")}
    ends = {p for r in by("small") for p in (r[2].start, r[2].goal)}
    assert {(0, 0), (63, 0), (63, 63), (0, 63)} <= ends
    assert all(any(p[a] == v for p in ends if p not in ((0, 0), (63, 0), (63, 63), (0, 63))) for a in (0, 1) for v in (0, 63))
    bb = ss.border_bitmap()
    assert bb[0].any() and bb[63].any() and bb[:, 0].any() and bb[:, 63].any()
    assert all(small[n_][3]["status"] == gm.FOUND for n_ in small if n_.startswith(("corner/", "border/", "plain/", "goal_adjacent/")))
    assert small["start_is_goal"][3]["path"] == [20 * 64 + 20] and small["start_is_goal"][3]["n_expanded"] == 1
    assert small["start_is_goal_occupied"][3]["status"] == gm.GOAL_BLOCKED and small["goal_occupied"][3]["status"] == gm.GOAL_BLOCKED
    assert bb[0, 12] and small["start_occupied"][3]["status"] == gm.FOUND
    assert all(small[f"goal_adjacent/{d}"][3]["path_len"] == 2 for d in range(8))
    for n_ in ("walled_in", "walled_in_corner"):
        assert small[n_][3]["status"] == gm.NO_PATH and small[n_][3]["n_expanded"] == 1 and small[n_][3]["n_pushed"] == 1
    full, trunc = M(f"max_path/{ss.MAX_PATH_LEN}")[0], M(f"max_path/{ss.MAX_PATH_LEN - 1}")[0]
    assert full["status"] == gm.FOUND and full["path_len"] == ss.MAX_PATH_LEN
    assert trunc["status"] == gm.PATH_TRUNC and trunc["path"] == full["path"][1:]

    # -- non-square grids: the first widths of K = 1 and K = 2 with the same cells, x and y through the 12-bit fields
    assert [F(f"strip/{w}")[0]["K"] for w in ss.STRIP_WIDTHS] == [0, 1, 1, 2]
    assert [w // 32 for w in ss.STRIP_WIDTHS] == [k["lw_k0"], k["lw_k0"] + 1, k["lw_k1"], k["lw_k1"] + 1]
    s512, s544 = by("strip/512")[0][2].bitmap, by("strip/544")[0][2].bitmap
    assert np.array_equal(s512[:, 1:511], s544[:, 1:511]) and s512.any()
    s1024, s1056 = by("strip/1024")[0][2].bitmap, by("strip/1056")[0][2].bitmap
    assert np.array_equal(s1024[:, 1:1023], s1056[:, 1:1023]) and np.array_equal(s512[:, 1:511], s1056[:, 1:511])
    for name, axis in (("strip/2048", 0), ("strip/32x2048", 1)):
        r = by(name)[0]
        assert r[4]["K"] == 2 and r[3]["status"] == gm.FOUND and {r[2].start[axis], r[2].goal[axis]} == {0, 2047}
        assert any(c_ % r[2].W == 2047 if axis == 0 else c_ // r[2].W == 2047 for c_ in r[3]["order"])
        assert any(j["dir"] in ((0, 4) if axis == 0 else (2, 6)) and (j["start"][axis] + (j["run"] if j["dir"] in (0, 2) else 0)) >> 5 == 63 for j in r[3]["jumps"])

    # -- the closed set leaving LDS: LIMIT sweeps across n_exp + 4 > kClosedMax, FOUND on either side, every place in a batch
    last_place = set()
    for name, K in (("closed_sweep/128", 0), ("closed_sweep/1056", 2)):
        sw = by(name)
        assert [r[1]["max_expansions"] for r in sw] == [cmax[K] + d for d in ss.SWEEP_SPAN]
        assert all(r[3]["status"] == gm.LIMIT and r[3]["n_expanded"] == r[1]["max_expansions"] and r[4]["K"] == K and not r[4]["retry"] for r in sw)
        spilled = [r[4]["closed_spill_step"] is not None for r in sw]
        assert not spilled[0] and spilled[-1] and spilled == sorted(spilled), (name, spilled)
        last_place |= {len(r[3]["steps"][-1]["closed"]) for r in sw}
    assert last_place == {1, 2, 3, 4}, last_place
    near = [r for r in by("open") if abs(r[3]["n_expanded"] - cmax[0]) <= 12]
    assert any(r[4]["path_walk"] == "lds" for r in near) and any(r[4]["path_walk"] == "hbm" for r in near)
    assert max(r[3]["n_expanded"] for r in near if r[4]["path_walk"] == "lds") >= cmax[0] - 10

    # -- a path longer than the hop list
    z = {r[2].name: r for r in by("zigzag/1056") + by("zigzag/1024")}
    walks = {n_: (r[3]["hops"], r[4]["path_walk"], r[4]["K"]) for n_, r in z.items()}
    assert walks["zigzag/1056x32/200"][0] > open_cap + 64 and walks["zigzag/1056x32/200"][1:] == ("chunked", 2), walks
    assert open_cap < walks["zigzag/1056x32/171"][0] <= open_cap + 2 and walks["zigzag/1056x32/171"][1] == "chunked", walks
    assert open_cap - 2 <= walks["zigzag/1056x32/170"][0] <= open_cap and walks["zigzag/1056x32/170"][1] == "lds", walks
    split = {hops: walks[f"zigzag/1056x32/{n_}+"] for n_, _, hops in ss.ZIGZAG_SPLIT}
    assert split == {open_cap + 1: (open_cap + 1, "chunked", 2), open_cap: (open_cap, "lds", 2)}, split          # the split itself
    assert walks["zigzag/1024x32/130"][1:] == ("hbm", 1) and walks["zigzag/1024x32/127"][1] == "hbm", walks
    assert walks["zigzag/1024x32/126"][1] == "lds" and walks["zigzag/1024x32/120"][1:] == ("lds", 1), walks
    assert all(r[3]["peak_open"] <= 2 and r[3]["n_expanded"] + k["DMPP_JPS_BATCH"] <= cmax[2] for r in by("zigzag/1056"))

    # -- the open list: 256 | 257 slots read, 512 live entries without a retry, 513 with one, bucket_cap on the peak and below
    op = {r[2].name.split("/")[-1]: r for r in by("open")}
    peaks = {s: op[str(s)][3]["peak_open"] for s in (ss.PEAK_256, ss.PEAK_257, ss.PEAK_512, ss.PEAK_513)}
    assert list(peaks.values()) == [k["upper_at"], k["upper_at"] + 1, open_cap, open_cap + 1], peaks
    crafted_f = [r[4] for r in rows]
    assert any(not f["upper_keys"] and f["peak_slots"] > k["upper_at"] // 2 for f in crafted_f)
    assert any(f["upper_keys"] for f in crafted_f)
    assert not op[str(ss.PEAK_512)][4]["retry"] and op[str(ss.PEAK_512)][3]["status"] == gm.FOUND
    assert op[str(ss.PEAK_513)][4]["retry"] and op[str(ss.PEAK_513)][3]["status"] == gm.FOUND
    # ... a squeeze with every slot of LDS in use by dead and live entries, and no retry: dead slots alone never cause one
    assert any(f["squeezes"] and not f["retry"] and f["squeeze_live_max"] == open_cap for f in F("open"))
    assert any(s[1] == "pop" for f in F("open") for s in f["squeezes"]) and any(s[1] == "push" for f in F("open") for s in f["squeezes"])
    for cap, status, retry in ((513, gm.FOUND, True), (512, gm.OVERFLOW, False), (256, gm.FOUND, False), (255, gm.OVERFLOW, False)):
        r = by(f"bucket_cap/{cap}")[0]
        assert (r[3]["status"], r[4]["retry"]) == (status, retry), (cap, r[3]["status"], r[4]["retry"])

    # -- ties
    steps = [(r, st) for r in rows for st in r[3].get("steps", [])]
    ties = {st["n_ties"] for _, st in steps}
    assert {4, 5} <= ties and max(ties) >= 9, sorted(ties)
    assert any(r[4]["tie_registers"] >= 2 for r in rows)
    assert any(st["dropped_twice"] for _, st in steps) and any(st["dropped_closed"] for _, st in steps)
    goal_place = {len(r[3]["steps"][-1]["closed"]) for r in rows if r[3]["status"] == gm.FOUND and r[3]["steps"]}
    cut = [r for r in rows if r[3]["status"] == gm.FOUND and r[3]["steps"][-1]["n_ties"] > len(r[3]["steps"][-1]["taken"])]
    assert goal_place == {1, 2, 3, 4} and cut, goal_place          # ... and ties behind the goal that are not taken, not counted

    # -- forms of the launch
    r0 = rows[0]
    cfg0 = _model(dm, r0[2], r0[1])[1]
    wide = k["kScoreWideMaxScenes"]
    assert [ss.forms(r0[3], cfg0, n_, k)["setup_waves"] for n_ in (1, wide, wide + 1)] == [16, 16, 4]
    for g in (GROUPS[n_] for n_ in CRAFTED):
        sizes = {len(items) for _, items in _launches(g)}
        assert {1, wide, wide + 1} <= sizes, (g.name, sizes)
        for form, items in _launches(g):
            if form == "128":
                assert all(items[j] == items[wide - 1 - j] for j in range(wide))          # every case early and late in the batch


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _only_max_expansions(a, b):
    return {k_: v for k_, v in a.items() if k_ != "max_expansions"} == {k_: v for k_, v in b.items() if k_ != "max_expansions"}


def _n_obs(g):
    """Obstacle entries per scene in every launch of a group: the occupied cells of its fullest bitmap."""
    return max(1, max(int(np.count_nonzero(c.bitmap)) for c in g.cases))


def _oracle_tick(dm, oracle, g, over):
    """The oracle's whole tick over the cases of a group, one scene per case (every scene of a batch has the same base)."""
    def make():
        cfg = _model(dm, g.cases[0], over)[1]
        sc = ss.build(dm, cfg, [(c.bitmap, c.start, c.goal) for c in g.cases], _n_obs(g))
        st = sc["state"].copy()
        plan, gout, _ = oracle.plan_tick_batch(cfg, sc, st, n_threads=8)
        return plan, gout, st
    return _cached(("oracle", g.name, _okey(over)), make)


def _launches(g):
    """(form, [case index per item]) of a group: what runs in one launch each."""
    n = len(g.cases)
    idx = list(range(n))
    if not g.crafted:
        return [("whole", idx)]
    out = [("alone", [i]) for i in idx]
    for a in range(0, n, 64):                     # 128 items: the chunk's cases, repeated, then the same backwards: case i at item i and at 127 - i
        half = [idx[a + j % min(64, n - a)] for j in range(64)]
        out.append(("128", half + half[::-1]))
    for a in range(0, n, 129):
        out.append(("129", [idx[a + j % min(129, n - a)] for j in range(129)]))
    if n > 1:
        out.append(("whole", idx))
    out.append(("dense", idx))
    return out


def _run_group(dm, g):
    """Every launch of a group under every config of it: [(form, over, items, GridOut, PlanOut, SceneState, orders, paths, grids)]."""
    order_cap = 64 + max([_model(dm, c, o)[0].get("n_expanded", 4096) for o in g.overs for c in g.cases])
    runs = []
    pl, pl_key = None, None
    spent = {}                                    # seconds per (form, phase), printed for the record

    def lap(form, phase, t0):
        spent[(form, phase)] = spent.get((form, phase), 0.0) + time.perf_counter() - t0
        return time.perf_counter()
    old = os.environ.get("DMPP_SEARCH_GBM")
    try:
        for form, items in _launches(g):
            scenes = [(g.cases[i].bitmap, g.cases[i].start, g.cases[i].goal) for i in items]
            sc = None
            for over in g.overs:
                t0 = time.perf_counter()
                cfg = _model(dm, g.cases[0], over)[1]
                if sc is None:
                    sc = ss.build(dm, cfg, scenes, _n_obs(g))
                # a handle is reused for the next launch of the same kind; lone scenes only while the bitmap stays the same: the LDS
                # budget of a handle follows the need of earlier ticks downwards, and a fuller bitmap could then go dense unnoticed
                key = (form == "dense", len(items), id(scenes[0][0]) if form == "alone" else 0)
                if pl is not None and pl_key[0] == key and _only_max_expansions(pl_key[1], over):
                    pl.set_config(cfg)
                else:
                    if pl is not None:
                        pl.close()
                    if form == "dense":
                        os.environ["DMPP_SEARCH_GBM"] = "1"
                    else:
                        os.environ.pop("DMPP_SEARCH_GBM", None)
                    pl = dm.Planner(cfg, device=0, max_scenes=len(items), max_obs_total=len(items) * sc["n_obs"], order_cap=order_cap)
                    pl_key = (key, dict(over))
                t0 = lap(form, "handle", t0)
                pl.set_scenes(sc)
                pl.set_state(sc["state"])
                pl.tick(sync=True)
                t0 = lap(form, "tick", t0)
                gout, plan, state = pl.get_grid_out(), pl.get_plan(), pl.get_state()
                orders, paths = [], []
                for s in range(len(items)):
                    full = int(gout["status"][s]) not in STATUS_ONLY
                    n_o, n_p = min(int(gout["n_expanded"][s]), order_cap), int(gout["path_len"][s])
                    orders.append((pl.get_order(s, n_o) if n_o else np.zeros(0, np.int32)) if full else None)
                    paths.append((pl.get_path(s, n_p) if n_p else np.zeros(0, np.int32)) if full else None)
                grids = [pl.get_grid(s) for s in range(len(items))] if form in ("alone", "dense") or not g.crafted else None
                _, _, dense = pl.search_info()
                # the dense path really ran for every scene | every other launch searched the sparse line-mask views
                assert dense == (len(items) if form == "dense" else 0), (g.name, form, items[:4], dense, len(items))
                lap(form, "fetch", t0)
                runs.append((form, over, items, gout, plan, state, orders, paths, grids))
    finally:
        if pl is not None:
            pl.close()
        if old is None:
            os.environ.pop("DMPP_SEARCH_GBM", None)
        else:
            os.environ["DMPP_SEARCH_GBM"] = old
    print(f"{g.name}: seconds " + ", ".join(f"{f_}/{ph} {v:.2f}" for (f_, ph), v in spent.items()))
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ss.GROUP_NAMES)
def test_device_search_equals_model_and_oracle_in_every_form(dm, oracle, name):
    """One group of the case list through Planner: every launch of `_launches` under every config of the group.  Device against
    the model (status, counters, order, digest, path), against the oracle (whole tick), `get_grid` against the bitmap, and a
    case's records the same bytes wherever it ran."""
    g = GROUPS[name]
    k = ss.kernel_constants()
    bad, seen = [], {}
    for form, over, items, gout, plan, state, orders, paths, grids in _run_group(dm, g):
        plan_o, gout_o, state_o = _oracle_tick(dm, oracle, g, over)
        for s, ci in enumerate(items):
            c = g.cases[ci]
            m, cfg = _model(dm, c, over)
            tag = f"{form}[{s}] {c.name}{over or ''}"
            rec = gout[s]
            assert int(rec["status"]) != gm.INTERNAL, tag
            bad += _against_model(int(rec["status"]), rec, None if orders[s] is None else orders[s].tolist(),
                                  None if paths[s] is None else paths[s].tolist(), m, tag)
            if (int(rec["start_cell"]), int(rec["goal_cell"])) != (_cell(c, c.start), _cell(c, c.goal)):
                bad.append(f"{tag}: start / goal cell {int(rec['start_cell'])} / {int(rec['goal_cell'])}")
            bad += compare(plan[s:s + 1], plan_o[ci:ci + 1], tag + " plan") + compare(state[s:s + 1], state_o[ci:ci + 1], tag + " state")
            if m["status"] in STATUS_ONLY:
                bad += compare(gout["status"][s:s + 1], gout_o["status"][ci:ci + 1], tag + " grid.status")
            else:
                bad += compare(gout[s:s + 1], gout_o[ci:ci + 1], tag + " grid")
            if grids is not None and not np.array_equal(grids[s], c.bitmap):
                bad.append(f"{tag}: get_grid differs from the bitmap in {int((grids[s] != c.bitmap).sum())} cells")
            if m["status"] not in STATUS_ONLY:          # the same bytes in every form of the launch
                blob = (rec.tobytes(), orders[s].tobytes(), paths[s].tobytes(), plan[s].tobytes())
                first = seen.setdefault((ci, _okey(over)), (tag, blob, gout[s:s + 1].copy(), plan[s:s + 1].copy()))
                if first[1] != blob:
                    diff = compare(gout[s:s + 1], first[2], "grid", rtol=0.0, atol=0.0) + compare(plan[s:s + 1], first[3], "plan", rtol=0.0, atol=0.0)
                    which = [w for w, a_, b_ in (("order", blob[1], first[1][1]), ("path", blob[2], first[1][2])) if a_ != b_]
                    bad.append(f"{tag}: records differ from those of {first[0]}: " + "; ".join(diff + which))
            if form in ("alone", "129", "dense") or not g.crafted:          # the form taken, once per case and kind of launch, for the record
                key = ("line", ci, _okey(over), form)
                if key not in seen and (g.name != "seam" or ci % 24 == 0):
                    seen[key] = True
                    f = ss.forms(m, cfg, len(items), k)
                    print(f"{form:5s} waves {f['setup_waves']:2d} dense {int(form == 'dense')} " + _form_line(g, over, c, m, f))
    assert not bad, "\n".join(bad[:20])
