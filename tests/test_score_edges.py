"""The scoring pass (G3; `score_body` of csrc/kernels_score.hpp, run as k_score<16> / k_score<4>) on crafted scenes
that sit ON its case splits, against a 40-digit model written from the specification (tests/grid_score_model.py).

The crafted scenes and the form the kernel takes for each are tests/score_scenes.py.  CPU tests: the oracle against the
model, the coverage of the case list, the distance of every case from the specification's two discontinuities, the tie's
known answer.  GPU tests: the device against the model and against the oracle - every case alone, in a batch of
kScoreWideMaxScenes scenes (sixteen waves per scene) and in a batch of one more (four waves) -, the whole GridOut record byte
for byte the same in the three settings (the tree sums stay bit-exact under the quarter split and the packed
pass), and n_lattice 16 .. 0 and the lookahead_cells list stepped with set_config on one handle per width.

Ticks are synchronous and the batches stay below the 256 scenes from which ticks are piped into groups (`pipeline_min` of
dmpp_hip.hip), so every tick is one launch of its own and its work items are the scenes: `items <= kScoreWideMaxScenes`
in flush_group is then a statement about the scene count.

Bars: integers (n_candidates, best_candidate) and cand_prog exact, floats within parity_util.RTOL / ATOL.  Measured (CPU
oracle; the device figures are in profiles/r16_score_kat.txt): oracle against model 1.4e-10 relative at worst."""
import numpy as np
import pytest

import grid_score_model as gm
import score_scenes as ss
from parity_util import ATOL, RTOL, bit_identical_fraction, compare

LOOKAHEADS = [0, 2, 3, 4, 5, 120, 199, 400]
LATTICES = list(range(16, -1, -1))
FLOATS = ("cand_col", "cand_curv", "cand_cost")
# A case must stay this far from the specification's discontinuities (ten times the hand-over band of the kernel's fence;
# a micrometre of clearance is ~1e7 times the rounding error of a distance of tens of metres)
MIN_ABS_CLEARANCE = 1e-6
MIN_FENCE = 1e-5
# ... and its winner must be the winner in every arithmetic: oracle, kernel and model differ by rounding only, and the largest
# such difference is the kernel's curvature from squared lengths, ~1e-9 relative; the winner has to lead by a
# hundred times that on the two costs involved (the tie is the one case with margin 0: its winner is the rule "lowest index")
MARGIN_REL = 100 * 1e-9

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _cfg(dm, n_lattice=16, lookahead=120):
    cfg = ss.config(dm)
    cfg["n_lattice"], cfg["lookahead_cells"] = n_lattice, lookahead
    return cfg


def _reference(dm, oracle, names, n_obs, n_lattice=16, lookahead=120):
    """Oracle GridOut + path, model and form of one scene per name (computed once per process, never modified)."""
    def make():
        cfg = _cfg(dm, n_lattice, lookahead)
        sc = ss.build(dm, cfg, list(names), n_obs)
        k = ss.kernel_constants()
        out = []
        for s, name in enumerate(names):
            _, go, _, _, path = oracle.plan_tick_one(cfg, sc, s, sc["state"].copy())
            obs = ss.scene_obstacles(sc, s)
            status = int(go["status"])
            out.append(dict(name=name, gout=go.copy(), path=path.copy(), model=gm.score_scene(cfg, sc["scene_in"][s], obs, path, status),
                            form=ss.forms(cfg, sc["scene_in"][s], obs, path, status, k)))
        return out
    return _cached(("ref", tuple(names), n_obs, n_lattice, lookahead), make)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    return float(np.max(d / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300), initial=0.0))


def _against_model(go, m, tag):
    """Mismatches of one GridOut record against the model's result, and the largest relative difference of its floats."""
    bad, worst = [], 0.0
    nc = m["n_candidates"]
    for f in ("n_candidates", "best_candidate"):
        if int(go[f]) != m[f]:
            bad.append(f"{tag}.{f}: {int(go[f])} vs model {m[f]}")
    if not np.array_equal(go["cand_prog"], m["cand_prog"]):
        bad.append(f"{tag}.cand_prog: {go['cand_prog'].tolist()} vs model {m['cand_prog'].tolist()}")
    pairs = [(f, go[f], m[f]) for f in FLOATS]
    pairs.append(("best_path", np.stack([go["best_path"]["x"], go["best_path"]["y"]], -1), m["best_path"]))
    for f, a, b in pairs:
        ok = np.abs(a - b) <= ATOL + RTOL * np.maximum(np.abs(a), np.abs(b))
        if not ok.all():
            i = tuple(np.argwhere(~ok)[0])
            bad.append(f"{tag}.{f}: {int((~ok).sum())} beyond the bar, first at {i}: {a[i]!r} vs model {b[i]!r}")
        worst = max(worst, _rel(a[:nc] if f != "best_path" else a, b[:nc] if f != "best_path" else b))
    for f in FLOATS + ("cand_prog",):                      # entries beyond the candidates read zero
        if np.any(go[f][nc:] != 0):
            bad.append(f"{tag}.{f}: stale entries beyond candidate {nc}: {go[f][nc:].tolist()}")
    return bad, worst


def _tree_sum(v):
    """The 64-leaf tree of DESIGN §5 G3 in float64: leaf l = v[l] + v[l+64] + v[l+128] + v[l+192], folds 32 .. 1."""
    part = np.zeros(64)
    for l in range(64):
        acc = 0.0
        for q in range(4):
            if l + 64 * q < len(v):
                acc += v[l + 64 * q]
        part[l] = acc
    s = 32
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return float(part[0])


def _all_references(dm, oracle):
    """Every (tag, reference) the tests use: the two case batches, the edge case, and the two sweeps on the base scene."""
    refs = []
    for n_obs in ss.BATCH_N_OBS:
        refs += [(f"{r['name']}/{n_obs}", r) for r in _reference(dm, oracle, ss.CASE_NAMES, n_obs)]
    refs += [(f"{r['name']}/{ss.EDGE_CASE[1]}", r) for r in _reference(dm, oracle, [ss.EDGE_CASE[0]], ss.EDGE_CASE[1])]
    for nl in LATTICES:
        refs += [(f"{r['name']}/n_lattice {nl}", r) for r in _reference(dm, oracle, [ss.BASE, "blocked_goal"], 256, n_lattice=nl)]
    for la in LOOKAHEADS:
        refs += [(f"{r['name']}/lookahead {la}", r) for r in _reference(dm, oracle, [ss.BASE, "blocked_goal"], 256, lookahead=la)]
    return refs


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_oracle_scores_equal_the_model(dm, oracle):
    """The oracle's G3 against the 40-digit model on every case, on n_lattice 0 .. 16 and on the lookahead_cells list."""
    print("model arithmetic:", gm.ARITHMETIC)
    bad, worst = [], 0.0
    for tag, r in _all_references(dm, oracle):
        b, w = _against_model(r["gout"], r["model"], tag)
        bad += b
        worst = max(worst, w)
    print(f"oracle against model, largest relative difference: {worst:.3g}")
    assert not bad, "\n".join(bad[:20])


def test_cases_keep_away_from_the_discontinuities_and_have_a_clear_winner(dm, oracle):
    """clearance <= 0 and sinA < 0.001 are jumps of the specification: no point of any case comes near either (no point is
    excluded, nothing is capped), and - but for the tie - the winner leads by far more than rounding moves a cost (MARGIN_REL)."""
    bad = []
    for tag, r in _all_references(dm, oracle):
        m = r["model"]
        print(f"{tag:28s} clearance {m['min_abs_clearance']:.3g} m  fence {m['min_fence']:.3g}  margin {m['margin']:.3g}")
        if m["min_abs_clearance"] < MIN_ABS_CLEARANCE:
            bad.append(f"{tag}: a point with |clearance| = {m['min_abs_clearance']:.3g} m")
        if m["min_fence"] < MIN_FENCE:
            bad.append(f"{tag}: a point {m['min_fence']:.3g} (relative) from the fence sinA = 0.001")
        if m["n_candidates"] > 1:
            need = ATOL + MARGIN_REL * (2 * abs(float(m["cand_cost"][m["best_candidate"]])) + m["margin"])
            if not tag.startswith("tie/") and m["margin"] < need:
                bad.append(f"{tag}: the winner leads by {m['margin']:.3g}, less than {need:.3g}")
    assert not bad, "\n".join(bad)


def test_case_list_covers_every_form_and_both_sides_of_every_threshold(dm, oracle):
    """The forms of score_body, from the rule in its header comment with the constants read from the sources: the case list
    must put a scene on either side of every threshold.  A changed constant fails here."""
    k = ss.kernel_constants()
    rows = []
    for n_obs in ss.BATCH_N_OBS:
        rows += [(n_obs, r) for r in _reference(dm, oracle, ss.CASE_NAMES, n_obs)]
    rows += [(ss.EDGE_CASE[1], r) for r in _reference(dm, oracle, [ss.EDGE_CASE[0]], ss.EDGE_CASE[1])]
    print("case            n_obs status path_len  nc   a n_rel culled form             fullest first_near")
    for n_obs, r in rows:
        f, go = r["form"], r["gout"]
        print(f"{r['name']:15s} {n_obs:5d} {int(go['status']):6d} {int(go['path_len']):8d} {f['nc']:3d} {f['a']:3d} {f['n_rel']:5d} "
              f"{int(f['culled']):6d} {f['form']:16s} {f['fullest']:7d} {f['first_near']:10d}")
    F = [r["form"] for _, r in rows]
    assert {f["form"] for f in F} == {"lds_plain", "lds_buckets", "snapshot_buckets", "hbm_plain"}
    n_rels = {f["n_rel"] for f in F}
    assert {0, k["kBucketMinObs"] - 1, k["kBucketMinObs"], k["kMaxRelObs"], k["kMaxRelObs"] + 1} <= n_rels, n_rels
    fullest = {f["fullest"] for f in F if f["bucketed"]}
    assert {k["kBucketCap"], k["kBucketCap"] + 1} <= fullest, fullest
    assert any(f["overflow"] for f in F) and any(f["bucketed"] and not f["overflow"] for f in F)
    not_culled = {f["m"] for f in F if not f["culled"]}
    assert {k["snapshot_bucket_max"], k["snapshot_bucket_max"] + 1} <= not_culled and max(not_culled) >= 300, not_culled
    # a scene bucketed from the snapshot keeps its near obstacles at the END of its list: an index cut to less than 8 bits shows
    assert all(f["first_near"] >= 127 for f in F if f["form"] == "snapshot_buckets")
    # ... and some of the buckets its candidates read are within the capacity, so the 8-bit entries are used: under the line of discs
    lb = [f for f in F if f["form"] == "snapshot_buckets" and f["n_rel"] == k["kMaxRelObs"] + 1 and f["fullest"] > k["kBucketCap"]]
    assert any(all(1 <= f["fill_at"](x, 18.0) <= k["kBucketCap"] for x in (8.0, 12.0, 16.0, 20.0, 24.0)) for f in lb)
    # found / blocked / one-cell path
    by_name = {r["name"]: r for n_obs, r in rows if n_obs == 256}
    for name, r in by_name.items():
        go = r["gout"]
        if name == "blocked_goal":
            assert int(go["status"]) == 4 and r["form"]["nc"] == 16 and not r["form"]["have_path"]
        elif name == "goal_is_ego":
            assert int(go["status"]) == 0 and int(go["path_len"]) == 1 and r["form"]["a"] == 0
        else:
            assert int(go["status"]) == 0 and int(go["path_len"]) == 105, (name, int(go["status"]), int(go["path_len"]))
    # the path prefix: the ego's heading (a = 0), the shortened baseline (a < 4), the full one, the whole path
    a_seen = {_reference(dm, oracle, [ss.BASE, "blocked_goal"], 256, lookahead=la)[0]["form"]["a"] for la in LOOKAHEADS}
    assert a_seen == {0, 2, 3, 4, 5, 104}, a_seen
    # the detour's north pebble is inside the cull box only through the box of the path's cells, and the path candidate wins
    d = by_name["detour"]
    thr = 0.1 + 0.5 * 1.8 + 1.0
    assert d["form"]["hull"][3] + thr < 22.2 <= d["form"]["box"][3] + thr and d["form"]["n_rel"] == 2
    assert d["model"]["best_candidate"] == 16
    # ... and in detour_west the pebble decides the path candidate's penalty: without it the model's cand_col moves by far more than the bar
    dw = by_name["detour_west"]
    assert dw["form"]["hull"][3] + thr < 22.2 <= dw["form"]["box"][3] + thr and dw["form"]["n_rel"] == 2 and dw["model"]["best_candidate"] == 16
    cfg = _cfg(dm)
    sc = ss.build(dm, cfg, ["detour_west"], 256)
    obs = ss.scene_obstacles(sc, 0).copy()
    assert obs["y"][254] == sc["scene_in"]["grid_origin"]["y"][0] + 22.2
    obs["y"][254] += 100.0
    without = gm.score_scene(cfg, sc["scene_in"][0], obs, dw["path"], 0)
    assert dw["model"]["cand_col"][16] - without["cand_col"][16] > 1e-3 * dw["model"]["cand_col"][16]
    # the tail's first hits lie in the fourth pass (points 192 .. 199) alone
    prog = by_name["tail"]["model"]["cand_prog"]
    assert np.any(prog > 0) and np.all(prog[prog > 0] <= 8 / 200), prog
    # every way of dealing nc candidates to NW waves: found scenes give nc = n_lattice + 1, blocked ones nc = n_lattice
    seen = set()
    for nl in LATTICES:
        seen |= {r["form"]["nc"] for r in _reference(dm, oracle, [ss.BASE, "blocked_goal"], 256, n_lattice=nl)}
    assert seen == set(range(18)), seen
    kinds = {(nw, s["rounds"] > 0, s["split"] > 0, s["packed"]) for nw in (4, 16) for nc in seen for s in [ss.schedule(nw, nc)]}
    assert {(4, True, True, True), (4, True, False, True), (4, True, False, False), (4, True, True, False), (4, False, True, False),
            (16, False, True, False), (16, True, True, False), (16, True, False, False), (16, False, False, False)} <= kinds, kinds


def test_tie_goes_to_the_lowest_index(dm, oracle):
    """Heading 0 with the line of nine: candidates 7 (the straight Bezier) and 16 (the straight grid path) are both fenced at
    every interior point and touch nothing, so both cost w_curv * (tree sum of 198 x 1e-6) exactly; 7 is published."""
    r = {x["name"]: x for x in _reference(dm, oracle, ss.CASE_NAMES, 256)}["tie"]
    _assert_tie(r["gout"])
    m = r["model"]
    assert m["best_candidate"] == 7 and m["margin"] == 0.0
    assert abs(m["cand_curv"][7] - 198e-6) < 1e-18 and m["cand_curv"][7] == m["cand_curv"][16]


def _assert_tie(go):
    k2 = (1.0 / 1000.0) * (1.0 / 1000.0)
    want = _tree_sum(np.array([0.0] + [k2] * 198 + [0.0]))
    assert int(go["best_candidate"]) == 7 and int(go["n_candidates"]) == 17
    for k in (7, 16):
        assert go["cand_curv"][k] == want and go["cand_col"][k] == 0.0 and go["cand_prog"][k] == 0.0 and go["cand_cost"][k] == want, \
            (k, go["cand_curv"][k], want)
    assert np.all(np.delete(go["cand_cost"], [7, 16]) > want)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _widths():
    k = ss.kernel_constants()["kScoreWideMaxScenes"]
    return {"wide": k, "narrow": k + 1}      # scenes of a batch: sixteen waves per scene up to k, four beyond


def _fill(names, n):
    return [names[i % len(names)] for i in range(n)]


def _tick(dm, cfg, sc, pl=None):
    n = len(sc["scene_in"])
    own = pl is None
    if own:
        pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * sc["n_obs"])
    pl.set_scenes(sc)
    pl.set_state(sc["state"])
    pl.tick(sync=True)
    go = pl.get_grid_out()
    if own:
        pl.close()
    return go


def _device_runs(dm, n_obs):
    """GridOut of every case in the three settings (once per process): alone, in the wide batch, in the narrow batch."""
    def make():
        cfg = _cfg(dm)
        runs = {}
        pl = dm.Planner(cfg, device=0, max_scenes=1, max_obs_total=n_obs)
        runs["alone"] = np.concatenate([_tick(dm, cfg, ss.build(dm, cfg, [name], n_obs), pl) for name in ss.CASE_NAMES])
        pl.close()
        for w, n in _widths().items():
            runs[w] = _tick(dm, cfg, ss.build(dm, cfg, _fill(ss.CASE_NAMES, n), n_obs))
        return runs
    return _cached(("dev", n_obs), make)


def _check(gouts, refs, tag):
    """Device records against the oracle's (parity_util.compare) and the model's, reference i % len(refs) for record i."""
    bad, worst = [], 0.0
    for i in range(len(gouts)):
        r = refs[i % len(refs)]
        t = f"{tag}[{i}] {r['name']}"
        bad += compare(gouts[i:i + 1], r["gout"].reshape(1), t)
        b, w = _against_model(gouts[i], r["model"], t)
        bad += b
        worst = max(worst, w)
    ref = np.concatenate([refs[i % len(refs)]["gout"].reshape(1) for i in range(len(gouts))])
    print(f"{tag}: {len(gouts)} records, device against model {worst:.3g} relative at worst, "
          f"bytes equal to the oracle's {bit_identical_fraction(gouts, ref):.6f}")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("n_obs", ss.BATCH_N_OBS)
@pytest.mark.parametrize("setting", ["alone", "wide", "narrow"])
def test_device_scores_equal_model_and_oracle(dm, oracle, n_obs, setting):
    """Every case alone (k_score<16>, one work item), in a batch of kScoreWideMaxScenes (k_score<16>) and of one more
    (k_score<4>): GridOut against the oracle and cand_* / winner / best_path against the model."""
    refs = _reference(dm, oracle, ss.CASE_NAMES, n_obs)
    bad = _check(_device_runs(dm, n_obs)[setting], refs, f"{setting}/{n_obs}")
    assert not bad, "\n".join(bad[:20])
    if n_obs == 256:
        _assert_tie(_device_runs(dm, n_obs)[setting][ss.CASE_NAMES.index("tie")])


@pytest.mark.gpu
def test_device_first_obstacle_count_beyond_the_snapshot_buckets(dm, oracle):
    """129 near obstacles of 257: not culled and one obstacle too many for 8-bit bucket entries - the plain loop over HBM."""
    name, n_obs = ss.EDGE_CASE
    refs = _reference(dm, oracle, [name], n_obs)
    assert refs[0]["form"]["form"] == "hbm_plain"
    cfg = _cfg(dm)
    bad = _check(_tick(dm, cfg, ss.build(dm, cfg, [name], n_obs)), refs, f"alone/{n_obs}")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("n_obs", ss.BATCH_N_OBS)
def test_device_record_is_the_same_bytes_alone_and_in_either_batch(dm, n_obs):
    """the quarter split and the packed fourth pass add the terms in the order one wave would have added them.  So
    the whole GridOut record of a scene does not depend on the schedule: alone, sixteen waves in a batch, four waves."""
    runs = _device_runs(dm, n_obs)
    bad = []
    for w in ("wide", "narrow"):
        for i in range(len(runs[w])):
            c = i % len(ss.CASE_NAMES)
            if runs[w][i].tobytes() != runs["alone"][c].tobytes():
                bad.append(f"{ss.CASE_NAMES[c]}: record {i} of the {w} batch differs from the scene alone: " +
                           "; ".join(compare(runs[w][i:i + 1], runs["alone"][c:c + 1], "", rtol=0.0, atol=0.0)))
    assert not bad, "\n".join(bad[:20])


def _sweep(dm, oracle, width, field, values):
    """One handle, the config stepped with set_config, one synchronous tick per value over found and blocked-goal scenes."""
    names = [ss.BASE, "blocked_goal"]
    n = _widths()[width]
    cfg = _cfg(dm)
    sc = ss.build(dm, cfg, _fill(names, n), 256)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * 256)
    pl.set_scenes(sc)
    pl.set_state(sc["state"])
    bad = []
    for v in values:
        cfg[field] = v
        pl.set_config(cfg)
        pl.tick(sync=True)
        refs = _reference(dm, oracle, names, 256, **{"n_lattice" if field == "n_lattice" else "lookahead": v})
        bad += _check(pl.get_grid_out(), refs, f"{width}/{field} {v}")
    pl.close()
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("width", ["wide", "narrow"])
def test_device_every_candidate_count_on_one_handle(dm, oracle, width):
    """n_lattice 16 -> 0 on one handle, found scenes (nc = n_lattice + 1) beside blocked-goal scenes (nc = n_lattice): every
    nc of 0 .. 17 on this width - whole rounds, quarter splits, the packed pass - and the entries a smaller nc leaves
    behind read zero."""
    bad = _sweep(dm, oracle, width, "n_lattice", LATTICES)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("width", ["wide", "narrow"])
def test_device_every_path_prefix_on_one_handle(dm, oracle, width):
    """lookahead_cells 0 (the ego's heading), 2 and 3 (shortened baseline), 4, 5, and three values beyond the path's end."""
    bad = _sweep(dm, oracle, width, "lookahead_cells", LOOKAHEADS)
    assert not bad, "\n".join(bad[:20])
