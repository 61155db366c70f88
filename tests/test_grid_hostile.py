"""The grid engine (G1 rasteriser, G2 start / goal cell and search, G3 scoring) on obstacles, ego, goal and grid origin
that are not finite or lie far outside the range of int - the rule is DESIGN §5 "Values outside the grid's range", the scenes
are tests/hostile_scenes.py.

CPU: the conditions on the case list (box rasteriser == brute force == the numpy statement of the predicate; what every hostile
value class does to the grid by the rule; every status one whose record is fully specified; oracle search == the Python model),
the oracle's scores against the 40-digit model on every obstacle case of the list (every tick, every twin) and on a sweep of
single hostile entries through each obstacle path of the scoring kernel, and the oracle's C under -fsanitize=undefined,float-cast-overflow in a
stand-alone program (tests/native/grid_hostile.c) on every case.

GPU: every case on one handle per grid shape - `get_grid` cell for cell, one tick against the model's status, counters, digest,
expansion order and path, its whole GridOut record (cand_*, best_*) against the oracle's and the 40-digit model's unless the ego,
goal or origin is hostile (`_scored`), then the case's ordinary twin on the same handle; the dense forms; one launch of 64 scenes that
interleaves hostile cases with ordinary twins; and the scoring pass on each of its obstacle paths with one hostile entry in the
list, alone and in the 16-wave and 4-wave batches.

Bars: integers and grids exact; scores within parity_util.RTOL / ATOL (a NaN equals a NaN).

What fails without each part of the change: the index rule in the oracle - test_oracle_c_has_no_undefined_behaviour_on_any_case
(against the earlier sources the program stops at the first NaN obstacle: "nan is outside the range of representable values of
type 'int'" in orc_rasterise); the `R >= 0` term - test_case_list_conditions on the oracle (r=-1 becomes a disc of 0.9 m) and
test_device_every_case_then_its_ordinary_twin on the device (r=neg_tiny sits on a cell centre, where 0 <= R*R holds); the clamp
in double in `footprint_of` - the far_right / far_left / far_below cases of the device tests (the saturated conversion + 1 wraps
and the box of a disc that reaches in becomes empty); a NaN upper bound as the widest one - the x=-inf,r=+inf and y=-inf,r=+inf
cases (the box would be empty where the predicate holds everywhere).  The scoring pass needed no change: DESIGN §5 shows that an obstacle with a
negative cutoff cannot change a penalty, and every other hostile value is treated alike by the cull, the buckets and the plain
loop - test_device_scores_with_a_hostile_obstacle holds all three to the plain loop's record."""
import os
import struct
import subprocess

import numpy as np
import pytest

import grid_score_model as gm
import grid_search_model as gsm
import hostile_scenes as hs
import score_scenes as scs
from parity_util import ATOL, RTOL, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIFIED = (gsm.FOUND, gsm.NO_PATH, gsm.GOAL_BLOCKED, gsm.LIMIT)
SEARCH_FIELDS = ("status", "n_expanded", "n_pushed", "n_rounds", "path_cost", "path_len", "order_digest")
# value classes whose entries occupy nothing BY THE RULE: a NaN compares false; d2 = +inf or >= (1e12 - 32)^2 exceeds the
# R*R of an ordinary radius; R < 0
NOTHING_BY_RULE = ("x=nan", "y=nan", "r=nan", "x=+inf", "x=-inf", "y=+inf", "y=-inf", "x=+1e300", "x=-1e300", "y=+1e300", "y=-1e300",
                   "x=+1e12", "x=-1e12", "y=+1e12", "y=-1e12", "x=q+2147483647", "x=q+2147483648", "x=q-2147483649", "y=q+2147483647",
                   "y=q+2147483648", "y=q-2147483649", "r=-inf", "r=-1", "r=neg_tiny", "r=-3", "x=nan,r=+inf")

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _cases():
    return _cached("cases", hs.cases)


def _cfg(dm, c):
    return hs.config(dm, c.W, c.H, dynamic=1 if c.mot else 0)


def _scored(c):
    """The scores (cand_*, best_*) are checked on the obstacle cases: every case but those with a hostile ego, goal or grid origin
    (not specified when these are not finite - the Bezier control points, or the centres of the path's cells, are not
    finite then - and at 1e300 the squares overflow)."""
    return c.ego == c.twin_ego and c.goal == c.twin_goal and c.origin == c.twin_origin


def _model_search(cfg, grid, start, goal):
    key = ("search", grid.shape, grid.tobytes(), start, goal, int(cfg["max_expansions"][0]), int(cfg["bucket_cap"][0]), int(cfg["max_path"][0]))
    return _cached(key, lambda: gsm.search(grid.reshape(-1), grid.shape[1], grid.shape[0], start, goal, int(cfg["max_expansions"][0]),
                                           int(cfg["bucket_cap"][0]), int(cfg["max_path"][0]), trace=False))


def _reference(dm, oracle, c):
    """Per tick of the case: the effective obstacles, the grid by the predicate, start and goal cell and the model's search."""
    def make():
        cfg = _cfg(dm, c)
        sc = hs.build(dm, cfg, [c])
        obs, mot = hs.scene_obstacles(sc, 0), sc["mot_pool"][:len(c.obs)]
        state = sc["state"].copy()
        out = []
        for t in range(c.ticks):
            eff = oracle.effective_obstacles(cfg, obs, mot, t) if c.mot else obs.copy()
            grid = gsm.occupancy(c.W, c.H, hs.CELL, hs.INFLATE, c.origin, eff)
            start = gsm.cell_of(c.W, c.H, hs.CELL, c.origin, c.ego[0], c.ego[1])
            goal = gsm.cell_of(c.W, c.H, hs.CELL, c.origin, c.goal[0], c.goal[1])
            _, go, _, _, path = oracle.plan_tick_one(cfg, sc, 0, state)           # (advances `state`: tick t of the case)
            score = None
            if _scored(c):
                with np.errstate(all="ignore"):
                    score = gm.score_scene(cfg, sc["scene_in"][0], eff, path, int(go["status"]))
            out.append(dict(eff=eff, grid=grid, start=start, goal=goal, model=_model_search(cfg, grid, start, goal), gout=go.copy(),
                            path=path.copy(), score=score))
        return out
    return _cached(("ref", c.name), make)


def _search_mismatches(go, order, path, m, tag):
    bad = []
    for f in SEARCH_FIELDS:
        if int(go[f]) != int(m[f]):
            bad.append(f"{tag}.{f}: {int(go[f])} vs model {int(m[f])}")
    if order is not None and list(map(int, order)) != list(m["order"]):
        bad.append(f"{tag}: expansion order differs from the model's")
    if path is not None and list(map(int, path)) != list(m["path"]):
        bad.append(f"{tag}: path differs from the model's")
    return bad


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_case_list_conditions(dm, oracle):
    """Rasterise (box form) == brute force == the predicate in numpy on every case; what each value class does to the grid; the
    statuses; oracle search == model; the cell of a hostile ego / goal."""
    bad, seen_effect = [], {}
    for c in _cases():
        cfg = _cfg(dm, c)
        for t, r in enumerate(_reference(dm, oracle, c)):
            tag = f"{c.name}@{t}"
            brute = oracle.rasterise(cfg, c.origin, r["eff"], brute=True)
            box = oracle.rasterise(cfg, c.origin, r["eff"])
            if not np.array_equal(box, brute):
                bad.append(f"{tag}: orc_rasterise differs from brute force in {int((box != brute).sum())} cells")
            if not np.array_equal(r["grid"], brute):
                bad.append(f"{tag}: the predicate in numpy differs from brute force in {int((r['grid'] != brute).sum())} cells")
            keep = [j for j in range(len(r["eff"])) if j not in c.hostile]
            plain = gsm.occupancy(c.W, c.H, hs.CELL, hs.INFLATE, c.origin, r["eff"][keep])
            alone = gsm.occupancy(c.W, c.H, hs.CELL, hs.INFLATE, c.origin, r["eff"][c.hostile])
            moved = c.mot is not None and t == 0 and c.klass == "vx=1e308"       # (an ordinary disc at tick 0: 1e308 * 0 = 0)
            if c.expect == "nothing" and not moved and not np.array_equal(brute, plain):
                bad.append(f"{tag}: the hostile entries occupy {int((brute != plain).sum())} cells, the rule says none")
            if c.expect == "differs" and (np.array_equal(brute, plain) or brute.all()):
                bad.append(f"{tag}: the grid should differ from the ordinary discs' and not be full")
            if c.expect == "all" and not brute.all():
                bad.append(f"{tag}: {int((brute == 0).sum())} cells are free, the rule says none")
            if c.expect == "empty" and brute.any():
                bad.append(f"{tag}: {int(brute.sum())} cells occupied under a non-finite origin")
            if c.family == "far" and not 1 <= int(alone.sum()) <= c.W * c.H - 1:
                bad.append(f"{tag}: the far disc alone occupies {int(alone.sum())} cells")
            if c.family in ("xy", "radius", "far") and not np.array_equal(brute, plain):
                seen_effect[c.klass] = True
            # start and goal
            for who, p, cell in (("ego", c.ego, r["start"]), ("goal", c.goal, r["goal"])):
                if oracle.cell_of(cfg, c.origin, p[0], p[1]) != cell:
                    bad.append(f"{tag}: orc_cell_of({who}) = {oracle.cell_of(cfg, c.origin, p[0], p[1])}, the rule says {cell}")
            m = r["model"]
            if m["status"] not in SPECIFIED:
                bad.append(f"{tag}: model status {gsm.STATUS_NAMES[m['status']]} - only the status would be specified")
                continue
            go, order, path = oracle.grid_search(cfg, brute, r["start"], r["goal"], order_cap=c.W * c.H)
            bad += _search_mismatches(go[0], order, path, m, tag)
    classes = {c.klass for c in _cases() if c.family in ("xy", "radius", "far")}
    for k in sorted(classes):
        if not seen_effect.get(k) and k not in NOTHING_BY_RULE:
            bad.append(f"class {k}: no case whose grid differs from the ordinary discs', and the rule does not say it occupies nothing")
        if seen_effect.get(k) and k in NOTHING_BY_RULE:
            bad.append(f"class {k}: occupies cells although the rule says nothing")
    assert {"r=+inf", "r=flt_max", "r=1e10", "r=0", "r=-0", "far_right", "far_left", "far_below"} <= {k for k in classes if seen_effect.get(k)}
    by = {c.name: c for c in _cases()}
    for oi in range(len(hs.ORIGINS)):
        assert _reference(dm, oracle, by[f"o{oi}/r=+inf/middle"])[0]["grid"].all()
        # -0.0 is 0: the same grid, and one cell more than the ordinary discs (the cell the entry sits on)
        g0, gm0 = _reference(dm, oracle, by[f"o{oi}/r=0/first"])[0]["grid"], _reference(dm, oracle, by[f"o{oi}/r=-0/first"])[0]["grid"]
        plain = _reference(dm, oracle, by[f"o{oi}/ordinary"])[0]["grid"]
        assert np.array_equal(g0, gm0) and int(g0.sum()) == int(plain.sum()) + 1
        # an ego at +inf searches from the last column, one at NaN from column 0; the same for the goal
        assert _reference(dm, oracle, by[f"o{oi}/ego.x=+inf"])[0]["start"] % hs.W == hs.W - 1
        assert _reference(dm, oracle, by[f"o{oi}/ego.x=nan"])[0]["start"] % hs.W == 0
        assert _reference(dm, oracle, by[f"o{oi}/goal.y=-inf"])[0]["goal"] // hs.W == 0
        assert _reference(dm, oracle, by[f"o{oi}/goal.y=q+2147483648"])[0]["goal"] // hs.W == hs.H - 1
    # the chunk case: a whole staging chunk and one more of entries, none of which has a cell
    ch = by["o0/chunk"]
    assert len(ch.hostile) == hs.raster_chunk() + 1 and ch.hostile[-1] == len(ch.obs) - 4
    statuses = {_reference(dm, oracle, c)[0]["model"]["status"] for c in _cases()}
    assert {gsm.FOUND, gsm.GOAL_BLOCKED} <= statuses, statuses
    assert not bad, "\n".join(bad[:30])


SCORE_BASES = [("n_rel_7", 256), ("n_rel_8", 256), ("n_rel_129", 256), ("n_rel_129", 300)]
SCORE_FORMS = ["lds_plain", "lds_buckets", "snapshot_buckets", "hbm_plain"]
# (name, x, y, radius): the hostile entry that replaces padding disc 0 of a score scene; x, y in metres from the grid origin
SCORE_HOSTILE = [("x=nan", hs.NAN, 18.0, 0.5), ("y=nan", 16.0, hs.NAN, 0.5), ("x=+inf", hs.INF, 18.0, 0.5), ("y=-inf", 16.0, -hs.INF, 0.5),
                 ("x=1e300", 1e300, 18.0, 0.5), ("x=-1e12", -1e12, 18.0, 0.5), ("r=nan", 16.0, 18.0, hs.NAN), ("r=+inf", 16.0, 18.0, hs.INF),
                 ("r=-inf", 16.0, 18.0, -hs.INF), ("r=flt_max", 16.0, 18.0, float(np.finfo(np.float32).max)), ("r=1e10", 16.0, 18.0, 1e10),
                 ("r=-1", 16.0, 17.2, -1.0), ("r=-0", 16.0, 17.2, -0.0), ("r=-3", 16.0, 17.2, -3.0), ("r=-3/edge", 2.5, 16.0, -3.0),
                 # 2^33 m away with a radius of 2^33 m: its edge crosses the candidates at x = 20 m (d - r cancels to ~ 1e-6 m absolute)
                 ("far_right", hs.FAR + 20.0, 16.0, hs.FAR)]


def _score_scenes(dm):
    """cfg and, per (base, hostile entry), the one-scene inputs; entry 0 of the obstacle list (a padding disc) becomes hostile."""
    def make():
        cfg = scs.config(dm)
        out = []
        for base, n_obs in SCORE_BASES:
            for hname, x, y, r in SCORE_HOSTILE:
                sc = scs.build(dm, cfg, [base], n_obs)
                ox, oy = float(sc["scene_in"]["grid_origin"]["x"][0]), float(sc["scene_in"]["grid_origin"]["y"][0])
                ob = sc["obs_pool"]
                ob["x"][0], ob["y"][0], ob["radius"][0] = ox + x, oy + y, r
                out.append((f"{base}/{n_obs}/{hname}", n_obs, sc))
        return cfg, out
    return _cached("score_scenes", make)


def _score_reference(dm, oracle):
    def make():
        cfg, scenes = _score_scenes(dm)
        k = scs.kernel_constants()
        out = []
        for tag, n_obs, sc in scenes:
            _, go, _, _, path = oracle.plan_tick_one(cfg, sc, 0, sc["state"].copy())
            obs = scs.scene_obstacles(sc, 0)
            with np.errstate(all="ignore"):
                model = gm.score_scene(cfg, sc["scene_in"][0], obs, path, int(go["status"]))
                form = scs.forms(cfg, sc["scene_in"][0], obs, path, int(go["status"]), k)
            out.append(dict(tag=tag, gout=go.copy(), path=path.copy(), model=model, form=form))
        return out
    return _cached("score_ref", make)


def _score_against_model(go, m, tag):
    bad = []
    for f in ("n_candidates", "best_candidate"):
        if int(go[f]) != m[f]:
            bad.append(f"{tag}.{f}: {int(go[f])} vs model {m[f]}")
    if not np.array_equal(go["cand_prog"], m["cand_prog"]):
        bad.append(f"{tag}.cand_prog: {go['cand_prog'].tolist()} vs model {m['cand_prog'].tolist()}")
    for f in ("cand_col", "cand_curv", "cand_cost"):
        a, b = np.asarray(go[f], np.float64), np.asarray(m[f], np.float64)
        with np.errstate(all="ignore"):
            ok = (np.isnan(a) & np.isnan(b)) | (a == b) | (np.abs(a - b) <= ATOL + RTOL * np.maximum(np.abs(a), np.abs(b)))
        if not ok.all():
            i = int(np.flatnonzero(~ok)[0])
            print(f"{tag}.{f}[{i}]: {a[i]!r} vs model {b[i]!r}")
            bad.append(f"{tag}.{f}: {int((~ok).sum())} beyond the bar, first at {i}: {a[i]!r} vs model {b[i]!r}")
    return bad


def test_oracle_scores_equal_the_model_on_every_obstacle_case(dm, oracle):
    """G3 of the oracle against the 40-digit model on every case of the list whose ego, goal and origin are finite, every tick of
    the moving ones and every twin; and no case sits on a discontinuity of the specification (tests/test_score_edges.py: a
    micrometre of clearance, 1e-5 of the fence), where a rounding could choose the side."""
    print("model arithmetic:", gm.ARITHMETIC)
    bad, n = [], 0
    for c0 in _cases():
        for c in (c0, hs.twin(c0)):
            if not _scored(c):
                continue
            for t, r in enumerate(_reference(dm, oracle, c)):
                tag = f"{c.name}@{t}"
                n += 1
                bad += _score_against_model(r["gout"], r["score"], tag)
                if r["score"]["min_abs_clearance"] < 1e-6 or r["score"]["min_fence"] < 1e-5:
                    bad.append(f"{tag}: |clearance| {r['score']['min_abs_clearance']:.3g} m, fence {r['score']['min_fence']:.3g}: on a discontinuity")
    assert n > 400, n
    assert not bad, "\n".join(bad[:20])


def test_oracle_scores_equal_the_model_with_a_hostile_obstacle(dm, oracle):
    """G3 of the oracle (the plain loop: the rule) against the 40-digit model, one hostile entry in the obstacle list of a scene of
    each form of score_body; and the forms are the ones the device tests mean to cover."""
    print("model arithmetic:", gm.ARITHMETIC)
    bad = []
    refs = _score_reference(dm, oracle)
    for r in refs:
        bad += _score_against_model(r["gout"], r["model"], r["tag"])
    forms = {}
    for r in refs:
        forms.setdefault(r["tag"].rsplit("/", 1)[0] if not r["tag"].endswith("/edge") else r["tag"].rsplit("/", 2)[0], set()).add(r["form"]["form"])
    print(forms)
    assert {f for v in forms.values() for f in v} >= set(SCORE_FORMS)
    by = {r["tag"]: r for r in refs}
    # R = +inf, FLT_MAX, 1e10: every point of every candidate collides; a NaN or -inf radius changes nothing
    plain = by["n_rel_7/256/r=nan"]["gout"]
    for h in ("r=+inf", "r=flt_max", "r=1e10"):
        g = by[f"n_rel_7/256/{h}"]["gout"]
        assert np.all(g["cand_col"][:int(g["n_candidates"])] == 200000.0) and np.all(g["cand_prog"][:int(g["n_candidates"])] == 1.0), h
    for h in ("r=-inf", "x=nan", "y=nan", "x=+inf", "y=-inf", "x=1e300", "x=-1e12", "r=-3", "r=-3/edge"):
        assert by[f"n_rel_7/256/{h}"]["gout"].tobytes() == plain.tobytes(), h
    assert not bad, "\n".join(bad[:20])


def _write_cases(dm, path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            cfg = _cfg(dm, c)
            sc = hs.build(dm, cfg, [c])
            attr = sc.get("attr_pool")
            blobs = [cfg.tobytes(), sc["scene_in"][:1].tobytes(), sc["state"][:1].tobytes(), sc["lane_pool"].tobytes(),
                     attr.tobytes() if attr is not None else b"", sc["ref_pool"].tobytes()]
            n_obs = len(sc["obs_pool"])
            f.write(struct.pack("<8i", *[len(b) for b in blobs], n_obs, c.ticks))
            for b in blobs:
                f.write(b)
            f.write(sc["obs_pool"].tobytes())
            f.write(sc["mot_pool"][:n_obs].tobytes())


def _build_native(exe, oracle_dir):
    src = [os.path.join(ROOT, "tests", "native", "grid_hostile.c")] + [os.path.join(oracle_dir, f) for f in ("dmpp_oracle.c", "dmpp_grid_oracle.c", "dmpp_oracle_batch.c")]
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-D_GNU_SOURCE", "-fsanitize=undefined,float-cast-overflow",
           "-fno-sanitize-recover=all", "-I" + oracle_dir, "-o", exe] + src + ["-lm", "-lpthread"]
    subprocess.check_call(cmd)


def test_oracle_c_has_no_undefined_behaviour_on_any_case(dm, oracle, tmp_path):
    """tests/native/grid_hostile.c with the oracle's sources under UBSan (float-cast-overflow included, no recovery): orc_cell_of, both
    rasterisers and whole oracle ticks on every case; its results are the models'."""
    cases = _cases()
    data, exe = str(tmp_path / "cases.bin"), str(tmp_path / "grid_hostile")
    _write_cases(dm, data, cases)
    _build_native(exe, os.path.join(ROOT, "oracle"))
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=600, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and f"grid_hostile ok: {len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    want = [(i, t, ref) for i, c in enumerate(cases) for t, ref in enumerate(_reference(dm, oracle, c))]
    assert len(lines) == len(want)
    for ln, (i, t, ref) in zip(lines, want):
        got = dict(zip(ln[0::2], ln[1::2]))
        m = ref["model"]
        assert (int(got["case"]), int(got["tick"])) == (i, t)
        assert (int(got["start"]), int(got["goal"]), int(got["occupied"])) == (ref["start"], ref["goal"], int(ref["grid"].sum())), (cases[i].name, got)
        assert (int(got["status"]), int(got["expanded"]), int(got["digest"], 16)) == (m["status"], m["n_expanded"], m["order_digest"]), (cases[i].name, got)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k_, v in old.items():
            if v is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v


def _run_case(dm, oracle, pl, c, check_grid=True, expect_dense=None):
    """The case's ticks on `pl` against the model; returns the mismatches."""
    bad = []
    cfg = _cfg(dm, c)
    sc = hs.build(dm, cfg, [c])
    pl.set_scenes(sc)
    pl.set_state(sc["state"])
    for t, r in enumerate(_reference(dm, oracle, c)):
        tag = f"{c.name}@{t}"
        m = r["model"]
        pl.tick(sync=True)
        go = pl.get_grid_out()[0]
        budget, need, dense = pl.search_info()
        if check_grid:                                             # (the grid of the tick just run: its obstacle snapshot)
            g = pl.get_grid(0)
            if not np.array_equal(g, r["grid"]):
                bad.append(f"{tag}: get_grid differs from the predicate in {int((g != r['grid']).sum())} cells")
        if not 0 <= need <= c.W * c.H // 32:
            bad.append(f"{tag}: search_info need = {need}")
        if expect_dense is not None and dense != expect_dense:
            bad.append(f"{tag}: dense = {dense}, expected {expect_dense}")
        if (int(go["start_cell"]), int(go["goal_cell"])) != (r["start"], r["goal"]):
            bad.append(f"{tag}: start / goal cell {int(go['start_cell'])} / {int(go['goal_cell'])} vs {r['start']} / {r['goal']}")
        order = pl.get_order(0, int(go["n_expanded"])) if int(go["n_expanded"]) == m["n_expanded"] else None
        path = pl.get_path(0, int(go["path_len"])) if int(go["path_len"]) == m["path_len"] else None
        bad += _search_mismatches(go, order, path, m, tag)
        if r["score"] is not None:                                 # (not specified under a non-finite ego, goal or origin)
            bad += compare(pl.get_grid_out()[0:1], r["gout"].reshape(1), tag)
            bad += _score_against_model(go, r["score"], tag)
    return bad


def _planner(dm, c, n=1, max_obs=512, budget=None):
    cfg = _cfg(dm, c)
    env = {"DMPP_LDS_BUDGET": str(budget if budget is not None else c.W * c.H // 32)}
    return _with_env(env, lambda: dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=max_obs, order_cap=c.W * c.H))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["128x128", "2048x32"])
def test_device_every_case_then_its_ordinary_twin(dm, oracle, shape):
    """One handle per grid shape: every case (grid, status, counters, digest, order, path), then its twin on the same handle."""
    todo = [c for c in _cases() if f"{c.W}x{c.H}" == shape]
    assert todo
    bad = []
    for moving in (False, True):                                   # (dynamic_obstacles is a field of the configuration: a handle each)
        mine = [c for c in todo if bool(c.mot) == moving]
        if not mine:
            continue
        pl = _planner(dm, mine[0])
        try:
            for c in mine:
                dense = None if c.family == "wide" else 0          # (2048 x 32 all ones may exceed what a workgroup can have of LDS)
                bad += _run_case(dm, oracle, pl, c, expect_dense=dense)
                if c.hostile or c.origin != c.twin_origin or c.ego != c.twin_ego or c.goal != c.twin_goal:
                    tw = hs.twin(c)
                    bad += _run_case(dm, oracle, pl, tw._replace(mot=[(0.0, 0.0)] * len(tw.obs)) if moving else tw, expect_dense=dense)
        finally:
            pl.close()
    assert not bad, "\n".join(bad[:30])


DENSE_FAMILIES = ("all", "chunk", "far")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gbm", "overflow"])
def test_device_dense_forms(dm, oracle, form):
    """The dense form of the views (forced, and for a scene that does not fit a tiny LDS budget): the all-at-once, chunk and
    far-and-large cases, each followed by its twin."""
    todo = [c for c in _cases() if c.family in DENSE_FAMILIES and c.name.startswith("o") and (c.family != "far" or c.name.endswith("/middle"))]
    assert len(todo) >= 10
    env = {"DMPP_SEARCH_GBM": "1"} if form == "gbm" else {"DMPP_LDS_BUDGET": "16"}
    bad = []

    def run():
        cfg = _cfg(dm, todo[0])
        pl = dm.Planner(cfg, device=0, max_scenes=1, max_obs_total=512, order_cap=hs.W * hs.H)
        try:
            for c in todo:
                for cc in (c, hs.twin(c)):
                    r = _reference(dm, oracle, cc)[0]
                    fits = form == "overflow" and int(r["grid"].sum()) == 0
                    bad.extend(_run_case(dm, oracle, pl, cc, expect_dense=None if fits else 1))
        finally:
            pl.close()
    _with_env(env, run)
    assert not bad, "\n".join(bad[:30])


@pytest.mark.gpu
def test_device_batch_of_64_hostile_beside_ordinary(dm, oracle):
    """One launch of 64 scenes (the 4-wave set-up of the batch path), hostile cases interleaved with ordinary twins: the record
    and the path of every ordinary twin are the bytes the same scene gives alone, and every hostile scene gives the model's answer."""
    pool = [c for c in _cases() if (c.W, c.H) == (hs.W, hs.H) and c.family in ("xy", "radius", "far", "all") and not c.mot and len(c.obs) <= 48]
    pick = [c for c in pool if c.name.endswith("/middle") or c.family == "all"][::2][:32]
    assert len(pick) == 32
    n_obs = 48
    scenes = [x for c in pick for x in (c, hs.twin(c))]
    cfg = _cfg(dm, pick[0])
    sc = hs.build(dm, cfg, scenes, n_obs)
    pl = dm.Planner(cfg, device=0, max_scenes=64, max_obs_total=64 * n_obs)
    one = dm.Planner(cfg, device=0, max_scenes=1, max_obs_total=n_obs)
    bad = []
    try:
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
        pl.tick(sync=True)
        gout = pl.get_grid_out()
        for s, c in enumerate(scenes):
            r = _reference(dm, oracle, c)[0]
            go = gout[s]
            path = pl.get_path(s, int(go["path_len"]))
            bad += _search_mismatches(go, None, path if int(go["path_len"]) == r["model"]["path_len"] else None, r["model"], f"batch[{s}] {c.name}")
            if r["score"] is not None:                             # (the padding discs lie beyond every cutoff: the same scores)
                bad += compare(gout[s:s + 1], r["gout"].reshape(1), f"batch[{s}] {c.name}") + _score_against_model(go, r["score"], f"batch[{s}] {c.name}")
            if s % 2 == 1:
                sc1 = hs.build(dm, cfg, [c], n_obs)
                one.set_scenes(sc1)
                one.set_state(sc1["state"])
                one.tick(sync=True)
                g1 = one.get_grid_out()[0]
                if g1.tobytes() != go.tobytes():
                    bad.append(f"batch[{s}] {c.name}: GridOut differs from the scene alone: " + "; ".join(compare(gout[s:s + 1], one.get_grid_out()[0:1], "", rtol=0.0, atol=0.0)))
                if one.get_path(0, int(g1["path_len"])).tobytes() != path.tobytes():
                    bad.append(f"batch[{s}] {c.name}: path differs from the scene alone")
    finally:
        one.close()
        pl.close()
    assert not bad, "\n".join(bad[:30])


def _score_tick(dm, cfg, scs_list, n_obs):
    """One launch over the given one-scene inputs (all with `n_obs` obstacles), laid out as a batch."""
    n = len(scs_list)
    sc = scs.build(dm, cfg, [scs.BASE] * n, n_obs)
    for s, one in enumerate(scs_list):
        sc["scene_in"][s] = one["scene_in"][0]
        sc["scene_in"]["obs_off"][s] = s * n_obs
        sc["state"][s] = one["state"][0]
        sc["obs_pool"][s * n_obs:(s + 1) * n_obs] = one["obs_pool"][:n_obs]
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
    try:
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
        pl.tick(sync=True)
        return pl.get_grid_out()
    finally:
        pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_obs", [256, 300])
def test_device_scores_with_a_hostile_obstacle(dm, oracle, n_obs):
    """score_body on each of its obstacle paths (culled LDS list with and without buckets, buckets from the snapshot, the plain
    loop over HBM) with one hostile entry in the list: alone (k_score<16>), in a batch of kScoreWideMaxScenes (k_score<16>) and of
    one more (k_score<4>) against the oracle and the 40-digit model, and the same bytes in the three settings."""
    cfg, scenes = _score_scenes(dm)
    refs = [r for r, (_, no, _) in zip(_score_reference(dm, oracle), scenes) if no == n_obs]
    mine = [sc for _, no, sc in scenes if no == n_obs]
    k = scs.kernel_constants()["kScoreWideMaxScenes"]
    runs = {"alone": np.concatenate([_score_tick(dm, cfg, [sc], n_obs) for sc in mine])}
    for w, n in (("wide", k), ("narrow", k + 1)):
        runs[w] = _score_tick(dm, cfg, [mine[i % len(mine)] for i in range(n)], n_obs)
    bad = []
    for w, gouts in runs.items():
        for i in range(len(gouts)):
            r = refs[i % len(refs)]
            tag = f"{w}[{i}] {r['tag']} ({r['form']['form']})"
            bad += compare(gouts[i:i + 1], r["gout"].reshape(1), tag)
            bad += _score_against_model(gouts[i], r["model"], tag)
            if gouts[i].tobytes() != runs["alone"][i % len(refs)].tobytes():
                bad.append(f"{tag}: the record differs from the scene alone")
    assert not bad, "\n".join(bad[:20])
