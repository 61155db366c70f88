"""Packed streamed fetch: pp_set_packed_fetch / pp_fetch_packed_async / pp_unpack_plan / pp_unpack_grid.

CPU: the two wire records against their numpy dtypes; the unpackers against tests/packed_model.py on the oracle's results for
the crafted scoring scenes (tests/score_scenes.py, n_lattice 0, 1, 16) and for the step-plane scenes (tests/packed_scenes.py,
the lookahead sweep) - the plan half and the grid-path / no-candidate records byte for byte against the ORACLE, a lattice
winner byte for byte against the model's own Bezier evaluation; every hostile record refused with the neighbours and the
guard words around the outputs intact.

GPU: unpack(packed) against the full fetch of the same tick on the same handle, byte for byte (cand_*[k != best] are 0 by
specification): streamed ticks at 300 and 40 scenes and at the wave edges 1, 63, 64, 65; the crafted scenes alone, inside a
batch of 129 and as 300 copies, their packed records the same bytes in all three and equal to the model's pack of the
device's own GridOut, path and SceneIn; the life cycle.
"""
import ctypes as C

import numpy as np
import pytest

import packed_model as pm
import packed_scenes as ps
import score_scenes as ss
from parity_util import move_ego

LATTICES = (0, 1, 16)
N_OBS_SCORE = 256
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _b(a):
    return np.ascontiguousarray(a).tobytes()


def _score_cfg(dm, nl):
    cfg = ss.config(dm)
    cfg["n_lattice"] = nl
    return cfg


def _oracle_refs(dm, oracle, key, cfg, sc, names):
    """Oracle PlanOut, GridOut and path of one scene per name (computed once per process, never modified)."""
    def make():
        out = []
        for s, name in enumerate(names):
            plan, go, _, _, path = oracle.plan_tick_one(cfg, sc, s, sc["state"].copy())
            out.append(dict(name=name, cfg=cfg, si=sc["scene_in"][s].copy(), plan=plan.copy(), gout=go.copy(), path=path.copy()))
        return out
    return _cached(key, make)


def _score_refs(dm, oracle, nl):
    cfg = _score_cfg(dm, nl)
    return _oracle_refs(dm, oracle, ("score", nl), cfg, ss.build(dm, cfg, ss.CASE_NAMES, N_OBS_SCORE), ss.CASE_NAMES)


def _step_refs(dm, oracle, la):
    cfg = ps.config(dm, la)
    return _oracle_refs(dm, oracle, ("steps", la), cfg, ps.build(dm, cfg, ps.CASE_NAMES), ps.CASE_NAMES)


def _expected_grid(dm, go, pk):
    """What pp_unpack_grid must deliver for GridOut `go` packed as `pk`: the record with cand_*[k != best] zeroed - and, for a
    lattice winner, best_path as the model evaluates the record's control points."""
    exp = pm.masked_grid_out(go)
    if int(pk["kind"]) == pm.LATTICE:
        pts = pm.bezier_points(pk["geo"])
        exp["best_path"]["x"][0], exp["best_path"]["y"][0] = pts[:, 0], pts[:, 1]
    return exp


def _check_model_roundtrip(dm, r, tag):
    """Pack r's oracle results with the model, unpack with the library, compare.  Returns the PackedGrid record."""
    cfg = r["cfg"]
    res, show, dec = dm.unpack_plan(cfg, np.array([pm.pack_plan(dm, r["plan"])]))
    assert _b(res[0]) == _b(r["plan"]["result"]), f"{tag}: PlanningOut"
    assert _b(show[0]) == _b(r["plan"]["show"]), f"{tag}: PlanningStatus"
    assert _b(dec[0]) == _b(r["plan"]["dec"]), f"{tag}: DecisionOutPod"
    pk = pm.pack_grid(dm, cfg, r["si"], r["gout"], r["path"])
    assert not int(pk["kind"]) & pm.BAD, f"{tag}: the oracle's path is no chain of neighbours from start_cell"
    out = dm.unpack_grid(cfg, np.array([pk]))
    exp = _expected_grid(dm, r["gout"], pk)
    if _b(out) != _b(exp):
        bad = [f for f in dm.GridOut.names if _b(out[f]) != _b(exp[f])]
        d = np.flatnonzero((out["best_path"]["x"][0] != exp["best_path"]["x"][0]) | (out["best_path"]["y"][0] != exp["best_path"]["y"][0]))
        raise AssertionError(f"{tag}: kind {int(pk['kind'])}, fields {bad}, best_path points {d[:8].tolist()} of {len(d)} differ")
    return pk


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_wire_records_sizes_and_offsets(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(43) == dm.PackedPlan.itemsize == 1744 and lib.pp_sizeof(44) == dm.PackedGrid.itemsize == 248
    off = lambda dt, f: dt.fields[f][1]
    assert [off(dm.PackedPlan, f) for f in ("brakedis", "cnt", "afresh_cause", "near_ob_dist", "planacc", "trafficlight", "ob_flag", "dec", "path_points")] == \
        [0, 48, 76, 80, 96, 104, 108, 112, 144]
    assert off(dm.PackedPlan, "afresh_cause") == off(dm.PlanningOut, "_pad")
    assert [off(dm.PackedGrid, f) for f in ("order_digest", "status", "n_candidates", "best_cost", "best_prog", "kind", "n_steps", "geo", "planes")] == \
        [0, 8, 44, 48, 72, 80, 84, 88, 152]
    for f in pm.GRID_HEAD:                                   # the first 48 bytes of GridOut as they stand
        assert dm.PackedGrid.fields[f] == dm.GridOut.fields[f]
    assert off(dm.GridOut, "cand_cost") == 48
    assert dm.PackedPlan.itemsize + dm.PackedGrid.itemsize == 1992
    assert dm.PlanningOut.itemsize + dm.PlanningStatus.itemsize + dm.GridOut.itemsize == 7104
    assert (dm.PACKED_NONE, dm.PACKED_LATTICE, dm.PACKED_PATH, dm.PACKED_BAD) == (pm.NONE, pm.LATTICE, pm.PATH, pm.BAD) == (0, 1, 2, 4)


def test_unpackers_against_the_model_on_the_scoring_cases(dm, oracle):
    kinds, statuses = set(), set()
    for nl in LATTICES:
        for r in _score_refs(dm, oracle, nl):
            pk = _check_model_roundtrip(dm, r, f"{r['name']}/n_lattice {nl}")
            kind, status = int(pk["kind"]), int(r["gout"]["status"])
            kinds.add(kind)
            statuses.add(status)
            if nl == 0:                                      # a found path must win; without one there is no candidate
                assert kind == (pm.PATH if status == pm.G_FOUND else pm.NONE), (r["name"], kind, status)
        if nl == 0:
            by_name = {r["name"]: int(r["gout"]["status"]) for r in _score_refs(dm, oracle, 0)}
            assert by_name["blocked_goal"] == dm.G_GOAL_BLOCKED and by_name[ss.BASE] == dm.G_FOUND
    assert kinds == {pm.NONE, pm.LATTICE, pm.PATH}, kinds
    assert statuses - {pm.G_FOUND}, statuses


def test_step_planes_on_the_lookahead_sweep(dm, oracle):
    codes = set()
    for la in ps.LOOKAHEADS:
        for r in _step_refs(dm, oracle, la):
            tag = f"{r['name']}/lookahead {la}"
            path_len = int(r["gout"]["path_len"])
            assert int(r["gout"]["status"]) == pm.G_FOUND, tag
            if r["name"] in ps.LONG:
                assert path_len - 1 >= ps.MIN_APART, (tag, path_len)
            pk = _check_model_roundtrip(dm, r, tag)
            assert int(pk["kind"]) == pm.PATH, tag
            assert int(pk["n_steps"]) == min(path_len - 1, la, 199), (tag, int(pk["n_steps"]), path_len)
            codes |= set(pm.step_codes(pk))
    short = {r["name"]: int(r["gout"]["path_len"]) for r in _step_refs(dm, oracle, 400)}["short"]
    assert 1 < short - 1 < min(la for la in ps.LOOKAHEADS if la > 1), short      # one path shorter than the lookaheads
    assert codes == set(range(8)), codes
    mixed = [r for r in _step_refs(dm, oracle, 199) if r["name"] == "mixed"][0]
    assert len(set(pm.step_codes(pm.pack_grid(dm, mixed["cfg"], mixed["si"], mixed["gout"], mixed["path"])))) >= 3


def _hostile_records(dm, oracle):
    """(name, record) pairs no tick packs, made from valid records of the step scenes."""
    refs = {r["name"]: r for r in _step_refs(dm, oracle, 199)}
    cfg = refs["east"]["cfg"]
    W, H = int(cfg["grid_w"][0]), int(cfg["grid_h"][0])
    good = {k: pm.pack_grid(dm, cfg, r["si"], r["gout"], r["path"]) for k, r in refs.items()}
    out = []

    def add(name, base, **kw):
        pk = good[base].copy()
        for f, v in kw.items():
            pk[f] = v
        out.append((name, pk))
    for v in (-1, 200, 256, 2 ** 31 - 1, -2 ** 31):
        add(f"n_steps {v}", "east", n_steps=v)
    for v in (3, 5, 8, 16, -1, 2 ** 31 - 1, -2 ** 31):
        add(f"kind {v}", "east", kind=v)
    add("bad bit on a path record", "east", kind=pm.PATH | pm.BAD)
    add("bad bit on a lattice record", "east", kind=pm.LATTICE | pm.BAD)
    add("bad bit alone", "east", kind=pm.BAD)
    for v in (-1, 17, 2 ** 31 - 1, -2 ** 31):
        add(f"best_candidate {v} (path)", "east", best_candidate=v)
        add(f"best_candidate {v} (lattice)", "east", best_candidate=v, kind=pm.LATTICE)
    for v in (-1, W * H, 2 ** 31 - 1, -2 ** 31):
        add(f"start_cell {v}", "east", start_cell=v)
    add("walk leaves the east edge", "east", start_cell=W - 10)
    add("walk leaves the west edge", "west", start_cell=10)
    add("walk leaves the north edge", "north", start_cell=(H - 10) * W + 5)
    add("walk leaves the south edge", "south", start_cell=10 * W + 5)
    add("walk leaves a corner", "north_east", start_cell=(H - 3) * W + W - 3)
    add("every plane bit set", "east", planes=np.full(12, 2 ** 64 - 1, np.uint64), start_cell=5, n_steps=199)
    return cfg, good, out


def test_hostile_records_are_refused_and_nothing_else_is_touched(dm, oracle):
    lib = dm.load_library()
    cfg, good, hostile = _hostile_records(dm, oracle)
    ok = good["mixed"]
    want_ok = _b(dm.unpack_grid(cfg, np.array([ok])))
    guard, item = 4096, dm.GridOut.itemsize
    for name, pk in hostile:
        recs = np.array([ok, pk, ok])
        raw = np.full(2 * guard + 3 * item, 0xA5, np.uint8)
        out = np.frombuffer(raw, dm.GridOut, 3, guard)
        rc = lib.pp_unpack_grid(C.c_void_p(cfg.ctypes.data), C.c_void_p(recs.ctypes.data), 3, C.c_void_p(out.ctypes.data))
        assert rc == dm.PP_ERR_ARG, (name, rc)
        assert (raw[:guard] == 0xA5).all() and (raw[-guard:] == 0xA5).all(), name
        assert _b(out[0]) == want_ok and _b(out[2]) == want_ok, name
        assert not np.frombuffer(_b(out[1]), np.uint8).any(), name
        with pytest.raises(dm.PlannerError):
            dm.unpack_grid(cfg, np.array([pk]))
    # a grid of another size than the records were packed for: refused or unpacked, never outside the arrays
    small = cfg.copy()
    small["grid_w"], small["grid_h"] = 32, 32
    for name in ("east", "north_east", "mixed"):
        raw = np.full(2 * guard + item, 0xA5, np.uint8)
        out = np.frombuffer(raw, dm.GridOut, 1, guard)
        rec = np.array([good[name]])
        rc = lib.pp_unpack_grid(C.c_void_p(small.ctypes.data), C.c_void_p(rec.ctypes.data), 1, C.c_void_p(out.ctypes.data))
        assert rc == dm.PP_ERR_ARG and not raw[guard:-guard].any() and (raw[:guard] == 0xA5).all() and (raw[-guard:] == 0xA5).all(), name
    # the plan half has no record to refuse: every output may be NULL, and each is written inside its own array only
    r = _step_refs(dm, oracle, 199)[0]
    pkp = np.array([pm.pack_plan(dm, r["plan"])] * 2)
    for which in range(8):
        bufs, ptrs = [], []
        for bit, dt in enumerate((dm.PlanningOut, dm.PlanningStatus, dm.DecisionOutPod)):
            raw = np.full(2 * guard + 2 * dt.itemsize, 0xA5, np.uint8)
            bufs.append((raw, dt, bool(which >> bit & 1)))
            ptrs.append(C.c_void_p(raw.ctypes.data + guard) if which >> bit & 1 else None)
        assert lib.pp_unpack_plan(C.c_void_p(cfg.ctypes.data), C.c_void_p(pkp.ctypes.data), 2, *ptrs) == dm.PP_OK
        for (raw, dt, used), f in zip(bufs, ("result", "show", "dec")):
            assert (raw[:guard] == 0xA5).all() and (raw[-guard:] == 0xA5).all()
            if used:
                assert raw[guard:-guard].tobytes() == _b(r["plan"][f]) * 2, f
            else:
                assert (raw == 0xA5).all()
    assert lib.pp_unpack_grid(None, C.c_void_p(pkp.ctypes.data), 1, C.c_void_p(pkp.ctypes.data)) == dm.PP_ERR_ARG
    assert lib.pp_unpack_plan(C.c_void_p(cfg.ctypes.data), None, 1, None, None, None) == dm.PP_ERR_ARG


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _buffers(dm, n, grid=True):
    return (dm.pinned_empty(n, dm.PlanOut), dm.pinned_empty(n, dm.GridOut) if grid else None,
            dm.pinned_empty(n, dm.PackedPlan), dm.pinned_empty(n, dm.PackedGrid) if grid else None)


def _fetch_both(pl, bufs):
    plan, gout, pkp, pkg = bufs
    a, b = pl.fetch_async(plan, gout), pl.fetch_packed_async(pkp, pkg)
    assert a == b == pl.tick_id()
    return a


def _assert_unpacks_to(dm, cfg, bufs, tag):
    plan, gout, pkp, pkg = bufs
    res, show, dec = dm.unpack_plan(cfg, np.array(pkp))
    assert _b(res) == _b(plan["result"]), f"{tag}: PlanningOut"
    assert _b(show) == _b(plan["show"]), f"{tag}: PlanningStatus"
    assert _b(dec) == _b(plan["dec"]), f"{tag}: DecisionOutPod"
    assert np.array_equal(pkp["ob_flag"], plan["ob_flag"]), f"{tag}: ob_flag"
    if gout is not None:
        out, exp = dm.unpack_grid(cfg, np.array(pkg)), pm.masked_grid_out(np.array(gout))
        if _b(out) != _b(exp):
            rows = [s for s in range(len(out)) if _b(out[s]) != _b(exp[s])]
            bad = [f for f in dm.GridOut.names if _b(out[rows[0]][f]) != _b(exp[rows[0]][f])]
            raise AssertionError(f"{tag}: {len(rows)} scene(s) differ, first {rows[0]} (kind {int(pkg['kind'][rows[0]])}) in {bad}")


def _streamed(dm, n, n_obs, grid, ticks, seed):
    cfg = dm.default_config(grid)
    cfg["force_replan"] = 1
    cfg["dynamic_obstacles"] = 0
    sc = dm.gen_scenes(cfg, seed, n, n_obs, junction_every=8)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    pl.set_packed_fetch(True)
    rng = np.random.default_rng(seed)
    keep, ids, bufs = [], [], [_buffers(dm, n) for _ in range(ticks)]
    for t in range(ticks):
        move_ego(sc, 1 + (t % 3), dlat=0.05 * ((t % 5) - 2))
        sc["obs_pool"]["x"] += rng.uniform(-0.4, 0.4, len(sc["obs_pool"]))
        sc["obs_pool"]["y"] += rng.uniform(-0.4, 0.4, len(sc["obs_pool"]))
        keep.append((dm.pinned_copy(sc["scene_in"]), dm.pinned_copy(sc["obs_pool"])))
        pl.update_async(*keep[-1])
        pl.tick()
        ids.append(_fetch_both(pl, bufs[t]))
    assert ids == list(range(ids[0], ids[0] + ticks))
    for t in reversed(range(ticks)):
        assert pl.wait_tick(ids[t]) == 0
    kinds = set()
    for t in range(ticks):
        _assert_unpacks_to(dm, cfg, bufs[t], f"n {n}, tick {t}")
        kinds |= set(np.unique(bufs[t][3]["kind"]).tolist())
    pl.close()
    return kinds


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 40])
def test_streamed_ticks_unpack_to_the_full_fetch(dm, n):
    kinds = _streamed(dm, n, 24, 128, 6, 9100 + n)
    assert kinds <= {0, 1, 2} and kinds & {1, 2}, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_one_tick_at_the_wave_edges(dm, n):
    _streamed(dm, n, 24, 128, 1, 9200 + n)


_handles = {}


def _handle(dm, grid, cfg, n_obs):
    """One armed handle per grid size for the crafted scenes, re-configured per case (closed by the module's finaliser)."""
    if grid not in _handles:
        pl = dm.Planner(cfg, device=0, max_scenes=300, max_obs_total=300 * n_obs)
        pl.set_packed_fetch(True)
        _handles[grid] = pl
    _handles[grid].set_config(cfg)
    return _handles[grid]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for pl in _handles.values():
        pl.close()
    _handles.clear()


def _run(dm, pl, cfg, sc, with_motion=False):
    n = len(sc["scene_in"])
    pl.set_scenes(sc, with_motion=with_motion)
    pl.set_state(sc["state"])
    bufs = _buffers(dm, n)
    pl.tick()
    assert pl.wait_tick(_fetch_both(pl, bufs)) == 0
    _assert_unpacks_to(dm, cfg, bufs, f"{n} scenes")
    return bufs


def _join_scenes(singles):
    """One batch out of one-scene dicts (as gen_scenes lays a batch out: scene i's slices in the i-th share of every pool): scene i
    of the batch is singles[i] in every byte but the five slice offsets, which move with its share."""
    n = len(singles)
    out = {k: np.concatenate([s[k] for s in singles]) for k in ("scene_in", "lane_pool", "attr_pool", "ref_pool", "obs_pool", "mot_pool", "state")}
    out["n_obs"] = singles[0]["n_obs"]
    si = out["scene_in"]
    for i, s in enumerate(singles):
        assert s["n_obs"] == out["n_obs"] and len(s["scene_in"]) == 1
        for f in ("cur_off", "left_off", "right_off"):
            si["lanes"][f][i] += i * len(s["lane_pool"])
        si["ref_off"][i] += i * len(s["ref_pool"])
        si["obs_off"][i] += i * len(s["obs_pool"])
    assert len(si) == n
    return out


SINCOS_NOTE = ("  (For a lattice winner the model's control points come from the C library's sin / cos / atan and the device's from its own "
               "sincos / atan: that the two agree bit for bit is an observation on the toolchains this was written with, not a guarantee "
               "of either library - if ONLY geo of kind-1 records differs, by an ulp, after a compiler or libm change, the model's "
               "transcendentals moved, not the pack kernel.)")


def _crafted_on_device(dm, pl, cfg, build, names, n_obs):
    """Every scene alone, all of them inside one batch of 129, each as 300 copies: the same packed bytes - PackedPlan and
    PackedGrid - in all three, equal to the model's pack of the device's own PlanOut, GridOut, path and SceneIn."""
    alone, kinds, single = [], set(), {}
    for s, name in enumerate(names):
        sc = single[name] = build([name])
        plan, gout, pkp, pkg = _run(dm, pl, cfg, sc)
        path = pl.get_path(0, max(int(gout["path_len"][0]), 1))
        want_p, want_g = pm.pack_plan(dm, plan[0]), pm.pack_grid(dm, cfg, sc["scene_in"][0], gout[0], path)
        assert _b(pkp[0]) == _b(want_p), f"{name}: PackedPlan against the model"
        if _b(pkg[0]) != _b(want_g):
            bad = [f for f in dm.PackedGrid.names if _b(pkg[0][f]) != _b(want_g[f])]
            raise AssertionError(f"{name}: PackedGrid against the model differs in {bad}: device {[pkg[0][f] for f in bad]}, model {[want_g[f] for f in bad]}" + SINCOS_NOTE)
        alone.append((np.array(pkp[0]), np.array(pkg[0])))
        kinds.add(int(pkg["kind"][0]))
    _, _, pkp, pkg = _run(dm, pl, cfg, _join_scenes([single[names[i % len(names)]] for i in range(129)]))
    for i in range(129):
        s = i % len(names)
        assert _b(pkp[i]) == _b(alone[s][0]), f"{names[s]}: PackedPlan of scene {i} of the batch of 129"
        assert _b(pkg[i]) == _b(alone[s][1]), f"{names[s]}: PackedGrid of scene {i} of the batch of 129"
    for s, name in enumerate(names):
        _, _, pkp, pkg = _run(dm, pl, cfg, _join_scenes([single[name]] * 300))
        assert _b(pkp) == _b(alone[s][0]) * 300, f"{name}: PackedPlan, 300 copies"
        assert _b(pkg) == _b(alone[s][1]) * 300, f"{name}: PackedGrid, 300 copies"
    return kinds


@pytest.mark.gpu
@pytest.mark.parametrize("nl", LATTICES)
def test_crafted_scoring_scenes_on_the_device(dm, nl):
    cfg = _score_cfg(dm, nl)
    pl = _handle(dm, ss.GRID, cfg, N_OBS_SCORE)
    kinds = _crafted_on_device(dm, pl, cfg, lambda names: ss.build(dm, cfg, list(names), N_OBS_SCORE), ss.CASE_NAMES, N_OBS_SCORE)
    assert kinds == ({pm.NONE, pm.PATH} if nl == 0 else kinds) and (nl == 0 or pm.LATTICE in kinds), kinds


@pytest.mark.gpu
@pytest.mark.parametrize("la", ps.LOOKAHEADS)
def test_step_planes_on_the_device(dm, la):
    cfg = ps.config(dm, la)
    pl = _handle(dm, ps.GRID, cfg, ps.N_OBS)
    kinds = _crafted_on_device(dm, pl, cfg, lambda names: ps.build(dm, cfg, list(names)), ps.CASE_NAMES, ps.N_OBS)
    assert kinds == {pm.PATH}, kinds


def _small(dm, n=64, n_obs=16, grid=128, grid_stage=1, seed=9400):
    cfg = dm.default_config(grid)
    cfg["force_replan"] = 1
    cfg["dynamic_obstacles"] = 0
    cfg["grid_stage"] = grid_stage
    sc = dm.gen_scenes(cfg, seed, n, n_obs, junction_every=8)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * n_obs)
    pl.set_scenes(sc, with_motion=False)
    pl.set_state(sc["state"])
    return cfg, sc, pl


@pytest.mark.gpu
def test_error_paths_and_rearming(dm):
    lib = dm.load_library()
    cfg, sc, pl = _small(dm)
    n = pl.n
    plan, gout, pkp, pkg = bufs = _buffers(dm, n)
    fetch = lambda a, b: lib.pp_fetch_packed_async(pl.h, C.c_void_p(a.ctypes.data) if a is not None else None, C.c_void_p(b.ctypes.data) if b is not None else None, None)
    pl.tick()
    assert fetch(pkp, pkg) == dm.PP_ERR_STATE                      # not armed
    pl.set_packed_fetch(True)
    assert fetch(pkp, pkg) == dm.PP_ERR_STATE                      # the tick ran before arming
    assert fetch(None, None) == dm.PP_ERR_ARG
    pl.tick()
    assert fetch(None, None) == dm.PP_ERR_ARG
    assert pl.wait_tick(_fetch_both(pl, bufs)) == 0
    _assert_unpacks_to(dm, cfg, bufs, "armed")
    pl.set_packed_fetch(False)
    pl.tick()
    assert fetch(pkp, pkg) == dm.PP_ERR_STATE                      # disarmed
    pl.set_packed_fetch(True)
    assert fetch(pkp, None) == dm.PP_ERR_STATE                     # ... and that tick ran while it was
    pl.set_packed_fetch(True)                                      # arming twice changes nothing
    for t in range(3):
        pl.tick()
        assert pl.wait_tick(_fetch_both(pl, bufs)) == 0
        _assert_unpacks_to(dm, cfg, bufs, f"armed again, tick {t}")
    # the grid half asked for by itself, and joined to a published fetch of the same tick
    pl.tick()
    res, show = dm.pinned_empty(n, dm.PlanningOut), dm.pinned_empty(n, dm.PlanningStatus)
    a = pl.fetch_published_async(res, show, gout)
    assert pl.fetch_packed_async(None, pkg) == a and pl.fetch_packed_async(pkp, None) == a
    assert pl.wait_tick(a) == 0
    r2, s2, _ = dm.unpack_plan(cfg, np.array(pkp))
    assert _b(r2) == _b(res) and _b(s2) == _b(show)
    assert _b(dm.unpack_grid(cfg, np.array(pkg))) == _b(pm.masked_grid_out(np.array(gout)))
    pl.close()
    # grid stage off: the plan half works, the grid half is refused
    cfg, sc, pl = _small(dm, grid_stage=0)
    pl.set_packed_fetch(True)
    pl.tick()
    assert fetch(pkp, pkg) == dm.PP_ERR_STATE and fetch(None, pkg) == dm.PP_ERR_STATE
    bufs = _buffers(dm, n, grid=False)
    assert pl.wait_tick(_fetch_both(pl, bufs)) == 0
    _assert_unpacks_to(dm, cfg, bufs, "grid stage off")
    pl.close()


@pytest.mark.gpu
def test_survives_new_scenes_and_a_rollout(dm):
    cfg, sc, pl = _small(dm, n=96)
    pl.set_packed_fetch(True)
    bufs = _buffers(dm, 96)
    pl.tick()
    assert pl.wait_tick(_fetch_both(pl, bufs)) == 0
    _assert_unpacks_to(dm, cfg, bufs, "96 scenes")
    sc2 = dm.gen_scenes(cfg, 9500, 33, 16, junction_every=8)       # another n on the same armed handle
    _run(dm, pl, cfg, sc2)
    # a rollout of 5 ticks, then the packed records of its last tick against the synchronous getters
    last = pl.rollout(5)
    pkp, pkg = dm.pinned_empty(33, dm.PackedPlan), dm.pinned_empty(33, dm.PackedGrid)
    assert pl.fetch_packed_async(pkp, pkg) == last
    assert pl.wait_tick(last) == 0
    plan, gout = pl.get_plan(), pl.get_grid_out()
    res, show, dec = dm.unpack_plan(cfg, np.array(pkp))
    assert _b(res) == _b(plan["result"]) and _b(show) == _b(plan["show"]) and _b(dec) == _b(plan["dec"])
    assert _b(dm.unpack_grid(cfg, np.array(pkg))) == _b(pm.masked_grid_out(gout))
    pl.close()


@pytest.mark.gpu
def test_an_unarmed_handle_computes_the_same_and_launches_no_pack_kernel(dm):
    cfg, sc, armed = _small(dm)
    _, _, plain = _small(dm)
    armed.set_packed_fetch(True)
    for pl in (armed, plain):
        pl.set_profile(True)
        pl.reset_kernel_ms()
    bufs = _buffers(dm, armed.n)
    for t in range(4):
        armed.tick()
        plain.tick()
        assert armed.wait_tick(_fetch_both(armed, bufs)) == 0
    for name, get in (("PlanOut", lambda p: p.get_plan()), ("GridOut", lambda p: p.get_grid_out()), ("SceneState", lambda p: p.get_state())):
        assert _b(get(armed)) == _b(get(plain)), name
    ka, kp = armed.kernel_ms(), plain.kernel_ms()
    assert ka["k_pack_plan"][1] == 4 and ka["k_pack_grid"][1] == 4, ka
    assert kp["k_pack_plan"][1] == 0 and kp["k_pack_grid"][1] == 0 and kp["k_planning"][1] == 4, kp
    armed.close()
    plain.close()


@pytest.mark.gpu
def test_requests_that_join_only_in_part_lose_no_destination(dm):
    """Several requests for one tick, overlapping in what they ask for (the same side, the same record kind, twice): every
    destination a call accepted is filled - each call is download records of its own, one per side, none joins another."""
    cfg, sc, pl = _small(dm, n=300, n_obs=24)
    pl.set_packed_fetch(True)
    n = pl.n
    a, b = _buffers(dm, n), _buffers(dm, n)
    for t in range(3):
        for bufs in (a, b):
            for x in bufs:
                x.view(np.uint8)[:] = 0xA5
        pl.tick()
        ids = [pl.fetch_async(a[0], None), pl.fetch_packed_async(a[2], None),      # plan side: PlanOut, then PackedPlan
               pl.fetch_async(b[0], b[1]),                                         # both sides: a second PlanOut, the first GridOut
               pl.fetch_packed_async(b[2], b[3]),                                  # both sides: a second PackedPlan, the first PackedGrid
               pl.fetch_packed_async(None, a[3]), pl.fetch_async(None, a[1])]
        assert len(set(ids)) == 1
        assert pl.wait_tick(ids[0]) == 0
        for k, name in enumerate(("PlanOut", "GridOut", "PackedPlan", "PackedGrid")):
            assert _b(a[k]) == _b(b[k]), f"tick {t}: {name}"
        _assert_unpacks_to(dm, cfg, a, f"tick {t}")
    pl.close()
