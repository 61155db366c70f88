"""The search in 19 LDS granules ("LDS budget and the dense form"): the expansion number packed into the word of the
closed-set hash, and the co-residency step behind the budget policy.

CPU: `pp_coresident_budget`, the step as a pure function, row by row.

GPU, the packed word (`ClosedWord` of csrc/kernels_s.hpp): bitmap scenes of tests/search_scenes.py, one to four per launch,
against tests/grid_search_model.py in status, counters, digest, expansion order and path, and against the oracle for the whole
tick.  The scenes sit where the packing can go wrong:
  * the highest cell of a 512 x 512 and of a 1024 x 1024 grid closed with an expansion number >= 256 (the top cell bit and the
    top number bit in one word) and on the path;
  * a search that ends inside a batch of four (LIMIT on the first node of a step that would close four): the others were
    inserted but never expanded and carry the marker; they must not count in the digest;
  * max_expansions 384 | 385 and searches of 374 .. 389 expansions: the hash is replayed into HBM, the number stripped;
  * a path of more than 512 hops on 1056 x 32 and one 2048 x 2048 scene: the form that keeps the numbers in an array.
All integers; the float scores of the whole-tick comparison use parity_util.RTOL.

GPU, the step: 1,600 scenes of 64 obstacles at 512 x 512 - six searching workgroups on each of 256 CUs are 1,536 slots, so the
items of one tick outnumber them - with the step on and off."""
import ctypes
import os

import numpy as np
import pytest

import grid_search_model as gm
import search_scenes as ss
from parity_util import compare

FIELDS = ("n_expanded", "n_pushed", "n_rounds", "path_cost", "path_len", "order_digest")
BIG = dict(max_path=8192)


# ---- CPU: the step as a function -----------------------------------------------------------------------------------------
def test_coresident_budget_arithmetic(dm):
    """pp_coresident_budget, no device: static LDS 7,344, metas 4,096, dense-form LDS 8,192, at most 8,192 words, 256 CUs.  A
    workgroup is 7,344 + 64 + 4,096 + 8 * budget bytes in granules of 1,280; a CU has 128; 12 must stay free."""
    lib = dm.load_library()
    i32 = ctypes.c_int32
    lib.pp_coresident_budget.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(i32)]
    FIXED, DENSE = 1, 2
    rows = [  # items, need, policy budget, mode -> launch budget
        ((3072, 1498, 1792, 0), 1600),          # the headline: 21 granules, six per CU, 2 free -> 19 granules, 14 free
        ((1024, 1498, 1792, 0), 1792),          # a slot for every item
        ((3072, 1505, 1792, 0), 1792),          # tight is 1,664 = 20 granules: 8 free, nothing gained
        ((3072, 1498, 1792, FIXED), 1792),
        ((3072, 1498, 1792, DENSE), 1792),
        ((2048, 4350, 5056, 0), 4608),          # configs[3]: 41 granules, three per CU, 5 free -> 38 granules, 14 free
        ((3072, 1300, 1536, 0), 1536),          # 23,888 bytes are 19 granules already: 14 free
        ((3072, -1, 1792, 0), 1792),            # no need has landed: no tight budget to stay above
    ]
    for args, want in rows:
        out = i32(-7)
        assert lib.pp_coresident_budget(7344, 4096, 8192, 8192, 256, *args, ctypes.byref(out)) == 0
        assert out.value == want, (args, want, out.value)
    g = lambda b: -(-(7344 + 64 + 4096 + 8 * b) // 1280)
    assert (g(1792), g(1600), 128 - 6 * g(1600)) == (21, 19, 14) and (g(5056), g(4608), 128 - 3 * g(4608)) == (41, 38, 14)


# ---- GPU: the packed word ------------------------------------------------------------------------------------------------
def _corner_case(W, seed, name):
    """A 72 x 72 block of density 0.18 in the top corner of a W x W grid, the goal on the highest cell: FOUND after 274 .. 377
    expansions (seeds found by scanning with the model), so the goal's word holds cell W * W - 1 and a number >= 256."""
    rng = np.random.default_rng([seed, 512, 9])
    b = np.zeros((W, W), np.uint8)
    b[W - 72:, W - 72:] = (rng.random((72, 72)) < 0.18).astype(np.uint8)
    st = (W - 70, W - 66)
    b[W - 1, W - 1] = b[st[1], st[0]] = 0
    return ss.Case(name, W, W, b, st, (W - 1, W - 1), {})


CORNER_SEEDS = (0, 1, 15)               # 300, 377, 274 expansions


def _launch_cases():
    """name -> (cases of one launch, config fields changed)."""
    sweep = ss.walled_case(ss.SWEEP_128)
    wide = np.zeros((2048, 2048), np.uint8)
    rng = np.random.default_rng(2048)
    wide[1900:2040, 1900:2040] = (rng.random((140, 140)) < 0.03).astype(np.uint8)
    wide[2047, 2047] = wide[1904, 1910] = 0
    out = {
        "corner/512": ([_corner_case(512, s, f"corner/512/{s}") for s in CORNER_SEEDS], {}),
        "corner/1024": ([_corner_case(1024, s, f"corner/1024/{s}") for s in CORNER_SEEDS], {}),
        # steps 149 and 148 of the unlimited search close four cells from 272 and 268 expansions on: LIMIT on their first | second node
        "limit_in_batch/273": ([sweep], dict(max_expansions=273)),
        "limit_in_batch/270": ([sweep], dict(max_expansions=270)),
        "closed/384": ([sweep], dict(max_expansions=384)),
        "closed/385": ([sweep], dict(max_expansions=385)),
        "near_closed_max": ([ss.walled_case(s) for s in ss.NEAR_CLOSED_MAX[:4]], {}),
        "hops/601": ([ss.zigzag_case(ss.ZIGZAG_1056[0], 1056)], BIG),
        "grid/2048": ([ss.Case("corner/2048", 2048, 2048, wide, (1910, 1904), (2047, 2047), {})], BIG),
    }
    return out


LAUNCHES = ["corner/512", "corner/1024", "limit_in_batch/273", "limit_in_batch/270", "closed/384", "closed/385", "near_closed_max",
            "hops/601", "grid/2048"]
_cache = {}


def _launch(name):
    if "launches" not in _cache:
        _cache["launches"] = _launch_cases()
    return _cache["launches"][name]


def _cell(c, p):
    return p[1] * c.W + p[0]


def _model(c, cfg):
    return gm.search(c.bitmap.tobytes(), c.W, c.H, _cell(c, c.start), _cell(c, c.goal), int(cfg["max_expansions"][0]),
                     int(cfg["bucket_cap"][0]), int(cfg["max_path"][0]))


def test_packed_word_scenes_sit_on_their_edges(dm):
    """CPU: what the scenes are there for, from the model's trace and the kernel's constants."""
    k = ss.kernel_constants()
    assert set(LAUNCHES) == set(_launch_cases())
    for name in LAUNCHES:
        cases, over = _launch(name)
        assert 1 <= len(cases) <= 4
        for c in cases:
            cfg = ss.config(dm, c.W, c.H, **over)
            m = _model(c, cfg)
            f = ss.forms(m, cfg, len(cases), k)
            if name.startswith("corner/"):
                W = c.W
                assert f["K"] == {512: 0, 1024: 1}[W] and m["status"] == gm.FOUND and f["closed_spill_step"] is None
                seq = m["order"].index(W * W - 1)
                # the word holds cell + 1 = W * W: bit 18 | 20, the top one any cell of the kind sets, beside bit 8 of the number
                assert 256 <= seq < k["kClosedMax"][f["K"]] and m["path"][-1] == W * W - 1 and W * W == 1 << (18 if W == 512 else 20)
            elif name.startswith("limit_in_batch/"):
                unlimited = _model(c, ss.config(dm, c.W, c.H))
                n, step = 0, None
                for st in unlimited["steps"]:
                    if n + len(st["closed"]) >= int(over["max_expansions"]):
                        step = st
                        break
                    n += len(st["closed"])
                # the step that reaches the limit would have closed more cells than it may: the rest were inserted and cut off
                assert m["status"] == gm.LIMIT and f["closed_spill_step"] is None and n + len(step["closed"]) > int(over["max_expansions"])
            elif name.startswith("closed/"):
                assert m["status"] == gm.LIMIT and f["closed_spill_step"] is not None and m["n_expanded"] == int(over["max_expansions"])
            elif name == "near_closed_max":
                assert m["status"] == gm.FOUND and 374 <= m["n_expanded"] <= 389
            elif name == "hops/601":
                assert f["K"] == 2 and m["status"] == gm.FOUND and m["hops"] > k["DMPP_OPEN_CAP"] and f["closed_spill_step"] is None
            elif name == "grid/2048":
                assert f["K"] == 2 and m["status"] == gm.FOUND and m["n_expanded"] > 8
    spilled = [ss.forms(_model(c, ss.config(dm, 128, 128)), ss.config(dm, 128, 128), 4, k)["closed_spill_step"] is not None
               for c in _launch("near_closed_max")[0]]
    assert any(spilled) and not all(spilled)              # on either side of n_exp + 4 > 384


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAUNCHES)
def test_device_search_with_packed_hash_word(dm, oracle, name):
    cases, over = _launch(name)
    c0 = cases[0]
    cfg = ss.config(dm, c0.W, c0.H, **over)
    models = [_model(c, cfg) for c in cases]
    n_obs = max(1, max(int(np.count_nonzero(c.bitmap)) for c in cases))
    sc = ss.build(dm, cfg, [(c.bitmap, c.start, c.goal) for c in cases], n_obs)
    st_o = sc["state"].copy()
    plan_o, gout_o, _ = oracle.plan_tick_batch(cfg, sc, st_o, n_threads=4)
    order_cap = 64 + max(m["n_expanded"] for m in models)
    pl = dm.Planner(cfg, device=0, max_scenes=len(cases), max_obs_total=len(cases) * n_obs, order_cap=order_cap)
    try:
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
        pl.tick(sync=True)
        gout, plan, state = pl.get_grid_out(), pl.get_plan(), pl.get_state()
        _, _, dense = pl.search_info()
        assert dense == 0
        bad = []
        for s, (c, m) in enumerate(zip(cases, models)):
            rec, tag = gout[s], f"{name}[{s}] {c.name}"
            assert int(rec["status"]) == m["status"], (tag, int(rec["status"]), gm.STATUS_NAMES[m["status"]])
            bad += [f"{tag}.{f}: {int(rec[f])} vs model {m[f]}" for f in FIELDS if int(rec[f]) != m[f]]
            order = pl.get_order(s, m["n_expanded"]).tolist() if m["n_expanded"] else []
            path = pl.get_path(s, m["path_len"]).tolist() if m["path_len"] else []
            if order != m["order"]:
                bad.append(f"{tag}: expansion order differs from the model's")
            if path != m["path"]:
                bad.append(f"{tag}: path differs from the model's")
            bad += compare(gout[s:s + 1], gout_o[s:s + 1], tag + " grid") + compare(plan[s:s + 1], plan_o[s:s + 1], tag + " plan")
            bad += compare(state[s:s + 1], st_o[s:s + 1], tag + " state")
        assert not bad, "\n".join(bad[:20])
    finally:
        pl.close()


# ---- GPU: the step -----------------------------------------------------------------------------------------------------------
STEP_SCENES = 1600
STEP_FIRST = 2048           # generated scenes 2048 .. 3647: the densest needs 1,504 words, the tight budget is 1,600 (scenes 0 .. 1599: 1,507 and 1,664, where the step has nothing to give)


def _run_step(dm, cfg, sc, knob):
    old = os.environ.get("DMPP_CORESIDENT")
    if knob is None:
        os.environ.pop("DMPP_CORESIDENT", None)
    else:
        os.environ["DMPP_CORESIDENT"] = knob
    try:
        pl = dm.Planner(cfg, device=0, max_scenes=STEP_SCENES, max_obs_total=STEP_SCENES * 64)
    finally:
        if old is None:
            os.environ.pop("DMPP_CORESIDENT", None)
        else:
            os.environ["DMPP_CORESIDENT"] = old
    try:
        pl.set_scenes(sc)
        pl.set_state(sc["state"])
        infos = []
        for _ in range(4):
            pl.tick(sync=True)
            infos.append(pl.search_info())
        return pl.get_plan().tobytes(), pl.get_state().tobytes(), pl.get_grid_out().tobytes(), infos
    finally:
        pl.close()


@pytest.mark.gpu
def test_coresident_step_changes_the_budget_and_nothing_else(dm):
    lib = dm.load_library()
    i32 = ctypes.c_int32
    lib.pp_coresident_budget.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(i32)]
    cfg = dm.default_config(512, 512)
    sc = dm.gen_scenes(cfg, STEP_FIRST, STEP_SCENES, 64)
    on, off = _run_step(dm, cfg, sc, None), _run_step(dm, cfg, sc, "0")
    for what, a, b in zip(("PlanOut", "SceneState", "GridOut"), on[:3], off[:3]):
        assert a == b, f"{what} of tick 4 differs with the step on and off"
    print("search_info per tick (budget, need, dense): on", on[3], "off", off[3])
    assert all(i[2] == 0 for i in on[3] + off[3])
    # the budget reported is the exported function of the need reported and of the policy's budget, which is what the handle
    # without the step reports (the policy sees the same needs in both runs: the step's output never feeds it)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (b_on, need, _), (b_off, need_off, _) in zip(on[3], off[3]):
        assert need == need_off and need > 0
        out = i32()
        assert lib.pp_coresident_budget(7344, 4096, 8192, 8192, cus, STEP_SCENES, need, b_off, 0, ctypes.byref(out)) == 0
        assert b_on == out.value, (b_on, b_off, out.value, need)
    assert on[3][-1][0] < off[3][-1][0], "the step lowers the budget of this batch"
