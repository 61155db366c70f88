#!/usr/bin/env python3
"""Runs ON THE GPU BOX: fleet coupling soak - random world partitions, K, range and seeds on the map store.
Per case: the byte-exact step check against tests/fleet_model.py after pp_set_fleet and after every advance, and the
open-loop equality (a fleet-less handle fed the traced SceneIn and obstacle pool plans the same PlanOut / GridOut / SceneState).
    python tests/soak_fleet.py [cases] [scenes] [ticks] [first seed] > profiles/r7_soak_fleet.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: see tests/conftest.py)
import dmpp_amd as dm
import fleet_model as fl
import map_scenes as ms
from test_fleet import _pool_of, _strided

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
ticks = int(sys.argv[3]) if len(sys.argv) > 3 else 10
seed0 = int(sys.argv[4]) if len(sys.argv) > 4 else 0
n_obs = 12
cfg = dm.default_config(128)
m = ms.build_map(dm, n_roads=5)
bad_cases = 0
for case in range(cases):
    rng = np.random.default_rng(seed0 + case)
    K = int(rng.choice([0, 1, 3, 8, 17, 64]))
    reach = float(rng.choice([0.5, 2.0, 3.0, 6.0, 60.0]))
    cuts = np.unique(rng.integers(1, n, int(rng.integers(0, 40))))
    wf = np.concatenate([[0], cuts, [n]]).astype(np.int32)
    sc = _strided(dm, ms.make_egos(dm, cfg, m, n, n_obs, seed=100 + seed0 + case), n, n_obs, K)
    fm = dm.default_fleet_model()
    fm["range"], fm["max_peers"] = reach, K
    caps = dict(max_scenes=n, max_obs_total=n * (n_obs + K), max_lane_pts_total=len(m["points"]), max_ref_pts_total=max(len(m["jpoints"]), 1))
    off, own = sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"]
    pls = []
    for k in range(2):
        pl = dm.Planner(cfg, device=0, **caps)
        pl.set_map(m), pl.set_egos(sc, with_motion=False), pl.set_state(sc["state"])
        pls.append(pl)
    a, b = pls
    a.set_fleet(wf, fm)
    model = dm.default_ego_model()
    step_bad = open_bad = 0
    hist = np.zeros(K + 1, np.int64)
    base = sc["obs_pool"]
    for t in range(ticks + 1):
        sin, pool, slices = _pool_of(a, n, base)
        want, wpool, _ = fl.couple(fm, wf, off, own, sin, base)
        step_bad += int(sin.tobytes() != want.tobytes())
        step_bad += sum(slices[s].tobytes() != wpool[int(off[s]):int(off[s]) + int(want["obs_n"][s])].tobytes() for s in range(n))
        hist += np.bincount(sin["obs_n"] - own, minlength=K + 1)
        keep = (dm.pinned_copy(sin), dm.pinned_copy(pool))
        b.update_async(*keep)
        a.tick(), b.tick()
        a.sync(), b.sync()
        for get in ("get_plan", "get_grid_out", "get_state"):
            open_bad += int(getattr(a, get)().tobytes() != getattr(b, get)().tobytes())
        if t < ticks:
            a.advance_async(model)
        base = pool
    a.close(), b.close()
    bad_cases += int(step_bad + open_bad > 0)
    print(f"case {seed0 + case}: {n} scenes, {len(wf) - 1} worlds, K {K}, range {reach} m, {ticks + 1} sets: step mismatches {step_bad}, "
          f"open-loop mismatches {open_bad}, peers per scene-set {hist.tolist()}", flush=True)
print(f"{cases} cases, {bad_cases} with a mismatch")
sys.exit(1 if bad_cases else 0)
