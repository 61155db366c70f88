"""Phase timing of k_decision / k_planning (debug build: make -C .../csrc debug): cycle stamps per scene, alone on the GPU."""
import os, sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import dmpp_amd as dm
dm.load_library(os.environ.get("DMPP_LIB") or os.path.join(os.path.dirname(dm.LIB_PATH), 'libdmpp_dbg.so'))   # DMPP_LIB: another debug build
cfg = dm.default_config(512)
cfg["grid_stage"] = 0
n = 1024
n_obs = int(sys.argv[1]) if len(sys.argv) > 1 else 64          # obstacles per scene (the benchmark: 64; configs[3]: 256)
sc = dm.gen_scenes(cfg, 0, n, n_obs, 8)
pl = dm.Planner(cfg, max_scenes=n, max_obs_total=n * n_obs)
pl.set_scenes(sc); pl.set_state(sc['state'])
for _ in range(3):
    pl.tick(sync=True)
D, P, A, AP = [], [], [], []
for s in range(n):
    r = pl.get_refpath(s, 512)
    A.append([r["x"][483], r["y"][483], r["x"][484], r["y"][484], r["x"][485], r["y"][485]])     # in-order additions per corridor search
    AP.append(r["x"][493])                                                                        # ... of Planning's search
    D.append([r["x"][480], r["y"][480], r["x"][481], r["y"][481], r["x"][482], r["y"][482]])
    P.append([r["x"][490], r["y"][490], r["x"][491], r["y"][491], r["x"][492], r["y"][492]])
D, P, A, AP = np.array(D), np.array(P), np.array(A), np.array(AP)      # (A, AP: negative = the search took the second pass)
pos = sc["scene_in"]["loc"]["pos"]
attr = sc["scene_in"]["lanes"]["lanechg_attribute"]
for name, sel in (("road, no lane change", (pos == 0) & (attr == 0)), ("road, lane change allowed", (pos == 0) & (attr != 0)), ("junction", pos != 0)):
    print(name, int(sel.sum()), "scenes")
    print("  k_decision stamps (cycles): snapshot, LoadRefPath, AroundObstacle, sweep, rem-length, tree, end: median", np.median(D[sel], axis=0).astype(int).tolist())
    # (third tick, count != 0: loads and lengths of both | aim walk beside nearest point + remain, joined | aim finished, local state stored)
    print("  k_planning stamps (cycles): head, aim walk || localise, local state, path, SearchObstacle, end: median", np.median(P[sel], axis=0).astype(int).tolist())
    # (a build from before the deferred sum does not write these slots: it always adds n - 1 lengths per search)
    absA = np.abs(A)
    tot = absA[sel].sum(axis=1) if (pos[sel] == 0).all() else absA[sel][:, 0]
    print("  in-order additions: corridor F / junction path median %d max %d; all corridor searches of the scene median %d max %d; Planning median %d max %d"
          % (np.median(absA[sel][:, 0]), absA[sel][:, 0].max(), np.median(tot), tot.max(), np.median(np.abs(AP[sel])), np.abs(AP[sel]).max()))
print("searches that took the second pass (the whole sum): corridor searches / junction path in %d of %d scenes, Planning in %d of %d"
      % (int((A < 0).any(axis=1).sum()), n, int((AP < 0).sum()), n))
