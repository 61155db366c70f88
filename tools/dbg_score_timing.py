"""Phase timing of k_score (debug build: make -C .../csrc debug): cycle stamps of thread 0 of every scene, the kernels alone
on the GPU (one tick, host wait, next tick).
    python tools/dbg_score_timing.py [obstacles] [dynamic] [scenes]"""
import ctypes as C
import os
import sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import dmpp_amd as dm
lib = dm.load_library(os.environ.get("DMPP_LIB") or os.path.join(os.path.dirname(dm.LIB_PATH), 'libdmpp_dbg.so'))   # DMPP_LIB: another debug build
n_obs = int(sys.argv[1]) if len(sys.argv) > 1 else 64          # obstacles per scene (the benchmark: 64; configs[3]: 256)
dyn = int(sys.argv[2]) if len(sys.argv) > 2 else 0
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1024            # above 128 scenes: k_score<4>, up to 128: k_score<16>
cfg = dm.default_config(512)
cfg["dynamic_obstacles"] = dyn
cfg["force_replan"] = dyn
sc = dm.gen_scenes(cfg, 0, n, n_obs, 8)
pl = dm.Planner(cfg, max_scenes=n, max_obs_total=n * n_obs)
pl.set_scenes(sc); pl.set_state(sc['state'])
PH = 8
names = ["entry", "inputs landed", "set-up", "cull and buckets", "whole candidates", "packed pass", "left-over candidate", "winner and stores"]
buf = (C.c_uint * (n * PH))()
for t in range(4):
    pl.tick(sync=True)
    if lib.pp_debug_score_stamps(buf, n):
        raise SystemExit("pp_debug_score_stamps failed (not a debug build?)")
    st = np.frombuffer(buf, np.uint32).reshape(n, PH).astype(np.int64)
    d = np.diff(np.concatenate([np.zeros((n, 1), np.int64), st], axis=1), axis=1)      # cycles spent IN each phase
    print("tick %d, %d scenes x %d obstacles, dynamic %d: cycles per phase of k_score, thread 0 of each scene" % (t, n, n_obs, dyn))
    for k, name in enumerate(names):
        print("  %-20s median %7d  max %7d" % (name, int(np.median(d[:, k])), int(d[:, k].max())))
    print("  %-20s median %7d  max %7d" % ("total", int(np.median(st[:, PH - 1])), int(st[:, PH - 1].max())))
