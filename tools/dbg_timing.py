
import sys
sys.path.insert(0,'.'); sys.path.insert(0,'tests')
import os
import numpy as np, dmpp_amd as dm
dm.load_library(os.path.join(os.path.dirname(dm.LIB_PATH), os.environ.get('DMPP_DBG_LIB', 'libdmpp_dbg.so')))   # make -C .../csrc debug
cfg = dm.default_config(512)
n=1024
N_OBS = int(sys.argv[1]) if len(sys.argv) > 1 else 64
DYN = int(sys.argv[2]) if len(sys.argv) > 2 else 0
cfg["dynamic_obstacles"] = DYN; cfg["force_replan"] = DYN
sc = dm.gen_scenes(cfg, 0, n, N_OBS, 8)
pl = dm.Planner(cfg, max_scenes=n, max_obs_total=n*N_OBS)
pl.set_scenes(sc); pl.set_state(sc['state']); pl.tick(sync=True); pl.tick(sync=True)
g = pl.get_grid_out()
mp=int(cfg['max_path'][0])
rows=[]
setup=[]
tail=[]
for s in range(n):
    pp_=pl.get_path(s, mp)
    p=pp_[-16:]
    setup.append(pp_[-32:-24].tolist())
    tail.append([int(pp_[-64+6])]+pp_[-64+12:-64+16].tolist()+[int(p[10])])
    rows.append([int(g['n_expanded'][s]), int(g['n_pushed'][s])]+p[:16].tolist())
rows=np.array(rows)[g['status']==0]
names=['n_exp','n_push','iter','popped','jump_iters','diag_jobs','rounds','cyc_pop','cyc_closed','cyc_cand','cyc_jump','cyc_push','cyc_walk','cyc_search','cyc_setup','cyc_kernel','hw_id','xcc_id']
print(names, '(cycles/16)')
idx=np.argsort(-rows[:,15])[:6]
for i in idx: print(rows[i].tolist())
print('median', np.median(rows,axis=0).astype(int).tolist())
print('sum', rows.sum(axis=0).tolist())

hw = rows[:,16].astype(np.int64) & 0xFFFFFFFF
simd = (hw >> 4) & 3
print('searching waves per SIMD id:', np.bincount(simd, minlength=4).tolist(), ' wave slot ids:', np.bincount(hw & 15, minlength=16).tolist())

setup=np.array(setup)[g['status']==0]
print('setup phases (cycles) entry, clear, stage, pass1 (exact spans), offsets, zero, pass2 (OR), tail: median', np.median(setup,axis=0).astype(int).tolist(), 'max', setup.max(axis=0).tolist())

# the tail of search_core (behind the step loop), split by DBG_MARK 12 .. 15; cyc_walk above is their sum plus the remainder
tail=np.array(tail)[g['status']==0].astype(np.int64)
tnames=['hops','hash_pass','chain','path_cells','reductions','tail']
print('tail split', tnames, '(cycles, but hops)')
tc=tail*np.array([1,16,16,16,16,16])
print('  median', np.median(tc,axis=0).astype(int).tolist())
print('  max   ', tc.max(axis=0).tolist())
print('  sum   ', tc.sum(axis=0).tolist())
i=int(np.argmax(tc[:,0])); print('  the scene with the most hops', tc[i].tolist())
print('  search minus tail, summed (cycles):', int(16*(rows[:,13]-rows[:,12]).sum()))
