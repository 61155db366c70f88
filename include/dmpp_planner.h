/*
 * dmpp_planner.h — C-ABI of the MI355X planning engine (libdmpp.so).
 *
 * The reference has no plugin/FFI interface: its boundary is the C++ class surface of
 * CPlanning / CDecision (Planning.h:38-85, Decision.h:106-107), fed from an MFC
 * blackboard (Planning.cpp:95-112) and drained into it (Planning.cpp:186,214).  This
 * header is what a binding for that path binds instead: plain pointers
 * and sizes, POD structs from dmpp_types.h, int status codes, no C++ or torch types.
 * Every data pointer may be a host pointer or a HIP device pointer (copies use
 * hipMemcpyDefault).  A handle owns its GPU streams and all device scratch; calls on one
 * handle are serialised by the caller (the reference is one thread per module,
 * Planning.cpp:24-39).  All cross-tick state is the caller-visible SceneState.
 *
 * Return value: 0 = ok, negative = error (pp_last_error() has the text).  Nothing here
 * falls back to the CPU: without a usable GPU pp_create fails.
 */
#ifndef DMPP_PLANNER_H
#define DMPP_PLANNER_H

#include "dmpp_types.h"
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK            0
#define PP_ERR_ARG      -1
#define PP_ERR_HIP      -2
#define PP_ERR_CAPACITY -3
#define PP_ERR_STATE    -4

/* strides of the pools filled by pp_gen_scenes */
#define PP_GEN_LANE_PTS 320
#define PP_GEN_REF_PTS  128

typedef struct pp_planner* pp_handle;

typedef struct PlannerCaps {
    int32_t max_scenes;         /* scenes per batch */
    int32_t max_obs_total;      /* obstacle-pool entries */
    int32_t max_lane_pts_total; /* lane-pool points */
    int32_t max_ref_pts_total;  /* refpath-pool points */
    int32_t order_cap;          /* expansion-order cells kept per scene (0 = digest only) */
    int32_t _pad;
} PlannerCaps;

/* kernels of one tick, in launch order; index into pp_get_kernel_ms.  PP_K_PACK_PLAN / PP_K_PACK_GRID: the two pack kernels of
 * the packed streamed fetch (launched only while pp_set_packed_fetch is on); PP_K_PERCEIVE: k_perceive, launched in the place of the
 * snapshot kernel while pp_set_perception is on (PP_K_OBSTACLES counts nothing then) */
enum { PP_K_OBSTACLES = 0, PP_K_DECISION, PP_K_PLANNING, PP_K_SEARCH, PP_K_SCORE, PP_K_PACK_PLAN, PP_K_PACK_GRID, PP_K_PERCEIVE, PP_K_COUNT };
/* device buffers addressable through pp_device_ptr (for RCCL scatter/gather by the caller); PP_BUF_OBS_NOW: the last tick's
 * obstacle snapshot (max_obs_total records, only the slots some scene's slice covers are written); PP_BUF_OBS_SEEN: the perceived
 * snapshot of the same tick, same layout (NULL, 0 bytes on a handle that never called pp_set_perception) */
enum { PP_BUF_SCENE_IN = 0, PP_BUF_LANE_POOL, PP_BUF_REF_POOL, PP_BUF_OBS_POOL, PP_BUF_MOT_POOL, PP_BUF_STATE,
       PP_BUF_PLAN_OUT, PP_BUF_GRID_OUT, PP_BUF_GRID, PP_BUF_PATH, PP_BUF_ORDER, PP_BUF_LANE_ATTR, PP_BUF_OBS_NOW, PP_BUF_OBS_SEEN, PP_BUF_COUNT };

const char* pp_last_error(void);

/* ---- host-side helpers (no GPU needed) ------------------------------------------------ */
/* Values for every macro the reference leaves undefined + grid-engine defaults. */
void pp_default_config(PlannerConfig* cfg, int grid_w, int grid_h);
/* Zeroed state with the constructor values of Planning.cpp:10. */
void pp_init_state(SceneState* st, int lane_num);
/* Seeded synthetic scenes.  Pools must hold n*3*PP_GEN_LANE_PTS lane points (and as many
 * lane attribute bytes), n*PP_GEN_REF_PTS refpath points, n*n_obs obstacles
 * (lane_attr_pool/mot_pool/state may be NULL). */
int  pp_gen_scenes(const PlannerConfig* cfg, int first_scene, int n_scenes, int n_obs, int junction_every,
                   SceneIn* in, GlobalPoint3D* lane_pool, uint8_t* lane_attr_pool, GlobalPoint2D* ref_pool,
                   ObPoint* obs_pool, ObMotion* mot_pool, SceneState* state);

/* ---- lifetime -------------------------------------------------------------------------- */
/* Replaces CPlanning::Instance()/CDecision::Instance() + thread start (Planning.cpp:18-33). */
int  pp_create(const PlannerConfig* cfg, int device, const PlannerCaps* caps, pp_handle* out);
int  pp_destroy(pp_handle h);
int  pp_set_config(pp_handle h, const PlannerConfig* cfg);   /* grid size / caps may not grow */

/* ---- resident-data path ------------------------------------------------------------------
 * Replaces the blackboard reads of Planning.cpp:95-112 / Decision.cpp:155-160. */
/* lane_attr_pool[i] is decision_MapData[..][..][id].lanechg_attribute of lane point i (Decision.cpp:1179,1212):
 * one byte per lane-pool point, same indexing.  Required when cfg.lanechg_stage is 1. */
/* Every scene's slices (obs_off/obs_n, lanes.*_off/_n, ref_off/ref_n) are checked on the device against the pool
 * sizes given here; a slice outside its pool is PP_ERR_ARG and leaves no scenes resident (no kernel ever follows it). */
int  pp_set_scenes(pp_handle h, int n_scenes, const SceneIn* in,
                   const GlobalPoint3D* lane_pool, const uint8_t* lane_attr_pool, int n_lane_pts,
                   const GlobalPoint2D* ref_pool, int n_ref_pts,
                   const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total);
int  pp_set_state(pp_handle h, const SceneState* state, int n_scenes);
/* Map store: the whole map once, shared by every scene of the handle - replaces the
 * app->planning_MapData / planning_InterMapData members the threads index (Planning.cpp:331-356,
 * Decision.cpp:346-348,562-578).  Needs caps.max_lane_pts_total >= map->n_points and
 * caps.max_ref_pts_total >= map->n_jpoints.  Host or device pointers. */
int  pp_set_map(pp_handle h, const MapDesc* map);
/* Scenes on the resident map: SceneIn.lanes and SceneIn.ref_off / ref_n are IGNORED on input and derived on the
 * device from loc.road_num / lane_num / id[] (current, left, right lane; lane_sum; lanechg_attribute and
 * lane_width at the ego point) and from loc.last_roadnum / next_roadnum / last_lanenum / next_lanenum (the
 * junction polyline; none -> empty).  A road or lane outside the map is an error (the reference would index
 * out of its vectors). */
int  pp_set_egos(pp_handle h, int n_scenes, const SceneIn* in,
                 const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total);
/* The resident SceneIn records (after pp_set_egos: with the derived lane views; after pp_advance_async: the records it
 * produced for the next tick). */
int  pp_get_scene_in(pp_handle h, SceneIn* out, int n_scenes);

/* One Decision+Planning(+grid) tick for every resident scene: the bodies of
 * Decision.cpp:172-205 and Planning.cpp:114-223.  Asynchronous: the kernels of a tick run on several streams of the
 * handle (large batches: three chains side by side, consecutive ticks overlapping), so work a caller enqueues on
 * pp_stream(h) is NOT ordered after a tick by itself.  Every pp_get_* / pp_set_* call orders itself after all ticks
 * enqueued so far; for anything else on pp_stream(h) (an RCCL gather out of pp_device_ptr buffers) call pp_join first. */
int  pp_plan_tick(pp_handle h);
/* Makes pp_stream(h) wait, on the device, for every tick enqueued so far; returns at once (no host wait). */
int  pp_join(pp_handle h);
/* pp_join + host wait (and, once streamed ticks are in use, every staged update and download). */
int  pp_sync(pp_handle h);
/* pp_sync + hipDeviceSynchronize: every stream of the handle's device, the caller's included. */
int  pp_device_synchronize(pp_handle h);
/* Replaces SetPlanningStatus/SetUdpSendCtrl (Planning.cpp:186,214) and SetDecisionOut (Decision.cpp:203). */
int  pp_get_plan(pp_handle h, PlanOut* out, int n_scenes);
int  pp_get_state(pp_handle h, SceneState* state, int n_scenes);
int  pp_get_grid_out(pp_handle h, GridOut* out, int n_scenes);
int  pp_get_grid(pp_handle h, int scene, uint8_t* grid);                 /* grid_w*grid_h bytes, 0 free / 1 occupied: rasterised on demand from the last tick's obstacle snapshot by the search's own footprint code */
int  pp_get_order(pp_handle h, int scene, int32_t* order, int cap);      /* needs caps.order_cap > 0 */
int  pp_get_path(pp_handle h, int scene, int32_t* path, int cap);
/* DecisionOut.refpath published by the decision stage (Decision.cpp:195); PlanOut.dec.refpath_n points are valid */
int  pp_get_refpath(pp_handle h, int scene, GlobalPoint2D* pts, int cap);

/* ---- one-shot batch call (the SURVEY §8b signature): upload, tick, download ---------------- */
int  pp_plan_tick_batch(pp_handle h, int n_scenes, const SceneIn* in,
                        const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total,
                        const GlobalPoint3D* lane_pool, const uint8_t* lane_attr_pool, int n_lane_pts,
                        const GlobalPoint2D* ref_pool, int n_ref_pts,
                        SceneState* state_inout, PlanOut* out, GridOut* grid_out /* may be NULL */);

/* ---- streamed ticks: new inputs in, results out, every tick, with no host wait in between --------------------------
 * The reference reads obstacles / location / decision from its blackboard at the top of every tick (Planning.cpp:95-112,
 * Decision.cpp:155-160) and publishes at the end of it (Planning.cpp:186,214; Decision.cpp:203).  pp_set_* / pp_get_* do that
 * with a host wait each, which drains the pipeline of overlapping ticks; the calls below never wait on the host:
 *
 *     pp_update_async(h, n, in_t, obs_t, NULL, n_obs);     // snapshot of tick t (pinned host memory, or device memory)
 *     pp_plan_tick(h);
 *     pp_fetch_async(h, plan_t, grid_t, &id_t);            // into pinned host memory (or device memory)
 *     ... the same for t + 1, t + 2 ...                    // a few ticks deep
 *     pp_wait_tick(h, id_t, NULL);                         // plan_t / grid_t are complete; in_t / obs_t may be reused
 *
 * Inputs are ring-buffered on the device (the searches of three ticks are in flight behind the newest front chain), PlanOut
 * and GridOut too; uploads and downloads run on their own streams beside the kernels.  SceneState stays on the device.
 * Host buffers should come from pp_host_alloc (or be pinned with pp_host_register): copies from / to pageable memory work
 * but are staged by the runtime and wait on the host. */
/* Replaces the per-tick inputs of the resident scenes for the NEXT pp_plan_tick (and the ticks after it, until the next
 * update).  n_scenes must equal the resident count.  `in` NULL: SceneIn records carried over; obs_pool NULL: obstacles (and
 * motion) carried over; mot_pool NULL with an obs_pool: static obstacles.  After pp_set_scenes the SceneIn slices are the
 * caller's (lane and refpath pools stay resident); after pp_set_egos they are derived from the resident map as there.
 * Nothing is refused asynchronously: a scene whose slices fall outside their pools (or whose road / lane is off the map) is
 * POISONED - it runs that tick with empty lanes, refpath and obstacles - and pp_wait_tick reports how many there were.
 * The source buffers must stay untouched until pp_wait_tick of the tick that adopts them (or pp_sync) has returned. */
int  pp_update_async(pp_handle h, int n_scenes, const SceneIn* in, const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total);
/* Downloads PlanOut and / or GridOut (either may be NULL) of the LAST enqueued tick, ordered after that tick's kernels only:
 * PlanOut as soon as its Planning kernel has finished, GridOut after its scoring pass.  *tick_id (may be NULL) names the tick
 * for pp_wait_tick.  The device copies are overwritten 12 ticks later, which those ticks order
 * themselves after - the destination buffers are the caller's to rotate. */
int  pp_fetch_async(pp_handle h, PlanOut* plan, GridOut* grid, long long* tick_id);
/* The same for only what the reference publishes on every tick - PlanningOut (SetUdpSendCtrl, Planning.cpp:214) and
 * PlanningStatus (SetPlanningStatus, Planning.cpp:186) of every scene, as two contiguous arrays (strided copies out of the
 * PlanOut records: 3.3 of their 6.9 KB) - and / or GridOut.  Any of the three may be NULL. */
int  pp_fetch_published_async(pp_handle h, PlanningOut* result, PlanningStatus* show, GridOut* grid, long long* tick_id);
/* ---- packed streamed fetch ----------------------------------------------------------------------------------
 * pp_set_packed_fetch(h, 1) arms the handle: it becomes a streamed one (ticks in groups of 1, as after the first pp_fetch_async),
 * allocates one PackedPlan set per PlanOut set and one PackedGrid set per GridOut group position, and from the next tick on every
 * pp_plan_tick launches k_pack_plan behind its Planning kernel and - with the grid stage on - k_pack_grid behind its scoring pass,
 * in stream order (no event, no wait).  pp_set_packed_fetch(h, 0) disarms: the sets stay allocated, nothing more is launched.  It is no
 * rollout feature: no set call retires it, and it survives pp_set_scenes / pp_set_egos / pp_set_n_scenes / pp_set_config.  A handle
 * that never arms allocates and launches nothing.
 * pp_fetch_packed_async downloads the packed records of the LAST enqueued tick (either pointer may be NULL): 1744 + 248 B per scene
 * in the place of the 6896 + 3792 B of pp_fetch_async.  Same ordering rules, same pp_wait_tick.  Several requests - of any of the
 * three fetch calls - may name one tick: all return its id, every destination a call accepted is filled, and pp_wait_tick of that id
 * covers all of them.  PP_ERR_STATE: not armed; the last tick ran before arming; `grid` with the grid stage off.  PP_ERR_ARG: both
 * pointers NULL.
 * pp_unpack_plan / pp_unpack_grid: pure host code, no handle, no device, built from the kernels' own functions - they rebuild
 * PlanningOut (pnts through the WGS84 line of cfg), PlanningStatus, DecisionOutPod (each output may be NULL) and GridOut, equal in
 * every byte to what pp_fetch_async of the same tick delivers, except GridOut.cand_*[k] for k != best_candidate, which are 0.
 * cfg: the configuration the tick ran with.  A hostile record - n_steps outside 0 .. 199, an unknown kind, DMPP_PACKED_BAD, a
 * best_candidate outside 0 .. 16, a walk that leaves grid_w x grid_h - leaves that scene's GridOut zeroed; the call goes on with the
 * other scenes and returns PP_ERR_ARG.  Neither reads or writes outside its arrays, whatever a record holds. */
int  pp_set_packed_fetch(pp_handle h, int on);
int  pp_fetch_packed_async(pp_handle h, PackedPlan* plan, PackedGrid* grid, long long* tick_id);
int  pp_unpack_plan(const PlannerConfig* cfg, const PackedPlan* in, int n, PlanningOut* result, PlanningStatus* show, DecisionOutPod* dec);
int  pp_unpack_grid(const PlannerConfig* cfg, const PackedGrid* in, int n, GridOut* out);
/* Host wait for the downloads of one tick (at most 32 ticks back).  *n_poisoned (may be NULL): scenes of that tick's update
 * that were poisoned; PP_ERR_ARG when there were any (the other scenes' results are valid), PP_OK otherwise. */
int  pp_wait_tick(pp_handle h, long long tick_id, int* n_poisoned);
long long pp_tick_id(pp_handle h);                   /* ticks enqueued on this handle so far = the id of the last one */
/* Pinned host memory for the buffers above (hipHostMalloc / hipHostRegister). */
void* pp_host_alloc(size_t bytes);
void  pp_host_free(void* p);
int   pp_host_register(void* p, size_t bytes);
int   pp_host_unregister(void* p);

/* ---- closed-loop rollout: every ego follows its own plan, on the device -----------------------------------
 * pp_advance_async is a DEVICE-GENERATED update: it does what pp_update_async(h, n, in, NULL, NULL, 0) does, except that the
 * SceneIn records of the next tick are produced by one kernel on the upload stream (k_advance_egos) from the SceneIn, PlanOut
 * and SceneState of the last tick - speed towards result.desspd (or along result.desacc) within the model's limits, position
 * and heading along PlanOut.road_points from SceneState.path_near_id, the three lane ids of loc.id[] by a windowed nearest-
 * point search, and (egos on a resident map only) the lane number.  Obstacles and motion are carried over; the lane views are
 * derived again (pp_set_egos) and the slices checked (poisoning) as after any update.  After pp_set_scenes lane_num is HELD:
 * the caller's three lane slices cannot be rotated, so a lane change is only followed after pp_set_egos.  Road and junction
 * transitions belong to a localisation module and are out of scope: an ego that nears the end of its lane is flagged
 * (DMPP_EGO_*) and FROZEN - later advances carry its SceneIn over unchanged, it still ticks, its flags are sticky until the
 * next pp_set_scenes / pp_set_egos / pp_set_n_scenes (or, with pp_set_episodes, until the ego restarts: DESIGN.md §4k).
 * It waits - on the device - for the Planning kernel of the last tick only, never for its search, and never on the host.
 * PP_ERR_STATE: no tick enqueued since the scenes were set, or an update already staged for the next tick (a pp_update_async
 * with SceneIn records on top of a staged advance is PP_ERR_STATE too; an obstacles-only one is fine).
 * trace (may be NULL; device or pinned host memory, n records): the egos the next tick plans from, written by the kernel. */
void pp_default_ego_model(EgoModel* m);              /* dt 0.1 s, max_acc 2 m/s^2, max_dec 4 m/s^2, window 32 points */
int  pp_advance_async(pp_handle h, const EgoModel* m, EgoTrace* trace);
/* n_ticks times (pp_advance_async, pp_plan_tick) with no host wait, after one initial tick if none has run since the scenes
 * were set.  trace (may be NULL): n_ticks * n records, row t = the egos of the t-th tick enqueued here.  *last_tick_id (may be
 * NULL): the id of the last tick, for pp_fetch_async / pp_wait_tick.  Rollout ticks are streamed ticks (tick groups of 1). */
int  pp_rollout(pp_handle h, int n_ticks, const EgoModel* m, EgoTrace* trace, long long* last_tick_id);
/* The DMPP_EGO_* flag words after the last advance (all zero on a handle that never advanced).  Host wait. */
int  pp_get_ego_flags(pp_handle h, int32_t* flags, int n_scenes);

/* ---- rollout scorecard: per-scene safety and progress totals kept on the device -----------------------------------
 * Between pp_score_begin and pp_score_end EVERY pp_plan_tick is scored exactly once - rollout ticks, ticks fed by pp_update_async
 * and ticks on unchanged inputs alike - into one RolloutScore record per scene: two small kernels per tick (k_score_ego behind the
 * tick's Planning kernel on the upload stream, k_score_grid behind its scoring pass), no host wait, nothing downloaded.  Scored
 * ticks are streamed ticks (tick groups of 1, like rollout ticks; the handle stays in that mode afterwards, as after any streamed
 * call).  A handle that never calls pp_score_begin allocates and launches none of this.
 * pp_score_begin: allocates on first use, sets every record to its starting values (a second call restarts the totals) and turns
 * scoring on (one host wait).  dt_score: seconds between ticks, the divisor of max_acc / max_dec; finite and > 0, else PP_ERR_ARG.
 * pp_set_scenes / pp_set_egos / pp_set_n_scenes while scoring is on restart the totals, as they clear the ego flags.
 * pp_score_end: scoring off; the records stay readable and later ticks leave them alone.
 * pp_get_rollout_score: the records of the first n_scenes scenes into host memory, the last enqueued tick included.  Host wait.
 * PP_ERR_STATE on a handle that never began. */
int  pp_score_begin(pp_handle h, double dt_score);
int  pp_score_end(pp_handle h);
int  pp_get_rollout_score(pp_handle h, RolloutScore* out, int n_scenes);

/* ---- score trace: the last scored ticks of every scene, frozen on an incident ---------------------------------------
 * The scorecard says THAT scene 713 first collided at scored tick 4180; the trace says what happened before.  pp_set_score_trace gives
 * every scene a ring of m->depth ScoreTick records (64 B) and a ScoreTraceInfo header on the device.  While it AND the scorecard are on,
 * k_score_ego stores one record per scene and scored tick - the ego, its clearance and the obstacle that gave it, the flag word, the
 * plan's behaviour and counters, the causes the tick met - and a ring whose tick meets a cause of m->trigger takes m->post more ticks
 * and freezes: the approach is still there when the host comes to read it.  trigger 0: a plain ring that never freezes.  One more
 * 64-byte store per scene and tick in a kernel that already runs; no kernel, no launch and no host wait is added.
 * It belongs to the scorecard's life cycle and is no rollout feature: no set call retires it, and what restarts the totals -
 * pp_score_begin, pp_set_scenes / pp_set_egos / pp_set_n_scenes while scoring is on - puts the headers of a recorder that is on back
 * to their starting values (armed, n_written 0).  An episode restart does not touch it: k runs on and the tick behind the restart
 * carries DMPP_TICK_START.
 * pp_default_score_trace: depth 64, post 8, trigger DMPP_TRACE_COLLISION, flag_mask 0, near 0.5 m, brake 6 m/s^2.
 * pp_set_score_trace: legal before or after pp_score_begin.  Allocates caps.max_scenes * depth records and the headers, sets every
 * header to its starting values (a second call starts again) and turns the recorder on; one host wait, behind every tick and advance
 * enqueued so far.  m == NULL: the recorder off; rings and headers stay readable and no longer change.  PP_ERR_ARG, with nothing
 * changed: depth outside 1 .. DMPP_SCORE_TRACE_MAX, post outside 0 .. depth - 1, bits outside 15 in trigger or outside 31 in flag_mask,
 * a near that is not finite, a brake that is not finite and > 0.  A handle that never makes the call allocates and launches
 * exactly what it did without it.
 * pp_get_score_trace_info: the headers of the first n_scenes scenes, the last enqueued tick included; waits as pp_get_rollout_score.
 * pp_read_score_trace: the records of one scene's ring, min(n_written, depth) of them, oldest first (at most two copies), and - info
 * may be NULL - the header they were read under; returns their number (>= 0; an error code is negative).  PP_ERR_CAPACITY when cap is
 * smaller than that number, PP_ERR_ARG for a scene outside the resident ones; nothing changes on either.  rearm != 0: the header goes
 * back to armed (state 0, trigger_k -1, trigger 0, post_left 0) behind the read; the ring and n_written stay, so the next incident
 * keeps its lead-in.  Both reads: PP_ERR_STATE on a handle that never made the set call. */
void pp_default_score_trace(ScoreTraceModel* m);
int  pp_set_score_trace(pp_handle h, const ScoreTraceModel* m);
int  pp_get_score_trace_info(pp_handle h, ScoreTraceInfo* out, int n_scenes);
int  pp_read_score_trace(pp_handle h, int scene, ScoreTick* out, int cap, ScoreTraceInfo* info, int rearm);

/* ---- conflict score: time to collision and braking demand per scene -------------------------------------------------
 * The scorecard judges a run by disc clearance alone: it cannot tell an ego that passed a parked car at 0.4 m from one that was 0.4 s
 * from a head-on hit.  pp_set_conflict_score keeps the obstacle snapshot of the scored tick before on the device.  While it AND the
 * scorecard are on, k_score_ego gives every entry of the scene's slice a velocity by differencing the two snapshots - per-scene traffic,
 * world traffic, peers, moving own obstacles and plain pp_update_async feeds alike, no producer of obstacles changes - and the ego one by
 * differencing its own positions, and folds the smallest time to collision t* of the tick and the largest braking demand into one
 * ConflictScore record per scene: the minimum, where and against what, the warn and critical ticks, the time-integrated TTC.  An entry
 * whose slot changed hands (another type or radius, a moved or grown slice, a jump above v_max * dt_score) and an ego that restarted
 * have one tick without a velocity, never a wrong one.  No kernel, no launch and no host wait is added to a tick.
 * Like the score trace it belongs to the scorecard's life cycle and is no rollout feature: no set call retires it, and what restarts
 * the totals - pp_score_begin, pp_set_scenes / pp_set_egos / pp_set_n_scenes while scoring is on - puts the records of a step that is
 * on back to their starting values.
 * pp_default_conflict: ttc_warn 3 s, ttc_crit 1.5 s, v_max 70 m/s, min_closing 0.
 * pp_set_conflict_score: legal before or after pp_score_begin.  Allocates caps.max_scenes records and the previous-snapshot buffers
 * (two of caps.max_obs_total ObPoint: one is read while the other is written), sets every record to its starting values (a second
 * call starts again) and turns the step on; one host wait, behind every tick and advance enqueued so far.  m == NULL: the step off;
 * the records stay readable and no longer change.  PP_ERR_ARG, with nothing changed: a field that is not finite, ttc_warn, ttc_crit or
 * v_max not > 0, ttc_crit > ttc_warn, min_closing < 0.  A handle that never makes the call allocates and launches exactly what it did
 * without it.
 * pp_get_conflict_score: the records of the first n_scenes scenes, the last enqueued tick included; waits as pp_get_rollout_score.
 * PP_ERR_STATE on a handle that never made the set call. */
void pp_default_conflict(ConflictModel* m);
int  pp_set_conflict_score(pp_handle h, const ConflictModel* m);
int  pp_get_conflict_score(pp_handle h, ConflictScore* out, int n_scenes);

/* ---- perception model: the planner sees what a sensor would -------------------------------------------------------------
 * Without it the planner is handed the obstacle snapshot as it is: every entry from the first tick, exact, through other vehicles, behind
 * the ego and at any distance.  While a model is set, ONE kernel, k_perceive, takes the place of the snapshot kernel on every tick of the
 * handle - plain ticks, tick groups, streamed ticks, rollout ticks, pp_tick_io.  It stores the truth snapshot as before and, beside it, a
 * PERCEIVED snapshot of the same layout: per entry in view (range, field of view about the ego's heading), not occluded (the sight line
 * to its centre clears the disc of every nearer entry of the slice), not missed (a hash of seed, scene, entry and tick id against
 * p_miss), then through a track per pool entry that reports only after `confirm` + 1 detections in a row, adds position noise that
 * grows with distance, and coasts on its last report through `coast` missing ticks.  Decision, Planning, the search, its scoring pass
 * and pp_get_grid read the perceived snapshot; the scorecard, the score trace, the conflict score, PP_BUF_OBS_NOW, the episode and
 * traffic kernels keep the truth.  Entry j of the perceived slice is entry j of the truth (PlanOut.ob, around[] and min_clearance_obs
 * name the same object); an unseen entry is the hidden record { 1e12, 1e12, type, 0 }, which no stage of the tick reacts to.
 * The model belongs to the handle like the ego tracker: no rollout feature, no set call retires it.  PerceptionStats counts per scene
 * the entry-ticks by cause and by output, and keeps the closest thing the planner did not see.
 * pp_default_perception: range 60 m, cos_half_fov cos 60 deg, sigma0 0.1 m, sigma_gain 0.005, p_miss 2 % of 2^32, seed 1, occlusion on,
 * confirm 2, coast 3 - a starting point, not tuned values.
 * pp_set_perception: allocates the perceived ring, caps.max_obs_total tracks and caps.max_scenes stats at the first call, restarts
 * tracks and stats at every call, one host wait behind every tick and advance enqueued so far.  m == NULL: off, the next tick runs
 * exactly the kernels of a handle that never made the call; tracks and stats stay readable.  PP_ERR_ARG, with nothing changed:
 * !(range > 0), cos_half_fov outside [-1, 1], sigma0 / sigma_gain not finite or < 0, occlusion not 0 | 1, confirm or coast outside
 * 0 .. 255, _pad != 0.  Legal while an update or an advance is staged (the call reads nothing of the resident set: the staged tick is the
 * first one perceived).  Every call that replaces the resident scenes or moves
 * slices - pp_set_scenes, pp_set_egos, pp_set_n_scenes, pp_set_fleet, pp_set_traffic, pp_set_world_traffic (with or without actors) - restarts
 * tracks and stats, also while the model is switched off.  The set call starts the perceived ring as a copy of the truth ring.
 * pp_get_perception_stats: the records of the first n_scenes scenes, the last enqueued tick included (host wait).
 * pp_get_perception_tracks: n tracks from pool entry `first` on.  Both: PP_ERR_STATE on a handle that never made the set call. */
void pp_default_perception(PerceptionModel* m);
int  pp_set_perception(pp_handle h, const PerceptionModel* m);
int  pp_get_perception_stats(pp_handle h, PerceptionStats* out, int n_scenes);
int  pp_get_perception_tracks(pp_handle h, PerceptTrack* out, int first, int n);

/* ---- fleet coupling: the egos of one world see each other during a rollout -----------------------------------
 * pp_set_fleet groups the resident scenes into WORLDS: world w is the contiguous run of scenes [world_first[w], world_first[w+1]);
 * world_first has n_worlds + 1 entries, starts at 0, ends at the resident scene count and is strictly increasing (host pointer).
 * From then on every input set that is staged - by pp_advance_async, by pp_update_async - passes through one more kernel on the
 * upload stream (k_couple_fleet) that writes, behind every scene's own obstacles, the K = fm->max_peers nearest egos of its world
 * within fm->range (squared distance <= range * range, ties to the lower scene index) at the poses of that set, as
 * ObPoint { x, y, type = DMPP_OB_PEER | peer scene, radius = fm->radius } with zero ObMotion, and sets obs_n = own + peers found.
 * Decision, Planning, search, scoring and the scorecard read the obstacle list and so react to peers with no change.
 * The call PINS every scene's obstacle slice: (obs_off, n_own = obs_n) of the resident records are recorded and the K pool entries
 * [obs_off + n_own, obs_off + n_own + K) are the scene's peer slots; obs_off / obs_n of SceneIn records uploaded later are
 * overwritten by the pinned values, and an obstacle pool uploaded later must leave the peer slots free.  Such a pool must also
 * cover every scene's own entries: one that ends before them is PP_ERR_ARG from pp_update_async (the device's slice check
 * runs against the end of the peer slots and would not see it).  The used size of the
 * obstacle pool grows to the largest slot end.  Checked on the host, with nothing changed on failure: every extended slice
 * [obs_off, obs_off + n_own + K) inside caps.max_obs_total (PP_ERR_CAPACITY) and disjoint from every other, 0 <= K <=
 * DMPP_FLEET_MAX_PEERS, range finite and > 0, radius finite and >= 0, world_first as above (PP_ERR_ARG); no resident scenes or an
 * update staged for the next tick: PP_ERR_STATE.  The resident set is coupled inside the call (the next tick sees the peers); one
 * host wait.  n_worlds = 0 (pointers may be NULL): fleet off, the resident records get their own slices back.  pp_set_scenes /
 * pp_set_egos / pp_set_n_scenes switch the fleet off too (every such rule in one table: DESIGN.md §7, "Feature life cycle").
 * A handle that never calls pp_set_fleet allocates and launches none of this.  Peers have no velocity and no orientation; a world lives on one handle.  A scene that an earlier streamed update POISONED
 * carries obs_off = 0, obs_n = 0: its peer slots would be [0, K), which collide with the slice of whichever scene owns the start
 * of the pool, and the call is refused with the overlap message - set good scenes first. */
void pp_default_fleet_model(FleetModel* fm);         /* range 60 m, radius half the default Vehicle_Width, 8 peers */
int  pp_set_fleet(pp_handle h, int n_worlds, const int32_t* world_first, const FleetModel* fm);
/* The obstacle slice of one scene - its own entries, then the peers - of the input set pp_get_scene_in reads (the staged one after
 * an advance).  At most cap entries are written; returns obs_n (>= 0), or a negative error.  A debugging read-back, not for
 * per-tick use: two small copies with a host wait each, and it drains the pipeline of overlapping ticks like every pp_get_*.
 * Only the obs_n entries the tick reads are returned: peer slots beyond them (left as they are) are not. */
int  pp_get_obstacles(pp_handle h, int scene, ObPoint* out, int cap);

/* ---- route following: rollout egos cross junctions onto the next road -----------------------------------------
 * pp_set_route gives every resident scene a ROUTE: the legs [route_first[s], route_first[s+1]) of `legs` (host pointers;
 * route_first has n_scenes + 1 entries, starts at 0, ends at n_legs_total and never decreases; an empty run leaves the scene
 * unrouted).  loc.path_num is the 0-based index of the ego's current leg within its own route.  From then on pp_advance_async
 * runs the routed form of its kernel (k_advance_route): an unfrozen scene with a route and 0 <= path_num < its leg count is moved
 * road -> pre-junction (pos 1, from rm->pre_points lane points before the end of its lane, when the map has a junction from its
 * lane to the next leg's road) -> junction (pos 2, on the last lane point) -> next road (pos 0, at the end of the polyline;
 * path_num, out_lane_no and stub_attribute become those of the next leg), and the lane end only freezes an ego that has no
 * junction to take: DMPP_EGO_LANE_END alone when it missed its exit lane, DMPP_EGO_LANE_END | DMPP_EGO_ROUTE_END on the last leg.
 * Every other scene advances as before.  The resident records are not touched: the first tick reads what the caller uploaded.
 * PP_ERR_STATE: the scenes are not resident from pp_set_map + pp_set_egos, there are none, or an update is staged for the next
 * tick.  PP_ERR_ARG: a bad route_first, a road_num outside the map, pre_points < 0.  Nothing changes on these.  (A device error
 * during the upload itself, PP_ERR_HIP, leaves routing off: never half a route.)  One host wait.
 * n_legs_total = 0 (pointers may be NULL): routing off; pp_set_scenes / pp_set_egos / pp_set_n_scenes / pp_set_map switch it off
 * too (§7, "Feature life cycle").  A handle that never calls pp_set_route allocates and launches none of this. */
int  pp_default_route_model(RouteModel* rm);         /* pre_points 60: 30 m of 0.5 m points */
int  pp_set_route(pp_handle h, int n_legs_total, const RouteLeg* legs, const int32_t* route_first, const RouteModel* rm);

/* ---- a grid that follows the ego: the advance step re-centres grid and goal ------------------------------------
 * Without it SceneIn.grid_origin and SceneIn.goal are carried over by every advance, and an ego that runs the grid stage leaves the
 * caller's grid after a few dozen metres (DMPP_EGO_OFF_GRID, frozen).  pp_set_grid_follow switches following on: every advance
 * (k_advance_egos and k_advance_route alike) then gives a scene that entered it unfrozen and did not get BAD_PATH
 *     goal        = PlanOut.road_points[gf->goal_point] of the plan it followed (skipped for a non-finite point), and
 *     grid_origin = the old one while ego and goal both lie at least gf->margin_cells cells inside the grid, otherwise
 *                   (floor(m / cell) - W / 2) * cell per axis, m the midpoint of ego and goal: a whole number of cells,
 * and tests DMPP_EGO_OFF_GRID against the new frame.  Every bit of the eight words is specified (§4g).  Nothing else of the record
 * changes; frozen scenes keep their frame; records that arrive through pp_update_async are the caller's and are not touched.
 * The model belongs to the HANDLE and holds no per-scene data: it survives pp_set_scenes / pp_set_egos / pp_set_n_scenes /
 * pp_set_map (unlike the fleet and the routes) and takes effect from the next pp_advance_async on, a staged update or not.
 * gf == NULL: following off - the advance is then the one of a handle that never set it, byte for byte.
 * PP_ERR_ARG, with nothing changed: goal_point outside 1 .. DMPP_PATH_POINTS - 1, margin_cells < 0, or
 * 2 * margin_cells >= min(grid_w, grid_h) of the handle's configuration (pp_set_config refuses, with PP_ERR_ARG, a grid the
 * margin of a model that is switched on no longer fits).  Legal with grid_stage = 0: the frame is maintained, nothing reads
 * it, and there is no OFF_GRID test.  No device work, no host wait. */
void pp_default_grid_follow(GridFollow* gf);         /* goal_point 199 (the end of the planned path), margin_cells 32 (8 m at 0.25 m) */
int  pp_set_grid_follow(pp_handle h, const GridFollow* gf);

/* ---- ego tracking model: rollout egos steer a bicycle model along the plan -------------------------------------
 * Without it every advance puts the ego ON point k0 of its planned path and walks s metres along it (§4c 3.): the lateral error
 * is dropped, and the planner's replan causes 2 (|path_lat_dis| > 0.2 m) and 3 (|path_dir_err| > 45 deg) can never occur in a
 * rollout.  pp_set_ego_tracker gives every ego a pose of its own: one EgoTrackState per scene (unit heading, curvature) is kept on
 * the device, and every advance (k_advance_egos<true> / k_advance_route<true>) steers towards the path point
 * ld = look_min + look_gain * v' / 3.6 metres ahead of k0 by pure pursuit in curvature - clamped to +-max_curv, rate-limited by
 * curv_rate * dt, curv_bias added - and moves the ego s metres from where it STANDS in n_sub substeps.  Speed, distance and
 * everything behind the pose (ids, lane number, route step, grid follow, flags, trace) are unchanged.  Every bit of EgoTrackState
 * and of the staged x, y, velocity is specified (§4q); dir is GetRoadAngle of the heading vector.
 * A state is re-derived (kappa 0, heading from loc.globalpoint.dir, n_init + 1) when it is not valid, when the pose bits of the
 * record the advance reads are not the ones this model stored last (pp_update_async, pp_tick_io, a respawn), or - episodes on -
 * when EpisodeStats.age is 0.  The model belongs to the HANDLE, like GridFollow: no rollout feature bit, no set call retires it,
 * it survives pp_set_scenes / pp_set_egos / pp_set_n_scenes / pp_set_map (which clear the per-scene states).  It takes effect
 * from the next pp_advance_async.  tk == NULL: off - the advance is then the one of a handle that never set it, byte for byte;
 * the states stay as they are and stay readable (switched on again, a state whose ego moved meanwhile is re-derived by the key
 * rule).  The states are allocated and zeroed by the first successful call with a model (one host wait, that call only; every
 * other call does no device work); a handle that never calls it allocates and launches nothing new.
 * PP_ERR_ARG, with nothing changed: a non-finite field, look_min <= 0, look_gain < 0, max_curv <= 0, curv_rate <= 0, n_sub
 * outside 1 .. 8.
 * pp_get_ego_track_state: the states of the first n scenes, a staged advance included (host wait, as pp_get_ego_flags);
 * PP_ERR_STATE when the tracker was never set on this handle. */
void pp_default_ego_tracker(EgoTracker* tk);         /* look_min 3 m, look_gain 0.5 s, max_curv 0.2, curv_rate 0.3, bias 0, n_sub 2 */
int  pp_set_ego_tracker(pp_handle h, const EgoTracker* tk);
int  pp_get_ego_track_state(pp_handle h, EgoTrackState* out, int n);

/* ---- lane traffic: scripted vehicles that drive the map during a rollout ------------------------------------------
 * pp_set_traffic gives the handle n_tracks TRACKS (polylines: slices of `points`, host pointers; a closed track has one more
 * segment from its last point back to its first) and n_actors ACTORS.  Actor a drives tracks[a.track] at a.speed m/s from arc
 * length a.s0 and owns entry a.slot of scene a.scene's OWN obstacle entries.  From then on every input set that is staged passes
 * through one more kernel on the upload stream (k_move_traffic, one thread per actor) that writes
 * ObPoint { x, y, a.type, a.radius } - the point at arc length s of the track - into that entry, with zero ObMotion when the set
 * carries a motion pool: pp_advance_async steps s by speed * EgoModel.dt first (an open track clamps at its ends, a closed one
 * wraps), pp_update_async places the actors at the current s.  The resident set is placed inside the call: the next tick sees the
 * traffic.  Decision, Planning, search, scoring and the scorecard read the obstacle list and so react with no change; SceneIn is
 * never written.  Every arithmetic step is specified (§4h): a numpy restatement gives the same bytes.
 * The call PINS every actor's pool entry, obs_off[scene] + slot of the resident records: SceneIn records uploaded later must keep
 * the slices, and an obstacle pool uploaded later must cover every pinned entry (else PP_ERR_ARG from pp_update_async; whatever it
 * holds in those entries is overwritten).  pp_set_fleet and pp_set_traffic may be called in either order: the fleet only adds
 * slots behind a scene's own entries.
 * Checked on the host, with nothing changed on failure.  PP_ERR_STATE: no resident scenes, or an update staged for the next tick.
 * PP_ERR_ARG: a track slice outside `points` or with n_points < 2, a non-finite point, a closed track whose length is not > 0;
 * a non-finite s0 or speed, a radius that is not finite or is negative, a scene or track out of range, a slot outside the scene's
 * own entries (the resident obs_n, or - fleet set - the pinned n_own), two actors on one (scene, slot).  One host wait.
 * n_actors = 0 (pointers may be NULL): traffic off - the entries keep the last pose written and are plain obstacles again.
 * pp_set_scenes / pp_set_egos / pp_set_n_scenes switch it off too; pp_set_map and pp_set_config do not (§7, "Feature life cycle").  A handle that never calls
 * pp_set_traffic allocates and launches none of this. */
int  pp_set_traffic(pp_handle h, int n_tracks, const TrafficTrack* tracks, const GlobalPoint2D* points, int n_points,
                    int n_actors, const TrafficActor* actors);
/* The arc length of actors 0 .. n - 1 in the input set pp_get_scene_in reads (the staged one after an advance).  Host wait.
 * PP_ERR_STATE while traffic is off. */
int  pp_get_traffic_state(pp_handle h, double* s, int n);

/* ---- car-following traffic: actors keep a gap to the ego and to each other ---------------------------------------
 * Without it an actor drives its track at a constant speed whatever is in front of it.  pp_set_traffic_follow switches a
 * deterministic car-following law on: while traffic is set, pp_advance_async launches k_follow_traffic (one wave per actor) in the
 * place of k_move_traffic.  Every actor carries a speed v beside its arc length s; an actor with speed > 0 takes speed as its
 * desired speed, looks tf->look metres ahead along its track for the nearest actor of its own scene on the same track and for
 * its scene's ego (the ego counts when it lies within tf->lateral of the nearest track vertex of that window), and accelerates by
 * the intelligent-driver model, clamped at -max_dec; v never goes below 0.  An actor with speed <= 0 steps as before.  The step is
 * a Jacobi step: every actor reads the s and v all actors had before the advance, and the ego pose the advance has just staged.
 * Every arithmetic step is specified (§4i): a numpy restatement gives the same bytes.
 * v is set to the actors' speed by pp_set_traffic while following is on and by pp_set_traffic_follow(non-NULL) while traffic is
 * on; pp_update_async leaves it alone.  The model belongs to the handle: it survives pp_set_scenes / pp_set_egos /
 * pp_set_n_scenes / pp_set_map / pp_set_config and takes effect only while traffic is on.  tf NULL: off (the actors go on at
 * their constant speed from where they are).  A handle that never switches it on allocates and launches none of this.
 * PP_ERR_ARG (nothing changes): a field that is not finite; look, gap, max_acc, comfort_dec, max_dec or min_net not > 0; lateral
 * or headway < 0.  PP_ERR_STATE: an update is staged for the next tick.  One host wait while traffic is on, none otherwise. */
void pp_default_traffic_follow(TrafficFollow* tf);   /* { 60, 1.5, 2, 1.5, 1, 2, 6, 0.1 } */
int  pp_set_traffic_follow(pp_handle h, const TrafficFollow* tf);
/* The speed of actors 0 .. n - 1, as pp_get_traffic_state gives their arc length (same set, same wait).  PP_ERR_STATE while
 * traffic or following is off. */
int  pp_get_traffic_speed(pp_handle h, double* v, int n);

/* ---- world traffic: one vehicle per world, seen by and seeing every ego of it --------------------------------------
 * pp_set_traffic gives a vehicle to ONE scene: a world of W scenes (pp_set_fleet) has to list it W times, and with following on
 * every copy sees only its own scene's ego, so the copies drift apart.  pp_set_world_traffic takes the same records and reads two
 * fields differently:
 *     TrafficActor.scene is a WORLD index of the fleet in force, 0 <= scene < n_worlds;
 *     TrafficActor.slot  indexes the own entries of EVERY member scene m of that world: 0 <= slot < n_own[m] (the fleet's pinned
 *                        counts), and the vehicle's pool entry in member m is pin[m].obs_off + slot.
 * There is one record and one (s, v) state per vehicle.  k_move_world_traffic / k_follow_world_traffic (one wave per vehicle) take
 * the places of k_move_traffic / k_follow_traffic: the same ObPoint bytes - and a zero ObMotion when the set carries a motion pool -
 * go into that entry of every member scene, and with following on (pp_set_traffic_follow, either order) the ego leader is the
 * nearest of ALL egos of the world: the smallest (g_e, e), a tie in the gap going to the lower scene index; a flagged ego leads
 * with speed 0.  Actor leaders are the vehicles of the same world on the same track.  Every arithmetic step is specified (§4j): a
 * numpy restatement gives the same bytes, and with worlds of one scene each the bytes are those of pp_set_traffic.
 * ONE TRAFFIC SET PER HANDLE: per scene or per world.  Either set call replaces the whole traffic; n_actors = 0 through either call
 * switches it off (the entries keep the last pose written).  pp_get_traffic_state / pp_get_traffic_speed return one value per
 * vehicle; pp_set_traffic_follow and pp_update_async (the vehicles placed at the current s in every member, no step; the pool must
 * reach the last pinned entry of any member) work as for scene traffic.
 * REQUIRES A FLEET: the worlds and the pinned slices are the fleet's (max_peers = 0 is a legal fleet for callers who want shared
 * traffic without peer obstacles).  Every SUCCESSFUL later pp_set_fleet switches world traffic off, n_worlds = 0 included - the
 * worlds it was pinned to are gone -; a refused pp_set_fleet changes nothing; pp_set_scenes / pp_set_egos / pp_set_n_scenes
 * switch it off as they do scene traffic and the fleet (§7, "Feature life cycle").  (Scene traffic keeps its relation to pp_set_fleet: either order.)
 * Checked on the host, with nothing changed on failure.  PP_ERR_STATE: no resident scenes, an update staged for the next tick, no
 * fleet.  PP_ERR_ARG: everything pp_set_traffic refuses in tracks, points, s0, speed and radius; a world out of range; a slot that
 * is not an own entry of some member scene (the message names the first such scene); two actors on one (world, slot).  One host
 * wait.  A handle that never calls pp_set_world_traffic allocates and launches none of this. */
int  pp_set_world_traffic(pp_handle h, int n_tracks, const TrafficTrack* tracks, const GlobalPoint2D* points, int n_points,
                          int n_actors, const TrafficActor* actors);

/* ---- episodic rollouts: ended egos restart on the device from start records ---------------------------------------
 * Without it every DMPP_EGO_* flag is sticky: an ego that arrived (ROUTE_END), ran out of lane or path or left its grid is frozen
 * until the host uploads new scenes.  pp_set_episodes captures every resident scene's START RECORDS - the SceneIn records of the
 * current input set, as the next tick would read them, and the SceneState array - as device copies, sets the stats to their starting
 * values and switches episodes on.  From then on every pp_advance_async runs one more kernel on the upload stream (k_respawn_egos,
 * one wave per scene) directly behind its advance kernel: it counts the advance into the running episode (age, distance), and a
 * scene whose flag word meets em->end_mask, or whose episode has reached em->max_ticks advances (DMPP_EGO_TIMEOUT in the cause word;
 * 0: no timeout), ends its episode: the stats record how, the staged SceneIn and the SceneState become the start records - every
 * byte, SceneState.tick included -, the flag word becomes 0, the trace record of the call (if any) is the start record's with
 * flags = old flags | DMPP_EGO_RESPAWNED | (cause & DMPP_EGO_TIMEOUT), and - scorecard on - RolloutScore.last_pos / last_speed move
 * to the start record, so the jump adds nothing to dist, max_acc or max_dec.  The traffic kernels, k_couple_fleet, k_resolve_map and
 * k_sanitise_scenes run behind it and see the restarted ego in the same set.  A scene frozen by a flag outside the mask stays
 * frozen until a timeout.  Every step is specified (§4k): a numpy restatement gives the same bytes.
 * A second call captures again and restarts the stats.  em NULL: episodes off - the stats stay readable and flagged egos freeze
 * again as in §4c.  pp_set_scenes / pp_set_egos / pp_set_n_scenes switch episodes off, like the fleet (§7, "Feature life cycle").
 * CALL IT LAST: later pp_set_route / pp_set_state / pp_set_grid_follow / pp_set_fleet / pp_set_traffic* / pp_set_world_traffic do
 * not touch the captured records - a restart puts back the slices, the state and the leg index of the capture.
 * PP_ERR_STATE: no resident scenes, or an update staged for the next tick.  PP_ERR_ARG: bits outside 31 in end_mask, max_ticks < 0,
 * or end_mask == 0 && max_ticks == 0 (no episode would ever end).  Nothing changes on these.  One host wait, behind every tick and
 * advance enqueued so far.  A handle that never calls pp_set_episodes allocates and launches none of this.
 * With episodes on the upload stream writes SceneState: pp_get_state / pp_set_state order themselves behind a staged advance.
 * pp_get_episode_stats: the records of the first n_scenes scenes, a staged advance included (host wait, as pp_get_ego_flags).
 * PP_ERR_STATE on a handle that never set episodes. */
void pp_default_episode_model(EpisodeModel* em);     /* end_mask 31 (all five flags), max_ticks 0 (no timeout) */
int  pp_set_episodes(pp_handle h, const EpisodeModel* em);
int  pp_get_episode_stats(pp_handle h, EpisodeStats* out, int n_scenes);

/* ---- episode spawn model: start-record pools, contact ending, spawn clearance -------------------------------------
 * On top of pp_set_episodes, which it requires to be on (PP_ERR_STATE otherwise).  While the spawn model is on, k_respawn_spawn runs
 * in the place of k_respawn_egos: with sp->contact != 0 an ego whose position lies within half a vehicle width of an obstacle of its
 * slice - the plain pool entries of the set the advance read, the motion pool ignored - ends its episode with DMPP_EGO_CONTACT in
 * the cause word; a restart draws one of sp->n_starts start records (order 0: a hash of seed, scene and episode number; 1: round
 * robin), skips the candidates that stand within sp->clearance of an obstacle of the slice (check bit 0) or of an ego of the scene's
 * world at the pose the advance read (check bit 1, only while a fleet is on), and takes the first clear one - or its first
 * choice if none is clear (EpisodeSpawnStats.n_blocked).  The restart itself is that of §4k with the chosen record.
 * starts_in / starts_state: (n_starts - 1) * n records each, record k (1 .. n_starts - 1) of scene s at index (k - 1) * n + s, so
 * that every k is a plain array of n records as pp_set_egos / pp_set_state take them; both may be NULL with n_starts == 1.  Record 0
 * is the capture of pp_set_episodes.  Lane views and junction slices of the records are derived from the resident map as for
 * pp_set_egos, obs_off / obs_n become those of the scene's record 0.  n_starts > 1 needs scenes resident from pp_set_map +
 * pp_set_egos (PP_ERR_STATE).  A staged update: PP_ERR_STATE.  PP_ERR_ARG: n_starts outside 1 .. DMPP_EPISODE_MAX_STARTS, a clearance
 * that is not finite or is negative, order outside 0 | 1, check & ~3, NULL arrays with n_starts > 1, a record that names a road or
 * lane outside the map.  Nothing changes on any of these.  One host wait.
 * sp NULL: the spawn model off, k_respawn_egos runs again, the stats stay readable.  Every successful pp_set_episodes - NULL
 * included - switches it off (its record 0 is gone), and so do pp_set_scenes / pp_set_egos / pp_set_n_scenes (§7, "Feature life cycle").
 * pp_get_episode_spawn_stats waits as pp_get_episode_stats does; PP_ERR_STATE on a handle that never set a spawn model. */
void pp_default_episode_spawn(EpisodeSpawn* sp);     /* seed 1, clearance 2 m, n_starts 1, order 0, contact 1, check 3 */
int  pp_set_episode_spawn(pp_handle h, const EpisodeSpawn* sp, const SceneIn* starts_in, const SceneState* starts_state);
int  pp_get_episode_spawn_stats(pp_handle h, EpisodeSpawnStats* out, int n_scenes);

/* ---- scenario schedule: start records drawn by their outcomes, on the device --------------------------------------
 * Start record k plus traffic set k is scenario k; the hashed choice of §4l plays them uniformly, however the episodes on each went.
 * While a schedule is in force, k_respawn_sched runs in the place of k_respawn_spawn and draws the FIRST CHOICE k0 of a restart by
 * weights: the device keeps, per start record, how many counted episodes ran on it (n_end) and how many of them failed (n_fail: the
 * cause word meets fail_mask and not pass_mask), a record's failure rate r = n_fail * 65536 / n_end (prior below min_samples), and
 *     w_k = floor_w + ((gain * (65536 - |r - target|)) >> 16),
 * k0 = the lowest k whose running sum of weights exceeds ((u >> 32) * sum) >> 32, u the hash of §4l.  Integers only; every draw of
 * an advance reads the counts as they stood before that advance's endings are folded in; window >= 2 halves a record's two counts
 * whenever n_end reaches it.  Everything else - contact, the clearance walk from k0, the restart, stats, trace - is §4l unchanged,
 * and gain == 0 gives the bytes of §4l with order 0.  scope 0: one row per scene, folded by the scene itself; scope 1: one row for the
 * handle, folded by one more kernel (k_fold_schedule, one workgroup) behind k_respawn_sched and in front of k_log_episodes.
 * The schedule is PART OF THE SPAWN MODEL IN FORCE: it needs one with order 0 (PP_ERR_STATE otherwise), and every successful
 * pp_set_episode_spawn - NULL included - and whatever retires the spawn model (§7, "Feature life cycle") leaves no schedule; it
 * retires nothing itself.  m NULL: the schedule off, k_respawn_spawn runs again.  A staged update: PP_ERR_STATE.  PP_ERR_ARG: a field
 * outside its range (dmpp_types.h), mask bits outside 31 | 64 | 128.  Nothing changes on a refusal.  A successful call zeroes the
 * rows; one host wait, behind every tick and advance enqueued so far.  A handle that never makes the call allocates and launches none of this.
 * pp_get_episode_schedule: the rows - n == 1 in pooled scope, n <= the resident scenes in per-scene scope -, a staged advance
 * included (host wait, as pp_get_episode_spawn_stats); readable after the schedule went off.  PP_ERR_STATE on a handle that never
 * made the set call.
 * pp_episode_schedule_weights: pure host code, no handle, no device - the weights w[0 .. M) the next draw would use for `row`, from
 * the function the kernel calls (w[M .. 16) = 0).  PP_ERR_ARG: M outside 1 .. 16, a model out of range, a row with n_fail outside
 * 0 .. n_end. */
void pp_default_episode_schedule(EpisodeSchedule* m);     /* scope 1, fail_mask 207, pass_mask 16, min_samples 4, window 256, floor_w 4096, gain 61440, target 32768, prior 32768 */
int  pp_set_episode_schedule(pp_handle h, const EpisodeSchedule* m);
int  pp_get_episode_schedule(pp_handle h, EpisodeScheduleRow* rows, int n);
int  pp_episode_schedule_weights(const EpisodeSchedule* m, const EpisodeScheduleRow* row, int M, int32_t w[16]);

/* ---- episode traffic reset: a restarted scene puts its traffic back on a start state ------------------------------
 * Without it a restart restores SceneIn and SceneState and leaves the scene's actors (pp_set_traffic) wherever the last episode
 * drove them: later episodes do not repeat the first.  pp_set_episode_traffic gives every actor n_sets START STATES and switches the
 * reset on: from then on every pp_advance_async runs one more kernel on the upload stream (k_reset_traffic, one thread per actor)
 * behind its traffic kernel and in front of k_couple_fleet.  For every scene that restarted in this advance (EpisodeStats.age == 0
 * behind the episode step) it discards the step the traffic kernel has just made for the scene's actors and writes
 *     s' = wrap(s*),  v' = v* (an actor with speed > 0; otherwise v' = speed),
 * (s*, v*) = set k of the actor, k = EpisodeSpawnStats.cur_start of the scene with n_sets > 1 and 0 with n_sets == 1: s' into the
 * current arc lengths, v' - following on - into the current speeds, the ObPoint at s' (zero ObMotion with a motion pool) into the
 * actor's pinned pool entry, and counts the reset.  The restarted ego is staged AT its start record and its traffic AT its start
 * states; actors of scenes that go on keep the bytes the traffic kernel wrote.  Every step is specified (§4m): a numpy restatement
 * gives the same bytes.  The clearance check of §4l still reads the pool the advance READ: the actors where they stood before.
 * SET 0 IS A CAPTURE made by the call, on the device: the current s of every actor and - following on - its current v, else its
 * speed.  Sets 1 .. n_sets - 1 come from `starts`, set k of actor a at index (k - 1) * n_actors + a; `starts` may be NULL with
 * n_sets == 1.  n_sets is 1 or EpisodeSpawn.n_starts of the spawn model in force (without one: 1); with n_sets == 1 and n_starts > 1
 * every start record uses set 0.  n_sets == 0: the reset off.  A second call builds a new table and restarts the counters.
 * CALL IT LAST: every successful pp_set_traffic / pp_set_world_traffic / pp_set_traffic_follow / pp_set_episodes /
 * pp_set_episode_spawn (NULL or n = 0 included), and pp_set_scenes / pp_set_egos / pp_set_n_scenes through them, switches the reset
 * off - each invalidates what the table was captured from (§7, "Feature life cycle").
 * Refused with nothing changed - PP_ERR_STATE: no per-scene traffic on (world traffic, §4j, has no owning scene: pp_set_episode_world_traffic below),
 * episodes off, an update staged for the next tick.  PP_ERR_ARG: n_sets < 0 or neither 1 nor n_starts, NULL starts with n_sets > 1,
 * an s that is not finite, a v that is not finite or is < 0.  One host wait, behind every tick and advance enqueued so far.
 * A handle that never makes the call allocates and launches none of this.
 * pp_get_episode_traffic_resets: how often actors 0 .. n - 1 were reset since the last successful set call; readable after the
 * reset went off.  Waits as pp_get_traffic_state does.  PP_ERR_STATE on a handle that never made the set call, PP_ERR_ARG for n
 * outside 0 .. n_actors. */
int  pp_set_episode_traffic(pp_handle h, int n_sets, const TrafficStart* starts);
int  pp_get_episode_traffic_resets(pp_handle h, int32_t* n_resets, int n);

/* ---- traffic manoeuvres: triggered lane changes, lateral offsets and speed changes -----------------------------
 * An actor of pp_set_traffic drives one track for its whole life.  pp_set_traffic_manoeuvres gives actors a list of MOVES, each
 * started by a trigger - the actor's own clock (advances), or the ego of its scene coming within `dist` metres or within `time`
 * seconds at the ego's own speed, optionally only from behind or from ahead - and made of: a new desired / scripted speed, a
 * change onto another track (the pose is projected onto it and the actor belongs to it AT ONCE: a cut-in is a cut-in for the
 * followers behind) and a lateral offset that runs from where the actor is to `lat_end` in n_steps advances along a smoothstep.
 * The records of one actor are contiguous, the actors non-decreasing; an actor's records run one after the other.  While a list
 * is in force k_manoeuvre_traffic takes the place of k_move_traffic / k_follow_traffic on every staged set; every step is specified
 * to the last bit (§4v; tests/traffic_manoeuvre_model.py).  pp_update_async places the actors at their current (s, offset): no step,
 * no trigger, no clock.  pp_set_traffic_follow leaves the states alone and sets v = v0.  While pp_set_episode_traffic is on as well
 * the actors of a restarted scene go back to the state of this call (n_done is kept).
 * The list lives inside the traffic set: it has no feature bit; every successful pp_set_traffic (no actors included),
 * pp_set_world_traffic and whatever gives the handle new resident scenes frees it.  n = 0: off - every actor becomes a plain actor
 * of the track it is on at the speed it wants, the offset is dropped at the next staged set.  A call while a list is in force
 * ends that list the same way first and places the actors without their offsets into the resident set.
 * Refused with nothing changed - PP_ERR_STATE: no per-scene traffic, world traffic, an update staged, the episode traffic reset on
 * (this call comes BEFORE pp_set_episode_traffic, which - while a list is in force - is refused unless every actor still has the
 * state this call gave it); PP_ERR_ARG: whatever pp_check_traffic_manoeuvres refuses.  One host wait.  A handle that never makes
 * the call allocates and launches none of this.
 * pp_get_traffic_manoeuvre_state: the states of actors 0 .. n_actors - 1; waits as pp_get_traffic_state does; PP_ERR_STATE while no
 * list is in force.
 * pp_check_traffic_manoeuvres: pure host, no handle, no device: -1 when the list is legal for n_actors actors and n_tracks tracks
 * (n = 0 is), else the index of the first record that is not (0 for n < 0 or a NULL list with n > 0) - an actor or track out of range, records out of order or more than
 * DMPP_MANOEUVRE_MAX for one actor, an unknown kind or side (sides belong to the EGO kinds), a dist / time that is not finite or
 * is negative for its kind, a non-finite lat_end, an infinite speed, after < 0, n_steps outside 1 .. 4096, _pad != 0. */
int  pp_set_traffic_manoeuvres(pp_handle h, int n, const TrafficManoeuvre* m);   /* n = 0: off */
int  pp_get_traffic_manoeuvre_state(pp_handle h, TrafficManoeuvreState* out, int n_actors);
int  pp_check_traffic_manoeuvres(int n_actors, int n_tracks, int n, const TrafficManoeuvre* m);

/* ---- world episodes: the egos of a world restart together ----------------------------------------------------------
 * With the spawn model alone every scene ends and restarts on its own: on a fleet (pp_set_fleet) the partner of an ended ego drives on
 * through the next "episode".  pp_set_episode_worlds(h, 1) makes the WORLD the unit of an episode: from then on every pp_advance_async
 * runs k_respawn_world in the place of k_respawn_spawn.  When any ego of a world has a cause of its own (a flag of end_mask, TIMEOUT,
 * CONTACT - contact with a peer slot included), EVERY ego of that world ends on this advance: cause word = its own | DMPP_EGO_WORLD
 * when another member had a cause (a sole ender carries no WORLD bit; a member with no cause of its own ends with exactly 256).  The
 * world draws ONE start record index k - the hash / round robin of §4l on the world's first scene -, walks the candidates with the
 * clearance test against the OWN obstacle entries of every member (EpisodeSpawn.check bit 0; bit 1 is ignored: every ego of the world
 * moves), and every member restarts on its record k; the EpisodeSpawnStats words of the step are the same in every member.  WORLD,
 * like CONTACT, has no n_end slot.  Worlds are those of the fleet in force AT EACH ADVANCE; without a fleet every scene is a world
 * of one and every byte is §4l's.  The per-scene traffic reset (§4m), the episode log (§4n: cause carries 256), the score trace and
 * the ego tracker run unchanged behind it.
 * Part of the spawn model in force, like the schedule: every successful pp_set_episode_spawn (NULL included) and whatever switches
 * the spawn model off switches it off; it retires nothing itself.  on == 0: off (k_respawn_spawn runs again; the world traffic reset
 * below goes off with it).  Refused with nothing changed - PP_ERR_STATE: an update staged, the spawn model off, a schedule in force
 * (pp_set_episode_schedule is refused in turn while world episodes are on).  No host wait.
 *
 * ---- world traffic reset: the vehicles of a restarted world go back to a start state ---------------------------------
 * pp_set_episode_world_traffic is pp_set_episode_traffic for the vehicles of pp_set_world_traffic: set 0 is captured by the call,
 * sets 1 .. n_sets - 1 come from `starts` (set k of vehicle a at (k - 1) * n_actors + a), n_sets is 1 or n_starts.  From then on every
 * pp_advance_async runs k_reset_world_traffic behind its world-traffic kernel: a vehicle of world w resets iff EpisodeStats.age == 0
 * at the world's FIRST scene behind the episode step, onto set cur_start of that scene (n_sets > 1) or set 0; s', v', the ObPoint in
 * every member scene and the counter as §4m.  n_sets == 0: off.  Switched off by everything that switches the per-scene reset off,
 * by world traffic, the spawn model or episodes going off or being set again, by pp_set_fleet, and by pp_set_episode_worlds(h, 0).
 * Refused with nothing changed - PP_ERR_STATE: world traffic not on, episodes / spawn model / world episodes not on, an update staged;
 * PP_ERR_ARG: as pp_set_episode_traffic.  One host wait.  pp_get_episode_world_traffic_resets: one counter per vehicle since the last
 * successful set call, readable after the reset went off; waits as pp_get_traffic_state does. */
int  pp_set_episode_worlds(pp_handle h, int on);
int  pp_set_episode_world_traffic(pp_handle h, int n_sets, const TrafficStart* starts);
int  pp_get_episode_world_traffic_resets(pp_handle h, int32_t* n_resets, int n);

/* ---- episode log: one record per ended episode, appended on the device ---------------------------------------------
 * EpisodeStats is an aggregate per scene and RolloutScore runs across restarts: neither says which episode ended how.  pp_set_episode_log
 * gives the handle a ring of cap EpisodeRecord on the device and switches the log on: from then on every pp_advance_async runs one
 * more kernel on the upload stream (k_log_episodes, ONE workgroup of 1024 threads) directly behind k_respawn_egos / k_respawn_spawn, in front of the
 * traffic kernels.  It appends one record for every scene whose episode the advance ended (EpisodeStats.age == 0 behind the episode
 * step): scene, episode number, start record, cause, age, metres, the pose and speed of the record the ending advance READ, the number
 * of the advance (seq, counted from the set call) and of the tick it read, and the episode's OWN scorecard.  The records of one advance
 * stand in the order of their scene indices, those of successive advances behind each other - a scan, not a race for a counter - so a
 * log is reproducible byte for byte.  With more endings in one advance than the ring holds only the last cap are written.
 * The episode's scorecard: while the log AND the scorecard (pp_score_begin) are on, every scored tick is folded a second time
 * (k_score_ego<true>, §4d steps 2 - 4) into a record per scene that restarts - to the starting values of §4d - whenever the scene's
 * episode ends, pp_score_begin is called or a set call restarts the totals.  Its grid half stays at the starting values.  Without
 * pp_score_begin the record carries the starting values (n_ticks == 0).
 * CALL IT LAST: every successful pp_set_episodes / pp_set_episode_spawn (NULL included), and pp_set_scenes / pp_set_egos /
 * pp_set_n_scenes through them, switch the log off (§7, "Feature life cycle").  cap == 0: the log off; what was logged stays readable.  A second call with
 * cap > 0 starts a new log (total 0, seq 0, nothing unread).  PP_ERR_ARG: cap < 0 or > DMPP_EPISODE_LOG_MAX.  PP_ERR_STATE: an update
 * staged for the next tick; cap > 0 with episodes off.  A refused call changes nothing.  One host wait, behind every tick and advance
 * enqueued so far.  A handle that never makes the call allocates and launches none of this.
 * pp_read_episode_log: waits for a staged advance as pp_get_episode_stats does, then copies the oldest unread records still in the ring,
 * at most max_records of them, oldest first (at most two copies), marks them read and returns their number (>= 0; an error code is
 * negative).  *n_lost (may be NULL): records that were overwritten before any read saw them, newly counted by this call.  What does
 * not fit into max_records stays unread.  PP_ERR_STATE on a handle that never made the set call.
 * pp_get_episode_log_info: *total - records appended since the set call; *lost_total - records overwritten unread so far, those the
 * next read will report included.  Either may be NULL.  Waits as pp_read_episode_log does. */
int  pp_set_episode_log(pp_handle h, int cap);
int  pp_read_episode_log(pp_handle h, EpisodeRecord* out, int max_records, long long* n_lost);
int  pp_get_episode_log_info(pp_handle h, long long* total, long long* lost_total);

/* ---- one scene, one call, one host wait: the latency path of the class surface ------------------------------------------
 * CPlanning::plan(...) / CDecision::decide(...) take everything by value on every call (Planning.h:57-75) and own the
 * cross-tick state as members.  A PpSceneIo block (pinned host memory: pp_host_alloc(sizeof(PpSceneIo))) carries exactly that
 * - location + decision, obstacle list, refpath / junction polyline, state in; PlanOut, state, GridOut, published refpath
 * out - and pp_tick_io moves it with two small kernels that read / write the block over PCIe on the handle's stream, around
 * one pp_plan_tick: no copy command, one host wait.  The handle must hold ONE resident scene (pp_set_scenes: its lane pool
 * stays; io->in.lanes must lie inside it).  io->in.obs_off / obs_n / ref_off / ref_n are set from n_obs / n_ref.
 * COUNTS.  Nothing is ever dropped: 0 <= n_obs <= min(PP_IO_MAX_OBS, caps.max_obs_total) and 0 <= n_ref <= min(DMPP_MAX_REFPATH,
 * caps.max_ref_pts_total).  A negative count is PP_ERR_ARG, a count above its limit PP_ERR_CAPACITY; a handle that does not
 * hold exactly one scene, and PP_IO_WANT_GRID on a handle whose grid stage is off, are PP_ERR_STATE.  A call refused for any of
 * these launches nothing: the block, the handle and pp_tick_id are as before, and the next call is an ordinary one.  Every call lists ALL obstacles of its tick: nothing
 * of an earlier, longer list is read again.
 * A LANE SLICE outside the resident pool (off < 0, n < 0 or off + n past it) is not refused: no slice is dereferenced, the scene
 * runs with all three lanes empty, status is 1, every output is written as usual and the call returns PP_ERR_ARG.
 * CALL ORDER.  The call may follow anything on the handle - unsynced pp_plan_tick calls included, which it orders itself behind.
 * It SUPERSEDES an update staged by pp_update_async / pp_advance_async and not yet adopted by a tick: that update is gone, no later
 * tick brings it back.  The block carries no ObMotion, so the tick runs WITHOUT a motion pool - its obstacles are static whatever
 * cfg.dynamic_obstacles says - and the handle keeps that setting afterwards: later pp_plan_tick calls read the block's obstacles,
 * static, until a pp_set_scenes / pp_set_egos / pp_update_async brings a motion pool again.  pp_get_plan / pp_get_state /
 * pp_get_grid_out / pp_get_path / pp_get_refpath afterwards return what the block holds.
 * UNTOUCHED in the block: in, n_obs, n_ref, want, obs, ref always; grid without PP_IO_WANT_GRID; dec_ref without PP_IO_WANT_REFPATH,
 * and with it every point from plan.dec.refpath_n on.  state, status and plan are written by every call that is not refused. */
#define PP_IO_MAX_OBS       1024
#define PP_IO_WANT_GRID     1     /* io->grid is filled (the tick must run the grid stage) */
#define PP_IO_WANT_REFPATH  2     /* io->dec_ref[0 .. plan.dec.refpath_n) is filled (decision stage) */
typedef struct PpSceneIo {
    SceneIn       in;
    SceneState    state;                      /* in / out */
    int32_t       n_obs, n_ref, want, status; /* status out: 0 ok, 1 a lane slice outside the resident pool (scene ran with empty lanes) */
    ObPoint       obs[PP_IO_MAX_OBS];
    GlobalPoint2D ref[DMPP_MAX_REFPATH];
    PlanOut       plan;                       /* out */
    GridOut       grid;                       /* out (PP_IO_WANT_GRID) */
    GlobalPoint2D dec_ref[DMPP_MAX_REFPATH];  /* out (PP_IO_WANT_REFPATH) */
} PpSceneIo;
int  pp_tick_io(pp_handle h, PpSceneIo* io);

/* ---- stand-alone operators on the path ------------------------------------------------------
 * CShare::SearchObstacle (11 call sites, e.g. Planning.cpp:168, Decision.cpp:811): query q
 * uses path points [path_off[q], path_off[q+1]) and obstacles [obs_off[q], obs_off[q+1]). */
int  pp_search_obstacle_batch(pp_handle h, int n_queries,
                              const GlobalPoint2D* paths, const int32_t* path_off,
                              const ObPoint* obs, const int32_t* obs_off,
                              const double* lat_lo, const double* lat_hi, Path_Obs* out);
/* CPlanning::GetLatDis / GetRoadAngle / GetAngleErr (Planning.cpp:686-786), n independent items.
 * op 0: out = GetLatDis(a[i], b[i], c[i]);  op 1: out = GetRoadAngle(a[i], b[i]);
 * op 2: out = GetAngleErr(a[i].x, a[i].y);  op 3: out = CShare::CalcDistance(a[i], b[i]);
 * op 4 / 5: the .lat / .lng of CShare::GlobalToWGS84(a[i]) (Planning.cpp:209). */
int  pp_geom_batch(pp_handle h, int op, int n, const GlobalPoint2D* a, const GlobalPoint2D* b,
                   const GlobalPoint2D* c, double* out);
/* One scalar stage of the planning tick on explicit arguments:
 *  op 0 CPlanning::UpdatePlanJudge (Planning.cpp:797-832): in = {last_behavior, behavior, pos, path_lat_dis,
 *       path_dir_err, remain_dis} -> out = {afresh, cause}
 *  op 1 CPlanning::SpeedPlanning (Planning.cpp:888-990): in = {pos, ob_flag, mindist_lon, faraim_dis,
 *       velocity_expect, brake_speed, acc_flag, des_acc} -> out = {brake_speed, acc_flag, des_acc}
 *  op 2 CPlanning::CalculateRadius (Planning.cpp:1000-1019): in = {path_near_id, path_front_near_id},
 *       last_Bpoints = 200 points -> out = {radius} */
int  pp_scalar_stage(pp_handle h, int op, const double* in, int n_in, const GlobalPoint2D* last_Bpoints,
                     double* out, int n_out);
/* CShare::BezierPlanning / MeanPoints / CreateNewPath on one polyline each (host pointers). */
int  pp_bezier(pp_handle h, GlobalPoint3D start, GlobalPoint3D end, GlobalPoint2D* out, int n);
int  pp_mean_points(pp_handle h, const GlobalPoint2D* in, int n_in, GlobalPoint2D* out, int n_out);
int  pp_create_new_path(pp_handle h, const GlobalPoint2D* path, int n, double offset, GlobalPoint2D* out);

/* ---- measurement / multi-GPU plumbing --------------------------------------------------------- */
/* on = 1: every kernel launch of pp_plan_tick is bracketed by HIP events on the stream it is launched on; on = 2: only the
 * search kernel (an event pair costs a few microseconds of queue time: 2 is what a throughput measurement wants); 0: off. */
int   pp_set_profile(pp_handle h, int on);
/* Sum of event-measured durations (ms) and launch count of kernel k since the last reset. */
int   pp_get_kernel_ms(pp_handle h, int k, float* ms_total, int* launches);
int   pp_reset_kernel_ms(pp_handle h);
/* Raw device pointer + byte size of an internal buffer, so a caller can scatter inputs into /
 * gather results out of it with RCCL without a host hop. */
void* pp_device_ptr(pp_handle h, int which, size_t* bytes);
void* pp_stream(pp_handle h);       /* hipStream_t; ordered after the ticks only after pp_join / pp_sync (see pp_plan_tick) */
/* sizeof of an ABI struct, for bindings to check their mirror: 0 PlannerConfig, 1 PlannerCaps,
 * 2 SceneIn, 3 SceneState, 4 PlanOut, 5 GridOut, 6 ObPoint, 7 ObMotion, 8 Path_Obs, 9 LocationOut,
 * 10 DecisionOutPod, 11 LaneView, 12 PlanningOut, 13 PlanningStatus, 14 AimPoint, 15 MapLane, 16 MapJunction,
 * 17 MapDesc, 18 PpSceneIo, 19 EgoModel, 20 EgoTrace, 21 RolloutScore, 22 FleetModel, 23 RouteLeg, 24 RouteModel,
 * 25 GridFollow, 26 TrafficTrack, 27 TrafficActor, 28 TrafficFollow, 29 EpisodeModel, 30 EpisodeStats,
 * 31 EpisodeSpawn, 32 EpisodeSpawnStats, 33 TrafficStart, 34 EpisodeRecord, 35 ScoreTraceModel, 36 ScoreTick,
 * 37 ScoreTraceInfo, 38 EpisodeSchedule, 39 EpisodeScheduleRow, 40 EgoTracker, 41 EgoTrackState,
 * (42 unassigned) 43 PackedPlan, 44 PackedGrid, 45 ConflictModel, 46 ConflictScore, 47 TrafficManoeuvre,
 * 48 TrafficManoeuvreState, (49 unassigned) 50 PerceptionModel, 51 PerceptTrack, 52 PerceptionStats */
size_t pp_sizeof(int which);
/* Tick groups (pp_plan_tick): a piped tick defers its search and scoring until G ticks are enqueued, then launches them for
 * all G at once.  G for n scenes per tick, given the search's workgroup slots and the tick slots the handle holds (gcap);
 * forced > 0: that many (env DMPP_TICK_GROUP).  pp_tick_group_cap: the tick slots a handle allocates for.
 * pp_tick_group_const: 0 slots per group at most, 1 search sets, 2 / 3 group positions / sets of the obstacle snapshot,
 * 4 / 5 group positions / sets of GridOut.  No device needed. */
int pp_tick_group_size(int n_scenes, int search_slots, int gcap, int forced);
int pp_tick_group_cap(int max_scenes, int pipeline_min, int forced, size_t item_bytes);
int pp_tick_group_const(int which);
/* The LDS budget of a tick group's search (data words per view) and the workgroup slots it gives, from plain integers: the search
 * kernel's static LDS, per-line meta bytes and dense-form LDS, the largest budget, the CUs; scenes per tick, ticks per group, the
 * obstacle pool size; what the densest scene of an earlier group needed (-1: nothing yet); the budget in force (0: none) and
 * whether it came from a need; mode: bit 0 a fixed budget (env DMPP_LDS_BUDGET), bit 1 dense forced (env DMPP_SEARCH_GBM).
 * Out (any may be NULL): the new budget, whether it now comes from a need, the slots.  No device needed. */
int pp_search_budget(int static_lds, int meta_bytes, int gbm_lds, int lds_budget_max, int n_cus, int n_scenes, int group, int n_obs_total,
                     int need, int budget, int from_need, int mode, int32_t* budget_out, int32_t* from_need_out, int32_t* slots_out);
/* The co-residency step behind that policy ("LDS budget and the dense form"): the budget a group's search is launched
 * with, given the one pp_search_budget chose (`budget`), the work items of the group (scenes x ticks) and the need.  It is lowered -
 * to the largest multiple of 64 words that is not below need + max(need / 32, 96) - only when the items outnumber the workgroup
 * slots, the policy's budget leaves less LDS free on a CU than a k_planning or k_score workgroup holds, and the lower one leaves
 * that much with as many searching workgroups per CU; mode as above (either bit: unchanged).  env DMPP_CORESIDENT=0 switches the
 * step off in a handle.  pp_get_search_info reports the budget the launch used.  No device needed. */
int pp_coresident_budget(int static_lds, int meta_bytes, int gbm_lds, int lds_budget_max, int n_cus, int items, int need, int budget,
                         int mode, int32_t* budget_out);
/* The rollout feature table ("Feature life cycle"): which features a successful set call switches off, and what holds
 * between the features that are on.  Feature bits: 1 fleet, 2 route, 4 traffic per scene, 8 world traffic, 16 traffic follow,
 * 32 episodes, 64 spawn model, 128 traffic reset, 256 episode log, 512 scenario schedule, 1024 world episodes, 2048 world traffic reset
 * (the set calls of the last three have no cause: they retire nothing).  Causes: 0 pp_set_scenes / pp_set_egos / pp_set_n_scenes, 1 pp_set_map,
 * 2 pp_set_fleet, 3 pp_set_route, 4 pp_set_traffic, 5 pp_set_world_traffic, 6 pp_set_traffic_follow, 7 pp_set_episodes,
 * 8 pp_set_episode_spawn, 9 pp_set_episode_traffic, 10 pp_set_episode_log (2 + i: the set call of feature bit i, i < 9), 11 pp_set_traffic /
 * pp_set_world_traffic with no actors, 12 pp_set_grid_follow, 13 pp_score_begin / pp_score_end.  pp_feature_retires: the bits the cause switches off, -1 for no such cause.
 * pp_feature_consistent: 1 when the features in `mask` may be on together on a handle with / without a resident map and with that
 * resident mode (0 pp_set_scenes, 1 pp_set_egos), else 0.  No device needed. */
int pp_feature_retires(int cause);
int pp_feature_consistent(unsigned mask, int have_map, int resident_mode);
/* The search keeps a scene's obstacle bitmaps sparse in LDS; a launch gives every scene `lds_budget_words` words per view
 * (sized from what the densest scene of an earlier tick needed) and a scene that needs more is searched on dense bitmaps
 * in HBM instead.  After a tick: the budget of that tick, the words the densest scene seen so far needed, and how many
 * scenes of the last tick took the dense path.  Any pointer may be NULL. */
int   pp_get_search_info(pp_handle h, int32_t* lds_budget_words, int32_t* need_words, int32_t* dense_scenes);
/* After filling the input buffers through pp_device_ptr (an RCCL scatter straight into them): declares what is resident -
 * scenes, the used part of each pool, whether the motion pool / the lane attribute pool were filled - and checks every
 * scene's slices against those pools, like pp_set_scenes does. */
int   pp_set_n_scenes(pp_handle h, int n_scenes, int n_lane_pts, int n_ref_pts, int n_obs_total, int have_motion, int have_lane_attr);

#ifdef __cplusplus
}
#endif
#endif /* DMPP_PLANNER_H */
