"""Python host binding of the MI355X planning engine (ctypes over include/dmpp_planner.h).

The product is libdmpp.so (hand-written HIP kernels behind a C-ABI).  This module only
mirrors the ABI structs as numpy dtypes and forwards calls; it never computes planning
results itself and it raises if the library is missing (no CPU fallback).

Reference surface mirrored: CPlanning / CDecision (Planning.h:38-85, Decision.h:106-107)
as one batched `Planner.tick()`; see INTEGRATION.md.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdmpp.so")

PATH_POINTS, OUT_POINTS, LANESUM, MAX_REFPATH, MAX_LATTICE = 200, 100, 8, 512, 17
GEN_LANE_PTS, GEN_REF_PTS = 320, 128

G_FOUND, G_NO_PATH, G_LIMIT, G_OVERFLOW, G_GOAL_BLOCKED, G_PATH_TRUNC, G_INTERNAL, G_COST_RANGE = range(8)
G_STATUS_COUNT = 8
K_NAMES = ["k_effective_obstacles", "k_decision", "k_planning", "k_search", "k_score", "k_pack_plan", "k_pack_grid", "k_perceive"]
(BUF_SCENE_IN, BUF_LANE_POOL, BUF_REF_POOL, BUF_OBS_POOL, BUF_MOT_POOL, BUF_STATE, BUF_PLAN_OUT, BUF_GRID_OUT,
 BUF_GRID, BUF_PATH, BUF_ORDER, BUF_LANE_ATTR, BUF_OBS_NOW, BUF_OBS_SEEN) = range(14)


def _dt(fields):
    return np.dtype(fields, align=True)


f8, i4, u4, f4, u8, u2 = np.float64, np.int32, np.uint32, np.float32, np.uint64, np.uint16
GlobalPoint2D = _dt([("x", f8), ("y", f8)])
GlobalPoint3D = _dt([("x", f8), ("y", f8), ("dir", f8)])
AimPoint = _dt([("Aim_point", GlobalPoint3D), ("Aim_id", i4), ("_pad", i4)])
ObPoint = _dt([("x", f8), ("y", f8), ("type", i4), ("radius", f4)])
ObMotion = _dt([("vx", f8), ("vy", f8)])
LaneView = _dt([("cur_off", i4), ("cur_n", i4), ("left_off", i4), ("left_n", i4), ("right_off", i4), ("right_n", i4),
                ("lane_sum", i4), ("lanechg_attribute", i4), ("lane_width", f8)])
LocationOut = _dt([("globalpoint", GlobalPoint3D), ("velocity", f8), ("pos", i4), ("road_num", i4), ("lane_num", i4),
                   ("last_roadnum", i4), ("next_roadnum", i4), ("last_lanenum", i4), ("next_lanenum", i4),
                   ("path_num", i4), ("id", i4, (LANESUM,))])
DecisionOutPod = _dt([("velocity_expect", f8), ("behavior", i4), ("target_roadnum", i4), ("target_lanenum", i4),
                   ("light", i4), ("behavior_to_dlg", i4), ("refpath_n", i4)])
Obs_To_Veh = _dt([("dis_lat", f8), ("dis_lng", f8)])
Path_Obs = _dt([("Ob_Pose", Obs_To_Veh), ("Ob_Attr", ObPoint), ("Obs_flag", i4), ("Ob_Pathid", i4)])
PlanningOut = _dt([("brakedis", f8), ("brake_speed", f8), ("desacc", f8), ("desspd", f8), ("desstr", f8), ("radius", f8),
                   ("cnt", i4), ("APA", i4), ("desaccVd", i4), ("desstrVd", i4), ("light", i4), ("road_type", i4),
                   ("sstop", i4), ("_pad", i4), ("pnts", GlobalPoint2D, (OUT_POINTS,))])
PlanningStatus = _dt([("near_ob_dist", f8), ("planspeed", f8), ("planacc", f8), ("afresh_cause", i4), ("trafficlight", i4),
                      ("path_points", GlobalPoint2D, (OUT_POINTS,))])
SceneState = _dt([("last_Bpoints", GlobalPoint2D, (PATH_POINTS,)), ("aimpoint_far", AimPoint), ("aimpoint_near", AimPoint),
                  ("path_lat_dis", f8), ("remain_dis", f8), ("path_dir_err", f8), ("brakespeed", f8), ("des_acc", f8),
                  ("faraim_dis", f4), ("nearaim_dis", f4), ("path_near_id", i4), ("path_front_near_id", i4),
                  ("his_behavior", i4), ("afresh_planning", i4), ("afresh_cause", i4), ("acc_flag", i4), ("count", i4),
                  ("z_behavior", i4), ("z_light_status", i4), ("z_target_lanenum", i4), ("z_target_roadnum", i4),
                  ("z_behavior_to_dlg", i4), ("z_segment_lanechg_status", i4), ("z_segment_obsavoid_status", i4),
                  ("d_his_behavior", i4), ("d_his_light_status", i4), ("d_his_target_lanenum", i4),
                  ("obsavoid_time", u4), ("no_obsaviod_time", u4), ("frontobs_time", u4), ("tick", i4), ("_pad", i4),
                  ("z_velocity_expect", f8), ("leftlight_time", f8), ("rightlight_time", f8)])
SceneIn = _dt([("loc", LocationOut), ("dec", DecisionOutPod), ("lanes", LaneView), ("ref_off", i4), ("ref_n", i4),
               ("obs_off", i4), ("obs_n", i4), ("stub_attribute", i4), ("_pad", i4), ("out_lane_no", u2, (LANESUM,)),
               ("period_last", f8), ("grid_origin", GlobalPoint2D),
               ("goal", GlobalPoint2D)])
GridOut = _dt([("order_digest", u8), ("status", i4), ("n_expanded", i4), ("n_pushed", i4), ("n_rounds", i4),
               ("path_len", i4), ("path_cost", i4), ("start_cell", i4), ("goal_cell", i4), ("best_candidate", i4),
               ("n_candidates", i4), ("cand_cost", f8, (MAX_LATTICE,)), ("cand_col", f8, (MAX_LATTICE,)),
               ("cand_curv", f8, (MAX_LATTICE,)), ("cand_prog", f8, (MAX_LATTICE,)),
               ("best_path", GlobalPoint2D, (PATH_POINTS,))])
PlanOut = _dt([("result", PlanningOut), ("show", PlanningStatus), ("road_points", GlobalPoint2D, (PATH_POINTS,)),
               ("around", Path_Obs, (6,)), ("dec", DecisionOutPod), ("ob_dis_lat", f8), ("ob_dis_lng", f8), ("ob", ObPoint),
               ("ob_flag", i4), ("ob_pathid", i4), ("sweep_side", i4), ("sweep_index", i4), ("navi_lanechg", i4),
               ("navi_lanechg_times", i4)])
PlannerConfig = _dt([("ROAD_FARAIM_MAX", f8), ("ROAD_FARAIM_MIN", f8), ("PRE_INTER_FARAIM", f8), ("INTER_FARAIM", f8),
                     ("ROAD_REMAIN_DISTANCE", f8), ("INTER_REMAIN_DISTANCE", f8), ("EPSILON", f8), ("PI", f8),
                     ("Vehicle_Width", f8), ("NO_OBSTACLE_DIS", f8), ("wgs_lat0", f8), ("wgs_lng0", f8),
                     ("wgs_deg_per_m_lat", f8), ("wgs_deg_per_m_lng", f8), ("ID_MORE", i4), ("decision_stage", i4),
                     ("lanechg_stage", i4), ("grid_stage", i4), ("grid_w", i4), ("grid_h", i4), ("max_expansions", i4), ("bucket_cap", i4),
                     ("max_path", i4), ("n_lattice", i4), ("lookahead_cells", i4), ("dynamic_obstacles", i4),
                     ("force_replan", i4), ("_cfg_pad", i4), ("cell", f8), ("inflate", f8), ("lattice_step", f8), ("d_safe", f8),
                     ("w_col", f8), ("w_curv", f8), ("w_prog", f8), ("w_off", f8), ("dyn_dt", f8)])
PlannerCaps = _dt([("max_scenes", i4), ("max_obs_total", i4), ("max_lane_pts_total", i4), ("max_ref_pts_total", i4),
                   ("order_cap", i4), ("_pad", i4)])

EgoModel = _dt([("dt", f8), ("max_acc", f8), ("max_dec", f8), ("window", i4), ("_pad", i4)])
EgoTrace = _dt([("pose", GlobalPoint3D), ("velocity", f8), ("id_cur", i4), ("lane_num", i4), ("flags", i4), ("_pad", i4)])
EGO_PATH_END, EGO_BAD_PATH, EGO_LANE_END, EGO_OFF_GRID = 1, 2, 4, 8      # sticky rollout flags (DMPP_EGO_*)
# rollout scorecard: one record per scene, folded on the device over the scored ticks
RolloutScore = _dt([("min_clearance", f8), ("dist", f8), ("max_speed", f8), ("max_acc", f8), ("max_dec", f8),
                    ("last_pos", GlobalPoint2D), ("last_speed", f8), ("n_ticks", i4), ("min_clearance_tick", i4),
                    ("min_clearance_obs", i4), ("first_collision_tick", i4), ("n_collision_ticks", i4), ("n_replans", i4),
                    ("n_ob_flag", i4), ("n_desacc", i4), ("behavior_ticks", i4, (8,)), ("ego_flags", i4), ("_pad", i4),
                    ("n_grid_ticks", i4), ("n_grid_path_candidate", i4), ("grid_status_ticks", i4, (G_STATUS_COUNT,))])
# fleet coupling: the egos of one world are each other's obstacles during a rollout
FleetModel = _dt([("range", f8), ("radius", f4), ("max_peers", i4)])
OB_PEER = 0x40000000          # ObPoint.type of a peer slot: OB_PEER | scene index of the peer (DMPP_OB_PEER)
FLEET_MAX_PEERS = 64
# route following: rollout egos cross junctions onto the next road of their route
RouteLeg = _dt([("road_num", i4), ("stub_attribute", i4), ("out_lane_no", u2, (LANESUM,))])
RouteModel = _dt([("pre_points", i4), ("_pad", i4)])
EGO_ROUTE_END = 16            # the ego came to the end of the last leg of its route (DMPP_EGO_ROUTE_END)
# a grid that follows the ego: the advance step re-centres grid_origin and goal
GridFollow = _dt([("goal_point", i4), ("margin_cells", i4)])
# ego tracking model: rollout egos keep a pose of their own and steer a bicycle model along the plan
EgoTracker = _dt([("look_min", f8), ("look_gain", f8), ("max_curv", f8), ("curv_rate", f8), ("curv_bias", f8), ("n_sub", i4), ("_pad", i4)])
EgoTrackState = _dt([("hx", f8), ("hy", f8), ("kappa", f8), ("key_x", u8), ("key_y", u8), ("key_dir", u8), ("max_kappa", f8),
                     ("valid", i4), ("n_init", i4), ("n_sat", i4), ("_pad", i4)])
# lane traffic: scripted vehicles that drive a polyline and sit in their scene's own obstacle entries
TrafficTrack = _dt([("point_off", i4), ("n_points", i4), ("closed", i4), ("_pad", i4)])
TrafficActor = _dt([("s0", f8), ("speed", f8), ("scene", i4), ("slot", i4), ("track", i4), ("type", i4), ("radius", f4), ("_pad", i4)])
# car-following traffic: actors with speed > 0 keep a gap to the ego and to each other
TrafficFollow = _dt([("look", f8), ("lateral", f8), ("gap", f8), ("headway", f8), ("max_acc", f8), ("comfort_dec", f8), ("max_dec", f8), ("min_net", f8)])
# episodic rollouts: ended egos restart on the device from start records; how every episode ended is counted
EpisodeModel = _dt([("end_mask", i4), ("max_ticks", i4)])
EpisodeStats = _dt([("n_episodes", i4), ("age", i4), ("n_end", i4, (6,)), ("last_cause", i4), ("last_age", i4), ("min_age", i4), ("max_age", i4),
                    ("ticks_total", np.int64), ("dist", f8), ("last_dist", f8), ("dist_total", f8)])
EGO_RESPAWNED = 32            # EgoTrace.flags only: the record is the start of a new episode (DMPP_EGO_RESPAWNED)
EGO_TIMEOUT = 64              # cause word only: the episode reached EpisodeModel.max_ticks (DMPP_EGO_TIMEOUT)
# episode spawn model: a pool of start records per scene, contact ends an episode, a start record must be clear
EPISODE_MAX_STARTS = 16
EpisodeSpawn = _dt([("seed", np.uint64), ("clearance", f8), ("n_starts", i4), ("order", i4), ("contact", i4), ("check", i4)])
EpisodeSpawnStats = _dt([("n_contact", i4), ("n_blocked", i4), ("n_rejected", i4), ("cur_start", i4), ("n_used", i4, (EPISODE_MAX_STARTS,))])
EGO_CONTACT = 128             # cause words only: the ego touched an obstacle of its slice (DMPP_EGO_CONTACT)
EGO_WORLD = 256               # cause words only: another ego of the scene's world ended on this advance (DMPP_EGO_WORLD, §4s)
# episode traffic reset: the actors of a restarted scene go back to a start state, one set per start record
TrafficStart = _dt([("s", f8), ("v", f8)])
# traffic manoeuvres: triggered lane changes, lateral offsets and speed changes of the actors of set_traffic
MANOEUVRE_MAX = 8
TRIG_ADVANCES, TRIG_EGO_DIST, TRIG_EGO_TIME = 0, 1, 2          # TrafficManoeuvre.trigger = kind | side << 8 (side 1: ego behind, 2: ego ahead)
TrafficManoeuvre = _dt([("dist", f8), ("time", f8), ("lat_end", f8), ("speed", f8), ("actor", i4), ("trigger", i4), ("after", i4), ("track", i4),
                        ("n_steps", i4), ("_pad", i4)])
TrafficManoeuvreState = _dt([("lat", f8), ("lat0", f8), ("v0", f8), ("track", i4), ("next", i4), ("k", i4), ("clock", i4), ("n_done", i4), ("_pad", i4)])
# episode log: one record per ended episode, appended on the device in the order of the scenes
EPISODE_LOG_MAX = 1 << 20
EpisodeRecord = _dt([("scene", i4), ("episode", i4), ("start", i4), ("cause", i4), ("age", i4), ("seq", i4), ("tick", np.int64),
                     ("dist", f8), ("end_pos", GlobalPoint2D), ("end_speed", f8), ("score", RolloutScore)])
# score trace: a ring of the last scored ticks per scene, frozen shortly after an incident
SCORE_TRACE_MAX = 256
TRACE_COLLISION, TRACE_NEAR, TRACE_FLAG, TRACE_BRAKE = 1, 2, 4, 8          # cause bits (DMPP_TRACE_*)
TICK_REPLAN, TICK_OB_FLAG, TICK_DESACC, TICK_START = 1, 2, 4, 8            # low bits of ScoreTick.marks (DMPP_TICK_*)
ScoreTraceModel = _dt([("depth", i4), ("post", i4), ("trigger", i4), ("flag_mask", i4), ("near", f8), ("brake", f8)])
ScoreTick = _dt([("k", i4), ("flags", i4), ("tick", np.int64), ("x", f8), ("y", f8), ("v", f8), ("clearance", f8), ("obs", i4), ("ob_type", i4),
                 ("behavior", i4), ("marks", i4)])
ScoreTraceInfo = _dt([("n_written", i4), ("state", i4), ("trigger_k", i4), ("trigger", i4), ("post_left", i4), ("n_trigger_ticks", i4), ("_pad", i4, (2,))])
# conflict score: time to collision and braking demand per scene from the snapshots of consecutive scored ticks
ConflictModel = _dt([("ttc_warn", f8), ("ttc_crit", f8), ("v_max", f8), ("min_closing", f8)])
ConflictScore = _dt([("min_ttc", f8), ("max_drac", f8), ("tit_warn", f8), ("last_pos", GlobalPoint2D), ("n_ticks", i4), ("n_conflict_ticks", i4),
                     ("n_warn_ticks", i4), ("n_crit_ticks", i4), ("min_ttc_tick", i4), ("min_ttc_obs", i4), ("min_ttc_type", i4), ("first_crit_tick", i4),
                     ("max_drac_tick", i4), ("n_no_history_ticks", i4), ("prev_off", i4), ("prev_n", i4)])
# perception model: the planner reads a perceived snapshot - range, field of view, occlusion, misses, noise, tracks
PERCEPT_HIDDEN_XY = 1.0e12          # x = y of the hidden record (DMPP_PERCEPT_HIDDEN_XY); its type is the truth's, its radius 0
PerceptionModel = _dt([("range", f8), ("cos_half_fov", f8), ("sigma0", f8), ("sigma_gain", f8), ("p_miss", np.uint32), ("seed", np.uint32),
                       ("occlusion", i4), ("confirm", i4), ("coast", i4), ("_pad", i4)])
PerceptTrack = _dt([("last", ObPoint), ("hits", np.uint16), ("misses", np.uint16), ("confirmed", np.uint8), ("_pad", np.uint8, (3,))])
PerceptionStats = _dt([("n_ticks", np.int64), ("n_entries", np.int64), ("n_out", np.int64), ("n_occluded", np.int64), ("n_missed", np.int64),
                       ("n_detected", np.int64), ("n_fresh", np.int64), ("n_coasted", np.int64), ("n_hidden", np.int64),
                       ("min_hidden_clearance", f8), ("min_hidden_tick", np.int64), ("min_hidden_obs", i4), ("min_hidden_type", i4)])
# scenario schedule: the start record of a restart drawn by weights from per-record outcome counts kept on the device
EpisodeSchedule = _dt([("scope", i4), ("fail_mask", i4), ("pass_mask", i4), ("min_samples", i4), ("window", i4), ("floor_w", i4), ("gain", i4),
                       ("target", i4), ("prior", i4), ("_pad", i4)])
EpisodeScheduleRow = _dt([("n_end", i4, (EPISODE_MAX_STARTS,)), ("n_fail", i4, (EPISODE_MAX_STARTS,))])
# packed streamed fetch: a tick's results packed on the device into 1744 + 248 B per scene, unpacked on the host
PACKED_NONE, PACKED_LATTICE, PACKED_PATH, PACKED_BAD = 0, 1, 2, 4          # PackedGrid.kind (DMPP_PACKED_*)
PackedPlan = _dt([("brakedis", f8), ("brake_speed", f8), ("desacc", f8), ("desspd", f8), ("desstr", f8), ("radius", f8),
                  ("cnt", i4), ("APA", i4), ("desaccVd", i4), ("desstrVd", i4), ("light", i4), ("road_type", i4), ("sstop", i4),
                  ("afresh_cause", i4), ("near_ob_dist", f8), ("planspeed", f8), ("planacc", f8), ("trafficlight", i4), ("ob_flag", i4),
                  ("dec", DecisionOutPod), ("path_points", GlobalPoint2D, (OUT_POINTS,))])
PackedGrid = _dt([("order_digest", u8), ("status", i4), ("n_expanded", i4), ("n_pushed", i4), ("n_rounds", i4), ("path_len", i4),
                  ("path_cost", i4), ("start_cell", i4), ("goal_cell", i4), ("best_candidate", i4), ("n_candidates", i4),
                  ("best_cost", f8), ("best_col", f8), ("best_curv", f8), ("best_prog", f8), ("kind", i4), ("n_steps", i4),
                  ("geo", f8, (8,)), ("planes", u8, (12,))])

# one scene, one call (pp_tick_io): the pinned block that carries the inputs, the state and the outputs of the latency path
PP_OK, PP_ERR_ARG, PP_ERR_HIP, PP_ERR_CAPACITY, PP_ERR_STATE = 0, -1, -2, -3, -4
PP_IO_MAX_OBS, PP_IO_WANT_GRID, PP_IO_WANT_REFPATH = 1024, 1, 2
PpSceneIo = _dt([("in", SceneIn), ("state", SceneState), ("n_obs", i4), ("n_ref", i4), ("want", i4), ("status", i4),
                 ("obs", ObPoint, (PP_IO_MAX_OBS,)), ("ref", GlobalPoint2D, (MAX_REFPATH,)), ("plan", PlanOut), ("grid", GridOut),
                 ("dec_ref", GlobalPoint2D, (MAX_REFPATH,))])

MapLane = _dt([("point_off", i4), ("n_points", i4), ("lane_sum", i4), ("_pad", i4)])
MapJunction = _dt([("last_road", i4), ("next_road", i4), ("last_lane", i4), ("next_lane", i4), ("point_off", i4), ("n_points", i4)])

_SIZEOF_ORDER = [PlannerConfig, PlannerCaps, SceneIn, SceneState, PlanOut, GridOut, ObPoint, ObMotion, Path_Obs,
                 LocationOut, DecisionOutPod, LaneView, PlanningOut, PlanningStatus, AimPoint, MapLane, MapJunction]


class MapDesc(C.Structure):          # include/dmpp_types.h: the map store handed to pp_set_map
    _fields_ = [("n_roads", C.c_int32), ("n_lanes", C.c_int32), ("n_points", C.c_int32), ("n_junctions", C.c_int32),
                ("n_jpoints", C.c_int32), ("_pad", C.c_int32), ("road_first_lane", C.c_void_p), ("lanes", C.c_void_p),
                ("points", C.c_void_p), ("lanechg_attribute", C.c_void_p), ("lane_width_cm", C.c_void_p),
                ("junctions", C.c_void_p), ("jpoints", C.c_void_p)]



class _P3(C.Structure):          # GlobalPoint3D passed by value
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("dir", C.c_double)]


_vp, _ci, _f8, _pll = C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_longlong)
# One entry per feature that came after the first release: (probe symbol, {function: (argtypes, restype)}, {pp_sizeof index: dtype}).
# load_library binds an entry as a whole.  The package's own library must have every entry; an OLDER build named through DMPP_LIB /
# `path` (A/B measurements against a parent commit) may lack whole entries - those whose probe symbol it does not export.
_FEATURES = [
    ("pp_advance_async", {"pp_default_ego_model": ([_vp], None), "pp_advance_async": ([_vp, _vp, _vp], _ci),
                          "pp_rollout": ([_vp, _ci, _vp, _vp, _pll], _ci), "pp_get_ego_flags": ([_vp, _vp, _ci], _ci)}, {19: EgoModel, 20: EgoTrace}),
    ("pp_score_begin", {"pp_score_begin": ([_vp, _f8], _ci), "pp_score_end": ([_vp], _ci), "pp_get_rollout_score": ([_vp, _vp, _ci], _ci)}, {21: RolloutScore}),
    ("pp_set_fleet", {"pp_default_fleet_model": ([_vp], None), "pp_set_fleet": ([_vp, _ci, _vp, _vp], _ci),
                      "pp_get_obstacles": ([_vp, _ci, _vp, _ci], _ci)}, {22: FleetModel}),
    ("pp_set_route", {"pp_default_route_model": ([_vp], _ci), "pp_set_route": ([_vp, _ci, _vp, _vp, _vp], _ci)}, {23: RouteLeg, 24: RouteModel}),
    ("pp_set_grid_follow", {"pp_default_grid_follow": ([_vp], None), "pp_set_grid_follow": ([_vp, _vp], _ci)}, {25: GridFollow}),
    ("pp_set_traffic", {"pp_set_traffic": ([_vp, _ci, _vp, _vp, _ci, _ci, _vp], _ci), "pp_get_traffic_state": ([_vp, _vp, _ci], _ci)},
     {26: TrafficTrack, 27: TrafficActor}),
    ("pp_set_world_traffic", {"pp_set_world_traffic": ([_vp, _ci, _vp, _vp, _ci, _ci, _vp], _ci)}, {}),
    ("pp_set_traffic_follow", {"pp_default_traffic_follow": ([_vp], None), "pp_set_traffic_follow": ([_vp, _vp], _ci),
                               "pp_get_traffic_speed": ([_vp, _vp, _ci], _ci)}, {28: TrafficFollow}),
    ("pp_set_episodes", {"pp_default_episode_model": ([_vp], None), "pp_set_episodes": ([_vp, _vp], _ci),
                         "pp_get_episode_stats": ([_vp, _vp, _ci], _ci)}, {29: EpisodeModel, 30: EpisodeStats}),
    ("pp_set_episode_spawn", {"pp_default_episode_spawn": ([_vp], None), "pp_set_episode_spawn": ([_vp, _vp, _vp, _vp], _ci),
                              "pp_get_episode_spawn_stats": ([_vp, _vp, _ci], _ci)}, {31: EpisodeSpawn, 32: EpisodeSpawnStats}),
    ("pp_set_episode_traffic", {"pp_set_episode_traffic": ([_vp, _ci, _vp], _ci), "pp_get_episode_traffic_resets": ([_vp, _vp, _ci], _ci)}, {33: TrafficStart}),
    ("pp_set_episode_log", {"pp_set_episode_log": ([_vp, _ci], _ci), "pp_read_episode_log": ([_vp, _vp, _ci, _pll], _ci),
                            "pp_get_episode_log_info": ([_vp, _pll, _pll], _ci)}, {34: EpisodeRecord}),
    ("pp_set_score_trace", {"pp_default_score_trace": ([_vp], None), "pp_set_score_trace": ([_vp, _vp], _ci),
                            "pp_get_score_trace_info": ([_vp, _vp, _ci], _ci), "pp_read_score_trace": ([_vp, _ci, _vp, _ci, _vp, _ci], _ci)},
     {35: ScoreTraceModel, 36: ScoreTick, 37: ScoreTraceInfo}),
    ("pp_set_episode_schedule", {"pp_default_episode_schedule": ([_vp], None), "pp_set_episode_schedule": ([_vp, _vp], _ci),
                                 "pp_get_episode_schedule": ([_vp, _vp, _ci], _ci), "pp_episode_schedule_weights": ([_vp, _vp, _ci, _vp], _ci)},
     {38: EpisodeSchedule, 39: EpisodeScheduleRow}),
    ("pp_set_ego_tracker", {"pp_default_ego_tracker": ([_vp], None), "pp_set_ego_tracker": ([_vp, _vp], _ci),
                            "pp_get_ego_track_state": ([_vp, _vp, _ci], _ci)}, {40: EgoTracker, 41: EgoTrackState}),
    ("pp_set_packed_fetch", {"pp_set_packed_fetch": ([_vp, _ci], _ci), "pp_fetch_packed_async": ([_vp, _vp, _vp, _pll], _ci),
                             "pp_unpack_plan": ([_vp, _vp, _ci, _vp, _vp, _vp], _ci), "pp_unpack_grid": ([_vp, _vp, _ci, _vp], _ci)},
     {43: PackedPlan, 44: PackedGrid}),          # (pp_sizeof id 42 stays unassigned)
    ("pp_set_episode_worlds", {"pp_set_episode_worlds": ([_vp, _ci], _ci), "pp_set_episode_world_traffic": ([_vp, _ci, _vp], _ci),
                               "pp_get_episode_world_traffic_resets": ([_vp, _vp, _ci], _ci)}, {}),
    ("pp_set_conflict_score", {"pp_default_conflict": ([_vp], None), "pp_set_conflict_score": ([_vp, _vp], _ci),
                               "pp_get_conflict_score": ([_vp, _vp, _ci], _ci)}, {45: ConflictModel, 46: ConflictScore}),
    ("pp_set_traffic_manoeuvres", {"pp_set_traffic_manoeuvres": ([_vp, _ci, _vp], _ci), "pp_get_traffic_manoeuvre_state": ([_vp, _vp, _ci], _ci),
                                   "pp_check_traffic_manoeuvres": ([_ci, _ci, _ci, _vp], _ci)}, {47: TrafficManoeuvre, 48: TrafficManoeuvreState}),
    ("pp_set_perception", {"pp_default_perception": ([_vp], None), "pp_set_perception": ([_vp, _vp], _ci),
                           "pp_get_perception_stats": ([_vp, _vp, _ci], _ci), "pp_get_perception_tracks": ([_vp, _vp, _ci, _ci], _ci)},
     {50: PerceptionModel, 51: PerceptTrack, 52: PerceptionStats}),          # (pp_sizeof id 49 stays unassigned)
]

_lib = None
_hip = None          # the HIP runtime itself, for Planner.write_device only


class PlannerError(RuntimeError):
    pass


def load_library(path=None):
    """Load libdmpp.so (built by `make -C csrc` / __graft_entry__.build()). Raises if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("DMPP_LIB") or LIB_PATH          # DMPP_LIB: another build of the library (A/B measurements)
    if not os.path.exists(path):
        raise PlannerError(f"{path} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()')")
    lib = C.CDLL(path)
    vp, ci, cz = C.c_void_p, C.c_int, C.c_size_t
    lib.pp_last_error.restype = C.c_char_p
    lib.pp_sizeof.restype = cz
    lib.pp_sizeof.argtypes = [ci]
    lib.pp_default_config.argtypes = [vp, ci, ci]
    lib.pp_default_config.restype = None
    lib.pp_init_state.argtypes = [vp, ci]
    lib.pp_init_state.restype = None
    lib.pp_gen_scenes.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_create.argtypes = [vp, ci, vp, C.POINTER(vp)]
    lib.pp_destroy.argtypes = [vp]
    lib.pp_set_config.argtypes = [vp, vp]
    lib.pp_set_scenes.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, vp, ci]
    lib.pp_set_n_scenes.argtypes = [vp, ci, ci, ci, ci, ci, ci]
    lib.pp_join.argtypes = [vp]
    lib.pp_get_search_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    lib.pp_set_map.argtypes = [vp, vp]
    lib.pp_set_egos.argtypes = [vp, ci, vp, vp, vp, ci]
    lib.pp_get_scene_in.argtypes = [vp, vp, ci]
    lib.pp_set_state.argtypes = [vp, vp, ci]
    lib.pp_plan_tick.argtypes = [vp]
    lib.pp_sync.argtypes = [vp]
    lib.pp_device_synchronize.argtypes = [vp]
    lib.pp_get_plan.argtypes = [vp, vp, ci]
    lib.pp_get_state.argtypes = [vp, vp, ci]
    lib.pp_get_grid_out.argtypes = [vp, vp, ci]
    lib.pp_get_grid.argtypes = [vp, ci, vp]
    lib.pp_get_order.argtypes = [vp, ci, vp, ci]
    lib.pp_get_path.argtypes = [vp, ci, vp, ci]
    lib.pp_get_refpath.argtypes = [vp, ci, vp, ci]
    lib.pp_plan_tick_batch.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, ci, vp, ci, vp, vp, vp]
    lib.pp_search_obstacle_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.pp_geom_batch.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    lib.pp_scalar_stage.argtypes = [vp, ci, vp, ci, vp, vp, ci]
    lib.pp_bezier.argtypes = [vp, _P3, _P3, vp, ci]
    lib.pp_mean_points.argtypes = [vp, vp, ci, vp, ci]
    lib.pp_create_new_path.argtypes = [vp, vp, ci, C.c_double, vp]
    lib.pp_set_profile.argtypes = [vp, ci]
    lib.pp_get_kernel_ms.argtypes = [vp, ci, C.POINTER(C.c_float), C.POINTER(ci)]
    lib.pp_reset_kernel_ms.argtypes = [vp]
    lib.pp_device_ptr.argtypes = [vp, ci, C.POINTER(cz)]
    lib.pp_device_ptr.restype = vp
    lib.pp_stream.argtypes = [vp]
    lib.pp_stream.restype = vp
    lib.pp_update_async.argtypes = [vp, ci, vp, vp, vp, ci]
    lib.pp_fetch_async.argtypes = [vp, vp, vp, C.POINTER(C.c_longlong)]
    lib.pp_fetch_published_async.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_longlong)]
    lib.pp_wait_tick.argtypes = [vp, C.c_longlong, C.POINTER(ci)]
    lib.pp_tick_id.argtypes = [vp]
    lib.pp_tick_id.restype = C.c_longlong
    lib.pp_tick_io.argtypes = [vp, vp]
    for probe, fns, sizes in _FEATURES:
        if not hasattr(lib, probe) and path != LIB_PATH:          # an OLDER build named through DMPP_LIB / `path` may lack the feature
            continue
        for name, (argtypes, restype) in fns.items():            # (the package's own library must have every one: AttributeError)
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
        for which, dt in sizes.items():
            if lib.pp_sizeof(which) != dt.itemsize:
                raise PlannerError(f"ABI mismatch for struct #{which}: C {lib.pp_sizeof(which)} B, binding {dt.itemsize} B")
    lib.pp_host_alloc.argtypes = [cz]
    lib.pp_host_alloc.restype = vp
    lib.pp_host_free.argtypes = [vp]
    lib.pp_host_free.restype = None
    lib.pp_host_register.argtypes = [vp, cz]
    lib.pp_host_unregister.argtypes = [vp]
    if lib.pp_sizeof(17) != C.sizeof(MapDesc):
        raise PlannerError(f"ABI mismatch for MapDesc: C {lib.pp_sizeof(17)} B, binding {C.sizeof(MapDesc)} B")
    for which, dt in list(enumerate(_SIZEOF_ORDER)) + [(18, PpSceneIo)]:
        if lib.pp_sizeof(which) != dt.itemsize:
            raise PlannerError(f"ABI mismatch for struct #{which}: C {lib.pp_sizeof(which)} B, binding {dt.itemsize} B")
    _lib = lib
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):          # raw host/device address
        return a
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def _check(rc):
    if rc != 0:
        raise PlannerError(f"libdmpp error {rc}: {load_library().pp_last_error().decode()}")


def _default(dtype, fn_name, *args, checked=False):
    """One record of `dtype`, filled by the library's pp_default_* function `fn_name`."""
    rec = np.zeros(1, dtype)
    rc = getattr(load_library(), fn_name)(_ptr(rec), *args)
    if checked:
        _check(rc)
    return rec


def default_config(grid_w=512, grid_h=None):
    """PlannerConfig record with the build-chosen values for every undefined reference macro."""
    return _default(PlannerConfig, "pp_default_config", grid_w, grid_h or grid_w)


def default_ego_model():
    """EgoModel record of the closed-loop rollout (pp_default_ego_model): dt, acceleration limits, id search window."""
    return _default(EgoModel, "pp_default_ego_model")


def default_fleet_model():
    """FleetModel record of the fleet coupling (pp_default_fleet_model): range, peer radius, peer slots per scene."""
    return _default(FleetModel, "pp_default_fleet_model")


def default_route_model():
    """RouteModel record of the route following (pp_default_route_model): lane points of pre-junction before a lane's end."""
    return _default(RouteModel, "pp_default_route_model", checked=True)


def default_grid_follow():
    """GridFollow record of the grid that follows the ego (pp_default_grid_follow): the path point the goal is taken from, the margin in cells."""
    return _default(GridFollow, "pp_default_grid_follow")


def default_ego_tracker():
    """EgoTracker record of the ego tracking model (pp_default_ego_tracker): look-ahead 3 m + 0.5 s, |curvature| <= 0.2 1/m,
    0.3 1/(m s) curvature rate, no bias, 2 substeps."""
    return _default(EgoTracker, "pp_default_ego_tracker")


def default_episode_model():
    """EpisodeModel record of the episodic rollouts (pp_default_episode_model): end_mask 31 (all five EGO_* flags), max_ticks 0 (no timeout)."""
    return _default(EpisodeModel, "pp_default_episode_model")


def default_episode_spawn():
    """EpisodeSpawn record of the episode spawn model (pp_default_episode_spawn): seed 1, clearance 2 m, n_starts 1, order 0 (hashed),
    contact 1, check 3 (the obstacle slice and the egos of the world)."""
    return _default(EpisodeSpawn, "pp_default_episode_spawn")


def default_episode_schedule():
    """EpisodeSchedule record of the scenario schedule (pp_default_episode_schedule): scope 1 (pooled), fail_mask 207, pass_mask 16
    (every cause but ROUTE_END fails), min_samples 4, window 256, floor_w 4096, gain 61440, target and prior 32768 (a 50 % failure rate)."""
    return _default(EpisodeSchedule, "pp_default_episode_schedule")


def episode_schedule_weights(model, row, n_starts):
    """pp_episode_schedule_weights: the weights of start records 0 .. n_starts - 1 that the next draw would use for the
    EpisodeScheduleRow `row` under `model` - pure host code from the function the kernel calls, no handle, no device."""
    m = np.array(model, EpisodeSchedule).reshape(1).copy()
    r = np.array(row, EpisodeScheduleRow).reshape(1).copy()
    w = np.zeros(EPISODE_MAX_STARTS, np.int32)
    _check(load_library().pp_episode_schedule_weights(_ptr(m), _ptr(r), int(n_starts), _ptr(w)))
    return w[:int(n_starts)].copy()


def unpack_plan(cfg, packed, result=True, show=True, dec=True):
    """pp_unpack_plan: (PlanningOut, PlanningStatus, DecisionOutPod) arrays rebuilt from PackedPlan records under the configuration
    their tick ran with - pure host code, no handle, no device.  An output switched off comes back as None."""
    pk = np.ascontiguousarray(packed, PackedPlan).reshape(-1)
    n = len(pk)
    out = [np.zeros(n, dt) if want else None for dt, want in ((PlanningOut, result), (PlanningStatus, show), (DecisionOutPod, dec))]
    c = np.array(cfg, PlannerConfig).reshape(1).copy()          # (kept in a local: the call reads it)
    _check(load_library().pp_unpack_plan(_ptr(c), _ptr(pk), n, *[_ptr(o) for o in out]))
    return tuple(out)


def unpack_grid(cfg, packed, out=None):
    """pp_unpack_grid: GridOut records rebuilt from PackedGrid records - pure host code, no handle, no device.  Equal to the device's in
    every byte except cand_*[k] for k != best_candidate, which are 0.  Raises PlannerError when a record is none a tick packs (that
    scene's GridOut is left zeroed; `out`, when given, receives the records either way)."""
    pk = np.ascontiguousarray(packed, PackedGrid).reshape(-1)
    if out is None:
        out = np.zeros(len(pk), GridOut)
    assert out.dtype == GridOut and len(out) >= len(pk)
    c = np.array(cfg, PlannerConfig).reshape(1).copy()          # (kept in a local: the call reads it)
    _check(load_library().pp_unpack_grid(_ptr(c), _ptr(pk), len(pk), _ptr(out)))
    return out


def default_conflict():
    """ConflictModel record of the conflict score (pp_default_conflict): ttc_warn 3 s, ttc_crit 1.5 s, v_max 70 m/s, min_closing 0."""
    return _default(ConflictModel, "pp_default_conflict")


def default_perception():
    """PerceptionModel record of the perception model (pp_default_perception): range 60 m, cos_half_fov cos 60 deg, sigma0 0.1 m,
    sigma_gain 0.005, p_miss 2 % of 2^32, seed 1, occlusion on, confirm 2, coast 3 - a starting point, not tuned values."""
    return _default(PerceptionModel, "pp_default_perception")


def transparent_perception():
    """The PerceptionModel that hides nothing and changes nothing: the perceived snapshot is the truth's bytes for every finite entry."""
    m = np.zeros(1, PerceptionModel)
    m["range"], m["cos_half_fov"] = np.inf, -1.0
    return m


def default_score_trace():
    """ScoreTraceModel record of the score trace (pp_default_score_trace): depth 64, post 8, trigger TRACE_COLLISION, flag_mask 0,
    near 0.5 m, brake 6 m/s^2."""
    return _default(ScoreTraceModel, "pp_default_score_trace")


def default_traffic_follow():
    """TrafficFollow record of the car-following traffic (pp_default_traffic_follow): look 60 m, lateral 1.5 m, gap 2 m, headway 1.5 s,
    max_acc 1, comfort_dec 2, max_dec 6 m/s^2, min_net 0.1 m."""
    return _default(TrafficFollow, "pp_default_traffic_follow")


def gen_scenes(cfg, first_scene, n_scenes, n_obs, junction_every=8):
    """Seeded synthetic scenes. Returns a dict of numpy arrays."""
    lib = load_library()
    sc = dict(
        scene_in=np.zeros(n_scenes, SceneIn),
        lane_pool=np.zeros(n_scenes * 3 * GEN_LANE_PTS, GlobalPoint3D),
        attr_pool=np.zeros(n_scenes * 3 * GEN_LANE_PTS, np.uint8),
        ref_pool=np.zeros(n_scenes * GEN_REF_PTS, GlobalPoint2D),
        obs_pool=np.zeros(max(n_scenes * n_obs, 1), ObPoint),
        mot_pool=np.zeros(max(n_scenes * n_obs, 1), ObMotion),
        state=np.zeros(n_scenes, SceneState),
    )
    _check(lib.pp_gen_scenes(_ptr(cfg), first_scene, n_scenes, n_obs, junction_every, _ptr(sc["scene_in"]),
                             _ptr(sc["lane_pool"]), _ptr(sc["attr_pool"]), _ptr(sc["ref_pool"]), _ptr(sc["obs_pool"]),
                             _ptr(sc["mot_pool"]), _ptr(sc["state"])))
    sc["n_obs"] = n_obs
    return sc


class _Pinned:
    """Owner of one pp_host_alloc block (freed when the last numpy view of it goes)."""

    def __init__(self, nbytes):
        self.lib = load_library()
        self.ptr = self.lib.pp_host_alloc(max(int(nbytes), 1))
        if not self.ptr:
            raise PlannerError("pp_host_alloc failed: " + self.lib.pp_last_error().decode())
        self.buf = (C.c_char * max(int(nbytes), 1)).from_address(self.ptr)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.lib.pp_host_free(self.ptr)
            self.ptr = None


def pinned_empty(n, dtype):
    """numpy array of n records in pinned host memory (pp_host_alloc): what pp_update_async / pp_fetch_async want."""
    dtype = np.dtype(dtype)
    owner = _Pinned(n * dtype.itemsize)
    a = np.frombuffer(owner.buf, dtype=dtype, count=n)      # keeps `owner.buf` (and through it nothing else) alive ...
    a = a.view(_PinnedArray)
    a._owner = owner                                          # ... so the owner rides on the array
    return a


class _PinnedArray(np.ndarray):
    _owner = None

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


def _io_block(io):
    """Refuses anything but a one-record PpSceneIo array that lies inside a pp_host_alloc block (a copy of one does not)."""
    if not isinstance(io, np.ndarray) or io.dtype != PpSceneIo or io.shape != (1,) or not io.flags["C_CONTIGUOUS"]:
        raise ValueError("tick_io: the block must be pinned_empty(1, PpSceneIo): one C-contiguous PpSceneIo record")
    owner = getattr(io, "_owner", None)
    first = io.ctypes.data
    if owner is None or not owner.ptr or first < owner.ptr or first + io.nbytes > owner.ptr + len(owner.buf):
        raise ValueError("tick_io: the block must lie in pinned host memory (pinned_empty(1, PpSceneIo)): the device reads and writes it")


def pinned_copy(a):
    out = pinned_empty(len(a), a.dtype)
    out[...] = a
    return out


class Planner:
    """One GPU, one stream, resident scenes: the batched stand-in for the CDecision + CPlanning threads."""

    def __init__(self, cfg, device=0, max_scenes=1024, max_obs_total=None, max_lane_pts_total=None,
                 max_ref_pts_total=None, order_cap=0):
        self.lib = load_library()
        self.cfg = np.array(cfg, PlannerConfig).reshape(1).copy()
        caps = np.zeros(1, PlannerCaps)
        caps["max_scenes"] = max_scenes
        caps["max_obs_total"] = max_obs_total if max_obs_total is not None else max_scenes * 256
        caps["max_lane_pts_total"] = max_lane_pts_total if max_lane_pts_total is not None else max_scenes * 3 * GEN_LANE_PTS
        caps["max_ref_pts_total"] = max_ref_pts_total if max_ref_pts_total is not None else max_scenes * GEN_REF_PTS
        caps["order_cap"] = order_cap
        self.caps = caps
        h = C.c_void_p()
        _check(self.lib.pp_create(_ptr(self.cfg), device, _ptr(caps), C.byref(h)))
        self.h = h
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.pp_destroy(self.h)
            self.h = None

    __del__ = close

    def set_config(self, cfg):
        self.cfg = np.array(cfg, PlannerConfig).reshape(1).copy()
        _check(self.lib.pp_set_config(self.h, _ptr(self.cfg)))

    def set_scenes(self, sc, with_motion=True):
        n = len(sc["scene_in"])
        _check(self.lib.pp_set_scenes(self.h, n, _ptr(sc["scene_in"]), _ptr(sc["lane_pool"]), _ptr(sc.get("attr_pool")),
                                      len(sc["lane_pool"]),
                                      _ptr(sc["ref_pool"]), len(sc["ref_pool"]), _ptr(sc["obs_pool"]),
                                      _ptr(sc["mot_pool"]) if with_motion else None, n * sc["n_obs"]))
        self.n = n

    def set_map(self, m):
        """Resident map store (pp_set_map). `m`: dict with road_first_lane (int32, n_roads + 1), lanes (MapLane),
        points (GlobalPoint3D), lanechg_attribute (uint8), lane_width_cm (uint16), junctions (MapJunction),
        jpoints (GlobalPoint2D)."""
        keep = {k: np.ascontiguousarray(m[k]) for k in ("road_first_lane", "lanes", "points", "lanechg_attribute", "lane_width_cm",
                                                        "junctions", "jpoints")}
        d = MapDesc(len(keep["road_first_lane"]) - 1, len(keep["lanes"]), len(keep["points"]), len(keep["junctions"]),
                    len(keep["jpoints"]), 0, *[_ptr(keep[k]) if len(keep[k]) else None for k in
                                               ("road_first_lane", "lanes", "points", "lanechg_attribute", "lane_width_cm",
                                                "junctions", "jpoints")])
        _check(self.lib.pp_set_map(self.h, C.addressof(d)))

    def set_egos(self, sc, with_motion=True):
        """Scenes on the resident map (pp_set_egos): lane views and junction slices are derived on the device."""
        n = len(sc["scene_in"])
        _check(self.lib.pp_set_egos(self.h, n, _ptr(sc["scene_in"]), _ptr(sc["obs_pool"]),
                                    _ptr(sc["mot_pool"]) if with_motion else None, n * sc["n_obs"]))
        self.n = n

    def get_scene_in(self):
        out = np.zeros(self.n, SceneIn)
        _check(self.lib.pp_get_scene_in(self.h, _ptr(out), self.n))
        return out

    def set_state(self, state):
        _check(self.lib.pp_set_state(self.h, _ptr(state), len(state)))

    def tick(self, sync=False):
        _check(self.lib.pp_plan_tick(self.h))
        if sync:
            self.sync()

    def sync(self):
        _check(self.lib.pp_sync(self.h))

    # ---- one scene, one call, one host wait: the latency path of the class surface ----------
    def tick_io(self, io, check=True):
        """pp_tick_io: `io` is ONE PpSceneIo record in pinned memory - pinned_empty(1, PpSceneIo) - that carries location + decision,
        obstacle list, refpath and state in, and PlanOut, state, GridOut and the published refpath out (the kernels of the call read
        and write the block itself, so nothing else is accepted).  Returns the return code; with check=True a non-zero code raises."""
        _io_block(io)
        rc = self.lib.pp_tick_io(self.h, io.ctypes.data)
        if check:
            _check(rc)
        return rc

    # ---- streamed ticks (no host wait) ---------------------------------------------------
    def update_async(self, scene_in=None, obs_pool=None, mot_pool=None, n_obs_total=None):
        """pp_update_async: the inputs of the next tick.  Arrays should be pinned (pinned_empty / pinned_copy) and must stay
        untouched until wait_tick of the tick that adopts them."""
        if n_obs_total is None:
            n_obs_total = len(obs_pool) if obs_pool is not None else 0
        _check(self.lib.pp_update_async(self.h, self.n, _ptr(scene_in), _ptr(obs_pool), _ptr(mot_pool), int(n_obs_total)))

    # ---- closed-loop rollout: the egos follow their own plans on the device ---------------
    def advance_async(self, model=None, trace=None):
        """pp_advance_async: the SceneIn records of the next tick from the last tick's plan.  `trace`: EgoTrace array of self.n
        records in pinned memory (or a device address), written by the kernel; it is complete after the next sync / wait_tick."""
        m = default_ego_model() if model is None else np.array(model, EgoModel).reshape(1).copy()
        _check(self.lib.pp_advance_async(self.h, _ptr(m), _ptr(trace)))

    def rollout(self, n_ticks, model=None, trace=False):
        """pp_rollout: n_ticks times (advance, tick) with no host wait.  Returns the id of the last tick, or - with trace=True -
        (that id, a pinned EgoTrace array of shape (n_ticks, self.n)): row t is complete once the ticks have finished (sync())."""
        m = default_ego_model() if model is None else np.array(model, EgoModel).reshape(1).copy()
        tr = pinned_empty(max(n_ticks * self.n, 1), EgoTrace) if trace else None
        t = C.c_longlong()
        _check(self.lib.pp_rollout(self.h, int(n_ticks), _ptr(m), _ptr(tr), C.byref(t)))
        if trace:
            return t.value, tr[:n_ticks * self.n].reshape(n_ticks, self.n)
        return t.value

    def ego_flags(self):
        """pp_get_ego_flags: the sticky EGO_* flag word of every scene after the last advance (host wait)."""
        out = np.zeros(self.n, np.int32)
        _check(self.lib.pp_get_ego_flags(self.h, _ptr(out), self.n))
        return out

    # ---- rollout scorecard: per-scene totals of the scored ticks, kept on the device -----
    def score_begin(self, dt=None):
        """pp_score_begin: every tick from here on is folded into one RolloutScore record per scene (totals restart).
        `dt`: seconds between ticks, the divisor of max_acc / max_dec (default: the default ego model's dt)."""
        if dt is None:
            dt = float(default_ego_model()["dt"][0])
        _check(self.lib.pp_score_begin(self.h, float(dt)))

    def score_end(self):
        """pp_score_end: scoring off; the records stay readable."""
        _check(self.lib.pp_score_end(self.h))

    def rollout_score(self):
        """pp_get_rollout_score: the RolloutScore records, the last enqueued tick included (host wait)."""
        out = np.zeros(self.n, RolloutScore)
        _check(self.lib.pp_get_rollout_score(self.h, _ptr(out), self.n))
        return out

    # ---- score trace: the last scored ticks of every scene, frozen on an incident ------------------
    def set_score_trace(self, model=None, off=False):
        """pp_set_score_trace, before or after score_begin: every scene gets a ring of model.depth ScoreTick records
        on the device; while the scorecard is on every scored tick stores one, and a ring freezes model.post ticks after a tick that
        meets a cause of model.trigger.  model None: the default model.  A second call starts again.  off=True: the recorder off;
        rings and headers stay readable."""
        if off:
            _check(self.lib.pp_set_score_trace(self.h, None))
            return
        m = default_score_trace() if model is None else np.array(model, ScoreTraceModel).reshape(1).copy()
        _check(self.lib.pp_set_score_trace(self.h, _ptr(m)))
        self.score_trace_depth = int(m["depth"][0])

    def score_trace_info(self):
        """pp_get_score_trace_info: the ScoreTraceInfo headers, the last enqueued tick included (host wait)."""
        out = np.zeros(self.n, ScoreTraceInfo)
        _check(self.lib.pp_get_score_trace_info(self.h, _ptr(out), self.n))
        return out

    def read_score_trace(self, scene, rearm=False, cap=None):
        """pp_read_score_trace: (the ScoreTick records of the scene's ring, oldest first, the ScoreTraceInfo header they were read
        under); rearm: the header goes back to armed behind the read, the ring and n_written stay (host wait)."""
        want = getattr(self, "score_trace_depth", 0) if cap is None else int(cap)
        out, info = np.zeros(max(want, 1), ScoreTick), np.zeros(1, ScoreTraceInfo)
        n = self.lib.pp_read_score_trace(self.h, int(scene), _ptr(out), want, _ptr(info), 1 if rearm else 0)
        if n < 0:
            _check(n)
        return out[:n].copy(), info[0].copy()

    def set_conflict_score(self, model):
        """pp_set_conflict_score, before or after score_begin: while the scorecard is on, every scored tick differences
        the obstacle snapshot against the one of the scored tick before and folds the tick's smallest time to collision and largest
        braking demand into one ConflictScore record per scene.  model: a ConflictModel record (default_conflict()); a second call
        starts again.  None: the step off; the records stay readable."""
        if model is None:
            _check(self.lib.pp_set_conflict_score(self.h, None))
            return
        m = np.array(model, ConflictModel).reshape(1).copy()
        _check(self.lib.pp_set_conflict_score(self.h, _ptr(m)))

    def conflict_score(self):
        """pp_get_conflict_score: the ConflictScore records, the last enqueued tick included (host wait)."""
        out = np.zeros(self.n, ConflictScore)
        _check(self.lib.pp_get_conflict_score(self.h, _ptr(out), self.n))
        return out

    def set_perception(self, model):
        """pp_set_perception: from the next tick on k_perceive takes the place of the snapshot kernel; Decision,
        Planning, the search and its scoring read the perceived snapshot (BUF_OBS_SEEN), every judge keeps the truth (BUF_OBS_NOW).
        model: a PerceptionModel record (default_perception()); every call restarts tracks and stats.  None: off, they stay readable."""
        if model is None:
            _check(self.lib.pp_set_perception(self.h, None))
            return
        m = np.array(model, PerceptionModel).reshape(1).copy()
        _check(self.lib.pp_set_perception(self.h, _ptr(m)))

    def perception_stats(self):
        """pp_get_perception_stats: the PerceptionStats records, the last enqueued tick included (host wait)."""
        out = np.zeros(self.n, PerceptionStats)
        _check(self.lib.pp_get_perception_stats(self.h, _ptr(out), self.n))
        return out

    def perception_tracks(self, first=0, count=None):
        """pp_get_perception_tracks: `count` PerceptTrack records from pool entry `first` on (default: the obstacle pool of the
        resident set), the last enqueued tick included (host wait)."""
        n = int(self.n_obs_total if count is None else count)
        out = np.zeros(n, PerceptTrack)
        _check(self.lib.pp_get_perception_tracks(self.h, _ptr(out), int(first), n))
        return out

    # ---- fleet coupling: the egos of one world are each other's obstacles ------------------
    def set_fleet(self, world_first=None, fm=None):
        """pp_set_fleet: world w = scenes [world_first[w], world_first[w + 1]); every scene's obstacle slice is pinned and the
        fm.max_peers pool entries behind it become its peer slots.  world_first None (or one entry): fleet off."""
        if world_first is None or len(world_first) < 2:
            _check(self.lib.pp_set_fleet(self.h, 0, None, None))
            return
        wf = np.ascontiguousarray(world_first, np.int32)
        m = default_fleet_model() if fm is None else np.array(fm, FleetModel).reshape(1).copy()
        _check(self.lib.pp_set_fleet(self.h, len(wf) - 1, _ptr(wf), _ptr(m)))

    # ---- route following: routed egos cross junctions onto the next road ------------------
    def set_route(self, legs=None, route_first=None, model=None):
        """pp_set_route: the route of scene s is legs[route_first[s] : route_first[s + 1]] (RouteLeg records; an empty run leaves
        the scene unrouted); loc.path_num indexes the ego's current leg within it.  legs None (or empty): routing off."""
        if legs is None or len(legs) == 0:
            _check(self.lib.pp_set_route(self.h, 0, None, None, None))
            return
        lg = np.ascontiguousarray(legs, RouteLeg)
        rf = np.ascontiguousarray(route_first, np.int32)
        if self.n > 0 and len(rf) != self.n + 1:          # (no resident scenes: the library answers before it reads them)
            raise PlannerError(f"set_route: route_first needs {self.n + 1} entries (one per resident scene and the end), got {len(rf)}")
        m = default_route_model() if model is None else np.array(model, RouteModel).reshape(1).copy()
        _check(self.lib.pp_set_route(self.h, len(lg), _ptr(lg), _ptr(rf), _ptr(m)))

    # ---- a grid that follows the ego: the advance step re-centres grid_origin and goal ------
    def set_grid_follow(self, gf=None):
        """pp_set_grid_follow: from the next advance on the goal is point gf.goal_point of the followed path and the grid frame is
        held or re-centred on whole cells about ego and goal.  The model belongs to the handle: it survives
        set_scenes / set_egos / set_map.  gf None: following off."""
        if gf is None:
            _check(self.lib.pp_set_grid_follow(self.h, None))
            return
        m = np.array(gf, GridFollow).reshape(1).copy()
        _check(self.lib.pp_set_grid_follow(self.h, _ptr(m)))

    # ---- ego tracking model: the egos steer a bicycle model along the plan ---------------------
    def set_ego_tracker(self, tk=None):
        """pp_set_ego_tracker: from the next advance on every ego keeps a pose of its own - position, unit heading, curvature - and
        chases its planned path by pure pursuit instead of being put on it.  The model belongs to the handle: it
        survives set_scenes / set_egos / set_map (the per-scene states are re-derived).  tk None: tracking off."""
        if tk is None:
            _check(self.lib.pp_set_ego_tracker(self.h, None))
            return
        m = np.array(tk, EgoTracker).reshape(1).copy()
        _check(self.lib.pp_set_ego_tracker(self.h, _ptr(m)))

    def ego_track_state(self):
        """pp_get_ego_track_state: one EgoTrackState record per scene, a staged advance included (host wait)."""
        out = np.zeros(self.n, EgoTrackState)
        _check(self.lib.pp_get_ego_track_state(self.h, _ptr(out), self.n))
        return out

    # ---- lane traffic: scripted vehicles in the scenes' own obstacle entries -----------------
    def set_traffic(self, tracks=None, points=None, actors=None):
        """pp_set_traffic: TrafficTrack records (slices of `points`, GlobalPoint2D) and TrafficActor records; every staged input
        set then carries the actors at their arc length.  tracks / actors None (or no actors): traffic off."""
        if tracks is None or actors is None or len(actors) == 0:
            _check(self.lib.pp_set_traffic(self.h, 0, None, None, 0, 0, None))
            self.n_traffic = 0
            return
        tr = np.ascontiguousarray(tracks, TrafficTrack)
        pt = np.ascontiguousarray(points, GlobalPoint2D)
        ac = np.ascontiguousarray(actors, TrafficActor)
        _check(self.lib.pp_set_traffic(self.h, len(tr), _ptr(tr), _ptr(pt), len(pt), len(ac), _ptr(ac)))
        self.n_traffic = len(ac)

    def set_world_traffic(self, tracks=None, points=None, actors=None):
        """pp_set_world_traffic: as set_traffic, with TrafficActor.scene a WORLD of the fleet in force and TrafficActor.slot an own
        entry of every member scene of that world - one vehicle per world, written into every member and, with following on, led by
        the nearest of all the world's egos.  Needs set_fleet first; replaces whatever traffic the handle had.
        tracks / actors None (or no actors): traffic off."""
        if tracks is None or actors is None or len(actors) == 0:
            _check(self.lib.pp_set_world_traffic(self.h, 0, None, None, 0, 0, None))
            self.n_traffic = 0
            return
        tr = np.ascontiguousarray(tracks, TrafficTrack)
        pt = np.ascontiguousarray(points, GlobalPoint2D)
        ac = np.ascontiguousarray(actors, TrafficActor)
        _check(self.lib.pp_set_world_traffic(self.h, len(tr), _ptr(tr), _ptr(pt), len(pt), len(ac), _ptr(ac)))
        self.n_traffic = len(ac)

    def set_traffic_follow(self, tf=None):
        """pp_set_traffic_follow: from the next advance on every actor with speed > 0 follows the vehicle ahead of it on its track -
        an actor of its scene or the scene's ego - by the intelligent-driver model; speed is its desired speed.
        The model belongs to the handle and takes effect while traffic is set.  tf None: following off."""
        if tf is None:
            _check(self.lib.pp_set_traffic_follow(self.h, None))
            return
        m = np.array(tf, TrafficFollow).reshape(1).copy()
        _check(self.lib.pp_set_traffic_follow(self.h, _ptr(m)))

    # ---- episodic rollouts: ended egos restart on the device from start records ----------------
    def set_episodes(self, model=None, off=False):
        """pp_set_episodes: captures the resident SceneIn records and the SceneState array as start records, zeroes the stats and
        switches episodes on - from the next advance on an ego whose flag word meets model.end_mask, or whose episode reached
        model.max_ticks advances, restarts from them.  Call it after set_route / set_state / set_fleet /
        set_traffic: they do not touch the captured records.  model None: the default model.  off=True: episodes off, the stats
        stay readable and flagged egos freeze again."""
        if off:
            _check(self.lib.pp_set_episodes(self.h, None))
            return
        m = default_episode_model() if model is None else np.array(model, EpisodeModel).reshape(1).copy()
        _check(self.lib.pp_set_episodes(self.h, _ptr(m)))

    def episode_stats(self):
        """pp_get_episode_stats: one EpisodeStats record per scene, a staged advance included (host wait)."""
        out = np.zeros(self.n, EpisodeStats)
        _check(self.lib.pp_get_episode_stats(self.h, _ptr(out), self.n))
        return out

    def set_episode_spawn(self, sp, starts_in=None, starts_state=None):
        """pp_set_episode_spawn, after set_episodes: contact ends an episode (sp.contact), a restart draws one of
        sp.n_starts start records and skips those within sp.clearance of an obstacle of the scene's slice or an ego of its world
        (sp.check).  starts_in / starts_state: SceneIn / SceneState arrays of (n_starts - 1) * n records, record k (1 ..) of scene s
        at (k - 1) * n + s; record 0 is the capture of set_episodes.  sp None: the spawn model off, the stats stay readable."""
        if sp is None:
            _check(self.lib.pp_set_episode_spawn(self.h, None, None, None))
            return
        m = np.array(sp, EpisodeSpawn).reshape(1).copy()
        want = (int(m["n_starts"][0]) - 1) * self.n
        si = None if starts_in is None else np.ascontiguousarray(starts_in, SceneIn).reshape(-1)
        st = None if starts_state is None else np.ascontiguousarray(starts_state, SceneState).reshape(-1)
        for a, name in ((si, "starts_in"), (st, "starts_state")):
            if a is not None and 1 <= int(m["n_starts"][0]) <= EPISODE_MAX_STARTS and len(a) != want:          # (the library refuses the other counts)
                raise ValueError(f"{name}: {len(a)} records, n_starts and the resident scenes ask for {want}")
        _check(self.lib.pp_set_episode_spawn(self.h, _ptr(m), _ptr(si), _ptr(st)))

    def episode_spawn_stats(self):
        """pp_get_episode_spawn_stats: one EpisodeSpawnStats record per scene, a staged advance included (host wait)."""
        out = np.zeros(self.n, EpisodeSpawnStats)
        _check(self.lib.pp_get_episode_spawn_stats(self.h, _ptr(out), self.n))
        return out

    def set_episode_schedule(self, model=None, off=False):
        """pp_set_episode_schedule, after set_episode_spawn with order 0: from the next advance on the first choice
        of a restart is drawn by weights from the outcome counts per start record (model None: default_episode_schedule()).  The
        schedule is part of the spawn model in force: set_episode_spawn and whatever retires the spawn model leave none.
        off=True: the schedule off, the rows stay readable."""
        if off:
            _check(self.lib.pp_set_episode_schedule(self.h, None))
            return
        m = default_episode_schedule() if model is None else np.array(model, EpisodeSchedule).reshape(1).copy()
        _check(self.lib.pp_set_episode_schedule(self.h, _ptr(m)))
        self.episode_schedule_scope = int(m["scope"][0])

    def episode_schedule(self):
        """pp_get_episode_schedule: the EpisodeScheduleRow records - one in pooled scope, one per scene in per-scene scope -, a
        staged advance included (host wait)."""
        out = np.zeros(1 if getattr(self, "episode_schedule_scope", 1) == 1 else self.n, EpisodeScheduleRow)
        _check(self.lib.pp_get_episode_schedule(self.h, _ptr(out), len(out)))
        return out

    def set_episode_traffic(self, n_sets, starts=None):
        """pp_set_episode_traffic, after set_traffic, set_traffic_follow, set_episodes and set_episode_spawn: from
        the next advance on the actors of a scene whose ego restarts go back to a start state.  Set 0 is captured by the call (the
        current s and v of every actor); starts: TrafficStart records of sets 1 .. n_sets - 1, set k of actor a at
        (k - 1) * n_actors + a.  n_sets is 1 or the n_starts of the spawn model in force; 0: the reset off, the counters stay readable."""
        self._set_traffic_reset(self.lib.pp_set_episode_traffic, "n_traffic_reset", "actors", n_sets, starts)

    def episode_traffic_resets(self):
        """pp_get_episode_traffic_resets: how often every actor was put back on a start state since set_episode_traffic, a staged
        advance included (host wait)."""
        return self._traffic_resets(self.lib.pp_get_episode_traffic_resets, "n_traffic_reset")

    def _set_traffic_reset(self, call, count, who, n_sets, starts):
        """The set call of a traffic reset, per scene or per world; `count`: the attribute that keeps how many counters it has."""
        st = None if starts is None else np.ascontiguousarray(starts, TrafficStart).reshape(-1)
        want = (int(n_sets) - 1) * getattr(self, "n_traffic", 0)
        if st is not None and int(n_sets) >= 1 and len(st) != want:          # (the library refuses the other counts)
            raise ValueError(f"starts: {len(st)} records, n_sets and the {who} ask for {want}")
        _check(call(self.h, int(n_sets), _ptr(st)))
        if int(n_sets) > 0:
            setattr(self, count, getattr(self, "n_traffic", 0))          # (the counters outlive the traffic they counted)

    def _traffic_resets(self, call, count):
        out = np.zeros(getattr(self, count, 0), np.int32)
        _check(call(self.h, _ptr(out), len(out)))
        return out

    # ---- world episodes: the egos of a world restart together, with its vehicles -------------------
    def set_episode_worlds(self, on=True):
        """pp_set_episode_worlds, after set_episode_spawn: from the next advance on the WORLD (set_fleet; without a
        fleet: the scene) is the unit of an episode - when any ego of a world ends, every ego of it restarts on the same start record
        index.  Part of the spawn model in force: a later set_episode_spawn switches it off.  on False: off."""
        _check(self.lib.pp_set_episode_worlds(self.h, 1 if on else 0))

    def set_episode_world_traffic(self, n_sets, starts=None):
        """pp_set_episode_world_traffic, after set_world_traffic, set_traffic_follow and set_episode_worlds:
        set_episode_traffic for the vehicles of a world.  starts: TrafficStart records of sets 1 .. n_sets - 1, set k of vehicle a at
        (k - 1) * n_actors + a.  0: the reset off, the counters stay readable."""
        self._set_traffic_reset(self.lib.pp_set_episode_world_traffic, "n_world_traffic_reset", "vehicles", n_sets, starts)

    def episode_world_traffic_resets(self):
        """pp_get_episode_world_traffic_resets: how often every vehicle was put back on a start state since
        set_episode_world_traffic, a staged advance included (host wait)."""
        return self._traffic_resets(self.lib.pp_get_episode_world_traffic_resets, "n_world_traffic_reset")

    # ---- episode log: one record per ended episode, appended on the device ------------------------
    def set_episode_log(self, cap):
        """pp_set_episode_log, after set_episodes / set_episode_spawn / set_episode_traffic - call it last: from the
        next advance on every ended episode appends one EpisodeRecord to a ring of `cap` records on the device, in the order of the
        scene indices.  A second call starts a new log.  cap 0: the log off; what was logged stays readable."""
        _check(self.lib.pp_set_episode_log(self.h, int(cap)))
        if int(cap) > 0:
            self.episode_log_cap = int(cap)

    def read_episode_log(self, max_records=None):
        """pp_read_episode_log: (the oldest unread EpisodeRecord records still in the ring - at most max_records, by default all of
        them -, the number of records that were overwritten before a read saw them, newly counted by this call); a staged advance
        included (host wait).  What does not fit stays unread."""
        want = getattr(self, "episode_log_cap", 0) if max_records is None else int(max_records)
        out, lost = np.zeros(max(want, 1), EpisodeRecord), C.c_longlong()
        n = self.lib.pp_read_episode_log(self.h, _ptr(out), want, C.byref(lost))
        if n < 0:
            _check(n)
        return out[:n].copy(), lost.value

    def episode_log_info(self):
        """pp_get_episode_log_info: (records appended since set_episode_log, records overwritten unread so far - those the next
        read will report included); a staged advance included (host wait)."""
        total, lost = C.c_longlong(), C.c_longlong()
        _check(self.lib.pp_get_episode_log_info(self.h, C.byref(total), C.byref(lost)))
        return total.value, lost.value

    def set_traffic_manoeuvres(self, records=None):
        """pp_set_traffic_manoeuvres, after set_traffic and before set_episode_traffic: TrafficManoeuvre records, those
        of one actor contiguous and in list order, the actors non-decreasing.  records None (or none): off - every actor goes on as
        a plain actor of the track it is on."""
        m = np.zeros(0, TrafficManoeuvre) if records is None else np.ascontiguousarray(records, TrafficManoeuvre).reshape(-1)
        _check(self.lib.pp_set_traffic_manoeuvres(self.h, len(m), _ptr(m) if len(m) else None))

    def get_traffic_manoeuvre_state(self):
        """pp_get_traffic_manoeuvre_state: the TrafficManoeuvreState of every actor, as traffic_state gives the arc lengths (host wait)."""
        out = np.zeros(getattr(self, "n_traffic", 0), TrafficManoeuvreState)
        _check(self.lib.pp_get_traffic_manoeuvre_state(self.h, _ptr(out), len(out)))
        return out

    def traffic_speed(self):
        """pp_get_traffic_speed: the speed (m/s) of every actor, as traffic_state gives the arc lengths (host wait)."""
        out = np.zeros(getattr(self, "n_traffic", 0), np.float64)
        _check(self.lib.pp_get_traffic_speed(self.h, _ptr(out), len(out)))
        return out

    def traffic_state(self):
        """pp_get_traffic_state: the arc length of every actor in the input set get_scene_in reads (host wait)."""
        out = np.zeros(getattr(self, "n_traffic", 0), np.float64)
        _check(self.lib.pp_get_traffic_state(self.h, _ptr(out), len(out)))
        return out

    def get_obstacles(self, scene, cap=256):
        """pp_get_obstacles: the scene's obstacle slice - own entries, then peers - of the input set get_scene_in reads."""
        out = np.zeros(max(cap, 1), ObPoint)
        n = self.lib.pp_get_obstacles(self.h, int(scene), _ptr(out), cap)
        if n > cap:
            return self.get_obstacles(scene, n)
        if n < 0:
            _check(n)
        return out[:n].copy()

    def fetch_async(self, plan=None, grid=None):
        """pp_fetch_async of the last enqueued tick into `plan` / `grid` (pinned arrays of self.n records). Returns the tick id."""
        t = C.c_longlong()
        _check(self.lib.pp_fetch_async(self.h, _ptr(plan), _ptr(grid), C.byref(t)))
        return t.value

    def fetch_published_async(self, result=None, show=None, grid=None):
        """pp_fetch_published_async: PlanningOut / PlanningStatus arrays (what the reference publishes) and / or GridOut of the last tick."""
        t = C.c_longlong()
        _check(self.lib.pp_fetch_published_async(self.h, _ptr(result), _ptr(show), _ptr(grid), C.byref(t)))
        return t.value

    def set_packed_fetch(self, on=True):
        """pp_set_packed_fetch: arm (or disarm) the packed streamed fetch - every later tick packs its results on the device."""
        _check(self.lib.pp_set_packed_fetch(self.h, int(bool(on))))

    def fetch_packed_async(self, plan=None, grid=None):
        """pp_fetch_packed_async: PackedPlan / PackedGrid arrays (pinned, self.n records) of the last tick. Returns the tick id;
        unpack_plan / unpack_grid rebuild what fetch_async would have delivered."""
        t = C.c_longlong()
        _check(self.lib.pp_fetch_packed_async(self.h, _ptr(plan), _ptr(grid), C.byref(t)))
        return t.value

    def unpack_plan(self, packed, **kw):
        return unpack_plan(self.cfg, packed, **kw)

    def unpack_grid(self, packed, out=None):
        return unpack_grid(self.cfg, packed, out)

    def wait_tick(self, tick_id, allow_poisoned=False):
        """pp_wait_tick: host wait for that tick's downloads. Returns the number of poisoned scenes (raises on any unless allowed)."""
        bad = C.c_int()
        rc = self.lib.pp_wait_tick(self.h, tick_id, C.byref(bad))
        if rc != 0 and not (allow_poisoned and bad.value > 0):
            _check(rc)
        return bad.value

    def tick_id(self):
        return self.lib.pp_tick_id(self.h)

    def device_synchronize(self):
        """pp_device_synchronize: pp_sync + hipDeviceSynchronize (what torch.cuda.synchronize() does, without torch)."""
        _check(self.lib.pp_device_synchronize(self.h))

    def join(self):
        """pp_join: the handle's stream waits (on the device) for every tick enqueued so far."""
        _check(self.lib.pp_join(self.h))

    def get_plan(self):
        out = np.zeros(self.n, PlanOut)
        _check(self.lib.pp_get_plan(self.h, _ptr(out), self.n))
        return out

    def get_state(self):
        out = np.zeros(self.n, SceneState)
        _check(self.lib.pp_get_state(self.h, _ptr(out), self.n))
        return out

    def get_grid_out(self):
        out = np.zeros(self.n, GridOut)
        _check(self.lib.pp_get_grid_out(self.h, _ptr(out), self.n))
        return out

    def get_grid(self, scene):
        w, hgt = int(self.cfg["grid_w"][0]), int(self.cfg["grid_h"][0])
        out = np.zeros((hgt, w), np.uint8)
        _check(self.lib.pp_get_grid(self.h, scene, _ptr(out)))
        return out

    def search_info(self):
        """(LDS budget in words per view, words the densest scene needed, scenes of the last tick on the dense path)."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(self.lib.pp_get_search_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def get_order(self, scene, n):
        out = np.zeros(max(n, 1), np.int32)
        _check(self.lib.pp_get_order(self.h, scene, _ptr(out), n))
        return out[:n]

    def get_path(self, scene, n):
        out = np.zeros(max(n, 1), np.int32)
        _check(self.lib.pp_get_path(self.h, scene, _ptr(out), n))
        return out[:n]

    def get_refpath(self, scene, n):
        out = np.zeros(max(n, 1), GlobalPoint2D)
        _check(self.lib.pp_get_refpath(self.h, scene, _ptr(out), n))
        return out[:n]

    def plan_tick_batch(self, sc, state, with_motion=True, want_grid=True):
        """One-shot upload + tick + download (pp_plan_tick_batch). Updates `state` in place."""
        n = len(sc["scene_in"])
        plan = np.zeros(n, PlanOut)
        gout = np.zeros(n, GridOut) if want_grid else None
        _check(self.lib.pp_plan_tick_batch(self.h, n, _ptr(sc["scene_in"]), _ptr(sc["obs_pool"]),
                                           _ptr(sc["mot_pool"]) if with_motion else None, n * sc["n_obs"],
                                           _ptr(sc["lane_pool"]), _ptr(sc.get("attr_pool")), len(sc["lane_pool"]),
                                           _ptr(sc["ref_pool"]),
                                           len(sc["ref_pool"]), _ptr(state), _ptr(plan), _ptr(gout)))
        self.n = n
        return plan, gout

    # ---- stand-alone operators --------------------------------------------------------
    def search_obstacle_batch(self, paths, path_off, obs, obs_off, lat_lo, lat_hi):
        nq = len(lat_lo)
        out = np.zeros(nq, Path_Obs)
        _check(self.lib.pp_search_obstacle_batch(self.h, nq, _ptr(paths), _ptr(path_off), _ptr(obs), _ptr(obs_off),
                                                 _ptr(lat_lo), _ptr(lat_hi), _ptr(out)))
        return out

    def geom_batch(self, op, a, b=None, c=None):
        n = len(a)
        out = np.zeros(n, np.float64)
        _check(self.lib.pp_geom_batch(self.h, op, n, _ptr(a), _ptr(b), _ptr(c), _ptr(out)))
        return out

    def scalar_stage(self, op, args, last_Bpoints=None, n_out=3):
        a = np.asarray(args, np.float64).copy()
        out = np.zeros(n_out, np.float64)
        _check(self.lib.pp_scalar_stage(self.h, op, _ptr(a), len(a), _ptr(last_Bpoints), _ptr(out), n_out))
        return out

    def bezier(self, start, end, n=PATH_POINTS):
        out = np.zeros(n, GlobalPoint2D)
        _check(self.lib.pp_bezier(self.h, _P3(*start), _P3(*end), _ptr(out), n))
        return out

    def mean_points(self, pts, n_out=PATH_POINTS):
        out = np.zeros(n_out, GlobalPoint2D)
        _check(self.lib.pp_mean_points(self.h, _ptr(pts) if len(pts) else None, len(pts), _ptr(out), n_out))
        return out

    def create_new_path(self, path, offset):
        out = np.zeros(len(path), GlobalPoint2D)
        _check(self.lib.pp_create_new_path(self.h, _ptr(path), len(path), float(offset), _ptr(out)))
        return out

    # ---- measurement -------------------------------------------------------------------
    def set_profile(self, on):
        _check(self.lib.pp_set_profile(self.h, int(on)))

    def reset_kernel_ms(self):
        _check(self.lib.pp_reset_kernel_ms(self.h))

    def kernel_ms(self):
        out = {}
        names = K_NAMES if hasattr(self.lib, "pp_set_perception") else K_NAMES[:7] if hasattr(self.lib, "pp_set_packed_fetch") else K_NAMES[:5]      # (an older build named through DMPP_LIB)
        for k, name in enumerate(names):
            ms, cnt = C.c_float(), C.c_int()
            _check(self.lib.pp_get_kernel_ms(self.h, k, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    def device_ptr(self, which):
        sz = C.c_size_t()
        p = self.lib.pp_device_ptr(self.h, which, C.byref(sz))
        return p, sz.value

    def write_device(self, which, array):
        """Host wait (pp_sync), then a blocking hipMemcpy of `array` over the start of the handle's buffer `which` (pp_device_ptr):
        inputs written where an RCCL scatter would put them, or records a test puts in the place of a finished tick's."""
        global _hip
        self.sync()
        ptr, size = self.device_ptr(which)
        raw = np.frombuffer(np.ascontiguousarray(array).tobytes(), np.uint8)
        if not ptr or raw.size > size:
            raise PlannerError(f"write_device: buffer {which} holds {size} B, the array has {raw.size} B")
        if _hip is None:
            _hip = C.CDLL("libamdhip64.so")          # the runtime the process already has (libdmpp.so is loaded)
            _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = _hip.hipMemcpy(ptr, raw.ctypes.data, raw.size, 1)          # hipMemcpyHostToDevice
        if rc != 0:
            raise PlannerError(f"write_device: hipMemcpy failed with {rc}")

    def read_device(self, which, dtype, count):
        """The counterpart of write_device: host wait (pp_sync), then a blocking hipMemcpy of the first `count` records of the
        handle's buffer `which` (pp_device_ptr) into a new array - pool entries no getter returns (a test reads the peer slots
        beyond obs_n and the motion pool of the current input set)."""
        global _hip
        self.sync()
        ptr, size = self.device_ptr(which)
        out = np.zeros(int(count), dtype)
        if not ptr or out.nbytes > size:
            raise PlannerError(f"read_device: buffer {which} holds {size} B, {out.nbytes} B were asked for")
        if _hip is None:
            _hip = C.CDLL("libamdhip64.so")
            _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if out.nbytes:
            rc = _hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2)          # hipMemcpyDeviceToHost
            if rc != 0:
                raise PlannerError(f"read_device: hipMemcpy failed with {rc}")
        return out
