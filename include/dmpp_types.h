/*
 * dmpp_types.h — plain-C data types of the planning hot path.
 *
 * The reference defines none of these: every struct below lives in its unshipped
 * `Share.h` (included at Planning.h:2 / Decision.h:2).  Field sets are exactly the
 * fields the reference touches; scalar widths and layouts are
 * chosen here and are part of this library's ABI.  Coordinates are `double`
 * (the only width consistent with every use in Planning.cpp / Decision.cpp).
 *
 * This header is pure C99, shared by the C-ABI (`dmpp_planner.h`), the C++ host
 * classes, the HIP kernels and — as data layout only — the CPU oracle.
 */
#ifndef DMPP_TYPES_H
#define DMPP_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fixed sizes taken from the reference ------------------------------------ */
#define DMPP_PATH_POINTS   200 /* GlobalPoint2D road_points[200]    Planning.cpp:115, Planning.h:33 */
#define DMPP_OUT_POINTS    100 /* every 2nd point is published      Planning.cpp:180-183,205-212    */
#define DMPP_FRONT_POINTS  120 /* corridor ahead  "120 points ~60m" Decision.cpp:581                */
#define DMPP_REAR_POINTS    40 /* corridor behind "40 points  ~20m" Decision.cpp:590                */
#define DMPP_STUB_NEXT_PTS  60 /* exit-lane points added in a junction, Decision.cpp:446            */
#define DMPP_LANESUM         8 /* LocationOut.id[LANESUM]; value is build-chosen       */
#define DMPP_MAX_SWEEP       8 /* lateral sweep candidates per side bound (BYTE i loop, Decision.cpp:940) */
#define DMPP_MAX_REFPATH   512 /* cap on DecisionOut.refpath length carried on device               */

/* ---- geometry (Share.h types) ------------------------------------- */
typedef struct GlobalPoint2D { double x, y; } GlobalPoint2D;             /* 16 B */
typedef struct GlobalPoint3D { double x, y, dir; } GlobalPoint3D;        /* 24 B; dir: degrees CCW from east */
typedef struct GPSPoint2D    { double lat, lng; } GPSPoint2D;

/* AimPoint{Aim_point, Aim_id}: Planning.cpp:418-421 */
typedef struct AimPoint { GlobalPoint3D Aim_point; int32_t Aim_id; int32_t _pad; } AimPoint; /* 32 B */

/* ObPoint is opaque in the reference (no field is ever read).  24 B as SURVEY §8
 * prices it: position + type, the pad word carries the footprint radius the grid
 * engine rasterises (metres, f32). */
typedef struct ObPoint { double x, y; int32_t type; float radius; } ObPoint;        /* 24 B */
/* constant-velocity model for dynamic obstacles (row G4; Decision.h:14-15 declares
 * dynamic-obstacle lists the reference never fills). m/s in world axes. */
typedef struct ObMotion { double vx, vy; } ObMotion;

/* map element: planning_MapData[road][lane][id] -> {global_point, lane_sum,
 * lanechg_attribute, lane_width(cm)}  (Decision.cpp:563,566,578; Planning.cpp:413-420).
 * On this ABI a lane is a flat array of GlobalPoint3D; the per-lane scalars travel in
 * LaneView. */
typedef struct LaneView {
    int32_t cur_off,   cur_n;   /* current lane  : points [cur_off, cur_off+cur_n) of the lane-point pool */
    int32_t left_off,  left_n;  /* left  lane (lane_num-2); n = 0 when absent   Planning.cpp:359-368 */
    int32_t right_off, right_n; /* right lane (lane_num);   n = 0 when absent   Planning.cpp:371-380 */
    int32_t lane_sum;           /* [0].lane_sum                                 Planning.cpp:331      */
    int32_t lanechg_attribute;  /* 0 none,1 left,2 right,3 both at ego id       Decision.cpp:566      */
    double  lane_width;         /* metres (= lane_width/100.0)                  Decision.cpp:578      */
} LaneView;                                                                  /* 40 B */

/* LocationOut: fields read on the path. */
typedef struct LocationOut {
    GlobalPoint3D globalpoint;        /* ego pose                                   Planning.cpp:599,637 */
    double  velocity;                 /* km/h                                       Planning.cpp:258     */
    int32_t pos;                      /* 0 road, 1 pre-junction, 2 junction         Planning.cpp:247     */
    int32_t road_num, lane_num;       /* 1-based                                    Planning.cpp:329-330 */
    int32_t last_roadnum, next_roadnum, last_lanenum, next_lanenum;
    int32_t path_num;
    int32_t id[DMPP_LANESUM];         /* ego point id on each lane                  Planning.cpp:338     */
} LocationOut;                                                              /* 96 B */

/* DecisionOut (Decision.cpp:187-196) minus the std::vector and the two period fields: refpath is flattened to
 * (offset,len) into a point pool at the C-ABI.  The C++ host surface (host/dmpp_share.hpp) declares
 * `struct DecisionOut` - the type the reference's methods take, Planning.h:57-75 - on top of this POD. */
typedef struct DecisionOutPod {
    double  velocity_expect;
    int32_t behavior;         /* 1 keep,2 left chg,3 right chg,4 left avoid,5 right avoid,6 grid search (Decision.h:36) */
    int32_t target_roadnum, target_lanenum;
    int32_t light;            /* 0 none,1 left,2 right,3 hazard (Decision.h:39) */
    int32_t behavior_to_dlg;
    int32_t refpath_n;        /* number of valid refpath points (<= DMPP_MAX_REFPATH) */
} DecisionOutPod;                                                           /* 32 B */

/* Obs_To_Veh / Path_Obs: Decision.cpp:847-850 */
typedef struct Obs_To_Veh { double dis_lat, dis_lng; } Obs_To_Veh;
typedef struct Path_Obs {
    Obs_To_Veh Ob_Pose;
    ObPoint    Ob_Attr;
    int32_t    Obs_flag;
    int32_t    Ob_Pathid;
} Path_Obs;                                                                 /* 48 B */

/* Behavior_Dec: Decision.cpp:286-291 */
typedef struct Behavior_Dec {
    int32_t behavior, light_status, target_lanenum;
    int32_t lanechg_status, obsavoid_status, behavior_to_dlg;
} Behavior_Dec;

/* PlanningOut (Planning.cpp:189-212) */
typedef struct PlanningOut {
    double  brakedis, brake_speed, desacc, desspd, desstr, radius;
    int32_t cnt, APA, desaccVd, desstrVd, light, road_type, sstop, _pad;
    GlobalPoint2D pnts[DMPP_OUT_POINTS];      /* .x = lat, .y = lng */
} PlanningOut;                                                              /* 1680 B */

/* PlanningStatus (Planning.cpp:174-183) */
typedef struct PlanningStatus {
    double  near_ob_dist, planspeed, planacc;
    int32_t afresh_cause, trafficlight;
    GlobalPoint2D path_points[DMPP_OUT_POINTS];
} PlanningStatus;                                                           /* 1632 B */

/* ---- per-scene cross-tick state ------------------------------------------------
 * Everything the reference keeps in statics / members between ticks
 * (Planning.cpp:6,52-53,216-223; Planning.h:20-23,42-52; Decision.cpp:199-201,915-917;
 * Decision.h:27-44) made explicit so scenes are independent and batchable. */
typedef struct SceneState {
    GlobalPoint2D last_Bpoints[DMPP_PATH_POINTS];   /* Planning.h:33               3200 B */
    AimPoint aimpoint_far, aimpoint_near;           /* Planning.h:22-23 (stale across ticks by design) */
    double  path_lat_dis, remain_dis, path_dir_err; /* Planning.h:42-46 */
    double  brakespeed, des_acc;                    /* Planning.h:50-52 */
    float   faraim_dis, nearaim_dis;                /* FLOAT members, Planning.h:20-21 */
    int32_t path_near_id, path_front_near_id;       /* Planning.h:47-48 */
    int32_t his_behavior;                           /* Planning.h:49, ctor sets 1 (Planning.cpp:10) */
    int32_t afresh_planning, afresh_cause;          /* Planning.h:43-44 */
    int32_t acc_flag;                               /* Planning.h:51 */
    int32_t count;                                  /* BYTE count, Planning.cpp:51,219-223 */
    /* Decision side */
    int32_t z_behavior, z_light_status, z_target_lanenum, z_target_roadnum; /* Decision.h:36-39 */
    int32_t z_behavior_to_dlg;                                              /* Decision.h:27    */
    int32_t z_segment_lanechg_status, z_segment_obsavoid_status;            /* Decision.h:28-29 */
    int32_t d_his_behavior, d_his_light_status, d_his_target_lanenum;       /* Decision.h:41-44 */
    uint32_t obsavoid_time, no_obsaviod_time, frontobs_time;                /* statics, Decision.cpp:915-917 */
    int32_t tick;                                   /* ticks elapsed; drives the dynamic-obstacle model (G4) */
    int32_t _pad;
    double  z_velocity_expect;                      /* Decision.h:47 */
    double  leftlight_time, rightlight_time;        /* Decision.h:31-32: turn-signal timers, ms */
} SceneState;

/* ---- per-scene per-tick input ---------------------------------------------------- */
typedef struct SceneIn {
    LocationOut loc;          /* app->GetLocationOut()   Planning.cpp:101 */
    DecisionOutPod dec;       /* app->GetDesicionOut()   Planning.cpp:96  — used as is when the decision stage is off */
    LaneView    lanes;        /* slice of the lane-point pool standing in for planning_MapData */
    int32_t ref_off, ref_n;   /* DecisionOut.refpath / junction polyline: slice of the refpath pool */
    int32_t obs_off, obs_n;   /* app->GetObj() snapshot: slice of the obstacle pool (Planning.cpp:111) */
    int32_t stub_attribute;   /* z_RoadNavi[path_num].stub_attribute, Decision.cpp:385 */
    int32_t _pad;
    /* lane-change rule tree inputs (Decision.cpp:685-738, 1011-1772) */
    uint16_t out_lane_no[DMPP_LANESUM]; /* z_RoadNavi[path_num].out_lane_no[]: exit lanes of this road, 0-terminated (Decision.cpp:696) */
    double   period_last;     /* z_period_last: milliseconds since the previous decision tick (Decision.cpp:137) */
    /* grid engine (rows G1-G4; absent from the reference) */
    GlobalPoint2D grid_origin;/* world coordinates of the corner of cell (0,0) */
    GlobalPoint2D goal;       /* goal position, world */
} SceneIn;

/* ---- closed-loop rollout (build-defined: the reference has no vehicle) ----------------------
 * pp_advance_async moves every ego along the path its last tick planned.  EgoModel: the time step and the
 * acceleration limits of the speed ramp, and how many lane points ahead of its id a lane view is searched. */
typedef struct EgoModel {
    double  dt;                 /* seconds per tick                                            */
    double  max_acc, max_dec;   /* m/s^2: most the speed rises / falls towards result.desspd   */
    int32_t window;             /* lane points searched from each id, [id, id + window)        */
    int32_t _pad;
} EgoModel;                                                                 /* 32 B */
/* sticky per-scene flags of the rollout; a scene that carries any is frozen (its SceneIn is carried over) */
#define DMPP_EGO_PATH_END  1   /* the step reached past point 199 of the path: the ego stopped there           */
#define DMPP_EGO_BAD_PATH  2   /* a non-finite coordinate (or step length) on the walked part: loc untouched   */
#define DMPP_EGO_LANE_END  4   /* the current id came within `window` points of the end of its lane            */
#define DMPP_EGO_OFF_GRID  8   /* grid stage on and the new position lies outside the scene's grid             */
/* the ego one tick plans from, as pp_advance_async produced it */
typedef struct EgoTrace {
    GlobalPoint3D pose;
    double  velocity;           /* km/h */
    int32_t id_cur, lane_num, flags, _pad;
} EgoTrace;                                                                 /* 48 B */

/* ---- map store ------------------------------------------------------
 * planning_MapData[road][lane][id] / decision_MapData (Planning.cpp:331-356; Decision.cpp:562-578) and
 * planning_InterMapData[last_road][next_road][last_lane][next_lane][id] (Planning.cpp:342; Decision.cpp:348)
 * flattened: one point pool shared by every scene, structure-of-arrays for the per-point attributes, a lane
 * table indexed through the roads' first-lane offsets, and a junction table.  Roads and lanes are 1-based as
 * in the reference; lane l of road r is lanes[road_first_lane[r-1] + l-1]. */
typedef struct MapLane {
    int32_t point_off, n_points;   /* points [point_off, point_off + n_points) of the point pool        */
    int32_t lane_sum;              /* [road][lane][0].lane_sum                       Planning.cpp:331    */
    int32_t _pad;
} MapLane;
typedef struct MapJunction {
    int32_t last_road, next_road, last_lane, next_lane;   /* the four indices of planning_InterMapData, 1-based */
    int32_t point_off, n_points;   /* slice of the junction point pool                                   */
} MapJunction;
typedef struct MapDesc {
    int32_t n_roads, n_lanes, n_points, n_junctions, n_jpoints, _pad;
    const int32_t*       road_first_lane;     /* n_roads + 1 entries                                        */
    const MapLane*       lanes;               /* n_lanes                                                    */
    const GlobalPoint3D* points;              /* n_points: global_point                                     */
    const uint8_t*       lanechg_attribute;   /* n_points: 0 none, 1 left, 2 right, 3 both  Decision.cpp:566 */
    const uint16_t*      lane_width_cm;       /* n_points: centimetres                      Decision.cpp:578 */
    const MapJunction*   junctions;           /* n_junctions                                                */
    const GlobalPoint2D* jpoints;             /* n_jpoints: junction polylines                              */
} MapDesc;

/* ---- grid-engine result (rows G2,G3) ---------------------------------------------- */
#define DMPP_G_FOUND      0
#define DMPP_G_NO_PATH    1   /* open set exhausted */
#define DMPP_G_LIMIT      2   /* max_expansions reached */
#define DMPP_G_OVERFLOW   3   /* more than bucket_cap live open-list entries */
#define DMPP_G_GOAL_BLOCKED 4 /* goal cell occupied: no search run */
#define DMPP_G_PATH_TRUNC 5   /* path longer than max_path cells */
#define DMPP_G_INTERNAL   6   /* a loop bound of the device search was hit: never expected, reported instead of hanging */
#define DMPP_G_COST_RANGE 7   /* a successor's f = g + h reached DMPP_F_LIMIT: only `status` is defined (as for OVERFLOW) */
#define DMPP_G_STATUS_COUNT 8

#define DMPP_JPS_BATCH 4       /* entries of the minimal f taken per step of the jump-point search */
#define DMPP_DIAG_JUMP 8       /* cells a diagonal jump of the jump-point search looks ahead before it settles for a plain node */
#define DMPP_OPEN_CAP 512      /* open-list slots the device keeps in LDS (496 is the most any generated scene needs); beyond them the entries
                                  that pop last live in a spill area in HBM, up to bucket_cap: a storage detail, not a limit of the specification */

/* f = g + h of an open-list entry must stay below this (the device keeps f/2 in 16 bits, 0xFFFF = dead slot): ~13,000
 * straight cells of detour.  A push that would reach it ends the search with DMPP_G_COST_RANGE, checked - per push, in
 * push order - before the open-list capacity. */
#define DMPP_F_LIMIT 131070

#define DMPP_MAX_LATTICE 17   /* n_lattice Bezier candidates + 1 grid-path candidate */

typedef struct GridOut {
    uint64_t order_digest;    /* sum over expansions of mix64(seq<<32 | cell)   */
    int32_t  status;
    int32_t  n_expanded;      /* closed cells, in expansion order                      */
    int32_t  n_pushed;        /* open-set insertions                                   */
    int32_t  n_rounds;        /* distinct f levels visited                             */
    int32_t  path_len;        /* cells on the chosen path, start..goal inclusive       */
    int32_t  path_cost;       /* integer g at the goal (10 straight / 14 diagonal)     */
    int32_t  start_cell, goal_cell;
    int32_t  best_candidate;  /* argmin of cand_cost, ties to the lowest index         */
    int32_t  n_candidates;
    double   cand_cost[DMPP_MAX_LATTICE];
    double   cand_col[DMPP_MAX_LATTICE], cand_curv[DMPP_MAX_LATTICE], cand_prog[DMPP_MAX_LATTICE];
    GlobalPoint2D best_path[DMPP_PATH_POINTS];
} GridOut;

/* ---- per-scene per-tick output ------------------------------------------------------ */
typedef struct PlanOut {
    PlanningOut    result;      /* what SetUdpSendCtrl receives, Planning.cpp:214 */
    PlanningStatus show;        /* what SetPlanningStatus receives, Planning.cpp:186 */
    GlobalPoint2D  road_points[DMPP_PATH_POINTS];  /* the 200-point path of this tick */
    Path_Obs       around[6];   /* F,R,LF,LR,RF,RR  (Decision.cpp:847-880) */
    DecisionOutPod dec;         /* decision published this tick (Decision.cpp:187-196) */
    double         ob_dis_lat, ob_dis_lng;   /* SearchObstacle outputs of Planning.cpp:168 */
    ObPoint        ob;
    int32_t        ob_flag, ob_pathid;
    int32_t        sweep_side, sweep_index;  /* which candidate of Decision.cpp:940-973 was accepted (-1 none) */
    int32_t        navi_lanechg;             /* Nav_LaneChange result, Decision.cpp:685-738: 0 none, 1 left, 2 right */
    int32_t        navi_lanechg_times;       /* CalcNaviLaneChgTimes, Decision.cpp:498-538 */
} PlanOut;

/* ---- packed streamed fetch (build-defined) --------------------------------------------------------
 * pp_set_packed_fetch makes every tick pack its results on the device into one PackedPlan (and, with the grid stage, one
 * PackedGrid) per scene; pp_fetch_packed_async downloads those, and pp_unpack_plan / pp_unpack_grid - pure host code - rebuild
 * PlanningOut, PlanningStatus, DecisionOutPod and GridOut from them, byte for byte.  Every byte of both records is specified. */
typedef struct PackedPlan {
    double  brakedis, brake_speed, desacc, desspd, desstr, radius;     /* PlanOut.result, its six doubles ...              */
    int32_t cnt, APA, desaccVd, desstrVd, light, road_type, sstop;     /* ... and its seven ints                           */
    int32_t afresh_cause;             /* PlanOut.show.afresh_cause, in the place of result._pad (always 0 on the device)  */
    double  near_ob_dist, planspeed, planacc;                          /* PlanOut.show                                     */
    int32_t trafficlight;             /* PlanOut.show.trafficlight                                                         */
    int32_t ob_flag;                  /* PlanOut.ob_flag                                                                   */
    DecisionOutPod dec;               /* PlanOut.dec                                                                       */
    GlobalPoint2D path_points[DMPP_OUT_POINTS];   /* PlanOut.show.path_points; result.pnts is their WGS84 image (unpacker) */
} PackedPlan;                                                               /* 1744 B */

#define DMPP_PACKED_NONE    0   /* PackedGrid.kind: no candidate, best_path is zeros                                      */
#define DMPP_PACKED_LATTICE 1   /* a lattice candidate won: geo = its four control points                                 */
#define DMPP_PACKED_PATH    2   /* the grid-path candidate won: geo[0..1] = grid origin, planes = the steps of the prefix  */
#define DMPP_PACKED_BAD     4   /* bit 2 of kind: the path cells were no chain of neighbours from start_cell (never expected) */
typedef struct PackedGrid {
    uint64_t order_digest;            /* the first 48 B of GridOut as they stand ...                                       */
    int32_t  status, n_expanded, n_pushed, n_rounds, path_len, path_cost, start_cell, goal_cell, best_candidate, n_candidates;
    double   best_cost, best_col, best_curv, best_prog;   /* cand_*[best_candidate]; 0 when n_candidates == 0              */
    int32_t  kind;                    /* DMPP_PACKED_NONE / LATTICE / PATH, | DMPP_PACKED_BAD                              */
    int32_t  n_steps;                 /* kind PATH: min(path_len - 1, lookahead_cells, 199); otherwise 0                   */
    double   geo[8];                  /* LATTICE: x0 y0 x1 y1 x2 y2 x3 y3; PATH: grid_origin.x, .y, then 0; NONE: 0        */
    uint64_t planes[12];              /* PATH: bit i & 63 of planes[3 (i >> 6) + b] = bit b of the direction of step i     */
} PackedGrid;                                                               /* 248 B */

/* ---- rollout scorecard (build-defined) ------------------------------------------------------
 * One record per scene, folded on the device over the ticks scored between pp_score_begin and pp_score_end, in tick
 * order.  Tick indices are 0-based counts of scored ticks; obstacle indices count within the scene's slice.  Every field is
 * specified exactly (§4d): a numpy restatement gives the same bytes. */
typedef struct RolloutScore {
    double  min_clearance;          /* smallest clearance_t (m); +inf while no tick had one                          */
    double  dist;                   /* sum over ticks of the distance between successive ego positions (m)           */
    double  max_speed;              /* largest loc.velocity (km/h); starts at 0                                      */
    double  max_acc, max_dec;       /* largest rise / fall of the speed between successive ticks (m/s^2, both >= 0)  */
    GlobalPoint2D last_pos;         /* ego position of the last scored tick                                          */
    double  last_speed;             /* ... and its loc.velocity (km/h)                                               */
    int32_t n_ticks;                /* ticks scored                                                                  */
    int32_t min_clearance_tick, min_clearance_obs;       /* where min_clearance first occurred; -1, -1 while none    */
    int32_t first_collision_tick, n_collision_ticks;     /* ticks with clearance_t <= 0; first: -1 while none        */
    int32_t n_replans;              /* ticks that left SceneState.afresh_planning != 0                               */
    int32_t n_ob_flag, n_desacc;    /* ticks with PlanOut.ob_flag != 0; with PlanOut.result.desaccVd != 0            */
    int32_t behavior_ticks[8];      /* histogram of PlanOut.dec.behavior clamped to 0..7                             */
    int32_t ego_flags;              /* DMPP_EGO_* word the ego of the last scored tick carried                       */
    int32_t _pad;
    /* grid half (k_score_grid): only ticks that ran the grid stage */
    int32_t n_grid_ticks;
    int32_t n_grid_path_candidate;  /* ticks whose grid-path candidate (the last one) was the best                   */
    int32_t grid_status_ticks[DMPP_G_STATUS_COUNT];      /* histogram of GridOut.status; out of range: DMPP_G_INTERNAL */
} RolloutScore;                                                             /* 176 B */

/* ---- fleet coupling (build-defined: the reference has no fleet) ------------------------------
 * pp_set_fleet groups the resident scenes into worlds; after every staged input set the nearest egos of a scene's own
 * world are written into the peer slots behind its obstacle slice.  FleetModel: how far an ego sees its peers, the
 * footprint radius a peer is given as an obstacle, and how many peer slots every scene gets. */
typedef struct FleetModel {
    double  range;              /* metres: a peer is a candidate when its squared distance is <= range * range   */
    float   radius;             /* ObPoint.radius of a peer slot (metres)                                        */
    int32_t max_peers;          /* K: peer slots per scene, 0 .. DMPP_FLEET_MAX_PEERS                            */
} FleetModel;                                                               /* 16 B */
#define DMPP_FLEET_MAX_PEERS 64
/* ObPoint.type of a peer slot: DMPP_OB_PEER | scene index of the peer (nothing on the device reads `type`; it travels
 * into PlanOut.ob.type / PlanOut.around[k].Ob_Attr.type and tells the caller WHICH ego was in the way) */
#define DMPP_OB_PEER 0x40000000

/* ---- route following (build-defined: the simulated localisation module of a rollout) --------
 * pp_set_route gives every scene a route: a run of RouteLeg records, one per road it drives.  The advance step then
 * moves a routed ego road -> pre-junction -> junction -> next road; loc.path_num is the 0-based index of the ego's
 * current leg within its own route. */
typedef struct RouteLeg {               /* one z_RoadNavi entry (PathInfo): what Decision.cpp reads of it */
    int32_t  road_num;                  /* 1-based road of this leg                                       */
    int32_t  stub_attribute;            /* Decision.cpp:385,470                                           */
    uint16_t out_lane_no[DMPP_LANESUM]; /* exit lanes of this road, 0-terminated (Decision.cpp:696)       */
} RouteLeg;                                                                 /* 24 B */
typedef struct RouteModel {
    int32_t pre_points;                 /* lane points before the end of a lane from which the ego is in the pre-junction */
    int32_t _pad;
} RouteModel;                                                               /* 8 B */
#define DMPP_EGO_ROUTE_END 16  /* the ego came to the end of the LAST leg of its route: it arrived                */

/* ---- a grid that follows the ego (build-defined) ---------------------------------------------
 * pp_set_grid_follow makes the advance step keep SceneIn.grid_origin and SceneIn.goal with the ego: the goal is a point of
 * the path the last tick planned, and the grid frame is re-centred - on whole cells - on the midpoint of ego and goal
 * whenever either of them comes within margin_cells of its edge. */
typedef struct GridFollow {
    int32_t goal_point;    /* index into PlanOut.road_points the goal is taken from, 1 .. DMPP_PATH_POINTS - 1 */
    int32_t margin_cells;  /* the frame is held while ego and goal lie at least this many cells inside it      */
} GridFollow;              /* 8 B */

/* ---- ego tracking model (build-defined) -------------------------------------------------------
 * pp_set_ego_tracker gives every rollout ego a pose of its own: the advance step no longer puts the ego ON its planned path
 * but integrates position, heading and curvature as a kinematic bicycle that chases the path by pure pursuit.  The look-ahead
 * is ld = look_min + look_gain * v / 3.6 metres (v: the new speed, km/h). */
typedef struct EgoTracker {
    double  look_min;      /* m; > 0                                                                          */
    double  look_gain;     /* s; >= 0                                                                         */
    double  max_curv;      /* 1/m; the bound on the commanded |curvature|; > 0                                */
    double  curv_rate;     /* 1/(m s); the most the curvature state changes per second; > 0                   */
    double  curv_bias;     /* 1/m; a steering misalignment, added to the applied curvature after the limits   */
    int32_t n_sub;         /* substeps of the motion per advance, 1 .. 8                                      */
    int32_t _pad;
} EgoTracker;              /* 48 B */
typedef struct EgoTrackState {          /* one per scene; every byte is specified (§4q) */
    double   hx, hy;                    /* unit heading vector                                                         */
    double   kappa;                     /* curvature state, 1/m (without curv_bias)                                    */
    uint64_t key_x, key_y, key_dir;     /* the bits of loc.globalpoint this model last stored into SceneIn             */
    double   max_kappa;                 /* the largest |kappa| seen                                                    */
    int32_t  valid;                     /* 0: the state is re-derived from SceneIn by the next advance                 */
    int32_t  n_init;                    /* how many times the state was re-derived                                     */
    int32_t  n_sat;                     /* advances whose commanded curvature met +-max_curv                           */
    int32_t  _pad;
} EgoTrackState;                        /* 72 B */

/* ---- lane traffic (build-defined: scripted vehicles that drive a polyline during a rollout) ------
 * pp_set_traffic gives the handle TRACKS - polylines, each a slice of one point array, closed ones with one more segment
 * from the last point back to the first - and ACTORS: each drives one track at its own constant speed and is written, on
 * every staged input set, into one of its scene's OWN obstacle entries.  Actors react to nothing. */
typedef struct TrafficTrack {
    int32_t point_off, n_points;   /* points [point_off, point_off + n_points) of the array given with the tracks; n_points >= 2 */
    int32_t closed;                /* != 0: one more segment, from the last point back to the first                       */
    int32_t _pad;
} TrafficTrack;                                                             /* 16 B */
typedef struct TrafficActor {
    double  s0, speed;             /* metres along the track at set time; m/s (negative: backwards)                        */
    int32_t scene, slot;           /* slot: index inside the scene's OWN obstacle entries (never a peer slot)              */
                                   /* (pp_set_world_traffic, §4j: scene = a WORLD of the fleet, slot = own entry of every member) */
    int32_t track, type;           /* type: ObPoint.type of the slot (nothing on the device reads it)                      */
    float   radius;                /* ObPoint.radius of the slot (metres), finite and >= 0                                 */
    int32_t _pad;
} TrafficActor;                                                             /* 40 B */

/* ---- car-following traffic (build-defined) ----------------------------------------------------
 * pp_set_traffic_follow makes every actor with speed > 0 keep a gap to the vehicle ahead of it on its track - another
 * actor of its scene, or the scene's ego - by the intelligent-driver model; speed is then its DESIRED speed. */
typedef struct TrafficFollow {
    double look;         /* m: how far ahead along its track an actor sees                     */
    double lateral;      /* m: the ego counts as on the track within this distance of a vertex */
    double gap;          /* m: standstill gap                                                  */
    double headway;      /* s: time headway                                                    */
    double max_acc;      /* m/s^2: free-road acceleration                                      */
    double comfort_dec;  /* m/s^2: comfortable deceleration                                    */
    double max_dec;      /* m/s^2: hardest braking (the clamp)                                 */
    double min_net;      /* m: the net gap is never taken smaller than this                    */
} TrafficFollow;                                                            /* 64 B */

/* ---- episodic rollouts (build-defined) ---------------------------------------------------------
 * pp_set_episodes captures every scene's START RECORDS - its SceneIn and its SceneState - and from then on an ego whose flag
 * word meets end_mask, or whose episode reached max_ticks advances, is put back on them inside the advance that ended it:
 * the scene plays episode after episode with no host in the loop, and EpisodeStats counts how each one ended. */
#define DMPP_EGO_RESPAWNED 32   /* EgoTrace.flags only: this record is the start of a new episode          */
#define DMPP_EGO_TIMEOUT   64   /* cause word only: the episode reached EpisodeModel.max_ticks              */
typedef struct EpisodeModel {
    int32_t end_mask;           /* the DMPP_EGO_* flags (bits 1 .. 16) that end an episode                  */
    int32_t max_ticks;          /* > 0: an episode also ends with its max_ticks-th advance; 0: no timeout   */
} EpisodeModel;                                                             /* 8 B */
typedef struct EpisodeStats {
    int32_t n_episodes;         /* episodes ended                                                          */
    int32_t age;                /* advances of the running episode                                         */
    int32_t n_end[6];           /* ended episodes whose cause word had PATH_END, BAD_PATH, LANE_END, OFF_GRID, ROUTE_END, TIMEOUT (one count per bit set) */
    int32_t last_cause, last_age;
    int32_t min_age, max_age;   /* over ended episodes; -1, -1 while none                                  */
    int64_t ticks_total;        /* sum of the ages of ended episodes                                       */
    double  dist, last_dist, dist_total;   /* metres: running episode, last ended one, all ended ones      */
} EpisodeStats;                                                             /* 80 B */

/* ---- episode spawn model (build-defined), on top of pp_set_episodes -------------------------------
 * pp_set_episode_spawn gives every scene a POOL of up to 16 start records (record 0 is the capture of pp_set_episodes), lets
 * contact with an obstacle of the scene's slice end an episode, and checks a start record's pose against the slice and the
 * egos of the scene's world before a restart takes it. */
#define DMPP_EPISODE_MAX_STARTS 16
#define DMPP_EGO_CONTACT 128    /* cause words only (last_cause, EgoTrace.flags of a restart): the ego touched an obstacle */
#define DMPP_EGO_WORLD 256      /* cause words only (EpisodeStats.last_cause, EpisodeRecord.cause): another ego of the scene's world ended on this advance (§4s) */
typedef struct EpisodeSpawn {
    uint64_t seed;              /* of the hashed start choice                                              */
    double   clearance;         /* metres, finite, >= 0: a start record this close to an obstacle or ego is blocked */
    int32_t  n_starts;          /* M: 1 .. DMPP_EPISODE_MAX_STARTS; record 0 is the capture of pp_set_episodes */
    int32_t  order;             /* 0: hashed, 1: round robin                                               */
    int32_t  contact;           /* != 0: contact ends an episode                                           */
    int32_t  check;             /* bit 0: the scene's obstacle slice; bit 1: the egos of its world         */
} EpisodeSpawn;                                                             /* 32 B */
typedef struct EpisodeSpawnStats {
    int32_t n_contact;          /* ended episodes whose cause word had CONTACT                             */
    int32_t n_blocked;          /* restarts for which no start record was clear                            */
    int32_t n_rejected;         /* start records rejected by the clearance check, all restarts             */
    int32_t cur_start;          /* start record of the running episode (0 after the set call)              */
    int32_t n_used[DMPP_EPISODE_MAX_STARTS];   /* restarts onto record k (the first episode is not counted) */
} EpisodeSpawnStats;                                                        /* 80 B */

/* ---- episode traffic reset (build-defined), on top of pp_set_traffic and pp_set_episodes ----------------
 * pp_set_episode_traffic gives every actor of the per-scene traffic one START STATE per start record of its scene (set 0 is
 * captured by the call, like start record 0); when an ego restarts, the actors of its scene go back to the set of the start
 * record the restart took: start record k plus traffic set k is scenario k. */
typedef struct TrafficStart {
    double s, v;                /* arc length (m, wrapped / clamped onto the actor's track); speed (m/s, finite, >= 0) */
} TrafficStart;                                                             /* 16 B */

/* ---- traffic manoeuvres (build-defined), on top of pp_set_traffic ------------------------------------------
 * pp_set_traffic_manoeuvres gives actors of the per-scene traffic a list of triggered moves: a lateral offset from the track, a
 * change onto another track (cut-in, cut-out) and a change of the desired / scripted speed, started by the actor's own clock or
 * by the ego of its scene coming within a distance or a time.  The records of one actor are contiguous, in non-decreasing `actor`
 * order, and run one after the other in list order. */
#define DMPP_MANOEUVRE_MAX 8          /* records per actor */
#define DMPP_TRIG_ADVANCES 0          /* the actor's clock alone */
#define DMPP_TRIG_EGO_DIST 1          /* ego of the actor's scene within `dist` metres of the actor */
#define DMPP_TRIG_EGO_TIME 2          /* ... within `time` seconds at the ego's own speed */
typedef struct TrafficManoeuvre {
    double  dist, time;         /* m, s: finite and >= 0 for the kind that reads them */
    double  lat_end;            /* m, left of the direction of travel positive: offset from the (target) track when the move ends */
    double  speed;              /* m/s: the actor's desired / scripted speed from the trigger on; NaN: keep */
    int32_t actor;
    int32_t trigger;            /* kind | side << 8; side 0 any, 1 ego behind the actor, 2 ego ahead (EGO kinds only) */
    int32_t after;              /* >= 0: advances on the actor's clock before the trigger is looked at at all */
    int32_t track;              /* target track, or -1: stay on the current one */
    int32_t n_steps;            /* 1 .. 4096: advances the lateral move takes */
    int32_t _pad;               /* 0 */
} TrafficManoeuvre;                                                         /* 56 B */
typedef struct TrafficManoeuvreState {
    double  lat, lat0, v0;      /* current offset; offset at the trigger; current desired speed */
    int32_t track, next;        /* current track; index of the actor's next record within its own run */
    int32_t k, clock;           /* steps of the running move done (0: idle); advances since the clock was started */
    int32_t n_done, _pad;       /* moves finished since the set call */
} TrafficManoeuvreState;                                                    /* 48 B */

/* ---- episode log (build-defined), on top of pp_set_episodes ------------------------------------------
 * pp_set_episode_log makes every advance append one record per episode it ended to a ring on the device - in the order of the
 * scene indices, whatever the scheduling - which the host drains whenever it likes (pp_read_episode_log).  No heading: it is
 * the one field the device and the host round differently (§4c), and a record is comparable byte for byte. */
#define DMPP_EPISODE_LOG_MAX (1 << 20)
typedef struct EpisodeRecord {
    int32_t scene, episode;     /* scene index; number of this episode within the scene, 0-based (EpisodeStats.n_episodes - 1 behind the restart) */
    int32_t start, cause;       /* start record the ENDED episode ran on (0 without a spawn model); cause word (DMPP_EGO_* | TIMEOUT | CONTACT | WORLD) */
    int32_t age, seq;           /* advances of the episode; number of the advance that ended it, counted from pp_set_episode_log (first = 0) */
    int64_t tick;               /* pp_tick_id of the last tick of the episode: the tick the ending advance read */
    double  dist;               /* EpisodeStats.last_dist */
    GlobalPoint2D end_pos;      /* loc.globalpoint.x / .y of the SceneIn record the ending advance READ */
    double  end_speed;          /* its loc.velocity, km/h */
    RolloutScore score;         /* the episode's own scorecard: the front half of §4d over the episode's scored ticks; starting values without pp_score_begin */
} EpisodeRecord;                                                            /* 240 B */

/* ---- score trace (build-defined), inside the scorecard's life cycle ---------------------------------------
 * pp_set_score_trace gives every scene a ring of `depth` ScoreTick records on the device: while the scorecard is on, every scored
 * tick stores one compact record, and the ring stops by itself `post` ticks after an incident - contact, a near miss, a hard
 * brake, an ego flag - so that the approach is still there when the host reads it (pp_read_score_trace). */
#define DMPP_SCORE_TRACE_MAX 256          /* records per scene */
/* cause bits (ScoreTraceModel.trigger, ScoreTraceInfo.trigger, ScoreTick.marks >> 8) */
#define DMPP_TRACE_COLLISION 1   /* the tick has a clearance and clearance <= 0            */
#define DMPP_TRACE_NEAR      2   /* the tick has a clearance and clearance <= near         */
#define DMPP_TRACE_FLAG      4   /* (flag word of the tick & flag_mask) != 0               */
#define DMPP_TRACE_BRAKE     8   /* k > 0 and -a >= brake, a as in §4d 3.                  */
/* low bits of ScoreTick.marks */
#define DMPP_TICK_REPLAN 1       /* st.afresh_planning != 0 */
#define DMPP_TICK_OB_FLAG 2      /* po.ob_flag != 0         */
#define DMPP_TICK_DESACC 4       /* po.result.desaccVd != 0 */
#define DMPP_TICK_START 8        /* episodes on and EpisodeStats.age == 0: the tick read a start record */
typedef struct ScoreTraceModel {
    int32_t depth;       /* 1 .. DMPP_SCORE_TRACE_MAX records per scene                         */
    int32_t post;        /* 0 .. depth - 1: ticks recorded after the triggering one             */
    int32_t trigger;     /* DMPP_TRACE_* that freeze a ring; 0: never freezes (a plain ring)    */
    int32_t flag_mask;   /* DMPP_EGO_* bits (1 .. 16) for DMPP_TRACE_FLAG                       */
    double  near;        /* m, finite                                                           */
    double  brake;       /* m/s^2, finite, > 0                                                  */
} ScoreTraceModel;                                                          /* 32 B */
typedef struct ScoreTick {
    int32_t k, flags;        /* index among the scored ticks (RolloutScore.n_ticks before the fold); ego flag word */
    int64_t tick;            /* pp_tick_id of the tick */
    double  x, y, v;         /* si.loc.globalpoint.x / .y, si.loc.velocity (km/h) */
    double  clearance;       /* §4d 1.; +inf when the tick has none */
    int32_t obs, ob_type;    /* j* and snapshot[obs_off + j*].type (DMPP_OB_PEER | scene for a peer); -1, 0 without a clearance */
    int32_t behavior, marks; /* po.dec.behavior as it is; DMPP_TICK_* | cause word of this tick << 8 */
} ScoreTick;                                                                /* 64 B */
typedef struct ScoreTraceInfo {
    int32_t n_written;       /* records written since the start; slot of record i: i % depth */
    int32_t state;           /* 0 armed, 1 counting post, 2 frozen */
    int32_t trigger_k, trigger;   /* k and cause word of the triggering tick; -1, 0 while armed */
    int32_t post_left, n_trigger_ticks;   /* n_trigger_ticks: scored ticks with a cause != 0, frozen or not */
    int32_t _pad[2];
} ScoreTraceInfo;                                                           /* 32 B */

/* ---- conflict score (build-defined), inside the scorecard's life cycle -------------------------------------
 * pp_set_conflict_score keeps the obstacle snapshot of the scored tick before on the device: while the scorecard is on, every
 * scored tick gives every entry of the scene's slice a velocity by differencing, and the smallest time to collision (discs of
 * radius + half the vehicle width, constant relative velocity) and the largest braking demand are folded into one record per scene. */
typedef struct ConflictModel {
    double ttc_warn;     /* s, finite, > 0: a tick with t* <= ttc_warn is a warn tick                  */
    double ttc_crit;     /* s, finite, 0 < ttc_crit <= ttc_warn                                        */
    double v_max;        /* m/s, finite, > 0: a displacement above v_max * dt_score gives no velocity  */
    double min_closing;  /* m/s, finite, >= 0: a closing speed must be > min_closing                   */
} ConflictModel;                                                            /* 32 B */
typedef struct ConflictScore {
    double  min_ttc;                 /* s; +inf while no tick had a conflict */
    double  max_drac;                /* m/s^2: the largest deceleration rate to avoid a crash, vc^2 / (2 gap) */
    double  tit_warn;                /* s^2: sum of (ttc_warn - t*) * dt_score over the warn ticks (time-integrated TTC) */
    GlobalPoint2D last_pos;          /* the ego of the scored tick before */
    int32_t n_ticks;                 /* scored ticks while the step was on */
    int32_t n_conflict_ticks, n_warn_ticks, n_crit_ticks;
    int32_t min_ttc_tick, min_ttc_obs, min_ttc_type;   /* k, j* and snapshot[obs_off + j*].type of min_ttc; -1, -1, 0 without one */
    int32_t first_crit_tick;         /* k of the first tick with t* <= ttc_crit; -1 */
    int32_t max_drac_tick;           /* k of max_drac; -1 */
    int32_t n_no_history_ticks;      /* ticks k > 0 whose ego had no usable tick before: a restart, or a jump above v_max * dt_score */
    int32_t prev_off, prev_n;        /* state of the step: the slice the previous-snapshot buffer holds for this scene */
} ConflictScore;                                                            /* 88 B */

/* ---- perception model (build-defined), belongs to the handle ---------------------------------------------
 * pp_set_perception splits the tick's obstacle snapshot in two: the truth, as before, and what a sensor on the ego would report -
 * range, field of view, occlusion by nearer discs, hashed misses, position noise, a track per pool entry that confirms and coasts.
 * Decision, Planning, the search and its scoring read the perceived snapshot; everything that judges the run keeps the truth.
 * Entry j of the perceived slice is entry j of the truth; an entry the planner must not see is the HIDDEN record
 * { x = y = DMPP_PERCEPT_HIDDEN_XY, type = the truth's, radius = 0 }. */
#define DMPP_PERCEPT_HIDDEN_XY 1.0e12
typedef struct PerceptionModel {
    double   range;          /* m, > 0, may be +inf: in view needs dx dx + dy dy <= range * range                 */
    double   cos_half_fov;   /* -1 .. 1: in view needs (d . heading) >= cos_half_fov * |d|; <= -1: all round       */
    double   sigma0;         /* m, finite, >= 0: position noise at the ego ...                                    */
    double   sigma_gain;     /* finite, >= 0: ... plus this much per metre of distance                            */
    uint32_t p_miss;         /* an in-view, unoccluded entry is missed when the high word of its hash is < p_miss */
    uint32_t seed;
    int32_t  occlusion;      /* 0 | 1: the sight line to the centre must clear the disc of every nearer entry     */
    int32_t  confirm;        /* 0 .. 255: a track is confirmed by more than this many detections in a row         */
    int32_t  coast;          /* 0 .. 255: a confirmed track is reported through this many missing ticks           */
    int32_t  _pad;           /* 0 */
} PerceptionModel;                                                          /* 56 B */
typedef struct PerceptTrack {        /* one per POOL entry */
    ObPoint  last;           /* the last FRESH report; type and radius: the truth's of the last tick (a change restarts the track) */
    uint16_t hits, misses;   /* detections in a row; missing ticks in a row while confirmed */
    uint8_t  confirmed, _pad[3];
} PerceptTrack;                                                             /* 32 B */
typedef struct PerceptionStats {     /* one per scene; both groups of counters sum to n_entries */
    int64_t n_ticks, n_entries;                          /* ticks; entry-ticks */
    int64_t n_out, n_occluded, n_missed, n_detected;     /* by cause, the first that applies */
    int64_t n_fresh, n_coasted, n_hidden;                /* by output */
    double  min_hidden_clearance;    /* m: the closest thing the planner did not see, sqrt(d2) - radius - Vehicle_Width / 2; +inf */
    int64_t min_hidden_tick;         /* its tick id (the first minimum by tick, then by entry); -1 */
    int32_t min_hidden_obs;          /* its entry j; -1 */
    int32_t min_hidden_type;         /* its type; 0 */
} PerceptionStats;                                                          /* 96 B */

/* ---- scenario schedule (build-defined), part of the spawn model in force --------------------------------
 * pp_set_episode_schedule makes the hashed start choice of §4l a WEIGHTED one: the device keeps, per start record, how many
 * episodes ended on it and how many of those failed, and a record's weight peaks where its failure rate meets `target`.
 * Integers only: rates and weights are 16.16 fixed point. */
typedef struct EpisodeSchedule {
    int32_t scope;        /* 0: one row per scene; 1: one row for the handle, pooled over all scenes */
    int32_t fail_mask;    /* cause bits that make an ended episode a FAILURE (bits of 31 | 64 | 128) */
    int32_t pass_mask;    /* ... unless the cause also has one of these (same bit range) */
    int32_t min_samples;  /* >= 1: below this many counted episodes a record's rate is `prior` */
    int32_t window;       /* 0: counts never decay; >= 2: halve a record's two counts whenever n_end >= window */
    int32_t floor_w;      /* 1 .. 65535: every record keeps this weight */
    int32_t gain;         /* 0 .. 65535 */
    int32_t target;       /* 0 .. 65536: the failure rate (x 65536) that gets the largest weight */
    int32_t prior;        /* 0 .. 65536 */
    int32_t _pad;         /* 0 */
} EpisodeSchedule;                                                          /* 40 B */
typedef struct EpisodeScheduleRow {
    int32_t n_end[DMPP_EPISODE_MAX_STARTS];    /* counted episodes that ran on record k  */
    int32_t n_fail[DMPP_EPISODE_MAX_STARTS];   /* ... of which failures                  */
} EpisodeScheduleRow;                                                       /* 128 B */

/* ---- every macro the reference uses but never defines ------------------ */
typedef struct PlannerConfig {
    double ROAD_FARAIM_MAX, ROAD_FARAIM_MIN;      /* Planning.cpp:260,264 */
    double PRE_INTER_FARAIM, INTER_FARAIM;        /* Planning.cpp:275,283 */
    double ROAD_REMAIN_DISTANCE, INTER_REMAIN_DISTANCE; /* Planning.cpp:821,826 */
    double EPSILON, PI;                           /* Planning.cpp:690,728 */
    double Vehicle_Width;                         /* Decision.cpp:370 */
    double NO_OBSTACLE_DIS;                       /* value SearchObstacle leaves in dis_lat/dis_lng when nothing is found */
    /* GlobalToWGS84: local equirectangular frame (projection is unpinned) */
    double wgs_lat0, wgs_lng0, wgs_deg_per_m_lat, wgs_deg_per_m_lng;
    int32_t ID_MORE;                              /* Decision.cpp:581 */
    int32_t decision_stage;                       /* 1: run the CDecision corridor queries + sweep on device */
    int32_t lanechg_stage;                        /* 1: run the lane-change rule tree (Decision.cpp:1017-1772) when the map allows a change */
    /* grid engine (build-defined) */
    int32_t grid_stage;                           /* 1: run G1-G3 every tick */
    int32_t grid_w, grid_h;                       /* cells */
    int32_t max_expansions, bucket_cap, max_path;
    int32_t n_lattice, lookahead_cells;
    int32_t dynamic_obstacles;                    /* 1: obstacle j sits at p0 + v*(dyn_dt*tick) */
    int32_t force_replan;                         /* 1: config "replan every tick" (BASELINE configs[3]) */
    int32_t _cfg_pad;
    double cell;                                  /* metres per cell */
    double inflate;                               /* added to every footprint radius when rasterising */
    double lattice_step, d_safe, w_col, w_curv, w_prog, w_off, dyn_dt;
} PlannerConfig;

#ifdef __cplusplus
}
#endif
#endif /* DMPP_TYPES_H */
