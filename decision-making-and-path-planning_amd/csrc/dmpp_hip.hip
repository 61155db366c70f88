// dmpp_hip.hip — the C-ABI of include/dmpp_planner.h over the HIP kernels (gfx950 only).
//
// One handle = one device and all device buffers.  Streams: the handle's stream (copies, stand-alone operators, the whole
// tick of a small batch), kBuf search streams (stream_m[0] is the handle's stream: the searches of consecutive tick groups
// run side by side, each preceded by its launch order and followed by its own scoring pass; a group is G ticks in one launch), the FRONT stream stream_r (obstacle
// snapshot, Decision, Planning: highest priority, running ahead of the searches), and - once streamed
// ticks are in use (pp_update_async / pp_fetch_async) - one upload and two download streams.  tick_streams describes the
// launch order and the events between the chains; batches below pipeline_min scenes run on the handle's stream with only
// Decision + Planning forked beside the grid engine.  pp_set_* / pp_get_* join the chains first (join_all) and wait on
// the host; the streamed calls never wait on the host (pp_wait_tick waits for one tick's downloads only).
// Nothing here computes planning results on the host; without a GPU pp_create fails.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <string>
#include <cstdlib>
#include <vector>
#include <new>
#include <algorithm>
#include "../../include/dmpp_planner.h"
#include "kernels_r.hpp"
#include "kernels_a.hpp"
#include "kernels_rt.hpp"
#include "kernels_ep.hpp"
#include "kernels_es.hpp"
#include "kernels_ev.hpp"
#include "kernels_ew.hpp"
#include "kernels_g.hpp"
#include "kernels_sc.hpp"
#include "kernels_el.hpp"
#include "kernels_f.hpp"
#include "kernels_t.hpp"
#include "kernels_tm.hpp"
#include "kernels_op.hpp"
#include "kernels_pk.hpp"
#include "kernels_pc.hpp"
#include "search_budget.hpp"
#include "rollout_features.hpp"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess)                                                                \
            return fail(PP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)

// A device allocation that belongs to the handle and goes with it.  reserve() is grow-only and does not keep the contents; the new
// block is allocated before the old one is released, so a failed allocation leaves the old block - and what it holds - in place.
// Converts to T*: a buffer is passed to kernels and copies like the pointer it owns.
template <class T> struct DevBuf {
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~DevBuf() { if (p_) (void)hipFree(p_); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }              // in elements
    int reserve(size_t count)
    {
        if (count == 0) count = 1;
        if (count <= cap_) return PP_OK;
        T* fresh = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&fresh), count * sizeof(T)));
        if (p_) (void)hipFree(p_);
        p_ = fresh; cap_ = count;
        return PP_OK;
    }
private:
    T* p_ = nullptr; size_t cap_ = 0;
};
// ... and of a pinned host array, allocated once and never handed on
template <class T> struct HostPin {
    HostPin() = default;
    HostPin(const HostPin&) = delete; HostPin& operator=(const HostPin&) = delete;
    ~HostPin() { if (p_) (void)hipHostFree(p_); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    int alloc(size_t count) { if (!p_) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T), hipHostMallocDefault)); return PP_OK; }
private:
    T* p_ = nullptr;
};
// ... and of a timing-disabled event that orders one stream behind another, with the fact that it has been recorded: a point that
// was never recorded - or was forgotten - is waited for by nobody.  Created at the first record (or by create(), off the latency path).
struct SyncPoint {
    SyncPoint() = default;
    SyncPoint(const SyncPoint&) = delete; SyncPoint& operator=(const SyncPoint&) = delete;
    ~SyncPoint() { if (ev_) (void)hipEventDestroy(ev_); }
    int create() { if (!ev_) HIP_TRY(hipEventCreateWithFlags(&ev_, hipEventDisableTiming)); return PP_OK; }
    int record(hipStream_t st) { if (int r = create()) return r; HIP_TRY(hipEventRecord(ev_, st)); rec_ = true; return PP_OK; }
    int wait(hipStream_t st) const { if (rec_) HIP_TRY(hipStreamWaitEvent(st, ev_, 0)); return PP_OK; }
    // A stream wait - unless the point has completed: then no barrier packet is needed (uploads and downloads run ticks ahead /
    // behind the chains that wait for them)
    int wait_unless_done(hipStream_t st) const { return done() ? PP_OK : wait(st); }
    int host_wait() const { if (rec_) HIP_TRY(hipEventSynchronize(ev_)); return PP_OK; }
    void forget() { rec_ = false; }
    bool recorded() const { return rec_; }
    // nothing recorded, or what was has completed (hipErrorNotReady is not an error here)
    bool done() const { if (!rec_ || hipEventQuery(ev_) == hipSuccess) return true; (void)hipGetLastError(); return false; }
private:
    hipEvent_t ev_ = nullptr; bool rec_ = false;
};
// (a call that returns the project's error code, inside a function that does)
#define PP_TRY(expr) do { if (int r__ = (expr)) return r__; } while (0)

struct EvPair { hipEvent_t a, b; int k; int w; };      // w: the ticks the launch between a and b stands for (a tick group's)

// Tick groups.  The piped tick (pp_plan_tick) launches the searches and scoring passes of G consecutive ticks together: one
// k_search, one k_search_spill and one k_score over G * n work items (dmpp::TickGroup), G <= kGroupMax.  A search launch ends with
// its slowest scenes; with more work items than workgroup slots the freed slots take the remaining items while those run, so
// that tail is paid once per group instead of once per tick.
constexpr int kGroupMax = dmpp::kGroupMax;
// Work buffers that a group's search and scoring touch exist kBuf times, used round-robin ("parity"): up to kBuf groups' searches
// are in flight at once, each on its own stream, and the scoring of one group never holds up the search of the next.  Each set
// holds up to gcap * caps.max_scenes work items (gcap: the largest G the handle allocates for, see pp_create).
#ifndef DMPP_KBUF
#define DMPP_KBUF 3
#endif
constexpr int kBuf = DMPP_KBUF;
// The obstacle snapshot (with the path cells and the LDS need of its search) exists once per (group position, tick slot): kRing =
// 2 * kBuf group positions of kGroupMax slots.  The front chain of a tick writes the set of its slot in group k while the groups
// k - 1 .. k - 2 kBuf + 1 may still read theirs; it waits for the scoring pass of group k - 2 kBuf, the last reader of that set
// (events, since that pass ran on another stream), so it may run up to 2 kBuf groups ahead of the scoring.
constexpr int kRing = 2 * kBuf;
constexpr int kObs = kRing * kGroupMax;
// Streamed ticks (pp_update_async / pp_fetch_async): the per-tick inputs - SceneIn records, obstacle pool, motion pool - exist
// kIn times.  An update is copied into the set after the current one while the ticks in flight still read theirs (a search
// runs up to kBuf ticks behind the front chain of its tick); a set is written again only after every kernel of the ticks that
// read it (TickRec) has finished.  PlanOut exists kPlan times, so that Planning(t + 1) does not wait for the download of tick t.
constexpr int kIn = 12;
constexpr int kPlan = 12;
// GridOut sets: one per (GridOut group position, tick slot), kGoutRing = 4 kBuf group positions.  Group k and group k + kGoutRing
// use the same search stream (a multiple of kBuf apart), so a set is rewritten behind the scoring pass of its last writer in
// stream order; a download is issued when its scoring pass has finished, up to ~8 groups behind the newest front chain.
constexpr int kGoutRing = 4 * kBuf;
constexpr int kGout = kGoutRing * kGroupMax;
// Work buffers of one search set: at most this many bytes per set for the slots of a tick group (beyond it, fewer slots: G = 1
// at 2048 x 2048, where one scene has 8 MiB of closed-set spill area)
constexpr size_t kGroupBytes = size_t(4) << 30;
constexpr int kDone = 32;          // ticks whose downloads pp_wait_tick can still name

struct InputSet {
    DevBuf<SceneIn> d_in; DevBuf<ObPoint> d_obs; DevBuf<ObMotion> d_mot;
    bool have_motion = false; int n_obs_total = 0;
    SyncPoint up;                                     // behind the kernels that staged the set (upload stream)
    ObMotion* mot() const { return have_motion ? d_mot.get() : nullptr; }      // the velocities, if the set carries any
};
// one tick in flight: which input set it reads, and the events that close its front chain and its last kernel
struct TickRec { long long tick; int in_set; hipEvent_t ev_front, ev_tail; };
// A download asked for by pp_fetch_async.  Its copies are ISSUED only once the kernels they follow have finished (polled by
// every streamed call; forced by pp_wait_tick and by the tick that is about to overwrite the device set): a copy command
// enqueued behind an unfinished dependency sits at the head of its hardware queue / DMA queue as a blocked barrier, and
// streams that share that queue - there are more HIP streams here than hardware queues - stall behind it (measured: the
// front chain's kernels took 2 - 6 times as long with the GridOut copy of each tick enqueued three ticks ahead of its
// scoring pass).
//
// One record is one SIDE of one call: the plan side reads the tick's PlanOut set (or the PackedPlan set of the same index) behind
// the tick's ev_front, the grid side its GridOut set (or the PackedGrid set of its group position) behind ev_tail - ev_front for a
// tick without one.  Requests do not join: a second request for a tick is more records, issued behind the same event on the same
// stream, so every destination a call accepted is filled.
struct FetchCopy { void* dst; const void* src; size_t bytes, stride; };      // per scene: `bytes` out of every `stride` (stride == bytes: one contiguous copy)
struct FetchRec {
    long long tick; int slot, set;      // slot: tick % kDone; set: the PlanOut / GridOut set the copies read
    hipEvent_t dep;                     // the tick's event (prune_inflight keeps the TickRec that owns it until the record is issued)
    size_t n; bool issued;
    int n_copies; FetchCopy copy[2];    // plan side: PlanOut, or result + show, or PackedPlan; grid side: GridOut or PackedGrid
    void add(void* dst, const void* src, size_t bytes, size_t stride) { if (dst) copy[n_copies++] = { dst, src, bytes, stride }; }
};
// What a side owns: its download stream, its records in the order they were asked for, and the points "behind the last download
// that read device set q" (what the tick that rewrites the set waits for) and "behind the downloads of tick done_tick[slot]".
enum { kPlanSide = 0, kGridSide = 1 };
struct FetchSide {
    hipStream_t stream = nullptr;
    SyncPoint fetched[kGout > kPlan ? kGout : kPlan];      // plan side: kPlan sets in use, grid side: kGout
    SyncPoint done[kDone];
    std::vector<FetchRec> queue;
};
// What one fetch call asks for, built by the three typed entry points (pp_fetch_async, pp_fetch_published_async,
// pp_fetch_packed_async): at most two copies on the plan side and one on the grid side (a copy with a null destination is not asked
// for), and whether they read the packed sets.  fetch_async turns it into at most one record per side, appended to that side's queue.
struct FetchAsk { bool packed; FetchCopy plan[2]; FetchCopy grid; };
template <class T> FetchCopy whole_records(T* dst, const T* src) { return { dst, src, sizeof(T), sizeof(T) }; }
template <class T> FetchCopy plan_slice(T* dst, const PlanOut* src, size_t off)      // one member out of every PlanOut record
{ return { dst, reinterpret_cast<const char*>(src) + off, sizeof(T), sizeof(PlanOut) }; }

// closed-loop rollout (first pp_advance_async): the sticky DMPP_EGO_* word of every scene; adv follows the last advance kernel;
// staged_by_advance: the staged input set was produced on the device; set_tick: tick_seq when the resident scenes were last set
// (an advance needs a tick of THESE scenes behind it)
struct RolloutState {
    DevBuf<int32_t> d_flags; SyncPoint adv; bool staged_by_advance = false;
    long long set_tick = 0;
};
// rollout scorecard (first pp_score_begin): the records, one part array of grid counters per search set, ego
// behind the last k_score_ego (upload stream); grp_scored: the open group's tick is scored
struct ScoreState {
    DevBuf<RolloutScore> d_score; DevBuf<dmpp::ScoreGridPart> d_grid[kBuf]; SyncPoint ego;
    bool on = false, grp_scored = false; double dt = 0;
};
// fleet coupling (first pp_set_fleet): world_first, the world of every scene and the pinned slices on the device;
// the pinned slices on the host too (a second pp_set_fleet starts from the scenes' OWN entries); end: the largest end of a
// peer-slot run, base: the used pool size before the fleet grew it, own_end: the largest end of a scene's OWN entries
struct FleetState {
    bool on = false; FleetModel fm = { 0, 0, 0 }; int end = 0, base = 0, own_end = 0, n_worlds = 0;
    DevBuf<int32_t> d_world_first, d_world_of; DevBuf<dmpp::FleetPin> d_pin;
    std::vector<dmpp::FleetPin> pin;
};
// route following (first pp_set_route): the legs of every scene's route and route_first on the device; while on,
// pp_advance_async launches k_advance_route in the place of k_advance_egos
struct RouteState { bool on = false; RouteModel rm = { 0, 0 }; DevBuf<RouteLeg> d_legs; DevBuf<int32_t> d_first; };
// lane traffic (first pp_set_traffic): the actors with their pinned pool entries, the tracks, the compact point
// array and the cumulative-length table; d_s[cur]: the arc length of every actor, SINGLE-COPY like the rollout flags (the advances
// that step it are serial on the upload stream; d_s[1] exists only while following is on, and cur is 0 without it).  end: the
// largest pinned pool entry + 1.
// world (pp_set_world_traffic): one vehicle per WORLD of the fleet in force - d_pin[a].pool is then the SLOT, d_world
// (allocated by that call only) every vehicle's world, scene_of the worlds, and the pins are the fleet's FleetPin table
struct TrafficState {
    bool on = false, world = false; int actors = 0, end = 0, n_tracks = 0;
    DevBuf<int32_t> d_world;
    DevBuf<dmpp::TrafficPin> d_pin; DevBuf<dmpp::TrafficTrackDev> d_tracks; DevBuf<double> d_cum; DevBuf<GlobalPoint2D> d_pts; DevBuf<double> d_s[2];
    std::vector<int32_t> scene_of, track_of;      // host: what a later pp_set_traffic_follow groups the actors by
    int cur = 0;                                  // which arc-length array is current
};
// car-following traffic (pp_set_traffic_follow): the model, and - allocated only while traffic AND following are on -
// TrafficState::d_s[1], the two speed arrays (the step is a Jacobi step: an advance reads pair traffic.cur and writes the
// other, then flips cur; the advances are serial on the upload stream) and the group tables: every actor's scene and group, the
// first member of every group and the actor indices sorted by (scene, track, index)
// episodic rollouts (first pp_set_episodes): the model, every scene's start records - its SceneIn and SceneState as
// captured by the call - and the stats; while on, pp_advance_async launches k_respawn_egos behind its advance kernel.  The stats
// stay readable after episodes went off
struct EpisodeState {
    bool on = false; EpisodeModel em = { 0, 0 };
    DevBuf<SceneIn> d_start_in; DevBuf<SceneState> d_start_state; DevBuf<EpisodeStats> d_stats;
};
// episode spawn model (first pp_set_episode_spawn): the model, the pool of start records - record k of scene s at
// k * stride + s, stride even - and the stats; two sets of all three, so that a refused call leaves the one in force untouched (cur:
// the one in force, or the last that was).  A pool is M * stride * (248 + 3424) B - 0.24 GB at 4096 scenes and M = 16 - and stays allocated
// while the model is off; the second one exists only during a set call (and after a refused one, until the next): the pool it replaces is released once the new one is in force.  While on (only with episodes on), pp_advance_async launches k_respawn_spawn in the place of k_respawn_egos
struct SpawnState {
    bool on = false, ever = false; EpisodeSpawn sp = {}; int stride = 0, cur = 0;      // ever: a set call succeeded on this handle (the stats are readable)
    DevBuf<SceneIn> d_in[2]; DevBuf<SceneState> d_state[2]; DevBuf<EpisodeSpawnStats> d_stats[2];
    // scenario schedule (first pp_set_episode_schedule): feature kSchedule, on only while `on` is.  While on,
    // pp_advance_async launches k_respawn_sched in the place of k_respawn_spawn and, in pooled scope, k_fold_schedule behind it.
    // The rows stay readable after it went off
    bool sched_on = false, sched_ever = false; EpisodeSchedule sched = {};
    DevBuf<EpisodeScheduleRow> d_rows; DevBuf<int32_t> d_fold_word;      // scope 0: a row per scene; scope 1: one row and a word per scene
    // world episodes (first pp_set_episode_worlds): feature kWorldEpisodes, on only while `on` is and never beside
    // the schedule.  While on, pp_advance_async launches k_respawn_world in the place of k_respawn_spawn, one workgroup per world
    // of the fleet in force AT THAT ADVANCE (no fleet: per scene); d_world_end is the kernel's per-scene scratch
    bool worlds_on = false; DevBuf<dmpp::WorldEnd> d_world_end;
};
struct FollowState {
    bool on = false; TrafficFollow tf = {};
    DevBuf<double> d_v[2]; DevBuf<dmpp::TrafficRef> d_ref; DevBuf<int32_t> d_first, d_members;
};
// traffic manoeuvres (pp_set_traffic_manoeuvres): part of the per-scene traffic set - no feature bit, no cause: `on`
// never outlives traffic.on (drop_manoeuvres).  The records and every actor's run of them, every actor's scene and the actor
// indices by (scene, index), and the states twice: while on, TrafficState::d_s[1] exists as well, every advance reads set
// traffic.cur of (s, v, state) and writes the other one (manoeuvre_traffic), with following or without.  All of it is allocated
// by the first successful set call, never before
struct ManoeuvreState {
    bool on = false;
    DevBuf<TrafficManoeuvre> d_recs; DevBuf<int32_t> d_rec_first, d_scene_of, d_scene_first, d_members;
    DevBuf<TrafficManoeuvreState> d_state[2];
};
// episode traffic reset (first pp_set_episode_traffic): every actor's scene, the table of start states - set k of
// actor a at k * actors + a - and the counters; two sets of table and counters, so that a failed call leaves the ones in force
// untouched (cur: the ones in force, or the last that were).  While on (only with per-scene traffic and episodes on),
// pp_advance_async launches k_reset_traffic behind its traffic kernel.  The counters stay readable after the reset went off.
// A second instance is the world traffic reset (first pp_set_episode_world_traffic): the same for the vehicles of
// pp_set_world_traffic, without d_scene; while on (only with world traffic and world episodes on), k_reset_world_traffic
struct TrafficResetState {
    bool on = false, ever = false; int n_sets = 0, actors = 0, cur = 0;      // ever: a set call succeeded on this handle (the counters are readable)
    DevBuf<int32_t> d_scene; DevBuf<TrafficStart> d_starts[2]; DevBuf<int32_t> d_resets[2];
};
// episode log (first pp_set_episode_log): the ring of `cap` records, the count of records appended since the set call,
// every scene's start record and - only on a handle with a scorecard - the scorecard of its running episode; on the host the number
// of the next advance, the ordinal of the oldest unread record and the records lost so far.  While on (only with episodes on),
// pp_advance_async launches k_log_episodes behind its respawn kernel and a scored tick runs k_score_ego<true>.  What was logged stays
// readable after the log went off
struct EpisodeLogState {
    bool on = false, ever = false; int cap = 0, seq = 0; long long read = 0, lost = 0;
    DevBuf<EpisodeRecord> d_ring; DevBuf<long long> d_total; DevBuf<int32_t> d_start_of; DevBuf<RolloutScore> d_score;
};
// score trace (first pp_set_score_trace): the model, caps.max_scenes rings of tm.depth records and one header per
// scene.  It lives inside the scorecard's life cycle - no rollout feature, no set call retires it: while it AND the scorecard are on,
// a scored tick runs k_score_ego<., true>, and whatever restarts the scorecard (reset_scores) restarts the headers.  Rings and
// headers stay readable after it went off
struct ScoreTraceState {
    bool on = false, ever = false; ScoreTraceModel tm = {};
    DevBuf<ScoreTick> d_ring; DevBuf<ScoreTraceInfo> d_info;
};
// conflict score (first pp_set_conflict_score): the model, caps.max_scenes records and two previous-snapshot buffers of
// caps.max_obs_total entries - a scored tick reads d_prev[cur] and writes d_prev[cur ^ 1], then cur flips.  Inside the scorecard's life
// cycle like the trace: while it AND the scorecard are on, a scored tick runs k_score_ego<., ., true>, and reset_scores restarts the
// records.  They stay readable after it went off
struct ConflictState {
    bool on = false, ever = false; int cur = 0; ConflictModel cm = {};
    DevBuf<ConflictScore> d_score; DevBuf<ObPoint> d_prev[2];
};
// perception model (first pp_set_perception): the model, the perceived snapshot ring - the layout of obs_now_mem /
// d_obs_now, slot stride included, so that TickGroup.obs_now + slot * obs_stride works on it -, one track per pool entry and one
// stats record per scene (single copies: only k_perceive of consecutive ticks touches them, and front chains are serial).  While
// on, a tick launches k_perceive in the place of the snapshot kernel and hands the perceived set to Decision, Planning, the search,
// its scoring pass and pp_get_grid.  Belongs to the handle like the ego tracker: no rollout feature, no set call retires it; what
// replaces the resident scenes or moves slices restarts tracks and stats (reset_perception).  They stay readable after it went off
struct PerceptionState {
    bool on = false, ever = false; PerceptionModel pm = {};
    DevBuf<ObPoint> seen_mem[kRing]; ObPoint* d_seen[kObs] = {};
    DevBuf<PerceptTrack> d_track; DevBuf<PerceptionStats> d_stats;
};
// packed streamed fetch (first pp_set_packed_fetch(h, 1)): one PackedPlan set per PlanOut set and one PackedGrid
// set per GridOut group position (an armed handle is a streamed one: groups of 1, tick slot 0 only), each written by its tick's pack
// kernel in stream order behind the kernel that wrote the PlanOut / GridOut set of the same index - so a set is rewritten only
// behind its last download, by the waits that already guard those (FetchSide::fetched).  No rollout feature: no set call
// retires it, and the sets hold caps.max_scenes records, so nothing that changes the resident scenes re-allocates.  plan_tick /
// grid_tick: the last tick whose k_pack_plan / k_pack_grid was launched (what pp_fetch_packed_async may name)
struct PackedState {
    bool on = false; long long plan_tick = 0, grid_tick = 0;
    DevBuf<PackedPlan> d_plan[kPlan]; DevBuf<PackedGrid> d_grid[kGoutRing];
};

}  // namespace

// The handle: the engine (inputs, outputs, grid engine, tick groups, streams and events), the streamed ticks, one block per
// rollout feature, profiling.  Every device buffer is a DevBuf, released with the handle; plain pointers are views.
struct pp_planner {
    PlannerConfig cfg;
    PlannerCaps caps;
    int device = 0;
    int n_scenes = 0;
    hipStream_t stream = nullptr;
    // inputs: the SceneIn records, the obstacle and motion pools and their sizes are those of the current input set, cur_in(); one
    // set (pp_create) until streamed ticks begin
    InputSet in_sets[kIn]; int in_cur = 0, in_staged = -1;
    InputSet& cur_in() { return in_sets[in_cur]; }
    const InputSet& cur_in() const { return in_sets[in_cur]; }
    DevBuf<GlobalPoint3D> d_lane; DevBuf<uint8_t> d_attr; bool have_attr = false; DevBuf<GlobalPoint2D> d_ref;
    int n_lane_pts = 0, n_ref_pts = 0;   // pool sizes of the resident scenes (slice validation)
    int resident_mode = 0;       // 0: scenes with their own slices (pp_set_scenes), 1: egos on the resident map (pp_set_egos)
    DevBuf<int> d_bad;           // k_validate_scenes: scenes with a slice outside its pool
    // map store (pp_set_map): lane / junction tables; the point pools are d_lane / d_attr / d_ref
    DevBuf<int32_t> d_map_first; DevBuf<MapLane> d_map_lanes; DevBuf<uint16_t> d_map_width; DevBuf<MapJunction> d_map_junc;
    DevBuf<int> d_map_bad; int map_roads = 0, map_lanes = 0, map_junctions = 0; bool have_map = false;
    // state / outputs.  The obstacle snapshot, GridOut and the path cells are rings of sets: one allocation per group position
    // (*_mem), the sets of its tick slots at a fixed stride inside it (dmpp::TickGroup; slots beyond gcap: none)
    DevBuf<SceneState> d_state;
    DevBuf<PlanOut> d_plan_ring[kPlan]; int plan_cur = 0;        // PlanOut sets: one (pp_create) until streamed ticks begin
    PlanOut* plan_out() const { return d_plan_ring[plan_cur]; }  // the last tick's
    DevBuf<ObPoint> obs_now_mem[kRing]; ObPoint* d_obs_now[kObs] = {};
    DevBuf<GridOut> gout_mem[kGoutRing]; GridOut* d_gout[kGout] = {}; int gout_set = 0;   // kGout sets (a download of tick t must not hold up the searches after it); gout_set: the last grid tick's
    DevBuf<GlobalPoint2D> d_dec_ref;
    // grid engine.  Consecutive searches overlap their tails: a search and its scoring pass run on stream_m[k % kBuf] for tick
    // group k, and every work buffer they touch exists kBuf times (stream_m[0] is the handle's stream)
    DevBuf<uint8_t> d_grid; DevBuf<uint16_t> d_pinfo[kBuf]; DevBuf<uint32_t> d_closed[kBuf];
    DevBuf<int32_t> d_order[kBuf]; DevBuf<uint32_t> d_gbm[kBuf];
    DevBuf<int32_t> path_mem[kRing]; int32_t* d_path[kObs] = {};       // d_path, d_need: per snapshot set (the scoring pass of a group reads them beside the searches of the next groups)
    int path_set = 0;                                  // the set of the last tick with the grid stage
    DevBuf<int32_t> d_perm[kBuf], d_cost[kBuf];
    DevBuf<uint2> d_ospill[kBuf]; int spill_cap = 0; DevBuf<int32_t> d_retry[kBuf];     // open-list spill areas (bucket_cap0 entries per scene; none when bucket_cap0 <= the LDS list)
    hipStream_t stream_m[kBuf] = {};
    size_t grid_cells = 0;       // per scene, at creation
    int bucket_cap0 = 0, max_path0 = 0;
    // search: k_search_lds<kind> with `lds_budget` data words per view in LDS; scenes that need more go to k_search_gbm
    int search_kind = 0; int search_meta_bytes = 0; int lds_budget = 0, lds_budget_max = 0; bool lds_budget_fixed = false, search_force_gbm = false, budget_from_need = false;
    int lds_budget_launch = 0; bool coresident = true;     // the budget the group's search is launched with (dmpp::coresident_budget of lds_budget; DMPP_CORESIDENT=0: the same)
    int gbm_lds = 0; int search_slots = 512; size_t search_static_lds = 0;   // static LDS of k_search<kind>
    DevBuf<int32_t> d_ovf[kBuf], d_need[kObs]; HostPin<int32_t> h_need;   // h_need: pinned, [kObs], written by k_score (-1: nothing yet)
    int need_seen = 0;
    DevBuf<int> d_gridbad;
    // tick groups: gcap = the most tick slots the work buffers hold (each set: gcap * caps.max_scenes work items); tick_group =
    // env DMPP_TICK_GROUP (0: G derived from n and the search's workgroup slots).  The open group: grp_ticks ticks enqueued on the
    // front chain whose searches wait for grp_G of them (flush_group launches them; so does every entry point that reads
    // results, waits or changes state).
    int gcap = 1, tick_group = 0;
    int grp_ticks = 0, grp_G = 1, grp_n = 0, grp_p_prev = 0; bool grp_piped = false;
    int grp_set[kGroupMax] = {}, grp_gs[kGroupMax] = {}; const SceneIn* grp_in = nullptr;      // (the ticks of a group read one input set: a new one - streamed ticks - comes with G = 1)
    int ring = 0, gring = 0;     // group positions of the last group: snapshot sets (kRing), GridOut sets (kGoutRing)
    int item_off = 0;            // work item of scene 0 of the last grid tick in its group's buffers (pp_get_order / pp_get_search_info)
    int need_set = 0;            // the snapshot set whose d_need / h_need the last group's search and scoring used

    hipStream_t stream_r = nullptr; SyncPoint fork, join;   // the R kernels run beside the grid engine; join: behind the last Planning kernel
    // the scoring pass of a group runs behind its search, beside the front chains and searches of the next groups: the obstacle
    // snapshot, the path cells and GridOut exist per (group position, tick slot); searched[p] = the last search that used the
    // work buffers p, scored[q] = the last scoring pass that read snapshot set q; raster: the snapshot of the group's last tick
    SyncPoint searched[kBuf], scored[kObs], raster;
    SyncPoint io_in;              // pp_tick_io in front of a piped tick: behind k_io_in (handle's stream), waited for by the front chain
    bool front_unjoined = false;  // the last Planning kernel ran beside a piped tick: a one-stream front chain has yet to wait for it
    int parity = 0;              // work buffers of the last group
    bool last_piped = false;     // the last tick ran as three chains on several streams (else it ended on the handle's stream)
    int obs_set = 0;             // obstacle snapshot of the last tick (d_obs_now[obs_set])
    bool front_snapshot = true;  // k_decision writes the snapshot itself where both share a stream (env DMPP_FRONT_SNAPSHOT=0: never)
    int n_cus = 256;
    int pipeline_min = 256;      // batches at least this large run the three chains on three streams (env DMPP_PIPELINE_MIN)
    bool r_on_main = false;      // the last tick ran Decision + Planning on the handle's stream (grid stage off)
    // op scratch (stand-alone operators), in bytes
    DevBuf<char> d_scratch;
    // streamed ticks (the other input and PlanOut sets and the streams are allocated by the first pp_update_async / pp_fetch_async)
    bool streaming = false;
    hipStream_t stream_up = nullptr;                          // upload
    FetchSide dl[2];                                          // downloads: [kPlanSide] of PlanOut / PackedPlan, [kGridSide] of GridOut / PackedGrid
    long long done_tick[kDone];                               // the tick whose downloads dl[.].done[slot] stand behind
    HostPin<int32_t> h_bad;     // pinned, [kDone]: poisoned scenes of the tick (copied down with its PlanOut)
    long long tick_seq = 0;      // ticks enqueued so far on this handle (the id of the last one)
    TickRec rec_last = { -1, 0, nullptr, nullptr };
    std::vector<TickRec> inflight; std::vector<hipEvent_t> sync_events;   // sync_events: a pool of timing-disabled events
    // one block per rollout feature.  Which call switches which feature off, and what holds between the `on` flags, is the table of
    // rollout_features.hpp; a set call writes its own flag, retire() every other one, features_ok() checks the result
    RolloutState rollout;
    ScoreState score;
    FleetState fleet;
    RouteState route;
    TrafficState traffic;
    FollowState follow;
    ManoeuvreState man;                                       // inside the per-scene traffic set (§4v): no feature bit
    EpisodeState episode;
    SpawnState spawn;
    TrafficResetState treset, wreset;                         // per scene (§4m), per world (§4t)
    EpisodeLogState elog;
    ScoreTraceState strace;
    ConflictState conflict;
    PerceptionState percept;
    PackedState packed;
    // a grid that follows the ego: the model travels to both advance kernels as an argument; goal_point 0 = off.
    // It belongs to the handle and holds no per-scene data: nothing that replaces the scenes or the map resets it
    GridFollow grid_follow = { 0, 0 };
    // ego tracking model (first pp_set_ego_tracker): the model and one EgoTrackState per scene.  Like the grid follow it
    // belongs to the handle - no rollout feature, no set call retires it; while on, pp_advance_async launches k_advance_*<true>.
    // A call that replaces the resident scenes zeroes the states (resident_replaced); they stay readable after it went off
    struct TrackerState { bool on = false; EgoTracker tk = {}; DevBuf<EgoTrackState> d_state; } tracker;
    // profiling
    int profile = 0;             // 0 off, 1 every kernel of a tick between HIP events, 2 only the search kernel
    std::vector<EvPair> pending; std::vector<hipEvent_t> free_events;
    float k_ms[PP_K_COUNT] = {0}; int k_launches[PP_K_COUNT] = {0};
};

namespace {

int check_cfg(const PlannerConfig* c)
{
    if (!c) return fail(PP_ERR_ARG, "config is null");
    if (c->grid_stage) {
        if (c->grid_w <= 0 || c->grid_h <= 0 || (c->grid_w % 32) != 0 || (c->grid_h % 32) != 0)
            return fail(PP_ERR_ARG, "grid_w and grid_h must be positive multiples of 32");
        if (c->grid_w > 2048 || c->grid_h > 2048) return fail(PP_ERR_ARG, "grids above 2048x2048 are not supported (one wave scans 64 words of a line)");
        if ((long long)c->grid_w * c->grid_h > (1ll << 24)) return fail(PP_ERR_ARG, "grid larger than 2^24 cells (cell index is 24 bits in an open-set entry)");
        if (c->bucket_cap < 16 || c->max_path < 2) return fail(PP_ERR_ARG, "bucket_cap/max_path too small");
        if (!(c->cell > 0)) return fail(PP_ERR_ARG, "cell size must be positive");
        if (c->n_lattice < 0 || c->n_lattice > DMPP_MAX_LATTICE - 1) return fail(PP_ERR_ARG, "n_lattice out of range");
    }
    return PP_OK;
}

hipEvent_t get_event(pp_planner* h)
{
    if (!h->free_events.empty()) { hipEvent_t e = h->free_events.back(); h->free_events.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// timing-disabled events for cross-stream ordering, pooled
hipEvent_t get_sync_event(pp_planner* h)
{
    if (!h->sync_events.empty()) { hipEvent_t e = h->sync_events.back(); h->sync_events.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
}

void note_current_set(pp_planner* h)          // after a pp_set_* call changed what the current set holds
{
    h->in_staged = -1;                        // an update staged before it is superseded
    h->rollout.staged_by_advance = false; h->rollout.set_tick = h->tick_seq;
}

// Fleet coupling of one input set on the stream that stages it: behind the copies / the advance that produced its
// SceneIn records and obstacle pool, in front of k_resolve_map / k_sanitise_scenes.  Reads and writes only that set.
void couple_fleet(pp_planner* h, hipStream_t st, SceneIn* d_in, ObPoint* d_obs, ObMotion* d_mot)
{
    const int n = h->n_scenes;
    hipLaunchKernelGGL(dmpp::k_couple_fleet, dim3((unsigned)((n + dmpp::kFleetScenes - 1) / dmpp::kFleetScenes)), dim3(dmpp::kBlock), 0, st,
                       n, h->fleet.fm.range * h->fleet.fm.range, h->fleet.fm.radius, h->fleet.fm.max_peers, h->fleet.d_world_first, h->fleet.d_world_of,
                       h->fleet.d_pin, d_in, d_obs, d_mot);
}

// every wave-per-actor traffic kernel runs kTrafficWaves actors per block
unsigned traffic_wave_blocks(int n) { return (unsigned)((n + dmpp::kTrafficWaves - 1) / dmpp::kTrafficWaves); }

// Lane traffic of one input set on the stream that stages it: behind the copies of its obstacle pool, in front of
// k_couple_fleet (the two write disjoint entries: traffic a scene's own, the fleet the peer slots behind them) and of
// k_resolve_map / k_sanitise_scenes.  step: 0 places the actors where they are, EgoModel.dt moves them first.
void move_traffic(pp_planner* h, hipStream_t st, ObPoint* d_obs, ObMotion* d_mot, double step)
{
    const int n = h->traffic.actors;
    if (h->traffic.world) {               // one vehicle per world, written into every member scene (§4j)
        hipLaunchKernelGGL(dmpp::k_move_world_traffic, dim3(traffic_wave_blocks(n)), dim3(dmpp::kBlock), 0, st,
                           n, step, h->traffic.d_pin, h->traffic.d_world, h->fleet.d_world_first, h->fleet.d_pin, h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts,
                           h->traffic.d_s[h->traffic.cur], d_obs, d_mot);
        return;
    }
    hipLaunchKernelGGL(dmpp::k_move_traffic, dim3((unsigned)((n + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, st,
                       n, step, h->traffic.d_pin, h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts, h->traffic.d_s[h->traffic.cur], d_obs, d_mot);
}

// Car-following traffic of the input set an advance stages, in the place of move_traffic: behind k_advance_*, whose
// SceneIn records and flag words it reads.  Reads the current (s, v) pair, writes the other one and - once the launch is accepted -
// makes that the current one.
int follow_traffic(pp_planner* h, hipStream_t st, const SceneIn* d_in, ObPoint* d_obs, ObMotion* d_mot, double dt)
{
    const int n = h->traffic.actors, cur = h->traffic.cur;
    if (h->traffic.world)                 // the leader is the nearest of all the world's egos (§4j)
        hipLaunchKernelGGL(dmpp::k_follow_world_traffic, dim3(traffic_wave_blocks(n)), dim3(dmpp::kBlock), 0, st,
                           n, dt, h->follow.tf, 0.5 * h->cfg.Vehicle_Width, h->traffic.d_pin, h->follow.d_ref, h->follow.d_first, h->follow.d_members,
                           h->fleet.d_world_first, h->fleet.d_pin, h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts, h->traffic.d_s[cur], h->follow.d_v[cur],
                           h->traffic.d_s[cur ^ 1], h->follow.d_v[cur ^ 1], d_in, h->rollout.d_flags, d_obs, d_mot);
    else
    hipLaunchKernelGGL(dmpp::k_follow_traffic, dim3(traffic_wave_blocks(n)), dim3(dmpp::kBlock), 0, st,
                       n, dt, h->follow.tf, 0.5 * h->cfg.Vehicle_Width, h->traffic.d_pin, h->follow.d_ref, h->follow.d_first, h->follow.d_members,
                       h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts, h->traffic.d_s[cur], h->follow.d_v[cur], h->traffic.d_s[cur ^ 1], h->follow.d_v[cur ^ 1],
                       d_in, h->rollout.d_flags, d_obs, d_mot);
    HIP_TRY(hipGetLastError());
    h->traffic.cur = cur ^ 1;
    return PP_OK;
}

// Traffic with manoeuvres of one input set, in the place of move_traffic and follow_traffic while
// pp_set_traffic_manoeuvres is in force.  step = 0 (an update, the set call) places every actor at its current (s, lat) and writes
// no state; an advance reads the current (s, v, state) set, writes the other one and - once the launch is accepted - makes that the
// current one.  d_in: the SceneIn records being staged (read by an advance only).
int manoeuvre_traffic(pp_planner* h, hipStream_t st, const SceneIn* d_in, ObPoint* d_obs, ObMotion* d_mot, double step)
{
    const int n = h->traffic.actors, cur = h->traffic.cur, nxt = step != 0 ? cur ^ 1 : cur;
    const ManoeuvreState& M = h->man;
    if (h->follow.on)
        hipLaunchKernelGGL(dmpp::k_manoeuvre_traffic<true>, dim3(traffic_wave_blocks(n)), dim3(dmpp::kBlock), 0, st,
                           n, step, h->follow.tf, 0.5 * h->cfg.Vehicle_Width, h->traffic.d_pin, M.d_scene_of, M.d_scene_first, M.d_members, M.d_recs, M.d_rec_first,
                           h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts, h->traffic.d_s[cur], h->follow.d_v[cur], M.d_state[cur],
                           h->traffic.d_s[nxt], h->follow.d_v[nxt], M.d_state[nxt], d_in, h->rollout.d_flags, d_obs, d_mot);
    else
        hipLaunchKernelGGL(dmpp::k_manoeuvre_traffic<false>, dim3(traffic_wave_blocks(n)), dim3(dmpp::kBlock), 0, st,
                           n, step, h->follow.tf, 0.5 * h->cfg.Vehicle_Width, h->traffic.d_pin, M.d_scene_of, M.d_scene_first, M.d_members, M.d_recs, M.d_rec_first,
                           h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts, h->traffic.d_s[cur], nullptr, M.d_state[cur],
                           h->traffic.d_s[nxt], nullptr, M.d_state[nxt], d_in, h->rollout.d_flags, d_obs, d_mot);
    HIP_TRY(hipGetLastError());
    h->traffic.cur = nxt;
    return PP_OK;
}
// Whatever ends or replaces the per-scene traffic frees the manoeuvres with it ("Feature life cycle")
void drop_manoeuvres(pp_planner* h)
{
    if (!h->man.on) return;
    h->man = ManoeuvreState();
}

// Episode traffic reset of the input set an advance stages: behind the episode step, whose EpisodeStats.age and
// EpisodeSpawnStats.cur_start it reads, and behind the traffic kernel of the advance, whose arrays - the current ones: with
// following the pair follow_traffic has just flipped to - and pool entries it overwrites for the actors of restarted scenes.
// world: the same for the vehicles of a world that has just restarted, written into every member scene.
void reset_traffic(pp_planner* h, bool world, hipStream_t st, ObPoint* d_obs, ObMotion* d_mot)
{
    const TrafficResetState& R = world ? h->wreset : h->treset;
    const int n = R.actors, cur = h->traffic.cur;
    const EpisodeSpawnStats* sstats = R.n_sets > 1 ? h->spawn.d_stats[h->spawn.cur].get() : nullptr;
    double* v_arr = h->follow.on ? h->follow.d_v[cur].get() : nullptr;
    if (world)
        hipLaunchKernelGGL(dmpp::k_reset_world_traffic, dim3(traffic_wave_blocks(n)), dim3(dmpp::kBlock), 0, st,
                           n, R.n_sets, h->traffic.d_pin, h->traffic.d_world, h->fleet.d_world_first, h->fleet.d_pin, h->episode.d_stats, sstats, R.d_starts[R.cur],
                           h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts, h->traffic.d_s[cur], v_arr, R.d_resets[R.cur], d_obs, d_mot);
    else
        hipLaunchKernelGGL(dmpp::k_reset_traffic, dim3((unsigned)((n + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, st,
                           n, R.n_sets, h->traffic.d_pin, R.d_scene, h->episode.d_stats, sstats, R.d_starts[R.cur],
                           h->traffic.d_tracks, h->traffic.d_cum, h->traffic.d_pts, h->traffic.d_s[cur], v_arr, R.d_resets[R.cur], d_obs, d_mot);
    if (!world && h->man.on)              // ... and their manoeuvres back to the state of the set call (§4v)
        hipLaunchKernelGGL(dmpp::k_reset_manoeuvres, dim3((unsigned)((n + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, st,
                           n, h->traffic.d_pin, h->man.d_scene_of, h->episode.d_stats, h->man.d_state[cur]);
}

// The advance kernel of the input set an advance stages, in the place of the copy of its SceneIn records: reads the
// records `prev` of the current set, the last tick's PlanOut and SceneState, writes d_in.  Routed egos cross junctions (§4f:
// k_advance_route; the scenes without a route advance as in k_advance_egos).
template <bool kTrack>
void launch_advance(pp_planner* h, hipStream_t st, const EgoModel& ego, const SceneIn* prev, SceneIn* d_in, EgoTrace* trace, typename dmpp::AdvTrackArg<kTrack>::type trk)
{
    const int n = h->n_scenes;
    const dim3 grid((unsigned)((n + dmpp::kAdvScenes - 1) / dmpp::kAdvScenes)), block(dmpp::kBlock);
    if (h->route.on)
        hipLaunchKernelGGL(dmpp::k_advance_route<kTrack>, grid, block, 0, st,
                           h->cfg, ego, h->route.rm, h->grid_follow, n, prev, d_in, h->plan_out(), h->d_state, h->d_lane, h->d_ref, h->map_junctions, h->d_map_junc,
                           h->route.d_legs, h->route.d_first, h->rollout.d_flags, trace, trk);
    else
        hipLaunchKernelGGL(dmpp::k_advance_egos<kTrack>, grid, block, 0, st,
                           h->cfg, ego, h->grid_follow, n, h->resident_mode == 1 ? 1 : 0, prev, d_in, h->plan_out(), h->d_state, h->d_lane, h->rollout.d_flags, trace, trk);
}
// with an ego tracker the pose step is the bicycle model of DESIGN.md §4q: the <true> form of the same kernel; the episode stats
// it reads are those the episode step of the advance BEFORE left (same stream)
void advance_egos(pp_planner* h, hipStream_t st, const EgoModel& ego, const SceneIn* prev, SceneIn* d_in, EgoTrace* trace)
{
    if (h->tracker.on) launch_advance<true>(h, st, ego, prev, d_in, trace, { h->tracker.tk, h->tracker.d_state, h->episode.on ? h->episode.d_stats.get() : nullptr });
    else launch_advance<false>(h, st, ego, prev, d_in, trace, 0);
}

// The episode step of the input set an advance stages, directly behind the advance kernel: ended egos restart from their start
// records, so the traffic, the peers and the views behind it see the restarted ego.  P: the set the advance read.
void step_episodes(pp_planner* h, hipStream_t st, const InputSet& P, SceneIn* d_in, EgoTrace* trace)
{
    const int n = h->n_scenes, cur = h->spawn.cur;
    const dim3 grid((unsigned)((n + dmpp::kEpScenes - 1) / dmpp::kEpScenes)), block(dmpp::kBlock);
    const double hw = 0.5 * h->cfg.Vehicle_Width;
    const int32_t* world_first = h->fleet.on ? h->fleet.d_world_first.get() : nullptr;
    const int32_t* world_of = h->fleet.on ? h->fleet.d_world_of.get() : nullptr;
    RolloutScore* score = h->score.on ? h->score.d_score.get() : nullptr;
    if (!h->spawn.on)
        hipLaunchKernelGGL(dmpp::k_respawn_egos, grid, block, 0, st,
                           h->episode.em, n, P.d_in, d_in, h->d_state, h->episode.d_start_in, h->episode.d_start_state, h->rollout.d_flags, h->episode.d_stats, trace, score);
    else if (h->spawn.worlds_on)      // world episodes (§4s): one workgroup per world of the fleet in force, or per scene without one
        hipLaunchKernelGGL(dmpp::k_respawn_world, dim3((unsigned)(h->fleet.on ? h->fleet.n_worlds : n)), block, 0, st,
                           h->episode.em, h->spawn.sp, hw, h->spawn.stride, P.d_in, P.d_obs, P.n_obs_total, d_in, h->d_state, h->spawn.d_in[cur], h->spawn.d_state[cur],
                           world_first, h->fleet.on ? h->fleet.d_pin.get() : nullptr, h->rollout.d_flags, h->episode.d_stats, h->spawn.d_stats[cur], trace, score,
                           h->spawn.d_world_end);
    else if (!h->spawn.sched_on)      // the spawn model of §4l: contact ends an episode, the start record is drawn from a pool and checked for clearance
        hipLaunchKernelGGL(dmpp::k_respawn_spawn, grid, block, 0, st,
                           h->episode.em, h->spawn.sp, hw, n, h->spawn.stride, P.d_in, P.d_obs, P.n_obs_total, d_in, h->d_state, h->spawn.d_in[cur], h->spawn.d_state[cur],
                           world_first, world_of, h->rollout.d_flags, h->episode.d_stats, h->spawn.d_stats[cur], trace, score);
    else {                            // ... and a schedule over its start records (§4p): the first choice is drawn by weights
        EpisodeScheduleRow* rows = h->spawn.d_rows;
        hipLaunchKernelGGL(dmpp::k_respawn_sched, grid, block, 0, st,
                           h->episode.em, h->spawn.sp, h->spawn.sched, hw, n, h->spawn.stride, P.d_in, P.d_obs, P.n_obs_total, d_in, h->d_state, h->spawn.d_in[cur],
                           h->spawn.d_state[cur], world_first, world_of, h->rollout.d_flags, h->episode.d_stats, h->spawn.d_stats[cur], trace, score, rows, h->spawn.d_fold_word);
        if (h->spawn.sched.scope == 1)      // the endings of this advance into the handle's one row, behind every draw
            hipLaunchKernelGGL(dmpp::k_fold_schedule, dim3(1), dim3(dmpp::kFoldBlock), 0, st, n, h->spawn.sched.window, h->episode.d_stats, h->spawn.d_fold_word, rows);
    }
    if (h->elog.on) {      // one record per episode the kernel above ended, in the order of the scenes; the kernels behind it do not read it
        hipLaunchKernelGGL(dmpp::k_log_episodes, dim3(1), dim3(dmpp::kLogBlock), 0, st,
                           n, h->elog.cap, h->elog.seq, h->tick_seq, P.d_in, h->episode.d_stats, h->spawn.on ? h->spawn.d_stats[cur].get() : nullptr,
                           h->elog.d_ring, h->elog.d_total, h->elog.d_start_of, h->elog.d_score);
        h->elog.seq++;
    }
}

// The buffers of following for the actors pp_set_traffic has just uploaded, and v = speed.  The caller has joined the chains and
// the handle's stream is idle; traffic.cur stays.  On failure the caller switches traffic off.
int build_follow(pp_planner* h)
{
    const size_t n = (size_t)h->traffic.actors;
    std::vector<int32_t> members(n);
    for (size_t a = 0; a < n; a++) members[a] = (int32_t)a;
    const std::vector<int32_t>& sc = h->traffic.scene_of; const std::vector<int32_t>& tr = h->traffic.track_of;
    std::sort(members.begin(), members.end(), [&](int32_t p, int32_t q) {
        if (sc[(size_t)p] != sc[(size_t)q]) return sc[(size_t)p] < sc[(size_t)q];
        if (tr[(size_t)p] != tr[(size_t)q]) return tr[(size_t)p] < tr[(size_t)q];
        return p < q;
    });
    std::vector<dmpp::TrafficRef> ref(n); std::vector<int32_t> first;
    for (size_t m = 0; m < n; m++) {
        const size_t a = (size_t)members[m];
        if (m == 0 || sc[a] != sc[(size_t)members[m - 1]] || tr[a] != tr[(size_t)members[m - 1]]) first.push_back((int32_t)m);
        ref[a] = { sc[a], (int32_t)first.size() - 1 };
    }
    first.push_back((int32_t)n);
    int rc;
    if ((rc = h->traffic.d_s[1].reserve(n)) || (rc = h->follow.d_v[0].reserve(n)) || (rc = h->follow.d_v[1].reserve(n)) || (rc = h->follow.d_ref.reserve(n)) ||
        (rc = h->follow.d_first.reserve(first.size())) || (rc = h->follow.d_members.reserve(n))) return rc;
    HIP_TRY(hipMemcpyAsync(h->follow.d_ref, ref.data(), n * sizeof(dmpp::TrafficRef), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->follow.d_first, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->follow.d_members, members.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    // v = speed: the first 8 bytes of every 24-byte pin
    static_assert(offsetof(dmpp::TrafficPin, speed) == 0, "the speeds are copied out of the pins at their stride");
    HIP_TRY(hipMemcpy2DAsync(h->follow.d_v[h->traffic.cur], sizeof(double), h->traffic.d_pin, sizeof(dmpp::TrafficPin), sizeof(double), n, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));            // (the host arrays above go out of scope)
    return PP_OK;
}

// Issues the copies of the pending downloads whose kernels have finished.  force_tick: that tick's copies are issued whatever
// the state of its kernels (behind a stream wait); force_plan_set / force_grid_set: likewise the copies that read that
// PlanOut / GridOut set (the next tick is about to overwrite it).
int pump_fetches(pp_planner* h, long long force_tick = -1, int force_plan_set = -1, int force_grid_set = -1)
{
    const int force_set[2] = { force_plan_set, force_grid_set };
    // The grid side first: a tick's scoring pass ends ticks behind its Planning kernel, so the grid record that has become ready
    // belongs to an OLDER tick than the plan record that has - the tick pp_wait_tick is called for next.  Its copy goes out ahead of
    // the newer tick's (measured: plan side first, the streamed leg of bench.py lost 7 - 9 %: profiles/r35_streamed_io.txt)
    for (int side : { kGridSide, kPlanSide }) {
        FetchSide& S = h->dl[side];
        for (FetchRec& f : S.queue) {
            if (f.issued) continue;
            const bool ready = hipEventQuery(f.dep) == hipSuccess;
            if (!ready && f.tick != force_tick && f.set != force_set[side]) continue;
            (void)hipGetLastError();
            if (!ready) HIP_TRY(hipStreamWaitEvent(S.stream, f.dep, 0));
            for (int i = 0; i < f.n_copies; i++) {
                const FetchCopy& c = f.copy[i];
                if (c.stride == c.bytes) HIP_TRY(hipMemcpyAsync(c.dst, c.src, f.n * c.bytes, hipMemcpyDefault, S.stream));
                else HIP_TRY(hipMemcpy2DAsync(c.dst, c.bytes, c.src, c.stride, c.bytes, f.n, hipMemcpyDefault, S.stream));
            }
            PP_TRY(S.fetched[f.set].record(S.stream));
            PP_TRY(S.done[f.slot].record(S.stream));
            f.issued = true;
        }
        size_t k = 0;                         // issued records leave from the front (prune_inflight looks at the first one left)
        while (k < S.queue.size() && S.queue[k].issued) k++;
        S.queue.erase(S.queue.begin(), S.queue.begin() + (long)k);
    }
    (void)hipGetLastError();                  // hipErrorNotReady is not an error here
    return PP_OK;
}

// ticks whose kernels have all finished leave the in-flight list (oldest first; the list stays short: a tick's front chain
// waits for the scoring pass 2 * kBuf ticks before it).  Their events go back to the pool: rec_last may still name the
// events of the last tick, which are recorded again by the next tick at the earliest - and then rec_last names that one.
int prune_inflight(pp_planner* h)
{
    long long named = h->tick_seq + 1;        // the oldest tick whose events a download not issued yet still names: the older of the two front records
    for (const FetchSide& S : h->dl) if (!S.queue.empty()) named = std::min(named, S.queue.front().tick);
    size_t k = 0;
    while (k < h->inflight.size()) {
        const TickRec& r = h->inflight[k];
        if (r.tick >= named) break;
        if (hipEventQuery(r.ev_front) != hipSuccess || (r.ev_tail && hipEventQuery(r.ev_tail) != hipSuccess)) break;
        h->sync_events.push_back(r.ev_front); if (r.ev_tail) h->sync_events.push_back(r.ev_tail);
        k++;
    }
    (void)hipGetLastError();                  // hipErrorNotReady is not an error here
    h->inflight.erase(h->inflight.begin(), h->inflight.begin() + (long)k);
    if (h->inflight.size() > 256) {           // a caller that never lets the device catch up: wait for the oldest
        HIP_TRY(hipEventSynchronize(h->inflight.front().ev_front));
        if (h->inflight.front().ev_tail) HIP_TRY(hipEventSynchronize(h->inflight.front().ev_tail));
    }
    return PP_OK;
}

constexpr int kScoreWideMaxScenes = 128;     // up to here k_score runs 16 waves per scene (one scene per CU at most)

// Tick slots the work buffers of a handle are allocated for: kGroupMax when its batches can run piped (max_scenes >= pipeline_min)
// and the knob does not pin G to 1, fewer when a set of kGroupMax * max_scenes work items would exceed kGroupBytes.
int group_cap(int max_scenes, int pipeline_min, int forced, size_t item_bytes)
{
    if (max_scenes < pipeline_min || forced == 1) return 1;
    int g = kGroupMax;
    while (g > 1 && (size_t)g * (size_t)max_scenes * item_bytes > kGroupBytes) g--;
    return g;
}
// Ticks per group for a batch of n scenes: the knob if set (DMPP_TICK_GROUP), else the smallest G whose G * n work items are at
// least twice the search's workgroup slots (the slots freed by the short scenes then have work while the long ones run);
// at most the slots the handle's buffers hold (gcap <= kGroupMax).
// The workgroup that should fit beside the searching workgroups of a CU (dmpp::coresident_budget): the larger of k_planning's and
// k_score<4>'s, both all dynamic LDS.  (k_decision's 16 granules start in what a retiring search frees.)
constexpr size_t kBesideSearchLds = std::max(sizeof(dmpp::PlanShared), sizeof(dmpp::ScoreShared<4>));
static_assert(dmpp::lds_granules(sizeof(dmpp::SearchLds<dmpp::closed_log_of<0>()>) + 64 + 4096 + 8 * 1600) * 6 + dmpp::lds_granules(kBesideSearchLds) <= (int)(dmpp::kLdsPerCu / dmpp::kLdsGranule),
              "512 x 512, 1,600 words per view: six searching workgroups of 19 granules and a k_planning or k_score workgroup on one CU");

int group_size(int n, int search_slots, int gcap, int forced)
{
    int g = forced;
    if (g <= 0) {
        g = 1;
        while (g < kGroupMax && (long long)g * n < 2ll * search_slots) g++;
    }
    return std::max(1, std::min({ g, gcap, kGroupMax }));
}

int flush_group(pp_planner* h);

// Everything the ticks enqueued so far started - on any of the four streams - is ordered before whatever the handle's
// stream does next: scored[q] closes the raster -> search -> score chain of the last group that used snapshot set q, join
// the Decision -> Planning chain (stream order covers the earlier ticks).  An open tick group is launched first.  No host wait.
int join_all(pp_planner* h)
{
    { int r = flush_group(h); if (r) return r; }
    for (const SyncPoint& sp : h->scored) PP_TRY(sp.wait(h->stream));
    PP_TRY(h->join.wait(h->stream));
    PP_TRY(h->score.ego.wait(h->stream));
    return PP_OK;
}

// Rollout features (rollout_features.hpp; DESIGN.md §7 "Feature life cycle").  The features that are on, as the table's bits ...
unsigned feature_mask(const pp_planner* h)
{
    using namespace dmpp;
    return (h->fleet.on ? kFleet : 0u) | (h->route.on ? kRoute : 0u) | (h->traffic.on ? (h->traffic.world ? kWorldTraffic : kTraffic) : 0u) | (h->follow.on ? kFollow : 0u) |
           (h->episode.on ? kEpisodes : 0u) | (h->spawn.on ? kSpawn : 0u) | (h->treset.on ? kTrafficReset : 0u) | (h->elog.on ? kEpisodeLog : 0u) |
           (h->spawn.sched_on ? kSchedule : 0u) | (h->spawn.worlds_on ? kWorldEpisodes : 0u) | (h->wreset.on ? kWorldReset : 0u);
}
// ... and the bits as flags: the ONLY code that writes the flag of a feature other than the caller's own
void switch_features(pp_planner* h, unsigned m, bool on)
{
    using namespace dmpp;
    if (m & kFleet) h->fleet.on = on;
    if (m & kRoute) h->route.on = on;
    if (m & (h->traffic.world ? kWorldTraffic : kTraffic)) { h->traffic.on = on; if (!on) drop_manoeuvres(h); }      // (§4v: the manoeuvres live inside the traffic set)
    if (m & kFollow) h->follow.on = on;
    if (m & kEpisodes) h->episode.on = on;
    if (m & kSpawn) h->spawn.on = on;
    if (m & kTrafficReset) h->treset.on = on;
    if (m & kEpisodeLog) h->elog.on = on;
    if (m & kSchedule) h->spawn.sched_on = on;
    if (m & kWorldEpisodes) h->spawn.worlds_on = on;
    if (m & kWorldReset) h->wreset.on = on;
    static_assert(dmpp::kFeatureCount == 12, "a new feature bit needs its flag here and in feature_mask");
}
void retire(pp_planner* h, int cause) { switch_features(h, dmpp::retires(cause), false); }
// the common success exit of every set call
int features_ok(const pp_planner* h, const char* fn)
{
    if (dmpp::consistent(feature_mask(h), h->have_map, h->resident_mode)) return PP_OK;
    return fail(PP_ERR_STATE, std::string("internal: rollout feature flags inconsistent after ") + fn);
}
// A set call refuses while an update is staged: the staged set was built from what the call would replace.
int refuse_if_staged(const pp_planner* h, const std::string& fn, const char* what)
{
    if (h->in_staged < 0) return PP_OK;
    return fail(PP_ERR_STATE, fn + ": an update is staged for the next tick (set " + what + " before staging, or after the tick)");
}
// In front of what a set call changes: every tick and every advance enqueued so far is ordered before the handle's stream (nothing
// is staged, or the call supersedes it: every advance was adopted by a tick, and join_all is behind those); host_wait: and has finished.
int quiesce(pp_planner* h, bool host_wait)
{
    HIP_TRY(hipSetDevice(h->device));
    PP_TRY(join_all(h));
    PP_TRY(h->rollout.adv.wait(h->stream));
    if (host_wait) HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

// HIP events around a launch.  A launch for a tick group counts as its w ticks: w launches, its time spread over them (the
// averages of pp_get_kernel_ms stay per tick).
struct Timed {
    pp_planner* h; int k; hipStream_t st; int w; hipEvent_t a = nullptr, b = nullptr; bool on = false;
    Timed(pp_planner* h_, int k_, hipStream_t st_ = nullptr, int w_ = 1) : h(h_), k(k_), st(st_ ? st_ : h_->stream), w(w_) {
        on = h->profile == 1 || (h->profile == 2 && k == PP_K_SEARCH);
        if (on) { a = get_event(h); b = get_event(h); if (a) (void)hipEventRecord(a, st); }
    }
    ~Timed() {
        if (on && a && b) { (void)hipEventRecord(b, st); h->pending.push_back({a, b, k, w}); }
    }
};

int drain_events(pp_planner* h)
{
    { int r = flush_group(h); if (r) return r; }         // (a profile switch applies from the next group on)
    if (h->pending.empty()) return PP_OK;
    { int r = join_all(h); if (r) return r; }
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (auto& p : h->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { h->k_ms[p.k] += ms; h->k_launches[p.k] += p.w; }
        h->free_events.push_back(p.a); h->free_events.push_back(p.b);
    }
    h->pending.clear();
    return PP_OK;
}

int setup_grid_launch(pp_planner* h)
{
    const PlannerConfig& c = h->cfg;
    if (!c.grid_stage) return PP_OK;
    const size_t N = (size_t)c.grid_w * c.grid_h;
    // search: per-line metas of both sparse views + the budgeted data words in dynamic LDS (kernels_s.hpp)
    const int lw = (int)std::max((size_t)c.grid_w / 32, (size_t)c.grid_h / 32);
    h->search_kind = lw <= 16 ? 0 : (lw <= 32 ? 1 : 2);
    const size_t per_line = h->search_kind == 0 ? 4 : (h->search_kind == 1 ? 8 : 10);
    h->search_meta_bytes = (int)((((size_t)c.grid_w + c.grid_h) * per_line + 15) & ~(size_t)15);
    h->search_static_lds = h->search_kind == 2 ? sizeof(dmpp::SearchLds<dmpp::closed_log_of<2>()>) : sizeof(dmpp::SearchLds<dmpp::closed_log_of<0>()>);
    static_assert(dmpp::closed_log_of<0>() == dmpp::closed_log_of<1>(), "one static LDS size for the kinds 0 and 1");
    const size_t static_lds = h->search_static_lds + 64;
    size_t lds_max = 64u * 1024u;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device) == hipSuccess && (size_t)v > lds_max) lds_max = (size_t)v;
    }
    lds_max = std::min(lds_max, dmpp::kLdsPerCu);
    h->gbm_lds = (int)(((size_t)c.grid_w + c.grid_h) * 8);
    if (std::max((size_t)h->search_meta_bytes + 2 * 64 * 4, (size_t)h->gbm_lds) + static_lds > lds_max)
        return fail(PP_ERR_CAPACITY, "grid too large for the search kernel's LDS tables");
    {
        const size_t room = (lds_max - static_lds - (size_t)h->search_meta_bytes) / 8;        // data words per view that fit at all
        const size_t dense = N / 32;                                                            // ... that a view can ever need
        h->lds_budget_max = (int)std::min(room, dense);
        const void* fns[3] = { reinterpret_cast<const void*>(&dmpp::k_search<0, dmpp::kSearchSetupWaves>), reinterpret_cast<const void*>(&dmpp::k_search<1, dmpp::kSearchSetupWaves>),
                               reinterpret_cast<const void*>(&dmpp::k_search<2, dmpp::kSearchSetupWaves>) };
        const void* fnw[3] = { reinterpret_cast<const void*>(&dmpp::k_search<0, dmpp::kSearchSetupWavesWide>), reinterpret_cast<const void*>(&dmpp::k_search<1, dmpp::kSearchSetupWavesWide>),
                               reinterpret_cast<const void*>(&dmpp::k_search<2, dmpp::kSearchSetupWavesWide>) };
        const void* fnr[3] = { reinterpret_cast<const void*>(&dmpp::k_search_spill<0>), reinterpret_cast<const void*>(&dmpp::k_search_spill<1>),
                               reinterpret_cast<const void*>(&dmpp::k_search_spill<2>) };
        const void* fne[3] = { reinterpret_cast<const void*>(&dmpp::k_export_grid<0>), reinterpret_cast<const void*>(&dmpp::k_export_grid<1>),
                               reinterpret_cast<const void*>(&dmpp::k_export_grid<2>) };
        const int dyn_max = std::max(h->search_meta_bytes + 8 * h->lds_budget_max, h->gbm_lds);
        if (dyn_max + (int)static_lds > 48 * 1024) {
            if (hipFuncSetAttribute(fns[h->search_kind], hipFuncAttributeMaxDynamicSharedMemorySize, dyn_max) != hipSuccess ||
                hipFuncSetAttribute(fnw[h->search_kind], hipFuncAttributeMaxDynamicSharedMemorySize, dyn_max) != hipSuccess ||
                hipFuncSetAttribute(fnr[h->search_kind], hipFuncAttributeMaxDynamicSharedMemorySize, dyn_max) != hipSuccess ||
                hipFuncSetAttribute(fne[h->search_kind], hipFuncAttributeMaxDynamicSharedMemorySize, dyn_max) != hipSuccess) {
                (void)hipGetLastError();
                h->lds_budget_max = (int)std::min((size_t)h->lds_budget_max, (48u * 1024u - static_lds - (size_t)h->search_meta_bytes) / 8);
            }
        }
    }
    if (const char* e = std::getenv("DMPP_SEARCH_GBM")) h->search_force_gbm = std::atoi(e) != 0;          // test / measurement knob: the dense form in HBM for every scene
    if (const char* e = std::getenv("DMPP_LDS_BUDGET")) {                                                // ... a fixed budget (words per view)
        h->lds_budget = std::max(1, std::min(std::atoi(e), h->lds_budget_max)); h->lds_budget_fixed = true;
    } else h->lds_budget = 0;                                                                            // chosen at the first tick (obstacle density), then adaptive
    h->lds_budget_launch = h->lds_budget;
    if (const char* e = std::getenv("DMPP_CORESIDENT")) h->coresident = std::atoi(e) != 0;               // A/B knob: 0 = launch with the policy's budget as it is
    const size_t items = (size_t)h->gcap * h->caps.max_scenes;          // work items of a search set
    auto zeroed_once = [&](DevBuf<int32_t>& b, size_t count) {           // allocated - and cleared - by the first configuration with the grid stage
        if (b) return (int)PP_OK;
        PP_TRY(b.reserve(count));
        HIP_TRY(hipMemsetAsync(b, 0, count * sizeof(int32_t), h->stream));
        return (int)PP_OK;
    };
    for (int q = 0; q < kBuf; q++) {
        PP_TRY(zeroed_once(h->d_ovf[q], items)); PP_TRY(zeroed_once(h->d_perm[q], items)); PP_TRY(zeroed_once(h->d_cost[q], items));
        if (!h->d_retry[q]) PP_TRY(h->d_retry[q].reserve(items));
    }
    for (int q = 0; q < kObs; q++) PP_TRY(zeroed_once(h->d_need[q], 2));   // [0] LDS need of the search, [1] its retry count
    { int r = h->h_need.alloc(kObs); if (r) return r; }
    for (int q = 0; q < kObs; q++) h->h_need[q] = -1;       // (a new configuration: what earlier searches needed says nothing; no search is in flight here)
    h->budget_from_need = false;
    if (!h->d_gridbad) { int r = h->d_gridbad.reserve((size_t)2); if (r) return r; }
    if (sizeof(dmpp::ScoreShared<16>) > 48u * 1024u)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dmpp::k_score<16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(dmpp::ScoreShared<16>));
    // the dense form of the two views (row- then column-major), only written by the scenes that do not fit the LDS budget
    for (int q = 0; q < kBuf; q++) { int r = h->d_gbm[q].reserve(items * 2 * (h->grid_cells / 32)); if (r) return r; }
    return PP_OK;
}

}  // namespace

extern "C" {

const char* pp_last_error(void) { return g_err.c_str(); }

int pp_create(const PlannerConfig* cfg, int device, const PlannerCaps* caps, pp_handle* out)
{
    if (!out || !caps) return fail(PP_ERR_ARG, "null argument");
    *out = nullptr;
    int r = check_cfg(cfg); if (r) return r;
    if (caps->max_scenes <= 0) return fail(PP_ERR_ARG, "max_scenes must be positive");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(PP_ERR_HIP, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(PP_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    pp_planner* h = new (std::nothrow) pp_planner();
    if (!h) return fail(PP_ERR_HIP, "out of host memory");
    h->cfg = *cfg; h->caps = *caps; h->device = device;
    if (const char* e = std::getenv("DMPP_PIPELINE_MIN")) h->pipeline_min = std::atoi(e);      // tuning knob: 0 = always, large = never
    if (const char* e = std::getenv("DMPP_TICK_GROUP")) h->tick_group = std::atoi(e);          // A/B knob: ticks per search launch (1: one, as before groups)
    if (const char* e = std::getenv("DMPP_FRONT_SNAPSHOT")) h->front_snapshot = std::atoi(e) != 0;   // A/B knob: 0 = the snapshot stays a launch of its own (k_effective_obstacles) on every path
    if (cfg->grid_stage) {
        // tick slots the work buffers hold: kGroupMax for a handle that runs piped ticks, as long as a set stays within kGroupBytes
        const size_t cells = (size_t)cfg->grid_w * cfg->grid_h;
        const size_t item_bytes = cells * sizeof(uint16_t) + 3 * (cells / 32) * sizeof(uint32_t) + (size_t)std::max(caps->order_cap, 0) * sizeof(int32_t) +
                                  (cfg->bucket_cap > DMPP_OPEN_CAP ? (size_t)cfg->bucket_cap * sizeof(uint2) : 0) + 4 * sizeof(int32_t);
        h->gcap = group_cap(caps->max_scenes, h->pipeline_min, h->tick_group, item_bytes);
    }
    auto bail = [&](int code) { pp_destroy(h); return code; };
    // Queue priorities.  The FRONT chain (obstacle snapshot, Decision, Planning) is a short serial chain that every tick's
    // search waits for: it gets the highest dispatch priority (and its waves raise their issue priority, s_setprio).  The
    // searches are the bulk of the work and overlap each other, each followed on its stream by its scoring pass: normal priority.
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    const int prio_normal = (prio_least + prio_greatest) / 2;
    if (hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, prio_normal) != hipSuccess) return bail(fail(PP_ERR_HIP, "hipStreamCreate failed"));
    h->stream_m[0] = h->stream;
    for (int q = 1; q < kBuf; q++)
        if (hipStreamCreateWithPriority(&h->stream_m[q], hipStreamNonBlocking, prio_normal) != hipSuccess) return bail(fail(PP_ERR_HIP, "hipStreamCreate failed"));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->n_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithPriority(&h->stream_r, hipStreamNonBlocking, prio_greatest) != hipSuccess) return bail(fail(PP_ERR_HIP, "hipStreamCreate failed"));
    // the one-stream tick records these two every tick: created here, off the latency path (the piped, streamed and rollout paths
    // create theirs at the first record)
    if ((r = h->fork.create()) || (r = h->join.create())) return bail(r);
    const size_t ns = (size_t)caps->max_scenes;
    if ((r = h->in_sets[0].d_in.reserve(ns))) return bail(r);
    if ((r = h->d_lane.reserve((size_t)caps->max_lane_pts_total))) return bail(r);
    if ((r = h->d_attr.reserve((size_t)caps->max_lane_pts_total + 1))) return bail(r);
    if ((r = h->d_ref.reserve((size_t)caps->max_ref_pts_total))) return bail(r);
    if ((r = h->in_sets[0].d_obs.reserve((size_t)caps->max_obs_total))) return bail(r);
    if ((r = h->in_sets[0].d_mot.reserve((size_t)caps->max_obs_total))) return bail(r);
    if (hipMemsetAsync(h->in_sets[0].d_mot, 0, (size_t)(caps->max_obs_total > 0 ? caps->max_obs_total : 1) * sizeof(ObMotion), h->stream) != hipSuccess)
        return bail(fail(PP_ERR_HIP, "memset failed"));     // velocities nobody uploaded are zero, never uninitialised
    if ((r = h->d_bad.reserve((size_t)1))) return bail(r);
    // the sets of the tick slots of a group position lie at a fixed stride in one allocation (dmpp::TickGroup); slots beyond gcap: none
    const size_t obs_stride = (size_t)std::max(caps->max_obs_total, 1);
    for (int q = 0; q < kObs; q += kGroupMax) {
        if ((r = h->obs_now_mem[q / kGroupMax].reserve(h->gcap * obs_stride))) return bail(r);
        for (int i = 0; i < h->gcap; i++) h->d_obs_now[q + i] = h->obs_now_mem[q / kGroupMax] + i * obs_stride;
    }
    if ((r = h->d_state.reserve(ns))) return bail(r);
    if ((r = h->d_plan_ring[0].reserve(ns))) return bail(r);
    if (hipMemsetAsync(h->d_plan_ring[0], 0, ns * sizeof(PlanOut), h->stream) != hipSuccess) return bail(fail(PP_ERR_HIP, "memset failed"));
    for (int q = 0; q < kDone; q++) h->done_tick[q] = -1;
    for (int q = 0; q < kGout; q += kGroupMax) {
        if ((r = h->gout_mem[q / kGroupMax].reserve(h->gcap * ns))) return bail(r);
        for (int i = 0; i < h->gcap; i++) h->d_gout[q + i] = h->gout_mem[q / kGroupMax] + i * ns;
    }
    if ((r = h->d_dec_ref.reserve(ns * DMPP_MAX_REFPATH))) return bail(r);
    for (int q = 0; q < kGout; q += kGroupMax)
        if (hipMemsetAsync(h->d_gout[q], 0, h->gcap * ns * sizeof(GridOut), h->stream) != hipSuccess) return bail(fail(PP_ERR_HIP, "memset failed"));
    if (cfg->grid_stage) {
        h->grid_cells = (size_t)cfg->grid_w * cfg->grid_h;
        h->bucket_cap0 = cfg->bucket_cap; h->max_path0 = cfg->max_path;
        if ((r = h->d_grid.reserve(h->grid_cells))) return bail(r);             // one scene as bytes, filled on demand (pp_get_grid)
        const size_t items = (size_t)h->gcap * ns;          // work items of a search set
        for (int q = 0; q < kBuf; q++) {
            if ((r = h->d_pinfo[q].reserve(items * h->grid_cells))) return bail(r);
            if ((r = h->d_closed[q].reserve(items * (h->grid_cells / 32)))) return bail(r);
        }
        for (int q = 0; q < kObs; q += kGroupMax) {
            if ((r = h->path_mem[q / kGroupMax].reserve(h->gcap * ns * (size_t)cfg->max_path))) return bail(r);
            for (int i = 0; i < h->gcap; i++) h->d_path[q + i] = h->path_mem[q / kGroupMax] + i * ns * (size_t)cfg->max_path;
        }
        for (int q = 0; q < kBuf; q++) if (caps->order_cap > 0 && (r = h->d_order[q].reserve(items * (size_t)caps->order_cap))) return bail(r);
        if (cfg->bucket_cap > DMPP_OPEN_CAP) {
            h->spill_cap = cfg->bucket_cap;
            for (int q = 0; q < kBuf; q++) if ((r = h->d_ospill[q].reserve(items * (size_t)h->spill_cap))) return bail(r);
        }
        if ((r = setup_grid_launch(h))) return bail(r);
    }
    if ((r = h->d_scratch.reserve(4u << 20))) return bail(r);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return bail(fail(PP_ERR_HIP, "sync failed"));
    *out = h;
    return PP_OK;
}

int pp_destroy(pp_handle h)
{
    if (!h) return PP_OK;
    (void)hipSetDevice(h->device);
    (void)flush_group(h);                     // (the open group's work buffers go with the handle: its launches are enqueued and waited for)
    // every stream is idle before the first buffer is released (the buffers go last, with the handle)
    std::vector<hipStream_t> streams = { h->stream, h->stream_r, h->stream_up, h->dl[kPlanSide].stream, h->dl[kGridSide].stream };
    for (int q = 1; q < kBuf; q++) streams.push_back(h->stream_m[q]);      // (stream_m[0] is the handle's stream)
    for (hipStream_t st : streams) if (st) (void)hipStreamSynchronize(st);
    for (auto& p : h->pending) { h->free_events.push_back(p.a); h->free_events.push_back(p.b); }
    for (auto& r : h->inflight) { h->sync_events.push_back(r.ev_front); h->sync_events.push_back(r.ev_tail); }
    for (auto* evs : { &h->free_events, &h->sync_events }) for (hipEvent_t e : *evs) if (e) (void)hipEventDestroy(e);      // the two pools; every SyncPoint goes with the handle
    for (hipStream_t st : streams) if (st) (void)hipStreamDestroy(st);
    delete h;
    return PP_OK;
}

int pp_set_config(pp_handle h, const PlannerConfig* cfg)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    PP_TRY(check_cfg(cfg));
    if (h->grid_follow.goal_point > 0 && 2LL * h->grid_follow.margin_cells >= (long long)std::min(cfg->grid_w, cfg->grid_h))
        return fail(PP_ERR_ARG, "pp_set_config: the margin of the grid-follow model no longer fits the grid (2 * margin_cells < min(grid_w, grid_h)): switch following off first");
    if (cfg->grid_stage) {
        if (!h->d_grid) return fail(PP_ERR_STATE, "handle was created without the grid stage");
        if ((size_t)cfg->grid_w * cfg->grid_h > h->grid_cells || cfg->max_path > h->max_path0)
            return fail(PP_ERR_CAPACITY, "grid size / max_path may not grow after pp_create");
        if (cfg->bucket_cap > DMPP_OPEN_CAP && cfg->bucket_cap > h->spill_cap)
            return fail(PP_ERR_CAPACITY, "bucket_cap may not grow after pp_create beyond the larger of its value then and DMPP_OPEN_CAP (it sizes the open list's spill area)");
    }
    PP_TRY(quiesce(h, true));      // a configuration change may move the next tick's kernels to other streams (grid stage on / off): finish what is queued
    h->cfg = *cfg;
    PP_TRY(setup_grid_launch(h));
    return features_ok(h, "pp_set_config");
}

// New resident scenes: the rollout flags of the old ones go (behind the last advance; the caller's host wait follows).
static int reset_ego_flags(pp_handle h)
{
    if (!h->rollout.d_flags) return PP_OK;
    PP_TRY(h->rollout.adv.wait(h->stream));
    HIP_TRY(hipMemsetAsync(h->rollout.d_flags, 0, (size_t)h->caps.max_scenes * sizeof(int32_t), h->stream));
    return PP_OK;
}

// The headers of the score trace at their starting values (§4o), on the handle's stream: behind join_all, as reset_scores.
static int reset_score_trace(pp_handle h)
{
    if (!h->strace.d_info) return PP_OK;
    const int ns = h->caps.max_scenes;
    hipLaunchKernelGGL(dmpp::k_score_trace_reset, dim3((unsigned)((ns + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream, ns, h->strace.d_info);
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

// The records of the conflict score at their starting values (§4u 0.), on the handle's stream: behind join_all, as reset_scores.
static int reset_conflict(pp_handle h)
{
    if (!h->conflict.d_score) return PP_OK;
    const int ns = h->caps.max_scenes;
    hipLaunchKernelGGL(dmpp::k_conflict_reset, dim3((unsigned)((ns + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream, ns, h->conflict.d_score);
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

// Tracks and stats of the perception model at their starting values (§4w 4., 5.), on the handle's stream: behind join_all - every
// k_perceive enqueued so far has finished before it, and the next front chain starts behind the caller's host wait.
static int reset_perception(pp_handle h)
{
    if (!h->percept.d_stats) return PP_OK;
    const int ns = h->caps.max_scenes, nt = std::max(h->caps.max_obs_total, 1), nn = std::max(ns, nt);
    hipLaunchKernelGGL(dmpp::k_percept_reset, dim3((unsigned)((nn + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream,
                       ns, h->percept.d_stats.get(), nt, h->percept.d_track.get());
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

// The scorecard's starting values, on the handle's stream behind join_all (every scoring kernel enqueued so far has finished
// before it); the caller's host wait follows.
static int reset_scores(pp_handle h)
{
    if (!h->score.d_score) return PP_OK;
    const int ns = h->caps.max_scenes;
    hipLaunchKernelGGL(dmpp::k_score_reset, dim3((unsigned)((ns + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream, ns, h->score.d_score);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < kBuf; q++) HIP_TRY(hipMemsetAsync(h->score.d_grid[q], 0, (size_t)ns * sizeof(dmpp::ScoreGridPart), h->stream));
    if (h->elog.d_score) {                              // the scorecards of the running episodes restart with the totals (§4n 3.)
        hipLaunchKernelGGL(dmpp::k_score_reset, dim3((unsigned)((ns + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream, ns, h->elog.d_score);
        HIP_TRY(hipGetLastError());
    }
    if (h->strace.on) PP_TRY(reset_score_trace(h));       // the score trace restarts where the scorecard does (§4o)
    if (h->conflict.on) PP_TRY(reset_conflict(h));        // ... and the conflict score (§4u)
    return PP_OK;
}

// Slices of the resident SceneIn records against the resident pools (k_validate_scenes); syncs the handle's stream.
static int validate_resident(pp_handle h, int n_scenes, const char* who)
{
    int bad = 0;
    if (n_scenes > 0) {
        HIP_TRY(hipMemsetAsync(h->d_bad, 0, sizeof(int), h->stream));
        hipLaunchKernelGGL(dmpp::k_validate_scenes, dim3((unsigned)((n_scenes + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream,
                           n_scenes, h->cur_in().d_in, h->cur_in().n_obs_total, h->n_lane_pts, h->n_ref_pts, h->d_bad);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&bad, h->d_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (bad) {
        h->n_scenes = 0;                                // nothing a tick could follow out of its pool stays resident
        return fail(PP_ERR_ARG, std::string(who) + ": " + std::to_string(bad) + " scene(s) with an obstacle / lane / refpath slice outside its pool");
    }
    return PP_OK;
}

// The obstacle and motion pools of new resident scenes, into the current input set (handle's stream).
static int upload_pools(pp_handle h, const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total)
{
    InputSet& I = h->cur_in();
    if (n_obs_total && obs_pool) HIP_TRY(hipMemcpyAsync(I.d_obs, obs_pool, (size_t)n_obs_total * sizeof(ObPoint), hipMemcpyDefault, h->stream));
    I.have_motion = false;
    if (n_obs_total && mot_pool) {
        HIP_TRY(hipMemcpyAsync(I.d_mot, mot_pool, (size_t)n_obs_total * sizeof(ObMotion), hipMemcpyDefault, h->stream));
        I.have_motion = true;
    }
    return PP_OK;
}

// The end of every call that replaces the resident scenes (h->n_scenes and the pool sizes are the new ones): the features that
// hold per-scene data of the old scenes go off, the rollout flags and the scorecard start again, the slices are checked
// last (which syncs: the caller may reuse its buffers).  map_bad: scenes that k_resolve_map could not place (pp_set_egos).
static int resident_replaced(pp_handle h, int mode, const char* who, int map_bad = 0)
{
    h->resident_mode = mode; retire(h, dmpp::kResidentReplaced); note_current_set(h);
    PP_TRY(reset_ego_flags(h));
    if (h->tracker.d_state)                              // every tracked pose is re-derived from the new records (§4q 1.)
        HIP_TRY(hipMemsetAsync(h->tracker.d_state, 0, (size_t)h->caps.max_scenes * sizeof(EgoTrackState), h->stream));
    if (h->score.on) PP_TRY(reset_scores(h));
    PP_TRY(reset_perception(h));      // no track outlives the scenes it followed (§4w)
    if (map_bad) { h->n_scenes = 0; return fail(PP_ERR_ARG, std::string(who) + ": " + std::to_string(map_bad) + " scene(s) name a road or lane outside the map"); }
    PP_TRY(validate_resident(h, h->n_scenes, who));
    return features_ok(h, who);
}

int pp_set_scenes(pp_handle h, int n_scenes, const SceneIn* in, const GlobalPoint3D* lane_pool, const uint8_t* lane_attr_pool,
                  int n_lane_pts, const GlobalPoint2D* ref_pool, int n_ref_pts, const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total)
{
    if (!h || !in) return fail(PP_ERR_ARG, "null argument");
    if (n_scenes < 0 || n_scenes > h->caps.max_scenes) return fail(PP_ERR_CAPACITY, "n_scenes exceeds caps.max_scenes");
    if (n_lane_pts > h->caps.max_lane_pts_total || n_ref_pts > h->caps.max_ref_pts_total || n_obs_total > h->caps.max_obs_total)
        return fail(PP_ERR_CAPACITY, "pool larger than the capacity given to pp_create");
    if (n_lane_pts < 0 || n_ref_pts < 0 || n_obs_total < 0) return fail(PP_ERR_ARG, "negative size");
    PP_TRY(quiesce(h, false));
    HIP_TRY(hipMemcpyAsync(h->cur_in().d_in, in, (size_t)n_scenes * sizeof(SceneIn), hipMemcpyDefault, h->stream));
    if (n_lane_pts && lane_pool) HIP_TRY(hipMemcpyAsync(h->d_lane, lane_pool, (size_t)n_lane_pts * sizeof(GlobalPoint3D), hipMemcpyDefault, h->stream));
    h->have_attr = false;
    if (n_lane_pts && lane_attr_pool) {
        HIP_TRY(hipMemcpyAsync(h->d_attr, lane_attr_pool, (size_t)n_lane_pts, hipMemcpyDefault, h->stream));
        h->have_attr = true;
    }
    if (n_ref_pts && ref_pool) HIP_TRY(hipMemcpyAsync(h->d_ref, ref_pool, (size_t)n_ref_pts * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    PP_TRY(upload_pools(h, obs_pool, mot_pool, n_obs_total));
    h->n_scenes = n_scenes; h->cur_in().n_obs_total = n_obs_total; h->n_lane_pts = n_lane_pts; h->n_ref_pts = n_ref_pts;
    return resident_replaced(h, 0, "pp_set_scenes");
}

static int fetch(pp_handle h, void* dst, const void* src, size_t bytes);

int pp_set_map(pp_handle h, const MapDesc* m)
{
    if (!h || !m) return fail(PP_ERR_ARG, "null argument");
    if (m->n_roads < 0 || m->n_lanes < 0 || m->n_points < 0 || m->n_junctions < 0 || m->n_jpoints < 0) return fail(PP_ERR_ARG, "negative size");
    if (m->n_points > h->caps.max_lane_pts_total || m->n_jpoints > h->caps.max_ref_pts_total)
        return fail(PP_ERR_CAPACITY, "map larger than caps.max_lane_pts_total / max_ref_pts_total");
    if ((m->n_lanes && (!m->road_first_lane || !m->lanes)) || (m->n_points && (!m->points || !m->lanechg_attribute || !m->lane_width_cm)) ||
        (m->n_junctions && !m->junctions) || (m->n_jpoints && !m->jpoints)) return fail(PP_ERR_ARG, "null map array");
    // the tables are host arrays: every slice is checked here, so that no scene can index outside the pools
    if (m->n_roads && (m->road_first_lane[0] != 0 || m->road_first_lane[m->n_roads] != m->n_lanes)) return fail(PP_ERR_ARG, "road_first_lane must run from 0 to n_lanes");
    for (int r = 0; r < m->n_roads; r++) if (m->road_first_lane[r + 1] < m->road_first_lane[r]) return fail(PP_ERR_ARG, "road_first_lane must not decrease");
    for (int l = 0; l < m->n_lanes; l++) {
        const MapLane& L = m->lanes[l];
        if (L.point_off < 0 || L.n_points < 0 || (long long)L.point_off + L.n_points > m->n_points) return fail(PP_ERR_ARG, "lane slice outside the point pool");
    }
    for (int j = 0; j < m->n_junctions; j++) {
        const MapJunction& J = m->junctions[j];
        if (J.point_off < 0 || J.n_points < 0 || (long long)J.point_off + J.n_points > m->n_jpoints) return fail(PP_ERR_ARG, "junction slice outside the junction point pool");
    }
    PP_TRY(quiesce(h, true));
    h->have_map = false;                                 // (until the new tables have landed)
    retire(h, dmpp::kMapReplaced);                       // (the routes named roads of the old map)
    int r;
    if ((r = h->d_map_first.reserve((size_t)m->n_roads + 1)) || (r = h->d_map_lanes.reserve((size_t)m->n_lanes)) || (r = h->d_map_junc.reserve((size_t)m->n_junctions)) ||
        (r = h->d_map_width.reserve((size_t)h->caps.max_lane_pts_total + 1)) || (r = h->d_map_bad.reserve((size_t)1))) return r;
    if (m->n_roads) HIP_TRY(hipMemcpyAsync(h->d_map_first, m->road_first_lane, ((size_t)m->n_roads + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(hipMemsetAsync(h->d_map_first, 0, sizeof(int32_t), h->stream));
    if (m->n_lanes) HIP_TRY(hipMemcpyAsync(h->d_map_lanes, m->lanes, (size_t)m->n_lanes * sizeof(MapLane), hipMemcpyHostToDevice, h->stream));
    if (m->n_junctions) HIP_TRY(hipMemcpyAsync(h->d_map_junc, m->junctions, (size_t)m->n_junctions * sizeof(MapJunction), hipMemcpyHostToDevice, h->stream));
    if (m->n_points) {
        HIP_TRY(hipMemcpyAsync(h->d_lane, m->points, (size_t)m->n_points * sizeof(GlobalPoint3D), hipMemcpyDefault, h->stream));
        HIP_TRY(hipMemcpyAsync(h->d_attr, m->lanechg_attribute, (size_t)m->n_points, hipMemcpyDefault, h->stream));
        HIP_TRY(hipMemcpyAsync(h->d_map_width, m->lane_width_cm, (size_t)m->n_points * sizeof(uint16_t), hipMemcpyDefault, h->stream));
    }
    if (m->n_jpoints) HIP_TRY(hipMemcpyAsync(h->d_ref, m->jpoints, (size_t)m->n_jpoints * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->map_roads = m->n_roads; h->map_lanes = m->n_lanes; h->map_junctions = m->n_junctions;
    h->n_lane_pts = m->n_points; h->n_ref_pts = m->n_jpoints;
    h->have_map = true; h->have_attr = true;
    return features_ok(h, "pp_set_map");
}

int pp_set_egos(pp_handle h, int n_scenes, const SceneIn* in, const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total)
{
    if (!h || !in) return fail(PP_ERR_ARG, "null argument");
    if (!h->have_map) return fail(PP_ERR_STATE, "pp_set_egos needs a resident map (pp_set_map)");
    if (n_scenes < 0 || n_scenes > h->caps.max_scenes) return fail(PP_ERR_CAPACITY, "n_scenes exceeds caps.max_scenes");
    if (n_obs_total < 0 || n_obs_total > h->caps.max_obs_total) return fail(PP_ERR_CAPACITY, "obstacle pool larger than caps.max_obs_total");
    PP_TRY(quiesce(h, false));
    HIP_TRY(hipMemcpyAsync(h->cur_in().d_in, in, (size_t)n_scenes * sizeof(SceneIn), hipMemcpyDefault, h->stream));
    PP_TRY(upload_pools(h, obs_pool, mot_pool, n_obs_total));
    HIP_TRY(hipMemsetAsync(h->d_map_bad, 0, sizeof(int), h->stream));
    if (n_scenes)
        hipLaunchKernelGGL(dmpp::k_resolve_map, dim3((unsigned)((n_scenes + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream,
                           n_scenes, h->cur_in().d_in, h->map_roads, h->d_map_first, h->d_map_lanes, h->d_attr, h->d_map_width,
                           h->map_junctions, h->d_map_junc, h->d_map_bad);
    HIP_TRY(hipGetLastError());
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, h->d_map_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->n_scenes = n_scenes; h->cur_in().n_obs_total = n_obs_total;
    return resident_replaced(h, 1, "pp_set_egos", bad);         // (the obstacle slices are still the caller's: checked there)
}

int pp_get_scene_in(pp_handle h, SceneIn* out, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    if (h->in_staged >= 0 && h->rollout.staged_by_advance) {      // the records the advance produced for the next tick exist only on the device
        HIP_TRY(hipSetDevice(h->device));
        PP_TRY(h->in_sets[h->in_staged].up.wait(h->stream));
        return fetch(h, out, h->in_sets[h->in_staged].d_in, (size_t)n * sizeof(SceneIn));
    }
    return fetch(h, out, h->cur_in().d_in, (size_t)n * sizeof(SceneIn));
}

int pp_set_n_scenes(pp_handle h, int n_scenes, int n_lane_pts, int n_ref_pts, int n_obs_total, int have_motion, int have_lane_attr)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (n_scenes < 0 || n_scenes > h->caps.max_scenes) return fail(PP_ERR_CAPACITY, "n_scenes exceeds caps.max_scenes");
    if (n_lane_pts < 0 || n_ref_pts < 0 || n_obs_total < 0) return fail(PP_ERR_ARG, "negative size");
    if (n_lane_pts > h->caps.max_lane_pts_total || n_ref_pts > h->caps.max_ref_pts_total || n_obs_total > h->caps.max_obs_total)
        return fail(PP_ERR_CAPACITY, "pool larger than the capacity given to pp_create");
    PP_TRY(quiesce(h, false));
    h->n_scenes = n_scenes; h->cur_in().n_obs_total = n_obs_total; h->n_lane_pts = n_lane_pts; h->n_ref_pts = n_ref_pts;
    h->cur_in().have_motion = have_motion != 0; h->have_attr = have_lane_attr != 0;
    return resident_replaced(h, 0, "pp_set_n_scenes");
}

int pp_set_state(pp_handle h, const SceneState* state, int n)
{
    if (!h || !state) return fail(PP_ERR_ARG, "null argument");
    if (n < 0 || n > h->caps.max_scenes) return fail(PP_ERR_CAPACITY, "n exceeds caps.max_scenes");
    HIP_TRY(hipSetDevice(h->device));
    { int r = join_all(h); if (r) return r; }
    if (h->episode.on) PP_TRY(h->rollout.adv.wait(h->stream));      // (episodes: a staged advance may still be restoring start states on the upload stream)
    HIP_TRY(hipMemcpyAsync(h->d_state, state, (size_t)n * sizeof(SceneState), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

}  // extern "C"

namespace {

// One tick = two chains.  FRONT (stream_r, highest priority): obstacle snapshot, Decision, Planning - short kernels, serial
// from tick to tick through SceneState.  SEARCH (stream_m[k % kBuf] for tick group k): launch order, k_search,
// k_search_spill, k_score - the long one, for the G ticks of the group at once (flush_group).  Consecutive searches overlap: a
// search ends with a handful of long scenes and would leave most of the chip idle, so the searches of kBuf consecutive groups
// run side by side on their own streams, each followed on its stream by its own scoring pass.
//   search(k) waits for the snapshot of the front chain of its last tick [raster] - the front chain is one stream, so that covers
//             all G - and follows score(k - kBuf) on its stream;
//   front(t)  waits for score(k - 2 kBuf), the last reader of the snapshot set it overwrites - so it may run up to 2 kBuf
//             groups ahead of the scoring.
// What a search and its scoring pass write exists kBuf times (closed sets, orders, ...: work buffers of G * n items), what
// the scoring pass reads beside later searches once per (group position, slot) - kObs times (snapshot, path cells, LDS need),
// GridOut kGout times.  The search of a tick is a function of its inputs and its snapshot alone, so which ticks share a launch
// changes no result.
// Small batches and ticks without the grid stage stay on one stream, one tick per group (a cross-stream hand-over costs tens
// of microseconds; only Decision + Planning run beside the grid engine there); so do streamed ticks (pp_update_async /
// pp_fetch_async: every tick is fetched, and its downloads wait for its own scoring pass).
// (a tick without the grid stage leaves the search buffers alone: pp_get_grid_out / pp_get_path keep returning the last search)
struct TickStreams { hipStream_t front, dp, search, score; };          // dp: Decision + Planning
// whether the next tick of the resident scenes runs piped (pp_plan_tick; pp_tick_io orders the front chain of such a tick behind k_io_in)
bool tick_piped(const pp_planner* h) { return h->cfg.grid_stage && h->n_scenes >= h->pipeline_min; }
TickStreams tick_streams(const pp_planner* h, bool piped, bool grid_stage, int parity)
{
    hipStream_t search = piped ? h->stream_m[parity] : h->stream;
    return { piped ? h->stream_r : h->stream, grid_stage ? h->stream_r : h->stream, search, search };
}

// Launches the searches and scoring passes of the open tick group (nothing when no group is open): one k_order (when the work
// items outnumber the search's workgroup slots), one k_search, one k_search_spill and one k_score over the G * n work items.
int flush_group(pp_planner* h)
{
    const int G = h->grp_ticks;
    if (G == 0) return PP_OK;
    h->grp_ticks = 0;
    const PlannerConfig& c = h->cfg;
    const int n = h->grp_n, items = G * n, p = h->parity;
    const bool piped = h->grp_piped;
    const TickStreams T = tick_streams(h, piped, true, p);
    hipStream_t sm = T.search, ss = T.score;
    // Work buffers p were last used by group k - kBuf (its tick slot 0 used snapshot set set_b)
    const int set0 = h->grp_set[0], set_b = ((h->ring + kBuf) % kRing) * kGroupMax;
    PP_TRY(h->scored[set_b].wait(sm));
    if (!piped)                                                        // one search at a time (also after a switch of mode)
        for (int q = 0; q < kBuf; q++) if (q != p) PP_TRY(h->searched[q].wait(sm));
    if (T.front != sm) PP_TRY(h->raster.wait(sm));
    for (int i = 0; i < G; i++)
        if (h->streaming) PP_TRY(h->dl[kGridSide].fetched[h->grp_gs[i]].wait_unless_done(sm));   // GridOut set still being downloaded
    dmpp::TickGroup tg;                                                // slot i: sets grp_set[0] + i, grp_gs[0] + i
    tg.n = n; tg.in = h->grp_in;
    tg.obs_now = h->percept.on ? h->percept.d_seen[set0] : h->d_obs_now[set0]; tg.obs_stride = std::max(h->caps.max_obs_total, 1);
    tg.paths = h->d_path[set0]; tg.path_stride = (long long)h->caps.max_scenes * h->max_path0;
    tg.gout = h->d_gout[h->grp_gs[0]]; tg.gout_stride = h->caps.max_scenes;
    // launch order of the search (heaviest work items first) - pointless while every item is resident at once.  Keyed by the
    // times of the group kBuf back, the one before it on its stream (one-stream tick: by the previous one's).
    const bool order_scenes = items > h->search_slots;
    const int32_t* perm = order_scenes ? h->d_perm[p] : nullptr;
    if (perm)
        hipLaunchKernelGGL(dmpp::k_order, dim3(1), dim3(dmpp::kOrderBlock), 0, sm, items, h->d_cost[piped ? p : h->grp_p_prev], h->d_perm[p]);
    int32_t* need = h->d_need[set0];                                   // the group's LDS need and retry count
    {
        const int budget = h->search_force_gbm ? 0 : h->lds_budget_launch;
        const bool wide = items <= kScoreWideMaxScenes;       // a few scenes: sixteen waves set each scene up (the latency-bound tick)
        const size_t dyn = std::max((size_t)h->search_meta_bytes + 8 * (size_t)budget, (size_t)h->gbm_lds);
        const bool use_spill = h->d_ospill[p] != nullptr && c.bucket_cap > DMPP_OPEN_CAP;     // scenes whose open list outgrows LDS are searched again, spilling
        Timed t(h, PP_K_SEARCH, sm, G);
        switch (h->search_kind) {
#define DMPP_LAUNCH_SEARCH(K)                                                                                                                  \
        case K:                                                                                                                                \
            if (wide) hipLaunchKernelGGL((dmpp::k_search<K, dmpp::kSearchSetupWavesWide>), dim3(items), dim3(dmpp::kSearchSetupWavesWide * DMPP_WAVE), dyn, sm, c, items, tg, \
                                         h->caps.order_cap, budget, perm, h->d_closed[p], h->d_pinfo[p], h->d_order[p], h->d_gbm[p],                   \
                                         h->d_cost[p], h->d_ovf[p], need, h->d_ospill[p], h->spill_cap, h->d_retry[p], use_spill ? need + 1 : nullptr); \
            else hipLaunchKernelGGL((dmpp::k_search<K, dmpp::kSearchSetupWaves>), dim3(items), dim3(dmpp::kSearchBlock), dyn, sm, c, items, tg,        \
                                    h->caps.order_cap, budget, perm, h->d_closed[p], h->d_pinfo[p], h->d_order[p], h->d_gbm[p],                        \
                                    h->d_cost[p], h->d_ovf[p], need, h->d_ospill[p], h->spill_cap, h->d_retry[p], use_spill ? need + 1 : nullptr);      \
            if (use_spill) hipLaunchKernelGGL((dmpp::k_search_spill<K>), dim3(std::min(items, 2)), dim3(dmpp::kSearchBlock), dyn, sm, c, items, tg,    \
                                              h->caps.order_cap, budget, h->d_closed[p], h->d_pinfo[p], h->d_order[p], h->d_gbm[p],                    \
                                              h->d_cost[p], h->d_ovf[p], need, h->d_ospill[p], h->spill_cap, h->d_retry[p], need + 1);                  \
            break;
        DMPP_LAUNCH_SEARCH(0) DMPP_LAUNCH_SEARCH(1) DMPP_LAUNCH_SEARCH(2)
#undef DMPP_LAUNCH_SEARCH
        }
    }
    if (piped) PP_TRY(h->searched[p].record(sm));     // (what a later one-stream group waits for)
    else h->searched[p].forget();                     // (one-stream mode: stream order is enough, no events on the latency path)
    {
        Timed t(h, PP_K_SCORE, ss, G);
        int32_t* need_host = (!h->lds_budget_fixed && !h->search_force_gbm) ? &h->h_need[set0] : nullptr;
        if (items <= kScoreWideMaxScenes)     // few scenes: sixteen waves per scene (17 candidates in two rounds)
            hipLaunchKernelGGL(dmpp::k_score<16>, dim3(items), dim3(16 * DMPP_WAVE), sizeof(dmpp::ScoreShared<16>), ss, c, items, tg, need, need_host);
        else
            hipLaunchKernelGGL(dmpp::k_score<4>, dim3(items), dim3(4 * DMPP_WAVE), sizeof(dmpp::ScoreShared<4>), ss, c, items, tg, need, need_host);
    }
    if (h->score.grp_scored) {                             // scorecard, grid half: behind the tick's k_score, in front of scored[] / the tick's ev_tail (a scored tick is a group of 1)
        hipLaunchKernelGGL(dmpp::k_score_grid, dim3((unsigned)((n + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, ss,
                           n, std::min(c.n_lattice, DMPP_MAX_LATTICE - 1), h->d_gout[h->grp_gs[G - 1]], h->score.d_grid[p]);
        h->score.grp_scored = false;
    }
    if (h->packed.on && h->packed.d_grid[0]) {             // packed fetch, grid half: behind the tick's k_score in stream order, in front of scored[] / the tick's ev_tail (an armed handle runs groups of 1)
        Timed t(h, PP_K_PACK_GRID, ss);
        hipLaunchKernelGGL(dmpp::k_pack_grid, dim3((unsigned)((n + dmpp::kPkGridWaves - 1) / dmpp::kPkGridWaves)), dim3(dmpp::kPkGridWaves * DMPP_WAVE), 0, ss,
                           c, n, tg, G - 1, h->packed.d_grid[h->grp_gs[G - 1] / kGroupMax].get());
    }
    for (int i = 0; i < G; i++) {                 // the group's scoring pass is the last reader of its G snapshot sets
        if (piped) PP_TRY(h->scored[h->grp_set[i]].record(ss));
        else h->scored[h->grp_set[i]].forget();
    }
    if (!piped) PP_TRY(h->join.wait(h->stream));     // one-stream mode: the tick is complete on the handle's stream
    h->need_set = set0; h->item_off = (G - 1) * n;
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

// Opens a tick group at the next ring positions: its size G - from the workgroup slots the last group's budget gave -, then the
// LDS budget of its search (dmpp::search_budget).  The need of the densest scene of an earlier group: the scoring pass behind
// each search stores it in pinned memory, which is simply read here - whatever has landed; never waited for.
void open_group(pp_planner* h, int n, bool piped)
{
    const bool grid = h->cfg.grid_stage != 0;
    h->grp_p_prev = h->parity;
    if (grid) { h->parity = (h->parity + 1) % kBuf; h->gring = (h->gring + 1) % kGoutRing; }
    h->ring = (h->ring + 1) % kRing;
    h->grp_G = (piped && !h->streaming) ? group_size(n, h->search_slots, h->gcap, h->tick_group) : 1;
    h->grp_n = n; h->grp_piped = piped;
    if (!grid) return;
    int need = -1;
    if (!h->lds_budget_fixed && !h->search_force_gbm) {
        for (int q = 0; q < kBuf; q++) need = std::max(need, (int)reinterpret_cast<volatile int32_t*>(h->h_need.get())[((h->ring + kRing - 1 - q) % kRing) * kGroupMax]);     // the last kBuf groups' sets
        if (need >= 0) h->need_seen = need;
    }
    const dmpp::SearchBudget b = dmpp::search_budget(h->search_static_lds, h->search_meta_bytes, h->gbm_lds, h->lds_budget_max, h->n_cus, n, h->grp_G, h->cur_in().n_obs_total,
                                                     need, h->lds_budget, h->budget_from_need, h->lds_budget_fixed, h->search_force_gbm);
    h->lds_budget = b.budget; h->budget_from_need = b.from_need; h->search_slots = b.slots;
    // what the launch gets: room for a front or scoring workgroup beside the searches, where a tighter budget buys it.  The
    // policy's own budget stays in lds_budget for the next group's hysteresis; G and search_slots keep the policy's count.
    h->lds_budget_launch = h->coresident ? dmpp::coresident_budget(h->search_static_lds, h->search_meta_bytes, h->gbm_lds, h->lds_budget_max, h->n_cus, h->grp_G * n, need,
                                                                    b.budget, h->lds_budget_fixed, h->search_force_gbm, kBesideSearchLds)
                                         : b.budget;
}

}  // namespace

extern "C" {

int pp_plan_tick(pp_handle h)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    const int n = h->n_scenes;
    if (n <= 0) return PP_OK;
    HIP_TRY(hipSetDevice(h->device));
    const PlannerConfig& c = h->cfg;
    if (c.decision_stage && c.lanechg_stage && !h->have_attr)
        return fail(PP_ERR_ARG, "cfg.lanechg_stage needs the lane attribute pool (pp_set_scenes lane_attr_pool)");
    const bool piped = tick_piped(h);                                  // the chains and their streams: tick_streams
    // streamed inputs: the update staged by pp_update_async becomes the set this tick (and the following ones) read
    bool adopted = false;
    if (h->in_staged >= 0) { h->in_cur = h->in_staged; h->in_staged = -1; h->rollout.staged_by_advance = false; adopted = true; }
    if (h->grp_ticks == 0) open_group(h, n, piped);
    const int slot = h->grp_ticks, G = h->grp_G;
    const int po = h->ring * kGroupMax + slot;                                        // this tick's snapshot set
    const int gs = c.grid_stage ? h->gring * kGroupMax + slot : h->gout_set;          // ... and GridOut set
    if (h->streaming) {
        // downloads whose kernels have finished are issued now; one that still reads a set this tick overwrites is issued whatever
        int r = pump_fetches(h, -1, (h->plan_cur + 1) % kPlan, c.grid_stage ? gs : -1); if (r) return r;
        r = prune_inflight(h); if (r) return r;
        h->plan_cur = (h->plan_cur + 1) % kPlan;
        if (!adopted) h->h_bad[(h->tick_seq + 1) % kDone] = 0;
    }
    const TickStreams T = tick_streams(h, piped, c.grid_stage != 0, h->parity);
    hipStream_t sf = T.front, sr = T.dp;
    // The front chain overwrites snapshot set po: it waits for the scoring pass of the last group that read it (2 kBuf groups back).
    // It does not wait for the search kBuf groups back: it runs ahead - up to 2 kBuf groups, bounded by the snapshot
    // sets - so its kernels no longer start together with the scoring pass that follows that search (+ 2 %), and the launch order,
    // which needs that search's times, is computed on the search's own stream.
    PP_TRY(h->scored[po].wait(sf));
    if (sf == h->stream && h->front_unjoined) PP_TRY(h->join.wait(sf));   // Planning(t-1) -> snapshot(t) when not on the same stream
    h->front_unjoined = false;
    if (h->r_on_main && sf != h->stream) {         // Planning(t-1) ran on the handle's stream (grid stage off then): the front chain reads its state
        PP_TRY(h->fork.record(h->stream)); PP_TRY(h->fork.wait(sf));
    }
    h->r_on_main = sr == h->stream;
    const InputSet& I = h->cur_in(); PlanOut* d_plan = h->plan_out();      // the sets this tick reads and writes
    const SyncPoint& up = I.up;
    const bool behind_upload = adopted && up.recorded();
    if (behind_upload) PP_TRY(up.wait_unless_done(sf));                   // every kernel of the tick follows the snapshot kernel
    if (h->streaming) PP_TRY(h->dl[kPlanSide].fetched[h->plan_cur].wait_unless_done(sr));   // PlanOut set still being downloaded (kPlan ticks ago)
    // Scorecard: k_score_ego of the last scored tick (upload stream) reads the SceneState this front chain rewrites, and sets of the
    // PlanOut and snapshot rings that a later one does.  A tick that adopts an update or an advance waits for that set's `up`,
    // recorded behind the kernel on the same stream (staging always follows the tick it follows); any other tick waits here.
    if (h->score.ego.done()) h->score.ego.forget();
    else if (!behind_upload) PP_TRY(h->score.ego.wait(sf));
    ObPoint* obs_now = h->d_obs_now[po];
    // Perception (§4w): k_perceive writes the truth into obs_now and what the planner may see into the set of the same index of the
    // perceived ring - same writer, same readers as obs_now[po], so scored[po] above covers both.  Planners get obs_plan, judges obs_now.
    const bool perceive = h->percept.on;
    const ObPoint* obs_plan = perceive ? h->percept.d_seen[po] : obs_now;
    // Snapshot and Decision on one stream (piped ticks, ticks without the grid stage): the snapshot is the head of k_decision<true>,
    // one launch less per tick.  Every reader of the set waits for something behind that kernel: the searches for `raster`,
    // recorded behind it; Planning, k_score_ego (ev_front) and join_all for stream order on sr.  (`raster` behind k_planning
    // instead, beside `join`, was measured: the gap an event costs between two kernels moves with it and doubles there, and the
    // 20-step leg loses 2 % to the later start of its searches - profiles/r25_front_two_launch.txt.)
    // Streamed handles keep the separate launch: their groups are single ticks, every search waits for its own tick's `raster`, and
    // starting each one k_decision later cost the streamed leg 1.3 %, more than its spread (same file).
    const bool snap_fused = h->front_snapshot && c.decision_stage && sf == sr && !h->streaming && !perceive;
    const ObMotion* mot = I.mot();
    if (perceive) {
        Timed t(h, PP_K_PERCEIVE, sf);
        hipLaunchKernelGGL(dmpp::k_perceive, dim3((unsigned)((n + dmpp::kPcScenes - 1) / dmpp::kPcScenes)), dim3(dmpp::kBlock), 0, sf, c, h->percept.pm, n,
                           std::min(I.n_obs_total, h->caps.max_obs_total), h->tick_seq + 1, I.d_in, h->d_state, I.d_obs, mot,
                           h->episode.on ? h->episode.d_stats.get() : nullptr, obs_now, h->percept.d_seen[po], h->percept.d_track.get(), h->percept.d_stats.get());
    } else if (!snap_fused) {
        Timed t(h, PP_K_OBSTACLES, sf);
        hipLaunchKernelGGL(dmpp::k_effective_obstacles, dim3(n), dim3(dmpp::kBlock), 0, sf, c, n, I.d_in, h->d_state, I.d_obs, mot, obs_now);
    }
    if (sr != sf) { PP_TRY(h->fork.record(sf)); PP_TRY(h->fork.wait(sr)); }   // small batches: Decision + Planning beside the grid engine
    const bool search_waits = c.grid_stage && sf != T.search;                // the search rasterises for itself: it only needs the obstacle snapshot
    if (search_waits && !snap_fused) PP_TRY(h->raster.record(sf));
    if (c.decision_stage) {
        Timed t(h, PP_K_DECISION, sr);
        if (snap_fused)
            hipLaunchKernelGGL(dmpp::k_decision<true>, dim3(n), dim3(dmpp::kBlock), sizeof(dmpp::DecShared), sr, c, n, I.d_in, h->d_lane,
                               h->d_attr, h->d_ref, I.d_obs, mot, obs_now, h->d_state, d_plan, h->d_dec_ref);
        else
            hipLaunchKernelGGL(dmpp::k_decision<false>, dim3(n), dim3(dmpp::kBlock), sizeof(dmpp::DecShared), sr, c, n, I.d_in, h->d_lane,
                               h->d_attr, h->d_ref, I.d_obs, mot, const_cast<ObPoint*>(obs_plan), h->d_state, d_plan, h->d_dec_ref);
    }
    if (search_waits && snap_fused) PP_TRY(h->raster.record(sf));
    {
        Timed t(h, PP_K_PLANNING, sr);
        hipLaunchKernelGGL(dmpp::k_planning, dim3(n), dim3(dmpp::kBlock), sizeof(dmpp::PlanShared), sr, c, n, I.d_in, h->d_lane,
                           h->d_ref, h->d_dec_ref, obs_plan, h->d_state, d_plan);
    }
    if (h->packed.on) {          // packed fetch, plan half: behind the Planning kernel in stream order, in front of `join` and the tick's ev_front
        {
            Timed t(h, PP_K_PACK_PLAN, sr);
            const long long chunks = (long long)n * dmpp::kPkPlanChunks;
            hipLaunchKernelGGL(dmpp::k_pack_plan, dim3((unsigned)((chunks + dmpp::kPkBlock - 1) / dmpp::kPkBlock)), dim3(dmpp::kPkBlock), 0, sr,
                               n, d_plan, h->packed.d_plan[h->plan_cur].get());
        }
        h->packed.plan_tick = h->tick_seq + 1;
        if (c.grid_stage) h->packed.grid_tick = h->tick_seq + 1;      // (its group - of 1 - is launched below)
    }
    if (sr != h->stream) { PP_TRY(h->join.record(sr)); h->front_unjoined = piped; }
    h->obs_set = po;
    if (c.grid_stage) {
        h->grp_set[slot] = po; h->grp_gs[slot] = gs; h->grp_in = I.d_in;
        h->grp_ticks = slot + 1;
        h->gout_set = gs; h->path_set = po;
        h->score.grp_scored = h->score.on;
        if (slot + 1 == G) { int r = flush_group(h); if (r) return r; }
    }
    h->last_piped = piped;
    h->tick_seq++;
    if (h->streaming) {          // what a later update of this tick's input set, and a download of its results, wait for
        TickRec rec = { h->tick_seq, h->in_cur, get_sync_event(h), c.grid_stage ? get_sync_event(h) : nullptr };
        if (!rec.ev_front || (c.grid_stage && !rec.ev_tail)) return fail(PP_ERR_HIP, "event creation failed");
        HIP_TRY(hipEventRecord(rec.ev_front, sr));
        if (rec.ev_tail) HIP_TRY(hipEventRecord(rec.ev_tail, T.score));
        h->inflight.push_back(rec); h->rec_last = rec;
        if (h->score.on) {        // scorecard, front half: behind this tick's Planning kernel, on the upload stream - in front of the advance that may follow
            hipStream_t su = h->stream_up;
            HIP_TRY(hipStreamWaitEvent(su, rec.ev_front, 0));
            const dim3 sgrid((unsigned)((n + dmpp::kScScenes - 1) / dmpp::kScScenes));
            // episode log: the tick is folded into the scorecards of the running episodes too (§4n 3.); score trace: lane 0 stores the
            // tick's record into the scene's ring in front of the fold (§4o) - EpisodeStats only while episodes are on
            // conflict score: every lane differences its entries against the snapshot of the scored tick before and stores them for the
            // next one, lane 0 folds the tick's TTC and DRAC in front of both (§4u); the two buffers change places behind every launch
            const bool log = h->elog.on && h->elog.d_score, trace = h->strace.on, conflict = h->conflict.on;
            RolloutScore* ep_score = log ? h->elog.d_score.get() : nullptr;
            const EpisodeStats* ep_stats = (trace || conflict) && h->episode.on ? h->episode.d_stats.get() : nullptr;
            ScoreTraceInfo* tinfo = trace ? h->strace.d_info.get() : nullptr;
            ScoreTick* tring = trace ? h->strace.d_ring.get() : nullptr;
            ConflictScore* cscore = conflict ? h->conflict.d_score.get() : nullptr;
            const ObPoint* prev = conflict ? h->conflict.d_prev[h->conflict.cur].get() : nullptr;
            ObPoint* prev_next = conflict ? h->conflict.d_prev[h->conflict.cur ^ 1].get() : nullptr;
            auto* kern = conflict ? (log ? (trace ? dmpp::k_score_ego<true, true, true> : dmpp::k_score_ego<true, false, true>)
                                         : (trace ? dmpp::k_score_ego<false, true, true> : dmpp::k_score_ego<false, false, true>))
                                  : (log ? (trace ? dmpp::k_score_ego<true, true, false> : dmpp::k_score_ego<true, false, false>)
                                         : (trace ? dmpp::k_score_ego<false, true, false> : dmpp::k_score_ego<false, false, false>));
            hipLaunchKernelGGL(kern, sgrid, dim3(dmpp::kBlock), 0, su, 0.5 * c.Vehicle_Width, h->score.dt, n, I.n_obs_total,
                               I.d_in, d_plan, h->d_state, obs_now, h->rollout.d_flags, h->score.d_score, ep_score,
                               h->tick_seq, h->strace.tm, ep_stats, tinfo, tring, h->conflict.cm, cscore, prev, prev_next);
            if (conflict) h->conflict.cur ^= 1;
            PP_TRY(h->score.ego.record(su));
        }
    }
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

int pp_join(pp_handle h)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    return join_all(h);
}

int pp_sync(pp_handle h)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    { int r = join_all(h); if (r) return r; }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->streaming) {          // staged updates and downloads too (everything has finished: every pending copy is issued)
        int r = pump_fetches(h); if (r) return r;
        for (hipStream_t st : { h->stream_up, h->dl[kPlanSide].stream, h->dl[kGridSide].stream }) HIP_TRY(hipStreamSynchronize(st));
    }
    return PP_OK;
}

int pp_device_synchronize(pp_handle h)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    { int r = pp_sync(h); if (r) return r; }
    HIP_TRY(hipDeviceSynchronize());
    return PP_OK;
}

static int fetch(pp_handle h, void* dst, const void* src, size_t bytes)
{
    HIP_TRY(hipSetDevice(h->device));
    PP_TRY(join_all(h));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}
// ... of what the upload stream writes: behind a staged advance too, and - also_staged_update - behind a staged update, which rewrites the same values
static int fetch_behind_advance(pp_handle h, void* dst, const void* src, size_t bytes, bool also_staged_update)
{
    HIP_TRY(hipSetDevice(h->device));
    PP_TRY(h->rollout.adv.wait(h->stream));
    if (also_staged_update && h->in_staged >= 0) PP_TRY(h->in_sets[h->in_staged].up.wait(h->stream));
    return fetch(h, dst, src, bytes);
}

int pp_get_plan(pp_handle h, PlanOut* out, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    return fetch(h, out, h->plan_out(), (size_t)n * sizeof(PlanOut));
}
int pp_get_state(pp_handle h, SceneState* st, int n)
{
    if (!h || !st) return fail(PP_ERR_ARG, "null argument");
    if (n < 0 || n > h->caps.max_scenes) return fail(PP_ERR_ARG, "n exceeds capacity");
    if (h->episode.on) {      // episodes: the upload stream writes SceneState too (a staged advance restores start states), and fetch only joins the tick streams
        HIP_TRY(hipSetDevice(h->device));
        PP_TRY(h->rollout.adv.wait(h->stream));
    }
    return fetch(h, st, h->d_state, (size_t)n * sizeof(SceneState));
}
int pp_get_grid_out(pp_handle h, GridOut* out, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    return fetch(h, out, h->d_gout[h->gout_set], (size_t)n * sizeof(GridOut));
}
int pp_get_grid(pp_handle h, int scene, uint8_t* grid)
{
    if (!h || !grid || !h->d_grid) return fail(PP_ERR_ARG, "no grid");
    if (scene < 0 || scene >= h->n_scenes) return fail(PP_ERR_ARG, "scene out of range");
    const PlannerConfig& c = h->cfg;
    const size_t N = (size_t)c.grid_w * c.grid_h;
    // No occupancy grid exists after a tick: the search builds its sparse bitmaps in LDS and drops them.  The grid asked for is
    // produced here, from the obstacle snapshot of the last tick, by the same footprint code (k_export_grid), which also checks
    // the column-major view against the row-major one (unless the scene is too dense for one workgroup's LDS).
    HIP_TRY(hipSetDevice(h->device));
    { int r = join_all(h); if (r) return r; }       // the snapshot of the last tick was written on another stream
    const ObPoint* obs_now = h->percept.on ? h->percept.d_seen[h->obs_set] : h->d_obs_now[h->obs_set];      // what the search rasterised (§4w)
    int bad[2] = { 0, 0 };
    HIP_TRY(hipMemsetAsync(h->d_gridbad, 0, 2 * sizeof(int), h->stream));
    const int budget = h->search_force_gbm ? 1 : h->lds_budget_max;      // (1 word: nothing fits, the span-by-span path)
    const size_t dyn = (size_t)h->search_meta_bytes + 8 * (size_t)budget;
    switch (h->search_kind) {
    case 0: hipLaunchKernelGGL(dmpp::k_export_grid<0>, dim3(1), dim3(dmpp::kSearchBlock), dyn, h->stream, c, scene, budget, h->cur_in().d_in, obs_now, h->d_grid, h->d_gridbad); break;
    case 1: hipLaunchKernelGGL(dmpp::k_export_grid<1>, dim3(1), dim3(dmpp::kSearchBlock), dyn, h->stream, c, scene, budget, h->cur_in().d_in, obs_now, h->d_grid, h->d_gridbad); break;
    default: hipLaunchKernelGGL(dmpp::k_export_grid<2>, dim3(1), dim3(dmpp::kSearchBlock), dyn, h->stream, c, scene, budget, h->cur_in().d_in, obs_now, h->d_grid, h->d_gridbad); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(bad, h->d_gridbad, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (bad[0]) return fail(PP_ERR_STATE, "pp_get_grid: the row-major and column-major views of the scene differ in " + std::to_string(bad[0]) + " cell(s)");
    return fetch(h, grid, h->d_grid, N);
}
int pp_get_search_info(pp_handle h, int32_t* lds_budget_words, int32_t* need_words, int32_t* dense_scenes)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!h->d_ovf[0]) return fail(PP_ERR_STATE, "handle was created without the grid stage");
    HIP_TRY(hipSetDevice(h->device));
    { int r = flush_group(h); if (r) return r; }          // parity / item_off / need_set name the last tick only once its group is launched
    if (lds_budget_words) *lds_budget_words = h->search_force_gbm ? 0 : h->lds_budget_launch;
    if (need_words) {                      // what the densest scene of the last tick needed (its scoring pass has stored it by now)
        { int r = join_all(h); if (r) return r; }
        HIP_TRY(hipStreamSynchronize(h->stream));
        const int32_t v = reinterpret_cast<volatile int32_t*>(h->h_need.get())[h->need_set];
        if (v >= 0) h->need_seen = v;
        *need_words = h->need_seen;
    }
    if (dense_scenes) {
        std::vector<int32_t> ovf((size_t)std::max(h->n_scenes, 1));
        int r = fetch(h, ovf.data(), h->d_ovf[h->parity] + h->item_off, (size_t)h->n_scenes * sizeof(int32_t)); if (r) return r;
        int k = 0; for (int i = 0; i < h->n_scenes; i++) k += ovf[(size_t)i] != 0;
        *dense_scenes = k;
    }
    return PP_OK;
}
int pp_get_order(pp_handle h, int scene, int32_t* order, int cap)
{
    if (!h || !order || !h->d_order[0]) return fail(PP_ERR_STATE, "expansion order was not requested (caps.order_cap == 0)");
    if (scene < 0 || scene >= h->n_scenes) return fail(PP_ERR_ARG, "scene out of range");
    if (cap > h->caps.order_cap) cap = h->caps.order_cap;
    HIP_TRY(hipSetDevice(h->device));
    { int r = flush_group(h); if (r) return r; }          // (item_off is the last tick's only once its group is launched)
    return fetch(h, order, h->d_order[h->parity] + ((size_t)h->item_off + scene) * h->caps.order_cap, (size_t)cap * sizeof(int32_t));
}
int pp_get_refpath(pp_handle h, int scene, GlobalPoint2D* pts, int cap)
{
    if (!h || !pts) return fail(PP_ERR_ARG, "null argument");
    if (scene < 0 || scene >= h->n_scenes) return fail(PP_ERR_ARG, "scene out of range");
    if (cap > DMPP_MAX_REFPATH) cap = DMPP_MAX_REFPATH;
    return fetch(h, pts, h->d_dec_ref + (size_t)scene * DMPP_MAX_REFPATH, (size_t)cap * sizeof(GlobalPoint2D));
}
int pp_get_path(pp_handle h, int scene, int32_t* path, int cap)
{
    if (!h || !path || !h->d_path[0]) return fail(PP_ERR_ARG, "no path buffer");
    if (scene < 0 || scene >= h->n_scenes) return fail(PP_ERR_ARG, "scene out of range");
    if (cap > h->cfg.max_path) cap = h->cfg.max_path;
    return fetch(h, path, h->d_path[h->path_set] + (size_t)scene * h->cfg.max_path, (size_t)cap * sizeof(int32_t));
}

int pp_plan_tick_batch(pp_handle h, int n_scenes, const SceneIn* in, const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total,
                       const GlobalPoint3D* lane_pool, const uint8_t* lane_attr_pool, int n_lane_pts,
                       const GlobalPoint2D* ref_pool, int n_ref_pts, SceneState* state_inout, PlanOut* out, GridOut* grid_out)
{
    if (!h || !state_inout || !out) return fail(PP_ERR_ARG, "null argument");
    int r;
    if ((r = pp_set_scenes(h, n_scenes, in, lane_pool, lane_attr_pool, n_lane_pts, ref_pool, n_ref_pts, obs_pool, mot_pool, n_obs_total))) return r;
    if ((r = pp_set_state(h, state_inout, n_scenes))) return r;
    if ((r = pp_plan_tick(h))) return r;
    if ((r = pp_get_plan(h, out, n_scenes))) return r;
    if ((r = pp_get_state(h, state_inout, n_scenes))) return r;
    if (grid_out && h->cfg.grid_stage && (r = pp_get_grid_out(h, grid_out, n_scenes))) return r;
    return PP_OK;
}

// ---------------------------------------------------------------------------------------
// Streamed ticks: new inputs every tick, results out every tick, no host wait in between.
// The reference reads its blackboard at the top of every tick (Planning.cpp:95-112, Decision.cpp:155-160) and publishes at
// the end of it (Planning.cpp:186,214; Decision.cpp:203).

static int ensure_streaming(pp_handle h)
{
    if (h->streaming) return PP_OK;
    const size_t ns = (size_t)h->caps.max_scenes, no = (size_t)(h->caps.max_obs_total > 0 ? h->caps.max_obs_total : 1);
    int r;
    for (int q = 0; q < kIn; q++) {
        InputSet& I = h->in_sets[q];
        if (!I.d_in && (r = I.d_in.reserve(ns))) return r;
        if (!I.d_obs && (r = I.d_obs.reserve(no))) return r;
        if (!I.d_mot) { if ((r = I.d_mot.reserve(no))) return r; HIP_TRY(hipMemsetAsync(I.d_mot, 0, no * sizeof(ObMotion), h->stream)); }
    }
    for (int q = 1; q < kPlan; q++) if (!h->d_plan_ring[q]) {
        if ((r = h->d_plan_ring[q].reserve(ns))) return r;
        HIP_TRY(hipMemsetAsync(h->d_plan_ring[q], 0, ns * sizeof(PlanOut), h->stream));
    }
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    // the upload carries two small kernels (map views, slice check) that the next front chain waits for: top priority
    if (!h->stream_up) HIP_TRY(hipStreamCreateWithPriority(&h->stream_up, hipStreamNonBlocking, prio_greatest));
    for (FetchSide& S : h->dl) if (!S.stream) HIP_TRY(hipStreamCreateWithPriority(&S.stream, hipStreamNonBlocking, prio_least));
    if (!h->h_bad) { int r2 = h->h_bad.alloc(kDone); if (r2) return r2; for (int q = 0; q < kDone; q++) h->h_bad[q] = 0; }
    // everything enqueued before streaming began (ticks, the memsets above) is ordered before the three new streams
    { int r2 = join_all(h); if (r2) return r2; }
    hipEvent_t e = get_sync_event(h);
    if (!e) return fail(PP_ERR_HIP, "event creation failed");
    HIP_TRY(hipEventRecord(e, h->stream));
    for (hipStream_t st : { h->stream_up, h->dl[kPlanSide].stream, h->dl[kGridSide].stream }) HIP_TRY(hipStreamWaitEvent(st, e, 0));
    HIP_TRY(hipStreamSynchronize(h->stream));      // (once per handle) so that e can go back to the pool
    h->sync_events.push_back(e);
    h->streaming = true;
    return PP_OK;
}

// What the next tick reads, staged on the upload stream by pp_update_async (host arrays: `in` and / or `obs_pool`) or by
// pp_advance_async (`ego`: the SceneIn records are produced on the device)
struct StageSource {
    const SceneIn* in = nullptr; const ObPoint* obs_pool = nullptr; const ObMotion* mot_pool = nullptr; int n_obs_total = 0;
    const EgoModel* ego = nullptr; EgoTrace* trace = nullptr;
};

// Stages an input set for the next tick; the callers have checked their arguments.  An update goes into the set after the current
// one, or - a second update - onto the set already staged, and carries over from that set what it leaves alone.  An advance
// (closed-loop rollout) always takes the set after the current one - its caller refuses while something is
// staged - and puts k_advance_egos / k_advance_route in the place of the copy of the SceneIn records: the kernel reads what the
// last tick's Planning kernel wrote (PlanOut, SceneState), so the upload stream waits for that tick's front-chain event, not for
// its search; the next tick's front chain, the only writer of SceneState, waits for the set's `up` in turn.
// Order on the upload stream ("The upload stream of one advance"): SceneIn records - an advance: advance_egos -> step_episodes - and obstacle
// pool -> k_move_traffic / follow_traffic (-> k_reset_traffic, §4m) -> k_couple_fleet (the two write disjoint pool
// entries: traffic a scene's own, the fleet the peer slots behind them, at the poses just staged) -> k_resolve_map ->
// k_sanitise_scenes -> `up`, which the tick that adopts the set waits for.
static int stage_inputs(pp_handle h, const StageSource& src)
{
    const bool advance = src.ego != nullptr;
    { int r = flush_group(h); if (r) return r; }          // the ticks before streaming began are launched as they stand
    { int r = ensure_streaming(h); if (r) return r; }     // (a tick enqueued before streaming began has finished behind this: one host wait per handle)
    { int r = pump_fetches(h); if (r) return r; }
    { int r = prune_inflight(h); if (r) return r; }
    hipStream_t su = h->stream_up;
    if (advance && !h->rollout.d_flags) {
        int r = h->rollout.d_flags.reserve((size_t)h->caps.max_scenes); if (r) return r;
        HIP_TRY(hipMemsetAsync(h->rollout.d_flags, 0, (size_t)h->caps.max_scenes * sizeof(int32_t), su));
    }
    const bool restage = h->in_staged >= 0;
    const int s = restage ? h->in_staged : (h->in_cur + 1) % kIn, n = h->n_scenes;
    // what the call leaves alone is carried over from the set it replaces (the staged one if there is one)
    const InputSet& P = h->in_sets[restage ? h->in_staged : h->in_cur];
    InputSet& I = h->in_sets[s];
    for (const TickRec& r : h->inflight) if (r.in_set == s) {      // the ticks that still read set s (a whole ring ago: long finished, as a rule)
        HIP_TRY(hipStreamWaitEvent(su, r.ev_front, 0));
        if (r.ev_tail) HIP_TRY(hipStreamWaitEvent(su, r.ev_tail, 0));
    }
    if (advance && h->rec_last.tick == h->tick_seq && h->rec_last.ev_front) HIP_TRY(hipStreamWaitEvent(su, h->rec_last.ev_front, 0));
    if (src.in) HIP_TRY(hipMemcpyAsync(I.d_in, src.in, (size_t)n * sizeof(SceneIn), hipMemcpyDefault, su));
    else if (!advance && &P != &I) HIP_TRY(hipMemcpyAsync(I.d_in, P.d_in, (size_t)n * sizeof(SceneIn), hipMemcpyDeviceToDevice, su));
    int n_obs = src.n_obs_total; bool have_motion = false;
    if (src.obs_pool) {
        if (n_obs) HIP_TRY(hipMemcpyAsync(I.d_obs, src.obs_pool, (size_t)n_obs * sizeof(ObPoint), hipMemcpyDefault, su));
        if (n_obs && src.mot_pool) { HIP_TRY(hipMemcpyAsync(I.d_mot, src.mot_pool, (size_t)n_obs * sizeof(ObMotion), hipMemcpyDefault, su)); have_motion = true; }
    } else {
        n_obs = P.n_obs_total; have_motion = P.have_motion;
        if (&P != &I && n_obs) {
            HIP_TRY(hipMemcpyAsync(I.d_obs, P.d_obs, (size_t)n_obs * sizeof(ObPoint), hipMemcpyDeviceToDevice, su));
            if (have_motion) HIP_TRY(hipMemcpyAsync(I.d_mot, P.d_mot, (size_t)n_obs * sizeof(ObMotion), hipMemcpyDeviceToDevice, su));
        }
    }
    SceneIn* d_in = I.d_in; ObPoint* d_obs = I.d_obs; ObMotion* d_mot = have_motion ? I.d_mot.get() : nullptr;
    if (advance) {
        advance_egos(h, su, *src.ego, P.d_in, d_in, src.trace);
        if (h->episode.on) step_episodes(h, su, P, d_in, src.trace);
    }
    if (h->traffic.on) {                  // an advance moves the actors one step on - by the car-following law while that is on (§4i) -, an update places them where they are
        if (h->man.on) { int r = manoeuvre_traffic(h, su, d_in, d_obs, d_mot, advance ? src.ego->dt : 0.0); if (r) return r; }      // (§4v: in the place of either)
        else if (advance && h->follow.on) { int r = follow_traffic(h, su, d_in, d_obs, d_mot, src.ego->dt); if (r) return r; }
        else move_traffic(h, su, d_obs, d_mot, advance ? src.ego->dt : 0.0);
    }
    if (advance && h->treset.on) reset_traffic(h, false, su, d_obs, d_mot);      // the actors of a scene that has just restarted go back to a start state (§4m)
    if (advance && h->wreset.on) reset_traffic(h, true, su, d_obs, d_mot);      // ... and the vehicles of a world that has (§4t)
    if (h->fleet.on) {                    // the peers of this set, at the poses it carries; the pinned slices replace the incoming ones
        if (!advance) n_obs = std::max(n_obs, h->fleet.end);      // (an advance inherits the count of the current set)
        couple_fleet(h, su, d_in, d_obs, d_mot);
    }
    // The count of poisoned scenes is written by the two kernels below straight into pinned host memory: the slot of the tick
    // that will adopt this set - no memset and no copy command on the upload stream.
    // OWNER RULE of h_bad[slot of tick T + 1]: the HOST owns the slot while nothing is staged for T + 1 (no kernel that counts
    // into it has been enqueued: it zeroes it here, at the first update or advance staged for T + 1, or in pp_plan_tick when
    // T + 1 adopts nothing).  From the first staged update until pp_plan_tick adopts it the UPLOAD STREAM owns the slot:
    // k_resolve_map / k_sanitise_scenes add to it in stream order, and a repeated update that brings new SceneIn records
    // restarts the count with k_zero_word on that stream - behind the kernels of the earlier update, which a store from the
    // host could overtake.  After the adoption nobody writes it; pp_wait_tick reads it behind the tick's downloads.
    int32_t* bad_slot = &h->h_bad[(h->tick_seq + 1) % kDone];
    if (!restage) *reinterpret_cast<volatile int32_t*>(bad_slot) = 0;
    else if (src.in) hipLaunchKernelGGL(dmpp::k_zero_word, dim3(1), dim3(1), 0, su, bad_slot);      // (a second, obstacles-only update of a staged set keeps the count of the first)
    const dim3 grid((unsigned)((n + dmpp::kBlock - 1) / dmpp::kBlock)), block(dmpp::kBlock);
    if (h->resident_mode == 1 && (advance || src.in))      // egos on the resident map: lane views and junction slices from road / lane numbers (new records only)
        hipLaunchKernelGGL(dmpp::k_resolve_map, grid, block, 0, su, n, d_in, h->map_roads, h->d_map_first, h->d_map_lanes, h->d_attr, h->d_map_width,
                           h->map_junctions, h->d_map_junc, bad_slot);
    hipLaunchKernelGGL(dmpp::k_sanitise_scenes, grid, block, 0, su, n, d_in, n_obs, h->n_lane_pts, h->n_ref_pts, bad_slot);
    HIP_TRY(hipGetLastError());
    PP_TRY(I.up.record(su));
    if (advance) PP_TRY(h->rollout.adv.record(su));
    I.have_motion = have_motion; I.n_obs_total = n_obs;
    h->in_staged = s; if (advance) h->rollout.staged_by_advance = true;
    return PP_OK;
}

int pp_update_async(pp_handle h, int n_scenes, const SceneIn* in, const ObPoint* obs_pool, const ObMotion* mot_pool, int n_obs_total)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (n_scenes <= 0 || n_scenes != h->n_scenes)
        return fail(PP_ERR_STATE, "pp_update_async replaces the per-tick inputs of the resident scenes: n_scenes must be the resident count (pp_set_scenes / pp_set_egos come first)");
    if (!in && !obs_pool) return fail(PP_ERR_ARG, "nothing to update");
    if (obs_pool && (n_obs_total < 0 || n_obs_total > h->caps.max_obs_total)) return fail(PP_ERR_CAPACITY, "obstacle pool larger than caps.max_obs_total");
    if (!obs_pool && mot_pool) return fail(PP_ERR_ARG, "a motion pool without its obstacle pool");
    // with a fleet the slices are the pinned ones and the slice check runs against the end of the peer slots: a pool that stops
    // short of a scene's OWN entries would not be caught there, so it is refused here, before anything is enqueued
    if (obs_pool && h->fleet.on && n_obs_total < h->fleet.own_end)
        return fail(PP_ERR_ARG, "pp_update_async: with a fleet set the obstacle pool must cover every scene's own entries (up to entry " + std::to_string(h->fleet.own_end) + ")");
    // with traffic set every actor's pool entry is pinned: a pool that stops short of one is refused here, like the one above
    if (obs_pool && h->traffic.on && n_obs_total < h->traffic.end)
        return fail(PP_ERR_ARG, "pp_update_async: with traffic set the obstacle pool must cover every actor's entry (up to entry " + std::to_string(h->traffic.end) + ")");
    if (in && h->in_staged >= 0 && h->rollout.staged_by_advance)
        return fail(PP_ERR_STATE, "pp_update_async: the SceneIn records of the next tick were already produced by pp_advance_async");
    HIP_TRY(hipSetDevice(h->device));
    StageSource src;
    src.in = in; src.obs_pool = obs_pool; src.mot_pool = mot_pool; src.n_obs_total = n_obs_total;
    return stage_inputs(h, src);
}

int pp_advance_async(pp_handle h, const EgoModel* m, EgoTrace* trace)
{
    if (!h || !m) return fail(PP_ERR_ARG, "null argument");
    if (!(m->dt > 0) || !std::isfinite(m->dt) || !(m->max_acc >= 0) || !std::isfinite(m->max_acc) || !(m->max_dec >= 0) || !std::isfinite(m->max_dec) ||
        m->window < 1 || m->window > (1 << 20))
        return fail(PP_ERR_ARG, "pp_advance_async: the model needs a finite dt > 0, finite max_acc / max_dec >= 0 and a window of 1 .. 2^20 points");
    if (h->n_scenes <= 0 || h->tick_seq <= h->rollout.set_tick)
        return fail(PP_ERR_STATE, "pp_advance_async: no tick has been enqueued for the resident scenes (the egos follow the plan of their last tick)");
    if (h->in_staged >= 0) return fail(PP_ERR_STATE, "pp_advance_async: an update is already staged for the next tick");
    HIP_TRY(hipSetDevice(h->device));
    StageSource src;
    src.ego = m; src.trace = trace;
    return stage_inputs(h, src);
}

int pp_rollout(pp_handle h, int n_ticks, const EgoModel* m, EgoTrace* trace, long long* last_tick_id)
{
    if (!h || !m) return fail(PP_ERR_ARG, "null argument");
    if (n_ticks < 0) return fail(PP_ERR_ARG, "pp_rollout: negative tick count");
    if (h->n_scenes <= 0) return fail(PP_ERR_STATE, "pp_rollout: no resident scenes");
    if (h->tick_seq <= h->rollout.set_tick) { int r = pp_plan_tick(h); if (r) return r; }      // the plan the first advance follows
    for (int t = 0; t < n_ticks; t++) {
        int r = pp_advance_async(h, m, trace ? trace + (size_t)t * (size_t)h->n_scenes : nullptr); if (r) return r;
        r = pp_plan_tick(h); if (r) return r;
    }
    if (last_tick_id) *last_tick_id = h->tick_seq;
    return PP_OK;
}

int pp_get_ego_flags(pp_handle h, int32_t* flags, int n)
{
    if (!h || !flags) return fail(PP_ERR_ARG, "null argument");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    if (!h->rollout.d_flags) { std::memset(flags, 0, (size_t)n * sizeof(int32_t)); return PP_OK; }
    return fetch_behind_advance(h, flags, h->rollout.d_flags, (size_t)n * sizeof(int32_t), false);
}

// Rollout scorecard.  Scored ticks are streamed ticks: k_score_ego hangs on the tick's front-chain event.
int pp_score_begin(pp_handle h, double dt_score)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!(dt_score > 0) || !std::isfinite(dt_score)) return fail(PP_ERR_ARG, "pp_score_begin: dt_score must be finite and > 0");
    HIP_TRY(hipSetDevice(h->device));
    PP_TRY(flush_group(h));
    PP_TRY(ensure_streaming(h));
    if (!h->score.d_score) {
        const size_t ns = (size_t)h->caps.max_scenes;
        PP_TRY(h->score.d_score.reserve(ns));
        for (int q = 0; q < kBuf; q++) PP_TRY(h->score.d_grid[q].reserve(ns));
    }
    if (h->elog.on) PP_TRY(h->elog.d_score.reserve((size_t)h->caps.max_scenes));      // the episode log gets its scorecards once scoring comes on (§4n)
    PP_TRY(join_all(h));                                 // the ticks scored so far (a restart) and everything before
    if (h->elog.on) PP_TRY(h->rollout.adv.wait(h->stream));      // (... and a staged advance: k_log_episodes writes the scorecards of the episodes it ended)
    PP_TRY(reset_scores(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->score.on = true; h->score.dt = dt_score;
    return features_ok(h, "pp_score_begin");
}

int pp_score_end(pp_handle h)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    h->score.on = false;
    return features_ok(h, "pp_score_end");
}

int pp_get_rollout_score(pp_handle h, RolloutScore* out, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->score.d_score) return fail(PP_ERR_STATE, "pp_get_rollout_score: pp_score_begin was never called on this handle");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    HIP_TRY(hipSetDevice(h->device));
    { int r = join_all(h); if (r) return r; }            // behind both halves: score.ego (k_score_ego), scored[] / stream order (k_score_grid)
    if (h->episode.on) PP_TRY(h->rollout.adv.wait(h->stream));      // (episodes: a staged advance may have moved last_pos / last_speed to a start record)
    std::vector<dmpp::ScoreGridPart> parts((size_t)kBuf * (size_t)std::max(n, 1));
    HIP_TRY(hipMemcpyAsync(out, h->score.d_score, (size_t)n * sizeof(RolloutScore), hipMemcpyDefault, h->stream));
    for (int q = 0; q < kBuf && n > 0; q++)
        HIP_TRY(hipMemcpyAsync(parts.data() + (size_t)q * n, h->score.d_grid[q], (size_t)n * sizeof(dmpp::ScoreGridPart), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int q = 0; q < kBuf; q++)                       // the grid half: one part per search set, added here
        for (int s = 0; s < n; s++) {
            const dmpp::ScoreGridPart& p = parts[(size_t)q * n + s];
            out[s].n_grid_ticks += p.n_grid_ticks; out[s].n_grid_path_candidate += p.n_grid_path_candidate;
            for (int k = 0; k < DMPP_G_STATUS_COUNT; k++) out[s].grid_status_ticks[k] += p.status[k];
        }
    return PP_OK;
}

// Score trace.  Everything is checked on the host before anything changes.
void pp_default_score_trace(ScoreTraceModel* m)
{
    if (!m) return;
    m->depth = 64; m->post = 8; m->trigger = DMPP_TRACE_COLLISION; m->flag_mask = 0; m->near = 0.5; m->brake = 6.0;
}

int pp_set_score_trace(pp_handle h, const ScoreTraceModel* m)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!m) { h->strace.on = false; return PP_OK; }      // (what was recorded stays readable)
    if (m->depth < 1 || m->depth > DMPP_SCORE_TRACE_MAX) return fail(PP_ERR_ARG, "pp_set_score_trace: depth must be 1 .. DMPP_SCORE_TRACE_MAX");
    if (m->post < 0 || m->post > m->depth - 1) return fail(PP_ERR_ARG, "pp_set_score_trace: post must be 0 .. depth - 1");
    if ((m->trigger & ~15) != 0) return fail(PP_ERR_ARG, "pp_set_score_trace: trigger holds bits outside the four DMPP_TRACE_* causes (15)");
    if ((m->flag_mask & ~31) != 0) return fail(PP_ERR_ARG, "pp_set_score_trace: flag_mask holds bits outside the five DMPP_EGO_* flags (31)");
    if (!std::isfinite(m->near)) return fail(PP_ERR_ARG, "pp_set_score_trace: near must be finite");
    if (!std::isfinite(m->brake) || !(m->brake > 0)) return fail(PP_ERR_ARG, "pp_set_score_trace: brake must be finite and > 0");
    PP_TRY(quiesce(h, false));                            // every scored tick so far is in front of the handle's stream
    const size_t ns = (size_t)h->caps.max_scenes;         // room first, the headers (allocated once) in front of the ring: a failed allocation changes nothing in force
    PP_TRY(h->strace.d_info.reserve(ns)); PP_TRY(h->strace.d_ring.reserve(ns * (size_t)m->depth));
    PP_TRY(reset_score_trace(h));
    HIP_TRY(hipStreamSynchronize(h->stream));            // the one host wait: the upload stream reads all of it from its next launch on
    h->strace.tm = *m; h->strace.on = true; h->strace.ever = true;
    return PP_OK;
}

// the headers behind every scored tick, waiting as pp_get_rollout_score does (host wait)
static int fetch_trace_info(pp_handle h, ScoreTraceInfo* out, int first, int n)
{
    HIP_TRY(hipSetDevice(h->device));
    PP_TRY(join_all(h));
    if (h->episode.on) PP_TRY(h->rollout.adv.wait(h->stream));
    HIP_TRY(hipMemcpyAsync(out, h->strace.d_info + first, (size_t)n * sizeof(ScoreTraceInfo), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

int pp_get_score_trace_info(pp_handle h, ScoreTraceInfo* out, int n_scenes)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->strace.ever) return fail(PP_ERR_STATE, "pp_get_score_trace_info: pp_set_score_trace was never called on this handle");
    if (n_scenes < 0 || n_scenes > h->n_scenes) return fail(PP_ERR_ARG, "n_scenes exceeds the resident scenes");
    if (n_scenes == 0) return PP_OK;
    return fetch_trace_info(h, out, 0, n_scenes);
}

int pp_read_score_trace(pp_handle h, int scene, ScoreTick* out, int cap, ScoreTraceInfo* info, int rearm)
{
    if (!h || cap < 0 || (!out && cap > 0)) return fail(PP_ERR_ARG, "pp_read_score_trace: null argument or negative count");
    if (!h->strace.ever) return fail(PP_ERR_STATE, "pp_read_score_trace: pp_set_score_trace was never called on this handle");
    if (scene < 0 || scene >= h->n_scenes) return fail(PP_ERR_ARG, "pp_read_score_trace: no such resident scene");
    ScoreTraceInfo hd;
    PP_TRY(fetch_trace_info(h, &hd, scene, 1));
    const long long depth = h->strace.tm.depth, written = (long long)(uint32_t)hd.n_written, n = std::min(written, depth);      // (unsigned, as the kernel's slot)
    if (n > (long long)cap) return fail(PP_ERR_CAPACITY, "pp_read_score_trace: the ring holds " + std::to_string(n) + " records, cap is " + std::to_string(cap));
    const ScoreTick* ring = h->strace.d_ring + (size_t)scene * (size_t)depth;
    const long long i0 = (written - n) % depth, n0 = std::min(n, depth - i0);      // the run up to the end of the ring, then the run from its start
    if (n0 > 0) HIP_TRY(hipMemcpyAsync(out, ring + i0, (size_t)n0 * sizeof(ScoreTick), hipMemcpyDeviceToHost, h->stream));
    if (n > n0) HIP_TRY(hipMemcpyAsync(out + n0, ring, (size_t)(n - n0) * sizeof(ScoreTick), hipMemcpyDeviceToHost, h->stream));
    if (info) *info = hd;                                 // (the header the records were read under: before a rearm)
    if (rearm) {      // armed again; the ring and n_written stay, so the next incident keeps its lead-in.  Pageable source: the copy has left `hd` on return
        hd.state = 0; hd.trigger_k = -1; hd.trigger = 0; hd.post_left = 0;
        HIP_TRY(hipMemcpyAsync(h->strace.d_info + scene, &hd, sizeof(ScoreTraceInfo), hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return (int)n;
}

// Conflict score.  Everything is checked on the host before anything changes.
void pp_default_conflict(ConflictModel* m)
{
    if (!m) return;
    m->ttc_warn = 3.0; m->ttc_crit = 1.5; m->v_max = 70.0; m->min_closing = 0.0;
}

int pp_set_conflict_score(pp_handle h, const ConflictModel* m)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!m) { h->conflict.on = false; return PP_OK; }    // (the records stay readable)
    if (!std::isfinite(m->ttc_warn) || !(m->ttc_warn > 0)) return fail(PP_ERR_ARG, "pp_set_conflict_score: ttc_warn must be finite and > 0");
    if (!std::isfinite(m->ttc_crit) || !(m->ttc_crit > 0) || !(m->ttc_crit <= m->ttc_warn)) return fail(PP_ERR_ARG, "pp_set_conflict_score: ttc_crit must be finite, > 0 and <= ttc_warn");
    if (!std::isfinite(m->v_max) || !(m->v_max > 0)) return fail(PP_ERR_ARG, "pp_set_conflict_score: v_max must be finite and > 0");
    if (!std::isfinite(m->min_closing) || !(m->min_closing >= 0)) return fail(PP_ERR_ARG, "pp_set_conflict_score: min_closing must be finite and >= 0");
    PP_TRY(quiesce(h, false));                            // every scored tick so far is in front of the handle's stream
    const size_t ns = (size_t)h->caps.max_scenes, no = (size_t)std::max(h->caps.max_obs_total, 1);      // room first: a failed allocation changes nothing in force
    PP_TRY(h->conflict.d_score.reserve(ns)); PP_TRY(h->conflict.d_prev[0].reserve(no)); PP_TRY(h->conflict.d_prev[1].reserve(no));
    PP_TRY(reset_conflict(h));
    HIP_TRY(hipStreamSynchronize(h->stream));            // the one host wait: the upload stream reads all of it from its next launch on
    h->conflict.cm = *m; h->conflict.on = true; h->conflict.ever = true;
    return PP_OK;
}

int pp_get_conflict_score(pp_handle h, ConflictScore* out, int n_scenes)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->conflict.ever) return fail(PP_ERR_STATE, "pp_get_conflict_score: pp_set_conflict_score was never called on this handle");
    if (n_scenes < 0 || n_scenes > h->n_scenes) return fail(PP_ERR_ARG, "n_scenes exceeds the resident scenes");
    if (n_scenes == 0) return PP_OK;
    HIP_TRY(hipSetDevice(h->device));
    PP_TRY(join_all(h));                                  // behind score.ego, as pp_get_rollout_score
    if (h->episode.on) PP_TRY(h->rollout.adv.wait(h->stream));
    HIP_TRY(hipMemcpyAsync(out, h->conflict.d_score, (size_t)n_scenes * sizeof(ConflictScore), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

// Perception model.  Everything is checked on the host before anything changes.
void pp_default_perception(PerceptionModel* m)
{
    if (!m) return;
    m->range = 60.0; m->cos_half_fov = 0.5; m->sigma0 = 0.1; m->sigma_gain = 0.005;      // (cos 60 deg; a starting point, not tuned values)
    m->p_miss = 85899346u; m->seed = 1u; m->occlusion = 1; m->confirm = 2; m->coast = 3; m->_pad = 0;      // p_miss: 2 % of 2^32
}

static const char* check_perception(const PerceptionModel* m)
{
    if (!(m->range > 0)) return "range must be > 0 (+inf is allowed)";
    if (!(m->cos_half_fov >= -1.0 && m->cos_half_fov <= 1.0)) return "cos_half_fov must lie in [-1, 1]";
    if (!std::isfinite(m->sigma0) || !(m->sigma0 >= 0)) return "sigma0 must be finite and >= 0";
    if (!std::isfinite(m->sigma_gain) || !(m->sigma_gain >= 0)) return "sigma_gain must be finite and >= 0";
    if (m->occlusion != 0 && m->occlusion != 1) return "occlusion must be 0 or 1";
    if (m->confirm < 0 || m->confirm > 255) return "confirm must lie in 0 .. 255";
    if (m->coast < 0 || m->coast > 255) return "coast must lie in 0 .. 255";
    if (m->_pad != 0) return "_pad must be 0";
    return nullptr;
}

int pp_set_perception(pp_handle h, const PerceptionModel* m)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (m) if (const char* why = check_perception(m)) return fail(PP_ERR_ARG, std::string("pp_set_perception: ") + why);
    // (no refuse_if_staged: the call reads nothing of the resident set - tracks follow pool entries of whatever set a tick reads - so an
    // update or an advance staged for the next tick stays staged, and that tick is the first one perceived)
    PP_TRY(quiesce(h, false));                           // every tick so far is in front of the handle's stream (an open group is launched with the old setting)
    if (!m) { h->percept.on = false; return PP_OK; }      // (tracks and stats stay readable)
    PerceptionState& P = h->percept;
    const size_t obs_stride = (size_t)std::max(h->caps.max_obs_total, 1);      // room first: a failed allocation changes nothing in force
    for (int q = 0; q < kObs; q += kGroupMax) {
        PP_TRY(P.seen_mem[q / kGroupMax].reserve(h->gcap * obs_stride));
        for (int i = 0; i < h->gcap; i++) P.d_seen[q + i] = P.seen_mem[q / kGroupMax] + i * obs_stride;
    }
    PP_TRY(P.d_track.reserve(obs_stride)); PP_TRY(P.d_stats.reserve((size_t)h->caps.max_scenes));
    // the perceived ring starts as a copy of the truth ring: until the first perceived tick pp_get_grid and PP_BUF_OBS_SEEN show
    // what the last tick's search rasterised, never memory nobody wrote
    for (int q = 0; q < kRing; q++)
        HIP_TRY(hipMemcpyAsync(P.seen_mem[q].get(), h->obs_now_mem[q].get(), h->gcap * obs_stride * sizeof(ObPoint), hipMemcpyDeviceToDevice, h->stream));
    PP_TRY(reset_perception(h));
    HIP_TRY(hipStreamSynchronize(h->stream));            // the one host wait: the front chain of the next tick may start on another stream
    P.pm = *m; P.on = true; P.ever = true;
    return PP_OK;
}

// (k_perceive runs on the front chain: behind join_all)
int pp_get_perception_stats(pp_handle h, PerceptionStats* out, int n_scenes)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->percept.ever) return fail(PP_ERR_STATE, "pp_get_perception_stats: pp_set_perception was never called on this handle");
    if (n_scenes < 0 || n_scenes > h->n_scenes) return fail(PP_ERR_ARG, "n_scenes exceeds the resident scenes");
    if (n_scenes == 0) return PP_OK;
    return fetch(h, out, h->percept.d_stats, (size_t)n_scenes * sizeof(PerceptionStats));
}

int pp_get_perception_tracks(pp_handle h, PerceptTrack* out, int first, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->percept.ever) return fail(PP_ERR_STATE, "pp_get_perception_tracks: pp_set_perception was never called on this handle");
    if (first < 0 || n < 0 || (long long)first + n > (long long)h->caps.max_obs_total) return fail(PP_ERR_ARG, "pp_get_perception_tracks: the range lies outside the obstacle pool (caps.max_obs_total)");
    if (n == 0) return PP_OK;
    return fetch(h, out, h->percept.d_track + first, (size_t)n * sizeof(PerceptTrack));
}

// Every resident scene's OWN obstacle entries (obs_off, obs_n): of the resident records, or - fleet on - the ones pinned then
// (obs_n counts the peers now).  Behind join_all; waits on the host.  *rc: PP_OK, or the error (the vector is empty then).
static std::vector<dmpp::FleetPin> own_slices(pp_handle h, int* rc)
{
    *rc = PP_OK;
    if (h->fleet.on) return h->fleet.pin;
    const size_t n = (size_t)h->n_scenes;
    std::vector<SceneIn> rec(n);
    hipError_t e = hipMemcpyAsync(rec.data(), h->cur_in().d_in, n * sizeof(SceneIn), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { *rc = fail(PP_ERR_HIP, std::string("reading the resident SceneIn records: ") + hipGetErrorString(e)); return {}; }
    std::vector<dmpp::FleetPin> pin(n);
    for (size_t s = 0; s < n; s++) { pin[s].obs_off = rec[s].obs_off; pin[s].n_own = rec[s].obs_n; }
    return pin;
}

// Fleet coupling.  Everything is checked on the host before anything changes.
int pp_set_fleet(pp_handle h, int n_worlds, const int32_t* world_first, const FleetModel* fm)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (n_worlds < 0) return fail(PP_ERR_ARG, "pp_set_fleet: negative world count");
    PP_TRY(refuse_if_staged(h, "pp_set_fleet", "the fleet"));
    const int n = h->n_scenes;
    if (n_worlds == 0) {
        if (!h->fleet.on) return PP_OK;
        PP_TRY(quiesce(h, false));
        hipLaunchKernelGGL(dmpp::k_fleet_restore, dim3((unsigned)((n + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream, n, h->fleet.d_pin, h->cur_in().d_in);
        HIP_TRY(hipGetLastError());
        PP_TRY(reset_perception(h));   // the slices move (§4w)
        HIP_TRY(hipStreamSynchronize(h->stream));
        // (the slices are the pinned ones again; they were inside fleet.base when they were pinned)
        const int back = std::max(h->fleet.base, h->fleet.own_end);
        h->fleet.on = false; h->cur_in().n_obs_total = back;
        retire(h, dmpp::kSetFleet);                       // (the worlds that world traffic was pinned to are gone: §4j)
        return features_ok(h, "pp_set_fleet");
    }
    if (!world_first || !fm) return fail(PP_ERR_ARG, "null argument");
    if (n <= 0) return fail(PP_ERR_STATE, "pp_set_fleet: no resident scenes");
    const int K = fm->max_peers;
    if (K < 0 || K > DMPP_FLEET_MAX_PEERS) return fail(PP_ERR_ARG, "pp_set_fleet: max_peers must be 0 .. " + std::to_string(DMPP_FLEET_MAX_PEERS));
    if (!std::isfinite(fm->range) || !(fm->range > 0) || !std::isfinite(fm->radius) || !(fm->radius >= 0))
        return fail(PP_ERR_ARG, "pp_set_fleet: range must be finite and > 0, radius finite and >= 0");
    if (n_worlds > n || world_first[0] != 0 || world_first[n_worlds] != n) return fail(PP_ERR_ARG, "pp_set_fleet: world_first must run from 0 to the resident scene count");
    for (int w = 0; w < n_worlds; w++) if (world_first[w + 1] <= world_first[w]) return fail(PP_ERR_ARG, "pp_set_fleet: world_first must be strictly increasing");
    PP_TRY(quiesce(h, false));
    int rc;
    std::vector<dmpp::FleetPin> pin = own_slices(h, &rc); if (rc) return rc;
    const int base = h->fleet.on ? h->fleet.base : h->cur_in().n_obs_total;
    std::vector<std::pair<long long, long long>> ext;       // non-empty extended slices [off, off + n_own + K)
    long long end_max = base, own_end = 0;
    for (int s = 0; s < n; s++) {
        const long long off = pin[(size_t)s].obs_off, len = (long long)pin[(size_t)s].n_own + K;
        if (pin[(size_t)s].n_own < 0) return fail(PP_ERR_ARG, "pp_set_fleet: scene " + std::to_string(s) + " has a negative obs_n");
        if (pin[(size_t)s].n_own > 0) own_end = std::max(own_end, off + pin[(size_t)s].n_own);
        if (len == 0) continue;
        if (off < 0) return fail(PP_ERR_ARG, "pp_set_fleet: scene " + std::to_string(s) + " has a negative obs_off");
        if (off + len > (long long)h->caps.max_obs_total)
            return fail(PP_ERR_CAPACITY, "pp_set_fleet: the obstacle slice of scene " + std::to_string(s) + " with its peer slots ends beyond caps.max_obs_total");
        ext.emplace_back(off, off + len);
        end_max = std::max(end_max, off + len);
    }
    std::sort(ext.begin(), ext.end());
    for (size_t k = 1; k < ext.size(); k++)
        if (ext[k].first < ext[k - 1].second) return fail(PP_ERR_ARG, "pp_set_fleet: two scenes' obstacle slices overlap once the peer slots are added (leave max_peers free entries behind every slice)");
    std::vector<int32_t> world_of((size_t)n);
    for (int w = 0; w < n_worlds; w++) for (int s = world_first[w]; s < world_first[w + 1]; s++) world_of[(size_t)s] = w;
    const size_t ns = (size_t)h->caps.max_scenes;
    if ((rc = h->fleet.d_world_first.reserve(ns + 1)) || (rc = h->fleet.d_world_of.reserve(ns)) || (rc = h->fleet.d_pin.reserve(ns))) return rc;
    HIP_TRY(hipMemcpyAsync(h->fleet.d_world_first, world_first, ((size_t)n_worlds + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->fleet.d_world_of, world_of.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->fleet.d_pin, pin.data(), (size_t)n * sizeof(dmpp::FleetPin), hipMemcpyHostToDevice, h->stream));
    h->fleet.pin.swap(pin); h->fleet.fm = *fm; h->fleet.base = base; h->fleet.end = (int)end_max; h->fleet.own_end = (int)std::min(own_end, (long long)h->caps.max_obs_total); h->fleet.on = true;
    h->fleet.n_worlds = n_worlds;
    retire(h, dmpp::kSetFleet);                           // world traffic was pinned to the worlds this call replaces (§4j)
    h->cur_in().n_obs_total = (int)end_max;
    couple_fleet(h, h->stream, h->cur_in().d_in, h->cur_in().d_obs, h->cur_in().mot());      // the resident set: the next tick sees the peers
    HIP_TRY(hipGetLastError());
    PP_TRY(reset_perception(h));      // the slices grow by their peer slots (§4w)
    HIP_TRY(hipStreamSynchronize(h->stream));            // (the host arrays above go out of scope)
    return features_ok(h, "pp_set_fleet");
}

// Lane traffic.  Everything is checked on the host before anything changes; the cumulative lengths are computed
// here, in order (+, * and sqrt round as on the device), and uploaded.  world: pp_set_world_traffic - an actor's
// `scene` is a world of the fleet in force and its slot an own entry of EVERY member scene of that world.
static int set_traffic(pp_handle h, bool world, int n_tracks, const TrafficTrack* tracks, const GlobalPoint2D* points, int n_points, int n_actors, const TrafficActor* actors)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    const std::string fn = world ? "pp_set_world_traffic" : "pp_set_traffic";
    if (n_tracks < 0 || n_points < 0 || n_actors < 0) return fail(PP_ERR_ARG, fn + ": negative count");
    PP_TRY(refuse_if_staged(h, fn, "the traffic"));
    if (n_actors == 0) {
        retire(h, dmpp::kTrafficOff);
        if (h->percept.d_stats) {                         // the vehicles leave their slots: tracks and stats of the perception model start again (§4w)
            PP_TRY(quiesce(h, false)); PP_TRY(reset_perception(h)); HIP_TRY(hipStreamSynchronize(h->stream));
        }
        return features_ok(h, fn.c_str());
    }
    const int n = h->n_scenes;
    if (n <= 0) return fail(PP_ERR_STATE, fn + ": no resident scenes");
    if (world && !h->fleet.on) return fail(PP_ERR_STATE, fn + ": no fleet is set (the worlds are those of pp_set_fleet; max_peers = 0 is a legal fleet)");
    if (!tracks || !points || !actors || n_tracks == 0) return fail(PP_ERR_ARG, fn + ": actors need tracks and points");
    // tracks: compact copies of their points, and the cumulative lengths (closed: one more segment, back to the first point)
    std::vector<dmpp::TrafficTrackDev> tdev((size_t)n_tracks);
    std::vector<GlobalPoint2D> pts; std::vector<double> cum;
    for (int k = 0; k < n_tracks; k++) {
        const TrafficTrack& T = tracks[k];
        const std::string who = fn + ": track " + std::to_string(k);
        if (T.n_points < 2) return fail(PP_ERR_ARG, who + " has fewer than 2 points");
        if (T.point_off < 0 || (long long)T.point_off + T.n_points > (long long)n_points) return fail(PP_ERR_ARG, who + " lies outside the point array");
        if (pts.size() + (size_t)T.n_points > (size_t)INT32_MAX / 2) return fail(PP_ERR_ARG, fn + ": more than 2^30 track points");
        const GlobalPoint2D* P = points + T.point_off;
        for (int i = 0; i < T.n_points; i++)
            if (!std::isfinite(P[i].x) || !std::isfinite(P[i].y)) return fail(PP_ERR_ARG, who + " has a non-finite point");
        const bool closed = T.closed != 0;
        const int nseg = closed ? T.n_points : T.n_points - 1;
        tdev[(size_t)k] = { (int32_t)pts.size(), T.n_points, closed ? 1 : 0, (int32_t)cum.size() };
        pts.insert(pts.end(), P, P + T.n_points);
        double c = 0; cum.push_back(c);
        for (int i = 0; i < nseg; i++) {
            const GlobalPoint2D& A = P[i]; const GlobalPoint2D& B = P[i + 1 < T.n_points ? i + 1 : 0];
            const double dx = B.x - A.x, dy = B.y - A.y;
            const double xx = dx * dx, yy = dy * dy;      // (separate statements: no contraction, whatever the compiler flags)
            c = c + std::sqrt(xx + yy); cum.push_back(c);
        }
        if (closed && !(c > 0)) return fail(PP_ERR_ARG, who + " is closed and has no length");
    }
    PP_TRY(quiesce(h, false));                            // nobody reads the old arrays from here on; the host wait follows the checks
    int rc;
    const std::vector<dmpp::FleetPin> own = own_slices(h, &rc); if (rc) return rc;
    std::vector<dmpp::TrafficPin> pin((size_t)n_actors); std::vector<double> s0((size_t)n_actors); std::vector<long long> taken((size_t)n_actors);
    std::vector<int32_t> scene_of((size_t)n_actors), track_of((size_t)n_actors);
    std::vector<int32_t> world_first;                     // world: the fleet's, read back (the host keeps no copy of it)
    if (world) {
        world_first.resize((size_t)h->fleet.n_worlds + 1);
        HIP_TRY(hipMemcpyAsync(world_first.data(), h->fleet.d_world_first, world_first.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    long long end_max = 0;
    for (int a = 0; a < n_actors; a++) {
        const TrafficActor& A = actors[a];
        const std::string who = fn + ": actor " + std::to_string(a);
        if (!std::isfinite(A.s0) || !std::isfinite(A.speed)) return fail(PP_ERR_ARG, who + " has a non-finite s0 or speed");
        if (!std::isfinite(A.radius) || !(A.radius >= 0)) return fail(PP_ERR_ARG, who + ": radius must be finite and >= 0");
        if (world && (A.scene < 0 || A.scene >= h->fleet.n_worlds)) return fail(PP_ERR_ARG, who + " names a world that the fleet does not have");
        if (!world && (A.scene < 0 || A.scene >= n)) return fail(PP_ERR_ARG, who + " names a scene that is not resident");
        if (A.track < 0 || A.track >= n_tracks) return fail(PP_ERR_ARG, who + " names a track that was not given");
        // the slot must be an own entry of the scene or, per world, of every member scene; the pin keeps the entry or the slot
        const int m0 = world ? world_first[(size_t)A.scene] : A.scene, m1 = world ? world_first[(size_t)A.scene + 1] : A.scene + 1;
        long long pool = 0;
        for (int m = m0; m < m1; m++) {
            const dmpp::FleetPin& O = own[(size_t)m];
            pool = (long long)O.obs_off + A.slot;
            if (A.slot < 0 || A.slot >= O.n_own || O.obs_off < 0 || pool >= (long long)h->caps.max_obs_total)
                return fail(PP_ERR_ARG, who + ": slot " + std::to_string(A.slot) + " is not one of the " + std::to_string(std::max(O.n_own, 0)) + " own obstacle entries of scene " + std::to_string(m) +
                                        (world ? " (world " + std::to_string(A.scene) + ")" : ""));
            end_max = std::max(end_max, pool + 1);
        }
        pin[(size_t)a] = { A.speed, world ? A.slot : (int32_t)pool, A.track, A.type, A.radius };
        scene_of[(size_t)a] = A.scene; track_of[(size_t)a] = A.track;
        s0[(size_t)a] = A.s0; taken[(size_t)a] = ((long long)A.scene << 32) | (long long)A.slot;
    }
    std::sort(taken.begin(), taken.end());
    for (size_t k = 1; k < taken.size(); k++)
        if (taken[k] == taken[k - 1]) return fail(PP_ERR_ARG, fn + ": two actors on slot " + std::to_string((int)(taken[k] & 0xffffffff)) + (world ? " of world " : " of scene ") + std::to_string((int)(taken[k] >> 32)));
    HIP_TRY(hipStreamSynchronize(h->stream));
    // room first.  An allocation that fails leaves its own array as it was, but may follow one that replaced another: the old
    // traffic then goes off rather than run on half a set
    retire(h, world ? dmpp::kSetWorldTraffic : dmpp::kSetTraffic);      // (the start states of §4m were captured from the actors this call replaces)
    if ((rc = h->traffic.d_pin.reserve((size_t)n_actors)) || (rc = h->traffic.d_s[0].reserve((size_t)n_actors)) || (rc = h->traffic.d_tracks.reserve((size_t)n_tracks)) ||
        (rc = h->traffic.d_cum.reserve(cum.size())) || (rc = h->traffic.d_pts.reserve(pts.size())) ||
        (world && (rc = h->traffic.d_world.reserve((size_t)n_actors)))) { h->traffic.on = false; drop_manoeuvres(h); return rc; }
    drop_manoeuvres(h);                                   // (a set that replaces world traffic retires no per-scene bit: §4v's list goes here)
    h->traffic.on = false;                                // (until everything below has landed: a device error leaves traffic off, never half a set)
    HIP_TRY(hipMemcpyAsync(h->traffic.d_pin, pin.data(), (size_t)n_actors * sizeof(dmpp::TrafficPin), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->traffic.d_s[0], s0.data(), (size_t)n_actors * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->traffic.d_tracks, tdev.data(), (size_t)n_tracks * sizeof(dmpp::TrafficTrackDev), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->traffic.d_cum, cum.data(), cum.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->traffic.d_pts, pts.data(), pts.size() * sizeof(GlobalPoint2D), hipMemcpyHostToDevice, h->stream));
    if (world) HIP_TRY(hipMemcpyAsync(h->traffic.d_world, scene_of.data(), (size_t)n_actors * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    h->traffic.actors = n_actors; h->traffic.end = (int)end_max; h->traffic.cur = 0; h->traffic.world = world; h->traffic.n_tracks = n_tracks;
    h->traffic.scene_of.swap(scene_of); h->traffic.track_of.swap(track_of);
    move_traffic(h, h->stream, h->cur_in().d_obs, h->cur_in().mot(), 0.0);      // s = wrap(s0), and the resident set: the next tick sees the traffic
    HIP_TRY(hipGetLastError());
    PP_TRY(reset_perception(h));      // other vehicles own the slots from here on (§4w)
    HIP_TRY(hipStreamSynchronize(h->stream));            // (the host arrays above go out of scope)
    if (h->follow.on) PP_TRY(build_follow(h));           // following is on: its tables for these actors, v = speed (§4i)
    h->traffic.on = true;
    return features_ok(h, fn.c_str());
}

int pp_set_traffic(pp_handle h, int n_tracks, const TrafficTrack* tracks, const GlobalPoint2D* points, int n_points, int n_actors, const TrafficActor* actors)
{ return set_traffic(h, false, n_tracks, tracks, points, n_points, n_actors, actors); }
// World traffic: the same records, read per world of the fleet in force; replaces whatever traffic the handle had.
int pp_set_world_traffic(pp_handle h, int n_tracks, const TrafficTrack* tracks, const GlobalPoint2D* points, int n_points, int n_actors, const TrafficActor* actors)
{ return set_traffic(h, true, n_tracks, tracks, points, n_points, n_actors, actors); }

int pp_get_traffic_state(pp_handle h, double* s, int n)
{
    if (!h || (!s && n > 0)) return fail(PP_ERR_ARG, "null argument");
    if (!h->traffic.on) return fail(PP_ERR_STATE, "pp_get_traffic_state: no traffic is set");
    if (n < 0 || n > h->traffic.actors) return fail(PP_ERR_ARG, "n exceeds the actors");
    if (n == 0) return PP_OK;
    return fetch_behind_advance(h, s, h->traffic.d_s[h->traffic.cur], (size_t)n * sizeof(double), true);
}

// Car-following traffic: host checks first; the model is a kernel argument of the next advance.
void pp_default_traffic_follow(TrafficFollow* tf)
{
    if (!tf) return;
    tf->look = 60.0; tf->lateral = 1.5; tf->gap = 2.0; tf->headway = 1.5; tf->max_acc = 1.0; tf->comfort_dec = 2.0; tf->max_dec = 6.0; tf->min_net = 0.1;
}

int pp_set_traffic_follow(pp_handle h, const TrafficFollow* tf)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (tf) {
        const double f[8] = { tf->look, tf->lateral, tf->gap, tf->headway, tf->max_acc, tf->comfort_dec, tf->max_dec, tf->min_net };
        for (double x : f) if (!std::isfinite(x)) return fail(PP_ERR_ARG, "pp_set_traffic_follow: every field must be finite");
        if (!(tf->look > 0) || !(tf->gap > 0) || !(tf->max_acc > 0) || !(tf->comfort_dec > 0) || !(tf->max_dec > 0) || !(tf->min_net > 0))
            return fail(PP_ERR_ARG, "pp_set_traffic_follow: look, gap, max_acc, comfort_dec, max_dec and min_net must be > 0");
        if (tf->lateral < 0 || tf->headway < 0) return fail(PP_ERR_ARG, "pp_set_traffic_follow: lateral and headway must be >= 0");
    }
    PP_TRY(refuse_if_staged(h, "pp_set_traffic_follow", "the model"));
    retire(h, dmpp::kSetFollow);                          // (nothing below refuses: the start states of §4m were captured under the model this call replaces)
    if (!h->traffic.on) {                                 // takes effect with the next pp_set_traffic
        h->follow.on = tf != nullptr; if (tf) h->follow.tf = *tf;
        return features_ok(h, "pp_set_traffic_follow");
    }
    PP_TRY(quiesce(h, true));                             // nobody reads the arrays
    if (!tf) {                                            // off: the arc lengths go back to the one array of §4h
        if (h->man.on) { h->follow.on = false; return features_ok(h, "pp_set_traffic_follow"); }      // (§4v keeps both sets of s and its states: cur stays)
        if (h->follow.on && h->traffic.cur == 1) {
            HIP_TRY(hipMemcpyAsync(h->traffic.d_s[0], h->traffic.d_s[1], (size_t)h->traffic.actors * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        h->traffic.cur = 0; h->follow.on = false;
        return features_ok(h, "pp_set_traffic_follow");
    }
    PP_TRY(build_follow(h));                              // (a failed allocation or copy leaves the model that was set, or none)
    if (h->man.on) {                                      // §4v: the states stay, v = v0 - the desired speed a manoeuvre may have changed
        static_assert(offsetof(TrafficManoeuvreState, v0) == 16, "the desired speeds are copied out of the states at their stride");
        HIP_TRY(hipMemcpy2DAsync(h->follow.d_v[h->traffic.cur], sizeof(double), &h->man.d_state[h->traffic.cur].get()->v0, sizeof(TrafficManoeuvreState), sizeof(double),
                                 (size_t)h->traffic.actors, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->follow.tf = *tf; h->follow.on = true;
    return features_ok(h, "pp_set_traffic_follow");
}

int pp_get_traffic_speed(pp_handle h, double* v, int n)
{
    if (!h || (!v && n > 0)) return fail(PP_ERR_ARG, "null argument");
    if (!h->traffic.on || !h->follow.on) return fail(PP_ERR_STATE, "pp_get_traffic_speed: traffic or following is off");
    if (n < 0 || n > h->traffic.actors) return fail(PP_ERR_ARG, "n exceeds the actors");
    if (n == 0) return PP_OK;
    return fetch_behind_advance(h, v, h->follow.d_v[h->traffic.cur], (size_t)n * sizeof(double), true);
}

// Traffic manoeuvres.  The list is checked on the host, by the function any caller may use without a handle.
static const char* manoeuvre_fault(int n_actors, int n_tracks, const TrafficManoeuvre& M, int prev_actor, int run)
{
    if (M.actor < 0 || M.actor >= n_actors) return "names an actor that the traffic does not have";
    if (M.actor < prev_actor) return "is out of order (the records of an actor are contiguous, the actors non-decreasing)";
    if (run >= DMPP_MANOEUVRE_MAX) return "is more than DMPP_MANOEUVRE_MAX records for one actor";
    if (M.track < -1 || M.track >= n_tracks) return "names a track that was not given";
    const int kind = M.trigger & 255, side = M.trigger >> 8;
    if (M.trigger < 0 || kind > DMPP_TRIG_EGO_TIME) return "has an unknown trigger kind";
    if (side > 2 || (side != 0 && kind == DMPP_TRIG_ADVANCES)) return "has an unknown side (sides 1 and 2 belong to the EGO kinds)";
    if (kind == DMPP_TRIG_EGO_DIST && !(std::isfinite(M.dist) && M.dist >= 0)) return ": dist must be finite and >= 0";
    if (kind == DMPP_TRIG_EGO_TIME && !(std::isfinite(M.time) && M.time >= 0)) return ": time must be finite and >= 0";
    if (!std::isfinite(M.lat_end)) return "has a non-finite lat_end";
    if (std::isinf(M.speed)) return "has an infinite speed (NaN keeps the speed)";
    if (M.after < 0) return ": after must be >= 0";
    if (M.n_steps < 1 || M.n_steps > 4096) return ": n_steps must be 1 .. 4096";
    if (M._pad != 0) return ": _pad must be 0";
    return nullptr;
}
static int check_manoeuvres(int n_actors, int n_tracks, int n, const TrafficManoeuvre* m, const char** why)
{
    int prev = 0, run = 0;
    for (int i = 0; i < n; i++) {
        if (i > 0 && m[i].actor != prev) run = 0;
        if (const char* f = manoeuvre_fault(n_actors, n_tracks, m[i], i > 0 ? prev : 0, run)) { if (why) *why = f; return i; }
        prev = m[i].actor; run++;
    }
    return -1;
}
int pp_check_traffic_manoeuvres(int n_actors, int n_tracks, int n, const TrafficManoeuvre* m)
{
    if (n == 0) return -1;
    if (n < 0 || !m) return 0;                            // (no list to read: what pp_set_traffic_manoeuvres refuses is not legal here either)
    return check_manoeuvres(n_actors, n_tracks, n, m, nullptr);
}

// The states of every actor as the set call makes them, from the pins and tracks the host keeps
static std::vector<TrafficManoeuvreState> initial_manoeuvre_states(const pp_planner* h, const std::vector<dmpp::TrafficPin>& pin)
{
    std::vector<TrafficManoeuvreState> st(pin.size());
    for (size_t a = 0; a < pin.size(); a++) { st[a] = TrafficManoeuvreState(); st[a].v0 = pin[a].speed; st[a].track = pin[a].track; }
    return st;
}

int pp_set_traffic_manoeuvres(pp_handle h, int n, const TrafficManoeuvre* m)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    const std::string fn = "pp_set_traffic_manoeuvres";
    if (n < 0 || (n > 0 && !m)) return fail(PP_ERR_ARG, fn + ": n records need the records");
    PP_TRY(refuse_if_staged(h, fn, "the manoeuvres"));
    if (!h->traffic.on) return fail(PP_ERR_STATE, fn + ": no traffic is set (pp_set_traffic comes first)");
    if (h->traffic.world) return fail(PP_ERR_STATE, fn + ": world traffic is in force (manoeuvres belong to the actors of pp_set_traffic)");
    if (h->treset.on) return fail(PP_ERR_STATE, fn + ": the episode traffic reset is on (the call comes before pp_set_episode_traffic)");
    const size_t na = (size_t)h->traffic.actors;
    const int n_tracks = (int)h->traffic.n_tracks;
    const char* why = nullptr;
    const int bad = check_manoeuvres((int)na, n_tracks, n, m, &why);
    if (bad >= 0) return fail(PP_ERR_ARG, fn + ": record " + std::to_string(bad) + " " + why);
    if (n == 0 && !h->man.on) return features_ok(h, fn.c_str());
    PP_TRY(quiesce(h, true));                             // nobody reads or writes the arrays
    const int cur = h->traffic.cur;
    std::vector<dmpp::TrafficPin> pin(na);
    HIP_TRY(hipMemcpy(pin.data(), h->traffic.d_pin, na * sizeof(dmpp::TrafficPin), hipMemcpyDeviceToHost));
    std::vector<int32_t> track_now(h->traffic.track_of);
    if (h->man.on) {
        // a list in force ends first: every actor becomes a plain actor of the track it is on, at the speed it wants (the off form).
        // Host copies only, up to here: the pins and track_of are written once the room below is there
        std::vector<TrafficManoeuvreState> was(na);
        HIP_TRY(hipMemcpy(was.data(), h->man.d_state[cur], na * sizeof(TrafficManoeuvreState), hipMemcpyDeviceToHost));
        for (size_t a = 0; a < na; a++) { pin[a].track = was[a].track; pin[a].speed = was[a].v0; track_now[a] = was[a].track; }
    }
    auto plain_actors = [&]() -> int {                    // the off form's write: nothing can be refused behind it
        if (!h->man.on) return PP_OK;
        h->traffic.track_of = track_now;
        HIP_TRY(hipMemcpy(h->traffic.d_pin, pin.data(), na * sizeof(dmpp::TrafficPin), hipMemcpyHostToDevice));
        return PP_OK;
    };
    if (n == 0) {
        PP_TRY(plain_actors());
        if (h->follow.on) {                               // the groups of the tracks the actors are on now; v stays
            std::vector<double> v(na);
            HIP_TRY(hipMemcpy(v.data(), h->follow.d_v[cur], na * sizeof(double), hipMemcpyDeviceToHost));
            PP_TRY(build_follow(h));
            HIP_TRY(hipMemcpy(h->follow.d_v[cur], v.data(), na * sizeof(double), hipMemcpyHostToDevice));
        } else if (cur == 1) {                            // the arc lengths go back to the one array of §4h
            HIP_TRY(hipMemcpy(h->traffic.d_s[0], h->traffic.d_s[1], na * sizeof(double), hipMemcpyDeviceToDevice));
            h->traffic.cur = 0;
        }
        drop_manoeuvres(h);
        return features_ok(h, fn.c_str());
    }
    // the tables: every actor's run of records, every actor's scene, the actors by (scene, index)
    std::vector<int32_t> rec_first(na + 1, 0), members(na), scene_first((size_t)h->n_scenes + 1, 0);
    for (int i = 0; i < n; i++) rec_first[(size_t)m[i].actor + 1]++;
    for (size_t a = 0; a < na; a++) rec_first[a + 1] += rec_first[a];
    const std::vector<int32_t>& sc = h->traffic.scene_of;
    for (size_t a = 0; a < na; a++) scene_first[(size_t)sc[a] + 1]++;
    for (size_t c = 0; c < (size_t)h->n_scenes; c++) scene_first[c + 1] += scene_first[c];
    { std::vector<int32_t> at(scene_first.begin(), scene_first.end() - 1); for (size_t a = 0; a < na; a++) members[(size_t)at[(size_t)sc[a]]++] = (int32_t)a; }
    const std::vector<TrafficManoeuvreState> st = initial_manoeuvre_states(h, pin);
    ManoeuvreState& M = h->man;
    int rc;
    if ((rc = M.d_recs.reserve((size_t)n)) || (rc = M.d_rec_first.reserve(na + 1)) || (rc = M.d_scene_of.reserve(na)) || (rc = M.d_scene_first.reserve(scene_first.size())) ||
        (rc = M.d_members.reserve(na)) || (rc = M.d_state[0].reserve(na)) || (rc = M.d_state[1].reserve(na))) { if (!M.on) M = ManoeuvreState(); return rc; }
    if (!h->traffic.d_s[1] || h->traffic.d_s[1].capacity() < na) {      // the second array of arc lengths (following has it already)
        if (cur == 1) return fail(PP_ERR_STATE, fn + ": internal: the current arc lengths are in an array that does not exist");
        if ((rc = h->traffic.d_s[1].reserve(na))) { if (!M.on) M = ManoeuvreState(); return rc; }
    }
    PP_TRY(plain_actors());                               // room first (above), then the writes
    HIP_TRY(hipMemcpy(M.d_recs, m, (size_t)n * sizeof(TrafficManoeuvre), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(M.d_rec_first, rec_first.data(), rec_first.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(M.d_scene_of, sc.data(), na * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(M.d_scene_first, scene_first.data(), scene_first.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(M.d_members, members.data(), na * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(M.d_state[cur], st.data(), na * sizeof(TrafficManoeuvreState), hipMemcpyHostToDevice));
    const bool was_on = M.on;
    M.on = true;
    if (was_on) {                                         // the offsets of the list that ended are dropped: the resident set carries the plain poses
        PP_TRY(manoeuvre_traffic(h, h->stream, h->cur_in().d_in, h->cur_in().d_obs, h->cur_in().mot(), 0.0));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return features_ok(h, fn.c_str());
}

int pp_get_traffic_manoeuvre_state(pp_handle h, TrafficManoeuvreState* out, int n_actors)
{
    if (!h || (!out && n_actors > 0)) return fail(PP_ERR_ARG, "null argument");
    if (!h->traffic.on || !h->man.on) return fail(PP_ERR_STATE, "pp_get_traffic_manoeuvre_state: no manoeuvres are set");
    if (n_actors < 0 || n_actors > h->traffic.actors) return fail(PP_ERR_ARG, "n_actors exceeds the actors");
    if (n_actors == 0) return PP_OK;
    return fetch_behind_advance(h, out, h->man.d_state[h->traffic.cur], (size_t)n_actors * sizeof(TrafficManoeuvreState), true);      // waits as pp_get_traffic_state does
}

// Route following.  Everything is checked on the host before anything changes; the resident records are not touched.
int pp_default_route_model(RouteModel* rm)
{
    if (!rm) return fail(PP_ERR_ARG, "null argument");
    rm->pre_points = 60; rm->_pad = 0;       // 30 m of 0.5 m points: the PRE_INTER distances of the default configuration
    return PP_OK;
}

int pp_set_route(pp_handle h, int n_legs_total, const RouteLeg* legs, const int32_t* route_first, const RouteModel* rm)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (n_legs_total < 0) return fail(PP_ERR_ARG, "pp_set_route: negative leg count");
    PP_TRY(refuse_if_staged(h, "pp_set_route", "the route"));
    if (n_legs_total == 0) { h->route.on = false; return features_ok(h, "pp_set_route"); }
    const int n = h->n_scenes;
    if (n <= 0) return fail(PP_ERR_STATE, "pp_set_route: no resident scenes");
    if (h->resident_mode != 1 || !h->have_map) return fail(PP_ERR_STATE, "pp_set_route: routes need egos on a resident map (pp_set_map, then pp_set_egos)");
    if (!legs || !route_first || !rm) return fail(PP_ERR_ARG, "null argument");
    if (rm->pre_points < 0) return fail(PP_ERR_ARG, "pp_set_route: pre_points must be >= 0");
    if (route_first[0] != 0 || route_first[n] != n_legs_total) return fail(PP_ERR_ARG, "pp_set_route: route_first must run from 0 to n_legs_total");
    for (int s = 0; s < n; s++) if (route_first[s + 1] < route_first[s]) return fail(PP_ERR_ARG, "pp_set_route: route_first must not decrease");
    for (int k = 0; k < n_legs_total; k++)
        if (legs[k].road_num < 1 || legs[k].road_num > h->map_roads) return fail(PP_ERR_ARG, "pp_set_route: leg " + std::to_string(k) + " names a road outside the map");
    PP_TRY(quiesce(h, true));                             // nobody reads the old legs
    PP_TRY(h->route.d_first.reserve((size_t)h->caps.max_scenes + 1));      // room first: a failed allocation leaves the old route
    PP_TRY(h->route.d_legs.reserve((size_t)n_legs_total));
    h->route.on = false;                                  // (until the copies below have landed: a failed copy leaves routing off, not half a route)
    HIP_TRY(hipMemcpyAsync(h->route.d_legs, legs, (size_t)n_legs_total * sizeof(RouteLeg), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->route.d_first, route_first, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));            // (the caller's arrays may go; the upload stream reads the copies from its next launch on)
    h->route.rm = *rm; h->route.rm._pad = 0; h->route.on = true;
    return features_ok(h, "pp_set_route");
}

// Episodic rollouts.  Everything is checked on the host before anything changes.
void pp_default_episode_model(EpisodeModel* em)
{
    if (!em) return;
    em->end_mask = DMPP_EGO_PATH_END | DMPP_EGO_BAD_PATH | DMPP_EGO_LANE_END | DMPP_EGO_OFF_GRID | DMPP_EGO_ROUTE_END; em->max_ticks = 0;
}

int pp_set_episodes(pp_handle h, const EpisodeModel* em)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    PP_TRY(refuse_if_staged(h, "pp_set_episodes", "the episodes"));
    if (!em) { h->episode.on = false; retire(h, dmpp::kSetEpisodes); return features_ok(h, "pp_set_episodes"); }
    const int n = h->n_scenes;
    if (n <= 0) return fail(PP_ERR_STATE, "pp_set_episodes: no resident scenes");
    if ((em->end_mask & ~31) != 0) return fail(PP_ERR_ARG, "pp_set_episodes: end_mask holds bits outside the five DMPP_EGO_* flags (31)");
    if (em->max_ticks < 0) return fail(PP_ERR_ARG, "pp_set_episodes: max_ticks must be >= 0");
    if (em->end_mask == 0 && em->max_ticks == 0) return fail(PP_ERR_ARG, "pp_set_episodes: a model with no end flag and no timeout ends no episode");
    PP_TRY(quiesce(h, true));                             // nobody reads the old start records
    const size_t ns = (size_t)h->caps.max_scenes;         // room first, sized once: a failed allocation leaves the old records
    PP_TRY(h->episode.d_start_in.reserve(ns)); PP_TRY(h->episode.d_start_state.reserve(ns)); PP_TRY(h->episode.d_stats.reserve(ns));
    h->episode.on = false;                                // (until the copies below have landed: a failed copy leaves episodes off, not half a capture)
    retire(h, dmpp::kSetEpisodes);                        // (record 0 of the spawn model's pool was the old capture, set 0 of the traffic reset went with it, and so did the episodes the log numbered: §4l - §4n)
    HIP_TRY(hipMemcpyAsync(h->episode.d_start_in, h->cur_in().d_in, (size_t)n * sizeof(SceneIn), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->episode.d_start_state, h->d_state, (size_t)n * sizeof(SceneState), hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(dmpp::k_episode_reset, dim3((unsigned)((ns + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream, (int)ns, h->episode.d_stats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));            // (the upload stream reads the copies from its next launch on)
    h->episode.em = *em; h->episode.on = true;
    return features_ok(h, "pp_set_episodes");
}

int pp_get_episode_stats(pp_handle h, EpisodeStats* out, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->episode.d_stats) return fail(PP_ERR_STATE, "pp_get_episode_stats: pp_set_episodes was never called on this handle");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    return fetch_behind_advance(h, out, h->episode.d_stats, (size_t)n * sizeof(EpisodeStats), false);      // a staged advance included, as pp_get_ego_flags
}

// Episode spawn model.  Everything the host can check is checked before anything changes; the new pool is built
// beside the one in force and takes its place only once every record is on the map.
void pp_default_episode_spawn(EpisodeSpawn* sp)
{
    if (!sp) return;
    sp->seed = 1; sp->clearance = 2.0; sp->n_starts = 1; sp->order = 0; sp->contact = 1; sp->check = 3;
}

int pp_set_episode_spawn(pp_handle h, const EpisodeSpawn* sp, const SceneIn* starts_in, const SceneState* starts_state)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    PP_TRY(refuse_if_staged(h, "pp_set_episode_spawn", "the spawn model"));
    if (!sp) { h->spawn.on = false; retire(h, dmpp::kSetSpawn); return features_ok(h, "pp_set_episode_spawn"); }
    if (!h->episode.on) return fail(PP_ERR_STATE, "pp_set_episode_spawn: episodes are off (pp_set_episodes comes first: its capture is start record 0)");
    const int n = h->n_scenes, M = sp->n_starts;
    if (M < 1 || M > DMPP_EPISODE_MAX_STARTS) return fail(PP_ERR_ARG, "pp_set_episode_spawn: n_starts must be 1 .. DMPP_EPISODE_MAX_STARTS");
    if (!std::isfinite(sp->clearance) || sp->clearance < 0) return fail(PP_ERR_ARG, "pp_set_episode_spawn: clearance must be finite and >= 0");
    if (sp->order != 0 && sp->order != 1) return fail(PP_ERR_ARG, "pp_set_episode_spawn: order must be 0 (hashed) or 1 (round robin)");
    if ((sp->check & ~3) != 0) return fail(PP_ERR_ARG, "pp_set_episode_spawn: check holds bits outside 3");
    if (M > 1 && (!starts_in || !starts_state)) return fail(PP_ERR_ARG, "pp_set_episode_spawn: n_starts > 1 needs the start records");
    if (M > 1 && (h->resident_mode != 1 || !h->have_map))
        return fail(PP_ERR_STATE, "pp_set_episode_spawn: start records are placed on the resident map (pp_set_map + pp_set_egos come first)");
    PP_TRY(quiesce(h, false));                            // nobody reads the pool in force
    // The new pool, its stats included, is built in the set that is NOT in force (or was last): a refusal below leaves the one in
    // force - and the readable stats of a model that went off - untouched
    const int o = h->spawn.ever ? 1 - h->spawn.cur : h->spawn.cur, stride = (n + 1) & ~1;
    const size_t recs = (size_t)M * (size_t)stride;       // room first: a failed allocation changes nothing
    PP_TRY(h->spawn.d_in[o].reserve(recs)); PP_TRY(h->spawn.d_state[o].reserve(recs)); PP_TRY(h->spawn.d_stats[o].reserve((size_t)h->caps.max_scenes));
    const unsigned was = feature_mask(h) & (dmpp::kSpawn | dmpp::retires(dmpp::kSetSpawn));
    h->spawn.on = false;                                  // (until everything below has landed: a failed copy leaves the spawn model off, not half a pool)
    retire(h, dmpp::kSetSpawn);                           // (the traffic reset of §4m and the episode log of §4n read cur_start of the model in force, schedule, world episodes and world reset are part of it: they go with it)
    SceneIn* pin = h->spawn.d_in[o]; SceneState* pst = h->spawn.d_state[o];
    HIP_TRY(hipMemcpyAsync(pin, h->episode.d_start_in, (size_t)n * sizeof(SceneIn), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(pst, h->episode.d_start_state, (size_t)n * sizeof(SceneState), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->spawn.d_stats[o], 0, (size_t)h->caps.max_scenes * sizeof(EpisodeSpawnStats), h->stream));
    int bad = 0;
    if (M > 1) {
        const dim3 grid((unsigned)((n + dmpp::kBlock - 1) / dmpp::kBlock)), block(dmpp::kBlock);
        HIP_TRY(hipMemsetAsync(h->d_map_bad, 0, sizeof(int), h->stream));
        for (int k = 1; k < M; k++) {                     // views and junction slices from the resident map, as pp_set_egos derives them
            SceneIn* rec = pin + (size_t)k * stride;
            HIP_TRY(hipMemcpyAsync(rec, starts_in + (size_t)(k - 1) * n, (size_t)n * sizeof(SceneIn), hipMemcpyDefault, h->stream));
            HIP_TRY(hipMemcpyAsync(pst + (size_t)k * stride, starts_state + (size_t)(k - 1) * n, (size_t)n * sizeof(SceneState), hipMemcpyDefault, h->stream));
            hipLaunchKernelGGL(dmpp::k_resolve_map, grid, block, 0, h->stream, n, rec, h->map_roads, h->d_map_first, h->d_map_lanes, h->d_attr, h->d_map_width,
                               h->map_junctions, h->d_map_junc, h->d_map_bad);
        }
        hipLaunchKernelGGL(dmpp::k_spawn_pin_slices, dim3((unsigned)(((size_t)n * (M - 1) + dmpp::kBlock - 1) / dmpp::kBlock)), block, 0, h->stream, n, M, stride, pin);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&bad, h->d_map_bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));            // the one host wait: the caller's arrays may go; the upload stream reads the pool from its next launch on
    if (bad) {
        switch_features(h, was, true);                    // (nothing in force was touched: the spawn model and everything the call retires are as they were)
        return fail(PP_ERR_ARG, "pp_set_episode_spawn: " + std::to_string(bad) + " start record(s) name a road or lane outside the map");
    }
    if (o != h->spawn.cur) {                              // the pool that was in force goes (nobody reads it: joined and waited above); its stats are 80 B a scene and stay
        h->spawn.d_in[h->spawn.cur] = DevBuf<SceneIn>(); h->spawn.d_state[h->spawn.cur] = DevBuf<SceneState>();
    }
    h->spawn.sp = *sp; h->spawn.stride = stride; h->spawn.cur = o; h->spawn.on = true; h->spawn.ever = true;
    return features_ok(h, "pp_set_episode_spawn");
}

int pp_get_episode_spawn_stats(pp_handle h, EpisodeSpawnStats* out, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->spawn.ever) return fail(PP_ERR_STATE, "pp_get_episode_spawn_stats: pp_set_episode_spawn was never called on this handle");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    return fetch_behind_advance(h, out, h->spawn.d_stats[h->spawn.cur], (size_t)n * sizeof(EpisodeSpawnStats), false);      // a staged advance included, as pp_get_episode_stats
}

// Scenario schedule.  Everything is checked on the host before anything changes.
void pp_default_episode_schedule(EpisodeSchedule* m)
{
    if (!m) return;
    *m = EpisodeSchedule{ 1, DMPP_EGO_PATH_END | DMPP_EGO_BAD_PATH | DMPP_EGO_LANE_END | DMPP_EGO_OFF_GRID | DMPP_EGO_TIMEOUT | DMPP_EGO_CONTACT, DMPP_EGO_ROUTE_END,
                          4, 256, 4096, 61440, 32768, 32768, 0 };
}

static int check_episode_schedule(const EpisodeSchedule* m, const char* fn)
{
    const int causes = 31 | DMPP_EGO_TIMEOUT | DMPP_EGO_CONTACT;
    const std::string f(fn);
    if (m->scope != 0 && m->scope != 1) return fail(PP_ERR_ARG, f + ": scope must be 0 (a row per scene) or 1 (one pooled row)");
    if ((m->fail_mask & ~causes) != 0 || (m->pass_mask & ~causes) != 0) return fail(PP_ERR_ARG, f + ": fail_mask / pass_mask hold bits outside 31 | 64 | 128");
    if (m->min_samples < 1) return fail(PP_ERR_ARG, f + ": min_samples must be >= 1");
    if (m->window != 0 && m->window < 2) return fail(PP_ERR_ARG, f + ": window must be 0 (no decay) or >= 2");
    if (m->floor_w < 1 || m->floor_w > 65535) return fail(PP_ERR_ARG, f + ": floor_w must be 1 .. 65535");
    if (m->gain < 0 || m->gain > 65535) return fail(PP_ERR_ARG, f + ": gain must be 0 .. 65535");
    if (m->target < 0 || m->target > 65536 || m->prior < 0 || m->prior > 65536) return fail(PP_ERR_ARG, f + ": target and prior must be 0 .. 65536");
    if (m->_pad != 0) return fail(PP_ERR_ARG, f + ": _pad must be 0");
    return PP_OK;
}

int pp_set_episode_schedule(pp_handle h, const EpisodeSchedule* m)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    PP_TRY(refuse_if_staged(h, "pp_set_episode_schedule", "the schedule"));
    if (!m) { h->spawn.sched_on = false; return features_ok(h, "pp_set_episode_schedule"); }
    if (!h->episode.on || !h->spawn.on) return fail(PP_ERR_STATE, "pp_set_episode_schedule: the spawn model is off (pp_set_episode_spawn comes first: the schedule draws its start records)");
    if (h->spawn.worlds_on) return fail(PP_ERR_STATE, "pp_set_episode_schedule: world episodes are on (pp_set_episode_worlds: one draw per world, a schedule keeps rows per scene)");
    if (h->spawn.sp.order != 0) return fail(PP_ERR_STATE, "pp_set_episode_schedule: the spawn model in force is round robin (order 1): a schedule replaces the HASHED choice");
    PP_TRY(check_episode_schedule(m, "pp_set_episode_schedule"));
    PP_TRY(quiesce(h, false));                            // (the upload stream, which reads and folds the rows, is behind the last advance)
    const size_t ns = (size_t)h->caps.max_scenes, n_rows = m->scope == 0 ? ns : 1;      // room first: a failed allocation changes nothing
    if (m->scope == 1) PP_TRY(h->spawn.d_fold_word.reserve(ns));
    PP_TRY(h->spawn.d_rows.reserve(n_rows));
    HIP_TRY(hipMemsetAsync(h->spawn.d_rows, 0, n_rows * sizeof(EpisodeScheduleRow), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));            // the one host wait: the upload stream reads the rows from its next launch on
    h->spawn.sched = *m; h->spawn.sched_on = true; h->spawn.sched_ever = true;
    return features_ok(h, "pp_set_episode_schedule");
}

int pp_get_episode_schedule(pp_handle h, EpisodeScheduleRow* rows, int n)
{
    if (!h || !rows) return fail(PP_ERR_ARG, "null argument");
    if (!h->spawn.sched_ever) return fail(PP_ERR_STATE, "pp_get_episode_schedule: pp_set_episode_schedule was never called on this handle");
    if (h->spawn.sched.scope == 1 ? n != 1 : (n < 0 || n > h->n_scenes || (size_t)n > h->spawn.d_rows.capacity()))
        return fail(PP_ERR_ARG, "pp_get_episode_schedule: n must be 1 in pooled scope and at most the resident scenes in per-scene scope");
    if (n == 0) return PP_OK;
    return fetch_behind_advance(h, rows, h->spawn.d_rows, (size_t)n * sizeof(EpisodeScheduleRow), false);      // a staged advance included, as pp_get_episode_spawn_stats
}

// pure host code: the weights the next draw would use for a row (the function k_respawn_sched calls)
int pp_episode_schedule_weights(const EpisodeSchedule* m, const EpisodeScheduleRow* row, int M, int32_t* w)
{
    if (!m || !row || !w) return fail(PP_ERR_ARG, "null argument");
    if (M < 1 || M > DMPP_EPISODE_MAX_STARTS) return fail(PP_ERR_ARG, "pp_episode_schedule_weights: M must be 1 .. DMPP_EPISODE_MAX_STARTS");
    PP_TRY(check_episode_schedule(m, "pp_episode_schedule_weights"));
    for (int k = 0; k < M; k++)
        if (row->n_fail[k] < 0 || row->n_fail[k] > row->n_end[k]) return fail(PP_ERR_ARG, "pp_episode_schedule_weights: a row has 0 <= n_fail <= n_end for every record");
    for (int k = 0; k < DMPP_EPISODE_MAX_STARTS; k++) w[k] = k < M ? dmpp::schedule_weight(*m, row->n_end[k], row->n_fail[k]) : 0;
    return PP_OK;
}

// Episode traffic reset.  Everything is checked on the host before anything changes; the new table and its counters
// are built beside the ones in force and take their place only once every copy has landed.  world: pp_set_episode_world_traffic
//  - the same for the vehicles of pp_set_world_traffic, which reset when their whole world restarts.
static int set_traffic_reset(pp_handle h, bool world, int n_sets, const TrafficStart* starts)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    const std::string fn = world ? "pp_set_episode_world_traffic" : "pp_set_episode_traffic";
    TrafficResetState& R = world ? h->wreset : h->treset;
    PP_TRY(refuse_if_staged(h, fn, world ? "the world traffic reset" : "the traffic reset"));
    if (n_sets == 0) { R.on = false; return features_ok(h, fn.c_str()); }
    if (world) {
        if (!h->traffic.on || !h->traffic.world) return fail(PP_ERR_STATE, fn + ": no world traffic is set (pp_set_world_traffic comes first)");
        if (!h->episode.on || !h->spawn.on || !h->spawn.worlds_on)
            return fail(PP_ERR_STATE, fn + ": world episodes are off (pp_set_episode_worlds comes first: a vehicle resets when its whole world restarts)");
    } else {
        if (!h->traffic.on) return fail(PP_ERR_STATE, fn + ": no traffic is set (pp_set_traffic comes first)");
        if (h->traffic.world) return fail(PP_ERR_STATE, fn + ": world traffic is in force (one vehicle belongs to many egos: a reset has no owner)");
        if (!h->episode.on) return fail(PP_ERR_STATE, fn + ": episodes are off (pp_set_episodes comes first)");
    }
    const int M = h->spawn.on ? h->spawn.sp.n_starts : 1;
    if (n_sets < 0 || (n_sets != 1 && n_sets != M))
        return fail(PP_ERR_ARG, fn + ": n_sets must be 1 or the n_starts of the spawn model in force (" + std::to_string(M) + ")");
    if (n_sets > 1 && !starts) return fail(PP_ERR_ARG, fn + ": n_sets > 1 needs the start states");
    const size_t n = (size_t)h->traffic.actors, given = starts ? (size_t)(n_sets - 1) * n : 0;
    for (size_t i = 0; i < given; i++) {
        if (!std::isfinite(starts[i].s)) return fail(PP_ERR_ARG, fn + ": start state " + std::to_string(i) + " has a non-finite s");
        if (!std::isfinite(starts[i].v) || starts[i].v < 0) return fail(PP_ERR_ARG, fn + ": start state " + std::to_string(i) + ": v must be finite and >= 0");
    }
    PP_TRY(quiesce(h, false));                            // (the upload stream, which writes s / v, is behind the last advance)
    if (!world && h->man.on) {                            // §4v: set 0 is an arc length on the INITIAL track, so every actor must still have the set call's state
        std::vector<dmpp::TrafficPin> pin(n); std::vector<TrafficManoeuvreState> st(n);
        HIP_TRY(hipMemcpyAsync(pin.data(), h->traffic.d_pin, n * sizeof(dmpp::TrafficPin), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(st.data(), h->man.d_state[h->traffic.cur], n * sizeof(TrafficManoeuvreState), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        const std::vector<TrafficManoeuvreState> want = initial_manoeuvre_states(h, pin);
        for (size_t a = 0; a < n; a++) {
            if (std::memcmp(&want[a], &st[a], sizeof st[a]) != 0)
                return fail(PP_ERR_STATE, fn + ": actor " + std::to_string(a) + " has left the state pp_set_traffic_manoeuvres gave it (set the manoeuvres again, then the reset)");
        }
    }
    const int o = R.ever ? 1 - R.cur : R.cur;
    if (!world) PP_TRY(R.d_scene.reserve(n));
    PP_TRY(R.d_starts[o].reserve((size_t)n_sets * n)); PP_TRY(R.d_resets[o].reserve(n));      // room first: a failed allocation changes nothing
    // (d_scene is single: while the reset is on it holds the scenes of the traffic in force, which is what is written again)
    if (!world) HIP_TRY(hipMemcpyAsync(R.d_scene, h->traffic.scene_of.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    TrafficStart* tab = R.d_starts[o];
    static_assert(sizeof(TrafficStart) == 16 && offsetof(TrafficStart, s) == 0 && offsetof(TrafficStart, v) == 8, "set 0 is gathered field by field");
    // set 0, the capture: s of the current array; v of the current array while following is on, else the speed of every pin
    HIP_TRY(hipMemcpy2DAsync(&tab->s, sizeof(TrafficStart), h->traffic.d_s[h->traffic.cur], sizeof(double), sizeof(double), n, hipMemcpyDeviceToDevice, h->stream));
    if (h->follow.on)
        HIP_TRY(hipMemcpy2DAsync(&tab->v, sizeof(TrafficStart), h->follow.d_v[h->traffic.cur], sizeof(double), sizeof(double), n, hipMemcpyDeviceToDevice, h->stream));
    else
        HIP_TRY(hipMemcpy2DAsync(&tab->v, sizeof(TrafficStart), h->traffic.d_pin, sizeof(dmpp::TrafficPin), sizeof(double), n, hipMemcpyDeviceToDevice, h->stream));
    if (given) HIP_TRY(hipMemcpyAsync(tab + n, starts, given * sizeof(TrafficStart), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(R.d_resets[o], 0, n * sizeof(int32_t), h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));            // the one host wait: the caller's array may go; the upload stream reads the table from its next launch on
    if (o != R.cur) R.d_starts[R.cur] = DevBuf<TrafficStart>();      // the table that was in force goes; its counters are 4 B an actor and stay
    R.n_sets = n_sets; R.actors = (int)n; R.cur = o; R.on = true; R.ever = true;
    return features_ok(h, fn.c_str());
}

static int get_traffic_resets(pp_handle h, bool world, int32_t* n_resets, int n)
{
    if (!h || (!n_resets && n > 0)) return fail(PP_ERR_ARG, "null argument");
    const TrafficResetState& R = world ? h->wreset : h->treset;
    if (!R.ever)
        return fail(PP_ERR_STATE, world ? "pp_get_episode_world_traffic_resets: pp_set_episode_world_traffic was never called on this handle"
                                        : "pp_get_episode_traffic_resets: pp_set_episode_traffic was never called on this handle");
    if (n < 0 || n > R.actors) return fail(PP_ERR_ARG, world ? "n exceeds the vehicles" : "n exceeds the actors");
    if (n == 0) return PP_OK;
    return fetch_behind_advance(h, n_resets, R.d_resets[R.cur], (size_t)n * sizeof(int32_t), true);      // waits as pp_get_traffic_state does
}

int pp_set_episode_traffic(pp_handle h, int n_sets, const TrafficStart* starts) { return set_traffic_reset(h, false, n_sets, starts); }
int pp_get_episode_traffic_resets(pp_handle h, int32_t* n_resets, int n) { return get_traffic_resets(h, false, n_resets, n); }
int pp_set_episode_world_traffic(pp_handle h, int n_sets, const TrafficStart* starts) { return set_traffic_reset(h, true, n_sets, starts); }
int pp_get_episode_world_traffic_resets(pp_handle h, int32_t* n_resets, int n) { return get_traffic_resets(h, true, n_resets, n); }

// World episodes: part of the spawn model in force.  Captures nothing from the fleet: the step reads the fleet in force
// at each advance.
int pp_set_episode_worlds(pp_handle h, int on)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    PP_TRY(refuse_if_staged(h, "pp_set_episode_worlds", "the world episodes"));
    if (!h->episode.on || !h->spawn.on) return fail(PP_ERR_STATE, "pp_set_episode_worlds: the spawn model is off (pp_set_episode_spawn comes first: a world restarts on its start records)");
    if (h->spawn.sched_on) return fail(PP_ERR_STATE, "pp_set_episode_worlds: a schedule is in force (pp_set_episode_schedule keeps rows per scene, a world draws once)");
    PP_TRY(quiesce(h, false));                            // (the upload stream, which runs the episode step, is behind the last advance)
    if (on) PP_TRY(h->spawn.d_world_end.reserve((size_t)h->caps.max_scenes));      // room first: a failed allocation changes nothing
    if (on) h->spawn.worlds_on = true;
    else switch_features(h, dmpp::kWorldEpisodes | dmpp::dependants(dmpp::kWorldEpisodes), false);      // (the world reset of §4t keys on every member restarting together: it goes with the mode)
    return features_ok(h, "pp_set_episode_worlds");
}

// Episode log.  Everything is checked on the host before anything changes.
int pp_set_episode_log(pp_handle h, int cap)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (cap < 0 || cap > DMPP_EPISODE_LOG_MAX) return fail(PP_ERR_ARG, "pp_set_episode_log: cap must be 0 .. DMPP_EPISODE_LOG_MAX");
    PP_TRY(refuse_if_staged(h, "pp_set_episode_log", "the log"));
    if (cap == 0) { h->elog.on = false; return features_ok(h, "pp_set_episode_log"); }
    if (!h->episode.on) return fail(PP_ERR_STATE, "pp_set_episode_log: episodes are off (pp_set_episodes comes first)");
    PP_TRY(quiesce(h, false));                            // (the upload stream, which appends, is behind the last advance)
    const size_t ns = (size_t)h->caps.max_scenes;         // room first: a failed allocation changes nothing
    PP_TRY(h->elog.d_ring.reserve((size_t)cap)); PP_TRY(h->elog.d_total.reserve(1)); PP_TRY(h->elog.d_start_of.reserve(ns));
    if (h->score.on) PP_TRY(h->elog.d_score.reserve(ns));
    HIP_TRY(hipMemsetAsync(h->elog.d_total, 0, sizeof(long long), h->stream));
    static_assert(sizeof(EpisodeSpawnStats) == 80 && offsetof(EpisodeSpawnStats, cur_start) == 12, "cur_start is gathered out of the spawn stats");
    if (h->spawn.on)      // the start record every running episode is on
        HIP_TRY(hipMemcpy2DAsync(h->elog.d_start_of, sizeof(int32_t), &h->spawn.d_stats[h->spawn.cur].get()->cur_start, sizeof(EpisodeSpawnStats), sizeof(int32_t),
                                 (size_t)h->n_scenes, hipMemcpyDeviceToDevice, h->stream));
    else HIP_TRY(hipMemsetAsync(h->elog.d_start_of, 0, ns * sizeof(int32_t), h->stream));
    if (h->elog.d_score) {
        hipLaunchKernelGGL(dmpp::k_score_reset, dim3((unsigned)((ns + dmpp::kBlock - 1) / dmpp::kBlock)), dim3(dmpp::kBlock), 0, h->stream, (int)ns, h->elog.d_score);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(h->stream));            // the one host wait: the upload stream reads all of it from its next launch on
    h->elog.cap = cap; h->elog.seq = 0; h->elog.read = 0; h->elog.lost = 0; h->elog.on = true; h->elog.ever = true;
    return features_ok(h, "pp_set_episode_log");
}

// records appended since the set call, a staged advance included as in pp_get_episode_stats (host wait)
static int episode_log_total(pp_handle h, long long* total) { return fetch_behind_advance(h, total, h->elog.d_total, sizeof(long long), false); }

int pp_read_episode_log(pp_handle h, EpisodeRecord* out, int max_records, long long* n_lost)
{
    if (!h || max_records < 0 || (!out && max_records > 0)) return fail(PP_ERR_ARG, "pp_read_episode_log: null argument or negative count");
    if (!h->elog.ever) return fail(PP_ERR_STATE, "pp_read_episode_log: pp_set_episode_log was never called on this handle");
    long long total = 0;
    PP_TRY(episode_log_total(h, &total));
    const long long cap = h->elog.cap, oldest = std::max(h->elog.read, total - cap), lost = oldest - h->elog.read;
    const long long n = std::min(total - oldest, (long long)max_records);
    const long long i0 = oldest % cap, n0 = std::min(n, cap - i0);      // the run up to the end of the ring, then the run from its start
    if (n0 > 0) HIP_TRY(hipMemcpyAsync(out, h->elog.d_ring + i0, (size_t)n0 * sizeof(EpisodeRecord), hipMemcpyDeviceToHost, h->stream));
    if (n > n0) HIP_TRY(hipMemcpyAsync(out + n0, h->elog.d_ring, (size_t)(n - n0) * sizeof(EpisodeRecord), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->elog.read = oldest + n; h->elog.lost += lost;
    if (n_lost) *n_lost = lost;
    return (int)n;
}

int pp_get_episode_log_info(pp_handle h, long long* total, long long* lost_total)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!h->elog.ever) return fail(PP_ERR_STATE, "pp_get_episode_log_info: pp_set_episode_log was never called on this handle");
    long long t = 0;
    PP_TRY(episode_log_total(h, &t));
    if (total) *total = t;
    if (lost_total) *lost_total = h->elog.lost + std::max(0ll, t - (long long)h->elog.cap - h->elog.read);      // (what the next read will report included)
    return PP_OK;
}

// A grid that follows the ego: host checks only; the model is a kernel argument of the next advance.
void pp_default_grid_follow(GridFollow* gf)
{
    if (!gf) return;
    gf->goal_point = DMPP_PATH_POINTS - 1; gf->margin_cells = 32;       // the end of the planned path; 8 m at the default 0.25 m cell
}

int pp_set_grid_follow(pp_handle h, const GridFollow* gf)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!gf) { h->grid_follow = GridFollow{ 0, 0 }; return features_ok(h, "pp_set_grid_follow"); }
    if (gf->goal_point < 1 || gf->goal_point > DMPP_PATH_POINTS - 1)
        return fail(PP_ERR_ARG, "pp_set_grid_follow: goal_point must be 1 .. " + std::to_string(DMPP_PATH_POINTS - 1));
    if (gf->margin_cells < 0) return fail(PP_ERR_ARG, "pp_set_grid_follow: margin_cells must be >= 0");
    if (2LL * gf->margin_cells >= (long long)std::min(h->cfg.grid_w, h->cfg.grid_h))
        return fail(PP_ERR_ARG, "pp_set_grid_follow: 2 * margin_cells must be smaller than min(grid_w, grid_h)");
    h->grid_follow = *gf;
    return features_ok(h, "pp_set_grid_follow");
}

// Ego tracking model: host checks; the model is a kernel argument of the next advance, the per-scene states are
// allocated and zeroed by the first call that brings a model.
void pp_default_ego_tracker(EgoTracker* tk)
{
    if (!tk) return;
    tk->look_min = 3.0; tk->look_gain = 0.5; tk->max_curv = 0.2; tk->curv_rate = 0.3; tk->curv_bias = 0.0; tk->n_sub = 2; tk->_pad = 0;
}

int pp_set_ego_tracker(pp_handle h, const EgoTracker* tk)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!tk) { h->tracker.on = false; return PP_OK; }
    if (!std::isfinite(tk->look_min) || !std::isfinite(tk->look_gain) || !std::isfinite(tk->max_curv) || !std::isfinite(tk->curv_rate) || !std::isfinite(tk->curv_bias))
        return fail(PP_ERR_ARG, "pp_set_ego_tracker: every field must be finite");
    if (!(tk->look_min > 0) || !(tk->look_gain >= 0) || !(tk->max_curv > 0) || !(tk->curv_rate > 0))
        return fail(PP_ERR_ARG, "pp_set_ego_tracker: look_min, max_curv and curv_rate must be > 0, look_gain >= 0");
    if (tk->n_sub < 1 || tk->n_sub > 8) return fail(PP_ERR_ARG, "pp_set_ego_tracker: n_sub must be 1 .. 8");
    if (!h->tracker.d_state) {
        HIP_TRY(hipSetDevice(h->device));
        PP_TRY(h->tracker.d_state.reserve((size_t)h->caps.max_scenes));
        HIP_TRY(hipMemsetAsync(h->tracker.d_state, 0, (size_t)h->caps.max_scenes * sizeof(EgoTrackState), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));       // (the first advance runs on the upload stream)
    }
    h->tracker.tk = *tk; h->tracker.tk._pad = 0; h->tracker.on = true;
    return PP_OK;
}

int pp_get_ego_track_state(pp_handle h, EgoTrackState* out, int n)
{
    if (!h || !out) return fail(PP_ERR_ARG, "null argument");
    if (!h->tracker.d_state) return fail(PP_ERR_STATE, "pp_get_ego_track_state: pp_set_ego_tracker was never called on this handle");
    if (n < 0 || n > h->n_scenes) return fail(PP_ERR_ARG, "n exceeds the resident scenes");
    return fetch_behind_advance(h, out, h->tracker.d_state, (size_t)n * sizeof(EgoTrackState), false);      // a staged advance included, as pp_get_ego_flags
}

int pp_get_obstacles(pp_handle h, int scene, ObPoint* out, int cap)
{
    if (!h || (!out && cap > 0)) return fail(PP_ERR_ARG, "null argument");
    if (scene < 0 || scene >= h->n_scenes || cap < 0) return fail(PP_ERR_ARG, "pp_get_obstacles: scene or cap out of range");
    const bool staged = h->in_staged >= 0 && h->rollout.staged_by_advance;      // (the set pp_get_scene_in reads)
    const InputSet& I = h->in_sets[staged ? h->in_staged : h->in_cur];
    HIP_TRY(hipSetDevice(h->device));
    if (staged) PP_TRY(I.up.wait(h->stream));
    int32_t sl[2] = { 0, 0 };
    { int r = fetch(h, sl, &I.d_in[scene].obs_off, sizeof(sl)); if (r) return r; }
    static_assert(offsetof(SceneIn, obs_n) == offsetof(SceneIn, obs_off) + 4, "obs_off and obs_n are read as one pair");
    if (sl[1] == 0) return 0;
    if (sl[0] < 0 || sl[1] < 0 || (long long)sl[0] + sl[1] > (long long)h->caps.max_obs_total)
        return fail(PP_ERR_STATE, "pp_get_obstacles: the scene's obstacle slice lies outside the pool");
    const int m = std::min(sl[1], cap);
    if (m > 0) { int r = fetch(h, out, I.d_obs + sl[0], (size_t)m * sizeof(ObPoint)); if (r) return r; }
    return sl[1];
}

// One request for the last tick's results (FetchAsk), from one of the three typed entry points below.
static int fetch_async(pp_handle h, const FetchAsk& ask, long long* tick_id)
{
    if (!ask.plan[0].dst && !ask.plan[1].dst && !ask.grid.dst) return fail(PP_ERR_ARG, "nothing to fetch");
    if (h->tick_seq == 0 || h->n_scenes <= 0) return fail(PP_ERR_STATE, "pp_fetch_async: no tick has been enqueued");
    if (ask.grid.dst && !h->cfg.grid_stage) return fail(PP_ERR_STATE, "pp_fetch_async: the last tick ran without the grid stage");
    if (ask.packed) {
        if (!h->packed.on) return fail(PP_ERR_STATE, "pp_fetch_packed_async: the packed fetch is not armed (pp_set_packed_fetch)");
        if (h->packed.plan_tick != h->tick_seq || (ask.grid.dst && h->packed.grid_tick != h->tick_seq))
            return fail(PP_ERR_STATE, "pp_fetch_packed_async: the last tick ran before the packed fetch was armed");
    }
    HIP_TRY(hipSetDevice(h->device));
    { int r = flush_group(h); if (r) return r; }          // the downloads follow the last tick's scoring pass: it must be enqueued
    { int r = ensure_streaming(h); if (r) return r; }
    const long long T = h->tick_seq;
    const int slot = (int)(T % kDone);
    if (h->rec_last.tick != T) {
        // the last tick was enqueued before streaming began: one event behind everything stands in for its two
        { int r = join_all(h); if (r) return r; }
        hipEvent_t e = get_sync_event(h);
        if (!e) return fail(PP_ERR_HIP, "event creation failed");
        HIP_TRY(hipEventRecord(e, h->stream));
        TickRec rec = { T, h->in_cur, e, nullptr };
        h->inflight.push_back(rec); h->rec_last = rec;
    }
    const TickRec& R = h->rec_last;
    if (h->done_tick[slot] != T) { h->done_tick[slot] = T; for (FetchSide& S : h->dl) S.done[slot].forget(); }      // (an earlier tick's downloads)
    FetchRec p = { T, slot, h->plan_cur, R.ev_front, (size_t)h->n_scenes, false, 0, {} };
    FetchRec g = { T, slot, h->gout_set, R.ev_tail ? R.ev_tail : R.ev_front, (size_t)h->n_scenes, false, 0, {} };
    for (const FetchCopy& c : ask.plan) p.add(c.dst, c.src, c.bytes, c.stride);
    g.add(ask.grid.dst, ask.grid.src, ask.grid.bytes, ask.grid.stride);
    if (p.n_copies) h->dl[kPlanSide].queue.push_back(p);
    if (g.n_copies) h->dl[kGridSide].queue.push_back(g);
    { int r = pump_fetches(h); if (r) return r; }
    if (tick_id) *tick_id = T;
    return PP_OK;
}

// The sources are those of the last enqueued tick: PlanOut set plan_cur, GridOut set gout_set
int pp_fetch_async(pp_handle h, PlanOut* plan, GridOut* grid, long long* tick_id)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    const GridOut* gout = h->d_gout[h->gout_set];
    return fetch_async(h, { false, { whole_records(plan, (const PlanOut*)h->plan_out()), {} }, whole_records(grid, gout) }, tick_id);
}
int pp_fetch_published_async(pp_handle h, PlanningOut* result, PlanningStatus* show, GridOut* grid, long long* tick_id)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    const GridOut* gout = h->d_gout[h->gout_set];
    return fetch_async(h, { false, { plan_slice(result, h->plan_out(), offsetof(PlanOut, result)), plan_slice(show, h->plan_out(), offsetof(PlanOut, show)) },
                            whole_records(grid, gout) }, tick_id);
}


// ---------------------------------------------------------------------------------------
// Packed streamed fetch
int pp_set_packed_fetch(pp_handle h, int on)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!on) { h->packed.on = false; return PP_OK; }          // the sets stay; a pending download of an earlier tick still reads them
    if (h->packed.on) return PP_OK;
    HIP_TRY(hipSetDevice(h->device));
    PP_TRY(flush_group(h));                                   // the ticks before arming are launched as they stand, unpacked
    PP_TRY(ensure_streaming(h));
    const size_t ns = (size_t)h->caps.max_scenes;
    for (int q = 0; q < kPlan; q++) PP_TRY(h->packed.d_plan[q].reserve(ns));
    if (h->d_grid) for (int q = 0; q < kGoutRing; q++) PP_TRY(h->packed.d_grid[q].reserve(ns));      // (a handle created with the grid stage)
    h->packed.on = true;
    return PP_OK;
}
int pp_fetch_packed_async(pp_handle h, PackedPlan* plan, PackedGrid* grid, long long* tick_id)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (!plan && !grid) return fail(PP_ERR_ARG, "pp_fetch_packed_async: nothing to fetch");
    // the packed records of the same tick: PackedPlan set plan_cur, PackedGrid set of the GridOut set's group position (null until armed: refused before use)
    const PackedPlan* pkp = h->packed.d_plan[h->plan_cur]; const PackedGrid* pkg = h->packed.d_grid[h->gout_set / kGroupMax];
    return fetch_async(h, { true, { whole_records(plan, pkp), {} }, whole_records(grid, pkg) }, tick_id);
}
int pp_unpack_plan(const PlannerConfig* cfg, const PackedPlan* in, int n, PlanningOut* result, PlanningStatus* show, DecisionOutPod* dec)
{
    if (!cfg || !in || n < 0) return fail(PP_ERR_ARG, "pp_unpack_plan: null argument or negative count");
    for (int s = 0; s < n; s++) dmpp::unpack_plan_one(*cfg, in[s], result ? result + s : nullptr, show ? show + s : nullptr, dec ? dec + s : nullptr);
    return PP_OK;
}
int pp_unpack_grid(const PlannerConfig* cfg, const PackedGrid* in, int n, GridOut* out)
{
    if (!cfg || !in || !out || n < 0) return fail(PP_ERR_ARG, "pp_unpack_grid: null argument or negative count");
    int bad = 0, first = -1;
    for (int s = 0; s < n; s++) if (!dmpp::unpack_grid_one(*cfg, in[s], out + s)) { if (bad++ == 0) first = s; }
    if (bad) return fail(PP_ERR_ARG, "pp_unpack_grid: " + std::to_string(bad) + " record(s) no tick packs (first: scene " + std::to_string(first) +
                                     "): n_steps outside 0 .. 199, an unknown kind or DMPP_PACKED_BAD, best_candidate outside 0 .. 16, or a walk that leaves the grid; their GridOut is zeroed");
    return PP_OK;
}

long long pp_tick_id(pp_handle h) { return h ? h->tick_seq : -1; }

int pp_wait_tick(pp_handle h, long long tick_id, int* n_poisoned)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    if (n_poisoned) *n_poisoned = 0;
    if (tick_id <= 0 || tick_id > h->tick_seq) return fail(PP_ERR_ARG, "pp_wait_tick: no such tick");
    const int slot = (int)(tick_id % kDone);
    if (!h->streaming || h->done_tick[slot] != tick_id)
        return fail(PP_ERR_ARG, "pp_wait_tick: no pp_fetch_async was issued for that tick (or more than " + std::to_string(kDone) + " ticks ago)");
    HIP_TRY(hipSetDevice(h->device));
    { int r = flush_group(h); if (r) return r; }
    { int r = pump_fetches(h, tick_id); if (r) return r; }
    for (const FetchSide& S : h->dl) PP_TRY(S.done[slot].host_wait());      // (recorded by pump_fetches above, behind the copies it issued - if any were asked for)
    const int bad = (int)reinterpret_cast<volatile int32_t*>(h->h_bad.get())[slot];
    if (n_poisoned) *n_poisoned = bad;
    if (bad) return fail(PP_ERR_ARG, "tick " + std::to_string(tick_id) + ": " + std::to_string(bad) + " scene(s) of its update had a slice outside its pool (or a road / lane outside the map) and ran with empty inputs");
    return PP_OK;
}

int pp_tick_io(pp_handle h, PpSceneIo* io)
{
    if (!h || !io) return fail(PP_ERR_ARG, "null argument");
    if (h->n_scenes != 1) return fail(PP_ERR_STATE, "pp_tick_io moves ONE resident scene (pp_set_scenes with n_scenes = 1 comes first: its lane pool stays)");
    if ((io->want & PP_IO_WANT_GRID) && !h->cfg.grid_stage) return fail(PP_ERR_STATE, "PP_IO_WANT_GRID: the handle's configuration has the grid stage off");
    // The counts are checked here, in front of everything: a refused call launches nothing and leaves block, handle and tick id
    // as they were.  (k_io_in clamps them again: a fence, never the rule.)
    const int max_obs = std::min(PP_IO_MAX_OBS, h->caps.max_obs_total), max_ref = std::min(DMPP_MAX_REFPATH, h->caps.max_ref_pts_total);
    const int n_obs = io->n_obs, n_ref = io->n_ref;
    if (n_obs < 0 || n_ref < 0) return fail(PP_ERR_ARG, "pp_tick_io: io->n_obs and io->n_ref must not be negative");
    if (n_obs > max_obs)
        return fail(PP_ERR_CAPACITY, "pp_tick_io: io->n_obs = " + std::to_string(n_obs) + " obstacles, the handle takes " + std::to_string(max_obs) + " (PP_IO_MAX_OBS, caps.max_obs_total)");
    if (n_ref > max_ref)
        return fail(PP_ERR_CAPACITY, "pp_tick_io: io->n_ref = " + std::to_string(n_ref) + " refpath points, the handle takes " + std::to_string(max_ref) + " (DMPP_MAX_REFPATH, caps.max_ref_pts_total)");
    HIP_TRY(hipSetDevice(h->device));
    // k_io_in rewrites the inputs (and the state) that the kernels of earlier ticks read.  A one-stream tick has ended on the
    // handle's stream: launching an open group is enough.  A piped one ran on the other streams: all of them are joined first.
    if (h->last_piped) { int r = join_all(h); if (r) return r; }
    else {
        { int r = flush_group(h); if (r) return r; }
        PP_TRY(h->score.ego.wait(h->stream));             // ... and the scorecard of the last tick
    }
    h->in_staged = -1; h->rollout.staged_by_advance = false;
    hipLaunchKernelGGL(dmpp::k_io_in, dim3(1), dim3(dmpp::kBlock), 0, h->stream, io, max_obs, max_ref, h->n_lane_pts, h->cur_in().d_in, h->d_state, h->cur_in().d_obs, h->d_ref);
    HIP_TRY(hipGetLastError());
    h->cur_in().n_obs_total = n_obs; h->cur_in().have_motion = false;
    h->n_ref_pts = std::max(h->n_ref_pts, max_ref);
    note_current_set(h);
    // A piped tick (one scene: grid stage on and DMPP_PIPELINE_MIN <= 1) starts its front chain on another stream, which nothing
    // else orders behind k_io_in.  The one-stream tick starts on the handle's stream: no event and no wait there.
    if (tick_piped(h)) {
        const hipStream_t front = tick_streams(h, true, true, h->parity).front;
        if (front != h->stream) { PP_TRY(h->io_in.record(h->stream)); PP_TRY(h->io_in.wait(front)); }
    }
    { int r = pp_plan_tick(h); if (r) return r; }
    if (h->last_piped) { int r = join_all(h); if (r) return r; }      // (a one-scene tick ends on the handle's stream, as a rule: nothing to join)
    hipLaunchKernelGGL(dmpp::k_io_out, dim3(1), dim3(dmpp::kBlock), 0, h->stream, io, (int)io->want, h->plan_out(), h->d_state,
                       h->cfg.grid_stage ? h->d_gout[h->gout_set] : nullptr, h->d_dec_ref);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (reinterpret_cast<volatile int32_t*>(&io->status)[0]) return fail(PP_ERR_ARG, "pp_tick_io: a lane slice of io->in lies outside the resident lane pool (the scene ran with empty lanes)");
    return PP_OK;
}

#ifdef DMPP_DEBUG_SEARCH
int pp_debug_score_counters(int* out8, int reset)          // debug build only (tools/dbg_score.py)
{
    HIP_TRY(hipMemcpyFromSymbol(out8, HIP_SYMBOL(dmpp::g_dbg_score), 8 * sizeof(int)));
    if (reset) { int z[8] = { 0 }; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(dmpp::g_dbg_score), z, sizeof(z))); }
    return PP_OK;
}
int pp_debug_score_stamps(unsigned* out, int n_items)      // debug build only (tools/dbg_score_timing.py): [n_items][kDbgScorePhases] cycles
{
    if (!out || n_items < 0 || n_items > dmpp::kDbgScoreItems) return fail(PP_ERR_ARG, "pp_debug_score_stamps: bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(dmpp::g_dbg_score_ph), (size_t)n_items * dmpp::kDbgScorePhases * sizeof(unsigned)));
    return PP_OK;
}
#endif

void* pp_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); g_err = "hipHostMalloc failed"; return nullptr; }
    return p;
}
void pp_host_free(void* p) { if (p) (void)hipHostFree(p); }
int pp_host_register(void* p, size_t bytes)
{
    if (!p || !bytes) return fail(PP_ERR_ARG, "null argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return PP_OK;
}
int pp_host_unregister(void* p) { if (!p) return PP_OK; HIP_TRY(hipHostUnregister(p)); return PP_OK; }

// ---------------------------------------------------------------------------------------
// stand-alone operators
static int need_scratch(pp_handle h, size_t bytes)
{
    if (bytes <= h->d_scratch.capacity()) return PP_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return h->d_scratch.reserve(bytes);
}
static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

int pp_search_obstacle_batch(pp_handle h, int nq, const GlobalPoint2D* paths, const int32_t* path_off, const ObPoint* obs,
                             const int32_t* obs_off, const double* lat_lo, const double* lat_hi, Path_Obs* out)
{
    if (!h || !paths || !path_off || !obs_off || !lat_lo || !lat_hi || !out) return fail(PP_ERR_ARG, "null argument");
    if (nq <= 0) return PP_OK;
    HIP_TRY(hipSetDevice(h->device));
    // offsets are small host arrays by contract here (they size the copies)
    const int np = path_off[nq], no = obs_off[nq];
    for (int q = 0; q < nq; q++) if (path_off[q + 1] - path_off[q] > dmpp::kSoMaxPts) return fail(PP_ERR_CAPACITY, "a path longer than 2048 points");
    size_t o_paths = 0, o_poff = o_paths + al256((size_t)np * sizeof(GlobalPoint2D)), o_obs = o_poff + al256((size_t)(nq + 1) * 4),
           o_ooff = o_obs + al256((size_t)no * sizeof(ObPoint)), o_lo = o_ooff + al256((size_t)(nq + 1) * 4),
           o_hi = o_lo + al256((size_t)nq * 8), o_out = o_hi + al256((size_t)nq * 8), total = o_out + al256((size_t)nq * sizeof(Path_Obs));
    int r = need_scratch(h, total); if (r) return r;
    char* d = (char*)h->d_scratch;
    if (np) HIP_TRY(hipMemcpyAsync(d + o_paths, paths, (size_t)np * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(d + o_poff, path_off, (size_t)(nq + 1) * 4, hipMemcpyDefault, h->stream));
    if (no && obs) HIP_TRY(hipMemcpyAsync(d + o_obs, obs, (size_t)no * sizeof(ObPoint), hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(d + o_ooff, obs_off, (size_t)(nq + 1) * 4, hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(d + o_lo, lat_lo, (size_t)nq * 8, hipMemcpyDefault, h->stream));
    HIP_TRY(hipMemcpyAsync(d + o_hi, lat_hi, (size_t)nq * 8, hipMemcpyDefault, h->stream));
    hipLaunchKernelGGL(dmpp::k_search_obstacle_batch, dim3(nq), dim3(DMPP_WAVE), 0, h->stream, h->cfg, nq,
                       (const GlobalPoint2D*)(d + o_paths), (const int32_t*)(d + o_poff), (const ObPoint*)(d + o_obs),
                       (const int32_t*)(d + o_ooff), (const double*)(d + o_lo), (const double*)(d + o_hi), (Path_Obs*)(d + o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d + o_out, (size_t)nq * sizeof(Path_Obs), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

int pp_geom_batch(pp_handle h, int op, int n, const GlobalPoint2D* a, const GlobalPoint2D* b, const GlobalPoint2D* c3, double* out)
{
    if (!h || !a || !out || op < 0 || op > 5) return fail(PP_ERR_ARG, "bad argument");
    if (((op <= 1 || op == 3) && !b) || (op == 0 && !c3)) return fail(PP_ERR_ARG, "missing operand");
    if (n <= 0) return PP_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t pb = al256((size_t)n * sizeof(GlobalPoint2D));
    int r = need_scratch(h, 3 * pb + al256((size_t)n * 8)); if (r) return r;
    char* d = (char*)h->d_scratch;
    HIP_TRY(hipMemcpyAsync(d, a, (size_t)n * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    if (b) HIP_TRY(hipMemcpyAsync(d + pb, b, (size_t)n * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    if (c3) HIP_TRY(hipMemcpyAsync(d + 2 * pb, c3, (size_t)n * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    hipLaunchKernelGGL(dmpp::k_geom_batch, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->cfg, op, n, (const GlobalPoint2D*)d,
                       (const GlobalPoint2D*)(d + pb), (const GlobalPoint2D*)(d + 2 * pb), (double*)(d + 3 * pb));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d + 3 * pb, (size_t)n * 8, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

int pp_scalar_stage(pp_handle h, int op, const double* in, int n_in, const GlobalPoint2D* last_Bpoints, double* out, int n_out)
{
    if (!h || !in || !out || op < 0 || op > 2 || n_in < 1 || n_in > 8 || n_out < 1 || n_out > 4) return fail(PP_ERR_ARG, "bad argument");
    if (op == 2 && !last_Bpoints) return fail(PP_ERR_ARG, "CalculateRadius needs the 200 path points");
    HIP_TRY(hipSetDevice(h->device));
    int r = need_scratch(h, 4096 + DMPP_PATH_POINTS * sizeof(GlobalPoint2D)); if (r) return r;
    char* d = (char*)h->d_scratch;
    HIP_TRY(hipMemcpyAsync(d, in, (size_t)n_in * 8, hipMemcpyDefault, h->stream));
    if (op == 2) HIP_TRY(hipMemcpyAsync(d + 4096, last_Bpoints, DMPP_PATH_POINTS * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    hipLaunchKernelGGL(dmpp::k_scalar_stage, dim3(1), dim3(64), 0, h->stream, h->cfg, op, (const double*)d,
                       (const GlobalPoint2D*)(d + 4096), (double*)(d + 2048));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d + 2048, (size_t)n_out * 8, hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

int pp_bezier(pp_handle h, GlobalPoint3D s, GlobalPoint3D e, GlobalPoint2D* out, int n)
{
    if (!h || !out || n <= 0) return fail(PP_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    int r = need_scratch(h, (size_t)n * sizeof(GlobalPoint2D)); if (r) return r;
    hipLaunchKernelGGL(dmpp::k_bezier, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->cfg, s, e, (GlobalPoint2D*)h->d_scratch.get(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->d_scratch, (size_t)n * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

int pp_mean_points(pp_handle h, const GlobalPoint2D* in, int n_in, GlobalPoint2D* out, int n_out)
{
    if (!h || !out || n_out <= 0 || n_in < 0 || (n_in > 0 && !in)) return fail(PP_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    const size_t ib = al256((size_t)(n_in > 0 ? n_in : 1) * sizeof(GlobalPoint2D)), cb = al256((size_t)(n_in > 0 ? n_in : 1) * 8);
    int r = need_scratch(h, ib + cb + (size_t)n_out * sizeof(GlobalPoint2D)); if (r) return r;
    char* d = (char*)h->d_scratch;
    if (n_in) HIP_TRY(hipMemcpyAsync(d, in, (size_t)n_in * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    hipLaunchKernelGGL(dmpp::k_cumlen, dim3(1), dim3(DMPP_WAVE), 0, h->stream, (const GlobalPoint2D*)d, n_in, (double*)(d + ib));
    hipLaunchKernelGGL(dmpp::k_mean_points, dim3((n_out + 255) / 256), dim3(256), 0, h->stream, h->cfg, (const GlobalPoint2D*)d,
                       (const double*)(d + ib), n_in, (GlobalPoint2D*)(d + ib + cb), n_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d + ib + cb, (size_t)n_out * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

int pp_create_new_path(pp_handle h, const GlobalPoint2D* path, int n, double offset, GlobalPoint2D* out)
{
    if (!h || !path || !out || n < 0) return fail(PP_ERR_ARG, "bad argument");
    if (n == 0) return PP_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t pb = al256((size_t)n * sizeof(GlobalPoint2D));
    int r = need_scratch(h, 2 * pb); if (r) return r;
    char* d = (char*)h->d_scratch;
    HIP_TRY(hipMemcpyAsync(d, path, (size_t)n * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    hipLaunchKernelGGL(dmpp::k_create_new_path, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->cfg, (const GlobalPoint2D*)d, n, offset,
                       (GlobalPoint2D*)(d + pb));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d + pb, (size_t)n * sizeof(GlobalPoint2D), hipMemcpyDefault, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PP_OK;
}

// ---------------------------------------------------------------------------------------
int pp_set_profile(pp_handle h, int on)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    int r = drain_events(h); if (r) return r;
    h->profile = on < 0 ? 0 : (on > 2 ? 1 : on);
    return PP_OK;
}
int pp_get_kernel_ms(pp_handle h, int k, float* ms_total, int* launches)
{
    if (!h || k < 0 || k >= PP_K_COUNT) return fail(PP_ERR_ARG, "bad argument");
    int r = drain_events(h); if (r) return r;
    if (ms_total) *ms_total = h->k_ms[k];
    if (launches) *launches = h->k_launches[k];
    return PP_OK;
}
int pp_reset_kernel_ms(pp_handle h)
{
    if (!h) return fail(PP_ERR_ARG, "null handle");
    int r = drain_events(h); if (r) return r;
    for (int k = 0; k < PP_K_COUNT; k++) { h->k_ms[k] = 0; h->k_launches[k] = 0; }
    return PP_OK;
}
void* pp_device_ptr(pp_handle h, int which, size_t* bytes)
{
    if (!h) return nullptr;
    if (flush_group(h)) return nullptr;                   // the buffers of the last tick: its group's launches are enqueued
    const size_t ns = (size_t)h->caps.max_scenes;
    void* p = nullptr; size_t b = 0;
    switch (which) {
    case PP_BUF_SCENE_IN: p = h->cur_in().d_in; b = ns * sizeof(SceneIn); break;
    case PP_BUF_LANE_POOL: p = h->d_lane; b = (size_t)h->caps.max_lane_pts_total * sizeof(GlobalPoint3D); break;
    case PP_BUF_REF_POOL: p = h->d_ref; b = (size_t)h->caps.max_ref_pts_total * sizeof(GlobalPoint2D); break;
    case PP_BUF_OBS_POOL: p = h->cur_in().d_obs; b = (size_t)h->caps.max_obs_total * sizeof(ObPoint); break;
    case PP_BUF_MOT_POOL: p = h->cur_in().d_mot; b = (size_t)h->caps.max_obs_total * sizeof(ObMotion); break;
    case PP_BUF_STATE: p = h->d_state; b = ns * sizeof(SceneState); break;
    case PP_BUF_PLAN_OUT: p = h->plan_out(); b = ns * sizeof(PlanOut); break;
    case PP_BUF_GRID_OUT: p = h->d_gout[h->gout_set]; b = ns * sizeof(GridOut); break;      // the buffers of the last tick
    case PP_BUF_GRID: p = nullptr; b = 0; break;      // no occupancy grid is kept after a tick (the search builds it in LDS): use pp_get_grid
    case PP_BUF_PATH: p = h->d_path[h->path_set]; b = ns * (size_t)h->max_path0 * 4; break;
    case PP_BUF_LANE_ATTR: p = h->d_attr; b = (size_t)h->caps.max_lane_pts_total; break;
    case PP_BUF_OBS_NOW: p = h->d_obs_now[h->obs_set]; b = (size_t)h->caps.max_obs_total * sizeof(ObPoint); break;   // the last tick's snapshot
    case PP_BUF_OBS_SEEN: p = h->percept.d_seen[h->obs_set]; b = p ? (size_t)h->caps.max_obs_total * sizeof(ObPoint) : 0; break;   // ... and its perceived one (§4w)
    case PP_BUF_ORDER: p = h->d_order[h->parity] ? h->d_order[h->parity] + (size_t)h->item_off * h->caps.order_cap : nullptr; b = ns * (size_t)h->caps.order_cap * 4; break;
    default: break;
    }
    if (bytes) *bytes = b;
    return p;
}
// tick-group arithmetic (pp_plan_tick), without a device: the size of a group, the tick slots a handle allocates for, ring sizes,
// the LDS budget of a group's search (mode: bit 0 fixed budget, bit 1 dense forced)
int pp_tick_group_size(int n_scenes, int search_slots, int gcap, int forced) { return group_size(n_scenes, search_slots, gcap, forced); }
int pp_tick_group_cap(int max_scenes, int pipeline_min, int forced, size_t item_bytes) { return group_cap(max_scenes, pipeline_min, forced, item_bytes); }
int pp_tick_group_const(int which)
{
    switch (which) {
    case 0: return kGroupMax;
    case 1: return kBuf;
    case 2: return kRing;
    case 3: return kObs;
    case 4: return kGoutRing;
    case 5: return kGout;
    default: return -1;
    }
}
int pp_search_budget(int static_lds, int meta_bytes, int gbm_lds, int lds_budget_max, int n_cus, int n_scenes, int group, int n_obs_total,
                     int need, int budget, int from_need, int mode, int32_t* budget_out, int32_t* from_need_out, int32_t* slots_out)
{
    const dmpp::SearchBudget b = dmpp::search_budget((size_t)static_lds, meta_bytes, gbm_lds, lds_budget_max, n_cus, n_scenes, group, n_obs_total,
                                                     need, budget, from_need != 0, (mode & 1) != 0, (mode & 2) != 0);
    if (budget_out) *budget_out = b.budget;
    if (from_need_out) *from_need_out = b.from_need;
    if (slots_out) *slots_out = b.slots;
    return PP_OK;
}
int pp_coresident_budget(int static_lds, int meta_bytes, int gbm_lds, int lds_budget_max, int n_cus, int items, int need, int budget, int mode, int32_t* budget_out)
{
    if (!budget_out) return fail(PP_ERR_ARG, "null output");
    *budget_out = dmpp::coresident_budget((size_t)static_lds, meta_bytes, gbm_lds, lds_budget_max, n_cus, items, need, budget, (mode & 1) != 0, (mode & 2) != 0, kBesideSearchLds);
    return PP_OK;
}
// the rollout feature table (rollout_features.hpp), without a device: the feature bits a cause retires (-1: no such cause), and
// whether a set of features may be on together
int pp_feature_retires(int cause) { return cause >= 0 && cause < dmpp::kCauseCount ? (int)dmpp::retires(cause) : -1; }
int pp_feature_consistent(unsigned mask, int have_map, int resident_mode) { return dmpp::consistent(mask, have_map != 0, resident_mode) ? 1 : 0; }
void* pp_stream(pp_handle h) { return h && !flush_group(h) ? (void*)h->stream : nullptr; }

size_t pp_sizeof(int which)
{
    switch (which) {
    case 0: return sizeof(PlannerConfig); case 1: return sizeof(PlannerCaps); case 2: return sizeof(SceneIn);
    case 3: return sizeof(SceneState); case 4: return sizeof(PlanOut); case 5: return sizeof(GridOut);
    case 6: return sizeof(ObPoint); case 7: return sizeof(ObMotion); case 8: return sizeof(Path_Obs);
    case 9: return sizeof(LocationOut); case 10: return sizeof(DecisionOutPod); case 11: return sizeof(LaneView);
    case 12: return sizeof(PlanningOut); case 13: return sizeof(PlanningStatus); case 14: return sizeof(AimPoint);
    case 15: return sizeof(MapLane); case 16: return sizeof(MapJunction); case 17: return sizeof(MapDesc); case 18: return sizeof(PpSceneIo);
    case 19: return sizeof(EgoModel); case 20: return sizeof(EgoTrace); case 21: return sizeof(RolloutScore); case 22: return sizeof(FleetModel);
    case 23: return sizeof(RouteLeg); case 24: return sizeof(RouteModel); case 25: return sizeof(GridFollow);
    case 26: return sizeof(TrafficTrack); case 27: return sizeof(TrafficActor); case 28: return sizeof(TrafficFollow);
    case 29: return sizeof(EpisodeModel); case 30: return sizeof(EpisodeStats);
    case 31: return sizeof(EpisodeSpawn); case 32: return sizeof(EpisodeSpawnStats); case 33: return sizeof(TrafficStart);
    case 34: return sizeof(EpisodeRecord);
    case 35: return sizeof(ScoreTraceModel); case 36: return sizeof(ScoreTick); case 37: return sizeof(ScoreTraceInfo);
    case 38: return sizeof(EpisodeSchedule); case 39: return sizeof(EpisodeScheduleRow);
    case 40: return sizeof(EgoTracker); case 41: return sizeof(EgoTrackState);
    case 43: return sizeof(PackedPlan); case 44: return sizeof(PackedGrid);      // (42 stays unassigned)
    case 45: return sizeof(ConflictModel); case 46: return sizeof(ConflictScore);
    case 47: return sizeof(TrafficManoeuvre); case 48: return sizeof(TrafficManoeuvreState);
    case 50: return sizeof(PerceptionModel); case 51: return sizeof(PerceptTrack); case 52: return sizeof(PerceptionStats);      // (49 stays unassigned)
    default: return 0;
    }
}

}  // extern "C"
