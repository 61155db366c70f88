// kernels_sc.hpp — rollout scorecard (build-defined): per-scene safety and progress totals folded on the
// device over the scored ticks, so that a closed-loop rollout can be judged without fetching every tick.
//
//   k_score_ego   : the front half.  One 64-lane wave per scene, four scenes per 256-thread block, no LDS, no barrier (the
//                   shape of k_advance_egos).  The lanes stride over the scene's records of the tick's obstacle snapshot; the
//                   smallest distance is a (value, index) wave minimum that keeps the first minimum (wave_first_min); lane 0
//                   folds the scalars into the record.  Reads SceneIn_t, PlanOut_t, SceneState after tick t, the snapshot of
//                   tick t and the ego flag word; writes the front half of RolloutScore.
//                   <., ., true>, while the conflict score is on (§4u): in the same loop every lane differences the entries it reads
//                   against the snapshot of the scored tick before and stores them for the next one; one more wave_first_min and a
//                   wave maximum give the tick's smallest time to collision and largest braking demand, which lane 0 folds into
//                   the scene's ConflictScore in front of the trace and the fold.
//   k_score_grid  : the grid half.  One thread per scene: the header of GridOut_t into a ScoreGridPart.  The searches of
//                   consecutive ticks run on kBuf streams side by side, so every search stream counts into a part array of
//                   its own (stream order serialises its ticks) and pp_get_rollout_score adds the parts into the records.
//   k_score_reset : the starting values (+inf, -1: not all zero bits).
//   score_fold    : steps 2. - 4. of §4d on one record: k_score_ego applies it to the scene's RolloutScore and - k_score_ego<true>,
//                   while the episode log is on (§4n) - to the scorecard of the scene's running episode.
#pragma once
#include "dev_geom.hpp"

namespace dmpp {

constexpr int kScScenes = 4;           // scenes (waves) per block of k_score_ego

struct ScoreGridPart { int32_t n_grid_ticks, n_grid_path_candidate, status[DMPP_G_STATUS_COUNT]; };

// §4d 0.: the starting values of a record
__device__ __forceinline__ RolloutScore score_start()
{
    RolloutScore r;
    r.min_clearance = __builtin_huge_val(); r.dist = 0; r.max_speed = 0; r.max_acc = 0; r.max_dec = 0;
    r.last_pos.x = 0; r.last_pos.y = 0; r.last_speed = 0;
    r.n_ticks = 0; r.min_clearance_tick = -1; r.min_clearance_obs = -1; r.first_collision_tick = -1; r.n_collision_ticks = 0;
    r.n_replans = 0; r.n_ob_flag = 0; r.n_desacc = 0;
    for (int k = 0; k < 8; k++) r.behavior_ticks[k] = 0;
    r.ego_flags = 0; r._pad = 0; r.n_grid_ticks = 0; r.n_grid_path_candidate = 0;
    for (int k = 0; k < DMPP_G_STATUS_COUNT; k++) r.grid_status_ticks[k] = 0;
    return r;
}

__global__ void __launch_bounds__(kBlock)
k_score_reset(int n_scenes, RolloutScore* __restrict__ score)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_scenes) return;
    score[s] = score_start();
}

// §4d 2. - 4.: one scored tick of scene s folded into record s of `score` (lane 0 of the scene's wave).  x, y, v: the ego of the tick;
// (md, mi): its nearest obstacle edge, mi < 0 without one; plan, state, flags: as k_score_ego.
__device__ __forceinline__ void score_fold(RolloutScore* __restrict__ score, int s, double x, double y, double v, double md, int mi, double half_width, double dt_score,
                                           const PlanOut* __restrict__ plan, const SceneState* __restrict__ state, const int32_t* __restrict__ flags)
{
    RolloutScore& r = score[s];
    const int k = r.n_ticks;                            // this tick's index among the scored ones
    // 2. clearance and collisions
    if (mi >= 0) {
        const double cl = md - half_width;
        if (cl < r.min_clearance) { r.min_clearance = cl; r.min_clearance_tick = k; r.min_clearance_obs = mi; }
        if (cl <= 0) {
            if (r.first_collision_tick < 0) r.first_collision_tick = k;
            r.n_collision_ticks = r.n_collision_ticks + 1;
        }
    }
    // 3. distance and speed against the ego of the tick before
    if (k > 0) {
        const double dx = x - r.last_pos.x, dy = y - r.last_pos.y;
        r.dist = r.dist + sqrt(dx * dx + dy * dy);
        const double a = (v - r.last_speed) / 3.6 / dt_score, fall = -a;
        if (a > r.max_acc) r.max_acc = a;
        if (fall > r.max_dec) r.max_dec = fall;
    }
    if (v > r.max_speed) r.max_speed = v;
    r.last_pos.x = x; r.last_pos.y = y; r.last_speed = v;
    // 4. counters of the tick's plan
    const PlanOut& po = plan[s];
    if (state[s].afresh_planning != 0) r.n_replans = r.n_replans + 1;
    if (po.ob_flag != 0) r.n_ob_flag = r.n_ob_flag + 1;
    if (po.result.desaccVd != 0) r.n_desacc = r.n_desacc + 1;
    const int b = clampi(po.dec.behavior, 0, 7);
    r.behavior_ticks[b] = r.behavior_ticks[b] + 1;
    r.ego_flags = flags ? flags[s] : 0;
    r.n_ticks = k + 1;
}

// §4o: the headers of the score trace at their starting values (armed, nothing written, no triggering tick)
__global__ void __launch_bounds__(kBlock)
k_score_trace_reset(int n_scenes, ScoreTraceInfo* __restrict__ info)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_scenes) return;
    ScoreTraceInfo hd;
    hd.n_written = 0; hd.state = 0; hd.trigger_k = -1; hd.trigger = 0; hd.post_left = 0; hd.n_trigger_ticks = 0; hd._pad[0] = 0; hd._pad[1] = 0;
    info[s] = hd;
}

static_assert(sizeof(ScoreTick) == 64 && offsetof(ScoreTick, k) == 0 && offsetof(ScoreTick, flags) == 4 && offsetof(ScoreTick, tick) == 8 && offsetof(ScoreTick, x) == 16 &&
              offsetof(ScoreTick, y) == 24 && offsetof(ScoreTick, v) == 32 && offsetof(ScoreTick, clearance) == 40 && offsetof(ScoreTick, obs) == 48 &&
              offsetof(ScoreTick, ob_type) == 52 && offsetof(ScoreTick, behavior) == 56 && offsetof(ScoreTick, marks) == 60, "ScoreTick layout (DESIGN.md §4o)");
static_assert(sizeof(ScoreTraceModel) == 32 && sizeof(ScoreTraceInfo) == 32, "ScoreTraceModel / ScoreTraceInfo layout (DESIGN.md §4o)");
typedef unsigned int TickPiece __attribute__((ext_vector_type(4)));        // (a native vector: one 16-byte store, which the compiler does not take apart)
struct TickPieces { TickPiece p[4]; };
static_assert(sizeof(TickPieces) == sizeof(ScoreTick), "the pieces of a record");

// §4o 1. - 4.: one scored tick of scene s into its ring and header (lane 0 of the scene's wave), IN FRONT of score_fold: k and last_speed
// are those of record s of `score` before the fold.  x, y, v, (md, mi), plan, state, flags: as score_fold; ob_type: the type of the
// snapshot entry mi names (0 without one); ep_stats: EpisodeStats while episodes are on, else null.
__device__ __forceinline__ void trace_step(const ScoreTraceModel& tm, ScoreTraceInfo* __restrict__ info, ScoreTick* __restrict__ ring, long long tick,
                                           const EpisodeStats* __restrict__ ep_stats, const RolloutScore* __restrict__ score, int s, double x, double y, double v,
                                           double md, int mi, int ob_type, double half_width, double dt_score, const PlanOut* __restrict__ plan,
                                           const SceneState* __restrict__ state, const int32_t* __restrict__ flags)
{
    // 1. the record
    const PlanOut& po = plan[s];
    ScoreTick R;
    R.k = score[s].n_ticks; R.flags = flags ? flags[s] : 0; R.tick = tick; R.x = x; R.y = y; R.v = v;
    R.clearance = mi >= 0 ? md - half_width : __builtin_huge_val();
    R.obs = mi >= 0 ? mi : -1; R.ob_type = mi >= 0 ? ob_type : 0;
    R.behavior = po.dec.behavior;
    int marks = 0;
    if (state[s].afresh_planning != 0) marks |= DMPP_TICK_REPLAN;
    if (po.ob_flag != 0) marks |= DMPP_TICK_OB_FLAG;
    if (po.result.desaccVd != 0) marks |= DMPP_TICK_DESACC;
    if (ep_stats && ep_stats[s].age == 0) marks |= DMPP_TICK_START;
    // 2. the cause word: a NaN compares false everywhere
    int c = 0;
    if (mi >= 0 && R.clearance <= 0) c |= DMPP_TRACE_COLLISION;
    if (mi >= 0 && R.clearance <= tm.near) c |= DMPP_TRACE_NEAR;
    if ((R.flags & tm.flag_mask) != 0) c |= DMPP_TRACE_FLAG;
    if (R.k > 0) {
        const double a = (v - score[s].last_speed) / 3.6 / dt_score, fall = -a;
        if (fall >= tm.brake) c |= DMPP_TRACE_BRAKE;
    }
    c &= tm.trigger;
    R.marks = marks | (c << 8);
    // 3., 4. the header and the ring
    ScoreTraceInfo hd = info[s];
    if (c != 0) hd.n_trigger_ticks = hd.n_trigger_ticks + 1;
    if (hd.state != 2) {
        // 64 B divide into four 16-byte pieces, and a device allocation starts on a 16-byte boundary: so does every record
        const TickPieces q = __builtin_bit_cast(TickPieces, R);
        // (unsigned: the slot stays inside the scene's ring whatever the header holds)
        TickPiece* dst = reinterpret_cast<TickPiece*>(ring + ((size_t)s * (size_t)tm.depth + (size_t)((unsigned)hd.n_written % (unsigned)tm.depth)));
#pragma unroll
        for (int i = 0; i < 4; i++) dst[i] = q.p[i];
        hd.n_written = hd.n_written + 1;
        if (hd.state == 0 && c != 0) { hd.trigger_k = R.k; hd.trigger = c; hd.post_left = tm.post; hd.state = tm.post > 0 ? 1 : 2; }
        else if (hd.state == 1) { hd.post_left = hd.post_left - 1; if (hd.post_left == 0) hd.state = 2; }
    }
    info[s] = hd;
}

// ---- conflict score ---------------------------------------------------------------------------------------------
static_assert(sizeof(ConflictModel) == 32 && sizeof(ConflictScore) == 88 && offsetof(ConflictScore, min_ttc) == 0 && offsetof(ConflictScore, max_drac) == 8 &&
              offsetof(ConflictScore, tit_warn) == 16 && offsetof(ConflictScore, last_pos) == 24 && offsetof(ConflictScore, n_ticks) == 40 &&
              offsetof(ConflictScore, n_conflict_ticks) == 44 && offsetof(ConflictScore, n_warn_ticks) == 48 && offsetof(ConflictScore, n_crit_ticks) == 52 &&
              offsetof(ConflictScore, min_ttc_tick) == 56 && offsetof(ConflictScore, min_ttc_obs) == 60 && offsetof(ConflictScore, min_ttc_type) == 64 &&
              offsetof(ConflictScore, first_crit_tick) == 68 && offsetof(ConflictScore, max_drac_tick) == 72 && offsetof(ConflictScore, n_no_history_ticks) == 76 &&
              offsetof(ConflictScore, prev_off) == 80 && offsetof(ConflictScore, prev_n) == 84 && sizeof(ConflictScore) % 8 == 0, "ConflictModel / ConflictScore layout (DESIGN.md §4u)");

// §4u 0.: the starting values of the records.  prev_n = 0: the previous-snapshot buffers need not be cleared.
__global__ void __launch_bounds__(kBlock)
k_conflict_reset(int n_scenes, ConflictScore* __restrict__ cs)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_scenes) return;
    ConflictScore r;
    r.min_ttc = __builtin_huge_val(); r.max_drac = 0; r.tit_warn = 0; r.last_pos.x = 0; r.last_pos.y = 0;
    r.n_ticks = 0; r.n_conflict_ticks = 0; r.n_warn_ticks = 0; r.n_crit_ticks = 0;
    r.min_ttc_tick = -1; r.min_ttc_obs = -1; r.min_ttc_type = 0; r.first_crit_tick = -1; r.max_drac_tick = -1; r.n_no_history_ticks = 0;
    r.prev_off = 0; r.prev_n = 0;
    cs[s] = r;
}

// §4u 1.: what every lane of the scene's wave needs of the ego before the loop (the same loads on every lane)
struct ConflictEgo { bool ok; double ux, uy, lim; int prev_n; };
__device__ __forceinline__ ConflictEgo conflict_ego(const ConflictModel& cm, const ConflictScore& C, const EpisodeStats* __restrict__ ep_stats, int s, double x, double y,
                                                    int off, double dt)
{
    ConflictEgo e;
    const bool hist = C.n_ticks > 0 && !(ep_stats && ep_stats[s].age == 0);
    const double ex = x - C.last_pos.x, ey = y - C.last_pos.y;
    e.lim = cm.v_max * dt;
    e.ok = hist && sqrt(ex * ex + ey * ey) <= e.lim;
    e.ux = ex / dt; e.uy = ey / dt;
    e.prev_n = C.prev_off == off ? C.prev_n : 0;        // (a moved slice: no entry has a velocity)
    return e;
}

// §4u 2.: entry j of the slice, o now and p one scored tick ago, against the ego (x, y) with velocity (ux, uy).  Returns whether the entry
// has a TTC; drac stays 0 without one.  R = radius + half_width.
__device__ __forceinline__ bool conflict_entry(const ConflictModel& cm, const ConflictEgo& e, const ObPoint& o, const ObPoint& p, double x, double y, double half_width, double dt,
                                               double& ttc, double& drac)
{
    drac = 0;
    const double gx = o.x - p.x, gy = o.y - p.y;
    if (!(p.type == o.type && p.radius == o.radius && sqrt(gx * gx + gy * gy) <= e.lim)) return false;
    const double px = o.x - x, py = o.y - y;
    const double wx = gx / dt - e.ux, wy = gy / dt - e.uy;
    const double R = (double)o.radius + half_width;
    const double q = px * px + py * py, c = q - R * R;
    if (c <= 0) { ttc = 0; return true; }               // in contact: a TTC whatever w is, no DRAC
    const double dist = sqrt(q), b = px * wx + py * wy, vc = (-b) / dist;
    if (!(vc > cm.min_closing)) return false;
    const double a = wx * wx + wy * wy, disc = b * b - a * c;
    if (!(disc >= 0)) return false;                     // a miss
    ttc = c / ((-b) + sqrt(disc));                      // the root without cancellation
    const double gap = dist - R;
    if (gap > 0) drac = vc * vc / (2 * gap);
    return true;
}

// §4u 4., 5.: the tick folded into record s (lane 0 of the scene's wave), IN FRONT of trace_step / score_fold.  (tt, ti): the smallest TTC
// and its first index, ti < 0 without one; dd: the largest DRAC; ob_type: the type of entry ti.
__device__ __forceinline__ void conflict_fold(const ConflictModel& cm, ConflictScore* __restrict__ cs, int s, bool ego_ok, double x, double y, int off, int m,
                                              double tt, int ti, double dd, int ob_type, double dt)
{
    ConflictScore& C = cs[s];
    const int k = C.n_ticks;
    if (k > 0 && !ego_ok) C.n_no_history_ticks = C.n_no_history_ticks + 1;
    if (ti >= 0) {
        C.n_conflict_ticks = C.n_conflict_ticks + 1;
        if (tt < C.min_ttc) { C.min_ttc = tt; C.min_ttc_tick = k; C.min_ttc_obs = ti; C.min_ttc_type = ob_type; }
        if (tt <= cm.ttc_warn) { C.n_warn_ticks = C.n_warn_ticks + 1; C.tit_warn = C.tit_warn + (cm.ttc_warn - tt) * dt; }
        if (tt <= cm.ttc_crit) { C.n_crit_ticks = C.n_crit_ticks + 1; if (C.first_crit_tick == -1) C.first_crit_tick = k; }
        if (dd > C.max_drac) { C.max_drac = dd; C.max_drac_tick = k; }
    }
    C.last_pos.x = x; C.last_pos.y = y; C.prev_off = off; C.prev_n = m; C.n_ticks = k + 1;
}

// obs_cap: entries of a snapshot set; a slice outside it (no set call and no update lets one through) counts as empty.
// kLog: the episode log is on and the tick is folded a second time, into the scorecard of the scene's running
// episode, ep_score[s]; without it ep_score is null and never read.
// kTrace: the score trace is on and lane 0 stores the tick's record into the scene's ring in front of the fold; without
// it tick, tm, ep_stats, tinfo and tring are never read, and the kernel is the one without them.
// kConflict: the conflict score is on: every lane differences the entries it reads against `prev`, the snapshot of the
// scored tick before (indexed inside the slice checked against obs_cap only; both buffers hold caps.max_obs_total >= obs_cap entries),
// and stores them into `prev_next`, which the next scored tick reads - two buffers, so that no scene reads an entry that a scene with
// an overlapping slice has already stored; lane 0 folds the tick into cscore[s] in front of the trace and the fold.  Without it cm,
// cscore, prev and prev_next are never read (and ep_stats only by the trace).
template <bool kLog, bool kTrace, bool kConflict>
__global__ void __launch_bounds__(kBlock)
k_score_ego(double half_width, double dt_score, int n_scenes, int obs_cap, const SceneIn* __restrict__ in, const PlanOut* __restrict__ plan,
            const SceneState* __restrict__ state, const ObPoint* __restrict__ now, const int32_t* __restrict__ flags,
            RolloutScore* __restrict__ score, RolloutScore* __restrict__ ep_score,
            long long tick, ScoreTraceModel tm, const EpisodeStats* __restrict__ ep_stats, ScoreTraceInfo* __restrict__ tinfo, ScoreTick* __restrict__ tring,
            ConflictModel cm, ConflictScore* __restrict__ cscore, const ObPoint* __restrict__ prev, ObPoint* __restrict__ prev_next)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * kScScenes + (threadIdx.x >> 6);
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    const SceneIn& si = in[s];
    const double x = si.loc.globalpoint.x, y = si.loc.globalpoint.y, v = si.loc.velocity;
    const int off = si.obs_off;
    int m = si.obs_n;
    if (off < 0 || m < 0 || (long long)off + (long long)m > (long long)obs_cap) m = 0;
    // 1. the nearest obstacle edge: first index of the smallest d_j, a NaN is never the minimum
    double md = 0; int mi = -1;
    ConflictEgo ce = {};
    if (kConflict) ce = conflict_ego(cm, cscore[s], ep_stats, s, x, y, off, dt_score);
    double tt = 0, dd = 0; int ti = -1;                 // §4u 3.: smallest TTC with its first index, largest DRAC
    for (int j = lane; j < m; j += 64) {
        const ObPoint o = now[off + j];
        const double dx = o.x - x, dy = o.y - y;
        const double d = sqrt(dx * dx + dy * dy) - (double)o.radius;
        if (d == d && (mi < 0 || d < md)) { md = d; mi = j; }
        if (kConflict) {
            if (ce.ok && j < ce.prev_n) {
                const ObPoint p = prev[off + j];
                double t, dr;
                if (conflict_entry(cm, ce, o, p, x, y, half_width, dt_score, t, dr)) {
                    if (t == t && (ti < 0 || t < tt)) { tt = t; ti = j; }
                    if (dr > dd) dd = dr;
                }
            }
            prev_next[off + j] = o;
        }
    }
    wave_first_min(md, mi);
    if (kConflict) {
        wave_first_min(tt, ti);
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) { const double o_d = shfl_xor_f64(dd, sft); if (o_d > dd) dd = o_d; }
    }
    if (lane != 0) return;
    if (kConflict) conflict_fold(cm, cscore, s, ce.ok, x, y, off, m, tt, ti, dd, ti >= 0 ? now[off + ti].type : 0, dt_score);
    if (kTrace) trace_step(tm, tinfo, tring, tick, ep_stats, score, s, x, y, v, md, mi, mi >= 0 ? now[off + mi].type : 0, half_width, dt_score, plan, state, flags);
    score_fold(score, s, x, y, v, md, mi, half_width, dt_score, plan, state, flags);
    if (kLog) score_fold(ep_score, s, x, y, v, md, mi, half_width, dt_score, plan, state, flags);
}

__global__ void __launch_bounds__(kBlock)
k_score_grid(int n_scenes, int n_lattice, const GridOut* __restrict__ gout, ScoreGridPart* __restrict__ part)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_scenes) return;
    const GridOut& g = gout[s];
    ScoreGridPart& p = part[s];
    int st = g.status;
    if (st < 0 || st >= DMPP_G_STATUS_COUNT) st = DMPP_G_INTERNAL;
    p.n_grid_ticks = p.n_grid_ticks + 1;
    p.status[st] = p.status[st] + 1;
    const int nc = g.n_candidates;
    if (nc == n_lattice + 1 && g.best_candidate == nc - 1) p.n_grid_path_candidate = p.n_grid_path_candidate + 1;
}

}  // namespace dmpp
