// kernels_a.hpp — closed-loop rollout: k_advance_egos moves every ego along the path its last tick planned (DESIGN.md §4c;
// build-defined: the reference has no vehicle).  It is a device-generated update: it reads the SceneIn records the last tick
// read, that tick's PlanOut and the SceneState it left, and writes the SceneIn records of the next input set.
//
// One 64-lane wave per scene, four scenes per 256-thread block, no LDS, no barrier.  The lanes compute the lengths of the 64
// path segments ahead of k0 side by side; the sum is then taken in index order - by every lane alike, on values broadcast out
// of the lane that holds them, so the walk is wave-uniform and its rounding is that of a scalar loop - and stops at s (a
// handful of segments at 0.5 m spacing).  The three id searches are (value, index) wave minima that keep the first minimum
// (wave_first_min, the reduction of GetVhclLocalState in k_planning).  The steps are device functions and adv_scene holds them in
// §4c's order: the routed form of the kernel (k_advance_route, kernels_rt.hpp) is the same adv_scene with §4f at §4c 4. - 5.
// Both kernels are templates on kTrack: <false> puts the ego on its path (§4c 3., adv_speed_pose), <true> - a handle with an
// EgoTracker - moves it as a kinematic bicycle that chases the path (§4q, adv_speed_pose_tracked) and keeps one EgoTrackState per
// scene.  The two pose steps share the speed step (adv_speed) and the arc walk (adv_walk).
#pragma once
#include "dev_geom.hpp"

namespace dmpp {

constexpr int kAdvScenes = 4;          // scenes (waves) per block of k_advance_egos

__device__ __forceinline__ bool finite_f64(double v) { return __builtin_isfinite(v); }
// First index of the smallest squared distance to (x, y) over the points [max(id0, 0), min(id0 + window, n)) of one lane view (or
// junction polyline: P is GlobalPoint3D or GlobalPoint2D); a NaN distance is never the minimum.  idx < 0: no such point (the id
// keeps its value).  The result is the same in every lane.
template <class P>
__device__ __forceinline__ void wave_view_nearest(const P* __restrict__ pts, int n, int id0, int window, double x, double y,
                                                  int lane, double& best_d2, int& best_idx)
{
    const int lo = max(id0, 0);
    const long long hi_ll = (long long)id0 + (long long)window;
    const int hi = (int)(hi_ll < (long long)n ? hi_ll : (long long)n);
    double md = 0; int mi = -1;
    for (int i = lo + lane; i < hi; i += 64) {
        const double dx = pts[i].x - x, dy = pts[i].y - y;
        const double d = dx * dx + dy * dy;
        if (d == d && (mi < 0 || d < md)) { md = d; mi = i; }
    }
    wave_first_min(md, mi);
    best_d2 = md; best_idx = mi;
}

// The record travels as 32-bit words, one per lane: lane k holds word k of SceneIn[s] and stores word k of the new record, so
// every word is written once and nothing is indexed in registers.  loc.id[j] is word kIdWord + j, held by that lane.
constexpr int kSiWords = (int)(sizeof(SceneIn) / 4), kIdWord = (int)(offsetof(LocationOut, id) / 4), kLaneNumWord = (int)(offsetof(LocationOut, lane_num) / 4);
static_assert(sizeof(SceneIn) % 4 == 0 && kSiWords <= 64 && offsetof(SceneIn, loc) == 0, "SceneIn is moved as 32-bit words, one per lane");
static_assert(offsetof(LocationOut, globalpoint) == 0 && offsetof(LocationOut, velocity) == 24, "x, y, dir, velocity are words 0 .. 7");
__device__ __forceinline__ int adv_get_id(int w, int slot) { return __shfl(w, kIdWord + slot, 64); }      // (a shuffle: every lane takes part)
__device__ __forceinline__ void adv_set_id(int& w, int lane, int slot, int v) { if (lane == kIdWord + slot) w = v; }

// §4c 1. - 2.: the new speed (km/h) and the distance of this advance (m); the same in every lane
struct AdvSpeed { double v, vn, dist; };
__device__ __forceinline__ AdvSpeed adv_speed(const EgoModel& m, const SceneIn& si, const PlanOut& po)
{
    const PlanningOut& R = po.result;
    // 1. speed (km/h)
    const double v = si.loc.velocity;
    double vn;
    if (R.desaccVd) { vn = v + R.desacc * m.dt * 3.6; if (!(vn > 0)) vn = 0; }
    else {
        const double tgt = R.desspd;
        if (!finite_f64(tgt)) vn = v;
        else if (tgt > v) { vn = v + m.max_acc * m.dt * 3.6; if (vn > tgt) vn = tgt; }
        else { vn = v - m.max_dec * m.dt * 3.6; if (vn < tgt) vn = tgt; }
    }
    // 2. distance (m)
    AdvSpeed r; r.v = v; r.vn = vn; r.dist = 0.5 * (v + vn) / 3.6 * m.dt;
    return r;
}
// The arc walk of §4c 3. (and of the target of §4q 2.): the point d metres along the path from P[k0], the sum of the segment lengths
// taken in index order.  ran_out: no segment reached d, the point is P[199]; bad: a length that is not finite came first (nothing
// else is defined).  d <= 0 (or NaN): P[k0].  kDir: dir is GetRoadAngle of the segment the walk ended on - or, ran out, of the last
// one of non-zero length it passed - and dir0 where there is none.  The same in every lane.
struct AdvWalk { double x, y, dir; bool bad, ran_out; };
template <bool kDir>
__device__ __forceinline__ AdvWalk adv_walk(const PlannerConfig& c, const GlobalPoint2D* __restrict__ P, int k0, double dist, double dir0, int lane)
{
    double x = P[k0].x, y = P[k0].y, dir = dir0;
    bool bad = false, path_end = false;
    if (dist > 0) {
        double acc = 0; bool done = false; int last_seg = -1;
        for (int c0 = k0; c0 < DMPP_PATH_POINTS - 1 && !done && !bad; c0 += 64) {
            const int i = c0 + lane;
            double L = 0;
            if (i < DMPP_PATH_POINTS - 1) { const double dx = P[i + 1].x - P[i].x, dy = P[i + 1].y - P[i].y; L = sqrt(dx * dx + dy * dy); }
            const int cnt = min(64, DMPP_PATH_POINTS - 1 - c0);
            for (int j = 0; j < cnt; j++) {
                const double Lj = shfl_f64(L, j);
                if (!finite_f64(Lj)) { bad = true; break; }
                if (Lj == 0) continue;
                last_seg = c0 + j;
                if (acc + Lj >= dist) {
                    const GlobalPoint2D a = P[last_seg], b = P[last_seg + 1];
                    const double t = (dist - acc) / Lj;
                    x = a.x + t * (b.x - a.x); y = a.y + t * (b.y - a.y);
                    if constexpr (kDir) dir = GetRoadAngle(c, a, b);
                    done = true; break;
                }
                acc = acc + Lj;
            }
        }
        if (!bad && !done) {
            path_end = true;
            x = P[DMPP_PATH_POINTS - 1].x; y = P[DMPP_PATH_POINTS - 1].y;
            if constexpr (kDir) if (last_seg >= 0) dir = GetRoadAngle(c, P[last_seg], P[last_seg + 1]);
        }
    }
    AdvWalk r; r.x = x; r.y = y; r.dir = dir; r.bad = bad; r.ran_out = path_end;
    return r;
}
// (path_near_id is the ego's index on the path the tick LOCALISED on; a tick that replanned published a new path that starts at the ego)
__device__ __forceinline__ int adv_k0(const SceneState& st) { return st.afresh_planning ? 0 : clampi(st.path_near_id, 0, DMPP_PATH_POINTS - 1); }

// §4c 1. - 3.: the new speed and pose of one scene on its path (the same in every lane).  bad: BAD_PATH, nothing else is defined.
struct AdvPose { double x, y, dir, vn; bool bad, path_end; };
__device__ __forceinline__ AdvPose adv_speed_pose(const PlannerConfig& c, const EgoModel& m, const SceneIn& si, const PlanOut& po, const SceneState& st, int lane)
{
    const GlobalPoint2D* __restrict__ P = po.road_points;
    const AdvSpeed sp = adv_speed(m, si, po);
    // 3. pose: the ego is put on its path
    const int k0 = adv_k0(st);
    const GlobalPoint2D p0 = P[k0];
    AdvPose r; r.x = p0.x; r.y = p0.y; r.dir = si.loc.globalpoint.dir; r.vn = sp.vn; r.path_end = false;
    r.bad = !finite_f64(sp.dist) || !finite_f64(p0.x) || !finite_f64(p0.y);
    if (!r.bad) {
        const AdvWalk w = adv_walk<true>(c, P, k0, sp.dist, r.dir, lane);
        r.x = w.x; r.y = w.y; r.dir = w.dir; r.bad = w.bad; r.path_end = w.ran_out;
    }
    return r;
}

// ---- §4q: the tracked pose.  The ego keeps a pose of its own - (x, y) of its record, a unit heading and a curvature in its
// EgoTrackState - and chases the path by pure pursuit.  Every operand below is the same in all lanes of the wave; the arithmetic is
// + - * / sqrt (and floor, fabs) in the order §4q writes it, so every bit of the state and of x, y is the model's.
struct AdvTrack { EgoTracker tk; EgoTrackState* state; const EpisodeStats* ep; };       // ep: nullptr while episodes are off
template <bool kTrack> struct AdvTrackArg { using type = int; };                           // (<false>: one unused word)
template <> struct AdvTrackArg<true> { using type = AdvTrack; };
// §4q 1.: the unit heading of an angle in degrees by a fixed polynomial (no sin / cos call: their last bit is the library's)
__device__ __forceinline__ void trk_heading(double dir, double& hx, double& hy)
{
    hx = 1; hy = 0;
    if (!finite_f64(dir)) return;
    const double q = floor((dir + 45.0) / 90.0);
    const double r = dir - q * 90.0;
    const int qi = (int)(q - 4.0 * floor(q / 4.0));
    const double x = r * 0.017453292519943295;
    const double x2 = x * x;
    double ps = 2.8114572543455206e-15;
    ps = ps * x2 + -7.6471637318198164e-13;
    ps = ps * x2 + 1.6059043836821613e-10;
    ps = ps * x2 + -2.505210838544172e-08;
    ps = ps * x2 + 2.7557319223985893e-06;
    ps = ps * x2 + -0.00019841269841269841;
    ps = ps * x2 + 0.0083333333333333332;
    ps = ps * x2 + -0.16666666666666666;
    ps = ps * x2 + 1.0;
    const double sn = ps * x;
    double pc = 4.7794773323873853e-14;
    pc = pc * x2 + -1.1470745597729725e-11;
    pc = pc * x2 + 2.08767569878681e-09;
    pc = pc * x2 + -2.7557319223985888e-07;
    pc = pc * x2 + 2.4801587301587302e-05;
    pc = pc * x2 + -0.0013888888888888889;
    pc = pc * x2 + 0.041666666666666664;
    pc = pc * x2 + -0.5;
    pc = pc * x2 + 1.0;
    const double cs = pc;
    double ax, ay;
    if (qi == 0) { ax = cs; ay = sn; } else if (qi == 1) { ax = -sn; ay = cs; } else if (qi == 2) { ax = -cs; ay = -sn; } else { ax = sn; ay = -cs; }
    const double n = sqrt(ax * ax + ay * ay);
    hx = ax / n; hy = ay / n;
}
__device__ __forceinline__ unsigned long long f64_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
// §4q for one scene: speed and distance as §4c 1. - 2., then validity, target, steering, motion.  BAD_PATH: neither the record nor
// the state is touched.  Lane 0 stores the new state.
__device__ __forceinline__ AdvPose adv_speed_pose_tracked(const PlannerConfig& c, const EgoModel& m, const AdvTrack& a, const SceneIn& si, const PlanOut& po,
                                                          const SceneState& st, int s, int lane)
{
    const GlobalPoint2D* __restrict__ P = po.road_points;
    const EgoTracker& tk = a.tk;
    const AdvSpeed sp = adv_speed(m, si, po);
    const int k0 = adv_k0(st);
    const GlobalPoint2D p0 = P[k0];
    AdvPose r; r.x = si.loc.globalpoint.x; r.y = si.loc.globalpoint.y; r.dir = si.loc.globalpoint.dir; r.vn = sp.vn; r.path_end = false;
    r.bad = !finite_f64(sp.dist) || !finite_f64(p0.x) || !finite_f64(p0.y);
    if (r.bad) return r;
    // 2. the walk for s gives the flags of §4c 3. only; the target is the point ld metres along the path
    const AdvWalk ws = adv_walk<false>(c, P, k0, sp.dist, 0.0, lane);
    if (ws.bad) { r.bad = true; return r; }
    const double ld = tk.look_min + tk.look_gain * sp.vn / 3.6;
    const AdvWalk wt = adv_walk<false>(c, P, k0, ld, 0.0, lane);
    if (wt.bad || !finite_f64(wt.x) || !finite_f64(wt.y)) { r.bad = true; return r; }
    r.path_end = ws.ran_out;
    // 1. the state, re-derived when it is stale
    EgoTrackState S = a.state[s];
    const bool stale = S.valid == 0 || S.key_x != f64_bits(r.x) || S.key_y != f64_bits(r.y) || S.key_dir != f64_bits(r.dir) || (a.ep && a.ep[s].age == 0);
    if (stale) { trk_heading(r.dir, S.hx, S.hy); S.kappa = 0; S.n_init = S.n_init + 1; }
    // 3. steering: pure pursuit in curvature, clamped, rate-limited
    const double ex = wt.x - r.x, ey = wt.y - r.y;
    const double ly = ey * S.hx - ex * S.hy, d2 = ex * ex + ey * ey;
    double kc = 0;
    if (d2 != 0) kc = 2.0 * ly / d2;
    if (kc != kc) kc = 0;
    int sat = 0;
    if (kc >= tk.max_curv) { kc = tk.max_curv; sat = 1; }
    if (kc <= -tk.max_curv) { kc = -tk.max_curv; sat = 1; }
    const double dk = tk.curv_rate * m.dt, k_lo = S.kappa - dk, k_hi = S.kappa + dk;
    double kn = kc;
    if (kn > k_hi) kn = k_hi;
    if (kn < k_lo) kn = k_lo;
    S.kappa = kn; S.n_sat = S.n_sat + sat;
    const double ak = fabs(kn);
    if (ak > S.max_kappa) S.max_kappa = ak;
    const double ka = kn + tk.curv_bias;
    // 4. motion: n_sub substeps of half turn, move, half turn, renormalise
    double px = r.x, py = r.y, hx = S.hx, hy = S.hy;
    if (sp.dist > 0) {
        const double ds = sp.dist / (double)tk.n_sub;
        const double t = 0.25 * ka * ds, t2 = t * t, den = 1.0 + t2;
        const double rc = (1.0 - t2) / den, rs = 2.0 * t / den;
#pragma unroll 1
        for (int k = 0; k < tk.n_sub; k++) {
            const double mx = rc * hx - rs * hy, my = rs * hx + rc * hy;
            px = px + ds * mx; py = py + ds * my;
            const double nx = rc * mx - rs * my, ny = rs * mx + rc * my;
            const double n = sqrt(nx * nx + ny * ny);
            hx = nx / n; hy = ny / n;
        }
    }
    // 5. output
    GlobalPoint2D o, h; o.x = 0; o.y = 0; h.x = hx; h.y = hy;
    r.x = px; r.y = py; r.dir = GetRoadAngle(c, o, h);
    S.hx = hx; S.hy = hy; S.key_x = f64_bits(r.x); S.key_y = f64_bits(r.y); S.key_dir = f64_bits(r.dir); S.valid = 1; S._pad = 0;
    if (lane == 0) a.state[s] = S;
    return r;
}
__device__ __forceinline__ void adv_store_pose(int& w, int lane, const AdvPose& p)
{
    if (lane < 8) {
        const int q = lane >> 1;
        const double d = q == 0 ? p.x : q == 1 ? p.y : q == 2 ? p.dir : p.vn;
        w = (lane & 1) ? __double2hiint(d) : __double2loint(d);
    }
}

// §4c 4.: the localisation ids of the current, left and right view (the slots k_planning reads), searched from the ids the record
// words hold and written back into them.  i* < 0: the view is absent or has no nearest point.
struct AdvIds { double dc, dl, dr; int ic, il, ir; bool has_c; };
__device__ __forceinline__ AdvIds adv_search_ids(const GlobalPoint3D* __restrict__ lane_pool, const LaneView& lv, int ln, int window, double x, double y,
                                                 int lane, int& w)
{
    AdvIds r;
    r.has_c = ln >= 1 && ln <= DMPP_LANESUM && lv.cur_n > 0;
    const bool has_l = ln > 1 && ln - 2 < DMPP_LANESUM && lv.left_n > 0;
    const bool has_r = ln < lv.lane_sum && ln >= 0 && ln < DMPP_LANESUM && lv.right_n > 0;
    r.dc = 0; r.dl = 0; r.dr = 0; r.ic = -1; r.il = -1; r.ir = -1;
    if (r.has_c) wave_view_nearest(lane_pool + lv.cur_off, lv.cur_n, adv_get_id(w, ln - 1), window, x, y, lane, r.dc, r.ic);
    if (has_l) wave_view_nearest(lane_pool + lv.left_off, lv.left_n, adv_get_id(w, ln - 2), window, x, y, lane, r.dl, r.il);
    if (has_r) wave_view_nearest(lane_pool + lv.right_off, lv.right_n, adv_get_id(w, ln), window, x, y, lane, r.dr, r.ir);
    return r;
}
__device__ __forceinline__ void adv_store_ids(int& w, int lane, int ln, const AdvIds& r)
{
    if (r.ic >= 0) adv_set_id(w, lane, ln - 1, r.ic);
    if (r.il >= 0) adv_set_id(w, lane, ln - 2, r.il);
    if (r.ir >= 0) adv_set_id(w, lane, ln, r.ir);
}
// §4c 5.: the lane number the nearest points give (the current view has one: r.ic >= 0)
__device__ __forceinline__ int adv_lane_number(const LaneView& lv, int ln, const AdvIds& r)
{
    const double margin = 0.25 * lv.lane_width, rc = sqrt(r.dc);
    if (r.il >= 0 && rc - sqrt(r.dl) > margin) return ln - 1;
    if (r.ir >= 0 && rc - sqrt(r.dr) > margin) return ln + 1;
    return ln;
}
// §4c 6.: the grid does not follow the ego (a handle without a GridFollow model; with one: adv_follow_grid below)
__device__ __forceinline__ bool adv_off_grid(const PlannerConfig& c, const SceneIn& si, double x, double y)
{
    const double fx = floor((x - si.grid_origin.x) / c.cell), fy = floor((y - si.grid_origin.y) / c.cell);
    return !(fx >= 0 && fx < (double)c.grid_w && fy >= 0 && fy < (double)c.grid_h);
}
// §4g: the grid follows the ego.  In the place of §4c 6. for a handle with a GridFollow model (gf.goal_point > 0): the goal becomes
// point gf.goal_point of the path the advance followed and the frame is held, or re-centred on whole cells about the midpoint of
// ego and goal; the eight words of grid_origin and goal are replaced in the lanes that hold them, OFF_GRID is tested on the new
// frame.  A non-finite goal point skips the step: the frame is carried over and tested as in §4c 6.  Every operand is the same
// in all lanes.  Returns the OFF_GRID verdict.
constexpr int kOriginWord = (int)(offsetof(SceneIn, grid_origin) / 4), kGoalWord = (int)(offsetof(SceneIn, goal) / 4);
static_assert(offsetof(SceneIn, grid_origin) % 8 == 0 && kGoalWord == kOriginWord + 4 && kGoalWord + 4 <= kSiWords && sizeof(GlobalPoint2D) == 16,
              "origin.x, origin.y, goal.x, goal.y are the eight words from kOriginWord, each double on an even word");
__device__ __forceinline__ bool adv_follow_grid(const PlannerConfig& c, const GridFollow& gf, const SceneIn& si, const PlanOut& po, double x, double y,
                                                int lane, int& w)
{
    GlobalPoint2D o = si.grid_origin;
    const GlobalPoint2D g = po.road_points[gf.goal_point];
    if (finite_f64(g.x) && finite_f64(g.y)) {
        const double lo = (double)gf.margin_cells, hx = (double)(c.grid_w - gf.margin_cells), hy = (double)(c.grid_h - gf.margin_cells);
        const double ex = floor((x - o.x) / c.cell), gx = floor((g.x - o.x) / c.cell);
        const double ey = floor((y - o.y) / c.cell), gy = floor((g.y - o.y) / c.cell);
        const bool hold = lo <= ex && ex < hx && lo <= gx && gx < hx && lo <= ey && ey < hy && lo <= gy && gy < hy;      // (a NaN: not held)
        if (!hold) {
            const double mx = 0.5 * (x + g.x), my = 0.5 * (y + g.y);
            o.x = (floor(mx / c.cell) - (double)(c.grid_w / 2)) * c.cell;
            o.y = (floor(my / c.cell) - (double)(c.grid_h / 2)) * c.cell;
        }
        if (lane >= kOriginWord && lane < kOriginWord + 8) {
            const int q = (lane - kOriginWord) >> 1;
            const double d = q == 0 ? o.x : q == 1 ? o.y : q == 2 ? g.x : g.y;
            w = (lane & 1) ? __double2hiint(d) : __double2loint(d);
        }
    }
    if (!c.grid_stage) return false;
    const double fx = floor((x - o.x) / c.cell), fy = floor((y - o.y) / c.cell);
    return !(fx >= 0 && fx < (double)c.grid_w && fy >= 0 && fy < (double)c.grid_h);
}
__device__ __forceinline__ void adv_store_trace(EgoTrace* __restrict__ trace, int s, int lane, int w, int ln_new, int f)
{                                                       // (shuffles: every lane takes part)
    const int id_cur = adv_get_id(w, clampi(ln_new - 1, 0, DMPP_LANESUM - 1));
    const double tx = __hiloint2double(__shfl(w, 1, 64), __shfl(w, 0, 64)), ty = __hiloint2double(__shfl(w, 3, 64), __shfl(w, 2, 64));
    const double td = __hiloint2double(__shfl(w, 5, 64), __shfl(w, 4, 64)), tv = __hiloint2double(__shfl(w, 7, 64), __shfl(w, 6, 64));
    if (lane == 0) {
        EgoTrace t;
        t.pose.x = tx; t.pose.y = ty; t.pose.dir = td; t.velocity = tv;
        t.id_cur = id_cur; t.lane_num = ln_new; t.flags = f; t._pad = 0;
        trace[s] = t;
    }
}
// §4c 4.: the search window from id idc reaches the end of the current view
__device__ __forceinline__ bool adv_lane_ends(const LaneView& lv, int idc, int window) { return (long long)idc + window >= (long long)lv.cur_n; }
// §4c 4. - 5. for a scene that follows no route: ids, LANE_END, lane number
__device__ __forceinline__ void adv_lane_step(const GlobalPoint3D* __restrict__ lane_pool, const LaneView& lv, int ln, int window, int map_mode,
                                              double x, double y, int lane, int& w, int& f, int& ln_new)
{
    const AdvIds r = adv_search_ids(lane_pool, lv, ln, window, x, y, lane, w);
    if (r.has_c) {
        const int idc = r.ic >= 0 ? r.ic : adv_get_id(w, ln - 1);
        if (adv_lane_ends(lv, idc, window)) f |= DMPP_EGO_LANE_END;
    }
    adv_store_ids(w, lane, ln, r);
    // 5. lane number: only on a resident map, where k_resolve_map derives the new views
    if (map_mode && r.ic >= 0) {
        ln_new = adv_lane_number(lv, ln, r);
        if (lane == kLaneNumWord) w = ln_new;
    }
}

// One scene of an advance, §4c from the record load to the flag word: the frame k_advance_egos and k_advance_route share.  step(s, si,
// ln, p, lane, w, f, ln_new) is what stands at §4c 4. - 5.: ids, LANE_END and lane number at the new pose p.  kTrack: the pose step is
// §4q's (a handle with an EgoTracker); <false> is the kernel of a handle without one and takes one unused word.
template <bool kTrack, class Step>
__device__ __forceinline__ void adv_scene(const PlannerConfig& c, const EgoModel& m, const GridFollow& gf, int n_scenes, const SceneIn* __restrict__ in,
                                          SceneIn* __restrict__ out, const PlanOut* __restrict__ plan, const SceneState* __restrict__ state,
                                          int32_t* __restrict__ flags, EgoTrace* __restrict__ trace, const typename AdvTrackArg<kTrack>::type& trk, Step step)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * kAdvScenes + (threadIdx.x >> 6);
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    const SceneIn& si = in[s];
    int w = lane < kSiWords ? reinterpret_cast<const int*>(&si)[lane] : 0;
    const int f_in = flags[s];
    const int ln = si.loc.lane_num;
    int f = f_in, ln_new = ln;
    if (f_in == 0) {
        AdvPose p;
        if constexpr (kTrack) p = adv_speed_pose_tracked(c, m, trk, si, plan[s], state[s], s, lane);
        else p = adv_speed_pose(c, m, si, plan[s], state[s], lane);
        if (p.bad) f |= DMPP_EGO_BAD_PATH;
        else {
            if (p.path_end) f |= DMPP_EGO_PATH_END;
            adv_store_pose(w, lane, p);
            step(s, si, ln, p, lane, w, f, ln_new);
            if (gf.goal_point > 0 ? adv_follow_grid(c, gf, si, plan[s], p.x, p.y, lane, w) : (c.grid_stage && adv_off_grid(c, si, p.x, p.y)))
                f |= DMPP_EGO_OFF_GRID;
        }
    }
    if (lane < kSiWords) reinterpret_cast<int*>(&out[s])[lane] = w;
    if (trace) adv_store_trace(trace, s, lane, w, ln_new, f);
    if (lane == 0) flags[s] = f;
}

template <bool kTrack>
__global__ void __launch_bounds__(kBlock)
k_advance_egos(PlannerConfig c, EgoModel m, GridFollow gf, int n_scenes, int map_mode, const SceneIn* __restrict__ in, SceneIn* __restrict__ out,
               const PlanOut* __restrict__ plan, const SceneState* __restrict__ state, const GlobalPoint3D* __restrict__ lane_pool,
               int32_t* __restrict__ flags, EgoTrace* __restrict__ trace, typename AdvTrackArg<kTrack>::type trk)
{
    adv_scene<kTrack>(c, m, gf, n_scenes, in, out, plan, state, flags, trace, trk,
                      [&](int, const SceneIn& si, int ln, const AdvPose& p, int lane, int& w, int& f, int& ln_new) {
                          adv_lane_step(lane_pool, si.lanes, ln, m.window, map_mode, p.x, p.y, lane, w, f, ln_new);
                      });
}

// h_bad slot reset in stream order (pp_update_async on top of an update already staged: see the owner rule there)
__global__ void k_zero_word(int32_t* p) { *p = 0; }

}  // namespace dmpp
