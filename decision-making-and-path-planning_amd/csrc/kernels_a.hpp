// kernels_a.hpp — closed-loop rollout: k_advance_egos moves every ego along the path its last tick planned (DESIGN.md §4c;
// build-defined: the reference has no vehicle).  It is a device-generated update: it reads the SceneIn records the last tick
// read, that tick's PlanOut and the SceneState it left, and writes the SceneIn records of the next input set.
//
// One 64-lane wave per scene, four scenes per 256-thread block, no LDS, no barrier.  The lanes compute the lengths of the 64
// path segments ahead of k0 side by side; the sum is then taken in index order - by every lane alike, on values broadcast out
// of the lane that holds them, so the walk is wave-uniform and its rounding is that of a scalar loop - and stops at s (a
// handful of segments at 0.5 m spacing).  The three id searches are (value, index) wave minima that keep the first minimum
// (wave_first_min, the reduction of GetVhclLocalState in k_planning).
#pragma once
#include "dev_geom.hpp"

namespace dmpp {

constexpr int kAdvScenes = 4;          // scenes (waves) per block of k_advance_egos

__device__ __forceinline__ bool finite_f64(double v) { return __builtin_isfinite(v); }
// First index of the smallest squared distance to (x, y) over the points [max(id0, 0), min(id0 + window, n)) of one lane view;
// a NaN distance is never the minimum.  idx < 0: no such point (the id keeps its value).  The result is the same in every lane.
__device__ __forceinline__ void wave_view_nearest(const GlobalPoint3D* __restrict__ pts, int n, int id0, int window, double x, double y,
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

__global__ void __launch_bounds__(kBlock)
k_advance_egos(PlannerConfig c, EgoModel m, int n_scenes, int map_mode, const SceneIn* __restrict__ in, SceneIn* __restrict__ out,
               const PlanOut* __restrict__ plan, const SceneState* __restrict__ state, const GlobalPoint3D* __restrict__ lane_pool,
               int32_t* __restrict__ flags, EgoTrace* __restrict__ trace)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * kAdvScenes + (threadIdx.x >> 6);
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    const SceneIn& si = in[s];
    // The record travels as 32-bit words, one per lane: lane k holds word k of SceneIn[s] and stores word k of the new record, so
    // every word is written once and nothing is indexed in registers.  loc.id[j] is word kIdWord + j, held by that lane.
    constexpr int kWords = (int)(sizeof(SceneIn) / 4), kIdWord = (int)(offsetof(LocationOut, id) / 4), kLaneNumWord = (int)(offsetof(LocationOut, lane_num) / 4);
    static_assert(sizeof(SceneIn) % 4 == 0 && kWords <= 64 && offsetof(SceneIn, loc) == 0, "SceneIn is moved as 32-bit words, one per lane");
    static_assert(offsetof(LocationOut, globalpoint) == 0 && offsetof(LocationOut, velocity) == 24, "x, y, dir, velocity are words 0 .. 7");
    int w = lane < kWords ? reinterpret_cast<const int*>(&si)[lane] : 0;
    auto get_id = [&](int slot) { return __shfl(w, kIdWord + slot, 64); };
    auto set_id = [&](int slot, int v) { if (lane == kIdWord + slot) w = v; };
    const int f_in = flags[s];
    const int ln = si.loc.lane_num;
    int f = f_in, ln_new = ln;
    if (f_in == 0) {
        const PlanningOut& R = plan[s].result;
        const GlobalPoint2D* __restrict__ P = plan[s].road_points;
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
        const double dist = 0.5 * (v + vn) / 3.6 * m.dt;
        // 3. pose
        // (path_near_id is the ego's index on the path the tick LOCALISED on; a tick that replanned published a new path that starts at the ego)
        const int k0 = state[s].afresh_planning ? 0 : clampi(state[s].path_near_id, 0, DMPP_PATH_POINTS - 1);
        const GlobalPoint2D p0 = P[k0];
        bool bad = !finite_f64(dist) || !finite_f64(p0.x) || !finite_f64(p0.y);
        double x = p0.x, y = p0.y, dir = si.loc.globalpoint.dir;
        bool path_end = false;
        if (!bad && dist > 0) {
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
                        dir = GetRoadAngle(c, a, b);
                        done = true; break;
                    }
                    acc = acc + Lj;
                }
            }
            if (!bad && !done) {
                path_end = true;
                x = P[DMPP_PATH_POINTS - 1].x; y = P[DMPP_PATH_POINTS - 1].y;
                if (last_seg >= 0) dir = GetRoadAngle(c, P[last_seg], P[last_seg + 1]);
            }
        }
        if (bad) f |= DMPP_EGO_BAD_PATH;
        else {
            if (path_end) f |= DMPP_EGO_PATH_END;
            if (lane < 8) {
                const int q = lane >> 1;
                const double d = q == 0 ? x : q == 1 ? y : q == 2 ? dir : vn;
                w = (lane & 1) ? __double2hiint(d) : __double2loint(d);
            }
            // 4. localisation ids of the current, left and right view (the slots k_planning reads)
            const int window = m.window;
            const LaneView lv = si.lanes;
            const bool has_c = ln >= 1 && ln <= DMPP_LANESUM && lv.cur_n > 0;
            const bool has_l = ln > 1 && ln - 2 < DMPP_LANESUM && lv.left_n > 0;
            const bool has_r = ln < lv.lane_sum && ln >= 0 && ln < DMPP_LANESUM && lv.right_n > 0;
            double dc = 0, dl = 0, dr = 0; int ic = -1, il = -1, ir = -1;
            if (has_c) wave_view_nearest(lane_pool + lv.cur_off, lv.cur_n, get_id(ln - 1), window, x, y, lane, dc, ic);
            if (has_l) wave_view_nearest(lane_pool + lv.left_off, lv.left_n, get_id(ln - 2), window, x, y, lane, dl, il);
            if (has_r) wave_view_nearest(lane_pool + lv.right_off, lv.right_n, get_id(ln), window, x, y, lane, dr, ir);
            if (has_c) {
                const int idc = ic >= 0 ? ic : get_id(ln - 1);
                if ((long long)idc + window >= (long long)lv.cur_n) f |= DMPP_EGO_LANE_END;
            }
            if (ic >= 0) set_id(ln - 1, ic);
            if (il >= 0) set_id(ln - 2, il);
            if (ir >= 0) set_id(ln, ir);
            // 5. lane number: only on a resident map, where k_resolve_map derives the new views
            if (map_mode && ic >= 0) {
                const double margin = 0.25 * lv.lane_width, rc = sqrt(dc);
                if (il >= 0 && rc - sqrt(dl) > margin) ln_new = ln - 1;
                else if (ir >= 0 && rc - sqrt(dr) > margin) ln_new = ln + 1;
                if (lane == kLaneNumWord) w = ln_new;
            }
            // 6. the grid does not follow the ego
            if (c.grid_stage) {
                const double fx = floor((x - si.grid_origin.x) / c.cell), fy = floor((y - si.grid_origin.y) / c.cell);
                if (!(fx >= 0 && fx < (double)c.grid_w && fy >= 0 && fy < (double)c.grid_h)) f |= DMPP_EGO_OFF_GRID;
            }
        }
    }
    if (lane < kWords) reinterpret_cast<int*>(&out[s])[lane] = w;
    if (trace) {                                        // (shuffles: every lane takes part)
        const int id_cur = get_id(clampi(ln_new - 1, 0, DMPP_LANESUM - 1));
        const double tx = __hiloint2double(__shfl(w, 1, 64), __shfl(w, 0, 64)), ty = __hiloint2double(__shfl(w, 3, 64), __shfl(w, 2, 64));
        const double td = __hiloint2double(__shfl(w, 5, 64), __shfl(w, 4, 64)), tv = __hiloint2double(__shfl(w, 7, 64), __shfl(w, 6, 64));
        if (lane == 0) {
            EgoTrace t;
            t.pose.x = tx; t.pose.y = ty; t.pose.dir = td; t.velocity = tv;
            t.id_cur = id_cur; t.lane_num = ln_new; t.flags = f; t._pad = 0;
            trace[s] = t;
        }
    }
    if (lane == 0) flags[s] = f;
}

// h_bad slot reset in stream order (pp_update_async on top of an update already staged: see the owner rule there)
__global__ void k_zero_word(int32_t* p) { *p = 0; }

}  // namespace dmpp
