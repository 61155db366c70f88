// kernels_t.hpp — lane traffic (build-defined: the reference has no other vehicles): k_move_traffic steps every
// scripted actor along its track and writes it into its pinned entry of the obstacle pool being staged, so that the tick's
// kernels - which only ever read the obstacle list - react to traffic with no change.
//
// One thread per actor, 256-thread blocks, no LDS, no barrier, no scratch.  A thread reads its 24-byte actor record (8 + 16
// bytes), its arc length, the 16-byte track header (one load), log2(nseg) + 3 entries of the cumulative-length table and two
// 16-byte points; it writes the arc length, one ObPoint (16 + 8 bytes) and - with a motion pool - one 16-byte ObMotion.  The
// pool entries of a launch are distinct (checked by pp_set_traffic), so the threads do not depend on each other.  Every
// operation is exact or correctly rounded (-ffp-contract=off) and the segment index is unique, so the result is specified to
// the last bit.
#pragma once
#include "dev_geom.hpp"
#include "kernels_f.hpp"

namespace dmpp {

// what pp_set_traffic keeps of a TrafficActor: the pool entry is absolute (obs_off[scene] + slot of the resident records)
struct alignas(8) TrafficPin { double speed; int32_t pool, track, type; float radius; };                          // 24 B
// a track on the device: its points [point_off, point_off + n_points) of the handle's compact point array and its
// nseg + 1 cumulative lengths from cum_off on (nseg = n_points, closed, or n_points - 1)
struct alignas(16) TrafficTrackDev { int32_t point_off, n_points, closed, cum_off; };                              // 16 B

// §4h `wrap`: an open track clamps, a closed one (L > 0, checked at set time) takes s modulo L
__device__ inline double traffic_wrap(double s, double L, bool closed)
{
    if (closed) {
        const double q = floor(s / L);
        s = s - q * L;
        if (!(s >= 0)) s = 0;
        if (s >= L) s = 0;
    } else {
        if (!(s >= 0)) s = 0;
        if (s > L) s = L;
    }
    return s;
}

// ---- the steps every traffic kernel shares, each written once (the kernels below are thin over them)

// a track as one thread or wave sees it: the header, its cumulative lengths c[0 .. nseg], nseg (= n, closed, or n - 1) and L = c[nseg]
struct TrackView { TrafficTrackDev tk; const double* c; int n, nseg; bool closed; double L; };

__device__ __forceinline__ TrackView traffic_view(const TrafficTrackDev* __restrict__ tracks, const double* __restrict__ cum, int track)
{
    TrackView t;
    t.tk = tracks[track];
    t.closed = t.tk.closed != 0;
    t.n = t.tk.n_points; t.nseg = t.closed ? t.n : t.n - 1;
    t.c = cum + t.tk.cum_off;
    t.L = t.c[t.nseg];
    return t;
}

// §4h 2. - 3.: the step of a scripted actor; step = 0 places it where it is (the product is rounded, then the sum: no contraction)
__device__ __forceinline__ double traffic_step(const TrackView& t, double s, double speed, double step)
{
    if (step != 0) s = s + speed * step;
    return traffic_wrap(s, t.L, t.closed);
}

// §4h 4., first line: the largest i in [0, nseg) with cum[i] <= s (cum is non-decreasing and cum[0] = 0 <= s)
__device__ __forceinline__ int traffic_locate(const double* __restrict__ c, int nseg, double s)
{
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

// §4h 4. - 5.: the obstacle of an actor at arc length s
__device__ __forceinline__ ObPoint traffic_pose(const TrackView& t, const GlobalPoint2D* __restrict__ pts, const TrafficPin& pin, double s)
{
    const int i = traffic_locate(t.c, t.nseg, s);
    const double c0 = t.c[i], d = t.c[i + 1] - c0;
    const double u = d > 0 ? (s - c0) / d : 0.0;
    const GlobalPoint2D P = pts[t.tk.point_off + i];
    const GlobalPoint2D Q = pts[t.tk.point_off + (i + 1 < t.n ? i + 1 : 0)];             // (the closing segment ends on point 0)
    ObPoint o;
    o.x = P.x + u * (Q.x - P.x); o.y = P.y + u * (Q.y - P.y); o.type = pin.type; o.radius = pin.radius;
    return o;
}

// pool entry e of the set being staged; mot: nullptr when the set carries no motion pool
__device__ __forceinline__ void traffic_store(ObPoint* __restrict__ obs, ObMotion* __restrict__ mot, int e, const ObPoint& o)
{
    obs[e] = o;
    if (mot) { ObMotion z; z.vx = 0; z.vy = 0; mot[e] = z; }
}

// §4j: the same entry of every member scene [p0, p1) of a world; the lanes stride the members
__device__ __forceinline__ void world_store(ObPoint* __restrict__ obs, ObMotion* __restrict__ mot, const FleetPin* __restrict__ fpin, int lane, int p0, int p1,
                                            int slot, const ObPoint& o)
{
    for (int m = p0 + lane; m < p1; m += 64)
        traffic_store(obs, mot, fpin[m].obs_off + slot, o);      // (the slot is an own entry of every member: checked by pp_set_world_traffic)
}

// §4i 1. the actor ahead: the smallest (g, b) over the members of `group`, the same in every lane; i < 0: none
// kOnTrack (§4v, manoeuvres): the group is the actor's whole SCENE and a member counts only while its current track, st[b].track, is `track`
struct TrafficAhead { double g; int i; };

template <bool kOnTrack = false>
__device__ __forceinline__ TrafficAhead follow_actor_ahead(const TrackView& t, int group, int a, double s, double look, const int32_t* __restrict__ group_first,
                                                           const int32_t* __restrict__ members, const double* __restrict__ s_in, int lane,
                                                           const TrafficManoeuvreState* __restrict__ st = nullptr, int track = 0)
{
    double bg = 0; int bi = -1;
    for (int m = group_first[group] + lane, m1 = group_first[group + 1]; m < m1; m += 64) {
        const int b = members[m];
        if (b == a) continue;
        if (kOnTrack) { if (st[b].track != track) continue; }
        double g = s_in[b] - s;
        bool ok = true;
        if (t.closed) { if (g < 0 || (g == 0 && b > a)) g = g + t.L; }
        else ok = g > 0 || (g == 0 && b < a);
        if (ok && g <= look && (bi < 0 || g < bg)) { bg = g; bi = b; }       // (b rises within a lane: ties keep the lower index; a NaN compares false)
    }
    wave_first_min(bg, bi);
    return { bg, bi };
}

// §4i 2., the window: the gap g_k to the k-th vertex past segment i0 and that vertex's index pj (a closed track runs on over point 0)
__device__ __forceinline__ double follow_window_gap(const TrackView& t, int i0, double s, int k, int& pj)
{
    const int j = i0 + k;
    if (j <= t.n - 1) { pj = j; return t.c[j] - s; }
    pj = j - t.n; return (t.L - s) + t.c[pj];
}

// §4i 3. - 5., wave-uniform: the leader - actor `ahead` (i < 0: none) or the ego of scene e at gap g_e (e < 0: none; the ego wins a
// tie) -, the intelligent-driver acceleration and the integration; returns s1 and sets v1
__device__ __forceinline__ double follow_drive(const TrackView& t, const TrafficFollow& tf, const TrafficPin& pin, double s, double v, double dt, double half_w,
                                               TrafficAhead ahead, int e, double g_e, const TrafficPin* __restrict__ actors, const double* __restrict__ v_in,
                                               const SceneIn* __restrict__ in, const int32_t* __restrict__ flags, double& v1)
{
    // 3. the leader
    bool lead = false; double g = 0, vl = 0, rl = 0;
    if (ahead.i >= 0) { lead = true; g = ahead.g; vl = v_in[ahead.i]; rl = (double)actors[ahead.i].radius; }
    if (e >= 0 && (!lead || g_e <= g)) {
        lead = true; g = g_e; rl = half_w;
        vl = flags[e] != 0 ? 0.0 : in[e].loc.velocity / 3.6;
    }
    // 4. the acceleration
    const double r = v / pin.speed, r2 = r * r, fr = 1 - r2 * r2;
    double acc;
    if (!lead) acc = tf.max_acc * fr;
    else {
        double net = g - (double)pin.radius - rl;
        if (!(net > tf.min_net)) net = tf.min_net;
        const double dv = v - vl;
        const double c2 = 2 * sqrt(tf.max_acc * tf.comfort_dec);
        double dyn = v * tf.headway + (v * dv) / c2;
        if (!(dyn > 0)) dyn = 0;
        const double star = tf.gap + dyn, q = star / net;
        acc = tf.max_acc * (fr - q * q);
    }
    if (!(acc >= -tf.max_dec)) acc = -tf.max_dec;       // (a NaN brakes)
    // 5. integrate
    v1 = v + acc * dt;
    if (!(v1 > 0)) v1 = 0;
    return traffic_wrap(s + 0.5 * (v + v1) * dt, t.L, t.closed);
}

// step: 0 (pp_set_traffic, pp_update_async: the actors are placed where they are) or EgoModel.dt (pp_advance_async).
// mot: nullptr when the set carries no motion pool.
__global__ void __launch_bounds__(kBlock)
k_move_traffic(int n_actors, double step, const TrafficPin* __restrict__ actors, const TrafficTrackDev* __restrict__ tracks,
               const double* __restrict__ cum, const GlobalPoint2D* __restrict__ pts, double* __restrict__ s_arr,
               ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= n_actors) return;
    const TrafficPin pin = actors[a];
    const TrackView t = traffic_view(tracks, cum, pin.track);
    const double s = traffic_step(t, s_arr[a], pin.speed, step);
    s_arr[a] = s;
    traffic_store(obs, mot, pin.pool, traffic_pose(t, pts, pin, s));
}

// ---- episode traffic reset.  What both reset kernels share: the start state actor a goes back to - set
// cur_start of scene c's spawn record (n_sets > 1) or set 0; set k of actor a at k * n_actors + a -, its pin and its track:
// s' = wrap(s*) and v' = v* (speed > 0) or speed (§4i: a parked or reversing actor keeps v = speed).  sstats: read only with n_sets > 1
struct TrafficRestart { TrafficPin pin; TrackView t; double s, v; };
__device__ __forceinline__ TrafficRestart traffic_restart(int a, int c, int n_actors, int n_sets, const TrafficPin* __restrict__ actors, const EpisodeSpawnStats* __restrict__ sstats,
                                                          const TrafficStart* __restrict__ starts, const TrafficTrackDev* __restrict__ tracks, const double* __restrict__ cum)
{
    int k = 0;
    if (n_sets > 1) { k = sstats[c].cur_start; if (k < 0 || k >= n_sets) k = 0; }      // (the set call checked n_sets == n_starts: never taken)
    const TrafficStart st = starts[(size_t)k * (size_t)n_actors + (size_t)a];
    const TrafficPin pin = actors[a]; const TrackView t = traffic_view(tracks, cum, pin.track);
    return { pin, t, traffic_wrap(st.s, t.L, t.closed), pin.speed > 0 ? st.v : pin.speed };
}

// k_reset_traffic runs in an advance behind k_move_traffic / k_follow_traffic while pp_set_episode_traffic is in force and puts the
// actors of every scene that RESTARTED in this advance - EpisodeStats.age == 0 behind the episode step - back on a start state.
// One thread per actor, 256-thread blocks, no LDS, no barrier, no scratch: the shape of k_move_traffic.  A thread whose scene
// goes on leaves after two loads (its scene, the scene's age).  The others discard the step the traffic kernel has just made:
// s' and - following on - v' go into the CURRENT arrays (the ones that kernel wrote), the pose of s' into the pinned pool entry
// with a zero ObMotion, and the actor's counter goes up by one.  v_arr: nullptr while following is off.
__global__ void __launch_bounds__(kBlock)
k_reset_traffic(int n_actors, int n_sets, const TrafficPin* __restrict__ actors, const int32_t* __restrict__ scene_of,
                const EpisodeStats* __restrict__ stats, const EpisodeSpawnStats* __restrict__ sstats, const TrafficStart* __restrict__ starts,
                const TrafficTrackDev* __restrict__ tracks, const double* __restrict__ cum, const GlobalPoint2D* __restrict__ pts,
                double* __restrict__ s_arr, double* __restrict__ v_arr, int32_t* __restrict__ n_resets, ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= n_actors) return;
    const int c = scene_of[a];
    if (stats[c].age != 0) return;                      // the scene goes on: its actors stay as the traffic kernel wrote them
    const TrafficRestart r = traffic_restart(a, c, n_actors, n_sets, actors, sstats, starts, tracks, cum);
    s_arr[a] = r.s;
    if (v_arr) v_arr[a] = r.v;
    traffic_store(obs, mot, r.pin.pool, traffic_pose(r.t, pts, r.pin, r.s));
    n_resets[a] = n_resets[a] + 1;
}

// ---- car-following traffic: k_follow_traffic takes the place of k_move_traffic in an advance while following is on.
//
// One 64-lane wave per actor, four actors per 256-thread block, no LDS, no barrier, no scratch (the shape of k_couple_fleet).  The
// step is a Jacobi step: the wave reads s and v of the arrays all actors had BEFORE the advance and writes the other pair, so the
// waves of a launch do not depend on each other.  An actor with !(speed > 0) steps exactly as k_move_traffic does.  A follower
//   1. strides the members of its (scene, track) group - actor indices sorted by (scene, track, index), built by the host - for
//      the nearest actor ahead within `look` (follow_actor_ahead);
//   2. strides the vertices ahead of its segment, 64 per pass, for the one nearest its scene's ego as k_advance_* has just staged
//      it, stopping after the first pass in which no lane is within `look` (the gaps never decrease): a (d2, k) wave minimum;
//   3. - 5. follow_drive, and lane 0 stores s, v, the ObPoint and, with a motion pool, a zero ObMotion.
// Only + - * / sqrt floor on doubles, every one rounded once (-ffp-contract=off), and both orders are total: the result is specified
// to the last bit.
constexpr int kTrafficWaves = 4;       // actors or vehicles (waves) per block of k_follow_traffic and the two world-traffic kernels

struct TrafficRef { int32_t scene, group; };       // what a follower needs beside its pin: its scene's records, its group's members

// §4i 2. per scene: the first nearest vertex to the ego at (x, y) among the window's, the same in every lane; k < 0: none
__device__ __forceinline__ int follow_scene_ego(const TrackView& t, const GlobalPoint2D* __restrict__ pts, int i0, int kmax, double s, double look,
                                                double x, double y, int lane, double& ed)
{
    int ek = -1; ed = 0;
    for (int k0 = 1; k0 <= kmax; k0 += 64) {
        const int k = k0 + lane;
        bool within = false;
        if (k <= kmax) {
            int pj; const double g = follow_window_gap(t, i0, s, k, pj);
            if (g <= look) {
                within = true;
                const GlobalPoint2D P = pts[t.tk.point_off + pj];
                const double ex = P.x - x, ey = P.y - y;
                const double d2 = ex * ex + ey * ey;
                if ((ek < 0 && d2 == d2) || d2 < ed) { ed = d2; ek = k; }       // (k rises within a lane; a NaN is never the minimum)
            }
        }
        if (!__any(within)) break;
    }
    wave_first_min(ed, ek);
    return ek;
}

// in: the SceneIn records being staged (read: loc.globalpoint, loc.velocity); flags: the ego flag words as the advance left them.
// s_in / v_in and s_out / v_out are different arrays.  half_w = 0.5 * Vehicle_Width (rounded once, on the host: exact).
__global__ void __launch_bounds__(kBlock)
k_follow_traffic(int n_actors, double dt, TrafficFollow tf, double half_w, const TrafficPin* __restrict__ actors, const TrafficRef* __restrict__ refs,
                 const int32_t* __restrict__ group_first, const int32_t* __restrict__ members, const TrafficTrackDev* __restrict__ tracks,
                 const double* __restrict__ cum, const GlobalPoint2D* __restrict__ pts, const double* __restrict__ s_in, const double* __restrict__ v_in,
                 double* __restrict__ s_out, double* __restrict__ v_out, const SceneIn* __restrict__ in, const int32_t* __restrict__ flags,
                 ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * kTrafficWaves + (threadIdx.x >> 6);
    if (a >= n_actors) return;                          // (whole waves leave: no barrier below)
    const TrafficPin pin = actors[a];
    const TrackView t = traffic_view(tracks, cum, pin.track);
    const double s = s_in[a];
    double s1, v1;
    if (!(pin.speed > 0)) {                             // parked or reversing: §4h's step, v = speed
        s1 = traffic_step(t, s, pin.speed, dt); v1 = pin.speed;
    } else {
        const double v = v_in[a];
        const TrafficRef ref = refs[a];
        const TrafficAhead ahead = follow_actor_ahead(t, ref.group, a, s, tf.look, group_first, members, s_in, lane);
        // 2. the ego: the first nearest vertex of the window ahead, a leader if it is within `lateral` of it
        const int i0 = traffic_locate(t.c, t.nseg, s);
        double ed;
        const int ek = follow_scene_ego(t, pts, i0, t.closed ? t.n : t.n - 1 - i0, s, tf.look, in[ref.scene].loc.globalpoint.x, in[ref.scene].loc.globalpoint.y, lane, ed);
        int e = -1, pj; double g_e = 0;
        if (ek >= 0 && ed <= tf.lateral * tf.lateral) { e = ref.scene; g_e = follow_window_gap(t, i0, s, ek, pj); }
        s1 = follow_drive(t, tf, pin, s, v, dt, half_w, ahead, e, g_e, actors, v_in, in, flags, v1);
    }
    if (lane == 0) {
        s_out[a] = s1; v_out[a] = v1;
        traffic_store(obs, mot, pin.pool, traffic_pose(t, pts, pin, s1));
    }
}

// ---- world traffic: one vehicle per WORLD of the fleet in force, written into entry pin[m].obs_off + slot of
// every member scene m and - following - led by the nearest of all the world's egos.  k_move_world_traffic and
// k_follow_world_traffic take the places of k_move_traffic and k_follow_traffic while the handle's traffic was set with
// pp_set_world_traffic; a TrafficPin then carries the SLOT in `pool` and a TrafficRef the WORLD in `scene`.
//
// One 64-lane wave per vehicle, four per 256-thread block, no LDS, no barrier, no scratch.  The vehicle index is made wave-uniform
// (readfirstlane), so its record, its track and its state are scalar loads and the pose is computed once per wave; the lanes
// stride the world's members to store it - the same bytes into every member's entry, plain vector stores (world_store).  The
// follow kernel
//   1. strides its (world, track) group exactly as k_follow_traffic strides its (scene, track) group;
//   2. strides the member EGOS, 64 per pass: every lane walks the window vertices k = 1, 2, .. while g_k <= look (the trip count
//      and the vertex loads are wave-uniform), keeps the first minimum d2 of its own ego, applies the lateral test and keeps its
//      best (g_e, e) across passes (e rises within a lane: a tie keeps the lower scene); one wave_first_min picks the leader;
//   3. - 5. as k_follow_traffic, wave-uniform.

// §4i 2. per world: the member ego [p0, p1) with the smallest (g_e, e) that is within `lateral` of its first nearest window vertex,
// the same in every lane; e < 0: none
__device__ __forceinline__ int follow_world_ego(const TrackView& t, const GlobalPoint2D* __restrict__ pts, int i0, int kmax, double s, double look,
                                                double lat2, const SceneIn* __restrict__ in, int p0, int p1, int lane, double& eg)
{
    int ee = -1; eg = 0;
    for (int e0 = p0; e0 < p1; e0 += 64) {
        const int e = e0 + lane;
        const bool mine = e < p1;
        double x = 0, y = 0;
        if (mine) { x = in[e].loc.globalpoint.x; y = in[e].loc.globalpoint.y; }
        double md = 0, mg = 0; bool have = false;
        for (int k = 1; k <= kmax; k++) {               // (wave-uniform: g depends on the vehicle alone)
            int pj; const double g = follow_window_gap(t, i0, s, k, pj);
            if (!(g <= look)) break;                    // (the gaps never decrease with k: the vertices that take part are a prefix)
            const GlobalPoint2D P = pts[t.tk.point_off + pj];
            const double ex = P.x - x, ey = P.y - y;
            const double d2 = ex * ex + ey * ey;
            if ((!have && d2 == d2) || d2 < md) { md = d2; mg = g; have = true; }      // (k rises: the first minimum; a NaN is never the minimum)
        }
        if (mine && have && md <= lat2 && (ee < 0 || mg < eg)) { eg = mg; ee = e; }      // (e rises within a lane: ties keep the lower scene)
    }
    wave_first_min(eg, ee);
    return ee;
}

// step: 0 (pp_set_world_traffic, pp_update_async) or EgoModel.dt (pp_advance_async with following off).  world: every vehicle's world.
__global__ void __launch_bounds__(kBlock)
k_move_world_traffic(int n_actors, double step, const TrafficPin* __restrict__ actors, const int32_t* __restrict__ world,
                     const int32_t* __restrict__ world_first, const FleetPin* __restrict__ fpin, const TrafficTrackDev* __restrict__ tracks,
                     const double* __restrict__ cum, const GlobalPoint2D* __restrict__ pts, double* __restrict__ s_arr,
                     ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int lane = threadIdx.x & 63;
    const int a = __builtin_amdgcn_readfirstlane(blockIdx.x * kTrafficWaves + (threadIdx.x >> 6));
    if (a >= n_actors) return;                          // (whole waves leave: no barrier below)
    const TrafficPin pin = actors[a];
    const TrackView t = traffic_view(tracks, cum, pin.track);
    const double s = traffic_step(t, s_arr[a], pin.speed, step);
    if (lane == 0) s_arr[a] = s;
    const int w = world[a];
    world_store(obs, mot, fpin, lane, world_first[w], world_first[w + 1], pin.pool, traffic_pose(t, pts, pin, s));
}

// As k_follow_traffic, with refs[a].scene = the vehicle's WORLD and the groups those of (world, track); in / flags: the records and
// ego flag words of every scene as staged.
__global__ void __launch_bounds__(kBlock)
k_follow_world_traffic(int n_actors, double dt, TrafficFollow tf, double half_w, const TrafficPin* __restrict__ actors, const TrafficRef* __restrict__ refs,
                       const int32_t* __restrict__ group_first, const int32_t* __restrict__ members, const int32_t* __restrict__ world_first,
                       const FleetPin* __restrict__ fpin, const TrafficTrackDev* __restrict__ tracks, const double* __restrict__ cum,
                       const GlobalPoint2D* __restrict__ pts, const double* __restrict__ s_in, const double* __restrict__ v_in,
                       double* __restrict__ s_out, double* __restrict__ v_out, const SceneIn* __restrict__ in, const int32_t* __restrict__ flags,
                       ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int lane = threadIdx.x & 63;
    const int a = __builtin_amdgcn_readfirstlane(blockIdx.x * kTrafficWaves + (threadIdx.x >> 6));
    if (a >= n_actors) return;                          // (whole waves leave: no barrier below)
    const TrafficPin pin = actors[a];
    const TrackView t = traffic_view(tracks, cum, pin.track);
    const double s = s_in[a];
    const TrafficRef ref = refs[a];
    const int p0 = world_first[ref.scene], p1 = world_first[ref.scene + 1];
    double s1, v1;
    if (!(pin.speed > 0)) {                             // parked or reversing: §4h's step, v = speed
        s1 = traffic_step(t, s, pin.speed, dt); v1 = pin.speed;
    } else {
        const double v = v_in[a];
        const TrafficAhead ahead = follow_actor_ahead(t, ref.group, a, s, tf.look, group_first, members, s_in, lane);
        const int i0 = traffic_locate(t.c, t.nseg, s);
        double g_e;
        const int e = follow_world_ego(t, pts, i0, t.closed ? t.n : t.n - 1 - i0, s, tf.look, tf.lateral * tf.lateral, in, p0, p1, lane, g_e);
        s1 = follow_drive(t, tf, pin, s, v, dt, half_w, ahead, e, g_e, actors, v_in, in, flags, v1);
    }
    if (lane == 0) { s_out[a] = s1; v_out[a] = v1; }
    world_store(obs, mot, fpin, lane, p0, p1, pin.pool, traffic_pose(t, pts, pin, s1));
}

// ---- world traffic reset: k_reset_world_traffic is k_reset_traffic for the vehicles of pp_set_world_traffic, in an
// advance behind k_move_world_traffic / k_follow_world_traffic while pp_set_episode_world_traffic is in force.  A vehicle goes back
// to a start state when its WORLD restarted in this advance: with world episodes (§4s) every member restarts together, so the world's
// first scene stands for it - EpisodeStats.age == 0 there, and its cur_start names the set.
//
// One wave per vehicle, four per block, no LDS, no barrier, no scratch: the shape of k_move_world_traffic.  A wave whose world goes
// on leaves after three scalar loads (its world, the world's first scene, that scene's age).
__global__ void __launch_bounds__(kBlock)
k_reset_world_traffic(int n_actors, int n_sets, const TrafficPin* __restrict__ actors, const int32_t* __restrict__ world,
                      const int32_t* __restrict__ world_first, const FleetPin* __restrict__ fpin, const EpisodeStats* __restrict__ stats,
                      const EpisodeSpawnStats* __restrict__ sstats, const TrafficStart* __restrict__ starts, const TrafficTrackDev* __restrict__ tracks,
                      const double* __restrict__ cum, const GlobalPoint2D* __restrict__ pts, double* __restrict__ s_arr, double* __restrict__ v_arr,
                      int32_t* __restrict__ n_resets, ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int lane = threadIdx.x & 63;
    const int a = __builtin_amdgcn_readfirstlane(blockIdx.x * kTrafficWaves + (threadIdx.x >> 6));
    if (a >= n_actors) return;                          // (whole waves leave: no barrier below)
    const int w = world[a];
    const int p0 = world_first[w];
    if (stats[p0].age != 0) return;                     // the world goes on: its vehicles stay as the traffic kernel wrote them
    const int p1 = world_first[w + 1];
    const TrafficRestart r = traffic_restart(a, p0, n_actors, n_sets, actors, sstats, starts, tracks, cum);
    if (lane == 0) {
        s_arr[a] = r.s;
        if (v_arr) v_arr[a] = r.v;
        n_resets[a] = n_resets[a] + 1;
    }
    world_store(obs, mot, fpin, lane, p0, p1, r.pin.pool, traffic_pose(r.t, pts, r.pin, r.s));
}

}  // namespace dmpp
