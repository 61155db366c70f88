// kernels_tm.hpp — traffic manoeuvres (build-defined: the reference has no other vehicles): triggered lane changes,
// lateral offsets and speed changes of the actors of pp_set_traffic.  While pp_set_traffic_manoeuvres is in force
// k_manoeuvre_traffic<kFollow> takes the place of k_move_traffic (<false>) and k_follow_traffic (<true>) on every staged set, and
// k_reset_manoeuvres runs behind k_reset_traffic while §4m's reset is on as well.
//
// One 64-lane wave per actor, kTrafficWaves per 256-thread block, no LDS, no barrier, no atomics: the shape of k_follow_traffic.  An
// advance is a Jacobi step: the wave reads s, v and the TrafficManoeuvreState that all actors had BEFORE the advance and writes the
// other set, so the waves of a launch do not depend on each other.  Per advance, in §4v's order:
//   trigger  (wave-uniform) an idle actor with a record left and clock >= after looks at its record's trigger: its own clock, or the
//            ego of its scene as k_advance_* has just staged it, within a distance or a time of the actor's pose, on the wanted side;
//   start    (wave-uniform but for the projection) v0, lat0 and - onto another track - the projection of the pose: the lanes stride
//            ALL vertices of the target, 64 per pass, for the first nearest one (wave_first_min), then the foot on the at most two
//            segments that meet there gives s and lat0; the actor is on the target from this advance on;
//   step     §4h 2. - 3. with v0, or - kFollow and v0 > 0 - §4i 1. - 5. with v0 as the desired speed and, as candidates of step 1, the
//            actors of the same SCENE whose current track in the before-state is this actor's (the lanes stride the scene's members);
//   ramp     (wave-uniform) k, the smoothstep offset, and the end of the move; an idle actor's clock goes up;
//   pose     §4h 4. on the current track plus lat * the located segment's left normal when lat != 0; lane 0 stores.
// step = 0 (pp_update_async, the set call): the pose of the current (s, lat) on the current track, nothing else.
// Only + - * / sqrt floor on doubles, every one rounded once (-ffp-contract=off), and every order is total: the result is specified to
// the last bit (tests/traffic_manoeuvre_model.py restates it in numpy).
#pragma once
#include "kernels_t.hpp"

namespace dmpp {

// §4v pose: §4h 4.'s point of arc length s on track t, (dx, dy) of the segment it lies on, and - only when lat != 0 and the segment
// has a length - lat times that segment's left normal added
struct ManPose { ObPoint o; double dx, dy; };
__device__ __forceinline__ ManPose manoeuvre_pose(const TrackView& t, const GlobalPoint2D* __restrict__ pts, const TrafficPin& pin, double s, double lat)
{
    ManPose p;
    p.o = traffic_pose(t, pts, pin, s);
    const int i = traffic_locate(t.c, t.nseg, s);
    const GlobalPoint2D P = pts[t.tk.point_off + i];
    const GlobalPoint2D Q = pts[t.tk.point_off + (i + 1 < t.n ? i + 1 : 0)];
    p.dx = Q.x - P.x; p.dy = Q.y - P.y;
    if (lat != 0) {
        const double len = sqrt(p.dx * p.dx + p.dy * p.dy);
        if (len > 0) {
            const double nx = -p.dy / len, ny = p.dx / len;
            p.o.x = p.o.x + lat * nx; p.o.y = p.o.y + lat * ny;
        }
    }
    return p;
}

// §4v start, one candidate segment i of the target for the pose (x, y): the foot with the parameter clamped to [0, 1]; kept if its
// squared distance is strictly smaller than the best so far (a NaN never is; a zero-length segment is skipped)
struct ManFoot { double f2, u, lat; int i; };
__device__ __forceinline__ void manoeuvre_foot(const TrackView& T, const GlobalPoint2D* __restrict__ pts, int i, double x, double y, ManFoot& best)
{
    if (i < 0) return;
    const GlobalPoint2D A = pts[T.tk.point_off + i];
    const GlobalPoint2D B = pts[T.tk.point_off + (i + 1 < T.n ? i + 1 : 0)];
    const double dx = B.x - A.x, dy = B.y - A.y;
    const double l2 = dx * dx + dy * dy;
    if (!(l2 > 0)) return;
    const double ax = x - A.x, ay = y - A.y;
    double u = (ax * dx + ay * dy) / l2;
    if (!(u >= 0)) u = 0;
    if (u > 1) u = 1;
    const double fx = A.x + u * dx, fy = A.y + u * dy;
    const double gx = x - fx, gy = y - fy;
    const double f2 = gx * gx + gy * gy;
    if ((best.i < 0 && f2 == f2) || f2 < best.f2) {
        best.f2 = f2; best.u = u; best.i = i;
        best.lat = (dx * ay - dy * ax) / sqrt(l2);       // the signed distance from the segment's line, left positive
    }
}

// §4v start: the pose (x, y) projected onto track T, the same in every lane; false: no vertex of T has a distance (nothing changes)
__device__ __forceinline__ bool manoeuvre_project(const TrackView& T, const GlobalPoint2D* __restrict__ pts, double x, double y, int lane, double& s, double& lat0)
{
    double bd = 0; int bj = -1;
    for (int j = lane; j < T.n; j += 64) {
        const GlobalPoint2D P = pts[T.tk.point_off + j];
        const double ex = P.x - x, ey = P.y - y;
        const double d2 = ex * ex + ey * ey;
        if ((bj < 0 && d2 == d2) || d2 < bd) { bd = d2; bj = j; }       // (j rises within a lane: the first minimum; a NaN is never the minimum)
    }
    wave_first_min(bd, bj);
    if (bj < 0) return false;
    // the segments that meet in vertex bj, the earlier one first: bj - 1 (the closing segment for vertex 0 of a closed track) and bj
    const int before = bj > 0 ? bj - 1 : (T.closed ? T.n - 1 : -1);
    const int behind = bj < T.nseg ? bj : -1;
    ManFoot best; best.f2 = 0; best.u = 0; best.lat = 0; best.i = -1;
    manoeuvre_foot(T, pts, before < behind ? before : behind, x, y, best);
    manoeuvre_foot(T, pts, before < behind ? behind : before, x, y, best);
    if (best.i < 0) { s = T.c[bj]; lat0 = 0; }           // both segments without a length: the vertex itself
    else { const double c0 = T.c[best.i]; s = c0 + best.u * (T.c[best.i + 1] - c0); lat0 = best.lat; }
    s = traffic_wrap(s, T.L, T.closed);
    return true;
}

// step: 0 (the set call, pp_update_async) or EgoModel.dt (pp_advance_async).  scene_of: every actor's scene; scene_first / members:
// the actor indices sorted by (scene, index) and the first of every scene; recs / rec_first: the records and every actor's run of
// them.  s_in / v_in / st_in and s_out / v_out / st_out are different arrays (step = 0 writes none of them); v_in / v_out: read and
// written only by <true>.  in / flags: the SceneIn records being staged and the ego flag words as the advance left them.
template <bool kFollow>
__global__ void __launch_bounds__(kBlock)
k_manoeuvre_traffic(int n_actors, double step, TrafficFollow tf, double half_w, const TrafficPin* __restrict__ actors, const int32_t* __restrict__ scene_of,
                    const int32_t* __restrict__ scene_first, const int32_t* __restrict__ members, const TrafficManoeuvre* __restrict__ recs,
                    const int32_t* __restrict__ rec_first, const TrafficTrackDev* __restrict__ tracks, const double* __restrict__ cum,
                    const GlobalPoint2D* __restrict__ pts, const double* __restrict__ s_in, const double* __restrict__ v_in,
                    const TrafficManoeuvreState* __restrict__ st_in, double* __restrict__ s_out, double* __restrict__ v_out,
                    TrafficManoeuvreState* __restrict__ st_out, const SceneIn* __restrict__ in, const int32_t* __restrict__ flags,
                    ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int lane = threadIdx.x & 63;
    const int a = __builtin_amdgcn_readfirstlane(blockIdx.x * kTrafficWaves + (threadIdx.x >> 6));
    if (a >= n_actors) return;                          // (whole waves leave: no barrier below)
    TrafficPin pin = actors[a];
    TrafficManoeuvreState st = st_in[a];
    double s = s_in[a];
    pin.track = st.track; pin.speed = st.v0;            // a plain actor of its current track that wants v0
    TrackView t = traffic_view(tracks, cum, st.track);
    if (step == 0) {                                    // placed where it is: no trigger, no step, no clock
        if (lane == 0) traffic_store(obs, mot, pin.pool, manoeuvre_pose(t, pts, pin, s, st.lat).o);
        return;
    }
    const int c = scene_of[a];
    const int r0 = rec_first[a];
    const bool have = st.next >= 0 && st.next < rec_first[a + 1] - r0;
    TrafficManoeuvre m = {};
    if (have) m = recs[r0 + st.next];
    // trigger
    bool fire = false;
    if (have && st.k == 0 && st.clock >= m.after) {
        const int kind = m.trigger & 255, side = m.trigger >> 8;
        const ManPose P = manoeuvre_pose(t, pts, pin, s, st.lat);
        if (kind == DMPP_TRIG_ADVANCES) fire = true;
        else {
            const double ex = P.o.x - in[c].loc.globalpoint.x, ey = P.o.y - in[c].loc.globalpoint.y;
            const double d2 = ex * ex + ey * ey;
            double r2;
            if (kind == DMPP_TRIG_EGO_DIST) r2 = m.dist * m.dist;
            else {
                const double ve = flags[c] != 0 ? 0.0 : in[c].loc.velocity / 3.6;
                const double r = m.time * ve;
                r2 = r * r;
            }
            const double p = ex * P.dx + ey * P.dy;
            fire = d2 <= r2 && (side == 0 || (side == 1 && p >= 0) || (side == 2 && p <= 0));       // (a NaN compares false)
        }
        // start of the move
        if (fire) {
            if (m.speed == m.speed) { st.v0 = m.speed; pin.speed = m.speed; }
            st.lat0 = st.lat;
            if (m.track >= 0 && m.track != st.track) {
                const TrackView T = traffic_view(tracks, cum, m.track);
                double s2, l0;
                if (manoeuvre_project(T, pts, P.o.x, P.o.y, lane, s2, l0)) { s = s2; st.lat0 = l0; st.track = m.track; pin.track = m.track; t = T; }
            }
        }
    }
    // step
    double s1, v1;
    if (!kFollow || !(pin.speed > 0)) {                 // scripted, parked or reversing: §4h's step, v = v0
        s1 = traffic_step(t, s, pin.speed, step); v1 = pin.speed;
    } else {
        const double v = v_in[a];
        const TrafficAhead ahead = follow_actor_ahead<true>(t, c, a, s, tf.look, scene_first, members, s_in, lane, st_in, st.track);
        const int i0 = traffic_locate(t.c, t.nseg, s);
        double ed;
        const int ek = follow_scene_ego(t, pts, i0, t.closed ? t.n : t.n - 1 - i0, s, tf.look, in[c].loc.globalpoint.x, in[c].loc.globalpoint.y, lane, ed);
        int e = -1, pj; double g_e = 0;
        if (ek >= 0 && ed <= tf.lateral * tf.lateral) { e = c; g_e = follow_window_gap(t, i0, s, ek, pj); }
        s1 = follow_drive(t, tf, pin, s, v, step, half_w, ahead, e, g_e, actors, v_in, in, flags, v1);
    }
    // ramp
    if (have && (fire || st.k > 0)) {
        st.k = st.k + 1;
        const double tau = (double)st.k / (double)m.n_steps;
        const double w = tau * tau * (3 - 2 * tau);
        st.lat = st.lat0 + (m.lat_end - st.lat0) * w;
        if (st.k == m.n_steps) { st.lat = m.lat_end; st.k = 0; st.next = st.next + 1; st.n_done = st.n_done + 1; st.clock = 0; }
    } else if (st.clock < INT32_MAX) st.clock = st.clock + 1;
    if (lane == 0) {
        s_out[a] = s1;
        if (kFollow) v_out[a] = v1;
        st_out[a] = st;
        traffic_store(obs, mot, pin.pool, manoeuvre_pose(t, pts, pin, s1, st.lat).o);
    }
}

// k_reset_manoeuvres runs in an advance directly behind k_reset_traffic while §4m's reset and manoeuvres are both on: the actors of
// every scene that RESTARTED in this advance (EpisodeStats.age == 0) go back to the state of the set call - on pin.track, where
// k_reset_traffic has just put s, v and the pose - and keep n_done.  One thread per actor, 256-thread blocks; st_arr: the CURRENT states.
__global__ void __launch_bounds__(kBlock)
k_reset_manoeuvres(int n_actors, const TrafficPin* __restrict__ actors, const int32_t* __restrict__ scene_of, const EpisodeStats* __restrict__ stats,
                   TrafficManoeuvreState* __restrict__ st_arr)
{
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= n_actors) return;
    if (stats[scene_of[a]].age != 0) return;
    TrafficManoeuvreState st = {};
    st.v0 = actors[a].speed; st.track = actors[a].track; st.n_done = st_arr[a].n_done;
    st_arr[a] = st;
}

}  // namespace dmpp
