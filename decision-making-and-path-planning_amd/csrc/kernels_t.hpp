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
    const TrafficTrackDev tk = tracks[pin.track];
    const bool closed = tk.closed != 0;
    const int nseg = closed ? tk.n_points : tk.n_points - 1;
    const double* c = cum + tk.cum_off;
    const double L = c[nseg];
    double s = s_arr[a];
    if (step != 0) s = s + pin.speed * step;             // (the product is rounded, then the sum: no contraction)
    s = traffic_wrap(s, L, closed);
    s_arr[a] = s;
    // the largest i in [0, nseg) with cum[i] <= s: cum is non-decreasing and cum[0] = 0 <= s
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= s) lo = mid; else hi = mid;
    }
    const double c0 = c[lo], d = c[lo + 1] - c0;
    const double t = d > 0 ? (s - c0) / d : 0.0;
    const GlobalPoint2D P = pts[tk.point_off + lo];
    const GlobalPoint2D Q = pts[tk.point_off + (lo + 1 < tk.n_points ? lo + 1 : 0)];      // (the closing segment ends on point 0)
    ObPoint o;
    o.x = P.x + t * (Q.x - P.x); o.y = P.y + t * (Q.y - P.y); o.type = pin.type; o.radius = pin.radius;
    obs[pin.pool] = o;
    if (mot) { ObMotion z; z.vx = 0; z.vy = 0; mot[pin.pool] = z; }
}

}  // namespace dmpp
