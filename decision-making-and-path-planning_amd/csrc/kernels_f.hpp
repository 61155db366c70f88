// kernels_f.hpp — fleet coupling (build-defined: the reference has no vehicle and no fleet): k_couple_fleet writes,
// into every scene's obstacle slice, the nearest egos of its own world at the poses of the input set being staged, so that the
// tick's kernels - which only ever read the obstacle list - react to peers with no change.
//
// One 64-lane wave per scene, four scenes per 256-thread block, no LDS, no barrier, no scratch (the shape of k_advance_egos).
// The lanes stride over the members of the scene's world and read 16 bytes of each SceneIn record (loc.globalpoint.x, .y).  A
// first pass marks which of a lane's members lie within range (one bit per stride step, 64 steps = worlds of up to 4096
// members; beyond that every step is looked at again); then c <= K rounds each take the smallest (d2, p) that is larger than
// the last one taken - a (value, index) wave minimum that keeps the lower index (wave_first_min) - looking only at the marked
// members.  Lane k keeps the peer of round k and writes slot k; lane 0 writes obs_off / obs_n.  The order (d2, p) is total and
// every operation is exact or correctly rounded (-ffp-contract=off), so the result is specified to the last bit.
#pragma once
#include "dev_geom.hpp"

namespace dmpp {

constexpr int kFleetScenes = 4;        // scenes (waves) per block of k_couple_fleet

struct FleetPin { int32_t obs_off, n_own; };      // a scene's pinned obstacle slice: its own entries; the K peer slots follow them

// range2 = fm.range * fm.range (rounded once, on the host).  in[] is read (x, y of every member) and written (obs_off, obs_n of
// the wave's own scene): different words, so the waves of a launch do not depend on each other.  mot: nullptr when the set
// carries no motion pool.
__global__ void __launch_bounds__(kBlock)
k_couple_fleet(int n_scenes, double range2, float radius, int K, const int32_t* __restrict__ world_first, const int32_t* __restrict__ world_of,
               const FleetPin* __restrict__ pin, SceneIn* in, ObPoint* __restrict__ obs, ObMotion* __restrict__ mot)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * kFleetScenes + (threadIdx.x >> 6);
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    const int w = world_of[s];
    const int p0 = world_first[w], p1 = world_first[w + 1];
    const FleetPin pn = pin[s];
    const double x = in[s].loc.globalpoint.x, y = in[s].loc.globalpoint.y;
    const bool self_ok = __builtin_isfinite(x) && __builtin_isfinite(y);
    auto dist2 = [&](int p) {
        const double dx = in[p].loc.globalpoint.x - x, dy = in[p].loc.globalpoint.y - y;
        return dx * dx + dy * dy;
    };
    // pass 1: bit i of `near` = this lane's member of stride step i is a candidate (steps >= 64 are not marked: always looked at)
    unsigned long long near = 0;
    if (self_ok && K > 0) {
        int i = 0;
        for (int p = p0 + lane; p < p1 && i < 64; p += 64, i++)
            if (p != s && dist2(p) <= range2) near |= 1ull << i;       // (a NaN distance compares false)
    }
    // rounds: the smallest (d2, p) above the last one taken
    double last_d = 0; int last_p = -1, mine = -1, c = 0;
    const bool long_world = p1 - p0 > 64 * 64;
    for (int k = 0; k < K; k++) {
        if (!self_ok) break;
        double md = 0; int mi = -1;
        auto look = [&](int p) {
            const double d = dist2(p);
            if (!(d <= range2)) return;
            if (last_p >= 0 && (d < last_d || (d == last_d && p <= last_p))) return;
            if (mi < 0 || d < md) { md = d; mi = p; }                   // (p rises within a lane: ties keep the lower index)
        };
        for (unsigned long long m = near; m; m &= m - 1) look(p0 + lane + 64 * (int)__builtin_ctzll(m));
        if (long_world)
            for (int p = p0 + lane + 64 * 64; p < p1; p += 64) if (p != s) look(p);
        wave_first_min(md, mi);
        if (mi < 0) break;                              // (wave-uniform: every lane holds the result)
        if (lane == k) mine = mi;
        if (mi >= p0 + lane && mi < p0 + lane + 64 * 64 && ((mi - p0 - lane) & 63) == 0) near &= ~(1ull << ((mi - p0 - lane) >> 6));
        last_d = md; last_p = mi; c = k + 1;
    }
    if (lane < c) {
        ObPoint o;
        o.x = in[mine].loc.globalpoint.x; o.y = in[mine].loc.globalpoint.y; o.type = (int32_t)(DMPP_OB_PEER | mine); o.radius = radius;
        obs[pn.obs_off + pn.n_own + lane] = o;
        if (mot) { ObMotion z; z.vx = 0; z.vy = 0; mot[pn.obs_off + pn.n_own + lane] = z; }
    }
    if (lane == 0) { in[s].obs_off = pn.obs_off; in[s].obs_n = pn.n_own + c; }
}

// pp_set_fleet(h, 0, ..): the resident records get their own slices back
__global__ void __launch_bounds__(kBlock)
k_fleet_restore(int n_scenes, const FleetPin* __restrict__ pin, SceneIn* __restrict__ in)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_scenes) return;
    in[s].obs_off = pin[s].obs_off; in[s].obs_n = pin[s].n_own;
}

}  // namespace dmpp
