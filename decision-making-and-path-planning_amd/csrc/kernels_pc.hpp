// kernels_pc.hpp — perception model (build-defined): while pp_set_perception is in force, k_perceive runs in the place
// of k_effective_obstacles on every tick of the handle.  It stores the truth snapshot exactly as that kernel does - from the one copy
// of effective_obstacle() - and beside it the PERCEIVED snapshot, the one Decision, Planning, the search and its scoring pass read.
//
//   k_perceive      : one 64-lane wave per scene, four scenes per 256-thread block, no LDS, no scratch, no atomics, no barrier (the
//                     shape of k_score_ego / k_couple_fleet).  The scene index is wave-uniform (readfirstlane), so the ego, its heading
//                     and the slice bounds are scalar.  The lanes stride the slice in chunks of 64, one entry per lane per chunk.  For
//                     occlusion the wave walks the slice a second time per chunk: every lane holds one candidate occluder of the inner
//                     chunk as (dx, dy, R^2, d2) and a wave-uniform loop broadcasts them one by one (v_readlane with a scalar lane
//                     index: the occluder lives in SGPRs) against the 64 targets; a chunk with nothing in view skips the walk.  The
//                     counters are ballots (wave-uniform), the closest hidden entry one wave_first_min per scene; lane 0 folds both
//                     into the scene's PerceptionStats with plain stores.  A track is read and written by the one lane that owns
//                     its entry, and slices of different scenes do not overlap in what they own (§4w 4.).
//   k_percept_reset : tracks all zero, stats at their starting values (+inf, -1: not all zero bits).
#pragma once
#include "kernels_es.hpp"      // spawn_mix (§4l), through it kernels_ep.hpp
#include "kernels_a.hpp"       // trk_heading (§4q), finite_f64
#include "kernels_r.hpp"       // effective_obstacle, kBlock

namespace dmpp {

constexpr int kPcScenes = 4;           // scenes (waves) per block of k_perceive

static_assert(sizeof(PerceptionModel) == 56 && offsetof(PerceptionModel, p_miss) == 32 && offsetof(PerceptionModel, seed) == 36 && offsetof(PerceptionModel, occlusion) == 40 &&
              offsetof(PerceptionModel, confirm) == 44 && offsetof(PerceptionModel, coast) == 48, "PerceptionModel layout (DESIGN.md §4w)");
static_assert(sizeof(PerceptTrack) == 32 && offsetof(PerceptTrack, hits) == 24 && offsetof(PerceptTrack, misses) == 26 && offsetof(PerceptTrack, confirmed) == 28,
              "PerceptTrack layout (DESIGN.md §4w)");
static_assert(sizeof(PerceptionStats) == 96 && offsetof(PerceptionStats, n_out) == 16 && offsetof(PerceptionStats, n_fresh) == 48 &&
              offsetof(PerceptionStats, min_hidden_clearance) == 72 && offsetof(PerceptionStats, min_hidden_tick) == 80 && offsetof(PerceptionStats, min_hidden_obs) == 88 &&
              offsetof(PerceptionStats, min_hidden_type) == 92, "PerceptionStats layout (DESIGN.md §4w)");

__global__ void __launch_bounds__(kBlock)
k_percept_reset(int n_scenes, PerceptionStats* __restrict__ stats, int n_tracks, PerceptTrack* __restrict__ tracks)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n_tracks) {
        PerceptTrack t;
        t.last.x = 0; t.last.y = 0; t.last.type = 0; t.last.radius = 0; t.hits = 0; t.misses = 0; t.confirmed = 0; t._pad[0] = 0; t._pad[1] = 0; t._pad[2] = 0;
        tracks[i] = t;
    }
    if (i < n_scenes) {
        PerceptionStats r;
        r.n_ticks = 0; r.n_entries = 0; r.n_out = 0; r.n_occluded = 0; r.n_missed = 0; r.n_detected = 0; r.n_fresh = 0; r.n_coasted = 0; r.n_hidden = 0;
        r.min_hidden_clearance = __builtin_huge_val(); r.min_hidden_tick = -1; r.min_hidden_obs = -1; r.min_hidden_type = 0;
        stats[i] = r;
    }
}

__device__ __forceinline__ int wave_count(bool p) { return __popcll(wave_ballot(p)); }

// §4w 3.: one standard normal deviate (to 1e-5 in variance, |n| <= 3.47) from the four 16-bit fields of a mixed word
__device__ __forceinline__ double percept_normal(unsigned long long w)
{
    const int a = (int)(w & 0xFFFFull) + (int)((w >> 16) & 0xFFFFull) + (int)((w >> 32) & 0xFFFFull) + (int)((w >> 48) & 0xFFFFull);
    return (double)(a - 131070) / 37837.0;
}

// obs_cap: entries of a snapshot set (and tracks); a slice outside it (no set call and no update lets one through) counts as empty.
// T: the tick's id.  ep_stats: EpisodeStats while episodes are on, else null.
__global__ void __launch_bounds__(kBlock)
k_perceive(PlannerConfig c, PerceptionModel pm, int n_scenes, int obs_cap, long long T, const SceneIn* __restrict__ in, const SceneState* __restrict__ st,
           const ObPoint* __restrict__ obs, const ObMotion* __restrict__ mot, const EpisodeStats* __restrict__ ep_stats,
           ObPoint* __restrict__ now, ObPoint* __restrict__ seen, PerceptTrack* __restrict__ tracks, PerceptionStats* __restrict__ stats)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * kPcScenes + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= n_scenes) return;                          // (whole waves leave: no barrier below)
    __builtin_amdgcn_s_setprio(3);                      // as k_effective_obstacles: every search waits for the front chain
    const SceneIn& si = in[s];
    const double x = si.loc.globalpoint.x, y = si.loc.globalpoint.y, dir = si.loc.globalpoint.dir;
    const int off = si.obs_off;
    int m = si.obs_n;
    if (off < 0 || m < 0 || (long long)off + (long long)m > (long long)obs_cap) m = 0;
    const double t = c.dyn_dt * (double)st[s].tick;
    const bool ego_ok = finite_f64(x) && finite_f64(y) && finite_f64(dir);
    double hx, hy;
    trk_heading(dir, hx, hy);
    const double r2 = pm.range * pm.range, half_width = 0.5 * c.Vehicle_Width;
    const bool all_round = pm.cos_half_fov <= -1.0;
    const bool fresh_scene = ep_stats && ep_stats[s].age == 0;
    const unsigned long long hs = spawn_mix((unsigned long long)pm.seed + (unsigned long long)s);
    int n_out = 0, n_occ = 0, n_miss = 0, n_det = 0, n_fresh = 0, n_coast = 0, n_hid = 0;      // wave-uniform
    double mv = 0; int mj = -1;                         // the closest hidden entry of this lane: first index of the smallest clearance
    for (int base = 0; base < m; base += 64) {
        const int j = base + lane;
        const bool act = j < m;
        ObPoint o; o.x = 0; o.y = 0; o.type = 0; o.radius = 0;
        if (act) { o = effective_obstacle(c, obs, mot, off + j, t); now[off + j] = o; }
        // 1. in view
        const double dx = o.x - x, dy = o.y - y;
        const double d2 = dx * dx + dy * dy;
        const double dist = sqrt(d2);
        const bool in_view = act && ego_ok && d2 <= r2 && (all_round || dx * hx + dy * hy >= pm.cos_half_fov * dist);
        // 2. occluded: some entry k of the slice, strictly nearer, whose disc the sight line to the centre passes through
        bool occluded = false;
        if (pm.occlusion != 0 && wave_ballot(in_view) != 0) {
            for (int base2 = 0; base2 < m; base2 += 64) {
                const int k = base2 + lane;
                double kdx = 0, kdy = 0, kd2 = 0, kR2 = 0;                  // (R^2 = 0: not an occluder)
                if (k < m) {
                    const ObPoint ok = effective_obstacle(c, obs, mot, off + k, t);
                    const double R = (double)ok.radius;
                    kdx = ok.x - x; kdy = ok.y - y; kd2 = kdx * kdx + kdy * kdy;
                    if (finite_f64(R) && R > 0) kR2 = R * R;
                }
                const int cnt = m - base2 < 64 ? m - base2 : 64;
                for (int q = 0; q < cnt; q++) {
                    const double sR2 = readlane_f64(kR2, q);
                    if (!(sR2 > 0)) continue;                               // (wave-uniform)
                    const double sdx = readlane_f64(kdx, q), sdy = readlane_f64(kdy, q), sd2 = readlane_f64(kd2, q);
                    if (sd2 < d2) {
                        double tt = (sdx * dx + sdy * dy) / d2;
                        if (tt > 0) {
                            if (tt > 1) tt = 1;
                            const double px = sdx - tt * dx, py = sdy - tt * dy;
                            if (px * px + py * py <= sR2) occluded = true;
                        }
                    }
                }
            }
        }
        // 3. missed
        const unsigned long long h0 = spawn_mix(spawn_mix(hs + (unsigned long long)j) + (unsigned long long)T);
        const bool missed = (unsigned)(h0 >> 32) < pm.p_miss;
        const bool detected = in_view && !occluded && !missed;
        n_out += wave_count(act && !in_view);
        n_occ += wave_count(in_view && occluded);
        n_miss += wave_count(in_view && !occluded && missed);
        n_det += wave_count(detected);
        // 4. the track of the pool entry
        bool fresh = false, coasted = false;
        if (act) {
            PerceptTrack tr = tracks[off + j];
            if (fresh_scene || tr.last.type != o.type || __float_as_uint(tr.last.radius) != __float_as_uint(o.radius)) {
                tr.last.x = 0; tr.last.y = 0; tr.hits = 0; tr.misses = 0; tr.confirmed = 0; tr._pad[0] = 0; tr._pad[1] = 0; tr._pad[2] = 0;
            }
            tr.last.type = o.type; tr.last.radius = o.radius;            // (what the next tick compares the slot's owner with)
            ObPoint out; out.x = DMPP_PERCEPT_HIDDEN_XY; out.y = DMPP_PERCEPT_HIDDEN_XY; out.type = o.type; out.radius = 0.0f;
            if (detected) {
                tr.hits = tr.hits < 65535 ? tr.hits + 1 : 65535; tr.misses = 0;
                if ((int)tr.hits > pm.confirm) tr.confirmed = 1;
                if (tr.confirmed) {
                    out = o;
                    const double sigma = pm.sigma0 + pm.sigma_gain * dist;
                    if (sigma > 0) {                                     // (sigma = 0: the truth's bytes, -0.0 included)
                        out.x = o.x + sigma * percept_normal(spawn_mix(h0 + 1ull));
                        out.y = o.y + sigma * percept_normal(spawn_mix(h0 + 2ull));
                    }
                    tr.last = out; fresh = true;
                }
            } else {
                tr.hits = 0;
                if (tr.confirmed) {
                    tr.misses = tr.misses < 65535 ? tr.misses + 1 : 65535;
                    if ((int)tr.misses <= pm.coast) { out = tr.last; coasted = true; }
                    else tr.confirmed = 0;
                }
            }
            tracks[off + j] = tr;
            seen[off + j] = out;
        }
        const bool hidden = act && !fresh && !coasted;
        n_fresh += wave_count(fresh); n_coast += wave_count(coasted); n_hid += wave_count(hidden);
        // 5. the closest thing the planner did not see (a NaN is never the minimum)
        if (hidden) {
            const double cl = dist - (double)o.radius - half_width;
            if (cl == cl && (mj < 0 || cl < mv)) { mv = cl; mj = j; }
        }
    }
    wave_first_min(mv, mj);
    if (lane != 0) return;
    PerceptionStats r = stats[s];
    r.n_ticks = r.n_ticks + 1; r.n_entries = r.n_entries + m;
    r.n_out = r.n_out + n_out; r.n_occluded = r.n_occluded + n_occ; r.n_missed = r.n_missed + n_miss; r.n_detected = r.n_detected + n_det;
    r.n_fresh = r.n_fresh + n_fresh; r.n_coasted = r.n_coasted + n_coast; r.n_hidden = r.n_hidden + n_hid;
    if (mj >= 0 && mv < r.min_hidden_clearance) {
        r.min_hidden_clearance = mv; r.min_hidden_tick = T; r.min_hidden_obs = mj; r.min_hidden_type = obs[off + mj].type;
    }
    stats[s] = r;
}

}  // namespace dmpp
