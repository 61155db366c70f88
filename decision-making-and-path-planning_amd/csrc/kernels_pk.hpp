// kernels_pk.hpp — packed streamed fetch: two kernels that pack a tick's results into PackedPlan / PackedGrid
// records on the device, and the host functions that unpack them again.  Lossless: the unpackers are made from the functions the
// kernels themselves call (dev_geom.hpp: cell_centre, CalcDistance, serial_prefix_inplace, mean_point, bezier_point,
// global_to_wgs84), and the library is built with -ffp-contract=off, so +, -, *, / and sqrt round on the host as on the device.
#pragma once
#include <cstring>
#include "dev_geom.hpp"
#include "kernels_s.hpp"

namespace dmpp {

// ---------------------------------------------------------------------------------------
// PlanOut -> PackedPlan: a strided gather, 16 bytes per lane.  A PackedPlan is kPkPlanChunks chunks of 16 bytes, every one of
// them a 16-byte-aligned run of its PlanOut record except two: chunk 4 ends in show.afresh_cause (in the place of result._pad),
// chunk 6 is planacc, trafficlight, ob_flag.
constexpr int kPkChunk = 16;
constexpr int kPkPlanChunks = (int)(sizeof(PackedPlan) / kPkChunk);
constexpr int kPkBlock = 256;
static_assert(sizeof(PackedPlan) == 1744 && sizeof(PackedPlan) % kPkChunk == 0 && sizeof(PlanOut) % kPkChunk == 0, "PackedPlan: whole 16-byte chunks");
static_assert(offsetof(PackedPlan, afresh_cause) == offsetof(PlanningOut, _pad) && offsetof(PlanningOut, _pad) == 76 && offsetof(PlanningOut, pnts) == 80,
              "PackedPlan starts with the first 80 bytes of PlanningOut, afresh_cause in the place of _pad");
static_assert(offsetof(PackedPlan, near_ob_dist) == 80 && offsetof(PackedPlan, planacc) == 96 && offsetof(PackedPlan, trafficlight) == 104 &&
              offsetof(PackedPlan, ob_flag) == 108 && offsetof(PackedPlan, dec) == 112 && offsetof(PackedPlan, path_points) == 144, "PackedPlan layout (DESIGN.md §4r)");
static_assert((offsetof(PlanOut, show) + offsetof(PlanningStatus, near_ob_dist)) % kPkChunk == 0 && offsetof(PlanningStatus, planacc) == 16 &&
              (offsetof(PlanOut, show) + offsetof(PlanningStatus, path_points)) % kPkChunk == 0 && offsetof(PlanOut, dec) % kPkChunk == 0 &&
              sizeof(DecisionOutPod) == 2 * kPkChunk, "k_pack_plan: the runs it copies start on 16-byte boundaries of PlanOut");

__global__ void __launch_bounds__(kPkBlock)
k_pack_plan(int n, const PlanOut* __restrict__ plan, PackedPlan* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * kPkBlock + threadIdx.x;
    const int scene = (int)(t / kPkPlanChunks), j = (int)(t - (long long)scene * kPkPlanChunks);
    if (scene >= n) return;
    const PlanOut& po = plan[scene];
    const uint4* src = reinterpret_cast<const uint4*>(&po);
    constexpr int kShow = (int)((offsetof(PlanOut, show) + offsetof(PlanningStatus, near_ob_dist)) / kPkChunk);
    constexpr int kPts = (int)((offsetof(PlanOut, show) + offsetof(PlanningStatus, path_points)) / kPkChunk);
    constexpr int kDec = (int)(offsetof(PlanOut, dec) / kPkChunk);
    uint4 v;
    if (j < 4) v = src[j];                                         // the six doubles, cnt .. desstrVd
    else if (j == 4) { v = src[4]; v.w = (unsigned)po.show.afresh_cause; }      // light, road_type, sstop | afresh_cause
    else if (j == 5) v = src[kShow];                               // near_ob_dist, planspeed
    else if (j == 6) {                                             // planacc | trafficlight | ob_flag
        const uint2 pa = *reinterpret_cast<const uint2*>(&po.show.planacc);
        v.x = pa.x; v.y = pa.y; v.z = (unsigned)po.show.trafficlight; v.w = (unsigned)po.ob_flag;
    }
    else if (j < 9) v = src[kDec + (j - 7)];                       // dec
    else v = src[kPts + (j - 9)];                                  // path_points
    reinterpret_cast<uint4*>(out + scene)[j] = v;
}

// ---------------------------------------------------------------------------------------
// GridOut (+ the path cells and the SceneIn record of the tick) -> PackedGrid: one wave per scene, behind the scoring pass of the
// tick on its stream.  The winner's control points are recomputed from the inputs score_body read, by the functions it calls
// (lattice_terminal, lattice_bezier; sincos of the same angles on the same device gives the same bits).  The steps of the
// grid-path prefix are wave-native: lane l of block q holds step 64 q + l, and each plane is one ballot.  No LDS, no atomics.
constexpr int kPkGridWaves = 4;
constexpr int kPkGridWords = (int)(sizeof(PackedGrid) / 8);
static_assert(sizeof(PackedGrid) == 248 && kPkGridWords <= DMPP_WAVE && offsetof(GridOut, cand_cost) == 48 && offsetof(PackedGrid, best_cost) == 48 &&
              offsetof(PackedGrid, kind) == 80 && offsetof(PackedGrid, geo) == 88 && offsetof(PackedGrid, planes) == 152 && sizeof(GridOut) % 8 == 0,
              "PackedGrid: 31 words of 8 bytes, one per lane (DESIGN.md §4r)");
static_assert(DMPP_PATH_POINTS - 1 <= 4 * DMPP_WAVE - 1 && 3 * 4 == sizeof(((PackedGrid*)0)->planes) / 8, "k_pack_grid: up to 199 steps in four blocks of 64, three planes each");
// direction code of a step (dx, dy), dx, dy in -1 .. 1, at nibble (dy + 1) * 3 + (dx + 1); 15: no step
//   (1,0) 0   (1,1) 1   (0,1) 2   (-1,1) 3   (-1,0) 4   (-1,-1) 5   (0,-1) 6   (1,-1) 7
constexpr unsigned long long kPkDirCodes = 0x1230F4765ull;

__global__ void __launch_bounds__(kPkGridWaves * DMPP_WAVE)
k_pack_grid(PlannerConfig c, int n, const TickGroup g, int slot, PackedGrid* __restrict__ out)
{
    const int lane = threadIdx.x & (DMPP_WAVE - 1);
    const int scene = blockIdx.x * kPkGridWaves + (threadIdx.x >> 6);
    if (scene >= n) return;                                        // (whole waves)
    const SceneIn& si = g.in[scene];
    const GridOut& go = g.gout[slot * g.gout_stride + scene];
    const int32_t* __restrict__ path = g.paths + slot * g.path_stride + (size_t)scene * c.max_path;
    const int W = c.grid_w;
    const long long cells = (long long)c.grid_w * c.grid_h;
    const int status = go.status, path_len = go.path_len, nc = go.n_candidates;
    const int best = clampi(go.best_candidate, 0, DMPP_MAX_LATTICE - 1);      // (a fence: k_score writes 0 .. n_candidates - 1)
    const bool have_path = (status == DMPP_G_FOUND) && path_len >= 1;
    const int nl = min(c.n_lattice, DMPP_MAX_LATTICE - 1);
    int a = 0;                                                     // as score_body computes it
    if (have_path) {
        a = min(path_len - 1, c.lookahead_cells);
        if (a > DMPP_PATH_POINTS - 1) a = DMPP_PATH_POINTS - 1;
        a = clampi(a, 0, max(c.max_path - 1, 0));                  // (a fence for the reads below: a < path_len <= max_path)
    }
    const int kind = nc <= 0 ? DMPP_PACKED_NONE : (best < nl ? DMPP_PACKED_LATTICE : DMPP_PACKED_PATH);
    const GlobalPoint2D org = si.grid_origin;
    double geo[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    unsigned long long planes[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    int bad = 0, n_steps = 0;
    if (kind == DMPP_PACKED_LATTICE) {
        const GlobalPoint3D ego = si.loc.globalpoint;
        GlobalPoint2D pa0 = { 0.0, 0.0 }, pa = { 0.0, 0.0 }, T;
        if (have_path) { pa0 = cell_centre(c, org, path[max(a - 4, 0)], W); pa = cell_centre(c, org, path[a], W); }
        const double thT = lattice_terminal(c, ego, si.goal, have_path, a, pa0, pa, T);
        const double ang = (lane == 0 ? ego.dir : thT) * c.PI / 180;       // lane 0: the start heading, the others: the terminal one
        double sv, cv;
        sincos(ang, &sv, &cv);
        const Bezier bz = lattice_bezier(c, ego, T, readlane_f64(cv, 0), readlane_f64(sv, 0), readlane_f64(cv, 1), readlane_f64(sv, 1), best, nl);
        geo[0] = bz.x0; geo[1] = bz.y0; geo[2] = bz.x1; geo[3] = bz.y1; geo[4] = bz.x2; geo[5] = bz.y2; geo[6] = bz.x3; geo[7] = bz.y3;
    } else if (kind == DMPP_PACKED_PATH) {
        geo[0] = org.x; geo[1] = org.y;
        n_steps = a;
        bool wrong = path[0] != go.start_cell;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = q * DMPP_WAVE + lane;
            int d = 0;
            if (i < a) {                                           // step i: cell i -> cell i + 1 (i + 1 <= a < max_path)
                const int p0 = path[i], p1 = path[i + 1];
                int code = 15;
                if (p0 >= 0 && p0 < cells && p1 >= 0 && p1 < cells) {
                    const int dx = p1 % W - p0 % W, dy = p1 / W - p0 / W;
                    if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) code = (int)((kPkDirCodes >> (4 * ((dy + 1) * 3 + (dx + 1)))) & 15);
                }
                if (code == 15) wrong = true; else d = code;
            }
            planes[3 * q + 0] = wave_ballot((d & 1) != 0);
            planes[3 * q + 1] = wave_ballot((d & 2) != 0);
            planes[3 * q + 2] = wave_ballot((d & 4) != 0);
        }
        if (wave_ballot(wrong) != 0) bad = DMPP_PACKED_BAD;
    }
    // lane w stores word w of the record
    const unsigned long long* gw = reinterpret_cast<const unsigned long long*>(&go);
    unsigned long long v = 0;
    if (lane < 6) v = gw[lane];                                    // order_digest .. n_candidates
    else if (lane < 10) { if (nc > 0) v = gw[6 + DMPP_MAX_LATTICE * (lane - 6) + best]; }       // cand_cost / col / curv / prog [best]
    else if (lane == 10) v = (unsigned long long)(unsigned)(kind | bad) | ((unsigned long long)(unsigned)n_steps << 32);
#pragma unroll
    for (int k = 0; k < 8; k++) if (lane == 11 + k) v = (unsigned long long)__double_as_longlong(geo[k]);
#pragma unroll
    for (int k = 0; k < 12; k++) if (lane == 19 + k) v = planes[k];
    if (lane < kPkGridWords) reinterpret_cast<unsigned long long*>(out + scene)[lane] = v;
}

// ---------------------------------------------------------------------------------------
// The unpackers: host code, one scene each.

inline void unpack_plan_one(const PlannerConfig& c, const PackedPlan& pk, PlanningOut* result, PlanningStatus* show, DecisionOutPod* dec)
{
    if (result) {
        std::memcpy(result, &pk, offsetof(PlanningOut, _pad));     // the six doubles and the seven ints
        result->_pad = 0;
        for (int k = 0; k < DMPP_OUT_POINTS; k++) result->pnts[k] = global_to_wgs84(c, pk.path_points[k]);
    }
    if (show) {
        show->near_ob_dist = pk.near_ob_dist; show->planspeed = pk.planspeed; show->planacc = pk.planacc;
        show->afresh_cause = pk.afresh_cause; show->trafficlight = pk.trafficlight;
        std::memcpy(show->path_points, pk.path_points, sizeof(pk.path_points));
    }
    if (dec) *dec = pk.dec;
}

// false: a record no tick packs (the output is zeroed).  Every check comes before the first write to *out, the points go straight
// into out->best_path, and only what the record does not determine is zeroed: no pass over the 3.8 KB of a GridOut but the writes.
inline bool unpack_grid_one(const PlannerConfig& c, const PackedGrid& pk, GridOut* out)
{
    const int kind = pk.kind, a = pk.n_steps, best = pk.best_candidate;
    GlobalPoint2D pts[DMPP_PATH_POINTS]; double cum[DMPP_PATH_POINTS];       // kind 2: the prefix in metres and its arc lengths
    bool ok = (kind == DMPP_PACKED_NONE || kind == DMPP_PACKED_LATTICE || kind == DMPP_PACKED_PATH) &&      // (not: unknown, or DMPP_PACKED_BAD)
              a >= 0 && a <= DMPP_PATH_POINTS - 1 && (kind == DMPP_PACKED_NONE || (best >= 0 && best <= DMPP_MAX_LATTICE - 1));
    if (ok && kind == DMPP_PACKED_PATH) {
        // the prefix: start_cell, then one neighbour per step; its cells in metres (cell_centre)
        const int W = c.grid_w, H = c.grid_h;
        ok = W > 0 && H > 0 && pk.start_cell >= 0 && (long long)pk.start_cell < (long long)W * H;
        if (ok) {
            static const int kDx[8] = { 1, 1, 0, -1, -1, -1, 0, 1 }, kDy[8] = { 0, 1, 1, 1, 0, -1, -1, -1 };
            const GlobalPoint2D org = { pk.geo[0], pk.geo[1] };
            int x = pk.start_cell % W, y = pk.start_cell / W;
            pts[0] = cell_centre(c, org, pk.start_cell, W);
            for (int i = 0; i < a && ok; i++) {
                const int w = 3 * (i >> 6), b = i & 63;
                const int d = (int)((pk.planes[w] >> b) & 1) | (int)((pk.planes[w + 1] >> b) & 1) << 1 | (int)((pk.planes[w + 2] >> b) & 1) << 2;
                x += kDx[d]; y += kDy[d];
                ok = x >= 0 && x < W && y >= 0 && y < H;
                if (ok) pts[i + 1] = cell_centre(c, org, y * W + x, W);
            }
        }
    }
    if (!ok) { std::memset(out, 0, sizeof(GridOut)); return false; }
    std::memcpy(out, &pk, offsetof(GridOut, cand_cost));            // order_digest .. n_candidates
    std::memset(out->cand_cost, 0, offsetof(GridOut, best_path) - offsetof(GridOut, cand_cost));
    if (kind != DMPP_PACKED_NONE) {
        out->cand_cost[best] = pk.best_cost; out->cand_col[best] = pk.best_col; out->cand_curv[best] = pk.best_curv; out->cand_prog[best] = pk.best_prog;
    }
    if (kind == DMPP_PACKED_NONE) std::memset(out->best_path, 0, sizeof(out->best_path));
    else if (kind == DMPP_PACKED_LATTICE) {
        Bezier bz;
        bz.x0 = pk.geo[0]; bz.y0 = pk.geo[1]; bz.x1 = pk.geo[2]; bz.y1 = pk.geo[3]; bz.x2 = pk.geo[4]; bz.y2 = pk.geo[5]; bz.x3 = pk.geo[6]; bz.y3 = pk.geo[7];
        for (int i = 0; i < DMPP_PATH_POINTS; i++) out->best_path[i] = bezier_point(bz, i, DMPP_PATH_POINTS);
    } else {
        // the arc lengths summed in index order (wave_cumlen: CalcDistance per segment, serial_prefix_inplace), the 200 points by mean_point
        const int n_in = a + 1;
        for (int i = 1; i < n_in; i++) cum[i] = CalcDistance(pts[i], pts[i - 1]);
        cum[0] = 0; serial_prefix_inplace(cum, 1, n_in, 0.0);
        for (int i = 0; i < DMPP_PATH_POINTS; i++) out->best_path[i] = mean_point(c, pts, cum, n_in, i, DMPP_PATH_POINTS);
    }
    return true;
}

}  // namespace dmpp
