// kernels_score.hpp — G3: candidate scoring (specification: DESIGN.md §5, oracle/dmpp_grid_oracle.c).  One device function,
// score_body, called by the stand-alone k_score (kernels_g.hpp) for one scene per workgroup; the search kernel does not score.
// A candidate's points are never stored: a lane computes its own point of the current pass and takes the neighbours i - 1 and
// i + 1 of the curvature term from the adjacent lanes (a whole-wave DPP shift), so the workgroup's LDS holds only what the
// candidates are made from: 10 granules of 1,280 bytes, two scoring workgroups in the room a retiring search leaves.
#pragma once
#include "dev_geom.hpp"

namespace dmpp {

// G3.  256 threads = 4 waves per scene; wave w scores candidates w, w+4, ...
// NW waves per scene score the candidates NW at a time: 4 for batches (four scenes per CU), 16 for the few scenes of a
// latency-bound tick (17 candidates in 2 rounds instead of 5).
constexpr int kBoxWaves = 4;
constexpr int kTailRounds = 4;                        // packed fourth pass: candidates per wave
template <int NW> constexpr bool kPackTail = NW <= 4;
static_assert(DMPP_PATH_POINTS - 192 == 8 && kTailRounds * 8 <= DMPP_WAVE, "packed fourth pass: lane 8 c + j = point 192 + j of candidate c");
static_assert(DMPP_PATH_POINTS <= kBoxWaves * DMPP_WAVE && DMPP_MAX_LATTICE <= 32, "score_body: lane layouts");
constexpr int kMaxRelObs = 128;      // culled obstacle list kept in LDS; a scene with more candidates near its paths reads the whole list from HBM
// Many obstacles near the candidates (256-obstacle scenes keep ~10 - 30 after the cull): a coarse bucket grid over the box of
// the candidates, each culled obstacle entered into every bucket its cutoff disc can touch, so that a point only looks at the
// list of ITS bucket.  The clearance is a minimum over the obstacles within their cutoff of the point - every one of them is in
// the point's bucket - so the result is the same number (a minimum does not depend on the order or on extra far members).
constexpr int kBucketN = 12, kBucketCap = 12, kBucketMinObs = 8;
#ifdef DMPP_DEBUG_SEARCH
__device__ int g_dbg_score[8];       // debug build: scenes scored, sum of n_rel, bucketed, bucket overflow, not culled, max n_rel
// debug build: cycles since the kernel's first instruction, thread 0 of each work item, at the END of each phase (tools/dbg_score_timing.py):
// 0 entry (score_body reached), 1 inputs landed (path prefix converted), 2 set-up (terminal pose, sincos, wave_cumlen, lattice),
// 3 cull and buckets, 4 whole candidates, 5 packed pass, 6 left-over candidate, 7 winner and stores (= total)
constexpr int kDbgScoreItems = 4096, kDbgScorePhases = 8;
__device__ unsigned g_dbg_score_ph[kDbgScoreItems][kDbgScorePhases];
#define SCORE_MARK(slot) { if (threadIdx.x == 0 && blockIdx.x < kDbgScoreItems) g_dbg_score_ph[blockIdx.x][slot] = (unsigned)(clock64() - dbg_t0); }
#define SCORE_DBG_PARAM , long long dbg_t0
#else
#define SCORE_MARK(slot)
#define SCORE_DBG_PARAM
#endif
// What point_terms reads about the obstacles: the culled list and the bucket grid over it, contiguous.
struct ScoreLists {
    double rx[kMaxRelObs], ry[kMaxRelObs], rr[kMaxRelObs], rt2[kMaxRelObs];   // obstacles that can matter: x, y, radius, cutoff^2
    int bcnt[kBucketN * kBucketN];                             // bucket fill counts (beyond kBucketCap: the bucket's points take the plain loop)
    unsigned char bent[kBucketN * kBucketN][kBucketCap];       // indices into rx / ry / rr / rt2
};
// Per-lane partial sums of one quarter of a left-over candidate (one wave's).  They are written once every wave is past its
// last point_terms - the lists above are dead by then - and so lie over them.
struct ScorePart { double pen[DMPP_WAVE], k2[DMPP_WAVE]; int hit[DMPP_WAVE]; };
template <int NW>
struct ScoreShared {
    GlobalPoint2D pts[DMPP_PATH_POINTS];     // grid-path prefix in metres (lookahead_cells+1 <= 200)
    double cum[DMPP_PATH_POINTS];
    union { ScoreLists ls; ScorePart part[NW]; };              // (16 waves: the partial sums are the larger member)
    Bezier bz[DMPP_MAX_LATTICE];             // control points of the lattice candidates
    double trig[4];                          // cos, sin of the start heading; cos, sin of the terminal heading
    double bb[4];                            // box of all lattice candidates: x0, x1, y0, y1
    GlobalPoint2D T;                         // terminal point
    double cost[DMPP_MAX_LATTICE];
    int box[4][4];                           // per wave: min / max cell column and row of the grid-path prefix
    int best, n_rel;
};
static_assert(sizeof(ScorePart) * 4 <= sizeof(ScoreLists), "k_score<4>: the partial sums of the left-over candidate fit over the obstacle lists and buckets");
// A searching workgroup of the configs[1] launch budget holds 19 LDS granules of 1,280 bytes and six of them leave 14 of a CU's
// 128 free (dmpp::coresident_budget): one scoring workgroup starts beside six searches, and a retiring search frees room for 33
// granules, which is THREE scoring workgroups at 11 granules each.  (At 21 + 2 = 23, the policy's own budget, it is two.)
static_assert(sizeof(ScoreShared<4>) <= 11 * 1280, "k_score<4>: one workgroup in the 14 granules beside six searches, two per freed search slot even at the policy's budget");

// The value of the lane below / above in the wave; lane 0 / lane 63 keep their own.  A whole-wave DPP shift (wave_shr:1: lane l
// reads lane l - 1; wave_shl:1: lane l + 1) is one v_mov per dword, against an LDS-crossbar permute with its address and its wait.
__device__ __forceinline__ double lane_below_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_above_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_tree_sum(double acc)
{
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) acc += shfl_xor_f64(acc, sft);
    return acc;
}

// Scores the candidates of one scene and writes cand_* / best_* of its GridOut.  All NW waves of the workgroup; `status` and
// `path_len` are the search's results for the scene, `path` its cells, `gobs` / `m` the obstacle snapshot of the tick.
template <int NW>
__device__ __forceinline__ void score_body(const PlannerConfig& c, const SceneIn& si, const ObPoint* __restrict__ gobs, int m,
                                           const int32_t* __restrict__ path, GridOut& go, int status, int path_len, ScoreShared<NW>& sh SCORE_DBG_PARAM)
{
    SCORE_MARK(0)
    constexpr int kThreads = NW * DMPP_WAVE;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int W = c.grid_w;
    // Every global input is requested here, before the first of them is waited for: the scene's record, (in the caller) the
    // search's status and path length, the cell of the path prefix this thread would convert - whether or not there is a path:
    // the buffer holds max_path cells per scene, and without a path the value is not used - and the thread's obstacle record,
    // which the cull reads two barriers further down.  One round trip to memory instead of three dependent ones.
    static_assert(DMPP_PATH_POINTS <= kThreads, "one cell of the path prefix per thread");
    const GlobalPoint3D ego = si.loc.globalpoint;
    const GlobalPoint2D org = si.grid_origin, goal = si.goal;
    int pc_mine = 0;
    if (tid <= min(c.lookahead_cells, DMPP_PATH_POINTS - 1) && tid < c.max_path) pc_mine = path[tid];
    ObPoint o_mine; o_mine.x = 0; o_mine.y = 0; o_mine.radius = 0;
    if (tid < m) o_mine = gobs[tid];
    const bool have_path = (status == DMPP_G_FOUND) && path_len >= 1;
    const int nl = min(c.n_lattice, DMPP_MAX_LATTICE - 1);
    const int nc = nl + (have_path ? 1 : 0);
    const double half_w = 0.5 * c.Vehicle_Width;
    int a = 0;
    if (have_path) {
        a = min(path_len - 1, c.lookahead_cells);
        if (a > DMPP_PATH_POINTS - 1) a = DMPP_PATH_POINTS - 1;
        // the prefix in metres, and the box of its cells (per wave here, combined below): the path candidate lies inside it
        int cx0 = 0x7fffffff, cx1 = -1, cy0 = 0x7fffffff, cy1 = -1;
        if (tid <= a) {                    // (a < path_len <= max_path: the cell was read)
            const int px = pc_mine % W, py = pc_mine / W;
            sh.pts[tid] = cell_centre(c, org, pc_mine, W);
            cx0 = px; cx1 = px; cy0 = py; cy1 = py;
        }
        if (wave < kBoxWaves) {            // DMPP_PATH_POINTS <= 256 points: only the first four waves hold any
#pragma unroll
            for (int sft = 32; sft >= 1; sft >>= 1) {
                cx0 = min(cx0, __shfl_xor(cx0, sft, 64)); cx1 = max(cx1, __shfl_xor(cx1, sft, 64));
                cy0 = min(cy0, __shfl_xor(cy0, sft, 64)); cy1 = max(cy1, __shfl_xor(cy1, sft, 64));
            }
            if (lane == 0) { sh.box[wave][0] = cx0; sh.box[wave][1] = cx1; sh.box[wave][2] = cy0; sh.box[wave][3] = cy1; }
        }
    }
    SCORE_MARK(1)
    __syncthreads();                       // the prefix is in LDS
    // Between this barrier and the next, side by side: wave 0 sums the arc lengths of the prefix (lane 0's in-order sum of up to
    // 120 lengths, which only the grid-path candidate and a winning grid path need), and the last wave computes what is the
    // same for every candidate - the terminal pose, the sine and cosine of the start and terminal headings (lane 0 takes the
    // start heading, lane 1 the terminal one, so one pass through sincos yields all four values) - and then the lattice.
    if (have_path && wave == 0) wave_cumlen(sh.pts, a + 1, sh.cum, lane);
    if (wave == NW - 1) {
        // the terminal is the prefix's last cell and the baseline starts four cells before it: sh.pts holds both, by the
        // expressions that would convert the cells here (lattice_terminal, shared with k_pack_grid)
        GlobalPoint2D T;
        const double thT = lattice_terminal(c, ego, goal, have_path, a, sh.pts[max(a - 4, 0)], sh.pts[a], T);
        const double ang = (lane == 0 ? ego.dir : thT) * c.PI / 180;
        double sv, cv;
        sincos(ang, &sv, &cv);
        if (lane == 0) { sh.trig[0] = cv; sh.trig[1] = sv; sh.T = T; }
        if (lane == 1) { sh.trig[2] = cv; sh.trig[3] = sv; }
        wave_sync();                       // (the same wave reads them back)
        // ---- the lattice: candidate k is the cubic Bezier of BezierPlanning(ego -> terminal k) (as bezier_setup); lane k of the
        //      last wave sets it up for every wave to read.  Obstacles that can matter at all lie inside the box of every candidate
        //      grown by their cutoff: a Bezier lies in the hull of its control points. ----
        double X0 = __builtin_inf(), X1 = -__builtin_inf(), Y0 = __builtin_inf(), Y1 = -__builtin_inf();
        if (lane < nl) {
            const double c0 = sh.trig[0], s0 = sh.trig[1], cs = sh.trig[2], sn = sh.trig[3];
            const Bezier bz = lattice_bezier(c, ego, sh.T, c0, s0, cs, sn, lane, nl);
            sh.bz[lane] = bz;
            X0 = fmin(fmin(bz.x0, bz.x1), fmin(bz.x2, bz.x3)); X1 = fmax(fmax(bz.x0, bz.x1), fmax(bz.x2, bz.x3));
            Y0 = fmin(fmin(bz.y0, bz.y1), fmin(bz.y2, bz.y3)); Y1 = fmax(fmax(bz.y0, bz.y1), fmax(bz.y2, bz.y3));
        }
#pragma unroll
        for (int sft = 16; sft >= 1; sft >>= 1) {          // DMPP_MAX_LATTICE <= 32 candidates: lanes 0..31
            X0 = fmin(X0, shfl_xor_f64(X0, sft)); X1 = fmax(X1, shfl_xor_f64(X1, sft));
            Y0 = fmin(Y0, shfl_xor_f64(Y0, sft)); Y1 = fmax(Y1, shfl_xor_f64(Y1, sft));
        }
        if (lane == 0) { sh.bb[0] = X0; sh.bb[1] = X1; sh.bb[2] = Y0; sh.bb[3] = Y1; sh.n_rel = 0; }
    }
    __syncthreads();
    SCORE_MARK(2)
    double X0 = sh.bb[0], X1 = sh.bb[1], Y0 = sh.bb[2], Y1 = sh.bb[3];
    if (have_path) {
        // the box of the path's own cells (not a box around the ego: an ego outside the grid is clamped to a border cell),
        // one cell wider - the resampled points lie on the segments between the cell centres
        int cx0 = 0x7fffffff, cx1 = -1, cy0 = 0x7fffffff, cy1 = -1;
        for (int w = 0; w < (NW < kBoxWaves ? NW : kBoxWaves); w++) {
            cx0 = min(cx0, sh.box[w][0]); cx1 = max(cx1, sh.box[w][1]); cy0 = min(cy0, sh.box[w][2]); cy1 = max(cy1, sh.box[w][3]);
        }
        X0 = fmin(X0, org.x + ((double)cx0 - 0.5) * c.cell); X1 = fmax(X1, org.x + ((double)cx1 + 1.5) * c.cell);
        Y0 = fmin(Y0, org.y + ((double)cy0 - 0.5) * c.cell); Y1 = fmax(Y1, org.y + ((double)cy1 + 1.5) * c.cell);
    }
    // the obstacles near the candidates, collected in LDS (kMaxRelObs of them); when more qualify, the scoring loop reads the
    // whole list from HBM instead (the same minimum over the same thresholds either way).  A thread's first record was
    // requested at the top: up to kThreads obstacles there is nothing left to load here.
    for (int j = tid; j < m; j += kThreads) {
        const ObPoint o = j == tid ? o_mine : gobs[j];
        const double thr = (double)o.radius + half_w + c.d_safe;
        if (o.x >= X0 - thr && o.x <= X1 + thr && o.y >= Y0 - thr && o.y <= Y1 + thr) {
            const int q = atomicAdd(&sh.n_rel, 1);           // order is irrelevant: only a minimum is taken
            if (q < kMaxRelObs) { sh.ls.rx[q] = o.x; sh.ls.ry[q] = o.y; sh.ls.rr[q] = (double)o.radius; sh.ls.rt2[q] = thr * thr; }
        }
    }
    __syncthreads();
    const bool culled = sh.n_rel <= kMaxRelObs;
    const int n_rel = culled ? sh.n_rel : m;
    // ---- bucket grid (uniform decision per scene) ----
    const double inv_bx = (X1 > X0) ? (double)kBucketN / (X1 - X0) : 0.0, inv_by = (Y1 > Y0) ? (double)kBucketN / (Y1 - Y0) : 0.0;
    auto bucket_x = [&](double v) { return clampi((int)floor((v - X0) * inv_bx), 0, kBucketN - 1); };      // monotone in v: the obstacle's range and the
    auto bucket_y = [&](double v) { return clampi((int)floor((v - Y0) * inv_by), 0, kBucketN - 1); };      // point's bucket come from the same expression
    // culled scenes: entries index the LDS list; a scene with more than kMaxRelObs obstacles near its candidates (not culled) is
    // bucketed straight from the snapshot in HBM (entries index it: <= 256 obstacles), so that its points read a few records
    // instead of all of them.  A bucket that overflows sends only ITS points to the plain loop.
    const bool bucketed = culled ? n_rel >= kBucketMinObs : m <= 256;
    if (bucketed) {
        for (int i = tid; i < kBucketN * kBucketN; i += kThreads) sh.ls.bcnt[i] = 0;
        __syncthreads();
        for (int j = tid; j < n_rel; j += kThreads) {
            double ox, oy, r;
            if (culled) { ox = sh.ls.rx[j]; oy = sh.ls.ry[j]; r = sh.ls.rr[j]; }
            else { const ObPoint o = gobs[j]; ox = o.x; oy = o.y; r = (double)o.radius; }
            // the cutoff, a hair wider: a point exactly at the cutoff (where the penalty is zero anyway) stays inside
            const double thr = (r + half_w + c.d_safe) * (1.0 + 1e-9) + 1e-9;
            if (!(ox >= X0 - thr && ox <= X1 + thr && oy >= Y0 - thr && oy <= Y1 + thr)) continue;       // (always true for the culled list)
            const int bx0 = bucket_x(ox - thr), bx1 = bucket_x(ox + thr), by0 = bucket_y(oy - thr), by1 = bucket_y(oy + thr);
            for (int by = by0; by <= by1; by++)
                for (int bx = bx0; bx <= bx1; bx++) {
                    const int b = by * kBucketN + bx;
                    const int q = atomicAdd(&sh.ls.bcnt[b], 1);
                    if (q < kBucketCap) sh.ls.bent[b][q] = (unsigned char)j;
                }
        }
        __syncthreads();
    }
#ifdef DMPP_DEBUG_SEARCH
    if (tid == 0) {
        atomicAdd(&g_dbg_score[0], 1); atomicAdd(&g_dbg_score[1], sh.n_rel); atomicAdd(&g_dbg_score[2], bucketed ? 1 : 0);
        { int ov = 0; if (bucketed) for (int i = 0; i < kBucketN * kBucketN; i++) ov += sh.ls.bcnt[i] > kBucketCap; atomicAdd(&g_dbg_score[3], ov); }
        atomicAdd(&g_dbg_score[4], culled ? 0 : 1);
        atomicMax(&g_dbg_score[5], sh.n_rel);
    }
#endif
    SCORE_MARK(3)
    // Point i of candidate k: a lattice candidate by bezier_point (the basis weights come from t each time - keeping those of a
    // lane's four points cost 32 registers; keeping t alone, 8 registers, measured slower beside the searches), the grid-path
    // candidate by mean_point.  The same expressions whichever lane evaluates a point and for whatever it is wanted, so a
    // point has ONE value: as itself, as a neighbour, in the output.
    auto cand_point = [&](int k, int i) -> GlobalPoint2D {
        if (k < nl) return bezier_point(sh.bz[k], i, DMPP_PATH_POINTS);
        return mean_point(c, sh.pts, sh.cum, a + 1, clampi(i, 0, DMPP_PATH_POINTS - 1), DMPP_PATH_POINTS);
    };
    // the point of the lane below / above (all 64 lanes call these together); lane 0 / lane 63 get their own value back
    auto from_lane_below = [&](const GlobalPoint2D p) -> GlobalPoint2D { GlobalPoint2D r; r.x = lane_below_f64(p.x); r.y = lane_below_f64(p.y); return r; };
    auto from_lane_above = [&](const GlobalPoint2D p) -> GlobalPoint2D { GlobalPoint2D r; r.x = lane_above_f64(p.x); r.y = lane_above_f64(p.y); return r; };
    const double kk2_fenced = 0.001 * 0.001;           // R fenced to 1000
    // penalty and squared curvature of point i (= p) of a candidate; pa, pf: its points i - 1 and i + 1 (read for 1 <= i <= 198 only)
    auto point_terms = [&](int i, const GlobalPoint2D p, const GlobalPoint2D pa, const GlobalPoint2D pf, double& pen, double& kk2, bool& hit) {
        double clear = __builtin_inf();
        int nb = 0, b = 0;
        if (bucketed) { b = bucket_y(p.y) * kBucketN + bucket_x(p.x); nb = sh.ls.bcnt[b]; }
        if (bucketed && nb <= kBucketCap) {
            for (int e = 0; e < nb; e++) {
                const int j = sh.ls.bent[b][e];
                double ox, oy, r, t2;
                if (culled) { ox = sh.ls.rx[j]; oy = sh.ls.ry[j]; r = sh.ls.rr[j]; t2 = sh.ls.rt2[j]; }
                else { ox = gobs[j].x; oy = gobs[j].y; r = (double)gobs[j].radius; const double thr = r + half_w + c.d_safe; t2 = thr * thr; }
                const double dx = p.x - ox, dy = p.y - oy;
                const double d2 = dx * dx + dy * dy;
                if (d2 > t2) continue;
                const double v = sqrt(d2) - r;
                if (v < clear) clear = v;
            }
        } else if (__builtin_expect(culled, 1)) {
            for (int j = 0; j < n_rel; j++) {
                const double dx = p.x - sh.ls.rx[j], dy = p.y - sh.ls.ry[j];
                const double d2 = dx * dx + dy * dy;
                if (d2 > sh.ls.rt2[j]) continue;                 // cannot produce a penalty (no sqrt needed)
                const double v = sqrt(d2) - sh.ls.rr[j];
                if (v < clear) clear = v;
            }
        } else {
            for (int j = 0; j < m; j++) {
                const double dx = p.x - gobs[j].x, dy = p.y - gobs[j].y;
                const double d2 = dx * dx + dy * dy;
                const double thr = (double)gobs[j].radius + half_w + c.d_safe;
                if (d2 > thr * thr) continue;
                const double v = sqrt(d2) - (double)gobs[j].radius;
                if (v < clear) clear = v;
            }
        }
        clear = clear - half_w;
        hit = false;
        if (clear <= 0) { pen = 1000.0; hit = true; }
        else if (clear < c.d_safe) { const double qq = (c.d_safe - clear) / c.d_safe; pen = qq * qq; }
        else pen = 0;
        kk2 = 0;
        if (i >= 1 && i <= DMPP_PATH_POINTS - 2) {
            // (1 / R)^2 of the circumradius of (P[i-1], P[i], P[i+1]), R = 0.5 * dis3 / sinA fenced to 1000 - from the
            // SQUARED side lengths, with one division and no square root:
            //   cosA = (d1 + d2 - d3) / (2 sqrt(d1 d2))   =>   sinA^2 = (4 d1 d2 - (d1 + d2 - d3)^2) / (4 d1 d2),
            //   (1 / R)^2 = sinA^2 / (0.25 d3) = (4 d1 d2 - (d1 + d2 - d3)^2) / (d1 d2 d3).
            // Against the oracle's sqrt / divide chain this differs by rounding only (<= ~1e-9 relative where sinA is at
            // its fence of 0.001, less elsewhere; the scores are compared to 1e-6) - except AT the fence, see below.
            const double d1 = (pa.x - p.x) * (pa.x - p.x) + (pa.y - p.y) * (pa.y - p.y);
            const double d2 = (p.x - pf.x) * (p.x - pf.x) + (p.y - pf.y) * (p.y - pf.y);
            const double d3 = (pa.x - pf.x) * (pa.x - pf.x) + (pa.y - pf.y) * (pa.y - pf.y);
            const double den2 = 4 * d1 * d2, num = d1 + d2 - d3;
            const double diff = den2 - num * num, fence = kk2_fenced * den2;        // sinA >= 0.001  <=>  diff >= fence
            kk2 = kk2_fenced;
            if (den2 > 0) {
                if (__builtin_expect(fabs(diff - fence) <= 1e-6 * fence, 0)) {
                    // The fence is a discontinuity of the specification (1 / R jumps from 0.001 to sinA / (0.5 dis3)), so the side a
                    // point falls on must be the oracle's own decision, not one taken from a differently rounded expression: where
                    // the squared form cannot tell (its rounding error is ~1e-9 of the fence for sides of similar length; this band is 1e-6) the
                    // oracle's chain of operations is evaluated as it stands.  About one point in 1e6 comes here
                    // (tests/test_oracle_properties.py replays both forms around the fence).
                    const double dis1 = sqrt(d1), dis2 = sqrt(d2), dis3 = sqrt(d3);
                    const double den = 2 * dis1 * dis2;
                    if (den > 0) {
                        const double cosA = (dis1 * dis1 + dis2 * dis2 - dis3 * dis3) / den;
                        const double sinA = sqrt(1 - cosA * cosA);
                        if (sinA >= 0.001) { const double R = 0.5 * dis3 / sinA; const double kq = 1 / R; kk2 = kq * kq; }
                    }
                } else if (diff > fence) kk2 = diff / (d1 * d2 * d3);
            }
        }
    };
    auto publish = [&](int k, double off, double pen_acc, double k2_acc, int first_hit) {      // the whole wave
        const double col = wave_tree_sum(pen_acc), curv = wave_tree_sum(k2_acc);
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) first_hit = min(first_hit, __shfl_xor(first_hit, sft, 64));
        const double prog = (first_hit == DMPP_PATH_POINTS) ? 0.0 : (double)(DMPP_PATH_POINTS - first_hit) / (double)DMPP_PATH_POINTS;
        const double cost = c.w_col * col + c.w_curv * curv + c.w_prog * prog + c.w_off * fabs(off);
        if (lane == 0) { go.cand_col[k] = col; go.cand_curv[k] = curv; go.cand_prog[k] = prog; go.cand_cost[k] = cost; sh.cost[k] = cost; }
    };
    // Whole rounds: one candidate per wave.  What is left over (17 candidates on 4 waves leave one) is split by quarter of the
    // points, one quarter per wave, when the waves suffice (4 * left <= NW); the per-lane partial sums are then added in the
    // order of the quarters, which is the order one wave would have added them in.
    const int left = nc % NW, n_whole = (4 * left <= NW) ? nc - left : nc;
    // One whole candidate: passes 0 .. n_pass - 1 over its points (64 per pass).  The fourth pass holds only the points 192 .. 199:
    // a wave that scores several candidates (four waves per scene) leaves it out and runs ONE packed pass for all of them at the
    // end - lane 8 c + j takes point 192 + j of its c-th candidate - and then adds each term to the lane that would have added it
    // (lane j, after its three earlier terms: the order of the sums does not change).
    // (The loops over a wave's candidates and over a candidate's passes are NOT unrolled: point_terms is ~1,000 instructions, and
    // eighteen copies of it made this kernel 129 KB of code; rolled it is 36 KB and exactly as fast, alone and beside the searches.)
    // A lane holds point i = lane + 64 q in pass q; its neighbours are the points of the lanes beside it.  What lies across a
    // pass border is taken from the pass beyond it: the points of pass q + 1 are computed before pass q is scored (lane 0 of
    // them is point i + 1 of lane 63), and lane 63 of pass q stays behind as point i - 1 of lane 0 of pass q + 1.
    auto whole_candidate = [&](int k, int n_pass, double& off, double& pen_acc, double& k2_acc, int& first_hit) {
        off = 0;
        if (k < nl) off = (double)(k - (nl - 1) / 2) * c.lattice_step;
        pen_acc = 0; k2_acc = 0; first_hit = DMPP_PATH_POINTS;
        GlobalPoint2D P = cand_point(k, lane), below = P;      // below: point 64 q - 1 (pass 0: not read, point 0 has no curvature term)
#pragma nounroll
        for (int q = 0; q < n_pass; q++) {
            const int i = lane + 64 * q;
            GlobalPoint2D N = P;
            if (64 * (q + 1) < DMPP_PATH_POINTS) N = cand_point(k, i + 64);       // (with the packed pass to come: point 192 for lane 63 of pass 2)
            GlobalPoint2D pa = from_lane_below(P), pf = from_lane_above(P);
            const GlobalPoint2D above = { readlane_f64(N.x, 0), readlane_f64(N.y, 0) };
            if (lane == 0) pa = below;
            if (lane == DMPP_WAVE - 1) pf = above;
            if (i < DMPP_PATH_POINTS) {
                double pen, kk2; bool hit;
                point_terms(i, P, pa, pf, pen, kk2, hit);
                pen_acc += pen; k2_acc += kk2;
                if (hit && i < first_hit) first_hit = i;
            }
            below.x = readlane_f64(P.x, DMPP_WAVE - 1); below.y = readlane_f64(P.y, DMPP_WAVE - 1);
            P = N;
        }
    };
    const int rounds = (n_whole - wave + NW - 1) / NW;                 // whole candidates of this wave
    const bool pack_tail = kPackTail<NW> && (n_whole + NW - 1) / NW >= 2 && (n_whole + NW - 1) / NW <= kTailRounds;       // (uniform over the block)
    {
        double accP[kTailRounds], accK[kTailRounds], accOff[kTailRounds]; int accH[kTailRounds];
#pragma unroll
        for (int t = 0; t < kTailRounds; t++) { accP[t] = 0; accK[t] = 0; accOff[t] = 0; accH[t] = DMPP_PATH_POINTS; }
#pragma nounroll
        for (int ci = 0; ci < rounds; ci++) {
            const int k = wave + ci * NW;
            double off, pen_acc, k2_acc; int first_hit;
            whole_candidate(k, pack_tail ? 3 : 4, off, pen_acc, k2_acc, first_hit);
            if (!pack_tail) publish(k, off, pen_acc, k2_acc, first_hit);
            else {
#pragma unroll
                for (int t = 0; t < kTailRounds; t++) if (t == ci) { accP[t] = pen_acc; accK[t] = k2_acc; accOff[t] = off; accH[t] = first_hit; }
            }
        }
        SCORE_MARK(4)
        if (pack_tail) {
            {   // the packed pass: lane 8 c + j = point 192 + j of candidate c.  Point 191, the neighbour of a candidate's first lane, is
                // evaluated for it; point 199 has no curvature term, so what its lane receives from the next candidate's is not read.
                const int cl = lane >> 3, i = 192 + (lane & 7);
                const int kc = wave + (cl < rounds ? cl : 0) * NW;             // lanes beyond the wave's candidates compute (and drop) its first one (rounds >= 1 here)
                double pen = 0, kk2 = 0; bool hit = false;
                const GlobalPoint2D p = cand_point(kc, i), p191 = cand_point(kc, 191);
                GlobalPoint2D pa = from_lane_below(p);
                const GlobalPoint2D pf = from_lane_above(p);
                if ((lane & 7) == 0) pa = p191;
                if (cl < rounds) point_terms(i, p, pa, pf, pen, kk2, hit);
                const int hv = hit ? i : DMPP_PATH_POINTS;
#pragma unroll
                for (int ci = 0; ci < kTailRounds; ci++) {
                    const double vp = shfl_f64(pen, 8 * ci + (lane & 7)), vk = shfl_f64(kk2, 8 * ci + (lane & 7));
                    const int vh = __shfl(hv, 8 * ci + (lane & 7), 64);
                    if (ci < rounds && lane < DMPP_PATH_POINTS - 192) { accP[ci] += vp; accK[ci] += vk; accH[ci] = min(accH[ci], vh); }
                }
            }
#pragma unroll
            for (int ci = 0; ci < kTailRounds; ci++) if (ci < rounds) publish(wave + ci * NW, accOff[ci], accP[ci], accK[ci], accH[ci]);
        }
    }
    SCORE_MARK(5)
    if (n_whole < nc) {
        // A left-over candidate by quarters: wave 4 j + q holds points 64 q .. 64 q + 63 of candidate n_whole + j.  The neighbours
        // inside the quarter come from the lanes beside; lanes 0 and 63 evaluate the one that belongs to the wave next door.
        const bool mine = wave < 4 * left;
        const int j = wave >> 2, q = wave & 3, k = n_whole + j, i = lane + 64 * q;
        double pen = 0, kk2 = 0; bool hit = false;
        if (mine) {                                        // (whole waves)
            const GlobalPoint2D p = cand_point(k, i), e = cand_point(k, lane == 0 ? i - 1 : i + 1);
            GlobalPoint2D pa = from_lane_below(p), pf = from_lane_above(p);
            if (lane == 0) pa = e;
            if (lane == DMPP_WAVE - 1) pf = e;
            if (i < DMPP_PATH_POINTS) point_terms(i, p, pa, pf, pen, kk2, hit);
        }
        __syncthreads();                                   // every wave is past its last point_terms: the obstacle lists and buckets are dead ...
        if (mine) { sh.part[wave].pen[lane] = pen; sh.part[wave].k2[lane] = kk2; sh.part[wave].hit[lane] = hit ? i : DMPP_PATH_POINTS; }      // ... and the partial sums lie over them
        __syncthreads();
        if (wave < left) {                                 // wave j2 = wave adds the quarters of left-over candidate j2 up, in order
            const int k2i = n_whole + wave;
            double pen_acc = 0, k2_acc = 0; int first_hit = DMPP_PATH_POINTS;
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
                if (lane + 64 * qq < DMPP_PATH_POINTS) {
                    const ScorePart& pt = sh.part[wave * 4 + qq];
                    pen_acc += pt.pen[lane]; k2_acc += pt.k2[lane]; first_hit = min(first_hit, pt.hit[lane]);
                }
            }
            const double off2 = k2i < nl ? (double)(k2i - (nl - 1) / 2) * c.lattice_step : 0.0;
            publish(k2i, off2, pen_acc, k2_acc, first_hit);
        }
    }
    __syncthreads();
    SCORE_MARK(6)
    if (tid == 0) {
        double best = 0; int bi = 0;
        for (int k = 0; k < nc; k++) if (k == 0 || sh.cost[k] < best) { best = sh.cost[k]; bi = k; }
        sh.best = bi; go.best_candidate = bi; go.n_candidates = nc;
        for (int k = nc; k < DMPP_MAX_LATTICE; k++) { go.cand_cost[k] = 0; go.cand_col[k] = 0; go.cand_curv[k] = 0; go.cand_prog[k] = 0; }
    }
    __syncthreads();
    {   // regenerate the winner into the output
        const int k = sh.best;
        if (tid < DMPP_PATH_POINTS) {
            GlobalPoint2D p = { 0.0, 0.0 };                 // no candidate at all (n_lattice = 0 and no grid path): zeros
            if (k < nl) {
                p = bezier_point(sh.bz[k], tid, DMPP_PATH_POINTS);
            } else if (nc > 0) p = mean_point(c, sh.pts, sh.cum, a + 1, tid, DMPP_PATH_POINTS);
            go.best_path[tid] = p;
        }
    }
    SCORE_MARK(7)
}

}  // namespace dmpp
