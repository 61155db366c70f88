// kernels_op.hpp — the kernels of the stand-alone operators (pp_search_obstacle_batch, pp_geom_batch, pp_scalar_stage, pp_bezier,
// pp_mean_points, pp_create_new_path): one method of the reference on explicit arguments each, through the device functions
// the tick's kernels use (dev_geom.hpp, kernels_r.hpp).  The operands lie in the handle's scratch buffer.
#pragma once
#include "kernels_r.hpp"

namespace dmpp {

constexpr int kSoMaxPts = 2048;

__global__ void __launch_bounds__(DMPP_WAVE)
k_search_obstacle_batch(PlannerConfig c, int nq, const GlobalPoint2D* __restrict__ paths, const int32_t* __restrict__ path_off,
                        const ObPoint* __restrict__ obs, const int32_t* __restrict__ obs_off, const double* __restrict__ lo,
                        const double* __restrict__ hi, Path_Obs* __restrict__ out)
{
    __shared__ double s[kSoMaxPts];
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int lane = threadIdx.x;
    const int p0 = path_off[q], n = path_off[q + 1] - p0, o0 = obs_off[q], m = obs_off[q + 1] - o0;
    SoResult r = wave_search_obstacle(c, paths + p0, n, s, obs + o0, m, lo[q], hi[q], lane);
    if (lane == 0) store_path_obs(&out[q], r, obs + o0, true);
}

__global__ void k_geom_batch(PlannerConfig c, int op, int n, const GlobalPoint2D* a, const GlobalPoint2D* b, const GlobalPoint2D* cc, double* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 0) out[i] = GetLatDis(c, a[i], b[i], cc[i]);
    else if (op == 1) out[i] = GetRoadAngle(c, a[i], b[i]);
    else if (op == 2) out[i] = GetAngleErr(a[i].x, a[i].y);
    else if (op == 3) out[i] = CalcDistance(a[i], b[i]);
    else if (op == 4) out[i] = c.wgs_lat0 + a[i].y * c.wgs_deg_per_m_lat;      // GlobalToWGS84 .lat
    else out[i] = c.wgs_lng0 + a[i].x * c.wgs_deg_per_m_lng;                   // GlobalToWGS84 .lng
}

// One scalar stage of the planning tick on explicit arguments (the CPlanning methods of the same name).
//   op 0 UpdatePlanJudge : in = {last_behavior, behavior, pos, path_lat_dis, path_dir_err, remain_dis} -> out = {afresh, cause}
//   op 1 SpeedPlanning   : in = {pos, ob_flag, mindist_lon, faraim_dis, velocity_expect, brake_speed, acc_flag, des_acc} -> out = {brake_speed, acc_flag, des_acc}
//   op 2 CalculateRadius : in = {path_near_id, path_front_near_id}, pts = last_Bpoints[200] -> out = {radius}
__global__ void k_scalar_stage(PlannerConfig c, int op, const double* in, const GlobalPoint2D* pts, double* out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (op == 0) {
        int cause = 0;
        const int afresh = d_UpdatePlanJudge(c, (int)in[0], (int)in[1], (int)in[2], in[3], in[4], in[5], cause);
        out[0] = afresh; out[1] = cause;
    } else if (op == 1) {
        double bs = in[5], da = in[7]; int af = (int)in[6];
        d_SpeedPlanning((int)in[0], (int)in[1], in[2], (float)in[3], in[4], bs, af, da);
        out[0] = bs; out[1] = af; out[2] = da;
    } else {
        out[0] = d_CalculateRadius(pts, (int)in[0], (int)in[1]);
    }
}

__global__ void k_bezier(PlannerConfig c, GlobalPoint3D s, GlobalPoint3D e, GlobalPoint2D* out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Bezier bz = bezier_setup(c, s, e);
    out[i] = bezier_point(bz, i, n);
}

__global__ void __launch_bounds__(DMPP_WAVE)
k_cumlen(const GlobalPoint2D* in, int n, double* cum) { wave_cumlen(in, n, cum, threadIdx.x); }

__global__ void k_mean_points(PlannerConfig c, const GlobalPoint2D* in, const double* cum, int n_in, GlobalPoint2D* out, int n_out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_out) out[k] = mean_point(c, in, cum, n_in, k, n_out);
}

__global__ void k_create_new_path(PlannerConfig c, const GlobalPoint2D* path, int n, double offset, GlobalPoint2D* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = offset_point(c, path, n, i, offset);
}

}  // namespace dmpp
