"""ctypes harness of the C++ class surface (libdmpp_host.so: CShare / CPlanning / CDecision over libdmpp.so).

The class surface is what a caller written against the reference's Planning.h / Decision.h links; this module drives
it through the library's few `extern "C"` entry points (host/dmpp_host.cpp) so that tests and bench.py can compare
CDecision::decide -> CPlanning::plan with the oracle and time it.  Nothing here computes planning results."""
import ctypes as C
import os
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libdmpp_host.so")


class HostMembers(C.Structure):          # DmppHostMembers: CPlanning's public members (Planning.h:42-52)
    _fields_ = [("path_lat_dis", C.c_double), ("remain_dis", C.c_double), ("path_dir_err", C.c_double), ("brakespeed", C.c_double),
                ("des_acc", C.c_double), ("afresh_planning", C.c_int32), ("afresh_cause", C.c_int32), ("path_near_id", C.c_int32),
                ("path_front_near_id", C.c_int32), ("his_behavior", C.c_int32), ("acc_flag", C.c_int32)]


_host = None


def load():
    global _host
    if _host is not None:
        return _host
    if not os.path.exists(HOST_LIB_PATH):
        raise OSError(f"{HOST_LIB_PATH} not found: make -C decision-making-and-path-planning_amd/host")
    L = C.CDLL(HOST_LIB_PATH)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    L.dmpp_host_start.restype = ci
    L.dmpp_host_error.restype = C.c_char_p
    L.dmpp_host_config.restype = vp
    L.dmpp_host_reset.argtypes = [ci]
    L.dmpp_host_set_map.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, cd, vp, ci, vp]
    L.dmpp_host_tick.argtypes = [vp, vp, ci, vp, ci, ci, cd, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.dmpp_host_plan.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, vp, vp]
    L.dmpp_host_set_grid_frame.argtypes = [cd, cd, cd, cd]
    L.dmpp_host_planning_state.restype = vp
    L.dmpp_host_decision_state.restype = vp
    _host = L
    return L


class HostSurface:
    """One ego on the class surface: SetMap once, then tick() = CDecision::decide -> CPlanning::plan."""

    def __init__(self, dm, cfg):
        self.dm = dm
        self.L = load()
        dst = np.frombuffer((C.c_char * dm.PlannerConfig.itemsize).from_address(self.L.dmpp_host_config()), dm.PlannerConfig)
        dst[0] = np.array(cfg, dm.PlannerConfig).reshape(1)[0]           # CShare::Config(): read on every call
        rc = self.L.dmpp_host_start()
        if rc:
            raise dm.PlannerError(f"class surface: {self.L.dmpp_host_error().decode()}")
        self.L.dmpp_host_reset(1)

    def set_scene_map(self, sc, s=0):
        """The lane views of scene `s` of a gen_scenes-style batch as the LaneMap of both singletons."""
        dm = self.dm
        si = sc["scene_in"][s]
        lv = si["lanes"]

        def view(off, n):
            a = np.ascontiguousarray(sc["lane_pool"][int(off):int(off) + int(n)])
            return a, (a.ctypes.data if len(a) else None), len(a)
        cur, pc, nc = view(lv["cur_off"], lv["cur_n"])
        left, plf, nl = view(lv["left_off"], lv["left_n"])
        right, pr, nr = view(lv["right_off"], lv["right_n"])
        attr = np.ascontiguousarray(sc["attr_pool"][int(lv["cur_off"]):int(lv["cur_off"]) + int(lv["cur_n"])])
        out_lanes = np.ascontiguousarray(si["out_lane_no"])
        self.L.dmpp_host_set_grid_frame(float(si["grid_origin"]["x"]), float(si["grid_origin"]["y"]), float(si["goal"]["x"]), float(si["goal"]["y"]))
        self.L.dmpp_host_set_map(pc, nc, plf, nl, pr, nr, int(lv["lane_sum"]), int(lv["lanechg_attribute"]), float(lv["lane_width"]),
                                 attr.ctypes.data if len(attr) else None, len(attr), out_lanes.ctypes.data)

    def tick(self, sc, s=0, want_grid=False):
        """decide -> plan on scene `s`: returns dict(dec, refpath, around, result, show, road_points, members[, grid])."""
        dm = self.dm
        si = sc["scene_in"][s]
        loc = np.ascontiguousarray(sc["scene_in"]["loc"][s:s + 1])
        obs = np.ascontiguousarray(sc["obs_pool"][int(si["obs_off"]):int(si["obs_off"]) + int(si["obs_n"])])
        pos = int(si["loc"]["pos"])
        junc = np.ascontiguousarray(sc["ref_pool"][int(si["ref_off"]):int(si["ref_off"]) + int(si["ref_n"])]) if pos in (1, 2) else np.zeros(0, dm.GlobalPoint2D)
        dec = np.zeros(1, dm.DecisionOutPod)
        ref = np.zeros(dm.MAX_REFPATH, dm.GlobalPoint2D)
        around = np.zeros(6, dm.Path_Obs)
        result, show = np.zeros(1, dm.PlanningOut), np.zeros(1, dm.PlanningStatus)
        road = np.zeros(dm.PATH_POINTS, dm.GlobalPoint2D)
        mem = HostMembers()
        grid = np.zeros(1, dm.GridOut) if want_grid else None
        rc = self.L.dmpp_host_tick(loc.ctypes.data, obs.ctypes.data if len(obs) else None, len(obs),
                                   junc.ctypes.data if len(junc) else None, len(junc), int(si["stub_attribute"]), float(si["period_last"]),
                                   dec.ctypes.data, ref.ctypes.data, len(ref), around.ctypes.data, result.ctypes.data, show.ctypes.data,
                                   road.ctypes.data, C.addressof(mem), grid.ctypes.data if want_grid else None)
        self.last_code = rc          # CShare::LastStatus().code of the call (0, or a PP_ERR_* value)
        if rc:
            raise dm.PlannerError(f"class surface: {self.L.dmpp_host_error().decode()}")
        out = dict(dec=dec[0], refpath=ref[:int(dec["refpath_n"][0])], around=around, result=result[0], show=show[0], road_points=road,
                   members={f: getattr(mem, f) for f, _ in HostMembers._fields_})
        if want_grid:
            out["grid"] = grid[0]
        return out

    def planning_state(self):
        dm = self.dm
        return np.frombuffer((C.c_char * dm.SceneState.itemsize).from_address(self.L.dmpp_host_planning_state()), dm.SceneState).copy()

    def decision_state(self):
        dm = self.dm
        return np.frombuffer((C.c_char * dm.SceneState.itemsize).from_address(self.L.dmpp_host_decision_state()), dm.SceneState).copy()


def p50_plan_ms(dm, cfg, sc, device=0, ticks=200, want_grid=True):
    """p50 wall time of CPlanning::plan(...) at batch 1 (the literal drop-in call), in milliseconds: DecisionOut from one
    CDecision::decide, then `ticks` plan() calls on the same inputs (grid stage as in `cfg`)."""
    os.environ.setdefault("DMPP_DEVICE", str(device))
    hs = HostSurface(dm, cfg)
    hs.set_scene_map(sc, 0)
    first = hs.tick(sc, 0, want_grid=want_grid)
    si = sc["scene_in"][0]
    loc = np.ascontiguousarray(sc["scene_in"]["loc"][0:1])
    obs = np.ascontiguousarray(sc["obs_pool"][int(si["obs_off"]):int(si["obs_off"]) + int(si["obs_n"])])
    dec = np.array([first["dec"]], dm.DecisionOutPod)
    ref = np.ascontiguousarray(first["refpath"])
    result, show = np.zeros(1, dm.PlanningOut), np.zeros(1, dm.PlanningStatus)
    road = np.zeros(dm.PATH_POINTS, dm.GlobalPoint2D)
    grid = np.zeros(1, dm.GridOut)
    args = (dec.ctypes.data, ref.ctypes.data if len(ref) else None, len(ref), loc.ctypes.data, obs.ctypes.data if len(obs) else None, len(obs),
            result.ctypes.data, show.ctypes.data, road.ctypes.data, grid.ctypes.data if want_grid else None)
    for _ in range(10):
        hs.L.dmpp_host_plan(*args)
    lat = []
    for _ in range(ticks):
        a = time.perf_counter()
        rc = hs.L.dmpp_host_plan(*args)
        lat.append((time.perf_counter() - a) * 1e3)
        if rc:
            raise dm.PlannerError(f"class surface: {hs.L.dmpp_host_error().decode()}")
    return float(np.percentile(lat, 50))
