"""Ego tracking model (pp_set_ego_tracker): rollout egos keep a pose of their own and steer a bicycle model along the plan.

CPU: the ABI mirror and defaults, the heading polynomial, hand-derived known answers of one step on the numpy model
(tests/ego_track_model.py), and the closed loop of oracle tick + models on the ring of tests/route_scenes.py - the default tracker
crosses a junction with no replan of cause 2 or 3, a steering bias makes the planner replan on cause 2, which no run without a
tracker (and none with bias 0) ever does.
GPU: the known answers on k_advance_egos<true>, alone and as distinct scenes of launches of 5 and 7; k_advance_route<true> on the ring
against the model step by step; episodes; off is off; the error paths.

The steering known answers stand still (0 km/h towards 0 km/h: s = 0, ld = look_min = 3 m, on a path of 0.5 m spacing the target is
P[k0 + 6] to the bit - the walk ends exactly on a vertex, t = 1), so the ego's position, its heading and the target are whatever the
case writes and every expected value is worked out in the comment above its assertion."""
import math

import numpy as np
import pytest

import ego_model as em
import ego_track_backends as eb
import ego_track_model as etm
import map_scenes as ms
import route_scenes as rs
from test_rollout import _scene, _state
from test_route import _planner

gpu = pytest.mark.gpu
BAD_PATH, PATH_END = em.BAD_PATH, em.PATH_END


def _cfg(dm):
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    return cfg


def _tk(dm, **kw):
    tk = dm.default_ego_tracker()
    for k, v in kw.items():
        tk[k] = v
    return tk


def _fast(dm, **kw):
    """A tracker whose rate limit never binds in one step (curv_rate 100: 10 1/m per advance): kappa is the clamped command."""
    return _tk(dm, curv_rate=100.0, **kw)


def _path(dm, xs, ys, desspd=0.0):
    po = np.zeros(1, dm.PlanOut)
    po["road_points"]["x"][0], po["road_points"]["y"][0] = xs, ys
    po["result"]["desspd"] = desspd
    return po


def _north(dm, x=50.0, desspd=0.0):
    """A path up the line x = 50 from (50, 0) at 0.5 m spacing: standing on k0 = 0 the target is P[6] = (50, 3)."""
    return _path(dm, x, 0.5 * np.arange(200), desspd)


def _east(dm, x0=100.0, y=0.0, desspd=36.0):
    """A path along +x from (x0, y) at 0.5 m spacing; at 36 km/h towards 36 km/h the ego goes s = 1 m and looks ld = 3 + 0.5 * 10 = 8 m."""
    return _path(dm, x0 + 0.5 * np.arange(200), y, desspd)


class _Adv:
    """One scene on k_advance_egos<true> / the model: three straight lanes in slice mode, the ego wherever the case puts it."""
    def __init__(self, dm, name, log=None):
        self.dm, self.name, self.log = dm, name, log

    def steps(self, tk, pose, steps, v=0.0, model=None):
        """pose: (x, y, dir) of the ego; steps: (PlanOut, k0) or (PlanOut, k0, update) with update a dict of loc.globalpoint fields
        a caller's pp_update_async changes before that step.  Returns [(SceneIn record, flags, EgoTrackState record)]."""
        dm = self.dm
        cfg = _cfg(dm)
        si, pool = _scene(dm, cfg, v=v)
        g = si["loc"]["globalpoint"]
        g["x"], g["y"], g["dir"] = pose
        run = eb.Runner(self.name, tk, self.log)
        full = []
        for st in steps:
            if len(st) == 2:
                full.append((st[0], _state(dm, st[1])))
            else:
                full.append((st[0], _state(dm, st[1]), st[2], np.ones(1, bool)))
        res = self._run(run, cfg, model, si, full, pool)
        return [(r.out[0], int(r.flags[0]), r.track[0]) for r in res]

    def _run(self, run, cfg, model, si, full, pool):
        dm = self.dm
        model = dm.default_ego_model() if model is None else model
        if not any(len(s) == 4 for s in full):
            return run(cfg, model, si, full, dict(lane_pool=pool))
        # the update of step k is the record step k - 1 staged with some pose fields changed: found on the model, which the device must equal
        ref = eb.ModelBackend(run.tk)
        done = []
        for k, s in enumerate(full):
            if len(s) == 4:
                prev = ref.run(cfg, model, si, done, dict(lane_pool=pool))[-1].out.copy()
                for name, val in s[2].items():
                    prev["loc"]["globalpoint"][name] = val(float(prev["loc"]["globalpoint"][name][0])) if callable(val) else val
                s = (s[0], s[1], prev, s[3])
            done.append(s)
        return run(cfg, model, si, done, dict(lane_pool=pool))

    def __call__(self, tk, pose, po, k0=0, **kw):
        return self.steps(tk, pose, [(po, k0)], **kw)[0]


def _st(S):
    return (float(S["hx"]), float(S["hy"]), float(S["kappa"]), int(S["valid"]), int(S["n_init"]), int(S["n_sat"]), float(S["max_kappa"]))


def _pose(out):
    g = out["loc"]["globalpoint"]
    return float(g["x"]), float(g["y"]), float(g["dir"])


# ---------------------------------------------------------------------------------------------------------------
# known answers of one step
def _kat_straight(dm, adv):
    """On the path, heading along it: e = (8, 0), ly = 0 * 1 - 8 * 0 = 0, kc = 0; t = 0, c = 1, sn = 0: two substeps of 0.5 m along
    (1, 0) from (100, 0) end on (101, 0); dir = atan(0 / 1) = 0.  Standing still: the same state, the pose kept."""
    out, f, S = adv(_tk(dm), (100.0, 0.0, 0.0), _east(dm), v=36.0)
    assert (_pose(out), float(out["loc"]["velocity"]), f) == ((101.0, 0.0, 0.0), 36.0, 0)
    assert _st(S) == (1.0, 0.0, 0.0, 1, 1, 0, 0.0)
    assert (int(S["key_x"]), int(S["key_y"]), int(S["key_dir"])) == (etm.bits(101.0), 0, 0)
    out, f, S = adv(_tk(dm), (100.0, 0.0, 0.0), _east(dm, desspd=0.0))
    assert (_pose(out), f, _st(S)) == ((100.0, 0.0, 0.0), 0, (1.0, 0.0, 0.0, 1, 1, 0, 0.0))


def _kat_abeam_and_on_target(dm, adv):
    """Heading east at (50, -13), the target (50, 3) exactly abeam: e = (0, 16), ly = 16 * 1 - 0 * 0 = 16, d2 = 256, kc = 32 / 256 =
    0.125 (left), inside max_curv 0.2.  s = 0: the pose and the heading are kept, the curvature moves.  Mirrored at (50, 19):
    e = (0, -16), kc = -0.125.  On the target itself, (50, 3): d2 = 0, kc = 0."""
    out, f, S = adv(_fast(dm), (50.0, -13.0, 0.0), _north(dm))
    assert (_pose(out), f, _st(S)) == ((50.0, -13.0, 0.0), 0, (1.0, 0.0, 0.125, 1, 1, 0, 0.125))
    out, f, S = adv(_fast(dm), (50.0, 19.0, 0.0), _north(dm))
    assert (_pose(out), f, _st(S)) == ((50.0, 19.0, 0.0), 0, (1.0, 0.0, -0.125, 1, 1, 0, 0.125))
    out, f, S = adv(_fast(dm), (50.0, 3.0, 0.0), _north(dm))
    assert (_pose(out), f, _st(S)) == ((50.0, 3.0, 0.0), 0, (1.0, 0.0, 0.0, 1, 1, 0, 0.0))


def _kat_clamp(dm, adv):
    """kc = +-0.125 as above.  max_curv 0.125: the command is ON the bound - it counts as met (n_sat 1) and kappa is the bound.
    max_curv one ulp above 0.125: inside, n_sat 0.  max_curv 0.1: clamped to +-0.1, n_sat 1."""
    above = math.nextafter(0.125, 1.0)
    for y, sign in ((-13.0, 1.0), (19.0, -1.0)):
        S = adv(_fast(dm, max_curv=0.125), (50.0, y, 0.0), _north(dm))[2]
        assert _st(S) == (1.0, 0.0, sign * 0.125, 1, 1, 1, 0.125)
        S = adv(_fast(dm, max_curv=above), (50.0, y, 0.0), _north(dm))[2]
        assert _st(S) == (1.0, 0.0, sign * 0.125, 1, 1, 0, 0.125)
        S = adv(_fast(dm, max_curv=0.1), (50.0, y, 0.0), _north(dm))[2]
        assert _st(S) == (1.0, 0.0, sign * 0.1, 1, 1, 1, 0.1)


def _kat_rate_limit(dm, adv):
    """dt = 0.125 s (exact).  curv_rate 1: dk = 0.125, hi = 0 + 0.125 = kc: the step lands exactly on kc.  curv_rate 0.5: dk = 0.0625,
    kappa = 0.0625 after one advance and - the pose bits are the ones stored, so the state is kept - 0.125 after the second, exactly
    on kc, and stays there; n_init stays 1.  Towards kc = -0.125 alike."""
    model = dm.default_ego_model()
    model["dt"] = 0.125
    S = adv(_tk(dm, curv_rate=1.0), (50.0, -13.0, 0.0), _north(dm), model=model)[2]
    assert _st(S) == (1.0, 0.0, 0.125, 1, 1, 0, 0.125)
    res = adv.steps(_tk(dm, curv_rate=0.5), (50.0, -13.0, 0.0), [(_north(dm), 0)] * 3, model=model)
    assert [_st(S) for _, _, S in res] == [(1.0, 0.0, 0.0625, 1, 1, 0, 0.0625), (1.0, 0.0, 0.125, 1, 1, 0, 0.125), (1.0, 0.0, 0.125, 1, 1, 0, 0.125)]
    res = adv.steps(_tk(dm, curv_rate=0.5), (50.0, 19.0, 0.0), [(_north(dm), 0)] * 2, model=model)
    assert [_st(S) for _, _, S in res] == [(1.0, 0.0, -0.0625, 1, 1, 0, 0.0625), (1.0, 0.0, -0.125, 1, 1, 0, 0.125)]


def _kat_bias_turns_a_straight_ego(dm, adv):
    """On the path, heading along it, kc = 0 - but curv_bias 0.5 is applied behind the limits: with n_sub 1, s = 1: t = 0.25 * 0.5 * 1
    = 0.125, t2 = 0.015625, c = 0.984375 / 1.015625 = 63 / 65, sn = 0.25 / 1.015625 = 16 / 65: the ego moves 1 m along (63, 16) / 65
    and its heading turns by twice that angle; kappa itself stays 0."""
    out, f, S = adv(_tk(dm, curv_bias=0.5, n_sub=1), (100.0, 0.0, 0.0), _east(dm), v=36.0)
    c, sn = 0.984375 / 1.015625, 0.25 / 1.015625
    assert (float(out["loc"]["globalpoint"]["x"]), float(out["loc"]["globalpoint"]["y"])) == (100.0 + 1.0 * c, 0.0 + 1.0 * sn)
    nx, ny = c * c - sn * sn, sn * c + c * sn
    n = math.sqrt(nx * nx + ny * ny)
    assert (float(S["hx"]), float(S["hy"]), float(S["kappa"]), int(S["n_sat"])) == (nx / n, ny / n, 0.0, 0)
    assert abs(float(out["loc"]["globalpoint"]["dir"]) - math.degrees(4.0 * math.atan(0.125))) < 1e-9 and f == 0


def _kat_walk_chunks(dm, adv):
    """k0 on the 64-segment chunks of the walk, the ego 0.25 m left of a straight path at 36 km/h (s = 1 m, ld = 8 m = 16 segments):
    k0 = 0: four chunks, the target P[16]; 135: one chunk of exactly 64; 136: 63 segments; 190: 4.5 m of path left - the target is
    P[199], no PATH_END; 198: one segment of 0.5 m - both walks run out: PATH_END, the ego is NOT put on P[199]; 199: no segment."""
    for k0, flag in ((0, 0), (135, 0), (136, 0), (190, 0), (198, PATH_END), (199, PATH_END)):
        x0 = 100.0 + 0.5 * k0
        out, f, S = adv(_tk(dm), (x0, 0.25, 0.0), _east(dm), k0=k0, v=36.0)
        assert f == flag and int(S["valid"]) == 1 and float(S["kappa"]) < 0.0
        assert x0 + 0.99 < float(out["loc"]["globalpoint"]["x"]) < x0 + 1.0 and 0.235 <= float(out["loc"]["globalpoint"]["y"]) < 0.25          # (|kappa| <= 0.03 after one rate step: at most 0.03 * 1 * 1 / 2 = 0.015 m sideways)
    # a target 40 m ahead crosses a chunk edge with segments of non-zero length: look_min 40 -> segment 79 from k0 = 0
    out, f, S = adv(_tk(dm, look_min=40.0), (100.0, 0.25, 0.0), _east(dm, desspd=0.0))
    # standing: e = (40, -0.25), ly = -0.25, d2 = 1600.0625, kc = -0.5 / 1600.0625, limited to -0.03
    assert (f, float(S["kappa"])) == (0, -0.5 / 1600.0625)


def _kat_zero_length_segments(dm, adv):
    """70 copies of P[0] in front of the path (zero-length segments across the first chunk edge), and a run of five at the target:
    they are skipped, the target standing still is the vertex 3 m along, (103, 0)."""
    xs = np.concatenate([np.full(70, 100.0), 100.0 + 0.5 * np.arange(1, 131)])
    xs[76:81] = 103.0                                   # P[75] = 102.5, P[76 .. 80] = 103: the walk ends on segment 75, t = 1
    out, f, S = adv(_fast(dm), (103.0, -16.0, 0.0), _path(dm, xs, 0.0))
    assert (f, _st(S)) == (0, (1.0, 0.0, 0.125, 1, 1, 0, 0.125))      # e = (0, 16): abeam
    out, f, S = adv(_tk(dm), (100.0, 0.0, 0.0), _path(dm, xs, 0.0, desspd=36.0), v=36.0)
    assert (_pose(out), f) == ((101.0, 0.0, 0.0), 0)


def _kat_bad_paths(dm, adv):
    """BAD_PATH leaves the record AND the state untouched (a state that was never stored stays zero; one that was keeps every byte).
    A NaN point 4 m ahead: beyond s = 1 m but inside ld = 8 m.  An infinite one alike.  k0 = 199 on a non-finite P[199] (the only
    way to a non-finite target that is not a non-finite length first).  A NaN inside s."""
    for k_bad, val, k0 in ((8, np.nan, 0), (8, np.inf, 0), (199, np.nan, 199), (1, np.nan, 0)):
        po = _east(dm)
        po["road_points"]["x"][0, k_bad] = val
        res = adv.steps(_tk(dm), (100.0, 0.25, 10.0), [(_east(dm), 0), (po, k0), (_east(dm), 0)], v=36.0)
        (a, fa, Sa), (b, fb, Sb), (c, fc, Sc) = res
        assert (fa, fb, fc) == (0, BAD_PATH, BAD_PATH)
        assert b.tobytes() == a.tobytes() and Sb.tobytes() == Sa.tobytes() and c.tobytes() == a.tobytes() and Sc.tobytes() == Sa.tobytes()
    po = _east(dm)
    po["road_points"]["y"][0, 8] = np.nan
    out, f, S = adv(_tk(dm), (100.0, 0.25, 10.0), po, v=36.0)
    assert f == BAD_PATH and not S.tobytes().strip(b"\0") and _pose(out) == (100.0, 0.25, 10.0)


def _kat_frozen_keeps_the_state(dm, adv):
    """PATH_END on the first advance (k0 = 198), frozen from the second: the record and the state are carried over to the byte."""
    (a, fa, Sa), (b, fb, Sb) = adv.steps(_tk(dm), (199.0, 0.25, 0.0), [(_east(dm), 198), (_east(dm), 0)], v=36.0)
    assert (fa, fb) == (PATH_END, PATH_END) and int(Sa["valid"]) == 1
    assert b.tobytes() == a.tobytes() and Sb.tobytes() == Sa.tobytes()


def _kat_stale_by_each_pose_field(dm, adv):
    """Two advances 2 m beside the path (kc = 2 * -2 / (64 + 4) = -0.059 at first: the curvature state goes 0 -> -0.03 -> -0.051), then
    the caller updates the records: with the bits the model stored the state is kept (n_init 1, kappa follows kc from where it was:
    beyond -0.03, which a state re-derived in that advance - one rate step from 0 - cannot reach); with x, y or dir alone changed - x and y by one ulp - it is re-derived: n_init 2, kappa starts again from 0 (one rate step: -0.03), the
    heading is that of the record's dir."""
    two = [(_east(dm), 0), (_east(dm), 2)]
    kept = adv.steps(_tk(dm), (100.0, 2.0, 0.0), two + [(_east(dm), 4, {})], v=36.0)
    assert [int(S["n_init"]) for _, _, S in kept] == [1, 1, 1] and float(kept[0][2]["kappa"]) == -0.3 * 0.1
    assert -0.06 < float(kept[1][2]["kappa"]) < -0.03 and -0.06 < float(kept[2][2]["kappa"]) < -0.03
    for field, change in (("x", lambda v: math.nextafter(v, 1e9)), ("y", lambda v: math.nextafter(v, 1e9)), ("dir", 3.0)):
        res = adv.steps(_tk(dm), (100.0, 2.0, 0.0), two + [(_east(dm), 4, {field: change})], v=36.0)
        S = res[2][2]
        assert (int(S["n_init"]), int(S["valid"])) == (2, 1) and float(S["kappa"]) == -0.3 * 0.1, field
        assert float(S["max_kappa"]) == float(res[1][2]["max_kappa"]) > 0.03          # the totals go on
    # the heading of dir = 3 degrees, turned by the one step of 1 m at kappa = -0.03: 2 substeps * 4 * atan(0.25 * -0.03 * 0.5)
    assert abs(math.atan2(float(S["hy"]), float(S["hx"])) - (math.radians(3.0) + 8.0 * math.atan(0.25 * -0.03 * 0.5))) < 1e-12


KATS = [_kat_straight, _kat_abeam_and_on_target, _kat_clamp, _kat_rate_limit, _kat_bias_turns_a_straight_ego, _kat_walk_chunks,
        _kat_zero_length_segments, _kat_bad_paths, _kat_frozen_keeps_the_state, _kat_stale_by_each_pose_field]


# ---------------------------------------------------------------------------------------------------------------
# CPU
def test_abi_mirror_and_default_tracker(dm):
    lib = dm.load_library()
    assert lib.pp_sizeof(40) == dm.EgoTracker.itemsize == 48 and lib.pp_sizeof(41) == dm.EgoTrackState.itemsize == 72
    assert lib.pp_sizeof(42) == 0
    tk = dm.default_ego_tracker()
    assert [float(tk[k][0]) for k in ("look_min", "look_gain", "max_curv", "curv_rate", "curv_bias")] == [3.0, 0.5, 0.2, 0.3, 0.0]
    assert (int(tk["n_sub"][0]), int(tk["_pad"][0])) == (2, 0)
    assert (lib.pp_feature_retires(13), lib.pp_feature_retires(14)) == (0, -1)          # no feature bit, no cause: the table is as it was


def test_heading_polynomial():
    """Within 1e-12 of numpy's cos / sin (degrees through the same product by pi / 180 for the big angles: the reduction is exact, a
    product of 1e6 by pi / 180 is not); unit length to an ulp; (1, 0) for a non-finite angle; the coefficients are 1 / n!."""
    assert [abs(c) for c in etm.SIN_C] == [1.0 / math.factorial(n) for n in range(1, 18, 2)]
    assert [abs(c) for c in etm.COS_C] == [1.0 / math.factorial(n) for n in range(0, 17, 2)]
    sweep = [0.0, 45.0, 90.0, 135.0, 180.0, 270.0, math.nextafter(360.0, 0.0), -0.0, -45.0, -44.999, -90.0, -179.5, -360.0, -1e6, 360.0, 405.0,
             725.25, 1e6, 44.999999999, 45.000000001, 1e-300, 12345.678] + list(np.linspace(-720.0, 720.0, 577))
    worst = 0.0
    for d in sweep:
        hx, hy = etm.heading(d)
        r = math.fmod(d, 360.0)                          # exact
        worst = max(worst, abs(hx - float(np.cos(np.deg2rad(r)))), abs(hy - float(np.sin(np.deg2rad(r)))))
        assert abs(hx * hx + hy * hy - 1.0) < 5e-16
    assert worst <= 1e-12, worst
    assert etm.heading(0.0) == (1.0, 0.0) and etm.heading(90.0) == (0.0, 1.0) and etm.heading(180.0) == (-1.0, 0.0) and etm.heading(270.0) == (0.0, -1.0)
    assert etm.heading(1e6) == etm.heading(1e6 - 360.0 * 2777)          # 1e6 = 2777 * 360 + 280
    for d in (np.nan, np.inf, -np.inf):
        assert etm.heading(d) == (1.0, 0.0)


def test_model_functions_known_answers():
    """The pieces of §4q 3. - 4. on their own: the command either side of d2 = 0 and of the bound, a NaN, the rate limit, no motion at
    s = 0, and a circle of radius 20 m driven in steps of 2 m: the radius error after a quarter turn shrinks from n_sub 1 to 8."""
    assert etm.command(0.0, 0.0, 1.0, 0.0, 0.0, 16.0, 0.2) == (0.125, 0)
    assert etm.command(0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.2) == (0.0, 0)
    assert etm.command(0.0, 0.0, 1.0, 0.0, 0.0, 16.0, 0.125) == (0.125, 1) and etm.command(0.0, 0.0, 1.0, 0.0, 0.0, -16.0, 0.125) == (-0.125, 1)
    assert etm.command(0.0, 0.0, 1.0, 0.0, 0.0, 16.0, math.nextafter(0.125, 1.0)) == (0.125, 0)
    assert etm.command(np.nan, 0.0, 1.0, 0.0, 0.0, 16.0, 0.2) == (0.0, 0) and etm.command(0.0, 0.0, 1.0, 0.0, np.inf, np.inf, 0.2) == (0.0, 0)
    assert etm.rate_limit(0.0, 0.125, 1.0, 0.125) == 0.125 and etm.rate_limit(0.0, 0.125, 0.5, 0.125) == 0.0625 and etm.rate_limit(0.0625, -1.0, 0.5, 0.125) == 0.0
    assert etm.move(1.0, 2.0, 0.6, 0.8, 0.1, 0.0, 4) == (1.0, 2.0, 0.6, 0.8) and etm.move(1.0, 2.0, 0.6, 0.8, 0.1, -1.0, 4) == (1.0, 2.0, 0.6, 0.8)
    err = {}
    for n_sub in (1, 8):
        x, y, hx, hy = 20.0, 0.0, 0.0, 1.0
        for _ in range(16):                              # 32 m: about a quarter of the circle
            x, y, hx, hy = etm.move(x, y, hx, hy, 0.05, 2.0, n_sub)
        err[n_sub] = abs(math.sqrt(x * x + y * y) - 20.0)
        assert abs(hx * hx + hy * hy - 1.0) < 5e-16
    print("radius error after 32 m at R = 20 m:", err)
    # a substep moves ds along the chord direction, and the chord of an arc ds = R * th is ds * (1 - th^2 / 24) long: the ego drifts outwards
    # by about ds * th^2 / 24 per substep - 16 * 2 * 0.1^2 / 24 = 0.0133 m at n_sub 1, and 1 / 64 of that at n_sub 8 (second order)
    assert err[8] < err[1] / 32.0 and err[1] < 1.1 * 16 * 2.0 * 0.1 ** 2 / 24.0


def test_walk_is_the_walk_of_the_ego_model(dm):
    """etm.walk against ego_model.walk_path on the same paths: point and flags (the factored walk returns no heading)."""
    cfg, rng = _cfg(dm), np.random.default_rng(5)
    for trial in range(200):
        px, py = np.cumsum(rng.uniform(0.0, 1.0, 200)), np.cumsum(rng.uniform(-0.3, 0.3, 200))
        if trial % 3 == 0:
            px[60:70], py[60:70] = px[60], py[60]
        if trial % 7 == 0:
            px[int(rng.integers(1, 200))] = np.nan
        k0, d = int(rng.integers(0, 200)), float(rng.uniform(-1.0, 120.0))
        if not (math.isfinite(px[k0]) and math.isfinite(py[k0])):
            continue
        x, y, _, f = em.walk_path(cfg, px, py, k0, d, 5.0)
        wx, wy, seg, bad, ran_out = etm.walk(px, py, k0, d)
        assert (bad, ran_out) == (bool(f & BAD_PATH), bool(f & PATH_END))
        assert bad or (x, y) == (wx, wy)


@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_model(dm, kat):
    kat(dm, _Adv(dm, "model"))


def test_model_with_tracker_off_is_the_wrapped_model(dm):
    cfg, model = _cfg(dm), dm.default_ego_model()
    si, pool = _scene(dm, cfg)
    st, flags, track = _state(dm, 3), np.zeros(1, np.int32), np.zeros(1, dm.EgoTrackState)
    want = em.advance(cfg, model, si, _east(dm), st, flags, pool, False)
    got = etm.advance(dm, cfg, model, None, track, si, _east(dm), st, flags, lane_pool=pool)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[3] is track


# ---- the ring: 16 routed egos, oracle tick + models.  The figures in the assertions are those of this loop (profiles/r33_ego_tracker.txt)
E2E_N = 16
BIAS = 0.02          # 1/m: a car that pulls to the left on a 50 m radius with the wheel straight
_CPU = {}


def _e2e_scene(dm):
    cfg = _cfg(dm)
    m = rs.build_ring(dm)
    sc, legs, rf = rs.make_egos(dm, cfg, m, E2E_N, seed=3, lanes=(1, 2), ids=(150, 200), legs=(2, 4))
    return cfg, m, sc, legs, rf


def _cpu_loop(dm, oracle, which, ticks):
    if (which, ticks) in _CPU:
        return _CPU[which, ticks]
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    tk = {"off": None, "default": _tk(dm), "bias": _tk(dm, curv_bias=BIAS)}[which]
    model, rm = dm.default_ego_model(), dm.default_route_model()
    si, st, flags = ms.resolve(dm, m, sc["scene_in"]), sc["state"].copy(), np.zeros(E2E_N, np.int32)
    track, cause, lat = np.zeros(E2E_N, dm.EgoTrackState), np.zeros((6, E2E_N), np.int64), np.zeros(E2E_N)
    for t in range(ticks):
        plan, _, _ = oracle.plan_tick_batch(cfg, dict(sc, scene_in=si, mot_pool=None), st, n_threads=8, want_grid=False)
        for c in range(6):
            cause[c] += (st["afresh_planning"] != 0) & (st["afresh_cause"] == c)
        lat = np.maximum(lat, np.abs(st["path_lat_dis"]))
        si, flags, _, track = etm.advance(dm, cfg, model, tk, track, si, plan, st, flags, route=(rm, legs, rf, m))
    _CPU[which, ticks] = dict(si=si, flags=flags, cause=cause, track=track, lat=lat)
    return _CPU[which, ticks]


def test_ring_default_tracker_crosses_a_junction_without_tracking_replans(dm, oracle):
    """300 ticks, the default tracker against no tracker: every ego crosses its first junction onto the next road with the flags the
    on-path model gives (none), never replans on cause 3 (heading error) - nor on cause 2: the largest |path_lat_dis| any tick saw is
    0.016 m against the 0.2 m of cause 2 - and never meets max_curv (the largest |kappa| is 0.019 1/m)."""
    on, off = _cpu_loop(dm, oracle, "default", 300), _cpu_loop(dm, oracle, "off", 300)
    print("default: cause counts", on["cause"].sum(axis=1).tolist(), "max |lat|", float(on["lat"].max()), "max |kappa|", float(on["track"]["max_kappa"].max()),
          "| off: cause counts", off["cause"].sum(axis=1).tolist())
    for r in (on, off):
        assert (r["si"]["loc"]["path_num"] >= 1).all() and (r["si"]["loc"]["pos"] == 0).all()
    assert np.array_equal(on["flags"], off["flags"]) and not on["flags"].any()
    assert not on["cause"][3].any() and not on["cause"][2].any() and not off["cause"][2].any() and not off["cause"][3].any()
    assert 0.0 < on["lat"].max() < 0.05
    assert (on["track"]["n_init"] == 1).all() and (on["track"]["n_sat"] == 0).all() and 0.0 < on["track"]["max_kappa"].max() < 0.05


def test_ring_steering_bias_makes_the_planner_replan_on_lateral_error(dm, oracle):
    """What the feature is for.  curv_bias 0.02 1/m, 200 ticks: every ego replans on cause 2 (|path_lat_dis| > 0.2 m) on at least three
    ticks - 33 .. 59 per ego, 836 in all, in the run recorded in the profile file - where the default tracker (bias 0) and a handle
    without a tracker do so on none; no ego is flagged and none replans on cause 3."""
    bias, zero, off = (_cpu_loop(dm, oracle, w, 200) for w in ("bias", "default", "off"))
    print("cause 2 per ego with bias", BIAS, ":", bias["cause"][2].tolist(), "total", int(bias["cause"][2].sum()), "max |lat|", float(bias["lat"].max()))
    assert (bias["cause"][2] >= 3).all()
    assert not zero["cause"][2].any() and not off["cause"][2].any()
    assert not bias["cause"][3].any() and not bias["flags"].any()
    assert bias["lat"].max() > 0.2


# ---------------------------------------------------------------------------------------------------------------
# GPU
@gpu
@pytest.mark.parametrize("kat", KATS, ids=lambda f: f.__name__[5:])
def test_kat_on_the_device(dm, kat):
    """The known answers on k_advance_egos<true> (injected PlanOut / SceneState), each step also held against the model to the bit."""
    kat(dm, _Adv(dm, "device"))


@gpu
def test_kat_batches_of_5_and_7_equal_each_case_alone(dm):
    """Every known answer once more on the device, logged, then as distinct scenes of launches of 5 and 7 scenes per group of calls
    that can share one (same ego model, tracker, number of steps) - a frozen scene and a BAD_PATH scene among them.  Every scene gives
    the bytes it gave alone: SceneIn, flags, trace, EgoTrackState."""
    log = []
    a = _Adv(dm, "device", log)
    for kat in KATS:
        kat(dm, a)
    assert any(int(r.flags[0]) == BAD_PATH for c in log for r in c["res"]) and any(int(c["res"][0].flags[0]) == PATH_END and len(c["res"]) > 1 for c in log)
    sizes = eb.batched(log)
    print(f"{len(log)} calls in batches of {sizes}")
    assert sum(sizes) >= len(log) and set(sizes) <= {5, 7} and 5 in sizes


@gpu
def test_set_scenes_clears_the_states(dm):
    """valid = 0 after pp_set_scenes: two advances leave a state (n_init 1, n_sat counted), pp_set_scenes with the same records zeroes
    every byte of it, and the next advance re-derives it (n_init 1 again, kappa from 0) - the model survived the call."""
    cfg, model, tk = _cfg(dm), dm.default_ego_model(), _tk(dm, max_curv=0.005)          # kc = 2 * -0.25 / (64 + 0.0625) = -0.0078: beyond the bound on every advance
    si, pool = _scene(dm, cfg)
    g = si["loc"]["globalpoint"]
    g["x"], g["y"], g["dir"] = 100.0, 0.25, 0.0
    sc = dict(scene_in=si, obs_pool=np.zeros(1, dm.ObPoint), mot_pool=np.zeros(1, dm.ObMotion), n_obs=0, lane_pool=pool,
              attr_pool=np.zeros(len(pool), np.uint8), ref_pool=np.zeros(1, dm.GlobalPoint2D))
    pl = dm.Planner(cfg, device=0, max_scenes=1, max_obs_total=1, max_lane_pts_total=len(pool), max_ref_pts_total=1)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        pl.ego_track_state()                                   # never set
    pl.set_ego_tracker(tk)
    pl.set_scenes(sc, with_motion=False)

    def two():
        got = []
        for k0 in (0, 2):
            pl.tick()
            pl.write_device(dm.BUF_PLAN_OUT, _east(dm))
            pl.write_device(dm.BUF_STATE, _state(dm, k0))
            pl.advance_async(model)
            got.append(pl.ego_track_state()[0].copy())
        return got

    a = two()
    assert [(int(S["valid"]), int(S["n_init"]), int(S["n_sat"])) for S in a] == [(1, 1, 1), (1, 1, 2)]
    pl.tick()
    pl.set_scenes(sc, with_motion=False)
    assert not pl.ego_track_state().tobytes().strip(b"\0")
    b = two()
    pl.close()
    assert [S.tobytes() for S in a] == [S.tobytes() for S in b]


RING_TICKS = 30


def _ring_planner(dm, tk):
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    pl = _planner(dm, cfg, m, sc)
    pl.set_route(legs, rf)
    if tk is not None:
        pl.set_ego_tracker(tk)
    return pl, (cfg, m, sc, legs, rf)


@gpu
def test_ring_route_kernel_against_the_model_step_by_step(dm):
    """k_advance_route<true> on the ring, 30 ticks of the device's own plans (nothing injected), a biased tracker so that the planner
    replans on the way: every advance is held against the model applied to the device's own records of the step before -
    SceneIn, flags, EgoTrackState to the bit, dir within DIR_TOL."""
    tk = _tk(dm, curv_bias=0.04)
    pl, (cfg, m, sc, legs, rf) = _ring_planner(dm, tk)
    model, n = dm.default_ego_model(), E2E_N
    sin, flags, track = pl.get_scene_in(), np.zeros(n, np.int32), np.zeros(n, dm.EgoTrackState)
    trace = dm.pinned_empty(n, dm.EgoTrace)
    for t in range(RING_TICKS):
        pl.tick()
        plan, state = pl.get_plan(), pl.get_state()
        pl.advance_async(model, trace)
        got = eb.Result(pl.get_scene_in(), pl.ego_flags(), None, pl.ego_track_state())
        pl.sync()
        got.trace = np.array(trace)
        eb.ab.check_trace(got, f"tick {t}")
        want = eb.model_step(cfg, model, tk, track, sin, plan, state, flags, dict(map=m), (legs, rf, None))
        eb.compare(got, want, f"tick {t}")
        sin, flags, track = got.out, got.flags, got.track
    pl.close()
    print("max |kappa|", float(track["max_kappa"].max()), "flags", flags.tolist())
    assert (track["valid"] == 1).all() and (track["n_init"] == 1).all() and track["max_kappa"].min() > 0.0 and not flags.any()


@gpu
def test_episodes_restart_the_state_and_replay(dm):
    """pp_set_episodes with max_ticks 6 on the ring, a biased tracker: the advance AFTER a restart finds EpisodeStats.age = 0 and
    re-derives the state - n_init goes up by one per episode and kappa is one rate step from 0 - and the second episode repeats the
    first in x, y and kappa byte for byte (the restart puts the ego on the very records it started from)."""
    tk = _tk(dm, curv_bias=0.04)
    pl, (cfg, m, sc, legs, rf) = _ring_planner(dm, tk)
    em_ = dm.default_episode_model()
    em_["max_ticks"] = 6
    pl.set_episodes(em_)
    model, rows = dm.default_ego_model(), []
    for t in range(13):
        pl.tick()
        pl.advance_async(model)
        g, S, st = pl.get_scene_in()["loc"]["globalpoint"], pl.ego_track_state(), pl.episode_stats()
        rows.append((g["x"].tobytes(), g["y"].tobytes(), S["kappa"].tobytes(), S["n_init"].copy(), st["age"].copy(), st["n_episodes"].copy()))
    pl.close()
    age = [int(r[4][0]) for r in rows]
    assert age == [1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 0, 1] and [int(r[5][0]) for r in rows] == [0] * 5 + [1] * 6 + [2] * 2
    # advance 0 derives the state (the capture left age 0), advance 5 is the one whose respawn restarts the scene, advance 6 the first of episode 2
    assert [int(r[3][0]) for r in rows] == [1] * 6 + [2] * 6 + [3] and all((r[3] == r[3][0]).all() for r in rows)
    for k in range(5):
        assert rows[k][:3] == rows[6 + k][:3], f"advance {k} of the episode"
    assert rows[6][2] != rows[5][2]


@gpu
def test_tracker_off_is_the_engine_without_it(dm):
    """20 rollout ticks on a handle that never set a tracker, one that set it and cleared it with NULL, and one that set it, called
    pp_set_egos (which the model survives) and then cleared it: SceneIn, flags, trace and PlanOut bytes are identical; a fourth that
    leaves it on differs."""
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    outs = []
    for mode in ("never", "off", "egos_off", "on"):
        pl = _planner(dm, cfg, m, sc)
        if mode != "never":
            pl.set_ego_tracker(_tk(dm, curv_bias=0.04))
        if mode == "egos_off":
            pl.set_egos(sc, with_motion=False)
            pl.set_state(sc["state"])
        if mode in ("off", "egos_off"):
            pl.set_ego_tracker(None)
        pl.set_route(legs, rf)
        _, trace = pl.rollout(20, trace=True)
        pl.sync()
        outs.append((pl.get_scene_in(), pl.ego_flags(), np.array(trace), pl.get_plan()))
        if mode == "off":
            assert not pl.ego_track_state().tobytes().strip(b"\0")          # readable, and no advance touched it
        pl.close()
    for other in outs[1:3]:
        for a, b, name in zip(outs[0], other, ("SceneIn", "flags", "trace", "PlanOut")):
            assert a.tobytes() == b.tobytes(), name
    assert outs[3][0]["loc"]["globalpoint"].tobytes() != outs[0][0]["loc"]["globalpoint"].tobytes()


@gpu
def test_bad_arguments_leave_the_tracker_as_it_was(dm):
    """Every PP_ERR_ARG case on a handle with a tracker in force: afterwards it runs exactly like a handle that only ever set that
    tracker.  PP_ERR_STATE from the read-back of a handle that never set one."""
    cfg, m, sc, legs, rf = _e2e_scene(dm)
    good = _tk(dm, curv_bias=0.03, n_sub=3)
    ref, _ = _ring_planner(dm, good)
    pl, _ = _ring_planner(dm, good)
    bad = [dict(look_min=0.0), dict(look_min=-1.0), dict(look_gain=-0.5), dict(max_curv=0.0), dict(max_curv=-0.2), dict(curv_rate=0.0),
           dict(curv_rate=-1.0), dict(n_sub=0), dict(n_sub=9), dict(n_sub=-1)]
    bad += [{k: v} for k in ("look_min", "look_gain", "max_curv", "curv_rate", "curv_bias") for v in (np.nan, np.inf, -np.inf)]
    for kw in bad:
        with pytest.raises(dm.PlannerError, match="error -1:"):
            pl.set_ego_tracker(_tk(dm, **kw))
    pl.set_ego_tracker(_tk(dm, look_gain=0.0, n_sub=8))          # the edges that are legal
    pl.set_ego_tracker(_tk(dm, n_sub=1))
    pl.set_ego_tracker(good)
    with pytest.raises(dm.PlannerError, match="error -1:"):
        pl.set_ego_tracker(_tk(dm, n_sub=0))
    outs = []
    for p in (pl, ref):
        p.rollout(10)
        p.sync()
        outs.append((p.get_scene_in(), p.ego_flags(), p.ego_track_state()))
        p.close()
    for a, b, name in zip(outs[0], outs[1], ("SceneIn", "flags", "EgoTrackState")):
        assert a.tobytes() == b.tobytes(), name
    assert (outs[0][2]["valid"] == 1).all()
    never = _planner(dm, cfg, m, sc)
    with pytest.raises(dm.PlannerError, match="error -4:"):
        never.ego_track_state()
    never.close()
