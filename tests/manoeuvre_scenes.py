"""Cases and backends for the traffic-manoeuvre tests (tests/test_traffic_manoeuvres.py).

A case = some tracks, some SCENES - each an ego (x, y, velocity in km/h, flagged or not) and the actors of that scene as rows
(s0, speed, track, type, radius) -, the manoeuvre records (traffic_manoeuvre_model.record, `actor` = the flat index over the
scenes, row by row), a TrafficFollow model or None (following off), and what the case expects of the model's branch record.  The
ego is staged at the same pose, with the same velocity, by every advance (tests/traffic_follow_backends.py has the staging).

run_model runs tests/traffic_manoeuvre_model.py; run_device runs the handle - pp_set_traffic, pp_set_traffic_follow,
pp_set_traffic_manoeuvres, then per step pp_plan_tick and pp_advance_async - and holds the states, s, v and the pinned pool entries
against the model after every advance, byte for byte, the model fed with the SceneIn records and flag words the device ITSELF staged.
join lays cases one behind the other as the scenes of ONE launch."""
import types

import numpy as np

import traffic_follow_backends as fb
import traffic_follow_model as fm
import traffic_manoeuvre_model as mm
import traffic_scenes as ts

DT, STEPS = 0.5, 6
FAR = (4096.0, 4096.0, 0.0, False)          # an ego nowhere near any track


def line(dm, n, x0=0.0, y=0.0, step=1.0):
    """n vertices every `step` metres along +x from (x0, y): every cumulative length and every foot is exact."""
    return ts.polyline(dm, [(x0 + step * i, y) for i in range(n)])


def case(name, polylines, scenes, recs, tf=None, expect=None):
    return types.SimpleNamespace(name=name, polylines=polylines, scenes=scenes, recs=mm.records(*recs), tf=tf, expect=expect or {})


def n_actors(c):
    return sum(len(sc["actors"]) for sc in c.scenes)


def join(cases):
    """The cases as scenes of one launch: tracks, scenes and actors one behind the other, the records' actors and tracks moved.
    Returns (the joined case, per case (first actor, first track))."""
    polylines, scenes, recs, base = [], [], [], []
    a0 = 0
    for c in cases:
        t0 = len(polylines)
        base.append((a0, t0))
        polylines += c.polylines
        scenes += [dict(ego=sc["ego"], actors=[(r[0], r[1], r[2] + t0, r[3], r[4]) for r in sc["actors"]]) for sc in c.scenes]
        r = c.recs.copy()
        r["actor"] += a0
        r["track"] = np.where(r["track"] >= 0, r["track"] + t0, r["track"])
        recs.append(r)
        a0 += n_actors(c)
    assert len({None if c.tf is None else tuple(sorted(fm.params(c.tf).items())) for c in cases}) == 1, "one launch has one model"
    return case("+".join(c.name for c in cases), polylines, scenes, recs, cases[0].tf), base


class Result:
    def __init__(self):
        self.s, self.v, self.st, self.ob, self.info = [], [], [], [], [None]          # lists over stages (0: after the set calls)


def _model_of(dm, c, act, stride, n_sc):
    tracks, pts = ts.pack(dm, c.polylines)
    return mm.Manoeuvres(tracks, pts, act, np.arange(n_sc) * stride, c.recs)


def run_model(dm, c, si_of_step=None, flags_of_step=None, steps=STEPS, dt=DT):
    act, stride, _, _ = fb._layout(dm, c.scenes, None)
    si, flags = fb._egos(dm, c.scenes)
    tr = _model_of(dm, c, act, stride, len(c.scenes))
    if c.tf is not None:
        tr.set_follow()
    pool = ts.filled(dm.ObPoint, len(c.scenes) * stride)
    pool, _ = tr.place(pool, None, 0.0)                          # pp_set_traffic
    res = Result()
    width = float(dm.default_config(128)["Vehicle_Width"][0])
    for k in range(steps + 1):
        if k:
            pool, _ = tr.advance(pool, None, dt, c.tf, si if si_of_step is None else si_of_step(k), flags if flags_of_step is None else flags_of_step(k), width)
            res.info.append(tr.minfo)
        res.s.append(tr.s.copy()), res.v.append(tr.v.copy()), res.st.append(tr.st.copy()), res.ob.append(pool[tr.pool_index].copy())
    return res


def open_device(dm, c, with_motion=False, manoeuvres=True, before=None, peers=0):
    """The handle of a case with everything set; returns (planner, actor records, stride, EgoModel, staging PlanOut).  before(pl) runs
    in front of pp_set_traffic; peers: every scene's slice is followed by that many free pool entries (the peer slots of a fleet)."""
    act, stride, _, _ = fb._layout(dm, c.scenes, None)
    tracks, pts = ts.pack(dm, c.polylines)
    n = len(c.scenes)
    want_si, _ = fb._egos(dm, c.scenes)
    cfg = dm.default_config(128)
    cfg["grid_stage"] = 0
    width = stride + peers
    sc = dm.gen_scenes(cfg, 0, n, width, junction_every=0)
    sc["obs_pool"] = ts.filled(dm.ObPoint, n * width)
    sc["mot_pool"] = ts.filled(dm.ObMotion, n * width)
    sc["scene_in"]["obs_off"], sc["scene_in"]["obs_n"] = np.arange(n) * width, stride
    for f in ("x", "y"):
        sc["scene_in"]["loc"]["globalpoint"][f] = want_si["loc"]["globalpoint"][f]
    sc["scene_in"]["loc"]["velocity"] = want_si["loc"]["velocity"]
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=n * width)
    pl.set_scenes(sc, with_motion=with_motion)
    pl.set_state(sc["state"])
    pl.scenes = sc                                               # (for a test that makes the scenes resident again)
    if before is not None:
        before(pl)
    pl.set_traffic(tracks, pts, act)
    if c.tf is not None:
        pl.set_traffic_follow(fb.fm_record(dm, c.tf))
    if manoeuvres:
        pl.set_traffic_manoeuvres(c.recs.astype(dm.TrafficManoeuvre))
    model = dm.default_ego_model()
    model["dt"], model["window"] = DT, 1
    return pl, act, stride, model, fb.staging_plan(dm, [s["ego"] for s in c.scenes], DT)


def read_actors(dm, pl, act, stride, n):
    got = np.zeros(len(act), dm.ObPoint)
    slices = [pl.get_obstacles(s, cap=stride) for s in range(n)]
    for a in range(len(act)):
        got[a] = slices[int(act["scene"][a])][int(act["slot"][a])]
    return got


def run_device(dm, c, steps=STEPS):
    pl, act, stride, model, po = open_device(dm, c)
    n = len(c.scenes)
    want_si, want_flags = fb._egos(dm, c.scenes)
    res, seen_si, seen_flags = Result(), {}, {}
    for k in range(steps + 1):
        if k:
            seen_si[k], seen_flags[k] = fb.staged_step(dm, pl, model, po)
        res.s.append(pl.traffic_state()), res.st.append(pl.get_traffic_manoeuvre_state().astype(mm.STATE))
        res.v.append(pl.traffic_speed() if c.tf is not None else act["speed"].astype(np.float64))
        res.ob.append(read_actors(dm, pl, act, stride, n))
    pl.close()
    fb.check_staged_egos(seen_si, seen_flags, want_si, want_flags, steps)
    want = run_model(dm, c, lambda k: seen_si[k], lambda k: seen_flags[k], steps)
    for k in range(steps + 1):
        what = f"{c.name}, stage {k}"
        assert res.st[k].tobytes() == want.st[k].tobytes(), f"{what}: states differ from the model's at actors {np.flatnonzero(res.st[k] != want.st[k]).tolist()[:20]}"
        assert res.s[k].tobytes() == want.s[k].tobytes(), f"{what}: arc lengths differ from the model's at actors {np.flatnonzero(res.s[k] != want.s[k]).tolist()[:20]}"
        if c.tf is not None:
            assert res.v[k].tobytes() == want.v[k].tobytes(), f"{what}: speeds differ from the model's at actors {np.flatnonzero(res.v[k] != want.v[k]).tolist()[:20]}"
        assert res.ob[k].tobytes() == want.ob[k].tobytes(), f"{what}: pool entries differ from the model's at actors {np.flatnonzero(res.ob[k] != want.ob[k]).tolist()[:20]}"
    res.info = want.info
    return res


def same_alone(batch, base, cases, alone):
    """Every actor of a launch of all cases gives the bytes it gave alone (the states' track numbers moved back)."""
    for c, (a0, t0), r in zip(cases, base, alone):
        sl = slice(a0, a0 + n_actors(c))
        for k in range(len(r.s)):
            st = batch.st[k][sl].copy()
            st["track"] -= t0
            what = f"{c.name} in the launch of all cases, stage {k}"
            assert st.tobytes() == r.st[k].tobytes(), f"{what}: states"
            assert batch.s[k][sl].tobytes() == r.s[k].tobytes(), f"{what}: s"
            assert batch.v[k][sl].tobytes() == r.v[k].tobytes(), f"{what}: v"
            assert batch.ob[k][sl].tobytes() == r.ob[k].tobytes(), f"{what}: ObPoint"
