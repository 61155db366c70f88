"""What the backends of the advance family share (advance_backends.py and the modules built on it: grid follow, ego tracker,
episodes, spawn, episode traffic, episode log, schedule): the handle with crafted records resident, the injection of one advance,
the assembly of single-scene calls into one launch, and the loop that holds a device run against the model.  Each piece stands
here once; a family module keeps its Case / Result fields, its model_step, its compare and the feature's own set calls and reads.

Why injection.  The device cannot be handed PlanOut, SceneState or flag words, so they are injected: the handle ticks once (a tick
is what an advance follows), the host waits, the crafted records are copied over the tick's PlanOut and SceneState buffers
(Planner.write_device) and pp_advance_async runs on them.  A flag word that is set on the way in is reached the honest way: an
earlier step of the same call sets it, the handle ticks, and the next step is injected (the model chains its own steps alike).
The tick's own results are overwritten before anything reads them; the scenes keep every slice inside its pool, so the slice check
behind the advance changes nothing and the model needs no rule for it."""
import types

import numpy as np

import dmpp_amd as dm

VIEW_OFFSETS = ("cur_off", "left_off", "right_off")


def route_of(route, n):
    """(legs, route_first, route model) of an optional (legs, route_first, model or None): no route is n empty ones."""
    if route is None:
        return None, np.zeros(n + 1, np.int32), dm.default_route_model()
    legs, rf, rm = route
    return legs, np.ascontiguousarray(rf, np.int32), dm.default_route_model() if rm is None else rm


def same_route_model(a, b):
    return (a is None) == (b is None) and (a is None or route_of(a, 1)[2].tobytes() == route_of(b, 1)[2].tobytes())


def open_planner(cfg, si, world, obs=None, mot_pool=None, with_motion=False, route=None, state=None, first=None, then=None, check=True):
    """A handle with the crafted records resident.  world: dict(map=...) - pp_set_map + pp_set_egos, and pp_set_route with a
    route - or dict(lane_pool=..., ref_pool=...) - pp_set_scenes.  obs: (obstacle pool, slot width); None is the one-entry dummy
    pool with n_obs = 0.  state: None is what pp_init_state gives.  `first(pl)` makes the set calls that come before the records
    (the models of the ego tracker and of grid follow, which must survive them), `then(pl)` the feature's own behind pp_set_state;
    last, unless check is off, the resident records are held against `si`."""
    n = len(si)
    pool, n_obs = (np.zeros(1, dm.ObPoint), 0) if obs is None else obs
    sc = dict(scene_in=si, obs_pool=pool, mot_pool=mot_pool, n_obs=n_obs)
    if "map" in world:
        m = world["map"]
        lane_pts, ref_pts = len(m["points"]), max(len(m["jpoints"]), 1)
    else:
        lanes, ref = world["lane_pool"], world.get("ref_pool", np.zeros(1, dm.GlobalPoint2D))
        sc.update(lane_pool=lanes, attr_pool=np.zeros(len(lanes), np.uint8), ref_pool=ref)
        lane_pts, ref_pts = len(lanes), len(ref)
    pl = dm.Planner(cfg, device=0, max_scenes=n, max_obs_total=len(pool), max_lane_pts_total=lane_pts, max_ref_pts_total=ref_pts)
    if first is not None:
        first(pl)
    if "map" in world:
        pl.set_map(m)
        pl.set_egos(sc, with_motion=with_motion)
        if route is not None:
            pl.set_route(*route_of(route, n))
    else:
        pl.set_scenes(sc, with_motion=with_motion)
    if state is None:
        state = np.zeros(n, dm.SceneState)
        pl.lib.pp_init_state(state.ctypes.data, n)
    pl.set_state(state)
    if then is not None:
        then(pl)
    if check:
        assert pl.get_scene_in().tobytes() == si.tobytes(), "the resident records are the crafted ones (views resolved, slices inside the pools)"
    return pl


def inject_advance(pl, model, po, st, trace=None, after_tick=None, before_advance=None):
    """One advance on crafted PlanOut / SceneState records (the head of this module on why).  after_tick(pl) reads what the tick
    itself left, before it is replaced; before_advance(pl) reads the handle as the advance finds it.  What is read behind the
    advance, and whether the host waits for it, is the caller's."""
    pl.tick()                                             # the tick an advance follows; what it wrote is replaced below
    if after_tick is not None:
        after_tick(pl)
    pl.write_device(dm.BUF_PLAN_OUT, po)
    pl.write_device(dm.BUF_STATE, st)
    if before_advance is not None:
        before_advance(pl)
    pl.advance_async(model, trace)


# ---- batch assembly: single-scene calls as the scenes of one launch ------------------------------------------------------------
def join_steps(cases):
    """Per step the (PlanOut, SceneState) of the cases, one behind the other."""
    return [(np.concatenate([c.steps[t][0] for c in cases]), np.concatenate([c.steps[t][1] for c in cases])) for t in range(len(cases[0].steps))]


def join_routes(routes):
    """(legs, route_first, route model) of one-scene routes laid one behind the other - the model is the first one's; None for None."""
    if routes[0] is None:
        return None
    legs, rf = [], [0]
    for r in routes:
        lg, f1, _ = route_of(r, 1)
        legs.append(lg[int(f1[0]):int(f1[1])])
        rf.append(rf[-1] + len(legs[-1]))
    return np.concatenate(legs), np.array(rf, np.int32), route_of(routes[0], 1)[2]


def join_lane_pools(cases):
    """Slice-mode lane pools laid one behind the other, equal pools once: (the pool, the offset of each case's pool,
    moved(records, sign=1): a copy of SceneIn records with the three lane views moved by sign * offset)."""
    pools, where, offs = [], {}, np.zeros(len(cases), np.int64)
    for k, c in enumerate(cases):
        p = c.world["lane_pool"]
        if p.tobytes() not in where:
            where[p.tobytes()] = sum(len(q) for q in pools)
            pools.append(p)
        offs[k] = where[p.tobytes()]

    def moved(rec, sign=1):
        rec = rec.copy()
        for name in VIEW_OFFSETS:
            rec["lanes"][name] += sign * offs.astype(np.int32)
        return rec
    return np.concatenate(pools), offs, moved


def join_world(cases):
    """(world, route, moved) of one-scene cases that share a launch: a map and the joined routes, or the joined lane pools."""
    if "map" in cases[0].world:
        return cases[0].world, join_routes([c.route for c in cases]), lambda rec, sign=1: rec
    pool, _, moved = join_lane_pools(cases)
    return dict(lane_pool=pool), None, moved


class Call:
    """A logged call: the case (an object with the call's arguments as attributes) and its results.  call[name] reads either."""
    def __init__(self, case, res):
        self.case, self.res = case, res

    def __getitem__(self, name):
        return self.res if name == "res" else getattr(self.case, name)


def case_of(steps, **fields):
    """The case of a logged call whose arguments are plain arrays: every array copied."""
    return types.SimpleNamespace(steps=[tuple(np.copy(a) for a in s) for s in steps], **{k: v.copy() if isinstance(v, np.ndarray) else v for k, v in fields.items()})


def group_calls(log, same_launch):
    """The logged calls in groups that can share a launch (same_launch(case, case)), in the order they were made."""
    groups = []
    for call in log:
        assert len(call.case.si) == 1
        for g in groups:
            if same_launch(g[0].case, call.case):
                g.append(call)
                break
        else:
            groups.append([call])
    return groups


def ends_episode(res):
    return any(int(r.stats["n_episodes"][0]) > (int(res[t - 1].stats["n_episodes"][0]) if t else 0) for t, r in enumerate(res))


def place_ends(ends, goes, n):
    """A batch of n calls with a call of `ends` first, last and on either side of the block edge 4 | 5, calls of `goes` between
    (each list in rotation; whichever is empty is filled from the other).  Returns (the batch, the indices of the calls of `ends`)."""
    assert n > 4 and n % 4 != 0
    want_end = {0, 3, 4, n - 1} if ends else set()
    e, g, batch = 0, 0, []
    for k in range(n):
        pool, idx = (ends, e) if (k in want_end or not goes) else (goes, g)
        batch.append(pool[idx % len(pool)])
        e, g = (e + 1, g) if pool is ends else (e, g + 1)
    return batch, sorted(k for k in range(n) if any(batch[k] is x for x in ends))


def batches(log, same_launch, ends_of, sizes):
    """(n, the n calls, the indices of the calls that end) for every group of calls that can share a launch and every size of `sizes`,
    a call that ends (ends_of(res)) first, last and on either side of the block edge 4 | 5 where the group has both kinds."""
    for calls in group_calls(log, same_launch):
        ends, goes = [c for c in calls if ends_of(c.res)], [c for c in calls if not ends_of(c.res)]
        for n in sizes:
            yield (n,) + place_ends(ends, goes, n)


NAMES = dict(out="SceneIn", flags="flags", trace="trace", track="EgoTrackState", state="SceneState", stats="EpisodeStats", sstats="EpisodeSpawnStats")


def same_alone(r, t, calls, attrs, obs_width=None, moved=None):
    """Step t of a batch, scene by scene, against the bytes the call gave alone, for the Result attributes `attrs`.  obs_width: the
    batch laid the scenes' obstacle slots out with this width (obs_off = k * width); moved: the lane views were (join_lane_pools)."""
    out = r.out if moved is None else moved(r.out, -1)
    for k, c in enumerate(calls):
        alone, what = c.res[t], f"batch of {len(calls)}, scene {k}, step {t}"
        for a in attrs:
            got, want = (out if a == "out" else getattr(r, a))[k], getattr(alone, a)[0]
            if a == "out" and obs_width is not None:
                want = want.copy()
                want["obs_off"] = k * obs_width
            assert (int(got) == int(want)) if a == "flags" else (got.tobytes() == want.tobytes()), f"{what}: {NAMES[a]}"


# ---- the loop of a Runner ------------------------------------------------------------------------------------------------------
def hold_run(name, res, si, model_step, compare, carried=None, trace_check=None):
    """The loop of a Runner over the results of one call: the family's trace check on either backend and, on the device, step k against
    model_step(k, records, flags, **carried) - the model applied to the device's own records of step k - 1, `carried` being what
    the model keeps from step to step (name -> value before the first step; then a copy of that attribute of the device's Result)."""
    cur, flags, carried = si, np.zeros(len(si), np.int32), dict(carried or {})
    for k, r in enumerate(res):
        if trace_check is not None:
            trace_check(r, f"{name} step {k}")
        if name == "device":
            if k:
                carried = {a: getattr(res[k - 1], a).copy() for a in carried}
            compare(r, model_step(k, cur, flags, **carried), f"step {k}")
        cur, flags = r.out, r.flags
