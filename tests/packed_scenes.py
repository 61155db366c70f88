"""Scenes for the step planes of the packed streamed fetch (shared by the CPU and GPU tests of
tests/test_packed_fetch.py): an obstacle-free grid of 256 x 256 cells of 0.25 m with ego and goal more than 201 cells apart in
the four axis directions and along the four diagonals - every one of the eight direction codes, on paths longer than the 199
steps a record holds -, one route that two discs bend, and one path shorter than any lookahead of the sweep.  Laid out as
tests/score_scenes.py lays its cases out: padding discs outside the grid first, a case's own discs last.
"""
GRID = 256
N_OBS = 8
PAD = (-40.0, -40.0)
LOOKAHEADS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 198, 199, 200, 400]

# name -> (ego, goal, discs (x, y, r)), metres relative to the grid origin; the grid is 64 m wide
CASES = {
    "east":       ((5.0, 32.0), (59.0, 32.0), []),
    "west":       ((59.0, 32.0), (5.0, 32.0), []),
    "north":      ((32.0, 5.0), (32.0, 59.0), []),
    "south":      ((32.0, 59.0), (32.0, 5.0), []),
    "north_east": ((5.0, 5.0), (59.0, 59.0), []),
    "north_west": ((59.0, 5.0), (5.0, 59.0), []),
    "south_west": ((59.0, 59.0), (5.0, 5.0), []),
    "south_east": ((5.0, 59.0), (59.0, 5.0), []),
    "mixed":      ((5.0, 32.0), (59.0, 30.0), [(20.0, 33.0, 4.0), (42.0, 29.0, 4.0)]),
    "short":      ((5.0, 32.0), (9.0, 33.0), []),
}
CASE_NAMES = list(CASES)
LONG = CASE_NAMES[:8]                  # ego and goal at least this many cells apart
MIN_APART = 201


def config(dm, lookahead):
    cfg = dm.default_config(GRID)
    cfg["dynamic_obstacles"] = 0
    cfg["n_lattice"] = 0
    cfg["lookahead_cells"] = lookahead
    return cfg


def build(dm, cfg, names):
    """One scene per entry of `names` (a case may repeat)."""
    n = len(names)
    sc = dm.gen_scenes(cfg, 0, n, N_OBS, junction_every=0)
    si = sc["scene_in"]
    sc["mot_pool"][:] = 0
    for s, name in enumerate(names):
        ego, goal, discs = CASES[name]
        assert int(si["obs_off"][s]) == s * N_OBS and int(si["obs_n"][s]) == N_OBS and len(discs) <= N_OBS
        ox, oy = float(si["grid_origin"]["x"][s]), float(si["grid_origin"]["y"][s])
        rows = [(PAD[0] - 0.5 * i, PAD[1], 0.1) for i in range(N_OBS - len(discs))] + list(discs)
        ob = sc["obs_pool"][s * N_OBS:(s + 1) * N_OBS]
        for j, (x, y, r) in enumerate(rows):
            ob[j]["x"], ob[j]["y"], ob[j]["radius"], ob[j]["type"] = ox + x, oy + y, r, 0
        gp = si["loc"]["globalpoint"]
        gp["x"][s], gp["y"][s], gp["dir"][s] = ox + ego[0], oy + ego[1], 0.0
        si["goal"]["x"][s], si["goal"]["y"][s] = ox + goal[0], oy + goal[1]
    return sc
