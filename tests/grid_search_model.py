"""G2, the jump-point A* of the grid engine, restated from DESIGN §5 in plain Python integers (test infrastructure).

Written from the text of the specification, not from the kernel and not from the oracle's C: a second opinion on what the
device is held to bit for bit - the expansion order, `order_digest`, `n_pushed`, `n_rounds`, "latest push first", the entries
dropped inside a batch of four, the path rebuilt from (direction, run).

The specification as this file reads it
---------------------------------------
Grid: `W x H` bytes, row-major, non-zero = occupied.  A cell outside the grid is blocked; an occupied cell is blocked, but
for the start cell, which is free whatever its byte says.  One exception comes first: an occupied GOAL cell ends everything
with GOAL_BLOCKED before the start cell is freed - also when the goal IS the start.

Directions `0..7 = E, NE, N, NW, W, SW, S, SE`, x to the east, y to the north; a straight cell costs 10, a diagonal one 14
(a diagonal step may pass between two blocked cells: corner cutting is allowed).  `h(c) = 10 max(|dx|, |dy|) + 4 min(|dx|,
|dy|)` to the goal.

Forced neighbours.  A traveller standing on the free cell `c`, having arrived with direction `t`, has forced diagonals:
  t straight, side n (one of the two unit vectors perpendicular to t): `c + n` blocked and `c + t + n` free -> the diagonal
             `t + n` is forced;
  t diagonal (tx, ty): `c - (tx, 0)` blocked and `c + (-tx, ty)` free -> the diagonal `(-tx, ty)` is forced;
             `c - (0, ty)` blocked and `c + (tx, -ty)` free -> the diagonal `(tx, -ty)` is forced.
`jump(p, t)`, t straight: walk `c = p + t, p + 2t, ...`; c blocked -> none; c the goal -> c; c has a forced diagonal -> c.
`jump(p, t)`, t diagonal: walk at most `DIAG_JUMP = 8` cells; c blocked -> none; c the goal -> c; c has a forced diagonal
-> c; a straight jump from c along (tx, 0) or along (0, ty) finds something -> c; the 8th cell -> that cell.
Successors of a closed node p with arriving direction d, tried for `s = 0..7` in turn: the start (d = 8): `jump(p, s)` for
every s; d straight: `jump(p, d)` and the forced diagonals of (p, d); d diagonal: `jump(p, s)` for d and its two straight
components and for the forced diagonals of (p, d).

Open set: a list in push order of entries `(f, cell, arriving direction, run length)`; `g = f - h(cell)`.  It starts with
`(h(start), start, 8, 0)`, which counts as the first push.  A step: `fmin` = the smallest f in the list; up to `BATCH = 4`
entries with `f = fmin` are taken, the most recently pushed first; a taken entry whose cell is already closed (in an earlier
step, or by an entry taken before it in the same step) is dropped; the others are closed in that order - the k-th cell
closed is expansion k, `order_digest += mix64(k * 2^32 + cell)`, and `n_rounds` counts the closed entries whose f exceeds
every f closed before.  Closing the goal ends the search at once (FOUND, `path_cost = f`; entries not yet taken stay
untaken, nothing more is counted); else `n_expanded == max_expansions` ends it at once (LIMIT).  Otherwise the closed
entries of the step, in that order, push their successors, `s = 0..7` in turn; a successor is pushed whether or not its
cell is closed or already in the list.  Per push: `f >= F_LIMIT` -> COST_RANGE; else `bucket_cap` entries already in the
list -> OVERFLOW (for both only the status is defined).  An empty list at the start of a step: NO_PATH.

Path: from the goal back, every closed cell knows its arriving direction and run length; all cells start .. goal.  Longer
than `max_path` cells: PATH_TRUNC, the last `max_path` cells (`path_len = max_path`; every other field as for FOUND).

Start and goal cell of a position, and G1 itself, for every IEEE value ("Values outside the grid's range"): `cell_index`,
`cell_of` and `occupancy` below, in numpy float64 - the comparison is made on the float, the conversion afterwards.

Besides the outputs the model keeps what the coverage checks of tests/test_search_edges.py need - facts of the specified
search, not of any implementation: per step the live entries before the pop and after the push, the entries taken, those
dropped as closed earlier and those dropped as the same cell twice in the batch; the hops of the path; and for every jump
that produced a successor its direction, start, run, what ended it and the bit positions of start and stop."""

FOUND, NO_PATH, LIMIT, OVERFLOW, GOAL_BLOCKED, PATH_TRUNC, INTERNAL, COST_RANGE = range(8)
STATUS_NAMES = ["FOUND", "NO_PATH", "LIMIT", "OVERFLOW", "GOAL_BLOCKED", "PATH_TRUNC", "INTERNAL", "COST_RANGE"]

BATCH = 4
DIAG_JUMP = 8
F_LIMIT = 131070

VEC = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
DIR_OF = {v: i for i, v in enumerate(VEC)}
M64 = (1 << 64) - 1


def cell_index(v, origin, cell, n):
    """DESIGN §5 "Values outside the grid's range": the index of coordinate `v` on an axis of `n` cells.  q = floor((v - origin) /
    cell) in double; 0 when not q >= 0 (a NaN included), n - 1 when q > n - 1, else q.  Compared as floats, converted afterwards."""
    import numpy as np
    with np.errstate(all="ignore"):
        q = np.floor((np.float64(v) - np.float64(origin)) / np.float64(cell))
    if not q >= 0:
        return 0
    if q > n - 1:
        return n - 1
    return int(q)


def cell_of(W, H, cell, origin, x, y):
    """The cell `y * W + x` of a position (the start cell of the ego, the goal cell)."""
    return cell_index(y, origin[1], cell, H) * W + cell_index(x, origin[0], cell, W)


def occupancy(W, H, cell, inflate, origin, obs):
    """G1 by its definition, for every IEEE value: cell (ix, iy) is occupied iff for some obstacle R >= 0 and dx*dx + dy*dy <= R*R,
    R = (double)radius + inflate, (dx, dy) from the cell's centre origin + (i + 0.5) * cell.  A comparison with a NaN is false.
    `obs`: ObPoint records.  Returns H x W bytes."""
    import numpy as np
    grid = np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        cx = np.float64(origin[0]) + (np.arange(W, dtype=np.float64) + 0.5) * np.float64(cell)
        cy = np.float64(origin[1]) + (np.arange(H, dtype=np.float64) + 0.5) * np.float64(cell)
        for o in obs:
            R = np.float64(o["radius"]) + np.float64(inflate)
            if not R >= 0:
                continue
            dx, dy = cx - np.float64(o["x"]), cy - np.float64(o["y"])
            grid |= (dx * dx)[None, :] + (dy * dy)[:, None] <= R * R
    return grid


def mix64(v):
    """SplitMix64 finaliser."""
    z = (v + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def digest_of(order):
    return sum(mix64((k << 32) | int(c)) for k, c in enumerate(order)) & M64


class _Grid:
    """The blocked predicate over a frame of blocked cells, and the jumps."""

    def __init__(self, grid, W, H, start, goal):
        self.W, self.H, self.P = W, H, W + 2
        b = bytearray([1]) * ((W + 2) * (H + 2))
        raw = bytes(grid)
        assert len(raw) == W * H
        for y in range(H):
            row = raw[y * W:(y + 1) * W]
            b[(y + 1) * self.P + 1:(y + 1) * self.P + 1 + W] = bytes(1 if v else 0 for v in row)
        self.b = b
        self.start = self.at(start % W, start // W)
        self.goal = self.at(goal % W, goal // W)
        self.b[self.start] = 0
        self.off = tuple(dy * self.P + dx for dx, dy in VEC)
        self.memo = {}

    def at(self, x, y):
        return (y + 1) * self.P + x + 1

    def xy(self, i):
        return i % self.P - 1, i // self.P - 1

    def forced(self, i, t):
        """The forced diagonals (directions) of a traveller on cell index i that arrived with direction t."""
        b, off = self.b, self.off
        tx, ty = VEC[t]
        out = []
        if t & 1 == 0:
            for n in ((-ty, tx), (ty, -tx)):            # the two sides
                no = n[1] * self.P + n[0]
                if b[i + no] and not b[i + off[t] + no]:
                    out.append(DIR_OF[(tx + n[0], ty + n[1])])
        else:
            if b[i - tx] and not b[i - tx + ty * self.P]:
                out.append(DIR_OF[(-tx, ty)])
            if b[i - ty * self.P] and not b[i + tx - ty * self.P]:
                out.append(DIR_OF[(tx, -ty)])
        return out

    def straight(self, i, t):
        """(run, reason) of jump(i, t), t straight; run 0 = none."""
        key = (i, t)
        r = self.memo.get(key)
        if r is None:
            c, k, step = i, 0, self.off[t]
            while True:
                c += step
                k += 1
                if self.b[c]:
                    r = (0, None)
                elif c == self.goal:
                    r = (k, "goal")
                elif self.forced(c, t):
                    r = (k, "forced")
                else:
                    continue
                break
            self.memo[key] = r
        return r

    def diagonal(self, i, t):
        tx, ty = VEC[t]
        th, tv = DIR_OF[(tx, 0)], DIR_OF[(0, ty)]
        c = i
        for k in range(1, DIAG_JUMP + 1):
            c += self.off[t]
            if self.b[c]:
                return 0, None
            if c == self.goal:
                return k, "goal"
            if self.forced(c, t):
                return k, "forced"
            if self.straight(c, th)[0] or self.straight(c, tv)[0]:
                return k, "straight"
        return DIAG_JUMP, "cap"

    def jump(self, i, t):
        return self.diagonal(i, t) if t & 1 else self.straight(i, t)

    def successors(self, i, d):
        """Directions tried from a node closed with arriving direction d, ascending."""
        if d == 8:
            return list(range(8))
        if d & 1 == 0:
            return sorted([d] + self.forced(i, d))
        return sorted([d, (d + 1) & 7, (d + 7) & 7] + self.forced(i, d))


def search(grid, W, H, start, goal, max_expansions, bucket_cap, max_path, trace=True):
    """Runs G2.  `grid`: W * H bytes (row-major, non-zero = occupied); `start`, `goal`: cells `y * W + x`.

    Returns a dict: status, and - unless the status is OVERFLOW or COST_RANGE, where nothing else is defined - n_expanded,
    n_pushed, n_rounds, path_cost, path_len, order, order_digest, path; hops (the (direction, run) hops of the path); and
    with `trace`: peak_open, entries (push number -> (f, cell, direction, run)), steps, jumps (see the module docstring)."""
    raw = bytes(grid)
    if raw[goal]:
        return dict(status=GOAL_BLOCKED, n_expanded=0, n_pushed=0, n_rounds=0, path_cost=0, path_len=0, order=[], order_digest=0,
                    path=[], hops=0, peak_open=0, entries=[], steps=[], jumps=[])
    G = _Grid(raw, W, H, start, goal)
    gx, gy = goal % W, goal // W

    def h(x, y):
        dx, dy = abs(x - gx), abs(y - gy)
        return 10 * max(dx, dy) + 4 * min(dx, dy)

    entries = [(h(start % W, start // W), G.start, 8, 0)]       # by push number: (f, cell index in the frame, direction, run)
    live = [0]                                                  # push numbers, in push order
    closed = {}                                                 # frame index -> (direction, run)
    order, steps, jumps = [], [], []
    n_rounds, fmax, path_cost, peak = 0, -1, 0, 1
    status = None
    while status is None:
        if not live:
            status = NO_PATH
            break
        peak = max(peak, len(live))
        fmin = min(entries[e][0] for e in live)
        ties = [k for k in range(len(live)) if entries[live[k]][0] == fmin]
        take = ties[::-1][:BATCH]                               # positions in the list, latest push first
        rec = dict(live_before=len(live), fmin=fmin, n_ties=len(ties), tie_positions=ties, taken=[], dropped_closed=[], dropped_twice=[],
                   closed=[], pushed=[])
        batch, batch_cells, gone = [], set(), []
        for k in take:
            e = live[k]
            gone.append(k)
            rec["taken"].append(e)
            f, c, d, run = entries[e]
            if c in closed:
                rec["dropped_twice" if c in batch_cells else "dropped_closed"].append(e)
                continue
            closed[c] = (d, run)
            batch_cells.add(c)
            if f > fmax:
                fmax, n_rounds = f, n_rounds + 1
            x, y = G.xy(c)
            order.append(y * W + x)
            batch.append(e)
            rec["closed"].append(e)
            if c == G.goal:
                status, path_cost = FOUND, f
                break
            if len(order) >= max_expansions:
                status = LIMIT
                break
        for k in sorted(gone, reverse=True):
            del live[k]
        if status is None:
            for e in batch:
                f, c, d, _ = entries[e]
                x, y = G.xy(c)
                g = f - h(x, y)
                for s in G.successors(c, d):
                    run, why = G.jump(c, s)
                    if not run:
                        continue
                    nx, ny = x + run * VEC[s][0], y + run * VEC[s][1]
                    fn = g + run * (14 if s & 1 else 10) + h(nx, ny)
                    if fn >= F_LIMIT:
                        status = COST_RANGE
                        break
                    if len(live) >= bucket_cap:
                        status = OVERFLOW
                        break
                    entries.append((fn, G.at(nx, ny), s, run))
                    live.append(len(entries) - 1)
                    rec["pushed"].append(len(entries) - 1)
                    if trace:
                        a0, a1 = (x, nx) if VEC[s][0] else (y, ny)
                        jumps.append(dict(dir=s, start=(x, y), run=run, end=why, bit_start=a0 & 31, bit_stop=a1 & 31,
                                          seams=abs((a1 >> 5) - (a0 >> 5)), step=len(steps)))
                if status is not None:
                    break
        rec["live_after"] = len(live)
        peak = max(peak, len(live))
        if trace:
            steps.append(rec)
    if status in (OVERFLOW, COST_RANGE):
        return dict(status=status, peak_open=peak, steps=steps, entries=entries, jumps=jumps)
    out = dict(status=status, n_expanded=len(order), n_pushed=len(entries), n_rounds=n_rounds, path_cost=path_cost, path_len=0,
               order=order, order_digest=digest_of(order), path=[], hops=0, peak_open=peak, steps=steps, jumps=jumps,
               entries=[(f, (c // G.P - 1) * W + c % G.P - 1, d, r) for f, c, d, r in entries] if trace else [])
    if status == FOUND:
        cells, c, hops = [], G.goal, 0
        while c != G.start:
            d, run = closed[c]
            for k in range(run):
                cells.append(c - k * G.off[d])
            c -= run * G.off[d]
            hops += 1
        cells.append(G.start)
        cells.reverse()
        path = [(c // G.P - 1) * W + c % G.P - 1 for c in cells]
        out["hops"], out["full_path_len"] = hops, len(path)
        if len(path) > max_path:
            out["status"] = PATH_TRUNC
            path = path[len(path) - max_path:]
        out["path"], out["path_len"] = path, len(path)
    return out
