"""Tracks and actors for the lane-traffic tests, built from the ring of tests/route_scenes.py.

A track is any polyline; the caller concatenates lane points and junction polylines.  ring_track does that for one lane number
round the whole ring (a CLOSED track: the junction from road 4 back to road 1 is followed by the closing segment onto the first
point of road 1), lane_track takes one lane alone (an OPEN track), pack turns a list of polylines into the two arrays
pp_set_traffic takes."""
import numpy as np

import route_scenes as rs

SEG = rs.PTS + rs.JPTS          # points one road and the junction behind it add to a ring track
FILL = 0xA5                     # every byte of a pool before traffic is set: an entry nobody pinned still holds it


def filled(dtype, count):
    return np.frombuffer(bytes([FILL]) * (count * np.dtype(dtype).itemsize), dtype).copy()


def lane_points(dm, m, road, lane):
    """The points of lane `lane` of road `road` (both 1-based) as GlobalPoint2D."""
    L = m["lanes"][int(m["road_first_lane"][road - 1]) + lane - 1]
    p = m["points"][int(L["point_off"]):int(L["point_off"]) + int(L["n_points"])]
    out = np.zeros(len(p), dm.GlobalPoint2D)
    out["x"], out["y"] = p["x"], p["y"]
    return out


def junction_points(dm, m, road, lane):
    """The polyline from lane `lane` of `road` to the same lane of the next road of the ring."""
    nxt = road % 4 + 1
    J = [q for q in m["junctions"] if q["last_road"] == road and q["next_road"] == nxt and q["last_lane"] == lane and q["next_lane"] == lane][0]
    return m["jpoints"][int(J["point_off"]):int(J["point_off"]) + int(J["n_points"])].copy()


def ring_track(dm, m, lane):
    """Lane `lane` (1 or 2: the lanes every road has) of roads 1 .. 4 with the junction polylines between them: 4 * 300 points.
    Point 300 (r - 1) + k is point k of the lane on road r - where an ego with loc.id = k on that lane stands."""
    parts = []
    for road in (1, 2, 3, 4):
        parts += [lane_points(dm, m, road, lane), junction_points(dm, m, road, lane)]
    return np.concatenate(parts)


def lane_track(dm, m, road, lane):
    return lane_points(dm, m, road, lane)


def pack(dm, polylines):
    """polylines: a list of (GlobalPoint2D array, closed).  Returns (TrafficTrack records, the point array)."""
    tracks = np.zeros(len(polylines), dm.TrafficTrack)
    off = 0
    for k, (p, closed) in enumerate(polylines):
        tracks[k] = (off, len(p), 1 if closed else 0, 0)
        off += len(p)
    return tracks, np.concatenate([p for p, _ in polylines]) if polylines else np.zeros(0, dm.GlobalPoint2D)


def actors(dm, rows):
    """rows: (s0, speed, scene, slot, track, type, radius) each."""
    a = np.zeros(len(rows), dm.TrafficActor)
    for k, r in enumerate(rows):
        a[k] = tuple(r) + (0,)
    return a


def polyline(dm, xy):
    p = np.zeros(len(xy), dm.GlobalPoint2D)
    p["x"], p["y"] = [q[0] for q in xy], [q[1] for q in xy]
    return p
