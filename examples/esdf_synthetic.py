#!/usr/bin/env python3
"""Clearance for a planner on the synthetic Replica stream: the frames are fused, the Euclidean signed distance field
(GeoWrapper.distanceField) of a box around the room's centre is computed in one call, and the clearance along a
straight path towards the far wall is read from it.

    python examples/esdf_synthetic.py [--frames 20] [--reach 1.0]

The field only sees surface inside its box, so the box is the region of interest padded by the reach.  Cells further than the
reach from every fused surface come back as +-reach with the "far" bit set: "at least that far".
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrhash.src.pygeowrapper import GeoWrapper  # noqa: E402  (the reference's import path)
from mrhash_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reach", type=float, default=1.0, help="metres up to which distances are exact")
    args = ap.parse_args()

    K = synth.REPLICA_640
    p = synth.REPLICA_PARAMS  # configurations/replica.cfg
    near, far = 0.1, 8.0
    g = GeoWrapper(
        sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=p["sdf_truncation_scale"],
        integration_weight_sample=p["integration_weight_sample"], virtual_voxel_size=p["virtual_voxel_size"],
        n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=p["voxel_extents_scale"],
        viewer_active=False, marching_cubes_threshold=p["marching_cubes_threshold"],
        min_weight_threshold=p["min_weight_threshold"], min_depth=near, max_depth=far)
    g.setCamera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, near, far, 0)
    for f in synth.replica_stream(args.frames):
        g.setCurrPose(f.t, f.q)
        g.setDepthImage(f.depth)
        g.setRGBImage(f.rgb)
        g.compute()

    # the path: from the room's centre towards the far wall (z = -2 m), drifting sideways and down (y points down)
    a, b = np.array([0.0, 0.0, 0.0]), np.array([0.8, 0.9, -1.9])
    lo = np.minimum(a, b) - args.reach
    hi = np.maximum(a, b) + args.reach
    t0 = time.perf_counter()
    dist, state, origin, dims = g.distanceField(lo.astype(np.float32), hi.astype(np.float32), args.reach)
    ms = (time.perf_counter() - t0) * 1e3
    vs = p["virtual_voxel_size"]
    print(f"field of {dims[0]} x {dims[1]} x {dims[2]} voxels at origin {origin}: {ms:.1f} ms, "
          f"{100.0 * np.mean((state & capi.ESDF_SITE) != 0):.2f} % surface cells, {100.0 * np.mean((state & capi.ESDF_FAR) != 0):.1f} % beyond the reach")
    print("  s [m]   position                 clearance [m]")
    n = int(np.ceil(np.linalg.norm(b - a) / 0.25))
    for k in range(n + 1):
        pnt = a + (b - a) * k / n
        i, j, kk = (np.floor(pnt / vs + 0.5).astype(int) - np.array(origin))
        d, st = float(dist[kk, j, i]), int(state[kk, j, i])
        note = " (at least)" if st & capi.ESDF_FAR else " (on the surface)" if st & capi.ESDF_SITE else ""
        print(f"  {np.linalg.norm(pnt - a):5.2f}   ({pnt[0]:+.2f}, {pnt[1]:+.2f}, {pnt[2]:+.2f})   {d:+.3f}{note}")


if __name__ == "__main__":
    main()
