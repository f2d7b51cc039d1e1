#!/usr/bin/env python3
"""Point queries on the synthetic Replica stream: the frames are fused, a LiDAR view of the map is rendered from the last pose
(GeoWrapper.raycastScan), and its crossings — sensor-frame points, (0, 0, 0) where a ray hit nothing — are handed back to the map
as a list of positions (GeoWrapper.queryPoints with sensor_frame=True): distance, gradient and colour per point.

    python examples/query_synthetic.py [--frames 20] [--rows 32] [--cols 512]

The points are crossings of the map's own field, so their distance should be close to 0 in both fields: exactly the residual a
scan-to-map registration would minimise.  The MAP field is the one the render used (the mean of eight cells, piecewise constant
inside a dual cell); the SMOOTH field is the continuous one a planner or a registration differentiates.
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
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--cols", type=int, default=512)
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

    cam = synth.spherical_camera(args.rows, args.cols)
    g.setCamera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["rows"], cam["cols"], near, far, 1)  # the LiDAR's view, same pose
    rng, _, _, points = g.raycastScan()
    hits = rng.reshape(-1) > 0
    print(f"LiDAR view of {args.rows} x {args.cols} rays: {100.0 * hits.mean():.1f} % hit the map")
    for smooth in (False, True):
        t0 = time.perf_counter()
        dist, grad, rgbw, state = g.queryPoints(points, smooth=smooth, sensor_frame=True)
        ms = (time.perf_counter() - t0) * 1e3
        refused = (state & capi.QUERY_REFUSED) != 0
        valid = (state & capi.QUERY_DIST) != 0
        assert np.array_equal(refused, ~hits)  # a miss is (0, 0, 0): refused, every output 0
        has_grad = (state & capi.QUERY_GRAD) != 0
        norm = np.linalg.norm(grad[has_grad], axis=1)
        coloured = rgbw[~refused, 3] > 0
        print(f"{'SMOOTH' if smooth else 'MAP   '} field: {ms:6.2f} ms, distance at {100.0 * valid[hits].mean():.1f} % of the crossings, "
              f"mean |dist| {1e3 * np.abs(dist[valid]).mean():.3f} mm (voxel {1e3 * p['virtual_voxel_size']:.0f} mm), "
              f"gradient at {100.0 * has_grad[hits].mean():.1f} % with mean norm {norm.mean():.3f}, {100.0 * coloured.mean():.1f} % coloured")


if __name__ == "__main__":
    main()
