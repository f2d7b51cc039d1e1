#!/usr/bin/env python3
"""An RGB-D SLAM front end on the synthetic Replica stream: the first frame is fused at its true pose, every later frame is
tracked against the map (GeoWrapper.trackDepthImage) from the previous frame's estimate and fused at the
pose the tracker found.  Prints the drift against the true poses.

    python examples/track_synthetic.py --frames 60 [--start 10]

The stream starts at orbit pose --start.  From the orbit's first poses the camera sees one wall, the floor and the ceiling: a
translation along that wall leaves every point-to-plane residual unchanged, the first step's system is degenerate (on the analytic
model the pivot gate reports it as lost; on a one-frame map it is merely ill-conditioned), and the estimate slides along the wall.
From pose 10 on a side wall is in view and all six degrees of freedom are observable.  --start 0 shows the slide.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrhash.src.pygeowrapper import GeoWrapper  # noqa: E402  (the reference's import path)
from mrhash_amd import synth  # noqa: E402


def rotation_angle_deg(Ra, Rb):
    """Angle of Ra Rb^T from the skew part (no arccos of a trace: small angles keep their digits)."""
    D = Ra.astype(np.float64) @ Rb.astype(np.float64).T
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.rad2deg(np.arcsin(min(1.0, s))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--start", type=int, default=10, help="orbit pose of the first frame")
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

    frames = list(synth.replica_stream(args.start + args.frames))[args.start:]  # stands in for the dataset reader
    t, q = frames[0].t, frames[0].q  # the first pose is given
    lost = 0
    track_s = 0.0
    for i, f in enumerate(frames):
        if i:
            t0 = time.perf_counter()
            t_new, q_new, info = g.trackDepthImage(f.depth, t, q)
            track_s += time.perf_counter() - t0
            if info["status"] == 0:
                t, q = t_new, q_new
            else:
                lost += 1  # keep the last pose and go on
        g.setCurrPose(t, q)
        g.setDepthImage(f.depth)
        g.setRGBImage(f.rgb)
        g.compute()
        if i and (i % 10 == 0 or i == len(frames) - 1):
            dt = float(np.linalg.norm(np.asarray(t, np.float64) - f.t.astype(np.float64)))
            dr = rotation_angle_deg(synth.quat_to_rot(q), f.R)
            print(f"frame {i:4d}: drift {dt * 1e3:7.2f} mm, {dr:7.4f} deg; {info['pixels']} pixels, rms {info['rms'] * 1e3:.2f} mm")
    g.streamAllOut()
    n = max(len(frames) - 1, 1)
    print(f"tracked {n} frames, {lost} lost, {track_s / n * 1e3:.2f} ms per trackDepthImage")


if __name__ == "__main__":
    main()
