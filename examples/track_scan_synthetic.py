#!/usr/bin/env python3
"""A LiDAR SLAM front end on the synthetic street: the first scan is fused at its true pose, every later scan is tracked against
the map (GeoWrapper.trackPointCloud) from the previous scan's estimate and fused at the pose the tracker found.
Prints the drift against the true poses.

    python examples/track_scan_synthetic.py --scans 40 [--truncation 0.8]

The map is vbr.cfg's (20 cm voxels) with a truncation of 4 voxels instead of 2: a map that renders no ground leaves the height of
the sensor unobservable, and the five-scan street of the raycast tests renders none at 2 voxels.  This
stream — a scan every half metre, fused through the point path — still tracks at --truncation 0.4, with fewer points associated
(DESIGN.md §4.10 has both runs).  The model render is the 64 x 512 spherical camera given to setCamera.
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
    ap.add_argument("--scans", type=int, default=40)
    ap.add_argument("--truncation", type=float, default=0.8, help="sdf_truncation in metres (vbr.cfg: 0.4)")
    args = ap.parse_args()

    p = dict(synth.VBR_PARAMS, min_weight_threshold=1, sdf_truncation=args.truncation)
    near, far = p["min_depth"], 60.0
    cam = synth.spherical_camera(64, 512)
    g = GeoWrapper(
        sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=p["sdf_truncation_scale"],
        integration_weight_sample=p["integration_weight_sample"], virtual_voxel_size=p["virtual_voxel_size"],
        n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=p["voxel_extents_scale"],
        viewer_active=False, marching_cubes_threshold=p["marching_cubes_threshold"],
        min_weight_threshold=p["min_weight_threshold"], min_depth=near, max_depth=far, projective_sdf=True)
    g.setCamera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["rows"], cam["cols"], near, far, 1)

    scene = synth.street_canyon()
    poses = synth.drive_poses(args.scans)  # half a metre apart; stands in for the dataset reader
    t, q = poses[0]  # the first pose is given
    lost = 0
    track_s = 0.0
    info = None
    for i, (t_true, q_true) in enumerate(poses):
        pts = synth.lidar_scan(scene, t_true, q_true, rows=32, cols=512, max_range=far)
        if i:
            t0 = time.perf_counter()
            t_new, q_new, info = g.trackPointCloud(pts, t, q)
            track_s += time.perf_counter() - t0
            if info["status"] == 0:
                t, q = t_new, q_new
            else:
                lost += 1  # keep the last pose and go on
        g.setCurrPose(t, q)
        g.setPointCloud(pts, False)
        g.compute()
        if i and (i % 10 == 0 or i == len(poses) - 1):
            dt = float(np.linalg.norm(np.asarray(t, np.float64) - np.asarray(t_true, np.float64)))
            dr = rotation_angle_deg(synth.quat_to_rot(q), synth.quat_to_rot(q_true))
            print(f"scan {i:4d}: drift {dt * 1e3:8.2f} mm, {dr:7.4f} deg; {info['pixels']} points, rms {info['rms'] * 1e3:.2f} mm")
    g.streamAllOut()
    n = max(len(poses) - 1, 1)
    print(f"tracked {n} scans, {lost} lost, {track_s / n * 1e3:.2f} ms per trackPointCloud")


if __name__ == "__main__":
    main()
