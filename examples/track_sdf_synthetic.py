#!/usr/bin/env python3
"""The SLAM front end of examples/track_synthetic.py run twice on the synthetic Replica stream, side by side: once with the
rendering tracker (GeoWrapper.trackDepthImage) and once with the render-free one (GeoWrapper.trackDepthImageSDF,
D20), each on a map of its own.  The first frame is fused at its true pose; every later frame is tracked against the map from the
previous frame's estimate and fused at the pose the tracker found.  Prints both drifts against the true poses and the time per call.

    python examples/track_sdf_synthetic.py --frames 40 [--start 10]

The render-free tracker takes rows only from pixels that lie within the truncation of the surface at the current estimate: the
inter-frame motion has to stay inside that band, which the orbit's 31 mm and 1.8 degrees per frame do for most of the image.
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


class FrontEnd:
    def __init__(self, name, K, p, near, far):
        self.name = name
        self.g = GeoWrapper(
            sdf_truncation=p["sdf_truncation"], sdf_truncation_scale=p["sdf_truncation_scale"],
            integration_weight_sample=p["integration_weight_sample"], virtual_voxel_size=p["virtual_voxel_size"],
            n_frames_invalidate_voxels=p["n_frames_invalidate_voxels"], voxel_extents_scale=p["voxel_extents_scale"],
            viewer_active=False, marching_cubes_threshold=p["marching_cubes_threshold"],
            min_weight_threshold=p["min_weight_threshold"], min_depth=near, max_depth=far)
        self.g.setCamera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, near, far, 0)
        self.track = self.g.trackDepthImageSDF if name == "sdf" else self.g.trackDepthImage
        self.t = self.q = self.info = None
        self.lost, self.seconds = 0, 0.0

    def step(self, i, f):
        if i == 0:
            self.t, self.q = f.t, f.q  # the first pose is given
        else:
            t0 = time.perf_counter()
            t_new, q_new, self.info = self.track(f.depth, self.t, self.q)
            self.seconds += time.perf_counter() - t0
            if self.info["status"] == 0:
                self.t, self.q = t_new, q_new
            else:
                self.lost += 1  # keep the last pose and go on
        self.g.setCurrPose(self.t, self.q)
        self.g.setDepthImage(f.depth)
        self.g.setRGBImage(f.rgb)
        self.g.compute()

    def drift(self, f):
        dt = float(np.linalg.norm(np.asarray(self.t, np.float64) - f.t.astype(np.float64)))
        return f"{self.name} {dt * 1e3:7.2f} mm {rotation_angle_deg(synth.quat_to_rot(self.q), f.R):7.4f} deg, {self.info['pixels']} px, rms {self.info['rms'] * 1e3:.2f} mm"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--start", type=int, default=10, help="orbit pose of the first frame")
    args = ap.parse_args()

    K, p = synth.REPLICA_640, synth.REPLICA_PARAMS  # configurations/replica.cfg
    ends = [FrontEnd(name, K, p, 0.1, 8.0) for name in ("icp", "sdf")]
    frames = list(synth.replica_stream(args.start + args.frames))[args.start:]  # stands in for the dataset reader
    for i, f in enumerate(frames):
        for e in ends:
            e.step(i, f)
        if i and (i % 10 == 0 or i == len(frames) - 1):
            print(f"frame {i:4d}: " + " | ".join(e.drift(f) for e in ends))
    n = max(len(frames) - 1, 1)
    for e in ends:
        e.g.streamAllOut()
        print(f"{e.name}: tracked {n} frames, {e.lost} lost, {e.seconds / n * 1e3:.2f} ms per call")


if __name__ == "__main__":
    main()
