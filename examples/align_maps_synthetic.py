#!/usr/bin/env python3
"""Map-to-map registration on the synthetic room: the scenario of examples/fuse_maps_synthetic.py — frames 0-9 go into map A, frames
10-19 into map B, a second session whose frame is displaced from A's world by a rigid transform T — but T is recovered from the two
maps alone (Engine.align_map) from a start a few centimetres and degrees off: no depth frame of the second session
is kept, nothing is tracked, no pose is composed.  B is then fused into A under the recovered T (Engine.fuse_map) and the result is
compared with a single map of all 20 frames.

    python examples/align_maps_synthetic.py [--frames 20]

Printed: the error of the start and of the recovered transform, what the registration saw, and — as in fuse_maps_synthetic.py —
the voxels the fused map shares with the 20-frame map and the mean and 95th percentile of |sdf difference| there, for the recovered
and for the known transform.  The numbers are a record, not a test.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fuse_maps_synthetic import agreement, engine, feed, rotation  # noqa: E402
from mrhash_amd import capi, synth  # noqa: E402


def off_by(R, t, T_R, T_t):
    ang = np.degrees(np.arccos(np.clip((np.trace(np.asarray(R, np.float64) @ T_R.T) - 1) / 2, -1, 1)))
    return float(ang), 1e3 * float(np.linalg.norm(np.asarray(t, np.float64) - T_t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()
    lib = capi.load_hip()
    frames = list(synth.replica_stream(args.frames))
    half = len(frames) // 2
    T_R, T_t = rotation((0.2, 1.0, -0.3), 0.35), np.array([0.4, -0.25, 0.15])  # B's frame in A's world: W = T_R P + T_t

    whole, a, b = engine(lib), engine(lib), engine(lib)
    for f in frames:
        feed(whole, f)
    for f in frames[:half]:
        feed(a, f)
    for f in frames[half:]:  # the same camera poses, expressed in B's frame: T^-1 o pose
        feed(b, f, T_R.T @ f.R.astype(np.float64), T_R.T @ (f.t.astype(np.float64) - T_t))

    start_R, start_t = rotation((1, -2, 0.5), 0.04) @ T_R, T_t + np.array([0.03, -0.03, 0.03])
    R, t, info = a.align_map(b, start_R, start_t)
    print(f"{len(frames)} frames; map B holds frames {half} .. {len(frames) - 1}.  Start off by {off_by(start_R, start_t, T_R, T_t)[0]:.3f} deg and "
          f"{off_by(start_R, start_t, T_R, T_t)[1]:.2f} mm; align_map: status {info['status']}, {info['iterations_done']} iterations, "
          f"{info['accepted']} of {info['samples']} samples from {info['source_blocks']} blocks, rms {1e3 * info['rms']:.3f} mm; "
          f"the recovered transform is off by {off_by(R, t, T_R, T_t)[0]:.4f} deg and {off_by(R, t, T_R, T_t)[1]:.3f} mm")
    alone = agreement(a, whole)
    known = engine(lib)
    for f in frames[:half]:
        feed(known, f)
    for label, e, (FR, Ft) in (("recovered transform", a, (R, t)), ("known transform    ", known, (T_R, T_t))):
        fi = e.fuse_map(b, np.asarray(FR, np.float32), np.asarray(Ft, np.float32))
        n, mean, p95 = agreement(e, whole)
        print(f"{label}: {fi['records']} records, {fi['taken']} taken; {n} voxels shared with the {len(frames)}-frame map, |d sdf| mean {mean:.3f} mm, "
              f"p95 {p95:.3f} mm (map A alone: {alone[0]} voxels, mean {alone[1]:.3f} mm)")
    for e in (whole, a, b, known):
        e.close()


if __name__ == "__main__":
    main()
