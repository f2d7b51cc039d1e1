#!/usr/bin/env python3
"""Map-to-map fusion on the synthetic room: frames 0-9 go into map A; frames 10-19 go into map B, a second session whose frame is
displaced from A's world by a rigid transform T.  B is fused into A (Engine.fuse_map) once with the known T and once
with the T recovered by tracking B's first depth frame against A (Engine.track_depth), and the result is compared with a single map
of all 20 frames.

    python examples/fuse_maps_synthetic.py [--frames 20]

Printed: per variant, the voxels the fused map shares with the 20-frame map, the mean and 95th percentile of |sdf difference| there,
and — as the baseline — the same for map A alone.  The numbers are a record, not a test.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrhash_amd import capi, synth  # noqa: E402

K = synth.REPLICA_640


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def engine(lib):
    p = capi.Params(num_sdf_blocks=131072, **synth.REPLICA_PARAMS)
    e = capi.Engine(lib, p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    return e


def feed(e, f, R=None, t=None):
    e.set_pose(f.R if R is None else R, f.t if t is None else t)
    e.upload_depth(f.depth)
    e.upload_rgb(f.rgb)
    e.integrate()


def agreement(e, ref):
    """(shared observed voxels, mean |d sdf| in mm, 95th percentile in mm) between two maps of one lattice."""
    (da, va), (db, vb) = e.dump_blocks(), ref.dump_blocks()
    key = lambda d: (d["x"].astype(np.int64) << 42) + (d["y"].astype(np.int64) << 21) + d["z"]  # noqa: E731
    _, ia, ib = np.intersect1d(key(da), key(db), return_indices=True)
    a, b = va[ia], vb[ib]
    both = (a["weight"] > 0) & (b["weight"] > 0)
    diff = np.abs(a["sdf"][both].astype(np.float64) - b["sdf"][both])
    return int(both.sum()), 1e3 * float(diff.mean()), 1e3 * float(np.percentile(diff, 95))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()
    lib = capi.load_hip()
    frames = list(synth.replica_stream(args.frames))
    half = len(frames) // 2
    T_R, T_t = rotation((0.2, 1.0, -0.3), 0.35), np.array([0.4, -0.25, 0.15])  # B's frame in A's world: W = T_R P + T_t

    whole, b = engine(lib), engine(lib)
    for f in frames:
        feed(whole, f)
    for f in frames[half:]:  # the same camera poses, expressed in B's frame: T^-1 o pose
        feed(b, f, T_R.T @ f.R.astype(np.float64), T_R.T @ (f.t.astype(np.float64) - T_t))
    vs = synth.REPLICA_PARAMS["virtual_voxel_size"]
    print(f"{len(frames)} frames, voxel {1e3 * vs:.0f} mm; map B holds frames {half} .. {len(frames) - 1} in a frame displaced by "
          f"{np.degrees(0.35):.1f} deg and {np.linalg.norm(T_t):.2f} m")

    def fused(R, t, label):
        a = engine(lib)
        for f in frames[:half]:
            feed(a, f)
        alone = agreement(a, whole)
        info = a.fuse_map(b, R.astype(np.float32), t.astype(np.float32))
        n, mean, p95 = agreement(a, whole)
        print(f"{label}: {info['records']} records of {info['candidate_blocks']} candidate blocks, {info['valid_voxels']} voxels, {info['taken']} taken; "
              f"{n} voxels shared with the {len(frames)}-frame map, |d sdf| mean {mean:.3f} mm, p95 {p95:.3f} mm "
              f"(map A alone: {alone[0]} voxels, mean {alone[1]:.3f} mm)")
        return a

    a = fused(T_R, T_t, "known transform    ")
    # the transform from tracking: B's first frame has the pose (R_B, t_B) in B; tracked against A it has (R_A, t_A) in A's world;
    # T = pose_A o pose_B^-1.  The start is the true pose, off by 3 cm and about a degree
    f = frames[half]
    R_B, t_B = T_R.T @ f.R.astype(np.float64), T_R.T @ (f.t.astype(np.float64) - T_t)
    a0 = engine(lib)
    for g in frames[:half]:
        feed(a0, g)
    start_R = rotation((1, 1, 0), 0.02) @ f.R.astype(np.float64)
    start_t = f.t.astype(np.float64) + np.array([0.02, -0.02, 0.01])
    p = a0.params
    R_A, t_A, info = a0.track_depth(f.depth, K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, start_R, start_t, p.min_depth, p.max_depth)
    a0.close()
    R_A, t_A = R_A.astype(np.float64), t_A.astype(np.float64)
    u, _, vt = np.linalg.svd(R_A @ R_B.T)  # the product of two float rotations, back onto a rotation
    est_R = u @ vt
    est_t = t_A - est_R @ t_B
    ang = np.degrees(np.arccos(np.clip((np.trace(est_R @ T_R.T) - 1) / 2, -1, 1)))
    print(f"tracking: status {info['status']}, {info['pixels']} pixels, rms {1e3 * info['rms']:.2f} mm; the recovered transform is off by "
          f"{ang:.3f} deg and {1e3 * np.linalg.norm(est_t - T_t):.2f} mm")
    a2 = fused(est_R, est_t, "recovered transform")
    for e in (a, a2, b, whole):
        e.close()


if __name__ == "__main__":
    main()
