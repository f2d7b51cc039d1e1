#!/usr/bin/env python3
"""Ray queries on the synthetic Replica stream: the frames are fused, then the map is asked two things a planner
asks and no render answers.

    python examples/rays_synthetic.py [--frames 20]

  line of sight     for every pair of the camera positions the stream was fused from: is the segment between them free of surfaces
                    AND of unobserved space (Engine.line_of_sight: one ray per segment, status == 0)?
  information gain  for a few candidate views — a coarse fan of 16 x 32 rays from a camera position, turned by a yaw — the share
                    of ray samples that are still unknown (Engine.cast_rays: counts[:, 1]), which is what a next-best-view
                    planner ranks views by, and the share of rays that end on a surface
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrhash_amd import capi, synth  # noqa: E402


def fan(rows, cols, yaw, v_fov=0.6, h_fov=1.2):
    """Unit directions of a rows x cols fan around the horizontal direction `yaw` (radians), world frame, row-major: neighbouring
    rays are neighbours in the list, which is the order the kernel likes."""
    el, az = np.meshgrid(np.linspace(-v_fov / 2, v_fov / 2, rows), yaw + np.linspace(-h_fov / 2, h_fov / 2, cols), indexing="ij")
    return np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], -1).reshape(-1, 3).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()

    K = synth.REPLICA_640
    p = capi.Params(num_sdf_blocks=262144, **synth.REPLICA_PARAMS)
    e = capi.Engine(capi.load_hip(), p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    stops = []
    for f in synth.replica_stream(args.frames):
        e.set_pose(f.R, f.t)
        e.upload_depth(f.depth)
        e.upload_rgb(f.rgb)
        e.integrate()
        stops.append(np.asarray(f.t, np.float32))
    e.sync()
    stops = np.array(stops[:: max(1, len(stops) // 6)])

    # A TSDF hash map stores blocks near surfaces only: space further than the truncation from every surface has no block and is
    # "unknown" to D21, however often a camera looked through it.  So the strict test (status == 0) holds for segments that stay
    # inside the band of an observed surface; "crosses no surface" (neither HIT nor INSIDE) is the test for the space between.
    i, j = np.triu_indices(len(stops), 1)
    strict = e.line_of_sight(stops[i], stops[j])
    seg = stops[j] - stops[i]
    r = e.cast_rays(stops[i], seg, max_range=float(np.linalg.norm(seg, axis=1).max()), tmax=np.linalg.norm(seg, axis=1), normals=False, colors=False)
    clear = (r["status"] & (capi.RAY_HIT | capi.RAY_INSIDE | capi.RAY_BAD)) == 0
    print(f"{len(strict)} segments between {len(stops)} camera positions: {int(clear.sum())} cross no surface, "
          f"{int(strict.sum())} are observed free space over their whole length; on average {r['counts'][:, 1].mean():.1f} of "
          f"{(r['counts'].sum(axis=1)).mean():.1f} samples of a segment are unknown")

    # the band in front of a surface IS stored: along the last camera's axis to the surface, then the last centimetres before it
    f = list(synth.replica_stream(args.frames))[-1]
    d = np.asarray(f.R, np.float32) @ np.array([0, 0, 1], np.float32)
    ahead = e.cast_rays(np.asarray(f.t, np.float32)[None], d[None], max_range=8.0)
    if ahead["status"][0] & capi.RAY_HIT:
        wall = np.asarray(f.t, np.float32) + ahead["range"][0] * d
        a = wall - 0.05 * d
        before, through = e.line_of_sight(a[None], (wall - 0.01 * d)[None], step=0.005)[0], e.line_of_sight(a[None], (wall + 0.03 * d)[None], step=0.005)[0]
        print(f"the camera's axis meets a surface {ahead['range'][0]:.3f} m out (normal {np.round(ahead['normals'][0], 2)}, {int(ahead['counts'][0, 1])} unknown and "
              f"{int(ahead['counts'][0, 0])} free samples on the way); from 5 cm to 1 cm in front of it: {'observed free space' if before else 'not free'}; "
              f"from 5 cm in front to 3 cm behind: {'free' if through else 'blocked'}")

    origin = stops[len(stops) // 2]
    rows, cols, reach = 16, 32, 8.0
    print(f"candidate views from {np.round(origin, 2)}, {rows} x {cols} rays of {reach} m each:")
    for yaw_deg in (0, 60, 120, 180, 240, 300):
        d = fan(rows, cols, np.deg2rad(yaw_deg))
        r = e.cast_rays(np.broadcast_to(origin, d.shape), d, max_range=reach, normals=False, colors=False)
        n_free, n_unknown = r["counts"][:, 0].astype(np.int64), r["counts"][:, 1].astype(np.int64)
        hit = (r["status"] & capi.RAY_HIT) != 0
        print(f"  yaw {yaw_deg:3d} deg: {100.0 * hit.mean():5.1f} % of the rays end on a surface, {n_unknown.mean():6.1f} unknown and {n_free.mean():5.1f} free samples "
              f"per ray in front of it — the fewer rays end on a surface, the more the view has left to see")
    e.close()


if __name__ == "__main__":
    main()
