#!/usr/bin/env python3
"""The free-space layer on the synthetic Replica stream: the frames are fused and, next to every mrh_integrate,
carved into a layer of 8 cm cells around the room.

    python examples/freespace_synthetic.py [--frames 20]

  line of sight   for every pair of the camera positions the stream was fused from: is the segment between them free?  Before
                  the carve only the map can be asked (Engine.line_of_sight: observed free space by D21, which the map knows near
                  surfaces only); after it, Engine.line_of_sight_free asks the layer as well
  frontier        how many cells of the room's box are known free space next to space nothing is known about — where an
                  exploration planner goes next
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mrhash_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()

    K = synth.REPLICA_640
    p = capi.Params(num_sdf_blocks=262144, **synth.REPLICA_PARAMS)
    e = capi.Engine(capi.load_hip(), p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    shift = 3
    cell = p.virtual_voxel_size * (1 << shift)
    origin, dims = (-64, -64, -64), (128, 128, 128)  # 10.24 m per side around the orbit
    e.freespace_create(origin, dims, shift)
    frames = list(synth.replica_stream(args.frames))
    stops = np.array([np.asarray(f.t, np.float32) for f in frames][:: max(1, len(frames) // 6)])
    i, j = np.triu_indices(len(stops), 1)

    for f in frames:  # the map first, without a carve: what the readers could say before this layer existed
        e.set_pose(f.R, f.t)
        e.upload_depth(f.depth)
        e.upload_rgb(f.rgb)
        e.integrate()
    before_map = int(e.line_of_sight(stops[i], stops[j]).sum())
    before_layer = int(e.line_of_sight_free(stops[i], stops[j]).sum())
    for f in frames:  # a ray stops one cell short of its measurement: the cell that holds the surface is not carved
        e.freespace_carve_depth(f.depth, K.fx, K.fy, K.cx, K.cy, f.R, f.t, min_depth=p.min_depth, max_depth=8.0, margin=cell)
    after = e.line_of_sight_free(stops[i], stops[j])
    seg_status, seg_counts = e.freespace_segments(stops[i], stops[j])
    print(f"{len(after)} segments between {len(stops)} camera positions: {before_map} are observed free space for the map alone "
          f"(line_of_sight), {before_layer} are free before the carve and {int(after.sum())} after it (line_of_sight_free); "
          f"{int(seg_counts[:, 1].sum())} of {int(seg_counts[:, 0].sum())} samples lie in carved cells")

    st = e.freespace_box(tuple(o - 1 for o in origin), tuple(d + 2 for d in dims)[:2] + (dims[2] + 2,)) if max(dims) + 2 <= 512 else None
    n = lambda bit: int(np.count_nonzero(st & bit))  # noqa: E731
    print(f"the room's box, {dims[0] + 2} x {dims[1] + 2} x {dims[2] + 2} cells of {cell:.2f} m: {n(capi.FREE_FREE)} free, {n(capi.FREE_OBSERVED)} observed by the map, "
          f"{n(capi.FREE_OCCUPIED)} occupied, {n(capi.FREE_FRONTIER)} frontier cells; {int(np.count_nonzero(st == 0))} cells nothing is known about")
    k, jj, ii = np.nonzero(st & capi.FREE_FRONTIER)
    if len(k):
        c = (np.stack([ii, jj, k], -1).mean(0) + np.array(origin) - 0.5) * cell
        print(f"the frontier's centroid lies at {np.round(c, 2)} m")
    e.close()


if __name__ == "__main__":
    main()
