"""Point-query timing (include/mrhash_query.h): 307 200 points on the Replica stand-in after 20 fused frames — the
crossings of a 640 x 480 render from the last fused pose, as sensor-frame points in pixel order (a pixel without a hit is (0, 0, 0),
a missing return, and is refused), and the same points shuffled.  Prints one JSON line:

  <field>.<order>.us            mrh_query_points_device (all four outputs) + mrh_sync, median over >= 200 calls after a warm-up
  ... .queries_per_s            points / us
  raycast_us                    the yardstick: mrh_raycast_device (depth, normals, colours) of the same view, same run
  ... .ratio_to_raycast         us / raycast_us
  <field>.dist_fraction, .grad_fraction, refused_fraction

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_query.py` the kernels' own times are the k_query rows."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(_pos[0]) if _pos else 200
K = synth.REPLICA_640
NEAR, FAR = 0.1, 8.0


def median_us(fn, e):
    for _ in range(10):  # warm-up
        fn()
    e.sync()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        e.sync()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e6)


def crossings(depth):
    """The render's crossings as sensor-frame points [rows * cols, 3] (camera.cuh:88 with the pixel's depth); a miss is (0, 0, 0)."""
    r, c = np.mgrid[0:K.rows, 0:K.cols]
    ifx, ify = np.float32(1.0) / np.float32(K.fx), np.float32(1.0) / np.float32(K.fy)
    x = ifx * (c.astype(np.float32) - np.float32(K.cx) - np.float32(0.5))
    y = ify * (r.astype(np.float32) - np.float32(K.cy) - np.float32(0.5))
    return np.stack([depth * x, depth * y, depth], -1).reshape(-1, 3).astype(np.float32)


def main():
    p = capi.Params(num_sdf_blocks=262144, **synth.REPLICA_PARAMS)
    e = capi.Engine(capi.load_hip(), p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    for f in synth.replica_stream(20):
        e.set_pose(f.R, f.t)
        e.upload_depth(f.depth)
        e.upload_rgb(f.rgb)
        e.integrate()
    e.sync()
    view = (K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, f.R, f.t, NEAR, FAR)
    depth, _, _ = e.raycast(*view)
    pts = crossings(depth)
    n = len(pts)
    shuffled = pts[np.random.default_rng(0).permutation(n)]
    img = (hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n), hipmem.DeviceBuffer(3 * n))
    out = dict(calls=CALLS, points=n, blocks=int(e.stats().occupied_fine), hit_fraction=round(float(np.count_nonzero(depth) / depth.size), 4))
    out["raycast_us"] = round(median_us(lambda: e.raycast_device(*view, d_depth=img[0].ptr, d_normals=img[1].ptr, d_rgb=img[2].ptr), e), 1)
    bufs = (hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n), hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(n))
    for field, smooth in (("map", False), ("smooth", True)):
        for order, host in (("pixel_order", pts), ("shuffled", shuffled)):
            d_pts = hipmem.DeviceBuffer.from_numpy(host)
            us = median_us(lambda: e.query_device(d_pts.ptr, n, f.R, f.t, smooth=smooth, d_dist=bufs[0].ptr, d_grad=bufs[1].ptr, d_rgbw=bufs[2].ptr,
                                                  d_state=bufs[3].ptr), e)
            out[f"{field}.{order}"] = dict(us=round(us, 1), queries_per_s=round(n / (us * 1e-6)), ratio_to_raycast=round(us / out["raycast_us"], 3))
            if order == "pixel_order":
                state = bufs[3].to_numpy(np.uint8)
                out[f"{field}.dist_fraction"] = round(float(((state & capi.QUERY_DIST) != 0).mean()), 4)
                out[f"{field}.grad_fraction"] = round(float(((state & capi.QUERY_GRAD) != 0).mean()), 4)
                out["refused_fraction"] = round(float(((state & capi.QUERY_REFUSED) != 0).mean()), 4)
            d_pts.free()
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
