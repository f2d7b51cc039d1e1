"""Raycast timing (include/mrhash_raycast.h): 640x480 renders of the Replica stand-in after 20 and after 100 fused frames and of
the ScanNet stand-in, at the last fused pose.  Prints one JSON line:

  us_per_render       mrh_raycast_device + mrh_sync, median over >= 200 renders after a warm-up
  us_per_render_host  the same through mrh_raycast (blocking, read-back of depth / normals / colours included)
  rays_per_s          rows * cols / us_per_render
  hit_fraction        pixels with a hit
  fuse_render_fps     frames/s of a loop of mrh_integrate + mrh_raycast_device (no sync in between; every render restarts the
                      frame pipeline, as any map reader does) against fuse_only_fps, the same loop without the render

--spherical adds the leg "street_spherical": a 128 x 1024 spherical render (mrh_raycast_spherical_device, all four images) of
the street map fused from ten 128 x 1024 range images (drive_poses(10, 0.5), vbr.cfg parameters), at the last pose, with the same
fields plus ms_per_render; the pinhole figures come from the same run.

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_raycast.py` the kernel's own time is k_raycast's row."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, hipmem, synth  # noqa: E402

SPHERICAL = "--spherical" in sys.argv
_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
RENDERS = int(_pos[0]) if _pos else 200
K = synth.REPLICA_640
NEAR, FAR = 0.1, 8.0
hip = capi.load_hip()


def engine(params):
    p = capi.Params(num_sdf_blocks=262144, **params)
    e = capi.Engine(hip, p)
    e.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    return e


def feed(e, f):
    e.set_pose(f.R, f.t)
    e.upload_depth(f.depth)
    e.upload_rgb(f.rgb)
    e.integrate()


def time_renders(e, f, bufs):
    args = (K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, f.R, f.t, NEAR, FAR)
    for _ in range(10):  # warm-up
        e.raycast_device(*args, d_depth=bufs[0].ptr, d_normals=bufs[1].ptr, d_rgb=bufs[2].ptr)
    e.sync()
    dev = []
    for _ in range(RENDERS):
        t0 = time.perf_counter()
        e.raycast_device(*args, d_depth=bufs[0].ptr, d_normals=bufs[1].ptr, d_rgb=bufs[2].ptr)
        e.sync()
        dev.append(time.perf_counter() - t0)
    host = []
    for _ in range(RENDERS):
        t0 = time.perf_counter()
        depth, _, _ = e.raycast(*args)
        host.append(time.perf_counter() - t0)
    us = float(np.median(dev) * 1e6)
    return dict(us_per_render=round(us, 1), us_per_render_host=round(float(np.median(host) * 1e6), 1),
                rays_per_s=round(K.rows * K.cols / (us * 1e-6)), hit_fraction=round(float(np.count_nonzero(depth) / depth.size), 4))


def spherical_leg():
    cam = synth.spherical_camera(128, 1024)
    args = (cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["rows"], cam["cols"])
    p = capi.Params(num_sdf_blocks=262144, **synth.VBR_PARAMS)
    e = capi.Engine(hip, p)
    e.set_camera(*args, p.min_depth, p.max_depth, model=1)
    scene = synth.street_canyon()
    for t, q in synth.drive_poses(10, 0.5):
        depth, rgb = synth.spherical_range_image(scene, t, q, cam)
        R = synth.quat_to_rot(q)
        e.set_pose(R, t)
        e.upload_depth(depth)
        e.upload_rgb(rgb)
        e.integrate()
    e.sync()
    n = cam["rows"] * cam["cols"]
    bufs = (hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n), hipmem.DeviceBuffer(3 * n), hipmem.DeviceBuffer(12 * n))
    pose = (R, t, p.min_depth, p.max_depth)
    dev_kw = dict(d_range=bufs[0].ptr, d_normals=bufs[1].ptr, d_rgb=bufs[2].ptr, d_points=bufs[3].ptr)
    for _ in range(10):  # warm-up
        e.raycast_spherical_device(*args, *pose, **dev_kw)
    e.sync()
    dev, host = [], []
    for _ in range(RENDERS):
        t0 = time.perf_counter()
        e.raycast_spherical_device(*args, *pose, **dev_kw)
        e.sync()
        dev.append(time.perf_counter() - t0)
    for _ in range(RENDERS):
        t0 = time.perf_counter()
        rng = e.raycast_spherical(*args, *pose, points=True)[0]
        host.append(time.perf_counter() - t0)
    us = float(np.median(dev) * 1e6)
    out = dict(rows=cam["rows"], cols=cam["cols"], min_depth=p.min_depth, max_depth=p.max_depth, us_per_render=round(us, 1),
               ms_per_render=round(us * 1e-3, 3), us_per_render_host=round(float(np.median(host) * 1e6), 1), rays_per_s=round(n / (us * 1e-6)),
               hit_fraction=round(float(np.count_nonzero(rng) / rng.size), 4), blocks=int(e.stats().occupied_fine))
    e.close()
    return out


def fuse_fps(frames, params, bufs, render):
    e = engine(params)
    feed(e, frames[0])
    e.sync()
    t0 = time.perf_counter()
    for f in frames[1:]:
        feed(e, f)
        if render:
            e.raycast_device(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, f.R, f.t, NEAR, FAR, d_depth=bufs[0].ptr, d_normals=bufs[1].ptr, d_rgb=bufs[2].ptr)
    e.sync()
    fps = (len(frames) - 1) / (time.perf_counter() - t0)
    e.close()
    return round(fps, 1)


def main():
    n = K.rows * K.cols
    bufs = (hipmem.DeviceBuffer(4 * n), hipmem.DeviceBuffer(12 * n), hipmem.DeviceBuffer(3 * n))
    out = {"renders": RENDERS, "rows": K.rows, "cols": K.cols, "min_depth": NEAR, "max_depth": FAR}
    replica = list(synth.replica_stream(100))
    e = engine(synth.REPLICA_PARAMS)
    for i, f in enumerate(replica):
        feed(e, f)
        if i + 1 in (20, 100):
            e.sync()
            out[f"replica_{i + 1}"] = dict(time_renders(e, f, bufs), blocks=int(e.stats().occupied_fine))
    e.close()
    scannet = list(synth.scannet_stream(60))
    e = engine(synth.SCANNET_PARAMS)
    for f in scannet:
        feed(e, f)
    e.sync()
    out["scannet_60"] = dict(time_renders(e, scannet[-1], bufs), blocks=int(e.stats().occupied_fine))
    e.close()
    out["fuse_only_fps"] = fuse_fps(replica, synth.REPLICA_PARAMS, bufs, False)
    out["fuse_render_fps"] = fuse_fps(replica, synth.REPLICA_PARAMS, bufs, True)
    if SPHERICAL:
        out["street_spherical"] = spherical_leg()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
