"""Map-to-map fusion timing (include/mrhash_remap.h): the Replica stand-in after 20 fused frames, resampled under
the generic pose of the tests (0.7 rad about (1, 2, 3) / sqrt(14), t = (0.31, -0.17, 0.23)) and fused into a second map of the same
lattice.  Prints one JSON line:

  resample_us      mrh_resample_map (blocking: selection, candidates, sort, flags, sample), median over CALLS calls after a warm-up
  fuse_us          mrh_fuse_map into a map that already holds the records (resample + MRH_UNPACK_MERGE)
  aligned_us       the yardstick, same run, same map: mrh_pack_blocks(OWNER) + mrh_unpack_blocks(MERGE) — the lattice-aligned merge
  source_blocks, candidate_blocks, records, valid_voxels, bytes_written (records * 6160), aligned_records

The phases — k_remap_candidates, the sort, k_remap_flags, k_remap_sample — are the kernel rows of
`rocprofv3 --kernel-trace --stats -- python tools/bench_remap.py 20`; the sample kernel's GB/s is bytes_written over its row."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mrhash_amd import capi, synth  # noqa: E402

_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
CALLS = int(_pos[0]) if _pos else 50
K = synth.REPLICA_640


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)).astype(np.float32)


R, T = rotation((1, 2, 3), 0.7), np.array([0.31, -0.17, 0.23], np.float32)


def median_us(fn):
    for _ in range(3):  # warm-up: the buffers grow on the first call
        fn()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()  # every call timed here blocks
        t.append(time.perf_counter() - t0)
    return round(float(np.median(t) * 1e6), 1)


def main():
    hip = capi.load_hip()
    p = capi.Params(num_sdf_blocks=262144, **synth.REPLICA_PARAMS)
    src, dst, aligned = capi.Engine(hip, p), capi.Engine(hip, p), capi.Engine(hip, p)
    src.set_camera(K.fx, K.fy, K.cx, K.cy, K.rows, K.cols, p.min_depth, p.max_depth)
    for f in synth.replica_stream(20):
        src.set_pose(f.R, f.t)
        src.upload_depth(f.depth)
        src.upload_rgb(f.rgb)
        src.integrate()
    src.sync()
    _, n, info = src.resample_map_device(R, T)
    out = dict(calls=CALLS, **{k: info[k] for k in ("source_blocks", "candidate_blocks", "records", "valid_voxels")}, bytes_written=n * capi.RECORD_BYTES)
    out["resample_us"] = median_us(lambda: src.resample_map_device(R, T))
    out["fuse_us"] = median_us(lambda: dst.fuse_map(src, R, T))

    def aligned_merge():
        ptr, m, dev = src.pack_blocks(capi.PACK_OWNER, 0)
        aligned.unpack_blocks(capi.UNPACK_MERGE, ptr, m, dev)
        return m

    out["aligned_records"] = aligned_merge()
    out["aligned_us"] = median_us(aligned_merge)
    for e in (src, dst, aligned):
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
