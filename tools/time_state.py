"""Checkpoints at config 3 ("k_state_checksum"): the particle digest with the records current and stale, against
the copy yardstick of the same run scaled by bytes moved, and the wall time of save / load beside download / upload of the same engine,
with the blob's size per section (every feature on: tracers, a diffuse pool with crest births, two scalar channels with buoyancy and a
source, a paddle and a volume-bound body, a gate, two monitors).

  records current   the engine's bracket (SPH_OPT_TIMING, class `other`) around k_state_checksum alone: one streaming read of 80 n bytes
  records stale     after a substep in the default record mode: the digest first brings the 80-byte records up to date (class
                    `writeback`, k_writeback: it reads the engine's own arrays and writes 80 n bytes), then the same kernel
  whole call        device events on the stream around sph_state_digest(particles): kernel, the 128-byte upload of the host's sums and
                    the 128-byte read

    python tools/time_state.py [out.json]"""
import ctypes as C
import sys
import time

import numpy as np
import torch

import timing
from timing import pkg


def wall(fn, reps=5):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1000.0)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls": reps}


def main():
    cfg, rec, sp = timing.config3()
    n = len(rec)
    stream = torch.cuda.Stream()
    f = pkg.SPHFluidGPU.from_particles(rec, sp, stream=stream.cuda_stream)
    f.DispatchN(3)
    f.download()
    d = pkg.SphStateDigest()
    particles = 1 << pkg.STATE_SECTIONS.index("particles")

    def digest():
        pkg.engine._check(f._L.sph_state_digest(f._h, particles, C.byref(d)))

    res = timing.header("time_state", cfg, rec)
    res["copy_yardstick"] = dict(timing.copy_yardstick(n, stream), bytes=64 * n)
    copy_rate = 64 * n / res["copy_yardstick"]["median_us"]             # bytes per microsecond
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    kernel, _ = timing.series(f, digest)
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    res["digest_records_current"] = dict(kernel, bytes=80 * n, covers="k_state_checksum alone")
    res["digest_whole_call_records_current"] = dict(timing.events(digest, stream), covers="sph_state_digest(particles): kernel, two 128-byte copies")
    f.set_option(pkg.SPH_OPT_TIMING, 1)
    stale_other, stale_wb = [], []
    for k in range(3 + timing.REPS):
        f.DispatchCompute()
        f.kernel_times(reset=True)
        digest()
        t = f.kernel_times(reset=True)
        if k >= 3:
            stale_other.append(t["other"][0] * 1000.0)
            stale_wb.append(t["writeback"][0] * 1000.0)
    f.set_option(pkg.SPH_OPT_TIMING, 0)
    res["digest_records_stale"] = {"k_state_checksum": timing.stats(stale_other), "k_writeback": timing.stats(stale_wb),
                                   "covers": "after one substep in the default record mode: the write-back of the 80-byte records, then the kernel"}
    rate = 80 * n / kernel["median_us"]
    res["rates"] = {"digest_GBps": rate / 1e3, "copy_GBps_bytes_moved": copy_rate / 1e3, "digest_over_copy": rate / copy_rate}

    # save / load beside download / upload, every feature on
    c, ext = np.zeros(3, np.float32), float(min(sp.param_boxHalf))
    rng = np.random.default_rng(1)
    f.set_tracers((rng.random((100000, 3)).astype(np.float32) - 0.5) * np.float32(ext), history=8, stride=4)
    f.set_gates([pkg.gate(pkg.SPH_GATE_RECT, c, (ext, 0, 0), (0, 0, ext))], history=64, stride=4)
    f.set_monitor((rng.random((4096, 3)).astype(np.float32) - 0.5) * np.float32(ext), slot=0, history=16, ring_points=64)
    f.set_monitor(lattice=(c - np.float32(0.5 * ext), ext / 64.0, (64, 64, 64)), slot=1, every=4)
    f.set_diffuse(capacity=1 << 20, threshold=0.0, rate=200000.0)
    f.set_diffuse_crest(every=4)
    f.set_scalars(rng.random((n, 2)).astype(np.float32), diffusivity=0.1)
    f.set_scalar_buoyancy(beta=(0.01, 0.0), ref=0.5)
    f.set_scalar_sources([pkg.scalar_source(pkg.SPH_SOURCE_SPHERE, c, 0.2 * ext, rate=1.0)])
    f.set_obstacles([pkg.obstacle(pkg.SPH_OBSTACLE_BOX, c, (0.3 * ext, 0.2 * ext, 0.05 * ext), omega=(0, 3.0, 0)),
                     pkg.obstacle(pkg.SPH_OBSTACLE_BOX, c + np.float32(0.3 * ext), (0.1 * ext,) * 3)])
    g = (np.arange(64, dtype=np.float32) - 31.5) * np.float32(0.1 * ext / 32.0)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    f.bind_obstacle_volume(1, f.create_volume((np.sqrt(x * x + y * y + z * z) - np.float32(0.09 * ext)).astype(np.float32), 0.1 * ext / 32.0))
    f.DispatchN(8)
    need = C.c_size_t()
    pkg.engine._check(f._L.sph_state_size(f._h, C.byref(need)))
    blob = np.zeros(need.value, np.uint8)
    out = np.zeros(n, pkg.PARTICLE_DTYPE)
    res["save_ms"] = wall(lambda: pkg.engine._check(f._L.sph_state_save(f._h, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(need))))
    res["download_ms"] = wall(lambda: pkg.engine._check(f._L.sph_download_particles(f._h, out.ctypes.data_as(C.c_void_p), n)))
    res["load_ms"] = wall(lambda: pkg.engine._check(f._L.sph_state_load(f._h, blob.ctypes.data_as(C.c_void_p), blob.size)))
    res["upload_ms"] = wall(lambda: pkg.engine._check(f._L.sph_upload_particles(f._h, out.ctypes.data_as(C.c_void_p), n)))
    res["peek_ms"] = wall(lambda: pkg.state_info(blob))
    info = pkg.state_info(blob)
    res["blob_bytes"] = dict({name: s["bytes"] for name, s in info["sections"].items()}, total=int(blob.size))
    f.close()
    print({k: res[k] for k in ("rates", "save_ms", "load_ms", "download_ms", "upload_ms", "blob_bytes")})
    timing.write_json(res, timing.out_path(sys.argv[1:], "state"))


if __name__ == "__main__":
    main()
