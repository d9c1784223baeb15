"""Camera noise (lk_camera_noise, lk_sector_noise) on config 2's geometry: K = 2, 3, 8 and 16 static
frames of 2048 x 2048 in ring slots, the whole frame for the frame kernel and the 10 000 sectors of 19 x 19 for the sector
kernel.  Per call the median and minimum of `reps` HIP-event times (lk_internal_noise_last: the clearing of the tables and
the kernels) and the algorithmic rate, K x rows x cols bytes over that time - the frame kernel reads K bytes per pixel and
nothing else.  Beside it the rate of a device-to-device copy of the same byte count (torch's copy_ of a u8 tensor, timed with
events in this script on this machine; a copy reads and writes, so its traffic is twice the count).  No threshold: the file
records what was measured.  Writes one header line (date, commit, device) and one JSON line per case to --out (default
profiles/noise_bench.txt) unless --no-write.
Usage: python scripts/noise_bench.py [--reps K] [--out PATH] [--commit TEXT]"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import correlation_amd as ca  # noqa: E402
from correlation_amd.workload import C2  # noqa: E402

FRAMES = (2, 3, 8, 16)


def timed(call, e, reps):
    """-> (the last result, device ms per rep, workgroups, median host ms of the synchronous call)"""
    times, host, out, wg = [], [], None, 0
    for k in range(reps + 1):   # (the first warms up)
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        ms, wg = e.noise_last()
        if k:
            times.append(ms)
            host.append((t1 - t0) * 1e3)
    return out, np.array(times), wg, float(np.median(host))


def copy_ms(n_bytes, reps):
    """device-to-device copies of n_bytes, event-timed one by one -> ms per rep"""
    src = torch.randint(0, 256, (n_bytes,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        if k:
            times.append(a.elapsed_time(b))
    return np.array(times)


def commit_text():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_bench.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    w = C2
    e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
    und, _ = ca.speckle.speckle_pair(w.size, w.size, p=w.truth, seed=7, device="cuda")
    base = torch.as_tensor(und, device="cuda").float()
    gen = torch.Generator(device="cuda").manual_seed(11)
    K_max = max(FRAMES)
    e.sequence_reserve(K_max)
    frames = [(base + 2.0 * torch.randn(base.shape, generator=gen, device="cuda")).round().clamp(0, 255).to(torch.uint8).contiguous()
              for _ in range(K_max)]
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        e.sequence_set_frame_device(i, f.data_ptr(), w.size, w.size)
    e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
    e.commit_sectors()
    common = {"case": w.name, "image": [w.size, w.size], "reps": args.reps}
    lines = []
    for K in FRAMES:
        n_bytes = K * w.size * w.size
        rec, t, wg, call = timed(lambda: e.camera_noise(ring_first=0, n_frames=K, grey_low=5, grey_high=250, min_count=100), e, args.reps)
        c = copy_ms(n_bytes, args.reps)
        lines.append(dict(common, **{"pass": "camera_noise", "K": K, "bytes": n_bytes, "workgroups": wg,
                                     "device_ms_median": float(np.median(t)), "device_ms_min": float(t.min()), "call_ms_median": call,
                                     "GB_per_s_median": n_bytes / (float(np.median(t)) * 1e-3) / 1e9,
                                     "GB_per_s_best": n_bytes / (float(t.min()) * 1e-3) / 1e9,
                                     "copy_ms_median": float(np.median(c)), "copy_ms_min": float(c.min()),
                                     "copy_GB_per_s_median": n_bytes / (float(np.median(c)) * 1e-3) / 1e9,
                                     "status": int(rec["status"]), "sigma": float(rec["sigma"]), "a": float(rec["a"]), "b": float(rec["b"]),
                                     "bins_used": int(rec["bins_used"])}))
        print(json.dumps(lines[-1]), flush=True)
    for K in FRAMES:
        out, t, _, call = timed(lambda: e.sector_noise(ring_first=0, n_frames=K), e, args.reps)
        samples = int(out["n"].sum())
        lines.append(dict(common, **{"pass": "sector_noise", "K": K, "sectors": e.n_sectors, "samples": samples, "bytes": K * samples,
                                     "device_ms_median": float(np.median(t)), "device_ms_min": float(t.min()), "call_ms_median": call,
                                     "GB_per_s_median": K * samples / (float(np.median(t)) * 1e-3) / 1e9,
                                     "sigma_median": float(np.median(out["sigma"]))}))
        print(json.dumps(lines[-1]), flush=True)
    # a flat scene, the worst case for the workgroup's table: every pixel of every lane in one bin
    flat = torch.full((w.size, w.size), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i in range(2):
        e.sequence_set_frame_device(i, flat.data_ptr(), w.size, w.size)
    rec, t, wg, call = timed(lambda: e.camera_noise(ring_first=0, n_frames=2), e, args.reps)
    lines.append(dict(common, **{"pass": "camera_noise (flat frames, one bin)", "K": 2, "bytes": 2 * w.size * w.size, "workgroups": wg,
                                 "device_ms_median": float(np.median(t)), "device_ms_min": float(t.min()),
                                 "GB_per_s_median": 2 * w.size * w.size / (float(np.median(t)) * 1e-3) / 1e9, "status": int(rec["status"])}))
    print(json.dumps(lines[-1]), flush=True)
    e.close()
    head = json.dumps({"date": datetime.date.today().isoformat(), "commit": args.commit or commit_text(),
                       "device": torch.cuda.get_device_name(0)})
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write("\n".join([head] + [json.dumps(line) for line in lines]) + "\n")


if __name__ == "__main__":
    main()
