"""The two-camera rig (lk_stereo_points, lk_stereo_strain) on config 2's grid (10 000 sectors) and on
config 4's (50 176), with one and with 16 frames of synthetic records of a tilted plane that stretches, seen by the rig of
tests/stereo_ref.py scaled to the image.  Per case the medians of `reps` HIP-event times (lk_internal_stereo_last):
lk_stereo_points against a device-to-device copy of the bytes it reads and writes, timed in the same script; lk_stereo_strain
per frame, with both lane groups (LK_STEREO_GROUP) and radii of 2 and 5 pitches, against lk_strain_field of one frame's records
on the same domain and radius.  Recorded figures: no time and no ratio is asserted.

    python scripts/stereo_bench.py [--reps K]     on the GPU: writes profiles/stereo_bench.txt
    python scripts/stereo_bench.py --resources    anywhere: VGPRs, LDS and scratch of the kernels of csrc/lk_stereo.hip from a
                                                  compile with the resource remarks; asserts that none uses scratch; writes
                                                  profiles/stereo_resources.txt"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "stereo_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "stereo_resources.txt")


def resources():
    from correlation_amd import build
    lines = ["# python scripts/stereo_bench.py --resources",
             "kernel: VGPRs AGPRs SGPRs scratch[bytes/lane] waves/SIMD LDS[bytes/block]"]
    with tempfile.TemporaryDirectory() as tmp:
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run([build.hipcc_path()] + flags + ["-c", "lk_stereo.hip", "-o", os.path.join(tmp, "lk_stereo.o")], cwd=build.CSRC,
                           capture_output=True, text=True, check=True)
    scratch = []
    for block in r.stderr.split("Function Name: ")[1:]:
        mangled = block.split()[0]
        got = dict(re.findall(r"remark:\s+([A-Za-z][\w \[\]/]*): (\w+) \[", block))
        name = re.search(r"lk_stereo_\w+?_kernel", mangled).group(0)
        g = re.search(r"kernelILi(\d+)E", mangled)
        lines.append("%-36s %s %s %s %s %s %s" % (name + ("<GROUP = %s>" % g.group(1) if g else ""), got["VGPRs"], got["AGPRs"], got["TotalSGPRs"],
                                                  got["ScratchSize [bytes/lane]"], got["Occupancy [waves/SIMD]"], got["LDS Size [bytes/block]"]))
        scratch.append(int(got["ScratchSize [bytes/lane]"]))
    lines.append("# scratch, bytes per lane: at most %d over the %d kernels" % (max(scratch), len(scratch)))
    assert len(scratch) == 3 and max(scratch) == 0, lines
    return lines


def timing(reps):
    import torch
    import correlation_amd as ca
    import stereo_ref as sr
    from correlation_amd.workload import C2, C4
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    dev = torch.device("cuda", 0)
    lines = []

    def strain_field_ms(e):
        ms = C.c_float()
        fn = e.lib.lk_internal_strain_last
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
        assert fn(e._h, C.byref(ms), None, None, None) == 0
        return ms.value

    def copy_ms(n_bytes):
        """a device-to-device copy that reads and writes n_bytes in all: the median of reps"""
        src = torch.empty(n_bytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms = []
        for k in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(src)
            b.record()
            b.synchronize()
            if k >= 2:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms))

    for w in (C2, C4):
        e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
        blank = np.zeros((w.size, w.size), np.uint8)
        e.set_undeformed_image(blank)
        e.set_deformed_image(blank)
        e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
        e.commit_sectors()
        S = e.n_sectors
        cen = np.float32([e.sector_info(s)[1:] for s in range(S)])
        pitch = float(np.abs(np.diff(np.unique(cen[:, 0]))).min())
        # the test rig, its pixels scaled to this image (no lenses: their domain is the small image's)
        rig = sr.make_rig(lenses=(sr.NO_LENS, sr.NO_LENS))
        k = w.size / sr.SIZE
        for c in rig:
            for name in ("fx", "fy", "cx", "cy", "skew"):
                c[name] *= k
        cams = sr.as_records(rig)
        P_ref = sr.on_plane(rig, cen.astype(np.float64))
        t1, t2, nrm = sr.plane_basis()
        for F in (1, 16):
            frames = []
            for f in range(F):
                A = (1.0 + 0.002 * (f + 1)) * np.outer(t1, t1) + (1.0 - 0.001 * (f + 1)) * np.outer(t2, t2) + np.outer(nrm, nrm)
                frames.append((P_ref - P_ref[0]) @ A.T + P_ref[0] + np.float64([0.5, -0.25, 1.0]) * (f + 1))
            ref1, rec0, rec1 = sr.rig_records(rig, cen, P_ref, frames)
            row = {"case": w.name, "sectors": S, "frames": F, "reps": reps, "pitch": pitch}
            ms = []
            for r in range(reps + 2):
                ref_pts, pts = e.stereo_points(cams, ref1, rec0, rec1)
                if r >= 2:
                    ms.append(e.stereo_last()[0])
            assert (pts["status"] == 0).all() and (ref_pts["status"] == 0).all()
            n_bytes = S * 8 + S * 48 + 2 * F * S * 48 + (F + 1) * S * 64
            row.update(points_device_ms_median=float(np.median(ms)), points_bytes=n_bytes, copy_same_bytes_ms_median=copy_ms(n_bytes))
            row["points_over_copy"] = row["points_device_ms_median"] / row["copy_same_bytes_ms_median"]
            for pitches in (2.0, 5.0):
                radius = pitches * pitch
                ms = []
                for r in range(reps + 2):
                    e.strain_field(radius, records=rec0[0])
                    if r >= 2:
                        ms.append(strain_field_ms(e))
                base = float(np.median(ms))
                row["strain_field_ms_median_r%g" % pitches] = base
                for group in (16, 64):
                    os.environ["LK_STEREO_GROUP"] = str(group)
                    ms = []
                    for r in range(reps + 2):
                        out = e.stereo_strain(radius)
                        last = e.stereo_last()
                        if r >= 2:
                            ms.append(last[0])
                    assert last[1] == group and (out["status"] == 0).all()
                    per_frame = float(np.median(ms)) / F
                    row["stereo_strain_ms_per_frame_r%g_g%d" % (pitches, group)] = per_frame
                    row["stereo_strain_over_strain_field_r%g_g%d" % (pitches, group)] = per_frame / base
                del os.environ["LK_STEREO_GROUP"]
                e.stereo_strain(radius)
                row["default_group_r%g" % pitches], row["members_r%g" % pitches] = e.stereo_last()[1], e.stereo_last()[2]
            print(json.dumps(row), flush=True)
            lines.append(json.dumps(row))
        e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    lines = resources() if args.resources else (["# python scripts/stereo_bench.py --reps %d" % args.reps] + timing(args.reps))
    if args.resources:
        print("\n".join(lines), flush=True)
    if not args.no_write:
        with open(OUT_RESOURCES if args.resources else OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
