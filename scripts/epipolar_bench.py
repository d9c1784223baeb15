"""The stereo initial guess along the epipolar curve (lk_search_epipolar) on config 2's grid (10 000
sectors of 19 x 19) and config 4's (50 176 of 7 x 7) at pyramid levels 1 and 2, bands 1 and 2, 17 nodes, on a speckle pair and
the rig of tests/stereo_ref.py scaled to the image (no lenses: their domain is the small image's).  The depth range is chosen
per level so that a curve has about 41 stations, the length of the test rig's curves at level 1.  Per case the medians of `reps`
calls: the two kernels by HIP events and the host's curve table by its own clock (lk_internal_epipolar_last), the whole
asynchronous call by the wall clock, the search kernel once more under the cut by node (LK_EPIPOLAR_RUNS=1), and - the yardstick, in the same script and run - lk_search_guesses at the same level
about the middle of every curve with the radius that covers the longest curve, by the wall clock from the call to the end of
the stream (there is no event hook for it; min_samples = 1 for both, so that config 4's 3 x 3 level-2 sectors are searched).
Recorded figures: no time and no ratio is asserted.

    python scripts/epipolar_bench.py [--reps K]     on the GPU: writes profiles/epipolar_bench.txt
    python scripts/epipolar_bench.py --resources    anywhere: VGPRs, LDS and scratch of the kernels of csrc/lk_epipolar_search.hip
                                                    from a compile with the resource remarks; asserts that none uses scratch;
                                                    writes profiles/epipolar_resources.txt"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "epipolar_bench.txt")
OUT_RESOURCES = os.path.join(ROOT, "profiles", "epipolar_resources.txt")


def resources():
    from correlation_amd import build
    lines = ["# python scripts/epipolar_bench.py --resources",
             "kernel: VGPRs AGPRs SGPRs scratch[bytes/lane] waves/SIMD static-LDS[bytes/block]"]
    with tempfile.TemporaryDirectory() as tmp:
        flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run([build.hipcc_path()] + flags + ["-c", "lk_epipolar_search.hip", "-o", os.path.join(tmp, "lk_epipolar_search.o")],
                           cwd=build.CSRC, capture_output=True, text=True, check=True)
    scratch = []
    for block in r.stderr.split("Function Name: ")[1:]:
        mangled = block.split()[0]
        got = dict(re.findall(r"remark:\s+([A-Za-z][\w \[\]/]*): (\w+) \[", block))
        name = re.search(r"lk_epipolar_\w+?_kernel", mangled).group(0)
        g = re.search(r"kernelILb(\d)E", mangled)
        lines.append("%-40s %s %s %s %s %s %s" % (name + ("<shape = %s>" % g.group(1) if g else ""), got["VGPRs"], got["AGPRs"], got["TotalSGPRs"],
                                                  got["ScratchSize [bytes/lane]"], got["Occupancy [waves/SIMD]"], got["LDS Size [bytes/block]"]))
        scratch.append(int(got["ScratchSize [bytes/lane]"]))
    lines.append("# scratch, bytes per lane: at most %d over the %d kernels" % (max(scratch), len(scratch)))
    lines.append("# dynamic LDS of the search kernel: 8 bytes per candidate and 4 per station of the launch's longest run, 5120 for the")
    lines.append("# template chunk, and the window bound of the launch (lk_epipolar_search.cpp; profiles/epipolar_bench.txt has it per case).")
    lines.append("# A workgroup is 4 waves, one per SIMD: the registers allow as many workgroups per CU as waves per SIMD above; with a")
    lines.append("# window of a few hundred bytes a workgroup holds about 11.5 KB of LDS with its static part, 13 per CU of 160 KB, so the")
    lines.append("# registers bound the occupancy of small sectors and the window that of large ones")
    assert len(scratch) == 3 and max(scratch) == 0, lines
    return lines


def timing(reps):
    import correlation_amd as ca
    import stereo_ref as sr
    from correlation_amd.workload import C2, C4
    lines = []
    for w in (C2, C4):
        und, dfm = ca.speckle.speckle_pair(w.size, w.size, p=(6.0, -2.0, 0.0, 0.0, 0.0, 0.0), seed=3)
        e = ca.HipCorrelationEngine(fitting_model=w.model, py_stop=w.py_stop)
        e.set_undeformed_image(und)
        e.set_deformed_image(dfm)
        e.set_rect_grid(w.x_begin, w.x_begin, w.x_end, w.x_end, w.hs, w.vs)
        e.commit_sectors()
        S = e.n_sectors
        cen = np.float32([e.sector_info(s)[1:] for s in range(S)])
        rig = sr.make_rig(lenses=(sr.NO_LENS, sr.NO_LENS))
        k = w.size / sr.SIZE
        for c in rig:
            for name in ("fx", "fy", "cx", "cy", "skew"):
                c[name] *= k
        cams = sr.as_records(rig)
        for level in (1, 2):
            # about 41 stations: the disparity is f b / z pixels, so its range over the depths is f b (1 / z_near - 1 / z_far)
            spread = 40.0 * (1 << level) / (rig[0]["fx"] * sr.BASELINE)
            z_near, z_far = 1.0 / (1.0 / sr.Z0 + spread / 2), 1.0 / (1.0 / sr.Z0 - spread / 2)
            for band in (1, 2):
                table = ca.epipolar_curves(cams, cen, z_near, z_far, level, band=band)
                n_st = table["curves"]["n_stations"]
                radius = int(min(ca._ffi.GS_MAX_RADIUS, np.ceil((n_st.max() - 1) / 2 + band)))
                row = {"case": w.name.split(":")[0], "sectors": S, "level": level, "band": band, "nodes": 17, "reps": reps,
                       "stations_per_sector": float(n_st.mean()), "candidates_per_sector": float(n_st.mean() * (2 * band + 1)),
                       "square_radius": radius, "square_candidates_per_sector": (2 * radius + 1) ** 2}
                row["candidate_ratio"] = row["candidates_per_sector"] / row["square_candidates_per_sector"]
                def timed():
                    search, reduce_, curves, wall = [], [], [], []
                    for r in range(reps + 2):           # (two calls first: allocations, code upload, clocks)
                        assert e.lib.lk_synchronize(e._h) == 0
                        t0 = time.perf_counter()
                        e.search_epipolar(cams, z_near, z_far, level=level, band=band, min_samples=1)
                        assert e.lib.lk_synchronize(e._h) == 0
                        t1 = time.perf_counter()
                        last = e.epipolar_last()
                        if r >= 2:
                            search.append(last[0]), reduce_.append(last[1]), curves.append(last[2]), wall.append((t1 - t0) * 1e3)
                    return search, reduce_, curves, wall, last
                # the other cut first: a workgroup per (sector, node), what shape = 1 uses, forced onto shape 0 by the library's hook
                os.environ["LK_EPIPOLAR_RUNS"] = "1"
                by_node = timed()
                del os.environ["LK_EPIPOLAR_RUNS"]
                row.update(by_node_search_kernel_ms_median=float(np.median(by_node[0])), by_node_longest_run=by_node[4][5])
                search, reduce_, curves, wall, last = timed()
                info = e.epipolar_search_info()
                row.update(search_kernel_ms_median=float(np.median(search)), reduce_kernel_ms_median=float(np.median(reduce_)),
                           host_curves_ms_median=float(np.median(curves)), whole_call_wall_ms_median=float(np.median(wall)),
                           lds_window_bytes=last[4], longest_run=last[5], ok_sectors=int((info["status"] == ca.GS_OK).sum()))
                # the yardstick: the square search about the middle of every curve
                mid = np.zeros((S, 6), np.float32)
                first = table["curves"]["first_index"] + n_st // 2
                mid[:, 0] = (table["curves"]["first_station"] + n_st // 2) * (1 << level)
                mid[:, 1] = table["other"][first] * (1 << level)
                e.search_guesses(0, level=level, guesses=mid, min_samples=1, min_score=2.0)      # (uploads them; writes none)
                sq = []
                for r in range(reps + 2):
                    e.search_guesses(0, level=level, guesses=mid, min_samples=1, min_score=2.0)
                    assert e.lib.lk_synchronize(e._h) == 0
                    t0 = time.perf_counter()
                    e.search_guesses(radius, level=level, min_samples=1, min_score=2.0)
                    assert e.lib.lk_synchronize(e._h) == 0
                    if r >= 2:
                        sq.append((time.perf_counter() - t0) * 1e3)
                row["square_search_wall_ms_median"] = float(np.median(sq))
                # two quotients: the kernels alone (HIP events) over the square search (wall clock: launch overhead and the binding
                # are in its figure, a few per cent in the new pass's favour), and call against call on the same wall clock
                row["kernels_over_square"] = (row["search_kernel_ms_median"] + row["reduce_kernel_ms_median"]) / row["square_search_wall_ms_median"]
                row["whole_call_over_square"] = row["whole_call_wall_ms_median"] / row["square_search_wall_ms_median"]
                row["by_node_kernels_over_square"] = (row["by_node_search_kernel_ms_median"] + row["reduce_kernel_ms_median"]) / row["square_search_wall_ms_median"]
                row["host_curves_over_kernels"] = row["host_curves_ms_median"] / (row["search_kernel_ms_median"] + row["reduce_kernel_ms_median"])
                print(json.dumps(row), flush=True)
                lines.append(json.dumps(row))
        e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = resources() if args.resources else (["# python scripts/epipolar_bench.py --reps %d" % args.reps] + timing(args.reps))
    if args.resources:
        print("\n".join(lines), flush=True)
    if not args.no_write:
        with open(args.out or (OUT_RESOURCES if args.resources else OUT), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
