"""The lens recovered from rendered frames: speckle blobs carried through four shifts and a lens with
k1 = -0.03, rendered at 256 x 256 (tests/lens_ref.py: lens_frames), solved against the unshifted frame on the 12 x 12 test
domain with the true shift as the guess, then k1 and the centre fitted with a translation per frame by lk_lens_fit and taken
out by lk_lens_correct.  Reported: k1 against the truth, and the rms of the displacements about their frame mean before and
after the correction (tests/test_lens_gpu.py asserts k1 within 10 % and a ratio of at most a third; tests/test_lens_host.py
checks both on a CPU solver's records of the same frames and prints its figures, which profiles/lens_recovery.txt quotes).

    python scripts/lens_recovery.py     on the GPU: writes the device's line of profiles/lens_recovery.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "lens_recovery.txt")
SIDE, X0, N = 19, 8, 12


def report(tag, k1, sigma, centre, before, after, rms_before, rms, n):
    import lens_ref
    true = lens_ref.IMAGE_LENS["k1"]
    return ("%s: k1 %.5f +- %.2g of %.3f (%.1f %% off), centre (%.2f, %.2f) of (126, 117); rms about the frame mean %.4f -> %.4f px "
            "(ratio %.3f); residual rms %.4f -> %.4f px over %d records"
            % (tag, k1, sigma, true, 100 * abs(k1 - true) / abs(true), centre[0], centre[1], before, after, after / before, rms_before, rms, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    import correlation_amd as ca
    import lens_ref
    und, shifted = lens_ref.lens_frames()
    rects = [(X0 + SIDE * i, X0 + SIDE * j, X0 + SIDE * i + SIDE - 1, X0 + SIDE * j + SIDE - 1) for i in range(N) for j in range(N)]
    free = ca.LENS_FREE_K1 | ca.LENS_FREE_CENTRE
    start = lens_ref.make_lens(121.5, 121.5, 147.785)
    header = "# python scripts/lens_recovery.py"
    lines = [header.ljust(60) + "(on an MI355X)"]
    e = ca.HipCorrelationEngine(fitting_model=ca.FM_UVUXUYVXVY, precision=1e-3, py_stop=2)
    e.set_undeformed_image(und)
    e.set_deformed_image(shifted[0])
    for s, r in enumerate(rects):
        e.resetPolygon_rect(s, *r)
    e.commit_sectors()
    dev = np.zeros((4, len(rects)), ca.RESULT_DTYPE)
    for f, t in enumerate(lens_ref.IMAGE_SHIFTS):
        e.set_deformed_image(shifted[f])
        g = np.zeros((len(rects), 6), np.float32)
        g[:, :2] = t
        dev[f] = e.correlate_all(g)
    good = lens_ref.is_good(dev, 6, 0.0)
    got = e.lens_fit(free, ca.LENS_TRANSLATION, init=lens_ref.as_record(start), records=dev)
    out = e.lens_correct(got["lens"], records=dev)
    lines.append(report("device records, lk_lens_fit / lk_lens_correct (status %d, %d iterations)" % (got["status"], got["iterations"]),
                        float(got["lens"]["k1"]), got["sigma"][0], (got["lens"]["cx"], got["lens"]["cy"]),
                        lens_ref.spread_about_frame_mean(dev, good), lens_ref.spread_about_frame_mean(out, good),
                        got["rms_before"], got["rms"], int(got["n_records"])))
    e.close()
    print("\n".join(lines), flush=True)
    if not args.no_write:
        # the lines before this script's own header (the CPU solver's, from tests/test_lens_host.py) stay
        kept = []
        if os.path.exists(OUT):
            for line in open(OUT).read().splitlines():
                if line.startswith(header):
                    break
                kept.append(line)
        with open(OUT, "w") as f:
            f.write("\n".join(kept + lines) + "\n")


if __name__ == "__main__":
    main()
