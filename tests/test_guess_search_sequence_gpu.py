"""The automatic initial guess inside tracked sequences (lk_tracker_set_guess_search): frame 0 of a 9-frame speckle
sequence is offset by about 30 px, beyond the LM solve's capture range.  Every frame loop of lk_sequence_run - windows,
pair by pair (LK_SEQ_WINDOW=1), synchronous (LK_SEQ_SYNC=1), with the device-guess check (LK_SEQ_CHECK=1) - must give the
same frame_results and report text, and frame 0 must start from the searched guesses."""
import numpy as np
import pytest

import correlation_amd as ca
from correlation_amd import tracker as tk

pytestmark = pytest.mark.gpu

RADIUS, LEVEL = 20, 1


@pytest.fixture(scope="module")
def frames():
    und = ca.speckle.speckle_pair(384, 384, seed=23)[0]
    return [und] + [ca.speckle.speckle_pair(384, 384, p=(29.0 + 0.6 * k, -17.0 - 0.4 * k, 0.001, 0.0, 0.0, -0.001),
                                            seed=23)[1] for k in range(8)]


def engine():
    e = ca.HipCorrelationEngine()
    e.set_batch_invariant(True)
    return e


def rect_tracker():
    t = tk.SequenceTracker(ca.FM_UVUXUYVXVY, tk.DOMAIN_RECT)
    t.set_rect_domain(70.0, 70.0, 313.0, 313.0, 191.5, 191.5, 8, 8)
    t.set_guess_search(RADIUS, level=LEVEL)
    return t


def run(frames, env, monkeypatch):
    for k in ("LK_SEQ_WINDOW", "LK_SEQ_SYNC", "LK_SEQ_CHECK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e, t = engine(), rect_tracker()
    assert tk.run_sequence(e, t, frames) == len(frames) - 1
    out = (t.results(), t.report(), e.guess_search_info())
    e.close()
    t.close()
    return out


def test_every_frame_loop_gives_the_same_results_from_the_searched_guesses(frames, monkeypatch):
    base_res, base_rep, base_info = run(frames, {}, monkeypatch)
    assert (base_info["status"] == ca.GS_OK).all()
    assert (base_res["error_code"] == ca.ERROR_NONE).mean() > 0.95
    for env in ({"LK_SEQ_WINDOW": "1"}, {"LK_SEQ_SYNC": "1"}, {"LK_SEQ_CHECK": "1"}, {"LK_SEQ_CHECK": "1", "LK_SEQ_WINDOW": "1"}):
        res, rep, info = run(frames, env, monkeypatch)
        assert res.tobytes() == base_res.tobytes(), env
        assert rep == base_rep, env
        assert info.tobytes() == base_info.tobytes(), env
    # without the search the same sequence does not track (the offset is beyond the solve's capture range)
    e, t = engine(), rect_tracker()
    t.set_guess_search(0)
    tk.run_sequence(e, t, frames)
    plain = t.results()
    assert ((plain["error_code"] != ca.ERROR_NONE) | (np.abs(plain["resulting_parameters"][:, :2] -
                                                             base_res["resulting_parameters"][:, :2]).max(1) > 1)).mean() > 0.5
    e.close()
    t.close()


def test_frame_zero_starts_from_the_search(frames, monkeypatch):
    monkeypatch.delenv("LK_SEQ_WINDOW", raising=False)
    e, t = engine(), rect_tracker()
    tk.run_sequence(e, t, frames[:2])
    info = e.guess_search_info()
    g = t.results()["initial_guess"]
    assert g[:, 0].tolist() == ((info["center_x"] + info["shift_x"]) * (1 << LEVEL)).astype(np.float32).tolist()
    assert g[:, 1].tolist() == ((info["center_y"] + info["shift_y"]) * (1 << LEVEL)).astype(np.float32).tolist()
    assert t.results()["previous_resulting_parameters"].tobytes() == g.tobytes()
    e.close()
    t.close()


def test_annular_sync_path_equals_a_python_driven_loop(frames):
    def tracker():
        t = tk.SequenceTracker(ca.FM_UVUXUYVXVY, tk.DOMAIN_ANNULAR)
        t.set_annular_domain(40.0, 150.0, 191.5, 191.5, 3, 8)
        return t

    e, t = engine(), tracker()
    t.set_guess_search(RADIUS, level=LEVEL)
    tk.run_sequence(e, t, frames)
    want_res, want_rep = t.results(), t.report()
    e.close()
    t.close()

    e, t = engine(), tracker()
    e.set_undeformed_image(frames[0])
    for k in range(len(frames) - 1):
        e.set_deformed_image(frames[k + 1])
        cmds, guesses = t.begin_frame(k)
        if k == 0:
            for s, c in enumerate(cmds):
                assert c["kind"] == tk.SECTOR_ANNULAR
                e.resetPolygon_annular(s, c["r"], c["dr"], c["a"], c["da"], c["cx"], c["cy"], c["as"])
            e.commit_sectors()
            guesses = e.search_guesses(RADIUS, level=LEVEL, guesses=guesses)
            t.override_guesses(guesses)
        rec = e.correlate_all(guesses)
        t.end_frame(k, "frame0", f"frame{k + 1}", rec)
    assert t.results().tobytes() == want_res.tobytes()
    assert t.report() == want_rep
    assert (want_res["error_code"] == ca.ERROR_NONE).mean() > 0.9
    e.close()
    t.close()
