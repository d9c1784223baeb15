"""The fixture of tests/test_solve_instances_gpu.py on the CPU: what the oracle gives on it is what the GPU tests assume, and
the float terms of an evaluation (solve_instances_ref.eval_terms) are the oracle's own - its sequential float sums lie
within the rounding bound of one chain over all samples around their float64 sum."""
import numpy as np
import pytest

import correlation_amd as ca

import solve_instances_ref as si


@pytest.mark.parametrize("model,interp", si.CASES, ids=si.CASE_IDS)
def test_oracle_facts_of_the_fixture(oracle, model, interp):
    want = si.assert_oracle_facts(oracle, model, interp)
    assert want["error_code"][si.LEAVES] == si.OUT_OF_IMAGE
    # the centres: an implicit rectangle's own, the one given with the list, the float mean of the annular samples
    for s in range(si.S):
        c = si.given_center(s)
        if c is not None:
            assert (want["und_cx"][s], want["und_cy"][s]) == c
    win = si.oracle_window(oracle, model, interp)
    assert win.shape == (si.WINDOW_FRAMES, len(si.WINDOW_SECTORS)) and (win["error_code"] == 0).all()
    if interp != ca.IM_NEAREST:      # the sequence tracks: three more times the truth's 0.6 px between the first and the last frame
        assert (win["p"][-1, :, 0] - win["p"][0, :, 0] > 1.0).all(), win["p"][:, :, 0]


def test_the_groups_restate_the_size_classes():
    import frame_shapes_ref as fs
    assert tuple(fs.GROUP_OF_CLASS[fs.size_class(n)] for n in si.COUNTS) == si.NATURAL_GROUPS
    assert tuple(16 if fs.size_class(n) == 0 else 64 for n in si.COUNTS) == si.REFERENCE_GROUPS
    assert si.classes_of(si.NATURAL_GROUPS) == [(16, 2), (32, 4), (64, 1)]
    assert si.classes_of(si.NATURAL_GROUPS, si.WINDOW_SECTORS) == [(16, 2), (32, 3), (64, 1)]


@pytest.mark.parametrize("model", [ca.FM_U, ca.FM_UVQ, ca.FM_UVUXUYVXVY], ids=["u", "uvq", "affine"])
def test_eval_terms_are_the_oracles_terms(oracle, model):
    interp = ca.IM_BICUBIC
    want = si.oracle_records(oracle, model, interp)
    und, dfm = si.frames()
    o = oracle.Oracle(interp=interp, model=model)
    o.set_image(0, und)
    o.set_image(1, dfm)
    for s, lvl in ((0, 0), (1, 1), (4, 2), (5, 0)):
        xy = si.lists(oracle)[s]
        lxy = xy if lvl == 0 else oracle.decimate(xy, lvl)
        inv = np.float32(1.0 / (1 << lvl))
        cx, cy = np.float32(want["und_cx"][s]) * inv, np.float32(want["und_cy"][s]) * inv
        p = si.eval_parameters(model, lvl)
        ul, dl = o.get_level(0, lvl), o.get_level(1, lvl)
        A, b, chi, err = oracle.evaluate(interp, model, ul, dl, lxy, cx, cy, p)
        terms, flagged = si.eval_terms(oracle, interp, model, ul, dl, lxy, cx, cy, p)
        assert err == 0 and not flagged
        total, bound = si.sum_bound(terms, 0)
        off = np.abs(si.pack_sums(A, b, chi) - total)
        assert (off <= bound).all() and total[42] > 0, (s, lvl, off, bound)
        # a sum of another sector is far outside the bound: the bound separates
        assert bound[42] < 1e-3 * total[42]
        # and a chain of 16 lanes has a tighter bound than the sequential one from 32 samples on
        if len(lxy) >= 64:
            assert (si.sum_bound(terms, 16)[1] <= bound).all()
    o.close()
