"""The fixtures of the second pass under background_model = 'svd' (tests/svd_second_pass_cases.py), checked on the CPU with the float64 oracles alone:
svd_bg_oracle's fit, then greedy_oracle.greedy_block on the float64 Yres = Y - A0 C0 - (b f + b0) of every patch.  Every withheld neuron must be found and every
decision margin of the run must reach the bounds of tests/greedy_cases.py -- otherwise a comparison of discrete decisions on the device would test rounding, not
the code.  Also here: the refusals that stay for an engine that declares neither supports_bg_svd_init_residual nor supports_bg_svd_demix."""
import numpy as np
import pytest

import residual_cases as rc
import svd_second_pass_cases as sp2


@pytest.mark.parametrize("name", list(sp2.CASES))
def test_fixture_margins_and_withheld_neurons(name):
    ora = sp2.oracle(name)
    print("margins %s: %s" % (name, {k: "%.2e" % v for k, v in sorted(ora["margins"].items())}))
    assert not rc.margins_clear(ora["margins"]), rc.margins_clear(ora["margins"])
    want, got = sp2.true_centres(name), ora["center"]
    assert got.shape[0] == want.shape[0] >= 1, (got, want)
    for w in want:                                                         # every withheld neuron within a pixel and a half of an accepted centre
        assert np.min(np.hypot(*(got - w).T)) <= 1.5, (w, got)
    assert ora["A"].shape[1] == got.shape[0] and np.all(ora["A"].max(axis=0) > 0)


def test_yres_before_any_fit_is_y_minus_ac():
    """b = f = b0 = 0 (what the constructor sets): the reference's expression is Y - A C"""
    o = sp2.oracle_loop("small")
    idx = (0, 0)
    d = o._data(o.patch_pos[idx]).shape[0]
    got = sp2.yres(o, idx, np.zeros((d, 1)), np.zeros((1, o.T)), np.zeros(d))
    assert np.array_equal(got, o._data(o.patch_pos[idx]) - o.A.toarray() @ o.C)


def test_engine_flags_are_listed_and_an_engine_without_them_is_refused():
    import svd_bg_cases as sc
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import Sources2D
    assert Engine.supports_bg_svd_init_residual is True and Engine.supports_bg_svd_demix is True

    class NoFlags:
        supports_bg_svd = True

    s = Sources2D.__new__(Sources2D)
    s.engine, s.bg_model, s.video = NoFlags(), "svd", object()
    for call in (s.initComponents_residual_parallel, s.show_demixed_video, lambda: next(s.demixed_frames())):
        with pytest.raises(NotImplementedError, match="svd"):
            call()
    assert sc.SHAPES["one"]["T"] % 4 == 3                                   # the tail the GPU tests rely on
