"""demixed_frames / show_demixed_video under background_model = 'svd' on the device (cnmfe_demix_frames_lowrank; csrc/demix.hpp, k_demix_panels_lowrank) on the
recordings of tests/svd_bg_cases.py after two iterations: `one` (T mod 4 = 3, d no multiple of 256) with nb = 1 and 3, `quad` (2 x 2 patches) with nb = 2.
demixed_frames(kt=3, frame_range=(2, T), chunk=7): a stride, a last displayed frame in the T mod 4 tail (`one`: frame 203), several chunks.

    bg         |bg - (b0 + b f)| <= 2^-23 (|b0| + sum_i |b_i f_i|) elementwise against the float64 factors of get_b / get_f / get_b0 (one rounding of an fp64 chain);
               against s.reconstruct_background(): rel <= 2.4e-7, BOUND_BG_F32 of tests/test_gpu_svd_bg.py
    raw, denoised, mixed   the assertions of tests/test_gpu_demix.py: raw within 2^-22 max|Y| of the recording (Yc + Ymean: two fp32 roundings); denoised within 6e-7
               of the float64 A CC relative to its maximum; mixed equal wherever the float64 value is farther than 0.05 from a rounding boundary, within one count
               elsewhere.  That file's second bound on raw, 0, is 10 x what its own recording showed (every sample within a factor 2 of its pixel mean, where
               fl(fl(Y - m) + m) = Y); these recordings span -80 .. 480 around a mean of 200 and IEEE arithmetic itself does not give them back -- the host's own
               (Y - m) + m in fp32 differs from Y too -- so that bound is not taken over, the derived one is
    signal     == raw - bg in fp32
    residual   == fl32((double)raw - (double)bg - acc), EQUAL: acc is formed on the host by scipy's CSR product -- a plain loop over the row's stored entries in
               ascending column order, no BLAS -- and every product of two fp32 values is exact in fp64, so the loop's multiply-add has the kernel's fma's bits
    chunks of 7 equal one call of all frames, bit for bit; the call leaves the residual state alone; show_demixed_video(path=None) returns the ranges.

Observed on the MI355X, one nb 1 / one nb 3 / quad nb 2: bg error over its bound 0.497 / 0.495 / 0.499 (one rounding is half the bound); bg against
reconstruct_background 0 / 0 / 0 (the host forms the same float64 value and rounds it once); raw 1.8e-8 / 1.8e-8 / 1.7e-8 of max|Y|; denoised 5.6e-8 / 3.3e-8 / 3.1e-8;
mixed: no sample differs (99.2 % / 99.2 % / 99.6 % of them lie farther than 0.05 from a rounding boundary); signal, residual and denoised equal the host's bits."""
import numpy as np
import pytest
import scipy.sparse as sp

import demix_cases as dc
import demix_oracle as do
import svd_bg_cases as sc
from parity_util import rel

pytestmark = pytest.mark.gpu

BOUND_BG_F32 = 2.4e-7              # tests/test_gpu_svd_bg.py
BOUND_DENOISED = 6e-7              # tests/test_gpu_demix.py BOUNDS["denoised"]
KT, CHUNK = 3, 7
PANELS = ("raw", "bg", "signal", "denoised", "residual")
CASES = [("one", 1), ("one", 3), ("quad", 2)]
_states = {}


class _State:
    """a recording after two iterations on an engine of its own, and its panels: in chunks of 7 and in one call"""

    def __init__(self, name, nb):
        from cnmf_e_amd.engine import Engine
        from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
        self.case = case = sc.make_case(name, nb)
        self.eng = Engine(0)
        self.video = PatchedVideo(case["d1"], case["d2"], case["T"], case["patch"], case["halo"], self.eng)
        self.video.upload_from_full(case["Y"])
        self.s = Sources2D(self.video, Options(ring_radius=case["halo"], background_model="svd", nb=nb, maxIter=5), case["A"], case["C"],
                           np.ones(case["d1"] * case["d2"], np.float32))
        for _ in range(2):
            self.s.update_background_parallel(); self.s.update_spatial_parallel(); self.s.update_temporal_parallel()
        self.col = dc.colors(self.s.A.shape[1])
        self.kw = dict(kt=KT, frame_range=(2, case["T"]), amp_ac=dc.AMP_AC, colors=self.col)
        self.frames = np.arange(1, case["T"], KT)                            # 0-based
        self.parts = list(self.s.demixed_frames(chunk=CHUNK, **self.kw))
        self.whole = list(self.s.demixed_frames(chunk=1000, **self.kw))

    def flat(self, ch, name):
        a = ch[name]
        return a.reshape((self.case["d1"] * self.case["d2"],) + a.shape[2:], order="F")


def _state(name, nb):
    if (name, nb) not in _states:
        _states[(name, nb)] = _State(name, nb)
    return _states[(name, nb)]


@pytest.fixture(scope="module")
def states():
    """the states by (name, nb), each built once and shared; their engines are closed behind the module's last test"""
    yield _state
    for st in _states.values():
        st.eng.close()
    _states.clear()


@pytest.mark.parametrize("name,nb", CASES)
def test_panels(states, name, nb, observed):
    st = states(name, nb)
    s, case, v = st.s, st.case, st.video
    T, fr = case["T"], st.frames
    assert len(st.whole) == 1 and len(st.parts) == -(-fr.size // CHUNK) > 1
    ch = st.whole[0]
    assert np.array_equal(ch["frames"], fr + 1) and (name != "one" or (fr[-1] == T - 1 and T % 4 == 3))      # the last displayed frame lies in the tail quad
    for nm in PANELS + ("mixed",):                                          # chunking changes no bit
        assert np.array_equal(ch[nm], np.concatenate([c[nm] for c in st.parts], axis=2)), nm
    P = {nm: st.flat(ch, nm) for nm in PANELS}
    assert all(P[nm].dtype == np.float32 for nm in PANELS)
    # bg against the float64 factors, one rounding
    worst = 0.0
    for idx in v.owned:
        pp = v.patch_pix[idx]
        b, f, b0 = s.get_b(idx), s.get_f(idx), np.asarray(s.get_b0(idx), dtype=np.float64)
        assert b.shape == (pp.size, nb) and f.shape == (nb, T)
        exact = b0[:, None] + b @ f[:, fr]
        bound = 2.0 ** -23 * (np.abs(b0)[:, None] + np.abs(b) @ np.abs(f[:, fr]))
        err = np.abs(P["bg"][pp].astype(np.float64) - exact)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (idx, float((err / bound).max()))
    e_bg = rel(ch["bg"], s.reconstruct_background()[:, :, fr])
    # raw, denoised, mixed: the assertions of tests/test_gpu_demix.py
    Y = case["Y"].T[:, fr]
    e_raw = float(np.abs(P["raw"] - Y).max() / np.abs(Y).max())
    A = sp.csr_matrix(s.A).astype(np.float64); A.sort_indices()
    CC = np.asarray(s.C, dtype=np.float64)[:, fr]
    acc = np.asarray(A @ CC)                                                # the CSR loop: entries of a row in ascending column order, exact products
    e_den = float(np.abs(P["denoised"] - acc).max() / np.abs(acc).max())
    md = do.mixed_double(s.A, CC, st.col, dc.AMP_AC)
    want = do.matlab_uint16(md).astype(np.int64)
    got = st.flat(ch, "mixed").astype(np.int64)
    far = do.rounding_distance(md) > dc.MIXED_MARGIN
    ndiff = int((got != want).sum())
    print("svd panels %s nb %d: bg error / bound %.3f, bg against reconstruct_background %.2e, raw %.2e, denoised %.2e, mixed differ %d of %d (far %.4f)"
          % (name, nb, worst, e_bg, e_raw, e_den, ndiff, got.size, far.mean()))
    observed["svd_demix_%s_nb%d" % (name, nb)] = dict(bg_over_bound=worst, bg_reconstruct=e_bg, raw=e_raw, denoised=e_den, mixed_differ=ndiff, far=float(far.mean()))
    assert e_bg <= BOUND_BG_F32, e_bg
    assert np.abs(P["raw"] - Y).max() <= 2.0 ** -22 * np.abs(Y).max()       # Yc + Ymean: two fp32 roundings of the video (test_exact_relations of tests/test_gpu_demix.py)    assert e_den <= BOUND_DENOISED and np.abs(P["denoised"] - acc.astype(np.float32)).max() <= 2.0 ** -22 * np.abs(acc).max()
    assert got.shape == want.shape and st.flat(ch, "mixed").dtype == np.uint16
    assert far.mean() > 0.98 and want.max() > 0
    assert np.array_equal(got[far], want[far])
    assert np.abs(got - want).max() <= 1
    # signal and residual: exact relations on the returned panels
    assert np.array_equal(P["signal"], P["raw"] - P["bg"])
    assert np.array_equal(P["residual"], (P["raw"].astype(np.float64) - P["bg"].astype(np.float64) - acc).astype(np.float32))
    assert np.array_equal(P["denoised"], acc.astype(np.float32))


def test_the_call_leaves_the_residual_state_alone(states):
    """per patch: a temporal update on the resident low-rank residual, the panels, the same update again WITHOUT a new request -- still valid, equal bits; and a
    patch that has no resident residual has none afterwards"""
    from cnmf_e_amd._lib import CnmfeError
    st = states("quad", 2)
    s, eng, v = st.s, st.eng, st.video
    CC = np.ascontiguousarray(np.asarray(s.C), dtype=np.float32)
    done = 0
    for idx in v.owned:
        pid = v.pid[idx]
        ind, A_pp = s._slice(s.A, idx, "patch")
        if not ind.size:
            continue
        eng.residual_lowrank(pid)
        before = eng.hals_temporal(pid, A_pp, CC[ind], 2)[1]
        full = eng.demix_frames_lowrank(pid, A_pp, CC, ind, st.col[ind], 1000.0, 1, KT, 5)
        assert np.array_equal(before, eng.hals_temporal(pid, A_pp, CC[ind], 2)[1])
        eng.bg_svd_set(pid, *eng.bg_svd_get(pid))                            # (a set drops the residual)
        again = eng.demix_frames_lowrank(pid, A_pp, CC, ind, st.col[ind], 1000.0, 1, KT, 5)
        for nm in PANELS + ("mixed",):
            assert np.array_equal(full[nm], again[nm]), nm
        with pytest.raises(CnmfeError, match="error -4"):
            eng.hals_temporal(pid, A_pp, CC[ind], 2)
        none = eng.demix_frames_lowrank(pid, None, CC, np.zeros(0, np.int32), np.zeros((0, 3), np.float32), 1000.0, 1, KT, 5)
        assert not none["denoised"].any() and not none["mixed"].any() and np.array_equal(none["bg"], full["bg"]) and np.array_equal(none["residual"], none["signal"])
        with pytest.raises(CnmfeError, match="error -1"):
            eng.demix_frames_lowrank(pid, A_pp, CC, ind, st.col[ind], 1000.0, st.case["T"] - 2, KT, 2)      # a frame >= T
        done += 1
    assert done == 2
    eng.create_patch(900, [1, 2, 1, 2], [1, 2, 1, 2], 2, 2, 16)
    with pytest.raises(CnmfeError, match="error -4"):                        # no background on that patch
        eng.demix_frames_lowrank(900, None, CC, np.zeros(0, np.int32), np.zeros((0, 3), np.float32), 1000.0, 0, 1, 1)


def test_show_demixed_video_returns_the_ranges(states):
    st = states("one", 1)
    r = st.s.show_demixed_video(path=None, kt=KT, frame_range=(2, st.case["T"]))
    assert {"range_ac", "range_res", "range_Y", "multi_factor", "amp_ac"} <= set(r) and np.isfinite(r["amp_ac"]) and r["amp_ac"] > 0
