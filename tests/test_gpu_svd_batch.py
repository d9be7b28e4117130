"""Batch mode under background_model = 'svd' on the device (cnmf_e_amd/batch.py on top of cnmfe_init_temporal_lowrank): one recording of the 40 x 36 field of
tests/svd_init_temporal_cases.py cut into two batches of 96 and 80 frames, 2 x 2 patches, nb = 1.

1. initComponents_batch against the same steps written out on a second set of engines -- batch 2: set_bg_svd(b of batch 1, zeros, zeros), initTemporal,
   update_background_parallel, initComponents_residual_parallel -- bit for bit in A, C, C_raw, b, f, b0; every output is finite.
2. the remaining batch methods run (demo_batch_2p.m:112-134 without save_workspace_batch) and concatenate_temporal_batch has the right shape; once more with
   deconv_flag: C, C_raw and S are finite."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import residual_cases as rc
import svd_init_temporal_cases as sic
import svd_second_pass_cases as sp2

pytestmark = pytest.mark.gpu


def _options(deconv=False):
    from cnmf_e_amd.sources2d import Options
    return Options(ring_radius=sic.HALO, background_model="svd", nb=1, gSig=sp2.GSIG, gSiz=sp2.GSIZ, min_corr=sp2.MIN_CORR, min_pnr=sp2.MIN_PNR, maxIter=5, bd=rc.BD,
                   deconv_flag=deconv, deconv_options=dict(sic.DECONV) if deconv else {})


def _make_batches(opts):
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    Y, _, ranges = sic.batch_recording()
    d = sic.D1 * sic.D2
    out = []
    try:
        for t0, t1 in ranges:
            eng = Engine(0)
            out.append(eng)
            video = PatchedVideo(sic.D1, sic.D2, t1 - t0, sic.PDIMS, sic.HALO, eng)
            video.upload_from_full(Y[t0:t1])
            s = Sources2D(video, opts, sp.csc_matrix((d, 0), dtype=np.float32), np.zeros((0, t1 - t0), np.float32), np.zeros(d, np.float32))
            s.estimate_noise()
            out[-1] = s
    except Exception:
        for x in out:
            (x.engine if hasattr(x, "engine") else x).close()
        raise
    return out


def _close(batches):
    for s in batches:
        s.engine.close()


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _state(s):
    A = sp.csc_matrix(s.A); A.sort_indices()
    out = dict(A_ptr=A.indptr.copy(), A_idx=A.indices.copy(), A_val=A.data.copy(), C=np.array(s.C, dtype=np.float32), C_raw=np.array(s.C_raw, dtype=np.float32))
    for idx in s.video.owned:
        out["b%s" % (idx,)], out["f%s" % (idx,)], out["b0%s" % (idx,)] = s.get_b(idx), s.get_f(idx), s.get_b0(idx)
    return out


def test_init_components_batch_equals_the_hand_sequence():
    from cnmf_e_amd.batch import Sources2DBatch
    opts = _options()
    bat, hand = _make_batches(opts), _make_batches(opts)
    try:
        b = Sources2DBatch(bat, opts)
        b.initComponents_batch()
        # the same by hand: batch 1 as a single recording ...
        h1, h2 = hand
        h1.initComponents_parallel(None)
        h1.update_background_parallel()
        h1.initComponents_residual_parallel()
        K1 = h1.A.shape[1]
        assert K1 >= 1, "batch 1 found no neuron: batch 2 would have no trace to initialise"
        # ... batch 2: the parent's A, batch 1's b with zeros of batch 2's shapes, initTemporal, the fit, the second pass
        h2._set_A(h1.A); h2.ids = np.array(h1.ids); h2.tags = np.array(h1.tags); h2.P["k_ids"] = int(h1.P["k_ids"])
        for idx in h2.video.owned:
            bp = h1.get_b(idx)
            assert bp.shape == (h2.video.patch_pix[idx].size, 1)
            h2.set_bg_svd(idx, bp, np.zeros((1, h2.video.T)), np.zeros(bp.shape[0]))
        h2.initTemporal()
        h2.update_background_parallel()
        h2.initComponents_residual_parallel()
        if h1.A.shape[1] != h2.A.shape[1]:                    # the second loop of initComponents_batch.m:86-113
            h1._set_A(h2.A); h1.ids = np.array(h2.ids); h1.tags = np.array(h2.tags); h1.P["k_ids"] = int(h2.P["k_ids"])
            h1._grow_K(h2.A.shape[1])
            h1.update_temporal_parallel()
        print("svd batch: K after batch 1 %d, after batch 2 %d" % (K1, h2.A.shape[1]))
        assert b.A.shape[1] == h2.A.shape[1] and [s.A.shape[1] for s in bat] == [b.A.shape[1]] * 2
        for m, (s, h) in enumerate(zip(bat, hand)):
            got, want = _state(s), _state(h)
            for k in want:
                assert np.isfinite(got[k]).all(), (m, k)
                assert _same_bits(got[k], want[k]), (m, k)
        # batch 2's f and b0 are its own fit's, not the zeros it was handed
        assert any(bat[1].get_f(idx).any() for idx in bat[1].video.owned)
    finally:
        _close(bat); _close(hand)


@pytest.mark.parametrize("deconv", [False, True])
def test_demo_sequence_runs(deconv):
    """demo_batch_2p.m:112-134: initComponents_batch, then update_background_batch / update_spatial_batch / update_temporal_batch, correlation_pnr_batch and
    concatenate_temporal_batch: everything finite, the concatenated traces K x (96 + 80)"""
    from cnmf_e_amd.batch import Sources2DBatch
    opts = _options(deconv)
    bat = _make_batches(opts)
    try:
        b = Sources2DBatch(bat, opts)
        b.initComponents_batch()
        K = b.A.shape[1]
        assert K >= 1
        b.update_background_batch()
        b.update_spatial_batch()
        b.update_temporal_batch()
        pairs = b.correlation_pnr_batch()
        assert len(pairs) == 2 and all(np.isfinite(Cn).all() and np.isfinite(PNR).all() for Cn, PNR in pairs)
        b.concatenate_temporal_batch()
        K = b.A.shape[1]
        assert b.C.shape == b.C_raw.shape == (K, 176) and b.C.dtype == np.float32 and (b.S is not None) == deconv
        assert np.isfinite(b.C).all() and np.isfinite(b.C_raw).all() and (not deconv or (b.S.shape == (K, 176) and np.isfinite(b.S).all()))
        assert np.isfinite(b.A.toarray()).all() and b.C.any()
        for s in bat:
            for idx in s.video.owned:
                assert all(np.isfinite(x).all() for x in (s.get_b(idx), s.get_f(idx), s.get_b0(idx)))
    finally:
        _close(bat)
