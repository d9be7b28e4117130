"""cnmfe_mex('seed_images', h, pid, psf, nframes, Q) through the mock MEX runtime (tests/mex_stub, the harness of tests/test_gpu_mex_gateway.py): the command
the twin @Sources2D/correlation_pnr_parallel.m issues per patch, merged as the twin merges it, must give the images of the Python host's
correlation_pnr_parallel on the same library -- EQUAL arrays: the gateway only marshals (double psf -> float, column-major Q, nr_b x nc_b double outputs)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


class _Geometry:
    def create_patch(self, *a):
        pass


@pytest.mark.parametrize("nk", [1, 3], ids=["plain", "detrend"])
def test_the_gateway_command_gives_the_python_hosts_images(nk):
    from test_gpu_mex_gateway import Mex
    from test_gpu_seed_images import CASES, _input
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options, seed_psf, bspline_basis
    c = CASES["A"]
    f, Y = _input("A")
    d1, d2 = c["dims"]
    T, r = c["T"], c["r"]
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, c["pdims"], r, eng)
        video.upload_from_full(Y)
        s = Sources2D(video, Options(ring_radius=r, gSig=c["gSig"], gSiz=c["gSiz"], nk=nk), f.A_init, f.C_init, f.sn)
        Cn_ref, PNR_ref = s.correlation_pnr_parallel()
    finally:
        eng.close()
    geo = PatchedVideo(d1, d2, T, c["pdims"], r, _Geometry())
    psf = seed_psf(c["gSig"], c["gSiz"], True)
    Q = np.linalg.qr(bspline_basis(T, nk))[0] if nk > 1 else np.zeros((0, 0))
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        Cn = np.zeros((d1, d2)); PNR = np.zeros((d1, d2))
        for i, idx in enumerate(geo.order):
            pid = float(i + 1)
            p, b = geo.patch_pos[idx], geo.block_pos[idx]
            mex("patch", h, pid, p.astype(np.float64), b.astype(np.float64), d1, d2, T)
            mex("upload", h, pid, np.ascontiguousarray(Y[:, geo.block_pix[idx]].T), 0)
            cn_b, pnr_b = mex("seed_images", h, pid, psf, T, Q, nout=2)
            assert cn_b.shape == (b[1] - b[0] + 1, b[3] - b[2] + 1) and cn_b.dtype == np.float64 and pnr_b.shape == cn_b.shape
            rr = slice(p[0] - b[0], p[1] - b[0] + 1); cc = slice(p[2] - b[2], p[3] - b[2] + 1)
            Cn[p[0] - 1:p[1], p[2] - 1:p[3]] = cn_b[rr, cc]
            PNR[p[0] - 1:p[1], p[2] - 1:p[3]] = pnr_b[rr, cc]
        assert np.array_equal(Cn, Cn_ref) and np.array_equal(PNR, PNR_ref)
        with pytest.raises(RuntimeError, match="odd-sized"):
            mex("seed_images", h, 1.0, np.ones((4, 4)), T, np.zeros((0, 0)), nout=2)
        with pytest.raises(RuntimeError, match="not created through this gateway"):
            mex("seed_images", h, 99.0, psf, T, nout=2)
    finally:
        mex("destroy", h)
