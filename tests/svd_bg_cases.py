"""Small recordings for background_model = 'svd': `nb` planted background components (smooth maps x slow time courses, strengths a factor 3 apart) over a few
neurons, white noise and a baseline.  The shapes are the kernels' edges (tests/test_gpu_svd_bg.py):
    one    40 x 36, T = 203, one patch     d_b = 1440 > T, T mod 4 = 3, d_b no multiple of 256, rows no multiple of 16
    small  12 x 10, T = 301, one patch     d_b = 120 < T
    quad   48 x 48, T = 256, 2 x 2 patches with a halo of 5: the patch is a strict interior of its block, one neuron straddles the border of two patches, and the two
           right-hand blocks hold no neuron (the reference's A = ones, C = zeros branch on the first run, the skip rule on later runs)
Every case is deterministic (numpy.random.default_rng).  The CPU tests assert for every block that the planted spectrum makes the reference's answer well-posed and
bounds the iteration's rate: sigma_nb / sigma_(nb+1) >= 3 and sigma_17 / sigma_nb <= 0.5 (well_posed)."""
import numpy as np
import scipy.sparse as sp

from cnmf_e_amd import synth

SHAPES = {
    "one": dict(d1=40, d2=36, T=203, patch=[40, 36], halo=5, centres=[(9.3, 8.1), (20.6, 17.2), (30.2, 9.7), (12.4, 27.5), (29.1, 26.3)]),
    "small": dict(d1=12, d2=10, T=301, patch=[12, 10], halo=3, centres=[(4.2, 4.1), (7.6, 5.8)]),
    "quad": dict(d1=48, d2=48, T=256, patch=[24, 24], halo=5, centres=[(8.4, 7.3), (24.4, 9.2), (38.7, 8.6), (14.2, 12.1)]),
}
NOISE = 0.5
BASE = 200.0


# (shape, with neurons): without any, every block takes the reference's A = ones, C = zeros branch (K = 0); quad has such blocks beside blocks with neurons
CASES = [("one", True), ("one", False), ("small", True), ("small", False), ("quad", True)]


def make_case(name, nb, neurons=True, seed=0):
    """-> dict: d1, d2, T, patch, halo, Y (T, d) float32, A (d x K csc float32), C (K x T float32), nb"""
    s = SHAPES[name]
    d1, d2, T = s["d1"], s["d2"], s["T"]
    rng = np.random.default_rng(1000 * (1 + list(SHAPES).index(name)) + 10 * nb + seed)
    K = len(s["centres"])
    A = synth._footprints(d1, d2, np.asarray(s["centres"]), rng.uniform(0.8, 1.2, K), 1.5, 7)
    spikes = (rng.random((K, T)) < 0.02) * rng.uniform(5.0, 12.0, (K, T))
    C = synth._ar1(spikes, 0.9)
    rr, cc = np.meshgrid((np.arange(d1) + 0.5) / d1, (np.arange(d2) + 0.5) / d2, indexing="ij")
    Y = np.zeros((T, d1 * d2))
    for i in range(max(nb, 1)):
        # smooth, mutually near-orthogonal maps; slow time courses of unit variance
        m = np.cos(np.pi * (i + 1) * rr) * np.cos(np.pi * ((i + 1) // 2) * cc) + 0.3 * np.sin(np.pi * (i + 2) * cc)
        m = m / np.sqrt(np.mean(m * m))
        g = synth._ar1(rng.normal(0.0, 1.0, T), 0.97); g = (g - g.mean()) / g.std()
        Y += (60.0 / 3.0 ** i) * np.outer(g, m.reshape(-1, order="F"))
    if neurons:
        Y += C.T @ A.T.toarray()
    else:
        A, C = A[:, :0], C[:0]
    Y += BASE + rng.normal(0.0, NOISE, Y.shape)
    return dict(name=name, d1=d1, d2=d2, T=T, patch=s["patch"], halo=s["halo"], nb=nb, Y=np.ascontiguousarray(Y, dtype=np.float32),
                A=sp.csc_matrix(A, dtype=np.float32), C=np.ascontiguousarray(C, dtype=np.float32))


def block_inputs(case, block_pix):
    """(Y_block (d_b, T) float64, ind, A_block (d_b x len(ind) csc), C_block) of one block: the neurons that touch it"""
    A = case["A"].tocsr()[block_pix].tocsc()
    ind = np.nonzero(np.asarray(A.sum(axis=0)).ravel() > 0)[0]
    return case["Y"][:, block_pix].T.astype(np.float64), ind, A[:, ind], case["C"][ind]


def well_posed(sv, nb):
    """the two ratios the tests assert: (sigma_nb / sigma_(nb+1), sigma_17 / sigma_nb)"""
    return sv[nb - 1] / sv[nb], sv[16] / sv[nb - 1]
