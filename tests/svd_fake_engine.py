"""TEST DOUBLE ONLY: tests/fake_engine.FakeEngine with the five calls of background_model = 'svd' in float64 NumPy (tests/svd_bg_oracle.py), so that the host mirror of
cnmf_e_amd.sources2d runs without a GPU."""
import warnings

import numpy as np
import scipy.sparse as sp

import svd_bg_oracle as so
from fake_engine import FakeEngine


class SvdFakeEngine(FakeEngine):
    supports_bg_svd = True
    max_iter_hit = False          # tests: pretend the iteration cap was reached

    def __init__(self):
        super().__init__()
        self.calls = []

    def ring_init(self, pid, radius, num_neighbors=None):
        self.calls.append(("ring_init", pid))
        return super().ring_init(pid, radius, num_neighbors)

    def bg_svd_set(self, pid, b, f, b0):
        q = self.p[pid]
        n = int(q["ip"].sum())
        q["svd"] = (np.array(b, dtype=np.float64).reshape(n, -1), np.array(f, dtype=np.float64).reshape(-1, q["T"]), np.array(b0, dtype=np.float64).reshape(n))
        q.pop("Ysig", None)

    def bg_svd_get(self, pid):
        return tuple(x.copy() for x in self.p[pid]["svd"])

    def bg_svd_fit(self, pid, nb, A_block=None, C_block=None):
        self.calls.append(("bg_svd_fit", pid))
        q = self.p[pid]
        A = None if A_block is None else sp.csc_matrix(A_block).astype(np.float64)
        q["svd"] = so.fit_svd_model(q["Y"].T, nb, A, None if C_block is None else np.asarray(C_block, dtype=np.float64), ind_patch=q["ip"])
        q.pop("Ysig", None)
        if self.max_iter_hit:
            warnings.warn("low-rank background of patch %d: the iteration cap was reached" % pid, RuntimeWarning, stacklevel=2)
        return self.bg_svd_stats(pid)

    def bg_svd_stats(self, pid):
        nb = self.p[pid]["svd"][0].shape[1]
        return dict(passes=0, iterations=0, converged=not self.max_iter_hit, nb=nb, residual=np.zeros(nb), s=np.zeros(nb))

    def residual_lowrank(self, pid, want=False):
        self.calls.append(("residual_lowrank", pid))
        q = self.p[pid]
        b, f, b0 = q["svd"]
        q["Ysig"] = q["Y"].T[q["ip"]] - (b @ f + b0[:, None])
        return q["Ysig"].T.astype(np.float32) if want else None

    def hals_temporal(self, pid, A_patch, C_patch, maxIter=5, want_C=True, want_raw=True, want_aa=True):
        return super().hals_temporal(pid, A_patch, C_patch, maxIter, want_C, want_raw)
