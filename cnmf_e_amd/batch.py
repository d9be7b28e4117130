"""Batch mode: the reference's ``obj.batches`` workflow (demos/demo_batch_1p.m:120-142) on several resident recordings.

Several recordings of one field of view -- the sessions of an animal, or one long recording cut into temporal batches -- share ONE set of footprints ``A``;
every batch has its own traces and its own background.  ``Sources2DBatch`` is the parent object: it holds the batches (one ``Sources2D`` each, on its own
``PatchedVideo`` and its own ``Engine`` context, all alive at once on one device) and restates

    initComponents_batch(K, save_avi)       @Sources2D/initComponents_batch.m:36-113
    update_spatial_batch()                  @Sources2D/update_spatial_batch.m:11-45
    update_temporal_batch()                 @Sources2D/update_temporal_batch.m:19-33
    update_background_batch()               @Sources2D/update_background_batch.m:13-24
    correlation_pnr_batch()                 @Sources2D/Sources2D.m:1901-1912
    concatenate_temporal_batch()            @Sources2D/Sources2D.m:708-738

in terms of the single-recording methods, which are taken as they are.  What a batch call adds on the device is small on purpose (cnmfe.h, "Batch mode"): the
weights of the footprint average are taken where the traces lie (cnmfe_trace_energy), and a batch whose K grows gets its zero rows there (cnmfe_traces_grow).

Not built: getReady_batch's file handling (the caller uploads every batch; ``from_full`` cuts one recording), save_workspace_batch, ``shifts``, batches sharded
over ranks, MATLAB twins of these methods.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .sources2d import Options, PatchedVideo, Sources2D, _mround      # (_mround: MATLAB's round, halves away from zero; Python's round goes to even)

__all__ = ["Sources2DBatch", "batch_frame_ranges"]


def batch_frame_ranges(T, batch_frames=None):
    """The frame ranges getReady_batch cuts a recording of T frames into (Sources2D.m:298-318), 1-based and inclusive, as a list of (first, last):
    nbatches = round(T / batch_frames) with MATLAB's rounding; at most one batch gives [1, T]; else the edges are round(linspace(1, T, nbatches + 1)) and every
    range but the last ends one frame before the next begins.  batch_frames = None (the reference's []): one batch."""
    T = int(T)
    if T < 1:
        raise ValueError("batch_frame_ranges: T = %d" % T)
    if batch_frames is None:
        batch_frames = T                                                  # :299-301
    if not batch_frames > 0:
        raise ValueError("batch_frame_ranges: batch_frames = %r" % (batch_frames,))
    nb = int(_mround(T / float(batch_frames)))                            # :302
    if nb <= 1:
        return [(1, T)]                                                   # :303-304
    edges = _mround(np.linspace(1.0, float(T), nb + 1)).astype(np.int64)  # :306
    return [(int(edges[n]), int(edges[n + 1]) - (1 if n != nb - 1 else 0)) for n in range(nb)]      # :313


class Sources2DBatch:
    """The parent object of batch mode: ``batches`` (a list of Sources2D), ``options`` (ONE Options object, shared by every batch as initComponents_batch.m:40,92
    assigns it), ``A``, ``ids``, ``tags``, ``P["k_ids"]``, ``P["numFrames"]``, ``file_id``; after concatenate_temporal_batch ``C``, ``C_raw`` and, under deconv_flag,
    ``S``.  Every batch is resident: nothing is swapped out, and every context reserves the buffers of a background fit ("Temporal batches").
    ``use_parallel`` is accepted and ignored, as by the single-recording methods.
    Side effects of the constructor on what the caller hands in: every batch's ``options`` attribute is REPLACED by the shared object (the reference's assignment), and
    ``options.d1`` / ``options.d2`` are filled in from the batches when they are unset (0); set to anything else than the batches' size they are refused (ValueError)."""

    def __init__(self, batches, options: Options, file_id=None):
        batches = list(batches)
        if not batches:
            raise ValueError("Sources2DBatch needs at least one batch")
        v0 = batches[0].video
        self.svd = str(options.background_model).lower() == "svd" or any(getattr(s, "bg_model", "ring") == "svd" for s in batches)
        if self.svd:
            if any(getattr(s, "bg_model", "ring") != "svd" for s in batches) or str(options.background_model).lower() != "svd":
                raise ValueError("background_model = 'svd' must be the model of the shared options and of every batch")
            if not all(getattr(s.engine, "supports_bg_svd_init_temporal", False) for s in batches):
                raise NotImplementedError("Sources2DBatch under background_model = 'svd' needs engines with init_temporal_lowrank (supports_bg_svd_init_temporal)")
        for m, s in enumerate(batches):
            v = s.video
            if getattr(s, "dist", None) is not None:
                raise ValueError("batch %d carries a dist_group: sharded batches are not built" % (m + 1))
            if (v.d1, v.d2) != (v0.d1, v0.d2):
                raise ValueError("batch %d is %d x %d pixels, batch 1 is %d x %d" % (m + 1, v.d1, v.d2, v0.d1, v0.d2))
            if v.order != v0.order or any(tuple(v.patch_pos[i]) != tuple(v0.patch_pos[i]) or tuple(v.block_pos[i]) != tuple(v0.block_pos[i]) for i in v0.order):
                raise ValueError("batch %d is cut into other patches than batch 1 (patch_dims / ring_radius)" % (m + 1))
            if int(s.options.ring_radius) != int(options.ring_radius) or int(v.w_overlap) != int(v0.w_overlap) or int(s.options.bg_ssub) != int(options.bg_ssub):
                raise ValueError("batch %d was made with ring_radius %s / bg_ssub %s, the shared options have %s / %s"
                                 % (m + 1, s.options.ring_radius, s.options.bg_ssub, options.ring_radius, options.bg_ssub))
            if v.T < 64:
                raise ValueError("batch %d has %d frames: at least 64 are needed" % (m + 1, v.T))
            if any(s.engine is t.engine for t in batches[:m]):
                raise ValueError("batch %d shares its engine with an earlier batch: every batch has its own context" % (m + 1))
        self.batches = batches
        self.options = options
        for s in batches:
            s.options = options
        d = v0.d1 * v0.d2
        if (int(options.d1), int(options.d2)) == (0, 0):                   # (unset: filled in, as Sources2D's constructor fills its own options in)
            options.d1, options.d2 = v0.d1, v0.d2
        elif (int(options.d1), int(options.d2)) != (v0.d1, v0.d2):
            raise ValueError("the shared options say %d x %d pixels, the batches have %d x %d" % (options.d1, options.d2, v0.d1, v0.d2))
        self.A = sp.csc_matrix((d, 0), dtype=np.float32)
        self.ids = np.zeros(0, dtype=np.int64)
        self.tags = np.zeros(0, dtype=np.uint16)
        self.P = {"k_ids": 0, "numFrames": np.array([s.video.T for s in batches], dtype=np.int64)}      # Sources2D.m:318,324
        self.file_id = np.ones(len(batches), dtype=np.uint8) if file_id is None else np.asarray(file_id, dtype=np.uint8)      # :316,323
        if self.file_id.size != len(batches):
            raise ValueError("file_id has %d entries for %d batches" % (self.file_id.size, len(batches)))
        self.C = self.C_raw = self.S = None

    @classmethod
    def from_full(cls, Y_td, batch_frames, patch_dims, options: Options, device=0):
        """One recording Y_td ((T, d1*d2), frame-major, options.d1 x options.d2 pixels) cut by batch_frame_ranges(T, batch_frames): one engine, one video and one
        Sources2D per batch, each with A = d x 0 and sn from its own estimate_noise (Sources2D.m:292-318 without the files)."""
        from .engine import Engine
        T, d = Y_td.shape
        d1, d2 = int(options.d1), int(options.d2)
        if d1 * d2 != d:
            raise ValueError("Y_td has %d pixels per frame, options.d1 x options.d2 = %d x %d" % (d, d1, d2))
        batches = []
        for f0, f1 in batch_frame_ranges(T, batch_frames):
            n = f1 - f0 + 1
            if n < 64:
                raise ValueError("frames [%d, %d]: a batch needs at least 64 frames" % (f0, f1))
            eng = Engine(device)
            video = PatchedVideo(d1, d2, n, patch_dims, options.ring_radius, eng)
            video.upload_from_full(Y_td[f0 - 1:f1])
            s = Sources2D(video, options, sp.csc_matrix((d, 0), dtype=np.float32), np.zeros((0, n), dtype=np.float32), np.zeros(d, dtype=np.float32))
            s.estimate_noise()
            batches.append(s)
        return cls(batches, options)

    def close(self):
        """close every batch's engine (last one first)"""
        for s in reversed(self.batches):
            s.engine.close()

    # -- what travels between the parent and a batch ------------------------------------------------------------------------------------------------------
    def _hand_down(self, s):
        """neuron_k.A = obj.A; neuron_k.P.k_ids = obj.P.k_ids; neuron_k.ids = obj.ids; neuron_k.tags = obj.tags (initComponents_batch.m:53-58,97-100)"""
        s._set_A(self.A)
        s.P["k_ids"] = int(self.P["k_ids"])
        s.ids = np.array(self.ids, copy=True); s.tags = np.array(self.tags, copy=True)

    def _collect(self, s):
        """obj.A = neuron_k.A; obj.ids, obj.tags, obj.P.k_ids likewise (:75-83; W, b, f, b0 stay with the batch: see initComponents_batch)"""
        self.A = s.A
        self.ids = np.array(s.ids, copy=True); self.tags = np.array(s.tags, copy=True)
        self.P["k_ids"] = int(s.P["k_ids"])

    @staticmethod
    def _same_W(W0, W1):
        W0, W1 = sp.csr_matrix(W0), sp.csr_matrix(W1)
        return (W0.shape == W1.shape and np.array_equal(W0.indptr, W1.indptr) and np.array_equal(W0.indices, W1.indices)
                and np.array_equal(np.asarray(W0.data, dtype=np.float32).view(np.uint32), np.asarray(W1.data, dtype=np.float32).view(np.uint32)))

    # -- the methods ----------------------------------------------------------------------------------------------------------------------------------------
    def initComponents_batch(self, K=None, save_avi=False, use_parallel=True):
        """obj.initComponents_batch(K, save_avi, use_parallel)  (@Sources2D/initComponents_batch.m:36-113).  Batch 1 runs initComponents_parallel(K); every later
        batch receives the parent's A, ids, tags and P.k_ids and runs initTemporal(); every batch then runs update_background_parallel() and
        initComponents_residual_parallel(), and the parent collects its A, ids, tags, P.k_ids (:75-83).  Second loop (:86-113): every batch whose K is below the
        final one receives the parent's A, ids, tags, its C grows by zero rows (:103-106, on the device: Sources2D._grow_K) and it runs update_temporal_parallel().
        The reference hands W_init, b0_init of batch 1 to the later batches (:47-50,60-63): what initComponents_parallel left BEFORE any fit, the uniform ring mean
        and zeros (initComponents_parallel.m:213-236) -- exactly what a fresh Sources2D of the same geometry holds.  That equality is asserted once per batch (get_W,
        bit for bit) and nothing is transplanted: set_W would mark the ring as fitted, and the first-run test of update_background_parallel.m:143 must still say
        "first run".  save_avi is not built.
        background_model = 'svd': there is no W and nothing is asserted.  Every batch after the first receives, per owned patch,
        set_bg_svd(idx, b_prev, zeros((nb, T_k)), zeros(d_patch)) with b_prev = get_b(idx) of the batch BEFORE it, taken after that batch's
        update_background_parallel and second pass; its initTemporal then fits the footprints and b_prev jointly and replaces f and b0.  This is a deviation:
        initComponents_batch.m:55-56 assigns exactly that b (neuron_k.b = obj.b), but :61 overwrites it with b_init, the zeros(nr*nc, nb) of
        initComponents_parallel.m:272, which makes tmp_A'*tmp_A of initTemporal.m:182 singular for every nb >= 1 -- the reference's own demo yields non-finite
        traces from its second batch on.  Everything else is literal, with its consequences: update_background_parallel's first-run test sees a non-zero b{1}
        in the later batches, so a patch without neurons keeps f = 0, b0 = 0 there until it has one."""
        if save_avi:
            raise NotImplementedError("initComponents_batch: save_avi is not built")
        W_init = b_prev = None
        for m, s in enumerate(self.batches):
            s.options = self.options                                       # :40
            if m == 0:
                s.initComponents_parallel(K)                               # :45 (the batch's recording is its frame range)
                if not self.svd:
                    W_init = {idx: s.get_W(idx) for idx in s.video.owned}  # :47-50: before its first fit
            else:
                self._hand_down(s)                                         # :53-58
                for idx in s.video.owned:
                    if self.svd:                                           # :55-56 (and NOT :61, see above)
                        b = np.asarray(b_prev[idx], dtype=np.float64)
                        s.set_bg_svd(idx, b, np.zeros((b.shape[1], s.video.T)), np.zeros(b.shape[0]))
                    elif not self._same_W(W_init[idx], s.get_W(idx)):      # :60-63, as an assertion
                        raise RuntimeError("batch %d: W{%s} is not the unfitted ring of batch 1 (a batch must come fresh to initComponents_batch)" % (m + 1, idx))
                if self.A.shape[1]:                                        # (no neuron so far: no trace to initialise, the residual pass below may find the first)
                    s.initTemporal()                                       # :65
            s.update_background_parallel()                                 # :68
            s.initComponents_residual_parallel()                           # :71
            if self.svd:
                b_prev = {idx: s.get_b(idx) for idx in s.video.owned}      # obj.b of :75-83: what the next batch starts from
            self._collect(s)                                               # :75-83
        K_all = self.A.shape[1]                                            # :87
        for s in self.batches:
            s.options = self.options                                       # :92
            # :94-96 `break`s at the first complete batch.  K only grows along the list, so the complete batches are a suffix of it: `continue` does the same
            if s.A.shape[1] == K_all:
                continue
            self._hand_down(s)                                             # :97-100
            s._grow_K(K_all)                                               # :103-106
            s.update_temporal_parallel()                                   # :108

    def update_spatial_batch(self, use_parallel=True, spread_all=False):
        """obj.update_spatial_batch(use_parallel)  (@Sources2D/update_spatial_batch.m:11-45): every batch runs update_spatial_parallel(); with the weights
        cc_k = sum(C_k.^2, 2) (float64, taken where the traces lie: cnmfe_trace_energy) the parent's footprints are the energy-weighted average
        A = (sum_k A_k diag(cc_k)) diag(1 ./ sum_k cc_k), accumulated as float64 sparse on the host and stored float32.
        Three things about the reference:
        1. `obj.post_process_spatial()` at :34 drops its result (the method returns the processed matrix, nothing is assigned): it has no effect, none is run here.
        2. the spread loop at :37 stops at nbatches - 1: the LAST batch keeps its own update.  The default reproduces this; spread_all=True hands the average
           to every batch.
        3. a neuron without energy in any batch is a NaN column in the reference (0 * Inf on a dense matrix); here it is an empty column, and the method RETURNS the
           0-based indices of such neurons.
        A batch receives the new A as a spatial update would leave it (Sources2D._set_A); its traces are not touched or uploaded again.  "No K x T matrix moves" holds
        while a batch's C is its engine's bound matrix, as every update method leaves it; a C the caller replaced without binding it is uploaded once for its weights
        (counter merge_trace_uploads)."""
        d, K = self.A.shape
        if K == 0:
            return np.zeros(0, dtype=np.int64)                             # :14-17 "You have to initialize neurons first"
        acc = sp.csc_matrix((d, K), dtype=np.float64)                      # :18
        cc = np.zeros((len(self.batches), K), dtype=np.float64)            # :19
        for m, s in enumerate(self.batches):
            s.update_spatial_parallel()                                    # :28
            if s.A.shape[1] != K:
                raise ValueError("batch %d has %d neurons, the parent %d" % (m + 1, s.A.shape[1], K))
            cc[m] = s._trace_energy()                                      # :29
            Ak = sp.csc_matrix(s.A, dtype=np.float64)
            dead = np.repeat(cc[m] == 0, np.diff(Ak.indptr))               # (a column without energy contributes nothing, whatever its update left in it: no 0 * NaN)
            if dead.any():
                Ak = Ak.copy(); Ak.data[dead] = 0.0
            acc = acc + Ak @ sp.diags(cc[m])                               # :30
        tot = cc.sum(axis=0)
        live = tot > 0
        inv = np.zeros(K, dtype=np.float64)
        inv[live] = 1.0 / tot[live]
        A = sp.csc_matrix(sp.csc_matrix(acc) @ sp.diags(inv), dtype=np.float32)      # :33
        A.eliminate_zeros(); A.sort_indices()
        self.A = A
        for s in (self.batches if spread_all else self.batches[:-1]):      # :37-45
            s._set_A(A)
        return np.flatnonzero(~live)

    def update_temporal_batch(self, use_parallel=True):
        """obj.update_temporal_batch(use_parallel)  (@Sources2D/update_temporal_batch.m:19-33): per batch, C grows by zero rows where the parent's K is larger
        (:24-27), then update_temporal_parallel()"""
        K = self.A.shape[1]
        if K == 0:
            return                                                         # :13-16
        for s in self.batches:
            if K > s.C.shape[0]:
                s._grow_K(K)                                               # :25-27
            s.update_temporal_parallel()                                   # :29

    def update_background_batch(self, use_parallel=True):
        """obj.update_background_batch(use_parallel)  (@Sources2D/update_background_batch.m:13-24)"""
        for s in self.batches:
            s.update_background_parallel()                                 # :20

    def correlation_pnr_batch(self):
        """obj.correlation_pnr_batch()  (Sources2D.m:1901-1912): Cn, PNR of every batch, set on the batch; returns the list of (Cn, PNR)"""
        out = []
        for s in self.batches:
            s.Cn, s.PNR = s.correlation_pnr_parallel()                     # :1907
            out.append((s.Cn, s.PNR))
        return out

    def concatenate_temporal_batch(self):
        """obj.concatenate_temporal_batch()  (Sources2D.m:708-738): C, C_raw and, under deconv_flag, S of the parent, K x sum(T_k) float32; every batch's matrix is
        copied straight into its column range"""
        T_k = [int(t) for t in self.P["numFrames"]]                        # :709
        K = self.A.shape[1]                                                # :711
        names = ("C", "C_raw") + (("S",) if self.options.deconv_flag else ())
        out = {n: np.zeros((K, sum(T_k)), dtype=np.float32) for n in names}      # :712-717
        t = 0
        for s, n_t in zip(self.batches, T_k):
            for n in names:
                out[n][:, t:t + n_t] = getattr(s, n)                       # :723-730 (a shape that does not fit raises)
            t += n_t
        self.C, self.C_raw = out["C"], out["C_raw"]                        # :733-734
        if self.options.deconv_flag:
            self.S = out["S"]                                              # :735-737
