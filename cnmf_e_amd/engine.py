"""Thin numpy-facing wrapper over the C ABI (one Engine == one cnmfe_ctx == one GPU).

Mirrors the reference's per-patch kernel functions (SURVEY.md section 8(b) level 2):
  fit_ring_model, the residual expression, HALS_spatial(_thresh), nnls_spatial,
  HALS_temporal, post_process_spatial.
All arrays cross the boundary as plain pointers; sparse matrices are scipy CSC
(MATLAB's layout).  Trace matrices are numpy (K, T) C-order == CNMFE_ROWMAJOR.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from . import _lib as L

_DT = {np.dtype(np.float32): L.F32, np.dtype(np.float64): L.F64, np.dtype(np.uint16): L.U16,
       np.dtype(np.uint8): L.U8, np.dtype(np.float16): L.F16}


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None and a.size else C.cast(None, t)


def _csc(A, nrow):
    """-> (K, colptr int64, rowidx int32, val float32) with sorted, de-duplicated columns."""
    A = sp.csc_matrix(A)
    if A.shape[0] != nrow:
        raise ValueError("sparse matrix has %d rows, expected %d" % (A.shape[0], nrow))
    if not A.has_canonical_format:
        A = A.copy(); A.sum_duplicates(); A.sort_indices()
    return (A.shape[1], np.ascontiguousarray(A.indptr, dtype=np.int64),
            np.ascontiguousarray(A.indices, dtype=np.int32), np.ascontiguousarray(A.data, dtype=np.float32))


def _traces(Cm, K, T):
    Cm = np.ascontiguousarray(Cm, dtype=np.float32)
    if Cm.shape != (K, T):
        raise ValueError("trace matrix has shape %s, expected %s" % (Cm.shape, (K, T)))
    return Cm


class BoundRows:
    """C(ind, :) of a trace matrix, kept as (matrix, row indices): when the matrix is the one bound on the engine the rows are gathered
    on the device (CNMFE_BOUND_ROWS); anywhere else it behaves like the array C[ind] (np.asarray)"""
    def __init__(self, parent, ind):
        self.parent = parent
        self.ind = np.ascontiguousarray(ind, dtype=np.int32)
        self.shape = (int(self.ind.size), int(parent.shape[1]))
        self.dtype = parent.dtype
        self.ndim = 2
    def __array__(self, dtype=None, copy=None):
        a = self.parent[self.ind]
        return a if dtype is None else a.astype(dtype, copy=False)
    def __len__(self):
        return self.shape[0]
    def __getitem__(self, key):
        return np.asarray(self)[key]
    def mean(self, *a, **k):
        return np.asarray(self).mean(*a, **k)


class DeviceTraces:
    """A K x T fp32 trace matrix that lives in a torch DEVICE tensor (what the sharded temporal update's all-reduce produces).  It is bound on
    the engine device-to-device, row subsets go through BoundRows, row means are taken on the device; a host copy is only made when
    somebody actually reads the values (np.asarray), and then kept."""
    def __init__(self, tensor):
        self.tensor = tensor.contiguous()
        self.shape = tuple(int(x) for x in tensor.shape)
        self.dtype = np.dtype(np.float32)
        self.ndim = 2
        self.flags = {"C_CONTIGUOUS": True}
        self._host = None
    def host(self):
        if self._host is None:
            self._host = self.tensor.cpu().numpy()
        return self._host
    def __array__(self, dtype=None, copy=None):
        a = self.host()
        return a if dtype is None else a.astype(dtype, copy=False)
    def __getitem__(self, key):
        return self.host()[key]
    def __len__(self):
        return self.shape[0]
    def mean(self, axis=None, dtype=None, **k):
        import torch
        if axis == 1 and self._host is None:
            return self.tensor.to(torch.float64).mean(dim=1).cpu().numpy().astype(dtype or np.float64)
        return self.host().mean(axis=axis, dtype=dtype, **k)
    def copy(self):
        return self.host().copy()
    def data_ptr(self):
        return self.tensor.data_ptr()


class BoundOnly:
    """identity of a trace matrix that exists only as the engine's bound device matrix (stitch_finish(want="bound")): it can be passed where the bound
    matrix is meant; it has no host values"""
    def __init__(self, K, T):
        self.shape = (int(K), int(T)); self.dtype = np.dtype(np.float32); self.ndim = 2
        self.flags = {"C_CONTIGUOUS": True}
    def __array__(self, dtype=None, copy=None):
        raise RuntimeError("this trace matrix was left on the device only (stitch_finish(want='bound')): deconvolve or download it through the engine")


class _PinnedBlock:
    """Owner of one pinned host buffer of a LazyHostTraces.  The ctypes array every ndarray view of the buffer is built on holds the only strong
    reference to this object, so the block goes back to the engine's pool -- or is freed, once the engine is closed or gone -- when the LAST view
    dies: an array taken from `s.C` (np.asarray, a slice, .T) stays valid for as long as somebody holds it, whatever happens to `s` or the engine."""
    def __init__(self, eng, nbytes):
        import weakref
        self.eng = weakref.ref(eng); self.nbytes = nbytes; self.ready = False
        self.gen = None                                   # the download batch that fills the buffer (Engine._mark_batch): what wait() waits for
        self.ptr = eng._pinned_take(nbytes)
        self._free = L.lib.cnmfe_host_free                # the library that allocated the buffer frees it, whatever `L` is when the last view dies
    def _wait_ctx(self, ctx, check):
        # this block's batch only: the copy stream may already hold the NEXT iteration's downloads, which a release of this buffer must not wait for
        rc = L.lib.cnmfe_stitch_wait(ctx) if self.gen is None else L.lib.cnmfe_copy_wait(ctx, self.gen)
        if check:
            L.check(rc)
    def wait(self):
        if not self.ready:
            eng = self.eng()
            if eng is not None and getattr(eng, "_ctx", None):
                self._wait_ctx(eng._ctx, True)                   # cnmfe_destroy drains the copy stream itself
            self.ready = True
    def __del__(self):
        try:
            eng = self.eng()
            if eng is not None and getattr(eng, "_ctx", None):
                if not self.ready:
                    self._wait_ctx(eng._ctx, False)              # the copy may still be writing into the buffer
                eng._pinned_give(self.ptr, self.nbytes)
            else:
                self._free(self.ptr)
        except Exception:
            pass


class LazyHostTraces:
    """The K x T result of the temporal update as the host sees it: the engine keeps the matrix bound on the device (that is what the next
    background / spatial / temporal calls read) and streams a copy into pinned host memory on a second stream; the first time somebody
    READS the values (np.asarray, indexing, mean) this object waits for that copy -- never for the compute stream.  Identity of the bound
    matrix like any array returned by stitch_finish.  Arrays handed out are views of the pinned buffer and keep it alive (_PinnedBlock);
    np.array(x) / x.copy() / x.astype(...) are copies as for an ndarray."""
    def __init__(self, eng, K, T):
        self._eng = eng
        self.shape = (int(K), int(T)); self.dtype = np.dtype(np.float32); self.ndim = 2
        self.flags = {"C_CONTIGUOUS": True}
        n = max(1, K * T)
        blk = _PinnedBlock(eng, n * 4)
        buf = (C.c_float * n).from_address(blk.ptr)
        buf._owner = blk                                  # buf <- memoryview <- ndarray (and every view of it): the block lives as long as they do
        self._ptr = blk.ptr
        self._blk = __import__("weakref").ref(blk)
        self._arr = np.frombuffer(buf, dtype=np.float32, count=K * T).reshape(K, T)
    @property
    def _ready(self):
        return self._blk().ready
    def host(self):
        self._blk().wait()
        return self._arr
    def __array__(self, dtype=None, copy=None):
        a = self.host()
        if dtype is not None and np.dtype(dtype) != a.dtype:
            if copy is False:
                raise ValueError("a float32 trace matrix cannot be viewed as %s without a copy" % np.dtype(dtype))
            return a.astype(dtype)
        return a.copy() if copy else a
    def __getitem__(self, key):
        return self.host()[key]
    def __len__(self):
        return self.shape[0]
    def mean(self, *a, **k):
        return self.host().mean(*a, **k)
    def copy(self):
        return self.host().copy()
    def astype(self, *a, **k):
        return self.host().astype(*a, **k)
    def __getattr__(self, name):                      # everything else an ndarray has (.T, .sum, .max, ...): the host copy's
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.host(), name)


class GrownTraces:
    """[X; zeros(n, T)] of a trace matrix X that Engine.traces_grow grew ON THE DEVICE: the host object that stands for the grown matrix (its identity is the
    bound matrix' or a resident's from then on).  No value moves when it is made; X -- an array, or a LazyHostTraces whose rows may not even have arrived -- stays valid and
    is read, below n zero rows, the first time somebody reads the values."""
    def __init__(self, old, K_new):
        self._old = old
        self.shape = (int(K_new), int(old.shape[1])); self.dtype = np.dtype(np.float32); self.ndim = 2
        self.flags = {"C_CONTIGUOUS": True}
        self._arr = None
    def host(self):
        if self._arr is None:
            a = np.zeros(self.shape, dtype=np.float32)
            a[:self._old.shape[0]] = np.asarray(self._old)
            self._arr, self._old = a, None
        return self._arr
    def __array__(self, dtype=None, copy=None):
        a = self.host()
        if dtype is not None and np.dtype(dtype) != a.dtype:
            if copy is False:
                raise ValueError("a float32 trace matrix cannot be viewed as %s without a copy" % np.dtype(dtype))
            return a.astype(dtype)
        return a.copy() if copy else a
    def __getitem__(self, key):
        return self.host()[key]
    def __len__(self):
        return self.shape[0]
    def mean(self, *a, **k):
        return self.host().mean(*a, **k)
    def copy(self):
        return self.host().copy()
    def astype(self, *a, **k):
        return self.host().astype(*a, **k)
    def __getattr__(self, name):                      # everything else an ndarray has: the host copy's (as LazyHostTraces)
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.host(), name)


for _cls in (LazyHostTraces, GrownTraces):
    for _op in ("add", "sub", "mul", "truediv", "radd", "rsub", "rmul", "rtruediv", "lt", "le", "gt", "ge", "eq", "ne", "neg", "abs", "matmul", "rmatmul"):
        setattr(_cls, "__%s__" % _op, (lambda op: lambda self, *a: getattr(self.host(), "__%s__" % op)(*a))(_op))
    _cls.__hash__ = object.__hash__


class SpatialResult:
    """The spatial update of one patch that update_spatial(defer=True) queued: the sweeps are in flight, the caller does other host work under them and calls this
    object for the values (before the next spatial update).  r() is the updated A as a CSC matrix with exactly IND's pattern (explicit zeros kept).
    connected_fov = (d1, d2): the patch is the whole field of view -- also apply the connectivity constraint on the device and return (A_raw, A) instead of A_raw.
    compact: without the stored zeros of the mask pattern (rows sorted); with connected_fov, A_raw then comes as a callable that builds it on first use."""
    def __init__(self, eng, d, K, icp, iri, out):
        self._eng, self._d, self._K, self._icp, self._iri, self._out = eng, d, K, icp, iri, out
        self._pend = None                                 # the queued download: None, or (ticket, pinned block, its bytes, True: the keep flags come with the values)

    def _queue(self, nbytes, keep, call):
        """a download into a pooled pinned block (by size class), queued by call(block, ticket)"""
        if self._out.size == 0 or self._pend is not None:
            return
        nb = 1 << max(12, int(nbytes - 1).bit_length())
        ptr = self._eng._pinned_take(nb)
        tk = C.c_int64(0)
        try:
            L.check(call(ptr, C.byref(tk)))
        except Exception:
            self._eng._pinned_give(ptr, nb)
            raise
        self._pend = (tk.value, ptr, nb, keep)

    def _collect(self, keep=None):
        """the queued download (keep: the one with the keep flags): wait for its ticket, copy out of the pinned block, give the block back.  False: none of that kind"""
        if self._pend is None or self._pend[3] != (keep is not None):
            return False
        (tk, ptr, nb, _), self._pend, out = self._pend, None, self._out
        try:
            L.check(L.lib.cnmfe_ticket_wait(self._eng._ctx, tk))
            C.memmove(out.ctypes.data, ptr, out.size * 4)
            if keep is not None:
                C.memmove(keep.ctypes.data, ptr + out.size * 4, out.size)
        finally:
            self._eng._pinned_give(ptr, nb)
        return True

    def start(self):
        """queue the download into pinned memory right behind the sweeps: r() then waits for that point of the stream only, so the caller may queue the next patch first"""
        n = int(self._out.size)
        self._queue(n * 4, False, lambda ptr, tk: L.lib.cnmfe_update_spatial_fetch_async(self._eng._ctx, ptr, n, tk))

    def start_connected(self, connected_fov):
        """queue the connectivity constraint + the downloads of (values, keep flags) into pinned memory now; r(connected_fov=...) then only waits for them"""
        n = int(self._out.size)
        self._queue(n * 5, True, lambda ptr, tk: L.lib.cnmfe_update_spatial_fetch_connected_async(
            self._eng._ctx, int(connected_fov[0]), int(connected_fov[1]), self._K, _p(self._icp, L.i64p), _p(self._iri, L.i32p), ptr, ptr + n * 4, tk))

    def temporal_early(self):
        """behind start_connected: queue the temporal update's projection of the post-processed result where it lies (cnmfe_temporal_early_project).
        Returns a token for temporal_early_claim, 0 when the engine declines"""
        if self._pend is None or not self._pend[3] or not hasattr(L.lib, "cnmfe_temporal_early_project"):
            return 0
        tk = C.c_int64(0)
        L.check(L.lib.cnmfe_temporal_early_project(self._eng._ctx, self._K, _p(self._icp, L.i64p), _p(self._iri, L.i32p), C.byref(tk)))
        return tk.value

    def compacted(self, vals, keep=None):
        """CSC of the non-zero values (keep: and flagged entries) on IND's pattern, rows sorted: one pass in the library's host helper --
        scipy's eliminate_zeros() on the 250 k-entry mask pattern was the longest host step between the spatial and the temporal update"""
        K, icp, iri = self._K, self._icp, self._iri
        optr = np.empty(K + 1, dtype=np.int64); orow = np.empty(max(1, vals.size), dtype=np.int32); oval = np.empty(max(1, vals.size), dtype=np.float32)
        n = C.c_int64(0)
        L.check(L.lib.cnmfe_csc_drop_zeros(K, icp.ctypes.data, iri.ctypes.data, vals.ctypes.data, None if keep is None else keep.ctypes.data,
                                           optr.ctypes.data, orow.ctypes.data, oval.ctypes.data, C.byref(n)))
        M = sp.csc_matrix((oval[:n.value], orow[:n.value], optr), shape=(self._d, K))
        M.has_canonical_format = True                            # (sorted rows, no duplicates: the mask's pattern was canonical)
        return M

    def _on_pattern(self, vals):
        return sp.csc_matrix((vals, self._iri.copy(), self._icp.copy()), shape=(self._d, self._K))

    def __call__(self, connected_fov=None, compact=False):
        eng, out = self._eng, self._out
        if connected_fov is None:
            if not self._collect():
                L.check(L.lib.cnmfe_update_spatial_fetch(eng._ctx, _p(out, L.f32p), int(out.size)))
            return self.compacted(out) if compact else self._on_pattern(out)
        keep = np.zeros(out.size, dtype=np.uint8)
        if not self._collect(keep):
            L.check(L.lib.cnmfe_update_spatial_fetch_connected(eng._ctx, int(connected_fov[0]), int(connected_fov[1]), self._K, _p(self._icp, L.i64p),
                                                               _p(self._iri, L.i32p), _p(out, L.f32p), _p(keep, L.u8p)))
        if compact:                                  # the raw update (obj.A before post-processing) is compacted when somebody reads it: nothing in the iteration does
            return (lambda: self.compacted(out)), self.compacted(out, keep)
        return self._on_pattern(out), self._on_pattern(out * keep)


class Engine:
    # what this engine offers beyond the blocking calls.  Sources2D asks these flags, where it decides, and nothing else; every stand-in for an engine declares them
    supports_lazy_traces = True       # update_spatial(defer=True) -> SpatialResult, stitch_finish(want="lazy")
    supports_temporal_jobs = True     # hals_temporal_job / temporal_jobs_sweep / stitch_add_job: several patches' temporal updates swept together
    supports_queued_fetch = True      # SpatialResult.start() and r(compact=True): a patch's result collected late
    supports_connected_start = True   # SpatialResult.start_connected()
    supports_temporal_early = True    # SpatialResult.temporal_early(), temporal_early_claim(), hals_temporal(want_aa=False)
    supports_bound_traces = True      # bind_traces()
    supports_bound_deconv = True      # deconv_temporal_bound()
    supports_fit_reserve = True       # fit_reserve()
    supports_synchronize = True       # synchronize()
    supports_init_temporal = True     # init_temporal() / init_temporal_job()
    supports_init_ds = True           # seed_images_ds() / peel_open_ds(): options.ssub / options.tsub of the seed images and the first initialisation
    supports_init_residual_ds = True  # peel_open_residual_ds(): options.ssub / options.tsub of the second pass (initComponents_residual_parallel)
    supports_traces_grow = True       # traces_grow(): zero rows under the bound matrix and its residents, on the device
    supports_image_ops = True         # circular_constraints() / search_dilate() / trim_spatial(): the image operations on single footprints (footprint_ops.hpp)
    supports_bg_svd = True            # bg_svd_fit() / bg_svd_get() / bg_svd_set() / bg_svd_stats() / residual_lowrank(): options.background_model = 'svd'
    supports_bg_svd_init_residual = True  # peel_open_lowrank(): the second pass (initComponents_residual_parallel) under the svd model
    supports_bg_svd_init_temporal = True  # init_temporal_lowrank(): initTemporal (and with it batch mode) under the svd model
    supports_bg_svd_demix = True      # demix_frames_lowrank(): demixed_frames / show_demixed_video under the svd model
    IMAGE_OPS_MAX_BOX = 4096          # cells of the largest box those kernels take (FP_MAX_CELLS); a column above it is computed by hostops and spliced in

    # pinned buffers of LazyHostTraces, recycled by size (page-locking 20 MB costs milliseconds)
    def _pinned_take(self, nbytes):
        pool = self.__dict__.setdefault("_pinned_pool", {})
        lst = pool.get(nbytes)
        if lst:
            return lst.pop()
        p = L.lib.cnmfe_host_alloc(nbytes)
        if not p:
            raise L.CnmfeError(L.lib.cnmfe_last_error().decode("utf-8", "replace"))
        return p
    def _pinned_give(self, ptr, nbytes):
        pool = self.__dict__.get("_pinned_pool")
        if pool is None or getattr(self, "_ctx", None) is None:
            L.lib.cnmfe_host_free(ptr)
        else:
            pool.setdefault(nbytes, []).append(ptr)

    # -- bound traces: obj.C is the same matrix for several calls of one iteration; bind_traces uploads it once and every
    # call that is handed THAT array object afterwards passes (NULL, CNMFE_BOUND).  The array must not be mutated in place
    # while it is bound (Sources2D replaces C, it never writes into it).
    def bind_traces(self, Cm, device_ptr=None):
        """device_ptr: address of a row-major fp32 DEVICE copy of Cm (e.g. the tensor an all-reduce just produced): the engine then binds
        with a device-to-device copy; Cm stays the host-side identity of the bound matrix"""
        Cm = None if Cm is None or Cm.shape[0] == 0 else Cm
        self._res = None                                  # (a new binding: the context's C_raw / S no longer belong to the bound matrix)
        if isinstance(Cm, DeviceTraces):
            device_ptr = Cm.data_ptr()
        if Cm is None or Cm.dtype != np.float32 or not Cm.flags["C_CONTIGUOUS"]:
            self._bound = None
            L.check(L.lib.cnmfe_traces_bind(self._ctx, 0, 0, None, L.ROWMAJOR))
            return
        src = _p(Cm, L.f32p) if device_ptr is None else C.cast(int(device_ptr), L.f32p)
        L.check(L.lib.cnmfe_traces_bind(self._ctx, Cm.shape[0], Cm.shape[1], src, L.ROWMAJOR))
        self._bound = Cm

    def _targs(self, Cm, K, T):
        """(pointer, c_order, keep-alive) for a K x T trace argument"""
        if K == 0 or Cm is None:
            return None, L.ROWMAJOR, None
        if Cm is getattr(self, "_bound", None) and Cm.shape == (K, T):
            return None, L.BOUND, None
        if isinstance(Cm, BoundRows) and Cm.parent is getattr(self, "_bound", None) and Cm.shape == (K, T):
            return C.cast(Cm.ind.ctypes.data, L.f32p), L.BOUND_ROWS, Cm.ind
        a = _traces(Cm, K, T)
        return _p(a, L.f32p), L.ROWMAJOR, a

    def __init__(self, device: int = 0):
        self._opts_set = {}
        self._ctx = L.lib.cnmfe_create(int(device))
        if not self._ctx:
            raise L.CnmfeError("cnmfe_create failed: " + L.lib.cnmfe_last_error().decode())
        self.device = device
        self._patch = {}
        self._peel = {}                     # patch id -> (frames, rows, columns) of its open peel session: the block, or the patch of a residual session

    def close(self):
        if getattr(self, "_ctx", None):
            L.lib.cnmfe_destroy(self._ctx)
            self._ctx = None
            for lst in self.__dict__.pop("_pinned_pool", {}).values():
                for ptr in lst:
                    L.lib.cnmfe_host_free(ptr)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data plane ---------------------------------------------------------
    def create_patch(self, pid, patch_rect, block_rect, d1, d2, T):
        pr = np.asarray(patch_rect, dtype=np.int32); br = np.asarray(block_rect, dtype=np.int32)
        L.check(L.lib.cnmfe_patch_create(self._ctx, pid, _p(pr, L.i32p), _p(br, L.i32p), d1, d2, T))
        nr, nc = int(pr[1] - pr[0] + 1), int(pr[3] - pr[2] + 1)
        nrb, ncb = int(br[1] - br[0] + 1), int(br[3] - br[2] + 1)
        self._patch[pid] = dict(d=nr * nc, d_b=nrb * ncb, T=int(T), nr=nr, nc=nc, nr_b=nrb, nc_b=ncb)

    def upload_block(self, pid, Y, t0=0):
        """Y: (nt, d_b) host array (float32/float64/uint16/uint8/float16), frames t0..t0+nt."""
        Y = np.ascontiguousarray(Y)
        if Y.dtype not in _DT:
            # element types the ABI has no code for (int16 TIFF / HDF5 recordings, int32, bool): widened on the host to the narrowest float that holds
            # them exactly -- the device stores fp32 either way
            if Y.dtype.kind not in "iub":
                raise TypeError("cannot upload a block of %s" % Y.dtype)
            Y = Y.astype(np.float32 if Y.dtype.itemsize <= 2 else np.float64)
        info = self._patch[pid]
        if Y.ndim != 2 or Y.shape[1] != info["d_b"]:
            raise ValueError("block must be (frames, %d), got %s" % (info["d_b"], Y.shape))
        L.check(L.lib.cnmfe_upload_block(self._ctx, pid, Y.ctypes.data_as(C.c_void_p), _DT[Y.dtype], L.HOST, t0, Y.shape[0]))

    def upload_block_device(self, pid, dev_ptr, nt, t0=0, dtype=L.F32):
        """dev_ptr: raw device address of an (nt, d_b) array already in HBM (e.g. torch tensor .data_ptr())."""
        L.check(L.lib.cnmfe_upload_block(self._ctx, pid, C.c_void_p(int(dev_ptr)), dtype, L.DEVICE, t0, nt))

    def ymean(self, pid):
        out = np.empty(self._patch[pid]["d_b"], dtype=np.float64)
        L.check(L.lib.cnmfe_get_ymean(self._ctx, pid, _p(out, L.f64p)))
        return out

    # ---- ring -----------------------------------------------------------------
    def ring_init(self, pid, radius, num_neighbors=None):
        L.check(L.lib.cnmfe_ring_init(self._ctx, pid, int(radius), int(num_neighbors or 0)))

    def fit_reserve(self, pid):
        """allocate the ring fit's large device buffers of this patch now (cnmfe_fit_reserve): the first fit then queues its kernels without a hipMalloc"""
        L.check(L.lib.cnmfe_fit_reserve(self._ctx, pid))

    def ring_csr(self, pid):
        nnz = C.c_int64(); p = C.c_int32()
        L.check(L.lib.cnmfe_ring_nnz(self._ctx, pid, C.byref(nnz), C.byref(p)))
        info = self._patch[pid]
        rowptr = np.empty(info["d"] + 1, dtype=np.int64)
        col = np.empty(nnz.value, dtype=np.int32); val = np.empty(nnz.value, dtype=np.float32)
        L.check(L.lib.cnmfe_ring_get_csr(self._ctx, pid, _p(rowptr, L.i64p), _p(col, L.i32p), _p(val, L.f32p)))
        return sp.csr_matrix((val, col, rowptr), shape=(info["d"], info["d_b"]))

    def ring_first_run(self, pid):
        f = C.c_int()
        L.check(L.lib.cnmfe_ring_first_run(self._ctx, pid, C.byref(f)))
        return bool(f.value)

    def ring_set_values(self, pid, val):
        val = np.ascontiguousarray(val, dtype=np.float32)
        L.check(L.lib.cnmfe_ring_set_values(self._ctx, pid, _p(val, L.f32p)))

    def b0(self, pid):
        out = np.empty(self._patch[pid]["d"], dtype=np.float32)
        L.check(L.lib.cnmfe_b0_get(self._ctx, pid, _p(out, L.f32p)))
        return out

    def set_b0(self, pid, b0):
        b0 = np.ascontiguousarray(b0, dtype=np.float32)
        L.check(L.lib.cnmfe_b0_set(self._ctx, pid, _p(b0, L.f32p)))

    def estimate_noise(self, pid, nframes=None):
        """GetSn of the first `nframes` (default min(T, 3000), Sources2D.m:333-335) frames of the raw video, per block pixel"""
        info = self._patch[pid]
        n = min(info["T"], 3000) if nframes is None else int(nframes)
        out = np.empty(info["d_b"], dtype=np.float32)
        L.check(L.lib.cnmfe_estimate_noise(self._ctx, pid, n, _p(out, L.f32p)))
        return out

    def seed_images(self, pid, psf, nframes=None, Q=None, sig=3.0, frame0=0):
        """[Cn, PNR] = correlation_image_endoscope(Ypatch, options) of the BLOCK of a patch (correlation_image_endoscope.m:36-96) over the first `nframes`
        frames (default all): psf = the spatial filter (sources2d.seed_psf; None = no filter), Q = nframes x M orthonormal detrend basis (None = none),
        sig = the threshold factor.  Two float32 arrays of d_b pixels, column-major in the block."""
        info, n, psf_a, psf_n, Q_a, M = self._seed_args(pid, psf, nframes, Q)
        Cn = np.empty(info["d_b"], dtype=np.float32); PNR = np.empty(info["d_b"], dtype=np.float32)
        L.check(L.lib.cnmfe_seed_images(self._ctx, pid, _p(psf_a, L.f32p), psf_n, int(frame0), n, _p(Q_a, L.f64p), M, float(sig),
                                        _p(Cn, L.f32p), _p(PNR, L.f32p)))
        return Cn, PNR

    # ---- greedy initialisation: a peel session per patch (cnmfe_peel_* in include/cnmfe.h) ----
    def _seed_args(self, pid, psf, nframes, Q):
        info = self._patch[pid]
        n = info["T"] if nframes is None else int(nframes)
        psf_a, psf_n = None, 0
        if psf is not None and np.size(psf):
            psf = np.asarray(psf, dtype=np.float32)
            if psf.ndim != 2 or psf.shape[0] != psf.shape[1]:
                raise ValueError("psf must be square, got %s" % (psf.shape,))
            psf_n = int(psf.shape[0])
            psf_a = np.ascontiguousarray(psf.T)                            # column-major
        Q_a, M = None, 0
        if Q is not None and np.size(Q):
            Q = np.asarray(Q, dtype=np.float64)
            if Q.ndim != 2 or Q.shape[0] != n:
                raise ValueError("Q must be (%d, M), got %s" % (n, Q.shape))
            M = int(Q.shape[1])
            Q_a = np.ascontiguousarray(Q.T)                                # column-major
        return info, n, psf_a, psf_n, Q_a, M

    @staticmethod
    def peel_box(nr_b, nc_b, r, c, reach):
        """(r0, r1, c0, c1), 0-based half-open, of the box of `reach` around the 0-based block pixel (r, c) (greedyROI_endoscope.m:299-300,310-311)"""
        return max(0, r - reach), min(nr_b, r + reach + 1), max(0, c - reach), min(nc_b, c + reach + 1)

    def peel_open(self, pid, psf, nframes=None, Q=None, sig=3.0, frame0=0):
        """open the peel session of a patch: (Cn, PNR, Sn) of its block as seed_images gives them (+ GetSn of the filtered traces), d_b float32 each"""
        info, n, psf_a, psf_n, Q_a, M = self._seed_args(pid, psf, nframes, Q)
        Cn = np.empty(info["d_b"], dtype=np.float32); PNR = np.empty(info["d_b"], dtype=np.float32); Sn = np.empty(info["d_b"], dtype=np.float32)
        L.check(L.lib.cnmfe_peel_open(self._ctx, pid, _p(psf_a, L.f32p), psf_n, int(frame0), n, _p(Q_a, L.f64p), M, float(sig),
                                      _p(Cn, L.f32p), _p(PNR, L.f32p), _p(Sn, L.f32p)))
        self._peel[pid] = (n, info["nr_b"], info["nc_b"])
        return Cn, PNR, Sn

    def peel_open_residual(self, pid, A_patch, C, psf, sig=3.0, want_video=False):
        """open the peel session of the SECOND pass on a patch (initComponents_residual_parallel.m:186-220): the session runs on the patch and on
        Yres = Ysig - A_patch C, Ysig the resident residual (residual() / residual_ssub() first, with the block's current neurons).  A_patch: d x K sparse over the
        patch rows (None: no neuron), C: their K x T traces.  Returns (Cn, PNR, Sn, Yres): d float32 each, column-major in the patch; Yres (want_video) is the
        (T, d) float32 video the session searches, else None.  extract / apply then take seeds 0-based in the PATCH.  Closing the session drops the residual."""
        info = self._patch[pid]
        _i, n, psf_a, psf_n, _q, _m = self._seed_args(pid, psf, None, None)
        K, cp, ri, va = _csc(A_patch, info["d"]) if A_patch is not None and A_patch.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C, K, info["T"])
        Cn = np.empty(info["d"], dtype=np.float32); PNR = np.empty(info["d"], dtype=np.float32); Sn = np.empty(info["d"], dtype=np.float32)
        out = np.empty((info["T"], info["d"]), dtype=np.float32) if want_video else None
        dst = out.ctypes.data_as(L.C.c_void_p) if want_video else L.C.c_void_p(None)      # (C is the trace matrix here)
        L.check(L.lib.cnmfe_peel_open_residual(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord, _p(psf_a, L.f32p), psf_n, float(sig),
                                               _p(Cn, L.f32p), _p(PNR, L.f32p), _p(Sn, L.f32p), dst, L.HOST))
        self._peel[pid] = (n, info["nr"], info["nc"])
        return Cn, PNR, Sn, out

    def peel_open_residual_ds(self, pid, ssub, tsub, A_patch, C, psf, sig=3.0, want_video=False):
        """peel_open_residual on dsData(Yres) of the PATCH (options.ssub / options.tsub of the second pass, greedyROI_endoscope.m:46-61): the device forms
        dsData(Ysig) - A_ds C_ds off the resident residual, so no full-resolution Yres exists.  A_patch, C as for peel_open_residual (FULL resolution; the
        library down-samples both).  Returns (Cn, PNR, Sn, Yds): d1s * d2s float32 each, column-major on the ceil(nr / ssub) x ceil(nc / ssub) grid; Yds
        (want_video) is the (Ts, d1s * d2s) float32 video the session searches, Ts = floor(T / tsub), else None.  extract / apply then take seeds 0-based on that
        grid and traces of Ts samples.  ssub = tsub = 1 is peel_open_residual bit for bit.  Closing the session drops the residual."""
        info = self._patch[pid]
        _i, n, psf_a, psf_n, _q, _m = self._seed_args(pid, psf, None, None)
        fs, ft = max(int(ssub), 1), max(int(tsub), 1)                      # (factors below 1 are the library's to refuse: only the buffers are sized here)
        d1s, d2s, Ts = -(-info["nr"] // fs), -(-info["nc"] // fs), n // ft
        K, cp, ri, va = _csc(A_patch, info["d"]) if A_patch is not None and A_patch.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C, K, info["T"])
        ds = max(d1s * d2s, 1)
        Cn = np.empty(ds, dtype=np.float32); PNR = np.empty(ds, dtype=np.float32); Sn = np.empty(ds, dtype=np.float32)
        out = np.empty((max(Ts, 0), d1s * d2s), dtype=np.float32) if want_video else None
        dst = out.ctypes.data_as(L.C.c_void_p) if want_video else L.C.c_void_p(None)
        L.check(L.lib.cnmfe_peel_open_residual_ds(self._ctx, pid, int(ssub), int(tsub), K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord,
                                                  _p(psf_a, L.f32p), psf_n, float(sig), _p(Cn, L.f32p), _p(PNR, L.f32p), _p(Sn, L.f32p), dst, L.HOST))
        self._peel[pid] = (Ts, d1s, d2s)
        return Cn[:d1s * d2s], PNR[:d1s * d2s], Sn[:d1s * d2s], out

    # ---- options.ssub / options.tsub: the same two calls on dsData of the block (cnmfe_seed_images_ds / cnmfe_peel_open_ds) ----
    def ds_dims(self, pid, ssub, tsub, nframes=None):
        """(d1s, d2s, Ts) of dsData (utilities/dsData.m:29-31) of a patch's block over the first `nframes` frames"""
        info = self._patch[pid]
        n = info["T"] if nframes is None else int(nframes)
        ssub, tsub = max(int(ssub), 1), max(int(tsub), 1)                  # (factors below 1 are the library's to refuse: only the buffers are sized here)
        return -(-info["nr_b"] // ssub), -(-info["nc_b"] // ssub), n // tsub

    def seed_images_ds(self, pid, ssub, tsub, psf, nframes=None, Q=None, sig=3.0):
        """seed_images of Yds = dsData(block) (correlation_pnr_parallel.m:86-96): the block is down-sampled on the device (box resize to ceil(nr_b / ssub) x
        ceil(nc_b / ssub), means of tsub frames, Ts = floor(nframes / tsub)), then filtered with `psf` (built from the SCALED gSig / gSiz) and detrended against
        Q, Ts x M.  Two float32 arrays of d1s * d2s pixels, column-major on the low-resolution grid."""
        d1s, d2s, Ts = self.ds_dims(pid, ssub, tsub, nframes)
        _info, n, psf_a, psf_n, _q, _m = self._seed_args(pid, psf, nframes, None)
        Q_a, M = None, 0
        if Q is not None and np.size(Q):
            Q = np.asarray(Q, dtype=np.float64)
            if Q.ndim != 2 or Q.shape[0] != Ts:
                raise ValueError("Q must be (%d, M) for the down-sampled series, got %s" % (Ts, Q.shape))
            M = int(Q.shape[1]); Q_a = np.ascontiguousarray(Q.T)
        Cn = np.empty(max(d1s * d2s, 1), dtype=np.float32); PNR = np.empty(max(d1s * d2s, 1), dtype=np.float32)
        L.check(L.lib.cnmfe_seed_images_ds(self._ctx, pid, int(ssub), int(tsub), _p(psf_a, L.f32p), psf_n, n, _p(Q_a, L.f64p), M, float(sig),
                                           _p(Cn, L.f32p), _p(PNR, L.f32p)))
        return Cn[:d1s * d2s], PNR[:d1s * d2s]

    def peel_open_ds(self, pid, ssub, tsub, psf, nframes=None, Qpre=None, sig=3.0, want_video=False):
        """open the peel session of a patch on Yds = dsData(block) (greedyROI_endoscope.m:46-61).  Qpre: nframes x Mpre, the FULL-LENGTH detrend basis: the block
        is detrended before it is down-sampled (initComponents_parallel.m:341-343), on the device and without a full-resolution copy.  Returns (Cn, PNR, Sn,
        Yds): d1s * d2s float32 each, column-major on the low-resolution grid; Yds (want_video) is the (Ts, d1s * d2s) float32 video the session searches, else
        None.  extract / apply then take seeds 0-based on the d1s x d2s grid and traces of Ts samples."""
        d1s, d2s, Ts = self.ds_dims(pid, ssub, tsub, nframes)
        _info, n, psf_a, psf_n, Q_a, M = self._seed_args(pid, psf, nframes, Qpre)
        ds = max(d1s * d2s, 1)
        Cn = np.empty(ds, dtype=np.float32); PNR = np.empty(ds, dtype=np.float32); Sn = np.empty(ds, dtype=np.float32)
        out = np.empty((max(Ts, 0), d1s * d2s), dtype=np.float32) if want_video else None
        dst = out.ctypes.data_as(L.C.c_void_p) if want_video else L.C.c_void_p(None)
        L.check(L.lib.cnmfe_peel_open_ds(self._ctx, pid, int(ssub), int(tsub), _p(psf_a, L.f32p), psf_n, n, _p(Q_a, L.f64p), M, float(sig),
                                         _p(Cn, L.f32p), _p(PNR, L.f32p), _p(Sn, L.f32p), dst, L.HOST))
        self._peel[pid] = (Ts, d1s, d2s)
        return Cn[:d1s * d2s], PNR[:d1s * d2s], Sn[:d1s * d2s], out

    def peel_extract(self, pid, r, c, gSiz):
        """extract_ac.m:19-58 around the 0-based block pixel (r, c): (corr, ai) as nr x nc float64 images of the box, ci (nframes float64), stats = dict of
        max_diff, std_diff (greedyROI_endoscope.m:287-293), norm_ci, sn_ci (GetSn(ci)), n_hi, n_lo (the sizes of {corr > 0.9}, {corr < 0.3})"""
        info = self._patch[pid]
        n, nr_b, nc_b = self._peel.get(pid, (info["T"], info["nr_b"], info["nc_b"]))      # the session's geometry
        r0, r1, c0, c1 = self.peel_box(nr_b, nc_b, int(r), int(c), int(gSiz))
        npix = max(r1 - r0, 0) * max(c1 - c0, 0)
        corr = np.empty(max(npix, 1), dtype=np.float64); ai = np.empty(max(npix, 1), dtype=np.float64)
        ci = np.empty(n, dtype=np.float64); st = np.empty(6, dtype=np.float64)
        L.check(L.lib.cnmfe_peel_extract(self._ctx, pid, int(r), int(c), int(gSiz), _p(corr, L.f64p), _p(ai, L.f64p), _p(ci, L.f64p), _p(st, L.f64p)))
        sh = (r1 - r0, c1 - c0)
        stats = dict(max_diff=st[0], std_diff=st[1], norm_ci=st[2], sn_ci=st[3], n_hi=int(st[4]), n_lo=int(st[5]))
        return corr[:npix].reshape(sh, order="F"), ai[:npix].reshape(sh, order="F"), ci, stats

    def peel_apply(self, pid, r, c, gSiz, ai_box, Hai_box2, ci, sig, min_pnr, min_corr):
        """greedyROI_endoscope.m:378-402: subtract ai ci from the working video and Hai ci from HY, return (PNR, Cn) of the (4 gSiz + 1)^2 box as float32 images"""
        info = self._patch[pid]
        n, nr_b, nc_b = self._peel.get(pid, (info["T"], info["nr_b"], info["nc_b"]))      # the session's geometry
        r0, r1, c0, c1 = self.peel_box(nr_b, nc_b, int(r), int(c), int(gSiz))
        s0, s1, t0, t1 = self.peel_box(nr_b, nc_b, int(r), int(c), 2 * int(gSiz))
        ai = np.ascontiguousarray(np.asarray(ai_box, dtype=np.float64).reshape(-1, order="F"))
        hai = np.ascontiguousarray(np.asarray(Hai_box2, dtype=np.float64).reshape(-1, order="F"))
        ci = np.ascontiguousarray(ci, dtype=np.float64)
        if ai.size != (r1 - r0) * (c1 - c0) or hai.size != (s1 - s0) * (t1 - t0) or ci.size != n:
            raise ValueError("peel_apply: ai %d, Hai %d, ci %d do not match the boxes %d, %d and %d frames" % (ai.size, hai.size, ci.size, (r1 - r0) * (c1 - c0), (s1 - s0) * (t1 - t0), n))
        pnr = np.empty(max(hai.size, 1), dtype=np.float32); cn = np.empty(max(hai.size, 1), dtype=np.float32)
        L.check(L.lib.cnmfe_peel_apply(self._ctx, pid, int(r), int(c), int(gSiz), _p(ai, L.f64p), _p(hai, L.f64p), _p(ci, L.f64p), float(sig), float(min_pnr),
                                       float(min_corr), _p(pnr, L.f32p), _p(cn, L.f32p)))
        sh = (s1 - s0, t1 - t0)
        return pnr[:hai.size].reshape(sh, order="F"), cn[:hai.size].reshape(sh, order="F")

    def peel_close(self, pid):
        self._peel.pop(pid, None)
        L.check(L.lib.cnmfe_peel_close(self._ctx, pid))

    def set_noise(self, pid, sn_block):
        """sn of the block pixels (update_background_parallel.m:131,137); read by the outlier branch of fit_ring_model only"""
        sn_block = np.ascontiguousarray(sn_block, dtype=np.float32).ravel()
        assert sn_block.size == self._patch[pid]["d_b"], (sn_block.size, self._patch[pid]["d_b"])
        L.check(L.lib.cnmfe_set_noise(self._ctx, pid, _p(sn_block, L.f32p)))

    # ---- kernels ----------------------------------------------------------------
    def fit_ring_model(self, pid, A_block, C_block, thresh_outlier=float("nan"), with_projection=True, want_b0=True):
        """[W, b0] = fit_ring_model(Y, A, C, W_old, thresh_outlier, sn, ind_patch, with_projection); W stays resident."""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_block, info["d_b"]) if A_block is not None else (0, None, None, None)
        cptr, cord, _keep = self._targs(C_block, K, info["T"])
        b0 = np.empty(info["d"], dtype=np.float32) if want_b0 else None
        inf = np.zeros(4, dtype=np.int64)
        L.check(L.lib.cnmfe_fit_ring_model(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr,
                                           cord, float(thresh_outlier), int(bool(with_projection)), _p(b0, L.f32p), _p(inf, L.i64p)))
        return b0, dict(first_run=bool(inf[0]), frame_stride=int(inf[1]), n_active=int(inf[2]), pmax=int(inf[3]))

    def ring_solve_stats(self, pid):
        """diagnostics of the last fit's ring solve out of the cached inverses (cnmfe_ring_solve_stats): pixels left to the factorising kernel, ridge-series terms,
        pixels with at least one term, inverses rebuilt; all -1 without inverses"""
        out = np.zeros(4, dtype=np.int64)
        L.check(L.lib.cnmfe_ring_solve_stats(self._ctx, pid, _p(out, L.i64p)))
        return dict(left_over=int(out[0]), series_terms=int(out[1]), pixels_with_terms=int(out[2]), rebuilt=int(out[3]))

    # -- bg_ssub > 1 ---------------------------------------------------------------------------------------------
    def patch_derive(self, src_pid, new_pid, ssub, mode):
        """low-resolution patch of src_pid (mode 'nearest' | 'bicubic'); its FOV is the ceil(nr_b/s) x ceil(nc_b/s) grid"""
        src = self._patch[src_pid]
        L.check(L.lib.cnmfe_patch_derive(self._ctx, src_pid, new_pid, int(ssub), 0 if mode == "nearest" else 1))
        d1s, d2s = -(-src["nr_b"] // ssub), -(-src["nc_b"] // ssub)
        self._patch[new_pid] = dict(d=d1s * d2s, d_b=d1s * d2s, T=src["T"], nr=d1s, nc=d2s, nr_b=d1s, nc_b=d2s)

    def fit_ring_model_ssub(self, pid, fit_pid, res_pid, ssub, A_block, C_block, thresh_outlier=float("nan"), with_projection=True):
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_block, info["d_b"]) if A_block is not None else (0, None, None, None)
        cptr, cord, _keep = self._targs(C_block, K, info["T"])
        inf = np.zeros(4, dtype=np.int64)
        L.check(L.lib.cnmfe_fit_ring_model_ssub(self._ctx, pid, fit_pid, res_pid, int(ssub), K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p),
                                                cptr, cord, float(thresh_outlier), int(bool(with_projection)), _p(inf, L.i64p)))
        return None, dict(first_run=bool(inf[0]), frame_stride=int(inf[1]), n_active=int(inf[2]), pmax=int(inf[3]))

    def residual_ssub(self, pid, res_pid, ssub, A_prev_block=None, C_prev=None, want=False):
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_prev_block, info["d_b"]) if A_prev_block is not None and A_prev_block.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C_prev, K, info["T"])
        out = np.empty((info["T"], info["d"]), dtype=np.float32) if want else None
        dst = out.ctypes.data_as(C.c_void_p) if want else C.c_void_p(None)
        L.check(L.lib.cnmfe_residual_ssub(self._ctx, pid, res_pid, int(ssub), K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr,
                                          cord, dst, L.HOST))
        return out

    def residual(self, pid, A_prev_block=None, C_prev=None, want=False, out_dev_ptr=None):
        """want=True returns Ysig as a (T, d) host array; out_dev_ptr: raw device address of a (T, d) fp32 buffer that
        receives a device-to-device copy instead."""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_prev_block, info["d_b"]) if A_prev_block is not None and A_prev_block.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C_prev, K, info["T"])
        out = np.empty((info["T"], info["d"]), dtype=np.float32) if want else None
        if out_dev_ptr is not None:
            dst, space = C.c_void_p(int(out_dev_ptr)), L.DEVICE
        else:
            dst, space = (out.ctypes.data_as(C.c_void_p) if want else C.c_void_p(None)), L.HOST
        L.check(L.lib.cnmfe_residual(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord, dst, space))
        return out

    # -- background_model = 'svd' (cnmfe_bg_svd_*, cnmfe_residual_lowrank) ---------------------------------------
    def bg_svd_fit(self, pid, nb, A_block=None, C_block=None):
        """[b, f, b0] = fit_svd_model(Y, nb, A, C, ...) of one patch (update_background_parallel.m:238-242); the factors stay resident.  Returns bg_svd_stats(pid);
        a fit that stopped at the iteration cap is no error: it raises a RuntimeWarning."""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_block, info["d_b"]) if A_block is not None and A_block.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C_block, K, info["T"])
        L.check(L.lib.cnmfe_bg_svd_fit(self._ctx, pid, int(nb), K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord))
        st = self.bg_svd_stats(pid)
        if not st["converged"]:
            import warnings
            warnings.warn("low-rank background of patch %d: %d iterations did not reach the tolerance (residuals %s)"
                          % (pid, st["iterations"], np.array2string(st["residual"], precision=2)), RuntimeWarning, stacklevel=2)
        return st

    def bg_svd_stats(self, pid):
        out = np.zeros(20, dtype=np.float64)
        L.check(L.lib.cnmfe_bg_svd_stats(self._ctx, pid, _p(out, L.f64p)))
        nb = int(out[3])
        return dict(passes=int(out[0]), iterations=int(out[1]), converged=bool(out[2]), nb=nb, residual=out[4:4 + nb].copy(), s=out[12:12 + nb].copy())

    def bg_svd_get(self, pid):
        """(b (d, nb), f (nb, T), b0 (d,)) of one patch, float64"""
        info = self._patch[pid]
        nb = self.bg_svd_stats(pid)["nb"]
        b = np.zeros((nb, info["d"]), dtype=np.float64); f = np.zeros((nb, info["T"]), dtype=np.float64); b0 = np.zeros(info["d"], dtype=np.float64)
        L.check(L.lib.cnmfe_bg_svd_get(self._ctx, pid, _p(b, L.f64p), _p(f, L.f64p), _p(b0, L.f64p)))
        return np.ascontiguousarray(b.T), f, b0

    def bg_svd_set(self, pid, b, f, b0):
        """transplant a saved background: b (d, nb), f (nb, T), b0 (d,)"""
        info = self._patch[pid]
        b = np.asarray(b, dtype=np.float64).reshape(info["d"], -1); nb = b.shape[1]
        f = np.ascontiguousarray(np.asarray(f, dtype=np.float64).reshape(nb, info["T"]))
        b0 = np.ascontiguousarray(np.asarray(b0, dtype=np.float64).reshape(info["d"]))
        bt = np.ascontiguousarray(b.T)                        # nb columns of d, one after the other
        L.check(L.lib.cnmfe_bg_svd_set(self._ctx, pid, nb, _p(bt, L.f64p), _p(f, L.f64p), _p(b0, L.f64p)))

    def residual_lowrank(self, pid, want=False):
        """Ysig = Y(patch) - (b f + b0), resident for the updates (update_spatial_parallel.m:184-187); want=True returns it as a (T, d) host array"""
        info = self._patch[pid]
        out = np.empty((info["T"], info["d"]), dtype=np.float32) if want else None
        L.check(L.lib.cnmfe_residual_lowrank(self._ctx, pid, out.ctypes.data_as(C.c_void_p) if want else C.c_void_p(None), L.HOST))
        return out

    def peel_open_lowrank(self, pid, ssub, tsub, A_patch, C, psf, sig=3.0, want_video=False):
        """open the peel session of the SECOND pass under the svd model (initComponents_residual_parallel.m:107-122,195-199,224-227): the session runs on the PATCH
        and on Yres = Y(patch) - A_patch C - (b f + b0), written in one pass from the resident video and the patch's factors (no residual_lowrank() is needed, none
        is made, and the patch's residual is as valid after peel_close as it was before).  ssub / tsub other than 1: dsData(Yres), through the realised Ysig and
        peel_open_residual_ds' session (closing that one drops the residual).  Arguments and returns as peel_open_residual_ds."""
        info = self._patch[pid]
        _i, n, psf_a, psf_n, _q, _m = self._seed_args(pid, psf, None, None)
        fs, ft = max(int(ssub), 1), max(int(tsub), 1)                      # (factors below 1 are the library's to refuse: only the buffers are sized here)
        d1s, d2s, Ts = -(-info["nr"] // fs), -(-info["nc"] // fs), n // ft
        K, cp, ri, va = _csc(A_patch, info["d"]) if A_patch is not None and A_patch.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C, K, info["T"])
        ds = max(d1s * d2s, 1)
        Cn = np.empty(ds, dtype=np.float32); PNR = np.empty(ds, dtype=np.float32); Sn = np.empty(ds, dtype=np.float32)
        out = np.empty((max(Ts, 0), d1s * d2s), dtype=np.float32) if want_video else None
        dst = out.ctypes.data_as(L.C.c_void_p) if want_video else L.C.c_void_p(None)
        L.check(L.lib.cnmfe_peel_open_lowrank(self._ctx, pid, int(ssub), int(tsub), K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord,
                                              _p(psf_a, L.f32p), psf_n, float(sig), _p(Cn, L.f32p), _p(PNR, L.f32p), _p(Sn, L.f32p), dst, L.HOST))
        self._peel[pid] = (Ts, d1s, d2s)
        return Cn[:d1s * d2s], PNR[:d1s * d2s], Sn[:d1s * d2s], out

    def get_sn(self, pid):
        """sn = GetSn(Ysig) per patch pixel (update_spatial_parallel.m:191-194); needs residual() first"""
        out = np.empty(self._patch[pid]["d"], dtype=np.float32)
        L.check(L.lib.cnmfe_get_sn(self._ctx, pid, _p(out, L.f32p)))
        return out

    def update_spatial(self, pid, algorithm, A_patch, C_patch, IND_patch, sn=None, param=3, defer=False):
        """Returns the updated A as a CSC matrix with exactly IND's pattern (explicit zeros kept).  defer=True returns with the sweeps
        queued, and a SpatialResult that fetches it."""
        info = self._patch[pid]
        alg = {"hals": L.SPATIAL_HALS, "hals_thresh": L.SPATIAL_HALS_THRESH, "nnls": L.SPATIAL_NNLS}[algorithm]
        K, cp, ri, va = _csc(A_patch, info["d"])
        IND = sp.csc_matrix(IND_patch).astype(np.float32)
        IND.sort_indices()
        K2, icp, iri, _ = _csc(IND, info["d"])
        if K2 != K:
            raise ValueError("A and IND disagree on K")
        cptr, cord, _keep = self._targs(C_patch, K, info["T"])
        snf = np.ascontiguousarray(sn, dtype=np.float32).ravel() if sn is not None else None
        out = np.zeros(icp[-1], dtype=np.float32)
        L.check(L.lib.cnmfe_update_spatial(self._ctx, pid, alg, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord,
                                           _p(icp, L.i64p), _p(iri, L.i32p), _p(snf, L.f32p), int(param), None if defer else _p(out, L.f32p)))
        if defer:
            return SpatialResult(self, info["d"], K, icp, iri, out)
        return sp.csc_matrix((out, iri.copy(), icp.copy()), shape=(info["d"], K))

    def hals_temporal(self, pid, A_patch, C_patch, maxIter=5, want_C=True, want_raw=True, want_aa=True):
        """[C, C_raw] = HALS_temporal(Ysig, A, C, maxIter); want_C=False skips the download of C (the caller of
        update_temporal_parallel.m:180 only keeps C_raw), want_raw=False that of C_raw too: it stays on the device for stitch_add.
        want_aa=False: aa stays there as well (returned as None) and the call does not wait for it."""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_patch, info["d"])
        T = info["T"]
        cptr, cord, _keep = self._targs(C_patch, K, T)
        Cout = np.empty((K, T), dtype=np.float32) if want_C else None
        Craw = np.empty((K, T), dtype=np.float32) if want_raw else None
        aa = np.empty(K, dtype=np.float32) if want_aa else None
        L.check(L.lib.cnmfe_hals_temporal(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord,
                                          int(maxIter), _p(Cout, L.f32p), _p(Craw, L.f32p), _p(aa, L.f32p)))
        return Cout, Craw, aa

    def fast_temporal(self, pid, A_patch, want_raw=True):
        """[aa, C_raw] = fast_temporal(Ysig, A) (update_temporal_parallel.m:314-337); returns (C_raw, aa)"""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_patch, info["d"])
        Craw = np.empty((K, info["T"]), dtype=np.float32) if want_raw else None
        aa = np.empty(K, dtype=np.float32)
        L.check(L.lib.cnmfe_fast_temporal(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), L.ROWMAJOR,
                                          _p(Craw, L.f32p), _p(aa, L.f32p)))
        return Craw, aa

    def reconstruct_background(self, pid, b0_block, b0_new_patch, frame0=0, nframes=None):
        """Ybg of one patch (Sources2D.m:1247-1355), frames [frame0, frame0 + nframes): (nframes, d) array; needs the resident residual of (A_prev, C_prev)"""
        info = self._patch[pid]
        nframes = info["T"] - frame0 if nframes is None else int(nframes)
        bb = np.ascontiguousarray(b0_block, dtype=np.float32).ravel(); bn = np.ascontiguousarray(b0_new_patch, dtype=np.float32).ravel()
        out = np.empty((nframes, info["d"]), dtype=np.float32)
        L.check(L.lib.cnmfe_reconstruct_background(self._ctx, pid, _p(bb, L.f32p), _p(bn, L.f32p), int(frame0), nframes, _p(out, L.f32p), L.HOST))
        return out

    def compute_rss(self, pid, A_patch, C_patch, b0_block, b0_new_patch):
        """RSS of one patch, compute_RSS (Sources2D.m:1358-1510): needs the resident residual of (A_prev, C_prev) on the block"""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_patch, info["d"]) if A_patch is not None and A_patch.shape[1] else (0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        cptr, cord, _keep = self._targs(C_patch, K, info["T"])
        bb = np.ascontiguousarray(b0_block, dtype=np.float32).ravel(); bn = np.ascontiguousarray(b0_new_patch, dtype=np.float32).ravel()
        if bb.size != info["d_b"] or bn.size != info["d"]:
            raise ValueError("b0_block / b0_new have %d / %d entries, expected %d / %d" % (bb.size, bn.size, info["d_b"], info["d"]))
        out = C.c_double(0.0)
        L.check(L.lib.cnmfe_compute_rss(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord, _p(bb, L.f32p), _p(bn, L.f32p), C.byref(out)))
        return float(out.value)

    # -- the same two with bg_ssub > 1 ('nearest' resizes, Sources2D.m:1325-1334,1479-1486) --
    def background_ssub(self, pid, fit_pid, ssub, A_prev_block, C_prev, b0_block):
        """W * imresize(Y_block - b0_block - A_prev*C_prev, 1/s, 'nearest') on the fit patch, kept on the device for the two readers below"""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_prev_block, info["d_b"]) if A_prev_block is not None and A_prev_block.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C_prev, K, info["T"])
        bb = np.ascontiguousarray(b0_block, dtype=np.float32).ravel()
        if bb.size != info["d_b"]:
            raise ValueError("b0_block has %d entries, expected %d" % (bb.size, info["d_b"]))
        L.check(L.lib.cnmfe_background_ssub(self._ctx, pid, fit_pid, int(ssub), K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord, _p(bb, L.f32p)))

    def reconstruct_background_ssub(self, pid, b0_new_patch, frame0=0, nframes=None):
        info = self._patch[pid]
        nframes = info["T"] - frame0 if nframes is None else int(nframes)
        bn = np.ascontiguousarray(b0_new_patch, dtype=np.float32).ravel()
        out = np.empty((nframes, info["d"]), dtype=np.float32)
        L.check(L.lib.cnmfe_reconstruct_background_ssub(self._ctx, pid, _p(bn, L.f32p), int(frame0), nframes, _p(out, L.f32p), L.HOST))
        return out

    def compute_rss_ssub(self, pid, A_patch, C_patch, b0_new_patch):
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_patch, info["d"]) if A_patch is not None and A_patch.shape[1] else (0, None, None, None)
        cptr, cord, _keep = self._targs(C_patch, K, info["T"])
        bn = np.ascontiguousarray(b0_new_patch, dtype=np.float32).ravel()
        out = C.c_double(0.0)
        L.check(L.lib.cnmfe_compute_rss_ssub(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord, _p(bn, L.f32p), C.byref(out)))
        return float(out.value)

    @staticmethod
    def _dopts(deconv_options, maxIter=10):
        """deconv_options struct of demo_large_data_1p.m:38-43 -> cnmfe_deconv_opts"""
        o = dict(type="ar1", method="foopsi", smin=-5.0, optimize_pars=True, optimize_b=True, max_tau=100.0)
        o.update(deconv_options or {})
        if str(o["type"]).lower() != "ar1" or str(o["method"]).lower() != "foopsi":
            raise NotImplementedError("only deconv_options type='ar1', method='foopsi' is built")
        return L.DeconvOpts(1, 1, float(o["smin"]), float(o.get("lambda", 0.0)), float(o["max_tau"]),
                            int(bool(o["optimize_b"])), int(bool(o["optimize_pars"])), int(o.get("maxIter", maxIter)))

    # ---- the overlap-region stitch on the device (update_temporal_parallel.m:264-286; cnmfe_stitch_* in include/cnmfe.h) ----
    def stitch_begin(self, K, T):
        L.check(L.lib.cnmfe_stitch_begin(self._ctx, int(K), int(T)))
        self._stitch_shape = (int(K), int(T))

    # ---- several patches per context: set the patches' temporal updates up, sweep them together, add each to the stitch (cnmfe_hals_temporal_job) ----
    def hals_temporal_job(self, pid, A_patch, C_patch, maxIter, deconv_options=None, kernel_pars=None):
        """everything of hals_temporal / hals_temporal_deconv up to the Gauss-Seidel sweeps; returns the job number (for stitch_add_job)"""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_patch, info["d"])
        cptr, cord, _keep = self._targs(C_patch, K, info["T"])
        opts = pars = None
        if deconv_options is not None:
            opts = self._dopts(deconv_options)
            pars = np.zeros(K, dtype=np.float32) if kernel_pars is None else np.ascontiguousarray(kernel_pars, dtype=np.float32)
        job = C.c_int32(-1)
        L.check(L.lib.cnmfe_hals_temporal_job(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord, int(maxIter),
                                              None if opts is None else C.byref(opts), _p(pars, L.f32p), C.byref(job)))
        return job.value

    # ---- (f) known footprints: initTemporal.m:156-168 of one patch (cnmfe_init_temporal in include/cnmfe.h) ----
    def init_temporal(self, pid, A_block, iters_plain=10, iters_last=2, deconv_options=None, want=True):
        """the traces of the footprints A_block (d_b x K, BLOCK rows) under the patch's resident W on its resident video: the rough start of
        HALS_temporal.m:34-41, iters_plain plain sweeps and iters_last more (with deconv_options: the in-sweep AR(1) FOOPSI, kernel parameters estimated fresh).
        Returns (C, C_raw, S, kernel_pars, sn, AA); want=False downloads nothing but AA (C_raw and AA stay on the device for stitch_add)."""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_block, info["d_b"])
        T = info["T"]
        opts = None if deconv_options is None else self._dopts(deconv_options)
        Cout = np.empty((K, T), dtype=np.float32) if want else None
        Craw = np.empty((K, T), dtype=np.float32) if want else None
        dec = want and opts is not None
        S = np.empty((K, T), dtype=np.float32) if dec else None
        pars = np.zeros(K, dtype=np.float32) if dec else None
        sn = np.zeros(K, dtype=np.float32) if dec else None
        AA = np.empty(K, dtype=np.float32)
        L.check(L.lib.cnmfe_init_temporal(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), int(iters_plain), int(iters_last),
                                          None if opts is None else C.byref(opts), _p(Cout, L.f32p), _p(Craw, L.f32p), _p(S, L.f32p), _p(pars, L.f32p),
                                          _p(sn, L.f32p), _p(AA, L.f32p), L.ROWMAJOR))
        return Cout, Craw, S, pars, sn, AA

    def init_temporal_lowrank(self, pid, A_block, iters_plain=10, iters_last=2, deconv_options=None, want=True):
        """init_temporal under background_model = 'svd' (initTemporal.m:180-192): the joint least-squares fit of the footprints A_block (d_b x K, BLOCK rows; the
        rows outside the patch are dropped) and the patch's resident b to every frame, then the sweeps from that C on Y - (b f + b0).  The patch's f and b0 are
        replaced (b0 = the pixel mean).  Returns (C, C_raw, S, kernel_pars, sn, AA, f, b0); want=False downloads nothing but AA (C_raw and AA stay on the device
        for stitch_add).  counter('init_temporal_lowrank_video_reads'): the projection passes of the last call (1 unless a 16 x 16 block meets more than 64 columns)."""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_block, info["d_b"])
        T = info["T"]
        opts = None if deconv_options is None else self._dopts(deconv_options)
        Cout = np.empty((K, T), dtype=np.float32) if want else None
        Craw = np.empty((K, T), dtype=np.float32) if want else None
        dec = want and opts is not None
        S = np.empty((K, T), dtype=np.float32) if dec else None
        pars = np.zeros(K, dtype=np.float32) if dec else None
        sn = np.zeros(K, dtype=np.float32) if dec else None
        AA = np.empty(K, dtype=np.float32)
        nb = self.bg_svd_stats(pid)["nb"] if want else 0
        f = np.zeros((nb, T), dtype=np.float64) if want else None
        b0 = np.zeros(info["d"], dtype=np.float64) if want else None
        L.check(L.lib.cnmfe_init_temporal_lowrank(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), int(iters_plain), int(iters_last),
                                                  None if opts is None else C.byref(opts), _p(Cout, L.f32p), _p(Craw, L.f32p), _p(S, L.f32p), _p(pars, L.f32p),
                                                  _p(sn, L.f32p), _p(AA, L.f32p), _p(f, L.f64p), _p(b0, L.f64p), L.ROWMAJOR))
        return Cout, Craw, S, pars, sn, AA, f, b0

    def init_temporal_job(self, pid, A_block, iters_plain=10, iters_last=2, deconv_options=None):
        """init_temporal for several patches per engine: the plain sweeps run at once, the last ones with the other jobs' in temporal_jobs_sweep; returns
        the job number (for stitch_add_job, which adds AA .* C_raw)"""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_block, info["d_b"])
        opts = None if deconv_options is None else self._dopts(deconv_options)
        job = C.c_int32(-1)
        L.check(L.lib.cnmfe_init_temporal_job(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), int(iters_plain), int(iters_last),
                                              None if opts is None else C.byref(opts), None, C.byref(job)))
        return job.value

    def temporal_jobs_sweep(self):
        """level l of EVERY job set up since stitch_begin in one launch (the patches are independent)"""
        L.check(L.lib.cnmfe_temporal_jobs_sweep(self._ctx))

    def stitch_add_job(self, job, ind):
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        L.check(L.lib.cnmfe_stitch_add_job(self._ctx, int(job), ind.size, _p(ind, L.i32p)))

    def stitch_add(self, ind):
        """rows `ind` of the accumulator += aa .* C_raw of the temporal call just made (its result is still on the device)"""
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        L.check(L.lib.cnmfe_stitch_add(self._ctx, ind.size, _p(ind, L.i32p)))

    def stitch_allreduce(self, group):
        """one process per GPU: the all-reduce of the accumulators over the torch.distributed group, in place on the device buffer
        (nccl == RCCL over xGMI).  gloo (CPU test hook with every rank on one device) goes through a host copy."""
        import torch
        import torch.distributed as td
        ptr = L.f32p(); ld = C.c_int64(); sp_ = C.c_void_p()
        nccl = td.get_backend(group) == "nccl"
        K, _ = self._stitch_shape
        if nccl:
            # RCCL: the collective is enqueued with the ENGINE's stream as torch's current stream -- the process group orders its own stream behind and in front
            # of it with events, so neither the additions before it nor the finish after it need the host (two drains of the stream per update until round 3)
            L.check(L.lib.cnmfe_stitch_buffer_stream(self._ctx, C.byref(ptr), C.byref(ld), C.byref(sp_)))
        else:
            L.check(L.lib.cnmfe_stitch_buffer(self._ctx, C.byref(ptr), C.byref(ld)))      # (gloo goes through the host: everything added so far must have landed)
        n = K * ld.value
        if n == 0:
            return

        class _View:                                                    # zero-copy torch view of the engine's accumulator
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (C.cast(ptr, C.c_void_p).value, False), "version": 2}
        # ONE tensor per (address, length), kept: a tensor over a Python object's memory is released through that object's deleter, which needs the GIL -- and the
        # process group's watchdog thread, which drops the last reference of a finished collective's operands, then took the GIL for ~50 ms at a time, every
        # ~100 ms, wherever the main thread happened to be (profiles/r04/forced_collectives.txt: c4 on one rank of RCCL 26 -> 50-58 ms per iteration)
        key = (C.cast(ptr, C.c_void_p).value, n)
        cached = getattr(self, "_stitch_view", None)
        if cached is None or cached[0] != key:
            cached = self._stitch_view = (key, torch.as_tensor(_View(), device="cuda"))
        t = cached[1]
        if nccl:
            ext = torch.cuda.ExternalStream(int(sp_.value), device=torch.device("cuda", torch.cuda.current_device()))
            with torch.cuda.stream(ext):
                # (test hook of the one-rank measurements: honoured on a ONE-rank group only -- with more ranks skipping the reduction would silently return wrong traces)
                if not (os.environ.get("CNMFE_SKIP_STITCH_ALLREDUCE") == "1" and td.get_world_size(group) == 1):
                    td.all_reduce(t, group=group)
            return
        h = t.cpu(); td.all_reduce(h, group=group); t.copy_(h)
        torch.cuda.current_stream().synchronize()                       # the engine continues on its own stream

    def stitch_finish(self, subtract_min, want=True):
        """C_raw = acc ./ aa (aa == 0 -> 1), minus the row minima without deconvolution (:279-286); the result becomes the engine's bound
        trace matrix, and the returned host copy its identity: passing THAT array to later calls costs no upload"""
        K, T = self._stitch_shape
        if want == "lazy" and K > 0:
            out = LazyHostTraces(self, K, T)
            L.check(L.lib.cnmfe_stitch_finish_async(self._ctx, int(bool(subtract_min)), C.cast(out._ptr, L.f32p)))
            self._mark_batch(out)
            self._bound = out
            return out
        if want == "bound" and K > 0:                    # no host copy at all: the caller goes on with the bound matrix (deconv_temporal_bound)
            L.check(L.lib.cnmfe_stitch_finish(self._ctx, int(bool(subtract_min)), None, L.ROWMAJOR))
            self._bound = BoundOnly(K, T)
            return self._bound
        out = np.empty((K, T), dtype=np.float32) if want else None
        L.check(L.lib.cnmfe_stitch_finish(self._ctx, int(bool(subtract_min)), _p(out, L.f32p), L.ROWMAJOR))
        self._bound = out if (want and K > 0) else None
        return out

    def hals_temporal_deconv(self, pid, A_patch, C_patch, maxIter, deconv_options, kernel_pars=None, want_all=True):
        """[C, C_raw, results_deconv] = HALS_temporal(Y, A, C, maxIter, deconv_options): returns
        (C, C_raw, S, sn, kernel_pars, aa).  want_all=False skips the download of C and S (update_temporal_parallel.m:106-110
        only keeps C_raw and aa; two K x T copies over PCIe otherwise)."""
        info = self._patch[pid]
        K, cp, ri, va = _csc(A_patch, info["d"])
        T = info["T"]
        cptr, cord, _keep = self._targs(C_patch, K, T)                   # (the bound matrix or rows of it: no K x T upload, as in hals_temporal)
        Craw = np.empty((K, T), dtype=np.float32) if want_all is not None else None      # want_all=None: nothing but aa comes back (C_raw stays on the device for stitch_add)
        Cout = np.empty((K, T), dtype=np.float32) if want_all else None
        S = np.empty((K, T), dtype=np.float32) if want_all else None
        aa = np.empty(K, dtype=np.float32); sn = np.zeros(K, dtype=np.float32) if want_all is not None else None   # want_all=None: the call returns with the sweeps in flight
        pars = np.zeros(K, dtype=np.float32) if kernel_pars is None else np.ascontiguousarray(kernel_pars, dtype=np.float32).copy()
        opts = self._dopts(deconv_options)
        L.check(L.lib.cnmfe_hals_temporal_deconv(self._ctx, pid, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, cord,
                                                 int(maxIter), C.byref(opts), _p(pars, L.f32p), _p(Cout, L.f32p), _p(Craw, L.f32p),
                                                 _p(S, L.f32p), _p(sn, L.f32p), _p(aa, L.f32p)))
        if want_all is None:                                 # nothing was copied back (the ABI treats kernel_pars as input only then): no stale copies of the inputs
            return None, None, None, None, None, aa
        return Cout, Craw, S, sn, pars, aa

    def deconv_temporal(self, C_raw, deconv_options, overwrite=False):
        """obj.deconvTemporal(): returns (C, C_raw, S, kernel_pars, sn).  The ABI updates C_raw in place (ck_raw - b); overwrite=True
        lets it do that to the caller's array (when that is a C-contiguous float32 one) instead of to a copy."""
        Craw = np.ascontiguousarray(C_raw, dtype=np.float32)
        if not overwrite or not isinstance(C_raw, np.ndarray) or not np.shares_memory(Craw, C_raw):
            # in-place only on the caller's own plain array when it asked for it; anything else (a DeviceTraces' cached host copy, a view
            # np.ascontiguousarray passed through) gets a private copy, so the write never lands in memory somebody else still reads
            if np.shares_memory(Craw, np.asarray(C_raw)):
                Craw = Craw.copy()
        K, T = Craw.shape
        Cout = np.empty_like(Craw); S = np.empty_like(Craw)
        pars = np.zeros(K, dtype=np.float32); sn = np.zeros(K, dtype=np.float32)
        opts = self._dopts(deconv_options)
        L.check(L.lib.cnmfe_deconv_temporal(self._ctx, K, T, _p(Craw, L.f32p), L.ROWMAJOR, C.byref(opts), _p(Cout, L.f32p), _p(S, L.f32p),
                                            _p(pars, L.f32p), _p(sn, L.f32p)))
        return Cout, Craw, S, pars, sn

    def deconv_temporal_bound(self, deconv_options):
        """obj.deconvTemporal() on the engine's BOUND trace matrix (the C_raw that stitch_finish left on the device): returns (C, C_raw, S, kernel_pars, sn) as
        lazy host views (LazyHostTraces: the values arrive in pinned memory behind the kernels, the first read waits for that copy only); C is the
        engine's bound matrix from here on.  No K x T array crosses PCIe before the call returns."""
        K, T = self._bound.shape
        Cout, Craw, S = LazyHostTraces(self, K, T), LazyHostTraces(self, K, T), LazyHostTraces(self, K, T)
        pars, sn = LazyHostTraces(self, 1, K), LazyHostTraces(self, 1, K)
        opts = self._dopts(deconv_options)
        L.check(L.lib.cnmfe_deconv_temporal_bound(self._ctx, C.byref(opts), C.cast(Cout._ptr, L.f32p), C.cast(Craw._ptr, L.f32p), C.cast(S._ptr, L.f32p),
                                                  C.cast(pars._ptr, L.f32p), C.cast(sn._ptr, L.f32p)))
        self._mark_batch(Cout, Craw, S, pars, sn)
        self._bound = Cout
        self._res = (Cout, Craw, S)                       # C_raw - b and S stay in the context beside the bound C: what the merge entry points read
        return Cout, Craw, S, pars, sn

    # ---- merging (cnmfe.h section (h)): the K x T side of merge_high_corr / merge_neurons_dist_corr / merge_close_neighbors / tag_neurons_parallel ----
    # The context's RESIDENT matrices (C bound, C_raw and S beside it) are known to this wrapper by the identity of the host objects that stand for them, like the
    # bound matrix: _res = (C, C_raw, S or None), valid while C is still the bound one.
    def residents_are(self, Cm, C_raw, S):
        r = getattr(self, "_res", None)
        return (r is not None and Cm is not None and r[0] is getattr(self, "_bound", None) and Cm is r[0] and C_raw is r[1] and S is r[2])

    def traces_load(self, Cm, C_raw=None, S=None, kernel_pars=None):
        """the caller's C, C_raw (None: C), S (None: none) and kernel_pars become the context's matrices (cnmfe_traces_load): two or three K x T uploads"""
        K, T = Cm.shape
        if K == 0:
            self._res = None
            return
        c = _traces(Cm, K, T)
        r = c if (C_raw is None or C_raw is Cm) else _traces(C_raw, K, T)
        s_ = None if S is None else _traces(S, K, T)
        kp = None if kernel_pars is None else np.ascontiguousarray(np.asarray(kernel_pars, dtype=np.float32).ravel())
        if kp is not None and kp.size != K:
            kp = None
        L.check(L.lib.cnmfe_traces_load(self._ctx, K, T, _p(c, L.f32p), _p(r, L.f32p), _p(s_, L.f32p), _p(kp, L.f32p), L.ROWMAJOR))
        self._bound = Cm
        self._res = (Cm, Cm if C_raw is None else C_raw, S)

    def _tsrc(self, X):
        """(pointer, source, K, T, keep-alive) of a trace source: the bound matrix, a resident, the last trace_diff_spikes ("diff"), or a host matrix"""
        r = getattr(self, "_res", None)
        live = r is not None and r[0] is getattr(self, "_bound", None)
        if isinstance(X, str) and X == "diff":
            K, T = self._diff_shape
            return None, L.RES_DIFF, K, T, None
        K, T = X.shape
        if K and X is getattr(self, "_bound", None):
            return None, L.BOUND, K, T, None
        if K and live and X is r[1]:
            return None, L.RES_CRAW, K, T, None
        if K and live and r[2] is not None and X is r[2]:
            return None, L.RES_S, K, T, None
        a = _traces(X, K, T)
        return _p(a, L.f32p), L.ROWMAJOR, K, T, a

    def trace_corr(self, X, raw=False):
        """corr(X') (raw: X X') of a K x T trace matrix as K x K float64 -- no upload when X is the bound matrix, a resident, or "diff" """
        ptr, src, K, T, _keep = self._tsrc(X)
        out = np.empty((K, K), dtype=np.float64)
        L.check(L.lib.cnmfe_trace_corr(self._ctx, K, T, ptr, src, int(bool(raw)), _p(out, L.f64p)))
        return out

    def trace_energy(self, X):
        """sum(X.^2, 2) of a K x T trace matrix as K float64 (update_spatial_batch.m:29) -- no upload when X is the bound matrix, a resident, or "diff" """
        ptr, src, K, T, _keep = self._tsrc(X)
        out = np.zeros(K, dtype=np.float64)
        L.check(L.lib.cnmfe_trace_energy(self._ctx, K, T, ptr, src, _p(out, L.f64p)))
        return out

    def traces_grow(self, K_new):
        """[C; zeros(K_new - K, T)] of the bound matrix and, while they belong to it, of the residents C_raw / S (kernel_pars, sn: zeros appended), on the device
        (cnmfe_traces_grow).  Returns (C, C_raw, S): the host objects that stand for the grown matrices from here on -- GrownTraces over the old ones, whose values stay
        valid; C_raw / S are None when the context holds no residents (or no S) for the bound matrix.  K_new == K returns the objects as they are."""
        old = getattr(self, "_bound", None)
        r = getattr(self, "_res", None)
        live = r is not None and old is not None and r[0] is old
        L.check(L.lib.cnmfe_traces_grow(self._ctx, int(K_new)))            # (refuses when nothing is bound, or K_new < K)
        if old is None:                                                     # (bound through the C ABI behind this wrapper's back: no host object to stand for)
            return None, None, None
        if int(K_new) == old.shape[0]:
            return old, (r[1] if live else None), (r[2] if live else None)
        new = GrownTraces(old, K_new)
        self._bound = new
        if not live:
            return new, None, None
        raw = new if r[1] is old else GrownTraces(r[1], K_new)
        s_ = None if r[2] is None else GrownTraces(r[2], K_new)
        self._res = (new, raw, s_)
        return new, raw, s_

    def trace_diff_spikes(self, X, want=False):
        """merge_high_corr.m:57-66 without S: the thresholded difference traces stay on the device as the source "diff"; want=True also returns (sn, S_)"""
        ptr, src, K, T, _keep = self._tsrc(X)
        sn = np.zeros(K, dtype=np.float32) if want else None
        S_ = np.zeros((K, T), dtype=np.float32) if want else None
        L.check(L.lib.cnmfe_trace_diff_spikes(self._ctx, K, T, ptr, src, _p(sn, L.f32p), _p(S_, L.f32p)))
        self._diff_shape = (K, T)
        return (sn, S_) if want else "diff"

    def trace_tags(self):
        """per trace of the context's C, C_raw, S: [max(C), std(C_raw - C), GetSn(C_raw), |{S(2:end) > 0}|] as K x 4 float64 (cnmfe_trace_tags)"""
        K = self._res[0].shape[0]
        out = np.empty((K, 4), dtype=np.float64)
        L.check(L.lib.cnmfe_trace_tags(self._ctx, K, _p(out, L.f64p)))
        return out

    def merge_apply(self, groups, weights, keep, deconv_options=None):
        """cnmfe_merge_apply on the context's matrices: groups / weights = lists of row-index / float64 arrays (a group's first row receives the merged trace),
        keep = the rows that stay.  Returns the new (C, C_raw, S or None, kernel_pars, sn) as host arrays; C is the bound matrix, the others the residents."""
        had_s = self._res[2] is not None
        T = self._res[0].shape[1]
        keep = np.ascontiguousarray(keep, dtype=np.int32)
        gptr = np.zeros(len(groups) + 1, dtype=np.int32)
        for i, g in enumerate(groups):
            gptr[i + 1] = gptr[i] + len(g)
        gidx = np.ascontiguousarray(np.concatenate([np.asarray(g) for g in groups]) if groups else np.zeros(0), dtype=np.int32)
        w = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64) for x in weights]) if groups else np.zeros(0), dtype=np.float64)
        opts = self._dopts(deconv_options) if groups else None
        n = keep.size
        Cn, Rn = np.empty((n, T), dtype=np.float32), np.empty((n, T), dtype=np.float32)
        Sn = np.empty((n, T), dtype=np.float32) if had_s else None
        kp, sn = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        L.check(L.lib.cnmfe_merge_apply(self._ctx, len(groups), _p(gptr, L.i32p), _p(gidx, L.i32p), _p(w, L.f64p), n, _p(keep, L.i32p),
                                        None if opts is None else C.byref(opts), _p(Cn, L.f32p), _p(Rn, L.f32p), _p(Sn, L.f32p), _p(kp, L.f32p), _p(sn, L.f32p)))
        self._bound = Cn if n else None
        self._res = (Cn, Rn, Sn) if n else None
        return Cn, Rn, Sn, kp, sn

    # ---- dF/F (cnmfe.h section (i)): extract_DF_F_endoscope without the d x T background (Sources2D.m:540-570) ----
    def df_begin(self, K, T):
        """the K x T float64 accumulator of Yf = (A ./ sum(A.^2, 1))' * Ybg, zeroed (cnmfe_df_begin)"""
        L.check(L.lib.cnmfe_df_begin(self._ctx, int(K), int(T)))

    @staticmethod
    def _df_a(A, nrow, ind):
        Km, cp, ri, va = _csc(A, nrow)
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        if ind.size != Km:
            raise ValueError("%d accumulator rows for %d columns of A" % (ind.size, Km))
        return Km, cp, ri, va, ind

    def df_add_frames(self, Ybg, frame0, A, ind):
        """acc[ind, frame0 + t] += A' * Ybg[t]: Ybg (nframes, d) float32 (frame-major), A d x len(ind) sparse (cnmfe_df_add_frames)"""
        Y = np.ascontiguousarray(Ybg, dtype=np.float32)
        n, d = Y.shape
        Km, cp, ri, va, ind = self._df_a(A, d, ind)
        L.check(L.lib.cnmfe_df_add_frames(self._ctx, d, int(frame0), n, Y.ctypes.data_as(C.c_void_p), L.HOST, Km, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p),
                                          _p(ind, L.i32p)))

    def df_add_background(self, pid, b0_block, b0_new_patch, A_patch, ind):
        """the same for all frames of one patch, the background taken from the resident residual of (A_prev, C_prev) as reconstruct_background takes it"""
        info = self._patch[pid]
        Km, cp, ri, va, ind = self._df_a(A_patch, info["d"], ind)
        bb = np.ascontiguousarray(b0_block, dtype=np.float32).ravel(); bn = np.ascontiguousarray(b0_new_patch, dtype=np.float32).ravel()
        if bb.size != info["d_b"] or bn.size != info["d"]:
            raise ValueError("b0_block / b0_new have %d / %d entries, expected %d / %d" % (bb.size, bn.size, info["d_b"], info["d"]))
        L.check(L.lib.cnmfe_df_add_background(self._ctx, pid, _p(bb, L.f32p), _p(bn, L.f32p), Km, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), _p(ind, L.i32p)))

    def df_add_background_ssub(self, pid, b0_new_patch, A_patch, ind):
        """bg_ssub > 1: after background_ssub of that patch, as reconstruct_background_ssub takes it"""
        info = self._patch[pid]
        Km, cp, ri, va, ind = self._df_a(A_patch, info["d"], ind)
        bn = np.ascontiguousarray(b0_new_patch, dtype=np.float32).ravel()
        if bn.size != info["d"]:
            raise ValueError("b0_new has %d entries, expected %d" % (bn.size, info["d"]))
        L.check(L.lib.cnmfe_df_add_background_ssub(self._ctx, pid, _p(bn, L.f32p), Km, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), _p(ind, L.i32p)))

    def df_dims(self):
        K = C.c_int32(0); T = C.c_int64(0)
        L.check(L.lib.cnmfe_df_dims(self._ctx, C.byref(K), C.byref(T)))
        return K.value, T.value

    def df_close(self):
        """drop an open accumulator (a finish without outputs); nothing happens when none is open"""
        K = C.c_int32(0); T = C.c_int64(0)
        if L.lib.cnmfe_df_dims(self._ctx, C.byref(K), C.byref(T)) != 0:
            return
        inv = np.ones(max(K.value, 1), dtype=np.float64)
        L.lib.cnmfe_df_finish(self._ctx, _p(inv, L.f64p), 50.0, 0, None, L.ROWMAJOR, None, L.ROWMAJOR, None, None, None, None)

    def df_fetch(self):
        """the accumulator as a K x T float64 array"""
        K, T = self.df_dims()
        out = np.empty((K, T), dtype=np.float64)
        L.check(L.lib.cnmfe_df_fetch(self._ctx, _p(out, L.f64p)))
        return out

    def df_load(self, Yf):
        """a K x T float64 array becomes the accumulator (opens one if none is open)"""
        Yf = np.ascontiguousarray(Yf, dtype=np.float64)
        L.check(L.lib.cnmfe_df_load(self._ctx, Yf.shape[0], Yf.shape[1], _p(Yf, L.f64p)))

    def df_finish(self, inv_norm, df_prctile, df_window, Cm, C_raw, want_Yf=False):
        """scale by inv_norm = 1 / sum(A.^2, 1) (float64), take the baseline, divide: (C_df, C_raw_df, Df[, Yf]); Df is (K,) without a window, (K, T) with one.
        Cm / C_raw that are the engine's bound matrix / resident C_raw are read where they lie (no upload)."""
        K, T = self.df_dims()
        inv = np.ascontiguousarray(inv_norm, dtype=np.float64).ravel()
        if inv.size != K:
            raise ValueError("inv_norm has %d entries, expected %d" % (inv.size, K))
        w = 0 if df_window is None else int(df_window)
        win = 0 < w <= T
        cptr, csrc, _, _, _k1 = self._tsrc(Cm) if K else (None, L.ROWMAJOR, 0, T, None)
        rptr, rsrc, _, _, _k2 = self._tsrc(C_raw) if K else (None, L.ROWMAJOR, 0, T, None)
        if K and (tuple(Cm.shape) != (K, T) or tuple(C_raw.shape) != (K, T)):
            raise ValueError("C / C_raw are not %d x %d" % (K, T))
        C_df = np.empty((K, T), dtype=np.float32); R_df = np.empty((K, T), dtype=np.float32)
        Df = np.empty((K, T) if win else (K,), dtype=np.float64)
        Yf = np.empty((K, T), dtype=np.float64) if want_Yf else None
        L.check(L.lib.cnmfe_df_finish(self._ctx, _p(inv, L.f64p), float(df_prctile), w, cptr, csrc, rptr, rsrc, _p(C_df, L.f32p), _p(R_df, L.f32p), _p(Df, L.f64p),
                                      _p(Yf, L.f64p)))
        return (C_df, R_df, Df, Yf) if want_Yf else (C_df, R_df, Df)

    # ---- closing calls (cnmfe.h section (f)): orderROIs' statistics and the panels of show_demixed_video ----
    def trace_order_stats(self):
        """per trace of the context's C, C_raw: [mean(C), var(C), var(C_raw - C), max(C), ||C_raw||_2, ||C_raw||_1, max(C_raw)] as K x 7 float64
        (cnmfe_trace_order_stats)"""
        K = self._res[0].shape[0]
        out = np.empty((K, 7), dtype=np.float64)
        L.check(L.lib.cnmfe_trace_order_stats(self._ctx, K, _p(out, L.f64p)))
        return out

    def _demix_traces(self, CC, ind, Ksel, T):
        """(pointer, source, rows, keep-alive) of the traces of a demix call: CC as the bound matrix / the resident C_raw with the rows `ind`, or CC[ind] from the host"""
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        if Ksel == 0:
            return None, L.ROWMAJOR, None, None
        r = getattr(self, "_res", None)
        live = r is not None and r[0] is getattr(self, "_bound", None)
        if CC is getattr(self, "_bound", None):
            return None, L.BOUND, ind, None
        if live and CC is r[1]:
            return None, L.RES_CRAW, ind, None
        a = _traces(np.asarray(CC)[ind], Ksel, T)
        return _p(a, L.f32p), L.ROWMAJOR, None, a

    def demix_frames(self, pid, b0_block, b0_new_patch, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes, want=None, _lowrank=False):
        """the six panels of show_demixed_video for the displayed frames frame0 + j stride (0-based), j < nframes, of one patch (cnmfe_demix_frames; b0_block = None:
        cnmfe_demix_frames_ssub, after background_ssub).  A_patch: d x Ksel over the patch rows, ind: its columns' rows in CC (K x T; the bound matrix and the resident
        C_raw are read where they lie), col: Ksel x 3.  Returns a dict of (nframes, d) float32 arrays raw, bg, signal, denoised, residual and mixed (3, nframes, d)
        uint16; want: the names to compute (default all)."""
        info = self._patch[pid]
        d, T = info["d"], info["T"]
        Ksel, cp, ri, va = _csc(A_patch, d) if A_patch is not None and A_patch.shape[1] else (0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        ind = np.zeros(0, np.int32) if ind is None else np.asarray(ind)
        if ind.size != Ksel:
            raise ValueError("%d trace rows for %d columns of A" % (ind.size, Ksel))
        col = np.ascontiguousarray(col, dtype=np.float32).reshape(-1, 3)
        if col.shape[0] != Ksel:
            raise ValueError("col is %s, expected (%d, 3)" % (col.shape, Ksel))
        cptr, csrc, rows, _keep = self._demix_traces(CC, ind, Ksel, T)
        if _lowrank:
            head, fn = (self._ctx, pid), L.lib.cnmfe_demix_frames_lowrank
        else:
            bn = np.ascontiguousarray(b0_new_patch, dtype=np.float32).ravel()
            bb = None if b0_block is None else np.ascontiguousarray(b0_block, dtype=np.float32).ravel()
            if bn.size != d or (bb is not None and bb.size != info["d_b"]):
                raise ValueError("b0_block / b0_new do not have the block's / the patch's size")
            head = (self._ctx, pid) + (() if bb is None else (_p(bb, L.f32p),)) + (_p(bn, L.f32p),)
            fn = L.lib.cnmfe_demix_frames_ssub if bb is None else L.lib.cnmfe_demix_frames
        nframes = int(nframes)
        names = ("raw", "bg", "signal", "denoised", "residual", "mixed") if want is None else tuple(want)
        n = max(nframes, 0)
        out = {k: np.zeros((n, d), dtype=np.float32) for k in names if k != "mixed"}
        if "mixed" in names:
            out["mixed"] = np.zeros((3, n, d), dtype=np.uint16)
        ptr = lambda k: _p(out[k], L.f32p) if k in out and out[k].size else None       # (zero frames: NULL, nothing is written)
        mix = out["mixed"].ctypes.data_as(L.u16p) if "mixed" in out and out["mixed"].size else None
        L.check(fn(*head, Ksel, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), cptr, csrc, _p(rows, L.i32p) if rows is not None else None,
                   _p(col, L.f32p), float(mix_scale), int(frame0), int(stride), nframes, ptr("raw"), ptr("bg"), ptr("signal"), ptr("denoised"), ptr("residual"), mix, L.HOST))
        return out

    def demix_frames_lowrank(self, pid, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes, want=None):
        """demix_frames under the svd model (cnmfe_demix_frames_lowrank): bg = b0 + b f from the patch's resident factors, no b0 argument and no residual"""
        return self.demix_frames(pid, None, None, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes, want, _lowrank=True)

    def _mark_batch(self, *lazies):
        """the asynchronous call just made queued one batch of downloads: its generation number goes to the buffers it fills"""
        g = C.c_int64(0)
        L.check(L.lib.cnmfe_copy_generation(self._ctx, C.byref(g)))
        for x in lazies:
            blk = x._blk()
            if blk is not None:
                blk.gen = g.value

    def post_process_spatial(self, A_full, d1, d2):
        K, cp, ri, va = _csc(A_full, d1 * d2)
        keep = np.zeros(cp[-1], dtype=np.uint8)
        L.check(L.lib.cnmfe_post_process_spatial(self._ctx, d1, d2, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), _p(keep, L.u8p)))
        out = sp.csc_matrix((va * keep, ri.copy(), cp.copy()), shape=(d1 * d2, K))
        out.eliminate_zeros()
        return out

    # ---- image operations on single footprints (include/cnmfe.h, "footprint image operations") -----------------------
    @staticmethod
    def _box_cells(box, off, K, d1):
        """(column, pixel) of every cell of the boxes, in the order of the device's result: column after column, column-major inside a box"""
        h = box[:, 2].astype(np.int64)
        col = np.repeat(np.arange(K), (off[1:] - off[:-1]))
        loc = np.arange(int(off[K]), dtype=np.int64) - off[col]
        hc = h[col]
        return col, (box[col, 1] + loc // hc) * d1 + box[col, 0] + loc % hc

    @staticmethod
    def _splice(out, host, sel, shape, dtype):
        """`out` with the columns `sel`, empty so far, taken from `host` (the same columns computed by hostops)"""
        host = sp.coo_matrix(host)
        add = sp.csc_matrix((host.data.astype(dtype), (host.row, sel[host.col])), shape=shape)
        out = sp.csc_matrix(out + add, dtype=dtype)
        out.sort_indices()
        return out

    def _boxed(self, fn, head, tail, K, d1, out_dtype, out_ptr):
        """the two calls of a boxed operation: the sizes, then the result"""
        box = np.zeros((max(K, 1), 4), dtype=np.int32); off = np.zeros(K + 1, dtype=np.int64); host_col = np.zeros(max(K, 1), dtype=np.uint8)
        none = C.cast(None, out_ptr)
        L.check(fn(*head, *tail, _p(box, L.i32p), _p(off, L.i64p), none, 0, _p(host_col, L.u8p), L.HOST))
        out = np.zeros(int(off[K]), dtype=out_dtype)
        if out.size:
            L.check(fn(*head, *tail, _p(box, L.i32p), _p(off, L.i64p), _p(out, out_ptr), out.size, _p(host_col, L.u8p), L.HOST))
        col, pix = self._box_cells(box[:K], off, K, d1)
        nz = np.flatnonzero(out)
        return col[nz], pix[nz], out[nz], np.flatnonzero(host_col[:K])

    def circular_constraints(self, A_full, d1, d2):
        """circular_constraints (endoscope/circular_constraints.m:8-55) of every column of the d1*d2 x K matrix: what hostops.circular_constraints_columns
        returns, as float32.  A column whose bounding box has more than IMAGE_OPS_MAX_BOX cells is computed there (counter image_ops_host_columns)."""
        from . import hostops
        A_full = sp.csc_matrix(A_full)
        K, cp, ri, va = _csc(A_full, d1 * d2)
        col, pix, val, sel = self._boxed(L.lib.cnmfe_circular_constraints, (self._ctx, d1, d2, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p)), (), K, d1,
                                         np.float32, L.f32p)
        out = sp.csc_matrix((val, pix, np.concatenate([[0], np.cumsum(np.bincount(col, minlength=K))])), shape=(d1 * d2, K))
        if sel.size:
            out = self._splice(out, hostops.circular_constraints_columns(A_full[:, sel].astype(np.float32), d1, d2), sel, out.shape, np.float32)
        return out

    def search_dilate(self, A_full, d1, d2, se, nb=1, nrgthr=0.99):
        """IND = determine_search_location(A, 'dilate', ...) with the structuring element `se`: what hostops.search_location_dilate returns"""
        from . import hostops
        A_full = sp.csc_matrix(A_full)
        K, cp, ri, va = _csc(A_full, d1 * d2)
        se8 = np.ascontiguousarray(np.atleast_2d(np.asarray(se, dtype=bool)), dtype=np.uint8)
        col, pix, val, sel = self._boxed(L.lib.cnmfe_search_dilate, (self._ctx, d1, d2, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p)),
                                         (_p(se8, L.u8p), se8.shape[0], se8.shape[1], int(nb), float(nrgthr)), K, d1, np.uint8, L.u8p)
        out = sp.csc_matrix((np.ones(pix.size, dtype=bool), pix, np.concatenate([[0], np.cumsum(np.bincount(col, minlength=K))])), shape=(d1 * d2, K))
        if sel.size:
            # (the rule for the last nb columns counts from the end of the WHOLE matrix)
            host = sp.hstack([hostops.search_location_dilate(A_full[:, [k]].astype(np.float32), d1, d2, se, 1 if k >= K - nb else 0, nrgthr) for k in sel], format="csc")
            out = self._splice(out, host, sel, out.shape, bool)
        return out

    def trim_spatial(self, A_full, d1, d2, thr=0.01, sz=5, min_pixel=0):
        """trimSpatial (@Sources2D/Sources2D.m:942-965): (the trimmed matrix as float32, ind_small) -- what hostops.trim_spatial returns"""
        from . import hostops
        sz = int(sz)
        if sz < 1 or sz > 9 or sz % 2 == 0:
            raise ValueError("trim_spatial: sz = %d; the square's side is odd, 1 .. 9" % sz)
        A_full = sp.csc_matrix(A_full)
        K, cp, ri, va = _csc(A_full, d1 * d2)
        keep = np.ones(cp[-1], dtype=np.uint8); small = np.zeros(max(K, 1), dtype=np.uint8); host_col = np.zeros(max(K, 1), dtype=np.uint8)
        L.check(L.lib.cnmfe_trim_spatial(self._ctx, d1, d2, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), float(thr), sz, int(min_pixel), _p(keep, L.u8p),
                                         _p(small, L.u8p), _p(host_col, L.u8p), L.HOST))
        out = sp.csc_matrix((va * keep, ri.copy(), cp.copy()), shape=(d1 * d2, K))
        out.eliminate_zeros()
        small = small[:K].astype(bool)
        sel = np.flatnonzero(host_col[:K])
        if sel.size:
            hA, hs = hostops.trim_spatial(A_full[:, sel].astype(np.float32), d1, d2, thr, sz, min_pixel)
            keep_cols = np.ones(K, dtype=np.float32); keep_cols[sel] = 0
            out = self._splice(out @ sp.diags(keep_cols), hA, sel, out.shape, np.float32)
            out.eliminate_zeros()
            small[sel] = hs
        return out, small

    # ---- measurement ---------------------------------------------------------------
    def profile(self, on=True):
        """True / 1: events around every kernel; 2: only around the roofline kernels (cnmfe.h); False: off"""
        L.check(L.lib.cnmfe_profile_enable(self._ctx, int(on)))

    def profile_reset(self):
        L.check(L.lib.cnmfe_profile_reset(self._ctx))

    def profile_table(self):
        n = L.lib.cnmfe_profile_count(self._ctx)
        out = {}
        for i in range(n):
            name = C.create_string_buffer(128); ms = C.c_double(); calls = C.c_int64()
            L.check(L.lib.cnmfe_profile_get(self._ctx, i, name, 128, C.byref(ms), C.byref(calls)))
            out[name.value.decode()] = dict(total_ms=ms.value, calls=calls.value)
        return out

    def synchronize(self):
        L.check(L.lib.cnmfe_synchronize(self._ctx))

    def set_option(self, name, value):
        L.check(L.lib.cnmfe_set_option(self._ctx, name.encode(), int(value)))
        self._opts_set[name] = int(value)

    def temporal_early_claim(self, token):
        """the A of the next hals_temporal IS the spatial result `token` was given for: it may start from the projection queued then"""
        if token and hasattr(L.lib, "cnmfe_temporal_early_claim"):
            L.check(L.lib.cnmfe_temporal_early_claim(self._ctx, int(token)))

    def counter(self, name):
        """a read-only counter of the library (cnmfe_get_option: temporal_early_hits, temporal_early_drops, temporal_nowait, ...)"""
        v = C.c_int64(0)
        L.check(L.lib.cnmfe_get_option(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def get_option(self, name, default):
        """the value this engine's option has: what set_option gave it last, else what CNMFE_OPTS preset at cnmfe_create, else `default` (the library's own)"""
        if name in self._opts_set:
            return self._opts_set[name]
        for kv in os.environ.get("CNMFE_OPTS", "").split(","):
            k, _, v = kv.partition("=")
            if k == name and v:
                try:
                    return int(v)
                except ValueError:
                    pass
        return default
