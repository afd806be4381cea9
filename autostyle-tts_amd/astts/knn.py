"""Style bank resident in HBM + brute-force kNN -- COSINE (the reference's collection), IP, L2 -- (host side of astts_knn_*).

This is the engine under the ``MilvusClient.search`` shim (astts/compat/pymilvus.py).  It
replaces what the reference gets from milvus-lite for
/root/reference/milvus/search_embeddings.py:15-22 and /root/reference/src/search_milvus.py:140-147.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib, _lib_knn, _lib_knn_grouped, _lib_knn_ivf


KNN_SCANS = ("DIRECT", "REGISTER", "GEMM", "GEMM_BLOCKS", "GEMM_N_FIRST")      # ASTTS_KNN_SCAN_*
KNN_FINISHES = ("FUSED", "BLOCKS", "STREAM", "SELECT", "SELECT_MERGE")       # ASTTS_KNN_FINISH_*


def _route_groups(n: int, d: int, nq: int, k: int, masked: bool, aligned: bool):
    lib = _lib.load()
    rows, scan, finish, passes = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    done = group = 0
    while done < nq or group == 0:      # (a shape the library refuses raises on group 0)
        _lib.check(lib.astts_knn_route(n, d, nq, k, 1 if masked else 0, 1 if aligned else 0, group, ctypes.byref(rows), ctypes.byref(scan),
                                       ctypes.byref(finish), ctypes.byref(passes)))
        yield rows.value, KNN_SCANS[scan.value], KNN_FINISHES[finish.value], passes.value
        done += rows.value
        group += 1


def route(n: int, d: int, nq: int, k: int, masked: bool = False, aligned: bool = True):
    """The launches a search of ``nq`` queries for ``k`` hits against an ``n x d`` bank takes, as the launcher itself decides them
    (astts_knn_route: a host query, no GPU call): one ``(rows, scan, finish)`` per query group, names from KNN_SCANS / KNN_FINISHES.
    ``masked``: with a row mask; ``aligned``: the queries at a 16-byte aligned address (every torch allocation is)."""
    return [g[:3] for g in _route_groups(n, d, nq, k, masked, aligned)]


def route_passes(n: int, d: int, nq: int, k: int) -> int:
    """Selection + re-score passes of that search over one scan per query group: ``ceil(k / 32)`` when ``k > 32``, else 1."""
    return next(_route_groups(n, d, nq, k, False, True))[3]


def _require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("astts.knn needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback in the product path")


# ---- what every search form shares: queries, outputs, row mask, workspace, host conversion
def _as_queries(queries: torch.Tensor, d: int, device: torch.device) -> torch.Tensor:
    """``queries`` as the ABI takes them: fp32, contiguous ``[Q, d]`` on ``device`` (a tensor that already is, is passed as is)."""
    if queries.dim() != 2 or queries.shape[1] != d:
        raise ValueError(f"queries must be [Q, {d}], got {tuple(queries.shape)}")
    if queries.dtype != torch.float32 or queries.device != device or not queries.is_contiguous():
        return queries.to(device=device, dtype=torch.float32).contiguous()
    return queries


def _outputs(nq: int, columns: int, return_f64: bool, device: torch.device, out_idx=None, out_score=None):
    """-> (idx int64, score fp32, score fp64 or None), each ``[nq, columns]`` on ``device``; a caller's ``out_idx`` / ``out_score``
    are used in place of new ones (an empty search returns new empties)."""
    if out_idx is None or nq == 0:
        out_idx = torch.empty((nq, columns), dtype=torch.int64, device=device)
    if out_score is None or nq == 0:
        out_score = torch.empty((nq, columns), dtype=torch.float32, device=device)
    return out_idx, out_score, torch.empty((nq, columns), dtype=torch.float64, device=device) if return_f64 else None


def _row_mask(row_mask: Optional[torch.Tensor], nq: int, n: int, device: torch.device):
    """-> (the uint8 mask on ``device`` -- to be kept referenced across the call --, its pointer, its stride per query): ``[n]`` is one
    mask for every query (stride 0), ``[nq, n]`` one per query (stride ``n``); without a mask (None, None, 0)."""
    if row_mask is None:
        return None, None, 0
    m = row_mask.to(device=device)
    m = (m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)).contiguous()
    if m.shape != (n,) and m.shape != (nq, n):
        raise ValueError(f"row_mask must be [{n}] or [{nq}, {n}], got {tuple(m.shape)}")
    return m, m.data_ptr(), 0 if m.dim() == 1 else n


class _Workspace:
    """The device buffer one search form works in: it grows to the largest search seen, and the calls get its 256-byte aligned
    base and the bytes behind it.  Nothing outside holds a pointer into it, so replacing the buffer leaves nothing stale."""

    def __init__(self, device: torch.device):
        self.device = device
        self.buf: Optional[torch.Tensor] = None
        self.base = self.nbytes = 0
        self.fits = set()                            # the search shapes the buffer is known to hold

    def fit(self, key: tuple, invalid, sizing, *handles):
        """Room for a search of shape ``key``, which needs ``sizing(*handles, *key)`` bytes (asked once per shape; 0: the library
        refuses the shape -> ``ValueError(invalid())``).  -> (aligned base, bytes behind it)."""
        if key not in self.fits:
            need = int(sizing(*handles, *key))
            if need == 0:
                raise ValueError(invalid())
            if self.buf is None or self.buf.numel() < need + 256:      # (+ 256: the aligned part holds ``need`` wherever the buffer starts)
                self.buf = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
                start = self.buf.data_ptr()
                self.base = (start + 255) // 256 * 256
                self.nbytes = self.buf.numel() - (self.base - start)
            self.fits.add(key)
        return self.base, self.nbytes

    def forget(self) -> None:
        """The sizes are per (rows, tombstone state, index): ask again, keep the buffer."""
        self.fits.clear()


def _host_inputs(queries, row_mask, device: torch.device):
    """numpy / lists -> (queries fp32 ``[Q, D]`` on ``device`` -- one ``[D]`` vector is one query --, row mask uint8 tensor or None)."""
    q = torch.as_tensor(np.asarray(queries, dtype=np.float32))
    if q.dim() == 1:
        q = q[None, :]
    if row_mask is not None and not isinstance(row_mask, torch.Tensor):
        row_mask = torch.from_numpy(np.ascontiguousarray(np.asarray(row_mask) != 0).astype(np.uint8))
    return q.to(device), row_mask


class StyleBank:
    """``N x D`` style-embedding bank held on one GPU.

    ``vectors``: numpy / torch array ``[N, D]`` (fp16 or fp32).  Row index == style id.

    The bank can change while it stays on the GPU (include/knn/astts_knn_mutable.h): ``append`` packs the new rows behind the old ones
    (cost O(new rows); a grown bank returns bit for bit what a bank created at once from the same rows returns), ``delete_rows``
    tombstones rows (no search returns them; row indices stay), ``compact`` squeezes the tombstones out and renumbers.  ``n`` rows,
    ``live`` of them not deleted, ``capacity`` rows allocated.  None of these may run while a search of this bank is in flight on
    another stream or thread.

    ``build_index`` adds an IVF_FLAT index (include/knn/astts_knn_ivf.h): ``search_ivf`` / ``search_ivf_device`` then return the exact
    answer over the rows of the ``nprobe`` lists closest to each query.  ``search`` / ``search_device`` stay the brute-force search.
    With an index present ``append`` assigns the new rows to their lists and ``compact`` renumbers the lists; ``delete_rows`` needs
    nothing (the list scan skips tombstones).
    """

    def __init__(self, vectors, device: Optional[torch.device] = None, metric: str = "COSINE"):
        _require_gpu()
        lib = _lib.load()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(vectors, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(vectors))
        else:
            t = vectors
        if t.dim() != 2:
            raise ValueError(f"bank must be [N, D], got {tuple(t.shape)}")
        if t.dtype not in (torch.float16, torch.float32):
            t = t.to(torch.float32)
        metric_id = {"COSINE": _lib.METRIC_COSINE, "IP": _lib.METRIC_IP, "L2": _lib.METRIC_L2}.get(metric.upper())
        if metric_id is None:
            raise ValueError(f"unknown metric {metric!r}")
        with torch.cuda.device(self.device):
            src = t.to(self.device).contiguous()
            h = ctypes.c_void_p()
            _lib.check(lib.astts_knn_create(
                src.data_ptr(), src.shape[0], src.shape[1],
                _lib.DTYPE_F16 if src.dtype == torch.float16 else _lib.DTYPE_F32,
                metric_id, _lib.stream_ptr(), ctypes.byref(h)))
        self._h = h
        self.metric = metric.upper()
        self.d = int(src.shape[1])
        self._index = int(self.device.index)
        self._ws = _Workspace(self.device)           # the plain search's, sized per (nq, k); last_fallbacks reads it
        self._gws = _Workspace(self.device)          # the grouped search's, per (nq, limit, group_size, n_groups)
        self._iws = _Workspace(self.device)          # the IVF search's, per (nq, k, nprobe)
        self.last_rounds = 0                         # rounds the last grouped search took (rounds_host)
        self._ivf = None                             # astts_knn_ivf_t* (build_index)
        self._search, self._search_bytes = lib.astts_knn_search, lib.astts_knn_workspace_bytes
        self._refresh()

    def _refresh(self) -> None:
        """``n``, ``live``, ``capacity`` and ``scan_plane_exact`` from the handle; the workspaces forget which search shapes fit (the sizes are per n and
        tombstone state)."""
        n, live, cap, exact = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        _lib.check(_lib_knn.load().astts_knn_stats(self._h, ctypes.byref(n), ctypes.byref(live), ctypes.byref(cap)))
        _lib.check(_lib.load().astts_knn_info(self._h, None, None, ctypes.byref(exact)))
        self.n, self.live, self.capacity = int(n.value), int(live.value), int(cap.value)
        self.scan_plane_exact = bool(exact.value)
        for ws in (self._ws, self._gws, self._iws):
            ws.forget()

    def _enter(self) -> Optional[int]:
        """Make the bank's device the current one for a call: -> the device to go back to afterwards, None when it was current
        already (the usual case, which then costs one comparison: ``with torch.cuda.device`` is too slow for a 12 us search).  The
        caller restores it in a ``finally``: ``if prev is not None: torch.cuda.set_device(prev)``."""
        prev = torch.cuda.current_device()
        if prev == self._index:
            return None
        torch.cuda.set_device(self._index)
        return prev

    # ---- mutation (each call synchronises the current stream, as the constructor does)
    def reserve(self, capacity: int) -> None:
        """Room for ``capacity`` rows (rounded up to a multiple of 128; never shrinks), so that appends up to it copy nothing."""
        with torch.cuda.device(self.device):
            try:
                _lib.check(_lib_knn.load().astts_knn_reserve(self._h, int(capacity), _lib.stream_ptr()))
            finally:
                self._refresh()

    def append(self, vectors) -> int:
        """``vectors``: numpy / torch ``[M, D]`` (or one ``[D]`` row), fp16 or fp32 -> the row index of the first new row.  fp32 rows
        that are not fp16-exact promote an fp16-exact bank (``scan_plane_exact`` turns False).  Non-finite values raise
        (ASTTS_ERR_RANGE) and leave the bank as it was."""
        t = torch.from_numpy(np.ascontiguousarray(vectors)) if isinstance(vectors, np.ndarray) else torch.as_tensor(vectors)
        if t.dim() == 1:
            t = t[None, :]
        if t.dim() != 2 or t.shape[1] != self.d:
            raise ValueError(f"rows must be [M, {self.d}], got {tuple(t.shape)}")
        if t.dtype not in (torch.float16, torch.float32):
            t = t.to(torch.float32)
        first = ctypes.c_int64()
        with torch.cuda.device(self.device):
            src = t.to(self.device).contiguous()
            try:
                _lib.check(_lib_knn.load().astts_knn_append(self._h, src.data_ptr(), src.shape[0],
                                                            _lib.DTYPE_F16 if src.dtype == torch.float16 else _lib.DTYPE_F32,
                                                            _lib.stream_ptr(), ctypes.byref(first)))
            finally:
                self._refresh()
            if self._ivf is not None:
                _lib.check(_lib_knn_ivf.load().astts_knn_ivf_assign(self._ivf, self._h, _lib.stream_ptr()))
        return int(first.value)

    def delete_rows(self, rows) -> None:
        """Tombstone ``rows`` (indices into the bank): no search returns them.  A row outside ``[0, n)`` raises and deletes nothing;
        deleting a row twice is harmless."""
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        with torch.cuda.device(self.device):
            try:
                _lib.check(_lib_knn.load().astts_knn_set_deleted(self._h, r.ctypes.data, int(r.size), _lib.stream_ptr()))
            finally:
                self._refresh()

    def compact(self) -> np.ndarray:
        """Remove the tombstoned rows; the survivors keep their order.  -> int64 ``[old n]``: the new index of every old row, -1 for
        a removed one.  A bank whose rows are all deleted cannot be compacted (ASTTS_ERR_UNSUPPORTED): close it."""
        old_to_new = np.empty(self.n, dtype=np.int64)
        with torch.cuda.device(self.device):
            try:
                _lib.check(_lib_knn.load().astts_knn_compact(self._h, _lib.stream_ptr(), None, old_to_new.ctypes.data))
            finally:
                self._refresh()
            if self._ivf is not None:
                _lib.check(_lib_knn_ivf.load().astts_knn_ivf_remap(self._ivf, old_to_new.ctypes.data, self.n, _lib.stream_ptr()))
        return old_to_new

    def close(self) -> None:
        if getattr(self, "_ivf", None):
            self.drop_index()
        if getattr(self, "_h", None):
            _lib.load().astts_knn_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def search_device(self, queries: torch.Tensor, k: int, force_exact: bool = False,
                      out_idx: Optional[torch.Tensor] = None, out_score: Optional[torch.Tensor] = None, return_f64: bool = False,
                      row_mask: Optional[torch.Tensor] = None):
        """queries: fp32 ``[Q, D]`` on this bank's GPU.  Returns (idx int64 [Q,k], score fp32 [Q,k])
        on the GPU, enqueued on the current stream (no synchronisation), closest first (COSINE / IP: score descending; L2:
        squared distance ascending; ties by row index).  ``return_f64``: a third tensor with the fp64 scores (what a
        bank-sharded search merges on: astts.parallel.bank_sharded_search).  ``row_mask``: uint8 / bool ``[N]`` (one mask for
        every query) or ``[Q, N]`` on the GPU -- only rows with a non-zero entry can be hits (a Milvus ``filter``)."""
        q = _as_queries(queries, self.d, self.device)
        if not 1 <= k <= _lib.KNN_MAX_K:
            raise ValueError(f"k must be in 1..{_lib.KNN_MAX_K}, got {k}")
        # (a config-2 search is ~12 us of GPU time: the host side of this call is kept to a handful of attribute reads and ONE ctypes
        # call -- the workspace's size is asked once per (queries, k), tensors that already are what the ABI takes are passed as is)
        nq = int(q.shape[0])
        out = _outputs(nq, k, return_f64, self.device, out_idx, out_score)
        out_idx, out_score, s64 = out
        if nq:
            prev = self._enter()
            try:
                base, ws_bytes = self._ws.fit((nq, k), lambda: f"invalid search shape nq={nq} k={k}", self._search_bytes, self._h)
                m, mptr, mstride = _row_mask(row_mask, nq, self.n, self.device)
                rc = self._search(self._h, q.data_ptr(), nq, k, out_idx.data_ptr(), out_score.data_ptr(), None if s64 is None else s64.data_ptr(),
                                  mptr, mstride, base, ws_bytes, _lib.KNN_FORCE_EXACT if force_exact else 0,
                                  torch.cuda.current_stream(self._index).cuda_stream)
                if rc != 0:
                    _lib.check(rc)
            finally:
                if prev is not None:
                    torch.cuda.set_device(prev)
        return out if return_f64 else out[:2]

    def search(self, queries, k: int, force_exact: bool = False, row_mask=None):
        """Host convenience: accepts numpy / lists, returns numpy (idx int64 [Q,k], score fp32 [Q,k])."""
        q, row_mask = _host_inputs(queries, row_mask, self.device)
        idx, sc = self.search_device(q, k, force_exact, row_mask=row_mask)
        return idx.cpu().numpy(), sc.cpu().numpy()

    # ---- grouped and ranged search (include/knn/astts_knn_grouped.h)
    def search_grouped_device(self, queries: torch.Tensor, limit: int, group_size: int = 1, groups: Optional[torch.Tensor] = None,
                              n_groups: Optional[int] = None, radius: Optional[float] = None, range_filter: Optional[float] = None,
                              row_mask: Optional[torch.Tensor] = None, force_exact: bool = False, return_f64: bool = False,
                              max_rounds: int = 0):
        """The ``limit`` groups whose best row is closest, ``group_size`` rows of each, within the range: -> (idx int64, score fp32
        ``[Q, limit * group_size]``) on the GPU (``return_f64``: and the fp64 scores), slot ``g * group_size + j`` = the j-th row of the
        g-th group, -1 / -inf (+inf for L2) where a row or a group is missing.  Ids are exact with respect to the definition in
        include/knn/astts_knn_grouped.h; the scores are bit for bit those of ``search_device``.

        ``queries`` / ``row_mask`` / ``force_exact``: as in ``search_device``.  ``groups``: int32 ``[N]`` on this bank's GPU, the group
        code of every row in ``[0, n_groups)`` (``n_groups``: default ``groups.max() + 1``, which synchronises); ``None``: every row is
        its own group.  ``radius`` / ``range_filter``: COSINE / IP ``radius < score <= range_filter``, L2
        ``range_filter <= distance < radius``.  Runs on the current stream and SYNCHRONISES it once per round (one round when the
        first 32 hits settle every query; ``last_rounds`` tells how many it took; ``max_rounds`` 0 = 64, beyond it the call raises)."""
        q = _as_queries(queries, self.d, self.device)
        limit, group_size = int(limit), int(group_size)
        if limit < 1 or group_size < 1 or limit * group_size > _lib.KNN_MAX_K:
            raise ValueError(f"limit * group_size must be in 1..{_lib.KNN_MAX_K}, got {limit} x {group_size}")
        nq = int(q.shape[0])
        out = _outputs(nq, limit * group_size, return_f64, self.device)
        out_idx, out_score, s64 = out
        self.last_rounds = 0
        if nq:
            lib = _lib_knn_grouped.load()
            prev = self._enter()
            try:
                gptr, ng = None, 1
                if groups is not None:
                    if groups.shape != (self.n,) or groups.dtype != torch.int32 or groups.device != self.device:
                        raise ValueError(f"groups must be int32 [{self.n}] on {self.device}, got {groups.dtype} {tuple(groups.shape)} on {groups.device}")
                    groups = groups.contiguous()
                    ng = int(n_groups) if n_groups is not None else int(groups.max()) + 1
                    gptr = groups.data_ptr()
                base, ws_bytes = self._gws.fit(
                    (nq, limit, group_size, ng if groups is not None else 0),
                    lambda: f"invalid grouped search shape nq={nq} limit={limit} group_size={group_size} n_groups={ng} (n={self.n})",
                    lib.astts_knn_grouped_workspace_bytes, self._h)
                m, mptr, mstride = _row_mask(row_mask, nq, self.n, self.device)
                rad = None if radius is None else ctypes.c_double(float(radius))
                rf = None if range_filter is None else ctypes.c_double(float(range_filter))
                rounds = ctypes.c_int32()
                rc = lib.astts_knn_search_grouped(self._h, q.data_ptr(), nq, limit, group_size, gptr, ng,
                                                  None if rad is None else ctypes.addressof(rad), None if rf is None else ctypes.addressof(rf),
                                                  out_idx.data_ptr(), out_score.data_ptr(), None if s64 is None else s64.data_ptr(),
                                                  mptr, mstride, base, ws_bytes, _lib.KNN_FORCE_EXACT if force_exact else 0, int(max_rounds),
                                                  ctypes.addressof(rounds), torch.cuda.current_stream(self._index).cuda_stream)
                self.last_rounds = int(rounds.value)
                if rc != 0:
                    _lib.check(rc)
            finally:
                if prev is not None:
                    torch.cuda.set_device(prev)
        return out if return_f64 else out[:2]

    def search_grouped(self, queries, limit: int, group_size: int = 1, groups=None, n_groups: Optional[int] = None,
                       radius: Optional[float] = None, range_filter: Optional[float] = None, row_mask=None, force_exact: bool = False,
                       max_rounds: int = 0):
        """Host convenience of ``search_grouped_device``: accepts numpy / lists (``groups``: integer codes ``[N]``, checked to lie in
        ``[0, n_groups)``), returns numpy (idx int64, score fp32 ``[Q, limit * group_size]``)."""
        q, row_mask = _host_inputs(queries, row_mask, self.device)
        if groups is not None and not isinstance(groups, torch.Tensor):
            g = np.ascontiguousarray(np.asarray(groups).reshape(-1).astype(np.int64))
            if n_groups is None:
                n_groups = int(g.max()) + 1 if g.size else 1
            if g.size != self.n or (g.size and (g.min() < 0 or g.max() >= n_groups)):
                raise ValueError(f"groups must be {self.n} codes in [0, {n_groups})")
            groups = torch.from_numpy(g.astype(np.int32)).to(self.device)
        idx, sc = self.search_grouped_device(q, limit, group_size, groups, n_groups, radius, range_filter, row_mask,
                                             force_exact, max_rounds=max_rounds)
        return idx.cpu().numpy(), sc.cpu().numpy()

    # ---- IVF_FLAT index (include/knn/astts_knn_ivf.h)
    def build_index(self, nlist: int, niter: int = _lib_knn_ivf.DEFAULT_NITER, centroids=None) -> dict:
        """Train ``min(nlist, live rows)`` k-means lists over the bank (``niter`` Lloyd iterations from ``centroids`` -- numpy / torch
        fp32 ``[nlist, D]`` -- or, when None, from evenly spaced live rows) and assign every row to its closest centroid; replaces an
        index the bank has.  Deterministic: the same bank and arguments give byte-identical centroids and lists.  ``niter=0`` with
        given centroids is a pure assignment.  Synchronises the current stream.  -> ``index_info()``."""
        nlist, niter = int(nlist), int(niter)
        if not 1 <= nlist <= _lib_knn_ivf.MAX_NLIST or niter < 0:
            raise ValueError(f"nlist must be in 1..{_lib_knn_ivf.MAX_NLIST} and niter >= 0, got nlist={nlist} niter={niter}")
        cptr = None
        if centroids is not None:
            c = centroids.detach().cpu().numpy() if isinstance(centroids, torch.Tensor) else np.asarray(centroids)
            c = np.ascontiguousarray(c, dtype=np.float32)
            if c.shape != (nlist, self.d):
                raise ValueError(f"centroids must be [{nlist}, {self.d}], got {tuple(c.shape)}")
            cptr = c.ctypes.data
        self.drop_index()
        ivf = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib_knn_ivf.load().astts_knn_ivf_create(self._h, nlist, niter, cptr, _lib.stream_ptr(), ctypes.byref(ivf)))
        self._ivf = ivf
        return self.index_info()

    def drop_index(self) -> None:
        if self._ivf is not None:
            _lib_knn_ivf.load().astts_knn_ivf_destroy(self._ivf)
            self._ivf = None
        self._iws.forget()

    def index_info(self) -> Optional[dict]:
        """None without an index, else ``{"index_type": "IVF_FLAT", "nlist", "n_indexed", "max_list_len"}`` (``nlist``: the lists that
        exist, ``min`` of the request and the live rows at build time; ``max_list_len`` counts tombstoned rows)."""
        if self._ivf is None:
            return None
        nl, ni, ml = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib_knn_ivf.load().astts_knn_ivf_info(self._ivf, ctypes.byref(nl), ctypes.byref(ni), ctypes.byref(ml)))
        return {"index_type": "IVF_FLAT", "nlist": int(nl.value), "n_indexed": int(ni.value), "max_list_len": int(ml.value)}

    def index_export(self):
        """-> (centroids fp32 ``[nlist, D]``, list_of int32 ``[n]``) as numpy arrays (synchronises)."""
        info = self.index_info()
        if info is None:
            raise RuntimeError("the bank has no index: build_index first")
        cent = np.empty((info["nlist"], self.d), np.float32)
        list_of = np.empty(info["n_indexed"], np.int32)
        with torch.cuda.device(self.device):
            _lib.check(_lib_knn_ivf.load().astts_knn_ivf_export(self._ivf, cent.ctypes.data, list_of.ctypes.data))
        return cent, list_of

    def search_ivf_device(self, queries: torch.Tensor, k: int, nprobe: int = _lib_knn_ivf.DEFAULT_NPROBE,
                          row_mask: Optional[torch.Tensor] = None, return_f64: bool = False):
        """``search_device`` over the rows of the ``min(nprobe, nlist)`` lists whose centroids are closest to each query: the same
        order, and for every hit bit for bit the scores ``search_device`` returns for it; -1 / -inf (+inf for L2) where the probed
        lists hold fewer than ``k`` allowed rows.  ``nprobe >= nlist`` is the brute-force result.  Enqueued on the current stream,
        no synchronisation."""
        if self._ivf is None:
            raise RuntimeError("the bank has no index: build_index first (there is no quiet fall-back to the brute-force search)")
        q = _as_queries(queries, self.d, self.device)
        k, nprobe = int(k), int(nprobe)
        if not 1 <= k <= _lib.KNN_MAX_K:
            raise ValueError(f"k must be in 1..{_lib.KNN_MAX_K}, got {k}")
        if nprobe < 1:
            raise ValueError(f"nprobe must be >= 1, got {nprobe}")
        nq = int(q.shape[0])
        out = _outputs(nq, k, return_f64, self.device)
        out_idx, out_score, s64 = out
        if nq:
            lib = _lib_knn_ivf.load()
            prev = self._enter()
            try:
                base, ws_bytes = self._iws.fit((nq, k, nprobe), lambda: f"invalid IVF search shape nq={nq} k={k} nprobe={nprobe}",
                                               lib.astts_knn_ivf_workspace_bytes, self._ivf, self._h)
                m, mptr, mstride = _row_mask(row_mask, nq, self.n, self.device)
                rc = lib.astts_knn_ivf_search(self._ivf, self._h, q.data_ptr(), nq, k, nprobe, out_idx.data_ptr(), out_score.data_ptr(),
                                              None if s64 is None else s64.data_ptr(), mptr, mstride, base, ws_bytes,
                                              torch.cuda.current_stream(self._index).cuda_stream)
                if rc != 0:
                    _lib.check(rc)
            finally:
                if prev is not None:
                    torch.cuda.set_device(prev)
        return out if return_f64 else out[:2]

    def search_ivf(self, queries, k: int, nprobe: int = _lib_knn_ivf.DEFAULT_NPROBE, row_mask=None, return_f64: bool = False):
        """Host convenience of ``search_ivf_device``: accepts numpy / lists, returns numpy (idx int64 [Q,k], score fp32 [Q,k] and,
        with ``return_f64``, score fp64 [Q,k])."""
        q, row_mask = _host_inputs(queries, row_mask, self.device)
        out = self.search_ivf_device(q, k, nprobe, row_mask=row_mask, return_f64=return_f64)
        return tuple(t.cpu().numpy() for t in out)

    def route(self, nq: int, k: int, masked: bool = False, aligned: bool = True):
        """``route`` (above) for a search of this bank: ``[(rows, scan, finish), ...]``, one per query group.  A bank with tombstones
        searches as a masked one."""
        return route(self.n, self.d, nq, k, masked or self.live < self.n, aligned)

    def last_fallbacks(self) -> int:
        """How many queries of the last search needed the exact fp64 scan (synchronises)."""
        if self._ws.buf is None:
            return 0
        out = ctypes.c_int32()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().astts_knn_last_fallbacks(self._h, self._ws.base, _lib.stream_ptr(), ctypes.byref(out)))
        return int(out.value)

    # ---- bench-only: time the scan kernel with HIP events on the search stream
    def profile_enable(self, on: bool = True) -> None:
        _lib.check(_lib.load().astts_knn_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        ms = ctypes.c_double()
        cnt = ctypes.c_int64()
        _lib.check(_lib.load().astts_knn_profile_read(self._h, ctypes.byref(ms), ctypes.byref(cnt)))
        return float(ms.value), int(cnt.value)
