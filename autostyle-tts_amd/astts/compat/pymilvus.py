"""``MilvusClient`` call surface of the reference, served by the HBM-resident StyleBank.

Mirrors exactly the calls the reference makes (paths under /root/reference):
  MilvusClient(db_path)                                     milvus/search_embeddings.py:31
  .has_collection(collection_name=)                         src/search_milvus.py:177
  .get_collection_info(name) / .describe_collection(name)   src/search_milvus.py:183
  .search(collection_name=, data=[vec], anns_field="vector", metric_type="COSINE" | param={...},
          limit=, filter=None, output_fields=[...])          milvus/search_embeddings.py:15-22,
                                                            src/search_milvus.py:140-147,
                                                            milvus/search_json.py:246-252
  .create_collection(collection_name, dimension) / .insert(collection_name, data=[{...}]) /
  .drop_collection(collection_name)                          milvus/RAG.py:49-57,541-544
and the calls that maintain a collection after ``insert`` (not made by the reference; pymilvus' names and result keys):
  .delete(collection_name, ids= | filter=) / .upsert(collection_name, data) / .query(...) / .get(collection_name, ids) /
  .get_collection_stats(collection_name) / .compact(collection_name)
  .search(..., group_by_field=, group_size=, strict_group_size=, offset=, search_params={"params": {"radius":, "range_filter":}})
                                                            the ``limit`` closest groups / the hits inside a score band: search_rows
  FieldSchema / CollectionSchema / DataType, .create_collection(schema=CollectionSchema(...)), .create_index(...)
                                                            milvus/insert_embeddings.py:52-79 (auto_id pk, VARCHAR fields)
Result shape: ``list[Q]`` of ``list[k]`` of ``{'id': pk, 'distance': cosine_similarity,
'entity': {field: value}}`` sorted by similarity descending (``distance`` IS the similarity for
COSINE: output_emb/search_results.json holds 0.81..0.95, larger = closer).  Collections created with ``metric_type`` IP / L2
return the inner product (descending) / the squared Euclidean distance (ascending), as Milvus does.  ``filter``: scalar
expressions over the primary key and the dynamic fields (astts.milvus_filter) become a row mask of the search kernels;
``limit`` up to 1024 (32 hits per selection pass over one scan).

``MilvusClient(uri, use_index=True)`` honours ``create_index(... "IVF_FLAT", {"nlist": N})`` and ``param={"nprobe": P}``
(include/knn/astts_knn_ivf.h: k-means lists, the exact answer over the rows of the P closest lists).  Without the keyword -- the
default -- an index request only records its parameters, ``nprobe`` is ignored and every search is the exact brute-force one.

The file behind ``db_path`` is read with astts.milvus_lite (SQLite + protobuf wire format); the
vectors go to HBM once per collection and stay there: ``insert`` appends to the resident bank, ``delete`` / ``upsert`` tombstone its
rows, ``compact`` squeezes them out (astts.knn.StyleBank.append / delete_rows / compact).  Errors raise ``MilvusException`` -- the
reference wraps every call in try/except and degrades to ``[]`` itself
(milvus/search_embeddings.py:24-27), so the shim does not swallow anything.

Extra keys beyond pymilvus: each hit also carries ``'row'`` (row index in the bank == style id,
because the reference's pk restarts per speaker and is not unique: milvus/RAG.py:507).  A row keeps its index through inserts and
deletes; ``compact`` renumbers the rows that are left.
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..milvus_lite import MilvusLiteFile, MilvusLiteWriter


class DataType:
    """The pymilvus.DataType members the reference's bank builders use (milvus/insert_embeddings.py:53-56)."""
    BOOL, INT8, INT16, INT32, INT64 = 1, 2, 3, 4, 5
    FLOAT, DOUBLE = 10, 11
    VARCHAR, JSON = 21, 23
    FLOAT_VECTOR = 101


class FieldSchema:
    def __init__(self, name: str, dtype: int, description: str = "", is_primary: bool = False, auto_id: bool = False,
                 dim: Optional[int] = None, max_length: Optional[int] = None, **_kw):
        self.name, self.dtype, self.description = name, dtype, description
        self.is_primary, self.auto_id, self.dim, self.max_length = bool(is_primary), bool(auto_id), dim, max_length


class CollectionSchema:
    """Explicit schema (milvus/insert_embeddings.py:52-63).  ``metric_type`` rides on the schema there (pymilvus ignores
    unknown keyword arguments of CollectionSchema; the collection then gets its metric from the index) -- here it selects
    the collection's metric directly, COSINE when absent."""

    def __init__(self, fields: Sequence[FieldSchema], description: str = "", enable_dynamic_field: bool = False, **kw):
        self.fields, self.description, self.enable_dynamic_field = list(fields), description, enable_dynamic_field
        self.metric_type = kw.get("metric_type")
        pks = [f for f in self.fields if f.is_primary]
        vecs = [f for f in self.fields if f.dtype == DataType.FLOAT_VECTOR]
        if len(pks) != 1 or len(vecs) != 1 or not vecs[0].dim:
            raise MilvusException(1, "schema needs exactly one primary key and one FLOAT_VECTOR field with a dim")
        self.primary_field, self.vector_field = pks[0], vecs[0]
        self.auto_id = pks[0].auto_id
        self.dim = int(vecs[0].dim)


class MilvusException(Exception):
    def __init__(self, code: int = 1, message: str = ""):
        super().__init__(f"<MilvusException: (code={code}, message={message})>")
        self.code = code
        self.message = message


class _Collection:
    def __init__(self, name: str, dim: int, metric: str = "COSINE", pk_field: str = "id",
                 vector_field: str = "vector", index_params: Optional[Dict[str, str]] = None):
        self.name = name
        self.dim = int(dim)
        self.metric = metric.upper()
        self.pk_field = pk_field
        self.vector_field = vector_field
        self.index_params = dict(index_params or {})
        self.auto_id = False
        self.vectors: List[np.ndarray] = []
        self.pks: List[int] = []
        self.metas: List[Dict[str, Any]] = []
        self.live: List[bool] = []      # vectors / pks / metas / live are row-aligned with the bank; a deleted row stays until compact
        self.n_live = 0
        self._bank = None  # astts.knn.StyleBank, built lazily by the first search, then kept up to date in place
        self.use_index = False      # MilvusClient(use_index=True): an IVF_FLAT index request is built on the resident bank
        self._index_nlist: Optional[int] = None      # the nlist the bank's index was built for
        self._group_codes: Dict[str, Any] = {}      # group_by_field -> (int32 codes [rows], groups); dropped whenever the rows change

    def group_codes(self, field: str):
        """Dense group codes of the rows under ``field`` (a scalar field or the primary key), cached per field: -> (int32 ``[rows]``,
        number of groups).  Equal values of one type share a code, in the order of their first row; a row without the field forms
        a group of its own."""
        if field == self.vector_field:
            raise MilvusException(1100, f"unsupported field type for group by: field {field!r} is the vector field")
        hit = self._group_codes.get(field)
        if hit is not None:
            return hit
        if field != self.pk_field and not any(field in m for m in self.metas):
            raise MilvusException(1100, f"groupBy field not found in schema: field not found[field={field}]")
        codes = np.empty(len(self.pks), np.int32)
        seen: Dict[Any, int] = {}
        for i, meta in enumerate(self.metas):
            if field == self.pk_field:
                key = ("pk", self.pks[i])
            elif field in meta:
                v = meta[field]
                key = (type(v).__name__, v if isinstance(v, (bool, int, float, str, bytes, type(None))) else repr(v))
            else:
                key = ("row", i)
            codes[i] = seen.setdefault(key, len(seen))
        self._group_codes[field] = (codes, max(len(seen), 1))
        return self._group_codes[field]

    def ivf_nlist(self) -> Optional[int]:
        """``nlist`` of the recorded index request when its type is IVF_FLAT (default 128, Milvus' own), else None.  The request is
        kept as strings (create_index; the Milvus-Lite file): ``nlist`` flat or inside the ``params`` dictionary."""
        if str(self.index_params.get("index_type", "")).upper() != "IVF_FLAT":
            return None
        nlist = self.index_params.get("nlist")
        if nlist is None:
            inner = self.index_params.get("params")
            if isinstance(inner, str):
                import ast
                try:
                    inner = ast.literal_eval(inner)
                except (ValueError, SyntaxError):
                    inner = None
            if isinstance(inner, dict):
                nlist = inner.get("nlist")
        try:
            nlist = int(nlist) if nlist is not None else 128
        except (TypeError, ValueError):
            raise MilvusException(1100, f"invalid nlist {nlist!r} of the IVF_FLAT index of {self.name}") from None
        if nlist < 1:
            raise MilvusException(1100, f"invalid nlist {nlist} of the IVF_FLAT index of {self.name}")
        return nlist

    def sync_index(self) -> None:
        """The resident bank's index as the recorded request and ``use_index`` want it: built (trained once, when the bank goes
        resident or the request arrives; inserts, deletes and compaction keep it in step through StyleBank), or absent."""
        if self._bank is None or self._bank.live == 0:      # (an index needs a live row: built by the first search after an insert)
            return
        nlist = self.ivf_nlist() if self.use_index else None
        have = self._bank.index_info()
        if nlist is None:
            if have is not None:
                self._bank.drop_index()
        elif have is None or self._index_nlist != nlist:
            self._bank.build_index(nlist)
            self._index_nlist = nlist

    def live_rows(self) -> List[int]:
        return [i for i, on in enumerate(self.live) if on]

    def matrix(self) -> np.ndarray:
        if not self.vectors:
            return np.zeros((0, self.dim), np.float32)
        return np.stack(self.vectors).astype(np.float32, copy=False)

    def bank(self):
        if self._bank is None:
            from ..knn import StyleBank  # needs the GPU + libastts.so; raises otherwise

            m = self.matrix()
            m16 = m.astype(np.float16)
            # upload as fp16 when that is lossless (half the HBM traffic of every scan)
            self._bank = StyleBank(m16 if np.array_equal(m16.astype(np.float32), m) else m, metric=self.metric)
            if self.n_live < len(self.live):      # rows deleted before the first search: the bank stays row-aligned with the lists
                self._bank.delete_rows([i for i, on in enumerate(self.live) if not on])
            self._index_nlist = None
            self.sync_index()
        return self._bank


class MilvusClient:
    def __init__(self, uri: str = "./milvus_demo.db", persist: bool = True, use_index: bool = False, **_kwargs):
        """``uri`` is a Milvus-Lite file path, loaded if it exists.  As with pymilvus, create_collection / insert /
        drop_collection are written through to that file (created on first write) unless ``persist=False``.

        ``use_index``: a collection whose recorded index type is IVF_FLAT gets that index (its ``nlist``) when its bank goes
        resident, and ``search`` probes ``nprobe`` lists (``param`` / ``search_params``; 8 when absent).  FLAT / AUTOINDEX / no
        index, grouped and ranged searches: brute force.  Centroids are not stored in the file: training is deterministic, a
        reload rebuilds the same index.  Off by default: ``nprobe`` is then ignored and every search is exact."""
        self.uri = uri
        self._use_index = bool(use_index)
        self._persist = bool(persist) and "://" not in uri
        self._writer: Optional[MilvusLiteWriter] = None
        self._colls: Dict[str, _Collection] = {}
        if os.path.exists(uri):
            f = MilvusLiteFile(uri)
            try:
                for name in f.collections():
                    info = f.info(name)
                    c = _Collection(name, info.dim, info.metric_type, info.pk_field,
                                    info.vector_field.name if info.vector_field else "vector",
                                    info.index_params)
                    v, pks, metas = f.load(name)
                    c.vectors = [v[i] for i in range(v.shape[0])]
                    c.pks = [int(x) for x in pks]
                    c.metas = metas
                    c.live = [True] * len(c.pks)
                    c.n_live = len(c.pks)
                    c.use_index = self._use_index
                    self._colls[name] = c
            finally:
                f.close()

    def _file(self) -> Optional[MilvusLiteWriter]:
        if self._persist and self._writer is None:
            self._writer = MilvusLiteWriter(self.uri)
        return self._writer

    # ------------------------------------------------------------------ collection management
    def has_collection(self, collection_name: str, **_kw) -> bool:
        return collection_name in self._colls

    def list_collections(self, **_kw) -> List[str]:
        return list(self._colls)

    def _get(self, name: str) -> _Collection:
        if name not in self._colls:
            raise MilvusException(100, f"collection not found[collection={name}]")
        return self._colls[name]

    def describe_collection(self, collection_name: str, **_kw) -> Dict[str, Any]:
        c = self._get(collection_name)
        return {
            "collection_name": c.name,
            "auto_id": c.auto_id,
            "num_shards": 0,
            "description": "",
            "fields": [
                {"field_id": 100, "name": c.pk_field, "description": "", "type": 5, "params": {}, "is_primary": True},
                {"field_id": 101, "name": c.vector_field, "description": "", "type": 101, "params": {"dim": c.dim}},
            ],
            "enable_dynamic_field": True,
            "num_entities": c.n_live,
            "metric_type": c.metric,
        }

    get_collection_info = describe_collection  # src/search_milvus.py:183 uses this older name

    def create_collection(self, collection_name: str, dimension: Optional[int] = None,
                          primary_field_name: str = "id", vector_field_name: str = "vector",
                          metric_type: str = "COSINE", schema=None, index_params=None, **_kw) -> None:
        auto_id = False
        if isinstance(schema, CollectionSchema):      # explicit schema: field names, auto id, metric from the schema object
            dimension = schema.dim
            primary_field_name, vector_field_name = schema.primary_field.name, schema.vector_field.name
            metric_type = schema.metric_type or metric_type
            auto_id = schema.auto_id
        elif schema is not None and dimension is None:
            dimension = getattr(schema, "dim", None) or (schema.get("dim") if isinstance(schema, dict) else None)
        if not dimension:
            raise MilvusException(1, "create_collection needs a dimension")
        if collection_name in self._colls:
            return
        self._colls[collection_name] = _Collection(collection_name, int(dimension), metric_type,
                                                   primary_field_name, vector_field_name)
        self._colls[collection_name].auto_id = auto_id
        self._colls[collection_name].use_index = self._use_index
        if self._file():
            self._file().create_collection(collection_name, int(dimension), metric_type, primary_field_name,
                                           vector_field_name)

    def create_index(self, collection_name: str, field_name: Optional[str] = None, index_params=None, **_kw) -> None:
        """milvus/insert_embeddings.py:75-79.  By default the search here is exact brute force on the GPU, so an index request only
        records its parameters (and a metric, if it names one, for a collection that has no rows yet).  A client made with
        ``use_index=True`` builds an IVF_FLAT request on the resident bank (at once when the bank is resident, else when it goes)."""
        c = self._get(collection_name)
        params = dict(index_params) if isinstance(index_params, dict) else {}
        mt = params.get("metric_type") or (params.get("params") or {}).get("metric_type")
        if mt and not c.pks:
            c.metric = str(mt).upper()
        c.index_params.update({k: str(v) for k, v in params.items()})
        if self._use_index:
            if "nlist" in c.index_params and "nlist" not in params:      # (an earlier request's: this one names its own, or none)
                del c.index_params["nlist"]
            c.ivf_nlist()           # a bad nlist is refused here, not at the first search
            c.sync_index()

    def drop_collection(self, collection_name: str, **_kw) -> None:
        if self._colls.pop(collection_name, None) is not None and self._file():
            self._file().drop_collection(collection_name)

    def _append_rows(self, c: _Collection, rows) -> List[int]:
        """Validate ``rows`` and append them to the host lists and, when the collection has one, to the resident bank (fp32 rows: the
        kernel decides whether they are fp16-exact).  Nothing is written to the file.  -> their primary keys."""
        for r in rows:      # validate the whole request before any row lands (a bad row rejects the request)
            if np.asarray(r[c.vector_field]).shape != (c.dim,):
                raise MilvusException(1100, f"the dim ({np.asarray(r[c.vector_field]).size}) of field data"
                                            f"({c.vector_field}) is not equal to schema dim ({c.dim})")
        vecs = [np.asarray(r[c.vector_field], dtype=np.float32) for r in rows]
        if c._bank is not None and vecs:
            from .._lib import AsttsError
            try:
                c._bank.append(np.stack(vecs))      # first: a refused batch (non-finite values) leaves bank and lists as they were
            except AsttsError as e:
                raise MilvusException(1100, f"insert refused: {e}") from None
        ids = []
        for r, vec in zip(rows, vecs):
            c.vectors.append(vec)
            pk = (max(c.pks) + 1 if c.pks else 1) if c.auto_id else int(r.get(c.pk_field, len(c.pks)))
            c.pks.append(pk)
            ids.append(pk)
            c.metas.append({k: v for k, v in r.items() if k not in (c.vector_field, c.pk_field)})
            c.live.append(True)
        c.n_live += len(rows)
        c._group_codes = {}
        return ids

    def _tombstone(self, c: _Collection, rows: Sequence[int]) -> int:
        """Delete the live rows among ``rows`` on the host and in the resident bank.  -> how many were live."""
        rows = [int(i) for i in rows if c.live[int(i)]]
        for i in rows:
            c.live[i] = False
        c.n_live -= len(rows)
        c._group_codes = {}
        if rows and c._bank is not None:
            c._bank.delete_rows(rows)
        return len(rows)

    def _rewrite(self, c: _Collection) -> None:
        """delete / upsert / compact in the Milvus-Lite file: the collection is written again from its live rows, in order (the
        existing writer; Milvus-Lite's own delete records are not reproduced).  Reopening the file shows the live rows, compacted."""
        f = self._file()
        if not f:
            return
        f.drop_collection(c.name)
        f.create_collection(c.name, c.dim, c.metric, c.pk_field, c.vector_field)
        f.insert(c.name, ((c.pks[i], c.vectors[i], c.metas[i]) for i in c.live_rows()), c.pk_field, c.vector_field)

    def insert(self, collection_name: str, data, **_kw) -> Dict[str, Any]:
        c = self._get(collection_name)
        rows = [data] if isinstance(data, dict) else list(data)
        first_new = len(c.pks)
        ids = self._append_rows(c, rows)
        if self._file():
            self._file().insert(c.name, ((c.pks[i], c.vectors[i], c.metas[i]) for i in range(first_new, len(c.pks))),
                                c.pk_field, c.vector_field)
        return {"insert_count": len(rows), "ids": ids}

    def _select(self, c: _Collection, ids, filter: Optional[str]) -> List[int]:
        """The live rows whose primary key is in ``ids`` (when given) and that satisfy ``filter`` (when given), in row order."""
        keep = np.asarray(c.live, dtype=bool)
        if ids is not None:
            want = {int(i) for i in ([ids] if isinstance(ids, (int, np.integer)) else ids)}
            keep &= np.fromiter((pk in want for pk in c.pks), dtype=bool, count=len(c.pks))
        if filter:
            keep &= self._filter_mask(c, filter).astype(bool)
        return [int(i) for i in np.flatnonzero(keep)]

    @staticmethod
    def _filter_mask(c: _Collection, filter: str) -> np.ndarray:
        """``filter`` compiled to a mask over the rows of ``c`` (astts.milvus_filter), non-zero where a row satisfies it."""
        from ..milvus_filter import FilterSyntaxError, row_mask
        try:
            return row_mask(filter, c.pk_field, c.pks, c.metas)
        except FilterSyntaxError as e:
            raise MilvusException(1100, f"failed to create query plan: cannot parse expression: {filter}, error: {e}") from None

    def delete(self, collection_name: str, ids=None, filter: Optional[str] = None, **_kw) -> Dict[str, Any]:
        """Exactly one of ``ids`` (one primary key or a list) / ``filter``.  -> ``{"delete_count": rows deleted}``: every live row
        with one of the keys (the reference's keys are not unique), or that satisfies the filter."""
        c = self._get(collection_name)
        if (ids is None) == (not filter):
            raise MilvusException(1, "delete needs exactly one of ids and filter")
        count = self._tombstone(c, self._select(c, ids, filter))
        if count:
            self._rewrite(c)
        return {"delete_count": count}

    def upsert(self, collection_name: str, data, **_kw) -> Dict[str, Any]:
        """For each row: every live row with its primary key is deleted, then the row is inserted.  -> ``{"upsert_count": n}``."""
        c = self._get(collection_name)
        rows = [data] if isinstance(data, dict) else list(data)
        first_new = len(c.pks)
        keys = {int(r[c.pk_field]) for r in rows if c.pk_field in r}
        old = self._select(c, keys, None) if keys else []
        ids = self._append_rows(c, rows)      # (first: a request that is refused deletes nothing)
        self._tombstone(c, old)
        last = {pk: first_new + j for j, pk in enumerate(ids)}      # of rows of this request that share a key, the last one stays
        self._tombstone(c, [first_new + j for j, pk in enumerate(ids) if last[pk] != first_new + j])
        self._rewrite(c)
        return {"upsert_count": len(rows)}

    def query(self, collection_name: str, filter: str = "", output_fields: Optional[Sequence[str]] = None, limit: Optional[int] = None,
              ids=None, **_kw) -> List[Dict[str, Any]]:
        """The live rows that satisfy ``filter`` / carry one of ``ids``, in row order, at most ``limit``: dicts with the primary key
        and the fields of ``output_fields`` (``["*"]``: every scalar field; the vector only when it is named)."""
        c = self._get(collection_name)
        if not filter and ids is None and limit is None:
            raise MilvusException(1100, "empty expression should be used with limit")
        if limit is not None and int(limit) < 1:
            raise MilvusException(1, f"limit {limit} is invalid")
        rows = self._select(c, ids, filter)
        fields = list(output_fields or [])
        out = []
        for i in rows[:None if limit is None else int(limit)]:
            rec = {c.pk_field: c.pks[i]}
            for f in fields:
                if f == "*":
                    rec.update(c.metas[i])
                elif f == c.vector_field:
                    rec[f] = c.vectors[i].tolist()
                elif f in c.metas[i]:
                    rec[f] = c.metas[i][f]
            out.append(rec)
        return out

    def get(self, collection_name: str, ids, output_fields: Optional[Sequence[str]] = None, **_kw) -> List[Dict[str, Any]]:
        return self.query(collection_name, ids=ids, output_fields=output_fields)

    def get_collection_stats(self, collection_name: str, **_kw) -> Dict[str, Any]:
        return {"row_count": self._get(collection_name).n_live}

    def compact(self, collection_name: str, **_kw) -> int:
        """Drop the deleted rows from the host lists and from the resident bank; the rows that are left keep their order and are
        renumbered (a hit's ``'row'``).  -> how many rows were removed (pymilvus returns a job id here)."""
        c = self._get(collection_name)
        removed = len(c.live) - c.n_live
        if removed == 0:
            return 0
        if c._bank is not None:
            if c.n_live == 0:      # (a bank holds at least one row)
                c._bank.close()
                c._bank = None
            else:
                old_to_new = c._bank.compact()
                assert int((old_to_new >= 0).sum()) == c.n_live
        keep = c.live_rows()
        c.vectors, c.pks, c.metas = [c.vectors[i] for i in keep], [c.pks[i] for i in keep], [c.metas[i] for i in keep]
        c.live = [True] * len(keep)
        c._group_codes = {}
        self._rewrite(c)
        return removed

    # ------------------------------------------------------------------ search (the hot path)
    def search(self, collection_name: str, data, filter: Optional[str] = "", limit: int = 10,
               output_fields: Optional[Sequence[str]] = None, search_params: Optional[dict] = None,
               anns_field: Optional[str] = None, metric_type: Optional[str] = None,
               param: Optional[dict] = None, group_by_field: Optional[str] = None, group_size: int = 1,
               strict_group_size: Optional[bool] = None, offset: int = 0, **_kw) -> List[List[Dict[str, Any]]]:
        """``group_by_field`` (a scalar field or the primary key), ``group_size``, ``offset`` and ``radius`` / ``range_filter`` (in
        ``search_params["params"]``, ``param["params"]`` or flat in ``search_params``): see ``search_rows``.  Hits of a grouped
        search carry the group field in ``entity``, as pymilvus adds it to the output fields."""
        idx, score = self.search_rows(collection_name, data, filter=filter, limit=limit, search_params=search_params,
                                      anns_field=anns_field, metric_type=metric_type, param=param, group_by_field=group_by_field,
                                      group_size=group_size, strict_group_size=strict_group_size, offset=offset)
        return self.hits_from_rows(collection_name, idx, score, output_fields, group_by_field=group_by_field)

    @staticmethod
    def _request_param(name: str, sources):
        """``name`` of a request: its value in the first of ``sources`` -- dictionaries, or None where the request has none, in the
        order of their precedence -- that holds one; None when absent."""
        for src in sources:
            if isinstance(src, dict) and src.get(name) is not None:
                return src[name]
        return None

    @staticmethod
    def _nprobe_of(search_params: Optional[dict], param: Optional[dict]) -> int:
        """``nprobe`` of a request: from param["params"], search_params["params"], flat ``param`` (the reference:
        ``param={"nprobe": 10}``) or flat ``search_params``; 8 when absent.  Below 1 is refused."""
        given = MilvusClient._request_param("nprobe", ((param or {}).get("params"), (search_params or {}).get("params"), param, search_params))
        if given is None:
            from .._lib_knn_ivf import DEFAULT_NPROBE
            return DEFAULT_NPROBE
        try:
            nprobe = int(given)
        except (TypeError, ValueError):
            raise MilvusException(1100, f"invalid nprobe {given!r}") from None
        if nprobe < 1:
            raise MilvusException(1100, f"nprobe {nprobe} is invalid: it must be at least 1")
        return nprobe

    @staticmethod
    def _range_of(metric: str, search_params: Optional[dict], param: Optional[dict]):
        """(radius, range_filter) of a request, None where absent: from search_params["params"], param["params"], flat search_params."""
        sources = ((search_params or {}).get("params"), (param or {}).get("params"), search_params)
        radius, range_filter = (None if v is None else float(v)
                                for v in (MilvusClient._request_param(name, sources) for name in ("radius", "range_filter")))
        if radius is not None and range_filter is not None and (range_filter >= radius if metric == "L2" else radius >= range_filter):
            raise MilvusException(1100, f"range_filter({range_filter}) must be "
                                        f"{'less' if metric == 'L2' else 'greater'} than radius({radius}) for {metric}")
        return radius, range_filter

    def search_rows(self, collection_name: str, data, filter: Optional[str] = "", limit: int = 10, search_params: Optional[dict] = None,
                    anns_field: Optional[str] = None, metric_type: Optional[str] = None, param: Optional[dict] = None,
                    group_by_field: Optional[str] = None, group_size: int = 1, strict_group_size: Optional[bool] = None,
                    offset: int = 0, **_kw):
        """The arithmetic half of ``search``: -> (row index int64 [Q, k], cosine similarity fp32 [Q, k]) as numpy arrays, -1 = no hit
        (k = min(limit, live rows); k = 0 columns for an empty collection).  Row index == style id.  The data-parallel drivers shard
        THIS call over the ranks and all-gather its result (astts.parallel.sharded_search); ``hits_from_rows`` turns rows into the
        pymilvus result shape wherever the records are written.

        Selection controls (include/knn/astts_knn_grouped.h has the definition; a call that uses none of them takes the plain path):
        ``radius`` / ``range_filter``: only rows with ``radius < score <= range_filter`` (COSINE / IP) or
        ``range_filter <= distance < radius`` (L2) are hits.  ``group_by_field``: the ``limit`` groups whose best row is closest, in
        that order, ``group_size`` rows of each -- columns ``g * group_size + j``, -1 where a group has fewer rows.
        ``strict_group_size`` is accepted for compatibility: the result is ALWAYS the strict one (every returned group holds its
        ``group_size`` closest eligible rows, or all it has), not Milvus' approximation.  ``offset`` skips the first ``offset`` groups
        (hits without grouping): ``limit + offset`` are searched and sliced, ``(limit + offset) * group_size`` at most 1024.  The
        bank-sharded merge of astts.parallel is not group-aware."""
        c = self._get(collection_name)
        radius, range_filter = self._range_of(c.metric, search_params, param)
        if int(offset) < 0 or int(group_size) < 1:
            raise MilvusException(1100, f"offset {offset} / group_size {group_size} is invalid")
        groups = c.group_codes(group_by_field) if group_by_field else None
        selecting = groups is not None or int(offset) > 0 or radius is not None or range_filter is not None
        mask = self._filter_mask(c, filter) if filter else None      # (the reference passes None: milvus/search_json.py:246-252)
        if anns_field is not None and anns_field != c.vector_field:
            raise MilvusException(1, f"anns_field {anns_field!r} does not exist (vector field is {c.vector_field!r})")
        mt = metric_type or (search_params or {}).get("metric_type") or (param or {}).get("metric_type")
        if mt is not None and mt.upper() != c.metric:
            raise MilvusException(1100, f"metric type not match: invalid parameter[expected={c.metric}][actual={mt}]")
        q = np.asarray(data, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != c.dim:
            raise MilvusException(1100, f"vector dimension mismatch, expected vector size(byte) {c.dim * 4}, "
                                        f"actual {q.shape[-1] * 4}")
        if c.n_live == 0:
            return np.zeros((q.shape[0], 0), np.int64), np.zeros((q.shape[0], 0), np.float32)
        if limit < 1:
            raise MilvusException(1, f"limit {limit} is invalid")
        from .._lib import KNN_MAX_K, AsttsError
        skip = 0            # columns sliced away behind the search
        if selecting:       # limit + offset groups (hits) of group_size rows, sliced behind the search
            gs = min(int(group_size), c.n_live) if groups is not None else 1
            want = min(int(limit) + int(offset), c.n_live)
            if want * gs > KNN_MAX_K:
                raise MilvusException(1100, f"limit {limit} (+ offset {offset}, x group_size {gs}) is not supported by this build: at most "
                                            f"{KNN_MAX_K} hits per query (collection holds {c.n_live} rows)")
            codes, n_groups = groups if groups is not None else (None, None)
            skip = min(int(offset), want) * gs
            # (refused: the rounds ran out -- never a partial answer)
            what, method, args = "grouped search", "search_grouped", (q, want, gs)
            kwargs = dict(groups=codes, n_groups=n_groups, radius=radius, range_filter=range_filter, row_mask=mask)
        else:
            k = min(int(limit), c.n_live)
            if k > KNN_MAX_K:
                # pymilvus accepts limit up to 16384; the reference asks for 1 or 3 (milvus/search_json.py:411,
                # milvus/search_embeddings.py:64).  Here: 32 certified hits per selection pass, at most 32 passes.
                raise MilvusException(1100, f"limit {limit} is not supported by this build: at most {KNN_MAX_K} hits per query "
                                            f"(collection holds {c.n_live} rows)")
            if self._use_index and c.ivf_nlist() is not None:      # (grouped and ranged searches stay on the brute-force path above)
                nprobe = self._nprobe_of(search_params, param)
                c.bank()
                c.sync_index()
                # (refused: more than 1024 lists to probe -- never answered by another search)
                what, method, args, kwargs = "IVF_FLAT search", "search_ivf", (q, k, nprobe), dict(row_mask=mask)
            else:           # what = None: an error of the plain search is passed on as it is.  Unfiltered, it is search(q, k) and no more
                what, method, args, kwargs = None, "search", (q, k), ({} if mask is None else dict(row_mask=mask))
        try:
            idx, score = getattr(c.bank(), method)(*args, **kwargs)
        except AsttsError as e:
            if what is None:
                raise
            raise MilvusException(1100, f"{what} refused: {e}") from None
        return np.asarray(idx, dtype=np.int64)[:, skip:], np.asarray(score, dtype=np.float32)[:, skip:]

    def hits_from_rows(self, collection_name: str, idx, score, output_fields: Optional[Sequence[str]] = None,
                       group_by_field: Optional[str] = None) -> List[List[Dict[str, Any]]]:
        """(row index [Q, k], similarity [Q, k]) -> ``list[Q]`` of ``list[<= k]`` of {'id', 'distance', 'entity', 'row'}.
        ``group_by_field``: the field a grouped search grouped by; every hit carries it in ``entity`` (when the row has it)."""
        c = self._get(collection_name)
        idx, score = np.asarray(idx), np.asarray(score)
        out: List[List[Dict[str, Any]]] = []
        for qi in range(idx.shape[0]):
            hits = []
            for j in range(idx.shape[1]):
                row = int(idx[qi, j])
                if row < 0:
                    continue
                meta = c.metas[row]
                if output_fields:
                    ent = {f: meta[f] for f in output_fields if f in meta}
                else:
                    ent = {}
                if group_by_field == c.pk_field:
                    ent[group_by_field] = c.pks[row]
                elif group_by_field in meta:
                    ent[group_by_field] = meta[group_by_field]
                hits.append({"id": c.pks[row], "distance": float(score[qi, j]), "entity": ent, "row": row})
            out.append(hits)
        return out

    def close(self) -> None:
        for c in self._colls.values():
            if c._bank is not None:
                c._bank.close()
                c._bank = None
        if self._writer is not None:
            self._writer.close()
            self._writer = None
