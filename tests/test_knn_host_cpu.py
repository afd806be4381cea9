"""CPU tests of the pieces the three style-bank searches share (astts/knn.py: workspace, row mask, queries), of the one binder of
the headers beside include/astts.h (astts._lib.bind_headers) and of the request-parameter lookup of the MilvusClient shim.  The
pieces run here on CPU tensors, with a fake sizing function in place of the library.  No GPU is needed."""
import pytest
import torch

CPU = torch.device("cpu")


def test_workspace_grows_once_and_hands_out_no_stale_pointer():
    from astts.knn import _Workspace

    ws, asked = _Workspace(CPU), []

    def sizing(handle, *key):
        asked.append((handle,) + key)
        return {(2, 3): 1000, (70, 40): 5000, (1, 1): 1000, (9, 9): 0}[key]

    def fit(key):
        base, nbytes = ws.fit(key, lambda: f"invalid shape {key}", sizing, "h")
        start = ws.buf.data_ptr()
        assert base % 256 == 0 and start <= base and base + nbytes == start + ws.buf.numel()      # inside the CURRENT buffer, to its end
        return nbytes

    bufs = []
    for key, need in (((2, 3), 1000), ((70, 40), 5000), ((1, 1), 1000), ((2, 3), 1000)):      # the last: the first key again, after the growth
        assert fit(key) >= need
        if not bufs or bufs[-1] is not ws.buf:
            bufs.append(ws.buf)
    assert len(bufs) == 2 and asked == [("h", 2, 3), ("h", 70, 40), ("h", 1, 1)]      # allocated twice; every shape sized once
    with pytest.raises(ValueError, match=r"invalid shape \(9, 9\)"):
        fit((9, 9))
    ws.forget()
    assert fit((2, 3)) >= 1000 and ws.buf is bufs[-1] and asked[-2:] == [("h", 9, 9), ("h", 2, 3)]      # same buffer, sized again


def test_row_mask_shapes_strides_and_conversion():
    from astts.knn import _row_mask

    n, nq = 7, 3
    assert _row_mask(None, nq, n, CPU) == (None, None, 0)
    one = torch.tensor([1, 0, 2, 0, 0, 1, 0], dtype=torch.uint8)
    m, ptr, stride = _row_mask(one, nq, n, CPU)
    assert stride == 0 and ptr == m.data_ptr() and m.dtype == torch.uint8 and torch.equal(m, one)
    per_query = torch.rand(nq, n) < 0.5
    m, ptr, stride = _row_mask(per_query, nq, n, CPU)
    assert stride == n and ptr == m.data_ptr() and m.dtype == torch.uint8 and m.is_contiguous() and torch.equal(m != 0, per_query)
    for bad in (torch.ones(n - 1, dtype=torch.uint8), torch.ones(nq + 1, n, dtype=torch.bool)):
        with pytest.raises(ValueError, match=rf"row_mask must be \[{n}\] or \[{nq}, {n}\], got "):
            _row_mask(bad, nq, n, CPU)


def test_queries_pass_through_or_are_coerced():
    from astts.knn import _as_queries

    q = torch.randn(4, 6)
    assert _as_queries(q, 6, CPU) is q
    for other in (q.double(), torch.randn(6, 4).t()):
        got = _as_queries(other, 6, CPU)
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (4, 6) and torch.equal(got, other.float())
    for bad in (torch.randn(4, 5), torch.randn(6)):
        with pytest.raises(ValueError, match=r"queries must be \[Q, 6\], got "):
            _as_queries(bad, 6, CPU)


def test_every_binder_module_binds_its_headers(tmp_path):
    from astts import _lib, _lib_knn, _lib_knn_grouped, _lib_knn_ivf, _lib_llm, _lib_session

    for mod, paths in ((_lib_knn, [_lib_knn.HEADER_PATH]), (_lib_knn_grouped, [_lib_knn_grouped.HEADER_PATH]),
                       (_lib_knn_ivf, [_lib_knn_ivf.HEADER_PATH]), (_lib_llm, [_lib_llm.HEADER_PATH]),
                       (_lib_session, [_lib_session.HEADER_PATH, _lib_session.FLOW_HEADER_PATH, _lib_session.FLOW_SHARE_HEADER_PATH])):
        want = {}
        for path in paths:
            with open(path) as f:
                want.update(_lib.parse_prototypes(f.read()))
        assert want and mod.signatures() == want and mod.signatures() is mod.signatures()
        lib = mod.load()
        assert lib is _lib.load()
        for name, (res, args) in want.items():
            assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    missing = str(tmp_path / "astts_absent.h")
    signatures, load = _lib.bind_headers(_lib_llm.HEADER_PATH, missing, what="a header that is not there")
    for call in (signatures, load):
        with pytest.raises(_lib.AsttsLibraryMissing, match="astts_absent.h not found") as e:
            call()
        assert missing in str(e.value)


def test_request_parameters_keep_their_two_orders():
    from astts.compat.pymilvus import MilvusClient

    assert MilvusClient._nprobe_of({"nprobe": 3}, {"params": {"nprobe": 5}}) == 5
    both = ({"params": {"radius": 0.2, "range_filter": 0.9}}, {"params": {"radius": 0.4, "range_filter": 0.8}})
    assert MilvusClient._range_of("COSINE", *both) == (0.2, 0.9)      # search_params["params"] before param["params"]
    assert MilvusClient._range_of("COSINE", {"radius": 0.1}, {"params": {"radius": 0.4}}) == (0.4, None)      # ... before flat search_params
    assert MilvusClient._request_param("x", (None, "no dictionary", {"x": None}, {"x": 0}, {"x": 1})) == 0
    assert MilvusClient._request_param("x", ({}, None)) is None
