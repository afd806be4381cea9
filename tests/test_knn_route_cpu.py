"""Which launches a kNN search takes, asked of the library itself (astts_knn_route: a host query, no GPU, no handle -- the plan
astts_knn_search runs).  Cases are (n, d, nq, k); G(qg, n) = ceil(qg / 64) * ceil(n / 64) >= 256 with qg = min(nq, 256) is the GEMM
threshold (a group also needs >= 64 queries); defaults: no row mask, aligned queries, no ASTTS_KNN_* switch set, ring kernels on."""
import pytest


@pytest.fixture(scope="module")
def knn():
    from astts import knn

    return knn


def _one(knn, shape, **kw):
    """The route of a search that is one query group, with its passes: (scan, finish, passes)."""
    groups = knn.route(*shape, **kw)
    assert len(groups) == 1 and groups[0][0] == shape[2], groups
    return groups[0][1], groups[0][2], knn.route_passes(*shape)


def test_small_banks(knn):
    assert _one(knn, (1000, 6144, 8, 3)) == ("DIRECT", "FUSED", 1)
    assert _one(knn, (1000, 6144, 8, 3), aligned=False) == ("REGISTER", "FUSED", 1)
    assert _one(knn, (1000, 6208, 8, 3)) == ("REGISTER", "FUSED", 1)               # d is not a multiple of 128
    assert _one(knn, (1000, 8320, 8, 3)) == ("REGISTER", "FUSED", 1)               # d above 8192
    assert _one(knn, (1000, 6144, 33, 3)) == ("REGISTER", "FUSED", 1)              # more than one query tile
    assert _one(knn, (1000, 6144, 8, 40)) == ("REGISTER", "SELECT", 2)


def test_gemm_threshold_and_single_segment_banks(knn):
    assert _one(knn, (8193, 64, 8, 3)) == ("REGISTER", "SELECT_MERGE", 1)          # two segments
    assert _one(knn, (8192, 64, 8, 3)) == ("REGISTER", "FUSED", 1)                 # one segment; d % 128 != 0 excludes DIRECT
    assert _one(knn, (4096, 64, 256, 3)) == ("GEMM", "FUSED", 1)                   # G = 256
    assert _one(knn, (4032, 64, 256, 3)) == ("REGISTER", "FUSED", 1)               # G = 252
    assert knn.route(4096, 64, 300, 3) == [(150, "GEMM", "SELECT")] * 2


def test_block_maximum_range(knn):
    from astts import ops

    shape = (8200, 128, 128, 5)
    assert _one(knn, shape) == ("GEMM_BLOCKS", "BLOCKS", 1)
    assert _one(knn, shape, masked=True) == ("GEMM", "STREAM", 1)
    assert _one(knn, (8200, 128, 128, 33)) == ("GEMM", "STREAM", 2)
    ops.set_gemm_ring_mode(0)           # the ring kernels carry the block-maximum epilogue: without them the plain GEMM and the stream
    try:
        assert _one(knn, shape) == ("GEMM", "STREAM", 1)
    finally:
        ops.set_gemm_ring_mode(-1)
    assert _one(knn, shape) == ("GEMM_BLOCKS", "BLOCKS", 1)
    assert _one(knn, (8200, 128, 64, 5)) == ("REGISTER", "SELECT_MERGE", 1)        # G = 129
    assert _one(knn, (524288, 64, 64, 3)) == ("GEMM_BLOCKS", "BLOCKS", 1)          # 8192 blocks of 64 rows: one selection segment of maxima
    assert _one(knn, (524289, 64, 64, 3)) == ("GEMM", "STREAM", 1)


def test_group_splitting(knn):
    from astts import _lib

    assert knn.route(20000, 256, 300, 5) == [(150, "GEMM_BLOCKS", "BLOCKS")] * 2
    # the first query count whose equal groups of <= 256 leave a tail below 64: 193 x 256 + 63
    assert knn.route(20000, 256, 49471, 5) == [(256, "GEMM_BLOCKS", "BLOCKS")] * 193 + [(63, "REGISTER", "SELECT_MERGE")]
    lib = _lib.load()
    assert lib.astts_knn_route(20000, 256, 300, 5, 0, 1, 1, None, None, None, None) == _lib.OK
    for group in (2, -1):               # past the last group
        assert lib.astts_knn_route(20000, 256, 300, 5, 0, 1, group, None, None, None, None) == _lib.ERR_INVALID
    with pytest.raises(_lib.AsttsError):
        knn.route(20000, 256, 300, 0)
