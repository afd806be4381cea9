"""GPU tests of the seams between the three search forms of astts.knn.StyleBank (plain, grouped, IVF), which share one query
coercion, one output allocation, one row-mask marshalling, one workspace class and one device switch.

One 300 x 64 fp16 bank (COSINE: one selection segment, the register scan).  The references are those of the three kNN test files:
oracle.knn for the plain search (ids equal, scores within 1e-6), tests/knn_grouped_ref.py for the grouped ids, and the plain search,
bit for bit, for an IVF search that probes every list."""
import functools

import numpy as np
import pytest
import torch

import knn_grouped_ref as gref
from oracle import knn as oknn

pytestmark = pytest.mark.gpu

N, D, SCORE_ATOL = 300, 64, 1e-6


@functools.lru_cache(maxsize=None)
def case():
    """-> (bank fp16 [305, 64] -- the tests' bank is its first 300 rows, the other 5 are appended --, queries fp32 [70, 64])"""
    rng = np.random.default_rng(41)
    bank = rng.standard_normal((N + 5, D)).astype(np.float16)
    q = (bank[rng.integers(0, N, 70)].astype(np.float32) + 0.5 * rng.standard_normal((70, D))).astype(np.float32)
    bank.setflags(write=False)
    q.setflags(write=False)
    return bank, q


def new_bank():
    from astts.knn import StyleBank

    sb = StyleBank(case()[0][:N].copy())
    assert sb.scan_plane_exact and sb.route(2, 3) == [(2, "REGISTER", "FUSED")]
    return sb


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def plain_ok(got, q, k, mask=None, rows=N):
    """a plain (or full-probe IVF) result against oracle.knn over the first ``rows`` rows"""
    idx, sc = (t.cpu().numpy() for t in got)
    eidx, esc = oknn.knn_search(case()[0][:rows], q, k, row_mask=mask)
    assert np.array_equal(idx, eidx), np.argwhere(idx != eidx)[:5].tolist()
    assert np.allclose(sc, esc, atol=SCORE_ATOL, rtol=0)


def grouped_ok(got, q, limit, group_size, groups, mask=None, rows=N):
    idx, sc = (t.cpu().numpy() for t in got)
    eidx, esc = gref.grouped_search(case()[0][:rows], q, limit, group_size, groups, "COSINE", row_mask=mask)
    assert np.array_equal(idx, eidx), np.argwhere(idx != eidx)[:5].tolist()
    assert np.allclose(sc[idx >= 0], esc[idx >= 0], atol=SCORE_ATOL, rtol=0) and np.all(np.isneginf(sc[idx < 0]))


def same_bits(a, b):
    assert torch.equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_a_larger_search_replaces_the_workspace_under_a_known_size():
    from astts.knn import route_passes

    sb = new_bank()
    _, q = case()
    q2, q70 = dev(q[:2]), dev(q)
    mask = np.random.default_rng(5).random((70, N)) < 0.6
    mt = dev(mask)
    assert route_passes(N, D, 70, 40) == 2
    first = sb.search_device(q2, 3)                                     # no synchronisation between these three
    large = sb.search_device(q70, 40, row_mask=mt)
    out_idx = torch.full((2, 3), -7, dtype=torch.int64, device="cuda")
    out_score = torch.full((2, 3), float("nan"), dtype=torch.float32, device="cuda")
    again = sb.search_device(q2, 3, out_idx=out_idx, out_score=out_score)
    assert again[0] is out_idx and again[1] is out_score
    plain_ok(first, q[:2], 3)
    plain_ok(large, q, 40, mask)
    plain_ok(again, q[:2], 3)
    same_bits(again, first)
    assert 0 <= sb.last_fallbacks() <= 2                                # (of the last search's two queries; read behind the workspace's base)
    sb.close()


def test_the_three_workspaces_do_not_disturb_each_other():
    sb = new_bank()
    _, q = case()
    q2 = dev(q[:2])
    groups = (np.arange(N) % 5).astype(np.int32)
    first = sb.search_device(q2, 3)
    grouped = sb.search_grouped_device(q2, 2, 2, dev(groups), 5)
    assert sb.last_rounds >= 1
    assert sb.build_index(4)["nlist"] == 4
    ivf = sb.search_ivf_device(q2, 3, nprobe=4)
    again = sb.search_device(q2, 3)
    plain_ok(first, q[:2], 3)
    grouped_ok(grouped, q[:2], 2, 2, groups)
    same_bits(ivf, first)
    same_bits(again, first)
    sb.close()


def test_one_mask_function_behind_three_searches():
    sb = new_bank()
    sb.build_index(4)
    bank, q = case()
    q2 = dev(q[:2])
    groups = (np.arange(N) % 5).astype(np.int32)
    best = oknn.knn_search(bank[:N], q[:2], 1)[0][:, 0]
    shared = np.ones(N, np.uint8)
    shared[best] = 0                                                    # [N] uint8: neither query's best row
    own = np.ones((2, N), bool)
    own[np.arange(2), best] = False                                     # [Q, N] bool: each query without its own best row
    for mask in (shared, own):
        mt = dev(mask)
        assert mt.dtype == (torch.uint8 if mask is shared else torch.bool)
        plain = sb.search_device(q2, 3, row_mask=mt)
        plain_ok(plain, q[:2], 3, mask)
        assert not np.any(plain[0].cpu().numpy() == best[:, None])
        grouped_ok(sb.search_grouped_device(q2, 2, 2, dev(groups), 5, row_mask=mt), q[:2], 2, 2, groups, mask)
        same_bits(sb.search_ivf_device(q2, 3, nprobe=4, row_mask=mt), plain)
    sb.close()


def test_append_forgets_the_sizes_and_assigns_the_new_rows():
    sb = new_bank()
    sb.build_index(4)
    bank, q = case()
    q2 = dev(q[:2])
    q2_new = np.ascontiguousarray(bank[N:N + 2].astype(np.float32))     # two of the rows to come: their own best hits afterwards
    groups = (np.arange(N + 5) % 5).astype(np.int32)
    sb.search_device(q2, 3), sb.search_grouped_device(q2, 2, 2, dev(groups[:N]), 5), sb.search_ivf_device(q2, 3, nprobe=4)
    assert sb.append(bank[N:].copy()) == N and sb.n == N + 5 and sb.index_info()["n_indexed"] == N + 5
    for qn in (q[:2], q2_new):
        qt = dev(qn)
        plain = sb.search_device(qt, 3)
        plain_ok(plain, qn, 3, rows=N + 5)
        grouped_ok(sb.search_grouped_device(qt, 2, 2, dev(groups), 5), qn, 2, 2, groups, rows=N + 5)
        same_bits(sb.search_ivf_device(qt, 3, nprobe=4), plain)
    assert sb.search_device(dev(q2_new), 1)[0].cpu().tolist() == [[N], [N + 1]]
    sb.close()


def test_a_search_with_another_device_current():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: the bank's device is the only one")
    sb = new_bank()                                                     # on the current device
    sb.build_index(4)
    _, q = case()
    home, other = sb.device.index, (sb.device.index + 1) % torch.cuda.device_count()
    q2 = dev(q[:2]).to(sb.device)
    try:
        torch.cuda.set_device(other)
        plain = sb.search_device(q2, 3)
        ivf = sb.search_ivf_device(q2, 3, nprobe=4)
        assert torch.cuda.current_device() == other
    finally:
        torch.cuda.set_device(home)
    plain_ok(plain, q[:2], 3)
    same_bits(ivf, plain)
    sb.close()
