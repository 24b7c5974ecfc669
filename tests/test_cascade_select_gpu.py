"""GPU suite: mms_cascade_select (csrc/cascade.hip) against ensemble.cascade_keep, entry for entry (kept bytes, kept_list, n_kept, the query counts of
the status word): one row, no row, a query longer than a wavefront, many small interleaved queries, pure ties, odd ids, equal bytes on a repeated
call, and the two flags that keep everything."""
import numpy as np
import pytest
import torch

from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, lib

pytestmark = pytest.mark.gpu


def _select(q, s, keep):
    """the raw call -> (kept uint8 [n], kept_list int32 [n] with -7 where nothing was written, status [4]) as numpy"""
    l = lib.load()
    n = len(q)
    dq = torch.as_tensor(np.ascontiguousarray(q, np.int64)).cuda()
    ds = torch.as_tensor(np.ascontiguousarray(s, np.float32)).cuda()
    kept = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    lst = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ws_bytes = l.mms_cascade_workspace_bytes(n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    rc = l.mms_cascade_select(dq.data_ptr(), ds.data_ptr(), n, keep, kept.data_ptr(), lst.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, l.mms_global_error()
    torch.cuda.synchronize()
    return kept.cpu().numpy()[:n], lst.cpu().numpy()[:n], status.cpu().numpy()


def _check(q, s, keep):
    kept, lst, status = _select(q, s, keep)
    want, want_list = ensemble.cascade_keep(q, s, keep)
    sizes = np.unique(np.asarray(q), return_counts=True)[1]
    assert status.tolist() == [0, len(want_list), len(sizes), int(sizes.max())], (status, keep)
    assert np.array_equal(kept, want.astype(np.uint8)), keep
    assert np.array_equal(lst[:len(want_list)], want_list) and (lst[len(want_list):] == -7).all(), keep
    info = {}
    dk, dl = ensemble.cascade_keep_device(q, s, keep, info=info)                         # the wrapper hands out the same
    assert info == dict(path="device", flags=0, n_kept=len(want_list), queries=len(sizes), largest_query=int(sizes.max()))
    assert dk.dtype == torch.bool and np.array_equal(dk.cpu().numpy(), want) and np.array_equal(dl.cpu().numpy(), want_list)
    return kept, lst


def test_one_row_and_no_row():
    _check(np.array([42], np.int64), np.array([0.3], np.float32), 1)
    _check(np.array([42], np.int64), np.array([0.3], np.float32), 7)
    kept, lst, status = _select(np.zeros(0, np.int64), np.zeros(0, np.float32), 3)       # n = 0: a zero status, nothing else
    assert status.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("keep", [1, 64, 199, 200, 1000])
def test_one_query_longer_than_a_wavefront(keep):
    rng = np.random.default_rng(17)
    s = (rng.integers(0, 50, 200) / 64).astype(np.float32)                               # 200 rows, 50 distinct scores: ties inside and across the 64-lane strides
    _check(np.full(200, 123456789, np.int64), s, keep)


def test_many_small_queries_interleaved():
    rng = np.random.default_rng(23)
    sizes = rng.integers(1, 10, 300)                                                     # 300 queries of 1..9 rows
    q = np.repeat(7000 + np.arange(300, dtype=np.int64), sizes)[rng.permutation(int(sizes.sum()))]
    s = rng.random(len(q)).astype(np.float32)
    _check(q, s, 3)
    _check(np.sort(q), s, 3)                                                             # grouped: the run batching of the query counts


def test_pure_ties_and_signed_zeros():
    q = np.repeat(np.arange(5, dtype=np.int64), 70)
    _check(q, np.full(350, 0.5, np.float32), 4)                                          # all scores equal: row order alone
    s = np.where(np.arange(350) % 2 == 0, 0.0, -0.0).astype(np.float32)                  # -0.0 == +0.0
    kept, lst = _check(q, s, 3)
    assert lst[:3].tolist() == [0, 1, 2]


def test_odd_ids():
    ids = np.array([-2, 1 << 62, 0, -(1 << 63), (1 << 63) - 1], np.int64)
    rng = np.random.default_rng(29)
    q = ids[rng.integers(0, 5, 500)]
    _check(q, rng.standard_normal(500).astype(np.float32), 6)


def test_equal_inputs_give_equal_bytes():
    rng = np.random.default_rng(31)
    q = rng.integers(0, 180, 5000).astype(np.int64)
    s = (rng.integers(0, 4096, 5000) / 4096).astype(np.float32)
    a = _check(q, s, 10)
    b = _select(q, s, 10)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("what", ["nan", "inf", "reserved"])
def test_a_flag_keeps_everything(what):
    rng = np.random.default_rng(37)
    q = rng.integers(0, 20, 700).astype(np.int64)
    s = rng.random(700).astype(np.float32)
    if what == "reserved":
        q[333] = -1
    else:
        s[333] = np.nan if what == "nan" else -np.inf
    flag = ensemble.CASCADE_FLAG_RESERVED_ID if what == "reserved" else ensemble.CASCADE_FLAG_NON_FINITE
    kept, lst, status = _select(q, s, 2)
    assert status[0] == flag and status[1] == 700
    assert (kept == 1).all() and np.array_equal(lst, np.arange(700, dtype=np.int32))
    info = {}
    dk, dl = ensemble.cascade_keep_device(q, s, 2, info=info)                            # served by the host form
    assert info["path"] == "host" and info["flags"] == flag
    if what != "nan":
        want = ensemble.cascade_keep(q, s, 2)
        assert np.array_equal(dk.cpu().numpy(), want[0]) and np.array_equal(dl.cpu().numpy(), want[1])
