"""CPU suite: the host half of the device feature decode (NativeFeaturizer(feat_decode="device")): libmmfeat's feat_span and
mmf_gather_spans, the device-mode batches against the host-mode ones, and the featurizer lease of pipeline.py (LRU, a featurizer one pass holds is
neither evicted nor handed out twice)."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import featurizer as F
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import featurizer_native as N

D = os.path.join(GOLDEN, "featurizer")
VOCAB = os.path.join(D, "vocab_small.txt")
TABLE = F.load_label_table(os.path.join(D, "labels.txt"))


def random_records(n, seed, bits=False, nbs=None):
    """TSV records with num_boxes 0 .. 14 (or ``nbs``); bits=True: the features are random uint32 bit patterns (NaN payloads, infinities, denormals)."""
    rng = np.random.default_rng(seed)
    classes = [int(k) for k in TABLE]
    out = []
    for i in range(n):
        nb = int(nbs[i % len(nbs)]) if nbs is not None else int(rng.integers(0, 15))
        h, w = int(rng.integers(50, 1200)), int(rng.integers(50, 1200))
        boxes = rng.uniform(0, 1, (nb, 4)).astype(np.float32) * np.array([h, w, h, w], np.float32)
        if bits:
            u = rng.integers(0, 1 << 32, (nb, 2048), dtype=np.uint64).astype(np.uint32)
            u[:, :6] = [0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFB00001]    # +-inf, denormals, quiet / signalling NaN payloads
            feats = u.view(np.float32)
        else:
            feats = rng.standard_normal((nb, 2048)).astype(np.float32)
        out.append(F.encode_record(int(rng.integers(1, 1 << 40)), h, w, boxes, feats, rng.choice(classes, nb), "red dress %d" % i, i // 3))
    return out


def _needed(nb):
    return (min(max(int(nb), 0), 10) * 8192 * 4 + 2) // 3


def _golden_lines():
    return open(os.path.join(D, "records.tsv")).read().splitlines()


@pytest.mark.parametrize("source", ["golden", "random"])
def test_feat_span_is_the_sixth_field(source):
    lines = _golden_lines() if source == "golden" else random_records(45, 3, nbs=np.random.default_rng(3).permutation(45) % 15)
    nf = N.NativeFeaturizer(VOCAB, TABLE, "zk", threads=3, feat_decode="device")
    a = nf.featurize(lines)
    data = "".join(lines).encode()
    pos = 0
    for i, l in enumerate(lines):
        b = l.encode()
        fields = b.split(b"\t")
        start = pos + len(b"\t".join(fields[:5])) + 1                 # the 6th field's byte range, from a Python split
        assert (int(a["feat_span"][i, 0]), int(a["feat_span"][i, 1])) == (start, start + len(fields[5])), i
        assert data[start:start + len(fields[5])] == fields[5]
        pos += len(b)
    if source == "random":
        assert set(a["num_boxes"].tolist()) >= {0, 10, 14}


@pytest.mark.parametrize("threads", [1, 7])
def test_gather_spans_copies_the_needed_prefix(threads):
    lines = random_records(64, 5, nbs=np.random.default_rng(5).permutation(64) % 15)
    nf = N.NativeFeaturizer(VOCAB, TABLE, "zk", threads=threads, feat_decode="device")
    a = nf.featurize(lines)
    off, chars = a["feat_char_off"], a["feat_chars"]
    assert off.dtype == np.int64 and a["feat_rows"].dtype == np.int32 and chars.dtype == np.uint8
    assert np.all(off % 16 == 0) and off[0] == 0
    assert np.array_equal(a["feat_rows"], np.minimum(a["num_boxes"], 10))
    need = np.array([_needed(n) for n in a["num_boxes"]])
    assert np.array_equal(off[1:], np.cumsum((need[:-1] + 15) // 16 * 16))
    assert chars.size >= off[-1] + (need[-1] + 15) // 16 * 16            # the last record's final 16-byte load is inside
    for i, l in enumerate(lines):
        field = l.encode().split(b"\t")[5]
        assert bytes(chars[off[i]:off[i] + need[i]]) == field[:need[i]], i


def test_gather_spans_abi():
    lib = N.load()
    h = N.NativeFeaturizer(VOCAB, TABLE, "zk")
    src = b"0123456789abcdefXYZ"
    dst = np.zeros(48, np.uint8)
    s_, l_, o_ = np.array([0, 10, 16], np.int64), np.array([4, 6, 3], np.int64), np.array([0, 16, 32], np.int64)
    assert lib.mmf_gather_spans(h._h, src, s_.ctypes.data, l_.ctypes.data, 3, dst.ctypes.data, o_.ctypes.data, 2) == 0
    assert bytes(dst[:4]) == b"0123" and bytes(dst[16:22]) == b"abcdef" and bytes(dst[32:35]) == b"XYZ" and not dst[4:16].any()
    assert lib.mmf_gather_spans(h._h, None, None, None, 0, None, None, 1) == 0
    bad = np.array([-1], np.int64)
    assert lib.mmf_gather_spans(h._h, src, s_.ctypes.data, bad.ctypes.data, 1, dst.ctypes.data, o_.ctypes.data, 1) == -1
    assert b"negative" in lib.mmf_last_error()
    assert lib.mmf_gather_spans(h._h, src, None, l_.ctypes.data, 1, dst.ctypes.data, o_.ctypes.data, 1) == -1


@pytest.mark.parametrize("model", ["zk", "lds", "lxmert"])
def test_device_mode_batches_equal_host_mode_but_the_features(model):
    lines = random_records(50, 9) + _golden_lines()
    host = N.NativeFeaturizer(VOCAB, TABLE, model, threads=4, pinned=False, reuse_buffers=True, pools=3)
    dev = N.NativeFeaturizer(VOCAB, TABLE, model, threads=4, pinned=False, reuse_buffers=True, pools=3, feat_decode="device")
    feat_key = {"zk": "np_images_features", "lds": "features", "lxmert": "feats"}[model]
    for s2f in (False, True):
        for chunk in (lines[:7], lines, lines[3:20]):             # reused buffer sets, shrinking and growing
            h, d = host.batch(chunk, sen2forest=s2f), dev.batch(chunk, sen2forest=s2f)
            assert h[feat_key] is not None and d[feat_key] is None
            assert set(d) - set(h) == set(N.FEAT_TEXT_KEYS) and set(h) - set(d) == set()
            for k in h:
                if k != feat_key:
                    assert np.array_equal(np.asarray(h[k]), np.asarray(d[k])) and np.asarray(h[k]).dtype == np.asarray(d[k]).dtype, k
            assert len(d["feat_char_off"]) == len(chunk)
    assert dev._caps[0] > 0 and all(p is None or "feats" not in p or p["feats"][0].shape[0] == 0 for p in dev._pools)   # no feats pools


def test_device_mode_keeps_the_size_check():
    lines = random_records(3, 5, nbs=[2, 3, 1])
    f = lines[1].split("\t")
    f[3] = str(int(f[3]) + 1)                                   # num_boxes disagrees with the payloads
    nf = N.NativeFeaturizer(VOCAB, TABLE, "zk", feat_decode="device")
    with pytest.raises(ValueError, match="record 2: .*num_boxes"):
        nf.batch([lines[0], lines[2], "\t".join(f)])
    with pytest.raises(ValueError, match="feat_decode"):
        N.NativeFeaturizer(VOCAB, TABLE, "zk", feat_decode="gpu")


def test_feat_text_layout():
    need, off, size = N.feat_text_layout(np.array([0, 1, 2, 3, 11, -1], np.int32))
    assert need.tolist() == [_needed(n) for n in (0, 1, 2, 3, 11, -1)]
    assert need[1] == 10923 and need[2] == 21846 and need[3] == 32768
    assert off.tolist() == [0, 0, 10928, 32784, 65552, 174784] and size == 174784
    assert N.feat_text_layout(np.zeros(0, np.int32))[2] == 0


def test_featurizer_lease_is_lru_and_a_pass_keeps_its_three(monkeypatch):
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import pipeline
    monkeypatch.setattr(pipeline, "_FEATURIZERS", {})
    monkeypatch.setattr(pipeline, "_BUSY", set())

    def one(threads, model="zk", want_feats=True, feat_decode="host"):
        with pipeline._lease(VOCAB, TABLE, threads, (model, want_feats, feat_decode)) as (nf,):
            return nf
    made = [one(t) for t in range(1, 7)]                                         # six cached keys
    assert one(1) is made[0]                                                     # a hit moves the entry last ...
    extra = one(7)
    assert not made[1]._h and made[0]._h                                        # ... so the miss evicts the least recently used (threads=2)
    # one ensemble pass: three new featurizers leased as score_tsv_native leases them -- none of them may close another
    with pipeline._lease(VOCAB, TABLE, 8, ("zk", True, "device"), ("zk", False, "host"), ("lxmert", False, "host")) as (zk, s2f, lx):
        assert zk._h and s2f._h and lx._h and zk.gather_feats and not s2f.gather_feats
        assert len(pipeline._FEATURIZERS) == 6
    assert one(8, feat_decode="device") is zk
    assert one(8) is not zk                                                      # the mode is part of the key
    # a pass's featurizers never evict each other, even when the cache holds one
    monkeypatch.setattr(pipeline, "_FEATURIZER_CACHE", 1)
    with pipeline._lease(VOCAB, TABLE, 9, ("zk", True, "host"), ("lds", True, "host")) as (a, b):
        assert a._h and b._h and a is not b
        assert len(pipeline._FEATURIZERS) <= 1
    for nf in list(pipeline._FEATURIZERS.values()) + made + [extra, zk, s2f, lx, a, b]:
        nf.close()


def test_featurizer_lease_busy_entries_and_exceptions(monkeypatch):
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import pipeline
    monkeypatch.setattr(pipeline, "_FEATURIZERS", {})
    monkeypatch.setattr(pipeline, "_BUSY", set())
    spec = ("zk", True, "host")
    with pipeline._lease(VOCAB, TABLE, 3, spec) as (a,):
        with pipeline._lease(VOCAB, TABLE, 3, spec) as (b,):                   # busy: a second pass gets a private featurizer ...
            assert b is not a and b._h
        assert not b._h and a._h                                               # ... closed when that pass ends; the cached one is not
        assert list(pipeline._FEATURIZERS.values()) == [a]
    monkeypatch.setattr(pipeline, "_FEATURIZER_CACHE", 1)
    with pipeline._lease(VOCAB, TABLE, 3, spec) as (a2,):
        assert a2 is a
        with pipeline._lease(VOCAB, TABLE, 4, spec) as (c,):                   # a miss while the only entry is busy: not evicted
            assert a._h and c._h and list(pipeline._FEATURIZERS.values()) == [a]
        assert not c._h
    with pytest.raises(RuntimeError, match="mid-pass"):                        # a pass that raises releases its lease
        with pipeline._lease(VOCAB, TABLE, 3, spec) as (d,):
            assert d is a
            raise RuntimeError("mid-pass")
    assert not pipeline._BUSY
    with pipeline._lease(VOCAB, TABLE, 3, spec) as (e,):
        assert e is a
    a.close()
