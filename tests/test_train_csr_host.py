"""Host-side tests of 1-vs-all training from sparse labels (include/coper_hip.h: coper_train_step_csr): the `labels="csr"` mode of
`OneVsAllTrainDataset` against its dense mode, the loaders' `sparse_labels` switch, and the ctypes side of the two new entry points."""
import os
import re

import numpy as np
import pytest

from coper_amd import _lib
from coper_amd.data import OneVsAllTrainDataset, SyntheticKGLoader, _ascending_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _densify(batch, num_ent):
    ip, ix, row = np.asarray(batch["lab_indptr"]), np.asarray(batch["lab_idx"]), np.asarray(batch["lab_row"])
    out = np.zeros((len(row), num_ent), np.float32)
    for b, r in enumerate(row):
        out[b, ix[ip[r]:ip[r + 1]]] = 1.0
    return out


def _samples(E=23, n_rec=9, seed=0):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(E, size=int(rng.integers(1, 6)), replace=False)) for _ in range(n_rec)]
    return dict(e1=rng.integers(0, E, n_rec), rel=rng.integers(0, 4, n_rec),
                tail_indptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                tail_idx=np.concatenate(rows).astype(np.int64))


@pytest.mark.parametrize("device", [None, "cpu"])
def test_csr_dataset_yields_the_dense_datasets_records_and_labels(device):
    """Same seed, same records: e1 / rel equal batch by batch, and densifying (lab_row, lab_indptr, lab_idx) gives the dense e2_multi.
    Nine records in batches of 16 out of a shuffle buffer of 10: the record stream repeats, so a batch holds a record more than once."""
    E, s = 23, _samples()
    dense = iter(OneVsAllTrainDataset(s, E, batch_size=16, seed=4, shuffle_buffer=10, device=device))
    csr = iter(OneVsAllTrainDataset(s, E, batch_size=16, seed=4, shuffle_buffer=10, device=device, labels="csr"))
    repeated = False
    shared = None
    for _ in range(5):
        a, b = next(dense), next(csr)
        assert sorted(b) == ["e1", "e2", "lab_idx", "lab_indptr", "lab_row", "rel"]
        if device is None:
            assert all(isinstance(v, np.ndarray) for v in b.values())
        assert np.array_equal(np.asarray(a["e1"]), np.asarray(b["e1"])) and np.array_equal(np.asarray(a["rel"]), np.asarray(b["rel"]))
        assert np.array_equal(np.asarray(b["e2"]), np.full(16, -1)) and np.asarray(b["lab_row"]).dtype == np.int64
        assert np.array_equal(_densify(b, E), np.asarray(a["e2_multi"]))
        repeated |= len(set(np.asarray(b["lab_row"]).tolist())) < 16
        # the table is shared: the same objects in every batch, nothing built per batch
        if shared is None:
            shared = (b["lab_indptr"], b["lab_idx"])
        assert b["lab_indptr"] is shared[0] and b["lab_idx"] is shared[1]
    assert repeated


def test_csr_dataset_sorts_rows_that_are_not_ascending():
    """The membership search of the loss kernel needs strictly ascending rows: a table that is not (records of a TFRecord directory are
    stored in file order) is sorted once, with repeats dropped; a sorted one is passed through as it is."""
    ip, ix = np.array([0, 3, 3, 5], np.int64), np.array([5, 2, 2, 1, 0], np.int64)
    ip2, ix2 = _ascending_rows(ip, ix)
    assert ip2.tolist() == [0, 2, 2, 4] and ix2.tolist() == [2, 5, 0, 1]
    s = _samples()
    ip3, ix3 = _ascending_rows(s["tail_indptr"], s["tail_idx"])
    assert ip3 is s["tail_indptr"] and ix3 is s["tail_idx"]
    ds = OneVsAllTrainDataset(dict(e1=[0, 1, 2], rel=[0, 0, 0], tail_indptr=ip, tail_idx=ix), 7, batch_size=3, labels="csr")
    b = next(iter(ds))
    want = np.zeros((3, 7), np.float32)
    for i, r in enumerate(b["lab_row"]):
        want[i, ix[ip[r]:ip[r + 1]]] = 1.0
    assert np.array_equal(_densify(b, 7), want)
    with pytest.raises(ValueError):
        OneVsAllTrainDataset(s, 23, batch_size=3, labels="coo")


def test_loaders_take_sparse_labels(tmp_path):
    from coper_amd import data as cdata
    md = cdata.model_descriptors("nations_cpg", num_ent=60, num_rel=8)
    ld = SyntheticKGLoader("nations_plain_like", seed=1, queries=100, md=md)
    ds = ld.train_dataset(None, batch_size=8, num_labels=None, sparse_labels=True)
    assert isinstance(ds, OneVsAllTrainDataset) and ds.labels == "csr"
    assert ld.train_dataset(None, batch_size=8, num_labels=None).labels == "dense"      # the default stays dense
    b, a = next(iter(ds)), next(iter(ld.train_dataset(None, batch_size=8, num_labels=None)))
    assert np.array_equal(_densify(b, ld.num_ent), a["e2_multi"]) and np.array_equal(a["e1"], b["e1"])
    from coper_amd.kg_loader import TFRecordKGLoader, TSVKGLoader
    import inspect
    for cls in (TSVKGLoader, TFRecordKGLoader):
        assert inspect.signature(cls.train_dataset).parameters["sparse_labels"].default is False


def test_the_csr_entry_points_are_declared_and_prototyped():
    with open(os.path.join(ROOT, "include", "coper_hip.h")) as f:
        header = f.read()
    for name, n_args in (("coper_train_step_csr", 10), ("coper_train_forward_csr", 12)):
        decl = re.search(r"COPER_API int %s\(([^;]*)\);" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == n_args
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args
    # one_vs_all_chunk took the first reserved slot: the struct is as large as it was, the fields in front of it where they were
    import ctypes as C
    cfg = _lib.coper_train_config
    assert C.sizeof(cfg) == 4 * 20 and cfg.one_vs_all_chunk.offset == 4 * 13 and cfg.reserved.offset == 4 * 14
    assert "int32_t one_vs_all_chunk;" in header and "int32_t reserved[6];" in header
    assert _lib.coper_train_config().one_vs_all_chunk == 0
