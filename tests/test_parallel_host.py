"""CPU: coper_amd.parallel.shard_batch -- even slices of a training batch in each of its three label forms."""
import numpy as np
import pytest

from coper_amd.parallel import shard_batch


def _sampled(B=12, L=5, E=50):
    rng = np.random.default_rng(0)
    return dict(e1=rng.integers(0, E, B), rel=rng.integers(0, 4, B), lookup_values=rng.integers(0, E, (B, L)).astype(np.int32),
                e2_multi=rng.random((B, L)).astype(np.float32))


def _dense(B=12, E=50):
    rng = np.random.default_rng(1)
    return dict(e1=rng.integers(0, E, B), rel=rng.integers(0, 4, B), lookup_values=np.zeros((B, 0), np.int32),
                e2_multi=(rng.random((B, E)) < 0.1).astype(np.float32))


def _csr(B=12, E=50, with_rows=True):
    rng = np.random.default_rng(2)
    n_rows = 7 if with_rows else B
    rows = [np.nonzero(rng.random(E) < 0.1)[0] for _ in range(n_rows)]
    b = dict(e1=rng.integers(0, E, B), rel=rng.integers(0, 4, B),
             lab_indptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), lab_idx=np.concatenate(rows).astype(np.int64))
    if with_rows:
        b["lab_row"] = rng.integers(0, n_rows, B).astype(np.int64)
    return b


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("make", [_sampled, _dense, _csr])
def test_concatenated_shards_restore_the_batch(make, world):
    batch = make()
    shards = [shard_batch(batch, r, world) for r in range(world)]
    for s in shards:
        assert sorted(s) == sorted(batch) and len(s["e1"]) == 12 // world
    for k in ("e1", "rel", "lookup_values", "e2_multi", "lab_row"):
        if k in batch:
            assert np.array_equal(np.concatenate([s[k] for s in shards]), batch[k]), k


def test_csr_table_is_shared_not_copied():
    batch = _csr()
    for r in range(3):
        s = shard_batch(batch, r, 3)
        assert s["lab_indptr"] is batch["lab_indptr"] and s["lab_idx"] is batch["lab_idx"]
        assert np.array_equal(s["lab_row"], batch["lab_row"][4 * r:4 * r + 4])


def test_csr_batch_without_lab_row_gets_the_slice_row_numbers():
    batch = _csr(with_rows=False)
    shards = [shard_batch(batch, r, 4) for r in range(4)]
    assert np.array_equal(np.concatenate([s["lab_row"] for s in shards]), np.arange(12))
    assert all(s["lab_indptr"] is batch["lab_indptr"] for s in shards)


def test_torch_batches_are_sliced_as_views():
    import torch
    batch = {k: torch.as_tensor(v) for k, v in _sampled().items()}
    s = shard_batch(batch, 1, 2)
    assert torch.equal(s["e2_multi"], batch["e2_multi"][6:]) and s["e2_multi"].data_ptr() == batch["e2_multi"][6:].data_ptr()


def test_uneven_batch_and_bad_rank_raise():
    with pytest.raises(ValueError, match="evenly"):
        shard_batch(_sampled(B=10), 0, 4)
    with pytest.raises(ValueError):
        shard_batch(_sampled(), 2, 2)
