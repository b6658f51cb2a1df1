"""The reference of the known-facts tests checked against a reference of its own (no GPU).

`tests.helpers.known_filter_np` is what every lookup of tests/test_gpu_known*.py is compared with.  It finds a query's row by
`searchsorted` over the keys e1 * num_rel + rel -- the idea of the kernel it judges.  Here it is compared with
`known_filter_brute`: a dict {(e1, rel): list} and a Python loop, no key and no search, on the crafted indexes of the GPU tests."""
import numpy as np
import pytest

from coper_amd import data as cdata
from tests.helpers import empty_row_indexes, geometry_index, known_filter_brute, known_filter_np, known_index, known_probe_queries

MD = cdata.model_descriptors("fb15k237_plain", num_ent=4099)


def _indexes():
    out = dict(empty_row_indexes(MD))
    out["gather geometry"] = geometry_index(MD)[0]
    return out


@pytest.mark.parametrize("name", sorted(_indexes()))
def test_numpy_filter_equals_brute_force(name):
    kf = _indexes()[name]
    for seed in range(3):
        e1, rel = known_probe_queries(kf, MD, seed)
        E, R = MD["num_ent"], MD["num_rel"]
        outside = (e1 < 0) | (e1 >= E) | (rel < 0) | (rel >= R)
        assert outside.sum() == 7 and len(e1) > 2 * len(kf["e1"])
        ip, ix = known_filter_np(kf, MD, e1, rel)
        wip, wix = known_filter_brute(kf, MD, e1, rel)
        assert ip.dtype == np.int64 and ix.dtype == np.int64
        bad = np.flatnonzero(ip != wip)
        assert bad.size == 0, "%s: indptr differs first at query %d: %d, brute force %d" % (name, bad[0] - 1, ip[bad[0]], wip[bad[0]])
        assert np.array_equal(ix, wix), name
        assert np.all(np.diff(ip)[outside] == 0)
        # the probe is no vacuous one: every non-empty row of the index is in the answer, absent pairs are among the queries
        held = set(zip(kf["e1"].tolist(), kf["rel"].tolist()))
        asked = set(zip(e1.tolist(), rel.tolist()))
        assert held <= asked and len(asked - held) > 0
        assert ip[-1] >= 2 * len(kf["tail_idx"])


def test_brute_force_by_hand():
    """The brute-force oracle itself, on an index small enough to write the answer down."""
    kf = known_index({(1, 1): [5, 9], (1, 2): [], (1, 3): [3, 4]})
    assert kf["tail_indptr"].tolist() == [0, 2, 2, 4] and kf["tail_idx"].tolist() == [5, 9, 3, 4]
    E, R = MD["num_ent"], MD["num_rel"]
    e1 = [1, 1, 1, 1, 0, E, 1, -1, 1]
    rel = [3, 2, 1, 0, 1, 1, R, 1, 3]
    for f in (known_filter_brute, known_filter_np):
        ip, ix = f(kf, MD, e1, rel)
        assert ip.tolist() == [0, 2, 2, 4, 4, 4, 4, 4, 4, 6] and ix.tolist() == [3, 4, 5, 9, 3, 4]
