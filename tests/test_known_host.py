"""CPU: the host side of the known-facts index.  `TSVKGLoader.known_facts()` is the table whose rows ARE the filter rows
`encoded_split` replays per query (the reference's e1rel_to_e2_full.json, data.py:464-469, 494-503), in the layout
coper_set_known_facts takes; `data.known_facts_from_queries` is the same for synthetic query sets."""
import os
import shutil

import numpy as np
import pytest

from coper_amd import data as cdata
from coper_amd.kg_loader import TSVKGLoader


@pytest.fixture(scope="module")
def loader(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("kg")
    for f in ("train.txt", "dev.txt", "test.txt"):
        shutil.copy(os.path.join(golden_dir, "kg_tsv", f), d)
    ld = TSVKGLoader(str(d), "nell-995-test")
    ld.assign_ids()
    return ld


def _check_layout(kf, num_ent, num_rel):
    e1, rel, ip, ix = kf["e1"], kf["rel"], kf["tail_indptr"], kf["tail_idx"]
    assert all(a.dtype == np.int64 for a in (e1, rel, ip, ix))
    assert len(e1) == len(rel) == len(ip) - 1 and len(e1) > 0
    key = e1 * num_rel + rel
    assert np.all(np.diff(key) > 0)                                  # strictly ascending: sorted, no pair twice
    assert e1.min() >= 0 and e1.max() < num_ent and rel.min() >= 0 and rel.max() < num_rel
    assert ip[0] == 0 and ip[-1] == len(ix) and np.all(np.diff(ip) >= 0)
    assert ix.min() >= 0 and ix.max() < num_ent
    down = np.flatnonzero(np.diff(ix) <= 0) + 1                      # a step that does not ascend sits on a row boundary
    assert np.all(np.isin(down, ip))
    return key


def test_known_facts_layout(loader):
    kf = loader.known_facts()
    _check_layout(kf, loader.num_ent, loader.num_rel)
    # the forward half alone: the same rows, without the _reverse relations
    fwd = loader.known_facts(include_inv_relations=False)
    _check_layout(fwd, loader.num_ent, loader.num_rel)
    inv = {i for n, i in loader.relation_ids.items() if n.endswith("_reverse")}
    assert inv and not set(fwd["rel"].tolist()) & inv and set(kf["rel"].tolist()) & inv
    # train alone holds no more than the union
    assert loader.known_facts(splits=("train",))["tail_idx"].size < kf["tail_idx"].size


@pytest.mark.parametrize("split", ["dev", "test"])
def test_every_query_finds_its_filter_row(loader, split):
    kf = loader.known_facts()
    key = kf["e1"] * loader.num_rel + kf["rel"]
    q = loader.encoded_split(split, include_inv_relations=True)
    assert len(q["e1"]) > 0
    pos = np.searchsorted(key, q["e1"] * loader.num_rel + q["rel"])
    assert np.all(pos < len(key)) and np.array_equal(key[pos], q["e1"] * loader.num_rel + q["rel"])
    for b in range(len(q["e1"])):
        want = q["filt_idx"][q["filt_indptr"][b]:q["filt_indptr"][b + 1]]
        got = kf["tail_idx"][kf["tail_indptr"][pos[b]]:kf["tail_indptr"][pos[b] + 1]]
        assert np.array_equal(got, want), b


def test_known_facts_from_queries_takes_the_first_occurrence():
    md = cdata.model_descriptors("nations_cpg")
    q = cdata.synthetic_queries(md, 40, seed=3)
    # plant a repeated pair with ANOTHER row: query 30 asks query 5's (e1, rel)
    q["e1"][30], q["rel"][30] = q["e1"][5], q["rel"][5]
    row5 = q["filt_idx"][q["filt_indptr"][5]:q["filt_indptr"][5 + 1]]
    row30 = q["filt_idx"][q["filt_indptr"][30]:q["filt_indptr"][30 + 1]]
    assert not np.array_equal(row5, row30)
    kf = cdata.known_facts_from_queries(q)
    key = _check_layout(kf, md["num_ent"], md["num_rel"])
    qkey = q["e1"] * md["num_rel"] + q["rel"]
    assert np.array_equal(key, np.unique(qkey))
    seen = set()
    for b in range(40):
        pos = int(np.searchsorted(key, qkey[b]))
        got = kf["tail_idx"][kf["tail_indptr"][pos]:kf["tail_indptr"][pos + 1]]
        first = int(np.flatnonzero(qkey == qkey[b])[0])
        assert np.array_equal(got, q["filt_idx"][q["filt_indptr"][first]:q["filt_indptr"][first + 1]]), b
        seen.add(first)
    assert 30 not in seen and 5 in seen
