#!/usr/bin/env python3
"""Answering queries: which entities complete (e1, rel, ?).

    python examples/predict_topk.py [--k 5] [--queries 6] [--score-mode bf16x3]

Loads the synthetic FB15k-237-shaped CoPER-ConvE model, asks for the k best tails of a handful of (e1, rel) pairs -- once raw, once
with the known answers of each pair filtered out, given as a CSR, once with the same known answers looked up in the index the model
keeps on the device (`set_known_facts`: the caller then holds bare (e1, rel) pairs) -- and prints the entity ids with their logits.  The answer is exact in both score
modes: values, set and order are those of the fp32 chain (include/coper_hip.h: coper_predict_topk); no [B, num_entities] matrix is
formed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from coper_amd import data as cdata  # noqa: E402
from coper_amd.models import ConvE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--queries", type=int, default=6)
    ap.add_argument("--score-mode", default="bf16x3", choices=["bf16x3", "f32"])
    a = ap.parse_args()
    md = cdata.model_descriptors("fb15k237_cpg")
    m = ConvE(md, device="cuda:0", score_mode=a.score_mode).load_parameters(cdata.synthetic_params(md, 0)).prepare()
    q = cdata.synthetic_queries(md, a.queries, seed=0)
    raw_v, raw_i = m.predict_topk(q["e1"], q["rel"], a.k)
    fil_v, fil_i = m.predict_topk(q["e1"], q["rel"], a.k, q["filt_indptr"], q["filt_idx"])
    # the known facts of the KG, set once (a KG on disk: TSVKGLoader.known_facts()); every later batch is three ids per query
    m.set_known_facts(**cdata.known_facts_from_queries(q))
    res_v, res_i = m.predict_topk_known(q["e1"], q["rel"], a.k)
    for b in range(a.queries):
        known = q["filt_idx"][q["filt_indptr"][b]:q["filt_indptr"][b + 1]].tolist()
        print("(e1 = %d, rel = %d, ?)   known answers: %s" % (q["e1"][b], q["rel"][b], known))
        print("   raw      " + "  ".join("%d (%.4f)" % (i, v) for i, v in zip(raw_i[b].tolist(), raw_v[b].tolist())))
        print("   filtered " + "  ".join("%d (%.4f)" % (i, v) for i, v in zip(fil_i[b].tolist(), fil_v[b].tolist())))
        print("   resident " + "  ".join("%d (%.4f)" % (i, v) for i, v in zip(res_i[b].tolist(), res_v[b].tolist())))
    print("statistics:", m.predict_stats())
    m.close()


if __name__ == "__main__":
    main()
