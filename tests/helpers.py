"""Shared by the GPU tests: the logits that DEFINE a mode's ranks.

f32 mode: the mode's own logits (they are the documented fp32 chain, bit for bit).  bf16x3 mode: its count kernel decides
only comparisons wider than its own error; closer ones go to the fp32 chain (the exact band), so its ranks and tie counts
are those of the C restatement of that chain applied to the mode's h -- the mode's own logits (score_all, top-k values)
stay within the 1e-3 gate of it but do not define the ranks."""
import numpy as np

PLANT_TOP = 64            # planted_queries: the target and the planted known answers come from the row's top 64
PLANT_MAX_KNOWN = 8       # ... 0 .. 8 known answers among the other 63
PLANT_MAX_EXTRA = 5       # ... 0 .. 5 further known answers drawn uniformly over the table


def top_of_rows(lg64, n):
    """[Q, n] ids: the first n positions of every row's DESCENDING order under a stable sort (ties: ascending id), without
    sorting the rows: the entities at or above the row's n-th largest value, ordered by (-value, id)."""
    lg64 = np.asarray(lg64, np.float64)
    Q, E = lg64.shape
    n = min(int(n), E)
    kth = np.partition(lg64, E - n, axis=1)[:, E - n]
    out = np.empty((Q, n), np.int64)
    for i in range(Q):
        cand = np.flatnonzero(lg64[i] >= kth[i])                       # ascending ids: the stable sort keeps them so among equals
        out[i] = cand[np.argsort(-lg64[i, cand], kind="stable")[:n]]
    return out


def planted_queries(md, lg64, e1, rel, seed):
    """Queries whose target sits near the top of the ranking, as a trained model's do (synthetic_queries draws e2 uniformly:
    its ranks are uniform over the table and 14 of 20,480 land in the top 10).

    lg64 [Q, |E|]: the float64 oracle's logits of the (e1, rel) queries.  Per query, from ONE default_rng(seed):
      target         e2 = the entity at position pos of the row's descending order (stable sort), pos in [0, 64) drawn with
                     weight 1 / (1 + pos);
      known answers  0 .. 8 of the other 63 entities of the top 64, without replacement (a trained model's known answers are the
                     best-scoring entities of the row: some above the target, some below, some next to it);
      extras         0 .. 5 further entities, uniform over the table;
      filter row     known answers, extras and e2 itself, sorted and unique (the reference's e2_multi holds the target too).
    Returns (q, (indptr, idx)): the usual dict e1 / rel / e2 / filt_indptr / filt_idx, and the same CSR WITHOUT e2 in its own
    row -- the filter of a prediction, which exempts no entity (predict_topk)."""
    rng = np.random.default_rng(seed)
    lg64 = np.asarray(lg64, np.float64)
    Q, E = lg64.shape
    assert E == int(md["num_ent"]) and len(e1) == Q and len(rel) == Q
    top = top_of_rows(lg64, PLANT_TOP)
    n_top = top.shape[1]
    w = 1.0 / (1.0 + np.arange(n_top))
    w /= w.sum()
    e2 = np.empty(Q, np.int64)
    rows, rows_wo = [], []
    for i in range(Q):
        pos = int(rng.choice(n_top, p=w))
        e2[i] = top[i, pos]
        others = np.delete(top[i], pos)
        known = rng.choice(others, min(int(rng.integers(0, PLANT_MAX_KNOWN + 1)), len(others)), replace=False)
        extra = rng.integers(0, E, int(rng.integers(0, PLANT_MAX_EXTRA + 1)), dtype=np.int64)
        row = np.unique(np.concatenate([known, extra, e2[i:i + 1]]))
        rows.append(row)
        rows_wo.append(row[row != e2[i]])
    q = dict(e1=np.asarray(e1, np.int64).copy(), rel=np.asarray(rel, np.int64).copy(), e2=e2)
    q["filt_indptr"], q["filt_idx"] = rows_to_csr(rows)
    return q, rows_to_csr(rows_wo)


def rows_to_csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows).astype(np.int64) if len(rows) and indptr[-1] else np.zeros(0, np.int64)
    return indptr, idx


def csr_rows(indptr, idx, sel=None):
    """The rows of a CSR as a list of arrays (all of them, or those of `sel`)."""
    sel = range(len(indptr) - 1) if sel is None else sel
    return [np.asarray(idx[indptr[i]:indptr[i + 1]], np.int64) for i in sel]


def take_queries(q, sel, csr=None):
    """The queries `sel` of a query dict (with `csr` = (indptr, idx): that filter in place of the dict's own)."""
    sel = np.asarray(sel, np.int64)
    ip, ix = csr if csr is not None else (q["filt_indptr"], q["filt_idx"])
    out = dict(e1=q["e1"][sel], rel=q["rel"][sel], e2=q["e2"][sel])
    out["filt_indptr"], out["filt_idx"] = rows_to_csr(csr_rows(ip, ix, sel))
    return out


def concat_queries(parts):
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("e1", "rel", "e2")}
    out["filt_indptr"], out["filt_idx"] = concat_csr([(p["filt_indptr"], p["filt_idx"]) for p in parts])
    return out


def concat_csr(csrs):
    base, ips, ixs = 0, [np.zeros(1, np.int64)], []
    for ip, ix in csrs:
        ips.append(np.asarray(ip[1:], np.int64) + base)
        ixs.append(np.asarray(ix, np.int64))
        base += int(ip[-1])
    return np.concatenate(ips), (np.concatenate(ixs) if ixs else np.zeros(0, np.int64))


def float64_rank_facts(lg64, q, band=0.0):
    """What the float64 oracle says about filtered ranks, per query (NumPy, int64 / float64 [Q]):
      rank      1 + #(unfiltered others > t)                      (metrics.py:44-50 on the float64 row)
      lo, hi    1 + #(others > t + band), 1 + #(others > t - band): the ranks an arithmetic within band / 2 per logit may report
      gap       the distance of the closest unfiltered competitor to the target
      above, inside, below   known answers (the filter row without e2) above t + band, within band of t, below t - band"""
    lg64 = np.asarray(lg64, np.float64)
    Q, E = lg64.shape
    ip, ix, e2 = q["filt_indptr"], q["filt_idx"], q["e2"]
    rows = np.repeat(np.arange(Q), np.diff(ip))
    t = lg64[np.arange(Q), e2]
    known = ix != e2[rows]
    d = lg64[rows[known], ix[known]] - t[rows[known]]
    count = lambda m: np.bincount(rows[known][m], minlength=Q).astype(np.int64)
    out = dict(above=count(d > band), inside=count(np.abs(d) <= band), below=count(d < -band))
    others = lg64 - t[:, None]                           # (a copy: the caller's logits stay as they are)
    others[rows, ix] = -np.inf
    others[np.arange(Q), e2] = -np.inf
    out["rank"] = 1 + (others > 0).sum(1)
    out["lo"] = 1 + (others > band).sum(1)
    out["hi"] = 1 + (others > -band).sum(1)
    others[rows, ix] = np.inf                            # (|.| of a filtered entity must not be the minimum)
    others[np.arange(Q), e2] = np.inf
    out["gap"] = np.abs(others).min(1)
    return out


def rank_defining_logits(O, m, h, params):
    if m.score_mode == "f32":
        return m.score_all(h).cpu().numpy()
    lo, hi = m.shard
    return O.score_chain(np.ascontiguousarray(h.cpu().numpy()), np.ascontiguousarray(np.asarray(params["ent_emb"], np.float32)[lo:hi]),
                         np.ascontiguousarray(np.asarray(params["pred_bias"], np.float32)[lo:hi]))


# ---------------------------------------------------------------------------------------------------- the known-facts index
def known_filter_np(kf, md, e1, rel):
    """The CSR of the queries (e1, rel) from the host index: absent keys and ids outside the model's range give empty rows."""
    E, R = int(md["num_ent"]), int(md["num_rel"])
    e1, rel = np.asarray(e1, np.int64), np.asarray(rel, np.int64)
    key = kf["e1"] * R + kf["rel"]
    ok = (e1 >= 0) & (e1 < E) & (rel >= 0) & (rel < R)
    qk = np.where(ok, e1 * R + rel, -1)
    pos = np.minimum(np.searchsorted(key, qk), len(key) - 1)
    ok &= key[pos] == qk
    rows = [kf["tail_idx"][kf["tail_indptr"][p]:kf["tail_indptr"][p + 1]] if f else np.zeros(0, np.int64) for p, f in zip(pos, ok)]
    ip = np.zeros(len(e1) + 1, np.int64)
    ip[1:] = np.cumsum([len(r) for r in rows])
    return ip, (np.concatenate(rows).astype(np.int64) if len(rows) and ip[-1] else np.zeros(0, np.int64))


def known_filter_brute(kf, md, e1, rel):
    """What known_filter_np computes, without a search and without a key: a dict {(e1, rel): list of tails} filled row by row from
    the index, and one Python loop over the queries."""
    E, R = int(md["num_ent"]), int(md["num_rel"])
    table = {}
    for i in range(len(kf["e1"])):
        pair = (int(kf["e1"][i]), int(kf["rel"][i]))
        assert pair not in table
        table[pair] = [int(t) for t in kf["tail_idx"][int(kf["tail_indptr"][i]):int(kf["tail_indptr"][i + 1])]]
    ip, ix = [0], []
    for a, r in zip(e1, rel):
        a, r = int(a), int(r)
        if 0 <= a < E and 0 <= r < R:
            ix.extend(table.get((a, r), []))
        ip.append(len(ix))
    return np.array(ip, np.int64), np.array(ix, np.int64)


def known_index(rows):
    """{(e1, rel): tails} -> dict(e1, rel, tail_indptr, tail_idx), rows ascending by (e1, rel); a row may be empty."""
    pairs = sorted(rows)
    ip = np.zeros(len(pairs) + 1, np.int64)
    ip[1:] = np.cumsum([len(rows[p]) for p in pairs])
    tails = [np.asarray(rows[p], np.int64) for p in pairs]
    return dict(e1=np.array([p[0] for p in pairs], np.int64), rel=np.array([p[1] for p in pairs], np.int64), tail_indptr=ip,
                tail_idx=np.concatenate(tails) if ip[-1] else np.zeros(0, np.int64))


GEOMETRY_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
GEOMETRY_ONES = 300           # further one-tail rows: a wave of 64 and a workgroup of 256 DIFFERENT one-entry owners


def geometry_index(md):
    """The index of the gather-geometry cases: an empty row at the first possible key, in the middle and at the last possible key; a
    row of every length of GEOMETRY_LENGTHS; GEOMETRY_ONES further one-tail rows.  Returns (index, names): names maps a row's length
    (the rows of GEOMETRY_LENGTHS), ("one", i), "empty_first" / "empty_mid" / "empty_last" and "absent" (a pair between two rows
    that the index does not hold) to the pair (e1, rel)."""
    E, R = int(md["num_ent"]), int(md["num_rel"])
    assert E >= 1200 + GEOMETRY_ONES and R >= 8
    rng = np.random.default_rng(23)
    rows, names = {}, {}
    for i, n in enumerate(GEOMETRY_LENGTHS):
        names[n] = (10 + 3 * i, (5 * i) % R)
        rows[names[n]] = np.sort(rng.choice(E, n, replace=False))
    for i in range(GEOMETRY_ONES):
        names[("one", i)] = (1000 + i, i % 7)
        rows[names[("one", i)]] = [(i * 37 + 11) % E]
    names.update(empty_first=(0, 0), empty_mid=(500, 3), empty_last=(E - 1, R - 1), absent=(700, 2))
    for k in ("empty_first", "empty_mid", "empty_last"):
        rows[names[k]] = []
    assert names["absent"] not in rows
    return known_index(rows), names


def empty_row_indexes(md):
    """Small indexes that must be ACCEPTED, by name: empty rows at the front, in the middle and at the end; a descent of the tails
    across row boundaries only ([5, 9], an empty row, [3, 4]); one key; every row empty (nnz == 0, n_keys > 0)."""
    E, R = int(md["num_ent"]), int(md["num_rel"])
    return {
        "empty rows at the front, in the middle and at the end": known_index(
            {(0, 0): [], (0, 1): [], (2, 1): [4, 8], (2, 2): [], (2, 3): [], (3, 0): [0, 1, E - 1], (3, 1): [7], (E - 1, R - 2): [], (E - 1, R - 1): []}),
        "a descent across boundaries only": known_index({(1, 1): [5, 9], (1, 2): [], (1, 3): [3, 4]}),
        "one key": known_index({(7, 3): [1, 2, 6]}),
        "every row empty": known_index({(0, 0): [], (5, 1): [], (5, 2): [], (E - 1, R - 1): []}),
    }


def known_probe_queries(kf, md, seed):
    """(e1, rel) that look at an index from every side: each of its keys (shuffled, some twice), the pairs next to each key, both ends
    of the key range, and ids outside the model's range on either side."""
    E, R = int(md["num_ent"]), int(md["num_rel"])
    rng = np.random.default_rng(seed)
    key = kf["e1"] * R + kf["rel"]
    near = np.concatenate([key, key, key - 1, key + 1, [0, E * R - 1]])
    near = near[(near >= 0) & (near < E * R)]
    rng.shuffle(near)
    e1, rel = near // R, near % R
    out = np.array([[E, 0], [-1, 0], [0, R], [0, -1], [E, R], [int(kf["e1"][0]), R], [E, int(kf["rel"][0])]], np.int64)
    at = rng.integers(0, len(e1) + 1, len(out))
    return np.insert(e1, at, out[:, 0]), np.insert(rel, at, out[:, 1])
