"""The keyword-index merge (np_hip_text_build_merge) restated in numpy: from a base index A, a verdict per old document
(remap: -1 = removed, otherwise its new id) and the index B of a batch of new texts, the index of the resulting table --
every instance computes its own destination, as the device does.  tests/test_textmerge_restate_cpu.py pins it to a live
SQLite FTS5 table that went through the same operations.

The arrays are textbuild_restate.arrays(): terms (byte strings in memcmp order, the shorter first = Python's bytes order),
term_offsets, inst_doc, inst_pos, n_rows.

The rule:
  host    the union of the two sorted vocabularies numbers every term of A and of B; bound[j] = the smallest OLD id whose
          survivor id is >= delta_ids[j] (n_old if none): old ids ascend inside a run of A and so do the survivors' new ids,
          so "A instances before batch document j" is a lower bound over OLD ids, holes or not
  keep    keep[i] = remap[doc_A[i]] >= 0;  S = exclusive scan of keep
  terms   cnt[u] = kept instances of its A term + instances of its B term; off = exclusive scan of cnt; a term is alive
          while cnt[u] > 0 and the alive terms are numbered by a scan
  A       kept instance i of term a:  off[u] + (S[i] - S[toff_A[a]]) + #{B instances of the term with new id < its own}
  B       instance k of term b:       off[u] + (k - toff_B[b]) + (S[lb] - S[toff_A[a]]), lb = the first A instance of the
          term whose OLD id is >= bound[doc_B[k]]

`defect` plants one wrong step."""
import numpy as np

DEFECTS = ("le_in_b_bound", "dead_terms_kept", "remap_not_applied", "inclusive_s", "bound_from_new_ids")
# "<=" for "<" in the A side's lower bound changes nothing on valid input: delta_ids never equals a survivor's id
UNOBSERVABLE = ("le_in_a_bound",)


def union_terms(terms_a, terms_b):
    """(the united vocabulary, union id per A term, union id per B term, A term per union id or -1, B term likewise)."""
    ua, ub, terms, a_of, b_of = [], [], [], [], []
    i = j = 0
    while i < len(terms_a) or j < len(terms_b):
        if j >= len(terms_b) or (i < len(terms_a) and terms_a[i] < terms_b[j]):
            c = -1
        elif i >= len(terms_a) or terms_b[j] < terms_a[i]:
            c = 1
        else:
            c = 0
        u = len(terms)
        terms.append(terms_a[i] if c <= 0 else terms_b[j])
        a_of.append(i if c <= 0 else -1)
        b_of.append(j if c >= 0 else -1)
        if c <= 0:
            ua.append(u)
            i += 1
        if c >= 0:
            ub.append(u)
            j += 1
    return terms, ua, ub, a_of, b_of


def bounds(remap, delta_ids, defect=None):
    remap = np.asarray(remap, np.int64)
    delta_ids = np.asarray(delta_ids, np.int64)
    if defect == "bound_from_new_ids":
        return np.minimum(delta_ids, remap.size)
    surv = np.flatnonzero(remap >= 0)
    at = np.searchsorted(remap[surv], delta_ids, "left")
    return np.where(at < surv.size, np.append(surv, remap.size)[at], remap.size).astype(np.int64)


def merge(a, remap, b, delta_ids, n_rows_out, defect=None):
    remap = np.asarray(remap, np.int64).reshape(-1)
    delta_ids = np.asarray(delta_ids, np.int64).reshape(-1)
    toff_a, doc_a, pos_a = a["term_offsets"], a["inst_doc"], a["inst_pos"]
    toff_b, doc_b, pos_b = b["term_offsets"], b["inst_doc"], b["inst_pos"]
    terms, ua, ub, a_of, b_of = union_terms(list(a["terms"]), list(b["terms"]))
    bound = bounds(remap, delta_ids, defect)
    na = int(doc_a.size)
    keep = (remap[doc_a] >= 0).astype(np.int64) if na else np.zeros(0, np.int64)
    S = np.concatenate([[0], np.cumsum(keep)])
    if defect == "inclusive_s":
        S = np.concatenate([np.cumsum(keep), [int(keep.sum())]])
    new_b = delta_ids[doc_b] if doc_b.size else np.zeros(0, np.int64)
    U = len(terms)
    cnt = np.zeros(U, np.int64)
    for u in range(U):
        if a_of[u] >= 0:
            cnt[u] += S[toff_a[a_of[u] + 1]] - S[toff_a[a_of[u]]]
        if b_of[u] >= 0:
            cnt[u] += toff_b[b_of[u] + 1] - toff_b[b_of[u]]
    off = np.concatenate([[0], np.cumsum(cnt)])
    alive = np.ones(U, bool) if defect == "dead_terms_kept" else cnt > 0
    total = int(off[-1])
    out_doc, out_pos = np.full(total, -7, np.int64), np.full(total, -7, np.int32)
    for t in range(len(a["terms"])):
        u, lo = ua[t], int(toff_a[t])
        bl, bh = (int(toff_b[b_of[u]]), int(toff_b[b_of[u] + 1])) if b_of[u] >= 0 else (0, 0)
        for i in range(lo, int(toff_a[t + 1])):
            if not keep[i]:
                continue
            nid = int(remap[doc_a[i]])
            before = int(np.searchsorted(new_b[bl:bh], nid, "right" if defect == "le_in_a_bound" else "left"))
            dst = int(off[u] + (S[i] - S[lo]) + before)
            if 0 <= dst < total:       # a planted defect may point outside; the rule itself never does
                out_doc[dst] = int(doc_a[i]) if defect == "remap_not_applied" else nid
                out_pos[dst] = pos_a[i]
    for t in range(len(b["terms"])):
        u, lo = ub[t], int(toff_b[t])
        al, ah = (int(toff_a[a_of[u]]), int(toff_a[a_of[u] + 1])) if a_of[u] >= 0 else (0, 0)
        for k in range(lo, int(toff_b[t + 1])):
            lb = al + int(np.searchsorted(doc_a[al:ah], bound[doc_b[k]], "right" if defect == "le_in_b_bound" else "left"))
            dst = int(off[u] + (k - lo) + (S[lb] - S[al]))
            if 0 <= dst < total:
                out_doc[dst] = new_b[k]
                out_pos[dst] = pos_b[k]
    return dict(terms=[terms[u] for u in range(U) if alive[u]],
                term_offsets=np.asarray([off[u] for u in range(U) if alive[u]] + [total], np.int64),
                inst_doc=out_doc, inst_pos=out_pos, n_rows=int(n_rows_out))


def plan_update(n_old, delete=(), replace_ids=(), n_new=0, renumber=True):
    """remap, delta_ids and the result's row count of TextIndexData.updated: the batch is the replacements in id order, then
    the new texts.  renumber: the survivors (replaced ones included) are numbered densely in order, as delete + rebuild
    leave them; otherwise every id stays.  New texts follow the last id."""
    gone = set(int(d) for d in delete)
    rep = sorted(int(r) for r in replace_ids)
    remap = np.full(n_old, -1, np.int64)
    new_id = {}
    nxt = 0
    for d in range(n_old):
        if d in gone:
            continue
        new_id[d] = nxt if renumber else d
        nxt += 1
    for d, v in new_id.items():
        if d not in rep:
            remap[d] = v
    top = nxt if renumber else n_old
    delta_ids = np.asarray([new_id[r] for r in rep] + [top + i for i in range(n_new)], np.int64)
    return remap, delta_ids, (nxt if renumber else n_old - len(gone)) + n_new
