"""The resident keyword index (np_textres.hip) restated in numpy: heads, postings and doc_len of an instance table as
np_hip_index_set_text_build derives them, the device check's first offender, and the way back from the postings to the
instances as np_hip_index_text_merge and np_hip_index_get_text take it.  `defect` plants one of DEFECTS; the shape generators
are the ones the device tests install.

For tests/test_textres_limits_cpu.py and tests/test_gpu_textres_limits.py also: the check's reduction as tr_check_heads and the
host form it (block_offenders: CHUNK instances per block, eight per thread, a thread's first offender, the block's lowest;
reduced_offender: the minimum over the blocks, named as name_offender names it from two fetched instances), and the two counts
over the handle's documents that np_hip_index_text_merge takes (count_docs, beyond, distinct_result)."""
import numpy as np

CHUNK = 2048           # NP_TB_SCAN_CHUNK: instances per block of the check / heads launch and of a scan launch
SCAN_ROUND = 256       # block sums that tb_scan_sums takes per round

LAYOUT_DEFECTS = ("head_on_document_change_only", "tf_off_by_one_at_term_end", "post_off_of_empty_term", "doc_len_per_posting",
                  "bisection_off_by_one")                      # of layout() and instances()
CHECK_DEFECTS = ("min_over_the_first_block_only", "thread_keeps_its_last_offender", "block_start_has_no_predecessor")
COUNT_DEFECTS = ("count_ignores_remap", "count_ignores_doc_len", "beyond_counts_from_zero", "beyond_skips_its_first_document",
                 "batch_documents_counted_per_instance", "batch_empty_rows_counted")
DEFECTS = LAYOUT_DEFECTS + CHECK_DEFECTS + COUNT_DEFECTS
THREAD = 8            # instances per thread of the check / heads launch
NO_OFFENDER = np.iinfo(np.int64).max


def layout(term_offsets, inst_doc, n_docs, defect=None):
    """(post_off, post_doc, post_tf, post_first, doc_len) of an instance table over a handle of n_docs documents."""
    toff = np.asarray(term_offsets, np.int64)
    doc = np.asarray(inst_doc, np.int64)
    n, T = doc.size, toff.size - 1
    head = np.zeros(n, bool)
    if n:
        head[1:] = doc[1:] != doc[:-1]
        head[0] = True
        if defect != "head_on_document_change_only":
            starts = toff[:-1][toff[:-1] < toff[1:]]          # the terms that hold an instance
            head[starts] = True
    rank = np.concatenate([[0], np.cumsum(head)]).astype(np.int64)     # exclusive scan, rank[n] = n_post
    post_first = np.nonzero(head)[0].astype(np.int64)
    post_doc = doc[post_first].astype(np.int32)
    nxt = np.concatenate([post_first[1:], [n]]).astype(np.int64)
    post_tf = (nxt - post_first).astype(np.int32)
    if defect == "tf_off_by_one_at_term_end" and post_first.size:
        ends = np.isin(nxt, toff[1:])                                  # postings that end where a term ends
        post_tf = post_tf - ends.astype(np.int32)
    post_off = rank[np.minimum(toff, n)]
    if defect == "post_off_of_empty_term":
        empty = np.nonzero(toff[:-1] == toff[1:])[0]
        post_off = post_off.copy()
        post_off[empty] = np.maximum(post_off[empty] - 1, 0)
    doc_len = np.zeros(max(int(n_docs), 0), np.int64)
    if defect == "doc_len_per_posting":
        np.add.at(doc_len, post_doc, 1)
    else:
        np.add.at(doc_len, post_doc, post_tf)
    return post_off.astype(np.int64), post_doc, post_tf, post_first, doc_len.astype(np.int32)


def instances(post_off, post_doc, post_first, n_inst, defect=None):
    """(term_offsets, inst_doc) regenerated from the postings."""
    post_off, post_first = np.asarray(post_off, np.int64), np.asarray(post_first, np.int64)
    n_post = post_first.size
    toff = np.where(post_off < n_post, post_first[np.minimum(post_off, max(n_post - 1, 0))] if n_post else 0, n_inst).astype(np.int64)
    i = np.arange(n_inst, dtype=np.int64)
    at = np.searchsorted(post_first, i, side="left" if defect == "bisection_off_by_one" else "right") - 1
    inst_doc = np.asarray(post_doc, np.int64)[np.maximum(at, 0)] if n_inst else np.zeros(0, np.int64)
    return toff, inst_doc.astype(np.int64)


def _rules(term_offsets, inst_doc, inst_pos, n_docs, block_starts_are_first=False):
    """Per instance the rule it fails (0 = none), and whether it is the first of its term."""
    toff = np.asarray(term_offsets, np.int64)
    doc, pos = np.asarray(inst_doc, np.int64), np.asarray(inst_pos, np.int64)
    n = doc.size
    first = np.zeros(n, bool)
    if n == 0:
        return np.zeros(0, np.int64), first
    first[toff[:-1][toff[:-1] < toff[1:]]] = True
    first[0] = True
    if block_starts_are_first:
        first[::CHUNK] = True
    pd, pp = np.concatenate([[0], doc[:-1]]), np.concatenate([[0], pos[:-1]])
    r1 = (doc < 0) | (doc >= n_docs)
    r2 = pos < 0
    r3 = ~first & ((pd > doc) | ((pd == doc) & (pp >= pos)))
    return np.where(r1, 1, np.where(r2, 2, np.where(r3, 3, 0))).astype(np.int64), first


def first_offender(term_offsets, inst_doc, inst_pos, n_docs):
    """(instance, rule) of the lowest instance that fails np_hip_index_set_text's checks, or None.  Rules: 1 = document
    outside [0, n_docs), 2 = negative position, 3 = not after its predecessor in (document, position) order."""
    rule, _ = _rules(term_offsets, inst_doc, inst_pos, n_docs)
    bad = np.nonzero(rule)[0]
    return None if bad.size == 0 else (int(bad[0]), int(rule[bad[0]]))


def blocks(n, per=CHUNK):
    return -(-int(n) // per)


def block_offenders(term_offsets, inst_doc, inst_pos, n_docs, defect=None):
    """bad[block] as tr_check_heads leaves it: every thread keeps the first offender of its THREAD instances, the block takes
    the lowest of its threads; NO_OFFENDER where a block is clean.  int64 [blocks(n_inst)]."""
    rule, _ = _rules(term_offsets, inst_doc, inst_pos, n_docs, defect == "block_start_has_no_predecessor")
    n = rule.size
    nb = blocks(n)
    padded = np.zeros(nb * CHUNK, np.int64)
    padded[:n] = rule
    bad = padded.reshape(nb, CHUNK // THREAD, THREAD) != 0
    at = np.arange(nb * CHUNK, dtype=np.int64).reshape(bad.shape)
    if defect == "thread_keeps_its_last_offender":
        per_thread = np.where(bad, at, -1).max(axis=2)
        per_thread = np.where(per_thread < 0, NO_OFFENDER, per_thread)
    else:
        per_thread = np.where(bad, at, NO_OFFENDER).min(axis=2)
    return per_thread.min(axis=1).astype(np.int64) if nb else np.zeros(0, np.int64)


def reduced_offender(term_offsets, inst_doc, inst_pos, n_docs, defect=None):
    """(instance, rule) as install_impl and name_offender give it: the minimum of block_offenders, its term from the term
    starts, its rule recomputed from the instance and -- unless it starts its term -- its predecessor.  None = accepted."""
    per_block = block_offenders(term_offsets, inst_doc, inst_pos, n_docs, defect)
    if defect == "min_over_the_first_block_only":
        per_block = per_block[:1]
    low = int(per_block.min()) if per_block.size else NO_OFFENDER
    if low == NO_OFFENDER:
        return None
    toff = np.asarray(term_offsets, np.int64)
    doc, pos = np.asarray(inst_doc, np.int64), np.asarray(inst_pos, np.int64)
    term = int(np.searchsorted(toff, low, side="right")) - 1
    first = (term >= 0 and int(toff[term]) == low) or low == 0
    d, p = int(doc[low]), int(pos[low])
    pd, pp = (0, 0) if first else (int(doc[low - 1]), int(pos[low - 1]))
    if d < 0 or d >= n_docs:
        return low, 1
    if p < 0:
        return low, 2
    return (low, 3) if not first and (pd > d or (pd == d and pp >= p)) else (low, 0)


# ---- the counts over the handle's documents (np_hip_index_text_merge) ----------------------------------------------------------
def count_docs(doc_len, remap=None, defect=None):
    """The number of d with doc_len[d] > 0 and, where remap is given, remap[d] >= 0 (tr_doc_flags and the scan's total)."""
    doc_len = np.asarray(doc_len, np.int64)
    flag = np.ones(doc_len.size, bool) if defect == "count_ignores_doc_len" else doc_len > 0
    if remap is not None and defect != "count_ignores_remap":
        flag = flag & (np.asarray(remap, np.int64)[: doc_len.size] >= 0)
    return int(np.count_nonzero(flag))


def beyond(doc_len, n_remap, defect=None):
    """The documents of the handle at or behind n_remap that hold a token: the merge refuses any."""
    doc_len = np.asarray(doc_len, np.int64)
    told = min(int(n_remap), doc_len.size)
    if defect == "beyond_counts_from_zero":
        told = 0
    if defect == "beyond_skips_its_first_document":
        told += 1
    return count_docs(doc_len[told:])


def distinct_result(doc_len, remap, n_remap, delta_inst_doc, n_delta_docs=None, defect=None):
    """The documents of the merge's result that hold a token: the survivors among the handle's first n_remap documents that
    hold one, plus the distinct documents of the batch that do (a batch row without a token is no instance's document)."""
    doc_len = np.asarray(doc_len, np.int64)
    told = min(int(n_remap), doc_len.size)
    survivors = count_docs(doc_len[:told], np.asarray(remap, np.int64)[:told], defect)
    b = np.asarray(delta_inst_doc, np.int64).reshape(-1)
    if defect == "batch_documents_counted_per_instance":
        batch = int(b.size)
    elif defect == "batch_empty_rows_counted":
        batch = int(n_delta_docs)
    else:
        batch = int(np.unique(b).size)
    return survivors + batch


# ---- shapes: (term_offsets, inst_doc, inst_pos, n_docs), every one a well-formed table ----------------------------------------
def table(rows, n_docs=None):
    """rows: per term a list of (document, position), ascending.  Terms may be empty."""
    toff = np.zeros(len(rows) + 1, np.int64)
    toff[1:] = np.cumsum([len(r) for r in rows])
    doc = np.asarray([d for r in rows for d, _ in r], np.int64).reshape(-1)
    pos = np.asarray([p for r in rows for _, p in r], np.int32).reshape(-1)
    if n_docs is None:
        n_docs = int(doc.max()) + 1 if doc.size else 0
    return toff, doc, pos, int(n_docs)


def shapes():
    """name -> table.  The ones a build can make, and (marked *_host) the ones only np_hip_index_set_text takes: empty terms."""
    s = {}
    s["no_instances"] = table([], 3)
    s["one_instance"] = table([[(0, 0)]])
    s["every_instance_its_own_posting"] = table([[(d, 0) for d in range(5)], [(d, 1) for d in range(1, 5)]])
    s["one_posting_across_a_chunk"] = table([[(0, p) for p in range(CHUNK + 5)]])
    # heads at instances 2047, 2048 and 2049: one long posting of 2047 positions, then three documents
    s["heads_at_the_chunk_edge"] = table([[(0, p) for p in range(CHUNK - 1)] + [(1, 0), (2, 0), (3, 0), (3, 1)]])
    # neighbouring terms that end and begin with the same document: only the term start keeps the postings apart
    s["terms_meet_in_one_document"] = table([[(0, 0), (2, 0)], [(2, 1), (2, 4)], [(2, 2)], [(1, 0), (2, 3)]])
    s["documents_without_tokens"] = table([[(2, 0), (4, 0)], [(2, 1), (5, 0), (5, 1)]], 9)
    s["tf_above_one"] = table([[(0, 0), (0, 3), (1, 1)], [(0, 1), (0, 2), (1, 0), (1, 2), (1, 3)]])
    s["empty_terms_host"] = table([[(0, 0)], [], [], [(0, 1), (1, 0)], [], [(1, 1)], [], []])
    s["only_empty_terms_host"] = table([[], []], 2)
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(40):
        docs = np.sort(rng.choice(60, int(rng.integers(1, 30)), replace=False))
        rows.append([(int(d), int(p)) for d in docs for p in np.sort(rng.choice(50, int(rng.integers(1, 4)), replace=False))])
    s["random"] = table(rows, 64)
    return s
