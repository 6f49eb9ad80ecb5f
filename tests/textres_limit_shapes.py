"""The cases of tests/test_gpu_textres_limits.py -- the resident keyword index's check, its counts over the handle's documents
and its read-back at the edges of their own kernels (np_textres.hip) -- each with a census of the edges it reaches, stated on
tests/textres_restate.py and on SQLite's index of the rows alone.  tests/test_textres_limits_cpu.py asserts every census entry
and that each planted defect of the restatement is rejected by a named case; the device test installs the same rows.

CHUNK = 2048 instances (or documents) per block of the check and of a scan launch, eight per thread."""
import numpy as np

from next_plaid_amd.text import TextIndexData

import textres_restate as X

CHUNK = X.CHUNK
blocks = X.blocks

N_CHECK = 2040                               # the handle of the C cases
N_UPLOADED = N_CHECK + 2100                  # ... and the one that holds all their rows
N_FAR = (2047, 2048, 2049, 4097)             # the handles of N1
N_COUNT = 4097                               # the handle of N2, N3: three blocks of documents
BATCH = ["q", "", "q q", ""]                 # two rows that hold a token (one of them twice), two that hold none


# ---- C: the check --------------------------------------------------------------------------------------------------------------
C1_LEADS = (7, 8, 9, 15, 16)


def offender_rows(s):
    """C1: "m" in every one of N_UPLOADED rows and s times "a" in front of row 0: term "a" holds the instances 0 .. s - 1 and row
    d's "m" is instance s + d.  On a handle of N_CHECK documents the rows from N_CHECK on offend: instance s + N_CHECK first."""
    rows = ["m"] * N_UPLOADED
    rows[0] = "a " * s + "m"
    return rows


def first_of_term_rows():
    """C2: "z" occurs in row N_CHECK alone, behind 8 instances of "a" and N_CHECK of "m": its one instance is instance CHUNK, the
    first of block 1, of its thread and of its term -- no predecessor is read, on the device or by the host that names it."""
    rows = ["m"] * N_CHECK + ["z"]
    rows[0] = "a " * 8 + "m"
    return rows


UPLOADED_FALLBACK = [5, 100]


def uploaded_rows():
    """C3: C1 at s = 8 with two rows that are not ASCII, which the device hands back: the build is merged on the host and the
    install uploads it.  Their extra terms sort behind "m", so the offender stays where C1 has it."""
    rows = offender_rows(8)
    rows[5], rows[100] = "m né", "zoë m"
    return rows


def check_census(rows, n_docs):
    """What the check meets on SQLite's index of `rows` over a handle of n_docs documents."""
    want = TextIndexData.from_texts(rows)
    low, rule = X.first_offender(want.term_offsets, want.inst_doc, want.inst_pos, n_docs)
    per_block = X.block_offenders(want.term_offsets, want.inst_doc, want.inst_pos, n_docs)
    return dict(want=want, low=low, rule=rule, doc=int(want.inst_doc[low]), block=low // CHUNK, thread=low % CHUNK // X.THREAD,
                slot=low % X.THREAD, first_of_term=low in set(want.term_offsets.tolist()), per_block=per_block,
                offending_blocks=np.nonzero(per_block != X.NO_OFFENDER)[0].tolist())


# ---- N: counts over the documents ---------------------------------------------------------------------------------------------
def holder_rows(n_docs, holders, word="w"):
    rows = [""] * n_docs
    for d in holders:
        rows[d] = word
    return rows


def far_holders(n_docs):
    return sorted({d for d in (0, 2046, 2047, 2048, n_docs - 1) if d < n_docs})


def far_rows(n_docs):
    """N1: n_docs rows without a token but for rows 0, 2046, 2047, 2048 (where present) and the last."""
    return holder_rows(n_docs, far_holders(n_docs))


def doc_len_of(rows, n_docs):
    want = TextIndexData.from_texts(rows)
    return X.layout(want.term_offsets, want.inst_doc, n_docs)[4]


def batch_docs(batch):
    """inst_doc of the batch's own build: its rows numbered from 0."""
    return np.zeros(0, np.int64) if not batch else TextIndexData.from_texts(list(batch)).inst_doc


def merge_call(n_docs, holders, remap, batch, n_rows_out=None):
    """One raw np_hip_index_text_merge on the base holder_rows(n_docs, holders): its arguments, and what the restatement says of
    the two counts."""
    remap = np.asarray(remap, np.int64)
    doc_len = doc_len_of(holder_rows(n_docs, holders), n_docs)
    delta = batch_docs(batch)
    n_delta = 0 if batch is None else len(batch)
    distinct = X.distinct_result(doc_len, remap, remap.size, delta, n_delta)
    return dict(n_docs=n_docs, holders=list(holders), remap=remap, batch=batch, doc_len=doc_len, delta_inst_doc=delta, n_delta_docs=n_delta,
                delta_ids=n_docs + np.arange(n_delta, dtype=np.int64), distinct=distinct, beyond=X.beyond(doc_len, remap.size),
                n_told=min(remap.size, n_docs), n_survivors=int(np.count_nonzero(remap >= 0)),
                n_rows_out=distinct if n_rows_out is None else n_rows_out)


def survivor_calls():
    """N2: name -> call.  remap is the identity with one -1: at a document that holds a token on either side of the chunk edge,
    or at one that holds none (which must not change the count)."""
    holders = far_holders(N_COUNT)

    def call(gone, batch):
        remap = np.arange(N_COUNT, dtype=np.int64)
        remap[gone] = -1
        return merge_call(N_COUNT, holders, remap, batch)
    return {"holder 2047 goes": call(2047, BATCH), "holder 2048 goes": call(2048, BATCH), "empty 2049 goes": call(2049, BATCH),
            "no batch": call(2047, None), "a batch of empty rows": call(2048, ["", "", ""])}


N_REMAPS = (N_COUNT, N_COUNT - 1, 2049, 2047, 1, 0)


def behind_calls():
    """N3: n_remap -> (the accepted call, [refused calls]).  The accepted base holds tokens inside [0, n_remap) only -- at its
    first and last document and around document 2047 --; a refused one also at the first document behind n_remap ("one"), or at
    that one, on either side of the first chunk edge counted from n_remap, and at the last document ("many")."""
    out = {}
    for n_remap in N_REMAPS:
        inside = sorted({d for d in (0, 2046, 2047, 2048, n_remap - 1) if 0 <= d < n_remap})
        ident = np.arange(n_remap, dtype=np.int64)
        accepted = merge_call(N_COUNT, inside, ident, BATCH)
        refused = []
        one = [n_remap] if n_remap < N_COUNT else []
        many = sorted({d for d in (n_remap, n_remap + CHUNK - 1, n_remap + CHUNK, N_COUNT - 1) if d < N_COUNT})
        for behind in ([one] if one else []) + ([many] if len(many) > 1 else []):
            refused.append(merge_call(N_COUNT, inside + behind, ident, None, n_rows_out=n_remap))
        out[n_remap] = (accepted, refused)
    return out


# ---- W: the read-back ---------------------------------------------------------------------------------------------------------
def host_data(shape, n_rows):
    """A table of tests/textres_restate.py's shapes() as the TextIndexData that set_text takes; its terms are t000, t001, ..."""
    toff, doc, pos, _ = X.shapes()[shape]
    terms = [f"t{i:03d}" for i in range(toff.size - 1)]
    return TextIndexData("unicode61", terms, toff, doc, pos.astype(np.int32), n_rows, {t: i for i, t in enumerate(terms)})


# ---- P: four states of equal sizes ---------------------------------------------------------------------------------------------
STATE_DOCS = 40
STATE_SWAPS = ((0, 7), (3, 12), (5, 19))


def states():
    """Four lists of 20 rows; each is the one before with the texts of two rows swapped, which keeps the vocabulary and every
    size of the index.  Returns (the lists, the replace= of the three updates)."""
    rows = [f"w{i % 5} v{i % 7} tail" + " w1" * (i % 3) for i in range(20)]
    out, steps = [list(rows)], []
    for i, j in STATE_SWAPS:
        steps.append({i: rows[j], j: rows[i]})
        rows[i], rows[j] = rows[j], rows[i]
        out.append(list(rows))
    return out, steps


def state_keys(rows, n_docs=STATE_DOCS):
    """(the five layout arrays' bytes, the three table arrays' bytes) of one state."""
    want = TextIndexData.from_texts(rows)
    lay = X.layout(want.term_offsets, want.inst_doc, n_docs)
    return tuple(a.tobytes() for a in lay), (want.term_offsets.tobytes(), want.inst_doc.tobytes(), want.inst_pos.tobytes())
