"""tests/textres_restate.py against itself and against np_hip_index_set_text's host loop restated: the round trip instances ->
layout -> instances is the identity on every shape the device tests install, each planted defect changes the result on at
least one of them, and the first offender is the one text_check_index names.  Needs no device."""
import numpy as np
import pytest

import textres_restate as X


def host_layout(toff, doc, n_docs):
    """set_text_impl's serial loop (np_text.hip), the oracle of the layout."""
    post_off, post_doc, post_tf, post_first = [0], [], [], []
    doc_len = np.zeros(n_docs, np.int32)
    for k in range(toff.size - 1):
        first = True
        for i in range(int(toff[k]), int(toff[k + 1])):
            d = int(doc[i])
            if first or post_doc[-1] != d:
                post_doc.append(d)
                post_tf.append(0)
                post_first.append(i)
                first = False
            post_tf[-1] += 1
            doc_len[d] += 1
        post_off.append(len(post_doc))
    return (np.asarray(post_off, np.int64), np.asarray(post_doc, np.int32).reshape(-1), np.asarray(post_tf, np.int32).reshape(-1),
            np.asarray(post_first, np.int64).reshape(-1), doc_len)


SHAPES = X.shapes()


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_layout_is_the_host_loops_and_the_round_trip_is_the_identity(name):
    toff, doc, pos, n_docs = SHAPES[name]
    lay = X.layout(toff, doc, n_docs)
    assert same(lay, host_layout(toff, doc, n_docs))
    post_off, post_doc, post_tf, post_first, doc_len = lay
    assert int(post_tf.sum()) == doc.size == int(doc_len.sum())
    back_toff, back_doc = X.instances(post_off, post_doc, post_first, doc.size)
    assert np.array_equal(back_toff, toff) and np.array_equal(back_doc, doc)
    assert X.first_offender(toff, doc, pos, n_docs) is None


@pytest.mark.parametrize("defect", X.LAYOUT_DEFECTS)   # (the check's and the counts': tests/test_textres_limits_cpu.py)
def test_every_planted_defect_shows_on_a_listed_shape(defect):
    hit = []
    for name, (toff, doc, pos, n_docs) in SHAPES.items():
        good = X.layout(toff, doc, n_docs)
        if defect == "bisection_off_by_one":
            got = X.instances(good[0], good[1], good[3], doc.size, defect=defect)
            if not (np.array_equal(got[0], toff) and np.array_equal(got[1], doc)):
                hit.append(name)
        elif not same(X.layout(toff, doc, n_docs, defect=defect), good):
            hit.append(name)
    assert hit, defect
    if defect == "head_on_document_change_only":
        assert "terms_meet_in_one_document" in hit      # the case that must bite: two postings fuse


def test_the_first_offender_is_the_lowest_and_names_its_rule():
    toff, doc, pos, n_docs = X.table([[(0, 0), (1, 0)], [(1, 1), (2, 0), (2, 1)]] , 3)
    assert X.first_offender(toff, doc, pos, n_docs) is None
    assert X.first_offender(toff, doc, pos, 2) == (3, 1)                      # documents >= n_docs: the lowest instance
    p = pos.copy(); p[4] = -1
    assert X.first_offender(toff, doc, p, n_docs) == (4, 2)
    d = doc.copy(); d[1] = 0                                                  # (0, 0) twice in term 0
    assert X.first_offender(toff, d, pos, n_docs) == (1, 3)
    d = doc.copy(); d[2] = 0                                                  # a term's FIRST instance has no predecessor
    assert X.first_offender(toff, d, pos, n_docs) is None
    d = doc.copy(); d[0] = 5; p = pos.copy(); p[0] = -1                       # two rules on one instance: the document's first
    assert X.first_offender(toff, d, p, n_docs) == (0, 1)
    big = X.table([[(0, q) for q in range(3 * X.CHUNK)]])
    for at in (X.CHUNK - 1, X.CHUNK, X.CHUNK + 1):
        p = big[2].copy(); p[at] = p[at - 1]
        p2 = p.copy(); p2[2 * X.CHUNK + 7] = -3                               # a later block offends too
        assert X.first_offender(big[0], big[1], p2, 1) == (at, 3)


# ---- np_textres_plan.h, stand-alone ------------------------------------------------------------------------------------------
def test_plan_header_against_hand_written_answers(tmp_path):
    """tests/cpp/textres_plan_check.cpp built with the host compiler alone, plain and under ASan + UBSan, each a program of
    its own; both must print the same."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "textres_plan_check.cpp")
    outs = []
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"textres_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, src, "-o", str(exe)])
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout.splitlines())
    assert outs[0] == outs[1] and outs[0][-1] == "all checks passed", outs[0][-5:]
