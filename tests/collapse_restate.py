"""The collapse of a ranked list to groups, restated in plain Python: the walk np_hip_collapse promises (include/nextplaid_hip.h),
which is ColGREP's collapse_by_file (colgrep/src/index/mod.rs:4394-4413) with a member limit.  No score is read: the order
of the list is the order.  Also an independent numpy formulation, the padded layout of the device's outputs, and a checker
that compares a device result with the walk field by field and bit by bit.  Pure host code."""
import numpy as np


def walk(ids, scores, group_ids, top_k, group_size, num_documents=None):
    """One ranked list -> the groups in order of admission: [(group_id, [ids], [score bits] or None, total)].  `ids` is the
    list as far as its count goes; an id outside [0, num_documents) is absent (the device form's rule; the host form refuses
    it before this point)."""
    n = len(group_ids) if num_documents is None else num_documents
    bits = None if scores is None else np.asarray(scores, np.float32).view(np.uint32).tolist()
    groups, where = [], {}
    for r, d in enumerate(np.asarray(ids, np.int64).tolist()):
        if d < 0 or d >= n:
            continue
        g = int(group_ids[d])
        if g in where:
            rec = groups[where[g]]
            rec[3] += 1
            if len(rec[1]) < group_size:
                rec[1].append(d)
                if bits is not None:
                    rec[2].append(bits[r])
        elif len(groups) < top_k:
            where[g] = len(groups)
            groups.append([g, [d], None if bits is None else [bits[r]], 1])
        # else: a new group after top_k groups is skipped
    return [(g, m, s, t) for g, m, s, t in groups]


def walk_numpy(ids, scores, group_ids, top_k, group_size):
    """The same result by another route: a stable argsort by group, the rank inside the group, and the order of the groups'
    first occurrences.  Every id must be in range."""
    ids = np.asarray(ids, np.int64)
    if ids.size == 0:
        return []
    bits = None if scores is None else np.asarray(scores, np.float32).view(np.uint32)
    g = np.asarray(group_ids)[ids].astype(np.int64)
    order = np.argsort(g, kind="stable")                       # groups together, list order inside
    gs = g[order]
    start = np.r_[True, gs[1:] != gs[:-1]]
    first_pos = np.nonzero(start)[0]
    run = np.cumsum(start) - 1                                 # which run a sorted entry belongs to
    member = np.arange(ids.size) - first_pos[run]              # its rank inside the group
    totals = np.diff(np.r_[first_pos, ids.size])
    leader_rank = order[first_pos]                             # list rank of every group's first occurrence
    admitted = np.argsort(leader_rank, kind="stable")[:top_k]  # runs in order of first occurrence
    out = []
    for rn in admitted.tolist():
        sel = order[(run == rn) & (member < group_size)]
        out.append((int(gs[first_pos[rn]]), ids[sel].tolist(), None if bits is None else bits[sel].tolist(), int(totals[rn])))
    return out


def padded(groups_per_query, top_k, group_size, with_scores=True):
    """What the device writes for a batch of walks: (ids [B][top_k][group_size] i64, score bits u32 likewise or None, group,
    members, total [B][top_k] i32, counts [B] i32), padded with zeros."""
    B = len(groups_per_query)
    ids = np.zeros((B, top_k, group_size), np.int64)
    sc = np.zeros((B, top_k, group_size), np.uint32) if with_scores else None
    grp, mem, tot = (np.zeros((B, top_k), np.int32) for _ in range(3))
    cnt = np.zeros(B, np.int32)
    for b, groups in enumerate(groups_per_query):
        cnt[b] = len(groups)
        for j, (g, m, s, t) in enumerate(groups):
            ids[b, j, : len(m)] = m
            if with_scores:
                sc[b, j, : len(m)] = s
            grp[b, j], mem[b, j], tot[b, j] = g, len(m), t
    return ids, sc, grp, mem, tot, cnt


def walk_batch(ids, scores, counts, stride, group_ids, top_k, group_size, num_documents=None):
    """The padded outputs for B lists in np_hip_collapse's layout (ids / scores [B * stride], counts clamped to the stride)."""
    counts = np.asarray(counts)
    B = counts.size
    ids = np.asarray(ids, np.int64).reshape(B, stride)
    sc = None if scores is None else np.asarray(scores, np.float32).reshape(B, stride)
    groups = []
    for b in range(B):
        c = min(max(int(counts[b]), 0), stride)
        groups.append(walk(ids[b, :c], None if sc is None else sc[b, :c], group_ids, top_k, group_size, num_documents))
    return padded(groups, top_k, group_size, sc is not None)


NAMES = ("ids", "scores", "group", "members", "total", "counts")


def check(got, want, what=""):
    """A device result (the six padded arrays; scores as f32 or u32, or None) equals the walk's, every field, padding
    included, score bits included."""
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None or name == "scores", f"{what}: {name} present without a reference"
            continue
        assert g is not None, f"{what}: {name} is missing"
        g = np.asarray(g)
        if name == "scores":
            g = g.view(np.uint32)
        g = g.reshape(w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0].tolist()
            raise AssertionError(f"{what}: {name} differs first at {bad}: got {g[tuple(bad)]}, want {w[tuple(bad)]}")


def listed(groups):
    """The public return value (group_id, passage_ids, scores, total) as comparable tuples of ints and score bits."""
    return [(int(g), np.asarray(m).tolist(), None if s is None else np.asarray(s, np.float32).view(np.uint32).tolist(), int(t))
            for g, m, s, t in groups]


def walked(groups):
    return [(g, list(m), None if s is None else list(s), t) for g, m, s, t in groups]
