"""resolveGraphFilter (pkg/engine/graph.go:173-246) in plain Python over graph node numbers: the FIFO queue, the visited set and the
depth rule as written there; out- and in-lists from (source, relation code, target) triples of ACTIVE edges; the engine's AND with
the metadata list (ops.go:950-957).  Node g <= count is internal id g; higher numbers are traversed and never allowed."""
from collections import deque

import numpy as np

OUT, IN, BOTH, NONE = 0, 1, 2, 3


def resolve(out, inn, count, root, max_depth, direction, rel_mask):
    """the set of allowed internal ids of one query"""
    if root == 0:  # the mirror does not know the id in the graph
        return set()
    allowed = {root} if root <= count else set()
    max_depth = 1 if max_depth <= 0 else 5 if max_depth > 5 else max_depth
    visited = {root}
    queue = deque([(root, 0)])
    while queue:
        node, depth = queue.popleft()
        if depth >= max_depth:
            continue
        for follows, lists in ((direction in (OUT, BOTH), out), (direction in (IN, BOTH), inn)):
            for r, t in lists.get(node, ()) if follows else ():
                if (rel_mask >> r) & 1 and t not in visited:
                    visited.add(t)
                    queue.append((t, depth + 1))  # enqueued whether or not the index holds it
                    if t <= count:
                        allowed.add(t)
    return allowed


def lists_of(edges, count, queries, words, and_lists=None, and_of_query=None):
    """(lists [B, words] uint64, card [B] uint32) of queries = (root, max_depth, direction, _, rel_mask) records"""
    out, inn = {}, {}
    for s, r, t in edges:
        out.setdefault(int(s), []).append((int(r), int(t)))
        inn.setdefault(int(t), []).append((int(r), int(s)))
    lists = np.zeros((len(queries), words), dtype=np.uint64)
    for b, q in enumerate(queries):
        for i in resolve(out, inn, count, int(q[0]), int(q[1]), int(q[2]), int(q[4])):
            lists[b, i >> 6] |= np.uint64(1 << (i & 63))
        if and_lists is not None and int(and_of_query[b]) & 0xFFFFFFFF != 0xFFFFFFFF:
            lists[b] &= and_lists[int(and_of_query[b])]
    card = np.array([sum(bin(int(w)).count("1") for w in row) for row in lists], dtype=np.uint32)
    return lists, card
