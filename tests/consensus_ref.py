"""The numpy restatement of CalculateConsensus (pkg/engine/epistemic_types.go:126-178) and of the per-node similarity of
Engine.VBeliefState (pkg/engine/epistemic.go:81) that the consensus tests compare against (no test in here).

Order is what makes the sums reproducible, so the restatement keeps the reference's: the centroid is a float32 sum node after node
(vectorised over the columns, which are independent), every dot product and squared norm is a float64 sum over the columns in
ascending order (a loop over the columns, vectorised over the pairs, which are independent), the variance is a sum over the nodes in
list order.  float32 products widened to float64 are exact, so multiply-then-add here equals a fused multiply-add elsewhere."""
import numpy as np

REC = np.dtype([("score", "<f8"), ("variance", "<f8"), ("max_pair", "<f8"), ("n_found", "<u4"), ("n_active", "<u4")])


def cosine_distance(dot, na, nb):
    """CosineDistance (:299-320) from its three float64 sums; math.Max / math.Min keep a NaN"""
    with np.errstate(all="ignore"):
        sim = dot / (np.sqrt(na) * np.sqrt(nb))
        sim = np.where(sim > 1.0, 1.0, sim)
        sim = np.where(sim <= 0.0, 0.0, sim)
        d = 1.0 - sim
    return np.where((na == 0.0) | (nb == 0.0), 1.0, d)


def restate(V, found, active, Q=None):
    """V [B, S, dim] float32: the vector of every list entry (ignored where not found); found, active [B, S] bool; Q [B, dim] or None.
    -> dict(rec [B] REC, similarity [B, S] (-1.0: not found), centroid [B, dim] f32, gram [B, S + 1, S + 1] f64, index S the centroid,
    rows and columns of entries that are not active zero)"""
    V = np.ascontiguousarray(V, dtype=np.float32)
    B, S, dim = V.shape
    found = np.asarray(found, dtype=bool).reshape(B, S)
    act = found & np.asarray(active, dtype=bool).reshape(B, S)
    n = act.sum(axis=1)
    V = np.where(found[:, :, None], V, np.float32(0.0))
    cen = np.zeros((B, dim), dtype=np.float32)
    many = n > 1
    with np.errstate(all="ignore"):
        for i in range(S):                                       # node after node, float32
            m = many & act[:, i]
            cen[m] = cen[m] + V[m, i]
        cen[many] = cen[many] / n[many].astype(np.float32)[:, None]
    for b in np.nonzero(n == 1)[0]:
        cen[b] = V[b, int(np.argmax(act[b]))]                    # "return 1.0, 0.0, nodes[0].Vector"
    q = np.zeros((B, dim), dtype=np.float32) if Q is None else np.ascontiguousarray(Q, dtype=np.float32).reshape(B, dim)
    W = np.concatenate([V, cen[:, None, :], q[:, None, :]], axis=1).astype(np.float64)     # slots: S = centroid, S + 1 = query
    G = np.zeros((B, S + 2, S + 2), dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in range(dim):                                     # ascending columns into every accumulator
            x = W[:, :, c]
            G = G + x[:, :, None] * x[:, None, :]
    diag = np.einsum("bii->bi", G)
    sim = 1.0 - cosine_distance(G[:, :S, S + 1], diag[:, :S], diag[:, S + 1][:, None])
    sim = np.where(found, sim, -1.0)
    dc = cosine_distance(G[:, :S, S], diag[:, :S], diag[:, S][:, None])
    ssum = np.zeros(B, dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(S):                                       # in list order
            ssum = np.where(act[:, i], ssum + dc[:, i] * dc[:, i], ssum)
        var = np.where(many, ssum / np.maximum(n, 1).astype(np.float64), 0.0)
    D = cosine_distance(G[:, :S, :S], diag[:, :S, None], diag[:, None, :S])
    pair = act[:, :, None] & act[:, None, :] & np.triu(np.ones((S, S), dtype=bool), 1)[None]
    mv = np.where(pair & ~np.isnan(D), D, 0.0).reshape(B, -1).max(axis=1) if S else np.zeros(B)
    mv = np.where(many, mv, 0.0)                                 # `d > maxVar` from 0: a NaN never wins
    with np.errstate(all="ignore"):
        r = var / (mv * mv)
        r = np.where(r > 1.0, 1.0, r)                            # math.Min(r, 1): a NaN stays
        score = np.where(mv < 1e-10, 1.0, 1.0 - r)
    score = np.where(n == 0, 0.0, np.where(n == 1, 1.0, score))
    rec = np.zeros(B, dtype=REC)
    rec["score"], rec["variance"], rec["max_pair"] = score, var, mv
    rec["n_found"], rec["n_active"] = found.sum(axis=1), n
    okg = np.concatenate([act, np.ones((B, 1), dtype=bool)], axis=1)
    gram = np.where(okg[:, :, None] & okg[:, None, :], G[:, :S + 1, :S + 1], 0.0)
    return {"rec": rec, "similarity": sim, "centroid": cen, "gram": gram, "dist_centroid": np.where(act, dc, 0.0)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
