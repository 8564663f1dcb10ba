"""fp64 restatement of unimm_seq_pref's contract (include/unimm_hip.h), in per-group loops and plain Python floats (IEEE
doubles): sums are serial chains in index order, as the kernel forms them, so only exp and log can differ from the device.

    seq_pref(rownll, ref_rownll | None, row_seq, n_rows, seq_group, seq_weight, groups, beta, length_normalize)
        -> dict(adv [len(rownll)], seq_score [B], seq_prob [B], group_loss [groups], alive_inv, alive [groups] bool,
                written_rows: the rows whose adv the kernel writes)
Every output is float64; the caller rounds to fp32 for the comparison.  n_rows: min(n, *n_dev)."""
import math

import numpy as np

MAX_MEMBERS = 128


def seq_pref(rownll, ref_rownll, row_seq, n_rows, seq_group, seq_weight, groups, beta, length_normalize):
    rownll = np.asarray(rownll, dtype=np.float64)
    ref = None if ref_rownll is None else np.asarray(ref_rownll, dtype=np.float64)
    row_seq = np.asarray(row_seq, dtype=np.int64)
    seq_group = np.asarray(seq_group, dtype=np.int64)
    w32 = np.asarray(seq_weight, dtype=np.float32)
    B = seq_group.shape[0]
    beta = float(np.float32(beta))
    n_rows = max(int(n_rows), 0)
    out = dict(adv=np.zeros(rownll.shape[0]), seq_score=np.full(B, np.nan), seq_prob=np.zeros(B), group_loss=np.zeros(groups),
               alive_inv=float("nan"), alive=np.zeros(groups, dtype=bool), written_rows=n_rows)
    if n_rows == 0:
        return out
    # ---- per sequence: rows in ascending index -----------------------------------------------------------------------
    S, R, Ln = [0.0] * B, [0.0] * B, [0] * B
    for r in range(n_rows):
        j = int(row_seq[r])
        if 0 <= j < B:
            S[j] -= float(rownll[r])
            if ref is not None:
                R[j] -= float(ref[r])
            Ln[j] += 1
    D = [float("nan")] * B
    for j in range(B):
        if Ln[j] > 0:
            D[j] = (S[j] - R[j]) / (float(Ln[j]) if length_normalize else 1.0)
            out["seq_score"][j] = D[j]
    # ---- per group: members in ascending sequence index ----------------------------------------------------------------
    c = [0.0] * B
    for g in range(groups):
        mem = [j for j in range(B) if seq_group[j] == g and Ln[j] > 0]
        if not mem:
            continue
        w = [float(w32[j]) for j in mem]
        if len(mem) > MAX_MEMBERS or any(not (x >= 0.0 and x < math.inf) for x in w):
            out["group_loss"][g] = np.nan
            out["seq_prob"][mem] = np.nan
            continue
        z = [beta * D[j] for j in mem]
        m = -math.inf
        for x in z:
            m = max(m, x)
        s = 0.0
        for x in z:
            s += math.exp(x - m)
        lse = m + math.log(s)
        W = 0.0
        for x in w:
            W += x
        alive = W > 0.0
        loss = 0.0
        for k, j in enumerate(mem):
            logP = z[k] - lse
            P = math.exp(logP)
            loss += w[k] * logP
            out["seq_prob"][j] = P
            if alive:
                c[j] = beta * (w[k] - W * P) / (float(Ln[j]) if length_normalize else 1.0)
        out["group_loss"][g] = -loss if alive else 0.0
        out["alive"][g] = alive
    n_alive = int(out["alive"].sum())
    out["alive_inv"] = 1.0 / n_alive if n_alive else float("nan")
    for r in range(n_rows):
        j = int(row_seq[r])
        out["adv"][r] = c[j] if 0 <= j < B else 0.0
    out["c"] = np.asarray(c)
    return out


def mean_loss(res):
    """sum(group_loss) / #alive in fp64 (NaN when no group is alive)"""
    return float(np.sum(res["group_loss"])) * res["alive_inv"]
