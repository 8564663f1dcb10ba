"""The float64 restatement of the CIDEr-D definition of include/unimm_reward.h, in plain Python loops over dicts of tuples: what
tests/test_reward_cpu.py holds to hand-worked cases and tests/test_gpu_reward_*.py hold the kernel to.  It is written from the
definition, not from the kernel; it also restates, in numpy and on its own, the hash and the probing of the document-frequency
table.  Answers are sequences of ints with a length that counts the [SEP]; length <= 0 = absent."""
import math

import numpy as np

ORDERS = 4
EMPTY = -2
HASH_BASIS, HASH_PRIME = 2166136261, 16777619


# ---- the table: hash, probe, document frequencies ------------------------------------------------------------------------------

def key_of(x):
    """an n-gram (tuple of 1 .. 4 ints) as its key: padded with -1"""
    return tuple(x) + (-1,) * (4 - len(x))


def hash_key(key):
    """FNV-1a over the four words in uint32 arithmetic, then h ^= h >> 16"""
    h = np.uint32(HASH_BASIS)
    with np.errstate(over="ignore"):
        for word in key:
            h = np.uint32((h ^ np.uint32(word & 0xFFFFFFFF)) * np.uint32(HASH_PRIME))
    return int(h ^ (h >> np.uint32(16)))


def probe(table_keys, key):
    """(slot, found, probes): linear probing from the home slot until the key, an empty slot or cap probes"""
    cap = len(table_keys)
    assert cap >= 1 and cap & (cap - 1) == 0
    slot = hash_key(key) & (cap - 1)
    for i in range(cap):
        if int(table_keys[slot][0]) == EMPTY:
            return slot, False, i + 1
        if tuple(int(v) for v in table_keys[slot]) == tuple(key):
            return slot, True, i + 1
        slot = (slot + 1) & (cap - 1)
    return slot, False, cap


def table_idf(table_keys, table_values, default_idf):
    """idf(x) as a lookup in a built table (each n-gram is probed once, then remembered)"""
    keys = [tuple(int(v) for v in row) for row in table_keys]
    known = {}

    def idf(x):
        if x not in known:
            slot, found, _ = probe(keys, key_of(x))
            known[x] = float(table_values[slot]) if found else float(default_idf)
        return known[x]
    return idf


def windows(tokens, length, n):
    L = max(0, int(length) - 1)
    return [tuple(int(t) for t in tokens[p:p + n]) for p in range(max(0, L - n + 1))]


def document_frequencies(tokens, lengths):
    """({n-gram: number of corpus answers holding it}, D)"""
    df = {}
    for row, length in zip(tokens, lengths):
        seen = set()
        for n in range(1, ORDERS + 1):
            seen.update(windows(row, length, n))
        for x in seen:
            df[x] = df.get(x, 0) + 1
    return df, len(lengths)


def corpus_idf(tokens, lengths):
    """idf(x) = log(D) - log(max(1, df(x))) of a corpus"""
    df, D = document_frequencies(tokens, lengths)
    return lambda x: math.log(D) - math.log(max(1, df.get(x, 0)))


def unit_idf(x):
    """without a table every idf is exactly 1"""
    return 1.0


# ---- the score ------------------------------------------------------------------------------------------------------------------

def vector(tokens, length, n, idf):
    """{n-gram: tf * idf} in order of first position"""
    tf = {}
    for x in windows(tokens, length, n):
        tf[x] = tf.get(x, 0) + 1
    return {x: c * idf(x) for x, c in tf.items()}


def norm(v):
    s = 0.0
    for val in v.values():
        s = s + val * val
    return math.sqrt(s)


def val_n(h, h_len, r, r_len, n, idf, sigma, memo=None):
    """memo: a dict that keeps a reference's vector between hypotheses (the same values, formed once)"""
    vh = vector(h, h_len, n, idf)
    if memo is None:
        vr = vector(r, r_len, n, idf)
    else:
        if (id(r), n) not in memo:
            memo[(id(r), n)] = vector(r, r_len, n, idf)
        vr = memo[(id(r), n)]
    val = 0.0
    for x, a in vh.items():
        b = vr.get(x, 0.0)
        val = val + min(a, b) * b
    den = norm(vh) * norm(vr)
    if den != 0.0:
        val = val / den
    d = float((int(h_len) - 1) - (int(r_len) - 1))
    factor = 1.0 if math.isinf(sigma) else math.exp(-(d * d) / (2.0 * sigma * sigma))
    return val * factor


def score_row(h, h_len, refs, ref_lens, weights=None, idf=unit_idf, sigma=6.0, memo=None):
    """(reward, [c_1 .. c_4]) of one hypothesis against its dialog's references"""
    zeros = [0.0] * ORDERS
    if int(h_len) - 1 <= 0:
        return 0.0, zeros
    present = [j for j in range(len(ref_lens)) if int(ref_lens[j]) > 0]
    w = [1.0 if weights is None else float(weights[j]) for j in range(len(ref_lens))]
    wsum = 0.0
    for j in present:
        wsum = wsum + w[j]
    if not present or wsum == 0.0:
        return 0.0, zeros
    c = []
    for n in range(1, ORDERS + 1):
        acc = 0.0
        for j in present:
            v = 0.0 if int(ref_lens[j]) - 1 <= 0 else val_n(h, h_len, refs[j], ref_lens[j], n, idf, sigma, memo)
            acc = acc + w[j] * v
        c.append(acc / wsum)
    return 10.0 * (((c[0] + c[1]) + c[2]) + c[3]) / 4.0, c


def score_rows(hyp, hyp_len, hyp_group, ref, ref_len, ref_weight=None, idf=unit_idf, sigma=6.0):
    """(rewards float64 [S], per_order float64 [S, 4]): row s against the references of dialog hyp_group[s]"""
    S = len(hyp_len)
    rewards, orders = np.zeros(S), np.zeros((S, ORDERS))
    ref = [[[int(t) for t in row] for row in group] for group in ref]          # plain lists: one object per reference
    memo = {}
    for s in range(S):
        g = int(hyp_group[s])
        rewards[s], orders[s] = score_row([int(t) for t in hyp[s]], hyp_len[s], ref[g], ref_len[g],
                                          None if ref_weight is None else ref_weight[g], idf, sigma, memo)
    return rewards, orders


def score(tokens, lengths, ref, ref_len, ref_weight=None, idf=unit_idf, sigma=6.0):
    """rewards float64 [G, N] of tokens [G, N, W], lengths [G, N]"""
    G, N = np.asarray(lengths).shape
    flat_t = [tokens[g][i] for g in range(G) for i in range(N)]
    flat_l = [lengths[g][i] for g in range(G) for i in range(N)]
    r, _ = score_rows(flat_t, flat_l, [g for g in range(G) for _ in range(N)], ref, ref_len, ref_weight, idf, sigma)
    return r.reshape(G, N)
