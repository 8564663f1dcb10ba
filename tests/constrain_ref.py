"""numpy restatement of the two history rules of answer generation (unimm_amd/generation.py, `unimm_lm_history` in
include/unimm_hip.h), written from their definition: for one row, the set of ids the no-repeat n-gram rule bans and the fp32
row the repetition penalty selects by.  A row's sources are its answer tokens `answer` = a[0, k) and, optionally, its dialog's
context tokens `context`; both are plain integer sequences, already cut to their lengths."""
import numpy as np


def sources(answer, context=None):
    out = [[int(t) for t in answer]]
    if context is not None:
        out.append([int(t) for t in context])
    return out


def ban_set(answer, context, n, V, sep):
    """Ids banned at step k = len(answer): t such that some source s and some end e >= n - 1 have
    s[e-n+1 .. e) == a[k-n+1 .. k) and s[e] == t; never `sep`, never an id outside [0, V)."""
    a = [int(t) for t in answer]
    k = len(a)
    banned = set()
    if n <= 0 or k < n - 1:
        return banned
    for s in sources(a, context):
        for e in range(n - 1, len(s)):
            match = True
            for d in range(1, n):                            # s[e - d] against a[k - d]
                if s[e - d] != a[k - d]:
                    match = False
            if match and 0 <= s[e] < V and s[e] != sep:
                banned.add(s[e])
    return banned


def penalised_row(x, answer, context, penalty, inv_penalty):
    """x'_i = x_i > 0 ? x_i * inv_penalty : x_i * penalty for every id i of a source, x_i elsewhere: fp32 products."""
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    r, inv = np.float32(penalty), np.float32(inv_penalty)
    for s in sources(answer, context):
        for t in s:
            if 0 <= t < x.shape[0]:
                with np.errstate(invalid="ignore"):
                    out[t] = x[t] * inv if x[t] > 0 else x[t] * r
    return out


def repeats_ngram(tokens, n, context=None):
    """Does the answer `tokens` (without its [SEP]) complete an n-gram twice, or (context given) one of the context's?  The
    independent check of the searches' results: a set of tuples."""
    tokens = [int(t) for t in tokens]
    seen = set()
    if context is not None:
        c = [int(t) for t in context]
        seen = {tuple(c[i:i + n]) for i in range(len(c) - n + 1)}
    for i in range(len(tokens) - n + 1):
        g = tuple(tokens[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False
