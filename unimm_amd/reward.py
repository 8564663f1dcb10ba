"""The reward of self-critical answer training, computed on the device: CIDEr-D, the n-gram TF-IDF consensus of a hypothesis
with the reference answers of its dialog (for Visual Dialog: a round's candidate options weighted by their dense relevance, the
data `policy.relevance_targets` consumes).  The definition, the document-frequency table and the limits are stated ONCE, in
include/unimm_reward.h; the kernel is `unimm_ngram_reward` of libunimm_reward.so (unimm_amd/reward_abi.py), and there is no host
fallback.  Parity with a CIDEr library is unpinned (none was at hand); tests/reward_ref.py restates the header in float64 Python.

    table = NgramTable.from_corpus(tokens, lengths)            # document frequencies of a corpus of answers, once
    reward = CiderD(table)                                     # or CiderD(): every idf = 1, no corpus needed
    trainer.self_critical_step(..., reward_fn=reward, ...)     # batch carries reference_tokens / reference_lengths [/ _weights]
    mean, per_answer = metrics.cider_d(answers, None, reference_tokens, reference_lengths, table=table)

An answer is a token row "tokens, then [SEP], zero padded" with a length that counts the [SEP] (0 = absent): the convention of
`GeneratedAnswers` and of `candidate_training_batch`, for hypotheses and references alike."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import reward_abi as A

MAX_LEN, MAX_REFS, ORDERS = A.MAX_LEN, A.MAX_REFS, A.ORDERS


def ngram_hash(keys):
    """The header's hash of n-gram keys (int [K, 4], tokens padded with -1) -> uint32 [K]: FNV-1a over the four words in uint32
    arithmetic, then h ^= h >> 16.  The home slot of a key in a table of `cap` slots is `hash & (cap - 1)`."""
    k = np.asarray(keys).astype(np.int64).astype(np.uint32).reshape(-1, 4)     # two's complement words
    h = np.full(k.shape[0], A.HASH_BASIS, dtype=np.uint32)
    for i in range(4):
        h = (h ^ k[:, i]) * np.uint32(A.HASH_PRIME)                            # wraps modulo 2^32
    return h ^ (h >> np.uint32(16))


def corpus_ngrams(tokens, lengths):
    """(keys int32 [K, 4] sorted, df int64 [K]) of a corpus: every distinct n-gram (n = 1 .. 4) of the answers `tokens` [D, W] with
    `lengths` [D] (counting the [SEP]; <= 0 = an empty document, which still counts in D), and the number of DOCUMENTS holding it."""
    tok = np.asarray(tokens).astype(np.int64)
    L = np.maximum(np.asarray(lengths).astype(np.int64).reshape(-1) - 1, 0)
    if tok.ndim != 2 or L.shape[0] != tok.shape[0]:
        raise ValueError(f"corpus: tokens must be [D, W] and lengths [D], got {tok.shape} and {np.asarray(lengths).shape}")
    if L.size and int(L.max()) > min(MAX_LEN, tok.shape[1] - 1):
        raise ValueError(f"corpus: lengths: an answer of {int(L.max())} tokens (at most {MAX_LEN}, and its [SEP] inside the row)")
    D, W = tok.shape
    rows = []
    for n in range(1, ORDERS + 1):
        if W - n + 1 <= 0:
            continue
        pos = np.arange(W - n + 1)
        doc, p = np.nonzero(pos[None, :] + n <= L[:, None])
        key = np.full((doc.size, 5), -1, dtype=np.int64)
        key[:, 0] = doc
        for e in range(n):
            key[:, 1 + e] = tok[doc, p + e]
        rows.append(np.unique(key, axis=0))                                    # once per document
    allrows = np.concatenate(rows) if rows else np.zeros((0, 5), np.int64)
    keys, df = np.unique(allrows[:, 1:], axis=0, return_counts=True)
    return keys.astype(np.int32), df.astype(np.int64)


def build_table(keys, values, max_load=0.5, cap=None):
    """(table_keys int32 [cap, 4], table_values float64 [cap]) of the header's open-addressing table: cap the smallest power of
    two with K <= max_load * cap (or the given one), every key at the first free slot of its linear probe, empty slots marked
    `reward_abi.EMPTY` in their first word."""
    keys = np.asarray(keys, dtype=np.int32).reshape(-1, 4)
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    K = keys.shape[0]
    if not 0.0 < max_load <= 1.0:
        raise ValueError(f"build_table: max_load must be in (0, 1], got {max_load}")
    if cap is None:
        cap = 1
        while cap * max_load < K or cap < 2:
            cap *= 2
    if cap < max(K, 1) or cap & (cap - 1):
        raise ValueError(f"build_table: cap must be a power of two that holds {K} keys, got {cap}")
    tk = np.full((cap, 4), -1, dtype=np.int32)
    tk[:, 0] = A.EMPTY
    tv = np.zeros(cap, dtype=np.float64)
    used = np.zeros(cap, dtype=bool)
    slot = (ngram_hash(keys) & np.uint32(cap - 1)).astype(np.int64)
    pending = np.arange(K)
    while pending.size:
        s = slot[pending]
        free = ~used[s]
        _, first = np.unique(s[free], return_index=True)                       # one winner per free slot: the first in key order
        win = pending[free][first]
        tk[slot[win]], tv[slot[win]], used[slot[win]] = keys[win], values[win], True
        pending = np.setdiff1d(pending, win, assume_unique=True)
        slot[pending] = (slot[pending] + 1) & (cap - 1)                        # a loser's slot is taken now: probe on
    return tk, tv


class NgramTable:
    """The document-frequency table of a corpus as the kernel reads it: `keys` int32 [cap, 4], `idf` float64 [cap] (log(D) -
    log(df), taken on the host in float64), `default_idf` = log(D) for n-grams it does not hold, `num_docs` = D."""

    def __init__(self, keys, idf, default_idf, num_docs):
        self.keys = torch.as_tensor(keys, dtype=torch.int32).contiguous()
        self.idf = torch.as_tensor(idf, dtype=torch.float64).contiguous().to(self.keys.device)
        cap = self.keys.shape[0]
        if self.keys.dim() != 2 or self.keys.shape[1] != 4 or tuple(self.idf.shape) != (cap,) or cap < 1 or cap & (cap - 1):
            raise ValueError(f"NgramTable: keys must be int32 [cap, 4] and idf float64 [cap] with cap a power of two, got "
                             f"{tuple(self.keys.shape)} and {tuple(self.idf.shape)}")
        self.default_idf, self.num_docs = float(default_idf), int(num_docs)

    @classmethod
    def from_corpus(cls, tokens, lengths, max_load=0.5, device=None):
        """Count on the host (numpy) and build the table; `device` (default: the current GPU when there is one) is where it goes."""
        tok = tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else np.asarray(tokens)
        ln = lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
        keys, df = corpus_ngrams(tok, ln)
        D = tok.shape[0]
        if D < 1:
            raise ValueError("NgramTable.from_corpus: the corpus is empty")
        log_d = math.log(D)
        idf = np.array([log_d - math.log(max(1, int(c))) for c in df], dtype=np.float64)
        tk, tv = build_table(keys, idf, max_load)
        table = cls(tk, tv, log_d, D)
        if device is None and torch.cuda.is_available():
            device = "cuda"
        return table.to(device) if device is not None else table

    @property
    def device(self):
        return self.keys.device

    @property
    def cap(self):
        return self.keys.shape[0]

    def to(self, device):
        out = NgramTable.__new__(NgramTable)
        out.keys, out.idf, out.default_idf, out.num_docs = self.keys.to(device), self.idf.to(device), self.default_idf, self.num_docs
        return out

    def state_dict(self):
        return {"keys": self.keys.cpu(), "idf": self.idf.cpu(), "default_idf": self.default_idf, "num_docs": self.num_docs}

    def load_state_dict(self, state):
        new = NgramTable(state["keys"], state["idf"], state["default_idf"], state["num_docs"]).to(self.device)
        self.keys, self.idf, self.default_idf, self.num_docs = new.keys, new.idf, new.default_idf, new.num_docs
        return self


class DeviceReward:
    """A reward `trainer.self_critical_step` computes on the device: instead of `reward_fn(tokens.cpu(), lengths.cpu())` the step
    calls `score(answers.tokens, answers.lengths, batch["reference_tokens"], batch["reference_lengths"],
    batch.get("reference_weights"))` -> fp32 [G, N] on the device, and brings only that to the host."""

    def score(self, tokens, lengths, reference_tokens, reference_lengths, reference_weights=None):
        raise NotImplementedError


def _host_max(t):
    return int(t.max()) if t.numel() else 0


def _device_of(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return None


class CiderD(DeviceReward):
    """CIDEr-D against weighted references (include/unimm_reward.h).  table: an `NgramTable` on the device, or None for idf = 1
    everywhere; sigma: of the length factor, math.inf = none."""

    def __init__(self, table=None, sigma=6.0):
        if table is not None and not isinstance(table, NgramTable):
            raise ValueError(f"CiderD: table must be an NgramTable or None, got {type(table).__name__}")
        sigma = float(sigma)
        if not sigma > 0.0:
            raise ValueError(f"CiderD: sigma must be positive, got {sigma}")
        self.table, self.sigma = table, sigma

    def score(self, tokens, lengths, reference_tokens, reference_lengths, reference_weights=None):
        """tokens [G, N, W], lengths [G, N] (int64 or int32, on the device or the host; host input is staged) against
        reference_tokens [G, M, Wr], reference_lengths [G, M], reference_weights [G, M] >= 0 or None -> fp32 [G, N], device."""
        tokens, lengths = torch.as_tensor(tokens), torch.as_tensor(lengths)
        if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]):
            raise ValueError(f"CiderD.score: tokens must be [G, N, W] and lengths [G, N], got {tuple(tokens.shape)} and "
                             f"{tuple(lengths.shape)}")
        G, N, W = tokens.shape
        if torch.as_tensor(reference_tokens).dim() == 3 and torch.as_tensor(reference_tokens).shape[0] != G:
            raise ValueError(f"CiderD.score: reference_tokens must hold the {G} dialogs of tokens, got "
                             f"{tuple(torch.as_tensor(reference_tokens).shape)}")
        groups = torch.arange(G, dtype=torch.int32).repeat_interleave(N)
        out = self.score_rows(tokens.reshape(G * N, W), lengths.reshape(G * N), groups, reference_tokens, reference_lengths,
                              reference_weights)
        return out.view(G, N)

    def score_rows(self, tokens, lengths, groups, reference_tokens, reference_lengths, reference_weights=None, per_order=False):
        """The flat form: tokens [S, W], lengths [S], groups [S] (the dialog whose references row s is scored against, in any
        order) -> fp32 [S] on the device; per_order=True -> (that, the c_n as float64 [S, 4]).
        Everything is checked before anything is staged (ValueError naming the argument); lengths that live on the device are
        checked through one two-number readback."""
        tokens, lengths, groups = torch.as_tensor(tokens), torch.as_tensor(lengths), torch.as_tensor(groups)
        rt, rl = torch.as_tensor(reference_tokens), torch.as_tensor(reference_lengths)
        rw = None if reference_weights is None else torch.as_tensor(reference_weights)
        if tokens.dim() != 2 or tokens.shape[1] < 1:
            raise ValueError(f"CiderD: tokens must be [S, W], got {tuple(tokens.shape)}")
        S, W = tokens.shape
        if tuple(lengths.shape) != (S,):
            raise ValueError(f"CiderD: lengths must be [{S}], got {tuple(lengths.shape)}")
        if tuple(groups.shape) != (S,):
            raise ValueError(f"CiderD: groups must be [{S}], got {tuple(groups.shape)}")
        if rt.dim() != 3 or rt.shape[0] < 1 or rt.shape[1] < 1 or rt.shape[2] < 1:
            raise ValueError(f"CiderD: reference_tokens must be [G, M, Wr], got {tuple(rt.shape)}")
        G, M, Wr = rt.shape
        if M > MAX_REFS:
            raise ValueError(f"CiderD: reference_tokens: {M} references per dialog, at most {MAX_REFS}")
        if tuple(rl.shape) != (G, M):
            raise ValueError(f"CiderD: reference_lengths must be [{G}, {M}], got {tuple(rl.shape)}")
        if rw is not None:
            if tuple(rw.shape) != (G, M):
                raise ValueError(f"CiderD: reference_weights must be [{G}, {M}], got {tuple(rw.shape)}")
            if rw.numel() and not bool((torch.isfinite(rw.float()) & (rw >= 0)).all()):
                raise ValueError("CiderD: reference_weights must be finite and >= 0")
        for name, t in (("tokens", tokens), ("lengths", lengths), ("groups", groups), ("reference_tokens", rt),
                        ("reference_lengths", rl)):
            if t.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"CiderD: {name} must be int64 or int32, got {t.dtype}")
        for name, t, width in (("lengths", lengths, W), ("reference_lengths", rl, Wr)):
            top = _host_max(t)
            if top - 1 > MAX_LEN or top > width:
                raise ValueError(f"CiderD: {name}: a length of {top} (at most {MAX_LEN} tokens and a [SEP], inside a row of {width})")
        if S and (int(groups.min()) < 0 or int(groups.max()) >= G):
            raise ValueError(f"CiderD: groups must lie in [0, {G})")
        device = _device_of(tokens, lengths, groups, rt, rl, rw)
        if self.table is not None:
            if not self.table.device.type == "cuda" or (device is not None and device != self.table.device):
                raise ValueError(f"CiderD: table is on {self.table.device}, the input on {device}: move it with table.to(device)")
            device = self.table.device
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        for name, t in (("tokens", tokens), ("lengths", lengths), ("groups", groups), ("reference_tokens", rt),
                        ("reference_lengths", rl), ("reference_weights", rw)):
            if t is not None and t.is_cuda and t.device != device:
                raise ValueError(f"CiderD: {name} is on {t.device}, other input on {device}")

        def stage(t, dtype):
            return t.to(device=device, dtype=dtype).contiguous()
        with torch.cuda.device(device):
            hyp, hl, hg = stage(tokens, torch.int32), stage(lengths, torch.int32), stage(groups, torch.int32)
            ref, rln = stage(rt, torch.int32), stage(rl, torch.int32)
            wts = None if rw is None else stage(rw, torch.float32)
            reward = torch.empty(S, dtype=torch.float32, device=device)
            orders = torch.empty((S, ORDERS), dtype=torch.float64, device=device) if per_order else None
            tab = self.table
            A.ngram_reward(hyp, hl, hg, ref, rln, wts, None if tab is None else tab.keys, None if tab is None else tab.idf,
                           0.0 if tab is None else tab.default_idf, self.sigma, reward, orders,
                           max_hyp_len=min(W, MAX_LEN + 1), max_ref_len=min(Wr, MAX_LEN + 1))
        return (reward, orders) if per_order else reward
