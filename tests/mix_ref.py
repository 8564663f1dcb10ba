"""Float64 definition of unimm_lm_mix (include/unimm_mix.h) -- TEST INFRASTRUCTURE, the reference of tests/test_mix_cpu.py,
tests/test_gpu_mix_edges.py and tests/test_gpu_ensemble.py -- and a float32 restatement in the kernel's operation order
(`mix_f32`; unimm_amd/csrc/mix/lm_mix.hip states the order at its top).

Per row, K members with fp32 logits x_m[0:V] and weights w_m (rounded to fp32, as the argument struct holds them):

    LOGIT   z_i = sum_m w_m x_m,i                      (fp32: product by product, sum by sum, m ascending -- bit for bit)
    PROB    z_i = log sum_m w_m softmax(x_m)_i         (members with w_m = 0 skipped; -inf entries are probability 0)
    CUT     log_alpha > -inf: m0 = max of x_0 over the eligible ids (not banned, not sep under flags & 1), b the smallest id
            that reaches it, thr = fp32(m0 + log_alpha); out_i = -inf where i != sep, i != b, x_0,i < thr; z_i elsewhere.

The cut is decided in fp32 on fp32 inputs (one add, one compare), so the float64 definition and the restatement share `cut_mask`.

PROB_BUDGET: the largest |mix_f32 - mix_f64| over the finite entries of `budget_cases()` (the -inf pattern must be equal),
measured by tests/test_mix_cpu.py::test_prob_restatement_inside_budget, which prints the figure per case.  Measured 6.21e-06, at
the case "wide" (V = 30522, K = 5, logits of scale 8): its smallest log-probabilities are near -56, where one fp32 rounding is
1.9e-06, and x - lse, t_m, the sum and T + log s each add theirs.  The constant is that figure rounded up to 6.3e-06; the GPU
test holds the device to 4 x PROB_BUDGET (its expf / logf differ from numpy's in the last places, and the compiler may fuse a product
into a sum)."""
import numpy as np

NEG = float("-inf")
F32, F64 = np.float32, np.float64
LOGIT, PROB = 0, 1
NTHREADS, WAVE = 256, 64
PROB_BUDGET = 6.3e-6


def _rows(xs, V):
    return [np.asarray(x)[:, :V] for x in xs]


def cut_mask(x0, banned, flags, sep, log_alpha):
    """bool [rows, V]: the ids the plausibility cut removes.  x0: fp32 [rows, V]; banned: ids (any, those outside [0, V) ban
    nothing); flags: int [rows] or None."""
    x0 = np.asarray(x0, dtype=F32)
    rows, V = x0.shape
    cut = np.zeros((rows, V), dtype=bool)
    if not np.float32(log_alpha) > NEG:
        return cut
    elig = np.ones((rows, V), dtype=bool)
    for b in (banned if banned is not None else ()):
        if 0 <= int(b) < V:
            elig[:, int(b)] = False
    if flags is not None and 0 <= sep < V:
        elig[(np.asarray(flags) & 1) != 0, sep] = False
    for r in range(rows):
        ids = np.nonzero(elig[r])[0]
        if ids.size == 0:
            continue                                       # no eligible id: the row is not cut
        m0 = x0[r, ids].max()
        best = int(ids[np.argmax(x0[r, ids] == m0)])        # the smallest id that reaches it
        with np.errstate(invalid="ignore"):
            thr = np.float32(m0) + np.float32(log_alpha)    # one fp32 add
            c = x0[r] < thr
        c[best] = False
        if 0 <= sep < V:
            c[sep] = False
        cut[r] = c
    return cut


def _lse64(x):
    m = x.max(1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return m[:, 0] + np.log(np.exp(x - m).sum(1))


def mix_f64(xs, weights, mode, V, banned=None, flags=None, sep=102, log_alpha=NEG):
    """The definition in float64 -> float64 [rows, V] (-inf where cut, or where the mixture has probability 0)."""
    xs = _rows(xs, V)
    w = [F64(F32(v)) for v in weights]
    x64 = [x.astype(F64) for x in xs]
    if mode == LOGIT:
        z = sum(wm * x for wm, x in zip(w, x64))
    else:
        ts = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for wm, x in zip(w, x64):
                if wm != 0:
                    ts.append(np.where(x > NEG, x - _lse64(x)[:, None] + np.log(wm), NEG))
            T = np.max(ts, axis=0)
            Ts = np.where(np.isfinite(T), T, 0.0)
            z = np.where(T > NEG, Ts + np.log(sum(np.exp(t - Ts) for t in ts)), NEG)
    return np.where(cut_mask(xs[0], banned, flags, sep, log_alpha), NEG, z)


def lse_f32(x):
    """logsumexp of fp32 rows in the kernel's order (the scalar path): 256 threads fold columns t, t + 256, ... into (mx, s)
    pairs, the xor butterfly combines them over each wave, the four waves combine in order."""
    x = np.asarray(x, dtype=F32)
    rows, V = x.shape
    steps = -(-V // NTHREADS)
    pad = np.full((rows, steps * NTHREADS), NEG, dtype=F32)
    pad[:, :V] = x
    pad = pad.reshape(rows, steps, NTHREADS)
    mx = np.full((rows, NTHREADS), NEG, dtype=F32)
    sm = np.zeros((rows, NTHREADS), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(steps):
            v = pad[:, t]
            mn = np.maximum(mx, v)
            ok = mn > NEG
            s = sm * np.exp(mx - mn) + np.exp(v - mn)       # a column past V (-inf) adds exp(-inf) = 0 to s * exp(0)
            sm, mx = np.where(ok, s, sm).astype(F32), np.where(ok, mn, mx)
        lane = np.arange(NTHREADS)
        for o in (32, 16, 8, 4, 2, 1):
            m2, s2 = mx[:, lane ^ o], sm[:, lane ^ o]
            M = np.maximum(mx, m2)
            s = (sm * np.exp(mx - M) + s2 * np.exp(m2 - M)).astype(F32)
            sm, mx = np.where(M == NEG, F32(0), s), M
        wm, ws = mx[:, ::WAVE], sm[:, ::WAVE]               # lane 0 of every wave
        M = wm.max(1)
        tot = np.zeros(rows, dtype=F32)
        for k in range(NTHREADS // WAVE):
            tot = np.where(wm[:, k] > NEG, tot + ws[:, k] * np.exp(wm[:, k] - M), tot).astype(F32)
        with np.errstate(divide="ignore"):
            return (M + np.log(tot)).astype(F32)


def mix_f32(xs, weights, mode, V, banned=None, flags=None, sep=102, log_alpha=NEG):
    """The restatement in float32, every operation rounded on its own -> float32 [rows, V]."""
    xs = [np.asarray(x, dtype=F32) for x in _rows(xs, V)]
    w = [F32(v) for v in weights]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode == LOGIT:
            z = w[0] * xs[0]
            for wm, x in zip(w[1:], xs[1:]):
                z = z + wm * x
        else:
            ts = []
            for wm, x in zip(w, xs):
                if wm != 0:
                    ts.append(np.where(x > NEG, (x - lse_f32(x)[:, None]) + np.log(wm), F32(NEG)).astype(F32))
            T = ts[0]
            for t in ts[1:]:
                T = np.maximum(T, t)
            s = np.zeros_like(T)
            for t in ts:
                s = s + np.exp(t - T)
            z = np.where(T > NEG, T + np.log(s), F32(NEG))
    assert z.dtype == F32
    return np.where(cut_mask(xs[0], banned, flags, sep, log_alpha), F32(NEG), z)


def prob_weights(K):
    """Uneven convex weights of K members, one of them 0 from K = 3 on (a skipped member)."""
    w = np.arange(1, K + 1, dtype=F64)
    if K >= 3:
        w[1] = 0.0
    return [float(v) for v in (w / w.sum()).astype(F32)]


def logit_weights(K):
    """Weights of both signs, member 0's positive."""
    return [float(F32(v)) for v in (1.5, -0.5, 0.25, -1.25, 0.75)[:K]]


def edge_rows(V, rows, K, seed, scale=4.0, holes=True, first=False):
    """K blocks of fp32 logits [rows, V]: normal logits of the given scale, a different offset per member and row (a log-sum-exp
    away from 0); with `holes`, a tenth of the entries -inf in every member from member 1 on (with `first`, in member 0 too) and
    the last member's last row -inf throughout."""
    rng = np.random.RandomState(seed)
    xs = []
    for m in range(K):
        x = (rng.standard_normal((rows, V)) * scale + rng.uniform(-20, 20, (rows, 1))).astype(F32)
        if holes and (m >= 1 or first):
            x[rng.random_sample((rows, V)) < 0.1] = NEG
        xs.append(x)
    if holes and K >= 2 and V >= 3:
        xs[-1][rows - 1, :] = NEG                          # a member without any probability in one row
    return xs


def budget_cases():
    """(name, V, K, xs, weights): the inputs PROB_BUDGET is measured on -- the GPU edge test's shapes and scales."""
    out = []
    for V in (3, 16, 257, 30522, 65536):
        for K in (1, 2, 3, 5):
            rows = 3 if V >= 30522 else 7
            out.append((f"edge V={V}", V, K, edge_rows(V, rows, K, 100 + V % 97 + K, first=K % 2 == 1), prob_weights(K)))
    out.append(("wide", 30522, 5, edge_rows(30522, 3, 5, 7, scale=8.0), prob_weights(5)))
    out.append(("peaked", 257, 2, [np.where(np.arange(257)[None] == 5, F32(60.0), x) for x in edge_rows(257, 4, 2, 9, holes=False)],
                [0.5, 0.5]))
    x = edge_rows(257, 4, 2, 11, holes=False)
    x[0][:, 3], x[1][:, 3] = NEG, NEG                      # probability 0 in every contributing member
    out.append(("all -inf at an id", 257, 2, x, [0.25, 0.75]))
    return out
