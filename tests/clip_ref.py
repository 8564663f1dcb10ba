"""Float64 numpy restatement of the gradient-norm pass (include/unimm_hip.h: unimm_grad_norm), for the clipping tests.

A 64-element chunk counts when its group id is below n_groups; every counted element is squared and summed in float64 per group,
the groups are added in index order, and
    norm = |grad_scale| sqrt(sumsq);  nonfinite = !isfinite(sumsq);  coef = min(1, max_norm / (norm + 1e-6))
(coef = 1 when max_norm is +inf or when nonfinite is set);  scale = float32(float64(grad_scale) * coef).
tests/test_clip_ref_cpu.py pins this to torch.nn.utils.clip_grad_norm_."""
import numpy as np

MAX_GROUPS = 8


def clip_ref(g, elem_group, n_groups, grad_scale=1.0, max_norm=np.inf):
    """g: float32 [n]; elem_group: the group id of every ELEMENT (np.repeat(table, 64)).  -> dict(group_sumsq [8], sumsq, norm,
    coef (float64), scale (float32), nonfinite (0 / 1))"""
    g = np.asarray(g, np.float32)
    elem_group = np.asarray(elem_group)
    assert g.shape == elem_group.shape and 1 <= n_groups <= MAX_GROUPS
    grad_scale = np.float32(grad_scale)
    group_sumsq = np.zeros(MAX_GROUPS, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(n_groups):
            x = g[elem_group == k].astype(np.float64)          # elements of other chunks are never looked at
            group_sumsq[k] = np.sum(x * x)
        sumsq = np.float64(0.0)
        for k in range(n_groups):
            sumsq = sumsq + group_sumsq[k]
        nonfinite = int(not np.isfinite(sumsq))
        norm = np.abs(np.float64(grad_scale)) * np.sqrt(sumsq)
        coef = np.float64(1.0)
        if not nonfinite and np.isfinite(max_norm):
            coef = min(np.float64(1.0), np.float64(max_norm) / (norm + 1e-6))
        scale = np.float32(np.float64(grad_scale) * coef)
    return dict(group_sumsq=group_sumsq, sumsq=sumsq, norm=norm, coef=coef, scale=scale, nonfinite=nonfinite)
