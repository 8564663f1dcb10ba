"""FusedAdamW's gradient-norm clipping and non-finite guard on the small model (tests/golden/small_mixed.npz, set up as in
tests/test_gpu_optim.py): the norm against the parameters' own .grad tensors, the clipped update against the oracle tensor by
tensor, the unclipped one against a plain FusedAdamW bit for bit, grad_scale, the skipped step, the constructor's refusals.

One model per engine and ONE backward: every scenario starts from the same saved parameter arena and the same saved gradient
arena (a backward's bits are not reproducible, its weight-gradient sums use atomics) with an optimizer of its own, so two
scenarios compare as a model and its twin would.  Norms: rtol 1e-12, the bound of include/unimm_hip.h (fp64 sums of exact
squares); torch's fp64 sum over each p.grad is the reference."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-12
LR, IMAGE_LR = 2e-3, 1e-2


class Ctx:
    def __init__(self, golden_dir, compute):
        from tests import test_gpu_model as TM, test_gpu_x3_model as TX
        from unimm_amd import params as P
        from unimm_amd.optim import FusedAdamW, reference_param_groups
        mod = TM if compute == "bf16" else TX
        self.model, _, _ = mod.build_small(golden_dir)
        self.model.eval()
        g = np.load(os.path.join(golden_dir, "small_mixed.npz"))
        args, kw = mod.kwargs_from(g)
        self.names = [n for n, _ in self.model.named_parameters()]
        self.lang = [n for i, n in enumerate(self.names) if i % 3 != 0]
        self.unused = {n: P.is_unused(n) for n in self.names}
        self._groups = lambda: reference_param_groups(self.model, lr=LR, image_lr=IMAGE_LR, language_weights=self.lang)
        self._cls = FusedAdamW
        opt = self.optimizer()
        opt.zero_grad()
        lm, img, nsp_l, _, _, _ = self.model(*args, **kw, _want_lm_scores=False)
        (lm + img + nsp_l).sum().backward()
        torch.cuda.synchronize()
        self.arena = A = self.model.engine.arena
        self.P0, self.G = A.flat.clone(), A.grad_flat.clone()
        self.grads = {n: p.grad.detach().cpu().numpy().copy() for n, p in self.model.named_parameters() if p.grad is not None}
        # float64 norms over the parameters' own gradients: all that take a step, and per (lr, weight_decay) pair
        self.pair_sumsq, total = {}, 0.0
        for (n, p), gr in zip(self.model.named_parameters(), opt.param_groups):
            if self.unused[n] or p.grad is None:
                continue
            s = float(p.grad.double().square().sum())
            k = (float(gr["lr"]), float(gr["weight_decay"]))
            self.pair_sumsq[k] = self.pair_sumsq.get(k, 0.0) + s
            total += s
        self.norm = float(np.sqrt(total))

    def optimizer(self, **kw):
        return self._cls(self._groups(), self.model.engine, lr=LR, **kw)

    def start(self, grad_factor=1.0, **kw):
        """the saved parameters and gradients back in the arenas, and a fresh optimizer (zero moments) over them"""
        self.arena.flat.copy_(self.P0)
        self.arena.grad_flat.copy_(self.G * grad_factor)
        self.model.engine.w16.zero_()
        return self.optimizer(**kw)

    def snapshot(self, opt):
        torch.cuda.synchronize()
        return dict(p=self.arena.flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), w16=self.model.engine.w16.clone())


_CTX = {}


@pytest.fixture
def ctx(golden_dir, request):
    compute = getattr(request, "param", "bf16")
    if compute not in _CTX:
        _CTX[compute] = Ctx(golden_dir, compute)
    return _CTX[compute]


def same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("ctx", ["bf16", "fp32x3"], indirect=True)
def test_norm_equals_the_norm_of_the_parameters_own_gradients(ctx):
    """the same data read through p.grad and through the arena: padding that is not zero, or a counted parameter that should not
    be, shows as a difference"""
    opt = ctx.start()
    before = ctx.snapshot(opt)
    got = opt.grad_norm()
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
    print(f"\n{type(ctx.model.engine).__name__}: grad norm {float(got):.17g}, over p.grad {ctx.norm:.17g}")
    assert ctx.norm > 0 and abs(float(got) - ctx.norm) <= RTOL * ctx.norm
    pairs = opt.last_group_grad_norms()
    assert set(pairs) == set(ctx.pair_sumsq) and len(pairs) == 4
    for k, v in pairs.items():
        want = float(np.sqrt(ctx.pair_sumsq[k]))
        assert want > 0 and abs(float(v) - want) <= RTOL * want, k
    assert float(opt.last_clip_coef) == 1.0 and int(opt.last_nonfinite) == 0
    same(before, ctx.snapshot(opt), "grad_norm() updated something")
    assert opt.step_count == 0 and opt.skipped_steps == 0
    opt.grad_scale = 0.25                                         # the norm is that of the gradient the update would see
    assert abs(float(opt.grad_norm()) - 0.25 * ctx.norm) <= RTOL * ctx.norm


def clipped_run(ctx, factor, grad_scale):
    max_norm = 0.5 * ctx.norm
    opt = ctx.start(grad_factor=factor, max_grad_norm=max_norm)
    opt.grad_scale = grad_scale
    lrs = [gr["lr"] for gr in opt.param_groups]
    opt.step()
    snap = ctx.snapshot(opt)
    norm, coef = float(opt.last_grad_norm), float(opt.last_clip_coef)
    assert abs(norm - ctx.norm) <= RTOL * ctx.norm
    assert coef == max_norm / (norm + 1e-6) and coef < 1.0
    assert int(opt.last_nonfinite) == 0 and opt.skipped_steps == 0 and opt.step_count == 1
    return opt, lrs, snap, norm, coef


def test_clipping_active(ctx):
    from oracle import adamw_ref as AR
    opt, lrs, _, _, coef = clipped_run(ctx, 1.0, 1.0)
    scale = np.float32(coef)
    for n, p, gr, lr in zip(ctx.names, ctx.model.parameters(), opt.param_groups, lrs):
        got = p.detach().cpu().numpy()
        p0 = ctx.arena.view(n, ctx.P0).cpu().numpy()
        if ctx.unused[n]:
            assert np.array_equal(got, p0), n
            continue
        if n not in ctx.grads:
            continue
        ref, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
        AR.adamw_step(ref, ctx.grads[n] * scale, m, v, lr, gr["weight_decay"], 1)
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-7), n
        assert not np.array_equal(got, p0) or not ctx.grads[n].any(), n


def test_doubled_gradients_with_grad_scale_half_give_the_same_bits(ctx):
    """accumulation over two micro-batches with grad_scale = 1 / 2: scaling by 2 is exact, in the norm pass and in the update"""
    _, _, snap1, norm1, coef1 = clipped_run(ctx, 1.0, 1.0)
    _, _, snap2, norm2, coef2 = clipped_run(ctx, 2.0, 0.5)
    assert norm1 == norm2 and coef1 == coef2
    same(snap1, snap2, "doubled gradients with grad_scale 0.5")


def test_clipping_inactive_is_the_plain_step(ctx):
    plain_opt = ctx.start()
    plain_opt.step()
    plain = ctx.snapshot(plain_opt)
    assert not torch.equal(plain["p"], ctx.P0)
    for factor, grad_scale in ((1.0, 1.0), (2.0, 0.5)):
        opt = ctx.start(grad_factor=factor, max_grad_norm=10.0 * ctx.norm)
        opt.grad_scale = grad_scale
        opt.step()
        assert float(opt.last_clip_coef) == 1.0 and abs(float(opt.last_grad_norm) - ctx.norm) <= RTOL * ctx.norm
        same(plain, ctx.snapshot(opt), f"max_grad_norm = 10 x norm, gradients x {factor}, grad_scale {grad_scale}")
    guard = ctx.start(skip_nonfinite=True)                         # the guard alone, on a finite gradient
    guard.step()
    same(plain, ctx.snapshot(guard), "skip_nonfinite on a finite gradient")
    assert guard.skipped_steps == 0


def test_nonfinite_guard_skips_the_step(ctx):
    opt = ctx.start(skip_nonfinite=True, max_grad_norm=1.0)
    before = ctx.snapshot(opt)
    name = next(n for n in ctx.names if not ctx.unused[n] and n in ctx.grads and ctx.grads[n].ndim == 2)
    dict(ctx.model.named_parameters())[name].grad[1, 2] = float("inf")
    opt.step()
    same(before, ctx.snapshot(opt), "a skipped step")
    assert int(opt.last_nonfinite) == 1 and float(opt.last_clip_coef) == 1.0
    assert opt.skipped_steps == 1 and opt.step_count == 1
    ctx.arena.grad_flat.copy_(ctx.G)                               # the next, clean step updates
    opt.step()
    after = ctx.snapshot(opt)
    assert not torch.equal(after["p"], before["p"]) and not torch.equal(after["m"], before["m"])
    assert int(opt.last_nonfinite) == 0 and opt.skipped_steps == 1 and opt.step_count == 2
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}
    k0 = next(iter(sd["state"]))
    assert set(sd["state"][k0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][k0]["step"] == 2     # attempted steps
    # without the guard the same poison goes through, as it always did
    opt2 = ctx.start(max_grad_norm=1.0)
    dict(ctx.model.named_parameters())[name].grad[1, 2] = float("nan")
    opt2.step()
    assert int(opt2.last_nonfinite) == 1
    assert torch.isnan(dict(ctx.model.named_parameters())[name].detach()[1, 2])
    ctx.arena.flat.copy_(ctx.P0)


@pytest.mark.parametrize("bad", [0, 0.0, -1, float("nan"), float("inf"), "1", True])
def test_constructor_refuses(ctx, bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        ctx.optimizer(max_grad_norm=bad)
