"""Fused AdamW over the full-size arena: time per step, HBM bytes per second (30 B per parameter: p, g, m, v
read; p, m, v and the bf16 copy written), and the cost of the transposed-copy refresh that follows it.
Then the gradient-norm pass of `max_grad_norm` / `skip_nonfinite` alone (it reads g once: 4 B per parameter; the skipped
chunks of the arena are not read, both rates count the whole arena) beside the AdamW kernel's rate from the same run, and
optimizer.step() with max_grad_norm set against the plain step as alternating pairs in this one process."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics
import torch
from unimm_amd import VisualDialogEncoder, lib
from unimm_amd.optim import FusedAdamW, default_language_weights, reference_param_groups

dev = torch.device("cuda", 0)
enc = VisualDialogEncoder(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unimm_amd", "config", "bert_base_6layer_6conect.json")).to(dev)
eng = enc.bert_pretrained.engine
groups = lambda: reference_param_groups(enc, 2e-5, 1e-4, default_language_weights(enc))
opt = FusedAdamW(groups(), eng, lr=2e-5)
A = eng.arena
A.grad_flat.normal_()
def t(fn, it=10):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / it
combos, ids = opt._combos()
opt.step()
k = lambda: lib.adamw_step(A.flat, A.grad_flat, opt.exp_avg, opt.exp_avg_sq, opt._group_dev, [c[0] for c in combos], [c[1] for c in combos], 2, w16=eng.w16)
ms = t(k)
print(f"arena {A.numel / 1e6:.1f} M elements, {len(combos)} (lr, wd) groups")
print(f"adamw kernel: {ms:.3f} ms  -> {30 * A.numel / ms / 1e9:.2f} TB/s of 30 B/parameter (HBM peak 8, achievable ~6.3)")
ms_r = t(lambda: eng.refresh_weights(force=True, cast=False))
print(f"transposed-copy refresh: {ms_r:.3f} ms;  optimizer.step() total: {t(opt.step):.3f} ms")

# -- the norm pass (unimm_grad_norm: the sum-of-squares kernel and its one-workgroup finish) -----------------------------------
ws, state = torch.empty(lib.GRAD_NORM_WS_DOUBLES, dtype=torch.float64, device=dev), lib.new_clip_state(dev)
norm = lambda: lib.grad_norm(A.grad_flat, opt._group_dev, len(combos), ws, state, grad_scale=1.0, max_norm=1.0)
ms_n, ms_k = t(norm, it=50), t(k, it=50)
rate_n, rate_k = 4 * A.numel / ms_n / 1e9, 30 * A.numel / ms_k / 1e9
print(f"grad-norm pass: {ms_n:.3f} ms -> {rate_n:.2f} TB/s of 4 B/parameter;  adamw kernel in the same run: {ms_k:.3f} ms -> "
      f"{rate_k:.2f} TB/s of 30 B/parameter  (norm pass at {rate_n / rate_k:.2f} x the kernel's bytes per second)")
clipped = lambda: lib.adamw_step(A.flat, A.grad_flat, opt.exp_avg, opt.exp_avg_sq, opt._group_dev, [c[0] for c in combos],
                                 [c[1] for c in combos], 2, w16=eng.w16, clip_state=state)
print(f"clipped kernel (scale from device memory): {t(clipped, it=50):.3f} ms")

# -- optimizer.step() with and without max_grad_norm: alternating pairs, medians ------------------------------------------
A.grad_flat.normal_()
opt_c = FusedAdamW(groups(), eng, lr=2e-5, max_grad_norm=1.0)
opt_c.exp_avg, opt_c.exp_avg_sq = opt.exp_avg, opt.exp_avg_sq          # one pair of moment arenas: same footprint for both
for o in (opt, opt_c):
    o.step()
plain_ms, clip_ms = [], []
for _ in range(15):
    plain_ms.append(t(opt.step, it=10))
    clip_ms.append(t(opt_c.step, it=10))
mp, mc = statistics.median(plain_ms), statistics.median(clip_ms)
print(f"optimizer.step() plain: median {mp:.3f} ms (min {min(plain_ms):.3f}, max {max(plain_ms):.3f});  max_grad_norm=1.0: median "
      f"{mc:.3f} ms (min {min(clip_ms):.3f}, max {max(clip_ms):.3f});  difference {mc - mp:+.3f} ms over 15 alternating pairs of 10 steps")
print(f"last norm {float(opt_c.last_grad_norm):.6g}, coefficient {float(opt_c.last_clip_coef):.6g}, skipped {opt_c.skipped_steps}")
