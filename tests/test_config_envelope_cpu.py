"""The config envelope on the CPU: the four cases of tests/envelope_case.py against the float64 oracle alone, and what
`BertConfig.validate_for_hip()` admits and refuses.

  * the four configurations build, take the seeded state dict with strict=True and run the oracle's training step;
  * THE GATE BITES at these shapes: for every dropout site of every configuration (96 in all) the oracle with that site's mask
    replaced by the next step's moves some live tensor by more than 2 G in relative L2, G = `grad_ref.gate()` = 0.1323 -- so a
    per-tensor check at G (tests/test_gpu_config_envelope.py) sees a wrong mask at any site.  A condition on the batch, not a
    measurement: smallest values swapped 0.276, odd 0.295, narrow 0.307, wide 0.343.  If a change to the batch breaks it, the
    batch changes, not the factor;
  * live / dead tensor counts as found: swapped 178 / 11, narrow 103 / 6, wide 103 / 6, odd 148 / 9;
  * `validate_for_hip`: one refusal per rule, matched on its message, and an acceptance at each limit."""
import json
import os

import pytest
import torch

from tests import envelope_case as EC
from tests import grad_ref as GR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("case", EC.IDS)
def test_case_builds_loads_and_runs_the_oracle(case):
    from unimm_amd import BertForMultiModalPreTraining
    c = EC.build(case)
    model = BertForMultiModalPreTraining(c["cfg"])
    model.load_state_dict(c["sd"], strict=True)
    base = c["base"]
    for k, v in base["losses"].items():
        assert torch.isfinite(v).all() and float(v.sum()) > 0, (k, v)
    assert base["nsp"].shape[0] == EC.N_SEQ and torch.isfinite(base["nsp"]).all()
    cmp = GR.compare(base["grads"], base["grads"])
    live = sum(not v["dead"] for v in cmp.values())
    assert (live, len(cmp) - live) == EC.LIVE_DEAD[case], (live, len(cmp) - live)
    assert len(base["sites"]) == 3 + 3 * (c["ocfg"].num_hidden_layers + c["ocfg"].v_num_hidden_layers) + 6 * len(c["ocfg"].v_biattention_id)


def test_the_four_cases_have_96_sites():
    assert sum(len(GR.site_names(EC.build(case)["ocfg"])) for case in EC.IDS) == 96


@pytest.mark.parametrize("case", EC.IDS)
def test_gate_bites_at_every_dropout_site(case):
    c = EC.build(case)
    G = GR.gate()
    moved = {}
    for site in GR.site_names(c["ocfg"]):
        mut = EC.oracle_run(c, {site: "key"})
        cmp = GR.compare(mut["grads"], c["base"]["grads"])
        moved[site] = max(v["l2"] for v in cmp.values() if not v["dead"])
    weakest = min(moved, key=moved.get)
    print(f"\n{case}: {len(moved)} sites, smallest largest-change {moved[weakest]:.4f} at {weakest} (2 G = {2 * G:.4f})")
    assert all(v > 2 * G for v in moved.values()), sorted((v, s) for s, v in moved.items() if v <= 2 * G)
    a, b = EC.control_sites(c["ocfg"])
    assert a in moved and b in moved


# ---- validate_for_hip -------------------------------------------------------------------------------------------------------
def _cfg(**switches):
    from unimm_amd import BertConfig
    with open(os.path.join(GOLDEN, "small_config.json")) as f:
        return BertConfig.from_dict(dict(json.load(f), **switches))


FAMILIES = {"text": ("hidden_size", "num_attention_heads"), "image": ("v_hidden_size", "v_num_attention_heads"),
            "bi": ("bi_hidden_size", "bi_num_attention_heads")}
SIZES = ("hidden_size", "v_hidden_size", "bi_hidden_size", "intermediate_size", "v_intermediate_size", "v_feature_size")


def test_small_config_and_the_default_pass():
    from unimm_amd import BertConfig
    _cfg().validate_for_hip()
    BertConfig(30522).validate_for_hip()                       # 768 / 768 / 1024, heads 12 / 12 / 16: every head size 64


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("head", [32, 96, 256])
def test_refuses_head_sizes_other_than_64_and_128(family, head):
    width, heads = FAMILIES[family]
    cfg = _cfg(**{width: 2 * head, heads: 2})                  # widths 64, 192, 512: multiples of 64, only the head size is wrong
    with pytest.raises(ValueError, match=rf"{family} head size {head} not in \(64,128\)"):
        cfg.validate_for_hip()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_refuses_a_width_that_is_no_multiple_of_its_head_count(family):
    width, heads = FAMILIES[family]
    cfg = _cfg(**{width: 320, heads: 3})                       # 320 // 3 = 106
    with pytest.raises(ValueError, match=rf"{family} head size 106 not in \(64,128\)"):
        cfg.validate_for_hip()
    cfg = _cfg(**{width: 448, heads: 3})                       # 448 // 3 = 149; and 192 / 3 passes
    with pytest.raises(ValueError, match=rf"{family} head size 149"):
        cfg.validate_for_hip()
    cfg = _cfg(**{width: 194, heads: 3})                       # 194 // 3 = 64, but 194 % 3 != 0: the head size alone is not the rule
    with pytest.raises(ValueError, match=rf"{family} head size 64 not in"):
        cfg.validate_for_hip()
    _cfg(**{width: 192, heads: 3}).validate_for_hip()


@pytest.mark.parametrize("name", SIZES)
def test_refuses_sizes_that_are_no_multiple_of_64(name):
    heads = {w: (h, f) for f, (w, h) in FAMILIES.items()}
    if name in heads:
        # A width of h heads of 64 or 128 IS a multiple of 64, so the head-size rule, checked first, is the one that refuses a
        # width that is not: 160 / 2 = 80, and 160 with one head is a head of 160.
        h, family = heads[name]
        for n_heads, d in ((2, 80), (1, 160)):
            with pytest.raises(ValueError, match=rf"{family} head size {d} not in"):
                _cfg(**{name: 160, h: n_heads}).validate_for_hip()
        return
    for bad in (32, 96, 200):
        with pytest.raises(ValueError, match=f"{name} must be a multiple of 64"):
            _cfg(**{name: bad}).validate_for_hip()


@pytest.mark.parametrize("name,heads", [("hidden_size", "num_attention_heads"), ("v_hidden_size", "v_num_attention_heads")])
def test_refuses_widths_above_1024(name, heads):
    with pytest.raises(ValueError, match="hidden sizes above 1024"):
        _cfg(**{name: 1088, heads: 17}).validate_for_hip()     # head size 64: only the width is wrong


def test_refuses_the_rest_one_rule_each():
    with pytest.raises(ValueError, match="type_vocab_size must be 2"):
        _cfg(type_vocab_size=3).validate_for_hip()
    for side in ("hidden_act", "v_hidden_act"):
        with pytest.raises(ValueError, match="only erf-GELU"):
            _cfg(**{side: "relu"}).validate_for_hip()
    with pytest.raises(ValueError, match="fusion_method must be 'mul' or 'sum'"):
        _cfg(fusion_method="cat").validate_for_hip()
    for flag in ("fast_mode", "in_batch_pairs"):
        with pytest.raises(ValueError, match="fast_mode / in_batch_pairs"):
            _cfg(**{flag: True}).validate_for_hip()
    _cfg(fusion_method="sum").validate_for_hip()


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("width,heads", [(64, 1), (1024, 8), (1024, 16)])
def test_accepts_each_width_at_its_limits(family, width, heads):
    w, h = FAMILIES[family]
    _cfg(**{w: width, h: heads}).validate_for_hip()


@pytest.mark.parametrize("name", ("intermediate_size", "v_intermediate_size", "v_feature_size"))
def test_accepts_the_other_sizes_at_64_and_1024(name):
    for size in (64, 1024):
        _cfg(**{name: size}).validate_for_hip()


# ---- the call forms with a narrower envelope: their refusals need no device ------------------------------------------------------
@pytest.mark.parametrize("case", EC.IDS)
def test_text_head_size_128_is_refused_on_the_host_by_the_forms_that_take_64(case):
    """tests/test_gpu_config_envelope.py holds the whole table; here the two refusals by head size on a model that was never
    moved to a device -- nothing can have been launched -- and the shared step's check accepting a head size of 64."""
    import numpy as np
    from unimm_amd import BertForMultiModalPreTraining
    from unimm_amd.inputs import DialogMaskSpec
    from unimm_amd.scoring import SharedContextPlan, check_shared_training
    c = EC.build(case)
    text_head = EC.HEAD_SIZES[case][0]
    model = BertForMultiModalPreTraining(c["cfg"])
    B, T, Rg = 4, EC.T, EC.REGIONS
    ids = torch.zeros((B, T), dtype=torch.int64)
    feat, loc = torch.zeros((B, Rg, c["cfg"].v_feature_size)), torch.zeros((B, Rg, 5))
    spec = DialogMaskSpec(np.ones(B), np.full(B, 20), np.full(B, 3))            # generative, context 17 + answer 3, copy 3
    groups = [0, 0, 1, 1]
    if text_head == 64:
        plan = check_shared_training(c["cfg"], "bf16", (1.0, 0.0, 0.0), spec, groups, T, Rg)
        assert isinstance(plan, SharedContextPlan) and plan.G == 2
        return
    with pytest.raises(ValueError, match=f"shared_context training: text head size {text_head}"):
        check_shared_training(c["cfg"], "bf16", (1.0, 0.0, 0.0), spec, groups, T, Rg)
    with pytest.raises(ValueError, match=f"text head size {text_head}"):
        model.forward_backward(ids, feat, loc, (1.0, 0.0, 0.0), attention_mask=spec, masked_lm_labels=torch.full((B, T), -1),
                               shared_context=groups)
    with pytest.raises(ValueError, match=f"generate_answers: text head size {text_head}"):
        model.generate_answers(ids, feat, loc, np.full(B, 17), beams=2, max_answer_len=4)
    assert not any(p.is_cuda for p in model.parameters())
