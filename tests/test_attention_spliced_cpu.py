"""Host side of the spliced attention's training pair and of the shared-context training step: the group lists, the argument
marshalling of `lib.attn_spliced_bwd`, and what `forward_backward(shared_context=...)` refuses before touching a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "small_config.json")


def test_group_lists():
    from unimm_amd import lib
    first, seq = lib.group_lists([2, 0, 2, 1, 0, 2])
    assert first.dtype == np.int32 and seq.dtype == np.int32
    assert first.tolist() == [0, 2, 3, 6] and seq.tolist() == [1, 4, 3, 0, 2, 5]          # members in batch order, not adjacent
    first, seq = lib.group_lists([1, 1], G=3)                                           # groups without a member
    assert first.tolist() == [0, 0, 2, 2] and seq.tolist() == [0, 1]
    for bad in ([], [-1, 0], [0, 3]):
        with pytest.raises(ValueError):
            lib.group_lists(bad, G=3)


def test_spliced_bwd_struct_begins_with_the_bwd_struct():
    """`_attn_common` fills both through the same field names (the struct against the header: tests/test_abi.py)"""
    from unimm_amd import lib
    assert [f[0] for f in lib.AttnSplicedBwdArgs._fields_][:len(lib.AttnBwdArgs._fields_)] == [f[0] for f in lib.AttnBwdArgs._fields_]


def test_spliced_bwd_marshalling():
    from unimm_amd import lib
    HD = 128
    qkv = torch.zeros((50, 3 * HD), dtype=torch.bfloat16)
    g = torch.zeros((50, 3 * HD + 8), dtype=torch.bfloat16)
    out, dout = torch.zeros((50, HD), dtype=torch.bfloat16), torch.zeros((50, HD + 16), dtype=torch.bfloat16)
    lse = torch.zeros((3, 2, 32))
    words = torch.zeros((3, 32, 8), dtype=torch.int32)
    i32 = lambda *x: torch.tensor(x, dtype=torch.int32)
    qv, kv, ks = (i32(0, 10, 20), i32(3, 4, 5)), (i32(0, 10, 20), i32(3, 4, 5)), (i32(30, 30, 40), i32(7, 7, 9), 1)
    first, seq = lib.group_lists([0, 0, 1])
    gr = (torch.from_numpy(first), torch.from_numpy(seq))
    a = lib.spliced_bwd_args(qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:], out, dout[:, 16:], lse, g[:, :HD], g[:, HD:2 * HD],
                             g[:, 2 * HD:3 * HD], words, 3, 2, 32, 256, 64, 0.125, 8, 256, (5, 1 << 30, 4.0 / 3.0), qv, kv, ks, gr,
                             accumulate=True)
    assert (a.B, a.H, a.Tq, a.Tk, a.D, a.G, a.ks_ins, a.accumulate) == (3, 2, 32, 256, 64, 2, 1, 1)
    assert (a.ldq, a.ldk, a.ldv, a.ldo, a.lddo, a.lddq, a.lddk, a.lddv) == (384, 384, 384, 128, 144, 392, 392, 392)
    assert a.k == qkv.data_ptr() + 2 * HD and a.dv == g.data_ptr() + 4 * HD and a.dout == dout.data_ptr() + 32
    assert (a.q_off, a.k_len, a.ks_off, a.ks_len) == (qv[0].data_ptr(), kv[1].data_ptr(), ks[0].data_ptr(), ks[1].data_ptr())
    assert (a.g_first, a.g_seq) == (gr[0].data_ptr(), gr[1].data_ptr())
    assert (a.drop_key, a.drop_thr, a.mask_q_stride, a.mask_b_stride) == (5, 1 << 30, 8, 256)
    assert a.order is None and a.delta is None and abs(a.scale - 0.125) < 1e-9
    assert C.sizeof(lib.AttnSplicedBwdArgs) > C.sizeof(lib.AttnBwdArgs)


def _model(compute="bf16", **cfg_over):
    from unimm_amd import BertConfig, BertForMultiModalPreTraining
    cfgd = json.load(open(CFG))
    cfgd.update(cfg_over)
    return BertForMultiModalPreTraining(BertConfig.from_dict(cfgd), compute_dtype=compute)


def _inputs(K=4, T=64, R=37, c=10, n=3):
    from unimm_amd.inputs import DialogMaskSpec
    ids = torch.zeros((K, T), dtype=torch.int64)
    labels = torch.full((K, T), -1, dtype=torch.int64)
    spec = DialogMaskSpec(np.ones(K), np.full(K, c + n), np.full(K, n))
    return (ids, torch.zeros((2, R, 192)), torch.zeros((2, R, 5))), dict(attention_mask=spec, masked_lm_labels=labels)


def test_forward_backward_shared_context_refusals_need_no_device():
    from unimm_amd.inputs import DialogMaskSpec
    args, kw = _inputs()
    grp = torch.tensor([0, 0, 1, 1])
    m = _model()

    def refused(match, model=m, weights=(1.0, 0.0, 0.0), groups=grp, **over):
        with pytest.raises(ValueError, match=match):
            model.forward_backward(*args, weights, shared_context=groups, **{**kw, **over})

    refused(r"\(c, 0, 0\)", weights=(1.0, 0.5, 0.0))
    refused(r"\(c, 0, 0\)", weights=(1.0, 0.0, 2.0))
    refused("generative-mode DialogMaskSpec", attention_mask=torch.ones((4, 64, 64)))
    refused("generative-mode DialogMaskSpec", attention_mask=None)
    refused("generative-mode DialogMaskSpec", attention_mask=DialogMaskSpec(np.array([1, 1, 0, 1]), np.full(4, 13), np.full(4, 3)))
    refused("one group id", groups=torch.tensor([0, 0, 1]))
    refused("32-row query tile", attention_mask=DialogMaskSpec(np.ones(4), np.full(4, 30), np.full(4, 17)))
    refused("length > T", attention_mask=DialogMaskSpec(np.ones(4), np.full(4, 60), np.full(4, 8)))
    spec = DialogMaskSpec(np.ones(4), np.array([13, 14, 13, 13]), np.full(4, 3))      # the second member's context is one longer
    refused("context length", attention_mask=spec)
    refused("bf16 engine only", model=_model("fp32x3"))
    refused("with_coattention", model=_model(with_coattention=False))
    refused("no frozen layers", model=_model(fixed_t_layer=1))
    refused("no frozen layers", model=_model(fixed_v_layer=1))
    refused("masked_lm_labels", masked_lm_labels=None)


def test_graph_executor_declines_the_shared_step():
    from unimm_amd.graphs import StepGraphs
    eng = type("E", (), dict(text_priority=False, cfg=type("Cfg", (), dict(predict_feature=False))()))()
    sg = StepGraphs.__new__(StepGraphs)
    sg.eng = eng
    assert sg.eligible(dict(shared_context=[0, 0]), dict(want_seq=False)) is False
