"""The config-envelope cases -- TEST INFRASTRUCTURE shared by tests/test_config_envelope_cpu.py and
tests/test_gpu_config_envelope.py.  No engine is called here.

`BertConfig.validate_for_hip()` admits any width that is a multiple of 64 up to 1024, head size 64 or 128 on each of the three
attention families independently, any head count and any connection schedule; the other model-level tests run 128 / 256 / 256
(small goldens) and 768 / 1024 / 1024 (full config), text heads of 64 and image / connection heads of 128 throughout.  The four
configurations below are tests/golden/small_config.json with these switches:

  id        hidden / heads   v_hidden / heads   bi_hidden / heads   intermediate / v_int   other                      t / v layers, t_bi, v_bi
  swapped   256 / 2 (D 128)  192 / 3  (D 64)    320 / 5 (D 64)      320 / 192              v_feature 64, v_target 37  3 / 3, [1,2], [0,2]
  narrow     64 / 1 (D 64)   128 / 1  (D 128)    64 / 1 (D 64)       64 /  64              v_feature 64               2 / 1, [1],   [0]
  wide     1024 / 8 (D 128) 1024 / 16 (D 64)    768 / 6 (D 128)     128 /  64                                         2 / 1, [1],   [0]
  odd       192 / 3 (D 64)   640 / 5  (D 128)   448 / 7 (D 64)      576 / 832              v_feature 320              2 / 2, [0,1], [0,1]

Between them: each head size on each family; Hb below (narrow: 64 = H < Hv; wide: 768 < both), between (odd: 192 < 448 < 640) and
above (swapped: 320 > 256 > 192) the other two widths; Hv < H (swapped); equal text and image widths at the limit (wide);
1, 3, 5 and 7 heads; widths that are odd multiples of 64; v_intermediate > intermediate (odd); an image layer between two
connections (swapped: v_biattention_id [0, 2]); a connection before any text layer (odd: t_biattention_id starts at 0).

Batch: unimm_amd.synth.make_batch(n_seq=6, T=80, R=37, seed=3, sequences_per_image=3), weights init_state_dict(seed=11), dropout
seed 77 from step 4 as tests/test_gpu_train_grads.py (the masks are those of step 5).  T = 80 on purpose: with T <= 64 every
text launch would take the few-keys or few-queries kernels; at 80 tokens against 37 regions the three attention families
dispatch as in production (long x long, few keys, few queries).

`build(id)` asserts what the case rests on (conditions, not measurements): the config passes `validate_for_hip()`, the batch has
real padding (valid rows < B T), and the dropout sites the replay saw are `grad_ref.site_names`."""
import json
import os

from oracle import vilbert_ref as R
from tests import grad_ref as GR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_SEQ, T, REGIONS, PER_IMAGE, BATCH_SEED, WEIGHT_SEED = 6, 80, 37, 3, 3, 11
SEED, STEP0 = 77, 4                      # as tests/test_gpu_train_grads.py: forward() bumps the step, the masks are those of step 5
STEP = STEP0 + 1
VALID_ROWS = 341                         # of N_SEQ * T = 480 (the batch does not depend on the configuration's widths)

SWITCHES = {
    "swapped": dict(hidden_size=256, num_attention_heads=2, v_hidden_size=192, v_num_attention_heads=3, bi_hidden_size=320,
                    bi_num_attention_heads=5, intermediate_size=320, v_intermediate_size=192, v_feature_size=64, v_target_size=37,
                    num_hidden_layers=3, v_num_hidden_layers=3, t_biattention_id=[1, 2], v_biattention_id=[0, 2]),
    "narrow": dict(hidden_size=64, num_attention_heads=1, v_hidden_size=128, v_num_attention_heads=1, bi_hidden_size=64,
                   bi_num_attention_heads=1, intermediate_size=64, v_intermediate_size=64, v_feature_size=64,
                   num_hidden_layers=2, v_num_hidden_layers=1, t_biattention_id=[1], v_biattention_id=[0]),
    "wide": dict(hidden_size=1024, num_attention_heads=8, v_hidden_size=1024, v_num_attention_heads=16, bi_hidden_size=768,
                 bi_num_attention_heads=6, intermediate_size=128, v_intermediate_size=64,
                 num_hidden_layers=2, v_num_hidden_layers=1, t_biattention_id=[1], v_biattention_id=[0]),
    "odd": dict(hidden_size=192, num_attention_heads=3, v_hidden_size=640, v_num_attention_heads=5, bi_hidden_size=448,
                bi_num_attention_heads=7, intermediate_size=576, v_intermediate_size=832, v_feature_size=320,
                num_hidden_layers=2, v_num_hidden_layers=2, t_biattention_id=[0, 1], v_biattention_id=[0, 1]),
}
IDS = tuple(SWITCHES)
#                 text, image, connection head size
HEAD_SIZES = {"swapped": (128, 64, 64), "narrow": (64, 128, 64), "wide": (128, 64, 128), "odd": (64, 128, 64)}
# live / dead parameter tensors of the oracle's gradients (grad_ref.compare's DEAD rule), as found
LIVE_DEAD = {"swapped": (178, 11), "narrow": (103, 6), "wide": (103, 6), "odd": (148, 9)}


def config_dict(case):
    with open(os.path.join(GOLDEN, "small_config.json")) as f:
        return dict(json.load(f), **SWITCHES[case])


def kwargs_of(b):
    """A synth.make_batch dict -> (args, kw) of the model's and the oracle's forward."""
    kw = dict(token_type_ids=b["token_type_ids"], position_ids=b["token_position_ids"], attention_mask=b["attention_mask"],
              image_attention_mask=b["image_attention_mask"], co_attention_mask=b["co_attention_mask"],
              masked_lm_labels=b["masked_lm_labels"], image_label=b["image_label"], image_target=b["image_target"],
              next_sentence_label=b["next_sentence_label"], nsp_weight=b["nsp_weight"], lm_weight=b["lm_weight"])
    return (b["input_ids"], b["image_feat"], b["image_loc"]), kw


_CASES = {}


def oracle_run(c, mutate=None, packed=True):
    """One float64 oracle run of the case with the replayed masks of STEP -> dict(losses, nsp, grads, sites)."""
    fn = GR.replay_drop_fn(SEED, STEP, c["rows"] if packed else None, mutate)
    losses, nsp, grads = GR.oracle_grads(c["sd"], c["ocfg"], c["args"], c["kw"], fn)
    return dict(losses=losses, nsp=nsp, grads=grads, sites=sorted(fn.sites))


def build(case):
    """The case, built once per process -> dict(id, cfgd, cfg, ocfg, sd, args, kw, rows, Mv, base); `base` is the unmutated
    float64 oracle run of the training step (`oracle_run`)."""
    if case in _CASES:
        return _CASES[case]
    from unimm_amd import BertConfig, synth
    cfgd = config_dict(case)
    cfg = BertConfig.from_dict(cfgd)
    cfg.validate_for_hip()
    ocfg = R.make_config(cfgd)
    dt, dv, db = HEAD_SIZES[case]
    assert (cfg.hidden_size // cfg.num_attention_heads, cfg.v_hidden_size // cfg.v_num_attention_heads,
            cfg.bi_hidden_size // cfg.bi_num_attention_heads) == (dt, dv, db)
    b = synth.make_batch(n_seq=N_SEQ, T=T, R=REGIONS, cfg=cfg, seed=BATCH_SEED, sequences_per_image=PER_IMAGE)
    args, kw = kwargs_of(b)
    rows = GR.packed_rows(kw["attention_mask"], kw["co_attention_mask"], kw["masked_lm_labels"], kw["lm_weight"])
    Mv = int(rows.numel())
    assert 0 < Mv < N_SEQ * T, (Mv, N_SEQ * T)                           # real padding: packed != padded coordinates
    assert Mv == VALID_ROWS, Mv
    assert T > 64 and REGIONS <= 64                                      # long x long, few keys, few queries
    c = dict(id=case, cfgd=cfgd, cfg=cfg, ocfg=ocfg, sd=R.init_state_dict(ocfg, seed=WEIGHT_SEED), args=args, kw=kw, rows=rows, Mv=Mv)
    c["base"] = oracle_run(c)
    assert c["base"]["sites"] == GR.site_names(ocfg), (c["base"]["sites"], GR.site_names(ocfg))
    _CASES[case] = c
    return c


def control_sites(ocfg):
    """The two sites of the GPU test's negative control: one text row-wise site (packed row coordinates) and one image or
    connection site -- the last text layer's output dropout and the last connection layer's image-side output dropout."""
    a = f"bert.encoder.layer.{ocfg.num_hidden_layers - 1}.out"
    b = f"bert.encoder.c_layer.{len(ocfg.v_biattention_id) - 1}.vout"
    assert GR.is_text_rowwise(a) and not GR.is_text_rowwise(b)
    return a, b
