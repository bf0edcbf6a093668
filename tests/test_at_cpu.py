"""CPU: the Actor-Transformer baseline's fixtures (tests/golden/at_*.npz, tools/gen_golden_at.py), state_dict names, registry, config, the
drop-in re-export and the four C-ABI symbols.

The fixtures are checked against a float64 restatement of the block written here from its definition: box centre ((x1 + x2) / 2,
(y1 + y2) / 2) scaled to image px, divided by the fp32 table 10000 ** (2 * (i // 2) / (NFB / 2)), sin on even and cos on odd indices, x half
then y half, added to the features; (mean over T with temporal_pooled_first;) per group softmax_rows(Q K^T / sqrt(NFB)) V; LayerNorm1 of
(x + that); FFN_linear1, ReLU, FFN_linear2; LayerNorm2 of (x + that).

Bar.  The restatement and the stored fp64 run are both fp64; they differ only in operation order (1e-16 per operation, a few thousand
operations per output, amplified by sin / cos of arguments up to 160 rad: 1e-12 at most).  The fixture records how far the reference's own
fp32 run is from its fp64 run (`yard_*`, about 2e-6); BAR = yard * MARGIN with MARGIN = 1e-3 sits three decades under anything fp32 could
produce and three above fp64 rounding.  Every wrong variant must miss that bar by at least 10x AND miss the GPU test's fixture bar
(max(5 * yard, 1e-4), tests/test_gpu_at.py) by at least 10x: a bar that cannot tell them apart is not a bar."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
AT_CASES = sorted(glob.glob(os.path.join(GOLDEN, "at_*.npz")))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MARGIN = 1e-3
NAMES = ["at_vgg16_96x160", "at_vgg16_96x160_pooled", "at_vgg16_96x160_eval_n12", "at_inv3_139x203"]


def _load(path):
    from gen_golden_at import at_params, at_shapes
    from oracle import din_oracle as O
    z = np.load(path)
    B, T, N, H, W, OH, OW, D, NFB, A = (int(v) for v in z["meta"])
    p = at_params(at_shapes(str(z["backbone"]), D, 5, NFB, A), int(z["seed"]))
    _, boxes, _ = O.synth_inputs(B, T, N, H, W, OH, OW, A, seed=int(z["seed"]))
    return z, {k[3:]: v.double() for k, v in p.items() if k.startswith("AT.")}, boxes.double(), dict(H=H, W=W, OH=OH, OW=OW, NFB=NFB)


def restated(z, p, boxes, g, variant=None):
    """float64 position embedding and Actor_Transformer on the stored trunk output -> (embedded features, attention, block output)"""
    x = torch.as_tensor(z["pe_in64"])                                    # [B, T, N, NFB]
    C = g["NFB"]
    cx, cy = (boxes[..., 0] + boxes[..., 2]) / 2, (boxes[..., 1] + boxes[..., 3]) / 2
    if variant != "feature_px":
        cx, cy = cx * g["W"] / g["OW"], cy * g["H"] / g["OH"]
    d = torch.arange(C // 2, dtype=torch.float32)
    dim_t = (10000 ** (2 * (d // 2) / (C // 2))).double()               # (formed in fp32, as the reference forms it)
    px, py = cx[..., None] / dim_t, cy[..., None] / dim_t
    even, odd = (torch.cos, torch.sin) if variant == "sin_cos_swapped" else (torch.sin, torch.cos)
    px = torch.stack((even(px[..., 0::2]), odd(px[..., 1::2])), dim=-1).flatten(-2)
    py = torch.stack((even(py[..., 0::2]), odd(py[..., 1::2])), dim=-1).flatten(-2)
    pe = x + (torch.cat((py, px), -1) if variant == "halves_swapped" else torch.cat((px, py), -1))
    h = pe.mean(1) if bool(z["pooled"]) else pe.reshape(-1, pe.shape[2], C)
    q, k, v = h @ p["Q_W.weight"].t(), h @ p["K_W.weight"].t(), h @ p["V_W.weight"].t()
    s = q @ k.transpose(1, 2)
    if variant != "no_sqrt":
        s = s / math.sqrt(C)
    att = torch.softmax(s, dim=1 if variant == "softmax_axis" else 2)
    ln = lambda t, n: F.layer_norm(t, (C,), p[n + ".weight"], p[n + ".bias"], 1e-5)                       # noqa: E731
    h = (h + ln(att @ v, "layernorm1")) if variant == "ln_before_residual" else ln(h + att @ v, "layernorm1")
    f = torch.relu(h @ p["FFN_linear1.weight"].t() + p["FFN_linear1.bias"]) @ p["FFN_linear2.weight"].t() + p["FFN_linear2.bias"]
    return pe, att, ln(h + f, "layernorm2")


def err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def test_at_fixtures_are_the_four_cases_of_the_table():
    assert [os.path.basename(p)[:-4] for p in AT_CASES] == sorted(NAMES)
    largest_arg = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "arg_*.npz")))
    for p in AT_CASES:
        assert os.path.getsize(p) <= largest_arg, p
    z = np.load(os.path.join(GOLDEN, "at_vgg16_96x160_eval_n12.npz"))
    assert tuple(int(v) for v in z["meta"][[2, 8]]) == (12, 128) and str(z["mode"]) == "eval"
    assert bool(np.load(os.path.join(GOLDEN, "at_vgg16_96x160_pooled.npz"))["pooled"])
    assert str(np.load(os.path.join(GOLDEN, "at_inv3_139x203.npz"))["backbone"]) == "inv3"


@pytest.mark.parametrize("path", AT_CASES, ids=[os.path.basename(p)[:-4] for p in AT_CASES])
def test_fixture_conditions_hold(path):
    z = np.load(path)
    N = int(z["meta"][2])
    assert float(z["loss64"]) >= 1e-2
    rowmax = float(torch.as_tensor(z["att64"]).max(-1).values.mean())
    assert abs(rowmax - float(z["rowmax_mean"])) < 1e-12 and 1.5 / N <= rowmax <= 0.9
    assert torch.equal(torch.as_tensor(z["at_out"]).argmax(1), torch.as_tensor(z["at_out64"]).argmax(1))
    assert float(z["yard_activities"]) < 1e-5
    assert not any(k.startswith(("g.fc_actions", "gsum.fc_actions")) for k in z.files)
    assert err(z["pe"], z["pe64"]) <= float(z["yard_pe"]) * (1 + 1e-9)
    assert err(z["att"], z["att64"]) <= float(z["yard_att"]) * (1 + 1e-9)
    assert err(z["at_out"], z["at_out64"]) <= float(z["yard_at_out"]) * (1 + 1e-9)


@pytest.mark.parametrize("path", AT_CASES, ids=[os.path.basename(p)[:-4] for p in AT_CASES])
def test_float64_restatement_reproduces_the_fixture(path):
    z, p, boxes, g = _load(path)
    pe, att, out = restated(z, p, boxes, g)
    for name, got in (("pe", pe), ("att", att), ("at_out", out)):
        e, bar = err(got, z[name + "64"]), float(z["yard_" + name]) * MARGIN
        print(f"restatement {name}: {e:.2e} (bar {bar:.2e})")
        assert e <= bar, name


WRONG = [("no_sqrt", "at_vgg16_96x160"), ("softmax_axis", "at_vgg16_96x160"), ("halves_swapped", "at_vgg16_96x160"),
         ("feature_px", "at_vgg16_96x160_eval_n12"), ("sin_cos_swapped", "at_inv3_139x203"), ("ln_before_residual", "at_vgg16_96x160_pooled")]


@pytest.mark.parametrize("variant,case", WRONG, ids=[v for v, _ in WRONG])
def test_wrong_variants_miss_the_bar_by_ten(variant, case):
    z, p, boxes, g = _load(os.path.join(GOLDEN, case + ".npz"))
    pe, att, out = restated(z, p, boxes, g, variant)
    # the stage the variant changes first, and everything after it
    first = {"no_sqrt": "att", "softmax_axis": "att", "ln_before_residual": "at_out"}.get(variant, "pe")
    stages = [("pe", pe), ("att", att), ("at_out", out)]
    stages = stages[[n for n, _ in stages].index(first):]
    for name, got in stages:
        miss, yard = err(got, z[name + "64"]), float(z["yard_" + name])
        print(f"{variant} {name}: misses by {miss:.2e}")
        assert miss >= 10 * yard * MARGIN, name
        assert miss >= 10 * max(5.0 * yard, 1e-4), f"the GPU test's bar on {name} could not tell this variant from the definition"


def _fixture_cfg(z):
    from din_amd.config import Config
    B, T, N, H, W, OH, OW, D, NFB, A = (int(v) for v in z["meta"])
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = str(z["backbone"]), (H, W), (OH, OW), D
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_activities = N, T, NFB, A
    cfg.temporal_pooled_first = bool(z["pooled"])
    return cfg


@pytest.mark.parametrize("name", ["at_vgg16_96x160", "at_inv3_139x203"])
def test_state_dict_matches_the_reference_key_list(name):
    from din_amd.infer_model import AT_volleyball
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = AT_volleyball(_fixture_cfg(z))
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in z["key_shapes"]]
    keys = list(sd.keys())
    assert keys.index("nl_emb_1.bias") < keys.index("AT.Q_W.weight") < keys.index("fc_activities.weight") < keys.index("fc_actions.weight")
    assert sum(k.startswith("AT.") for k in sd) == 11 and not any("dropout" in k or k.startswith("PE.") for k in sd)
    named = dict(model.named_parameters())
    assert not named["fc_actions.weight"].requires_grad and not named["fc_actions.bias"].requires_grad
    assert all(v.requires_grad for k, v in named.items() if k.startswith(("AT.", "fc_activities.", "fc_emb_1.", "nl_emb_1.")))
    assert float(named["fc_actions.weight"].abs().max()) > 0 and float(named["fc_actions.bias"].abs().max()) == 0   # kaiming / zeros
    assert (model.AT.dropout1.p, model.AT.dropout2.p, model.AT.FFN_dropout.p) == (0.1, 0.1, 0.1)


def test_module_constructors_take_the_reference_arguments():
    from din_amd.config import Config
    from din_amd.infer_module.AT_infer_module import Actor_Transformer, Embfeature_PositionEmbedding
    cfg = Config("volleyball")
    pe = Embfeature_PositionEmbedding(cfg, num_pos_feats=512, temperature=10000, normalize=False, scale=None)
    assert len(list(pe.parameters())) == 0 and pe.num_pos_feats == 512
    with pytest.raises(ValueError, match="normalize should be True"):
        Embfeature_PositionEmbedding(cfg, scale=1.0)
    d = torch.arange(512, dtype=torch.float32)
    assert torch.equal(pe.dim_t(torch.device("cpu")), 10000 ** (2 * (d // 2) / 512)) and pe.dim_t(torch.device("cpu")).dtype == torch.float32
    at = Actor_Transformer(64, True, dropout=0.2)
    assert at.temporal_pooled_first and at.dropout1.p == 0.2 and at.Q_W.bias is None and at.FFN_linear1.bias is not None
    with pytest.raises(ValueError, match="already averaged over T"):      # one pooling path: the position kernel's
        at(torch.zeros((1, 2, 3, 64)))
    assert Embfeature_PositionEmbedding(cfg, 32, pool_t=True).pool_t and not pe.pool_t


def test_registry_config_and_dropin():
    from din_amd.config import Config
    from din_amd.infer_model import AT_volleyball
    from din_amd.train_net_dynamic import build_model
    cfg = Config("volleyball")
    assert cfg.temporal_pooled_first is False
    cfg.backbone, cfg.inference_module_name, cfg.emb_features, cfg.num_features_boxes = "vgg16", "at_volleyball", 512, 16
    assert type(build_model(cfg)) is AT_volleyball
    cfg.backbone = "res18"
    with pytest.raises(NotImplementedError):
        build_model(cfg)
    cfg.backbone = "vgg16"
    for other in ("pctdm_volleyball", "higcin_volleyball", "sacrf_biute_volleyball"):
        cfg.inference_module_name = other
        with pytest.raises(NotImplementedError, match="MI355X hot path"):
            build_model(cfg)
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dropin_at", os.path.join(ROOT, "dropin", "infer_module", "AT_infer_module.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from din_amd.infer_module.AT_infer_module import Actor_Transformer, Embfeature_PositionEmbedding
    assert mod.Actor_Transformer is Actor_Transformer and mod.Embfeature_PositionEmbedding is Embfeature_PositionEmbedding
    assert not hasattr(mod, "PositionEmbeddingSine")
    spec = importlib.util.spec_from_file_location("_dropin_im", os.path.join(ROOT, "dropin", "infer_model.py"))
    im = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(im)
    assert im.AT_volleyball is AT_volleyball


def test_header_binding_and_makefile_agree_on_the_four_symbols():
    from din_amd import _lib
    syms = _lib.header_symbols()
    counts = (("din_actor_position_fwd", 14), ("din_actor_position_bwd", 8), ("din_actor_attn_fwd", 19), ("din_actor_attn_bwd", 25))
    text = open(_lib.HEADER_PATH).read()
    assert text.count("AT_infer_module.py:52-96") >= 1 and text.count("AT_infer_module.py:130-138") >= 1
    for name, nargs in counts:
        assert name in syms and name in _lib.SIGNATURES
        decl = text[text.index("int " + name + "("):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1]), name
    assert sorted(syms) == sorted(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 9 and "#define DIN_ABI_VERSION 9" in text
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, name) for name, _ in counts)
    assert "actor_attention.hip" in open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    src = open(os.path.join(_lib.CSRC_DIR, "actor_attention.hip")).read()
    assert "getenv" not in src and "atomic" not in src.replace("no atomics", "")
    for fast in ("__sinf", "__cosf", "__fdividef", "__expf", "__frcp_rn"):
        assert fast not in src, fast
