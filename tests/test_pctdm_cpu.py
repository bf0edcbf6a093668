"""CPU: the PCTDM baseline's fixtures (tests/golden/pctdm_*.npz, tools/gen_golden_pctdm.py), state_dict names, registry, the drop-in
re-exports and the eight C-ABI symbols.

The module fixtures are checked against a float64 restatement of the block written from its definition (tests/pctdm_reference.py): a
bidirectional LSTM over the N players with gate order i, f, g, o, the reverse direction's outputs stored at the positions they belong to;
the max over the two direction halves of every player; the mean over the players; softmax of w_e . tanh(source + context) + b_e inside
each team of N / 2 players; x + x * gamma; one LSTM over each team, its last position; the two teams side by side.

Bar.  The restatement and the stored fp64 run are both fp64 and differ only in operation order (1e-16 per operation, a few thousand operations
per output: 1e-12 at most).  The fixture records how far the reference's own fp32 run is from its fp64 run (`yard_*`, about 1e-6);
BAR = yard * MARGIN with MARGIN = 1e-3 sits three decades under anything fp32 could produce and three above fp64 rounding.  Every wrong
variant must miss that bar by at least 10x AND miss the GPU test's fixture bar (max(5 * yard, 1e-4), tests/test_gpu_pctdm.py) by at least
10x: a bar that cannot tell them apart is not a bar."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import pctdm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
MARGIN = 1e-3
MODULE_CASES = ["pctdm_module_g3_n4", "pctdm_module_g2_n12"]
MODEL_CASES = ["pctdm_vgg16_96x160", "pctdm_vgg16_96x160_eval_n12"]
STAGES = ("lstm_out", "pooled", "gamma", "out")
_CACHE = {}


def _load(name):
    """(fixture, float64 parameters, float64 input): built once per case and left unchanged"""
    if name not in _CACHE:
        from gen_golden_pctdm import module_input, module_shapes, pctdm_params
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        B, T, N = (int(v) for v in z["meta"][:3])
        p = {k: v.double() for k, v in pctdm_params(module_shapes(), int(z["seed"]), float(z["extra_scale"])).items()}
        _CACHE[name] = (z, p, module_input(B, T, N, int(z["seed"])).double())
    return _CACHE[name]


def stage_err(z, name, got):
    """max |got - fixture fp64| / max |fixture fp64| over what the fixture stores of the stage"""
    got = torch.as_tensor(got).double().flatten()
    if "idx." + name in z.files:
        got, scale = got[torch.as_tensor(z["idx." + name])], float(z["max64_" + name])
    else:
        scale = float(np.abs(z[name + "64"]).max())
    return float((got - torch.as_tensor(z[name + "64"]).flatten()).abs().max()) / scale


def test_pctdm_fixtures_are_the_four_cases_of_the_table():
    import glob
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "pctdm_*.npz")))
    assert names == sorted(MODULE_CASES + MODEL_CASES)
    for n in names:
        assert os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < (1 << 20), n
    want = {"pctdm_module_g3_n4": (1, 3, 4, "module", "train"), "pctdm_module_g2_n12": (1, 2, 12, "module", "train"),
            "pctdm_vgg16_96x160": (2, 2, 4, "model", "train"), "pctdm_vgg16_96x160_eval_n12": (1, 3, 12, "model", "eval")}
    for n, (B, T, N, scope, mode) in want.items():
        z = np.load(os.path.join(GOLDEN, n + ".npz"))
        assert tuple(int(v) for v in z["meta"][:3]) == (B, T, N) and int(z["meta"][8]) == 1024, n
        assert str(z["scope"]) == scope and str(z["mode"]) == mode, n


@pytest.mark.parametrize("name", MODULE_CASES + MODEL_CASES)
def test_fixture_conditions_hold(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    B, T, N = (int(v) for v in z["meta"][:3])
    G = B * T
    if str(z["scope"]) == "model":
        assert float(z["loss64"]) >= 1e-2 and float(z["yard_activities"]) < 1e-5
    assert float(z["min_gap"]) >= 20.0 * float(z["lstm_err"]) > 0.0
    rowmax = float(torch.as_tensor(z["gamma64"]).reshape(G, 2, N // 2).max(-1).values.mean())
    assert abs(rowmax - float(z["rowmax_mean"])) < 1e-12 and 1.5 / (N // 2) <= rowmax <= 0.9
    assert 0.2 < float(z["gate_mean"]) < 0.8
    # the stored winners are those of the stored fp32 Bi-LSTM output, and the stored fp32 pooled features are its direction maximum
    lo = torch.as_tensor(z["lstm_out"]).reshape(G, N, 2, 1000)
    winner = torch.as_tensor(np.unpackbits(z["winner"])[:G * N * 1000].reshape(G, N, 1000)).bool()
    assert torch.equal(lo[:, :, 1] > lo[:, :, 0], winner)
    assert torch.equal(torch.as_tensor(z["pooled"]).reshape(G, N, 1000), torch.maximum(lo[:, :, 0], lo[:, :, 1]))
    assert 0.3 < float(winner.float().mean()) < 0.7
    for k in STAGES:
        assert 0.0 < float(z["yard_" + k]) < 1e-4, k
    assert not any(k.startswith(("g.fc_actions", "gsum.fc_actions", "g.pctdm.fc_actions")) for k in z.files)
    assert sum(k.startswith("g64.") for k in z.files) == (18 if str(z["scope"]) == "module" else 26)


@pytest.mark.parametrize("name", MODULE_CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    z, p, x = _load(name)
    r = R.module(p, x)
    for k in STAGES:
        e, bar = stage_err(z, k, r[k]), float(z["yard_" + k]) * MARGIN
        print(f"restatement {k}: {e:.2e} (bar {bar:.2e})")
        assert e <= bar, k
    G, N = r["gamma"].shape
    assert torch.equal(r["winner"], torch.as_tensor(np.unpackbits(z["winner"])[:G * N * 1000].reshape(G, N, 1000)).bool())


def test_float64_restatement_gradients_reproduce_the_fixture():
    from gen_golden_pctdm import module_cot
    name = MODULE_CASES[0]
    z, p, x = _load(name)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xs = x.clone().requires_grad_(True)
    out = R.module(leaves, xs)["out"]
    (out * module_cot(out.shape[0], int(z["seed"])).double()).sum().backward()
    e = float((xs.grad.flatten()[torch.as_tensor(z["idx.gx"])] - torch.as_tensor(z["gx64"])).abs().max()) / float(z["max64_gx"])
    assert e <= float(z["yard_gx"]) * MARGIN, e
    for k, v in leaves.items():
        got = v.grad.flatten()
        if "gidx." + k in z.files:
            got = got[torch.as_tensor(z["gidx." + k])]
        e = float((got - torch.as_tensor(z["g64." + k])).abs().max()) / float(z["gmax64." + k])
        print(f"restatement gradient {k}: {e:.2e} (yard {float(z['yard.' + k]):.2e})")
        if k == "att_extra_weights.0.bias":                              # zero in exact arithmetic: both sides hold rounding noise only
            assert float(v.grad.abs().max()) <= 1e-9 * float(leaves["att_extra_weights.0.weight"].grad.abs().max())
            continue
        assert e <= float(z["yard." + k]) * MARGIN, k


WRONG = [("gate_order_igfo", "pctdm_module_g3_n4", "lstm_out"), ("reverse_not_realigned", "pctdm_module_g3_n4", "lstm_out"),
         ("max_over_adjacent_players", "pctdm_module_g2_n12", "pooled"), ("softmax_over_all_players", "pctdm_module_g2_n12", "gamma"),
         ("no_residual", "pctdm_module_g3_n4", "out"), ("last_step_from_first_position", "pctdm_module_g2_n12", "out")]


@pytest.mark.parametrize("variant,case,first", WRONG, ids=[v for v, _, _ in WRONG])
def test_wrong_variants_miss_the_bar_by_ten(variant, case, first):
    z, p, x = _load(case)
    r = R.module(p, x, variant)
    for k in STAGES[STAGES.index(first):]:                               # the stage the variant changes first, and everything after it
        miss, yard = stage_err(z, k, r[k]), float(z["yard_" + k])
        print(f"{variant} {k}: misses by {miss:.2e}")
        assert miss >= 10 * yard * MARGIN, k
        assert miss >= 10 * max(5.0 * yard, 1e-4), f"the GPU test's bar on {k} could not tell this variant from the definition"


def _cfg(nfb=1024, n=12, t=10):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.inference_module_name, cfg.emb_features = "vgg16", "pctdm_volleyball", 512
    cfg.image_size, cfg.out_size = (96, 160), (3, 5)
    cfg.num_features_boxes, cfg.num_boxes, cfg.num_frames = nfb, n, t
    return cfg


@pytest.fixture(scope="module")
def built():
    from din_amd.train_net_dynamic import build_model
    z = np.load(os.path.join(GOLDEN, "pctdm_vgg16_96x160.npz"))
    B, T, N = (int(v) for v in z["meta"][:3])
    cfg = _cfg(1024, N, T)
    cfg.num_activities = int(z["meta"][9])
    return z, build_model(cfg)


def test_state_dict_matches_the_reference_key_list(built):
    from din_amd.infer_model import PCTDM_volleyball
    z, model = built
    assert type(model) is PCTDM_volleyball
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in z["key_shapes"]]
    keys = list(sd.keys())
    assert keys.index("nl_emb_1.bias") < keys.index("pctdm.Bi_Lstm.weight_ih_l0") < keys.index("pctdm_nl.weight") \
        < keys.index("fc_activities.weight") < keys.index("fc_actions.weight")
    assert sum(k.startswith("pctdm.") for k in sd) == 18
    for k in ("pctdm.Bi_Lstm.bias_hh_l0_reverse", "pctdm.att_source_weights.0.weight", "pctdm.att_context_weights.0.bias",
              "pctdm.att_extra_weights.0.weight", "pctdm.Intra_Group_LSTM.weight_hh_l0"):
        assert k in sd, k
    zm = np.load(os.path.join(GOLDEN, MODULE_CASES[0] + ".npz"))
    assert ["pctdm." + str(k) for k in zm["keys"]] == [k for k in keys if k.startswith("pctdm.")]
    named = dict(model.named_parameters())
    assert not named["fc_actions.weight"].requires_grad and not named["fc_actions.bias"].requires_grad
    assert all(v.requires_grad for k, v in named.items() if k.startswith(("pctdm.", "pctdm_nl.", "fc_activities.", "fc_emb_1.", "nl_emb_1.")))
    assert float(named["fc_actions.weight"].abs().max()) > 0 and float(named["fc_actions.bias"].abs().max()) == 0   # kaiming / zeros
    assert float(named["pctdm.att_source_weights.0.bias"].abs().max()) == 0          # the model's init loop reaches the block's Linear layers
    assert (model.pctdm.input_size, model.pctdm.hidden_size, model.pctdm.num_groups) == (1024, 1000, 2)
    assert tuple(model.pctdm_nl.normalized_shape) == (int(z["meta"][1]), 2000)


def test_registry_refusals_and_dropin():
    from din_amd.infer_model import PCTDM_volleyball
    from din_amd.infer_module.pctdm_infer_module import PCTDM
    from din_amd.train_net_dynamic import build_model
    with pytest.raises(NotImplementedError, match="MI355X hot path"):
        build_model(_cfg(16))
    with pytest.raises(NotImplementedError, match="num_features_boxes = 64"):
        PCTDM_volleyball(_cfg(64))
    for other in ("higcin_volleyball", "sacrf_biute_volleyball"):
        cfg = _cfg()
        cfg.inference_module_name = other
        with pytest.raises(NotImplementedError, match="MI355X hot path"):
            build_model(cfg)
    for n in (2, 5):
        with pytest.raises(ValueError, match="two teams"):
            PCTDM(_cfg(n=n))
    assert PCTDM(_cfg(n=4)).num_players == 4
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dropin_pctdm", os.path.join(ROOT, "dropin", "infer_module", "pctdm_infer_module.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.PCTDM is PCTDM
    spec = importlib.util.spec_from_file_location("_dropin_im2", os.path.join(ROOT, "dropin", "infer_model.py"))
    im = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(im)
    assert im.PCTDM_volleyball is PCTDM_volleyball


def test_forward_refuses_another_player_count_or_width():
    from din_amd.infer_module.pctdm_infer_module import PCTDM
    m = PCTDM(_cfg(n=4))
    with pytest.raises(ValueError, match="PCTDM takes"):
        m(torch.zeros((1, 1, 6, 1024)))
    with pytest.raises(ValueError, match="PCTDM takes"):
        m(torch.zeros((1, 1, 4, 1000)))


def test_header_binding_and_makefile_agree_on_the_eight_symbols():
    from din_amd import _lib
    syms = _lib.header_symbols()
    counts = (("din_lstm_fwd", 10), ("din_lstm_bwd_workspace", 3), ("din_lstm_bwd", 13), ("din_pctdm_pool_fwd", 8), ("din_pctdm_pool_bwd", 8),
              ("din_pctdm_att_fwd", 11), ("din_pctdm_att_bwd_workspace", 2), ("din_pctdm_att_bwd", 17))
    text = open(_lib.HEADER_PATH).read()
    for cite in ("pctdm_infer_module.py:23-24", "pctdm_infer_module.py:94-96", "pctdm_infer_module.py:52-59"):
        assert text.count(cite) >= 1, cite
    for name, nargs in counts:
        assert name in syms and name in _lib.SIGNATURES
        decl = text[text.index(("int64_t " if name.endswith("_workspace") else "int ") + name + "("):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1]), name
    assert sorted(syms) == sorted(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 9 and "#define DIN_ABI_VERSION 9" in text
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, name) for name, _ in counts)
    mk = open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    for f in ("lstm.hip", "pctdm_attention.hip"):
        assert f in mk
        src = open(os.path.join(_lib.CSRC_DIR, f)).read()
        assert "getenv" not in src and "atomic" not in src.replace("no atomics", "")
        for fast in ("__expf", "__tanhf", "__fdividef", "__frcp_rn", "cooperative_groups", "hipLaunchCooperativeKernel"):
            assert fast not in src, (f, fast)
