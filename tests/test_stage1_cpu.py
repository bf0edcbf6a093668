"""CPU: stage-1 (Basenet) fixtures, checkpoint layout, state_dict names, and the trainer's refusal of the ARG / GCN stage 2."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import din_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAGE1_CASES = sorted(glob.glob(os.path.join(GOLDEN, "stage1_*.npz")))


def _cfg(dataset, backbone="vgg16", D=512, NFB=64):
    from din_amd.config import Config
    cfg = Config(dataset)
    cfg.backbone, cfg.emb_features, cfg.num_features_boxes = backbone, D, NFB
    return cfg


def test_stage1_fixtures_are_present_and_self_consistent():
    names = {os.path.basename(p)[:-4] for p in STAGE1_CASES}
    assert {"stage1_vgg16_96x160_t1", "stage1_vgg16_96x160_t3", "stage1_inv3_139x203", "stage1_collective_inv3_139x203"} <= names
    for path in STAGE1_CASES:
        z = np.load(path)
        B, T, N, H, W, OH, OW, D, NFB, A_act, A_grp = (int(v) for v in z["meta"])
        collective = str(z["dataset"]) == "collective"
        rows = int(z["counts"].sum()) if collective else B * N
        assert z["actions"].shape == (rows, A_act) and z["activities"].shape == ((B * T if collective else B), A_grp), path
        if collective:
            c = z["counts"]
            assert c.shape == (B, T) and c.min() == 1 and c.max() == N and len({tuple(r) for r in c}) == B    # ragged inside clips
        # the fp32-vs-fp64 gap of the reference itself is recorded and small (the yardstick of the GPU tests)
        assert 0.0 < float(z["yard_actions"]) < 1e-5 and 0.0 < float(z["yard_activities"]) < 1e-5, path
        assert abs(float(z["loss"]) - float(z["loss64"])) <= 1e-5 * abs(float(z["loss64"]))
        assert abs(float(z["loss"]) - float(z["activities_loss"]) - float(z["actions_loss"])) <= 1e-5 * float(z["loss"])
        ys = [k for k in z.files if k.startswith("yard.")]
        assert len(ys) >= 5 and all(float(z[k]) < 1e-5 for k in ys), path
        for k in z.files:
            if k.startswith("gsum.") and not k.startswith("gsum64."):
                name = k[5:]
                # (backbone: single ReLU / max-pool routing flips between the fp32 and fp64 runs move a stem BatchNorm sum by ~2e-4 of
                #  sum |g|, measured; the model_* fixtures' 6e-3 bar)
                tol = 6e-3 if name.startswith("backbone.") else 1e-5
                assert abs(float(z[k]) - float(z["gsum64." + name])) <= tol * float(z["gabs." + name]) + 1e-7, (path, name)
        assert float(z["max_margin"]) > 1e-4, "a near-tie in the max over boxes would make the gradient route unstable"
        assert os.path.getsize(path) < 512 * 1024


def test_savemodel_and_loadmodel_use_the_reference_checkpoint_layout(tmp_path):
    from din_amd.base_model import Basenet_collective, Basenet_volleyball
    vb = Basenet_volleyball(_cfg("volleyball"))
    path = str(tmp_path / "stage1.pth")
    vb.savemodel(path)
    state = torch.load(path, map_location="cpu")
    assert set(state) == {"backbone_state_dict", "fc_emb_state_dict", "fc_actions_state_dict", "fc_activities_state_dict"}
    assert set(state["fc_emb_state_dict"]) == {"weight", "bias"}
    with torch.no_grad():
        for p in vb.parameters():
            p.add_(1.0)
    vb.loadmodel(path)                                               # volleyball restores all four
    for k in ("fc_actions", "fc_activities", "fc_emb"):
        assert torch.equal(getattr(vb, k).weight, state[k + "_state_dict"]["weight"])
    assert all(torch.equal(v, vb.backbone.state_dict()[k]) for k, v in state["backbone_state_dict"].items())
    # collective restores backbone + embedding only (reference base_model.py:188-192); its checkpoint names the embedding fc_emb too
    cfg = _cfg("collective", "inv3", 1056)
    co = Basenet_collective(cfg)
    cpath = str(tmp_path / "stage1_collective.pth")
    co.savemodel(cpath)
    cst = torch.load(cpath, map_location="cpu")
    assert set(cst) == set(state)
    with torch.no_grad():
        co.fc_emb_1.weight.add_(1.0)
        co.fc_actions.weight.add_(1.0)
    moved = co.fc_actions.weight.detach().clone()
    co.loadmodel(cpath)
    assert torch.equal(co.fc_emb_1.weight, cst["fc_emb_state_dict"]["weight"]) and torch.equal(co.fc_actions.weight, moved)


@pytest.mark.parametrize("dataset,backbone,D", [("volleyball", "vgg16", 512), ("volleyball", "inv3", 1056), ("collective", "inv3", 1056)])
def test_state_dict_built_from_reference_names_loads_strictly(dataset, backbone, D):
    from din_amd.base_model import Basenet_collective, Basenet_volleyball
    cls = Basenet_collective if dataset == "collective" else Basenet_volleyball
    model = cls(_cfg(dataset, backbone, D))
    fc_emb = "fc_emb_1" if dataset == "collective" else "fc_emb"
    K, NFB = 5, 64
    shapes = {k: v for k, v in O.model_param_shapes(O.OracleCfg(backbone=backbone, emb_features=D, num_features_boxes=NFB)).items()
              if k.startswith("backbone.")}
    shapes.update({fc_emb + ".weight": (NFB, K * K * D), fc_emb + ".bias": (NFB,), "fc_actions.weight": (9, NFB), "fc_actions.bias": (9,),
                   "fc_activities.weight": (8, NFB), "fc_activities.bias": (8,)})
    sd = O.synth_params(shapes, seed=1)
    sd.update({k: v for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")})   # BatchNorm buffers of the reference too
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.fc_actions.weight, sd["fc_actions.weight"])


def test_basenet_differences_between_the_two_classes():
    from din_amd.base_model import Basenet_collective, Basenet_volleyball
    from din_amd.backbone.backbone import MyInception_v3
    cfg = _cfg("volleyball")
    cfg.train_backbone = False                                       # volleyball never freezes (reference base_model.py:18-27)
    vb = Basenet_volleyball(cfg)
    assert all(p.requires_grad for p in vb.backbone.parameters())
    assert all(float(m.bias.detach().abs().sum()) == 0.0 for m in (vb.fc_emb, vb.fc_actions, vb.fc_activities))   # zero-init biases
    assert vb.dropout_emb.p == cfg.train_dropout_prob
    for frozen in (False, True):
        c = _cfg("collective", "vgg16", 1056)                        # collective always builds Inception-v3 (:158)
        c.train_backbone = not frozen
        co = Basenet_collective(c)
        assert isinstance(co.backbone, MyInception_v3)
        assert all(p.requires_grad != frozen for p in co.backbone.parameters())
    assert float(co.fc_actions.bias.detach().abs().sum()) > 0.0              # collective keeps nn.Linear's default bias init
    bad = _cfg("volleyball", "res18")
    with pytest.raises(NotImplementedError, match="the MI355X hot path covers 'vgg16' and 'inv3'"):
        Basenet_volleyball(bad)


def test_train_net_refuses_stage_two():
    from din_amd.train_net import train_net
    cfg = _cfg("volleyball")
    cfg.training_stage = 2
    with pytest.raises(NotImplementedError, match="gcn_model"):
        train_net(cfg)


def test_compact_actions_matches_the_reference_loop():
    from din_amd.train_net import compact_actions
    g = torch.Generator().manual_seed(3)
    actions = torch.randint(0, 6, (6, 5), generator=g)
    counts = torch.tensor([5, 1, 3, 2, 5, 4], dtype=torch.int32)
    ref = torch.cat([actions[bt, :int(counts[bt])] for bt in range(6)])    # reference train_net.py:284-290
    assert torch.equal(compact_actions(actions, counts, int(counts.sum())), ref)


def test_dropin_train_net_exposes_config_and_the_stage1_entry_points():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from train_net import *\ncfg = Config('volleyball')\nassert train_net.__module__ == 'din_amd.train_net'\n"
            "from base_model import Basenet_volleyball, Basenet_collective\nassert Basenet_volleyball.__module__ == 'din_amd.base_model'\n"
            "print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, PYTHONPATH=os.path.join(root, "dropin")),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
