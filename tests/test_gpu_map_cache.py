"""The map cache (cfg.map_cache_gb) on the MI355X: the MapCache round trip behind infer_model._cached_crops (slabs of two slots, a mixed
batch, a frame twice, a full cache, an altered trailer, the gather replayed from a captured graph), Dynamic_TCE_volleyball,
Dynamic_collective, Dynamic_volleyball and ARG_volleyball's eval fold fed the same clips as an images tensor and as FrameRefs, two epochs
of train_net over tests/golden/dataset_tree with the setting against the same run without it, and the launches of a step with the setting
at 0.  VGG16; volleyball 96 x 160 -> (3, 5), collective 64 x 96 -> (2, 3) with 13 boxes; T = 3."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import Measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

T = 3


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _cfg(name, dataset="volleyball"):
    from din_amd.config import Config
    cfg = Config(dataset)
    cfg.backbone, cfg.emb_features = "vgg16", 512
    if dataset == "volleyball":
        cfg.image_size, cfg.out_size, cfg.num_boxes = (96, 160), (3, 5), 12
    else:
        cfg.image_size, cfg.out_size, cfg.num_boxes, cfg.num_activities = (64, 96), (2, 3), 13, 5
    cfg.num_frames, cfg.num_features_boxes, cfg.num_features_gcn = T, 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers, cfg.pos_threshold = 16, 4, 1, 0.5
    cfg.inference_module_name, cfg.training_stage, cfg.train_dropout_prob = name, 2, 0.0
    return cfg


def _map_cache(gpu, cfg, capacity=1 << 30, chunk_frames=2):
    from din_amd.feature_cache import MapCache, map_shape_and_itemsize
    return MapCache(gpu, *map_shape_and_itemsize(cfg), capacity, chunk_frames=chunk_frames)


def _clips(cfg, gpu, count, frames=T, seed=4):
    """(uint8 images [count, frames, 3, H, W], boxes [count, frames, N, 4]) on the device"""
    from din_amd.train_net_dynamic import SyntheticVolleyball
    dcfg = copy.copy(cfg)
    dcfg.num_frames = frames
    clips = [SyntheticVolleyball(dcfg, length=count, seed=seed)[i] for i in range(count)]
    return torch.stack([c[0] for c in clips]).to(gpu), torch.stack([c[1] for c in clips]).to(gpu)


def _count_trunk(monkeypatch, model):
    """wraps the model's forward_nhwc: the list gains the number of frames of every call"""
    calls, real = [], model.backbone.forward_nhwc

    def trunk(x, *a, **kw):
        calls.append(int(x.shape[0]))
        return real(x, *a, **kw)

    monkeypatch.setattr(model.backbone, "forward_nhwc", trunk)
    return calls, real


def _slot(cache, fid):
    slab, off = cache.table.locate(cache.table.slot_of[fid])
    return cache.slabs[slab][off:off + cache.table.stride]


# ---- 1. the cache behind _cached_crops ----------------------------------------------------------------------------------------------------
def test_map_cache_round_trip_in_slabs_of_two(gpu, monkeypatch):
    from din_amd import infer_model as IM, ops
    from din_amd.feature_cache import FrameRefs
    from din_amd.train_net_dynamic import build_model
    cfg = _cfg("dynamic_volleyball")
    torch.manual_seed(3)
    model = build_model(cfg).to(gpu).eval()
    calls, trunk = _count_trunk(monkeypatch, model)
    images, boxes = _clips(cfg, gpu, 5)                          # 15 frames: 0..5 the first batch, 6..8 the new ones of the mixed batch
    frames = images.reshape(15, 3, 96, 160)
    N, H, W = cfg.num_boxes, 96, 160
    maps_of = lambda x: trunk(x.contiguous())[0][0].clone()     # (a clone: the trunk's output buffer may be reused by its next call)
    with torch.no_grad():
        want6, want3 = maps_of(frames[:6]), maps_of(frames[6:9])
    assert tuple(want6.shape) == (6, 3, 5, 512) and want6.dtype == torch.float32
    cache = _map_cache(gpu, cfg)
    assert (cache.row_bytes, cache.box_bytes, cache.table.stride) == (30720, 16, 30736) and not cache.slabs and cache.map_dtype is None

    def crops(ids, miss, pos, bx):
        refs = FrameRefs(np.asarray(ids).reshape(2, T), miss, pos, cache)
        out = IM._cached_crops(model, refs, bx, N)
        return refs, refs.context[0], out

    ids = [100 + 7 * i for i in range(6)]                        # frame ids are names, not slot numbers
    bx = boxes[:2]
    refs, fm, out = crops(ids, frames[:6], range(6), bx)         # all missed
    assert calls == [6] and refs.inserted == ids and torch.equal(fm, want6) and cache.map_dtype == torch.float32
    assert cache.table.slab_slots == [2, 2, 2] and (cache.hits, cache.misses, cache.inserted) == (0, 6, 6)
    plain = model.roi_align(want6, bx.reshape(-1, 4), ops.boxes_frame_index(6, N, gpu), nhwc=True, channels=512, relu_masked=cache.relu_masked)
    assert tuple(out.shape) == (6 * N, 512, 5, 5) and torch.equal(out, plain) and not out.requires_grad
    refs, fm2, out2 = crops(ids, frames[:0], [], bx)             # all resident: no backbone call
    assert calls == [6] and refs.inserted == [] and torch.equal(fm2, want6) and torch.equal(out2, out) and cache.hits == 6
    # M = 3 of 6: rows 1, 3, 4 are new frames, the others come from their slots
    new = [900, 901, 902]
    mixed = [ids[0], new[0], ids[1], new[1], new[2], ids[2]]
    refs, fm3, _ = crops(mixed, frames[6:9], [1, 3, 4], bx)
    assert calls == [6, 3] and refs.inserted == new
    assert torch.equal(fm3[[0, 2, 5]], want6[:3]) and torch.equal(fm3[[1, 3, 4]], want3)
    assert cache.table.slab_slots == [2, 2, 2, 2, 2] and cache.inserted == 9 and len(cache.table.slot_of) == 9     # the fifth slab is half full
    for fid, want in ((ids[0], want6[0]), (ids[5], want6[5]), (new[2], want3[2])):     # a slot: the map's bytes, then (id, OH, OW, C)
        got = _slot(cache, fid).cpu().numpy()
        assert got[:30720].tobytes() == want.cpu().numpy().tobytes()
        assert got[30720:].view(np.float32).tolist() == [float(fid), 3.0, 5.0, 512.0]
    # a frame twice in one batch, both decoded: served both times from the first computed map
    twice = [950, 951, 950, ids[3], ids[4], ids[5]]
    refs, fm4, _ = crops(twice, frames[[9, 10, 11]], [0, 1, 2], bx)
    with torch.no_grad():
        want_t = maps_of(frames[[9, 10, 11]])
    assert calls == [6, 3, 3] and refs.inserted == [950, 951] and cache.inserted == 11
    assert torch.equal(fm4[0], want_t[0]) and torch.equal(fm4[2], want_t[0]) and torch.equal(fm4[1], want_t[1]) and torch.equal(fm4[3:], want6[3:])
    refs, fm5, _ = crops([950, 951] + ids[:4], frames[:0], [], bx)
    assert torch.equal(fm5[:2], want_t[:2]) and torch.equal(fm5[2:], want6[:4])
    cache.check()                                                # every served row met its own trailer
    with pytest.raises(KeyError):
        crops([5, 6, 7] + ids[:3], frames[:0], [], bx)


def test_a_full_map_cache_serves_computed_maps_without_keeping_them(gpu, monkeypatch):
    from din_amd import infer_model as IM
    from din_amd.feature_cache import FrameRefs
    from din_amd.train_net_dynamic import build_model
    cfg = _cfg("dynamic_volleyball")
    torch.manual_seed(3)
    model = build_model(cfg).to(gpu).eval()
    calls, trunk = _count_trunk(monkeypatch, model)
    images, boxes = _clips(cfg, gpu, 2)
    frames = images.reshape(6, 3, 96, 160)
    with torch.no_grad():
        want = trunk(frames)[0][0].clone()
        want2 = trunk(frames[4:].contiguous())[0][0].clone()
    cache = _map_cache(gpu, cfg, capacity=4 * 30736 + 100)       # four slots
    ids = np.arange(40, 46)
    refs = FrameRefs(ids.reshape(2, T), frames, np.arange(6), cache)
    IM._cached_crops(model, refs, boxes, cfg.num_boxes)
    assert refs.inserted == [40, 41, 42, 43] and cache.table.full and cache.table.slab_slots == [2, 2] and torch.equal(refs.context[0], want)
    refs = FrameRefs(ids.reshape(2, T), frames[4:], [4, 5], cache)           # the two that did not fit are decoded and computed again
    IM._cached_crops(model, refs, boxes, cfg.num_boxes)
    assert calls == [6, 2] and refs.inserted == [] and cache.inserted == 4
    assert torch.equal(refs.context[0][:4], want[:4]) and torch.equal(refs.context[0][4:], want2)
    cache.check()


def test_an_altered_trailer_ends_the_pass_in_check(gpu):
    cfg = _cfg("dynamic_volleyball")
    cache = _map_cache(gpu, cfg)
    g = torch.Generator().manual_seed(5)
    maps = torch.randn((5, 3, 5, 512), generator=g).to(gpu)
    ids = [11, 12, 13, 14, 15]
    fm, new = cache.maps(ids, range(5), maps, relu_masked=True)
    assert new == ids and torch.equal(fm, maps) and cache.relu_masked is True
    cache.check()                                                # inserts compare nothing
    _slot(cache, 13)[30720:30724].view(torch.float32).add_(1.0)  # the slot now says it holds frame 14
    _slot(cache, 15)[30728:30732].view(torch.float32).fill_(7.0)  # ... and this one a map 7 wide
    fm, _ = cache.maps([15, 11, 13, 12], [], None)
    assert torch.equal(fm, maps[[4, 0, 2, 1]])                   # the rows are served all the same; the pass ends with the error
    with pytest.raises(RuntimeError) as e:
        cache.check()
    assert "map cache" in str(e.value) and "2 rows" in str(e.value) and "(0, 15)" in str(e.value) and "(2, 13)" in str(e.value)
    cache.check()                                                # the flags were cleared
    with pytest.raises(ValueError):                              # other maps than the slots were sized for
        cache.maps([20], [0], maps[:1, :, :4].contiguous())
    with pytest.raises(ValueError):
        cache.maps([21], [0], maps[:1].bfloat16())


def test_the_map_gather_replays_from_a_captured_graph(gpu):
    """the launch behind MapCache.maps with map-sized rows and the 16-byte trailer: recorded into a graph and replayed, it writes the
    bytes the direct call wrote (served rows, a kept row with its trailer, the trailer comparison)"""
    from din_amd import ops
    cfg = _cfg("dynamic_volleyball")
    cache = _map_cache(gpu, cfg)
    g = torch.Generator().manual_seed(6)
    maps = torch.randn((4, 3, 5, 512), generator=g).to(gpu)
    cache.maps([1, 2, 3], range(3), maps[:3].contiguous())
    cache.check()
    rb = cache.row_bytes
    out = torch.zeros((4, rb // 4), device=gpu)
    spare = torch.zeros(rb + 16, dtype=torch.uint8, device=gpu)  # a "slot" for the computed row
    trailers = torch.from_numpy(cache.trailers([3, 1, 9, 2])).to(gpu)
    trailers[3, 0] = 5.0                                         # row 3 asks slot 2 for frame 5: flagged
    flags = torch.zeros(4, dtype=torch.uint8, device=gpu)
    tab = lambda v: torch.tensor(v, dtype=torch.int64, device=gpu)
    slots = [cache.slot_address(cache.table.slot_of[f]) for f in (3, 1, 2)]
    src = tab([slots[0], slots[1], maps[3].data_ptr(), slots[2]])
    dst = tab([out.data_ptr() + i * rb for i in range(4)])
    keep = tab([0, 0, spare.data_ptr(), 0])
    ref = tab([slots[0] + rb, slots[1] + rb, 0, slots[2] + rb])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.feat_rows(src, dst, rb, keep, ref, trailers, flags, 16)
    out.zero_(), spare.zero_(), flags.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(4, 3, 5, 512), maps[[2, 0, 3, 1]]) and flags.tolist() == [0, 0, 0, 1]
    assert torch.equal(spare[:rb].view(torch.float32), maps[3].reshape(-1)) and spare[rb:].view(torch.float32).tolist() == [9.0, 3.0, 5.0, 512.0]


# ---- 2.-4. through the models ----------------------------------------------------------------------------------------------------------
def _three_ways(gpu, monkeypatch, cfg, images, boxes, extra=()):
    """the same clips through a frozen model in eval(): as an images tensor, as FrameRefs with every frame missed, as FrameRefs with every
    frame resident.  Returns (model, cache, scores of the three calls); asserts the backbone calls."""
    from din_amd.feature_cache import FrameRefs
    from din_amd.train_net_dynamic import build_model
    torch.manual_seed(3)
    model = build_model(cfg).to(gpu).eval()
    assert not any(p.requires_grad for p in model.backbone.parameters())
    calls, _ = _count_trunk(monkeypatch, model)
    B, frames = images.shape[0], images.shape[1]
    H, W = cfg.image_size
    cache = _map_cache(gpu, cfg)
    ids = np.arange(1000, 1000 + B * frames).reshape(B, frames)
    with torch.no_grad():
        plain = model((images, boxes, *extra))["activities"]
        assert calls == [B * frames]
        first = FrameRefs(ids, images.reshape(B * frames, 3, H, W), np.arange(B * frames), cache)
        out1 = model((first, boxes, *extra))["activities"]
        assert calls == [B * frames] * 2 and first.inserted == ids.reshape(-1).tolist()
        second = FrameRefs(ids, images.reshape(B * frames, 3, H, W)[:0], [], cache)
        out2 = model((second, boxes, *extra))["activities"]
        assert calls == [B * frames] * 2, "the backbone ran for a batch whose frames are all resident"
    torch.cuda.synchronize()
    cache.check()
    assert (cache.hits, cache.misses, cache.inserted) == (B * frames, B * frames, B * frames) and second.inserted == []
    return model, cache, (plain, out1, out2)


def _backward_both_ways(gpu, model, cache_cfg, images, boxes, labels, extra=()):
    """training mode under ops.deterministic(): the gradients of a step fed an images tensor and of the same step fed all-missed refs,
    each on a fresh model with `model`'s weights (so the dropout counters agree)"""
    from din_amd import ops
    from din_amd.feature_cache import FrameRefs
    from din_amd.train_net_dynamic import build_model
    B, frames = images.shape[0], images.shape[1]
    H, W = cache_cfg.image_size
    refs = FrameRefs(np.arange(B * frames).reshape(B, frames), images.reshape(B * frames, 3, H, W), np.arange(B * frames), _map_cache(gpu, cache_cfg))
    grads = []
    with ops.deterministic():
        for first in (images, refs):
            m = build_model(cache_cfg).to(gpu).train()
            m.load_state_dict(model.state_dict())
            loss = F.cross_entropy(m((first, boxes, *extra))["activities"], labels)
            loss.backward()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(loss)) and all(p.grad is None for p in m.backbone.parameters())
            grads.append({k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None})
    assert grads[0] and grads[0].keys() == grads[1].keys() and any(bool(v.any()) for v in grads[0].values())
    differ = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert not differ, f"head gradients differ between the images tensor and the refs: {differ}"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tce_reads_its_context_from_the_map_cache(gpu, monkeypatch, dtype):
    """under backbone_dtype = 'bf16' the slots hold the bf16 map the backbone emits: half the bytes, the same bits"""
    cfg = _cfg("dynamic_tce_volleyball")
    cfg.train_dropout_prob, cfg.backbone_dtype = 0.3, dtype
    images, boxes = _clips(cfg, gpu, 2)
    model, cache, (plain, out1, out2) = _three_ways(gpu, monkeypatch, cfg, images, boxes)
    assert cache.map_dtype == (torch.float32 if dtype == "fp32" else torch.bfloat16) and cache.row_bytes == 3 * 5 * 512 * cache.itemsize
    assert plain.shape == (2, cfg.num_activities)
    assert torch.equal(plain, out1), "scores through all-missed refs differ from those of the images tensor"
    assert torch.equal(out1, out2), "scores from the slots differ from those of the computed maps"
    labels = torch.tensor([1, 6], device=gpu)
    _backward_both_ways(gpu, model, cfg, images, boxes, labels)


def test_collective_runs_roi_align_on_its_own_boxes(gpu, monkeypatch):
    """per-clip actor counts 1, 7 and 13 of MAX_N = 13: the maps do not depend on the boxes, so one cache serves them all"""
    cfg = _cfg("dynamic_collective", "collective")
    cfg.train_dropout_prob = 0.3
    images, boxes = _clips(cfg, gpu, 3)
    counts = torch.tensor([1, 7, 13], dtype=torch.int32, device=gpu)
    for b, n in enumerate(counts.tolist()):
        boxes[b, :, n:] = 0.0                                    # padding boxes are zero (collective.py)
    num = counts[:, None].repeat(1, T).contiguous()
    model, cache, (plain, out1, out2) = _three_ways(gpu, monkeypatch, cfg, images, boxes, (num,))
    assert plain.shape == (3, cfg.num_activities) and torch.equal(plain, out1) and torch.equal(out1, out2)
    _backward_both_ways(gpu, model, cfg, images, boxes, torch.tensor([0, 3, 4], device=gpu), (num,))


@pytest.mark.parametrize("name,frames", [("dynamic_volleyball", T), ("arg_volleyball", 3 * T)], ids=["dynamic", "arg_eval_fold"])
def test_the_other_models_take_the_refs_too(gpu, monkeypatch, name, frames):
    cfg = _cfg(name)
    images, boxes = _clips(cfg, gpu, 2, frames)
    _, _, (plain, out1, out2) = _three_ways(gpu, monkeypatch, cfg, images, boxes)
    assert plain.shape == (2, cfg.num_activities) and torch.equal(plain, out1) and torch.equal(out1, out2)


def test_the_feature_cache_still_has_no_context_for_tce(gpu):
    from din_amd.feature_cache import FeatureCache, FrameRefs, row_and_box_bytes
    from din_amd.train_net_dynamic import build_model
    cfg = _cfg("dynamic_tce_volleyball")
    model = build_model(cfg).to(gpu).eval()
    images, boxes = _clips(cfg, gpu, 1)
    refs = FrameRefs(np.arange(T).reshape(1, T), images.reshape(T, 3, 96, 160), np.arange(T), FeatureCache(gpu, *row_and_box_bytes(cfg), 1 << 26))
    with pytest.raises(ValueError, match="map_cache_gb"), torch.no_grad():
        model((refs, boxes))


# ---- 5. two epochs through the trainer --------------------------------------------------------------------------------------------------
def _trainer_cfg(module, dataset, map_cache_gb, deterministic):
    cfg = _cfg(module, dataset)
    cfg.data_path = os.path.join(GOLDEN, "dataset_tree", dataset)
    cfg.train_seqs, cfg.test_seqs = ([1], [4]) if dataset == "volleyball" else ([1], [15])
    cfg.num_before, cfg.num_after = 1, 1
    cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 2, 2, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.3, 1e-4, {}, 5
    cfg.result_path = None
    cfg.map_cache_gb, cfg.deterministic = map_cache_gb, deterministic
    return cfg


def _run_two_epochs(cfg):
    """train_net with decodes, backbone calls, map caches and the model recorded.  A decode or backbone call is recorded with the number
    of model calls made before it."""
    from din_amd import collective as Cc, feature_cache as FE, train_net_dynamic as TD, volleyball as V
    from din_amd.backbone.backbone import MyVGG16
    decodes, trunks, caches, models, rows, n_calls = [], [], [], [], [], [0]
    mods = (V, Cc)
    real_loads = [m.load_frame_u8 for m in mods]
    real_init, real_trunk, real_build = FE.MapCache.__init__, MyVGG16.forward_nhwc, TD.build_model

    def counting_load(k):
        def load(path, size):
            decodes.append(n_calls[0])
            return real_loads[k](path, size)
        return load

    def recording_init(self, *a, **kw):
        real_init(self, *a, **kw)
        caches.append(self)

    def counting_trunk(self, x):
        trunks.append((n_calls[0], int(x.shape[0])))
        return real_trunk(self, x)

    def recording_build(c):
        models.append(real_build(c))
        return models[-1]

    def pre_hook(module, args):
        if module is models[-1]:
            first = args[0][0]
            assert isinstance(first, FE.FrameRefs) == (cfg.map_cache_gb > 0) and tuple(first.shape[1:]) == (T, 3) + tuple(cfg.image_size)
            rows.append(first.shape[0] * T)
            n_calls[0] += 1

    handle = torch.nn.modules.module.register_module_forward_pre_hook(pre_hook)
    for k, m in enumerate(mods):
        m.load_frame_u8 = counting_load(k)
    FE.MapCache.__init__, MyVGG16.forward_nhwc, TD.build_model = recording_init, counting_trunk, recording_build
    try:
        infos = TD.train_net(cfg)
        torch.cuda.synchronize()
    finally:
        handle.remove()
        for m, real in zip(mods, real_loads):
            m.load_frame_u8 = real
        FE.MapCache.__init__, MyVGG16.forward_nhwc, TD.build_model = real_init, real_trunk, real_build
    weights = {k: v.detach().clone() for k, v in models[-1].state_dict().items()}
    return dict(decodes=decodes, trunks=trunks, caches=caches, infos=infos, weights=weights, rows=rows)


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "atomics"])
@pytest.mark.parametrize("module,dataset", [("dynamic_tce_volleyball", "volleyball"), ("dynamic_collective", "collective")])
def test_train_net_two_epochs_with_the_map_cache(gpu, module, dataset, deterministic):
    """two epochs with cfg.map_cache_gb = 1 against two epochs with 0, frozen VGG16, dropout on, same seed.  Epoch 1 decodes every frame
    once and runs the trunk on what a step decoded; epoch 2 decodes nothing and never calls the trunk; the infos' counters add up.
    Under cfg.deterministic the final weights are equal to the last bit; without it the per-epoch losses agree within the 1e-4 relative
    bound tests/test_gpu_feature_cache.py holds the feature cache to for the same reason (atomics in the backward)."""
    off = _run_two_epochs(_trainer_cfg(module, dataset, 0, deterministic))
    on = _run_two_epochs(_trainer_cfg(module, dataset, 1, deterministic))
    assert not off["caches"] and off["rows"] == on["rows"] and len(on["caches"]) == 2
    steps = len(on["rows"]) // 2                                 # model calls of one epoch (training steps, then validation steps)
    frames = sum(on["rows"][:steps])
    assert [n for _, n in off["trunks"]] == off["rows"] and len(off["decodes"]) == 2 * frames
    for e, (i0, i1) in enumerate(zip(off["infos"], on["infos"])):
        for part in ("train", "test"):
            assert "map_cache_hits" not in i0[part] and "map_cache_inserted" not in i0[part]
    # epoch 1: every frame decoded once, the trunk once per step over the step's decoded frames; epoch 2: nothing
    assert len(on["decodes"]) == frames and all(c < steps for c in on["decodes"])
    assert on["trunks"] == [(k + 1, on["rows"][k]) for k in range(steps)], on["trunks"]      # (recorded inside model call k)
    first, second = on["infos"]
    assert first["train"]["map_cache_inserted"] + first["test"]["map_cache_inserted"] == frames == sum(c.inserted for c in on["caches"])
    assert first["train"]["map_cache_hits"] == first["test"]["map_cache_hits"] == 0
    assert second["train"]["map_cache_inserted"] == second["test"]["map_cache_inserted"] == 0
    assert second["train"]["map_cache_hits"] + second["test"]["map_cache_hits"] == frames == sum(c.hits for c in on["caches"])
    for i0, i1 in zip(off["infos"], on["infos"]):
        for part in ("train", "test"):
            a, b = i1[part]["loss"], i0[part]["loss"]
            print(f"{module} epoch {i0[part]['epoch']} {part} loss, cache off {b!r}, cache on {a!r}, relative difference {abs(a - b) / max(1.0, abs(b)):.3e}")
            assert Measured(abs(a - b)) <= 1e-4 * max(1.0, abs(b)), (part, a, b)
    if deterministic:
        differ = [k for k in off["weights"] if not torch.equal(off["weights"][k], on["weights"][k])]
        assert not differ, f"{module}: final weights differ between map_cache_gb = 0 and 1 under cfg.deterministic: {differ}"


# ---- 6. the setting at 0 -------------------------------------------------------------------------------------------------------------
def test_a_step_with_the_setting_at_zero_launches_what_it_always_did(gpu, monkeypatch):
    """the C-ABI entry points called, in order, by one epoch of train_net for dynamic_tce_volleyball (one training step, one validation
    step): with cfg.map_cache_gb = 0 they are the ones of a cfg that has no such attribute at all -- the cfg of before the setting existed
    -- and neither run calls a gather entry point, builds a cache or reports a map-cache counter."""
    from din_amd import _lib as L, feature_cache as FE
    from din_amd.train_net_dynamic import train_net
    lib, calls = L.load(), []

    def wrap(name, real):
        def call(*a):
            calls.append(name)
            return real(*a)
        return call

    for name in L.SIGNATURES:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    monkeypatch.setattr(FE.MapCache, "__init__", lambda *a, **k: pytest.fail("a map cache was built with the setting at 0"))
    surveys = []
    for absent in (False, True):
        cfg = _trainer_cfg("dynamic_tce_volleyball", "volleyball", 0, False)
        cfg.max_epoch = 1
        if absent:
            del cfg.map_cache_gb
        del calls[:]
        info, = train_net(cfg)
        torch.cuda.synchronize()
        assert not any("map_cache" in k for part in ("train", "test") for k in info[part])
        surveys.append([c for c in calls if c not in ("din_get_option", "din_set_option", "din_last_error_string")])
    assert surveys[0] == surveys[1] and len(surveys[0]) > 50
    assert not any(c.startswith(("din_feat_rows", "din_copy_rows")) for c in surveys[0])
    assert "din_roi_align_fwd" in surveys[0] and any(c.startswith("din_conv") for c in surveys[0])
