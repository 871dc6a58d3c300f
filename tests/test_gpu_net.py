"""GPU parity of the whole RetinaNet forward (stem -> ResNet-50 -> FPN -> heads -> decode/NMS) against the
torch-CPU oracle (oracle/ref_net.py; parity unpinned: no Keras/TF here, no checkpoint in the reference).

Tolerances (stated, measured on MI355X):
  fp32 path : every decoded box within 1e-3 px and every score within 1e-5 of the float64 oracle
              (BASELINE.json north_star: "boxes within 1e-3 of the Keras reference").
  bf16 path : boxes within 2 px and scores within 2e-2 of the float64 oracle AND of the oracle run in bf16
              emulation (bf16 weights, bf16 activations between layers, fp32 accumulate).  Measured on MI355X on
              this 160x224 canvas: 0.58 px / 9.2e-3 vs float64, 0.59 px / 7.7e-3 vs the emulation — the two are the
              same size because a different fp32 summation order flips bf16 roundings (1 ulp = 0.4 %) layer after
              layer, so bf16 runs only agree with each other to the bf16 noise floor (torch-CPU's own bf16
              emulation sits 0.83 px / 7.9e-3 from float64).
Post-processing is checked bit-exactly by feeding the engine's own head outputs through the oracle's
filter_detections."""
import importlib

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from oracle.ref_net import RefNet

pytestmark = pytest.mark.gpu
CANVAS = (160, 224)


def mods(pkg):
    return importlib.import_module(pkg.__name__ + ".engine"), importlib.import_module(pkg.__name__ + ".weights")


def make_images(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    # heavy-tailed distance-map-like pixels in [0,255] -> custom_tf normalisation
    raw = torch.clamp(torch.empty(B, CANVAS[0], CANVAS[1], 3).exponential_(1 / 12.0, generator=g) *
                      torch.rand(B, CANVAS[0], CANVAS[1], 3, generator=g), 0, 255).round()
    return raw.to(torch.uint8)


@pytest.fixture(scope="module")
def state(pkg):
    _, Wt = mods(pkg)
    return Wt.init_state("resnet50", 1, 9, seed=0, randomize_bn=True, cls_bias=0.0, tame=True)


def decoded(reg, canvas):
    a32 = R.anchors_f32(canvas + (3,))
    return np.stack([R.decode_boxes_f32(a32, reg[b], canvas) for b in range(reg.shape[0])])


def test_fp32_network_boxes_within_1e3_px(pkg, state):
    E, _ = mods(pkg)
    img_u8 = make_images(2)
    x = torch.as_tensor(R.preprocess_custom_tf(img_u8.numpy()))
    eng = E.Engine("resnet50", 1, 9, dtype="f32")
    eng.load_state(state)
    reg, cls = eng.forward(x.cuda())
    torch.cuda.synchronize()
    reg, cls = reg.cpu().numpy(), cls.cpu().numpy()
    oreg, ocls = RefNet(state, dtype=torch.float64).forward(x.numpy())
    oreg, ocls = oreg.numpy(), ocls.numpy()
    assert reg.shape == oreg.shape and cls.shape == ocls.shape
    dbox = np.abs(decoded(reg, CANVAS).astype(np.float64) - decoded(oreg.astype(np.float32), CANVAS)).max()
    dcls = np.abs(cls - ocls).max()
    treg, tcls = RefNet(state, dtype=torch.float32).forward(x.numpy())          # yardstick: oneDNN fp32 vs float64
    tbox = np.abs(decoded(treg.numpy(), CANVAS).astype(np.float64) - decoded(oreg.astype(np.float32), CANVAS)).max()
    print("fp32 path: max |box diff| = %.3e px (torch-CPU fp32 yardstick %.3e), max |score diff| = %.3e, "
          "max |regression diff| = %.3e, |regression| max %.2f rms %.3f" %
          (dbox, tbox, dcls, np.abs(reg - oreg).max(), np.abs(oreg).max(), np.sqrt((oreg ** 2).mean())))
    assert dbox <= 1e-3 and dcls <= 1e-5
    # the uint8 entry (normalisation fused into the stem packer) gives the same bits as the float entry
    reg8, cls8 = eng.forward(img_u8.cuda())
    torch.cuda.synchronize()
    assert np.array_equal(reg8.cpu().numpy(), reg) and np.array_equal(cls8.cpu().numpy(), cls)
    # post-processing: bit-exact given the same head outputs
    boxes, scores, labels = eng.detect(x.cuda())
    torch.cuda.synchronize()
    for b in range(2):
        wb, ws, wl = R.filter_detections(decoded(reg, CANVAS)[b], cls[b])
        assert np.array_equal(boxes[b].cpu().numpy(), wb) and np.array_equal(scores[b].cpu().numpy(), ws)
        assert np.array_equal(labels[b].cpu().numpy(), wl)
    assert (scores[0] > 0).sum() > 0


def test_bf16_network_vs_bf16_emulating_oracle(pkg, state):
    E, _ = mods(pkg)
    img_u8 = make_images(2, seed=1)
    x = torch.as_tensor(R.preprocess_custom_tf(img_u8.numpy()))
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    reg, cls = eng.forward(x.cuda())
    torch.cuda.synchronize()
    reg, cls = reg.cpu().numpy(), cls.cpu().numpy()
    ereg, ecls = RefNet(state, dtype=torch.float32, emulate_bf16=True).forward(x.numpy())
    oreg, ocls = RefNet(state, dtype=torch.float64).forward(x.numpy())
    ereg, ecls, oreg, ocls = ereg.numpy(), ecls.numpy(), oreg.numpy(), ocls.numpy()
    db_e = np.abs(decoded(reg, CANVAS).astype(np.float64) - decoded(ereg, CANVAS)).max()
    ds_e = np.abs(cls - ecls).max()
    db_o = np.abs(decoded(reg, CANVAS).astype(np.float64) - decoded(oreg.astype(np.float32), CANVAS)).max()
    ds_o = np.abs(cls - ocls).max()
    print("bf16 path vs bf16-emulating oracle: box %.3e px, score %.3e; vs float64 oracle: box %.3e px, score %.3e" %
          (db_e, ds_e, db_o, ds_o))
    assert db_e <= 2.0 and ds_e <= 2e-2
    assert db_o <= 2.0 and ds_o <= 2e-2
    boxes, scores, labels = eng.detect(x.cuda())
    torch.cuda.synchronize()
    for b in range(2):
        wb, ws, wl = R.filter_detections(decoded(reg, CANVAS)[b], cls[b])
        assert np.array_equal(boxes[b].cpu().numpy(), wb) and np.array_equal(scores[b].cpu().numpy(), ws)


def test_prior_probability_bias_gives_empty_detections(pkg):
    """PriorProbability (model/initializers.py:19-22): with the classification output kernel at zero every score is
    sigmoid(-log(99)) = 0.01 < 0.05, so the padded outputs are all -1 (model/layers.py:250-253)."""
    E, Wt = mods(pkg)
    st = Wt.init_state("resnet50", 1, 9, seed=1, tame=True, randomize_bn=True)
    st["pyramid_classification/kernel"] = np.zeros_like(st["pyramid_classification/kernel"])
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(st)
    x = torch.as_tensor(R.preprocess_custom_tf(make_images(1).numpy())).cuda()
    reg, cls = eng.forward(x)
    assert torch.allclose(cls, torch.full_like(cls, 0.01), atol=1e-6)
    boxes, scores, labels = eng.detect(x)
    torch.cuda.synchronize()
    assert torch.all(scores == -1) and torch.all(labels == -1) and torch.all(boxes == -1)


def test_backbone_validation(pkg):
    E, _ = mods(pkg)
    with pytest.raises(ValueError):
        E.Engine("vgg16", 1, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,B,hw", [("bf16", 2, (320, 416)), ("f32", 1, (256, 256)), ("bf16", 3, (512, 672))])
def test_stream_lanes_give_the_single_stream_bits(pkg, state, dtype, B, hw):
    """The forward pass runs the graph's forks (branch1, P6/P7, P5/P4, the classification tower) on side HIP streams with
    events on every cross-lane read (engine.Engine._schedule).  A missing dependency or a shared scratch buffer shows up
    as different bits: compare with the single-stream order, several passes back to back."""
    E, _ = mods(pkg)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, hw[0], hw[1], 3, generator=g) * 2 - 1).cuda()
    eng = E.Engine("resnet50", 1, 9, dtype=dtype)
    eng.load_state(state)
    eng.two_streams = False
    r0, c0 = [t.clone() for t in eng.forward(x)]
    torch.cuda.synchronize()
    eng.two_streams = True
    sched = eng._plan(B, hw[0], hw[1])["sched"]
    assert sched["nlanes"] >= 3 and len(sched["joins"]) >= 2
    for _ in range(4):
        r1, c1 = eng.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(r0, r1) and torch.equal(c0, c1)


@pytest.mark.gpu
@pytest.mark.parametrize("hw,src", [((64, 96), "bf16"), ((67, 101), "f32"), ((33, 35), "u8"), ((130, 71), "bf16")])
def test_fused_stem_matches_the_three_kernel_stem(pkg, state, hw, src):
    """rtn_stem_conv_pool (conv1 + ReLU + pool1 in one kernel, inference bf16 path) against the same engine running
    rtn_stem_pack -> rtn_conv2d_fwd -> rtn_maxpool3x3s2_tfsame_fwd.  Both multiply bf16 inputs and weights and round the ReLU
    output to bf16 once; only the f32 summation order differs, so outputs agree to one bf16 ulp of the activation scale
    (stated: 2^-7 relative to the largest activation; most elements are identical).  Odd sizes exercise both pool paddings
    (H1 even: pad 0/1, H1 odd: pad 1/1), partial tiles and the image border inside a tile."""
    E, _ = mods(pkg)
    B = 2
    g = torch.Generator().manual_seed(11)
    if src == "u8":
        x = torch.randint(0, 256, (B, hw[0], hw[1], 3), generator=g, dtype=torch.uint8).cuda()
    else:
        x = (torch.rand(B, hw[0], hw[1], 3, generator=g) * 2 - 1).to({"bf16": torch.bfloat16, "f32": torch.float32}[src]).cuda()
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    outs = {}
    for fuse in (False, True):
        eng.fuse_stem = fuse
        [op for op in eng._plan(B, hw[0], hw[1])["ops"] if op[0] == "pool"][0][2].fill_(-3.0)     # both paths write this buffer
        eng.forward(x)
        torch.cuda.synchronize()
        plan = eng._plan(B, hw[0], hw[1])
        pool_out = [op for op in plan["ops"] if op[0] == "pool"][0][2]
        outs[fuse] = pool_out.float().cpu().clone()
        assert any(op[0] == "stem" for op in eng.active_ops(plan)) == fuse
    a, b = outs[False], outs[True]
    scale = float(a.abs().max())
    assert scale > 0.1
    err = float((a - b).abs().max())
    same = float((a == b).float().mean())
    print("fused stem: max |diff| %.3e (scale %.2f), identical elements %.4f" % (err, scale, same))
    assert err <= scale * 2.0 ** -7 and same > 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("hw,grid", [((64, 96), 0), ((131, 203), 3), ((97, 160), 1), ((33, 35), 0)])
def test_stem_with_branch2a_matches_the_separate_layer(pkg, state, monkeypatch, hw, grid):
    """rtn_stem_conv_pool_branch2a: the persistent stem kernel also applies res2a_branch2a (1x1, 64 -> 64, BN, ReLU; keras_resnet
    bottleneck behind model/defineModel.py:376-380) to the pooled pixels.  pool1 must equal the stem-only kernel's BIT FOR BIT (same
    MFMA order); the branch2a tensor is compared with the separate rtn_conv2d_fwd launch on that pool1: same bf16 operands, another
    f32 summation order (bias first), so one bf16 ulp of the activation scale (stated: 2^-7 of the largest activation, most elements
    identical).  RTN_STEM_GRID limits the workgroups: up to 60 tiles per workgroup through the register prefetch of the next patch."""
    E, _ = mods(pkg)
    B = 2
    if grid:
        monkeypatch.setenv("RTN_STEM_GRID", str(grid))
    g = torch.Generator().manual_seed(hw[0])
    x = (torch.rand(B, hw[0], hw[1], 3, generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    plan = eng._plan(B, hw[0], hw[1])
    pool_out = [op for op in plan["ops"] if op[0] == "pool"][0][2]
    a_out = [op for op in plan["ops"] if op[0] == "conv" and op[2] == "res2a_branch2a"][0][3]["ys"][0]
    outs = {}
    for with2a in (False, True):
        eng.fuse_stem_2a = with2a
        pool_out.fill_(-3.0)
        a_out.fill_(-3.0)
        reg, cls = eng.forward(x)
        torch.cuda.synchronize()
        names = [op[2] for op in eng.active_ops(plan) if op[0] == "conv"]
        stem = [op for op in eng.active_ops(plan) if op[0] == "stem"][0]
        assert ("res2a_branch2a" in names) == (not with2a) and (stem[7] is not None) == with2a
        outs[with2a] = (pool_out.clone(), a_out.float().cpu().clone(), reg.clone(), cls.clone())
    assert torch.equal(outs[False][0], outs[True][0])
    a, b = outs[False][1], outs[True][1]
    scale = float(a.abs().max())
    err, same = float((a - b).abs().max()), float((a == b).float().mean())
    print("branch2a in the stem: max |diff| %.3e (scale %.2f), identical elements %.4f" % (err, scale, same))
    assert scale > 0.1 and err <= scale * 2.0 ** -7 and same > 0.9
    assert torch.isfinite(outs[True][2]).all() and torch.isfinite(outs[True][3]).all()
    # a second run repeats bit for bit (tile order and prefetch do not matter)
    eng.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(a_out.float().cpu(), b)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,hw", [("bf16", (160, 224)), ("f32", (96, 128))])
def test_fused_shortcut_matches_separate_layers(pkg, state, dtype, hw):
    """rtn_conv1x1_dual_fwd folds the projection shortcut of every stage's first block into its branch2c as extra K
    (inference only).  The separate path rounds the shortcut tensor to the storage dtype before the add; the fused one adds
    in f32, so the two agree to the storage rounding of the block output: fp32 2e-5 relative, bf16 2^-6 of the activation
    scale (stated; measured values are printed).  Stages 3-5 exercise the stride-2 sampling of the second source."""
    E, _ = mods(pkg)
    B = 2
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(B, hw[0], hw[1], 3, generator=g) * 2 - 1).cuda()
    eng = E.Engine("resnet50", 1, 9, dtype=dtype)
    eng.load_state(state)
    eng.fuse_stem = False
    feats = {}
    for fuse in (False, True):
        eng.fuse_shortcut = fuse
        plan = eng._plan(B, hw[0], hw[1])
        for t in plan["feats"]:
            t.fill_(-7.0)
        eng.forward(x)
        torch.cuda.synchronize()
        assert any(op[0] == "dual" for op in eng.active_ops(plan)) == fuse
        feats[fuse] = [t.float().cpu().clone() for t in plan["feats"]]
    tol = 2e-5 if dtype == "f32" else 2.0 ** -6
    for lvl, (a, b) in enumerate(zip(feats[False], feats[True])):
        scale = float(a.abs().max())
        err = float((a - b).abs().max())
        print("C%d: max |diff| %.3e, scale %.2f" % (lvl + 2, err, scale))
        assert scale > 0.05 and err <= tol * scale


@pytest.mark.gpu
def test_plan_builds_only_the_variants_that_run(pkg, state):
    """A plan builds the fused op list of a fusion key on its first use (engine.Engine._variant), not every key up front: an
    inference and a training forward leave exactly their two variants, and both run the same folded-shortcut ops - one descriptor
    and one workspace per stage-first block for the whole plan."""
    E, _ = mods(pkg)
    B = 2
    x = (torch.rand(B, CANVAS[0], CANVAS[1], 3, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    eng.forward(x)
    infer = eng._fused()
    eng.training = True
    try:
        eng.forward(x)
        train = eng._fused()
    finally:
        eng.training = False
    torch.cuda.synchronize()
    plan = eng._plan(B, CANVAS[0], CANVAS[1])
    assert infer != train and set(plan["variants"]) == {infer, train}
    infer_dual, train_dual = [{op[2]: op[1] for op in plan["variants"][k]["ops"] if op[0] == "dual"} for k in (infer, train)]
    assert len(infer_dual) >= 3 and set(infer_dual) == set(train_dual)
    for name, d in infer_dual.items():
        assert d is train_dual[name] and d.workspace == train_dual[name].workspace


@pytest.mark.gpu
def test_full_size_passes_repeat_bit_for_bit(pkg, state):
    """BASELINE configuration (batch 8, 800x1333, bf16, every fusion and the stream lanes on): 40 back-to-back detect() calls must
    give the same bits as the first one (the kernels are deterministic - split-K sums in slice order, no float atomics in
    inference - so any difference is a missing cross-stream dependency or a reused buffer)."""
    E, _ = mods(pkg)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(8, 800, 1333, 3, generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    st = dict(state)
    st["pyramid_classification/bias"] = (state["pyramid_classification/bias"] * 0 - 2.0).astype("float32")   # a few thousand candidates
    eng.load_state(st)
    b0, s0, l0 = [t.clone() for t in eng.detect(x)]
    plan = eng._plan(8, 800, 1333)
    r0, c0 = plan["regression"].clone(), plan["classification"].clone()
    torch.cuda.synchronize()
    assert int((l0 >= 0).sum()) > 100
    for _ in range(40):
        b, s, l = eng.detect(x)
    torch.cuda.synchronize()
    assert torch.equal(plan["regression"], r0) and torch.equal(plan["classification"], c0)
    assert torch.equal(b, b0) and torch.equal(s, s0) and torch.equal(l, l0)


@pytest.mark.gpu
def test_full_size_backbone_outputs_repeat_and_match_the_unfused_path(pkg, state):
    """The fused bottleneck blocks (rtn_bottleneck64_fwd) and the persistent kernels at the BASELINE size: six forward passes must
    give identical C2..C5 bits (a store-data hazard in the fused kernel once corrupted a few hundred pixels per launch, differently
    every run - see the guard in csrc/rtn_bottleneck.hip), and the fused path must agree with the same engine running every
    bottleneck layer as its own launch to 2^-6 of each feature map's scale (same bf16 rounding points, other f32 summation order)."""
    E, _ = mods(pkg)
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(8, 800, 1333, 3, generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    feats = {}
    for fuse in (True, False):
        eng.fuse_bottleneck = fuse
        plan = eng._plan(8, 800, 1333)
        first = None
        for rep in range(6 if fuse else 1):
            for t in plan["feats"]:
                t.fill_(-7.0)
            eng.forward(x)
            torch.cuda.synchronize()
            cur = [t.clone() for t in plan["feats"]]
            if first is None:
                first = cur
            else:
                for lvl, (a, b) in enumerate(zip(first, cur)):
                    assert torch.equal(a, b), "C%d differs between passes %d and 0" % (lvl + 2, rep)
        feats[fuse] = first
    for lvl, (a, b) in enumerate(zip(feats[False], feats[True])):
        a, b = a.float(), b.float()
        scale, err = float(a.abs().max()), float((a - b).abs().max())
        print("C%d: fused vs separate max |diff| %.3e, scale %.2f" % (lvl + 2, err, scale))
        assert err <= 2.0 ** -6 * scale


@pytest.mark.gpu
def test_map_of_the_device_paths_against_the_float64_oracle(pkg, state):
    """BASELINE.json's metric asks for 'box mAP vs ref'.  No trained checkpoint or labelled set exists in the reference, so the
    float64 oracle's own detections (its top-scoring boxes after NMS) play the ground truth and each device path is scored
    against them with the evaluator (model/eval.py): AP at IoU 0.5 / 0.75 / 0.9.  A box that drifts by a fraction of a pixel
    keeps IoU > 0.9 on all but the smallest anchors; what costs AP is a change of WHICH candidates survive NMS (score ties
    broken differently by a 1e-2 score drift).  Stated floors: fp32 path AP50 = AP75 = 1, AP90 >= 0.99; bf16 AP50 >= 0.95,
    AP75 >= 0.9."""
    E, _ = mods(pkg)
    Ev = importlib.import_module("retinanet-for-table-detection_amd.model.eval")
    img_u8 = make_images(2, seed=3)
    x = torch.as_tensor(R.preprocess_custom_tf(img_u8.numpy()))
    st = dict(state)
    st["pyramid_classification/bias"] = (state["pyramid_classification/bias"] * 0 - 1.0).astype("float32")
    oreg, ocls = RefNet(st, dtype=torch.float64).forward(x.numpy())
    oreg, ocls = oreg.numpy().astype(np.float32), ocls.numpy().astype(np.float32)
    anns = []
    for b in range(2):
        wb, ws, wl = R.filter_detections(decoded(oreg, CANVAS)[b], ocls[b], max_detections=60)
        anns.append([wb[ws >= 0].astype(np.float64)])
        assert len(anns[-1][0]) >= 20
    for dtype, floors in (("f32", (1.0, 1.0, 0.99)), ("bf16", (0.95, 0.9, 0.0))):
        eng = E.Engine("resnet50", 1, 9, dtype=dtype)
        eng.load_state(st)
        boxes, scores, labels = eng.detect(x.cuda(), max_detections=60)
        torch.cuda.synchronize()
        dets = [Ev.split_detections(boxes[b].cpu().numpy(), scores[b].cpu().numpy(), labels[b].cpu().numpy(), 1, max_detections=60)
                for b in range(2)]
        aps = [Ev.evaluate_detections(dets, anns, 1, iou_threshold=t)[0][0] for t in (0.5, 0.75, 0.9)]
        print("%s path vs float64 oracle detections: AP50 %.4f AP75 %.4f AP90 %.4f" % (dtype, *aps))
        for ap, floor in zip(aps, floors):
            assert ap >= floor


@pytest.mark.gpu
@pytest.mark.parametrize("K,B,hw,src,thr,nms,md", [
    (3, 1, (97, 131), "f32", 0.05, 0.5, 300),     # odd canvas, three classes, one image
    (1, 3, (224, 160), "u8", 0.30, 0.3, 17),      # portrait canvas, uint8 pages, tight thresholds, 17 detections
    (2, 2, (64, 64), "bf16", 0.60, 0.7, 100),     # tiny canvas: P6/P7 are 1x1 and 1x1
    (20, 2, (97, 131), "bf16", 0.05, 0.5, 300),   # twenty classes: 180 classification channels, per-class NMS over 20 lists
])
def test_detect_parameters_and_shapes(pkg, K, B, hw, src, thr, nms, md):
    """End to end on unusual shapes and detection parameters: the post-processing must equal the oracle's filter_detections on
    the engine's own head outputs bit for bit (model/layers.py:177-264), whatever the class count, thresholds or
    max_detections; the head outputs stay within the bf16 tolerance of the bf16-emulating oracle."""
    E, Wt = mods(pkg)
    st = Wt.init_state("resnet50", K, 9, seed=3, randomize_bn=True, cls_bias=0.5, tame=True)
    g = torch.Generator().manual_seed(9)
    u8 = torch.randint(0, 256, (B, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    xf = torch.as_tensor(R.preprocess_custom_tf(u8.numpy()))
    x = {"u8": u8, "f32": xf, "bf16": xf.to(torch.bfloat16)}[src].cuda()
    eng = E.Engine("resnet50", K, 9, dtype="bf16")
    eng.load_state(st)
    boxes, scores, labels = eng.detect(x, score_threshold=thr, nms_threshold=nms, max_detections=md)
    torch.cuda.synchronize()
    assert boxes.shape == (B, md, 4) and scores.shape == (B, md) and labels.shape == (B, md)
    plan = eng._plan(B, hw[0], hw[1])
    reg, cls = plan["regression"].cpu().numpy(), plan["classification"].cpu().numpy()
    assert cls.shape == (B, plan["N"], K)
    a32 = R.anchors_f32(hw + (3,))
    n_det = 0
    for b in range(B):
        wb, ws, wl = R.filter_detections(R.decode_boxes_f32(a32, reg[b], hw), cls[b], score_threshold=thr, max_detections=md,
                                         nms_threshold=nms)
        assert np.array_equal(boxes[b].cpu().numpy(), wb) and np.array_equal(scores[b].cpu().numpy(), ws)
        assert np.array_equal(labels[b].cpu().numpy(), wl)
        n_det += int((ws >= 0).sum())
    assert n_det > 0
    xin = xf if src != "bf16" else xf.to(torch.bfloat16).float()
    ereg, ecls = RefNet(st, num_classes=K, dtype=torch.float32, emulate_bf16=True).forward(xin.numpy())
    dbox = np.abs(np.stack([R.decode_boxes_f32(a32, reg[b], hw) for b in range(B)]).astype(np.float64) -
                  np.stack([R.decode_boxes_f32(a32, ereg.numpy()[b], hw) for b in range(B)])).max()
    dcls = np.abs(cls - ecls.numpy()).max()
    print("K=%d B=%d %s %s: box %.3e px, score %.3e, %d detections" % (K, B, hw, src, dbox, dcls, n_det))
    assert dbox <= 2.0 and dcls <= 2e-2


def test_batches_in_flight_give_the_bits_of_one_at_a_time(pkg):
    """Engine.in_flight = 2: consecutive detect() calls run on two buffer sets, each on a HIP stream of its own, and overlap on the
    device.  Five different batches through it (so both buffer sets are reused, the second time behind their own previous batch)
    must give, after join(), exactly what the same batches give one at a time; the page tensor may be overwritten as soon as detect()
    has returned (the packer consumed it in the caller's stream order)."""
    E = importlib.import_module(pkg.__name__ + ".engine")
    Wt = importlib.import_module(pkg.__name__ + ".weights")
    state = Wt.init_state("resnet50", 1, 9, seed=0, randomize_bn=True, cls_bias=-3.0, tame=True)
    eng = E.Engine("resnet50", 1, 9, dtype="bf16")
    eng.load_state(state)
    g = torch.Generator().manual_seed(9)
    pages = [torch.randint(0, 256, (2, 160, 224, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(5)]
    want = []
    for p in pages:
        b, s, l = eng.detect(p)
        torch.cuda.synchronize()
        want.append((b.clone(), s.clone(), l.clone()))
    assert sum(int((w[1] >= 0).sum()) for w in want) > 10              # there is something to compare
    eng.in_flight = 2
    buf = torch.empty_like(pages[0])
    got = []
    for p in pages:
        buf.copy_(p)
        got.append(eng.detect(buf))
        buf.fill_(0)                                                   # the caller overwrites its page at once
        if len(got) >= 2:                                              # the buffer set of call i is reused by call i + 2: copy i out first
            eng.join()
            got[-2] = tuple(t.clone() for t in got[-2])
    eng.join()
    got[-1] = tuple(t.clone() for t in got[-1])
    torch.cuda.synchronize()
    for i, (w, gt) in enumerate(zip(want, got)):
        for a, b_ in zip(w, gt):
            assert torch.equal(a, b_), "batch %d differs between one at a time and two in flight" % i
    # ... and with nothing between the calls (the two batches really overlap): the last two results are still in their buffer sets
    last = [eng.detect(p) for p in pages[1:5]][-2:]
    eng.join()
    torch.cuda.synchronize()
    for w, gt in zip(want[3:5], last):
        for a, b_ in zip(w, gt):
            assert torch.equal(a, b_)
    eng.in_flight = 1
    b, s, l = eng.detect(pages[0])                                     # back to one at a time on the same engine
    torch.cuda.synchronize()
    assert torch.equal(b, want[0][0]) and torch.equal(s, want[0][1])
