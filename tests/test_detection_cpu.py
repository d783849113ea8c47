"""Detection side tree on the CPU: RCNNKD (DKD / ReviewKD / ReviewDKD, with and
without masks) forward + backward on tiny synthetic batches, ROI sampling
invariants, ReviewKD chain + HCL parity with the reference module
(`detection/model/reviewkd.py`, its stored outputs), the COCO evaluator, and
the train_net CLI with checkpoint/resume."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from mdistiller_ddp_amd.detection.config import get_det_cfg, merge_det_file
from mdistiller_ddp_amd.detection.data import build_detection_data
from mdistiller_ddp_amd.detection.engine import coco_evaluate, warmup_multistep_lr
from mdistiller_ddp_amd.detection.rcnn import build_kd_trans, build_model, hcl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = os.path.join(ROOT, "detection", "configs")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def tiny_cfg(path, mask=None):
    cfg = get_det_cfg()
    merge_det_file(cfg, os.path.join(CFGS, path))
    cfg.RUNTIME.SYNTHETIC_SIZE = (96, 128)
    cfg.SOLVER.IMS_PER_BATCH = 2
    for m in (cfg.MODEL, cfg.TEACHER.MODEL):
        m.RPN.POST_NMS_TOPK_TRAIN = 100
        m.RPN.PRE_NMS_TOPK_TRAIN = 200
        m.RPN.POST_NMS_TOPK_TEST = 50
        m.RPN.PRE_NMS_TOPK_TEST = 100
        m.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
        m.ROI_HEADS.NUM_CLASSES = 8
    if mask is not None:
        cfg.MODEL.MASK_ON = mask
    return cfg


@pytest.mark.parametrize("path", ["DKD/DKD-R18-R101.yaml", "ReviewKD/ReviewKD-R18-R101-Mask.yaml",
                                  "DKD/ReviewDKD-MV2-R50.yaml"])
def test_rcnnkd_train_step(path):
    torch.manual_seed(0)
    cfg = tiny_cfg(path)
    model = build_model(cfg).train()
    _, loader = build_detection_data(cfg)
    batch = next(iter(loader))
    losses = model(batch)
    kd = cfg.KD.TYPE
    expect = {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
    if kd in ("DKD", "ReviewDKD"):
        expect.add("loss_dkd")
    if kd in ("ReviewKD", "ReviewDKD"):
        expect.add("loss_reviewkd")
    if cfg.MODEL.MASK_ON:
        expect.add("loss_mask")
    assert set(losses) == expect
    for k, v in losses.items():
        assert torch.isfinite(v), (k, v)
    sum(losses.values()).backward()
    for n, p in model.named_parameters():
        if n.startswith("teacher."):
            assert p.grad is None, n
    got = [n for n, p in model.named_parameters() if p.grad is not None and p.grad.abs().sum() > 0]
    assert any(n.startswith("roi_heads.box_predictor") for n in got)
    assert any(n.startswith("backbone.fpn_") for n in got)
    if kd != "DKD":
        assert any(n.startswith("kd_trans.") for n in got)
    # inference path
    model.eval()
    out = model(batch[:1])[0]["instances"]
    assert out.has("pred_boxes") and out.has("scores") and len(out) <= 100
    if cfg.MODEL.MASK_ON:
        assert out.pred_masks.shape[1:] == (batch[0]["height"], batch[0]["width"])


def test_roi_sampling_invariants():
    torch.manual_seed(0)
    cfg = tiny_cfg("DKD/DKD-R18-R101.yaml")
    model = build_model(cfg).train()
    _, loader = build_detection_data(cfg)
    batch = next(iter(loader))
    gts = [x["instances"] for x in batch]
    from mdistiller_ddp_amd.detection.structures import Instances
    props = [Instances(g.image_size, proposal_boxes=torch.cat([g.gt_boxes + 3, g.gt_boxes * 0.5])) for g in gts]
    sampled = model.roi_heads.label_and_sample_proposals(props, gts)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    for s, g in zip(sampled, gts):
        assert len(s) <= cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE
        fg = (s.gt_classes >= 0) & (s.gt_classes < K)
        assert fg.sum() >= len(g)  # appended gt boxes are always foreground
        assert fg.sum() <= int(cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE * cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION)
        assert ((s.gt_classes == K) | fg).all()


def test_reviewkd_chain_and_hcl_match_reference():
    # the reference module's parameters, inputs, outputs and HCL value, stored by
    # scripts/gen_ref_fixtures.py::det_reviewkd
    inp = load_file(os.path.join(GOLDEN, "ref_det_reviewkd_inputs.safetensors"))
    ref = load_file(os.path.join(GOLDEN, "ref_det_reviewkd_outputs.safetensors"))
    ours = build_kd_trans(None, channels=32, levels=5).train()
    # parameter order matches: abfs reversed in both
    theirs_sd = {k[3:]: v for k, v in inp.items() if k.startswith("sd/")}
    assert set(ours.state_dict()) == set(theirs_sd)
    ours.load_state_dict(theirs_sd)
    feats = [inp[f"feat{i}"] for i in range(5)]
    assert [f.shape[-1] for f in feats] == [32, 16, 8, 4, 2]
    a = ours([f.clone() for f in feats])
    b = [ref[f"out{i}"] for i in range(5)]
    assert len(a) == len(b)
    for x, y in zip(a, b):
        torch.testing.assert_close(x, y, atol=1e-4, rtol=1e-4)
    t = [ref[f"target{i}"] for i in range(5)]
    torch.testing.assert_close(hcl(a, t), ref["hcl"], atol=1e-5, rtol=1e-5)


def test_coco_evaluator_perfect_and_empty():
    rng = np.random.default_rng(0)
    gts, perfect, empty = [], [], []
    for _ in range(4):
        xy = rng.uniform(0, 300, (5, 2))
        wh = rng.uniform(10, 150, (5, 2))
        b = np.concatenate([xy, xy + wh], 1)
        c = rng.integers(0, 3, 5)
        gts.append({"boxes": b, "classes": c})
        perfect.append({"boxes": b.copy(), "classes": c.copy(), "scores": rng.uniform(0.5, 1, 5)})
        empty.append({"boxes": np.zeros((0, 4)), "classes": np.zeros(0, int), "scores": np.zeros(0)})
    r = coco_evaluate(perfect, gts, 3)
    assert abs(r["AP"] - 100) < 1e-6 and abs(r["AP50"] - 100) < 1e-6
    assert coco_evaluate(empty, gts, 3)["AP"] == 0.0
    # half the boxes shifted off: AP50 drops below 100 but stays positive
    shifted = [{"boxes": p["boxes"] + np.array([[200, 200, 200, 200]] * 2 + [[0, 0, 0, 0]] * 3),
                "classes": p["classes"], "scores": p["scores"]} for p in perfect]
    r2 = coco_evaluate(shifted, gts, 3)
    assert 0 < r2["AP50"] < 100


def test_warmup_multistep_lr():
    assert warmup_multistep_lr(0, 0.02, (10, 20), 0.1, 5, 0.001) == pytest.approx(0.02 * 0.001)
    assert warmup_multistep_lr(5, 0.02, (10, 20), 0.1, 5, 0.001) == pytest.approx(0.02)
    assert warmup_multistep_lr(15, 0.02, (10, 20), 0.1, 5, 0.001) == pytest.approx(0.002)
    assert warmup_multistep_lr(25, 0.02, (10, 20), 0.1, 5, 0.001) == pytest.approx(0.0002)


def test_train_net_cli_checkpoint_resume(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "detection"))
    spec = importlib.util.spec_from_file_location("_det_train_net", os.path.join(ROOT, "detection", "train_net.py"))
    tn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tn)
    common = ["--config-file", os.path.join(CFGS, "DKD/DKD-R18-R101.yaml"),
              "SOLVER.IMS_PER_BATCH", "2", "RUNTIME.SYNTHETIC_SIZE", "(96,128)",
              "RUNTIME.SYNTHETIC_VAL_IMAGES", "2", "RUNTIME.LOG_PERIOD", "1",
              "MODEL.RPN.POST_NMS_TOPK_TRAIN", "100", "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", "32",
              "SOLVER.CHECKPOINT_PERIOD", "2", "OUTPUT_DIR", str(tmp_path)]
    assert tn.main(common + ["SOLVER.MAX_ITER", "2"]) == 0
    assert (tmp_path / "last_checkpoint").read_text().strip() == "model_0000001.pth"
    assert tn.main(["--resume"] + common + ["SOLVER.MAX_ITER", "3"]) == 0
    out = capsys.readouterr().out
    assert "iter 3/3" in out and "iter 1/3" not in out  # resumed after iteration 2
    assert "AP" in json.loads((tmp_path / "metrics.json").read_text())["bbox"]
