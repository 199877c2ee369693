"""Generate g25_retinaface.npz: outputs of the reference's own ``RetinaFace`` (swap_face_fine/gpen/face_detect/facemodels/retinaface.py), ``PriorBox``,
``decode``, ``decode_landm``, ``py_cpu_nms`` and ``RetinaFaceDetection.detect`` (retinaface_detection.py:61-131) in eval mode on the CPU, with the seeded weights
(``seeded.seeded_retinaface_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_retinaface.py [out.npz]

Only the build container has the reference tree.  What is wired (no reference source is copied):
  * ``torchvision`` is not installed: ``torchvision.models.resnet50`` and ``torchvision.models._utils.IntermediateLayerGetter`` are stubs that build the
    documented ResNet-50 v1.5 layer list and the documented getter (weights irrelevant: the seeded state_dict is loaded over them);
  * ``cv2`` is an empty module (``detect`` touches it only above 1500 pixels);
  * ``RetinaFaceDetection.__init__`` loads a checkpoint file: the object is made without it and given the network.
Per case of ``tests/retinaface_model.py``: the uint8 BGR input ``img``, the reference's float32 ``loc`` / ``conf`` / ``landms``, ``PriorBox``'s ``priors``, and
per image ``detect``'s ``dets`` and ``landms``.  ``keys.default``: the reference's ``state_dict`` key names and shapes for ``cfg_re50``, one ``name|d0xd1x...`` line
per key.  ``nms.*``: seeded box sets with ``py_cpu_nms``'s keep lists.  No weights are stored: the tests make them from the seed, and the seed of a case is the
first (0, 1, 2, ...) at which every image of the case meets ``retinaface_model.admission`` in float64; the script searches and asserts that
``retinaface_model.WEIGHT_SEEDS`` names it.  It asserts what tests/test_retinaface_cpu.py asserts."""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_shim as shim  # noqa: E402
import retinaface_model as RM  # noqa: E402


def _stub_torchvision():
    """torchvision's documented ResNet-50 (v1.5: the stride on the 3 x 3 convolution of a Bottleneck) and IntermediateLayerGetter."""
    class Bottleneck(nn.Module):
        def __init__(self, cin, width, stride, downsample):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width)
            self.conv2, self.bn2 = nn.Conv2d(width, width, 3, stride, 1, bias=False), nn.BatchNorm2d(width)
            self.conv3, self.bn3 = nn.Conv2d(width, width * 4, 1, bias=False), nn.BatchNorm2d(width * 4)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = downsample

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            return self.relu(out + (x if self.downsample is None else self.downsample(x)))

    class ResNet50(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
            self.relu, self.maxpool = nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)
            cin = 64
            for i, n in enumerate((3, 4, 6, 3)):
                width, stride = 64 << i, 1 if i == 0 else 2
                ds = nn.Sequential(nn.Conv2d(cin, width * 4, 1, stride, bias=False), nn.BatchNorm2d(width * 4))
                setattr(self, f"layer{i + 1}", nn.Sequential(Bottleneck(cin, width, stride, ds), *[Bottleneck(width * 4, width, 1, None) for _ in range(n - 1)]))
                cin = width * 4
            self.avgpool, self.fc = nn.AdaptiveAvgPool2d((1, 1)), nn.Linear(2048, 1000)

    class IntermediateLayerGetter(nn.ModuleDict):
        def __init__(self, model, return_layers):
            layers, left = {}, dict(return_layers)
            for name, module in model.named_children():
                layers[name] = module
                left.pop(name, None)
                if not left:
                    break
            super().__init__(layers)
            self.return_layers = dict(return_layers)

        def forward(self, x):
            out = {}
            for name, module in self.items():
                x = module(x)
                if name in self.return_layers:
                    out[self.return_layers[name]] = x
            return out

    tv = types.ModuleType("torchvision")
    names = ("torchvision.models", "torchvision.models._utils", "torchvision.models.detection", "torchvision.models.detection.backbone_utils",
             "torchvision.transforms")
    mods = {n: types.ModuleType(n) for n in names}
    tv.models, tv.transforms = mods["torchvision.models"], mods["torchvision.transforms"]
    tv.models._utils, tv.models.detection = mods["torchvision.models._utils"], mods["torchvision.models.detection"]
    tv.models.detection.backbone_utils = mods["torchvision.models.detection.backbone_utils"]
    tv.models.resnet50 = lambda pretrained=False, **kw: ResNet50()
    tv.models._utils.IntermediateLayerGetter = IntermediateLayerGetter
    sys.modules["torchvision"] = tv
    sys.modules.update(mods)


def key_lines(net):
    return "\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items())


def first_admissible_seed(tag):
    bs, H, W, c = RM.CASES[tag]
    x = RM.to_input(RM.case_image(tag))
    for seed in range(1000):
        loc, conf, lm = (t.numpy() for t in RM.network(RM.state_dict(tag, seed), x))
        if all(not RM.admission(loc[b], conf[b], lm[b], H, W) for b in range(bs)):
            return seed
    raise AssertionError(f"case {tag}: no admissible seed below 1000")


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    shim.install()
    _stub_torchvision()
    sys.modules["cv2"] = types.ModuleType("cv2")
    det_mod = importlib.import_module("swap_face_fine.gpen.face_detect.retinaface_detection")
    nms_mod = importlib.import_module("swap_face_fine.gpen.face_detect.utils.nms.py_cpu_nms")
    out = {}
    with torch.device("meta"):
        out["keys.default"] = np.array(key_lines(det_mod.RetinaFace(cfg=det_mod.cfg_re50, phase="test")))
    assert len(str(out["keys.default"]).split("\n")) == 456
    for tag, (bs, H, W, c) in RM.CASES.items():
        seed = first_admissible_seed(tag)
        assert seed == RM.WEIGHT_SEEDS[tag], (tag, seed, RM.WEIGHT_SEEDS[tag])
        k = RM.case(tag)
        cfg = dict(det_mod.cfg_re50, out_channel=c)
        net = det_mod.RetinaFace(cfg=cfg, phase="test").eval()
        net.load_state_dict(k["sd"], strict=True)
        loc, conf, landms = (t.numpy() for t in net(torch.from_numpy(k["x"])))
        errs = [RM.max_err(loc, k["loc64"]), RM.max_err(conf, k["conf64"]), RM.max_err(landms, k["landms64"])]
        assert errs[0] <= k["bar_loc"] and errs[1] <= k["bar_conf"] and errs[2] <= k["bar_landms"], (tag, errs)
        pr = det_mod.PriorBox(cfg, image_size=(H, W)).forward().numpy()
        assert pr.dtype == np.float32 and np.array_equal(pr, RM.priors(H, W))
        d = object.__new__(det_mod.RetinaFaceDetection)
        d.net, d.device, d.cfg = net, "cpu", cfg
        out[f"{tag}.img"], out[f"{tag}.loc"], out[f"{tag}.conf"], out[f"{tag}.landms"], out[f"{tag}.priors"] = k["img"], loc, conf, landms, pr
        for b in range(bs):
            assert not RM.admission(k["loc64"][b], k["conf64"][b], k["landms64"][b], H, W)
            dets, lm = d.detect(k["img"][b].copy())
            want = k["det"][b]
            dist = RM.detect_distance((dets, lm), (want["dets"], want["landms"]), k["bar_xy"], k["bar_conf"])
            assert dets.dtype == np.float32 and lm.dtype == np.float32 and dist <= 1.0, (tag, b, dist, len(dets), len(want["dets"]))
            out[f"{tag}.{b}.dets"], out[f"{tag}.{b}.landms"] = dets, lm
            print(f"  {tag}.{b}: seed {seed}, {k['N']} anchors, {len(want['cand'])} candidates, {len(dets)} kept, detect {dist:.2f} bars from the model; net "
                  f"{errs[0] / k['e32_loc']:.2f} / {errs[1] / k['e32_conf']:.2f} / {errs[2] / k['e32_landms']:.2f} e32, loc std {loc.std():.2f}")
    for name, (n, thresh) in RM.NMS_SETS.items():
        boxes, scores = RM.nms_box_set(name)
        keep = nms_mod.py_cpu_nms(np.hstack((boxes, scores[:, None])).astype(np.float32), thresh)
        assert [int(i) for i in keep] == RM.nms(boxes.astype(np.float64), thresh), name
        out[name + ".boxes"], out[name + ".scores"], out[name + ".keep"] = boxes, scores, np.asarray(keep, dtype=np.int64)
        print(f"  {name}: {len(boxes)} boxes, {len(keep)} kept at {thresh}")
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays")
    assert size < 750_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g25_retinaface.npz"))
