"""Row f14: GPEN face enhancement, stage 3 — the face detector, ``RetinaFaceDetection.detect`` of swap_face_fine/gpen/face_detect/retinaface_detection.py:61-131
with the ``RetinaFace`` of facemodels/retinaface.py (ResNet-50 body, ``FPN`` and ``SSH`` of facemodels/net.py, three head families; ``cfg_re50``, phase 'test'),
``PriorBox``, ``decode``, ``decode_landm`` and ``py_cpu_nms``, in eval mode on the device: ``retinaface_forward``, ``retinaface_detect``.
``FaceEnhancement.process`` runs it on every frame, at 4 x the frame's size.  Scope: the Resnet50 configuration with any ``out_channel`` (a multiple of 4), any
input up to 1500 on its longer side (beyond that the reference resizes with cv2, which is not done here), odd sizes included.

    the input          e4s_retina_input: uint8 [bs, H, W, 3] to the BGR planes of pixel - (104, 117, 123), exact
    body.conv1         e4s_conv2d (exact fp32, 7 x 7, stride 2, pad 3: three input channels) + folded BatchNorm + ReLU, then e4s_maxpool3x3s2
    a Bottleneck       1 x 1, 3 x 3 (the stride on it: ResNet v1.5), 1 x 1 on the split-bf16 kernels of conv.hip with BatchNorm folded in float64 and ReLU fused;
                       the last takes the identity, or the 1 x 1 stride-s ``downsample`` convolution's output, as ``residual``
    FPN                three 1 x 1 lateral convolutions, e4s_retina_up_add (nearest to the finer map's size + add, one pass), two 3 x 3 merges
    SSH                five 3 x 3 convolutions and e4s_retina_cat_relu (cat + ReLU for any batch, one pass)
    the heads          per level one 1 x 1 convolution with 32 outputs: BboxHead's 8, ClassHead's 4, LandmarkHead's 20 concatenated
    the tail           e4s_retina_decode (dense loc / softmax conf / landms, or priors + decode + decode_landm + scale), e4s_retina_compact (threshold, ordered
                       compaction into sort keys, top_k), torch.sort on the keys, e4s_retina_nms (gather + greedy NMS + keep_top_k + landmark reorder)

LeakyReLU(0) is the ReLU epilogue; the 0.1 slope of ``out_channel <= 64`` is the PReLU epilogue with a constant slope vector.  ``ARITH`` picks the convolutions'
arithmetic: ``"sb3"`` (three-way split bf16, fp32-class: the default) or ``"sb"`` (two-way).  The whole batch goes through each launch; no host synchronisation
before the one read of the kept counts at the end of ``retinaface_detect``; the same inputs give the same bits; after one eager call (which prepares the weights)
``retinaface_forward`` and ``retinaface_detect_padded`` capture in a graph."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import lib
from .lossnet import bn_fold, conv_exact, conv_sb, prep_exact, prep_fwd
from .ops import _p, _stream
from .netweights import EVAL_ONLY, PreparedNet, _Net, _image_checked, _placed_checked, _validated, bn_shapes, check_loaded, prepare

ARITH = "sb3"                                # "sb3": e4s_conv2d_sb3 (fp32-class); "sb": e4s_conv2d_sb (two-way split bf16)
RETINAFACE_MAX_SIDE = 1500                              # detect resizes a larger image with cv2 first (retinaface_detection.py:67-70): out of scope
MEAN_BGR = (104, 117, 123)
RESNET50_BLOCKS = (3, 4, 6, 3)
MAX_TOP_K = 16384                            # e4s_retina_compact / e4s_retina_nms: candidates per image

# data/config.py: cfg_re50, the values the eval-mode detector reads
RETINAFACE_CFG_RE50 = {"name": "Resnet50", "min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32], "variance": [0.1, 0.2], "clip": False, "pretrain": False,
            "return_layers": {"layer2": 1, "layer3": 2, "layer4": 3}, "in_channel": 256, "out_channel": 256}


# ------------------------------------------------------------------------------------------------ the module: the reference's keys, a stock-PyTorch forward
class _Bottleneck(nn.Module):
    """torchvision's ``Bottleneck`` (ResNet v1.5: the stride on the 3 x 3 convolution)."""

    def __init__(self, cin, width, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, width * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(width * 4)
        self.relu = nn.ReLU(inplace=True)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(cin, width * 4, 1, stride, bias=False), nn.BatchNorm2d(width * 4))

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (self.downsample(x) if hasattr(self, "downsample") else x))


class _Body(nn.Module):
    """``IntermediateLayerGetter(resnet50(), {'layer2': 1, 'layer3': 2, 'layer4': 3})``: the children up to layer4, no avgpool, no fc."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for i, n in enumerate(RESNET50_BLOCKS):
            width, stride = 64 << i, 1 if i == 0 else 2
            blocks = [_Bottleneck(cin, width, stride, True)] + [_Bottleneck(width * 4, width, 1, False) for _ in range(n - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
            cin = width * 4

    def forward(self, x):
        x = self.layer1(self.maxpool(self.relu(self.bn1(self.conv1(x)))))
        c2 = self.layer2(x)
        c3 = self.layer3(c2)
        return c2, c3, self.layer4(c3)


def _conv_bn(cin, cout, k, leaky=None):
    layers = [nn.Conv2d(cin, cout, k, 1, k // 2, bias=False), nn.BatchNorm2d(cout)]
    return nn.Sequential(*layers, *([] if leaky is None else [nn.LeakyReLU(negative_slope=leaky, inplace=True)]))


def _leaky(out_channel):
    return 0.1 if out_channel <= 64 else 0       # net.py:44-46, 71-73


class _FPN(nn.Module):
    def __init__(self, cins, c):
        super().__init__()
        lk = _leaky(c)
        self.output1, self.output2, self.output3 = (_conv_bn(ci, c, 1, lk) for ci in cins)
        self.merge1, self.merge2 = _conv_bn(c, c, 3, lk), _conv_bn(c, c, 3, lk)

    def forward(self, feats):
        o1, o2, o3 = self.output1(feats[0]), self.output2(feats[1]), self.output3(feats[2])
        o2 = self.merge2(o2 + F.interpolate(o3, size=[o2.size(2), o2.size(3)], mode="nearest"))
        o1 = self.merge1(o1 + F.interpolate(o2, size=[o1.size(2), o1.size(3)], mode="nearest"))
        return o1, o2, o3


class _SSH(nn.Module):
    def __init__(self, c):
        super().__init__()
        lk = _leaky(c)
        self.conv3X3 = _conv_bn(c, c // 2, 3)
        self.conv5X5_1 = _conv_bn(c, c // 4, 3, lk)
        self.conv5X5_2 = _conv_bn(c // 4, c // 4, 3)
        self.conv7X7_2 = _conv_bn(c // 4, c // 4, 3, lk)
        self.conv7x7_3 = _conv_bn(c // 4, c // 4, 3)

    def forward(self, x):
        a = self.conv3X3(x)
        t = self.conv5X5_1(x)
        return F.relu(torch.cat([a, self.conv5X5_2(t), self.conv7x7_3(self.conv7X7_2(t))], dim=1))


class _Head(nn.Module):
    def __init__(self, c, per_anchor):
        super().__init__()
        self.per_anchor = per_anchor
        self.conv1x1 = nn.Conv2d(c, 2 * per_anchor, 1)

    def forward(self, x):
        out = self.conv1x1(x).permute(0, 2, 3, 1).contiguous()
        return out.view(out.shape[0], -1, self.per_anchor)


def _checked_cfg(cfg, phase):
    cfg = dict(RETINAFACE_CFG_RE50) if cfg is None else cfg
    if cfg.get("name") != "Resnet50":
        raise ValueError(f"RetinaFace: cfg['name'] is {cfg.get('name')!r}: the native detector is the 'Resnet50' configuration (cfg_re50)")
    if phase != "test":
        raise ValueError(f"RetinaFace: phase {phase!r} is not implemented: the native detector is phase='test' (eval mode, softmax scores)")
    c, cin = cfg.get("out_channel", 256), cfg.get("in_channel", 256)
    if not isinstance(c, int) or c < 4 or c % 4 or cin != 256:
        raise ValueError(f"RetinaFace: out_channel {c!r} must be a positive multiple of 4 and in_channel {cin!r} must be 256 (ResNet-50)")
    return cfg, c


class RetinaFace(nn.Module):
    """``RetinaFace(cfg, phase)`` of swap_face_fine/gpen/face_detect/facemodels/retinaface.py for ``cfg_re50`` (the default) and ``phase='test'``, with its
    ``state_dict`` keys, shapes and order: ``RetinaFace-R50.pth`` with its ``module.`` prefix stripped loads with ``strict=True``.  ``forward`` is the plain
    PyTorch composition in eval mode, ``(loc [bs, N, 4], softmax conf [bs, N, 2], landms [bs, N, 10])`` — what the tests and the timing compare with;
    ``retinaface_forward(x, module)`` runs the same weights on the HIP kernels.  It starts with random weights and the native entries refuse it until
    ``load_state_dict`` has filled it."""

    def __init__(self, cfg=None, phase="test"):
        super().__init__()
        self.cfg, c = _checked_cfg(cfg, phase)
        self.phase, self.out_channel = phase, c
        self.body = _Body()
        self.fpn = _FPN((512, 1024, 2048), c)
        self.ssh1, self.ssh2, self.ssh3 = _SSH(c), _SSH(c), _SSH(c)
        self.ClassHead = nn.ModuleList(_Head(c, 2) for _ in range(3))
        self.BboxHead = nn.ModuleList(_Head(c, 4) for _ in range(3))
        self.LandmarkHead = nn.ModuleList(_Head(c, 10) for _ in range(3))
        self.requires_grad_(False)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if "body.conv1.weight" in state_dict and "ClassHead.0.conv1x1.weight" in state_dict:
            self._loaded = True
        return out

    def forward(self, inputs):
        if self.training:
            raise NotImplementedError("RetinaFace: training mode is not implemented; call .eval()")
        with torch.no_grad():
            fpn = self.fpn(self.body(inputs))
            feats = [self.ssh1(fpn[0]), self.ssh2(fpn[1]), self.ssh3(fpn[2])]
            loc = torch.cat([self.BboxHead[i](f) for i, f in enumerate(feats)], dim=1)
            cls = torch.cat([self.ClassHead[i](f) for i, f in enumerate(feats)], dim=1)
            ldm = torch.cat([self.LandmarkHead[i](f) for i, f in enumerate(feats)], dim=1)
            return loc, F.softmax(cls, dim=-1), ldm


# ------------------------------------------------------------------------------------------------ weights
def _bottlenecks():
    """[(key prefix, cin, width, stride, has a downsample convolution)] of the ResNet-50 body in key order."""
    out, cin = [], 64
    for i, n in enumerate(RESNET50_BLOCKS):
        width = 64 << i
        for j in range(n):
            out.append((f"body.layer{i + 1}.{j}", cin, width, 2 if (i > 0 and j == 0) else 1, j == 0))
            cin = width * 4
    return out


def _seqs(c):
    """[(key prefix of a conv + BatchNorm pair, cin, cout, k, has an activation)] behind the body, in key order."""
    out = [(f"fpn.output{i + 1}", ci, c, 1, True) for i, ci in enumerate((512, 1024, 2048))] + [("fpn.merge1", c, c, 3, True), ("fpn.merge2", c, c, 3, True)]
    for s in ("ssh1", "ssh2", "ssh3"):
        out += [(f"{s}.conv3X3", c, c // 2, 3, False), (f"{s}.conv5X5_1", c, c // 4, 3, True), (f"{s}.conv5X5_2", c // 4, c // 4, 3, False),
                (f"{s}.conv7X7_2", c // 4, c // 4, 3, True), (f"{s}.conv7x7_3", c // 4, c // 4, 3, False)]
    return out


_HEADS = (("ClassHead", 4), ("BboxHead", 8), ("LandmarkHead", 20))


def retinaface_state_dict_shapes(out_channel: int = 256):
    """``{key: shape}`` of ``RetinaFace(cfg_re50 with that out_channel, 'test').state_dict()``, in its order."""
    c, out = int(out_channel), {}
    out["body.conv1.weight"] = (64, 3, 7, 7)
    bn_shapes(out, "body.bn1", 64)
    for p, cin, width, _, ds in _bottlenecks():
        for i, (ci, co, k) in enumerate(((cin, width, 1), (width, width, 3), (width, width * 4, 1))):
            out[f"{p}.conv{i + 1}.weight"] = (co, ci, k, k)
            bn_shapes(out, f"{p}.bn{i + 1}", co)
        if ds:
            out[p + ".downsample.0.weight"] = (width * 4, cin, 1, 1)
            bn_shapes(out, p + ".downsample.1", width * 4)
    for p, ci, co, k, _ in _seqs(c):
        out[p + ".0.weight"] = (co, ci, k, k)
        bn_shapes(out, p + ".1", co)
    for name, n in _HEADS:
        for i in range(3):
            out[f"{name}.{i}.conv1x1.weight"] = (n, c, 1, 1)
            out[f"{name}.{i}.conv1x1.bias"] = (n,)
    return out


def _variant_of_keys(name, sd):
    t = sd.get("fpn.output1.0.weight")
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise KeyError(f"{name}: the weights lack 'fpn.output1.0.weight': expected the keys of RetinaFace (ops.retinaface_state_dict_shapes())")
    return int(t.shape[0])


_RETINA_NET = _Net("RetinaFace", retinaface_state_dict_shapes, ("module.",), False, ("body.conv1.weight",), _variant_of_keys, EVAL_ONLY,
                   ("num_batches_tracked",))


def retinaface_weight_tensors(weights, name: str = "retinaface_forward"):
    """The float tensors of the network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _RETINA_NET)[2]


class PreparedRetinaFace(PreparedNet):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage or ``ARITH`` changes.  ``stem``: body.conv1 with bn1
    folded, K-major fp32 ``[3][49][64]`` and bias; per Bottleneck the slabs and biases of its three (four) convolutions with their BatchNorms folded in
    float64; the FPN's and the SSHs' the same way; ``heads``: per level the Bbox, Class and Landmark 1 x 1 convolutions as one with 32 outputs; ``slope``: the
    constant slope vectors of the leaky configuration (``out_channel <= 64``), else None."""

    __slots__ = ()
    _entry, _net = "retinaface_forward", _RETINA_NET

    def _settings(self):
        return (ARITH,)

    def _build(self, sd, c, dev):
        if ARITH not in ("sb3", "sb"):
            raise ValueError(f"ops_retinaface.ARITH is {ARITH!r}: 'sb3' or 'sb'")
        terms = 3 if ARITH == "sb3" else 2

        def normed(conv, bn):
            return prep_fwd(sd[conv + ".weight"], *bn_fold(sd, bn), terms=terms)

        blocks = [dict(stride=stride, c1=normed(p + ".conv1", p + ".bn1"), c2=normed(p + ".conv2", p + ".bn2"), c3=normed(p + ".conv3", p + ".bn3"),
                       ds=normed(p + ".downsample.0", p + ".downsample.1") if ds else None) for p, _, _, stride, ds in _bottlenecks()]
        seq = {p: normed(p + ".0", p + ".1") for p, *_ in _seqs(c)}
        heads = []
        for i in range(3):
            w = torch.cat([sd[f"{n}.{i}.conv1x1.weight"] for n in ("BboxHead", "ClassHead", "LandmarkHead")])
            bias = torch.cat([sd[f"{n}.{i}.conv1x1.bias"] for n in ("BboxHead", "ClassHead", "LandmarkHead")])
            heads.append(prep_fwd(w, None, bias.double(), terms=terms))
        lk = _leaky(c)
        slope = {n: torch.full((n,), lk, dtype=torch.float32, device=dev) for n in (c, c // 4)} if lk else None
        return dict(c=c, stem=prep_exact(sd["body.conv1.weight"], *bn_fold(sd, "body.bn1")), blocks=blocks, seq=seq, heads=heads, slope=slope)


# ------------------------------------------------------------------------------------------------ the forward pass
def retinaface_level_sizes(H: int, W: int):
    """[(h, w)] of the three levels, ``PriorBox``'s ceil(H / step), and the number of anchors."""
    sizes = [(-(-H // s), -(-W // s)) for s in (8, 16, 32)]
    return sizes, 2 * sum(h * w for h, w in sizes)


def _up_add(a, b):
    bs, c, h, w = a.shape
    out = torch.empty_like(a)
    lib().call("e4s_retina_up_add", _p(out), _p(a), _p(b), bs * c, h, w, b.shape[2], b.shape[3], _stream())
    return out


def _heads(P, x):
    """The three levels' 32-channel head maps of a float ``x [bs, 3, H, W]`` (mean subtracted, BGR planes)."""
    bs, dev = x.shape[0], x.device
    cur = conv_exact(x, *P["stem"], k=7, stride=2, relu=True)
    ho, wo = cur.shape[2:]
    pooled = torch.empty((bs, 64, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1), dtype=torch.float32, device=dev)
    lib().call("e4s_maxpool3x3s2", _p(pooled), _p(cur), bs * 64, ho, wo, _stream())
    cur, taps = pooled, []
    for i, L in enumerate(P["blocks"]):
        o = conv_sb(cur, *L["c1"], k=1, relu=True)
        o = conv_sb(o, *L["c2"], k=3, stride=L["stride"], relu=True)
        idn = conv_sb(cur, *L["ds"], k=1, stride=L["stride"]) if L["ds"] is not None else cur
        cur = conv_sb(o, *L["c3"], k=1, residual=idn, relu=True)
        if i + 1 in (7, 13, 16):                         # the ends of layer2, layer3, layer4
            taps.append(cur)
    seq, c = P["seq"], P["c"]

    def act(p, t, k, n=c, on=True):
        """conv + folded BatchNorm (+ LeakyReLU: ReLU at slope 0, the PReLU epilogue otherwise)."""
        if not on:
            return conv_sb(t, *seq[p], k=k)
        return conv_sb(t, *seq[p], k=k, relu=True) if P["slope"] is None else conv_sb(t, *seq[p], k=k, slope=P["slope"][n])

    o1, o2, o3 = (act(f"fpn.output{i + 1}", t, 1) for i, t in enumerate(taps))
    o2 = act("fpn.merge2", _up_add(o2, o3), 3)
    o1 = act("fpn.merge1", _up_add(o1, o2), 3)
    out = []
    for i, f in enumerate((o1, o2, o3)):
        s = f"ssh{i + 1}"
        a = act(s + ".conv3X3", f, 3, on=False)
        t = act(s + ".conv5X5_1", f, 3, c // 4)
        b5 = act(s + ".conv5X5_2", t, 3, on=False)
        b7 = act(s + ".conv7x7_3", act(s + ".conv7X7_2", t, 3, c // 4), 3, on=False)
        h, w = f.shape[2:]
        cat = torch.empty((bs, c, h, w), dtype=torch.float32, device=dev)
        lib().call("e4s_retina_cat_relu", _p(cat), _p(a), _p(b5), _p(b7), bs, c // 2, c // 4, c // 4, h * w, _stream())
        out.append(conv_sb(cat, *P["heads"][i], k=1))
    return out


def _decode(heads, H, W, dense: bool, decoded: bool):
    """``e4s_retina_decode``: (loc, conf, landms) and / or (score, boxes, lmk)."""
    bs, dev = heads[0].shape[0], heads[0].device
    N = retinaface_level_sizes(H, W)[1]
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)          # noqa: E731
    d = (new(bs, N, 4), new(bs, N, 2), new(bs, N, 10)) if dense else (None, None, None)
    e = (new(bs, N), new(bs, N, 4), new(bs, N, 10)) if decoded else (None, None, None)
    lib().call("e4s_retina_decode", *[_p(t) for t in d + e], _p(heads[0]), _p(heads[1]), _p(heads[2]), bs, H, W, _stream())
    return d, e


def retinaface_priors(H: int, W: int, device) -> torch.Tensor:
    """``PriorBox(cfg_re50, image_size=(H, W)).forward()`` on the device: float32 ``[N, 4]`` of (cx, cy, s_kx, s_ky), bit for bit."""
    out = torch.empty((retinaface_level_sizes(int(H), int(W))[1], 4), dtype=torch.float32, device=device)
    lib().call("e4s_retina_priors", _p(out), int(H), int(W), _stream())
    return out


def retinaface_detection_tail(score, boxes, lmk, confidence_threshold=0.9, nms_threshold=0.4, top_k=5000, keep_top_k=750):
    """Everything of ``detect`` behind the decoded anchors, for ``score [bs, N]``, ``boxes [bs, N, 4]``, ``lmk [bs, N, 10]`` on the device: threshold, ordered
    compaction, top_k, the sort by score, ``py_cpu_nms``, keep_top_k and the landmark reorder.  Returns ``(dets [bs, keep_top_k, 5], landms [bs, keep_top_k, 10],
    keep [bs, keep_top_k] int32, nkeep [bs] int32, counts [bs, 2] int32)``; rows behind ``nkeep`` are zero.  No host synchronisation."""
    bs, N = score.shape
    if not (1 <= int(top_k) <= MAX_TOP_K) or int(keep_top_k) < 1:
        raise ValueError(f"retinaface_detection_tail: top_k must be 1 .. {MAX_TOP_K} and keep_top_k at least 1, got {top_k} and {keep_top_k}")
    dev, cap, keep_n = score.device, int(top_k), int(keep_top_k)
    keys = torch.empty((bs, cap), dtype=torch.int64, device=dev)
    counts = torch.empty((bs, 2), dtype=torch.int32, device=dev)
    lib().call("e4s_retina_compact", _p(keys), _p(counts), _p(score), bs, N, cap, float(confidence_threshold), _stream())
    keys = torch.sort(keys, dim=1, descending=True)[0].contiguous()
    dets = torch.zeros((bs, keep_n, 5), dtype=torch.float32, device=dev)
    landms = torch.zeros((bs, keep_n, 10), dtype=torch.float32, device=dev)
    keep = torch.zeros((bs, keep_n), dtype=torch.int32, device=dev)
    nkeep = torch.empty((bs,), dtype=torch.int32, device=dev)
    cbox = torch.empty((bs, cap, 4), dtype=torch.float32, device=dev)
    lib().call("e4s_retina_nms", _p(dets), _p(landms), _p(keep), _p(nkeep), _p(cbox), _p(keys), _p(counts), _p(boxes), _p(lmk), bs, N, cap, keep_n,
               float(nms_threshold), _stream())
    return dets, landms, keep, nkeep, counts


def _checked_all(name, weights, x=None, img_u8=None):
    """Everything that can be refused, before any launch: the checked weights."""
    check_loaded(name, weights, "the RetinaFace weights")
    checked = _validated(name, weights, _RETINA_NET)
    t, nm, H, W, c = _image_checked(name, x, img_u8, "a float32 [bs, 3, H, W] image", "a uint8 [bs, H, W, 3] image")
    if c != 3:
        raise ValueError(f"{name}: {nm} is {tuple(t.shape)}: expected three colour channels")
    if min(H, W) < 1:
        raise ValueError(f"{name}: {nm} is {tuple(t.shape)}: an empty image")
    if max(H, W) > RETINAFACE_MAX_SIDE:
        raise ValueError(f"{name}: {nm} is {H} x {W}: the longer side is limited to {RETINAFACE_MAX_SIDE} (beyond it the reference resizes the image first, which is "
                         "not done here)")
    _placed_checked(name, nm, t, checked[2])
    return checked


def retinaface_forward(x: torch.Tensor, net):
    """``RetinaFace.forward(x)`` in test phase on the device: ``(loc [bs, N, 4], conf [bs, N, 2] softmax, landms [bs, N, 10])`` from a float32
    ``x [bs, 3, H, W]`` (BGR planes, mean subtracted), ``N = 2 sum ceil(H / s) ceil(W / s)`` over s = 8, 16, 32.  ``net``: a module with the network's keys
    (``RetinaFace``, the drop-in) or the mapping ``torch.load`` returns (a ``module.`` prefix is stripped).  A module's prepared weights are cached per parameter
    version; a mapping is prepared on every call.  Every argument is checked before any launch."""
    name = "retinaface_forward"
    checked = _checked_all(name, net, x=x)
    H, W = int(x.shape[2]), int(x.shape[3])
    if x.shape[0] == 0:
        N = retinaface_level_sizes(H, W)[1]
        return x.new_empty((0, N, 4)), x.new_empty((0, N, 2)), x.new_empty((0, N, 10))
    with torch.no_grad():
        P = prepare(PreparedRetinaFace, net, checked)
        return _decode(_heads(P, x.detach().contiguous()), H, W, True, False)[0]


def retinaface_detect_padded(img_u8: torch.Tensor, net, bgr: bool = True, confidence_threshold: float = 0.9, nms_threshold: float = 0.4, top_k: int = 5000,
                             keep_top_k: int = 750):
    """``retinaface_detect`` without its read of the counts: ``(dets [bs, keep_top_k, 5], landms [bs, keep_top_k, 10], nkeep [bs] int32)`` on the device, rows
    behind ``nkeep`` zero.  No host synchronisation: this is the form that captures in a graph."""
    name = "retinaface_detect"
    if not (1 <= int(top_k) <= MAX_TOP_K) or int(keep_top_k) < 1:
        raise ValueError(f"{name}: top_k must be 1 .. {MAX_TOP_K} and keep_top_k at least 1, got {top_k} and {keep_top_k}")
    checked = _checked_all(name, net, img_u8=img_u8)
    bs, H, W = (int(v) for v in img_u8.shape[:3])
    dev = img_u8.device
    if bs == 0:
        return (torch.zeros((0, keep_top_k, 5), device=dev), torch.zeros((0, keep_top_k, 10), device=dev), torch.zeros((0,), dtype=torch.int32, device=dev))
    with torch.no_grad():
        P = prepare(PreparedRetinaFace, net, checked)
        x = torch.empty((bs, 3, H, W), dtype=torch.float32, device=dev)
        lib().call("e4s_retina_input", _p(x), _p(img_u8.contiguous()), 1 if bgr else 0, bs, H, W, _stream())
        score, boxes, lmk = _decode(_heads(P, x), H, W, False, True)[1]
        dets, landms, _, nkeep, _ = retinaface_detection_tail(score, boxes, lmk, confidence_threshold, nms_threshold, top_k, keep_top_k)
    return dets, landms, nkeep


def retinaface_detect(img_u8: torch.Tensor, net, bgr: bool = True, confidence_threshold: float = 0.9, nms_threshold: float = 0.4, top_k: int = 5000,
                      keep_top_k: int = 750):
    """``RetinaFaceDetection.detect`` (retinaface_detection.py:61-131, ``resize=1``) for a batch on the device: uint8 ``[bs, H, W, 3]`` images (BGR as the
    reference takes them, or RGB with ``bgr=False``) to a list of ``(dets [n, 5] float32: x1, y1, x2, y2, score; landms [n, 10] float32: x0..x4, y0..y4)`` per
    image, on the device, in ``detect``'s order (score descending).  One device-to-host read, of the kept counts, at the end.  Image ``i`` of a batch gives the
    bits of the single-image call.  ``max(H, W) > 1500`` raises ``ValueError``: the reference resizes such an image with cv2 first."""
    dets, landms, nkeep = retinaface_detect_padded(img_u8, net, bgr, confidence_threshold, nms_threshold, top_k, keep_top_k)
    return [(dets[b, :n], landms[b, :n]) for b, n in enumerate(nkeep.tolist())]


__all__ = ["RetinaFace", "PreparedRetinaFace", "RETINAFACE_CFG_RE50", "RETINAFACE_MAX_SIDE", "retinaface_state_dict_shapes", "retinaface_weight_tensors", "retinaface_level_sizes",
           "retinaface_priors", "retinaface_detection_tail", "retinaface_forward", "retinaface_detect_padded", "retinaface_detect"]
