"""Row f21: CodeFormer face restoration, stage 1 — everything in ``CodeFormer.forward`` (swap_face_fine/archs/codeformer_arch.py:219-262) up to ``quant_feat``,
eval mode, forward only, float32 NCHW on the device: the VQGAN encoder with its four taps, the 9-layer transformer, the logits head, the top-1 codes, the
codebook lookup and the AdaIN.  The VQGAN generator with its ``Fuse_sft_block``s is stage 2 (row f22, ``ops_codeformer_gen``): ``CodeFormer`` below constructs
and loads it, nothing in this module runs it natively.

    conv_in                 3 channels: the exact e4s_conv2d
    GroupNorm(32, 1e-6)     e4s_cf_group_stats over the bs 32 contiguous runs of a group (one block per 16384 floats, the pieces merged in float64), then
                            e4s_cf_group_norm (swish fused; plain for AttnBlock.norm and the encoder's last norm)
    a ResBlock              norm1 + swish, conv1, norm2 + swish, conv2 with ``x_in`` (or conv_out(x_in), a 1 x 1) as its residual: e4s_conv2d_sb3
    Downsample              e4s_cf_pad_rb (right and bottom only), then the 3 x 3 stride-2 convolution with pad 0
    an AttnBlock            norm, q | k | v as ONE 1 x 1 convolution with cout 3 C, e4s_cf_attention (1 head, d = C, scale C^-0.5), proj_out with x as residual
    the transformer         channel-major [bs, E, h, w] throughout (tokens innermost, as NCHW has them): feat_emb, the in-projection (q | k as one convolution on
                            norm1(x) + pos, v on norm1(x)), out_proj, linear1, linear2 are 1 x 1 convolutions on e4s_conv2d_sb3 with the residual adds folded;
                            e4s_cf_layer_norm (with the ``+ pos`` second output), e4s_cf_attention (n_head heads), e4s_cf_gelu
    the head                e4s_cf_layer_norm, then Linear(E, codebook) without bias as a 1 x 1 on the exact e4s_conv2d (its argmax decides the output);
                            e4s_cf_argmax (the softmax in front of topk is monotone and not computed), e4s_cf_quant (gather + AdaIN)

No host synchronisation; the same inputs give the same bits, a sample of a batch the bits it gets alone; after one eager call (which prepares the weights) a
call captures in a graph.  Every argument is checked before any launch."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import lib
from .lossnet import conv_exact, conv_sb, prep_exact, prep_fwd
from .netweights import PreparedNet, _Net, _cuda_checked, _devices_checked, _keys_shapes, _tensor_checked, _validated, module_net, prepare
from .ops import _p, _stream

CF_NF, CF_CH_MULT, CF_EMB = 64, (1, 2, 2, 4, 4, 8), 256           # the parent VQAutoEncoder's fixed arguments (codeformer_arch.py:166)
CF_GROUPS, CF_GN_EPS, CF_LN_EPS, CF_ADAIN_EPS = 32, 1e-6, 1e-5, 1e-5
CF_MAX_TOKENS, CF_MAX_HEAD = 1024, 512
CF_GN_CHUNK = 16384                                                # floats of a group's run per statistics block
CF_CONNECT = ("32", "64", "128", "256")
CF_TAP_BLOCKS = {"32": 14, "64": 11, "128": 8, "256": 5}           # fuse_encoder_block: the tap is the output of that encoder block
CF_CHANNELS = {"16": 512, "32": 256, "64": 256, "128": 128, "256": 128, "512": 64}
_PREFIXES = ("params_ema.", "params.", "module.")


def _plan(decoder: bool):
    """The block list of the VQGAN ``Encoder`` / ``Generator`` at (nf 64, ch_mult (1, 2, 2, 4, 4, 8), two ResBlocks per level, attention at the sixth level) as
    (kind, cin, cout) tuples, in ``blocks`` order."""
    chans = [CF_NF * m for m in CF_CH_MULT]
    if not decoder:
        out, cin = [("conv", 3, CF_NF)], CF_NF
        for i, c in enumerate(chans):
            for _ in range(2):
                out.append(("res", cin, c))
                cin = c
                if i == len(chans) - 1:
                    out.append(("attn", c, c))
            if i != len(chans) - 1:
                out.append(("down", c, c))
        return out + [("res", cin, cin), ("attn", cin, cin), ("res", cin, cin), ("norm", cin, cin), ("conv", cin, CF_EMB)]
    cin = chans[-1]
    out = [("conv", CF_EMB, cin), ("res", cin, cin), ("attn", cin, cin), ("res", cin, cin)]
    for i in reversed(range(len(chans))):
        for _ in range(2):
            out.append(("res", cin, chans[i]))
            cin = chans[i]
            if i == len(chans) - 1:
                out.append(("attn", cin, cin))
        if i != 0:
            out.append(("up", cin, cin))
    return out + [("norm", cin, cin), ("conv", cin, 3)]


ENCODER_PLAN = tuple(_plan(False))


# ------------------------------------------------------------------------------------------------ the mirror module
def _gn(c):
    return nn.GroupNorm(CF_GROUPS, c, eps=CF_GN_EPS, affine=True)


def _swish(x):
    return x * torch.sigmoid(x)


class _ResBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm1, self.conv1 = _gn(cin), nn.Conv2d(cin, cout, 3, 1, 1)
        self.norm2, self.conv2 = _gn(cout), nn.Conv2d(cout, cout, 3, 1, 1)
        if cin != cout:
            self.conv_out = nn.Conv2d(cin, cout, 1)

    def forward(self, x_in):
        x = self.conv1(_swish(self.norm1(x_in)))
        x = self.conv2(_swish(self.norm2(x)))
        return x + (self.conv_out(x_in) if hasattr(self, "conv_out") else x_in)


class _AttnBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.norm = _gn(c)
        self.q, self.k, self.v, self.proj_out = (nn.Conv2d(c, c, 1) for _ in range(4))

    def forward(self, x):
        h = self.norm(x)
        b, c, hh, ww = h.shape
        q, k, v = (m(h).reshape(b, c, hh * ww) for m in (self.q, self.k, self.v))
        w = F.softmax(torch.bmm(q.permute(0, 2, 1), k) * (int(c) ** (-0.5)), dim=2)
        return x + self.proj_out(torch.bmm(v, w.permute(0, 2, 1)).reshape(b, c, hh, ww))


class _Downsample(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class _Upsample(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 1, 1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


def _block(kind, cin, cout):
    return {"conv": lambda: nn.Conv2d(cin, cout, 3, 1, 1), "res": lambda: _ResBlock(cin, cout), "attn": lambda: _AttnBlock(cin), "down": lambda: _Downsample(cin),
            "up": lambda: _Upsample(cin), "norm": lambda: _gn(cin)}[kind]()


class _Blocks(nn.Module):
    def __init__(self, decoder):
        super().__init__()
        self.blocks = nn.ModuleList([_block(*b) for b in _plan(decoder)])

    def forward(self, x):
        for block in self.blocks:
            x = block(x)
        return x


class _Quantizer(nn.Module):
    def __init__(self, codebook_size, emb_dim):
        super().__init__()
        self.embedding = nn.Embedding(codebook_size, emb_dim)


class _SALayer(nn.Module):
    def __init__(self, dim, n_head, dim_mlp):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(dim, n_head, dropout=0.0)
        self.linear1, self.linear2 = nn.Linear(dim, dim_mlp), nn.Linear(dim_mlp, dim)
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)

    def forward(self, tgt, query_pos=None):
        n = self.norm1(tgt)
        qk = n if query_pos is None else n + query_pos
        tgt = tgt + self.self_attn(qk, qk, value=n)[0]
        return tgt + self.linear2(F.gelu(self.linear1(self.norm2(tgt))))


class _FuseSft(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.encode_enc = _ResBlock(2 * c, c)
        self.scale = nn.Sequential(nn.Conv2d(c, c, 3, padding=1), nn.LeakyReLU(0.2, True), nn.Conv2d(c, c, 3, padding=1))
        self.shift = nn.Sequential(nn.Conv2d(c, c, 3, padding=1), nn.LeakyReLU(0.2, True), nn.Conv2d(c, c, 3, padding=1))

    def forward(self, enc_feat, dec_feat, w=1):
        enc_feat = self.encode_enc(torch.cat([enc_feat, dec_feat], dim=1))
        return dec_feat + w * (dec_feat * self.scale(enc_feat) + self.shift(enc_feat))


def _config_checked(name, dim_embd, n_head, n_layers, codebook_size, latent_size, connect_list, quantizer="nearest"):
    """The configuration as a hashable tuple; refused by name: a gumbel quantizer, sizes that are no positive ints, ``dim_embd`` not divisible by ``n_head``, a head
    width the attention kernel refuses, more tokens than it takes, a ``connect_list`` entry outside the four."""
    if quantizer != "nearest":
        raise NotImplementedError(f"{name}: quantizer={quantizer!r}: the native path is the nearest-code quantizer the caller builds; 'gumbel' is not offered")
    for nm, v in (("dim_embd", dim_embd), ("n_head", n_head), ("n_layers", n_layers), ("codebook_size", codebook_size), ("latent_size", latent_size)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name}: {nm} is a positive int, got {v!r}")
    if dim_embd % n_head:
        raise ValueError(f"{name}: dim_embd {dim_embd} is not divisible by n_head {n_head}")
    d = dim_embd // n_head
    if d % 16 or d > CF_MAX_HEAD or dim_embd > 512:
        raise ValueError(f"{name}: head width dim_embd / n_head = {d}: the attention kernel takes a multiple of 16 up to {CF_MAX_HEAD} (and dim_embd up to 512)")
    if latent_size > CF_MAX_TOKENS:
        raise ValueError(f"{name}: latent_size {latent_size}: at most {CF_MAX_TOKENS} tokens")
    connect = tuple(connect_list)
    for s in connect:
        if s not in CF_CONNECT:
            raise ValueError(f"{name}: connect_list entry {s!r} is not one of {list(CF_CONNECT)}")
    return dim_embd, n_head, n_layers, codebook_size, latent_size, connect


class CodeFormer(nn.Module):
    """``CodeFormer`` of swap_face_fine/archs/codeformer_arch.py with its constructor arguments and ``state_dict`` layout (``codeformer.pth['params_ema']`` loads
    with ``strict=True``), without basicsr.  ``front`` is the plain PyTorch composition of everything up to ``quant_feat`` — what the tests and the timing
    compare ``codeformer_front`` with; ``forward`` goes on through the generator as the reference does, in stock PyTorch too (what the tests and the timing compare
``ops_codeformer_gen.codeformer_restore`` with), choosing the fuse blocks by block index so that it runs at any size."""

    def __init__(self, dim_embd=512, n_head=8, n_layers=9, codebook_size=1024, latent_size=256, connect_list=("32", "64", "128", "256"),
                 fix_modules=("quantize", "generator"), quantizer="nearest"):
        super().__init__()
        self.config = _config_checked("CodeFormer", dim_embd, n_head, n_layers, codebook_size, latent_size, connect_list, quantizer)
        self.connect_list, self.n_layers, self.dim_embd, self.dim_mlp, self.n_head = list(connect_list), n_layers, dim_embd, dim_embd * 2, n_head
        self.codebook_size, self.latent_size = codebook_size, latent_size
        self.position_emb = nn.Parameter(torch.zeros(latent_size, dim_embd))
        self.encoder = _Blocks(False)
        self.quantize = _Quantizer(codebook_size, CF_EMB)
        self.generator = _Blocks(True)
        self.feat_emb = nn.Linear(CF_EMB, dim_embd)
        self.ft_layers = nn.Sequential(*[_SALayer(dim_embd, n_head, self.dim_mlp) for _ in range(n_layers)])
        self.idx_pred_layer = nn.Sequential(nn.LayerNorm(dim_embd), nn.Linear(dim_embd, codebook_size, bias=False))
        self.fuse_convs_dict = nn.ModuleDict({s: _FuseSft(CF_CHANNELS[s]) for s in self.connect_list})
        self.fuse_generator_block = {"16": 6, "32": 9, "64": 12, "128": 15, "256": 18, "512": 21}
        for m in fix_modules or ():
            for p in getattr(self, m).parameters():
                p.requires_grad = False

    def front(self, x, adain=True):
        """dict(quant_feat, logits, lq_feat, idx, taps) of ``x [n, 3, H, W]`` in stock PyTorch: the reference's arithmetic with the latent's own shape in place
        of the hard-coded ``[b, 16, 16, 256]``."""
        taps, by_block = {}, {b: s for s, b in CF_TAP_BLOCKS.items() if s in self.connect_list}
        for i, block in enumerate(self.encoder.blocks):
            x = block(x)
            if i in by_block:
                taps[by_block[i]] = x.clone()
        lq_feat = x
        n, c, h, w = lq_feat.shape
        pos = self.position_emb.unsqueeze(1).repeat(1, n, 1)
        q = self.feat_emb(lq_feat.flatten(2).permute(2, 0, 1))
        for layer in self.ft_layers:
            q = layer(q, query_pos=pos)
        logits = self.idx_pred_layer(q).permute(1, 0, 2)
        idx = torch.topk(F.softmax(logits, dim=2), 1, dim=2)[1][..., 0]
        quant = self.quantize.embedding.weight[idx.reshape(-1)].view(n, h, w, c).permute(0, 3, 1, 2).contiguous()
        if adain:
            quant = adain_reference(quant, lq_feat)
        return dict(quant_feat=quant, logits=logits, lq_feat=lq_feat, idx=idx, taps=taps)

    def forward(self, x, w=0, detach_16=True, code_only=False, adain=False):
        f = self.front(x, adain)
        if code_only:
            return f["logits"], f["lq_feat"]
        x = f["quant_feat"].detach() if detach_16 else f["quant_feat"]
        fuse = {self.fuse_generator_block[s]: s for s in self.connect_list}
        for i, block in enumerate(self.generator.blocks):
            x = block(x)
            if i in fuse and w > 0:
                x = self.fuse_convs_dict[fuse[i]](f["taps"][fuse[i]].detach(), x, w)
        return x, f["logits"], f["lq_feat"]


def adain_reference(content, style, eps=CF_ADAIN_EPS):
    """``adaptive_instance_normalization`` (codeformer_arch.py:12-43) in stock PyTorch: unbiased variance, eps added to it inside the square root."""
    b, c = content.shape[:2]
    stat = lambda t: (t.reshape(b, c, -1).mean(2).view(b, c, 1, 1), (t.reshape(b, c, -1).var(2) + eps).sqrt().view(b, c, 1, 1))  # noqa: E731
    (sm, ss), (cm, cs) = stat(style), stat(content)
    return (content - cm) / cs * ss + sm


def codeformer_state_dict_shapes(dim_embd=512, n_head=8, n_layers=9, codebook_size=1024, latent_size=256, connect_list=CF_CONNECT):
    """``{key: shape}`` of ``CodeFormer(...).state_dict()``, in its order."""
    cfg = _config_checked("codeformer_state_dict_shapes", dim_embd, n_head, n_layers, codebook_size, latent_size, connect_list)
    return dict(_keys_shapes(CodeFormer, *cfg))


def _cf_shapes(variant):
    return codeformer_state_dict_shapes(*variant)


def _cf_variant(name, sd):
    """The configuration read off a mapping's keys and shapes; the head count is not in them: 8, as the caller builds it (a module states its own)."""
    for probe in ("position_emb", "feat_emb.weight", "quantize.embedding.weight"):
        if probe not in sd or not hasattr(sd[probe], "shape") or len(sd[probe].shape) != 2:
            raise KeyError(f"{name}: the weights lack '{probe}': expected the keys of CodeFormer (ops_codeformer.codeformer_state_dict_shapes())")
    n_layers = 0
    while f"ft_layers.{n_layers}.norm1.weight" in sd:
        n_layers += 1
    connect = tuple(s for s in CF_CONNECT if f"fuse_convs_dict.{s}.scale.0.weight" in sd)
    return _config_checked(name, int(sd["feat_emb.weight"].shape[0]), 8, n_layers, int(sd["quantize.embedding.weight"].shape[0]), int(sd["position_emb"].shape[0]),
                           connect)


_CF_NET = _Net("CodeFormer", _cf_shapes, _PREFIXES, True, ("position_emb",), _cf_variant,
               "the native path is the eval-mode forward (inference_codeformer.py calls net.eval())", ())


def _net_of(weights):
    return module_net(_CF_NET, weights.config) if isinstance(weights, CodeFormer) else _CF_NET


class PreparedCodeFormer(PreparedNet):
    """The kernels' copies of the front's weights, rebuilt when a tensor changes version or storage: per encoder block its convolutions as three-way split slabs
    with their biases (conv_in as the exact kernel's K-major float32 weight; q | k | v of an AttnBlock concatenated to one convolution) and its GroupNorm
    vectors; the transformer's linears as 1 x 1 slabs (the in-projection cut into q | k and v), ``pos`` = position_emb transposed to ``[E, T]``; the head's
    LayerNorm and its exact K-major weight; the codebook.  The generator's and the fuse blocks' weights are validated and watched, not prepared: those are
    ``ops_codeformer_gen.PreparedCodeFormerGenerator``'s."""

    __slots__ = ()
    _entry = "codeformer_front"

    def _net(self, weights):
        return _net_of(weights)

    def _build(self, sd, variant, dev):
        E, n_head, n_layers, K, T, _ = variant
        sb = lambda k, w=None, b=None: prep_fwd(sd[k + ".weight"] if w is None else w, None, sd.get(k + ".bias") if b is None else b)   # noqa: E731
        gn = lambda k: (sd[k + ".weight"], sd[k + ".bias"])                                                                             # noqa: E731
        lin = lambda w: w.reshape(w.shape[0], w.shape[1], 1, 1)                                                                         # noqa: E731
        blocks = []
        for i, (kind, cin, cout) in enumerate(ENCODER_PLAN):
            p = f"encoder.blocks.{i}"
            if kind == "conv":
                blocks.append(prep_exact(sd[p + ".weight"], None, sd[p + ".bias"]) if cin == 3 else sb(p))
            elif kind == "res":
                blocks.append(dict(n1=gn(p + ".norm1"), c1=sb(p + ".conv1"), n2=gn(p + ".norm2"), c2=sb(p + ".conv2"), out=sb(p + ".conv_out") if cin != cout else None))
            elif kind == "attn":
                qkv = sb(p, torch.cat([sd[f"{p}.{m}.weight"] for m in "qkv"]), torch.cat([sd[f"{p}.{m}.bias"] for m in "qkv"]))
                blocks.append(dict(norm=gn(p + ".norm"), qkv=qkv, proj=sb(p + ".proj_out")))
            elif kind == "down":
                blocks.append(sb(p + ".conv"))
            else:
                blocks.append(gn(p))
        layers = []
        for i in range(n_layers):
            p = f"ft_layers.{i}"
            w, b = sd[p + ".self_attn.in_proj_weight"], sd[p + ".self_attn.in_proj_bias"]
            layers.append(dict(n1=gn(p + ".norm1"), n2=gn(p + ".norm2"), qk=sb(p, lin(w[:2 * E]), b[:2 * E].contiguous()), v=sb(p, lin(w[2 * E:]), b[2 * E:].contiguous()),
                               out=sb(p, lin(sd[p + ".self_attn.out_proj.weight"]), sd[p + ".self_attn.out_proj.bias"]),
                               l1=sb(p, lin(sd[p + ".linear1.weight"]), sd[p + ".linear1.bias"]), l2=sb(p, lin(sd[p + ".linear2.weight"]), sd[p + ".linear2.bias"])))
        return dict(config=variant, blocks=blocks, layers=layers, feat_emb=sb("feat_emb", lin(sd["feat_emb.weight"]), sd["feat_emb.bias"]),
                    pos=sd["position_emb"].t().contiguous(), head_ln=gn("idx_pred_layer.0"), head=prep_exact(lin(sd["idx_pred_layer.1.weight"]))[0],
                    emb=sd["quantize.embedding.weight"])


# ------------------------------------------------------------------------------------------------ the kernel-level operators
def _new(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _gn_run(x, gamma, beta, swish, groups=CF_GROUPS):
    bs, C, h, w = x.shape
    hw = h * w
    run = C // groups * hw
    chunks = min(64, -(-run // CF_GN_CHUNK))                                                  # from the shapes alone
    part, stats = _new(x, bs * groups, chunks, 2), _new(x, bs * groups, 3)
    lib().call("e4s_cf_group_stats", _p(stats), _p(part), _p(x), bs * groups, run, chunks, CF_GN_EPS, _stream())
    out = torch.empty_like(x)
    lib().call("e4s_cf_group_norm", _p(out), _p(x), _p(stats), _p(gamma), _p(beta), bs, C, groups, hw, int(swish), _stream())
    return out


def group_norm_swish(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, swish: bool = True) -> torch.Tensor:
    """``GroupNorm(32, C, eps=1e-6)`` of ``x [bs, C, h, w]`` followed by swish ``s * sigmoid(s)``, or the plain normalisation with ``swish=False``.  The
    statistics are two passes over pieces of each group's contiguous run, merged in float64 in a fixed order."""
    name = "group_norm_swish"
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, C, h, w] tensor")
    bs, C, h, w = x.shape
    if C % CF_GROUPS or h * w < 1 or bs * C > 65535:
        raise ValueError(f"{name}: x is {tuple(x.shape)}: C is a multiple of {CF_GROUPS}, the planes are not empty and bs C <= 65535")
    for nm, t in (("gamma", gamma), ("beta", beta)):
        _tensor_checked(name, nm, t, torch.float32, 1, f"a float32 [{C}] vector")
        if t.shape[0] != C:
            raise ValueError(f"{name}: {nm}: expected a float32 [{C}] vector, got {tuple(t.shape)}")
    _cuda_checked(name, x=x, gamma=gamma, beta=beta)
    if bs == 0:
        return torch.empty_like(x)
    return _gn_run(x.detach().contiguous(), gamma.detach().contiguous(), beta.detach().contiguous(), swish)


def _attn_run(q, k, v, heads, scale, bs, C, T):
    out = _new(q, bs, C, T)
    lib().call("e4s_cf_attention", _p(out), _p(q), _p(k), _p(v), q.stride(0), k.stride(0), v.stride(0), C * T, bs, heads, C // heads, T, float(scale), _stream())
    return out


def _head_checked(name, C, heads, T):
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1 or C % heads:
        raise ValueError(f"{name}: {C} channels are not divisible into {heads!r} heads")
    d = C // heads
    if d % 16 or d > CF_MAX_HEAD:
        raise ValueError(f"{name}: head width {d}: a multiple of 16 up to {CF_MAX_HEAD}")
    if not 1 <= T <= CF_MAX_TOKENS:
        raise ValueError(f"{name}: {T} tokens: 1 .. {CF_MAX_TOKENS}")


def attention_cm(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale=None) -> torch.Tensor:
    """Softmax attention on channel-major operands ``[bs, heads d, T]``: ``out[b, h d + c, i] = sum_j softmax_j(scale q_i . k_j) v[c, j]`` in exact float32;
    ``scale`` defaults to ``d ** -0.5``.  An operand may be a channel slice of a larger tensor (its batch stride is passed on).  ``T`` 1 .. 1024, ``d`` a multiple
    of 16 up to 512."""
    name = "attention_cm"
    for nm, t in (("q", q), ("k", k), ("v", v)):
        _tensor_checked(name, nm, t, torch.float32, 3, "a float32 [bs, heads d, T] tensor")
        if t.shape != q.shape:
            raise ValueError(f"{name}: {nm} is {tuple(t.shape)}, q is {tuple(q.shape)}")
    bs, C, T = q.shape
    _head_checked(name, C, heads, T)
    _cuda_checked(name, q=q, k=k, v=v)
    if bs == 0:
        return _new(q, 0, C, T)
    ops = [t.detach() if t.stride(2) == 1 and t.stride(1) == T and (bs == 1 or t.stride(0) >= C * T) else t.detach().contiguous() for t in (q, k, v)]
    return _attn_run(*ops, heads, (C // heads) ** -0.5 if scale is None else scale, bs, C, T)


def _ln_run(x, gamma, beta, pos, bs, C, T):
    y = torch.empty_like(x)
    yp = torch.empty_like(x) if pos is not None else None
    lib().call("e4s_cf_layer_norm", _p(y), _p(yp), _p(x), _p(gamma), _p(beta), _p(pos), bs, C, T, CF_LN_EPS, _stream())
    return y if pos is None else (y, yp)


def layer_norm_cm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, pos=None):
    """``LayerNorm(C)`` (eps 1e-5) over the channels of every token of a channel-major ``x [bs, C, T]``; with ``pos [C, T]`` the pair ``(y, y + pos)``."""
    name = "layer_norm_cm"
    _tensor_checked(name, "x", x, torch.float32, 3, "a float32 [bs, C, T] tensor")
    bs, C, T = x.shape
    if not 1 <= C <= 512 or T < 1:
        raise ValueError(f"{name}: x is {tuple(x.shape)}: 1 .. 512 channels and at least one token")
    for nm, t in (("gamma", gamma), ("beta", beta)):
        _tensor_checked(name, nm, t, torch.float32, 1, f"a float32 [{C}] vector")
        if t.shape[0] != C:
            raise ValueError(f"{name}: {nm}: expected a float32 [{C}] vector, got {tuple(t.shape)}")
    if pos is not None:
        _tensor_checked(name, "pos", pos, torch.float32, 2, f"a float32 [{C}, {T}] tensor")
        if tuple(pos.shape) != (C, T):
            raise ValueError(f"{name}: pos: expected a float32 [{C}, {T}] tensor, got {tuple(pos.shape)}")
        _cuda_checked(name, pos=pos)
    _cuda_checked(name, x=x, gamma=gamma, beta=beta)
    if bs == 0:
        return torch.empty_like(x) if pos is None else (torch.empty_like(x), torch.empty_like(x))
    return _ln_run(x.detach().contiguous(), gamma.detach().contiguous(), beta.detach().contiguous(), None if pos is None else pos.detach().contiguous(), bs, C, T)


# ------------------------------------------------------------------------------------------------ the front
def _res(x, B):
    h = conv_sb(_gn_run(x, *B["n1"], True), *B["c1"], k=3)
    return conv_sb(_gn_run(h, *B["n2"], True), *B["c2"], k=3, residual=x if B["out"] is None else conv_sb(x, *B["out"], k=1))


def _attn_block(x, B):
    bs, C, h, w = x.shape
    qkv = conv_sb(_gn_run(x, *B["norm"], False), *B["qkv"], k=1)
    a = _attn_run(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], 1, int(C) ** (-0.5), bs, C, h * w)
    return conv_sb(a.view(bs, C, h, w), *B["proj"], k=1, residual=x)


def _down(x, B):
    bs, C, h, w = x.shape
    padded = _new(x, bs, C, h + 1, w + 1)
    lib().call("e4s_cf_pad_rb", _p(padded), _p(x), bs * C, h, w, _stream())
    return conv_sb(padded, *B, k=3, stride=2, pad=0)


def _encode(x, P, connect):
    taps, by_block = {}, {b: s for s, b in CF_TAP_BLOCKS.items() if s in connect}
    for i, ((kind, cin, _), B) in enumerate(zip(ENCODER_PLAN, P["blocks"])):
        if kind == "conv":
            x = conv_exact(x, *B, k=3) if cin == 3 else conv_sb(x, *B, k=3)
        elif kind == "res":
            x = _res(x, B)
        elif kind == "attn":
            x = _attn_block(x, B)
        elif kind == "down":
            x = _down(x, B)
        else:
            x = _gn_run(x, *B, False)
        if i in by_block:
            taps[by_block[i]] = x                     # every layer writes a tensor of its own: nothing behind a tap touches it
    return x, taps


def _logits(lq_feat, P):
    E, n_head = P["config"][:2]
    bs, _, h, w = lq_feat.shape
    T = h * w
    x = conv_sb(lq_feat, *P["feat_emb"], k=1)                                                # [bs, E, h, w]: channel-major, the tokens innermost
    for L in P["layers"]:
        n, npos = _ln_run(x, *L["n1"], P["pos"], bs, E, T)
        qk = conv_sb(npos, *L["qk"], k=1)
        v = conv_sb(n, *L["v"], k=1)
        a = _attn_run(qk[:, :E], qk[:, E:], v, n_head, (E // n_head) ** -0.5, bs, E, T)
        x = conv_sb(a.view(bs, E, h, w), *L["out"], k=1, residual=x)
        hid = conv_sb(_ln_run(x, *L["n2"], None, bs, E, T), *L["l1"], k=1)
        lib().call("e4s_cf_gelu", _p(hid), _p(hid), hid.numel(), _stream())
        x = conv_sb(hid, *L["l2"], k=1, residual=x)
    cm = conv_exact(_ln_run(x, *P["head_ln"], None, bs, E, T), P["head"], None, k=1)          # [bs, codebook, h, w], exact float32 products
    return cm.view(bs, -1, T).transpose(1, 2)                                                # [bs, T, codebook] as the reference returns it (a view)


def _codes(logits):
    bs, T, K = logits.shape
    idx = torch.empty((bs, T), dtype=torch.int64, device=logits.device)
    lib().call("e4s_cf_argmax", _p(idx), _p(logits), bs, T, K, logits.stride(0), logits.stride(1), logits.stride(2), _stream())
    return idx


def _quant(idx, lq_feat, emb, adain):
    bs, C, h, w = lq_feat.shape
    out = torch.empty_like(lq_feat)
    lib().call("e4s_cf_quant", _p(out), _p(idx), _p(emb), _p(lq_feat), bs, C, h * w, emb.shape[0], int(bool(adain)), CF_ADAIN_EPS, _stream())
    return out


def _weights_checked(name, weights):
    return _validated(name, weights, _net_of(weights))


def _image_checked(name, x, cfg, adain):
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [n, 3, H, W] image")
    n, c3, H, W = x.shape
    if c3 != 3 or H < 32 or W < 32 or H % 32 or W % 32:
        raise ValueError(f"{name}: x: expected a float32 [n, 3, H, W] image with H and W multiples of 32 (five Downsamples), got {tuple(x.shape)}")
    _tokens_checked(name, H // 32 * (W // 32), cfg, adain, f"x is {H} x {W}")


def _tokens_checked(name, T, cfg, adain, what):
    if T != cfg[4]:
        raise ValueError(f"{name}: {what}: T = {T} tokens, position_emb has latent_size = {cfg[4]} rows")
    if T > CF_MAX_TOKENS:
        raise ValueError(f"{name}: {what}: T = {T} tokens, at most {CF_MAX_TOKENS}")
    if adain and T < 2:
        raise ValueError(f"{name}: {what}: T = {T} token: the AdaIN's unbiased variance of one value is undefined (adain=False takes it)")


def _lq_checked(name, lq_feat, cfg, adain):
    _tensor_checked(name, "lq_feat", lq_feat, torch.float32, 4, f"a float32 [n, {CF_EMB}, h, w] tensor")
    if lq_feat.shape[1] != CF_EMB or lq_feat.shape[2] < 1 or lq_feat.shape[3] < 1:
        raise ValueError(f"{name}: lq_feat: expected a float32 [n, {CF_EMB}, h, w] tensor, got {tuple(lq_feat.shape)}")
    _tokens_checked(name, lq_feat.shape[2] * lq_feat.shape[3], cfg, adain, f"lq_feat is {lq_feat.shape[2]} x {lq_feat.shape[3]}")


def _placed(name, nm, t, checked):
    _devices_checked(name, nm, t, checked[2])
    _cuda_checked(name, **{nm: t})


def codeformer_encode(x: torch.Tensor, weights):
    """``(lq_feat [n, 256, H / 32, W / 32], taps)`` of the VQGAN encoder on ``x [n, 3, H, W]``; ``taps``: the dict ``'32' | '64' | '128' | '256'`` (those in the
    module's ``connect_list``) of the tensors after encoder blocks 14, 11, 8, 5, which no later layer writes to.  ``weights``: a ``CodeFormer`` module or a
    mapping with its keys (bare, or under ``params_ema`` / ``params``; a mapping is taken to have 8 heads)."""
    name = "codeformer_encode"
    checked = _weights_checked(name, weights)
    _image_checked(name, x, checked[1], False)
    _placed(name, "x", x, checked)
    with torch.no_grad():
        return _encode(x.detach().contiguous(), prepare(PreparedCodeFormer, weights, checked), checked[1][5])


def codeformer_logits(lq_feat: torch.Tensor, weights) -> torch.Tensor:
    """``logits [n, T, codebook]`` of the transformer and the head on ``lq_feat [n, 256, h, w]``, ``T = h w = latent_size`` (a view of the channel-major
    ``[n, codebook, T]`` the head writes)."""
    name = "codeformer_logits"
    checked = _weights_checked(name, weights)
    _lq_checked(name, lq_feat, checked[1], False)
    _placed(name, "lq_feat", lq_feat, checked)
    with torch.no_grad():
        return _logits(lq_feat.detach().contiguous(), prepare(PreparedCodeFormer, weights, checked))


def codeformer_codes(logits: torch.Tensor) -> torch.Tensor:
    """The top-1 code ``idx [n, T]`` (int64) of ``logits [n, T, codebook]``, the lowest index winning an exact tie (the softmax in front of the reference's
    ``topk`` is monotone and not computed)."""
    name = "codeformer_codes"
    _tensor_checked(name, "logits", logits, torch.float32, 3, "a float32 [n, T, codebook] tensor")
    if logits.shape[1] < 1 or logits.shape[2] < 1:
        raise ValueError(f"{name}: logits: expected a float32 [n, T, codebook] tensor, got {tuple(logits.shape)}")
    _cuda_checked(name, logits=logits)
    return _codes(logits.detach())


def codeformer_quant(idx: torch.Tensor, lq_feat: torch.Tensor, weights, adain: bool = True) -> torch.Tensor:
    """``quant_feat [n, 256, h, w]``: ``quantize.embedding.weight[idx]`` laid out like ``lq_feat`` and, with ``adain``, ``adaptive_instance_normalization`` of it
    against ``lq_feat`` (unbiased variance, eps 1e-5 inside the root, for both operands)."""
    name = "codeformer_quant"
    checked = _weights_checked(name, weights)
    _lq_checked(name, lq_feat, checked[1], adain)
    _tensor_checked(name, "idx", idx, torch.int64, 2, "an int64 [n, T] tensor")
    if tuple(idx.shape) != (lq_feat.shape[0], lq_feat.shape[2] * lq_feat.shape[3]):
        raise ValueError(f"{name}: idx is {tuple(idx.shape)}, lq_feat {tuple(lq_feat.shape)}: expected [n, h w]")
    _placed(name, "lq_feat", lq_feat, checked)
    _cuda_checked(name, idx=idx)
    with torch.no_grad():
        return _quant(idx.contiguous(), lq_feat.detach().contiguous(), prepare(PreparedCodeFormer, weights, checked)["emb"], adain)


def codeformer_front(x: torch.Tensor, weights, adain: bool = True):
    """``dict(quant_feat, logits, lq_feat, idx, taps)`` of ``x [n, 3, H, W]`` (float32, ``(v / 255 - 0.5) / 0.5`` of an RGB face): ``CodeFormer.forward`` up to
    the generator's input.  Refused by name before any launch: a module in training mode, another dtype, H or W no multiple of 32, ``H / 32 * W / 32`` other
    than ``latent_size`` or over 1024, one token with ``adain=True``."""
    name = "codeformer_front"
    checked = _weights_checked(name, weights)
    _image_checked(name, x, checked[1], adain)
    _placed(name, "x", x, checked)
    with torch.no_grad():
        return _front_run(x, weights, checked, adain)


def _front_run(x, weights, checked, adain):
    """The front on checked arguments (``codeformer_front``, and ``ops_codeformer_gen.codeformer_restore`` after its own checks)."""
    P = prepare(PreparedCodeFormer, weights, checked)
    lq_feat, taps = _encode(x.detach().contiguous(), P, checked[1][5])
    logits = _logits(lq_feat, P)
    idx = _codes(logits)
    return dict(quant_feat=_quant(idx, lq_feat, P["emb"], adain), logits=logits, lq_feat=lq_feat, idx=idx, taps=taps)


__all__ = ["CodeFormer", "PreparedCodeFormer", "ENCODER_PLAN", "CF_TAP_BLOCKS", "adain_reference", "codeformer_state_dict_shapes", "group_norm_swish", "attention_cm",
           "layer_norm_cm", "codeformer_encode", "codeformer_logits", "codeformer_codes", "codeformer_quant", "codeformer_front"]
