"""PTI fine-tuning step on the drop-in ``Net3`` (SURVEY §8 row f1 / BASELINE configs[3]).

Mirrors one inner iteration of ``VideoSwapPTICoach.train_e4s`` (training/video_swap_ft_coach.py:253-299) for the part that lives on the
hot path: ``cal_style_codes`` -> ``gen_img`` -> pixel loss -> ``backward`` -> optimiser step, with the style vectors and region map of a
frame as fixed inputs.  The forward runs on the fused HIP kernels; the backward of the synthesis layers differentiates from their
outputs with the gradient kernels of ``csrc/modconv_bwd.hip`` + ``csrc/gemm_sb.hip`` (``ops._MaskedStyledConvGrad`` /
``ops._SingleStyledConvGrad``), only the small per-layer style tables go through autograd (``torch_ref.py``).  The loss is ``calc_loss``'s
(:176-223) L2 term plus, with ``lpips=`` (the drop-in ``criteria.lpips.LPIPS`` with its weights loaded), ``lpips_lambda`` times its LPIPS-AlexNet
term at three scales (:201-211) — forward and input gradient on the HIP kernels of ``ops_lpips``, on the foreground-masked images as the
video coach computes it (:188-190); ``style_vector_step`` takes it unmasked, as optimization.py:111-146 does.  With ``id_loss=`` (the drop-in
``criteria.id_loss.IDLoss`` with its weights loaded) ``id_lambda`` times the ArcFace identity term (:192-195) is added the same way (``ops_id``),
and with ``face_parsing=`` (the drop-in ``criteria.face_parsing.face_parsing_loss.FaceParsingLoss`` with its weights loaded) ``face_parsing_lambda``
times the unet face-parsing feature term (:212-216, ``ops_fp``).  That completes one call of ``calc_loss``; ``extra_loss`` remains for anything else.
``recolor=`` adds the second call, ``recolor_lambda`` times the same terms against the recoloured driven frame (:274-287), sharing the
reconstruction's loss-network passes with the first (``_loss_recolor``, ``TargetCache``).

Several GPUs: one process per GPU, each on its own frame; the one exchange step is the gradient average before the
optimiser step (``sync_gradients``: a few large flat all-reduces over RCCL, not one per tensor).  That is a batch-of-N Adam step, not
the reference's N sequential batch-1 steps, so result parity with the reference is not claimed for the multi-GPU mode.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Callable, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import ops, ops_fp, ops_id, ops_lpips, ops_multi
from .netweights import weights_key


def trainable_parameters(net):
    """``configure_optimizer`` (video_swap_ft_coach.py:171-177): every parameter the constructor left ``requires_grad=True``."""
    return [p for p in net.parameters() if p.requires_grad]


def _id_multiscale(id_loss) -> bool:
    """``opts.id_loss_multiscale`` of a drop-in ``IDLoss`` (the reference's default, True, for a bare network or mapping)."""
    return bool(getattr(getattr(id_loss, "opts", None), "id_loss_multiscale", True))


# One loss-network term of calc_loss: ``module`` (the weights) and ``lam``; ``name``: its TargetCache attribute, ``label``: its name in messages;
# ``loss(a, b, module)``, ``loss_multi(a, targets, tw, module, frame)`` and ``target_features(images, module)`` of its ops module.
_Term = namedtuple("_Term", "module lam name label check_loaded weight_tensors loss loss_multi target_features")


def _terms(lpips=None, lpips_lambda: float = 0.8, id_loss=None, id_lambda: float = 0.1, face_parsing=None, face_parsing_lambda: float = 0.1):
    """The loss-network terms that have a module, in the order they are summed: LPIPS (calc_loss :201-211), identity (:192-195), face-parsing
    (:212-216)."""
    ms = _id_multiscale(id_loss)
    table = (_Term(lpips, lpips_lambda, "lpips", "LPIPS", ops_lpips.check_loaded, ops_lpips.weight_tensors, ops_lpips.lpips_multiscale,
                   ops_lpips.lpips_multiscale_multi, ops_lpips.target_features),
             _Term(id_loss, id_lambda, "id", "ArcFace (id_loss)", ops_id.check_loaded, ops_id.weight_tensors,
                   lambda a, b, m: ops_id.id_loss(a, b, m, ms), lambda a, ys, tw, m, frame: ops_id.id_loss_multi(a, ys, tw, m, ms, frame),
                   lambda images, m: ops_id.target_features(images, m, ms)),
             _Term(face_parsing, face_parsing_lambda, "fp", "face-parsing", ops_fp.check_loaded, ops_fp.weight_tensors, ops_fp.fp_loss,
                   ops_fp.fp_loss_multi, ops_fp.target_features))
    return [t for t in table if t.module is not None]


def _check_loaded(terms):
    for t in terms:
        t.check_loaded(t.module)


def _loss(net, style_vectors, mask, target, foreground_mask, l2_lambda, extra_loss, randomize_noise, lpips=None, lpips_lambda: float = 0.8,
          id_loss=None, id_lambda: float = 0.1, face_parsing=None, face_parsing_lambda: float = 0.1):
    codes = net.cal_style_codes(style_vectors)
    recon, _, _ = net.gen_img(None, codes, mask, randomize_noise=randomize_noise)
    a, b = (recon, target) if foreground_mask is None else (recon * foreground_mask, target * foreground_mask)
    loss = l2_lambda * F.mse_loss(a, b)                                      # calc_loss :196-199 (loss_l2)
    for t in _terms(lpips, lpips_lambda, id_loss, id_lambda, face_parsing, face_parsing_lambda):     # on the masked images
        loss = loss + t.lam * t.loss(a, b, t.module)
    if extra_loss is not None:
        loss = loss + extra_loss(recon, target)
    return loss, recon


class TargetCache:
    """The target side of the two-target PTI objective: the foreground-weighted driven and recoloured frames (``images[j] * fg``) and their
    features in every loss network given, for ``n`` frames (a clip, read through the device int32 ``frame``) or for the batch of one step.
    The target side does not change over the passes of a clip, so ``tune_clip`` builds it once.  Like ``GraphedPTIStep``, the cache
    remembers the loss weights it was built with and refuses to be used after they change."""

    def __init__(self, images, foreground_mask=None, lpips=None, id_loss=None, face_parsing=None):
        n = images[0].shape[0]
        if any(t.shape != images[0].shape for t in images):
            raise ValueError("TargetCache: the target images must have the same shape")
        self.n = n
        self.images = [(t * foreground_mask if foreground_mask is not None else t).contiguous() for t in images]
        terms = _terms(lpips=lpips, id_loss=id_loss, face_parsing=face_parsing)
        self._modules = (lpips, id_loss, face_parsing)
        self._tensors = [w for t in terms for w in t.weight_tensors(t.module)]
        self._key = weights_key(self._tensors)
        self.lpips = self.id = self.fp = None                    # per term: a target_features list per image of ``images``
        for t in terms:
            setattr(self, t.name, [t.target_features(im, t.module) for im in self.images])
        self.frame = torch.zeros((1,), dtype=torch.int32, device=images[0].device)

    def check(self, lpips=None, id_loss=None, face_parsing=None):
        """Raises unless the cache holds features for exactly these loss modules, with the weights it was built from."""
        if any(m is not g for m, g in zip(self._modules, (lpips, id_loss, face_parsing))):
            raise ValueError("TargetCache: built for other loss modules than the step's")
        if weights_key(self._tensors) != self._key:
            raise RuntimeError("TargetCache: the loss weights changed after the target features were cached; build a new cache")

    def select(self, i: int):
        """Points the cache's device frame index at frame ``i``."""
        i = int(i)
        if not 0 <= i < self.n:
            raise IndexError(f"TargetCache: frame {i} of {self.n}")
        self.frame.fill_(i)

    @property
    def nbytes(self) -> int:
        ts = list(self.images) + [t for fs in (self.lpips or []) + (self.id or []) + (self.fp or []) for t in fs]
        return sum(t.numel() * t.element_size() for t in ts)


def _loss_recolor(net, style_vectors, mask, target, foreground_mask, l2_lambda, extra_loss, randomize_noise, lpips, lpips_lambda, id_loss, id_lambda,
                  face_parsing, face_parsing_lambda, recolor, recolor_lambda: float, cache: Optional[TargetCache] = None):
    """``_loss`` of the driven frame + ``recolor_lambda`` x the same terms against the recoloured frame (video_swap_ft_coach.py:274-287).
    With ``foreground_mask`` both terms weight by it and share the reconstruction side: one forward pass and input gradient per loss network, the
    heads against both targets (from ``cache``, at its device frame index, or from target features computed here).  Without one the driven term is
    unmasked (:284) and the recolor term uses the foreground weight of ``mask`` (:277-280, 286): the inputs differ, so nothing is shared."""
    codes = net.cal_style_codes(style_vectors)
    recon, _, _ = net.gen_img(None, codes, mask, randomize_noise=randomize_noise)
    return recolor_objective(recon, target, recolor, foreground_mask, mask, l2_lambda, lpips, lpips_lambda, id_loss, id_lambda, face_parsing,
                             face_parsing_lambda, recolor_lambda, extra_loss, cache), recon


def recolor_objective(recon, target, recolor, foreground_mask, mask, l2_lambda: float = 1.0, lpips=None, lpips_lambda: float = 0.8, id_loss=None,
                      id_lambda: float = 0.1, face_parsing=None, face_parsing_lambda: float = 0.1, recolor_lambda: float = 5.0, extra_loss=None,
                      cache: Optional[TargetCache] = None):
    """The two-target objective of ``train_e4s`` on a given reconstruction (0-d, differentiable in ``recon``): ``calc_loss(target, recon, fg) +
    recolor_lambda * calc_loss(recolor, recon, fg)`` (video_swap_ft_coach.py:277-287) — see ``_loss_recolor``.  ``mask`` (the region map) is read only
    without a ``foreground_mask``; ``cache`` replaces ``target`` / ``recolor`` (then at its device frame index)."""
    rl = float(recolor_lambda)
    terms = _terms(lpips, lpips_lambda, id_loss, id_lambda, face_parsing, face_parsing_lambda)
    if foreground_mask is None:
        loss = l2_lambda * F.mse_loss(recon, target)
        for t in terms:
            loss = loss + t.lam * t.loss(recon, target, t.module)
        labels = mask if mask.dtype == torch.uint8 else ops.mask_to_labels(mask)
        fg = prepare_clip(labels, None, recon.shape[-2:])[1]
        tgt, tw = TargetCache([recolor], fg, lpips, id_loss, face_parsing), [rl]
    else:
        fg = foreground_mask
        loss = None
        tgt = cache if cache is not None else TargetCache([target, recolor], fg, lpips, id_loss, face_parsing)
        tw = [1.0, rl]
    frame = tgt.frame if cache is not None else None
    a = recon * fg
    # the targets' weights are (1, recolor_lambda), the term lambdas stay outside as in _loss: with recolor_lambda = 0 the heads give _loss's bits
    term = l2_lambda * ops_multi.mse_multi(recon, fg, tgt.images, tw, frame)
    loss = term if loss is None else loss + term
    for t in terms:
        loss = loss + t.lam * t.loss_multi(a, getattr(tgt, t.name), tw, t.module, frame)
    if extra_loss is not None:
        loss = loss + extra_loss(recon, target)
    return loss


def _check_recolor(recolor, images, what: str):
    if recolor is not None and (not isinstance(recolor, torch.Tensor) or recolor.shape != images.shape):
        raise ValueError(f"{what}: recolor must have the images' shape {tuple(images.shape)}, got "
                         f"{tuple(recolor.shape) if isinstance(recolor, torch.Tensor) else type(recolor).__name__}")


def sync_gradients(params, group=None, bucket_bytes: int = 256 << 20, active_ranks: Optional[int] = None) -> int:
    """Average ``p.grad`` over the ranks of ``group`` in place: gradients are packed into flat buckets of about ``bucket_bytes``
    (xGMI rings are per-link bound, so few large all-reduces: SURVEY §8e), one ``all_reduce`` each, launched back to back and waited
    for together.  Which parameters take part is agreed on first — one small MAX all-reduce of a has-gradient flag per parameter: a
    parameter that NO rank has a gradient for (the optimiser's list follows the reference and includes the whole encoder, which the PTI
    loss never reaches) is skipped exactly as a single-GPU step skips it — no zero gradient, no Adam state, no xGMI traffic; one that only
    some ranks have a gradient for contributes zeros from the others (every rank must issue the same collectives).
    ``active_ranks``: divide the summed gradients by this number instead of the world size (a round of ``tune_clip`` in which only some
    ranks still have a frame).  Returns the number of gradient all-reduces issued; a no-op (0) outside a process group or at world size 1."""
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    world = dist.get_world_size(group)
    if world == 1:
        return 0
    params = [p for p in params if p.requires_grad]
    if not params:
        return 0
    flags = torch.tensor([0 if p.grad is None else 1 for p in params], dtype=torch.int32, device=params[0].device)
    dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=group)
    params = [p for p, f in zip(params, flags.tolist()) if f]
    buckets, cur, cur_bytes = [], [], 0
    for p in params:
        nbytes = p.numel() * p.element_size()
        if cur and (cur_bytes + nbytes > bucket_bytes or cur[0].dtype != p.dtype):
            buckets.append(cur)
            cur, cur_bytes = [], 0
        cur.append(p)
        cur_bytes += nbytes
    if cur:
        buckets.append(cur)
    pending = []
    denom = float(world if active_ranks is None else max(int(active_ranks), 1))
    for bucket in buckets:
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in bucket])
        pending.append((dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group, async_op=True), flat, bucket))
    for work, flat, bucket in pending:
        work.wait()
        flat.div_(denom)
        off = 0
        for p in bucket:
            n = p.numel()
            if p.grad is None:
                p.grad = flat[off:off + n].view_as(p).clone()
            else:
                p.grad.copy_(flat[off:off + n].view_as(p))
            off += n
    return len(buckets)


class GraphedPTIStep:
    """The whole optimiser step (forward, backward, Adam update) captured once as a hipGraph and replayed per frame: at batch 1 the
    eager step issues several thousand short launches and is bound by the host (~0.12 s) rather than by the GPU.

    ``optimizer`` must be capture-safe (``torch.optim.Adam(..., capturable=True, fused=True)``: the fused multi-tensor update is 6 ms
    per step cheaper than the default one over the generator's 263 tensors); shapes are fixed by the example inputs;
    ``mask`` must be a uint8 region map ``[bs, 512, 512]`` (the one-hot check of a float mask reads a flag back to the host).
    The ``warmup`` eager steps that precede the capture are real optimiser steps on the example frame.  Weight re-layout kernels are
    part of the captured step (the parameters change under them), so every replay prepares its weights from their current values."""

    def __init__(self, net, optimizer, style_vectors, mask, target, foreground_mask=None, l2_lambda: float = 1.0, extra_loss=None,
                 randomize_noise: bool = True, warmup: int = 3, warm_inputs=None, lpips=None, lpips_lambda: float = 0.8, id_loss=None,
                 id_lambda: float = 0.1, face_parsing=None, face_parsing_lambda: float = 0.1, recolor=None, recolor_lambda: float = 5.0,
                 target_cache: Optional[TargetCache] = None, frame: Optional[int] = None, warm_frames=None):
        """``warm_inputs``: the frames of the eager steps that precede the capture, as ``(style_vectors, mask, target[, foreground_mask])``
        tuples (default: the example frame ``warmup`` times).  They are real optimiser steps: a loop passes its own first frames here
        (``tune_clip``) and continues with the replayed step from the next one; ``self.warm_losses`` holds their losses.
        ``lpips`` / ``lpips_lambda``: the LPIPS term as in ``pti_step`` (its kernels are captured with the rest of the step).  Load the LPIPS
        weights before constructing the step: the captured graph reads copies prepared from them, and a replay after they have changed raises.
        ``id_loss`` / ``face_parsing`` and their lambdas: the identity and face-parsing terms, under the same rule.
        ``recolor`` / ``recolor_lambda``: adds the terms against the recoloured frame (``pti_step``); the step then takes ``recolor=`` on every call.
        ``target_cache``: a ``TargetCache`` of the clip's driven and recoloured frames (built with the same foreground weights and loss modules) that
        the step reads instead of running the target side; every call then names its ``frame`` (``frame`` / ``warm_frames``: those of the capture
        example and of the warm-up steps), which is written to the cache's device index before the replay."""
        if mask.dtype != torch.uint8:
            raise TypeError("GraphedPTIStep needs the uint8 region map (ops.mask_to_labels(onehot)), not a float mask")
        # the loss networks' weights are prepared (re-laid-out) once, before the capture, and the graph reads those copies: weights loaded later would
        # not reach the replays, so the step remembers which weights it was captured with and refuses to replay after they change
        self._watched = [(t.label, ts, weights_key(ts)) for t in _terms(lpips=lpips, id_loss=id_loss, face_parsing=face_parsing)
                         for ts in [t.weight_tensors(t.module)]]
        self.net = net
        self.static = [style_vectors.clone(), mask.clone(), target.clone()] + ([foreground_mask.clone()] if foreground_mask is not None else [])
        fg = self.static[3] if foreground_mask is not None else None
        args = (net, self.static[0], self.static[1], self.static[2], fg, l2_lambda, extra_loss, randomize_noise, lpips, lpips_lambda, id_loss, id_lambda,
                face_parsing, face_parsing_lambda)
        self.cache, self.cache_modules = target_cache, (lpips, id_loss, face_parsing)
        self._recolor = recolor is not None and target_cache is None          # a static recolor buffer, copied per call
        if target_cache is not None:
            if foreground_mask is None or recolor is not None:
                raise ValueError("GraphedPTIStep: a target cache needs the foreground weight and takes the recolor frames from the cache")
            target_cache.check(lpips, id_loss, face_parsing)
            if frame is None or (warm_inputs is not None and (warm_frames is None or len(warm_frames) != len(warm_inputs))):
                raise ValueError("GraphedPTIStep: with a target cache, name the frame of the example (frame=) and of each warm input (warm_frames=)")
            target_cache.select(frame)
            args = args + (None, recolor_lambda, target_cache)
        elif recolor is not None:
            _check_recolor(recolor, target, "GraphedPTIStep")
            self.static.append(recolor.clone())
            args = args + (self.static[-1], recolor_lambda, None)
        loss_fn = _loss_recolor if (recolor is not None or target_cache is not None) else _loss
        self.stream = torch.cuda.Stream()                 # warm-up and capture on one stream of our own (see graphs.GraphedCall)
        ops.prepare_stream_context(self.stream)
        self.stream.wait_stream(torch.cuda.current_stream())
        self.warm_losses = []
        with torch.cuda.stream(self.stream):
            for i, w in enumerate(warm_inputs if warm_inputs is not None else [None] * warmup):
                if w is not None:
                    for dst, src in zip(self.static, w):
                        dst.copy_(src)
                    if target_cache is not None:
                        target_cache.select(warm_frames[i])
                optimizer.zero_grad(set_to_none=True)
                loss, _ = loss_fn(*args)
                loss.backward()
                optimizer.step()
                self.warm_losses.append(loss.detach().clone())
            if warm_inputs is not None:                       # the capture's example inputs back in the static buffers
                for dst, src in zip(self.static, [style_vectors, mask, target] + ([foreground_mask] if foreground_mask is not None else []) +
                                    ([recolor] if self._recolor else [])):
                    dst.copy_(src)
                if target_cache is not None:
                    target_cache.select(frame)
        torch.cuda.current_stream().wait_stream(self.stream)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.loss, self.recon = loss_fn(*args)
            self.loss.backward()
            optimizer.step()
        ops.invalidate_weight_caches(net)

    def __call__(self, style_vectors, mask, target, foreground_mask=None, recolor=None, frame: Optional[int] = None):
        """Copies the frame into the static buffers and replays the step; returns the (static) loss and reconstruction tensors.
        ``recolor``: the recoloured frame, iff the step was captured with one; ``frame``: the frame's index in the target cache, iff it has one."""
        if (recolor is not None) != self._recolor:
            raise ValueError("GraphedPTIStep: recolor must be given iff the step was captured with a recolor frame (without a target cache)")
        if (frame is not None) != (self.cache is not None):
            raise ValueError("GraphedPTIStep: frame must be given iff the step was captured with a target cache")
        new = [style_vectors, mask, target] + ([foreground_mask] if foreground_mask is not None else []) + ([recolor] if recolor is not None else [])
        for label, ts, key in self._watched:
            if weights_key(ts) != key:
                raise RuntimeError(f"GraphedPTIStep: the {label} weights changed after the capture (the graph reads copies prepared from the old "
                                   "ones); capture a new step")
        if len(new) != len(self.static):
            raise ValueError("foreground_mask must be given iff the step was captured with one")
        if self.cache is not None:
            self.cache.check(*self.cache_modules)
            self.cache.select(frame)
        for dst, src in zip(self.static, new):
            if dst.shape != src.shape or dst.dtype != src.dtype:
                raise ValueError(f"captured for {tuple(dst.shape)} {dst.dtype}, got {tuple(src.shape)} {src.dtype}")
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        # The replay has just moved the parameters (fused Adam inside the graph) without running any Python forward and without bumping a
        # tensor version: a re-laid-out copy cached by an earlier no_grad forward (a preview between steps) would otherwise still match
        # its key and render with the old weights.  Forgetting the copies costs a few attribute writes; the next eval rebuilds them.
        ops.invalidate_weight_caches(self.net)
        return self.loss, self.recon


def pti_step(net, optimizer: torch.optim.Optimizer, style_vectors: torch.Tensor, mask: torch.Tensor, target: torch.Tensor,
             foreground_mask: Optional[torch.Tensor] = None, l2_lambda: float = 1.0,
             extra_loss: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None, group=None, lpips=None,
             lpips_lambda: float = 0.8, id_loss=None, id_lambda: float = 0.1, face_parsing=None, face_parsing_lambda: float = 0.1,
             recolor: Optional[torch.Tensor] = None, recolor_lambda: float = 5.0):
    """One optimiser step.  ``style_vectors [bs, 12, 1280]``, ``mask`` one-hot ``[bs, 12, 512, 512]`` (or uint8 labels),
    ``target [bs, 3, 1024, 1024]`` in [-1, 1]; ``foreground_mask [bs, 1, 1024, 1024]`` restricts the loss as at :283-288.
    ``lpips``: a loaded ``criteria.lpips.LPIPS`` (or its state_dict) adds ``lpips_lambda * sum_{i<3} LPIPS(pool_i(a), pool_i(b))`` on the
    masked images ``a``, ``b`` (video_swap_ft_coach.py:188-211).  ``id_loss``: a loaded ``criteria.id_loss.IDLoss`` (or a ``Backbone``
    state_dict) adds ``id_lambda * IDLoss(a, b)`` (:192-195).  ``face_parsing``: a loaded ``criteria.face_parsing.face_parsing_loss.FaceParsingLoss``
    (or a ``unet`` state_dict) adds ``face_parsing_lambda * FaceParsingLoss(a, b)`` (:212-216).  ``extra_loss(recon, target)`` gets the unmasked images.
    ``recolor [bs, 3, H, W]`` (the recoloured driven frame, ``D_recolor_%04d.png``): adds ``recolor_lambda`` x the same terms against it, always under
    the foreground weight (video_swap_ft_coach.py:274-287) — ``foreground_mask``, or without one the weight ``prepare_clip`` computes from ``mask``.
    Inside a ``torch.distributed`` process group every rank passes its own frame and the gradients are averaged before the update.
    Returns ``(loss value, reconstruction)``."""
    _check_loaded(_terms(lpips=lpips, id_loss=id_loss, face_parsing=face_parsing))
    if recolor is not None:
        _check_recolor(recolor, target, "pti_step")
        loss, recon = _loss_recolor(net, style_vectors, mask, target, foreground_mask, l2_lambda, extra_loss, True, lpips, lpips_lambda, id_loss,
                                    id_lambda, face_parsing, face_parsing_lambda, recolor, recolor_lambda)
    else:
        loss, recon = _loss(net, style_vectors, mask, target, foreground_mask, l2_lambda, extra_loss, True,   # the coach calls gen_img with fresh noise
                            lpips, lpips_lambda, id_loss, id_lambda, face_parsing, face_parsing_lambda)
    optimizer.zero_grad()
    loss.backward()
    sync_gradients([p for g in optimizer.param_groups for p in g["params"]], group)
    optimizer.step()
    return loss.detach(), recon.detach()


def style_vector_step(net, optimizer: torch.optim.Optimizer, latent: torch.Tensor, mask: torch.Tensor, target: torch.Tensor,
                      l2_lambda: float = 1.0, extra_loss: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None,
                      randomize_noise: bool = True, lpips=None, lpips_lambda: float = 0.8, id_loss=None, id_lambda: float = 0.1, face_parsing=None,
                      face_parsing_lambda: float = 0.1):
    """One step of the reference's W-optimisation (``Optimizer.optim_W_online``, optimization.py:321-349): the per-region style
    vectors ``latent [bs, 12, 1280]`` (``requires_grad``, held by ``optimizer``) are tuned so that ``gen_img(cal_style_codes(latent))``
    matches ``target``; the network's own parameters are left alone (they are not in ``optimizer``).  ``lpips``: adds
    ``lpips_lambda * sum_{i<3} LPIPS(pool_i(recon), pool_i(target))`` on the unmasked images (optimization.py:111-146); ``id_loss``:
    ``id_lambda * IDLoss(recon, target)``, unmasked as well (optimization.py:115); ``face_parsing``: ``face_parsing_lambda *
    FaceParsingLoss(recon, target)``, unmasked (optimization.py:135-139)."""
    _check_loaded(_terms(lpips=lpips, id_loss=id_loss, face_parsing=face_parsing))
    optimizer.zero_grad()
    loss, recon = _loss(net, latent, mask, target, None, l2_lambda, extra_loss, randomize_noise, lpips, lpips_lambda, id_loss, id_lambda,
                        face_parsing, face_parsing_lambda)
    loss.backward()
    optimizer.step()
    return loss.detach(), recon.detach()


# ------------------------------------------------------------------------------------------------ the PTI loop over a clip (BASELINE configs[3])
def prepare_clip(labels: torch.Tensor, erode_radius: Optional[int] = None, size=(1024, 1024)):
    """Per-frame masks of the PTI loop (training/video_swap_ft_coach.py:257-279), computed once for the clip on the device:
    the region map the synthesis runs on — ``erode_mask(driven_m, radius)`` when the coach erodes (:259-263), else the map itself — and the
    loss's foreground weight, ``not {background, hair, ear-rings}`` of THAT map, bilinearly resized to 1024 x 1024 (:277-280).
    ``labels``: uint8 ``[n, 512, 512]`` 12-class maps; ``size``: the images' (H, W).  Returns ``(maps uint8 [n, 512, 512], foreground float [n, 1, H, W])``."""
    maps = ops.erode_labels(labels, erode_radius) if erode_radius else ops._labels_u8(labels, "labels")
    fg = torch.ones_like(maps, dtype=torch.float32)
    for c in ops.PTI_BG_CLASSES:
        fg = fg * (maps != c)
    fg = ops.bilinear_resize(fg[:, None].contiguous(), tuple(size), align_corners=False)
    return maps, fg


def tune_clip(net, optimizer, images: torch.Tensor, labels: torch.Tensor, style_vectors: torch.Tensor, steps: int,
              erode_radius: Optional[int] = None, l2_lambda: float = 1.0, extra_loss=None, group=None, graphed: Optional[bool] = None,
              randomize_noise: bool = True, step_fn=None, on_epoch=None, local_only: bool = False, lpips=None, lpips_lambda: float = 0.8,
              id_loss=None, id_lambda: float = 0.1, face_parsing=None, face_parsing_lambda: float = 0.1, recolor: Optional[torch.Tensor] = None,
              recolor_lambda: float = 5.0, cache_targets: bool = True):
    """The fine-tuning loop of ``VideoSwapPTICoach.train_e4s`` (training/video_swap_ft_coach.py:242-317) for the part on the hot path:
    ``steps`` passes over the clip's frames, one optimiser step per frame — ``cal_style_codes`` -> ``gen_img`` on the (eroded) region map ->
    L2 against the frame under the foreground weight (+ ``lpips_lambda`` x the three-scale LPIPS-AlexNet term when ``lpips`` is given,
    + ``id_lambda`` x the ArcFace identity term when ``id_loss`` is given, + ``face_parsing_lambda`` x the face-parsing term when ``face_parsing``
    is given, + ``extra_loss``) ->
    backward -> Adam.  ``images [n, 3, 1024, 1024]`` in [-1, 1], ``labels`` uint8 ``[n, 512, 512]``, ``style_vectors [n, 12, 1280]``.

    Several GPUs (BASELINE configs[3]: 32 frames on 4 GPUs): every rank holds the whole clip's inputs or at least its own block; rank ``r``
    tunes on frames ``shard_range(n, r, world)`` and round ``i`` of a pass = every rank's ``i``-th frame, gradients averaged over the ranks
    that still have one (``sync_gradients``) — a batch-of-N step, so the parameters stay identical on all ranks (not the reference's N
    sequential steps: no parity claim for this mode).  A rank whose block is shorter takes part in the remaining rounds with no gradient.

    Single GPU: the step runs as one replayed hipGraph (``GraphedPTIStep``) unless ``graphed=False``.
    ``local_only``: ignore an initialised process group (this rank tunes on the frames it is given, no collective) — the pre-flight step of
    ``bench.py``'s multi-GPU section.
    ``recolor [n, 3, 1024, 1024]``: the recoloured driven frames (``D_recolor_%04d.png``); adds ``recolor_lambda`` x the same terms against them under
    the foreground weight (video_swap_ft_coach.py:274-287).  The reconstruction side is shared by both targets, and with ``cache_targets`` the
    target side (both frames' features in every loss network) is computed once for this rank's frames (``TargetCache``) instead of on every step.
    ``step_fn(net, optimizer, vec, map, image, fg, group, active) -> loss`` replaces the step (tests); with ``recolor`` it also gets the frame's
    ``recolor=`` as a keyword.  Returns the mean loss of each pass."""
    from .runner import shard_range
    _check_loaded(_terms(lpips=lpips, id_loss=id_loss, face_parsing=face_parsing))
    distributed = (not local_only) and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    n = images.shape[0]
    if labels.shape[0] != n or style_vectors.shape[0] != n:
        raise ValueError("tune_clip: images, labels and style vectors must describe the same frames")
    _check_recolor(recolor, images, "tune_clip")
    lo, hi = shard_range(n, rank, world)
    rounds = max(shard_range(n, r, world)[1] - shard_range(n, r, world)[0] for r in range(world))
    if step_fn is None:
        maps, fgs = prepare_clip(labels[lo:hi].contiguous(), erode_radius, images.shape[-2:])
    else:
        maps, fgs = labels[lo:hi], [None] * (hi - lo)
    if graphed is None:
        graphed = not distributed and step_fn is None and hi > lo
    cache = None
    if recolor is not None and cache_targets and step_fn is None and hi > lo:
        cache = TargetCache([images[lo:hi], recolor[lo:hi]], fgs, lpips, id_loss, face_parsing)
    rec = (lambda i: recolor[lo + i:lo + i + 1]) if recolor is not None else None                       # noqa: E731
    params = [p for g in optimizer.param_groups for p in g["params"]]
    step = None
    if graphed and distributed:
        raise ValueError("tune_clip: the graph-captured step has no gradient exchange; use graphed=False with several ranks")
    # A capture needs an initialised optimiser state, library handles and allocator pools on its stream: GraphedPTIStep runs warm-up steps
    # eagerly on the capture stream first.  Here those ARE the loop's first two steps (frames 0, 1 of the first pass), not extra ones.
    EAGER_FIRST = min(2, steps * rounds - 1) if graphed else 0
    sched = [(e, i) for e in range(steps) for i in range(rounds)]
    warm_losses = []
    if graphed:
        static_rec = rec is not None and cache is None
        frame = lambda i: (style_vectors[lo + i:lo + i + 1], maps[i:i + 1], images[lo + i:lo + i + 1], fgs[i:i + 1]) + \
            ((rec(i),) if static_rec else ())                                                                   # noqa: E731
        ex_i = sched[EAGER_FIRST][1]
        ex = frame(ex_i)
        step = GraphedPTIStep(net, optimizer, ex[0], ex[1], ex[2], ex[3], l2_lambda, extra_loss, randomize_noise,
                              warm_inputs=[frame(i) for _, i in sched[:EAGER_FIRST]], lpips=lpips, lpips_lambda=lpips_lambda,
                              id_loss=id_loss, id_lambda=id_lambda, face_parsing=face_parsing, face_parsing_lambda=face_parsing_lambda,
                              recolor=ex[4] if static_rec else None, recolor_lambda=recolor_lambda, target_cache=cache,
                              frame=ex_i if cache is not None else None, warm_frames=[i for _, i in sched[:EAGER_FIRST]] if cache is not None else None)
        warm_losses = list(step.warm_losses)
    done = 0
    history = []
    for epoch in range(steps):
        losses = []
        for i in range(rounds):
            f = lo + i
            have = f < hi
            active = sum(1 for r in range(world) if shard_range(n, r, world)[0] + i < shard_range(n, r, world)[1])
            done += 1
            if graphed and done <= EAGER_FIRST:                # already taken (eagerly, on the capture stream)
                losses.append(warm_losses[done - 1])
                continue
            if step_fn is not None:
                kw = {"recolor": recolor[f:f + 1] if have else None} if recolor is not None else {}
                loss = step_fn(net, optimizer, style_vectors[f:f + 1] if have else None, maps[i:i + 1] if have else None,
                               images[f:f + 1] if have else None, None, group, active, **kw)
            elif step is not None:
                loss = step(style_vectors[f:f + 1], maps[i:i + 1], images[f:f + 1], fgs[i:i + 1], recolor=rec(i) if static_rec else None,
                            frame=i if cache is not None else None)[0].clone()
            else:
                optimizer.zero_grad(set_to_none=True)
                loss = None
                if have and recolor is not None:
                    if cache is not None:
                        cache.check(lpips, id_loss, face_parsing)
                        cache.select(i)
                    loss, _ = _loss_recolor(net, style_vectors[f:f + 1], maps[i:i + 1], images[f:f + 1], fgs[i:i + 1], l2_lambda, extra_loss,
                                            randomize_noise, lpips, lpips_lambda, id_loss, id_lambda, face_parsing, face_parsing_lambda,
                                            recolor[f:f + 1], recolor_lambda, cache)
                    loss.backward()
                elif have:
                    loss, _ = _loss(net, style_vectors[f:f + 1], maps[i:i + 1], images[f:f + 1], fgs[i:i + 1], l2_lambda, extra_loss, randomize_noise,
                                    lpips, lpips_lambda, id_loss, id_lambda, face_parsing, face_parsing_lambda)
                    loss.backward()
                if distributed:
                    sync_gradients(params, group, active_ranks=active)
                optimizer.step()
            if loss is not None:
                losses.append(loss.detach() if isinstance(loss, torch.Tensor) else torch.tensor(float(loss)))
        mean = torch.stack([l.float().reshape(()) for l in losses]).mean().item() if losses else float("nan")
        history.append(mean)
        if on_epoch is not None:
            on_epoch(epoch, mean)
    return history
