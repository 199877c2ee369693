"""Batched full-swap unit on the device: per face
    2 x parse (BiSeNet, 19 -> 12 classes) + 2 x get_style_vectors + style-vector mix + cal_style_codes + gen_img (+ tensor2im)
which is what ``face_swap_video_pipeline.py`` does per frame between its CPU stages (:212-219 parsing, :332-354 style vectors,
:429-443 mix + synthesis), here for a whole batch without leaving the GPU.  With ``mask_surgery=True`` the synthesis is driven by
``swap_head_mask_hole_first(driven_map, target_map)`` as at face_swap_video_pipeline.py:420 (row f2, ``ops.swap_head_mask``) and the
paste-back masks of :456-463 (row f3, ``ops.foreground_masks``) are returned too; the default keeps BASELINE configs[2]'s unit of
work, where the target's own region map drives the synthesis.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from . import netweights, ops, ops_post, ops_recolor

DEFAULT_COMP_INDICES = tuple(sorted(set(range(12)) - {0, 4, 11}))      # face_swap_video_pipeline.py:436: keep target background, hair, ear-rings
# the two-image caller (Face_swap_with_two_imgs.py:469-472): it also keeps the target's eye glasses (10) and, with colour transfer, its neck and ears
IMAGE_COMP_INDICES = tuple(sorted(set(range(12)) - {0, 10, 4, 11}))
IMAGE_COMP_INDICES_CT = tuple(sorted(set(range(12)) - {0, 10, 4, 8, 7, 11}))


TWO_STREAMS = True               # (module attributes; ``swap_batch`` also takes them as arguments)
_sel_cache = {}
_side = {}


SWAP_CHAINS = 2     # 2 = driven | target; 4 = each additionally split into half batches
# Driven and target faces as ONE batch of 2*bs through parser and encoder (default): the 32x32 and 16x16 stages of the encoder and the
# launch-bound glue between its convolutions fill the chip better at twice the batch than as two concurrent chains (measured at bs 8:
# parse + encode 4.3 + 13.7 ms for 16 images against 2 x (2.5 + 8.1) ms on one stream and 21.0 ms on two streams).
SWAP_BATCHED = True
PARSE_BESIDE_ENCODE = True    # (batched route) the face parser on a side stream next to the encoder body
ENCODE_ISSUED_FIRST = os.environ.get("E4S_SWAP_ENC_FIRST", "1") != "0"     # (with PARSE_BESIDE_ENCODE) host issue order: encoder body, then the parser


def _side_stream(device, idx=0):
    key = (str(device), idx)
    st = _side.get(key)
    if st is None:
        st = _side[key] = torch.cuda.Stream(device=device)
    return st


def _selector(device, comp_indices, n):
    """bool [n] on ``device`` marking the components taken from the driven face; built once per (device, indices) so that no
    host-to-device copy happens inside a hipGraph capture."""
    key = (str(device), tuple(comp_indices), n)
    sel = _sel_cache.get(key)
    if sel is None:
        m = torch.zeros(n, dtype=torch.bool)
        m[list(comp_indices)] = True
        sel = _sel_cache[key] = m.to(device)
    return sel


def mix_style_vectors(target_vec: torch.Tensor, driven_vec: torch.Tensor, comp_indices: Sequence[int] = DEFAULT_COMP_INDICES,
                      below_face_interpolation: bool = False, ear_interpolation: bool = True) -> torch.Tensor:
    """``swap_comp_style_vector`` (swap_face_fine/swap_face_mask.py:336-367) for a batch, without host synchronisation:
    take the listed components from the driven face; ears (7) = mean of both; ear-rings (11) from the target; neck (8) optionally the
    mean; teeth (9) from the target when the driven face has none (its style vector sums to exactly 0).
    ``ear_interpolation=False``: the two-image caller's ``_swap_comp_style_vector`` (Face_swap_with_two_imgs.py:416-453), which does not
    average the ears: they follow ``comp_indices`` like any other component."""
    sel = _selector(target_vec.device, comp_indices, target_vec.shape[1])
    out = torch.where(sel[None, :, None], driven_vec, target_vec)
    if ear_interpolation:
        out[:, 7, :] = (target_vec[:, 7, :] + driven_vec[:, 7, :]) / 2
    out[:, 11, :] = target_vec[:, 11, :]
    if below_face_interpolation:
        out[:, 8, :] = (target_vec[:, 8, :] + driven_vec[:, 8, :]) / 2
    no_teeth = (driven_vec[:, 9, :].sum(dim=1, keepdim=True) == 0)
    out[:, 9, :] = torch.where(no_teeth, target_vec[:, 9, :], out[:, 9, :])
    return out


@torch.no_grad()
def swap_batch(net, parser, driven: torch.Tensor, target: torch.Tensor, comp_indices: Sequence[int] = DEFAULT_COMP_INDICES,
               randomize_noise: bool = False, to_uint8: bool = True, timings: Optional[dict] = None, mask_surgery: bool = False,
               paste_radius: int = 5, two_streams: Optional[bool] = None, batched: Optional[bool] = None, guard: Optional[list] = None,
               ear_interpolation: bool = True):
    """``driven`` / ``target``: ``[bs, 3, 1024, 1024]`` in [-1, 1] on the device.  Returns uint8 ``[bs, 1024, 1024, 3]`` frames
    (or the float image) and the 12-class region maps the synthesis used; with ``mask_surgery`` a third value
    ``{"hole_mask", "hole_map", "lines", "content", "border", "full", "target_labels"}`` (the reference's paste-back inputs, :456-463, and the
    target's own 12-class map, which the image caller's colour transfer needs).
    ``ear_interpolation`` goes to ``mix_style_vectors``.

    f16 range (``ops.MxGuard``): parser, encoder and the masked synthesis layers run in f16-based split arithmetic.  The batch is bracketed by ONE
    guard; by default the call waits for it at its end and re-runs the whole batch in the split-bf16 arithmetic if a value left the f16 range
    (``ops.mx_fallbacks`` counts those).  Callers that keep several batches in flight pass ``guard=[]``: the armed guard is appended instead of
    awaited, and the caller checks ``guard[-1].tripped()`` where it synchronises anyway, repeating the call under ``with ops.mx_exact():``."""
    args = (net, parser, driven, target, comp_indices, randomize_noise, to_uint8, timings, mask_surgery, paste_radius, two_streams, batched, ear_interpolation)
    if guard is None and ops.mx_guard_owned():        # a caller up the stack brackets this batch with its own guard (runner.run_clip_streamed, bench.py)
        return _swap_batch_once(*args)
    with ops.mx_guard_scope() as g:
        out = _swap_batch_once(*args)
        g.arm()
    if guard is not None:
        guard.append(g)
        return out
    if g.tripped():
        ops.mx_fallbacks += 1
        with ops.mx_exact():        # (the exact re-run leaves the caller's `timings` alone: its stage marks belong to the first pass)
            out = _swap_batch_once(net, parser, driven, target, comp_indices, randomize_noise, to_uint8, None, mask_surgery, paste_radius, two_streams, batched,
                                   ear_interpolation)
    return out


def _swap_batch_once(net, parser, driven, target, comp_indices, randomize_noise, to_uint8, timings, mask_surgery, paste_radius, two_streams, batched,
                     ear_interpolation=True):
    def mark(name):
        if timings is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            timings.setdefault("_events", []).append((name, ev))
    mark("start")
    if batched is None:
        batched = SWAP_BATCHED and two_streams is None                 # an explicit two_streams= argument (True or False) selects the unbatched routes
    if two_streams is None:
        two_streams = TWO_STREAMS
    if batched:
        bs = driven.shape[0]
        enc = getattr(net, "encoder", None)
        if PARSE_BESIDE_ENCODE and hasattr(enc, "features"):
            # the encoder needs the region maps only for its last step (masked average pooling): the parser runs on a side stream next to
            # the encoder's body.  Driven and target faces go through both as ONE batch, but the 2 x bs full-size images are never concatenated,
            # shifted to [0, 1] or copied: the two down-sampling kernels in front of parser and encoder read them where they are.
            main, side = torch.cuda.current_stream(), _side_stream(driven.device, 0)

            def parse_on_side():
                with torch.cuda.stream(side):
                    out = parser.parse_batch((driven, target), seg12=True, pm1=True)   # uint8 [2 bs, 512, 512]
                driven.record_stream(side)
                target.record_stream(side)
                return out
            if ENCODE_ISSUED_FIRST:
                # the encoder body is the critical path of a batch (9 ms against the parser's 3): its launches are issued first, the parser's ~40 behind them —
                # the other way round the encoder's first kernel waits for the HOST to have issued the whole parser
                inputs_ready = torch.cuda.Event()
                inputs_ready.record(main)
            else:
                side.wait_stream(main)
                lab = parse_on_side()
            small = torch.empty((2 * bs, driven.shape[1], 256, 256), dtype=torch.float32, device=driven.device)
            ops.bilinear_resize(driven, (256, 256), align_corners=False, out=small[:bs])             # Net3._encode (networks.py:217)
            ops.bilinear_resize(target, (256, 256), align_corners=False, out=small[bs:])
            taps = enc.features(small)
            if ENCODE_ISSUED_FIRST:
                side.wait_event(inputs_ready)
                lab = parse_on_side()
            main.wait_stream(side)
            lab.record_stream(main)
            vec, _ = enc.codes(taps, lab)
        else:
            both = torch.cat([driven, target])
            lab = parser.parse_batch(both, seg12=True, pm1=True)          # uint8 [2 bs, 512, 512]
            vec, _ = net.get_style_vectors(both, lab)
        lab_d, lab_t, vec_d, vec_t = lab[:bs], lab[bs:], vec[:bs], vec[bs:]
        mark("parse+encode_x2")
    elif two_streams:
        # The driven and the target face are independent until the style-vector mix: run the parse -> encode chains on separate HIP
        # streams so that the launch-bound glue kernels and short-K convolutions of one fill the idle CUs of the others.
        main = torch.cuda.current_stream()
        bs = driven.shape[0]
        halves = SWAP_CHAINS // 2 if (SWAP_CHAINS >= 4 and bs % (SWAP_CHAINS // 2) == 0) else 1
        step = bs // halves
        jobs = [(img, i * step, (i + 1) * step) for img in (driven, target) for i in range(halves)]
        outs = []
        for j, (img, lo, hi) in enumerate(jobs):
            st = main if j == len(jobs) - 1 else _side_stream(driven.device, j)
            if st is not main:
                st.wait_stream(main)
            with torch.cuda.stream(st):
                part = img[lo:hi]
                lab = parser.parse_batch((part + 1) / 2, seg12=True)
                vec, _ = net.get_style_vectors(part, lab)
            outs.append((lab, vec, st))
        for lab, vec, st in outs:
            if st is not main:
                main.wait_stream(st)
                lab.record_stream(main)
                vec.record_stream(main)
        lab_d = torch.cat([o[0] for o in outs[:halves]]) if halves > 1 else outs[0][0]
        vec_d = torch.cat([o[1] for o in outs[:halves]]) if halves > 1 else outs[0][1]
        lab_t = torch.cat([o[0] for o in outs[halves:]]) if halves > 1 else outs[1][0]
        vec_t = torch.cat([o[1] for o in outs[halves:]]) if halves > 1 else outs[1][1]
        mark("parse+encode_x2")
    else:
        lab_d = parser.parse_batch((driven + 1) / 2, seg12=True)          # uint8 [bs, 512, 512]
        lab_t = parser.parse_batch((target + 1) / 2, seg12=True)
        mark("parse_x2")
        vec_d, _ = net.get_style_vectors(driven, lab_d)
        vec_t, _ = net.get_style_vectors(target, lab_t)
        mark("encode_x2")
    codes = net.cal_style_codes(mix_style_vectors(vec_t, vec_d, comp_indices, ear_interpolation=ear_interpolation))
    mark("mix+mlps")
    extra = None
    lab = lab_t
    if mask_surgery:
        lab, hole, hole_map, lines = ops.swap_head_mask(lab_d, lab_t)
        content, border, full = ops.foreground_masks(lab, hole, paste_radius)
        extra = {"hole_mask": hole, "hole_map": hole_map, "lines": lines, "content": content, "border": border, "full": full, "target_labels": lab_t}
        mark("mask_surgery")
    img, _, _ = net.gen_img(None, codes, lab, randomize_noise=randomize_noise)
    mark("gen_img")
    out = ops.tensor2im_u8(img) if to_uint8 else img
    mark("tensor2im")
    return (out, lab) if extra is None else (out, lab, extra)


@torch.no_grad()
def paste_back(swapped_u8: torch.Tensor, target_u8: torch.Tensor, content: torch.Tensor, border: torch.Tensor, soften: bool = True) -> torch.Tensor:
    """The reference's "past back" of a swapped face into its target crop (face_swap_video_pipeline.py:447, 464-473), on the device:

        swapped -> PIL resize to 512 x 512 and back to 1024 x 1024 (default BICUBIC; ``soften``, :447), bit-exact with Pillow
        content, border -> bilinear to the frame size (align_corners=False)
        pasted = swapped * content + T * (1 - content)
        out    = blending(T, pasted, mask=border)             (swap_face_fine/multi_band_blending.py:51-74, ten pyramid levels)

    ``swapped_u8`` / ``target_u8``: uint8 ``[bs, 1024, 1024, 3]`` (what ``swap_batch`` returns / the aligned target crop); ``content`` /
    ``border``: float ``[bs, 1, h, w]`` from ``swap_batch(..., mask_surgery=True)``.  Returns uint8 ``[bs, 1024, 1024, 3]``.
    """
    if swapped_u8.dtype != torch.uint8 or target_u8.dtype != torch.uint8 or swapped_u8.shape != target_u8.shape or swapped_u8.shape[-1] != 3:
        raise ValueError("paste_back: swapped and target frames are uint8 [bs, H, W, 3] of the same shape")
    bs, h, w, _ = swapped_u8.shape
    if soften:
        swapped_u8 = ops.pil_resize(ops.pil_resize(swapped_u8, (512, 512)), (w, h))
    t = target_u8.permute(0, 3, 1, 2).contiguous()
    sw = swapped_u8.permute(0, 3, 1, 2).float()
    cm = ops.bilinear_resize(content.float().contiguous(), (h, w), align_corners=False)
    bm = ops.bilinear_resize(border.float().contiguous(), (h, w), align_corners=False)
    pasted = torch.lerp(t.float(), sw, cm)                       # swapped * content + T * (1 - content)
    return ops.blending(t, pasted, bm).permute(0, 2, 3, 1).contiguous()


@torch.no_grad()
def swap_frames(net, parser, driven: torch.Tensor, target_frames_u8: torch.Tensor, plan, **swap_batch_kwargs) -> torch.Tensor:
    """The video pipeline's per-frame loop with ``use_crop=True`` (face_swap_video_pipeline.py:181-210, 404-483) for a batch of video frames:

        crop_align (row f5) -> frames_to_tensor -> swap_batch(mask_surgery=True) -> paste_back -> paste_into_frames (row f5)

    ``driven``: ``[n, 3, 1024, 1024]`` in [-1, 1] as for ``swap_batch``; ``target_frames_u8``: uint8 ``[n, H, W, 3]`` video frames on the device;
    ``plan``: their ``align.CropPlan`` (``align.plan_from_landmarks``).  Returns uint8 ``[n, H, W, 3]``: the frames with the swapped faces
    pasted in, every pixel outside the faces' quads untouched.  Further keyword arguments go to ``swap_batch`` (its f16 guard and stream
    behaviour apply: with ``guard=[]`` the caller checks the guard and repeats the call).  As a ``synth_fn`` of ``runner.run_clip_streamed``:
    ``lambda shared, i: swap_frames(net, parser, *i)`` with ``frame_inputs(lo, hi) = (driven[lo:hi], frames[lo:hi], plan[lo:hi])``."""
    for k in ("mask_surgery", "to_uint8"):
        if k in swap_batch_kwargs:
            raise TypeError(f"swap_frames: {k} is fixed (the paste needs the uint8 face and the mask-surgery paste masks)")
    crops = ops.crop_align(target_frames_u8, plan)
    target = ops.frames_to_tensor(crops)
    swapped, _, extra = swap_batch(net, parser, driven, target, mask_surgery=True, **swap_batch_kwargs)
    blended = paste_back(swapped, crops, extra["content"], extra["border"])
    return ops.paste_into_frames(blended, target_frames_u8, plan)


# ------------------------------------------------------------------------------------ f6: the two-image caller (Face_swap_with_two_imgs.py)
def _crops_checked(name, *frames):
    a = frames[0]
    for f in frames:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 or f.shape != a.shape:
            raise ValueError(f"{name}: the frames are uint8 [bs, H, W, 3] of one shape")


@torch.no_grad()
def paste_back_soft(swapped_u8: torch.Tensor, target_u8: torch.Tensor, labels: torch.Tensor, hole_mask: Optional[torch.Tensor] = None,
                    radius: int = 2) -> torch.Tensor:
    """The image caller's ``_past_back`` (Face_swap_with_two_imgs.py:159-219) up to its multi-band blend, on the device:

        content, border = soft_paste_masks(labels, hole_mask, radius)    (:177-191; every mask through SoftErosion, radius 2 where the video uses 5)
        content, border -> bilinear to the frame size (align_corners=False)                                                      (:202-206)
        pasted = uint8(swapped * content + T * (1 - content))            (:216-217; truncated to 8 bits, no 512 x 512 Pillow round trip)
        out    = blending(T, pasted, mask=border)                        (:218-219)

    ``swapped_u8`` / ``target_u8``: uint8 ``[bs, 1024, 1024, 3]``; ``labels`` / ``hole_mask``: uint8 ``[bs, h, w]`` (the swapped map and hole of
    ``swap_batch(..., mask_surgery=True)``).  Returns uint8 ``[bs, 1024, 1024, 3]``."""
    _crops_checked("paste_back_soft", swapped_u8, target_u8)
    bs, h, w, _ = swapped_u8.shape
    content, border, _ = ops.soft_paste_masks(labels, hole_mask, radius)
    if content.shape[0] != bs:
        raise ValueError(f"paste_back_soft: {content.shape[0]} label maps for {bs} frames")
    if bs == 0:
        return torch.empty_like(target_u8)
    cm = ops.bilinear_resize(content, (h, w), align_corners=False)
    bm = ops.bilinear_resize(border, (h, w), align_corners=False)
    pasted = ops.blend_with_mask(target_u8, swapped_u8, cm, 1.0)
    t = target_u8.permute(0, 3, 1, 2).contiguous()
    return ops.blending(t, pasted.permute(0, 3, 1, 2).float(), bm).permute(0, 2, 3, 1).contiguous()


@torch.no_grad()
def color_blend(swapped_u8: torch.Tensor, recolored_u8: torch.Tensor, labels: torch.Tensor, edge: Optional[torch.Tensor] = None,
                up_ratio: float = 0.75) -> torch.Tensor:
    """Step 2 of ``face_swap_pipeline`` (Face_swap_with_two_imgs.py:912-924): the colour-transferred face blended over the swapped one,

        mask = clip(facial_mask12(labels, frame size) - edge, 0, 1);   out = blend_with_mask(swapped, recolored, mask, up_ratio)

    ``edge``: the caller's ``Trick.get_edge(swapped)`` image scaled to [0, 1] as a float ``[bs, H, W]`` or ``[bs, 1, H, W]`` tensor (the edge
    detector is cv2 code and stays with the caller), or None for no high-frequency cut-out."""
    _crops_checked("color_blend", swapped_u8, recolored_u8)
    bs, h, w, _ = swapped_u8.shape
    mask = ops.facial_mask12(labels, (h, w))
    if edge is not None:
        if not isinstance(edge, torch.Tensor) or not edge.is_floating_point() or edge.numel() != bs * h * w:
            raise ValueError(f"color_blend: edge is a float [{bs}, 1, {h}, {w}] tensor in [0, 1]")
        mask = (mask - edge.to(mask.dtype).reshape(mask.shape)).clamp_(0, 1)
    return ops.blend_with_mask(swapped_u8, recolored_u8, mask, up_ratio)


CT_FACE_CLASSES = (1, 2, 3, 5, 6, 9, 7, 8)        # _color_transfer's face (Face_swap_with_two_imgs.py:540-541): facial_mask12's classes plus the ears
CT_BORDER_RADIUS = 10                             # :549


@torch.no_grad()
def color_transfer(swapped_u8: torch.Tensor, target_u8: torch.Tensor, swapped_labels: torch.Tensor, target_labels: torch.Tensor,
                   ct_mode: str = "lct") -> torch.Tensor:
    """The arithmetic branch of the image caller's ``_color_transfer`` (Face_swap_with_two_imgs.py:537-572) for ``ct_mode`` 'lct' / 'mkl', on the device:

        md, mt = the face classes of the swapped / the target map, bilinear to the frame size (align_corners=False)                  (:540-547)
        border = soft_expansion_masks(md, radius 10)[1]                                                                             (:549)
        composed, _ = skin_color_transfer(D, T, md, mt, ct_mode)                                                                    (:555-568)
        out = blending(D, composed, mask=border)                                                                                    (:570)

    ``swapped_u8`` (D) / ``target_u8`` (T): uint8 ``[bs, 1024, 1024, 3]``; the maps uint8 ``[bs, h, w]`` (``lab`` and ``extra["target_labels"]`` of
    ``swap_batch(..., mask_surgery=True)``).  Returns uint8 ``[bs, 1024, 1024, 3]``.  No host synchronisation; capturable in a hipGraph.  The reference's
    default mode (the Blender network) and its cv2 / random-rotation modes raise ``ValueError``."""
    ops_post._ct_mode_checked(ct_mode, "color_transfer")
    _crops_checked("color_transfer", swapped_u8, target_u8)
    bs, h, w, _ = swapped_u8.shape
    ld, lt = ops._labels_u8(swapped_labels, "swapped_labels"), ops._labels_u8(target_labels, "target_labels")
    if ld.shape != lt.shape or ld.shape[0] != bs:
        raise ValueError(f"color_transfer: {tuple(ld.shape)} and {tuple(lt.shape)} label maps for {bs} frames")
    if bs == 0:
        return torch.empty_like(swapped_u8)
    lut = ops_post._class_lut(CT_FACE_CLASSES, ld.device)
    both = lut[torch.cat([ld, lt]).long()][:, None]
    both = ops.bilinear_resize(both, (h, w), align_corners=False) if tuple(both.shape[-2:]) != (h, w) else both
    md, mt = both[:bs], both[bs:]
    border = ops.soft_expansion_masks(md, CT_BORDER_RADIUS)[1]
    composed, _ = ops.skin_color_transfer(swapped_u8, target_u8, md, mt, ct_mode, with_q=False)
    d = swapped_u8.permute(0, 3, 1, 2).contiguous()
    return ops.blending(d, composed, border).permute(0, 2, 3, 1).contiguous()


def _recolor_nets_checked(ct_mode, recolor_fn, recolor_nets):
    """``(blender, esr)`` for ``ct_mode='blender'``, their layouts and keys checked, or None; ``TypeError`` where ``recolor_nets`` does not belong."""
    if recolor_nets is None:
        return None
    if recolor_fn is not None:
        raise TypeError("swap_images: recolor_nets and recolor_fn are two ways to do step 2, the colour transfer: pass one of them")
    if ct_mode != "blender":
        raise TypeError(f"swap_images: recolor_nets goes with ct_mode='blender' (the other modes are arithmetic), got ct_mode={ct_mode!r}")
    if not isinstance(recolor_nets, (tuple, list)) or len(recolor_nets) != 2:
        raise TypeError("swap_images: recolor_nets is the pair (blender, esr): the recolouring network's weights and the Real-ESRGAN network's")
    blender, esr = recolor_nets
    ops_recolor._blender_weights("swap_images", blender)                # both fail here, before the crop and the swap are launched
    ops_recolor.rrdbnet_weight_tensors(esr, "swap_images")
    return blender, esr


@torch.no_grad()
def swap_images(net, parser, driven: torch.Tensor, target_images_u8: torch.Tensor, plan, recolor_fn=None, ct_mode: Optional[str] = None,
                recolor_nets=None, **swap_batch_kwargs) -> torch.Tensor:
    """The two-image caller's chain (``FaceSwap.face_swap_pipeline``, Face_swap_with_two_imgs.py:796-963, without its GPEN network and without its
    inpainting step, whose network and ``inpainting()`` are ``inpaint_faces`` below while the rest of ``_inpaint_face`` is not built yet: row f25, stage 2) for a batch of target images, all on the device:

        crop_align -> frames_to_tensor -> swap_batch(mask_surgery=True, ear_interpolation=False, comp_indices=IMAGE_COMP_INDICES[_CT])
        [-> color_blend(swapped, recolored, labels)]                                   (:909-924, when ``ct_mode`` or ``recolor_fn`` is given)
        -> paste_back_soft(swapped map, hole)                                          (:938)
        -> paste_back_soft(all-skin rectangle map, no hole)                            (:883, :958)
        -> paste_into_frames

    ``driven``: ``[n, 3, 1024, 1024]`` in [-1, 1]; ``target_images_u8``: uint8 ``[n, H, W, 3]`` on the device; ``plan``: their ``align.CropPlan``;
    ``ct_mode`` 'lct' / 'mkl': step 2 on the device, ``recolored = color_transfer(swapped, crops, swapped map, target map, ct_mode)``;
    ``recolor_fn(swapped_u8, crops_u8) -> uint8 [n, 1024, 1024, 3]``: a colour transfer of the caller's own instead (the reference's other modes need cv2
    or a network); passing both raises ``TypeError``.  ``ct_mode='blender'`` with ``recolor_nets=(blender, esr)``: the reference's default mode,
    ``recolored = color_transfer_blender(swapped, crops, parser, blender, esr)`` (the recolouring network and the Real-ESRGAN step, rows f8 - f11, with the
    weights as ``ops.blender_forward`` and ``ops.realesr_forward`` take them); without ``recolor_nets`` that mode raises ``ValueError``, and ``recolor_nets``
    with any other mode or with ``recolor_fn`` raises ``TypeError``.  Returns uint8 ``[n, H, W, 3]``, every pixel outside the faces' quads untouched.  Further keyword arguments go to ``swap_batch``, with the guard and stream behaviour of ``swap_frames``."""
    for k in ("mask_surgery", "to_uint8", "ear_interpolation", "comp_indices"):
        if k in swap_batch_kwargs:
            raise TypeError(f"swap_images: {k} is fixed (the image caller's style mix, and the paste needs the uint8 face and the mask-surgery hole)")
    if ct_mode is not None and recolor_fn is not None:
        raise TypeError("swap_images: ct_mode and recolor_fn are two ways to do step 2, the colour transfer: pass one of them")
    blender_nets = _recolor_nets_checked(ct_mode, recolor_fn, recolor_nets)
    if ct_mode is not None and blender_nets is None:
        if ct_mode == "blender":
            raise ValueError(f"swap_images: ct_mode 'blender' needs recolor_nets=(blender, esr), the recolouring network and the Real-ESRGAN network; "
                             f"without them the modes are {list(ops_post.CT_MODES)}")
        ops_post._ct_mode_checked(ct_mode, "swap_images")
    recolor = ct_mode is not None or recolor_fn is not None
    crops = ops.crop_align(target_images_u8, plan)
    target = ops.frames_to_tensor(crops)
    # (mask_surgery=True also computes the video caller's hard radius-5 paste masks, which this path does not use: one byte-wise launch per batch,
    # < 0.1 ms, accepted rather than giving swap_batch another switch)
    swapped, lab, extra = swap_batch(net, parser, driven, target, mask_surgery=True, ear_interpolation=False,
                                     comp_indices=IMAGE_COMP_INDICES_CT if recolor else IMAGE_COMP_INDICES, **swap_batch_kwargs)
    if blender_nets is not None:
        swapped = color_blend(swapped, color_transfer_blender(swapped, crops, parser, *blender_nets), lab)
    elif ct_mode is not None:
        swapped = color_blend(swapped, color_transfer(swapped, crops, lab, extra["target_labels"], ct_mode), lab)
    elif recolor_fn is not None:
        swapped = color_blend(swapped, recolor_fn(swapped, crops), lab)
    pasted = paste_back_soft(swapped, crops, lab, extra["hole_mask"])
    pasted = paste_back_soft(pasted, crops, torch.full_like(lab, 6), None)
    return ops.paste_into_frames(pasted, target_images_u8, plan)


BLENDER_SIZE = 256                      # BlenderInfer.infer_image resizes everything to 256 x 256 (inference.py:101-105)


def blender_infer_inputs(img_a_u8: torch.Tensor, img_t_u8: torch.Tensor, labels_a_u8: torch.Tensor, labels_t_u8: torch.Tensor):
    """The network inputs of ``BlenderInfer.infer_image`` (inference.py:101-114) for a batch, on the device: ``(img_a, img_t, labels_a, labels_t)``, float32
    ``[bs, 3, 256, 256]`` and uint8 ``[bs, 256, 256]``, from uint8 ``[bs, H, W, 3]`` images and uint8 ``[bs, H, W]`` 19-class maps.

    Everything goes through ``PIL.Image.resize((256, 256))`` with Pillow's default BICUBIC (``ops.pil_resize``, bit for bit).  That includes the label maps,
    as mode-``L`` images: an oddity of the reference (a bicubic blend of class ids invents classes along every border), kept because the network was
    trained and is run behind it.  The images then take ``ToTensor`` and ``Normalize`` in their order, in float32: ``(u8 / 255 - mean) / std``."""
    name = "blender_infer_image"
    for nm, t in (("img_a_u8", img_a_u8), ("img_t_u8", img_t_u8)):
        ops_post._frames_u8(t, f"{name}: {nm}")
    for nm, t in (("labels_a_u8", labels_a_u8), ("labels_t_u8", labels_t_u8)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {nm} must be a torch.Tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {nm} must be a CUDA tensor")
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise ValueError(f"{name}: {nm}: expected a uint8 [bs, H, W] label map, got {t.dtype} {tuple(t.shape)}")
    bs = img_a_u8.shape[0]
    if any(t.shape[0] != bs for t in (img_t_u8, labels_a_u8, labels_t_u8)):
        raise ValueError(f"{name}: the four inputs hold {[t.shape[0] for t in (img_a_u8, img_t_u8, labels_a_u8, labels_t_u8)]} samples")
    size = (BLENDER_SIZE, BLENDER_SIZE)
    _, _, mean, std = ops_recolor._consts(img_a_u8.device)
    # a tensor as the divisor: by a Python scalar PyTorch multiplies by the rounded reciprocal on the device, which is not ToTensor's division on the host
    full = torch.full((1,), 255.0, dtype=torch.float32, device=img_a_u8.device)
    imgs = [((ops.pil_resize(t, size).permute(0, 3, 1, 2).float() / full) - mean) / std for t in (img_a_u8, img_t_u8)]
    labels = [ops.pil_resize(t[..., None], size)[..., 0].contiguous() for t in (labels_a_u8, labels_t_u8)]
    return imgs[0].contiguous(), imgs[1].contiguous(), labels[0], labels[1]


@torch.no_grad()
def blender_infer_image(weights, img_a_u8: torch.Tensor, img_t_u8: torch.Tensor, labels_a_u8: torch.Tensor, labels_t_u8: torch.Tensor,
                        flip_target=None) -> torch.Tensor:
    """``BlenderInfer.infer_image`` (inference.py:96-121) for a batch on the device: the colour of ``img_t`` transferred to ``img_a``, uint8
    ``[bs, 256, 256, 3]`` = ``uint8(pred * 255)`` (truncating) of ``ops.blender_forward`` on ``blender_infer_inputs``.  ``weights`` and ``flip_target`` as
    ``ops.blender_forward`` takes them (``ops.BlenderNet().eval()`` with ``latest_netG.pth`` loaded, or the reference's ``Blender`` over the drop-ins)."""
    img_a, img_t, labels_a, labels_t = blender_infer_inputs(img_a_u8, img_t_u8, labels_a_u8, labels_t_u8)
    pred, _, _ = ops.blender_forward(img_a, img_t, labels_a, labels_t, weights, flip_target)
    return (pred * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------ f11: the Real-ESRGAN step and ct_mode 'blender'
ESR_IN = 256                            # RealESRBatchInfer.infer_batch resizes its input to 256 x 256 (image_infer.py:65)
ESR_OUT = 1024                          # infer_image asks for 1024 x 1024 (:77), which is what the x4 network gives


def _esr_size_checked(name, nm, v):
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 16384:
        raise ValueError(f"{name}: {nm} is an int in 1..16384, got {v!r}")
    return v


@torch.no_grad()
def realesr_infer_batch(weights, x: torch.Tensor, out_hw=None, in_size: int = ESR_IN) -> torch.Tensor:
    """``RealESRBatchInfer.infer_batch`` (swap_face_fine/realesr/image_infer.py:60-69) on the device: float32 ``[bs, 3, H, W]`` in [-1, 1] to
    ``[bs, 3, *out_hw]`` in [-1, 1] (``out_hw`` defaults to ``(H, W)``):

        clamp(x * 0.5 + 0.5, 0, 1) -> bilinear to 256 x 256 (align_corners=True) -> RRDBNet (ops.realesr_forward) -> bilinear to out_hw -> clamp(r * 2 - 1, -1, 1)

    The second resize is skipped when ``out_hw`` is the network's output size, where it is the identity.  ``weights`` as ``ops.realesr_forward`` takes them;
    ``in_size`` is the reference's 256."""
    name = "realesr_infer_batch"
    ops_recolor.rrdbnet_weight_tensors(weights, name)
    netweights._tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, 3, H, W] image in [-1, 1]")
    if x.shape[1] != 3 or x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError(f"{name}: x: expected a float32 [bs, 3, H, W] image in [-1, 1], got {tuple(x.shape)}")
    in_size = _esr_size_checked(name, "in_size", in_size)
    out_hw = tuple(x.shape[2:]) if out_hw is None else tuple(out_hw)
    if len(out_hw) != 2:
        raise ValueError(f"{name}: out_hw is (height, width), got {out_hw!r}")
    out_hw = (_esr_size_checked(name, "out_hw[0]", out_hw[0]), _esr_size_checked(name, "out_hw[1]", out_hw[1]))
    netweights._cuda_checked(name, x=x)
    small = ops.bilinear_resize((x * 0.5 + 0.5).clamp(0, 1).contiguous(), (in_size, in_size), align_corners=True)
    r = ops.realesr_forward(small, weights)
    if tuple(r.shape[2:]) != out_hw:
        r = ops.bilinear_resize(r, out_hw, align_corners=True)
    return (r * 2. - 1.).clamp(-1, 1)


@torch.no_grad()
def realesr_infer_image(weights, img_u8: torch.Tensor, in_size: int = ESR_IN, out_size: int = ESR_OUT) -> torch.Tensor:
    """``RealESRBatchInfer.infer_image`` (image_infer.py:71-80) for a batch on the device: uint8 ``[bs, H, W, 3]`` to uint8 ``[bs, 1024, 1024, 3]``,

        v / 127.5 - 1 -> infer_batch(out_hw=(1024, 1024)) -> clamp(r * 127.5 + 127.5, 0, 255) -> uint8 (truncating)

    With ``out_size == 4 * in_size`` (the reference's sizes) everything around the network's convolutions is two kernels (``ops.realesr_image``); otherwise
    the x4 output goes through ``ops.bilinear_resize`` first.  ``in_size`` / ``out_size`` are the reference's 256 / 1024."""
    name = "realesr_infer_image"
    in_size, out_size = _esr_size_checked(name, "in_size", in_size), _esr_size_checked(name, "out_size", out_size)
    if out_size == 4 * in_size:
        return ops.realesr_image(img_u8, weights, in_size)
    ops_recolor.rrdbnet_weight_tensors(weights, name)
    x = ops.realesr_input(img_u8, (in_size, in_size))
    if x.shape[0] == 0:
        return torch.empty((0, out_size, out_size, 3), dtype=torch.uint8, device=x.device)
    r = ops.bilinear_resize(ops.realesr_forward(x, weights), (out_size, out_size), align_corners=True)
    r = (r * 2. - 1.).clamp(-1, 1)
    return (r * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def gpen_enhance(weights, img_u8: torch.Tensor) -> torch.Tensor:
    """``FaceGAN.process`` (swap_face_fine/gpen/face_model/face_gan.py:36-47) behind its ``cv2.resize`` and without its BGR flips, on the device: uint8
    ``[bs, size, size, 3]`` RGB faces, already at the network's size, to the enhanced uint8 faces of the same shape (``ops.gpen_image``).  ``weights`` as
    ``ops.gpen_forward`` takes them.  The detector, the warps, the parsing mask and the paste of ``FaceEnhancement.process`` stay with the caller."""
    return ops.gpen_image(img_u8, weights)


def gpen_face_mask(parsenet, faces_u8: torch.Tensor) -> torch.Tensor:
    """``FaceParse.process`` (swap_face_fine/gpen/face_parse/face_parsing.py:39-45) behind its ``cv2.resize``, on the device: uint8 ``[bs, S, S, 3]`` RGB faces
    at the network's ``in_size`` — what ``gpen_enhance`` returns — to the uint8 paste masks ``[bs, S', S']`` of 0 / 255 (``ops.parsenet_mask`` with
    ``bgr=False``: the reference's BGR flip and this caller's RGB cancel).  ``parsenet`` as ``ops.parsenet_forward`` takes weights.  The Gaussian blurs of
    ``mask_postprocess`` and the paste stay with the caller."""
    return ops.parsenet_mask(faces_u8, parsenet, bgr=False)


def gpen_detect_faces(net, frames_u8: torch.Tensor, bgr: bool = True):
    """``RetinaFaceDetection.detect`` (swap_face_fine/gpen/face_detect/retinaface_detection.py:61-131) as ``FaceEnhancement.process`` calls it, for a batch of
    frames on the device: uint8 ``[bs, H, W, 3]`` (BGR as the reference takes them, RGB with ``bgr=False``) to a list of ``(dets [n, 5], landms [n, 10])`` per
    frame (``ops.retinaface_detect`` at the reference's thresholds).  ``net`` as ``ops.retinaface_forward`` takes weights.  The 5-point ``warpAffine`` pair
    around the enhancement stays with the caller."""
    return ops.retinaface_detect(frames_u8, net, bgr=bgr)


def reenact_keypoints(kp_detector, he_estimator, source: torch.Tensor, driving: torch.Tensor, estimate_jacobian: Optional[bool] = None):
    """What ``make_animation`` (swap_face_fine/face_vid2vid/drive_demo.py:182-) computes in front of the generator, for a clip on the device: float32 ``source
    [1, 3, H, W]`` and ``driving [n, 3, H, W]`` in [0, 1] to ``(kp_canonical, kp_source, kp_driving)`` — the detector once on the source, ONE head-pose pass over
    the n + 1 images, ``kp_driving`` batched over the frames (``ops.reenact_keypoints``).  The two networks as ``ops.kp_detector_forward`` and
    ``ops.he_estimator_forward`` take weights.  The dense-motion network and the generator stay with the caller."""
    return ops.reenact_keypoints(source, driving, kp_detector, he_estimator, estimate_jacobian)


def reenact_dense_motion(dense_motion, feature: torch.Tensor, kp_driving, kp_source):
    """What ``OcclusionAwareSPADEGenerator.forward`` (swap_face_fine/face_vid2vid/modules/generator.py) asks of its ``dense_motion_network`` per driven frame, on
    the device: the float32 feature volume ``[bs, C, D, H, W]`` and the two keypoint dicts to ``{'mask', 'deformation'[, 'occlusion_map']}``
    (``ops.dense_motion_forward``).  ``dense_motion`` as ``ops.dense_motion_forward`` takes weights: a module, a mapping, or the generator's checkpoint.  The
    generator itself stays with the caller."""
    return ops.dense_motion_forward(feature, kp_driving, kp_source, dense_motion)


def reenact_source_feature(generator, source: torch.Tensor):
    """The part of ``OcclusionAwareSPADEGenerator.forward`` that sees the source alone (generator.py:212-219), once per clip: float32 ``source [1, 3, H, W]`` in
    [0, 1] to the appearance volume ``feature_3d [1, reshape_channel, reshape_depth, h, w]`` (``ops.appearance_feature``).  ``make_animation`` recomputes it for
    every driving frame; here it is held and handed to ``reenact_warp``.  ``generator`` as ``ops.appearance_feature`` takes weights."""
    return ops.appearance_feature(source, generator)


def reenact_warp(generator, feature_3d: torch.Tensor, kp_driving, kp_source):
    """The per-frame part of the generator in front of its decoder (generator.py:221-244), for the n driving frames of the keypoint dicts at once: the dense-motion
    network, the warp of the held ``feature_3d`` (batch 1: shared by every frame), ``third``, ``fourth`` and the occlusion product, to ``{'mask',
    'deformation'[, 'occlusion_map'], 'feature'}`` (``ops.generator_warp``); ``feature`` is the ``SPADEDecoder``'s input.  The decoder stays with the caller."""
    return ops.generator_warp(feature_3d, kp_driving, kp_source, generator)


def reenact_frames(generator, feature_3d: torch.Tensor, kp_driving, kp_source):
    """The per-frame part of the generator with its ``SPADEDecoder`` (generator.py:221-250), for the n driving frames of the keypoint dicts at once:
    ``reenact_warp`` and the decoder, to the reference's ``output_dict`` ``{'mask'[, 'occlusion_map'], 'prediction' [n, 3, H, W]}``
    (``ops.generator_frames``).  ``feature_3d`` is ``reenact_source_feature``'s, held once per clip."""
    return ops.generator_frames(feature_3d, kp_driving, kp_source, generator)


def reenact_clip(generator, kp_detector, he_estimator, source: torch.Tensor, driving: torch.Tensor, **kw):
    """``make_animation`` (swap_face_fine/face_vid2vid/drive_demo.py:182-211) for a clip on the device: float32 ``source [1, 3, H, W]`` and ``driving
    [n, 3, H, W]`` in [0, 1] to the reenacted frames ``[n, 3, H', W']`` (``ops.make_animation``; ``kw``: its ``estimate_jacobian``, ``free_view``, ``yaw``,
    ``pitch``, ``roll`` and ``batch``).  Nothing stays with the caller."""
    return ops.make_animation(source, driving, generator, kp_detector, he_estimator, **kw)


@torch.no_grad()
def gpen_enhance_frames(detector, gpen, parsenet, frames_u8: torch.Tensor, base_u8: Optional[torch.Tensor] = None, return_faces: bool = False):
    """``FaceEnhancement.process(img, aligned=False)`` (swap_face_fine/gpen/face_enhancement.py:68-110) behind its ``use_sr`` branch, for a batch of frames on
    the device: RGB uint8 ``[bs, H, W, 3]`` to the enhanced uint8 frames of the same shape,

        dets, landms   = gpen_detect_faces(detector, frames, bgr=False)          (:68; every frame's faces concatenated in detector order)
        T, flags       = ops.gpen_face_transforms(...)                           (:75-80, :93; warp_and_crop_face's similarity pair, score and size flags)
        of             = ops.gpen_warp_crop(frames, frame_of_face, T, S)         (:80; cv2.warpAffine to the S x S crop, S the generator's size)
        ef             = gpen_enhance(gpen, of)                                  (:83)
        mask           = ops.gpen_mask_feather(gpen_face_mask(parsenet, ef))     (:89; mask_postprocess)
        out            = ops.gpen_paste(base, ops.gpen_smooth_small(ef, flags), mask, T, flags, face_begin)     (:91-108)

    at the reference's constants (``ops.GPEN_PASTE_DEFAULTS``).  ``base_u8`` is what the faces are pasted over: the frames themselves, or — the reference's
    ``use_sr`` — a super-resolved frame of the same shape (its RealESRNet pass and the resize of the frame to its size are ``gpen_face_enhancement``'s).  With
    ``return_faces`` the result is ``(out, orig_faces, enhanced_faces)``: per frame the uint8 ``[n_b, S, S, 3]`` crops and enhanced faces of the faces above the
    score threshold, the reference's second and third results.  A frame without a face comes back as ``base``.  The one device-to-host read is the detector's, of
    its kept counts (with ``return_faces`` the flags are read too, to drop the skipped faces).  Refused: a ParseNet whose mask is not S x S (the reference
    resizes it with cv2), frames that are not uint8 ``[bs, H, W, 3]`` on the device, a ``base_u8`` of another shape.  A non-contiguous view is accepted and
    copied."""
    name = "gpen_enhance_frames"
    from . import ops_gpen, ops_parsenet
    netweights._tensor_checked(name, "frames_u8", frames_u8, torch.uint8, 4, "uint8 [bs, H, W, 3] RGB frames")
    if frames_u8.shape[3] != 3 or frames_u8.shape[0] < 1:
        raise ValueError(f"{name}: frames_u8: expected uint8 [bs, H, W, 3] RGB frames with bs >= 1, got {tuple(frames_u8.shape)}")
    netweights._cuda_checked(name, frames_u8=frames_u8)
    if base_u8 is not None:
        netweights._tensor_checked(name, "base_u8", base_u8, torch.uint8, 4, "uint8 [bs, H, W, 3] frames")
        if base_u8.shape != frames_u8.shape or base_u8.device != frames_u8.device:
            raise ValueError(f"{name}: base_u8 is {tuple(base_u8.shape)} on {base_u8.device}: expected the frames' {tuple(frames_u8.shape)} on {frames_u8.device} "
                             "(resizing the frame to a super-resolved size is the caller's)")
    S = int(ops_gpen._weights_checked(name, gpen)[1][0])
    structure = netweights._validated(name, parsenet, ops_parsenet._net_of(parsenet))[1]
    if ops_parsenet.parsenet_output_size(structure, S, S) != (S, S):
        raise ValueError(f"{name}: the ParseNet turns a {S} x {S} face into a {ops_parsenet.parsenet_output_size(structure, S, S)} mask: expected {S} x {S} "
                         "(the reference resizes the mask with cv2, which is not done here)")
    D = ops.GPEN_PASTE_DEFAULTS
    frames = frames_u8.contiguous()
    bs, dev = frames.shape[0], frames.device
    per_frame = gpen_detect_faces(detector, frames, bgr=False)
    counts = [int(d.shape[0]) for d, _ in per_frame]
    dets, landms = torch.cat([d for d, _ in per_frame]), torch.cat([l for _, l in per_frame])
    begin = [0]
    for c in counts:
        begin.append(begin[-1] + c)
    face_begin = torch.tensor(begin, dtype=torch.int32, device=dev)
    frame_of_face = torch.tensor([b for b, c in enumerate(counts) for _ in range(c)], dtype=torch.int32, device=dev)
    T, flags = ops.gpen_face_transforms(dets, landms, ops.gpen_reference_points(S), D["threshold"], D["small_face"])
    of = ops.gpen_warp_crop(frames, frame_of_face, T, S)
    ef = gpen_enhance(gpen, of)
    masks = ops.gpen_mask_feather(gpen_face_mask(parsenet, ef), D["ksize"], D["sigma"], D["thres"])
    out = ops.gpen_paste(frames if base_u8 is None else base_u8, ops.gpen_smooth_small(ef, flags), masks, T, flags, face_begin)
    if not return_faces:
        return out
    kept = ((flags & ops.GPEN_FACE_SKIP) == 0).cpu()
    return out, [of[a:b][kept[a:b]] for a, b in zip(begin, begin[1:])], [ef[a:b][kept[a:b]] for a, b in zip(begin, begin[1:])]


def gpen_super_resolve(sr, frames_u8: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    """``RealESRNet.process`` (swap_face_fine/gpen/sr_model/real_esrnet.py:26-60) for a batch on the device under this module's RGB convention
    (``ops.gpen_sr_image``; ``bgr=True``: BGR in and out, as the reference takes it): uint8 ``[bs, H, W, 3]`` to the super-resolved uint8
    ``[bs, Ho, Wo, 3]``, ``(Ho, Wo) = ops.gpen_sr_output_size(H, W, scale)[0]``.  ``sr`` as ``ops.gpen_sr_forward`` takes weights."""
    return ops.gpen_sr_image(frames_u8, sr, bgr=bgr)


@torch.no_grad()
def gpen_face_enhancement(detector, gpen, parsenet, sr, frames_u8: torch.Tensor, aligned: bool = False, return_faces: bool = False):
    """The whole of ``FaceEnhancement.process(img, aligned)`` (swap_face_fine/gpen/face_enhancement.py:51-110) for a batch of RGB uint8 frames on the device;
    ``sr`` None is the reference's ``use_sr=False``.

    ``aligned=True`` (:53-61): the frames are faces at the generator's size; ``ef = gpen_enhance(gpen, frames)`` and, with ``sr``, ``out =
    gpen_super_resolve(sr, ef)``, otherwise ``out = ef``.  ``detector`` and ``parsenet`` are not used and may be None.

    ``aligned=False`` with ``sr`` (:63-66, :105-106): ``img_sr = gpen_super_resolve(sr, frames)``, the frames resized to its size
    (``ops.cv_resize_linear``), and ``gpen_enhance_frames`` on the resized frames with ``img_sr`` as the base the faces are pasted over.  Without ``sr``
    exactly ``gpen_enhance_frames``.

    Returns ``out``, or with ``return_faces`` the reference's triple ``(out, orig_faces, enhanced_faces)``: aligned, ``[frames]`` and ``[ef]``; otherwise as
    ``gpen_enhance_frames`` gives them.  Every argument is checked before any launch."""
    name = "gpen_face_enhancement"
    from . import ops_gpen, ops_gpen_sr
    netweights._tensor_checked(name, "frames_u8", frames_u8, torch.uint8, 4, "uint8 [bs, H, W, 3] RGB frames")
    if frames_u8.shape[3] != 3 or frames_u8.shape[0] < 1:
        raise ValueError(f"{name}: frames_u8: expected uint8 [bs, H, W, 3] RGB frames with bs >= 1, got {tuple(frames_u8.shape)}")
    if sr is not None:
        netweights._devices_checked(name, "frames_u8", frames_u8, ops_gpen_sr.gpen_sr_weight_tensors(sr, name))
    netweights._cuda_checked(name, frames_u8=frames_u8)
    if aligned:
        S = int(ops_gpen._weights_checked(name, gpen)[1][0])
        if tuple(frames_u8.shape[1:3]) != (S, S):
            raise ValueError(f"{name}: aligned faces are {S} x {S}, the generator's size (the reference resizes them with cv2, which is not done here), "
                             f"got {tuple(frames_u8.shape)}")
        ef = gpen_enhance(gpen, frames_u8)
        out = ef if sr is None else gpen_super_resolve(sr, ef)
        return (out, [frames_u8], [ef]) if return_faces else out
    if sr is None:
        return gpen_enhance_frames(detector, gpen, parsenet, frames_u8, return_faces=return_faces)
    from . import ops_parsenet
    ops_gpen._weights_checked(name, gpen)                                     # what gpen_enhance_frames refuses, before the RealESRNet pass runs
    netweights._validated(name, parsenet, ops_parsenet._net_of(parsenet))
    img_sr = gpen_super_resolve(sr, frames_u8)
    resized = ops.cv_resize_linear(frames_u8, (img_sr.shape[2], img_sr.shape[1]))
    return gpen_enhance_frames(detector, gpen, parsenet, resized, base_u8=img_sr, return_faces=return_faces)


@torch.no_grad()
def color_transfer_blender(swapped_u8: torch.Tensor, target_u8: torch.Tensor, parser, blender, esr, flip_target=None) -> torch.Tensor:
    """The ``'blender'`` branch of the image caller's ``_color_transfer`` (Face_swap_with_two_imgs.py:525-536), the reference's default mode, for a batch on
    the device:

        la, lt = the 19-class maps of the swapped face and of the target crop (:526, :595)
        small  = BlenderInfer.infer_image(swapped, target, la, lt)             (:529-531; blender_infer_image, uint8 [bs, 256, 256, 3])
        face   = small.resize(swapped.size)                                    (:533; Pillow's BICUBIC, ops.pil_resize)
        out    = RealESRBatchInfer.infer_image(face)                           (:534; realesr_infer_image, uint8 [bs, 1024, 1024, 3])

    ``swapped_u8`` / ``target_u8``: uint8 ``[bs, S, S, 3]`` crops (1024 in the pipeline); ``parser``: the ``FaceParser``; ``blender`` as
    ``ops.blender_forward`` takes its weights, ``esr`` as ``ops.realesr_forward``; ``flip_target`` as ``ops.blender_features``."""
    name = "color_transfer_blender"
    _crops_checked(name, swapped_u8, target_u8)
    if not swapped_u8.is_cuda:
        raise RuntimeError(f"{name}: the frames must be CUDA tensors")
    ops_recolor.rrdbnet_weight_tensors(esr, name)
    ops_recolor._blender_weights(name, blender)
    bs, h, w, _ = swapped_u8.shape
    if bs == 0:
        return torch.empty((0, ESR_OUT, ESR_OUT, 3), dtype=torch.uint8, device=swapped_u8.device)
    to01 = lambda u8: u8.permute(0, 3, 1, 2).float() / 255                    # noqa: E731  (parse_batch takes [bs, 3, S, S] in [0, 1])
    la = parser.parse_batch(to01(swapped_u8), seg12=False)
    lt = parser.parse_batch(to01(target_u8), seg12=False)
    small = blender_infer_image(blender, swapped_u8, target_u8, la, lt, flip_target)
    return realesr_infer_image(esr, ops.pil_resize(small, (w, h)))


@torch.no_grad()
def codeformer_front(net, faces_u8: torch.Tensor, adain: bool = True):
    """The tensor end in front of ``CodeFormer`` (swap_face_fine/inference_codeformer.py:160-163: ``img2tensor(img / 255., bgr2rgb=False)``, then
    ``normalize(x, 0.5, 0.5)``) and ``ops.codeformer_front`` for a batch of uint8 ``[n, 3, 512, 512]`` RGB faces on the device: ``dict(quant_feat, logits,
    lq_feat, idx, taps)``, the tensors stage 2's generator starts from.  Faces of another size go through ``ops.pil_resize`` to 512 x 512 first.  ``net``: an
    ``ops.CodeFormer`` in eval mode, or a mapping with its keys."""
    from . import ops_codeformer
    return ops_codeformer.codeformer_front(_codeformer_input("codeformer_front", net, faces_u8), net, adain=adain)


def _codeformer_input(name, net, faces_u8, max_batch=None):
    """The tensor end in front of ``CodeFormer``, checked before its first launch: float32 ``[n, 3, 512, 512]`` in [-1, 1] of uint8 RGB faces."""
    from . import ops_codeformer
    checked = ops_codeformer._weights_checked(name, net)
    netweights._tensor_checked(name, "faces_u8", faces_u8, torch.uint8, 4, "uint8 [n, 3, H, W] RGB faces")
    if faces_u8.shape[1] != 3 or faces_u8.shape[2] < 1 or faces_u8.shape[3] < 1:
        raise ValueError(f"{name}: faces_u8: expected uint8 [n, 3, H, W] RGB faces, got {tuple(faces_u8.shape)}")
    if max_batch is not None and faces_u8.shape[0] > max_batch:
        raise ValueError(f"{name}: faces_u8 is {tuple(faces_u8.shape)}: at most {max_batch} faces a call")
    netweights._devices_checked(name, "faces_u8", faces_u8, checked[2])
    netweights._cuda_checked(name, faces_u8=faces_u8)
    if tuple(faces_u8.shape[2:]) != (512, 512):
        faces_u8 = ops.pil_resize(faces_u8.permute(0, 2, 3, 1).contiguous(), (512, 512)).permute(0, 3, 1, 2)
    return (((faces_u8.float() / 255.0) - 0.5) / 0.5).contiguous()


@torch.no_grad()
def codeformer_restore(net, faces_u8: torch.Tensor, w=0.8, adain: bool = True) -> torch.Tensor:
    """``CodeFormerInfer.infer_image`` on the device for a batch of uint8 ``[n, 3, 512, 512]`` RGB faces: ``codeformer_front``'s tensor end,
    ``ops.codeformer_restore`` at fusion weight ``w`` (the caller's recolor target uses 0.8), and ``tensor2img(output, min_max=(-1, 1))`` as ``ops.image_u8``:
    uint8 ``[n, 3, 512, 512]``, RGB like the input (the reference's ``rgb2bgr`` and the caller's ``[:, :, ::-1]`` cancel)."""
    name = "codeformer_restore"
    from . import ops_codeformer_gen as G
    w = G._w_checked(name, w)
    x = _codeformer_input(name, net, faces_u8, max_batch=65535 // G._WIDEST)
    return G.image_u8(G.codeformer_restore(x, net, w=w, adain=adain)[0])


# ------------------------------------------------------------------------------------ f23: the tiled Real-ESRGAN x2 step and the recolor loop
def _upscale_checked(name, upscale):
    import math
    if isinstance(upscale, bool) or not isinstance(upscale, (int, float)) or not math.isfinite(upscale) or upscale <= 0:
        raise ValueError(f"{name}: upscale is a finite positive real, got {upscale!r}")
    return upscale


def _enhance_args_checked(name, net, esr, faces_u8, w, upscale):
    """What ``codeformer_enhance`` refuses, in front of its first launch: both networks, ``w``, ``upscale`` and the faces, in ``codeformer_restore``'s order."""
    from . import ops_codeformer, ops_codeformer_gen as G, ops_esrgan
    w = G._w_checked(name, w)
    _upscale_checked(name, upscale)
    checked = ops_codeformer._weights_checked(name, net)
    netweights._tensor_checked(name, "faces_u8", faces_u8, torch.uint8, 4, "uint8 [n, 3, H, W] RGB faces")
    if faces_u8.shape[1] != 3 or faces_u8.shape[2] < 1 or faces_u8.shape[3] < 1:
        raise ValueError(f"{name}: faces_u8: expected uint8 [n, 3, H, W] RGB faces, got {tuple(faces_u8.shape)}")
    probe = torch.empty((faces_u8.shape[0], 3, 512, 512), dtype=torch.uint8, device="meta")   # what the restoration hands the Real-ESRGAN step: shapes only
    esr_checked = ops_esrgan._enhance_checked(name, probe, esr, upscale, ops_esrgan.ESRGAN_TILE, ops_esrgan.ESRGAN_TILE_PAD, ops_esrgan.ESRGAN_PRE_PAD, True)[0]
    netweights._devices_checked(name, "faces_u8", faces_u8, checked[2])
    netweights._devices_checked(name, "faces_u8", faces_u8, esr_checked[2])
    return w


@torch.no_grad()
def codeformer_enhance(net, esr, faces_u8: torch.Tensor, w=0.8, adain: bool = True, upscale=2) -> torch.Tensor:
    """The whole of ``CodeFormerInfer.infer_image`` (swap_face_fine/inference_codeformer.py:157-178) for a batch on the device: ``codeformer_restore`` (the
    resize to 512 x 512, the network, ``tensor2img``) and ``RealESRGANer.enhance(restored_face, outscale=upscale)`` as ``ops.esrgan_enhance(..., chw=True)`` at
    the reference's ``tile=400, tile_pad=40, pre_pad=0``: 2 x 2 overlapping tiles through RRDBNet x4plus, the 2048 x 2048 image, ``cv2.resize`` at INTER_LANCZOS4
    on uint8.  uint8 ``[n, 3, H, W]`` RGB faces to uint8 ``[n, 3, 512 upscale, 512 upscale]``, in ``codeformer_restore``'s layout.  ``net`` as
    ``codeformer_restore`` takes it, ``esr`` as ``ops.esrgan_enhance`` takes weights (the x4 network, in eval mode).  The Real-ESRGAN step runs the reference's
    ``half=False`` arithmetic (``ops_esrgan`` says why).  The reference's ``except`` fallback — the input face where CodeFormer fails — is not reproduced: errors
    raise.  Both networks and every argument are checked before the first launch."""
    name = "codeformer_enhance"
    w = _enhance_args_checked(name, net, esr, faces_u8, w, upscale)
    netweights._cuda_checked(name, faces_u8=faces_u8)
    restored = codeformer_restore(net, faces_u8, w=w, adain=adain)
    return ops.esrgan_enhance(restored, esr, outscale=upscale, chw=True).permute(0, 3, 1, 2).contiguous()


def _recolor_args_checked(name, parser, blender, codeformer, esr, swapped_u8, targets_u8, w):
    """What ``recolor_frames`` refuses, in front of its first launch: (bs, S, w)."""
    for nm, t in (("swapped_u8", swapped_u8), ("targets_u8", targets_u8)):
        netweights._tensor_checked(name, nm, t, torch.uint8, 4, "uint8 [bs, H, W, 3] crops")
        if t.shape[3] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
            raise ValueError(f"{name}: {nm}: expected uint8 [bs, H, W, 3] crops, got {tuple(t.shape)}")
    if swapped_u8.shape[1] != swapped_u8.shape[2]:
        raise ValueError(f"{name}: swapped_u8: the swapped crops are square, got {tuple(swapped_u8.shape)}")
    if targets_u8.shape[0] != swapped_u8.shape[0] or targets_u8.device != swapped_u8.device:
        raise ValueError(f"{name}: {swapped_u8.shape[0]} swapped crops on {swapped_u8.device}, {targets_u8.shape[0]} target crops on {targets_u8.device}")
    if not callable(getattr(parser, "parse_batch", None)):
        raise TypeError(f"{name}: parser has no parse_batch (the FaceParser), got {type(parser).__name__}")
    ops_recolor._blender_weights(name, blender)
    bs, S = swapped_u8.shape[0], swapped_u8.shape[1]
    w = _enhance_args_checked(name, codeformer, esr, swapped_u8.permute(0, 3, 1, 2), w, 2)
    netweights._cuda_checked(name, swapped_u8=swapped_u8, targets_u8=targets_u8)
    return bs, S, w


@torch.no_grad()
def recolor_frames(parser, blender, codeformer, esr, swapped_u8: torch.Tensor, targets_u8: torch.Tensor, flip_target=None, w=0.8) -> torch.Tensor:
    """The body of the video pipeline's recolor loop (face_swap_video_pipeline.py:270-304) for a batch on the device: the ``D_recolor`` frames, uint8
    ``[bs, 1024, 1024, 3]``, from the swapped crops uint8 ``[bs, S, S, 3]`` and the target crops uint8 ``[bs, Ht, Wt, 3]``:

        T       = targets.resize(swapped.size)                                   (:274; ops.pil_resize)
        la, lt  = the 19-class maps of the swapped face and of T                  (:276-277; as color_transfer_blender takes them)
        small   = BlenderInfer.infer_image(swapped, T, la, lt)                   (:278-281; blender_infer_image, uint8 [bs, 256, 256, 3])
        recolor = small.resize(swapped.size)                                     (:283)
        recolor = CodeFormerInfer.infer_image(recolor)                           (:284; codeformer_enhance, whose input end resizes to 512 x 512: 1024 x 1024)
        recolor = recolor.resize((512, 512)).resize(recolor.size)                (:285, "resize down to avoid too high-res")

    ``parser``: the ``FaceParser``; ``blender`` as ``ops.blender_forward`` takes weights, ``codeformer`` and ``esr`` as ``codeformer_enhance`` takes them;
    ``flip_target`` as ``ops.blender_features``; ``w`` the fusion weight.  Every argument is checked before the first launch.  The whole-clip chain from
    the source image and the target crops to these frames is ``reenact_recolor_clip``."""
    name = "recolor_frames"
    bs, S, w = _recolor_args_checked(name, parser, blender, codeformer, esr, swapped_u8, targets_u8, w)
    if bs == 0:
        return torch.empty((0, 1024, 1024, 3), dtype=torch.uint8, device=swapped_u8.device)
    T = ops.pil_resize(targets_u8, (S, S))
    to01 = lambda u8: u8.permute(0, 3, 1, 2).float() / 255                    # noqa: E731  (parse_batch takes [bs, 3, S, S] in [0, 1])
    la = parser.parse_batch(to01(swapped_u8), seg12=False)
    lt = parser.parse_batch(to01(T), seg12=False)
    small = blender_infer_image(blender, swapped_u8, T, la, lt, flip_target)
    recolor = ops.pil_resize(small, (S, S))
    recolor = codeformer_enhance(codeformer, esr, recolor.permute(0, 3, 1, 2), w=w).permute(0, 2, 3, 1).contiguous()
    size = (recolor.shape[2], recolor.shape[1])
    return ops.pil_resize(ops.pil_resize(recolor, (512, 512)), size)


# ------------------------------------------------------------------------------------ f24: the whole-clip reenactment chain
_ANIMATION_KW = ("estimate_jacobian", "free_view", "yaw", "pitch", "roll")


def _stage_checked(name, fn, *args):
    """``fn(*args)`` — a stage's own check, or the stage on an EMPTY batch, which refuses what it refuses and launches nothing — with this entry's name in front."""
    try:
        return fn(*args)
    except (TypeError, ValueError, KeyError, RuntimeError) as e:
        raise type(e)(f"{name}: {e.args[0] if e.args else e}") from None


def _reenact_args_checked(name, generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, source_u8, targets_u8, size, enhance, channel_order, batch, chunk,
                          kw):
    """What ``reenact_drivens`` refuses, in front of its first launch: ((H', W') of the predictions, (Ho, Wo) of the D frames)."""
    from . import ops_gpen, ops_gpen_sr, ops_parsenet, ops_reenact_frames, ops_retinaface, ops_rrdb, ops_sk
    for nm, v in (("size", size), ("batch", batch), ("chunk", chunk)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name}: {nm} is a positive int, got {v!r}")
    if channel_order not in ("reference", "rgb"):
        raise ValueError(f"{name}: channel_order is 'reference' (the reference's RGB array handed to a BGR interface) or 'rgb', got {channel_order!r}")
    unknown = sorted(set(kw) - set(_ANIMATION_KW))
    if unknown:
        raise TypeError(f"{name}: unexpected keyword {unknown[0]!r}: make_animation takes {', '.join(_ANIMATION_KW)}")
    for nm in ("yaw", "pitch", "roll"):
        v = kw.get(nm, 0)
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float))):
            raise TypeError(f"{name}: {nm} is a number of degrees or None, got {type(v).__name__}")
    ops_sk._sk_resize_checked(name, "source_u8", source_u8, (size, size))
    ops_sk._sk_resize_checked(name, "targets_u8", targets_u8, (size, size))
    if source_u8.shape[0] != 1:
        raise ValueError(f"{name}: source_u8 is ONE image, uint8 [1, H, W, 3], got {tuple(source_u8.shape)}")
    if targets_u8.device != source_u8.device:
        raise ValueError(f"{name}: source_u8 on {source_u8.device}, targets_u8 on {targets_u8.device}")
    netweights._cuda_checked(name, source_u8=source_u8, targets_u8=targets_u8)
    probe = torch.empty((0, 3, size, size), dtype=torch.float32, device=source_u8.device)     # an empty batch: every refusal of a stage, no launch
    ops_reenact_frames._frames_checked(name, generator)
    f3 = _stage_checked(name, ops.appearance_feature, probe, generator)
    _stage_checked(name, ops.kp_detector_forward, probe, kp_detector)
    _stage_checked(name, ops.he_estimator_forward, probe, he_estimator)
    pred_hw = (4 * f3.shape[3], 4 * f3.shape[4])                               # as make_animation sizes an empty clip
    if not enhance:
        return pred_hw, pred_hw
    g_checked = ops_gpen._weights_checked(name, gpen)
    S = int(g_checked[1][0])
    p_checked = netweights._validated(name, parsenet, ops_parsenet._net_of(parsenet))
    if ops_parsenet.parsenet_output_size(p_checked[1], S, S) != (S, S):
        raise ValueError(f"{name}: the ParseNet turns a {S} x {S} face into a {ops_parsenet.parsenet_output_size(p_checked[1], S, S)} mask: expected {S} x {S} "
                         "(the reference resizes the mask with cv2, which is not done here)")
    tensors = [g_checked[2], p_checked[2], ops_retinaface.retinaface_weight_tensors(detector, name)]
    out_hw = pred_hw
    if sr is not None:
        s_checked = netweights._validated(name, sr, ops_rrdb._GSR_NET)
        tensors.append(s_checked[2])
        out_hw, pads = ops_gpen_sr.gpen_sr_output_size(pred_hw[0], pred_hw[1], int(s_checked[1][2]))
        if pred_hw[0] <= pads[0] or pred_hw[1] <= pads[1] or max(out_hw) > ops_gpen_sr.GPEN_SR_MAX_SIDE:
            raise ValueError(f"{name}: the {pred_hw[0]} x {pred_hw[1]} predictions cannot go through the x{int(s_checked[1][2])} RealESRNet pass (reflect pad "
                             f"{pads}, output {out_hw}, sides up to {ops_gpen_sr.GPEN_SR_MAX_SIDE})")
    for ts in tensors:
        netweights._devices_checked(name, "source_u8", source_u8, ts)
    return pred_hw, out_hw


def _reenact_drivens_run(generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, source_u8, targets_u8, size, enhance, channel_order, batch, chunk, kw):
    source = ops.sk_resize(source_u8, (size, size))
    driving = ops.sk_resize(targets_u8, (size, size))
    pred = reenact_clip(generator, kp_detector, he_estimator, source, driving, batch=batch, **kw)
    flip = enhance and channel_order == "reference"
    frames = ops.frames_u8(pred, flip=flip)
    if not enhance:
        return frames
    out = [gpen_face_enhancement(detector, gpen, parsenet, sr, frames[i:i + chunk]) for i in range(0, frames.shape[0], chunk)]
    out = out[0] if len(out) == 1 else torch.cat(out)
    return out.flip(3) if flip else out


@torch.no_grad()
def reenact_drivens(generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, source_u8: torch.Tensor, targets_u8: torch.Tensor, size: int = 256,
                    enhance: bool = True, channel_order: str = "reference", batch: int = 4, chunk: int = 8, **make_animation_kw) -> torch.Tensor:
    """The video caller's ``_process_face_reenact`` up to its D frames (face_swap_video_pipeline.py:248-257) for a clip on the device: the source image uint8
    ``[1, H, W, 3]`` and the n target crops uint8 ``[n, Ht, Wt, 3]`` (RGB) to the driven frames D, uint8 ``[n, 4 size, 4 size, 3]`` with the x4 RealESRNet ``sr``:

        source_256, targets_256 = resize(np.array(im) / 255.0, (size, size))      (:248-249; ops.sk_resize, skimage's float64 resize)
        predictions             = drive_source_demo(...)                           (:251; reenact_clip, ``batch`` frames per generator call)
        predictions             = (pred * 255).astype(np.uint8)                    (:253; ops.frames_u8)
        predictions             = GPENInfer.infer_image(pred)                      (:255-257, gpen_demo.py:18-26, 59-77; gpen_face_enhancement(aligned=False),
                                                                                   ``chunk`` frames per call: a frame's bytes do not depend on its chunk)

    ``enhance=False`` stops after the third line: the ``size x size`` uint8 predictions, the image caller's ``driven`` (Face_swap_with_two_imgs.py:741-743);
    the four GPEN networks are not looked at then.  ``sr`` None is ``use_sr=False``: D has the predictions' size.

    ``channel_order``.  ``GPENInfer.infer_image`` hands ``np.array(img_lq)``, an RGB array, to ``FaceEnhancement.process``, which treats it as BGR — the
    detector's mean, the RealESRNet pass and the generator all see the channels reversed.  The native GPEN path is RGB-convention, ``native(Y) ==
    reference(Y[..., ::-1])[..., ::-1]``, so ``"reference"`` (the default) reproduces the reference's call as ``native(X[..., ::-1])[..., ::-1]``: the frames
    enter channel-reversed (``frames_u8(flip=True)``) and the result is reversed back, a pass of its own over D.  ``"rgb"`` does neither: what the reference
    would compute if it converted to BGR first.

    ``GPEN_demo``'s ``alpha = 1.0`` blend, ``(img_out * alpha + img * (1 - alpha)).clip(0, 255).astype(uint8)``, and the ``cv2.resize`` that feeds it are not
    built: for a byte x and any byte y, ``x * 1.0 + y * 0.0`` is exactly x in float64, the clip keeps it and the cast returns it.

    ``make_animation_kw``: ``estimate_jacobian``, ``free_view``, ``yaw``, ``pitch``, ``roll`` of ``ops.make_animation``.  The networks as the stages take them.
    Every argument of every stage is checked before the first launch (a stage's own refusals by running it on an empty batch, which launches nothing).  An empty
    clip returns an empty tensor of the right shape."""
    name = "reenact_drivens"
    pred_hw, out_hw = _reenact_args_checked(name, generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, source_u8, targets_u8, size, enhance,
                                            channel_order, batch, chunk, make_animation_kw)
    if targets_u8.shape[0] == 0:
        return torch.empty((0,) + out_hw + (3,), dtype=torch.uint8, device=targets_u8.device)
    return _reenact_drivens_run(generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, source_u8, targets_u8, size, enhance, channel_order, batch, chunk,
                                make_animation_kw)


@torch.no_grad()
def reenact_recolor_clip(generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, parser, blender, codeformer, esr, source_u8: torch.Tensor,
                         targets_u8: torch.Tensor, size: int = 256, channel_order: str = "reference", batch: int = 4, chunk: int = 8, flip_target=None, w=0.8,
                         **make_animation_kw):
    """``_process_face_reenact(targets, source, use_recolor=True)`` (face_swap_video_pipeline.py:239-314) for a clip on the device: ``(D, D_recolor)``.  ``D`` is
    ``reenact_drivens(...)``, uint8 ``[n, S, S, 3]``; ``D_recolor`` is ``recolor_frames(parser, blender, codeformer, esr, D, targets_u8, flip_target, w)``,
    uint8 ``[n, 1024, 1024, 3]``, run ``chunk`` frames at a time.  D is PTI's input and D_recolor its recolor-guidance target.  ``flip_target=None`` draws once per
    chunk (the reference draws per frame: ``chunk=1``).  The reference's per-frame PNG saves are not made.  Every argument of every stage is checked before the
    first launch; an empty clip returns empty tensors of the right shapes."""
    name = "reenact_recolor_clip"
    if flip_target is not None and not isinstance(flip_target, bool):
        raise TypeError(f"{name}: flip_target is True, False or None, got {type(flip_target).__name__}")
    _, out_hw = _reenact_args_checked(name, generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, source_u8, targets_u8, size, True, channel_order,
                                      batch, chunk, make_animation_kw)
    dev, n = targets_u8.device, targets_u8.shape[0]
    w = _recolor_args_checked(name, parser, blender, codeformer, esr, torch.empty((0,) + out_hw + (3,), dtype=torch.uint8, device=dev), targets_u8[:0], w)[2]
    if n == 0:
        return torch.empty((0,) + out_hw + (3,), dtype=torch.uint8, device=dev), torch.empty((0, 1024, 1024, 3), dtype=torch.uint8, device=dev)
    D = _reenact_drivens_run(generator, kp_detector, he_estimator, detector, gpen, parsenet, sr, source_u8, targets_u8, size, True, channel_order, batch, chunk,
                             make_animation_kw)
    rec = [recolor_frames(parser, blender, codeformer, esr, D[i:i + chunk], targets_u8[i:i + chunk], flip_target, w) for i in range(0, n, chunk)]
    return D, (rec[0] if len(rec) == 1 else torch.cat(rec))


# ------------------------------------------------------------------------------------ f25: face inpainting, stage 1
@torch.no_grad()
def inpaint_faces(net, faces_u8: torch.Tensor, mask: torch.Tensor, noise=None, generator=None) -> torch.Tensor:
    """The whole of ``inpainting(face_img, mask)`` (swap_face_fine/face_inpainting.py:21-51) for a batch on the device: ``ops.pil_resize(faces, (S, S))``
    (Pillow's default BICUBIC, bit-exact), ``ops.cv_mask_support(mask, S)`` (``cv2.resize(mask.astype(float), (S, S)) > 0``, a restatement cv2 was never run
    against) and ``ops.inpaint_image`` (the network's input with each face's own hole share, ``FaceInpaintingArch``, the clamp, the composite and the rounding).
    ``faces_u8``: uint8 ``[n, H, W, 3]`` RGB; ``mask``: non-negative float32 or uint8 ``[n, h, w]``, anything above zero is hole; ``net``: an
    ``ops.FaceInpainting`` in eval mode or a mapping with its keys, whose size ``S`` (256 for ``net_g_50000.pth``) is read off them; ``noise`` / ``generator`` as
    ``ops.inpaint_forward`` takes them (None: fresh normal noise per call, as the reference draws it).  Returns uint8 ``[n, S, S, 3]``; an empty batch returns an
    empty tensor.  The rest of the caller's ``_inpaint_face`` (the dilation and blurs of the mask, CodeFormer, the resize back and the blend) is stage 2.  Every
    argument is checked before the first launch."""
    from . import ops_inpaint
    name = "inpaint_faces"
    checked = ops_inpaint._weights_checked(name, net)
    S = checked[1][0]
    netweights._tensor_checked(name, "faces_u8", faces_u8, torch.uint8, 4, "uint8 [n, H, W, 3] RGB faces")
    n, H, W, c = faces_u8.shape
    if c != 3 or H < 1 or W < 1:
        raise ValueError(f"{name}: faces_u8: expected uint8 [n, H, W, 3] RGB faces, got {tuple(faces_u8.shape)}")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.float32, torch.uint8) or mask.dim() != 3:
        raise ValueError(f"{name}: mask: expected a float32 or uint8 [n, h, w] tensor, got {getattr(mask, 'dtype', type(mask).__name__)} "
                         f"{tuple(getattr(mask, 'shape', ()))}")
    if mask.shape[0] != n or mask.shape[1] < 1 or mask.shape[2] < 1 or max(mask.shape[1:]) > ops_inpaint.INPAINT_MAX_SIDE:
        raise ValueError(f"{name}: mask is {tuple(mask.shape)}: a mask of another batch or an empty or oversized one, expected [{n}, h, w] with "
                         f"1 <= h, w <= {ops_inpaint.INPAINT_MAX_SIDE}")
    netweights._cuda_checked(name, faces_u8=faces_u8, mask=mask)
    netweights._devices_checked(name, "faces_u8", faces_u8, checked[2])
    if mask.device != faces_u8.device:
        raise RuntimeError(f"{name}: device mismatch: mask on {mask.device}, faces_u8 on {faces_u8.device}")
    if noise is not None:
        ops_inpaint._noise_checked(name, noise, n, S, faces_u8.device)
    ops_inpaint._generator_checked(name, generator, faces_u8.device)
    ops_inpaint._arith_checked(name)
    if n == 0:
        return torch.empty((0, S, S, 3), dtype=torch.uint8, device=faces_u8.device)
    return ops_inpaint.inpaint_image(ops.pil_resize(faces_u8, (S, S)), ops_inpaint.cv_mask_support(mask, S), net, noise=noise, generator=generator)
