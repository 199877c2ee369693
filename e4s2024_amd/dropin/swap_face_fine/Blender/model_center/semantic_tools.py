"""Drop-in for the reference's ``swap_face_fine/Blender/model_center/semantic_tools.py``: the helpers ``Referencer.forward`` calls, with the semantic colour
reference on the HIP kernels of ``e4s2024_amd.ops_recolor`` (``csrc/colorref.hip``).  Signatures and return structures are the reference's.

Where this differs from the reference, each time where the reference's result is not a function of its inputs (``ops_recolor`` has the details):

* a batch is processed per sample, each sample as a batch-of-one call (the reference pads to the batch's largest part through ``topk`` ties);
* ``light=True`` (top-1000 subsampling: the same tie problem at batch 1) raises ``NotImplementedError``;
* a part with a single pixel gets its softmax's value like any other part (the reference divides 0 by 0 in its pixel numbering and writes zero);
* ``'head'`` of the part dictionaries is taken to be the sum of the eight parts, which is what ``get_part_dict`` makes it.

``get_color_refer`` reads the 9 presence flags per sample back ONCE per call, to know the dictionary's keys; the reference synchronises about twenty times
(two ``.item()`` per part and the asserts of its grids)."""
import torch
import torch.nn.functional as F

from e4s2024_amd import ops

name_to_ids = {name: list(ids) for name, ids in ops.BLENDER_PART_IDS.items()}

_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


def chunk_cosine_similarity(x1: torch.Tensor, x2: torch.Tensor, dim: int = 1):
    """Cosine similarity of ``[1, D, N, 1]`` against ``[1, D, 1, M]`` -> ``[1, N, M]``.  Kept for callers of the name; ``get_color_refer`` never forms this
    matrix (the scores live in registers, tile by tile)."""
    return F.cosine_similarity(x1, x2, dim=dim)


def _parts_from_dict(part_dict, which):
    missing = [n for n in ops.BLENDER_PARTS if n not in part_dict]
    if missing:
        raise KeyError(f"get_color_refer: {which} lacks the parts {missing}")
    return torch.stack([part_dict[n] != 0 for n in ops.BLENDER_PARTS], dim=1).to(torch.uint8)


def get_color_refer(img_T, feats_A, feats_T, part_dict_A, part_dict_T, trainable_tao, compute_inv=True, light=False):
    """``(color_ref_dict, color_inv_ref_pair)``: per part present in ANY sample its reference ``[bs, 3, h, w]``, already multiplied by the part's mask (samples
    that lack the part hold zeros), in the order of the parts; and ``[inv, inv_target]`` (``[]`` without ``compute_inv``)."""
    if light:
        raise NotImplementedError("get_color_refer: light=True (top-1000 subsampling through topk ties) is not offered")
    parts_a, parts_t = _parts_from_dict(part_dict_A, "part_dict_A"), _parts_from_dict(part_dict_T, "part_dict_T")
    tau = trainable_tao
    if isinstance(tau, torch.Tensor):
        tau = tau.detach().float().reshape(1) if tau.is_cuda else float(tau)
    out = ops.color_reference(img_T, feats_A, feats_T, parts_a, parts_t, tau, compute_inv=compute_inv)
    refs, present = out[0], out[1]
    any_present = present.any(0).cpu().tolist()                             # the one read-back
    color_ref_dict = {n: refs[:, p] for p, n in enumerate(ops.BLENDER_PARTS) if any_present[p]}
    return color_ref_dict, ([out[2], out[3]] if compute_inv else [])


def get_part_dict(masks):
    """``[bs, H, W]`` 19-class maps -> the eight part masks (int64 0/1) and ``'head'``, their sum."""
    part_dict = {name: sum((masks == i) for i in ids).long() for name, ids in name_to_ids.items()}
    part_dict["head"] = sum(part_dict.values())
    return part_dict


def get_greyscale_head(img_A, mask_A_head):
    """``clamp(0.299 R + 0.587 G + 0.114 B, 0, 1) * head`` of the de-normalised image: ``[bs, H, W]``."""
    img01 = (img_A * img_A.new_tensor(_STD).view(1, 3, 1, 1) + img_A.new_tensor(_MEAN).view(1, 3, 1, 1)).clamp(0, 1)
    grey = img01[:, 0] * 0.299 + img01[:, 1] * 0.587 + img01[:, 2] * 0.114
    return grey.clamp(0, 1) * mask_A_head


def get_dilated_mask(mask, ratio=0.1):
    """The flat ``k x k`` maximum of a ``[bs, H, W]`` mask, ``k = int(W * ratio / 2) * 2 + 1``, as int64 (``ops.grey_dilate``)."""
    radius = int(mask.shape[-1] * ratio / 2)
    return ops.grey_dilate(mask[:, None].float(), radius)[:, 0].long()
