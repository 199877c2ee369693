"""CPU side of the PTI recolor term: the ``D_recolor`` frames in the hand-off (dump / load, a directory written the reference's way) and the argument
refusals of ``pti_step``, ``GraphedPTIStep`` and ``tune_clip`` that come before any launch."""
import os

import numpy as np
import pytest
import torch

from e4s2024_amd import handoff, pti


def _frames(n, seed, side=16):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, side, side), generator=g) * 2 - 1


def test_recolor_dump_load_round_trip(tmp_path):
    drv, rec = _frames(2, 1), _frames(2, 2)
    handoff.dump(handoff.ClipBatch(driven=drv, driven_recolor=rec), str(tmp_path), first_index=3)
    assert sorted(os.listdir(tmp_path / "imgs")) == ["D_0003.png", "D_0004.png", "D_recolor_0003.png", "D_recolor_0004.png"]
    back = handoff.load(str(tmp_path), first_index=3, size=16)
    assert back.driven_recolor.shape == (2, 3, 16, 16) and len(back) == 2
    u8 = ((rec.clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8).float()          # tensor2im's truncating cast
    assert torch.allclose(back.driven_recolor, u8 / 127.5 - 1, atol=1e-6)
    assert handoff.ClipBatch(driven_recolor=rec).to("cpu").driven_recolor is not None


def test_load_reads_reference_recolor_directory(tmp_path):
    """The video pipeline writes imgs/D_recolor_%04d.png (face_swap_video_pipeline.py:306-310); the coach converts them with im2tensor(std=False)."""
    from PIL import Image
    os.makedirs(tmp_path / "imgs")
    arr = np.random.default_rng(0).integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)
    for i in range(2):
        Image.fromarray(arr[i]).save(tmp_path / "imgs" / f"D_recolor_{i:04d}.png")
    clip = handoff.load(str(tmp_path), size=8)
    assert clip.driven is None
    want = torch.from_numpy(arr).permute(0, 3, 1, 2).float() / 127.5 - 1
    assert torch.equal(clip.driven_recolor, want)
    assert handoff.load(str(tmp_path), count=1, size=8).driven_recolor.shape[0] == 1


class _NoNet:
    def cal_style_codes(self, *a, **k):
        raise AssertionError("nothing may run before the arguments are checked")

    gen_img = cal_style_codes


def test_pti_step_refuses_mismatched_recolor():
    tgt = torch.zeros((1, 3, 16, 16))
    with pytest.raises(ValueError, match="recolor"):
        pti.pti_step(_NoNet(), None, torch.zeros((1, 12, 1280)), torch.zeros((1, 16, 16), dtype=torch.uint8), tgt, recolor=torch.zeros((2, 3, 16, 16)))


def test_graphed_step_refuses_mismatched_recolor():
    tgt = torch.zeros((1, 3, 16, 16))
    with pytest.raises(ValueError, match="recolor"):
        pti.GraphedPTIStep(_NoNet(), None, torch.zeros((1, 12, 1280)), torch.zeros((1, 16, 16), dtype=torch.uint8), tgt, torch.ones((1, 1, 16, 16)),
                           recolor=torch.zeros((1, 3, 8, 8)))


def test_tune_clip_refuses_recolor_frame_count():
    imgs = torch.zeros((3, 3, 16, 16))
    with pytest.raises(ValueError, match="recolor"):
        pti.tune_clip(_NoNet(), None, imgs, torch.zeros((3, 16, 16), dtype=torch.uint8), torch.zeros((3, 12, 1280)), 1, recolor=torch.zeros((2, 3, 16, 16)))


def test_target_cache_frame_range():
    c = pti.TargetCache.__new__(pti.TargetCache)
    c.n, c.frame = 2, torch.zeros((1,), dtype=torch.int32)
    c.select(1)
    assert int(c.frame) == 1
    with pytest.raises(IndexError):
        c.select(2)
