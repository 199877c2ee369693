"""GPU tests of row f8, the semantic colour reference of the Blender recolouring network on the device (``csrc/colorref.hip``): ``ops.color_reference``,
``ops.blender_part_masks`` / ``blender_packages`` and the drop-in ``semantic_tools`` against the float64 model (``colorref_model``) and the reference's own
outputs (``g20_color_refer.npz``).

The bound of a case is ``4 * e32`` with a floor of 2e-7 (three float32 ulps at 1.0), where ``e32`` is the MODEL run in float32 against the model in
float64 on the same inputs — the reference's arithmetic class, computed here, never the code under test.  Four, because the tiled online softmax sums in
another order and rescales partial sums; no fixed number, because the error of ``exp(tau c)`` grows with ``tau`` by itself.  The mask, grey and
background channels of the packages are exact.

Measured on an MI355X: worst ``err / e32`` = 1.46 (the hand-built parts at tau = 40), 0.21 .. 1.25 on the other cases."""
import numpy as np
import pytest
import torch

import colorref_model as RM
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
_WORST = {"ratio": 0.0}


def _dev(*arrays):
    return tuple(T(a).to(DEV) for a in arrays)


def _keys(present_row):
    return [n for i, n in enumerate(RM.PARTS) if present_row[i]]


def _e32(tag):
    return RM.max_err([RM.reference_outputs(tag, torch.float32)[i] for i in (0, 2, 3)], [RM.reference_outputs(tag)[i] for i in (0, 2, 3)])


def _note(tag, err, e32):
    _WORST["ratio"] = max(_WORST["ratio"], err / max(e32, RM.FLOOR / RM.MARGIN))
    print(f"{tag}: kernel against float64 {err:.3e}, e32 {e32:.3e}, bound {RM.bound(e32):.3e}")
    record_parity("colorref.worst_err_over_e32", _WORST["ratio"], RM.MARGIN, "kernel against the float64 model, in units of the float32 model's own error")


@pytest.mark.parametrize("tag", RM.FIXTURE_REFER_CASES + RM.MODEL_ONLY_CASES)
def test_kernel_against_the_float64_model(tag):
    img_t, fa, ft, pa, pt, tau = RM.reference_inputs(tag)
    want = RM.reference_outputs(tag)
    refs, present, inv, inv_target = ops.color_reference(*_dev(img_t, fa, ft, pa, pt), tau)
    assert refs.dtype == inv.dtype == inv_target.dtype == torch.float32 and present.dtype == torch.uint8 and present.is_cuda
    assert tuple(refs.shape) == want[0].shape and tuple(inv.shape) == tuple(inv_target.shape) == want[2].shape
    assert np.array_equal(present.cpu().numpy(), want[1])
    err = RM.max_err((refs.cpu().numpy(), inv.cpu().numpy(), inv_target.cpu().numpy()), (want[0], want[2], want[3]))
    e32 = _e32(tag)
    _note(tag, err, e32)
    assert err <= RM.bound(e32)
    assert not refs.cpu().numpy()[want[0] == 0].any()                              # zero outside a part's A pixels and for absent parts
    if tag == "batch3":
        for b, name in enumerate(RM.BATCH3_ABSENT):
            assert _keys(want[1][b]) == [n for n in RM.PARTS if n != name]


@pytest.mark.parametrize("tag", RM.FIXTURE_REFER_CASES)
def test_present_flags_and_dropin_against_the_fixture(tag):
    g = load_golden("g20_color_refer")
    install_dropin()
    from swap_face_fine.Blender.model_center import semantic_tools as st
    img_t, fa, ft, pa, pt, tau = RM.reference_inputs(tag)
    keys = str(g[f"{tag}.keys"]).split(",")
    d_img, d_fa, d_ft, d_pa, d_pt = _dev(img_t, fa, ft, pa, pt)
    _, present = ops.color_reference(d_img, d_fa, d_ft, d_pa, d_pt, tau, compute_inv=False)
    assert _keys(present[0].cpu().numpy()) == keys
    da, dt = ({k: v.to(DEV) for k, v in d.items()} for d in RM.part_dicts(pa, pt))
    refs, pair = st.get_color_refer(d_img, d_fa, d_ft, da, dt, torch.nn.Parameter(torch.tensor(float(tau), device=DEV)), True, False)
    assert list(refs) == keys and len(pair) == 2
    assert all(tuple(v.shape) == (1, 3) + fa.shape[-2:] and v.dtype == torch.float32 for v in list(refs.values()) + pair)
    e32 = _e32(tag)
    if tag in ("forward", "two_class"):                                           # the fixture holds the packages of these; the pair is the same call's
        got, ref = (pair[0][0], pair[1][0]), (g[f"{tag}.inv"], g[f"{tag}.inv_target"])
        err = RM.max_err([v.cpu().numpy() for v in got], ref)
    else:
        ru, iu = RM.one_pixel_outputs(pa, pt, *fa.shape[-2:])                     # the reference writes zero for one-pixel parts: not compared
        planes = np.zeros((9, 3) + fa.shape[-2:], np.float32)
        for k, v in refs.items():
            planes[RM.PARTS.index(k)] = v[0].cpu().numpy()
        ru, iu = np.broadcast_to(ru, planes.shape), np.broadcast_to(iu, (3,) + fa.shape[-2:])
        err = RM.max_err((np.where(ru, 0, planes), np.where(iu, 0, pair[0][0].cpu().numpy()), pair[1][0].cpu().numpy()),
                         (np.where(ru, 0, g[f"{tag}.refs"]), np.where(iu, 0, g[f"{tag}.inv"]), g[f"{tag}.inv_target"]))
    print(f"{tag}: drop-in against the reference {err:.3e}, e32 {e32:.3e}, bound {RM.bound(e32):.3e}")
    assert err <= RM.bound(e32)
    assert st.get_color_refer(d_img, d_fa, d_ft, da, dt, float(tau), compute_inv=False)[1] == []


def test_dropin_helpers_on_the_device():
    install_dropin()
    from swap_face_fine.Blender.model_center import semantic_tools as st
    _, _, la, lt, _, _, _ = RM.case_forward()
    pa, pt, head_a, head_t, e_at = RM.part_masks(la, lt)
    d = st.get_part_dict(T(la).to(DEV).long())
    assert np.array_equal(d["head"].cpu().numpy(), head_a[:, 0])
    dil = st.get_dilated_mask((d["head"] + st.get_part_dict(T(lt).to(DEV).long())["head"]).clamp(0, 1))
    assert dil.dtype == torch.int64 and np.array_equal(dil.cpu().numpy(), e_at[:, 0])


@pytest.mark.parametrize("tag,maker", [("forward", RM.case_forward), ("two_class", RM.case_two_class)])
def test_packages_against_the_fixture_and_the_model(tag, maker):
    g = load_golden("g20_color_refer")
    c = maker()
    want, (w_inv, w_tgt), w_present = RM.packages(*c)
    w32, (i32, t32), _ = RM.packages(*c, dtype=torch.float32)
    e32 = RM.max_err((w32[:, :6], i32, t32), (want[:, :6], w_inv, w_tgt))
    pa, pt, head_a, head_t, e_at = RM.part_masks(c[2], c[3])
    got_masks = ops.blender_part_masks(*_dev(c[2], c[3]))
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got_masks, (pa, pt, head_a, head_t, e_at)))
    assert got_masks[0].dtype == torch.uint8 and got_masks[2].dtype == torch.float32
    pack, (inv, inv_target) = ops.blender_packages(*_dev(*c[:6]), c[6])
    pack, inv, inv_target = pack.cpu().numpy(), inv.cpu().numpy(), inv_target.cpu().numpy()
    assert pack.shape == want.shape and pack.dtype == np.float32
    assert np.array_equal(pack[0, 6:], g[f"{tag}.packages"][6:]) and np.array_equal(pack[:, 6:], want[:, 6:].astype(np.float32))     # exact
    err = RM.max_err((pack[:, :6], inv, inv_target), (want[:, :6], w_inv, w_tgt))
    _note(f"packages.{tag}", err, e32)
    assert err <= RM.bound(e32)
    err_ref = RM.max_err((pack[0, :6], inv[0], inv_target[0]), (g[f"{tag}.packages"][:6], g[f"{tag}.inv"], g[f"{tag}.inv_target"]))
    print(f"packages.{tag}: against the reference {err_ref:.3e}")
    assert err_ref <= RM.bound(e32)


def test_fewer_than_two_parts_give_zero_references():
    img_a, img_t, la, lt, fa, ft, tau = RM.case_two_class()
    la = la.copy()
    la[:] = 1
    pack, _ = ops.blender_packages(*_dev(img_a, img_t, la, lt, fa, ft), tau)
    assert not pack[:, :6].any() and bool(pack[:, 6].all())


def test_batch_is_per_sample_and_runs_are_reproducible():
    c = RM.case_batch3()
    dev = _dev(*c[:6])
    whole = ops.blender_packages(*dev, c[6])
    again = ops.blender_packages(*dev, c[6])
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1][0], again[1][0]) and torch.equal(whole[1][1], again[1][1])
    img_t, fa, ft, pa, pt, tau = RM.reference_inputs("batch3")
    d = _dev(img_t, fa, ft, pa, pt)
    refs = ops.color_reference(*d, tau)
    for b in range(3):
        one = ops.blender_packages(*(t[b:b + 1] for t in dev), c[6])
        assert torch.equal(one[0], whole[0][b:b + 1]) and torch.equal(one[1][0], whole[1][0][b:b + 1]) and torch.equal(one[1][1], whole[1][1][b:b + 1])
        r1 = ops.color_reference(*(t[b:b + 1] for t in d), tau)
        assert all(torch.equal(x, y[b:b + 1]) for x, y in zip(r1, refs))


def test_graph_capture_and_tau_on_the_device():
    """No host synchronisation: ``blender_packages`` captured in a graph and replayed twice gives the eager bits; ``tau`` as a device tensor is read by the
    kernel at every replay."""
    c = RM.case_forward()
    dev = _dev(*c[:6])
    tau = torch.tensor([7.0], device=DEV)
    eager7 = ops.blender_packages(*dev, tau)
    assert torch.equal(eager7[0], ops.blender_packages(*dev, 7.0)[0])            # a float and a device tensor: the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.blender_packages(*dev, tau)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.blender_packages(*dev, tau)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager7[0]) and torch.equal(out[1][0], eager7[1][0]) and torch.equal(out[1][1], eager7[1][1])
    tau.fill_(-3.0)
    graph.replay()
    torch.cuda.synchronize()
    eager_m3 = ops.blender_packages(*dev, -3.0)
    assert torch.equal(out[0], eager_m3[0]) and torch.equal(out[1][0], eager_m3[1][0]) and not torch.equal(out[0], eager7[0])


def test_without_the_inverse_the_references_are_the_same_bits():
    img_t, fa, ft, pa, pt, tau = RM.reference_inputs("large")
    d = _dev(img_t, fa, ft, pa, pt)
    full = ops.color_reference(*d, tau)
    short = ops.color_reference(*d, tau, compute_inv=False)
    assert len(short) == 2 and len(full) == 4
    assert torch.equal(short[0], full[0]) and torch.equal(short[1], full[1])
    assert ops.color_reference(*(t[:0] for t in d), tau)[0].shape == (0, 9, 3, 64, 64)
