"""CPU suite of the depthwise 3x3 backward passes and of ShuffleNetV2 training: tests/dwconv_restate.py against torch's
float64 autograd (so that the GPU tests compare the kernels with a restatement that is itself held to torch), the
zero-stuffing identities train.conv3x3_s2's backward rests on, train.shufflenet_forward with torch's float64 operations
against the plain restatement of the reference forward, encode.get_loss_shufflenet against the written-out formula, the
shape-only queries of the C ABI, and every refusal that needs no device."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwconv_restate as dr


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(pkg.__name__ + ".encode")


@pytest.fixture(scope="module")
def shuf(pkg):
    return importlib.import_module(pkg.__name__ + ".shufflenet")


# ---- the restatements against float64 autograd ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dr.CASES, ids=dr.case_id)
def test_restatements_are_exact_on_integers(c):
    x, gy, wt = dr.exact_operands(c)
    _, dx64, dw64 = dr.autograd64(x, wt, gy, c.stride)
    dw, db, sw, sb = dr.wgrad_restate(x.numpy(), gy.numpy(), c.stride)
    assert max(sw.max(), sb.max()) < 2 ** 24
    assert np.array_equal(dw, dw64.numpy()) and np.array_equal(db, gy.double().sum((0, 2, 3)).numpy())
    for dt in (np.float32, np.float64):
        dx = dr.dgrad_restate(gy.numpy(), wt.numpy(), c.h, c.w, c.stride, dt)
        assert dx.dtype == dt and np.array_equal(dx.astype(np.float64), dx64.numpy())


@pytest.mark.parametrize("c", dr.CASES, ids=dr.case_id)
def test_restatements_on_random_operands(c):
    x, gy, wt = dr.random_operands(c)
    _, dx64, dw64 = dr.autograd64(x, wt, gy, c.stride)
    dw, db, sw, sb = dr.wgrad_restate(x.numpy(), gy.numpy(), c.stride)
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    p = c.n * ho * wo
    # two float64 sums of the same terms in different orders: (P - 1) u sum |terms| each
    assert (np.abs(dw - dw64.numpy()) <= 2 * p * dr.U * sw).all()
    assert (np.abs(db - gy.double().sum((0, 2, 3)).numpy()) <= 2 * p * dr.U * sb).all()
    dx = dr.dgrad_restate(gy.numpy(), wt.numpy(), c.h, c.w, c.stride, np.float64)
    # at most 9 products and 9 adds per element, each term at most max |gy| * |w|
    bound = 9 * 2 * dr.U * np.abs(gy.numpy()).astype(np.float64).max() * np.abs(wt.numpy()).astype(np.float64).reshape(c.c, 9).sum(1)
    assert (np.abs(dx - dx64.numpy()) <= bound.reshape(1, c.c, 1, 1)).all()
    # the fp32 restatement: at most 9 products and 9 adds, each within 2^-24 of a partial sum bounded by the same quantity
    dx32 = dr.dgrad_restate(gy.numpy(), wt.numpy(), c.h, c.w, c.stride)
    bound32 = 18 * dr.U32 * np.abs(gy.numpy()).astype(np.float64).max() * np.abs(wt.numpy()).astype(np.float64).reshape(c.c, 9).sum(1)
    assert (np.abs(dx32.astype(np.float64) - dx64.numpy()) <= bound32.reshape(1, c.c, 1, 1)).all()


def test_tap_major_is_the_forwards_packing():
    w = torch.arange(2 * 9, dtype=torch.float32).reshape(2, 1, 3, 3)
    t = dr.tap_major(w.numpy())
    assert t.shape == (9, 2) and all(t[ky * 3 + kx, c] == w[c, 0, ky, kx] for c in range(2) for ky in range(3) for kx in range(3))


@pytest.mark.parametrize("c", dr.SLAB_CASES, ids=dr.case_id)
def test_slab_cases_keep_their_promise(capi, c):
    slab, slabs = dr.slab_geometry(c.n, c.h, c.w, c.stride)
    assert capi.lib.rtpose_dwconv3x3_wgrad_slabs(c.c, c.n, c.h, c.w, c.stride) == slabs
    assert dr.slab_facts(c, slab, slabs) == dict(slabs=5, ragged=True, inside=True, at_image=True)


def test_queries_follow_the_shape_only(capi):
    lib = capi.lib
    for c in dr.CASES:
        assert lib.rtpose_dwconv3x3_wgrad_slabs(c.c, c.n, c.h, c.w, c.stride) == dr.slab_geometry(c.n, c.h, c.w, c.stride)[1]
        assert lib.rtpose_dwconv3x3_wgrad_workspace_doubles(c.c, c.n, c.h, c.w, c.stride) == dr.workspace_doubles(c.c, c.n, c.h, c.w, c.stride)
    # the network's own shapes at batch 32: 46 x 46 outputs, slabs of 128 pixels
    assert dr.slab_geometry(32, 92, 92, 2) == dr.slab_geometry(32, 46, 46, 1) == (128, 529)
    assert lib.rtpose_dwconv3x3_wgrad_slabs(116, 32, 46, 46, 1) == 529
    for bad in ((0, 1, 4, 4, 1), (-1, 1, 4, 4, 2), (4, 0, 4, 4, 1), (4, 1, 0, 4, 1), (4, 1, 4, 0, 1), (4, 1, 4, 4, 0), (4, 1, 4, 4, 3),
                (4, 1 << 16, 1 << 8, 1 << 8, 1)):
        assert lib.rtpose_dwconv3x3_wgrad_slabs(*bad) == 0 and lib.rtpose_dwconv3x3_wgrad_workspace_doubles(*bad) == 0, bad


def test_c_abi_refusals_before_any_hip_call(capi):
    c = dr.CASES[3]          # 2 x 3 x 5 x 7 at stride 2
    assert (c.n, c.c, c.h, c.w, c.stride) == (2, 3, 5, 7, 2)
    bufs = [np.zeros(64, np.float64) for _ in range(7)]           # host memory: refused before anything could read it
    for what, rc in dr.host_refusals(capi, c, *[capi.ptr(b) for b in bufs]):
        assert rc == -1, what                                      # RTPOSE_E_INVAL
        assert capi.last_error(), what


# ---- the stem's backward by zero stuffing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(8, 6), (7, 9), (8, 9), (5, 4), (1, 1), (2, 3)])
def test_zero_stuffing_identities_of_the_stem(h, w):
    g = torch.Generator().manual_seed(h * 16 + w)
    for exact in (True, False):
        if exact:
            x, wt = torch.randint(-3, 4, (2, 3, h, w), generator=g).double(), torch.randint(-2, 3, (24, 3, 3, 3), generator=g).double()
        else:
            x, wt = torch.randn(2, 3, h, w, generator=g).double(), torch.randn(24, 3, 3, 3, generator=g).double()
        x.requires_grad_(True), wt.requires_grad_(True)
        y = F.conv2d(x, wt, None, 2, 1)
        assert tuple(y.shape[2:]) == dr.out_size(h, w, 2)
        gy = torch.randint(-3, 4, y.shape, generator=g).double() if exact else torch.randn(y.shape, generator=g).double()
        dx64, dw64 = torch.autograd.grad(y, (x, wt), gy)
        dw, dx = dr.stem_grads_by_stuffing(x.detach(), wt.detach(), gy)
        if exact:
            assert torch.equal(dw, dw64) and torch.equal(dx, dx64)
        else:
            assert torch.allclose(dw, dw64, rtol=0, atol=1e-12 * (1 + dw64.abs().max().item()))
            assert torch.allclose(dx, dx64, rtol=0, atol=1e-12 * (1 + dx64.abs().max().item()))


# ---- train.shufflenet_forward with torch's operations against the plain restatement ---------------------------------------------------------
@pytest.fixture(scope="module")
def model64(shuf):
    torch.manual_seed(0)
    return dr.seed_module(shuf.Network(1.0), 5).double().train()


def test_shufflenet_forward_is_the_reference_forward(train, model64):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 36, 44, generator=g).double()         # maps: 18 x 22 at the stem, 9 x 11 at the pool, 5 x 6 at the heads
    sd = dr.tensors_of(model64)
    paf_r, heat_r = dr.ref_forward(sd, x)
    before = {k: v.clone() for k, v in model64.state_dict().items()}
    out, saved = train.shufflenet_forward(model64, x, *dr.torch_ops())
    try:
        assert isinstance(out, list) and isinstance(saved, list) and out[0] is saved[0] and out[1] is saved[1]
        assert tuple(out[0].shape) == (2, 38, 5, 6) and tuple(out[1].shape) == (2, 19, 5, 6)
        assert torch.equal(out[0], paf_r) and torch.equal(out[1], heat_r)
        after = model64.state_dict()
        moved = 0
        for k, v in after.items():
            assert torch.equal(v, sd[k].detach()), k
            if k.endswith("num_batches_tracked"):
                assert int(v) == 1, k
            elif k.endswith(("running_mean", "running_var")):
                moved += int(not torch.equal(v, before[k]))
        assert moved == 2 * sum(1 for k in after if k.endswith("running_mean"))
        # gradients too: the same operations in the same order
        (out[0].square().mean() + out[1].square().mean()).backward()
        (paf_r.square().mean() + heat_r.square().mean()).backward()
        for n, p in model64.named_parameters():
            assert torch.equal(p.grad, sd[n].grad), n
    finally:
        model64.load_state_dict(before)
        model64.zero_grad(set_to_none=True)


def test_shufflenet_block_orders(train, shuf):
    """both kinds of block against the restatement: the two-branch block (conv0 beside conv) and the split block"""
    for cin, cout, stride, two in ((24, 116, 2, True), (116, 116, 1, False), (116, 232, 1, True)):
        blk = dr.seed_module(shuf.BasicBlock(cin, cout, stride, two), cin + stride).double().train()
        sd = {"b." + k: v for k, v in dr.tensors_of(blk).items()}
        x = torch.randn(2, cin, 9, 8, generator=torch.Generator().manual_seed(cin)).double()
        conv, bn, dw, _ = dr.torch_ops()
        got = train.shufflenet_block(blk, x, conv, bn, dw)
        assert torch.equal(got, dr.ref_block(sd, "b", x, stride, two))
        assert got.shape[1] == cout


# ---- encode.get_loss_shufflenet -----------------------------------------------------------------------------------------------------------
def test_get_loss_shufflenet_is_the_written_out_formula(encode):
    g = torch.Generator().manual_seed(9)
    paf, heat = torch.randn(2, 38, 5, 6, generator=g).double().requires_grad_(True), torch.randn(2, 19, 5, 6, generator=g).double()
    vec, ht = torch.randn(2, 38, 5, 6, generator=g).double(), torch.rand(2, 19, 5, 6, generator=g).double()
    vw, hw = (torch.rand(2, 38, 5, 6, generator=g) > 0.3).double(), (torch.rand(2, 19, 5, 6, generator=g) > 0.3).double()
    total, log = encode.get_loss_shufflenet([paf, heat], ht, hw, vec, vw)
    l1 = ((paf * vw - vec * vw) ** 2).sum() / paf.numel()
    l2 = ((heat * hw - hw * ht) ** 2).sum() / heat.numel()
    assert torch.allclose(total, l1 + l2, rtol=1e-14, atol=0) and total.grad_fn is not None
    assert list(log) == ["paf", "heatmap", "max_ht", "min_ht", "max_paf", "min_paf"]
    assert abs(log["paf"] - l1.item()) <= 1e-14 * l1.item() and abs(log["heatmap"] - l2.item()) <= 1e-14 * l2.item()
    assert log["max_ht"] == heat[:, :-1].max().item() and log["min_ht"] == heat[:, :-1].min().item()
    assert log["max_paf"] == paf.max().item() and log["min_paf"] == paf.min().item()
    ones, _ = encode.get_loss_shufflenet([paf, heat], ht, torch.ones_like(ht), vec, torch.ones_like(vec))
    none, _ = encode.get_loss_shufflenet([paf, heat], ht, None, vec, None)
    assert torch.equal(ones, none) and torch.equal(none, F.mse_loss(paf, vec) + F.mse_loss(heat, ht))
    with pytest.raises(ValueError, match="get_loss_shufflenet wants"):
        encode.get_loss_shufflenet([paf], ht, None, vec, None)


# ---- refusals that need no device ------------------------------------------------------------------------------------------------------------
def test_python_refusals(capi, train, shuf, pkg):
    err = capi.RtposeError
    m = shuf.Network(1.0)
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(TypeError, match="takes a shufflenet.Network"):
        train.shufflenet_forward(torch.nn.Conv2d(1, 1, 1), x, *dr.torch_ops())
    with pytest.raises(err, match=r"call \.train\(\) first"):
        train.shufflenet_forward(m.eval(), x, *dr.torch_ops())
    m.train()
    with pytest.raises(err, match="no CPU fallback"):
        train.forward_train(m, x)
    with pytest.raises(TypeError, match="freezes nothing of a shufflenet.Network"):
        train.freeze_trunk(m)
    with pytest.raises(TypeError, match="shufflenet.Network; got Conv2d"):
        train.forward_train(torch.nn.Conv2d(1, 1, 1), x)
    vgg = importlib.import_module(pkg.__name__ + ".network").RtposeVGG()
    with pytest.raises(TypeError, match="heat_mask / paf_mask belong to"):
        train.train_step(vgg, None, x, None, None, heat_mask=x)
    w = torch.zeros(4, 1, 3, 3)
    with pytest.raises(err, match="train.dwconv3x3 runs only on an MI355X"):
        train.dwconv3x3(torch.zeros(1, 4, 5, 5), w)
    with pytest.raises(err, match="train.conv3x3_s2 runs only on an MI355X"):
        train.conv3x3_s2(x, torch.zeros(24, 3, 3, 3))

