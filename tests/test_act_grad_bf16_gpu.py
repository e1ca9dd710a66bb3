"""GPU suite of rtpose_relu_grad_bf16 (header section 2b, csrc/act_grad_bf16.hip): raw bits against
tests/act_grad_bf16_restate.py on slices of wider buffers whose other channels, gaps and slack hold a NaN sentinel - after
every launch they are intact, bit for bit.

The grid (act_grad_bf16_restate): N = 3, 5 x 7 maps, channels 1 / 8 / 19 / 38 / 48 at choff 0, 8 (16-byte pieces, with a partial
last unit where channels % 8) and 3 (element by element) of a cstride of 64; bases on and off a 16-byte boundary; gaps of
0, 1 and 3 chosen differently for y, gy and out; in place and out of place.  y holds +-0, NaNs, +-Inf, subnormals and negatives,
gy NaNs with payloads and Inf."""
import ctypes as C

import numpy as np
import pytest
import torch

import act_grad_bf16_restate as ar
import conv_driver as cd
import layout_restate as lr

pytestmark = pytest.mark.gpu

SLACK = 8         # elements in front of a buffer: room for the base shifts


def host_buffer(capi, lay, bits=None):
    """A layout buffer on the host as uint16: the sentinel everywhere, `bits` [n, ch, h, w] at the valid pixels of the slice"""
    a = np.full(cd.npx(capi, lay, ar.N, ar.H, ar.W) * lay.cstride, ar.SENTINEL16, dtype=np.uint16)
    return a if bits is None else lr.scatter(a, lay, bits)


def on_device(host, shift, dev):
    """(whole allocation, the view that starts `shift` elements past a 16-byte boundary and holds `host`)"""
    whole = torch.full((SLACK + host.size,), int(np.uint16(ar.SENTINEL16).view(np.int16)), dtype=torch.int16, device=dev)
    view = whole[shift:shift + host.size]
    view.copy_(torch.from_numpy(host.view(np.int16).copy()))
    assert whole.data_ptr() % 16 == 0 and view.data_ptr() == whole.data_ptr() + 2 * shift
    return whole, view


def bits(t):
    return t.cpu().numpy().view(np.uint16)


def run(capi, dev, c):
    y, gy = ar.operands(c)
    ly, lgy, lout = ar.layouts(c)
    yh, gh = host_buffer(capi, ly, y), host_buffer(capi, lgy, gy)
    y_all, yv = on_device(yh, c.shifts[0], dev)
    g_all, gv = on_device(gh, c.shifts[1], dev)
    if c.inplace:
        oh, o_all, ov = gh, g_all, gv
    else:
        oh = host_buffer(capi, lout)
        o_all, ov = on_device(oh, c.shifts[2], dev)
    capi.check(capi.lib.rtpose_relu_grad_bf16(capi.ptr(yv), C.byref(cd.L(capi, ly)), capi.ptr(gv), C.byref(cd.L(capi, lgy)),
                                              capi.ptr(ov), C.byref(cd.L(capi, lout)), c.channels, ar.N, ar.H, ar.W,
                                              capi.current_stream()), "rtpose_relu_grad_bf16")
    torch.cuda.synchronize()
    want = np.transpose(ar.relu_grad_bf16_bits(y, gy), (0, 2, 3, 1))
    io = lr.index(lout, ar.N, ar.H, ar.W, c.channels)
    got_all = bits(o_all)
    got = got_all[c.shifts[1 if c.inplace else 2]:][:oh.size]
    assert np.array_equal(got[io], want), "%d of %d elements differ" % (int((got[io] != want).sum()), want.size)
    # nothing but the valid pixels of out's slice changed: gaps, neighbouring channels, the slack around the view
    expect = np.full(got_all.size, ar.SENTINEL16, dtype=np.uint16)
    body = oh.copy()
    body[io] = want
    expect[c.shifts[1 if c.inplace else 2]:][:oh.size] = body
    assert np.array_equal(got_all, expect), "written outside the valid pixels of the slice"
    # the operands are as they were
    y_expect = np.full(y_all.numel(), ar.SENTINEL16, dtype=np.uint16)
    y_expect[c.shifts[0]:][:yh.size] = yh
    assert np.array_equal(bits(y_all), y_expect), "y was modified"
    if not c.inplace:
        g_expect = np.full(g_all.numel(), ar.SENTINEL16, dtype=np.uint16)
        g_expect[c.shifts[1]:][:gh.size] = gh
        assert np.array_equal(bits(g_all), g_expect), "gy was modified"


@pytest.mark.parametrize("choff", ar.CHOFFS)
@pytest.mark.parametrize("channels", ar.CHANNELS)
def test_bits_and_untouched_surroundings(capi, cuda, channels, choff):
    grid = ar.cases(channels, choff)
    assert len(grid) == 18 and {c.inplace for c in grid} == {False, True}
    if choff % 8 == 0:
        assert {ar.is_vector(c) for c in grid} == {False, True}
    for c in grid:
        run(capi, cuda, c)


def test_several_workgroups_and_channel_tiles(capi, cuda):
    """more than 64 pixels (two workgroups, the second partial) on the grid above; here more than 64 units of 8 channels: a
    second channel tile, its last unit partial"""
    n, h, w, ch, cs = 1, 3, 5, 64 * 8 + 11, 64 * 8 + 16
    g = np.random.default_rng(5)
    y = g.integers(0, 1 << 16, size=(n, ch, h, w), dtype=np.uint32).astype(np.uint16)
    gy = g.integers(0, 1 << 16, size=(n, ch, h, w), dtype=np.uint32).astype(np.uint16)
    ly, lg = lr.padded(cs, h, w, 1), lr.padded(cs, h, w, 3)
    size = lambda lay: cd.npx(capi, lay, n, h, w) * lay.cstride     # noqa: E731
    yb = torch.from_numpy(lr.scatter(np.zeros(size(ly), dtype=np.uint16), ly, y).view(np.int16).copy()).to(cuda)
    gh = lr.scatter(np.zeros(size(lg), dtype=np.uint16), lg, gy)
    gb = torch.from_numpy(gh.view(np.int16).copy()).to(cuda)
    capi.check(capi.lib.rtpose_relu_grad_bf16(capi.ptr(yb), C.byref(cd.L(capi, ly)), capi.ptr(gb), C.byref(cd.L(capi, lg)),
                                              capi.ptr(gb), C.byref(cd.L(capi, lg)), ch, n, h, w, capi.current_stream()),
               "rtpose_relu_grad_bf16")
    torch.cuda.synchronize()
    want = lr.scatter(np.zeros(size(lg), dtype=np.uint16), lg, ar.relu_grad_bf16_bits(y, gy))
    assert np.array_equal(bits(gb), want)       # zero gaps and pad channels stayed zero: the buffer is still convolvable
