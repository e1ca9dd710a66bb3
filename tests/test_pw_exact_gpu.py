"""The five ShuffleNetV2 pointwise-chain launches (csrc/pw_fused.hip, pw_fused_bf16.hip, pw_head.hip, pw_head_bf16.hip,
unit_bf16.hip) against tests/pw_restate.py, BIT FOR BIT, on every case of pr.EXACT_CASES: integer operands make every
fp32 sum exact in any order and every bf16 rounding the rounding of an exact value (tests/test_pw_restate_cpu.py asserts
the conditions), so one differing bit is a wrong term, a dropped or doubled pixel, a stale halo or a wrong channel.

Per case, through tests/pw_driver.py (host-built inputs, sentinel-filled outputs, host-read bits):
  * the output == the float64 restatement (rounded by lr.bf16_rne where it is stored as bf16), every written word finite,
    every other word of the buffer untouched;
  * a second launch gives the same bits;
  * image 0 launched alone gives the bits it has in the batch;
  * the input as a slice of a wider pixel with decoys around it gives the same bits as the compact input.
The walk cases are sized from the device's CU count so that the work items exceed the launcher's grid cap by 1.5 x with a
ragged last round; their whole output is compared."""
import ctypes as C

import numpy as np
import pytest
import torch

import pw_driver as pd
import pw_restate as pr

pytestmark = pytest.mark.gpu


def _exact(capi, cuda, case):
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    c = pr.sized(case, cus)
    o = pr.exact_operands(c)
    if c.walk is not None:      # (sized here: the conditions of the other cases are asserted on the CPU)
        S, rounded, share = pr.exact_bounds(c, o)
        assert S < 2 ** 24 and rounded <= 256 and share >= 0.40
        cap, items = pr.walk_cap(c, cus), pr.work_items(c, c.n)
        assert items >= 1.5 * cap and items % cap != 0
    P = pd.prepare(capi, cuda, c, o, "compact")
    bits = pd.launch(P)
    pd.check(P, bits)
    assert np.array_equal(pd.launch(P), bits), "a second launch gave other bits"
    if c.n > 1:
        one = pd.launch(P, 1)
        pd.check(P, one, images=1)
        for a, b in zip(pd.written_bits(P, one, 1), pd.written_bits(P, bits, 1)):
            assert np.array_equal(a, b), "image 0 alone differs from image 0 of the batch"
    Q = pd.prepare(capi, cuda, c, o, "slice")
    sbits = pd.launch(Q)
    pd.check(Q, sbits)
    for a, b in zip(pd.written_bits(Q, sbits), pd.written_bits(P, bits)):
        assert np.array_equal(a, b), "the slice input and the compact input give different bits"


@pytest.mark.parametrize("case", pr.EXACT_CASES["pw_fused"], ids=lambda c: c.tag)
def test_pw_fused_exact(capi, cuda, case):
    _exact(capi, cuda, case)


@pytest.mark.parametrize("case", pr.EXACT_CASES["pw_fused_bf16"], ids=lambda c: c.tag)
def test_pw_fused_bf16_exact(capi, cuda, case):
    _exact(capi, cuda, case)


@pytest.mark.parametrize("case", pr.EXACT_CASES["pw_head"], ids=lambda c: c.tag)
def test_pw_head_exact(capi, cuda, case):
    _exact(capi, cuda, case)


@pytest.mark.parametrize("case", pr.EXACT_CASES["pw_head_bf16"], ids=lambda c: c.tag)
def test_pw_head_bf16_exact(capi, cuda, case):
    _exact(capi, cuda, case)


@pytest.mark.parametrize("case", pr.EXACT_CASES["unit_bf16"], ids=lambda c: c.tag)
def test_unit_bf16_exact(capi, cuda, case):
    _exact(capi, cuda, case)


def test_pw_head_refuses_a_16_channel_input(capi, cuda):
    """rtpose_pw_head has no instance below 32 input channels (one whole 32-channel chunk; rtpose_pw_head_fits): the shape
    is refused before any launch and nothing is written; rtpose_pw_head_bf16 takes 16 (its cin16 case above)"""
    case = next(c for c in pr.EXACT_CASES["pw_head"] if c.tag == "cin32")
    P = pd.prepare(capi, cuda, case, pr.exact_operands(case), "compact")
    d1, d2 = P.d
    d1.cin = 16
    out = pd.fresh(P)
    d2.out = out.data_ptr()
    assert capi.lib.rtpose_pw_head_fits(C.byref(d1), C.byref(d2)) == 0
    assert capi.lib.rtpose_pw_head(C.byref(d1), C.byref(d2), case.n, case.h, case.w, capi.current_stream()) != 0
    torch.cuda.synchronize()
    assert np.all(pd.host_bits(out) == pd.SENTINEL["f32"])


@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("variant", ["bias", "no_bias", "cin_map"])
def test_both_fp32_packer_doors_pack_the_same_bytes(capi, cuda, K, variant):
    """rtpose_pack_pw_weights and rtpose_pack_pw_weights_cols(col_map = NULL, ncols = cout) are one packer behind two doors:
    into sentinel-filled buffers both write byte-identical packed weights and biases, which are pr.pack_pw's - the three
    columns from col_off and nothing else.  cin_map holds a negative entry (a zero K row) and an entry past cin_src."""
    lib, stream = capi.lib, capi.current_stream()
    cout, coutp, col_off, cin_src = 3, 64, 5, 6
    rng = np.random.default_rng(K)
    w = rng.standard_normal((cout, cin_src)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if variant != "no_bias" else None
    cmap = None
    if variant == "cin_map":
        cmap = rng.integers(0, cin_src, K).astype(np.int32)
        cmap[1], cmap[K - 2] = -1, cin_src
    assert lib.rtpose_packed_pw_floats(K, coutp) == K * coutp
    wd, bd, md = pd.f32(cuda, w), None if b is None else pd.f32(cuda, b), None if cmap is None else pd.i32(cuda, cmap)
    got = []
    for door in ("plain", "cols"):
        wp, bp = pd.sentinel_buffer(K * coutp, "f32", cuda), pd.sentinel_buffer(coutp, "f32", cuda)
        if door == "plain":
            capi.check(lib.rtpose_pack_pw_weights(capi.ptr(wd), capi.ptr(bd), cout, cin_src, capi.ptr(md), K, coutp, col_off,
                                                  capi.ptr(wp), capi.ptr(bp), stream))
        else:
            capi.check(lib.rtpose_pack_pw_weights_cols(capi.ptr(wd), capi.ptr(bd), cout, cin_src, capi.ptr(md), K, cout, None,
                                                       coutp, col_off, capi.ptr(wp), capi.ptr(bp), stream))
        torch.cuda.synchronize()
        got.append((pd.host_bits(wp), pd.host_bits(bp)))
    sent_w = np.full(K * coutp, pd.SENTINEL["f32"], np.uint32).view(np.float32)
    sent_b = np.full(coutp, pd.SENTINEL["f32"], np.uint32).view(np.float32)
    want_w, want_b = pr.pack_pw(w, b, K, coutp, col_off, cin_map=cmap, wp=sent_w, bp=sent_b)
    for gw, gb in got:
        assert np.array_equal(gw, want_w.view(np.uint32)) and np.array_equal(gb, want_b.view(np.uint32))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
