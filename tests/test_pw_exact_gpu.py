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
