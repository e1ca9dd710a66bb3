"""The recording proxy of tests/train_trace.py without a device: what it writes down of a call, and that it puts the
library back."""
import ctypes as C
import os
import types

import train_trace as tt


def test_the_proxy_records_geometry_and_no_address(capi):
    lay = capi.Layout.padded(8, 3, 4, 1)
    d = capi.ConvDesc()
    d.inp, d.lin, d.cin, d.k = 0x1000, lay, 8, 3
    assert tt._normalise(C.byref(lay)) == [8, 0, 5, 4, 6]
    got = tt._normalise(C.byref(d))
    assert got[:7] == ["ConvDesc", "ptr", "null", "null", "null", [8, 0, 5, 4, 6], [0, 0, 0, 0, 0]] and got[7:11] == [8, 0, 3, 0]
    assert len(got) == 1 + len(capi.ConvDesc._fields_) and "4096" not in tt.canonical(got)
    assert [tt._normalise(a) for a in (None, C.c_void_p(0), C.c_void_p(64), 3, 0.5, True)] == ["null", "null", "ptr", 3, 0.5, 1]
    holder = types.SimpleNamespace(lib=capi.lib)
    with tt.recording(holder) as calls:
        pixels = holder.lib.rtpose_layout_pixels(C.byref(lay), 2, 3, 4)
        rc = holder.lib.rtpose_conv2d_wgrad_bf16(None, 2, 3, 4, None)      # refused on the host: a NULL descriptor
    assert holder.lib is capi.lib and rc == -1
    assert calls == [["rtpose_layout_pixels", [8, 0, 5, 4, 6], 2, 3, 4, pixels], ["rtpose_conv2d_wgrad_bf16", "null", 2, 3, 4]]
    assert tt.histogram(calls) == {"rtpose_layout_pixels": 1, "rtpose_conv2d_wgrad_bf16": 1}


def test_every_case_has_a_way_to_be_stored():
    assert len(tt.CASES) == 154 and all(c.store in ("full", "summary") for c in tt.CASES.values())
    assert sum(1 for n in tt.CASES if n.startswith("conv2d-")) == 4 * 2 * 3 * 4
    assert sum(1 for n in tt.CASES if n.startswith("conv_chain-")) == 2 * 2 * 2 * 5


def test_the_fixture_holds_every_case_and_no_other():
    golden = tt.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_launch_trace.json"))
    assert sorted(golden) == sorted(tt.CASES)
    for name, entry in golden.items():
        assert set(entry) - {"tensors", "tensors_sha256"} == set(tt.stored(name, [])), name
        assert ("tensors" in entry) == (tt.CASES[name].store != "summary"), name
