"""train.py launches what it launched when tests/golden/train_launch_trace.json was recorded: per case of
tests/train_trace.py the same library calls in the same order with the same geometry, and - where the fixture holds
digests - the same bits in y and in every gradient.  The fixture is regenerated (tools/make_golden_train_trace.py) only
when a change of the launch sequence is intended; what it pins and what it leaves free is in tests/train_trace.py."""
import importlib
import os

import pytest

import train_trace as tt

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_launch_trace.json")


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def golden():
    return tt.load(GOLD)


def first_difference(want, got):
    at = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
    return "%d calls recorded, %d now; first difference at call %d:\n  recorded %s\n  now      %s" % (
        len(want), len(got), at, want[at] if at < len(want) else "(none)", got[at] if at < len(got) else "(none)")


@pytest.mark.parametrize("name", list(tt.CASES))
def test_launch_sequence_is_the_recorded_one(cuda, train, golden, name):
    want = golden[name]
    trace, digests = tt.run_case(train, cuda, name)
    assert train.lib is importlib.import_module(tt.PKG + "._capi").lib
    if "trace" in want:
        assert trace == want["trace"], first_difference(want["trace"], trace)
    else:
        assert (len(trace), tt.histogram(trace)) == (want["calls"], want["histogram"])
    have = tt.stored(name, trace)
    if "tensors" in want:
        assert digests is not None
        have = tt.with_tensors(have, digests)
        assert have["tensors"] == want["tensors"]
        assert have["tensors_sha256"] == want["tensors_sha256"], "y or a gradient has other bits than recorded; now %s" % digests
    assert have == want
