"""Generates tests/golden/train_launch_trace.json: the library calls of train.py, case by case, recorded on an MI355X.

    python tools/make_golden_train_trace.py [--out PATH]

The fixture pins train.py's launch sequence to the commit it was generated at (DESIGN section 3.3o names it); a rewrite of
train.py is checked against it by tests/test_train_trace_gpu.py and does NOT regenerate it.  Regenerating records the
behaviour of the commit at hand: do that only when a change of the launch sequence is intended, and say so.

Cases, proxy and normal form are tests/train_trace.py's.  Every case runs twice, each time on a cold packing cache
(train.drop_packed_filters()); the two traces must be equal - a trace that is not reproducible ends the run - and no conv
may fall back unless the case plays a refusal.  Where the case has outputs, one sha256 over the sha256 of y and of every gradient
is stored if the two runs agree on all of them; if they do not, the case keeps its trace alone and is printed as a finding.
"""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_trace as tt  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "train_launch_trace.json")


def main():
    train = importlib.import_module(tt.PKG + ".train")
    dev = torch.device("cuda:0")
    out, findings = {}, []
    for name in tt.CASES:
        trace, digests = tt.run_case(train, dev, name)
        fallbacks = dict(train.bf16_fallbacks, chain=train.chain_fallbacks)
        again, digests_again = tt.run_case(train, dev, name)
        if trace != again:
            at = next((i for i, (a, b) in enumerate(zip(trace, again)) if a != b), min(len(trace), len(again)))
            sys.exit("%s: the trace is not reproducible: %d and %d calls, first difference at call %d" % (name, len(trace), len(again), at))
        if not name.startswith("refused-") and any(fallbacks.values()):
            sys.exit("%s: fell back %s" % (name, fallbacks))
        entry = tt.stored(name, trace)
        if digests is not None:
            if digests == digests_again:
                entry = tt.with_tensors(entry, digests)
            else:
                findings.append(name)
                print("FINDING %s: not reproducible between two runs: %s"
                      % (name, sorted(n for n in digests if digests[n] != digests_again.get(n))))
        out[name] = entry
        print("%-72s %4d calls%s" % (name, len(trace), "" if digests is None else "  %d digests" % len(entry.get("tensors", ()))))
    path = GOLD
    if "--out" in sys.argv[1:]:
        path = sys.argv[sys.argv.index("--out") + 1]
    tt.dump(path, out)
    print("wrote %s (%d bytes, %d cases, %d without reproducible digests)" % (path, os.path.getsize(path), len(out), len(findings)))


if __name__ == "__main__":
    main()
