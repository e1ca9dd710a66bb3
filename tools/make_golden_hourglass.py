"""Generates tests/golden/hourglass_small.npz from the REFERENCE stacked hourglass itself.

Needs a checkout of the reference project (the directory that holds its lib/network/rtpose_hourglass.py):
    python tools/make_golden_hourglass.py REFERENCE_ROOT
Imports lib/network/rtpose_hourglass.py from the reference unmodified (it imports only torch), loads the seeded
state_dict of tests/hourglass_restate.py into hg(num_stacks, num_blocks, 38, 19) for every configuration below, runs a
seeded 1 x 3 x 64 x 128 input on the CPU in eval mode and stores the input, the seeds, the last stack's two maps and the
state_dict key names and shapes.  The weights are not stored: the tests regenerate them from the seed.  Before writing
anything it asserts that the CPU restatement (hourglass_restate.forward) reproduces the reference module to fp32
rounding and that every map lies in the 0.1 .. 100 range the parity tests call sane.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hourglass_restate as R  # noqa: E402

# (num_stacks, num_blocks, gain of the residual branches)
CONFIGS = ((8, 1, R.BRANCH_GAIN), (2, 1, R.BRANCH_GAIN), (2, 2, R.BRANCH_GAIN), (1, 1, R.STRONG_GAIN))
PAF, HEAT = 38, 19
SEED = 2025
INPUT_SEED = 4321
SHAPE = (1, 3, 64, 128)


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/make_golden_hourglass.py REFERENCE_ROOT")
    path = os.path.join(sys.argv[1], "lib", "network", "rtpose_hourglass.py")
    spec_ = importlib.util.spec_from_file_location("reference_rtpose_hourglass", path)
    ref_mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(ref_mod)  # reference code, imported not copied
    x = np.random.Generator(np.random.PCG64(INPUT_SEED)).uniform(-0.5, 0.5, SHAPE).astype(np.float32)
    out = {"x": x, "seed": np.int64(SEED), "input_seed": np.int64(INPUT_SEED)}
    for stacks, blocks, gain in CONFIGS:
        tag = "s%d_b%d" % (stacks, blocks)
        ref = ref_mod.hg(num_stacks=stacks, num_blocks=blocks, paf_classes=PAF, ht_classes=HEAT)
        spec = R.state_dict_spec(stacks, blocks, PAF, HEAT)
        got = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        assert got == [(k, tuple(s)) for k, s in spec], "state_dict layout of the reference differs from the spec"
        sd = R.seeded_state_dict(spec, SEED, gain)
        ref.load_state_dict(sd)
        ref.eval()
        with torch.no_grad():
            (paf, heat), _ = ref(torch.from_numpy(x))
            paf_o, heat_o = R.forward(sd, torch.from_numpy(x), stacks, blocks)
        scale = max(1.0, paf.abs().max().item(), heat.abs().max().item())
        worst = max((paf - paf_o).abs().max().item(), (heat - heat_o).abs().max().item())
        assert worst <= 2e-6 * scale, "restatement differs from the reference module by %g (scale %g)" % (worst, scale)
        for t in (paf, heat):
            assert 0.1 <= t.abs().max().item() <= 100.0, "map range %g outside 0.1 .. 100" % t.abs().max().item()
        out[tag + "_paf"], out[tag + "_heat"] = paf.numpy(), heat.numpy()
        out[tag + "_gain"] = np.float64(gain)
        out[tag + "_keys"] = np.array([k for k, _ in got])
        out[tag + "_shapes"] = np.array(["x".join(map(str, s)) for _, s in got])
        print("%s gain %g: restatement max|diff| %g, maps max|value| paf %.3f heat %.3f" %
              (tag, gain, worst, paf.abs().max().item(), heat.abs().max().item()))
    dst = os.path.join(ROOT, "tests", "golden", "hourglass_small.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%d bytes)" % (dst, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
