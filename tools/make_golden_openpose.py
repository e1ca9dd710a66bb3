"""Generates tests/golden/openpose_small.npz from the REFERENCE OpenPose_Model itself.

Needs a checkout of the reference project (the directory that holds its lib/network/openpose.py):
    python tools/make_golden_openpose.py REFERENCE_ROOT
Imports lib.network.openpose.OpenPose_Model from the reference unmodified (torch-only imports), loads the seeded
state_dict of tests/openpose_restate.py into it for (4, 2, 38, 19) and (4, 2, 14, 9), runs a seeded 1x3x48x56 input on
the CPU and stores the input, every saved_for_loss tensor, the seed and the state_dict key names and shapes.  The
weights are not stored: the tests regenerate them from the seed.  Before writing anything it asserts that the CPU
restatement (openpose_restate.forward) reproduces the reference module to 1e-6.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import openpose_restate as R  # noqa: E402

CONFIGS = ((4, 2, 38, 19), (4, 2, 14, 9))
SEED = 2024
INPUT_SEED = 1234


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/make_golden_openpose.py REFERENCE_ROOT")
    ref_root = sys.argv[1]
    sys.path.insert(0, ref_root)
    from lib.network.openpose import OpenPose_Model  # reference code, imported not copied
    x = np.random.Generator(np.random.PCG64(INPUT_SEED)).uniform(-0.5, 0.5, (1, 3, 48, 56)).astype(np.float32)
    out = {"x": x, "seed": np.int64(SEED)}
    for cfg in CONFIGS:
        tag = "c%d_%d_%d_%d" % cfg
        ref = OpenPose_Model(*cfg)
        spec = R.state_dict_spec(*cfg)
        got = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        assert got == [(k, tuple(s)) for k, s in spec], "state_dict layout of the reference differs from the spec"
        sd = R.seeded_state_dict(spec, SEED)
        ref.load_state_dict(sd)
        ref.eval()
        with torch.no_grad():
            _, (paf_ret, heat_ret) = ref(torch.from_numpy(x))
            paf_o, heat_o = R.forward(sd, torch.from_numpy(x), cfg[0], cfg[1])
        worst = max((a - b).abs().max().item() for a, b in zip(paf_ret + heat_ret, paf_o + heat_o))
        assert worst <= 1e-6, "restatement differs from the reference module by %g" % worst
        for i, t in enumerate(paf_ret + heat_ret):
            out["%s_out%d" % (tag, i)] = t.numpy()
        out["%s_keys" % tag] = np.array([k for k, _ in got])
        out["%s_shapes" % tag] = np.array(["x".join(map(str, s)) for _, s in got])
        print("%s: restatement max|diff| %g, maps max|value| %s" %
              (tag, worst, ", ".join("%.3f" % t.abs().max().item() for t in paf_ret + heat_ret)))
    path = os.path.join(ROOT, "tests", "golden", "openpose_small.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
