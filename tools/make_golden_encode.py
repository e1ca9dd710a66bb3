"""Generates tests/golden/encode_ref.npz from the reference's OWN target generators (needs the reference tree).

    python tools/make_golden_encode.py [--out PATH]

Loads lib/datasets/datasets.py of the reference tree (RTPOSE_REFERENCE, default /root/reference) with its heatmap.py /
paf.py and calls ``CocoKeypoints.get_ground_truth`` - which calls ``add_neck``, ``remove_illegal_joint``,
``putGaussianMaps`` and ``putVecMaps`` - unbound on a namespace object.  Modules the reference imports but this path
never calls (cv2, torchvision, pycocotools, ...) are registered as permissive empty shells first wherever they are not
installed, in the manner of oracle/ref_harness.py:install.  If datasets.py does not import that way the script stops
with the import error: there is no second way to the targets in it.  The fixture's ``meta`` says how it was made.

Scenes (COCO-17 annotations in, 18-part targets out):
  s0  184 x 184  no people
  s1  184 x 184  one person
  s2  184 x 184  six overlapping people: two share a joint exactly (the heat sum clips at 1), three share a limb's cells
                 (the count reaches 3), one has coincident joints (norm 0), joints at x = 184 and x = -1 (illegal),
                 visibilities 0, 1 and 2
  s3  184 x 184  axis-aligned limbs whose min / stride - 1 and max / stride + 1 land on k + 0.5: half-even rounding
                 decides the box
  s4  368 x 368  four people
Per scene: kp17_<s> [K, 17, 3] the annotations, kp18_<s> [K, 18, 3] what add_neck makes of them (before
remove_illegal_joint), heat_<s> / paf_<s> the float64 targets stored as float32, heat_zero_<s> / paf_zero_<s> the float64
zero pattern (np.packbits of == 0).  The file is written with fixed zip timestamps: a second run reproduces it byte for
byte.
"""
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("RTPOSE_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "encode_ref.npz")

# our part i is COCO-17 keypoint OUR_ORDER[i]; 17 = the neck add_neck appends (datasets.py:241-242)
OUR_ORDER = [0, 17, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3]

# a standing figure in unit coordinates (x right, y down), 18-part order
TEMPLATE = np.array([
    [0.00, -0.80], [0.00, -0.60], [-0.18, -0.58], [-0.26, -0.32], [-0.28, -0.08], [0.18, -0.58], [0.26, -0.32],
    [0.28, -0.08], [-0.11, -0.05], [-0.12, 0.35], [-0.12, 0.75], [0.11, -0.05], [0.12, 0.35], [0.12, 0.75],
    [-0.04, -0.84], [0.04, -0.84], [-0.09, -0.80], [0.09, -0.80]])


class _Shell(types.ModuleType):
    """An absent third-party module: any attribute is another shell, calling one returns a shell."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        m = _Shell(self.__name__ + "." + name)
        setattr(self, name, m)
        return m

    def __call__(self, *a, **k):
        return _Shell(self.__name__ + "()")


def _absent(name):
    try:
        importlib.import_module(name)
        return False
    except Exception:
        return True


def load_reference():
    """-> (how, stubbed module names, the reference's datasets module,
    ground_truth(kp17 [K, 17, 3], input_y, input_x, stride) -> (heat, paf, kp18)).  Stops the script if datasets.py
    does not import under the stubs."""
    stubbed = []
    for name in ("cv2", "torchvision", "pycocotools", "pycocotools.coco", "matplotlib", "matplotlib.pyplot", "scipy.misc"):
        if _absent(name):
            sys.modules[name] = _Shell(name)
            stubbed.append(name)
    pkg = types.ModuleType("refds")                # the package shell: lib/datasets/__init__.py is not run
    pkg.__path__ = [os.path.join(REF, "lib", "datasets")]
    sys.modules["refds"] = pkg
    try:
        ds = importlib.import_module("refds.datasets")
    except Exception as e:
        raise SystemExit("lib/datasets/datasets.py of the reference did not import under the stubs (%s: %s)"
                         % (type(e).__name__, e))
    cls = ds.CocoKeypoints

    def ground_truth(kp17, input_y, input_x, stride):
        self = types.SimpleNamespace(input_y=input_y, input_x=input_x, stride=stride,
                                     HEATMAP_COUNT=len(ds.get_keypoints()),
                                     LIMB_IDS=ds.kp_connections(ds.get_keypoints()))
        self.add_neck = lambda k: cls.add_neck(self, k)
        # (an image without people: np.array([]) is 1-D and the reference's own indexing fails; the shim hands it the
        # empty [0, 18, 3] array it means)
        self.remove_illegal_joint = lambda k: cls.remove_illegal_joint(self, np.asarray(k, np.float64).reshape(-1, 18, 3))
        anns = [{"keypoints": k.reshape(-1).tolist()} for k in kp17]
        heat, paf = cls.get_ground_truth(self, anns)
        kp18 = np.array([cls.add_neck(self, np.array(a["keypoints"]).reshape(17, 3)) for a in anns],
                        np.float64).reshape(-1, 18, 3)
        return heat, paf, kp18
    return "CocoKeypoints.get_ground_truth + add_neck, unbound on a namespace object", stubbed, ds, ground_truth


def to17(p18, v=2.0):
    """18-part (x, y) -> a COCO-17 annotation (x, y, v); the neck is dropped (add_neck derives it from the shoulders)."""
    kp = np.zeros((17, 3), np.float64)
    for i, c in enumerate(OUR_ORDER):
        if c != 17:
            kp[c, :2] = p18[i]
            kp[c, 2] = v
    return kp


def figure(rng, size, cx, scale, quant=None):
    ang = rng.uniform(-0.25, 0.25)
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    pts = (TEMPLATE + rng.normal(0, 0.015, TEMPLATE.shape)) @ rot.T * (scale * size) + [cx * size, 0.55 * size]
    return np.round(pts) if quant else pts


def coco(part):
    return OUR_ORDER[part]


def scenes():
    rng = np.random.default_rng(20240614)
    out = [("s0", 184, np.zeros((0, 17, 3), np.float64))]
    out.append(("s1", 184, np.stack([to17(figure(rng, 184, 0.5, 0.4))])))
    # s2: six overlapping people on integer coordinates
    base = figure(rng, 184, 0.45, 0.42, quant=True)
    ppl = [base.copy() for _ in range(3)]            # 0, 1, 2 share every limb's cells: the count reaches 3
    ppl[1] += [1.0, 0.0]
    ppl[1][0] = ppl[0][0]                            # ... and 0 / 1 share the nose exactly: the sum clips at 1
    ppl[2] += [0.0, 2.0]
    ppl.append(figure(rng, 184, 0.6, 0.38, quant=True))
    ppl.append(figure(rng, 184, 0.3, 0.45, quant=True))
    ppl.append(figure(rng, 184, 0.75, 0.4, quant=True))
    ppl[3][4] = ppl[3][3]                            # RWrist on RElbow: norm 0
    k = [to17(p) for p in ppl]
    k[4][coco(7), 0] = 184.0                         # LWrist at x = input_x: illegal
    k[4][coco(13), 0] = -1.0                         # LAnkle at x = -1: illegal
    k[5][:, 2] = 1.0                                 # visible-but-occluded everywhere (v = 1 > 0.5)
    k[5][coco(10), 2] = 0.0                          # RAnkle not labelled
    k[3][coco(0), 2] = 0.0                           # Nose not labelled
    k[2][coco(2), 2] = 1.0                           # one shoulder v = 1: the neck gets v = 1 * 2
    k[4][coco(5), 2] = 0.0                           # LShoulder not labelled: the neck gets v = 0
    out.append(("s2", 184, np.stack(k)))
    # s3: axis-aligned limbs, stride 8: 12 / 8 - 1 = 0.5 -> 0, 20 / 8 - 1 = 1.5 -> 2, 28 / 8 + 1 = 4.5 -> 4,
    # 36 / 8 + 1 = 5.5 -> 6 (round half up would give 1, 2, 5, 6)
    def stick(pairs):
        p = np.zeros((17, 3), np.float64)
        for part, (x, y) in pairs.items():
            p[coco(part)] = (x, y, 2.0)
        return p
    k = [stick({8: (12, 20), 9: (12, 84), 10: (60, 84)}),            # RHip-RKnee vertical at x = 12, RKnee-RAnkle horizontal
         stick({11: (28, 12), 12: (28, 100), 13: (100, 100)}),       # LHip-LKnee vertical at x = 28, LKnee-LAnkle at y = 100
         stick({2: (36, 20), 3: (116, 20), 4: (116, 108)}),          # RShoulder-RElbow horizontal at y = 20, then vertical
         stick({5: (140, 36), 6: (140, 140), 7: (52, 140)}),         # LShoulder-LElbow vertical at x = 140, then horizontal
         stick({0: (100, 44), 14: (100, 12), 16: (172, 12)})]        # Nose-REye vertical at x = 100, REye-REar at y = 12
    out.append(("s3", 184, np.stack(k)))
    out.append(("s4", 368, np.stack([to17(figure(rng, 368, cx, sc)) for cx, sc in
                                     ((0.2, 0.4), (0.45, 0.33), (0.55, 0.45), (0.8, 0.38))])))
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps (a second run gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    if not os.path.isdir(REF):
        raise SystemExit("%s not present: this script only runs where the reference tree is" % REF)
    mode, stubbed, ds, ground_truth = load_reference()
    out = {}
    names = []
    for name, size, kp17 in scenes():
        heat, paf, kp18 = ground_truth(kp17, size, size, 8)
        assert heat.dtype == np.float64 and paf.dtype == np.float64
        out["kp17_" + name] = kp17
        out["kp18_" + name] = kp18
        out["heat_" + name] = heat.astype(np.float32)
        out["paf_" + name] = paf.astype(np.float32)
        out["heat_zero_" + name] = np.packbits(heat == 0)
        out["paf_zero_" + name] = np.packbits(paf == 0)
        names.append(name)
        print("%s  %3d x %3d  %d people  heat max %.6f (cells at 1: %d)  paf cells != 0: %d" % (
            name, size, size, len(kp17), heat[:, :, :18].max() if heat.size else 0.0, int((heat[:, :, :18] == 1.0).sum()),
            int((paf != 0).sum())))
    out["kp_connections"] = np.array(ds.kp_connections(ds.get_keypoints()), np.int32)
    out["keypoint_names"] = np.array(ds.get_keypoints())
    out["meta"] = np.array(json.dumps({
        "how": mode, "stubbed_modules": stubbed, "scenes": names, "stride": 8, "sigma": 7.0, "numpy": np.__version__,
        "sizes": {n: s for n, s, _ in scenes()}}))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv[1:] else OUT
    write_npz(path, out)
    print(mode)
    print("wrote %s (%d bytes, %d entries)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
