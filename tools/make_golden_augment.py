"""Generates tests/golden/augment_ref.npz from the reference's OWN loader code (needs the reference tree and Pillow).

    python tools/make_golden_augment.py [--out PATH]

Loads lib/datasets/{transforms,utils,datasets}.py of the reference tree (RTPOSE_REFERENCE) the
way tools/make_golden_encode.py loads datasets.py - absent third-party modules (cv2, torchvision, ...) as permissive
empty shells - and runs, per case, the preprocess chain of train/train_VGG19.py:124-130

    Compose([Normalize(), RandomApply(HFlip(), p), RescaleRelative(scale_range), Crop(S), CenterPad(S)])

and then ``CocoKeypoints.single_image_processing`` (image_transform, utils.mask_valid_area, get_ground_truth with
input_x = input_y = S, stride 8) unbound on a namespace object.  Two things the shells cannot give are restated here,
and the fixture's ``meta`` says so: ``torchvision.transforms.functional.pad`` is three lines of PIL (a new image of the
fill colour, the old one pasted at (left, top)), and ``image_transform`` (ToTensor + Normalize) is its torch
restatement ``uint8 -> float32 -> .div(255) -> .sub_(mean).div_(std)`` with float32 mean / std.

Sources are synthetic (smooth plus noise, with patches that saturate to 0 and 255: tests/augment_restate.py), the
annotations synthetic COCO-17 people.  Cases:
  s<seed>_<k>  seeds 0..3: the four sources one after another under one torch.manual_seed(seed), scale_range (0.5, 1.0),
               flip probability 0.5; canvas 48 for the even seeds, 40 for the odd ones
  t_*          targeted: a float scale_range, the flip forced by the probability (1.0 / 0.0) and Crop's torch.randint
               scripted (the value the clamp then sees), see TARGETED below
Per case <c>: src_<c> the name of its source, par_<c> = (hflip, hr, wr, crop_x, crop_y, S), factor_<c> the float64 factor,
canvas_<c> the final uint8 canvas, image_<c> the normalised and masked float32 tensor, kp_<c> [K, 17, 3] the augmented
keypoints in the reference's dtype, bbox_<c>, the meta entries offset_<c> / scale_<c> / valid_area_<c> /
width_height_<c>, heat_<c> / paf_<c> the targets of get_ground_truth as float32 with heat_zero_<c> / paf_zero_<c> the
float64 zero pattern (np.packbits of == 0).  The file is written with fixed zip timestamps: a second run reproduces it
byte for byte.
"""
import json
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import augment_restate as R                                           # noqa: E402  (the synthetic sources)
from make_golden_encode import REF, load_reference, write_npz         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "augment_ref.npz")
SOURCES = {"A": (97, 131), "B": (64, 48), "C": (37, 200), "D": (40, 40)}          # (h0, w0)
SEEDS = (0, 1, 2, 3)
# name: (source, factor, flip, canvas, scripted randint values in draw order)
TARGETED = {
    "t_half_flip": ("A", 0.5, True, 48, [40]),            # 65 x 48 -> crop x at its maximum 17 (clamped), y untouched, 9 taps
    "t_copy_crop": ("A", 1.0, False, 48, [30, 20]),       # no resize at all, an interior crop on both axes
    "t_pad_odd": ("B", 0.618, True, 48, []),              # 29 x 39: pad on both axes with odd remainders 19 and 9
    "t_crop_pad": ("C", 0.75, False, 40, [-5]),           # 150 x 27: crop x at 0 (clamped), pad y by 6 / 7
    "t_quarter": ("B", 0.25, False, 40, []),              # 12 x 16, 17 taps (exactly 0.25): pad both
}


def pil_pad(image, ltrb, fill):
    """torchvision.transforms.functional.pad(image, (left, top, right, bottom), fill=...) for a PIL image, constant
    mode."""
    from PIL import Image
    out = Image.new(image.mode, (image.size[0] + ltrb[0] + ltrb[2], image.size[1] + ltrb[1] + ltrb[3]), tuple(fill))
    out.paste(image, (ltrb[0], ltrb[1]))
    return out


def image_transform(image):
    """ToTensor + Normalize(mean, std) of torchvision, restated in torch."""
    a = torch.from_numpy(np.array(image, dtype=np.uint8)).permute(2, 0, 1).contiguous()
    t = a.to(torch.float32).div(255)
    mean = torch.as_tensor([0.485, 0.456, 0.406], dtype=torch.float32)[:, None, None]
    std = torch.as_tensor([0.229, 0.224, 0.225], dtype=torch.float32)[:, None, None]
    return t.sub_(mean).div_(std)


class ScriptedTorch:
    """torch as transforms.py sees it, with randint answering from a script (Crop's two draws)."""

    def __init__(self, script):
        self.script = list(script)

    def __getattr__(self, name):
        return getattr(torch, name)

    def randint(self, low, high, size):
        v = self.script.pop(0)
        assert low <= v < high, "scripted draw %d outside [%d, %d)" % (v, low, high)
        return torch.tensor([v])


def people(h0, w0, seed):
    """Two synthetic COCO-17 people inside (and slightly outside) an h0 x w0 image."""
    rng = np.random.default_rng(seed)
    anns = []
    for k in range(2):
        cx, cy = rng.uniform(0.25, 0.75) * w0, rng.uniform(0.3, 0.7) * h0
        pts = np.stack([cx + rng.normal(0, 0.22 * w0, 17), cy + rng.normal(0, 0.25 * h0, 17)], 1)
        kp = np.concatenate([np.round(pts, 1), rng.choice([0.0, 1.0, 2.0, 2.0], 17)[:, None]], 1)
        kp[5, 2] = kp[6, 2] = 2.0 if k == 0 else 1.0                  # the neck's two visibility rules
        x0, y0 = pts.min(0)
        x1, y1 = pts.max(0)
        anns.append({"keypoints": kp.reshape(-1).tolist(), "bbox": [float(x0), float(y0), float(x1 - x0), float(y1 - y0)],
                     "segmentation": []})
    return anns


def main():
    from PIL import Image
    import PIL
    if not os.path.isdir(REF):
        raise SystemExit("%s not present: this script only runs where the reference tree is" % REF)
    how, stubbed, ds, _ = load_reference()
    tr, utils = ds.transforms, ds.utils
    sys.modules["torchvision"].transforms.functional.pad = pil_pad
    real_torch = tr.torch
    cls = ds.CocoKeypoints
    sources = {n: R.synthetic_source(h, w, 100 + i) for i, (n, (h, w)) in enumerate(sorted(SOURCES.items()))}
    anns_of = {n: people(h, w, 200 + i) for i, (n, (h, w)) in enumerate(sorted(SOURCES.items()))}
    out = {"source_" + n: s for n, s in sources.items()}
    for n, a in anns_of.items():
        out["anns_kp_" + n] = np.array([x["keypoints"] for x in a], np.float64)
        out["anns_bbox_" + n] = np.array([x["bbox"] for x in a], np.float64)
    cases = []

    def run(case, src, scale_range, flip_p, canvas, script=None):
        seen = {}
        rescale = tr.RescaleRelative(scale_range)
        inner = rescale.scale

        def scale(image, anns, factor):
            seen["factor"] = factor
            res = inner(image, anns, factor)
            seen["resized"] = res[0].size
            return res
        rescale.scale = scale
        crop = tr.Crop(canvas)
        inner_crop = crop.crop

        def crop_fn(image, anns):
            res = inner_crop(image, anns)
            seen["ltrb"] = [int(v) for v in res[2]]
            return res
        crop.crop = crop_fn
        chain = tr.Compose([tr.Normalize(), tr.RandomApply(tr.HFlip(), flip_p), rescale, crop, tr.CenterPad(canvas)])
        tr.torch = ScriptedTorch(script) if script is not None else real_torch
        try:
            image, anns, meta = chain(Image.fromarray(sources[src]), anns_of[src], None)
        finally:
            left = tr.torch.script if script is not None else []
            tr.torch = real_torch
        assert not left, "case %s: scripted draws %s were not consumed" % (case, left)
        assert image.size == (canvas, canvas)
        canvas_u8 = np.array(image, dtype=np.uint8)
        self = types.SimpleNamespace(image_transform=image_transform, input_x=canvas, input_y=canvas, stride=8,
                                     HEATMAP_COUNT=len(ds.get_keypoints()), LIMB_IDS=ds.kp_connections(ds.get_keypoints()),
                                     log=logging.getLogger("golden"))
        self.add_neck = lambda k: cls.add_neck(self, k)
        self.remove_illegal_joint = lambda k: cls.remove_illegal_joint(self, k)
        self.get_ground_truth = lambda a: cls.get_ground_truth(self, a)
        meta_for_item = dict(meta)
        tensor, heat, paf = cls.single_image_processing(self, image, anns, meta_for_item, {})
        heat64, paf64 = cls.get_ground_truth(self, anns)
        assert np.array_equal(heat64.transpose(2, 0, 1).astype(np.float32), heat.numpy())
        kp = np.array([a["keypoints"] for a in anns])
        assert all(a["keypoints"].dtype == kp.dtype for a in anns)
        wr, hr = seen["resized"]
        out["src_" + case] = np.array(src)
        out["par_" + case] = np.array([int(meta["hflip"]), hr, wr, seen["ltrb"][0], seen["ltrb"][1], canvas], np.int32)
        out["factor_" + case] = np.array(seen["factor"], np.float64)
        out["canvas_" + case] = canvas_u8
        out["image_" + case] = tensor.numpy()
        out["kp_" + case] = kp
        out["bbox_" + case] = np.array([a["bbox"] for a in anns])
        for key in ("offset", "scale", "valid_area", "width_height"):
            out[key + "_" + case] = np.asarray(meta[key])
        out["heat_" + case] = heat.numpy()
        out["paf_" + case] = paf.numpy()
        out["heat_zero_" + case] = np.packbits(heat64.transpose(2, 0, 1) == 0)
        out["paf_zero_" + case] = np.packbits(paf64.transpose(2, 0, 1) == 0)
        cases.append(case)
        print("%-12s src %s  flip %d  factor %.6f -> %3d x %3d  crop (%d, %d)  canvas %d  kp %s  valid_area %s"
              % (case, src, meta["hflip"], seen["factor"], hr, wr, seen["ltrb"][0], seen["ltrb"][1], canvas, kp.dtype,
                 np.round(meta["valid_area"], 3).tolist()))

    for seed in SEEDS:
        torch.manual_seed(seed)
        for k, src in enumerate(sorted(SOURCES)):
            run("s%d_%d" % (seed, k), src, (0.5, 1.0), 0.5, 48 if seed % 2 == 0 else 40)
    for case, (src, factor, flip, canvas, script) in TARGETED.items():
        run(case, src, factor, 1.0 if flip else 0.0, canvas, script)
    out["meta"] = np.array(json.dumps({
        "how": "transforms.Compose([Normalize, RandomApply(HFlip), RescaleRelative, Crop, CenterPad]) + "
               "CocoKeypoints.single_image_processing, unbound on a namespace object",
        "restated": {"torchvision.transforms.functional.pad": "PIL: Image.new(mode, padded size, fill) + paste at (left, top)",
                     "image_transform (ToTensor + Normalize)": "torch: uint8 -> float32 -> .div(255) -> .sub_(mean).div_(std), "
                                                                "float32 mean / std"},
        "stubbed_modules": stubbed, "cases": cases, "seeds": list(SEEDS), "seeded_sources": sorted(SOURCES),
        "seeded_scale_range": [0.5, 1.0], "seeded_hflip_p": 0.5, "stride": 8, "sigma": 7.0,
        "targeted": {k: {"source": v[0], "factor": v[1], "flip": v[2], "canvas": v[3], "randint": v[4]}
                     for k, v in TARGETED.items()},
        "numpy": np.__version__, "torch": torch.__version__.split("+")[0], "pillow": PIL.__version__}))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv[1:] else OUT
    write_npz(path, out)
    print("wrote %s (%d bytes, %d entries)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
