"""Generates tests/golden/color_jitter.npz with Pillow itself (needs Pillow; no reference tree, no torchvision).

    python tools/make_golden_jitter.py [--out PATH]

``image_transform_train`` of the reference (lib/datasets/transforms.py:53-65) is torchvision's ColorJitter,
RandomApply([jpeg]), RandomGrayscale, ToTensor, Normalize.  torchvision is not installed where this was written and the
reference pins no version of it, so what its PIL back end does per operation is restated here in PIL's own calls, and
the fixture's ``meta`` says so:

  adjust_brightness   ImageEnhance.Brightness(img).enhance(f)
  adjust_contrast     ImageEnhance.Contrast(img).enhance(f)
  adjust_saturation   ImageEnhance.Color(img).enhance(f)
  adjust_hue          h, s, v = img.convert('HSV').split(); h += uint8(f * 255) modulo 256;
                      Image.merge('HSV', (h, s, v)).convert('RGB')
  rgb_to_grayscale    img.convert('L') copied to three channels (num_output_channels=3)
  ToTensor, Normalize uint8 -> float32 -> .div(255) -> .sub_(mean).div_(std), float32 mean / std (as
                      tools/make_golden_augment.py restates them)

and utils.mask_valid_area as four integers: everything outside [x0, x1) x [y0, y1) is 0.  The JPEG step is left out
(it is not built).  Per case <c>: canvas_<c> the uint8 [h, w, 3] input, order_<c> (four operations, -1 = none),
factor_<c> the float64 brightness / contrast / saturation factors, hue_<c> the float64 hue factor, gray_<c>, mask_<c>,
u8_<c> the uint8 result before ToTensor, image_<c> the normalised and masked float32 [3, h, w] tensor.  The file is
written with fixed zip timestamps: a second run reproduces it byte for byte.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import augment_restate as R                                           # noqa: E402  (the synthetic sources)
from make_golden_augment import image_transform                       # noqa: E402
from make_golden_encode import write_npz                              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "color_jitter.npz")
FILL = (124, 116, 104)
# name: (h, w, source seed, order, (brightness, contrast, saturation), hue factor, gray, mask (x0, y0, x1, y1), pad columns)
CASES = {
    "drawn_a": (48, 48, 1, (3, 1, 0, 2), (1.0792889595031738, 0.9911255836486816, 1.0264612436294556),
                -0.030221307650208473, 0, (0, 0, 48, 48), 0),
    "drawn_b": (40, 40, 2, (0, 1, 2, 3), (0.932205855846405, 0.9564536809921265, 1.036321759223938),
                0.0830387994647026, 0, (3, 0, 37, 40), 3),
    "contrast_first": (37, 45, 3, (1, 3, 2, 0), (0.9, 1.1, 0.9), 0.1, 0, (0, 5, 45, 31), 0),
    "hue_zero": (24, 31, 4, (3, -1, -1, -1), (1.0, 1.0, 1.0), 0.0, 0, (0, 0, 31, 24), 0),
    "gray": (33, 29, 5, (2, 0, 3, 1), (1.1, 0.9, 1.1), -0.1, 1, (2, 1, 29, 30), 2),
    "wide_factors": (16, 48, 6, (0, 2, 1, -1), (1.5, 2.0, 0.0), 0.0, 0, (0, 0, 48, 16), 0),
}


def apply_ops(img, order, factor, hue_factor, gray):
    from PIL import Image, ImageEnhance
    for op in order:
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(factor[0])
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(factor[1])
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(factor[2])
        elif op == 3:
            h, s, v = img.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.array(int(hue_factor * 255)).astype(np.uint8)
            img = Image.merge("HSV", (Image.fromarray(np_h), s, v)).convert("RGB")
    if gray:
        lum = np.array(img.convert("L"), dtype=np.uint8)
        img = Image.fromarray(np.dstack([lum, lum, lum]))
    return img


def main():
    import PIL
    from PIL import Image
    out = OUT
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    arrays = {}
    for name, (h, w, seed, order, factor, hue_factor, gray, mask, pad) in CASES.items():
        canvas = R.synthetic_source(h, w, 200 + seed)
        if pad:                                     # CenterPad's fill beside the picture, as the canvas has it
            canvas[:, :pad] = FILL
            canvas[:, w - pad:] = FILL
        res = apply_ops(Image.fromarray(canvas), order, factor, hue_factor, gray)
        t = image_transform(res)
        keep = torch.zeros(t.shape[1:], dtype=torch.bool)
        keep[mask[1]:mask[3], mask[0]:mask[2]] = True
        t[:, ~keep] = 0
        arrays["canvas_" + name] = canvas
        arrays["order_" + name] = np.array(order, np.int32)
        arrays["factor_" + name] = np.array(factor, np.float64)
        arrays["hue_" + name] = np.array(hue_factor, np.float64)
        arrays["gray_" + name] = np.array(gray, np.int32)
        arrays["mask_" + name] = np.array(mask, np.int32)
        arrays["u8_" + name] = np.array(res, dtype=np.uint8)
        arrays["image_" + name] = t.numpy()
    meta = {"cases": list(CASES), "pillow": PIL.__version__, "numpy": np.__version__, "torch": torch.__version__,
            "torchvision": "not installed; the reference pins no version.  Its PIL back end is restated per operation in "
                           "PIL's own calls (ImageEnhance, convert, merge), ToTensor as uint8 -> float32 -> div(255)",
            "jpeg": "RandomApply([jpeg], p=0.1) is not part of the fixture: the re-compression is not built"}
    arrays["meta"] = np.array(json.dumps(meta))
    write_npz(out, arrays)
    print("wrote %s (%d bytes, %d cases, Pillow %s)" % (out, os.path.getsize(out), len(CASES), PIL.__version__))


if __name__ == "__main__":
    main()
