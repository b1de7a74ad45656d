#!/usr/bin/env python
"""Write tests/golden/video_prep.npz: the motion boxes and padded crops the REFERENCE's own `find_cluster`, `crop_image` and `padding_square`
(Data_loaders/Image_preprocess.py) produce on the synthetic clips of tests/video_prep_common.py.

Image_preprocess.py runs `resave_data()` when it is imported, so it cannot be imported whole: the module is parsed with `ast` and only the three
function definitions are executed, in a namespace that holds numpy, a `cv2` stand-in whose `copyMakeBorder` is a constant `np.pad`, and nothing
else.  `crop_image` takes a `LoadFlow`; a stand-in with `len_flows` and `__getitem__` serves the synthetic frames.  The crop itself
(`image[h_min:h_max, w_min:w_max]`, Image_preprocess.py:263-265) is repeated here.

The fixture holds, per case: the case's parameters, the reference's box, and the shape and a SHA-256 digest of each padded array.  Frames are
regenerated from closed formulas by the tests; no program text of the reference is stored.

    python tools/make_video_prep_golden.py --reference /path/to/reference
"""
import argparse
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WANTED = ("find_cluster", "crop_image", "padding_square")


class Cv2StandIn:
    BORDER_CONSTANT = 0

    @staticmethod
    def copyMakeBorder(image, top, bottom, left, right, border_type, value):
        assert border_type == Cv2StandIn.BORDER_CONSTANT and len(set(value)) == 1
        pad = ((top, bottom), (left, right)) + ((0, 0),) * (image.ndim - 2)
        return np.pad(image, pad, mode="constant", constant_values=value[0])


class LoadFlowStandIn:
    def __init__(self, image, flow_x, flow_y):
        self.image, self.flow_x, self.flow_y = image, flow_x, flow_y
        self.len_flows = flow_x.shape[0]

    def __getitem__(self, item):
        return self.flow_x[item], self.flow_y[item], self.image[item]

    def __len__(self):
        return self.len_flows


def reference_functions(reference):
    path = os.path.join(reference, "Data_loaders", "Image_preprocess.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED), [d.name for d in defs]
    ns = {"np": np, "cv2": Cv2StandIn}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "video_prep.npz"))
    a = ap.parse_args()
    import video_prep_common as V
    ref = reference_functions(a.reference)
    out = {"cases": np.array(json.dumps(V.CASES))}
    for i, c in enumerate(V.CASES):
        image, fx, fy = V.case_frames(c)
        w0, w1, h0, h1 = (int(v) for v in ref["crop_image"](LoadFlowStandIn(image, fx, fy)))
        ok = int(not ((w1 - w0) < 50 or (h1 - h0) < 50))                       # Image_preprocess.py:257
        out["box%d" % i] = np.array([w0, w1, h0, h1, ok], dtype=np.int32)
        shapes, digests = [], []
        if w1 > w0 and h1 > h0:                                                # an empty crop has nothing to pad
            for plane in (image[0], fx[0], fy[0], image[-1]):
                padded = ref["padding_square"](plane[h0:h1, w0:w1])
                shapes.append(list(padded.shape) + [0] * (3 - padded.ndim))
                digests.append(V.digest(padded.astype(np.uint8)))
        out["shapes%d" % i] = np.array(shapes, dtype=np.int32).reshape(-1, 3)
        out["digests%d" % i] = np.array(digests, dtype="U64")
        print("%-30s box %s  padded %s" % (c["name"], out["box%d" % i].tolist(), [s for s in shapes]))
    np.savez_compressed(a.out, **out)
    print("wrote %s (%.1f KB)" % (a.out, os.path.getsize(a.out) / 1024))


if __name__ == "__main__":
    main()
