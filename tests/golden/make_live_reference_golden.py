"""Generates tests/golden/live_reference_ssdlite320.npz: what the REAL reference (via oracle/run_reference.py, on CPU in the
authoring container) returns for the case of tests/test_oracle.py::test_oracle_matches_live_reference, so that the test needs
nothing outside the repository.

    python tests/golden/make_live_reference_golden.py

Case: ssdlite320_mobilenet_v3_large, 91 classes, synthetic weights seed 2 (demonet_amd/synth.py), one synthetic image seed 1013.
Stored: the reference model's state_dict key names, and the detections of that image (labels int64, scores / boxes float32).
Nothing from the reference's source is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from demonet_amd import spec, synth  # noqa: E402
import run_reference as rr  # noqa: E402

NAME, NCLS, WSEED, ISEED = "ssdlite320_mobilenet_v3_large", 91, 2, 1013


def main():
    g = spec.GRAPHS[NAME](num_classes=NCLS)
    ref = rr.build_reference_model(NAME, NCLS, synth.state_dict(g, WSEED))
    W, H = g.size
    imgs = [torch.from_numpy(synth.images(ISEED, 1, H, W)[0])]
    with torch.no_grad():
        rd = ref(imgs)
    out = os.path.join(HERE, "live_reference_ssdlite320.npz")
    np.savez_compressed(out, keys=np.array(sorted(ref.state_dict().keys())), labels=rd[0]["labels"].numpy().astype(np.int64),
                        scores=rd[0]["scores"].numpy().astype(np.float32), boxes=rd[0]["boxes"].numpy().astype(np.float32),
                        case=np.array([WSEED, ISEED, NCLS], np.int64))
    print(out, len(rd[0]["labels"]), "detections")


if __name__ == "__main__":
    main()
