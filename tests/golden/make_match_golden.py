"""Authoring-time generator of tests/golden/ssd_match_ties.npz: ground-truth boxes that sit on ties of the anchor matching, and the
matched indices / losses the REAL reference computes for them -- `proposal_matcher(box_iou(boxes, anchors))` (SSDMatcher,
_utils.py:264-294,348-362, as SSD.forward calls it at generalized_ssd.py:316-330) and `SSD.compute_loss` (:210-269) of a reference
`ssdlite320_mobilenet_v3_large` instance; matcher and loss do not depend on the network, so the same instance serves the default boxes
of all four models, which are the reference DefaultBoxGenerator outputs pinned under "anchors" in tests/golden/<model>.npz.
torchvision's box_iou comes from oracle/ref_shim. Needs the reference checkout (oracle/run_reference.py); tests never import or run
this file, the .npz is the committed fixture and carries everything they need.

One batch of 4 images per model: a full image of 256 boxes (the matcher kernel's capacity) that mixes the families below, an image
without boxes, an image with one box, and a mixed image of 64 boxes. Every box carries the code of its family:
  0 copy       an exact copy of an anchor
  1 half       an anchor's centre and width with half its height, or the transpose: IoU 0.5 in real arithmetic with that anchor --
               the threshold -- and equal IoU with the anchors that share its centre
  2 midpoint   the arithmetic midpoint of two neighbouring anchors of one level and shape: both tie for the box's best
  3 duplicate  a box of this image listed again (twice or three times in all): argmax over the gts takes the first, the
               "every gt keeps its best anchor" pass lets the last one win
  4 pixel      integer-pixel and half-pixel corners
  5 shared     an anchor and two shrunk copies of it: three boxes with the same best anchor
The boxes of family 1, 2 and 4 are drawn from seeded candidates; half of each quota prefers candidates on which rounding the IoU's
union once (a fused multiply-add) instead of operation by operation changes the match of that box alone (the emulation of
tests/test_loss_match.py), so that a kernel with that rounding cannot pass. The condition itself is asserted by the tests."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODELS = {"ssdlite320_mobilenet_v3_large": 320, "ssd_lite_mobilenet_v2": 320, "ssd300_vgg16": 300, "ssd512_vgg16": 512}
K = 21
COPY, HALF, MIDPOINT, DUPLICATE, PIXEL, SHARED = range(6)
# boxes per family: (copy, half, midpoint, pixel, shared groups of 3, duplicate listings)
FULL = (30, 90, 40, 50, 6, 28)          # 30 + 90 + 40 + 50 + 18 + 28 = 256
MIXED = (8, 24, 10, 12, 2, 4)           # 8 + 24 + 10 + 12 + 6 + 4 = 64


def _sensitive(boxes, anchors):
    """per box: does the single-rounding union change which anchors this box alone is matched to"""
    from test_loss_match import emulate_iou
    out = np.zeros(len(boxes), bool)
    for i in range(0, len(boxes), 128):
        sets = []
        for fused in (False, True):
            q = emulate_iou(boxes[i:i + 128], anchors, fused)
            m = q >= np.float32(0.5)
            m[np.arange(q.shape[0]), q.argmax(1)] = True
            sets.append(m)
        out[i:i + 128] = (sets[0] != sets[1]).any(1)
    return out


def _pick(cand, sens, k):
    """k of the candidates: the sensitive ones first for half the quota, then in draw order; and which of the k are sensitive"""
    first = list(np.where(sens)[0][:k // 2])
    rest = [i for i in range(len(cand)) if i not in set(first)][:k - len(first)]
    idx = np.array(first + rest, dtype=np.int64)
    return cand[idx], sens[idx]


def _half(anchors, idx, transpose):
    a = anchors[idx]
    w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    cx, cy = a[:, 0] + np.float32(0.5) * w, a[:, 1] + np.float32(0.5) * h
    b = a.copy()
    q = np.float32(0.25)
    b[transpose, 0], b[transpose, 2] = (cx - q * w)[transpose], (cx + q * w)[transpose]
    b[~transpose, 1], b[~transpose, 3] = (cy - q * h)[~transpose], (cy + q * h)[~transpose]
    return b


def _midpoints(anchors, idx):
    w, h = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    cx, cy = anchors[:, 0] + anchors[:, 2], anchors[:, 1] + anchors[:, 3]
    out = []
    for i in idx:
        same = (np.abs(w - w[i]) < 1e-3) & (np.abs(h - h[i]) < 1e-3)
        d = np.abs(cx - cx[i]) + np.abs(cy - cy[i])
        d[~same | (d < 1e-3)] = np.inf
        out.append(np.float32(0.5) * (anchors[i] + anchors[int(d.argmin())]))
    return np.stack(out).astype(np.float32)


def _pixels(rng, n, size):
    xy = rng.randint(0, size - 16, (n, 2))
    wh = rng.randint(8, size // 2, (n, 2))
    b = np.concatenate([xy, np.minimum(xy + wh, size)], 1).astype(np.float32)
    halfpix = rng.randint(0, 2, n).astype(bool)
    b[halfpix] += rng.randint(0, 2, (int(halfpix.sum()), 4)).astype(np.float32) * np.float32(0.5)
    return b


def _image(rng, anchors, size, quota):
    n_copy, n_half, n_mid, n_pix, n_shared, n_dup = quota
    A = anchors.shape[0]
    boxes = [anchors[rng.choice(A, n_copy, replace=False)]]
    fam = [COPY] * n_copy
    sens = [np.zeros(n_copy, bool)]
    for family, k, cand in ((HALF, n_half, _half(anchors, rng.choice(A, 12 * n_half, replace=False), rng.randint(0, 2, 12 * n_half).astype(bool))),
                            (MIDPOINT, n_mid, _midpoints(anchors, rng.choice(A, 8 * n_mid, replace=False))),
                            (PIXEL, n_pix, _pixels(rng, 40 * n_pix, size))):
        b, s = _pick(cand, _sensitive(cand, anchors), k)
        boxes.append(b)
        sens.append(s)
        fam += [family] * k
    from test_loss_match import emulate_iou
    groups = 0
    for a0 in anchors[rng.choice(A, 8 * n_shared, replace=False)]:
        w, h = a0[2] - a0[0], a0[3] - a0[1]
        group = np.stack([a0 + np.array([f * w, f * h, -f * w, -f * h], np.float32) for f in (0.0, 1.0 / 32, 1.0 / 16)]).astype(np.float32)
        if groups < n_shared and len(set(emulate_iou(group, anchors, False).argmax(1).tolist())) == 1:         # one best anchor for all three
            boxes.append(group)
            fam += [SHARED] * 3
            groups += 1
    assert groups == n_shared
    boxes = np.concatenate(boxes).astype(np.float32)
    sens = np.where(np.concatenate(sens))[0]                         # duplicates of the sensitive boxes while there are any,
    rest = np.setdiff1d(np.arange(len(boxes)), sens)                 # half of them listed three times
    src = np.concatenate([rng.permutation(sens), rng.permutation(rest)])[:n_dup // 2]
    dup = np.concatenate([src, src[:n_dup - len(src)]])
    boxes = np.concatenate([boxes, boxes[dup]])
    fam = np.array(fam + [DUPLICATE] * n_dup, np.int8)
    order = rng.permutation(len(boxes))
    return boxes[order], fam[order]


def make_images(name, anchors):
    rng = np.random.RandomState(20260000 + sum(map(ord, name)))
    full = _image(rng, anchors, MODELS[name], FULL)
    mixed = _image(rng, anchors, MODELS[name], MIXED)
    one = _half(anchors, rng.choice(anchors.shape[0], 1), np.array([False]))
    return [full, (np.zeros((0, 4), np.float32), np.zeros((0,), np.int8)), (one, np.array([HALF], np.int8)), mixed]


def main():
    import run_reference as rr
    rr.import_reference_models()
    from torchvision.ops import boxes as box_ops          # the shim
    ref = rr.build_reference_model("ssdlite320_mobilenet_v3_large", K)
    out = {"iou_thresh": np.float32(0.5), "neg_to_pos_ratio": np.float32(ref.neg_to_pos_ratio), "num_classes": np.int64(K),
           "models": np.array(list(MODELS))}
    for mi, name in enumerate(MODELS):
        anchors_np = np.load(os.path.join(HERE, name + ".npz"))["anchors"].astype(np.float32)
        anchors = torch.from_numpy(anchors_np)
        A = anchors.shape[0]
        images = make_images(name, anchors_np)
        n = len(images)
        rng = np.random.RandomState(77 + mi)
        targets, matched = [], []
        for boxes, fam in images:
            assert (boxes[:, 2:] > boxes[:, :2]).all()
            t = {"boxes": torch.from_numpy(boxes), "labels": torch.from_numpy(rng.randint(1, K, (len(boxes),)).astype(np.int64))}
            targets.append(t)
            if len(boxes) == 0:
                matched.append(torch.full((A,), -1, dtype=torch.int64))
                continue
            q = box_ops.box_iou(t["boxes"], anchors)
            matched.append(ref.proposal_matcher(q))
            best = q.argmax(1)
            for a0 in set(best[torch.from_numpy(fam == SHARED)].tolist()):          # family 5: three boxes per best anchor
                assert int(((best == a0) & torch.from_numpy(fam == SHARED)).sum()) >= 3, name
        seed = 900 + mi
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(n, A, K, generator=g) * 2.0
        reg = torch.randn(n, A, 4, generator=g)
        losses = ref.compute_loss(targets, {"cls_logits": logits, "bbox_regression": reg}, [anchors] * n, matched)
        gmax = max(len(b) for b, _ in images)
        gb, gl, gf = np.zeros((n, gmax, 4), np.float32), np.zeros((n, gmax), np.int64), np.full((n, gmax), -1, np.int8)
        for i, (boxes, fam) in enumerate(images):
            gb[i, :len(boxes)], gl[i, :len(boxes)], gf[i, :len(boxes)] = boxes, targets[i]["labels"].numpy(), fam
        m = torch.stack(matched).numpy()
        assert m.max() < 2 ** 15
        out[f"{name}_gt_boxes"], out[f"{name}_gt_labels"], out[f"{name}_family"] = gb, gl, gf
        out[f"{name}_gt_counts"] = np.array([len(b) for b, _ in images], np.int32)
        out[f"{name}_logits_seed"] = np.int64(seed)
        out[f"{name}_matched"] = m.astype(np.int16)
        out[f"{name}_bbox_regression"] = np.float32(losses["bbox_regression"].item())
        out[f"{name}_classification"] = np.float32(losses["classification"].item())
        print(f"{name}: A={A} boxes {[len(b) for b, _ in images]} matched anchors {[int((x >= 0).sum()) for x in matched]} "
              f"bbox {losses['bbox_regression'].item():.6f} cls {losses['classification'].item():.6f}")
    path = os.path.join(HERE, "ssd_match_ties.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
