"""The loop around the hot path: the reference's `evaluate` (demonet/engine.py:70-110) with the forwards kept in flight.

The reference walks the data loader one batch at a time: images to the device, synchronize, `model(images)`, every output to the
host, `{image_id: output}` into the evaluator (engine.py:84-100). Here the same loop submits each batch to a
`pipeline.ForwardPipeline` and collects a batch's detections `depth` submissions later, so the device works on the next batches
while the host converts the previous ones: same `{image_id: {"boxes", "scores", "labels"}}` records (host tensors), same order.
The COCO evaluator itself (pycocotools, `data/coco_eval.py`) is third-party and absent here; `evalrec.coco_detection_records`
turns the records into the list `CocoEvaluator.prepare_for_coco_detection` builds (data/coco_eval.py:76-98) and
`evalrec.voc_mean_ap` scores them the PASCAL VOC way. `evaluate_voc` is the same loop with the scoring on the device: the detections stay
there and only the mAP comes back (demonet_amd/voceval.py). `evaluate_coco` is that loop with pycocotools' matching and its twelve numbers
(demonet_amd/cocoeval.py).
"""
import collections
import time
from typing import Dict, Iterable, List, Tuple

import torch

from .pipeline import ForwardPipeline


def _image_id(target):
    v = target["image_id"]
    return int(v.item()) if hasattr(v, "item") else int(v)


@torch.no_grad()
def evaluate(model, data_loader: Iterable, device="cuda:0", depth: int = 3) -> Tuple[Dict[int, Dict[str, torch.Tensor]], Dict[str, float]]:
    """data_loader yields (images, targets) as the reference's loaders do (engine.py:84): images = a list of [3,H,W] float tensors
    in [0,1] (or one [N,3,H,W] tensor), targets = a list of dicts holding "image_id". Batches whose images share one size go through
    the pipeline (any size: the device resizes to the network size and maps the boxes back, transform.py:27-53,278-292); a batch of
    mixed sizes is run by `model(images)` after the pipeline has drained, so the records keep the loader's order.
    Returns ({image_id: {"boxes" [n,4], "scores" [n], "labels" [n] int64}} on the host, {"images", "seconds", "images_per_sec",
    "model_seconds" (host time spent submitting and collecting)})."""
    device = torch.device(device)
    model.eval()
    results: Dict[int, Dict[str, torch.Tensor]] = collections.OrderedDict()
    pending = collections.deque()
    pipe = None
    shape = None
    n_images = 0
    model_time = 0.0

    def collect(ticket, ids):
        boxes, scores, labels, counts = pipe.result(ticket)
        host = [t.cpu() for t in (boxes, scores, labels, counts)]           # engine.py:92: outputs to the host
        for i, image_id in enumerate(ids):
            c = int(host[3][i])
            results[image_id] = {"boxes": host[0][i, :c].clone(), "scores": host[1][i, :c].clone(), "labels": host[2][i, :c].clone()}

    def drain():
        while pending:
            collect(*pending.popleft())

    t_start = time.perf_counter()
    for images, targets in data_loader:
        ids = [_image_id(t) for t in targets]
        same = isinstance(images, torch.Tensor) or len({tuple(im.shape) for im in images}) == 1
        t0 = time.perf_counter()
        if same:
            batch = images if isinstance(images, torch.Tensor) else torch.stack(list(images))
            batch = batch.to(device, non_blocking=True)
            if pipe is None or tuple(batch.shape) != shape:
                drain()
                if pipe is not None:
                    pipe.close()
                shape = tuple(batch.shape)
                pipe = ForwardPipeline(model, shape[0], height=shape[2], width=shape[3], depth=depth, device=device)
            if len(pending) == depth:                                       # its slot is about to be reused
                collect(*pending.popleft())
            pending.append((pipe.submit(batch), ids))
        else:
            drain()
            outputs = model([im.to(device) for im in images])              # engine.py:90
            for image_id, out in zip(ids, outputs):
                results[image_id] = {k: v.cpu() for k, v in out.items()}
        model_time += time.perf_counter() - t0
        n_images += len(ids)
    t0 = time.perf_counter()
    drain()
    if pipe is not None:
        pipe.close()
    model_time += time.perf_counter() - t0
    dt = time.perf_counter() - t_start
    return results, {"images": n_images, "seconds": dt, "images_per_sec": n_images / max(dt, 1e-9), "model_seconds": model_time}


def _evaluate_on_device(model, data_loader: Iterable, device, depth: int, acc) -> Tuple[int, float]:
    """`evaluate`'s loop with the detections left on the device: every batch goes to `acc.update(boxes, scores, labels, counts, targets)` on the
    current stream once its slot is about to be reused (`pipe.wait`: the current stream waits, the host does not), on the slot's own output
    tensors (`pipe.outputs`); the next submit on that slot orders itself behind the current stream. A batch of mixed sizes is run by
    `model(images)` after the pipeline has drained and padded to [n][detections_per_img]. Returns (images, model_seconds)."""
    model.eval()
    pending = collections.deque()
    pipe = None
    shape = None
    n_images = 0
    model_time = 0.0

    def collect(ticket, targets):
        pipe.wait(ticket)                                                   # the current stream waits; the host does not
        acc.update(*pipe.outputs(ticket), targets)

    def drain():
        while pending:
            collect(*pending.popleft())

    for images, targets in data_loader:
        same = isinstance(images, torch.Tensor) or len({tuple(im.shape) for im in images}) == 1
        t0 = time.perf_counter()
        if same:
            batch = images if isinstance(images, torch.Tensor) else torch.stack(list(images))
            batch = batch.to(device, non_blocking=True)
            if pipe is None or tuple(batch.shape) != shape:
                drain()
                if pipe is not None:
                    pipe.close()
                shape = tuple(batch.shape)
                pipe = ForwardPipeline(model, shape[0], height=shape[2], width=shape[3], depth=depth, device=device)
            if len(pending) == depth:                                       # its slot is about to be reused
                collect(*pending.popleft())
            pending.append((pipe.submit(batch), targets))
        else:
            drain()
            outputs = model([im.to(device) for im in images])
            n, D = len(outputs), model.detections_per_img
            boxes = torch.zeros((n, D, 4), dtype=torch.float32, device=device)
            scores = torch.zeros((n, D), dtype=torch.float32, device=device)
            labels = torch.zeros((n, D), dtype=torch.int64, device=device)
            lens = [int(o["scores"].shape[0]) for o in outputs]
            for i, (o, c) in enumerate(zip(outputs, lens)):
                boxes[i, :c], scores[i, :c], labels[i, :c] = o["boxes"], o["scores"], o["labels"]
            acc.update(boxes, scores, labels, torch.tensor(lens, dtype=torch.int32).to(device), targets)
        model_time += time.perf_counter() - t0
        n_images += len(targets)
    t0 = time.perf_counter()
    drain()
    if pipe is not None:
        pipe.close()
    model_time += time.perf_counter() - t0
    return n_images, model_time


@torch.no_grad()
def evaluate_voc(model, data_loader: Iterable, device="cuda:0", depth: int = 3, thresholds=(0.5,), use_07_metric: bool = False,
                 pixel_offset: float = 1.0) -> Tuple[dict, Dict[str, float]]:
    """PASCAL VOC mAP of `model` over `data_loader` with the detections left on the device. The loop is `evaluate`'s; the targets
    hold the reference's `boxes` [k, 4] xyxy, `labels` [k] and, optionally, `difficult` [k] (num_classes is the model's). A batch's detections
    never reach the host: once its slot is about to be reused, the current stream waits for the forward (`pipe.wait`) and
    `voceval.VocAccumulator.update` marks true and false positives there, on the slot's own output tensors (`pipe.outputs`), and keeps copies
    of scores, labels and flags on the device; the next submit on that slot orders itself behind the current stream. A batch of mixed sizes
    is run by `model(images)` after the pipeline has drained and padded to [n][detections_per_img]. Only `summarize` waits for the device.
    Returns (VocAccumulator.summarize(use_07_metric), stats) with the stats keys of `evaluate`; "seconds" includes the summary."""
    from .voceval import VocAccumulator
    device = torch.device(device)
    acc = VocAccumulator(model.graph.num_classes, thresholds, pixel_offset)
    t_start = time.perf_counter()
    n_images, model_time = _evaluate_on_device(model, data_loader, device, depth, acc)
    summary = acc.summarize(use_07_metric)
    dt = time.perf_counter() - t_start
    return summary, {"images": n_images, "seconds": dt, "images_per_sec": n_images / max(dt, 1e-9), "model_seconds": model_time}


@torch.no_grad()
def evaluate_coco(model, data_loader: Iterable, device="cuda:0", depth: int = 3, iou_thresholds=None, area_ranges=None,
                  max_dets=(1, 10, 100)) -> Tuple[dict, Dict[str, float]]:
    """The COCO numbers of `model` over `data_loader` with the detections left on the device: what the reference's `evaluate` gets
    from `CocoEvaluator` (data/coco_eval.py:23-64) and pycocotools. The loop is `evaluate_voc`'s; the targets hold the reference's `boxes`
    [k, 4] xyxy, `labels` [k] and, optionally, `iscrowd` [k] and `area` [k] (num_classes is the model's; the loader's order stands in for
    ascending image ids). `cocoeval.CocoAccumulator.update` matches every batch on the device and keeps scores, labels, flags and ranks
    there; only `summarize` waits for the device. Returns (CocoAccumulator.summarize() = {"stats": the twelve numbers, "precision", "recall"},
    stats) with the stats keys of `evaluate`; "seconds" includes the summary, "summarize_seconds" is the summary alone."""
    from . import cocoeval
    device = torch.device(device)
    acc = cocoeval.CocoAccumulator(model.graph.num_classes, cocoeval.IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds,
                                   cocoeval.AREA_RANGES if area_ranges is None else area_ranges, max_dets)
    t_start = time.perf_counter()
    n_images, model_time = _evaluate_on_device(model, data_loader, device, depth, acc)
    t0 = time.perf_counter()
    summary = acc.summarize()
    t1 = time.perf_counter()
    dt = t1 - t_start
    return summary, {"images": n_images, "seconds": dt, "images_per_sec": n_images / max(dt, 1e-9), "model_seconds": model_time,
                     "summarize_seconds": t1 - t0}


def coco_records(results: Dict[int, Dict[str, torch.Tensor]]) -> List[dict]:
    """The list `CocoEvaluator.prepare_for_coco_detection` builds from such a dict (data/coco_eval.py:76-98; xyxy -> xywh :162-164)."""
    out = []
    for image_id, pred in results.items():
        if len(pred["boxes"]) == 0:                                         # coco_eval.py:79-80
            continue
        b = pred["boxes"]
        xywh = torch.stack((b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), dim=1).tolist()
        scores, labels = pred["scores"].tolist(), pred["labels"].tolist()
        out.extend({"image_id": image_id, "category_id": labels[k], "bbox": xywh[k], "score": scores[k]} for k in range(len(xywh)))
    return out
